// Stand-alone check of the GPU Huffman decode ON THE HOST: csrc/jpeg_entropy_dev.h holds the per-thread bodies of
// kernels_jpeg_entropy.hip as plain functions; this program runs them thread by thread (sync rounds, write pass, DC pass)
// beside csrc/jpeg_entropy.cc, built as ONE ordinary program under -fsanitize=address,undefined
// (tests/test_jpeg_scan_host.py does both).
//
//   jpeg_entropy_gpu_check emulate [--list K] [--part I/N] file.jpg ...
//       per file: the file itself, every truncation of its scan (re-terminated with an EOI) and 2 x 2000 seeded single-byte
//       corruptions of the scan.  --part I/N: the work of a long scan on N processes -- this one takes the cut points and
//       the corruptions whose index is I modulo N; the N parts together are the whole set.
//       For each input gitmi_jpeg_scan_prepare writes a scan record into a heap block of EXACTLY its size, the emulation
//       decodes it into a block of exactly the coefficient record's size with a workspace of exactly the size the library
//       asks for; its verdict must be OK exactly when gitmi_jpeg_entropy_decode returns OK on the same
//       bytes, and the record then byte-equal.  --list K prints the first K truncations (evenly spread) and corruptions as
//       "case <file index> <kind> <offset> <value> <host status>": the inputs tests/test_gpu_jpeg_entropy.py sends to the GPU.
//   jpeg_entropy_gpu_check prepare file.jpg ...
//       gitmi_jpeg_scan_prepare on every truncation of the FILE and 2 x 2000 corruptions anywhere / inside the tables.
//   jpeg_entropy_gpu_check decode in.scan out.coef
//       one scan record (a file) through the emulation; writes the coefficient record; exit 0 when the status is 0.
// Exit 0 = clean.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../generativeimage2text_amd/csrc/jpeg_entropy_dev.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

static long g_inputs = 0, g_prepared = 0, g_ok = 0, g_rejected = 0, g_max_rounds = 0, g_max_sub = 0;

// the four kernels of kernels_jpeg_entropy.hip for one image, thread by thread; -> status, *rounds
static int emulate(const uint8_t* rec, size_t rec_bytes, uint8_t* coef, size_t coef_size, long* rounds) {
    const uint64_t cap = jd_nsub_bound(rec_bytes);
    JdCtx* x = (JdCtx*)malloc(sizeof(JdCtx));
    uint8_t* tmp = (uint8_t*)malloc((size_t)jd_workspace_bytes(cap));
    int status = 0;
    *rounds = 0;
    jd_setup(x, rec, rec_bytes, coef_size, cap);
    if (!x->ok) { free(tmp); free(x); return JD_ST_RECORD; }
    for (int tid = 0; tid < JD_THREADS; ++tid) jd_setup_tables(x, rec, tid, JD_THREADS);
    const JdWork w = jd_work(tmp, cap);
    w.flags[0] = 0;
    memcpy(coef, rec, GITMI_JPEG_HEADER_BYTES);                        // zero kernel
    memset(coef + GITMI_JPEG_HEADER_BYTES, 0, coef_size - GITMI_JPEG_HEADER_BYTES);
    const uint32_t* words = (const uint32_t*)(rec + JD_SCAN_AT);
    const uint32_t nsub = x->nsub;
    for (int tid = 0; tid < JD_THREADS; ++tid)                        // sync kernel, round 0
        for (uint32_t i = (uint32_t)tid; i < nsub; i += JD_THREADS) {
            const jd_state in = jd_pack(i * (uint32_t)JD_SUB_BITS, 0, 0);
            uint32_t n;
            w.in[i] = in;
            w.exit[i] = jd_walk(*x, words, i, in, &n);
            w.count[i] = n;
        }
    // every thread of a round reads the exit states as the round before left them: the slowest propagation the GPU can show
    // (there a thread may also see a neighbour's store of the same round), so the round loop runs as often as it ever will
    bool fixed = false;
    std::vector<jd_state> before(nsub);
    for (uint32_t round = 0; round <= nsub && !fixed; ++round) {
        int changed = 0;
        for (uint32_t i = 0; i < nsub; ++i) before[i] = w.exit[i];
        for (int tid = 0; tid < JD_THREADS; ++tid)
            for (uint32_t i = (uint32_t)tid; i < nsub; i += JD_THREADS) {
                if (i == 0) continue;
                const jd_state in = before[i - 1];
                if (in == w.in[i]) continue;
                uint32_t n;
                w.in[i] = in;
                w.exit[i] = jd_walk(*x, words, i, in, &n);
                w.count[i] = n;
                changed = 1;
            }
        fixed = !changed;
        *rounds = (long)round + 1;
    }
    if (!fixed) status |= JD_ST_ROUNDS;
    w.flags[1] = (uint32_t)*rounds;
    uint32_t carry = 0;
    for (uint32_t i = 0; i < nsub; ++i) { w.first[i] = carry; carry += w.count[i]; }
    for (uint32_t i = 0; i < nsub; ++i) {                             // write kernel
        bool last;
        status |= jd_write(*x, words, i, w.in[i], w.first[i], coef, &last);
        if (last) w.flags[0] = 1;
    }
    if (!w.flags[0]) status |= JD_ST_SHORT;                           // dc kernel
    for (int c = 0; c < (int)x->ncomp; ++c) {
        jd_setup_dc_limit(x, rec, c);
        int pred = 0;
        for (uint32_t j = 0; j < x->nblk[c]; ++j) {
            pred += jd_dc_load(*x, c, j, coef);
            status |= jd_dc_store(*x, c, j, pred, coef);
        }
    }
    if ((long)nsub > g_max_sub) g_max_sub = (long)nsub;
    free(tmp);
    free(x);
    return status;
}

// one input through prepare + emulation + the host decoder, all in exact-size heap blocks; -> the host decoder's status
static int check(const uint8_t* src, size_t n, const char* what) {
    ++g_inputs;
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    memcpy(in, src, n);
    gitmi_jpeg_info info, info2;
    uint64_t sbytes = 0;
    int host = gitmi_jpeg_entropy_decode(in, n, nullptr, 0, &info);
    uint8_t* ref = nullptr;
    if (host == GITMI_JPEG_NO_SPACE) {
        ref = (uint8_t*)malloc((size_t)info.record_bytes);
        host = gitmi_jpeg_entropy_decode(in, n, ref, (size_t)info.record_bytes, &info);
    }
    int rc = gitmi_jpeg_scan_prepare(in, n, nullptr, 0, &info2, &sbytes);
    if (rc == GITMI_JPEG_NO_SPACE) {
        ++g_prepared;
        if (!ref || info2.record_bytes != info.record_bytes) { fprintf(stderr, "%s: prepare takes what the host parse declines\n", what); exit(3); }
        uint8_t* rec = (uint8_t*)malloc((size_t)sbytes);
        rc = gitmi_jpeg_scan_prepare(in, n, rec, (size_t)sbytes, &info2, &sbytes);
        if (rc != GITMI_JPEG_OK) { fprintf(stderr, "%s: prepare: %d after NO_SPACE\n", what, rc); exit(3); }
        uint8_t* coef = (uint8_t*)malloc((size_t)info2.record_bytes);
        long rounds;
        const int st = emulate(rec, (size_t)sbytes, coef, (size_t)info2.record_bytes, &rounds);
        if (rounds > g_max_rounds) g_max_rounds = rounds;
        if ((st == 0) != (host == GITMI_JPEG_OK)) { fprintf(stderr, "%s: verdict %d, host decoder %d\n", what, st, host); exit(3); }
        if (st == 0) {
            ++g_ok;
            if (memcmp(coef, ref, (size_t)info.record_bytes)) { fprintf(stderr, "%s: the records differ\n", what); exit(3); }
        } else {
            ++g_rejected;
        }
        free(coef);
        free(rec);
    } else if (rc != GITMI_JPEG_UNSUPPORTED) {
        fprintf(stderr, "%s: prepare: unexpected status %d\n", what, rc);
        exit(3);
    }
    free(ref);
    free(in);
    return host;
}

// prepare alone on an exact-size copy; -> status
static int prepare_only(const uint8_t* src, size_t n, size_t cap) {
    ++g_inputs;
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, src, n);
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    gitmi_jpeg_info info;
    uint64_t sbytes = 0;
    const int rc = gitmi_jpeg_scan_prepare(n ? in : nullptr, n, cap ? out : nullptr, cap, &info, &sbytes);
    if (rc == GITMI_JPEG_OK) {
        ++g_ok;
        gitmi_jpeg_scan sc;
        memcpy(&sc, out + GITMI_JPEG_HEADER_BYTES, sizeof(sc));
        if (sc.magic != GITMI_JPEG_SCAN_MAGIC || sc.scan_record_bytes != sbytes || sbytes > cap ||
            sc.scan_offset + sc.scan_bytes + 8 > sbytes) { fprintf(stderr, "a scan record that does not describe itself\n"); exit(3); }
    } else if (rc != GITMI_JPEG_UNSUPPORTED && rc != GITMI_JPEG_NO_SPACE) {
        fprintf(stderr, "unexpected status %d\n", rc);
        exit(3);
    }
    free(in);
    free(out);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s emulate|prepare [--list K] file.jpg ...\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "decode")) {
        if (argc != 4) { fprintf(stderr, "usage: %s decode in.scan out.coef\n", argv[0]); return 2; }
        FILE* f = fopen(argv[2], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        std::vector<uint8_t> d;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) d.insert(d.end(), chunk, chunk + got);
        fclose(f);
        if (d.size() < GITMI_JPEG_HEADER_BYTES) { fprintf(stderr, "%s: no scan record\n", argv[2]); return 3; }
        uint8_t* rec = (uint8_t*)malloc(d.size());
        memcpy(rec, d.data(), d.size());
        gitmi_jpeg_header h;
        memcpy(&h, rec, sizeof(h));
        if (h.record_bytes < GITMI_JPEG_HEADER_BYTES || h.record_bytes > ((uint64_t)1 << 32)) { fprintf(stderr, "%s: no scan record\n", argv[2]); return 3; }
        uint8_t* coef = (uint8_t*)malloc((size_t)h.record_bytes);
        long rounds;
        const int st = emulate(rec, d.size(), coef, (size_t)h.record_bytes, &rounds);
        printf("jpeg_entropy_gpu_check decode: status %d, %ld rounds\n", st, rounds);
        if (st == 0) {
            FILE* o = fopen(argv[3], "wb");
            if (!o || fwrite(coef, 1, (size_t)h.record_bytes, o) != (size_t)h.record_bytes) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
            fclose(o);
        }
        free(coef);
        free(rec);
        return st == 0 ? 0 : 4;
    }
    const bool emu = !strcmp(argv[1], "emulate");
    int a = 2, list = 0, part = 0, parts = 1;
    if (a + 1 < argc && !strcmp(argv[a], "--list")) { list = atoi(argv[a + 1]); a += 2; }
    if (a + 1 < argc && !strcmp(argv[a], "--part")) {
        if (sscanf(argv[a + 1], "%d/%d", &part, &parts) != 2 || parts < 1 || part < 0 || part >= parts) { fprintf(stderr, "--part I/N\n"); return 2; }
        a += 2;
    }
    for (int fi = 0; a < argc; ++a, ++fi) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> d;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) d.insert(d.end(), chunk, chunk + got);
        fclose(f);
        const size_t n = d.size();
        // the table segments and the scan: behind the SOS segment, in front of the EOI that ends the file
        std::vector<size_t> table_bytes;
        size_t scan0 = 0;
        for (size_t p = 2; p + 4 <= n && d[p] == 0xFF;) {
            const unsigned m = d[p + 1];
            const size_t len = ((size_t)d[p + 2] << 8) | d[p + 3];
            if (m == 0xDB || m == 0xC4)
                for (size_t i = p + 4; i < p + 2 + len && i < n; ++i) table_bytes.push_back(i);
            p += 2 + len;
            if (m == 0xDA) { scan0 = p; break; }
        }
        if (!scan0 || n < scan0 + 2 || d[n - 2] != 0xFF || d[n - 1] != 0xD9 || table_bytes.empty()) {
            fprintf(stderr, "%s: no scan that runs to an EOI at the end of the file\n", argv[a]);
            return 3;
        }
        const size_t scan_len = n - 2 - scan0;
        g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
        if (emu) {
            if (check(d.data(), n, argv[a]) != GITMI_JPEG_OK) { fprintf(stderr, "%s: the clean file does not decode\n", argv[a]); return 3; }
            std::vector<uint8_t> t;
            for (size_t len = 0; len < scan_len; ++len) {             // every truncation of the scan, EOI put back
                if (len % (size_t)parts != (size_t)part) continue;
                t.assign(d.begin(), d.begin() + (long)(scan0 + len));
                t.push_back(0xFF); t.push_back(0xD9);
                const int host = check(t.data(), t.size(), argv[a]);
                const size_t step = scan_len / (size_t)(list > 0 ? list : 1) + 1;
                if (list && len % step == step / 2) printf("case %d cut %zu 0 %d\n", fi, len, host);
            }
            std::vector<uint8_t> m(d);
            for (int i = 0; i < 4000; ++i) {                          // 2 x 2000 single-byte corruptions of the scan
                const size_t at = scan0 + rnd() % scan_len;
                const uint8_t to = (uint8_t)rnd();
                if (i % parts != part) continue;
                const uint8_t old = m[at];
                m[at] = to;
                const int host = check(m.data(), n, argv[a]);
                if (i < list) printf("case %d byte %zu %u %d\n", fi, at, (unsigned)m[at], host);
                m[at] = old;
            }
        } else {
            gitmi_jpeg_info info;
            uint64_t sbytes = 0;
            if (gitmi_jpeg_scan_prepare(d.data(), n, nullptr, 0, &info, &sbytes) != GITMI_JPEG_NO_SPACE) {
                fprintf(stderr, "%s: not a JPEG prepare takes\n", argv[a]);
                return 3;
            }
            const size_t cap = (size_t)sbytes;
            if (prepare_only(d.data(), n, cap) != GITMI_JPEG_OK) { fprintf(stderr, "%s: the clean file is not prepared\n", argv[a]); return 3; }
            if (prepare_only(d.data(), n, cap - 1) != GITMI_JPEG_NO_SPACE) { fprintf(stderr, "%s: one byte short is not NO_SPACE\n", argv[a]); return 3; }
            for (size_t len = 0; len < n; ++len)                      // every truncation: no EOI, never a record
                if (prepare_only(d.data(), len, cap) == GITMI_JPEG_OK) { fprintf(stderr, "%s: a scan record from %zu of %zu bytes\n", argv[a], len, n); return 3; }
            std::vector<uint8_t> m(d);
            for (int i = 0; i < 4000; ++i) {
                const size_t at = i < 2000 ? rnd() % n : table_bytes[rnd() % table_bytes.size()];
                const uint8_t old = m[at];
                m[at] = (uint8_t)rnd();
                prepare_only(m.data(), n, cap + 4096);                // a corrupted FF 00 makes the scan a byte longer
                m[at] = old;
            }
        }
    }
    printf("jpeg_entropy_gpu_check %s: %ld inputs, %ld prepared, %ld records, %ld rejected, at most %ld subsequences and %ld rounds, no report\n",
           argv[1], g_inputs, g_prepared, g_ok, g_rejected, g_max_sub, g_max_rounds);
    return 0;
}
