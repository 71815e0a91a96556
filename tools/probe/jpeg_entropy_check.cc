// Stand-alone memory-safety check of csrc/jpeg_entropy.cc: built WITH it by the host compiler under
// -fsanitize=address,undefined and run as an ordinary program (tests/test_jpeg_host.py does both).
//
//   jpeg_entropy_check file.jpg [file.jpg ...]
//
// For every file the decoder is fed every truncation length, 2000 seeded single-byte corruptions anywhere and 2000 inside
// the Huffman and quantisation table segments.  Input and output live in heap blocks of EXACTLY n and out_cap bytes, so a
// read or write one byte outside them is a sanitizer report.  Every call must return a record or a status.  Exit 0 = clean.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/gitmi_jpeg.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

static long g_calls = 0, g_ok = 0, g_unsupported = 0;

// one call on an exact-size copy of `src`; returns the status
static int run(const uint8_t* src, size_t n, size_t out_cap) {
    uint8_t* in = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(in, src, n);
    uint8_t* out = (uint8_t*)malloc(out_cap ? out_cap : 1);
    gitmi_jpeg_info info;
    const int rc = gitmi_jpeg_entropy_decode(n ? in : nullptr, n, out_cap ? out : nullptr, out_cap, &info);
    ++g_calls;
    if (rc == GITMI_JPEG_OK) {
        ++g_ok;
        gitmi_jpeg_header h;
        memcpy(&h, out, sizeof(h));
        if (h.magic != GITMI_JPEG_MAGIC || h.record_bytes > out_cap || h.record_bytes != info.record_bytes) {
            fprintf(stderr, "a record that does not describe itself\n");
            exit(3);
        }
    } else if (rc == GITMI_JPEG_UNSUPPORTED) {
        ++g_unsupported;
    } else if (rc != GITMI_JPEG_NO_SPACE) {
        fprintf(stderr, "unexpected status %d\n", rc);
        exit(3);
    }
    free(in);
    free(out);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> d;
        uint8_t chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) d.insert(d.end(), chunk, chunk + got);
        fclose(f);
        const size_t n = d.size();
        g_state = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;

        gitmi_jpeg_info info;
        if (gitmi_jpeg_entropy_decode(d.data(), n, nullptr, 0, &info) != GITMI_JPEG_NO_SPACE) {
            fprintf(stderr, "%s: not a JPEG of the fast path\n", argv[a]);
            return 3;
        }
        const size_t cap = (size_t)info.record_bytes;
        if (run(d.data(), n, cap) != GITMI_JPEG_OK) { fprintf(stderr, "%s: the clean file does not decode\n", argv[a]); return 3; }
        if (run(d.data(), n, cap - 1) != GITMI_JPEG_NO_SPACE) { fprintf(stderr, "%s: one byte short is not NO_SPACE\n", argv[a]); return 3; }

        // the table segments (DQT = DB, DHT = C4) in front of the scan
        std::vector<size_t> table_bytes;
        for (size_t p = 2; p + 4 <= n && d[p] == 0xFF;) {
            const unsigned m = d[p + 1];
            const size_t len = ((size_t)d[p + 2] << 8) | d[p + 3];
            if (m == 0xDB || m == 0xC4)
                for (size_t i = p + 4; i < p + 2 + len && i < n; ++i) table_bytes.push_back(i);
            if (m == 0xDA) break;
            p += 2 + len;
        }
        if (table_bytes.empty()) { fprintf(stderr, "%s: no table segments found\n", argv[a]); return 3; }

        for (size_t len = 0; len < n; ++len)                          // every truncation: never a record
            if (run(d.data(), len, cap) == GITMI_JPEG_OK) { fprintf(stderr, "%s: a record from %zu of %zu bytes\n", argv[a], len, n); return 3; }
        std::vector<uint8_t> m(d);
        for (int i = 0; i < 2000; ++i) {                              // single-byte corruptions anywhere
            const size_t at = rnd() % n;
            const uint8_t old = m[at];
            m[at] = (uint8_t)rnd();
            run(m.data(), n, cap);
            m[at] = old;
        }
        for (int i = 0; i < 2000; ++i) {                              // ... and inside the tables
            const size_t at = table_bytes[rnd() % table_bytes.size()];
            const uint8_t old = m[at];
            m[at] = (uint8_t)rnd();
            run(m.data(), n, cap);
            m[at] = old;
        }
    }
    printf("jpeg_entropy_check: %ld calls, %ld records, %ld unsupported, no report\n", g_calls, g_ok, g_unsupported);
    return 0;
}
