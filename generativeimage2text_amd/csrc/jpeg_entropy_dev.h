// The per-thread bodies of the GPU Huffman decode (include/gitmi_jpeg.h: gitmi_jpeg_entropy_batch), as plain functions that
// kernels_jpeg_entropy.hip runs on the GPU and tools/probe/jpeg_entropy_gpu_check.cc runs thread by thread on the host under
// the sanitizers: validation of a scan record, the look-ahead tables, one symbol, the walk of one subsequence (sync rounds),
// the write pass of one subsequence, one step of the DC pass.
//
// The scan of a baseline JPEG is cut into subsequences of JD_SUB_BITS bits.  Decoder state at a symbol boundary is
// (bit position, block index within the MCU, zig-zag position k).  The walk of subsequence i is a TOTAL function f_i of its
// input state: where the host decoder (jpeg_entropy.cc) would decline -- no such code, k > 63, an EOBn, a DC size > 11, an AC
// size > 10, a read past the last scan bit -- the walk skips one bit, restarts at (block 0, k 0) and goes on.  So "decode
// subsequence i from the exit state of i - 1" is defined on any bytes, and its fixpoint with exit[-1] = (0, 0, 0) is the
// sequential decode by induction over i.  An absorbing error state instead would be as exact but would never let a decoder
// that started in the wrong place fall into step: with the wrong block index it reads luma with the chroma tables and runs
// into an invalid code within a few blocks (measured: as many rounds as subsequences).  The ANOMALY itself is judged in the
// write pass, which walks every subsequence from its true state: the first place where the walk would have to skip, in
// front of the image's last block, is where the host decoder returns GITMI_JPEG_UNSUPPORTED.
//
// Nothing here trusts the record: every offset is checked before it is used, every loop is bounded by the subsequence's bit
// length or the block count, every store by the block total.
#pragma once
#include <stdint.h>

#include "../../include/gitmi_jpeg.h"

#if defined(__HIPCC__)
#define JD_FN __host__ __device__ __forceinline__
#else
#define JD_FN inline
#endif

constexpr int JD_SUB_BITS = 1024;                   // bits per subsequence (a multiple of 32)
constexpr int JD_THREADS = 256;                     // threads of a workgroup
constexpr int JD_LOOK = 9;                          // look-ahead bits, as on the host
constexpr int JD_COEF_LIMIT = 2047;                 // jpeg_entropy.cc: kCoefLimit
constexpr uint64_t JD_SCAN_AT = GITMI_JPEG_HEADER_BYTES + GITMI_JPEG_SCAN_BYTES;

typedef unsigned long long jd_state;                // (pos << 16) | (block in MCU << 8) | k
constexpr jd_state JD_NO_STATE = ~0ull;             // never an exit state
JD_FN jd_state jd_pack(uint32_t pos, int b, int k) { return ((jd_state)pos << 16) | ((jd_state)b << 8) | (jd_state)k; }

// status bits of an image
constexpr int JD_ST_RECORD = 1;                     // the scan record or the caller's sizes do not check out: nothing else is written
constexpr int JD_ST_STREAM = 2;                     // an anomaly of the Huffman data in front of the last block
constexpr int JD_ST_LIMIT = 4;                      // a coefficient beyond 2047 / q
constexpr int JD_ST_TAIL = 8;                       // a whole byte or more behind the last block
constexpr int JD_ST_SHORT = 16;                     // the scan ends in front of the last block
constexpr int JD_ST_ROUNDS = 32;                    // no fixpoint within nsub + 1 rounds (cannot happen)

struct JdTable {
    uint16_t look[1 << JD_LOOK];                    // (length << 8) | symbol for codes of up to JD_LOOK bits, 0: longer
    int32_t maxcode[18];
    int32_t valoff[17];
    int32_t nvals;
    uint8_t vals[256];
};

// one image, in LDS on the GPU
struct JdCtx {
    uint32_t ok;
    uint32_t nbits;                                 // of the scan
    uint32_t nsub;
    uint32_t total;                                 // blocks
    uint32_t mcus_w;
    uint32_t ncomp, bpm;
    uint32_t bw[3], nblk[3], ch[3], cv[3];          // blocks per row, blocks, sampling factors of a component
    uint64_t plane_off[3];                          // in the coefficient record
    uint8_t blk_comp[8], blk_h[8], blk_v[8];        // block in MCU -> component, position inside the MCU
    int16_t lim[3][64];                             // largest |coefficient| by zig-zag position
    JdTable dc[3], ac[3];                           // per component
};

// zig-zag position -> natural position
JD_FN int jd_natural_of(int k) {
    constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63];
}

// subsequences of a scan record of `record_bytes`: what the workspace is sized for (the device's own count, from the
// record's scan_bytes, is checked against it)
JD_FN uint64_t jd_nsub_bound(uint64_t record_bytes) {
    const uint64_t scan = record_bytes > JD_SCAN_AT ? record_bytes - JD_SCAN_AT : 0;
    const uint64_t n = (scan * 8 + JD_SUB_BITS - 1) / JD_SUB_BITS;
    return n ? n : 1;
}
// workspace of one image: 16 bytes of flags, then exit state, last input state (8 bytes each), completed blocks and first block
// ordinal (4 bytes each) per subsequence; a multiple of 128
JD_FN uint64_t jd_workspace_bytes(uint64_t nsub_cap) { return (16 + 24 * nsub_cap + 127) / 128 * 128; }

struct JdWork {
    uint32_t* flags;                                // [0]: the last block was completed, [1]: re-decode rounds of the sync kernel
    jd_state* exit;
    jd_state* in;
    uint32_t* count;
    uint32_t* first;
};
JD_FN JdWork jd_work(uint8_t* tmp, uint64_t nsub_cap) {
    JdWork w;
    w.flags = (uint32_t*)tmp;
    w.exit = (jd_state*)(tmp + 16);
    w.in = w.exit + nsub_cap;
    w.count = (uint32_t*)(w.in + nsub_cap);
    w.first = w.count + nsub_cap;
    return w;
}

// Validation of one scan record and of the caller's sizes, by ONE thread; fills everything of ctx but the tables' look[] /
// vals[] and lim[] (jd_setup_tables).  rec: the record, rec_bytes: what the caller says it has (already inside the buffer);
// coef_size: the bytes the caller gives the coefficient record; nsub_cap: the subsequences the workspace holds.
JD_FN void jd_setup(JdCtx* x, const uint8_t* rec, uint64_t rec_bytes, uint64_t coef_size, uint64_t nsub_cap) {
    x->ok = 0;
    if (rec_bytes < JD_SCAN_AT + 8) return;
    const gitmi_jpeg_header* h = (const gitmi_jpeg_header*)rec;
    const gitmi_jpeg_scan* s = (const gitmi_jpeg_scan*)(rec + GITMI_JPEG_HEADER_BYTES);
    if (h->magic != GITMI_JPEG_MAGIC || h->header_bytes != GITMI_JPEG_HEADER_BYTES) return;
    if (s->magic != GITMI_JPEG_SCAN_MAGIC || s->scan_struct_bytes != GITMI_JPEG_SCAN_BYTES) return;
    const uint32_t nc = h->ncomp, W = h->width, H = h->height;
    if ((nc != 1 && nc != 3) || s->ncomp != nc || h->restart_interval != 0) return;
    if (W < 1 || H < 1 || W > GITMI_JPEG_MAX_DIM || H > GITMI_JPEG_MAX_DIM) return;
    const uint32_t h0 = h->comp[0].h_samp, v0 = h->comp[0].v_samp;
    if (nc == 1 ? (h0 != 1 || v0 != 1) : !((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2))) return;
    const uint32_t mw = (W + 8u * h0 - 1) / (8u * h0), mh = (H + 8u * v0 - 1) / (8u * v0);
    if (h->mcus_w != mw || h->mcus_h != mh) return;
    uint64_t bytes = GITMI_JPEG_HEADER_BYTES;
    uint32_t bpm = 0;
    for (uint32_t c = 0; c < nc; ++c) {
        const uint32_t hs = c ? 1 : h0, vs = c ? 1 : v0;
        const gitmi_jpeg_comp& hc = h->comp[c];
        const uint64_t nblk = (uint64_t)(mw * hs) * (mh * vs);
        if (hc.h_samp != hs || hc.v_samp != vs || hc.tq > 3 || hc.blocks_w != mw * hs || hc.blocks_h != mh * vs ||
            hc.plane_offset != bytes || nblk > GITMI_JPEG_SCAN_MAX_BLOCKS || s->td[c] > 3 || s->ta[c] > 3)
            return;
        x->bw[c] = mw * hs; x->nblk[c] = (uint32_t)nblk; x->ch[c] = hs; x->cv[c] = vs; x->plane_off[c] = bytes;
        for (uint32_t v = 0; v < vs; ++v)
            for (uint32_t hh = 0; hh < hs; ++hh) {
                x->blk_comp[bpm] = (uint8_t)c; x->blk_h[bpm] = (uint8_t)hh; x->blk_v[bpm] = (uint8_t)v;
                ++bpm;                              // at most 2 * 2 + 1 + 1 = 6
            }
        bytes += nblk * 128;
    }
    if (h->record_bytes != bytes || coef_size != bytes) return;
    const uint64_t total = (uint64_t)mw * mh * bpm;
    if (s->blocks_per_mcu != bpm || s->total_blocks != total) return;
    const uint64_t sb = s->scan_bytes;
    if (s->scan_offset != JD_SCAN_AT || sb >= GITMI_JPEG_SCAN_MAX_BYTES || sb + 8 > rec_bytes - JD_SCAN_AT) return;
    const uint64_t nsub = (sb * 8 + JD_SUB_BITS - 1) / JD_SUB_BITS;
    if (nsub > nsub_cap) return;
    // the code tables: canonical codes as jpeg_entropy.cc: build_huff assigns them
    for (uint32_t t = 0; t < 2 * nc; ++t) {
        const uint32_t c = t >> 1;
        const gitmi_jpeg_dht& d = (t & 1) ? s->ac[s->ta[c]] : s->dc[s->td[c]];
        JdTable& T = (t & 1) ? x->ac[c] : x->dc[c];
        int code = 0, idx = 0;
        for (int l = 1; l <= 16; ++l) {
            const int cnt = d.counts[l - 1];
            T.valoff[l] = idx - code;
            if (cnt) {
                if (code + cnt > (1 << l)) return;
                code += cnt;
                idx += cnt;
                T.maxcode[l] = code - 1;
            } else {
                T.maxcode[l] = -1;
            }
            code <<= 1;
        }
        if (idx > 256) return;
        T.maxcode[0] = -1; T.maxcode[17] = 0x7fffffff; T.valoff[0] = 0;
        T.nvals = idx;
    }
    x->nbits = (uint32_t)(sb * 8); x->nsub = (uint32_t)nsub; x->total = (uint32_t)total; x->mcus_w = mw;
    x->ncomp = nc; x->bpm = bpm;
    x->ok = 1;
}

// look[], vals[] and lim[] of a checked record, by all `nthreads` threads
JD_FN void jd_setup_tables(JdCtx* x, const uint8_t* rec, int tid, int nthreads) {
    const gitmi_jpeg_header* h = (const gitmi_jpeg_header*)rec;
    const gitmi_jpeg_scan* s = (const gitmi_jpeg_scan*)(rec + GITMI_JPEG_HEADER_BYTES);
    const int nt = 2 * (int)x->ncomp;
    for (int e = tid; e < nt * 512; e += nthreads) {
        const int t = e >> 9, i = e & 511, c = t >> 1;
        const gitmi_jpeg_dht& d = (t & 1) ? s->ac[s->ta[c]] : s->dc[s->td[c]];
        JdTable& T = (t & 1) ? x->ac[c] : x->dc[c];
        uint16_t entry = 0;
        for (int l = 1; l <= JD_LOOK; ++l) {        // the first length whose largest code is not below the prefix
            const int code = i >> (JD_LOOK - l);
            if (code <= T.maxcode[l]) {
                const int at = T.valoff[l] + code;  // within [0, nvals): code >= the first code of the length
                entry = (uint16_t)((l << 8) | d.symbols[at & 255]);
                break;
            }
        }
        T.look[i] = entry;
        if (i < 256) T.vals[i] = d.symbols[i];
    }
    for (int e = tid; e < (int)x->ncomp * 64; e += nthreads) {
        const int c = e >> 6, k = e & 63;
        const unsigned q = h->qt[h->comp[c].tq][jd_natural_of(k)];
        x->lim[c][k] = (int16_t)(q ? JD_COEF_LIMIT / (int)q : JD_COEF_LIMIT);
    }
}

// lim[c][0] alone, for the DC pass (one thread)
JD_FN void jd_setup_dc_limit(JdCtx* x, const uint8_t* rec, int c) {
    const gitmi_jpeg_header* h = (const gitmi_jpeg_header*)rec;
    const unsigned q = h->qt[h->comp[c].tq][0];
    x->lim[c][0] = (int16_t)(q ? JD_COEF_LIMIT / (int)q : JD_COEF_LIMIT);
}

JD_FN uint32_t jd_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

// the 32 bits at bit `pos` < nbits of the scan (aligned words; the record has 8 zero bytes behind the scan)
JD_FN uint32_t jd_peek32(const uint32_t* words, uint32_t pos) {
    const uint32_t w = pos >> 5, s = pos & 31;
    const uint32_t hi = jd_bswap(words[w]);
    if (!s) return hi;
    return (hi << s) | (jd_bswap(words[w + 1]) >> (32 - s));
}

JD_FN int jd_extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// one Huffman code at the top of `bits`; -> symbol and *len, or -1
JD_FN int jd_symbol(const JdTable& T, uint32_t bits, int* len) {
    const uint16_t e = T.look[bits >> (32 - JD_LOOK)];
    if (e) {
        *len = e >> 8;
        return e & 255;
    }
    for (int l = JD_LOOK + 1; l <= 16; ++l) {
        const int code = (int)(bits >> (32 - l));
        if (code <= T.maxcode[l]) {
            const int i = T.valoff[l] + code;
            if (i < 0 || i >= T.nvals) return -1;
            *len = l;
            return T.vals[i];
        }
    }
    return -1;
}

// One symbol with its magnitude bits at state (pos, b, k), pos < nbits.  false: an anomaly, the state is left as it was.
// *zz >= 0: the symbol carries the value *val for zig-zag position *zz of the block it belongs to (0: the DC difference);
// *done: it completes that block.
JD_FN bool jd_step(const JdCtx& x, const uint32_t* words, uint32_t& pos, int& b, int& k, int* zz, int* val, bool* done) {
    const int c = x.blk_comp[b];
    const uint32_t bits = jd_peek32(words, pos);
    *zz = -1;
    *done = false;
    int len = 0;
    if (k == 0) {
        const int t = jd_symbol(x.dc[c], bits, &len);
        if (t < 0 || t > 11) return false;
        if (len + t > (int)(x.nbits - pos)) return false;
        *zz = 0;
        *val = t ? jd_extend((bits << len) >> (32 - t), t) : 0;
        pos += (uint32_t)(len + t);
        k = 1;
        return true;
    }
    const int rs = jd_symbol(x.ac[c], bits, &len);
    if (rs < 0) return false;
    const int r = rs >> 4, s = rs & 15;
    if (len + s > (int)(x.nbits - pos)) return false;
    int nk = k;
    if (s == 0) {
        if (r == 0) {
            nk = 64;                                // end of block
        } else {
            if (r != 15) return false;              // EOBn belongs to progressive scans
            nk += 16;
            if (nk > 63) return false;              // a run that no coefficient follows
        }
    } else {
        if (s > 10) return false;
        nk += r;
        if (nk > 63) return false;
        *zz = nk;
        *val = jd_extend((bits << len) >> (32 - s), s);
        ++nk;
    }
    pos += (uint32_t)(len + s);
    k = nk;
    if (k >= 64) {
        k = 0;
        b = b + 1 == (int)x.bpm ? 0 : b + 1;
        *done = true;
    }
    return true;
}

// false: not a state subsequence i can be entered with
JD_FN bool jd_unpack(const JdCtx& x, uint32_t i, jd_state st, uint32_t& pos, int& b, int& k) {
    pos = (uint32_t)(st >> 16);
    b = (int)((st >> 8) & 255);
    k = (int)(st & 255);
    return (st >> 48) == 0 && pos >= i * (uint32_t)JD_SUB_BITS && b < (int)x.bpm && k < 64;
}

JD_FN uint32_t jd_sub_end(const JdCtx& x, uint32_t i) {
    const uint64_t e = ((uint64_t)i + 1) * JD_SUB_BITS;
    return e < x.nbits ? (uint32_t)e : x.nbits;
}

// Sync: subsequence i from state `in`: every symbol that STARTS in front of the subsequence's end; an anomaly skips one bit
// and restarts at (block 0, k 0).  -> the exit state; *count: blocks completed.  At most JD_SUB_BITS iterations: every
// iteration moves at least one bit on.
JD_FN jd_state jd_walk(const JdCtx& x, const uint32_t* words, uint32_t i, jd_state in, uint32_t* count) {
    uint32_t pos;
    int b, k;
    if (!jd_unpack(x, i, in, pos, b, k)) { pos = i * (uint32_t)JD_SUB_BITS; b = 0; k = 0; }    // no exit state is such a value
    const uint32_t end = jd_sub_end(x, i);
    uint32_t n = 0;
    while (pos < end) {
        int zz, val;
        bool done;
        if (!jd_step(x, words, pos, b, k, &zz, &val, &done)) { ++pos; b = 0; k = 0; continue; }
        n += done ? 1u : 0u;
    }
    *count = n;
    return jd_pack(pos, b, k);
}

// Write: subsequence i once more from its final input state, `ordinal` = blocks completed in front of it.  Values go to
// the planes of the coefficient record `coef` (zeroed before): AC to their natural position, the DC DIFFERENCE to position 0.
// -> status bits; *last: this subsequence completed the image's last block.
JD_FN int jd_write(const JdCtx& x, const uint32_t* words, uint32_t i, jd_state in, uint32_t ordinal, uint8_t* coef, bool* last) {
    *last = false;
    uint32_t pos;
    int b, k;
    if (ordinal >= x.total) return 0;               // behind the last block: nothing to write, nothing to judge
    if (!jd_unpack(x, i, in, pos, b, k)) return JD_ST_STREAM;                 // no exit state is such a value
    const uint32_t end = jd_sub_end(x, i);
    int status = 0;
    int16_t* blk = nullptr;
    const int16_t* lim = x.lim[0];
    bool fresh = true;                              // (b, ordinal) changed: find the block
    while (pos < end) {
        if (fresh) {
            const uint32_t mcu = ordinal / x.bpm, mx = mcu % x.mcus_w, my = mcu / x.mcus_w;
            const int c = x.blk_comp[b];
            const uint64_t at = (uint64_t)(my * x.cv[c] + x.blk_v[b]) * x.bw[c] + (mx * x.ch[c] + x.blk_h[b]);
            blk = at < x.nblk[c] ? (int16_t*)(coef + x.plane_off[c] + at * 128) : nullptr;
            lim = x.lim[c];
            fresh = false;
        }
        int zz, val;
        bool done;
        if (!jd_step(x, words, pos, b, k, &zz, &val, &done)) return status | JD_ST_STREAM;
        if (zz >= 0) {
            if (zz > 0 && (val > lim[zz] || val < -lim[zz])) status |= JD_ST_LIMIT;
            if (blk) blk[jd_natural_of(zz)] = (int16_t)val;
        }
        if (done) {
            fresh = true;
            if (++ordinal == x.total) {
                *last = true;
                if (x.nbits - pos >= 8) status |= JD_ST_TAIL;
                return status;
            }
        }
    }
    return status;
}

// DC: plane block of the j-th block of component c in coding order (MCU order, then v, h inside the MCU)
JD_FN uint32_t jd_dc_block(const JdCtx& x, int c, uint32_t j) {
    const uint32_t per = x.ch[c] * x.cv[c], mcu = j / per, in = j - mcu * per;
    const uint32_t mx = mcu % x.mcus_w, my = mcu / x.mcus_w, v = in / x.ch[c], hh = in - v * x.ch[c];
    return (my * x.cv[c] + v) * x.bw[c] + mx * x.ch[c] + hh;
}
// the predictor of a block goes to its position 0; -> status bits
JD_FN int jd_dc_store(const JdCtx& x, int c, uint32_t j, int pred, uint8_t* coef) {
    const uint32_t at = jd_dc_block(x, c, j);
    if (at >= x.nblk[c]) return JD_ST_RECORD;
    const int lim = x.lim[c][0];
    if (pred > lim || pred < -lim) return JD_ST_LIMIT;  // the host stops here; the value would not fit 16 bits at worst
    *(int16_t*)(coef + x.plane_off[c] + (uint64_t)at * 128) = (int16_t)pred;
    return 0;
}
JD_FN int jd_dc_load(const JdCtx& x, int c, uint32_t j, const uint8_t* coef) {
    const uint32_t at = jd_dc_block(x, c, j);
    return at < x.nblk[c] ? *(const int16_t*)(coef + x.plane_off[c] + (uint64_t)at * 128) : 0;
}
