// Host half of the split JPEG decode (include/gitmi_jpeg.h): marker parsing and Huffman decoding of a baseline / extended
// sequential JPEG into a coefficient record.  Plain C++17, no HIP header, no GPU: decode-pool workers load this library.
//
// The fast path only ever sees clean streams: everything outside it, and ANY anomaly inside it, returns
// GITMI_JPEG_UNSUPPORTED and the caller decodes that image with Pillow, which stays the sole judge of broken and exotic files.
// Reads stay inside [jpg, jpg + n), writes inside [out, out + out_cap), whatever the bytes are.
#include "../../include/gitmi_jpeg.h"

#include <string.h>

namespace {

const uint8_t kNatural[64] = {                 // zig-zag position -> natural (row-major) position
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// A dequantised coefficient of an 8-bit image is at most 1024 in magnitude (an orthonormal 8x8 basis function has an L1 norm
// of at most 8, samples are within +-128) plus half a quantiser step (<= 127.5 for 8-bit tables, more for 16-bit ones whose
// steps an honest encoder then never reaches).  Within +-2047 every 16-bit intermediate of libjpeg-turbo's SIMD inverse DCT
// holds what the C source's 32-bit ones hold (pass 1 is at most 16 * max |input|), so the arithmetic is DEFINED and the GPU
// reproduces it; a stream beyond the bound is not a clean stream and goes to Pillow.
const int kCoefLimit = 2047;
const int kLook = 9;                           // look-ahead bits of the Huffman tables

struct Huff {
    uint16_t look[1 << kLook];                 // (length << 8) | symbol for codes of up to kLook bits, 0: longer
    int16_t fast_ac[1 << kLook];               // AC only: code and magnitude bits both inside the look-ahead:
                                               // (value << 8) | (run << 4) | total bits, 0: none
    int32_t maxcode[18];                       // largest code of each length, -1: no code of that length
    int32_t valoff[17];                        // index of a length's first symbol minus its first code
    uint8_t vals[256];
    int nvals;
    bool defined;
};

bool build_huff(Huff& h, const uint8_t counts[16], const uint8_t* symbols, int nsym, bool ac) {
    memset(&h, 0, sizeof(h));
    memcpy(h.vals, symbols, (size_t)nsym);
    h.nvals = nsym;
    int code = 0, idx = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = counts[l - 1];
        h.valoff[l] = idx - code;
        if (cnt) {
            if (code + cnt > (1 << l)) return false;                 // more codes than the length has
            if (l <= kLook) {
                for (int i = 0; i < cnt; ++i) {
                    const int c = (code + i) << (kLook - l);
                    const uint16_t e = (uint16_t)((l << 8) | symbols[idx + i]);
                    for (int j = 0; j < (1 << (kLook - l)); ++j) h.look[c + j] = e;
                }
            }
            code += cnt;
            idx += cnt;
            h.maxcode[l] = code - 1;
        } else {
            h.maxcode[l] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    if (ac) {
        for (int i = 0; i < (1 << kLook); ++i) {
            const uint16_t e = h.look[i];
            if (!e) continue;
            const int len = e >> 8, run = (e >> 4) & 15, mag = e & 15;
            if (mag == 0 || len + mag > kLook) continue;
            int k = ((i << len) & ((1 << kLook) - 1)) >> (kLook - mag);
            if (k < (1 << (mag - 1))) k += (int)((~0u) << mag) + 1;
            if (k >= -128 && k <= 127) h.fast_ac[i] = (int16_t)(k * 256 + run * 16 + len + mag);
        }
    }
    h.defined = true;
    return true;
}

// 64-bit bit buffer over the entropy-coded segment.  Bytes enter at the low end; FF 00 is unstuffed; at a marker or at the end
// of the data the reader stops consuming and feeds zero bits, counted in `pad`, so that running past the segment is seen
// (cnt - pad < 0) and never reads past `end`.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf;
    int cnt;
    long long pad;
    bool stopped;

    void reset(const uint8_t* at) { p = at; buf = 0; cnt = 0; pad = 0; stopped = false; }

    void fill_slow() {
        while (cnt <= 56) {
            if (!stopped) {
                if (p >= end) { stopped = true; continue; }
                const uint8_t b = *p;
                if (b == 0xFF) {
                    if (end - p < 2 || p[1] != 0) { stopped = true; continue; }
                    p += 2;
                } else {
                    ++p;
                }
                buf = (buf << 8) | b;
                cnt += 8;
            } else {
                buf <<= 8;
                cnt += 8;
                pad += 8;
            }
        }
    }

    inline void fill() {
        if (!stopped && end - p >= 8) {
            uint64_t w;
            memcpy(&w, p, 8);
            w = __builtin_bswap64(w);
            const uint64_t x = ~w;                                    // a zero byte of x is an FF byte of w
            if (!((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull)) {
                const int nb = (64 - cnt) >> 3;
                if (nb == 8) buf = w;
                else if (nb > 0) buf = (buf << (8 * nb)) | (w >> (64 - 8 * nb));
                cnt += 8 * nb;
                p += nb;
                return;
            }
        }
        fill_slow();
    }

    inline unsigned peek(int k) const { return (unsigned)(buf >> (cnt - k)) & ((1u << k) - 1); }
    inline void skip(int k) { cnt -= k; }
};

inline int extend(unsigned v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// one Huffman symbol; needs >= 16 bits in the buffer.  -1: no such code.
inline int decode_symbol(Bits& b, const Huff& h) {
    const uint16_t e = h.look[b.peek(kLook)];
    if (e) {
        b.skip(e >> 8);
        return e & 255;
    }
    for (int l = kLook + 1; l <= 16; ++l) {
        const int code = (int)b.peek(l);
        if (code <= h.maxcode[l]) {
            const int i = h.valoff[l] + code;
            if (i < 0 || i >= h.nvals) return -1;
            b.skip(l);
            return h.vals[i];
        }
    }
    return -1;
}

struct Comp {
    int id, h, v, tq, td, ta;
    uint32_t blocks_w, blocks_h;
    uint64_t offset;
    int pred;
    int16_t lim[64];                                                  // largest |coefficient| by zig-zag position
};

// one 8x8 block into blk (natural order); false: anomaly
inline bool decode_block(Bits& b, const Huff& dc, const Huff& ac, Comp& c, int16_t* blk) {
    memset(blk, 0, 128);
    if (b.cnt < 32) b.fill();
    int t = decode_symbol(b, dc);
    if (t < 0 || t > 11) return false;
    if (t) {
        const int diff = extend(b.peek(t), t);
        b.skip(t);
        c.pred += diff;
    }
    if (c.pred > c.lim[0] || c.pred < -c.lim[0]) return false;
    blk[0] = (int16_t)c.pred;
    int k = 1;
    while (k < 64) {
        if (b.cnt < 32) b.fill();
        const int f = ac.fast_ac[b.peek(kLook)];
        if (f) {
            k += (f >> 4) & 15;
            if (k > 63) return false;
            b.skip(f & 15);
            const int v = f >> 8;
            if (v > c.lim[k] || v < -c.lim[k]) return false;
            blk[kNatural[k]] = (int16_t)v;
            ++k;
            continue;
        }
        const int rs = decode_symbol(b, ac);
        if (rs < 0) return false;
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r == 0) break;                                        // end of block
            if (r != 15) return false;                                // EOBn belongs to progressive scans
            k += 16;
            if (k > 63) return false;                                 // a run that no coefficient follows
            continue;
        }
        if (s > 10) return false;
        k += r;
        if (k > 63) return false;
        const int v = extend(b.peek(s), s);
        b.skip(s);
        if (v > c.lim[k] || v < -c.lim[k]) return false;
        blk[kNatural[k]] = (int16_t)v;
        ++k;
    }
    return true;
}

inline unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

// Everything in front of the entropy-coded segment, shared by gitmi_jpeg_entropy_decode and gitmi_jpeg_scan_prepare: the
// marker segments, libjpeg's colour-space decision, the sampling factors of the fast path and the layout of the record.
struct Parsed {
    gitmi_jpeg_header hdr;                                            // qt[] only; the rest is filled by fill_header()
    Huff huff[2][4];                                                  // [dc / ac][table]
    gitmi_jpeg_dht dht[2][4];                                         // the same tables as the file has them
    Comp comp[3];
    int ncomp, restart;
    unsigned width, height;
    const uint8_t* scan;                                              // first byte behind the SOS segment
    uint32_t mcus_w, mcus_h;
    uint64_t bytes;                                                   // of the coefficient record
};

// GITMI_JPEG_OK or GITMI_JPEG_UNSUPPORTED; the caller has checked n >= 4 and the SOI
int parse_markers(const uint8_t* jpg, size_t n, Parsed& P) {
    gitmi_jpeg_header& hdr = P.hdr;
    memset(&hdr, 0, sizeof(hdr));
    memset(P.dht, 0, sizeof(P.dht));
    Huff (&huff)[2][4] = P.huff;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 4; ++j) huff[i][j].defined = false;
    bool have_qt[4] = {false, false, false, false};
    Comp (&comp)[3] = P.comp;
    int ncomp = 0, restart = 0;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    unsigned width = 0, height = 0;

    size_t pos = 2;
    const uint8_t* scan = nullptr;
    while (!scan) {
        // a marker: FF, any number of fill FFs, the code
        if (n - pos < 2 || jpg[pos] != 0xFF) return GITMI_JPEG_UNSUPPORTED;
        while (pos < n && jpg[pos] == 0xFF) ++pos;
        if (pos >= n) return GITMI_JPEG_UNSUPPORTED;
        const unsigned m = jpg[pos++];
        if (m == 0x00 || m == 0x01 || m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7)) return GITMI_JPEG_UNSUPPORTED;
        if (n - pos < 2) return GITMI_JPEG_UNSUPPORTED;
        const size_t len = be16(jpg + pos);
        if (len < 2 || len > n - pos) return GITMI_JPEG_UNSUPPORTED;
        const uint8_t* d = jpg + pos + 2;                             // the segment's data
        const size_t dl = len - 2;
        pos += len;
        switch (m) {
        case 0xC0: case 0xC1: {                                       // SOF0 / SOF1
            if (have_sof || dl < 6) return GITMI_JPEG_UNSUPPORTED;
            if (d[0] != 8) return GITMI_JPEG_UNSUPPORTED;
            height = be16(d + 1);
            width = be16(d + 3);
            ncomp = d[5];
            if ((ncomp != 1 && ncomp != 3) || dl != 6 + 3 * (size_t)ncomp) return GITMI_JPEG_UNSUPPORTED;
            if (width < 1 || height < 1 || width > GITMI_JPEG_MAX_DIM || height > GITMI_JPEG_MAX_DIM) return GITMI_JPEG_UNSUPPORTED;
            for (int c = 0; c < ncomp; ++c) {
                comp[c].id = d[6 + 3 * c];
                comp[c].h = d[7 + 3 * c] >> 4;
                comp[c].v = d[7 + 3 * c] & 15;
                comp[c].tq = d[8 + 3 * c];
                if (comp[c].h < 1 || comp[c].h > 4 || comp[c].v < 1 || comp[c].v > 4 || comp[c].tq > 3) return GITMI_JPEG_UNSUPPORTED;
            }
            have_sof = true;
            break;
        }
        case 0xC4: {                                                  // DHT
            size_t o = 0;
            while (o < dl) {
                if (dl - o < 17) return GITMI_JPEG_UNSUPPORTED;
                const int tc = d[o] >> 4, th = d[o] & 15;
                if (tc > 1 || th > 3) return GITMI_JPEG_UNSUPPORTED;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += d[o + 1 + i];
                if (total > 256 || dl - o - 17 < (size_t)total) return GITMI_JPEG_UNSUPPORTED;
                if (!build_huff(huff[tc][th], d + o + 1, d + o + 17, total, tc == 1)) return GITMI_JPEG_UNSUPPORTED;
                memset(&P.dht[tc][th], 0, sizeof(gitmi_jpeg_dht));
                memcpy(P.dht[tc][th].counts, d + o + 1, 16);
                memcpy(P.dht[tc][th].symbols, d + o + 17, (size_t)total);
                o += 17 + (size_t)total;
            }
            break;
        }
        case 0xDB: {                                                  // DQT
            size_t o = 0;
            while (o < dl) {
                const int pq = d[o] >> 4, tq = d[o] & 15;
                if (pq > 1 || tq > 3) return GITMI_JPEG_UNSUPPORTED;
                const size_t need = pq ? 128 : 64;
                if (dl - o - 1 < need) return GITMI_JPEG_UNSUPPORTED;
                for (int i = 0; i < 64; ++i)
                    hdr.qt[tq][kNatural[i]] = pq ? (uint16_t)be16(d + o + 1 + 2 * i) : d[o + 1 + i];
                have_qt[tq] = true;
                o += 1 + need;
            }
            break;
        }
        case 0xDD:                                                    // DRI
            if (dl != 2) return GITMI_JPEG_UNSUPPORTED;
            restart = (int)be16(d);
            break;
        case 0xE0:                                                    // APP0: JFIF
            if (dl >= 14 && !memcmp(d, "JFIF\0", 5)) jfif = true;
            break;
        case 0xEE:                                                    // APP14: Adobe
            if (dl >= 12 && !memcmp(d, "Adobe", 5)) { adobe = true; adobe_transform = d[11]; }
            break;
        case 0xDA: {                                                  // SOS
            if (!have_sof || dl < 1 || d[0] != ncomp || dl != 4 + 2 * (size_t)ncomp) return GITMI_JPEG_UNSUPPORTED;
            for (int c = 0; c < ncomp; ++c) {
                if (d[1 + 2 * c] != comp[c].id) return GITMI_JPEG_UNSUPPORTED;
                comp[c].td = d[2 + 2 * c] >> 4;
                comp[c].ta = d[2 + 2 * c] & 15;
                if (comp[c].td > 3 || comp[c].ta > 3 || !huff[0][comp[c].td].defined || !huff[1][comp[c].ta].defined ||
                    !have_qt[comp[c].tq])
                    return GITMI_JPEG_UNSUPPORTED;
            }
            const uint8_t* t = d + 1 + 2 * ncomp;
            if (t[0] != 0 || t[1] != 63 || t[2] != 0) return GITMI_JPEG_UNSUPPORTED;       // Ss, Se, Ah / Al of a sequential scan
            scan = jpg + pos;
            break;
        }
        default:
            // every other frame type (progressive, lossless, arithmetic, hierarchical), DAC, DNL, DHP, EXP: not the fast path
            if ((m >= 0xC2 && m <= 0xCF) || (m >= 0xDC && m <= 0xDF)) return GITMI_JPEG_UNSUPPORTED;
            break;                                                    // APPn, COM, reserved: skipped
        }
    }

    // colour space as libjpeg decides it, and the sampling factors of the fast path
    if (ncomp == 3) {
        if (jfif) {
        } else if (adobe) {
            if (adobe_transform != 1) return GITMI_JPEG_UNSUPPORTED;
        } else if (comp[0].id != 1 || comp[1].id != 2 || comp[2].id != 3) {
            return GITMI_JPEG_UNSUPPORTED;
        }
        if (comp[1].h != 1 || comp[1].v != 1 || comp[2].h != 1 || comp[2].v != 1) return GITMI_JPEG_UNSUPPORTED;
        if (!((comp[0].h == 1 && comp[0].v == 1) || (comp[0].h == 2 && comp[0].v == 1) || (comp[0].h == 2 && comp[0].v == 2)))
            return GITMI_JPEG_UNSUPPORTED;
    } else {
        comp[0].h = comp[0].v = 1;                                    // a single-component scan codes ceil(w / 8) x ceil(h / 8) blocks
    }
    const uint32_t mcu_w = 8u * comp[0].h, mcu_h = 8u * comp[0].v;
    const uint32_t mcus_w = (width + mcu_w - 1) / mcu_w, mcus_h = (height + mcu_h - 1) / mcu_h;
    uint64_t bytes = GITMI_JPEG_HEADER_BYTES;
    for (int c = 0; c < ncomp; ++c) {
        comp[c].blocks_w = mcus_w * comp[c].h;
        comp[c].blocks_h = mcus_h * comp[c].v;
        comp[c].offset = bytes;
        bytes += (uint64_t)comp[c].blocks_w * comp[c].blocks_h * 128;
        comp[c].pred = 0;
        for (int k = 0; k < 64; ++k) {
            const unsigned q = hdr.qt[comp[c].tq][kNatural[k]];
            comp[c].lim[k] = (int16_t)(q ? kCoefLimit / (int)q : kCoefLimit);
        }
    }
    P.ncomp = ncomp; P.restart = restart; P.width = width; P.height = height; P.scan = scan;
    P.mcus_w = mcus_w; P.mcus_h = mcus_h; P.bytes = bytes;
    return GITMI_JPEG_OK;
}

void fill_info(const Parsed& P, gitmi_jpeg_info* info) {
    if (!info) return;
    info->width = P.width; info->height = P.height; info->ncomp = (uint32_t)P.ncomp;
    info->h_samp = (uint32_t)P.comp[0].h; info->v_samp = (uint32_t)P.comp[0].v;
    info->record_bytes = P.bytes;
}

// the header of the coefficient record, complete
void fill_header(Parsed& P) {
    gitmi_jpeg_header& hdr = P.hdr;
    hdr.magic = GITMI_JPEG_MAGIC;
    hdr.header_bytes = GITMI_JPEG_HEADER_BYTES;
    hdr.width = P.width; hdr.height = P.height; hdr.ncomp = (uint32_t)P.ncomp;
    hdr.mcus_w = P.mcus_w; hdr.mcus_h = P.mcus_h;
    hdr.restart_interval = (uint32_t)P.restart;
    hdr.record_bytes = P.bytes;
    for (int c = 0; c < P.ncomp; ++c) {
        const Comp& k = P.comp[c];
        hdr.comp[c].h_samp = (uint8_t)k.h; hdr.comp[c].v_samp = (uint8_t)k.v; hdr.comp[c].tq = (uint8_t)k.tq;
        hdr.comp[c].blocks_w = k.blocks_w; hdr.comp[c].blocks_h = k.blocks_h;
        hdr.comp[c].plane_offset = k.offset;
    }
}

}  // namespace

extern "C" int gitmi_jpeg_abi_version(void) { return GITMI_JPEG_ABI_VERSION; }

extern "C" int gitmi_jpeg_entropy_decode(const uint8_t* jpg, size_t n, void* out, size_t out_cap, gitmi_jpeg_info* info) {
    if ((!jpg && n) || (!out && out_cap) || ((uintptr_t)out & 7)) return GITMI_JPEG_BAD_ARGUMENT;
    if (info) memset(info, 0, sizeof(*info));
    if (n < 4 || jpg[0] != 0xFF || jpg[1] != 0xD8) return GITMI_JPEG_UNSUPPORTED;

    static_assert(sizeof(gitmi_jpeg_header) == GITMI_JPEG_HEADER_BYTES, "record header layout");
    Parsed P;
    if (parse_markers(jpg, n, P) != GITMI_JPEG_OK) return GITMI_JPEG_UNSUPPORTED;
    Huff (&huff)[2][4] = P.huff;
    Comp (&comp)[3] = P.comp;
    const int ncomp = P.ncomp, restart = P.restart;
    const uint8_t* scan = P.scan;
    const uint32_t mcus_w = P.mcus_w, mcus_h = P.mcus_h;
    const uint64_t bytes = P.bytes;
    fill_info(P, info);
    if (bytes > out_cap) return GITMI_JPEG_NO_SPACE;

    uint8_t* rec = (uint8_t*)out;
    Bits b;
    b.end = jpg + n;
    b.reset(scan);
    const uint64_t total = (uint64_t)mcus_w * mcus_h;
    uint32_t mx = 0, my = 0;
    int next_rst = 0;
    for (uint64_t mcu = 0; mcu < total; ++mcu) {
        if (restart && mcu && mcu % (uint64_t)restart == 0) {
            // the interval ends on a byte boundary (fewer than 8 padding bits left) right in front of the expected RSTn
            const long long rem = b.cnt - b.pad;
            if (rem < 0 || rem >= 8 || b.end - b.p < 2 || b.p[0] != 0xFF || b.p[1] != 0xD0 + next_rst) return GITMI_JPEG_UNSUPPORTED;
            next_rst = (next_rst + 1) & 7;
            b.reset(b.p + 2);
            for (int c = 0; c < ncomp; ++c) comp[c].pred = 0;
        }
        for (int c = 0; c < ncomp; ++c) {
            Comp& cc = comp[c];
            const Huff& dc = huff[0][cc.td];
            const Huff& ac = huff[1][cc.ta];
            for (int v = 0; v < cc.v; ++v)
                for (int h = 0; h < cc.h; ++h) {
                    const uint64_t blk = (uint64_t)(my * cc.v + v) * cc.blocks_w + (mx * cc.h + h);
                    if (!decode_block(b, dc, ac, cc, (int16_t*)(rec + cc.offset + blk * 128))) return GITMI_JPEG_UNSUPPORTED;
                }
        }
        if (b.cnt - b.pad < 0) return GITMI_JPEG_UNSUPPORTED;         // the data ended inside this MCU
        if (++mx == mcus_w) { mx = 0; ++my; }
    }
    const long long rem = b.cnt - b.pad;
    if (rem < 0 || rem >= 8 || b.end - b.p < 2 || b.p[0] != 0xFF || b.p[1] != 0xD9) return GITMI_JPEG_UNSUPPORTED;      // EOI

    fill_header(P);
    memcpy(rec, &P.hdr, sizeof(P.hdr));
    return GITMI_JPEG_OK;
}

// The parse above, then the entropy-coded segment as it is: FF 00 -> FF, nothing decoded.  The segment must run to an EOI with
// no other marker in it; restart intervals, which the GPU Huffman decode does not take, are declined here (and decoded by
// gitmi_jpeg_entropy_decode).
extern "C" int gitmi_jpeg_scan_prepare(const uint8_t* jpg, size_t n, void* out, size_t out_cap, gitmi_jpeg_info* info,
                                       uint64_t* scan_record_bytes) {
    if ((!jpg && n) || (!out && out_cap) || ((uintptr_t)out & 7)) return GITMI_JPEG_BAD_ARGUMENT;
    if (info) memset(info, 0, sizeof(*info));
    if (scan_record_bytes) *scan_record_bytes = 0;
    if (n < 4 || jpg[0] != 0xFF || jpg[1] != 0xD8) return GITMI_JPEG_UNSUPPORTED;

    static_assert(sizeof(gitmi_jpeg_scan) == GITMI_JPEG_SCAN_BYTES, "scan description layout");
    static_assert(sizeof(gitmi_jpeg_dht) == 272, "scan description layout");
    Parsed P;
    if (parse_markers(jpg, n, P) != GITMI_JPEG_OK) return GITMI_JPEG_UNSUPPORTED;
    if (P.restart != 0) return GITMI_JPEG_UNSUPPORTED;
    uint32_t per_mcu = 0;
    for (int c = 0; c < P.ncomp; ++c) {
        if ((uint64_t)P.comp[c].blocks_w * P.comp[c].blocks_h > GITMI_JPEG_SCAN_MAX_BLOCKS) return GITMI_JPEG_UNSUPPORTED;
        per_mcu += (uint32_t)(P.comp[c].h * P.comp[c].v);
    }

    // the length of the unstuffed segment: up to the first FF that no 00 follows, which must be the EOI
    const uint8_t* const end = jpg + n;
    const uint8_t* p = P.scan;
    uint64_t stuffed = 0;
    for (;;) {
        p = (const uint8_t*)memchr(p, 0xFF, (size_t)(end - p));
        if (!p || end - p < 2) return GITMI_JPEG_UNSUPPORTED;          // no EOI
        if (p[1] == 0x00) { ++stuffed; p += 2; continue; }
        if (p[1] != 0xD9) return GITMI_JPEG_UNSUPPORTED;              // RSTn, fill bytes, any other marker
        break;
    }
    const uint64_t scan_bytes = (uint64_t)(p - P.scan) - stuffed;
    if (scan_bytes >= GITMI_JPEG_SCAN_MAX_BYTES) return GITMI_JPEG_UNSUPPORTED;
    const uint64_t at = GITMI_JPEG_HEADER_BYTES + GITMI_JPEG_SCAN_BYTES;
    const uint64_t total = at + ((scan_bytes + 8 + 15) & ~(uint64_t)15);
    fill_info(P, info);
    if (scan_record_bytes) *scan_record_bytes = total;
    if (total > out_cap) return GITMI_JPEG_NO_SPACE;

    uint8_t* rec = (uint8_t*)out;
    fill_header(P);
    memcpy(rec, &P.hdr, sizeof(P.hdr));
    gitmi_jpeg_scan sc;
    memset(&sc, 0, sizeof(sc));
    sc.magic = GITMI_JPEG_SCAN_MAGIC;
    sc.scan_struct_bytes = GITMI_JPEG_SCAN_BYTES;
    sc.ncomp = (uint32_t)P.ncomp;
    sc.blocks_per_mcu = per_mcu;
    sc.total_blocks = P.mcus_w * P.mcus_h * per_mcu;
    sc.scan_bytes = (uint32_t)scan_bytes;
    sc.scan_offset = at;
    sc.scan_record_bytes = total;
    for (int c = 0; c < P.ncomp; ++c) {
        sc.td[c] = (uint8_t)P.comp[c].td;
        sc.ta[c] = (uint8_t)P.comp[c].ta;
        sc.dc[P.comp[c].td] = P.dht[0][P.comp[c].td];
        sc.ac[P.comp[c].ta] = P.dht[1][P.comp[c].ta];
    }
    memcpy(rec + GITMI_JPEG_HEADER_BYTES, &sc, sizeof(sc));
    uint8_t* w = rec + at;
    const uint8_t* s = P.scan;
    while (s < p) {                                                   // runs between the FFs, each FF 00 pair as one FF
        const uint8_t* f = (const uint8_t*)memchr(s, 0xFF, (size_t)(p - s));
        const size_t run = (size_t)((f ? f + 1 : p) - s);
        memcpy(w, s, run);
        w += run;
        s += run + (f ? 1 : 0);
    }
    memset(w, 0, (size_t)(rec + total - w));
    return GITMI_JPEG_OK;
}
