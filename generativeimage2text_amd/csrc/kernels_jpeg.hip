// GPU half of the split JPEG decode (include/gitmi_jpeg.h): coefficient records -> uint8 [H, W, 3], bit for bit what Pillow's
// Image.open(...).convert("RGB") returns.  libjpeg's default reconstruction is fixed-point integer arithmetic with a defined
// result; it is restated here (and in numpy in tools/jpeg_oracle.py):
//   pass 1  dequantise + jpeg_idct_islow (13-bit constants, PASS1_BITS = 2, columns then rows, DESCALE rounding, +128, clamp)
//           -> uint8 component planes at block-padded size in the workspace;
//   pass 2  fancy (triangle) upsampling of the chroma planes for h2v1 / h2v2, fused with ycc_rgb_convert's 16.16 colour
//           conversion and the RGB store.
// Two launches per JPEG_CHUNK images, grids over (tile, image): the submitting host thread bounds a per-image form.
// The records come from files from outside: each kernel validates the record header against the caller's (H, W) and the
// buffer sizes before it forms any address, and leaves an image whose record does not check out unwritten.
#include "jpeg_common.h"

namespace {

struct JpegView {
    int ncomp, h2, v2;                              // luma sampled 2x horizontally / vertically
    int bw[3], bh[3];                               // blocks of each plane
    const int16_t* coef[3];
    const uint16_t* qt[3];
    uint8_t* plane[3];                              // uint8 [bh * 8][bw * 8]
};

__device__ __forceinline__ bool jpeg_view(const uint8_t* coef, size_t coef_bytes, const JpegImg& d, uint8_t* tmp, JpegView& v) {
    const gitmi_jpeg_header* h = (const gitmi_jpeg_header*)(coef + d.coef_off);      // the host checked coef_off + header <= coef_bytes
    if (h->magic != GITMI_JPEG_MAGIC || h->header_bytes != GITMI_JPEG_HEADER_BYTES) return false;
    if ((int)h->width != d.W || (int)h->height != d.H) return false;
    const int nc = (int)h->ncomp;
    if (nc != 1 && nc != 3) return false;
    const int h0 = h->comp[0].h_samp, v0 = h->comp[0].v_samp;
    if (nc == 1 ? (h0 != 1 || v0 != 1) : !((h0 == 1 && v0 == 1) || (h0 == 2 && v0 == 1) || (h0 == 2 && v0 == 2))) return false;
    const unsigned mw = ((unsigned)d.W + 8u * h0 - 1) / (8u * h0), mh = ((unsigned)d.H + 8u * v0 - 1) / (8u * v0);
    if (h->mcus_w != mw || h->mcus_h != mh) return false;
    const size_t room = coef_bytes - d.coef_off;
    size_t planes = 0;
    v.ncomp = nc; v.h2 = h0 == 2; v.v2 = v0 == 2;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                   // unrolled, no early exit: the view's arrays stay in registers
        const bool used = c < nc;
        const int hs = c ? 1 : h0, vs = c ? 1 : v0;
        const gitmi_jpeg_comp& hc = h->comp[c];
        const size_t bytes = (size_t)(mw * hs) * (mh * vs) * 128;
        const unsigned long long off = hc.plane_offset;
        const bool good = hc.h_samp == hs && hc.v_samp == vs && hc.tq <= 3 && hc.blocks_w == mw * hs && hc.blocks_h == mh * vs &&
                          off >= GITMI_JPEG_HEADER_BYTES && !(off & 127) && off <= room && bytes <= room - off;
        ok = ok && (good || !used);
        const bool take = used && good;
        v.bw[c] = take ? (int)(mw * hs) : 0; v.bh[c] = take ? (int)(mh * vs) : 0;
        v.coef[c] = (const int16_t*)(coef + d.coef_off + (take ? off : 0));
        v.qt[c] = h->qt[take ? hc.tq : 0];
        v.plane[c] = tmp + d.tmp_off + planes;
        planes += take ? bytes / 2 : 0;             // 64 samples per 128-byte block
    }
    if (!ok) return false;
    return planes <= jpeg_plane_bytes_bound(d.H, d.W);
}

constexpr int C_0_298631336 = 2446, C_0_390180644 = 3196, C_0_541196100 = 4433, C_0_765366865 = 6270, C_0_899976223 = 7373,
              C_1_175875602 = 9633, C_1_501321110 = 12299, C_1_847759065 = 15137, C_1_961570560 = 16069, C_2_053119869 = 16819,
              C_2_562915447 = 20995, C_3_072711026 = 25172;

// one 8-point pass of jpeg_idct_islow, in place; the results are DESCALEd by `shift`
template <int shift>
__device__ __forceinline__ void idct_1d(int (&x)[8]) {
    int z1 = (x[2] + x[6]) * C_0_541196100;
    const int tmp2 = z1 - x[6] * C_1_847759065;
    const int tmp3 = z1 + x[2] * C_0_765366865;
    const int tmp0 = (x[0] + x[4]) * 8192;
    const int tmp1 = (x[0] - x[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * C_1_175875602;
    t0 *= C_0_298631336; t1 *= C_2_053119869; t2 *= C_3_072711026; t3 *= C_1_501321110;
    z1 *= -C_0_899976223; z2 *= -C_2_562915447;
    z3 = z3 * -C_1_961570560 + z5;
    z4 = z4 * -C_0_390180644 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr int r = 1 << (shift - 1);
    x[0] = (tmp10 + t3 + r) >> shift; x[7] = (tmp10 - t3 + r) >> shift;
    x[1] = (tmp11 + t2 + r) >> shift; x[6] = (tmp11 - t2 + r) >> shift;
    x[2] = (tmp12 + t1 + r) >> shift; x[5] = (tmp12 - t1 + r) >> shift;
    x[3] = (tmp13 + t0 + r) >> shift; x[4] = (tmp13 - t0 + r) >> shift;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

constexpr int IDCT_BLOCKS = 32;                     // 8x8 blocks per workgroup: 8 lanes each
constexpr int IDCT_LDS = 72;                        // ints per block in LDS: 64 + 8, so that the 8 blocks of a wave fall on all 64 banks

// grid (blocks of all planes / 32, image).  Lane j of a block's 8 loads coefficient ROW j as one 16-byte vector (a wave reads
// eight whole 128-byte blocks contiguously), transposes through LDS, runs column j, then row j, and stores 8 pixels of row j.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* __restrict__ coef, size_t coef_bytes, uint8_t* __restrict__ tmp,
                                                        JpegChunk ch) {
    __shared__ int ws[IDCT_BLOCKS * IDCT_LDS];
    const JpegImg& d = ch.d[blockIdx.y];
    JpegView v;
    if (!jpeg_view(coef, coef_bytes, d, tmp, v)) return;              // uniform over the workgroup
    const int lane = threadIdx.x & 7, lb = threadIdx.x >> 3;
    long long blk = (long long)blockIdx.x * IDCT_BLOCKS + lb;
    bool active = false;
    const int16_t* cp = nullptr;                    // the plane this lane's block belongs to
    const uint16_t* qp = nullptr;
    uint8_t* pp = nullptr;
    int bw = 1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < v.ncomp && !active) {
            const long long nb = (long long)v.bw[i] * v.bh[i];
            if (blk < nb) { active = true; cp = v.coef[i]; qp = v.qt[i]; pp = v.plane[i]; bw = v.bw[i]; }
            else blk -= nb;
        }
    }
    int* w = ws + lb * IDCT_LDS;
    int x[8];
    if (active) {
        const uint4 raw = *(const uint4*)(cp + blk * 64 + lane * 8);
        const uint4 q = *(const uint4*)(qp + lane * 8);
        const unsigned rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[lane * 8 + 2 * i] = (int)(short)(rw[i] & 0xffff) * (int)(qw[i] & 0xffff);
            w[lane * 8 + 2 * i + 1] = (int)(short)(rw[i] >> 16) * (int)(qw[i] >> 16);
        }
    }
    __syncthreads();
    if (active) {                                   // column `lane`: read and written by this lane alone
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = w[k * 8 + lane];
        idct_1d<13 - 2>(x);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * 8 + lane] = x[k];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = w[lane * 8 + k];
        idct_1d<13 + 2 + 3>(x);
        uint2 px;
        px.x = (unsigned)clamp255(x[0] + 128) | ((unsigned)clamp255(x[1] + 128) << 8) | ((unsigned)clamp255(x[2] + 128) << 16) |
               ((unsigned)clamp255(x[3] + 128) << 24);
        px.y = (unsigned)clamp255(x[4] + 128) | ((unsigned)clamp255(x[5] + 128) << 8) | ((unsigned)clamp255(x[6] + 128) << 16) |
               ((unsigned)clamp255(x[7] + 128) << 24);
        const int by = (int)(blk / bw), bx = (int)(blk - (long long)by * bw);
        *(uint2*)(pp + ((size_t)by * 8 + lane) * ((size_t)bw * 8) + (size_t)bx * 8) = px;
    }
}

// one chroma sample at full resolution: libjpeg's fancy upsampling over the REAL downsampled samples (cw x chh), edges
// replicated -- which is what its first / last column special cases and its replicated context rows compute
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, int pitch, int y, int x, int cw, int chh, bool h2, bool v2) {
    if (!h2) return p[(size_t)y * pitch + x];
    const int j = x >> 1;
    if (cw <= 2) return p[(size_t)(v2 ? y >> 1 : y) * pitch + j];    // libjpeg: box filter at a downsampled width of 2 or less
    const int jn = (x & 1) ? (j + 1 < cw ? j + 1 : j) : (j > 0 ? j - 1 : 0);
    if (!v2) {
        const uint8_t* row = p + (size_t)y * pitch;
        return (3 * row[j] + row[jn] + 1 + (x & 1)) >> 2;
    }
    const int r = y >> 1;
    const int rf = (y & 1) ? (r + 1 < chh ? r + 1 : r) : (r > 0 ? r - 1 : 0);
    const uint8_t* near = p + (size_t)r * pitch;
    const uint8_t* far = p + (size_t)rf * pitch;
    const int cur = 3 * near[j] + far[j], nb = 3 * near[jn] + far[jn];
    return (3 * cur + nb + 8 - (x & 1)) >> 4;
}

struct Rgb12 { unsigned a, b, c; };

// grid (pixels / 1024, image): the image's output is ONE run of H * W * 3 bytes (the pitch is 3 W), so a thread takes 4
// consecutive pixels of that run -- across a row end if need be -- and stores them as three aligned 32-bit words
__global__ __launch_bounds__(256) void jpeg_color_kernel(const uint8_t* __restrict__ coef, size_t coef_bytes, uint8_t* __restrict__ tmp,
                                                         uint8_t* __restrict__ rgb, JpegChunk ch) {
    const JpegImg& d = ch.d[blockIdx.y];
    JpegView v;
    if (!jpeg_view(coef, coef_bytes, d, tmp, v)) return;
    const unsigned npix = (unsigned)d.H * (unsigned)d.W;
    const unsigned p0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (p0 >= npix) return;
    const int W = d.W, H = d.H;
    int y = (int)(p0 / (unsigned)W), x = (int)(p0 - (unsigned)y * (unsigned)W);
    const int cnt = npix - p0 < 4u ? (int)(npix - p0) : 4;
    const int py = v.bw[0] * 8;
    const int pc = v.ncomp == 3 ? v.bw[1] * 8 : 0;
    const int cw = v.h2 ? (W + 1) >> 1 : W, chh = v.v2 ? (H + 1) >> 1 : H;
    unsigned char o[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < cnt) {
            const int Y = v.plane[0][(size_t)y * py + x];
            int r = Y, g = Y, b = Y;
            if (v.ncomp == 3) {
                const int cb = chroma_at(v.plane[1], pc, y, x, cw, chh, v.h2, v.v2) - 128;
                const int cr = chroma_at(v.plane[2], pc, y, x, cw, chh, v.h2, v.v2) - 128;
                r = clamp255(Y + ((91881 * cr + 32768) >> 16));
                g = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
                b = clamp255(Y + ((116130 * cb + 32768) >> 16));
            }
            o[3 * i] = (unsigned char)r; o[3 * i + 1] = (unsigned char)g; o[3 * i + 2] = (unsigned char)b;
            if (++x == W) { x = 0; ++y; }
        } else {
            o[3 * i] = o[3 * i + 1] = o[3 * i + 2] = 0;
        }
    }
    uint8_t* dst = rgb + d.rgb_off + (size_t)p0 * 3;
    if (cnt == 4) {
        Rgb12 pk;
        pk.a = o[0] | (o[1] << 8) | (o[2] << 16) | ((unsigned)o[3] << 24);
        pk.b = o[4] | (o[5] << 8) | (o[6] << 16) | ((unsigned)o[7] << 24);
        pk.c = o[8] | (o[9] << 8) | (o[10] << 16) | ((unsigned)o[11] << 24);
        *(Rgb12*)dst = pk;
    } else {
        for (int i = 0; i < 3 * cnt; ++i) dst[i] = o[i];
    }
}

}  // namespace

hipError_t launch_jpeg_reconstruct(const uint8_t* coef, size_t coef_bytes, const JpegImg* imgs, int n, uint8_t* tmp, uint8_t* rgb,
                                   hipStream_t s) {
    for (int lo = 0; lo < n; lo += JPEG_CHUNK) {
        const int nc = n - lo < JPEG_CHUNK ? n - lo : JPEG_CHUNK;
        JpegChunk ch{};
        size_t max_blocks = 1, max_pix = 1;
        for (int i = 0; i < nc; ++i) {
            ch.d[i] = imgs[lo + i];
            const size_t blocks = jpeg_plane_bytes_bound(ch.d[i].H, ch.d[i].W) / 64, pix = (size_t)ch.d[i].H * ch.d[i].W;
            if (blocks > max_blocks) max_blocks = blocks;
            if (pix > max_pix) max_pix = pix;
        }
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS), nc), dim3(256), 0, s, coef,
                           coef_bytes, tmp, ch);
        hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_pix + 1023) / 1024), nc), dim3(256), 0, s, coef, coef_bytes, tmp, rgb,
                           ch);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
