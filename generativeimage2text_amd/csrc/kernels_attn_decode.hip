// Decode attention on the matrix cores (bf16): one new text position per beam row against
// [image K/V shared by all beams of a sentence | that beam's text K/V] -- BertSelfAttention for the appended row
// (modeling_bert.py:41-47, 122-159) with the image rows' K/V cached once per image.
//
// The image part is the bulk (197 keys at 224 px, 1182 for 6 video frames) and identical for every beam, so it runs as
// two tiny MFMA products per 32-key step,  S = Q K^T  (16 beam rows x 32 keys, K = 64 dims)  and  O += P V  (16 rows x
// 64 dims, K = 32 keys), with the softmax in between in registers.  The scalar formulation this replaces spent
// ~1500 VALU instructions per wave on dot products and shuffles: 6.6 of its 8.9 us per launch were arithmetic, not
// memory (profiles/r02_a_decode_kernel_ablation.txt, dbg1).
//
// Cache layouts (written once per generate by kv_repack_frag_kernel), per (image, head), keys padded to 32 with zeros:
//   K  : fragment-major [key tile of 16][dim step of 32][lane][8]: a wave's K operand of one MFMA is ONE contiguous
//        1-KiB read (lane = (dim%32)/8*16 + key%16 holds 8 consecutive dims of its key);
//   V^T: [key step of 32][dim tile of 16][lane][8], lane = lg*16 + dim%16; the 8 contraction slots of lane group lg hold
//        keys  32s + lg*4 + {0,1,2,3}  and  32s + 16 + lg*4 + {0,1,2,3}  -- exactly the 8 scores that lane already holds
//        in the accumulators of the two S tiles of the step, so P goes from the S accumulators into the P V operand
//        WITHOUT any cross-lane movement or LDS round trip.
// A workgroup serves two heads with two waves each; a wave keeps (max, sum, O) per beam row for its half of the keys.
// The text keys differ per beam (histories are re-ordered by index, kv_src) and are few (<= max_text_len): they keep the
// 8-lanes-per-key scalar path and are folded into the wave's partial before the two halves are combined.
#include "gitmi_common.h"
#include "launchers.h"
#include "dgemm_shared.h"      // before the pragma below: its functions keep the default contraction (the chain GEMMs' arithmetic)
#include <algorithm>
#include <type_traits>

// Every fused multiply-add of the softmax bookkeeping is written out (fmaf): with contraction left to the compiler the
// a*b + c*d updates fuse differently per instantiation, and results must not depend on the packing or the kernel form.
// File scope: the shared per-pair functions and both kernels are covered.
#pragma clang fp contract(off)

namespace gitmi {

static constexpr int HD = 64;

// grid = (key steps, H, B); block = 256.  qkv: prefill layout [B*N, 3d] (q|k|v); one workgroup repacks the K and V of
// one (image, head, 32-key step).
__global__ __launch_bounds__(256) void kv_repack_frag_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kf,
                                                             bf16_t* __restrict__ vt, int N, int Np, int H, int d) {
    __shared__ bf16_t vs[32][HD + 8];          // the step's V tile [key][dim], padded rows
    const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int nsteps = Np >> 5;
    bf16_t* kdst = kf + ((size_t)b * H + h) * Np * HD;
    bf16_t* vdst = vt + ((size_t)b * H + h) * Np * HD;
    // 32 keys x 64 dims = 256 chunks of 8: thread -> (key, chunk)
    const int key = tid >> 3, ch = tid & 7;
    const int n = s * 32 + key;
    u32x4_t kv = {0u, 0u, 0u, 0u}, vv = kv;
    if (n < N) {
        const bf16_t* src = qkv + ((size_t)b * N + n) * 3 * d + d + h * HD + ch * 8;
        kv = *reinterpret_cast<const u32x4_t*>(src);
        vv = *reinterpret_cast<const u32x4_t*>(src + d);
    }
    // K: fragment-major, rows = keys, 2 dim steps: element (key n, dim c*8..) -> tile n/16, step c/4, lane (c%4)*16 + n%16
    *reinterpret_cast<u32x4_t*>(kdst + frag_tile(n >> 4, ch >> 2, 2, (ch & 3) * 16 + (n & 15))) = kv;
    *reinterpret_cast<u32x4_t*>(&vs[key][ch * 8]) = vv;
    __syncthreads();
    // V^T: 4 dim tiles x 64 lanes chunks of 8 keys (permuted slots, see header): thread -> (dim tile, lane)
    const int dt = tid >> 6, lane = tid & 63, lg = lane >> 4, dim = dt * 16 + (lane & 15);
    bf16_t o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = vs[(e >> 2) * 16 + lg * 4 + (e & 3)][dim];
    u32x4_t ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = (uint32_t)o[2 * e] | ((uint32_t)o[2 * e + 1] << 16);
    *reinterpret_cast<u32x4_t*>(vdst + (((size_t)s * 4 + dt) * 64 + lane) * 8) = ov;
}

__device__ __forceinline__ void unpack8(const u32x4_t& r, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unpack2op(r[i], v[2 * i], v[2 * i + 1]);
    }
}
__device__ __forceinline__ void ld8bf(const bf16_t* p, float (&v)[8]) { unpack8(*reinterpret_cast<const u32x4_t*>(p), v); }

// ---- the arithmetic of one (sentence, head) pair, written ONCE for both kernels ---------------------------------------
// The register kernel and the streaming kernel below differ in how pairs map to waves, where the K/V operands of the MFMAs
// come from and which barriers their form needs; everything a wave COMPUTES for a pair is in these functions, so the two
// cannot drift apart (gitmi_set_shared_device's promise of identical results rests on it).  A pair is shared by `ngrp`
// eight-lane groups (8 per wave); t = thread of the pair, grp = t / 8, sub = t % 8.
constexpr int ACS = 4;          // key steps per chunk and wave

struct Pair {
    int h, row0;       // head; first beam row of the sentence
    bool on;           // false: a packed workgroup's pair past the last one (the wave runs along on zeros, writes nothing)
};

// Where the new position's q | k | v of the pair's beam rows are, this head's 64 columns of each: the rows the QKV GEMM wrote
// (qkv_rows), or the workgroup's LDS rows in the form that projects them itself (attn_decode_qkv_kernel)
struct QkvSrc {
    const bf16_t* q0;          // q of beam row 0
    int row_stride, part;      // elements between beam rows, and from q to k and from k to v
    __device__ __forceinline__ const bf16_t* q(int j) const { return q0 + (size_t)j * row_stride; }
    __device__ __forceinline__ const bf16_t* k(int j) const { return q(j) + part; }
    __device__ __forceinline__ const bf16_t* v(int j) const { return q(j) + 2 * part; }
};
__device__ __forceinline__ QkvSrc qkv_rows(const AttnDecodeArgs& a, const Pair& p) {
    return QkvSrc{reinterpret_cast<const bf16_t*>(a.qkv) + (size_t)p.row0 * (3 * a.d) + p.h * HD, 3 * a.d, a.d};
}

// K / V of text item (beam j, position s), this lane's 8 dims: the new position from the QKV rows, earlier ones from the
// text cache through the beam indirection
template <int KB>
__device__ __forceinline__ void load_text_kv(const AttnDecodeArgs& a, const Pair& p, const QkvSrc& qs, int j, int s, int sub, u32x4_t& kr, u32x4_t& vr) {
    if (s == a.pos) {
        kr = *reinterpret_cast<const u32x4_t*>(qs.k(j) + sub * 8);
        vr = *reinterpret_cast<const u32x4_t*>(qs.v(j) + sub * 8);
    } else {
        // one beam: histories are never re-ordered, the cache row is the row itself (no dependent index load)
        const int srow = KB == 1 ? p.row0 : a.kv_src[(size_t)(p.row0 + j) * a.ld_src + s];
        const size_t off = ((size_t)srow * a.T_max + s) * a.d + p.h * HD + sub * 8;
        kr = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const bf16_t*>(a.txt_k) + off);
        vr = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const bf16_t*>(a.txt_v) + off);
    }
}

// the first TI text items of every group, requested up front (item = beam * (pos + 1) + position)
template <int KB, int TI>
struct TextItems {
    int j[TI];                  // beam of item u, -1: none
    u32x4_t kr[TI], vr[TI];
    __device__ __forceinline__ void load(const AttnDecodeArgs& a, const Pair& p, const QkvSrc& qs, int grp, int ngrp, int sub) {
        const int nt = a.pos + 1;
#pragma unroll
        for (int u = 0; u < TI; ++u) {
            const int it = grp + ngrp * u;
            j[u] = (p.on && it < a.beams * nt) ? it / nt : -1;
            const int s = it < a.beams * nt ? it % nt : 0;
            kr[u] = u32x4_t{0u, 0u, 0u, 0u};
            vr[u] = kr[u];
            if (j[u] >= 0) load_text_kv<KB>(a, p, qs, j[u], s, sub, kr[u], vr[u]);
        }
    }
};

// append this position's K/V of every beam to the text cache (16-byte copies by the first beams*8 threads of the pair)
__device__ __forceinline__ void append_text_cache(const AttnDecodeArgs& a, const Pair& p, const QkvSrc& qs, int t, int sub) {
    if (p.on && t < a.beams * 8) {
        const int j = t >> 3;
        const size_t dst = ((size_t)(p.row0 + j) * a.T_max + a.pos) * a.d + p.h * HD + sub * 8;
        *reinterpret_cast<u32x4_t*>(reinterpret_cast<bf16_t*>(a.txt_k) + dst) = *reinterpret_cast<const u32x4_t*>(qs.k(j) + sub * 8);
        *reinterpret_cast<u32x4_t*>(reinterpret_cast<bf16_t*>(a.txt_v) + dst) = *reinterpret_cast<const u32x4_t*>(qs.v(j) + sub * 8);
    }
}

// Q operand of the S MFMAs: lane (row = l15, lg) holds dims ds*32 + lg*8 .. +8 of beam row l15, pre-scaled by 1/8 (exact in bf16)
__device__ __forceinline__ void load_q_frag(const AttnDecodeArgs& a, const Pair& p, const QkvSrc& qs, int l15, int lg, bf16x8_t (&qf)[2]) {
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
        float qv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (p.on && l15 < a.beams)
            ld8bf(qs.q(l15) + ds * 32 + lg * 8, qv);
        u32x4_t t;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = pack2bf(qv[2 * e] * a.scale, qv[2 * e + 1] * a.scale);
        qf[ds] = __builtin_bit_cast(bf16x8_t, t);
    }
}

// running softmax of beam row l15 over the wave's image keys: max, (per-lane partial) sum, O accumulators of the P V MFMAs
struct ImagePartial {
    float m, l;
    f32x4_t o[4];
    __device__ __forceinline__ void init() {
        m = -INFINITY;
        l = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    // the two score tiles of key step s (lane (row l15, lg) holds keys 32s + t*16 + lg*4 + r): masks padded keys / steps and
    // folds the rest into the lane's maximum over the chunk
    __device__ __forceinline__ static void mask_max(f32x4_t (&sc)[2], int s, int nimg_steps, int n_img, int lg, float& cm) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (s * 32 + t * 16 + lg * 4 + r >= n_img || s >= nimg_steps) sc[t][r] = -INFINITY;   // padded keys / steps
                cm = fmaxf(cm, sc[t][r]);
            }
    }
    // the row's new max after a chunk with per-lane max cm; every chunk but the first rescales what is accumulated.  Returns
    // the max the chunk's exponentials are taken against.
    __device__ __forceinline__ float new_max(float cm, bool rescale) {
        cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
        cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
        const float mn = fmaxf(m, cm);                     // the chunk's first step holds >= 1 real key: mn is finite
        if (rescale) {
            const float al = fast_exp(m - mn);
            l *= al;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) { o[dt][0] *= al; o[dt][1] *= al; o[dt][2] *= al; o[dt][3] *= al; }
        }
        m = mn;
        return mn;
    }
    // one key step: its 8 exponentials into the sum, and as the P operand of the step's P V MFMAs
    __device__ __forceinline__ bf16x8_t p_frag(const f32x4_t (&sc)[2], float mn) {
        float p[8];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[t * 4 + r] = fast_exp(sc[t][r] - mn);    // exp(-inf) = 0 for padded keys
                l += p[t * 4 + r];
            }
        u32x4_t pp;
#pragma unroll
        for (int e = 0; e < 4; ++e) pp[e] = pack2bf(p[2 * e], p[2 * e + 1]);
        return __builtin_bit_cast(bf16x8_t, pp);
    }
    // after the last chunk: the row's sum over the four lane groups
    __device__ __forceinline__ void finish() {
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
    }
    // to the wave's LDS slot [beam]: o[64], m, l.  Lane (row l15 < beams, lg) holds dims dt*16 + lg*4 + r
    template <int KB>
    __device__ __forceinline__ void publish(float (&slot)[KB][HD + 2], int k, int l15, int lg) const {
        if (l15 < k) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) slot[l15][dt * 16 + lg * 4 + r] = o[dt][r];
            if (lg == 0) { slot[l15][HD] = m; slot[l15][HD + 1] = l; }
        }
    }
};

// text keys (beam-specific): 8 lanes per key, online update per beam row; this lane's 8 dims of q (pre-scaled) and o
template <int KB>
struct TextPartial {
    float q[KB][8], m[KB], l[KB], o[KB][8];
    __device__ __forceinline__ void init(const AttnDecodeArgs& a, const Pair& p, const QkvSrc& qs, int sub) {
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            m[j] = -INFINITY;
            l[j] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { q[j][e] = 0.f; o[j][e] = 0.f; }
            if (p.on && j < a.beams) {
                ld8bf(qs.q(j) + sub * 8, q[j]);
#pragma unroll
                for (int e = 0; e < 8; ++e) q[j][e] *= a.scale;
            }
        }
    }
    // one key of beam jj (uniform within the 8-lane group)
    __device__ __forceinline__ void item(int jj, const u32x4_t& kr, const u32x4_t& vr) {
        float kv[8], vv[8];
        unpack8(kr, kv);
        unpack8(vr, vv);
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (j == jj) {
                float sv = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) sv = fmaf(q[j][e], kv[e], sv);
                sv += __shfl_xor(sv, 1, 64);
                sv += __shfl_xor(sv, 2, 64);
                sv += __shfl_xor(sv, 4, 64);                // all 8 lanes of the group hold the 64-dim dot product
                const float mn = fmaxf(m[j], sv);
                const float al = fast_exp(m[j] - mn);
                const float pe = fast_exp(sv - mn);
                l[j] = fmaf(l[j], al, pe);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[j][e] = fmaf(o[j][e], al, pe * vv[e]);
                m[j] = mn;
            }
        }
    }
    template <int TI>
    __device__ __forceinline__ void items(const TextItems<KB, TI>& ti, bool enabled) {
#pragma unroll
        for (int u = 0; u < TI; ++u) {
            if (ti.j[u] >= 0 && enabled) item(ti.j[u], ti.kr[u], ti.vr[u]);
        }
    }
    // long texts: the items past the TI up-front ones, on a dependent-load path
    template <int TI>
    __device__ __forceinline__ void tail(const AttnDecodeArgs& a, const Pair& p, const QkvSrc& qs, int grp, int ngrp, int sub) {
        if (!p.on) return;
        const int nt = a.pos + 1;
        for (int it = grp + ngrp * TI; it < a.beams * nt; it += ngrp) {
            u32x4_t kr, vr;
            load_text_kv<KB>(a, p, qs, it / nt, it % nt, sub, kr, vr);
            item(it / nt, kr, vr);
        }
    }
    // merge the 8 groups of the wave (lanes with equal `sub`): lanes 0..7 end up with the wave's text partial (m, l, o[8])
    __device__ __forceinline__ void merge_groups() {
#pragma unroll
        for (int j = 0; j < KB; ++j) {
#pragma unroll
            for (int off = 8; off < 64; off <<= 1) {
                const float m2 = __shfl_xor(m[j], off, 64);
                const float l2 = __shfl_xor(l[j], off, 64);
                const float mn = fmaxf(m[j], m2);
                const float a1 = m[j] == -INFINITY ? 0.f : fast_exp(m[j] - mn);
                const float a2 = m2 == -INFINITY ? 0.f : fast_exp(m2 - mn);
                l[j] = fmaf(l[j], a1, l2 * a2);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float o2 = __shfl_xor(o[j][e], off, 64);
                    o[j][e] = fmaf(o[j][e], a1, o2 * a2);
                }
                m[j] = mn;
            }
        }
    }
    // fold the wave's text partial into its published image partial (lanes 0..7, one beam row at a time; text part: lanes
    // 0..7 hold dims sub*8 + e of row j)
    __device__ __forceinline__ void fold_into(float (&slot)[KB][HD + 2], int k, int lane, int sub) const {
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            if (lane < 8 && j < k) {
                const float mi = slot[j][HD], li = slot[j][HD + 1];
                const float mn = fmaxf(mi, m[j]);
                const float a1 = mi == -INFINITY ? 0.f : fast_exp(mi - mn);
                const float a2 = m[j] == -INFINITY ? 0.f : fast_exp(m[j] - mn);
#pragma unroll
                for (int e = 0; e < 8; ++e) slot[j][sub * 8 + e] = fmaf(slot[j][sub * 8 + e], a1, o[j][e] * a2);
                if (sub == 0) { slot[j][HD] = mn; slot[j][HD + 1] = fmaf(li, a1, l[j] * a2); }
            }
        }
    }
};

__device__ __forceinline__ void store_out(const AttnDecodeArgs& a, int row, int col, float r) {
    bf16_t* O = reinterpret_cast<bf16_t*>(a.out);
    if (a.out_frag) O[frag_offset(row, col, a.d >> 5)] = f2bf(r);
    else O[(size_t)row * a.d + col] = f2bf(r);
}
// the pair's output rows from ONE partial per row (one wave per pair); nthr threads of the pair, this is thread t
template <int KB>
__device__ __forceinline__ void write_rows(const AttnDecodeArgs& a, const Pair& p, const float (&s0)[KB][HD + 2], int t, int nthr) {
    if (!p.on) return;
    for (int i = t; i < a.beams * HD; i += nthr) {
        const int j = i / HD, dd = i % HD;
        const float r1 = s0[j][dd] / s0[j][HD + 1];
        store_out(a, p.row0 + j, p.h * HD + dd, r1);
    }
}
// ... from the partials of the two waves that split the pair's key steps
template <int KB>
__device__ __forceinline__ void write_rows(const AttnDecodeArgs& a, const Pair& p, const float (&s0)[KB][HD + 2],
                                           const float (&s1)[KB][HD + 2], int t, int nthr) {
    if (!p.on) return;
    for (int i = t; i < a.beams * HD; i += nthr) {
        const int j = i / HD, dd = i % HD;
        const float m0 = s0[j][HD], m1 = s1[j][HD];
        const float mm = fmaxf(m0, m1);
        const float a0 = m0 == -INFINITY ? 0.f : fast_exp(m0 - mm);
        const float a1 = m1 == -INFINITY ? 0.f : fast_exp(m1 - mm);
        const float num = fmaf(a0, s0[j][dd], a1 * s1[j][dd]);
        const float den = fmaf(a0, s0[j][HD + 1], a1 * s1[j][HD + 1]);
        const float r = num / den;
        store_out(a, p.row0 + j, p.h * HD + dd, r);
    }
}

// grid = (H, sentences); block = 128 = the 2 waves of one head (768 workgroups at B = 64: three per CU, evenly -- pairing
// two heads per workgroup left half the CUs with twice the K/V to ingest).  The two waves split the key steps (even / odd)
// and its text items; each wave requests ALL of its image K/V fragments (up to 4 steps = 32 sixteen-byte loads per
// lane) in its first instructions, computes every score tile, does ONE max / exp pass and then the P V products; the two
// halves meet once in LDS.  KB >= beams (1, 2, 4 or 8); TI: text items per 8-lane group loaded up front.
//
// PW: (sentence, head) pairs per workgroup (a wave needs 214 registers, so 8 waves fill a CU).  1 spreads a launch over
// every CU (fastest on an idle device); next to the image encoder of another context every CU that holds even one of
// these waves is closed to a GEMM workgroup (8 waves x 232 registers, 128 KiB LDS) until the wave retires, so the launcher
// packs the one-wave kernel (launch_attn_decode_mfma).
// NH: waves per pair.  2 = the two waves of a head split its key steps (one memory round trip each); 1 = ONE wave walks
// all key steps in chunks of ACS (two round trips at 197 image keys): half the resident waves for ~1.3x the time.
// RAGGED: a.ntok gives every image's keys (a separate instantiation: the uniform ones are the kernels as they were)
template <int KB, int TI = 3, int PW = 1, int NH = 2, bool RAGGED = false>
__global__ __launch_bounds__(64 * NH * PW) void attn_decode_mfma_kernel(AttnDecodeArgs a) {
    __shared__ float part[PW][NH][KB][HD + 2];    // [pair][half][beam]: o[64], m, l
    constexpr int PT = 64 * NH;                   // threads of a pair

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int hp = wave / NH, half = wave % NH;    // pair of the workgroup, half of the head's keys
    const int H = a.d / HD;
    const int k = a.beams;                       // k <= KB <= 8 < 16 MFMA rows
    const int Np = a.N_pad, nsteps = Np >> 5;
    // PW == 1 keeps the (head, sentence) grid of the two-wave kernel; packed workgroups: the last one's pairs may not exist
    const int pair = NH == 2 ? (int)(blockIdx.y * H + blockIdx.x) : (int)blockIdx.x * PW + hp;
    Pair p;
    p.on = PW == 1 || pair < a.n_pairs;
    p.h = p.on ? pair % H : 0;
    const int b = p.on ? pair / H : 0;
    p.row0 = b * k;
    const int bi = a.img_of ? a.img_of[b] : b;   // sentence -> image (several questions per image)
    const bf16_t* Kf = reinterpret_cast<const bf16_t*>(a.img_k) + ((size_t)bi * H + p.h) * Np * HD;
    const bf16_t* Vt = reinterpret_cast<const bf16_t*>(a.img_v) + ((size_t)bi * H + p.h) * Np * HD;
    // ragged batches: the image's own keys; its 32-key steps past them are skipped (N_pad stays the row stride)
    const int n_img = RAGGED ? a.ntok[bi] : a.N_img;
    const int nimg_steps = (!p.on || (a.dbg & 1)) ? 0 : RAGGED ? (n_img + 31) >> 5 : nsteps;

    // ---- image K/V of a chunk of key steps: requested before anything else (the longest latency) ---------------
    bf16x8_t kq[ACS][2][2], vq[ACS][4];
    auto load_chunk = [&](int s0) {                               // steps s0, s0 + NH, ... (this half's parity)
#pragma unroll
        for (int c = 0; c < ACS; ++c) {
            const int s = s0 + NH * c;
            const bool on = s < nimg_steps && !(a.dbg & 8);
            const bf16_t* kp = Kf + frag_tile(2 * s, 0, 2, lane);              // the step's 4 KiB of K, then of V^T: contiguous
            const bf16_t* vp = Vt + ((size_t)s * 4 * 64 + lane) * 8;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int ds = 0; ds < 2; ++ds) {
                    const bf16x8_t* q = reinterpret_cast<const bf16x8_t*>(kp + (t * 2 + ds) * 512);
                    kq[c][t][ds] = !on ? bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0} : (a.dbg & 16) ? *q : __builtin_nontemporal_load(q);
                }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8_t* q = reinterpret_cast<const bf16x8_t*>(vp + dt * 512);
                vq[c][dt] = !on ? bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0} : (a.dbg & 16) ? *q : __builtin_nontemporal_load(q);
            }
        }
    };
    load_chunk(half);

    // ---- text items (the 8 * NH eight-lane groups of the pair share them), text-cache append, Q operand -------------
    const int t = tid % PT, grp = t >> 3, sub = tid & 7;
    const QkvSrc qs = qkv_rows(a, p);
    TextItems<KB, TI> ti;
    ti.load(a, p, qs, grp, 8 * NH, sub);
    append_text_cache(a, p, qs, t, sub);
    bf16x8_t qf[2];
    load_q_frag(a, p, qs, l15, lg, qf);

    // ---- image part on the matrix cores -------------------------------------------------------------------------
    ImagePartial ip;
    ip.init();
    for (int s0 = half; s0 < nimg_steps; s0 += NH * ACS) {
        if (s0 != half) load_chunk(s0);                    // later chunks (long image sequences: video, VQA resolutions)
        f32x4_t sc[ACS][2];                                // every score tile of the chunk
        float cm = -INFINITY;
#pragma unroll
        for (int c = 0; c < ACS; ++c) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                sc[c][u] = mfma16(kq[c][u][0], qf[0], f32x4_t{0.f, 0.f, 0.f, 0.f});
                sc[c][u] = mfma16(kq[c][u][1], qf[1], sc[c][u]);
            }
            ip.mask_max(sc[c], s0 + NH * c, nimg_steps, RAGGED ? n_img : a.N_img, lg, cm);
        }
        const float mn = ip.new_max(cm, s0 != half);
#pragma unroll
        for (int c = 0; c < ACS; ++c) {
            const bf16x8_t pf = ip.p_frag(sc[c], mn);
            if (a.dbg & 4) {      // timing experiment: no P V product
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) asm volatile("" ::"v"(vq[c][dt]));
                asm volatile("" ::"v"(pf));
                continue;
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) ip.o[dt] = mfma16(vq[c][dt], pf, ip.o[dt]);
        }
    }
    ip.finish();
    // ---- text keys ------------------------------------------------------------------------------------------------
    TextPartial<KB> tp;
    tp.init(a, p, qs, sub);
    tp.items(ti, !(a.dbg & 2));
    tp.template tail<TI>(a, p, qs, grp, 8 * NH, sub);
    tp.merge_groups();
    // ---- this wave's partial per beam row = its image keys + its text items, through LDS ----------------------------
    ip.publish(part[hp][half], k, l15, lg);
    // NH == 1: a wave reads back only what it wrote itself (LDS operations of a wave complete in order): no workgroup barrier
    if constexpr (NH > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    tp.fold_into(part[hp][half], k, lane, sub);
    if constexpr (NH > 1) __syncthreads(); else __builtin_amdgcn_wave_barrier();
    if constexpr (NH == 1) write_rows(a, p, part[hp][0], t, PT);
    else write_rows(a, p, part[hp][0], part[hp][NH - 1], t, PT);
}

// ---- the 8-pair one-wave form with the QKV projection inside ---------------------------------------------------------
// attn_decode_mfma_kernel<1, TI, 8, 1> preceded, in the same launch, by the part of the QKV GEMM its pairs need.  A
// (sentence, head) pair reads 192 of the 3 d projected columns of one row -- q, k and v of its head -- and while its first
// image K/V chunk is on its way (~8 us) the wave has nothing to do.  So a workgroup takes 8 consecutive SENTENCES of ONE head
// (the packed form above takes 8 consecutive pairs: 8 heads of one sentence); its 8 waves request their pairs' image K, then
// compute the 8 rows x 192 columns together -- 12 weight strips x 4 K slices, wave w the slice w % 4 of strips 6 (w / 4) .. + 5
// -- exchange partials and results through LDS, and go on as the form above, with q | k | v of the row coming from LDS
// instead of the QKV GEMM's output.  One launch per layer less, and no launch boundary between the two.
// Arithmetic: the projected values are the bits of dgemm_kernel<4, 4, DEPI_BF16> because this kernel calls the same code
// (dgemm_shared.h): k_slice over 4 slices, mfma_slice with the weights as first operand, sum_waves in slice order,
// DGEMM_CONSUMER_FINISH under the default contraction, pack2bf.  A row's result does not depend on the rows sharing its MFMA
// tile, so computing a 16-row tile for 8 of its rows changes nothing.  The head's 295 KB of weights are read by its
// ceil(B / 8) workgroups: the map from blockIdx to (head, sentence block) keeps them on one blockIdx % 8 residue (one XCD's L2
// where workgroups are dealt round-robin) -- performance only, any placement gives the same results.
// Image V^T of the first chunk is requested AFTER the projection's MFMAs: the K and V^T chunks are 64 registers each, the
// activation slice 24 and two weight strips in flight 48, of 256 (the kernel takes 204); K alone keeps the CU's HBM stream
// busy for longer than the projection takes.  The weight strips are read by CACHEABLE loads (load_w_slice<false>): the head's
// other workgroups read them again from the L2 (21.8 us per launch; 23.3 with the chain GEMMs' non-temporal loads, which is what
// QKV launch + attention took as two launches: docs/LAB_NOTEBOOK.md, profiles/r14_attn_qkv_*).
constexpr int AQ_PW = 8;                     // pairs = waves = sentences of a workgroup
constexpr int AQ_STRIPS = 3 * HD / 16;       // weight strips of one head: 4 each of q, k and v

// workgroup-local barrier that orders LDS traffic only: __syncthreads() also waits for every global load in flight (vmcnt(0)),
// here the image K/V chunk the projection is meant to overlap
__device__ __forceinline__ void attn_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int TI>
__global__ __launch_bounds__(64 * AQ_PW) void attn_decode_qkv_kernel(AttnDecodeArgs a) {
    constexpr int KB = 1;
    __shared__ __attribute__((aligned(16))) f32x4_t red[AQ_STRIPS][4][1][64];     // [strip][K slice][row tile][lane]
    __shared__ __attribute__((aligned(16))) bf16_t rows[AQ_PW][3 * HD];           // q | k | v of the 8 sentences, this head
    __shared__ float part[AQ_PW][KB][HD + 2];                                     // [pair][beam]: o[64], m, l

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int H = a.d / HD, B = a.n_pairs / H;
    const int Np = a.N_pad, nsteps = Np >> 5;
    // (head, sentence block) of this workgroup: the launch has 8 * per workgroups, residue r = blockIdx % 8 takes the `per`
    // consecutive (head-major) blocks from r * per
    const int nsb = (B + AQ_PW - 1) / AQ_PW, total = H * nsb, per = (total + 7) >> 3;
    const int blk = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (blk >= total) return;                      // whole workgroup: before any barrier
    const int b0 = (blk % nsb) * AQ_PW;
    Pair p;
    p.h = blk / nsb;
    p.on = b0 + wave < B;
    const int b = p.on ? b0 + wave : 0;
    p.row0 = b;
    const int bi = a.img_of ? a.img_of[b] : b;
    const bf16_t* Kf = reinterpret_cast<const bf16_t*>(a.img_k) + ((size_t)bi * H + p.h) * Np * HD;
    const bf16_t* Vt = reinterpret_cast<const bf16_t*>(a.img_v) + ((size_t)bi * H + p.h) * Np * HD;
    const int nimg_steps = p.on ? nsteps : 0;

    // ---- image K / V^T of a chunk of key steps (the loads of attn_decode_mfma_kernel's load_chunk, K and V^T apart) -------
    bf16x8_t kq[ACS][2][2], vq[ACS][4];
    auto load_k = [&](int s0) {
#pragma unroll
        for (int c = 0; c < ACS; ++c) {
            const bool on = s0 + c < nimg_steps;
            const bf16_t* kp = Kf + frag_tile(2 * (s0 + c), 0, 2, lane);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int ds = 0; ds < 2; ++ds)
                    kq[c][t][ds] = !on ? bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0}
                                       : __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(kp + (t * 2 + ds) * 512));
        }
    };
    auto load_v = [&](int s0) {
#pragma unroll
        for (int c = 0; c < ACS; ++c) {
            const bool on = s0 + c < nimg_steps;
            const bf16_t* vp = Vt + ((size_t)(s0 + c) * 4 * 64 + lane) * 8;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                vq[c][dt] = !on ? bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0}
                                : __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(vp + dt * 512));
        }
    };
    load_k(0);

    // ---- q | k | v of the workgroup's 8 rows x 192 columns --------------------------------------------------------------
    const int ksteps = a.d >> 5, N = 3 * a.d;
    const int slice = wave & 3;
    const KSlice ks = k_slice(ksteps, 4, slice);
    const int rt = b0 >> 4;                                    // the 8 sentences are rows (b0 & 15) .. + 7 of row tile rt
    auto strip_of = [&](int ls) { return (ls >> 2) * (a.d >> 4) + p.h * 4 + (ls & 3); };     // head-local strip -> strip of the 3 d columns
    bf16x8_t xf[DW_KS][1];
    load_x_slice(xf, reinterpret_cast<const bf16_t*>(a.x), rt, ks, ksteps, lane);
#pragma unroll 2
    for (int u = 0; u < AQ_STRIPS / 2; ++u) {
        const int ls = (wave >> 2) * (AQ_STRIPS / 2) + u;
        const WSlice wf = load_w_slice<false>(reinterpret_cast<const bf16_t*>(a.w), strip_of(ls), ks, ksteps, lane);
        f32x4_t acc[1] = {f32x4_t{0.f, 0.f, 0.f, 0.f}};
        mfma_slice(acc, wf, xf, ks);
        red[ls][slice][0][lane] = acc[0];
    }
    load_v(0);
    // wave w finishes strips w and w + 8: its lane (l15, lg) row l15 of the tile, columns lg * 4 .. + 3 of the strip
    const int fm_raw = rt * 16 + l15;
    const int fm = fm_raw < a.M ? fm_raw : a.M - 1;
    const bool second = wave + AQ_PW < AQ_STRIPS;
    const int fn0 = strip_of(wave) * 16 + lg * 4, fn1 = strip_of(second ? wave + AQ_PW : wave) * 16 + lg * 4;
    RowStatLoads sl;
    if (a.stats_in) stats_issue(sl, a.stats_in, a.strips_in, a.M, fm, lg);
    const float4 bias4[2] = {load_cols4(a.bias, fn0, N), load_cols4(a.bias, fn1, N)};
    float4 cs4[2] = {float4{0.f, 0.f, 0.f, 0.f}, float4{0.f, 0.f, 0.f, 0.f}};
    if (a.stats_in) { cs4[0] = load_cols4(a.colsum, fn0, N); cs4[1] = load_cols4(a.colsum, fn1, N); }
    attn_lds_barrier();
    {
#pragma clang fp contract(fast)                    // the chain GEMMs' epilogue, under the contraction they are built with
        float mean = 0.f, rstd = 1.f;
        if (a.stats_in) stats_finish(sl, a.inv_d, a.eps_in, mean, rstd);
        const int i = l15 - (b0 & 15);             // sentence of the workgroup this lane's row is (outside 0..7: another block's)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (t == 1 && !second) break;
            const int ls = wave + t * AQ_PW;
            const f32x4_t tot = sum_waves<4>(red[ls], 0, lane);
            DGEMM_CONSUMER_FINISH(v, tot, bias4[t], cs4[t], a.stats_in, mean, rstd, GITMI_ACT_NONE);
            if (i >= 0 && i < AQ_PW) {
                uint2 o;
                o.x = pack2bf(v[0], v[1]);
                o.y = pack2bf(v[2], v[3]);
                *reinterpret_cast<uint2*>(&rows[i][ls * 16 + lg * 4]) = o;
            }
        }
    }
    attn_lds_barrier();
    const QkvSrc qs{rows[wave], 0, HD};

    // ---- from here on: attn_decode_mfma_kernel<1, TI, 8, 1> --------------------------------------------------------------
    const int grp = lane >> 3, sub = lane & 7;
    TextItems<KB, TI> ti;
    ti.load(a, p, qs, grp, 8, sub);
    append_text_cache(a, p, qs, lane, sub);
    bf16x8_t qf[2];
    load_q_frag(a, p, qs, l15, lg, qf);

    ImagePartial ip;
    ip.init();
    for (int s0 = 0; s0 < nimg_steps; s0 += ACS) {
        if (s0 != 0) { load_k(s0); load_v(s0); }
        f32x4_t sc[ACS][2];
        float cm = -INFINITY;
#pragma unroll
        for (int c = 0; c < ACS; ++c) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                sc[c][u] = mfma16(kq[c][u][0], qf[0], f32x4_t{0.f, 0.f, 0.f, 0.f});
                sc[c][u] = mfma16(kq[c][u][1], qf[1], sc[c][u]);
            }
            ip.mask_max(sc[c], s0 + c, nimg_steps, a.N_img, lg, cm);
        }
        const float mn = ip.new_max(cm, s0 != 0);
#pragma unroll
        for (int c = 0; c < ACS; ++c) {
            const bf16x8_t pf = ip.p_frag(sc[c], mn);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) ip.o[dt] = mfma16(vq[c][dt], pf, ip.o[dt]);
        }
    }
    ip.finish();
    TextPartial<KB> tp;
    tp.init(a, p, qs, sub);
    tp.items(ti, true);
    tp.template tail<TI>(a, p, qs, grp, 8, sub);
    tp.merge_groups();
    ip.publish(part[wave], a.beams, l15, lg);
    __builtin_amdgcn_wave_barrier();       // a wave reads back only what it wrote itself (its LDS operations complete in order)
    tp.fold_into(part[wave], a.beams, lane, sub);
    __builtin_amdgcn_wave_barrier();
    write_rows(a, p, part[wave], lane, 64);
}

// ---- streaming form of the one-wave kernel -----------------------------------------------------------------------
// The kernels above keep a pair's K/V chunk in REGISTERS (128 of a wave's 215): a wave can only ask for its next chunk when
// the registers are free, so every pair costs two exposed memory round trips and a CU never has more than its resident
// waves' chunks in flight -- 24 GB/s per CU, 96 CUs for 17.8 us per launch, while every one of those CUs is closed to the
// image encoder's GEMM workgroups.  Here the K/V of a wave's pairs STREAM through an LDS ring: 4-KiB slots (the K or the
// V^T of one 32-key step -- contiguous in the cache layouts above) are fetched by LDS-DMA (global_load_lds, lane-linear:
// the fragment-major layout lands so that lane l's operand of fragment f is the 16 bytes at f * 1 KiB + l * 16) in exactly
// the order the wave consumes them,
//        pair 0: K0 K1 K2 K3 | V0 V1 V2 V3 | K4 K5 K6 | V4 V5 V6      pair 1: ...
// RING slots ahead of the consumer, across chunk AND pair boundaries: the stream never drains between pairs, text keys,
// merge and output of one pair are worked off while the next pair's slots land.  A wave holds ~100 registers instead of
// 215, a workgroup is 4 waves x RING x 4 KiB of LDS = one per CU.
// The arithmetic is the one-wave kernel's because it is the same code: both kernels call the per-pair functions above
// (TextItems, ImagePartial, TextPartial, write_rows; same chunks of ACS key steps, same max / rescale order), so the
// two agree BIT FOR BIT over whole decodes: the engine selects between them by policy (engine.hip: streaming for a
// context alone with >= 384 (sentence, head) pairs and <= 256 padded keys, the register form otherwise), and
// gitmi_set_shared_device's promise of identical results rests on it.  Guards: tests/test_gpu_ops.py (streaming == register
// kernel on the unit entry) and tests/test_gpu_policy.py::test_shared_device_policy_is_bitwise_neutral (features, ids and
// log-probs of the benchmark geometry under both policies, bf16 / f16 / f32 builds).
// Ordering rules (MI355X_MICROARCH.md, LDS-DMA): a ds_read sees a DMA's bytes only after the issuing wave's counted vmcnt
// -- loads complete in order, so `vmcnt(4 * slots issued after this one)` retires the slot (other vector-memory operations
// issued in between only make that wait stricter); a slot is refilled only after the ds_reads that emptied it have
// returned (lgkmcnt(0)).  Rings are private to a wave: no workgroup barrier anywhere.
typedef __attribute__((address_space(3))) void attn_lds_void_t;

template <int N> __device__ __forceinline__ void attn_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// younger slots still in flight are allowed to stay in flight: 4 LDS-DMA instructions per slot
__device__ __forceinline__ void attn_wait_slots_ahead(int ahead) {
    switch (ahead) {
        case 0: attn_wait_vm<0>(); break;
        case 1: attn_wait_vm<4>(); break;
        case 2: attn_wait_vm<8>(); break;
        case 3: attn_wait_vm<12>(); break;
        case 4: attn_wait_vm<16>(); break;
        case 5: attn_wait_vm<20>(); break;
        case 6: attn_wait_vm<24>(); break;
        case 7: attn_wait_vm<28>(); break;
        case 8: attn_wait_vm<32>(); break;
        case 9: attn_wait_vm<36>(); break;
        case 10: attn_wait_vm<40>(); break;
        default: attn_wait_vm<44>(); break;       // ahead >= 11: waiting for fewer outstanding operations is always safe
    }
}

constexpr int AS_WAVES = 4;                    // waves (independent streams) per workgroup
constexpr int AS_SLOT = 4096;                  // bytes: K or V^T of one 32-key step of one (image, head)

template <int KB, int TI, int RING>
__global__ __launch_bounds__(64 * AS_WAVES) void attn_decode_stream_kernel(AttnDecodeArgs a) {
    static_assert(RING >= 2 && RING <= 12, "ring depth");
    __shared__ __attribute__((aligned(16))) unsigned char ring_mem[AS_WAVES][RING * AS_SLOT];
    __shared__ float part[AS_WAVES][KB][HD + 2];   // [wave][beam]: o[64], m, l

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int H = a.d / HD;
    const int k = a.beams;
    const int Np = a.N_pad, nsteps = Np >> 5;
    unsigned char* ring = ring_mem[wave];

    // pairs of this wave: w, w + W, w + 2W, ...  (W = waves of the launch)
    const int W = (int)gridDim.x * AS_WAVES, w0 = (int)blockIdx.x * AS_WAVES + wave;
    const int npw = w0 < a.n_pairs ? (a.n_pairs - 1 - w0) / W + 1 : 0;
    const int slots_per_pair = 2 * nsteps;
    const int total_slots = npw * slots_per_pair;

    // ---- producer: the next slot of the stream -> ring position issued % RING.  All state is wave-uniform.
    int issued = 0;                      // slots requested so far
    int p_ord = 0, p_s0 = 0, p_v = 0, p_c = 0;     // pair ordinal, chunk start step, 0 = K / 1 = V^T, step within the chunk
    const bf16_t* p_K = nullptr; const bf16_t* p_V = nullptr;
    auto producer_pair = [&]() {
        const int pair = w0 + p_ord * W;
        const int h = pair % H, b = pair / H;
        const int bi = a.img_of ? a.img_of[b] : b;
        p_K = reinterpret_cast<const bf16_t*>(a.img_k) + ((size_t)bi * H + h) * Np * HD;
        p_V = reinterpret_cast<const bf16_t*>(a.img_v) + ((size_t)bi * H + h) * Np * HD;
    };
    if (npw > 0) producer_pair();
    auto issue_slot = [&]() {
        if (issued >= total_slots) return;
        const bf16_t* src = (p_v ? p_V : p_K) + (size_t)(p_s0 + p_c) * (AS_SLOT / 2) + lane * 8;
        unsigned char* dst = ring + (issued % RING) * AS_SLOT;
#pragma unroll
        for (int f = 0; f < 4; ++f)
            __builtin_amdgcn_global_load_lds((const void*)(src + f * 512), (attn_lds_void_t*)(dst + f * 1024), 16, 0, 2);   // aux 2 = nt
        ++issued;
        const int nsc = min(ACS, nsteps - p_s0);
        if (++p_c == nsc) {
            p_c = 0;
            if (p_v == 0) p_v = 1;
            else {
                p_v = 0; p_s0 += ACS;
                if (p_s0 >= nsteps) { p_s0 = 0; ++p_ord; if (p_ord < npw) producer_pair(); }
            }
        }
    };
    for (int i = 0; i < RING; ++i) issue_slot();

    int consumed = 0;                    // slots read out of the ring so far
    // wait for the oldest unread slot, return its ring address
    auto slot_ready = [&]() -> const unsigned char* {
        const int ahead = issued - consumed - 1;
        if (ahead == RING - 1) attn_wait_vm<4 * (RING - 1)>();        // steady state
        else attn_wait_slots_ahead(ahead);
        return ring + (consumed % RING) * AS_SLOT;
    };
    // the slot's fragments are in registers (the caller has used them): free it and keep the stream RING slots ahead
    auto slot_done = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        ++consumed;
        issue_slot();
    };


    for (int ord = 0; ord < npw; ++ord) {
        const int pair = w0 + ord * W;
        const Pair p{pair % H, (pair / H) * k, true};

        // ---- text items (the 8 eight-lane groups of the wave share them), text-cache append, Q operand -------------
        const int grp = lane >> 3, sub = lane & 7;
        const QkvSrc qs = qkv_rows(a, p);
        TextItems<KB, TI> ti;
        ti.load(a, p, qs, grp, 8, sub);
        append_text_cache(a, p, qs, lane, sub);
        bf16x8_t qf[2];
        load_q_frag(a, p, qs, l15, lg, qf);

        // ---- image part on the matrix cores: operands from the ring ------------------------------------------------
        ImagePartial ip;
        ip.init();
        for (int s0 = 0; s0 < nsteps; s0 += ACS) {
            f32x4_t sc[ACS][2];
            float cm = -INFINITY;
#pragma unroll
            for (int c = 0; c < ACS; ++c) {
                if (s0 + c < nsteps) {                                         // wave-uniform
                    const unsigned char* sl = slot_ready();
                    bf16x8_t kq[2][2];
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int ds = 0; ds < 2; ++ds)
                            kq[t][ds] = *reinterpret_cast<const bf16x8_t*>(sl + (t * 2 + ds) * 1024 + lane * 16);
                    __builtin_amdgcn_sched_barrier(0);       // all four ds_reads in flight before the first MFMA waits for one
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        sc[c][t] = mfma16(kq[t][0], qf[0], f32x4_t{0.f, 0.f, 0.f, 0.f});
                        sc[c][t] = mfma16(kq[t][1], qf[1], sc[c][t]);
                    }
                    slot_done();
                } else {
                    sc[c][0] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                    sc[c][1] = sc[c][0];
                }
                ip.mask_max(sc[c], s0 + c, nsteps, a.N_img, lg, cm);
            }
            const float mn = ip.new_max(cm, s0 != 0);
#pragma unroll
            for (int c = 0; c < ACS; ++c) {
                const bf16x8_t pf = ip.p_frag(sc[c], mn);
                if (s0 + c < nsteps) {
                    const unsigned char* sl = slot_ready();
                    bf16x8_t vq[4];
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) vq[dt] = *reinterpret_cast<const bf16x8_t*>(sl + dt * 1024 + lane * 16);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) ip.o[dt] = mfma16(vq[dt], pf, ip.o[dt]);
                    slot_done();
                } else {
                    // the register kernel multiplies an all-zero V^T step by P = 0 here: adds +0 to every accumulator
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) ip.o[dt] = mfma16(bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0}, pf, ip.o[dt]);
                }
            }
        }
        ip.finish();
        // ---- text keys, then the wave's partial per beam row = image keys + text items, through its own LDS slot -------
        TextPartial<KB> tp;
        tp.init(a, p, qs, sub);
        tp.items(ti, true);
        tp.template tail<TI>(a, p, qs, grp, 8, sub);
        tp.merge_groups();
        ip.publish(part[wave], k, l15, lg);
        __builtin_amdgcn_wave_barrier();       // a wave reads back only what it wrote itself (its LDS operations complete in order)
        tp.fold_into(part[wave], k, lane, sub);
        __builtin_amdgcn_wave_barrier();
        write_rows(a, p, part[wave], lane, 64);
        __builtin_amdgcn_wave_barrier();       // the next pair reuses this wave's LDS slot
    }
}

// ---- host launchers ------------------------------------------------------------------
hipError_t launch_kv_repack_frag(const void* qkv, void* kf, void* vt, int B, int N, int N_pad, int H, int d, hipStream_t s) {
    if (B <= 0 || N <= 0) return hipSuccess;
    if (N_pad % 32 || N_pad < N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kv_repack_frag_kernel, dim3(N_pad / 32, H, B), dim3(256), 0, s, (const bf16_t*)qkv, (bf16_t*)kf,
                       (bf16_t*)vt, N, N_pad, H, d);
    return hipGetLastError();
}

// beams -> KB, the kernels' compile-time beam rows (1, 2, 4 or 8): f gets it as a std::integral_constant
template <typename F>
static void with_beam_rows(int beams, F&& f) {
    if (beams <= 1) f(std::integral_constant<int, 1>{});
    else if (beams <= 2) f(std::integral_constant<int, 2>{});
    else if (beams <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

int attn_decode_pairs_per_wg(const AttnDecodeArgs& a, int B, int H) {
    int pw = a.pairs_per_wg >= 8 ? 8 : a.pairs_per_wg >= 4 || a.pairs_per_wg <= 0 ? 4 : a.pairs_per_wg >= 2 ? 2 : 1;
    while (pw > 1 && B * H / pw < 96) pw >>= 1;
    if (a.beams > 4 && pw == 8) pw = 4;         // 8 beams: 269 registers, one wave per SIMD: 4 pairs fill a CU
    return pw;
}

bool attn_decode_qkv_form(const AttnDecodeArgs& a, int B, int H) {
    if (B <= 0 || a.beams != 1 || a.waves_per_pair == 2 || a.ntok || a.stream_wgs != 0 || a.dbg) return false;
    if (a.N_img < 1 || a.N_pad % 32 || a.N_pad < a.N_img || a.N_pad > 8 * 32) return false;
    if (a.d != H * HD || a.d > 4 * DW_KS * 32 || a.M < B) return false;           // K = d: whole k-steps, a wave's slice in registers
    if (!a.x || !a.w || !a.bias) return false;
    return !a.stats_in || (a.colsum && a.strips_in >= 1 && a.strips_in <= 4 * STRIP_SLOTS);
}

hipError_t launch_attn_decode_qkv(const AttnDecodeArgs& a, int B, int H, hipStream_t s) {
    if (!attn_decode_qkv_form(a, B, H)) return hipErrorInvalidValue;
    AttnDecodeArgs p = a;
    p.n_pairs = B * H;
    const int total = H * ((B + AQ_PW - 1) / AQ_PW);          // (head, block of 8 sentences) per workgroup; the kernel's map
    hipLaunchKernelGGL((attn_decode_qkv_kernel<3>), dim3(8 * ((total + 7) / 8)), dim3(64 * AQ_PW), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_attn_decode_mfma(const AttnDecodeArgs& a, int B, int H, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (a.beams > 8 || a.N_pad % 32 || a.N_pad < a.N_img || a.N_img < 1) return hipErrorInvalidValue;
    if (a.ntok && a.stream_wgs > 0) return hipErrorInvalidValue;      // ragged batches: the register kernels only
    AttnDecodeArgs p = a;
    p.n_pairs = B * H;
    // Which kernel: the GEOMETRY decides, so a model has ONE attention arithmetic (the two kernels differ in the last bits:
    // one partial per row instead of two).
    //  * ONE wave per (sentence, head) pair when the image keys fit two chunks (<= 8 key steps: one 224-pixel image).  Against
    //    two waves per pair it is 1.9 us slower per launch on an idle device (two memory round trips instead of one) and
    //    keeps half as many 214-register waves resident: +1.3 % captions/s in the mixed schedule, where every CU that holds
    //    one of these waves is closed to the image encoder's GEMM workgroups (profiles/r03_v_bench_lines.txt).
    //  * TWO waves per pair for long key sequences (6 video frames, a 480 x 640 VQA image: 37 steps would be 10 round trips
    //    in one wave, 5 in two; GIT_BASE_VATEX bs = 16: 1.78k captions/s with one wave, 1.90k with two).
    // waves_per_pair 1 / 2 (GITMI_ATTN_NH) force one of them for A/B.
    if (a.stream_wgs > 0) {
        // streaming kernel (the solo policy's choice, engine.hip; also the unit entry): workgroups = min(stream_wgs, pairs / 4)
        const int nwg = std::max(1, std::min(a.stream_wgs, (p.n_pairs + AS_WAVES - 1) / AS_WAVES));
        with_beam_rows(a.beams, [&](auto kb) {
            constexpr int KB = decltype(kb)::value;
            hipLaunchKernelGGL((attn_decode_stream_kernel<KB, 3, KB == 8 ? 8 : 9>), dim3(nwg), dim3(64 * AS_WAVES), 0, s, p);
        });
        return hipGetLastError();
    }
    const bool one_wave = a.waves_per_pair == 1 || (a.waves_per_pair != 2 && a.N_pad <= 8 * 32);
    if (a.ntok || !one_wave) {     // ragged batches: the two-wave kernel whatever the geometry (the VQA capacity grids choose it anyway)
        with_beam_rows(a.beams, [&](auto kb) {
            constexpr int KB = decltype(kb)::value;
            if (a.ntok) hipLaunchKernelGGL((attn_decode_mfma_kernel<KB, 3, 1, 2, true>), dim3(H, B), dim3(128), 0, s, p);
            else hipLaunchKernelGGL((attn_decode_mfma_kernel<KB>), dim3(H, B), dim3(128), 0, s, p);
        });
        return hipGetLastError();
    }
    // pairs per workgroup (same per-wave arithmetic whatever the packing): 4 by default, 8 = a full CU under the serving
    // policy (10.58k -> 10.67k captions/s in the mixed schedule, +11 us per decode step alone; profiles/r03_y_*) -- but
    // never fewer than 96 workgroups: a small batch packed onto a handful of CUs streams its K/V through too few of them
    const int pw = attn_decode_pairs_per_wg(a, B, H);
    with_beam_rows(a.beams, [&](auto kb) {
        constexpr int KB = decltype(kb)::value;
        auto packed = [&](auto pwc) {
            constexpr int PW = decltype(pwc)::value;
            hipLaunchKernelGGL((attn_decode_mfma_kernel<KB, 3, PW, 1>), dim3((p.n_pairs + PW - 1) / PW), dim3(64 * PW), 0, s, p);
        };
        if (pw == 8) { if constexpr (KB < 8) packed(std::integral_constant<int, 8>{}); }
        else if (pw == 4) packed(std::integral_constant<int, 4>{});
        else if (pw == 2) packed(std::integral_constant<int, 2>{});
        else packed(std::integral_constant<int, 1>{});
    });
    return hipGetLastError();
}

}  // namespace gitmi
