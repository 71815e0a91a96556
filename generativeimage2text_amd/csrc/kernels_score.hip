// Caption scoring (GITMI_SEARCH_SCORE): the textual head run once over whole token sequences, as
// CaptioningModel.forward_one_ce does (decoder.py:916-972), with the vocabulary head reduced to the two numbers per
// position the reference's losses need -- lp = log_softmax(z)[target] and mean_lp = mean_c log_softmax(z)[c].
//
// Rows of the text pass: sentence q, position j -> row q * Lp + j (Lp = the call's longest sentence rounded up to 16).
//   score_embed_ln_kernel  WordAndPositionalEmbedding + LayerNorm (decoder.py:41-90) of every position of every row
//   score_attn_mfma_kernel text-row attention of one decoder layer (16-bit modes; score_attn_kernel: the fp32 form of the
//                          f32 parity mode): the image K/V of the sentence's image (prefill layout, [B * N_img, 3d] packed
//                          q|k|v rows), then the sentence's own text keys, causal
//   score_head_kernel      logits tile on the matrix cores; the epilogue keeps (max, sum exp, sum (z - max)) per
//                          (row, 128-column tile) and z at the row's target column -- the logits never reach HBM
//   score_rowstats_kernel  the same statistics from materialised fp32 logits (f32 parity mode)
//   score_combine_kernel   tiles -> (lp, mean_lp) per position, non-finite flags per sentence
// Attention maps (GITMI_SEARCH_ATTEND): the two attention kernels also write the softmax statistics (m, l) of every (sentence,
// head, text row); score_attn_map_mfma_kernel / score_attn_map_kernel recompute S per key chunk and write the head mean of
// exp(s - m) / l.  Score calls instantiate the attention kernels without the statistics store: their results are what they were.
// Token trees (GITMI_SEARCH_TREE_SCORE): the rows are the nodes of trees in DFS pre-order.  tree_structure_kernel turns the
// caller's depths into (parent, end) tables and rejects a malformed tree; the embedding and the two attention kernels have a
// third instantiation (position = depth; the causal predicate becomes "ancestor or self", key blocks with no live key are
// skipped); the head keeps its per-row tiles and tree_gather_*_kernel / tree_combine_kernel add the logit of every child's token
// at its parent's row.  The score and attend instantiations compile to what they were.
#include "gitmi_common.h"
#include "launchers.h"

#include <math.h>

namespace gitmi {

// ---- embedding + LayerNorm of every text position --------------------------------------------------------------
// tokens int64 [Q][ld]; positions j >= ld are padding id 0 (text attention is causal: they change nothing before them)
// TREE (GITMI_SEARCH_TREE_SCORE): row = node; its token id and position (= depth) come from the node tables
// tree_structure_kernel wrote, already clamped -- `tokens` is not read.
template <typename TOut, bool TREE>
__global__ __launch_bounds__(256) void score_embed_ln_kernel(const long long* __restrict__ tokens, int ld, int Lp,
                                                             const float* __restrict__ words,
                                                             const float* __restrict__ positions,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             float* __restrict__ h_f, TOut* __restrict__ h_t, int D,
                                                             int vocab, int max_pos, const int* __restrict__ node_tok,
                                                             const int* __restrict__ node_depth) {
    __shared__ float s_part[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    int tok, pos;
    if constexpr (TREE) {
        tok = node_tok[row];
        pos = node_depth[row];
    } else {
        const int q = row / Lp, j = row - q * Lp;
        long long t = j < ld ? tokens[(size_t)q * ld + j] : 0;
        tok = t < 0 ? 0 : (t >= vocab ? vocab - 1 : (int)t);
        pos = j < max_pos ? j : max_pos - 1;
    }
    const int c = tid * 4;
    const bool on = c < D;
    f32x4_t a = {0.f, 0.f, 0.f, 0.f}, g4 = a, b4 = a;
    if (on) {
        const f32x4_t w4 = *reinterpret_cast<const f32x4_t*>(words + (size_t)tok * D + c);
        const f32x4_t p4 = *reinterpret_cast<const f32x4_t*>(positions + (size_t)pos * D + c);
        g4 = *reinterpret_cast<const f32x4_t*>(gamma + c);
        b4 = *reinterpret_cast<const f32x4_t*>(beta + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = w4[r] + p4[r];
    }
    const float sum = wave_sum(a[0] + a[1] + a[2] + a[3]);
    if (lane == 0) s_part[wave] = sum;
    __syncthreads();
    const float mean = (s_part[0] + s_part[1] + s_part[2] + s_part[3]) / (float)D;
    float sq = 0.f;
    if (on) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float dv = a[r] - mean; sq += dv * dv; }
    }
    sq = wave_sum(sq);
    if (lane == 0) s_part[4 + wave] = sq;
    __syncthreads();
    const float rstd = rsqrtf((s_part[4] + s_part[5] + s_part[6] + s_part[7]) / (float)D + eps);
    if (on) {
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (a[r] - mean) * rstd * g4[r] + b4[r];
        *reinterpret_cast<f32x4_t*>(h_f + (size_t)row * D + c) = f32x4_t{o[0], o[1], o[2], o[3]};
        if constexpr (sizeof(TOut) == 4) {
            *reinterpret_cast<f32x4_t*>(h_t + (size_t)row * D + c) = f32x4_t{o[0], o[1], o[2], o[3]};
        } else {
            uint2 u;
            u.x = pack2bf(o[0], o[1]);
            u.y = pack2bf(o[2], o[3]);
            *reinterpret_cast<uint2*>(h_t + (size_t)row * D + c) = u;
        }
    }
}

hipError_t launch_score_embed_ln(const long long* tokens, int ld, int Q, int Lp, const float* words, const float* positions,
                                 const float* gamma, const float* beta, float eps, float* h_f, void* h_t, bool t_is_f32,
                                 int D, int vocab, int max_pos, hipStream_t s, const TreeNodes* tree) {
    if (D > 1024 || (D & 3) || Q < 1 || Lp < 1 || max_pos < 1) return hipErrorInvalidValue;
    const dim3 grid(Q * Lp), block(256);
    const int *ntk = tree ? tree->tok : nullptr, *ndp = tree ? tree->depth : nullptr;
    auto go = [&](auto kernel, auto* ht) {
        hipLaunchKernelGGL(kernel, grid, block, 0, s, tokens, ld, Lp, words, positions, gamma, beta, eps, h_f, ht, D, vocab, max_pos,
                           ntk, ndp);
    };
    if (t_is_f32) {
        if (tree) go(score_embed_ln_kernel<float, true>, (float*)h_t);
        else go(score_embed_ln_kernel<float, false>, (float*)h_t);
    } else {
        if (tree) go(score_embed_ln_kernel<bf16_t, true>, (bf16_t*)h_t);
        else go(score_embed_ln_kernel<bf16_t, false>, (bf16_t*)h_t);
    }
    return hipGetLastError();
}

// sums / maxima over the 16 lanes that share lane / 16 (one row of an MFMA 16x16 output fragment)
__device__ __forceinline__ float xor16_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float xor16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- text attention ------------------------------------------------------------------------------------------------
// One wave per (sentence, head, 64-query tile); lane = query position.  Keys and values pass through LDS in chunks of
// SA_KC rows (fp32), every lane reads the same LDS row (broadcast): scores and P V are 64 fused multiply-adds per key
// and lane with the query and the output accumulator in registers.  Online softmax in fp32 over sub-chunks of 16 keys.
constexpr int SA_KC = 64;
__device__ __forceinline__ float ld_elem(const float* p) { return *p; }
__device__ __forceinline__ float ld_elem(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void ld8(const float* p, float* o) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[i] = a[i]; o[4 + i] = b[i]; }
}
__device__ __forceinline__ void ld8(const bf16_t* p, float* o) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    unpack2op(u.x, o[0], o[1]);
    unpack2op(u.y, o[2], o[3]);
    unpack2op(u.z, o[4], o[5]);
    unpack2op(u.w, o[6], o[7]);
}

// Visibility of text key t for query row j.  Sentence: causal.  Tree (rows = nodes in DFS pre-order, end = first index past the
// key's subtree): the key is the query itself or one of its ancestors.
template <bool TREE>
__device__ __forceinline__ bool text_key_visible(int t, int j, int end) {
    if constexpr (TREE) return t <= j && j < end;
    else return t <= j;
}
// Tree rows: does any of the 32 text keys t0 .. t0 + 31 reach the query tile that starts at j0?  A key with end <= j0 has its
// whole subtree before the tile; one with end > j0 is visible to row j0 (t <= j0) or to itself (t > j0), so the test is exact.
// Lanes l and l + 32 ask for the same key: every wave of a workgroup gets the same answer without a barrier.
__device__ __forceinline__ bool tree_block_live(const int* __restrict__ end, int t0, int Lp, int j0, int lane) {
    const int t = t0 + (lane & 31);
    return __ballot(t < Lp && end[t] > j0) != 0;
}

// STATS: also stats[(q * H + h) * Lp + j] = (m, l), the row's score maximum and sum of exp(s - m) over its visible keys
// TREE: node_end [Q * Lp] (tree_structure_kernel) replaces the causal predicate; key chunks past the image with no live key are skipped
template <typename T, bool STATS, bool TREE>
__global__ __launch_bounds__(64) void score_attn_kernel(const T* __restrict__ qkv, const T* __restrict__ img_kv,
                                                        const int* __restrict__ image_of, T* __restrict__ out, int d,
                                                        int N_img, int Lp, float scale, const int* __restrict__ ntok,
                                                        float2* __restrict__ stats, const int* __restrict__ node_end) {
    __shared__ float sK[SA_KC][64];
    __shared__ float sV[SA_KC][64];
    __shared__ int sEnd[TREE ? SA_KC : 1];
    const int lane = threadIdx.x;
    const int q = blockIdx.x, h = blockIdx.y, j0 = blockIdx.z * 64;
    const int j = j0 + lane;
    const int ld3 = 3 * d;
    const size_t row_base = (size_t)q * Lp;
    const int jq = j < Lp ? j : Lp - 1;              // lanes past the sentence's rows compute a copy of the last row
    float qv[64], acc[64];
    {
        const T* qp = qkv + (row_base + jq) * ld3 + h * 64;
#pragma unroll
        for (int c = 0; c < 64; c += 8) {
            float t8[8];
            ld8(qp + c, t8);
#pragma unroll
            for (int i = 0; i < 8; ++i) qv[c + i] = t8[i] * scale;
        }
    }
#pragma unroll
    for (int c = 0; c < 64; ++c) acc[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int img = image_of[q];
    const int n_i = ntok ? ntok[img] : N_img;        // the image's keys (ragged batches); N_img = row stride of its block
    const int j_last = min(Lp, j0 + 64) - 1;         // the last text key any lane of the tile may see
    const int n_keys = n_i + j_last + 1;
    // staging: 8 lanes per key row (8 elements each), 8 rows per pass
    const int sr = lane >> 3, sc = (lane & 7) * 8;
    for (int k0 = 0; k0 < n_keys; k0 += SA_KC) {
        const int kc = min(SA_KC, n_keys - k0);
        if constexpr (TREE) {
            if (k0 >= n_i && !tree_block_live(node_end + row_base, k0 - n_i, Lp, j0, lane) &&
                !tree_block_live(node_end + row_base, k0 - n_i + 32, Lp, j0, lane))
                continue;
        }
        __syncthreads();
        if constexpr (TREE) {
            const int t = k0 + lane - n_i;                 // text keys of the chunk are below n_keys - n_i <= Lp
            sEnd[lane] = lane < kc && t >= 0 ? node_end[row_base + t] : 0;
        }
        for (int r = sr; r < kc; r += 8) {
            const int key = k0 + r;
            const T* src = key < n_i ? img_kv + ((size_t)img * N_img + key) * ld3
                                     : qkv + (row_base + (key - n_i)) * ld3;
            float t8[8];
            ld8(src + d + h * 64 + sc, t8);
#pragma unroll
            for (int i = 0; i < 8; ++i) sK[r][sc + i] = t8[i];
            ld8(src + 2 * d + h * 64 + sc, t8);
#pragma unroll
            for (int i = 0; i < 8; ++i) sV[r][sc + i] = t8[i];
        }
        __syncthreads();
        for (int u0 = 0; u0 < kc; u0 += 16) {
            float sv[16];
            float mx = m;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int r = u0 + u;
                const int key = k0 + r;
                float sdot = -INFINITY;
                if (r < kc && (key < n_i || text_key_visible<TREE>(key - n_i, jq, TREE ? sEnd[r] : 0))) {
                    sdot = 0.f;
#pragma unroll
                    for (int c = 0; c < 64; c += 4) {
                        const f32x4_t k4 = *reinterpret_cast<const f32x4_t*>(&sK[r][c]);
                        sdot = fmaf(qv[c], k4[0], sdot);
                        sdot = fmaf(qv[c + 1], k4[1], sdot);
                        sdot = fmaf(qv[c + 2], k4[2], sdot);
                        sdot = fmaf(qv[c + 3], k4[3], sdot);
                    }
                }
                sv[u] = sdot;
                mx = fmaxf(mx, sdot);
            }
            if (mx == -INFINITY) continue;           // nothing visible in this sub-chunk yet (cannot happen after key 0)
            const float corr = __expf(m - mx);
            l *= corr;
#pragma unroll
            for (int c = 0; c < 64; ++c) acc[c] *= corr;
            m = mx;
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const float p = __expf(sv[u] - mx);
                if (sv[u] == -INFINITY) continue;
                l += p;
                const int r = u0 + u;
#pragma unroll
                for (int c = 0; c < 64; c += 4) {
                    const f32x4_t v4 = *reinterpret_cast<const f32x4_t*>(&sV[r][c]);
                    acc[c] = fmaf(p, v4[0], acc[c]);
                    acc[c + 1] = fmaf(p, v4[1], acc[c + 1]);
                    acc[c + 2] = fmaf(p, v4[2], acc[c + 2]);
                    acc[c + 3] = fmaf(p, v4[3], acc[c + 3]);
                }
            }
        }
    }
    if (j >= Lp) return;
    if constexpr (STATS) stats[((size_t)q * gridDim.y + h) * Lp + j] = make_float2(m, l);
    const float inv = 1.0f / l;
    T* op = out + (row_base + j) * d + h * 64;
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int c = 0; c < 64; c += 4)
            *reinterpret_cast<f32x4_t*>(op + c) = f32x4_t{acc[c] * inv, acc[c + 1] * inv, acc[c + 2] * inv, acc[c + 3] * inv};
    } else {
#pragma unroll
        for (int c = 0; c < 64; c += 8) {
            uint4 u;
            u.x = pack2bf(acc[c] * inv, acc[c + 1] * inv);
            u.y = pack2bf(acc[c + 2] * inv, acc[c + 3] * inv);
            u.z = pack2bf(acc[c + 4] * inv, acc[c + 5] * inv);
            u.w = pack2bf(acc[c + 6] * inv, acc[c + 7] * inv);
            *reinterpret_cast<uint4*>(op + c) = u;
        }
    }
}

// 16-bit modes: the same attention on the matrix cores.  Workgroup = 4 waves for (sentence, head, 64-query tile), wave w
// owns the 16 queries j0 + 16 w ..; keys in blocks of 32 staged through LDS by the whole workgroup: K row-major (the B
// operand of S = Q K^T), V transposed (the B operand of O = P V).  S and O on mfma_f32_16x16x32 (fp32 accumulation),
// online softmax in fp32 on the S fragments (lane holds queries 4 (lane / 16) + i, key lane % 16), P rounded to the
// operand type and passed through a per-wave LDS tile into the A-operand layout.
constexpr int SM_KB = 32;                 // keys per block
constexpr int SM_KP = 64 + 8;             // padded LDS row of sK (elements)
constexpr int SM_VP = SM_KB + 8;          // padded LDS row of sVt / sP
// TREE: as in score_attn_kernel; the end[] of a key block is staged with its keys (0 for image keys, which need none).
template <bool STATS, bool TREE>
__global__ __launch_bounds__(256) void score_attn_mfma_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ img_kv,
                                                              const int* __restrict__ image_of, bf16_t* __restrict__ out,
                                                              int d, int N_img, int Lp, float scale,
                                                              const int* __restrict__ ntok, float2* __restrict__ stats,
                                                              const int* __restrict__ node_end) {
    __shared__ __attribute__((aligned(16))) bf16_t sK[SM_KB][SM_KP];
    __shared__ __attribute__((aligned(16))) bf16_t sVt[64][SM_VP];
    __shared__ __attribute__((aligned(16))) bf16_t sP[4][16][SM_VP];
    __shared__ int sEnd[TREE ? SM_KB : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x, h = blockIdx.y, j0 = blockIdx.z * 64;
    const int jw = j0 + wave * 16;                   // first query of this wave
    const int g = lane >> 4, c = lane & 15;
    const int ld3 = 3 * d;
    const size_t row_base = (size_t)q * Lp;
    const int img = image_of[q];
    const int n_i = ntok ? ntok[img] : N_img;        // the image's keys (ragged batches); N_img = row stride of its block
    const int j_last = min(Lp, j0 + 64) - 1;
    const int n_keys = n_i + j_last + 1;
    // Q fragments (A operand): row = query jw + c (clamped), dims kk * 32 + 8 g ..
    bf16x8_t qf[2];
    {
        const bf16_t* qp = qkv + (row_base + min(jw + c, Lp - 1)) * ld3 + h * 64 + 8 * g;
        qf[0] = *reinterpret_cast<const bf16x8_t*>(qp);
        qf[1] = *reinterpret_cast<const bf16x8_t*>(qp + 32);
    }
    f32x4_t acc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) acc[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] = -INFINITY; l[i] = 0.f; }
    const int sk = tid >> 3, sc = (tid & 7) * 8;     // staging: key sk of the block, dims sc .. sc + 8
    for (int k0 = 0; k0 < n_keys; k0 += SM_KB) {
        if constexpr (TREE) {
            if (k0 >= n_i && !tree_block_live(node_end + row_base, k0 - n_i, Lp, j0, lane)) continue;   // the same in every wave
        }
        __syncthreads();
        {
            const int key = k0 + sk;
            uint4 kv = make_uint4(0, 0, 0, 0), vv = kv;
            if (key < n_keys) {
                const bf16_t* src = key < n_i ? img_kv + ((size_t)img * N_img + key) * ld3 : qkv + (row_base + (key - n_i)) * ld3;
                kv = *reinterpret_cast<const uint4*>(src + d + h * 64 + sc);
                vv = *reinterpret_cast<const uint4*>(src + 2 * d + h * 64 + sc);
            }
            if constexpr (TREE) {
                if (sc == 0) sEnd[sk] = key >= n_i && key < n_keys ? node_end[row_base + (key - n_i)] : 0;
            }
            *reinterpret_cast<uint4*>(&sK[sk][sc]) = kv;
            const bf16_t* v8 = reinterpret_cast<const bf16_t*>(&vv);
#pragma unroll
            for (int e = 0; e < 8; ++e) sVt[sc + e][sk] = v8[e];
        }
        __syncthreads();
        f32x4_t sfr[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            sfr[blk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(&sK[blk * 16 + c][kk * 32 + 8 * g]);
                sfr[blk] = mfma16(qf[kk], b, sfr[blk]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = jw + 4 * g + i;                // query row of this lane's element i
            float x[2];
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int key = k0 + blk * 16 + c;
                const bool ok = key < n_keys && (key < n_i || text_key_visible<TREE>(key - n_i, j, TREE ? sEnd[blk * 16 + c] : 0));
                x[blk] = ok ? sfr[blk][i] * scale : -INFINITY;
            }
            const float mx = xor16_max(fmaxf(x[0], x[1]));
            const float mn = fmaxf(m[i], mx);
            const float corr = mn == -INFINITY ? 1.f : __expf(m[i] - mn);
            const float p0 = mn == -INFINITY ? 0.f : __expf(x[0] - mn);
            const float p1 = mn == -INFINITY ? 0.f : __expf(x[1] - mn);
            l[i] = l[i] * corr + xor16_sum(p0 + p1);
            m[i] = mn;
#pragma unroll
            for (int db = 0; db < 4; ++db) acc[db][i] *= corr;
            sP[wave][4 * g + i][c] = f2bf(p0);
            sP[wave][4 * g + i][16 + c] = f2bf(p1);
        }
        __syncthreads();
        const bf16x8_t pa = *reinterpret_cast<const bf16x8_t*>(&sP[wave][c][8 * g]);
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(&sVt[db * 16 + c][8 * g]);
            acc[db] = mfma16(pa, b, acc[db]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = jw + 4 * g + i;
        if (j >= Lp) continue;
        if constexpr (STATS)
            if (c == 0) stats[((size_t)q * gridDim.y + h) * Lp + j] = make_float2(m[i], l[i]);
        const float inv = 1.0f / l[i];
        bf16_t* op = out + (row_base + j) * d + h * 64 + c;
#pragma unroll
        for (int db = 0; db < 4; ++db) op[db * 16] = f2bf(acc[db][i] * inv);
    }
}

hipError_t launch_score_attn(const void* qkv, const void* img_kv, const int* image_of, void* out, int Q, int H, int d,
                             int N_img, int Lp, float scale, bool is_f32, hipStream_t s, const int* ntok, float2* stats,
                             const int* node_end) {
    if (d != H * 64 || Q < 1 || Lp < 1 || N_img < 1 || (stats && node_end)) return hipErrorInvalidValue;
    const dim3 grid(Q, H, (Lp + 63) / 64);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    if (is_f32) {
        const auto k = node_end ? score_attn_kernel<float, false, true>
                                : stats ? score_attn_kernel<float, true, false> : score_attn_kernel<float, false, false>;
        hipLaunchKernelGGL(k, grid, dim3(64), 0, s, (const float*)qkv, (const float*)img_kv, image_of, (float*)out, d, N_img, Lp,
                           scale, ntok, stats, node_end);
    } else {
        const auto k = node_end ? score_attn_mfma_kernel<false, true>
                                : stats ? score_attn_mfma_kernel<true, false> : score_attn_mfma_kernel<false, false>;
        hipLaunchKernelGGL(k, grid, dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)img_kv, image_of, (bf16_t*)out, d, N_img,
                           Lp, scale, ntok, stats, node_end);
    }
    return hipGetLastError();
}

// ---- attention maps ------------------------------------------------------------------------------------------------
// out[q][j][col] = (1 / H) sum_h exp(s_h(j, col) - m_h(j)) / l_h(j) for the text rows j < len_q of sentence q: columns
// [0, N_img) are the image keys of image_of[q] (0 past the image's own ntok rows), columns N_img + t its text keys (0 for
// t > j).  A workgroup owns (sentence, 16 text rows, AM_COLS columns) and loops over the heads with the head sum in
// registers: every element is written once, by one thread, in a fixed order of additions -- no atomics, and the value does
// not depend on the grid.  s is recomputed exactly as the attention kernel of the same mode computes it (the same MFMA
// sequence / the same fused multiply-add chain), so that m is the maximum of the very values exponentiated here.
// Rows j >= len_q and columns >= N_img + Tc are not written (the caller's buffer is zero-filled).
constexpr int AM_ROWS = 16, AM_COLS = 128;

// the key row behind an output column and whether it is a key of this sentence at all (clamped to a readable row if not)
template <typename T>
__device__ __forceinline__ const T* map_key_row(const T* qkv, const T* img_kv, size_t row_base, int img, int n_i, int N_img,
                                                int Lp, int ld3, int col, bool* live) {
    if (col < N_img) {
        *live = col < n_i;
        return img_kv + ((size_t)img * N_img + (*live ? col : 0)) * ld3;
    }
    const int t = col - N_img;
    *live = t < Lp;
    return qkv + (row_base + (*live ? t : 0)) * ld3;
}

// 16-bit modes.  4 waves; wave w owns columns col0 + 32 w .. + 32 as two 16-column MFMA blocks.  Q rows (A operand) and key
// rows (B operand) are loaded straight from global memory in operand order, 16 bytes per lane and fragment.
__global__ __launch_bounds__(256) void score_attn_map_mfma_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ img_kv,
                                                                  const int* __restrict__ image_of, const int* __restrict__ ntok,
                                                                  const float2* __restrict__ stats, const int* __restrict__ lens,
                                                                  float* __restrict__ out, size_t out_sq, size_t out_sj, int Tc,
                                                                  int H, int N_img, int Lp, float scale, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x, j0 = blockIdx.y * AM_ROWS, col0 = blockIdx.z * AM_COLS + wave * 32;
    const int g = lane >> 4, c = lane & 15;
    const int len = lens ? min(lens[q], Lp) : Lp;
    const int Kc = N_img + Tc;
    if (j0 >= len || col0 >= Kc) return;
    const int d = H * 64, ld3 = 3 * d;
    const size_t row_base = (size_t)q * Lp;
    const int img = image_of[q];
    const int n_i = ntok ? ntok[img] : N_img;
    const bf16_t* kp[2];
    bool live[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
        kp[blk] = map_key_row(qkv, img_kv, row_base, img, n_i, N_img, Lp, ld3, col0 + blk * 16 + c, &live[blk]) + d + 8 * g;
    const bf16_t* qp = qkv + (row_base + min(j0 + c, Lp - 1)) * ld3 + 8 * g;          // A operand: row = query j0 + c
    float acc[2][4];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[blk][i] = 0.f;
    for (int h = 0; h < H; ++h) {
        const bf16x8_t q0 = *reinterpret_cast<const bf16x8_t*>(qp + h * 64), q1 = *reinterpret_cast<const bf16x8_t*>(qp + h * 64 + 32);
        f32x4_t sfr[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(kp[blk] + h * 64);
            const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(kp[blk] + h * 64 + 32);
            sfr[blk] = mfma16(q0, b0, f32x4_t{0.f, 0.f, 0.f, 0.f});
            sfr[blk] = mfma16(q1, b1, sfr[blk]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = j0 + 4 * g + i;                                              // query row of this lane's element i
            const float2 ml = stats[((size_t)q * H + h) * Lp + min(j, Lp - 1)];
            const float inv = 1.0f / ml.y;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const int col = col0 + blk * 16 + c;
                const bool ok = live[blk] && (col < N_img || col - N_img <= j);
                if (ok) acc[blk][i] += __expf(sfr[blk][i] * scale - ml.x) * inv;
            }
        }
    }
    const float invH = 1.0f / (float)H;
    bool nonfinite = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = j0 + 4 * g + i;
        if (j >= len) continue;
        float* op = out + (size_t)q * out_sq + (size_t)j * out_sj;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int col = col0 + blk * 16 + c;
            if (col >= Kc) continue;
            const float v = acc[blk][i] * invH;
            op[col] = v;
            nonfinite = nonfinite || !isfinite(v);
        }
    }
    if (nonfinite && bad) bad[q] = 1;
}

// f32 mode.  Thread = one column, its key row of the head in registers; the 16 query rows of the head (scaled, as the
// attention kernel scales them) and their statistics in LDS, read by every thread at the same address (broadcast).
__global__ __launch_bounds__(AM_COLS) void score_attn_map_kernel(const float* __restrict__ qkv, const float* __restrict__ img_kv,
                                                                 const int* __restrict__ image_of, const int* __restrict__ ntok,
                                                                 const float2* __restrict__ stats, const int* __restrict__ lens,
                                                                 float* __restrict__ out, size_t out_sq, size_t out_sj, int Tc,
                                                                 int H, int N_img, int Lp, float scale, int* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) float sQ[AM_ROWS][64];
    __shared__ float2 sMl[AM_ROWS];
    const int tid = threadIdx.x;
    const int q = blockIdx.x, j0 = blockIdx.y * AM_ROWS, col = blockIdx.z * AM_COLS + tid;
    const int len = lens ? min(lens[q], Lp) : Lp;
    const int Kc = N_img + Tc;
    if (j0 >= len) return;                                                             // the whole workgroup
    const int d = H * 64, ld3 = 3 * d;
    const size_t row_base = (size_t)q * Lp;
    const int img = image_of[q];
    const int n_i = ntok ? ntok[img] : N_img;
    bool live;
    const float* kp = map_key_row(qkv, img_kv, row_base, img, n_i, N_img, Lp, ld3, min(col, Kc - 1), &live) + d;
    live = live && col < Kc;
    const int sr = tid >> 3, sc = (tid & 7) * 8;                                       // staging: row sr, dims sc .. sc + 8
    float acc[AM_ROWS];
#pragma unroll
    for (int r = 0; r < AM_ROWS; ++r) acc[r] = 0.f;
    for (int h = 0; h < H; ++h) {
        __syncthreads();
        {
            float t8[8];
            ld8(qkv + (row_base + min(j0 + sr, Lp - 1)) * ld3 + h * 64 + sc, t8);
#pragma unroll
            for (int i = 0; i < 8; ++i) sQ[sr][sc + i] = t8[i] * scale;
            if (tid < AM_ROWS) {
                const float2 ml = stats[((size_t)q * H + h) * Lp + min(j0 + tid, Lp - 1)];
                sMl[tid] = make_float2(ml.x, 1.0f / ml.y);
            }
        }
        __syncthreads();
        float kv[64];
#pragma unroll
        for (int c = 0; c < 64; c += 8) ld8(kp + h * 64 + c, &kv[c]);
#pragma unroll 4
        for (int r = 0; r < AM_ROWS; ++r) {
            float sdot = 0.f;
#pragma unroll
            for (int c = 0; c < 64; c += 4) {
                const f32x4_t q4 = *reinterpret_cast<const f32x4_t*>(&sQ[r][c]);
                sdot = fmaf(q4[0], kv[c], sdot);
                sdot = fmaf(q4[1], kv[c + 1], sdot);
                sdot = fmaf(q4[2], kv[c + 2], sdot);
                sdot = fmaf(q4[3], kv[c + 3], sdot);
            }
            const bool ok = live && (col < N_img || col - N_img <= j0 + r);
            if (ok) acc[r] += __expf(sdot - sMl[r].x) * sMl[r].y;
        }
    }
    if (col >= Kc) return;
    const float invH = 1.0f / (float)H;
    bool nonfinite = false;
#pragma unroll
    for (int r = 0; r < AM_ROWS; ++r) {
        const int j = j0 + r;
        if (j >= len) break;
        const float v = acc[r] * invH;
        out[(size_t)q * out_sq + (size_t)j * out_sj + col] = v;
        nonfinite = nonfinite || !isfinite(v);
    }
    if (nonfinite && bad) bad[q] = 1;
}

hipError_t launch_score_attn_map(const void* qkv, const void* img_kv, const int* image_of, const int* ntok, const float2* stats,
                                 const int* lens, float* out, size_t out_sq, size_t out_sj, int Tc, int Q, int H, int N_img,
                                 int Lp, float scale, bool is_f32, int* bad, hipStream_t s) {
    if (Q < 1 || H < 1 || Lp < 1 || N_img < 1 || Tc < 1 || !stats || !out) return hipErrorInvalidValue;
    const dim3 grid(Q, (Lp + AM_ROWS - 1) / AM_ROWS, (N_img + Tc + AM_COLS - 1) / AM_COLS);
    if (is_f32)
        hipLaunchKernelGGL(score_attn_map_kernel, grid, dim3(AM_COLS), 0, s, (const float*)qkv, (const float*)img_kv, image_of, ntok,
                           stats, lens, out, out_sq, out_sj, Tc, H, N_img, Lp, scale, bad);
    else
        hipLaunchKernelGGL(score_attn_map_mfma_kernel, grid, dim3(256), 0, s, (const bf16_t*)qkv, (const bf16_t*)img_kv, image_of,
                           ntok, stats, lens, out, out_sq, out_sj, Tc, H, N_img, Lp, scale, bad);
    return hipGetLastError();
}

// ---- vocabulary head with fused log-softmax statistics (16-bit operands) ------------------------------------------
// Workgroup: 4 waves, 128 rows x 128 columns; wave w owns rows [32 w, 32 w + 32) of the tile.  Operands are loaded
// straight from the row-major activations A [M][lda] and weights W [V][K] in MFMA operand order (one 16-byte load per
// lane and fragment).  Rows >= M and columns >= V are clamped for loading and masked in the epilogue.
// part[row][tile] = (max z, sum exp(z - max), sum (z - max)) over the tile's valid columns; zt[row] = z at the row's target.
// (Sums relative to the tile maximum keep mean_lp exact when every logit of a row carries a large common offset.)
constexpr int SH_ROWS = 128, SH_COLS = 128;

__global__ __launch_bounds__(256) void score_head_kernel(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ W,
                                                         const float* __restrict__ bias, const int* __restrict__ tgt, int M,
                                                         int V, int K, float4* __restrict__ part, float* __restrict__ zt,
                                                         int ntiles) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x;
    const int col0 = tile * SH_COLS;
    const int row0 = blockIdx.y * SH_ROWS + wave * 32;
    const int rl = lane & 15, kq = (lane >> 4) * 8;
    const bf16_t* ap[2];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) ap[rb] = A + (size_t)min(row0 + rb * 16 + rl, M - 1) * lda + kq;
    const bf16_t* wp[8];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) wp[cb] = W + (size_t)min(col0 + cb * 16 + rl, V - 1) * K + kq;
    f32x4_t acc[2][8];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) acc[rb][cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 32) {
        bf16x8_t a[2], b[8];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) a[rb] = *reinterpret_cast<const bf16x8_t*>(ap[rb] + k0);
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) b[cb] = *reinterpret_cast<const bf16x8_t*>(wp[cb] + k0);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) acc[rb][cb] = mfma16(a[rb], b[cb], acc[rb][cb]);
    }
    // epilogue: acc[rb][cb][i] = z of row row0 + rb * 16 + 4 * (lane / 16) + i, column col0 + cb * 16 + lane % 16
    float bcol[8];
    bool cval[8];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
        const int col = col0 + cb * 16 + rl;
        cval[cb] = col < V;
        bcol[cb] = cval[cb] ? bias[col] : 0.f;
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + rb * 16 + (lane >> 4) * 4 + i;
            const int t = row < M ? tgt[row] : -1;
            float z[8];
            float mx = -INFINITY, sz = 0.f;
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                z[cb] = acc[rb][cb][i] + bcol[cb];
                if (cval[cb]) mx = fmaxf(mx, z[cb]);
                if (col0 + cb * 16 + rl == t) zt[row] = z[cb];
            }
            mx = xor16_max(mx);
            float se = 0.f;
#pragma unroll
            for (int cb = 0; cb < 8; ++cb)
                if (cval[cb]) { se += __expf(z[cb] - mx); sz += z[cb] - mx; }
            se = xor16_sum(se);
            sz = xor16_sum(sz);
            if (rl == 0 && row < M) part[(size_t)row * ntiles + tile] = make_float4(mx, se, sz, 0.f);
        }
}

int score_head_tiles(int V) { return (V + SH_COLS - 1) / SH_COLS; }

hipError_t launch_score_head(const void* A, int lda, const void* W, const float* bias, const int* tgt, int M, int V, int K,
                             float4* part, float* zt, hipStream_t s) {
    if (M < 1 || V < 1 || K % 32 || lda % 8) return hipErrorInvalidValue;
    const dim3 grid(score_head_tiles(V), (M + SH_ROWS - 1) / SH_ROWS), block(256);
    hipLaunchKernelGGL(score_head_kernel, grid, block, 0, s, (const bf16_t*)A, lda, (const bf16_t*)W, bias, tgt, M, V, K,
                       part, zt, score_head_tiles(V));
    return hipGetLastError();
}

// ---- f32 mode: the same statistics from materialised logits rows (one part per row) -------------------------------
__global__ __launch_bounds__(256) void score_rowstats_kernel(const float* __restrict__ logits, int ldl, int V,
                                                             const int* __restrict__ tgt, int row_off,
                                                             float4* __restrict__ part, float* __restrict__ zt) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x, row = row_off + r;
    const float* x = logits + (size_t)r * ldl;
    float mx = -INFINITY;
    for (int c = tid; c < V; c += 256) mx = fmaxf(mx, x[c]);
    mx = wave_max(mx);
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    __syncthreads();
    float se = 0.f, sz = 0.f;
    for (int c = tid; c < V; c += 256) { se += __expf(x[c] - mx); sz += x[c] - mx; }
    se = wave_sum(se);
    sz = wave_sum(sz);
    __shared__ float s_red2[8];
    if (lane == 0) { s_red2[wave] = se; s_red2[4 + wave] = sz; }
    __syncthreads();
    if (tid == 0) {
        part[row] = make_float4(mx, s_red2[0] + s_red2[1] + s_red2[2] + s_red2[3], s_red2[4] + s_red2[5] + s_red2[6] + s_red2[7], 0.f);
        const int t = tgt[row];
        if (t >= 0 && t < V) zt[row] = x[t];
    }
}

hipError_t launch_score_rowstats(const float* logits, int ldl, int V, const int* tgt, int row_off, int rows, float4* part,
                                 float* zt, hipStream_t s) {
    if (rows < 1) return hipSuccess;
    hipLaunchKernelGGL(score_rowstats_kernel, dim3(rows), dim3(256), 0, s, logits, ldl, V, tgt, row_off, part, zt);
    return hipGetLastError();
}

// ---- targets of every head row: row (q, j) predicts tokens[q][j + 1] when j + 1 < len_q, else -1 (no target) -------
__global__ void score_targets_kernel(const long long* __restrict__ tokens, int ld, int Lp, const int* __restrict__ lens,
                                     int V, int M, int* __restrict__ tgt) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M) return;
    const int q = row / Lp, j = row - q * Lp;
    int t = -1;
    if (j + 1 < lens[q]) {
        const long long v = tokens[(size_t)q * ld + j + 1];
        t = v < 0 ? 0 : (v >= V ? V - 1 : (int)v);
    }
    tgt[row] = t;
}

hipError_t launch_score_targets(const long long* tokens, int ld, int Lp, const int* lens, int V, int M, int* tgt,
                                hipStream_t s) {
    hipLaunchKernelGGL(score_targets_kernel, dim3((M + 255) / 256), dim3(256), 0, s, tokens, ld, Lp, lens, V, M, tgt);
    return hipGetLastError();
}

// ---- combine: per head row with a target, LSE over the tiles -> out[q][j + 1] = (lp, mean_lp); bad[q] = 1 when either
// value is not finite.  One wave per row.  Tile t covers min(tile_w, V - t tile_w) columns; with M = max over the tiles,
// S = sum_t se_t exp(m_t - M), D = sum_t (sz_t + n_t (m_t - M)) = sum_c (z_c - M):  LSE = M + log S, mean_lp = D / V - log S.
// (lp, mean_lp) of one head row from its tiles `p` and the logit z at the target, by the whole wave (the value is lane 0's)
__device__ __forceinline__ float2 combine_row(const float4* __restrict__ p, int ntiles, int tile_w, int V, float z, int lane) {
    float mx = -INFINITY;
    for (int t = lane; t < ntiles; t += 64) mx = fmaxf(mx, p[t].x);
    mx = wave_max(mx);
    float se = 0.f, sd = 0.f;
    for (int t = lane; t < ntiles; t += 64) {
        const float4 v = p[t];
        const float n = (float)min(tile_w, V - t * tile_w);
        se += v.y * __expf(v.x - mx);
        sd += v.z + n * (v.x - mx);
    }
    se = wave_sum(se);
    sd = wave_sum(sd);
    const float ls = logf(se);
    return make_float2((z - mx) - ls, sd / (float)V - ls);
}

__global__ __launch_bounds__(64) void score_combine_kernel(const float4* __restrict__ part, int ntiles, int tile_w,
                                                           const float* __restrict__ zt, const int* __restrict__ tgt,
                                                           int Lp, int ld, int V, float2* __restrict__ out,
                                                           int* __restrict__ bad) {
    const int lane = threadIdx.x;
    const int row = blockIdx.x;
    if (tgt[row] < 0) return;
    const float2 r = combine_row(part + (size_t)row * ntiles, ntiles, tile_w, V, zt[row], lane);
    if (lane == 0) {
        const int q = row / Lp, j = row - q * Lp;
        out[(size_t)q * ld + j + 1] = r;
        if (!isfinite(r.x) || !isfinite(r.y)) bad[q] = 1;
    }
}

hipError_t launch_score_combine(const float4* part, int ntiles, const float* zt, const int* tgt, int M, int Lp, int ld, int V,
                                float2* out, int* bad, hipStream_t s) {
    const int tile_w = ntiles == 1 ? V : SH_COLS;     // one statistics row per logits row (f32 mode) or the head's tiles
    hipLaunchKernelGGL(score_combine_kernel, dim3(M), dim3(64), 0, s, part, ntiles, tile_w, zt, tgt, Lp, ld, V, out, bad);
    return hipGetLastError();
}

// info = {ld, i1, i2, sentences with a non-finite value} (score: i1 = i2 = 0; attention maps: Kc, layers)
__global__ void score_info_kernel(const int* __restrict__ bad, int Q, int ld, int i1, int i2, int* __restrict__ info) {
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int n = 0;
    for (int q = threadIdx.x; q < Q; q += blockDim.x) n += bad[q] ? 1 : 0;
    atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0) { info[0] = ld; info[1] = i1; info[2] = i2; info[3] = s_n; }
}

hipError_t launch_score_info(const int* bad, int Q, int ld, int* info, hipStream_t s, int i1, int i2) {
    hipLaunchKernelGGL(score_info_kernel, dim3(1), dim3(256), 0, s, bad, Q, ld, i1, i2, info);
    return hipGetLastError();
}

// ---- token trees (GITMI_SEARCH_TREE_SCORE) -------------------------------------------------------------------------------
// The rows of the text pass are the nodes of Q trees in DFS pre-order: tree q, node i -> row q * Lp + i.  packed [Q][ld] int64 =
// (depth << 32 | token id); the parent of node i is the last k < i with depth[k] == depth[i] - 1.  In pre-order node k is an
// ancestor-or-self of node i exactly when k <= i < end[k], end[k] the first index past k's subtree.
//
// One wave per tree.  The verdict first, from local rules only (depth[0] == 0, 1 <= depth[i] <= depth[i - 1] + 1, depth <
// max_depth): a tree that fails gets bad[q] = 1 and the structure of rows past a tree's nodes -- every row a root of its own
// (depth 0, no parent, end = i + 1: it attends to the image and itself, has no target, and nothing is indexed by its depths).
// Then lane 0 walks the nodes in order with the current root path in LDS (max_depth entries): node i at depth dp closes the path
// entries at depths >= dp (their end is i) and takes path[dp - 1] as its parent.  Depths (the validated copies: the caller's table is
// not read again) and parents pass through LDS in chunks of 64 so that the global accesses of the walk are the whole wave's; every node's end is stored once, when the node is closed.
__global__ __launch_bounds__(64) void tree_structure_kernel(const long long* __restrict__ packed, int ld, int Lp,
                                                            const int* __restrict__ lens, int V, int max_depth, TreeNodes nd,
                                                            int* __restrict__ bad) {
    extern __shared__ int s_path[];
    __shared__ int s_dp[64], s_par[64];
    const int lane = threadIdx.x, q = blockIdx.x;
    const int n = max(0, min(lens[q], min(ld, Lp)));
    const long long* src = packed + (size_t)q * ld;
    const size_t row_base = (size_t)q * Lp;
    bool wrong = false;
    for (int i = lane; i < n; i += 64) {
        const long long dp = src[i] >> 32;
        const long long up = i ? (src[i - 1] >> 32) + 1 : 0;
        wrong = wrong || dp >= max_depth || dp > up || dp < (i ? 1 : 0);
    }
    const bool ok = __ballot(wrong) == 0;
    for (int i = lane; i < Lp; i += 64) {
        const bool live = ok && i < n;
        const long long v = i < n ? src[i] : 0;
        const int t = (int)(v & 0xffffffffll);
        nd.tok[row_base + i] = t < 0 ? 0 : (t >= V ? V - 1 : t);
        nd.depth[row_base + i] = live ? (int)(v >> 32) : 0;
        if (!live) { nd.parent[row_base + i] = -1; nd.end[row_base + i] = i + 1; }
    }
    if (!ok) {
        if (lane == 0) bad[q] = 1;
        return;
    }
    int top = -1;                                           // lane 0: depth of the node the path ends in
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int cn = min(64, n - c0);
        __syncthreads();
        if (lane < cn) s_dp[lane] = nd.depth[row_base + c0 + lane];      // the validated copy, written above by this very lane
        __syncthreads();
        if (lane == 0) {
            for (int r = 0; r < cn; ++r) {
                const int i = c0 + r, dp = s_dp[r];
                for (int k = top; k >= dp; --k) nd.end[row_base + s_path[k]] = i;
                s_par[r] = dp ? s_path[dp - 1] : -1;
                s_path[dp] = i;
                top = dp;
            }
        }
        __syncthreads();
        if (lane < cn) nd.parent[row_base + c0 + lane] = s_par[lane];
    }
    if (lane == 0)
        for (int k = top; k >= 0; --k) nd.end[row_base + s_path[k]] = n;
}

hipError_t launch_tree_structure(const long long* packed, int ld, int Q, int Lp, const int* lens, int V, int max_depth,
                                 const TreeNodes& nd, int* bad, hipStream_t s) {
    if (Q < 1 || Lp < 1 || ld < 1 || V < 1 || max_depth < 1 || max_depth > 8192) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tree_structure_kernel, dim3(Q), dim3(64), (size_t)max_depth * sizeof(int), s, packed, ld, Lp, lens, V,
                       max_depth, nd, bad);
    return hipGetLastError();
}

// The logit of every node's token at its parent's head row, zt[row of node i] = z[parent(i)][token(i)] (nodes without a parent:
// not written).  16-bit modes: the head's operands again -- A row of the parent, W row of the token, fp32 accumulation, + bias;
// one wave per node.
__global__ __launch_bounds__(256) void tree_gather_dot_kernel(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ W,
                                                              const float* __restrict__ bias, TreeNodes nd, int Lp, int M, int K,
                                                              float* __restrict__ zt) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int par = nd.parent[row];
    if (par < 0) return;
    const int tok = nd.tok[row];
    const bf16_t* a = A + ((size_t)(row / Lp) * Lp + par) * lda;
    const bf16_t* w = W + (size_t)tok * K;
    float acc = 0.f;
    for (int c = lane * 8; c < K; c += 512) {
        float x[8], y[8];
        ld8(a + c, x);
        ld8(w + c, y);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = fmaf(x[i], y[i], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) zt[row] = acc + bias[tok];
}
// f32 mode: from the materialised logits of head rows [row_off, row_off + rows); the children of those rows lie behind them in
// their own trees: nodes [row_off, first row of the tree after the chunk's last row)
__global__ void tree_gather_logits_kernel(const float* __restrict__ logits, int ldl, int row_off, int rows, TreeNodes nd, int Lp,
                                          int row_end, float* __restrict__ zt) {
    const int row = row_off + blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= row_end) return;
    const int par = nd.parent[row];
    if (par < 0) return;
    const int prow = (row / Lp) * Lp + par;
    if (prow < row_off || prow >= row_off + rows) return;
    zt[row] = logits[(size_t)(prow - row_off) * ldl + nd.tok[row]];
}

hipError_t launch_tree_gather_dot(const void* A, int lda, const void* W, const float* bias, const TreeNodes& nd, int Lp, int M,
                                  int K, float* zt, hipStream_t s) {
    if (M < 1 || Lp < 1 || K % 8 || lda % 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tree_gather_dot_kernel, dim3((M + 3) / 4), dim3(256), 0, s, (const bf16_t*)A, lda, (const bf16_t*)W, bias,
                       nd, Lp, M, K, zt);
    return hipGetLastError();
}
hipError_t launch_tree_gather_logits(const float* logits, int ldl, int row_off, int rows, const TreeNodes& nd, int Lp, int M,
                                     float* zt, hipStream_t s) {
    if (rows < 1) return hipSuccess;
    const int tree_end = ((row_off + rows - 1) / Lp + 1) * Lp, row_end = tree_end < M ? tree_end : M;
    hipLaunchKernelGGL(tree_gather_logits_kernel, dim3((row_end - row_off + 255) / 256), dim3(256), 0, s, logits, ldl, row_off,
                       rows, nd, Lp, row_end, zt);
    return hipGetLastError();
}

// combine: node i with a parent -> out[q][i] = (lp, mean_lp) from the tiles of the parent's head row and zt at the node's own row
__global__ __launch_bounds__(64) void tree_combine_kernel(const float4* __restrict__ part, int ntiles, int tile_w,
                                                          const float* __restrict__ zt, TreeNodes nd, int Lp, int ld, int V,
                                                          float2* __restrict__ out, int* __restrict__ bad) {
    const int lane = threadIdx.x;
    const int row = blockIdx.x;
    const int par = nd.parent[row];
    if (par < 0) return;
    const int q = row / Lp, i = row - q * Lp;             // a node with a parent is one of the tree's n_q <= ld nodes
    const float2 r = combine_row(part + ((size_t)q * Lp + par) * ntiles, ntiles, tile_w, V, zt[row], lane);
    if (lane == 0) {
        out[(size_t)q * ld + i] = r;
        if (!isfinite(r.x) || !isfinite(r.y)) bad[q] = 1;
    }
}

hipError_t launch_tree_combine(const float4* part, int ntiles, const float* zt, const TreeNodes& nd, int M, int Lp, int ld, int V,
                               float2* out, int* bad, hipStream_t s) {
    const int tile_w = ntiles == 1 ? V : SH_COLS;
    hipLaunchKernelGGL(tree_combine_kernel, dim3(M), dim3(64), 0, s, part, ntiles, tile_w, zt, nd, Lp, ld, V, out, bad);
    return hipGetLastError();
}

// ---- the head of a whole text pass (launchers.h) -----------------------------------------------------------------------------
// f32: a chunk's logits are overwritten by the next chunk's, so a tree's children are gathered chunk by chunk, each when the
// chunk that holds its parent's row is materialised
hipError_t launch_score_head_rows(const ScoreHeadArgs& h, bool f32, int M, int V, int K, const TreeNodes* tree, int Lp, int* ntiles,
                                  hipStream_t s) {
    if (M < 1 || V < 1 || K < 1 || (tree && Lp < 1)) return hipErrorInvalidValue;
    *ntiles = 1;
    if (!f32) {
        *ntiles = score_head_tiles(V);
        const hipError_t err = launch_score_head(h.A, K, h.W, h.bias, h.tgt, M, V, K, h.part, h.zt, s);
        if (err != hipSuccess || !tree) return err;
        return launch_tree_gather_dot(h.A, K, h.W, h.bias, *tree, Lp, M, K, h.zt, s);
    }
    if (!h.logits || h.chunk_rows < 1 || h.ldl < V) return hipErrorInvalidValue;
    for (int r0 = 0; r0 < M; r0 += h.chunk_rows) {
        const int rows = h.chunk_rows < M - r0 ? h.chunk_rows : M - r0;
        GemmArgs g{};
        g.A = (const float*)h.A + (size_t)r0 * K; g.W = h.W; g.bias = h.bias; g.C = h.logits;
        g.M = rows; g.N = V; g.K = K; g.lda = K; g.ldc = h.ldl;
        hipError_t err = launch_gemm(g, true, true, s);
        if (err == hipSuccess) err = launch_score_rowstats(h.logits, h.ldl, V, h.tgt, r0, rows, h.part, h.zt, s);
        if (err == hipSuccess && tree) err = launch_tree_gather_logits(h.logits, h.ldl, r0, rows, *tree, Lp, M, h.zt, s);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace gitmi
