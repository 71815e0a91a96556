// What the consumer GEMMs of the decode chain share, as device code: row statistics from strip partials, the K slice of a wave,
// the MFMA sequence over a register-held slice, the wave-order sum and the consumer epilogue.  Included by kernels_dgemm.hip (the
// chain GEMMs, the vocabulary head) and by kernels_attn_decode.hip (the attention form that computes its own q | k | v rows):
// every kernel that promises the bits of dgemm_kernel<4, 4, DEPI_BF16> keeps the promise by CALLING this code.
//
// Contraction: the functions here carry the DEFAULT contraction of the build.  A file that turns contraction off must include
// this header BEFORE its `#pragma clang fp contract(off)`, and expand DGEMM_CONSUMER_FINISH inside a block that turns it back on
// (`#pragma clang fp contract(fast)`): see the note at the macro.
#pragma once
#include "gitmi_common.h"

namespace gitmi {

// ---- row statistics from strip partials --------------------------------------------------------------
// stats[strip][row] = (sum, sum of squares) over the strip's 16 columns.  The 4 lanes that share a row (lane>>4 = 0..3)
// each take strips lg, lg+4, ... and combine with two shuffles; every lane ends with (mean, rstd) of its row.
constexpr int STRIP_SLOTS = 16;          // per lane: up to 64 strips = 1024 columns

struct RowStatLoads {
    float2 v[STRIP_SLOTS];
};
__device__ __forceinline__ void stats_issue(RowStatLoads& L, const float2* __restrict__ stats, int strips, int M,
                                            int row, int lg) {
#pragma unroll
    for (int u = 0; u < STRIP_SLOTS; ++u) {
        const int sidx = lg + 4 * u;
        L.v[u] = sidx < strips ? stats[(size_t)sidx * M + row] : float2{0.f, 0.f};
    }
}
// branch-free form (clamped strip index, zero-selected): no control flow around the loads
__device__ __forceinline__ void stats_issue_nb(RowStatLoads& L, const float2* __restrict__ stats, int strips, int M,
                                               int row, int lg) {
#pragma unroll
    for (int u = 0; u < STRIP_SLOTS; ++u) {
        const int sidx = lg + 4 * u;
        const float2 v = stats[(size_t)min(sidx, strips - 1) * M + row];
        L.v[u] = sidx < strips ? v : float2{0.f, 0.f};
    }
}
__device__ __forceinline__ void stats_finish(const RowStatLoads& L, float inv_d, float eps, float& mean, float& rstd) {
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int u = 0; u < STRIP_SLOTS; ++u) { s += L.v[u].x; q += L.v[u].y; }
    s += __shfl_xor(s, 16, 64); q += __shfl_xor(q, 16, 64);
    s += __shfl_xor(s, 32, 64); q += __shfl_xor(q, 32, 64);
    mean = s * inv_d;
    const float var = fmaxf(q * inv_d - mean * mean, 0.f);
    rstd = rsqrtf(var + eps);
}

// ---- what the GEMM kernels of the chain share ----------------------------------------------------------------------
// The two wide forms promise the bits of dgemm_kernel<4, 4, DEPI_BF16>, and the serving policy switches between the three.
// They keep the promise by CALLING the same code: the K slice of a wave, the MFMA sequence over a register-held slice, the
// wave-order sum and the consumer epilogue are written here and nowhere else.  A kernel body keeps what is its own: its row /
// strip mapping, which loads it issues and when, its LDS exchange buffers and barriers, its dbg switches.

// k-steps [kb, ke) of wave `wave` when `ksteps` k-steps of 32 are split over nw waves (kb >= ke: the wave has none)
struct KSlice { int kb, ke; };
__device__ __forceinline__ KSlice k_slice(int ksteps, int nw, int wave) {
    const int per = (ksteps + nw - 1) / nw;
    const int kb = wave * per;
    return KSlice{kb, min(kb + per, ksteps)};
}

// entries n .. n+3 of a per-column constant (bias, colsum) of N entries; indices past the end are clamped, their columns never stored
__device__ __forceinline__ float4 load_cols4(const float* p, int n, int N) {
    float4 r;
    r.x = p[n < N ? n : N - 1];
    r.y = p[n + 1 < N ? n + 1 : N - 1];
    r.z = p[n + 2 < N ? n + 2 : N - 1];
    r.w = p[n + 3 < N ? n + 3 : N - 1];
    return r;
}

// Register-held K slice of the wide forms: at most DW_KS k-steps per wave, zero past ke.
constexpr int DW_KS = 6;        // k-steps per wave held in registers: K <= 4 * 6 * 32 = 768
// the wave's slice of weight strip `strip` (read once: non-temporal).  Returned by value, and mfma_slice adds to accumulators the
// kernel has zeroed: with the fragments filled through a reference, or the zeroing inside mfma_slice, dgemm_wide_strips_kernel<6>
// loses the fused multiply-adds of its epilogue (same note as at DGEMM_CONSUMER_FINISH below)
struct WSlice { bf16x8_t f[DW_KS]; };
template <bool NT = true>       // false: cacheable loads, for a strip that other workgroups read again from the L2
__device__ __forceinline__ WSlice load_w_slice(const bf16_t* W, int strip, KSlice ks, int ksteps, int lane) {
    WSlice w;
    const bf16_t* wp = W + frag_tile(strip, 0, ksteps, lane);
#pragma unroll
    for (int u = 0; u < DW_KS; ++u)
        w.f[u] = ks.kb + u >= ks.ke ? bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0}
                 : NT ? __builtin_nontemporal_load(reinterpret_cast<const bf16x8_t*>(wp + (size_t)(ks.kb + u) * 512))
                      : *reinterpret_cast<const bf16x8_t*>(wp + (size_t)(ks.kb + u) * 512);
    return w;
}
// the wave's slice of the MT row tiles rt0 .. rt0+MT-1 of the activations (the chain GEMMs: 4; the attention's projection: 1)
template <int MT>
__device__ __forceinline__ void load_x_slice(bf16x8_t (&xf)[DW_KS][MT], const bf16_t* X, int rt0, KSlice ks, int ksteps, int lane) {
#pragma unroll
    for (int u = 0; u < DW_KS; ++u)
#pragma unroll
        for (int i = 0; i < MT; ++i)
            xf[u][i] = ks.kb + u < ks.ke ? *reinterpret_cast<const bf16x8_t*>(X + frag_tile(rt0 + i, ks.kb + u, ksteps, lane))
                                         : bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
}
// acc[i] += partial of row tile i over the slice.  The guard is uniform per wave and stays: it is what keeps the MFMA sequence
// of a wave equal to dgemm_kernel's (no MFMA on the zero fragments past ke)
template <int MT>
__device__ __forceinline__ void mfma_slice(f32x4_t (&acc)[MT], const WSlice& w, const bf16x8_t (&xf)[DW_KS][MT], KSlice ks) {
#pragma unroll
    for (int u = 0; u < DW_KS; ++u) {
        if (ks.kb + u < ks.ke) {
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i] = mfma16(w.f[u], xf[u][i], acc[i]);
        }
    }
}

// red[writer][row tile][lane]: the total of row tile `tile`, writers summed in the FIXED order 0 .. NW-1, component by component
template <int NW, int MT>
__device__ __forceinline__ f32x4_t sum_waves(f32x4_t (*red)[MT][64], int tile, int lane) {
    f32x4_t tot = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const f32x4_t t = red[w][tile][lane];
        tot[0] += t[0]; tot[1] += t[1]; tot[2] += t[2]; tot[3] += t[3];
    }
    return tot;
}

// consumer (QKV / FFN1) epilogue, arithmetic: declares  float v[4] = act(rstd * (tot - mean * colsum) + bias)  with the LayerNorm
// folded (have_stats), else act(tot + bias).  A MACRO, not a function, and the one place where that matters: kernels_dgemm.hip
// compiles with the default contraction, so which products fuse into FMAs is decided after inlining, from the shape the optimiser has
// given the code by then.  Written as a __forceinline__ function (tried: v by reference, returned by value, one function per
// arm, statistics inside or outside) the `+ biasv[r]` the two arms share ends up below their join in some or all kernels, the
// fold's outer multiply-add is then a multiply and an add, and the last bit differs from every earlier build.  Expanded in
// place, the statements compile to the instruction stream they had when each kernel carried its own copy (docs/LAB_NOTEBOOK.md,
// profiles/r12_dgemm_static_resources.txt).  Check the FMA counts per kernel after any change near it.
#define DGEMM_CONSUMER_FINISH(v, tot, bias4, cs4, have_stats, mean, rstd, act)              \
    float v[4] = {(tot)[0], (tot)[1], (tot)[2], (tot)[3]};                                  \
    {                                                                                       \
        const float biasv[4] = {(bias4).x, (bias4).y, (bias4).z, (bias4).w};                \
        if (have_stats) {                                                                   \
            const float cs[4] = {(cs4).x, (cs4).y, (cs4).z, (cs4).w};                       \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) v[r] = (rstd) * (v[r] - (mean) * cs[r]) + biasv[r]; \
        } else {                                                                            \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) v[r] += biasv[r];                 \
        }                                                                                   \
        if ((act) != GITMI_ACT_NONE) {                                                      \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) v[r] = apply_act(v[r], (act));    \
        }                                                                                   \
    }

}  // namespace gitmi
