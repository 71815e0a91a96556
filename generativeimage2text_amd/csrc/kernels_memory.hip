// Image memory snapshots (GITMI_SEARCH_KEEP / GITMI_SEARCH_RECALL, include/gitmi.h): the encoded memory of an image -- its
// feature rows and the K | V columns of its prefill rows of every decoder layer -- copied between the engine's buffers and a
// slot of the caller's store.  Pure copies: every lane moves 16 bytes per step, rows are walked so that consecutive lanes touch
// consecutive 16-byte pieces of a row.  One launch per call: grid (tiles of 16 rows, feature plane + layers, images).
// No address is formed from the bytes of a slot: the valid row count and the header come from the host-validated table.
// Features in (GITMI_SEARCH_FEATURES), at the end of the file: the caller's feature rows, cut into pieces, written into the same
// feature tensor -- a copy, or fp32 -> operand type with the temporal embedding of a piece added.
#include "launchers.h"
#include "gitmi_common.h"

#include <type_traits>

namespace gitmi {

constexpr int MEMORY_TILE_ROWS = 16;

// where plane `p` (0: features, 1 + l: layer l) of a block / of a slot starts, its row pitch and the bytes copied per row
struct MemoryPlane { char* eng; size_t slot_off; int eng_ld, row; };
__device__ inline MemoryPlane memory_plane(const MemoryArgs& a, int p, int image) {
    MemoryPlane pl;
    if (p == 0) {
        pl.eng = (char*)a.feats + (size_t)image * a.stride * a.feat_row;
        pl.slot_off = MEMORY_HEADER_BYTES;
        pl.eng_ld = a.feat_row; pl.row = a.feat_row;
    } else {
        pl.eng = (char*)a.kv[p - 1] + (size_t)image * a.stride * a.kv_ld + a.kv_col;
        pl.slot_off = MEMORY_HEADER_BYTES + a.feat_plane + (size_t)(p - 1) * a.kv_plane;
        pl.eng_ld = a.kv_ld; pl.row = a.kv_row;
    }
    return pl;
}

__global__ __launch_bounds__(256) void memory_pack_kernel(MemoryArgs a, char* __restrict__ store, const MemoryEntry* __restrict__ tab) {
    const MemoryEntry& en = tab[blockIdx.z];
    const int n = en.n, r0 = blockIdx.x * MEMORY_TILE_ROWS;
    char* slot = store + (size_t)en.slot * a.slot_bytes;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < MEMORY_HEADER_BYTES / 16) {
        const int t = threadIdx.x;          // 16 lanes x 16 bytes: the header words, then zeros
        const int4* h = reinterpret_cast<const int4*>(en.hdr);
        reinterpret_cast<int4*>(slot)[t] = t < MEMORY_HEADER_WORDS / 4 ? h[t] : int4{0, 0, 0, 0};
    }
    if (r0 >= n) return;
    const MemoryPlane pl = memory_plane(a, blockIdx.y, en.image);
    const int per_row = pl.row / 16, rows = min(MEMORY_TILE_ROWS, n - r0);
    const char* src = pl.eng + (size_t)r0 * pl.eng_ld;
    char* dst = slot + pl.slot_off + (size_t)r0 * pl.row;
    for (int i = threadIdx.x; i < rows * per_row; i += 256) {
        const int r = i / per_row, c = i - r * per_row;
        reinterpret_cast<uint4*>(dst + (size_t)r * pl.row)[c] = reinterpret_cast<const uint4*>(src + (size_t)r * pl.eng_ld)[c];
    }
}

__global__ __launch_bounds__(256) void memory_unpack_kernel(MemoryArgs a, const char* __restrict__ store,
                                                            const MemoryEntry* __restrict__ tab) {
    const MemoryEntry& en = tab[blockIdx.z];
    const int n = en.n, r0 = blockIdx.x * MEMORY_TILE_ROWS;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        a.ntok[en.image] = n;
        if (a.meta) a.meta[en.image] = int4{en.hdr[MEMW_H], en.hdr[MEMW_W], n, 0};
    }
    if (r0 >= a.stride) return;
    const MemoryPlane pl = memory_plane(a, blockIdx.y, en.image);
    const int per_row = pl.row / 16, rows = min(MEMORY_TILE_ROWS, a.stride - r0);
    const char* src = store + (size_t)en.slot * a.slot_bytes + pl.slot_off + (size_t)r0 * pl.row;
    char* dst = pl.eng + (size_t)r0 * pl.eng_ld;
    for (int i = threadIdx.x; i < rows * per_row; i += 256) {
        const int r = i / per_row, c = i - r * per_row;
        // rows [n, stride) of the block: zeros (never keys, and finite where a later prefill or repack reads them)
        const uint4 v = r0 + r < n ? reinterpret_cast<const uint4*>(src + (size_t)r * pl.row)[c] : make_uint4(0u, 0u, 0u, 0u);
        reinterpret_cast<uint4*>(dst + (size_t)r * pl.eng_ld)[c] = v;
    }
}

static bool memory_args_ok(const MemoryArgs& a, const void* store, const void* tab, int entries) {
    if (!store || !tab || entries < 1 || entries > 65535 || a.layers < 0 || a.layers > MEMORY_MAX_LAYERS || a.stride < 1) return false;
    if ((a.feat_row | a.kv_row | a.kv_ld | a.kv_col) & 15 || a.feat_row < 16 || a.kv_row < 16) return false;
    if (((uintptr_t)store | (uintptr_t)a.feats | a.slot_bytes | a.feat_plane | a.kv_plane) & 15) return false;
    for (int l = 0; l < a.layers; ++l)
        if (!a.kv[l] || ((uintptr_t)a.kv[l] & 15)) return false;
    return a.feats != nullptr;
}

hipError_t launch_memory_pack(const MemoryArgs& a, void* store, const MemoryEntry* tab, int entries, int max_n, hipStream_t s) {
    if (!memory_args_ok(a, store, tab, entries) || max_n < 0 || max_n > a.stride) return hipErrorInvalidValue;
    const int tiles = (max_n + MEMORY_TILE_ROWS - 1) / MEMORY_TILE_ROWS;
    hipLaunchKernelGGL(memory_pack_kernel, dim3(tiles > 0 ? tiles : 1, 1 + a.layers, entries), dim3(256), 0, s, a, (char*)store, tab);
    return hipGetLastError();
}

hipError_t launch_memory_unpack(const MemoryArgs& a, const void* store, const MemoryEntry* tab, int entries, hipStream_t s) {
    if (!memory_args_ok(a, store, tab, entries) || !a.ntok) return hipErrorInvalidValue;
    const int tiles = (a.stride + MEMORY_TILE_ROWS - 1) / MEMORY_TILE_ROWS;
    hipLaunchKernelGGL(memory_unpack_kernel, dim3(tiles, 1 + a.layers, entries), dim3(256), 0, s, a, (const char*)store, tab);
    return hipGetLastError();
}

// ---- features in (GITMI_SEARCH_FEATURES, include/gitmi.h): the caller's feature rows become the resident feature tensor ----------
// One launch: grid (tiles of 16 rows of an image's block, images).  The first 16 lanes of a workgroup resolve the tile's rows
// against the host-validated piece table (pieces start and end anywhere inside a tile; a row of [0, n_b) lies in exactly one
// piece of its image), the whole workgroup then moves them: a lane handles 8 consecutive elements of a row with 16-byte loads
// and stores.  Rows [n_b, stride) are written as zeros, so every row of every block has exactly one writer.  No address is
// formed from anything but the table.
//   fp32 source   : (+ temporal embedding, a separate fp32 add as in layernorm_kernel's add_after), then the store the
//                   LayerNorm kernels do: fp32 as is, or one round-to-nearest-even conversion to the operand type (st8)
//   16-bit source : without an embedding the 16 bytes are copied as they are; with one: widen, add, round once
template <bool SRC16, bool DST16>
__global__ __launch_bounds__(256) void feature_install_kernel(FeatureArgs a) {
    __shared__ int s_src[MEMORY_TILE_ROWS];
    __shared__ const float* s_te[MEMORY_TILE_ROWS];
    const int b = blockIdx.y, r0 = blockIdx.x * MEMORY_TILE_ROWS, n = a.count[b];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.ntok[b] = n;
        if (a.meta) a.meta[b] = int4{0, 0, n, 0};
    }
    if (threadIdx.x < MEMORY_TILE_ROWS) {
        const int r = r0 + threadIdx.x;
        int src = -1;
        const float* te = nullptr;
        if (r < n)
            for (int q = 0; q < a.pieces_n; ++q) {
                const FeaturePiece p = a.pieces[q];
                if (p.image == b && r >= p.dst0 && r - p.dst0 < p.rows) { src = p.src0 + (r - p.dst0); te = p.temb; }
            }
        s_src[threadIdx.x] = src;
        s_te[threadIdx.x] = te;
    }
    __syncthreads();
    using TSrc = typename std::conditional<SRC16, bf16_t, float>::type;
    using TDst = typename std::conditional<DST16, bf16_t, float>::type;
    const int D = a.D, per_row = D / 8, rows = min(MEMORY_TILE_ROWS, a.stride - r0);
    TDst* dst0 = (TDst*)a.feats + ((size_t)b * a.stride + r0) * D;
    for (int i = threadIdx.x; i < rows * per_row; i += 256) {
        const int r = i / per_row, c = (i - r * per_row) * 8;
        const int src = s_src[r];
        TDst* dst = dst0 + (size_t)r * D + c;
        if (src < 0) {          // rows [n_b, stride): zeros (never keys, and finite where the prefill reads them)
            const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            st8(dst, z);
            continue;
        }
        const TSrc* sp = (const TSrc*)a.src + (size_t)src * D + c;
        const float* te = s_te[r];
        if constexpr (SRC16 && DST16) {
            if (!te) {
                *reinterpret_cast<u32x4_t*>(dst) = *reinterpret_cast<const u32x4_t*>(sp);
                continue;
            }
        }
        float v[8];
        ld8(sp, v);
        if (te) {
            float t8[8];
            ld8(te + c, t8);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += t8[e];
        }
        st8(dst, v);
    }
}

hipError_t launch_feature_install(const FeatureArgs& a, int B, bool src16, bool dst16, hipStream_t s) {
    if (!a.feats || !a.src || !a.pieces || !a.count || !a.ntok || a.pieces_n < 1 || B < 1 || B > 65535 || a.stride < 1 || a.D < 8 ||
        a.D % 8 || (src16 && !dst16))
        return hipErrorInvalidValue;
    if (((uintptr_t)a.feats | (uintptr_t)a.src) & 15) return hipErrorInvalidValue;
    const dim3 grid((a.stride + MEMORY_TILE_ROWS - 1) / MEMORY_TILE_ROWS, B), block(256);
    if (src16) hipLaunchKernelGGL((feature_install_kernel<true, true>), grid, block, 0, s, a);
    else if (dst16) hipLaunchKernelGGL((feature_install_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((feature_install_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace gitmi
