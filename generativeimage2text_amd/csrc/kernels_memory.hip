// Image memory snapshots (GITMI_SEARCH_KEEP / GITMI_SEARCH_RECALL, include/gitmi.h): the encoded memory of an image -- its
// feature rows and the K | V columns of its prefill rows of every decoder layer -- copied between the engine's buffers and a
// slot of the caller's store.  Pure copies: every lane moves 16 bytes per step, rows are walked so that consecutive lanes touch
// consecutive 16-byte pieces of a row.  One launch per call: grid (tiles of 16 rows, feature plane + layers, images).
// No address is formed from the bytes of a slot: the valid row count and the header come from the host-validated table.
#include "launchers.h"

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

}  // namespace gitmi
