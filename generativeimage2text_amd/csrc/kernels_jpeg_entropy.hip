// Huffman decode of baseline JPEG scans on the GPU (include/gitmi_jpeg.h: gitmi_jpeg_entropy_batch): scan records ->
// coefficient records, byte for byte what the host decoder (jpeg_entropy.cc) writes.  The per-thread bodies are the plain
// functions of jpeg_entropy_dev.h (its header comment has the scheme and the fixpoint argument); this file holds what needs a
// workgroup: the round loop, the prefix sums and the grids.  Four launches per JPEG_CHUNK images:
//   zero    grid (16-byte pieces of the largest record / 256, image): status word, header copy, planes to zero
//   sync    grid (image): look-ahead tables in LDS, round 0 from (start bit, block 0, k 0), re-decode rounds to the fixpoint,
//           exclusive prefix sum of the completed blocks
//   write   grid (subsequences / 256, image): each subsequence once more from its final state into the planes
//   dc      grid (component, image): inclusive prefix sum of the DC differences in coding order
// Every kernel validates the record itself (jd_setup) before it forms an address; an image that does not check out gets
// JD_ST_RECORD from the zero kernel and no other store.
#include "jpeg_common.h"
#include "jpeg_entropy_dev.h"

namespace {

// the record of image `d` checked by thread 0 into LDS; -> ok (uniform)
__device__ __forceinline__ bool jd_enter(JdCtx* x, const uint8_t* scans, const JpegScanImg& d) {
    if (threadIdx.x == 0) jd_setup(x, scans + d.scan_off, d.scan_size, d.coef_size, d.nsub_cap);
    __syncthreads();
    return x->ok != 0;
}

__global__ __launch_bounds__(JD_THREADS) void jpeg_entropy_zero_kernel(const uint8_t* __restrict__ scans, uint8_t* __restrict__ coef,
                                                                      int* __restrict__ status, uint8_t* __restrict__ tmp,
                                                                      JpegScanChunk ch, int first_image) {
    __shared__ JdCtx x;
    const JpegScanImg& d = ch.d[blockIdx.y];
    const bool ok = jd_enter(&x, scans, d);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        status[first_image + blockIdx.y] = ok ? 0 : JD_ST_RECORD;
        if (ok) jd_work(tmp + d.tmp_off, d.nsub_cap).flags[0] = 0;
    }
    if (!ok) return;
    const unsigned long long at = ((unsigned long long)blockIdx.x * JD_THREADS + threadIdx.x) * 16;
    if (at >= d.coef_size) return;                  // coef_size is the record's own size here, a multiple of 128
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at < GITMI_JPEG_HEADER_BYTES) v = *(const uint4*)(scans + d.scan_off + at);
    *(uint4*)(coef + d.coef_off + at) = v;
}

__global__ __launch_bounds__(JD_THREADS) void jpeg_entropy_sync_kernel(const uint8_t* __restrict__ scans, int* __restrict__ status,
                                                                      uint8_t* __restrict__ tmp, JpegScanChunk ch, int first_image) {
    __shared__ JdCtx x;
    __shared__ uint32_t scan_lds[JD_THREADS];
    __shared__ int changed;
    const JpegScanImg& d = ch.d[blockIdx.x];
    if (!jd_enter(&x, scans, d)) return;
    const uint8_t* rec = scans + d.scan_off;
    jd_setup_tables(&x, rec, threadIdx.x, JD_THREADS);
    __syncthreads();
    const uint32_t* words = (const uint32_t*)(rec + JD_SCAN_AT);
    const JdWork w = jd_work(tmp + d.tmp_off, d.nsub_cap);
    const uint32_t nsub = x.nsub;
    const int tid = threadIdx.x;

    for (uint32_t i = tid; i < nsub; i += JD_THREADS) {          // round 0
        const jd_state in = jd_pack(i * (uint32_t)JD_SUB_BITS, 0, 0);
        uint32_t n;
        w.in[i] = in;
        w.exit[i] = jd_walk(x, words, i, in, &n);
        w.count[i] = n;
    }
    // After round r the first r + 1 subsequences are final, so nsub rounds always reach the fixpoint; the round in which no
    // input had changed proves it.  A thread may read exit[i - 1] while its owner rewrites it: it then decodes from the old
    // value, the owner has set `changed`, and the next round sees the difference to in[i].
    bool fixed = false;
    uint32_t rounds = 0;
    for (uint32_t round = 0; round <= nsub && !fixed; ++round, ++rounds) {
        if (tid == 0) changed = 0;
        __syncthreads();                                                            // also: the stores of the round before
        for (uint32_t i = tid; i < nsub; i += JD_THREADS) {
            if (i == 0) continue;                                                   // starts from the true state
            const jd_state in = w.exit[i - 1];
            if (in == w.in[i]) continue;
            uint32_t n;
            w.in[i] = in;
            w.exit[i] = jd_walk(x, words, i, in, &n);
            w.count[i] = n;
            changed = 1;
        }
        __syncthreads();
        fixed = changed == 0;
        __syncthreads();
    }
    if (!fixed && tid == 0) atomicOr(&status[first_image + blockIdx.x], JD_ST_ROUNDS);
    if (tid == 0) w.flags[1] = rounds;              // for measurements: re-decode rounds run, the last (idle) one included

    // first[i] = blocks completed in front of subsequence i
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nsub; base += JD_THREADS) {
        const uint32_t i = base + tid;
        const uint32_t v = i < nsub ? w.count[i] : 0;
        scan_lds[tid] = v;
        __syncthreads();
        for (int off = 1; off < JD_THREADS; off <<= 1) {
            const uint32_t a = tid >= off ? scan_lds[tid - off] : 0;
            __syncthreads();
            scan_lds[tid] += a;
            __syncthreads();
        }
        if (i < nsub) w.first[i] = carry + scan_lds[tid] - v;
        carry += scan_lds[JD_THREADS - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(JD_THREADS) void jpeg_entropy_write_kernel(const uint8_t* __restrict__ scans, uint8_t* __restrict__ coef,
                                                                       int* __restrict__ status, uint8_t* __restrict__ tmp,
                                                                       JpegScanChunk ch, int first_image) {
    __shared__ JdCtx x;
    const JpegScanImg& d = ch.d[blockIdx.y];
    if (!jd_enter(&x, scans, d)) return;
    if (blockIdx.x * (uint32_t)JD_THREADS >= x.nsub) return;                        // uniform
    const uint8_t* rec = scans + d.scan_off;
    jd_setup_tables(&x, rec, threadIdx.x, JD_THREADS);
    __syncthreads();
    const uint32_t i = blockIdx.x * (uint32_t)JD_THREADS + threadIdx.x;
    if (i >= x.nsub) return;
    const JdWork w = jd_work(tmp + d.tmp_off, d.nsub_cap);
    bool last;
    const int st = jd_write(x, (const uint32_t*)(rec + JD_SCAN_AT), i, w.in[i], w.first[i], coef + d.coef_off, &last);
    if (st) atomicOr(&status[first_image + blockIdx.y], st);
    if (last) w.flags[0] = 1;
}

__global__ __launch_bounds__(JD_THREADS) void jpeg_entropy_dc_kernel(const uint8_t* __restrict__ scans, uint8_t* __restrict__ coef,
                                                                    int* __restrict__ status, uint8_t* __restrict__ tmp,
                                                                    JpegScanChunk ch, int first_image) {
    __shared__ JdCtx x;
    __shared__ int scan_lds[JD_THREADS];
    const JpegScanImg& d = ch.d[blockIdx.y];
    if (!jd_enter(&x, scans, d)) return;
    const int c = blockIdx.x, tid = threadIdx.x;
    if (c >= (int)x.ncomp) return;
    if (tid == 0) jd_setup_dc_limit(&x, scans + d.scan_off, c);
    __syncthreads();
    int st = 0;
    if (c == 0 && tid == 0 && jd_work(tmp + d.tmp_off, d.nsub_cap).flags[0] == 0) st |= JD_ST_SHORT;
    uint8_t* rec = coef + d.coef_off;
    const uint32_t nblk = x.nblk[c];
    int carry = 0;                                  // |sum| <= 2^20 blocks * 2047 < 2^31
    for (uint32_t base = 0; base < nblk; base += JD_THREADS) {
        const uint32_t j = base + tid;
        scan_lds[tid] = j < nblk ? jd_dc_load(x, c, j, rec) : 0;
        __syncthreads();
        for (int off = 1; off < JD_THREADS; off <<= 1) {
            const int a = tid >= off ? scan_lds[tid - off] : 0;
            __syncthreads();
            scan_lds[tid] += a;
            __syncthreads();
        }
        if (j < nblk) st |= jd_dc_store(x, c, j, carry + scan_lds[tid], rec);
        carry += scan_lds[JD_THREADS - 1];
        __syncthreads();
    }
    if (st) atomicOr(&status[first_image + blockIdx.y], st);
}

}  // namespace

hipError_t launch_jpeg_entropy(const uint8_t* scans, const JpegScanImg* imgs, int n, uint8_t* coef, int* status, uint8_t* tmp,
                               hipStream_t s) {
    for (int lo = 0; lo < n; lo += JPEG_CHUNK) {
        const int nc = n - lo < JPEG_CHUNK ? n - lo : JPEG_CHUNK;
        JpegScanChunk ch{};
        unsigned long long max_bytes = 16, max_sub = 1;
        for (int i = 0; i < nc; ++i) {
            ch.d[i] = imgs[lo + i];
            if (ch.d[i].coef_size > max_bytes) max_bytes = ch.d[i].coef_size;
            if (ch.d[i].nsub_cap > max_sub) max_sub = ch.d[i].nsub_cap;
        }
        const unsigned per = JD_THREADS * 16;
        hipLaunchKernelGGL(jpeg_entropy_zero_kernel, dim3((unsigned)((max_bytes + per - 1) / per), nc), dim3(JD_THREADS), 0, s, scans,
                           coef, status, tmp, ch, lo);
        hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(nc), dim3(JD_THREADS), 0, s, scans, status, tmp, ch, lo);
        hipLaunchKernelGGL(jpeg_entropy_write_kernel, dim3((unsigned)((max_sub + JD_THREADS - 1) / JD_THREADS), nc), dim3(JD_THREADS), 0,
                           s, scans, coef, status, tmp, ch, lo);
        hipLaunchKernelGGL(jpeg_entropy_dc_kernel, dim3(3, nc), dim3(JD_THREADS), 0, s, scans, coef, status, tmp, ch, lo);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
