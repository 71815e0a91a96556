// Entry points of libgitmi_jpeg.so (include/gitmi_jpeg.h): argument checks on the host, then the two launches of
// kernels_jpeg.hip (reconstruction) or the four of kernels_jpeg_entropy.hip (Huffman decode) per JPEG_CHUNK images.  Independent of libgitmi*.so.
#include "jpeg_common.h"
#include "jpeg_entropy_dev.h"

#include <stdarg.h>
#include <stdio.h>

#include <vector>

namespace {
thread_local char g_error[512];

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return -1;
}

bool bad_dims(const int64_t* t) { return t[1] < 1 || t[2] < 1 || t[1] > GITMI_JPEG_MAX_DIM || t[2] > GITMI_JPEG_MAX_DIM; }
}  // namespace

extern "C" int gitmi_jpeg_abi_version(void) { return GITMI_JPEG_ABI_VERSION; }
extern "C" const char* gitmi_jpeg_last_error(void) { return g_error; }

extern "C" size_t gitmi_jpeg_workspace_bytes(const int64_t* rgb_desc_host, int n) {
    size_t need = 0;
    for (int i = 0; rgb_desc_host && i < n; ++i) {
        if (bad_dims(rgb_desc_host + 3 * i)) return 0;
        need += jpeg_plane_bytes_bound(rgb_desc_host[3 * i + 1], rgb_desc_host[3 * i + 2]);
    }
    return need;
}

extern "C" int gitmi_jpeg_reconstruct_batch(const uint8_t* coef, size_t coef_bytes, const int64_t* desc_host, int n, uint8_t* tmp,
                                            size_t tmp_bytes, uint8_t* rgb_out, size_t rgb_bytes, const int64_t* rgb_desc_host,
                                            void* stream) {
    if (!coef || !desc_host || !tmp || !rgb_out || !rgb_desc_host || n < 1) return fail("jpeg_reconstruct_batch: bad argument");
    if (((uintptr_t)coef & 127) || ((uintptr_t)rgb_out & 3) || ((uintptr_t)tmp & 127))
        return fail("jpeg_reconstruct_batch: coef and tmp must be 128-byte aligned, rgb_out 4-byte aligned");
    std::vector<JpegImg> imgs((size_t)n);
    size_t used = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t off = desc_host[i], roff = rgb_desc_host[3 * i], H = rgb_desc_host[3 * i + 1], W = rgb_desc_host[3 * i + 2];
        if (bad_dims(rgb_desc_host + 3 * i)) return fail("jpeg_reconstruct_batch: image %d: %lld x %lld is not a size this path takes", i, (long long)H, (long long)W);
        if (off < 0 || (off & 127) || (uint64_t)off > coef_bytes || coef_bytes - (uint64_t)off < GITMI_JPEG_HEADER_BYTES)
            return fail("jpeg_reconstruct_batch: record %d (offset %lld) does not lie 128-byte aligned inside the %zu coefficient bytes", i,
                        (long long)off, coef_bytes);
        if (roff < 0 || (roff & 3) || (uint64_t)roff > rgb_bytes || rgb_bytes - (uint64_t)roff < (uint64_t)H * W * 3)
            return fail("jpeg_reconstruct_batch: image %d (offset %lld, %lld x %lld) does not lie 4-byte aligned inside the %zu output bytes",
                        i, (long long)roff, (long long)H, (long long)W, rgb_bytes);
        imgs[i].coef_off = (unsigned long long)off;
        imgs[i].tmp_off = used;
        imgs[i].rgb_off = (unsigned long long)roff;
        imgs[i].H = (int)H;
        imgs[i].W = (int)W;
        used += jpeg_plane_bytes_bound(H, W);
    }
    if (used > tmp_bytes) return fail("jpeg_reconstruct_batch: workspace must hold %zu bytes", used);
    const hipError_t e = launch_jpeg_reconstruct(coef, coef_bytes, imgs.data(), n, tmp, rgb_out, (hipStream_t)stream);
    if (e != hipSuccess) return fail("jpeg_reconstruct_batch: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int gitmi_jpeg_entropy_constant(int which) {
    return which == 0 ? JD_SUB_BITS : which == 1 ? JD_THREADS : which == 2 ? 1 : 0;       // a thread walks subsequences tid, tid + JD_THREADS, ...: one per pass
}

extern "C" size_t gitmi_jpeg_entropy_workspace_bytes(const int64_t* scan_desc_host, int n) {
    size_t need = 0;
    for (int i = 0; scan_desc_host && i < n; ++i) {
        const int64_t bytes = scan_desc_host[2 * i + 1];
        if (bytes < 0) return 0;
        need += (size_t)jd_workspace_bytes(jd_nsub_bound((uint64_t)bytes));
    }
    return need;
}

extern "C" int gitmi_jpeg_entropy_batch(const uint8_t* scans, size_t scans_bytes, const int64_t* scan_desc_host, int n, uint8_t* coef_out,
                                        size_t coef_bytes, const int64_t* coef_desc_host, int32_t* status, uint8_t* tmp, size_t tmp_bytes,
                                        void* stream) {
    if (!scans || !scan_desc_host || !coef_out || !coef_desc_host || !status || !tmp || n < 1) return fail("jpeg_entropy_batch: bad argument");
    if (((uintptr_t)scans & 127) || ((uintptr_t)coef_out & 127) || ((uintptr_t)tmp & 127) || ((uintptr_t)status & 3))
        return fail("jpeg_entropy_batch: scans, coef_out and tmp must be 128-byte aligned, status 4-byte aligned");
    std::vector<JpegScanImg> imgs((size_t)n);
    size_t used = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t off = scan_desc_host[2 * i], bytes = scan_desc_host[2 * i + 1];
        const int64_t coff = coef_desc_host[2 * i], cbytes = coef_desc_host[2 * i + 1];
        if (off < 0 || (off & 127) || bytes < (int64_t)(JD_SCAN_AT + 8) || (uint64_t)off > scans_bytes || scans_bytes - (uint64_t)off < (uint64_t)bytes)
            return fail("jpeg_entropy_batch: scan record %d (offset %lld, %lld bytes) does not lie 128-byte aligned inside the %zu scan bytes",
                        i, (long long)off, (long long)bytes, scans_bytes);
        if (coff < 0 || (coff & 127) || cbytes < GITMI_JPEG_HEADER_BYTES || (cbytes & 127) || (uint64_t)coff > coef_bytes ||
            coef_bytes - (uint64_t)coff < (uint64_t)cbytes)
            return fail("jpeg_entropy_batch: coefficient record %d (offset %lld, %lld bytes) does not lie 128-byte aligned inside the %zu "
                        "output bytes", i, (long long)coff, (long long)cbytes, coef_bytes);
        imgs[i].scan_off = (unsigned long long)off;
        imgs[i].scan_size = (unsigned long long)bytes;
        imgs[i].coef_off = (unsigned long long)coff;
        imgs[i].coef_size = (unsigned long long)cbytes;
        imgs[i].tmp_off = used;
        imgs[i].nsub_cap = jd_nsub_bound((uint64_t)bytes);
        used += (size_t)jd_workspace_bytes(imgs[i].nsub_cap);
    }
    if (used > tmp_bytes) return fail("jpeg_entropy_batch: workspace must hold %zu bytes", used);
    const hipError_t e = launch_jpeg_entropy(scans, imgs.data(), n, coef_out, status, tmp, (hipStream_t)stream);
    if (e != hipSuccess) return fail("jpeg_entropy_batch: %s", hipGetErrorString(e));
    return 0;
}
