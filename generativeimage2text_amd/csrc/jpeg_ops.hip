// Entry points of libgitmi_jpeg.so (include/gitmi_jpeg.h): argument checks on the host, then the two launches of
// kernels_jpeg.hip per JPEG_CHUNK images.  Independent of libgitmi*.so.
#include "jpeg_common.h"

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
