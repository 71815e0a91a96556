// Shared by kernels_jpeg.hip (kernels + launcher) and jpeg_ops.hip (entry points of include/gitmi_jpeg.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gitmi_jpeg.h"

constexpr int JPEG_CHUNK = 64;                      // images per launch pair: their descriptors travel as kernel arguments

struct JpegImg {
    unsigned long long coef_off;                    // the record in the coefficient buffer (a multiple of 128)
    unsigned long long tmp_off;                     // this image's component planes in the workspace
    unsigned long long rgb_off;                     // uint8 [H, W, 3] in the output (a multiple of 4)
    int H, W;                                       // from the caller's table; the record must agree
};
struct JpegChunk { JpegImg d[JPEG_CHUNK]; };

// bytes of component planes an H x W image can need, whatever its sampling: 4:4:4 (3 planes padded to 8), 4:2:2
// (luma padded to 16 x 8 + 2 half-width planes), 4:2:0 (luma padded to 16 x 16 + 2 quarter planes); rounded to 128
__host__ __device__ inline size_t jpeg_plane_bytes_bound(long long H, long long W) {
    const size_t w8 = (size_t)(W + 7) / 8 * 8, h8 = (size_t)(H + 7) / 8 * 8, w16 = (size_t)(W + 15) / 16 * 16, h16 = (size_t)(H + 15) / 16 * 16;
    size_t a = 3 * w8 * h8, b = 2 * w16 * h8, c = w16 * h16 * 3 / 2;
    if (b > a) a = b;
    if (c > a) a = c;
    return (a + 127) / 128 * 128;
}

// gitmi_jpeg_entropy_batch: one image of a launch group; all sizes are the CALLER's, the device checks the record against them
struct JpegScanImg {
    unsigned long long scan_off, scan_size;         // the scan record in the scan buffer (offset a multiple of 128)
    unsigned long long coef_off, coef_size;         // the coefficient record to write (offset a multiple of 128)
    unsigned long long tmp_off;                     // this image's part of the workspace (a multiple of 128)
    unsigned long long nsub_cap;                    // subsequences that part holds
};
struct JpegScanChunk { JpegScanImg d[JPEG_CHUNK]; };

hipError_t launch_jpeg_entropy(const uint8_t* scans, const JpegScanImg* imgs, int n, uint8_t* coef, int* status, uint8_t* tmp,
                               hipStream_t s);
hipError_t launch_jpeg_reconstruct(const uint8_t* coef, size_t coef_bytes, const JpegImg* imgs, int n, uint8_t* tmp, uint8_t* rgb,
                                   hipStream_t s);
