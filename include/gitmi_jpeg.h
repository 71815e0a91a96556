/* gitmi_jpeg.h -- JPEG decoding split in two: entropy decode on the host, reconstruction on the GPU.
 *
 *   libgitmi_jpeg_host.so   gitmi_jpeg_entropy_decode(): marker parsing + Huffman decode of one baseline / extended sequential
 *                           JPEG into a COEFFICIENT RECORD.  Plain C++, no HIP: decode-pool workers load it and never open the GPU.
 *   libgitmi_jpeg.so        gitmi_jpeg_reconstruct_batch(): n records in one device buffer -> uint8 [H, W, 3] RGB per image,
 *                           bit for bit what Pillow's Image.open(...).convert("RGB") returns (libjpeg's JDCT_ISLOW inverse DCT,
 *                           fancy upsampling, fixed-point YCbCr -> RGB), in a fixed number of launches per 64 images.
 *
 * Both libraries are independent of libgitmi*.so and of include/gitmi.h (engine ABI 10 is unchanged).
 *
 * The coefficient record (little endian, natural alignment, all offsets relative to the start of the record):
 *
 *   gitmi_jpeg_header   GITMI_JPEG_HEADER_BYTES (640) bytes
 *   plane 0 .. ncomp-1  int16 [blocks_h][blocks_w][64] each, at comp[c].plane_offset (a multiple of 128):
 *                       still-quantised coefficients in NATURAL (row-major, de-zigzagged) order, padded to whole MCUs exactly
 *                       as the stream codes them; blocks the stream does not code do not exist.
 */
#ifndef GITMI_JPEG_H
#define GITMI_JPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GITMI_JPEG_ABI_VERSION 1
#define GITMI_JPEG_MAGIC 0x31434a47u /* "GJC1" */
#define GITMI_JPEG_HEADER_BYTES 640
#define GITMI_JPEG_MAX_DIM 16384     /* larger images take the Pillow path */

/* return codes of gitmi_jpeg_entropy_decode */
#define GITMI_JPEG_OK 0
#define GITMI_JPEG_UNSUPPORTED 1     /* not a JPEG, a JPEG outside the fast path, or ANY anomaly in the stream: decode it with Pillow */
#define GITMI_JPEG_NO_SPACE 2        /* supported so far, but the record needs info->record_bytes > out_cap; nothing was written */
#define GITMI_JPEG_BAD_ARGUMENT 3

typedef struct gitmi_jpeg_comp {
    uint8_t  h_samp, v_samp;         /* sampling factors (luma 1x1, 2x1 or 2x2; chroma 1x1) */
    uint8_t  tq;                     /* index into qt[] */
    uint8_t  reserved0;
    uint32_t blocks_w, blocks_h;     /* blocks of the plane = MCUs * sampling factor */
    uint32_t reserved1;
    uint64_t plane_offset;           /* bytes from the start of the record */
} gitmi_jpeg_comp;

typedef struct gitmi_jpeg_header {
    uint32_t magic;                  /* GITMI_JPEG_MAGIC */
    uint32_t header_bytes;           /* GITMI_JPEG_HEADER_BYTES */
    uint32_t width, height;
    uint32_t ncomp;                  /* 1 (grey) or 3 (YCbCr) */
    uint32_t mcus_w, mcus_h;
    uint32_t restart_interval;       /* of the stream; informational */
    uint64_t record_bytes;           /* header + planes */
    gitmi_jpeg_comp comp[3];
    uint16_t qt[4][64];              /* quantisation tables in natural order */
    uint8_t  pad[GITMI_JPEG_HEADER_BYTES - 112 - 512];
} gitmi_jpeg_header;

/* filled on GITMI_JPEG_OK and on GITMI_JPEG_NO_SPACE */
typedef struct gitmi_jpeg_info {
    uint32_t width, height;
    uint32_t ncomp;
    uint32_t h_samp, v_samp;         /* of the luma component: 1x1 = 4:4:4 (or grey), 2x1 = 4:2:2, 2x2 = 4:2:0 */
    uint32_t reserved;
    uint64_t record_bytes;
} gitmi_jpeg_info;

int gitmi_jpeg_abi_version(void);    /* exported by both libraries */

/* Host.  Reads only [jpg, jpg + n), writes only [out, out + out_cap).  Thread safe (no global state). */
int gitmi_jpeg_entropy_decode(const uint8_t* jpg, size_t n, void* out, size_t out_cap, gitmi_jpeg_info* info);

/* Device.  coef: n records in one DEVICE buffer of coef_bytes, record i at desc_host[i] (a multiple of 128).
 * rgb_desc_host: int64 [n][3] = (byte offset into rgb_out, H, W), the table gitmi_preprocess_batch takes; H and W must be
 * those of the record -- a record that says otherwise, or whose fields are not those of a record, is left unwritten: every
 * access is checked against coef_bytes / tmp_bytes / rgb_bytes on the device, whatever the bytes are.
 * tmp: device workspace of at least gitmi_jpeg_workspace_bytes(rgb_desc_host, n).
 * All launches go on `stream`; nothing synchronises.  Returns 0, or -1 (gitmi_jpeg_last_error()). */
size_t gitmi_jpeg_workspace_bytes(const int64_t* rgb_desc_host, int n);
int gitmi_jpeg_reconstruct_batch(const uint8_t* coef, size_t coef_bytes, const int64_t* desc_host, int n,
                                 uint8_t* tmp, size_t tmp_bytes, uint8_t* rgb_out, size_t rgb_bytes,
                                 const int64_t* rgb_desc_host, void* stream);
const char* gitmi_jpeg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
