/* gitmi_jpeg.h -- JPEG decoding split in two: entropy decode on the host, reconstruction on the GPU.
 *
 *   libgitmi_jpeg_host.so   gitmi_jpeg_entropy_decode(): marker parsing + Huffman decode of one baseline / extended sequential
 *                           JPEG into a COEFFICIENT RECORD.  Plain C++, no HIP: decode-pool workers load it and never open the GPU.
 *                           gitmi_jpeg_scan_prepare(): the same marker parsing, but the Huffman decode is left to the GPU: the
 *                           output is a SCAN RECORD (below) -- header, tables and the unstuffed entropy-coded bytes.
 *   libgitmi_jpeg.so        gitmi_jpeg_reconstruct_batch(): n records in one device buffer -> uint8 [H, W, 3] RGB per image,
 *                           bit for bit what Pillow's Image.open(...).convert("RGB") returns (libjpeg's JDCT_ISLOW inverse DCT,
 *                           fancy upsampling, fixed-point YCbCr -> RGB), in a fixed number of launches per 64 images.
 *                           gitmi_jpeg_entropy_batch(): n scan records -> n coefficient records, byte for byte what
 *                           gitmi_jpeg_entropy_decode() writes for the same files, in a fixed number of launches per 64 images.
 *
 * Both libraries are independent of libgitmi*.so and of include/gitmi.h (engine ABI 10 is unchanged).
 *
 * The coefficient record (little endian, natural alignment, all offsets relative to the start of the record):
 *
 *   gitmi_jpeg_header   GITMI_JPEG_HEADER_BYTES (640) bytes
 *   plane 0 .. ncomp-1  int16 [blocks_h][blocks_w][64] each, at comp[c].plane_offset (a multiple of 128):
 *                       still-quantised coefficients in NATURAL (row-major, de-zigzagged) order, padded to whole MCUs exactly
 *                       as the stream codes them; blocks the stream does not code do not exist.
 *
 * The scan record (little endian; what gitmi_jpeg_scan_prepare() writes and gitmi_jpeg_entropy_batch() reads):
 *
 *   gitmi_jpeg_header   the header of the coefficient record of this file, byte for byte; the GPU copies it
 *   gitmi_jpeg_scan     GITMI_JPEG_SCAN_BYTES (2304) bytes at offset 640: what the Huffman decode needs beside the header
 *   scan bytes          at scan_offset (2944): the entropy-coded segment with FF 00 -> FF, scan_bytes long, then zero bytes
 *                       (at least 8) up to scan_record_bytes
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

#define GITMI_JPEG_SCAN_MAGIC 0x31534a47u /* "GJS1" */
#define GITMI_JPEG_SCAN_BYTES 2304
#define GITMI_JPEG_SCAN_MAX_BLOCKS (1u << 20) /* per component: 32-bit DC prefix sums stay below 2^31 */
#define GITMI_JPEG_SCAN_MAX_BYTES (1u << 28)  /* unstuffed scan: bit positions fit 32 bits */

typedef struct gitmi_jpeg_dht {
    uint8_t counts[16];              /* codes of length 1 .. 16 */
    uint8_t symbols[256];            /* in code order; sum(counts) of them are used */
} gitmi_jpeg_dht;

typedef struct gitmi_jpeg_scan {
    uint32_t magic;                  /* GITMI_JPEG_SCAN_MAGIC */
    uint32_t scan_struct_bytes;      /* GITMI_JPEG_SCAN_BYTES */
    uint32_t ncomp;                  /* as in the header */
    uint32_t blocks_per_mcu;         /* sum of h_samp * v_samp */
    uint32_t total_blocks;           /* mcus_w * mcus_h * blocks_per_mcu */
    uint32_t scan_bytes;             /* unstuffed entropy-coded bytes, EOI not included */
    uint64_t scan_offset;            /* of the scan bytes from the start of the record: 640 + 2304 */
    uint64_t scan_record_bytes;      /* header + this + scan bytes + zero padding, a multiple of 16 */
    uint8_t  td[4], ta[4];           /* per component: index into dc[] / ac[] */
    uint8_t  reserved[80];
    gitmi_jpeg_dht dc[4], ac[4];     /* the DHT tables the components name; the others are zero */
} gitmi_jpeg_scan;

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

/* Host.  The marker parsing of gitmi_jpeg_entropy_decode (the same code: what the one declines in front of the scan the other
 * declines), then the scan record instead of the Huffman decode.  Same return codes and sizing protocol, with
 * *scan_record_bytes (may be NULL) in the role info->record_bytes has there: filled on OK and NO_SPACE; info->record_bytes is
 * the size of the COEFFICIENT record.  Additionally GITMI_JPEG_UNSUPPORTED for: a restart interval, any marker inside the scan
 * but the terminating FF D9, a missing EOI, more than GITMI_JPEG_SCAN_MAX_BLOCKS blocks in a component, a scan of
 * GITMI_JPEG_SCAN_MAX_BYTES or more.  Those go to gitmi_jpeg_entropy_decode.  An OK says nothing about the Huffman data:
 * the GPU's status word does. */
int gitmi_jpeg_scan_prepare(const uint8_t* jpg, size_t n, void* out, size_t out_cap, gitmi_jpeg_info* info,
                            uint64_t* scan_record_bytes);

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

/* Device.  Huffman decode of n scan records: scans is one DEVICE buffer of scans_bytes, scan_desc_host int64 [n][2] =
 * (byte offset, a multiple of 128; bytes of the record).  Coefficient record i goes to coef_out + coef_desc_host[i][0] (a
 * multiple of 128) and must be coef_desc_host[i][1] = info->record_bytes long; the layout is what
 * gitmi_jpeg_reconstruct_batch takes and the bytes are those of gitmi_jpeg_entropy_decode.  status: DEVICE int32 [n], 0: the
 * record is complete; non-zero: the scan record does not check out or the stream has an anomaly (the host decoder would
 * return GITMI_JPEG_UNSUPPORTED) -- the record's bytes are then undefined (never outside its coef_desc range) and the caller
 * decodes that image another way.  Every field of a scan record is validated on the device against scans_bytes, the desc
 * sizes and tmp before an address is formed; a record that does not check out gets its status and no other store.
 * tmp: device workspace of at least gitmi_jpeg_entropy_workspace_bytes(scan_desc_host, n), 128-byte aligned.
 * Four launches per 64 images, all on `stream`; nothing synchronises.  Returns 0, or -1 (gitmi_jpeg_last_error()). */
size_t gitmi_jpeg_entropy_workspace_bytes(const int64_t* scan_desc_host, int n);
int gitmi_jpeg_entropy_batch(const uint8_t* scans, size_t scans_bytes, const int64_t* scan_desc_host, int n,
                             uint8_t* coef_out, size_t coef_bytes, const int64_t* coef_desc_host, int32_t* status,
                             uint8_t* tmp, size_t tmp_bytes, void* stream);
/* compile-time constants of the GPU Huffman decode: which = 0: bits per subsequence, 1: threads per workgroup,
 * 2: subsequences a thread takes per pass of its strided walk (1: thread t walks t, t + threads, ...); anything else: 0 */
int gitmi_jpeg_entropy_constant(int which);

#ifdef __cplusplus
}
#endif
#endif
