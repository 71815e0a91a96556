"""numpy restatement of the GPU half of the split JPEG decode (csrc/kernels_jpeg.hip): a coefficient record of
libgitmi_jpeg_host.so (include/gitmi_jpeg.h) -> uint8 [H, W, 3], bit for bit what Pillow's
Image.open(...).convert("RGB") returns.  CPU only; tests/test_jpeg_host.py pins it against Pillow over its sweep, which is how
the edge rules below were settled before any kernel was written.

The arithmetic is libjpeg's default reconstruction:
  * jpeg_idct_islow: 13-bit constants, PASS1_BITS = 2, columns then rows, DESCALE rounding, +128 and a clamp to [0, 255]
    (the all-zero-AC shortcuts of the C source give the values of the full path, so only the full path is written);
  * fancy (triangle) upsampling of the chroma planes for h2v1 and h2v2, over the REAL downsampled samples only
    (ceil(W / 2) columns, ceil(H / 2) rows: the block padding is never read), edges replicated; plain replication when the
    downsampled width is 2 or less (libjpeg picks the box filter there);
  * ycc_rgb_convert's 16.16 fixed-point tables.
"""
from __future__ import annotations

import struct

import numpy as np

HEADER_BYTES = 640
MAGIC = 0x31434A47
_HEAD = struct.Struct("<8IQ")           # magic, header_bytes, width, height, ncomp, mcus_w, mcus_h, restart_interval, record_bytes
_COMP = struct.Struct("<4B3IQ")         # h_samp, v_samp, tq, -, blocks_w, blocks_h, -, plane_offset

C_0_298631336, C_0_390180644, C_0_541196100, C_0_765366865 = 2446, 3196, 4433, 6270
C_0_899976223, C_1_175875602, C_1_501321110, C_1_847759065 = 7373, 9633, 12299, 15137
C_1_961570560, C_2_053119869, C_2_562915447, C_3_072711026 = 16069, 16819, 20995, 25172


def parse_record(rec) -> dict:
    """bytes / uint8 array -> {"width", "height", "ncomp", "comps": [(h, v, tq, coefficients int16 [bh, bw, 64])], "qt"}"""
    raw = np.frombuffer(bytes(rec), dtype=np.uint8) if not isinstance(rec, np.ndarray) else rec
    head = _HEAD.unpack_from(raw, 0)
    assert head[0] == MAGIC and head[1] == HEADER_BYTES, "not a coefficient record"
    out = {"width": head[2], "height": head[3], "ncomp": head[4], "mcus_w": head[5], "mcus_h": head[6],
           "restart_interval": head[7], "record_bytes": head[8], "comps": []}
    out["qt"] = np.frombuffer(raw[112:624].tobytes(), dtype="<u2").reshape(4, 64)
    for c in range(out["ncomp"]):
        h, v, tq, _, bw, bh, _, off = _COMP.unpack_from(raw, 40 + 24 * c)
        coef = np.frombuffer(raw[off: off + bh * bw * 128].tobytes(), dtype="<i2").reshape(bh, bw, 64)
        out["comps"].append((h, v, tq, coef))
    return out


def _idct_1d(i0, i1, i2, i3, i4, i5, i6, i7, shift):
    z1 = (i2 + i6) * C_0_541196100
    tmp2 = z1 - i6 * C_1_847759065
    tmp3 = z1 + i2 * C_0_765366865
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C_1_175875602
    t0 = t0 * C_0_298631336
    t1 = t1 * C_2_053119869
    t2 = t2 * C_3_072711026
    t3 = t3 * C_1_501321110
    z1 = -z1 * C_0_899976223
    z2 = -z2 * C_2_562915447
    z3 = -z3 * C_1_961570560 + z5
    z4 = -z4 * C_0_390180644 + z5
    t0 = t0 + z1 + z3
    t1 = t1 + z2 + z4
    t2 = t2 + z2 + z3
    t3 = t3 + z1 + z4
    r = 1 << (shift - 1)
    return [(tmp10 + t3 + r) >> shift, (tmp11 + t2 + r) >> shift, (tmp12 + t1 + r) >> shift, (tmp13 + t0 + r) >> shift,
            (tmp13 - t0 + r) >> shift, (tmp12 - t1 + r) >> shift, (tmp11 - t2 + r) >> shift, (tmp10 - t3 + r) >> shift]


def idct_plane(coef: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """int16 [bh, bw, 64] quantised coefficients, uint16 [64] quantiser (both natural order) -> uint8 [bh * 8, bw * 8]"""
    bh, bw, _ = coef.shape
    x = (coef.astype(np.int64) * qt.astype(np.int64)).reshape(bh, bw, 8, 8)
    ws = np.stack(_idct_1d(*[x[:, :, k, :] for k in range(8)], shift=13 - 2), axis=2)            # columns -> [bh, bw, row, col]
    px = np.stack(_idct_1d(*[ws[:, :, :, k] for k in range(8)], shift=13 + 2 + 3), axis=3)       # rows
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample(plane: np.ndarray, H: int, W: int, h2: bool, v2: bool) -> np.ndarray:
    """a chroma plane at block-padded size -> int [H, W] at full resolution"""
    if not h2 and not v2:
        return plane[:H, :W].astype(np.int64)
    cw, ch = (W + 1) // 2, ((H + 1) // 2 if v2 else H)
    c = plane[:ch, :cw].astype(np.int64)
    if cw <= 2:                                             # libjpeg: no fancy upsampling at a downsampled width of 2 or less
        c = np.repeat(c, 2, axis=1)
        if v2:
            c = np.repeat(c, 2, axis=0)
        return c[:H, :W]
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    if not v2:                                              # h2v1: 3:1, +1 / +2
        out = np.empty((ch, 2 * cw), dtype=np.int64)
        out[:, 0::2] = (3 * c + left + 1) >> 2
        out[:, 1::2] = (3 * c + right + 2) >> 2
        return out[:H, :W]
    up = np.concatenate([c[:1], c[:-1]], axis=0)
    down = np.concatenate([c[1:], c[-1:]], axis=0)
    s = np.empty((2 * ch, cw), dtype=np.int64)              # column sums 3 * near + far
    s[0::2] = 3 * c + up
    s[1::2] = 3 * c + down
    sl = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    sr = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 0::2] = (3 * s + sl + 8) >> 4
    out[:, 1::2] = (3 * s + sr + 7) >> 4
    return out[:H, :W]


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr) -> np.ndarray:
    cb, cr = cb - 128, cr - 128
    r = y + ((_fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def reconstruct(rec) -> np.ndarray:
    """a coefficient record -> uint8 [H, W, 3]"""
    r = parse_record(rec)
    H, W = r["height"], r["width"]
    planes = [idct_plane(coef, r["qt"][tq]) for _, _, tq, coef in r["comps"]]
    if r["ncomp"] == 1:
        return np.repeat(planes[0][:H, :W, None], 3, axis=2)
    h2, v2 = r["comps"][0][0] == 2, r["comps"][0][1] == 2
    y = planes[0][:H, :W].astype(np.int64)
    return ycc_to_rgb(y, upsample(planes[1], H, W, h2, v2), upsample(planes[2], H, W, h2, v2))
