"""The JPEG sweep shared by tests/test_jpeg_host.py, tests/test_gpu_jpeg.py and tools/jpeg_host_bench.py: images written by
Pillow from seeded content, so nothing is stored.  One case = (name, JPEG bytes)."""
from __future__ import annotations

import io

import numpy as np

SIZES = [(1, 1), (7, 5), (8, 8), (9, 9), (15, 17), (16, 16), (17, 33), (33, 17), (64, 48), (100, 75)]      # (w, h)
MODES = [0, 1, 2, "L"]                    # Pillow's subsampling= 0 (4:4:4), 1 (4:2:2), 2 (4:2:0); mode L
QUALITIES = [30, 75, 95, 100]
CONTENTS = ["noise", "gradient", "flat", "checker"]


def content(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    """uint8 [h, w, 3]"""
    rng = np.random.RandomState(seed)
    if kind == "noise":                   # saturates the range limit and the colour tables
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1).astype(np.uint8)
    if kind == "flat":                    # DC-only blocks
        return np.broadcast_to(np.array([200, 30, 90], dtype=np.uint8), (h, w, 3)).copy()
    if kind == "checker":
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if kind == "photo":                   # smooth + texture + noise: photographic statistics for the host benchmark
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.empty((h, w, 3))
        for c in range(3):
            p = rng.uniform(0.5, 2.0, 6)
            smooth = 110 + 70 * np.sin(x / w * 3 * p[0] + p[1]) * np.cos(y / h * 3 * p[2])
            texture = 25 * np.sin(x / (3 + p[3])) * np.sin(y / (2 + p[4])) + 12 * np.sign(np.sin((x + 2 * y) / (5 + p[5])))
            img[:, :, c] = smooth + texture + rng.normal(0, 6, (h, w))
        return np.clip(img, 0, 255).astype(np.uint8)
    raise ValueError(kind)


def encode(arr: np.ndarray, mode, quality: int, **kw) -> bytes:
    from PIL import Image
    im = Image.fromarray(arr)
    buf = io.BytesIO()
    if mode == "L":
        im.convert("L").save(buf, format="JPEG", quality=quality, **kw)
    else:
        im.save(buf, format="JPEG", quality=quality, subsampling=mode, **kw)
    return buf.getvalue()


def sweep(qualities=QUALITIES):
    """every (size, subsampling, quality, content) case, then the variants: custom Huffman tables and restart markers"""
    for q in qualities:
        for w, h in SIZES:
            for mode in MODES:
                for i, kind in enumerate(CONTENTS):
                    yield "%dx%d-s%s-q%d-%s" % (w, h, mode, q, kind), encode(content(kind, w, h, seed=w * 131 + h + i), mode, q)
        for mode in MODES:
            for w, h in SIZES:
                yield "%dx%d-s%s-q%d-optimize" % (w, h, mode, q), encode(content("noise", w, h, seed=7), mode, q, optimize=True)
            for w, h in ((33, 17), (64, 48)):
                for kw in (dict(restart_marker_blocks=1), dict(restart_marker_rows=1)):
                    yield ("%dx%d-s%s-q%d-%s" % (w, h, mode, q, next(iter(kw))),
                           encode(content("noise", w, h, seed=11), mode, q, **kw))


def pillow_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
