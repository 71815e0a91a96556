#!/usr/bin/env python
"""Host cost per image of a decode-pool worker, CPU only, single thread: the default body

    base64 -> Image.open(...).convert("RGB") -> tobytes() -> copy into the slot

against the jpeg="gpu" body

    base64 -> entropy decode (libgitmi_jpeg_host.so) straight into the slot

and the jpeg="gpu_entropy" body

    base64 -> scan_prepare (marker parse + FF 00 removal) straight into the slot

on 640x480 JPEGs written by Pillow from synthetic content with photographic statistics (smooth + texture + noise), at
quality 75 / 85 / 95, 4:2:0 and 4:4:4.  One JSON line; --out writes it to a file as well (profiles/).

    python tools/jpeg_host_bench.py [--images 200] [--distinct 16] [--repeats 3] [--out profiles/NAME.json]
"""
from __future__ import annotations

import argparse
import base64
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3, help="the best of this many passes is reported")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from PIL import Image, features
    from generativeimage2text_amd import jpeg as J
    from tools import jpeg_cases as JC
    slot = np.zeros(4 << 20, dtype=np.uint8)
    mem = memoryview(slot)
    sets = []
    for sub, sub_name in ((2, "4:2:0"), (0, "4:4:4")):
        for q in (75, 85, 95):
            raws = [base64.b64encode(JC.encode(JC.content("photo", 640, 480, seed=100 + i), sub, q)) for i in range(args.distinct)]
            rows = [raws[i % args.distinct] for i in range(args.images)]

            def pillow_body():
                for b64 in rows:
                    img = Image.open(io.BytesIO(base64.b64decode(b64))).convert("RGB")
                    w, h = img.size
                    mem[0: h * w * 3] = img.tobytes()

            def entropy_body():
                for b64 in rows:
                    rc, _ = J.entropy_decode_into(base64.b64decode(b64), slot.ctypes.data, slot.size)
                    assert rc == J.OK

            def scan_body():
                for b64 in rows:
                    rc, _, _ = J.scan_prepare_into(base64.b64decode(b64), slot.ctypes.data, slot.size)
                    assert rc == J.OK

            best = {}
            for name, body in (("pillow", pillow_body), ("entropy", entropy_body), ("scan", scan_body)):
                body()                                        # warm-up
                ts = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    body()
                    ts.append((time.perf_counter() - t0) / len(rows) * 1e6)
                best[name] = min(ts)
            sets.append({"subsampling": sub_name, "quality": q, "jpeg_kb": round(sum(len(r) for r in raws) * 3 / 4 / len(raws) / 1024, 1),
                         "pillow_body_us": round(best["pillow"], 1), "entropy_body_us": round(best["entropy"], 1),
                         "ratio": round(best["pillow"] / best["entropy"], 2), "scan_body_us": round(best["scan"], 1),
                         "scan_record_kb": round(sum(J.scan_prepare_into(base64.b64decode(r), None, 0)[2] for r in raws) / len(raws) / 1024, 1)})
            print("%s q%d: Pillow body %.0f us, entropy body %.0f us, ratio %.2f, scan body %.0f us" % (
                sub_name, q, best["pillow"], best["entropy"], best["pillow"] / best["entropy"], best["scan"]), file=sys.stderr, flush=True)
    res = {"what": "host microseconds per 640x480 image of one decode-pool worker body, one thread: default (base64 -> Pillow RGB -> "
                   "tobytes -> slot copy) vs jpeg='gpu' (base64 -> entropy decode into the slot) vs jpeg='gpu_entropy' (base64 -> "
                   "scan_prepare into the slot)",
           "images": args.images, "distinct": args.distinct, "pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"),
           "sets": sets}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
