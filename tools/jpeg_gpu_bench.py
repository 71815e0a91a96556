#!/usr/bin/env python
"""GPU cost of the JPEG reconstruction: ONE gitmi_jpeg_reconstruct_batch call on 64 images of 640x480 4:2:0 (records already
on the device), timed with device events, and the bytes the two kernels must move.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/jpeg_gpu_bench.py` (on its own, no counters) for the per-kernel times:
the kernels are jpeg_idct_kernel and jpeg_color_kernel.  Needs the GPU.  One JSON line.

    python tools/jpeg_gpu_bench.py [--images 64] [--iters 50] [--quality 85] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from generativeimage2text_amd import jpeg as J
    from tools import jpeg_cases as JC
    assert torch.cuda.is_available(), "jpeg_gpu_bench needs the GPU"
    W, H = 640, 480
    datas = [JC.encode(JC.content("photo", W, H, seed=100 + i), 2, args.quality) for i in range(min(args.images, 16))]
    recs = [J.entropy_decode(d) for d in datas]
    recs = [recs[i % len(recs)] for i in range(args.images)]
    host, offs = J.pack_records(recs)
    coef = torch.from_numpy(host).cuda()
    per = (H * W * 3 + 63) // 64 * 64
    desc = [(i * per, H, W) for i in range(args.images)]
    rgb = torch.empty(per * args.images, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        J.decode_batch_to(rgb, desc, coef, offs)
    torch.cuda.synchronize()
    ref = JC.pillow_rgb(datas[0])
    assert (rgb[:H * W * 3].view(H, W, 3).cpu().numpy() == ref).all(), "reconstruction differs from Pillow"
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.iters):
        J.decode_batch_to(rgb, desc, coef, offs)
    t1.record()
    torch.cuda.synchronize()
    call_us = t0.elapsed_time(t1) * 1e3 / args.iters
    # bytes each kernel must move per image: coefficients in (2 B x 1.5 per pixel at 4:2:0, MCU-padded) + planes out;
    # planes in (1.5 B per pixel) + RGB out (3 B per pixel)
    coef_bytes = len(recs[0]) - J.HEADER_BYTES
    idct_bytes = (coef_bytes + coef_bytes // 2) * args.images
    color_bytes = (coef_bytes // 2 + H * W * 3) * args.images
    res = {"what": "one gitmi_jpeg_reconstruct_batch call, %d images of %dx%d 4:2:0 q%d, records resident" % (args.images, W, H, args.quality),
           "call_us_device_events": round(call_us, 1), "us_per_image": round(call_us / args.images, 2),
           "idct_bytes": idct_bytes, "color_bytes": color_bytes,
           "call_GBps_over_both_kernels": round((idct_bytes + color_bytes) / call_us / 1e3, 1)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
