#!/usr/bin/env python
"""GPU time of the Huffman decode (gitmi_jpeg_entropy_batch) for one batch of 640x480 JPEGs written by Pillow from the
`photo` content of tools/jpeg_cases.py: event-timed calls, the re-decode rounds of the sync kernel per image (read from the
workspace) and the bytes moved.  One JSON line; --out writes it to a file as well (profiles/).  Under
`rocprofv3 --kernel-trace --stats -- python tools/jpeg_entropy_gpu_bench.py` the per-kernel times come from the profiler.

    python tools/jpeg_entropy_gpu_bench.py [--images 64] [--subsampling 2] [--quality 85] [--iters 20] [--out profiles/NAME.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--subsampling", type=int, default=2)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from generativeimage2text_amd import jpeg as J
    from tools import jpeg_cases as JC
    datas = [JC.encode(JC.content("photo", 640, 480, seed=100 + i), args.subsampling, args.quality) for i in range(args.images)]
    recs = [J.scan_prepare(d) for d in datas]
    refs = [J.entropy_decode(d) for d in datas]
    assert all(r is not None for r in recs + refs)
    host, offs = J.pack_records(recs)
    scan_desc = [(o, len(r)) for o, r in zip(offs, recs)]
    desc, total = [], 0
    for r in refs:
        desc.append((total, len(r)))
        total += (len(r) + 127) // 128 * 128
    scans = torch.from_numpy(host).cuda()
    coef = torch.empty(total, dtype=torch.uint8, device="cuda")
    status = torch.empty(len(recs), dtype=torch.int32, device="cuda")
    work = torch.empty(J.entropy_workspace_bytes(scan_desc), dtype=torch.uint8, device="cuda")
    J.entropy_batch_to(coef, desc, scans, scan_desc, status, workspace=work)
    assert status.tolist() == [0] * len(recs)
    flat = coef.cpu().numpy()
    assert all(np.array_equal(flat[o: o + b], ref) for (o, b), ref in zip(desc, refs)), "records differ from the host decoder's"
    # the workspace of image i begins with its flags: [1] = rounds
    rounds, at = [], 0
    wk = work.cpu().numpy()
    bits = J.SUBSEQUENCE_BITS
    for _, nbytes in scan_desc:
        rounds.append(int(wk[at + 4: at + 8].view("<u4")[0]))
        cap = max(1, ((nbytes - J.SCAN_AT) * 8 + bits - 1) // bits)
        at += (16 + 24 * cap + 127) // 128 * 128
    times = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        J.entropy_batch_to(coef, desc, scans, scan_desc, status, workspace=work)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    res = {"what": "gitmi_jpeg_entropy_batch on %d 640x480 photo JPEGs, subsampling %d, quality %d: microseconds per call between "
                   "two events (four launches), best and median of %d" % (args.images, args.subsampling, args.quality, args.iters),
           "call_us_best": round(min(times), 1), "call_us_median": round(float(np.median(times)), 1),
           "us_per_image": round(min(times) / args.images, 2),
           "scan_record_kb_mean": round(sum(len(r) for r in recs) / len(recs) / 1024, 1),
           "coefficient_record_kb_mean": round(sum(len(r) for r in refs) / len(refs) / 1024, 1),
           "subsequences_mean": round(float(np.mean([(J.scan_bytes_of(r) * 8 + bits - 1) // bits for r in recs])), 1),
           "sync_rounds_per_image": {"min": min(rounds), "mean": round(float(np.mean(rounds)), 2), "max": max(rounds)},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
