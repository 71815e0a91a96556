#!/usr/bin/env python
"""Image memory snapshots (GITMI_SEARCH_KEEP / GITMI_SEARCH_RECALL, include/gitmi.h) against the full call they replace, with
the benchmark's synthetic weights: GIT_BASE at 224 x 224, 64 images, greedy captions, one context alone, hipGraph on.

Interleaved, iteration by iteration:
  recall_followup  RECALL of the 64 kept images (the context holds another batch at that moment), then the greedy follow-up
  full             the full call with the same sentences: image encoder + prefill + decode.  This change does not touch that
                   path: the figure is the parent commit's.
Alone, each between two events on the stream and as wall time (both calls synchronise the stream themselves):
  keep, recall
and, from gitmi_profile_enable(e, 2), the encode + prefill graph a RECALL stands in for.  The result says whether the recalled
follow-up is bit-equal to the follow-up over the originally encoded batch.

    python tools/memory_bench.py [--precision f16] [--batch 64] [--iters 20] [--out FILE]
Prints one JSON object (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from generativeimage2text_amd.configs import config_for_model  # noqa: E402
from generativeimage2text_amd.engine import Engine  # noqa: E402
from generativeimage2text_amd.synthetic import random_state_dict  # noqa: E402

MAX_STEPS = 20


def median(ts) -> float:
    ts = sorted(ts)
    return ts[len(ts) // 2]


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def between_events(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bit_equal(a, b) -> bool:
    return all(torch.equal(x.cpu().view(torch.int32) if x.dtype == torch.float32 else x.cpu(),
                           y.cpu().view(torch.int32) if y.dtype == torch.float32 else y.cpu()) for x, y in zip(a, b))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("memory_bench needs the MI355X")
    torch.cuda.set_device(0)
    B = a.batch
    cfg = config_for_model("GIT_BASE")
    g = torch.Generator().manual_seed(7)
    frames = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda()]
    others = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda()]
    eng = Engine(cfg, precision=a.precision, max_batch=B, max_beams=1, max_frames=1, max_text_len=MAX_STEPS)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    search = Engine.make_search("greedy", MAX_STEPS, 1, 1)
    slots = list(range(B))
    store = eng.memory_store(B)

    full = lambda: eng.generate(frames, search)                         # noqa: E731
    follow = lambda: eng.generate(None, search)                         # noqa: E731
    full()
    want = follow()
    kept = eng.keep(store, slots)
    geometry = kept["geometry"]

    def recall_followup():
        eng.recall(store, slots, geometry)
        return follow()

    eng.generate(others, search)                                        # another batch is resident when the recall arrives
    got = recall_followup()
    res = {"model": "GIT_BASE", "hw": [cfg.image_size, cfg.image_size], "images": B, "precision": a.precision,
           "max_steps": MAX_STEPS, "slot_bytes": eng.memory_slot_bytes(), "store_mb": round(store.numel() / 1e6, 1),
           "rows_per_image": kept["max_rows"], "outputs_equal": bit_equal(want, got)}
    for _ in range(3):
        recall_followup(), full()
    t_a, t_b = [], []
    for _ in range(a.iters):                                            # interleaved: a, b, a, b, ...
        eng.generate(others, search)
        t_a.append(wall(recall_followup))
        t_b.append(wall(full))
    res["recall_followup_ms"] = round(median(t_a), 3)
    res["full_ms"] = round(median(t_b), 3)
    res["followup_ms"] = round(median([wall(follow) for _ in range(a.iters)]), 3)
    full()
    res["keep_event_ms"] = round(median([between_events(lambda: eng.keep(store, slots)) for _ in range(a.iters)]), 3)
    res["keep_wall_ms"] = round(median([wall(lambda: eng.keep(store, slots)) for _ in range(a.iters)]), 3)
    res["recall_event_ms"] = round(median([between_events(lambda: eng.recall(store, slots, geometry)) for _ in range(a.iters)]), 3)
    res["recall_wall_ms"] = round(median([wall(lambda: eng.recall(store, slots, geometry)) for _ in range(a.iters)]), 3)
    full()
    eng.profile_enable(2)
    for _ in range(5):
        full()
    p = eng.profile_read()
    eng.profile_enable(0)
    res["encode_prefill_ms"] = round(p["vit_ms"], 3)
    res["decode_ms"] = round(p["decode_ms"], 3)
    res["recall_over_encode_prefill"] = round(res["recall_wall_ms"] / res["encode_prefill_ms"], 3)
    res["full_over_recall_followup"] = round(res["full_ms"] / res["recall_followup_ms"], 2)
    eng.close()
    out = {"tool": "memory_bench", "hip_graph": True,
           "timing": "median ms; wall = between device synchronisations, event = between two events on the stream", "result": res}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
