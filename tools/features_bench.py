#!/usr/bin/env python
"""Features in (GITMI_SEARCH_FEATURES, include/gitmi.h; model.FeatureStore) against the calls it replaces, with the benchmark's
synthetic weights, f16, one context alone, hipGraph on.  Numbers, not thresholds: medians of wall time between device
synchronisations, the legs of a comparison interleaved iteration by iteration.

  video   GIT_BASE_VATEX (6 frames), 16 videos, a caption per window, the window sliding by one frame:
            list      the list-form call with the 6 frames of the window: 6 x 16 images through the image encoder
            store     the ONE new frame of every video encoded into a FeatureStore (put), recall of the 16 slid windows
                      (install + prefill), the greedy follow-up (decode); the three parts are also timed apart
  image   GIT_BASE, 64 images, greedy captions:
            features  FeatureStore.recall of the 64 images + the greedy follow-up
            memory    ImageStore.recall of the same images + the same follow-up
            full      the full call: image encoder + prefill + decode
          and the bytes per image of both stores.

    python tools/features_bench.py [--iters 20] [--only video|image] [--out FILE]
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
from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel, FeatureStore, ImageStore  # noqa: E402
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


def make_model(name: str, B: int, precision: str) -> CaptioningModel:
    cfg = config_for_model(name)
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=MAX_STEPS, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision=precision, max_batch=B, max_text_len=MAX_STEPS)
    model.load_state_dict(random_state_dict(cfg, seed=1234))
    return model


def video(a) -> dict:
    B, F = 16, 6
    model = make_model("GIT_BASE_VATEX", B, a.precision)
    cfg, eng = model.cfg, model.engine
    search = Engine.make_search("greedy", MAX_STEPS, 1, 1)
    g = torch.Generator().manual_seed(11)
    n_frames = F + 3 + a.iters
    clip = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda() for _ in range(n_frames)]
    store = FeatureStore(model, B * (F + 1), dtype=torch.float32)
    for t in range(F):
        store.put(clip[t], [(v, t) for v in range(B)])
    windows = lambda t0: [[(v, t0 + i) for i in range(F)] for v in range(B)]                    # noqa: E731
    state = {}

    def list_call(t0):
        eng.set_temporal_embedding(True)
        state["list"] = eng.generate(clip[t0:t0 + F], search)

    def put(t0):
        store.put(clip[t0 + F - 1], [(v, t0 + F - 1) for v in range(B)])

    def recall(t0):
        state["h"] = store.recall(windows(t0))

    def follow(t0):
        state["store"] = state["h"].engine.generate(None, search)

    t_list, t_store, t_put, t_recall, t_follow, same = [], [], [], [], [], []
    for it in range(3 + a.iters):
        t0 = 1 + it                                                     # the window slides by one frame per iteration
        parts = [wall(lambda: put(t0)), wall(lambda: recall(t0)), wall(lambda: follow(t0))]
        full = wall(lambda: list_call(t0))
        same.append(int((state["list"][0].cpu() == state["store"][0].cpu()).all(dim=1).sum()))
        if it >= 3:
            t_put.append(parts[0]), t_recall.append(parts[1]), t_follow.append(parts[2])
            t_store.append(sum(parts)), t_list.append(full)
    res = {"model": "GIT_BASE_VATEX", "videos": B, "frames": F, "rows_per_window": F * eng.n_tok,
           "list_ms": round(median(t_list), 3), "store_ms": round(median(t_store), 3),
           "store_encode_ms": round(median(t_put), 3), "store_install_prefill_ms": round(median(t_recall), 3),
           "store_decode_ms": round(median(t_follow), 3), "list_over_store": round(median(t_list) / median(t_store), 2),
           "captions_equal_to_list_call": f"{min(same)}..{max(same)} of {B}", "store_bytes_per_frame": store.bytes_per_image}
    model.close()
    return res


def image(a) -> dict:
    B = 64
    model = make_model("GIT_BASE", B, a.precision)
    cfg, eng = model.cfg, model.engine
    search = Engine.make_search("greedy", MAX_STEPS, 1, 1)
    g = torch.Generator().manual_seed(7)
    images = torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda()
    others = torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda()
    keys = list(range(B))
    fstore = {"f32": FeatureStore(model, B, dtype=torch.float32), "f16": FeatureStore(model, B, dtype=torch.float16)}
    mstore = ImageStore(model, B)
    first = model.submit({"image": images})
    first.result()
    mstore.put(first, keys)
    want = [t.cpu() for t in eng.generate(None, search)]
    for s in fstore.values():
        s.put(images, keys)
    out = {}

    def via(store_recall):
        h = store_recall()
        out["got"] = h.engine.generate(None, search)

    legs = {"features_f32": lambda: via(lambda: fstore["f32"].recall([[k] for k in keys])),
            "features_f16": lambda: via(lambda: fstore["f16"].recall([[k] for k in keys])),
            "memory": lambda: via(lambda: mstore.recall(keys)),
            "full": lambda: out.__setitem__("got", eng.generate([images], search))}
    equal, times = {}, {k: [] for k in legs}
    for it in range(3 + a.iters):
        for name, fn in legs.items():                                   # interleaved: a, b, c, d, a, b, ...
            eng.generate([others], search)                              # another batch is resident when the recall arrives
            t = wall(fn)
            if it >= 3:
                times[name].append(t)
            equal[name] = all(torch.equal(x.cpu(), y) for x, y in zip(out["got"][:2], want[:2]))
    res = {"model": "GIT_BASE", "images": B, "outputs_equal_to_the_encoded_batch": equal,
           "feature_store_bytes_per_image": {k: s.bytes_per_image for k, s in fstore.items()},
           "image_store_bytes_per_image": eng.memory_slot_bytes()}
    for name in legs:
        res[f"{name}_ms"] = round(median(times[name]), 3)
    res["install_prefill_ms"] = round(median([wall(lambda: fstore["f32"].recall([[k] for k in keys])) for _ in range(a.iters)]), 3)
    res["memory_recall_ms"] = round(median([wall(lambda: mstore.recall(keys)) for _ in range(a.iters)]), 3)
    model.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="", choices=["", "video", "image"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("features_bench needs the MI355X")
    torch.cuda.set_device(0)
    out = {"tool": "features_bench", "precision": a.precision, "hip_graph": True, "max_steps": MAX_STEPS, "iters": a.iters,
           "timing": "median ms of wall time between device synchronisations; legs interleaved"}
    if a.only in ("", "video"):
        out["video"] = video(a)
    if a.only in ("", "image"):
        out["image"] = image(a)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
