#!/usr/bin/env python
"""Follow-up calls on resident images (frames == NULL, include/gitmi.h) against the full calls they replace, with the
benchmark's synthetic weights, one context alone, hipGraph on (the serving path).

Three cases:
  vqa_480x640      GIT_BASE_VQAv2 at 480 x 640, 8 images, 16 questions (two per image), greedy answers
  caption_224      GIT_BASE at 224 x 224, 64 images, greedy captions
  generate_score   caption_224's images: generate, then the per-token log-probs of the ids it returned
For each it times
  full      the full call (image encoder + prefill + decode, or + score pass)
  followup  the same sentences with frames = None over the images the full call left resident
  decode    the decode share of the full call from gitmi_profile_enable(e, 2) (graph replays, events between the encode + prefill
            graph and the decode graph); the score case has no decode graph (score runs eagerly): its figure is the full call
            minus the encode + prefill graph of the generate call over the same images
and reports whether the follow-up's outputs are bit-equal to the full call's.  The expectation to confirm or refute: a
follow-up costs about the decode graph of the same call.

    python tools/followup_bench.py [--precision f16] [--iters 20] [--out FILE]
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


def timed(fn, iters: int, warmup: int = 3) -> float:
    """median wall ms of fn() between device synchronisations"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def bit_equal(a, b) -> bool:
    return all(torch.equal(x.cpu().view(torch.int32) if x.dtype == torch.float32 else x.cpu(),
                           y.cpu().view(torch.int32) if y.dtype == torch.float32 else y.cpu()) for x, y in zip(a, b))


def profiled_split(eng, full) -> dict:
    """(encode + prefill, decode) ms of the full call as graph replays"""
    full()
    eng.profile_enable(2)
    for _ in range(5):
        full()
    p = eng.profile_read()
    eng.profile_enable(0)
    return {"encode_prefill_ms": round(p["vit_ms"], 3), "decode_ms": round(p["decode_ms"], 3),
            "decode_step_ms": round(p["decode_step_ms"], 4)}


def case(name: str, model: str, hw, B: int, per_image: int, precision: str, iters: int) -> list:
    cfg = config_for_model(model)
    g = torch.Generator().manual_seed(7)
    frames = [torch.randn(B, 3, *hw, generator=g).cuda()]
    Q = B * per_image
    eng = Engine(cfg, precision=precision, max_batch=Q, max_beams=1, max_frames=1, max_text_len=MAX_STEPS,
                 max_image_hw=hw if hw != (cfg.image_size, cfg.image_size) else None)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    search = Engine.make_search("greedy", MAX_STEPS, 1, 1)
    if per_image > 1 or "VQA" in model:
        prefixes = [[cfg.sos] + torch.randint(1000, cfg.vocab, (int(torch.randint(5, 12, (1,), generator=g)),), generator=g).tolist()
                    for _ in range(Q)]
        image_of = [q // per_image for q in range(Q)]
        full = lambda: eng.generate_prefixed(frames, search, prefixes, image_of=image_of)       # noqa: E731
        follow = lambda: eng.generate_prefixed(None, search, prefixes, image_of=image_of)      # noqa: E731
    else:
        full = lambda: eng.generate(frames, search)                                             # noqa: E731
        follow = lambda: eng.generate(None, search)                                             # noqa: E731
    ref = full()
    res = {"case": name, "model": model, "hw": list(hw), "images": B, "sentences": Q, "precision": precision,
           "outputs_equal": bit_equal(ref, follow())}
    res["full_ms"] = round(timed(full, iters), 3)
    full()
    res["followup_ms"] = round(timed(follow, iters), 3)
    res.update(profiled_split(eng, full))
    res["followup_over_decode"] = round(res["followup_ms"] / res["decode_ms"], 3)
    res["full_over_followup"] = round(res["full_ms"] / res["followup_ms"], 2)
    out = [res]
    if name == "caption_224":           # generate, then score the ids it returned
        ids = ref[0]
        full_s = lambda: eng.score(frames, ids)                                                # noqa: E731
        follow_s = lambda: eng.score(None, ids)                                                # noqa: E731
        a = full_s()
        full()
        sc = {"case": "generate_score", "model": model, "hw": list(hw), "images": B, "sentences": B, "precision": precision,
              "outputs_equal": bit_equal([a], [follow_s()])}
        sc["full_ms"] = round(timed(full_s, iters), 3)
        sc["followup_ms"] = round(timed(follow_s, iters), 3)
        sc["encode_prefill_ms"] = res["encode_prefill_ms"]
        sc["decode_ms"] = round(sc["full_ms"] - res["encode_prefill_ms"], 3)      # score pass = full - (encode + prefill)
        sc["followup_over_decode"] = round(sc["followup_ms"] / sc["decode_ms"], 3) if sc["decode_ms"] > 0 else None
        sc["full_over_followup"] = round(sc["full_ms"] / sc["followup_ms"], 2)
        out.append(sc)
    eng.close()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("followup_bench needs the MI355X")
    torch.cuda.set_device(0)
    results = case("vqa_480x640", "GIT_BASE_VQAv2", (480, 640), 8, 2, a.precision, a.iters) + \
        case("caption_224", "GIT_BASE", (224, 224), 64, 1, a.precision, a.iters)
    out = {"tool": "followup_bench", "hip_graph": True, "timing": "median wall ms between device synchronisations",
           "results": results}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
