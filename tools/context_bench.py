#!/usr/bin/env python
"""What a request with context tokens costs (GITMI_SEARCH_CONTEXT) against the plain request of the same
batch: GIT_BASE at 224 x 224 with the benchmark's synthetic weights, one context alone, greedy, hipGraph on.

  plain     gitmi_generate with frames: one graph replay (encoder + prefill + decode)
  context   the context call (eager encoder + context rows + prefill over B x stride rows), then the graphed follow-up search
  encode    the context call alone
and the same plain call again after the context requests (it must cost what it cost before).

    python tools/context_bench.py [--batch 64] [--context 32] [--precision f16] [--iters 20] [--out FILE]
Prints one JSON object (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from generativeimage2text_amd.configs import config_for_model  # noqa: E402
from generativeimage2text_amd.engine import Engine  # noqa: E402
from generativeimage2text_amd.synthetic import random_state_dict  # noqa: E402
from tools.followup_bench import MAX_STEPS, timed  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--context", type=int, default=32, help="context tokens per image")
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("context_bench needs the MI355X")
    torch.cuda.set_device(0)
    cfg = config_for_model("GIT_BASE")
    B, Cn = a.batch, a.context
    g = torch.Generator().manual_seed(7)
    frames = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda()]
    segments = torch.randint(1000, cfg.vocab, (B, Cn), generator=g)
    eng = Engine(cfg, precision=a.precision, max_batch=B, max_beams=1, max_frames=1, max_text_len=MAX_STEPS, max_context=Cn)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    search = Engine.make_search("greedy", MAX_STEPS, 1, 1)
    plain = lambda: eng.generate(frames, search)                                                # noqa: E731
    encode = lambda: eng.encode_context(frames, segments, lengths=[Cn] * B)                     # noqa: E731

    def context():
        encode()
        return eng.generate(None, search)

    ref = plain()
    res = {"model": "GIT_BASE", "images": B, "context_tokens_per_image": Cn, "precision": a.precision, "max_steps": MAX_STEPS}
    res["plain_ms"] = round(timed(plain, a.iters), 3)
    out = context()
    res["stride"] = eng.resident_geometry.stride
    res["ids_changed_rows"] = int((out[0] != ref[0]).any(dim=1).sum())
    res["context_ms"] = round(timed(context, a.iters), 3)
    res["context_encode_ms"] = round(timed(encode, a.iters), 3)
    res["plain_after_ms"] = round(timed(plain, a.iters), 3)
    again = plain()
    res["plain_unchanged"] = bool(torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1]))
    res["context_over_plain"] = round(res["context_ms"] / res["plain_ms"], 3)
    eng.close()
    out = {"tool": "context_bench", "hip_graph": True, "timing": "median wall ms between device synchronisations", "result": res}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
