#!/usr/bin/env python
"""What per-sentence decoding constraints cost (GITMI_SEARCH_CONSTRAIN) against the plain request of the
same batch: GIT_BASE at 224 x 224 with the benchmark's synthetic weights, one context alone, 20 steps, hipGraph on.

  greedy plain / armed    gitmi_generate with frames, greedy: one graph replay; armed = the arming call, then the same call
  beam4 plain / armed     the same under GeneratorWithBeamSearch (beam 4, per node 2, length penalty 0.6)
  arm + disarm            the arming call alone (host checks, copies enqueued on the stream, nothing waited for) and the Q == 0 call
The armed requests carry ngram = 3, min_new = 5 and one 100-token ban set on every sentence.  A plain call after the armed ones
must cost, and return, what it did before.

    python tools/constraints_bench.py [--batch 64] [--precision f16] [--iters 20] [--out FILE]
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
from generativeimage2text_amd.engine import Engine, constraint_tables  # noqa: E402
from generativeimage2text_amd.synthetic import random_state_dict  # noqa: E402
from tools.followup_bench import MAX_STEPS, timed  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("constraints_bench needs the MI355X")
    torch.cuda.set_device(0)
    cfg = config_for_model("GIT_BASE")
    B = a.batch
    g = torch.Generator().manual_seed(7)
    frames = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda()]
    banned = sorted(set(torch.randperm(cfg.vocab, generator=g)[:101].tolist()) - {cfg.eos})[:100]
    words, table = constraint_tables(B, cfg.vocab, cfg.eos, min_new_tokens=5, no_repeat_ngram_size=3, bad_tokens=banned)
    words = torch.from_numpy(words.view("int32")).cuda()
    eng = Engine(cfg, precision=a.precision, max_batch=B, max_beams=4, max_frames=1, max_text_len=MAX_STEPS)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    chain = a.precision not in ("f32", "fp32")
    res = {"model": "GIT_BASE", "images": B, "precision": a.precision, "max_steps": MAX_STEPS,
           "constraints": {"ngram": 3, "min_new": 5, "ban_set_tokens": len(banned), "sets": int(words.shape[0])}}
    arm = lambda: eng.constrain(words, table)                                                   # noqa: E731
    for name, search in (("greedy", Engine.make_search("greedy", MAX_STEPS, 1, 1)), ("beam4", Engine.make_search("beam", MAX_STEPS, 4, 2, 0.6))):
        plain = lambda: eng.generate(frames, search)                                            # noqa: E731

        def armed():
            arm()
            return eng.generate(frames, search)

        ref = plain()
        res[f"{name}_plain_ms"] = round(timed(plain, a.iters), 3)
        out = armed()
        res[f"{name}_ids_changed_rows"] = int((out[0] != ref[0]).any(dim=1).sum())
        res[f"{name}_armed_ms"] = round(timed(armed, a.iters), 3)
        res[f"{name}_plain_after_ms"] = round(timed(plain, a.iters), 3)
        again = plain()
        res[f"{name}_plain_unchanged"] = bool(torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1]))
        res[f"{name}_armed_over_plain"] = round(res[f"{name}_armed_ms"] / res[f"{name}_plain_ms"], 3)
        rows = B * (1 if name == "greedy" else 4)
        # the launch form of the vocabulary head (kernels_dgemm.hip launch_vocab_m; the f32 mode selects on materialised logits)
        res[f"{name}_head_form"] = {"plain": ("VOC_GREEDY" if rows <= 64 else "VOC_BEAM") if chain else "gemm + row_topm",
                                    "armed": "VOC_GENERIC, BAN" if chain else "gemm + row_topm<BAN>"}
    res["arm_and_disarm_ms"] = round(timed(lambda: (arm(), eng.constrain(None, [])), a.iters), 3)      # two calls: nothing stays armed
    eng.close()
    out = {"tool": "constraints_bench", "hip_graph": True, "timing": "median wall ms between device synchronisations", "result": res}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
