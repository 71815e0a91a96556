#!/usr/bin/env python
"""Caption scoring timings (GITMI_SEARCH_SCORE) on GIT_BASE with the benchmark's synthetic weights, one context alone.

  (a) score 64 images x 1 caption x 20 tokens  vs  gitmi_generate greedy 20 steps on the same batch
  (b) 16 images x 16 candidates x 16 tokens: the whole score call; with --trace the per-kernel times come from a
      `rocprofv3 --kernel-trace --stats` run of this script (score_head_kernel = the head, score_attn_kernel = attention)
  (c) the same scores from a gitmi_step_logits replay (t decode steps per position, logits to the host), for contrast
  --attend: an attention-map call (GITMI_SEARCH_ATTEND) on the sentences of (a) and of (b) as well; under rocprofv3 the map
      kernel is score_attn_map_mfma_kernel (score_attn_map_kernel in the f32 mode)

    python tools/score_bench.py [--precision f16] [--iters 20] [--out profiles/r07_score_bench.json]
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
from generativeimage2text_amd.configs import GitModelConfig  # noqa: E402
from generativeimage2text_amd.engine import Engine  # noqa: E402
from generativeimage2text_amd.synthetic import random_frames, random_state_dict  # noqa: E402

PEAK_16BIT = 2.5e15           # dense fp16 / bf16 MFMA FLOP/s of MI355X (spec)


def timed(fn, iters: int, warmup: int = 3) -> float:
    """median wall ms of fn() between stream synchronisations"""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-replay", action="store_true")
    ap.add_argument("--attend", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = GitModelConfig()
    sd = random_state_dict(cfg, seed=1234)
    res = {"precision": a.precision, "config": "GIT_BASE"}
    gen = torch.Generator().manual_seed(0)

    # (a) 64 x 1 x 20 against greedy generate on the same batch
    eng = Engine(cfg, precision=a.precision, max_batch=64, max_beams=8, max_frames=1, max_text_len=20)
    eng.load_state_dict(sd)
    frames = random_frames(cfg, 64, 1, seed=0)
    tok = torch.randint(1000, cfg.vocab, (64, 20), generator=gen)
    tok[:, 0] = cfg.sos
    search = Engine.make_search("greedy", 20, 1, 1)
    res["a_generate_ms"] = timed(lambda: eng.generate(frames, search), a.iters)
    res["a_score_ms"] = timed(lambda: eng.score(frames, tok), a.iters)
    res["a_score_lt_generate"] = res["a_score_ms"] < res["a_generate_ms"]
    if a.attend:
        res["a_attend_ms"] = timed(lambda: eng.attend(frames, tok), a.iters)
        res["a_attend_out_mb"] = 64 * 20 * cfg.dec_layers * (eng.n_tok + 20) * 4 / 1e6

    # (b) 16 images x 16 candidates x 16 tokens
    fr16 = [f[:16].contiguous() for f in frames]
    tb = torch.randint(1000, cfg.vocab, (256, 16), generator=gen)
    tb[:, 0] = cfg.sos
    image_of = [q // 16 for q in range(256)]
    res["b_score_ms"] = timed(lambda: eng.score(fr16, tb, image_of=image_of), a.iters)
    if a.attend:
        res["b_attend_ms"] = timed(lambda: eng.attend(fr16, tb, image_of=image_of), a.iters)
        res["b_attend_out_mb"] = 256 * 16 * cfg.dec_layers * (eng.n_tok + 16) * 4 / 1e6
    M = 256 * 16
    res["b_head_gflop"] = 2.0 * M * cfg.vocab * cfg.dec_hidden / 1e9
    res["b_head_peak_ms"] = 2.0 * M * cfg.vocab * cfg.dec_hidden / PEAK_16BIT * 1e3
    out_b = eng.score(fr16, tb, image_of=image_of).cpu()

    # (c) the step_logits replay of the same scores: position t needs t decode steps; logits of every row to the host.
    # gitmi_step_logits takes at most max_beams (8) rows per image: the first 8 candidates of every image (128 of the 256
    # rows, rows of one image contiguous); c_replay_ms_256 scales that to the whole set
    if not a.skip_replay:
        rows = torch.tensor([i * 16 + k for i in range(16) for k in range(8)])
        tr = tb[rows]

        def replay():
            lp = torch.zeros(128, 16)
            eng.encode(fr16, return_features=False)
            for t in range(1, 16):
                logits = eng.step_logits(tr[:, :t].cuda())
                ls = torch.log_softmax(logits.double(), -1).cpu()
                lp[:, t] = ls[torch.arange(128), tr[:, t]].float()
            return lp
        replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp_r = replay()
        torch.cuda.synchronize()
        res["c_replay_ms_128"] = (time.perf_counter() - t0) * 1e3
        res["c_replay_ms_256"] = 2.0 * res["c_replay_ms_128"]
        res["c_replay_vs_score_max_abs_lp"] = float((lp_r[:, 1:] - out_b[rows][:, 1:, 0]).abs().max())
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
