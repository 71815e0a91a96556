"""What the per-token trace costs (GITMI_SEARCH_TRACE): GIT_BASE, 64 images, 20 steps, f16, hipGraph on, one
context; median of 20 wall times per form, greedy and beam 4 --
  plain | traced n = 0 | traced n = 5 | (greedy only) plain + a GITMI_SEARCH_SCORE follow-up over the ids, the way to get token
  log-probs without the trace.
Writes one JSON object to --out (default $BENCH_OUT/token_scores_bench.json or ./out/).

    python tools/token_scores_bench.py [--out profiles/token_scores_bench.json] [--repeat 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import git_oracle as O  # noqa: E402
from generativeimage2text_amd.engine import Engine  # noqa: E402


def median_ms(fn, repeat):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(times), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(os.environ.get("BENCH_OUT", os.path.join(ROOT, "out")), "token_scores_bench.json"))
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    cfg, B, T = O.CONFIGS["GIT_BASE"], a.batch, 20
    w = O.make_weights(cfg, seed=1234)
    frames = [f.cuda() for f in O.make_images(cfg, B, 1, seed=0)]
    result = {"config": "GIT_BASE", "batch": B, "max_steps": T, "precision": "f16", "graph": True, "repeat": a.repeat, "ms": {}}
    for name, search in (("greedy", Engine.make_search("greedy", T, 1, 1)), ("beam4", Engine.make_search("beam", T, 4, 2, 0.6))):
        eng = Engine(cfg, precision="f16", max_batch=B, max_beams=int(search.beam_size), max_frames=1, max_text_len=T)
        eng.load_state_dict(w)
        ms = {"plain": median_ms(lambda: eng.generate(frames, search, sync=False), a.repeat)}
        for n in (0, 5):
            def traced():
                eng.trace(B, 1, T, n)
                eng.generate(frames, search, sync=False)
            ms[f"traced_n{n}"] = median_ms(traced, a.repeat)
        if name == "greedy":
            def plain_then_score():
                tokens, _, _ = eng.generate(frames, search, sync=False)
                eng.score(None, tokens)
            ms["plain_plus_score_followup"] = median_ms(plain_then_score, a.repeat)
        ms["plain_again"] = median_ms(lambda: eng.generate(frames, search, sync=False), a.repeat)
        result["ms"][name] = ms
        eng.close()
    g = result["ms"]["greedy"]
    result["traced_n0_cheaper_than_score_followup"] = bool(g["traced_n0"] < g["plain_plus_score_followup"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
