#!/usr/bin/env python
"""What banned token sequences cost (the search->reserved_ extension of GITMI_SEARCH_CONSTRAIN) under the
conditions of tools/constraints_bench.py: GIT_BASE at 224 x 224 with the benchmark's synthetic weights, one context alone,
20 steps, hipGraph on, greedy and beam 4.

  plain        gitmi_generate with frames: one graph replay
  set-only     the arming call of constraints_bench (ngram = 3, min_new = 5, one 100-token ban set on every sentence), then the call
  sequences    the same arming plus one list of --sequences (about 200) random sequences of 2 .. 5 tokens per sentence -- every
               sentence its own list, so the pool carries batch x sequences of them up to the cap of 4096 (then lists are shared)
The per-step difference between `sequences` and `set-only` is what ban_rows_kernel and its place in the graph cost.  A plain call
after the armed ones must cost, and return, what it did before.  --plain-only: the plain numbers alone (a tree without the
extension).

    python tools/ban_sequences_bench.py [--batch 64] [--precision f16] [--iters 20] [--sequences 200] [--out FILE]
Prints one JSON object (and writes it to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from generativeimage2text_amd import engine as E  # noqa: E402
from generativeimage2text_amd.configs import config_for_model  # noqa: E402
from generativeimage2text_amd.synthetic import random_state_dict  # noqa: E402
from tools.followup_bench import MAX_STEPS, timed  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sequences", type=int, default=200)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ban_sequences_bench needs the MI355X")
    torch.cuda.set_device(0)
    cfg = config_for_model("GIT_BASE")
    B = a.batch
    g = torch.Generator().manual_seed(7)
    frames = [torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=g).cuda()]
    banned = sorted(set(torch.randperm(cfg.vocab, generator=g)[:101].tolist()) - {cfg.eos})[:100]
    words, table = E.constraint_tables(B, cfg.vocab, cfg.eos, min_new_tokens=5, no_repeat_ngram_size=3, bad_tokens=banned)
    words = torch.from_numpy(words.view("int32")).cuda()
    res = {"model": "GIT_BASE", "images": B, "precision": a.precision, "max_steps": MAX_STEPS}
    pool = None
    if not a.plain_only:
        n_lists = max(1, min(B, E.SEQUENCE_MAX_SEQS // a.sequences))
        lists = []
        for _ in range(n_lists):
            lens = torch.randint(2, 6, (a.sequences,), generator=g).tolist()
            lists.append([torch.randint(1000, cfg.vocab, (m,), generator=g).tolist() for m in lens])
        singles, pool = E.banned_sequence_tables(B, cfg.vocab, [lists[q % n_lists] for q in range(B)])
        res["sequences"] = {"per_sentence": a.sequences, "lists": int(pool[0]), "total": int(pool[1]), "tokens": int(pool[2])}
    eng = E.Engine(cfg, precision=a.precision, max_batch=B, max_beams=4, max_frames=1, max_text_len=MAX_STEPS)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    for name, search in (("greedy", E.Engine.make_search("greedy", MAX_STEPS, 1, 1)),
                         ("beam4", E.Engine.make_search("beam", MAX_STEPS, 4, 2, 0.6))):
        plain = lambda: eng.generate(frames, search)                                            # noqa: E731

        def set_only():
            eng.constrain(words, table)
            return eng.generate(frames, search)

        def with_sequences():
            eng.constrain(words, table, sequences=pool)
            return eng.generate(frames, search)

        ref = plain()
        res[f"{name}_plain_ms"] = round(timed(plain, a.iters), 3)
        if a.plain_only:
            continue
        base = set_only()
        res[f"{name}_set_only_ms"] = round(timed(set_only, a.iters), 3)
        out = with_sequences()
        res[f"{name}_sequences_ms"] = round(timed(with_sequences, a.iters), 3)
        res[f"{name}_sequences_equal_set_only"] = bool(torch.equal(out[0], base[0]))      # random sequences: no hit expected
        res[f"{name}_per_step_us"] = round(1000.0 * (res[f"{name}_sequences_ms"] - res[f"{name}_set_only_ms"]) / (MAX_STEPS - 1), 2)
        res[f"{name}_plain_after_ms"] = round(timed(plain, a.iters), 3)
        again = plain()
        res[f"{name}_plain_unchanged"] = bool(torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1]))
    eng.close()
    out = {"tool": "ban_sequences_bench", "hip_graph": True, "timing": "median wall ms between device synchronisations", "result": res}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
