#!/usr/bin/env python
"""Closed-set ranking through the token trie against the same scores sentence by sentence.

Workload: a GIT_BASE_VQAv2-shaped engine (480 x 480 images, 901 image tokens), 8 images, one 10-token question each, a synthetic
answer list of 3129 candidates of 1-4 tokens (+ [SEP]), the benchmark's synthetic weights.
  tree : CaptioningModel.rank -- ONE engine call, every trie node scored once (GITMI_SEARCH_TREE_SCORE)
  score: the same scores from CaptioningModel.score -- `[CLS] question answer [SEP]` rows in chunks of max_batch x max_beams
         sentences, the first chunk with the images, the rest as follow-ups over the resident images (no re-encode)
Method: events around the calls, warm-up first, the two sides interleaved iteration by iteration, median of --iters (>= 11).

    python tools/tree_score_bench.py [--precision f16] [--iters 11] [--out profiles/tree_score_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/tree_score_bench.py --only tree --iters 1   (per-kernel split;
        likewise --only score; tools/rocprof_summary.py turns each .db into a table, --merge-stats folds the tables into --out)
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
from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel  # noqa: E402
from generativeimage2text_amd.synthetic import random_frames, random_state_dict  # noqa: E402

IMAGES, QUESTION, CANDIDATES = 8, 10, 3129


def candidate_list(vocab: int, gen: torch.Generator):
    """3129 distinct answers of 1-4 tokens over a small answer vocabulary, so that prefixes are shared as in a real list"""
    words = torch.randint(1000, vocab, (600,), generator=gen).tolist()
    seen, out = set(), []
    while len(out) < CANDIDATES:
        n = int(torch.randint(1, 5, (1,), generator=gen))
        c = tuple(words[int(i)] for i in torch.randint(0, len(words), (n,), generator=gen))
        if c not in seen:
            seen.add(c)
            out.append(list(c))
    return out


def event_ms(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def merge_stats(out: str, tables) -> None:
    """fold `name=path` kernel tables of tools/rocprof_summary.py into the JSON at `out`: per side, the kernels above 1 %"""
    with open(out) as f:
        res = json.loads(f.read())
    for item in tables:
        side, path = item.split("=", 1)
        rows = []
        for line in open(path):
            parts = line.split(None, 9)
            if line.startswith("#") or len(parts) < 10 or not parts[0].endswith("%"):
                continue
            pct = float(parts[0][:-1])
            if pct >= 1.0:
                rows.append({"pct": pct, "calls": int(parts[1]), "total_ms": float(parts[2]), "kernel": parts[9].strip()[:120]})
        res[f"{side}_kernels"] = rows
    with open(out, "w") as f:
        f.write(json.dumps(res) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=64, help="max_batch of the engine: score chunks hold max_batch x 8 sentences "
                    "(8 = the largest max_beams an engine takes), far more than the 8 images need")
    ap.add_argument("--only", choices=("tree", "score"), default=None, help="run one side only (kernel traces)")
    ap.add_argument("--out", default="")
    ap.add_argument("--merge-stats", nargs="*", default=None, metavar="SIDE=TABLE")
    a = ap.parse_args()
    if a.merge_stats is not None:
        merge_stats(a.out, a.merge_stats)
        return
    if a.iters < 11 and not a.only:
        ap.error("--iters must be at least 11 for the timed comparison (fewer only with --only, for kernel traces)")
    torch.cuda.set_device(0)
    cfg = config_for_model("GIT_BASE_VQAv2")
    T = 1 + QUESTION + 4 + 1
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=T, beam_size=8, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision=a.precision, max_batch=a.max_batch, max_frames=1, max_text_len=T)
    model.load_state_dict(random_state_dict(cfg, seed=1234))
    gen = torch.Generator().manual_seed(0)
    images = random_frames(cfg, IMAGES, 1, seed=0)[0]
    questions = torch.randint(1000, cfg.vocab, (IMAGES, QUESTION), generator=gen).tolist()
    cands = candidate_list(cfg.vocab, gen)
    chunk = a.max_batch * 8

    # the sentence form: [CLS] question answer [SEP], the question not counted
    rows = [(q, k) for q in range(IMAGES) for k in range(CANDIDATES)]
    sent = torch.zeros(len(rows), T, dtype=torch.int64)
    need = torch.zeros(len(rows), T, dtype=torch.int64)
    for r, (q, k) in enumerate(rows):
        s = [cfg.sos] + questions[q] + cands[k] + [cfg.eos]
        sent[r, :len(s)] = torch.tensor(s)
        need[r, 1 + QUESTION:len(s)] = 1
    image_of = [q for q, _ in rows]

    def by_tree():
        return model.rank(images, cands, prefixes=questions)

    def by_score():
        sums = []
        for c0 in range(0, len(rows), chunk):
            sl = slice(c0, c0 + chunk)
            out = model.score(images if c0 == 0 else None, sent[sl], image_of=image_of[sl], need_predict=need[sl])
            sums.append(out["sum"])
        return torch.cat(sums).view(IMAGES, CANDIDATES)

    sides = [("tree", by_tree), ("score", by_score)]
    if a.only:
        sides = [s for s in sides if s[0] == a.only]
    times = {name: [] for name, _ in sides}
    last = {}
    for it in range(a.warmup + a.iters):
        for name, fn in sides:                                   # interleaved: drift hits both sides alike
            holder = {}
            ms = event_ms(lambda: holder.setdefault("out", fn()))
            last[name] = holder["out"]
            if it >= a.warmup:
                times[name].append(ms)
    res = {"config": "GIT_BASE_VQAv2", "precision": a.precision, "images": IMAGES, "question_tokens": QUESTION,
           "candidates": CANDIDATES, "iters": a.iters, "warmup": a.warmup, "interleaved": a.only is None}
    for name, ts in times.items():
        ts.sort()
        res[f"{name}_ms_median"], res[f"{name}_ms_min"], res[f"{name}_ms_max"] = ts[len(ts) // 2], ts[0], ts[-1]
    if "tree" in last:
        lens = last["tree"]["tree"]["lengths"]
        res["tree_nodes_per_tree"] = int(lens[0])
        res["tree_rows"] = IMAGES * (-(-max(lens) // 16) * 16)
        res["tree_calls"] = 1
    if "score" in times:
        res["score_rows"] = len(rows) * (-(-T // 16) * 16)
        res["score_sentences"] = len(rows)
        res["score_chunk_sentences"] = chunk
        res["score_calls"] = -(-len(rows) // chunk)
    if len(last) == 2:
        diff = (last["tree"]["scores"] - last["score"]).abs().max().item()
        res["max_abs_score_difference"] = diff
        res["same_argmax_fraction"] = float((last["tree"]["best"] == last["score"].argmax(1)).float().mean())
        res["tree_speedup"] = res["score_ms_median"] / res["tree_ms_median"]
    model.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
