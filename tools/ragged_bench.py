#!/usr/bin/env python
"""Ragged image batches (gitmi_set_image_shape(e, 0, 0)) against today's calls grouped by shape, on the aspect-preserving VQA
models with the benchmark's synthetic weights, one context alone.

64 images drawn (fixed seed) from the MinMaxResizeForTest shapes (9 distinct) of 12 common photo sizes, 1-3 questions each, greedy answers:
  ragged  : ONE gitmi_generate_prefixed call over all 64 images (every image at its own size, padded to the capacity grid)
  by_shape: one call per distinct shape (what test_git_inference_single_tsv does without mixed_shapes)
Reports answers/s and ms per call of both, the padding share of the encoder rows sum(Nmax - n_b) / (B Nmax), and how many
answers agree between the two (16-bit modes: per-shape calls run other GEMM shapes, so rare last-bit flips are possible).

    python tools/ragged_bench.py [--models GIT_BASE_VQAv2,GIT_LARGE_VQAv2] [--precision f16] [--iters 10] [--out FILE]
    python tools/ragged_bench.py --no-graph ...     # control: both sides eager (no hipGraph capture or replay)
    python tools/ragged_bench.py --trace ragged|uniform --models GIT_BASE_VQAv2     # one eager call, for rocprofv3
With graphs on (the default, the serving path) an engine caches ONE captured graph keyed on (B, Q, H, W, ...): the by_shape loop
re-captures on each of its calls (every call has another key), while the ragged side replays the graph of an identical call --
in a TSV run Q changes from call to call, so ragged calls re-capture too.  --no-graph times both sides without graphs.
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
from generativeimage2text_amd.inference import MinMaxResizeForTest  # noqa: E402
from generativeimage2text_amd.synthetic import random_state_dict  # noqa: E402

# (width, height) of common photo sizes (COCO / VQAv2 / TextVQA-style): their MinMax shapes differ per model
SOURCE_WH = [(640, 480), (480, 640), (500, 500), (640, 360), (375, 500), (500, 333), (427, 640), (640, 427), (612, 612),
             (1024, 683), (333, 500), (720, 1280)]
N_IMAGES = 64
MAX_STEPS = 20


def timed(fn, iters: int, warmup: int = 2) -> float:
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


def workload(cfg, seed: int = 0):
    """-> images [3, h, w] (device), prefixes, image_of"""
    g = torch.Generator().manual_seed(seed)
    rs = MinMaxResizeForTest(cfg.image_size, max(cfg.max_image_hw))
    shapes = [rs.get_size(wh) for wh in SOURCE_WH]
    pick = torch.randint(0, len(shapes), (N_IMAGES,), generator=g).tolist()
    images = [torch.randn(3, *shapes[i], generator=g).cuda() for i in pick]
    prefixes, image_of = [], []
    for b in range(N_IMAGES):
        for _ in range(int(torch.randint(1, 4, (1,), generator=g))):
            n = int(torch.randint(5, 12, (1,), generator=g))
            prefixes.append([cfg.sos] + torch.randint(1000, cfg.vocab, (n,), generator=g).tolist())
            image_of.append(b)
    return images, prefixes, image_of


def run_model(name: str, precision: str, iters: int, trace: str = "", graph: bool = True) -> dict:
    cfg = config_for_model(name)
    images, prefixes, image_of = workload(cfg)
    Q = len(prefixes)
    eng = Engine(cfg, precision=precision, max_batch=Q, max_beams=1, max_frames=1, max_text_len=MAX_STEPS)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    search = Engine.make_search("greedy", MAX_STEPS, 1, 1)
    eng.set_graph(graph)
    Nmax = eng.max_tokens
    p = int(cfg.patch)
    ntok = [(im.shape[1] // p) * (im.shape[2] // p) + 1 for im in images]
    packed = eng.ragged(images)
    groups = {}
    for b, im in enumerate(images):
        groups.setdefault(tuple(im.shape[1:]), []).append(b)
    calls = []
    for shape, members in groups.items():
        pos = {b: i for i, b in enumerate(members)}
        qs = [q for q in range(Q) if image_of[q] in pos]
        calls.append((qs, [torch.stack([images[b] for b in members])], [prefixes[q] for q in qs],
                      [pos[image_of[q]] for q in qs]))

    def ragged():
        return eng.generate_prefixed(packed, search, prefixes, image_of=image_of)

    def by_shape():
        return [eng.generate_prefixed(fr, search, pf, image_of=io) for _, fr, pf, io in calls]

    if trace:
        eng.set_graph(False)
        (ragged if trace == "ragged" else lambda: eng.generate_prefixed(calls[0][1], search, calls[0][2], image_of=calls[0][3]))()
        torch.cuda.synchronize()
        return {"model": name, "trace": trace}
    res = {"model": name, "precision": precision, "hip_graph": graph, "images": N_IMAGES, "questions": Q, "Nmax": Nmax,
           "shapes": {f"{h}x{w}": len(m) for (h, w), m in sorted(groups.items())},
           "padding_row_share": round(sum(Nmax - n for n in ntok) / (N_IMAGES * Nmax), 4),
           "calls_by_shape": len(calls)}
    t_r = timed(ragged, iters)
    t_s = timed(by_shape, iters)
    res.update(ragged_ms_per_call=round(t_r, 3), ragged_answers_per_s=round(Q / t_r * 1e3, 1),
               by_shape_ms_total=round(t_s, 3), by_shape_ms_per_call=round(t_s / len(calls), 3),
               by_shape_answers_per_s=round(Q / t_s * 1e3, 1), speedup=round(t_s / t_r, 3))
    tok_r, _, sent_r, _ = ragged()
    tok_r, sent_r = tok_r.cpu(), sent_r.cpu()
    same = 0
    for (qs, _, _, _), (tok_s, _, sent_s, _) in zip(calls, by_shape()):
        tok_s, sent_s = tok_s.cpu(), sent_s.cpu()
        for i, q in enumerate(qs):
            L = int(sent_s[i, 0])
            same += int(int(sent_r[q, 0]) == L and torch.equal(tok_r[q, :L], tok_s[i, :L]))
    res["answers_equal_by_shape"] = f"{same}/{Q}"
    eng.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="GIT_BASE_VQAv2,GIT_LARGE_VQAv2")
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trace", default="", choices=["", "ragged", "uniform"])
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ragged_bench needs the MI355X")
    torch.cuda.set_device(0)
    out = {"tool": "ragged_bench", "results": [run_model(m, a.precision, a.iters, a.trace, not a.no_graph) for m in a.models.split(",")]}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
