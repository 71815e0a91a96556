"""Freeze the banned-sequence fixtures tests/golden/banseq_*.npz from the REFERENCE search classes (CPU only, run once).

The sibling of tools/make_constraints_golden.py for the sequence rule (include/gitmi.h, the extension of GITMI_SEARCH_CONSTRAIN):
tools/constrained_step.wrap_step, handed `sequences` / `list_of`, sets the banned logits of a step to -10000 and the unmodified
AutoRegressiveBeamSearch / GeneratorWithBeamSearch do the rest.  Everything else -- the reference model from seeded weights and
images, the margins from the oracle's restatement of the search, the fixture fields -- is that tool's, imported from it; a
fixture here carries one more array, `pool` (engine.banned_sequence_tables of the sentences' lists).

In every case the banned sequences are taken FROM the plain ids.  Asserted on the CPU for every constrained sentence: its plain
ids contain one of its sequences ending past the prefix (the ban fires), its constrained ids contain none, and they differ.

  banseq_tiny_greedy      B = 4, one call, sequences alone: lengths 2, 3, 5 and 2
  banseq_tiny_combined    the same with a set, min_new and ngram = 2 on every sentence
  banseq_tiny_prefix      one call with a prefix (the reference takes one prefix per call: batch 1); the sentence bans a
                          three-token sequence that begins at the last prefix token
  banseq_tiny_beam4       beam 4, one batch-1 call per image: hits after a beam reorder
  banseq_fullvocab        the TINY decoder with vocab 30522: a list that also ends in token 30521 (the last partial set word)

Margins follow make_constraints_golden.py: one-beam cases need every decision margin >= 2 x logit_bound("f16", span); the beam
case is frozen under 10 x F32_LOGIT_ABS (DESIGN.md sections 20 and 21 have the surveys).

    python tools/make_ban_sequences_golden.py [case ...]           search the seeds (a process pool; the smallest passing seed wins)
    python tools/make_ban_sequences_golden.py --check [case ...]   regenerate the committed fixtures from their recorded seeds, compare
    python tools/make_ban_sequences_golden.py --survey N case      N seeds: how many meet every other condition, how many the margin too
"""
from __future__ import annotations

import ast
import multiprocessing
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import git_oracle as O  # noqa: E402
from oracle.make_golden import GOLD, build_reference, dataclass_tuple  # noqa: E402
from generativeimage2text_amd.engine import banned_sequence_tables  # noqa: E402
from tools import make_constraints_golden as G  # noqa: E402
from tools.constrained_step import wrap_step  # noqa: E402
from tools.parity import F32_LOGIT_ABS, logit_bound  # noqa: E402

PREFIX = [101, 300, 2]
# name: (vocab override, weights kw, batch, search, prefix, sequence length per sentence (0: unconstrained), combined with a table)
CASES = {
    "banseq_tiny_greedy": (None, dict(eos_bias=1.5), 4, G.GREEDY_SHORT, None, (2, 3, 5, 2), False),
    "banseq_tiny_combined": (None, dict(eos_bias=1.5), 4, G.GREEDY_SHORT, None, (2, 3, 5, 2), True),
    "banseq_tiny_prefix": (None, dict(eos_bias=1.5), 1, G.GREEDY_SHORT, PREFIX, (3,), False),
    "banseq_tiny_beam4": (None, dict(eos_bias=1.5), 4, G.BEAM_SHORT, None, (2, 3, 2, 3), False),
    "banseq_fullvocab": (G.FULL_VOCAB, dict(eos_bias=1.0), 2, G.GREEDY_SHORT, None, (3, 0), False),
}
SEEDS = {name: range(100, 4000) for name in CASES}


def occurs_past(hist, seq, P):
    """Whether `seq` occurs in `hist` with its last token at or past position P (a generated token)"""
    m = len(seq)
    return any(hist[i:i + m] == list(seq) for i in range(max(P - m + 1, 0), len(hist) - m + 1))


def choose_sequences(lens, plain, P, cfg, prefixed):
    """One list per constrained sentence, from its plain history: the sequence of the given length that ends at the second
    generated token (later where the history's head is shorter than that; prefixed: the one that begins at the last prefix
    token, so it matches across the boundary), a decoy that shares its head and ends in token 0, and a five-token decoy whose head the history never holds -> (lists, list_of) or the reason"""
    lists, list_of = [], []
    for q, m in enumerate(lens):
        hist, _ = plain[q]
        if m == 0:
            list_of.append(-1)
            continue
        start = P - 1 if prefixed else max(P + 2 - m, 0)
        if start < 0 or start + m > len(hist) or cfg.eos in hist[start:start + m]:
            return f"sentence {q} is too short for a sequence of {m} tokens"
        seq = hist[start:start + m]
        decoys = [seq[:-1] + [0], [7, 7, 7, 7, 7]]
        if cfg.vocab == G.FULL_VOCAB:
            decoys.append(seq[:-1] + [cfg.vocab - 1])                       # a hit in the last, partial set word
        lists.append([seq] + [d for d in decoys if d != seq])
        list_of.append(len(lists) - 1)
    return lists, list_of


def attempt(name, seed):
    vocab, wkw, B, search, prefix, lens, combined = CASES[name]
    cfg = G.config_of("TINY", vocab)
    wkw = dict(wkw, seed=seed)
    w = O.make_weights(cfg, **wkw)
    image_seed = sum(map(ord, name)) + seed
    frames = O.make_images(cfg, B, 1, seed=image_seed)
    model = build_reference(cfg, w, search, wkw.get("tie_output", True))
    batched = search.kind == "greedy" and search.beam_size == 1
    pfx = torch.tensor(prefix, dtype=torch.long)[None] if prefix is not None else None
    P = 1 if prefix is None else len(prefix)
    lead = 1 if prefix is None else 0
    W = (cfg.vocab + 31) // 32
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if batched:
            plain, _, _, _ = G.run_search(model, cfg, search, {"image": frames[0]}, pfx, None)
        else:
            plain, _, _, _ = G.per_image(model, cfg, search, frames, pfx, B, None)
        was = G.histories(plain, lead, prefix, cfg)
        chosen = choose_sequences(lens, was, P, cfg, prefix is not None)
        if isinstance(chosen, str):
            return f"seed {seed}: {chosen}"
        lists, list_of = chosen
        sets, table = np.zeros((0, W), np.uint32), [[-1, 0, 0] for _ in range(B)]
        if combined:
            both = G.choose(("all",) * B, was, P, cfg, search.max_steps)
            if isinstance(both, str):
                return f"seed {seed}: {both}"
            sets, table = both
        if batched:
            wrap = lambda step: wrap_step(step, sets, table, cfg.eos, [P] * B, sequences=lists, list_of=list_of)
            preds, lps, margins, span = G.run_search(model, cfg, search, {"image": frames[0]}, pfx, wrap)
        else:
            wraps = [(lambda step, b=b: wrap_step(step, sets, [table[b]], cfg.eos, [P], sequences=lists, list_of=[list_of[b]]))
                     for b in range(B)]
            preds, lps, margins, span = G.per_image(model, cfg, search, frames, pfx, B, wraps)
    got = G.histories(preds, lead, prefix, cfg)
    for q in range(B):
        if list_of[q] < 0:
            continue
        seqs = lists[list_of[q]]
        assert any(occurs_past(was[q][0], s, P) for s in seqs), (name, q)            # the ban fires on the plain ids
        assert not any(occurs_past(got[q][0], s, P) for s in seqs), (name, q, got[q], seqs)   # the reference keeps the rule
        if got[q][0] == was[q][0]:
            return f"seed {seed}: sentence {q}: the constrained ids equal the plain ids"
        if combined:
            assert not G.violates(table[q], sets, got[q][0], P, cfg.eos, got[q][1], cfg.vocab), (name, q)
    need = 2.0 * logit_bound("f16", span[1] - span[0]) if batched else 10.0 * F32_LOGIT_ABS
    if float(margins.min()) < need:
        return f"seed {seed}: smallest decision margin {float(margins.min()):.2e} < {need:.2e}"
    singles, pool = banned_sequence_tables(B, cfg.vocab, [None if l < 0 else lists[l] for l in list_of])
    assert all(s is None for s in singles) and pool is not None
    print(f"[{name}] seed {seed}  lists {lists}  table {table}  min margin {float(margins.min()):.4f}  span {span[1] - span[0]:.2f}  "
          f"pred {preds.tolist()}  plain {plain.tolist()}", flush=True)
    return dict(
        config="TINY", vocab=np.int64(cfg.vocab), weights_kw=repr(wkw), batch=B, frames=1, image_seed=image_seed,
        hw=np.array([], dtype=np.int64), search=repr(dataclass_tuple(search)),
        prefix=np.array(prefix if prefix is not None else [], dtype=np.int64), per_image=not batched,
        sets=sets, table=np.array(table, dtype=np.int32), pool=pool,
        predictions=preds.numpy(), logprobs=lps.numpy(), predictions_plain=plain.numpy(),
        step_margin=margins.numpy().astype(np.float32), logit_min=np.float32(span[0]), logit_max=np.float32(span[1]))


def _attempt(args):
    return args[1], attempt(*args)


def run(name, workers=None):
    workers = workers or min(16, os.cpu_count() or 1)
    with multiprocessing.get_context("spawn").Pool(workers, initializer=G._init_worker) as pool:
        for seed, out in pool.imap(_attempt, ((name, s) for s in SEEDS[name]), chunksize=1):
            if isinstance(out, dict):
                np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
                return
    raise SystemExit(f"{name}: no seed of {SEEDS[name]} meets the conditions")


def survey(name, n, workers=None):
    met = passed = 0
    with multiprocessing.get_context("spawn").Pool(workers or min(16, os.cpu_count() or 1), initializer=G._init_worker) as pool:
        seeds = range(SEEDS[name].start, SEEDS[name].start + n)
        for seed, out in pool.imap(_attempt, ((name, s) for s in seeds), chunksize=1):
            passed += isinstance(out, dict)
            met += isinstance(out, dict) or "smallest decision margin" in out
    print(f"[{name}] survey: {n} seeds, {met} meet every other condition, {passed} the margin bound too", flush=True)


def regenerates(name):
    old = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    G._init_worker()
    new = attempt(name, ast.literal_eval(str(old["weights_kw"]))["seed"])
    assert isinstance(new, dict), new
    bad = [k for k in old.files if not np.array_equal(np.asarray(new[k]), old[k])]
    print(f"[{name}] {'regenerates bit for bit' if not bad else 'DIFFERS in ' + str(bad)}", flush=True)
    return not bad


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--survey", type=int, metavar="N")
    a = ap.parse_args()
    if a.check:
        sys.exit(0 if all([regenerates(n) for n in a.cases]) else 1)
    for n in a.cases:
        survey(n, a.survey) if a.survey else run(n)
