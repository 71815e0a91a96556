"""Freeze the feature fixtures tests/golden/features_*.npz from the REFERENCE model (CPU only, run once).

The reference's CaptioningModel.infer(batch, visual_features, visual_features_valid) takes the visual features as an argument:
the seam GITMI_SEARCH_FEATURES opens on the engine (include/gitmi.h).  Every case draws seeded weights and ARBITRARY feature
rows (unit normal: no image and no encoder pass stands behind them), cuts the row buffer into pieces -- images of unequal row
counts, an image made of two pieces -- and records, per image, what ONE batch-1 reference call over its rows returns:

  - counts [B], pieces [Q, 3] = (first row, rows, -1), image_of [Q], feat_seed (the rows are rebuilt from the seed: feature_rows),
  - greedy_predictions / greedy_logprobs / greedy_margin and beam_predictions / beam_logprobs / beam_margin: the reference's ids
    (padded with 0), its log-probs and the decision margins of every search step, from the oracle's restatement of the search
    driven by the reference's own decoding_step (asserted to return the reference's ids); the oracle's own pipeline
    (git_oracle.caption(feats=...)) is asserted to return the same ids first,
  - tf_tokens / tf_lengths / tf_lp: one caption per image with the per-position log-probs of the reference's fp32 logits
    (log_softmax in fp64, as tools/freeze_score_golden.py records them) and logit_min / logit_max of the rows that count.

Seeds are searched until every decision margin of every image, greedy and beam 4, is at least 10 x tools/parity.F32_LOGIT_ABS;
the script fails if no seed of its range does.

    python tools/make_features_golden.py [case ...]
"""
from __future__ import annotations

import functools
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import git_oracle as O  # noqa: E402
from tools.parity import F32_LOGIT_ABS  # noqa: E402

MIN_MARGIN = 10.0 * F32_LOGIT_ABS
_LONG = dict(tie_output=False, successor=2.0, eos_bias=1.5)
# name: (config, weights kw without the seed, [(image, rows)] per piece in buffer order)
CASES = {
    # key counts 17 / 18 / 32 / 33: either side of the decode attention's 32-key tile and of the 16-row install tile; image 1 is
    # two pieces (5 + 13) with image 2's rows between them in the buffer
    "features_tiny_counts": ("TINY", _LONG, [(0, 17), (1, 5), (2, 32), (1, 13), (3, 33)]),
    # vit_width 192 != dec_hidden 128: the rows pass through the visual projection (context tokens cannot exist on this model)
    "features_tinyl": ("TINY_L", _LONG, [(0, 17), (1, 33), (2, 9)]),
}
TF_LEN = 10


def feature_rows(cfg, rows: int, seed: int) -> torch.Tensor:
    """The row buffer of a case: fp32 [rows, vit_width], unit normal (the scale of LayerNorm outputs)."""
    return torch.randn(rows, cfg.vit_width, generator=torch.Generator().manual_seed(int(seed)))


def layout(pieces):
    """[(image, rows)] in buffer order -> (table [Q, 3] = (first row, rows, -1), image_of [Q], counts [B])"""
    table, image_of, src = [], [], 0
    counts = [0] * (max(im for im, _ in pieces) + 1)
    for im, n in pieces:
        table.append([src, n, -1])
        image_of.append(im)
        counts[im] += n
        src += n
    return table, image_of, counts


def image_features(rows, table, image_of, b):
    return torch.cat([rows[s:s + n] for (s, n, _), im in zip(table, image_of) if im == b], dim=0)[None]


def searched(model, cfg, w, search, vf):
    """The reference's answer for the features vf [1, n, D] and the margins of its decisions"""
    ref = model.infer({}, vf, None)
    mine = O.caption(cfg, w, None, search, feats=vf)
    assert torch.equal(mine["predictions"], ref["predictions"]), (mine["predictions"], ref["predictions"])
    assert (mine["logprobs"].reshape(-1) - ref["logprobs"].reshape(-1)).abs().max().item() < 1e-4
    history = model.use_history_for_infer
    model.use_history_for_infer, model.prev_encoded_layers = False, None
    try:
        step = functools.partial(model.decoding_step, vf, None, None)
        start = torch.full((1, 1), cfg.sos, dtype=torch.long)
        trace = []
        if search.kind == "greedy":
            preds, lps = O.search_autoregressive(start, step, cfg.eos, search.max_steps, search.beam_size,
                                                 search.per_node_beam_size, trace=trace)
        else:
            preds, lps = O.search_generator(start, step, cfg.eos, search.max_steps, search.beam_size, search.per_node_beam_size,
                                            search.length_penalty, trace=trace)
    finally:
        model.use_history_for_infer = history
    assert torch.equal(preds, ref["predictions"]), (preds, ref["predictions"])
    assert (lps.reshape(-1) - ref["logprobs"].reshape(-1)).abs().max().item() < 1e-4
    return ref["predictions"], ref["logprobs"].reshape(-1), torch.stack(trace, dim=1)


def per_image(model, cfg, w, search, feats):
    outs = [searched(model, cfg, w, search, vf) for vf in feats]
    B = len(outs)
    L, S = max(o[0].shape[1] for o in outs), max(o[2].shape[1] for o in outs)
    preds = torch.zeros(B, L, dtype=torch.long)
    margins = torch.full((B, S), float("inf"))
    for b, (p, _, m) in enumerate(outs):
        preds[b, :p.shape[1]] = p[0]
        margins[b, :m.shape[1]] = m[0]
    return preds, torch.cat([o[1] for o in outs]), margins


def teacher_forced(model, cfg, feats, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(feats)
    lens = [TF_LEN - (3 * b) % 5 for b in range(B)]
    tokens = torch.zeros(B, TF_LEN, dtype=torch.long)
    lp = torch.zeros(B, TF_LEN, dtype=torch.float64)
    lo, hi = float("inf"), float("-inf")
    for b, n in enumerate(lens):
        tokens[b, :n] = torch.randint(1, cfg.vocab, (n,), generator=g)
        tokens[b, 0] = cfg.sos
        logits = model.textual(feats[b], tokens[b:b + 1, :n]).float()
        ls = torch.log_softmax(logits.double(), dim=-1)
        for j in range(1, n):
            lp[b, j] = ls[0, j - 1, tokens[b, j]]
        lo, hi = min(lo, float(logits[0, :n - 1].min())), max(hi, float(logits[0, :n - 1].max()))
    return dict(tf_tokens=tokens.numpy(), tf_lengths=np.array(lens, dtype=np.int32), tf_lp=lp.numpy(), logit_min=np.float32(lo),
                logit_max=np.float32(hi))


def attempt(name, seed):
    cfg_name, wkw, pieces = CASES[name]
    cfg = O.CONFIGS[cfg_name]
    wkw = dict(wkw, seed=seed)
    w = O.make_weights(cfg, **wkw)
    table, image_of, counts = layout(pieces)
    feat_seed = sum(map(ord, name)) + seed
    rows = feature_rows(cfg, sum(counts), feat_seed)
    feats = [image_features(rows, table, image_of, b) for b in range(len(counts))]
    from oracle.make_golden import GOLD, build_reference
    out = {}
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tag, search in (("greedy", O.GREEDY), ("beam", O.BEAM4)):
            model = build_reference(cfg, w, search, wkw.get("tie_output", True))
            preds, lps, margins = per_image(model, cfg, w, search, feats)
            if float(margins.min()) < MIN_MARGIN:
                return f"seed {seed}: smallest {tag} decision margin {float(margins.min()):.2e} < {MIN_MARGIN:.0e}"
            out[f"{tag}_predictions"], out[f"{tag}_logprobs"] = preds.numpy(), lps.numpy()
            out[f"{tag}_margin"] = margins.numpy().astype(np.float32)
        tf = teacher_forced(model, cfg, feats, feat_seed + 1)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), config=cfg_name, weights_kw=repr(wkw), feat_seed=feat_seed,
                        counts=np.array(counts, dtype=np.int32), pieces=np.array(table, dtype=np.int32),
                        image_of=np.array(image_of, dtype=np.int32), **out, **tf)
    print(f"[{name}] seed {seed}  counts {counts}  min margins {float(out['greedy_margin'].min()):.4f} / "
          f"{float(out['beam_margin'].min()):.4f}  greedy {out['greedy_predictions'].tolist()}", flush=True)
    return None


def run(name, seeds=range(70, 4000)):
    from oracle.make_golden import import_reference
    _, D = import_reference()
    D.convert2valid = functools.partial(D.convert2valid, device="cpu")      # its default device is 'cuda' (decoder.py:612)
    for seed in seeds:
        why = attempt(name, seed)
        if why is None:
            return
        print(f"[{name}] {why}", flush=True)
    raise SystemExit(f"{name}: no seed of {seeds} gives decision margins >= {MIN_MARGIN:.0e}")


if __name__ == "__main__":
    for n in (sys.argv[1:] or list(CASES)):
        run(n)
