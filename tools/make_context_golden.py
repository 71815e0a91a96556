"""Freeze the context fixtures tests/golden/context_*.npz from the REFERENCE model (CPU only, run once).

The reference's CaptioningModel.forward_one accepts batch['context'], a list of {'tokens' [B, Lc], 'length' [B]}: it embeds the
tokens with the textual embedding, concatenates the rows to the visual features and masks the positions past every length as
keys.  Every case rebuilds the reference with oracle.make_golden.build_reference from seeded weights and images and records

  - the context (ctx_tokens_<i> [B, Lc], ctx_lengths_<i> [B] per list entry; ids past a length are random padding),
  - predictions / logprobs: what the reference returns for the batch WITH the context -- greedy cases from one batched call,
    beam cases from one batch-1 call per image (the reference cannot run B > 1 with beams > 1 and a context: decoding_step
    repeats the features per beam but not the validity mask),
  - predictions_plain: the same without the context,
  - step_margin: the decision margins of every search step, from the oracle's restatement of the search driven by the
    reference's own decoding_step (asserted to return the reference's ids),
  - tf_*: caption sequences with per-position log-probs (lp, mean_lp: log_softmax of the reference's fp32 logits in fp64, as
    tools/freeze_score_golden.py records them), logit_min / logit_max of the rows that count, and the reference's training-mode
    loss dict {'vl_<hint>_loss'} for batch['context_target_type'] = [hint].

Seeds are searched until (a) every image with context tokens gets ids that differ from its ids without them and (b) every
decision margin is at least 10 x tools/parity.F32_LOGIT_ABS; the script fails if no seed of its range does.  The key layout is
the one tests/conftest.golden_case reads, so tests rebuild weights and frames from the seeds.

    python tools/make_context_golden.py [case ...]
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
from oracle.make_golden import GOLD, build_reference, dataclass_tuple, import_reference  # noqa: E402
from tools.parity import F32_LOGIT_ABS  # noqa: E402

MIN_MARGIN = 10.0 * F32_LOGIT_ABS
_LONG = dict(tie_output=False, successor=2.0)
# name: (config, weights kw without the seed, batch, frames, search, prefix, [(Lc, lengths per image)] per context entry)
CASES = {
    # key counts 17 / 18 / 32 / 33 straddle the 32-key tile of the decode attention; image 3 has two segments (9 + 7)
    "context_tiny_greedy": ("TINY", _LONG, 4, 1, O.GREEDY, None, [(15, [0, 1, 15, 9]), (8, [0, 0, 0, 7])]),
    "context_tiny_beam4": ("TINY", dict(eos_bias=1.5, **_LONG), 4, 1, O.BEAM4, None, [(15, [0, 1, 15, 9]), (8, [0, 0, 0, 7])]),
    "context_tiny_prefix_beam4": ("TINY", dict(eos_bias=1.5, **_LONG), 1, 1, O.BEAM4, [101, 300, 2], [(8, [6])]),
    "context_video_greedy": ("TINY_VIDEO", _LONG, 2, 3, O.GREEDY, None, [(7, [5, 0]), (4, [3, 2])]),
}
TF_LEN = 12
HINT = "ocr"


def make_context(cfg, entries, B, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for Lc, lengths in entries:
        assert len(lengths) == B and max(lengths) <= Lc
        out.append({"tokens": torch.randint(1, cfg.vocab, (B, Lc), generator=g), "length": torch.tensor(lengths, dtype=torch.long)})
    return out


def slice_batch(frames, context, b):
    fr = [f[b:b + 1] for f in frames]
    batch = {"image": fr if len(fr) > 1 else fr[0]}
    if context is not None:
        batch["context"] = [{"tokens": c["tokens"][b:b + 1], "length": c["length"][b:b + 1]} for c in context]
    return batch


def run_reference(model, batch):
    """model(batch) plus the memory and validity mask forward_one handed on: -> (result, visual_features, visual_features_valid)"""
    seen = {}
    inner = model.forward_one_ce

    def spy(b, vf, vv, return_info=False):
        seen["vf"], seen["vv"] = vf, vv
        return inner(b, vf, vv, return_info)

    model.forward_one_ce = spy
    try:
        out = model(batch)
    finally:
        del model.forward_one_ce
    return out, seen["vf"], seen["vv"]


def searched(model, cfg, search, batch, prefix):
    """The reference's answer for `batch` and the margins of its decisions: -> (predictions, logprobs, margins [B, steps])"""
    if prefix is not None:
        batch = dict(batch, prefix=prefix)
    ref, vf, vv = run_reference(model, batch)
    # the oracle's restatement of the search, every step computed by the reference's decoding_step without its history cache
    history = model.use_history_for_infer
    model.use_history_for_infer, model.prev_encoded_layers = False, None
    try:
        step = functools.partial(model.decoding_step, vf, vv, None)
        B = vf.shape[0]
        start = prefix.long() if prefix is not None else torch.full((B, 1), cfg.sos, dtype=torch.long)
        trace = []
        if search.kind == "greedy":
            preds, lps = O.search_autoregressive(start, step, cfg.eos, search.max_steps, search.beam_size,
                                                 search.per_node_beam_size, trace=trace)
        else:
            preds, lps = O.search_generator(start, step, cfg.eos, search.max_steps, search.beam_size, search.per_node_beam_size,
                                            search.length_penalty, trace=trace)
    finally:
        model.use_history_for_infer = history
    if prefix is not None:
        preds = preds[:, start.shape[1]:]
    assert preds.shape == ref["predictions"].shape and torch.equal(preds, ref["predictions"]), (preds, ref["predictions"])
    assert (lps.reshape(-1) - ref["logprobs"].reshape(-1)).abs().max().item() < 1e-4
    return ref["predictions"], ref["logprobs"], torch.stack(trace, dim=1)


def per_image(model, cfg, search, frames, context, prefix, B):
    """One batch-1 reference call per image -> (predictions [B, L] padded with 0, logprobs [B, ...], margins [B, S] padded +inf)"""
    outs = [searched(model, cfg, search, slice_batch(frames, context, b), prefix) for b in range(B)]
    L = max(o[0].shape[1] for o in outs)
    S = max(o[2].shape[1] for o in outs)
    preds = torch.zeros(B, L, dtype=torch.long)
    margins = torch.full((B, S), float("inf"))
    for b, (p, _, m) in enumerate(outs):
        preds[b, :p.shape[1]] = p[0]
        margins[b, :m.shape[1]] = m[0]
    return preds, torch.cat([o[1] for o in outs], dim=0), margins


def teacher_forced(model, cfg, frames, context, B, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [TF_LEN - (3 * b) % 7 for b in range(B)]
    tokens = torch.zeros(B, TF_LEN, dtype=torch.long)
    need = torch.zeros(B, TF_LEN, dtype=torch.long)
    for b, n in enumerate(lens):
        tokens[b, :n] = torch.randint(1, cfg.vocab, (n,), generator=g)
        tokens[b, 0] = cfg.sos
        need[b, 1 + b % 3:n] = 1
    batch = {"image": frames if len(frames) > 1 else frames[0], "context": context}
    _, vf, vv = run_reference(model, batch)
    logits = model.textual(vf, tokens, hidden_valid_mask=vv).float()
    ls = torch.log_softmax(logits.double(), dim=-1)
    lp = torch.zeros(B, TF_LEN, dtype=torch.float64)
    mean_lp = torch.zeros(B, TF_LEN, dtype=torch.float64)
    counted = torch.zeros(B, TF_LEN, dtype=torch.bool)
    for b, n in enumerate(lens):
        counted[b, :n - 1] = True
        for j in range(1, n):
            lp[b, j] = ls[b, j - 1, tokens[b, j]]
            mean_lp[b, j] = ls[b, j - 1].mean()
    z = logits[counted]
    # the reference's loss: forward_one_ce with training set and every submodule in eval mode (no dropout)
    model.eval()
    model.training = True
    try:
        out = model(dict(batch, caption_tokens=tokens, need_predict=need, context_target_type=[HINT]))
    finally:
        model.training = False
    assert set(out) == {f"vl_{HINT}_loss"}, set(out)
    return dict(tf_tokens=tokens.numpy(), tf_need_predict=need.numpy(), tf_lengths=np.array(lens, dtype=np.int32),
                tf_lp=lp.numpy(), tf_mean_lp=mean_lp.numpy(), logit_min=np.float32(z.min()), logit_max=np.float32(z.max()),
                tf_loss=np.float64(float(out[f"vl_{HINT}_loss"])), tf_hint=HINT, tf_eps=np.float64(0.1))


def attempt(name, seed):
    cfg_name, wkw, B, F, search, prefix, entries = CASES[name]
    cfg = O.CONFIGS[cfg_name]
    wkw = dict(wkw, seed=seed)
    w = O.make_weights(cfg, **wkw)
    image_seed = sum(map(ord, name)) + seed
    frames = O.make_images(cfg, B, F, seed=image_seed)
    context = make_context(cfg, entries, B, image_seed + 1)
    counts = [sum(e[1][b] for e in entries) for b in range(B)]
    model = build_reference(cfg, w, search, wkw.get("tie_output", True))
    pfx = torch.tensor(prefix, dtype=torch.long)[None] if prefix is not None else None
    batched = search.kind == "greedy" and search.beam_size == 1
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if batched:
            full = {"image": frames if F > 1 else frames[0]}
            preds, lps, margins = searched(model, cfg, search, dict(full, context=context), pfx)
            plain, _, _ = searched(model, cfg, search, full, pfx)
            # batched greedy == one batch-1 call per image, up to each image's own end
            alone, alone_lp, _ = per_image(model, cfg, search, frames, context, pfx, B)
            for b in range(B):
                row = alone[b].tolist()
                n = row.index(cfg.eos) + 1 if cfg.eos in row else len([t for t in row if t])
                assert preds[b, :n].tolist() == row[:n], (name, b, preds[b], alone[b])
        else:
            preds, lps, margins = per_image(model, cfg, search, frames, context, pfx, B)
            plain, _, _ = per_image(model, cfg, search, frames, None, pfx, B)
        L = max(preds.shape[1], plain.shape[1])
        pad = lambda x: torch.cat([x, torch.zeros(B, L - x.shape[1], dtype=x.dtype)], 1)
        differs = [(pad(preds)[b] != pad(plain)[b]).any().item() for b in range(B)]
        if not all(d for d, c in zip(differs, counts) if c > 0):
            return f"seed {seed}: images {[b for b in range(B) if counts[b] and not differs[b]]} keep their ids with the context"
        if float(margins.min()) < MIN_MARGIN:
            return f"seed {seed}: smallest decision margin {float(margins.min()):.2e} < {MIN_MARGIN:.0e}"
        tf = teacher_forced(model, cfg, frames, context, B, image_seed + 2) if batched else {}
    ctx = {}
    for i, c in enumerate(context):
        ctx[f"ctx_tokens_{i}"] = c["tokens"].numpy()
        ctx[f"ctx_lengths_{i}"] = c["length"].numpy()
    np.savez_compressed(
        os.path.join(GOLD, name + ".npz"),
        config=cfg_name, weights_kw=repr(wkw), batch=B, frames=F, image_seed=image_seed, hw=np.array([], dtype=np.int64),
        search=repr(dataclass_tuple(search)), prefix=np.array(prefix if prefix is not None else [], dtype=np.int64),
        n_context=len(context), context_counts=np.array(counts, dtype=np.int32), per_image=not batched,
        predictions=preds.numpy(), logprobs=lps.numpy(), predictions_plain=plain.numpy(),
        step_margin=margins.numpy().astype(np.float32), **ctx, **tf)
    print(f"[{name}] seed {seed}  counts {counts}  min margin {float(margins.min()):.4f}  pred {tuple(preds.shape)}  "
          f"row0 {preds[0].tolist()}  plain row0 {plain[0].tolist()}", flush=True)
    return None


def run(name, seeds=range(70, 4000)):
    _, D = import_reference()
    D.convert2valid = functools.partial(D.convert2valid, device="cpu")      # its default device is 'cuda' (decoder.py:612)
    for seed in seeds:
        why = attempt(name, seed)
        if why is None:
            return
        print(f"[{name}] {why}", flush=True)
    raise SystemExit(f"{name}: no seed of {seeds} gives ids that change with the context and margins >= {MIN_MARGIN:.0e}")


if __name__ == "__main__":
    for n in (sys.argv[1:] or list(CASES)):
        run(n)
