"""Freeze the attention-map fixtures tests/golden/attend_*.npz from the REFERENCE model (CPU only, run once).

Every case rebuilds the reference CaptioningModel with oracle.make_golden.build_reference, sets output_attentions on the
six BertSelfAttention modules of the textual head, hooks them, runs model.textual(feats[image_of], tokens) and keeps the
text rows of the [Q, H, N + T, N + T] probabilities: att fp32 [Q, L, layers, N + L], the head mean taken in fp64, column
order [image tokens | text positions], 0 in rows past a sentence's length (and, by the mask, in text columns t > j).

The oracle's decoder weights are N(0, .02): the maps they give are nearly uniform and a wiring mistake (another layer, a
neighbouring position, the other image) would hide inside any 16-bit bound.  Every decoder layer's attention.self.query /
.key weights and biases are therefore multiplied by a scalar qk_gain (stored; the test applies it to the rebuilt weights).
It is chosen here, from the reference alone: the smallest value of GAINS at which
    p_max    = the largest per-head probability          <  0.99   (no head saturates), and
    swap_min = the smallest max-abs difference between the maps of adjacent layers, of positions j and j + 1, and of the
               same sentence over the other image         >= 0.01  (a wiring mistake is 4x any bound the test may hold).
The key layout is the one tests/conftest.golden_case reads (config, weights_kw, batch, frames, image_seed, hw, search, prefix).

    python tools/freeze_attend_golden.py [case ...]
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import git_oracle as O  # noqa: E402
from oracle.make_golden import build_reference, dataclass_tuple, GOLD  # noqa: E402

# name: (config, weights kw, images, frames, hw, sentences = (image, number of random ids after [CLS]))
# GIT_BASE: the maps of layers 4 and 5 of the N(0, .02) decoder are the closest pair; with sentences of fewer than ~15 tokens, or with
# weight seeds 83, 86 .. 90, some head passes 0.99 before they are 0.01 apart at any gain -- seed 85 and these lengths leave a window
CASES = {
    "attend_tiny_tied": ("TINY", dict(seed=81), 2, 1, None, [(1, 8), (0, 0), (0, 13), (1, 4)]),
    "attend_tiny_video": ("TINY_VIDEO", dict(seed=82, tie_output=False), 2, 3, None, [(0, 6), (1, 11), (1, 2)]),
    "attend_base": ("GIT_BASE", dict(seed=85), 2, 1, None, [(0, 19), (1, 15), (1, 22), (0, 17)]),
    "attend_vqa_480x640": ("GIT_BASE_VQAv2", dict(seed=84), 1, 1, (480, 640), [(0, 11)]),
}
GAINS = tuple(1.0 + 0.05 * i for i in range(61))          # 1.0 .. 4.0
P_MAX, SWAP_MIN = 0.99, 1e-2


def apply_qk_gain(w, gain: float):
    """The weights with every decoder layer's query / key projection (weight and bias) multiplied by `gain`."""
    out = dict(w)
    for k, v in w.items():
        if ".attention.self.query." in k or ".attention.self.key." in k:
            out[k] = v * gain
    return out


def text_row_maps(model, feats, tokens, N):
    """-> fp64 [Q, H, L, layers, N + L]: the text rows of every layer's attention probabilities"""
    mods = [m for m in model.textual.modules() if type(m).__name__ == "BertSelfAttention"]
    got, hooks = [], []
    for m in mods:
        m.output_attentions = True
        hooks.append(m.register_forward_hook(lambda _m, _i, out: got.append(out[1].double())))
    try:
        model.textual(feats, tokens)
    finally:
        for m, h in zip(mods, hooks):
            m.output_attentions = False
            h.remove()
    assert len(got) == len(mods)
    return torch.stack([p[:, :, N:, :] for p in got], dim=3)


def run(name: str) -> None:
    cfg_name, wkw, B, F, hw, sents = CASES[name]
    cfg = O.CONFIGS[cfg_name]
    w0 = O.make_weights(cfg, **wkw)
    seed = sum(map(ord, name))
    frames = O.make_images(cfg, B, F, seed=seed, hw=hw)
    g = torch.Generator().manual_seed(seed + 1)
    rows = [[cfg.sos] + torch.randint(1, cfg.vocab, (n,), generator=g).tolist() for _, n in sents]
    Q, L = len(rows), max(len(r) for r in rows)
    tokens = torch.zeros(Q, L, dtype=torch.long)
    for q, r in enumerate(rows):
        tokens[q, :len(r)] = torch.tensor(r)
    image_of = torch.tensor([s[0] for s in sents], dtype=torch.long)
    lens = [len(r) for r in rows]
    model = build_reference(cfg, w0, O.GREEDY, wkw.get("tie_output", True))
    qk = {n: p.data.clone() for n, p in model.textual.named_parameters()
          if ".attention.self.query." in n or ".attention.self.key." in n}
    assert len(qk) == 4 * cfg.dec_layers
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if F > 1:
            feats = [model.image_encoder(im) for im in frames]
            if cfg.num_frames:
                feats = [f + e for f, e in zip(feats, model.img_temperal_embedding)]
            feats = torch.cat(feats, dim=1)
        else:
            feats = model.image_encoder(frames[0])
    N = feats.shape[1]
    chosen = None
    for gain in GAINS:
        gain = round(gain, 2)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for n, p in model.textual.named_parameters():
                if n in qk:
                    p.data.copy_(qk[n] * gain)
            per_head = text_row_maps(model, feats[image_of], tokens, N)
            other = text_row_maps(model, feats[(image_of + 1) % B], tokens, N).mean(1) if B > 1 else None
        att = per_head.mean(1)                                                   # [Q, L, layers, N + L], fp64
        p_max, swaps = 0.0, []
        for q, n in enumerate(lens):
            a = att[q, :n]
            p_max = max(p_max, float(per_head[q, :, :n].max()))
            swaps += [(float((a[:, l] - a[:, l + 1]).abs().max()), f"sentence {q} layers {l}/{l + 1}") for l in range(a.shape[1] - 1)]
            swaps += [(float((a[j] - a[j + 1]).abs().max()), f"sentence {q} positions {j}/{j + 1}") for j in range(n - 1)]
            if other is not None:
                swaps.append((float((a - other[q, :n]).abs().max()), f"sentence {q} images"))
        swap_min, where = min(swaps)
        print(f"[{name}] gain {gain}: p_max {p_max:.4f} swap_min {swap_min:.3e} ({where})", flush=True)
        if p_max < P_MAX and swap_min >= SWAP_MIN:
            chosen = (gain, p_max, swap_min, att, N)
        if chosen is not None or p_max >= P_MAX:          # p_max grows with the gain: nothing further up can qualify
            break
    assert chosen is not None, f"{name}: no gain of {GAINS} gives p_max < {P_MAX} and swap_min >= {SWAP_MIN}"
    gain, p_max, swap_min, att, N = chosen
    for q, n in enumerate(lens):
        assert float((att[q, :n].sum(-1) - 1).abs().max()) < 1e-6
        att[q, n:] = 0
    np.savez_compressed(
        os.path.join(GOLD, name + ".npz"),
        config=cfg_name, weights_kw=repr(wkw), batch=B, frames=F, image_seed=seed,
        hw=np.array(hw if hw is not None else [], dtype=np.int64),
        search=repr(dataclass_tuple(O.GREEDY)), prefix=np.array([], dtype=np.int64),
        tokens=tokens.numpy(), image_of=image_of.numpy().astype(np.int32), lengths=np.array(lens, dtype=np.int32),
        att=att.float().numpy(), image_keys=np.int32(N), qk_gain=np.float64(gain), p_max=np.float64(p_max),
        swap_min=np.float64(swap_min),
    )
    print(f"[{name}] Q={Q} L={L} lens={lens} N={N} qk_gain={gain} p_max={p_max:.4f} swap_min={swap_min:.3e} "
          f"{os.path.getsize(os.path.join(GOLD, name + '.npz'))} bytes", flush=True)


if __name__ == "__main__":
    for n in (sys.argv[1:] or list(CASES)):
        run(n)
