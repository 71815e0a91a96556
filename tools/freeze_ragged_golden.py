"""Freeze the ragged-batch fixtures tests/golden/ragged_*.npz from the REFERENCE model (CPU only, run once).

The reference runs the aspect-preserving models one image per call (inference.py:172-199), so every image of a case is run
ALONE, at batch 1 and at its own shape, and every sentence with its own prefix:
  - ids [Q, L]: prefix + the reference's greedy answer (model({'image', 'prefix'}), prefix put back, 0-padded), lengths [Q];
  - teacher-forced logits of the reference's textual head over those ids (one pass, causal mask): for every position j < len - 1
    the logits that predict token j + 1 -- all columns for TINY, every COL_STRIDE-th column for GIT_BASE (1 MiB limit) --
    plus, from the full rows, their argmax and top-1 / top-2 margin (what the raw logits decide) and the span;
  - dec_margin [Q, L - 1]: the margin of the decision the greedy search actually makes at each answer position (the
    tools/parity.py margin): past a sentence's first search step the previous token is excluded (no immediate repeat,
    decoder.py:330), so top-1 / top-2 are taken over the other tokens; inf inside the prefix (no decision).
The key layout follows tests/conftest.golden_case (config, weights_kw, image_seed, search, hw), plus `shapes` [B, 2],
`image_of` [Q], `prefix_len` [Q].  Sentences are stored image-major (the questions of image b are consecutive).

    python tools/freeze_ragged_golden.py [case ...]
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

# name: (config, weights kw, capacity hw, image shapes, questions per image, question length range, max_steps, column stride)
CASES = {
    # TINY: 5 images of 4 sizes (token rows 17, 25, 33, 16, 25), one prefix each
    "ragged_tiny": ("TINY", dict(seed=61, tie_output=False, eos_bias=-1.0), (96, 128),
                    [(64, 64), (96, 64), (64, 128), (48, 80), (96, 64)], 1, (1, 4), 14, 1),
    # GIT_BASE_VQAv2: 4 MinMax shapes of the 480 / 640 model (1201, 1201, 901, 961 rows), two questions each
    "ragged_vqa_base": ("GIT_BASE_VQAv2", dict(seed=62, tie_output=False, successor=4.0), (480, 640),
                        [(480, 640), (640, 480), (480, 480), (360, 640)], 2, (4, 8), 14, 32),
}


def run(name: str) -> None:
    cfg_name, wkw, hw, shapes, nq, (qlo, qhi), T, stride = CASES[name]
    cfg = O.CONFIGS[cfg_name]
    w = O.make_weights(cfg, **wkw)
    seed = sum(map(ord, name))
    g = torch.Generator().manual_seed(seed)
    images = [torch.randn(1, 3, h, ww, generator=g) for h, ww in shapes]
    search = O.SearchConfig("greedy", T, 1, 1)
    model = build_reference(cfg, w, search, wkw.get("tie_output", True))
    rows, plen, image_of = [], [], []
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b, img in enumerate(images):
            for _ in range(nq):
                n = int(torch.randint(qlo, qhi + 1, (1,), generator=g))
                prefix = [cfg.sos] + torch.randint(200 if cfg.vocab < 2000 else 1000, cfg.vocab, (n,), generator=g).tolist()
                pred = model({"image": img, "prefix": torch.tensor([prefix])})["predictions"][0].tolist()
                r = prefix + pred
                r = r[:r.index(cfg.eos, 1) + 1] if cfg.eos in r[1:] else r
                rows.append(r)
                plen.append(len(prefix))
                image_of.append(b)
        Q, L = len(rows), max(len(r) for r in rows)
        ids = np.zeros((Q, L), dtype=np.int64)
        for q, r in enumerate(rows):
            ids[q, :len(r)] = r
        V = cfg.vocab
        cols = np.arange(0, V, stride)
        tf = np.zeros((Q, L - 1, len(cols)), dtype=np.float32)
        tf_argmax = np.full((Q, L - 1), -1, dtype=np.int64)
        tf_margin = np.zeros((Q, L - 1), dtype=np.float32)
        dec_margin = np.full((Q, L - 1), np.inf, dtype=np.float32)
        lo, hi = np.inf, -np.inf
        for q, r in enumerate(rows):
            feats = model.image_encoder(images[image_of[q]])
            z = model.textual(feats, torch.tensor([r]))[0].float()[:len(r) - 1]          # [len - 1, V]
            tf[q, :len(r) - 1] = z[:, cols].numpy()
            top = torch.topk(z.double(), 2, dim=-1)
            tf_argmax[q, :len(r) - 1] = top.indices[:, 0].numpy()
            tf_margin[q, :len(r) - 1] = (top.values[:, 0] - top.values[:, 1]).float().numpy()
            P = plen[q]
            for j in range(P - 1, len(r) - 1):                            # logits at j decide token j + 1
                zz = z[j].double().clone()
                if j >= P:
                    zz[r[j]] = -float("inf")
                t2 = torch.topk(zz, 2).values
                dec_margin[q, j] = float(t2[0] - t2[1])
            lo, hi = min(lo, float(z.min())), max(hi, float(z.max()))
    np.savez_compressed(
        os.path.join(GOLD, name + ".npz"),
        config=cfg_name, weights_kw=repr(wkw), image_seed=seed, hw=np.array(hw, dtype=np.int64),
        shapes=np.array(shapes, dtype=np.int64), search=repr(dataclass_tuple(search)),
        ids=ids, lengths=np.array([len(r) for r in rows], dtype=np.int32), prefix_len=np.array(plen, dtype=np.int32),
        image_of=np.array(image_of, dtype=np.int32), tf_cols=cols.astype(np.int32), tf_logits=tf, tf_argmax=tf_argmax,
        tf_margin=tf_margin, dec_margin=dec_margin, logit_min=np.float32(lo), logit_max=np.float32(hi),
    )
    print(f"[{name}] Q={Q} L={L} lengths={[len(r) for r in rows]} prefix={plen} logits [{lo:.3f}, {hi:.3f}] "
          f"min decision margin {float(dec_margin.min()):.4f}", flush=True)


if __name__ == "__main__":
    for n in (sys.argv[1:] or list(CASES)):
        run(n)
