"""Freeze the caption-scoring fixtures tests/golden/score_*.npz from the REFERENCE model (CPU only, run once).

Every case rebuilds the reference CaptioningModel with oracle.make_golden.build_reference and records, for a set of
caption sequences (each starting with [CLS], padded with 0) and the image every sequence belongs to:
  - lp / mean_lp [Q, L]: log_softmax of the reference's fp32 logits computed in fp64 -- lp[q, j] = log_softmax(z)[tok[q, j]],
    mean_lp[q, j] = mean over the vocabulary of log_softmax(z), z = the logits row at position j - 1 (0 at position 0 and
    past a row's length), logit_min / logit_max of the rows that count;
  - vl_l_loss: the reference's own smooth loss, model(batch) with model.training = True and its submodules in eval mode
    (decoder.py:938-966; dropout inactive), and ce_loss: the same with nn.CrossEntropyLoss(ignore_index=0).
The key layout is the one tests/conftest.golden_case reads (config, weights_kw, batch, frames, image_seed, hw, search,
prefix), so tests rebuild weights and frames from the seeds.

    python tools/freeze_score_golden.py [case ...]
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

# name: (config, weights kw, images, frames, hw, sentences) -- sentences: list of (image, tokens, need_predict prefix length)
#   tokens "greedy" = the reference's own greedy caption of that image; a list = given ids; ("rand", n) = [CLS] + n random ids
CASES = {
    "score_tiny_tied": ("TINY", dict(seed=41), 2, 1, None,
                        [(0, ("rand", 9), 1), (1, ("rand", 5), 1), (0, ("rand", 14), 4), (1, "greedy", 1)]),
    "score_tiny_untied": ("TINY", dict(seed=42, tie_output=False, eos_bias=1.0), 3, 1, None,
                          [(0, "greedy", 1), (1, ("rand", 18), 1), (2, ("rand", 3), 2), (2, ("rand", 1), 1), (0, ("rand", 11), 1)]),
    "score_tiny_video": ("TINY_VIDEO", dict(seed=43, tie_output=False, successor=2.0), 2, 3, None,
                         [(0, ("rand", 12), 1), (1, "greedy", 1), (1, ("rand", 7), 3)]),
    "score_base": ("GIT_BASE", dict(seed=44, tie_output=False, successor=1.0), 4, 1, None,
                   [(b, "greedy", 1) for b in range(4)] +
                   [(0, ("rand", 1), 1), (0, ("rand", 19), 1), (1, ("rand", 6), 3), (1, ("rand", 12), 5),
                    (2, ("rand", 9), 1), (2, ("rand", 15), 7), (3, ("rand", 4), 2), (3, ("rand", 17), 6)]),
    "score_vatex": ("GIT_BASE_VATEX", dict(seed=45), 1, 6, None, [(0, "greedy", 1), (0, ("rand", 10), 1)]),
    "score_vqa_480x640": ("GIT_BASE_VQAv2", dict(seed=46, tie_output=False, successor=4.0), 1, 1, (480, 640),
                          [(0, [101, 2054, 3609, 2003, 1996, 4937, 1029, 2304, 102], 7),
                           (0, [101, 2054, 3609, 2003, 1996, 4937, 1029, 2417, 102], 7),
                           (0, [101, 2054, 3609, 2003, 1996, 4937, 1029, 3756, 2630, 102], 7),
                           (0, [101, 2054, 3609, 2003, 1996, 4937, 1029, 2665, 102], 7)]),
}


def run(name: str) -> None:
    cfg_name, wkw, B, F, hw, sents = CASES[name]
    cfg = O.CONFIGS[cfg_name]
    w = O.make_weights(cfg, **wkw)
    seed = sum(map(ord, name))
    frames = O.make_images(cfg, B, F, seed=seed, hw=hw)
    model = build_reference(cfg, w, O.GREEDY, wkw.get("tie_output", True))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        greedy = None
        if any(t == "greedy" for _, t, _ in sents):
            greedy = O.caption(cfg, w, frames, O.GREEDY, cached=True)["predictions"]
        rows, npred = [], []
        for img, spec, p in sents:
            if spec == "greedy":
                r = greedy[img].tolist()                                    # [CLS] + the searched tokens
                r = r if r[0] == cfg.sos else [cfg.sos] + r
                r = r[:r.index(cfg.eos) + 1] if cfg.eos in r else r
            elif isinstance(spec, tuple):
                r = [cfg.sos] + torch.randint(1, cfg.vocab, (spec[1],), generator=g).tolist()
            else:
                r = list(spec)
            rows.append(r)
            npred.append(p)
        Q, L = len(rows), max(len(r) for r in rows)
        tokens = torch.zeros(Q, L, dtype=torch.long)
        need = torch.zeros(Q, L, dtype=torch.long)
        for q, r in enumerate(rows):
            tokens[q, :len(r)] = torch.tensor(r)
            need[q, npred[q]:len(r)] = 1
        image_of = torch.tensor([s[0] for s in sents], dtype=torch.long)
        lens = torch.tensor([len(r) for r in rows], dtype=torch.int32)
        # the reference's features, one row per sentence (its image), and its fp32 logits over the whole sequences
        if F > 1:
            feats = [model.image_encoder(im) for im in frames]
            if cfg.num_frames:
                feats = [f + e for f, e in zip(feats, model.img_temperal_embedding)]
            feats = torch.cat(feats, dim=1)
        else:
            feats = model.image_encoder(frames[0])
        logits = model.textual(feats[image_of], tokens).float()                   # [Q, L, V]
        ls = torch.log_softmax(logits.double(), dim=-1)
        lp = torch.zeros(Q, L, dtype=torch.float64)
        mean_lp = torch.zeros(Q, L, dtype=torch.float64)
        for q in range(Q):
            for j in range(1, int(lens[q])):
                lp[q, j] = ls[q, j - 1, tokens[q, j]]
                mean_lp[q, j] = ls[q, j - 1].mean()
        counted = torch.zeros(Q, L, dtype=torch.bool)
        for q in range(Q):
            counted[q, :int(lens[q]) - 1] = True
        z = logits[counted]
        # the reference's losses: forward_one_ce with training set and every submodule in eval mode (no dropout)
        batch = {"image": [f[image_of] for f in frames] if F > 1 else frames[0][image_of],
                 "caption_tokens": tokens, "need_predict": need}
        model.eval()
        model.training = True
        vl = float(model(batch)["vl_l_loss"])
        model.loss = torch.nn.CrossEntropyLoss(ignore_index=0)
        ce = float(model(batch)["vl_l_loss"])
        model.training = False
    np.savez_compressed(
        os.path.join(GOLD, name + ".npz"),
        config=cfg_name, weights_kw=repr(wkw), batch=B, frames=F, image_seed=seed,
        hw=np.array(hw if hw is not None else [], dtype=np.int64),
        search=repr(dataclass_tuple(O.GREEDY)), prefix=np.array([], dtype=np.int64),
        tokens=tokens.numpy(), need_predict=need.numpy(), image_of=image_of.numpy().astype(np.int32), lengths=lens.numpy(),
        lp=lp.numpy(), mean_lp=mean_lp.numpy(), logit_min=np.float32(z.min()), logit_max=np.float32(z.max()),
        vl_l_loss=np.float64(vl), ce_loss=np.float64(ce), eps=np.float64(0.1),
    )
    print(f"[{name}] Q={Q} L={L} lens={lens.tolist()} vl_l_loss={vl:.6f} ce={ce:.6f} "
          f"logits [{float(z.min()):.3f}, {float(z.max()):.3f}]", flush=True)


if __name__ == "__main__":
    for n in (sys.argv[1:] or list(CASES)):
        run(n)
