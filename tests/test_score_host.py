"""caption_loss (model.py) against the reference's own losses frozen in tests/golden/score_*.npz: fed the fixture's
per-position log-probabilities (computed in fp64 from the reference's fp32 logits), the host reduction must give the
reference's SmoothLabelCrossEntropyLoss / nn.CrossEntropyLoss values (decoder.py:620-671, 814-817, 938-966)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from generativeimage2text_amd.model import caption_loss

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "score_*.npz")))


def test_fixtures_present():
    assert {"score_tiny_tied", "score_tiny_untied", "score_tiny_video"} <= set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_losses_reduce_to_reference(name):
    from oracle import git_oracle as O
    g = load_golden(name)
    V = O.CONFIGS[str(g["config"])].vocab
    smooth = caption_loss(g["lp"], g["mean_lp"], g["tokens"], g["need_predict"], "smooth", float(g["eps"]), V)
    ce = caption_loss(g["lp"], g["mean_lp"], g["tokens"], g["need_predict"], None, 0.1, V)
    # the reference sums fp32 KL terms over the vocabulary: agreement to fp32 rounding of ~V terms
    assert abs(smooth - float(g["vl_l_loss"])) <= 2e-5 * max(1.0, abs(float(g["vl_l_loss"]))), (smooth, g["vl_l_loss"])
    assert abs(ce - float(g["ce_loss"])) <= 2e-6 * max(1.0, abs(float(g["ce_loss"]))), (ce, g["ce_loss"])


def _toy(V=7, seed=0):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(2, 5, V, generator=gen, dtype=torch.float64)
    tokens = torch.tensor([[101 % V, 3, 0, 5, 0], [1, 2, 6, 4, 1]])
    ls = torch.log_softmax(z, -1)
    lp = torch.zeros(2, 5, dtype=torch.float64)
    mean = torch.zeros(2, 5, dtype=torch.float64)
    for q in range(2):
        for j in range(1, 5):
            lp[q, j] = ls[q, j - 1, tokens[q, j]]
            mean[q, j] = ls[q, j - 1].mean()
    return z, tokens, lp, mean


def _reference_smooth(z, tokens, need, eps):
    """SmoothLabelCrossEntropyLoss(ignore_index=0) as decoder.py:620-671 computes it, in fp64."""
    target = tokens.clone()
    target[need == 0] = 0
    feat = z[:, :-1].reshape(-1, z.shape[-1])
    target = target[:, 1:].reshape(-1)
    keep = need[:, 1:].reshape(-1) == 1
    feat, target = feat[keep], target[keep]
    valid = target != 0
    feat, target = feat[valid], target[valid]
    n = feat.shape[1]
    one = torch.zeros_like(feat).scatter(1, target.view(-1, 1), 1)
    one = one * (1 - eps) + (1 - one) * eps / (n - 1)
    return float(torch.nn.functional.kl_div(torch.log_softmax(feat, 1), one, reduction="none").sum(1).mean())


def test_masking_rules():
    V = 7
    z, tokens, lp, mean = _toy(V)
    need = torch.tensor([[0, 1, 1, 1, 1], [0, 0, 1, 1, 1]])            # row 1: a question prefix of two tokens
    got = caption_loss(lp, mean, tokens, need, "smooth", 0.1, V)
    assert got == pytest.approx(_reference_smooth(z, tokens, need, 0.1), abs=1e-12)
    # positions with need_predict 0 or target 0 do not count: changing their scores changes nothing
    lp2, mean2 = lp.clone(), mean.clone()
    lp2[0, 2] = lp2[0, 4] = lp2[1, 1] = -1e3
    mean2[1, 1] = -1e3
    assert caption_loss(lp2, mean2, tokens, need, "smooth", 0.1, V) == got
    ce = caption_loss(lp, mean, tokens, need, None, 0.1, V)
    sel = (need[:, 1:] == 1) & (tokens[:, 1:] != 0)
    assert ce == pytest.approx(float(-lp[:, 1:][sel].mean()), abs=1e-12)


def test_all_masked():
    V = 7
    _, tokens, lp, mean = _toy(V)
    need = torch.zeros_like(tokens)
    with pytest.raises(AssertionError):
        caption_loss(lp, mean, tokens, need, "smooth", 0.1, V)       # the reference asserts target.numel() > 0
    assert np.isnan(caption_loss(lp, mean, tokens, need, None, 0.1, V))  # nn.CrossEntropyLoss: mean over nothing
