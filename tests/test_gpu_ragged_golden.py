"""Ragged image batches against fixtures frozen from the REFERENCE (tools/freeze_ragged_golden.py): every image run alone at
batch 1 and at its own shape, as the reference's inference.py does.  One ragged engine call must return the reference's ids
(f32: all of them; 16-bit: every row up to a decision whose fp32 margin -- over the tokens the search may pick -- is below the
tools/parity.py threshold), and the
custom-step path (gitmi_encode_frames + gitmi_prefill + gitmi_step_logits on the ragged batch) must give teacher-forced
logits within the tools/parity.py bound of the reference's."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import git_oracle as O
from tools.parity import tf_bounds

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "ragged_*.npz")))
PRECS = ("f32", "f16", "bf16")


def _case(name):
    g = load_golden(name)
    cfg = O.CONFIGS[str(g["config"])]
    w = O.make_weights(cfg, **ast.literal_eval(str(g["weights_kw"])))
    gen = torch.Generator().manual_seed(int(g["image_seed"]))          # the freeze tool draws the images first
    images = [torch.randn(3, int(h), int(ww), generator=gen) for h, ww in g["shapes"]]
    T = int(ast.literal_eval(str(g["search"]))[1])
    return g, cfg, w, images, T


def _engine(cfg, w, precision, g, T):
    from generativeimage2text_amd.engine import Engine
    Q = len(g["lengths"])
    beams = Q // len(g["shapes"])
    eng = Engine(cfg, precision=precision, max_batch=Q, max_beams=beams, max_frames=1, max_text_len=T,
                 max_image_hw=tuple(int(v) for v in g["hw"]))
    eng.load_state_dict(w)
    return eng


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_ragged_ids_match_reference(name, precision):
    from generativeimage2text_amd.engine import Engine
    g, cfg, w, images, T = _case(name)
    eng = _engine(cfg, w, precision, g, T)
    lens, plen, image_of = g["lengths"], g["prefix_len"], [int(i) for i in g["image_of"]]
    prefixes = [g["ids"][q, :plen[q]].tolist() for q in range(len(lens))]
    tok, _, sent, info = eng.generate_prefixed(eng.ragged([im.cuda() for im in images]), Engine.make_search("greedy", T, 1, 1),
                                               prefixes, image_of=image_of)
    tok, sent = tok.cpu(), sent.cpu()
    thr = tf_bounds(precision, float(g["logit_max"]) - float(g["logit_min"]))["thr"]
    for q in range(len(lens)):
        got, ref = tok[q, :int(sent[q, 0])].tolist(), g["ids"][q, :lens[q]].tolist()
        if precision == "f32":
            assert got == ref, (q, got, ref)
            continue
        diff = [i for i in range(min(len(got), len(ref))) if got[i] != ref[i]]
        if not diff:
            assert len(got) == len(ref) or g["dec_margin"][q].min() < thr, (q, got, ref)
            continue
        i = diff[0]
        assert i >= plen[q] and g["dec_margin"][q, :i].min() < thr, \
            f"row {q}: ids leave the reference at {i} although every earlier decision margin >= {thr:.4f}"
    eng.close()


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_ragged_teacher_forced_logits_match_reference(name, precision):
    """the custom-step path in ragged mode: encode + prefill of the ragged batch, then gitmi_step_logits over the reference's
    ids (rows of one image consecutive = its beams) at every position"""
    g, cfg, w, images, T = _case(name)
    eng = _engine(cfg, w, precision, g, T)
    eng.encode(eng.ragged([im.cuda() for im in images]), return_features=False)
    eng.prefill()
    b = tf_bounds(precision, float(g["logit_max"]) - float(g["logit_min"]))
    ids = torch.from_numpy(g["ids"])
    cols = torch.from_numpy(g["tf_cols"]).long()
    L = int(min(g["lengths"]))
    worst = 0.0
    for t in range(1, L):
        logits = eng.step_logits(ids[:, :t]).cpu()                     # predicts token t of every row
        err = (logits[:, cols] - torch.from_numpy(g["tf_logits"][:, t - 1])).abs().max().item()
        worst = max(worst, err)
        assert err < b["lerr"], (t, err, b["lerr"])
        sure = torch.from_numpy(g["tf_margin"][:, t - 1] >= b["thr"])
        am = logits.argmax(-1)
        assert torch.equal(am[sure], torch.from_numpy(g["tf_argmax"][:, t - 1])[sure]), t
    eng.close()
