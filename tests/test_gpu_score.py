"""Caption scoring on the MI355X (GITMI_SEARCH_SCORE, csrc/kernels_score.hip): per-token log-probabilities and the
reference's caption losses against fixtures frozen from the reference (tools/freeze_score_golden.py)."""
import ctypes as C
import glob
import os

import pytest
import torch

from conftest import GOLDEN, golden_case
from tools.parity import logit_bound

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "score_*.npz")))
PRECS = ("f32", "f16", "bf16")


def _engine(cfg, w, precision, B, F, Q, L, hw=None):
    from generativeimage2text_amd.engine import Engine
    beams = max(1, -(-Q // B))
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=beams, max_frames=F, max_text_len=max(L, 2),
                 max_image_hw=hw)
    eng.load_state_dict(w)
    return eng


def _case(name):
    g, cfg, w, frames, _, _ = golden_case(name)
    hw = tuple(int(v) for v in g["hw"]) if g["hw"].size else None
    return g, cfg, w, [f.cuda() for f in frames], hw


def _bound(g, precision):
    return 2.0 * logit_bound(precision, float(g["logit_max"]) - float(g["logit_min"]))


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_score_matches_reference(name, precision):
    from generativeimage2text_amd.model import caption_loss
    g, cfg, w, frames, hw = _case(name)
    tokens = torch.as_tensor(g["tokens"])
    Q, L = tokens.shape
    B, F = int(g["batch"]), int(g["frames"])
    eng = _engine(cfg, w, precision, B, F, Q, L, hw)
    out = eng.score(frames, tokens, lengths=g["lengths"].tolist(), image_of=g["image_of"].tolist()).cpu().double()
    eng.close()
    bound = _bound(g, precision)
    lp_ref, mean_ref = torch.as_tensor(g["lp"]), torch.as_tensor(g["mean_lp"])
    err_lp = (out[..., 0] - lp_ref).abs().max().item()
    err_mean = (out[..., 1] - mean_ref).abs().max().item()
    assert err_lp <= bound, (name, precision, err_lp, bound)
    assert err_mean <= bound, (name, precision, err_mean, bound)
    for loss_type, key in (("smooth", "vl_l_loss"), (None, "ce_loss")):
        got = caption_loss(out[..., 0], out[..., 1], tokens, g["need_predict"], loss_type, float(g["eps"]), cfg.vocab)
        ref = float(g[key])
        assert abs(got - ref) <= bound, (name, precision, key, got, ref)
        if precision == "f32":
            assert abs(got - ref) <= 1e-5 * abs(ref), (name, key, got, ref)


@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_score_equals_step_logits(precision):
    """lp at position t == log_softmax of the gitmi_step_logits row of the prefix tokens[:, :t] at tokens[:, t]."""
    from oracle import git_oracle as O
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=61, tie_output=False, successor=2.0)
    B, L = 3, 17
    frames = [f.cuda() for f in O.make_images(cfg, B, 1, seed=62)]
    gen = torch.Generator().manual_seed(63)
    tokens = torch.randint(1, cfg.vocab, (B, L), generator=gen)
    tokens[:, 0] = cfg.sos
    eng = _engine(cfg, w, precision, B, 1, B, L)
    out = eng.score(frames, tokens).cpu()
    ref_span = 0.0
    errs = []
    for t in (1, 2, 7, 16):
        eng.encode(frames, return_features=False)
        logits = eng.step_logits(tokens[:, :t].cuda()).double().cpu()
        ref_span = max(ref_span, float(logits.max() - logits.min()))
        ls = torch.log_softmax(logits, -1)
        errs.append((out[:, t, 0].double() - ls[torch.arange(B), tokens[:, t]]).abs().max().item())
        errs.append((out[:, t, 1].double() - ls.mean(-1)).abs().max().item())
    eng.close()
    assert max(errs) <= 2.0 * logit_bound(precision, ref_span), (errs, precision)


@pytest.mark.parametrize("precision", PRECS)
def test_batch_independence(precision):
    """Candidates scored together (ragged, several per image) == each scored alone."""
    from oracle import git_oracle as O
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=64, tie_output=False)
    B = 3
    frames = [f.cuda() for f in O.make_images(cfg, B, 1, seed=65)]
    gen = torch.Generator().manual_seed(66)
    lens = [2, 19, 7, 40, 1, 33, 16]
    image_of = [0, 0, 1, 2, 2, 1, 0]
    L = max(lens)
    tokens = torch.randint(1, cfg.vocab, (len(lens), L), generator=gen)
    tokens[:, 0] = cfg.sos
    eng = _engine(cfg, w, precision, B, 1, len(lens), L)
    together = eng.score(frames, tokens, lengths=lens, image_of=image_of).cpu()
    tol = 1e-6 if precision == "f32" else 2.0 * logit_bound(precision, 8.0)
    for q, (n, im) in enumerate(zip(lens, image_of)):
        alone = eng.score([f[im:im + 1] for f in frames], tokens[q:q + 1, :n]).cpu()
        assert (together[q, :n] - alone[0]).abs().max().item() <= tol, (q, precision)
        assert torch.all(together[q, n:] == 0)
        assert torch.all(together[q, 0] == 0)
    eng.close()


@pytest.mark.parametrize("name", ["score_tiny_untied", "score_tiny_video", "score_base"])
def test_training_forward_returns_reference_loss(name):
    """model.train(); model({'image', 'caption_tokens', 'need_predict'}) == the reference's vl_l_loss (decoder.py:938-966)."""
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel
    g, cfg, w, frames, hw = _case(name)
    image_of = torch.as_tensor(g["image_of"]).long()
    tokens = torch.as_tensor(g["tokens"])
    Q, L = tokens.shape
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=L, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision="f32", max_batch=Q, max_frames=int(g["frames"]), max_text_len=L)
    model.load_state_dict(w)
    assert model.training is False
    images = [f[image_of.cuda()] for f in frames] if int(g["frames"]) > 1 else frames[0][image_of.cuda()]
    batch = {"image": images, "caption_tokens": tokens, "need_predict": torch.as_tensor(g["need_predict"])}
    out = model.train()(batch)
    ref = float(g["vl_l_loss"])
    assert set(out) == {"vl_l_loss"}
    assert abs(float(out["vl_l_loss"]) - ref) <= 1e-5 * abs(ref), (float(out["vl_l_loss"]), ref)
    model.loss_type = None
    assert abs(float(model(batch)["vl_l_loss"]) - float(g["ce_loss"])) <= 1e-5 * float(g["ce_loss"])
    model.eval()
    assert model.training is False and "predictions" in model({"image": images})
    model.close()


@pytest.mark.parametrize("serving", (False, True))
def test_generate_score_generate_isolation(serving):
    """A score call between two generate calls on one engine (graphs on) leaves the generated ids unchanged."""
    from oracle import git_oracle as O
    from generativeimage2text_amd.engine import Engine
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=67, tie_output=False, successor=2.0)
    frames = [f.cuda() for f in O.make_images(cfg, 4, 1, seed=68)]
    other = [f.cuda() for f in O.make_images(cfg, 2, 1, seed=69)]
    eng = _engine(cfg, w, "f16", 4, 1, 8, 20)         # capacity 4 images x 2 candidates
    eng.set_graph(True)
    if serving:
        eng.set_shared_device(True)
    s = Engine.make_search("greedy", 20, 1, 1)
    t0, l0, _ = eng.generate(frames, s)
    tokens = torch.randint(1, cfg.vocab, (5, 12))
    tokens[:, 0] = cfg.sos
    eng.score(other, tokens, image_of=[0, 1, 1, 0, 1])
    t1, l1, _ = eng.generate(frames, s)
    assert torch.equal(t0.cpu(), t1.cpu())
    assert torch.equal(l0.cpu(), l1.cpu())
    eng.close()


def test_error_paths():
    from oracle import git_oracle as O
    from generativeimage2text_amd.engine import Engine, GitmiError, GitmiSearch, SEARCH_SCORE, _stream
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=70)
    frames = [f.cuda() for f in O.make_images(cfg, 2, 1, seed=71)]
    eng = _engine(cfg, w, "f32", 2, 1, 2, 10)          # capacity: 2 x 1 sentences of 10 tokens
    score = GitmiSearch()
    score.kind = SEARCH_SCORE
    with pytest.raises(GitmiError, match="SCORE"):
        eng.generate(frames, score)
    tok = torch.full((3, 12), 7, dtype=torch.int64, device="cuda")
    out = torch.empty(3, 12, 2, device="cuda")
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    arr = (C.c_void_p * 1)(frames[0].data_ptr())

    def call(Q, ld):
        lens = (C.c_int32 * Q)(*([2] * Q))
        img = (C.c_int32 * Q)(*([0] * Q))
        return eng.lib.gitmi_generate_prefixed(eng._h, arr, 1, 2, tok.data_ptr(), ld, lens, img, Q, C.byref(score), None,
                                               out.data_ptr(), None, info.data_ptr(), _stream())
    assert call(2, 11) != 0 and b"max_text_len" in eng.lib.gitmi_last_error()
    assert call(3, 10) != 0 and b"max_batch x max_beams" in eng.lib.gitmi_last_error()
    assert call(2, 10) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [10, 0, 0, 0]
    with pytest.raises(GitmiError):
        eng.score(frames, torch.full((3, 4), 7))
    with pytest.raises(ValueError):
        eng.score(frames, torch.full((2, 4), cfg.vocab))
    eng.close()


@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_long_sentences_against_oracle(precision):
    """Sentences longer than one 64-query attention tile (GIT_BASE, up to 100 tokens, ragged, image_of indirection) against
    the oracle's full recompute of the textual head (pinned to the reference in tests/test_oracle.py)."""
    from oracle import git_oracle as O
    cfg = O.CONFIGS["GIT_BASE"]
    w = O.make_weights(cfg, seed=72, tie_output=False, successor=1.0)
    frames = O.make_images(cfg, 2, 1, seed=73)
    gen = torch.Generator().manual_seed(74)
    lens, image_of = [100, 70, 5], [1, 0, 1]
    L = max(lens)
    tokens = torch.randint(1000, cfg.vocab, (3, L), generator=gen)
    tokens[:, 0] = cfg.sos
    with torch.no_grad():
        feats = O.visual_features(cfg, w, frames)
        z = O.textual_logits_full(cfg, w, feats[torch.tensor(image_of)], tokens).double()
    ls = torch.log_softmax(z, -1)
    eng = _engine(cfg, w, precision, 2, 1, 3, L)
    out = eng.score([f.cuda() for f in frames], tokens, lengths=lens, image_of=image_of).cpu().double()
    eng.close()
    span = 0.0
    errs = []
    for q, n in enumerate(lens):
        zq = z[q, :n - 1]
        span = max(span, float(zq.max() - zq.min()))
        lp = ls[q, torch.arange(n - 1), tokens[q, 1:n]]
        errs.append((out[q, 1:n, 0] - lp).abs().max().item())
        errs.append((out[q, 1:n, 1] - ls[q, :n - 1].mean(-1)).abs().max().item())
        assert torch.all(out[q, n:] == 0)
    assert max(errs) <= 2.0 * logit_bound(precision, span), (precision, errs)
