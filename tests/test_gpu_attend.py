"""Attention maps on the MI355X (GITMI_SEARCH_ATTEND, csrc/kernels_score.hip): Engine.attend against fixtures frozen from the
reference's BertSelfAttention.output_attentions (tools/freeze_attend_golden.py), and the call's contract -- the zeros, rows
that sum to 1, follow-up calls, batch independence, isolation from generate and score, the refusals.

Parity bound.  Measured once on the MI355X (profiles/attend_parity.json: the max-abs error per fixture and precision; DESIGN
section 14 repeats the table); BOUND is twice the worst recorded value of the precision -- the kernels are deterministic, the
margin covers compiler and runtime differences between machines and nothing else.  Every fixture also stores swap_min, the
smallest max-abs difference between maps a wiring mistake would confuse (adjacent layers, neighbouring positions, the two
images): the test requires BOUND <= swap_min / 4, so that no such mistake fits inside the bound."""
import ctypes as C
import glob
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT, golden_case
from tools.freeze_attend_golden import apply_qk_gain

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "attend_*.npz")))
PRECS = ("f32", "f16", "bf16")
MEASURED = json.load(open(os.path.join(ROOT, "profiles", "attend_parity.json")))["max_abs_error"]
BOUND = {p: 2.0 * max(MEASURED[n][p] for n in MEASURED) for p in PRECS}


def _engine(cfg, w, precision, B, F, Q, L, hw=None):
    from generativeimage2text_amd.engine import Engine
    beams = max(1, -(-Q // B))
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=beams, max_frames=F, max_text_len=max(L, 2), max_image_hw=hw)
    eng.load_state_dict(w)
    return eng


def _case(name):
    g, cfg, w, frames, _, _ = golden_case(name)
    hw = tuple(int(v) for v in g["hw"]) if g["hw"].size else None
    return g, cfg, apply_qk_gain(w, float(g["qk_gain"])), [f.cuda() for f in frames], hw


def _check_zeros_and_sums(att, lens, Nk, ntok=None, image_of=None):
    """att [Q, L, layers, Nk + L]: rows j >= len, text columns t > j and image columns past ntok are exactly 0; the other
    rows sum to 1 within 1e-4"""
    Q, L = att.shape[:2]
    for q, n in enumerate(lens):
        assert torch.all(att[q, n:] == 0), q
        for j in range(n):
            assert torch.all(att[q, j, :, Nk + j + 1:] == 0), (q, j)
        if ntok is not None:
            assert torch.all(att[q, :, :, ntok[image_of[q]]:Nk] == 0), q
        assert (att[q, :n].double().sum(-1) - 1).abs().max().item() <= 1e-4, q


def test_the_bound_discriminates_on_every_fixture():
    assert set(MEASURED) == set(CASES) and len(CASES) == 4
    for name in CASES:
        g = golden_case(name)[0]
        assert float(g["p_max"]) < 0.99 and float(g["swap_min"]) >= 1e-2, name
        for p in PRECS:
            assert BOUND[p] <= float(g["swap_min"]) / 4, (name, p, BOUND[p], float(g["swap_min"]))


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_attend_matches_reference(name, precision):
    g, cfg, w, frames, hw = _case(name)
    tokens = torch.as_tensor(g["tokens"])
    Q, L = tokens.shape
    B, F, Nk = int(g["batch"]), int(g["frames"]), int(g["image_keys"])
    lens, image_of = g["lengths"].tolist(), g["image_of"].tolist()
    eng = _engine(cfg, w, precision, B, F, Q, L, hw)
    att = eng.attend(frames, tokens, lengths=lens, image_of=image_of).cpu()
    eng.close()
    ref = torch.as_tensor(g["att"])
    assert att.shape == ref.shape == (Q, L, cfg.dec_layers, Nk + L)
    err = (att.double() - ref.double()).abs().max().item()
    print(f"ATTEND_PARITY {name} {precision} {err:.3e}")
    _check_zeros_and_sums(att, lens, Nk)
    assert BOUND[precision] <= float(g["swap_min"]) / 4, (name, precision, BOUND[precision], float(g["swap_min"]))
    assert err <= BOUND[precision], (name, precision, err, BOUND[precision])


def _tiny(seed, B, F=1):
    from oracle import git_oracle as O
    cfg = O.CONFIGS["TINY_VIDEO" if F > 1 else "TINY"]
    w = O.make_weights(cfg, seed=seed, tie_output=False, successor=2.0)
    frames = [f.cuda() for f in O.make_images(cfg, B, F, seed=seed + 1)]
    return cfg, w, frames


def _sentences(cfg, lens, seed):
    tokens = torch.randint(1, cfg.vocab, (len(lens), max(lens)), generator=torch.Generator().manual_seed(seed))
    tokens[:, 0] = cfg.sos
    return tokens


@pytest.mark.parametrize("precision", PRECS)
def test_followup_after_generate_is_bit_equal_to_the_full_call(precision):
    from generativeimage2text_amd.engine import Engine
    cfg, w, frames = _tiny(91, 3)
    lens, image_of = [5, 1, 12, 7], [2, 0, 0, 1]
    tokens = _sentences(cfg, lens, 92)
    eng = _engine(cfg, w, precision, 3, 1, 4, 12)
    full = eng.attend(frames, tokens, lengths=lens, image_of=image_of).cpu()
    eng.generate(frames, Engine.make_search("greedy", 12, 1, 1))
    follow = eng.attend(None, tokens, lengths=lens, image_of=image_of).cpu()
    eng.close()
    assert torch.equal(full, follow)


@pytest.mark.parametrize("precision", PRECS)
def test_batch_independence(precision):
    """Sentences attended together == each attended alone (over its own image, or as a subset of image_of), bit for bit;
    lengths on both sides of one 16-row tile of the map kernel."""
    cfg, w, frames = _tiny(93, 3, F=3)
    lens, image_of = [2, 19, 7, 33, 1, 16], [0, 0, 1, 2, 2, 1]
    tokens = _sentences(cfg, lens, 94)
    eng = _engine(cfg, w, precision, 3, 3, len(lens), max(lens))
    together = eng.attend(frames, tokens, lengths=lens, image_of=image_of).cpu()
    Nk = together.shape[-1] - max(lens)
    assert Nk == 3 * eng.n_tok
    _check_zeros_and_sums(together, lens, Nk)
    for q, (n, im) in enumerate(zip(lens, image_of)):
        alone = eng.attend([f[im:im + 1] for f in frames], tokens[q:q + 1, :n]).cpu()
        assert torch.equal(together[q, :n, :, :Nk + n], alone[0]), (q, precision)
    eng.attend(frames, tokens[:1], lengths=lens[:1], image_of=[0])
    subset = eng.attend(None, tokens[[3, 2]], lengths=[lens[3], lens[2]], image_of=[2, 1]).cpu()
    assert torch.equal(subset, together[[3, 2]])
    eng.close()


def test_generate_and_score_are_unchanged_by_an_attend_call():
    """generate -> attend -> generate returns identical ids (graphs on); a score call after an attend call equals one before"""
    from generativeimage2text_amd.engine import Engine
    cfg, w, frames = _tiny(95, 4)
    other = [f[:2].flip(0).contiguous() for f in frames]
    eng = _engine(cfg, w, "f16", 4, 1, 8, 20)
    eng.set_graph(True)
    s = Engine.make_search("greedy", 20, 1, 1)
    tokens = _sentences(cfg, [12] * 5, 96)
    t0, l0, _ = eng.generate(frames, s)
    sc0 = eng.score(frames, tokens, image_of=[0, 1, 3, 2, 1]).cpu()
    eng.attend(other, tokens, image_of=[0, 1, 1, 0, 1])
    t1, l1, _ = eng.generate(frames, s)
    sc1 = eng.score(None, tokens, image_of=[0, 1, 3, 2, 1]).cpu()
    eng.close()
    assert torch.equal(t0.cpu(), t1.cpu()) and torch.equal(l0.cpu(), l1.cpu())
    assert torch.equal(sc0, sc1)


def test_ragged_maps_end_at_every_images_own_tokens():
    """ragged input: Nk is the capacity, the image columns past an image's own tokens are exactly 0, and every image gets the
    map a call with that image alone gets (f32: bit for bit)"""
    from oracle import git_oracle as O
    from generativeimage2text_amd.engine import Engine
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=97, tie_output=False)
    p = cfg.patch
    gen = torch.Generator().manual_seed(98)
    imgs = [torch.randn(3, 2 * p, 3 * p, generator=gen).cuda(), torch.randn(3, 4 * p, 2 * p, generator=gen).cuda()]
    eng = Engine(cfg, precision="f32", max_batch=2, max_beams=2, max_frames=1, max_text_len=10, max_image_hw=(4 * p, 4 * p))
    eng.load_state_dict(w)
    lens, image_of = [4, 10, 1], [1, 0, 1]
    tokens = _sentences(cfg, lens, 99)
    att = eng.attend(eng.ragged(imgs), tokens, lengths=lens, image_of=image_of).cpu()
    Nk = eng.max_tokens
    assert att.shape == (3, 10, cfg.dec_layers, Nk + 10) and eng.resident_geometry == (Nk, 1, [(2, 3), (4, 2)])
    _check_zeros_and_sums(att, lens, Nk, ntok=[7, 9], image_of=image_of)
    for q, (n, im) in enumerate(zip(lens, image_of)):
        alone = eng.attend(eng.ragged([imgs[im]]), tokens[q:q + 1, :n]).cpu()
        assert torch.equal(att[q, :n, :, :Nk + n], alone[0]), q
    eng.close()


def test_refusals_and_info():
    from generativeimage2text_amd.engine import GitmiError, GitmiSearch, SEARCH_ATTEND, _stream
    cfg, w, frames = _tiny(100, 2)
    eng = _engine(cfg, w, "f32", 2, 1, 2, 10)
    attend = GitmiSearch()
    attend.kind = SEARCH_ATTEND
    with pytest.raises(GitmiError, match="ATTEND"):
        eng.generate(frames, attend)
    with pytest.raises(GitmiError, match="ATTEND"):
        eng.search_begin(attend, torch.full((2, 1), cfg.sos), cfg.vocab)
    with pytest.raises(GitmiError, match="no resident images"):
        eng.attend(None, torch.full((2, 4), 7), image_of=[0, 0])
    Kc = eng.n_tok + 10
    tok = torch.full((3, 12), 7, dtype=torch.int64, device="cuda")
    out = torch.empty(3 * 12 * cfg.dec_layers * (Kc + 2), device="cuda")
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    arr = (C.c_void_p * 1)(frames[0].data_ptr())

    def call(Q, ld):
        lens = (C.c_int32 * Q)(*([2] * Q))
        img = (C.c_int32 * Q)(*([0] * Q))
        return eng.lib.gitmi_generate_prefixed(eng._h, arr, 1, 2, tok.data_ptr(), ld, lens, img, Q, C.byref(attend), None,
                                               out.data_ptr(), None, info.data_ptr(), _stream())
    assert call(2, 11) != 0 and b"max_text_len" in eng.lib.gitmi_last_error()
    assert call(3, 10) != 0 and b"max_batch x max_beams" in eng.lib.gitmi_last_error()
    assert call(2, 10) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [10, Kc, cfg.dec_layers, 0]
    with pytest.raises(ValueError):
        eng.attend(frames, torch.full((2, 4), cfg.vocab))
    eng.close()


def test_captioning_model_attend_after_generate():
    """the natural use: caption the images, then one more call on the resident images for the maps of those captions"""
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel
    cfg, w, frames = _tiny(101, 2)
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=12, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision="f32", max_batch=2, max_text_len=12)
    model.load_state_dict(w)
    out = model({"image": frames[0]})
    captions = []
    for row in out["predictions"].tolist():                                   # the caption as generated, then three more ids
        ids = [int(t) for t in row if int(t) != cfg.eos]
        captions.append(([] if ids[:1] == [cfg.sos] else [cfg.sos]) + ids[:5] + [7, 8, 9])
    maps = model.attend(None, captions, on=out)
    full = model.attend(frames[0], captions)
    g = cfg.image_size // cfg.patch
    L = max(len(c) for c in captions)
    assert maps.image.shape == (2, L, cfg.dec_layers, g * g + 1) and maps.text.shape == (2, L, cfg.dec_layers, L)
    assert torch.equal(maps.image, full.image) and torch.equal(maps.text, full.text)
    grid = maps.patch_grid(1)
    assert grid.shape == (len(captions[1]), cfg.dec_layers, 1, g, g)
    assert torch.equal(grid[2, 1, 0, 1], maps.image[1, 2, 1, 1 + g:1 + 2 * g])
    model.close()
