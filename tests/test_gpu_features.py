"""Features in (include/gitmi.h: GITMI_SEARCH_FEATURES): caller-supplied visual feature rows become the resident image batch of a
context and every follow-up form runs over them.  The features of an encode handed back in must give every follow-up bit for
bit what it gave after the encode (every precision, fp32 and 16-bit rows); arbitrary rows of unequal counts must give every
image what the reference's CaptioningModel.infer(batch, visual_features, ...) returns for it alone (fixtures frozen by
tools/make_features_golden.py); video windows composed from per-frame rows plus the temporal index must equal the list-form
call; the rows a KEEP finds must be the expected conversion bit for bit; and every refusal must be a return code and a message
found on the host before any launch.  (On the parent commit every call of this kind fails with "search: bad kind".)"""
import ast
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_case, load_golden
from oracle import git_oracle as O

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16", "bf16")
OPERAND = {"f16": torch.float16, "bf16": torch.bfloat16}
# (engine precision, dtype of the installed rows)
ROWS = [("f32", "f32"), ("f16", "f32"), ("f16", "op"), ("bf16", "f32"), ("bf16", "op")]


def _engine(cfg, w, precision, B, beams=4, T=20, F=1, max_context=0, graph=True):
    from generativeimage2text_amd.engine import Engine
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=beams, max_frames=F, max_text_len=T, max_context=max_context)
    eng.load_state_dict(w)
    eng.set_graph(graph)
    return eng


def _search(kind, T, k=1, pn=1, lp=0.6, **kw):
    from generativeimage2text_amd.engine import Engine
    return Engine.make_search(kind, T, k, pn, lp, **kw)


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(_bits(x), _bits(y)), (x, y)


def _rows_as(feats, precision, kind):
    return feats if kind == "f32" else feats.to(OPERAND[precision])


CAPS = torch.tensor([[101, 5, 6, 7, 102, 0], [101, 9, 10, 102, 0, 0], [101, 300, 2, 9, 512, 102]])
CAP_LENS = [5, 4, 6]


def _followups(eng, T, B):
    """greedy, beam-4 (generator) and score follow-ups over the resident images"""
    out = list(eng.generate(None, _search("greedy", T)))
    out += list(eng.generate(None, _search("beam", T, 4, 2, 0.6)))
    out.append(eng.score(None, CAPS[:B], lengths=CAP_LENS[:B]))
    return [t.cpu() for t in out]


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision, rows", ROWS)
def test_features_of_an_encode_handed_back_restore_every_followup_bit_for_bit(precision, rows):
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=81, tie_output=False, successor=2.0, eos_bias=1.0)
    frames = [f.cuda() for f in O.make_images(cfg, 3, 1, seed=82)]
    T = 14
    eng = _engine(cfg, w, precision, 3, T=T)
    feats = eng.encode(frames)
    want = _followups(eng, T, 3)
    other = eng.generate([torch.roll(f, 1, dims=-1) * 0.5 + 0.25 for f in frames], _search("greedy", T))
    assert not torch.equal(other[0].cpu(), want[0])
    gen = eng.generation
    info = eng.install_features(_rows_as(feats, precision, rows))
    assert info == {"stride": 17, "max_rows": 17, "total_rows": 51}
    assert eng.resident == 3 and eng.generation > gen and eng.resident_geometry == (17, 1, [(4, 4)] * 3)
    _same(want, _followups(eng, T, 3))
    _same(want, _followups(eng, T, 3))                                  # the second round replays the follow-up graphs
    eng.close()


# ---- 2. arbitrary features, unequal counts: the reference per image ---------------------------------------------------------------
_FIX = {}


def _fixture(name):
    """(golden arrays, cfg, weights, feature rows fp32 [R, D] on the CPU), built once per session"""
    if name not in _FIX:
        from tools.make_features_golden import feature_rows
        g = load_golden(name)
        cfg = O.CONFIGS[str(g["config"])]
        w = O.make_weights(cfg, **ast.literal_eval(str(g["weights_kw"])))
        _FIX[name] = (g, cfg, w, feature_rows(cfg, int(g["counts"].sum()), int(g["feat_seed"])))
    return _FIX[name]


def _ids_equal(tok, ref, eos):
    for b in range(ref.shape[0]):
        row = ref[b].tolist()
        n = row.index(eos) + 1 if eos in row else len(row)
        assert tok[b, :n].tolist() == row[:n], (b, tok[b].tolist(), row)


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", ["features_tiny_counts", "features_tinyl"])
def test_arbitrary_rows_of_unequal_counts_give_every_image_its_reference_call(name, precision):
    """features_tiny_counts: key counts 17 / 18 / 32 / 33 (either side of the decode attention's 32-key tile and of the 16-row
    install tile), image 1 in two pieces 5 + 13 that are not adjacent in the buffer, an engine with max_image_tokens = 48.
    features_tinyl: vit_width 192 != dec_hidden 128, where context tokens cannot exist.  f32: the reference's ids, greedy and beam
    4 (every margin of the fixtures is >= 10 x F32_LOGIT_ABS, asserted when they were frozen), log-probs within 1e-4 as
    tests/test_gpu_context.py holds them; 16-bit: the teacher-forced log-probs of a score follow-up within 2 x logit_bound."""
    from tools.parity import F32_LOGIT_ABS, logit_bound
    g, cfg, w, rows = _fixture(name)
    counts = g["counts"].tolist()
    B, T = len(counts), 20
    assert min(float(g["greedy_margin"].min()), float(g["beam_margin"].min())) >= 10 * F32_LOGIT_ABS
    # five pieces for four images need max_frames = 2 (Q <= max_batch x max_frames); 31 more rows per frame: max_image_tokens = 48
    F, ctx = (2, 62) if name == "features_tiny_counts" else (1, 16)
    eng = _engine(cfg, w, precision, B, T=T, F=F, max_context=ctx)
    assert eng.max_tokens == (48 if name == "features_tiny_counts" else 33)
    info = eng.install_features(rows.cuda(), [tuple(p) for p in g["pieces"].tolist()], g["image_of"].tolist())
    stride = -(-max(counts) // 16) * 16 if -(-max(counts) // 16) * 16 <= eng.memory_rows else max(counts)
    assert info == {"stride": stride, "max_rows": max(counts), "total_rows": sum(counts)}
    geo = eng.resident_geometry
    assert geo.stride == stride and geo.rows == counts and geo.context == [0] * B and geo[2] == [None] * B
    if precision == "f32":
        tok, lp, inf = (t.cpu() for t in eng.generate(None, _search("greedy", T)))
        assert int(inf[3]) == 0
        _ids_equal(tok, g["greedy_predictions"], cfg.eos)
        assert np.allclose(lp.numpy(), g["greedy_logprobs"], atol=1e-4), (lp, g["greedy_logprobs"])
        tok, lp, inf = (t.cpu() for t in eng.generate(None, _search("beam", T, 4, 2, 0.6)))
        _ids_equal(tok, g["beam_predictions"], cfg.eos)
        assert np.allclose(lp.numpy().reshape(-1), g["beam_logprobs"], atol=1e-4), (lp, g["beam_logprobs"])
    bound = 2 * logit_bound(precision, float(g["logit_max"]) - float(g["logit_min"]))
    lens = g["tf_lengths"].tolist()
    got = eng.score(None, torch.from_numpy(g["tf_tokens"]), lengths=lens).cpu()[..., 0].double().numpy()
    for b, n in enumerate(lens):
        err = float(np.abs(got[b, 1:n] - g["tf_lp"][b, 1:n]).max())
        print(f"{name} {precision} image {b} ({counts[b]} rows): teacher-forced log-prob error {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (b, err, bound)
    eng.close()


# ---- 3. video windows --------------------------------------------------------------------------------------------------------------
def _window_pieces(order, B, N):
    """rows of a frame-major bare pass over len(order) frames of B videos -> the pieces of B windows, frame i at temporal index i"""
    pieces, image_of = [], []
    for b in range(B):
        for i, fr in enumerate(order):
            pieces.append(((fr * B + b) * N, N, i))
            image_of.append(b)
    return pieces, image_of


@pytest.mark.parametrize("precision", PRECS)
def test_video_windows_from_one_bare_pass_equal_the_list_call_bit_for_bit(precision):
    """2 videos, 4 frames.  The list call encodes its 3 frames as one pass of 6 images, frame-major; the bare call over the same 6
    images is the same pass without the temporal embedding, which install adds as layernorm_kernel's add_after does: a separate
    fp32 add.  The window (f0, f1, f2) and the slid window (f1, f2, f3) must each equal their own list call in every precision."""
    g, cfg, w, frames, _, _ = golden_case("tiny_video_greedy")
    frames = [f.cuda() for f in frames] + [f.cuda() for f in O.make_images(cfg, 2, 1, seed=4242)]
    T, N = 14, 17
    eng = _engine(cfg, w, precision, 6, T=T, F=3)
    for first in (0, 1):
        window = frames[first:first + 3]
        eng.set_temporal_embedding(True)
        eng.generate(window, _search("greedy", T))
        want = _followups(eng, T, 2)
        eng.set_temporal_embedding(False)
        feats = eng.encode([torch.cat(window, dim=0)])
        assert feats.shape == (6, N, cfg.vit_width)
        pieces, image_of = _window_pieces([0, 1, 2], 2, N)
        info = eng.install_features(feats.reshape(-1, cfg.vit_width), pieces, image_of, F=3)
        assert info == {"stride": 51, "max_rows": 51, "total_rows": 102} and eng.resident_geometry == (51, 3, [(4, 4)] * 2)
        _same(want, _followups(eng, T, 2))
    eng.close()


@pytest.mark.parametrize("name", ["tiny_video_greedy", "tiny_video_beam4"])
def test_video_windows_from_frames_encoded_one_at_a_time_reproduce_the_goldens_in_f32(name):
    g, cfg, w, frames, search, _ = golden_case(name)
    T = search.max_steps
    eng = _engine(cfg, w, "f32", 2, beams=search.beam_size, T=T, F=3)
    eng.set_temporal_embedding(False)
    rows = torch.cat([eng.encode([f.cuda()]).reshape(-1, cfg.vit_width) for f in frames], dim=0)      # [3 frames x 2 videos x 17, D]
    pieces, image_of = _window_pieces([0, 1, 2], 2, 17)
    eng.install_features(rows, pieces, image_of, F=3)
    tok, lp, inf = (t.cpu() for t in eng.generate(None, _search(search.kind, T, search.beam_size, search.per_node_beam_size,
                                                                search.length_penalty)))
    assert int(inf[3]) == 0
    _ids_equal(tok, g["predictions"], cfg.eos)
    assert np.allclose(lp.numpy().reshape(-1), g["logprobs"].reshape(-1), atol=1e-4), (lp, g["logprobs"])
    eng.close()


def test_bare_tensor_video_features_carry_no_temporal_embedding():
    """the expectation of tests/test_gpu_parity.py::test_video_model_with_bare_tensor_skips_temporal_embedding: rows installed
    without a temporal index are the bare-tensor call's features; with index 0 they are the list call's"""
    cfg = O.CONFIGS["TINY_VIDEO"]
    w = O.make_weights(cfg, seed=53, tie_output=False, successor=2.0)
    frames = O.make_images(cfg, 2, 1, seed=6)
    search = O.SearchConfig("greedy", 12, 1, 1)
    with torch.no_grad():
        ref_tensor = O.caption(cfg, w, frames, search, cached=True, feats=O.visual_features(cfg, w, frames, as_list=False))
        ref_list = O.caption(cfg, w, frames, search, cached=True)
    assert not torch.equal(ref_tensor["predictions"], ref_list["predictions"])
    eng = _engine(cfg, w, "f32", 2, beams=1, T=12, F=3)
    eng.set_temporal_embedding(False)
    feats = eng.encode([frames[0].cuda()])
    eng.install_features(feats)
    tok, _, info = eng.generate(None, _search("greedy", 12))
    assert torch.equal(tok[:, :int(info[0])].cpu(), ref_tensor["predictions"])
    eng.install_features(feats.reshape(-1, cfg.vit_width), [(0, 17, 0), (17, 17, 0)], [0, 1])
    tok, _, info = eng.generate(None, _search("greedy", 12))
    assert torch.equal(tok[:, :int(info[0])].cpu(), ref_list["predictions"])
    eng.close()


# ---- 4. stored rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision, rows", ROWS)
def test_kept_slots_hold_the_expected_conversion_of_every_row(precision, rows):
    """counts 17 / 33; image 1 is a piece of 17 rows with temporal index 1 and a piece of 16 rows without.  KEEP, then read the
    feature planes: fp32 rows + embedding in fp32, stored as is (f32) or rounded once to nearest even (torch's conversion); 16-bit
    rows without an index bit for bit, with one widened, added to and rounded once.  Header: n, 0 context rows, the F given."""
    cfg = O.CONFIGS["TINY_VIDEO"]
    w = O.make_weights(cfg, seed=19, tie_output=False, successor=2.0)
    D, T = cfg.vit_width, 12
    eng = _engine(cfg, w, precision, 2, beams=1, T=T, F=2)
    src = torch.randn(60, D, generator=torch.Generator().manual_seed(7)).cuda()
    src = _rows_as(src, precision, rows)
    pieces, image_of, counts = [(40, 17, None), (3, 17, 1), (22, 16, None)], [0, 1, 1], [17, 33]
    info = eng.install_features(src, pieces, image_of, F=2)
    assert info == {"stride": 33, "max_rows": 33, "total_rows": 50}     # round_up(33, 16) = 48 > cap = 34: the stride is max n
    want = [t.cpu() for t in eng.generate(None, _search("greedy", T))]
    store = eng.memory_store(2)
    kept = eng.keep(store, [1, 0])                                      # image 0 -> slot 1, image 1 -> slot 0
    assert kept["rows"] == counts and kept["geometry"] == [(2, None, 17, 0), (2, None, 33, 0)]
    te = w["img_temperal_embedding.1"].reshape(-1).cuda()
    dt = torch.float32 if precision == "f32" else OPERAND[precision]
    wide = src.float()
    expect = {1: wide[40:57].to(dt), 0: torch.cat([(wide[3:20] + te).to(dt), src[22:38] if src.dtype == dt else wide[22:38].to(dt)])}
    for slot, n in ((1, 17), (0, 33)):
        hdr = store[slot, :64].view(torch.int32).tolist()
        assert hdr[9:13] == [n, n, 0, 2], hdr                           # n, image rows, context rows, F
        plane = store[slot, 256:256 + n * D * expect[slot].element_size()].view(dt).reshape(n, D)
        assert torch.equal(plane.view(torch.int32 if dt == torch.float32 else torch.int16),
                           expect[slot].view(torch.int32 if dt == torch.float32 else torch.int16)), slot
    clone = eng.clone()
    clone.set_graph(True)
    clone.recall(store, [1, 0], kept["geometry"])
    _same(want, [t.cpu() for t in list(clone.generate(None, _search("greedy", T)))])
    clone.close()
    eng.close()


# ---- 5. reinstall ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_a_smaller_batch_after_a_larger_one_and_two_batches_of_one_stride(precision):
    """33 rows, then 17 rows in the same blocks: what the first install left behind row 17 must not be read (rows [n_b, stride)
    are rewritten as zeros, key counts bound the attention).  Two key-count batches of stride 32 with different counts replay one
    follow-up graph; each result must belong to its own features."""
    g, cfg, w, rows = _fixture("features_tiny_counts")
    rows = rows.cuda()
    T = 14

    def fresh(pieces, image_of):
        e = _engine(cfg, w, precision, 2, T=T, max_context=31)
        e.install_features(rows, pieces, image_of)
        out = _followups(e, T, 2)
        e.close()
        return out

    eng = _engine(cfg, w, precision, 2, T=T, max_context=31)
    big = ([(0, 33), (40, 33)], [0, 1])
    small = ([(50, 17), (10, 17)], [0, 1])                              # the uniform shape: no key counts
    a = ([(0, 17), (20, 20)], [0, 1])                                   # stride 32
    b = ([(30, 25), (5, 18)], [0, 1])                                   # stride 32, other counts, other rows
    assert eng.install_features(rows, *big)["stride"] == 48
    _followups(eng, T, 2)
    assert eng.install_features(rows, *small)["stride"] == 17 and not hasattr(eng.resident_geometry, "rows")
    _same(fresh(*small), _followups(eng, T, 2))
    want_a, want_b = fresh(*a), fresh(*b)
    assert not torch.equal(want_a[0], want_b[0]) or not torch.equal(_bits(want_a[1]), _bits(want_b[1]))
    for pieces, want in ((a, want_a), (b, want_b), (a, want_a)):
        assert eng.install_features(rows, *pieces)["stride"] == 32
        _same(want, _followups(eng, T, 2))
    eng.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def _raw(eng, ptr, dtype, ld, table, image_of, B, F=1, frames=None, Q=None):
    """gitmi_generate_prefixed with GITMI_SEARCH_FEATURES, unchecked by the wrapper -> the message of the refusal"""
    from generativeimage2text_amd.engine import GitmiSearch, SEARCH_FEATURES
    s = GitmiSearch()
    s.kind, s.reserved_ = SEARCH_FEATURES, dtype
    n = len(table)
    tab = (C.c_int32 * (3 * max(n, 1)))(*[v for p in table for v in p])
    img = None if image_of is None else (C.c_int32 * max(n, 1))(*image_of)
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    rc = eng.lib.gitmi_generate_prefixed(eng._h, frames, F, B, ptr, ld, tab, img, n if Q is None else Q, C.byref(s), None, None, None,
                                         info.data_ptr(), None)
    assert rc != 0 and info.tolist() == [-7] * 4
    return eng.lib.gitmi_last_error().decode()


def test_refusals_come_before_any_launch_and_leave_the_resident_images():
    from generativeimage2text_amd.engine import GitmiError, SEARCH_FEATURES
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=81, tie_output=False, successor=2.0, eos_bias=1.0)
    frames = [f.cuda() for f in O.make_images(cfg, 2, 1, seed=82)]
    T = 12
    eng = _engine(cfg, w, "f16", 2, beams=1, T=T, F=2)                  # cap = 34 rows per image, Q <= 4
    eng.generate(frames, _search("greedy", T))
    want = [t.cpu() for t in eng.generate(None, _search("greedy", T))]
    rows = torch.randn(40, cfg.vit_width, device="cuda")
    p, ok = rows.data_ptr(), [(0, 17, -1), (17, 17, -1)]
    held = (C.c_void_p * 1)(frames[0].data_ptr())
    cases = [
        (dict(ptr=p, dtype=0, ld=40, table=ok, image_of=None, B=2, frames=held), "frames != NULL"),
        (dict(ptr=p + 4, dtype=0, ld=40, table=ok, image_of=None, B=2), "not 16-byte aligned"),
        (dict(ptr=p, dtype=1, ld=40, table=ok, image_of=None, B=2), r"element type 1.*GITMI_DTYPE_F16 \(2\)"),
        (dict(ptr=p, dtype=7, ld=40, table=ok, image_of=None, B=2), "element type 7"),
        (dict(ptr=p, dtype=0, ld=40, table=[(0, 17, -1), (24, 17, -1)], image_of=None, B=2), r"piece 1 reads rows \[24,41\) of a buffer of 40"),
        (dict(ptr=p, dtype=0, ld=40, table=[(0, 17, -1), (-1, 17, -1)], image_of=None, B=2), "piece 1 reads rows"),
        (dict(ptr=p, dtype=0, ld=40, table=[(0, 0, -1), (17, 17, -1)], image_of=None, B=2), "piece 0 has 0 rows"),
        (dict(ptr=p, dtype=0, ld=40, table=[(0, 20, -1), (20, 15, -1), (0, 17, -1)], image_of=[0, 0, 1], B=2),
         "image 0 asks for 35 rows, the workspaces hold 34"),
        (dict(ptr=p, dtype=0, ld=40, table=ok, image_of=[0, 0], B=2), "image 1 has no piece"),
        (dict(ptr=p, dtype=0, ld=40, table=ok, image_of=[0, 2], B=2), "piece 1 names image 2 of 2"),
        (dict(ptr=p, dtype=0, ld=40, table=[(0, 17, 0), (17, 17, -1)], image_of=None, B=2), "piece 0 has temporal index 0, but the model has no"),
        (dict(ptr=p, dtype=0, ld=40, table=ok, image_of=None, B=2, F=3), r"F=3 outside \[1,2\]"),
        (dict(ptr=p, dtype=0, ld=40, table=ok, image_of=None, B=3), r"B=3 outside \[1,2\]"),
        (dict(ptr=p, dtype=0, ld=40, table=ok, image_of=None, B=2, Q=0), r"Q=0 pieces outside \[1,4\]"),
        (dict(ptr=p, dtype=0, ld=40, table=ok, image_of=None, B=2, Q=5), r"Q=5 pieces outside \[1,4\]"),
        (dict(ptr=p, dtype=0, ld=40, table=ok[:1], image_of=None, B=2), "without image_of, Q must equal B"),
        (dict(ptr=None, dtype=0, ld=40, table=ok, image_of=None, B=2), "null argument"),
    ]
    import re
    for kw, match in cases:
        msg = _raw(eng, **kw)
        assert msg.startswith("features: ") and re.search(match, msg), (match, msg)
        got = [t.cpu() for t in eng.generate(None, _search("greedy", T))]      # the images of before are still resident
        _same(want, got)
    # the wrapper's own refusal leaves them too
    with pytest.raises(ValueError, match="piece 1: rows"):
        eng.install_features(rows, [(0, 17), (30, 17)])
    assert eng.resident == 2
    # kind 9 is not a search
    s = _search("greedy", T)
    s.kind = SEARCH_FEATURES
    with pytest.raises(GitmiError, match="generate: GITMI_SEARCH_FEATURES installs given feature rows"):
        eng.generate(None, s)
    with pytest.raises(GitmiError, match="GITMI_SEARCH_FEATURES is not a search"):
        eng.search_begin(s, torch.full((2, 1), cfg.sos, dtype=torch.long), cfg.vocab)
    _same(want, [t.cpu() for t in eng.generate(None, _search("greedy", T))])
    eng.close()
    # an fp32 engine takes fp32 rows only; a video model checks t and F against num_frames
    vcfg = O.CONFIGS["TINY_VIDEO"]
    vw = O.make_weights(vcfg, seed=19, tie_output=False, successor=2.0)
    veng = _engine(vcfg, vw, "f32", 2, beams=1, T=T, F=4)
    assert re.search(r"element type 2.*GITMI_DTYPE_F32 \(0\) only", _raw(veng, p, 2, 40, ok, None, 2))
    assert "piece 1 has temporal index 3 outside [0,3)" in _raw(veng, p, 0, 40, [(0, 17, 2), (17, 17, 3)], None, 2)
    assert "piece 0 has temporal index -2" in _raw(veng, p, 0, 40, [(0, 17, -2), (17, 17, 0)], None, 2)
    assert "F=4 above the 3 frames of the model" in _raw(veng, p, 0, 40, ok, None, 2, F=4)
    assert veng.resident is None
    veng.install_features(rows, [(0, 17, 2), (17, 17, None)], None, F=3)      # and the valid forms of the same go through
    assert veng.resident == 2
    veng.close()


# ---- 7. FeatureStore ---------------------------------------------------------------------------------------------------------------
def _model(cfg, w, precision, B, T=12, **kw):
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=T, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision=precision, max_batch=B, **kw)
    model.load_state_dict(w)
    return model


@pytest.mark.parametrize("dtype", ["f32", "op"])
def test_feature_store_put_recall_eviction_and_handles(dtype):
    from generativeimage2text_amd.model import FeatureStore, StaleImagesError
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=81, tie_output=False, successor=2.0, eos_bias=1.0)
    images = O.make_images(cfg, 3, 1, seed=82)[0].cuda()
    model = _model(cfg, w, "f16", 3, max_frames=2)
    store = FeatureStore(model, 3, dtype=torch.float32 if dtype == "f32" else torch.float16)
    assert store.tensor.shape == (3, 17, cfg.vit_width) and store.bytes_per_image == 17 * cfg.vit_width * (4 if dtype == "f32" else 2)
    first = model.submit({"image": images})
    first.result()
    qs = [[cfg.sos], [cfg.sos, 7], [cfg.sos, 300, 2]]

    def ask(on, image_of):
        return model.submit_followup({"prefixes": qs, "image_of": image_of}, on=on).result()

    want = ask(first, [2, 0, 2])
    store.put(images, ["a", "b", "c"])                                  # its own encoder pass over the same batch
    with pytest.raises(StaleImagesError):
        ask(first, [2, 0, 2])                                           # that pass replaced the images of `first`
    model.submit({"image": torch.flip(images, dims=(-1,))}).result()
    h = store.recall([["c"], ["a"], ["c"]])                             # a repeat, mixed order
    assert h.result() == {"stride": 17, "max_rows": 17, "total_rows": 51}
    got = ask(h, [0, 1, 2])
    assert got["predictions"] == want["predictions"] and torch.equal(_bits(got["logprobs"]), _bits(want["logprobs"]))
    assert store.keys() == ["b", "a", "c"]
    store.put(images[1:2] * 0.5, ["d"])                                 # full: b, the least recently used, makes room
    assert "b" not in store and len(store) == 3
    with pytest.raises(StaleImagesError):
        ask(h, [0, 1, 2])                                               # put encoded on h's context
    with pytest.raises(KeyError, match="never put, or evicted"):
        store.recall([["b"]])
    two = store.recall([["a", "c"]])                                    # two keys concatenated: one image of 2 x 17 rows
    assert two.result() == {"stride": 34, "max_rows": 34, "total_rows": 34} and two.engine.resident == 1
    assert len(model.submit_followup({"prefixes": [[cfg.sos]], "image_of": [0]}, on=two).result()["predictions"]) == 1
    model.close()


def test_feature_store_recall_is_bound_to_the_recalling_context_of_a_pipeline():
    from generativeimage2text_amd.model import FeatureStore, StaleImagesError
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=81, tie_output=False, successor=2.0, eos_bias=1.0)
    images = O.make_images(cfg, 2, 1, seed=82)[0].cuda()
    model = _model(cfg, w, "f16", 2)
    first = model.submit({"image": images})
    first.result()
    want = model.submit_followup({"prefixes": [[cfg.sos]] * 2, "image_of": [1, 0]}, on=first).result()
    model.set_pipeline(2)
    store = FeatureStore(model, 2)
    store.put(images, ["x", "y"])
    ctxs = list(model._ctxs)
    h = store.recall([["y"], ["x"]], context=ctxs[1])
    assert h.engine is ctxs[1] and ctxs[1].resident == 2
    got = model.submit_followup({"prefixes": [[cfg.sos]] * 2, "image_of": [0, 1]}, on=h).result()
    assert got["predictions"] == want["predictions"] and torch.equal(_bits(got["logprobs"]), _bits(want["logprobs"]))
    h2 = store.recall([["x"]])                                          # the rotation picks a context itself
    assert h2.engine in ctxs
    if h2.engine is ctxs[1]:
        with pytest.raises(StaleImagesError):
            model.submit_followup({"prefixes": [[cfg.sos]], "image_of": [0]}, on=h)
    assert len(model.submit_followup({"prefixes": [[cfg.sos]], "image_of": [0]}, on=h2).result()["predictions"]) == 1
    model.close()


# ---- 8. attend ---------------------------------------------------------------------------------------------------------------------
def test_attend_over_installed_features():
    cfg = O.CONFIGS["TINY"]
    w = O.make_weights(cfg, seed=81, tie_output=False, successor=2.0, eos_bias=1.0)
    images = O.make_images(cfg, 3, 1, seed=82)[0].cuda()
    model = _model(cfg, w, "f16", 3, max_context=16)
    caps = [c[:n].tolist() for c, n in zip(CAPS, CAP_LENS)]
    want = model.attend(images, caps)
    feats = model.features(images)
    h = model.submit_features(feats)
    got = model.attend(None, caps, on=h)
    assert torch.equal(_bits(got.image), _bits(want.image)) and torch.equal(_bits(got.text), _bits(want.text))
    assert torch.equal(got.patch_grid(2), want.patch_grid(2)) and got.patch_grid(0).shape == (5, cfg.dec_layers, 1, 4, 4)
    # a key-count batch: 17 and 20 rows; the maps are over the stride's columns, every row of a caption sums to 1, no grid
    rows = feats.reshape(-1, cfg.vit_width)
    h = model.submit_features(rows, [(0, 17), (17, 20)], [0, 1])
    assert h.result() == {"stride": 32, "max_rows": 20, "total_rows": 37}
    maps = model.attend(None, caps[:2], on=h)
    assert maps.image.shape[-1] == 32
    for q, n in enumerate(CAP_LENS[:2]):
        total = maps.image[q, :n].sum(-1) + maps.text[q, :n].sum(-1)
        assert torch.allclose(total, torch.ones_like(total), atol=1e-3), total
        assert float(maps.image[q, :n, :, (17, 20)[q]:].abs().max()) == 0.0          # columns past the image's own rows
    with pytest.raises(ValueError, match="came without a shape"):
        maps.patch_grid(0)
    model.close()


# ---- the fp32 features of an encode at production width ---------------------------------------------------------------------------
@pytest.mark.parametrize("operands", ["f16", "bf16"])
@pytest.mark.parametrize("D", [768, 1024, 128])
def test_the_fp32_copy_of_ln_post_rounds_to_its_operand_copy(experiment_build, operands, D):
    """What makes the round trip exact in the 16-bit modes: the fp32 features gitmi_encode_frames hands back, rounded to nearest
    even, are the operand rows the encoder stored.  At D = 768 / 1024 those rows come from the wide LayerNorm kernel, whose
    partial sums run in another order than the one-wave-per-row kernel's: the fp32 copy must come from the same kernel."""
    from generativeimage2text_amd import engine as E
    g = torch.Generator().manual_seed(D)
    rows, N, F = 2 * 19, 19, 2
    x = (torch.randn(rows, D, generator=g) * 3).to(torch.float16).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    temb = torch.randn(D, generator=g).cuda()
    op = OPERAND[operands]
    for add in (None, temb):
        wide = torch.zeros(2 * F * N, D, device="cuda")
        half = torch.zeros(2 * F * N, D, dtype=op, device="cuda")
        E.op_layernorm_map(x, gamma, beta, 1e-5, add, wide, None, rows, D, N, F * N, N, operands=operands)
        E.op_layernorm_map(x, gamma, beta, 1e-5, add, half, None, rows, D, N, F * N, N, operands=operands)
        assert float(wide.abs().max()) > 0 and torch.equal(wide.to(op).view(torch.int16), half.view(torch.int16))
