"""Follow-up calls on resident images (include/gitmi.h: frames == NULL): a search or a score pass over the images the engine
already holds, without the image encoder and the prefill.  A follow-up must return exactly what the full call with the same
sentences returns (bit for bit, every precision, graphs on and off), the reference's ids for new questions (f32: equal;
16-bit: tools/parity.py's rules, as tests/test_gpu_parity.py and tests/test_gpu_ragged_golden.py apply them), and every
residency rule must fail with a return code and a message, never with a fault."""
import ast
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_case, load_golden
from oracle import git_oracle as O

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16", "bf16")
GRAPHS = (True, False)


def _engine(cfg, w, precision, B, beams=1, T=20, F=1, hw=None, graph=True):
    from generativeimage2text_amd.engine import Engine
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=beams, max_frames=F, max_text_len=T, max_image_hw=hw)
    eng.load_state_dict(w)
    eng.set_graph(graph)
    return eng


def _search(kind, T, k=1, pn=1, lp=0.6, **kw):
    from generativeimage2text_amd.engine import Engine
    return Engine.make_search(kind, T, k, pn, lp, **kw)


def _cpu(out):
    return tuple(t.cpu() for t in out)


def _same(a, b):
    """two results of generate / generate_prefixed: every tensor bit for bit (NaN log-probs compare as equal bits)"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), (x, y)


def _tiny(seed=81, B=3, img_seed=82, **kw):
    cfg = O.CONFIGS["TINY"]
    kw = dict(dict(tie_output=False, successor=2.0, eos_bias=1.0), **kw)
    return cfg, O.make_weights(cfg, seed=seed, **kw), [f.cuda() for f in O.make_images(cfg, B, 1, seed=img_seed)]


def _fixture(name):
    g, cfg, w, frames, search, prefix = golden_case(name)
    hw = tuple(frames[0].shape[2:])
    return g, cfg, w, [f.cuda() for f in frames], search, prefix, (hw if hw != (cfg.image_size, cfg.image_size) else None)


# ---- 1. the same sentences ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", ["tiny_prefix_greedy", "tiny_prefix_beam4", "tiny_video_greedy"])
def test_followup_with_the_same_sentences_is_bit_identical(name, precision, graph):
    """full call, then the same sentences with frames == NULL: tokens, log-probs, sent_out and info_out bit for bit, through
    gitmi_generate and through gitmi_generate_prefixed.  (On the parent commit the follow-up fails with "null argument".)"""
    g, cfg, w, frames, search, prefix, hw = _fixture(name)
    B, F = frames[0].shape[0], len(frames)
    eng = _engine(cfg, w, precision, B, search.beam_size, search.max_steps, F, hw, graph)
    s = _search(search.kind, search.max_steps, search.beam_size, search.per_node_beam_size, search.length_penalty)
    assert eng.resident is None
    full = _cpu(eng.generate(frames, s, prefix=prefix))
    assert eng.resident == B
    for _ in range(2):                                                  # the second one replays the follow-up graph
        _same(full, _cpu(eng.generate(None, s, prefix=prefix)))
    p = [cfg.sos] if prefix is None else prefix.reshape(-1).tolist()
    full_p = _cpu(eng.generate_prefixed(frames, s, [p] * B))
    _same(full_p, _cpu(eng.generate_prefixed(None, s, [p] * B)))
    assert torch.equal(full_p[0], full[0])                              # and both entry points agree on the ids
    eng.close()


# ---- 2. new questions against the reference -----------------------------------------------------------------------------------
def _check_ids(precision, got, ref_p, step_margin, g, kind, k):
    """f32: the reference's ids; 16-bit: tools/parity.py's rules exactly as tests/test_gpu_parity.py check_bf16 applies them"""
    if precision == "f32":
        assert np.array_equal(got, ref_p), (got, ref_p)
        return
    from tools.parity import ids_parity, logit_bound, margin_threshold
    ref = g["tf_logits"]
    lbound = logit_bound(precision, float(ref.max() - ref.min()))
    chained = not (kind == "greedy" and k == 1)
    ids_parity(got, ref_p, step_margin, margin_threshold(precision, lbound, chained), chained, first_decision_pos=0)


# vqa_base_480x640 (GIT_BASE_VQAv2 at real width) runs once: the fp16 build with graphs on, the path that is served
NEW_QUESTION_CASES = [(n, p, gr) for n in ("tiny_prefix_greedy", "tiny_prefix_beam4") for p in PRECS for gr in GRAPHS] + \
                     [("vqa_base_480x640", "f16", True)]


@pytest.mark.parametrize("name,precision,graph", NEW_QUESTION_CASES)
def test_followup_with_a_new_question_matches_the_reference(name, precision, graph):
    """These fixtures hold ONE question about one image, so there is no second half to keep back: the full call asks another
    question (the fixture's cut to its first two tokens), the follow-up then asks the fixture's question, which must come
    back as the reference answered it.  (tests below split ragged_tiny's five questions into true halves.)"""
    g, cfg, w, frames, search, prefix, hw = _fixture(name)
    kind, T, k, pn, lpen = ast.literal_eval(str(g["search"]))
    eng = _engine(cfg, w, precision, 1, k, T, 1, hw, graph)
    s = _search(kind, T, k, pn, lpen)
    p = prefix.reshape(-1).tolist()
    eng.generate_prefixed(frames, s, [p[:2]])
    tok, _, sent, info = _cpu(eng.generate_prefixed(None, s, [p], image_of=[0]))
    assert int(info[3]) == 0
    ref_p = g["predictions"]
    P, width = len(p), ref_p.shape[1]
    if kind == "greedy" and int(sent[0, 1]):
        got = tok[:, P:P + 1].numpy()
    else:
        got = tok[:, P:P + width].numpy()
    _check_ids(precision, got, ref_p, g["step_margin"], g, kind, k)
    eng.close()


def _ragged_case():
    g = load_golden("ragged_tiny")
    cfg = O.CONFIGS[str(g["config"])]
    w = O.make_weights(cfg, **ast.literal_eval(str(g["weights_kw"])))
    gen = torch.Generator().manual_seed(int(g["image_seed"]))
    images = [torch.randn(3, int(h), int(ww), generator=gen).cuda() for h, ww in g["shapes"]]
    T = int(ast.literal_eval(str(g["search"]))[1])
    return g, cfg, w, images, T


def _ragged_engine(cfg, w, precision, g, T, graph):
    return _engine(cfg, w, precision, len(g["lengths"]), 1, T, 1, tuple(int(v) for v in g["hw"]), graph)


def _check_ragged_rows(precision, g, rows, tok, sent):
    """rows of ragged_tiny against the reference, as tests/test_gpu_ragged_golden.py judges them"""
    from tools.parity import tf_bounds
    lens, plen = g["lengths"], g["prefix_len"]
    thr = tf_bounds(precision, float(g["logit_max"]) - float(g["logit_min"]))["thr"]
    for i, q in enumerate(rows):
        got, ref = tok[i, :int(sent[i, 0])].tolist(), g["ids"][q, :lens[q]].tolist()
        if precision == "f32":
            assert got == ref, (q, got, ref)
            continue
        diff = [j for j in range(min(len(got), len(ref))) if got[j] != ref[j]]
        if not diff:
            assert len(got) == len(ref) or g["dec_margin"][q].min() < thr, (q, got, ref)
            continue
        j = diff[0]
        assert j >= plen[q] and g["dec_margin"][q, :j].min() < thr, \
            f"row {q}: ids leave the reference at {j} although every earlier decision margin >= {thr:.4f}"


# ---- 6. ragged input (and the true halves of test 2) ----------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_ragged_followup_halves_match_reference_and_full_call(precision, graph):
    """ragged_tiny: a full ragged call with the first half of the questions, a follow-up with the other half (about the
    images encoded by the first): the reference's ids; and a follow-up with every question equals the full call bit for bit."""
    from generativeimage2text_amd.engine import Engine
    g, cfg, w, images, T = _ragged_case()
    eng = _ragged_engine(cfg, w, precision, g, T, graph)
    s = _search("greedy", T)
    plen, image_of = g["prefix_len"], [int(i) for i in g["image_of"]]
    prefixes = [g["ids"][q, :plen[q]].tolist() for q in range(len(plen))]
    Q = len(prefixes)
    first, second = list(range(0, Q // 2)), list(range(Q // 2, Q))
    packed = eng.ragged(images)
    eng.generate_prefixed(packed, s, [prefixes[q] for q in first], image_of=[image_of[q] for q in first])
    assert eng.resident == len(images)
    tok, _, sent, info = _cpu(eng.generate_prefixed(None, s, [prefixes[q] for q in second], image_of=[image_of[q] for q in second]))
    assert int(info[3]) == 0
    _check_ragged_rows(precision, g, second, tok, sent)
    full = _cpu(eng.generate_prefixed(packed, s, prefixes, image_of=image_of))
    _same(full, _cpu(eng.generate_prefixed(None, s, prefixes, image_of=image_of)))
    eng.close()


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_ragged_followup_keeps_rejected_entries(precision, graph):
    """a descriptor entry the device rejected (image 1: an offset inside the descriptor block) stays rejected in the follow-up:
    its sentences come back NaN and are counted in info[3]; the other images are unaffected"""
    g, cfg, w, images, T = _ragged_case()
    eng = _ragged_engine(cfg, w, precision, g, T, graph)
    s = _search("greedy", T)
    packed = eng.ragged(images[:3])
    desc = packed.buffer[:12].view(torch.int32)
    desc[1 * 4 + 2] = 4                                                 # offset of image 1 inside the descriptor block
    qs, image_of = [[cfg.sos, 5], [cfg.sos, 6, 7], [cfg.sos], [cfg.sos, 8]], [0, 1, 2, 1]
    full = _cpu(eng.generate_prefixed(packed, s, qs, image_of=image_of, sync=False))
    torch.cuda.synchronize()
    fu = _cpu(eng.generate_prefixed(None, s, qs, image_of=image_of, sync=False))
    torch.cuda.synchronize()
    _same(full, fu)
    lp, info = fu[1], fu[3]
    assert int(info[3]) == 2 and torch.isnan(lp[[1, 3]]).all() and torch.isfinite(lp[[0, 2]]).all()
    good = eng.ragged(images[:3])                                       # the unaffected images equal a clean call's
    clean = _cpu(eng.generate_prefixed(good, s, qs, image_of=image_of))
    for q in (0, 2):
        assert torch.equal(fu[0][q], clean[0][q]) and fu[1][q].item() == clean[1][q].item()
    eng.close()


# ---- 3. changing the search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_followup_with_another_search_equals_its_full_call(precision, graph):
    cfg, w, frames = _tiny()
    T = 16
    eng = _engine(cfg, w, precision, 3, 4, T, graph=graph)
    greedy = _search("greedy", T)
    others = [_search("beam", T, 4, 2, 0.6), _search("beam", T, 4, 2, 0.6, num_keep_best=3),
              _search("beam", T, 2, 2, 1.0, do_sample=True, top_k=20, top_p=0.9, temperature=0.8, seed=1234)]
    want = [_cpu(eng.generate(frames, s)) for s in others]
    eng.generate(frames, greedy)
    for s, ref in zip(others, want):
        _same(ref, _cpu(eng.generate(None, s)))
    assert want[1][0].shape == (3, 3, T)
    eng.close()


# ---- 4. changing the kind ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_generate_then_score_followup_and_back(precision, graph):
    from tools.parity import logit_bound
    g, cfg, w, frames, _, _, hw = _fixture("score_tiny_tied")
    ref_tokens = torch.as_tensor(g["tokens"])
    Q, L = ref_tokens.shape
    B = int(g["batch"])
    eng = _engine(cfg, w, precision, B, max(1, -(-Q // B)), L, 1, hw, graph)
    s = _search("greedy", L)
    gen_full = _cpu(eng.generate(frames, s))
    ids = gen_full[0]
    fu = eng.score(None, ids).cpu()                                     # the captions just generated, over their images
    # ... and the reference's sentences over the same resident images, within the bound of tests/test_gpu_score.py
    out = eng.score(None, ref_tokens, lengths=g["lengths"].tolist(), image_of=g["image_of"].tolist()).cpu().double()
    bound = 2.0 * logit_bound(precision, float(g["logit_max"]) - float(g["logit_min"]))
    assert (out[..., 0] - torch.as_tensor(g["lp"])).abs().max().item() <= bound
    assert (out[..., 1] - torch.as_tensor(g["mean_lp"])).abs().max().item() <= bound
    full = eng.score(frames, ids).cpu()
    assert torch.equal(fu.view(torch.int32), full.view(torch.int32))
    # score, then a generate follow-up
    _same(gen_full, _cpu(eng.generate(None, s)))
    eng.close()


# ---- 5. image_of ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_followup_image_of_subset_permutation_repetition(precision, graph):
    """5 sentences over images 2, 0, 2, 0, 2 of a 3-image batch (a subset, out of order, repeated, Q != B): every sentence
    equals its own single-image full call -- ids up to its end; log-prob within 1e-4 in f32 (the f32 mode's bound) and within
    twice tools/parity.py's logit bound in 16-bit (TINY's logits span < 8), as the ragged batch-independence tests have it"""
    from tools.parity import F32_LOGIT_ABS, logit_bound
    cfg, w, frames = _tiny(seed=83, img_seed=84)
    T = 14
    eng = _engine(cfg, w, precision, 5, 1, T, graph=graph)
    s = _search("greedy", T)
    qs = [[cfg.sos, 7, 44], [cfg.sos], [cfg.sos, 300, 2, 9, 512], [cfg.sos, 5], [cfg.sos, 7, 44, 13, 8, 2]]
    image_of = [2, 0, 2, 0, 2]
    eng.generate(frames, s)
    tok, lp, sent, info = _cpu(eng.generate_prefixed(None, s, qs, image_of=image_of))
    tol = F32_LOGIT_ABS if precision == "f32" else 2.0 * logit_bound(precision, 8.0)
    for q, (p, im) in enumerate(zip(qs, image_of)):
        t1, l1, s1, _ = _cpu(eng.generate_prefixed([frames[0][im:im + 1]], s, [p]))
        assert sent[q].tolist() == s1[0].tolist(), q
        n = int(s1[0, 0])
        assert tok[q, :n].tolist() == t1[0, :n].tolist(), (q, precision)
        assert abs(lp[q].item() - l1[0].item()) <= tol, (q, lp[q].item(), l1[0].item())
    eng.close()


# ---- 7. video --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_video_followup_with_new_prefixes_equals_full_call(precision, graph):
    g, cfg, w, frames, search, _, hw = _fixture("tiny_video_greedy")
    B, F, T = frames[0].shape[0], len(frames), search.max_steps
    eng = _engine(cfg, w, precision, 4, 1, T, F, hw, graph)
    s = _search("greedy", T)
    qs, image_of = [[cfg.sos, 9], [cfg.sos, 10, 11], [cfg.sos], [cfg.sos, 12]], [1, 0, 1, 1]
    want = _cpu(eng.generate_prefixed(frames, s, qs, image_of=image_of))
    eng.generate(frames, s)
    _same(want, _cpu(eng.generate_prefixed(None, s, qs, image_of=image_of)))
    eng.close()


# ---- 8. residency rules ------------------------------------------------------------------------------------------------------------
class _Raw:
    """gitmi_generate through ctypes: return code and message, no exception"""

    def __init__(self, eng, T):
        from generativeimage2text_amd.engine import _stream
        self.eng, self.T, self._stream = eng, T, _stream
        self.tok = torch.empty(eng.c.max_batch, T, dtype=torch.int64, device="cuda")
        self.lp = torch.empty(eng.c.max_batch, device="cuda")
        self.info = torch.empty(4, dtype=torch.int32, device="cuda")

    def __call__(self, frames, B, max_steps=None):
        s = _search("greedy", self.T if max_steps is None else max_steps)
        arr = None if frames is None else (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
        rc = self.eng.lib.gitmi_generate(self.eng._h, arr, 1, B, None, 1, C.byref(s), self.tok.data_ptr(), self.lp.data_ptr(),
                                         self.info.data_ptr(), self._stream())
        torch.cuda.synchronize()
        return rc, (self.eng.lib.gitmi_last_error() or b"").decode()

    def result(self, B):
        return self.tok[:B].cpu().clone(), self.lp[:B].cpu().clone(), self.info.cpu().clone()


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_residency_rules(precision, graph):
    cfg = O.CONFIGS["TINY_VIDEO"]                  # a model with temporal embeddings, so that the switch means something
    w = O.make_weights(cfg, seed=85, tie_output=False, successor=2.0)
    frames = [f.cuda() for f in O.make_images(cfg, 2, 1, seed=86)]
    small = [f[:, :, :48, :64].contiguous() for f in frames]
    T = 10
    eng = _engine(cfg, w, precision, 2, 1, T, 1, (64, 64), graph)
    raw = _Raw(eng, T)
    rc, msg = raw(None, 2)                                              # a fresh engine
    assert rc != 0 and "no resident images" in msg
    assert raw(frames, 2)[0] == 0
    want = raw.result(2)
    rc, msg = raw(None, 1)                                              # B mismatch: both numbers are named
    assert rc != 0 and "B=1" in msg and "2 images" in msg
    assert raw(None, 2)[0] == 0
    _same(want, raw.result(2))
    # an argument error found before any launch, in a follow-up and in a full call, leaves the images resident
    rc, msg = raw(None, 2, max_steps=T + 1)
    assert rc != 0 and "max_steps" in msg
    rc, msg = raw(frames, 2, max_steps=T + 1)
    assert rc != 0 and "max_steps" in msg
    assert raw(None, 2)[0] == 0
    _same(want, raw.result(2))
    # another shape
    eng._ck(eng.lib.gitmi_set_image_shape(eng._h, 48, 64, None))
    rc, msg = raw(None, 2)
    assert rc != 0 and "no resident images" in msg
    assert raw(small, 2)[0] == 0 and raw(None, 2)[0] == 0
    # ragged mode on, and off again
    eng._ck(eng.lib.gitmi_set_image_shape(eng._h, 0, 0, None))
    assert raw(None, 2)[0] != 0
    eng._ck(eng.lib.gitmi_set_image_shape(eng._h, 64, 64, None))
    assert raw(None, 2)[0] != 0
    assert raw(frames, 2)[0] == 0 and raw(None, 2)[0] == 0
    _same(want, raw.result(2))
    # the temporal-embedding switch: a flip drops the images, setting it to what it is does not
    eng._ck(eng.lib.gitmi_set_temporal_embedding(eng._h, 1))
    assert raw(None, 2)[0] == 0
    eng._ck(eng.lib.gitmi_set_temporal_embedding(eng._h, 0))
    rc, msg = raw(None, 2)
    assert rc != 0 and "no resident images" in msg
    eng._ck(eng.lib.gitmi_set_temporal_embedding(eng._h, 1))
    assert raw(None, 2)[0] != 0
    # gitmi_encode_frames alone makes images resident: the follow-up runs the prefill itself
    eng.encode(frames, return_features=False)
    assert eng.resident == 2
    assert raw(None, 2)[0] == 0
    _same(want, raw.result(2))
    assert raw(frames, 2)[0] == 0                                       # and the engine is as usable as before
    _same(want, raw.result(2))
    eng.close()


def test_python_mirror_of_the_residency_rules():
    """Engine.resident follows the library: set by calls that encode, kept through an argument error found before any launch
    (the library is asked), dropped by the setters; generation counts every change"""
    from generativeimage2text_amd.engine import GitmiError
    cfg, w, frames = _tiny()
    T = 10
    eng = _engine(cfg, w, "f32", 3, 1, T)
    s = _search("greedy", T)
    with pytest.raises(GitmiError, match="no resident images"):
        eng.generate(None, s)
    want = _cpu(eng.generate(frames, s))
    g0 = eng.generation
    with pytest.raises(GitmiError, match="max_steps"):
        eng.generate(frames, _search("greedy", T + 5))
    assert eng.resident == 3 and eng.generation > g0
    _same(want, _cpu(eng.generate(None, s)))
    with pytest.raises(GitmiError, match="beam_size"):                   # found after the encode started: the images are gone
        eng.set_graph(False)
        eng.generate(frames, _search("greedy", T, 3, 1))
    assert eng.resident is None
    with pytest.raises(GitmiError, match="no resident images"):
        eng.generate(None, s)
    eng.generate(frames, s)
    eng.set_temporal_embedding(True)
    assert eng.resident == 3
    eng.set_temporal_embedding(False)
    assert eng.resident is None
    eng.close()


# ---- 9. interleaving with graphs on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_interleaved_full_and_followup_calls_replay_their_own_graphs(precision):
    """full(A), follow-up(A), full(B), follow-up(B), full(A), follow-up(A) at constant shapes: with graphs on, every result
    equals its eager counterpart, and a follow-up after full(B) answers about B's images, not A's"""
    cfg, w, fa = _tiny(seed=87, img_seed=88)
    fb = [f.cuda() for f in O.make_images(cfg, 3, 1, seed=89)]
    T = 12
    eng = _engine(cfg, w, precision, 4, 1, T)
    s = _search("greedy", T)
    qs, image_of = [[cfg.sos, 21], [cfg.sos, 22, 23], [cfg.sos], [cfg.sos, 24]], [2, 0, 1, 2]

    def sequence():
        out = []
        for fr in (fa, fb, fa):
            out.append(_cpu(eng.generate(fr, s)))
            out.append(_cpu(eng.generate_prefixed(None, s, qs, image_of=image_of)))
        return out

    eng.set_graph(False)
    eager = sequence()
    eng.set_graph(True)
    graphed = sequence()
    for a, b in zip(eager, graphed):
        _same(a, b)
    assert not torch.equal(eager[1][0], eager[3][0])                    # A's and B's answers differ for these seeds ...
    _same(eager[1], eager[5])                                           # ... and A's come back after A is encoded again
    on_b = _cpu(eng.generate_prefixed(fb, s, qs, image_of=image_of))
    _same(on_b, graphed[3])
    eng.close()


# ---- profiling -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (1, 2))
def test_followup_profile_has_no_encoder_time(mode):
    cfg, w, frames = _tiny()
    T = 10
    eng = _engine(cfg, w, "f16", 3, 1, T)
    s = _search("greedy", T)
    want = _cpu(eng.generate(frames, s))
    eng.profile_enable(mode)
    _same(want, _cpu(eng.generate(None, s)))
    p = eng.profile_read()
    eng.profile_enable(0)
    assert p["vit_ms"] == 0 and p["prefill_ms"] == 0 and p["vit_gemm_launches"] == 0 and p["vit_gemm_ms"] == 0
    assert p["decode_ms"] > 0 and p["decode_steps"] == T - 1
    eng.close()


# ---- 10. contexts ----------------------------------------------------------------------------------------------------------------------
def test_clone_starts_without_resident_images():
    cfg, w, frames = _tiny()
    T = 10
    eng = _engine(cfg, w, "f32", 3, 1, T)
    s = _search("greedy", T)
    want = _cpu(eng.generate(frames, s))
    other = eng.clone()
    assert other.resident is None and eng.resident == 3
    rc, msg = _Raw(other, T)(None, 3)
    assert rc != 0 and "no resident images" in msg
    _same(want, _cpu(other.generate(frames, s)))
    _same(want, _cpu(other.generate(None, s)))
    _same(want, _cpu(eng.generate(None, s)))
    other.close()
    eng.close()


def test_pipeline_followup_reaches_the_context_of_its_handle():
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel, StaleImagesError
    cfg, w, fa = _tiny(seed=90, img_seed=91)
    fb = O.make_images(cfg, 3, 1, seed=92)[0].cuda()
    fa = fa[0]
    dec = AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=12, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    model = CaptioningModel(cfg, dec, precision="f32", max_batch=4)
    model.load_state_dict(w)
    qs, image_of = [[cfg.sos, 31], [cfg.sos, 32, 33], [cfg.sos, 34]], [2, 0, 2]
    want_a = model.submit_answers(fa, qs, image_of).result()
    want_b = model.submit_answers(fb, qs, image_of).result()
    assert want_a != want_b
    model.set_pipeline(2)
    pa = model.submit({"image": fa})
    pb = model.submit({"image": fb})
    assert pa.engine is not pb.engine
    got_b = model.submit_answers(None, qs, image_of).result()            # without on=: the most recent call's context
    got_a = model.submit_answers(None, qs, image_of, on=pa).result()
    assert list(got_a) == list(want_a) and list(got_b) == list(want_b)
    res_b = pb.result()
    out = model({"prefixes": qs, "image_of": image_of}, on=res_b)        # the result object is a handle too
    assert out["predictions"] == list(want_b)
    caps = [[cfg.sos, 5, 6, cfg.eos]] * 3
    sc = model.score(None, caps, image_of=[0, 1, 2], on=pa)
    pc = model.submit({"image": fb})                                     # rotates back to pa's context: its images are replaced
    assert pc.engine is pa.engine
    with pytest.raises(StaleImagesError):
        model.submit_answers(None, qs, image_of, on=pa)
    pc.result()
    assert torch.equal(sc["logprobs"], model.score(fa, caps)["logprobs"])
    model.close()
