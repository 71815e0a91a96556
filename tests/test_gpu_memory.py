"""Image memory snapshots (include/gitmi.h: GITMI_SEARCH_KEEP / GITMI_SEARCH_RECALL): the encoded memory of resident images is
copied into a caller-owned store and any mix of kept images is recalled later, into any context of the model.  A recalled
batch in its original order must give a follow-up bit for bit what it gave before (every precision, graphs on and off), a
mix from different calls what each image alone gives (the oracle's ids; f32: the engine's own batch-1 call bit for bit), and
every refusal must be a return code and a message found on the host before any launch, never a fault."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_case
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
    """two results of generate / generate_prefixed: every tensor bit for bit"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), (x, y)


def _tiny(seed=81, B=3, img_seed=82, hw=None, **kw):
    cfg = O.CONFIGS["TINY"]
    kw = dict(dict(tie_output=False, successor=2.0, eos_bias=1.0), **kw)
    return cfg, O.make_weights(cfg, seed=seed, **kw), [f.cuda() for f in O.make_images(cfg, B, 1, seed=img_seed, hw=hw)]


def _fixture(name):
    g, cfg, w, frames, search, prefix = golden_case(name)
    hw = tuple(frames[0].shape[2:])
    return g, cfg, w, [f.cuda() for f in frames], search, prefix, (hw if hw != (cfg.image_size, cfg.image_size) else None)


# ---- 1. the same batch in the same order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", ["tiny_prefix_greedy", "tiny_prefix_beam4", "tiny_video_greedy"])
def test_recall_in_the_original_order_restores_the_followup_bit_for_bit(name, precision, graph):
    """full call, follow-up (recorded), KEEP, an unrelated full call over other images, RECALL in the original order, the same
    follow-up: tokens, log-probs, sent_out and info_out bit for bit, through gitmi_generate and gitmi_generate_prefixed.
    tiny_video_greedy has F = 2 frames in one slot.  (On the parent commit the KEEP fails with "search: bad kind".)"""
    g, cfg, w, frames, search, prefix, hw = _fixture(name)
    B, F = frames[0].shape[0], len(frames)
    eng = _engine(cfg, w, precision, B, search.beam_size, search.max_steps, F, hw, graph)
    s = _search(search.kind, search.max_steps, search.beam_size, search.per_node_beam_size, search.length_penalty)
    p = [cfg.sos] if prefix is None else prefix.reshape(-1).tolist()
    eng.generate(frames, s, prefix=prefix)
    want = _cpu(eng.generate(None, s, prefix=prefix))
    want_p = _cpu(eng.generate_prefixed(None, s, [p] * B))
    geo = eng.resident_geometry
    store = eng.memory_store(B)
    kept = eng.keep(store, list(range(B)))
    assert kept["rows"] == [geo[0]] * B and kept["max_rows"] == geo[0] and kept["total_rows"] == B * geo[0]
    _same(want, _cpu(eng.generate(None, s, prefix=prefix)))             # KEEP changes nothing about residency
    others = [torch.roll(f, 1, dims=-1) * 0.5 + 0.25 for f in frames]
    other = _cpu(eng.generate(others, s, prefix=prefix))
    assert not torch.equal(other[0], want[0]) or not torch.equal(other[1], want[1])
    gen = eng.generation
    info = eng.recall(store, list(range(B)), kept["geometry"])
    assert info == {"stride": geo[0], "max_rows": geo[0], "total_rows": B * geo[0]}       # the uniform batch: no key counts
    assert eng.resident == B and eng.generation > gen and tuple(eng.resident_geometry) == tuple(geo)
    for _ in range(2):                                                  # the second one replays the follow-up graph
        _same(want, _cpu(eng.generate(None, s, prefix=prefix)))
    _same(want_p, _cpu(eng.generate_prefixed(None, s, [p] * B)))
    eng.close()


@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_score_and_tree_score_over_a_recalled_batch(precision):
    cfg, w, frames = _tiny()
    T = 12
    eng = _engine(cfg, w, precision, 3, 1, T)
    caps = torch.tensor([[cfg.sos, 5, 6, 7, cfg.eos, 0], [cfg.sos, 9, 10, cfg.eos, 0, 0], [cfg.sos, 300, 2, 9, 512, cfg.eos]])
    lens = [5, 4, 6]
    tree_tok = torch.tensor([[cfg.sos, 5, 6, 7, 9, cfg.eos]] * 3)
    tree_dep = torch.tensor([[0, 1, 2, 2, 1, 2]] * 3)
    eng.generate(frames, _search("greedy", T))
    want = eng.score(None, caps, lengths=lens).cpu()
    want_t = eng.score_tree(None, tree_tok, tree_dep).cpu()
    store = eng.memory_store(3)
    kept = eng.keep(store, [2, 0, 1])
    eng.generate([torch.flip(f, dims=(-1,)) for f in frames], _search("greedy", T))
    eng.recall(store, [2, 0, 1], kept["geometry"])
    assert torch.equal(eng.score(None, caps, lengths=lens).cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(eng.score_tree(None, tree_tok, tree_dep).cpu().view(torch.int32), want_t.view(torch.int32))
    att = eng.attend(None, caps, lengths=lens).cpu()                    # and ATTEND runs over it too: rows sum to 1
    assert torch.allclose(att[0, :5].sum(-1), torch.ones(5, cfg.dec_layers), atol=1e-3)
    eng.close()


# ---- 2 / 3. mixes: the oracle per image ---------------------------------------------------------------------------------------
def _oracle_greedy(cfg, w, image, prefix, T):
    """the reference's greedy call over one image: (ids with the prefix removed, log-prob, the margin of every decision, the span
    of the logits it saw)"""
    with torch.no_grad():
        feats = O.visual_features(cfg, w, [image.cpu()])
        inner = O.make_step(cfg, w, feats, cached=True)
        lo, hi = [], []

        def step(rows):
            z = inner(rows)
            lo.append(float(z.min())), hi.append(float(z.max()))
            return z

        tr = []
        preds, lps = O.search_autoregressive(torch.tensor([prefix]), step, cfg.eos, T, 1, 1, trace=tr)
    margins = torch.stack(tr, 1)[0].numpy() if tr else np.zeros(0)
    return preds[0, len(prefix):].tolist(), float(lps.flatten()[0]), margins, max(hi) - min(lo)


def _answer(tok, sent, q, P):
    L, early = int(sent[q, 0]), int(sent[q, 1])
    return (tok[q, P:P + 1] if early else tok[q, :L])[P:].tolist()


def _check_against_oracle(precision, cfg, w, image, prefix, T, got, got_lp):
    """f32: the reference's ids and its log-prob within the f32 bound of tests/test_gpu_parity.py (1e-4); 16-bit: tools/parity.py's
    rules as tests/test_gpu_followup.py applies them -- equal up to the first decision whose fp32 margin is below the threshold"""
    from tools.parity import ids_parity, logit_bound, margin_threshold
    ref, ref_lp, margins, span = _oracle_greedy(cfg, w, image, prefix, T)
    if precision == "f32":
        assert got == ref, (got, ref)
        assert abs(got_lp - ref_lp) <= 1e-4, (got_lp, ref_lp)
        return
    thr = margin_threshold(precision, logit_bound(precision, span), False)
    L = max(len(got), len(ref))
    pad = lambda r: np.array([r + [-1] * (L - len(r))])
    ids_parity(pad(got), pad(ref), margins[None, :], thr, False, first_decision_pos=0)


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_recall_of_a_mix_from_two_calls_with_a_repeat(precision, graph):
    """call A (3 images) and call B (2 images) are kept; [A2, B0, A0, A2] is recalled: every sentence returns what the oracle
    returns for its image alone and, in f32, what the engine's own batch-1 call returns, bit for bit"""
    cfg, w, fa = _tiny(seed=93, img_seed=94)
    fb = [f.cuda() for f in O.make_images(cfg, 2, 1, seed=95)]
    T = 14
    eng = _engine(cfg, w, precision, 4, 1, T, graph=graph)
    s = _search("greedy", T)
    store = eng.memory_store(5)
    eng.generate(fa, s)
    ka = eng.keep(store, [0, 1, 2])
    eng.generate(fb, s)
    kb = eng.keep(store, [4, 3], images=[1, 0])                         # B0 -> slot 3, B1 -> slot 4
    mix = [(fa[0][2:3], 2, ka["geometry"][2]), (fb[0][0:1], 3, kb["geometry"][1]), (fa[0][0:1], 0, ka["geometry"][0]),
           (fa[0][2:3], 2, ka["geometry"][2])]
    info = eng.recall(store, [m[1] for m in mix], [m[2] for m in mix])
    assert info == {"stride": 17, "max_rows": 17, "total_rows": 68} and eng.resident == 4
    qs = [[cfg.sos, 7, 44], [cfg.sos], [cfg.sos, 300, 2, 9, 512], [cfg.sos, 5]]
    tok, lp, sent, inf = _cpu(eng.generate_prefixed(None, s, qs))
    assert int(inf[3]) == 0
    for q, (p, (image, _, _)) in enumerate(zip(qs, mix)):
        _check_against_oracle(precision, cfg, w, image, p, T, _answer(tok, sent, q, len(p)), float(lp[q]))
    if precision == "f32":
        for q, (p, (image, _, _)) in enumerate(zip(qs, mix)):
            t1, l1, s1, _ = _cpu(eng.generate_prefixed([image], s, [p]))
            n = int(s1[0, 0])
            assert sent[q].tolist() == s1[0].tolist() and tok[q, :n].tolist() == t1[0, :n].tolist()
            assert lp[q].view(torch.int32).item() == l1[0].view(torch.int32).item(), (q, lp[q].item(), l1[0].item())
    eng.close()


@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_recall_of_different_key_counts_in_one_batch(precision, graph):
    """Key-count mode: a plain 64 x 128 image (n = 33, just above a 32-key tile of kv_repack_frag), a 64 x 96 image kept after a
    context call with segments of 1 and 5 tokens (n = 25 + 6 = 31, just below it) and a 48 x 64 image kept by a SECOND engine in
    ragged mode (n = 13), whose blob travels through host memory.  None of the three is a multiple of 16.  The plain and the
    ragged image are held to the oracle as in the mix test; every image to the engine's own call over it alone: bit for bit in
    f32, ids to its end and the log-prob within twice tools/parity.py's logit bound in 16-bit (TINY's logits span < 8), as
    tests/test_gpu_followup.py holds a batch to its single-image calls."""
    from tools.parity import logit_bound
    cfg, w, _ = _tiny(seed=96, B=1)
    hw = (64, 128)
    plain = O.make_images(cfg, 1, 1, seed=97, hw=(64, 128))[0].cuda()
    ctx_im = O.make_images(cfg, 1, 1, seed=98, hw=(64, 96))[0].cuda()
    rag_im = O.make_images(cfg, 1, 1, seed=99, hw=(48, 64))[0].cuda()
    segs = [[11, 12, 13, 14, 15], [21]]
    T = 14
    eng = _engine(cfg, w, precision, 3, 1, T, hw=hw, graph=graph)
    other = _engine(cfg, w, precision, 3, 1, T, hw=hw, graph=graph)
    s = _search("greedy", T)
    qs = [[cfg.sos, 7], [cfg.sos, 300, 2], [cfg.sos]]
    store, far = eng.memory_store(3), other.memory_store(1)
    # every image alone: its own call, and its blob
    own = []
    own.append(_cpu(eng.generate_prefixed([plain], s, [qs[0]])))
    g0 = eng.keep(store, [0])["geometry"]
    eng.encode_context([ctx_im], segs, image_of=[0, 0])
    own.append(_cpu(eng.generate_prefixed(None, s, [qs[1]])))
    kept = eng.keep(store, [1])
    assert kept["rows"] == [31]
    g1 = kept["geometry"]
    own.append(_cpu(other.generate_prefixed(other.ragged([rag_im[0]]), s, [qs[2]])))
    kept = other.keep(far, [0])
    assert kept["rows"] == [13]
    g2 = kept["geometry"]
    store[2].copy_(far[0].cpu().clone().cuda())                          # the blob is plain bytes: through the host
    info = eng.recall(store, [0, 1, 2], g0 + g1 + g2)
    assert info == {"stride": 33, "max_rows": 33, "total_rows": 77}      # 48 rows would exceed the 33 the workspaces hold
    geo = eng.resident_geometry
    assert geo.stride == 33 and geo.context == [0, 6, 0] and geo[2] == [(4, 8), (4, 6), (3, 4)]
    tok, lp, sent, inf = _cpu(eng.generate_prefixed(None, s, qs))
    assert int(inf[3]) == 0
    tol = 0.0 if precision == "f32" else 2.0 * logit_bound(precision, 8.0)
    for q in range(3):
        t1, l1, s1, _ = own[q]
        n = int(s1[0, 0])
        print(f"{precision} image {q}: lp {lp[q].item():.6f} own call {l1[0].item():.6f}")
        assert sent[q].tolist() == s1[0].tolist() and tok[q, :n].tolist() == t1[0, :n].tolist(), (q, tok[q], t1[0])
        assert abs(lp[q].item() - l1[0].item()) <= tol, (q, lp[q].item(), l1[0].item())
    for q, image in ((0, plain), (2, rag_im)):
        _check_against_oracle(precision, cfg, w, image, qs[q], T, _answer(tok, sent, q, len(qs[q])), float(lp[q]))
    from generativeimage2text_amd.engine import GitmiError
    with pytest.raises(GitmiError, match="context rows"):               # ATTEND keeps its refusal over context rows
        eng.attend(None, torch.tensor([[cfg.sos, 5]] * 3))
    other.close()
    eng.close()


# ---- 4. across contexts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
@pytest.mark.parametrize("precision", PRECS)
def test_keep_on_an_engine_recall_on_its_clone(precision, graph):
    cfg, w, frames = _tiny(seed=100, img_seed=101)
    T = 12
    eng = _engine(cfg, w, precision, 3, 4, T, graph=graph)
    s, beam = _search("greedy", T), _search("beam", T, 4, 2, 0.6)
    qs, image_of = [[cfg.sos, 21], [cfg.sos, 22, 23], [cfg.sos], [cfg.sos, 24]][:3], [2, 0, 1]
    eng.generate(frames, s)
    want = _cpu(eng.generate_prefixed(None, s, qs, image_of=image_of))
    want_beam = _cpu(eng.generate(None, beam))
    store = eng.memory_store(3)
    kept = eng.keep(store, [0, 1, 2])
    clone = eng.clone()
    clone.set_graph(graph)
    assert clone.resident is None
    clone.recall(store, [0, 1, 2], kept["geometry"])
    assert clone.resident == 3 and eng.resident == 3
    _same(want, _cpu(clone.generate_prefixed(None, s, qs, image_of=image_of)))
    _same(want_beam, _cpu(clone.generate(None, beam)))
    _same(want, _cpu(eng.generate_prefixed(None, s, qs, image_of=image_of)))     # the source is unaffected
    clone.close()
    eng.close()


# ---- 5. extremes -----------------------------------------------------------------------------------------------------------------
def test_size_query_and_the_slot_size_formula():
    from generativeimage2text_amd.engine import GitmiSearch, SEARCH_KEEP, _stream
    cfg, w, _ = _tiny(B=1)
    for precision, esz in (("f32", 4), ("f16", 2), ("bf16", 2)):
        eng = _engine(cfg, w, precision, 2, 1, 10, F=2, hw=(64, 96))
        rows = 2 * (4 * 6 + 1)                                          # max_frames x max_image_tokens
        want = -(-(256 + rows * (cfg.vit_width + cfg.dec_layers * 2 * cfg.dec_hidden) * esz) // 256) * 256
        assert eng.memory_slot_bytes() == want and eng.memory_rows == rows
        search = GitmiSearch()
        search.kind = SEARCH_KEEP
        info = torch.zeros(4, dtype=torch.int32, device="cuda")
        rc = eng.lib.gitmi_generate_prefixed(eng._h, None, 0, 0, None, 0, None, None, 0, C.byref(search), None, None, None,
                                             info.data_ptr(), _stream())
        assert rc == 0 and info.tolist() == [want // 256, 0, 0, 0]
        assert eng.clone().memory_slot_bytes() == want
        eng.close()


@pytest.mark.parametrize("precision", PRECS)
def test_extremes_one_image_a_full_batch_one_slot_subsets_and_overwrites(precision):
    cfg, w, frames = _tiny(seed=102, B=6, img_seed=103)
    T = 10
    eng = _engine(cfg, w, precision, 6, 1, T)
    s = _search("greedy", T)
    full = _cpu(eng.generate(frames, s))                                # B = max_batch
    store = eng.memory_store(6)
    kept = eng.keep(store, list(range(6)))
    eng.generate([frames[0][:1] * 0.5], s)
    eng.recall(store, list(range(6)), kept["geometry"])
    _same(full, _cpu(eng.generate(None, s)))
    # B = 1 out of a store of one slot
    one = eng.memory_store(1)
    k1 = eng.keep(one, [0], images=[4])
    eng.recall(one, [0], k1["geometry"])
    assert eng.resident == 1
    t1, l1, _ = _cpu(eng.generate(None, s))
    assert torch.equal(t1[0], full[0][4]) and (precision != "f32" or l1[0].item() == full[1][4].item())
    # a subset in permuted slot order, then a slot overwritten and recalled
    eng.generate(frames, s)
    sub = eng.memory_store(3)
    ks = eng.keep(sub, [2, 0, 1], images=[5, 1, 3])                     # slot 0 = image 1, slot 1 = image 3, slot 2 = image 5
    eng.recall(sub, [0, 1, 2], [ks["geometry"][1], ks["geometry"][2], ks["geometry"][0]])
    t3, _, _ = _cpu(eng.generate(None, s))
    assert [t3[i].tolist() for i in range(3)] == [full[0][i].tolist() for i in (1, 3, 5)]
    eng.generate(frames, s)
    ko = eng.keep(sub, [1], images=[0])                                 # slot 1 now holds image 0
    eng.recall(sub, [1, 1], ko["geometry"] * 2)
    t2, _, _ = _cpu(eng.generate(None, s))
    assert t2[0].tolist() == full[0][0].tolist() == t2[1].tolist()
    eng.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
class _Raw:
    """KEEP / RECALL through ctypes: return code and message, no exception"""

    def __init__(self, eng):
        from generativeimage2text_amd.engine import _stream
        self.eng, self._stream = eng, _stream
        self.info = torch.zeros(4, dtype=torch.int32, device="cuda")

    def __call__(self, kind, B, store_ptr, S, slots, images=None, frames=None, Q=None):
        from generativeimage2text_amd.engine import GitmiSearch
        search = GitmiSearch()
        search.kind = kind
        Q = len(slots) if Q is None else Q
        sl = (C.c_int32 * max(1, len(slots)))(*slots)
        im = None if images is None else (C.c_int32 * len(images))(*images)
        arr = None if frames is None else (C.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
        keep, recall = (store_ptr, None) if kind == 7 else (None, store_ptr)
        rc = self.eng.lib.gitmi_generate_prefixed(self.eng._h, arr, 1, B, recall, S, sl, im, Q, C.byref(search), None, keep, None,
                                                  self.info.data_ptr(), self._stream())
        torch.cuda.synchronize()
        return rc, (self.eng.lib.gitmi_last_error() or b"").decode()


@pytest.mark.parametrize("precision", PRECS)
def test_refusals_are_messages_and_leave_the_resident_set(precision):
    from generativeimage2text_amd.engine import GitmiSearch, _stream
    cfg, w, frames = _tiny(seed=104, img_seed=105)
    T = 10
    KEEP, RECALL = 7, 8
    eng = _engine(cfg, w, precision, 3, 1, T, F=2)
    raw = _Raw(eng)
    s = _search("greedy", T)
    store = eng.memory_store(4)
    store.zero_()
    base, S = store.data_ptr(), 4
    rc, msg = raw(KEEP, 0, base, S, [0])                                # KEEP without resident images
    assert rc != 0 and "no resident images" in msg
    eng.generate(frames, s)
    want = _cpu(eng.generate(None, s))
    kept = eng.keep(store, [0, 1], images=[0, 1])

    def still():
        assert torch.cuda.is_available() and eng.resident == 3
        _same(want, _cpu(eng.generate(None, s)))

    nbytes = eng.memory_slot_bytes()
    hdr = lambda slot: store[slot, :64].view(torch.int32)
    for what, call, words in [
        ("a zeroed slot", lambda: raw(RECALL, 1, base, S, [3]), ("slot 3", "magic")),
        ("a slot index >= ld", lambda: raw(RECALL, 1, base, S, [4]), ("slot 4", "4 slots")),
        ("a slot index >= ld in KEEP", lambda: raw(KEEP, 3, base, S, [0, 1, 4]), ("slot 4", "4 slots")),
        ("a duplicate destination", lambda: raw(KEEP, 3, base, S, [2, 3, 2]), ("both write slot 2",)),
        ("Q > max_batch", lambda: raw(RECALL, 4, base, S, [0, 1, 0, 1]), ("Q=4", "max_batch")),
        ("Q > max_batch in KEEP", lambda: raw(KEEP, 3, base, S, [0, 1, 2, 3], images=[0, 1, 2, 0]), ("Q=4", "max_batch")),
        ("frames != NULL", lambda: raw(RECALL, 1, base, S, [0], frames=frames), ("frames != NULL",)),
        ("frames != NULL in KEEP", lambda: raw(KEEP, 3, base, S, [0, 1, 2], frames=frames), ("frames != NULL",)),
        ("a misaligned base", lambda: raw(RECALL, 1, base + 16, S - 1, [0]), ("256-byte aligned",)),
        ("a misaligned base in KEEP", lambda: raw(KEEP, 3, base + 128, S - 1, [0, 1, 2]), ("256-byte aligned",)),
        ("image_of in RECALL", lambda: raw(RECALL, 1, base, S, [0], images=[0]), ("image_of_host must be NULL",)),
        ("B != Q", lambda: raw(RECALL, 2, base, S, [0]), ("B=2", "Q=1")),
        ("B != resident", lambda: raw(KEEP, 2, base, S, [0, 1]), ("B=2", "3 images")),
    ]:
        rc, msg = call()
        assert rc != 0 and all(wd in msg for wd in words), (what, msg)
        still()
    # n overwritten with capacity + 1 on a host copy of the header
    saved = store[0].clone()
    h = hdr(0).cpu()
    assert h[9].item() == 17 and h[12].item() == 1
    h[9] = eng.memory_rows + 1
    hdr(0).copy_(h)
    rc, msg = raw(RECALL, 1, base, S, [0])
    assert rc != 0 and "slot 0" in msg and f"n={eng.memory_rows + 1}" in msg and "capacity" in msg
    still()
    # slots with different F
    store[0].copy_(saved)
    h = hdr(0).cpu()
    h[12] = 2
    hdr(0).copy_(h)
    rc, msg = raw(RECALL, 2, base, S, [1, 0])
    assert rc != 0 and "slot 0" in msg and "F=2" in msg and "F=1" in msg
    still()
    store[0].copy_(saved)
    assert raw(RECALL, 2, base, S, [1, 0])[0] == 0                      # and the restored bytes are good again
    eng.generate(frames, s)
    # a blob kept by an engine of another precision: the fingerprint
    other_prec = "f32" if precision != "f32" else "f16"
    other = _engine(cfg, w, other_prec, 3, 1, T, F=2)
    if other.memory_slot_bytes() == nbytes:
        foreign = store
    else:
        foreign = other.memory_store(4)
    other.generate(frames, s)
    other.keep(foreign, [2], images=[0])
    if foreign is not store:
        store[2, :256].copy_(foreign[2, :256])                          # the header decides: it is what is validated
    rc, msg = raw(RECALL, 1, base, S, [2])
    assert rc != 0 and "slot 2" in msg and "fingerprint" in msg and "element" in msg
    still()
    other.close()
    # gitmi_generate and gitmi_search_begin refuse both kinds by name
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    start = (C.c_int64 * 3)(cfg.sos, cfg.sos, cfg.sos)
    for kind, name in ((KEEP, "GITMI_SEARCH_KEEP"), (RECALL, "GITMI_SEARCH_RECALL")):
        search = GitmiSearch()
        search.kind, search.max_steps, search.beam_size, search.per_node_beam_size = kind, T, 1, 1
        rc = eng.lib.gitmi_generate(eng._h, None, 1, 3, None, 1, C.byref(search), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), _stream())
        assert rc != 0 and name in eng.lib.gitmi_last_error().decode()
        rc = eng.lib.gitmi_search_begin(eng._h, C.byref(search), 3, start, 1, cfg.vocab, _stream())
        assert rc != 0 and name in eng.lib.gitmi_last_error().decode()
    still()
    eng.close()


@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_a_kept_rejected_ragged_entry_is_refused_at_recall(precision):
    from generativeimage2text_amd.engine import GitmiError
    cfg, w, _ = _tiny(B=1)
    gen = torch.Generator().manual_seed(5)
    images = [torch.randn(3, 48, 64, generator=gen).cuda(), torch.randn(3, 64, 48, generator=gen).cuda()]
    T = 10
    eng = _engine(cfg, w, precision, 2, 1, T, hw=(64, 64))
    s = _search("greedy", T)
    packed = eng.ragged(images)
    packed.buffer[:8].view(torch.int32)[1 * 4 + 2] = 4                  # offset of image 1 inside the descriptor block
    qs = [[cfg.sos, 5], [cfg.sos, 6]]
    want = _cpu(eng.generate_prefixed(packed, s, qs, sync=False))
    torch.cuda.synchronize()
    assert int(want[3][3]) == 1
    store = eng.memory_store(2)
    kept = eng.keep(store, [0, 1])
    assert kept["max_rows"] == 13 and kept["total_rows"] == 14           # the rejected entry keeps its class token only
    assert store[1, :64].view(torch.int32)[15].item() == 1
    with pytest.raises(GitmiError, match=r"slot 1.*rejected"):
        eng.recall(store, [0, 1])
    assert eng.resident == 2
    _same(want, _cpu(eng.generate_prefixed(None, s, qs, sync=False)))
    info = eng.recall(store, [0, 0])                                    # the good entry comes back, in ragged mode, twice
    assert info == {"stride": 16, "max_rows": 13, "total_rows": 26}
    tok, lp, sent, inf = _cpu(eng.generate_prefixed(None, s, [qs[0], qs[0]]))
    assert int(inf[3]) == 0 and torch.equal(tok[0], tok[1])
    assert precision != "f32" or torch.equal(tok[0], want[0][0])
    eng.close()
