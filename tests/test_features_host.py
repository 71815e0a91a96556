"""Features in, host side (no GPU): the header defines GITMI_SEARCH_FEATURES = 9 under ABI 10 with its argument mapping and
without a new export, engine.feature_pieces builds the piece table and rejects every malformed one by naming the piece,
Engine.install_features mirrors the resident set, and FeatureStore's keys, LRU eviction, windows and handles work against a
stub engine."""
import os
import re
import types

import pytest
import torch

from generativeimage2text_amd import engine
from generativeimage2text_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gitmi.h")).read()


def test_header_defines_kind_9_under_abi_10():
    hdr = _header()
    assert re.search(r"#define\s+GITMI_SEARCH_FEATURES\s+9\b", hdr) and engine.SEARCH_FEATURES == 9
    assert re.search(r"#define\s+GITMI_ABI_VERSION\s+10\b", hdr)
    assert len(engine.EXPORTED_SYMBOLS) == 40
    assert sorted(set(re.findall(r"\b(gitmi_[a-z_0-9]+)\s*\(", hdr))) == sorted(engine.EXPORTED_SYMBOLS)


def test_header_documents_the_argument_mapping():
    hdr = _header()
    doc = hdr[hdr.index("features in: search->kind == GITMI_SEARCH_FEATURES"):]
    doc = doc[:doc.index("int  gitmi_generate_prefixed(")]
    text = " ".join(doc.replace("*", " ").split())
    for phrase in ("frames : must be NULL", "B : the images to form, 1 .. max_batch", "<= num_frames where that is > 0",
                   "prefixes : the base address (read as bytes)", "16-byte aligned", "keeps no pointer to it",
                   "search->reserved_ : the element type of the rows", "refused by name", "ld_prefix : the rows the buffer holds",
                   "Q : the pieces, 1 .. max_batch x max_frames", "every image needs at least one piece",
                   "prefix_len_host : int32 [Q][3] = { first source row, rows (>= 1), temporal index t or -1 }",
                   "independent of gitmi_set_temporal_embedding",
                   "info_out : { row stride of an image's block, max_b n_b, sum_b n_b, 0 }", "cap = max_frames x max(N, max_image_tokens)",
                   "names the rows asked for and the capacity", "vit_width % 8 != 0 is refused", "WITHOUT key counts", "key-count batch",
                   "zeros in rows [n_b, stride)", "{ 0, 0, n_b, 0 }", "bit for bit in every precision",
                   "neither waits for nor signals the gitmi_set_encode_after chain", "features of another model of the same width go unnoticed",
                   "info_out[3] of the calls that follow", "refuse it by name", "keep their footprint"):
        assert phrase in text, phrase


# ---- engine.feature_pieces -----------------------------------------------------------------------------------------------------------
CAPS = dict(max_batch=4, max_frames=3, cap=51, num_frames=3)


def test_feature_pieces_accepts_and_lays_out():
    # one piece per image, no image_of
    assert engine.feature_pieces([(0, 17), (17, 17, None)], None, 34, **CAPS) == ([[0, 17, -1], [17, 17, -1]], None, [17, 17])
    # counts 17 / 18 / 32 / 33 with image 1 in two pieces (5 + 13) interleaved with image 2
    tab, img, counts = engine.feature_pieces([(0, 17), (17, 5), (22, 32), (54, 13), (67, 33)], [0, 1, 2, 1, 3], 100, **CAPS)
    assert counts == [17, 18, 32, 33] and img == [0, 1, 2, 1, 3] and tab[3] == [54, 13, -1]
    # a window of three frames with their temporal indices, the same rows used twice, F = 3
    tab, img, counts = engine.feature_pieces([(0, 17, 0), (17, 17, 1), (34, 17, 2), (17, 17, 0)], [0, 0, 0, 1], 51, F=3, **CAPS)
    assert counts == [51, 17] and [p[2] for p in tab] == [0, 1, 2, 0]
    # exactly the capacity, the last row of the buffer, Q at its bound
    assert engine.feature_pieces([(2, 51)], None, 53, **CAPS)[2] == [51]
    assert len(engine.feature_pieces([(0, 1)] * 12, [0, 1, 2, 3] * 3, 1, **CAPS)[0]) == 12


@pytest.mark.parametrize("pieces, image_of, rows, kw, match", [
    ([(0, 17), (17, 0)], None, 34, {}, "piece 1: 0 rows"),
    ([(0, 17), (-1, 3)], None, 34, {}, r"piece 1: rows \[-1, 2\) of a buffer of 34 rows"),
    ([(0, 17), (30, 5)], None, 34, {}, r"piece 1: rows \[30, 35\) of a buffer of 34 rows"),
    ([(0, 17, 3)], None, 34, {}, r"piece 0: temporal index 3 outside \[0, 3\)"),
    ([(0, 17, -2)], None, 34, {}, "piece 0: temporal index -2"),
    ([(0, 17, 0)], None, 34, {"num_frames": 0}, "piece 0: temporal index 0, but the model has no temporal embeddings"),
    ([(0, 30), (30, 22)], [0, 0], 60, {}, "piece 1: image 0 asks for 52 rows, the engine holds 51 per image"),
    ([(0, 17), (17, 17)], [0, 2], 34, {}, "image 1 has no piece"),
    ([(0, 17), (17, 17)], [0, -1], 34, {}, "piece 1: image -1 is negative"),
    ([(0, 17), (17, 17)], [0], 34, {}, "image_of has 1 entries for 2 pieces"),
    ([(0, 1)] * 13, [0] * 13, 34, {}, r"13 pieces outside \[1, 12\]"),
    ([], None, 34, {}, r"0 pieces outside \[1, 12\]"),
    ([(0, 1)] * 5, None, 34, {}, "5 images exceed max_batch=4"),
    ([(0, 17)], None, 34, {"F": 4}, r"F=4 outside \[1, 3\]"),
    ([(0, 17)], None, 34, {"F": 0}, r"F=0 outside \[1, 3\]"),
    ([(0, 17)], None, 34, {"F": 3, "num_frames": 2}, r"F=3 outside \[1, 2\]"),
    ([(0,)], None, 34, {}, "piece 0: expected"),
])
def test_feature_pieces_rejects_by_naming_the_piece(pieces, image_of, rows, kw, match):
    with pytest.raises(ValueError, match=match):
        engine.feature_pieces(pieces, image_of, rows, **dict(CAPS, **kw))


# ---- Engine.install_features' bookkeeping --------------------------------------------------------------------------------------------
class _FakeLib:
    def __init__(self):
        self.err, self.fail, self.calls = b"", None, []

    def gitmi_last_error(self):
        return self.err

    def gitmi_generate_prefixed(self, h, frames, F, B, prefixes, ld, lens, image_of, Q, search, tok, lp, sent, info, stream):
        s = search._obj
        self.calls.append((s.kind, s.reserved_, frames, F, B, prefixes, ld, [lens[i] for i in range(3 * Q)],
                           None if image_of is None else [image_of[q] for q in range(Q)], Q))
        if self.fail == "early":
            self.err = b"features: piece 0 reads rows [0,17) of a buffer of 3 rows"
            return 1
        if self.fail == "late":
            self.err = b"engine.hip:1: launch_feature_install -> invalid argument"
            return 1
        self.out[:] = torch.tensor(self.info)
        return 0


def _engine_mirror(monkeypatch, precision="f16", num_frames=3):
    eng = object.__new__(engine.Engine)
    eng.lib, eng._h, eng.device, eng.precision = _FakeLib(), None, 0, precision
    eng.c = types.SimpleNamespace(vit_width=128, dec_hidden=128, dec_layers=2, max_frames=3, max_batch=4, image_size=64, patch=16,
                                  max_image_tokens=0, num_frames=num_frames)
    eng._hw, eng.n_tok = (64, 64), 17
    eng._init_resident()
    monkeypatch.setattr(engine, "_stream", lambda: 0)
    real_zeros, real_device = torch.zeros, torch.device

    def zeros(*a, **k):                                                 # info lives on the host here
        k.pop("device", None)
        eng.lib.out = real_zeros(*a, **k)
        return eng.lib.out

    monkeypatch.setattr(engine.torch, "zeros", zeros)
    monkeypatch.setattr(engine.torch, "device", lambda *_a, **_k: real_device("cpu"))     # the rows of this test live on the host
    return eng


def test_install_features_bookkeeping(monkeypatch):
    eng = _engine_mirror(monkeypatch)
    rows = torch.zeros(3, 17, 128)
    eng.lib.info = [17, 17, 51, 0]
    g0 = eng.generation
    assert eng.install_features(rows) == {"stride": 17, "max_rows": 17, "total_rows": 51}
    kind, dtype, frames, F, B, ptr, ld, tab, image_of, Q = eng.lib.calls[-1]
    assert (kind, dtype, frames, F, B, ld, image_of, Q) == (9, 0, None, 1, 3, 51, None, 3) and ptr == rows.data_ptr()
    assert tab == [0, 17, -1, 17, 17, -1, 34, 17, -1]
    assert eng.resident == 3 and eng.generation == g0 + 1
    assert eng.resident_geometry == (17, 1, [(4, 4)] * 3) and not isinstance(eng.resident_geometry, engine.Geometry)
    # 16-bit rows of the engine's operand type, a window of three frames and a single frame: a key-count batch without grids
    half = torch.zeros(51, 128, dtype=torch.float16)
    eng.lib.info = [64, 51, 68, 0]
    eng.install_features(half, [(0, 17, 0), (17, 17, 1), (34, 17, 2), (0, 17)], [0, 0, 0, 1], F=3)
    kind, dtype, frames, F, B, ptr, ld, tab, image_of, Q = eng.lib.calls[-1]
    assert (dtype, F, B, ld, image_of, Q) == (2, 3, 2, 51, [0, 0, 0, 1], 4) and tab[:3] == [0, 17, 0] and tab[-3:] == [0, 17, -1]
    geo = eng.resident_geometry
    assert isinstance(geo, engine.Geometry) and geo == (64, 3, [None, None]) and geo.context == [0, 0] and geo.rows == [51, 17]
    assert eng.generation == g0 + 2
    # the uniform video window: grids are known
    eng.lib.info = [51, 51, 51, 0]
    eng.install_features(half, [(0, 17, 0), (17, 17, 1), (34, 17, 2)], [0, 0, 0], F=3)
    assert eng.resident_geometry == (51, 3, [(4, 4)])
    # what the wrapper refuses itself
    with pytest.raises(ValueError, match=r"\[R, 128\] or \[B, n, 128\]"):
        eng.install_features(torch.zeros(3, 17, 64))
    with pytest.raises(ValueError, match="torch.float32 or torch.float16"):
        eng.install_features(torch.zeros(3, 17, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="need pieces"):
        eng.install_features(torch.zeros(51, 128))
    with pytest.raises(ValueError, match="imply the pieces"):
        eng.install_features(rows, [(0, 17)])
    with pytest.raises(ValueError, match="piece 0: rows"):
        eng.install_features(half, [(40, 17)])
    assert eng.resident == 1 and eng.generation == g0 + 3
    # an argument error of the library leaves the resident set, a failed launch drops it
    eng.lib.fail = "early"
    with pytest.raises(engine.GitmiError, match="features: piece 0"):
        eng.install_features(rows)
    assert eng.resident == 1 and eng.generation == g0 + 3
    eng.lib.fail = "late"
    with pytest.raises(engine.GitmiError, match="launch_feature_install"):
        eng.install_features(rows)
    assert eng.resident is None and eng.generation == g0 + 4


def test_an_f32_engine_takes_fp32_rows_only(monkeypatch):
    eng = _engine_mirror(monkeypatch, precision="f32")
    with pytest.raises(ValueError, match="torch.float32 on this engine"):
        eng.install_features(torch.zeros(1, 17, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="torch.float32 on this engine"):
        eng.feature_store(2, torch.bfloat16)


# ---- FeatureStore against a stub engine ----------------------------------------------------------------------------------------------
class _FakeEngine:
    """An engine context as FeatureStore and the front end see it: element [0, 0] of an image's rows is its tag, and the
    installed batch remembers, per image, the (tag, temporal index) of every piece"""

    def __init__(self, name):
        self.name, self.calls = name, []
        self.resident, self.generation, self.images = None, 0, []
        self.c = types.SimpleNamespace(max_batch=8, max_frames=3, vit_width=4)
        self.n_tok, self.device = 2, 0

    def set_temporal_embedding(self, on):
        self.calls.append(("temb", on))

    def check_finite(self, info):
        pass

    def feature_store(self, slots, dtype=torch.float32):
        return torch.zeros(slots, self.n_tok, 4, dtype=dtype)

    def encode(self, frames):
        self.calls.append(("encode", len(frames)))
        x = frames[0]
        self.images = [[(int(v), None)] for v in x[:, 0, 0, 0]]
        self.resident, self.generation = len(self.images), self.generation + 1
        feats = torch.zeros(x.shape[0], self.n_tok, 4)
        feats[:, 0, 0] = x[:, 0, 0, 0]
        return feats

    def install_features(self, rows, pieces=None, image_of=None, F=1):
        self.calls.append(("install", list(pieces), list(image_of), F))
        B = max(image_of) + 1
        self.images = [[] for _ in range(B)]
        for (src, n, t), b in zip(pieces, image_of):
            assert n == self.n_tok and src % self.n_tok == 0
            self.images[b].append((int(rows[src, 0]), t))
        self.resident, self.generation = B, self.generation + 1
        n = [self.n_tok * len(im) for im in self.images]
        return {"stride": max(n), "max_rows": max(n), "total_rows": sum(n)}

    def generate_prefixed(self, frames, search, prefixes, image_of=None, sync=True, host_out=False):
        self.calls.append(("generate_prefixed", frames is None))
        Q, T = len(prefixes), search.max_steps
        tok = torch.full((Q, T), 102)
        for q, p in enumerate(prefixes):
            tok[q, :len(p)] = torch.tensor(p)
            tok[q, len(p)] = 1000 + self.images[image_of[q]][0][0]           # the answer names the first frame of its image
        return tok, torch.zeros(Q), torch.tensor([[len(p) + 1, 0] for p in prefixes]), torch.tensor([T, 0, 0, 0])

    def score(self, frames, tokens, lengths=None, image_of=None):
        self.calls.append(("score", frames is None))
        return torch.zeros(tokens.shape[0], tokens.shape[1], 2)


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: types.SimpleNamespace(synchronize=lambda: None))


def _model(contexts=1, num_frames=0):
    m = object.__new__(M.CaptioningModel)
    m.cfg = types.SimpleNamespace(num_frames=num_frames, sos=101, eos=102, vocab=30522)
    m.decoder = M.AutoRegressiveBeamSearch(eos_index=102, max_steps=10, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    m.engine, m._loaded, m.training = _FakeEngine("ctx0"), True, False
    if contexts > 1:
        m._ctxs = [m.engine] + [_FakeEngine(f"ctx{i}") for i in range(1, contexts)]
        m._streams = [None] * contexts
        m._next = 0
    return m


def _frames(*tags):
    x = torch.zeros(len(tags), 3, 8, 8)
    x[:, 0, 0, 0] = torch.tensor(tags, dtype=torch.float32)
    return x


def test_feature_store_keys_lru_and_eviction(no_device):
    m = _model()
    store = M.FeatureStore(m, 3)
    assert len(store) == 0 and "a" not in store and store.tensor.shape == (3, 2, 4) and store.bytes_per_image == 32
    store.put(_frames(10, 11), ["a", "b"])
    assert m.engine.calls[:2] == [("temb", False), ("encode", 1)]         # a bare tensor: no temporal embedding in the stored rows
    assert store.keys() == ["a", "b"] and len(store) == 2
    store.put_features(m.features(_frames(12)), ["c"])                   # the store is full now
    store.recall([["a"]])                                               # a is the most recently used now
    assert store.keys() == ["b", "c", "a"]
    store.put(_frames(20), ["d"])                                       # b, the least recently used, makes room
    assert "b" not in store and store.keys() == ["c", "a", "d"]
    store.put(_frames(21), ["a"])                                       # a key that is held is overwritten in its slot
    assert store.keys() == ["c", "d", "a"] and len(store) == 3
    h = store.recall([["a"], ["c"], ["a"]])                             # repeats and mixed order
    assert m.engine.images == [[(21, None)], [(12, None)], [(21, None)]] and h.engine is m.engine
    assert h.result() == {"stride": 2, "max_rows": 2, "total_rows": 6}
    out = m.submit_followup({"prefixes": [[101, 5]] * 3, "image_of": [0, 1, 2]}, on=h).result()
    assert out["predictions"] == [[1021], [1012], [1021]]
    store.evict("c")
    with pytest.raises(KeyError, match="never put, or evicted"):
        store.recall([["a", "c"]])
    with pytest.raises(KeyError):
        store.evict("zzz")
    with pytest.raises(ValueError, match="exceed the 3 slots"):
        store.put(_frames(1, 2, 3, 4), ["p", "q", "r", "s"])
    with pytest.raises(ValueError, match="every key once"):
        store.put(_frames(1, 2), ["p", "p"])
    with pytest.raises(ValueError, match="2 keys for 1 frames"):
        store.put(_frames(1), ["p", "q"])
    with pytest.raises(ValueError, match=r"\[1, 2, 4\]"):
        store.put_features(torch.zeros(1, 3, 4), ["p"])
    with pytest.raises(ValueError, match="at least one key"):
        store.recall([["a"], []])
    with pytest.raises(ValueError):
        M.FeatureStore(m, 0)


def test_feature_store_windows_and_temporal_defaults(no_device):
    m = _model(num_frames=3)
    store = M.FeatureStore(m, 5)
    store.put(_frames(1, 2, 3, 4), ["f0", "f1", "f2", "f3"])
    # a video model: embedding i on the i-th key of a window of more than one key, none on a single key
    h = store.recall([["f0", "f1", "f2"], ["f1", "f2", "f3"], ["f3"]])
    assert m.engine.images == [[(1, 0), (2, 1), (3, 2)], [(2, 0), (3, 1), (4, 2)], [(4, None)]]
    assert m.engine.calls[-1][3] == 3 and h.result()["total_rows"] == 14
    pieces, image_of, F = store.pieces([["f2", "f0"]], temporal=[[None, 2]])
    slot = {k: s for k, s in store._entries.items()}
    assert pieces == [(slot["f2"] * 2, 2, None), (slot["f0"] * 2, 2, 2)] and image_of == [0, 0] and F == 2
    with pytest.raises(ValueError, match="one index"):
        store.pieces([["f2", "f0"]], temporal=[[0]])
    # a model without temporal embeddings concatenates without any
    m0 = _model()
    s0 = M.FeatureStore(m0, 2)
    s0.put(_frames(5, 6), ["x", "y"])
    s0.recall([["x", "y"]])
    assert m0.engine.images == [[(5, None), (6, None)]]


def test_recall_handles_go_stale_and_work_as_on(no_device):
    m = _model()
    store = M.FeatureStore(m, 4)
    store.put(_frames(1, 2, 3), ["x", "y", "z"])
    h = store.recall([["z"], ["x"]])
    assert m.submit_answers(None, [[101, 9]], image_of=[0], on=h).result() == [[1003]]
    assert m.submit_answers(None, [[101, 9]], image_of=[1], on=h.result()).result() == [[1001]]
    m.score(None, [[101, 5, 102]], image_of=[1], on=h)
    assert m.engine.calls[-1] == ("score", True)
    store.put(_frames(9), ["w"])                                        # another encode on the context: the handle is stale
    with pytest.raises(M.StaleImagesError, match="no longer resident"):
        m.submit_answers(None, [[101]], image_of=[0], on=h)
    h2 = store.recall([["y"]])
    assert m.submit_answers(None, [[101]], image_of=[0], on=h2).result() == [[1002]]


def test_pipelined_store_binds_the_handle_to_the_recalling_context(no_device):
    m = _model(contexts=3)
    store = M.FeatureStore(m, 4)
    feats = torch.zeros(3, 2, 4)
    feats[:, 0, 0] = torch.tensor([5.0, 6.0, 7.0])
    store.put_features(feats, ["a", "b", "c"])                          # rows from anywhere: no context is involved
    assert all(c.resident is None for c in m._ctxs)
    h = store.recall([["c"], ["a"]])                                    # the next context of the rotation: ctx0
    assert h.engine is m._ctxs[0] and m._ctxs[1].resident is None
    h1 = store.recall([["b"]])                                          # and the one after it
    assert h1.engine is m._ctxs[1] and h1.engine.images == [[(6, None)]]
    assert h.engine.images == [[(7, None)], [(5, None)]]
    assert m.submit_answers(None, [[101]] * 2, image_of=[0, 1], on=h).result() == [[1007], [1005]]
    h2 = store.recall([["b"]], context=m._ctxs[2])                      # on a context of the caller's choice
    assert h2.engine is m._ctxs[2] and m._ctxs[2].images == [[(6, None)]]
    assert m.submit_answers(None, [[101]], image_of=[0], on=h2).result() == [[1006]]
