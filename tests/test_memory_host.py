"""Image memory snapshots, host side (no GPU): the header documents GITMI_SEARCH_KEEP / GITMI_SEARCH_RECALL with their argument
mapping and without a new export, the slot-size formula, Engine.recall's bookkeeping of the resident set, and ImageStore's
keys, LRU eviction and handles against a stub engine."""
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


def test_no_new_export_and_same_abi():
    hdr = _header()
    assert len(engine.EXPORTED_SYMBOLS) == 40
    assert sorted(set(re.findall(r"\b(gitmi_[a-z_0-9]+)\s*\(", hdr))) == sorted(engine.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+GITMI_ABI_VERSION\s+10\b", hdr)
    assert re.search(r"#define\s+GITMI_SEARCH_KEEP\s+7\b", hdr) and re.search(r"#define\s+GITMI_SEARCH_RECALL\s+8\b", hdr)
    assert (engine.SEARCH_KEEP, engine.SEARCH_RECALL) == (7, 8)
    import ctypes as C
    assert C.sizeof(engine.GitmiConfig) == 84 and C.sizeof(engine.GitmiSearch) == 72


def test_header_documents_both_kinds_with_their_argument_mapping():
    hdr = _header()
    doc = hdr[hdr.index("image memory snapshots: search->kind == GITMI_SEARCH_KEEP"):]
    doc = doc[:doc.index("int  gitmi_generate_prefixed(")]
    text = " ".join(doc.replace("*", " ").split())
    keep, recall = text[text.index("KEEP, the argument mapping"):text.index("RECALL, the argument mapping")], \
        text[text.index("RECALL, the argument mapping"):]
    for phrase in ("frames : must be NULL", "logprob_out : the store's base address", "256-byte aligned", "ld_prefix: the slots it has",
                   "image_of_host : int32 [Q], the resident image", "prefix_len_host : int32 [Q], the destination slot",
                   "at most once per call", "Q == 0 is the size query", "info_out : { slot_bytes / 256, max_q n_q, sum_q n_q, 0 }",
                   "KEEP changes nothing about residency"):
        assert phrase in keep, phrase
    for phrase in ("frames : must be NULL", "B == Q", "image_of_host: must be NULL", "prefixes : the store's base address",
                   "prefix_len_host : int32 [Q], the slot that becomes image q; repeats are allowed",
                   "info_out : { row stride of an image's block, max_q n_q, sum_q n_q, 0 }", "BEFORE any launch", "names the slot and the field",
                   "what was resident stays resident", "WITHOUT key counts", "key-count batch", "GITMI_SEARCH_ATTEND keeps its refusal"):
        assert phrase in recall, phrase
    for phrase in ("The store is the CALLER's", "keeps no pointer to it", "slot_bytes = round_up(256 + cap x (vit_width + dec_layers x 2 x "
                   "dec_hidden) x esz, 256)", "fingerprint", "CANNOT tell whether the weights are the same", "refuse them by name"):
        assert phrase in text, phrase
    assert "int  gitmi_generate_prefixed(gitmi_engine* e, const float* const* frames, int F, int B," in hdr


def test_slot_size_formula():
    # GIT_BASE at 224 x 224, 16-bit: 197 rows x (768 + 6 x 1536) x 2 bytes behind the header: 3.9 MB
    n = engine.memory_slot_bytes(768, 768, 6, 197, 2)
    assert n == -(-(256 + 197 * (768 + 6 * 2 * 768) * 2) // 256) * 256 and n % 256 == 0 and 3.9e6 < n < 4.0e6
    assert engine.memory_slot_bytes(128, 128, 2, 17, 4) == 256 + 17 * (128 + 2 * 256) * 4 == 43776
    assert engine.memory_slot_bytes(128, 128, 2, 17, 2) == 22016 == -(-(256 + 17 * 640 * 2) // 256) * 256
    assert engine.memory_slot_bytes(64, 64, 1, 1, 2) == 768          # 256 + 384, rounded up
    eng = object.__new__(engine.Engine)
    eng.c = types.SimpleNamespace(vit_width=128, dec_hidden=128, dec_layers=2, max_frames=2, image_size=64, patch=16, max_image_tokens=25)
    eng.precision = "f16"
    assert eng.memory_rows == 50 and eng.memory_slot_bytes() == engine.memory_slot_bytes(128, 128, 2, 50, 2)
    eng.precision = "f32"
    assert eng.memory_slot_bytes() == engine.memory_slot_bytes(128, 128, 2, 50, 4)


# ---- Engine.recall's bookkeeping -------------------------------------------------------------------------------------------------
class _FakeLib:
    """gitmi_generate_prefixed as KEEP / RECALL see it: argument errors carry the kind's name, a late failure does not"""

    def __init__(self):
        self.err, self.fail, self.calls = b"", None, []

    def gitmi_last_error(self):
        return self.err

    def gitmi_generate_prefixed(self, h, frames, F, B, prefixes, ld, lens, image_of, Q, search, tok, lp, sent, info, stream):
        kind = search._obj.kind
        self.calls.append((kind, B, ld, [lens[q] for q in range(Q)], None if image_of is None else [image_of[q] for q in range(Q)],
                           prefixes, lp))
        if self.fail == "early":
            self.err = b"recall: slot 3: bad magic 0x00000000 / version 0 (nothing was kept there)"
            return 1
        if self.fail == "late":
            self.err = b"engine.hip:1: launch_memory_unpack -> invalid argument"
            return 1
        self.out[:] = torch.tensor(self.info)
        return 0


def _engine_mirror(monkeypatch):
    eng = object.__new__(engine.Engine)
    eng.lib, eng._h, eng.device, eng.precision = _FakeLib(), None, 0, "f16"
    eng.c = types.SimpleNamespace(vit_width=128, dec_hidden=128, dec_layers=2, max_frames=1, image_size=64, patch=16, max_image_tokens=0)
    eng._hw = (64, 64)
    eng._init_resident()
    store = torch.zeros(4, eng.memory_slot_bytes(), dtype=torch.uint8)
    monkeypatch.setattr(eng, "_store_arg", lambda s: int(s.shape[0]))
    monkeypatch.setattr(engine, "_stream", lambda: 0)
    real_zeros = torch.zeros

    def zeros(*a, **k):                                                 # info lives on the host here
        k.pop("device", None)
        eng.lib.out = real_zeros(*a, **k)
        return eng.lib.out

    monkeypatch.setattr(engine.torch, "zeros", zeros)
    return eng, store


def test_engine_recall_bookkeeping(monkeypatch):
    eng, store = _engine_mirror(monkeypatch)
    assert eng.resident is None and eng.resident_geometry is None
    eng.lib.info = [17, 17, 51, 0]
    g0 = eng.generation
    geo = [(1, (4, 4), 17, 0)] * 3
    assert eng.recall(store, [2, 0, 2], geo) == {"stride": 17, "max_rows": 17, "total_rows": 51}
    kind, B, ld, slots, image_of, recall_ptr, keep_ptr = eng.lib.calls[-1]
    assert (kind, B, ld, slots, image_of, keep_ptr) == (8, 3, 4, [2, 0, 2], None, None) and recall_ptr == store.data_ptr()
    assert eng.resident == 3 and eng.generation == g0 + 1
    assert eng.resident_geometry == (17, 1, [(4, 4)] * 3) and not isinstance(eng.resident_geometry, engine.Geometry)
    # KEEP over them: the store as logprob_out, residency untouched
    eng.lib.info = [86, 17, 34, 0]
    kept = eng.keep(store, [1, 3], images=[2, 0])
    kind, B, ld, slots, image_of, recall_ptr, keep_ptr = eng.lib.calls[-1]
    assert (kind, B, ld, slots, image_of, recall_ptr) == (7, 3, 4, [1, 3], [2, 0], None) and keep_ptr == store.data_ptr()
    assert kept == {"rows": [17, 17], "max_rows": 17, "total_rows": 34, "geometry": [(1, (4, 4), 17, 0)] * 2}
    assert eng.resident == 3 and eng.generation == g0 + 1
    # a key-count batch: context rows and different row counts make a Geometry
    eng.lib.info = [32, 23, 53, 0]
    mixed = [(1, (4, 4), 17, 6), (1, (4, 4), 17, 0), (1, (3, 4), 13, 0)]
    eng.recall(store, [0, 1, 2], mixed)
    geo = eng.resident_geometry
    assert isinstance(geo, engine.Geometry) and geo == (32, 1, [(4, 4), (4, 4), (3, 4)])
    assert geo.stride == 32 and geo.context == [6, 0, 0] and eng.generation == g0 + 2
    assert eng.keep(store, [0], images=[0])["geometry"] == [(1, (4, 4), 17, 6)]
    # an argument error leaves the resident set, a failed launch drops it
    eng.lib.fail = "early"
    with pytest.raises(engine.GitmiError, match="slot 3: bad magic"):
        eng.recall(store, [3])
    assert eng.resident == 3 and eng.generation == g0 + 2
    eng.lib.fail = "late"
    with pytest.raises(engine.GitmiError, match="launch_memory_unpack"):
        eng.recall(store, [0])
    assert eng.resident is None and eng.generation == g0 + 3
    with pytest.raises(ValueError, match="geometry has 1 entries for 2 slots"):
        eng.recall(store, [0, 1], [(1, (4, 4), 17, 0)])


def test_store_argument_is_checked():
    eng = object.__new__(engine.Engine)
    eng.c = types.SimpleNamespace(vit_width=128, dec_hidden=128, dec_layers=2, max_frames=1, image_size=64, patch=16, max_image_tokens=0)
    eng.precision, eng.device = "f16", 0
    n = eng.memory_slot_bytes()
    for bad in (torch.zeros(2, n, dtype=torch.int8), torch.zeros(2, n + 256, dtype=torch.uint8), torch.zeros(2 * n, dtype=torch.uint8),
                [0] * 8):
        with pytest.raises(ValueError, match="uint8 tensor"):
            eng._store_arg(bad)
    with pytest.raises(ValueError, match="engine's device"):
        eng._store_arg(torch.zeros(2, n, dtype=torch.uint8))             # on the CPU


# ---- ImageStore against a stub engine ---------------------------------------------------------------------------------------------
class _FakeEngine:
    """An engine context as ImageStore and the front end see it: a store slot holds the tag of the image kept there"""

    def __init__(self, name):
        self.name, self.calls = name, []
        self.resident, self.generation, self.images = None, 0, []
        self.c = types.SimpleNamespace(max_batch=8, max_frames=1)

    def set_temporal_embedding(self, on):
        pass

    def check_finite(self, info):
        pass

    def memory_slot_bytes(self):
        return 8

    def memory_store(self, slots):
        return torch.zeros(slots, 8, dtype=torch.uint8)

    def generate(self, frames, search, prefix=None, sync=True, host_out=False):
        self.calls.append(("generate", frames is None))
        if frames is not None:
            self.images = [int(v) for v in frames[0][:, 0, 0, 0]]
            self.resident, self.generation = len(self.images), self.generation + 1
        B = self.resident
        return torch.full((B, search.max_steps), 102), torch.zeros(B), torch.tensor([search.max_steps, 0, 0, 0])

    def generate_prefixed(self, frames, search, prefixes, image_of=None, sync=True, host_out=False):
        self.calls.append(("generate_prefixed", frames is None))
        Q, T = len(prefixes), search.max_steps
        tok = torch.full((Q, T), 102)
        for q, p in enumerate(prefixes):
            tok[q, :len(p)] = torch.tensor(p)
            tok[q, len(p)] = 1000 + self.images[image_of[q]]                 # the answer names the image it was asked about
        return tok, torch.zeros(Q), torch.tensor([[len(p) + 1, 0] for p in prefixes]), torch.tensor([T, 0, 0, 0])

    def score(self, frames, tokens, lengths=None, image_of=None):
        self.calls.append(("score", frames is None))
        return torch.zeros(tokens.shape[0], tokens.shape[1], 2)

    def keep(self, store, slots, images=None):
        images = list(range(len(slots))) if images is None else images
        self.calls.append(("keep", list(slots), list(images)))
        for s, b in zip(slots, images):
            store[s, 0] = self.images[b]
        return {"rows": [17] * len(slots), "max_rows": 17, "total_rows": 17 * len(slots),
                "geometry": [(1, (4, 4), 17, 0)] * len(slots)}

    def recall(self, store, slots, geometry=None):
        self.calls.append(("recall", list(slots)))
        assert geometry == [(1, (4, 4), 17, 0)] * len(slots)
        self.images = [int(store[s, 0]) for s in slots]
        self.resident, self.generation = len(slots), self.generation + 1
        return {"stride": 17, "max_rows": 17, "total_rows": 17 * len(slots)}


@pytest.fixture
def no_device(monkeypatch):
    """Pending.result() waits for the current stream: nothing to wait for here"""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: types.SimpleNamespace(synchronize=lambda: None))


def _model(contexts=1):
    cfg = types.SimpleNamespace(num_frames=0, sos=101, eos=102, vocab=30522)
    m = object.__new__(M.CaptioningModel)
    m.cfg = cfg
    m.decoder = M.AutoRegressiveBeamSearch(eos_index=102, max_steps=10, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    m.engine, m._loaded, m.training = _FakeEngine("ctx0"), True, False
    if contexts > 1:
        m._ctxs = [m.engine] + [_FakeEngine(f"ctx{i}") for i in range(1, contexts)]
        m._streams = [None] * contexts
        m._next = 0
    return m


def _images(*tags):
    x = torch.zeros(len(tags), 3, 8, 8)
    x[:, 0, 0, 0] = torch.tensor(tags, dtype=torch.float32)
    return {"image": x}


def test_image_store_keys_lru_and_eviction(no_device):
    m = _model()
    store = M.ImageStore(m, 3)
    assert len(store) == 0 and "a" not in store and store.tensor.shape == (3, 8)
    first = m.submit(_images(10, 11, 12))
    store.put(first, ["a", "b"], images=[2, 0])                          # a = image 12, b = image 10
    assert len(store) == 2 and "a" in store and "b" in store and store.keys() == ["a", "b"]
    store.put(first.result(), ["c"], images=[1])                        # the result is a handle too; the store is full now
    assert store.keys() == ["a", "b", "c"]
    store.recall(["a"])                                                 # a is the most recently used now
    assert store.keys() == ["b", "c", "a"]
    second = m.submit(_images(20, 21))
    store.put(second, ["d"])                                            # b, the least recently used, makes room
    assert "b" not in store and store.keys() == ["c", "a", "d"] and len(store) == 3
    store.put(second, ["a"], images=[1])                                # a key that is held is overwritten in its slot
    assert len(store) == 3 and store.keys() == ["c", "d", "a"]
    h = store.recall(["a", "c", "a"])
    assert m.engine.images == [21, 11, 21]
    out = m.submit_followup({"prefixes": [[101, 5]] * 3, "image_of": [0, 1, 2]}, on=h).result()
    assert out["predictions"] == [[1021], [1011], [1021]]
    store.evict("c")
    assert "c" not in store and len(store) == 2
    with pytest.raises(KeyError, match="never kept, or evicted"):
        store.recall(["a", "c"])
    with pytest.raises(KeyError):
        store.evict("zzz")
    store.put(h, ["e", "f"], images=[1, 0])                             # from a recalled batch; one free slot, one eviction (d)
    assert store.keys() == ["a", "e", "f"]
    with pytest.raises(ValueError, match="exceed the 3 slots"):
        store.put(h, ["p", "q", "r", "s"], images=[0, 1, 2, 0])
    with pytest.raises(ValueError, match="every key once"):
        store.put(h, ["p", "p"])
    with pytest.raises(ValueError, match="resident images"):
        store.put(h, ["p"], images=[3])
    with pytest.raises(TypeError):
        store.put({"predictions": []}, ["p"])
    with pytest.raises(ValueError):
        M.ImageStore(m, 0)


def test_recall_handles_go_stale_and_work_as_on(no_device):
    m = _model()
    store = M.ImageStore(m, 4)
    first = m.submit(_images(1, 2, 3))
    store.put(first, ["x", "y", "z"])
    m.submit(_images(7, 8))                                             # forty other requests later ...
    with pytest.raises(M.StaleImagesError):
        store.put(first, ["late"])                                      # ... the images of `first` are gone from its context
    h = store.recall(["z", "x"])
    assert h.result() == {"stride": 17, "max_rows": 17, "total_rows": 34} and h.engine is m.engine
    assert m.submit_answers(None, [[101, 9]], image_of=[0], on=h).result() == [[1003]]
    assert m.submit_answers(None, [[101, 9]], image_of=[1], on=h.result()).result() == [[1001]]
    m.score(None, [[101, 5, 102]], image_of=[1], on=h)
    assert m.engine.calls[-1] == ("score", True)
    assert m({"prefixes": [[101]], "image_of": [1]})["predictions"] == [[1001]]      # without on=: the context of the recall
    m.submit(_images(9))                                                # another encode on the context: the handle is stale
    with pytest.raises(M.StaleImagesError, match="no longer resident"):
        m.submit_answers(None, [[101]], image_of=[0], on=h)
    with pytest.raises(M.StaleImagesError):
        m.score(None, [[101, 5]], image_of=[0], on=h)
    h2 = store.recall(["y"])                                            # and a new recall brings them back
    assert m.submit_answers(None, [[101]], image_of=[0], on=h2).result() == [[1002]]


def test_pipelined_store_reads_from_the_producer_and_binds_to_the_recalling_context(no_device):
    m = _model(contexts=3)
    store = M.ImageStore(m, 4)
    pa = m.submit(_images(1, 2))                                        # ctx0
    pb = m.submit(_images(5, 6, 7))                                     # ctx1
    store.put(pb, ["b0", "b2"], images=[0, 2])
    store.put(pa, ["a1"], images=[1])
    assert pa.engine.calls[-1][0] == "keep" and pb.engine.calls[-1][0] == "keep" and pa.engine is not pb.engine
    h = store.recall(["b2", "a1", "b0"])                                # the next context of the rotation: ctx2
    assert h.engine.name == "ctx2" and h.engine.images == [7, 2, 5]
    assert m.submit_answers(None, [[101]] * 3, image_of=[0, 1, 2], on=h).result() == [[1007], [1002], [1005]]
    assert pa.engine.resident == 2 and pb.engine.resident == 3          # the producers keep their own images
    assert m.submit_answers(None, [[101]], image_of=[1], on=pa).result() == [[1002]]
    h0 = store.recall(["b0"], context=pa.engine)                        # on a context of the caller's choice
    assert h0.engine is pa.engine
    with pytest.raises(M.StaleImagesError):
        m.submit_answers(None, [[101]], image_of=[1], on=pa)
    assert m.submit_answers(None, [[101]], image_of=[0]).result() == [[1005]]         # the most recent context is the recall's
