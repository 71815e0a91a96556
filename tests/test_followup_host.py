"""Follow-up calls on resident images, host side (no GPU): the header documents the frames == NULL form of both entry points
without a new export, Engine mirrors the residency rules, and the front end routes requests without images to the follow-up
path and refuses a handle whose images have been replaced."""
import os
import re
import types

import pytest
import torch

from generativeimage2text_amd import engine
from generativeimage2text_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the product ABI as it stood before follow-up calls: the feature is a new meaning of an argument, not a new entry point
SYMBOLS = """gitmi_abi_version gitmi_last_error gitmi_create gitmi_destroy gitmi_load_tensor gitmi_finalize_weights
gitmi_encode_frames gitmi_prefill gitmi_step_logits gitmi_generate gitmi_search_begin gitmi_search_rows gitmi_search_advance
gitmi_search_finish gitmi_profile_enable gitmi_profile_read gitmi_set_graph gitmi_op_gemm gitmi_op_layernorm gitmi_op_attention
gitmi_op_dgemm gitmi_op_dgemm_res gitmi_op_vocab_topm gitmi_clone gitmi_op_attn_decode gitmi_preprocess_image
gitmi_set_image_shape gitmi_preprocess_image_to gitmi_generate_prefixed gitmi_set_temporal_embedding gitmi_op_kv_repack
gitmi_set_encode_after gitmi_op_sample_rows gitmi_search_done_count gitmi_set_trie gitmi_operand_dtype gitmi_set_shared_device
gitmi_preprocess_batch gitmi_set_ln_fold gitmi_op_gemm_ln""".split()


def _header():
    return open(os.path.join(ROOT, "include", "gitmi.h")).read()


def test_no_new_export_and_same_abi():
    assert engine.EXPORTED_SYMBOLS == SYMBOLS and len(SYMBOLS) == 40
    hdr = _header()
    assert sorted(set(re.findall(r"\b(gitmi_[a-z_0-9]+)\s*\(", hdr))) == sorted(SYMBOLS)
    assert re.search(r"#define\s+GITMI_ABI_VERSION\s+10\b", hdr)
    import ctypes as C
    assert C.sizeof(engine.GitmiConfig) == 84 and C.sizeof(engine.GitmiSearch) == 72


def test_header_documents_the_null_frames_form_of_both_entry_points():
    hdr = _header()
    doc = hdr[hdr.index("follow-up calls on resident images"):]
    doc = doc[:doc.index("int  gitmi_generate(")]
    text = " ".join(doc.replace("*", " ").split())
    assert "gitmi_generate(e, frames = NULL" in text and "gitmi_generate_prefixed(e, frames = NULL" in text
    for phrase in ("GITMI_SEARCH_SCORE", "F is ignored", "B must equal the number of resident images", "gitmi_encode_frames",
                   "gitmi_set_image_shape", "gitmi_set_temporal_embedding", "gitmi_set_ln_fold", "a clone starts with none",
                   "info_out[3]", "re-captures neither", "vit_ms, prefill_ms and vit_gemm_"):
        assert phrase in text, phrase
    # the argument lists of the two declarations are what they were
    assert "int  gitmi_generate(gitmi_engine* e, const float* const* frames, int F, int B," in hdr
    assert "int  gitmi_generate_prefixed(gitmi_engine* e, const float* const* frames, int F, int B," in hdr


# ---- Engine's host mirror ----------------------------------------------------------------------------------------------------
class _FakeLib:
    """The residency rules of the library on the host: enough of gitmi_generate / the setters for Engine's mirror."""

    def __init__(self):
        self.resident, self.err, self.temb = None, b"", True

    def gitmi_last_error(self):
        return self.err

    def gitmi_generate(self, h, frames, F, B, prefix, P, search, tok, lp, info, stream):
        if frames is None:
            if self.resident is None:
                self.err = b"generate: frames == NULL is a follow-up call, but the engine holds no resident images"
                return 1
            if B != self.resident:
                self.err = b"generate: follow-up call with B=%d, but %d images are resident" % (B, self.resident)
                return 1
        if prefix is not None and P < 1:
            self.err = b"generate: prefix length 0 outside [1,40]"
            return 1
        if self.fail == "early":
            self.err = b"generate: max_steps 99 outside [P,40]"
            return 1
        if frames is not None:
            self.resident = None
            if self.fail == "late":
                self.err = b"search: beam_size 9 outside [1,4]"
                return 1
            self.resident = B
        return 0

    fail = None

    def gitmi_set_temporal_embedding(self, h, on):
        if bool(on) != self.temb:
            self.temb, self.resident = bool(on), None
        return 0


def _engine_mirror():
    eng = object.__new__(engine.Engine)
    eng.lib, eng._h, eng.device = _FakeLib(), None, 0
    eng._init_resident()
    eng._temb, eng._ln_fold = True, False
    return eng


def _generate(eng, frames, B):
    s = engine.GitmiSearch()
    rc = eng.lib.gitmi_generate(None, frames, 1, B, None, 1, s, None, None, None, None)
    eng._call(frames, rc, B)
    return rc


def test_engine_mirrors_the_residency_rules():
    eng = _engine_mirror()
    assert eng.resident is None and eng._frames_arg(None) == (None, [], 0)
    assert _generate(eng, ["frames"], 3) == 0
    assert eng.resident == 3 and eng._frames_arg(None) == (None, [], 3)
    g = eng.generation
    assert _generate(eng, None, 3) == 0 and eng.generation == g          # a follow-up changes nothing
    eng.lib.fail = "early"                                              # an argument error before any launch: still resident
    with pytest.raises(engine.GitmiError, match="max_steps 99"):
        _generate(eng, ["frames"], 2)
    assert eng.resident == 3 and eng.generation > g
    eng.lib.fail = "late"                                               # a failure after the encode started: gone
    with pytest.raises(engine.GitmiError, match="beam_size 9"):
        _generate(eng, ["frames"], 2)
    assert eng.resident is None
    eng.lib.fail = None
    _generate(eng, ["frames"], 2)
    g = eng.generation
    eng.set_temporal_embedding(True)                                    # no flip: kept
    assert eng.resident == 2 and eng.generation == g
    eng.set_temporal_embedding(False)
    assert eng.resident is None and eng.generation > g


# ---- the front end ------------------------------------------------------------------------------------------------------------------
class _FakeEngine:
    """An engine context as the front end sees it: records the calls, answers with the image index of every sentence"""

    def __init__(self, name):
        self.name, self.calls = name, []
        self.resident, self.generation = None, 0
        self.c = types.SimpleNamespace(max_batch=8, max_frames=1)

    def set_temporal_embedding(self, on):
        pass

    def check_finite(self, info):
        pass

    def _encode(self, frames):
        if frames is not None:
            self.resident, self.generation = int(frames[0].shape[0]), self.generation + 1

    def generate(self, frames, search, prefix=None, sync=True, host_out=False):
        self.calls.append(("generate", frames is None))
        self._encode(frames)
        B = self.resident
        return torch.full((B, search.max_steps), 102), torch.zeros(B), torch.tensor([search.max_steps, 0, 0, 0])

    def generate_prefixed(self, frames, search, prefixes, image_of=None, sync=True, host_out=False):
        self.calls.append(("generate_prefixed", frames is None))
        self._encode(frames)
        Q, T = len(prefixes), search.max_steps
        tok = torch.full((Q, T), 102)
        for q, p in enumerate(prefixes):
            tok[q, :len(p)] = torch.tensor(p)
            tok[q, len(p)] = 1000 + image_of[q]
        sent = torch.tensor([[len(p) + 1, 0] for p in prefixes])
        return tok, torch.zeros(Q), sent, torch.tensor([T, 0, 0, 0])

    def score(self, frames, tokens, lengths=None, image_of=None):
        self.calls.append(("score", frames is None))
        self._encode(frames)
        return torch.zeros(tokens.shape[0], tokens.shape[1], 2)


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


def test_batch_without_image_is_routed_to_the_followup_path(no_device):
    m = _model()
    with pytest.raises(M.StaleImagesError, match="no resident images"):
        m({"prefix": torch.tensor([[101, 7]]), "image_of": [0]})
    first = m({"image": torch.zeros(3, 3, 8, 8)})
    assert m.engine.calls == [("generate", False)] and m.engine.resident == 3
    out = m({"prefix": torch.tensor([[101, 7]]), "image_of": [2, 0, 2]})
    assert m.engine.calls[-1] == ("generate_prefixed", True)
    assert out["predictions"] == [[1002], [1000], [1002]] and out["logprobs"].shape == (3, 1)
    out = m({"prefixes": [[101], [101, 5, 6]], "image_of": [1, 1]}, on=first)
    assert out["predictions"] == [[1001], [1001]]
    with pytest.raises(ValueError, match="image_of"):
        m({"prefix": torch.tensor([[101, 7]])})
    with pytest.raises(ValueError, match="resident images"):
        m({"prefixes": [[101]], "image_of": [3]})
    assert m.submit_answers(None, [[101, 9]], image_of=[1]).result() == [[1001]]
    assert m.submit_ragged(None, [[101, 9]], image_of=[2]).result()["predictions"] == [[1002]]
    m.score(None, [[101, 5, 102]], image_of=[0])
    assert m.engine.calls[-1] == ("score", True)
    with pytest.raises(ValueError, match="follow-up"):
        m.submit({"image": torch.zeros(1, 3, 8, 8)}, on=first)
    assert m.engine.generation == 1                                     # no follow-up touched the images


def test_followup_runs_on_the_context_of_its_handle_and_refuses_a_stale_one(no_device):
    m = _model(contexts=2)
    pa = m.submit({"image": torch.zeros(2, 3, 8, 8)})
    pb = m.submit({"image": torch.zeros(3, 3, 8, 8)})
    assert (pa.engine.name, pb.engine.name) == ("ctx0", "ctx1") and (pa.generation, pb.generation) == (1, 1)
    m.submit_answers(None, [[101]], image_of=[2]).result()               # without on=: the most recent call's context
    assert pb.engine.calls[-1] == ("generate_prefixed", True) and len(pa.engine.calls) == 1
    m.submit_answers(None, [[101]], image_of=[1], on=pa).result()
    assert pa.engine.calls[-1] == ("generate_prefixed", True)
    m.submit_answers(None, [[101]], image_of=[0], on=pb.result()).result()   # the result object is a handle too
    assert len(pb.engine.calls) == 3 and m._next == 2                    # follow-ups do not advance the rotation
    pc = m.submit({"image": torch.zeros(2, 3, 8, 8)})                    # back on ctx0: pa's images are replaced
    assert pc.engine is pa.engine
    with pytest.raises(M.StaleImagesError, match="no longer resident"):
        m.submit_answers(None, [[101]], image_of=[0], on=pa)
    with pytest.raises(M.StaleImagesError):
        m.score(None, [[101, 5]], image_of=[0], on=pa.result())
    m.submit_answers(None, [[101]], image_of=[0], on=pc).result()
    with pytest.raises(TypeError):
        m.submit_answers(None, [[101]], image_of=[0], on={"predictions": []})
