"""Per-sentence decoding constraints, host side (no GPU): the header defines GITMI_SEARCH_CONSTRAIN = 10 under ABI 10 without a
new export, engine.constraint_tables normalises the search_param keys (scalar or per sentence, deduplicated sets, the complement
of an allowed list with the tail bits clear) and rejects every malformed value by naming sentence and field, the front end arms
the context it is about to submit to -- on that context's stream, immediately before the call -- and arms nothing without the
new keys, and tools/constrained_step.wrap_step equals a brute-force restatement of the definition."""
import contextlib
import os
import re
import types

import numpy as np
import pytest
import torch

from generativeimage2text_amd import engine
from generativeimage2text_amd import model as M
from tools.constrained_step import wrap_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gitmi.h")).read()


def test_header_defines_kind_10_under_abi_10():
    hdr = _header()
    assert re.search(r"#define\s+GITMI_SEARCH_CONSTRAIN\s+10\b", hdr) and engine.SEARCH_CONSTRAIN == 10
    assert re.search(r"#define\s+GITMI_ABI_VERSION\s+10\b", hdr)
    assert len(engine.EXPORTED_SYMBOLS) == 40
    assert sorted(set(re.findall(r"\b(gitmi_[a-z_0-9]+)\s*\(", hdr))) == sorted(engine.EXPORTED_SYMBOLS)


def test_header_documents_the_argument_mapping():
    hdr = _header()
    doc = hdr[hdr.index("search->kind == GITMI_SEARCH_CONSTRAIN arms"):]
    doc = doc[:doc.index("int  gitmi_generate_prefixed(")]
    text = " ".join(doc.replace("*", " ").split())
    for phrase in ("one-shot", "z[c] = -10000", "bit c % 32 of word c / 32", "t - P_s < min_new[s]", "n == 1 bans every token of the history",
                   "frames : must be NULL", "uint32 [n_sets][W], W = ceil(vocab / 32)", "keeps no pointer", "bits at or above vocab are ignored",
                   "ld_prefix : n_sets, 0 .. max_batch", "prefix_len_host : int32 [Q][3] = { set index or -1, min_new, ngram }",
                   "image_of_host : must be NULL", "Q == 0 disarms", "info_out : { Q, n_sets, W, 0 }", "set index in [-1, n_sets)",
                   "0 <= min_new <= max_text_len", "0 <= ngram <= 8", "names both numbers and stays armed",
                   "GITMI_SEARCH_TRIE and gitmi_search_begin refuse by name", "A clone starts disarmed", "keep their footprint",
                   "replay one graph"):
        assert phrase in text, phrase


# ---- engine.constraint_tables -------------------------------------------------------------------------------------------------------
V, EOS = 1000, 102


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")


def test_nothing_to_constrain_is_none():
    assert engine.constraint_tables(3, V, EOS) is None
    assert engine.constraint_tables(3, V, EOS, min_new_tokens=0, no_repeat_ngram_size=[0, 0, 0], bad_tokens=None) is None
    assert engine.constraint_tables(2, V, EOS, bad_tokens=[None, []]) is None           # an empty bad list bans nothing


def test_scalars_become_per_sentence_rows():
    words, table = engine.constraint_tables(3, V, EOS, min_new_tokens=4, no_repeat_ngram_size=3)
    assert words.shape == (0, 32) and words.dtype == np.uint32 and table == [[-1, 4, 3]] * 3
    words, table = engine.constraint_tables(3, V, EOS, min_new_tokens=[0, 2, 0], no_repeat_ngram_size=[1, 0, 8], bad_tokens=[5, 999])
    assert table == [[0, 0, 1], [0, 2, 0], [0, 0, 8]] and words.shape == (1, 32)
    assert np.flatnonzero(_bits(words[0])).tolist() == [5, 999]


def test_identical_sets_are_stored_once():
    words, table = engine.constraint_tables(5, V, EOS, bad_tokens=[[7, 3], None, [3, 7, 7], [8], torch.tensor([3, 7])])
    assert [r[0] for r in table] == [0, -1, 0, 1, 0] and words.shape == (2, 32)
    assert np.flatnonzero(_bits(words[1])).tolist() == [8]


def test_allowed_tokens_are_complemented_with_the_tail_clear():
    words, table = engine.constraint_tables(2, V, EOS, allowed_tokens=[[11, 12], None], bad_tokens=[None, [4]])
    assert table == [[0, 0, 0], [1, 0, 0]]
    b = _bits(words[0])
    assert b.size == 1024 and not b[1000:].any()                        # bits 1000 .. 1023 of the last word stay clear
    assert sorted(np.flatnonzero(b == 0)[:3].tolist()) == [11, 12, EOS] and int(b.sum()) == V - 3      # [SEP] stays allowed
    # ... unless it is banned explicitly; a bad token inside the allowed list is banned too
    words, _ = engine.constraint_tables(1, V, EOS, allowed_tokens=[11, 12], bad_tokens=[EOS, 12])
    assert np.flatnonzero(_bits(words[0]) == 0).tolist()[:2] == [11, 1000] and _bits(words[0])[EOS] == 1
    # a vocabulary that is no multiple of 32: 30522 = 953 words + 26 bits
    words, _ = engine.constraint_tables(1, 30522, EOS, allowed_tokens=[30521])
    assert words.shape == (1, 954) and int(words[0, 953]) == (1 << 25) - 1


@pytest.mark.parametrize("kw, match", [
    (dict(min_new_tokens=[1, 2]), "min_new_tokens has 2 entries for 3 sentences"),
    (dict(no_repeat_ngram_size=[1, 2, 3, 4]), "no_repeat_ngram_size has 4 entries for 3 sentences"),
    (dict(bad_tokens=[[1], [2]]), "bad_tokens has 2 entries for 3 sentences"),
    (dict(allowed_tokens=[[1]] * 4), "allowed_tokens has 4 entries for 3 sentences"),
    (dict(min_new_tokens=-1), r"sentence 0: min_new_tokens -1 outside \[0, 20\]"),
    (dict(min_new_tokens=[0, 21, 0]), r"sentence 1: min_new_tokens 21 outside \[0, 20\]"),
    (dict(min_new_tokens=[0, 1.5, 0]), "sentence 1: min_new_tokens 1.5"),
    (dict(no_repeat_ngram_size=9), r"sentence 0: no_repeat_ngram_size 9 outside \[0, 8\]"),
    (dict(no_repeat_ngram_size=[0, 0, -2]), r"sentence 2: no_repeat_ngram_size -2 outside \[0, 8\]"),
    (dict(bad_tokens=[1000]), r"sentence 0: bad_tokens holds token 1000 outside \[0, 1000\)"),
    (dict(bad_tokens=[None, [3, -1], None]), r"sentence 1: bad_tokens holds token -1 outside \[0, 1000\)"),
    (dict(allowed_tokens=[None, None, [5000]]), r"sentence 2: allowed_tokens holds token 5000 outside \[0, 1000\)"),
    (dict(bad_tokens=[None, "abc", None]), "sentence 1: bad_tokens must be a list of token ids"),
])
def test_every_malformed_value_names_sentence_and_field(kw, match):
    with pytest.raises(ValueError, match=match):
        engine.constraint_tables(3, V, EOS, max_new=20, **kw)


def test_no_sentences():
    with pytest.raises(ValueError, match="constraints for 0 sentences"):
        engine.constraint_tables(0, V, EOS, min_new_tokens=1)


# ---- the front end arms the context it submits to -----------------------------------------------------------------------------------
class _FakeEngine:
    def __init__(self, name, log):
        self.name, self.log = name, log
        self.resident, self.generation = None, 0
        self.c = types.SimpleNamespace(max_batch=8, max_frames=1, max_text_len=10, patch=16)
        self.max_tokens, self.max_context = 17, 0

    def _note(self, what, *more):
        self.log.append((self.name, _Cuda.current, what) + more)

    def set_temporal_embedding(self, on):
        pass

    def check_finite(self, info):
        pass

    def ragged(self, images):
        return ("ragged", len(images))

    def constrain(self, words, table):
        self._note("constrain", np.asarray(words).shape, [list(r) for r in table])

    def generate(self, frames, search, prefix=None, sync=True, host_out=False):
        self._note("generate")
        if frames is not None:
            self.resident, self.generation = 3, self.generation + 1
        return None, None, None

    def generate_prefixed(self, frames, search, prefixes, image_of=None, sync=True, host_out=False):
        self._note("generate_prefixed", len(prefixes))
        if frames is not None:
            self.resident, self.generation = 3, self.generation + 1
        return None, None, None, None


class _Cuda:
    """torch.cuda as model.Pending uses it, without a device: the stream a call is enqueued on is the one `stream()` entered"""
    current = "caller"

    @staticmethod
    def current_stream():
        return _Cuda.current

    @staticmethod
    @contextlib.contextmanager
    def stream(s):
        before, _Cuda.current = _Cuda.current, s.name
        try:
            yield
        finally:
            _Cuda.current = before

    class Event:
        def record(self):
            pass


class _Stream:
    def __init__(self, name):
        self.name = name

    def wait_stream(self, other):
        pass


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(M.torch, "cuda", _Cuda)


def _model(contexts=1, kind="greedy"):
    m = object.__new__(M.CaptioningModel)
    m.cfg = types.SimpleNamespace(num_frames=0, sos=101, eos=EOS, vocab=V)
    if kind == "greedy":
        m.decoder = M.AutoRegressiveBeamSearch(eos_index=EOS, max_steps=10, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    else:
        m.decoder = M.GeneratorWithBeamSearch(eos_index=EOS, max_steps=10, beam_size=2, per_node_beam_size=2, length_penalty=0.6)
    m.log = []
    m.engine, m._loaded, m.training = _FakeEngine("ctx0", m.log), True, False
    if contexts > 1:
        m._ctxs = [m.engine] + [_FakeEngine(f"ctx{i}", m.log) for i in range(1, contexts)]
        m._streams = [_Stream(f"s{i}") for i in range(contexts)]
        m._next = 0
    return m


IMAGES = torch.zeros(3, 3, 8, 8)
SP = dict(min_new_tokens=[0, 2, 0], no_repeat_ngram_size=2, bad_tokens=[[5], None, [5]])
TABLE = [[0, 0, 2], [-1, 2, 2], [0, 0, 2]]


def test_submit_arms_right_before_the_call(no_device):
    m = _model()
    m.submit({"image": IMAGES}, SP)
    assert m.log == [("ctx0", "caller", "constrain", (1, 32), TABLE), ("ctx0", "caller", "generate")]


def test_without_the_new_keys_nothing_is_armed(no_device):
    m = _model()
    m.submit({"image": IMAGES})
    m.submit({"image": IMAGES}, {"min_new_tokens": 0, "no_repeat_ngram_size": 0, "bad_tokens": None})
    m.submit_answers(IMAGES, [[101, 7]] * 2, image_of=[0, 1])
    m.submit_ragged([torch.zeros(3, 16, 16), torch.zeros(3, 32, 16)])
    assert [e[2] for e in m.log] == ["generate", "generate", "generate_prefixed", "generate"]


def test_pipelined_contexts_are_armed_on_their_own_stream(no_device):
    m = _model(contexts=3)
    m.submit({"image": IMAGES}, SP)
    m.submit({"image": IMAGES})
    first = m.submit({"image": IMAGES}, {"min_new_tokens": 3})
    assert m.log == [("ctx0", "s0", "constrain", (1, 32), TABLE), ("ctx0", "s0", "generate"), ("ctx1", "s1", "generate"),
                     ("ctx2", "s2", "constrain", (0, 32), [[-1, 3, 0]] * 3), ("ctx2", "s2", "generate")]
    # a follow-up goes to the context of the call it is about, armed there
    del m.log[:]
    m.submit_followup({"prefixes": [[101, 5], [101, 6]], "image_of": [2, 0]}, {"bad_tokens": [[9], [9]]}, on=first)
    assert m.log == [("ctx2", "s2", "constrain", (1, 32), [[0, 0, 0]] * 2), ("ctx2", "s2", "generate_prefixed", 2)]


def test_every_front_end_form_arms(no_device):
    m = _model()
    m.submit_answers(IMAGES, [[101, 7], [101, 8, 9]], image_of=[0, 2], search_param={"min_new_tokens": [1, 4]})
    m.submit_answers(None, [[101, 7]], image_of=[1], search_param={"no_repeat_ngram_size": 3})
    m.submit_ragged([torch.zeros(3, 16, 16), torch.zeros(3, 32, 16)], search_param={"allowed_tokens": [3, 4]})
    m.submit_ragged([torch.zeros(3, 16, 16)], prefixes=[[101, 1], [101, 2]], image_of=[0, 0], search_param={"min_new_tokens": [0, 5]})
    got = [(e[2],) + e[3:] for e in m.log]
    assert got == [("constrain", (0, 32), [[-1, 1, 0], [-1, 4, 0]]), ("generate_prefixed", 2),
                   ("constrain", (0, 32), [[-1, 0, 3]]), ("generate_prefixed", 1),
                   ("constrain", (1, 32), [[0, 0, 0]] * 2), ("generate",),
                   ("constrain", (0, 32), [[-1, 0, 0], [-1, 5, 0]]), ("generate_prefixed", 2)]


def test_num_return_sequences_replicates_the_rows(no_device):
    m = _model(kind="generator")
    m.submit({"image": IMAGES}, dict(SP, num_return_sequences=2, do_sample=True))
    assert m.log[0][4] == [row for row in TABLE for _ in range(2)] and m.log[1][2:] == ("generate_prefixed", 6)


def test_bad_words_go_through_the_tokenizer(no_device):
    m = _model()
    pieces = {"cat": [201], "dog": [202], "catapult": [201, 77]}
    m.tokenizer = lambda w, add_special_tokens=False: {"input_ids": pieces[w]}
    m.submit({"image": IMAGES}, {"bad_words": ["cat", "dog"], "bad_tokens": [3]})
    words = m._constraints({"bad_words": ["cat", "dog"], "bad_tokens": [3]}, 3)[0]
    assert np.flatnonzero(_bits(words[0])).tolist() == [3, 201, 202]
    assert m.log[0][4] == [[0, 0, 0]] * 3
    # per-sentence bad_tokens whose first entry is None, beside one word list for all
    words, table = m._constraints({"bad_words": ["cat"], "bad_tokens": [None, [3], None]}, 3)
    assert [r[0] for r in table] == [0, 1, 0]
    assert np.flatnonzero(_bits(words[0])).tolist() == [201] and np.flatnonzero(_bits(words[1])).tolist() == [3, 201]
    # per-sentence word lists
    words, table = m._constraints({"bad_words": [["cat"], None, ["dog"]]}, 3)
    assert [r[0] for r in table] == [0, -1, 1] and np.flatnonzero(_bits(words[1])).tolist() == [202]
    with pytest.raises(ValueError, match="bad_tokens has 2 entries for 3 sentences"):
        m._constraints({"bad_words": ["cat"], "bad_tokens": [None, [3]]}, 3)
    with pytest.raises(ValueError, match="'catapult' is 2 WordPieces"):
        m.submit({"image": IMAGES}, {"bad_words": ["cat", "catapult"]})
    m.tokenizer = None
    with pytest.raises(ValueError, match="needs the model's tokenizer"):
        m.submit({"image": IMAGES}, {"bad_words": ["cat"]})


def test_host_errors_come_before_anything_is_enqueued(no_device):
    m = _model()
    with pytest.raises(ValueError, match=r"sentence 1: min_new_tokens 11 outside \[0, 10\]"):
        m.submit({"image": IMAGES}, {"min_new_tokens": [0, 11, 0]})
    with pytest.raises(ValueError, match="bad_tokens has 2 entries for 3 sentences"):
        m.submit({"image": IMAGES}, {"bad_tokens": [[1], [2]]})
    with pytest.raises(NotImplementedError, match="frobnicate"):
        m.submit({"image": IMAGES}, {"frobnicate": 1})
    assert m.log == []


# ---- wrap_step against a brute-force restatement ------------------------------------------------------------------------------------
def _brute(z, tokens, sets, table, eos, plen):
    """the definition of include/gitmi.h, token by token"""
    z = z.clone()
    rows, t = tokens.shape
    beams = rows // len(table)
    for r in range(rows):
        s = r // beams
        set_index, min_new, n = table[s]
        x = tokens[r].tolist()
        for c in range(z.shape[1]):
            banned = set_index >= 0 and (int(sets[set_index][c // 32]) >> (c % 32)) & 1
            banned = banned or (c == eos and t - plen[s] < min_new)
            if n > 0 and t >= n - 1:
                for i in range(0, t - n + 1):
                    if x[i:i + n - 1] == x[t - n + 1:t] and x[i + n - 1] == c:
                        banned = True
            if banned:
                z[r, c] = -10000.0
    return z


@pytest.mark.parametrize("seed", range(6))
def test_wrap_step_equals_the_definition(seed):
    g = torch.Generator().manual_seed(seed)
    vocab, S, beams = 70, 4, 1 + seed % 3                       # 70 tokens: two full words and 6 bits of a third
    eos = 9
    sets = np.array([[0x80000001, 0x00000100, 0xffffffe1], [0, 0, 0x3f]], dtype=np.uint32)      # bits 70 .. 95 are set: ignored
    table = [[0, 0, 0], [-1, 3, 0], [1, 0, 1 + seed % 4], [0, 5, 2]]
    plen = [1, 2, 1, 3]
    for t in (1, 2, 3, 6, 9):
        # few distinct tokens: histories full of repeated n-grams
        tokens = torch.randint(0, 6, (S * beams, t), generator=g)
        z = torch.randn(S * beams, vocab, generator=g)
        got = wrap_step(lambda _tok: z, sets, table, eos, plen)(tokens)
        want = _brute(z, tokens, sets, table, eos, plen)
        assert torch.equal(got, want), (t, (got != want).nonzero())
        assert (got == -10000.0).any() and torch.equal(got[got != -10000.0], z[got != -10000.0])
