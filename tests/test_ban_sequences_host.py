"""Banned token sequences, host side (no GPU): engine.banned_sequence_tables (one list for all or one per sentence, deduplicated
lists, length-1 ids routed to the sets, every malformed value named, the pool layout word for word),
tools/constrained_step.sequence_banned against a brute-force restatement, the front end with a fake engine (sequences=, the
replication for num_return_sequences, the old two-argument call without the new keys, bad_words' old message), and the header:
ABI 10, 40 entry points, the extension named."""
import os
import re

import numpy as np
import pytest
import torch

import test_constraints_host as H
from generativeimage2text_amd import engine
from generativeimage2text_amd import model as M
from test_constraints_host import IMAGES, V, _bits, _model, no_device  # noqa: F401
from tools.constrained_step import BANNED, sequence_banned, wrap_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- engine.banned_sequence_tables ---------------------------------------------------------------------------------------------------
def test_one_list_for_all_sentences_and_the_pool_word_for_word():
    singles, pool = engine.banned_sequence_tables(3, V, [[5, 6], [7, 8, 9], [4]])
    assert singles == [[4]] * 3
    #                       L  S  T  0  list_of   list_off  seq_off   tok
    assert pool.dtype == np.int32 and pool.tolist() == [1, 2, 5, 0, 0, 0, 0, 0, 2, 0, 2, 5, 5, 6, 7, 8, 9]


def test_one_list_per_sentence_deduplicates_identical_lists():
    a, b = [[5, 6], [7, 8, 9]], [[1, 2]]
    singles, pool = engine.banned_sequence_tables(5, V, [a, None, b, [list(s) for s in a], [[3]]])
    assert singles == [None, None, None, None, [3]]
    L, S, T = pool[:3].tolist()
    assert (L, S, T) == (2, 3, 7) and pool[4:9].tolist() == [0, -1, 1, 0, -1]
    assert pool[9:12].tolist() == [0, 2, 3] and pool[12:16].tolist() == [0, 2, 5, 7] and pool[16:].tolist() == [5, 6, 7, 8, 9, 1, 2]
    # a duplicate inside a list is dropped; the same sequences in another order are another list
    _, pool = engine.banned_sequence_tables(2, V, [[[5, 6], [5, 6]], [[5, 6]]])
    assert pool[:3].tolist() == [1, 1, 2] and pool[4:6].tolist() == [0, 0]


def test_nothing_longer_than_one_token_gives_no_pool():
    assert engine.banned_sequence_tables(2, V, None) == ([None, None], None)
    assert engine.banned_sequence_tables(2, V, [[3], [4]]) == ([[3, 4], [3, 4]], None)
    assert engine.banned_sequence_tables(2, V, [None, []]) == ([None, None], None)


def test_malformed_values_are_named():
    for n, seqs, match in (
            (3, [[[1, 2]], None], "bad_sequences has 2 entries for 3 sentences"),
            (2, [[[1, 2]], [[3, "x"]]], r"sentence 1: sequence 0 must be a non-empty list of token ids"),
            (2, [[[1, 2], []], None], r"sentence 0: sequence 1 must be a non-empty list"),
            (1, [[1, V]], rf"sentence 0: sequence 0 holds token {V} outside \[0, {V}\)"),
            (1, [[1, 2], [-1, 2]], r"sentence 0: sequence 1 holds token -1 outside"),
            (1, [list(range(17))], "sentence 0: sequence 0 has 17 tokens, at most 16"),
            (2, [[[1, 2]], 7], "sentence 1: bad_sequences must be a list of id sequences or None, got int"),
            (1, 5, "bad_sequences must be a list"),
            (0, [[1, 2]], "banned sequences for 0 sentences")):
        with pytest.raises(ValueError, match=match):
            engine.banned_sequence_tables(n, V, seqs)
    many = [[i % V, (i // V) + 1, 3] for i in range(engine.SEQUENCE_MAX_SEQS + 1)]
    with pytest.raises(ValueError, match="at most 4096 sequences and 32768 tokens"):
        engine.banned_sequence_tables(1, V, many)


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def test_sequence_banned_equals_a_brute_force_restatement():
    g = np.random.RandomState(3)
    hit = 0
    for trial in range(300):
        t = int(g.randint(0, 12))
        hist = g.randint(0, 4, size=t).tolist()
        seqs = [g.randint(0, 4, size=int(g.randint(2, 6))).tolist() for _ in range(int(g.randint(0, 6)))]
        want = set()
        for c in range(4):
            for a in seqs:                                                  # appending c would complete an occurrence of `a` at the end
                m = len(a)
                if a[m - 1] == c and t >= m - 1 and all(hist[t - m + 1 + j] == a[j] for j in range(m - 1)):
                    want.add(c)
        assert sequence_banned(hist, seqs) == want, (hist, seqs)
        hit += bool(want)
    assert hit > 30                                                     # not vacuous: many of the random cases ban something


def test_wrap_step_takes_sequences_and_leaves_old_callers_alone():
    z = torch.zeros(4, 10)
    step = lambda tokens: z
    tokens = torch.tensor([[1, 2], [1, 3], [5, 2], [7, 7]])
    table = [[-1, 0, 0]] * 2
    assert torch.equal(wrap_step(step, [], table, 9, [1, 1])(tokens), z)
    out = wrap_step(step, [], table, 9, [1, 1], sequences=[[[2, 4], [1, 2, 6], [3, 5]]], list_of=[0, -1])(tokens)     # beams = 2
    want = z.clone()
    want[0, 4] = want[0, 6] = want[1, 5] = BANNED
    assert torch.equal(out, want)


# ---- the front end ----------------------------------------------------------------------------------------------------------------
class _SeqEngine(H._FakeEngine):
    def constrain(self, words, table, **kw):
        assert set(kw) <= {"sequences"}
        self._note("constrain", np.asarray(words).shape, [list(r) for r in table],
                   None if "sequences" not in kw else np.asarray(kw["sequences"]).tolist())


def _seq_model(kind="greedy"):
    m = _model(kind=kind)
    m.engine = _SeqEngine("ctx0", m.log)
    return m


def test_submit_passes_sequences_on_the_submitting_context(no_device):
    m = _seq_model()
    m.submit({"image": IMAGES}, {"bad_sequences": [[[5, 6]], None, [[5, 6], [9]]], "bad_tokens": [3]})
    name, stream, what, shape, table, pool = m.log[0]
    assert (name, stream, what, shape) == ("ctx0", "caller", "constrain", (2, 32)) and m.log[1][2] == "generate"
    assert table == [[0, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert pool == [1, 1, 2, 0, 0, -1, 0, 0, 1, 0, 2, 5, 6]
    words = m._constraints({"bad_sequences": [[[5, 6]], None, [[5, 6], [9]]], "bad_tokens": [3]}, 3)[0]
    assert np.flatnonzero(_bits(words[0])).tolist() == [3] and np.flatnonzero(_bits(words[1])).tolist() == [3, 9]


def test_sequences_alone_arm_an_empty_table(no_device):
    m = _seq_model()
    m.submit({"image": IMAGES}, {"bad_sequences": [[5, 6, 7]]})
    assert m.log[0][3:] == ((0, 32), [[-1, 0, 0]] * 3, [1, 1, 3, 0, 0, 0, 0, 0, 1, 0, 3, 5, 6, 7])


def test_num_return_sequences_replicates_list_of(no_device):
    m = _seq_model(kind="generator")
    m.submit({"image": IMAGES}, {"bad_sequences": [[[5, 6]], None, [[7, 8]]], "num_return_sequences": 2, "do_sample": True})
    pool = m.log[0][5]
    assert pool[:4] == [2, 2, 4, 0] and pool[4:10] == [0, 0, -1, -1, 1, 1] and len(m.log[0][4]) == 6
    assert pool[10:] == [0, 1, 2, 0, 2, 4, 5, 6, 7, 8]


def test_every_front_end_form_passes_sequences(no_device):
    m = _seq_model()
    sp = {"bad_sequences": [[1, 2]]}
    m.submit_answers(IMAGES, [[101, 7], [101, 8, 9]], image_of=[0, 2], search_param=sp)
    m.submit_answers(None, [[101, 7]], image_of=[1], search_param=sp)
    m.submit_ragged([torch.zeros(3, 16, 16), torch.zeros(3, 32, 16)], search_param=sp)
    first = m.submit({"image": IMAGES}, sp)
    m.submit_followup({"prefixes": [[101, 5], [101, 6]], "image_of": [2, 0]}, sp, on=first)
    arms = [e for e in m.log if e[2] == "constrain"]
    assert len(arms) == 5 and all(e[5] is not None and e[5][:3] == [1, 1, 2] for e in arms)
    assert [len(e[4]) for e in arms] == [2, 1, 2, 3, 2]


def test_without_the_new_keys_the_old_two_argument_call_is_made(no_device):
    m = _model()                    # test_constraints_host's fake engine: constrain(words, table) takes nothing else
    m.submit({"image": IMAGES}, H.SP)
    m.submit({"image": IMAGES}, {"bad_sequences": [[4]], "bad_phrases": None})          # one-token sequences are set bits
    assert [e[2] for e in m.log] == ["constrain", "generate", "constrain", "generate"] and m.log[0][4] == H.TABLE
    assert m.log[2][3:] == ((1, 32), [[0, 0, 0]] * 3)


def test_bad_phrases_go_through_the_tokenizer(no_device):
    m = _seq_model()
    pieces = {"cat": [201], "catapult": [201, 77], "hot dog stand": [301, 202, 303]}
    m.tokenizer = lambda w, add_special_tokens=False: {"input_ids": pieces[w]}
    m.submit({"image": IMAGES}, {"bad_phrases": ["catapult", "cat", "hot dog stand"], "bad_sequences": [[1, 2]], "bad_words": ["cat"]})
    assert m.log[0][5] == [1, 3, 7, 0, 0, 0, 0, 0, 3, 0, 2, 4, 7, 1, 2, 201, 77, 301, 202, 303]
    m.submit({"image": IMAGES}, {"bad_phrases": [["catapult"], None, ["cat"]]})
    assert m.log[2][4] == [[-1, 0, 0], [-1, 0, 0], [0, 0, 0]] and m.log[2][5][4:7] == [0, -1, -1]
    with pytest.raises(ValueError, match="'catapult' is 2 WordPieces"):                 # bad_words keeps its rule and its text
        m.submit({"image": IMAGES}, {"bad_words": ["catapult"]})
    with pytest.raises(ValueError, match="bad_phrases has 2 entries for 3 sentences"):
        m.submit({"image": IMAGES}, {"bad_phrases": [["cat"], None]})
    m.tokenizer = None
    with pytest.raises(ValueError, match="bad_phrases needs the model's tokenizer"):
        m.submit({"image": IMAGES}, {"bad_phrases": ["cat"]})


def test_trie_search_refuses_the_new_keys():
    m = object.__new__(M.CaptioningModel)
    m.decoder = type("D", (), {"kind": "trie"})()
    with pytest.raises(NotImplementedError, match="trie search"):
        m._constraints({"bad_sequences": [[1, 2]]}, 1)


# ---- the header -------------------------------------------------------------------------------------------------------------------
def test_header_keeps_abi_10_and_names_the_extension():
    hdr = open(os.path.join(ROOT, "include", "gitmi.h")).read()
    assert re.search(r"#define\s+GITMI_ABI_VERSION\s+10\b", hdr) and len(engine.EXPORTED_SYMBOLS) == 40
    assert sorted(set(re.findall(r"\b(gitmi_[a-z_0-9]+)\s*\(", hdr))) == sorted(engine.EXPORTED_SYMBOLS)
    text = " ".join(hdr.replace("*", " ").split())
    for phrase in ("search->reserved_ == 0 is the call above, exactly", "{ L, S, T, 0, list_of[Q], list_off[L + 1], seq_off[S + 1], tok[T] }",
                   "2 <= m <= 16", "x[t - m + 1 .. t) == a[0 .. m - 1)", "4096 sequences and 32768 tokens", "sent_out"):
        assert phrase in text, phrase
    exp = open(os.path.join(ROOT, "include", "gitmi_experiment.h")).read()
    assert "row_words_out" in exp and "pool_host" in exp
    assert engine.SEQUENCE_MAX_LEN == 16 and engine.SEQUENCE_MAX_SEQS == 4096 and engine.SEQUENCE_MAX_TOKENS == 32768
