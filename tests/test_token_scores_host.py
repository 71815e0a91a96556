"""Host side of the per-token trace (GITMI_SEARCH_TRACE): the search_param normaliser and the front end's arming, with a stub engine;
and the CPU restatement of the rule (tools/token_scores_rule.py) on a hand-made example and against a recording wrapper around the
oracle's search classes."""
import contextlib
import math
import types

import pytest
import torch

from generativeimage2text_amd import model as M
from oracle import git_oracle as O
from tools.token_scores_rule import check_sum, length_norm, records_of, simulate

EOS, V = 102, 1000


# ---- the normaliser ---------------------------------------------------------------------------------------------------------------
def test_defaults_ask_for_nothing():
    for sp in (None, {}, {"output_scores": False}, {"top_logprobs": 0}, {"top_logprobs": None}, {"do_sample": True, "top_k": 5}):
        assert M.trace_param(sp, "autoregressive") is None
        assert M.trace_param(sp, "trie") is None             # a trie request without the keys is not refused either


def test_keys_give_the_alternative_count():
    assert M.trace_param({"output_scores": True}, "autoregressive") == 0
    assert M.trace_param({"top_logprobs": 5}, "generator") == 5                      # above 0 implies output_scores
    assert M.trace_param({"output_scores": False, "top_logprobs": 8}, "generator") == 8
    assert M.trace_param({"output_scores": True, "do_sample": True}, "generator") == 0


@pytest.mark.parametrize("bad", [-1, 9, 2.5, "3", True])
def test_top_logprobs_range(bad):
    with pytest.raises(ValueError, match=r"top_logprobs .* outside \[0, 8\]"):
        M.trace_param({"top_logprobs": bad}, "autoregressive")


def test_refusals_name_the_combination():
    with pytest.raises(NotImplementedError, match="trie search"):
        M.trace_param({"output_scores": True}, "trie")
    with pytest.raises(NotImplementedError, match="top_logprobs with do_sample"):
        M.trace_param({"top_logprobs": 2, "do_sample": True}, "generator")


# ---- the front end arms the context it submits to ------------------------------------------------------------------------------------
class _FakeEngine:
    def __init__(self, log):
        self.log = log
        self.resident, self.generation = None, 0
        self.c = types.SimpleNamespace(max_batch=8, max_frames=1, max_text_len=10, patch=16)
        self.max_tokens, self.max_context = 17, 0

    def set_temporal_embedding(self, on):
        pass

    def check_finite(self, info):
        pass

    def ragged(self, images):
        return ("ragged", len(images))

    def trace(self, Q, nout=1, T=0, n=0, out_lp=None, out_tok=None, host_out=False):
        self.log.append(("trace", Q, nout, T, n))
        return "lp", ("tok" if n else None)

    def generate(self, frames, search, prefix=None, sync=True, host_out=False):
        self.log.append(("generate",))
        if frames is not None:
            self.resident, self.generation = 3, self.generation + 1
        return None, None, None

    def generate_prefixed(self, frames, search, prefixes, image_of=None, sync=True, host_out=False):
        self.log.append(("generate_prefixed", len(prefixes)))
        if frames is not None:
            self.resident, self.generation = 3, self.generation + 1
        return None, None, None, None


class _Cuda:
    @staticmethod
    def current_stream():
        return "caller"

    @staticmethod
    @contextlib.contextmanager
    def stream(s):
        yield

    class Event:
        def record(self):
            pass


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(M.torch, "cuda", _Cuda)


def _model(kind="greedy"):
    m = object.__new__(M.CaptioningModel)
    m.cfg = types.SimpleNamespace(num_frames=0, sos=101, eos=EOS, vocab=V)
    if kind == "greedy":
        m.decoder = M.AutoRegressiveBeamSearch(eos_index=EOS, max_steps=10, beam_size=1, per_node_beam_size=1, fix_missing_prefix=True)
    else:
        m.decoder = M.GeneratorWithBeamSearch(eos_index=EOS, max_steps=10, beam_size=2, per_node_beam_size=2, length_penalty=0.6)
    m.log = []
    m.engine, m._loaded, m.training = _FakeEngine(m.log), True, False
    return m


IMAGES = torch.zeros(3, 3, 8, 8)


def test_every_entry_point_arms_right_before_its_call(no_device):
    m = _model()
    m.submit({"image": IMAGES}, {"output_scores": True})
    m.submit_answers(IMAGES, [[101, 7]] * 2, image_of=[0, 1], search_param={"top_logprobs": 3})
    m.submit_followup({"prefixes": [[101, 7], [101, 8, 9]], "image_of": [0, 2]}, {"top_logprobs": 8})
    m.submit_ragged([torch.zeros(3, 16, 16), torch.zeros(3, 32, 16)], search_param={"output_scores": True, "top_logprobs": 1})
    assert m.log == [("trace", 3, 1, 10, 0), ("generate",), ("trace", 2, 1, 10, 3), ("generate_prefixed", 2),
                     ("trace", 2, 1, 10, 8), ("generate_prefixed", 2), ("trace", 2, 1, 10, 1), ("generate",)]


def test_replication_and_num_keep_best_size_the_trace(no_device):
    m = _model("beam")
    m.submit({"image": IMAGES[:2]}, {"top_logprobs": 2, "num_keep_best": 3, "num_return_sequences": 2})
    assert m.log == [("trace", 4, 3, 10, 2), ("generate_prefixed", 4)]


def test_without_the_keys_nothing_is_built_or_armed(no_device):
    m = _model()
    m.submit({"image": IMAGES})
    m.submit({"image": IMAGES}, {"output_scores": False, "top_logprobs": 0})
    m.submit_answers(IMAGES, [[101, 7]] * 2, image_of=[0, 1])
    assert m.log == [("generate",), ("generate",), ("generate_prefixed", 2)]


def test_results_are_cut_like_the_predictions():
    lp = torch.arange(2 * 6 * 3, dtype=torch.float32).reshape(2, 6, 3)
    tok = torch.arange(2 * 6 * 2).reshape(2, 6, 2)
    # per-sentence prefixes of 2 and 3 tokens, returned lengths 5 and 4 (autoregressive): positions [2, 5) and [3, 4)
    spans = M.trace_spans(2, 1, 6, [[5, 0], [4, 0]], [2, 3], "autoregressive")
    assert spans == [(2, 5), (3, 4)]
    out = M.format_trace((lp, tok), spans)
    assert out["token_logprobs"] == [[6.0, 9.0, 12.0], [27.0]]
    assert out["top_tokens"][1] == [[18, 19]] and out["top_logprobs"][0][0] == [7.0, 8.0]
    # batch-uniform: no prefix removes nothing ([CLS] stays, its lp is 0 by the rule); generator keeps all T positions per hypothesis
    assert M.trace_spans(2, 1, 6, [4, 0], None, "autoregressive") == [(0, 4), (0, 4)]
    assert M.trace_spans(1, 3, 6, [6, 0], 2, "generator") == [(2, 6)] * 3
    assert M.trace_spans(1, 1, 6, [2, 1], None, "autoregressive") == [(1, 2)]       # the early-[SEP] return
    assert "top_tokens" not in M.format_trace((lp, None), spans)


# ---- the rule on the CPU ---------------------------------------------------------------------------------------------------------------
def _lse(*xs):
    return math.log(sum(math.exp(x) for x in xs))


def test_hand_made_three_steps_with_a_tie_and_an_ended_beam():
    """V = 4, [SEP] = 3, prefix [2], beam 2 x 2, T = 4.
    step 1 (row 0 alone): logits [1, 1, 0, -5] -- tokens 0 and 1 tie, the lower id leads: beams [2, 0], [2, 1], both at a.
    step 2: row 0 [0, 0, 0, 6] with its last token 0 at -10000 -> [SEP] at c; row 1 [0, 9, 0, 0] with token 1 at -10000 -> 0, 2, 3 tie
            at -log 3.  Kept: (row 0, [SEP]) and, of the tied (row 1, 0) and (row 1, 2), the earlier candidate.
    step 3: row 0 has ended -> one-hot [SEP] at log-prob 0, everything else -inf; row 1 [0, 0, 4, 0] -> token 2 at d."""
    inf = float("-inf")
    xs = {1: torch.tensor([[1.0, 1, 0, -5], [0, 0, 0, 0]]), 2: torch.tensor([[0.0, 0, 0, 6], [0, 9, 0, 0]]),
          3: torch.tensor([[9.0, 9, 9, -9], [0, 0, 4, 0]])}
    a = 1.0 - _lse(1, 1, 0, -5)
    c = 6.0 - _lse(-10000, 0, 0, 6)
    tr = simulate("autoregressive", lambda t: xs[t], [[2]], 2, 2, 4, 3, 2)
    assert tr.tokens == [[2, 0, 3, 3]] and tr.length == [4]
    assert tr.lp[0] == pytest.approx([0.0, a, c, 0.0], abs=1e-12) and tr.lp[0][3] == 0.0
    assert tr.alt_tok[0] == [[-1, -1], [0, 1], [3, 1], [3, -1]]
    assert tr.alt_lp[0][1] == pytest.approx([a, a], abs=1e-12) and tr.alt_lp[0][1][0] == tr.alt_lp[0][1][1]
    assert tr.alt_lp[0][2] == pytest.approx([c, 0.0 - _lse(-10000, 0, 0, 6)], abs=1e-12)
    assert tr.alt_lp[0][3] == [0.0, inf]
    assert tr.logprob[0] == pytest.approx((a + c) / 2, abs=1e-6)                     # num_valid: tokens 0 and [SEP]
    assert check_sum(tr.lp[0], tr.logprob[0], 2, 4) is None
    assert check_sum(tr.lp[0], tr.logprob[0] + 1e-3, 2, 4) is not None


def _recorded(search, xs, k, **kw):
    """the oracle's search class over scripted logits (row b * k + j at the step that appends position t), its step calls recorded"""
    calls = []

    def step(tokens):
        t = tokens.shape[1]
        lg = xs[t][::k] if tokens.shape[0] * k == xs[t].shape[0] and search is O.search_autoregressive and t == 1 else xs[t]
        calls.append((tokens.clone(), lg.clone()))
        return lg.clone()

    return search(torch.full((xs[1].shape[0] // k, 1), 7, dtype=torch.int64), step, **kw), calls


@pytest.mark.parametrize("kind", ["autoregressive", "generator"])
def test_both_forms_of_the_rule_agree_with_the_oracle_search(kind):
    """simulate() (beams carry their records) and records_of() (records looked up in the recorded step calls of the oracle's own
    search) give the same trace, and the oracle's ids and log-probs are simulate()'s."""
    B, k, pn, Vs, T, eos, n = 2, 3, 2, 40, 7, 5, 4
    g = torch.Generator().manual_seed(3)
    xs = {t: 2.0 * torch.randn(B * k, Vs, generator=g) for t in range(1, T)}
    for t in xs:
        xs[t][:, eos] += 1.0 if kind == "generator" else 0.5 * t
    if kind == "autoregressive":
        (ids, lps), calls = _recorded(O.search_autoregressive, xs, k, eos=eos, max_steps=T, beam_size=k, per_node_beam_size=pn)
        tr = simulate(kind, lambda t: xs[t], [[7]] * B, k, pn, T, eos, n)
        nh, rp = 1, 1.0
        ids = ids[:, None, :]
    else:
        nh, rp = 2, 1.2
        (ids, lps), calls = _recorded(O.search_generator, xs, k, eos=eos, max_steps=T, beam_size=k, per_node_beam_size=pn,
                                      length_penalty=0.6, repetition_penalty=rp, num_keep_best=nh)
        tr = simulate(kind, lambda t: xs[t], [[7]] * B, k, pn, T, eos, n, num_keep_best=nh, length_penalty=0.6, repetition_penalty=rp,
                      prefixed=False)
    assert tr.margin > 1e-4
    for b in range(B):
        for i in range(nh):
            o = b * nh + i
            seq = ids[b, i].tolist()
            assert seq + [eos] * (T - len(seq)) == tr.tokens[o]
            assert float(lps.reshape(B, nh)[b, i]) == pytest.approx(tr.logprob[o], abs=1e-5)
            n_h = tr.length[o]
            # generator: position n_h is the finishing candidate -- [SEP] itself unless the step budget ended the hypothesis
            end = n_h if kind == "autoregressive" else (n_h + 1 if n_h + 1 < T else n_h)
            recs = records_of(kind, calls, tr.tokens[o], 1, end, n, eos, rp, sentence=b, sentences=B)
            for s, (lp, at, al) in zip(range(1, end), recs):
                assert lp == pytest.approx(tr.lp[o][s], abs=1e-12) and at == tr.alt_tok[o][s]
                assert al == pytest.approx(tr.alt_lp[o][s], abs=1e-12)
            div = length_norm(n_h, 0.6) if kind == "generator" else \
                max(1, sum(t != eos for t in seq) + (1 if eos in seq else 0) - 1)
            assert check_sum(tr.lp[o], tr.logprob[o], div, T) is None


def test_spans_cut_what_format_predictions_cuts():
    """trace_spans restates format_predictions' rule: on tokens that carry their own position the two must keep the same positions"""
    T = 7
    tokens = torch.arange(T).repeat(3, 1)                    # tokens[q][s] == s
    for kind in ("autoregressive", "generator"):
        for sent in ([5, 0], [2, 1]):
            for prefix in (None, 1, 2):
                if sent[1] and kind == "generator":
                    continue
                preds, _ = M.format_predictions(tokens, torch.zeros(3), sent, prefix, kind)
                spans = M.trace_spans(3, 1, T, sent, prefix, kind)
                assert [list(range(a, b)) for a, b in spans] == preds.tolist(), (kind, sent, prefix)
        plens = [1, 2, 3]
        sent = [[5, 0], [3, 1 if kind == "autoregressive" else 0], [6, 0]]
        preds, _ = M.format_predictions(tokens, torch.zeros(3), sent, plens, kind)
        assert [list(range(a, b)) for a, b in M.trace_spans(3, 1, T, sent, plens, kind)] == preds, (kind,)
