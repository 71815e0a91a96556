"""Op-level tests of the per-token trace (GITMI_SEARCH_TRACE) through the step seam: scripted fp32 logits drive the engine's search
(f32 mode, measurement build for per-sentence prefixes) and tools/token_scores_rule.simulate, the fp64 restatement of the rule in
which every beam carries its own records.  The engine's log -- one record per new row per step, read back through the K/V row
indirection -- must give the same numbers: tokens and alternative tokens exactly, values within tools/parity.F32_LOGIT_ABS.

TINY engine, B = 3 sentences with prefixes of 1, 3 and 2 tokens, T = 8, vocab 1000, k in {1, 4}.  The scripts plant exact ties
inside a row, [SEP] at different steps per beam (one-hot rows follow), a sentence that is done early (padding rows), hypotheses
that finish at cur_len + 1 == T, num_keep_best = 3 with slots replaced mid-search and a list that stays unfilled.  (One slot
refilled twice in ONE step needs candidates that are not in descending order, which only the sampling branch produces; the
greedy-beam branch scripted here cannot reach it.)"""
import dataclasses
import math

import pytest
import torch

from oracle import git_oracle as O
from tools.parity import F32_LOGIT_ABS
from tools.token_scores_rule import check_sum, length_norm, simulate

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("experiment_build")]

V, T, B = 1000, 8, 3
EOS, SOS = 102, 101
PREFIXES = [[SOS], [SOS, 5, 6], [SOS, 7]]
MIN_MARGIN = 10.0 * F32_LOGIT_ABS         # decisions of the scripts tolerate ten times the value bound

_ENGINE = []


@pytest.fixture(scope="module", autouse=True)
def _close_engine():
    yield
    for e in _ENGINE:
        e.close()
    _ENGINE.clear()


@pytest.fixture
def eng():
    """the module's f32 engine, created by the first test that needs it (inside the measurement build's fixture)"""
    if not _ENGINE:
        from generativeimage2text_amd.engine import Engine
        cfg = dataclasses.replace(O.CONFIGS["TINY"], vocab=V)
        assert cfg.eos == EOS and cfg.sos == SOS
        e = Engine(cfg, precision="f32", max_batch=4, max_beams=4, max_frames=1, max_text_len=T)
        e.load_state_dict(O.make_weights(cfg, seed=3))
        _ENGINE.append(e)
    return _ENGINE[0]


def _script(seed, k, plants):
    """logits[cur_len] fp32 [B * k, V] for cur_len in 1 .. T - 1: N(0, 2) noise with [SEP] at -9, then the plants:
    ("set", cur_len, row, token, value) and ("tie", cur_len, row, [tokens]) = the tokens share the row's maximum + 1.5."""
    g = torch.Generator().manual_seed(seed)
    xs = {c: 2.0 * torch.randn(B * k, V, generator=g) for c in range(1, T)}
    for x in xs.values():
        x[:, EOS] = -9.0
    for p in plants:
        if p[0] == "set":
            xs[p[1]][p[2], p[3]] = p[4]
        else:
            x = xs[p[1]][p[2]]
            x[p[3]] = float(x.max()) + 1.5
    return xs


# name: (kind, k, pn, num_keep_best, repetition_penalty, length_penalty, seed, plants)
CASES = {
    # sentence 0 ties its first pick (30 before 40), ends at position 3; sentence 1 ends at 5; sentence 2 never ends
    "greedy": ("autoregressive", 1, 1, 1, 1.0, 1.0, 11,
               [("tie", 1, 0, [40, 30]), ("set", 3, 0, EOS, 30.0), ("set", 5, 1, EOS, 30.0), ("tie", 4, 2, [900, 17, 450])]),
    # beams of a sentence end at different steps: [SEP] on single rows
    "ar_beam4": ("autoregressive", 4, 2, 1, 1.0, 1.0, 12,
                 [("tie", 1, 0, [40, 30, 20, 10, 50]), ("set", 2, 0, EOS, 12.0), ("set", 3, 1, EOS, 12.0), ("set", 4, 2, EOS, 14.0),
                  ("set", 4, 3, EOS, 14.0), ("set", 5, 0, EOS, 14.0), ("set", 5, 1, EOS, 14.0), ("set", 5, 2, EOS, 14.0),
                  ("set", 5, 3, EOS, 14.0), ("set", 4, 4, EOS, 9.0), ("tie", 3, 8, [7, 3]), ("set", 6, 9, EOS, 11.0)]),
    # sentence 0: [SEP] likely from its first steps on -> three hypotheses, then done (padding rows) while the others go on;
    # sentence 1: [SEP] candidates at steps 4 and 6 replace slots; sentence 2 finishes at cur_len + 1 == T alone
    "gen_beam4_keep3": ("generator", 4, 2, 3, 1.3, 0.6, 20,
                        [("set", 1, 0, EOS, 9.0), ("set", 2, 0, EOS, 9.0), ("set", 2, 1, EOS, 9.0), ("set", 2, 2, EOS, 8.0),
                         ("set", 3, 0, EOS, 9.0), ("set", 3, 1, EOS, 9.0),
                         ("set", 4, 4, EOS, 5.0), ("set", 4, 5, EOS, 5.5), ("set", 5, 4, EOS, 6.0), ("set", 6, 4, EOS, 9.0),
                         ("set", 6, 5, EOS, 9.0), ("set", 6, 6, EOS, 9.0), ("tie", 3, 8, [7, 3])]),
    # one beam, two candidates per step: the list of three can hold at most two hypotheses at T - 1 -> an unfilled slot;
    # sentence 1 gets one from an early [SEP] candidate
    "gen_beam1_keep3": ("generator", 1, 2, 3, 1.0, 1.0, 14, [("set", 4, 1, EOS, 7.0), ("tie", 1, 0, [40, 30])]),
}
NS = {"greedy": (0, 1, 5, 8), "ar_beam4": (0, 5, 8), "gen_beam4_keep3": (0, 5, 8), "gen_beam1_keep3": (1, 5)}

_SIM = {}


def _expected(name, n):
    kind, k, pn, nh, rp, alpha, seed, plants = CASES[name]
    if (name, n) not in _SIM:
        xs = _script(seed, k, plants)
        _SIM[name, n] = simulate(kind, lambda c: xs[c], PREFIXES, k, pn, T, EOS, n, num_keep_best=nh, length_penalty=alpha,
                                 repetition_penalty=rp)
    return _SIM[name, n]


def _run(eng, name, n, traced=True):
    from generativeimage2text_amd.engine import Engine
    kind, k, pn, nh, rp, alpha, seed, plants = CASES[name]
    xs = _script(seed, k, plants)
    s = Engine.make_search(kind if kind == "autoregressive" else "beam", T, k, pn, alpha, repetition_penalty=rp, num_keep_best=nh)
    lp = tok = None
    if traced:
        lp, tok = eng.trace(B, nh, T, n)
    eng.debug_search_begin_prefixed(s, PREFIXES, V)
    for c in range(min(len(p) for p in PREFIXES), T):
        eng.search_advance(xs[c])
    tokens, logprobs, _ = eng.search_finish()
    return tokens.cpu().reshape(B * nh, T), logprobs.cpu().reshape(B * nh), (lp.cpu() if traced else None), (tok.cpu() if tok is not None else None)


def _close(a, b):
    if a == b:                              # also -inf == -inf
        return True
    return math.isfinite(a) and math.isfinite(b) and abs(a - b) <= F32_LOGIT_ABS


@pytest.mark.parametrize("name,n", [(name, n) for name in CASES for n in NS[name]])
def test_trace_equals_the_rule(eng, name, n):
    kind, k, pn, nh, rp, alpha, seed, plants = CASES[name]
    ref = _expected(name, n)
    print(f"{name} n={n}: smallest decision margin of the script {ref.margin:.3e}")
    assert ref.margin >= MIN_MARGIN, "the script's own decisions are too close for an fp32 engine"
    tokens, logprobs, lp, tok = _run(eng, name, n)
    assert lp.shape == (B * nh, T, 1 + n) and (n == 0 or tok.shape == (B * nh, T, n))
    assert tokens.tolist() == ref.tokens
    worst = 0.0
    for o in range(B * nh):
        P = len(PREFIXES[o // nh])
        assert abs(float(logprobs[o]) - ref.logprob[o]) <= F32_LOGIT_ABS * max(1.0, abs(ref.logprob[o]))
        for s in range(T):
            got, want = float(lp[o, s, 0]), ref.lp[o][s]
            assert _close(got, want), (o, s, got, want)
            worst = max(worst, abs(got - want))
            if n:
                assert tok[o, s].tolist() == ref.alt_tok[o][s], (o, s)
                for j in range(n):
                    assert _close(float(lp[o, s, 1 + j]), ref.alt_lp[o][s][j]), (o, s, j)
            if s < P:
                assert got == 0.0 and (n == 0 or tok[o, s].tolist() == [-1] * n)
    print(f"{name} n={n}: largest |lp - fp64 rule| {worst:.2e}")
    # the script reaches what it is meant to reach
    if name == "greedy":
        assert ref.length[0] < ref.length[1] < T and ref.length[2] == T            # sentences end at different steps, one never
    if name == "ar_beam4":
        assert ref.length[0] < T and ref.length[1] == T                             # every beam of sentence 0 ends, not of sentence 1
        end = ref.tokens[1].index(EOS)                                              # whose best beam ends early: forced [SEP]s at lp 0
        assert end < T - 2 and ref.lp[1][end] < 0.0 and all(v == 0.0 for v in ref.lp[1][end + 1:])
        assert n == 0 or ref.alt_tok[1][end + 1] == [EOS] + [-1] * (n - 1)
    if name == "greedy" and n >= 2:
        assert ref.alt_tok[0][1][:2] == [30, 40] and ref.alt_lp[0][1][0] == ref.alt_lp[0][1][1]        # the tie, lower id first
    if name == "gen_beam4_keep3":
        assert all(ref.length[o] > 0 for o in range(B * nh))
        assert max(ref.length[0:3]) < 5 and ref.length[6] == T - 1                  # done early | finished by the step budget
    if name == "gen_beam1_keep3":
        assert ref.length[2] == 0 and ref.logprob[2] == -1e5                        # the unfilled slot
        assert lp[2].abs().sum() == 0 and bool((tok[2] == -1).all())


@pytest.mark.parametrize("name,n", [("greedy", 5), ("ar_beam4", 8), ("gen_beam4_keep3", 5), ("gen_beam1_keep3", 5)])
def test_invariants_and_plain_twin(eng, name, n):
    """Sum: the traced lps add up to logprob_out (x num_valid, or x len_norm(n_h)).  Alternatives: a chosen token that ranks below n
    is among them with the bit-identical lp; in greedy the first alternative IS the emitted token.  And the traced search returns
    bit for bit what the plain one returns."""
    kind, k, pn, nh, rp, alpha, seed, plants = CASES[name]
    tokens, logprobs, lp, tok = _run(eng, name, n)
    ptokens, plogprobs, _, _ = _run(eng, name, n, traced=False)
    assert torch.equal(tokens, ptokens) and torch.equal(logprobs, plogprobs)
    checked = 0
    for o in range(B * nh):
        P = len(PREFIXES[o // nh])
        row = tokens[o].tolist()
        if kind == "autoregressive":
            L = _expected(name, n).length[o]
            seq = row[:L]
            div = max(1, sum(t != EOS for t in seq) + (1 if EOS in seq else 0) - P)
            end = L
        else:
            if float(logprobs[o]) == -1e5:
                assert lp[o].abs().sum() == 0
                continue
            n_h = _expected(name, n).length[o]
            div, end = length_norm(n_h, alpha), n_h + 1
        assert float(lp[o, end:, 0].abs().sum()) == 0.0 and float(lp[o, :P, 0].abs().sum()) == 0.0
        err = check_sum(lp[o, :, 0].tolist(), float(logprobs[o]), div, T)
        assert err is None, (o, err)
        for s in range(P, min(end, T)):
            emitted = row[s] if (kind == "autoregressive" or s < end - 1) else None     # position n_h: the candidate that finished it
            alts = tok[o, s].tolist()
            if emitted is not None and emitted in alts:
                assert float(lp[o, s, 1 + alts.index(emitted)]) == float(lp[o, s, 0]), (o, s)
                checked += 1
            if k == 1 and kind == "autoregressive":
                assert alts[0] == emitted, (o, s)
            vals = lp[o, s, 1:].tolist()
            assert all(a >= b for a, b in zip(vals, vals[1:])), (o, s, vals)
    assert checked > 0


def test_arming_is_one_shot_and_refusals_keep_it(eng):
    from generativeimage2text_amd.engine import Engine, GitmiError
    s = Engine.make_search("autoregressive", T, 1, 1)
    start = torch.full((B, 1), SOS, dtype=torch.int64)
    lp, tok = eng.trace(B, 1, T, 2)
    lp.fill_(7.0)
    with pytest.raises(GitmiError, match=r"armed for 3 sentences, this call has 2"):
        eng.search_begin(s, start[:2], V)
    with pytest.raises(GitmiError, match=r"armed for max_steps 8, this call has 6"):
        eng.search_begin(Engine.make_search("autoregressive", 6, 1, 1), start, V)
    with pytest.raises(GitmiError, match=r"GITMI_SEARCH_TRACE is not a search"):
        t = Engine.make_search("autoregressive", T, 1, 1)
        t.kind = 11
        eng.search_begin(t, start, V)
    with pytest.raises(GitmiError, match=r"search->reserved_ = 9 alternatives outside \[0,8\]"):
        bad = Engine.make_search("autoregressive", T, 1, 1)
        bad.kind, bad.reserved_ = 11, 9
        eng._ck(eng.lib.gitmi_generate_prefixed(eng._h, None, 0, 0, None, 0, None, None, B, bad, None, lp.data_ptr(), None, None, None))
    xs = _script(5, 1, [])
    for traced in (True, False):            # the refused calls left it armed: the first search is traced, the second is not
        eng.search_begin(s, start, V)
        for c in range(1, T):
            eng.search_advance(xs[c])
        eng.search_finish()
        if traced:
            first = lp.clone()
            assert float(first[:, 0].abs().sum()) == 0.0 and float(first[:, 1:, 0].max()) < 0.0
            lp.fill_(7.0)
    assert bool((lp == 7.0).all())
