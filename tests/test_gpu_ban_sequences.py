"""Banned token sequences in whole calls on the MI355X (search_param bad_sequences -> the extension of GITMI_SEARCH_CONSTRAIN)
against fixtures frozen from the reference search classes under tools/constrained_step.wrap_step
(tools/make_ban_sequences_golden.py): f32 row for row, the 16-bit builds through tools/parity.ids_parity with section 20's
thresholds, the rule itself on every returned row, and the arming behaviour -- one-shot, replays under other sequences, an
unarmed engine's plain ids, no stale sequences, refusals that leave arming and residency alone."""
import ast
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_constraints import _case, _params, _same
from tools.parity import F32_LOGIT_ABS, ids_parity, logit_bound

GOLDEN = ("banseq_tiny_greedy", "banseq_tiny_combined", "banseq_tiny_prefix", "banseq_tiny_beam4", "banseq_fullvocab")
# Regression guard, NOT a tolerance (as test_gpu_constraints.F16_BEAM_IDENTICAL_FLOOR): rows of the beam-4 fixture, frozen under the
# f32 certificate, that the 16-bit builds must return identical to the reference although no margin certifies them.  Measured
# on the MI355X: 4 of 4 in f16; the floor sits one row under the measurement, as section 20's does.
F16_BEAM_IDENTICAL_FLOOR = {"banseq_tiny_beam4": 3}


def _lists(pool, Q):
    """The pool of a fixture -> one entry per sentence: None or its list of sequences"""
    pool = [int(v) for v in pool]
    L, S, T = pool[:3]
    list_of, list_off = pool[4:4 + Q], pool[4 + Q:5 + Q + L]
    seq_off, tok = pool[5 + Q + L:6 + Q + L + S], pool[6 + Q + L + S:]
    assert len(tok) == T
    seqs = [tok[seq_off[j]:seq_off[j + 1]] for j in range(S)]
    return [None if l < 0 else seqs[list_off[l]:list_off[l + 1]] for l in list_of]


def _sp(g, vocab):
    sp = {"bad_sequences": _lists(g["pool"], int(g["batch"]))}
    if any(row != [-1, 0, 0] for row in g["table"].tolist()):
        sp.update(_params(g, vocab))
    return sp


def _golden_run(name, precision):
    g, cfg, model, batch = _case(name, precision)
    out = model(batch, _sp(g, cfg.vocab))
    preds, lps = out["predictions"].cpu().numpy(), out["logprobs"].cpu().numpy()
    model.close()
    return g, cfg, preds, lps


def _greedy(g):
    kind, _, k, _, _ = ast.literal_eval(str(g["search"]))
    return kind == "greedy" and k == 1


def _hist(ids, g, cfg):
    head = [int(t) for t in g["prefix"]] if g["prefix"].size else []
    return [head + (row[:row.index(cfg.eos) + 1] if cfg.eos in row else row) for row in np.asarray(ids).tolist()]


def _occurs_past(hist, seq, P):
    m = len(seq)
    return any(hist[i:i + m] == list(seq) for i in range(max(P - m + 1, 0), len(hist) - m + 1))


def _rule_holds(g, cfg, preds):
    P = int(g["prefix"].size) or 1
    for q, (hist, seqs) in enumerate(zip(_hist(preds, g, cfg), _lists(g["pool"], int(g["batch"])))):
        assert seqs is None or not any(_occurs_past(hist, s, P) for s in seqs), (q, hist, seqs)


@pytest.mark.parametrize("name", GOLDEN)
def test_fixture_conditions(name):
    """What the tool asserted when it froze the fixture: the plain ids contain a banned sequence past the prefix, the reference's
    constrained ids contain none, and the margins reach the bound the case was frozen under"""
    from test_gpu_constraints import _golden
    g, cfg, *_ = _golden(name)
    P = int(g["prefix"].size) or 1
    lists = _lists(g["pool"], int(g["batch"]))
    assert any(l is not None for l in lists)
    for hist, seqs in zip(_hist(g["predictions_plain"], g, cfg), lists):
        assert seqs is None or any(_occurs_past(hist, s, P) for s in seqs)
    _rule_holds(g, cfg, g["predictions"])
    span = float(g["logit_max"]) - float(g["logit_min"])
    assert float(g["step_margin"].min()) >= (2 * logit_bound("f16", span) if _greedy(g) else 10 * F32_LOGIT_ABS)
    if name == "banseq_tiny_prefix":
        assert all(s[0] == int(g["prefix"][-1]) for s in lists[0][:2])       # the sequence begins at the last prefix token
    if name == "banseq_fullvocab":
        assert cfg.vocab == 30522 and any(s[-1] == 30521 for s in lists[0]) and lists[1] is None
    if name == "banseq_tiny_combined":
        assert all(row[0] >= 0 and row[1] > 0 and row[2] == 2 for row in g["table"].tolist())


@pytest.mark.parametrize("name", GOLDEN)
def test_f32_ids_equal_the_reference(name):
    g, cfg, preds, lps = _golden_run(name, "f32")
    assert preds.shape == g["predictions"].shape and np.array_equal(preds, g["predictions"]), (preds, g["predictions"])
    assert np.allclose(lps.reshape(-1), g["logprobs"].reshape(-1), atol=1e-4), (lps, g["logprobs"])
    assert not np.array_equal(preds, g["predictions_plain"])
    _rule_holds(g, cfg, preds)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("name", GOLDEN)
def test_16_bit_ids(name, precision):
    """Section 20's thresholds: every row whose decision margins reach 2 x logit_bound("f16", span) (bf16: logit_bound("bf16",
    span)) equals the reference -- ids_parity raises otherwise; in f16 that is every row of the greedy fixtures.  The beam fixture's
    f16 rows are held to the measured floor.  The rule itself holds on every returned row whatever the precision."""
    g, cfg, preds, _ = _golden_run(name, precision)
    span = float(g["logit_max"]) - float(g["logit_min"])
    assert preds.shape == g["predictions"].shape
    thr = 2 * logit_bound("f16", span) if precision == "f16" else logit_bound("bf16", span)
    stats = ids_parity(preds, g["predictions"], g["step_margin"], thr, chained=not _greedy(g),
                       first_decision_pos=0 if g["prefix"].size else 1,
                       min_identical=F16_BEAM_IDENTICAL_FLOOR.get(name) if precision == "f16" else None)
    print(name, precision, "identical rows", stats["identical"], "of", stats["rows"], stats)
    if _greedy(g) and precision == "f16":
        assert stats["safe_rows"] == stats["identical"] == stats["rows"]
    _rule_holds(g, cfg, preds)

pytestmark = pytest.mark.gpu


def _rows(out, cfg):
    """returned id rows cut after the first [SEP]"""
    rows = []
    for row in out["predictions"].cpu().tolist():
        rows.append(row[:row.index(cfg.eos) + 1] if cfg.eos in row else row)
    return rows


def _occurs(row, seq):
    return any(row[i:i + len(seq)] == list(seq) for i in range(len(row) - len(seq) + 1))


def _choose(rows, cfg):
    """One list per sentence: the bigram of its plain ids behind the start token, its first trigram behind that, and a
    five-token sequence that cannot occur (its head is not in the row)"""
    per = []
    for q, row in enumerate(rows):
        body = [t for t in row if t != cfg.eos]
        if len(body) < 5:                                                   # a short sentence: its first two ids
            per.append([row[0:2]])
            continue
        per.append([body[1:3], body[2:5], [1, 2, 3, 4, 5]] if q % 2 == 0 else [body[0:2]])
    return per


@pytest.mark.parametrize("precision", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("name", ["constraints_tiny_greedy", "constraints_tiny_beam4"])
def test_banned_sequences_hold_on_every_returned_row(name, precision):
    g, cfg, model, batch = _case(name, precision)
    plain = model(batch)
    per = _choose(_rows(plain, cfg), cfg)
    armed = model(batch, {"bad_sequences": per})
    for q, row in enumerate(_rows(armed, cfg)):
        assert not any(_occurs(row, s) for s in per[q]), (q, row, per[q])
    assert all(any(_occurs(row, s) for s in per[q]) for q, row in enumerate(_rows(plain, cfg)))
    assert _same(model(batch), plain)                                    # one-shot: the next call runs plain, bit for bit
    assert _same(model(batch, {"bad_sequences": per}), armed)            # the same arming again: the same answer
    model.close()


@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_arming_replays_and_leaves_nothing_behind(precision):
    """Armed, plain, armed with other sequences of equal shape: the graphed engine returns what an engine without graphs returns
    for each -- the values live in the tables, not in the captured graph (a graph that had captured them would replay the first
    lists); the plain call equals an engine that was never armed; a set-only arming after a sequence arming equals the set-only
    answer of an engine that never saw sequences, and a banned sequence occurs in it."""
    g, cfg, model, batch = _case("banseq_tiny_greedy", precision)
    B = int(g["batch"])
    lists = _lists(g["pool"], B)
    sp1 = {"bad_sequences": lists}
    sp2 = {"bad_sequences": [lists[(q + 1) % B] for q in range(B)]}       # the same shape (one pool layout), other values
    first = [[int(r[1])] for r in g["predictions"].tolist()]                # the first generated token under sp1: bans change the row
    sp_set = {"bad_tokens": [[t[0]] if t[0] != cfg.eos else None for t in first]}
    _, _, fresh, _ = _case("banseq_tiny_greedy", precision)
    fresh.engine.set_graph(False)
    want_plain, want_set = fresh(batch), fresh(batch, sp_set)               # before this engine is ever armed with sequences
    want1, want2 = fresh(batch, sp1), fresh(batch, sp2)
    fresh.close()
    assert not _same(want1, want2) and not _same(want1, want_plain) and not _same(want_set, want1)
    got1, got_plain, got2 = model(batch, sp1), model(batch), model(batch, sp2)
    assert _same(got1, want1) and _same(got_plain, want_plain) and _same(got2, want2)
    assert _same(model(batch, sp_set), want_set)                            # no stale sequences
    assert _same(model(batch, sp1), want1) and _same(model(batch), want_plain)
    model.close()


def test_refused_pools_leave_arming_and_residency():
    """Every refusal of the extension comes before any launch: what was armed still fires, the resident images still answer"""
    from generativeimage2text_amd import engine as E
    g, cfg, model, batch = _case("banseq_tiny_greedy", "f32")
    eng, B = model.engine, int(g["batch"])
    pool = [int(v) for v in g["pool"]]
    table = [[-1, 0, 0]] * B
    greedy = E.Engine.make_search("greedy", 14, 1, 1)
    plain = model(batch)
    armed = model(batch, {"bad_sequences": _lists(g["pool"], B)})
    before = [t.cpu() for t in eng.generate(None, greedy)[:2]]
    L, S, T = pool[:3]
    o_list_of, o_list_off, o_seq_off, o_tok = 4, 4 + B, 5 + B + L, 6 + B + L + S

    def changed(i, v):
        p = list(pool)
        p[i] = v
        return p
    eng.constrain(None, table, sequences=pool)                              # armed; every refusal below must leave it so
    for bad, match in ((changed(0, B + 100), "sequence lists outside"),
                       (changed(1, 5000), "sequences above the cap of 4096"),
                       (changed(2, 40000), "sequence tokens above the cap of 32768"),
                       (pool + [0], "needs"),
                       (changed(3, 1), "needs"),
                       (changed(o_list_of + 1, L), rf"constrain: sentence 1: sequence list {L} outside \[-1,{L}\)"),
                       (changed(o_list_of, -2), "constrain: sentence 0: sequence list -2 outside"),
                       (changed(o_list_off, 1), "list offsets run from 1"),
                       (changed(o_list_off + 1, S + 1), "offsets decrease|has|sequence offsets|list offsets"),
                       (changed(o_seq_off + 1, 1), "list 0: sequence 0 has 1 tokens, outside \\[2,16\\]"),
                       (changed(o_seq_off + S, T - 1), "sequence offsets run"),
                       (changed(o_tok, cfg.vocab), rf"list 0: sequence 0 holds token {cfg.vocab} outside \[0,{cfg.vocab}\)"),
                       (changed(o_tok + T - 1, -1), "holds token -1 outside")):
        with pytest.raises(E.GitmiError, match=match):
            eng.constrain(None, table, sequences=bad)
    s = E.GitmiSearch()
    s.kind, s.reserved_ = E.SEARCH_CONSTRAIN, len(pool)
    tab = (C.c_int32 * (3 * B))(*[v for r in table for v in r])
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(E.GitmiError, match="sent_out is NULL"):
        eng._ck(eng.lib.gitmi_generate_prefixed(eng._h, None, 0, 0, None, 0, tab, None, B, C.byref(s), None, None, None, info.data_ptr(),
                                                int(torch.cuda.current_stream().cuda_stream)))
    with pytest.raises(E.GitmiError, match=rf"armed for {B} sentences, this call has 2"):
        eng.generate_prefixed(None, greedy, [[cfg.sos]] * 2, image_of=[0, 1])
    with pytest.raises(E.GitmiError, match="GITMI_SEARCH_TRIE while decoding constraints are armed"):
        eng.generate(None, E.Engine.make_search("trie", 14, 1, 1))
    with pytest.raises(E.GitmiError, match=rf"search_begin: decoding constraints are armed for {B} sentences"):
        eng.search_begin(greedy, torch.full((B, 1), cfg.sos), cfg.vocab)
    assert _same(model(batch), armed)                                       # still armed after all of them: this call consumes it
    now = [t.cpu() for t in eng.generate(None, greedy)[:2]]
    assert eng.resident == B and torch.equal(before[0], now[0]) and torch.equal(before[1], now[1]) and _same(model(batch), plain)
    model.close()
