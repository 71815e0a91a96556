"""Per-sentence decoding constraints on the MI355X (GITMI_SEARCH_CONSTRAIN: banned tokens, a minimum length, no repeated n-grams)
against fixtures frozen from the reference search classes under tools/constrained_step.wrap_step
(tools/make_constraints_golden.py): ids in the three precisions, the rules themselves on every returned row, per-sentence
independence, one-shot arming, sampling, residency and captured graphs, and the calls that are refused.

What the suite asserts is what a fixture certifies.  The greedy fixtures (constraints_tiny_greedy, constraints_fullvocab) were
frozen with every decision margin >= 2 x logit_bound("f16", span): the fp16 build must return every row.  The two beam-4
fixtures could not be frozen under that bound (a beam step ranks 2k + 1 = 9 near-equal sums; DESIGN section 20 has the seed
survey), they carry the f32 certificate (10 x F32_LOGIT_ABS): f32 must return every row, and in the 16-bit builds a row is
held to the reference only where its own margins reach the threshold (tools/parity.ids_parity) -- on these fixtures none does,
so their f16 identical rows are held to a measured floor (F16_BEAM_IDENTICAL_FLOOR, a regression guard like parity.py's
WIDE_BEAM_FLOOR) and their bf16 count is printed, as the issue asks.  Also gated on them in every precision: the rules themselves on
every returned row (test_returned_rows_keep_their_rules), one-shot arming, residency and the refusals."""
import ast
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from conftest import load_golden
from tools.constrained_step import ngram_banned, set_mask
from tools.parity import F32_LOGIT_ABS, ids_parity, logit_bound

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16", "bf16")
CASES = ("constraints_tiny_greedy", "constraints_tiny_beam4", "constraints_tiny_prefix_beam4", "constraints_fullvocab")
_cache = {}


def _golden(name):
    """-> (fixture, cfg, weights, frames, search, prefix), rebuilt once from the recorded seeds and shared (read-only)"""
    if name not in _cache:
        from oracle import git_oracle as O
        g = load_golden(name)
        cfg = dataclasses.replace(O.CONFIGS[str(g["config"])], vocab=int(g["vocab"]))
        kind, max_steps, k, pn, lp = ast.literal_eval(str(g["search"]))
        w = O.make_weights(cfg, **ast.literal_eval(str(g["weights_kw"])))
        frames = O.make_images(cfg, int(g["batch"]), 1, seed=int(g["image_seed"]))
        prefix = torch.tensor(g["prefix"], dtype=torch.long)[None] if g["prefix"].size else None
        _cache[name] = (g, cfg, w, frames, O.SearchConfig(kind, max_steps, k, pn, lp), prefix)
    return _cache[name]


def _decoder(cfg, search):
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, GeneratorWithBeamSearch
    if search.kind == "greedy":
        return AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=search.max_steps, beam_size=search.beam_size,
                                        per_node_beam_size=search.per_node_beam_size, fix_missing_prefix=True)
    return GeneratorWithBeamSearch(eos_index=cfg.eos, max_steps=search.max_steps, beam_size=search.beam_size,
                                   per_node_beam_size=search.per_node_beam_size, length_penalty=search.length_penalty)


def _params(g, vocab, rows=None):
    """The fixture's sets and table as the front end's search_param keys (rows: use these table rows instead)"""
    table = g["table"].tolist() if rows is None else rows
    bad = [None if s < 0 else np.flatnonzero(set_mask(g["sets"][s], vocab).numpy()).tolist() for s, _, _ in table]
    return {"bad_tokens": bad, "min_new_tokens": [r[1] for r in table], "no_repeat_ngram_size": [r[2] for r in table]}


def _case(name, precision="f32", search=None):
    """-> (fixture, cfg, model, batch)"""
    from generativeimage2text_amd.model import CaptioningModel
    g, cfg, w, frames, gsearch, prefix = _golden(name)
    model = CaptioningModel(cfg, _decoder(cfg, search or gsearch), precision=precision, max_batch=int(g["batch"]), max_frames=1,
                            max_text_len=gsearch.max_steps)
    model.load_state_dict(w)
    batch = {"image": frames[0].cuda()}
    if prefix is not None:
        batch["prefix"] = prefix.cuda()
    return g, cfg, model, batch


def _same(a, b):
    return a["predictions"].shape == b["predictions"].shape and torch.equal(a["predictions"].cpu(), b["predictions"].cpu()) and \
        torch.equal(a["logprobs"].cpu(), b["logprobs"].cpu())


def _histories(ids, g, cfg):
    """Returned id rows -> [(the sentence's ids with its start tokens, cut after the first [SEP]; ended)]"""
    head = [int(t) for t in g["prefix"]] if g["prefix"].size else []
    out = []
    for row in np.asarray(ids).tolist():
        ended = cfg.eos in row
        out.append((head + (row[:row.index(cfg.eos) + 1] if ended else row), ended))
    return out


def _broken(row_of_table, sets, hist, ended, P, cfg):
    set_index, min_new, n = (int(v) for v in row_of_table)
    body, out = hist[P:], set()
    if set_index >= 0:
        mask = set_mask(sets[set_index], cfg.vocab)
        if any(bool(mask[t]) for t in body):
            out.add("set")
    if ended and len(body) - 1 < min_new:
        out.add("len")
    if n > 0 and any(hist[t] in ngram_banned(hist[:t], n) for t in range(P, len(hist))):
        out.add("ngram")
    return out


def _plen(g):
    return int(g["prefix"].size) or 1


def _run(name, precision):
    g, cfg, model, batch = _case(name, precision)
    out = model(batch, _params(g, cfg.vocab))
    preds, lps = out["predictions"].cpu().numpy(), out["logprobs"].cpu().numpy()
    model.close()
    return g, cfg, preds, lps


def _parity(g, preds, thr):
    kind, _, k, _, _ = ast.literal_eval(str(g["search"]))
    assert preds.shape == g["predictions"].shape, (preds.shape, g["predictions"].shape)
    return ids_parity(preds, g["predictions"], g["step_margin"], thr, chained=not (kind == "greedy" and k == 1),
                      first_decision_pos=0 if g["prefix"].size else 1)


def _greedy(g):
    kind, _, k, _, _ = ast.literal_eval(str(g["search"]))
    return kind == "greedy" and k == 1


# ---- the fixtures say what the tool asserted when it froze them ------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_conditions(name):
    g, cfg, *_ = _golden(name)
    P, table, kinds = _plen(g), g["table"].tolist(), [str(k) for k in g["kinds"]]
    got, was = _histories(g["predictions"], g, cfg), _histories(g["predictions_plain"], g, cfg)
    active = set()
    for q, row in enumerate(table):
        if row == [-1, 0, 0]:
            continue
        broken = _broken(row, g["sets"], *was[q], P, cfg)
        assert broken, (q, row, was[q])                          # an engine that ignores the constraint returns the plain ids
        assert not _broken(row, g["sets"], *got[q], P, cfg)
        active |= broken
    if len(table) == 4:
        assert sorted(kinds) == ["all", "len", "ngram", "set"] and active == {"set", "len", "ngram"}
    span = float(g["logit_max"]) - float(g["logit_min"])
    if _greedy(g):
        assert float(g["step_margin"].min()) >= 2 * logit_bound("f16", span)
    else:
        assert float(g["step_margin"].min()) >= 10 * F32_LOGIT_ABS
    if name == "constraints_tiny_greedy":
        lens = [len(h) for h, _ in got]
        assert any(table[q][2] > 0 and got[q][1] and max(lens) - lens[q] >= 3 for q in range(4))      # forced [SEP] under an n-gram rule
    if name == "constraints_fullvocab":
        assert cfg.vocab == 30522 and [-1, 0, 0] in table
        bits = np.unpackbits(g["sets"][0].view(np.uint8), bitorder="little")
        assert bits[[0, 127, 128, 30521]].all() and bits[30522:30528].all()          # the last six must be ignored
        plain = was[[r[0] for r in table].index(0)][0]
        assert bits[plain[1]] and bits[plain[2]]                                     # the plain argmax of the first two steps


# ---- 1. f32: the reference's ids, row for row --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_f32_ids_equal_the_reference(name):
    g, cfg, preds, lps = _run(name, "f32")
    stats = _parity(g, preds, 10 * F32_LOGIT_ABS)
    print(name, stats)
    assert stats["identical"] == stats["rows"] == g["predictions"].shape[0]
    assert np.allclose(lps.reshape(-1), g["logprobs"].reshape(-1), atol=1e-4), (lps, g["logprobs"])
    got, was = _histories(preds, g, cfg), _histories(g["predictions_plain"], g, cfg)
    for q, row in enumerate(g["table"].tolist()):
        if row != [-1, 0, 0]:
            assert got[q][0] != was[q][0], (q, got[q], was[q])


# ---- 2. / 3. the 16-bit builds -------------------------------------------------------------------------------------------------------------
# Regression guard, NOT a tolerance (the way tools/parity.py's WIDE_BEAM_FLOOR is one): rows of the beam-4 fixtures that the fp16
# build must return identical to the reference although no margin certifies them.  Measured on the MI355X: 4 of 4
# (constraints_tiny_beam4) and 1 of 1 (constraints_tiny_prefix_beam4) in every run so far, f16 and bf16 alike.  The four-row floor
# sits one row under the measurement (a re-ordered fp32 sum may move one near-tie row: margins down to 0.0015 against an fp16 logit
# bound of 0.0069); a one-row fixture has no room under it.  This is where the f16 ids of a whole constrained beam call meet the
# reference's; its kernel -- vocab_topm_kernel<8, VOC_GENERIC, 0, BAN> -- and the other BAN instantiations meet an fp64 reference
# launch by launch in tests/test_gpu_constraints_ops.py.
F16_BEAM_IDENTICAL_FLOOR = {"constraints_tiny_beam4": 3, "constraints_tiny_prefix_beam4": 1}


@pytest.mark.parametrize("name", CASES)
def test_f16_ids(name):
    """Every row whose decision margins all reach 2 x logit_bound("f16", span) equals the reference (ids_parity raises otherwise):
    that is every row of the greedy fixtures, asserted.  No beam row has such margins: there the identical rows are held to
    F16_BEAM_IDENTICAL_FLOOR."""
    g, cfg, preds, _ = _run(name, "f16")
    span = float(g["logit_max"]) - float(g["logit_min"])
    assert preds.shape == g["predictions"].shape, (preds.shape, g["predictions"].shape)
    stats = ids_parity(preds, g["predictions"], g["step_margin"], 2 * logit_bound("f16", span), chained=not _greedy(g),
                       first_decision_pos=0 if g["prefix"].size else 1, min_identical=F16_BEAM_IDENTICAL_FLOOR.get(name))
    print(name, "f16 identical rows", stats["identical"], "of", stats["rows"], stats)
    if _greedy(g):
        assert stats["safe_rows"] == stats["identical"] == stats["rows"]


@pytest.mark.parametrize("name", CASES)
def test_bf16_ids_leave_the_reference_only_at_a_near_tie(name):
    """No disagreement at a decision whose margin reaches logit_bound("bf16", span); the identical rows are printed, not gated"""
    g, cfg, preds, _ = _run(name, "bf16")
    span = float(g["logit_max"]) - float(g["logit_min"])
    stats = _parity(g, preds, logit_bound("bf16", span))
    print(name, "bf16 identical rows", stats["identical"], "of", stats["rows"], stats)


# ---- 4. the rules hold on every returned row, exactly ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_returned_rows_keep_their_rules(name, precision):
    g, cfg, preds, lps = _run(name, precision)
    assert np.isfinite(lps).all()
    for q, (hist, ended) in enumerate(_histories(preds, g, cfg)):
        assert not _broken(g["table"][q], g["sets"], hist, ended, _plen(g), cfg), (q, hist, g["table"][q])


# ---- 5. each sentence gets what its own call gets -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("constraints_tiny_greedy", "constraints_tiny_beam4"))
def test_a_sentence_is_not_touched_by_its_neighbours_constraints(name):
    g, cfg, model, batch = _case(name, "f32")
    mixed = model(batch, _params(g, cfg.vocab))
    B, table = int(g["batch"]), g["table"].tolist()
    for q in range(B):
        alone = model(batch, _params(g, cfg.vocab, [table[q]] * B))
        a, b = mixed["predictions"][q].tolist(), alone["predictions"][q].tolist()
        cut = lambda r: r[:r.index(cfg.eos) + 1] if cfg.eos in r else r          # the batch may end sooner or later than the sentence
        assert cut(a) == cut(b), (q, a, b)
        assert torch.equal(mixed["logprobs"][q].cpu(), alone["logprobs"][q].cpu()), q
    model.close()


# ---- 6. one-shot ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
def test_arming_is_consumed_by_one_call(precision):
    g, cfg, model, batch = _case("constraints_tiny_greedy", precision)
    B = int(g["batch"])
    plain = model(batch)
    armed = model(batch, _params(g, cfg.vocab))
    assert not _same(armed, plain)
    assert _same(model(batch), plain)                            # the call after a constrained call
    assert _same(model(batch, _params(g, cfg.vocab)), armed)
    # armed with nothing to enforce: the generic head, the plain ids
    assert model.engine.constrain(None, [[-1, 0, 0]] * B) == {"sentences": B, "sets": 0, "words": (cfg.vocab + 31) // 32}
    assert _same(model(batch), plain)
    # armed, then disarmed with Q == 0
    model.engine.constrain(g["sets"], g["table"].tolist())
    assert model.engine.constrain(None, [])["sentences"] == 0
    assert _same(model(batch), plain)
    # a clone starts disarmed
    model.engine.constrain(g["sets"], g["table"].tolist())
    other = model.engine.clone()
    from generativeimage2text_amd.engine import Engine
    t, lp, _ = other.generate([batch["image"]], Engine.make_search("greedy", 14, 1, 1))
    L = plain["predictions"].shape[1]
    assert torch.equal(t[:, :L].cpu(), plain["predictions"].cpu())
    other.close()
    assert _same(model(batch), armed)                            # ... and the source is still armed
    model.close()


# ---- 7. sampling ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_sampling_never_draws_a_banned_token(precision):
    """f16: the fused head's stored logits carry the ban and the filter reads them; f32: sample_rows applies it"""
    from oracle import git_oracle as O
    g, cfg, model, batch = _case("constraints_tiny_greedy", precision, search=O.SearchConfig("beam", 14, 2, 2, 0.6))
    B = int(g["batch"])
    rng = np.random.default_rng(0)
    banned = sorted(set(rng.choice(cfg.vocab, 600, replace=False).tolist()) - {cfg.eos})
    sp = dict(do_sample=True, top_k=50, bad_tokens=banned, min_new_tokens=[0, 3, 6, 9])
    first = None
    for seed in range(64):
        out = model(batch, dict(sp, seed=seed))
        rows = out["predictions"].cpu().tolist()
        for q, row in enumerate(rows):
            body = row[1:]
            gen = body[:body.index(cfg.eos)] if cfg.eos in body else body
            assert not set(gen) & set(banned), (seed, q, row)
            assert len(gen) >= sp["min_new_tokens"][q], (seed, q, row)
        if seed == 0:
            first = out
    assert _same(model(batch, dict(sp, seed=0)), first)
    assert not _same(model(batch, dict(sp, seed=1)), first)
    model.close()


# ---- 8. residency and graphs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_followups_and_graph_replays(precision):
    g, cfg, model, batch = _case("constraints_tiny_greedy", precision)
    B, table = int(g["batch"]), g["table"].tolist()
    sp1 = _params(g, cfg.vocab)
    sp2 = _params(g, cfg.vocab, [table[(q + 1) % B] for q in range(B)])          # the same shape, other values
    _, _, fresh, _ = _case("constraints_tiny_greedy", precision)
    fresh.engine.set_graph(False)
    want1, want2, want_plain = fresh(batch, sp1), fresh(batch, sp2), fresh(batch)
    fresh.close()
    assert not _same(want1, want2)
    got1 = model(batch, sp1)                     # captures the constrained graph
    got2 = model(batch, sp2)                     # replays it: the values live in the engine's tables
    got_plain = model(batch)                     # the plain graph ...
    got1b = model(batch, sp1)                    # ... and armed and plain calls alternate
    got_plain_b = model(batch)
    assert _same(got1, want1) and _same(got2, want2) and _same(got1b, want1)
    assert _same(got_plain, want_plain) and _same(got_plain_b, want_plain)
    # an armed follow-up over the resident images equals the armed full call: bit for bit through the same entry point ...
    from generativeimage2text_amd.engine import Engine
    first = model.submit(batch)
    first.result()
    eng, L = model.engine, want1["predictions"].shape[1]
    eng.constrain(*model._constraints(sp1, B))
    t, lp, _ = eng.generate(None, Engine.make_search("greedy", 14, 1, 1))
    assert torch.equal(t[:, :L].cpu(), want1["predictions"].cpu()) and torch.equal(lp.cpu().reshape(-1), want1["logprobs"].cpu().reshape(-1))
    # ... and through the front end (on=result), where every sentence stands for its own call
    follow = {"prefixes": [[cfg.sos]] * B, "image_of": list(range(B))}
    f1 = model.submit_followup(follow, sp1, on=first).result()
    f2 = model.submit_followup(follow, sp2, on=first).result()
    fp = model.submit_followup(follow, on=first).result()
    cut = lambda r: r[:r.index(cfg.eos) + 1] if cfg.eos in r else r
    for q in range(B):
        assert cut(f1["predictions"][q]) == cut(want1["predictions"][q, 1:].tolist()), (q, f1["predictions"][q], want1["predictions"][q])
        assert cut(f2["predictions"][q]) == cut(want2["predictions"][q, 1:].tolist()), q
        assert cut(fp["predictions"][q]) == cut(want_plain["predictions"][q, 1:].tolist()), q
    model.close()


# ---- 9. refusals: by message, before any launch, everything as it was ---------------------------------------------------------------------
def _raw_constrain(eng, frames, image_of, table, n_sets=0, words=None):
    from generativeimage2text_amd import engine as E
    s = E.GitmiSearch()
    s.kind = E.SEARCH_CONSTRAIN
    Q = len(table)
    arr = None if frames is None else eng._frames_arg(frames)[0]
    tab = (C.c_int32 * max(3 * Q, 1))(*[v for r in table for v in r])
    img = None if image_of is None else (C.c_int32 * len(image_of))(*image_of)
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    eng._ck(eng.lib.gitmi_generate_prefixed(eng._h, arr, 1, Q, None if words is None else words.data_ptr(), n_sets, tab, img, Q, C.byref(s),
                                            None, None, None, info.data_ptr(), int(torch.cuda.current_stream().cuda_stream)))


def test_refusals_leave_arming_and_residency():
    from generativeimage2text_amd import engine as E
    g, cfg, model, batch = _case("constraints_tiny_greedy", "f32")
    eng, B, table = model.engine, int(g["batch"]), g["table"].tolist()
    frames = [batch["image"]]
    greedy = E.Engine.make_search("greedy", 14, 1, 1)
    plain = model(batch)
    armed = model(batch, _params(g, cfg.vocab))

    def resident_answer():
        t, lp, _ = eng.generate(None, greedy)
        return t.cpu(), lp.cpu()

    before = resident_answer()

    def intact():
        after = resident_answer()
        return eng.resident == B and torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and _same(model(batch), plain)

    words = torch.from_numpy(g["sets"].view(np.int32)).cuda()
    n_sets = int(words.shape[0])
    for bad_row, match in (([n_sets, 0, 0], rf"constrain: sentence 2: set index {n_sets} outside \[-1,{n_sets}\)"),
                           ([-2, 0, 0], r"constrain: sentence 2: set index -2 outside"),
                           ([-1, 15, 0], r"constrain: sentence 2: min_new 15 outside \[0,14\]"),
                           ([-1, -1, 0], r"constrain: sentence 2: min_new -1 outside"),
                           ([-1, 0, 9], r"constrain: sentence 2: ngram 9 outside \[0,8\]"),
                           ([-1, 0, -1], r"constrain: sentence 2: ngram -1 outside")):
        rows = [list(r) for r in table]
        rows[2] = bad_row
        with pytest.raises(E.GitmiError, match=match):
            eng.constrain(g["sets"], rows)
        assert intact()
    with pytest.raises(E.GitmiError, match="constrain: frames != NULL"):
        _raw_constrain(eng, frames, None, table, n_sets, words)
    assert intact()
    with pytest.raises(E.GitmiError, match="constrain: image_of != NULL"):
        _raw_constrain(eng, None, list(range(B)), table, n_sets, words)
    assert intact()
    _raw_constrain(eng, frames, list(range(B)), [])               # Q == 0 disarms and reads nothing else
    assert intact()
    with pytest.raises(E.GitmiError, match=rf"constrain: Q={B + 1} sentences outside"):
        eng.constrain(None, [[-1, 1, 0]] * (B + 1))
    assert intact()
    # kind 10 is not a search
    s = E.Engine.make_search("greedy", 14, 1, 1)
    s.kind = E.SEARCH_CONSTRAIN
    with pytest.raises(E.GitmiError, match="generate: GITMI_SEARCH_CONSTRAIN arms decoding constraints: call gitmi_generate_prefixed"):
        eng.generate(frames, s)
    assert intact()
    with pytest.raises(E.GitmiError, match="GITMI_SEARCH_CONSTRAIN is not a search"):
        eng.search_begin(s, torch.full((B, 1), cfg.sos), cfg.vocab)
    assert intact()
    # while armed: another sentence count names both numbers and stays armed; the trie search and the seam refuse by name;
    # the kinds that are not searches run unconstrained and leave the arming alone
    eng.constrain(g["sets"], table)
    with pytest.raises(E.GitmiError, match=rf"armed for {B} sentences, this call has 2"):
        eng.generate_prefixed(None, greedy, [[cfg.sos]] * 2, image_of=[0, 1])
    with pytest.raises(E.GitmiError, match="GITMI_SEARCH_TRIE while decoding constraints are armed"):
        eng.generate(None, E.Engine.make_search("trie", 14, 1, 1))
    with pytest.raises(E.GitmiError, match=rf"search_begin: decoding constraints are armed for {B} sentences"):
        eng.search_begin(greedy, torch.full((B, 1), cfg.sos), cfg.vocab)
    sc = eng.score(None, torch.tensor([[cfg.sos, 5, 6]] * B))
    assert sc.shape == (B, 3, 2) and eng.resident == B
    # a refused arming call keeps what was armed
    with pytest.raises(E.GitmiError, match="ngram 9"):
        eng.constrain(None, [[-1, 0, 9]] * B)
    assert _same(model(batch), armed)                            # still armed: this call consumes it
    assert intact()
    model.close()
