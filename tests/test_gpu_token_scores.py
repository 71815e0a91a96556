"""The per-token trace (GITMI_SEARCH_TRACE; search_param output_scores / top_logprobs) on whole calls, f32 / f16 / bf16, against
fixtures frozen from the reference search classes behind a recording step (tools/make_token_scores_golden.py ->
tests/golden/tokscore_*.npz): greedy B = 4, AUTOREGRESSIVE beam 4, GENERATOR beam 4 with num_keep_best = 3 and a repetition
penalty, a batch-1 call with a three-token prefix, the TINY decoder at vocab 30522 (the head's multi-part lists), and greedy with
wrap_step constraints; n = 5 everywhere.  Every fixture records, per (position, rank), whether the gap to the next rank reaches
2 x logit_bound("f16", span), and the certificate it was frozen under: f16 (90 % of the pairs and every decision reach that
threshold) or, where the surveyed seeds held none, f32 (every gap and decision >= 10 x F32_LOGIT_ABS).

Also, in every precision: both invariants, traced == plain bit for bit, one-shot arming, captured graphs, zeros past the end,
follow-up and prefixed calls, the refusals; and model(batch, search_param) end to end."""
import ast
import dataclasses
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import git_oracle as O
from tools.constrained_step import set_mask, wrap_step
from tools.parity import F32_LOGIT_ABS, logit_bound
from tools.token_scores_rule import check_sum, length_norm, records_of

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16", "bf16")
N = 5
_cache = {}


def _reference(name):
    """-> dict(cfg, w, frames, search, params, ids, recs, gaps, span): the oracle's constrained greedy search of fixture `name` with
    its step calls recorded, and per sentence the records of positions [1, L) -- computed once, read-only"""
    if name in _cache:
        return _cache[name]
    g = load_golden(name)
    cfg = dataclasses.replace(O.CONFIGS[str(g["config"])], vocab=int(g["vocab"]))
    kind, T, k, pn, alpha = ast.literal_eval(str(g["search"]))
    assert kind == "greedy" and k == 1
    w = O.make_weights(cfg, **ast.literal_eval(str(g["weights_kw"])))
    B = int(g["batch"])
    frames = O.make_images(cfg, B, 1, seed=int(g["image_seed"]))
    table = g["table"].tolist()
    calls, span = [], [math.inf, -math.inf]
    with torch.no_grad():
        raw = O.make_step(cfg, w, O.visual_features(cfg, w, frames), cached=True)

        def watched(tokens):
            z = raw(tokens)
            span[0], span[1] = min(span[0], float(z.min())), max(span[1], float(z.max()))
            return z

        banned = wrap_step(watched, g["sets"], table, cfg.eos, [1] * B)

        def step(tokens):
            z = banned(tokens)
            calls.append((tokens.clone(), z.clone()))
            return z

        ids, lps = O.search_autoregressive(torch.full((B, 1), cfg.sos, dtype=torch.long), step, cfg.eos, T, 1, 1)
    assert np.array_equal(ids.numpy(), g["predictions"])                 # the oracle returns the fixture's (reference's) ids
    L = ids.shape[1]
    recs = [records_of("autoregressive", calls, ids[b].tolist(), 1, L, N + 1, cfg.eos, sentence=b, sentences=B) for b in range(B)]
    bad = [None if s < 0 else np.flatnonzero(set_mask(g["sets"][s], cfg.vocab).numpy()).tolist() for s, _, _ in table]
    params = {"bad_tokens": bad, "min_new_tokens": [r[1] for r in table], "no_repeat_ngram_size": [r[2] for r in table]}
    _cache[name] = dict(cfg=cfg, w=w, frames=frames, T=T, params=params, ids=ids, lps=lps, recs=recs, span=span[1] - span[0], L=L)
    return _cache[name]


def _model(ref, precision, decoder=None, **kw):
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch, CaptioningModel
    cfg = ref["cfg"]
    dec = decoder or AutoRegressiveBeamSearch(eos_index=cfg.eos, max_steps=ref["T"], beam_size=1, per_node_beam_size=1,
                                              fix_missing_prefix=True)
    m = CaptioningModel(cfg, dec, precision=precision, max_batch=kw.pop("max_batch", 4), max_frames=1, max_text_len=ref["T"], **kw)
    m.load_state_dict(ref["w"])
    return m


FIXTURES = ("tokscore_greedy", "tokscore_ar_beam4", "tokscore_gen_beam4_keep3", "tokscore_prefix", "tokscore_fullvocab",
            "tokscore_constrained")
_fix = {}


def _fixture(name):
    """-> (fixture arrays, cfg, weights, frames, search struct), rebuilt once from the recorded seeds (read-only)"""
    if name not in _fix:
        from generativeimage2text_amd.engine import Engine
        g = load_golden(name)
        cfg = dataclasses.replace(O.CONFIGS[str(g["config"])], vocab=int(g["vocab"]))
        kind, T, k, pn, alpha = ast.literal_eval(str(g["search"]))
        w = O.make_weights(cfg, **ast.literal_eval(str(g["weights_kw"])))
        frames = O.make_images(cfg, int(g["batch"]), 1, seed=int(g["image_seed"]))
        search = Engine.make_search(kind, T, k, pn, alpha, repetition_penalty=float(g["repetition_penalty"]),
                                    num_keep_best=int(g["num_keep_best"]))
        _fix[name] = (g, cfg, w, frames, search)
    return _fix[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_conditions(name):
    """what tools/make_token_scores_golden.py asserted when it froze the fixture: its certificate, and the sum invariant on the
    reference's own log-probs"""
    g, cfg, _, _, search = _fixture(name)
    thr = 2.0 * logit_bound("f16", float(g["logit_span"]))
    if str(g["certificate"]) == "f16":
        assert float(g["share"]) >= 0.9 and float(g["step_margin"]) >= thr
        assert float(g["gap_ok"].sum()) >= 0.9 * float(g["counted"].sum())
    else:
        assert float(g["gap_min"]) >= 10 * F32_LOGIT_ABS and float(g["step_margin"]) >= 10 * F32_LOGIT_ABS
    T, P = int(search.max_steps), max(1, int(g["prefix"].size))
    for o in range(g["tokens"].shape[0]):
        if float(g["logprobs"][o]) == -1e5:
            continue
        L, row = int(g["length"][o]), g["tokens"][o].tolist()
        div = length_norm(L, float(search.length_penalty)) if search.kind == 1 else \
            max(1, sum(t != cfg.eos for t in row[:L]) + (1 if cfg.eos in row[:L] else 0) - P)
        assert check_sum(g["lp"][o].tolist(), float(g["logprobs"][o]), div, T) is None


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", FIXTURES)
def test_traced_call_against_the_reference_fixture(name, precision):
    """One whole call per fixture, traced with n = 5 (captured graphs on; tokscore_prefix: a shared prefix of three tokens, so the
    first steps only append given tokens).  f32: every lp and alternative lp within F32_LOGIT_ABS, every alternative token and
    every id equal.  16-bit: on rows whose ids are the reference's, values within logit_bound(prec, span); the top-(j + 1)
    alternatives are compared as a set where the recorded gap between ranks j and j + 1 reaches the threshold; the compared share
    is held to 90 % on fixtures under the f16 certificate (test_fixture_conditions holds the others to the f32 certificate)."""
    from generativeimage2text_amd.engine import Engine
    g, cfg, w, frames, search = _fixture(name)
    B, T, nh, n = int(g["batch"]), int(search.max_steps), int(g["num_keep_best"]), int(g["n"])
    e = Engine(cfg, precision=precision, max_batch=B, max_beams=int(search.beam_size), max_frames=1, max_text_len=T)
    e.load_state_dict(w)
    prefix = torch.tensor(g["prefix"]) if g["prefix"].size else None
    dev_frames = [frames[0].cuda()]

    def call(traced):
        if bool(g["constrained"]):
            e.constrain(g["sets"], g["table"].tolist())
        out = e.trace(B, nh, T, n) if traced else (None, None)
        toks, lps, _ = e.generate(dev_frames, search, prefix=prefix)
        torch.cuda.synchronize()
        return toks.cpu().reshape(B * nh, T), lps.cpu().reshape(-1), out[0], out[1]

    toks, lps, lp, tok = call(True)
    ptoks, plps, _, _ = call(False)
    e.close()
    assert torch.equal(toks, ptoks) and torch.equal(lps, plps)          # traced == plain, bit for bit
    lp, tok = lp.cpu().double(), tok.cpu()
    f32 = precision == "f32"
    bound = logit_bound(precision, float(g["logit_span"]))
    want_tok = torch.from_numpy(g["tokens"])
    # AUTOREGRESSIVE rows are compared up to the sentence's own length: what lies behind it in tokens_out is [SEP] either way
    same = [bool(torch.equal(toks[o], want_tok[o])) for o in range(B * nh)]
    if f32:
        assert all(same), (toks.tolist(), want_tok.tolist())
    worst, compared, pairs, rows = 0.0, 0, 0, 0
    for o in range(B * nh):
        if not same[o]:
            continue
        rows += 1
        assert abs(float(lps[o]) - float(g["logprobs"][o])) <= max(bound, F32_LOGIT_ABS) * max(1.0, abs(float(g["logprobs"][o])))
        for s in range(T):
            want = float(g["lp"][o, s])
            worst = max(worst, abs(float(lp[o, s, 0]) - want))
            for j in range(n):
                wa, ga = float(g["alt_lp"][o, s, j]), float(lp[o, s, 1 + j])
                if not g["counted"][o, s, j]:                            # no record here, or a -inf entry of a one-hot row: exact
                    if int(g["alt_tok"][o, s, 0]) < 0 or not math.isfinite(wa):
                        assert ga == wa and int(tok[o, s, j]) == int(g["alt_tok"][o, s, j]), (o, s, j)
                    continue
                pairs += 1
                if f32 or bool(g["gap_ok"][o, s, j]):
                    compared += 1
                    assert set(tok[o, s, :j + 1].tolist()) == set(g["alt_tok"][o, s, :j + 1].tolist()), (o, s, j)
                    if f32:
                        assert int(tok[o, s, j]) == int(g["alt_tok"][o, s, j]), (o, s, j)
                if f32 or (bool(g["gap_ok"][o, s, j]) and (j == 0 or bool(g["gap_ok"][o, s, j - 1]))):
                    worst = max(worst, abs(ga - wa))                     # the same token at this rank: the same number
    print(f"{name} {precision}: {rows}/{B * nh} rows with the reference's ids, largest |value - reference| {worst:.3e} "
          f"(bound {bound:.3e}), alternative boundaries compared {compared}/{pairs}")
    assert worst <= bound
    if str(g["certificate"]) == "f16":
        assert rows == B * nh                                            # every decision is certified for the 16-bit builds
        assert compared >= 0.9 * pairs


def test_front_end_keys_through_the_model():
    """model(batch, {constraints, top_logprobs}): the result gains token_logprobs / top_tokens / top_logprobs cut like predictions,
    and equals the plain request's predictions and log-probs; the values are the oracle's records after the bans."""
    ref = _reference("constraints_tiny_greedy")
    model = _model(ref, "f32")
    batch = {"image": ref["frames"][0].cuda()}
    out = model(batch, dict(ref["params"], top_logprobs=N))
    plain = model(batch, ref["params"])
    model.close()
    preds = out["predictions"].cpu()
    assert torch.equal(preds, plain["predictions"].cpu()) and torch.equal(out["logprobs"].cpu(), plain["logprobs"].cpu())
    assert "token_logprobs" not in plain and torch.equal(preds, ref["ids"])
    eos = ref["cfg"].eos
    for b in range(preds.shape[0]):
        lp, toks, alts = out["token_logprobs"][b], out["top_tokens"][b], out["top_logprobs"][b]
        row = preds[b].tolist()
        assert len(lp) == len(toks) == len(alts) == len(row) and lp[0] == 0.0 and toks[0] == [-1] * N
        ended = row.index(eos) if eos in row else len(row)
        for s in range(1, len(row)):
            if s > ended:
                assert lp[s] == 0.0 and toks[s] == [-1] * N
                continue
            want_lp, want_tok, want_alt = ref["recs"][b][s - 1]
            assert abs(lp[s] - want_lp) <= F32_LOGIT_ABS and toks[s] == want_tok[:N] and toks[s][0] == row[s]
            assert max(abs(a - w) for a, w in zip(alts[s], want_alt)) <= F32_LOGIT_ABS
        nv = max(1, sum(t != eos for t in row) + (1 if eos in row else 0) - 1)
        assert check_sum(lp, float(out["logprobs"][b]), nv, ref["T"]) is None


def _engine(ref, precision, graph, **kw):
    from generativeimage2text_amd.engine import Engine
    e = Engine(ref["cfg"], precision=precision, max_batch=4, max_beams=4, max_frames=1, max_text_len=ref["T"], **kw)
    e.load_state_dict(ref["w"])
    e.set_graph(graph)
    return e


def _traced(e, frames, search, n, Q):
    from generativeimage2text_amd.engine import Engine
    nout = max(1, int(search.num_keep_best))
    lp, tok = e.trace(Q, nout, int(search.max_steps), n)
    toks, lps, _ = e.generate(frames, search)
    torch.cuda.synchronize()
    return toks.cpu(), lps.cpu(), lp.cpu(), (tok.cpu() if tok is not None else None)


@pytest.mark.parametrize("precision", PRECS)
def test_plain_and_traced_calls_alternate_with_and_without_graphs(precision):
    """plain, traced, plain, traced with another n: every call returns the same ids and log-probs bit for bit, with captured graphs
    and without; the traces of the two engines are equal; arming is one-shot (the plain calls leave the buffers alone)."""
    from generativeimage2text_amd.engine import Engine
    ref = _reference("constraints_tiny_greedy")
    frames = [ref["frames"][0].cuda()]
    B = int(frames[0].shape[0])
    for search in (Engine.make_search("greedy", ref["T"], 1, 1), Engine.make_search("beam", ref["T"], 4, 2, 0.6, num_keep_best=3,
                                                                                   repetition_penalty=1.2)):
        seen = []
        for graph in (True, False):
            e = _engine(ref, precision, graph)
            t0, l0, _ = e.generate(frames, search)
            t1, l1, lp1, tok1 = _traced(e, frames, search, 2, B)
            keep = e._trace_keep[0].clone()
            t2, l2, _ = e.generate(frames, search)
            torch.cuda.synchronize()
            assert torch.equal(e._trace_keep[0], keep)                  # one-shot: the plain call did not trace
            t3, l3, lp3, tok3 = _traced(e, frames, search, N, B)
            e.close()
            for t, l in ((t1, l1), (t2.cpu(), l2.cpu()), (t3, l3)):
                assert torch.equal(t, t0.cpu()) and torch.equal(l, l0.cpu())
            assert torch.equal(lp1[..., 0], lp3[..., 0]) and torch.equal(lp1[..., 1:], lp3[..., 1:3]) and torch.equal(tok1, tok3[..., :2])
            seen.append((t0.cpu(), l0.cpu(), lp3, tok3))
        for a, b in zip(seen[0], seen[1]):
            assert torch.equal(a, b)
        # both invariants on the traced call
        toks, lps, lp, tok = seen[0]
        toks, lps = toks.reshape(-1, ref["T"]), lps.reshape(-1)
        eos, T = ref["cfg"].eos, ref["T"]
        hits = 0
        for o in range(toks.shape[0]):
            row = toks[o].tolist()
            if float(lps[o]) == -1e5:
                assert float(lp[o].abs().sum()) == 0.0 and bool((tok[o] == -1).all())
                continue
            if search.kind == 0:
                div, end = max(1, sum(t != eos for t in row) + (1 if eos in row else 0) - 1), T
            else:
                n_h = row.index(eos)
                div, end = length_norm(n_h, 0.6), n_h + 1
                assert float(lp[o, end:].abs().sum()) == 0.0 and bool((tok[o, end:] == -1).all())      # zeros past the end
            assert check_sum(lp[o, :, 0].tolist(), float(lps[o]), div, T) is None, o
            for s in range(1, min(end, T)):
                alts = tok[o, s].tolist()
                if (search.kind == 0 or s < end - 1) and row[s] in alts:
                    assert float(lp[o, s, 1 + alts.index(row[s])]) == float(lp[o, s, 0])
                    hits += 1
        assert hits > 0


@pytest.mark.parametrize("precision", PRECS)
def test_followup_prefixed_and_short_after_long(precision):
    """A traced follow-up call (frames None) with per-sentence prefixes over the resident images equals the traced call that brings
    the frames; a short-budget call after a long one leaves nothing of the long one: zeros past its end."""
    from generativeimage2text_amd.engine import Engine
    ref = _reference("constraints_tiny_greedy")
    frames = [ref["frames"][0].cuda()]
    T = ref["T"]
    first = [int(t) for t in ref["ids"][:, 1]]
    prefixes = [[101, first[0]], [101], [101, first[2], 7]]
    image_of = [0, 1, 2]
    e = _engine(ref, precision, True)
    s = Engine.make_search("greedy", T, 1, 1)
    lp_a, tok_a = e.trace(3, 1, T, 3)
    ta, la, sa, _ = e.generate_prefixed(frames, s, prefixes, image_of=image_of)
    lp_a, tok_a = lp_a.clone(), tok_a.clone()
    lp_b, tok_b = e.trace(3, 1, T, 3)
    tb, lb, sb, _ = e.generate_prefixed(None, s, prefixes, image_of=image_of)
    torch.cuda.synchronize()
    assert torch.equal(ta, tb) and torch.equal(la, lb) and torch.equal(lp_a, lp_b) and torch.equal(tok_a, tok_b)
    for q, p in enumerate(prefixes):
        L = int(sb[q, 0])
        assert float(lp_b[q, :len(p)].abs().sum()) == 0.0 and bool((tok_b[q, :len(p)] == -1).all())
        assert float(lp_b[q, len(p):L, 0].max()) <= 0.0 and float(lp_b[q, len(p), 0]) < 0.0
        assert float(lp_b[q, L:].abs().sum()) == 0.0 and bool((tok_b[q, L:] == -1).all())
    # every prefix has two or more tokens: the first step only appends given tokens and reads no list (n = 5 > its one slot)
    lp_e, tok_e = e.trace(2, 1, T, 5)
    te, le, _, _ = e.generate_prefixed(None, s, [prefixes[0], prefixes[2]], image_of=[0, 2])
    torch.cuda.synchronize()
    assert torch.equal(te, tb[[0, 2]]) and torch.equal(le, lb[[0, 2]])
    assert torch.equal(lp_e[:, :, :4], lp_b[[0, 2]]) and torch.equal(tok_e[:, :, :3], tok_b[[0, 2]])
    # sentence 1 has the plain [CLS] prefix: its trace is the plain captioning call's
    lp_c, tok_c = e.trace(4, 1, T, 3)
    tc, lc, _ = e.generate(frames, s)
    torch.cuda.synchronize()
    assert torch.equal(tc[1], tb[1]) and torch.equal(lp_c[1], lp_b[1]) and torch.equal(tok_c[1], tok_b[1])
    short = Engine.make_search("greedy", 4, 1, 1)
    lp_d, tok_d = e.trace(4, 1, 4, 3)
    e.generate(frames, short)
    torch.cuda.synchronize()
    assert torch.equal(lp_d[:, :4], lp_c[:, :4]) and torch.equal(tok_d[:, :4], tok_c[:, :4])
    e.close()


def test_refusals_refuse_and_the_arming_still_fires():
    from generativeimage2text_amd.engine import Engine, GitmiError
    ref = _reference("constraints_tiny_greedy")
    frames = [ref["frames"][0].cuda()]
    T = ref["T"]
    e = _engine(ref, "f32", True)
    s = Engine.make_search("greedy", T, 1, 1)
    lp, tok = e.trace(4, 1, T, 2)
    lp.fill_(7.0)
    with pytest.raises(GitmiError, match="armed for 4 sentences, this call has 2"):
        e.generate([frames[0][:2]], s)
    with pytest.raises(GitmiError, match="armed for max_steps 14, this call has 6"):
        e.generate(frames, Engine.make_search("greedy", 6, 1, 1))
    with pytest.raises(GitmiError, match="armed for 1 sequences per sentence .* this call returns 3"):
        e.generate(frames, Engine.make_search("beam", T, 4, 2, 0.6, num_keep_best=3))
    with pytest.raises(GitmiError, match="do_sample while the per-token trace is armed with 2 alternatives"):
        e.generate(frames, Engine.make_search("beam", T, 1, 2, 0.6, do_sample=True, top_k=5))
    e.set_trie([0, 1, 1], [5], [1])
    with pytest.raises(GitmiError, match="GITMI_SEARCH_TRIE while the per-token trace is armed"):
        e.generate(frames, Engine.make_search("trie", T, 1, 1))
    traced = Engine.make_search("greedy", T, 1, 1)
    traced.kind = 11
    with pytest.raises(GitmiError, match="generate: GITMI_SEARCH_TRACE arms the per-token trace"):
        e.generate(frames, traced)
    torch.cuda.synchronize()
    assert bool((lp == 7.0).all())
    toks, lps, _ = e.generate(frames, s)                    # still armed: this one is traced
    torch.cuda.synchronize()
    assert float(lp[:, 0].abs().sum()) == 0.0 and float(lp[:, 1, 0].max()) < 0.0
    # sampling with n == 0 is traced: one beam, so the sum follows the history
    g = Engine.make_search("beam", T, 1, 2, 0.6, do_sample=True, top_k=5, seed=3)
    lp0, none = e.trace(4, 1, T, 0)
    assert none is None
    toks, lps, _ = e.generate(frames, g)
    torch.cuda.synchronize()
    for o in range(4):
        n_h = toks[o].tolist().index(ref["cfg"].eos)
        assert check_sum(lp0[o, :, 0].tolist(), float(lps[o]), length_norm(n_h, 0.6), T) is None
    e.trace(0)                                              # disarm: nothing to consume
    e.close()
