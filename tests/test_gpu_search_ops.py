"""Op-level tests of the fused decode step of the 16-bit builds (measurement build, include/gitmi_experiment.h):
the multi-part list merge of search_step_kernel on caller-supplied lists, the rules of vocab_topm_kernel (no immediate
repeat, repetition penalty) with real histories, both chained over several steps against the fp64 oracle, and the embedding
the search step fuses.  Shapes are the smallest at which these kernels can go wrong; every case takes a few seconds at most."""
import dataclasses
import math

import pytest
import torch

from oracle import git_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("experiment_build")]

PAD = 0x7fffffff
V_SMALL = 1000
NPARTS = [1, 8, 63, 64, 65, 128, 129, 192, 239, 250, 256]

_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng, _, _ in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def _engine(tag, vocab=V_SMALL, hidden=128, max_batch=8, max_beams=8, T=16):
    """(engine, cfg, weights) of a TINY-shaped model in the 16-bit mode of the measurement build, shared by the module's tests
    (the search seam keeps no state between searches).  `tag` tells twins apart."""
    key = (tag, vocab, hidden, max_batch, max_beams, T)
    if key not in _ENGINES:
        from generativeimage2text_amd.engine import Engine
        cfg = dataclasses.replace(O.CONFIGS["TINY"], vocab=vocab, dec_hidden=hidden, dec_heads=hidden // 64, dec_ffn=4 * hidden)
        w = O.make_weights(cfg, seed=3)
        eng = Engine(cfg, precision="bf16", max_batch=max_batch, max_beams=max_beams, max_frames=1, max_text_len=T)
        eng.load_state_dict(w)
        _ENGINES[key] = (eng, cfg, w)
    return _ENGINES[key]


# ---- the lists of the fused head, built on the CPU ---------------------------------------------------------------------------
def _bounds(V, nparts):
    """Column blocks of one row: width c = ceil(V / nparts) with a partial last block where that gives `nparts` blocks
    (V = 1000: 1, 8, 63, 250), else widths floor / ceil(V / nparts) (V = 1000 has no single width that gives 64, 65, 128, 129, 192,
    239 or 256 blocks).  The merge sees lists only; their widths do not reach it."""
    c = -(-V // nparts)
    if -(-V // c) == nparts:
        return [min(p * c, V) for p in range(nparts + 1)]
    return [p * V // nparts for p in range(nparts + 1)]


def _cpu_lists(x, bounds, slots):
    """What vocab_topm_kernel emits for the fp32 logits x [R, V] (CPU): per block the `slots` best (value descending, token
    ascending), unused slots (-inf, 0x7fffffff), and (block max, sum exp(x - max))."""
    R, n = x.shape[0], len(bounds) - 1
    pv = torch.full((R, n, slots), float("-inf"))
    pi = torch.full((R, n, slots), PAD, dtype=torch.int32)
    pl = torch.zeros(R, n, 2)
    for p in range(n):
        a, b = bounds[p], bounds[p + 1]
        blk = x[:, a:b]
        o = torch.sort(blk, dim=1, descending=True, stable=True)
        k = min(slots, b - a)
        pv[:, p, :k] = o.values[:, :k]
        pi[:, p, :k] = (o.indices[:, :k] + a).int()
        m = blk.max(1).values
        pl[:, p, 0] = m
        pl[:, p, 1] = torch.exp(blk - m[:, None]).sum(1)
    return pv, pi, pl


# ---- A. the merge against fp64, one step ---------------------------------------------------------------------------------------
def _merge_rows(bounds, eos, seed):
    """Six logit rows [6, V] with the winners placed where the merge can lose them: 0 plain; 1 all in one part (one list is popped
    over and over); 2 one per quarter q = 0..3 of the lane's register lists (parts 5 + 64 q); 3 the first column of the last part
    and the last of the first; 4 columns 0 and V - 1; 5 either side of the quarter boundaries (parts 63 | 64, 127 | 128, 191 | 192)."""
    n, V = len(bounds) - 1, bounds[-1]
    x = torch.randn(6, V, generator=torch.Generator().manual_seed(seed))
    x[:, eos] = -20.0
    first, last, width = (lambda p: bounds[p]), (lambda p: bounds[p + 1] - 1), (lambda p: bounds[p + 1] - bounds[p])
    p1 = n // 2
    plant = {1: [first(p1) + j for j in range(min(8, width(p1)))],
             2: [last(5 + 64 * q) for q in range(4) if 5 + 64 * q < n],
             3: [first(n - 1), last(0)],
             4: [0, V - 1],
             5: [first(p) + width(p) // 2 for p in (63, 64, 127, 128, 191, 192) if p < n]}
    for row, cols in plant.items():
        cols = list(dict.fromkeys(cols))
        assert eos not in cols
        for j, c in enumerate(cols):
            x[row, c] = 9.0 - 0.37 * ((j * 5) % 8) - 0.01 * j          # distinct, not in column order
    return x


# log-prob bound of the one-step merge: the lists carry exact fp32 logits, so the error is the log-sum-exp's -- <= 256 partial sums
# rescaled by one __expf each (relative error ~|x| 2^-24 + 1 ulp, |x| <= 16), a 64-lane tree, one logf, two roundings at magnitude
# <= 16 (2^-20 each): about 5e-6 in all.  2e-5 leaves a factor of four.
MERGE_LP_TOL = 2e-5


@pytest.mark.parametrize("nparts", NPARTS)
def test_merge_one_step_against_fp64(nparts):
    """search_step_kernel's phase A on lists cut from fp32 logits [R, 1000] into `nparts` parts: after one advance the beams of an
    AUTOREGRESSIVE search (k = 8 with 8 and 16 slots, k = 1, 2, 4) hold exactly the fp64 top-k tokens in order.  Of their
    log-probs the seam exposes the best beam's only (search_finish), so the AUTOREGRESSIVE runs check the top-1 log-prob; ALL
    merged log-probs are checked through a GENERATOR search whose budget ends with the step: every one of its 2 k candidates
    (8, 4, 2 for k = 4, 2, 1) becomes a hypothesis at length norm 1 and comes back from search_finish with its score."""
    from generativeimage2text_amd.engine import Engine
    eng, cfg, _ = _engine("a")
    V, B = V_SMALL, 6
    bounds = _bounds(V, nparts)
    assert len(bounds) == nparts + 1 and bounds[-1] == V and all(b > a for a, b in zip(bounds, bounds[1:]))
    x = _merge_rows(bounds, cfg.eos, seed=100 + nparts)
    ref_lp = torch.log_softmax(x.double(), dim=1)
    top_lp, top_tok = ref_lp.topk(9, dim=1)
    assert (top_lp[:, :-1] - top_lp[:, 1:]).min().item() > 0           # no ties: the fp64 order is THE order
    noise = torch.randn(B * 8, V, generator=torch.Generator().manual_seed(7))
    start = torch.full((B, 1), cfg.sos, dtype=torch.int64)

    def rows_of(k):                                                     # row b * k = sentence b's logits, the others are not read
        rows = noise[:B * k].clone()
        rows[::k] = x
        return rows

    for k, slot_list in ((8, (8, 16)), (1, (1,)), (2, (2,)), (4, (4,))):
        for slots in slot_list:
            eng.search_begin(Engine.make_search("autoregressive", 4, k, 1), start, V)
            eng.debug_search_advance_lists(*_cpu_lists(rows_of(k), bounds, slots))
            rows = eng.search_rows().cpu()
            _, lps, _ = eng.search_finish()
            assert rows.shape == (B * k, 2)
            assert torch.equal(rows[:, 1].reshape(B, k), top_tok[:, :k]), (nparts, k, slots)
            err = (lps.cpu().double() - top_lp[:, 0]).abs().max().item()
            print(f"nparts {nparts} AR k {k} slots {slots}: top-1 log-prob error {err:.2e}")
            assert err < MERGE_LP_TOL, (nparts, k, slots, err)
    for kg, slot_list in ((4, (8, 16)), (2, (4,)), (1, (2,))):          # GENERATOR: M = 2 kg candidates per row
        for slots in slot_list:
            eng.search_begin(Engine.make_search("beam", 2, kg, 2, 0.6, num_keep_best=2 * kg), start, V)
            eng.debug_search_advance_lists(*_cpu_lists(rows_of(kg), bounds, slots))
            _, lps, _ = eng.search_finish()
            err = (lps.cpu().double().reshape(B, 2 * kg) - top_lp[:, :2 * kg]).abs().max().item()
            print(f"nparts {nparts} GENERATOR k {kg} slots {slots}: log-prob error {err:.2e}")
            assert err < MERGE_LP_TOL, (nparts, kg, slots, err)


def test_advance_lists_refuses_bad_shapes():
    from generativeimage2text_amd.engine import Engine, GitmiError
    eng, cfg, _ = _engine("a")
    start = torch.full((2, 1), cfg.sos, dtype=torch.int64)
    eng.search_begin(Engine.make_search("autoregressive", 4, 4, 1), start, V_SMALL)
    x = torch.randn(8, V_SMALL, generator=torch.Generator().manual_seed(1))
    for bounds, slots, what in ((_bounds(V_SMALL, 257), 4, "nparts"), (_bounds(V_SMALL, 8), 3, "slots"), (_bounds(V_SMALL, 8), 2, "slots")):
        with pytest.raises(GitmiError, match=what):
            eng.debug_search_advance_lists(*_cpu_lists(x, bounds, slots))
    assert eng.search_rows().shape == (8, 1)                            # nothing advanced


# ---- B. ties ------------------------------------------------------------------------------------------------------------------
def _tie_logits(R, V, eos, step):
    """Integer-valued rows, 200 apart: hundreds of equal values per row, and exp(x - max) of every value below the maximum is
    exactly 0 in fp32, so the log-sum-exp is max + log(count of maxima) in ANY summation order -- the twin's single list per row and
    the many-part merge must then agree to the bit, log-probs included.  Three maxima, two runners-up, the rest in big groups."""
    g = torch.Generator().manual_seed(900 + step)
    x = -200.0 * torch.randint(2, 6, (R, V), generator=g).float()
    for r in range(R):
        cols = torch.randperm(V, generator=g)[:6].tolist()
        cols = [c for c in cols if c != eos][:5]
        x[r, cols[:3]] = 0.0
        x[r, cols[3:]] = -200.0
    x[:, eos] = -5000.0
    return x


@pytest.mark.parametrize("cols", [128, 16, 4])
@pytest.mark.parametrize("kind,k,pn,steps", [("autoregressive", 8, 1, 2), ("autoregressive", 1, 1, 4), ("autoregressive", 3, 3, 3),
                                             ("beam", 4, 2, 3)])
def test_merge_tie_order_equals_single_list_twin(cols, kind, k, pn, steps):
    """Equal logits across parts and lanes: the merged order is (value descending, token ascending) -- checked against a stable
    sort at the first step -- and every step's rows, the final tokens and the log-probs equal, bit for bit, those of a twin
    engine that gets the same logits through search_advance (one list per row from row_topm_kernel)."""
    from generativeimage2text_amd.engine import Engine
    a, cfg, _ = _engine("a")
    b, _, _ = _engine("b")
    V, B, P = V_SMALL, 2, 1
    bounds = _bounds(V, -(-V // cols))
    R = B * k
    slots = {1: 1, 2: 2, 3: 4, 4: 4, 8: 8, 9: 16}[max(k, pn) if kind == "autoregressive" else k * pn]
    s = Engine.make_search(kind, P + steps, k, pn, 0.6, num_keep_best=3 if kind == "beam" else 1)
    start = torch.full((B, P), cfg.sos, dtype=torch.int64)
    a.search_begin(s, start, V)
    b.search_begin(s, start, V)
    for step in range(steps):
        rows = a.search_rows().cpu()
        assert torch.equal(rows, b.search_rows().cpu()), step
        x = _tie_logits(R, V, cfg.eos, step)
        ruled = x.clone()
        if kind == "autoregressive" and step > 0:                       # decoder.py:330, as search_advance applies it
            ruled[torch.arange(R), rows[:, -1]] = -10000.0
        a.debug_search_advance_lists(*_cpu_lists(ruled, bounds, slots))
        b.search_advance(x)
        if step == 0:
            order = torch.sort(x[::k], dim=1, descending=True, stable=True).indices[:, :k]
            got = a.search_rows().cpu()[:, -1].reshape(B, k)
            assert torch.equal(got, order), (got, order)
    assert torch.equal(a.search_rows().cpu(), b.search_rows().cpu())
    for u, v in zip(a.search_finish(), b.search_finish()):
        assert torch.equal(u.cpu(), v.cpu()), (u, v)


# ---- C. the head's rules against fp64 --------------------------------------------------------------------------------------------
def _head_operands(V, K, seed):
    """(W [V, K], bias [V]) on the CPU; the 128-column block 2 is pushed below zero, so its best tokens are NEGATIVE logits that
    sit in a candidate list: a penalty that forgets negative logits changes that list."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(V, K, generator=g) * (K ** -0.5 * 2.0)
    bias = torch.randn(V, generator=g) * 0.5
    bias[256:384] -= 12.0
    return W, bias


def _histories(approx, cur_len, V, seed):
    """ids int32 [M, cur_len + 3] (3 columns past cur_len hold a token the rules must not see): duplicates, token 0, token V - 1,
    the best token of the 7-strip tail block, the best two of the all-negative block 2, the row's arg-max and arg-min."""
    M = approx.shape[0]
    g = torch.Generator().manual_seed(seed)
    tail0 = (V - 1) // 128 * 128
    ids = torch.empty(M, cur_len + 3, dtype=torch.int32)
    for r in range(M):
        neg = (approx[r, 256:384].topk(2).indices + 256).tolist()
        pool = [0, V - 1, tail0 + int(approx[r, tail0:].argmax()), neg[0], neg[1], neg[0], int(approx[r].argmax()),
                int(approx[r].argmin()), 0]
        pool = pool[r % len(pool):] + pool[:r % len(pool)]
        rnd = torch.randint(0, V, (max(cur_len - len(pool), 0),), generator=g).tolist()
        hist = (rnd + pool)[-cur_len:] if cur_len >= len(pool) else pool[:cur_len]
        ids[r, :cur_len] = torch.tensor(hist, dtype=torch.int32)
        ids[r, cur_len:] = int(approx[r, :256].argmax())                # beyond the history: must stay unpenalised
    return ids


def _ruled_fp64(lg, ids, cur_len, plen, beams, suppress_kind, rp):
    """The reference's rules on the materialised logits, in fp64: every history token's logit is divided (positive) or multiplied
    (negative) by the penalty once (decoder.py:1135-1144); then the last token goes to -10000 where the no-repeat rule holds.
    -> (ruled logits, bool mask of the entries whose value a penalty produced)."""
    sl = lg.double().clone()
    penalised = torch.zeros(sl.shape, dtype=torch.bool)
    rp64 = float(torch.tensor(rp, dtype=torch.float32))
    for r in range(sl.shape[0]):
        if rp not in (0.0, 1.0):
            for tok in set(ids[r, :cur_len].tolist()):
                sl[r, tok] = sl[r, tok] * rp64 if sl[r, tok] < 0 else sl[r, tok] / rp64
                penalised[r, tok] = True
        if suppress_kind and cur_len > int(plen[r // beams]):
            sl[r, int(ids[r, cur_len - 1])] = -10000.0
            penalised[r, int(ids[r, cur_len - 1])] = False             # -10000 is exact
    return sl, penalised


def _check_rule_lists(sl, pv, pi, pl, mtop, penalised, cols=128):
    """_check_vocab_lists' checks against ruled fp64 logits.  penalised: bool [M, V], the entries a penalty changed (none when it
    is off).  Such an entry is one fp32 multiply or divide by the fp32 penalty away from its fp64 value: 2 ulp (2^-22 relative)
    covers the rounding of either, at a list position that the reference or the kernel fills with one.  Every other entry --
    untouched logits, the -10000 of the no-repeat rule, everything at penalty 1.0 -- is compared exactly."""
    pv, pi, pl = pv.cpu().double(), pi.cpu().long(), pl.cpu().double()
    for p in range(pv.shape[1]):
        blk = sl[:, p * cols:(p + 1) * cols]
        k = min(mtop, blk.shape[1])
        tv, ti = blk.topk(k, dim=1)
        loose = torch.gather(penalised, 1, ti + p * cols) | torch.gather(penalised, 1, pi[:, p, :k])
        tol = torch.where(loose, tv.abs() * 2.0 ** -22, torch.zeros_like(tv))
        assert ((pv[:, p, :k] - tv).abs() <= tol).all(), p
        assert ((torch.gather(sl, 1, pi[:, p, :k]) - tv).abs() <= tol).all(), p
        m = blk.max(1).values
        assert ((pl[:, p, 0] - m).abs() <= tol[:, 0]).all(), p
        assert torch.allclose(pl[:, p, 1], torch.exp(blk - m[:, None]).sum(1), rtol=2e-5, atol=0), p
    got = torch.log((pl[:, :, 1] * torch.exp(pl[:, :, 0] - pl[:, :, 0].max(1, keepdim=True).values)).sum(1)) + pl[:, :, 0].max(1).values
    assert (got - torch.logsumexp(sl, 1)).abs().max().item() < 1e-4


def _check_head_rules(M, beams, V, K, cur_lens, seed):
    from generativeimage2text_amd import engine as E
    W, bias = _head_operands(V, K, seed)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed + 1)) * 1.1 + 0.15
    approx = x.bfloat16().double() @ W.bfloat16().double().t() + bias.double()
    mtop = {1: 1, 2: 4, 4: 8}[beams]
    xd, bd = x.bfloat16().cuda(), bias.cuda()
    Wf, bp = E.to_frag(W.bfloat16().cuda(), 128), E._pad_vec(bd, (V + 127) // 128 * 128)
    Af = E.to_frag(xd, 64)
    # mixed prefix lengths: sentences with cur_len <= plen are on (or before) their first step and must not be suppressed
    for cur_len in cur_lens:
        plen = torch.tensor([(1, cur_len, cur_len + 2, max(cur_len - 1, 1))[s % 4] for s in range(M // beams)], dtype=torch.int32)
        assert (plen >= cur_len).any() and ((plen < cur_len).any() or cur_len == 1)
        ids = _histories(approx, cur_len, V, seed + cur_len)
        for rp in (1.0, 1.3, 0.8):
            for suppress_kind in (1, 0):
                def head(**kw):
                    return E.op_vocab_topm_rules(Af, Wf, bp, mtop, ids.cuda(), cur_len, plen.cuda(), beams, suppress_kind, rp,
                                                 packed=True, rows=M, V=V, **kw)
                pv, pi, pl, lg = head(want_logits=True)
                lg = lg.cpu()
                assert (lg.double() - approx).abs().max().item() < 2e-4 * max(1.0, approx.abs().max().item())   # taken BEFORE the rules
                sl, penalised = _ruled_fp64(lg, ids, cur_len, plen, beams, suppress_kind, rp)
                assert penalised.any() == (rp != 1.0)
                neg_hist = sum(1 for r in range(M) for t in set(ids[r, :cur_len].tolist()) if lg[r, t] < 0)
                assert neg_hist >= M // 3                               # the histories do hold negative logits
                _check_rule_lists(sl, pv, pi, pl, mtop, penalised)
                for max_wgs in (0, 3, 60):                              # the decode-loop kernels where they apply, walked blocks
                    qv, qi, ql, _ = head(want_logits=False, max_wgs=max_wgs)
                    assert torch.equal(qv, pv) and torch.equal(qi, pi) and torch.equal(ql, pl), (cur_len, rp, suppress_kind, max_wgs)


@pytest.mark.parametrize("M,beams", [(12, 4), (70, 1), (130, 2)])
@pytest.mark.parametrize("cur_len", [1, 2, 9, 40])
def test_head_rules_against_fp64(M, beams, cur_len):
    """vocab_topm_kernel with real rule inputs (V = 1000, K = 128): the per-block lists and (max, sum exp) equal the reference's
    rules applied in fp64 to the logits the same launch materialises, for penalties 1.0 / 1.3 / 0.8 with and without the no-repeat
    rule; the launches without logits output (fewer, walking workgroups) give the same lists bit for bit."""
    _check_head_rules(M, beams, V_SMALL, 128, (cur_len,), seed=50 + M)


def test_head_rules_against_fp64_full_vocabulary():
    """The same at V = 30522, K = 768 (239 parts): without a penalty the lists come from the kernels of the decode loop -- the
    one-row-block form (12 rows) and the row-walking form (130 rows) -- with the rule inside them."""
    _check_head_rules(12, 4, 30522, 768, (9,), seed=71)
    _check_head_rules(130, 2, 30522, 768, (2,), seed=72)


def test_head_rules_refuse_long_history_with_penalty():
    from generativeimage2text_amd import engine as E
    x = torch.zeros(4, 128).bfloat16().cuda()
    W = torch.zeros(256, 128).bfloat16().cuda()
    ids = torch.zeros(4, 1030, dtype=torch.int32).cuda()
    plen = torch.ones(4, dtype=torch.int32).cuda()
    with pytest.raises(E.GitmiError, match="repetition penalty"):
        E.op_vocab_topm_rules(x, W, torch.zeros(256).cuda(), 4, ids, 1025, plen, 1, 0, 1.3)
    E.op_vocab_topm_rules(x, W, torch.zeros(256).cuda(), 4, ids, 1025, plen, 1, 1, 1.0)      # no penalty: any length


# ---- D. head -> merge -> search over several steps ----------------------------------------------------------------------------
# name: (V, K, kind, k, pn, num_keep_best, repetition penalty, prefixes, seed).  Seeds were chosen on the CPU (bf16-rounded operands,
# fp64 products) so that the oracle's smallest decision gap is above 2e-3, twice the asserted 1e-3.
CHAIN_T = 8
CHAIN = {
    "greedy": (V_SMALL, 128, "autoregressive", 1, 1, 1, 1.0, [[101]] * 5, 0),
    "ar_beam3_pn3": (V_SMALL, 128, "autoregressive", 3, 3, 1, 1.0, [[101]] * 2, 0),
    "generator_beam4_keep3_rp1.3": (V_SMALL, 128, "beam", 4, 2, 3, 1.3, [[101]] * 2, 1),
    "ar_beam2_prefixes": (V_SMALL, 128, "autoregressive", 2, 2, 1, 1.0, [[101], [101, 7, 999], [101, 640]], 0),
    "ar_beam3_full_vocabulary": (30522, 768, "autoregressive", 3, 3, 1, 1.0, [[101]] * 2, 0),
}


def _chain_model(name):
    V, K, kind, k, pn, nkeep, rp, prefixes, seed = CHAIN[name]
    g = torch.Generator().manual_seed(4000 + seed)
    W = torch.randn(V, K, generator=g) * (K ** -0.5 * 3.0)
    bias = torch.randn(V, generator=g) * 0.5
    bias[O.CONFIGS["TINY"].eos] = -30.0                                  # no sentence ends: eight full steps for every row
    table = torch.randn(1021, K, generator=g)
    return W, bias, table


def _chain_hidden(table, tokens):
    """The hidden row of a beam row from its tokens alone, so that every twin and the oracle see the same input for a history."""
    t = tokens.shape[1]
    pos = torch.arange(t)[None, :]
    return (table[(tokens * 7 + pos * 131) % 1021].sum(1) / math.sqrt(t)).bfloat16()


def _chain_oracle(name, logits_of):
    """The fp64 oracle on logits_of(tokens [n, t]) -> [n, V]: (tokens, log-probs, smallest decision gap)."""
    V, K, kind, k, pn, nkeep, rp, prefixes, seed = CHAIN[name]
    eos = O.CONFIGS["TINY"].eos
    T = min(len(p) for p in prefixes) + CHAIN_T
    step = lambda ids: logits_of(ids).double()
    trace = []
    if kind == "beam":
        start = torch.tensor(prefixes, dtype=torch.int64)
        pred, lp = O.search_generator(start, step, eos, T, k, pn, 0.6, trace=trace, repetition_penalty=rp, num_keep_best=nkeep)
    else:                                                               # every sentence is its own batch-1 call (decoder.py:984-989)
        outs = [O.search_autoregressive(torch.tensor([p], dtype=torch.int64), step, eos, T, k, pn, trace=trace) for p in prefixes]
        assert all(o[0].shape[1] == T for o in outs)
        pred, lp = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    return pred, lp, min(float(t.min()) for t in trace)


@pytest.mark.parametrize("name", sorted(CHAIN))
def test_head_merge_search_chain(name):
    """Eight steps of head lists -> advance_lists -> search_rows: ids identical to the fp64 oracle on the head's materialised
    logits and to a twin fed those logits through search_advance; log-probs within the scripted tests' 1e-4."""
    from generativeimage2text_amd import engine as E
    V, K, kind, k, pn, nkeep, rp, prefixes, seed = CHAIN[name]
    W, bias, table = _chain_model(name)
    Wf, bp = E.to_frag(W.bfloat16().cuda(), 128), E._pad_vec(bias.cuda(), (V + 127) // 128 * 128)
    B, minP = len(prefixes), min(len(p) for p in prefixes)
    T, R = minP + CHAIN_T, len(prefixes) * k
    mtop = max(k, pn) if kind == "autoregressive" else k * pn
    plen = torch.tensor([len(p) for p in prefixes], dtype=torch.int32).cuda()

    def head(tokens, rules, **kw):
        A = E.to_frag(_chain_hidden(table, tokens.cpu()).cuda(), 64)
        ids = tokens.int().cuda() if rules else None
        return E.op_vocab_topm_rules(A, Wf, bp, mtop, ids, tokens.shape[1], plen if rules else None, k,
                                     1 if kind == "autoregressive" else 0, rp, packed=True, rows=tokens.shape[0], V=V, **kw)

    ref_tok, ref_lp, gap = _chain_oracle(name, lambda ids: head(ids, False, want_logits=True)[3].cpu())
    print(f"{name}: smallest decision gap of the oracle {gap:.3e}")
    assert gap > 1e-3, gap                                              # a near-tie in the reference is not a kernel failure

    a, cfg, _ = _engine("a", vocab=V)
    b, _, _ = _engine("b", vocab=V)
    s = E.Engine.make_search(kind, T, k, pn, 0.6, repetition_penalty=rp, num_keep_best=nkeep)
    for eng in (a, b):
        if len(set(len(p) for p in prefixes)) > 1:
            eng.debug_search_begin_prefixed(s, prefixes, V)
        else:
            eng.search_begin(s, torch.tensor(prefixes, dtype=torch.int64), V)
    for _ in range(CHAIN_T):
        rows = a.search_rows()
        assert torch.equal(rows, b.search_rows())
        pv, pi, pl, _ = head(rows, True, want_logits=False)             # K = 768 without a penalty: the decode loop's kernels
        a.debug_search_advance_lists(pv, pi, pl)
        b.search_advance(head(rows, True, want_logits=True)[3])
    ta, la, _ = a.search_finish()
    tb, lb, _ = b.search_finish()
    ta, la, tb, lb = ta.cpu(), la.cpu(), tb.cpu(), lb.cpu()
    assert torch.equal(ta, tb)
    assert torch.equal(ta.reshape(ref_tok.shape), ref_tok), (ta, ref_tok)
    err = max((la.double().reshape(ref_lp.shape) - ref_lp.double()).abs().max().item(), (la - lb).abs().max().item())
    print(f"{name}: log-prob error {err:.2e}")
    assert err < 1e-4, err


# ---- E. the embedding inside the search step ------------------------------------------------------------------------------------
def _embed_ref(w, tok, pos):
    e = w["textual.embedding.words.weight"].double()[tok] + w["textual.embedding.positions.weight"].double()[pos]
    D = e.shape[1]
    return torch.nn.functional.layer_norm(e, (D,), w["textual.embedding.layer_norm.weight"].double(),
                                          w["textual.embedding.layer_norm.bias"].double(), 1e-8)


def _check_hidden(eng, w, rows):
    hf, ht = eng.debug_read_hidden(rows.shape[0])
    ref = _embed_ref(w, rows[:, -1], rows.shape[1] - 1)
    err = (hf.cpu().double() - ref).abs().max().item()
    print(f"embedding D {ref.shape[1]}: fp32 error {err:.2e}")
    assert err < 2e-5, err                                             # test_layernorm's fp32 bound
    assert ht.dtype == torch.bfloat16 and torch.equal(ht.cpu(), hf.cpu().bfloat16())     # the kernel packs the same values


@pytest.mark.parametrize("hidden", [768, 320])
def test_prefill_embedding(hidden):
    """embed_ln_kernel, the embedding of the teacher-forced positions (gitmi_step_logits embeds position after position; the
    search step's fused embedding takes over behind them): one call over t = 3 tokens on encoded frames leaves the rows of the
    last position, LayerNorm(words[token] + positions[2]), the 16-bit copy h_f rounded to the operand type."""
    eng, cfg, w = _engine("p", hidden=hidden, max_batch=4, max_beams=4)
    B, t = 3, 3
    eng.encode([f.cuda() for f in O.make_images(cfg, B, 1, seed=5)], return_features=False)
    g = torch.Generator().manual_seed(hidden + 1)
    rows = torch.randint(0, V_SMALL, (B, t), generator=g, dtype=torch.int64)
    rows[:, 0] = cfg.sos
    rows[0, -1], rows[1, -1] = 0, V_SMALL - 1                       # the first and the last row of the word table
    assert bool(torch.isfinite(eng.step_logits(rows)).all())
    _check_hidden(eng, w, rows)


@pytest.mark.parametrize("hidden", [768, 320])
def test_search_step_embedding(hidden):
    """embed = 1: h_f = LayerNorm(words[token] + positions[position], eps 1e-8) of the tokens the step appended, the 16-bit copy
    (fragment-major, read back row-major) is h_f rounded to the operand type -- the one-row form (greedy: the whole workgroup on
    a row) and the wave-per-row form (beams), D = 768 and a D that ends inside a wave's chunk group, and after a step that
    re-orders the beams: the rows follow the tokens the step selected, not the rows they came from."""
    from generativeimage2text_amd.engine import Engine
    V = V_SMALL
    eng, cfg, w = _engine("e", hidden=hidden, max_batch=4, max_beams=4)
    bounds = _bounds(V, 8)
    g = torch.Generator().manual_seed(hidden)
    # greedy, two steps (positions 1 and 2)
    B = 4
    eng.search_begin(Engine.make_search("autoregressive", 8, 1, 1), torch.full((B, 1), cfg.sos, dtype=torch.int64), V)
    for step in range(2):
        eng.debug_search_advance_lists(*_cpu_lists(torch.randn(B, V, generator=g), bounds, 1), embed=True)
        rows = eng.search_rows().cpu()
        assert rows.shape == (B, 2 + step)
        _check_hidden(eng, w, rows)
    # beam 3: the second step takes all its survivors from the WORST beam of the first (its row is sharply peaked, the others flat)
    B, k = 2, 3
    eng.search_begin(Engine.make_search("autoregressive", 8, k, 3), torch.full((B, 1), cfg.sos, dtype=torch.int64), V)
    eng.debug_search_advance_lists(*_cpu_lists(torch.randn(B * k, V, generator=g), bounds, 4), embed=True)
    rows1 = eng.search_rows().cpu()
    _check_hidden(eng, w, rows1)
    x = 0.01 * torch.randn(B * k, V, generator=g)
    x[:, cfg.eos] = -20.0
    for r in (2, 5):
        peak = [t for t in torch.randperm(V, generator=g).tolist() if t not in (cfg.eos, int(rows1[r, -1]))][:3]
        x[r, peak] = torch.tensor([20.0, 19.0, 18.0])
    x[torch.arange(B * k), rows1[:, -1]] = -10000.0                     # decoder.py:330
    eng.debug_search_advance_lists(*_cpu_lists(x, bounds, 4), embed=True)
    rows2 = eng.search_rows().cpu()
    for bsent in range(B):
        assert torch.equal(rows2[bsent * k:(bsent + 1) * k, :-1], rows1[bsent * k + 2].expand(k, -1)), (rows1, rows2)
    _check_hidden(eng, w, rows2)
