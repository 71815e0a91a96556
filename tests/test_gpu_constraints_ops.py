"""Op-level tests of the decoding-constraint (BAN) instantiations -- vocab_topm_kernel<., VOC_GENERIC, 0, true>,
row_topm_kernel<., ., true> and sample_rows_kernel<true> (csrc/ban_rules.h) -- through the hooks of the measurement build with a
gitmi_debug_ban (include/gitmi_experiment.h).  The definition of "banned" is tools/constrained_step.py (set_mask, ngram_banned,
t - plen < min_new), turned into a bool [rows, V] mask on the CPU; what follows the ban is test_gpu_search_ops._ruled_fp64, the
list checks are _check_rule_lists with its bounds.  A whole-call test sees a ban only where the banned token would have won:
here the stored logits of the head pin every (row, column) of the mask, and the whole-row kernels are held, bit for bit, to
their plain instantiations on logits banned on the CPU."""
import numpy as np
import pytest
import torch

from test_gpu_search_ops import _check_rule_lists, _head_operands, _histories, _ruled_fp64
from test_gpu_select_ops import HIST_CAP, _capacity_case, _colliding_history, _dev, _gen, _rule_logits, _slots
from tools.constrained_step import BANNED, ngram_banned, set_mask

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("experiment_build")]

NEG = float("-inf")


@pytest.fixture(params=["bf16", "f16"])
def operands(request):
    """The measurement library the hooks are called in (libgitmi_exp.so / libgitmi_f16_exp.so)."""
    return request.param


# ---- the reference: sets, tables, histories and the banned mask --------------------------------------------------------------------
# one bit of every nibble of both 16-bit halves of a set word (the head hands lane group lg nibble lg of each half), with every
# position 0..3 inside a nibble taken twice
BIT_K = (1, 6, 11, 12, 19, 20, 25, 30)
SET_RANDOM, SET_BIT0, SET_ONES, SET_ALLOWED, SET_LAST, SET_PAST, SET_EDGES, N_SETS = 0, 1, 9, 10, 11, 12, 13, 14
ALLOWED = (130, 165, 255)                                                # the three tokens SET_ALLOWED leaves, all in block 1


def _words(V, tokens):
    w = [0] * ((V + 31) // 32)
    for t in tokens:
        w[t >> 5] |= 1 << (t & 31)
    return w


def _sets(V, seed, forced):
    """uint32 [N_SETS, W]: 0 random at ~50 % with the tokens `forced`; 1..8 only bit k of every word, k = BIT_K; 9 all ones;
    10 everything but ALLOWED (the allowed_tokens shape); 11 the single token V - 1; 12 only the bits past V of the last word;
    13 tokens 0, 127, 128, V - 1.  Sets 0, 9, 10 and 13 also carry the bits past V."""
    W = (V + 31) // 32
    past = _words(32 * W, range(V, 32 * W))
    rnd = np.random.RandomState(seed).randint(0, 2 ** 32, size=W, dtype=np.uint64).tolist()
    rows = [[a | b | c for a, b, c in zip(rnd, _words(V, forced), past)]]
    rows += [[1 << k] * W for k in BIT_K]
    rows += [[0xffffffff] * W, [0xffffffff & ~a for a in _words(V, ALLOWED)], _words(V, [V - 1]), past,
             [a | b for a, b in zip(_words(V, [0, 127, 128, V - 1]), past)]]
    sets = np.array(rows, dtype=np.uint32)
    assert sets.shape == (N_SETS, W) and (32 * W == V or sets[SET_PAST].any())
    return sets


# sentence recipes (set, length state, takes an n-gram size); recipe 0 is the unconstrained sentence [-1, 0, 0]
RECIPES = ((-1, "off", False), (SET_RANDOM, "below", True), (SET_BIT0, "before", False), (-1, "at", True), (SET_ONES, "off", False),
           (SET_ALLOWED, "above", True), (SET_EDGES, "off", True), (SET_LAST, "below", False))
TRIPLE = 1                                                               # the recipe whose eos is banned, in its set and its last token


def _len_state(state, cur_len, alt):
    """(plen, min_new) with cur_len - plen: "before" -2 (inside the prefix: banned whatever min_new is), "below" min_new - 1,
    "at" min_new, "above" min_new + 1, "off" min_new = 0.  A prefix holds its start token: plen >= 1, so at cur_len = 1
    "above" does not exist and becomes "at"."""
    d = min(3, cur_len - 1)
    if state == "before":
        return cur_len + 2, (0, 2)[alt % 2]
    return cur_len - d, {"off": 0, "below": d + 1, "at": d, "above": max(d - 1, 0)}[state]


def _ngram_sizes(cur_len):
    """The sizes whose edge this history length is: n - 1, n, n + 1 = cur_len; every size for a long history."""
    return list(range(1, 9)) if cur_len >= 40 else [n for n in range(8, 0, -1) if cur_len in (n - 1, n, n + 1)]


def _table(S, cur_len, variant, short=(1, 0, 6)):
    """-> (table [S][3] = [set, min_new, ngram], plen [S], recipe of every sentence).  S >= 8: the recipes in turn, rotated by
    `variant`; fewer sentences: the recipes `short`.  Bit-k sets, "before" states and n-gram sizes are dealt in turn; where
    n = cur_len is among the sizes, the deal starts so that the first sentence with few set bits (recipe 3 or 6) gets it: a single
    start position, whose hit is the only thing that bans the row's arg-max there."""
    recipes = [(s + variant) % 8 for s in range(S)] if S >= 8 else list(short)[:S]
    ns = _ngram_sizes(cur_len)
    takers = [j for j in recipes if RECIPES[j][2]]
    clean = next((i for i, j in enumerate(takers) if j in (3, 6)), None)
    cnt = variant if clean is None or cur_len not in ns else ns.index(cur_len) - clean + len(ns) * len(takers)
    table, plen = [], []
    for s, j in enumerate(recipes):
        si, state, wants_n = RECIPES[j]
        if si == SET_BIT0:
            si += (s // 8 + variant) % 8
        if si == SET_LAST and (s // 8) % 2:
            si = SET_PAST
        p, min_new = _len_state(state, cur_len, s // 8)
        n = 0
        if wants_n:
            n, cnt = ns[cnt % len(ns)], cnt + 1
        table.append([si, min_new, n])
        plen.append(p)
    assert [-1, 0, 0] in table
    assert all(table[s] != table[s + 1] for s in range(S - 1))            # neighbouring sentences differ
    return table, torch.tensor(plen, dtype=torch.int32), recipes


def _ban_histories(approx, V, beams, cur_len, table, recipes, eos, seed):
    """ids int32 [M, cur_len + 3]: _histories, and on the rows of a sentence with an n-gram size n <= cur_len a history that bans
    the row's arg-max a -- by row in turn: a run of one token; two earlier occurrences of the tail followed by a and by a token
    of another 128-column block (one of the two in the tail block), where 3 n - 1 tokens fit, else a history of period 2;
    a history of period 3 (periods are cut to cur_len - n + 1, the number of start positions: at cur_len = n only the run is
    left, one start position whose window overlaps the tail).  The columns past cur_len of every n-gram row hold the row's
    second-best token, which a window that began one position too late would ban.  The row of a TRIPLE sentence whose arg-max
    is eos holds a run of eos: eos is its last token."""
    M, t = approx.shape[0], cur_len
    ids = _histories(approx, t, V, seed)
    g = _gen(seed + 1)
    tail0 = (V - 1) // 128 * 128
    for r in range(M):
        s = r // beams
        n = table[s][2]
        a, b2 = approx[r].topk(2).indices.tolist()
        eos_row = recipes[s] == TRIPLE and a == eos
        if n > 0:
            ids[r, t:] = b2
        if 0 < n <= t:
            fresh = [c for c in torch.randperm(V, generator=g)[:64].tolist() if c not in (a, b2, eos)]
            kind = 0 if eos_row else r % 3
            if kind == 1 and 3 * n - 1 <= t:
                in_tail = approx[r, tail0:].clone()
                in_tail[eos - tail0] = NEG                              # eos is left to the length rule
                v = tail0 + int(in_tail.argmax())
                if a >= tail0:
                    v = int(approx[r, :128].argmax())
                assert a // 128 != v // 128 and (a >= tail0 or v >= tail0)
                tail = fresh[:n - 1]
                body = tail + [a] + tail + [v] + tail
                other = fresh[n - 1:]                                   # the tail's tokens occur in the body only
                hist = [other[j % len(other)] for j in range(t - len(body))] + body
            else:
                d = 1 if kind == 0 else min(kind + 1, t - n + 1)
                base = fresh[:d]
                base[t % d] = a                                         # the banned token is x[t - d]
                hist = [base[j % d] for j in range(t)]
            assert len(hist) == t
            ids[r, :t] = torch.tensor(hist, dtype=torch.int32)
        if eos_row:
            ids[r, t - 1] = eos
    return ids


def _banned_mask(sets, table, eos, plen, beams, ids, cur_len, V):
    """tools/constrained_step.wrap_step's three rules for (sets, table, eos, plen, beams, ids, cur_len) -> (bool [R, V] banned,
    {"set" | "len" | "ngram": bool [R, V]} what each rule bans on its own)."""
    R = ids.shape[0]
    kinds = {k: torch.zeros(R, V, dtype=torch.bool) for k in ("set", "len", "ngram")}
    masks = [set_mask(w, V) for w in sets]
    for r in range(R):
        si, min_new, n = table[r // beams]
        if si >= 0:
            kinds["set"][r] = masks[si]
        if cur_len - int(plen[r // beams]) < min_new:
            kinds["len"][r, eos] = True
        for c in ngram_banned(ids[r, :cur_len].tolist(), n):
            kinds["ngram"][r, c] = True
    return kinds["set"] | kinds["len"] | kinds["ngram"], kinds


def _assert_not_vacuous(kinds, plain, table, cur_len, beams):
    """On the reference only: every rule kind that can fire in this case bans the PLAIN arg-max of at least one row."""
    am = plain.argmax(1)
    rows = torch.arange(plain.shape[0])
    active = {"set": any(si >= 0 and si != SET_PAST for si, _, _ in table), "len": bool(kinds["len"].any()),
              "ngram": any(0 < n <= cur_len for _, _, n in table)}
    for kind, on in active.items():
        assert not on or kinds[kind][rows, am].any(), kind
    return active


def _ban_dev(sets, table, eos):
    from generativeimage2text_amd import engine as E
    words = torch.from_numpy(sets.view(np.int32).copy()).cuda()
    tab = torch.tensor(table, dtype=torch.int32).t().contiguous().cuda()
    return E.DebugBan(words, sets.shape[0], sets.shape[1], tab[0], tab[1], tab[2], eos)


def _free_rows(table, beams):
    return torch.tensor([r for s, row in enumerate(table) if row == [-1, 0, 0] for r in range(s * beams, (s + 1) * beams)])


def _check_ruled_lists(lg, ids, cur_len, plen, beams, suppress_kind, rp, pv, pi, pl, mtop, cols):
    """_check_rule_lists against _ruled_fp64 of the banned logits lg, on every row it can judge.  It cannot judge a row whose
    MAXIMUM is a penalised -10000 (every logit banned, penalty below 1: history tokens at -8000): fp32 has no value within its
    1e-4 of the fp64 log-sum-exp there (-10000 x fp32(0.8) = -8000.000119; fp32 is spaced 4.9e-4 apart at 8000).  Such a row
    is held to MORE: all its logits are negative, so the penalty is one correctly rounded fp32 multiply and the ruled row is
    determinate in fp32 -- lists (stable descending sort) and block maxima must equal it bit for bit, the sums within the
    helper's rtol of 2e-5.  That fp32 row is itself checked against _ruled_fp64 within the helper's 2 ulp.
    -> (ruled fp64 logits, penalised mask, largest log-sum-exp error of the rows _check_rule_lists judged)"""
    sl, penalised = _ruled_fp64(lg, ids, cur_len, plen, beams, suppress_kind, rp)
    top = sl.max(1)
    deep = (top.values < -1000.0) & penalised[torch.arange(sl.shape[0]), top.indices]
    assert not deep.any() or rp < 1.0
    sh = (~deep).nonzero()[:, 0]
    pv, pi, pl = pv.cpu(), pi.cpu(), pl.cpu()
    _check_rule_lists(sl[sh], pv[sh], pi[sh], pl[sh], mtop, penalised[sh], cols=cols)
    m = pl[sh][:, :, 0].double().max(1, keepdim=True).values
    got = torch.log((pl[sh][:, :, 1].double() * torch.exp(pl[sh][:, :, 0].double() - m)).sum(1)) + m[:, 0]
    err = (got - torch.logsumexp(sl[sh], 1)).abs().max().item()
    for r in deep.nonzero()[:, 0].tolist():
        assert (lg[r] < 0).all()
        row = lg[r].clone()
        hist = torch.tensor(sorted(set(ids[r, :cur_len].tolist())))
        row[hist] = row[hist] * torch.tensor(rp, dtype=torch.float32)
        if suppress_kind and cur_len > int(plen[r // beams]):
            row[int(ids[r, cur_len - 1])] = BANNED
        assert ((row.double() - sl[r]).abs() <= sl[r].abs() * 2.0 ** -22).all()
        for p in range(pv.shape[1]):
            blk = row[p * cols:(p + 1) * cols]
            k = min(mtop, blk.numel())
            o = torch.sort(blk, descending=True, stable=True)
            assert torch.equal(pv[r, p, :k], o.values[:k]) and torch.equal(pi[r, p, :k].long(), o.indices[:k] + p * cols), (r, p)
            assert pl[r, p, 0] == o.values[0], (r, p)
            assert torch.allclose(pl[r, p, 1].double(), torch.exp(blk.double() - o.values[0].double()).sum(), rtol=2e-5, atol=0), (r, p)
    return sl, penalised, err


# ---- A. the head ------------------------------------------------------------------------------------------------------------------------
def _check_tie_blocks(sl, pv, pi, pl, mtop, rows, V):
    """Rows whose set bans (almost) a whole block, no penalty: the ruled values are exact, so the list of every block is THE stable
    descending sort -- the -10000 entries in ascending token order from the block's first banned column -- and an all-banned
    block has (max, sum exp) = (-10000, its columns below V)."""
    pv, pi, pl = pv.cpu(), pi.cpu().long(), pl.cpu()
    seen_all_banned = False
    for p in range(pv.shape[1]):
        a, b = p * 128, min(V, (p + 1) * 128)
        k = min(mtop, b - a)
        blk = sl[rows, a:b]
        o = torch.sort(blk, dim=1, descending=True, stable=True)
        assert torch.equal(pi[rows, p, :k], o.indices[:, :k] + a), p
        assert torch.equal(pv[rows, p, :k].double(), o.values[:, :k]), p
        full = (blk == BANNED).all(1)
        seen_all_banned |= bool(full.any())
        want = torch.tensor([BANNED, float(b - a)]).expand(int(full.sum()), 2)
        assert torch.equal(pl[rows[full], p], want), p
    assert seen_all_banned


def _check_head_ban(operands, V, K, M, beams, cur_len, mtop, variant, rps=(1.0, 1.3, 0.8), short=(1, 0, 6), seed=50):
    from generativeimage2text_amd import engine as E
    dt = torch.bfloat16 if operands == "bf16" else torch.float16
    S, eos = M // beams, V - 2                                           # eos in the tail block
    table, plen, recipes = _table(S, cur_len, variant, short)
    triple_row = recipes.index(TRIPLE) * beams
    W, bias = _head_operands(V, K, seed + M)
    x = torch.randn(M, K, generator=_gen(seed + M + 1)) * 1.1 + 0.15
    x[triple_row] += 5.0 * W[eos]                                        # |W[eos]|^2 ~ 4: eos is this row's plain arg-max
    approx = x.to(dt).double() @ W.to(dt).double().t() + bias.double()
    ids = _ban_histories(approx, V, beams, cur_len, table, recipes, eos, seed + cur_len)
    sets = _sets(V, seed + V, [int(approx[triple_row].argmax()), eos])
    banned, kinds = _banned_mask(sets, table, eos, plen, beams, ids, cur_len, V)
    ban = _ban_dev(sets, table, eos)
    free = _free_rows(table, beams)
    ties = torch.tensor([r for r in range(M) if table[r // beams][0] in (SET_ONES, SET_ALLOWED)])
    Wf, bp = E.to_frag(W.to(dt).cuda(), 128), E._pad_vec(bias.cuda(), (V + 127) // 128 * 128)
    Af = E.to_frag(x.to(dt).cuda(), 64)
    ids_d, plen_d = ids.cuda(), plen.cuda()
    active, worst = None, 0.0
    for rp in rps:
        for suppress_kind in (1, 0):
            def head(**kw):
                return E.op_vocab_topm_rules(Af, Wf, bp, mtop, ids_d, cur_len, plen_d, beams, suppress_kind, rp, packed=True, rows=M,
                                             V=V, **kw)
            pv0, pi0, pl0, lg0 = head(want_logits=True)
            pv, pi, pl, lg = head(want_logits=True, ban=ban)
            lg0, lg = lg0.cpu(), lg.cpu()
            if active is None:
                assert (lg0.double() - approx).abs().max().item() < 2e-4 * max(1.0, approx.abs().max().item())
                active = _assert_not_vacuous(kinds, lg0, table, cur_len, beams)
                assert int(lg0[triple_row].argmax()) == eos and banned[triple_row, eos] and kinds["set"][triple_row, eos]
            # the column -> bit map, every (row, column) at once: the stored logits carry the ban and nothing else
            want = torch.where(banned, torch.tensor(BANNED), lg0)
            assert torch.equal(lg, want), (cur_len, rp, suppress_kind, (lg != want).nonzero()[:8].tolist())
            sl, penalised, err = _check_ruled_lists(lg, ids, cur_len, plen, beams, suppress_kind, rp, pv, pi, pl, mtop, 128)
            assert penalised.any() == (rp != 1.0)
            worst = max(worst, err)
            if rp == 1.0 and len(ties):
                _check_tie_blocks(sl, pv, pi, pl, mtop, ties, V)
            for max_wgs in (0, 3, 60):
                qv, qi, ql, _ = head(want_logits=False, max_wgs=max_wgs, ban=ban)
                assert torch.equal(qv, pv) and torch.equal(qi, pi) and torch.equal(ql, pl), (cur_len, rp, suppress_kind, max_wgs)
            # independence: unconstrained sentences get what the same launch without tables gives them
            fr = free.cuda()
            assert torch.equal(pv[fr], pv0[fr]) and torch.equal(pi[fr], pi0[fr]) and torch.equal(pl[fr], pl0[fr])
            assert torch.equal(lg[free], lg0[free])
    print(f"head ban {operands} V {V} rows {M} beams {beams} cur_len {cur_len} mtop {mtop}: active {active}, banned per row "
          f"{int(banned.sum(1).min())}..{int(banned.sum(1).max())}, log-sum-exp error {worst:.2e} (bound 1e-4)")


# (V, rows): mtop, so that the five BAN instantiations of the head are launched
HEAD_MTOP = {(1000, 12): 8, (1000, 70): 1, (1000, 130): 4, (937, 12): 16, (937, 70): 2, (937, 130): 8}
# recipes of the three sentences of the (12, 4) shape, by cur_len in turn
HEAD_SHORT = ((1, 0, 6), (5, 0, 1), (1, 0, 4), (3, 0, 1), (7, 1, 0), (2, 0, 1))
HEAD_CUR_LENS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 40]


@pytest.mark.parametrize("M,beams", [(12, 4), (70, 1), (130, 2)])
@pytest.mark.parametrize("V", [1000, 937])
@pytest.mark.parametrize("cur_len", HEAD_CUR_LENS)
def test_head_ban_against_reference(operands, cur_len, V, M, beams):
    """vocab_topm_kernel<mtop, VOC_GENERIC, 0, true> (K = 128; V = 937: an odd vocabulary whose W = 30 set words put every set but
    the first at a word offset that is no multiple of the block's four): the logits a constrained launch stores equal, bit for
    bit, the plain launch's with -10000 on the reference's banned mask; lists and (max, sum exp) equal the reference's rules in
    fp64 on those logits at penalties 1.0 / 1.3 / 0.8 with and without the no-repeat rule; whole-banned blocks list their first
    columns in order; the walking launches return the same lists; unconstrained sentences are untouched.  cur_len 1..9 are the
    n-gram rule's edges n - 1, n, n + 1 for n = 1..8, cur_len 40 carries every n."""
    i = HEAD_CUR_LENS.index(cur_len)
    _check_head_ban(operands, V, 128, M, beams, cur_len, HEAD_MTOP[V, M], variant=i, short=HEAD_SHORT[i % len(HEAD_SHORT)])


@pytest.mark.parametrize("cur_len", [300, 1025])
def test_head_ban_long_history(operands, cur_len):
    """The head walks ids for the n-gram rule and keeps no set of them: a constrained call has no cap on cur_len (the
    repetition penalty has its own: off here past 1024 tokens)."""
    _check_head_ban(operands, 1000, 128, 12, 4, cur_len, 4, variant=2, rps=(1.0, 1.3) if cur_len <= HIST_CAP else (1.0,))


@pytest.mark.parametrize("M,beams,cur_len,mtop", [(12, 4, 9, 8), (130, 2, 2, 4)])
def test_head_ban_full_vocabulary(operands, M, beams, cur_len, mtop):
    """V = 30522, K = 768 (239 parts, W = 954 with six bits past the vocabulary): one row block and the row-block walk; a set with
    tokens 0, 127, 128 and 30521 (SET_EDGES) among the sentences', eos in the 58-column tail block."""
    _check_head_ban(operands, 30522, 768, M, beams, cur_len, mtop, variant=0, short=(1, 0, 6), seed=71)


# ---- B. row_topm ------------------------------------------------------------------------------------------------------------------------
def _whole_row_case(V, R, beams, cur_len, variant, seed, short=(1, 0, 6, 2), scale=None):
    """Logits [R, V] (test_gpu_select_ops._rule_logits), table, histories, sets and the banned mask for the whole-row kernels;
    eos = V - 2 is the plain arg-max of the TRIPLE sentence's first row, and the runner-up of the first row of every sentence
    that has just reached its min_new (recipe 3: eos must stay; the row's arg-max is what its history bans)."""
    eos = V - 2
    table, plen, recipes = _table(R // beams, cur_len, variant, short)
    x = _rule_logits(R, V, seed) if scale is None else torch.randn(R, V, generator=_gen(seed)) * scale
    triple_row = recipes.index(TRIPLE) * beams
    x[triple_row, eos] = x[triple_row].max() + 5.0
    for s, j in enumerate(recipes):
        if j == 3:
            x[s * beams, eos] = x[s * beams].topk(2).values.mean()
    ids = _ban_histories(x.double(), V, beams, cur_len, table, recipes, eos, seed + cur_len)
    sets = _sets(V, seed + 1, [eos])
    banned, kinds = _banned_mask(sets, table, eos, plen, beams, ids, cur_len, V)
    active = _assert_not_vacuous(kinds, x, table, cur_len, beams)
    return x, table, plen, ids, sets, banned, eos, active


@pytest.mark.parametrize("V,ldl,off", [(30522, 30524, 0), (30522, 30524, 1), (1000, 1000, 0)])
@pytest.mark.parametrize("M", [1, 2, 4, 8, 16])
def test_row_topm_ban_equals_banned_logits(operands, M, V, ldl, off):
    """row_topm_kernel<MMAX, NT, true>, every (MMAX, NT), on the 16-byte and the scalar load path: lists and (max, sum exp) of
    row_topm(x, ban) equal, bit for bit, those of the plain kernel on logits banned on the CPU, under the same histories, penalty
    and no-repeat rule -- and the reference's rules in fp64.  A banned history token is penalised AFTER the ban (-10000 x 1.3,
    -10000 x 0.8: the maximum of an all-banned row), an unbanned one is penalised and not banned."""
    from generativeimage2text_amd import engine as E
    R, beams, slots = 16, 2, _slots(M)
    worst = 0.0
    for cur_len in (3, 40):
        x, table, plen, ids, sets, banned, eos, active = _whole_row_case(V, R, beams, cur_len, cur_len + M, 500 + V + M)
        assert all(active.values()), active
        ban = _ban_dev(sets, table, eos)
        xb = torch.where(banned, torch.tensor(BANNED), x)
        d, db = _dev(x, ldl, off), _dev(xb, ldl, off)
        ids_d, plen_d = ids.cuda(), plen.cuda()
        free = _free_rows(table, beams)
        for rp in (1.0, 1.3, 0.8):
            for suppress_kind in (1, 0):
                args = (ids_d, cur_len, plen_d, beams, suppress_kind, rp)
                pv, pi, pl = E.op_row_topm(d, V, M, *args, operands=operands, ban=ban)
                qv, qi, ql = E.op_row_topm(db, V, M, *args, operands=operands)
                assert torch.equal(pv, qv) and torch.equal(pi, qi) and torch.equal(pl, ql), (cur_len, rp, suppress_kind)
                sl, penalised, err = _check_ruled_lists(xb, ids, cur_len, plen, beams, suppress_kind, rp, pv[:, None], pi[:, None],
                                                        pl[:, None], slots, V)
                worst = max(worst, err)
                if rp != 1.0:
                    assert (penalised & banned).any() and (penalised & ~banned).any()
                    ones = [r for r in range(R) if table[r // beams][0] == SET_ONES]
                    assert ones and all((sl[r].max().item() > BANNED) == (rp < 1.0) or suppress_kind for r in ones)
                fv, fi, fl = E.op_row_topm(d, V, M, *args, operands=operands)
                fr = free.cuda()
                assert torch.equal(pv[fr], fv[fr]) and torch.equal(pi[fr], fi[fr]) and torch.equal(pl[fr], fl[fr])
    print(f"row_topm ban {operands} M {M} V {V} ldl {ldl} off {off}: log-sum-exp error {worst:.2e} (bound 1e-4)")


def test_row_topm_ban_table_at_capacity(operands):
    """s_ban_tbl beside s_hist, both at 1024 distinct tokens with colliding hashes (test_gpu_select_ops._colliding_history):
    ngram = 1 bans the whole history and none of the outsiders that hash into the same probe runs."""
    from generativeimage2text_amd import engine as E
    V, ldl, R, M = 30522, 30524, 4, 16
    hist, outsiders, _, _ = _colliding_history(V)
    x, ids = _capacity_case(V, R, 41)
    table = [[-1, 0, 1], [-1, 0, 1], [-1, 0, 1], [-1, 0, 0]]
    plen = torch.ones(R, dtype=torch.int32)
    sets = _sets(V, 3, [])
    banned, kinds = _banned_mask(sets, table, V - 2, plen, 1, ids, HIST_CAP, V)
    assert banned.sum(1).tolist() == [HIST_CAP] * 3 + [0] and banned[:3][:, list(hist)].all() and not banned[:, list(outsiders)].any()
    assert kinds["ngram"][torch.arange(3), x[:3].argmax(1)].any()
    ban = _ban_dev(sets, table, V - 2)
    xb = torch.where(banned, torch.tensor(BANNED), x)
    d, db = _dev(x, ldl), _dev(xb, ldl)
    for rp in (1.0, 1.3):
        args = (ids.cuda(), HIST_CAP, plen.cuda(), 1, 1, rp)
        pv, pi, pl = E.op_row_topm(d, V, M, *args, operands=operands, ban=ban)
        qv, qi, ql = E.op_row_topm(db, V, M, *args, operands=operands)
        assert torch.equal(pv, qv) and torch.equal(pi, qi) and torch.equal(pl, ql), rp
        sl, penalised = _ruled_fp64(xb, ids, HIST_CAP, plen, 1, 1, rp)
        _check_rule_lists(sl, pv[:, None], pi[:, None], pl[:, None], 16, penalised, cols=V)
        got = pi.cpu().long()
        assert not torch.gather(banned, 1, got).any()                    # no member of the history is listed ...
        assert all(set(outsiders[:8]) <= set(got[r].tolist()) for r in range(3))      # ... the planted outsiders all are
        fv, fi, fl = E.op_row_topm(d, V, M, *args, operands=operands)
        assert torch.equal(pv[3], fv[3]) and torch.equal(pi[3], fi[3]) and torch.equal(pl[3], fl[3])


def _sentinels(*shapes):
    return tuple(torch.full(s, -7, dtype=dt).cuda() for s, dt in shapes)


def test_row_topm_ban_refuses_a_history_past_capacity(operands):
    from generativeimage2text_amd import engine as E
    V, R = 1000, 2
    x = _rule_logits(R, V, 9)
    ids = torch.randint(0, V, (R, HIST_CAP + 4), generator=_gen(2), dtype=torch.int32).cuda()
    plen = torch.ones(R, dtype=torch.int32).cuda()
    ban = _ban_dev(_sets(V, 1, []), [[0, 0, 2], [-1, 0, 0]], V - 2)
    out = _sentinels(((R, 4), torch.float32), ((R, 4), torch.int32), ((R, 2), torch.float32))
    with pytest.raises(E.GitmiError, match="invalid argument"):
        E.op_row_topm(_dev(x, V), V, 4, ids, HIST_CAP + 1, plen, 1, 1, 1.0, out=out, operands=operands, ban=ban)
    torch.cuda.synchronize()
    assert all((o == -7).all().item() for o in out)
    E.op_row_topm(_dev(x, V), V, 4, ids, HIST_CAP, plen, 1, 1, 1.0, out=out, operands=operands, ban=ban)      # at the capacity: runs
    assert (out[1] != -7).all().item()


# ---- C. sample_rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [30522, 32768])
@pytest.mark.parametrize("top_k,top_p", [(50, 1.0), (0, 0.9)])
def test_sample_rows_ban_equals_banned_logits(operands, top_k, top_p, V):
    """sample_rows_kernel<true> at temperature 0.7, with and without the repetition penalty: filtered logits, draws and their
    log-probs equal, bit for bit, the plain kernel's on logits banned on the CPU at the same (seed, step); no banned token is
    kept or drawn; unconstrained sentences equal the launch without tables.  The sets leave thousands of tokens (random, the
    four edge tokens, none), so no -10000 can be among the kept; one sentence is inside min_new, one has just reached it."""
    from generativeimage2text_amd import engine as E
    R, beams, cur_len, ndraw, stride = 8, 2, 8, 3, 4                        # n = 8 = cur_len on the SET_EDGES sentence, n = 7 on the other
    x, table, plen, ids, sets, banned, eos, active = _whole_row_case(V, R, beams, cur_len, 0, 700 + V, short=(1, 0, 6, 3), scale=3.0)
    assert all(active.values()), active
    assert not banned[6, eos] and x[6].topk(2).indices[1] == eos          # the sentence at its min_new keeps eos
    ban = _ban_dev(sets, table, eos)
    xb = torch.where(banned, torch.tensor(BANNED), x)
    d, db = _dev(x, V), _dev(xb, V)
    ids_d, plen_d = ids.cuda(), plen.cuda()
    free = _free_rows(table, beams)
    for rp in (0.0, 1.3):
        kw = dict(seed=5, step=2, stride=stride, ids=ids_d, cur_len=cur_len, rep_penalty=rp, operands=operands)
        filt, tok, lp = E.op_sample_rows_rules(d, V, 0.7, top_k, top_p, ndraw, plen=plen_d, beams=beams, ban=ban, **kw)
        filt2, tok2, lp2 = E.op_sample_rows_rules(db, V, 0.7, top_k, top_p, ndraw, **kw)
        assert torch.equal(filt, filt2) and torch.equal(tok, tok2) and torch.equal(lp, lp2), rp
        filt, tok, lp = filt.cpu(), tok.cpu().long(), lp.cpu()
        assert (filt[banned] == NEG).all() and filt[6, eos] > NEG
        kept = torch.isfinite(filt)
        assert (kept.sum(1) >= 3).all() and not torch.gather(banned, 1, tok[:, :ndraw]).any()
        assert torch.gather(kept, 1, tok[:, :ndraw]).all() and torch.isfinite(lp[:, :ndraw]).all()
        filt0, tok0, lp0 = E.op_sample_rows_rules(d, V, 0.7, top_k, top_p, ndraw, **kw)
        assert torch.equal(filt[free], filt0.cpu()[free]) and torch.equal(tok[free], tok0.cpu().long()[free])
        assert torch.equal(lp[free], lp0.cpu()[free])
        print(f"sample_rows ban {operands} V {V} k {top_k} p {top_p} penalty {rp}: kept {kept.sum(1).tolist()}, banned "
              f"{banned.sum(1).tolist()}")


def test_sample_rows_ban_refusals(operands):
    from generativeimage2text_amd import engine as E
    V, R = 3000, 2
    x = torch.randn(R, V, generator=_gen(1)).cuda()
    ids = torch.randint(0, 1000, (R, HIST_CAP + 4), generator=_gen(2), dtype=torch.int32).cuda()
    plen = torch.ones(R, dtype=torch.int32).cuda()
    ban = _ban_dev(_sets(V, 1, []), [[0, 0, 2], [-1, 0, 0]], V - 2)
    out = _sentinels(((R, 2), torch.float32), ((R, 2), torch.int32), ((R, V), torch.float32))
    kw = dict(top_k=50, top_p=0.9, ndraw=2, stride=2, out=out, operands=operands, ban=ban)
    with pytest.raises(E.GitmiError, match="invalid argument"):
        E.op_sample_rows_rules(x, V, ids=ids, cur_len=HIST_CAP + 1, plen=plen, **kw)
    with pytest.raises(E.GitmiError, match="ban without ids or plen"):
        E.op_sample_rows_rules(x, V, ids=ids, cur_len=9, plen=None, **kw)
    with pytest.raises(E.GitmiError, match="ban without ids or plen"):
        E.op_sample_rows_rules(x, V, ids=None, cur_len=9, plen=plen, **kw)
    torch.cuda.synchronize()
    assert all((o == -7).all().item() for o in out)


# ---- D. what the hooks refuse -------------------------------------------------------------------------------------------------------------
def _bad_bans(V, S):
    """(the hook's message, DebugBan) for every table the hooks refuse; S sentences."""
    from generativeimage2text_amd import engine as E
    W = (V + 31) // 32
    words = torch.zeros(3, W, dtype=torch.int32).cuda()
    col = lambda v, first=None: torch.tensor([v if first is None else first] + [v] * (S - 1), dtype=torch.int32).cuda()
    ok = dict(words=words, n_sets=3, W=W, set_of=col(0), min_new=col(0), ngram=col(0), eos=V - 1)
    bad = (("W=", dict(W=W + 1)), ("W=", dict(W=W - 1)), ("n_sets=-1", dict(n_sets=-1)), ("null table", dict(set_of=None)),
           ("null table", dict(min_new=None)), ("null table", dict(ngram=None)), ("words are null", dict(words=None, set_of=col(-1, 2))),
           (r"set_of\[0\]=3 outside", dict(set_of=col(0, 3))), (r"set_of\[0\]=-2 outside", dict(set_of=col(0, -2))),
           (r"min_new\[0\]=-1 is negative", dict(min_new=col(0, -1))), (r"ngram\[0\]=9 outside", dict(ngram=col(0, 9))),
           (r"ngram\[0\]=-1 outside", dict(ngram=col(0, -1))), ("eos=-1 outside", dict(eos=-1)), (f"eos={V} outside", dict(eos=V)))
    return [(what, E.DebugBan(**{**ok, **kw})) for what, kw in bad] + [(None, E.DebugBan(**{**ok, "words": None, "set_of": col(-1)}))]


def test_hooks_refuse_bad_ban_tables(operands):
    """Every refusal of gitmi_debug_ban by name, in each of the three hooks, nothing written; a table without any set needs no
    words and runs."""
    from generativeimage2text_amd import engine as E
    V, R, beams, K = 1000, 4, 2, 128
    dt = torch.bfloat16 if operands == "bf16" else torch.float16
    x = _rule_logits(R, V, 9)
    d = _dev(x, V)
    ids = torch.randint(0, V, (R, 12), generator=_gen(2), dtype=torch.int32).cuda()
    plen = torch.ones(R // beams, dtype=torch.int32).cuda()
    A, Wt, bias = torch.zeros(R, K).to(dt).cuda(), torch.zeros(V, K).to(dt).cuda(), torch.zeros(V).cuda()

    def head(ban, out, ids=ids, plen=plen):
        E.op_vocab_topm_rules(A, Wt, bias, 4, ids, 9, plen, beams, 1, 1.0, ban=ban, out=out)

    def topm(ban, out, ids=ids, plen=plen):
        E.op_row_topm(d, V, 4, ids, 9, plen, beams, 1, 1.0, out=out, operands=operands, ban=ban)

    def sample(ban, out, ids=ids, plen=plen):
        E.op_sample_rows_rules(d, V, 0.7, 50, 0.9, 2, stride=4, ids=ids, cur_len=9, out=out, operands=operands, plen=plen, beams=beams,
                               ban=ban)
    nparts = (V + 127) // 128
    outs = {head: _sentinels(((R, nparts, 4), torch.float32), ((R, nparts, 4), torch.int32), ((R, nparts, 2), torch.float32)) + (None,),
            topm: _sentinels(((R, 4), torch.float32), ((R, 4), torch.int32), ((R, 2), torch.float32)),
            sample: _sentinels(((R, 4), torch.float32), ((R, 4), torch.int32), ((R, V), torch.float32))}
    cases = _bad_bans(V, R // beams)
    for hook, out in outs.items():
        for what, ban in cases[:-1]:
            with pytest.raises(E.GitmiError, match=what):
                hook(ban, out)
        with pytest.raises(E.GitmiError, match="ban without ids or plen"):
            hook(cases[-1][1], out, ids=None, plen=None if hook is not head else plen)
        torch.cuda.synchronize()
        assert all((o == -7).all().item() for o in out if o is not None), hook.__name__
        hook(cases[-1][1], out)                                          # set_of all -1, words null: nothing to refuse
        torch.cuda.synchronize()
        assert (out[1] != -7).all().item(), hook.__name__
