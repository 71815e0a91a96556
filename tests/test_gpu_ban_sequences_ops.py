"""Op-level tests of banned token sequences (csrc/ban_rules.h, the sequence rule): ban_rows_kernel through the row_words_out form of gitmi_debug_row_topm
(engine.op_ban_rows), and the three consumers -- the fused head, row_topm, sample_rows -- with gitmi_debug_ban.row_words set.  The definition is
tools/constrained_step.sequence_banned / set_mask on the CPU.  The rule is integer logic: every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_search_ops import _head_operands
from test_gpu_select_ops import _gen, _rule_logits
from tools.constrained_step import BANNED, sequence_banned

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("experiment_build")]

SENTINEL = 0x5a5a5a5a
SEQ_CAP = 4096


@pytest.fixture(params=["bf16", "f16"])
def operands(request):
    return request.param


def _pack(V, tokens, W=None):
    W = (V + 31) // 32 if W is None else W
    w = np.zeros(W, dtype=np.uint32)
    for t in tokens:
        w[t >> 5] |= np.uint32(1 << (t & 31))
    return w


def _case(V, seed):
    """Four sentences: 0 list 0 + static set 0; 1 no list (-1) + static set 1; 2 list 0, no static set; 3 list 1 (fills the
    sequence cap) + static set 0.  List 0: lengths 2, 3, 16; (A, C, D) and (A, C, E) share a head; (A, B) and (G, A, B) share their
    last token B (bit 0 of a word); D is bit 31 of a word; the 16-token sequence ends in V - 1, the last bit of the last word used;
    one sequence ends in a token of the last word whose set bits past V must survive."""
    from generativeimage2text_amd import engine as E
    W = (V + 31) // 32
    A, B, C, D, Ee, G = 5, 64, 7, 95, 96, 9
    long16 = [300 + i for i in range(15)] + [V - 1]
    list0 = [[A, B], [A, C, D], [A, C, Ee], [G, A, B], long16, [11, 12, 32 * (W - 1)]]
    g = np.random.RandomState(seed)
    n1 = SEQ_CAP - len(list0)
    heads = g.permutation(np.arange(400, V - 40))[:64]
    list1 = [[int(heads[i % 64]), 400 + i // 64] for i in range(n1)]            # distinct pairs up to the cap
    lists = [list0, list1]
    per = [list0, None, list0, list1]
    singles, pool = E.banned_sequence_tables(4, V, per)
    assert singles == [None] * 4 and pool[0] == 2 and pool[1] == SEQ_CAP and pool[4:8].tolist() == [0, -1, 0, 1]
    past = list(range(V, 32 * W))
    sets = np.stack([_pack(32 * W, [0, 1, 127, 128, V - 2] + past, W), _pack(32 * W, [3, 33, V - 1] + past, W)])
    set_of = [0, 1, -1, 0]
    return lists, [0, -1, 0, 1], pool, sets, set_of, heads


def _histories(V, t, beams, lists, heads, seed, force=None):
    """ids int32 [4 * beams, t + 3]: row r ends with (a slice of) the head of a sequence of its turn (of `force` on every row of
    the sentences of list 0), behind filler tokens that occur in no sequence head; the three columns past t continue the head, so
    a window read one token too far would hit"""
    g = _gen(seed)
    list0, list1 = lists
    targets = [list0[0], list0[1], list0[4], list0[3], list0[5]]
    ids = torch.empty(4 * beams, t + 3, dtype=torch.int32)
    for r in range(4 * beams):
        s = r // beams
        seq = list1[(r * 131) % len(list1)] if s == 3 and (r + t) % 2 == 0 else targets[(r + t) % len(targets)]
        if force is not None and s in (0, 2):
            seq = force
        filler = torch.randint(100, 250, (t + 3,), generator=g).tolist()
        hist = (filler + list(seq[:-1]))[-t:] if t >= 1 else []
        ids[r, :t] = torch.tensor(hist, dtype=torch.int32)
        ids[r, t:] = torch.tensor((list(seq) + filler)[len(seq) - 1:len(seq) + 2] if t >= len(seq) - 1 else filler[:3], dtype=torch.int32)
    return ids


def _expected(V, sets, set_of, lists, list_of, ids, t, beams):
    """-> (uint32 words [rows, W] the kernel must write, bool [rows, V] the sequence rule's own bans)"""
    W = sets.shape[1]
    rows = ids.shape[0]
    want = np.zeros((rows, W), dtype=np.uint32)
    hits = torch.zeros(rows, V, dtype=torch.bool)
    for r in range(rows):
        s = r // beams
        if set_of[s] >= 0:
            want[r] = sets[set_of[s]]
        if list_of[s] >= 0:
            banned = sequence_banned(ids[r, :t].tolist(), lists[list_of[s]])
            want[r] |= _pack(V, banned, W)
            hits[r, sorted(banned)] = True
    return want, hits


def _ban(sets, set_of, S, eos, row_words=None):
    from generativeimage2text_amd import engine as E
    words = torch.from_numpy(sets.view(np.int32).copy()).cuda()
    z = torch.zeros(S, dtype=torch.int32).cuda()
    return E.DebugBan(words, sets.shape[0], sets.shape[1], torch.tensor(set_of, dtype=torch.int32).cuda(), z, z.clone(), eos,
                      row_words=row_words)


@pytest.mark.parametrize("V", [1000, 30522])
@pytest.mark.parametrize("beams", [1, 4])
def test_ban_rows_against_cpu_mask(operands, beams, V):
    """row_words of ban_rows_kernel equal, word for word, static set | sequence hits of the CPU definition, at t = m - 2, m - 1, m
    for m = 2, 3, 16, at 40 and at a history of 1024 tokens; beams = 4: every row of a sentence with its own history.  V = 30522:
    W = 954 (W % 4 != 0), the last word with bits 30522 .. 30527 that belong to no token.  Every word of every row is written, the
    row behind the last is not."""
    from generativeimage2text_amd import engine as E
    lists, list_of, pool, sets, set_of, heads = _case(V, seed=V + beams)
    W = sets.shape[1]
    ban = _ban(sets, set_of, 4, V - 2)
    seen = set()
    edges = [(m + d, seq) for seq in (lists[0][0], lists[0][1], lists[0][4]) for m in [len(seq)] for d in (-2, -1, 0) if m + d >= 1]
    for t, force in [(t, None) for t in (1, 2, 3, 14, 15, 16, 40, 1024)] + edges:
        ids = _histories(V, t, beams, lists, heads, seed=t, force=force)
        want, hits = _expected(V, sets, set_of, lists, list_of, ids, t, beams)
        if force is not None:                                               # t = m - 2: no hit; m - 1 and m: the last token
            assert bool(hits[0, force[-1]]) == (t >= len(force) - 1) and bool(hits[2 * beams, force[-1]]) == (t >= len(force) - 1)
        out = torch.full((4 * beams + 1, W), SENTINEL, dtype=torch.int32).cuda()
        E.op_ban_rows(ban, pool, ids.cuda(), t, beams, V, out=out[:4 * beams], operands=operands)
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:-1], want), (t, np.argwhere(got[:-1] != want)[:8].tolist())
        assert (got[-1] == SENTINEL).all()
        # list -1: the static set alone; no static set: the hits alone
        assert np.array_equal(got[beams:2 * beams], np.repeat(sets[1][None], beams, 0))
        assert not hits[beams:2 * beams].any()
        for r in range(4 * beams):
            if hits[r].sum() >= 2:
                seen.add("two hits")
            seen |= {("bit", int(c) & 31) for c in hits[r].nonzero()[:, 0].tolist() if int(c) & 31 in (0, 31)}
            if hits[r, 32 * (W - 1):].any():
                seen.add("last word")
            if r // beams == 3 and hits[r].any():
                seen.add("cap list")
    assert {"two hits", ("bit", 0), ("bit", 31), "last word", "cap list"} <= seen, seen


def test_ban_rows_refusals(operands):
    """The pool is checked by the arming call's own check before anything is launched: the output keeps its sentinel"""
    from generativeimage2text_amd import engine as E
    V = 1000
    sets = np.stack([_pack(V, [1])])
    ban = _ban(sets, [0, -1], 2, V - 2)
    ids = torch.zeros(2, 8, dtype=torch.int32).cuda()
    out = torch.full((2, sets.shape[1]), SENTINEL, dtype=torch.int32).cuda()
    good = [1, 2, 4, 0, 0, -1, 0, 2, 0, 2, 4, 5, 6, 7, 8]
    E.op_ban_rows(ban, good, ids, 4, 1, V, operands=operands)

    def bad(i, v, match):
        p = list(good)
        p[i] = v
        with pytest.raises(E.GitmiError, match=match):
            E.op_ban_rows(ban, p, ids, 4, 1, V, out=out, operands=operands)
    bad(0, 3, "sequence lists outside")
    bad(1, 5000, "sequences above the cap")
    bad(2, 5, "needs")
    bad(3, 1, "needs")
    bad(4, 1, "sentence 0: sequence list 1 outside")
    bad(5, -2, "sentence 1: sequence list -2 outside")
    bad(6, 1, "list offsets")
    bad(9, 1, "list 0: sequence 0 has 1 tokens")
    bad(9, 3, "list 0: sequence 0 has 3 tokens|sequence 1 has 1 tokens")
    bad(10, 3, "sequence offsets")
    bad(12, V, "list 0: sequence 0 holds token 1000 outside")
    bad(14, -1, "list 0: sequence 1 holds token -1 outside")
    with pytest.raises(E.GitmiError, match="has 17 tokens, outside"):
        E.op_ban_rows(ban, [1, 1, 17, 0, 0, 0, 0, 1, 0, 17] + [3] * 17, ids, 4, 1, V, out=out, operands=operands)
    with pytest.raises(E.GitmiError, match="cur_len=9 outside"):
        E.op_ban_rows(ban, good, ids, 9, 1, V, out=out, operands=operands)
    assert (out.cpu() == SENTINEL).all()


# ---- the consumers with row_words --------------------------------------------------------------------------------------------------
def _row_words_case(V, R, beams, t, seed):
    """Random per-row sets (~2 % of the tokens, the row's best two logits among them for every second row), histories, and a
    table whose static sets would ban something else: with row_words the static sets must not be read"""
    W = (V + 31) // 32
    g = np.random.RandomState(seed)
    ids = torch.randint(0, V, (R, t + 3), generator=_gen(seed), dtype=torch.int32)
    plen = torch.ones(R // beams, dtype=torch.int32)
    static = np.stack([_pack(V, range(0, V, 3), W)])
    set_of = [0 if s % 2 else -1 for s in range(R // beams)]
    return W, g, ids, plen, static, set_of


def _mask_of(words, V):
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").reshape(words.shape[0], -1)
    return torch.from_numpy(bits[:, :V].astype(bool))


def _random_row_words(g, logits, V, W):
    R = logits.shape[0]
    rw = np.zeros((R, W), dtype=np.uint32)
    for r in range(R):
        toks = g.randint(0, V, size=max(V // 50, 4)).tolist() + [0, V - 1]
        if r % 2 == 0:
            toks += logits[r].topk(2).indices.tolist()
        rw[r] = _pack(V, toks, W)
    rw[:, -1] |= _pack(32 * W, range(V, 32 * W), W)[-1]                      # bits past the vocabulary are ignored
    return rw


@pytest.mark.parametrize("V,R,beams,M", [(1000, 8, 4, 8), (30522, 6, 2, 3)])
def test_row_topm_with_row_words(operands, V, R, beams, M):
    """row_topm<BAN> with row_words == the plain instantiation on logits banned on the CPU, bit for bit; row_words == NULL ==
    today's hook"""
    from generativeimage2text_amd import engine as E
    t = 6
    W, g, ids, plen, static, set_of = _row_words_case(V, R, beams, t, seed=V + R)
    x = _rule_logits(R, V, seed=R)
    rw = _random_row_words(g, x, V, W)
    mask = _mask_of(rw, V)
    assert mask[torch.arange(0, R, 2), x[::2].argmax(1)].all()
    ids_d, plen_d, xd = ids.cuda(), plen.cuda(), x.cuda()
    rw_d = torch.from_numpy(rw.view(np.int32).copy()).cuda()
    for rp in (1.0, 1.3):
        want = E.op_row_topm(torch.where(mask, torch.tensor(BANNED), x).cuda(), V, M, ids_d, t, plen_d, beams, 1, rp, operands=operands)
        got = E.op_row_topm(xd, V, M, ids_d, t, plen_d, beams, 1, rp, operands=operands, ban=_ban(static, set_of, R // beams, V - 2, rw_d))
        for a, b in zip(got, want):
            assert torch.equal(a, b), rp
        old = E.op_row_topm(xd, V, M, ids_d, t, plen_d, beams, 1, rp, operands=operands, ban=_ban(static, set_of, R // beams, V - 2))
        smask = torch.stack([_mask_of(static, V)[0] if set_of[r // beams] >= 0 else torch.zeros(V, dtype=torch.bool) for r in range(R)])
        ref = E.op_row_topm(torch.where(smask, torch.tensor(BANNED), x).cuda(), V, M, ids_d, t, plen_d, beams, 1, rp, operands=operands)
        for a, b in zip(old, ref):
            assert torch.equal(a, b), rp


@pytest.mark.parametrize("V,R,beams", [(1000, 8, 4), (30522, 4, 2)])
def test_sample_rows_with_row_words(operands, V, R, beams):
    """sample_rows<true> with row_words == the plain instantiation on logits banned on the CPU: filtered logits, draws, log-probs"""
    from generativeimage2text_amd import engine as E
    t = 5
    W, g, ids, plen, static, set_of = _row_words_case(V, R, beams, t, seed=V + R + 1)
    x = _rule_logits(R, V, seed=R + 3)
    rw = _random_row_words(g, x, V, W)
    mask = _mask_of(rw, V)
    ids_d, plen_d = ids.cuda(), plen.cuda()
    rw_d = torch.from_numpy(rw.view(np.int32).copy()).cuda()
    kw = dict(temperature=0.9, top_k=50, top_p=0.95, ndraw=2, seed=1234, step=t, ids=ids_d, cur_len=t, rep_penalty=1.2, operands=operands)
    want = E.op_sample_rows_rules(torch.where(mask, torch.tensor(BANNED), x).cuda(), V, **kw)
    got = E.op_sample_rows_rules(x.cuda(), V, plen=plen_d, beams=beams, ban=_ban(static, set_of, R // beams, V - 2, rw_d), **kw)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # row_words == NULL: the static sets, as before
    smask = torch.stack([_mask_of(static, V)[0] if set_of[r // beams] >= 0 else torch.zeros(V, dtype=torch.bool) for r in range(R)])
    ref = E.op_sample_rows_rules(torch.where(smask, torch.tensor(BANNED), x).cuda(), V, **kw)
    old = E.op_sample_rows_rules(x.cuda(), V, plen=plen_d, beams=beams, ban=_ban(static, set_of, R // beams, V - 2), **kw)
    for a, b in zip(old, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("V,K,M,beams,mtop", [(1000, 128, 12, 4, 8), (937, 128, 130, 2, 4), (30522, 768, 12, 4, 4)])
def test_head_with_row_words(operands, V, K, M, beams, mtop):
    """The fused head's BAN instantiation with row_words: the stored logits are the plain launch's with -10000 exactly on the
    CPU mask of the rows' words; the lists and (max, sum exp) equal, bit for bit, those of the same launch given every row's words
    as a static set of its own (beams = 1 rows as sentences: the path the existing op tests hold to the reference), in the
    one-block-per-workgroup form, two walking forms and (M = 130) across row blocks.  row_words == NULL: today's launch."""
    from generativeimage2text_amd import engine as E
    dt = torch.bfloat16 if operands == "bf16" else torch.float16
    t = 7
    Wt, bias = _head_operands(V, K, seed=M + V)
    x = torch.randn(M, K, generator=_gen(M)) * 1.1 + 0.15
    approx = x.to(dt).double() @ Wt.to(dt).double().t() + bias.double()
    W, g, ids, plen, static, set_of = _row_words_case(V, M, beams, t, seed=V + M)
    rw = _random_row_words(g, approx.float(), V, W)
    mask = _mask_of(rw, V)
    Wf, bp = E.to_frag(Wt.to(dt).cuda(), 128), E._pad_vec(bias.cuda(), (V + 127) // 128 * 128)
    Af = E.to_frag(x.to(dt).cuda(), 64)
    ids_d, plen_d = ids.cuda(), plen.cuda()
    rw_d = torch.from_numpy(rw.view(np.int32).copy()).cuda()
    plen_rows = torch.ones(M, dtype=torch.int32).cuda()

    def head(**kw):
        return E.op_vocab_topm_rules(Af, Wf, bp, mtop, ids_d, t, kw.pop("plen", plen_d), kw.pop("beams", beams), 1, 1.3, packed=True,
                                     rows=M, V=V, **kw)
    ban_rows = _ban(static, set_of, M // beams, V - 2, rw_d)
    as_sets = E.DebugBan(rw_d, M, W, torch.arange(M, dtype=torch.int32).cuda(), torch.zeros(M, dtype=torch.int32).cuda(),
                         torch.zeros(M, dtype=torch.int32).cuda(), V - 2)
    pv0, pi0, pl0, lg0 = head(want_logits=True)
    pv, pi, pl, lg = head(want_logits=True, ban=ban_rows)
    assert torch.equal(lg.cpu(), torch.where(mask, torch.tensor(BANNED), lg0.cpu()))
    assert mask[torch.arange(M), lg0.cpu().argmax(1)].any()
    sv, si, sl, slg = head(want_logits=True, ban=as_sets, plen=plen_rows, beams=1)
    assert torch.equal(pv, sv) and torch.equal(pi, si) and torch.equal(pl, sl) and torch.equal(lg, slg)
    for max_wgs in (3, 60):
        qv, qi, ql, _ = head(want_logits=False, max_wgs=max_wgs, ban=ban_rows)
        assert torch.equal(qv, pv) and torch.equal(qi, pi) and torch.equal(ql, pl), max_wgs
    # row_words == NULL: the static sets, as before
    ov, oi, ol, olg = head(want_logits=True, ban=_ban(static, set_of, M // beams, V - 2))
    smask = torch.stack([_mask_of(static, V)[0] if set_of[r // beams] >= 0 else torch.zeros(V, dtype=torch.bool) for r in range(M)])
    assert torch.equal(olg.cpu(), torch.where(smask, torch.tensor(BANNED), lg0.cpu()))
