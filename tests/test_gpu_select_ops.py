"""Op-level tests of the three kernels that choose the next token from a materialised logits row (kernels_search.hip), through
the hooks of the measurement build (include/gitmi_experiment.h): row_topm_kernel (every instantiation, both load paths, tie
order, the rules with full and colliding history sets), trie_select_kernel (one call with rows in every state, a node wider than
the workgroup, ties across waves) and sample_rows_kernel at the production and the largest vocabulary.  References are fp64 torch
on the CPU.  The kernels are fp32 and the same in both 16-bit operand builds; every case runs once in each measurement library."""
import collections
import functools
import math

import pytest
import torch

from oracle import git_oracle as O
from test_gpu_search_ops import _check_rule_lists, _histories, _ruled_fp64

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("experiment_build")]

PAD = 0x7fffffff
NEG = float("-inf")
HIST_CAP = 1024                                                          # HIST_SLOTS / 2 (gitmi_common.h)


@pytest.fixture(params=["bf16", "f16"])
def operands(request):
    """The measurement library the hooks are called in (libgitmi_exp.so / libgitmi_f16_exp.so)."""
    return request.param


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dev(x, ldl, off=0):
    """x [R, V] on the device as rows of stride ldl that start `off` floats into an allocation; the padding columns hold 1e30 (a
    kernel that read one would report it as the maximum)."""
    R, V = x.shape
    buf = torch.full((R * ldl + off,), 1e30)
    buf[off:].view(R, ldl)[:, :V] = x
    d = buf.cuda()[off:].view(R, ldl)
    assert d.data_ptr() % 16 == (4 * off) % 16
    return d


def _hash(tok):
    """hist_hash of gitmi_common.h: the slot a token's probing starts at."""
    return ((tok * 2654435761) & 0xffffffff) >> 21


# ---- A. row_topm ---------------------------------------------------------------------------------------------------------------
TOPM_M = [1, 2, 3, 4, 5, 8, 9, 16]
TOPM_SHAPES = [(30522, 30522, 0), (30522, 30524, 0), (30522, 30524, 1), (1003, 1004, 0), (1000, 1000, 0), (12, 12, 0)]


def _slots(M):
    return 1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8 if M <= 8 else 16


def _threads(M):
    return 1024 if M <= 4 else 512 if M <= 8 else 256                    # launch_row_topm's instantiations


def _owned(V, NT, vec, t):
    """The tokens thread t of an NT-thread workgroup feeds, in its order: every NT-th token on the scalar path; on the 16-byte path
    the 4-float chunks t, t + NT, ... and then every NT-th token of the tail past the last whole chunk."""
    if not vec:
        return list(range(t, V, NT))
    nchunk = V // 4
    return [4 * c + r for c in range(t, nchunk, NT) for r in range(4)] + list(range(4 * nchunk + t, V, NT))


@functools.lru_cache(maxsize=None)
def _topm_rows(V, M, vec):
    """Six rows [6, V]: 0 Gaussian; 1 multiples of 0.5 (ties everywhere); 2 the 16 largest on tokens of ONE thread (its list depth);
    3 winners at token 0, at V - 1 and in the scalar tail; 4 -inf on about a third, the first value of every thread and one whole
    16-byte chunk among them; 5 a single finite entry."""
    NT = _threads(M)
    g = _gen(1000 + V + M)
    x = torch.randn(6, V, generator=g) * 3.0
    x[1] = torch.round(x[1] * 2.0) / 2.0
    for j, t in enumerate(_owned(V, NT, vec, 1)[:16]):
        x[2, t] = 40.0 - 0.25 * ((j * 7) % 16)                           # distinct, not in the thread's feeding order
    tail = V // 4 * 4
    for j, t in enumerate((0, V - 1, tail if 0 < tail < V - 1 else V - 2)):
        x[3, t] = 30.0 - 0.5 * j
    mask = torch.rand(V, generator=g) < 0.25
    mask[:min(4 * NT, V // 2)] = True                                    # scalar path: tokens 0..NT-1; 16-byte path: chunks 0..NT-1
    q = (V // 2) // 4 * 4
    mask[q:q + 4] = True
    mask[V - 1] = False
    x[4, mask] = NEG
    x[5] = NEG
    x[5, V // 2] = 1.5
    return x


def _expected_lists(x, slots):
    """Stable descending sort: value descending, token ascending.  A list entry that holds no logit -- past V, or a -inf one -- is
    the format's unused entry (-inf, 0x7fffffff): -inf never enters a thread's list."""
    R, V = x.shape
    o = torch.sort(x, dim=1, descending=True, stable=True)
    k = min(slots, V)
    ev = torch.full((R, slots), NEG)
    ei = torch.full((R, slots), PAD, dtype=torch.int64)
    ev[:, :k] = o.values[:, :k]
    ei[:, :k] = o.indices[:, :k]
    ei[ev == NEG] = PAD
    return ev, ei


def _check_lse(x, pl):
    """part_lse = (max, sum exp(x - max)): the max exact, the sum within _check_rule_lists' rtol, the log-sum-exp within its 1e-4."""
    x64, pl = x.double(), pl.cpu().double()
    m = x64.max(1).values
    assert torch.isfinite(pl).all(), pl
    assert torch.equal(pl[:, 0], m)
    assert torch.allclose(pl[:, 1], torch.exp(x64 - m[:, None]).sum(1), rtol=2e-5, atol=0)
    err = (pl[:, 0] + torch.log(pl[:, 1]) - torch.logsumexp(x64, 1)).abs().max().item()
    assert err < 1e-4, err
    return err


@pytest.mark.parametrize("V,ldl,off", TOPM_SHAPES)
@pytest.mark.parametrize("M", TOPM_M)
def test_row_topm_lists_and_lse(operands, M, V, ldl, off):
    """Every instantiation ((MMAX, NT) = (1, 1024), (2, 1024), (4, 1024), (8, 512), (16, 256)) on the scalar path, the 16-byte main
    loop + tail, a misaligned base (falls back), the 16-byte remainder loop alone and a list longer than the row: the whole
    `slots`-entry list equals the stable descending sort, bit for bit, and (max, sum exp) gives the fp64 log-sum-exp -- finite
    also where -inf is the first value a thread sees."""
    from generativeimage2text_amd import engine as E
    vec = ldl % 4 == 0 and off % 4 == 0
    x = _topm_rows(V, M, vec)
    slots = _slots(M)
    pv, pi, pl = E.op_row_topm(_dev(x, ldl, off), V, M, operands=operands)
    assert pv.shape == (6, slots)
    ev, ei = _expected_lists(x, slots)
    assert torch.equal(pv.cpu(), ev), (pv.cpu(), ev)
    assert torch.equal(pi.cpu().long(), ei), (pi.cpu(), ei)
    err = _check_lse(x, pl)
    print(f"row_topm M {M} V {V} ldl {ldl} off {off} ({'16-byte' if vec else 'scalar'} path): log-sum-exp error {err:.2e} (bound 1e-4)")
    none = torch.zeros(4, V, dtype=torch.bool)
    _check_rule_lists(x[:4].double(), pv[:4, None], pi[:4, None], pl[:4, None], slots, none, cols=V)


def _rule_logits(R, V, seed):
    """Gaussian rows (scale 3) with block [256, 384) pushed down, as the head tests have it; every second row entirely negative,
    so that its list holds negative logits a penalty multiplies."""
    x = torch.randn(R, V, generator=_gen(seed)) * 3.0
    x[:, 256:384] -= 12.0
    x[1::2] -= 25.0
    return x


@pytest.mark.parametrize("V,ldl", [(30522, 30524), (1000, 1000)])
@pytest.mark.parametrize("beams,M", [(1, 1), (1, 3), (4, 8), (4, 16)])
def test_row_topm_rules_against_fp64(operands, beams, M, V, ldl):
    """The no-repeat rule and the repetition penalty inside row_topm_kernel against the reference's rules in fp64: penalties
    1.0 / 1.3 / 0.8 with and without suppression, sentences at or before their first step (not suppressed), histories with
    duplicates, token 0, token V - 1, the arg-max and the arg-min."""
    from generativeimage2text_amd import engine as E
    R, slots = 8, _slots(M)
    x = _rule_logits(R, V, 300 + V + M)
    d = _dev(x, ldl)
    for cur_len in (1, 9):
        plen = torch.tensor([(1, cur_len, cur_len + 2, max(cur_len - 1, 1))[s % 4] for s in range(R // beams)], dtype=torch.int32)
        assert (plen >= cur_len).any() and ((plen < cur_len).any() or cur_len == 1)
        ids = _histories(x.double(), cur_len, V, 17 + cur_len)
        for rp in (1.0, 1.3, 0.8):
            for suppress_kind in (1, 0):
                pv, pi, pl = E.op_row_topm(d, V, M, ids.cuda(), cur_len, plen.cuda(), beams, suppress_kind, rp, operands=operands)
                sl, penalised = _ruled_fp64(x, ids, cur_len, plen, beams, suppress_kind, rp)
                assert penalised.any() == (rp != 1.0)
                _check_rule_lists(sl, pv[:, None], pi[:, None], pl[:, None], slots, penalised, cols=V)


def _probe_lengths(hist):
    """The LDS set of hist_insert mirrored on the CPU -> (table, slots probed to find each member).  Which slots end up occupied does
    not depend on the insertion order."""
    tbl = [-1] * (2 * HIST_CAP)
    for t in hist:
        h = _hash(t)
        while tbl[h] not in (-1, t):
            h = (h + 1) % len(tbl)
        tbl[h] = t
    probes = {}
    for t in hist:
        h, n = _hash(t), 1
        while tbl[h] != t:
            h, n = (h + 1) % len(tbl), n + 1
        probes[t] = n
    return tbl, probes


@functools.lru_cache(maxsize=None)
def _colliding_history(V):
    """-> (1024 distinct tokens, outsiders): the set at its capacity with
      * up to 40 tokens of ONE hash value (all but two of the fullest bucket: a vocabulary below 40 * 2048 has no 40) and the
        buckets after it filled until one run of occupied slots is more than 40 long, so that look-ups walk 40 and more slots;
      * every token but one of hash 2047 and of hash 0: probing wraps from the last slot to slot 0 and is pushed on from there.
    outsiders: tokens NOT in the set whose probing starts inside those runs (a wrong hit would penalise them)."""
    buckets = collections.defaultdict(list)
    for t in range(V):
        buckets[_hash(t)].append(t)
    h0 = max(range(64, 1900), key=lambda h: len(buckets[h]))
    common = buckets[h0][:max(min(40, len(buckets[h0]) - 2), 1)]
    hist, outsiders = list(common), buckets[h0][len(common):][:2]
    h = h0
    while len(hist) < 48:
        h += 1
        hist += buckets[h][:-1]
        outsiders += buckets[h][-1:]
    for hb in (2047, 0):
        assert len(buckets[hb]) >= 3
        hist += buckets[hb][:-1]
        outsiders += buckets[hb][-1:]
    taken = set(hist) | set(outsiders)
    rest = [t for t in torch.randperm(V, generator=_gen(5)).tolist() if t not in taken]
    hist += rest[:HIST_CAP - len(hist)]
    assert len(hist) == len(set(hist)) == HIST_CAP and not set(hist) & set(outsiders)
    # the chosen tokens really collide
    assert len({_hash(t) for t in common}) == 1 and (len(common) == 40 or V < 40 * 2048)
    tbl, probes = _probe_lengths(hist)
    assert max(probes.values()) >= 40, max(probes.values())
    wrapped = [t for t in hist if _hash(t) == 2047 and tbl.index(t) < 64]
    assert len(wrapped) >= 2 and tbl[0] != -1 and _hash(tbl[0]) == 2047, wrapped
    return tuple(hist), tuple(outsiders), tuple(common), tuple(wrapped)


def _capacity_case(V, R, seed):
    """Rows whose 16 largest logits sit on 8 members of the colliding history (from the common-hash group, the wrapped group and
    elsewhere) and on 8 tokens outside it (the outsiders first), so that the top-16 list shows every wrong hit or miss; ids row r =
    the history rotated by 257 r (another insertion order), three columns past cur_len hold an outsider."""
    hist, outsiders, common, wrapped = _colliding_history(V)
    g = _gen(seed)
    x = torch.randn(R, V, generator=g) * 3.0
    members = list(common[:3]) + list(common[-1:]) + list(wrapped[:2]) + [hist[-1], hist[-2]]
    taken = set(hist) | set(outsiders)
    others = list(outsiders) + [t for t in range(V) if t not in taken][:8]
    planted = list(dict.fromkeys(members))[:8] + others[:8]
    assert len(set(planted)) == 16
    for r in range(R):
        for j, t in enumerate(planted):
            x[r, t] = 20.0 + 0.37 * ((j * 5 + r) % 16)
    x[1::2] -= 60.0                                                       # odd rows: every logit negative, the planted ones still on top
    ids = torch.empty(R, HIST_CAP + 3, dtype=torch.int32)
    for r in range(R):
        k = (257 * r) % HIST_CAP
        ids[r, :HIST_CAP] = torch.tensor(hist[k:] + hist[:k], dtype=torch.int32)
        ids[r, HIST_CAP:] = outsiders[0]
    return x, ids


@pytest.mark.parametrize("V,ldl", [(30522, 30524), (131072, 131072)])
def test_row_topm_history_at_capacity_with_colliding_hashes(operands, V, ldl):
    """The LDS history set at its capacity of 1024 distinct tokens, with probe runs of 40 and more slots and a run that wraps from
    slot 2047 to slot 0: members are penalised once, tokens outside the set that hash into the same runs are not.  V = 131072 is
    the smallest power of two at which 40 tokens share ONE hash value (row_topm has no vocabulary limit); at V = 30522 a bucket
    holds 17 at most, and the run is made of that bucket and its neighbours."""
    from generativeimage2text_amd import engine as E
    R, M = 4, 16
    x, ids = _capacity_case(V, R, 41)
    plen = torch.ones(R, dtype=torch.int32)
    d = _dev(x, ldl)
    for rp in (1.3, 0.8):
        pv, pi, pl = E.op_row_topm(d, V, M, ids.cuda(), HIST_CAP, plen.cuda(), 1, 1, rp, operands=operands)
        sl, penalised = _ruled_fp64(x, ids, HIST_CAP, plen, 1, 1, rp)
        assert penalised.sum().item() == R * (HIST_CAP - 1)                # every member but the suppressed last token
        _check_rule_lists(sl, pv[:, None], pi[:, None], pl[:, None], 16, penalised, cols=V)
        hit = torch.gather(penalised, 1, pi.cpu().long())
        assert hit.any(1).all() and (~hit).any(1).all()                   # the lists hold both kinds


def test_row_topm_refuses_a_history_past_capacity(operands):
    from generativeimage2text_amd import engine as E
    V, R = 1000, 2
    x = _rule_logits(R, V, 9)
    ids = torch.randint(0, V, (R, HIST_CAP + 4), generator=_gen(2), dtype=torch.int32).cuda()
    plen = torch.ones(R, dtype=torch.int32).cuda()
    out = (torch.full((R, 4), -7.0).cuda(), torch.full((R, 4), -7, dtype=torch.int32).cuda(), torch.full((R, 2), -7.0).cuda())
    with pytest.raises(E.GitmiError, match="invalid argument"):
        E.op_row_topm(_dev(x, V), V, 4, ids, HIST_CAP + 1, plen, 1, 1, 1.3, out=out, operands=operands)
    with pytest.raises(E.GitmiError, match="invalid argument"):
        E.op_row_topm(_dev(x, V), V, 17, out=out, operands=operands)
    with pytest.raises(E.GitmiError, match="cur_len"):
        E.op_row_topm(_dev(x, V), V, 4, ids, HIST_CAP + 5, plen, 1, 1, 1.0, out=out, operands=operands)
    torch.cuda.synchronize()
    assert all((o == -7).all().item() for o in out)
    E.op_row_topm(_dev(x, V), V, 4, ids, HIST_CAP + 1, plen, 1, 1, 1.0, out=out, operands=operands)   # no penalty: no set, no limit
    assert torch.equal(out[1][:, 0].cpu().long(), _ruled_fp64(x, ids.cpu(), HIST_CAP + 1, plen.cpu(), 1, 1, 1.0)[0].argmax(1))


# ---- B. trie_select ------------------------------------------------------------------------------------------------------------
TRIE_NT = 1024
ROW_A, ROW_B, ROW_C, ROW_D, ROW_E, ROW_F, ROW_G, ROW_H = range(8)
TRIE_EOS = 2
TRIE_FREE = (0, 1, 3, 4, 65, 66, 67, 69)         # never children of the wide node; 1 | 66 and 5 | 70 sit in different waves


def _wave(i):
    return (i % TRIE_NT) // 64


@functools.lru_cache(maxsize=None)
def _trie_case(V):
    """One call, eight rows (cur_len = 4).  Trie: node 0 with min(2500, V - 9) edges over the whole vocabulary, two of them with
    tokens -1 and V; node 1 with two children; node 2 with one child; node 3 a leaf."""
    g = _gen(70 + V)
    cur_len, ld_ids = 4, 6
    nw = min(2500, V - 9)
    perm = [t for t in torch.randperm(V, generator=g).tolist() if t != TRIE_EOS and t not in TRIE_FREE]
    tok0 = perm[:nw]
    bad = (3, nw - 3)
    tok0[bad[0]], tok0[bad[1]] = -1, V
    node0 = [3] * nw
    e_b, e_b2, e_g, e_g2, e_f = 10, 20, nw - 5, 7, 40
    # (h): two edges in different waves, the LOWER token on the later edge
    e_h1, e_h2 = next((a, b) for a in range(44, 64) for b in range(nw - 1, 63, -1)
                      if _wave(a) != _wave(b) and tok0[a] > tok0[b] >= 0 and b not in bad and b != e_g)
    node0[e_b], node0[e_g], node0[e_h1], node0[e_h2] = 1, 2, 1, 2
    only = tok0[50]                                                       # the one child of node 2
    child_off = [0, nw, nw + 2, nw + 3, nw + 3]
    child_tok = tok0 + [tok0[30], tok0[31], only]
    child_node = node0 + [3, 3, 3]
    x = torch.randn(8, V, generator=g) * 3.0
    top = x.max(1).values
    ids = torch.full((8, ld_ids), 69, dtype=torch.int32)
    ids[:, cur_len:] = tok0[e_b2]                                         # past cur_len: never read
    plen = torch.tensor([5, 4, 2, 2, 2, 2, 2, 2], dtype=torch.int32)
    cursor = torch.tensor([1, 0, 2, 1, -1, 3, 0, 0], dtype=torch.int32)

    def plant(r, t, dv):
        x[r, t] = top[r] + dv
    ids[ROW_B, 3] = tok0[e_b]                                             # first step: the last PREFIX token is the best child
    plant(ROW_B, tok0[e_b], 4.0), plant(ROW_B, tok0[e_b2], 3.0)
    ids[ROW_C, 3] = only                                                  # the cursor's only child was just emitted
    ids[ROW_D, 3] = TRIE_EOS
    ids[ROW_E, 3] = 0                                                     # off-trie: the row maximum is the suppressed last token
    plant(ROW_E, 0, 6.0), plant(ROW_E, 5, 3.0), plant(ROW_E, 70, 3.0)
    ids[ROW_F, 3] = 3
    plant(ROW_F, 3, 6.0), plant(ROW_F, tok0[e_f], 3.0), plant(ROW_F, V - 1, 4.0)
    ids[ROW_G, 3] = 4                                                     # best child near the end of the edge list
    plant(ROW_G, 65, 6.0), plant(ROW_G, tok0[e_g], 4.0), plant(ROW_G, tok0[e_g2], 3.0)
    ids[ROW_H, 3] = 67                                                    # bit-equal children, bit-equal row maxima
    plant(ROW_H, 1, 6.0), plant(ROW_H, 66, 6.0), plant(ROW_H, tok0[e_h1], 4.0), plant(ROW_H, tok0[e_h2], 4.0)
    assert _wave(1) != _wave(66) and _wave(5) != _wave(70) and x[ROW_H, 1] == x[ROW_H, 66] and x[ROW_E, 5] == x[ROW_E, 70]
    assert x[ROW_H, tok0[e_h1]] == x[ROW_H, tok0[e_h2]]
    if nw == 2500:
        assert e_g // TRIE_NT == 2 and bad[1] // TRIE_NT == 2 and e_h2 // TRIE_NT == 2   # the third trip of the edge loop
    csr = tuple(torch.tensor(a, dtype=torch.int32) for a in (child_off, child_tok, child_node))
    want_tok = {ROW_B: tok0[e_b], ROW_C: only, ROW_D: TRIE_EOS, ROW_E: 5, ROW_F: V - 1, ROW_G: tok0[e_g], ROW_H: tok0[e_h2]}
    want_cur = {ROW_A: 1, ROW_B: 1, ROW_C: 3, ROW_D: 1, ROW_E: -1, ROW_F: -1, ROW_G: 2, ROW_H: 2}
    return x, ids, cur_len, plen, cursor, csr, want_tok, want_cur


def _trie_reference(x_row, first, last, node, csr, dtype):
    """trie_decoder.py:57-71, 115-158 for one sentence (batch 1, as oracle.git_oracle.search_trie) in `dtype`:
    -> (value, token, next cursor, bonus, log-prob of the token before the bonus, all values).  Equal values: the lowest token."""
    child_off, child_tok, child_node = (a.tolist() for a in csr)
    V = x_row.numel()
    z = x_row.to(dtype).clone()
    if not first:
        z[last] = -10000.0
    lp = torch.log_softmax(z, 0)
    bonus = z.max() - z.min() + 1
    edges = {} if node < 0 else {child_tok[e]: e for e in range(child_off[node + 1] - 1, child_off[node] - 1, -1)
                                 if 0 <= child_tok[e] < V}
    out = lp.clone()
    if edges:
        out[torch.tensor(sorted(edges))] += bonus
    tok = int((out == out.max()).nonzero()[0, 0])
    return out[tok].item(), tok, (child_node[edges[tok]] if tok in edges else -1), bonus.item(), lp[tok].item(), out


def _ulp32(m):
    return 2.0 ** (math.floor(math.log2(m)) - 23)


@pytest.mark.parametrize("V", [80, 1000, 1025, 30522])
def test_trie_select_rows_in_every_state(operands, V):
    """(a) inside the prefix: nothing written; (b) first step: no suppression; (c) the only child is the suppressed last token:
    still chosen; (d) ended: (0, eos), cursor kept; (e) off-trie: plain arg-max without the last token; (f) on a leaf: plain
    arg-max, cursor -1; (g) best child at the end of a 2500-edge list; (h) bit-equal children in different waves: the lower
    token, and the cursor follows ITS edge.  V = 1025 walks the vocabulary in two strides, V = 30522 the edges in three trips."""
    from generativeimage2text_amd import engine as E
    x, ids, cur_len, plen, cursor, csr, want_tok, want_cur = _trie_case(V)
    out = (torch.full((8,), -7.0).cuda(), torch.full((8,), -7, dtype=torch.int32).cuda(), torch.full((8, 2), -7.0).cuda())
    cur = cursor.cuda()
    E.op_trie_select(_dev(x, V + 3), V, ids.cuda(), cur_len, plen.cuda(), TRIE_EOS, *(a.cuda() for a in csr), cur, out,
                     operands=operands)
    pv, pi, pl, cur = out[0].cpu().double(), out[1].cpu().long(), out[2].cpu(), cur.cpu().long()
    assert pv[ROW_A] == -7 and pi[ROW_A] == -7 and (pl[ROW_A] == -7).all()
    assert torch.equal(pl[1:], torch.tensor([[0.0, 1.0]]).expand(7, 2))
    assert pv[ROW_D] == 0.0
    worst = 0.0
    for r in range(1, 8):
        first, last = cur_len == int(plen[r]), int(ids[r, cur_len - 1])
        if r != ROW_D:
            val, tok, nxt, bonus, lp_tok, _ = _trie_reference(x[r], first, last, int(cursor[r]), csr, torch.float64)
            assert tok == want_tok[r] and nxt == want_cur[r], (r, tok, nxt)          # the case is what its comment says
            # value bound: 2e-5 for the log-sum-exp -- the bound tests/test_gpu_search_ops.py derives for a 64-lane tree of __expf
            # partial sums at |x| <= 16 -- plus 4 fp32 ulps at the largest magnitude among |bonus| and |lp|: the three roundings
            # of ((x - max) - logsum) + bonus and the one of bonus = (max - min) + 1.  About 3e-5 on first-step rows (bonus ~ 25),
            # about 4e-3 where -10000 enters the minimum (bonus ~ 1e4, one ulp = 2^-10).
            tol = 2e-5 + 4 * _ulp32(max(abs(bonus), abs(lp_tok)))
            err = abs(pv[r].item() - val)
            print(f"trie_select V {V} row {'abcdefgh'[r]}: value error {err:.2e} (bound {tol:.2e})")
            assert err <= tol, (r, err, tol)
            worst = max(worst, err / tol)
            if r in (ROW_E, ROW_H):
                # the lowest-token rule IS the reference's behaviour: torch.topk(1) on the fp32 row picks the same token
                out32 = _trie_reference(x[r], first, last, int(cursor[r]), csr, torch.float32)[5]
                assert (out32 == out32.max()).sum().item() == 2 and int(out32.topk(1).indices[0]) == tok, r
        assert pi[r] == want_tok[r], (r, int(pi[r]), want_tok[r])
        assert cur[r] == want_cur[r], (r, int(cur[r]), want_cur[r])
    assert cur[ROW_A] == want_cur[ROW_A]
    assert pv[ROW_C] <= 1.0 + 5e-3                                        # (c): lp(-10000) + bonus = (max - logsumexp) + 1
    print(f"trie_select V {V}: largest error / bound {worst:.2f}")


def test_trie_select_refusals(operands):
    from generativeimage2text_amd import engine as E
    V = 80
    x, ids, cur_len, plen, cursor, csr, _, _ = _trie_case(V)
    out = (torch.full((8,), -7.0).cuda(), torch.full((8,), -7, dtype=torch.int32).cuda(), torch.full((8, 2), -7.0).cuda())
    cur, d = cursor.cuda(), _dev(x, V + 3)
    off, tok, node = (a.cuda() for a in csr)

    def call(off=off, tok=tok, node=node, V=V, cur=cur, n_nodes=4):
        E.op_trie_select(d, V, ids.cuda(), cur_len, plen.cuda(), TRIE_EOS, off, tok, node, cur, out, n_nodes=n_nodes, operands=operands)
    for kw, what in (({"off": None}, "null trie"), ({"tok": None}, "null trie"), ({"node": None}, "null trie"), ({"V": 1}, "V=1"),
                     ({"off": (csr[0] + 1).cuda()}, "start at 0"),
                     ({"off": torch.tensor([0, 5, 3, 6, 6], dtype=torch.int32).cuda()}, "non-decreasing"),
                     ({"node": torch.full_like(csr[2], 4).cuda()}, "leads to node"),
                     ({"cur": torch.full((8,), 4, dtype=torch.int32).cuda()}, "cursor")):
        with pytest.raises(E.GitmiError, match=what):
            call(**kw)
    torch.cuda.synchronize()
    assert all((o == -7).all().item() for o in out) and torch.equal(cur.cpu(), cursor)


# ---- C. sample_rows ------------------------------------------------------------------------------------------------------------
SAMPLE_PARAMS = [(0, 0.9, 1.0), (50, 1.0, 1.0), (20, 0.7, 1.3), (5, 0.3, 0.7), (0, 0.05, 1.0), (3, 0.999, 1.0), (1, 0.5, 2.0), (0, 1.0, 1.0)]
SAMPLE_SHAPES = [(30522, 30522), (30522, 30528), (32768, 32768)]
SAMPLE_SEED = 3


@functools.lru_cache(maxsize=None)
def _sample_logits(V):
    return torch.randn(6, V, generator=_gen(SAMPLE_SEED + V)) * 3.0


def _check_kept(logits, temp, top_k, top_p, filt):
    """The kept set against oracle.sampling_distribution by the rule of test_sampling_filter_equals_reference_filter: a token may
    differ only if the mass before it is within 1e-5 of top_p, at most 2 per call.  Before that cap is relied on: the oracle alone,
    fp32 against fp64 cumulative sums, stays within it on these logits.  -> (kept mask, reference log-probs, differing tokens)."""
    want = O.sampling_distribution(logits, temp, top_k, top_p)
    want64 = O.sampling_distribution(logits.double(), temp, top_k, top_p)
    assert (torch.isfinite(want) != torch.isfinite(want64)).sum().item() <= 2
    kept_ref, kept = torch.isfinite(want), torch.isfinite(filt)
    diff = kept_ref != kept
    if diff.any():
        srt, idx = torch.sort(logits / temp, descending=True)
        cum = torch.cumsum(torch.softmax(srt.double(), -1), -1)
        before = torch.zeros_like(cum)
        before[:, 1:] = cum[:, :-1]
        pos = torch.argsort(idx, dim=1)
        assert (torch.gather(before, 1, pos)[diff] - top_p).abs().max().item() < 1e-5
        assert diff.sum().item() <= 2
    return kept, kept_ref, want, int(diff.sum())


def _check_draws(filt, kept, tok, lp, ndraw, stride):
    """Draws without replacement: the first min(ndraw, kept tokens) are distinct tokens of the kept set with their filtered
    log-prob within 1e-4; a draw past the kept set has log-prob -inf; entries ndraw..stride are (-inf, 0x7fffffff)."""
    got_lp = torch.log_softmax(filt.double(), -1)
    tok, lp = tok.cpu().long(), lp.cpu().double()
    assert tok.shape == lp.shape == (filt.shape[0], stride)
    worst = 0.0
    for r in range(filt.shape[0]):
        n = min(ndraw, int(kept[r].sum()))
        t = tok[r, :n]
        assert len(set(t.tolist())) == n and kept[r, t].all(), (r, t)
        worst = max(worst, (got_lp[r, t] - lp[r, :n]).abs().max().item())
        assert (lp[r, n:] == NEG).all(), (r, lp[r])
    assert (tok[:, ndraw:] == PAD).all()
    assert worst < 1e-4, worst
    return worst


@pytest.mark.parametrize("V,ldl", SAMPLE_SHAPES)
@pytest.mark.parametrize("top_k,top_p,temp", SAMPLE_PARAMS)
def test_sample_rows_at_full_vocabulary(operands, top_k, top_p, temp, V, ldl):
    """The production vocabulary (30 of the 32 per-thread registers), a padded row stride and the launcher's limit of 32768, with
    1, 3 and 16 draws into lists of 1 and 16 entries."""
    from generativeimage2text_amd import engine as E
    logits = _sample_logits(V)
    d = _dev(logits, ldl)
    for ndraw, stride in ((1, 1), (16, 16), (3, 16)):
        filt, tok, lp = E.op_sample_rows_rules(d, V, temp, top_k, top_p, ndraw, seed=5, step=1, stride=stride, operands=operands)
        filt = filt.cpu()
        kept, kept_ref, want, ndiff = _check_kept(logits, temp, top_k, top_p, filt)
        same = kept & kept_ref
        err = (torch.log_softmax(filt.double(), -1)[same] - want.double()[same]).abs().max().item()
        assert err < 1e-4, err
        assert torch.equal(filt[kept], (logits / temp)[kept]) or torch.allclose(filt[kept], (logits / temp)[kept], rtol=1e-6)
        derr = _check_draws(filt, kept, tok, lp, ndraw, stride)
        _, tok2, lp2 = E.op_sample_rows_rules(d, V, temp, top_k, top_p, ndraw, seed=5, step=1, stride=stride, want_filtered=False,
                                              operands=operands)
        assert torch.equal(tok, tok2) and torch.equal(lp, lp2)            # same (seed, step): same draws
        print(f"sample_rows V {V} ldl {ldl} k {top_k} p {top_p} T {temp} ndraw {ndraw}/{stride}: kept {kept.sum(1).tolist()}, "
              f"{ndiff} boundary tokens, filtered log-prob error {err:.2e}, draw log-prob error {derr:.2e} (bounds 1e-4)")


def _penalised_fp32(x, ids, cur_len, rp):
    """rep_penalize on the fp32 logits: one fp32 multiply (negative) or divide by the fp32 penalty per history token."""
    out = x.clone()
    rp32 = torch.tensor(rp, dtype=torch.float32)
    for r in range(x.shape[0]):
        t = torch.tensor(sorted(set(ids[r, :cur_len].tolist())))
        out[r, t] = torch.where(x[r, t] < 0, x[r, t] * rp32, x[r, t] / rp32)
    return out


@pytest.mark.parametrize("cur_len", [9, HIST_CAP])
@pytest.mark.parametrize("rp", [1.3, 0.8])
def test_sample_rows_with_repetition_penalty(operands, rp, cur_len):
    """The penalty path (raw logits, before the temperature) at V = 30522 with a padded stride: the filtered logits are the
    reference's filter applied to the penalised fp32 logits, kept values within 2 ulp; at cur_len = 1024 the history is the
    colliding set of the row_topm tests, with members and same-run outsiders among the largest logits."""
    from generativeimage2text_amd import engine as E
    V, ldl = 30522, 30528
    if cur_len == HIST_CAP:
        x, ids = _capacity_case(V, 4, 43)
    else:
        x = _rule_logits(6, V, 77)
        ids = _histories(x.double(), cur_len, V, 21)
    pen = _penalised_fp32(x, ids, cur_len, rp)
    assert (pen != x).any(1).all()
    d = _dev(x, ldl)
    for top_k, top_p, temp in ((20, 0.7, 1.3), (0, 0.9, 1.0), (50, 1.0, 1.0)):
        filt, tok, lp = E.op_sample_rows_rules(d, V, temp, top_k, top_p, 3, seed=11, step=2, stride=16, ids=ids.cuda(), cur_len=cur_len,
                                               rep_penalty=rp, operands=operands)
        filt = filt.cpu()
        kept, kept_ref, want, ndiff = _check_kept(pen, temp, top_k, top_p, filt)
        ref = (pen / temp).double()
        err = ((filt.double() - ref)[kept].abs() / ref[kept].abs()).max().item()
        assert err <= 2.0 ** -22, err
        if top_k == 50:
            assert (kept & (pen != x)).any()                              # penalised tokens are among the kept ones
        same = kept & kept_ref
        lerr = (torch.log_softmax(filt.double(), -1)[same] - want.double()[same]).abs().max().item()
        assert lerr < 1e-4, lerr
        derr = _check_draws(filt, kept, tok, lp, 3, 16)
        print(f"sample_rows penalty {rp} cur_len {cur_len} k {top_k} p {top_p} T {temp}: kept value error {err / 2.0 ** -23:.2f} ulp "
              f"(bound 2), {ndiff} boundary tokens, filtered log-prob error {lerr:.2e}, draw log-prob error {derr:.2e} (bounds 1e-4)")


def test_sample_rows_refusals(operands):
    from generativeimage2text_amd import engine as E
    R = 2
    big = torch.randn(R, 32769, generator=_gen(1)).cuda()
    ids = torch.randint(0, 1000, (R, HIST_CAP + 4), generator=_gen(2), dtype=torch.int32).cuda()
    out = (torch.full((R, 17), -7.0).cuda(), torch.full((R, 17), -7, dtype=torch.int32).cuda(), torch.full((R, 32769), -7.0).cuda())
    for kw in (dict(V=32769, ndraw=2, stride=2), dict(V=3000, ndraw=3, stride=2), dict(V=3000, ndraw=17, stride=17),
               dict(V=3000, ndraw=2, stride=2, ids=ids, cur_len=HIST_CAP + 1, rep_penalty=1.3)):
        with pytest.raises(E.GitmiError, match="invalid argument"):
            E.op_sample_rows_rules(big, top_k=50, top_p=0.9, out=out, operands=operands, **kw)
    torch.cuda.synchronize()
    assert all((o == -7).all().item() for o in out)
