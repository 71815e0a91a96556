"""Inputs, fp64 references, fp32 emulations and tolerances of the op tests of the text pass around its attention and head
(csrc/kernels_score.hip), shared by tests/test_gpu_text_pass_ops.py (the kernels, on the GPU) and tests/test_text_pass_host.py
(CPU: that these inputs tell a wrong kernel from a right one).  Everything here is plain torch on the CPU."""
import torch

from test_gpu_tree_score_ops import _trees

U23 = 2.0 ** -23
SENT_F = -777.25          # the value the tests pre-fill the (lp, mean_lp) table with; no log-probability of these inputs is near it

# ---- embedding ---------------------------------------------------------------------------------------------------------
EMB_Q, EMB_LD, EMB_LP, EMB_MAXPOS, EMB_VOCAB = 3, 21, 32, 24, 50
EMB_EPS = 1e-8


def embed_inputs(D, offset=0.0):
    """One call: positions j >= ld embed id 0, positions j >= max_pos use the table's last row, ids -5, vocab and 2^33 + 1
    clamp.  Table rows are independent normal draws (an O(1) error for a wrong row).  positions_full has Lp rows: the engine's
    table is its first max_pos; the rest stands for the memory an unclamped position would read."""
    g = torch.Generator().manual_seed(1000 + D + int(offset))
    words = torch.randn(EMB_VOCAB, D, generator=g) + offset
    positions_full = torch.randn(EMB_LP, D, generator=g) * 0.7
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.3 * torch.randn(D, generator=g)
    tokens = torch.randint(0, EMB_VOCAB, (EMB_Q, EMB_LD), generator=g, dtype=torch.int64)
    tokens[0, 0], tokens[0, 1], tokens[0, 2] = -5, EMB_VOCAB, 2 ** 33 + 1
    tokens[2, EMB_LD - 1] = EMB_VOCAB - 1
    return dict(D=D, words=words, positions=positions_full[:EMB_MAXPOS].contiguous(), positions_full=positions_full, gamma=gamma,
                beta=beta, tokens=tokens)


def embed_rows(inp, clamp_pos=True):
    """(token id, position row) of every row (q, j), j < Lp, by the kernel's rule"""
    tok = torch.zeros(EMB_Q, EMB_LP, dtype=torch.int64)
    tok[:, :EMB_LD] = inp["tokens"].clamp(0, EMB_VOCAB - 1)
    pos = torch.arange(EMB_LP).expand(EMB_Q, EMB_LP)
    if clamp_pos:
        pos = pos.clamp(max=EMB_MAXPOS - 1)
    return tok.reshape(-1), pos.reshape(-1)


def embed_sum64(inp, tok, pos):
    return inp["words"].double()[tok] + inp["positions_full"].double()[pos]


def embed_emulate32(inp, tok, pos, first_wave_mean=False):
    """The kernel's arithmetic in fp32 (torch's summation order, not the kernel's).  first_wave_mean: the defect of a mean that
    sums the first wave's 256 columns only."""
    a = inp["words"][tok] + inp["positions_full"][pos]
    D = a.shape[1]
    mean = (a[:, :256] if first_wave_mean else a).sum(-1, keepdim=True) / D
    d = a - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / D + torch.tensor(EMB_EPS, dtype=torch.float32))
    return d * rstd * inp["gamma"] + inp["beta"]


def tree_embed_tables(seed=5):
    """node tables of the TREE instantiation: any token, any depth below max_pos, per row"""
    g = torch.Generator().manual_seed(seed)
    M = EMB_Q * EMB_LP
    return (torch.randint(0, EMB_VOCAB, (M,), generator=g, dtype=torch.int32),
            torch.randint(0, EMB_MAXPOS, (M,), generator=g, dtype=torch.int32))


# ---- trees -------------------------------------------------------------------------------------------------------------
TREE_LP, TREE_LD, TREE_V, TREE_MAX_DEPTH = 144, 136, 1001, 40


def tree_inputs(ld=TREE_LD, V=TREE_V):
    """The three trees of the tree attention's op test (a 16-chain, 70 leaves under a root, 130 nodes of random shape) with
    random tokens -> (packed int64 [3, ld], lens)"""
    trees = _trees()
    g = torch.Generator().manual_seed(11)
    packed = torch.zeros(len(trees), ld, dtype=torch.int64)
    for q, t in enumerate(trees):
        tok = torch.randint(0, V, (len(t),), generator=g, dtype=torch.int64)
        packed[q, :len(t)] = (torch.tensor(t, dtype=torch.int64) << 32) | tok
    return packed, [len(t) for t in trees]


def set_depth(packed, q, i, depth):
    out = packed.clone()
    out[q, i] = (depth << 32) | (int(out[q, i]) & 0xffffffff)
    return out


# one of each local rule of tree_structure_kernel, on tree 0 (the chain 0 .. 15): (name, node, depth, max_depth)
TREE_REJECTIONS = [("root_depth", 0, 1, TREE_MAX_DEPTH), ("jump_of_2", 9, 11, TREE_MAX_DEPTH),
                   ("depth_at_max", None, None, 15),          # node 15 has depth 15 == max_depth; the other trees stay below 7
                   ("second_root", 5, 0, TREE_MAX_DEPTH)]


def tree_tables_ref(packed, lens, Lp, V, max_depth):
    """Host walk -> (tables int32 [4, Q * Lp] = tok, depth, parent, end; bad [Q]).  The parent of node i is the last k < i with
    depth[k] == depth[i] - 1; end[k] the first index past k's subtree.  Rows past a tree's nodes and every row of a rejected
    tree: depth 0, no parent, end = i + 1.  Token ids: the low 32 bits as a signed int, clamped into [0, V)."""
    Q, ld = packed.shape
    tab = torch.zeros(4, Q, Lp, dtype=torch.int32)
    bad = torch.zeros(Q, dtype=torch.int32)
    for q in range(Q):
        n = max(0, min(int(lens[q]), ld, Lp))
        row = [int(v) for v in packed[q, :n]]
        dep = [v >> 32 for v in row]
        ok = all(d < max_depth and d <= (dep[i - 1] + 1 if i else 0) and d >= (1 if i else 0) for i, d in enumerate(dep))
        bad[q] = 0 if ok else 1
        for i in range(Lp):
            t = (row[i] & 0xffffffff) if i < n else 0
            t = t - (1 << 32) if t >= (1 << 31) else t
            tab[0, q, i] = min(max(t, 0), V - 1)
            tab[1, q, i] = dep[i] if ok and i < n else 0
            tab[2, q, i] = -1
            tab[3, q, i] = i + 1
        if not ok:
            continue
        path = {}
        for i, d in enumerate(dep):
            for k in [k for k in path if k >= d]:
                tab[3, q, path.pop(k)] = i
            tab[2, q, i] = path[d - 1] if d else -1
            path[d] = i
        for k in path:
            tab[3, q, path[k]] = n
    return tab.reshape(4, Q * Lp), bad


# ---- the tail: targets / structure, head, combine ------------------------------------------------------------------------
def head_tol(offset=0.0):
    """lp and mean_lp, fp32 and 16-bit operands alike (the operands are handed over rounded, both paths accumulate in fp32):
    test_score_head's fp32 bound -- 2e-4 + 16 fp32 ulps of the logits' magnitude"""
    return 2e-4 + 16 * max(1.0, offset) * U23


FLAT_F32 = dict(Q=5, ld=37, Lp=48, lens=[1, 2, 37, 20, 33], V=1001, K=128)       # ldl 1008, a partial last 256-stride
FLAT_16_BIG = dict(Q=3, ld=16, Lp=16, lens=[16, 2, 9], V=30522, K=768)


def flat_inputs(shape, dtype, offset=0.0):
    Q, ld, Lp, V, K = (shape[k] for k in ("Q", "ld", "Lp", "V", "K"))
    g = torch.Generator().manual_seed(V + K + int(offset))
    A = torch.randn(Q * Lp, K, generator=g).to(dtype)
    W = (torch.randn(V, K, generator=g) * 0.05).to(dtype)
    bias = torch.randn(V, generator=g) * 0.5 + offset
    tokens = torch.randint(0, V, (Q, ld), generator=g, dtype=torch.int64)
    q = 2                                                  # a sentence of full length: ids that clamp, the first and the last column
    tokens[q, 1], tokens[q, 2], tokens[q, 3], tokens[q, 4], tokens[q, 5] = -3, V + 5, 2 ** 33 + 1, 0, V - 1
    tokens[q, 6] = (V // 128) * 128                        # first column of the partial last 128-column tile
    return dict(A=A, W=W, bias=bias, tokens=tokens, lens=list(shape["lens"]), **{k: shape[k] for k in ("Q", "ld", "Lp", "V", "K")})


def flat_targets(inp):
    """tgt [Q * Lp]: row (q, j) predicts tokens[q][j + 1] (clamped into [0, V)) when j + 1 < len_q, else -1"""
    Q, ld, Lp, V = inp["Q"], inp["ld"], inp["Lp"], inp["V"]
    tgt = torch.full((Q, Lp), -1, dtype=torch.int32)
    for q in range(Q):
        for j in range(Lp):
            if j + 1 < inp["lens"][q]:
                tgt[q, j] = min(max(int(inp["tokens"][q, j + 1]), 0), V - 1)
    return tgt.reshape(-1)


def logits64(inp):
    return inp["A"].double() @ inp["W"].double().T + inp["bias"].double()


def flat_expected(inp, z=None):
    """fp64 -> ([Q, ld, 2] with SENT_F where nothing is written, bool [Q, ld] written)"""
    Q, ld, Lp = inp["Q"], inp["ld"], inp["Lp"]
    ls = torch.log_softmax(logits64(inp) if z is None else z, -1)
    out = torch.full((Q, ld, 2), SENT_F, dtype=torch.float64)
    written = torch.zeros(Q, ld, dtype=torch.bool)
    for row, t in enumerate(flat_targets(inp).tolist()):
        if t >= 0:
            q, j = divmod(row, Lp)
            out[q, j + 1, 0], out[q, j + 1, 1] = ls[row, t], ls[row].mean()
            written[q, j + 1] = True
    return out, written


def tiles32(z32, tile_w):
    """the head's per-tile statistics in fp32: [(max, sum exp(z - max), sum (z - max), columns)] per tile, each [rows]"""
    out = []
    for c0 in range(0, z32.shape[1], tile_w):
        t = z32[:, c0:c0 + tile_w]
        mx = t.max(-1).values
        out.append((mx, torch.exp(t - mx[:, None]).sum(-1), (t - mx[:, None]).sum(-1), t.shape[1]))
    return out


def combine32(tiles, zt32, V, full_last_tile=False, tile_w=128):
    """combine_row in fp32 -> (lp, mean_lp) per row.  full_last_tile: the defect of counting the partial last tile as tile_w
    columns."""
    M = torch.stack([t[0] for t in tiles]).max(0).values
    se = torch.zeros_like(M)
    sd = torch.zeros_like(M)
    for mx, e, sz, n in tiles:
        n = tile_w if full_last_tile else n
        se = se + e * torch.exp(mx - M)
        sd = sd + sz + torch.tensor(float(n)) * (mx - M)
    ls = torch.log(se)
    return (zt32 - M) - ls, sd / torch.tensor(float(V)) - ls


def logits32(inp):
    """the head's logits as an fp32 evaluation on the (already rounded) operands"""
    return inp["A"].float() @ inp["W"].float().T + inp["bias"]


def flat_emulate32(inp, f32_mode, **defect):
    """([Q, ld, 2] fp64 with SENT_F where nothing is written) of an fp32 rendering of the tail.  Defects (one at a time):
    full_last_tile; abs_row_chunk=c: the row statistics of chunks after the first read logits row row_off + r of a c-row
    buffer -- memory behind it, rendered as zeros; own_index: out[q * Lp + j] written in place of out[q * ld + j + 1] (writes
    past the table dropped)."""
    Q, ld, Lp, V = inp["Q"], inp["ld"], inp["Lp"], inp["V"]
    z = logits32(inp)
    if "abs_row_chunk" in defect:
        z = z.clone()
        z[defect["abs_row_chunk"]:] = 0.0
    tgt = flat_targets(inp)
    zt = z[torch.arange(z.shape[0]), tgt.clamp(min=0).long()]
    lp, mean = combine32(tiles32(z, V if f32_mode else 128), zt, V, defect.get("full_last_tile", False))
    out = torch.full((Q * ld, 2), SENT_F, dtype=torch.float64)
    for row, t in enumerate(tgt.tolist()):
        if t >= 0:
            q, j = divmod(row, Lp)
            i = q * Lp + j if defect.get("own_index") else q * ld + j + 1
            if i < Q * ld:
                out[i, 0], out[i, 1] = lp[row], mean[row]
    return out.reshape(Q, ld, 2)


def tree_tail_inputs(dtype, K, ld=TREE_LD, V=TREE_V):
    packed, lens = tree_inputs(ld, V)
    Q = packed.shape[0]
    g = torch.Generator().manual_seed(K)
    A = torch.randn(Q * TREE_LP, K, generator=g).to(dtype)
    W = (torch.randn(V, K, generator=g) * 0.05).to(dtype)
    bias = torch.randn(V, generator=g) * 0.5
    return dict(A=A, W=W, bias=bias, tokens=packed, lens=lens, Q=Q, ld=ld, Lp=TREE_LP, V=V, K=K)


def tree_rows(inp, max_depth=TREE_MAX_DEPTH):
    """(node row, row the logit is gathered from, token) of every node with a parent, + the verdicts"""
    tab, bad = tree_tables_ref(inp["tokens"], inp["lens"], inp["Lp"], inp["V"], max_depth)
    rows = (tab[2] >= 0).nonzero().flatten()
    prow = (rows // inp["Lp"]) * inp["Lp"] + tab[2][rows].long()
    return rows, prow, tab[0][rows].long(), bad


def tree_expected(inp, max_depth=TREE_MAX_DEPTH, own_row=False):
    """fp64 -> ([Q, ld, 2] with SENT_F where nothing is written, gathered logit z[parent row][token] per row (NaN: none)).
    own_row: the defect of gathering a child's logit at its own row."""
    Q, ld, Lp = inp["Q"], inp["ld"], inp["Lp"]
    z = logits64(inp)
    ls = torch.log_softmax(z, -1)
    rows, prow, tok, _ = tree_rows(inp, max_depth)
    src = rows if own_row else prow
    zt = torch.full((Q * Lp,), float("nan"), dtype=torch.float64)
    zt[rows] = z[src, tok]
    out = torch.full((Q, ld, 2), SENT_F, dtype=torch.float64)
    q, i = rows // Lp, rows % Lp
    out[q, i, 0] = zt[rows] - torch.logsumexp(z[prow], -1)
    out[q, i, 1] = ls[prow].mean(-1)
    return out, zt


def tree_emulate32(inp, f32_mode, max_depth=TREE_MAX_DEPTH, own_row=False):
    """([Q, ld, 2] fp64 with SENT_F where nothing is written) of an fp32 rendering of the tree tail: the head's tiles of the
    parent's row, the node's token gathered there.  own_row: the defect of gathering the logit at the child's own row."""
    Q, ld, Lp, V = inp["Q"], inp["ld"], inp["Lp"], inp["V"]
    z = logits32(inp)
    rows, prow, tok, _ = tree_rows(inp, max_depth)
    lp, mean = combine32(tiles32(z[prow], V if f32_mode else 128), z[rows if own_row else prow, tok], V)
    out = torch.full((Q, ld, 2), SENT_F, dtype=torch.float64)
    out[rows // Lp, rows % Lp, 0] = lp.double()
    out[rows // Lp, rows % Lp, 1] = mean.double()
    return out


def gather_dot_bound(inp, rows, prow, tok):
    """|zt - fp64 dot| of tree_gather_dot_kernel: a lane makes at most 16 fused adds, then 6 shuffle levels and the bias add, 23
    roundings in all: 32 u of sum |x_i w_i| (u = 2^-24: 2^-19), + a relative 2 u at |z| for the store"""
    sabs = (inp["A"].double()[prow].abs() * inp["W"].double()[tok].abs()).sum(-1)
    z = (inp["A"].double()[prow] * inp["W"].double()[tok]).sum(-1) + inp["bias"].double()[tok]
    return z, 2.0 ** -19 * sabs + U23 * z.abs()


def gather_dot32(inp, prow, tok, stop=None):
    """the dot in sequential fp32.  stop: the defect of a gather that ends at that column."""
    p = (inp["A"].float()[prow] * inp["W"].float()[tok])[:, :stop]
    return p.cumsum(-1)[:, -1] + inp["bias"][tok]
