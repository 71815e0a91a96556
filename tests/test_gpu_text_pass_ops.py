"""GPU: the kernels of the score / tree-score text pass around its attention (csrc/kernels_score.hip), op by op, through the
measurement build's hooks gitmi_debug_score_embed, gitmi_debug_tree_tables and gitmi_debug_score_tail (an argument check + the
launchers text_pass_impl calls; the head is launch_score_head_rows, the engine's own chunk loop): score_embed_ln_kernel (flat and
tree instantiation, fp32 and 16-bit copy), tree_structure_kernel's four tables, score_targets_kernel, score_rowstats_kernel in row
chunks, score_combine_kernel at Lp > 1 and ld != Lp, score_info_kernel, tree_gather_dot_kernel, tree_gather_logits_kernel and
tree_combine_kernel.  References are fp64 torch on the CPU from the same, already rounded, operands (text_pass_cases.py, which
tests/test_text_pass_host.py checks against renderings of the defects these inputs are chosen to catch).  Every output is
pre-filled with a sentinel and sits between sentinel margins that must come back untouched.

The head tolerance in force is T.head_tol: 2e-4 + 16 fp32 ulps of the logits' magnitude, for fp32 and 16-bit operands alike."""
import pytest
import torch

import text_pass_cases as T
from ln_reference import ln_ref_and_bound
from test_gpu_dgemm_forms import on_both_operand_builds
from test_gpu_frontend_ops import Guarded, _assert_within, _bits

pytestmark = pytest.mark.gpu

# Every test runs on the bf16 measurement build under its own name and, as <name>_f16, on the fp16 one (last line).
BUILD = {"ops": "bf16"}


def _op_dtype():
    return {"bf16": torch.bfloat16, "f16": torch.float16}[BUILD["ops"]]


def _E():
    from generativeimage2text_amd import engine
    return engine


def _dt(kind):
    return torch.float32 if kind == "f32" else _op_dtype()


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).cuda()


# ---- embedding -----------------------------------------------------------------------------------------------------------
def _run_embed(inp, dt, tokens, nodes=None):
    M, D = T.EMB_Q * T.EMB_LP, inp["D"]
    hf, ht = Guarded((M, D), torch.float32), Guarded((M, D), dt)
    ntk, ndp = (None, None) if nodes is None else (nodes[0].cuda(), nodes[1].cuda())
    _E().op_score_embed(tokens.cuda(), T.EMB_LP, inp["words"].cuda(), inp["positions"].cuda(), inp["gamma"].cuda(),
                        inp["beta"].cuda(), T.EMB_EPS, hf.t, ht.t, ntk, ndp, operands=BUILD["ops"])
    return hf.cpu("h_f"), ht.cpu("h_t")


def _check_embed(inp, dt, hf, ht, tok, pos, what):
    ref, bound = ln_ref_and_bound(T.embed_sum64(inp, tok, pos), inp["gamma"], inp["beta"], T.EMB_EPS)
    worst = float(((hf.double() - ref).abs() / bound).max())
    print(f"score embedding {what}: max error {float((hf.double() - ref).abs().max()):.3e}, {worst:.3f} of the element-wise bound "
          f"(largest bound {float(bound.max()):.3e})")
    _assert_within(hf, ref, bound, what)
    assert torch.equal(_bits(ht), _bits(hf.to(dt))), (what, "the operand copy is not the fp32 output rounded once")


@pytest.mark.parametrize("out", ["f32", "16"])
@pytest.mark.parametrize("D,offset", [(768, 0.0), (1024, 0.0), (128, 0.0), (100, 0.0), (768, 60.0)])
def test_score_embedding(experiment_build, D, offset, out):
    """D = 768: three active waves; 1024: every thread; 128: half a wave (the cross-wave sums add three zeros); 100: lanes masked
    by c < D.  Offset 60 on the word table: the mean carries it, the variance must not."""
    inp, dt = T.embed_inputs(D, offset), _dt(out)
    hf, ht = _run_embed(inp, dt, inp["tokens"])
    _check_embed(inp, dt, hf, ht, *T.embed_rows(inp), f"D={D} offset={offset} {out}")


@pytest.mark.parametrize("out", ["f32", "16"])
@pytest.mark.parametrize("D", [768, 100])
def test_score_embedding_of_tree_nodes(experiment_build, D, out):
    """TREE instantiation: token and position (= depth) come from the node tables; `tokens` holds ids the flat instantiation
    would clamp to the last word -- it is not read."""
    inp, dt = T.embed_inputs(D), _dt(out)
    ntk, ndp = T.tree_embed_tables()
    hf, ht = _run_embed(inp, dt, torch.full((T.EMB_Q, T.EMB_LD), 2 ** 40, dtype=torch.int64), (ntk, ndp))
    _check_embed(inp, dt, hf, ht, ntk.long(), ndp.long(), f"tree D={D} {out}")


# ---- tree tables -----------------------------------------------------------------------------------------------------------
def _run_tables(packed, lens, Lp=T.TREE_LP, V=T.TREE_V, max_depth=T.TREE_MAX_DEPTH):
    Q = packed.shape[0]
    tab, bad = Guarded((4, Q * Lp), torch.int32), Guarded((Q,), torch.int32)
    _E().op_tree_tables(packed.cuda(), _i32(lens), Lp, V, max_depth, tab.t, bad.t, operands=BUILD["ops"])
    return tab.cpu("tables"), bad.cpu("bad")


def _same_tables(got, ref, what):
    for name, g, r in zip(("tok", "depth", "parent", "end"), got, ref):
        assert torch.equal(g, r), (what, name, (g != r).nonzero().flatten().tolist()[:8])


def test_tree_tables_equal_the_host_walk(experiment_build):
    packed, lens = T.tree_inputs()
    got, bad = _run_tables(packed, lens)
    ref, ref_bad = T.tree_tables_ref(packed, lens, T.TREE_LP, T.TREE_V, T.TREE_MAX_DEPTH)
    assert bad.tolist() == ref_bad.tolist() == [0, 0, 0]
    _same_tables(got, ref, "trees")
    Lp = T.TREE_LP
    for q, n in enumerate(lens):                               # padding rows: parentless roots of their own
        pad = slice(q * Lp + n, (q + 1) * Lp)
        assert bool((got[2, pad] == -1).all()) and bool((got[1, pad] == 0).all())
        assert got[3, pad].tolist() == list(range(n + 1, Lp + 1))


def test_tree_tables_clamp_lengths_and_token_ids(experiment_build):
    """lens[2] = 140 > ld = 130 clamps to ld (the tree's 130 nodes); ids above V - 1 become V - 1, ids with bit 31 set 0"""
    ld, V = 130, T.TREE_V
    packed, lens = T.tree_inputs(ld=ld)
    packed[0, 3] = (3 << 32) | (V + 7)
    packed[0, 4] = (4 << 32) | 0x80000005
    packed[1, 69] = (1 << 32) | 0xffffffff
    lens = [lens[0], lens[1], 140]
    got, bad = _run_tables(packed, lens)
    ref, _ = T.tree_tables_ref(packed, lens, T.TREE_LP, V, T.TREE_MAX_DEPTH)
    assert bad.tolist() == [0, 0, 0]
    assert (int(ref[0, 3]), int(ref[0, 4]), int(ref[0, T.TREE_LP + 69])) == (V - 1, 0, 0)
    assert int(ref[3, 2 * T.TREE_LP]) == ld                    # the root of the clamped tree ends at ld
    _same_tables(got, ref, "clamps")


@pytest.mark.parametrize("name,node,depth,max_depth", T.TREE_REJECTIONS, ids=[r[0] for r in T.TREE_REJECTIONS])
def test_tree_tables_of_a_rejected_tree(experiment_build, name, node, depth, max_depth):
    """one tree breaks one rule: it is flagged and becomes parentless rows, the other trees' tables are what they were"""
    clean, lens = T.tree_inputs()
    packed = clean if node is None else T.set_depth(clean, 0, node, depth)
    got, bad = _run_tables(packed, lens, max_depth=max_depth)
    ref, _ = T.tree_tables_ref(packed, lens, T.TREE_LP, T.TREE_V, max_depth)
    clean_ref, _ = T.tree_tables_ref(clean, lens, T.TREE_LP, T.TREE_V, T.TREE_MAX_DEPTH)
    Lp = T.TREE_LP
    assert bad.tolist() == [1, 0, 0]
    assert bool((got[2, :Lp] == -1).all()) and bool((got[1, :Lp] == 0).all()) and got[3, :Lp].tolist() == list(range(1, Lp + 1))
    _same_tables(got, ref, name)
    _same_tables(got[:, Lp:], clean_ref[:, Lp:], name + ": the other trees")


# ---- the tail ----------------------------------------------------------------------------------------------------------------
def _run_tail(inp, chunk_rows=0, tree_max_depth=0):
    Q, ld, Lp = inp["Q"], inp["ld"], inp["Lp"]
    out, bad, info = Guarded((Q, ld, 2), torch.float32), Guarded((Q,), torch.int32), Guarded((4,), torch.int32)
    tgt, zt = Guarded((Q * Lp,), torch.int32), Guarded((Q * Lp,), torch.float32)
    out.t.fill_(T.SENT_F)
    _E().op_score_tail(inp["A"].cuda(), inp["W"].cuda(), inp["bias"].cuda(), inp["tokens"].cuda(), _i32(inp["lens"]), Lp, out.t, bad.t,
                       info.t, chunk_rows, tree_max_depth, tgt.t, zt.t, operands=BUILD["ops"])
    return out.cpu("out"), bad.cpu("bad").tolist(), info.cpu("info").tolist(), tgt.cpu("tgt"), zt.cpu("zt")


def _check_values(out, ref, tol, what):
    """placement: exactly the entries the reference fills were written; values: lp and mean_lp within tol"""
    written = ref[..., 0] != T.SENT_F
    assert torch.equal(out != T.SENT_F, written[..., None].expand_as(out)), (what, "entries written")
    err = (out.double() - ref).abs()[written]
    print(f"{what}: lp max error {float(err[:, 0].max()):.3e}, mean_lp max error {float(err[:, 1].max()):.3e}, bound {tol:.3e} "
          f"(2e-4 + 16 fp32 ulps of the logits' magnitude) over {int(written.sum())} positions")
    assert float(err[:, 0].max()) <= tol and float(err[:, 1].max()) <= tol, (what, err.max(0).values.tolist(), tol)


FLAT_CASES = [("f32", T.FLAT_F32, 0.0), ("f32", T.FLAT_F32, 1e3), ("16", T.FLAT_F32, 0.0), ("16", T.FLAT_16_BIG, 0.0),
              ("16", T.FLAT_16_BIG, 1e3)]


@pytest.mark.parametrize("kind,shape,offset", FLAT_CASES, ids=[f"{k}-V{s['V']}-K{s['K']}-off{int(o)}" for k, s, o in FLAT_CASES])
def test_flat_tail(experiment_build, kind, shape, offset):
    """targets, head, combine, info of a score call.  fp32: 240 rows in chunks of 64 (four chunks that cut through sentences)
    and in one chunk, bit for bit the same."""
    inp = T.flat_inputs(shape, _dt(kind), offset)
    what = f"flat tail {kind} V={shape['V']} K={shape['K']} offset={offset}"
    out, bad, info, tgt, _ = _run_tail(inp, chunk_rows=64 if kind == "f32" else 0)
    assert torch.equal(tgt, T.flat_targets(inp)), what
    assert bad == [0] * inp["Q"] and info == [inp["ld"], 0, 0, 0], (bad, info)
    assert bool((out[:, 0] == T.SENT_F).all()), (what, "position 0 has no prediction")
    _check_values(out, T.flat_expected(inp)[0], T.head_tol(offset), what)
    if kind == "f32":
        one = _run_tail(inp, chunk_rows=inp["Q"] * inp["Lp"])
        assert torch.equal(_bits(one[0]), _bits(out)) and torch.equal(one[3], tgt), (what, "one chunk against four")


@pytest.mark.parametrize("kind", ["f32", "16"])
def test_flat_tail_flags_a_non_finite_sentence(experiment_build, kind):
    """+inf in one text row of sentence 1: that sentence is flagged, the count says one, the others are bit for bit the clean run"""
    inp = T.flat_inputs(T.FLAT_F32, _dt(kind))
    chunk = 64 if kind == "f32" else 0
    clean = _run_tail(inp, chunk_rows=chunk)[0]
    inp["A"] = inp["A"].clone()
    inp["A"][1 * inp["Lp"] + 0, 5] = float("inf")
    out, bad, info, _, _ = _run_tail(inp, chunk_rows=chunk)
    assert bad == [0, 1, 0, 0, 0] and info == [inp["ld"], 0, 0, 1], (bad, info)
    assert not bool(torch.isfinite(out[1, 1]).all())
    keep = [0, 2, 3, 4]
    assert torch.equal(_bits(out[keep]), _bits(clean[keep]))
    assert bool((out[1, 2:] == T.SENT_F).all()) and bool((out[1, 0] == T.SENT_F).all())


TREE_CASES = [("16", 128), ("16", 544), ("16", 768), ("16", 1024), ("f32", 128)]


@pytest.mark.parametrize("kind,K", TREE_CASES, ids=[f"{k}-K{K}" for k, K in TREE_CASES])
def test_tree_tail(experiment_build, kind, K):
    """structure, head with the gather, tree combine, info of a tree-score call.  16-bit: the gather walks K in strides of 512 --
    one trip at 128, four live lanes in the second at 544, a partial second at 768, a full one at 1024.  fp32: chunks of 64 rows
    (the 70 leaves' parent row is up to two chunks back) and one chunk, bit for bit the same."""
    inp = T.tree_tail_inputs(_dt(kind), K)
    what = f"tree tail {kind} K={K}"
    out, bad, info, tgt, zt = _run_tail(inp, chunk_rows=64 if kind == "f32" else 0, tree_max_depth=T.TREE_MAX_DEPTH)
    ref, zt_ref = T.tree_expected(inp)
    assert bad == [0, 0, 0] and info == [inp["ld"], 0, 0, 0], (bad, info)
    assert bool((tgt == -1).all())
    assert torch.equal(torch.isnan(zt), torch.isnan(zt_ref)), (what, "logits gathered exactly for the nodes with a parent")
    _check_values(out, ref, T.head_tol(), what)
    if kind == "f32":
        one = _run_tail(inp, chunk_rows=inp["Q"] * inp["Lp"], tree_max_depth=T.TREE_MAX_DEPTH)
        assert torch.equal(_bits(one[0]), _bits(out)) and torch.equal(_bits(one[4]), _bits(zt)), (what, "one chunk against seven")
    else:
        rows, prow, tok, _ = T.tree_rows(inp)
        z, bound = T.gather_dot_bound(inp, rows, prow, tok)
        err = (zt[rows].double() - z).abs()
        print(f"{what}: gathered logit max error {float(err.max()):.3e}, {float((err / bound).max()):.3f} of the element-wise bound "
              f"2^-19 sum |x w| + 2^-23 |z| (largest bound {float(bound.max()):.3e})")
        _assert_within(zt[rows], z, bound, what + " gather dot")


@pytest.mark.parametrize("kind", ["f32", "16"])
def test_tree_tail_with_a_rejected_tree(experiment_build, kind):
    """a jump of 2 among the leaves of tree 1: flagged, its rows keep the sentinel, the other trees are bit for bit the clean run"""
    inp = T.tree_tail_inputs(_dt(kind), 128)
    chunk = 64 if kind == "f32" else 0
    clean = _run_tail(inp, chunk_rows=chunk, tree_max_depth=T.TREE_MAX_DEPTH)[0]
    inp["tokens"] = T.set_depth(inp["tokens"], 1, 40, 3)
    out, bad, info, _, _ = _run_tail(inp, chunk_rows=chunk, tree_max_depth=T.TREE_MAX_DEPTH)
    assert bad == [0, 1, 0] and info == [inp["ld"], 0, 0, 1], (bad, info)
    assert bool((out[1] == T.SENT_F).all())
    assert torch.equal(_bits(out[[0, 2]]), _bits(clean[[0, 2]]))


on_both_operand_builds(globals(), BUILD)
