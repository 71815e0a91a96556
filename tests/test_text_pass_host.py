"""CPU: the inputs of tests/test_gpu_text_pass_ops.py tell a wrong kernel from a right one.  For every defect below a CPU
rendering of the defect (text_pass_cases.py) differs from the fp64 reference by more than 10 times the tolerance the GPU test
applies at the named case, while the correct fp32 emulation of the same case stays inside that tolerance."""
import pytest
import torch

import text_pass_cases as T
from ln_reference import ln_ref_and_bound


def _excess(got, ref, bound):
    """max over the elements of |got - ref| / bound"""
    return float(((got.double() - ref).abs() / bound).max())


def _embed_case(D, **kw):
    inp = T.embed_inputs(D)
    tok, pos = T.embed_rows(inp)
    ref, bound = ln_ref_and_bound(T.embed_sum64(inp, tok, pos), inp["gamma"], inp["beta"], T.EMB_EPS)
    assert _excess(T.embed_emulate32(inp, tok, pos), ref, bound) <= 1.0
    return inp, ref, bound


def test_embedding_mean_over_the_first_wave_only():
    inp, ref, bound = _embed_case(768)
    tok, pos = T.embed_rows(inp)
    assert _excess(T.embed_emulate32(inp, tok, pos, first_wave_mean=True), ref, bound) > 10.0
    # D = 128 has no second wave: the same defect is invisible there, which is why 768 is among the sizes
    inp, ref, bound = _embed_case(128)
    tok, pos = T.embed_rows(inp)
    assert _excess(T.embed_emulate32(inp, tok, pos, first_wave_mean=True), ref, bound) <= 1.0


@pytest.mark.parametrize("D", [768, 1024, 128, 100])
def test_embedding_position_not_clamped(D):
    inp, ref, bound = _embed_case(D)
    tok, pos = T.embed_rows(inp, clamp_pos=False)
    assert int(pos.max()) >= T.EMB_MAXPOS
    assert _excess(T.embed_emulate32(inp, tok, pos), ref, bound) > 10.0


def _flat_err(got, ref):
    return float((got - ref).abs().max())


@pytest.mark.parametrize("shape", [T.FLAT_F32, T.FLAT_16_BIG], ids=["V1001", "V30522"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_last_tile_counted_as_128_columns(shape, dtype):
    inp = T.flat_inputs(shape, dtype)
    ref, written = T.flat_expected(inp)
    tol = T.head_tol()
    assert _flat_err(T.flat_emulate32(inp, False), ref) <= tol
    wrong = T.flat_emulate32(inp, False, full_last_tile=True)
    # the maximum shift over the rows: a row whose maximum lies in the last tile does not move at all
    shift = (wrong[..., 1] - ref[..., 1]).abs()[written]
    assert float(shift.max()) > 10 * tol, (float(shift.max()), tol)
    assert _flat_err(wrong[..., 0], ref[..., 0]) <= tol          # lp does not see the column count: only mean_lp catches it


def test_offset_case_emulation_stays_inside_the_tolerance():
    inp = T.flat_inputs(T.FLAT_16_BIG, torch.bfloat16, offset=1e3)
    ref, _ = T.flat_expected(inp)
    assert _flat_err(T.flat_emulate32(inp, False), ref) <= T.head_tol(1e3)


def test_logits_indexed_by_the_absolute_row_in_the_second_chunk():
    inp = T.flat_inputs(T.FLAT_F32, torch.float32)
    ref, _ = T.flat_expected(inp)
    tol = T.head_tol()
    assert _flat_err(T.flat_emulate32(inp, True), ref) <= tol
    assert _flat_err(T.flat_emulate32(inp, True, abs_row_chunk=64), ref) > 10 * tol
    # with one chunk the defect does not exist: the chunked run is what finds it
    assert _flat_err(T.flat_emulate32(inp, True, abs_row_chunk=inp["Q"] * inp["Lp"]), ref) <= tol


@pytest.mark.parametrize("shape", [T.FLAT_F32, T.FLAT_16_BIG], ids=["ld37_Lp48", "ld16_Lp16"])
def test_result_written_at_its_own_row_index(shape):
    inp = T.flat_inputs(shape, torch.float32)
    ref, written = T.flat_expected(inp)
    right = T.flat_emulate32(inp, True)
    assert _flat_err(right, ref) <= T.head_tol() and torch.equal(right[..., 0] != T.SENT_F, written)
    wrong = T.flat_emulate32(inp, True, own_index=True)
    assert _flat_err(wrong, ref) > 10 * T.head_tol()
    assert not torch.equal(wrong[..., 0] != T.SENT_F, written)     # the placement check alone sees it, at ld == Lp too (the + 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_child_gathered_from_its_own_row(dtype):
    inp = T.tree_tail_inputs(dtype, 128)
    f32_mode = dtype == torch.float32
    ref, _ = T.tree_expected(inp)
    assert _flat_err(T.tree_emulate32(inp, f32_mode), ref) <= T.head_tol()
    assert _flat_err(T.tree_emulate32(inp, f32_mode, own_row=True), ref) > 10 * T.head_tol()
    assert _flat_err(T.tree_expected(inp, own_row=True)[0], ref) > 10 * T.head_tol()     # the defect itself, without rounding
    # the 70 leaves' parent is row 2 of their tree: up to two 64-row chunks back
    rows, prow, _, bad = T.tree_rows(inp)
    assert bad.tolist() == [0, 0, 0] and int((rows // 64 - prow // 64).max()) == 2


@pytest.mark.parametrize("K", [544, 768, 1024])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gather_stopping_at_column_512(K, dtype):
    inp = T.tree_tail_inputs(dtype, K)
    rows, prow, tok, _ = T.tree_rows(inp)
    z, bound = T.gather_dot_bound(inp, rows, prow, tok)
    assert _excess(T.gather_dot32(inp, prow, tok), z, bound) <= 1.0
    assert _excess(T.gather_dot32(inp, prow, tok, stop=512), z, bound) > 10.0
    if K == 544:                                                 # the second stride's four live lanes: columns 512 .. 543
        assert _excess(T.gather_dot32(inp, prow, tok, stop=536), z, bound) > 1.0


def test_tree_tables_reference_on_a_known_tree():
    """the host walk itself, on a tree small enough to read: 0 -> (1 -> 2, 3), 4"""
    packed = torch.tensor([[(d << 32) | (10 + i) for i, d in enumerate([0, 1, 2, 2, 1])] + [0]], dtype=torch.int64)
    tab, bad = T.tree_tables_ref(packed, [5], 8, 12, 4)
    assert bad.tolist() == [0]
    assert tab[0].tolist() == [10, 11, 11, 11, 11, 0, 0, 0]                      # ids clamp to V - 1 = 11
    assert tab[1].tolist() == [0, 1, 2, 2, 1, 0, 0, 0]
    assert tab[2].tolist() == [-1, 0, 1, 1, 0, -1, -1, -1]
    assert tab[3].tolist() == [5, 4, 3, 4, 5, 6, 7, 8]
    for name, node, depth, max_depth in T.TREE_REJECTIONS:
        p, lens = T.tree_inputs()
        if node is not None:
            p = T.set_depth(p, 0, node, depth)
        tab, bad = T.tree_tables_ref(p, lens, T.TREE_LP, T.TREE_V, max_depth)
        assert bad.tolist() == [1, 0, 0], name
