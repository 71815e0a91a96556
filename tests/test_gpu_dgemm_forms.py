"""GPU: every launch form of the decode-chain GEMMs (csrc/kernels_dgemm.hip launch_dgemm_t) against fp64 torch, through the
measurement build's hook gitmi_debug_dgemm_form (include/gitmi_experiment.h): an argument check + the launcher the engine's
dgemm() calls, with the three DGemmArgs fields the engine sets by policy and gitmi_op_dgemm / gitmi_op_dgemm_res leave at 0 --
rows_per_wg (16 | 32 | 64 rows per workgroup), strips_per_wg (wide form, 33..64 rows) and no_row_walk (wide form, > 64 rows).

Forms: (a) the N = hidden producer dgemm_kernel<1 | 2 | 4, 4 | 8, DEPI_RES>; (b) the non-wide consumer <1 | 2 | 4, 4, DEPI_BF16>;
(c) the wide consumer above 64 rows, row-walking or one workgroup per (strip, row block), and at <= 32 rows; (d) the wide
consumer at 33..64 rows on 1 / 2 / 4 / 6 strips per workgroup with absent strips in the last workgroup; (e) refusals; (f) one
decoder layer's hand-over, every stage fed with the previous stage's device buffers as they are.

Every launch of the file runs on outputs pre-filled with a sentinel bit pattern and checks, bit for bit: the guard rows behind
C / x / xb, the rows M .. round_up(M, 16) inside a fragment-major xb / C, and a guard block behind the strip partials keep the
sentinel.  Every form is held to fp64 itself and must equal the default form (all three fields 0) as raw integers over the
whole output: NW depends on K only, so the summation order is the same in all forms of one shape.

Bounds (derived; tests/test_gpu_ops_f16.py holds the derivations): x fp32 -- _acc_err + 2 u (|bias| + |ref|), + 2e-5 where the
residual LayerNorm is rebuilt; xb -- equal to x.to(dtype) bit for bit (one rounding to nearest even); strip partials against
fp64 strip sums of the returned x -- |sum - ref| <= 16 u sum|x|, |sumsq - ref| <= 17 u sum x^2 (a value passes at most five
additions and one square); 16-bit consumer outputs -- test_dgemm_qkv_ffn1_form_f16's expressions with the half-ulp of the build's
type (bf16: 2^(e - 8); eight significant bits).  Tightness: the fp16 build runs _check16's assertion (the largest bound is
below half of bf16's half-ulp at the reference's largest magnitude: a bf16 rounding would not fit); the bf16 build asserts that the bound
WITHOUT its output-rounding term is below a quarter of a bf16 ulp at max |ref|, so a second rounding would not fit.  Both
assertions hold for every input of this file, computed on the CPU from the reference alone; the closest are recorded in
docs/LAB_NOTEBOOK.md."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from test_gpu_ops import _act, _rand
from test_gpu_ops_f16 import ACT_SLOPE, U, _acc_err, _check16, _fold_bound, _hulp

pytestmark = pytest.mark.gpu

GUARD = 3                # sentinel rows behind row-major outputs (fragment-major ones: one 16-row tile)
STAT_GUARD = 64          # sentinel floats behind the strip partials
EPS = 1e-12


# ---- both operand builds -------------------------------------------------------------------------------------------------------
# Every test of the file runs on the bf16 measurement build under its own name and, as <name>_f16, on the fp16 one
# (libgitmi_f16_exp.so): engine.op_dgemm_form picks the library by its tensors' type, BUILD says which type the test makes.
BUILD = {"ops": "bf16"}


def _op_dtype():
    return {"bf16": torch.bfloat16, "f16": torch.float16}[BUILD["ops"]]


def on_both_operand_builds(tests, build):
    """adds to the module namespace `tests` an fp16 twin <name>_f16 of every test_* function in it: the same marks, parameters
    and fixtures, run with build["ops"] = "f16" (test_gpu_attn_decode_forms.py and test_gpu_frontend_ops.py use it too)"""
    def twin_of(fn):
        @functools.wraps(fn)
        def twin(*args, **kw):
            build["ops"] = "f16"
            try:
                return fn(*args, **kw)
            finally:
                build["ops"] = "bf16"
        twin.__name__ = twin.__qualname__ = fn.__name__ + "_f16"
        return twin
    for name, fn in list(tests.items()):
        if name.startswith("test_") and callable(fn) and not name.endswith("_f16"):
            tests[name + "_f16"] = twin_of(fn)


def _dev(t):
    return t.cuda()


def _raw(t):
    """the elements as integers: bitwise comparisons that NaNs and signed zeros cannot blur"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _sentinel(shape, dtype):
    n = torch.full(shape, 0x7b7b7b7b if dtype == torch.float32 else 0x7b7b, dtype=torch.int32)
    return n.view(torch.float32) if dtype == torch.float32 else n.to(torch.int16).view(dtype)


def _is_sentinel(t):
    return bool((_raw(t) == (0x7b7b7b7b if t.dtype == torch.float32 else 0x7b7b)).all())


def _up(x, m):
    return (x + m - 1) // m * m


# ---- bounds ------------------------------------------------------------------------------------------------------------
RATIOS = {}              # (form family, build) -> worst error / bound seen (printed: docs/LAB_NOTEBOOK.md quotes them)
MARGINS = {}             # (form family, build) -> largest tightness figure / its limit seen


def _hold(out, ref, bound, rounding, dt, family, what):
    """|out - ref| <= bound element by element, after the build's tightness assertion on (ref, bound) alone.  rounding: the
    output-rounding term inside `bound` (0 for fp32 outputs)."""
    ref = ref.double()
    e = math.floor(math.log2(ref.abs().max().item()))
    key = (family, str(dt).split(".")[1])
    if dt == torch.float16:
        fig, lim = bound.max().item(), 0.5 * 2.0 ** (e - 8)                 # _check16's own assertion, repeated for the figure
    else:
        fig, lim = (bound - rounding).max().item(), 2.0 ** (e - 9)          # a quarter of a bf16 ulp at max |ref|
    MARGINS[key] = max(MARGINS.get(key, 0.0), fig / lim)
    assert fig < lim, (what, "bound too loose for its tightness assertion", fig, lim)
    err = (out.double() - ref).abs()
    assert torch.isfinite(err).all(), (what, "non-finite output")
    ratio = (err / bound).max().item()
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"RATIO {family} {key[1]} {ratio:.4f} worst {RATIOS[key]:.4f} | TIGHT {fig / lim:.4f} worst {MARGINS[key]:.4f}")
    if dt == torch.float16:
        _check16(out, ref, bound, what)
    elif ratio > 1.0:
        i = (err - bound).argmax()
        raise AssertionError(f"{what}: {int((err > bound).sum())} elements out of bound; worst: err {err.flatten()[i].item():.3e} "
                             f"bound {bound.flatten()[i].item():.3e} ref {ref.flatten()[i].item():.6g}")


def _same(got, base, what):
    """raw-integer equality of whole outputs (tuples of tensors)"""
    for name, a, b in zip(("first", "second", "third"), got, base):
        bad = (_raw(a) != _raw(b)).nonzero()
        assert bad.numel() == 0, (what, f"{name} output differs from the default form at", bad[0].tolist(), "in", bad.shape[0], "elements")


def _fold(W, bias, gamma, beta, dt):
    """gitmi_finalize_weights for a GEMM behind a LayerNorm: W' = dt(W . gamma), beta W^T + b, colsum(W')."""
    Wf = (W * gamma[None, :]).to(dt)
    return Wf, (bias.double() + W.double() @ beta.double()).float(), Wf.double().sum(1).float()


def _strip_sums(x):
    """fp64 strip sums of fp32 rows [M, N] -> (sum, sum of squares, sum |x|) each [N/16, M]"""
    xs = x.double().reshape(x.shape[0], -1, 16)
    return xs.sum(-1).t(), (xs * xs).sum(-1).t(), xs.abs().sum(-1).t()


def _check_partials(st, x, what):
    s, q, a = _strip_sums(x)
    es, eq = (st[..., 0].double() - s).abs(), (st[..., 1].double() - q).abs()
    assert (es <= 16 * U * a).all(), (what, "strip sums", (es / (16 * U * a).clamp_min(1e-300)).max().item())
    assert (eq <= 17 * U * q).all(), (what, "strip sums of squares", (eq / (17 * U * q).clamp_min(1e-300)).max().item())
    key = ("partials", "any")
    RATIOS[key] = max(RATIOS.get(key, 0.0), (es / (16 * U * a).clamp_min(1e-300)).max().item(),
                      (eq / (17 * U * q).clamp_min(1e-300)).max().item())
    print(f"RATIO partials worst {RATIOS[key]:.4f}")


# ---- producer (DEPI_RES) -----------------------------------------------------------------------------------------------
def _res_ref(A, W, bias, xprev, g, b, ln_res):
    """fp64 x = A W^T + bias + residual and its single-op bound"""
    N = W.shape[0]
    res = torch.nn.functional.layer_norm(xprev.double(), (N,), g.double(), b.double(), EPS) if ln_res else xprev.double()
    ref = A.double() @ W.double().t() + bias.double() + res
    return ref, _acc_err(A, W) + 2 * U * (bias.double().abs() + ref.abs()) + (2e-5 if ln_res else 0.0)


@functools.lru_cache(maxsize=2)
def _producer(dt, N, K, ln_res):
    """256 rows of inputs and reference, computed once: a launch over M rows uses the first M"""
    from generativeimage2text_amd import engine as E
    c = SimpleNamespace(dt=dt, N=N, K=K, ln_res=ln_res)
    c.A = _rand(256, K, seed=31).to(dt)
    c.W = _rand(N, K, seed=32, scale=K ** -0.5).to(dt)
    c.bias, c.xprev = _rand(N, seed=33), _rand(256, N, seed=34, scale=1.2) + 0.1
    c.g, c.b = 1 + _rand(N, seed=35, scale=0.1), _rand(N, seed=36, scale=0.1)
    c.ref, c.bound = _res_ref(c.A, c.W, c.bias, c.xprev, c.g, c.b, ln_res)
    c.res_stats = E.strip_stats(c.xprev)
    c.d = SimpleNamespace(W=_dev(E.to_frag(c.W)), bias=_dev(c.bias), g=_dev(c.g), b=_dev(c.b))
    return c


def _launch_res(A, W, bias, xprev, M, N, dt, form, res_stats=None, g=None, b=None, packed=False, xb_rows=None):
    """One producer launch on guarded outputs (all operands on the device) -> the three raw device buffers"""
    from generativeimage2text_amd import engine as E
    x = _dev(_sentinel((M + GUARD, N), torch.float32))
    xb = _dev(_sentinel(((xb_rows or _up(M, 16)) + 16, _up(N, 32)), dt))
    st = _dev(_sentinel(((N // 16) * M * 2 + STAT_GUARD,), torch.float32))
    E.op_dgemm_form(A, W, bias, M, res_x=xprev, res_stats=res_stats, res_gamma=g, res_beta=b, res_eps=EPS, x=x, xb=xb,
                    stats_out=st, packed=packed, **form)
    torch.cuda.synchronize()
    return x, xb, st


def _split_res(x, xb, st, M, N, what):
    """the guard checks of a producer's buffers (CPU copies) -> (x [M, N], xb decoded [M, N], partials [N/16, M, 2])"""
    from generativeimage2text_amd import engine as E
    Mp = _up(M, 16)
    assert _is_sentinel(x[M:]), (what, "guard rows behind x were written")
    assert _is_sentinel(xb[Mp:]), (what, "rows behind xb were written")
    rows = E.from_frag(xb[:Mp], Mp)                # round_up(N, 32) columns: N % 32 == 16 leaves the last k-step half used
    assert _is_sentinel(rows[M:]), (what, "rows M .. round_up(M, 16) of the fragment-major xb were written")
    assert _is_sentinel(rows[:, N:]), (what, "columns N .. round_up(N, 32) of the fragment-major xb were written")
    rows = rows[:, :N].contiguous()
    ns = (N // 16) * M * 2
    assert _is_sentinel(st[ns:]), (what, "guard block behind the strip partials was written")
    return x[:M], rows[:M], st[:ns].reshape(N // 16, M, 2)


def _check_res(got, ref, bound, dt, family, what):
    x, xb, st = got
    assert not _is_sentinel(x) and torch.isfinite(x).all(), (what, "x")
    _hold(x, ref, bound, 0.0, dt, family, what + " x")
    bad = (_raw(xb) != _raw(x.to(dt))).nonzero()
    assert bad.numel() == 0, (what, "xb is not x rounded once to nearest even; first at", bad[0].tolist(), "of", bad.shape[0])
    _check_partials(st, x, what)


ALL_M = (1, 16, 17, 32, 33, 48, 64, 65, 100, 256)
EDGE_M = (17, 33, 65, 100)
# (N, K): (16, 128) one strip, one k-step per wave | (80, 96) three k-steps for four waves, five strips | (768, 1152) 9 = 6 + 2 + 1
# k-steps per wave, all three chunk sizes | (1024, 2048) the first NW = 8 shape, all 64 strip slots of the residual's statistics
PRODUCER_SHAPES = [(16, 128, EDGE_M), (80, 96, EDGE_M), (768, 768, ALL_M), (768, 1152, EDGE_M), (1024, 2048, EDGE_M), (768, 3072, ALL_M)]


@pytest.mark.parametrize("N,K,rows", PRODUCER_SHAPES, ids=lambda v: str(v) if isinstance(v, int) else "M")
@pytest.mark.parametrize("ln_res", [False, True])
def test_producer_forms(experiment_build, N, K, rows, ln_res):
    """(a) out-proj / FFN2 form on 16 (default), 32 and 64 rows per workgroup: mt = 1 | 2 | 4 by the 16 | 17 and 32 | 33 row
    edges, blocks with one valid row (17, 33, 65), blocks with an absent tile (33 and 100 at 64 rows), the 512-thread forms
    at K >= 2048.  With more than one row tile wave i finishes tile i and writes that tile's strip partials."""
    from generativeimage2text_amd import engine as E
    dt = _op_dtype()
    c = _producer(dt, N, K, ln_res)
    for M in rows:
        A, xprev = _dev(E.to_frag(c.A[:M], 64)), _dev(c.xprev[:M].contiguous())
        kw = dict(res_stats=_dev(c.res_stats[:, :M].contiguous()), g=c.d.g, b=c.d.b) if ln_res else {}
        base = None
        for rpw in (0, 32, 64):
            what = f"M={M} rows_per_wg={rpw}"
            bufs = _launch_res(A, c.d.W, c.d.bias, xprev, M, N, dt, dict(rows_per_wg=rpw), **kw, packed=True)
            got = _split_res(*(t.cpu() for t in bufs), M, N, what)
            _check_res(got, c.ref[:M], c.bound[:M], dt, f"producer{rpw}", what)
            if base is None:
                base = got
            else:
                _same(got, base, what)


# ---- consumers (DEPI_BF16) -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _consumer(dt, N, K, fold, act, rows=300):
    """`rows` rows of inputs and reference of the QKV / FFN1 form, computed once.  Plain: A = dt(x).  Folded: x are the raw fp32
    rows behind A, LayerNorm(x) folded into W', the constant and colsum; statistics from the fp32 strip partials of x."""
    from generativeimage2text_amd import engine as E
    c = SimpleNamespace(dt=dt, N=N, K=K, fold=fold, act=act)
    W, bias = _rand(N, K, seed=22, scale=K ** -0.5), _rand(N, seed=23)
    c.x = _rand(rows, K, seed=21, scale=1.3) + 0.2
    c.A = c.x.to(dt)
    if not fold:
        c.W = W.to(dt)
        pre = c.A.double() @ c.W.double().t() + bias.double()
        c.ref = _act(pre, act)
        c.round = _hulp(c.ref, dt)
        c.bound = ACT_SLOPE * (_acc_err(c.A, c.W) + U * bias.double().abs()) + 8 * U * pre.abs() + c.round
        c.d = SimpleNamespace(W=_dev(E.to_frag(c.W)), bias=_dev(bias), cs=None)
        c.stats = None
        return c
    gamma, beta = 1 + _rand(K, seed=24, scale=0.1), _rand(K, seed=25, scale=0.1)
    c.W, bf, cs = _fold(W, bias, gamma, beta, dt)
    c.ref, c.bound, c.round = _fold_ref(c.x, c.W, bf, cs, act, dt)
    c.stats = E.strip_stats(c.x)
    c.d = SimpleNamespace(W=_dev(E.to_frag(c.W)), bias=_dev(bf), cs=_dev(cs))
    return c


def _fold_ref(x, Wf, bf, cs, act, dt):
    """fp64 act(rstd (dt(x) W'^T - mean colsum) + b') with mean / var of the raw fp32 rows -> (ref, bound, rounding term)"""
    mean, var = x.double().mean(1, keepdim=True), x.double().var(1, unbiased=False, keepdim=True)
    pre = (x.to(dt).double() @ Wf.double().t() - mean * cs.double()) / torch.sqrt(var + EPS)
    ref = _act(pre + bf.double(), act)
    return ref, _fold_bound(x, Wf, cs, ref, EPS, act, dt=dt), _hulp(ref, dt)


def _launch_c(A, W, bias, M, N, dt, form, frag, colsum=None, stats=None, act=0, packed=False, out_rows=None):
    """One consumer launch on a guarded output (operands on the device) -> the raw device buffer"""
    from generativeimage2text_amd import engine as E
    rows = (out_rows or _up(M, 16)) + 16 if frag else M + GUARD
    out = _dev(_sentinel((rows, N), dt))
    E.op_dgemm_form(A, W, bias, M, colsum=colsum, stats=stats, eps=EPS, act=act, frag_out=frag, out=out, packed=packed, **form)
    torch.cuda.synchronize()
    return out


def _split_c(out, M, frag, what):
    """the guard checks of a consumer's buffer (CPU copy) -> its rows [M, N]"""
    from generativeimage2text_amd import engine as E
    if not frag:
        assert _is_sentinel(out[M:]), (what, "guard rows behind C were written")
        return out[:M]
    Mp = _up(M, 16)
    assert _is_sentinel(out[Mp:]), (what, "rows behind the fragment-major C were written")
    rows = E.from_frag(out[:Mp], Mp)
    assert _is_sentinel(rows[M:]), (what, "rows M .. round_up(M, 16) of the fragment-major C were written")
    return rows[:M]


def _consumer_forms(c, M, forms, family, frags=(False,)):
    """every form of `forms` (the first: the default form) over the first M rows of case c, row-major and (frags) fragment-major:
    guards, fp64, and raw equality with the default form's row-major rows -> those rows"""
    from generativeimage2text_amd import engine as E
    A = _dev(E.to_frag(c.A[:M], 64))
    stats = _dev(c.stats[:, :M].contiguous()) if c.fold else None
    base = None
    for form in forms:
        for frag in frags:
            what = f"M={M} {form} frag={frag}"
            out = _launch_c(A, c.d.W, c.d.bias, M, c.N, c.dt, form, frag, colsum=c.d.cs, stats=stats, act=c.act, packed=True).cpu()
            rows = _split_c(out, M, frag, what)
            assert not _is_sentinel(rows), what
            _hold(rows, c.ref[:M], c.bound[:M], c.round[:M], c.dt, family, what)
            if base is None:
                base = rows
            else:
                _same((rows,), (base,), what)
    return base


@pytest.mark.parametrize("N", [130, 512, 1002, 1520])
@pytest.mark.parametrize("K", [96, 128, 768])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("act", [0, 2])
def test_narrow_consumer_forms(experiment_build, N, K, fold, act):
    """(b) N < 1536 on 16 / 32 / 64 rows per workgroup (MT = 1 | 2 | 4): what every small-config parity test runs.  130 and 1002
    have column tails and take the scalar store path; 512 also writes fragment-major."""
    c = _consumer(_op_dtype(), N, K, fold, act, rows=100)
    for M in EDGE_M:
        _consumer_forms(c, M, [dict(rows_per_wg=r) for r in (0, 32, 64)], "narrow", (False, True) if N % 32 == 0 else (False,))


@pytest.mark.parametrize("N,K", [(1536, 96), (1536, 768), (1560, 96), (1560, 768), (2304, 96), (2304, 768), (1536, 1024)])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("act", [0, 2])
def test_wide_consumer_above_64_rows(experiment_build, N, K, fold, act):
    """(c) the row-walking kernel (default) and one workgroup per (strip, row block) (no_row_walk: dgemm_kernel<4, 4> with
    gridDim.y > 1, the default of a context that has the device to itself): partial last blocks (65, 129, 300), whole ones (128,
    256).  K = 1024 is past the row walk's six k-steps per wave: both settings take the one-block kernel.  1560: a half strip."""
    c = _consumer(_op_dtype(), N, K, fold, act, rows=300)
    for M in (65, 128, 129, 256, 300) if K != 1024 else (65, 129, 300):
        _consumer_forms(c, M, [dict(no_row_walk=w) for w in (0, 1)], "wide>64", (False, True) if N % 32 == 0 else (False,))


@pytest.mark.parametrize("K", [96, 768])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("act", [0, 2])
def test_wide_consumer_up_to_32_rows(experiment_build, K, fold, act):
    """(c) N = 1536 at 1, 16 (<1, 4>), 17 and 32 rows (<2, 4>) on one row block: held to fp64, and equal bit for bit to rows
    [0, M) of a 64-row launch of the same rows."""
    dt = _op_dtype()
    c = _consumer(dt, 1536, K, fold, act, rows=300)
    full = _consumer_forms(c, 64, [dict()], "wide<=64")
    for M in (1, 16, 17, 32):
        rows = _consumer_forms(c, M, [dict()], "wide<=32", (False, True))
        _same((rows,), (full[:M],), f"M={M} against the 64-row launch")


@pytest.mark.parametrize("N", [1552, 1560])
@pytest.mark.parametrize("K", [96, 768])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("act", [0, 2])
def test_wide_consumer_strips_per_workgroup(experiment_build, N, K, fold, act):
    """(d) 33..64 rows on 1 (default: dgemm_kernel<4, 4>), 2, 4 and 6 strips per workgroup: 97 and 98 strips divide by none of
    4 and 6 (97 not by 2 either), so the last workgroup has absent strips; 1560 ends in a half strip."""
    c = _consumer(_op_dtype(), N, K, fold, act, rows=64)
    for M in (33, 48, 50, 64):
        _consumer_forms(c, M, [dict(strips_per_wg=s) for s in (0, 2, 4, 6)], "wide-strips")


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(experiment_build):
    """(e) every refusal of the hook: the error names it, nothing is launched (the outputs keep their sentinel).  M = 0 succeeds
    and writes nothing."""
    from generativeimage2text_amd import engine as E
    lib = E._exp_library(_op_dtype())
    hook = E._experiment_only(lib, "gitmi_debug_dgemm_form")
    zeros = torch.zeros(1 << 20, device="cuda")
    outs = _dev(_sentinel((3, 1 << 18), torch.float32))
    z, (c, x, xb), s = zeros.data_ptr(), (outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()), E._stream()
    st = outs[2][1 << 17:].data_ptr()

    def consumer(a_rows=64, bias=z, colsum=None, stats=None, strips=0, C=c, c_frag=0, x_out=None, M=64, N=64, K=64):
        return hook(z, a_rows, z, bias, colsum, stats, strips, EPS, C, c_frag, 0, None, None, 0, None, None, EPS, x_out, None, None,
                    M, N, K, 0, 0, 0, s)

    def producer(res_x=z, res_stats=None, res_strips=0, g=None, b=None, xb_out=xb, stats_out=st, C=None, M=64, N=64, K=64):
        return hook(z, 64, z, z, None, None, 0, EPS, C, 0, 0, res_x, res_stats, res_strips, g, b, EPS, x, xb_out, stats_out,
                    M, N, K, 0, 0, 0, s)

    refused = {
        "K must be a multiple of 32": lambda: consumer(K=48),
        "K must be a multiple of 32 ": lambda: producer(K=80),
        "x_out epilogue needs N %": lambda: producer(N=24),
        "c_frag needs N %": lambda: consumer(N=48, c_frag=1),
        "stats without colsum": lambda: consumer(stats=z, strips=4),
        "strips=66 outside": lambda: consumer(colsum=z, stats=z, strips=66, K=1056),
        "res_strips=65 outside": lambda: producer(res_stats=z, res_strips=65, g=z, b=z, N=1040),
        "exactly one of C and x_out": lambda: consumer(x_out=x),
        "exactly one of C and x_out ": lambda: consumer(C=None),
        "null argument": lambda: consumer(bias=None),
        "needs xb_out, stats_out and res_x": lambda: producer(xb_out=None),
        "needs xb_out, stats_out and res_x ": lambda: producer(stats_out=None),
        "needs xb_out, stats_out and res_x  ": lambda: producer(res_x=None),
        "res_stats without res_gamma": lambda: producer(res_stats=z, res_strips=4, g=z),
        "a_rows=64, but M=65": lambda: consumer(M=65),
        "a_rows=16, but M=16": lambda: consumer(a_rows=16, M=16),
    }
    for name, call in refused.items():
        with pytest.raises(E.GitmiError, match=name.strip()):
            E._ck(call(), lib)
    assert consumer(M=0) == 0 and producer(M=0) == 0
    torch.cuda.synchronize()
    assert _is_sentinel(outs.cpu()) and zeros.abs().sum().item() == 0
    own = torch.zeros(64, 64, dtype=_op_dtype(), device="cuda")            # each 16-bit type has its library: a mixed pair has none
    other = own.to(torch.float16 if own.dtype == torch.bfloat16 else torch.bfloat16)
    with pytest.raises(E.GitmiError, match="operands must"):
        E.op_dgemm_form(own, other, zeros[:64])
    with pytest.raises(E.GitmiError, match="operands must"):
        E.op_dgemm_form(own.float(), own.float(), zeros[:64])


# ---- one decoder layer's hand-over ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _layer(dt):
    """weights of one post-norm decoder layer's GEMM chain at d = 768, ffn = 3072 (+ the next layer's QKV), packed once"""
    from generativeimage2text_amd import engine as E
    d, ffn = 768, 3072
    L = SimpleNamespace(d=d, ffn=ffn)
    L.Wo, L.bo = _rand(d, d, seed=71, scale=d ** -0.5).to(dt), _rand(d, seed=72)
    L.g0, L.b0 = 1 + _rand(d, seed=73, scale=0.1), _rand(d, seed=74, scale=0.1)          # LayerNorm of the layer's input rows
    L.g1, L.b1 = 1 + _rand(d, seed=75, scale=0.1), _rand(d, seed=76, scale=0.1)          # attention-output LayerNorm
    L.g2, L.b2 = 1 + _rand(d, seed=77, scale=0.1), _rand(d, seed=78, scale=0.1)          # output LayerNorm
    L.W1, L.c1, L.cs1 = _fold(_rand(ffn, d, seed=79, scale=d ** -0.5), _rand(ffn, seed=80), L.g1, L.b1, dt)
    L.W2, L.b2f = _rand(d, ffn, seed=81, scale=ffn ** -0.5).to(dt), _rand(d, seed=82)
    L.Wq, L.cq, L.csq = _fold(_rand(3 * d, d, seed=83, scale=d ** -0.5), _rand(3 * d, seed=84), L.g2, L.b2, dt)
    L.dev = SimpleNamespace(**{k: _dev(E.to_frag(v) if k.startswith("W") else v) for k, v in vars(L).items()
                               if isinstance(v, torch.Tensor)})
    return L


@pytest.mark.parametrize("R", [33, 64, 100])
def test_layer_hand_over(experiment_build, R):
    """(f) out-proj -> FFN1 -> FFN2 -> next QKV with packed operands throughout, every stage reading the previous stage's device
    buffers as they are (xb and its strip partials, the fragment-major FFN1 output), under the fields of a context that has the
    device to itself (16 rows / 1 strip / no row walk) and of the serving policy (32 / 2 / row walk); above 64 rows both run 64
    rows per workgroup, as the engine's dgemm() sets it.  Every stage bit-equal between the two, and held to fp64 with the
    single-op bound against a reference computed from that stage's own read-back inputs, so bounds do not compound."""
    from generativeimage2text_amd import engine as E
    dt = _op_dtype()
    L, D = _layer(dt), _layer(dt).dev
    d, ffn, R64 = L.d, L.ffn, _up(R, 64)
    x0 = _rand(R, d, seed=90 + R, scale=1.2) + 0.1
    st0 = E.strip_stats(x0)
    ctx = _rand(R, d, seed=91 + R).to(dt)
    ctx_f = E.to_frag(ctx, 64)
    runs = []
    for name, rpw, spw, nrw in (("solo", 16, 1, 1), ("serving", 32, 2, 0)):
        form = dict(rows_per_wg=64 if R > 64 else rpw, strips_per_wg=spw, no_row_walk=nrw)
        b2 = _launch_res(_dev(ctx_f), D.Wo, D.bo, _dev(x0), R, d, dt, form, res_stats=_dev(st0), g=D.g0, b=D.b0, packed=True, xb_rows=R64)
        st1 = b2[2][:(d // 16) * R * 2].view(d // 16, R, 2)
        h = _launch_c(b2[1], D.W1, D.c1, R, ffn, dt, form, True, colsum=D.cs1, stats=st1, act=2, packed=True, out_rows=R64)
        b4 = _launch_res(h, D.W2, D.b2f, b2[0][:R], R, d, dt, form, res_stats=st1, g=D.g1, b=D.b1, packed=True, xb_rows=R64)
        st2 = b4[2][:(d // 16) * R * 2].view(d // 16, R, 2)
        qkv = _launch_c(b4[1], D.Wq, D.cq, R, 3 * d, dt, form, False, colsum=D.csq, stats=st2, act=0, packed=True)
        what = f"R={R} {name}"
        # guards: xb / h were allocated with round_up(R, 64) rows (they are operands of the next stage); rows past
        # round_up(R, 16) must still hold the sentinel
        s2 = _split_res(b2[0].cpu(), torch.cat([b2[1].cpu()[:_up(R, 16)], b2[1].cpu()[R64:]]), b2[2].cpu(), R, d, what + " out-proj")
        assert _is_sentinel(b2[1].cpu()[_up(R, 16):]), what
        hc = h.cpu()
        assert _is_sentinel(hc[_up(R, 16):]), (what, "rows behind the fragment-major FFN1 output were written")
        s3 = _split_c(hc[:_up(R, 16) + 16], R, True, what + " FFN1")
        s4 = _split_res(b4[0].cpu(), torch.cat([b4[1].cpu()[:_up(R, 16)], b4[1].cpu()[R64:]]), b4[2].cpu(), R, d, what + " FFN2")
        assert _is_sentinel(b4[1].cpu()[_up(R, 16):]), what
        s5 = _split_c(qkv.cpu(), R, False, what + " QKV")
        runs.append((s2, s3, s4, s5))
    (s2, s3, s4, s5), other = runs
    for stage, a, b in zip(("out-proj", "FFN1", "FFN2", "QKV"), runs[0], other):
        _same(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,), f"R={R} {stage}: solo against serving fields")
    ref, bound = _res_ref(ctx, L.Wo, L.bo, x0, L.g0, L.b0, True)
    _check_res(s2, ref, bound, dt, "layer", f"R={R} out-proj")
    x1 = s2[0]
    ref, bound, rnd = _fold_ref(x1, L.W1, L.c1, L.cs1, 2, dt)
    _hold(s3, ref, bound, rnd, dt, "layer", f"R={R} FFN1")
    ref, bound = _res_ref(s3, L.W2, L.b2f, x1, L.g1, L.b1, True)
    _check_res(s4, ref, bound, dt, "layer", f"R={R} FFN2")
    ref, bound, rnd = _fold_ref(s4[0], L.Wq, L.cq, L.csq, 0, dt)
    _hold(s5, ref, bound, rnd, dt, "layer", f"R={R} QKV")


on_both_operand_builds(globals(), BUILD)
