"""GPU: every launch form of the large-M GEMM (csrc/kernels_gemm10.hip gemm_p8_kernel) and the tile-kernel forms the engine
runs (csrc/kernels_gemm.hip) against fp64 torch, through the measurement builds' hook gitmi_debug_gemm_form
(include/gitmi_experiment.h): an argument check + launch_gemm with everything the engine's gemm_args / gemm_run / ln_gemm /
gemm_to_stream set -- leading dimensions of their own, `shared`, the folded-LayerNorm fields.  Tile heights (256 / 224 = 128 + 96 /
192 / 160 = 96 + 64 / 128 rows) and XCD partitions are forced through set_gemm_impl's bits.  Run on both operand builds
(libgitmi_exp.so, libgitmi_f16_exp.so); the folded forms exist in the fp16 one only.

Families: (a) the plain epilogues at every tile height; (b) the folded consumer (LNF 1) and producer (LNF 2) at every tile
height; (c) the prefill's K|V column slice of a [M, 3d] buffer; (d) forced XCD partitions; (e) the tile kernel's logits form
(N % 8 != 0, ldc = round_up(N, 8)) and the patch-embedding form (no bias, fp32 rows).

Every launch writes into sentinel-filled outputs and first checks, bit for bit: the guard rows behind C, the columns of C outside
[col0, col0 + N), the guard rows behind the producer's partials, and that the unused partial slots (slot 3 at N = 768) of the
zero-initialised partial rows are still exactly zero (launchers.h: "unused slots 0").  Every height, `shared = 1` and every
partition must equal the forced 256-row tile / the planned partition as raw integers; the base launch is held to fp64.

Row counts: every p8 case needs more than 512 rows.  For a height bm with half tiles (h0, h1): M = k bm + r with k the smallest
tile count reaching 512 rows and r in {1, h0, h0 + 1, bm - 1} -- a last tile of one row, of exactly the first half tile, one row
into the second, one row short -- and M = (k + 1) bm exactly.

Bounds (derived; tests/test_gpu_ops_f16.py holds _acc_err, ACT_SLOPE, _hulp, _fold_bound):
  plain: test_gemm_f16_epilogues' expressions with _hulp(., dt) of the build's type; a 16-bit epilogue with a residual is checked
    bit for bit as dt(fp32(y16) + res), y16 the same launch without the residual (gemm_p8_kernel adds the residual after rounding).
  consumer: _fold_bound without its statistics term, plus what THIS kernel does with the statistics: four fp32 (sum, sumsq)
    partials per row, supplied rounded once from fp64 (u each) and added as (p0 + p2) + (p1 + p3) (2 u more):
      |d sum| <= 3 u sum_t |s_t|,  |d sumsq| <= 3 u sumsq;   with am = sum_t |s_t| / K (|mean| <= am <= sqrt(E[x^2])):
      mean = sum * fl(1 / K): |d mean| <= 5 u am;   E2 = sumsq * fl(1 / K): 5 u E2;   mean^2: 2 |mean| |d mean| + u mean^2 <= 11 u am^2;
      the subtraction and the eps add: u E2 each at most  =>  |d var| <= 18 u E2,
      rstd: 0.5 |d var| / (var + eps) + 4 u (the reciprocal square root, as in _fold_bound) = 9 u E2 / (var + eps) + 4 u.
    The mean's error moves pre by rstd |d mean| |colsum|, the rstd's by |pre| d rstd; both pass the activation (ACT_SLOPE).
  producer rows: acc + half an fp16 ulp (plain); with a residual the kernel rounds y to fp16 first and adds after -- checked bit
    for bit as fp16(fp32(y16) + res16) against the plain producer launch, and held to fp64 with both roundings
    (acc + hulp16(y) + u |ref| + hulp16(|ref| + all of that): the rounded sum may lie one binade up); post-norm adds the rebuilt LayerNorm's error |g| rstd |d mean| +
    |(r - mean) rstd g| (d rstd + 2 u) + u |LN| with the statistics terms above (K -> N).
  producer partials against fp64 sums of the STORED rows: a thread adds its 8 values in pairs (3 roundings; the first add to 0
    is exact), the pair (1), then 5 DPP additions over the 32 lanes of the row: 9 roundings, the squares the same (x^2 of an
    fp16 value is exact in fp32, each fma rounds once): |sum - ref| <= g9 sum |x|, |sumsq - ref| <= g9 sum x^2, g9 = 9 u / (1 - 9 u).
  fp32 operands (tile kernel, v_mfma_f32_16x16x4_f32 = an fp32 fma chain over K): K u / (1 - K u) sum |a w| in place of _acc_err.
Tightness: every bound carries the assertion of its output's type before anything is compared -- fp16 and fp32 outputs
_check16's (the largest bound below half of bf16's half-ulp at the reference's largest magnitude), bf16 outputs that the bound
WITHOUT its output-rounding term is below a quarter of a bf16 ulp there.  They are conditions on the inputs: the offset-30
consumer case uses a bias of scale 8 so that the rstd term (|mean| / sigma up to ~70) stays under it.  Checked on the CPU for
every input of this file from the reference alone; docs/LAB_NOTEBOOK.md records the largest figures and the measured ratios."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from test_gpu_ln_fold import _stream_rows, _tile_partials
from test_gpu_ops import _act, _rand
from test_gpu_ops_f16 import ACT_SLOPE, U, _acc_err, _check16, _fold_bound, _hulp, _hulp16

pytestmark = pytest.mark.gpu

GUARD = 3                         # sentinel rows behind C and behind the row partials
OPS = ["bf16", "f16"]
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
HEIGHT_BITS = {256: 128, 224: 32768, 192: 64, 160: 16384, 128: 65536}          # set_gemm_impl: 9 | (bits << 8)
HALVES = {256: (128, 128), 224: (128, 96), 192: (96, 96), 160: (96, 64), 128: (64, 64)}
NG_BITS = {1: 1024, 2: 2048, 4: 4096, 8: 8192}
G9 = 9 * U / (1 - 9 * U)
MAX_ROWS = 896                    # 4 x 224: the largest row count of _edge_rows


def _edge_rows(bm):
    h0 = HALVES[bm][0]
    k = -(-512 // bm)
    return [k * bm + r for r in (1, h0, h0 + 1, bm - 1)] + [(k + 1) * bm]


def _dev(t):
    return t.cuda()


def _raw(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _sentinel(shape, dtype):
    """a device tensor of `dtype` whose every element is the bit pattern 0x7b7b(7b7b): finite, and no value these tests produce"""
    n = _dev(torch.full(shape, 0x7b7b7b7b if dtype == torch.float32 else 0x7b7b, dtype=torch.int32 if dtype == torch.float32 else torch.int16))
    return n.view(dtype)


def _is_sentinel(t):
    return t.numel() == 0 or bool((_raw(t) == (0x7b7b7b7b if t.dtype == torch.float32 else 0x7b7b)).all())


def _no_sentinel(t):
    return not bool((_raw(t) == (0x7b7b7b7b if t.dtype == torch.float32 else 0x7b7b)).any())


class _impl:
    """set_gemm_impl(9 | bits << 8) for a block (bits 0: the launcher's own height and partition), back to auto after"""

    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        from generativeimage2text_amd import engine as E
        E.set_gemm_impl(9 | (self.bits << 8) if self.bits else -1)

    def __exit__(self, *exc):
        from generativeimage2text_amd import engine as E
        E.set_gemm_impl(-1)


# ---- one launch on guarded outputs ----------------------------------------------------------------------------------------------
def _launch(A, W, M, N, K, out_dt, what, *, bits=0, ldc=None, col0=0, want_part=False, **kw):
    """gitmi_debug_gemm_form over the first M rows of A into columns [col0, col0 + N) of a sentinel-filled [M + GUARD, ldc] buffer
    (and, want_part, into zero-initialised partial rows [M, 4, 2] with sentinel rows behind them); the guard checks -> (C [M, N],
    partials [M, 4, 2] or None), on the device."""
    from generativeimage2text_amd import engine as E
    ldc = N if ldc is None else ldc
    buf = _sentinel((M + GUARD, ldc), out_dt)
    part = None
    if want_part:
        part = _sentinel((M + GUARD, 4, 2), torch.float32)
        part[:M] = 0
    with _impl(bits):
        E.op_gemm_form(A, W, buf[:, col0:], M, N, K, ldc=ldc, part_out=part, **kw)
    torch.cuda.synchronize()
    assert _is_sentinel(buf[M:]), (what, "guard rows behind C were written")
    assert _is_sentinel(buf[:M, :col0]) and _is_sentinel(buf[:M, col0 + N:]), (what, "columns of C outside [col0, col0 + N) were written")
    if want_part:
        assert _is_sentinel(part[M:]), (what, "guard rows behind the row partials were written")
        assert bool((_raw(part[:M, N // 256:]) == 0).all()), (what, "an unused partial slot is not exactly zero")
        part = part[:M]
    return buf[:M, col0:col0 + N], part


def _same(got, base, what):
    bad = (_raw(got) != _raw(base)).nonzero()
    assert bad.numel() == 0, (what, "differs from the base launch at", bad[0].tolist(), "in", bad.shape[0], "elements")


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
RATIOS = {}              # (family, build) -> worst error / bound seen (printed: docs/LAB_NOTEBOOK.md quotes them)
MARGINS = {}             # (family, build) -> largest tightness figure / its limit seen


def _hold(out, ref, bound, rounding, family, ops, what):
    """the tightness assertion of out's type on (ref, bound) alone, then |out - ref| <= bound element by element.  rounding: the
    output-rounding term inside `bound` (0 for fp32 outputs)."""
    out, ref = out.cpu(), ref.double()
    lim = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 9)           # half of bf16's half-ulp = a quarter of its ulp
    fig = ((bound - rounding) if out.dtype == torch.bfloat16 else bound).max().item()
    key = (family, ops)
    MARGINS[key] = max(MARGINS.get(key, 0.0), fig / lim)
    assert fig < lim, (what, "bound too loose for its tightness assertion", fig, lim)
    err = (out.double() - ref).abs()
    assert torch.isfinite(err).all(), (what, "non-finite output")
    ratio = (err / bound).max().item()
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"RATIO {family} {ops} {ratio:.4f} worst {RATIOS[key]:.4f} | TIGHT {fig / lim:.4f} worst {MARGINS[key]:.4f}")
    if out.dtype != torch.bfloat16:
        _check16(out, ref, bound, what)
    elif ratio > 1.0:
        i = (err - bound).argmax()
        raise AssertionError(f"{what}: {int((err > bound).sum())} elements out of bound; worst: err {err.flatten()[i].item():.3e} "
                             f"bound {bound.flatten()[i].item():.3e} ref {ref.flatten()[i].item():.6g}")


def _stat_terms(x):
    """(|d mean| bound, relative d rstd bound without eps) of a row's statistics rebuilt from four fp32 partials (module docstring)"""
    x = x.double()
    K = x.shape[1]
    am = _tile_partials(x)[:, :, 0].abs().sum(1, keepdim=True) / K
    e2, var = (x * x).mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    return 5 * U * am, e2, var


def _check_partials(part, rows, family, what):
    """producer partials against fp64 tile sums of the rows as stored: 9 roundings each"""
    x = rows.cpu().double()
    M, N = x.shape
    t = x.reshape(M, N // 256, 256)
    s, q, a = t.sum(-1), (t * t).sum(-1), t.abs().sum(-1)
    p = part.cpu().double()[:, :N // 256]
    es, eq = (p[..., 0] - s).abs(), (p[..., 1] - q).abs()
    rs, rq = (es / (G9 * a).clamp_min(1e-300)).max().item(), (eq / (G9 * q).clamp_min(1e-300)).max().item()
    key = (family, "partials")
    RATIOS[key] = max(RATIOS.get(key, 0.0), rs, rq)
    print(f"RATIO {family} partials {max(rs, rq):.4f} worst {RATIOS[key]:.4f}")
    assert rs <= 1.0, (what, "tile sums", rs)
    assert rq <= 1.0, (what, "tile sums of squares", rq)


# ---- (a) plain forms ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _plain_case(ops, N, K, rows=MAX_ROWS, in_f32=False):
    """`rows` rows of inputs, the fp64 pre-activation and its accumulation bound, computed once"""
    dt = torch.float32 if in_f32 else DT[ops]
    c = SimpleNamespace(ops=ops, dt=dt, N=N, K=K)
    c.A, c.W = _rand(rows, K, seed=1).to(dt), _rand(N, K, seed=2, scale=K ** -0.5).to(dt)
    c.bias, c.res = _rand(N, seed=3), _rand(rows, N, seed=4)
    c.res16 = c.res.half()
    c.mm = c.A.double() @ c.W.double().t()
    c.pre = c.mm + c.bias.double()
    if in_f32:
        c.acc_mm = K * U / (1 - K * U) * (c.A.double().abs() @ c.W.double().abs().t())
    else:
        c.acc_mm = _acc_err(c.A, c.W)
    c.d = SimpleNamespace(A=_dev(c.A), W=_dev(c.W), bias=_dev(c.bias), res=_dev(c.res), res16=_dev(c.res16))
    return c


def _plain_acc(c, act, bias=True):
    pre = c.pre if bias else c.mm
    return _act(pre, act), ACT_SLOPE * (c.acc_mm + (U * c.bias.double().abs() if bias else 0.0)) + 8 * U * pre.abs()


def _plain_forms(c, M, act, bits, what, shared=False):
    """the five plain epilogues of one (M, act) -> the outputs on the device, in a fixed order"""
    d, odt = c.d, c.dt
    kw = dict(bias=d.bias, act=act, bits=bits, shared=shared)
    res, res16 = d.res[:M], d.res16[:M]
    return [
        _launch(d.A, d.W, M, c.N, c.K, torch.float32, what + " fp32 + residual", res=res, ldr=c.N, **kw)[0],
        _launch(d.A, d.W, M, c.N, c.K, odt, what + " 16-bit", **kw)[0],
        _launch(d.A, d.W, M, c.N, c.K, odt, what + " 16-bit + residual", res=res, ldr=c.N, **kw)[0],
        _launch(d.A, d.W, M, c.N, c.K, torch.float16, what + " stream", stream_rows=True, **kw)[0],
        _launch(d.A, d.W, M, c.N, c.K, torch.float16, what + " stream + residual", stream_rows=True, res=res16, ldr=c.N, **kw)[0],
    ]


def _hold_plain(c, outs, M, act, family, what):
    f32r, o16, o16r, st, str_ = outs
    y, acc = _plain_acc(c, act)
    y, acc = y[:M], acc[:M]
    ref = y + c.res[:M].double()
    _hold(f32r, ref, acc + U * ref.abs(), 0.0, family, c.ops, what + " fp32 + residual")
    _hold(o16, y, acc + _hulp(y, c.dt), _hulp(y, c.dt), family, c.ops, what + " 16-bit")
    _same(o16r, (o16.float() + c.d.res[:M]).to(c.dt), what + " 16-bit + residual: dt(fp32(y16) + res)")
    _hold(st, y, acc + _hulp16(y), _hulp16(y), family, c.ops, what + " stream")
    _same(str_, (st.float() + c.d.res16[:M].float()).half(), what + " stream + residual: fp16(fp32(y16) + res16)")


@pytest.mark.parametrize("ops", OPS)
@pytest.mark.parametrize("N,K", [(768, 192), (512, 128)])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("bm", sorted(HEIGHT_BITS))
def test_plain_forms_at_every_tile_height(experiment_build, ops, N, K, act, bm):
    """(a) fp32 rows with an fp32 residual, operand-type rows with and without a residual, fp16 stream rows with and without an
    fp16 residual, at the ragged row counts of height bm: the forced height, the launcher's own and `shared = 1` equal the forced
    256-row tile as raw integers (shared = 1 IS that instantiation); the 256-row launch is held to fp64.  K = 128 is the
    shortest K loop (no steady-state K tile), K = 192 runs each of its three stages once."""
    c = _plain_case(ops, N, K)
    for M in _edge_rows(bm):
        what = f"{ops} N={N} K={K} act={act} M={M}"
        base = _plain_forms(c, M, act, HEIGHT_BITS[256], what + " bm=256")
        _hold_plain(c, base, M, act, "plain", what)
        variants = [("auto", dict(bits=0)), ("shared", dict(bits=0, shared=True))]
        if bm != 256:
            variants.insert(0, (f"bm={bm}", dict(bits=HEIGHT_BITS[bm])))
        for name, form in variants:
            for got, ref in zip(_plain_forms(c, M, act, what=f"{what} {name}", **form), base):
                _same(got, ref, f"{what} {name}")


# ---- (b) folded forms --------------------------------------------------------------------------------------------------------------
def _rows(M, N, seed, outliers=True, offset=0.0):
    """test_gpu_ln_fold._stream_rows; its outlier channels (17, 401, N - 3) need N > 401: narrower rows get the two that exist"""
    if not outliers or N > 401:
        return _stream_rows(M, N, seed, outliers=outliers, offset=offset)
    x = _stream_rows(M, N, seed, outliers=False, offset=offset).float()
    x[:, 17] += 300.0
    x[:, N - 3] += 1000.0
    return x.half()


@functools.lru_cache(maxsize=2)
def _consumer_case(N, K, act, offset=0.0, rows=MAX_ROWS):
    """raw fp16 stream rows (test_gpu_ln_fold._stream_rows: outlier channels, or a common offset of 30), the folded weight set, the
    row partials rounded once from fp64, the fp64 reference and its bound"""
    c = SimpleNamespace(N=N, K=K, act=act, eps=1e-5)
    c.X = _rows(rows, K, seed=31, outliers=not offset, offset=offset)
    W0, b0 = _rand(N, K, seed=32, scale=K ** -0.5), _rand(N, seed=33, scale=8.0 if offset else 0.1)
    gamma, beta = torch.exp(_rand(K, seed=34) * 0.6), _rand(K, seed=35)
    if not offset:
        gamma[[17, K - 3] + ([401] if K > 401 else [])] = 0.2        # a trained model scales its outlier channels down
    c.W = (W0 * gamma).half()
    c.cs = c.W.float().sum(1)
    c.bias = (b0.double() + W0.double() @ beta.double()).float()
    c.part = _tile_partials(c.X).float()
    x = c.X.double()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + c.eps)
    pre = (x @ c.W.double().t() - mean * c.cs.double()) * rstd
    c.ref = _act(pre + c.bias.double(), act)
    b, _ = _fold_bound(c.X, c.W, c.cs, c.ref, c.eps, act, exact_partials=bool(offset), rstd_term=False, dt=torch.float16)
    dmean, e2, _ = _stat_terms(c.X)
    drstd = 9 * U * e2 / (var + c.eps) + 4 * U
    c.bound = b + ACT_SLOPE * (rstd * dmean * c.cs.double().abs() + pre.abs() * drstd)
    c.round = _hulp16(c.ref)
    c.d = SimpleNamespace(X=_dev(c.X), W=_dev(c.W), cs=_dev(c.cs), bias=_dev(c.bias), part=_dev(c.part))
    return c


def _consumer_launch(c, M, bits, what, shared=False, **kw):
    d = c.d
    return _launch(d.X, d.W, M, c.N, c.K, torch.float16, what, bits=bits, shared=shared, bias=d.bias, act=c.act,
                   ln_part=d.part, colsum=d.cs, ln_eps=c.eps, **kw)[0]


def _height_variants(bm):
    return ([(f"bm={bm}", dict(bits=HEIGHT_BITS[bm]))] if bm != 256 else []) + [("auto", dict(bits=0)), ("shared", dict(bits=0, shared=True))]


@pytest.mark.parametrize("K,N,act,offset", [(256, 512, 0, 0.0), (256, 512, 1, 0.0), (256, 512, 2, 0.0), (768, 768, 0, 0.0),
                                            (768, 768, 1, 0.0), (768, 768, 2, 0.0), (1024, 1024, 0, 0.0), (1024, 1024, 1, 0.0),
                                            (1024, 1024, 2, 0.0), (768, 768, 2, 30.0)])
@pytest.mark.parametrize("bm", sorted(HEIGHT_BITS))
def test_folded_consumer_at_every_tile_height(experiment_build, K, N, act, offset, bm):
    """(b) LNF 1 with one, three and four partial slots in use, every activation, rows with outlier channels and (last case) a
    common offset of 30: every height, the launcher's own and shared = 1 equal the forced 256-row tile; that one against fp64."""
    c = _consumer_case(N, K, act, offset)
    for M in _edge_rows(bm):
        what = f"consumer N={N} K={K} act={act} offset={offset} M={M}"
        base = _consumer_launch(c, M, HEIGHT_BITS[256], what + " bm=256")
        _hold(base, c.ref[:M], c.bound[:M], c.round[:M], "consumer-offset" if offset else "consumer", "f16", what)
        for name, form in _height_variants(bm):
            _same(_consumer_launch(c, M, what=f"{what} {name}", **form), base, f"{what} {name}")


@functools.lru_cache(maxsize=2)
def _producer_case(N, K=256, rows=MAX_ROWS):
    """fp16 operands, raw fp16 residual rows with outlier channels and their partials; fp64 references of the three producer forms"""
    c = SimpleNamespace(N=N, K=K, eps=1e-12)
    c.A, c.W = _rand(rows, K, seed=41).half(), _rand(N, K, seed=42, scale=K ** -0.5).half()
    c.bias = _rand(N, seed=43, scale=0.1)
    c.R = _stream_rows(rows, N, seed=44)
    c.g, c.b = torch.exp(_rand(N, seed=45) * 0.5), _rand(N, seed=46, scale=0.5)
    c.rpart = _tile_partials(c.R).float()
    c.y = c.A.double() @ c.W.double().t() + c.bias.double()
    c.acc = ACT_SLOPE * (_acc_err(c.A, c.W) + U * c.bias.double().abs()) + 8 * U * c.y.abs()      # test_gemm_f16_epilogues' expression
    r = c.R.double()
    mean, var = r.mean(1, keepdim=True), r.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + c.eps)
    z = (r - mean) * rstd * c.g.double()
    c.ln = z + c.b.double()
    dmean, e2, _ = _stat_terms(c.R)
    c.ln_err = c.g.double().abs() * rstd * dmean + z.abs() * (9 * U * e2 / (var + c.eps) + 4 * U + 2 * U) + U * c.ln.abs()
    c.d = SimpleNamespace(A=_dev(c.A), W=_dev(c.W), bias=_dev(c.bias), R=_dev(c.R), g=_dev(c.g), b=_dev(c.b), rpart=_dev(c.rpart))
    return c


def _producer_launch(c, M, mode, bits, what, shared=False):
    d = c.d
    kw = {}
    if mode != "plain":
        kw.update(res=d.R[:M], ldr=c.N)
    if mode == "post_norm":
        kw.update(res_part=d.rpart, res_gamma=d.g, res_beta=d.b, res_eps=c.eps)
    return _launch(d.A, d.W, M, c.N, c.K, torch.float16, what, bits=bits, shared=shared, bias=d.bias, stream_rows=True, want_part=True, **kw)


@pytest.mark.parametrize("N", [768, 1024])
@pytest.mark.parametrize("bm", sorted(HEIGHT_BITS))
def test_folded_producer_at_every_tile_height(experiment_build, N, bm):
    """(b) LNF 2 plain, with the raw residual and with the post-norm residual rebuilt from its partials; three and four partial
    slots written (N = 768: slot 3 stays zero).  Rows and partials of every height, the launcher's own and shared = 1 equal the
    forced 256-row tile's; those are held to fp64, the residual form also bit for bit to fp16(fp32(plain rows) + residual), and
    the partials to fp64 tile sums of the rows as stored."""
    c = _producer_case(N)
    for M in _edge_rows(bm):
        base = {}
        for mode in ("plain", "residual", "post_norm"):
            what = f"producer {mode} N={N} M={M}"
            rows, part = base[mode] = _producer_launch(c, M, mode, HEIGHT_BITS[256], what + " bm=256")
            y = c.y[:M]
            first = c.acc[:M] + _hulp16(y)
            if mode == "plain":
                _hold(rows, y, first, _hulp16(y), "producer", "f16", what)
            else:
                ref = y + (c.R[:M].double() if mode == "residual" else c.ln[:M])
                before = first + (0.0 if mode == "residual" else c.ln_err[:M]) + U * ref.abs()
                last = _hulp16(ref.abs() + before)      # the sum that is rounded may lie in the binade above the reference's
                _hold(rows, ref, before + last, last, "producer+res", "f16", what)
            if mode == "residual":
                _same(rows, (base["plain"][0].float() + c.d.R[:M].float()).half(), what + ": fp16(fp32(y16) + res16)")
            _check_partials(part, rows, "producer", what)
            for name, form in _height_variants(bm):
                got = _producer_launch(c, M, mode, what=f"{what} {name}", **form)
                _same(got[0], rows, f"{what} {name} rows")
                _same(got[1], part, f"{what} {name} partials")


# ---- (c) the prefill's K|V slice ---------------------------------------------------------------------------------------------------
SLICE_FORMS = [("planned", 0), ("ng=4", NG_BITS[4]), ("bm=224", HEIGHT_BITS[224]), ("bm=160 ng=2", HEIGHT_BITS[160] | NG_BITS[2])]


@pytest.mark.parametrize("ops", OPS)
@pytest.mark.parametrize("d", [256, 768])
def test_kv_slice_plain(experiment_build, ops, d):
    """(c) the last prefill layer, unfolded: C = column d of a [M + guard, 3d] buffer, ldc = 3d, N = 2d, W and bias offset by d
    rows / elements.  Equal as raw integers to columns [d, 3d) of the full N = 3d launch, under the planned and forced partitions
    (d = 768: six column tiles, ng = 4 splits them 1 | 2 | 1 | 2) and heights; held to fp64."""
    c = _plain_case(ops, 3 * d, d, rows=700)
    M, D = 700, c.d
    y, acc = _plain_acc(c, 0)
    full = _launch(D.A, D.W, M, 3 * d, d, c.dt, "full", bias=D.bias)[0]
    _hold(full, y[:M], acc[:M] + _hulp(y[:M], c.dt), _hulp(y[:M], c.dt), "slice", ops, f"{ops} d={d} full")
    for name, bits in SLICE_FORMS:
        what = f"{ops} d={d} slice {name}"
        got = _launch(D.A, D.W[d:], M, 2 * d, d, c.dt, what, bits=bits, ldc=3 * d, col0=d, bias=D.bias[d:])[0]
        assert _no_sentinel(got), (what, "a tile was not written")
        _same(got, full[:, d:], what)


@pytest.mark.parametrize("d", [256, 768])
def test_kv_slice_folded(experiment_build, d):
    """(c) the same slice as the folded consumer launches it (fp16 build): colsum offset by d elements as well."""
    c = _consumer_case(3 * d, d, 0)
    M, D = 700, c.d
    full = _consumer_launch(c, M, 0, "full")
    _hold(full, c.ref[:M], c.bound[:M], c.round[:M], "slice", "f16-folded", f"d={d} full")
    for name, bits in SLICE_FORMS:
        what = f"folded d={d} slice {name}"
        got = _launch(D.X, D.W[d:], M, 2 * d, d, torch.float16, what, bits=bits, ldc=3 * d, col0=d, bias=D.bias[d:], act=0,
                      ln_part=D.part, colsum=D.cs[d:], ln_eps=c.eps)[0]
        assert _no_sentinel(got), (what, "a tile was not written")
        _same(got, full[:, d:], what)


# ---- (d) XCD partitions --------------------------------------------------------------------------------------------------------------
# (M, height bits): 600 rows are five 128-row tiles where the launcher picks that height, 650 rows three 224-row tiles: odd counts,
# a multiple of 8 / ng for ng = 8 only
PARTITION_ROWS = [(600, 0), (650, HEIGHT_BITS[224])]


@pytest.mark.parametrize("ops", OPS)
@pytest.mark.parametrize("N", [768, 1024, 1536, 2304])
def test_xcd_partitions_plain(experiment_build, ops, N):
    """(d) ng = 1, 2, 4, 8 forced where ng <= N / 256 (operand-type rows, erf-GELU): each equals the planned partition as raw
    integers, leaves every guard intact and no element of C unwritten; the planned one is held to fp64."""
    c = _plain_case(ops, N, 128, rows=650)
    y, acc = _plain_acc(c, 2)
    for M, hb in PARTITION_ROWS:
        what = f"{ops} N={N} M={M}"
        base = _launch(c.d.A, c.d.W, M, N, c.K, c.dt, what, bits=hb, bias=c.d.bias, act=2)[0]
        _hold(base, y[:M], acc[:M] + _hulp(y[:M], c.dt), _hulp(y[:M], c.dt), "partition", ops, what)
        for ng in (1, 2, 4, 8):
            if ng <= N // 256:
                got = _launch(c.d.A, c.d.W, M, N, c.K, c.dt, f"{what} ng={ng}", bits=hb | NG_BITS[ng], bias=c.d.bias, act=2)[0]
                assert _no_sentinel(got), (what, ng, "a tile was not written")
                _same(got, base, f"{what} ng={ng}")


@pytest.mark.parametrize("N", [768, 1024, 1536, 2304])
def test_xcd_partitions_folded(experiment_build, N):
    """(d) the folded consumer at every N, the folded producer (post-norm) where it exists (N <= 1024), fp16 build"""
    c = _consumer_case(N, 256, 1, rows=650)
    p = _producer_case(N, rows=650) if N <= 1024 else None
    for M, hb in PARTITION_ROWS:
        what = f"folded N={N} M={M}"
        base = _consumer_launch(c, M, hb, what)
        _hold(base, c.ref[:M], c.bound[:M], c.round[:M], "partition", "f16-folded", what)
        pbase = _producer_launch(p, M, "post_norm", hb, what + " producer") if p else None
        for ng in (1, 2, 4, 8):
            if ng <= N // 256:
                got = _consumer_launch(c, M, hb | NG_BITS[ng], f"{what} ng={ng}")
                assert _no_sentinel(got), (what, ng, "a tile was not written")
                _same(got, base, f"{what} consumer ng={ng}")
                if p:
                    rows, part = _producer_launch(p, M, "post_norm", hb | NG_BITS[ng], f"{what} producer ng={ng}")
                    assert _no_sentinel(rows), (what, ng, "a tile was not written")
                    _same(rows, pbase[0], f"{what} producer rows ng={ng}")
                    _same(part, pbase[1], f"{what} producer partials ng={ng}")


# ---- (e) tile-kernel forms the engine runs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ops", OPS)
@pytest.mark.parametrize("in_f32", [False, True])
def test_logits_form(experiment_build, ops, in_f32):
    """(e) the vocabulary GEMM of the f32 mode and of caption scoring: fp32 rows, N = 1002 (N % 8 != 0: the tile kernel whatever M),
    ldc = 1008 with the six padding columns untouched, A starting at a row offset inside a larger buffer; 1, 64 | 65 and 130 rows
    (64 x 64 tiles up to 64 rows, 64 x 128 above), 16-bit and fp32 operands."""
    N, K, off = 1002, 192, 5
    c = _plain_case(ops, N, K, rows=160, in_f32=in_f32)
    y, acc = _plain_acc(c, 0)
    for M in (1, 64, 65, 130):
        what = f"{ops} logits in_f32={in_f32} M={M}"
        out = _launch(c.d.A[off:], c.d.W, M, N, K, torch.float32, what, ldc=1008, bias=c.d.bias, operands=ops)[0]
        _hold(out, y[off:off + M], acc[off:off + M] + U * y[off:off + M].abs(), 0.0, "logits" + ("-f32" if in_f32 else ""), ops, what)


@pytest.mark.parametrize("ops", OPS)
@pytest.mark.parametrize("M", [130, 600])
def test_patch_embedding_form(experiment_build, ops, M):
    """(e) no bias, fp32 rows, 16-bit operands: the tile kernel at 130 rows, gemm_p8_kernel's direct fp32 epilogue without a
    residual at 600 (every height equal to the 256-row tile)."""
    c = _plain_case(ops, 768, 192)
    y, acc = _plain_acc(c, 0, bias=False)
    what = f"{ops} patch embedding M={M}"
    base = _launch(c.d.A, c.d.W, M, 768, 192, torch.float32, what, bits=HEIGHT_BITS[256] if M > 512 else 0)[0]
    _hold(base, y[:M], acc[:M] + U * y[:M].abs(), 0.0, "patch", ops, what)
    if M > 512:
        for bm in (224, 192, 160, 128):
            _same(_launch(c.d.A, c.d.W, M, 768, 192, torch.float32, f"{what} bm={bm}", bits=HEIGHT_BITS[bm])[0], base, f"{what} bm={bm}")
        _same(_launch(c.d.A, c.d.W, M, 768, 192, torch.float32, what + " auto")[0], base, what + " auto")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ops", OPS)
def test_refusals(experiment_build, ops):
    """what the launcher would misread is refused by name and nothing is launched (C keeps its sentinel)"""
    from generativeimage2text_amd import engine as E
    dt = DT[ops]
    A, W = _dev(torch.zeros(600, 256, dtype=dt)), _dev(torch.zeros(256, 256, dtype=dt))
    z = _dev(torch.zeros(600 * 8))
    C = _sentinel((600, 256), dt)
    other = torch.float16 if dt == torch.bfloat16 else torch.bfloat16
    folded = {} if ops == "f16" else {
        "fp16-operand library only": dict(ln_part=z, colsum=z),
        "fp16-operand library only ": dict(part_out=z, stream_rows=True),
    }
    cases = {
        "lda=128 < K": dict(lda=128),
        "ldc=128 < N": dict(ldc=128),
        "ldr=128 < N": dict(res=z, ldr=128),
        "colsum without ln_part": dict(colsum=z),
        "res_gamma / res_beta without res_part": dict(res_gamma=z),
        **folded,
    }
    if ops == "f16":
        cases.update({
            "ln_part without colsum": dict(ln_part=z),
            "consumer .* and producer": dict(ln_part=z, colsum=z, part_out=z),
            "producer writes fp16 stream rows": dict(part_out=z),
            "res_part without res": dict(part_out=z, res_part=z, stream_rows=True),
            "gemm_p8_kernel only": dict(ln_part=z, colsum=z, M=300),
        })
    for name, kw in cases.items():
        M = kw.pop("M", 600)
        with pytest.raises(E.GitmiError, match=name.strip()):
            E.op_gemm_form(A, W, C, M, 256, 256, **kw)
    with pytest.raises(E.GitmiError, match="operands must"):
        E.op_gemm_form(A, W.to(other), C, 600, 256, 256)
    with pytest.raises(E.GitmiError, match="operands must"):
        E.op_gemm_form(A, W, C.to(other), 600, 256, 256)
    torch.cuda.synchronize()
    assert _is_sentinel(C)
