"""GPU: the fp16-operand library (libgitmi_f16.so, the benchmarked build) kernel by kernel against fp64 torch on the same
fp16-rounded inputs.  Every bound is derived below from the arithmetic the kernel does -- fp16 output rounding, fp32
accumulation, operand rounding where weights are folded -- and every test also asserts that its bound is below half the
error that rounding the checked tensor through bf16 would cause, so a stage that rounds through bf16, or toward zero, or
flushes fp16 subnormals, fails here.  The bf16 twins of these tests are in test_gpu_ops.py."""
import math

import pytest
import torch

from test_gpu_ops import GEMM_SHAPES, _act, _attn_ref, _check_tie_order, _check_vocab_lists, _rand

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # fp32 unit roundoff
H16 = 2.0 ** -11        # fp16 relative half-ulp bound (10 stored mantissa bits)
ACT_SLOPE = 1.13        # max |d act / dx| of QuickGELU (1.10) and erf-GELU (1.13): how far an accumulator error moves the output
# the encoder's real row counts, which run the automatic p8 tile height: GIT_BASE 64 x 197 rows, GIT_LARGE 32 x 257,
# VATEX 16 x 6 x 197
ENCODER_SHAPES = [(12608, 768, 768), (12608, 2304, 768), (12608, 3072, 768), (12608, 768, 3072), (8224, 1024, 1024),
                  (8224, 4096, 1024), (8224, 1024, 4096), (18912, 768, 768)]


def _hulp16(x):
    """Half an fp16 ulp at |x|: what rounding x to fp16 (nearest-even) may cost; subnormals below 2^-14 have spacing 2^-24."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 11)


def _hulp(x, dt=torch.float16):
    """Half an ulp of the 16-bit type dt at |x|: fp16 as _hulp16; bf16 (8 significant bits, fp32's exponent range) 2^(e - 8)."""
    if dt == torch.float16:
        return _hulp16(x)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 8)


def _check16(out, ref, bound, what=""):
    """|out - ref| <= bound element by element, and the bound is tight enough to tell fp16 from bf16: its largest value is
    below half the error rounding ref through bf16 causes at ref's largest magnitude (half a bf16 ulp there, 2^(e - 8))."""
    ref = ref.double()
    bf = 2.0 ** (math.floor(math.log2(ref.abs().max().item())) - 8)
    assert bound.max().item() < 0.5 * bf, (what, "bound too loose to tell fp16 from bf16", bound.max().item(), bf)
    err = (out.double().to(ref.device) - ref).abs()
    bad = err > bound
    if bad.any():
        i = (err - bound).argmax()
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound; worst: err {err.flatten()[i].item():.3e} "
                             f"bound {bound.flatten()[i].item():.3e} ref {ref.flatten()[i].item():.6g} "
                             f"got {out.flatten()[i].item():.6g}")


def _acc_err(A, W, exact_partials=False):
    """Bound of the fp32 accumulation error of A W^T on the matrix cores (A, W hold exact fp16 values, so every product is
    exact in fp32).  An MFMA 16x16x32 adds 32 products to the accumulator; bound each of the K/32 updates by one rounding of
    the running sum, plus 5 roundings inside the instruction of its chunk's sum of |a w| (a 32-term tree is 5 deep):
        err <= u (sum_t |c_t| + 5 sum_k |a_k w_k|),
    c_t the running sum after chunk t.  exact_partials=False bounds |c_t| by S = sum_k |a_k w_k|: u (K/32 + 5) S; True uses
    the fp64 running sums themselves (rows with a large common mean: the sums stay far below S)."""
    A, W = A.double(), W.double()
    S = A.abs() @ W.abs().t()
    K = A.shape[1]
    if not exact_partials:
        return U * (K / 32 + 5) * S
    M, N = A.shape[0], W.shape[0]
    chunks = torch.einsum("mtk,ntk->mnt", A.reshape(M, K // 32, 32), W.reshape(N, K // 32, 32))
    return U * (chunks.cumsum(-1).abs().sum(-1) + 5 * S)


def _runs_p8(M, N, K):
    """kernels_gemm.hip gemm_uses_p8 for 16-bit operands: more than 512 rows, N % 256 == 0, K >= 128.  Its 16-bit epilogue
    stages act(acc + bias) through LDS in the output type and adds a residual after: two roundings, where the register-staged
    tile kernel rounds once."""
    return M > 512 and N % 256 == 0 and K >= 128 and K % 64 == 0


# ---- GEMM: the three epilogues ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES + ENCODER_SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_f16_epilogues(M, N, K, act):
    """fp32 rows (+ fp32 residual), fp16 operand rows (with and without fp32 residual) and fp16 stream rows (with and without
    an fp16 residual) of one fp16 GEMM.  Bound: the accumulation error (_acc_err) moved by the activation's slope, plus 8 u
    |pre| for the activation's fp32 evaluation, plus u |ref| for the residual add and the output rounding: fp32 rows add
    nothing more, fp16 rows add half an fp16 ulp.  In the p8 kernel a 16-bit epilogue with a residual is checked bit for bit
    as fp16(fp32(y16) + residual), y16 its own output without the residual (checked against fp64 here)."""
    from generativeimage2text_amd import engine as E
    dev = torch.device("cuda")
    A = _rand(M, K, seed=1).half().to(dev)
    W = _rand(N, K, seed=2, scale=K ** -0.5).half().to(dev)
    bias = _rand(N, seed=3).to(dev)
    res = _rand(M, N, seed=4).to(dev)
    res16 = res.half()
    pre = A.double() @ W.double().t() + bias.double()
    y = _act(pre, act)
    acc = ACT_SLOPE * (_acc_err(A, W) + U * bias.double().abs()) + 8 * U * pre.abs()
    del pre
    ref = y + res.double()
    _check16(E.op_gemm(A, W, bias, res, act, torch.float32), ref, acc + U * ref.abs(), "fp32 + residual")
    y16 = E.op_gemm(A, W, bias, None, act, torch.float16)
    _check16(y16, y, acc + _hulp16(y), "fp16")
    out = E.op_gemm(A, W, bias, res, act, torch.float16)
    if _runs_p8(M, N, K):
        assert torch.equal(out, (y16.float() + res).half()), "fp16 + residual"
    else:
        _check16(out, ref, acc + U * ref.abs() + _hulp16(ref), "fp16 + residual")
    st = E.op_gemm(A, W, bias, None, act, stream_rows=True)
    _check16(st, y, acc + _hulp16(y), "stream")
    ref = y + res16.double()
    out = E.op_gemm(A, W, bias, res16, act, stream_rows=True)
    if _runs_p8(M, N, K):
        assert torch.equal(out, (st.float() + res16.float()).half()), "stream + residual"
    else:
        _check16(out, ref, acc + U * ref.abs() + _hulp16(ref), "stream + residual")


def _integer_gemm(M, N, K, seed):
    """Integer operands exact in bf16 and fp16 (|v| <= 256) whose products A W^T spread over +-2048 ... 70 000: every fp32
    partial sum is an exact integer below 2^24, so the only rounding of the result is the output conversion."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float()
    A[:, 0] = torch.randint(1, 257, (M,), generator=g).float()
    W[:, 0] = torch.randint(-256, 257, (N,), generator=g).float()
    A[:2, 1:] = 0                                   # rows 0 and 1: exactly 256 / 255 times W[:, 0]
    A[0, 0], A[1, 0] = 256, 255
    W[:4, 0] = torch.tensor([256.0, -256.0, 255.0, -255.0])     # +-65536 -> +-inf, +-65280 finite
    return A, W


@pytest.mark.parametrize("operands", ["f16", "bf16"])
@pytest.mark.parametrize("M,N,K", [(200, 320, 128), (1000, 512, 128)])      # register-staged tile kernel | p8 kernel
@pytest.mark.parametrize("with_res", [False, True])
def test_gemm_16bit_output_rounding_is_exact(operands, M, N, K, with_res):
    """Both 16-bit epilogues round the exact fp32 result once, to nearest even: the output is exactly torch's conversion of
    the fp64 result -- ties to even (odd integers above 2048 in fp16) and +-inf beyond 65 520 included.  The bf16 library's
    fp16 stream rows are checked the same way."""
    from generativeimage2text_amd import engine as E
    dt = torch.float16 if operands == "f16" else torch.bfloat16
    A, W = _integer_gemm(M, N, K, seed=M + N)
    g = torch.Generator().manual_seed(5)
    bias = torch.randint(-1000, 1001, (N,), generator=g).float() if with_res else None
    res = torch.randint(-2048, 2049, (M, N), generator=g).float() if with_res else None
    if with_res:                                    # keep the +-65536 / +-65280 of rows 0, 1 and columns 0..3
        bias[:4] = 0
        res[:2] = 0
    ref = A.double() @ W.double().t() + (bias.double() if with_res else 0) + (res.double() if with_res else 0)
    assert ref.abs().max().item() < 2 ** 24 and torch.equal(A.to(dt).float(), A) and torch.equal(W.to(dt).float(), W)
    ties = (ref.abs() > 2048) & (ref.abs() < 4096) & (ref.remainder(2) == 1)
    assert ties.sum().item() > 100 and (ref.abs() > 65520).sum().item() >= 2 and ((ref.abs() > 4096) & (ref.abs() < 65504)).any()
    Ad, Wd = A.to(dt).cuda(), W.to(dt).cuda()
    bd = bias.cuda() if with_res else None
    want, want_st = ref.to(dt), ref.half()
    if with_res and _runs_p8(M, N, K):              # the residual is added to the rounded act(acc + bias): exact in fp32
        y = A.double() @ W.double().t() + bias.double()
        want, want_st = (y.to(dt).double() + res.double()).to(dt), (y.half().double() + res.double()).half()
    out = E.op_gemm(Ad, Wd, bd, res.cuda() if with_res else None, 0, dt).cpu()
    assert torch.equal(out, want), (out.double() - want.double()).abs().nan_to_num(1e9).max().item()
    st = E.op_gemm(Ad, Wd, bd, res.half().cuda() if with_res else None, 0, stream_rows=True).cpu()
    assert st.dtype == torch.float16 and torch.equal(st, want_st), (st.double() - want_st.double()).abs().nan_to_num(1e9).max().item()


@pytest.mark.parametrize("M,N,K", [(200, 256, 256), (1000, 512, 256)])
def test_f16_subnormal_operands_are_not_flushed(M, N, K):
    """A ~ 1e-5 (almost all fp16 subnormals: below 2^-14 = 6.1e-5) against W ~ 1e3 through the GEMM (tile and p8 kernels)
    and the decode-chain GEMM: products ~ 1e-2, sums ~ 0.1; a flush-to-zero of either operand path gives zeros.  Bounds as in
    test_gemm_f16_epilogues (subnormal operands are exact values, their products exact in fp32)."""
    from generativeimage2text_amd import engine as E
    A = _rand(M, K, seed=61, scale=1e-5).half()
    W = _rand(N, K, seed=62, scale=1e3).half()
    assert (A.abs() < 2.0 ** -14).float().mean().item() > 0.99
    ref = A.double() @ W.double().t()
    acc = _acc_err(A, W)
    Ad, Wd = A.cuda(), W.cuda()
    _check16(E.op_gemm(Ad, Wd, None, None, 0, torch.float32).cpu(), ref, acc + U * ref.abs(), "gemm fp32")
    _check16(E.op_gemm(Ad, Wd, None, None, 0, torch.float16).cpu(), ref, acc + _hulp16(ref), "gemm fp16")
    _check16(E.op_dgemm(Ad[:64].contiguous(), Wd, torch.zeros(N).cuda()).cpu(), ref[:64], acc[:64] + _hulp16(ref[:64]), "dgemm")


# ---- LayerNorm -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,D", [(5, 768), (1000, 1024), (33, 128), (7, 192), (12608, 768), (8224, 1024)])
@pytest.mark.parametrize("eps", [1e-5, 1e-12])
def test_layernorm_f16_output(rows, D, eps):
    """fp16 rows of LayerNorm(fp32 x): the fp32 computation's bound of test_layernorm (2e-5) plus half an fp16 ulp."""
    from generativeimage2text_amd import engine as E
    x = _rand(rows, D, seed=8, scale=3.0) + 0.5
    g, b = 1 + _rand(D, seed=9, scale=0.1), _rand(D, seed=10, scale=0.1)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), g.double(), b.double(), eps)
    out = E.op_layernorm(x.cuda(), g.cuda(), b.cuda(), eps, torch.float16)
    assert out.dtype == torch.float16
    _check16(out.cpu(), ref, 2e-5 + _hulp16(ref))


# ---- attention -------------------------------------------------------------------------------------------------------
def _attn_bound(q, k, v, ref):
    """Bound of a 16-bit softmax attention o = sum_j p_j v_j / l, p_j = exp(s_j - max), s = q k^T / 8, on exact fp16 q, k, v
    ([..., Nq, 64], [..., Nk, 64], [..., Nk, 64]; ref [..., Nq, 64] fp64).  The kernels compute s and exp in fp32, feed
    p rounded to fp16 to the P V product (relative to a running max, rescaled in fp32 after) and divide by the fp32 sum l:
      - scores: two chained MFMAs over 64 dims + the fp32 scale/exp argument: |ds_j| <= 4 u |q||k|_j / 8 + 4 u |s_j| + 4 u,
        a relative error of p_j that moves o by at most sum_j p_j ds_j (|v_j| + |o|) / l;
      - fp16 P: the key at the running max is exp(0) = 1, exact.  A normal p_j (>= 2^-14) rounds by at most 2^-11 p_j;
        these errors are independent, zero-mean, of variance <= (2^-11 p_j)^2 / 3: their sum stays within 6 sigma =
        6 / sqrt(3) 2^-11 sqrt(sum_j p_j^2 v_j^2) / l.  A subnormal p_j rounds by at most 2^-25: sum 2^-25 |v_j| / l;
      - fp32 sums over Nk keys of p v and p (chains of Nk / 32 + 8 roundings): (Nk / 32 + 8) u (sum_j p_j |v_j| / l + |o|);
      - the output: half an fp16 ulp."""
    q, k, v = q.double(), k.double(), v.double()
    s = q @ k.transpose(-1, -2) / 8.0
    p = torch.exp(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    ds = 4 * U * (q.abs() @ k.abs().transpose(-1, -2)) / 8.0 + 4 * U * s.abs() + 4 * U
    av = v.abs()
    pv_abs = (p @ av) / l
    b = ((p * ds) @ av) / l + ref.abs() * (p * ds).sum(-1, keepdim=True) / l
    normal = (p >= 2.0 ** -14) & (p < 1.0)
    pn = torch.where(normal, p, torch.zeros_like(p))
    b = b + 6 / math.sqrt(3) * H16 * torch.sqrt((pn * pn) @ (v * v)) / l
    b = b + 2.0 ** -25 * ((p < 2.0 ** -14).double() @ av) / l
    b = b + (k.shape[-2] / 32 + 8) * U * (pv_abs + ref.abs())
    return b + _hulp16(ref)


def _full_attn_bound(qkv, B, N, H, ref):
    q, k, v = qkv.double().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    r = ref.reshape(B, N, H, 64).permute(0, 2, 1, 3)
    return _attn_bound(q, k, v, r).permute(0, 2, 1, 3).reshape(B * N, H * 64)


def _flat_spiked_qkv(N, seed):
    """One head: every query close to q0, one key 11 above the nearly flat rest in score: 1181 probabilities of ~exp(-11)
    = 1.7e-5 -- fp16 subnormals -- that carry 2 % of the mass."""
    g = torch.Generator().manual_seed(seed)
    q0 = torch.randn(64, generator=g)
    qkv = torch.zeros(N, 192)
    qkv[:, :64] = q0 + 0.05 * torch.randn(N, 64, generator=g)
    qkv[:, 64:128] = 0.05 * torch.randn(N, 64, generator=g)
    qkv[N // 3, 64:128] = 88.0 * q0 / q0.dot(q0)
    qkv[:, 128:] = 1.5 * torch.randn(N, 64, generator=g)
    return qkv


@pytest.mark.parametrize("B,N,H", [(2, 17, 2), (3, 197, 12), (1, 257, 16), (2, 300, 3), (1, 1182, 2), (1, 64, 1),
                                   (2, 193, 3), (2, 208, 2), (2, 272, 2), (1, 209, 1), ("rescale", 200, 1), ("flat", 1182, 1)])
def test_attention_full_f16(B, N, H):
    """impl 1 (by geometry: single-pass kernel for 193..208 / 257..272 keys, else flash) and impl 2 (64-key flash) on fp16
    qkv: test_attention_full's shapes, its rescale-branch case and 1182 nearly flat keys (most probabilities subnormal)."""
    from generativeimage2text_amd import engine as E
    if B == "rescale":                   # test_attention_softmax_rescale_branch: a spiked key in a later tile
        B, qkv = 1, _rand(N, 192, seed=12, scale=0.5)
        qkv[150, 64:128] = qkv[3, 0:64] * 40.0
    elif B == "flat":
        B, qkv = 1, _flat_spiked_qkv(N, seed=13)
    else:
        qkv = _rand(B * N, 3 * H * 64, seed=11, scale=1.5)
    qh = qkv.half()
    ref = _attn_ref(qh.float(), B, N, H)
    bound = _full_attn_bound(qh, B, N, H, ref)
    for impl in (1, 2):
        out = E.op_attention(qh.cuda(), B, N, H, impl=impl)
        assert out.dtype == torch.float16
        _check16(out.cpu(), ref, bound, f"impl {impl}")


def _decode_ref(qkv, ik, iv, tk, tv, src, B, H, pos, beams, img_of=None, ntok=None):
    """fp64 decode attention, vectorised: row r = (sentence b, beam) attends to the keys of image img_of[b] (None: image b),
    its text history through kv_src (positions < pos) and its own new key; ntok (per IMAGE): image keys past the count are masked.
    -> (q, K, V, out) as [R, H, keys, 64] / [R, H, 1, 64]; K / V come back whole, the mask is applied to the scores only."""
    R, d = B * beams, H * 64
    q = qkv[:, :d].double().reshape(R, H, 1, 64)
    img = torch.arange(R) // beams
    if img_of is not None:
        img = torch.as_tensor(img_of).long()[img]
    rows = src[:, :pos].long()
    hk = tk.double()[rows, torch.arange(pos)].reshape(R, pos, H, 64).permute(0, 2, 1, 3)
    hv = tv.double()[rows, torch.arange(pos)].reshape(R, pos, H, 64).permute(0, 2, 1, 3)
    K = torch.cat([ik.double()[img], hk, qkv[:, d:2 * d].double().reshape(R, H, 1, 64)], 2)
    V = torch.cat([iv.double()[img], hv, qkv[:, 2 * d:].double().reshape(R, H, 1, 64)], 2)
    s = q @ K.transpose(-1, -2) / 8.0
    if ntok is not None:
        N_img = ik.shape[2]
        pad = torch.arange(N_img)[None, :] >= torch.as_tensor(ntok).long()[img][:, None]                  # [R, N_img]
        s[..., :N_img] = s[..., :N_img].masked_fill(pad[:, None, None, :], float("-inf"))
    o = torch.softmax(s, -1) @ V
    return q, K, V, o


@pytest.mark.parametrize("B,H,N_img,pos,beams", [(2, 2, 17, 0, 1), (3, 12, 197, 5, 1), (2, 12, 197, 7, 4), (1, 2, 300, 3, 3),
                                                  (1, 1, 1182, 11, 2), (2, 2, 40, 60, 4),
                                                  # packed one-wave forms with an absent pair in the last workgroup:
                                                  # 193 pairs -> 2 per workgroup, 387 pairs -> 4 per workgroup
                                                  (193, 1, 40, 2, 1), (129, 3, 40, 2, 2)])
def test_attention_decode_f16(B, H, N_img, pos, beams):
    """test_attention_decode's cases on fp16: the default, one-wave-per-pair and streaming (1, 2, 96 workgroups) forms against
    fp64 (_attn_bound; the text keys run in fp32, which the bound covers), and the streaming forms bitwise equal to the
    one-wave form."""
    from generativeimage2text_amd import engine as E
    d, R, T = H * 64, B * beams, max(pos + 1, 8) + 3
    g = torch.Generator().manual_seed(100 + N_img + pos)
    qkv = (torch.randn(R, 3 * d, generator=g) * 1.2).half()
    ik = torch.randn(B, H, N_img, 64, generator=g).half()
    iv = torch.randn(B, H, N_img, 64, generator=g).half()
    tk = torch.randn(R, T, d, generator=g).half()
    tv = torch.randn(R, T, d, generator=g).half()
    src = torch.stack([torch.randint(b * beams, (b + 1) * beams, (T,), generator=g) for b in range(B) for _ in range(beams)]).int()
    q, K, V, o = _decode_ref(qkv, ik, iv, tk, tv, src, B, H, pos, beams)
    ref = o.reshape(R, d)
    bound = _attn_bound(q, K, V, o).reshape(R, d)

    def run(form):
        out = E.op_attn_decode(qkv.cuda(), ik.cuda(), iv.cuda(), tk.cuda().clone(), tv.cuda().clone(), src.cuda(), B, H, N_img, T,
                               pos, beams, dbg=form)
        assert out.dtype == torch.float16
        return out.cpu()
    _check16(run(0), ref, bound, "default")
    one = run(1 << 16)
    _check16(one, ref, bound, "one wave")
    for wgs in (1, 2, 96):
        st = run(wgs << 18)
        assert torch.equal(st, one), (wgs, (st.double() - one.double()).abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,H,N", [(2, 3, 50), (1, 2, 64), (3, 1, 17)])
def test_kv_repack_moves_each_block(dtype, B, H, N):
    """kv_repack: per (image, head), kf / vt hold exactly that block's K / V elements plus zeros up to 32 keys.  Every input
    element is a distinct raw 16-bit code (no zero, no NaN in either encoding), so a block that takes another's elements, or a
    repack that converts values instead of moving them, changes the multiset."""
    from generativeimage2text_amd import engine as E
    Np = (N + 31) // 32 * 32
    n = B * H * N * 64
    codes = torch.arange(1, 0x7c00, dtype=torch.int32)                      # positive finite in fp16, and in bf16 below 0x7f80
    codes = torch.cat([codes, codes + 0x8000])                               # and their negatives
    perm = codes[torch.randperm(codes.numel(), generator=torch.Generator().manual_seed(B * 100 + H * 10 + N))[:2 * n]]
    raw = perm.to(torch.int16)
    ik = raw[:n].view(dtype).reshape(B, H, N, 64)
    iv = raw[n:].view(dtype).reshape(B, H, N, 64)
    kf, vt = E.kv_repack(ik.cuda(), iv.cuda())
    assert kf.dtype == dtype and vt.dtype == dtype and kf.numel() == B * H * Np * 64
    kf = kf.cpu().view(torch.int16).reshape(B, H, Np * 64)
    vt = vt.cpu().view(torch.int16).reshape(B, H, Np * 64)
    pad = torch.zeros((Np - N) * 64, dtype=torch.int16)
    for b in range(B):
        for h in range(H):
            for got, src in ((kf[b, h], ik[b, h]), (vt[b, h], iv[b, h])):
                want = torch.cat([src.reshape(-1).view(torch.int16), pad])
                assert torch.equal(torch.sort(got).values, torch.sort(want).values), (b, h)


# ---- decode-step GEMM chain (kernels_dgemm.hip) -------------------------------------------------------------------
def _fold16(W, bias, gamma, beta):
    """gitmi_finalize_weights of the fp16 library for a GEMM behind a LayerNorm: W' = fp16(W . gamma) (engine_weights.hip's
    bf16_round rounds to the build's operand type), beta W^T + b, colsum(W')."""
    Wf = (W * gamma[None, :]).half()
    return Wf, (bias.double() + W.double() @ beta.double()).float(), Wf.double().sum(1).float()


def _fold_bound(x, Wf, cs, exact, eps, act, exact_partials=False, rstd_term=True, dt=torch.float16):
    """Bound of the folded-LayerNorm epilogue act(rstd (A W'^T - mean colsum) + b') against fp64 on the same fp16 A = fp16(x)
    (dt: the 16-bit operand and output type, fp16 unless given),
    W' and fp32 colsum, mean / var of the raw fp32 rows:
      - A W'^T in fp32: _acc_err; mean colsum and the subtraction: 2 u |mean colsum| + u |A W'^T - mean colsum|;
      - the statistics: fp32 16-column strip sums (16 roundings) added over K/16 strips, so sum and sum of squares carry
        (16 + K/16) u relative error; var = E[x^2] - mean^2 then errs by (2 (16 + K/16) + 4) u E[x^2], and rstd by half
        that relative to var + eps, plus 4 u for the reciprocal square root;
    all moved by the activation's slope, plus 8 u |pre| for the activation and half an fp16 ulp for the output.
    rstd_term=False leaves out the rstd error (returned second: the bound of its relative size per row)."""
    K = x.shape[1]
    x64 = x.double()
    mean, var = x64.mean(1, keepdim=True), x64.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    A = x.to(dt)
    raw = A.double() @ Wf.double().t()
    mc = mean * cs.double()[None, :]
    e_acc = _acc_err(A, Wf, exact_partials) + 2 * U * mc.abs() + U * (raw - mc).abs()
    drstd = 0.5 * (2 * (16 + K / 16) + 4) * U * (x64 * x64).mean(1, keepdim=True) / (var + eps) + 4 * U
    pre = (raw - mc) * rstd
    b = ACT_SLOPE * (rstd * e_acc + (pre.abs() * drstd if rstd_term else 0.0)) + 8 * U * exact.abs() + _hulp(exact, dt)
    return b if rstd_term else (b, drstd)


def _gelu_slope(z):
    return 0.5 * (1.0 + torch.erf(z / 2 ** 0.5)) + z * torch.exp(-0.5 * z * z) / (2 * math.pi) ** 0.5


@pytest.mark.parametrize("M,N,K", [(64, 2304, 768), (64, 3072, 768), (256, 3072, 768), (5, 130, 128), (33, 1002, 96),
                                   (17, 512, 128), (100, 2304, 768)])
@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("fold", [False, True])
def test_dgemm_qkv_ffn1_form_f16(M, N, K, act, fold):
    """test_dgemm_qkv_ffn1_form on fp16 operands: plain and with the LayerNorm folded (fp16 weight folding).  Bitwise
    invariances as in bf16: strips_per_wg, and the row-walking kernel against the one-block kernel."""
    _dgemm_qkv_case(M, N, K, act, fold)


@pytest.mark.parametrize("M,N", [(64, 2304), (256, 3072), (100, 2304)])
@pytest.mark.parametrize("act", [0, 2])
def test_dgemm_folded_rows_with_a_mean_many_times_their_spread_f16(M, N, act):
    """The folded form on rows whose |mean| / sigma is 10..60 (the regime test_op_consumer_gemm_rows_with_a_mean_many_times_
    their_spread pins for the encoder fold), at the decoder's width K = 768."""
    _dgemm_qkv_case(M, N, 768, act, "mean")


def _dgemm_qkv_case(M, N, K, act, fold):
    from generativeimage2text_amd import engine as E
    W = _rand(N, K, seed=22, scale=K ** -0.5)
    bias = _rand(N, seed=23)
    if not fold:
        A = _rand(M, K, seed=21).half()
        W16 = W.half()
        pre = A.double() @ W16.double().t() + bias.double()
        ref = _act(pre, act)
        out = E.op_dgemm(A.cuda(), W16.cuda(), bias.cuda(), act=act)
        assert out.dtype == torch.float16
        _check16(out.cpu(), ref, ACT_SLOPE * (_acc_err(A, W16) + U * bias.double().abs()) + 8 * U * pre.abs() + _hulp16(ref))
        if N % 32 == 0:
            assert torch.equal(E.op_dgemm(A.cuda(), W16.cuda(), bias.cuda(), act=act, frag_out=True), out)
        if 32 < M <= 64 and N >= 1536:
            for nst in (2, 4, 6):
                assert torch.equal(E.op_dgemm(A.cuda(), W16.cuda(), bias.cuda(), act=act, strips_per_wg=nst), out)
        if M > 64:
            hi = min(M, 128)
            assert torch.equal(E.op_dgemm(A[64:hi].contiguous().cuda(), W16.cuda(), bias.cuda(), act=act), out[64:hi])
        return
    if K % 16:
        pytest.skip("strip partials need K % 16 == 0")
    x = _rand(M, K, seed=21, scale=1.3) + 0.2
    if fold == "mean":                   # row m: mean 10..60 sigma, alternating sign
        sigma = 0.05
        ratio = torch.linspace(10, 60, M)[:, None] * torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)[:, None]
        x = sigma * (_rand(M, K, seed=26) + ratio)
    gamma, beta = 1 + _rand(K, seed=24, scale=0.1), _rand(K, seed=25, scale=0.1)
    Wf, bf, cs = _fold16(W, bias, gamma, beta)
    stats = E.strip_stats(x.cuda())
    out_dev = E.op_dgemm(x.half().cuda(), Wf.cuda(), bf.cuda(), cs.cuda(), stats, 1e-12, act)
    assert out_dev.dtype == torch.float16
    if 32 < M <= 64 and N >= 1536:
        for nst in (2, 4, 6):
            assert torch.equal(E.op_dgemm(x.half().cuda(), Wf.cuda(), bf.cuda(), cs.cuda(), stats, 1e-12, act,
                                          strips_per_wg=nst), out_dev)
    if M > 64:
        hi = min(M, 128)
        sub = E.op_dgemm(x[64:hi].half().contiguous().cuda(), Wf.cuda(), bf.cuda(), cs.cuda(), stats[:, 64:hi].contiguous(), 1e-12, act)
        assert torch.equal(sub, out_dev[64:hi])
    mean, var = x.double().mean(1, keepdim=True), x.double().var(1, unbiased=False, keepdim=True)
    pre = (x.half().double() @ Wf.double().t() - mean * cs.double()) / torch.sqrt(var + 1e-12)
    exact = _act(pre + bf.double(), act)
    if fold is True:
        _check16(out_dev.cpu(), exact, _fold_bound(x, Wf, cs, exact, 1e-12, act))
        return
    # |mean| / sigma up to 60: the one-pass variance in fp32 loses up to ~3600x its relative precision -- an error of rstd, one
    # factor (1 + d_m) per row that no fp16 / bf16 distinction survives.  Fit d_m per row (least squares on the first-order
    # change g = act'(z) pre), bound it by the derivation of _fold_bound, and hold what is left to the bound without it (plus
    # the second-order term d^2 pre^2 max|act''| / 2, max|GELU''| = 0.8).
    # The fp32 mean errs too (by (16 + K/16) u mean|x|): a second per-row term, along rstd colsum.  Fit both per row.
    bound, drstd = _fold_bound(x, Wf, cs, exact, 1e-12, act, exact_partials=True, rstd_term=False)
    slope = _gelu_slope(pre + bf.double()) if act == 2 else torch.ones_like(pre)
    rstd = 1.0 / torch.sqrt(var + 1e-12)
    G = torch.stack([slope * pre, -slope * cs.double()[None, :] * rstd], -1)          # [M, N, 2]
    r = out_dev.cpu().double() - exact
    d = torch.linalg.solve(G.transpose(1, 2) @ G, (G.transpose(1, 2) @ r[..., None]))[..., 0]      # [M, 2]
    dmean = (16 + K / 16) * U * x.double().abs().mean(1)
    assert (d[:, 0].abs() <= drstd[:, 0]).all() and (d[:, 1].abs() <= dmean).all(), (d, drstd[:, 0], dmean)
    fit = (G * d[:, None, :]).sum(-1)
    _check16(out_dev.cpu(), exact + fit, bound + 0.4 * fit ** 2)


@pytest.mark.parametrize("M,N,K", [(64, 768, 768), (64, 768, 3072), (256, 768, 3072), (7, 128, 512), (33, 128, 128), (100, 768, 768)])
@pytest.mark.parametrize("ln_res", [False, True])
def test_dgemm_residual_stats_form_f16(M, N, K, ln_res):
    """test_dgemm_residual_stats_form on fp16 operands: x fp32 = A W^T + bias + r (r = the fp32 rows or their LayerNorm
    rebuilt from strip partials), its fp16 copy, the strip partials of x; bitwise reproducible and batch-independent.
    Bounds: x -- _acc_err + u (|bias| + |x|) for the adds, and for the post-norm residual the LayerNorm rebuilt in fp32
    (test_layernorm's 2e-5); the fp16 copy -- that plus half an fp16 ulp."""
    from generativeimage2text_amd import engine as E
    A = _rand(M, K, seed=31).half()
    W = _rand(N, K, seed=32, scale=K ** -0.5).half()
    bias, xprev = _rand(N, seed=33), _rand(M, N, seed=34, scale=1.2) + 0.1
    g, b = 1 + _rand(N, seed=35, scale=0.1), _rand(N, seed=36, scale=0.1)
    res = torch.nn.functional.layer_norm(xprev.double(), (N,), g.double(), b.double(), 1e-12) if ln_res else xprev.double()
    ref = A.double() @ W.double().t() + bias.double() + res
    args = (A.cuda(), W.cuda(), bias.cuda(), xprev.cuda())
    kw = dict(res_stats=E.strip_stats(xprev.cuda()), res_gamma=g.cuda(), res_beta=b.cuda()) if ln_res else {}
    x, xb, st = E.op_dgemm_res(*args, **kw)
    assert xb.dtype == torch.float16
    bx = _acc_err(A, W) + 2 * U * (bias.double().abs() + ref.abs()) + (2e-5 if ln_res else 0.0)
    _check16(x.cpu(), ref, bx, "x")
    _check16(xb.cpu(), ref, bx + _hulp16(ref), "fp16 copy")
    want = E.strip_stats(x).cpu()
    assert (st.cpu() - want).abs().max().item() < 1e-3 * max(1.0, want.abs().max().item())
    x2, xb2, st2 = E.op_dgemm_res(*args, **kw)
    assert torch.equal(x, x2) and torch.equal(xb, xb2) and torch.equal(st, st2)
    x3, _, _ = E.op_dgemm_res(A[:3].contiguous().cuda(), W.cuda(), bias.cuda(), xprev[:3].contiguous().cuda(),
                              **({k: (v[:, :3].contiguous() if k == "res_stats" else v) for k, v in kw.items()}))
    assert torch.equal(x3, x[:3])


# ---- vocabulary head ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V,K,mtop", [(64, 30522, 768, 1), (64, 30522, 768, 8), (256, 30522, 768, 8), (130, 30522, 768, 4),
                                        (5, 1000, 128, 4), (33, 1000, 128, 2), (16, 5003, 256, 16), (40, 999, 96, 8),
                                        (200, 1000, 128, 4), (7, 1000, 768, 16), (100, 2000, 768, 2)])
@pytest.mark.parametrize("fold", [False, True])
def test_vocab_head_fused_topm_f16(M, V, K, mtop, fold):
    """test_vocab_head_fused_topm on fp16 operands: the fp32 logits against fp64 (plain: _acc_err + u |bias| + u |logit|;
    folded: _fold_bound without the output rounding, the logits are fp32), then the same list checks (_check_vocab_lists):
    top-M and log-sum-exp of those logits, and every max_wgs of the decode-loop kernels bit for bit."""
    from generativeimage2text_amd import engine as E
    cols = 128
    W = _rand(V, K, seed=41, scale=K ** -0.5 * 2.0)
    bias = _rand(V, seed=42, scale=0.5)
    x = _rand(M, K, seed=43, scale=1.1) + 0.15
    sup = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(44), dtype=torch.int32)
    if fold:
        if K % 16:
            pytest.skip("strip partials need K % 16 == 0")
        gamma, beta = 1 + _rand(K, seed=45, scale=0.1), _rand(K, seed=46, scale=0.1)
        Wf, bf, cs = _fold16(W, bias, gamma, beta)
        mean, var = x.double().mean(1, keepdim=True), x.double().var(1, unbiased=False, keepdim=True)
        ref = (x.half().double() @ Wf.double().t() - mean * cs.double()) / torch.sqrt(var + 1e-12) + bf.double()
        bound = _fold_bound(x, Wf, cs, ref, 1e-12, 0) - _hulp16(ref) + U * ref.abs()

        def head(**kw):
            return E.op_vocab_topm(x.half().cuda(), Wf.cuda(), bf.cuda(), mtop, cols, cs.cuda(), E.strip_stats(x.cuda()), 1e-12,
                                   sup.cuda(), **kw)
    else:
        W16 = W.half()
        ref = x.half().double() @ W16.double().t() + bias.double()
        bound = _acc_err(x.half(), W16) + U * bias.double().abs() + U * ref.abs()

        def head(**kw):
            return E.op_vocab_topm(x.half().cuda(), W16.cuda(), bias.cuda(), mtop, cols, suppress_tok=sup.cuda(), **kw)
    pv, pi, pl, lg = head(want_logits=True)
    lg = lg.cpu()
    _check16(lg, ref, bound, "logits")
    _check_vocab_lists(head, lg, pv, pi, pl, sup, mtop, cols)


@pytest.mark.parametrize("M", [8, 70, 256])
@pytest.mark.parametrize("mtop", [2, 8])
def test_vocab_head_topm_tie_order_f16(M, mtop):
    """test_vocab_head_topm_tie_order on fp16 operands (the integer operands are exact in fp16 too)."""
    _check_tie_order(M, mtop, torch.float16)


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operands", ["bf16", "f16"])
def test_op_hooks_refuse_the_other_builds_16bit_dtype(operands):
    """gitmi_op_gemm (in and out dtype), gitmi_op_attention, gitmi_op_attn_decode and gitmi_op_layernorm (its output) refuse the
    16-bit code of the other library with a named error, before touching any buffer; the Python wrappers of the hooks without a
    dtype argument refuse mixed 16-bit tensors."""
    from generativeimage2text_amd import engine as E
    lib = E.load_library(operands)
    other = E.DTYPE_F16 if operands == "bf16" else E.DTYPE_BF16
    own = E.DTYPE_BF16 if operands == "bf16" else E.DTYPE_F16
    buf = torch.zeros(1 << 16, device="cuda")
    p, s = buf.data_ptr(), E._stream()
    calls = {
        "op_gemm: in_dtype": lambda: lib.gitmi_op_gemm(p, p, None, None, p, 64, 64, 64, 64, 64, other, E.DTYPE_F32, 0, s),
        "op_gemm: out_dtype": lambda: lib.gitmi_op_gemm(p, p, None, None, p, 64, 64, 64, 64, 64, own, other, 0, s),
        "op_attention: dtype": lambda: lib.gitmi_op_attention(p, p, 1, 16, 1, other, 1, s),
        "op_attn_decode: dtype": lambda: lib.gitmi_op_attn_decode(p, p, p, p, p, p, p, 1, 1, 16, 8, 0, 1, other, 0, s),
        "op_layernorm: out_dtype": lambda: lib.gitmi_op_layernorm(p, p, p, 1e-5, p, None, 4, 64, other, s),
    }
    for name, call in calls.items():
        with pytest.raises(E.GitmiError, match=name):
            E._ck(call(), lib)
    torch.cuda.synchronize()
    assert buf.abs().sum().item() == 0
    a, w = torch.zeros(64, 64, dtype=torch.float16, device="cuda"), torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    bias = torch.zeros(64, device="cuda")
    with pytest.raises(E.GitmiError):
        E.op_dgemm(a, w, bias)
    with pytest.raises(E.GitmiError):
        E.op_dgemm_res(a, w, bias, torch.zeros(64, 64, device="cuda"))
    with pytest.raises(E.GitmiError):
        E.op_vocab_topm(a, w, bias, 2)
    with pytest.raises(E.GitmiError):
        E.kv_repack(a.reshape(1, 1, 64, 64), w.reshape(1, 1, 64, 64))
    own16 = a if operands == "f16" else w
    with pytest.raises(E.GitmiError, match="stream form's residual"):          # fp32 residual rows handed to the stream form
        E.op_gemm(own16, own16, None, torch.zeros(64, 64, device="cuda"), 0, stream_rows=True)
