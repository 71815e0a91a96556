"""Op tests of the caption-scoring kernels (csrc/kernels_score.hip) against fp64 torch, through the measurement build's
hooks (include/gitmi_experiment.h): the text attention (MFMA form in the 16-bit build dtype, fp32 form of the parity mode)
and the vocabulary head with its fused log-softmax statistics."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _op_dtype():
    from generativeimage2text_amd import engine
    lib = engine.load_library()
    return {engine.DTYPE_BF16: torch.bfloat16, engine.DTYPE_F16: torch.float16}[lib.gitmi_operand_dtype()]


def _attn_ref(qkv, img_kv, image_of, Q, H, N_img, Lp):
    """fp64: row (q, j) attends to the N_img image keys of image_of[q] and to text keys 0..j of sentence q, scale 1/8."""
    d = H * 64
    x = qkv.double().cpu().view(Q, Lp, 3 * d)
    im = img_kv.double().cpu().view(-1, N_img, 3 * d)
    out = torch.empty(Q, Lp, d, dtype=torch.float64)
    causal = torch.triu(torch.full((Lp, Lp), float("-inf"), dtype=torch.float64), diagonal=1)
    for q in range(Q):
        b = int(image_of[q])
        for h in range(H):
            qh = x[q, :, h * 64:(h + 1) * 64]
            k = torch.cat([im[b, :, d + h * 64:d + (h + 1) * 64], x[q, :, d + h * 64:d + (h + 1) * 64]])
            v = torch.cat([im[b, :, 2 * d + h * 64:2 * d + (h + 1) * 64], x[q, :, 2 * d + h * 64:2 * d + (h + 1) * 64]])
            s = qh @ k.T / 8.0
            s[:, N_img:] += causal
            out[q, :, h * 64:(h + 1) * 64] = torch.softmax(s, -1) @ v
    return out.view(Q * Lp, d)


@pytest.mark.parametrize("dtype", ["f32", "16"])
@pytest.mark.parametrize("N_img", [50, 197, 1201])
@pytest.mark.parametrize("Lp", [1, 16, 40, 80, 130])
def test_score_attention(experiment_build, dtype, N_img, Lp):
    from generativeimage2text_amd.engine import op_score_attn
    dt = torch.float32 if dtype == "f32" else _op_dtype()
    Q, H, B = 3, 2, 2
    gen = torch.Generator().manual_seed(N_img * 1000 + Lp)
    qkv = torch.randn(Q * Lp, 3 * H * 64, generator=gen).to(dt)
    img_kv = torch.randn(B * N_img, 3 * H * 64, generator=gen).to(dt)
    # scores of a realistic spread: queries ~ N(0, 2), so that the softmax is neither flat nor one-hot
    qkv[:, :H * 64] = (qkv[:, :H * 64].float() * 2).to(dt)
    image_of = torch.tensor([1, 0, 1], dtype=torch.int32)            # the indirection: sentence 0 and 2 on image 1
    got = op_score_attn(qkv.cuda(), img_kv.cuda(), image_of, Q, H, N_img, Lp).double().cpu()
    ref = _attn_ref(qkv, img_kv, image_of, Q, H, N_img, Lp)
    err = (got - ref).abs().max().item()
    # fp32: summation order only; 16-bit: probabilities rounded to the operand type before P V (values are N(0, 1)) and
    # the output rounded once
    tol = 2e-5 if dtype == "f32" else (3e-2 if dt == torch.bfloat16 else 5e-3)
    assert err <= tol, (dtype, N_img, Lp, err)


def _head_ref(A, W, bias, tgt):
    z = A.double().cpu() @ W.double().cpu().T + bias.double().cpu()
    ls = torch.log_softmax(z, -1)
    out = torch.zeros(A.shape[0], 2, dtype=torch.float64)
    for m, t in enumerate(tgt.tolist()):
        if t >= 0:
            out[m, 0] = ls[m, t]
            out[m, 1] = ls[m].mean()
    return out, z


@pytest.mark.parametrize("dtype", ["f32", "16"])
@pytest.mark.parametrize("V", [30522, 1001])
@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_score_head(experiment_build, dtype, V, offset):
    from generativeimage2text_amd.engine import op_score_head
    dt = torch.float32 if dtype == "f32" else _op_dtype()
    M, K = 133, 768                                              # two 128-row blocks, the second nearly empty
    gen = torch.Generator().manual_seed(V + int(offset))
    A = torch.randn(M, K, generator=gen).to(dt)
    W = (torch.randn(V, K, generator=gen) * 0.05).to(dt)
    bias = torch.randn(V, generator=gen) * 0.5 + offset            # a common offset on every logit of every row
    tgt = torch.randint(0, V, (M,), generator=gen, dtype=torch.int32)
    tail = (V // 128) * 128                                       # first column of the partial last 128-column tile
    tgt[0], tgt[1], tgt[2], tgt[3] = 0, V - 1, tail, 127          # first / last column, tail tile, a tile edge
    tgt[4] = -1
    tgt[-1] = V - 2
    got = op_score_head(A.cuda(), W.cuda(), bias.cuda(), tgt).double().cpu()
    ref, _ = _head_ref(A, W, bias, tgt)
    assert torch.all(got[4] == 0)
    # the logits themselves carry fp32 rounding at their magnitude (|z| ~ offset): the bound scales with it.  One base for both
    # operand types: the operands arrive already rounded and both paths accumulate in fp32 (a tile-wise fp32 emulation of the
    # 16-bit head is within 1e-6 of fp64, 3e-5 at offset 1e3; a last tile counted as 128 columns moves mean_lp by 2e-3 and more)
    tol = 2e-4 + 16 * max(1.0, offset) * 2.0 ** -23                 # 16 fp32 ulps of the logits' magnitude
    err_lp = (got[:, 0] - ref[:, 0]).abs().max().item()
    err_mean = (got[:, 1] - ref[:, 1]).abs().max().item()
    print(f"score head {dtype} V={V} offset={offset}: lp max error {err_lp:.3e}, mean_lp max error {err_mean:.3e}, bound {tol:.3e}")
    assert err_lp <= tol, (dtype, V, offset, err_lp, tol)
    assert err_mean <= tol, (dtype, V, offset, err_mean, tol)
