"""Op tests of the ragged-batch attention (gitmi_set_image_shape(e, 0, 0)) against fp64 torch, through the measurement build's
hooks (include/gitmi_experiment.h): every image of a launch has its own key count inside the capacity block of N rows.
Encoder / prefill attention (VALU f32 form, short single-pass and 64-key flash MFMA forms) and decode attention (VALU f32,
two-wave MFMA) with 1, 31, 32, 33, 881, 901 and 1201 keys; padding query rows must come back as zeros."""
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = [1, 31, 32, 33, 881, 901, 1201]


def _op_dtype():
    from generativeimage2text_amd import engine
    lib = engine.load_library()
    return {engine.DTYPE_BF16: torch.bfloat16, engine.DTYPE_F16: torch.float16}[lib.gitmi_operand_dtype()]


def _full_ref(qkv, ntok, N, H):
    d = H * 64
    x = qkv.double().cpu().view(len(ntok), N, 3 * d)
    out = torch.zeros(len(ntok), N, d, dtype=torch.float64)
    for b, n in enumerate(ntok):
        for h in range(H):
            q = x[b, :n, h * 64:(h + 1) * 64]
            k = x[b, :n, d + h * 64:d + (h + 1) * 64]
            v = x[b, :n, 2 * d + h * 64:2 * d + (h + 1) * 64]
            out[b, :n, h * 64:(h + 1) * 64] = torch.softmax(q @ k.T / 8.0, -1) @ v
    return out.view(-1, d)


@pytest.mark.parametrize("N,ntok,impl", [(1201, COUNTS, 1), (1201, COUNTS, 2), (197, [1, 31, 32, 33, 150, 197], 1),
                                         (257, [1, 2, 33, 200, 257], 1), (1201, COUNTS, 0)])
def test_attention_ragged(experiment_build, N, ntok, impl):
    """impl 1 at N = 197 / 257 runs the ragged short single-pass kernels (13 / 17 sub-tiles), at 1201 the flash kernel; impl 0
    is the f32 VALU form of the parity mode"""
    from generativeimage2text_amd import engine as E
    H, B = 2, len(ntok)
    dtype = torch.float32 if impl == 0 else _op_dtype()
    g = torch.Generator().manual_seed(N + impl)
    qkv = torch.randn(B * N, 3 * H * 64, generator=g)
    qkv[:, :H * 64] *= 1.5
    for b, n in enumerate(ntok):          # padding rows hold garbage: it must neither leak in nor come out
        qkv[b * N + n:(b + 1) * N] = 1e4
    qkv = qkv.to(dtype)
    out = E.op_attention_ragged(qkv.cuda(), ntok, B, N, H, impl).cpu().double()
    ref = _full_ref(qkv, ntok, N, H)
    tol = 3e-5 if dtype == torch.float32 else 3e-2
    for b, n in enumerate(ntok):
        err = (out[b * N:b * N + n] - ref[b * N:b * N + n]).abs().max().item()
        assert err < tol, (b, n, err)
        assert torch.count_nonzero(out[b * N + n:(b + 1) * N]) == 0, (b, n, "padding query rows are not zero")


@pytest.mark.parametrize("N_img,ntok", [(1201, COUNTS), (200, [1, 31, 32, 33, 200])])
@pytest.mark.parametrize("beams,pos", [(1, 0), (2, 5)])
@pytest.mark.parametrize("f32", [True, False])
def test_attn_decode_ragged(experiment_build, N_img, ntok, beams, pos, f32):
    """N_img = 200 (N_pad 224): the one-wave geometry of a uniform call -- a ragged image of <= 32 keys leaves the second
    wave of the two-wave kernel without image steps"""
    from generativeimage2text_amd import engine as E
    H, B = 2, len(ntok)
    d, R, T = H * 64, B * beams, pos + 4
    dtype = torch.float32 if f32 else _op_dtype()
    g = torch.Generator().manual_seed(7 * N_img + pos)
    qkv = (torch.randn(R, 3 * d, generator=g) * 1.2).to(dtype)
    ik = torch.randn(B, H, N_img, 64, generator=g)
    iv = torch.randn(B, H, N_img, 64, generator=g)
    for b, n in enumerate(ntok):
        ik[b, :, n:] = 1e4
        iv[b, :, n:] = 1e4
    ik, iv = ik.to(dtype), iv.to(dtype)
    tk = torch.randn(R, T, d, generator=g).to(dtype)
    tv = torch.randn(R, T, d, generator=g).to(dtype)
    src = torch.stack([torch.randint(b * beams, (b + 1) * beams, (T,), generator=g) for b in range(B) for _ in range(beams)]).int()
    out = E.op_attn_decode_ragged(qkv.cuda(), ik.cuda(), iv.cuda(), tk.cuda().clone(), tv.cuda().clone(), src.cuda(), ntok, B, H,
                                  N_img, T, pos, beams).cpu().double()
    ref = torch.zeros(R, d, dtype=torch.float64)
    for r in range(R):
        b = r // beams
        n = ntok[b]
        for h in range(H):
            q = qkv[r, h * 64:(h + 1) * 64].double() * 0.125
            ks = [ik[b, h, :n].double()] + [tk[src[r, s], s, h * 64:(h + 1) * 64].double()[None] for s in range(pos)] + \
                 [qkv[r, d + h * 64:d + (h + 1) * 64].double()[None]]
            vs = [iv[b, h, :n].double()] + [tv[src[r, s], s, h * 64:(h + 1) * 64].double()[None] for s in range(pos)] + \
                 [qkv[r, 2 * d + h * 64:2 * d + (h + 1) * 64].double()[None]]
            p = torch.softmax(torch.cat(ks) @ q, 0)
            ref[r, h * 64:(h + 1) * 64] = p @ torch.cat(vs)
    tol = 3e-5 if f32 else 3e-2
    err = (out - ref).abs().max().item()
    assert err < tol, err
