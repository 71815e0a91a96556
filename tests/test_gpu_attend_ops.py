"""Op test of the attention-map kernels (csrc/kernels_score.hip: the softmax statistics of the text attention and
score_attn_map_mfma_kernel / score_attn_map_kernel) against fp64 torch, through the measurement build's hook
gitmi_debug_score_attn_map: one layer's [Q, Lp, N_img + Lp] head-mean probabilities.

Shapes: H = 3 (a head mean that is no power of two), the image_of indirection, N_img = 50 (the tail of a key block), 197,
257 (one column past two of the map kernel's 128-column chunks) and 1 201, Lp = 1, 16 and 80 (the map kernel's 16-row
tiles: one partial, one full, five; two 64-row tiles of the attention launch), one ragged case.

Bound 2e-5 max-abs in both dtypes -- the figure the fp32 attention is held to in test_gpu_score_ops: the 16-bit products are
exact in the fp32 accumulator and no probability is rounded to 16 bits (nothing feeds a P V here), so only the order of
fp32 sums differs from the reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, H, B = 3, 3, 2
IMAGE_OF = [1, 0, 1]


def _op_dtype():
    from generativeimage2text_amd import engine
    lib = engine.load_library()
    return {engine.DTYPE_BF16: torch.bfloat16, engine.DTYPE_F16: torch.float16}[lib.gitmi_operand_dtype()]


def _inputs(dt, N_img, Lp):
    """as test_gpu_score_ops.test_score_attention: queries ~ N(0, 2), so that the softmax is neither flat nor one-hot"""
    gen = torch.Generator().manual_seed(N_img * 1000 + Lp)
    qkv = torch.randn(Q * Lp, 3 * H * 64, generator=gen).to(dt)
    img_kv = torch.randn(B * N_img, 3 * H * 64, generator=gen).to(dt)
    qkv[:, :H * 64] = (qkv[:, :H * 64].float() * 2).to(dt)
    return qkv, img_kv


def _map_ref(qkv, img_kv, N_img, Lp, ntok=None):
    """fp64 -> (map [Q, Lp, N_img + Lp], visible [Q, Lp, N_img + Lp] bool): image keys below the image's count, text keys 0..j"""
    d = H * 64
    x = qkv.double().view(Q, Lp, 3 * d)
    im = img_kv.double().view(B, N_img, 3 * d)
    out = torch.zeros(Q, Lp, N_img + Lp, dtype=torch.float64)
    vis = torch.zeros(Q, Lp, N_img + Lp, dtype=torch.bool)
    for q in range(Q):
        b = IMAGE_OF[q]
        n = N_img if ntok is None else int(ntok[b])
        vis[q, :, :n] = True
        vis[q, :, N_img:] = torch.tril(torch.ones(Lp, Lp, dtype=torch.bool))
        for h in range(H):
            k = torch.cat([im[b, :, d + h * 64:d + (h + 1) * 64], x[q, :, d + h * 64:d + (h + 1) * 64]])
            s = x[q, :, h * 64:(h + 1) * 64] @ k.T / 8.0
            s[~vis[q]] = float("-inf")
            out[q] += torch.softmax(s, -1) / H
    return out, vis


def _check(got, ref, vis, what):
    print(what, "max-abs error", (got - ref).abs().max().item(), "row sums off by", (got.sum(-1) - 1).abs().max().item())
    assert torch.all(got[~vis] == 0), what                                   # masked entries are exactly 0
    assert (got.sum(-1) - 1).abs().max().item() <= 1e-4, what                # every row is valid here
    assert (got - ref).abs().max().item() <= 2e-5, what


@pytest.mark.parametrize("dtype", ["f32", "16"])
@pytest.mark.parametrize("N_img", [50, 197, 257, 1201])
@pytest.mark.parametrize("Lp", [1, 16, 80])
def test_attention_map(experiment_build, dtype, N_img, Lp):
    from generativeimage2text_amd.engine import op_score_attn_map
    dt = torch.float32 if dtype == "f32" else _op_dtype()
    qkv, img_kv = _inputs(dt, N_img, Lp)
    image_of = torch.tensor(IMAGE_OF, dtype=torch.int32)
    got = op_score_attn_map(qkv.cuda(), img_kv.cuda(), image_of, Q, H, N_img, Lp)
    again = op_score_attn_map(qkv.cuda(), img_kv.cuda(), image_of, Q, H, N_img, Lp)
    assert torch.equal(got, again)                                           # two launches: bit-equal
    ref, vis = _map_ref(qkv, img_kv, N_img, Lp)
    _check(got.double().cpu(), ref, vis, (dtype, N_img, Lp))


@pytest.mark.parametrize("dtype", ["f32", "16"])
def test_attention_map_ragged(experiment_build, dtype):
    """ntok = [50, 37]: image 1's keys end at 37 of its 50-row block; the columns past them are exactly 0"""
    from generativeimage2text_amd.engine import op_score_attn_map
    dt = torch.float32 if dtype == "f32" else _op_dtype()
    N_img, Lp = 50, 16
    qkv, img_kv = _inputs(dt, N_img, Lp)
    ntok = torch.tensor([50, 37], dtype=torch.int32)
    got = op_score_attn_map(qkv.cuda(), img_kv.cuda(), torch.tensor(IMAGE_OF, dtype=torch.int32), Q, H, N_img, Lp, ntok=ntok)
    ref, vis = _map_ref(qkv, img_kv, N_img, Lp, ntok=ntok)
    assert not vis[0, :, 37:N_img].any() and vis[1, :, 37:N_img].all()
    _check(got.double().cpu(), ref, vis, (dtype, "ragged"))
