"""The context kernel of GITMI_SEARCH_CONTEXT (csrc/kernels_norm.hip context_embed_kernel) on its own, through the measurement
build's hook, against an fp64 restatement: LayerNorm(words[tok] + positions[p], eps 1e-8) of every valid context token, written
behind the image rows of its image's block; zeros behind them; the key counts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N_IMG, VOCAB, MAX_POS, EPS = 3, 17, 211, 24, 1e-8
# segment q -> (image, length): image 0 none, image 1 one token, image 2 sixteen in three segments (7, 5, 4) interleaved with
# image 1's.  A kernel that let positions run on across the segments of an image embeds rows 7.. of image 2 with the wrong positions.
SEGMENTS = [(2, 7), (1, 1), (2, 5), (2, 4)]
COUNTS = [0, 1, 16]
LD = 9
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _tables(D, seed):
    g = torch.Generator().manual_seed(seed)
    words = 0.02 * torch.randn(VOCAB, D, generator=g)
    positions = 0.02 * torch.randn(MAX_POS, D, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    tokens = torch.randint(0, VOCAB, (len(SEGMENTS), LD), generator=g)
    for q, (_, n) in enumerate(SEGMENTS):
        tokens[q, n:] = (1 << 40) + q              # ids past a length are never read
    return words, positions, gamma, beta, tokens


def _reference(words, positions, gamma, beta, tokens, stride):
    """fp64: (rows [B, stride, D] with the context rows set and NaN everywhere else, ntok)"""
    D = words.shape[1]
    ref = torch.full((B, stride, D), float("nan"), dtype=torch.float64)
    used = [0] * B
    for q, (im, n) in enumerate(SEGMENTS):
        x = words[tokens[q, :n]].double() + positions[:n].double()          # positions restart at 0 in every segment
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        y = (x - mu) / torch.sqrt(var + EPS) * gamma.double() + beta.double()
        ref[im, N_IMG + used[im]:N_IMG + used[im] + n] = y
        used[im] += n
    assert used == COUNTS
    return ref, [N_IMG + c for c in COUNTS]


@pytest.mark.parametrize("stride", [40, 33])
@pytest.mark.parametrize("operand", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("D", [128, 768])
def test_context_rows_pad_rows_and_counts(experiment_build, D, operand, stride):
    from generativeimage2text_amd import engine
    dt = DTYPES[operand]
    words, positions, gamma, beta, tokens = _tables(D, seed=D + stride)
    ref, ntok_ref = _reference(words, positions, gamma, beta, tokens, stride)
    g = torch.Generator().manual_seed(7)
    before = torch.randn(B, stride, D, generator=g).to(dt).cuda()          # image rows as ln_post left them, garbage behind them
    feats = before.clone()
    ntok, copy = engine.op_context_embed(tokens.cuda(), [n for _, n in SEGMENTS], [im for im, _ in SEGMENTS], words.cuda(),
                                         positions.cuda(), gamma.cuda(), beta.cuda(), EPS, feats, N_IMG, want_f32=True,
                                         operands="f16" if operand == "f16" else "bf16")
    torch.cuda.synchronize()
    assert ntok.cpu().tolist() == ntok_ref                                  # exact
    feats_c, copy_c = feats.cpu(), copy.cpu()
    # image rows: bit-unchanged; the fp32 copy was not written there
    assert torch.equal(feats_c[:, :N_IMG].view(torch.uint8), before.cpu()[:, :N_IMG].view(torch.uint8))
    assert torch.all(copy_c[:, :N_IMG] == 0)
    for b in range(B):
        lo, hi = N_IMG, ntok_ref[b]
        # pad rows: exactly zero, in both outputs
        assert torch.all(feats_c[b, hi:].view(torch.uint8) == 0) and torch.all(copy_c[b, hi:] == 0), b
        if hi == lo:
            continue
        # context rows: the bounds of tests/test_gpu_search_ops.py::test_search_step_embedding for the same arithmetic --
        # the fp32 rows within 2e-5 of fp64 (test_layernorm's fp32 bound), the 16-bit rows the fp32 ones rounded to the operand type
        err = (copy_c[b, lo:hi].double() - ref[b, lo:hi]).abs().max().item()
        print(f"D {D} {operand} stride {stride} image {b}: fp32 error {err:.2e}")
        assert err < 2e-5, (b, err)
        assert torch.equal(feats_c[b, lo:hi], copy_c[b, lo:hi].to(dt)), b
    assert not torch.isnan(ref[2, N_IMG:N_IMG + 16]).any() and torch.isnan(ref[0]).all()


def test_context_hook_refuses_rows_outside_a_block(experiment_build):
    from generativeimage2text_amd import engine
    D, stride = 128, 32                                                     # 17 + 16 rows do not fit
    words, positions, gamma, beta, tokens = _tables(D, seed=3)
    feats = torch.zeros(B, stride, D, device="cuda")
    args = (words.cuda(), positions.cuda(), gamma.cuda(), beta.cuda(), EPS, feats, N_IMG)
    with pytest.raises(engine.GitmiError, match=r"needs 33 rows \(17 image rows \+ 16 context rows\), the capacity is 32 rows"):
        engine.op_context_embed(tokens.cuda(), [n for _, n in SEGMENTS], [im for im, _ in SEGMENTS], *args)
    with pytest.raises(engine.GitmiError, match=r"length 10 of context segment 0 outside \[1,9\]"):
        engine.op_context_embed(tokens.cuda(), [10, 1, 1, 1], [0, 0, 0, 0], *args)
    with pytest.raises(engine.GitmiError, match="names image 3 of 3"):
        engine.op_context_embed(tokens.cuda(), [1, 1, 1, 1], [0, 3, 0, 0], *args)
    assert torch.all(feats == 0)
