"""Op test of the tree attention (csrc/kernels_score.hip: tree_structure_kernel, then score_attn_mfma_kernel / score_attn_kernel in
their tree instantiation) against fp64 torch through the measurement build's hook gitmi_debug_score_attn_tree: every row attends to
the image keys of its image and to its own ancestors and itself, the ancestor matrix built on the host from the parents.

One call holds three trees in Lp = 144 rows: 16 nodes in a chain (a sentence; the tail of its rows is padding), 70 leaves under
the root (no key block past the first can be skipped for the queries it holds, every later block is skipped for the rest) and 130
nodes of random shape, deep enough that whole key blocks lie in finished subtrees (the skip fires) and others do not."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LP = 144


def _op_dtype():
    from generativeimage2text_amd import engine
    lib = engine.load_library()
    return {engine.DTYPE_BF16: torch.bfloat16, engine.DTYPE_F16: torch.float16}[lib.gitmi_operand_dtype()]


def _trees():
    gen = torch.Generator().manual_seed(7)
    deep = [0]
    for _ in range(129):
        deep.append(int(torch.randint(1, min(deep[-1] + 1, 39) + 1, (1,), generator=gen)))
    return [list(range(16)), [0] + [1] * 69, deep]


def _visible(depths):
    """[LP, LP] bool: text key t is node j itself or one of its ancestors; rows past the tree's nodes see themselves"""
    vis = torch.eye(LP, dtype=torch.bool)
    path = {}
    for j, d in enumerate(depths):
        path[d] = j
        for k in range(d):
            vis[j, path[k]] = True
    return vis


def _ref(qkv, img_kv, image_of, ntok, trees, H, N_img):
    d, Q = H * 64, len(trees)
    x = qkv.double().view(Q, LP, 3 * d)
    im = img_kv.double().view(-1, N_img, 3 * d)
    out = torch.empty(Q, LP, d, dtype=torch.float64)
    for q, depths in enumerate(trees):
        b, n_i = int(image_of[q]), int(ntok[int(image_of[q])])
        mask = torch.cat([torch.ones(LP, n_i, dtype=torch.bool), _visible(depths)], 1)
        for h in range(H):
            qh = x[q, :, h * 64:(h + 1) * 64]
            k = torch.cat([im[b, :n_i, d + h * 64:d + (h + 1) * 64], x[q, :, d + h * 64:d + (h + 1) * 64]])
            v = torch.cat([im[b, :n_i, 2 * d + h * 64:2 * d + (h + 1) * 64], x[q, :, 2 * d + h * 64:2 * d + (h + 1) * 64]])
            s = (qh @ k.T / 8.0).masked_fill(~mask, float("-inf"))
            out[q, :, h * 64:(h + 1) * 64] = torch.softmax(s, -1) @ v
    return out.view(Q * LP, d)


@pytest.mark.parametrize("dtype", ["f32", "16"])
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("N_img, ntok", [(5, None), (33, [33, 20])])
def test_tree_attention(experiment_build, dtype, H, N_img, ntok):
    from generativeimage2text_amd.engine import op_score_attn_tree, pack_trees
    dt = torch.float32 if dtype == "f32" else _op_dtype()
    trees = _trees()
    Q, B = len(trees), 2
    gen = torch.Generator().manual_seed(N_img * 10 + H)
    qkv = torch.randn(Q * LP, 3 * H * 64, generator=gen).to(dt)
    img_kv = torch.randn(B * N_img, 3 * H * 64, generator=gen).to(dt)
    qkv[:, :H * 64] = (qkv[:, :H * 64].float() * 2).to(dt)          # queries ~ N(0, 2): neither flat nor one-hot, as in the score op test
    image_of = torch.tensor([1, 0, 1], dtype=torch.int32)
    depths = torch.zeros(Q, LP, dtype=torch.int64)
    for q, t in enumerate(trees):
        depths[q, :len(t)] = torch.tensor(t)
    lens = [len(t) for t in trees]
    table, _ = pack_trees(torch.ones(Q, LP, dtype=torch.int64), depths, lens, vocab=2, max_depth=40)
    nt = None if ntok is None else torch.tensor(ntok, dtype=torch.int32)
    got, bad = op_score_attn_tree(qkv.cuda(), img_kv.cuda(), image_of, table, lens, 40, Q, H, N_img, LP, ntok=nt)
    assert bad.tolist() == [0, 0, 0]
    ref = _ref(qkv, img_kv, image_of, ntok or [N_img] * B, trees, H, N_img)
    err = (got.double().cpu() - ref).abs().max().item()
    # f32: within 1e-5 of the largest output; 16-bit: the operand rounding test_gpu_score_ops.py::test_score_attention allows
    # (probabilities rounded to the operand type before P V, values N(0, 1), the output rounded once)
    tol = 1e-5 * ref.abs().max().item() if dtype == "f32" else (3e-2 if dt == torch.bfloat16 else 5e-3)
    print(f"tree attention {dtype} H={H} N_img={N_img}: max error {err:.3e} tolerance {tol:.3e}")
    assert err <= tol, (dtype, H, N_img, err, tol)


@pytest.mark.parametrize("dtype", ["f32", "16"])
def test_rejected_tree_rows_see_the_image_and_themselves(experiment_build, dtype):
    """A tree that breaks the depth rules is flagged and becomes parentless rows: its attention is the padding rows' attention"""
    from generativeimage2text_amd.engine import op_score_attn_tree
    dt = torch.float32 if dtype == "f32" else _op_dtype()
    H, N_img = 1, 5
    gen = torch.Generator().manual_seed(3)
    qkv = torch.randn(3 * LP, 3 * 64, generator=gen).to(dt)
    img_kv = torch.randn(2 * N_img, 3 * 64, generator=gen).to(dt)
    trees = _trees()
    depths = torch.zeros(3, LP, dtype=torch.int64)
    for q, t in enumerate(trees):
        depths[q, :len(t)] = torch.tensor(t)
    depths[1, 40] = 3                                           # a jump of 2 among the leaves
    table = (depths << 32) | 1
    image_of = torch.tensor([1, 0, 1], dtype=torch.int32)
    got, bad = op_score_attn_tree(qkv.cuda(), img_kv.cuda(), image_of, table, [len(t) for t in trees], 40, 3, H, N_img, LP)
    assert bad.tolist() == [0, 1, 0]
    ref = _ref(qkv, img_kv, image_of, [N_img] * 2, [trees[0], [], trees[2]], H, N_img)
    tol = 1e-5 * ref.abs().max().item() if dtype == "f32" else (3e-2 if dt == torch.bfloat16 else 5e-3)      # test_tree_attention's
    assert (got.double().cpu() - ref).abs().max().item() <= tol
