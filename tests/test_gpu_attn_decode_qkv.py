"""GPU: the decode attention that computes its own q | k | v (csrc/kernels_attn_decode.hip attn_decode_qkv_kernel) against the
two launches it replaces, through the measurement builds' hook gitmi_debug_attn_decode_qkv (include/gitmi_experiment.h).

Reference, on the same operands: gitmi_debug_dgemm_form in the engine's QKV form (consumer epilogue, N = 3 d, the serving
policy's rows_per_wg = 32 / strips_per_wg = 2), then gitmi_debug_attn_decode_form with pairs_per_wg = 8, waves_per_pair = 1 and
fragment-major output.  The fused launch must give the same `out` and the same text K/V caches BIT FOR BIT (torch.equal on the
raw 16-bit words), in both operand builds: the engine switches between the two by policy and gitmi_set_shared_device promises
identical results.

Shapes: 8 sentences (one block), 9 (a partial second block), 24 and 64 (the benchmark's; 96 workgroups); 2 heads (K = 128: one
k-step per K slice) and 12 (K = 768: six); 5, 33 and 197 image keys (one key step, two, and two chunks with a partial step);
position 0, 3 and T_max - 1 (28 text items: past the 24 requested up front); with and without the folded LayerNorm's strip
statistics (layer 0 against later layers); sentence -> image indirection given and NULL."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T_MAX = 28
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def _raw(t):
    return t.contiguous().view(torch.int16)


class Inputs:
    """operands of one geometry, drawn once on the CPU in fp32 and rounded once to `dtype`; device copies"""

    def __init__(self, dtype, B, H, N_img, seed):
        from generativeimage2text_amd import engine as E
        d = H * 64
        g = torch.Generator().manual_seed(4200 + seed)
        # raw hidden rows with a mean and a per-row scale (what a folded LayerNorm is for), their strip partials
        x = torch.randn(B, d, generator=g) * (0.5 + torch.rand(B, 1, generator=g)) + 0.3 * torch.randn(B, 1, generator=g)
        xd = x.to(dtype)
        xs = xd.float().reshape(B, d // 16, 16)
        self.stats = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).permute(1, 0, 2).contiguous().cuda()    # [d / 16][B][2]
        W = (torch.randn(3 * d, d, generator=g) * (2.0 / d ** 0.5)).to(dtype)
        W[:d] *= 2.0                                    # queries wide enough that the softmax is not flat
        self.bias = (0.1 * torch.randn(3 * d, generator=g)).cuda()
        self.colsum = W.float().sum(1).cuda()
        self.xf = E.to_frag(xd, 64).cuda()
        self.wf = E.to_frag(W).cuda()
        ik = torch.randn(B, H, N_img, 64, generator=g).to(dtype).cuda()
        iv = torch.randn(B, H, N_img, 64, generator=g).to(dtype).cuda()
        self.kf, self.vt = E.kv_repack(ik, iv)
        self.tk = torch.randn(B, T_MAX, d, generator=g).to(dtype).cuda()
        self.tv = torch.randn(B, T_MAX, d, generator=g).to(dtype).cuda()
        self.src = torch.arange(B)[:, None].expand(B, T_MAX).contiguous().int().cuda()
        self.img_of = [(5 * b + 3) % B for b in range(B)]          # several sentences per image, some images unused
        self.B, self.H, self.N_img, self.d = B, H, N_img, d


def _two_launches(E, c, pos, stats, img_of):
    tk, tv = c.tk.clone(), c.tv.clone()
    kw = dict(colsum=c.colsum, stats=c.stats) if stats else {}
    qkv = E.op_dgemm_form(c.xf, c.wf, c.bias, M=c.B, packed=True, rows_per_wg=32, strips_per_wg=2, **kw)
    out = E.op_attn_decode_form(qkv, c.kf, c.vt, tk, tv, c.src, c.B, c.H, c.N_img, T_MAX, pos, 1, img_of=img_of, out_frag=True,
                                pairs_per_wg=8, waves_per_pair=1)
    return qkv, out, tk, tv


def _one_launch(E, c, pos, stats, img_of):
    tk, tv = c.tk.clone(), c.tv.clone()
    kw = dict(colsum=c.colsum, stats=c.stats) if stats else {}
    out = E.op_attn_decode_qkv(c.xf, c.wf, c.bias, c.kf, c.vt, tk, tv, c.src, c.B, c.H, c.N_img, T_MAX, pos, img_of=img_of,
                               out_frag=True, **kw)
    return out, tk, tv


@pytest.mark.parametrize("ops", sorted(DTYPES))
@pytest.mark.parametrize("N_img", [5, 33, 197])
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("B", [8, 9, 24, 64])
def test_fused_launch_equals_qkv_gemm_then_attention(experiment_build, B, H, N_img, ops):
    from generativeimage2text_amd import engine as E
    c = Inputs(DTYPES[ops], B, H, N_img, seed=B * 1000 + H * 10 + N_img)
    for pos in (0, 3, T_MAX - 1):
        for stats in (False, True):
            for img_of in (None, c.img_of):
                what = (ops, B, H, N_img, pos, stats, img_of is not None)
                qkv, ref, rk, rv = _two_launches(E, c, pos, stats, img_of)
                out, tk, tv = _one_launch(E, c, pos, stats, img_of)
                torch.cuda.synchronize()
                rows = E.from_frag(ref, B), E.from_frag(out, B)
                assert torch.isfinite(rows[0].float()).all(), what
                # the appended position is this step's k | v of every row (so the caches compare the projection itself) ...
                assert torch.equal(_raw(rk[:, pos]), _raw(qkv[:, c.d:2 * c.d])) and torch.equal(_raw(rv[:, pos]), _raw(qkv[:, 2 * c.d:])), what
                # ... and the fused launch leaves the same caches and the same output rows
                assert torch.equal(_raw(tk), _raw(rk)), (what, "text K cache")
                assert torch.equal(_raw(tv), _raw(rv)), (what, "text V cache")
                assert torch.equal(_raw(rows[1]), _raw(rows[0])), (what, "out", (rows[1].float() - rows[0].float()).abs().max().item())
                # two different positions or statistics must not give the same answer by accident of a stale buffer
                assert not torch.equal(_raw(tk), _raw(c.tk)), what


@pytest.mark.parametrize("ops", sorted(DTYPES))
def test_row_major_output_and_layer_statistics_change_the_result(experiment_build, ops):
    """out_frag = 0 works as well, and the folded statistics are really applied: with and without them the rows differ"""
    from generativeimage2text_amd import engine as E
    c = Inputs(DTYPES[ops], 16, 12, 33, seed=7)
    outs = {}
    for stats in (False, True):
        kw = dict(colsum=c.colsum, stats=c.stats) if stats else {}
        tk, tv = c.tk.clone(), c.tv.clone()
        outs[stats] = E.op_attn_decode_qkv(c.xf, c.wf, c.bias, c.kf, c.vt, tk, tv, c.src, c.B, c.H, c.N_img, T_MAX, 2, **kw)
        _, ref, _, _ = _two_launches(E, c, 2, stats, None)
        assert torch.equal(_raw(outs[stats]), _raw(E.from_frag(ref, c.B))), (ops, stats)
    assert not torch.equal(_raw(outs[False]), _raw(outs[True]))


@pytest.mark.parametrize("ops", sorted(DTYPES))
def test_calls_outside_the_form_are_refused_by_name(experiment_build, ops):
    """beam batches, ragged batches, two-wave pairs, the streaming form and other packings keep their QKV launch: the hook names
    what it refuses and launches nothing (the caches keep every element)"""
    from generativeimage2text_amd import engine as E
    c = Inputs(DTYPES[ops], 8, 2, 33, seed=11)
    tk, tv = c.tk.clone(), c.tv.clone()
    ntok = [33] * c.B
    for kw, name in ((dict(beams=4), "beams=4"), (dict(ntok=ntok), "ntok"), (dict(waves_per_pair=2), "waves_per_pair=2"),
                     (dict(stream_wgs=96), "stream_wgs=96"), (dict(pairs_per_wg=4), "pairs_per_wg=4")):
        B = c.B // kw.get("beams", 1)
        with pytest.raises(E.GitmiError, match=name):
            E.op_attn_decode_qkv(c.xf, c.wf, c.bias, c.kf, c.vt, tk, tv, c.src, B, c.H, c.N_img, T_MAX, 1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(_raw(tk), _raw(c.tk)) and torch.equal(_raw(tv), _raw(c.tv))


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_shared_device_policy_is_bitwise_neutral_at_8_sentences(precision):
    """Engine level, GIT_BASE geometry, B = 8, 6 steps: ids, log-probs and teacher-forced step logits under
    set_shared_device(True) equal those under False bit for bit.  (96 pairs: the launcher packs fewer than 8 pairs per workgroup
    here, so both policies keep the QKV launch; tests/test_gpu_policy.py holds the two policies to each other at the benchmark's
    64 sentences, where the serving policy runs the fused launch.)"""
    from generativeimage2text_amd.configs import config_for_model
    from generativeimage2text_amd.engine import Engine
    from generativeimage2text_amd.synthetic import random_frames, random_state_dict
    cfg = config_for_model("GIT_BASE")
    B, steps = 8, 6
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=1, max_frames=1, max_text_len=steps)
    eng.load_state_dict(random_state_dict(cfg, seed=1234))
    frames = random_frames(cfg, B, 1, seed=0)
    search = Engine.make_search("greedy", steps, 1, 1)
    out = {}
    for on in (False, True):
        eng.set_shared_device(on)
        tok, lp, _ = eng.generate(frames, search)
        eng.encode(frames, return_features=False)
        eng.prefill()
        logits = eng.step_logits(tok[:, :steps].clone())
        out[on] = (tok.clone(), lp.clone(), logits.clone())
    eng.close()
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
