"""GPU: the image front end of the encoder (kernels_norm.hip) op by op, through the measurement build's hooks
(include/gitmi_experiment.h: an argument check + the launcher gitmi_encode_frames itself calls, so the launcher's kernel
selection is what runs): patch gather (im2col_kernel, im2col_p16_kernel), positional resize (pos_bicubic_kernel), token
assembly + ln_pre (vit_assemble_ln_kernel), their ragged-batch forms (ragged_stage_kernel, im2col_ragged_kernel,
vit_assemble_ragged_kernel, zero_pad_rows_kernel) and the ln_post scatter (layernorm_kernel / layernorm_wide_kernel with
add_after and the row map).  References are torch fp64 on the CPU from the same inputs after their input rounding; gathers,
staging and the ragged forms are compared bit for bit.  Every output sits in a sentinel-filled buffer whose margins must come
back untouched.  The bounds are derived where they are used; docs/LAB_NOTEBOOK.md repeats them."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from ln_reference import ln_ref_and_bound
from test_gpu_dgemm_forms import on_both_operand_builds

pytestmark = pytest.mark.gpu

U = 2.0 ** -24           # fp32 unit roundoff
SENT = 0x5A              # sentinel byte: 0x5A5A5A5A = 1.5e16 as fp32, 0x5A5A = 203.25 as fp16, 1.5e16 as bf16
MARGIN = 4096            # sentinel bytes either side of every output


# Every test of the file runs on the bf16 measurement build under its own name and, as <name>_f16, on the fp16 one
# (on_both_operand_builds, last line).  Most front-end calls have no tensor in the operand type (fp32 and fp16-stream tensors
# exist in both builds), so the engine module the tests see passes operands=BUILD["ops"] to every front-end hook.
BUILD = {"ops": "bf16"}
FRONT_HOOKS = ("op_im2col", "op_pos_resize", "op_vit_assemble", "op_ragged_front", "op_zero_pad_rows", "op_layernorm_map")


class _Front:
    def __getattr__(self, name):
        from generativeimage2text_amd import engine
        attr = getattr(engine, name)
        return functools.partial(attr, operands=BUILD["ops"]) if name in FRONT_HOOKS else attr


def _E():
    return _Front()


def _op_dtype():
    return {"bf16": torch.bfloat16, "f16": torch.float16}[BUILD["ops"]]


def _bits(t):
    """The tensor's elements as integers: equality of these is equality bit for bit (-0 != +0, NaN == the same NaN)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class Guarded:
    """A device tensor of `shape` inside a buffer of sentinel bytes: .t the tensor (sentinel-filled too), check() asserts the
    margins before and after it were not written."""

    def __init__(self, shape, dtype):
        self.nbytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * MARGIN + self.nbytes,), SENT, dtype=torch.uint8, device="cuda")
        self.t = self.raw[MARGIN:MARGIN + self.nbytes].view(dtype).view(*shape)

    def check(self, what=""):
        torch.cuda.synchronize()
        assert bool((self.raw[:MARGIN] == SENT).all()), (what, "bytes in front of the output were written")
        assert bool((self.raw[MARGIN + self.nbytes:] == SENT).all()), (what, "bytes behind the output were written")

    def cpu(self, what=""):
        self.check(what)
        return self.t.cpu()


def _untouched(t):
    """True when every byte of the (CPU or device) tensor still holds the sentinel."""
    return bool((t.contiguous().view(torch.uint8) == SENT).all())


def _hulp(x, dtype):
    """Half an ulp of the 16-bit type at |x| (fp16: subnormal spacing below 2^-14)."""
    if dtype == torch.float16:
        return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14))) - 11)
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 8)


def _assert_within(out, ref, bound, what):
    err = (out.double() - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = (err - bound).flatten().argmax()
        raise AssertionError(f"{what}: {int(bad.sum())} elements out of bound; worst: err {err.flatten()[i].item():.3e} bound "
                             f"{bound.flatten()[i].item():.3e} ref {ref.flatten()[i].item():.6g} got {out.flatten()[i].item():.6g}")


# ---- patch gather: exact ---------------------------------------------------------------------------------------------
def _pattern(n, dtype, device):
    """n pixel values that survive the rounding to `dtype` unchanged and do not repeat (fp32: the integers 0 .. n - 1 < 2^24;
    bf16 / fp16: the type's positive normal bit patterns 0x0080 + i, i modulo the prime 30011 -- no repeat inside an image row
    or column block, so no permuted gather reproduces it)."""
    i = torch.arange(n, device=device, dtype=torch.int32)
    if dtype == torch.float32:
        assert n < 2 ** 24
        return i.float()
    i = 0x0080 + i % 30011
    if dtype == torch.bfloat16:
        return (i << 16).view(torch.float32)
    return i.to(torch.int16).view(torch.float16).float()


def _gather_ref(img, p, Kpad, dtype):
    """img CPU fp32 [B, 3, H, W] -> [B gh gw, Kpad]: row (b, gy, gx), column c p p + ky p + kx = img[b, c, gy p + ky, gx p + kx]
    rounded to dtype, zeros past 3 p p; the H % p bottom rows and W % p right columns are not read."""
    B, _, H, W = img.shape
    gh, gw = H // p, W // p
    x = img[:, :, :gh * p, :gw * p].reshape(B, 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, 3 * p * p)
    out = torch.zeros(B * gh * gw, Kpad, dtype=dtype)
    out[:, :3 * p * p] = x.to(dtype)
    return out


def _run_im2col(img_dev, B, H, W, p, Kpad, dtype):
    out = Guarded((B * (H // p) * (W // p), Kpad), dtype)
    _E().op_im2col(img_dev, out.t, B, H, W, p, Kpad)
    return out.cpu("im2col")


def _image(B, H, W, kind, dtype, shift=0):
    """A device image [B, 3, H, W] whose data pointer is `shift` floats past a 16-byte boundary."""
    n = B * 3 * H * W
    buf = torch.empty(n + 4, device="cuda", dtype=torch.float32)
    img = buf[shift:shift + n]
    if kind == "pattern":
        img.copy_(_pattern(n, dtype, "cuda"))
    else:
        img.copy_(torch.randn(n, device="cuda", generator=torch.Generator("cuda").manual_seed(H * W + B)) * 2.0)
    assert img.data_ptr() % 16 == 4 * shift
    return img.view(B, 3, H, W)


IM2COL_CASES = [
    # the p16 kernel: p == 16, K == Kpad == 768, W % 4 == 0, 16-byte aligned image; eight pixels per thread
    ("p16", 2, 32, 48, 16, 768, 0), ("p16", 2, 48, 32, 16, 768, 0), ("p16", 1, 224, 224, 16, 768, 0),
    ("p16", 2, 40, 52, 16, 768, 0),        # H % 16 = 8 and W % 16 = 4 remainders are never read; W % 4 == 0 still selects p16
    # the launcher's fall-backs to the generic kernel with 16-bit output
    ("op", 2, 32, 50, 16, 768, 0),         # W % 4 != 0
    ("op", 2, 32, 48, 16, 768, 1),         # image pointer one float past a 16-byte boundary
    # the generic kernel
    ("op", 2, 30, 45, 14, 640, 0), ("f32", 2, 30, 45, 14, 640, 0),       # K = 588 padded to 640: pad columns exact zeros
    ("op", 1, 64, 100, 32, 3072, 0), ("f32", 1, 64, 100, 32, 3072, 0),
    ("f32", 2, 32, 48, 16, 768, 0),
]


@pytest.mark.parametrize("kind", ["pattern", "random"])
@pytest.mark.parametrize("out,B,H,W,p,Kpad,shift", IM2COL_CASES)
def test_im2col_is_an_exact_gather(experiment_build, out, B, H, W, p, Kpad, shift, kind):
    """No tolerance: every output element is the operand-rounded pixel of its (image, channel, row, column), bit for bit."""
    dtype = torch.float32 if out == "f32" else _op_dtype()
    img = _image(B, H, W, kind, dtype, shift)
    got = _run_im2col(img, B, H, W, p, Kpad, dtype)
    ref = _gather_ref(img.cpu(), p, Kpad, dtype)
    assert torch.equal(_bits(got), _bits(ref)), (out, B, H, W, p, int((_bits(got) != _bits(ref)).sum()))


@pytest.mark.parametrize("out,B", [("f32", 16), ("p16", 112)])
def test_im2col_grid_stride_loop_takes_a_second_trip(experiment_build, out, B):
    """The launchers cap the grid at 8192 x 256 = 2 097 152 threads: B = 16 at 224 x 224 is 2 408 448 fp32 elements, B = 112 is
    2 107 392 eight-pixel groups of the p16 kernel, so the last elements of both come from the loop's second trip.  Inputs are
    generated on the device."""
    dtype = torch.float32 if out == "f32" else _op_dtype()
    H = W = 224
    total = B * 196 * 768 // (1 if out == "f32" else 8)
    assert 8192 * 256 < total < 2 * 8192 * 256
    img = _image(B, H, W, "pattern", dtype)
    got = _run_im2col(img, B, H, W, 16, 768, dtype)
    ref = _gather_ref(img.cpu(), 16, 768, dtype)
    assert torch.equal(_bits(got), _bits(ref))


# ---- positional resize -----------------------------------------------------------------------------------------------
# Bound of pos_bicubic_kernel against fp64 F.interpolate(mode='bicubic', align_corners=False) on a table with |v| <= M = 4,
# stored grids g <= 14 (u = 2^-24):
#   source coordinate  f = ((float)o + 0.5) * fl(g / go) - 0.5: the quotient, the product and the difference round once
#     each on values <= g: |df| <= 3 u g.  The interpolant is continuous in f (at t -> 1 the taps (0, 0, 1, 0) of one cell
#     are the taps (0, 1, 0, 0) of the next), so a floor() that flips next to an integer costs no more than df itself;
#     t = f - floor(f) is exact.  Sum_i |dw_i / dt| <= 3.1 on [0, 1] for A = -0.75: the four taps of an axis move by <= 9.3 u g
#     together.
#   tap polynomials: Horner forms with intermediate values <= 6.75 (outer taps: 8 A x with x <= 2; 5 roundings + the one of
#     x = t + 1 passed through |dw/dx| <= 2.5) and <= 2.25 (inner taps, 5 roundings): <= (6 * 6.75 + 2.5 * 2) u = 45.5 u per
#     outer and 11.3 u per inner tap, 114 u for the four.
#   the two-pass sum: Sum |wx| and Sum |wy| <= 1.375 each (t = 0.5); eight multiply-adds on partial sums <= 1.375^2 M.
#   error <= M [2 * 1.375 (9.3 g + 114) u + 8 * 1.9 u] = M (25.6 g + 329) u = 2.75 (g / 14 + 0.92) 1e-5 M <= 1.6e-4 at M = 4, g = 14.
# The reference alone: torch's fp32 interpolate differs from its fp64 one by at most POS_REF_ERR = 4.4e-6 on unit-normal tables
# over exactly these grids (CPU, docs/LAB_NOTEBOOK.md) -- a typical-case figure of the same arithmetic class.  The test's
# bound is POS_K = 48 times that, 2.1e-4: the smallest multiple of 16 that covers the worst-case derivation above, so a correct
# kernel cannot fail, while a wrong A (-0.5: errors to 0.2), a half-pixel offset or a wrong clamp (order 0.1 and more) is
# 500 times outside it.
POS_REF_ERR = 4.4e-6
POS_K = 48
POS_BOUND = POS_K * POS_REF_ERR
POS_M = 4.0


def _pos_derived(g):
    return POS_M * (25.6 * g + 329) * U


def _pos_table(g, D, seed):
    t = torch.randn(g * g + 1, D, generator=torch.Generator().manual_seed(seed)).clamp_(-POS_M, POS_M)
    return t


def _pos_ref(pos, g, gh, gw):
    D = pos.shape[1]
    grid = pos[1:].double().reshape(1, g, g, D).permute(0, 3, 1, 2)
    r = F.interpolate(grid, size=(gh, gw), mode="bicubic", align_corners=False)
    return torch.cat([pos[:1].double(), r.permute(0, 2, 3, 1).reshape(gh * gw, D)], 0)


def _run_pos(pos_dev, g, gh, gw):
    out = Guarded((gh * gw + 1, pos_dev.shape[1]), torch.float32)
    _E().op_pos_resize(pos_dev, out.t, g, gh, gw)
    return out.cpu(f"pos_resize {g} -> {gh}x{gw}")


def _targets(g):
    return [(30, 40), (10, 14), (14, 13), (37, 37), (3, 50), (2 * g, 2 * g), (1, 1), (1, g), (g, 1)]


@pytest.mark.parametrize("D", [96, 768])
@pytest.mark.parametrize("g", [14, 10, 4])
def test_pos_resize_matches_fp64_bicubic(experiment_build, g, D):
    """(30, 40) is the 480 x 640 VQA shape; the non-square targets carry a random (so transposed-asymmetric) table: scaling
    both axes by gw, or swapping gh and gw, moves outputs by the table's own magnitude.  The class row is copied bit for bit."""
    assert _pos_derived(14) <= POS_BOUND < 1e-3
    pos = _pos_table(g, D, seed=100 * g + D)
    assert not torch.allclose(pos[1:].reshape(g, g, D), pos[1:].reshape(g, g, D).transpose(0, 1))
    dev = pos.cuda()
    for gh, gw in _targets(g):
        if (gh, gw) == (g, g):
            continue
        out = _run_pos(dev, g, gh, gw)
        ref = _pos_ref(pos, g, gh, gw)
        assert torch.equal(_bits(out[0]), _bits(pos[0])), (g, gh, gw, "class row")
        err = (out.double() - ref).abs().max().item()
        print(f"pos_resize g={g} D={D} -> {gh}x{gw}: max err {err:.3e} (bound {POS_BOUND:.3e})")
        assert err <= POS_BOUND, (g, gh, gw, err)


@pytest.mark.parametrize("D", [96, 768])
@pytest.mark.parametrize("g", [14, 10, 4])
def test_pos_resize_to_the_stored_grid_returns_the_table(experiment_build, g, D):
    """At (g, g) the scale is 1, t = 0 and the taps are exactly (0, 1, 0, 0) in fp32: the kernel returns the table bit for bit."""
    pos = _pos_table(g, D, seed=7 * g + D)
    out = _run_pos(pos.cuda(), g, g, g)
    assert torch.equal(_bits(out), _bits(pos))


# ---- LayerNorm bound shared by ln_pre and ln_post: ln_reference.py (the text pass's embedding uses it too) ------------------


# ---- token assembly + ln_pre ----------------------------------------------------------------------------------------
def _assemble_inputs(B, N, D, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    patch = torch.randn(B * (N - 1), D, generator=g) + offset
    cls = torch.randn(D, generator=g) * 1.5 + offset
    pos = torch.randn(N, D, generator=g) * 0.7
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.3 * torch.randn(D, generator=g)
    return patch, cls, pos, gamma, beta


def _assemble_ref(patch, cls, pos, gamma, beta, eps, B, N):
    D = cls.numel()
    src = torch.cat([cls.double().expand(B, 1, D), patch.double().reshape(B, N - 1, D)], 1)
    v = (src + pos.double()[None]).reshape(B * N, D)
    return ln_ref_and_bound(v, gamma, beta, eps)


def _check_partials(part, x16, what):
    """Slot 0 = (sum, sum of squares) of the fp16 row the kernel RETURNED, in fp32: 16 sequential adds per lane, 6 shuffle
    levels and the square's rounding: 24 u sum |o| and 24 u sum o^2; slots 1 .. 3 exact zeros."""
    o = x16.double()
    assert torch.count_nonzero(_bits(part[:, 1:])) == 0, (what, "partial slots 1..3 are not zero")
    _assert_within(part[:, 0, 0], o.sum(-1), 24 * U * o.abs().sum(-1), what + " sum")
    _assert_within(part[:, 0, 1], (o * o).sum(-1), 24 * U * (o * o).sum(-1), what + " sum of squares")


ASSEMBLE_SHAPES = [(3, 5), (2, 197)]        # 15 rows: not a multiple of the 4 rows per workgroup


@pytest.mark.parametrize("stream", ["f32", "f16"])
@pytest.mark.parametrize("B,N", ASSEMBLE_SHAPES)
@pytest.mark.parametrize("D,offset", [(768, 0.0), (1024, 0.0), (192, 0.0), (100, 0.0), (768, 60.0)])
def test_vit_assemble_ln_pre(experiment_build, D, offset, B, N, stream):
    """Distinct class, patch and positional rows (a wrong b (N - 1) + n - 1 or positional row is an O(1) error); D = 100 masks
    lanes by c < D; offset 60: rows whose mean is ~40 times their spread.  f32 stream: the LayerNorm bound above; fp16 stream:
    that + half an fp16 ulp, and the partials are those of the stored row."""
    E = _E()
    patch, cls, pos, gamma, beta = _assemble_inputs(B, N, D, seed=D + N, offset=offset)
    ref, bound = _assemble_ref(patch, cls, pos, gamma, beta, 1e-5, B, N)
    dt = torch.float32 if stream == "f32" else torch.float16
    X = Guarded((B * N, D), dt)
    part = Guarded((B * N, 4, 2), torch.float32) if stream == "f16" else None
    E.op_vit_assemble(patch.cuda(), cls.cuda(), pos.cuda(), gamma.cuda(), beta.cuda(), 1e-5, X.t, B, N,
                      part=None if part is None else part.t)
    out = X.cpu("vit_assemble X")
    if stream == "f16":
        bound = bound + _hulp(ref.abs() + bound, torch.float16)
    print(f"vit_assemble D={D} off={offset} B={B} N={N} {stream}: max err {(out.double() - ref).abs().max().item():.3e} "
          f"max bound {bound.max().item():.3e}")
    _assert_within(out, ref, bound, f"vit_assemble {stream}")
    if part is not None:
        _check_partials(part.cpu("vit_assemble partials"), out, "vit_assemble")


def test_vit_assemble_refuses_partials_of_an_f32_stream(experiment_build):
    E = _E()
    patch, cls, pos, gamma, beta = _assemble_inputs(2, 5, 192, seed=1)
    X = Guarded((10, 192), torch.float32)
    part = Guarded((10, 4, 2), torch.float32)
    with pytest.raises(E.GitmiError):
        E.op_vit_assemble(patch.cuda(), cls.cuda(), pos.cuda(), gamma.cuda(), beta.cuda(), 1e-5, X.t, 2, 5, part=part.t)
    assert _untouched(X.cpu()) and _untouched(part.cpu())


# ---- ragged front ----------------------------------------------------------------------------------------------------
RP, RNMAX, RMAXPIX = 16, 49, 96 * 128
RSLOT = 3 * RMAXPIX
# (64, 64), the second image, is the native-grid one at g = 4; (17, 17): 867 floats, a float4 tail of 3; (96, 128): 49 tokens
RAGGED_SHAPES = [(16, 16), (64, 64), (96, 128), (40, 52), (17, 17), (32, 130)]


def _desc_floats(B):
    return (B * 16 + 255) // 256 * 64


def _ragged_buffer(entries, shift):
    """entries: (h, w, image [3, h, w] or None, offset override or None) -> (device buffer view whose pointer is `shift` floats
    past a 16-byte boundary, the offsets used).  Every offset, the overridden ones too, lies inside the buffer."""
    B = len(entries)
    off = _desc_floats(B)
    desc, offs = [], []
    for h, w, im, over in entries:
        n = 0 if im is None else 3 * h * w
        o = off if over is None else over
        desc.append([h, w, o, 0])
        offs.append(o)
        off += (n + 3) // 4 * 4 + 8            # 8 spare floats: an offset moved by 2 still ends inside the buffer
    host = torch.zeros(off, dtype=torch.float32)
    host[:4 * B].view(torch.int32).copy_(torch.tensor(desc, dtype=torch.int32).reshape(-1))
    for (h, w, im, over), o in zip(entries, offs):
        if im is not None and over is None:
            host[o:o + 3 * h * w] = im.reshape(-1)
    dev = torch.empty(off + 4, device="cuda", dtype=torch.float32)
    view = dev[shift:shift + off]
    view.copy_(host)
    assert view.data_ptr() % 16 == 4 * shift
    return view, offs


def _ragged_images(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, h, w, generator=g) for h, w in shapes]


def _run_stage(entries, shift, Nmax=RNMAX):
    B = len(entries)
    src, _ = _ragged_buffer(entries, shift)
    slots, meta, ntok = Guarded((B, RSLOT), torch.float32), Guarded((B, 4), torch.int32), Guarded((B,), torch.int32)
    _E().op_ragged_front(0, B, RP, RMAXPIX, Nmax, src=src, slots=slots.t, meta=meta.t, ntok=ntok.t)
    return slots.cpu("stage slots"), meta.cpu("stage meta"), ntok.cpu("stage ntok")


def _check_staged(entries, valid, slots, meta, ntok):
    for b, (h, w, im, _) in enumerate(entries):
        if valid[b]:
            n = 3 * h * w
            assert torch.equal(_bits(slots[b, :n]), _bits(im.reshape(-1))), (b, "staged planes differ from the source")
            assert _untouched(slots[b, n:]), (b, "slot written past the image")
            assert meta[b].tolist() == [h, w, (h // RP) * (w // RP) + 1, 0] and ntok[b].item() == (h // RP) * (w // RP) + 1, b
        else:
            assert meta[b].tolist() == [0, 0, 1, 1] and ntok[b].item() == 1, (b, meta[b].tolist(), ntok[b].item())
            assert _untouched(slots[b]), (b, "slot of a rejected image was written")


@pytest.mark.parametrize("shift", [0, 1])
def test_ragged_stage_copies_planes_and_writes_meta(experiment_build, shift):
    """shift 0: the float4 form (16-byte aligned source and slots); shift 1: a source one float off selects the scalar form."""
    ims = _ragged_images(RAGGED_SHAPES, seed=5)
    entries = [(h, w, im, None) for (h, w), im in zip(RAGGED_SHAPES, ims)]
    slots, meta, ntok = _run_stage(entries, shift)
    _check_staged(entries, [True] * len(entries), slots, meta, ntok)


@pytest.mark.parametrize("shift", [0, 1])
def test_ragged_stage_rejects_bad_descriptors(experiment_build, shift):
    """One image per rejection rule between valid ones: meta {0, 0, 1, 1}, ntok 1, slot untouched, neighbours staged as usual.
    At p = 16, Nmax = 49, max_pixels = 96 x 128 = 48 patches no image can break the token rule alone (49 patches are 12544
    pixels), so the batch is staged again with Nmax = 40: the 49 tokens of (96, 128) then break that rule and no other."""
    shapes = [(40, 52), (15, 64), (64, 15), (96, 128), (97, 127), (32, 32), (32, 32), (17, 17)]
    ims = _ragged_images(shapes, seed=6)
    entries = [(h, w, im, None) for (h, w), im in zip(shapes, ims)]
    _, offs = _ragged_buffer(entries, 0)
    entries[5] = (32, 32, ims[5], offs[5] + 2)                       # offset not a multiple of 4
    entries[6] = (32, 32, ims[6], _desc_floats(len(shapes)) - 4)     # offset inside the descriptor block
    #          ok    h < p  w < p  ok     h w > max_pixels (6 x 7 patches)  off % 4  off in desc  ok
    valid = [True, False, False, True, False, False, False, True]
    assert 97 * 127 > RMAXPIX and (97 // RP) * (127 // RP) + 1 <= RNMAX
    slots, meta, ntok = _run_stage(entries, shift)
    _check_staged(entries, valid, slots, meta, ntok)
    valid[3] = False
    assert 96 * 128 <= RMAXPIX and (96 // RP) * (128 // RP) + 1 > 40
    slots, meta, ntok = _run_stage(entries, shift, Nmax=40)
    _check_staged(entries, valid, slots, meta, ntok)


def _host_meta(shapes, bad=()):
    m = [[0, 0, 1, 1] if b in bad else [h, w, (h // RP) * (w // RP) + 1, 0] for b, (h, w) in enumerate(shapes)]
    return torch.tensor(m, dtype=torch.int32)


@pytest.mark.parametrize("Kpad", [768, 832])
@pytest.mark.parametrize("out", ["f32", "op"])
def test_im2col_ragged_equals_im2col_per_image(experiment_build, out, Kpad):
    """Every image's patch rows are bit-equal to the uniform launcher's on that image alone; rows past its grid, the rows of a
    rejected image and the columns past K are exact zeros (the slots hold NaN behind every image)."""
    E = _E()
    dtype = torch.float32 if out == "f32" else _op_dtype()
    shapes = RAGGED_SHAPES + [(32, 32)]
    B = len(shapes)
    bad = {B - 1}
    ims = _ragged_images(shapes, seed=8)
    slots = torch.full((B, RSLOT), float("nan"))
    for b, im in enumerate(ims):
        slots[b, :im.numel()] = im.reshape(-1)
    meta = _host_meta(shapes, bad)
    patches = Guarded((B, RNMAX - 1, Kpad), dtype)
    E.op_ragged_front(1, B, RP, RMAXPIX, RNMAX, slots=slots.cuda(), meta=meta.cuda(), patches=patches.t, Kpad=Kpad)
    got = patches.cpu("im2col_ragged")
    for b, ((h, w), im) in enumerate(zip(shapes, ims)):
        n = 0 if b in bad else (h // RP) * (w // RP)
        if n:
            one = _run_im2col(im.cuda().contiguous(), 1, h, w, RP, Kpad, dtype)
            assert torch.equal(_bits(got[b, :n]), _bits(one)), (b, h, w)
            assert torch.count_nonzero(_bits(got[b, :n, 768:])) == 0
        assert torch.count_nonzero(_bits(got[b, n:])) == 0, (b, "rows past the grid are not zero")


@pytest.mark.parametrize("stream", ["f32", "f16"])
@pytest.mark.parametrize("D", [192, 768])
@pytest.mark.parametrize("g", [4, 1])
def test_vit_assemble_ragged_is_bit_equal_to_the_uniform_kernels(experiment_build, g, D, stream):
    """Valid rows (and, on the fp16 stream, their partials) of every image equal vit_assemble fed the pos_resize table of that
    image's grid bit for bit -- the stored table itself for a native-grid image ((64, 64) at g = 4; (16, 16) and (17, 17) at
    g = 1) and for the class row of a rejected one; padding rows and their partials are exact zeros over a NaN pre-fill."""
    E = _E()
    shapes = RAGGED_SHAPES + [(32, 32)]
    B = len(shapes)
    bad = {B - 1}
    meta = _host_meta(shapes, bad)
    gen = torch.Generator().manual_seed(17 * g + D)
    patch = torch.randn(B * (RNMAX - 1), D, generator=gen).cuda()
    cls = (torch.randn(D, generator=gen) * 1.5).cuda()
    pos = torch.randn(g * g + 1, D, generator=gen).cuda()
    gamma = (1 + 0.2 * torch.randn(D, generator=gen)).cuda()
    beta = (0.3 * torch.randn(D, generator=gen)).cuda()
    dt = torch.float32 if stream == "f32" else torch.float16
    X = Guarded((B * RNMAX, D), dt)
    X.t.fill_(float("nan"))
    part = Guarded((B * RNMAX, 4, 2), torch.float32) if stream == "f16" else None
    if part is not None:
        part.t.fill_(float("nan"))
    E.op_ragged_front(2, B, RP, RMAXPIX, RNMAX, meta=meta.cuda(), patch_out=patch, cls=cls, pos=pos, g=g, gamma=gamma, beta=beta,
                      eps=1e-5, X=X.t, part=None if part is None else part.t)
    got = X.cpu("vit_assemble_ragged X").reshape(B, RNMAX, D)
    gpart = None if part is None else part.cpu("vit_assemble_ragged partials").reshape(B, RNMAX, 4, 2)
    natives = 0
    for b, (h, w) in enumerate(shapes):
        gh, gw = (0, 0) if b in bad else (h // RP, w // RP)
        n = gh * gw + 1
        if b in bad or (gh, gw) == (g, g):
            table = pos
            natives += b not in bad
        else:
            tab = Guarded((n, D), torch.float32)
            E.op_pos_resize(pos, tab.t, g, gh, gw)
            tab.check("pos_resize")
            table = tab.t
        one = Guarded((n, D), dt)
        opart = Guarded((n, 4, 2), torch.float32) if part is not None else None
        E.op_vit_assemble(patch[b * (RNMAX - 1):], cls, table, gamma, beta, 1e-5, one.t, 1, n, part=None if opart is None else opart.t)
        assert torch.equal(_bits(got[b, :n]), _bits(one.cpu())), (b, h, w, "rows differ from the uniform kernels'")
        assert torch.count_nonzero(_bits(got[b, n:])) == 0, (b, "padding rows are not zero")
        if gpart is not None:
            assert torch.equal(_bits(gpart[b, :n]), _bits(opart.cpu())), (b, h, w, "partials differ from the uniform kernel's")
            assert torch.count_nonzero(_bits(gpart[b, n:])) == 0, (b, "partials of padding rows are not zero")
    assert natives >= 1


@pytest.mark.parametrize("dtype", ["f32", "op", "f16"])
def test_zero_pad_rows(experiment_build, dtype):
    """Rows at or past ntok become zeros whatever they held (NaN, inf); rows before it keep their bits."""
    E = _E()
    dt = {"f32": torch.float32, "op": _op_dtype(), "f16": torch.float16}[dtype]
    ntok = [1, 2, RNMAX - 1, RNMAX]
    B, ld = len(ntok), 192
    x = Guarded((B, RNMAX, ld), dt)
    fill = torch.randn(B, RNMAX, ld)
    fill[:, :, 0::3] = float("nan")
    fill[:, :, 1::3] = float("inf")
    fill[:, :, 2::6] = -float("inf")
    x.t.copy_(fill.to(dt))
    before = x.t.cpu()
    E.op_zero_pad_rows(x.t, torch.tensor(ntok, dtype=torch.int32).cuda(), B, RNMAX, ld)
    after = x.cpu("zero_pad_rows")
    for b, n in enumerate(ntok):
        assert torch.equal(_bits(after[b, :n]), _bits(before[b, :n])), (b, "rows before ntok changed")
        assert torch.count_nonzero(_bits(after[b, n:])) == 0, (b, "rows past ntok are not zero")


@pytest.mark.parametrize("dtype,ld", [("f32", 102), ("op", 100)])
def test_zero_pad_rows_refuses_rows_that_are_no_multiple_of_16_bytes(experiment_build, dtype, ld):
    E = _E()
    dt = torch.float32 if dtype == "f32" else _op_dtype()
    x = Guarded((2, 4, ld), dt)
    with pytest.raises(E.GitmiError):
        E.op_zero_pad_rows(x.t, torch.tensor([1, 2], dtype=torch.int32).cuda(), 2, 4, ld)
    assert _untouched(x.cpu())


# ---- ln_post scatter -------------------------------------------------------------------------------------------------
LNF, LNB, LNN = 3, 2, 5


def _ln_post_case(D, src, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(LNF * LNB * LNN, D, generator=g) * 2.0 + 0.5
    x = x.to(torch.float16) if src == "f16" else x
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.3 * torch.randn(D, generator=g)
    temb = torch.randn(LNF, D, generator=g)               # a vector of its own per frame
    return x, gamma, beta, temb


def _run_ln_post(D, src, mode, with_temb, temb_shift=0):
    """The F calls of encode_frames' ln_post loop: frame fr's rows x[fr B N ...] with the map (N, F N, fr N).  After every call
    the rows of the frames still to come must hold the sentinel.  -> (outputs by name, fp64 reference, fp32-evaluation bound)."""
    E = _E()
    op = _op_dtype()
    x, gamma, beta, temb = _ln_post_case(D, src, seed=D + len(mode))
    rows = LNB * LNN
    tbuf = torch.zeros(LNF, D + 4, device="cuda")
    tdev = tbuf[:, temb_shift:temb_shift + D]
    tdev.copy_(temb)
    outs = {}
    if mode in ("f32", "op"):
        outs["t"] = Guarded((LNB * LNF * LNN, D), torch.float32 if mode == "f32" else op)
    else:                                                   # both: the operand copy and the copy in the source's type
        outs["t"] = Guarded((LNB * LNF * LNN, D), op)
        outs["s"] = Guarded((LNB * LNF * LNN, D), x.dtype)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    for fr in range(LNF):
        add = tdev[fr] if with_temb else None
        if add is not None:
            assert add.data_ptr() % 16 == 4 * temb_shift
        E.op_layernorm_map(xd[fr * rows:], gd, bd, 1e-5, add, outs["t"].t, outs["s"].t if "s" in outs else None, rows, D,
                           LNN, LNF * LNN, fr * LNN)
        for name, o in outs.items():
            now = o.cpu(f"ln_post {name}").reshape(LNB, LNF, LNN, D)
            assert _untouched(now[:, fr + 1:]), (name, fr, "rows of a later frame were written")
            assert not _untouched(now[:, fr]), (name, fr)
    ref = torch.empty(LNB, LNF, LNN, D, dtype=torch.float64)
    bound = torch.empty_like(ref)
    for fr in range(LNF):
        # input row fr B N + b N + n -> output row b F N + fr N + n; the embedding is added AFTER gamma and beta
        y, bd_ = ln_ref_and_bound(x[fr * rows:(fr + 1) * rows], gamma, beta, 1e-5, temb[fr] if with_temb else None)
        ref[:, fr] = y.reshape(LNB, LNN, D)
        bound[:, fr] = bd_.reshape(LNB, LNN, D)
    got = {name: o.cpu().reshape(LNB, LNF, LNN, D) for name, o in outs.items()}
    return got, ref, bound


def _check_ln_post(got, ref, bound, what):
    for name, o in got.items():
        b = bound if o.dtype == torch.float32 else bound + _hulp(ref.abs() + bound, o.dtype)
        print(f"ln_post {what} {name} {o.dtype}: max err {(o.double() - ref).abs().max().item():.3e} max bound {b.max().item():.3e}")
        _assert_within(o, ref, b, f"ln_post {what} {name}")


@pytest.mark.parametrize("with_temb", [True, False])
@pytest.mark.parametrize("mode", ["f32", "op", "both"])
@pytest.mark.parametrize("src", ["f32", "f16"])
@pytest.mark.parametrize("D", [768, 1024, 192])
def test_ln_post_scatter(experiment_build, D, src, mode, with_temb):
    """F = 3, B = 2, N = 5.  D = 768 / 1024 with a 16-bit operand output run the wide kernel, D = 192 and every fp32 output the
    one-wave-per-row kernel; src f16: the fp16 residual stream (layernorm_kernel<*, f16_t>, layernorm_wide_kernel<f16_t, *>).
    Bound: the fp32 LayerNorm evaluation (ln_ref_and_bound), + half an ulp of a 16-bit output."""
    got, ref, bound = _run_ln_post(D, src, mode, with_temb)
    _check_ln_post(got, ref, bound, f"D={D} src={src} {mode} temb={with_temb}")


@pytest.mark.parametrize("src", ["f32", "f16"])
@pytest.mark.parametrize("D", [768, 1024])
def test_ln_post_with_an_unaligned_embedding_falls_back_and_stays_correct(experiment_build, D, src):
    """add_after one float past a 16-byte boundary: the wide kernel's 16-byte loads do not apply, the launcher falls back to the
    one-wave-per-row kernel; same bound."""
    for mode in ("op", "both"):
        got, ref, bound = _run_ln_post(D, src, mode, True, temb_shift=1)
        _check_ln_post(got, ref, bound, f"unaligned D={D} src={src} {mode}")


on_both_operand_builds(globals(), BUILD)
