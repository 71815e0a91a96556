"""GPU: every launch form of the decode attention (csrc/kernels_attn_decode.hip, the fp32 kernel of csrc/kernels_attn.hip)
against fp64 torch, through the measurement build's hook gitmi_debug_attn_decode_form (include/gitmi_experiment.h): an
argument check + the launcher the engine's decode step calls, with the fields gitmi_op_attn_decode cannot set -- pairs per
workgroup, fragment-major output, the sentence -> image indirection, per-image key counts.

Forms: fp32 (VALU kernel) | 16-bit two waves per pair | 16-bit one wave per pair packed 1 / 2 / 4 / 8 pairs per workgroup |
16-bit streaming on 1 / 2 / 96 workgroups.  Within a case every packing and every streaming launch must equal pairs_per_wg = 1
bit for bit (the kernel's promise, gitmi_set_shared_device rests on it); every form is held to fp64.

Every launch here also checks, bit for bit: guard rows behind `out` and both text caches keep their sentinel; position `pos` of
both caches holds this step's K / V of every row and head; no other element of the caches moved.

Bounds: fp32 3e-5 (test_attention_decode); fp16 build _attn_bound + _check16 (tests/test_gpu_ops_f16.py, with its tightness
assertion); bf16 build 3e-2 where the values are N(0, 1) (test_attention_decode), and for the shifted / spiked inputs of the
key-count and softmax edge cases twice the error of a torch emulation of the documented arithmetic (_bf16_emulated)."""
import functools

import pytest
import torch

from test_gpu_dgemm_forms import on_both_operand_builds
from test_gpu_ops_f16 import _attn_bound, _check16, _decode_ref

pytestmark = pytest.mark.gpu

GUARD = 3                # sentinel rows behind `out` and the caches
# Queries of the plain (and shifted) cases are N(0, 2.5^2), values N(0, 1).  At test_attention_decode's 1.2 the softmax over
# 40+ keys is flat enough that max |ref| sits one binade lower while single elements keep their bound, and _check16's tightness
# assertion (largest bound < half a bf16 ulp of the reference) fails on 5 of the plain inputs below and on 3 of the key-count
# edges (32 shifted, 128, 257); at 2.5 it holds on every input of this file (computed on the CPU from the reference alone).
Q_SCALE = 2.5


# Every test of the file runs on the bf16 measurement build under its own name and, as <name>_f16, on the fp16 one
# (on_both_operand_builds, last line): 16-bit tensors pick their library by type, the fp32 cases run in BUILD's (operands=).
BUILD = {"ops": "bf16"}


def _op_dtype():
    return {"bf16": torch.bfloat16, "f16": torch.float16}[BUILD["ops"]]


TWO = ("two waves", dict(waves_per_pair=2))
PACKED = [(f"packed {pw}", dict(waves_per_pair=1, pairs_per_wg=pw)) for pw in (1, 2, 4, 8)]
STREAM = [(f"stream {w}", dict(stream_wgs=w)) for w in (1, 2, 96)]
ONE_WAVE = PACKED + STREAM      # PACKED[0] is what the others must equal bit for bit


def _raw(t):
    """the elements as integers: bitwise comparisons that NaNs and signed zeros cannot blur"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _sentinel(rows, cols, dtype):
    n = torch.full((rows, cols), 0x7b7b7b7b if dtype == torch.float32 else 0x7b7b, dtype=torch.int32)
    return n.view(torch.float32) if dtype == torch.float32 else n.to(torch.int16).view(dtype)


class Case:
    """Inputs of one launch geometry in `dtype` (drawn in fp32, rounded once) and their fp64 reference, computed once."""

    def __init__(self, dtype, B, H, N_img, pos, beams, T=None, seed=0, img_of=None, n_images=None, ntok=None, permute=True,
                 q_shared=False, q_scale=1.2):
        # q_scale: 1.2 in test_attention_decode; the plain cases here take Q_SCALE
        self.dtype, self.B, self.H, self.N_img, self.pos, self.beams = dtype, B, H, N_img, pos, beams
        self.T = T if T is not None else pos + 3
        self.img_of, self.ntok = img_of, ntok
        self.bound_bf16 = None        # None: 3e-2 (N(0, 1) values)
        d, R, nI = H * 64, B * beams, n_images or B
        self.d, self.R = d, R
        g = torch.Generator().manual_seed(1000 + seed)
        qkv = torch.randn(R, 3 * d, generator=g) * 1.2
        qkv[:, :d] *= q_scale / 1.2
        if q_shared:                # the beams of a sentence ask nearly the same question: image keys can be aimed at all of them
            q0 = torch.randn(B, 1, d, generator=g) * q_scale
            qkv[:, :d] = (q0 + 0.05 * torch.randn(B, beams, d, generator=g)).reshape(R, d)
        self.qkv = qkv
        # every image from a seed of its own: a sentence that reads another image's K/V misses by O(1)
        self.ik = torch.stack([torch.randn(H, N_img, 64, generator=torch.Generator().manual_seed(7000 + 13 * seed + i)) for i in range(nI)])
        self.iv = torch.stack([torch.randn(H, N_img, 64, generator=torch.Generator().manual_seed(9000 + 13 * seed + i)) for i in range(nI)])
        if ntok is not None:        # padding keys hold garbage that must not leak in
            for i, n in enumerate(ntok):
                self.ik[i, :, n:] = 1e4
                self.iv[i, :, n:] = 1e4
        self.tk = torch.randn(R, self.T, d, generator=g)
        self.tv = torch.randn(R, self.T, d, generator=g)
        # kv_src: per position a permutation of the sentence's beam rows (one beam: the row itself, the kernels do not read it)
        if permute and beams > 1:
            perm = torch.stack([torch.stack([torch.randperm(beams, generator=g) for _ in range(self.T)], 1) for _ in range(B)])
            self.src = (perm + (torch.arange(B) * beams)[:, None, None]).reshape(R, self.T).int()
        else:
            self.src = torch.arange(R)[:, None].expand(R, self.T).contiguous().int()

    def finish(self):
        """round to the dtype, compute the reference and the bounds"""
        dt = self.dtype
        for n in ("qkv", "ik", "iv", "tk", "tv"):
            setattr(self, n, getattr(self, n).to(dt))
        q, K, V, o = _decode_ref(self.qkv, self.ik, self.iv, self.tk, self.tv, self.src, self.B, self.H, self.pos, self.beams,
                                 self.img_of, self.ntok)
        self.ref = o.reshape(self.R, self.d)
        self.q, self.K, self.V = q, K, V
        if dt == torch.float16:
            self.bound16 = self._bound_f16(q, K, V, o)
        return self

    def _bound_f16(self, q, K, V, o):
        if self.ntok is None:
            return _attn_bound(q, K, V, o).reshape(self.R, self.d)
        # per-image key counts: the bound of every row over the keys it really has
        img = torch.as_tensor(self.img_of if self.img_of is not None else range(self.B)).long().repeat_interleave(self.beams)
        bound = torch.empty(self.R, self.H, 1, 64, dtype=torch.float64)
        for i, n in enumerate(self.ntok):
            rows = (img == i).nonzero()[:, 0]
            if rows.numel():
                keys = torch.cat([torch.arange(n), torch.arange(self.N_img, K.shape[2])])
                bound[rows] = _attn_bound(q[rows], K[rows][:, :, keys], V[rows][:, :, keys], o[rows])
        return bound.reshape(self.R, self.d)

    def image_of_row(self):
        img = torch.arange(self.R) // self.beams
        return img if self.img_of is None else torch.as_tensor(self.img_of).long()[img]


def _bf16_emulated(c):
    """The documented arithmetic of the bf16 kernels in plain torch: scores and exponentials in fp32, P rounded to bf16 before
    P V, fp32 sums, the output rounded once.  -> its largest error against the fp64 reference (what bf16 costs on THESE inputs)."""
    q, K, V = c.q.float(), c.K.float(), c.V.float()
    s = (q * 0.125) @ K.transpose(-1, -2)
    if c.ntok is not None:
        pad = torch.arange(c.N_img)[None, :] >= torch.as_tensor(c.ntok).long()[c.image_of_row()][:, None]
        s[..., :c.N_img] = s[..., :c.N_img].masked_fill(pad[:, None, None, :], float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = ((p.bfloat16().float() @ V) / p.sum(-1, keepdim=True)).bfloat16()
    return (o.double().reshape(c.R, c.d) - c.ref).abs().max().item()


RATIOS = {}              # (form family, dtype) -> worst error / bound seen (printed: docs/LAB_NOTEBOOK.md quotes them)


def _check(c, out, what):
    """out (row-major, CPU) against the case's fp64 reference within the dtype's bound"""
    err = (out.double() - c.ref).abs()
    assert torch.isfinite(err).all(), (what, "non-finite output")
    if c.dtype == torch.float16:
        ratio = (err / c.bound16).max().item()
    else:
        bound = 3e-5 if c.dtype == torch.float32 else c.bound_bf16 if c.bound_bf16 is not None else 3e-2
        ratio = err.max().item() / bound
    key = (what.split()[0], str(c.dtype).split(".")[1])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"RATIO {key[0]} {key[1]} {ratio:.4f} worst so far {RATIOS[key]:.4f}")
    if c.dtype == torch.float16:
        _check16(out, c.ref, c.bound16, what)
    else:
        assert ratio <= 1.0, (what, "error / bound", ratio, "max error", err.max().item())


def _run(c, form=None, out_frag=False, txt=None, ntok=None):
    """One launch on guarded buffers -> (out on the CPU without its guard rows, (txt_k, txt_v) after the call).  form: keyword
    arguments of op_attn_decode_form (None: the fp32 kernel's only form).  txt: (txt_k, txt_v) to use instead of the case's;
    ntok: key counts the case itself does not have (the output is then not the reference's)."""
    from generativeimage2text_amd import engine as E
    dt, R, d, T = c.dtype, c.R, c.d, c.T
    rows_out = (R + 15) // 16 * 16 if out_frag else R
    out = _sentinel(rows_out + (16 if out_frag else GUARD), d, dt).cuda()
    tk0, tv0 = txt if txt is not None else (c.tk, c.tv)
    caches = []
    for t0 in (tk0, tv0):
        buf = _sentinel(R + GUARD, T * d, dt)
        buf[:R] = t0.reshape(R, T * d)
        caches.append(buf.cuda())
    before = [b.cpu() for b in caches]
    E.op_attn_decode_form(c.qkv.cuda(), c.ik.cuda(), c.iv.cuda(), caches[0], caches[1], c.src.cuda(), c.B, c.H, c.N_img, T, c.pos,
                          c.beams, out=out, img_of=c.img_of, ntok=ntok if ntok is not None else c.ntok, out_frag=out_frag,
                          operands=BUILD["ops"], **(form or {}))
    torch.cuda.synchronize()
    out = out.cpu()
    sent = _raw(_sentinel(1, d, dt))
    assert (_raw(out[rows_out:]) == sent).all(), "guard rows behind out were written"
    after = [b.cpu() for b in caches]
    for name, b4, aft, col in (("txt_k", before[0], after[0], d), ("txt_v", before[1], after[1], 2 * d)):
        assert (_raw(aft[R:]) == _raw(b4[R:])).all(), f"guard rows behind {name} were written"
        want = b4[:R].reshape(R, T, d).clone()
        want[:, c.pos] = c.qkv[:, col:col + d]
        bad = (_raw(aft[:R].reshape(R, T, d)) != _raw(want)).nonzero()
        assert bad.numel() == 0, (name, "first wrong (row, position, column)", bad[0].tolist(), "of", bad.shape[0])
    return out[:rows_out], tuple(a[:R].reshape(R, T, d) for a in after)


def _run_forms(c, forms, base=None):
    """every form of `forms` equal to the first one (or to `base`) bit for bit; -> the first form's output"""
    for name, kw in forms:
        out, _ = _run(c, kw)
        if base is None:
            base = out
        else:
            assert torch.equal(_raw(out), _raw(base)), (name, "differs from", forms[0][0],
                                                        (out.double() - base.double()).abs().max().item())
    return base


@functools.lru_cache(maxsize=4)
def _plain_case(dtype, B, H, N_img, pos, beams, T=None, seed=0, img_of=None, n_images=None, ntok=None, permute=True, q_scale=Q_SCALE):
    return Case(dtype, B, H, N_img, pos, beams, T=T, seed=seed, img_of=img_of, n_images=n_images, ntok=ntok, permute=permute,
                q_scale=q_scale).finish()


# ---- (a) the serving form: 8 pairs per workgroup, 772 pairs -> 97 workgroups, the last with 4 absent pairs ----------------
@pytest.mark.parametrize("beams", [1, 2])
def test_serving_form(experiment_build, beams):
    """What the engine launches under gitmi_set_shared_device: pairs_per_wg = 8, waves_per_pair by geometry, fragment-major
    rows.  Every packing, the fragment-major twin and the streaming form equal one pair per workgroup bit for bit."""
    from generativeimage2text_amd.engine import from_frag
    c = _plain_case(_op_dtype(), 193, 4, 40, 2, beams, seed=beams)
    packings = [(f"packed {pw}", dict(pairs_per_wg=pw)) for pw in (1, 8, 4, 2)]
    one = _run_forms(c, packings + STREAM)
    _check(c, one, "packed (serving)")
    frag, _ = _run(c, dict(pairs_per_wg=8), out_frag=True)
    assert torch.equal(_raw(from_frag(frag, c.R)), _raw(one)), "pairs_per_wg = 8, fragment-major rows"


# ---- (b) eight beam rows (KB = 8) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 5])
@pytest.mark.parametrize("beams", [5, 8])
def test_eight_beam_rows(experiment_build, beams, pos):
    """beams 5..8 run the KB = 8 instantiations: packed (386 pairs: 193 / 97 workgroups, the last of 4 with 2 absent pairs)
    and streaming (ring of 8 slots) at 40 keys, two waves at 300 keys, fp32 at both."""
    dt = _op_dtype()
    c = _plain_case(dt, 193, 2, 40, pos, beams, seed=20 + beams + pos)
    _check(c, _run_forms(c, ONE_WAVE), "packed / stream")
    c = _plain_case(dt, 2, 2, 300, pos, beams, seed=30 + beams + pos)
    _check(c, _run(c, TWO[1])[0], "two waves")
    for N_img in (40, 300):
        c = _plain_case(torch.float32, 2, 2, N_img, pos, beams, seed=40 + beams + pos)
        _check(c, _run(c)[0], "fp32")


def test_eight_beams_pack_four_pairs(experiment_build):
    """772 pairs of 8 beams asked for 8 pairs per workgroup: the launcher's rule packs 4 (KB = 8 needs the registers)"""
    c = _plain_case(_op_dtype(), 193, 4, 40, 0, 8, seed=50)
    four = _run_forms(c, [PACKED[2], PACKED[3]])
    _check(c, four, "packed 4 (asked 8)")


# ---- (c) sentence -> image indirection ------------------------------------------------------------------------------------
IMG_OF = (1, 0, 1, 1, 0)


@pytest.mark.parametrize("beams", [1, 3])
def test_img_of(experiment_build, beams):
    """5 sentences on 2 images (drawn from different seeds), every form"""
    dt = _op_dtype()
    c = _plain_case(dt, 5, 2, 40, 2, beams, seed=60 + beams, img_of=IMG_OF, n_images=2)
    _check(c, _run_forms(c, ONE_WAVE), "packed / stream")
    _check(c, _run(c, TWO[1])[0], "two waves")
    c = _plain_case(torch.float32, 5, 2, 40, 2, beams, seed=60 + beams, img_of=IMG_OF, n_images=2)
    _check(c, _run(c)[0], "fp32")


@pytest.mark.parametrize("ntok", [(40, 23), (40, 1)])
@pytest.mark.parametrize("beams", [1, 3])
def test_img_of_with_key_counts(experiment_build, beams, ntok):
    """... with per-image key counts: sentences on image 1 see 23 keys, or 1 (the second wave has no image step); the
    counts are indexed by image, not by sentence.  The streaming form is refused."""
    from generativeimage2text_amd import engine as E
    for dt, form in ((torch.float32, None), (_op_dtype(), dict(TWO[1]))):
        c = _plain_case(dt, 5, 2, 40, 2, beams, seed=70 + beams, img_of=IMG_OF, n_images=2, ntok=ntok)
        _check(c, _run(c, form)[0], "fp32" if form is None else "two waves (ragged)")
    with pytest.raises(E.GitmiError, match="ragged"):
        _run(c, dict(stream_wgs=2))


def test_refusals(experiment_build):
    """argument errors are answered with an error, before any launch"""
    from generativeimage2text_amd import engine as E
    c = _plain_case(torch.float32, 2, 2, 40, 2, 2, seed=80)
    with pytest.raises(E.GitmiError, match="out_frag"):
        _run(c, out_frag=True)
    with pytest.raises(ValueError, match="img_of"):
        E.op_attn_decode_form(c.qkv.cuda(), c.ik.cuda(), c.iv.cuda(), c.tk.cuda(), c.tv.cuda(), c.src.cuda(), 2, 2, 40, c.T, 2, 2,
                              img_of=[0, 2])
    lib = E._exp_library(_op_dtype())
    buf = torch.zeros(1 << 16, device="cuda")
    p, s, f32 = buf.data_ptr(), E._stream(), E.DTYPE_F32

    def call(ptrs=(p,) * 7, n_images=1, beams=1):
        return lib.gitmi_debug_attn_decode_form(*ptrs, None, None, n_images, 1, 1, 16, 8, 0, beams, f32, 0, 0, 0, 0, s)
    for i in range(7):
        with pytest.raises(E.GitmiError, match="null"):
            E._ck(call(ptrs=tuple(None if j == i else p for j in range(7))), lib)
    for kw, msg in ((dict(beams=0), "beams"), (dict(beams=9), "beams"), (dict(n_images=0), "n_images")):
        with pytest.raises(E.GitmiError, match=msg):
            E._ck(call(**kw), lib)
    torch.cuda.synchronize()
    assert buf.abs().sum().item() == 0


# ---- (d) the text-cache contract ------------------------------------------------------------------------------------------
def _distinct(n, dtype, seed):
    """n distinct values of magnitude <= 2 -- 16-bit: distinct raw codes (no zero; finite in both encodings)"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return (torch.randperm(1 << 20, generator=g)[:n].float() - (1 << 19)) * 2.0 ** -18
    codes = torch.arange(1, 0x4001, dtype=torch.int32)
    codes = torch.cat([codes, codes + 0x8000])
    assert n <= codes.numel()
    return codes[torch.randperm(codes.numel(), generator=g)[:n]].to(torch.int16).view(dtype)


@pytest.mark.parametrize("slack", [0, 2])
@pytest.mark.parametrize("beams", [1, 3, 8])
def test_text_cache_append(experiment_build, beams, slack):
    """Caches pre-filled with distinct values (T_max == pos + 1 and beyond): after every form, ragged included, position pos
    holds this step's K / V of every row and head bit for bit and every other element is what it was (_run asserts both)."""
    B, H, pos = 3, 2, 2
    for dt in (torch.float32, _op_dtype()):
        c = _plain_case(dt, B, H, 40, pos, beams, T=pos + 1 + slack, seed=90 + beams)
        n = c.R * c.T * c.d
        fill = _distinct(2 * n, dt, seed=beams + slack)
        txt = (fill[:n].reshape(c.R, c.T, c.d), fill[n:].reshape(c.R, c.T, c.d))
        forms = [None] if dt == torch.float32 else [kw for _, kw in [TWO] + ONE_WAVE]
        for kw in forms:
            _run(c, kw, txt=txt)
            if kw is None or kw.get("waves_per_pair") == 2:             # the ragged instantiations
                _run(c, kw, txt=txt, ntok=(40, 7, 33))


# ---- (e) fragment-major output ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,beams", [(5, 1), (7, 3), (12, 4)])             # R = 5, 21, 48
def test_out_frag(experiment_build, B, beams):
    """from_frag(out)[:R] equals the row-major output of the same form bit for bit; write_rows stores rows row0 + j, j < beams
    only, so rows R .. round_up(R, 16) of the fragment buffer keep their sentinel (as do the guard rows, _run)."""
    from generativeimage2text_amd.engine import from_frag
    dt = _op_dtype()
    sent = _raw(_sentinel(1, 1, dt))
    for N_img, forms in ((40, [PACKED[0], PACKED[3], STREAM[1]]), (300, [TWO])):
        c = _plain_case(dt, B, 2, N_img, 2, beams, seed=110 + B)
        for name, kw in forms:
            rows, _ = _run(c, kw)
            frag, _ = _run(c, kw, out_frag=True)
            full = from_frag(frag, frag.shape[0])
            assert torch.equal(_raw(full[:c.R]), _raw(rows)), name
            assert (_raw(full[c.R:]) == sent).all(), (name, "rows past R of the fragment buffer were written")
            _check(c, rows, name)


# ---- (f) the up-front / tail boundary of the text items -------------------------------------------------------------------
@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("beams,pos,two_wave", [(4, 5, False), (5, 4, False), (8, 0, False), (8, 5, True), (7, 6, True), (8, 0, True)])
def test_text_item_boundary(experiment_build, beams, pos, two_wave, permute):
    """beams * (pos + 1) text items against the 24 (one wave, streaming) / 48 (two waves) loaded up front: 24 | 25, 48 | 49
    -- the last up-front item, the first item of the dependent-load tail -- and 8"""
    if two_wave:
        c = _plain_case(_op_dtype(), 2, 2, 300, pos, beams, seed=120 + beams, permute=permute)
        _check(c, _run(c, TWO[1])[0], "two waves")
    else:
        c = _plain_case(_op_dtype(), 2, 2, 40, pos, beams, seed=120 + beams, permute=permute)
        _check(c, _run_forms(c, ONE_WAVE), "packed / stream")


# ---- (g) key-count edges ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _negative_case(dtype, N_img):
    """every true score around -20: an unmasked zero padding key (score 0) would take nearly all the weight.  Keys = -160 q0 /
    |q0|^2 + N(0, 1) against queries q0 + 0.05 N(0, 1) per (sentence, head)."""
    B, H, pos, beams = 2, 2, 2, 2
    c = Case(dtype, B, H, N_img, pos, beams, seed=200 + N_img, q_shared=True, q_scale=Q_SCALE)
    d = c.d
    q0 = c.qkv[:, :d].reshape(B, beams, H, 64).mean(1)                        # [B, H, 64]
    base = -160.0 * q0 / (q0 * q0).sum(-1, keepdim=True)
    c.ik += base[:, :, None, :]
    per_row = base.repeat_interleave(beams, 0).reshape(c.R, d)
    c.tk += per_row[:, None, :]
    c.qkv[:, d:2 * d] += per_row
    c.finish()
    s = (c.q @ c.K.transpose(-1, -2) / 8.0)
    assert -30 < s.min().item() and s.max().item() < -10, (s.min().item(), s.max().item())
    if dtype == torch.bfloat16:
        c.bound_bf16 = 2 * _bf16_emulated(c)
    return c


# fp16 build: _check16's tightness assertion holds on all fourteen inputs (closest: 1.921e-3 < 1.953e-3).
# bf16 against fp64 on the shifted inputs (_bf16_emulated; the bound is twice this), N_img 1 .. 257:
#   1: 7.55e-03  32: 4.19e-03  33: 5.07e-03  128: 3.29e-03  129: 2.53e-03  256: 4.21e-03  257: 3.41e-03
# (the plain inputs, held to 3e-2: 7.20e-03  3.28e-03  5.71e-03  3.86e-03  2.69e-03  3.81e-03  4.05e-03)
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("N_img", [1, 32, 33, 128, 129, 256, 257])
def test_key_count_edges(experiment_build, N_img, negative):
    """One 32-key step, the step edges, the one-wave chunk (128 keys), the one- / two-wave switch (N_pad <= 256): waves per pair
    by geometry, 1 and 2 forced; the streaming form where the engine may choose it (N_pad <= 256); fp32"""
    for dt in (torch.float32, _op_dtype()):
        c = _negative_case(dt, N_img) if negative else _plain_case(dt, 2, 2, N_img, 2, 2, seed=130 + N_img)
        if dt == torch.float32:
            _check(c, _run(c)[0], "fp32")
            continue
        one = _run(c, dict(waves_per_pair=1))[0]
        two = _run(c, dict(waves_per_pair=2))[0]
        _check(c, one, "packed 1")
        _check(c, two, "two waves")
        auto = _run(c, dict(waves_per_pair=0))[0]
        assert torch.equal(_raw(auto), _raw(one if N_img <= 256 else two)), "the geometry's choice"
        if N_img <= 256:
            assert torch.equal(_raw(_run(c, STREAM[1][1])[0]), _raw(one)), "stream 2"


# ---- (h) softmax edges ------------------------------------------------------------------------------------------------------
SPIKES = ["last", "odd", "even", "text_front", "text_tail", "new", "both"]


@functools.lru_cache(maxsize=4)
def _spiked_case(dtype, two_wave, where):
    """One key (two for "both") whose score is about 40 above the rest: the key 320 q / |q|^2.
    Image spikes aim at all beams of a sentence (queries q0 + 0.05 N(0, 1)); text spikes at each row's own query.
      one wave, 197 keys (7 steps, chunks 0-3 | 4-6), 2 beams, pos 14: 30 text items, 24 up front
      two waves, 300 keys (10 steps: even | odd, chunks of 4 each), 4 beams, pos 14: 60 text items, 48 up front
    last: the last key (the last step: the second chunk, a late jump of the running max) | odd / even: key 40 (step 1) / 70
    (step 2): the max in one wave's half only | text_front: position 3 / 1, an up-front item for every beam | text_tail: position
    12 / 10, in the tail for the last beam | new: the new position | both: key 70 and text position 3 / 1, the same key vector."""
    B, H, pos = 2, 2, 14
    N_img, beams = (300, 4) if two_wave else (197, 2)
    c = Case(dtype, B, H, N_img, pos, beams, seed=300 + SPIKES.index(where), q_shared=True)
    d, R = c.d, c.R
    qr = c.qkv[:, :d].reshape(R, H, 64)
    q0 = qr.reshape(B, beams, H, 64).mean(1)
    img_spike = 320.0 * q0 / (q0 * q0).sum(-1, keepdim=True)                  # [B, H, 64]
    row_spike = (320.0 * qr / (qr * qr).sum(-1, keepdim=True)).reshape(R, d)
    if where == "both":
        row_spike = img_spike.repeat_interleave(beams, 0).reshape(R, d)       # equal scores: the same vector in both parts
    key = {"last": N_img - 1, "odd": 40, "even": 70, "both": 70}.get(where)
    if key is not None:
        c.ik[:, :, key] = img_spike
    s_txt = {"text_front": 1 if two_wave else 3, "text_tail": 10 if two_wave else 12, "both": 1 if two_wave else 3}.get(where)
    if s_txt is not None:
        up_front = 48 if two_wave else 24
        items = torch.arange(beams) * (pos + 1) + s_txt
        assert (items >= up_front).any() if where == "text_tail" else (items < up_front).all()
        c.tk[c.src[:, s_txt].long(), s_txt] = row_spike                      # src is a permutation per position: no row is hit twice
    if where == "new":
        c.qkv[:, d:2 * d] = row_spike
    c.finish()
    s = c.q @ c.K.transpose(-1, -2) / 8.0
    top = s.topk(3, -1).values[..., 0, :]
    gap = top[..., 1] - top[..., 2] if where == "both" else top[..., 0] - top[..., 1]
    assert gap.min().item() > 30, gap.min().item()
    if where == "both":
        assert (top[..., 0] - top[..., 1]).max().item() < 0.6
    if dtype == torch.bfloat16:
        c.bound_bf16 = 2 * _bf16_emulated(c)
    return c


# bf16 against fp64 on the spiked inputs (_bf16_emulated; the bound is twice this): a lone spike leaves the softmax one-hot and
# the output IS the spike's value row, already a bf16 number -- the emulation's error is what the other keys weigh, e^-38
#   one wave : last 5.77e-15  odd 7.99e-15  even 6.22e-15  text_front 6.66e-15  text_tail 7.55e-15  new 8.44e-15  both 3.91e-03
#   two waves: last 8.44e-15  odd 2.09e-14  even 9.77e-15  text_front 1.20e-14  text_tail 8.88e-15  new 9.77e-15  both 7.81e-03
# fp16 build: _check16's tightness assertion holds on all fourteen inputs (bounds 1.08e-3 .. 1.14e-3 against 3.9e-3).
@pytest.mark.parametrize("where", SPIKES)
@pytest.mark.parametrize("two_wave", [False, True])
def test_softmax_edges(experiment_build, two_wave, where):
    """The running max jumps late, sits in one wave's half, in the text part (the image partial is folded in with a factor of
    e^-40), at the new position, or twice with equal scores"""
    dt = _op_dtype()
    c = _spiked_case(dt, two_wave, where)
    if two_wave:
        _check(c, _run(c, TWO[1])[0], "two waves")
    else:
        _check(c, _run_forms(c, ONE_WAVE), "packed / stream")
    c = _spiked_case(torch.float32, two_wave, where)
    _check(c, _run(c)[0], "fp32")


on_both_operand_builds(globals(), BUILD)
