"""memory_pack_kernel / memory_unpack_kernel alone (kernels_memory.hip), through KEEP and RECALL on a TINY engine: the bytes of a
slot against the fp32 feature copy of gitmi_encode_frames, what a slot keeps of a store pre-filled with a byte pattern, and --
through the import hook of the measurement build, which copies a context's whole blocks -- the rows RECALL zeroes behind
every image and the key counts it writes."""
import pytest
import torch

from oracle import git_oracle as O

pytestmark = pytest.mark.gpu

PRECS = ("f32", "f16", "bf16")
DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
PATTERN = 0xA5


def _engine(cfg, w, precision, B, hw=None, T=10):
    from generativeimage2text_amd.engine import Engine
    eng = Engine(cfg, precision=precision, max_batch=B, max_beams=1, max_frames=1, max_text_len=T, max_image_hw=hw)
    eng.load_state_dict(w)
    return eng


def _tiny(seed=111):
    cfg = O.CONFIGS["TINY"]
    return cfg, O.make_weights(cfg, seed=seed, tie_output=False, successor=2.0, eos_bias=1.0)


def _planes(eng, slot, dtype):
    """a slot's bytes -> (header int32 [64], feature rows [cap, D], [K | V rows [cap, 2d]] per layer)"""
    c, cap, esz = eng.c, eng.memory_rows, torch.empty(0, dtype=dtype).element_size()
    off = 256
    feat = slot[off:off + cap * c.vit_width * esz].view(dtype).view(cap, c.vit_width)
    off += cap * c.vit_width * esz
    kv = []
    for _ in range(c.dec_layers):
        kv.append(slot[off:off + cap * 2 * c.dec_hidden * esz].view(dtype).view(cap, 2 * c.dec_hidden))
        off += cap * 2 * c.dec_hidden * esz
    assert off <= slot.numel() < off + 256
    return slot[:256].view(torch.int32), feat, kv, slot[off:]


def _bits(x):
    return x.contiguous().view(torch.int32 if x.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("precision", PRECS)
def test_pack_writes_the_header_and_exactly_the_valid_rows(precision):
    """A ragged batch (n = 13, 7 and 17 of 17 rows) kept into a store filled with 0xA5: the feature rows of every slot equal the
    rows of feats_out byte for byte (16-bit: feats_out rounded to the operand type, the value the engine stores), the K | V
    rows are written up to n, and every byte behind row n of every plane, the slot's tail and the slot that was not named still
    hold the pattern.  The KEEP follows gitmi_encode_frames alone: it runs the prefill itself."""
    from generativeimage2text_amd.engine import DTYPE_BF16, DTYPE_F16, DTYPE_F32
    cfg, w = _tiny()
    dtype = DTYPE[precision]
    gen = torch.Generator().manual_seed(7)
    images = [torch.randn(3, h, ww, generator=gen).cuda() for h, ww in ((48, 64), (32, 48), (64, 64))]
    ns = [13, 7, 17]
    eng = _engine(cfg, w, precision, 3, hw=(64, 64))
    feats = eng.encode(eng.ragged(images))                              # fp32 [3, 17, D], zeros past every image's rows
    store = eng.memory_store(4)
    store.fill_(PATTERN)
    kept = eng.keep(store, [2, 0, 3])                                   # slot 1 is not named
    assert kept["rows"] == ns and kept["max_rows"] == 17 and kept["total_rows"] == 37
    torch.cuda.synchronize()
    for b, slot_i in enumerate([2, 0, 3]):
        hdr, feat, kv, tail = _planes(eng, store[slot_i], dtype)
        n = ns[b]
        h, ww = images[b].shape[1:]
        code = {"f32": DTYPE_F32, "f16": DTYPE_F16, "bf16": DTYPE_BF16}[precision]
        assert hdr[:16].tolist() == [0x4d495447, 1, cfg.vit_width, cfg.dec_hidden, cfg.dec_layers, cfg.dec_heads, feat.element_size(),
                                     code, 17, n, n, 0, 1, h, ww, 0]
        assert not hdr[16:].any()
        assert torch.equal(_bits(feat[:n]), _bits(feats[b, :n].to(dtype))), (precision, b)
        assert (_bits(feat[n:]).view(torch.uint8) == PATTERN).all() and (tail == PATTERN).all()
        for l in range(cfg.dec_layers):
            assert torch.isfinite(kv[l][:n].float()).all() and kv[l][:n].float().abs().sum() > 0
            assert (_bits(kv[l][n:]).view(torch.uint8) == PATTERN).all()
    assert (store[1] == PATTERN).all()
    eng.close()


@pytest.mark.parametrize("precision", ("f32", "bf16"))      # the measurement build serves these two engine modes
def test_unpack_zeroes_the_padding_rows_and_writes_the_key_counts(precision, experiment_build):
    """Slots of 13, 7 and 17 rows are recalled into a context whose blocks (stride 17) hold the rows of an unrelated full-size
    batch.  A second context imports the whole blocks (gitmi_debug_import_stage copies B x stride rows of the features and of
    every layer's K/V) and keeps them as 17-row images: rows [0, n) are the kept bytes, rows [n, 17) are zeros, in every plane.
    The key counts: an attention map over the recalled batch is exactly 0 in the image columns >= n and not before."""
    cfg, w = _tiny(seed=112)
    dtype = DTYPE[precision]
    gen = torch.Generator().manual_seed(8)
    images = [torch.randn(3, h, ww, generator=gen).cuda() for h, ww in ((48, 64), (32, 48), (64, 64))]
    junk = [torch.randn(3, 64, 64, generator=gen).cuda() for _ in range(3)]
    ns = [13, 7, 17]
    eng = _engine(cfg, w, precision, 3, hw=(64, 64))
    eng.encode(eng.ragged(images), return_features=False)
    store = eng.memory_store(3)
    kept = eng.keep(store, [0, 1, 2])
    eng.encode(eng.ragged(junk), return_features=False)
    eng.prefill()                                                       # every row of every block now holds the junk batch
    info = eng.recall(store, [0, 1, 2], kept["geometry"])
    assert info == {"stride": 17, "max_rows": 17, "total_rows": 37}     # 32 rows would exceed the 17 the workspaces hold
    att = eng.attend(None, torch.tensor([[cfg.sos, 5, 6]] * 3)).cpu()   # [3, L, layers, 17 + L]
    for b, n in enumerate(ns):
        assert (att[b, :, :, n:17] == 0).all() and (att[b, :, :, :n] > 0).all(), (precision, b)
    blocks = eng.clone()
    blocks.debug_import_stage(eng, 2)
    whole = blocks.memory_store(3)
    whole.fill_(PATTERN)
    assert blocks.keep(whole, [0, 1, 2])["total_rows"] == 51
    torch.cuda.synchronize()
    for b, n in enumerate(ns):
        _, feat0, kv0, _ = _planes(eng, store[b], dtype)
        hdr, feat, kv, _ = _planes(blocks, whole[b], dtype)
        assert hdr[9].item() == 17
        assert torch.equal(_bits(feat[:n]), _bits(feat0[:n])) and not _bits(feat[n:]).any(), (precision, b)
        for l in range(cfg.dec_layers):
            assert torch.equal(_bits(kv[l][:n]), _bits(kv0[l][:n])) and not _bits(kv[l][n:]).any(), (precision, b, l)
    blocks.close()
    eng.close()
