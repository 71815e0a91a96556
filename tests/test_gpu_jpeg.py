"""GPU half of the split JPEG decode (csrc/kernels_jpeg.hip) through the C ABI (generativeimage2text_amd/jpeg.py): bit-exact
against Pillow's Image.open(...).convert("RGB") over the sweep of tools/jpeg_cases.py, the batch form, the hand-over to the
existing transform, and the TSV task end to end."""
import base64
import io

import numpy as np
import pytest
import torch

from tools import jpeg_cases as JC

pytestmark = pytest.mark.gpu


def _first_diff(got, ref):
    if got.shape != ref.shape:
        return "shape %s != %s" % (got.shape, ref.shape)
    d = np.argwhere(got != ref)
    return None if not len(d) else "%d bytes differ, first at (y, x, c) = %s: %d != %d" % (
        len(d), tuple(d[0]), got[tuple(d[0])], ref[tuple(d[0])])


@pytest.fixture(scope="module")
def sweep():
    """[(name, record, Pillow's RGB)] of every case, computed once"""
    from generativeimage2text_amd import jpeg as J
    out = []
    for name, data in JC.sweep():
        rec = J.entropy_decode(data)
        assert rec is not None, name
        out.append((name, rec, JC.pillow_rgb(data)))
    return out


@pytest.fixture(scope="module")
def singles(sweep):
    """one image per call: {name: uint8 [H, W, 3] on the host}"""
    from generativeimage2text_amd import jpeg as J
    outs = [(name, J.reconstruct_batch([rec])[0]) for name, rec, _ in sweep]
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in outs}


def test_reconstruction_is_bit_exact_one_image_per_call(sweep, singles):
    assert len(sweep) == 864
    for name, _, ref in sweep:
        diff = _first_diff(singles[name], ref)
        assert diff is None, "%s: %s" % (name, diff)


def _batch_with_guards(cases, guard=256):
    """gitmi_jpeg_reconstruct_batch on buffers pre-filled with 0xAA, guard bytes after every image; -> (images, guards intact)"""
    from generativeimage2text_amd import jpeg as J
    host, offs = J.pack_records([rec for _, rec, _ in cases])
    desc, total = [], 0
    for _, rec, _ in cases:
        h, w = J.record_size(rec)
        desc.append((total, h, w))
        total += (h * w * 3 + guard + 63) // 64 * 64
    rgb = torch.full((total,), 0xAA, dtype=torch.uint8, device="cuda")
    J.decode_batch_to(rgb, desc, torch.from_numpy(host).cuda(), offs)
    flat = rgb.cpu().numpy()
    imgs, intact = [], True
    for i, (o, h, w) in enumerate(desc):
        imgs.append(flat[o: o + h * w * 3].reshape(h, w, 3))
        end = desc[i + 1][0] if i + 1 < len(desc) else total
        intact = intact and bool((flat[o + h * w * 3: end] == 0xAA).all())
    return imgs, intact


@pytest.mark.parametrize("quality", JC.QUALITIES)
def test_batch_form_mixed_sizes_and_modes(sweep, singles, quality):
    cases = [c for c in sweep if "-q%d-" % quality in c[0]]
    assert len(cases) == 216
    for order in (cases, cases[::-1]):
        imgs, intact = _batch_with_guards(order)
        assert intact, "guard bytes behind an image were written"
        for (name, _, ref), got in zip(order, imgs):
            assert _first_diff(got, ref) is None, "%s: %s" % (name, _first_diff(got, ref))
            assert np.array_equal(got, singles[name]), name


@pytest.mark.parametrize("n", [1, 25])
def test_batch_form_small_counts(sweep, singles, n):
    cases = sweep[5::len(sweep) // 25][:n]            # mixed sizes and modes; 25 = one past the transform's 24-image launch group
    assert len(cases) == n
    imgs, intact = _batch_with_guards(cases)
    assert intact
    for (name, _, ref), got in zip(cases, imgs):
        assert _first_diff(got, ref) is None, "%s: %s" % (name, _first_diff(got, ref))
        assert np.array_equal(got, singles[name]), name


def test_bad_records_and_arguments_are_refused():
    from generativeimage2text_amd import jpeg as J
    rec = J.entropy_decode(JC.encode(JC.content("noise", 33, 17), 2, 75))
    host, offs = J.pack_records([rec])
    coef = torch.from_numpy(host).cuda()
    rgb = torch.full((4096,), 0xAA, dtype=torch.uint8, device="cuda")
    with pytest.raises(J.JpegError):                                    # the output does not fit
        J.decode_batch_to(rgb[:100], [(0, 17, 33)], coef, offs)
    with pytest.raises(J.JpegError):                                    # a record offset outside the buffer
        J.decode_batch_to(rgb, [(0, 17, 33)], coef, [coef.numel()])
    J.decode_batch_to(rgb, [(0, 33, 17)], coef, offs)                   # H and W swapped: the record disagrees -> left unwritten
    bad = host.copy()
    bad[40 + 16: 40 + 24] = 0xFF                                        # plane offset of component 0 far outside the record
    J.decode_batch_to(rgb, [(2048, 17, 33)], torch.from_numpy(bad).cuda(), offs)
    assert bool((rgb == 0xAA).all())


def _photo_jpegs():
    from PIL import Image
    out = []
    for i, (mode, w, h) in enumerate([(2, 300, 230), (0, 301, 237), (1, 299, 244), ("L", 310, 251), (2, 224, 258)]):
        out.append(JC.encode(JC.content("photo", w, h, seed=20 + i), mode, 85))
    return out


def test_into_the_transform():
    """gitmi_preprocess_batch on the reconstructed device buffer == on Pillow's RGB uploaded the old way"""
    from generativeimage2text_amd import jpeg as J
    from generativeimage2text_amd.engine import preprocess_batch
    datas = _photo_jpegs()
    recs = [J.entropy_decode(d) for d in datas]
    assert all(r is not None for r in recs)
    refs = [JC.pillow_rgb(d) for d in datas]
    desc, total = [], 0
    for r in refs:
        desc.append((total, r.shape[0], r.shape[1]))
        total += (r.size + 63) // 64 * 64
    old = torch.zeros(total, dtype=torch.uint8)
    for (o, h, w), r in zip(desc, refs):
        old[o: o + r.size] = torch.from_numpy(r.reshape(-1).copy())
    host, offs = J.pack_records(recs)
    new = torch.zeros(total, dtype=torch.uint8, device="cuda")
    J.decode_batch_to(new, desc, torch.from_numpy(host).cuda(), offs)
    a, b = preprocess_batch(new, desc, 224), preprocess_batch(old.cuda(), desc, 224)
    assert a.shape == (5, 3, 224, 224) and a.dtype == torch.float32
    assert torch.equal(a, b)


def test_task_end_to_end_gpu_jpeg(tmp_path, monkeypatch):
    """test_git_inference_single_tsv(gpu_jpeg=True) writes byte for byte the TSV of the default path"""
    from PIL import Image
    from oracle import git_oracle as O
    from generativeimage2text_amd import inference as I, tsv_io
    from generativeimage2text_amd.model import AutoRegressiveBeamSearch
    cfg = O.CONFIGS["GIT_BASE"]
    w = O.make_weights(cfg, seed=1240, tie_output=False, eos_bias=0.3)

    def b64(img, **kw):
        buf = io.BytesIO()
        img.save(buf, **kw)
        return base64.b64encode(buf.getvalue()).decode()

    ims = [Image.fromarray(JC.content("photo", 300, 230 + 7 * i, seed=40 + i)) for i in range(6)]
    rows = [["j420", b64(ims[0], format="JPEG", quality=85, subsampling=2)],
            ["j444", b64(ims[1], format="JPEG", quality=85, subsampling=0)],
            ["prog", b64(ims[2], format="JPEG", quality=85, progressive=True)],
            ["j422", b64(ims[3], format="JPEG", quality=85, subsampling=1)],
            ["png", b64(ims[4], format="PNG")],
            ["grey", b64(ims[5].convert("L"), format="JPEG", quality=85)]]
    tsv_io.tsv_writer(rows, str(tmp_path / "in.tsv"))
    monkeypatch.setattr(I, "get_tokenizer", lambda: I.IdTokenizer())
    real_build = I.build_model
    monkeypatch.setattr(I, "build_model", lambda name, tok, c, **kw: real_build(
        name, tok, c, decoder=AutoRegressiveBeamSearch(eos_index=102, max_steps=10, beam_size=1, per_node_beam_size=1,
                                                       fix_missing_prefix=True), **kw))
    monkeypatch.setenv("GIT_DECODE_PROCS", "4")
    for tag, kw in (("f32", dict(batch_size=4, precision="f32")), ("f16", dict(contexts=4, batch_size=2))):
        outs = {}
        for mode in (False, True):
            st = {}
            out = str(tmp_path / ("%s_%d.tsv" % (tag, mode)))
            # asked for by the argument in the first round, by the environment variable in the second
            ask = dict(gpu_jpeg=mode) if tag == "f32" else {}
            monkeypatch.setenv("GIT_DECODE_JPEG", "gpu" if (mode and not ask) else "host")
            I.test_git_inference_single_tsv(str(tmp_path / "in.tsv"), "GIT_BASE", None, out, checkpoint=w, stats=st, **ask, **kw)
            assert st["images"] == 6
            if mode:
                assert st["jpeg_gpu"] == 4 and st["jpeg_fallback"] == 2
            else:
                assert "jpeg_gpu" not in st
            outs[mode] = open(out, "rb").read()
        assert [r[0] for r in tsv_io.tsv_reader(str(tmp_path / ("%s_1.tsv" % tag)))] == [r[0] for r in rows]
        assert outs[True] == outs[False], tag
