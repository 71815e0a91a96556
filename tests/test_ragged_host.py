"""Ragged image batches, host side (no GPU): the input buffer layout of include/gitmi.h, host-side shape checks, the
binding, and the TSV task's bucketing with and without mixed_shapes."""
import base64
import json

import pytest
import torch

from generativeimage2text_amd import engine, inference, tsv_io


def _imgs(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(3, h, w, generator=g) for h, w in shapes]


def test_pack_ragged_layout_and_alignment():
    shapes = [(480, 640), (17, 33), (64, 64), (16, 16), (96, 80)]
    imgs = _imgs(shapes)
    r = engine.pack_ragged(imgs, patch=16, max_pixels=480 * 640, max_tokens=1201, max_batch=8)
    assert isinstance(r, engine.RaggedImages) and len(r) == 5 and r.shapes == shapes
    buf = r.buffer
    assert buf.dtype == torch.float32 and buf.dim() == 1
    desc = buf[:4 * len(shapes)].view(torch.int32).reshape(-1, 4).tolist()
    first = (len(shapes) * 16 + 255) // 256 * 64                     # descriptor block padded to 256 bytes, in floats
    assert desc[0][2] == first
    end = first
    for (h, w, off, zero), (hh, ww), im in zip(desc, shapes, imgs):
        assert (h, w, zero) == (hh, ww, 0)
        assert off % 4 == 0 and off >= end                            # 16-byte aligned, no overlap
        assert torch.equal(buf[off:off + 3 * h * w], im.reshape(-1))
        end = off + 3 * h * w
    assert buf.numel() >= end
    # more than 16 images: the descriptor block spans two 256-byte units
    r = engine.pack_ragged(_imgs([(16, 16)] * 17), 16, 256, 2, 32)
    assert r.buffer[:4 * 17].view(torch.int32).reshape(-1, 4)[0, 2].item() == 128


@pytest.mark.parametrize("shape, msg", [((15, 64), "smaller than one"), ((64, 10), "smaller than one"),
                                        ((500, 640), "max_image_pixels"), ((16, 1000), "max_image_tokens")])
def test_pack_ragged_rejects_bad_shapes(shape, msg):
    imgs = _imgs([(64, 64), shape])
    with pytest.raises(ValueError, match=msg):
        engine.pack_ragged(imgs, patch=16, max_pixels=480 * 640, max_tokens=60, max_batch=8)


def test_pack_ragged_rejects_bad_batches():
    with pytest.raises(ValueError, match="max_batch"):
        engine.pack_ragged(_imgs([(32, 32)] * 3), 16, 4096, 17, 2)
    with pytest.raises(ValueError, match="max_batch"):
        engine.pack_ragged([], 16, 4096, 17, 2)
    with pytest.raises(ValueError, match=r"\[3, h, w\]"):
        engine.pack_ragged([torch.zeros(1, 3, 32, 32)], 16, 4096, 17, 2)
    with pytest.raises(ValueError, match=r"\[3, h, w\]"):
        engine.pack_ragged([torch.zeros(4, 32, 32)], 16, 4096, 17, 2)


def test_ragged_mode_goes_through_the_existing_entry_point():
    """no new export: ragged input is gitmi_set_image_shape(e, 0, 0); the declared signature takes it"""
    import ctypes as C
    assert "gitmi_set_image_shape" in engine.EXPORTED_SYMBOLS
    assert not any("ragged" in n for n in engine.EXPORTED_SYMBOLS)
    lib = engine.load_library("bf16")
    assert lib.gitmi_set_image_shape.argtypes == [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    assert lib.gitmi_abi_version() == 10
    header = open(engine.__file__.rsplit("/", 2)[0] + "/include/gitmi.h").read()
    assert "gitmi_set_image_shape(e, 0, 0" in header


def _run(tmp_path, mixed, sizes, questions_per_image):
    rows = [["key%d" % i, base64.b64encode(b"img-%02d" % i).decode()] for i in range(len(sizes))]
    tsv_io.tsv_writer(rows, str(tmp_path / "img.tsv"))
    q = [["key%d" % i, json.dumps([{"question": "q%d-%d" % (i, j), "question_id": 100 * i + j} for j in range(n)])]
         for i, n in enumerate(questions_per_image)]
    tsv_io.tsv_writer(q, str(tmp_path / "q.tsv"))
    calls = []

    class Done:
        def __init__(self, v):
            self.v = v

        def result(self):
            return self.v

    def submit_answers(imgs, qss):
        calls.append([tuple(im.shape) for im in imgs])
        return Done([["ans<%s|%s>" % (tuple(im.shape), qq) for qq in qs] for im, qs in zip(imgs, qss)])

    out = str(tmp_path / ("out_%d.tsv" % mixed))
    inference.run_tsv_inference(
        str(tmp_path / "img.tsv"), str(tmp_path / "q.tsv"), out,
        transform=lambda b: torch.zeros(3, *sizes[int(b.decode()[4:])]),
        caption_batch=None, answer_questions=None, batch_size=4, rank=0, world=1,
        submit_answers=submit_answers, max_questions=6, **({"mixed_shapes": True} if mixed else {}))
    return calls, open(out, "rb").read()


def test_tsv_bucketing_by_shape_unchanged_and_mixed_across_shapes(tmp_path):
    sizes = [(32, 48), (48, 32), (32, 48), (32, 32), (48, 32), (32, 48), (32, 32), (32, 48), (48, 48), (32, 48)]
    nq = [1, 2, 1, 3, 1, 2, 1, 1, 2, 1]
    calls, rows = _run(tmp_path, False, sizes, nq)
    assert all(len(set(c)) == 1 for c in calls)                        # default: one shape per call, as before
    assert sorted(s for c in calls for s in c) == sorted((3,) + s for s in sizes)
    calls_m, rows_m = _run(tmp_path, True, sizes, nq)
    assert rows_m == rows                                               # the same answer rows, in input order
    assert any(len(set(c)) > 1 for c in calls_m)                        # shapes mixed inside a call
    assert len(calls_m) < len(calls)
    for c in calls_m:
        assert len(c) <= 4                                              # batch_size images per call
