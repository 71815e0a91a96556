"""Huffman decode of baseline JPEG scans on the GPU (csrc/kernels_jpeg_entropy.hip) through the C ABI
(generativeimage2text_amd/jpeg.py): scan records -> coefficient records, byte for byte what the host decoder
(jpeg.entropy_decode, pinned against Pillow by tests/test_jpeg_host.py) writes.  No tolerance anywhere."""
import base64
import io
import os
import subprocess

import numpy as np
import pytest
import torch

from tools import jpeg_cases as JC
from tools import jpeg_scan_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256


def _run(cases):
    """one gitmi_jpeg_entropy_batch call on [(name, scan record)]: every buffer pre-filled with 0xAA, guard bytes behind
    every coefficient record, the status array and the workspace.  -> (records, status list, guards intact)"""
    from generativeimage2text_amd import jpeg as J
    recs = [r for _, r in cases]
    host, offs = J.pack_records(recs)
    scan_desc = [(o, len(r)) for o, r in zip(offs, recs)]
    desc, total = [], 0
    for r in recs:
        b = J.scan_coef_bytes(r)
        desc.append((total, b))
        total += (b + GUARD + 127) // 128 * 128
    n = len(recs)
    need = J.entropy_workspace_bytes(scan_desc)
    coef = torch.full((total,), 0xAA, dtype=torch.uint8, device="cuda")
    work = torch.full((need + GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 16,), -0x55555556, dtype=torch.int32, device="cuda")         # 0xAAAAAAAA
    J.entropy_batch_to(coef, desc, torch.from_numpy(host).cuda(), scan_desc, status, workspace=work[:need])
    flat, st = coef.cpu().numpy(), status.cpu().numpy()
    intact = bool((st[n:] == -0x55555556).all()) and bool((work[need:] == 0xAA).all().item())
    out = []
    for i, (o, b) in enumerate(desc):
        out.append(flat[o: o + b])
        end = desc[i + 1][0] if i + 1 < n else total
        intact = intact and bool((flat[o + b: end] == 0xAA).all())
    return out, [int(v) for v in st[:n]], intact


def _prepared(cases):
    """[(name, JPEG bytes)] -> [(name, scan record, the host decoder's record)]"""
    from generativeimage2text_amd import jpeg as J
    out = []
    for name, data in cases:
        rec, ref = J.scan_prepare(data), J.entropy_decode(data)
        assert rec is not None and ref is not None, name
        out.append((name, rec, ref))
    return out


@pytest.fixture(scope="module")
def sweep():
    """the 800 cases of the sweep without restart markers, prepared and decoded on the host once"""
    return _prepared([c for c in JC.sweep() if "restart" not in c[0]])


@pytest.fixture(scope="module")
def singles(sweep):
    """one image per call: {name: record}"""
    out = {}
    for name, rec, _ in sweep:
        got, st, intact = _run([(name, rec)])
        assert st == [0] and intact, name
        out[name] = got[0]
    return out


def test_one_image_per_call_is_byte_equal(sweep, singles):
    assert len(sweep) == 800
    for name, _, ref in sweep:
        assert np.array_equal(singles[name], ref), name


@pytest.mark.parametrize("quality", JC.QUALITIES)
def test_batches_of_up_to_64_in_mixed_order(sweep, singles, quality):
    cases = [c for c in sweep if "-q%d-" % quality in c[0]]
    assert len(cases) == 200
    order = np.random.RandomState(quality).permutation(len(cases))
    for lo in range(0, len(cases), 64):
        part = [cases[i] for i in order[lo: lo + 64]]
        got, st, intact = _run([(name, rec) for name, rec, _ in part])
        assert intact, "guard bytes were written"
        assert st == [0] * len(part), [(c[0], s) for c, s in zip(part, st) if s]
        for (name, _, ref), g in zip(part, got):
            assert np.array_equal(g, ref), name


@pytest.mark.parametrize("n", [1, 65])
def test_batch_counts_around_the_launch_group(sweep, n):
    cases = sweep[3::len(sweep) // 65][:n]              # mixed sizes and modes; 65 = one past the 64 images of a launch group
    assert len(cases) == n
    got, st, intact = _run([(name, rec) for name, rec, _ in cases])
    assert intact and st == [0] * n
    for (name, _, ref), g in zip(cases, got):
        assert np.array_equal(g, ref), name


def test_cases_the_sweep_lacks():
    """scans shorter than a subsequence, ending on and one byte behind a subsequence boundary, more subsequences than a
    workgroup takes per pass, periodic streams (one subsequence per round, hundreds of blocks in a subsequence), 16-bit codes:
    one by one and as one batch"""
    cases = _prepared(SC.extra())
    solo = []
    for name, rec, ref in cases:
        got, st, intact = _run([(name, rec)])
        assert st == [0] and intact, (name, st)
        assert np.array_equal(got[0], ref), name
        solo.append(got[0])
    got, st, intact = _run([(name, rec) for name, rec, _ in cases[::-1]])
    assert intact and st == [0] * len(cases)
    for g, s in zip(got, solo[::-1]):
        assert np.array_equal(g, s)


@pytest.fixture(scope="module")
def broken(tmp_path_factory):
    """<= 64 truncations and corruptions of the scans of three files, each of which the CPU emulation of the kernels has just
    passed under the sanitizers (tools/probe/jpeg_entropy_gpu_check.cc --list): [(file index, JPEG bytes, host status)]"""
    tmp = tmp_path_factory.mktemp("broken")
    exe = SC.build_check_program(ROOT, str(tmp))
    files = _broken_files()
    paths = []
    for name, data in files:
        paths.append(str(tmp / (name + ".jpg")))
        with open(paths[-1], "wb") as f:
            f.write(data)
    res = subprocess.run([exe, "emulate", "--list", "32"] + paths, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0 and "no report" in res.stdout and "ERROR" not in res.stdout, res.stdout[-4000:]
    out = []
    for line in res.stdout.splitlines():
        if not line.startswith("case "):
            continue
        _, fi, kind, at, value, host = line.split()
        data = files[int(fi)][1]
        if kind == "cut":
            scan0 = len(data) - 2 - _scan_length(data)
            bad = data[: scan0 + int(at)] + b"\xff\xd9"
        else:
            bad = bytearray(data)
            bad[int(at)] = int(value)
            bad = bytes(bad)
        out.append((int(fi), bad, int(host)))
    return out


def _broken_files():
    files = SC.sanitizer_files()
    return [files[0], files[1], files[3]]               # 4:2:0, 4:4:4 and grey: the three with the shortest scans


def _scan_length(data: bytes) -> int:
    i = 2
    while True:
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        i += 2 + length
        if marker == 0xDA:
            return len(data) - 2 - i


def test_verdict_parity_on_broken_scans(broken):
    """status != 0 exactly where the host library declines; a byte-equal record where it does not; guards intact; the clean
    images of the same batch are what they are alone"""
    from generativeimage2text_amd import jpeg as J
    clean = _prepared(_broken_files())
    for fi in range(3):
        mine = [(bad, host) for f, bad, host in broken if f == fi]
        assert 8 <= len(mine) <= 64
        cases, expect = [], []
        for k, (bad, host) in enumerate(mine):
            rec = J.scan_prepare(bad)
            if rec is None:                             # the corruption made a marker: declined on the host already
                assert host == J.UNSUPPORTED
                continue
            cases.append(("broken%d" % k, rec))
            expect.append(J.entropy_decode(bad))
            assert (expect[-1] is not None) == (host == J.OK)
        assert any(e is None for e in expect)
        batch = [(clean[0][0], clean[0][1])] + cases + [(clean[fi][0], clean[fi][1])]
        got, st, intact = _run(batch)
        assert intact
        assert st[0] == 0 and st[-1] == 0
        assert np.array_equal(got[0], clean[0][2]) and np.array_equal(got[-1], clean[fi][2])
        for (name, _), g, s, ref in zip(cases, got[1:-1], st[1:-1], expect):
            assert (s == 0) == (ref is not None), (fi, name, s)
            if ref is not None:
                assert np.array_equal(g, ref), (fi, name)


def test_bad_arguments_are_refused_and_nothing_is_written():
    from generativeimage2text_amd import jpeg as J
    (name, rec, ref), = _prepared([("x", JC.encode(JC.content("noise", 33, 17), 2, 75))])
    host, offs = J.pack_records([rec])
    scans = torch.from_numpy(host).cuda()
    coef = torch.full((1 << 16,), 0xAA, dtype=torch.uint8, device="cuda")
    status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    b = len(ref)
    with pytest.raises(J.JpegError):                                    # the output is too small
        J.entropy_batch_to(coef[:b - 128], [(0, b)], scans, [(0, len(rec))], status)
    with pytest.raises(J.JpegError):                                    # an output offset outside the buffer
        J.entropy_batch_to(coef, [(coef.numel(), b)], scans, [(0, len(rec))], status)
    with pytest.raises(J.JpegError):                                    # a scan offset outside the buffer
        J.entropy_batch_to(coef, [(0, b)], scans, [(scans.numel(), len(rec))], status)
    with pytest.raises(J.JpegError):                                    # a scan record longer than the buffer
        J.entropy_batch_to(coef, [(0, b)], scans, [(0, scans.numel() + 128)], status)
    torch.cuda.synchronize()
    assert bool((coef == 0xAA).all()) and status.tolist() == [7, 7, 7, 7]
    J.entropy_batch_to(coef, [(0, b + 128)], scans, [(0, len(rec))], status)         # a size that disagrees with the record
    assert status.tolist() == [1, 7, 7, 7] and bool((coef == 0xAA).all())
    bad = host.copy()
    bad[J.HEADER_BYTES + 20: J.HEADER_BYTES + 24] = np.frombuffer(np.uint32(1 << 20).tobytes(), dtype=np.uint8)   # scan_bytes
    status.fill_(7)
    J.entropy_batch_to(coef, [(0, b)], torch.from_numpy(bad).cuda(), [(0, len(rec))], status)
    assert status.tolist() == [1, 7, 7, 7] and bool((coef == 0xAA).all())
    bad = host.copy()
    bad[40 + 16: 40 + 24] = 0xFF                                        # plane offset of component 0 far outside the record
    status.fill_(7)
    J.entropy_batch_to(coef, [(0, b)], torch.from_numpy(bad).cuda(), [(0, len(rec))], status)
    assert status.tolist() == [1, 7, 7, 7] and bool((coef == 0xAA).all())
    status.fill_(7)
    J.entropy_batch_to(coef, [(0, b)], scans, [(0, len(rec))], status)  # and the record as it is
    assert status.tolist() == [0, 7, 7, 7] and np.array_equal(coef[:b].cpu().numpy(), ref)


def _photo_jpegs():
    return [JC.encode(JC.content("photo", w, h, seed=20 + i), mode, 85)
            for i, (mode, w, h) in enumerate([(2, 300, 230), (0, 301, 237), (1, 299, 244), ("L", 310, 251), (2, 224, 258)])]


def test_reconstruction_of_the_gpu_decoded_records_is_pillows_rgb():
    from generativeimage2text_amd import jpeg as J
    datas = _photo_jpegs()
    records, status = J.decode_scans([J.scan_prepare(d) for d in datas])
    assert status.tolist() == [0] * 5
    packed = records[0]._base if records[0]._base is not None else records[0]
    refs = [JC.pillow_rgb(d) for d in datas]
    desc, total = [], 0
    for r in refs:
        desc.append((total, r.shape[0], r.shape[1]))
        total += (r.size + 63) // 64 * 64
    rgb = torch.zeros(total, dtype=torch.uint8, device="cuda")
    J.decode_batch_to(rgb, desc, packed, [int(r.storage_offset()) for r in records])
    flat = rgb.cpu().numpy()
    for (o, h, w), ref, d in zip(desc, refs, datas):
        assert np.array_equal(flat[o: o + ref.size].reshape(h, w, 3), ref)


def test_task_end_to_end_gpu_entropy(tmp_path, monkeypatch):
    """test_git_inference_single_tsv(gpu_jpeg="entropy"), and the same through GIT_DECODE_JPEG=gpu_entropy, writes byte for
    byte the TSV of the default path"""
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

    ims = [Image.fromarray(JC.content("photo", 300, 230 + 7 * i, seed=40 + i)) for i in range(7)]
    rows = [["j420", b64(ims[0], format="JPEG", quality=85, subsampling=2)],
            ["j444", b64(ims[1], format="JPEG", quality=85, subsampling=0)],
            ["restart", b64(ims[6], format="JPEG", quality=85, restart_marker_blocks=5)],
            ["prog", b64(ims[2], format="JPEG", quality=85, progressive=True)],
            ["j422", b64(ims[3], format="JPEG", quality=85, subsampling=1)],
            ["corrupt", base64.b64encode(SC.corrupted_photo()).decode()],
            ["png", b64(ims[4], format="PNG")],
            ["grey", b64(ims[5].convert("L"), format="JPEG", quality=85)]]
    tsv_io.tsv_writer(rows, str(tmp_path / "in.tsv"))
    monkeypatch.setattr(I, "get_tokenizer", lambda: I.IdTokenizer())
    real_build = I.build_model
    monkeypatch.setattr(I, "build_model", lambda name, tok, c, **kw: real_build(
        name, tok, c, decoder=AutoRegressiveBeamSearch(eos_index=102, max_steps=10, beam_size=1, per_node_beam_size=1,
                                                       fix_missing_prefix=True), **kw))
    monkeypatch.setenv("GIT_DECODE_PROCS", "4")
    outs = {}
    for mode, ask, env in (("host", {}, "host"), ("argument", dict(gpu_jpeg="entropy"), "host"), ("environment", {}, "gpu_entropy")):
        st = {}
        out = str(tmp_path / (mode + ".tsv"))
        monkeypatch.setenv("GIT_DECODE_JPEG", env)
        I.test_git_inference_single_tsv(str(tmp_path / "in.tsv"), "GIT_BASE", None, out, checkpoint=w, stats=st, batch_size=4,
                                        precision="f32", **ask)
        assert st["images"] == 8
        if mode == "host":
            assert "jpeg_entropy_gpu" not in st and "jpeg_gpu" not in st
        else:
            assert (st["jpeg_entropy_gpu"], st["jpeg_entropy_rejected"], st["jpeg_entropy_host"]) == (4, 1, 1), st
            assert (st["jpeg_gpu"], st["jpeg_fallback"]) == (5, 3), st
        outs[mode] = open(out, "rb").read()
    assert [r[0] for r in tsv_io.tsv_reader(str(tmp_path / "host.tsv"))] == [r[0] for r in rows]
    assert outs["argument"] == outs["host"] and outs["environment"] == outs["host"]
