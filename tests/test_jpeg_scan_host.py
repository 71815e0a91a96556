"""The GPU Huffman decode of the split JPEG path (include/gitmi_jpeg.h), as far as a CPU reaches: gitmi_jpeg_scan_prepare
(libgitmi_jpeg_host.so), the kernels' per-thread bodies (csrc/jpeg_entropy_dev.h) run thread by thread by a stand-alone
sanitizer program, and the decode pool's jpeg="gpu_entropy" protocol."""
import base64
import io
import os
import subprocess

import numpy as np
import pytest

from generativeimage2text_amd import jpeg as J
from tools import jpeg_cases as JC
from tools import jpeg_oracle as O
from tools import jpeg_scan_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    return SC.build_check_program(ROOT, str(tmp_path_factory.mktemp("jpeg_entropy_gpu_check")))


def _segment(data: bytes) -> bytes:
    """the entropy-coded segment of a file written by Pillow: behind the SOS segment, in front of the EOI"""
    i = 2
    while True:
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        i += 2 + length
        if marker == 0xDA:
            return data[i: data.rindex(b"\xff\xd9")]


def test_scan_prepare_over_the_sweep():
    """OK on the 800 cases without restart markers, UNSUPPORTED on the 64 with; the header is the host decoder's; the scan
    bytes, stuffed again, are the file's segment"""
    ok = declined = 0
    for name, data in JC.sweep():
        rec = J.scan_prepare(data)
        if "restart" in name:
            assert rec is None, name
            declined += 1
            continue
        assert rec is not None, name
        ref = J.entropy_decode(data)
        assert np.array_equal(rec[:J.HEADER_BYTES], ref[:J.HEADER_BYTES]), name
        assert J.scan_coef_bytes(rec) == len(ref), name
        n = J.scan_bytes_of(rec)
        assert len(rec) % 16 == 0 and len(rec) >= J.SCAN_AT + n + 8 and not rec[J.SCAN_AT + n:].any(), name
        assert bytes(rec[J.SCAN_AT: J.SCAN_AT + n]).replace(b"\xff", b"\xff\x00") == _segment(data), name
        ok += 1
    assert (ok, declined) == (800, 64)


def test_scan_description():
    data = JC.encode(JC.content("noise", 33, 17), 2, 75)
    rec = J.scan_prepare(data)
    magic, size, ncomp, per_mcu, total, scan_bytes = np.frombuffer(bytes(rec[640:664]), dtype="<u4")
    offset, record_bytes = np.frombuffer(bytes(rec[664:680]), dtype="<u8")
    assert (magic, size, ncomp, per_mcu, total) == (0x31534A47, J.SCAN_STRUCT_BYTES, 3, 6, 3 * 2 * 6)
    assert offset == J.SCAN_AT == 2944 and record_bytes == len(rec) and scan_bytes == J.scan_bytes_of(rec)
    assert list(rec[680:683]) == [0, 1, 1] and list(rec[684:687]) == [0, 1, 1]                  # td, ta of Pillow's files
    dht = data[data.index(b"\xff\xc4") + 5:]
    assert bytes(rec[768: 768 + 16]) == dht[:16]                                                # DC table 0: its counts ...
    assert bytes(rec[768 + 16: 768 + 16 + sum(dht[:16])]) == dht[16: 16 + sum(dht[:16])]        # ... and its symbols
    assert not rec[768 + 2 * 272: 768 + 4 * 272].any()                                          # tables no component names
    assert J.load_host_library().gitmi_jpeg_abi_version() == 1


def test_scan_prepare_declines_what_the_entropy_decode_declines():
    """the inputs of test_jpeg_host.py: test_classification_everything_else_is_unsupported, and a restart interval"""
    from PIL import Image
    im = Image.fromarray(JC.content("noise", 64, 48, seed=3))

    def save(img, **kw):
        buf = io.BytesIO()
        img.save(buf, **kw)
        return buf.getvalue()

    good = save(im, format="JPEG", quality=75)
    assert J.scan_prepare(good) is not None
    eoi = good.rindex(b"\xff\xd9")
    cases = {
        "progressive": save(im, format="JPEG", quality=75, progressive=True),
        "cmyk": save(im.convert("CMYK"), format="JPEG", quality=75),
        "keep_rgb": save(im, format="JPEG", quality=75, keep_rgb=True),
        "png": save(im, format="PNG"),
        "empty": b"",
        "cut at 50 %": good[: len(good) // 2],
        "EOI removed": good[:eoi] + good[eoi + 2:],
        "restart interval": save(im, format="JPEG", quality=75, restart_marker_blocks=2),
        "a marker inside the scan": good[:eoi - 10] + b"\xff\xd0" + good[eoi - 10:],
    }
    for name, data in cases.items():
        out = np.zeros(1 << 17, dtype=np.uint64)
        rc, _, _ = J.scan_prepare_into(data, out.ctypes.data, out.nbytes)
        assert rc == J.UNSUPPORTED, name
        assert J.scan_prepare(data) is None, name
    assert J.entropy_decode(cases["restart interval"]) is not None      # ... which the host Huffman decode still takes


def test_scan_prepare_one_byte_short_is_no_space_and_writes_nothing():
    data = JC.encode(JC.content("noise", 33, 17), 2, 75)
    ref = J.scan_prepare(data)
    need, guard = len(ref), 64
    buf = np.full((need + guard + 7) // 8 * 8, 0xAA, dtype=np.uint8)
    assert buf.ctypes.data % 8 == 0
    rc, info, said = J.scan_prepare_into(data, buf.ctypes.data, need - 1)
    assert rc == J.NO_SPACE and said == need and (info.width, info.height) == (33, 17)
    assert info.record_bytes == len(J.entropy_decode(data))
    assert (buf == 0xAA).all()
    rc, _, _ = J.scan_prepare_into(data, buf.ctypes.data, need)            # an exact fit: the guard region stays
    assert rc == J.OK and (buf[need:] == 0xAA).all()
    assert np.array_equal(buf[:need], ref)


def test_the_extra_cases_are_what_they_were_searched_for():
    bits = J.SUBSEQUENCE_BITS
    sizes = {name: J.scan_bytes_of(J.scan_prepare(data)) for name, data in SC.extra()}
    assert sizes["1x1"] * 8 < bits and sizes["8x8"] * 8 < bits
    assert sizes["multiple"] % (bits // 8) == 0 and sizes["multiple+1"] % (bits // 8) == 1
    per_pass = J.WORKGROUP_THREADS * J.SUBSEQUENCES_PER_THREAD_PER_PASS
    assert (sizes["many"] * 8 + bits - 1) // bits > per_pass
    assert all((sizes[name] * 8 + bits - 1) // bits >= 8 for name, _ in SC.periodic())
    assert SC.longest_code(SC.long_codes()[0][1]) == 16
    bad = SC.corrupted_photo()
    assert J.scan_prepare(bad) is not None and J.entropy_decode(bad) is None
    assert JC.pillow_rgb(bad).shape == (272, 300, 3)


def test_the_corrupted_row_of_the_task_test_through_the_emulation(check_program, tmp_path):
    """the one broken scan tests/test_gpu_jpeg_entropy.py: test_task_end_to_end_gpu_entropy sends to the GPU: the kernels'
    source rejects it on the CPU, under the sanitizers, without a report"""
    src, dst = str(tmp_path / "corrupt.scan"), str(tmp_path / "corrupt.coef")
    J.scan_prepare(SC.corrupted_photo()).tofile(src)
    res = subprocess.run([check_program, "decode", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 4 and "status" in res.stdout, res.stdout[-2000:]
    assert "status 0" not in res.stdout and "ERROR" not in res.stdout and "runtime error" not in res.stdout, res.stdout[-2000:]
    assert not os.path.exists(dst)


def _run_all(cmds):
    """the commands side by side, one core each, as many at a time as there are cores (16 at the most); -> their outputs"""
    from concurrent.futures import ThreadPoolExecutor

    def one(cmd):
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        return res.stdout, res.returncode
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        return list(pool.map(one, cmds))


def test_kernel_source_on_the_cpu_under_the_sanitizers(check_program, tmp_path):
    """the kernels' per-thread bodies, thread by thread, on every file, EVERY truncation of its scan and 2 x 2000 corruptions:
    verdict OK exactly when the host decoder says OK, then a byte-equal record; exact-size heap buffers; exit 0 and no report.
    The work on one file is quadratic in its scan, so a long scan is shared out over several processes (--part I/N: the parts
    together are the whole set).  Then scan_prepare alone on truncations and corruptions of the whole file."""
    files, cmds, names = [], [], []
    for name, data in SC.sanitizer_files() + SC.extra():
        files.append(str(tmp_path / (name + ".jpg")))
        with open(files[-1], "wb") as f:
            f.write(data)
        parts = 1 if len(data) < 8192 else 4 if len(data) < 24576 else 12
        for i in range(parts):
            cmds.append([check_program, "emulate", "--part", "%d/%d" % (i, parts), files[-1]])
            names.append("%s %d/%d" % (name, i, parts))
    outs = _run_all(cmds[::-1] + [[check_program, "prepare"] + files])      # the longest first
    rounds = 0
    for f, (out, rc) in zip(names[::-1] + ["prepare"], outs):
        assert rc == 0, "%s: %s" % (f, out[-4000:])
        assert "no report" in out and "ERROR" not in out and "runtime error" not in out, "%s: %s" % (f, out[-4000:])
        if f != "prepare":
            rounds = max(rounds, int(out.split(" rounds")[0].split()[-1]))
    assert rounds >= 8          # the periodic streams made the round loop run: one subsequence per round


def test_pool_gpu_entropy_mode_slots_and_records(check_program, tmp_path):
    """DecodePool(jpeg="gpu_entropy") against the pool with jpeg="host" on the same rows: scan slots where scan_prepare takes
    the file, a coefficient slot for the restart-marker file, Pillow RGB for the rest; every scan slot through the CPU
    emulation of the kernels and the restatement of the reconstruction == the host pool's RGB of that row"""
    from PIL import Image
    from generativeimage2text_amd import decode_pool as DP, tsv_io
    im = Image.fromarray(JC.content("photo", 120, 90, seed=1))

    def b64(img, **kw):
        buf = io.BytesIO()
        img.save(buf, **kw)
        return base64.b64encode(buf.getvalue()).decode()

    rows = [["j420", b64(im, format="JPEG", quality=85, subsampling=2)],
            ["j444", b64(im, format="JPEG", quality=85, subsampling=0)],
            ["grey", b64(im.convert("L"), format="JPEG", quality=85)],
            ["restart", b64(im, format="JPEG", quality=85, restart_marker_blocks=3)],
            ["prog", b64(im, format="JPEG", quality=85, progressive=True)],
            ["png", b64(im, format="PNG")]]
    expect = [DP.SLOT_SCAN, DP.SLOT_SCAN, DP.SLOT_SCAN, DP.SLOT_COEF, DP.SLOT_RGB, DP.SLOT_RGB]
    assert DP.SLOT_SCAN == 2
    tsv = str(tmp_path / "in.tsv")
    tsv_io.tsv_writer(rows, tsv)

    def collect(mode):
        pool = DP.DecodePool(tsv, 2, slots=len(rows), slot_bytes=1 << 18, **({} if mode == "host" else {"jpeg": mode}))
        try:
            for i in range(len(rows)):
                pool.submit(i, i)
            out = {}
            for _ in rows:
                slot, row, key, h, w = pool.next_result(timeout=60)
                assert slot == row and key == rows[row][0] and (h, w) == (90, 120)
                if mode == "host":
                    out[row] = (None, pool.buffer[slot * pool.slot_bytes: slot * pool.slot_bytes + h * w * 3].copy())
                else:
                    kind, payload = pool.slot_payload(slot)
                    out[row] = (kind, payload.copy())
            return out
        finally:
            pool.close()

    host, gpu = collect("host"), collect("gpu_entropy")
    for i, row in enumerate(rows):
        ref = host[i][1].reshape(90, 120, 3)
        kind, payload = gpu[i]
        assert kind == expect[i], row[0]
        if kind == DP.SLOT_SCAN:
            src, dst = str(tmp_path / ("%d.scan" % i)), str(tmp_path / ("%d.coef" % i))
            payload.tofile(src)
            res = subprocess.run([check_program, "decode", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert res.returncode == 0 and "ERROR" not in res.stdout, res.stdout[-2000:]
            payload = np.fromfile(dst, dtype=np.uint8)
            assert np.array_equal(payload, J.entropy_decode(base64.b64decode(row[1]))), row[0]
        got = payload.reshape(90, 120, 3) if kind == DP.SLOT_RGB else O.reconstruct(payload)
        assert np.array_equal(got, ref), row[0]
    with pytest.raises(ValueError):
        DP.DecodePool(tsv, 1, slots=1, jpeg="device")
