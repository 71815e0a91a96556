"""Inputs of the GPU Huffman decode's tests (tests/test_jpeg_scan_host.py, tests/test_gpu_jpeg_entropy.py) beside the sweep of
tools/jpeg_cases.py: the smallest streams at which that decoder can go wrong.  Written by Pillow from seeded content; the
seeds were searched on the CPU with jpeg.scan_prepare and are frozen here (the tests assert what each was searched for)."""
from __future__ import annotations

from tools import jpeg_cases as JC

MULTIPLE_SEED, MULTIPLE_PLUS_ONE_SEED = 9, 12       # 24 x 24 noise, 4:2:0, quality 75: 384 and 385 unstuffed scan bytes
MANY_SIZE = 92                                      # 4:4:4 quality-100 noise: 37355 scan bytes = 292 subsequences of 1024 bits
# e2e: one byte of the scan of photo(300 x 272, seed 47) at 4:2:0 quality 85, counted from the EOI: scan_prepare takes the file,
# the host Huffman decode declines it, Pillow decodes it without raising
CORRUPT_SEED, CORRUPT_AT, CORRUPT_VALUE = 47, -1654, 192


def short():
    return [("1x1", JC.encode(JC.content("noise", 1, 1, seed=0), 2, 75)),
            ("8x8", JC.encode(JC.content("noise", 8, 8, seed=0), 2, 75))]


def boundary():
    return [("multiple", JC.encode(JC.content("noise", 24, 24, seed=MULTIPLE_SEED), 2, 75)),
            ("multiple+1", JC.encode(JC.content("noise", 24, 24, seed=MULTIPLE_PLUS_ONE_SEED), 2, 75))]


def many():
    return [("many", JC.encode(JC.content("noise", MANY_SIZE, MANY_SIZE, seed=5), 0, 100))]


def periodic():
    """a mis-started decoder need never fall into step on these: the chain moves one subsequence per round"""
    return [("%s-s%s" % (kind, mode), JC.encode(JC.content(kind, 320, 240), mode, 75))
            for kind in ("flat", "checker", "gradient") for mode in (2, "L")]


def long_codes():
    """optimize=True tables with 16-bit codes"""
    return [("codes16", JC.encode(JC.content("noise", 160, 120, seed=0), "L", 95, optimize=True))]


def extra():
    return short() + boundary() + many() + periodic() + long_codes()


def sanitizer_files():
    """the files of tests/test_jpeg_host.py: test_standalone_sanitizer_program without the restart one"""
    return [("base%d" % i, JC.encode(JC.content("noise", w, h, seed=i), mode, 75, **kw))
            for i, (mode, w, h, kw) in enumerate([(2, 33, 17, {}), (0, 17, 33, {}), (1, 64, 48, dict(optimize=True)), ("L", 15, 17, {})])]


def corrupted_photo() -> bytes:
    data = bytearray(JC.encode(JC.content("photo", 300, 272, seed=CORRUPT_SEED), 2, 85))
    data[data.rindex(b"\xff\xd9") + CORRUPT_AT] = CORRUPT_VALUE
    return bytes(data)


def longest_code(data: bytes) -> int:
    """the longest Huffman code any DHT segment in front of the scan defines"""
    i, longest = 2, 0
    while i + 4 <= len(data):
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        if marker == 0xC4:
            o = i + 4
            while o < i + 2 + length:
                counts = data[o + 1: o + 17]
                longest = max([longest] + [l + 1 for l in range(16) if counts[l]])
                o += 17 + sum(counts)
        if marker == 0xDA:
            break
        i += 2 + length
    return longest


def build_check_program(root: str, out_dir: str) -> str:
    """tools/probe/jpeg_entropy_gpu_check.cc + csrc/jpeg_entropy.cc as ONE ordinary program under
    -fsanitize=address,undefined; -> its path"""
    import os
    import shutil
    import subprocess
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(out_dir, "jpeg_entropy_gpu_check")
    base = [cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            os.path.join(root, "tools", "probe", "jpeg_entropy_gpu_check.cc"),
            os.path.join(root, "generativeimage2text_amd", "csrc", "jpeg_entropy.cc"), "-o", exe]
    if subprocess.run(base + ["-static-libasan", "-static-libubsan"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode:
        subprocess.run(base, check=True)
    return exe
