"""ctypes bindings of the split JPEG decode (include/gitmi_jpeg.h).

  libgitmi_jpeg_host.so   entropy (Huffman) decode on the host: JPEG bytes -> coefficient record; or scan_prepare: JPEG bytes
                          -> scan record (header, tables, unstuffed scan bytes) whose Huffman decode the GPU runs.  No GPU, no
                          torch: decode-pool workers import this module and load only this library.
  libgitmi_jpeg.so        reconstruction on the GPU (HIP, gfx950): records -> uint8 [H, W, 3], bit for bit Pillow's
                          Image.open(...).convert("RGB"); entropy_batch_to: scan records -> coefficient records, byte for
                          byte the host decoder's.

Both are independent of libgitmi*.so (engine.load_library / EXPORTED_SYMBOLS are untouched).  A missing library is an error for
whoever asks for it by name; nothing here falls back to another decoder -- the CALLER decodes with Pillow what
entropy_decode() declines (None), so Pillow stays the sole judge of broken and exotic files.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libgitmi_jpeg_host.so")
GPU_LIB_PATH = os.path.join(_HERE, "libgitmi_jpeg.so")

ABI_VERSION = 1
HEADER_BYTES = 640
OK, UNSUPPORTED, NO_SPACE, BAD_ARGUMENT = 0, 1, 2, 3
SCAN_STRUCT_BYTES = 2304
SCAN_AT = HEADER_BYTES + SCAN_STRUCT_BYTES          # the unstuffed scan bytes of a scan record begin here
HOST_SYMBOLS = ["gitmi_jpeg_abi_version", "gitmi_jpeg_entropy_decode", "gitmi_jpeg_scan_prepare"]
GPU_SYMBOLS = ["gitmi_jpeg_abi_version", "gitmi_jpeg_reconstruct_batch", "gitmi_jpeg_workspace_bytes", "gitmi_jpeg_last_error",
               "gitmi_jpeg_entropy_batch", "gitmi_jpeg_entropy_workspace_bytes", "gitmi_jpeg_entropy_constant"]
# compile-time constants of the GPU Huffman decode (csrc/jpeg_entropy_dev.h; gitmi_jpeg_entropy_constant reports the library's)
SUBSEQUENCE_BITS = 1024
WORKGROUP_THREADS = 256
SUBSEQUENCES_PER_THREAD_PER_PASS = 1    # by definition: thread t walks subsequences t, t + WORKGROUP_THREADS, ... one per pass


class JpegError(RuntimeError):
    pass


class JpegInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("ncomp", C.c_uint32), ("h_samp", C.c_uint32),
                ("v_samp", C.c_uint32), ("reserved", C.c_uint32), ("record_bytes", C.c_uint64)]


_host = None
_gpu = None


def _open(path: str, what: str) -> C.CDLL:
    if not os.path.exists(path):
        raise JpegError(f"{path} not found ({what}): build it with `make -C generativeimage2text_amd/csrc` "
                        f"or `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    lib.gitmi_jpeg_abi_version.restype = C.c_int
    if lib.gitmi_jpeg_abi_version() != ABI_VERSION:
        raise JpegError(f"{path}: ABI {lib.gitmi_jpeg_abi_version()}, this module speaks {ABI_VERSION}")
    return lib


def load_host_library() -> C.CDLL:
    global _host
    if _host is None:
        lib = _open(HOST_LIB_PATH, "host half of the JPEG decode")
        lib.gitmi_jpeg_entropy_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(JpegInfo)]
        lib.gitmi_jpeg_entropy_decode.restype = C.c_int
        lib.gitmi_jpeg_scan_prepare.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(JpegInfo),
                                                C.POINTER(C.c_uint64)]
        lib.gitmi_jpeg_scan_prepare.restype = C.c_int
        _host = lib
    return _host


def load_gpu_library() -> C.CDLL:
    global _gpu
    if _gpu is None:
        lib = _open(GPU_LIB_PATH, "GPU half of the JPEG decode")
        i64p = C.POINTER(C.c_int64)
        lib.gitmi_jpeg_reconstruct_batch.argtypes = [C.c_void_p, C.c_size_t, i64p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                                     C.c_size_t, i64p, C.c_void_p]
        lib.gitmi_jpeg_reconstruct_batch.restype = C.c_int
        lib.gitmi_jpeg_workspace_bytes.argtypes = [i64p, C.c_int]
        lib.gitmi_jpeg_workspace_bytes.restype = C.c_size_t
        lib.gitmi_jpeg_last_error.restype = C.c_char_p
        lib.gitmi_jpeg_entropy_batch.argtypes = [C.c_void_p, C.c_size_t, i64p, C.c_int, C.c_void_p, C.c_size_t, i64p, C.c_void_p,
                                                 C.c_void_p, C.c_size_t, C.c_void_p]
        lib.gitmi_jpeg_entropy_batch.restype = C.c_int
        lib.gitmi_jpeg_entropy_workspace_bytes.argtypes = [i64p, C.c_int]
        lib.gitmi_jpeg_entropy_workspace_bytes.restype = C.c_size_t
        lib.gitmi_jpeg_entropy_constant.argtypes = [C.c_int]
        lib.gitmi_jpeg_entropy_constant.restype = C.c_int
        if [lib.gitmi_jpeg_entropy_constant(i) for i in range(3)] != [SUBSEQUENCE_BITS, WORKGROUP_THREADS,
                                                                      SUBSEQUENCES_PER_THREAD_PER_PASS]:
            raise JpegError(f"{GPU_LIB_PATH}: built with other constants of the GPU Huffman decode than this module exports")
        _gpu = lib
    return _gpu


def entropy_decode_into(data: bytes, out_address: int, out_cap: int) -> Tuple[int, JpegInfo]:
    """The C call as it is: JPEG bytes -> a record at `out_address` (8-byte aligned, `out_cap` bytes).  -> (status, info)."""
    info = JpegInfo()
    rc = load_host_library().gitmi_jpeg_entropy_decode(data, len(data), out_address, out_cap, C.byref(info))
    return rc, info


def entropy_decode(data: bytes) -> Optional[np.ndarray]:
    """JPEG bytes -> the coefficient record (uint8 array of record_bytes), or None when the stream is not one the fast path
    takes (decode it with Pillow)."""
    data = bytes(data)
    rc, info = entropy_decode_into(data, None, 0)             # the markers only: how large is the record?
    if rc != NO_SPACE:
        return None
    out = np.empty((int(info.record_bytes) + 7) // 8, dtype=np.uint64).view(np.uint8)[:int(info.record_bytes)]
    rc, _ = entropy_decode_into(data, out.ctypes.data, out.size)
    return out if rc == OK else None


def scan_prepare_into(data: bytes, out_address: int, out_cap: int) -> Tuple[int, JpegInfo, int]:
    """The C call as it is: JPEG bytes -> a scan record at `out_address` (8-byte aligned, `out_cap` bytes).
    -> (status, info, scan record bytes); info.record_bytes is the size of the COEFFICIENT record the GPU will write."""
    info = JpegInfo()
    need = C.c_uint64(0)
    rc = load_host_library().gitmi_jpeg_scan_prepare(data, len(data), out_address, out_cap, C.byref(info), C.byref(need))
    return rc, info, int(need.value)


def scan_prepare(data: bytes) -> Optional[np.ndarray]:
    """JPEG bytes -> the scan record (uint8 array), or None when the stream is not one the GPU Huffman decode takes (restart
    intervals among them: try entropy_decode, then Pillow)."""
    data = bytes(data)
    rc, _, need = scan_prepare_into(data, None, 0)
    if rc != NO_SPACE:
        return None
    out = np.empty((need + 7) // 8, dtype=np.uint64).view(np.uint8)[:need]
    rc, _, _ = scan_prepare_into(data, out.ctypes.data, out.size)
    return out if rc == OK else None


def scan_coef_bytes(scan_record) -> int:
    """bytes of the coefficient record a scan record decodes to (the header's record_bytes)"""
    return int(np.frombuffer(bytes(scan_record[32:40]), dtype="<u8")[0])


def scan_bytes_of(scan_record) -> int:
    """length of the unstuffed scan inside a scan record"""
    return int(np.frombuffer(bytes(scan_record[HEADER_BYTES + 20: HEADER_BYTES + 24]), dtype="<u4")[0])


def record_size(record) -> Tuple[int, int]:
    """(H, W) of a record"""
    w, h = np.frombuffer(bytes(record[8:16]), dtype="<u4")
    return int(h), int(w)


def _stream_handle(stream) -> int:
    import torch
    if stream is None:
        return int(torch.cuda.current_stream().cuda_stream)
    return int(getattr(stream, "cuda_stream", stream))


def decode_batch_to(rgb_buffer, desc: Sequence[Tuple[int, int, int]], coef, coef_offsets: Sequence[int], stream=None) -> None:
    """gitmi_jpeg_reconstruct_batch: `coef` (uint8 cuda tensor holding one record per image at `coef_offsets`, multiples of
    128) -> uint8 [H, W, 3] of image i at rgb_buffer[desc[i][0]:], desc[i] = (byte offset, H, W) -- the table
    engine.preprocess_batch takes.  Everything is enqueued on `stream` (default: the current one); nothing synchronises."""
    import torch
    lib = load_gpu_library()
    n = len(desc)
    assert n == len(coef_offsets) and n >= 1
    for t in (rgb_buffer, coef):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    table = (C.c_int64 * (3 * n))(*[int(v) for d in desc for v in d])
    offs = (C.c_int64 * n)(*[int(v) for v in coef_offsets])
    need = int(lib.gitmi_jpeg_workspace_bytes(table, n))
    if need == 0:
        raise JpegError("decode_batch_to: an image size outside [1, 16384]")
    tmp = torch.empty(need, dtype=torch.uint8, device=rgb_buffer.device)
    handle = _stream_handle(stream)
    if lib.gitmi_jpeg_reconstruct_batch(coef.data_ptr(), coef.numel(), offs, n, tmp.data_ptr(), tmp.numel(), rgb_buffer.data_ptr(),
                                        rgb_buffer.numel(), table, handle) != 0:
        raise JpegError(lib.gitmi_jpeg_last_error().decode("utf-8", "replace"))
    if stream is not None and hasattr(stream, "cuda_stream"):
        tmp.record_stream(stream)
        coef.record_stream(stream)


def entropy_workspace_bytes(scan_offsets: Sequence[Tuple[int, int]]) -> int:
    n = len(scan_offsets)
    table = (C.c_int64 * (2 * n))(*[int(v) for d in scan_offsets for v in d])
    return int(load_gpu_library().gitmi_jpeg_entropy_workspace_bytes(table, n))


def entropy_batch_to(coef_out, coef_desc: Sequence[Tuple[int, int]], scans, scan_offsets: Sequence[Tuple[int, int]], status,
                     stream=None, workspace=None) -> None:
    """gitmi_jpeg_entropy_batch: `scans` (uint8 cuda tensor, scan record i at scan_offsets[i] = (byte offset, a multiple of
    128; bytes of the record)) -> coefficient record i at coef_out[coef_desc[i][0]:], coef_desc[i] = (byte offset, a multiple
    of 128; record bytes = info.record_bytes of scan_prepare).  status: int32 cuda tensor [n]; 0 = the record is the host
    decoder's, anything else = decode that image another way.  workspace: uint8 cuda tensor of at least
    entropy_workspace_bytes(scan_offsets) (default: allocated here).  Everything is enqueued on `stream`; nothing synchronises."""
    import torch
    lib = load_gpu_library()
    n = len(coef_desc)
    assert n == len(scan_offsets) and n >= 1
    for t in (coef_out, scans):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()
    assert status.is_cuda and status.dtype == torch.int32 and status.is_contiguous() and status.numel() >= n
    sd = (C.c_int64 * (2 * n))(*[int(v) for d in scan_offsets for v in d])
    cd = (C.c_int64 * (2 * n))(*[int(v) for d in coef_desc for v in d])
    if workspace is None:
        workspace = torch.empty(max(int(lib.gitmi_jpeg_entropy_workspace_bytes(sd, n)), 128), dtype=torch.uint8, device=scans.device)
    assert workspace.is_cuda and workspace.dtype == torch.uint8 and workspace.is_contiguous()
    handle = _stream_handle(stream)
    if lib.gitmi_jpeg_entropy_batch(scans.data_ptr(), scans.numel(), sd, n, coef_out.data_ptr(), coef_out.numel(), cd,
                                    status.data_ptr(), workspace.data_ptr(), workspace.numel(), handle) != 0:
        raise JpegError(lib.gitmi_jpeg_last_error().decode("utf-8", "replace"))
    if stream is not None and hasattr(stream, "cuda_stream"):
        workspace.record_stream(stream)
        scans.record_stream(stream)


def decode_scans(records: Sequence[np.ndarray], stream=None):
    """Scan records (scan_prepare) -> (list of coefficient records, uint8 cuda tensors that are views of one device buffer;
    int32 cuda tensor [n] of status words): one upload and one fixed set of launches for the whole batch."""
    import torch
    assert len(records) >= 1
    host, offs = pack_records(records)
    sizes = [scan_coef_bytes(r) for r in records]
    desc, total = [], 0
    for b in sizes:
        desc.append((total, b))
        total += (b + 127) // 128 * 128
    ctx = torch.cuda.stream(stream) if stream is not None and hasattr(stream, "cuda_stream") else None
    if ctx is not None:
        ctx.__enter__()
    try:
        scans = torch.from_numpy(host).cuda()
        coef = torch.empty(max(total, 128), dtype=torch.uint8, device="cuda")
        status = torch.empty(len(records), dtype=torch.int32, device="cuda")
        entropy_batch_to(coef, desc, scans, [(o, len(r)) for o, r in zip(offs, records)], status, stream=stream)
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return [coef[o: o + b] for o, b in desc], status


def pack_records(records: Sequence[np.ndarray]) -> Tuple[np.ndarray, List[int]]:
    """records -> (one uint8 host array with every record at a multiple of 128, their offsets)"""
    offs, total = [], 0
    for r in records:
        offs.append(total)
        total += (len(r) + 127) // 128 * 128
    host = np.zeros(max(total, 128), dtype=np.uint8)
    for r, o in zip(records, offs):
        host[o: o + len(r)] = r
    return host, offs


def reconstruct_batch(records: Sequence[np.ndarray], stream=None) -> list:
    """Coefficient records (entropy_decode) -> list of uint8 [H, W, 3] cuda tensors, views of one device buffer: one upload
    and one fixed set of launches for the whole batch."""
    import torch
    assert len(records) >= 1
    host, offs = pack_records(records)
    sizes = [record_size(r) for r in records]
    desc, total = [], 0
    for h, w in sizes:
        desc.append((total, h, w))
        total += (h * w * 3 + 63) // 64 * 64
    ctx = torch.cuda.stream(stream) if stream is not None and hasattr(stream, "cuda_stream") else None
    if ctx is not None:
        ctx.__enter__()
    try:
        coef = torch.from_numpy(host).cuda()
        rgb = torch.empty(total, dtype=torch.uint8, device="cuda")
        decode_batch_to(rgb, desc, coef, offs, stream=stream)
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return [rgb[o: o + h * w * 3].view(h, w, 3) for o, h, w in desc]
