"""ctypes binding of libgitmi.so (include/gitmi.h) -- the only way Python reaches the HIP kernels.

PyTorch is used for device memory, streams and host<->device copies only; every FLOP of the
hot path runs inside the shared library.  There is no CPU fallback: if the library is missing
or no gfx950 device is present this module raises, it never silently computes on the host.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgitmi.so")                 # bf16 operands (BASELINE's named precision; bench.py: alt_precision)
LIB_PATH_F16 = os.path.join(_HERE, "libgitmi_f16.so")         # the same sources built for fp16 operands (-DGITMI_OPS_F16)
LIB_PATH_EXP = os.path.join(_HERE, "libgitmi_exp.so")         # measurement build of libgitmi.so (-DGITMI_EXPERIMENT): see use_experiment_build
LIB_PATH_F16_EXP = os.path.join(_HERE, "libgitmi_f16_exp.so") # measurement build of libgitmi_f16.so: the hooks of gitmi_experiment.h on fp16 operands

PREC_BF16, PREC_F32 = 0, 1
DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
DTYPE_F16_STREAM = 3      # gitmi_op_gemm's out_dtype only: fp16 residual-stream rows, fp16 residual rows in
SEARCH_AUTOREGRESSIVE, SEARCH_GENERATOR, SEARCH_TRIE = 0, 1, 2
SEARCH_SCORE = 3     # not a search: gitmi_generate_prefixed scores given sentences (Engine.score)
SEARCH_ATTEND = 4    # not a search: gitmi_generate_prefixed returns the attention maps of given sentences (Engine.attend)
SEARCH_CONTEXT = 5   # not a search: gitmi_generate_prefixed puts context tokens into the decoder memory (Engine.encode_context)
SEARCH_TREE_SCORE = 6  # not a search: gitmi_generate_prefixed scores every node of given token trees (Engine.score_tree)
SEARCH_KEEP = 7        # not a search: gitmi_generate_prefixed copies the memory of resident images into a caller's store (Engine.keep)
SEARCH_RECALL = 8      # not a search: gitmi_generate_prefixed makes kept slots the resident images (Engine.recall)
SEARCH_FEATURES = 9    # not a search: gitmi_generate_prefixed makes given feature rows the resident images (Engine.install_features)
SEARCH_CONSTRAIN = 10  # not a search: gitmi_generate_prefixed arms per-sentence decoding constraints for the next search (Engine.constrain)
SEARCH_TRACE = 11  # not a search: gitmi_generate_prefixed arms the per-token trace of the next search (Engine.trace)
TRACE_MAX_ALTERNATIVES = 8
MEMORY_HEADER_BYTES = 256      # header of a slot of an image store; slots are multiples of this size (include/gitmi.h)


def memory_slot_bytes(vit_width: int, dec_hidden: int, dec_layers: int, rows: int, esz: int) -> int:
    """Bytes of one slot of an image store (include/gitmi.h GITMI_SEARCH_KEEP): the header, then `rows` (the engine's per-image
    row capacity) feature rows and K | V rows of every decoder layer in elements of esz bytes, rounded up to 256."""
    raw = MEMORY_HEADER_BYTES + int(rows) * (int(vit_width) + int(dec_layers) * 2 * int(dec_hidden)) * int(esz)
    return -(-raw // MEMORY_HEADER_BYTES) * MEMORY_HEADER_BYTES
ACT_NONE, ACT_QUICKGELU, ACT_GELU_ERF = 0, 1, 2

EXPORTED_SYMBOLS = [
    "gitmi_abi_version", "gitmi_last_error", "gitmi_create", "gitmi_destroy", "gitmi_load_tensor",
    "gitmi_finalize_weights", "gitmi_encode_frames", "gitmi_prefill", "gitmi_step_logits",
    "gitmi_generate", "gitmi_search_begin", "gitmi_search_rows", "gitmi_search_advance",
    "gitmi_search_finish", "gitmi_profile_enable", "gitmi_profile_read", "gitmi_set_graph",
    "gitmi_op_gemm", "gitmi_op_layernorm", "gitmi_op_attention", "gitmi_op_dgemm", "gitmi_op_dgemm_res",
    "gitmi_op_vocab_topm", "gitmi_clone", "gitmi_op_attn_decode", "gitmi_preprocess_image",
    "gitmi_set_image_shape", "gitmi_preprocess_image_to", "gitmi_generate_prefixed", "gitmi_set_temporal_embedding", "gitmi_op_kv_repack", "gitmi_set_encode_after", "gitmi_op_sample_rows",
    "gitmi_search_done_count", "gitmi_set_trie", "gitmi_operand_dtype", "gitmi_set_shared_device", "gitmi_preprocess_batch",
    "gitmi_set_ln_fold", "gitmi_op_gemm_ln",
]
# libgitmi_exp.so and libgitmi_f16_exp.so only (include/gitmi_experiment.h): schedules that measured slower than the default, debug hooks
EXPERIMENT_SYMBOLS = [
    "gitmi_debug_import_stage", "gitmi_debug_head_from", "gitmi_debug_set_gemm_impl", "gitmi_debug_set_dgemm",
    "gitmi_debug_score_attn", "gitmi_debug_score_head", "gitmi_debug_attention_ragged", "gitmi_debug_attn_decode_ragged",
    "gitmi_debug_vocab_topm_rules", "gitmi_debug_search_begin_prefixed", "gitmi_debug_search_advance_lists", "gitmi_debug_read_hidden",
    "gitmi_debug_im2col", "gitmi_debug_pos_resize", "gitmi_debug_vit_assemble", "gitmi_debug_ragged_front", "gitmi_debug_zero_pad_rows",
    "gitmi_debug_layernorm_map", "gitmi_debug_score_attn_map", "gitmi_debug_attn_decode_form", "gitmi_debug_dgemm_form",
    "gitmi_debug_gemm_form", "gitmi_debug_context_embed", "gitmi_debug_attn_decode_qkv", "gitmi_debug_score_attn_tree",
    "gitmi_debug_row_topm", "gitmi_debug_trie_select", "gitmi_debug_sample_rows",
    "gitmi_debug_score_embed", "gitmi_debug_tree_tables", "gitmi_debug_score_tail",
]


class GitmiConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "image_size", "patch", "vit_width", "vit_layers", "vit_heads", "dec_hidden", "dec_layers",
        "dec_heads", "dec_ffn", "vocab", "max_pos", "num_frames", "sos", "eos", "precision",
        "max_batch", "max_beams", "max_frames", "max_text_len", "max_image_pixels", "max_image_tokens")]


class GitmiSearch(C.Structure):
    _fields_ = [("kind", C.c_int32), ("beam_size", C.c_int32), ("per_node_beam_size", C.c_int32),
                ("max_steps", C.c_int32), ("length_penalty", C.c_double),
                ("do_sample", C.c_int32), ("top_k", C.c_int32), ("top_p", C.c_double), ("temperature", C.c_double),
                ("seed", C.c_uint64), ("repetition_penalty", C.c_double),
                ("num_keep_best", C.c_int32), ("reserved_", C.c_int32)]


class GitmiProfile(C.Structure):
    _fields_ = [("vit_ms", C.c_float), ("prefill_ms", C.c_float), ("decode_ms", C.c_float),
                ("total_ms", C.c_float), ("gemm_ms", C.c_float), ("gemm_launches", C.c_int32),
                ("gemm_flops", C.c_double), ("vit_gemm_ms", C.c_float), ("vit_gemm_launches", C.c_int32),
                ("vit_gemm_flops", C.c_double), ("decode_step_ms", C.c_float), ("decode_steps", C.c_int32),
                ("decode_step_bytes", C.c_double)]

    def as_dict(self) -> Dict[str, float]:
        return {n: getattr(self, n) for n, _ in self._fields_}


class GitmiError(RuntimeError):
    pass


_libs: Dict[str, C.CDLL] = {}
_experiment = False
_MEASUREMENT_LIBS = ("exp", "f16_exp")
_gemm_impl = -1           # the last set_gemm_impl selector: a measurement library loaded later starts from it


def use_experiment_build(on: bool = True) -> None:
    """Measurement harnesses only (bench.py --experiment, tools/): serve "bf16" from libgitmi_exp.so, the same kernels built
    with -DGITMI_EXPERIMENT -- kernel-shape overrides and work-skipping switches read from GITMI_* environment variables
    at gitmi_create.  The product libraries read no environment; nothing in the package turns this on.  "f16" stays
    libgitmi_f16.so (Engine(precision="f16") is the product library either way); the wrappers of the measurement-only entry points
    (_exp_library) reach the fp16 measurement build, libgitmi_f16_exp.so, by the type of their tensors."""
    global _experiment
    _experiment = bool(on)


def load_library(operands: str = "bf16") -> C.CDLL:
    """dlopen libgitmi.so (operands="bf16") or libgitmi_f16.so (operands="f16"); raises (never falls back) when it has
    not been built.  "exp" / "f16_exp": their measurement builds."""
    if operands == "bf16" and _experiment:
        operands = "exp"
    if operands in _libs:
        return _libs[operands]
    path = {"bf16": LIB_PATH, "f16": LIB_PATH_F16, "exp": LIB_PATH_EXP, "f16_exp": LIB_PATH_F16_EXP}[operands]
    if not os.path.exists(path):
        raise GitmiError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C generativeimage2text_amd/csrc`.  There is no CPU fallback.")
    lib = C.CDLL(path)
    vp, i32, i64p, fp = C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p
    lib.gitmi_abi_version.restype = C.c_int
    lib.gitmi_last_error.restype = C.c_char_p
    lib.gitmi_create.argtypes = [C.POINTER(GitmiConfig), i32, C.POINTER(vp)]
    lib.gitmi_destroy.argtypes = [vp]
    lib.gitmi_destroy.restype = None
    lib.gitmi_load_tensor.argtypes = [vp, C.c_char_p, vp, i64p, i32, i32]
    lib.gitmi_finalize_weights.argtypes = [vp]
    lib.gitmi_encode_frames.argtypes = [vp, C.POINTER(vp), i32, i32, vp, vp]
    lib.gitmi_prefill.argtypes = [vp, vp]
    lib.gitmi_step_logits.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.gitmi_generate.argtypes = [vp, C.POINTER(vp), i32, i32, vp, i32, C.POINTER(GitmiSearch), vp, vp, vp, vp]
    lib.gitmi_search_begin.argtypes = [vp, C.POINTER(GitmiSearch), i32, vp, i32, i32, vp]
    lib.gitmi_search_rows.argtypes = [vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
    lib.gitmi_search_advance.argtypes = [vp, vp, vp]
    lib.gitmi_search_finish.argtypes = [vp, vp, vp, vp, vp]
    lib.gitmi_search_done_count.argtypes = [vp, C.POINTER(C.c_int), vp]
    lib.gitmi_set_trie.argtypes = [vp, i32, vp, vp, vp]
    lib.gitmi_profile_enable.argtypes = [vp, i32]
    lib.gitmi_profile_read.argtypes = [vp, C.POINTER(GitmiProfile)]
    lib.gitmi_set_graph.argtypes = [vp, i32]
    lib.gitmi_set_temporal_embedding.argtypes = [vp, i32]
    lib.gitmi_set_encode_after.argtypes = [vp, vp]
    lib.gitmi_set_shared_device.argtypes = [vp, i32]
    lib.gitmi_set_ln_fold.argtypes = [vp, i32]
    lib.gitmi_op_gemm.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.gitmi_op_gemm_ln.argtypes = [vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, C.c_float, vp, vp, i32, i32, i32, i32, vp]
    lib.gitmi_op_layernorm.argtypes = [vp, vp, vp, C.c_float, vp, vp, i32, i32, i32, vp]
    lib.gitmi_op_attention.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
    lib.gitmi_op_dgemm.argtypes = [vp, vp, vp, vp, vp, i32, C.c_float, vp, i32, i32, i32, i32, i32, i32, vp]
    lib.gitmi_op_dgemm_res.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, C.c_float, vp, vp, vp, i32, i32, i32, vp]
    lib.gitmi_op_vocab_topm.argtypes = [vp, vp, vp, vp, vp, i32, C.c_float, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.gitmi_generate_prefixed.argtypes = [vp, C.POINTER(vp), i32, i32, vp, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            i32, C.POINTER(GitmiSearch), vp, vp, vp, vp, vp]
    lib.gitmi_clone.argtypes = [vp, C.POINTER(vp)]
    lib.gitmi_preprocess_image.argtypes = [vp, i32, i32, i32, vp, C.c_size_t, vp, vp]
    lib.gitmi_preprocess_image_to.argtypes = [vp, i32, i32, i32, i32, vp, C.c_size_t, vp, vp]
    lib.gitmi_preprocess_batch.argtypes = [vp, C.c_size_t, i64p, i32, i32, vp, C.c_size_t, vp, vp]
    lib.gitmi_set_image_shape.argtypes = [vp, i32, i32, vp]
    lib.gitmi_op_attn_decode.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.gitmi_op_kv_repack.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    lib.gitmi_op_sample_rows.argtypes = [vp, i32, i32, C.c_float, i32, C.c_float, i32, C.c_uint64, i32, vp, vp, vp, vp]
    if operands in _MEASUREMENT_LIBS:
        lib.gitmi_debug_import_stage.argtypes = [vp, vp, i32, vp]
        lib.gitmi_debug_head_from.argtypes = [vp, vp, i32, vp, vp]
        lib.gitmi_debug_set_gemm_impl.argtypes = [i32]
        lib.gitmi_debug_set_dgemm.argtypes = [i32]
        lib.gitmi_debug_dgemm_form.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.c_float, vp, i32, i32, vp, vp, i32, vp, vp, C.c_float,
                                               vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_gemm_form.argtypes = [vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, C.c_float,
                                              vp, vp, vp, vp, C.c_float, vp]
        lib.gitmi_debug_score_attn.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_score_head.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
        lib.gitmi_debug_score_attn_map.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_score_attn_tree.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_attention_ragged.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_attn_decode_ragged.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_attn_decode_form.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                                     i32, i32, i32, vp]
        lib.gitmi_debug_attn_decode_qkv.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32,
                                                    i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_vocab_topm_rules.argtypes = [vp, vp, vp, vp, vp, i32, C.c_float, i32, i32, i32, i32, i32, vp, i32, i32, vp, i32,
                                                     i32, C.c_float, vp, vp, vp, vp, i32, vp, vp]
        lib.gitmi_debug_search_begin_prefixed.argtypes = [vp, C.POINTER(GitmiSearch), i32, vp, i32, vp, i32, vp]
        lib.gitmi_debug_search_advance_lists.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
        lib.gitmi_debug_read_hidden.argtypes = [vp, i32, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), vp]
        lib.gitmi_debug_im2col.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_pos_resize.argtypes = [vp, vp, i32, i32, i32, i32, vp]
        lib.gitmi_debug_vit_assemble.argtypes = [vp, vp, vp, vp, vp, C.c_float, vp, i32, i32, i32, i32, vp, vp]
        lib.gitmi_debug_ragged_front.argtypes = [i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, C.c_float, vp, i32, vp, i32, i32,
                                                 C.c_longlong, i32, i32, i32, i32, vp]
        lib.gitmi_debug_zero_pad_rows.argtypes = [vp, i32, i32, vp, i32, i32, vp]
        lib.gitmi_debug_layernorm_map.argtypes = [vp, i32, vp, vp, C.c_float, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]
        lib.gitmi_debug_context_embed.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, C.c_float, vp, i32, vp, vp, i32, i32,
                                                  i32, i32, vp]
        lib.gitmi_debug_row_topm.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, i32, i32, C.c_float, i32, vp, vp, vp, vp, vp]
        lib.gitmi_debug_trie_select.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        lib.gitmi_debug_sample_rows.argtypes = [vp, i32, i32, C.c_float, i32, C.c_float, i32, C.c_uint64, i32, vp, vp, vp, i32, vp, i32,
                                                i32, C.c_float, i32, vp, vp, i32, vp]
        lib.gitmi_debug_score_embed.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, C.c_float, i32, vp, vp, i32, vp, vp, vp]
        lib.gitmi_debug_tree_tables.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        lib.gitmi_debug_score_tail.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    for name in EXPORTED_SYMBOLS + (EXPERIMENT_SYMBOLS if operands in _MEASUREMENT_LIBS else []):
        if name not in ("gitmi_last_error", "gitmi_destroy"):
            getattr(lib, name).restype = C.c_int
    if lib.gitmi_abi_version() != 10:
        raise GitmiError("libgitmi.so ABI version mismatch")
    lib.gitmi_operand_dtype.restype = C.c_int
    if lib.gitmi_operand_dtype() != {"bf16": DTYPE_BF16, "f16": DTYPE_F16, "exp": DTYPE_BF16, "f16_exp": DTYPE_F16}[operands]:
        raise GitmiError(f"{path} was not built for {operands} operands")
    if operands in _MEASUREMENT_LIBS and _gemm_impl != -1:
        _ck(lib.gitmi_debug_set_gemm_impl(_gemm_impl), lib)
    _libs[operands] = lib
    return lib


def _experiment_only(lib, name: str):
    """An entry point of include/gitmi_experiment.h: present in libgitmi_exp.so / libgitmi_f16_exp.so only."""
    try:
        return getattr(lib, name)
    except AttributeError:
        raise GitmiError(f"{name} is exported by the measurement build only (libgitmi_exp.so, libgitmi_f16_exp.so): call "
                         f"generativeimage2text_amd.engine.use_experiment_build() before creating the engine") from None


def _ck(rc: int, lib=None) -> None:
    """Raise GitmiError with the failing library's own message (the message is thread-local PER LIBRARY and is not cleared
    by later successful calls: with both libgitmi.so and libgitmi_f16.so loaded, asking every library would report the other's
    stale text as well)."""
    if rc != 0:
        libs = [lib] if lib is not None else list(_libs.values())
        msgs = [m for m in ((l.gitmi_last_error() or b"").decode("utf-8", "replace") for l in libs) if m]
        raise GitmiError(" | ".join(msgs) or "gitmi call failed")


def _stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


def _torch_dtype_code(t: torch.Tensor) -> int:
    return {torch.float32: DTYPE_F32, torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_F16}[t.dtype]


_OPERAND_LIBS = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _op_library(*dtypes: torch.dtype, fp32_ok: bool = False) -> C.CDLL:
    """The library of a gitmi_op_* call, picked by the dtype of its 16-bit tensors: fp16 -> libgitmi_f16.so, bf16 ->
    libgitmi.so (or the measurement build, use_experiment_build).  They must share one dtype; fp32 ones are skipped, and an
    all-fp32 call (fp32_ok) goes to libgitmi.so."""
    dts = set(dtypes) - {torch.float32}
    if not dts and fp32_ok:
        return load_library()
    if len(dts) != 1 or next(iter(dts)) not in _OPERAND_LIBS:
        raise GitmiError(f"operands must all be bf16 or all fp16, got {sorted(str(d) for d in dts) or ['float32']}")
    return load_library(_OPERAND_LIBS[dts.pop()])


def _exp_library(*dtypes: torch.dtype, operands: Optional[str] = None) -> C.CDLL:
    """The library of a gitmi_debug_* call (include/gitmi_experiment.h), picked as _op_library picks the product one: by the
    dtype of the call's tensors in the 16-bit OPERAND type -- fp16 -> libgitmi_f16_exp.so, bf16 or none -> libgitmi_exp.so.
    operands ("bf16" | "f16") names it where no tensor can: fp16 residual-stream rows exist in both builds.  Without
    use_experiment_build() the product library of that type comes back, and _experiment_only says what is missing."""
    if operands is None:
        dts = set(dtypes) - {torch.float32}
        if len(dts) > 1 or not dts <= set(_OPERAND_LIBS):
            raise GitmiError(f"operands must all be bf16 or all fp16, got {sorted(str(d) for d in dts)}")
        operands = _OPERAND_LIBS[dts.pop()] if dts else "bf16"
    if operands not in ("bf16", "f16"):
        raise GitmiError(f"operands={operands!r}: bf16 or f16")
    return load_library("f16_exp" if operands == "f16" and _experiment else operands)


RAGGED_DESC_BYTES = 256    # the descriptor block of a ragged input is padded to this size (include/gitmi.h)


def id_table(rows: Sequence[Sequence[int]]) -> torch.Tensor:
    """Id lists of any lengths -> int64 [len(rows), longest] on the CPU, zero-padded past each row's end."""
    table = torch.zeros(len(rows), max(len(r) for r in rows), dtype=torch.int64)
    for q, r in enumerate(rows):
        table[q, :len(r)] = torch.as_tensor(list(r), dtype=torch.int64)
    return table


def _sentence_tables(lens: Sequence[int], image_of: Optional[Sequence[int]]):
    """(prefix_len_host, image_of_host) of gitmi_generate_prefixed as int32 arrays (image_of None: sentence q <-> image q)."""
    Q = len(lens)
    return (C.c_int32 * Q)(*lens), None if image_of is None else (C.c_int32 * Q)(*[int(i) for i in image_of])


CONSTRAINT_KEYS = ("min_new_tokens", "no_repeat_ngram_size", "bad_tokens", "allowed_tokens")


def constraint_tables(n: int, vocab: int, eos: int, min_new_tokens=0, no_repeat_ngram_size=0, bad_tokens=None, allowed_tokens=None,
                      max_new: Optional[int] = None):
    """Host side of Engine.constrain: the per-sentence decoding constraints of `n` sentences in the form of include/gitmi.h
    (GITMI_SEARCH_CONSTRAIN).  Every argument is one value for all sentences or a list of n values, one per sentence:
    min_new_tokens an int, no_repeat_ngram_size an int in 0 .. 8, bad_tokens / allowed_tokens a list of token ids (or None:
    no list for that sentence; for all sentences a flat list of ids, per sentence a list of n lists / Nones).  A sentence bans
    its bad tokens and everything outside its allowed tokens; [SEP] (`eos`) stays allowed unless it is a bad token.
    Identical sets are stored once.  max_new: the largest min_new_tokens the engine accepts (its max_text_len).
    -> (words, table): words a numpy uint32 [n_sets, ceil(vocab / 32)] (bit c % 32 of word c // 32 = token c; the bits at
    and above `vocab` are clear), table n rows [set index or -1, min_new, ngram]; or None when no sentence is constrained."""
    import numpy as np
    n, vocab = int(n), int(vocab)
    if n < 1:
        raise ValueError(f"constraints for {n} sentences")

    def per_sentence(name, value, scalar):
        if scalar(value):
            return [value] * n
        value = list(value)
        if len(value) != n:
            raise ValueError(f"{name} has {len(value)} entries for {n} sentences (one value for all, or one per sentence)")
        return value

    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    is_ids = lambda v: v is None or (isinstance(v, (list, tuple)) and all(is_int(t) for t in v)) or \
        (hasattr(v, "dim") and v.dim() == 1) or (isinstance(v, np.ndarray) and v.ndim == 1)
    min_new = per_sentence("min_new_tokens", 0 if min_new_tokens is None else min_new_tokens, is_int)
    ngram = per_sentence("no_repeat_ngram_size", 0 if no_repeat_ngram_size is None else no_repeat_ngram_size, is_int)
    bad = per_sentence("bad_tokens", bad_tokens, is_ids)
    allowed = per_sentence("allowed_tokens", allowed_tokens, is_ids)
    W = (vocab + 31) // 32
    sets, index, table = [], {}, []
    for q in range(n):
        if not is_int(min_new[q]) or min_new[q] < 0 or (max_new is not None and min_new[q] > max_new):
            raise ValueError(f"sentence {q}: min_new_tokens {min_new[q]!r} outside [0, {max_new if max_new is not None else 'max_text_len'}]")
        if not is_int(ngram[q]) or not 0 <= ngram[q] <= 8:
            raise ValueError(f"sentence {q}: no_repeat_ngram_size {ngram[q]!r} outside [0, 8]")
        ids = {}
        for name, lst in (("bad_tokens", bad[q]), ("allowed_tokens", allowed[q])):
            if lst is None:
                continue
            if not is_ids(lst):
                raise ValueError(f"sentence {q}: {name} must be a list of token ids")
            ids[name] = [int(t) for t in (lst.tolist() if hasattr(lst, "tolist") else lst)]
            for t in ids[name]:
                if t < 0 or t >= vocab:
                    raise ValueError(f"sentence {q}: {name} holds token {t} outside [0, {vocab})")
        set_index = -1
        if ids:
            bits = np.zeros(W * 32, dtype=bool)
            if "allowed_tokens" in ids:
                bits[:vocab] = True
                bits[ids["allowed_tokens"]] = False
                bits[int(eos)] = False
            if "bad_tokens" in ids:
                bits[ids["bad_tokens"]] = True
            if bits.any():
                words = np.packbits(bits.reshape(W, 32), axis=1, bitorder="little").view("<u4").reshape(W).astype(np.uint32)
                key = words.tobytes()
                if key not in index:
                    index[key] = len(sets)
                    sets.append(words)
                set_index = index[key]
        table.append([set_index, int(min_new[q]), int(ngram[q])])
    if all(row == [-1, 0, 0] for row in table):
        return None
    return (np.stack(sets) if sets else np.zeros((0, W), dtype=np.uint32)), table


SEQUENCE_MAX_LEN = 16          # tokens of one banned sequence (include/gitmi.h)
SEQUENCE_MAX_SEQS = 4096       # sequences of one arming call, all lists together
SEQUENCE_MAX_TOKENS = 32768    # their tokens


def banned_sequence_tables(n: int, vocab: int, sequences):
    """Host side of Engine.constrain(..., sequences=): the banned token sequences of `n` sentences in the form of include/gitmi.h
    (the extension of GITMI_SEARCH_CONSTRAIN).  sequences: one list of id sequences for all sentences, or n entries that are each
    None or such a list; an element that is a list of ints is a sequence.  A sequence of one token is a banned token: it comes
    back in `singles` for the sentence's bit set and never reaches the engine; the others have 2 .. SEQUENCE_MAX_LEN tokens.
    Identical lists (the same sequences in the same order, duplicates within a list dropped) are stored once.
    -> (singles, pool): singles n entries, each None or the list of single-token ids of the sentence; pool a numpy int32 array
    { L, S, T, 0, list_of[n], list_off[L + 1], seq_off[S + 1], tok[T] }, or None when no sentence has a longer sequence."""
    import numpy as np
    n, vocab = int(n), int(vocab)
    if n < 1:
        raise ValueError(f"banned sequences for {n} sentences")
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    is_seq = lambda v: isinstance(v, (list, tuple)) and len(v) > 0 and all(is_int(t) for t in v)
    if sequences is None:
        return [None] * n, None
    if not isinstance(sequences, (list, tuple)):
        raise ValueError("bad_sequences must be a list of id sequences, or one such list (or None) per sentence")
    if all(is_seq(v) for v in sequences):           # one list for every sentence (the empty list among them)
        per = [list(sequences)] * n
    else:
        per = list(sequences)
        if len(per) != n:
            raise ValueError(f"bad_sequences has {len(per)} entries for {n} sentences (one list for all, or one per sentence)")
    singles, list_of, lists, index = [], [], [], {}
    for q, lst in enumerate(per):
        if lst is None:
            singles.append(None)
            list_of.append(-1)
            continue
        if not isinstance(lst, (list, tuple)):
            raise ValueError(f"sentence {q}: bad_sequences must be a list of id sequences or None, got {type(lst).__name__}")
        one, many = [], []
        for j, seq in enumerate(lst):
            if not is_seq(seq):
                raise ValueError(f"sentence {q}: sequence {j} must be a non-empty list of token ids, got {seq!r}")
            seq = tuple(int(t) for t in seq)
            for t in seq:
                if t < 0 or t >= vocab:
                    raise ValueError(f"sentence {q}: sequence {j} holds token {t} outside [0, {vocab})")
            if len(seq) > SEQUENCE_MAX_LEN:
                raise ValueError(f"sentence {q}: sequence {j} has {len(seq)} tokens, at most {SEQUENCE_MAX_LEN} are supported")
            if len(seq) == 1:
                one.append(seq[0])
            elif seq not in many:
                many.append(seq)
        singles.append(one or None)
        if not many:
            list_of.append(-1)
            continue
        key = tuple(many)
        if key not in index:
            index[key] = len(lists)
            lists.append(many)
        list_of.append(index[key])
    if not lists:
        return singles, None
    list_off, seq_off, tok = [0], [0], []
    for many in lists:
        for seq in many:
            tok.extend(seq)
            seq_off.append(len(tok))
        list_off.append(len(seq_off) - 1)
    S, T = len(seq_off) - 1, len(tok)
    if S > SEQUENCE_MAX_SEQS or T > SEQUENCE_MAX_TOKENS:
        raise ValueError(f"bad_sequences: {S} distinct sequences with {T} tokens in {len(lists)} lists; one call carries at most "
                         f"{SEQUENCE_MAX_SEQS} sequences and {SEQUENCE_MAX_TOKENS} tokens")
    return singles, np.array([len(lists), S, T, 0] + list_of + list_off + seq_off + tok, dtype=np.int32)


class Geometry(tuple):
    """Engine.resident_geometry: the tuple (Nk, F, grids) -- Nk key rows of an image's block (its row stride), F frames, the token
    grid of every image -- plus, for a batch that carries context tokens (Engine.encode_context): image_rows, the F * n_tok image
    rows at the head of every block, and context, the valid context rows of every image behind them (all 0 without context)."""

    def __new__(cls, Nk: int, F: int, grids, image_rows: Optional[int] = None, context: Optional[Sequence[int]] = None):
        self = super().__new__(cls, (int(Nk), int(F), list(grids)))
        self.image_rows = int(Nk if image_rows is None else image_rows)
        self.context = [0] * len(self[2]) if context is None else [int(v) for v in context]
        return self

    @property
    def stride(self) -> int:
        return self[0]


def context_segments(context, B: int, vocab: int, max_pos: int):
    """The reference's batch['context'] -- a list of {'tokens': int [B, Lc], 'length': int [B]} (decoder.py:861-871) -- as the
    segments of Engine.encode_context: (segments [id lists], image_of [image of every segment]).  Segment i of the list gives
    image b the first length[b] ids of its row (ids past the length are padding: the reference masks them as keys); zero-length
    segments are dropped; the segments of one image keep the order of the list.  Every segment is embedded with positions
    0 .. length - 1 (they restart in every segment).  Raises ValueError for ids outside [0, vocab) and lengths outside
    [0, min(Lc, max_pos)]."""
    segments, image_of = [], []
    for i, seg in enumerate(context or []):
        tokens = torch.as_tensor(seg["tokens"]).detach().to("cpu", torch.int64)
        length = torch.as_tensor(seg["length"]).detach().to("cpu", torch.int64).reshape(-1)
        if tokens.dim() != 2 or int(tokens.shape[0]) != B or int(length.numel()) != B:
            raise ValueError(f"context[{i}]: 'tokens' must be [B, Lc] and 'length' [B] for the {B} images of the batch, got "
                             f"{tuple(tokens.shape)} and {tuple(length.shape)}")
        Lc = int(tokens.shape[1])
        for b in range(B):
            n = int(length[b])
            if n < 0 or n > Lc:
                raise ValueError(f"context[{i}]: length {n} of image {b} outside [0, {Lc}]")
            if n > max_pos:
                raise ValueError(f"context[{i}]: a segment of {n} tokens exceeds the {max_pos} positions of the textual embedding")
            if n == 0:
                continue
            ids = tokens[b, :n].tolist()
            if min(ids) < 0 or max(ids) >= vocab:
                raise ValueError(f"context[{i}]: token ids of image {b} outside [0, {vocab})")
            segments.append(ids)
            image_of.append(b)
    return segments, image_of


def feature_pieces(pieces, image_of, rows: int, *, max_batch: int, max_frames: int, cap: int, num_frames: int, F: int = 1):
    """Host side of Engine.install_features: the rules of include/gitmi.h (GITMI_SEARCH_FEATURES) checked on the piece list.
    pieces: (first source row, rows, temporal index t or -1 / None) per piece -- a 2-tuple means no temporal index; image_of: the
    image of every piece (None: piece q <-> image q); rows: the rows the caller's buffer holds.  The pieces of an image are
    concatenated in the order given.  -> (table [[src0, n, t]], image_of as a list or None, counts [rows of every image]).
    Raises ValueError naming the piece (or the image) that breaks a rule."""
    table = []
    for q, pc in enumerate(pieces):
        pc = tuple(pc)
        if len(pc) not in (2, 3):
            raise ValueError(f"piece {q}: expected (first row, rows[, temporal index]), got {pc!r}")
        t = -1 if len(pc) == 2 or pc[2] is None else int(pc[2])
        table.append([int(pc[0]), int(pc[1]), t])
    Q = len(table)
    if Q < 1 or Q > max_batch * max_frames:
        raise ValueError(f"{Q} pieces outside [1, {max_batch * max_frames}] (max_batch x max_frames)")
    if image_of is not None:
        image_of = [int(i) for i in image_of]
        if len(image_of) != Q:
            raise ValueError(f"image_of has {len(image_of)} entries for {Q} pieces")
        if min(image_of) < 0:
            raise ValueError(f"piece {image_of.index(min(image_of))}: image {min(image_of)} is negative")
    B = Q if image_of is None else max(image_of) + 1
    if B > max_batch:
        raise ValueError(f"{B} images exceed max_batch={max_batch}")
    if F < 1 or F > max_frames or (num_frames > 0 and F > num_frames):
        raise ValueError(f"F={F} outside [1, {min(max_frames, num_frames) if num_frames > 0 else max_frames}] "
                         f"(max_frames={max_frames}, num_frames={num_frames})")
    counts = [0] * B
    for q, (src0, n, t) in enumerate(table):
        b = q if image_of is None else image_of[q]
        if n < 1:
            raise ValueError(f"piece {q}: {n} rows (at least 1)")
        if src0 < 0 or src0 + n > rows:
            raise ValueError(f"piece {q}: rows [{src0}, {src0 + n}) of a buffer of {rows} rows")
        if t < -1:
            raise ValueError(f"piece {q}: temporal index {t} (-1 or None: none)")
        if t >= 0 and num_frames <= 0:
            raise ValueError(f"piece {q}: temporal index {t}, but the model has no temporal embeddings")
        if t >= num_frames and t >= 0:
            raise ValueError(f"piece {q}: temporal index {t} outside [0, {num_frames})")
        counts[b] += n
        if counts[b] > cap:
            raise ValueError(f"piece {q}: image {b} asks for {counts[b]} rows, the engine holds {cap} per image")
    for b, n in enumerate(counts):
        if n == 0:
            raise ValueError(f"image {b} has no piece")
    return table, image_of, counts


def context_capacity(image_size: int, patch: int, max_image_tokens: int, max_frames: int, max_context: int) -> int:
    """gitmi_config.max_image_tokens of an engine that must hold max_context context rows behind the image rows of every image
    (Engine(max_context=...)): the workspaces hold max_frames x max(N, max_image_tokens) rows per image, N = (image_size //
    patch)^2 + 1, and a context call needs max_frames * N + max_context of them at the native resolution.  max_context = 0
    returns max_image_tokens unchanged: today's footprint."""
    if max_context <= 0:
        return int(max_image_tokens)
    n_nat = (int(image_size) // int(patch)) ** 2 + 1
    return max(n_nat, int(max_image_tokens)) + -(-int(max_context) // max(1, int(max_frames)))


class RaggedImages:
    """B images of their own sizes in ONE device buffer: the input of a ragged engine call (gitmi_set_image_shape(e, 0, 0),
    include/gitmi.h).  buffer: fp32 [n] = int32 descriptor [B][4] = {h, w, offset, 0} padded to 256 bytes, then the [3, h, w]
    planes of every image at `offset` floats (a multiple of 4: 16-byte aligned).  shapes: [(h, w)] per image.  Built by
    Engine.pack_images; pass it wherever the engine takes frames (encode, generate, generate_prefixed, score)."""

    def __init__(self, buffer: torch.Tensor, shapes: Sequence[Tuple[int, int]]):
        self.buffer, self.shapes = buffer, [tuple(int(v) for v in hw) for hw in shapes]

    def __len__(self) -> int:
        return len(self.shapes)


def pack_ragged(images: Sequence[torch.Tensor], patch: int, max_pixels: int, max_tokens: int, max_batch: int,
                device=None) -> RaggedImages:
    """Pack fp32 [3, h, w] images of any sizes into the ragged input buffer, validating every shape on the host first
    (the engine checks again on the device): h, w >= patch, h * w <= max_pixels, (h // patch) * (w // patch) + 1 <=
    max_tokens, 1 <= B <= max_batch.  device: where the buffer lives (default: the first image's device)."""
    images = list(images)
    B = len(images)
    if not 1 <= B <= max_batch:
        raise ValueError(f"{B} images: a ragged call takes 1 .. max_batch={max_batch}")
    shapes = []
    for b, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dim() != 3 or int(im.shape[0]) != 3:
            raise ValueError(f"image {b}: expected a [3, h, w] tensor, got {getattr(im, 'shape', type(im))}")
        h, w = int(im.shape[1]), int(im.shape[2])
        if h < patch or w < patch:
            raise ValueError(f"image {b}: {h}x{w} is smaller than one {patch}-pixel patch")
        if h * w > max_pixels:
            raise ValueError(f"image {b}: {h}x{w} exceeds the max_image_pixels capacity ({max_pixels})")
        if (h // patch) * (w // patch) + 1 > max_tokens:
            raise ValueError(f"image {b}: a {h // patch}x{w // patch} token grid exceeds the max_image_tokens capacity "
                             f"({max_tokens})")
        shapes.append((h, w))
    desc_floats = (B * 16 + RAGGED_DESC_BYTES - 1) // RAGGED_DESC_BYTES * (RAGGED_DESC_BYTES // 4)
    offsets, off = [], desc_floats
    for h, w in shapes:
        offsets.append(off)
        off += (3 * h * w + 3) // 4 * 4
    dev = torch.device(device) if device is not None else images[0].device
    buf = torch.zeros(off, dtype=torch.float32, device=dev)
    desc = torch.tensor([[h, w, o, 0] for (h, w), o in zip(shapes, offsets)], dtype=torch.int32)
    buf[:4 * B].view(torch.int32).copy_(desc.reshape(-1))
    for im, (h, w), o in zip(images, shapes, offsets):
        buf[o:o + 3 * h * w].copy_(im.detach().to(dtype=torch.float32).reshape(-1))
    return RaggedImages(buf, shapes)


class Engine:
    """One GIT engine on one GPU.  Mirrors what `get_git_model(...).cuda()` holds in the reference."""

    def __init__(self, model_cfg, precision: str = "bf16", max_batch: int = 64, max_beams: int = 4,
                 max_frames: int = 1, max_text_len: int = 40, device: Optional[int] = None,
                 max_image_hw: Optional[Tuple[int, int]] = None, max_context: int = 0):
        """max_image_hw: largest (H, W) input the engine must accept when images are not all image_size x image_size
        (MinMaxResizeForTest models); default: the model config's max_image_hw, else the native square.
        max_context: context rows (encode_context) every image's block must hold behind max_frames frames of image rows at the
        largest resolution; 0 (default): none are reserved, the footprint is what it was."""
        if not torch.cuda.is_available():
            raise GitmiError("no GPU visible: the GIT engine runs on MI355X (gfx950) only, there is no CPU fallback")
        # precision: "f16" (the benchmarked build: fp16 operands) / "bf16" (the same kernels on bf16 operands) / "f32" (exact parity mode)
        self.lib = load_library("f16" if precision in ("f16", "fp16") else "bf16")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.cfg = model_cfg
        self.precision = precision
        c = GitmiConfig()
        for name in ("image_size", "patch", "vit_width", "vit_layers", "vit_heads", "dec_hidden", "dec_layers",
                     "dec_heads", "dec_ffn", "vocab", "max_pos", "num_frames", "sos", "eos"):
            setattr(c, name, int(getattr(model_cfg, name)))
        c.precision = {"bf16": PREC_BF16, "f16": PREC_BF16, "fp16": PREC_BF16, "f32": PREC_F32, "fp32": PREC_F32}[precision]
        c.max_batch, c.max_beams = int(max_batch), int(max_beams)
        c.max_frames, c.max_text_len = int(max_frames), int(max_text_len)
        if max_image_hw is None:
            max_image_hw = getattr(model_cfg, "max_image_hw", None)
        if max_image_hw is not None:
            mh, mw = int(max_image_hw[0]), int(max_image_hw[1])
            c.max_image_pixels = mh * mw
            c.max_image_tokens = (mh // c.patch) * (mw // c.patch) + 1
        c.max_image_tokens = context_capacity(c.image_size, c.patch, c.max_image_tokens, c.max_frames, max_context)
        self.max_context = int(max_context)
        self.c = c
        self.n_tok = (c.image_size // c.patch) ** 2 + 1          # tokens per frame at the CURRENT input resolution
        self._hw = (int(c.image_size), int(c.image_size))
        self._h = C.c_void_p()
        self._ck(self.lib.gitmi_create(C.byref(c), self.device, C.byref(self._h)))
        self._finalized = False
        self._init_resident()
        # host mirror of the two switches whose flip drops the resident images (gitmi_create's defaults)
        self._temb = True
        self._ln_fold = precision in ("f16", "fp16") and c.vit_width % 256 == 0 and c.dec_hidden % 256 == 0

    # -- lifecycle ---------------------------------------------------------------------------
    def _ck(self, rc: int) -> None:
        _ck(rc, self.lib)

    def clone(self) -> "Engine":
        """A second context sharing this engine's packed weights (own workspaces / KV caches / graph),
        for keeping several batches in flight on different streams.  Keep `self` alive while it is used."""
        other = object.__new__(Engine)
        other.lib, other.device, other.cfg, other.precision = self.lib, self.device, self.cfg, self.precision
        other.c = GitmiConfig.from_buffer_copy(self.c)
        other.max_context = self.max_context
        other.n_tok = (self.c.image_size // self.c.patch) ** 2 + 1
        other._hw = (int(self.c.image_size), int(self.c.image_size))
        other._h = C.c_void_p()
        self._ck(self.lib.gitmi_clone(self._h, C.byref(other._h)))
        other._finalized = True
        other._parent = self
        other._init_resident()                                  # every context has its own resident set; a clone starts with none
        other._temb, other._ln_fold = self._temb, self._ln_fold  # clones inherit the switches
        return other

    # -- resident images: what follow-up calls (frames=None) run over ---------------------------------------------------------
    def _init_resident(self) -> None:
        self._resident: Optional[int] = None
        self._generation = 0
        # (Nk image key rows per image, F frames, [(grid h, grid w)] per image): of the resident set / of the frames of this call
        self._geometry = self._call_geometry = None

    @property
    def resident(self) -> Optional[int]:
        """Number of images a follow-up call (generate / generate_prefixed / score with frames=None) would run over, or None:
        the host mirror of include/gitmi.h's residency rules -- set by every call that encodes images, dropped by a change of
        the image shape or mode, of the temporal embedding or of the LayerNorm folding."""
        return self._resident

    @property
    def generation(self) -> int:
        """Counts the changes of the resident set (a new encode, a drop): a handle that remembers it can tell whether the
        images it was issued for are still the ones this context holds (model.Pending)."""
        return self._generation

    @property
    def resident_geometry(self):
        """(Nk, F, [(grid rows, grid columns)] per image) of the resident images, or None: Nk image key rows per image (the
        image columns of Engine.attend), F frames of grid_h * grid_w + 1 tokens each (ragged input: F = 1, every image its own
        grid inside its max_tokens rows).  After encode_context a Geometry: Nk is the row stride of an image's block,
        .image_rows its F * n_tok image rows and .context the context rows of every image behind them."""
        return self._geometry if self._resident is not None else None

    def _drop_resident(self) -> None:
        self._resident = None
        self._generation += 1

    def _encoded(self, rc: int, B: int) -> None:
        """The tail of a call that takes frames: B images are resident if it succeeded.  If it failed, the images of before
        are still resident exactly when the error was found before the first launch; the library is asked (a follow-up call
        whose only fault is an empty prefix fails on that prefix if, and only if, they are), then the call's error is raised."""
        old = self._resident
        self._generation += 1
        if rc == 0:
            self._resident = int(B)
            self._geometry = self._call_geometry
            return
        msg = (self.lib.gitmi_last_error() or b"").decode("utf-8", "replace")
        if old is not None:
            s = GitmiSearch()
            s.max_steps = 1
            dummy = (C.c_int64 * 4)()
            self.lib.gitmi_generate(self._h, None, 0, old, dummy, 0, C.byref(s), dummy, dummy, dummy, None)
            still = b"prefix length" in (self.lib.gitmi_last_error() or b"")
            self._resident = old if still else None
        raise GitmiError(msg or "gitmi call failed")

    def _call(self, frames, rc: int, B: int) -> int:
        """rc of an entry point that was given `frames` (None: a follow-up call, which changes nothing about residency)."""
        if frames is not None:
            self._encoded(rc, B)
        return rc

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.gitmi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -------------------------------------------------------------------------------
    def load_state_dict(self, state_dict: Mapping[str, torch.Tensor]) -> None:
        """Reference keys; tensors may be fp32/bf16/fp16, any device."""
        for key, t in state_dict.items():
            if key == "image_encoder.proj" or key.endswith("attn_mask"):
                continue
            t = t.detach().to("cpu").contiguous()
            if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                t = t.float()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            self._ck(self.lib.gitmi_load_tensor(self._h, key.encode(), t.data_ptr(), shape, t.dim(), _torch_dtype_code(t)))
        self._ck(self.lib.gitmi_finalize_weights(self._h))
        self._finalized = True

    # -- phases --------------------------------------------------------------------------------
    def set_image_shape(self, H: int, W: int) -> None:
        """Input resolution of the following calls (CLIP/model.py:243-251: token grid (H//patch) x (W//patch),
        positional table resized on the device).  Called automatically from the frames' shape."""
        if (H, W) != self._hw:
            self._ck(self.lib.gitmi_set_image_shape(self._h, int(H), int(W), _stream()))
            self._hw = (int(H), int(W))
            self._drop_resident()
            self.n_tok = (H // self.c.patch) * (W // self.c.patch) + 1

    # -- ragged batches: every image of a call at its own size ------------------------------------------------------
    @property
    def max_pixels(self) -> int:
        return max(int(self.c.image_size) ** 2, int(self.c.max_image_pixels))

    @property
    def max_tokens(self) -> int:
        """Nmax: token rows every image owns in a ragged call (the capacity grid, class token included)."""
        return max((int(self.c.image_size) // int(self.c.patch)) ** 2 + 1, int(self.c.max_image_tokens))

    def pack_images(self, images: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
        """fp32 [3, h, w] images of any sizes -> (buffer, shapes): the ragged input of one engine call on this engine's
        device (include/gitmi.h), shapes validated against the engine's capacity here.  RaggedImages(buffer, shapes) -- or
        ragged() -- is what encode / generate / generate_prefixed / score take."""
        r = self.ragged(images)
        return r.buffer, r.shapes

    def ragged(self, images: Sequence[torch.Tensor]) -> RaggedImages:
        return pack_ragged(images, int(self.c.patch), self.max_pixels, self.max_tokens, int(self.c.max_batch),
                           device=f"cuda:{self.device}")

    def _frames_arg(self, frames) -> Tuple[Optional[C.Array], List[torch.Tensor], int]:
        """-> (the `frames` argument of the C call, the tensors to keep alive, B).  frames None: a follow-up call over the
        resident images (NULL, no tensors, their count -- 0 when there are none, which the library refuses by name)."""
        if frames is None:
            return None, [], int(self._resident or 0)
        if isinstance(frames, RaggedImages):
            if self._hw != (0, 0):
                self._ck(self.lib.gitmi_set_image_shape(self._h, 0, 0, _stream()))
                self._hw = (0, 0)
                self.n_tok = self.max_tokens
                self._drop_resident()
            p = int(self.c.patch)
            self._call_geometry = (self.max_tokens, 1, [(h // p, w // p) for h, w in frames.shapes])
            buf = frames.buffer
            if buf.device != torch.device(f"cuda:{self.device}") or buf.dtype != torch.float32:
                raise ValueError("a ragged input buffer must be fp32 on the engine's device (Engine.pack_images)")
            return (C.c_void_p * 1)(buf.data_ptr()), [buf], len(frames)
        keep = [f.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous() for f in frames]
        B, _, H, W = keep[0].shape
        for f in keep:
            assert f.shape == (B, 3, H, W), f"frame shape {tuple(f.shape)}: all frames of a call share one resolution"
        self.set_image_shape(H, W)
        F_eff = min(len(keep), self.c.num_frames) if self.c.num_frames > 0 else len(keep)
        self._call_geometry = (F_eff * self.n_tok, F_eff, [(H // self.c.patch, W // self.c.patch)] * B)
        arr = (C.c_void_p * len(keep))(*[f.data_ptr() for f in keep])
        return arr, keep, B

    def encode(self, frames: Sequence[torch.Tensor], return_features: bool = True) -> Optional[torch.Tensor]:
        arr, keep, B = self._frames_arg(frames)
        F = len(keep)
        F_eff = min(F, self.c.num_frames) if self.c.num_frames > 0 else F
        out = None
        if return_features:
            out = torch.empty(B, F_eff * self.n_tok, self.c.vit_width, device=keep[0].device, dtype=torch.float32)
        self._encoded(self.lib.gitmi_encode_frames(self._h, arr, F, B, _ptr(out), _stream()), B)
        return out

    def encode_context(self, frames: Sequence[torch.Tensor], segments: Sequence[Sequence[int]],
                       lengths: Optional[Sequence[int]] = None, image_of: Optional[Sequence[int]] = None) -> Dict[str, int]:
        """Encode `frames` with context tokens in the decoder memory (include/gitmi.h GITMI_SEARCH_CONTEXT; the reference's
        batch['context'], decoder.py:861-871): segments = id lists (or an int [Q, L] table with `lengths`), segment q belongs to
        image image_of[q] (default: segment q <-> image q); the segments of one image are appended behind its image rows in
        the order given, each embedded with positions from 0.  Runs the image encoder, the context kernel and the prefill; the
        images and their context are resident afterwards and every follow-up call (frames=None: generate, generate_prefixed,
        score) runs over [image | context].  -> {'stride', 'max_context', 'context_rows'}; resident_geometry has the rest.
        Refused by the library, by message and with the resident set untouched: frames None, a ragged batch, a model whose
        visual features and hidden states differ in width, rows beyond the engine's capacity (Engine(max_context=...))."""
        table = torch.as_tensor(segments).to(torch.int64) if lengths is not None else id_table(segments)
        lens = [int(v) for v in lengths] if lengths is not None else [len(r) for r in segments]
        Q = int(table.shape[0])
        if table.dim() != 2 or len(lens) != Q or (image_of is not None and len(image_of) != Q):
            raise ValueError(f"segments must be [Q, L] with Q lengths (and Q image indices), got {tuple(table.shape)}")
        arr, keep, B = self._frames_arg(frames)
        dev = torch.device(f"cuda:{self.device}")
        table = table.to(dev).contiguous()
        info = self._empty(4, torch.int32, dev)
        search = GitmiSearch()
        search.kind = SEARCH_CONTEXT
        rc = self.lib.gitmi_generate_prefixed(self._h, arr, len(keep), B, table.data_ptr(), int(table.shape[1]),
                                              *_sentence_tables(lens, image_of), Q, C.byref(search), None, None, None,
                                              info.data_ptr(), _stream())
        if frames is None:          # the library refuses a follow-up by name (appending context to resident images)
            self._ck(rc)
        if rc == 0:
            counts = [0] * B
            for q, n in enumerate(lens):
                counts[q if image_of is None else int(image_of[q])] += n
            Nk, F_eff, grids = self._call_geometry
            stride, max_c, total, _ = (int(v) for v in info.tolist())          # synchronises: the table upload did already
            self._call_geometry = Geometry(stride, F_eff, grids, image_rows=Nk, context=counts)
            assert max_c == max(counts) and total == sum(counts) and stride >= Nk + max_c
        self._encoded(rc, B)
        return {"stride": stride, "max_context": max_c, "context_rows": total}

    # -- image memory snapshots: keep encoded images in a caller's store, recall any mix of them later ---------------------------
    @property
    def memory_rows(self) -> int:
        """Rows per image the workspaces are sized for (max_frames x max_tokens): the row capacity of a store slot."""
        return int(self.c.max_frames) * self.max_tokens

    def memory_slot_bytes(self) -> int:
        """Bytes of one slot of an image store of this engine (include/gitmi.h GITMI_SEARCH_KEEP): a function of the
        configuration alone, the same for every clone."""
        esz = 4 if self.precision in ("f32", "fp32") else 2
        return memory_slot_bytes(self.c.vit_width, self.c.dec_hidden, self.c.dec_layers, self.memory_rows, esz)

    def memory_store(self, slots: int) -> torch.Tensor:
        """A store of `slots` slots for keep / recall: uint8 [slots, memory_slot_bytes()] on the engine's device (torch's
        allocator aligns it to 256 bytes and more)."""
        return torch.empty(int(slots), self.memory_slot_bytes(), dtype=torch.uint8, device=f"cuda:{self.device}")

    def _store_arg(self, store: torch.Tensor) -> int:
        """-> the slots of `store`, a uint8 tensor [S, slot_bytes] on the engine's device (contiguous, 256-byte aligned)"""
        nbytes = self.memory_slot_bytes()
        if not isinstance(store, torch.Tensor) or store.dtype != torch.uint8 or store.dim() != 2 or int(store.shape[1]) != nbytes:
            raise ValueError(f"an image store is a uint8 tensor [slots, {nbytes}], got {getattr(store, 'dtype', type(store))} "
                             f"{tuple(getattr(store, 'shape', ()))}")
        if store.device != torch.device(f"cuda:{self.device}") or not store.is_contiguous():
            raise ValueError("an image store must be contiguous on the engine's device")
        return int(store.shape[0])

    def _memory_call(self, kind: int, B: int, store_ptr: Optional[int], S: int, slots, images) -> List[int]:
        """gitmi_generate_prefixed with GITMI_SEARCH_KEEP / _RECALL -> info [4]; the call synchronises the stream itself."""
        search = GitmiSearch()
        search.kind = kind
        Q = len(slots)
        info = torch.zeros(4, dtype=torch.int32, device=f"cuda:{self.device}")
        slot_arr, img_arr = _sentence_tables([int(s) for s in slots], images) if Q else (None, None)
        keep, recall = (store_ptr, None) if kind == SEARCH_KEEP else (None, store_ptr)
        self._ck(self.lib.gitmi_generate_prefixed(self._h, None, 0, int(B), recall, int(S), slot_arr, img_arr, Q, C.byref(search),
                                                  None, keep, None, info.data_ptr(), _stream()))
        return [int(v) for v in info.tolist()]

    def keep(self, store: torch.Tensor, slots: Sequence[int], images: Optional[Sequence[int]] = None) -> Dict[str, object]:
        """Copy the encoded memory of resident images into slots of `store` (uint8 [S, memory_slot_bytes()] on the device):
        resident image images[q] (default: image q, all of them) goes to slot slots[q], every slot at most once per call.
        Residency does not change.  The blobs are plain bytes: Engine.recall on any context of the same model, precision
        and capacity -- a clone, or another engine after a copy through the host -- brings the images back.
        -> {'rows': [n per kept image], 'max_rows', 'total_rows', 'geometry': [per kept image (F, (grid h, grid w), image rows,
        context rows)], what recall(geometry=...) takes}"""
        S = self._store_arg(store)
        B = int(self._resident or 0)                # none resident: the library refuses by name
        info = self._memory_call(SEARCH_KEEP, B, store.data_ptr(), S, list(slots), images)
        geo = self._geometry
        if geo is None:                             # images imported through a debug hook: the host knows no geometry
            return {"rows": None, "max_rows": info[1], "total_rows": info[2], "geometry": None}
        per = []
        for q in range(len(slots)):
            b = q if images is None else int(images[q])
            ctx = geo.context[b] if isinstance(geo, Geometry) else 0
            rows = geo.image_rows if isinstance(geo, Geometry) else geo[0]
            if getattr(geo, "rows", None):                                   # a recalled mix: every image its own image rows
                rows = geo.rows[b]
            if self._hw == (0, 0) and not isinstance(geo, Geometry):       # ragged: every image its own grid inside max_tokens rows
                rows = geo[2][b][0] * geo[2][b][1] + 1
            per.append((geo[1], None if geo[2][b] is None else tuple(geo[2][b]), int(rows), int(ctx)))
        return {"rows": [p[2] + p[3] for p in per], "max_rows": info[1], "total_rows": info[2], "geometry": per}

    def recall(self, store: torch.Tensor, slots: Sequence[int], geometry=None) -> Dict[str, int]:
        """Make the images kept in `slots` of `store` (any order, repeats, from different earlier calls or contexts) the resident
        batch of this context: slot slots[q] becomes image q.  Every follow-up call (frames=None) then runs over them.
        The library validates every slot header on the host before anything is launched; a refusal raises GitmiError naming
        the slot and the field and leaves the resident set as it was.
        geometry: per slot what keep returned for it ('geometry': (F, grid, image rows, context rows)); gives
        resident_geometry its grids (attend's patch_grid) -- without it the grids are unknown (None).
        -> {'stride', 'max_rows', 'total_rows'}"""
        S = self._store_arg(store)
        Q = len(slots)
        if geometry is not None and len(geometry) != Q:
            raise ValueError(f"geometry has {len(geometry)} entries for {Q} slots")
        old = self._resident
        try:
            info = self._memory_call(SEARCH_RECALL, Q, store.data_ptr(), S, list(slots), None)
        except GitmiError as err:
            # an argument error ("recall: ...") is found before any launch: the images of before stay resident; a failed launch drops them
            if old is not None and not str(err).startswith("recall:"):
                self._drop_resident()
            raise
        stride, max_n, total, _ = info
        self._generation += 1
        self._resident = Q
        F = int(geometry[0][0]) if geometry else 1
        grids = [None if g[1] is None else tuple(g[1]) for g in geometry] if geometry else [None] * Q
        ctx = [int(g[3]) for g in geometry] if geometry else [0] * Q
        rows = [int(g[2]) for g in geometry] if geometry else [stride] * Q
        if any(ctx) or any(r != stride for r in rows):
            self._geometry = Geometry(stride, F, grids, image_rows=max(rows), context=ctx)
            self._geometry.rows = rows
        else:
            self._geometry = (stride, F, grids)
        return {"stride": stride, "max_rows": max_n, "total_rows": total}

    # -- features in: caller-supplied visual feature rows become the resident images --------------------------------------------
    def feature_store(self, slots: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """[slots, n_tok, vit_width] on the engine's device: feature rows of `slots` images of the current image shape, the
        buffer install_features reads pieces from (model.FeatureStore)."""
        f32 = self.precision in ("f32", "fp32")
        want = torch.float16 if self.precision in ("f16", "fp16") else torch.bfloat16
        if dtype != torch.float32 and (f32 or dtype != want):
            raise ValueError(f"feature rows are torch.float32{'' if f32 else ' or ' + str(want)} on this engine, got {dtype}")
        return torch.empty(int(slots), int(self.n_tok), int(self.c.vit_width), dtype=dtype, device=f"cuda:{self.device}")

    def install_features(self, rows: torch.Tensor, pieces=None, image_of: Optional[Sequence[int]] = None, F: int = 1) -> Dict[str, int]:
        """Make visual feature rows the resident image batch of this context and run the prefill (include/gitmi.h
        GITMI_SEARCH_FEATURES): the input side of encode()'s return value.  rows: a tensor [R, vit_width] on the engine's device
        with `pieces` = (first row, rows, temporal index or None) per piece and image_of = the image of every piece (default:
        piece q <-> image q), the pieces of an image concatenated in the order given; or [B, n, vit_width] with the pieces
        implied (image b = rows[b]).  dtype fp32, or the engine's 16-bit operand type.  F: the frames per image the rows stand
        for.  Every follow-up call (frames=None) then runs over them.  Grids are known only when every image has the F * n_tok
        rows of the current image shape; otherwise resident_geometry is a Geometry with grids None (AttentionMaps.patch_grid
        raises ValueError: the features came without a shape).  An argument error leaves the resident set as it was.
        -> {'stride', 'max_rows', 'total_rows'}"""
        if not isinstance(rows, torch.Tensor) or rows.dim() not in (2, 3) or int(rows.shape[-1]) != int(self.c.vit_width):
            raise ValueError(f"feature rows are a tensor [R, {int(self.c.vit_width)}] or [B, n, {int(self.c.vit_width)}], got "
                             f"{tuple(getattr(rows, 'shape', ()))}")
        if rows.dim() == 3:
            if pieces is not None or image_of is not None:
                raise ValueError("rows [B, n, D] imply the pieces (image b = rows[b]): pass [R, D] rows with pieces")
            n = int(rows.shape[1])
            pieces = [(b * n, n, None) for b in range(int(rows.shape[0]))]
        elif pieces is None:
            raise ValueError("rows [R, D] need pieces")
        f32 = self.precision in ("f32", "fp32")
        want = torch.float16 if self.precision in ("f16", "fp16") else torch.bfloat16
        if rows.dtype != torch.float32 and (f32 or rows.dtype != want):
            raise ValueError(f"feature rows are torch.float32{'' if f32 else ' or ' + str(want)} on this engine, got {rows.dtype}")
        if rows.device != torch.device(f"cuda:{self.device}") or not rows.is_contiguous():
            raise ValueError("feature rows must be contiguous on the engine's device")
        R = int(rows.numel()) // int(self.c.vit_width)
        table, image_of, counts = feature_pieces(pieces, image_of, R, max_batch=int(self.c.max_batch), max_frames=int(self.c.max_frames),
                                                 cap=self.memory_rows, num_frames=int(self.c.num_frames), F=int(F))
        Q, B = len(table), len(counts)
        search = GitmiSearch()
        search.kind = SEARCH_FEATURES
        search.reserved_ = _torch_dtype_code(rows)
        info = torch.zeros(4, dtype=torch.int32, device=f"cuda:{self.device}")
        tab = (C.c_int32 * (3 * Q))(*[v for pc in table for v in pc])
        img = None if image_of is None else (C.c_int32 * Q)(*image_of)
        old = self._resident
        try:
            self._ck(self.lib.gitmi_generate_prefixed(self._h, None, int(F), B, rows.data_ptr(), R, tab, img, Q, C.byref(search),
                                                      None, None, None, info.data_ptr(), _stream()))
        except GitmiError as err:
            # an argument error ("features: ...") is found before any launch: the images of before stay resident; a failed launch drops them
            if old is not None and not str(err).startswith("features:"):
                self._drop_resident()
            raise
        stride, max_n, total, _ = (int(v) for v in info.tolist())
        self._generation += 1
        self._resident = B
        p = int(self.c.patch)
        if self._hw != (0, 0) and all(n == int(F) * self.n_tok for n in counts):
            self._geometry = (stride, int(F), [(self._hw[0] // p, self._hw[1] // p)] * B)
        else:
            self._geometry = Geometry(stride, int(F), [None] * B, image_rows=max(counts), context=[0] * B)
            self._geometry.rows = list(counts)
        return {"stride": stride, "max_rows": max_n, "total_rows": total}

    # -- per-sentence decoding constraints ---------------------------------------------------------------------------------------
    def constrain(self, sets_words, table, sequences=None) -> Dict[str, int]:
        """Arm per-sentence decoding constraints for the NEXT search call of this context (include/gitmi.h
        GITMI_SEARCH_CONSTRAIN; constraint_tables builds the arguments): sets_words uint32 [n_sets, ceil(vocab / 32)] (a numpy
        array or a tensor; None: no sets), table one row [set index or -1, min_new, ngram] per sentence of that call.  One-shot:
        the call consumes them.  An empty table disarms.  The copies are enqueued on the current stream and nothing is read
        back: the host does not wait for the context's work in flight.
        sequences: the int32 pool of banned_sequence_tables for the same sentences (None: no banned sequences -- the C call is
        then exactly the one made without the keyword).
        -> {'sentences', 'sets', 'words'}"""
        import numpy as np
        table = [[int(v) for v in row] for row in (table or [])]
        if any(len(row) != 3 for row in table):
            raise ValueError("a constraint table row is [set index or -1, min_new, ngram]")
        Q, W = len(table), (int(self.c.vocab) + 31) // 32
        words, n_sets = None, 0
        if sets_words is not None and Q:
            if isinstance(sets_words, torch.Tensor):
                words = sets_words.view(torch.int32) if sets_words.dtype != torch.int32 else sets_words
            else:
                words = torch.from_numpy(np.ascontiguousarray(sets_words, dtype=np.uint32).view(np.int32))
            if words.dim() != 2 or int(words.shape[1]) != W:
                raise ValueError(f"ban sets are uint32 [n_sets, {W}] words, got {tuple(words.shape)}")
            n_sets = int(words.shape[0])
            words = words.to(torch.device(f"cuda:{self.device}")).contiguous() if n_sets else None
        search = GitmiSearch()
        search.kind = SEARCH_CONSTRAIN
        info = torch.empty(4, dtype=torch.int32, device=f"cuda:{self.device}")
        tab = (C.c_int32 * max(3 * Q, 1))(*[v for row in table for v in row])
        pool = None
        if sequences is not None and Q:
            seq = np.ascontiguousarray(sequences, dtype=np.int32).reshape(-1)
            if seq.size < 4 + Q:
                raise ValueError(f"a sequence pool for {Q} sentences has at least {4 + Q} words, got {seq.size}")
            pool = (C.c_int32 * int(seq.size))(*seq.tolist())      # host memory: read before the call returns
            search.reserved_ = int(seq.size)
        self._ck(self.lib.gitmi_generate_prefixed(self._h, None, 0, 0, _ptr(words), n_sets, tab, None, Q, C.byref(search),
                                                  None, None, pool, info.data_ptr(), _stream()))
        self._ban_keep = (words, info)  # the copies are enqueued on the stream: both outlive the call
        return {"sentences": Q, "sets": n_sets if Q else 0, "words": W}       # info_out's values (include/gitmi.h), not read back

    # -- per-token trace ---------------------------------------------------------------------------------------------------------
    def trace(self, Q: int, nout: int = 1, T: int = 0, n: int = 0, out_lp: Optional[torch.Tensor] = None,
              out_tok: Optional[torch.Tensor] = None, host_out: bool = False):
        """Arm the per-token trace of the NEXT search call of this context (include/gitmi.h GITMI_SEARCH_TRACE): that call -- Q
        sentences, nout returned sequences each (num_keep_best), max_steps T -- also fills
            out_lp  fp32 [Q * nout, T, 1 + n]: column 0 the log-prob of the token at every position (0 inside the prefix and past
                    the end), columns 1 .. n the log-probs of the n likeliest alternatives there, descending
            out_tok int64 [Q * nout, T, n]: their tokens (-1: none), or None when n == 0
        in the order of its tokens.  One-shot; Q == 0 disarms.  The buffers (made here when not given; host_out: page-locked host
        tensors) are valid once the stream has reached the end of the traced call.  Nothing is read back, the host does not wait.
        -> (out_lp, out_tok)"""
        Q, nout, T, n = int(Q), max(1, int(nout)), int(T), int(n)
        search = GitmiSearch()
        search.kind = SEARCH_TRACE
        if Q == 0:
            self._ck(self.lib.gitmi_generate_prefixed(self._h, None, 0, 0, None, 0, None, None, 0, C.byref(search), None, None, None,
                                                      None, _stream()))
            self._trace_keep = None
            return None, None
        if not 0 <= n <= TRACE_MAX_ALTERNATIVES:
            raise ValueError(f"top_logprobs={n} outside [0, {TRACE_MAX_ALTERNATIVES}]")
        if Q < 0 or T < 1:
            raise ValueError(f"a trace of {Q} sentences and {T} positions")
        dev = torch.device(f"cuda:{self.device}")
        if out_lp is None:
            out_lp = self._empty((Q * nout, T, 1 + n), torch.float32, dev, host_out)
        if out_tok is None and n > 0:
            out_tok = self._empty((Q * nout, T, n), torch.int64, dev, host_out)
        if out_lp.dtype != torch.float32 or out_lp.numel() != Q * nout * T * (1 + n) or not out_lp.is_contiguous():
            raise ValueError(f"out_lp is a contiguous fp32 [{Q * nout}, {T}, {1 + n}] tensor, got {out_lp.dtype} {tuple(out_lp.shape)}")
        if n > 0 and (out_tok.dtype != torch.int64 or out_tok.numel() != Q * nout * T * n or not out_tok.is_contiguous()):
            raise ValueError(f"out_tok is a contiguous int64 [{Q * nout}, {T}, {n}] tensor, got {out_tok.dtype} {tuple(out_tok.shape)}")
        search.num_keep_best, search.max_steps, search.reserved_ = nout, T, n
        self._ck(self.lib.gitmi_generate_prefixed(self._h, None, 0, 0, None, 0, None, None, Q, C.byref(search),
                                                  _ptr(out_tok) if n > 0 else None, out_lp.data_ptr(), None, None, _stream()))
        self._trace_keep = (out_lp, out_tok)    # the traced call writes them: both outlive it
        return out_lp, (out_tok if n > 0 else None)

    def prefill(self) -> None:
        self._ck(self.lib.gitmi_prefill(self._h, _stream()))

    def step_logits(self, tokens: torch.Tensor) -> torch.Tensor:
        tokens = tokens.to(device=f"cuda:{self.device}", dtype=torch.int64).contiguous()
        R, t = tokens.shape
        out = torch.empty(R, self.c.vocab, device=tokens.device, dtype=torch.float32)
        self._ck(self.lib.gitmi_step_logits(self._h, tokens.data_ptr(), R, t, out.data_ptr(), _stream()))
        return out

    @staticmethod
    def make_search(kind: str, max_steps: int, beam_size: int, per_node_beam_size: int,
                    length_penalty: float = 1.0, do_sample: bool = False, top_k: int = 0, top_p: float = 1.0,
                    temperature: float = 1.0, seed: int = 0, repetition_penalty: float = 1.0,
                    num_keep_best: int = 1) -> GitmiSearch:
        s = GitmiSearch()
        s.kind = (SEARCH_AUTOREGRESSIVE if kind in ("greedy", "autoregressive") else SEARCH_TRIE if kind == "trie"
                  else SEARCH_GENERATOR)
        s.beam_size, s.per_node_beam_size, s.max_steps = int(beam_size), int(per_node_beam_size), int(max_steps)
        s.length_penalty = float(length_penalty)
        s.do_sample, s.top_k, s.top_p = int(bool(do_sample)), int(top_k or 0), float(1.0 if top_p is None else top_p)
        s.temperature, s.seed = float(temperature), int(seed)
        s.repetition_penalty = float(repetition_penalty)
        s.num_keep_best = int(num_keep_best)
        return s

    @staticmethod
    def _empty(shape, dtype, dev, host: bool = False) -> torch.Tensor:
        """An output buffer on `dev`, or with host a PAGE-LOCKED host tensor that the request itself fills (valid once the
        stream has reached the end of the call): a server with other requests in flight reads it without a read-back."""
        return torch.empty(shape, dtype=dtype, pin_memory=True) if host else torch.empty(shape, dtype=dtype, device=dev)

    @classmethod
    def _out(cls, n_sent: int, search: GitmiSearch, dev, host: bool = False):
        """Output buffers of a search over n_sent sentences: tokens [n, T] / logprobs [n], or [n, num_keep_best, T] /
        [n, num_keep_best] when GeneratorWithBeamSearch keeps more than one hypothesis (decoder.py:1283-1290); info [4]."""
        nh = max(1, int(search.num_keep_best))
        shape = (n_sent,) if nh == 1 else (n_sent, nh)
        return (cls._empty((*shape, search.max_steps), torch.int64, dev, host), cls._empty(shape, torch.float32, dev, host),
                cls._empty(4, torch.int32, dev, host))

    def _done(self, rc: int, info, sync: bool) -> None:
        """The tail every request shares: raise on a failed call; with sync, wait for the stream and check info[3]."""
        self._ck(rc)
        if sync:
            torch.cuda.current_stream().synchronize()
            self.check_finite(info)

    def generate(self, frames: Optional[Sequence[torch.Tensor]], search: GitmiSearch,
                 prefix: Optional[torch.Tensor] = None, sync: bool = True, host_out: bool = False):
        """-> (tokens int64 [B, max_steps] incl. start tokens / EOS padded, logprobs fp32 [B], info int32 [4]).
        host_out: the three come back as page-locked host tensors (_empty).
        frames None: a follow-up call -- the search runs over the resident images (`resident`), nothing is encoded."""
        arr, keep, B = self._frames_arg(frames)
        dev = torch.device(f"cuda:{self.device}")
        tokens, logprobs, info = self._out(B, search, dev, host_out)
        P, pfx = 1, None
        if prefix is not None:
            pfx = prefix.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
            P = int(pfx.numel())
        self._done(self._call(frames, self.lib.gitmi_generate(self._h, arr, len(keep), B, _ptr(pfx), P, C.byref(search),
                                                              tokens.data_ptr(), logprobs.data_ptr(), info.data_ptr(), _stream()), B),
                   info, sync)
        return tokens, logprobs, info

    def check_finite(self, info) -> None:
        """info[3] of a finished call (include/gitmi.h): sequences with a non-finite log-prob -- an activation left the range
        of the 16-bit operand format (fp16 tops out at 65504).  Raises instead of handing back garbage ids; callers of
        generate(sync=False) call this once the stream has been synchronised."""
        bad = int(info[3]) if isinstance(info, (list, tuple)) else int(info[3].item())
        if bad:
            raise GitmiError(f"{bad} sequence(s) came back with a non-finite log-probability: an activation overflowed the "
                             f"{self.precision} operand range of this build -- run this checkpoint with precision='bf16' or 'f32'")

    def generate_coalesced(self, requests: Sequence[Sequence[torch.Tensor]], search: GitmiSearch, sync: bool = True):
        """Several requests (each a list of F frame tensors [B_i,3,H,W], same F and resolution) served by ONE engine pass
        over sum(B_i) rows: the decode chain's launches and weight reads are shared by all of them (measured on MI355X:
        two 64-image requests per pass +4.6 % captions/s at twice the batch latency).  Captions are independent
        of their batch neighbours, so every request gets what its own generate() call returns.
        -> ([(tokens [B_i, max_steps], logprobs [B_i]) per request], info)"""
        sizes = [int(r[0].shape[0]) for r in requests]
        F = len(requests[0])
        assert all(len(r) == F for r in requests), "coalesced requests must have the same number of frames"
        if sum(sizes) > self.c.max_batch:
            raise GitmiError(f"{sum(sizes)} coalesced rows exceed max_batch={self.c.max_batch}")
        frames = [torch.cat([r[f] for r in requests], dim=0) for f in range(F)] if len(requests) > 1 else list(requests[0])
        tokens, logprobs, info = self.generate(frames, search, sync=sync)
        out, lo = [], 0
        for n in sizes:
            out.append((tokens[lo:lo + n], logprobs[lo:lo + n]))
            lo += n
        return out, info

    def generate_prefixed(self, frames: Optional[Sequence[torch.Tensor]], search: GitmiSearch,
                          prefixes: Sequence[Sequence[int]], image_of: Optional[Sequence[int]] = None, sync: bool = True,
                          host_out: bool = False):
        """Batched VQA: sentence q starts from its own prefix `prefixes[q]` (token ids incl. [CLS], any lengths) and
        attends to image `image_of[q]` of the encoded batch (default: sentence q <-> image q).  Every sentence gets
        exactly what a batch-1 reference call with that image and prefix returns (decoder.py:984-1006).
        frames None: a follow-up call -- new questions (or another search) over the resident images, nothing is encoded.
        -> (tokens int64 [Q, max_steps], logprobs fp32 [Q], sent int32 [Q, 2] = (returned length, early), info int32 [4])"""
        arr, keep, B = self._frames_arg(frames)
        dev = torch.device(f"cuda:{self.device}")
        Q = len(prefixes)
        lens = [len(p) for p in prefixes]
        table = id_table(prefixes).to(dev)
        tokens, logprobs, info = self._out(Q, search, dev, host_out)
        sent = self._empty((Q, 2), torch.int32, dev, host_out)
        self._done(self._call(frames, self.lib.gitmi_generate_prefixed(
            self._h, arr, len(keep), B, table.data_ptr(), table.shape[1], *_sentence_tables(lens, image_of), Q, C.byref(search),
            tokens.data_ptr(), logprobs.data_ptr(), sent.data_ptr(), info.data_ptr(), _stream()), B), info, sync)
        return tokens, logprobs, sent, info

    def score(self, frames: Optional[Sequence[torch.Tensor]], tokens, lengths: Optional[Sequence[int]] = None,
              image_of: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Per-token log-probabilities of given sentences (include/gitmi.h GITMI_SEARCH_SCORE; the textual head of
        CaptioningModel.forward_one_ce, decoder.py:916-972, run once over whole sequences).
        tokens: int [Q, L] (each row starts with [CLS]; entries past a row's length are ignored), lengths: [Q] (default L),
        image_of: [Q] image of the encoded batch every sentence belongs to (default: sentence q <-> image q, Q == B).
        -> fp32 [Q, L, 2] on the device: (lp, mean_lp) at position j = (log_softmax(z)[tokens[q, j]],
        mean_c log_softmax(z)[c]) with z the logits at position j - 1; position 0 and positions >= length are 0.
        frames None: a follow-up call -- the sentences are scored over the resident images, nothing is encoded."""
        arr, keep, B, tok, lens = self._sentence_args(frames, tokens, lengths, image_of)
        Q, L = tok.shape
        out = self._empty((Q, L, 2), torch.float32, tok.device)
        self._sentence_call(SEARCH_SCORE, frames, arr, keep, B, tok, lens, image_of, out)
        return out

    def attend(self, frames: Optional[Sequence[torch.Tensor]], tokens, lengths: Optional[Sequence[int]] = None,
               image_of: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Where every token of given sentences looked (include/gitmi.h GITMI_SEARCH_ATTEND): the attention probabilities of
        the text rows of every decoder layer over [image tokens | text], averaged over the heads.  Arguments and checks as
        for score.
        -> fp32 [Q, L, layers, Kc] on the device, Kc = Nk + L: columns [0, Nk) the image tokens of the sentence's image in
        prefill order (frame-major, class token first; Nk = F * n_tok, or max_tokens in ragged mode), column Nk + t text
        position t.  Rows j >= length, text columns t > j and (ragged) image columns past the image's own tokens are 0.
        frames None: a follow-up call over the resident images, nothing is encoded."""
        arr, keep, B, tok, lens = self._sentence_args(frames, tokens, lengths, image_of)
        Q, L = tok.shape
        geometry = self._geometry if frames is None else self._call_geometry
        Nk = geometry[0] if geometry else 0              # no resident images: the library refuses the call by name
        out = self._empty((Q, L, int(self.c.dec_layers), Nk + L), torch.float32, tok.device)
        self._sentence_call(SEARCH_ATTEND, frames, arr, keep, B, tok, lens, image_of, out)
        return out

    def score_tree(self, frames: Optional[Sequence[torch.Tensor]], tokens, depths, lengths: Optional[Sequence[int]] = None,
                   image_of: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Log-probability of every node of given token trees (include/gitmi.h GITMI_SEARCH_TREE_SCORE): a closed candidate
        set as a trie, every shared prefix scored once.  tokens, depths: int [Q, L], tree q in DFS pre-order -- node 0 the root
        ([CLS]) at depth 0, the parent of node i the last k < i with depths[q, k] == depths[q, i] - 1; lengths: [Q] node counts
        (default L; L is not bounded by max_text_len, the depths are); image_of as for score.
        -> fp32 [Q, L, 2] on the device: (lp, mean_lp) at node i = (log_softmax(z)[tokens[q, i]], mean_c log_softmax(z)[c]) with
        z the logits at the node's parent, computed over [image (| context) | the ancestors]; node 0 and nodes >= length are 0.
        A chain (depths[q, i] = i) is a sentence and the result is score's.  Raises ValueError naming tree and node when a tree
        breaks the depth rules.  frames None: a follow-up call over the resident images, nothing is encoded."""
        arr, keep, B = self._frames_arg(frames)
        table, lens = pack_trees(tokens, depths, lengths, int(self.c.vocab), min(int(self.c.max_text_len), int(self.c.max_pos)))
        Q, L = table.shape
        if Q > self.c.max_batch * self.c.max_beams:
            raise GitmiError(f"{Q} trees exceed the capacity max_batch x max_beams = {self.c.max_batch * self.c.max_beams}")
        if image_of is None and Q != B:
            raise ValueError(f"{Q} trees over {B} images: image_of is required")
        if image_of is not None and len(image_of) != Q:
            raise ValueError(f"image_of has {len(image_of)} entries for {Q} trees")
        table = table.to(torch.device(f"cuda:{self.device}"))
        out = self._empty((Q, L, 2), torch.float32, table.device)
        self._sentence_call(SEARCH_TREE_SCORE, frames, arr, keep, B, table, lens, image_of, out)
        return out

    def _sentence_args(self, frames, tokens, lengths, image_of):
        """The argument checks score and attend share -> (frames argument, tensors to keep alive, B, tokens int64 [Q, L] on the
        device with zeros past every length, lengths)."""
        arr, keep, B = self._frames_arg(frames)
        dev = torch.device(f"cuda:{self.device}")
        tok = torch.as_tensor(tokens).detach().to("cpu", torch.int64)
        if tok.dim() != 2 or tok.shape[1] < 1:
            raise ValueError(f"tokens must be [Q, L], got {tuple(tok.shape)}")
        Q, L = int(tok.shape[0]), int(tok.shape[1])
        lens = [L] * Q if lengths is None else [int(v) for v in lengths]
        if len(lens) != Q or any(v < 1 or v > L for v in lens):
            raise ValueError(f"lengths must be {Q} values in [1, {L}]")
        if Q > self.c.max_batch * self.c.max_beams:
            raise GitmiError(f"{Q} sentences exceed the capacity max_batch x max_beams = {self.c.max_batch * self.c.max_beams}")
        if L > self.c.max_text_len:
            raise GitmiError(f"sentences of {L} tokens exceed max_text_len={self.c.max_text_len}")
        valid = torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]
        ids = tok[valid]
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.c.vocab):
            raise ValueError(f"token ids outside [0, {self.c.vocab})")
        tok = torch.where(valid, tok, torch.zeros_like(tok)).to(dev)
        if image_of is None and Q != B:
            raise ValueError(f"{Q} sentences over {B} images: image_of is required")
        if image_of is not None and len(image_of) != Q:
            raise ValueError(f"image_of has {len(image_of)} entries for {Q} sentences")
        return arr, keep, B, tok, lens

    def _sentence_call(self, kind: int, frames, arr, keep, B: int, tok: torch.Tensor, lens, image_of, out: torch.Tensor,
                       check: bool = True) -> torch.Tensor:
        """gitmi_generate_prefixed with a kind that is not a search (score, attend, score_tree): `out` is its logprob_out.
        -> info int32 [4] of the finished call; check False: info[3] (sentences rejected or non-finite) is the caller's to read."""
        Q, L = tok.shape
        info = self._empty(4, torch.int32, tok.device)
        search = GitmiSearch()
        search.kind = kind
        self._done(self._call(frames, self.lib.gitmi_generate_prefixed(
            self._h, arr, len(keep), B, tok.data_ptr(), L, *_sentence_tables(lens, image_of), Q, C.byref(search), None,
            out.data_ptr(), None, info.data_ptr(), _stream()), B), info, check)
        if not check:
            torch.cuda.current_stream().synchronize()
        return info

    # -- search seam ---------------------------------------------------------------------------
    def search_begin(self, search: GitmiSearch, start: torch.Tensor, vocab: int) -> None:
        start = start.to("cpu", torch.int64).contiguous()
        B, P = start.shape
        self._ck(self.lib.gitmi_search_begin(self._h, C.byref(search), B, start.data_ptr(), P, vocab, _stream()))
        self._search_k = search.beam_size
        self._search_B = B
        self._search_T = search.max_steps
        self._search_cfg = search

    def search_rows(self) -> torch.Tensor:
        R, t = C.c_int(), C.c_int()
        self._ck(self.lib.gitmi_search_rows(self._h, None, C.byref(R), C.byref(t), _stream()))
        out = torch.empty(R.value, t.value, device=f"cuda:{self.device}", dtype=torch.int64)
        self._ck(self.lib.gitmi_search_rows(self._h, out.data_ptr(), C.byref(R), C.byref(t), _stream()))
        return out

    def search_advance(self, logits: torch.Tensor) -> None:
        logits = logits.to(device=f"cuda:{self.device}", dtype=torch.float32).contiguous()
        self._keep_logits = logits
        self._ck(self.lib.gitmi_search_advance(self._h, logits.data_ptr(), _stream()))

    def set_trie(self, child_off, child_tok, child_node) -> None:
        """Token trie of the "trie" search kind as CSR int32 arrays (include/gitmi.h gitmi_set_trie); None removes it."""
        if child_off is None:
            self._ck(self.lib.gitmi_set_trie(self._h, 0, None, None, None))
            return
        off = torch.as_tensor(child_off, dtype=torch.int32).cpu().contiguous()
        tok = torch.as_tensor(child_tok, dtype=torch.int32).cpu().contiguous()
        node = torch.as_tensor(child_node, dtype=torch.int32).cpu().contiguous()
        assert off.numel() >= 2 and tok.numel() == node.numel() == int(off[-1])
        self._ck(self.lib.gitmi_set_trie(self._h, int(off.numel()) - 1, off.data_ptr(), tok.data_ptr() if tok.numel() else None,
                                    node.data_ptr() if node.numel() else None))

    # -- error attribution hooks (tools/error_attribution.py) ---------------------------------------
    def debug_import_stage(self, src: "Engine", stage: int) -> None:
        """Take the image features (stage 1) or features + image K/V of every decoder layer (stage 2) from `src`, a
        context of the same model in the other precision; step_logits() then continues from there."""
        self._ck(_experiment_only(self.lib, "gitmi_debug_import_stage")(self._h, src._h, int(stage), _stream()))
        self._resident = src._resident
        self._generation += 1

    def debug_head_from(self, src: "Engine", R: int) -> torch.Tensor:
        """This (bf16) context's fused vocabulary head on the last hidden state of src's (fp32) latest step_logits."""
        out = torch.empty(R, self.c.vocab, device=f"cuda:{self.device}", dtype=torch.float32)
        self._ck(_experiment_only(self.lib, "gitmi_debug_head_from")(self._h, src._h, int(R), out.data_ptr(), _stream()))
        torch.cuda.current_stream().synchronize()
        return out

    # -- op hooks of the search step (measurement build; tests/test_gpu_search_ops.py) ------------------------
    def debug_search_begin_prefixed(self, search: GitmiSearch, prefixes: Sequence[Sequence[int]], vocab: int) -> None:
        """search_begin with a prefix of its own length per sentence (every sentence = its own batch-1 reference call)."""
        start = id_table(prefixes)
        B, ld = start.shape
        plen = torch.tensor([len(p) for p in prefixes], dtype=torch.int32)
        self._ck(_experiment_only(self.lib, "gitmi_debug_search_begin_prefixed")(
            self._h, C.byref(search), B, start.data_ptr(), ld, plen.data_ptr(), vocab, _stream()))
        self._search_k, self._search_B, self._search_T, self._search_cfg = search.beam_size, B, search.max_steps, search

    def debug_search_advance_lists(self, part_val: torch.Tensor, part_idx: torch.Tensor, part_lse: torch.Tensor,
                                   embed: bool = False) -> None:
        """search_advance on candidate lists in the fused head's format -- part_val fp32 / part_idx int32 [R, nparts, slots],
        part_lse fp32 [R, nparts, 2] -- in place of logits: the multi-part merge of the search step."""
        dev = f"cuda:{self.device}"
        pv = part_val.to(device=dev, dtype=torch.float32).contiguous()
        pi = part_idx.to(device=dev, dtype=torch.int32).contiguous()
        pl = part_lse.to(device=dev, dtype=torch.float32).contiguous()
        R, nparts, slots = pv.shape
        if pi.shape != pv.shape or tuple(pl.shape) != (R, nparts, 2) or R != self._search_B * self._search_k:
            raise ValueError(f"candidate lists {tuple(pv.shape)} / {tuple(pi.shape)} / {tuple(pl.shape)} do not describe the "
                             f"{self._search_B * self._search_k} rows of the search")
        self._keep_lists = (pv, pi, pl)
        self._ck(_experiment_only(self.lib, "gitmi_debug_search_advance_lists")(
            self._h, pv.data_ptr(), pi.data_ptr(), pl.data_ptr(), nparts, slots, 1 if embed else 0, _stream()))

    def debug_read_hidden(self, R: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The embedded rows of the most recent step: (h_f fp32 [R, D], the compute-type copy [R, D] in row-major order)."""
        D = int(self.c.dec_hidden)
        dev = f"cuda:{self.device}"
        Rp = (R + 15) // 16 * 16
        hf = torch.empty(R, D, device=dev, dtype=torch.float32)
        raw = torch.empty(Rp * D * 4, device=dev, dtype=torch.uint8)
        frag, dt = C.c_int(), C.c_int()
        self._ck(_experiment_only(self.lib, "gitmi_debug_read_hidden")(self._h, int(R), hf.data_ptr(), raw.data_ptr(),
                                                                       C.byref(frag), C.byref(dt), _stream()))
        tdt = {DTYPE_F32: torch.float32, DTYPE_BF16: torch.bfloat16, DTYPE_F16: torch.float16}[dt.value]
        ht = raw.view(tdt)[:Rp * D].reshape(Rp, D)
        return hf, (from_frag(ht, R) if frag.value else ht[:R].contiguous())

    def search_done_count(self) -> int:
        """Sentences of the running search that need no further step (synchronises the stream)."""
        n = C.c_int()
        self._ck(self.lib.gitmi_search_done_count(self._h, C.byref(n), _stream()))
        return int(n.value)

    def search_finish(self):
        dev = f"cuda:{self.device}"
        tokens, logprobs, info = self._out(self._search_B, self._search_cfg, dev)
        self._ck(self.lib.gitmi_search_finish(self._h, tokens.data_ptr(), logprobs.data_ptr(), info.data_ptr(), _stream()))
        torch.cuda.current_stream().synchronize()
        return tokens, logprobs, info

    # -- profiling -----------------------------------------------------------------------------
    def profile_enable(self, on) -> None:
        """False/0 off; True/1 eager launches with per-launch HIP events; 2 graph replays split into an
        (encode + prefill) graph and a decode graph with events between them."""
        self._ck(self.lib.gitmi_profile_enable(self._h, int(on)))

    def profile_read(self) -> Dict[str, float]:
        p = GitmiProfile()
        self._ck(self.lib.gitmi_profile_read(self._h, C.byref(p)))
        return p.as_dict()

    def set_shared_device(self, on: bool = True) -> None:
        """Serving policy: other contexts run beside this one (kernel shapes by whole-device cost; bit-identical results).
        Clones made afterwards inherit it."""
        self._ck(self.lib.gitmi_set_shared_device(self._h, 1 if on else 0))

    def set_encode_after(self, other: Optional["Engine"]) -> None:
        """Serving schedule: this context's image encoder starts only after `other`'s (most recently submitted) has
        finished; chain contexts in a ring in submission order (one encoder in flight, decode chains fill in)."""
        self._ck(self.lib.gitmi_set_encode_after(self._h, other._h if other is not None else None))

    def set_temporal_embedding(self, on: bool) -> None:
        """on (default): frames come as a list -> frame i gets img_temperal_embedding[i]; off: a bare image tensor
        (decoder.py:845-857 adds the embedding only in the list branch)."""
        self._ck(self.lib.gitmi_set_temporal_embedding(self._h, 1 if on else 0))
        if bool(on) != self._temb:
            self._temb = bool(on)
            self._drop_resident()

    def set_ln_fold(self, on: bool) -> None:
        """fp16-operand library only: fold the encoder's / prefill's LayerNorms into the GEMMs either side of them (default
        there) or run one LayerNorm launch per module.  Raises if `on` is asked of an engine that cannot fold."""
        self._ck(self.lib.gitmi_set_ln_fold(self._h, 1 if on else 0))
        if bool(on) != self._ln_fold:
            self._ln_fold = bool(on)
            self._drop_resident()

    def set_graph(self, on: bool) -> None:
        self._ck(self.lib.gitmi_set_graph(self._h, 1 if on else 0))


# ---- single-kernel entry points (unit parity tests) -----------------------------------------------
def op_context_embed(tokens: torch.Tensor, lengths: Sequence[int], image_of: Optional[Sequence[int]], words: torch.Tensor,
                     positions: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, feats: torch.Tensor,
                     n_img: int, want_f32: bool = False, operands: Optional[str] = None):
    """The context kernel of GITMI_SEARCH_CONTEXT on its own (measurement build, include/gitmi_experiment.h): tokens int64
    [Q, ld] on the device, lengths / image_of as Engine.encode_context takes them; feats [B, stride, D] (fp32 or the 16-bit operand
    type) is updated IN PLACE: context rows behind the n_img image rows of every block, zeros behind them.
    -> (ntok int32 [B], the fp32 copy [B, stride, D] of the rows written (zeros elsewhere) or None)"""
    assert tokens.is_cuda and tokens.dtype == torch.int64 and tokens.is_contiguous() and feats.is_cuda and feats.is_contiguous()
    B, stride, D = feats.shape
    Q, ld = tokens.shape
    lib = _exp_library(feats.dtype, operands=operands)
    fn = _experiment_only(lib, "gitmi_debug_context_embed")
    f32 = lambda t: t.to(device=feats.device, dtype=torch.float32).contiguous()
    words, positions, gamma, beta = f32(words), f32(positions), f32(gamma), f32(beta)
    ntok = torch.full((B,), -1, dtype=torch.int32, device=feats.device)
    copy = torch.zeros(B, stride, D, dtype=torch.float32, device=feats.device) if want_f32 else None
    lens, img = _sentence_tables([int(v) for v in lengths], image_of)
    _ck(fn(tokens.data_ptr(), ld, lens, img, Q, words.data_ptr(), int(words.shape[0]), positions.data_ptr(), int(positions.shape[0]),
           gamma.data_ptr(), beta.data_ptr(), float(eps), feats.data_ptr(), _torch_dtype_code(feats), _ptr(copy), ntok.data_ptr(),
           B, int(n_img), stride, D, _stream()), lib)
    return ntok, copy


def op_gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
            residual: Optional[torch.Tensor] = None, act: int = ACT_NONE,
            out_dtype: torch.dtype = torch.float32, stream_rows: bool = False) -> torch.Tensor:
    """C = act(A W^T + bias) + residual in one of three epilogues: fp32 (out_dtype float32), the operands' 16-bit type
    (out_dtype = A.dtype), or fp16 residual-stream rows (stream_rows=True: C fp16 and the residual fp16 [M, N] rows).
    fp16 operands run in libgitmi_f16.so, bf16 ones in libgitmi.so; fp32 A / W with a 16-bit out_dtype run in that type's
    library."""
    assert A.is_cuda and W.is_cuda and A.dtype == W.dtype and A.is_contiguous() and W.is_contiguous()
    M, K = A.shape
    N = W.shape[0]
    if stream_rows:
        if A.dtype == torch.float32:
            raise GitmiError("op_gemm: fp16 stream rows need 16-bit operands")
        if residual is not None and (residual.dtype != torch.float16 or residual.shape != (M, N) or not residual.is_contiguous()):
            raise GitmiError("op_gemm: the stream form's residual is contiguous fp16 [M, N] rows")
        lib, out_code, out_dtype = _op_library(A.dtype), DTYPE_F16_STREAM, torch.float16
    else:
        if residual is not None and residual.dtype != torch.float32:
            raise GitmiError("op_gemm: the residual is fp32 (fp16 rows: stream_rows=True)")
        lib = _op_library(A.dtype, out_dtype, fp32_ok=True)
        out_code = {torch.float32: DTYPE_F32, torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_F16}[out_dtype]
    out = torch.empty(M, N, device=A.device, dtype=out_dtype)
    _ck(lib.gitmi_op_gemm(A.data_ptr(), W.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), M, N, K, K, N,
                          _torch_dtype_code(A), out_code, act, _stream()), lib)
    return out


def op_gemm_ln(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], *, colsum: Optional[torch.Tensor] = None,
               ln_part: Optional[torch.Tensor] = None, ln_eps: float = 1e-5, residual: Optional[torch.Tensor] = None,
               res_part: Optional[torch.Tensor] = None, res_gamma: Optional[torch.Tensor] = None,
               res_beta: Optional[torch.Tensor] = None, res_eps: float = 1e-12, want_part: bool = False, act: int = ACT_NONE):
    """The folded-LayerNorm forms of the large-M GEMM (fp16-operand library): consumer (ln_part given) or producer; returns C
    (fp16 [M, N]) and, for a producer with want_part, the row partials float [M, 4, 2]."""
    lib = load_library("f16")
    assert A.dtype == torch.float16 and W.dtype == torch.float16 and A.is_contiguous() and W.is_contiguous()
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty(M, N, device=A.device, dtype=torch.float16)
    part = torch.zeros(M, 4, 2, device=A.device, dtype=torch.float32) if want_part else None
    _ck(lib.gitmi_op_gemm_ln(A.data_ptr(), W.data_ptr(), _ptr(bias), _ptr(colsum), _ptr(ln_part), ln_eps, _ptr(residual),
                             _ptr(res_part), _ptr(res_gamma), _ptr(res_beta), res_eps, out.data_ptr(), _ptr(part), M, N, K, act,
                             _stream()), lib)
    return (out, part) if want_part else out


def op_gemm_form(A: torch.Tensor, W: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, *, lda: Optional[int] = None,
                 ldc: Optional[int] = None, bias=None, res=None, ldr: int = 0, act: int = ACT_NONE, stream_rows: bool = False,
                 shared: bool = False, ln_part=None, colsum=None, ln_eps: float = 1e-5, part_out=None, res_part=None,
                 res_gamma=None, res_beta=None, res_eps: float = 1e-5, operands: Optional[str] = None) -> None:
    """One launch_gemm with everything the engine's gemm_args / gemm_run / ln_gemm / gemm_to_stream set (measurement build;
    gitmi_debug_gemm_form): A / W / C / bias / res / colsum may be VIEWS that start inside larger buffers (a column slice: ldc > N),
    C and part_out are caller-supplied and pre-filled.  A, W fp32 or one 16-bit type (that type's measurement build; fp32: the
    one `operands` names, bf16 by default); C fp32, the operand type, or -- stream_rows -- fp16 residual-stream rows with an fp16
    residual.  Tile heights and XCD partitions are forced through set_gemm_impl."""
    if A.dtype != W.dtype:
        raise GitmiError(f"operands must share one type, got {A.dtype} / {W.dtype}")
    lib = _exp_library(A.dtype, *(() if stream_rows else (C.dtype,)), operands=operands)
    out_code = DTYPE_F16_STREAM if stream_rows else _torch_dtype_code(C)
    _ck(_experiment_only(lib, "gitmi_debug_gemm_form")(
        A.data_ptr(), int(K if lda is None else lda), W.data_ptr(), _ptr(bias), _ptr(res), int(ldr), C.data_ptr(),
        int(N if ldc is None else ldc), int(M), int(N), int(K), int(act), _torch_dtype_code(A), out_code, int(bool(shared)),
        _ptr(ln_part), _ptr(colsum), float(ln_eps), _ptr(part_out), _ptr(res_part), _ptr(res_gamma), _ptr(res_beta), float(res_eps),
        _stream()), lib)


def op_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                 out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """y = LayerNorm(x) of fp32 rows, written in out_dtype: fp32, or a 16-bit type (run in that type's library)."""
    lib = _op_library(out_dtype, fp32_ok=True)
    rows, D = x.shape
    out = torch.empty(rows, D, device=x.device, dtype=out_dtype)
    _ck(lib.gitmi_op_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, out.data_ptr(), None, rows, D,
                               _torch_dtype_code(out), _stream()), lib)
    return out


def op_attention(qkv: torch.Tensor, B: int, N: int, H: int, impl: int) -> torch.Tensor:
    lib = _op_library(qkv.dtype, fp32_ok=True)
    assert qkv.is_cuda and qkv.is_contiguous() and qkv.shape == (B * N, 3 * H * 64)
    out = torch.empty(B * N, H * 64, device=qkv.device, dtype=qkv.dtype)
    _ck(lib.gitmi_op_attention(qkv.data_ptr(), out.data_ptr(), B, N, H, _torch_dtype_code(qkv), impl, _stream()), lib)
    return out


def strip_stats(x: torch.Tensor) -> torch.Tensor:
    """Row partials of a [M, N] fp32 tensor per 16-column strip, in the layout the decode-chain kernels exchange:
    [N/16][M][2] = (sum, sum of squares)."""
    M, N = x.shape
    xs = x.float().reshape(M, N // 16, 16)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).permute(1, 0, 2).contiguous()


def to_frag(x: torch.Tensor, row_multiple: int = 16) -> torch.Tensor:
    """Row-major bf16 [R, K] -> the fragment-major operand layout of the decode chain (include/gitmi.h): 16-row x
    32-k tiles in MFMA operand order, rows zero-padded to `row_multiple`.  ACTIVATION operands of the decode-chain kernels
    must be padded to 64 rows: the wide GEMMs and the vocabulary head load four 16-row tiles at a time whatever M is
    (rows past M are loaded, never stored)."""
    R, K = x.shape
    Rp = (R + row_multiple - 1) // row_multiple * row_multiple
    xp = torch.zeros(Rp, K, dtype=x.dtype, device=x.device)
    xp[:R] = x
    return xp.reshape(Rp // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(Rp, K)


def from_frag(xf: torch.Tensor, rows: int) -> torch.Tensor:
    Rp, K = xf.shape
    return xf.reshape(Rp // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(Rp, K)[:rows].contiguous()


def _pad_vec(v: Optional[torch.Tensor], n: int) -> Optional[torch.Tensor]:
    if v is None:
        return None
    out = torch.zeros(n, dtype=v.dtype, device=v.device)
    out[:v.numel()] = v
    return out


def op_dgemm(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, colsum: Optional[torch.Tensor] = None,
             stats: Optional[torch.Tensor] = None, eps: float = 1e-12, act: int = ACT_NONE,
             frag_out: bool = False, packed: bool = False, strips_per_wg: int = 0) -> torch.Tensor:
    """Decode-chain GEMM, QKV / FFN1 form (kernels_dgemm.hip): 16-bit A [M,K], W [N,K] -> [M,N] in the same type (bf16:
    libgitmi.so, fp16: libgitmi_f16.so).
    With `stats` ([K/16][M][2] strip partials of the raw rows behind A) the LayerNorm in front of the GEMM is folded:
    out = rstd * (A W^T - mean * colsum) + bias.  Operands are given row-major and packed here (packed=True: A, W are
    already fragment-major and M, N are taken from bias / stats)."""
    lib = _op_library(A.dtype, W.dtype)
    if packed:
        Af, Wf, M, N, K = A, W, int(A.shape[0]), int(bias.numel()), int(A.shape[1])
        if stats is not None:
            M = int(stats.shape[1])
    else:
        M, K = A.shape
        N = W.shape[0]
        Af, Wf = to_frag(A, 64), to_frag(W)
    out = torch.empty((M + 15) // 16 * 16 if frag_out else M, N, device=A.device, dtype=A.dtype)
    strips = 0 if stats is None else int(stats.shape[0])
    _ck(lib.gitmi_op_dgemm(Af.data_ptr(), Wf.data_ptr(), bias.data_ptr(), _ptr(colsum), _ptr(stats), strips, eps,
                           out.data_ptr(), 1 if frag_out else 0, M, N, K, act, int(strips_per_wg), _stream()), lib)
    return from_frag(out, M) if (frag_out and not packed) else out


def op_dgemm_res(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, res_x: torch.Tensor,
                 res_stats: Optional[torch.Tensor] = None, res_gamma: Optional[torch.Tensor] = None,
                 res_beta: Optional[torch.Tensor] = None, res_eps: float = 1e-12, packed: bool = False):
    """Decode-chain GEMM, N = hidden form: x = A W^T + bias + residual, where the residual is `res_x` itself or
    LayerNorm(res_x) rebuilt from its strip partials.  -> (x fp32 [M,N], copy in A's 16-bit type, strip partials of x)."""
    lib = _op_library(A.dtype, W.dtype)
    M, N = res_x.shape
    K = A.shape[1]
    Af, Wf = (A, W) if packed else (to_frag(A, 64), to_frag(W))
    x = torch.empty(M, N, device=A.device, dtype=torch.float32)
    xb = torch.empty((M + 15) // 16 * 16, (N + 31) // 32 * 32, device=A.device, dtype=A.dtype)
    st = torch.empty(N // 16, M, 2, device=A.device, dtype=torch.float32)
    strips = 0 if res_stats is None else int(res_stats.shape[0])
    _ck(lib.gitmi_op_dgemm_res(Af.data_ptr(), Wf.data_ptr(), bias.data_ptr(), res_x.data_ptr(), _ptr(res_stats), strips,
                               _ptr(res_gamma), _ptr(res_beta), res_eps, x.data_ptr(), xb.data_ptr(), st.data_ptr(),
                               M, N, K, _stream()), lib)
    return x, (xb if packed else from_frag(xb, M)[:, :N].contiguous()), st


def op_dgemm_form(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, M: Optional[int] = None, *, colsum=None, stats=None,
                  eps: float = 1e-12, act: int = ACT_NONE, frag_out: bool = False, out: Optional[torch.Tensor] = None,
                  res_x=None, res_stats=None, res_gamma=None, res_beta=None, res_eps: float = 1e-12, x=None, xb=None,
                  stats_out=None, packed: bool = False, rows_per_wg: int = 0, strips_per_wg: int = 0, no_row_walk: int = 0):
    """op_dgemm / op_dgemm_res through the launcher with the three fields the engine's dgemm() sets by policy (measurement
    build): rows_per_wg, strips_per_wg, no_row_walk.  res_x given: the N = hidden form -> (x, xb, stats_out), else the QKV /
    FFN1 form -> out.  The outputs may be supplied (pre-filled, with guard rows behind them) by the caller; xb and a frag_out
    `out` come back as the raw fragment-major buffers (from_frag decodes them; xb is round_up(N, 32) columns wide).  packed=True: A (rows a multiple of 64) and W are
    fragment-major already and M is required; otherwise they are packed here and M is A's row count."""
    lib = _exp_library(A.dtype, W.dtype)
    own = A.dtype
    if own == torch.float32:
        raise GitmiError(f"operands must be bf16 or fp16, got {A.dtype} / {W.dtype}")
    if packed:
        if M is None:
            raise ValueError("packed operands: M is required")
        Af, Wf = A, W
    else:
        M = int(A.shape[0]) if M is None else int(M)
        Af, Wf = to_frag(A, 64), to_frag(W)
    M, N, K = int(M), int(bias.numel()), int(A.shape[1])
    Mp = (M + 15) // 16 * 16
    producer = res_x is not None
    if producer:
        x = torch.empty(M, N, device=A.device, dtype=torch.float32) if x is None else x
        xb = torch.empty(Mp, (N + 31) // 32 * 32, device=A.device, dtype=own) if xb is None else xb
        stats_out = torch.empty(N // 16, M, 2, device=A.device, dtype=torch.float32) if stats_out is None else stats_out
    elif out is None:
        out = torch.empty(Mp if frag_out else M, N, device=A.device, dtype=own)
    _ck(_experiment_only(lib, "gitmi_debug_dgemm_form")(
        Af.data_ptr(), int(Af.shape[0]), Wf.data_ptr(), _ptr(bias), _ptr(colsum), _ptr(stats),
        0 if stats is None else int(stats.shape[0]), eps, _ptr(out), int(bool(frag_out)), int(act), _ptr(res_x), _ptr(res_stats),
        0 if res_stats is None else int(res_stats.shape[0]), _ptr(res_gamma), _ptr(res_beta), res_eps, _ptr(x), _ptr(xb),
        _ptr(stats_out), M, N, K, int(rows_per_wg), int(strips_per_wg), int(no_row_walk), _stream()), lib)
    return (x, xb, stats_out) if producer else out


def _vocab_head_call(A, W, bias, mtop, cols_per_wg, colsum, stats, want_logits, packed, rows, V, measurement=False):
    """What op_vocab_topm and op_vocab_topm_rules share: the library of the operands' type (measurement: its measurement
    build), the packed operands and the output buffers -> (lib, leading arguments (A .. mtop) of the C entry point, trailing
    arguments, outputs)."""
    lib = _exp_library(A.dtype, W.dtype) if measurement else _op_library(A.dtype, W.dtype)
    K = A.shape[1]
    V = int(bias.numel()) if V is None else int(V)
    if packed:
        Af, Wf, M, bp, cp = A, W, int(rows), bias, colsum
    else:
        M = A.shape[0]
        Vp = (V + cols_per_wg - 1) // cols_per_wg * cols_per_wg
        Af, Wf, bp, cp = to_frag(A, 64), to_frag(W, cols_per_wg), _pad_vec(bias, Vp), _pad_vec(colsum, Vp)
    nparts = (V + cols_per_wg - 1) // cols_per_wg
    slots = 1 if mtop <= 1 else 2 if mtop <= 2 else 4 if mtop <= 4 else 8 if mtop <= 8 else 16
    pv = torch.empty(M, nparts, slots, device=A.device, dtype=torch.float32)
    pi = torch.empty(M, nparts, slots, device=A.device, dtype=torch.int32)
    pl = torch.empty(M, nparts, 2, device=A.device, dtype=torch.float32)
    lg = torch.empty(M, V, device=A.device, dtype=torch.float32) if want_logits else None
    strips = 0 if stats is None else int(stats.shape[0])
    keep = (Af, Wf, bp, cp)                                  # alive until the call has been enqueued
    return lib, M, (Af.data_ptr(), Wf.data_ptr(), bp.data_ptr(), _ptr(cp), _ptr(stats), strips), (M, V, K, cols_per_wg, mtop), \
        (pv.data_ptr(), pi.data_ptr(), pl.data_ptr(), _ptr(lg)), (pv, pi, pl, lg), keep


def op_vocab_topm(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, mtop: int, cols_per_wg: int = 128,
                  colsum: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None, eps: float = 1e-12,
                  suppress_tok: Optional[torch.Tensor] = None, want_logits: bool = False, packed: bool = False,
                  rows: Optional[int] = None, V: Optional[int] = None, max_wgs: int = 0):
    """Vocabulary head with the fused running top-M / log-sum-exp: -> (part_val [M, nparts, slots], part_idx,
    part_lse [M, nparts, 2] = (max, sum exp), logits [M, V] or None).  packed=True: A / W fragment-major (W rows and
    bias / colsum padded to a multiple of cols_per_wg), `rows` = M, `V` = vocabulary size.  A / W: bf16 or fp16 (that
    type's library)."""
    lib, _, ops, shape, outs, result, keep = _vocab_head_call(A, W, bias, mtop, cols_per_wg, colsum, stats, want_logits, packed, rows, V)
    _ck(lib.gitmi_op_vocab_topm(*ops, eps, *shape, _ptr(suppress_tok), *outs, int(max_wgs), _stream()), lib)
    return result


def op_vocab_topm_rules(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, mtop: int, ids: Optional[torch.Tensor],
                        cur_len: int, plen: Optional[torch.Tensor], beams: int = 1, suppress_kind: int = 0,
                        rep_penalty: float = 0.0, cols_per_wg: int = 128, colsum: Optional[torch.Tensor] = None,
                        stats: Optional[torch.Tensor] = None, eps: float = 1e-12, want_logits: bool = False, packed: bool = False,
                        rows: Optional[int] = None, V: Optional[int] = None, max_wgs: int = 0, ban: Optional["DebugBan"] = None,
                        out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = None):
    """op_vocab_topm with the rule inputs of a real search step (measurement build): ids int32 [M, ld_ids] row histories of
    cur_len tokens, plen int32 [M / beams] prefix lengths, suppress_kind (no immediate repeat on rows with cur_len > plen),
    rep_penalty.  Same outputs; the materialised logits are taken before the rules -- but after the ban of `ban` (DebugBan: the
    rows' decoding constraints), which they carry as -10000.  out: caller-supplied (part_val, part_idx, part_lse, logits or None)
    in place of fresh ones."""
    lib, M, ops, shape, outs, result, keep = _vocab_head_call(A, W, bias, mtop, cols_per_wg, colsum, stats, want_logits, packed, rows, V,
                                                              measurement=True)
    if ids is not None:
        ids = ids.to(device=A.device, dtype=torch.int32).contiguous()
        plen = plen.to(device=A.device, dtype=torch.int32).contiguous()
        if ids.dim() != 2 or ids.shape[0] != M or plen.numel() * beams != M:
            raise ValueError(f"ids {tuple(ids.shape)} / plen {tuple(plen.shape)} do not describe {M} rows of {beams} beams")
    if out is not None:
        result, outs = out, tuple(_ptr(t) for t in out)
    _ck(_experiment_only(lib, "gitmi_debug_vocab_topm_rules")(
        *ops, eps, *shape, _ptr(ids), 0 if ids is None else int(ids.shape[1]), int(cur_len), _ptr(plen), int(beams),
        int(suppress_kind), float(rep_penalty), *outs, int(max_wgs), _stream(), _ban_ref(ban)), lib)
    return result


def set_gemm_impl(impl: int) -> None:
    """Measurement build only (use_experiment_build()): -1 auto, 0 register-staged tile kernel only, 9 the LDS-DMA kernel
    wherever it can run; 9 | (bits << 8): 64 / 128 force its 192- / 256-row tile (tools/gemm_bench.py lists the others).
    The selector is a static of each library: it is set in the bf16 measurement build (loaded here, as before) and in the fp16
    one if that is loaded already; loaded later, it starts from the selector in force (load_library)."""
    global _gemm_impl
    lib = load_library()
    _ck(_experiment_only(lib, "gitmi_debug_set_gemm_impl")(int(impl)), lib)
    _gemm_impl = int(impl)
    other = _libs.get("f16_exp")
    if other is not None and other is not lib:
        _ck(other.gitmi_debug_set_gemm_impl(int(impl)), other)


def op_attn_decode(qkv, img_k, img_v, txt_k, txt_v, kv_src, B, H, N_img, T_max, pos, beams, dbg=0):
    """qkv [R,3d]; img_k/img_v [B,H,N_img,64]; txt_k/txt_v [R,T_max,d] (position pos gets appended); kv_src int32 [R,T_max].
    All fp32, or all in one 16-bit type (that type's library; image K/V head-major or already in kv_repack's layouts)."""
    lib = _op_library(qkv.dtype, img_k.dtype, img_v.dtype, txt_k.dtype, txt_v.dtype, fp32_ok=True)
    R, d = B * beams, H * 64
    out = torch.empty(R, d, device=qkv.device, dtype=qkv.dtype)
    if qkv.dtype != torch.float32 and img_k.dim() == 4:
        # head-major [B,H,N,64] given: build the prefill-layout rows and repack into the matrix-core layouts
        img_k, img_v = kv_repack(img_k, img_v)
    _ck(lib.gitmi_op_attn_decode(qkv.data_ptr(), img_k.data_ptr(), img_v.data_ptr(), txt_k.data_ptr(), txt_v.data_ptr(),
                                 kv_src.data_ptr(), out.data_ptr(), B, H, N_img, T_max, pos, beams, _torch_dtype_code(qkv),
                                 dbg, _stream()), lib)
    return out


def op_attention_ragged(qkv: torch.Tensor, ntok, B: int, N: int, H: int, impl: int) -> torch.Tensor:
    """op_attention with per-image row counts ntok [B] (measurement build): keys past ntok[b] unused, their queries zeros."""
    lib = load_library()
    nt = torch.as_tensor(ntok, dtype=torch.int32).to(qkv.device)
    out = torch.empty(B * N, H * 64, device=qkv.device, dtype=qkv.dtype)
    _ck(_experiment_only(lib, "gitmi_debug_attention_ragged")(qkv.data_ptr(), out.data_ptr(), nt.data_ptr(), B, N, H,
                                                              _torch_dtype_code(qkv), impl, _stream()), lib)
    return out


def op_attn_decode_ragged(qkv, img_k, img_v, txt_k, txt_v, kv_src, ntok, B, H, N_img, T_max, pos, beams):
    """op_attn_decode with per-image key counts ntok [B] (measurement build)."""
    lib = load_library()
    R, d = B * beams, H * 64
    nt = torch.as_tensor(ntok, dtype=torch.int32).to(qkv.device)
    out = torch.empty(R, d, device=qkv.device, dtype=qkv.dtype)
    if qkv.dtype != torch.float32 and img_k.dim() == 4:
        img_k, img_v = kv_repack(img_k, img_v)
    _ck(_experiment_only(lib, "gitmi_debug_attn_decode_ragged")(qkv.data_ptr(), img_k.data_ptr(), img_v.data_ptr(), txt_k.data_ptr(),
                                                                txt_v.data_ptr(), kv_src.data_ptr(), out.data_ptr(), nt.data_ptr(), B,
                                                                H, N_img, T_max, pos, beams, _torch_dtype_code(qkv), _stream()), lib)
    return out


def op_attn_decode_form(qkv, img_k, img_v, txt_k, txt_v, kv_src, B, H, N_img, T_max, pos, beams, *, out=None, img_of=None,
                        ntok=None, out_frag=False, pairs_per_wg=0, waves_per_pair=0, stream_wgs=0, operands=None):
    """op_attn_decode through the launcher with everything the engine's decode step sets (measurement build): img_of [B]
    sentence -> image (img_k / img_v / ntok are per image), ntok per-image key counts, out_frag (the fragment-major rows of the
    decode chain: the raw round_up(R, 16)-row buffer comes back, from_frag decodes it), pairs_per_wg / waves_per_pair /
    stream_wgs as in AttnDecodeArgs.  txt_k / txt_v are appended to in place; `out` may be supplied (pre-filled) by the caller.
    All in one 16-bit type (that type's measurement build), or all fp32 (the build `operands` names, bf16 by default)."""
    lib = _exp_library(qkv.dtype, img_k.dtype, img_v.dtype, txt_k.dtype, txt_v.dtype,
                       operands=operands if qkv.dtype == torch.float32 else None)
    R, d = B * beams, H * 64
    n_images = img_k.shape[0] if img_k.dim() == 4 else img_k.numel() // (H * ((N_img + 31) // 32 * 32) * 64)
    if qkv.dtype != torch.float32 and img_k.dim() == 4:
        img_k, img_v = kv_repack(img_k, img_v)
    if img_of is None:
        if n_images < B:
            raise ValueError(f"{n_images} images for {B} sentences and no img_of")
    else:
        host = torch.as_tensor(img_of, dtype=torch.int64).cpu()
        if host.numel() != B or int(host.min()) < 0 or int(host.max()) >= n_images:
            raise ValueError(f"img_of {host.tolist()} does not map {B} sentences onto {n_images} images")
        img_of = host.to(device=qkv.device, dtype=torch.int32)
    if ntok is not None:
        ntok = torch.as_tensor(ntok, dtype=torch.int32).to(qkv.device)
        if ntok.numel() != n_images:
            raise ValueError(f"ntok holds {ntok.numel()} counts for {n_images} images")
    if out is None:
        rows = (R + 15) // 16 * 16 if out_frag else R
        out = torch.empty(rows, d, device=qkv.device, dtype=qkv.dtype)
    _ck(_experiment_only(lib, "gitmi_debug_attn_decode_form")(
        qkv.data_ptr(), img_k.data_ptr(), img_v.data_ptr(), txt_k.data_ptr(), txt_v.data_ptr(), kv_src.data_ptr(), out.data_ptr(),
        _ptr(ntok), _ptr(img_of), n_images, B, H, N_img, T_max, pos, beams, _torch_dtype_code(qkv), int(bool(out_frag)),
        int(pairs_per_wg), int(waves_per_pair), int(stream_wgs), _stream()), lib)
    return out


def op_attn_decode_qkv(x, w, bias, img_k, img_v, txt_k, txt_v, kv_src, B, H, N_img, T_max, pos, beams=1, *, colsum=None, stats=None,
                       eps: float = 1e-12, out=None, img_of=None, ntok=None, out_frag=False, pairs_per_wg=8, waves_per_pair=1,
                       stream_wgs=0):
    """The decode attention that computes its own q | k | v (measurement build): op_attn_decode_form without qkv, plus the QKV
    GEMM's operands as op_dgemm_form(packed=True) takes them -- x fragment-major [>= round_up(B, 16), H * 64], w fragment-major
    [3 H 64, H 64], bias / colsum [3 H 64], stats [strips, B, 2] or None.  img_k / img_v in kv_repack's layouts (or head-major
    [images, H, N_img, 64]); txt_k / txt_v are appended to in place.  A call outside the form raises GitmiError."""
    lib = _exp_library(x.dtype, w.dtype, img_k.dtype, img_v.dtype, txt_k.dtype, txt_v.dtype)
    d = H * 64
    n_images = img_k.shape[0] if img_k.dim() == 4 else img_k.numel() // (H * ((N_img + 31) // 32 * 32) * 64)
    if img_k.dim() == 4:
        img_k, img_v = kv_repack(img_k, img_v)
    if img_of is not None:
        img_of = torch.as_tensor(img_of, dtype=torch.int32).to(x.device)
    if ntok is not None:
        ntok = torch.as_tensor(ntok, dtype=torch.int32).to(x.device)
    if out is None:
        out = torch.empty((B * beams + 15) // 16 * 16 if out_frag else B * beams, d, device=x.device, dtype=x.dtype)
    _ck(_experiment_only(lib, "gitmi_debug_attn_decode_qkv")(
        x.data_ptr(), int(x.shape[0]), w.data_ptr(), _ptr(bias), _ptr(colsum), _ptr(stats), 0 if stats is None else int(stats.shape[0]),
        eps, img_k.data_ptr(), img_v.data_ptr(), txt_k.data_ptr(), txt_v.data_ptr(), kv_src.data_ptr(), out.data_ptr(), _ptr(ntok),
        _ptr(img_of), n_images, B, H, N_img, T_max, pos, beams, _torch_dtype_code(x), int(bool(out_frag)), int(pairs_per_wg),
        int(waves_per_pair), int(stream_wgs), _stream()), lib)
    return out


def op_score_attn(qkv: torch.Tensor, img_kv: torch.Tensor, image_of: torch.Tensor, Q: int, H: int, N_img: int,
                  Lp: int) -> torch.Tensor:
    """Text attention of the score path (measurement build): qkv [Q * Lp, 3 H 64], img_kv [B * N_img, 3 H 64] (fp32 or the
    build's 16-bit dtype), image_of int [Q] -> [Q * Lp, H 64] in the input dtype."""
    lib = load_library()
    img = image_of.to(device=qkv.device, dtype=torch.int32).contiguous()
    out = torch.empty(Q * Lp, H * 64, device=qkv.device, dtype=qkv.dtype)
    _ck(_experiment_only(lib, "gitmi_debug_score_attn")(qkv.data_ptr(), img_kv.data_ptr(), img.data_ptr(), out.data_ptr(), Q, H,
                                                        N_img, Lp, _torch_dtype_code(qkv), _stream()), lib)
    return out


def op_score_attn_map(qkv: torch.Tensor, img_kv: torch.Tensor, image_of: torch.Tensor, Q: int, H: int, N_img: int, Lp: int,
                      ntok: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention map of one layer (measurement build): op_score_attn's operands, ntok int [B] (the image keys of every
    image; None: N_img each) -> fp32 [Q, Lp, N_img + Lp], the head mean of the probabilities of every text row."""
    lib = load_library()
    img = image_of.to(device=qkv.device, dtype=torch.int32).contiguous()
    nt = None if ntok is None else ntok.to(device=qkv.device, dtype=torch.int32).contiguous()
    out = torch.empty(Q, Lp, N_img + Lp, device=qkv.device, dtype=torch.float32)
    _ck(_experiment_only(lib, "gitmi_debug_score_attn_map")(qkv.data_ptr(), img_kv.data_ptr(), img.data_ptr(), _ptr(nt),
                                                            out.data_ptr(), Q, H, N_img, Lp, _torch_dtype_code(qkv), _stream()), lib)
    return out


def pack_trees(tokens, depths, lengths, vocab: int, max_depth: int):
    """Host side of Engine.score_tree: the rules of include/gitmi.h (GITMI_SEARCH_TREE_SCORE) checked on int [Q, L] tokens /
    depths -- depths[q, 0] == 0, 1 <= depths[q, i] <= depths[q, i - 1] + 1, depth < max_depth, ids in [0, vocab), lengths in [1, L]
    -- then the packed table.  Raises ValueError naming tree and node.
    -> (int64 [Q, L] on the CPU with depth << 32 | token, zeros past every length; lengths as a list)"""
    tok = torch.as_tensor(tokens).detach().to("cpu", torch.int64)
    dep = torch.as_tensor(depths).detach().to("cpu", torch.int64)
    if tok.dim() != 2 or tok.shape[1] < 1 or dep.shape != tok.shape:
        raise ValueError(f"tokens and depths must both be [Q, L], got {tuple(tok.shape)} and {tuple(dep.shape)}")
    Q, L = int(tok.shape[0]), int(tok.shape[1])
    lens = [L] * Q if lengths is None else [int(v) for v in lengths]
    if len(lens) != Q:
        raise ValueError(f"lengths has {len(lens)} entries for {Q} trees")
    for q, n in enumerate(lens):
        if n < 1 or n > L:
            raise ValueError(f"tree {q}: length {n} outside [1, {L}]")
    valid = torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]
    first = dep[:, 0] != 0
    if bool(first.any()):
        q = int(first.nonzero()[0])
        raise ValueError(f"tree {q}, node 0: the root must have depth 0, got {int(dep[q, 0])}")
    step = torch.zeros_like(valid)
    step[:, 1:] = (dep[:, 1:] < 1) | (dep[:, 1:] > dep[:, :-1] + 1)
    for wrong, what in ((step & valid, "must lie in [1, depth of the node before it + 1] (one root; a child is one level below)"),
                        ((dep >= max_depth) & valid, f"must be below {max_depth} (min(max_text_len, max_pos))")):
        if bool(wrong.any()):
            q, i = (int(v) for v in wrong.nonzero()[0])
            raise ValueError(f"tree {q}, node {i}: depth {int(dep[q, i])} {what}")
    ids = tok[valid]
    if int(ids.min()) < 0 or int(ids.max()) >= vocab:
        raise ValueError(f"token ids outside [0, {vocab})")
    table = torch.where(valid, (dep << 32) | tok, torch.zeros_like(tok)).contiguous()
    return table, lens


def op_score_attn_tree(qkv: torch.Tensor, img_kv: torch.Tensor, image_of: torch.Tensor, table: torch.Tensor, lens, max_depth: int,
                       Q: int, H: int, N_img: int, Lp: int, ntok: Optional[torch.Tensor] = None):
    """Tree attention of one layer (measurement build): op_score_attn's operands with the rows of every sentence the nodes of a
    token tree -- table int64 [Q, Lp] (pack_trees), lens int [Q] -> ([Q * Lp, H 64] in the input dtype, int32 [Q] verdicts:
    1 for a tree the structure launch rejected)."""
    lib = load_library()
    dev = qkv.device
    img = image_of.to(device=dev, dtype=torch.int32).contiguous()
    nt = None if ntok is None else ntok.to(device=dev, dtype=torch.int32).contiguous()
    tab = table.to(device=dev, dtype=torch.int64).contiguous()
    ln = torch.as_tensor(lens).to(device=dev, dtype=torch.int32).contiguous()
    if tuple(tab.shape) != (Q, Lp) or ln.numel() != Q:
        raise ValueError("table must be [Q, Lp] and lens [Q]")
    out = torch.empty(Q * Lp, H * 64, device=dev, dtype=qkv.dtype)
    bad = torch.empty(Q, device=dev, dtype=torch.int32)
    _ck(_experiment_only(lib, "gitmi_debug_score_attn_tree")(qkv.data_ptr(), img_kv.data_ptr(), img.data_ptr(), _ptr(nt),
                                                             tab.data_ptr(), ln.data_ptr(), max_depth, out.data_ptr(),
                                                             bad.data_ptr(), Q, H, N_img, Lp, _torch_dtype_code(qkv), _stream()),
        lib)
    return out, bad


def op_score_head(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """Vocabulary head of the score path with its log-softmax statistics (measurement build): A [M, K], W [V, K] (fp32 or the
    build's 16-bit dtype), bias fp32 [V], tgt int [M] (< 0: no target) -> fp32 [M, 2] = (lp, mean_lp)."""
    lib = load_library()
    M, K = A.shape
    V = W.shape[0]
    t = tgt.to(device=A.device, dtype=torch.int32).contiguous()
    out = torch.zeros(M, 2, device=A.device, dtype=torch.float32)
    _ck(_experiment_only(lib, "gitmi_debug_score_head")(A.data_ptr(), W.data_ptr(), bias.float().contiguous().data_ptr(),
                                                        t.data_ptr(), M, V, K, _torch_dtype_code(A), out.data_ptr(),
                                                        _stream()), lib)
    return out


# ---- op hooks of the text pass around its attention and head (measurement build; tests/test_gpu_text_pass_ops.py).  Every
# output is a caller-supplied device tensor, as for the front-end hooks below; operands as there.
def op_score_embed(tokens: torch.Tensor, Lp: int, words: torch.Tensor, positions: torch.Tensor, gamma: torch.Tensor,
                   beta: torch.Tensor, eps: float, h_f: torch.Tensor, h_t: torch.Tensor, node_tok: Optional[torch.Tensor] = None,
                   node_depth: Optional[torch.Tensor] = None, operands: Optional[str] = None) -> None:
    """tokens int64 [Q, ld] -> h_f fp32 / h_t (fp32 or the operand type) [Q * Lp, D]: the embedding + LayerNorm of every row of
    the text pass; node_tok / node_depth int32 [Q * Lp]: the tree instantiation (tokens is not read)."""
    lib, fn = _front("gitmi_debug_score_embed", h_t.dtype, operands=operands)
    Q, ld = tokens.shape
    _ck(fn(tokens.data_ptr(), Q, ld, Lp, words.data_ptr(), int(words.shape[0]), positions.data_ptr(), int(positions.shape[0]),
           gamma.data_ptr(), beta.data_ptr(), eps, int(words.shape[1]), h_f.data_ptr(), h_t.data_ptr(), _torch_dtype_code(h_t),
           _ptr(node_tok), _ptr(node_depth), _stream()), lib)


def op_tree_tables(packed: torch.Tensor, lens: torch.Tensor, Lp: int, V: int, max_depth: int, tables: torch.Tensor,
                   bad: torch.Tensor, operands: Optional[str] = None) -> None:
    """packed int64 [Q, ld] (depth << 32 | token), lens int32 [Q] -> tables int32 [4, Q * Lp] = (tok, depth, parent, end) of the
    structure launch and bad int32 [Q]."""
    lib, fn = _front("gitmi_debug_tree_tables", operands=operands)
    Q, ld = packed.shape
    if tuple(tables.shape) != (4, Q * Lp) or tables.dtype != torch.int32 or not tables.is_contiguous():
        raise ValueError("tables must be a contiguous int32 [4, Q * Lp]")
    _ck(fn(packed.data_ptr(), lens.data_ptr(), Q, ld, Lp, V, max_depth, tables[0].data_ptr(), tables[1].data_ptr(),
           tables[2].data_ptr(), tables[3].data_ptr(), bad.data_ptr(), _stream()), lib)


def op_score_tail(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, tokens: torch.Tensor, lens: torch.Tensor, Lp: int,
                  out: torch.Tensor, bad: torch.Tensor, info: torch.Tensor, chunk_rows: int = 0, tree_max_depth: int = 0,
                  tgt_out: Optional[torch.Tensor] = None, zt_out: Optional[torch.Tensor] = None,
                  operands: Optional[str] = None) -> None:
    """Everything behind the last decoder layer of a score (tree_max_depth = 0) or tree-score call: A [Q * Lp, K] text rows,
    W [V, K] (fp32 or the operand type), bias fp32 [V], tokens int64 [Q, ld] (or the packed tree table), lens int32 [Q] -> out
    fp32 [Q, ld, 2] (only the entries with a target / a parent are written), bad int32 [Q], info int32 [4]; tgt_out int32 /
    zt_out fp32 [Q * Lp]: the head rows' targets and gathered logits."""
    lib, fn = _front("gitmi_debug_score_tail", A.dtype, W.dtype, operands=operands)
    Q, ld = tokens.shape
    V, K = W.shape
    if tuple(A.shape) != (Q * Lp, K) or tuple(out.shape) != (Q, ld, 2) or bias.numel() != V or lens.numel() != Q:
        raise ValueError("A must be [Q * Lp, K], out [Q, ld, 2], bias [V], lens [Q]")
    _ck(fn(A.data_ptr(), W.data_ptr(), bias.data_ptr(), tokens.data_ptr(), lens.data_ptr(), Q, ld, Lp, V, K, _torch_dtype_code(A),
           int(chunk_rows), int(tree_max_depth), out.data_ptr(), bad.data_ptr(), info.data_ptr(), _ptr(tgt_out), _ptr(zt_out),
           _stream()), lib)


# ---- op hooks of the encoder's image front end (measurement build; tests/test_gpu_frontend_ops.py).  Every output is a
# caller-supplied device tensor (the tests put a sentinel-filled margin behind it); the launcher of encode_frames runs on it.
# operands ("bf16" | "f16"): the measurement build to run in, where no tensor of the call is in the 16-bit operand type (fp32
# and fp16-stream tensors exist in both builds); None: by the call's operand-type tensors, else bf16.
def _front(name: str, *dtypes: torch.dtype, operands: Optional[str] = None):
    lib = _exp_library(*dtypes, operands=operands)
    return lib, _experiment_only(lib, name)


def op_im2col(img: torch.Tensor, out: torch.Tensor, B: int, H: int, W: int, p: int, Kpad: int, operands: Optional[str] = None) -> None:
    """img fp32 [B, 3, H, W] (any 4-byte aligned view) -> out [B * (H // p) * (W // p), Kpad] patch rows, fp32 or the build's
    16-bit operand type, zeros past K = 3 p p."""
    lib, fn = _front("gitmi_debug_im2col", out.dtype, operands=operands)
    _ck(fn(img.data_ptr(), out.data_ptr(), _torch_dtype_code(out), B, H, W, p, 3 * p * p, Kpad, _stream()), lib)


def op_pos_resize(pos: torch.Tensor, out: torch.Tensor, g: int, gh: int, gw: int, operands: Optional[str] = None) -> None:
    """pos fp32 [g * g + 1, D] -> out fp32 [gh * gw + 1, D]: bicubic resize of the grid rows, class row copied."""
    lib, fn = _front("gitmi_debug_pos_resize", operands=operands)
    _ck(fn(pos.data_ptr(), out.data_ptr(), g, gh, gw, int(pos.shape[1]), _stream()), lib)


def op_vit_assemble(patch_out: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                    eps: float, X: torch.Tensor, B: int, N: int, part: Optional[torch.Tensor] = None,
                    operands: Optional[str] = None) -> None:
    """Class / patch rows + positional rows, ln_pre -> X [B * N, D] (fp32, or the fp16 stream when X is float16); part fp32
    [B * N, 4, 2]: the folded-LayerNorm partials (fp16 stream only)."""
    lib, fn = _front("gitmi_debug_vit_assemble", operands=operands)
    _ck(fn(patch_out.data_ptr(), cls.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, X.data_ptr(),
           1 if X.dtype == torch.float16 else 0, B, N, int(cls.numel()), _ptr(part), _stream()), lib)


def op_ragged_front(stage: int, B: int, p: int, max_pixels: int, Nmax: int, *, src=None, slots=None, meta=None, ntok=None,
                    patches=None, Kpad: int = 0, patch_out=None, cls=None, pos=None, g: int = 0, gamma=None, beta=None,
                    eps: float = 1e-5, X=None, part=None, operands: Optional[str] = None) -> None:
    """One stage of a ragged batch's front end on caller-supplied buffers: 0 staging (src -> slots, meta, ntok), 1 patch gather
    (slots, meta -> patches [B, Nmax - 1, Kpad]), 2 token assembly + ln_pre (patch_out, cls, pos, meta -> X [B * Nmax, D], part)."""
    lib, fn = _front("gitmi_debug_ragged_front", *(() if patches is None else (patches.dtype,)), operands=operands)
    _ck(fn(int(stage), _ptr(src), _ptr(slots), _ptr(meta), _ptr(ntok), _ptr(patches),
           DTYPE_F32 if patches is None else _torch_dtype_code(patches), _ptr(patch_out), _ptr(cls), _ptr(pos), int(g), _ptr(gamma),
           _ptr(beta), eps, _ptr(X), 1 if X is not None and X.dtype == torch.float16 else 0, _ptr(part), B, p, int(max_pixels), Nmax,
           3 * p * p, int(Kpad), 0 if cls is None else int(cls.numel()), _stream()), lib)


def op_zero_pad_rows(x: torch.Tensor, ntok: torch.Tensor, B: int, Nmax: int, ld: int, operands: Optional[str] = None) -> None:
    """Rows t >= ntok[b] of x [B, Nmax, ld] (fp32 or 16-bit elements) set to zero, in place."""
    lib, fn = _front("gitmi_debug_zero_pad_rows", operands=operands)
    _ck(fn(x.data_ptr(), 1 if x.dtype == torch.float32 else 0, ld, ntok.data_ptr(), B, Nmax, _stream()), lib)


def op_layernorm_map(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, add_after: Optional[torch.Tensor],
                     y_t: Optional[torch.Tensor], y_s: Optional[torch.Tensor], rows: int, D: int, map_n_in: int = 0,
                     map_n_out: int = 0, map_off: int = 0, operands: Optional[str] = None) -> None:
    """LayerNorm of `rows` rows of x (fp32, or fp16 stream rows) + add_after, scattered by the row map of ln_post: y_t fp32 or
    the build's 16-bit operand type, y_s the source's type (either may be None)."""
    lib, fn = _front("gitmi_debug_layernorm_map", *(() if y_t is None else (y_t.dtype,)), operands=operands)
    _ck(fn(x.data_ptr(), 1 if x.dtype == torch.float16 else 0, gamma.data_ptr(), beta.data_ptr(), eps, _ptr(add_after), _ptr(y_t),
           DTYPE_F32 if y_t is None else _torch_dtype_code(y_t), _ptr(y_s), rows, D, map_n_in, map_n_out, map_off, _stream()), lib)


def op_sample_rows(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, ndraw: int = 2,
                   seed: int = 0, step: int = 1, want_filtered: bool = True):
    """One step of the sampling branch (decoder.py:1146-1166) on fp32 logits [R, V]:
    -> (filtered logits [R, V] or None, draw tokens int32 [R, ndraw], their log-probs fp32 [R, ndraw])."""
    lib = load_library()
    logits = logits.float().contiguous()
    R, V = logits.shape
    lp = torch.empty(R, ndraw, device=logits.device, dtype=torch.float32)
    tok = torch.empty(R, ndraw, device=logits.device, dtype=torch.int32)
    filt = torch.empty(R, V, device=logits.device, dtype=torch.float32) if want_filtered else None
    _ck(lib.gitmi_op_sample_rows(logits.data_ptr(), R, V, float(temperature), int(top_k), float(top_p), int(ndraw), int(seed),
                                 int(step), lp.data_ptr(), tok.data_ptr(), _ptr(filt), _stream()), lib)
    return filt, tok, lp


# ---- op hooks of the whole-row selection kernels (measurement build; tests/test_gpu_select_ops.py).  logits: an fp32 device
# view [rows, >= V] with unit column stride; its row stride is ldl and its first V columns are the vocabulary (a padded or
# misaligned row is a slice of a wider tensor).  out: caller-supplied output tensors (the tests fill them with sentinels).
class _GitmiDebugBan(C.Structure):
    _fields_ = [("words", C.c_void_p), ("n_sets", C.c_int), ("W", C.c_int), ("set_of", C.c_void_p), ("min_new", C.c_void_p),
                ("ngram", C.c_void_p), ("eos", C.c_int), ("row_words", C.c_void_p),
                ("pool_host", C.c_void_p), ("n_pool", C.c_int), ("row_words_out", C.c_void_p)]


class DebugBan:
    """gitmi_debug_ban (include/gitmi_experiment.h) for op_vocab_topm_rules / op_row_topm / op_sample_rows_rules: words uint32
    [n_sets, W] as an int32 device tensor of the same bits (or None), set_of / min_new / ngram int32 device tensors with one entry
    per sentence, eos; row_words int32 [rows, W] (or None: as without it) the rows' own sets of the step, which the kernels then
    read in place of words[set_of] (op_ban_rows computes them).  The hooks check the tables; nothing is checked here.  Keeps the
    tensors alive."""

    def __init__(self, words: Optional[torch.Tensor], n_sets: int, W: int, set_of: Optional[torch.Tensor],
                 min_new: Optional[torch.Tensor], ngram: Optional[torch.Tensor], eos: int,
                 row_words: Optional[torch.Tensor] = None):
        self.tensors = (words, set_of, min_new, ngram, row_words)
        self.struct = _GitmiDebugBan(_ptr(words) or None, int(n_sets), int(W), _ptr(set_of) or None, _ptr(min_new) or None,
                                     _ptr(ngram) or None, int(eos), _ptr(row_words) or None)


def _ban_ref(ban: Optional[DebugBan]):
    return None if ban is None else C.addressof(ban.struct)


def op_ban_rows(ban: DebugBan, pool, ids: torch.Tensor, cur_len: int, beams: int, V: int, out: Optional[torch.Tensor] = None,
                operands: Optional[str] = None) -> torch.Tensor:
    """ban_rows_kernel through its launcher (measurement build; the form of gitmi_debug_row_topm that ban.row_words_out selects,
    include/gitmi_experiment.h): the per-row ban sets of one step under banned token sequences.
    ban: the static sets (words / n_sets / W / set_of); pool: the int32 host pool of banned_sequence_tables for ids.shape[0] /
    beams sentences; ids int32 [rows, ld_ids] device histories of cur_len tokens.  -> row_words int32 [rows, W] (the bits of the
    uint32 words), or `out`."""
    import numpy as np
    lib, fn = _front("gitmi_debug_row_topm", operands=operands)
    pool = np.ascontiguousarray(pool, dtype=np.int32)
    rows = int(ids.shape[0])
    rw = out if out is not None else torch.empty(rows, int(ban.struct.W), device=ids.device, dtype=torch.int32)
    f = {n: getattr(ban.struct, n) for n, _ in _GitmiDebugBan._fields_}
    f.update(row_words=None, pool_host=int(pool.ctypes.data), n_pool=int(pool.size), row_words_out=rw.data_ptr())
    call = _GitmiDebugBan(**f)
    _ck(fn(None, 0, int(V), rows, ids.data_ptr(), int(ids.stride(0)), int(cur_len), None, int(beams), 0, 0.0, 1, None, None, None,
           _stream(), C.addressof(call)), lib)
    return rw


def _logit_rows(logits: torch.Tensor, V: int) -> Tuple[int, int]:
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[1] < V:
        raise ValueError(f"logits must be an fp32 [rows, >= {V}] view with unit column stride")
    return int(logits.shape[0]), int(logits.stride(0))


def row_topm_slots(M: int) -> int:
    return 1 if M <= 1 else 2 if M <= 2 else 4 if M <= 4 else 8 if M <= 8 else 16


def op_row_topm(logits: torch.Tensor, V: int, M: int, ids: Optional[torch.Tensor] = None, cur_len: int = 0,
                plen: Optional[torch.Tensor] = None, beams: int = 1, suppress_kind: int = 0, rep_penalty: float = 0.0,
                out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, operands: Optional[str] = None,
                ban: Optional[DebugBan] = None):
    """row_topm_kernel through its launcher: -> (part_val fp32 [R, slots], part_idx int32 [R, slots], part_lse fp32 [R, 2]),
    slots = row_topm_slots(M).  ids int32 [R, ld_ids] device histories of cur_len tokens (None: no rules), plen int32 [R / beams];
    ban: the rows' decoding constraints."""
    lib, fn = _front("gitmi_debug_row_topm", operands=operands)
    R, ldl = _logit_rows(logits, V)
    slots = row_topm_slots(M)
    dev = logits.device
    pv, pi, pl = out if out is not None else (torch.empty(R, slots, device=dev), torch.empty(R, slots, device=dev, dtype=torch.int32),
                                              torch.empty(R, 2, device=dev))
    _ck(fn(logits.data_ptr(), ldl, int(V), R, _ptr(ids), 0 if ids is None else int(ids.stride(0)), int(cur_len), _ptr(plen), int(beams),
           int(suppress_kind), float(rep_penalty), int(M), pv.data_ptr(), pi.data_ptr(), pl.data_ptr(), _stream(), _ban_ref(ban)), lib)
    return pv, pi, pl


def op_trie_select(logits: torch.Tensor, V: int, ids: torch.Tensor, cur_len: int, plen: torch.Tensor, eos: int,
                   child_off: Optional[torch.Tensor], child_tok: Optional[torch.Tensor], child_node: Optional[torch.Tensor],
                   cursor: torch.Tensor, out: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], n_nodes: Optional[int] = None,
                   operands: Optional[str] = None) -> None:
    """trie_select_kernel through its launcher on a CSR trie of int32 device tensors; cursor int32 [B] is read and updated, out =
    (part_val fp32 [B], part_idx int32 [B], part_lse fp32 [B, 2]) written for the rows at or past their prefix."""
    lib, fn = _front("gitmi_debug_trie_select", operands=operands)
    B, ldl = _logit_rows(logits, V)
    pv, pi, pl = out
    if n_nodes is None:
        n_nodes = int(child_off.numel()) - 1
    _ck(fn(logits.data_ptr(), ldl, int(V), B, ids.data_ptr(), int(ids.stride(0)), int(cur_len), plen.data_ptr(), int(eos),
           _ptr(child_off), _ptr(child_tok), _ptr(child_node), int(n_nodes), cursor.data_ptr(), pv.data_ptr(), pi.data_ptr(),
           pl.data_ptr(), _stream()), lib)


def op_sample_rows_rules(logits: torch.Tensor, V: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, ndraw: int = 2,
                        seed: int = 0, step: int = 1, stride: Optional[int] = None, ids: Optional[torch.Tensor] = None,
                        cur_len: int = 0, rep_penalty: float = 0.0, want_filtered: bool = True,
                        out: Optional[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = None,
                        operands: Optional[str] = None, plen: Optional[torch.Tensor] = None, beams: int = 1,
                        ban: Optional[DebugBan] = None):
    """op_sample_rows with what the engine's sampling step also sets (measurement build): padded logit rows, the repetition
    penalty over ids int32 [R, ld_ids] (cur_len tokens) and lists of `stride` entries; ban: the rows' decoding constraints, with
    plen int32 [R / beams] and beams.
    -> (filtered logits [R, V] or None, tokens int32 [R, stride], log-probs fp32 [R, stride]); out = (log-probs, tokens, filtered)."""
    lib, fn = _front("gitmi_debug_sample_rows", operands=operands)
    R, ldl = _logit_rows(logits, V)
    stride = ndraw if stride is None else int(stride)
    if out is not None:
        lp, tok, filt = out
    else:
        lp = torch.empty(R, max(stride, 1), device=logits.device, dtype=torch.float32)
        tok = torch.empty(R, max(stride, 1), device=logits.device, dtype=torch.int32)
        filt = torch.empty(R, V, device=logits.device, dtype=torch.float32) if want_filtered else None
    _ck(fn(logits.data_ptr(), R, int(V), float(temperature), int(top_k), float(top_p), int(ndraw), int(seed), int(step), lp.data_ptr(),
           tok.data_ptr(), _ptr(filt), ldl, _ptr(ids), 0 if ids is None else int(ids.stride(0)), int(cur_len), float(rep_penalty),
           stride, _stream(), _ptr(plen), int(beams), _ban_ref(ban)), lib)
    return filt, tok, lp


def kv_repack(img_k: torch.Tensor, img_v: torch.Tensor):
    """Head-major 16-bit image K/V [B,H,N,64] -> the decode layouts of kernels_attn_decode.hip (flat [B*H*Npad*64] each, same
    dtype; bf16: libgitmi.so, fp16: libgitmi_f16.so)."""
    lib = _op_library(img_k.dtype, img_v.dtype)
    B, H, N, _ = img_k.shape
    d = H * 64
    rows = torch.zeros(B * N, 3 * d, device=img_k.device, dtype=img_k.dtype)
    rows[:, d:2 * d] = img_k.permute(0, 2, 1, 3).reshape(B * N, d)
    rows[:, 2 * d:] = img_v.permute(0, 2, 1, 3).reshape(B * N, d)
    Np = (N + 31) // 32 * 32
    kf = torch.empty(B * H * Np * 64, device=img_k.device, dtype=img_k.dtype)
    vt = torch.empty(B * H * Np * 64, device=img_k.device, dtype=img_k.dtype)
    _ck(lib.gitmi_op_kv_repack(rows.data_ptr(), kf.data_ptr(), vt.data_ptr(), B, N, H, _stream()), lib)
    return kf, vt


def preprocess_image(rgb_hwc: torch.Tensor, crop: int = 224) -> torch.Tensor:
    """uint8 [H,W,3] device tensor (a decoded RGB image) -> fp32 [3,crop,crop], bit-exact with the reference's
    PIL/torchvision transform (Resize(crop, BICUBIC) -> CenterCrop -> ToTensor -> Normalize)."""
    lib = load_library()
    assert rgb_hwc.is_cuda and rgb_hwc.dtype == torch.uint8 and rgb_hwc.dim() == 3 and rgb_hwc.shape[2] == 3
    rgb_hwc = rgb_hwc.contiguous()
    H, W = int(rgb_hwc.shape[0]), int(rgb_hwc.shape[1])
    nw = crop if W <= H else int(crop * W / H)
    tmp = torch.empty(H * nw * 3, dtype=torch.uint8, device=rgb_hwc.device)
    out = torch.empty(3, crop, crop, dtype=torch.float32, device=rgb_hwc.device)
    _ck(lib.gitmi_preprocess_image(rgb_hwc.data_ptr(), H, W, crop, tmp.data_ptr(), tmp.numel(), out.data_ptr(), _stream()), lib)
    return out


def preprocess_image_to(rgb_hwc: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """uint8 [H,W,3] device tensor -> fp32 [3,out_h,out_w]: Pillow-exact bicubic resize to (out_h, out_w), ToTensor,
    Normalize -- the MinMaxResizeForTest branch of the reference transform (inference.py:113-116)."""
    lib = load_library()
    assert rgb_hwc.is_cuda and rgb_hwc.dtype == torch.uint8 and rgb_hwc.dim() == 3 and rgb_hwc.shape[2] == 3
    rgb_hwc = rgb_hwc.contiguous()
    H, W = int(rgb_hwc.shape[0]), int(rgb_hwc.shape[1])
    tmp = torch.empty(H * out_w * 3, dtype=torch.uint8, device=rgb_hwc.device)
    out = torch.empty(3, out_h, out_w, dtype=torch.float32, device=rgb_hwc.device)
    _ck(lib.gitmi_preprocess_image_to(rgb_hwc.data_ptr(), H, W, int(out_h), int(out_w), tmp.data_ptr(), tmp.numel(),
                                      out.data_ptr(), _stream()), lib)
    return out


def preprocess_batch(staging: torch.Tensor, desc: Sequence[Tuple[int, int, int]], crop: int = 224) -> torch.Tensor:
    """A batch of decoded images in ONE uint8 device buffer -> fp32 [n, 3, crop, crop] (gitmi_preprocess_batch: the reference's
    Resize(BICUBIC) -> CenterCrop -> ToTensor -> Normalize, bit-exact with Pillow, one launch pair per 24 images).
    desc: (byte offset, H, W) of every image in `staging`."""
    lib = load_library()
    assert staging.is_cuda and staging.dtype == torch.uint8 and staging.is_contiguous()
    n = len(desc)
    table = (C.c_int64 * (3 * n))(*[int(v) for d in desc for v in d])
    need = 0
    for _, H, W in desc:
        nw = crop if W <= H else int(crop * W / H)
        if nw != W:
            need += (H * nw * 3 + 63) // 64 * 64
    tmp = torch.empty(max(need, 64), dtype=torch.uint8, device=staging.device)
    out = torch.empty(n, 3, crop, crop, dtype=torch.float32, device=staging.device)
    _ck(lib.gitmi_preprocess_batch(staging.data_ptr(), staging.numel(), table, n, int(crop), tmp.data_ptr(), tmp.numel(),
                                   out.data_ptr(), _stream()), lib)
    return out
