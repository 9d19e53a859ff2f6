"""ctypes binding of libmoonsr_hip.so (include/moonsr.h).  No CPU fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libmoonsr_hip.so")

MSR_OK = 0
MSR_ERR_INVALID = -1
MSR_ERR_DEVICE = -2
MSR_ERR_STATE = -3
MSR_ERR_NOMEM = -4

VARIANT_IDS = {"gaugan": 0, "gaugan_no_kl": 1, "cnn": 2, "pix2pix": 3}
# msr_config.flags: MSR_FLAG_BF16X3 = 1, MSR_FLAG_GB_F16X2 = 2 (opt-in 2-term fp16 products in the gamma|beta convs)
# MSR_FLAG_FP8 = 4: declared non-parity mode (fp8 weights x bf8 activations in the chip-filling convs)
# MSR_FLAG_F16C = 8: fp16 main term + fp8 cross terms in the chip-filling convs (parity-grade, 2 MFMA-equivalents per product)
# MSR_FLAG_F16_MAIN = 16 (with F16C): the cross terms left out of the stream / resident kernels ("f16": declared tolerance)
PRECISION_FLAGS = {"fp32": 0, "bf16x3": 1, "bf16x3_gbf16": 3, "fp8": 5, "f16c": 9, "f16": 25}
# MSR_FLAG_CROSS_FP6 = 32 (with F16C, not F16_MAIN): the format of the cross terms in the stream-kernel consumers, or-ed into
# the precision's flags (Generator(cross=...)); "fp8" is the f16c mode as it always was
CROSS_FLAGS = {"fp8": 0, "fp6": 32}
# MSR_FLAG_FUSED_HEAD = 64 (with F16C alone): the last residual conv emits the head's partial sums (Generator(head=...))
HEAD_FLAGS = {"separate": 0, "fused": 64}


class MsrConfig(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("batch_size", C.c_int32), ("latent_dim", C.c_int32),
                ("variant", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32)]


class MsrKernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("device_ms", C.c_double),
                ("flops", C.c_double), ("bytes", C.c_double)]


class MsrRangeStat(C.Structure):
    """msr_range_stat: one record of the activation-range scan (include/moonsr.h)."""
    _fields_ = [("tensor", C.c_char * 48), ("format", C.c_int32), ("producer", C.c_int32), ("max_abs", C.c_float),
                ("n_total", C.c_int64), ("n_cross_clipped", C.c_int64), ("n_clamped", C.c_int64),
                ("n_nonfinite", C.c_int64)]


RANGE_FORMAT_EMBED = 100    # MSR_RANGE_FORMAT_EMBED: a host-side bound on a conv_gb_resident embedding, not a scanned tensor

# every symbol include/moonsr.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("msr_abi_version", C.c_int, []),
    ("msr_create", C.c_int, [C.POINTER(MsrConfig), C.POINTER(_P)]),
    ("msr_destroy", C.c_int, [_P]),
    ("msr_last_error", C.c_char_p, [_P]),
    ("msr_load_weight", C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int32]),
    ("msr_weight_count", C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    ("msr_weight_name", C.c_char_p, [_P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("msr_forward", C.c_int, [_P, _P, _P, _P, C.c_int32, _P]),
    ("msr_forward_gated", C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P]),
    ("msr_graph_enable", C.c_int, [_P, C.c_int32]),
    ("msr_last_latent", C.c_int, [_P, _P, _P]),
    ("msr_sampler_noise", C.c_int, [_P, C.c_uint64, _P, C.c_uint32, _P, C.c_int32, C.c_int32, _P]),
    ("msr_patch_stats", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, C.c_int32, C.c_float, _P, _P, _P]),
    ("msr_extract_patches", C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P]),
    ("msr_compact_patches", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                      _P, _P, _P, _P]),
    ("msr_compact_patches_carry", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    ("msr_stitch_tile", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P, _P, _P, _P]),
    ("msr_stitch_partial", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    ("msr_stitch_accumulate", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, _P]),
    ("msr_stitch_accumulate_band", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("msr_halo_merge", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_float, _P, _P, _P, _P]),
    ("msr_set_blend_window", C.c_int, [_P, _P, C.c_int32]),
    ("msr_resize_area", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    ("msr_resize_cubic", C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, _P]),
    ("msr_resize_area_rows", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_float, C.c_int32, _P]),
    ("msr_resize_cubic_rows", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_float, C.c_int32, _P]),
    ("msr_crc32c", C.c_uint32, [_P, C.c_uint64, C.c_uint32]),
    ("msr_lzw_decode", C.c_int64, [_P, C.c_int64, _P, C.c_int64]),
    ("msr_lzw_encode", C.c_int64, [_P, C.c_int64, _P, C.c_int64]),
    ("msr_lzw_encode_strips", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("msr_lzw_encode_blocks", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("msr_lzw_encode_block_host", C.c_int64, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64]),
    ("msr_tiff_encode_strips", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P]),
    ("msr_tiff_encode_blocks", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                         _P, _P]),
    ("msr_tiff_encode_block_host", C.c_int64, [_P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                               C.c_int64]),
    ("msr_lzw_decode_strips", C.c_int, [_P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P]),
    ("msr_tiff_blocks_to_f32", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("msr_lzw_decode_strip_host", C.c_int64, [_P, C.c_int64, _P, C.c_int64]),
    ("msr_overview_half", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P, _P]),
    ("msr_overview_half_host", C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P]),
    ("msr_infill_workspace_bytes", C.c_int64, [C.c_int32, C.c_int32]),
    ("msr_infill_small_holes", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _P,
                                         C.c_int64, _P]),
    ("msr_debug_infill_stage", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _P,
                                         C.c_int64, _P, C.c_int32]),
    ("msr_infill_component_host", C.c_int32, [_P, C.c_int32, C.c_int32, C.c_float, _P, _P, C.c_int32, _P]),
    ("msr_profile_enable", C.c_int, [_P, C.c_int32]),
    ("msr_profile_reset", C.c_int, [_P]),
    ("msr_profile_read", C.c_int, [_P, C.POINTER(MsrKernelStat), C.c_int32, C.POINTER(C.c_int32)]),
    ("msr_profile_runs", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, C.c_int32, _P]),
    ("msr_forward_flops", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("msr_op_conv3x3", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    ("msr_op_conv_affine", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_float, C.c_int32, _P]),
    ("msr_op_conv3x3_bf16x3", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("msr_op_conv3x3_f16c", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                      C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    ("msr_op_conv3x3_f16c_head", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P,
                                           C.c_float, _P, _P, _P]),
    ("msr_op_spade_gbr", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    ("msr_op_spade_gbr_f16", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P,
                                       _P]),
    ("msr_op_spade_gbr_f16c6", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, _P,
                                         _P]),
    ("msr_op_conv_smallcin", C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_float, C.c_int32, C.c_int32, _P]),
    ("msr_op_norm_act", C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                  C.c_int32, _P]),
    ("msr_op_dense", C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("msr_op_latent", C.c_int, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P]),
    ("msr_op_head", C.c_int, [_P, _P, _P, C.c_float, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, _P]),
    ("msr_op_moments", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P, _P, _P]),
    ("msr_quantize_e4m3", C.c_int64, [_P, C.c_int64, _P]),
    ("msr_op_conv3x3_fp8", C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                     C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    ("msr_op_split_bf16", C.c_int, [_P, _P, _P, C.c_int64, _P]),
    ("msr_debug_tensor", C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    ("msr_debug_moment_forms", C.c_int, [_P, _P, C.c_int64]),
    ("msr_debug_conv_forms", C.c_int, [_P, _P, C.c_int64]),
    ("msr_debug_f16c_kernel", C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    ("msr_debug_form_table", C.c_int, [C.POINTER(MsrConfig), _P, C.c_int64]),
    ("msr_debug_workspace_list", C.c_int, [_P, _P, C.c_int64]),
    ("msr_debug_fill_workspace", C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("msr_device_bytes", C.c_int, [_P, C.POINTER(C.c_int64)]),
    ("msr_range_scan", C.c_int, [_P, _P]),
    ("msr_range_read", C.c_int, [_P, C.POINTER(MsrRangeStat), C.c_int32, C.POINTER(C.c_int32)]),
    ("msr_range_embed_bounds", C.c_int, [_P, C.POINTER(MsrRangeStat), C.c_int32, C.POINTER(C.c_int32)]),
    ("msr_op_range_scan", C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(MsrRangeStat), _P]),
]

_lib: Optional[C.CDLL] = None


STAMP_PATH = os.path.join(CSRC, ".build_stamp")


def sources_hash() -> str:
    """SHA-256 over the library's sources (csrc/*.hip, *.cpp, *.h, Makefile and include/moonsr.h)."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h")) or f == "Makefile")
    for f in [os.path.join(CSRC, f) for f in files] + [os.path.join(_HERE, "..", "include", "moonsr.h")]:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def is_stale() -> bool:
    """True if the .so is missing or was built from other sources than the ones in the tree (the .so is git-ignored,
    and file times do not survive a snapshot, so the check is by content: csrc/.build_stamp holds the hash)."""
    if not os.path.exists(LIB_PATH) or not os.path.exists(STAMP_PATH):
        return True
    with open(STAMP_PATH) as fh:
        return fh.read().strip() != sources_hash()


def build(verbose: bool = False, force: bool = False) -> str:
    """Compile libmoonsr_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if not (force or is_stale()):
        return LIB_PATH                     # the stamp says the .so was built from exactly these sources
    # Stale (or forced): file times do not survive a snapshot, so `make` alone could decide that objects of an OLDER
    # source state are up to date and the stamp below would then bless them.  Rebuild every object unconditionally.
    for f in os.listdir(CSRC):
        if f.endswith(".o") or f == os.path.basename(LIB_PATH):
            os.remove(os.path.join(CSRC, f))
    if os.path.exists(STAMP_PATH):
        os.remove(STAMP_PATH)
    want = sources_hash()
    res = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose or res.returncode:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode or not os.path.exists(LIB_PATH):
        raise RuntimeError("building libmoonsr_hip.so failed (see output above)")
    if sources_hash() == want:              # sources edited during the build: leave the tree marked stale
        with open(STAMP_PATH, "w") as fh:
            fh.write(want + "\n")
    return LIB_PATH


def load() -> C.CDLL:
    """Load the HIP library; raise (never fall back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MSR_LIB", LIB_PATH)   # another build of the same ABI (A/B kernel comparisons)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C moonsuperresolution_amd/csrc`).  moonsuperresolution_amd has no CPU fallback.")
    # torch first: its wheel bundles a HIP runtime, and whichever libamdhip64 is loaded first serves the whole process.  With
    # this library (and so the system runtime) loaded before torch, msr_create found no device on the GPU pool's boxes
    # (`python __graft_entry__.py smoke`, round 3) while torch in a fresh process saw it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = bind(C.CDLL(path), path)
    if lib.msr_abi_version() != 1:
        raise RuntimeError("libmoonsr_hip.so ABI version mismatch")
    _lib = lib
    return lib


def bind(lib, path: str):
    """Set the prototypes of every symbol of SYMBOLS on ``lib``.  A library that lacks one (an older build of the same ABI
    version: entries are only ever added) is an error that names the symbols, never a partial binding."""
    missing = [name for name, _, _ in SYMBOLS if not hasattr(lib, name)]
    if missing:
        raise RuntimeError(f"{path} lacks {', '.join(missing)}: it was built from older sources than this package; rebuild "
                           "it with `python -c 'import __graft_entry__ as g; g.build()'`")
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


def raise_for(lib: C.CDLL, handle, rc: int, what: str) -> None:
    """Map msr_status to the reference's exception style (ValueError / RuntimeError)."""
    if rc == MSR_OK:
        return
    msg = lib.msr_last_error(handle)
    text = f"{what}: {msg.decode() if msg else 'error'} (msr_status {rc})"
    if rc == MSR_ERR_INVALID:
        raise ValueError(text)
    if rc == MSR_ERR_NOMEM:
        raise MemoryError(text)
    raise RuntimeError(text)
