"""ctypes binding of libvfml_hip.so (include/vfml.h).

PyTorch is used for device memory and streams only: every call takes raw device pointers
(`tensor.data_ptr()`) and launches on torch's current HIP stream.  There is NO CPU fallback:
if the library is missing or a kernel rejects its arguments this raises.
"""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VFML_LIB") or os.path.join(_HERE, "libvfml_hip.so")   # VFML_LIB: experiment builds
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ["api.hip", "conv_gemm.hip", "conv_gemm_split.hip", "corr_ensure.hip", "conv_gemm_tapx.hip", "conv_split_plan.hip", "stem.hip", "flow_half.hip", "enc_conv.hip", "norm_pool.hip", "flow_ops.hip", "effects.hip", "correct.hip", "render.hip", "text.hip", "turbulence.hip", "resize.hip", "jpeg.hip", "jpeg_decode.hip", "jpeg_decode_sync.hip", "deflate.hip", "attention.hip", "dwconv.hip", "twins.hip", "warm_start.hip", "scene.hip"]

STATS_ROWS_F32, STATS_ROWS_S16 = 128, 32    # pixels per stats_part block (include/vfml.h VFML_STATS_ROWS_*)
EPI_NONE, EPI_RELU, EPI_TANH, EPI_SIGMOID, EPI_TANH_RELU, EPI_GRU_ZR, EPI_GRU_Q, EPI_ADD_AUX = range(8)
FMT_F32, FMT_S16, FMT_F16 = 0, 1, 2     # storage formats (include/vfml.h; FMT_F16: correlation volumes only)


def vol_f16_levels(mask):
    """vol_fmt of a lookup over pyramids whose levels in `mask` (bit l = level l) hold f16 texels (VFML_VOL_F16_LEVELS)."""
    return 0x100 | mask


def _vol_mask(vol_fmt, levels):
    return (15 if vol_fmt == FMT_F16 else (vol_fmt & 15 if vol_fmt & 0x100 else 0)) & ((1 << levels) - 1)

KORDER_TAP, KORDER_CBLOCK, KORDER_CBLOCK64 = 0, 1, 2   # K-axis order of split weight planes (include/vfml.h)
CONV_SWAP_CROSS, CONV_MFMA2, CONV_MFMA1, CONV_MFMA2A, CONV_PER_TAP = 1, 2, 4, 8, 16   # vfml_conv_desc.flags


class ConvDesc(ctypes.Structure):
    """Mirror of `vfml_conv_desc` (include/vfml.h)."""
    _fields_ = [
        ("in0", c_void_p), ("c0", c_int32), ("ld0", c_int32),
        ("in1", c_void_p), ("c1", c_int32), ("ld1", c_int32),
        ("n", c_int32), ("h", c_int32), ("w", c_int32),
        ("weight", c_void_p), ("bias", c_void_p),
        ("cout", c_int32), ("kh", c_int32), ("kw", c_int32), ("stride", c_int32),
        ("pad_h", c_int32), ("pad_w", c_int32),
        ("out", c_void_p), ("ldo", c_int32),
        ("epilogue", c_int32), ("split", c_int32), ("out_scale", c_float),
        ("aux0", c_void_p), ("ld_aux0", c_int32),
        ("aux1", c_void_p), ("ld_aux1", c_int32),
        ("addend", c_void_p), ("ld_addend", c_int32),
        ("out_t", c_void_p), ("ld_out_t", c_int32),
        ("flags", c_int32),
        ("stats_part", c_void_p),
        ("ksplit_ws", c_void_p),
        ("proj_hi", c_void_p), ("proj_lo", c_void_p), ("proj_n", c_int32), ("proj_kp", c_int32), ("proj_scale", c_float),
        ("proj_out", c_void_p), ("ld_proj", c_int32),
        ("addend_ind", c_void_p),
    ]


class CorrLevelDesc(ctypes.Structure):
    """Mirror of `vfml_corr_level_desc` (include/vfml.h): one level of vfml_corr_levels_ensure."""
    _fields_ = [("d", POINTER(ConvDesc)), ("w_hi", c_void_p), ("w_lo", c_void_p), ("kp", c_int32), ("w_scale", c_float),
                ("out_fmt", c_int32), ("level", c_int32), ("h", c_int32), ("w", c_int32)]


# Every source is built without the SLP vectoriser.  Left on, it pairs adjacent scalar f32 multiplies / adds into
# v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32; where such a packed op was the FIRST reader of a ds_read result, straight behind
# the s_waitcnt that covers it, the correlation lookup read a stale register in lanes 48-63 whenever one of this library's
# MFMA kernels ran on another stream (profiles/r02_kernel_anatomy.md section 7) - and the engine runs two streams by default
# (the encoder prefetch).  Round 2 closed the one observed instance; round 3 closes the class: no packed-f32 first reader of
# an LDS result anywhere in the shipped code object (tests/test_abi.py::test_no_packed_f32_first_reader_of_lds_results).
# Packed f32 ops beside MFMAs are an anti-lever anyway (MI355X_MICROARCH.md, cycle constants: 2 v_pk_add_f32 per MFMA gap
# cost +26 cycles against 2 v_fma_f32).
COMMON_FLAGS = ["-fno-slp-vectorize"]
EXTRA_FLAGS = {}


def build(force=False, verbose=False):
    """Compile the HIP sources for gfx950 into libvfml_hip.so (in-tree). Cross-compiles without a GPU."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    hdrs = [os.path.join(CSRC, "vfml_common.h"), os.path.join(CSRC, "conv_split_common.h"),
            os.path.join(CSRC, "gemm_resident_walk.h"), os.path.join(CSRC, "corr_window.h"),
            os.path.join(CSRC, "jet_table.inc"), os.path.join(CSRC, "jpeg_tables.inc"), os.path.join(CSRC, "jpeg_decode_common.h"),
            os.path.join(CSRC, "jpeg_sync_steps.h"), os.path.join(CSRC, "deflate_code.h"), os.path.join(_HERE, "..", "..", "include", "vfml.h")]
    deps = srcs + hdrs
    if not force and os.path.exists(LIB_PATH) and all(
            os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return LIB_PATH
    # one object per source, compiled side by side (objects kept under csrc/_obj: a changed source recompiles alone)
    objdir = os.path.join(CSRC, "_obj")
    os.makedirs(objdir, exist_ok=True)
    newest_hdr = max(os.path.getmtime(h) for h in hdrs)
    jobs = []
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), newest_hdr):
            cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + COMMON_FLAGS + EXTRA_FLAGS.get(os.path.basename(src), []) + [
                "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in jobs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = ["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB_PATH] + [
        os.path.join(objdir, os.path.basename(src) + ".o") for src in srcs]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


_lib = None


def lib():
    """Load the library (after torch, so that its libamdhip64.so.7 is the one HIP runtime in the process)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"vfml HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (needs hipcc). There is no CPU fallback for the flow engine.")
    L = ctypes.CDLL(LIB_PATH)
    L.vfml_last_error.restype = c_char_p
    L.vfml_abi_version.restype = c_int
    L.vfml_conv2d.argtypes = [POINTER(ConvDesc), c_void_p]
    L.vfml_conv2d_split.argtypes = [POINTER(ConvDesc), c_void_p, c_void_p, c_int, c_float, c_int, c_int, c_int, c_int,
                                    c_void_p]
    L.vfml_conv2d_variant.argtypes = [POINTER(ConvDesc), c_char_p, c_int]
    L.vfml_conv2d_split_variant.argtypes = L.vfml_conv2d_split.argtypes[:-1] + [c_char_p, c_int]
    L.vfml_conv2d_split_variant_at.argtypes = [c_int, c_char_p, c_int]
    L.vfml_to_s16.argtypes = [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_float, c_void_p]
    L.vfml_softmax_rows_s16.argtypes = [c_void_p, c_int64, c_int, c_int64, c_void_p, c_int64, c_float, c_void_p]
    L.vfml_transpose_split_f16.argtypes = [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p]
    L.vfml_split_f16.argtypes = [c_void_p, c_int64, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_void_p]
    L.vfml_frames_to_nhwc4.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p, c_void_p]
    L.vfml_instnorm_workspace_bytes.restype = c_int64
    L.vfml_instnorm_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.vfml_instnorm_stats.argtypes = [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]
    L.vfml_softmax_rows_f16.argtypes = [c_void_p, c_int64, c_int, c_int64, c_void_p, c_int64, c_float, c_void_p]
    L.vfml_attention_plane_workspace_bytes.restype = c_int64
    L.vfml_attention_plane_workspace_bytes.argtypes = [c_int]
    L.vfml_attention_plane_f16.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_float, c_float, c_void_p, c_int64,
                                           c_void_p, c_void_p]
    L.vfml_attention_bank_planes_f16.argtypes = [c_void_p, c_int64, POINTER(c_void_p), c_int64, c_int, c_int, c_int, c_float, c_float,
                                                 POINTER(c_void_p), c_int64, c_void_p, c_void_p]
    L.vfml_axpy_f32.argtypes = [c_void_p, c_void_p, c_int64, c_float, c_void_p]
    L.vfml_dwconv2d.argtypes = [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                                c_int, c_void_p]
    L.vfml_gelu_rows.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p]
    L.vfml_layernorm_rows.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_float, c_int, c_int,
                                      c_void_p]
    L.vfml_window_attention.argtypes = [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64,
                                        c_int, c_int, c_void_p]
    L.vfml_attention_shared_keys.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                             c_int64, c_int, c_int, c_int, c_void_p]
    L.vfml_transpose_to_s16.argtypes = [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_int64, c_void_p]
    L.vfml_add_to_s16.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_float, c_void_p]
    L.vfml_instnorm_finalize.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int64, c_void_p]
    L.vfml_instnorm_finalize_workspace_bytes.restype = c_int64
    L.vfml_instnorm_finalize_workspace_bytes.argtypes = [c_int, c_int]
    L.vfml_stem7x7s2_chunks.argtypes = [c_int, c_int]
    L.vfml_stem7x7s2.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]
    L.vfml_instnorm_apply.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]
    L.vfml_avgpool2x2.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    L.vfml_corr_lookup.argtypes = [POINTER(c_void_p), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                   c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]
    L.vfml_corr_lookup_indirect.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                            c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                            c_void_p]
    L.vfml_corr_lookup_indirect_bidir.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                                  c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int,
                                                  c_int, c_int, c_int, c_int, c_void_p]
    L.vfml_corr_lookup_indirect_bidir_cached.argtypes = L.vfml_corr_lookup_indirect_bidir.argtypes[:-1] + [
        c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    L.vfml_ptr_table_set.argtypes = [c_void_p, POINTER(c_void_p), c_int, c_void_p]
    L.vfml_corr_level0_ensure.argtypes = L.vfml_conv2d_split.argtypes[:5] + [c_int, c_int, c_int] + [
        c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    L.vfml_corr_levels_ensure.argtypes = [POINTER(CorrLevelDesc), c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p,
                                          c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    L.vfml_window_seed.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]
    L.vfml_tapsum3x3_update.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_int64, c_void_p, c_void_p,
                                        c_int, c_void_p, c_int, c_int, c_void_p]
    L.vfml_conv3x3_c64.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p,
                                   c_int, c_void_p, c_void_p]
    L.vfml_flow_half.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p, c_int, c_float,
                                 c_void_p, c_void_p, c_int, c_void_p]
    L.vfml_coords_init.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p]
    L.vfml_flow_rows7.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    L.vfml_tapsum3x3.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, ctypes.c_int64, c_void_p]
    L.vfml_coords_update.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                     c_int, c_void_p]
    L.vfml_flow_forward_interpolate_workspace_bytes.restype = c_int64
    L.vfml_flow_forward_interpolate_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.vfml_flow_forward_interpolate.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                                c_void_p]
    L.vfml_flow_lod.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p]
    L.vfml_flow_encode.argtypes = [c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_void_p,
                                   c_void_p]
    L.vfml_taa_blend.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_double,
                                 c_double, c_void_p]
    L.vfml_flow_quality_map.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]
    L.vfml_flow_correct_workspace_bytes.argtypes = [c_int, c_int]
    L.vfml_flow_correct_workspace_bytes.restype = ctypes.c_size_t
    L.vfml_flow_correct.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                    c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p, c_void_p,
                                    ctypes.c_int64, c_void_p, ctypes.c_size_t, c_void_p]
    L.vfml_flow_colorize.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    L.vfml_flow_decode.argtypes = [c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]
    L.vfml_flow_diff_overlay.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
    L.vfml_compose_frame.argtypes = [POINTER(c_void_p), POINTER(c_int32), c_int, c_int, c_int, c_int, c_int64, c_void_p,
                                     c_void_p]
    L.vfml_text_draw.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int64, c_int, c_void_p]
    L.vfml_flow_turbulence_workspace_bytes.argtypes = [c_int, c_int]
    L.vfml_flow_turbulence_workspace_bytes.restype = ctypes.c_size_t
    L.vfml_flow_turbulence_map.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p]
    L.vfml_resize_u8.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p,
                                 c_void_p]
    L.vfml_jpeg_workspace_bytes.restype = c_int64
    L.vfml_jpeg_workspace_bytes.argtypes = [c_int, c_int]
    L.vfml_jpeg_scan_capacity.restype = c_int64
    L.vfml_jpeg_scan_capacity.argtypes = [c_int, c_int]
    L.vfml_jpeg_encode_rgb.argtypes = [c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                       c_void_p]
    L.vfml_jpeg_sampled_workspace_bytes.restype = c_int64
    L.vfml_jpeg_sampled_workspace_bytes.argtypes = [c_int, c_int, c_int]
    L.vfml_jpeg_sampled_scan_capacity.restype = c_int64
    L.vfml_jpeg_sampled_scan_capacity.argtypes = [c_int, c_int, c_int]
    L.vfml_jpeg_encode_rgb_sampled.argtypes = [c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                                               c_void_p, c_void_p]
    L.vfml_jpeg_decode_workspace_bytes.restype = c_int64
    L.vfml_jpeg_decode_workspace_bytes.argtypes = [c_int, c_int, c_int64]
    L.vfml_jpeg_decode_rgb.argtypes = [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                       c_void_p, c_int64, c_void_p, c_void_p]
    L.vfml_jpeg_decode_sync_workspace_bytes.restype = c_int64
    L.vfml_jpeg_decode_sync_workspace_bytes.argtypes = [c_int, c_int, c_int64, c_int]
    L.vfml_jpeg_decode_rgb_sync.argtypes = [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                            c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
    L.vfml_jpeg_decode_sampled_workspace_bytes.restype = c_int64
    L.vfml_jpeg_decode_sampled_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int64]
    L.vfml_jpeg_decode_rgb_sampled.argtypes = [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                               c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
    L.vfml_jpeg_decode_sync_sampled_workspace_bytes.restype = c_int64
    L.vfml_jpeg_decode_sync_sampled_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int64, c_int]
    L.vfml_jpeg_decode_rgb_sync_sampled.argtypes = [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                                                    c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
    for fn in (L.vfml_deflate_capacity, L.vfml_deflate_workspace_bytes, L.vfml_inflate_workspace_bytes):
        fn.restype = c_int64
        fn.argtypes = [c_int64, c_int]
    L.vfml_deflate_huffman.argtypes = [c_void_p, c_int64, c_int, ctypes.c_uint32, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p]
    L.vfml_inflate_chunks.argtypes = [c_void_p, c_int64, c_void_p, c_int, c_int, c_int64, ctypes.c_uint32, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]
    L.vfml_convex_upsample.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    L.vfml_scene_distances.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    for name in EXPORTS:
        getattr(L, name)  # AttributeError here = header/library drift
    if L.vfml_abi_version() != 27:
        raise RuntimeError("libvfml_hip.so ABI version mismatch")
    _lib = L
    return L


EXPORTS = [
    "vfml_conv2d", "vfml_conv2d_split", "vfml_conv2d_variant", "vfml_conv2d_split_variant", "vfml_conv2d_split_variant_at", "vfml_split_f16", "vfml_to_s16", "vfml_softmax_rows_s16", "vfml_softmax_rows_f16", "vfml_attention_plane_workspace_bytes", "vfml_attention_plane_f16", "vfml_attention_bank_planes_f16", "vfml_axpy_f32", "vfml_dwconv2d", "vfml_gelu_rows", "vfml_layernorm_rows", "vfml_window_attention", "vfml_attention_shared_keys", "vfml_transpose_to_s16", "vfml_add_to_s16",
    "vfml_transpose_split_f16", "vfml_frames_to_nhwc4", "vfml_instnorm_workspace_bytes", "vfml_instnorm_stats",
    "vfml_instnorm_apply", "vfml_instnorm_finalize", "vfml_instnorm_finalize_workspace_bytes", "vfml_avgpool2x2", "vfml_corr_lookup", "vfml_corr_lookup_indirect", "vfml_corr_lookup_indirect_bidir",
    "vfml_corr_lookup_indirect_bidir_cached",
    "vfml_ptr_table_set", "vfml_corr_level0_ensure", "vfml_corr_levels_ensure", "vfml_window_seed", "vfml_coords_update", "vfml_coords_init", "vfml_tapsum3x3", "vfml_tapsum3x3_update", "vfml_flow_rows7", "vfml_flow_half", "vfml_conv3x3_c64",
    "vfml_flow_forward_interpolate_workspace_bytes", "vfml_flow_forward_interpolate",
    "vfml_convex_upsample", "vfml_stem7x7s2", "vfml_stem7x7s2_chunks", "vfml_flow_lod", "vfml_flow_encode", "vfml_taa_blend", "vfml_flow_quality_map", "vfml_flow_correct_workspace_bytes", "vfml_flow_correct",
    "vfml_flow_colorize", "vfml_compose_frame", "vfml_flow_decode", "vfml_flow_diff_overlay", "vfml_text_draw",
    "vfml_flow_turbulence_workspace_bytes", "vfml_flow_turbulence_map", "vfml_resize_u8",
    "vfml_jpeg_workspace_bytes", "vfml_jpeg_scan_capacity", "vfml_jpeg_encode_rgb",
    "vfml_jpeg_sampled_workspace_bytes", "vfml_jpeg_sampled_scan_capacity", "vfml_jpeg_encode_rgb_sampled",
    "vfml_jpeg_decode_workspace_bytes", "vfml_jpeg_decode_rgb",
    "vfml_jpeg_decode_sync_workspace_bytes", "vfml_jpeg_decode_rgb_sync",
    "vfml_jpeg_decode_sampled_workspace_bytes", "vfml_jpeg_decode_rgb_sampled",
    "vfml_jpeg_decode_sync_sampled_workspace_bytes", "vfml_jpeg_decode_rgb_sync_sampled",
    "vfml_deflate_capacity", "vfml_deflate_workspace_bytes", "vfml_deflate_huffman",
    "vfml_inflate_workspace_bytes", "vfml_inflate_chunks", "vfml_scene_distances",
    "vfml_last_error", "vfml_abi_version",
]


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {lib().vfml_last_error().decode()}")


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, offset=0):
    """Device pointer of a float32 tensor's storage start + `offset` floats (0/None-safe)."""
    if t is None:
        return None
    return c_void_p(t.data_ptr() + 4 * offset)


def _dev(t, dtype=torch.float32):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"expected a contiguous {dtype} device tensor, got {t.dtype} {t.device} "
                         f"contiguous={t.is_contiguous()}")
    return t


# -- optional per-launch timing of vfml_conv2d (bench.py's roofline leg) ---------------------------
_PROFILE = None


_PROFILE_HBM = None


def profile_begin():
    """Start recording (kernel variant, algorithmic FLOPs, start/end HIP events) per vfml_conv2d launch, and
    (kernel, algorithmic bytes, events) per correlation lookup.
    Events are recorded on the stream the kernels are launched on (torch's current stream)."""
    global _PROFILE, _PROFILE_HBM
    _PROFILE = []
    _PROFILE_HBM = []


def profile_end_hbm():
    """{kernel: {"launches", "bytes", "ms"}} of the HBM-bound launches recorded since profile_begin()
    (call before profile_end(), which stops the recording)."""
    rec = _PROFILE_HBM or []
    torch.cuda.synchronize()
    out = {}
    for name, nbytes, e0, e1 in rec:
        d = out.setdefault(name, {"launches": 0, "bytes": 0.0, "ms": 0.0})
        d["launches"] += 1
        d["bytes"] += nbytes
        d["ms"] += e0.elapsed_time(e1)
    return out


def profile_end():
    """Stop recording; returns {variant: {"launches", "flops", "bytes", "ms", "shapes"}} (synchronises); bytes = every operand
    read once and the result written once (the algorithmic HBM traffic of the launch); shapes = the same sums per layer
    shape "khxkw cin->cout" (one kernel variant serves several layers: bench.py's roofline.by_shape)."""
    global _PROFILE, _PROFILE_HBM
    rec, _PROFILE = _PROFILE or [], None
    _PROFILE_HBM = None
    torch.cuda.synchronize()
    out = {}
    for variant, flops, nbytes, e0, e1, shape in rec:
        d = out.setdefault(variant, {"launches": 0, "flops": 0.0, "bytes": 0.0, "ms": 0.0, "shapes": {}})
        ms = e0.elapsed_time(e1)
        for t in (d, d["shapes"].setdefault(shape, {"launches": 0, "flops": 0.0, "bytes": 0.0, "ms": 0.0})):
            t["launches"] += 1
            t["flops"] += flops
            t["bytes"] += nbytes
            t["ms"] += ms
    return out


class SplitWeight:
    """[rows][k] f32 matrix (times a power-of-two `scale`) as two f16 planes [rows][kp] (hi, lo) for
    vfml_conv2d_split."""

    def __init__(self, rows, k, device):
        self.rows, self.k, self.kp = rows, k, (k + 31) // 32 * 32
        self.scale = 1.0
        self.order = KORDER_TAP     # set to KORDER_CBLOCK by whoever fills it with pack_conv_weight(cblock=True)
        # one allocation: the LDS-DMA conv kernel reaches both planes through one buffer descriptor
        self.planes = torch.empty(2 * rows * self.kp, dtype=torch.float16, device=device)
        self.hi, self.lo = self.planes[:rows * self.kp], self.planes[rows * self.kp:]

    @staticmethod
    def auto_scale(absmax):
        """Largest power of two that keeps scale * absmax below 2^14 (f16 max is 65504)."""
        import math
        if not (absmax > 0.0) or not math.isfinite(absmax):
            return 1.0
        return 2.0 ** math.floor(math.log2(16384.0 / absmax))

    def fill_transposed(self, src, rows_src, ld=None, scale=1.0, src_off=0):
        """src: flat f32 [rows_src][self.rows] (row stride ld): planes of its transpose, k = source row."""
        self.scale = float(scale)
        _check(lib().vfml_transpose_split_f16(_ptr(_dev(src), src_off), rows_src, self.rows, ld or self.rows,
                                              self.scale, c_void_p(self.hi.data_ptr()), c_void_p(self.lo.data_ptr()),
                                              self.kp, _stream()), "vfml_transpose_split_f16")
        return self

    def fill(self, src, src_off=0, ld=None, scale=1.0):
        """src: flat f32 device tensor holding [rows][k] at float offset src_off with row stride ld."""
        self.scale = float(scale)
        _check(lib().vfml_split_f16(_ptr(_dev(src), src_off), self.rows, self.k, ld or self.k, self.scale,
                                    c_void_p(self.hi.data_ptr()), c_void_p(self.lo.data_ptr()), self.kp, _stream()),
               "vfml_split_f16")
        return self


def conv2d(in0, c0, ld0, n, h, w, weight, bias, cout, kh, kw, out, ldo, *, stride=1, pad_h=0, pad_w=0,
           in0_off=0, weight_off=0, in1=None, c1=0, ld1=0, in1_off=0, out_off=0, epilogue=EPI_NONE, split=0, out_scale=1.0,
           aux0=None, ld_aux0=0, aux0_off=0, aux1=None, ld_aux1=0, aux1_off=0,
           in_fmt=FMT_F32, out_fmt=FMT_F32, aux_fmt=FMT_F32, addend=None, ld_addend=0, addend_off=0,
           out_t=None, ld_out_t=0, out_t_off=0, swap_cross=False, stats_part=None, mfma=3, per_tap=False, ksplit_ws=None,
           proj=None, proj_out=None, ld_proj=0, addend_ind=None, variant_only=False):
    """Launch vfml_conv2d. Tensors are flat float32 device buffers; *_off are float offsets into them
    (channel slices of wider NHWC buffers).  mfma: terms of the split-f16 product (3; 2 or "2w" = weights as plain
    f16; "2a" = activations as plain f16; 1 = both operands plain f16 - VFML_CONV_MFMA2 / _MFMA2A / _MFMA1).  per_tap:
    VFML_CONV_PER_TAP (the per-tap staging kernel where the shared-stage one would run; same bits).
    proj (a SplitWeight [proj_n <= 48][cout]) with proj_out / ld_proj: the projection epilogue (vfml_conv_desc.proj_out) -
    relu(out) is not stored, proj_out receives cout / 128 partial maps [n*ho*wo][ld_proj] of relu(out) x proj^T.
    variant_only: launch nothing and return the name of the kernel the library would launch for this call, as
    rocprofv3 prints it (vfml_conv2d_variant / vfml_conv2d_split_variant: the library's own plan, csrc/conv_split_plan.hip)."""
    d = ConvDesc()
    d.in0, d.c0, d.ld0 = _ptr(_dev(in0), in0_off), c0, ld0
    d.in1, d.c1, d.ld1 = (_ptr(_dev(in1), in1_off) if in1 is not None else None), c1, ld1
    d.n, d.h, d.w = n, h, w
    is_split = isinstance(weight, (SplitWeight, PlainWeight))
    d.weight = None if is_split else _ptr(_dev(weight), weight_off)
    d.bias = _ptr(_dev(bias)) if bias is not None else None
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w = cout, kh, kw, stride, pad_h, pad_w
    d.out, d.ldo = _ptr(_dev(out), out_off), ldo
    d.epilogue, d.split, d.out_scale = epilogue, split, out_scale
    d.aux0, d.ld_aux0 = (_ptr(_dev(aux0), aux0_off) if aux0 is not None else None), ld_aux0
    d.aux1, d.ld_aux1 = (_ptr(_dev(aux1), aux1_off) if aux1 is not None else None), ld_aux1
    d.addend, d.ld_addend = (_ptr(_dev(addend), addend_off) if addend is not None else None), ld_addend
    d.out_t, d.ld_out_t = (_ptr(_dev(out_t), out_t_off) if out_t is not None else None), ld_out_t
    if mfma == "2w":
        mfma = 2
    if mfma not in (1, 2, 3, "2a") or (swap_cross and mfma != 3):
        raise ValueError(f"mfma={mfma!r}: 1, 2 ('2w'), '2a' or 3 (3 with swap_cross)")
    d.flags = (CONV_SWAP_CROSS if swap_cross else 0) | {3: 0, 2: CONV_MFMA2, "2a": CONV_MFMA2A, 1: CONV_MFMA1}[mfma] | (CONV_PER_TAP if per_tap else 0)
    d.stats_part = c_void_p(stats_part.data_ptr()) if stats_part is not None else None   # float64 workspace
    d.ksplit_ws = _ptr(_dev(ksplit_ws)) if ksplit_ws is not None else None      # GEMM form: second half of K (vfml.h)
    if addend_ind is not None:       # (table tensor, entry): the device cell that holds the addend pointer (vfml.h)
        tab, ent = addend_ind
        d.addend_ind = c_void_p(tab.data_ptr() + 8 * ent)
    if proj is not None:
        if not isinstance(proj, SplitWeight) or proj.lo is None or proj_out is None:
            raise ValueError("proj: a SplitWeight with both planes, and proj_out")
        d.proj_hi, d.proj_lo = c_void_p(proj.hi.data_ptr()), c_void_p(proj.lo.data_ptr())
        d.proj_n, d.proj_kp, d.proj_scale = proj.rows, proj.kp, proj.scale
        d.proj_out, d.ld_proj = _ptr(_dev(proj_out)), ld_proj
    if is_split:
        # weight_off counts rows of the split planes (each row kp halves)
        wargs = (c_void_p(weight.hi.data_ptr() + 2 * weight_off * weight.kp),
                 c_void_p(weight.lo.data_ptr() + 2 * weight_off * weight.kp) if weight.lo is not None else None, weight.kp,
                 weight.scale, in_fmt, out_fmt, aux_fmt, weight.order)

        def launch():
            _check(lib().vfml_conv2d_split(ctypes.byref(d), *wargs, _stream()), "vfml_conv2d_split")

        def variant():
            buf = ctypes.create_string_buffer(160)
            _check(lib().vfml_conv2d_split_variant(ctypes.byref(d), *wargs, buf, len(buf)), "vfml_conv2d_split_variant")
            return buf.value.decode()
    else:
        if in_fmt != FMT_F32 or out_fmt != FMT_F32 or aux_fmt != FMT_F32:
            raise ValueError("the exact-f32 kernel (vfml_conv2d) takes and writes plain f32 activations only")

        def launch():
            _check(lib().vfml_conv2d(ctypes.byref(d), _stream()), "vfml_conv2d")

        def variant():
            buf = ctypes.create_string_buffer(160)
            _check(lib().vfml_conv2d_variant(ctypes.byref(d), buf, len(buf)), "vfml_conv2d_variant")
            return buf.value.decode()
    if variant_only:
        return variant()
    if _PROFILE is None:
        launch()
        return
    ho = (h + 2 * pad_h - kh) // stride + 1
    wo = (w + 2 * pad_w - kw) // stride + 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    _PROFILE.append((variant(),       # the kernel the library chose
                     2.0 * n * ho * wo * (kh * kw * (c0 + c1) * cout + (cout * proj.rows if proj is not None else 0)),
                     # operands read once + result written once, 4 bytes per element in either activation format
                     4.0 * (n * h * w * (c0 + c1) + n * ho * wo * cout * (2 if out_t is not None else 1)
                            + cout * kh * kw * (c0 + c1) * (0.5 if is_split and weight.lo is None else 1.0)), e0, e1,
                     f"{kh}x{kw} {c0 + c1}->{cout}" + (f"->{proj.rows}" if proj is not None else "")))


def frames_to_nhwc4(src, n, H, W, scale, shift, dst):
    """src: uint8 [n,H,W,3] or float32 [n,3,H,W] device tensor -> dst float32 [n,H,W,4]."""
    if src.dtype == torch.uint8:
        kind = 0
    elif src.dtype == torch.float32:
        kind = 1
    else:
        raise ValueError(f"frames must be uint8 HWC or float32 CHW, got {src.dtype}")
    if not (src.is_cuda and src.is_contiguous()):
        raise ValueError("frames must be a contiguous device tensor")
    _check(lib().vfml_frames_to_nhwc4(c_void_p(src.data_ptr()), kind, n, H, W, scale, shift, _ptr(_dev(dst)),
                                      _stream()), "vfml_frames_to_nhwc4")


def instnorm_workspace_bytes(n, hw, c):
    return int(lib().vfml_instnorm_workspace_bytes(n, hw, c))


def instnorm_stats(x, n, hw, c, stats, workspace, eps=1e-5):
    _check(lib().vfml_instnorm_stats(_ptr(_dev(x)), n, hw, c, eps, _ptr(_dev(stats)),
                                     c_void_p(workspace.data_ptr()), _stream()), "vfml_instnorm_stats")


def instnorm_finalize_workspace_bytes(chunks, c):
    return int(lib().vfml_instnorm_finalize_workspace_bytes(chunks, c))


def instnorm_finalize(part, n, chunks, c, hw, stats, eps=1e-5, workspace=None):
    """Fold the partial sums a convolution left in `part` (conv2d(..., stats_part=part)) into {mean, rstd}.
    workspace: a float64 device tensor for the slice-wise first pass over many partials (instnorm_finalize_workspace_bytes;
    None: one is taken from torch's allocator for this call - stream-ordered, so concurrent streams never share it)."""
    need = instnorm_finalize_workspace_bytes(chunks, c)
    if need and (workspace is None or workspace.numel() * 8 < need):
        workspace = torch.empty(min(n, 8) * need // 8, dtype=torch.float64, device=stats.device)
    _check(lib().vfml_instnorm_finalize(c_void_p(part.data_ptr()), n, chunks, c, hw, eps, _ptr(_dev(stats)),
                                        c_void_p(workspace.data_ptr()) if workspace is not None else None,
                                        workspace.numel() * 8 if workspace is not None else 0, _stream()),
           "vfml_instnorm_finalize")


def stem_chunks(h, w):
    return int(lib().vfml_stem7x7s2_chunks(h, w))


def pack_stem_weight(w, device):
    """[64, 3|4, 7, 7] conv weight -> SplitWeight planes [64][224] in the stem kernel's K order (ky-major rows of 8 taps x 4
    channels, tap 7 and channel 3 zero)."""
    w = w.detach().to(device=device, dtype=torch.float32)
    cout, cin = w.shape[0], w.shape[1]
    if cout != 64 or cin not in (3, 4) or tuple(w.shape[2:]) != (7, 7):
        raise ValueError(f"pack_stem_weight: a [64, 3|4, 7, 7] weight expected, got {tuple(w.shape)}")
    k = torch.zeros(cout, 7, 8, 4, device=device)
    k[:, :, :7, :cin] = w.permute(0, 2, 3, 1)
    sw = SplitWeight(cout, 224, device)
    return sw.fill(k.reshape(-1).contiguous(), scale=SplitWeight.auto_scale(float(w.abs().max())))


def stem7x7s2(frames, n, h, w, weight, bias, out, stats_part=None):
    """vfml_stem7x7s2: frames f32 [n,h,w,4] -> out f32 [n,ho,wo,64] (+ per-tile statistics partials)."""
    if not isinstance(weight, SplitWeight) or weight.rows != 64 or weight.kp != 224:
        raise ValueError("stem7x7s2: weight must come from pack_stem_weight")
    _check(lib().vfml_stem7x7s2(_ptr(_dev(frames)), n, h, w, c_void_p(weight.hi.data_ptr()), c_void_p(weight.lo.data_ptr()),
                                weight.scale, _ptr(_dev(bias)) if bias is not None else None, _ptr(_dev(out)),
                                c_void_p(stats_part.data_ptr()) if stats_part is not None else None, _stream()), "vfml_stem7x7s2")


def instnorm_apply(x, stats, n, hw, c, out, res=None, res_stats=None, out_fmt=FMT_F32):
    """out_fmt FMT_S16: `out` (and a `res` without res_stats, an earlier out) are split rows."""
    _check(lib().vfml_instnorm_apply(_ptr(_dev(x)), _ptr(_dev(stats)), _ptr(res), _ptr(res_stats), n, hw, c,
                                     _ptr(_dev(out)), out_fmt, _stream()), "vfml_instnorm_apply")


def avgpool2x2(x, n, h, w, c, out):
    _check(lib().vfml_avgpool2x2(_ptr(_dev(x)), n, h, w, c, _ptr(_dev(out)), _stream()), "vfml_avgpool2x2")


def softmax_rows_s16(x, rows, cols, ld_in, out, ld_out, x_off=0, out_off=0, scale=1.0):
    """scale * row softmax of f32 scores -> split rows (FMT_S16), zero-filled to ld_out."""
    _check(lib().vfml_softmax_rows_s16(_ptr(_dev(x), x_off), rows, cols, ld_in, _ptr(_dev(out), out_off), ld_out,
                                       float(scale), _stream()), "vfml_softmax_rows_s16")


class PlainWeight:
    """One f16 plane [rows][kp] as the second operand of a GEMM (vfml_conv2d_split with w_lo == NULL)."""
    lo = None
    order = KORDER_TAP

    def __init__(self, rows, kp, device, scale=1.0):
        if kp % 32:
            raise ValueError("PlainWeight: kp must be a multiple of 32")
        self.rows, self.k, self.kp, self.scale = rows, kp, kp, float(scale)
        self.hi = torch.empty(rows * kp, dtype=torch.float16, device=device)


def softmax_rows_f16(x, rows, cols, ld_in, weight, x_off=0):
    """weight.scale * row softmax of f32 scores -> the f16 plane of a PlainWeight (rows of weight.kp halves)."""
    _check(lib().vfml_softmax_rows_f16(_ptr(_dev(x), x_off), rows, cols, ld_in, c_void_p(weight.hi.data_ptr()), weight.kp,
                                       weight.scale, _stream()), "vfml_softmax_rows_f16")


def attention_plane_workspace_bytes(p):
    return int(lib().vfml_attention_plane_workspace_bytes(p))


def attention_plane(q, k, p, plane, score_scale=None, d=128, ld_q=None, ld_k=None, q_off=0, k_off=0, workspace=None):
    """plane (a PlainWeight [p][kp]) = plane.scale * softmax_j(score_scale * q_i . k_j) as one f16 each, pad columns zero, from
    f32 rows q, k [p][d] (float offsets q_off / k_off, row strides ld_q / ld_k) in one call (vfml_attention_plane_f16: the
    scores never reach memory).  score_scale: 1 / sqrt(d) unless given.  workspace: a float32 device tensor of at least 2 p
    elements (None: taken from torch's allocator for this call - stream-ordered)."""
    if not isinstance(plane, PlainWeight):
        raise ValueError("attention_plane: plane must be a PlainWeight")
    if workspace is None:
        workspace = torch.empty(max(1, attention_plane_workspace_bytes(p) // 4), dtype=torch.float32, device=plane.hi.device)
    if workspace.dtype != torch.float32 or workspace.numel() * 4 < attention_plane_workspace_bytes(p) or plane.rows < p:
        raise ValueError("attention_plane: workspace of 2 p floats and a plane of at least p rows")
    _check(lib().vfml_attention_plane_f16(_ptr(_dev(q), q_off), ld_q or d, _ptr(_dev(k), k_off), ld_k or d, p, d,
                                          float(score_scale if score_scale is not None else 1.0 / d ** 0.5), plane.scale,
                                          c_void_p(plane.hi.data_ptr()), plane.kp, c_void_p(workspace.data_ptr()), _stream()),
           "vfml_attention_plane_f16")


ATT_BANK_MAX = 9        # key sets of one vfml_attention_bank_planes_f16 call


def attention_bank_planes(q, keys, p, planes, score_scale=None, d=128, ld_q=None, ld_k=None, q_off=0, k_offs=None,
                          workspace=None):
    """planes[s] (PlainWeights [p][kp] of one kp and one scale) = scale * the columns of key set s of the softmax taken JOINTLY
    over all len(keys) * p scores of every query: q f32 rows [p][d] against keys[s], f32 rows [p][d] of the common stride ld_k
    (float offsets q_off / k_offs[s]), in one call (vfml_attention_bank_planes_f16; the scores never reach memory).
    score_scale: 1 / sqrt(d) unless given.  workspace: a float32 device tensor of at least 2 p elements."""
    n = len(keys)
    if len(planes) != n or not all(isinstance(a, PlainWeight) for a in planes):
        raise ValueError("attention_bank_planes: one PlainWeight per key set")
    if n and any(a.kp != planes[0].kp or a.scale != planes[0].scale or a.rows < p for a in planes):
        raise ValueError("attention_bank_planes: planes of one row stride and one scale, at least p rows each")
    dev = planes[0].hi.device if n else q.device
    if workspace is None:
        workspace = torch.empty(max(1, attention_plane_workspace_bytes(p) // 4), dtype=torch.float32, device=dev)
    if workspace.dtype != torch.float32 or workspace.numel() * 4 < attention_plane_workspace_bytes(p):
        raise ValueError("attention_bank_planes: workspace of 2 p floats")
    k_offs = k_offs or [0] * n
    kptr = (c_void_p * max(1, n))(*[_dev(k).data_ptr() + 4 * o for k, o in zip(keys, k_offs)])
    pptr = (c_void_p * max(1, n))(*[a.hi.data_ptr() for a in planes])
    _check(lib().vfml_attention_bank_planes_f16(_ptr(_dev(q), q_off), ld_q or d, kptr, ld_k or d, n, p, d,
                                                float(score_scale if score_scale is not None else 1.0 / d ** 0.5),
                                                planes[0].scale if n else 1.0, pptr, planes[0].kp if n else 0,
                                                c_void_p(workspace.data_ptr()), _stream()),
           "vfml_attention_bank_planes_f16")


def axpy_f32(x, y, n, scale=1.0, x_off=0, y_off=0):
    """y += scale * x over n floats (vfml_axpy_f32)."""
    _check(lib().vfml_axpy_f32(_ptr(_dev(x), x_off), _ptr(_dev(y), y_off), n, float(scale), _stream()), "vfml_axpy_f32")


DW_RESIDUAL, DW_GELU = 1, 2      # flags of vfml_dwconv2d (include/vfml.h)


def dwconv2d(x, ld_x, n, h, w, c, k, weight, bias, out, ld_out, x_off=0, out_off=0, in_fmt=FMT_F32, out_fmt=FMT_F32,
             residual=False, gelu=False):
    """out = act(x + conv | conv): depthwise k x k convolution (weight [c][k][k] f32, bias [c]) over [n][h][w] rows of ld_x
    floats read at float offset x_off, written to rows of ld_out floats at out_off; residual and exact GELU fused
    (vfml_dwconv2d: f32 FMAs on the vector ALU, zero padding, frames independent)."""
    _check(lib().vfml_dwconv2d(_ptr(_dev(x), x_off), ld_x, n, h, w, c, k, _ptr(_dev(weight)), _ptr(_dev(bias)),
                               _ptr(_dev(out), out_off), ld_out, in_fmt, out_fmt,
                               (DW_RESIDUAL if residual else 0) | (DW_GELU if gelu else 0), _stream()), "vfml_dwconv2d")


def gelu_rows(x, ld_x, out, ld_out, rows, c, x_off=0, out_off=0, in_fmt=FMT_F32, out_fmt=FMT_F32):
    """out[r][:c] = gelu(x[r][:c]) (exact), rows of ld_x / ld_out floats in either format; in place allowed."""
    _check(lib().vfml_gelu_rows(_ptr(_dev(x), x_off), ld_x, _ptr(_dev(out), out_off), ld_out, rows, c, in_fmt, out_fmt,
                                _stream()), "vfml_gelu_rows")


def layernorm_rows(x, ld_x, out, ld_out, rows, c, gamma, beta, eps=1e-5, x_off=0, out_off=0, in_fmt=FMT_F32, out_fmt=FMT_F32):
    """out[r][:c] = LayerNorm(x[r][:c]) * gamma + beta (biased variance, f32 statistics), rows of ld_x / ld_out floats in
    either format; in place allowed where the row strides agree (vfml_layernorm_rows)."""
    _check(lib().vfml_layernorm_rows(_ptr(_dev(x), x_off), ld_x, _ptr(_dev(out), out_off), ld_out, rows, c, _ptr(_dev(gamma)),
                                     _ptr(_dev(beta)), float(eps), in_fmt, out_fmt, _stream()), "vfml_layernorm_rows")


def window_attention(qkv, ld, n, h, w, c, heads, ws, pad_row, out, ld_out, qkv_off=0, out_off=0, in_fmt=FMT_F32, out_fmt=FMT_F32):
    """Locally-grouped attention of the Twins-SVT encoders: qkv [n*h*w][ld] rows (q | k | v, c = heads * 32 each) of the real
    token grid, ws x ws windows anchored at (0, 0), positions outside the grid take pad_row ([3c] f32) and are NOT masked;
    out [n*h*w][ld_out] rows of c channels (vfml_window_attention)."""
    _check(lib().vfml_window_attention(_ptr(_dev(qkv), qkv_off), ld, n, h, w, c, heads, ws, _ptr(_dev(pad_row)),
                                       _ptr(_dev(out), out_off), ld_out, in_fmt, out_fmt, _stream()), "vfml_window_attention")


def attention_shared_keys(q, ld_q, kv, ld_kv, n, p, pk, c, heads, out, ld_out, q_off=0, kv_off=0, out_off=0, q_fmt=FMT_F32,
                          kv_fmt=FMT_F32, out_fmt=FMT_F32):
    """Per frame and head, p queries (q [n*p][ld_q]) against the same pk keys and values (kv [n*pk][ld_kv], k | v), head
    dimension 32: out [n*p][ld_out] = softmax(q k^T / sqrt 32) v, online softmax on the f32 matrix cores
    (vfml_attention_shared_keys)."""
    _check(lib().vfml_attention_shared_keys(_ptr(_dev(q), q_off), ld_q, _ptr(_dev(kv), kv_off), ld_kv, n, p, pk, c, heads,
                                            _ptr(_dev(out), out_off), ld_out, q_fmt, kv_fmt, out_fmt, _stream()),
           "vfml_attention_shared_keys")


def transpose_to_s16(src, rows, c, ld, dst, ld_dst, scale=1.0, src_off=0, dst_off=0):
    """f32 [rows][c] -> split rows [c][ld_dst] of its transpose times scale."""
    _check(lib().vfml_transpose_to_s16(_ptr(_dev(src), src_off), rows, c, ld, float(scale), _ptr(_dev(dst), dst_off), ld_dst,
                                       _stream()), "vfml_transpose_to_s16")


def add_to_s16(x, ldx, aux, ld_aux, out, ld_out, rows, c, scale=1.0, x_off=0, aux_off=0, out_off=0):
    """out = aux + scale * x (x f32, aux / out split rows)."""
    _check(lib().vfml_add_to_s16(_ptr(_dev(x), x_off), ldx, _ptr(_dev(aux), aux_off), ld_aux, _ptr(_dev(out), out_off), ld_out,
                                 rows, c, float(scale), _stream()), "vfml_add_to_s16")


def to_s16(src, rows, c, ld_src, dst, ld_dst, src_off=0, dst_off=0, scale=1.0):
    """scale * f32 rows [rows][c] -> split rows (FMT_S16) at float offset dst_off of dst."""
    _check(lib().vfml_to_s16(_ptr(_dev(src), src_off), rows, c, ld_src, _ptr(_dev(dst), dst_off), ld_dst, float(scale),
                             _stream()), "vfml_to_s16")


PTR_TABLE_MAX = 48      # pointers per vfml_ptr_table_set launch


def ptr_table_set(table, tensors):
    """Write the device pointers of `tensors` into `table` (an int64 device tensor), asynchronously on the current stream."""
    n = len(tensors)
    if not (table.is_cuda and table.dtype == torch.int64 and table.numel() >= n):
        raise ValueError("ptr_table_set: table must be an int64 device tensor with room for the pointers")
    vals = [t if isinstance(t, int) else t.data_ptr() for t in tensors]     # (an int: the cell's value itself)
    for at in range(0, n, PTR_TABLE_MAX):       # (a launch carries the values as its arguments: 48 of them)
        part = vals[at:at + PTR_TABLE_MAX]
        _check(lib().vfml_ptr_table_set(c_void_p(table.data_ptr() + 8 * at), (c_void_p * len(part))(*part), len(part), _stream()),
               "vfml_ptr_table_set")


def corr_bitmap_words(rows, cols):
    """uint32 words of a level's bitmap (vfml_corr_level0_ensure, vfml_corr_levels_ensure): one bit per 128-row x 64-column
    tile, whole words per row tile."""
    return ((rows + 127) // 128) * (((cols + 63) // 64 + 31) // 32)


def corr_level0_ensure(rows, c, weight, level0, n_rows, n_cols, ldo, out_scale, cells, centres, dirs, dir_cells, coords,
                       coords_off, ld_coords, dir_coords, h, w, radius, vol_tile, counter=None, in_fmt=FMT_S16, mfma=1):
    """The level-0 tiles the next lookup reads and the pyramids do not hold yet (include/vfml.h vfml_corr_level0_ensure).
    rows / weight / level0 (with c channels, n_rows x n_cols, ldo, out_scale, in_fmt, mfma): the dense level-0 call
    `conv2d(rows, c, c, 1, 1, n_rows, weight, None, n_cols, 1, 1, level0, ldo, ...)` of any one of the pyramids; cells: an
    int64 device tensor, four per (direction, centre) - query rows, target hi plane, level 0, bitmap (ptr_table_set);
    coords .. vol_tile: as corr_lookup's; counter: an int32 device cell the number of computed tiles is added to."""
    if not isinstance(weight, SplitWeight) or weight.lo is None:
        raise ValueError("corr_level0_ensure: the target operand is a SplitWeight")
    ndirs = 2 if dirs == 2 else 1
    if not (cells.is_cuda and cells.dtype == torch.int64 and cells.numel() >= 4 * ((ndirs - 1) * dir_cells + centres)):
        raise ValueError("corr_level0_ensure: cells must be an int64 device tensor, four per direction and centre frame")
    if counter is not None and not (counter.is_cuda and counter.dtype == torch.int32):
        raise ValueError("corr_level0_ensure: the counter is an int32 device tensor")
    d = ConvDesc()
    d.in0, d.c0, d.ld0 = _ptr(_dev(rows)), c, c
    d.n, d.h, d.w = 1, 1, n_rows
    d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w = n_cols, 1, 1, 1, 0, 0
    d.out, d.ldo = _ptr(_dev(level0)), ldo
    d.epilogue, d.split, d.out_scale = EPI_NONE, 0, out_scale
    d.flags = {3: 0, 2: CONV_MFMA2, 1: CONV_MFMA1}[mfma]
    _check(lib().vfml_corr_level0_ensure(ctypes.byref(d), c_void_p(weight.hi.data_ptr()), c_void_p(weight.lo.data_ptr()),
                                         weight.kp, weight.scale, in_fmt, FMT_F32, weight.order, c_void_p(cells.data_ptr()),
                                         centres, ndirs, dir_cells, _ptr(_dev(coords), coords_off), ld_coords, dir_coords, h, w,
                                         radius, vol_tile, c_void_p(counter.data_ptr()) if counter is not None else None,
                                         _stream()), "vfml_corr_level0_ensure")


def corr_levels_ensure(rows, c, n_rows, levels, out_scale, cells, centres, dirs, dir_cells, coords, coords_off, ld_coords,
                       dir_coords, h, w, radius, vol_tile, counters=None, in_fmt=FMT_S16, mfma=1):
    """The tiles of several pyramid levels that the next lookup reads and the pyramids do not hold yet, in one launch
    (include/vfml.h vfml_corr_levels_ensure).  rows (c channels, n_rows of them): the query rows of any one of the pyramids;
    levels: a list of (level, weight, volume, n_cols, ldo, h_l, w_l) in ascending order of level - the dense call
    `conv2d(rows, c, c, 1, 1, n_rows, weight, None, n_cols, 1, 1, volume, ldo, ...)` of that level and its image; cells: an
    int64 device tensor, 1 + 3 * len(levels) per (direction, centre) - query rows, then per level target hi plane, level
    buffer, bitmap (corr_bitmap_words(n_rows, n_cols) words); h, w: the query map; counters: an int32 device tensor, cell l
    counts the tiles computed at level l.  Everything else as corr_level0_ensure."""
    ndirs = 2 if dirs == 2 else 1
    per = 1 + 3 * len(levels)
    if not levels or any(not isinstance(lv[1], SplitWeight) or lv[1].lo is None for lv in levels):
        raise ValueError("corr_levels_ensure: every level's target operand is a SplitWeight")
    if not (cells.is_cuda and cells.dtype == torch.int64 and cells.numel() >= per * ((ndirs - 1) * dir_cells + centres)):
        raise ValueError("corr_levels_ensure: cells must be an int64 device tensor, 1 + 3 per level for each direction and "
                         "centre frame")
    if counters is not None and not (counters.is_cuda and counters.dtype == torch.int32
                                     and counters.numel() > max(lv[0] for lv in levels)):
        raise ValueError("corr_levels_ensure: the counters are an int32 device tensor with a cell per pyramid level")
    descs = (ConvDesc * len(levels))()
    lvs = (CorrLevelDesc * len(levels))()
    for i, (level, weight, volume, n_cols, ldo, hl, wl) in enumerate(levels):
        d = descs[i]
        d.in0, d.c0, d.ld0 = _ptr(_dev(rows)), c, c
        d.n, d.h, d.w = 1, 1, n_rows
        d.cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w = n_cols, 1, 1, 1, 0, 0
        d.out, d.ldo = _ptr(_dev(volume)), ldo
        d.epilogue, d.split, d.out_scale = EPI_NONE, 0, out_scale
        d.flags = {3: 0, 2: CONV_MFMA2, 1: CONV_MFMA1}[mfma]
        lv = lvs[i]
        lv.d = ctypes.pointer(d)
        lv.w_hi, lv.w_lo, lv.kp, lv.w_scale = weight.hi.data_ptr(), weight.lo.data_ptr(), weight.kp, weight.scale
        lv.out_fmt, lv.level, lv.h, lv.w = FMT_F32, level, hl, wl
    order = levels[0][1].order
    _check(lib().vfml_corr_levels_ensure(lvs, len(levels), in_fmt, order, c_void_p(cells.data_ptr()), centres, ndirs, dir_cells,
                                         _ptr(_dev(coords), coords_off), ld_coords, dir_coords, h, w, radius, vol_tile,
                                         c_void_p(counters.data_ptr()) if counters is not None else None, _stream()),
           "vfml_corr_levels_ensure")


SEED_NONE, SEED_LOAD, SEED_STORE = 0, 1, 2
LOOKUP_KEY_NONE = -2 ** 31       # a patch-cache key no window origin takes (corr_lookup's `cache`)


def window_seed(cells, ncentres, rows, cols, state, ld_state, h_off, mf_off, ld_ctx):
    """Window set-up of the recurrent state as one launch (include/vfml.h vfml_window_seed): per centre frame the cells
    (an int64 device tensor, three per frame: context map, slot, SEED_*; ptr_table_set writes them) name what is copied into
    the h columns, and into or out of the mf columns, of the frame's state rows."""
    if not (cells.is_cuda and cells.dtype == torch.int64 and cells.numel() >= 3 * ncentres):
        raise ValueError("window_seed: cells must be an int64 device tensor, three per centre frame")
    _check(lib().vfml_window_seed(c_void_p(cells.data_ptr()), ncentres, rows, cols, _ptr(_dev(state)), ld_state, h_off, mf_off,
                                  ld_ctx, _stream()), "vfml_window_seed")


def corr_lookup(pyrs, hl, wl, ld, radius, q_per_map, coords, coords_off, ld_coords, out, out_off, ld_out,
                out_fmt=FMT_F32, table=None, nmaps=None, vol_fmt=FMT_F32, vol_tile=0, bidir=None, cache=None):
    """pyrs: list (one entry per query map) of lists (one flat float32 device tensor per level, rows =
    that map's q_per_map queries).  Queries / coords / out rows are ordered map-major.
    table (with nmaps): instead of `pyrs`, an int64 device tensor holding the same pointers, map-major
    (ptr_table_set), read when the kernel runs (vfml_corr_lookup_indirect).
    vol_tile: 0 (row-major level images, rows in query order) or VolTile.code (include/vfml.h).
    bidir = (dir_coords, dir_out, dir_tab) with a table: both directions of the nmaps query maps in one launch
    (vfml_corr_lookup_indirect_bidir).
    cache (with bidir; radius 3 or 4) = (patches, keys, rows, row0, store, counter): the launch keeps every query's gathered
    patch and window origins in `patches` (f32) / `keys` (int32, LOOKUP_KEY_NONE = no entry) at row row0 + its query row of
    `rows` per direction, and gathers only where the origins differ from the kept ones
    (vfml_corr_lookup_indirect_bidir_cached; counter: None or an int32 device tensor [hits, misses])."""
    L = len(hl)
    if cache is not None:
        if bidir is None or table is None:
            raise ValueError("corr_lookup: the patch cache goes with the bidirectional table lookup")
        patches, keys, rows, row0, store, counter = cache
        if keys.dtype != torch.int32 or (counter is not None and counter.dtype != torch.int32):
            raise ValueError("corr_lookup: cache keys and counter are int32 device tensors")
        side = 2 * radius + 2
        if patches.numel() < 2 * rows * 4 * side * side or keys.numel() < 2 * rows * 8:
            raise ValueError(f"corr_lookup: cache of {patches.numel()} floats / {keys.numel()} keys is too small for 2 x {rows} rows")
    # the four entry points take the same arguments, plus the second direction's and then the cache's where they have them
    name = "vfml_corr_lookup"
    if bidir is None and table is None:
        if pyrs and torch.is_tensor(pyrs[0]):
            pyrs = [pyrs]
        nmaps, L = len(pyrs), len(pyrs[0])
        head = (c_void_p * (nmaps * L))(*[p.data_ptr() for m in pyrs for p in m])
    else:
        name += "_indirect"
        head = c_void_p(table.data_ptr())
    args = [head, (c_int32 * L)(*hl), (c_int32 * L)(*wl), (c_int32 * L)(*ld), L, radius, nmaps, q_per_map]
    src, dst = [_ptr(_dev(coords), coords_off), ld_coords], [_ptr(_dev(out), out_off), ld_out]
    if bidir is not None:
        name += "_bidir"
        dir_coords, dir_out, dir_tab = bidir
        src += [dir_coords]
        dst += [dir_out, dir_tab]
    args += src + dst + [out_fmt, vol_fmt, vol_tile]
    if cache is not None:
        name += "_cached"
        args += [_ptr(_dev(patches)), c_void_p(_dev(keys, torch.int32).data_ptr()), rows, row0, int(bool(store)),
                 c_void_p(counter.data_ptr()) if counter is not None else None]

    def launch():
        _check(getattr(lib(), name)(*args, _stream()), name)

    if _PROFILE_HBM is None:
        launch()
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    # algorithmic bytes: per query and level the (2r+2)^2 integer-grid patch in, (2r+1)^2 samples out
    q = (2 if bidir is not None else 1) * nmaps * q_per_map
    m16 = _vol_mask(vol_fmt, L)
    texel_bytes = sum(2.0 if (m16 >> l) & 1 else 4.0 for l in range(L))
    _PROFILE_HBM.append(("corr_lookup", q * ((2 * radius + 2) ** 2 * texel_bytes + L * (2 * radius + 1) ** 2 * 4.0), e0, e1))


class VolTile:
    """Tiled layout of the correlation volume (include/vfml.h vfml_corr_lookup, vol_tile): level images - and the level-0
    grid that orders the volume's rows - stored as 2^tws x 2^ths tiles.  The volume GEMM produces it for free when the rows
    of both its operands are in tile order: `position(h, w)` is where each row-major pixel goes, `count(h, w)` how many rows
    the whole tiles take (positions no pixel maps to are zero rows: their volume entries are never read)."""

    def __init__(self, tws, ths):
        self.tws, self.ths = tws, ths
        self.code = tws + 16 * ths
        self._pos = {}

    def count(self, h, w):
        return ((((h - 1) >> self.ths) + 1) * (((w - 1) >> self.tws) + 1)) << (self.tws + self.ths)

    def position(self, h, w, dev):
        key = (h, w, str(dev))
        if key not in self._pos:
            y = torch.arange(h, device=dev, dtype=torch.int64).view(h, 1)
            x = torch.arange(w, device=dev, dtype=torch.int64).view(1, w)
            tpr = ((w - 1) >> self.tws) + 1
            pos = ((((y >> self.ths) * tpr + (x >> self.tws)) << (self.tws + self.ths))
                   + ((y & ((1 << self.ths) - 1)) << self.tws) + (x & ((1 << self.tws) - 1)))
            self._pos[key] = pos.reshape(-1).contiguous()
        return self._pos[key]

    def rows(self, x, h, w, c):
        """x: flat [h*w*c] row-major pixels -> flat [count(h, w)*c] in tile order, zero rows where no pixel lands."""
        n = self.count(h, w)
        out = torch.zeros(n, c, device=x.device, dtype=x.dtype)
        out.index_copy_(0, self.position(h, w, x.device), x.view(h * w, c))
        return out.view(-1)


def coords_init(coords1, n, h, w):
    _check(lib().vfml_coords_init(_ptr(_dev(coords1)), n, h, w, _stream()), "vfml_coords_init")


def flow_rows7(flow, n, h, w, rows):
    """rows[p] = the seven horizontal taps' flow quads of pixel p as 32 split-row channels (include/vfml.h vfml_flow_rows7)."""
    _check(lib().vfml_flow_rows7(_ptr(_dev(flow)), n, h, w, _ptr(_dev(rows)), _stream()), "vfml_flow_rows7")


def tapsum3x3(t, ld_t, bias, n, h, w, out, parts=1, part_stride=0):
    """out[p][0:4] = bias + the nine taps' quads of the tap-major 36-column map t (include/vfml.h vfml_tapsum3x3); parts > 1: t is
    that many maps part_stride floats apart whose sum is meant (conv2d(..., proj_out=))."""
    _check(lib().vfml_tapsum3x3(_ptr(_dev(t)), ld_t, _ptr(bias) if bias is not None else None, n, h, w, _ptr(_dev(out)),
                                parts, part_stride, _stream()), "vfml_tapsum3x3")


def conv3x3_c64(src, ld_in, n, h, w, weight, bias, out, ldo, stats_part=None, src_off=0):
    """The encoders' 64 -> 64 channel 3x3 convolution over split rows with its norm partial sums (include/vfml.h
    vfml_conv3x3_c64; image width a multiple of 32, weights in KORDER_CBLOCK order)."""
    _check(lib().vfml_conv3x3_c64(_ptr(_dev(src), src_off), ld_in, n, h, w, c_void_p(weight.hi.data_ptr()),
                                  c_void_p(weight.lo.data_ptr()), weight.kp, weight.scale,
                                  _ptr(_dev(bias)) if bias is not None else None, _ptr(_dev(out)), ldo,
                                  c_void_p(stats_part.data_ptr()) if stats_part is not None else None, _stream()),
           "vfml_conv3x3_c64")


def flow_half(flow, n, h, w, w1, b1, w2, b2, out, ld_out, out_off=0):
    """relu(convf2(relu(convf1(flow)))) of the motion encoder as one launch (include/vfml.h vfml_flow_half): w1 / w2 the
    layers' SplitWeights (rows7 layout / 64-channel-block order), plain f16 products."""
    _check(lib().vfml_flow_half(_ptr(_dev(flow)), n, h, w, c_void_p(w1.hi.data_ptr()), w1.kp, w1.scale, _ptr(_dev(b1)),
                                c_void_p(w2.hi.data_ptr()), w2.kp, w2.scale, _ptr(_dev(b2)), _ptr(_dev(out), out_off), ld_out,
                                _stream()), "vfml_flow_half")


def tapsum3x3_update(t, ld_t, bias, n, h, w, coords1, parts=1, part_stride=0, flow_a=None, ld_a=0, flow_a_off=0, flow_b=None,
                     ld_b=0, flow_b_off=0, fmt_b=FMT_F32):
    """tapsum3x3 and coords_update(delta = that sum) as one launch (include/vfml.h vfml_tapsum3x3_update)."""
    _check(lib().vfml_tapsum3x3_update(_ptr(_dev(t)), ld_t, _ptr(bias) if bias is not None else None, n, h, w, parts, part_stride,
                                       _ptr(_dev(coords1)), _ptr(flow_a, flow_a_off), ld_a, _ptr(flow_b, flow_b_off), ld_b,
                                       fmt_b, _stream()), "vfml_tapsum3x3_update")


def coords_update(coords1, delta, n, h, w, flow_a=None, ld_a=0, flow_a_off=0, flow_b=None, ld_b=0, flow_b_off=0,
                  fmt_b=FMT_F32):
    _check(lib().vfml_coords_update(_ptr(_dev(coords1)), _ptr(delta), n, h, w,
                                    _ptr(flow_a, flow_a_off), ld_a, _ptr(flow_b, flow_b_off), ld_b, fmt_b, _stream()),
           "vfml_coords_update")


def flow_forward_interpolate_workspace(n, h, w, device):
    """The workspace of flow_forward_interpolate for n maps of h x w cells (vfml_flow_forward_interpolate_workspace_bytes)."""
    nbytes = lib().vfml_flow_forward_interpolate_workspace_bytes(n, h, w)
    return torch.empty(max(1, nbytes // 8), dtype=torch.int64, device=device)


def flow_forward_interpolate(flow, h=None, w=None, n=1, ld_in=None, out=None, ld_out=None, index=None, workspace=None):
    """A 1/8-resolution flow projected forward along itself (vfml_flow_forward_interpolate): every
    source cell moves by its own flow, every target cell takes the flow of the nearest landing point inside the frame, ties to
    the lowest source index, zero when no source stays inside.
    flow: float32 device tensor, [h, w, 2] (or [n, h, w, c], c = 2 or 4: then h, w, n and ld_in come from its shape) or flat
    rows of ld_in floats with h, w, n given.  out: rows of ld_out floats (default: flow's own layout, a new tensor); with
    ld_out = 4 channels 2..3 are written as zero: the `delta` operand of coords_update.  index: optional int32 tensor of
    n * h * w entries that receives the chosen source per cell (-1: none valid).  workspace: from
    flow_forward_interpolate_workspace, or allocated here.  Stream-ordered, no host synchronisation.  Returns out."""
    _dev(flow)
    shape = None
    if h is None or w is None:
        if flow.dim() not in (3, 4) or flow.shape[-1] not in (2, 4):
            raise ValueError(f"flow_forward_interpolate: flow [h, w, 2] or [n, h, w, c] expected (or flat rows with h, w), "
                             f"got {tuple(flow.shape)}")
        shape = tuple(flow.shape)
        h, w, ld_in = shape[-3], shape[-2], shape[-1]
        n = shape[0] if flow.dim() == 4 else 1
    ld_in = ld_in or 2
    ld_out = ld_out or ld_in
    if flow.numel() < n * h * w * ld_in:
        raise ValueError(f"flow_forward_interpolate: flow holds {flow.numel()} floats, {n} x {h} x {w} x {ld_in} expected")
    if out is None:
        out = torch.empty(shape[:-1] + (ld_out,) if shape else (n * h * w * ld_out,), dtype=torch.float32, device=flow.device)
    if _dev(out).device != flow.device or out.numel() < n * h * w * ld_out:
        raise ValueError(f"flow_forward_interpolate: out of {n} x {h} x {w} x {ld_out} floats on {flow.device} expected")
    if index is not None and (_dev(index, torch.int32).device != flow.device or index.numel() < n * h * w):
        raise ValueError(f"flow_forward_interpolate: index of {n} x {h} x {w} int32 on {flow.device} expected")
    if workspace is None:
        workspace = flow_forward_interpolate_workspace(n, h, w, flow.device)
    if _dev(workspace, torch.int64).device != flow.device:
        raise ValueError(f"flow_forward_interpolate: workspace on {flow.device} expected")
    _check(lib().vfml_flow_forward_interpolate(_ptr(flow), ld_in, n, h, w, _ptr(out), ld_out,
                                               None if index is None else c_void_p(index.data_ptr()),
                                               c_void_p(workspace.data_ptr()), workspace.numel() * 8, _stream()),
           "vfml_flow_forward_interpolate")
    return out


def flow_lods(flow, num_lods=5):
    """[H,W,2] float32 device tensor -> list of `num_lods` device tensors (level 0 is `flow` itself)."""
    lods = [_dev(flow.contiguous())]
    for _ in range(1, num_lods):
        h, w = lods[-1].shape[:2]
        out = torch.empty((h + 1) // 2, (w + 1) // 2, 2, device=flow.device, dtype=torch.float32)
        _check(lib().vfml_flow_lod(_ptr(lods[-1]), h, w, _ptr(out), _stream()), "vfml_flow_lod")
        lods.append(out)
    return lods


ENCODE_GAMEDEV, ENCODE_RG8, ENCODE_RGB8 = 0, 1, 2


def flow_encode(flow, mode, clamp_range, width=1.0, height=1.0, scale=1.0):
    """[H,W,2] float32 device tensor -> [H,W,3] uint8 device tensor (vfml_flow_encode)."""
    import numpy as np
    f = _dev(flow.contiguous())
    h, w = f.shape[:2]
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=f.device)
    _check(lib().vfml_flow_encode(_ptr(f), h, w, mode, float(np.float32(width)), float(np.float32(height)),
                                  float(np.float32(scale)), float(np.float32(clamp_range)),
                                  float(np.float32(2 * clamp_range)), c_void_p(out.data_ptr()), _stream()),
           "vfml_flow_encode")
    return out


TAA_SIMPLE, TAA_BILINEAR, TAA_BILATERAL = 0, 1, 2
_PIX = {torch.uint8: 0, torch.float32: 1, torch.float64: 2}


def taa_blend(current, flow, history, mode, alpha, sigma_color=25.0):
    """One TAA step on the device (vfml_taa_blend): current [H,W,3] u8/f32, flow [H,W,2] f32 or None, history
    [H,W,3] f32/f64 -> new history, in the dtype the reference's numpy arithmetic gives it."""
    cur, hist = current.contiguous(), history.contiguous()
    if not (cur.is_cuda and hist.is_cuda and cur.dtype in (torch.uint8, torch.float32)
            and hist.dtype in (torch.float32, torch.float64)):
        raise ValueError(f"taa_blend: device tensors u8/f32 + f32/f64 expected, got {cur.dtype} {hist.dtype}")
    h, w = cur.shape[:2]
    if tuple(cur.shape) != (h, w, 3) or tuple(hist.shape) != (h, w, 3):
        raise ValueError(f"taa_blend: [H,W,3] images expected, got {tuple(cur.shape)} {tuple(hist.shape)}")
    if mode != TAA_SIMPLE:
        flow = _dev(flow.contiguous())
        if tuple(flow.shape) != (h, w, 2):
            raise ValueError(f"taa_blend: flow {tuple(flow.shape)} does not match the frame {h}x{w}")
    out_dtype = hist.dtype if mode == TAA_SIMPLE else (torch.float32 if mode == TAA_BILINEAR else torch.float64)
    out = torch.empty((h, w, 3), dtype=out_dtype, device=cur.device)
    _check(lib().vfml_taa_blend(c_void_p(cur.data_ptr()), _PIX[cur.dtype], None if mode == TAA_SIMPLE else _ptr(flow),
                                c_void_p(hist.data_ptr()), _PIX[hist.dtype], c_void_p(out.data_ptr()), _PIX[out_dtype],
                                h, w, mode, float(alpha), float(sigma_color), _stream()), "vfml_taa_blend")
    return out


COLORIZE_HSV, COLORIZE_WHEEL = 0, 1


def flow_colorize(flow, mode):
    """[H,W,2] float32 device tensor -> [H,W,3] uint8 device tensor on the HSV or torchvision colour wheel
    (vfml_flow_colorize; the frame maximum is reduced on the device, no host sync)."""
    f = _dev(flow.contiguous())
    if f.dim() != 3 or f.shape[2] != 2:
        raise ValueError(f"flow_colorize: [H,W,2] flow expected, got {tuple(f.shape)}")
    h, w = f.shape[:2]
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=f.device)
    cell = torch.empty(1, dtype=torch.int32, device=f.device)
    _check(lib().vfml_flow_colorize(_ptr(f), h, w, mode, c_void_p(cell.data_ptr()), c_void_p(out.data_ptr()), _stream()),
           "vfml_flow_colorize")
    return out


def flow_decode(encoded, mode, clamp_range):
    """Encoded motion vectors [H,W,3] uint8 (device tensor with contiguous rows: a whole picture or a row slice of an
    uploaded frame) -> flow [H,W,2] float32 device tensor (vfml_flow_decode; ENCODE_RG8 or ENCODE_RGB8)."""
    import numpy as np
    e = _dev(encoded, torch.uint8)
    if e.dim() != 3 or e.shape[2] != 3:
        raise ValueError(f"flow_decode: [H,W,3] picture expected, got {tuple(e.shape)}")
    h, w = e.shape[:2]
    out = torch.empty((h, w, 2), dtype=torch.float32, device=e.device)
    _check(lib().vfml_flow_decode(c_void_p(e.data_ptr()), h, w, mode, float(np.float32(clamp_range)), _ptr(out),
                                  _stream()), "vfml_flow_decode")
    return out


def flow_diff_overlay(flow_a, flow_b):
    """Two flows [H,W,2] float32 (device tensors) -> the radar picture of their difference with its legend squares,
    [H,W,3] uint8 RGB device tensor (vfml_flow_diff_overlay)."""
    a, b = _dev(flow_a.contiguous()), _dev(flow_b.contiguous())
    if a.dim() != 3 or a.shape[2] != 2 or a.shape != b.shape:
        raise ValueError(f"flow_diff_overlay: two [H,W,2] flows of one size expected, got {tuple(a.shape)} "
                         f"{tuple(b.shape)}")
    h, w = a.shape[:2]
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=a.device)
    _check(lib().vfml_flow_diff_overlay(_ptr(a), _ptr(b), h, w, c_void_p(out.data_ptr()), _stream()),
           "vfml_flow_diff_overlay")
    return out


COMPOSE_SIDE_BY_SIDE, COMPOSE_STACKED, COMPOSE_GRID_2X2, COMPOSE_GRID_2X3 = 0, 1, 2, 3
COMPOSE_BGR, COMPOSE_BOTTOM_UP = 1, 2


def compose_frame(tiles, layout, bgr=True, bottom_up=False, row_stride=None, out=None):
    """One output frame (vfml_compose_frame): tiles = 2 (SIDE_BY_SIDE, STACKED), 4 (GRID_2X2) or 6 (GRID_2X3) device images [H,W,3],
    uint8 or float32 / float64 TAA histories -> uint8 device buffer [rows, row_stride] (row_stride defaults to 3 x the
    output width).  `out`, when given, is a contiguous uint8 device tensor of at least rows x row_stride bytes."""
    nt = {COMPOSE_GRID_2X2: 4, COMPOSE_GRID_2X3: 6}.get(layout, 2)
    if len(tiles) != nt:
        raise ValueError(f"compose_frame: layout {layout} takes {nt} tiles, got {len(tiles)}")
    ts = [t.contiguous() for t in tiles]
    h, w = ts[0].shape[:2]
    for t in ts:
        if not (t.is_cuda and t.dtype in _PIX and tuple(t.shape) == (h, w, 3)):
            raise ValueError(f"compose_frame: device [H,W,3] u8/f32/f64 tiles of one size expected, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    ow = w if layout == COMPOSE_STACKED else 2 * w
    oh = h if layout == COMPOSE_SIDE_BY_SIDE else (3 * h if layout == COMPOSE_GRID_2X3 else 2 * h)
    stride = 3 * ow if row_stride is None else int(row_stride)
    if out is None:
        out = torch.empty((oh, stride), dtype=torch.uint8, device=ts[0].device)
    elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= oh * stride):
        raise ValueError(f"compose_frame: out must be a contiguous uint8 device tensor of >= {oh * stride} bytes")
    ptrs = (c_void_p * nt)(*[t.data_ptr() for t in ts])
    types = (c_int32 * nt)(*[_PIX[t.dtype] for t in ts])
    flags = (COMPOSE_BGR if bgr else 0) | (COMPOSE_BOTTOM_UP if bottom_up else 0)
    _check(lib().vfml_compose_frame(ptrs, types, h, w, layout, flags, stride, c_void_p(out.data_ptr()), _stream()),
           "vfml_compose_frame")
    return out


class TextPlan:
    """A compiled draw list (visualization.text.build_plan) ready for text_draw: the host words, which vfml_text_draw checks
    before every launch, and their copy on `device`, which the kernel reads; the host words carry the copy's address."""

    def __init__(self, words, device):
        import numpy as np
        self.host = np.array(words, dtype=np.int32)
        if self.host.ndim != 1 or self.host.size < 8:
            raise ValueError("TextPlan: a one-dimensional int32 plan of at least 8 words expected")
        self.dev = torch.empty(self.host.size, dtype=torch.int32, device=device)
        addr = self.dev.data_ptr()
        self.host[2:4] = np.array([addr & 0xffffffff, addr >> 32], dtype=np.uint32).view(np.int32)
        self.dev.copy_(torch.from_numpy(self.host))

    @property
    def boxes(self):
        return int(self.host[4])


def text_draw(plan, img, h, w, row_stride=None, bottom_up=False):
    """Draw a TextPlan into a composed frame in place (vfml_text_draw): img is a contiguous uint8 device tensor holding
    h rows of row_stride bytes (default 3 w), channels in memory order; bottom_up as compose_frame writes a DIB."""
    stride = 3 * w if row_stride is None else int(row_stride)
    if not (img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.numel() >= h * stride):
        raise ValueError(f"text_draw: img must be a contiguous uint8 device tensor of >= {h * stride} bytes")
    if plan.dev.device != img.device:
        raise ValueError(f"text_draw: the plan lives on {plan.dev.device}, the frame on {img.device}")
    _check(lib().vfml_text_draw(plan.host.ctypes.data_as(c_void_p), plan.host.size, c_void_p(img.data_ptr()), h, w, stride,
                                COMPOSE_BOTTOM_UP if bottom_up else 0, _stream()), "vfml_text_draw")
    return img


def flow_quality_map(frame1, frame2, flow, threshold):
    """uint8 frames [H,W,3] + flow [fh,fw,2] f32 (device tensors) -> uint8 quality map [H,W,3] (vfml_flow_quality_map)."""
    f1, f2, fl = _dev(frame1.contiguous(), torch.uint8), _dev(frame2.contiguous(), torch.uint8), _dev(flow.contiguous())
    h, w = f1.shape[:2]
    if tuple(f1.shape) != (h, w, 3) or f2.shape != f1.shape or fl.dim() != 3 or fl.shape[2] != 2:
        raise ValueError(f"flow_quality_map: frames {tuple(f1.shape)} {tuple(f2.shape)}, flow {tuple(fl.shape)}")
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=f1.device)
    _check(lib().vfml_flow_quality_map(c_void_p(f1.data_ptr()), c_void_p(f2.data_ptr()), _ptr(fl), fl.shape[0], fl.shape[1],
                                       h, w, float(threshold), c_void_p(out.data_ptr()), _stream()), "vfml_flow_quality_map")
    return out


_TURBULENCE_WS = {}


def flow_turbulence_map(flow, height, width, kernel_size=25, want=()):
    """flow [fh,fw,2] f32 device tensor -> the turbulence map of a height x width frame, uint8 [height,width,3] in cv2's
    channel order (B first) on the device (vfml_flow_turbulence_map: stream-ordered, no host synchronisation).
    want: names of further results, returned after the picture in the order given - "index" (uint8 [H,W], the JET entry
    of each pixel), "tv" (float32 [H,W], the local deviation), "lohi" (float32 [2], its 5th and 95th percentile).
    The workspace is kept per device, picture size and stream."""
    f = _dev(flow.contiguous())
    if f.dim() != 3 or f.shape[2] != 2 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError(f"flow_turbulence_map: [fh,fw,2] flow expected, got {tuple(f.shape)}")
    h, w, k = int(height), int(width), int(kernel_size)
    if h < 1 or w < 1:
        raise ValueError(f"flow_turbulence_map: frame {h}x{w}")
    if k % 2 == 0 or not 1 <= k <= 63:
        raise ValueError(f"flow_turbulence_map: kernel_size {k} is not an odd number in 1..63")
    extra = {"index": ((h, w), torch.uint8), "tv": ((h, w), torch.float32), "lohi": ((2,), torch.float32)}
    for name in want:
        if name not in extra:
            raise ValueError(f"flow_turbulence_map: want={name!r}; one of {sorted(extra)}")
    L = lib()
    key = (f.device.index, h, w, torch.cuda.current_stream().cuda_stream)
    ws = _TURBULENCE_WS.get(key)
    if ws is None:
        ws = _TURBULENCE_WS[key] = torch.empty(L.vfml_flow_turbulence_workspace_bytes(h, w), dtype=torch.uint8,
                                               device=f.device)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=f.device)
    more = {name: torch.empty(extra[name][0], dtype=extra[name][1], device=f.device) for name in want}

    def opt(name):
        return c_void_p(more[name].data_ptr()) if name in more else None
    _check(L.vfml_flow_turbulence_map(_ptr(f), f.shape[0], f.shape[1], h, w, k, c_void_p(ws.data_ptr()),
                                      c_void_p(out.data_ptr()), opt("index"), opt("tv"), opt("lohi"), _stream()),
           "vfml_flow_turbulence_map")
    return (out, *[more[name] for name in want]) if want else out


_RESIZE_TABLES = {}


def resize_tables(S, D, device=None):
    """Taps and weights of one axis of the picture resize: int32 [D, 4] rows (s, s1, a0, a1) for a
    source of S and a destination of D pixels - the scheme's only float work, done here in numpy for the host path
    (video.resize_frame) and the kernel (vfml_resize_u8) alike.  device=None: the numpy table (read-only); else the same
    rows as a device tensor.  Cached per (S, D, device)."""
    import numpy as np
    S, D = int(S), int(D)
    if S < 1 or D < 1:
        raise ValueError(f"resize_tables: lengths {S} -> {D}")
    if device is not None:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
    key = (S, D, None if device is None else str(device))
    tab = _RESIZE_TABLES.get(key)
    if tab is not None:
        return tab
    if device is not None:
        tab = torch.tensor(resize_tables(S, D)).to(device)
    else:
        scale = np.float64(S) / np.float64(D)
        f = ((np.arange(D, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
        s = np.floor(f)
        f = (f - s).astype(np.float32)                  # float32 - float32
        s = s.astype(np.int64)
        lo, hi = s < 0, s >= S - 1
        s[lo], f[lo] = 0, 0
        s[hi], f[hi] = S - 1, 0
        tab = np.empty((D, 4), dtype=np.int32)
        tab[:, 0] = s
        tab[:, 1] = np.minimum(s + 1, S - 1)
        tab[:, 2] = np.rint((np.float32(1) - f) * np.float32(2048))     # rint: half to even, in float32
        tab[:, 3] = np.rint(f * np.float32(2048))
        tab.setflags(write=False)
    _RESIZE_TABLES[key] = tab
    return tab


def _pictures(t, name):
    """(n, H, W, frame stride in bytes) of a uint8 device tensor [H,W,3] or [F,H,W,3] whose rows are contiguous."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() in (3, 4) and t.shape[-1] == 3):
        raise ValueError(f"resize_u8: {name} must be a uint8 device tensor [H,W,3] or [F,H,W,3], got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    H, W = int(t.shape[-3]), int(t.shape[-2])
    if H < 1 or W < 1 or (t.dim() == 4 and t.shape[0] < 1):
        raise ValueError(f"resize_u8: empty {name} {tuple(t.shape)}")
    if t.stride(-1) != 1 or t.stride(-2) != 3 or (H > 1 and t.stride(-3) != 3 * W):
        raise ValueError(f"resize_u8: the rows of {name} must be contiguous (strides {t.stride()})")
    if t.dim() == 3:
        return 1, H, W, 3 * H * W
    if t.shape[0] > 1 and t.stride(0) < 3 * H * W:
        raise ValueError(f"resize_u8: the frames of {name} overlap (strides {t.stride()})")
    return int(t.shape[0]), H, W, (int(t.stride(0)) if t.shape[0] > 1 else 3 * H * W)


def resize_u8(src, size, out=None):
    """uint8 RGB pictures [H,W,3] or [F,H,W,3] (a device tensor with contiguous rows: whole pictures, frames of a clip or
    a row slice of a larger frame) -> [h,w,3] / [F,h,w,3], size = (h, w) (vfml_resize_u8: stream-ordered, no
    synchronisation; the tap tables are uploaded the first time a pair of lengths is seen on a device).  `out`: a device
    tensor of the result's shape with contiguous rows - a frame inside a clip, say - filled and returned."""
    h, w = int(size[0]), int(size[1])
    n, H, W, sstride = _pictures(src, "src")
    if h < 1 or w < 1:
        raise ValueError(f"resize_u8: size {(h, w)}")
    shape = (h, w, 3) if src.dim() == 3 else (n, h, w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != shape or out.device != src.device:
        raise ValueError(f"resize_u8: out must be a uint8 tensor {shape} on {src.device}, got "
                         f"{tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    dstride = _pictures(out, "out")[3]
    xt = yt = None
    if (h, w) != (H, W) and not (H == 2 * h and W == 2 * w):
        xt = c_void_p(resize_tables(W, w, src.device).data_ptr())
        yt = c_void_p(resize_tables(H, h, src.device).data_ptr())
    _check(lib().vfml_resize_u8(c_void_p(src.data_ptr()), n, H, W, sstride, c_void_p(out.data_ptr()), h, w, dstride, xt, yt,
                                _stream()), "vfml_resize_u8")
    return out


SCENE_CELLS, SCENE_BINS = 16, 64        # a frame's scene-cut signature: uint32 [16 cells][64 luma bins]


def scene_distances(frames, prev_sig=None, out=None):
    """uint8 RGB frames [n,H,W,3] (or one [H,W,3]; a contiguous device tensor, frames of a clip included) -> (sig, dist):
    int32 device tensors [n,1024] and [n] holding the uint32 signatures and distances of vfml_scene_distances (DESIGN.md
    section 20) - read them as uint32 (`.cpu().numpy().view(numpy.uint32)`).  Stream-ordered, no synchronisation.
    prev_sig: the signature (int32 [1024], device) of the frame before frames[0]; None: dist[0] = 0.
    out: (sig, dist) tensors of those shapes to fill - rows of larger buffers, say - instead of fresh ones."""
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (3, 4)
            and frames.shape[-1] == 3 and frames.is_contiguous()):
        raise ValueError(f"scene_distances: frames must be a contiguous uint8 device tensor [n,H,W,3] or [H,W,3], got "
                         f"{getattr(frames, 'dtype', type(frames))} {tuple(getattr(frames, 'shape', ()))}")
    n = 1 if frames.dim() == 3 else int(frames.shape[0])
    H, W = int(frames.shape[-3]), int(frames.shape[-2])
    words = SCENE_CELLS * SCENE_BINS
    if out is None:
        sig = torch.empty((n, words), dtype=torch.int32, device=frames.device)
        dist = torch.empty((n,), dtype=torch.int32, device=frames.device)
    else:
        sig, dist = out
        for t, shape, name in ((sig, (n, words), "sig"), (dist, (n,), "dist")):
            if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.device == frames.device and tuple(t.shape) == shape
                    and t.is_contiguous()):
                raise ValueError(f"scene_distances: out {name} must be a contiguous int32 tensor {shape} on {frames.device}")
    if prev_sig is not None and not (torch.is_tensor(prev_sig) and prev_sig.dtype == torch.int32 and prev_sig.numel() == words
                                     and prev_sig.device == frames.device and prev_sig.is_contiguous()):
        raise ValueError(f"scene_distances: prev_sig must be a contiguous int32 tensor of {words} counts on {frames.device}")
    _check(lib().vfml_scene_distances(c_void_p(frames.data_ptr()), n, H, W,
                                      None if prev_sig is None else c_void_p(prev_sig.data_ptr()), c_void_p(sig.data_ptr()),
                                      c_void_p(dist.data_ptr()), _stream()), "vfml_scene_distances")
    return sig, dist


_JPEG_WS = {}
_JPEG_QT = {}


JPEG_ENCODE_SAMPLINGS = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}      # VFML_JPEG_* of include/vfml.h that the encoder builds


def _jpeg_encode_sampling(sampling):
    code = JPEG_ENCODE_SAMPLINGS.get(sampling)
    if code is None:
        raise ValueError(f"jpeg_encode: sampling {sampling!r}; {', '.join(JPEG_ENCODE_SAMPLINGS)} are built")
    return code


def jpeg_header(h, w, quality=95, sampling="4:2:0"):
    """The bytes in front of the scan that jpeg_encode writes (storage/jpeg_tables.py jpeg_header)."""
    from storage import jpeg_tables
    return jpeg_tables.jpeg_header(h, w, quality, sampling)


def jpeg_file(header, scan_bytes):
    """header + scan + EOI: a complete JPEG file."""
    from storage import jpeg_tables
    return jpeg_tables.jpeg_file(header, scan_bytes)


def jpeg_scan_capacity(h, w, sampling="4:2:0"):
    """Bytes that hold the scan of any h x w picture (vfml_jpeg_sampled_scan_capacity)."""
    return int(lib().vfml_jpeg_sampled_scan_capacity(int(h), int(w), _jpeg_encode_sampling(sampling)))


def jpeg_encode(rgb, quality=95, out=None, sampling="4:2:0"):
    """RGB picture, uint8 device tensor [H,W,3] whose rows are contiguous (a row slice of a larger or wider buffer
    included: the row stride is the tensor's) -> (scan, length): the entropy-coded data of its baseline JPEG (DESIGN.md
    section 12) in a uint8 device tensor and its byte count in a uint32-valued int32 device cell [1]
    (vfml_jpeg_encode_rgb_sampled: stream-ordered, no synchronisation).  sampling: '4:2:0', '4:2:2' or '4:4:4'.
    jpeg_header(H, W, quality, sampling) + the first `length` bytes of the scan + EOI is the file (jpeg_file); jpeg_scan
    reads them back and checks the length.
    out: a contiguous uint8 device tensor that receives the scan - its size is the capacity, nothing is written past
    it; None: one of the worst-case size is allocated.  The workspace and the quantisation tables are kept per device,
    picture size and sampling / quality and stream."""
    from storage import jpeg_tables
    samp = _jpeg_encode_sampling(sampling)
    if not (torch.is_tensor(rgb) and rgb.is_cuda and rgb.dtype == torch.uint8 and rgb.dim() == 3 and rgb.shape[2] == 3
            and rgb.shape[0] >= 1 and rgb.shape[1] >= 1 and rgb.stride(2) == 1 and rgb.stride(1) == 3
            and (rgb.shape[0] == 1 or rgb.stride(0) >= 3 * rgb.shape[1])):
        raise ValueError(f"jpeg_encode: a uint8 device picture [H,W,3] with contiguous rows expected, got "
                         f"{getattr(rgb, 'dtype', type(rgb))} {tuple(getattr(rgb, 'shape', ()))}")
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    stride = int(rgb.stride(0)) if h > 1 else 3 * w
    L = lib()
    need = int(L.vfml_jpeg_sampled_workspace_bytes(h, w, samp))
    if need == 0:
        raise ValueError(f"jpeg_encode: picture {w}x{h} is too large for a JPEG")
    stream = torch.cuda.current_stream().cuda_stream
    key = (rgb.device.index, h, w, stream, samp)
    ws = _JPEG_WS.get(key)
    if ws is None:
        ws = _JPEG_WS[key] = torch.empty(need, dtype=torch.uint8, device=rgb.device)
    qkey = (rgb.device.index, int(quality))
    qt = _JPEG_QT.get(qkey)
    if qt is None:
        qt = _JPEG_QT[qkey] = torch.from_numpy(jpeg_tables.quant_tables(quality).copy()).to(rgb.device)
    if out is None:
        out = torch.empty(jpeg_scan_capacity(h, w, sampling), dtype=torch.uint8, device=rgb.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == rgb.device and out.dim() == 1
              and out.is_contiguous()):
        raise ValueError("jpeg_encode: out must be a contiguous one-dimensional uint8 tensor on the picture's device")
    length = torch.empty(1, dtype=torch.int32, device=rgb.device)
    _check(L.vfml_jpeg_encode_rgb_sampled(c_void_p(rgb.data_ptr()), h, w, stride, samp, c_void_p(qt.data_ptr()),
                                          c_void_p(ws.data_ptr()), c_void_p(out.data_ptr()), out.numel(),
                                          c_void_p(length.data_ptr()), _stream()),
           "vfml_jpeg_encode_rgb_sampled")
    return out, length


def jpeg_scan(scan, length):
    """The scan bytes of a jpeg_encode result on the host (synchronises).  A scan that did not fit its tensor raises and
    names the size it needs."""
    n = int(length.item()) & 0xFFFFFFFF
    if n > scan.numel():
        raise RuntimeError(f"jpeg_encode: the scan needs {n} bytes, its buffer holds {scan.numel()}")
    return scan[:n].cpu().numpy().tobytes()


_JPEG_DEC_WS = {}
_JPEG_DEC_TABLES = {}
JPEG_DECODE_ERRORS = ((1, "the scan does not hold the header's number of restart intervals"),
                      (2, "restart markers out of sequence"), (4, "a code that is in no Huffman table"),
                      (8, "a coefficient index past 63"), (16, "an interval's bits ran out before its MCUs did"))


def _jpeg_decode_tables(info, device):
    """The quantisation and Huffman lookup tables of `info` on the device ([192] uint8, [392] int32), kept per device
    and table content: the frames of an MJPG stream share theirs, and a frame whose tables are known costs one
    dictionary lookup.  Tables seen for the first time are built (jpeg_parse.decode_tables) and uploaded from pageable
    memory, which waits for the copy: a stream whose every frame brings Huffman tables of its own (optimize=True) pays
    that once per frame.  The oldest of 32 entries makes room for a new one."""
    from storage import jpeg_parse
    key = (device.index, info.qtables.tobytes(), info.huffman, info.selectors)
    got = _JPEG_DEC_TABLES.get(key)
    if got is None:
        if len(_JPEG_DEC_TABLES) >= 32:
            del _JPEG_DEC_TABLES[next(iter(_JPEG_DEC_TABLES))]
        qt, tables = jpeg_parse.decode_tables(info)
        got = _JPEG_DEC_TABLES[key] = (torch.from_numpy(qt.reshape(-1).copy()).to(device),
                                       torch.from_numpy(tables.copy()).to(device))
    return got


JPEG_SUBSEQ_BYTES = 128     # bytes of the scan per lane of the 'sync' plan (not measured yet)


def jpeg_subseq_bytes(scan_bytes):
    """The subsequence size jpeg_decode(plan='sync', subseq_bytes=None) uses for a scan: JPEG_SUBSEQ_BYTES, doubled (up
    to 1024) while the scan would hold more than 65536 subsequences - the chain kernel walks the groups of 256 in
    series on one workgroup, so their number is kept to a few hundred wherever the size allows it."""
    sub = JPEG_SUBSEQ_BYTES
    while sub < 1024 and int(scan_bytes) > sub << 16:
        sub <<= 1
    return sub


def jpeg_decode_plan(info):
    """'interval' or 'sync': the kernel jpeg_decode(plan=None) picks for a parsed file (storage.jpeg_parse.decode_plan)."""
    from storage import jpeg_parse
    return jpeg_parse.decode_plan(info)


def jpeg_decode(data, rows=None, out=None, device=None, info=None, plan=None, subseq_bytes=None):
    """A baseline JPEG file -> (rgb, status): the picture, uint8 device tensor [H,W,3], decoded on the device byte for
    byte as libjpeg (Pillow) decodes it (vfml_jpeg_decode_rgb_sampled; 4:2:0, 4:2:2, 4:4:4 or grey
    by info.sampling, a grey picture as R = G = B: stream-ordered, no
    synchronisation once the file's tables are on the device, see _jpeg_decode_tables), and the int32 device cell [1] that holds 0 or the error bits of a damaged scan
    (jpeg_decode_check reads it).
    data: the file's bytes - uploaded here - or a uint8 tensor that holds them, pinned (uploaded asynchronously; the
    caller keeps it unchanged until the copy has run) or on the device, together with info = storage.jpeg_parse.parse
    of them; a file the decoder does not take raises jpeg_parse.JpegUnsupported before anything is launched.
    rows=(y0, y1): rows y0 <= y < y1 of the picture alone ([y1-y0,W,3]); with one or more whole MCU rows per restart
    interval the other intervals are not read.  out: a uint8 device tensor [rows,W,3] with contiguous pixels and a row
    stride of at least 3 W (a row slice of a larger buffer) that receives the picture.  The workspace is kept per
    device, picture size, plan and stream, and holds the largest sampling it has met.
    plan: 'interval' (vfml_jpeg_decode_rgb: a wave per restart interval), 'sync' (vfml_jpeg_decode_rgb_sync, section
    13.1: a lane per subseq_bytes of the scan, whatever the restart interval) or None: jpeg_decode_plan(info).  Both
    give the same bytes.  subseq_bytes: a power of two 16..1024, None: jpeg_subseq_bytes of the scan's size rounded up
    to a power of two, as the workspace is (128 up to 8 MiB)."""
    if plan not in (None, "interval", "sync"):
        raise ValueError(f"jpeg_decode: plan {plan!r}; 'interval', 'sync' or None")
    if subseq_bytes is not None and plan == "interval":
        raise ValueError("jpeg_decode: subseq_bytes belongs to plan='sync'")
    from storage import jpeg_parse
    if torch.is_tensor(data):
        if info is None:
            raise ValueError("jpeg_decode: a tensor of file bytes needs info=storage.jpeg_parse.parse(...) of them")
        if not (data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()):
            raise ValueError("jpeg_decode: the file bytes must be a contiguous one-dimensional uint8 tensor")
        if data.is_cuda:
            device = data.device
        elif not data.is_pinned():
            raise ValueError("jpeg_decode: a host tensor of file bytes must be pinned")
    else:
        if info is None:
            info = jpeg_parse.parse(data, jpeg_parse.DEVICE_SAMPLINGS)
        data = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"jpeg_decode: device {device} is no GPU")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    s0, s1 = info.scan
    if not 0 <= s0 <= s1 <= data.numel():
        raise ValueError(f"jpeg_decode: scan range {info.scan} outside the {data.numel()} bytes given")
    h, w = info.h, info.w
    y0, y1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= y0 < y1 <= h:
        raise ValueError(f"jpeg_decode: rows {rows!r} of a picture of {h}")
    if out is None:
        out = torch.empty((y1 - y0, w, 3), dtype=torch.uint8, device=device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == device and out.dtype == torch.uint8
              and tuple(out.shape) == (y1 - y0, w, 3) and out.stride(2) == 1 and out.stride(1) == 3
              and (out.shape[0] == 1 or out.stride(0) >= 3 * w)):
        raise ValueError(f"jpeg_decode: out must be a uint8 tensor [{y1 - y0},{w},3] on {device} with contiguous rows")
    stride = int(out.stride(0)) if y1 - y0 > 1 else 3 * w
    L = lib()
    scan = data[s0:s1].to(device, non_blocking=True)
    # the workspace grows with the scan in powers of two, so the frames of a stream share one
    cap = 1 << max(12, int(s1 - s0 - 1).bit_length()) if s1 > s0 else 4096
    if plan is None:
        plan = jpeg_parse.decode_plan(info)
    sync = plan == "sync"
    sub = jpeg_subseq_bytes(cap) if subseq_bytes is None else int(subseq_bytes)
    if sync and (sub < 16 or sub > 1024 or sub & (sub - 1)):
        raise ValueError(f"jpeg_decode: subseq_bytes {sub}; a power of two 16..1024")
    samp = jpeg_parse.SAMPLING_CODE[info.sampling]
    need = int(L.vfml_jpeg_decode_sync_sampled_workspace_bytes(h, w, samp, cap, sub) if sync else
               L.vfml_jpeg_decode_sampled_workspace_bytes(h, w, samp, cap))
    if need == 0:
        raise ValueError(f"jpeg_decode: picture {w}x{h} with a scan of {s1 - s0} bytes is too large")
    key = (device.index, h, w, torch.cuda.current_stream(device).cuda_stream) + ((sub,) if sync else ())
    ws = _JPEG_DEC_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _JPEG_DEC_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    qt, tables = _jpeg_decode_tables(info, device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    if sync:
        with torch.cuda.device(device):
            _check(L.vfml_jpeg_decode_rgb_sync_sampled(
                c_void_p(scan.data_ptr()) if s1 > s0 else c_void_p(ws.data_ptr()), s1 - s0, h, w, samp,
                int(info.restart_interval), c_void_p(qt.data_ptr()), c_void_p(tables.data_ptr()), y0, y1, sub,
                c_void_p(ws.data_ptr()), c_void_p(out.data_ptr()), stride, c_void_p(status.data_ptr()), _stream()),
                "vfml_jpeg_decode_rgb_sync_sampled")
        return out, status
    with torch.cuda.device(device):
        _check(L.vfml_jpeg_decode_rgb_sampled(
            c_void_p(scan.data_ptr()) if s1 > s0 else c_void_p(ws.data_ptr()), s1 - s0, h, w, samp,
            int(info.restart_interval), c_void_p(qt.data_ptr()), c_void_p(tables.data_ptr()), y0, y1,
            c_void_p(ws.data_ptr()), c_void_p(out.data_ptr()), stride, c_void_p(status.data_ptr()), _stream()),
            "vfml_jpeg_decode_rgb_sampled")
    return out, status


def jpeg_decode_check(status):
    """Reads a jpeg_decode status cell (synchronises; a device cell or its pinned copy); a damaged scan raises
    RuntimeError and names what was found."""
    v = int(status.item()) if torch.is_tensor(status) else int(status)
    if v:
        found = [text for bit, text in JPEG_DECODE_ERRORS if v & bit] or [f"status {v}"]
        raise RuntimeError("jpeg_decode: damaged scan: " + "; ".join(found))


def convex_upsample(coords1, coords_off, ch, mask, mask_off, ld_mask, h, w, out, out_off=0):
    _check(lib().vfml_convex_upsample(_ptr(_dev(coords1), coords_off), ch, _ptr(_dev(mask), mask_off), ld_mask, h, w,
                                      _ptr(_dev(out), out_off), _stream()), "vfml_convex_upsample")


CORRECT_RECORD = 16


def flow_correct(frame1, frame2, flow, lod, twiddles, good_threshold, fine_threshold, region_radius=25,
                 template_radius=5.5, search_radius=25, records=None):
    """One frame's batch correction (vfml_flow_correct): uint8 frames [H,W,3], float32 flow [H,W,2] and LOD [lh,lw,2],
    float64 twiddles [2,50] (device tensors) -> (corrected flow [H,W,2], device int32 counts [2]: bad pixels before /
    after).  `records`: None, or a device float64 tensor [cap, 16] that receives the first cap bad pixels' records."""
    f1, f2 = _dev(frame1.contiguous(), torch.uint8), _dev(frame2.contiguous(), torch.uint8)
    fl, ld = _dev(flow.contiguous()), _dev(lod.contiguous())
    tw = _dev(twiddles.contiguous(), torch.float64)
    h, w = f1.shape[:2]
    if tuple(f1.shape) != (h, w, 3) or f2.shape != f1.shape:
        raise ValueError(f"flow_correct: frames {tuple(f1.shape)} {tuple(f2.shape)}")
    if tuple(fl.shape) != (h, w, 2):
        raise ValueError(f"flow_correct: flow {tuple(fl.shape)} is not at the frame's resolution {h}x{w}")
    if ld.dim() != 3 or ld.shape[2] != 2 or tuple(tw.shape) != (2, 50):
        raise ValueError(f"flow_correct: LOD {tuple(ld.shape)}, twiddles {tuple(tw.shape)}")
    cap = 0
    if records is not None:
        records = _dev(records, torch.float64)
        if records.dim() != 2 or records.shape[1] != CORRECT_RECORD or not records.is_contiguous():
            raise ValueError(f"flow_correct: records {tuple(records.shape)}, want contiguous [cap, {CORRECT_RECORD}]")
        cap = records.shape[0]
    L = lib()
    nbytes = L.vfml_flow_correct_workspace_bytes(h, w)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=f1.device)
    out = torch.empty_like(fl)
    counts = torch.zeros(2, dtype=torch.int32, device=f1.device)
    _check(L.vfml_flow_correct(c_void_p(f1.data_ptr()), c_void_p(f2.data_ptr()), _ptr(fl), _ptr(ld), ld.shape[0],
                               ld.shape[1], h, w, c_void_p(tw.data_ptr()), float(good_threshold), float(fine_threshold),
                               float(region_radius), float(template_radius), float(search_radius), _ptr(out),
                               c_void_p(counts.data_ptr()), None if records is None else c_void_p(records.data_ptr()),
                               cap, c_void_p(ws.data_ptr()), nbytes, _stream()), "vfml_flow_correct")
    return out, counts


# -- deflate / inflate of flow-cache members ---------------------------------------------------
_DEFLATE_WS = {}
_INFLATE_WS = {}
INFLATE_ERRORS = ((1, "bits that are no code of the block's table"), (2, "a length / distance symbol"),
                  (4, "a chunk that decodes to the wrong length"), (8, "a chunk's bits ran out"),
                  (16, "a bad stored-block length"), (32, "chunk offsets outside the data, or an oversized chunk"))


def deflate_capacity(raw_bytes, chunk_bytes=32768):
    """Bytes that hold the deflate stream of any raw_bytes bytes (vfml_deflate_capacity); 0: not coded on the device."""
    return int(lib().vfml_deflate_capacity(int(raw_bytes), int(chunk_bytes)))


def deflate_chunks(raw_bytes, chunk_bytes=32768):
    return (int(raw_bytes) + int(chunk_bytes) - 1) // int(chunk_bytes)


def _as_bytes(t, who):
    if not (torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.numel() >= 1):
        raise ValueError(f"{who}: a non-empty contiguous device tensor expected")
    return t.numel() * t.element_size()


def deflate(tensor, chunk_bytes=32768, crc_init=0, out=None):
    """The bytes of a contiguous device tensor (a slice of a larger buffer included, any alignment) -> (stream, cells):
    their literals-only deflate stream in chunks of chunk_bytes (vfml_deflate_huffman:
    stream-ordered, no synchronisation) in a uint8 device tensor, and an int32 device tensor of uint32 values
    [stream length, CRC-32 continued from crc_init, offset of chunk 0, 1, ...].  deflate_stream reads them back.
    out: a contiguous uint8 device tensor that receives the stream - its size is the capacity, nothing is written past
    it; None: one of the worst-case size is allocated.  The workspace is kept per device, size and stream."""
    nbytes = _as_bytes(tensor, "deflate")
    L = lib()
    cap = int(L.vfml_deflate_capacity(nbytes, int(chunk_bytes)))
    if cap == 0:
        raise ValueError(f"deflate: {nbytes} bytes in chunks of {chunk_bytes} are not coded on the device (chunk_bytes a power "
                         f"of two 1024..32768, below 2 GiB, at most 16000 chunks)")
    stream = torch.cuda.current_stream().cuda_stream
    key = (tensor.device.index, nbytes, int(chunk_bytes), stream)
    ws = _DEFLATE_WS.get(key)
    if ws is None:
        ws = _DEFLATE_WS[key] = torch.empty(int(L.vfml_deflate_workspace_bytes(nbytes, int(chunk_bytes))), dtype=torch.uint8,
                                            device=tensor.device)
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=tensor.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == tensor.device and out.dim() == 1
              and out.is_contiguous()):
        raise ValueError("deflate: out must be a contiguous one-dimensional uint8 tensor on the input's device")
    n = deflate_chunks(nbytes, chunk_bytes)
    cells = torch.empty(2 + n, dtype=torch.int32, device=tensor.device)
    base = cells.data_ptr()
    _check(L.vfml_deflate_huffman(c_void_p(tensor.data_ptr()), nbytes, int(chunk_bytes), int(crc_init) & 0xFFFFFFFF,
                                  c_void_p(ws.data_ptr()), c_void_p(out.data_ptr()), out.numel(), c_void_p(base + 8),
                                  c_void_p(base), c_void_p(base + 4), _stream()), "vfml_deflate_huffman")
    return out, cells


def deflate_stream(stream, cells):
    """(stream bytes, crc, [chunk offsets]) of a deflate result on the host (synchronises).  A stream that did not fit
    its tensor raises and names the size it needs."""
    host = [int(v) & 0xFFFFFFFF for v in cells.cpu().tolist()]
    if host[0] > stream.numel():
        raise RuntimeError(f"deflate: the stream needs {host[0]} bytes, its buffer holds {stream.numel()}")
    return stream[:host[0]].cpu().numpy().tobytes(), host[1], host[2:]


def inflate(data, offsets, chunk_bytes, raw_bytes, crc_init=0, out=None):
    """A chunked deflate stream -> (raw, cells): data, a contiguous one-dimensional uint8 device tensor (a slice
    included), whose chunk i starts at offsets[i] (a sequence, or an int32 device tensor) and decodes to chunk_bytes raw
    bytes (the last one to the rest of raw_bytes); raw: uint8 device tensor [raw_bytes] (out, when given), cells: int32
    device tensor [CRC-32 continued from crc_init, status] (vfml_inflate_chunks: stream-ordered, no synchronisation
    once the offsets are on the device).  inflate_check reads the cells."""
    if not (torch.is_tensor(data) and data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()):
        raise ValueError("inflate: data must be a contiguous one-dimensional uint8 device tensor")
    L = lib()
    raw_bytes, chunk_bytes = int(raw_bytes), int(chunk_bytes)
    need = int(L.vfml_inflate_workspace_bytes(raw_bytes, chunk_bytes))
    if need == 0:
        raise ValueError(f"inflate: {raw_bytes} bytes in chunks of {chunk_bytes} are not decoded on the device")
    n = deflate_chunks(raw_bytes, chunk_bytes)
    if not torch.is_tensor(offsets):
        offsets = torch.tensor([int(o) - (1 << 32) if int(o) >= (1 << 31) else int(o) for o in offsets], dtype=torch.int32).to(data.device)
    if not (offsets.is_cuda and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.numel() == n):
        raise ValueError(f"inflate: {n} chunk offsets expected (int32, on the device)")
    stream = torch.cuda.current_stream().cuda_stream
    key = (data.device.index, raw_bytes, chunk_bytes, stream)
    ws = _INFLATE_WS.get(key)
    if ws is None:
        ws = _INFLATE_WS[key] = torch.empty(need, dtype=torch.uint8, device=data.device)
    if out is None:
        out = torch.empty(raw_bytes, dtype=torch.uint8, device=data.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == data.device and out.dim() == 1
              and out.is_contiguous() and out.numel() == raw_bytes):
        raise ValueError(f"inflate: out must be a contiguous uint8 tensor [{raw_bytes}] on the data's device")
    cells = torch.empty(2, dtype=torch.int32, device=data.device)
    # (an empty tensor's data_ptr is 0: the library wants a pointer, and reads nothing through it when data_bytes is 0)
    dptr = data.data_ptr() if data.numel() else ws.data_ptr()
    _check(L.vfml_inflate_chunks(c_void_p(dptr), data.numel(), c_void_p(offsets.data_ptr()), n, chunk_bytes, raw_bytes,
                                 int(crc_init) & 0xFFFFFFFF, c_void_p(ws.data_ptr()), c_void_p(out.data_ptr()),
                                 c_void_p(cells.data_ptr()), c_void_p(cells.data_ptr() + 4), _stream()), "vfml_inflate_chunks")
    return out, cells


def inflate_check(cells, crc=None):
    """Reads an inflate result's cells (synchronises): a damaged stream raises, so does a CRC other than `crc`; -> crc."""
    got, status = (int(v) & 0xFFFFFFFF for v in cells.cpu().tolist())
    if status:
        raise RuntimeError("inflate: damaged stream: " + "; ".join(text for bit, text in INFLATE_ERRORS if status & bit))
    if crc is not None and got != (int(crc) & 0xFFFFFFFF):
        raise RuntimeError(f"inflate: CRC-32 {got:08x}, the archive says {int(crc) & 0xFFFFFFFF:08x}")
    return got
