"""ctypes binding of ``libartalk_hip.so`` (C ABI declared in ``include/artalk_hip.h``).

The library is the product path: if it is missing this module raises, there is no CPU fallback.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make -C artalk_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

from .config import ARTalkConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARTALK_LIB") or os.path.join(_HERE, "libartalk_hip.so")     # ARTALK_LIB: A/B runs of two builds on one box

OK, EINVAL, EKEY, EMISSING, EHIP, ESTATE, ECAPACITY, EBUSY = 0, -1, -2, -3, -4, -5, -6, -7
DTYPE_F32, DTYPE_I64 = 0, 1
FRAMES_RGB24, FRAMES_YUV420P = 1, 2      # ARTALK_FRAMES_* of include/artalk_hip.h
JPEG_420, JPEG_444, JPEG_HEADER_BYTES = 1, 2, 629      # ARTALK_JPEG_* of include/artalk_hip.h; the header every stream starts with
PCM_S16, PCM_F32, PCM_MAX_TAPS, PCM_MAX_CHANNELS = 1, 2, 1024, 8      # ARTALK_PCM_* of include/artalk_hip.h

# every symbol include/artalk_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "artalk_create", "artalk_destroy", "artalk_last_error", "artalk_set_tensor", "artalk_finalize_weights",
    "artalk_reserve", "artalk_workspace_bytes", "artalk_weight_bytes", "artalk_infer", "artalk_get_status", "artalk_poll_status", "artalk_last_ticket", "artalk_get_status_of", "artalk_style_encode", "artalk_stream_begin", "artalk_stream_chunk", "artalk_stream_end", "artalk_savgol", "artalk_flame_create", "artalk_flame_verts", "artalk_flame_destroy", "artalk_flame_last_error",
    "artalk_set_profiling", "artalk_get_profile", "artalk_get_kernel_sums", "artalk_set_graphs", "artalk_graph_count", "artalk_set_cu_mask", "artalk_set_audit", "artalk_get_audit", "artalk_calibrate", "artalk_reset_scales", "artalk_get_scales", "artalk_scale_sites", "artalk_get_site_scales", "artalk_set_site_scales", "artalk_set_tap", "artalk_tap_layout", "artalk_set_precision",
    "artalk_op_gemm", "artalk_op_gemm_ex", "artalk_op_gemm_bf16", "artalk_op_gemm_f16s", "artalk_op_pack_split", "artalk_op_gemm_f16s_packed", "artalk_op_release_scratch", "artalk_op_gemm_p8_plan", "artalk_op_create_masked_stream", "artalk_op_destroy_stream", "artalk_op_mfma_f32_peak", "artalk_op_layernorm", "artalk_op_attention", "artalk_op_w2v_front", "artalk_op_resample_mean", "artalk_op_pool_silu",
    "artalk_op_bsq_history",
    "artalk_sessions_reserve", "artalk_session_open", "artalk_session_step", "artalk_session_close", "artalk_session_count",
    "artalk_session_smooth", "artalk_op_savgol_stream", "artalk_op_session_smooth_check",
    "artalk_op_pack_split_ex", "artalk_op_layernorm_ex", "artalk_op_gemm_f16s_packed_ex", "artalk_op_gemm_f16s_ex", "artalk_op_attention_ex", "artalk_op_w2v_front_ex", "artalk_op_pool_silu_ex", "artalk_op_posconv_p8_ex",
    "artalk_op_bsq_history_ex", "artalk_op_ar_bits_next", "artalk_op_vq_embed", "artalk_op_ar_begin", "artalk_op_dec_input", "artalk_op_dec_finish", "artalk_op_enc_input_zero", "artalk_op_style_input", "artalk_op_add_row", "artalk_op_style_finish", "artalk_op_broadcast16", "artalk_op_session_gather", "artalk_op_session_scatter", "artalk_op_absmax",
    "artalk_op_gemm_rows", "artalk_op_layernorm_rows", "artalk_op_attention_rows", "artalk_op_gemm_rows_layout", "artalk_op_rows_dry_run",
    "artalk_op_w2v_front_rows", "artalk_op_pool_silu_rows", "artalk_op_posconv_rows",
    "artalk_op_attention_plan", "artalk_op_attention_rows_cus", "artalk_op_gemm_blocked",
    "artalk_infer_samples", "artalk_set_tail_skip", "artalk_conv_tail_geometry", "artalk_conv_tail_class",
    "artalk_render_create", "artalk_render_mesh", "artalk_render_set_slab", "artalk_render_destroy", "artalk_render_last_error",
    "artalk_splat_create", "artalk_splat_render", "artalk_splat_set_timing", "artalk_splat_get_timing", "artalk_splat_destroy",
    "artalk_splat_last_error",
    "artalk_styleunet_create", "artalk_styleunet_set_tensor", "artalk_styleunet_finalize", "artalk_styleunet_forward",
    "artalk_styleunet_set_slab", "artalk_styleunet_set_timing", "artalk_styleunet_get_timing", "artalk_styleunet_destroy",
    "artalk_styleunet_last_error", "artalk_op_conv2d", "artalk_op_resample2",
    "artalk_styleunet_set_precision", "artalk_styleunet_get_precision", "artalk_op_conv2d_ex", "artalk_styleunet_get_launch_timing",
    "artalk_op_conv2d_plan",
    "artalk_op_su_linear", "artalk_op_su_normstyle", "artalk_op_su_demod", "artalk_op_su_add", "artalk_op_su_to_nhwc", "artalk_op_su_to_nchw",
    "artalk_flame_dims", "artalk_styleunet_dims",
    "artalk_gaga_create", "artalk_gaga_set_avatar", "artalk_gaga_set_forehead", "artalk_gaga_set_watermark", "artalk_gaga_reset_state",
    "artalk_gaga_set_slab", "artalk_gaga_render", "artalk_gaga_set_timing", "artalk_gaga_get_timing", "artalk_gaga_destroy",
    "artalk_gaga_last_error", "artalk_gaga_cameras", "artalk_op_gaga_flame_inputs", "artalk_op_gaga_forehead", "artalk_op_gaga_means",
    "artalk_op_gaga_finish", "artalk_op_gaga_check",
    "artalk_frames_bytes", "artalk_frames_pack", "artalk_frames_last_error", "artalk_op_frames_check", "artalk_op_gaga_finish_pack",
    "artalk_gaga_render_u8",
    "artalk_splat_render_sets", "artalk_gaga_pool_reserve", "artalk_gaga_pool_set", "artalk_gaga_pool_clear", "artalk_gaga_stream_open",
    "artalk_gaga_stream_close", "artalk_gaga_stream_reset", "artalk_gaga_render_streams", "artalk_op_gaga_flame_inputs_sets",
    "artalk_op_gaga_forehead_streams", "artalk_op_gaga_means_sets", "artalk_op_gaga_streams_check", "artalk_gaga_streams_slab",
    "artalk_gsgen_create", "artalk_gsgen_set_tensor", "artalk_gsgen_finalize", "artalk_gsgen_planes", "artalk_gsgen_generate",
    "artalk_gsgen_set_timing", "artalk_gsgen_get_timing", "artalk_gsgen_dims", "artalk_gsgen_destroy", "artalk_gsgen_last_error",
    "artalk_op_conv2d_relu", "artalk_op_gs_local_input", "artalk_op_gs_global_input", "artalk_op_gs_concat_dir",
    "artalk_op_gs_local_attr", "artalk_op_gs_global_attr",
    "artalk_dino_create", "artalk_dino_set_tensor", "artalk_dino_finalize", "artalk_dino_prepare_image", "artalk_dino_forward",
    "artalk_dino_read", "artalk_dino_set_timing", "artalk_dino_get_timing", "artalk_dino_dims", "artalk_dino_destroy", "artalk_dino_last_error",
    "artalk_op_dino_resize_aa", "artalk_op_dino_normalize", "artalk_op_dino_im2col", "artalk_op_dino_tokens", "artalk_op_dino_layernorm",
    "artalk_op_dino_strip", "artalk_op_dino_shuffle", "artalk_op_dino_gather_s2", "artalk_op_dino_concat", "artalk_op_dino_resize_ac",
    "artalk_op_dino_add_relu", "artalk_op_dino_output",
    "artalk_pcm_create", "artalk_pcm_destroy", "artalk_pcm_last_error", "artalk_pcm_set_rate", "artalk_pcm_open", "artalk_pcm_close",
    "artalk_pcm_push", "artalk_pcm_end", "artalk_pcm_available", "artalk_pcm_take", "artalk_op_pcm_plan", "artalk_op_pcm_desc_bytes",
    "artalk_op_pcm_push", "artalk_op_pcm_take",
    "artalk_jpeg_default_cap", "artalk_jpeg_bound", "artalk_jpeg_header", "artalk_jpeg_create", "artalk_jpeg_destroy", "artalk_jpeg_last_error",
    "artalk_jpeg_encode", "artalk_op_jpeg_check", "artalk_jpeg_set_timing", "artalk_jpeg_get_timing",
]

# ARTALK_ATTN_* of include/artalk_hip.h: the kernels of attention.hip, as artalk_op_attention_plan names them
(ATTN_F32_64, ATTN_F32_32, ATTN_SHORT, ATTN_F16, ATTN_F16_P8, ATTN_F16_WIDE, ATTN_F16_PP, ATTN_F16_WIDE_AR,
 ATTN_F16_WIDE_AR_P8) = range(9)
ATTN_KERNELS = {
    ATTN_F32_64: "attention_kernel<64>", ATTN_F32_32: "attention_kernel<32>", ATTN_SHORT: "attention_short_kernel",
    ATTN_F16: "attention_f16_kernel<1>", ATTN_F16_P8: "attention_f16_kernel<1,1>", ATTN_F16_WIDE: "attention_f16_wide_kernel",
    ATTN_F16_PP: "attention_f16_pp_kernel", ATTN_F16_WIDE_AR: "attention_f16_wide_ar_kernel<1>",
    ATTN_F16_WIDE_AR_P8: "attention_f16_wide_ar_kernel<1,1,7,128>",
}


class ArtalkConfigStruct(C.Structure):
    _fields_ = [
        ("ar_depth", C.c_int32), ("ar_heads", C.c_int32),
        ("vae_depth", C.c_int32), ("vae_heads", C.c_int32), ("vae_hidden", C.c_int32),
        ("code_dim", C.c_int32), ("motion_dim", C.c_int32),
        ("n_levels", C.c_int32), ("patch_nums", C.c_int32 * 8),
        ("w2v_layers", C.c_int32), ("w2v_hidden", C.c_int32), ("w2v_heads", C.c_int32), ("w2v_ffn", C.c_int32),
        ("w2v_n_conv", C.c_int32), ("w2v_conv_kernel", C.c_int32 * 8), ("w2v_conv_stride", C.c_int32 * 8),
        ("w2v_conv_dim", C.c_int32),
        ("w2v_pos_kernel", C.c_int32), ("w2v_pos_groups", C.c_int32),
        ("w2v_ln_eps", C.c_float),
        ("style_dim", C.c_int32), ("style_heads", C.c_int32), ("style_layers", C.c_int32), ("style_ffn", C.c_int32),
        ("style_len", C.c_int32),
    ]


ROWMAP_IDENTITY = (2 ** 31 - 1, 0, 0)      # row(m) = (m // rpb) * bstride + off + m % rpb; rpb = INT32_MAX: row(m) = m


class GemmRowsArgs(C.Structure):
    """artalk_op_gemm_rows_args of include/artalk_hip.h (field for field).  A new object holds identity maps, no forced configuration,
    no split and the default exponents; sizes (*_elems) count 4-byte elements from the pointer of their buffer."""
    _fields_ = [
        ("mode", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("act", C.c_int32),
        ("A", C.c_void_p), ("lda", C.c_int64), ("a_elems", C.c_int64), ("a_exp", C.c_int32),
        ("W", C.c_void_p), ("ldw", C.c_int64), ("w_elems", C.c_int64),
        ("bias", C.c_void_p), ("bias_elems", C.c_int64),
        ("C", C.c_void_p), ("ldc", C.c_int64), ("c_elems", C.c_int64), ("cmap", C.c_int32 * 3),
        ("gate", C.c_void_p), ("ldg", C.c_int64), ("gate_elems", C.c_int64), ("gmap", C.c_int32 * 3),
        ("R", C.c_void_p), ("ldr", C.c_int64), ("r_elems", C.c_int64),
        ("c_p8", C.c_int32), ("c_exp", C.c_int32),
        ("force_cfg", C.c_int32), ("splitk", C.c_int32),
        ("ngrp", C.c_int32), ("grpW", C.c_int64), ("grpB", C.c_int64), ("grpC", C.c_int64),
        ("status_dev", C.c_void_p),
        ("ln_Y", C.c_void_p), ("ln_ldy", C.c_int64), ("ln_y_elems", C.c_int64),
        ("ln_scale", C.c_void_p), ("ln_shift", C.c_void_p), ("ln_ldm", C.c_int64), ("ln_mod_elems", C.c_int64), ("ln_mmap", C.c_int32 * 3),
        ("ln_eps", C.c_float), ("ln_out_p8", C.c_int32), ("ln_p8_exp", C.c_int32),
        ("used_cfg", C.POINTER(C.c_int32)), ("used_splitk", C.POINTER(C.c_int32)), ("fused_ln", C.POINTER(C.c_int32)),
        ("cus", C.c_int32),
    ]

    def __init__(self, **kw):
        super().__init__()
        self.a_exp = self.c_exp = self.ln_p8_exp = 4
        self.force_cfg, self.splitk, self.ln_eps = -1, 1, 1e-6
        for name in ("cmap", "gmap", "ln_mmap"):
            setattr(self, name, (C.c_int32 * 3)(*ROWMAP_IDENTITY))
        for k, v in kw.items():
            setattr(self, k, (C.c_int32 * 3)(*v) if k in ("cmap", "gmap", "ln_mmap") else v)


class PcmDesc(C.Structure):
    """artalk_pcm_desc of include/artalk_hip.h (field for field): one packet of one stream for ``artalk_op_pcm_push``."""
    _fields_ = [
        ("taps", C.c_void_p), ("data", C.c_void_p), ("carry_in", C.c_void_p), ("carry_out", C.c_void_p), ("ring", C.c_void_p),
        ("orig", C.c_int32), ("nw", C.c_int32), ("width", C.c_int32), ("nch", C.c_int32), ("format", C.c_int32), ("frames", C.c_int32),
        ("lead", C.c_int32), ("carry_n", C.c_int32), ("carry_from", C.c_int32), ("carry_out_n", C.c_int32), ("carry_stride", C.c_int32),
        ("ring_cap", C.c_int32), ("ring_pos", C.c_int32), ("n_out", C.c_int32),
        ("tile_groups", C.c_int32), ("n_tiles", C.c_int32),
    ]


class PcmTakeDesc(C.Structure):
    """artalk_pcm_take_desc of include/artalk_hip.h: one row of ``artalk_op_pcm_take``."""
    _fields_ = [("ring", C.c_void_p), ("ring_cap", C.c_int32), ("read_pos", C.c_int32), ("n_valid", C.c_int32), ("reserved", C.c_int32)]


def config_struct(cfg: ARTalkConfig) -> ArtalkConfigStruct:
    w = cfg.w2v
    if w.get("feat_extract_norm", "layer") != "layer" or not w.get("do_stable_layer_norm", True) or not w.get("conv_bias", True):
        raise ValueError("only the XLS-R style wav2vec2 (layer-norm conv stack, stable layer norm, conv bias) is supported")
    if len(set(w["conv_dim"])) != 1:
        raise ValueError("conv_dim must be uniform")
    s = ArtalkConfigStruct()
    s.ar_depth, s.ar_heads = cfg.ar_depth, cfg.ar_heads
    s.vae_depth, s.vae_heads, s.vae_hidden = cfg.vae_depth, cfg.vae_heads, cfg.vae_hidden
    s.code_dim, s.motion_dim = cfg.code_dim, cfg.motion_dim
    s.n_levels = len(cfg.patch_nums)
    for i, p in enumerate(cfg.patch_nums):
        s.patch_nums[i] = p
    s.w2v_layers, s.w2v_hidden = w["num_hidden_layers"], w["hidden_size"]
    s.w2v_heads, s.w2v_ffn = w["num_attention_heads"], w["intermediate_size"]
    s.w2v_n_conv = len(w["conv_kernel"])
    for i, (k, st) in enumerate(zip(w["conv_kernel"], w["conv_stride"])):
        s.w2v_conv_kernel[i], s.w2v_conv_stride[i] = k, st
    s.w2v_conv_dim = w["conv_dim"][0]
    s.w2v_pos_kernel, s.w2v_pos_groups = w["num_conv_pos_embeddings"], w["num_conv_pos_embedding_groups"]
    s.w2v_ln_eps = w["layer_norm_eps"]
    s.style_dim, s.style_heads, s.style_layers = cfg.style_dim, cfg.style_heads, cfg.style_layers
    s.style_ffn, s.style_len = cfg.style_ffn, cfg.style_len
    return s


_lib = None


def lib() -> C.CDLL:
    """Load the shared library once and declare the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    L.artalk_create.argtypes = [i32, C.POINTER(ArtalkConfigStruct), C.POINTER(vp)]
    L.artalk_create.restype = i32
    L.artalk_destroy.argtypes = [vp]
    L.artalk_destroy.restype = None
    L.artalk_last_error.argtypes = [vp]
    L.artalk_last_error.restype = C.c_char_p
    L.artalk_set_tensor.argtypes = [vp, C.c_char_p, vp, i32, i32, C.POINTER(i64)]
    L.artalk_set_tensor.restype = i32
    L.artalk_finalize_weights.argtypes = [vp]
    L.artalk_finalize_weights.restype = i32
    L.artalk_reserve.argtypes = [vp, i32, i32]
    L.artalk_reserve.restype = i32
    L.artalk_workspace_bytes.argtypes = [vp]
    L.artalk_workspace_bytes.restype = i64
    L.artalk_weight_bytes.argtypes = [vp]
    L.artalk_weight_bytes.restype = i64
    L.artalk_infer.argtypes = [vp, vp, i64, C.POINTER(i64), i32, vp, vp, vp, i64, vp, vp, vp, vp]
    L.artalk_infer.restype = i32
    if hasattr(L, "artalk_infer_samples"):      # (an older build loaded through ARTALK_LIB for an A/B run runs every chunk whole)
        L.artalk_infer_samples.argtypes = [vp, vp, i64, C.POINTER(i64), C.POINTER(i64), i32, vp, vp, vp, i64, vp, vp, vp, vp]
        L.artalk_infer_samples.restype = i32
        L.artalk_set_tail_skip.argtypes = [vp, i32]
        L.artalk_set_tail_skip.restype = i32
        pi = C.POINTER(i32)
        L.artalk_conv_tail_geometry.argtypes = [i64, i32, i32, pi, pi, pi, pi, pi, pi]
        L.artalk_conv_tail_geometry.restype = i32
        L.artalk_conv_tail_class.argtypes = [i64, i32]
        L.artalk_conv_tail_class.restype = i64
    L.artalk_get_status.argtypes = [vp, C.POINTER(C.c_int), vp]
    L.artalk_get_status.restype = i32
    L.artalk_poll_status.argtypes = [vp, C.POINTER(C.c_int)]
    L.artalk_poll_status.restype = i32
    L.artalk_last_ticket.argtypes = [vp]
    L.artalk_last_ticket.restype = C.c_longlong
    L.artalk_get_status_of.argtypes = [vp, C.c_longlong, C.POINTER(C.c_int)]
    L.artalk_get_status_of.restype = i32
    L.artalk_style_encode.argtypes = [vp, vp, i32, vp, vp]
    L.artalk_style_encode.restype = i32
    L.artalk_stream_begin.argtypes = [vp, i32, vp, vp, vp]
    L.artalk_stream_begin.restype = i32
    L.artalk_stream_end.argtypes = [vp]
    L.artalk_stream_end.restype = i32
    L.artalk_stream_chunk.argtypes = [vp, vp, i64, vp, i64, vp]
    L.artalk_stream_chunk.restype = i32
    if hasattr(L, "artalk_session_open"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the session entry points)
        L.artalk_sessions_reserve.argtypes = [vp, i32]
        L.artalk_sessions_reserve.restype = i32
        L.artalk_session_open.argtypes = [vp, i32, vp, vp, C.POINTER(i64), vp]
        L.artalk_session_open.restype = i32
        L.artalk_session_step.argtypes = [vp, C.POINTER(i64), i32, vp, i64, vp, i64, vp, vp, vp]
        L.artalk_session_step.restype = i32
        L.artalk_session_close.argtypes = [vp, C.POINTER(i64), i32]
        L.artalk_session_close.restype = i32
        L.artalk_session_count.argtypes = [vp]
        L.artalk_session_count.restype = i32
    if hasattr(L, "artalk_session_smooth"):    # (an older build loaded through ARTALK_LIB lacks the streaming smoother)
        pi32, pu8 = C.POINTER(i32), C.POINTER(C.c_uint8)
        L.artalk_session_smooth.argtypes = [vp, C.POINTER(i64), i32, vp, i64, pi32, pu8, vp, i64, pi32, pi32, vp]
        L.artalk_session_smooth.restype = i32
        L.artalk_op_savgol_stream.argtypes = [vp, vp, i64, pi32, pi32, pu8, vp, i64, i32, vp]
        L.artalk_op_savgol_stream.restype = i32
        L.artalk_op_session_smooth_check.argtypes = [C.POINTER(i64), C.POINTER(i64), pu8, i32, C.POINTER(i64), i32, C.POINTER(i64), i32, i32, i64,
                                                     pi32, pu8, i64, pi32, pi32, C.c_char_p, i32]
        L.artalk_op_session_smooth_check.restype = i32
    L.artalk_flame_create.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, C.POINTER(vp)]
    L.artalk_flame_create.restype = i32
    L.artalk_flame_verts.argtypes = [vp, vp, vp, i32, vp, vp]
    L.artalk_flame_verts.restype = i32
    L.artalk_flame_destroy.argtypes = [vp]
    L.artalk_flame_destroy.restype = None
    L.artalk_flame_last_error.argtypes = [vp]
    L.artalk_flame_last_error.restype = C.c_char_p
    if hasattr(L, "artalk_render_create"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the mesh renderer)
        L.artalk_render_create.argtypes = [i32, i32, i32, vp, i32, f32, C.POINTER(vp)]
        L.artalk_render_create.restype = i32
        L.artalk_render_mesh.argtypes = [vp, vp, i32, vp, f32, vp, vp, vp, vp]
        L.artalk_render_mesh.restype = i32
        L.artalk_render_set_slab.argtypes = [vp, i32]
        L.artalk_render_set_slab.restype = i32
        L.artalk_render_destroy.argtypes = [vp]
        L.artalk_render_destroy.restype = None
        L.artalk_render_last_error.argtypes = [vp]
        L.artalk_render_last_error.restype = C.c_char_p
    if hasattr(L, "artalk_splat_create"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the splat rasteriser)
        L.artalk_splat_create.argtypes = [i32, C.POINTER(vp)]
        L.artalk_splat_create.restype = i32
        L.artalk_splat_render.argtypes = [vp, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, i32, f32, f32, f32,
                                          vp, vp, vp, vp]
        L.artalk_splat_render.restype = i32
        L.artalk_splat_set_timing.argtypes = [vp, i32]
        L.artalk_splat_set_timing.restype = i32
        L.artalk_splat_get_timing.argtypes = [vp, C.POINTER(C.c_double), i32, C.POINTER(C.c_longlong), C.POINTER(i32)]
        L.artalk_splat_get_timing.restype = i32
        L.artalk_splat_destroy.argtypes = [vp]
        L.artalk_splat_destroy.restype = None
        L.artalk_splat_last_error.argtypes = [vp]
        L.artalk_splat_last_error.restype = C.c_char_p
    if hasattr(L, "artalk_styleunet_create"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the StyleUNet upsampler)
        L.artalk_styleunet_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        L.artalk_styleunet_create.restype = i32
        L.artalk_styleunet_set_tensor.argtypes = [vp, C.c_char_p, vp, i32, C.POINTER(i64)]
        L.artalk_styleunet_set_tensor.restype = i32
        L.artalk_styleunet_finalize.argtypes = [vp]
        L.artalk_styleunet_finalize.restype = i32
        L.artalk_styleunet_forward.argtypes = [vp, vp, i32, C.POINTER(vp), C.POINTER(i64), i32, vp, vp]
        L.artalk_styleunet_forward.restype = i32
        L.artalk_styleunet_set_slab.argtypes = [vp, i32]
        L.artalk_styleunet_set_slab.restype = i32
        L.artalk_styleunet_set_timing.argtypes = [vp, i32]
        L.artalk_styleunet_set_timing.restype = i32
        L.artalk_styleunet_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.artalk_styleunet_get_timing.restype = i32
        L.artalk_styleunet_destroy.argtypes = [vp]
        L.artalk_styleunet_destroy.restype = None
        L.artalk_styleunet_last_error.argtypes = [vp]
        L.artalk_styleunet_last_error.restype = C.c_char_p
        L.artalk_op_conv2d.argtypes = [vp, i64, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, f32, vp, i64, vp, vp, i32, vp, vp, vp, vp]
        L.artalk_op_conv2d.restype = i32
        L.artalk_op_resample2.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
        L.artalk_op_resample2.restype = i32
    if hasattr(L, "artalk_styleunet_set_precision"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the bf16 modes)
        L.artalk_styleunet_set_precision.argtypes = [vp, i32]
        L.artalk_styleunet_set_precision.restype = i32
        L.artalk_styleunet_get_precision.argtypes = [vp]
        L.artalk_styleunet_get_precision.restype = i32
        L.artalk_styleunet_get_launch_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32), i32]
        L.artalk_styleunet_get_launch_timing.restype = i32
        L.artalk_op_conv2d_ex.argtypes = L.artalk_op_conv2d.argtypes[:-1] + [i32, vp]
        L.artalk_op_conv2d_ex.restype = i32
    if hasattr(L, "artalk_op_conv2d_plan"):      # (an older build loaded through ARTALK_LIB lacks the conv planner's entry point)
        L.artalk_op_conv2d_plan.argtypes = [C.c_uint64, i64, C.c_uint64, C.c_uint64, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int32), i32]
        L.artalk_op_conv2d_plan.restype = i32
    if hasattr(L, "artalk_op_su_linear"):      # (an older build loaded through ARTALK_LIB lacks the style path's entry points)
        for name, args in (("linear", [vp, vp, vp, vp, i32, i32, i32, i32, vp]), ("normstyle", [vp, vp, i32, i32, vp]),
                           ("demod", [vp, i64, vp, vp, i32, i32, i32, vp]), ("add", [vp, vp, vp, i64, vp]),
                           ("to_nhwc", [vp, vp, i32, i32, i64, vp]), ("to_nchw", [vp, vp, i32, i32, i64, i32, vp])):
            fn = getattr(L, "artalk_op_su_" + name)
            fn.argtypes, fn.restype = args, i32
    if hasattr(L, "artalk_gaga_create"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the GAGAvatar head)
        pi = C.POINTER(i32)
        L.artalk_flame_dims.argtypes = [vp, pi, pi, C.POINTER(f32)]
        L.artalk_flame_dims.restype = i32
        L.artalk_styleunet_dims.argtypes = [vp, pi, pi, pi, pi, pi]
        L.artalk_styleunet_dims.restype = i32
        L.artalk_gaga_create.argtypes = [i32, vp, vp, vp, i32, i32, i32, C.POINTER(vp)]
        L.artalk_gaga_create.restype = i32
        L.artalk_gaga_set_avatar.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.artalk_gaga_set_avatar.restype = i32
        L.artalk_gaga_set_forehead.argtypes = [vp, vp, i32]
        L.artalk_gaga_set_forehead.restype = i32
        L.artalk_gaga_set_watermark.argtypes = [vp, vp, i32, i32]
        L.artalk_gaga_set_watermark.restype = i32
        L.artalk_gaga_reset_state.argtypes = [vp]
        L.artalk_gaga_reset_state.restype = i32
        L.artalk_gaga_set_slab.argtypes = [vp, i32]
        L.artalk_gaga_set_slab.restype = i32
        L.artalk_gaga_render.argtypes = [vp, vp, i64, i32, C.POINTER(vp), C.POINTER(i64), i32, vp, vp]
        L.artalk_gaga_render.restype = i32
        L.artalk_gaga_set_timing.argtypes = [vp, i32]
        L.artalk_gaga_set_timing.restype = i32
        L.artalk_gaga_get_timing.argtypes = [vp, C.POINTER(C.c_double), i32]
        L.artalk_gaga_get_timing.restype = i32
        L.artalk_gaga_destroy.argtypes = [vp]
        L.artalk_gaga_destroy.restype = None
        L.artalk_gaga_last_error.argtypes = [vp]
        L.artalk_gaga_last_error.restype = C.c_char_p
        L.artalk_gaga_cameras.argtypes = [vp, i64, i32, vp, vp, vp, vp]
        L.artalk_gaga_cameras.restype = i32
        L.artalk_op_gaga_flame_inputs.argtypes = [vp, i64, vp, i32, i32, vp, vp, vp]
        L.artalk_op_gaga_flame_inputs.restype = i32
        L.artalk_op_gaga_forehead.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
        L.artalk_op_gaga_forehead.restype = i32
        L.artalk_op_gaga_means.argtypes = [vp, vp, vp, i32, i32, i32, vp]
        L.artalk_op_gaga_means.restype = i32
        L.artalk_op_gaga_finish.argtypes = [vp, i32, i32, vp, i32, i32, vp]
        L.artalk_op_gaga_finish.restype = i32
        L.artalk_op_gaga_check.argtypes = [i32, i32, i32, vp, i32, i32, i32, i32, i64, i32, i32, C.c_char_p, i32]
        L.artalk_op_gaga_check.restype = i32
    if hasattr(L, "artalk_frames_pack"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the 8-bit frames)
        L.artalk_frames_bytes.argtypes = [i32, i32, i32]
        L.artalk_frames_bytes.restype = i64
        L.artalk_frames_pack.argtypes = [vp, i32, i32, i32, i32, vp, vp]
        L.artalk_frames_pack.restype = i32
        L.artalk_frames_last_error.argtypes = []
        L.artalk_frames_last_error.restype = C.c_char_p
        L.artalk_op_frames_check.argtypes = [i32, i32, i32, i32, i32, i32, C.c_char_p, i32]
        L.artalk_op_frames_check.restype = i32
        L.artalk_op_gaga_finish_pack.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp, vp]
        L.artalk_op_gaga_finish_pack.restype = i32
        L.artalk_gaga_render_u8.argtypes = [vp, vp, i64, i32, C.POINTER(vp), C.POINTER(i64), i32, i32, vp, vp, vp]
        L.artalk_gaga_render_u8.restype = i32
    if hasattr(L, "artalk_gaga_render_streams"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the live streams)
        L.artalk_splat_render_sets.argtypes = L.artalk_splat_render.argtypes[:-1] + [vp, i32, i64, i64, i64, i64, i64, vp]
        L.artalk_splat_render_sets.restype = i32
        L.artalk_gaga_pool_reserve.argtypes = [vp, i32, i32]
        L.artalk_gaga_pool_reserve.restype = i32
        L.artalk_gaga_pool_set.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.artalk_gaga_pool_set.restype = i32
        L.artalk_gaga_pool_clear.argtypes = [vp, i32]
        L.artalk_gaga_pool_clear.restype = i32
        L.artalk_gaga_stream_open.argtypes = [vp, C.POINTER(i32)]
        L.artalk_gaga_stream_open.restype = i32
        L.artalk_gaga_stream_close.argtypes = [vp, i32]
        L.artalk_gaga_stream_close.restype = i32
        L.artalk_gaga_stream_reset.argtypes = [vp, i32]
        L.artalk_gaga_stream_reset.restype = i32
        L.artalk_gaga_render_streams.argtypes = [vp, vp, i64, i32, vp, vp, vp, C.POINTER(vp), C.POINTER(i64), i32, i32, vp, vp, vp, vp]
        L.artalk_gaga_render_streams.restype = i32
        L.artalk_gaga_streams_slab.argtypes = [vp]
        L.artalk_gaga_streams_slab.restype = i32
        L.artalk_op_gaga_flame_inputs_sets.argtypes = [vp, i64, vp, vp, vp, i32, i32, vp, vp, vp]
        L.artalk_op_gaga_flame_inputs_sets.restype = i32
        L.artalk_op_gaga_forehead_streams.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        L.artalk_op_gaga_forehead_streams.restype = i32
        L.artalk_op_gaga_means_sets.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
        L.artalk_op_gaga_means_sets.restype = i32
        L.artalk_op_gaga_streams_check.argtypes = [i32, i32, i32, i32, i64, vp, vp, vp, vp, i32, vp, i32, i32, i32, C.c_char_p, i32]
        L.artalk_op_gaga_streams_check.restype = i32
    if hasattr(L, "artalk_gsgen_create"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the Gaussian generators)
        L.artalk_gsgen_create.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
        L.artalk_gsgen_create.restype = i32
        L.artalk_gsgen_set_tensor.argtypes = [vp, C.c_char_p, vp, i32, C.POINTER(i64)]
        L.artalk_gsgen_set_tensor.restype = i32
        L.artalk_gsgen_finalize.argtypes = [vp]
        L.artalk_gsgen_finalize.restype = i32
        L.artalk_gsgen_planes.argtypes = [vp, i32, vp, vp, vp]
        L.artalk_gsgen_planes.restype = i32
        L.artalk_gsgen_generate.argtypes = [vp] * 10
        L.artalk_gsgen_generate.restype = i32
        L.artalk_gsgen_set_timing.argtypes = [vp, i32]
        L.artalk_gsgen_set_timing.restype = i32
        L.artalk_gsgen_get_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.artalk_gsgen_get_timing.restype = i32
        L.artalk_gsgen_dims.argtypes = [vp] + [C.POINTER(C.c_int32)] * 6
        L.artalk_gsgen_dims.restype = i32
        L.artalk_gsgen_destroy.argtypes = [vp]
        L.artalk_gsgen_destroy.restype = None
        L.artalk_gsgen_last_error.argtypes = [vp]
        L.artalk_gsgen_last_error.restype = C.c_char_p
        L.artalk_op_conv2d_relu.argtypes = [vp, i64, vp, vp, i32, i32, i32, i32, i32, i32, vp, i32, vp]
        L.artalk_op_conv2d_relu.restype = i32
        L.artalk_op_gs_local_input.argtypes = [vp, vp, vp, i32, i32, vp]
        L.artalk_op_gs_local_input.restype = i32
        L.artalk_op_gs_global_input.argtypes = [vp, vp, vp, i32, i32, i32, vp]
        L.artalk_op_gs_global_input.restype = i32
        L.artalk_op_gs_concat_dir.argtypes = [vp, vp, vp, i32, i32, vp]
        L.artalk_op_gs_concat_dir.restype = i32
        L.artalk_op_gs_local_attr.argtypes = [vp, vp, i32, i32, i64, vp, vp, vp, vp, vp, vp]
        L.artalk_op_gs_local_attr.restype = i32
        L.artalk_op_gs_global_attr.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.artalk_op_gs_global_attr.restype = i32
    if hasattr(L, "artalk_dino_create"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks DINOBase)
        for name, args, res in (
                ("dino_create", [i32, i32, i32, i32, i32, i32, C.POINTER(vp)], i32),
                ("dino_set_tensor", [vp, C.c_char_p, vp, i32, C.POINTER(i64)], i32),
                ("dino_finalize", [vp], i32),
                ("dino_prepare_image", [vp, vp, i32, i32, vp, vp], i32),
                ("dino_forward", [vp, vp, i32, i32, vp, vp, vp], i32),
                ("dino_read", [vp, C.c_char_p, vp, i64, vp], i32),
                ("dino_set_timing", [vp, i32], i32),
                ("dino_get_timing", [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)], i32),
                ("dino_dims", [vp] + [C.POINTER(C.c_int32)] * 6, i32),
                ("dino_destroy", [vp], None),
                ("dino_last_error", [vp], C.c_char_p),
                ("op_dino_resize_aa", [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp], i32),
                ("op_dino_normalize", [vp, vp, i64, vp], i32),
                ("op_dino_im2col", [vp, vp, i32, vp], i32),
                ("op_dino_tokens", [vp, vp, vp, vp, i32, i32, vp], i32),
                ("op_dino_layernorm", [vp, vp, vp, vp, i32, i32, vp], i32),
                ("op_dino_strip", [vp, vp, i32, i32, vp], i32),
                ("op_dino_shuffle", [vp, vp, vp, i32, i32, i32, vp], i32),
                ("op_dino_gather_s2", [vp, vp, i32, i32, vp], i32),
                ("op_dino_concat", [vp, vp, vp, i64, i32, vp], i32),
                ("op_dino_resize_ac", [vp, vp, i32, i32, i32, i32, i32, vp], i32),
                ("op_dino_add_relu", [vp, vp, vp, vp, i64, vp], i32),
                ("op_dino_output", [vp, vp, i64, i32, vp, vp, i32, vp], i32)):
            f = getattr(L, "artalk_" + name)
            f.argtypes, f.restype = args, res
    if hasattr(L, "artalk_pcm_create"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the live audio front door)
        pi64 = C.POINTER(i64)
        for name, args, res in (
                ("pcm_create", [i32, i32, i32, i32, C.POINTER(vp)], i32),
                ("pcm_destroy", [vp], None),
                ("pcm_last_error", [vp], C.c_char_p),
                ("pcm_set_rate", [vp, i32, vp, i32, i32, i32], i32),
                ("pcm_open", [vp, i32, i32, i32, pi64], i32),
                ("pcm_close", [vp, i64], i32),
                ("pcm_push", [vp, pi64, i32, C.POINTER(vp), pi64, i32, vp], i32),
                ("pcm_end", [vp, pi64, i32, vp], i32),
                ("pcm_available", [vp, i64, pi64, C.POINTER(i32)], i32),
                ("pcm_take", [vp, pi64, i32, vp, i64, pi64, vp], i32),
                ("op_pcm_plan", [i64, i64, i32, i32, i32, i32, pi64], i32),
                ("op_pcm_desc_bytes", [i32], i32),
                ("op_pcm_push", [C.POINTER(PcmDesc), i32, vp, i64, vp], i32),
                ("op_pcm_take", [C.POINTER(PcmTakeDesc), i32, vp, i64, vp, i64, i32, vp], i32)):
            f = getattr(L, "artalk_" + name)
            f.argtypes, f.restype = args, res
    if hasattr(L, "artalk_jpeg_encode"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks the JPEG encoder)
        for name, args, res in (
                ("jpeg_default_cap", [i32, i32], i64),
                ("jpeg_bound", [i32, i32, i32], i64),
                ("jpeg_header", [i32, i32, i32, i32, vp, i32], i32),
                ("jpeg_create", [i32, C.POINTER(vp)], i32),
                ("jpeg_destroy", [vp], None),
                ("jpeg_last_error", [vp], C.c_char_p),
                ("jpeg_encode", [vp, vp, i32, i32, i32, i32, i32, vp, i64, vp, vp], i32),
                ("jpeg_set_timing", [vp, i32], i32),
                ("jpeg_get_timing", [vp, C.POINTER(C.c_double), i32], i32),
                ("op_jpeg_check", [i32, i32, i32, i32, i32, i64, i32, i32, i32, C.c_char_p, i32], i32)):
            f = getattr(L, "artalk_" + name)
            f.argtypes, f.restype = args, res
    L.artalk_savgol.argtypes = [vp, vp, vp, i32, vp]
    L.artalk_savgol.restype = i32
    L.artalk_set_profiling.argtypes = [vp, i32]
    L.artalk_set_profiling.restype = i32
    L.artalk_get_profile.argtypes = [vp, C.POINTER(C.c_double), i32]
    L.artalk_get_profile.restype = i32
    if hasattr(L, "artalk_get_kernel_sums"):      # (round 5)
        L.artalk_get_kernel_sums.argtypes = [vp, C.POINTER(C.c_double), i32]
        L.artalk_get_kernel_sums.restype = i32
    L.artalk_set_graphs.argtypes = [vp, i32]
    L.artalk_set_graphs.restype = i32
    if hasattr(L, "artalk_graph_count"):      # (round 5; an older build loaded through ARTALK_LIB lacks it)
        L.artalk_graph_count.argtypes = [vp, C.POINTER(C.c_longlong)]
        L.artalk_graph_count.restype = i32
    if hasattr(L, "artalk_set_audit"):      # (an older build loaded through ARTALK_LIB for an A/B run may lack it)
        L.artalk_set_audit.argtypes = [vp, i32]
        L.artalk_set_audit.restype = i32
        L.artalk_get_audit.argtypes = [vp, C.c_char_p, i32, C.POINTER(C.c_float), i32]
        L.artalk_get_audit.restype = i32
    if hasattr(L, "artalk_calibrate"):      # (round 5)
        L.artalk_calibrate.argtypes = [vp, f32]
        L.artalk_calibrate.restype = i32
        L.artalk_reset_scales.argtypes = [vp]
        L.artalk_reset_scales.restype = i32
        L.artalk_get_scales.argtypes = [vp, C.POINTER(C.c_int), i32]
        L.artalk_get_scales.restype = i32
    if hasattr(L, "artalk_set_site_scales"):
        L.artalk_scale_sites.argtypes = [vp, C.c_char_p, i32]
        L.artalk_scale_sites.restype = i32
        L.artalk_get_site_scales.argtypes = [vp, C.POINTER(C.c_int), i32]
        L.artalk_get_site_scales.restype = i32
        L.artalk_set_site_scales.argtypes = [vp, C.POINTER(C.c_int), i32]
        L.artalk_set_site_scales.restype = i32
    L.artalk_op_gemm.argtypes = [vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
    L.artalk_op_gemm.restype = i32
    L.artalk_set_precision.argtypes = [vp, i32]
    L.artalk_set_precision.restype = i32
    if hasattr(L, "artalk_op_gemm_bf16"):      # (an older build loaded through ARTALK_LIB for an A/B run lacks it)
        L.artalk_op_gemm_bf16.argtypes = [vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
        L.artalk_op_gemm_bf16.restype = i32
    L.artalk_op_gemm_f16s.argtypes = [vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.artalk_op_gemm_f16s.restype = i32
    L.artalk_op_pack_split.argtypes = [vp, vp, i64, i32, vp]
    L.artalk_op_pack_split.restype = i32
    L.artalk_op_gemm_f16s_packed.argtypes = [vp, i32, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.artalk_op_gemm_f16s_packed.restype = i32
    if hasattr(L, "artalk_set_tap"):      # (an older build loaded through ARTALK_LIB for a same-box A/B run lacks the round-4 entry points)
        L.artalk_set_tap.argtypes = [vp, vp, i32, i32]
        L.artalk_set_tap.restype = i32
        L.artalk_tap_layout.argtypes = [C.POINTER(C.c_int64), i32]
        L.artalk_tap_layout.restype = i32
        L.artalk_op_release_scratch.argtypes = []
        L.artalk_op_release_scratch.restype = i32
    L.artalk_set_cu_mask.argtypes = [vp, vp, i32]
    L.artalk_set_cu_mask.restype = i32
    L.artalk_op_create_masked_stream.argtypes = [vp, i32, C.POINTER(vp)]
    L.artalk_op_create_masked_stream.restype = i32
    L.artalk_op_destroy_stream.argtypes = [vp]
    L.artalk_op_destroy_stream.restype = i32
    L.artalk_op_gemm_p8_plan.argtypes = [i32, i32, i32, i32]
    L.artalk_op_gemm_p8_plan.restype = i32
    L.artalk_op_gemm_ex.argtypes = [vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    L.artalk_op_gemm_ex.restype = i32
    L.artalk_op_mfma_f32_peak.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_double), vp]
    L.artalk_op_mfma_f32_peak.restype = i32
    L.artalk_op_layernorm.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, vp]
    L.artalk_op_layernorm.restype = i32
    L.artalk_op_attention.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, i32, vp]
    L.artalk_op_attention.restype = i32
    L.artalk_op_w2v_front.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.artalk_op_w2v_front.restype = i32
    L.artalk_op_resample_mean.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp, i32, vp]
    L.artalk_op_resample_mean.restype = i32
    L.artalk_op_pool_silu.argtypes = [vp, i32, i32, i32, vp, vp]
    L.artalk_op_pool_silu.restype = i32
    L.artalk_op_bsq_history.argtypes = [vp, vp, vp, vp, i32, vp]
    L.artalk_op_bsq_history.restype = i32
    if hasattr(L, "artalk_op_pack_split_ex"):      # (an older build loaded through ARTALK_LIB lacks the entry points with site exponents)
        L.artalk_op_pack_split_ex.argtypes = [vp, vp, i64, i32, i32, vp, vp]
        L.artalk_op_pack_split_ex.restype = i32
        L.artalk_op_layernorm_ex.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, i32, i32, i32, vp, vp]
        L.artalk_op_layernorm_ex.restype = i32
        L.artalk_op_gemm_f16s_packed_ex.argtypes = [vp, i32, i64, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]
        L.artalk_op_gemm_f16s_packed_ex.restype = i32
        L.artalk_op_gemm_f16s_ex.argtypes = [vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]
        L.artalk_op_gemm_f16s_ex.restype = i32
        L.artalk_op_attention_ex.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, i32, i32, i32, i32, vp, vp]
        L.artalk_op_attention_ex.restype = i32
        L.artalk_op_w2v_front_ex.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
        L.artalk_op_w2v_front_ex.restype = i32
        L.artalk_op_pool_silu_ex.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, vp]
        L.artalk_op_pool_silu_ex.restype = i32
        L.artalk_op_posconv_p8_ex.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
        L.artalk_op_posconv_p8_ex.restype = i32
    if hasattr(L, "artalk_op_ar_bits_next"):      # (an older build loaded through ARTALK_LIB lacks the single-kernel glue entry points)
        for name, args in (
                ("bsq_history_ex", [vp, vp, vp, vp, i32, vp, vp]),
                ("ar_bits_next", [vp, vp, vp, vp, i32, i32, vp, vp]),
                ("vq_embed", [vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, i32, vp]),
                ("ar_begin", [vp, vp, vp, vp, i32, vp]),
                ("dec_input", [vp, vp, vp, vp, vp, i32, vp]),
                ("dec_finish", [vp, vp, vp, vp, vp, i64, i32, vp, i32, vp, vp]),
                ("enc_input_zero", [vp, vp, vp, vp, i32, vp]),
                ("style_input", [vp, vp, vp, vp, i32, vp]),
                ("add_row", [vp, vp, i32, i32, vp]),
                ("style_finish", [vp, vp, vp, vp, vp, vp, i32, vp, i64, vp]),
                ("broadcast16", [vp, vp, i64, i32, vp]),
                ("session_gather", [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
                ("session_scatter", [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
                ("absmax", [vp, i32, i32, i64, i32, i32, i32, i32, vp, vp])):
            f = getattr(L, "artalk_op_" + name)
            f.argtypes, f.restype = args, i32
    if hasattr(L, "artalk_op_gemm_rows"):      # (an older build loaded through ARTALK_LIB lacks the row-mapped entry points)
        L.artalk_op_gemm_rows.argtypes = [C.POINTER(GemmRowsArgs), vp]
        L.artalk_op_gemm_rows.restype = i32
        L.artalk_op_layernorm_rows.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, i32, i32, i32, i32, vp,
                                               i64, i64, i64, C.POINTER(C.c_int32), i64, i64, i64, vp]
        L.artalk_op_layernorm_rows.restype = i32
        L.artalk_op_attention_rows.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, i32, i32, i32, i32, vp,
                                               i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, vp]
        L.artalk_op_attention_rows.restype = i32
        L.artalk_op_gemm_rows_layout.argtypes = [C.POINTER(i64), i32]
        L.artalk_op_gemm_rows_layout.restype = i32
        L.artalk_op_rows_dry_run.argtypes = [i32]
        L.artalk_op_rows_dry_run.restype = i32
    if hasattr(L, "artalk_op_attention_plan"):      # (an older build loaded through ARTALK_LIB lacks the attention planner's entry points)
        L.artalk_op_attention_plan.argtypes = [i32] * 9
        L.artalk_op_attention_plan.restype = i32
        L.artalk_op_attention_rows_cus.argtypes = L.artalk_op_attention_rows.argtypes[:-1] + [i32, C.POINTER(C.c_int32), vp]
        L.artalk_op_attention_rows_cus.restype = i32
    if hasattr(L, "artalk_op_gemm_blocked"):      # (an older build loaded through ARTALK_LIB lacks the blocked-sum entry point)
        L.artalk_op_gemm_blocked.argtypes, L.artalk_op_gemm_blocked.restype = L.artalk_op_gemm.argtypes, i32
    if hasattr(L, "artalk_op_w2v_front_rows"):     # (an older build loaded through ARTALK_LIB lacks the chunk-strided wav2vec2 entry points)
        L.artalk_op_w2v_front_rows.argtypes = [vp, i64, C.POINTER(i64), i32, i32, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, vp]
        L.artalk_op_w2v_front_rows.restype = i32
        L.artalk_op_pool_silu_rows.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, i64, i64, i64, vp]
        L.artalk_op_pool_silu_rows.restype = i32
        L.artalk_op_posconv_rows.argtypes = [i32, vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]
        L.artalk_op_posconv_rows.restype = i32
    _lib = L
    return L


def ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def conv_tail_geometry(valid: int, cfg: ARTalkConfig = None):
    """``artalk_conv_tail_geometry`` for a chunk with ``valid`` real samples: (partial, t_const, Tp, Sp, samples_read), lists per conv
    layer.  Host only: needs no GPU."""
    cfg = cfg or ARTalkConfig.full()
    kernel, stride = list(cfg.w2v["conv_kernel"]), list(cfg.w2v["conv_stride"])
    n = len(kernel)
    arr = C.c_int32 * n
    k, st, tc, tp, sp = arr(*kernel), arr(*stride), arr(), arr(), arr()
    read = C.c_int32(0)
    rc = lib().artalk_conv_tail_geometry(int(valid), int(cfg.samples_per_chunk), n, k, st, tc, tp, sp, C.byref(read))
    if rc < 0:
        raise ValueError(f"artalk_conv_tail_geometry({valid}) failed ({rc})")
    return bool(rc), list(tc), list(tp), list(sp), int(read.value)


def conv_tail_class(valid: int, samples_per_chunk: int = 64000) -> int:
    """Upper bound, in samples, of the length class a chunk with ``valid`` real samples runs at (``artalk_conv_tail_class``)."""
    rc = int(lib().artalk_conv_tail_class(int(valid), int(samples_per_chunk)))
    if rc < 0:
        raise ValueError(f"artalk_conv_tail_class({valid}) failed ({rc})")
    return rc


CONV_PLAN_FIELDS = ("NT", "VA", "VB", "NP", "grid_x", "grid_y", "steps", "Cinp", "Kp")


def conv2d_plan(x_addr: int, x_bstride: int, w_addr: int, in_scale_addr: int, B: int, H: int, W: int, Cin: int, Cout: int, k: int,
                precision: int) -> dict:
    """``artalk_op_conv2d_plan`` as a dict over CONV_PLAN_FIELDS: the instantiation and grid ``artalk_op_conv2d_ex`` runs for these
    arguments (addresses are only looked at for presence and alignment; in_scale_addr 0 = no input scale).  Host only: needs no GPU."""
    out = (C.c_int32 * len(CONV_PLAN_FIELDS))()
    rc = int(lib().artalk_op_conv2d_plan(x_addr, x_bstride, w_addr, in_scale_addr, B, H, W, Cin, Cout, k, precision, out, len(out)))
    if rc < 0:
        raise ValueError(f"artalk_op_conv2d_plan refused its arguments ({rc})")
    assert rc == len(CONV_PLAN_FIELDS), rc
    return dict(zip(CONV_PLAN_FIELDS, out))


def conv_kernel_name(plan: dict) -> str:
    """The instantiation a plan of ``conv2d_plan`` names, as the sources spell it."""
    tf = lambda v: "true" if v else "false"
    if plan["NP"] == 0:
        return f"conv_mfma_kernel<{plan['NT']},{tf(plan['VA'])},{tf(plan['VB'])}>"
    return f"conv_bf16_kernel<{plan['NT']},{plan['NP']},{tf(plan['VA'])}>"
