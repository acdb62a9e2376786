"""ctypes binding of libsgg_hip.so (include/sgg_hip.h) on torch device tensors.

PyTorch is plumbing only here: it owns device memory and the stream; every arithmetic op of the hot path is a
hand-written HIP kernel behind the C ABI.  There is NO fallback: if the shared object is missing, fails to
load, or a tensor is not on a HIP device, the call raises.

Tensor conventions used by the host orchestration (trunk.py / head.py / step.py):
  * head tensors carry a leading "plane" dimension: [1, R, W] for plain fp32, [2, R, W] for dual numbers
    (plane 0 = real part, plane 1 = dual part; see csrc/dual.h).  Column slices of such buffers are passed as
    strided views; the binding extracts base pointers and the row stride (leading dimension).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_longlong, c_size_t, c_ulonglong, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsgg_hip.so")

_vp, _i, _f, _sz, _ll, _ull = c_void_p, c_int, c_float, c_size_t, c_longlong, c_ulonglong

# name -> (restype, argtypes); must list every symbol declared in include/sgg_hip.h
SIGNATURES = {
    "sgg_version": (_i, []),
    "sgg_last_error": (c_char_p, []),
    "sgg_device_info": (_i, [_vp, _vp, _vp, _vp, _i]),
    "sgg_hwio_to_hwoi": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sgg_conv_split_weights": (_i, [_vp, _vp, _ll, _i, _vp, _vp]),
    "sgg_absmax": (_i, [_vp, _ll, _vp, _vp]),
    "sgg_conv_wsplit_layout": (_i, [_i] * 8),
    "sgg_conv_wsplit_layout_presplit": (_i, [_i] * 8),
    "sgg_conv_s2d_weights": (_i, [_vp, _vp, _i, _i, _vp]),
    "sgg_conv_prepare_weights": (_i, [_vp, _i, _i, _vp]),
    "sgg_conv_split_weights_frag": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sgg_conv_split_weights_frag16": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sgg_conv2d_nhwc_fwd": (_i, [_vp, _vp, _vp, _vp, _vp] + [_i] * 14 + [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "sgg_conv2d_nhwc_fwd_tile_stats": (_i, [_i] * 9),
    "sgg_presplit16": (_i, [_vp, _vp, _ll, _vp, _vp]),
    "sgg_conv2d_nhwc_dgrad": (_i, [_vp, _vp, _vp, _vp] + [_i] * 14 + [_vp, _vp, _i, _vp]),
    "sgg_conv2d_nhwc_fwd_symbol": (_i, [_i] * 18 + [c_char_p, _i]),
    "sgg_conv2d_nhwc_dgrad_symbol": (_i, [_i] * 16 + [c_char_p, _i]),
    "sgg_conv2d_nhwc_wgrad_workspace_bytes": (_sz, [_i] * 9),
    "sgg_conv2d_nhwc_wgrad": (_i, [_vp, _vp, _vp] + [_i] * 14 + [_vp, _vp, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "sgg_conv2d_nhwc_wgrad_resident": (_i, [_i] * 9),
    "sgg_conv2d_nhwc_wgrad_symbol": (_i, [_i] * 16 + [_vp, c_char_p, _i]),
    "sgg_layernorm_hwc_elu_workspace_bytes": (_sz, [_i, _i, _i]),
    "sgg_layernorm_hwc_elu_fwd": (_i, [_vp] * 7 + [_i] * 10 + [_vp, _sz, _vp]),
    "sgg_layernorm_hwc_elu_bwd": (_i, [_vp] * 10 + [_i] * 9 + [_vp, _vp, _sz, _vp]),
    "sgg_layernorm_hwc_bwd_finalize": (_i, [_vp, _i, _vp]),
    "sgg_layernorm_hwc_finalize": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "sgg_spatial_mean_fwd": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "sgg_spatial_mean_bwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    "sgg_gemm_workspace_bytes": (_sz, [_i, _i, _i]),
    "sgg_gemm_skinny_fwd": (_i, [_i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _sz, _vp]),
    "sgg_gemm_skinny_dgrad": (_i, [_i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _sz, _vp]),
    "sgg_gemm_skinny_wgrad": (_i, [_i, _i, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _sz, _vp]),
    "sgg_gemm_skinny_symbol": (_i, [_i, _i, _i, _i, _vp, c_char_p, _i]),
    "sgg_attn_step_fwd_symbol": (_i, [_i, _i, _i, _i, _i, c_char_p, _i]),
    "sgg_attn_step_bwd_symbol": (_i, [_i, _i, _i, _i, _i, c_char_p, _i]),
    "sgg_layernorm_hwc_elu_bwd_sums": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "sgg_conv2d_nhwc_wgrad_c3_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "sgg_conv2d_nhwc_dgrad_c3": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sgg_conv2d_nhwc_dgrad_c3_ln": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sgg_attn_ctx_gemm_fwd": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgg_attn_ctx_gemm_dgrad": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "sgg_attn_ctx_gemm_wgrad": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "sgg_attn_step_fwd": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sgg_attn_step_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "sgg_lnlstm_gates_fwd": (_i, [_vp] * 9 + [_i, _i, _vp]),
    "sgg_lnlstm_gates_bwd": (_i, [_vp] * 7 + [_i] + [_vp] * 7 + [_i, _vp]),
    "sgg_colsum_workspace_bytes": (_sz, [_i, _i]),
    "sgg_colsum": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _sz, _vp]),
    "sgg_onehot": (_i, [_vp, _vp, _i, _i, _vp]),
    "sgg_resize_bilinear_tf1": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sgg_embed_gather_fwd": (_i, [_vp, _i, _vp, _i, _i, _vp, _i, _i, _vp]),
    "sgg_embed_gather_bwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp]),
    "sgg_interpolate": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "sgg_wgan_gp_loss_fwd": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "sgg_wgan_gp_loss_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "sgg_wgan_losses": (_i, [_vp, _vp, _f, _i, _i, _i, _vp, _vp]),
    "sgg_adam_tf_multi": (_i, [_vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _f, _vp]),
    "sgg_adam_tf_multi_ema": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _f, _f, _vp]),
    "sgg_swap_f32": (_i, [_vp, _vp, _ll, _vp]),
    "sgg_grad_accumulate": (_i, [_vp, _vp, _ll, _i, _vp]),
    "sgg_grad_guard_workspace_bytes": (_sz, [_ll]),
    "sgg_grad_guard": (_i, [_vp, _ll, _f, _f, _i, _i, _vp, _sz, _vp, _vp]),
    "sgg_adam_tf_multi_guarded": (_i, [_vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _vp, _vp]),
    "sgg_adam_tf_multi_ema_guarded": (_i, [_vp, _vp, _vp, _vp, _vp, _ll, _f, _f, _f, _f, _vp, _f, _vp]),
    "sgg_argmax_rows": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "sgg_rank_triples": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sgg_match_triples": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "sgg_kbest_triples": (_i, [_vp, _ll, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sgg_kbest_merge": (_i, [_vp, _vp, _ll, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sgg_ground_assign": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sgg_ground_pool": (_i, [_vp, _vp, _vp, _ll, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sgg_ground_resolve": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f] + [_vp] * 10),
    "sgg_softmax_xent": (_i, [_vp, _ll, _i, _i, _vp, _f, _i, _vp, _ll, _vp, _vp, _vp, _vp]),
    "sgg_xent_summary": (_i, [_vp, _vp, _i, _vp, _vp]),
    "sgg_triple_logp": (_i, [_vp, _ll, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sgg_query_logp": (_i, [_vp, _ll, _vp, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp, _ll, _ll, _vp]),
    "sgg_retrieve_topk": (_i, [_vp, _ll, _i, _i, _i, _vp, _vp, _vp]),
    "sgg_retrieve_ranks": (_i, [_vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sgg_pair_predicate_logp": (_i, [_vp, _ll, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _ll, _vp, _vp, _vp]),
    "sgg_predcls_pair_topk": (_i, [_vp, _ll, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "sgg_predcls_merge": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "sgg_relax_rows": (_i, [_vp, _ll, _i, _i, _f, _i, _ull, _ull, _vp, _ll, _vp, _ll, _vp]),
    "sgg_relax_rows_bwd": (_i, [_vp, _ll, _vp, _ll, _i, _i, _f, _f, _vp, _ll, _vp]),
    "sgg_relax_rows_hard": (_i, [_vp, _ll, _i, _i, _i, _ull, _ull, _vp, _ll, _vp, _vp]),
    "sgg_relax_rows_hard_bwd": (_i, [_vp, _ll, _vp, _ll, _i, _i, _f, _f, _i, _ull, _ull, _vp, _ll, _vp]),
    "sgg_score_advantage": (_i, [_vp, _ll, _i, _i, _i, _vp, _vp, _vp]),
    "sgg_score_rows": (_i, [_vp, _ll, _i, _i, _vp, _vp, _i, _f, _f, _i, _vp, _ll, _vp, _vp, _vp]),
    "sgg_score_summary": (_i, [_vp, _vp, _i, _vp, _vp]),
    "sgg_sample_rows_multi": (_i, [_vp, _ll, _i, _i, _i, _ull, _ull, _vp, _vp]),
    "sgg_score_advantage_multi": (_i, [_vp, _ll, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sgg_score_rows_multi": (_i, [_vp, _ll, _i, _i, _i, _vp, _vp, _i, _f, _f, _i, _vp, _ll, _vp, _vp, _vp]),
    "sgg_score_summary_multi": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "sgg_arena_stats_chunk": (_i, []),
    "sgg_arena_stats_nstat": (_i, []),
    "sgg_arena_stats_workspace_bytes": (_sz, [_i]),
    "sgg_arena_stats": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _f, _i, _vp, _sz, _vp, _vp]),
    "sgg_vector_stats": (_i, [_vp, _i, _f, _vp, _vp]),
    "sgg_fill": (_i, [_vp, _ll, _f, _vp]),
    "sgg_augment_plan_workspace_bytes": (_sz, [_i]),
    "sgg_augment_plan": (_i, [_vp] * 6 + [_i] * 7 + [_ull, _ull, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sgg_augment_resize": (_i, [_vp] * 6 + [_i, _vp, _i, _i, _i, _vp, _vp, _vp]),
}

# timing label of a conv_wgrad call by the first matching prefix of the kernel the library routes it to (bench.py's output and
# DESIGN.md are keyed by the labels)
WGRAD_LABELS = (("conv_c3_wgrad", "conv_c3_wgrad(call: kernel + slab reduce)"),
                ("conv_wgrad_dma", "conv_wgrad_dma(call: LDS-DMA kernel on pre-split operands + slab reduce)"),
                ("conv_wgrad", "conv_wgrad(call: wgrad kernel + slab reduce)"))

_lib = None


class ConvWeightDesc(ctypes.Structure):
    """sgg_conv_weight_desc of include/sgg_hip.h."""
    _fields_ = [("w", c_void_p), ("w_hwoi", c_void_p), ("w3", c_void_p), ("w3_hwoi", c_void_p), ("ws_fwd", c_void_p),
                ("ws_bwd", c_void_p), ("amax", c_void_p), ("taps", c_int), ("cin", c_int), ("cout", c_int), ("layout_fwd", c_int),
                ("layout_bwd", c_int)]


class LnFinalizeDesc(ctypes.Structure):
    """sgg_ln_finalize_desc of include/sgg_hip.h."""
    _fields_ = [("workspace", c_void_p), ("gamma", c_void_p), ("stats", c_void_p), ("dgamma", c_void_p), ("dbeta", c_void_p),
                ("dbias_prev", c_void_p), ("B", c_int), ("HW", c_int), ("C", c_int), ("HW_valid", c_int)]


class SggError(RuntimeError):
    pass


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libsgg_hip.so and bind every declared symbol. Raises if the library or a symbol is missing.
    SGG_HIP_LIB overrides the path (experimental -D builds, scripts/build_variant_lib.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SGG_HIP_LIB", path)
    if not os.path.exists(path):
        raise SggError("libsgg_hip.so not found at %s - run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)" % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def same_pads(in_size: int, k: int, s: int):
    """TF SAME padding (tf.layers.conv2d(padding="same"), generator_with_attention.py:29): (out, before, after)."""
    out = -(-in_size // s)
    total = max((out - 1) * s + k - in_size, 0)
    return out, total // 2, total - total // 2


def _p(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    """row stride of a 2-D view whose last dim is contiguous (torch reports arbitrary strides for size-1 dims)"""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


# Documented run-time options of HipKernels (the whole experiment surface: the library has no build-time switches).
# HipKernels(options={...}) takes any subset; scripts may override them without touching code through ONE environment variable, SGG_OPTIONS="key=value,key=value" (lists: values joined by '+').
DEFAULT_OPTIONS = {
    # Convolution contraction mode (csrc/conv_gather.hip, conv_wgrad.hip):
    #   2 (default) f32 operands scaled by a per-tensor power of two and split into two fp16 pieces with round-to-nearest
    #               (23 significant bits), 3 fp16 MFMAs per product, f32 accumulate: error against fp64 within 2x the native
    #               f32 path's + 3e-7 (tests/test_fullsize_conv_gpu.py);
    #   6           three bf16 pieces, 6 bf16 MFMAs (no scaling needed): also f32-equivalent, slower;
    #   0           native f32 MFMA (v_mfma_f32_32x32x2_f32, bit-exact f32 fmaf chain);
    #   3           two bf16 pieces, 3 MFMAs: drops 2^-17 cross terms (inside the stated 1e-4 tolerance);
    #   1 / 4       ONE fp16 / bf16 piece: mixed-precision modes, NOT the reference's arithmetic (include/sgg_hip.h).
    "conv_precision": 2,
    # False: every convolution on the gather kernels (no resident halo / band / producer-consumer kernels)
    "conv_halo": True,
    # False: the 128-column 3x3 layers stay on the four-wave halo kernel (w_split_layout 1 instead of 4)
    "halo_pc": True,
    # True: the dgrads of the 64-column 3x3 layers whose dy arrives pre-split (conv2_2, conv2_3) run on the four-block form of the
    # producer / consumer kernel (trunk._query_layouts; csrc/conv_halo_pc.hip NB = 4)
    "halo_pc64": True,
    # LayerNorm + ELU applied by the consuming convolution's patch staging (LN prologue): 1 (default) = per layer and per KIND of
    # encoder pass (forward-only / followed by a backward) where the measured cost models (trunk.ln_fusion_pays, pc_ln_fusion_pays) say it pays
    # (trunk._plan: with pre-split activations 20 of the 44 apply passes of a step at configs[1] run as prologues, 24 as
    # standalone passes - DESIGN.md "The LN prologue"); 2 = wherever the kernels allow (slower: DESIGN.md); 0 = never
    "ln_fusion": 1,
    # True: the LayerNorm kernels write their outputs pre-split for the convolutions that consume them (trunk._plan; fp16 modes)
    "presplit": True,
    # True (with presplit): the gradient the attention head hands to the last convolution is converted to the pre-split format once
    # per backward (sgg_presplit16), so that `downsampled`'s dgrad and filter gradient stage it by DMA as well
    "presplit_head_grad": True,
    # two-stream schedule: True = the filter gradient of layer j starts when dgrad_j has finished (beside the LayerNorm backward of
    # layer j - 1) instead of together with dgrad_j (trunk.backward)
    "wgrad_late": True,
    # two-stream schedule: HIP priority of the side streams (0 = default; positive = lower than the main stream's, negative = higher)
    "side_priority": 0,
    # two-stream schedule: 1 = G's encoder forward of the update after a critic update starts on a stream of its own as soon as that
    # critic update's G head has run, beside its heads and encoder backward (step.GanStep._g_early_stream)
    "g_early": 1,
    # ... and while it runs there its persistent convolution kernels occupy only this many of an XCD's 32 CUs (0 = all): the critic's
    # recurrent heads - a chain of short launches on the critical path - then find free CUs at once instead of waiting for a resident
    # workgroup of G's forward to finish its tile.  The convolutions lose nothing on 28 of 32 CUs (every persistent kernel capped at
    # 28: +0.25 ms per step only, profiles/r05_persistent_cu_cap_ab.log); 28 here: 42.75 / 42.80 against 43.04 / 42.97 ms per step, on
    # another box 44.02 / 44.07 against 44.32 / 44.18; 30, 26, 24, 20: equal to none (profiles/r05_early_forward_cu_cap_ab*.log).
    # Tiles, products and summation orders are unchanged: bit-identical results (tests/test_concurrency_gpu.py, tests/test_persistent_tiles_gpu.py)
    "g_early_cus": 28,
    # True: the LayerNorm backward of conv1_1's output runs without its apply pass - conv1_1's filter gradient, the only consumer of
    # that dy, computes it itself (sgg_conv2d_nhwc_wgrad_c3_ln): one read of y and da instead of the apply pass (2 reads + 1 write of
    # 411 MB at batch 64) + the filter gradient's read of dy, on the tail of every encoder backward
    "c3_ln_bwd_fused": True,
    "d_side_cus": 0,      # the same for D's encoder forward on the side stream (beside G's forward and G's head)
    "fwd_cus": 0,         # the same for every encoder forward (16: G's and D's forwards of an update on disjoint halves of the chip)
    # cost-model overrides for A/B runs (conv indices): never fuse / fuse in forward-only passes / fuse in passes with backward /
    # never fuse in passes with backward
    "ln_fusion_skip": (),
    "ln_fusion_force": (),
    "ln_fusion_force_bwd": (),
    "ln_fusion_skip_bwd": (),
}


# What each option means for a kernel set that does not declare it - one without resident kernels, operand formats or streams, such as
# the CPU reference kernels or a stub in a test: plain f32 convolutions, every LayerNorm a pass of its own, one stream.  The ONE set of
# off-values of the host schedule (trunk.py, step.py read every option through `option`).
OFF_OPTIONS = {key: () if isinstance(val, tuple) else type(val)(0) for key, val in DEFAULT_OPTIONS.items()}


def option(K, name):
    """Option `name` of the kernel set K: its attribute (HipKernels sets every one), else the off-value."""
    return getattr(K, name, OFF_OPTIONS[name])


def options_from_env(base=None):
    """DEFAULT_OPTIONS (or `base`) with the overrides of SGG_OPTIONS applied: the one environment hook of the host side."""
    opts = dict(DEFAULT_OPTIONS if base is None else base)
    for item in filter(None, os.environ.get("SGG_OPTIONS", "").split(",")):
        key, _, val = item.partition("=")
        key = key.strip()
        if key not in DEFAULT_OPTIONS:
            raise SggError("SGG_OPTIONS: unknown option %r (known: %s)" % (key, ", ".join(sorted(DEFAULT_OPTIONS))))
        d = DEFAULT_OPTIONS[key]
        if isinstance(d, bool):
            opts[key] = val.strip().lower() not in ("0", "false", "no", "off", "")
        elif isinstance(d, tuple):
            opts[key] = tuple(int(v) for v in val.split("+") if v.strip())
        else:
            opts[key] = int(val)
    return opts


class HipKernels:
    """Tensor-level wrapper of the C ABI. All tensors must be fp32 (int64 where stated) on one HIP device.
    options: a subset of DEFAULT_OPTIONS; they become attributes of the same name (read by trunk.py)."""

    name = "hip"

    def __init__(self, device=None, options=None):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise SggError("no HIP device visible: the scene-graph-gan_amd product path has no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self._ws_by_stream = {}
        self.timing = None      # bench.py sets this to a list: launches are then bracketed by HIP events
        self.timing_conv_only = False   # True: only the MFMA-bound convolution calls are bracketed (the timed region of bench.py)
        self.timing_symbols = None      # with timing_conv_only True: bracket only these kernel symbols (bench.py: the dominant one)
        opts = options_from_env()
        for key, val in (options or {}).items():
            if key not in DEFAULT_OPTIONS:
                raise SggError("HipKernels: unknown option %r" % key)
            opts[key] = val
        for key, val in opts.items():
            setattr(self, key, tuple(val) if isinstance(DEFAULT_OPTIONS[key], tuple) else val)
        self.conv_precision = int(self.conv_precision)
        assert self.conv_precision in (0, 1, 2, 3, 4, 6)       # 1 / 4: single-piece (mixed-precision) modes, include/sgg_hip.h
        self._amax_by_stream = {}

    def _timed(self, symbol, flops, fn, nbytes=0.0):
        """Run fn() between two HIP events on the launch stream when kernel timing is on (bench.py roofline legs).
        flops / nbytes: ALGORITHMIC work of the call (MFMA-bound convs: flops; HBM-bound kernels: bytes)."""
        # timing_conv_only: True = the forward / dgrad convolution launches only (the candidates of bench.py's `roofline`: every event
        # pair costs ~5 us of the timed region), "mfma" = every call with algorithmic FLOPs, False = everything
        if self.timing is None or (self.timing_conv_only == "mfma" and flops <= 0.0) or \
                (self.timing_conv_only is True and (not symbol.startswith(("conv_halo", "conv_s2", "conv_gather")) or
                                                   (self.timing_symbols is not None and symbol not in self.timing_symbols))):
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(self.device))
        r = fn()
        e1.record(torch.cuda.current_stream(self.device))
        self.timing.append((symbol, flops, nbytes, e0, e1))
        return r

    # -- plumbing ------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc, name):
        if rc != 0:
            raise SggError("%s failed (%d): %s" % (name, rc, self.lib.sgg_last_error().decode()))

    def _dev(self, *ts):
        for t in ts:
            if t is not None and (not t.is_cuda):
                raise SggError("tensor is not on a HIP device (no CPU fallback in the product path)")

    def workspace(self, nbytes: int):
        """Scratch buffer of the CURRENT stream (kernels on different streams may run concurrently)."""
        sid = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws_by_stream.get(sid)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(max(int(nbytes * 1.25) + 256, 1 << 20), dtype=torch.uint8, device=self.device)
            self._ws_by_stream[sid] = ws
        return ws

    def device_info(self):
        cu, lds, hbm = c_int(0), c_size_t(0), c_size_t(0)
        arch = ctypes.create_string_buffer(64)
        self._check(self.lib.sgg_device_info(ctypes.addressof(cu), ctypes.addressof(lds), ctypes.addressof(hbm),
                                             ctypes.addressof(arch), 64), "sgg_device_info")
        return {"cu_count": cu.value, "lds_bytes_per_cu": lds.value, "hbm_bytes": hbm.value, "arch": arch.value.decode()}

    # -- conv encoder ----------------------------------------------------------------------------------
    def hwio_to_hwoi(self, w, wt):
        self._dev(w, wt)
        kh, kw, ci, co = w.shape
        self._check(self.lib.sgg_hwio_to_hwoi(_p(w), _p(wt), kh * kw, ci, co, self._stream()), "sgg_hwio_to_hwoi")

    @staticmethod
    def _conv_dims(x_shape, w_shape, stride):
        B, Hi, Wi, Ci = x_shape
        KH, KW, Ci2, Co = w_shape
        assert Ci == Ci2
        Ho, pt, _ = same_pads(Hi, KH, stride)
        Wo, pl, _ = same_pads(Wi, KW, stride)
        return B, Hi, Wi, Ci, Ho, Wo, Co, KH, KW, stride, pt, pl

    def absmax(self, x, amax):
        """amax (1-element fp32 view, zeroed by the caller) = max(amax, max|x|)."""
        self._dev(x, amax)
        assert x.is_contiguous()
        self._check(self.lib.sgg_absmax(_p(x), x.numel(), _p(amax), self._stream()), "sgg_absmax")

    def presplit16(self, x, out, amax):
        """out = x in the pre-split format of the LayerNorm kernels (ln_elu_fwd(..., out_s16=True)) under the scale of the word `amax`
        (max|x| or a bound); x: contiguous f32 NHWC with C % 32 == 0; out: same shape (may be x)."""
        self._dev(x, out, amax)
        assert x.is_contiguous() and out.is_contiguous() and out.numel() == x.numel() and x.shape[-1] % 32 == 0
        self._check(self.lib.sgg_presplit16(_p(x), _p(out), x.numel(), _p(amax), self._stream()), "sgg_presplit16")

    def _amax_or_compute(self, t, amax, slot):
        """precision 2 needs max|t| on the device; callers that track it pass `amax`, otherwise it is computed here."""
        if self.conv_precision not in (1, 2) or amax is not None or t is None:
            return amax
        sid = torch.cuda.current_stream(self.device).cuda_stream     # scratch words per stream, like workspace()
        scratch = self._amax_by_stream.get(sid)
        if scratch is None:
            scratch = self._amax_by_stream[sid] = torch.zeros(8, dtype=torch.float32, device=self.device)
        w = scratch[slot:slot + 1]
        self.fill(w, 0.0)
        self.absmax(t, w)
        return w

    def conv_wsplit_layout(self, k, stride, H, W, cin, cout):
        """Layout the conv entry points want for the pre-split weights of this layer: 0 = planes, 1 / 2 / 3 = MFMA fragment order
        (1: halo-resident 3x3 stride-1 kernel, 2: band-resident 5x5 stride-2 kernel, 3: conv1_3 through the space-to-depth view;
        H, W = the full-resolution grid), 4 = the fragments of the K = 32 MFMA shape for the producer / consumer 3x3 kernel
        (128-column tiles); SGG_CONV_HALO=0 keeps every layer on the gather kernel."""
        if not self.conv_halo:
            return 0
        lay = self.lib.sgg_conv_wsplit_layout(k, k, stride, H, W, cin, cout, self.conv_precision)
        return 1 if (lay == 4 and not self.halo_pc) else lay

    def conv_wsplit_layout_presplit(self, k, stride, H, W, cin, cout):
        """conv_wsplit_layout for a launch whose source operand WILL be a pre-split tensor: the 64-column 3x3 layers then also take
        layout 4 (the four-block form of the producer / consumer kernel; option halo_pc64).  Such a launch must pass x_s16 / dy_s16."""
        if not self.conv_halo:
            return 0
        if not (self.halo_pc and self.halo_pc64):
            return self.conv_wsplit_layout(k, stride, H, W, cin, cout)
        return self.lib.sgg_conv_wsplit_layout_presplit(k, k, stride, H, W, cin, cout, self.conv_precision)

    def split_weights(self, w, out, amax=None, layout=0):
        """w fp32 [kh, kw, N, C] -> out int16 [P, n] sixteen-bit planes (layout 0) or MFMA B fragments (layout 1)."""
        self._dev(w, out, amax)
        amax = self._amax_or_compute(w, amax, 2)
        if layout == 4:         # fragments of the K = 32 MFMA shape (producer / consumer 3x3 kernel)
            kh, kw, n, c = w.shape
            self._check(self.lib.sgg_conv_split_weights_frag16(_p(w), _p(out), kh * kw, n, c, self.conv_precision, _p(amax),
                                                               self._stream()), "sgg_conv_split_weights_frag16")
            return
        if layout in (1, 2, 3):
            kh, kw, n, c = w.shape
            self._check(self.lib.sgg_conv_split_weights_frag(_p(w), _p(out), kh * kw, n, c, self.conv_precision, _p(amax),
                                                             self._stream()), "sgg_conv_split_weights_frag")
            return
        self._check(self.lib.sgg_conv_split_weights(_p(w), _p(out), w.numel(), self.conv_precision, _p(amax), self._stream()),
                    "sgg_conv_split_weights")

    def s2d_weights(self, w5, w3):
        """HWIO [5,5,Ci,Co] -> the 9-tap kernel [3,3,4*Ci,Co] of the same stride-2 convolution over the space-to-depth view of x
        (w_split_layout 3; include/sgg_hip.h)."""
        self._dev(w5, w3)
        kh, kw, ci, co = w5.shape
        assert (kh, kw) == (5, 5) and tuple(w3.shape) == (3, 3, 4 * ci, co) and w5.is_contiguous() and w3.is_contiguous()
        self._check(self.lib.sgg_conv_s2d_weights(_p(w5), _p(w3), ci, co, self._stream()), "sgg_conv_s2d_weights")

    def weight_descs(self, layers):
        """layers: dicts with w, w_fwd, (w3, w3_fwd), ws_fwd, ws_bwd, amax (1-word view or None), ws_layout, ws_layout_bwd ->
        a ctypes array of sgg_conv_weight_desc for prepare_weights (the tensors must stay alive and in place)."""
        arr = (ConvWeightDesc * len(layers))()
        for d, lay in zip(arr, layers):
            w = lay["w"]
            kh, kw, ci, co = w.shape
            self._dev(w, lay["w_fwd"], lay.get("w3"), lay.get("w3_fwd"), lay.get("ws_fwd"), lay.get("ws_bwd"), lay.get("amax"))
            d.w, d.w_hwoi = _p(w), _p(lay["w_fwd"])
            d.w3, d.w3_hwoi = _p(lay.get("w3")), _p(lay.get("w3_fwd"))
            d.ws_fwd, d.ws_bwd, d.amax = _p(lay.get("ws_fwd")), _p(lay.get("ws_bwd")), _p(lay.get("amax"))
            d.taps, d.cin, d.cout, d.layout_fwd, d.layout_bwd = kh * kw, ci, co, lay["ws_layout"], lay["ws_layout_bwd"]
        return arr

    def prepare_weights(self, descs):
        """Transposes, max|w|, space-to-depth kernels and both pre-split copies of every layer in `descs` (weight_descs): three
        launches for a whole encoder (sgg_conv_prepare_weights)."""
        self._check(self.lib.sgg_conv_prepare_weights(ctypes.addressof(descs), len(descs), self.conv_precision, self._stream()),
                    "sgg_conv_prepare_weights")

    def conv_tile_stats_count(self, y_shape, cin, k=0, stride=0, layout=0):
        """(count, mean, M2) triples per sample the forward conv emits for this output shape in the current mode (0: none)."""
        return self.lib.sgg_conv2d_nhwc_fwd_tile_stats(y_shape[1], y_shape[2], cin, y_shape[3], k, k, stride, self.conv_precision,
                                                       layout)

    def _conv_symbol(self, query, *args, name=None):
        """The kernel symbol(s) of a convolution launch, as the library's own routing reports them (sgg_conv2d_nhwc_fwd_symbol /
        _dgrad_symbol / _wgrad_symbol: the launch's validation and route, scalars only).  Asked only while kernel timing is on."""
        buf = ctypes.create_string_buffer(256)
        self._check(getattr(self.lib, query)(*args, buf, len(buf)), name or query)      # (name: a refusal reads as the launch's own)
        return buf.value.decode()

    def conv_fwd(self, x, w_hwio, w_fwd, bias, y, stride, w_split=None, amax_x=None, amax_w=None, tile_stats=None, w_split_layout=0,
                 ln=None, x_s16=False, cu_cap=0):
        """y = conv2d_same(x, w) + bias. w_fwd: HWOI transpose of w_hwio (or w_hwio itself when Cin == 3).
        ln = (stats [B,2], gamma, beta): x is the producing layer's PRE-LayerNorm output; the kernel applies LN + ELU while staging
        (halo-resident kernel only; amax_x = the word ln_finalize published).
        x_s16: x is a pre-split tensor (ln_elu_fwd(..., out_s16=True); amax_x = the word that call published).
        cu_cap (1 .. 31): the persistent kernels occupy at most that many of an XCD's 32 CUs (operand_format bits 8 .. 13)."""
        self._dev(x, w_fwd, bias, y)
        ln_s, ln_g, ln_b = ln if ln is not None else (None, None, None)
        self._dev(ln_s, ln_g, ln_b)
        d = self._conv_dims(x.shape, w_hwio.shape, stride)
        assert tuple(y.shape) == (d[0], d[4], d[5], d[6]) and x.is_contiguous() and y.is_contiguous()
        flops = 2.0 * d[0] * d[4] * d[5] * d[6] * d[7] * d[8] * d[3]
        fmt = int(bool(x_s16)) | ((int(cu_cap) & 63) << 8)
        sym = "" if self.timing is None else self._conv_symbol("sgg_conv2d_nhwc_fwd_symbol", *d, self.conv_precision, w_split_layout,
                                                               w_split is not None, tile_stats is not None, ln is not None, fmt)
        nb = 0.0
        if d[3] != 3:
            amax_x, amax_w = self._amax_or_compute(x, amax_x, 0), self._amax_or_compute(w_fwd, amax_w, 1)
        else:
            nb = 4.0 * (x.numel() + y.numel())      # conv1_1 (K = 27) is HBM-bound: the image read once, y written once
        self._check(self._timed(sym, flops, lambda: self.lib.sgg_conv2d_nhwc_fwd(
            _p(x), _p(w_fwd), _p(w_split), _p(bias), _p(y), *d, self.conv_precision, w_split_layout, _p(amax_x), _p(amax_w),
            _p(tile_stats), _p(ln_s), _p(ln_g), _p(ln_b), fmt, self._stream()), nb),
            "sgg_conv2d_nhwc_fwd")

    def conv_dgrad(self, dy, w_hwio, dx, stride, w_split=None, amax_dy=None, amax_w=None, w_split_layout=0, dy_s16=False):
        """dy_s16: dy is a pre-split tensor (ln_elu_bwd(..., out_s16=True); amax_dy = the word that call published)."""
        self._dev(dy, w_hwio, dx)
        d = self._conv_dims(dx.shape, w_hwio.shape, stride)
        assert tuple(dy.shape) == (d[0], d[4], d[5], d[6]) and dy.is_contiguous() and dx.is_contiguous()
        flops = 2.0 * d[0] * d[4] * d[5] * d[6] * d[7] * d[8] * d[3]
        amax_dy, amax_w = self._amax_or_compute(dy, amax_dy, 0), self._amax_or_compute(w_hwio, amax_w, 1)
        sym = "" if self.timing is None else self._conv_symbol("sgg_conv2d_nhwc_dgrad_symbol", *d, self.conv_precision, w_split_layout,
                                                               w_split is not None, int(bool(dy_s16)))
        self._check(self._timed(sym, flops, lambda: self.lib.sgg_conv2d_nhwc_dgrad(
            _p(dy), _p(w_hwio), _p(w_split), _p(dx), *d, self.conv_precision, w_split_layout, _p(amax_dy), _p(amax_w),
            int(bool(dy_s16)), self._stream())), "sgg_conv2d_nhwc_dgrad")

    def wgrad_resident(self, B, Ho, Wo, cin, cout, k, stride):
        """True if conv_wgrad of this shape runs on the halo-resident kernel (the one that takes pre-split operands)."""
        return bool(self.conv_halo and self.lib.sgg_conv2d_nhwc_wgrad_resident(B, Ho, Wo, cin, cout, k, k, stride, self.conv_precision))

    def conv_wgrad(self, x, dy, dw, stride, amax_x=None, amax_dy=None, ln=None, x_s16=False, dy_s16=False):
        """ln: as conv_fwd (x = pre-LayerNorm output of the producing layer; halo-resident wgrad kernel only).
        x_s16 / dy_s16: the operand is a pre-split tensor of ln_elu_fwd / ln_elu_bwd (out_s16=True)."""
        self._dev(x, dy, dw)
        ln_s, ln_g, ln_b = ln if ln is not None else (None, None, None)
        self._dev(ln_s, ln_g, ln_b)
        d = self._conv_dims(x.shape, dw.shape, stride)
        assert tuple(dy.shape) == (d[0], d[4], d[5], d[6]) and x.is_contiguous() and dy.is_contiguous() and dw.is_contiguous()
        need = self.lib.sgg_conv2d_nhwc_wgrad_workspace_bytes(*d[:9])
        ws = self.workspace(need)
        flops = 2.0 * d[0] * d[4] * d[5] * d[6] * d[7] * d[8] * d[3]
        fmt = int(bool(x_s16)) | (int(bool(dy_s16)) << 1)
        sym, nb = "", 0.0
        if self.timing is not None:
            kernels = self._conv_symbol("sgg_conv2d_nhwc_wgrad_symbol", *d, self.conv_precision, 0 if self.conv_halo else 1, ln is not None,
                                        fmt, None, name="sgg_conv2d_nhwc_wgrad")
            sym = next(label for prefix, label in WGRAD_LABELS if kernels.startswith(prefix))
        if d[3] != 3:
            amax_x, amax_dy = self._amax_or_compute(x, amax_x, 0), self._amax_or_compute(dy, amax_dy, 1)
        else:
            nb = 4.0 * (x.numel() + dy.numel())      # conv1_1: HBM-bound
        self._check(self._timed(sym, flops, lambda: self.lib.sgg_conv2d_nhwc_wgrad(
            _p(x), _p(dy), _p(dw), *d, self.conv_precision, 0 if self.conv_halo else 1, _p(amax_x), _p(amax_dy), _p(ln_s), _p(ln_g), _p(ln_b),
            fmt, _p(ws), ws.numel(), self._stream()), nb),
            "sgg_conv2d_nhwc_wgrad")

    @staticmethod
    def _region(region, H, W):
        """(y0, x0, Hv, Wv) valid region of the H x W plane -> the C ABI's (W, y0, x0, Hv, Wv); W = 0: everything is valid."""
        if region is None:
            return (0, 0, 0, 0, 0)
        y0, x0, hv, wv = region
        assert 0 <= y0 and 0 <= x0 and y0 + hv <= H and x0 + wv <= W, (region, H, W)
        return (W, y0, x0, hv, wv)

    def ln_elu_fwd(self, y, gamma, beta, a, stats, amax_out=None, tile_stats=None, region=None, out_s16=False):
        """tile_stats [B, n, 4]: per-tile (count, mean, M2, max dev) written by conv_fwd's epilogue (skips the statistics pass).
        region (y0, x0, Hv, Wv): LayerNorm over that window of every sample only; `a` is written as zeros outside it.
        out_s16: `a` is written pre-split for the consuming convolutions (include/sgg_hip.h, out_format 1); amax_out (zeroed by the
        caller) then receives an upper bound of max|a|."""
        self._dev(y, gamma, beta, a, stats, amax_out, tile_stats)
        B, H, W, C = y.shape
        assert region is None or tile_stats is None
        need = self.lib.sgg_layernorm_hwc_elu_workspace_bytes(B, H * W, C)
        ws = self.workspace(need)
        nts = 0 if tile_stats is None else tile_stats.shape[1]
        # algorithmic bytes: read y (twice without epilogue statistics: statistics pass + apply pass), write a
        nb = 4.0 * y.numel() * (2 if nts else 3)
        self._check(self._timed("ln_elu_fwd(call)", 0.0, lambda: self.lib.sgg_layernorm_hwc_elu_fwd(
            _p(y), _p(gamma), _p(beta), _p(a), _p(stats), _p(amax_out), _p(tile_stats), nts, B, H * W, C,
            *self._region(region, H, W), int(bool(out_s16)), _p(ws), ws.numel(), self._stream()), nb), "sgg_layernorm_hwc_elu_fwd")

    def ln_finalize(self, tile_stats, gamma, beta, stats, amax_out, hw):
        """Statistics only: stats [B,2] = (mean, rstd) from the conv epilogue's tile partials [B,n,4]; amax_out (1 word, may be None)
        is max-ed with an upper bound of max|ELU(LN(y))|.  For consumers with an LN prologue (conv_fwd / conv_wgrad ln=...)."""
        self._dev(tile_stats, gamma, beta, stats, amax_out)
        B, nts, _ = tile_stats.shape
        self._check(self.lib.sgg_layernorm_hwc_finalize(_p(tile_stats), nts, _p(gamma), _p(beta), _p(stats), _p(amax_out), B, hw,
                                                        gamma.shape[0], self._stream()), "sgg_layernorm_hwc_finalize")

    def ln_prologue_ok(self, k, stride, H, W, cin, cout):
        """True if conv_fwd AND conv_wgrad of this layer can apply the producing layer's LayerNorm + ELU themselves
        (halo-resident kernels of the split modes: 3x3 stride 1, and conv1_3 - forward through the space-to-depth view, wgrad in
        its four parity-class launches; the C ABI rejects the prologue elsewhere)."""
        if not (self.conv_halo and self.conv_precision in (2, 3) and cin <= 512):
            return False
        if self.lib.sgg_conv_wsplit_layout(k, k, stride, H, W, cin, cout, self.conv_precision) not in (1, 2, 3, 4):
            return False
        # the filter gradient: does the library route the launch with an LN prologue?  (one sample: short of the 2 GiB tensor limits the family does not depend on the batch)
        (Ho, pad_t, _), (Wo, pad_l, _) = same_pads(H, k, stride), same_pads(W, k, stride)
        return self.lib.sgg_conv2d_nhwc_wgrad_symbol(1, H, W, cin, Ho, Wo, cout, k, k, stride, pad_t, pad_l, self.conv_precision, 0, 1, 0,
                                                     None, ctypes.create_string_buffer(256), 256) == 0

    def ln_prologue_fwd_ok(self, k, stride, H, W, cin, cout):
        """True if conv_fwd of this layer can apply the producing layer's LayerNorm + ELU itself (forward-only passes): the
        resident kernels (halo incl. conv1_3 through the space-to-depth view, band-resident 5x5 stride 2)."""
        return (self.conv_halo and self.conv_precision in (2, 3) and cin <= 512 and
                self.lib.sgg_conv_wsplit_layout(k, k, stride, H, W, cin, cout, self.conv_precision) in (1, 2, 3, 4))

    def ln_elu_bwd_sums(self, y, da, gamma, beta, stats, means, ws):
        """The reduction half of ln_elu_bwd (partial sums into the layer's own workspace `ws` for ln_bwd_finalize) + the two per-sample
        means [B,2] of the backward, WITHOUT the apply pass: the consumer computes dy itself (conv_c3_wgrad_ln)."""
        self._dev(y, da, gamma, beta, stats, means, ws)
        B, H, W, C = y.shape
        nb = 4.0 * 2 * y.numel()
        self._check(self._timed("ln_elu_bwd_sums(call)", 0.0, lambda: self.lib.sgg_layernorm_hwc_elu_bwd_sums(
            _p(y), _p(da), _p(gamma), _p(beta), _p(stats), _p(means), None, None, None, B, H * W, C, _p(ws), ws.numel(), self._stream()), nb),
            "sgg_layernorm_hwc_elu_bwd_sums")

    def conv_c3_wgrad_ln(self, x, y, da, gamma, beta, stats, means, dw):
        """conv1_1's filter gradient with dy = LayerNormBackward(y, da) computed inside the kernel (include/sgg_hip.h)."""
        self._dev(x, y, da, gamma, beta, stats, means, dw)
        B, H, W, _ = x.shape
        assert tuple(y.shape) == (B, H, W, 32) and tuple(da.shape) == (B, H, W, 32) and tuple(dw.shape) == (3, 3, 3, 32)
        assert x.is_contiguous() and y.is_contiguous() and da.is_contiguous() and dw.is_contiguous()
        need = self.lib.sgg_conv2d_nhwc_wgrad_workspace_bytes(B, H, W, 3, H, W, 32, 3, 3)
        ws = self.workspace(need)
        flops = 2.0 * B * H * W * 32 * 27
        nb = 4.0 * (x.numel() + y.numel() + da.numel())
        self._check(self._timed("conv_c3_wgrad_ln(call: LN-backward apply fused + slab reduce)", flops, lambda: self.lib.sgg_conv2d_nhwc_wgrad_c3_ln(
            _p(x), _p(y), _p(da), _p(gamma), _p(beta), _p(stats), _p(means), _p(dw), B, H, W, 1, 1, _p(ws), ws.numel(), self._stream()), nb),
            "sgg_conv2d_nhwc_wgrad_c3_ln")

    def conv_c3_dgrad(self, dy, w_hwio, dx):
        """conv1_1's input gradient: dx [B,H,W,3] = Conv2DBackpropInput(dy [B,H,W,32], w [3,3,3,32]), 3x3 stride 1 SAME, exact f32."""
        self._dev(dy, w_hwio, dx)
        B, H, W, _ = dx.shape
        if tuple(dy.shape) != (B, H, W, 32) or tuple(w_hwio.shape) != (3, 3, 3, 32) or tuple(dx.shape) != (B, H, W, 3):
            raise SggError("conv_c3_dgrad: shapes dy %s, w %s, dx %s (want [B,H,W,32], [3,3,3,32], [B,H,W,3])"
                           % (tuple(dy.shape), tuple(w_hwio.shape), tuple(dx.shape)))
        assert dy.is_contiguous() and w_hwio.is_contiguous() and dx.is_contiguous()
        flops = 2.0 * B * H * W * 32 * 27
        nb = 4.0 * (dy.numel() + dx.numel())
        self._check(self._timed("conv_c3_dgrad_kernel<false>", flops, lambda: self.lib.sgg_conv2d_nhwc_dgrad_c3(
            _p(dy), _p(w_hwio), _p(dx), B, H, W, 1, 1, self._stream()), nb), "sgg_conv2d_nhwc_dgrad_c3")

    def conv_c3_dgrad_ln(self, y, da, gamma, beta, stats, means, w_hwio, dx):
        """conv_c3_dgrad with dy = LayerNormBackward(y, da) computed inside the kernel (means from ln_elu_bwd_sums; include/sgg_hip.h)."""
        self._dev(y, da, gamma, beta, stats, means, w_hwio, dx)
        B, H, W, _ = dx.shape
        if (tuple(y.shape) != (B, H, W, 32) or tuple(da.shape) != (B, H, W, 32) or tuple(w_hwio.shape) != (3, 3, 3, 32)
                or tuple(dx.shape) != (B, H, W, 3) or tuple(stats.shape) != (B, 2) or tuple(means.shape) != (B, 2)):
            raise SggError("conv_c3_dgrad_ln: shapes y %s, da %s, stats %s, means %s, w %s, dx %s" % tuple(
                tuple(t.shape) for t in (y, da, stats, means, w_hwio, dx)))
        assert all(t.is_contiguous() for t in (y, da, gamma, beta, stats, means, w_hwio, dx))
        flops = 2.0 * B * H * W * 32 * 27
        nb = 4.0 * (y.numel() + da.numel() + dx.numel())
        self._check(self._timed("conv_c3_dgrad_kernel<true>", flops, lambda: self.lib.sgg_conv2d_nhwc_dgrad_c3_ln(
            _p(y), _p(da), _p(gamma), _p(beta), _p(stats), _p(means), _p(w_hwio), _p(dx), B, H, W, 1, 1, self._stream()), nb),
            "sgg_conv2d_nhwc_dgrad_c3_ln")

    def ln_workspace_bytes(self, shape):
        B, H, W, C = shape
        return self.lib.sgg_layernorm_hwc_elu_workspace_bytes(B, H * W, C)

    def ln_finalize_descs(self, layers):
        """layers: dicts with ws (the layer's own workspace), gamma, stats, dgamma, dbeta, dbias, shape (B, H, W, C), region ->
        ctypes array for ln_bwd_finalize (the tensors must stay alive and in place)."""
        arr = (LnFinalizeDesc * len(layers))()
        for d, lay in zip(arr, layers):
            B, H, W, C = lay["shape"]
            self._dev(lay["ws"], lay["gamma"], lay["stats"], lay["dgamma"], lay["dbeta"], lay.get("dbias"))
            d.workspace, d.gamma, d.stats = _p(lay["ws"]), _p(lay["gamma"]), _p(lay["stats"])
            d.dgamma, d.dbeta, d.dbias_prev = _p(lay["dgamma"]), _p(lay["dbeta"]), _p(lay.get("dbias"))
            d.B, d.HW, d.C = B, H * W, C
            d.HW_valid = H * W if lay.get("region") is None else lay["region"][2] * lay["region"][3]
        return arr

    def ln_bwd_finalize(self, descs):
        """dgamma, dbeta and the producing convolutions' bias gradients of several LayerNorms whose ln_elu_bwd ran with
        deferred reductions (dgamma=None, ws=...): one launch (sgg_layernorm_hwc_bwd_finalize)."""
        self._check(self.lib.sgg_layernorm_hwc_bwd_finalize(ctypes.addressof(descs), len(descs), self._stream()),
                    "sgg_layernorm_hwc_bwd_finalize")

    def ln_elu_bwd(self, y, da, gamma, beta, stats, dy, dgamma, dbeta, dbias_prev, amax_out=None, region=None, ws=None, out_s16=False,
                   pq=None):
        """dgamma = dbeta = None with a workspace `ws` of the layer's own: the parameter-gradient reductions are deferred to
        ln_bwd_finalize.  out_s16: dy is written pre-split (amax_out receives an upper bound of max|dy|); pq: two ZEROED words for
        the maxima that bound is made of (default: a pair zeroed here - one more launch)."""
        self._dev(y, da, gamma, beta, stats, dy, dgamma, dbeta, dbias_prev, amax_out, ws)
        B, H, W, C = y.shape
        need = self.lib.sgg_layernorm_hwc_elu_workspace_bytes(B, H * W, C)
        assert (dgamma is None) == (dbeta is None) and (dgamma is not None or ws is not None)
        if ws is None:
            ws = self.workspace(need)
        if out_s16 and pq is None:
            pq = torch.zeros(2, dtype=torch.float32, device=y.device)
        self._dev(pq)
        assert ws.numel() * ws.element_size() >= need
        # bytes: the reduction reads y and da, the apply pass reads them again and writes dy
        self._check(self._timed("ln_elu_bwd(call)", 0.0, lambda: self.lib.sgg_layernorm_hwc_elu_bwd(
            _p(y), _p(da), _p(gamma), _p(beta), _p(stats), _p(dy), _p(dgamma), _p(dbeta), _p(dbias_prev), _p(amax_out), B, H * W, C,
            *self._region(region, H, W), int(bool(out_s16)), _p(pq), _p(ws), ws.numel() * ws.element_size(), self._stream()), 4.0 * y.numel() * 5),
            "sgg_layernorm_hwc_elu_bwd")

    # -- heads -----------------------------------------------------------------------------------------
    def spatial_mean_fwd(self, ctx, out_c, out_h):
        """ctx [B,L,C]; out_c / out_h: [R,C] (strided) views; row r gets mean_l ctx[r % B]."""
        self._dev(ctx, out_c, out_h)
        B, L, C = ctx.shape
        R = out_c.shape[0]
        self._check(self.lib.sgg_spatial_mean_fwd(_p(ctx), _p(out_c), _ld(out_c), _p(out_h), _ld(out_h), R, B, L, C,
                                                  self._stream()), "sgg_spatial_mean_fwd")

    def spatial_mean_bwd(self, dc0, dh0, dctx, accumulate):
        self._dev(dc0, dh0, dctx)
        B, L, C = dctx.shape
        R = dc0.shape[0]
        self._check(self.lib.sgg_spatial_mean_bwd(_p(dc0), _ld(dc0), _p(dh0), _ld(dh0), _p(dctx), R, B, L, C,
                                                  int(accumulate), self._stream()), "sgg_spatial_mean_bwd")

    def _gemm(self, mode, M, N, K, A, Bm, C, bias, accumulate):
        self._dev(A, Bm, C, bias)
        assert A.stride(1) == 1 and Bm.stride(1) == 1 and C.stride(1) == 1
        need = self.lib.sgg_gemm_workspace_bytes(M, N, K)
        ws = self.workspace(need)
        if mode == 0:
            rc = self.lib.sgg_gemm_skinny_fwd(M, N, K, _p(A), _ld(A), _p(Bm), _ld(Bm), _p(C), _ld(C), _p(bias),
                                              int(accumulate), _p(ws), ws.numel(), self._stream())
        else:
            fn = self.lib.sgg_gemm_skinny_dgrad if mode == 1 else self.lib.sgg_gemm_skinny_wgrad
            rc = fn(M, N, K, _p(A), _ld(A), _p(Bm), _ld(Bm), _p(C), _ld(C), int(accumulate), _p(ws), ws.numel(),
                    self._stream())
        self._check(rc, ("sgg_gemm_skinny_fwd", "sgg_gemm_skinny_dgrad", "sgg_gemm_skinny_wgrad")[mode])

    def _head_symbol(self, query, *args):
        """The kernels of a head launch, in launch order and separated by ';', as the library's own routing reports them
        (sgg_gemm_skinny_symbol / sgg_attn_step_fwd_symbol / _bwd_symbol: the launch's validation and route, scalars only)."""
        buf = ctypes.create_string_buffer(96)
        self._check(getattr(self.lib, query)(*args, buf, len(buf)), query)
        return buf.value.decode()

    def gemm_symbol(self, mode, M, N, K):
        """(kernels, nsplit) of sgg_gemm_skinny_{fwd, dgrad, wgrad}[mode](M, N, K)."""
        ns = c_int(0)
        return self._head_symbol("sgg_gemm_skinny_symbol", mode, M, N, K, ctypes.addressof(ns)), ns.value

    def attn_step_fwd_symbol(self, R, B, L, C, dual):
        return self._head_symbol("sgg_attn_step_fwd_symbol", R, B, L, C, int(dual))

    def attn_step_bwd_symbol(self, R, B, L, C, dual):
        return self._head_symbol("sgg_attn_step_bwd_symbol", R, B, L, C, int(dual))

    def gemm_nn(self, A, Bm, C, bias=None, accumulate=False):
        """C[M,N] (+)= A[M,K] @ B[K,N] (+ bias)"""
        M, K = A.shape
        K2, N = Bm.shape
        assert K == K2 and tuple(C.shape) == (M, N)
        self._gemm(0, M, N, K, A, Bm, C, bias, accumulate)

    def gemm_nt(self, A, Bm, C, accumulate=False):
        """C[M,N] (+)= A[M,K] @ B[N,K]^T"""
        M, K = A.shape
        N, K2 = Bm.shape
        assert K == K2 and tuple(C.shape) == (M, N)
        self._gemm(1, M, N, K, A, Bm, C, None, accumulate)

    def gemm_tn(self, A, Bm, C, accumulate=False):
        """C[M,N] (+)= A[K,M]^T @ B[K,N]"""
        K, M = A.shape
        K2, N = Bm.shape
        assert K == K2 and tuple(C.shape) == (M, N)
        self._gemm(2, M, N, K, A, Bm, C, None, accumulate)

    def attn_ctx_fwd(self, ctx_flat, W_ctx, bias, P):
        """P[B,L] = ctx_flat[B,L*C] @ W_ctx[L*C,L] + bias: the step-invariant part of the attention perceptron."""
        self._dev(ctx_flat, W_ctx, bias, P)
        B, LC = ctx_flat.shape
        L = P.shape[1]
        assert ctx_flat.is_contiguous() and W_ctx.is_contiguous() and P.is_contiguous() and tuple(W_ctx.shape) == (LC, L)
        ws = self.workspace(self.lib.sgg_gemm_workspace_bytes(B, L, LC))
        nb = 4.0 * (LC * L + B * LC + B * L)       # W_ctx streamed once + ctx + P
        self._check(self._timed("attn_ctx_gemm_fwd(call: split-K gemm + reduce)", 2.0 * B * L * LC, lambda: self.lib.sgg_attn_ctx_gemm_fwd(
            B, L, LC, _p(ctx_flat), _p(W_ctx), _p(bias), _p(P), _p(ws), ws.numel(), self._stream()), nb), "sgg_attn_ctx_gemm_fwd")

    def attn_ctx_dgrad(self, dP, W_ctx, dctx_flat, accumulate=True):
        self._dev(dP, W_ctx, dctx_flat)
        B, L = dP.shape
        LC = W_ctx.shape[0]
        assert dP.is_contiguous() and W_ctx.is_contiguous() and dctx_flat.is_contiguous()
        ws = self.workspace(self.lib.sgg_gemm_workspace_bytes(B, LC, L))
        nb = 4.0 * (LC * L + B * L + B * LC * (2 if accumulate else 1))
        self._check(self._timed("attn_ctx_gemm_dgrad(call)", 2.0 * B * L * LC, lambda: self.lib.sgg_attn_ctx_gemm_dgrad(
            B, L, LC, _p(dP), _p(W_ctx), _p(dctx_flat), int(accumulate), _p(ws), ws.numel(), self._stream()), nb),
            "sgg_attn_ctx_gemm_dgrad")

    def attn_ctx_wgrad(self, ctx_flat, dP, dW_ctx, accumulate=True):
        self._dev(ctx_flat, dP, dW_ctx)
        B, LC = ctx_flat.shape
        L = dP.shape[1]
        assert ctx_flat.is_contiguous() and dP.is_contiguous() and dW_ctx.is_contiguous()
        ws = self.workspace(self.lib.sgg_gemm_workspace_bytes(LC, L, B))
        nb = 4.0 * (LC * L * (2 if accumulate else 1) + B * L + B * LC)
        self._check(self._timed("attn_ctx_gemm_wgrad(call)", 2.0 * B * L * LC, lambda: self.lib.sgg_attn_ctx_gemm_wgrad(
            B, L, LC, _p(ctx_flat), _p(dP), _p(dW_ctx), int(accumulate), _p(ws), ws.numel(), self._stream()), nb),
            "sgg_attn_ctx_gemm_wgrad")

    @staticmethod
    def _planes(t):
        """[np, R, W] (strided) -> (ptr_real, ptr_dual or None, ld)"""
        if t is None:
            return None, None, 0
        assert t.dim() == 3 and t.stride(2) == 1
        ld = t.stride(1) if t.shape[1] > 1 else max(t.stride(1), t.shape[2])
        return t[0].data_ptr(), (t[1].data_ptr() if t.shape[0] == 2 else None), ld

    def attn_step_fwd(self, P, ec, ctx, alpha, z):
        """P [B,L]; ec, alpha [np,R,L]; z [np,R,C] view; ctx [B,L,C]."""
        self._dev(P, ec, ctx, alpha, z)
        B, L, C = ctx.shape
        R = ec.shape[1]
        er, ed, lde = self._planes(ec)
        ar, ad, lda = self._planes(alpha)
        zr, zd, ldz = self._planes(z)
        assert lda == L
        np_ = ec.shape[0]
        nb = 4.0 * (B * L * C + B * L + np_ * R * (2 * L + C))     # feature map once per image + P + ec, alpha, z
        self._check(self._timed("attn_step_fwd_kernel<%s>" % ("Dual" if np_ == 2 else "float"), 0.0, lambda: self.lib.sgg_attn_step_fwd(
            _p(P), er, ed, lde, _p(ctx), ar, ad, zr, zd, ldz, R, B, L, C, self._stream()), nb), "sgg_attn_step_fwd")

    def attn_step_bwd(self, ctx, alpha, dz, de, dP, dctx, accumulate):
        self._dev(ctx, alpha, dz, de, dP, dctx)
        B, L, C = ctx.shape
        R = alpha.shape[1]
        ar, ad, lda = self._planes(alpha)
        zr, zd, ldz = self._planes(dz)
        er, ed, lde = self._planes(de)
        assert lda == L and lde == L
        np_ = alpha.shape[0]
        nb = 4.0 * (B * L * C * (3 if accumulate else 2) + B * L * 2 + np_ * R * (2 * L + C))   # ctx read, dctx read+write
        self._check(self._timed("attn_step_bwd(call)<%s>" % ("Dual" if np_ == 2 else "float"), 0.0, lambda: self.lib.sgg_attn_step_bwd(
            _p(ctx), ar, ad, zr, zd, ldz, er, ed, _p(dP), _p(dctx), R, B, L, C, int(accumulate), self._stream()), nb),
            "sgg_attn_step_bwd")

    def lstm_fwd(self, gates, c_prev, ln_params, c_new, h_new):
        """gates [np,R,2048], c_prev/c_new [np,R,512] contiguous, h_new [np,R,512] view, ln_params [10,512]."""
        self._dev(gates, c_prev, ln_params, c_new, h_new)
        R = gates.shape[1]
        gr, gd, ldg = self._planes(gates)
        cr, cd, ldc = self._planes(c_prev)
        nr, nd, ldn = self._planes(c_new)
        hr, hd, ldh = self._planes(h_new)
        assert ldg == 2048 and ldc == 512 and ldn == 512
        np_ = gates.shape[0]
        nb = 4.0 * (np_ * R * (2048 + 512 + 1024) + 10 * 512)     # gates + c in, c', h' out (+ the LN vectors)
        self._check(self._timed("lnlstm_gates_fwd_kernel<%s>" % ("Dual" if np_ == 2 else "float"), 0.0, lambda: self.lib.sgg_lnlstm_gates_fwd(
            gr, gd, cr, cd, _p(ln_params), nr, nd, hr, hd, ldh, R, self._stream()), nb), "sgg_lnlstm_gates_fwd")

    def lstm_bwd(self, gates, c_prev, ln_params, dh, dc_new, dgates, dc_prev, pgrad):
        """dh [np,R,512] view; dc_new [np,R,512] or None; outputs dgates [np,R,2048], dc_prev [np,R,512], pgrad [R,10,512]."""
        self._dev(gates, c_prev, ln_params, dh, dc_new, dgates, dc_prev, pgrad)
        R = gates.shape[1]
        gr, gd, ldg = self._planes(gates)
        cr, cd, ldc = self._planes(c_prev)
        hr, hd, ldh = self._planes(dh)
        nr, nd, ldn = self._planes(dc_new)
        dgr, dgd, lddg = self._planes(dgates)
        dpr, dpd, lddp = self._planes(dc_prev)
        assert ldg == 2048 and ldc == 512 and lddg == 2048 and lddp == 512 and (dc_new is None or ldn == 512)
        np_ = gates.shape[0]
        nb = 4.0 * (np_ * R * (2048 + 512 + 512 + (512 if dc_new is not None else 0) + 2048 + 512) + R * 5120 + 5120)
        self._check(self._timed("lnlstm_gates_bwd_kernel<%s>" % ("Dual" if np_ == 2 else "float"), 0.0, lambda: self.lib.sgg_lnlstm_gates_bwd(
            gr, gd, cr, cd, _p(ln_params), hr, hd, ldh, nr, nd, dgr, dgd, dpr, dpd, _p(pgrad), R, self._stream()), nb),
            "sgg_lnlstm_gates_bwd")

    def colsum(self, X, out, accumulate=False):
        self._dev(X, out)
        rows, cols = X.shape
        assert X.stride(1) == 1
        ws = self.workspace(self.lib.sgg_colsum_workspace_bytes(rows, cols))
        self._check(self.lib.sgg_colsum(_p(X), rows, cols, _ld(X), _p(out), int(accumulate), _p(ws), ws.numel(), self._stream()),
                    "sgg_colsum")

    # -- loss / optimiser / misc -----------------------------------------------------------------------
    def onehot(self, labels, out):
        self._dev(labels, out)
        assert labels.dtype == torch.int64 and labels.is_contiguous() and out.is_contiguous()
        V = out.shape[-1]
        self._check(self.lib.sgg_onehot(_p(labels), _p(out), labels.numel(), V, self._stream()), "sgg_onehot")

    def embed_gather_fwd(self, labels, W, out):
        """labels: int64 [R] (strided) view; W [V,E]; out [R,E] view: out[r] = W[labels[r]] (tf.matmul(one_hot, W))."""
        self._dev(labels, W, out)
        assert labels.dtype == torch.int64 and labels.dim() == 1 and W.is_contiguous() and out.stride(1) == 1
        V, E = W.shape
        R = labels.shape[0]
        self._check(self.lib.sgg_embed_gather_fwd(_p(labels), max(labels.stride(0), 1), _p(W), V, E, _p(out), _ld(out), R,
                                                  self._stream()), "sgg_embed_gather_fwd")

    def embed_gather_bwd(self, labels, dY, dW):
        """dW[labels[r]] += dY[r] (deterministic)."""
        self._dev(labels, dY, dW)
        assert labels.dtype == torch.int64 and labels.dim() == 1 and dW.is_contiguous() and dY.stride(1) == 1
        V, E = dW.shape
        R = labels.shape[0]
        self._check(self.lib.sgg_embed_gather_bwd(_p(labels), max(labels.stride(0), 1), _p(dY), _ld(dY), _p(dW), V, E, R,
                                                  self._stream()), "sgg_embed_gather_bwd")

    def resize_bilinear_tf1(self, packed, offsets, heights, widths, out, means, stds):
        """packed uint8 [nbytes] (RGB images back to back), offsets int64 [B], heights / widths int32 [B] -> out [B,oh,ow,3] fp32 =
        (tf.image.resize_images(img, [oh, ow]) - means) / stds  (train.py:171-172)."""
        self._dev(packed, offsets, heights, widths, out, means, stds)
        assert packed.dtype == torch.uint8 and offsets.dtype == torch.int64 and heights.dtype == torch.int32 and widths.dtype == torch.int32
        B, oh, ow, _ = out.shape
        self._check(self.lib.sgg_resize_bilinear_tf1(_p(packed), _p(offsets), _p(heights), _p(widths), _p(out), B, oh, ow, _p(means),
                                                     _p(stds), self._stream()), "sgg_resize_bilinear_tf1")

    def augment_plan(self, packed, offsets, heights, widths, labels_in, swap, amplitudes_q, seed, draw0, box, factors, labels_out):
        """The augmentation table of a packed batch (include/sgg_hip.h, "training-time augmentation"): amplitudes_q = (crop, flip,
        brightness, contrast, saturation) as 16-bit fixed point, example b at stream position draw0 + b -> box int32 [B,6], factors
        fp32 [B,4], labels_out int64 [B,3] (labels_in [B,3] with mirrored examples remapped through swap int32 [V])."""
        self._dev(packed, offsets, heights, widths, labels_in, swap, box, factors, labels_out)
        assert packed.dtype == torch.uint8 and offsets.dtype == torch.int64 and heights.dtype == torch.int32 and widths.dtype == torch.int32
        assert labels_in.dtype == torch.int64 and labels_out.dtype == torch.int64 and swap.dtype == torch.int32
        assert box.dtype == torch.int32 and factors.dtype == torch.float32
        B = offsets.shape[0]
        assert labels_in.is_contiguous() and labels_out.is_contiguous() and box.is_contiguous() and factors.is_contiguous()
        assert labels_in.shape == (B, 3) and labels_out.shape == (B, 3) and box.shape == (B, 6) and factors.shape == (B, 4)
        crop_q, flip_q, bright_q, contrast_q, sat_q = (int(q) for q in amplitudes_q)
        ws, nbytes = None, 0
        if contrast_q > 0:
            nbytes = self.lib.sgg_augment_plan_workspace_bytes(B)
            ws = self.workspace(nbytes)
        self._check(self.lib.sgg_augment_plan(_p(packed), _p(offsets), _p(heights), _p(widths), _p(labels_in), _p(swap), swap.numel(), B,
                                              crop_q, flip_q, bright_q, contrast_q, sat_q, int(seed) & (2 ** 64 - 1),
                                              int(draw0) & (2 ** 64 - 1), _p(box), _p(factors), _p(labels_out), _p(ws), nbytes,
                                              self._stream()), "sgg_augment_plan")

    def augment_resize(self, packed, offsets, heights, widths, box, factors, stages, out, means, stds):
        """out [B,oh,ow,3] fp32 = the crop box of every image resized on the TF-1.x grid, mirrored where box[b,4] != 0, the colour
        stages of `stages` (bit 0 saturation, 1 contrast, 2 brightness) applied, standardised: a function of the source and the table."""
        self._dev(packed, offsets, heights, widths, box, factors, out, means, stds)
        assert packed.dtype == torch.uint8 and offsets.dtype == torch.int64 and heights.dtype == torch.int32 and widths.dtype == torch.int32
        assert box.dtype == torch.int32 and factors.dtype == torch.float32 and box.is_contiguous() and factors.is_contiguous()
        B, oh, ow, _ = out.shape
        assert out.is_contiguous() and box.shape == (B, 6) and factors.shape == (B, 4)
        self._check(self.lib.sgg_augment_resize(_p(packed), _p(offsets), _p(heights), _p(widths), _p(box), _p(factors), int(stages),
                                                _p(out), B, oh, ow, _p(means), _p(stds), self._stream()), "sgg_augment_resize")

    def interpolate(self, real, fake, alpha, out):
        self._dev(real, fake, alpha, out)
        assert real.is_contiguous() and fake.is_contiguous() and alpha.is_contiguous() and out.is_contiguous()
        B = real.shape[0]
        self._check(self.lib.sgg_interpolate(_p(real), _p(fake), _p(alpha), _p(out), B, real.numel() // B, self._stream()),
                    "sgg_interpolate")

    def gp_fwd(self, g, slopes, pen):
        self._dev(g, slopes, pen)
        assert g.is_contiguous() and slopes.is_contiguous() and pen.is_contiguous()
        B = g.shape[0]
        self._check(self.lib.sgg_wgan_gp_loss_fwd(_p(g), _p(slopes), _p(pen), B, g.numel() // B, self._stream()),
                    "sgg_wgan_gp_loss_fwd")

    def gp_bwd(self, g, slopes, pen, v, scale):
        self._dev(g, slopes, pen, v)
        assert g.is_contiguous() and slopes.is_contiguous() and pen.is_contiguous() and v.is_contiguous()
        B = g.shape[0]
        self._check(self.lib.sgg_wgan_gp_loss_bwd(_p(g), _p(slopes), _p(pen), _p(v), B, g.numel() // B, float(scale),
                                                  self._stream()), "sgg_wgan_gp_loss_bwd")

    def wgan_losses(self, d_out, pen, lam, B, T, has_real, out4):
        self._dev(d_out, pen, out4)
        assert d_out.is_contiguous() and (pen is None or pen.is_contiguous()) and out4.is_contiguous()
        self._check(self.lib.sgg_wgan_losses(_p(d_out), _p(pen), float(lam), B, T, int(has_real), _p(out4), self._stream()),
                    "sgg_wgan_losses")

    # -- the optimiser's whole-arena passes (csrc/optim.hip) --------------------------------------------
    def _adam(self, suffix, params, grads, m, v, ema, hyper, scale, one_minus_decay=None):
        """The four Adam entry points sgg_adam_tf_multi<suffix> (one kernel body, csrc/optim.hip).  scale: the gradient scale, or the
        fp64 record [8] of grad_guard that holds it (the guarded forms); ema with one_minus_decay: the forms that keep the average.
        28 n bytes, 36 n with the average."""
        arenas = (params, grads, m, v) if ema is None else (params, grads, m, v, ema)
        guarded = torch.is_tensor(scale)
        self._dev(*arenas, scale if guarded else None)
        n = params.numel()
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in arenas)
        assert not guarded or (scale.dtype == torch.float64 and tuple(scale.shape) == (8,) and scale.is_contiguous())
        args = [_p(t) for t in arenas] + [n] + [float(x) for x in hyper] + [_p(scale) if guarded else float(scale)]
        if ema is not None:
            args.append(float(one_minus_decay))
        fn = getattr(self.lib, "sgg_adam_tf_multi" + suffix)
        self._check(self._timed("adam%s_kernel" % suffix, 0.0, lambda: fn(*args, self._stream()), (28.0 if ema is None else 36.0) * n),
                    "sgg_adam_tf_multi" + suffix)

    def adam(self, params, grads, m, v, lr_t, b1, b2, eps, grad_scale=1.0):
        self._adam("", params, grads, m, v, None, (lr_t, b1, b2, eps), grad_scale)

    def adam_ema(self, params, grads, m, v, ema, lr_t, b1, b2, eps, grad_scale=1.0, one_minus_decay=0.0):
        """adam() and, in the same pass, ema -= (ema - params_new) * one_minus_decay (include/sgg_hip.h): params, m and v
        bit-identical to adam().  ema: fp32, as long as params, overlapping none of the other operands."""
        self._adam("_ema", params, grads, m, v, ema, (lr_t, b1, b2, eps), grad_scale, one_minus_decay)

    def adam_guarded(self, params, grads, m, v, lr_t, b1, b2, eps, record):
        """adam() with the gradient scale (float)record[4] read on the device, or nothing at all where record[5] == 0 (the record of
        grad_guard, below)."""
        assert torch.is_tensor(record)
        self._adam("_guarded", params, grads, m, v, None, (lr_t, b1, b2, eps), record)

    def adam_ema_guarded(self, params, grads, m, v, ema, lr_t, b1, b2, eps, record, one_minus_decay=0.0):
        """adam_ema() with the gradient scale (float)record[4] read on the device, or nothing at all where record[5] == 0."""
        assert torch.is_tensor(record)
        self._adam("_ema_guarded", params, grads, m, v, ema, (lr_t, b1, b2, eps), record, one_minus_decay)

    def swap(self, a, b):
        """Exchange the contents of two fp32 ranges of equal length bit for bit."""
        self._dev(a, b)
        n = a.numel()
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in (a, b))
        self._check(self._timed("swap_kernel", 0.0, lambda: self.lib.sgg_swap_f32(_p(a), _p(b), n, self._stream()), 16.0 * n),
                    "sgg_swap_f32")

    def grad_accumulate(self, acc, g, first=False):
        """acc = g (first) or acc += g, one fp32 addition per element: the pass of gradient accumulation."""
        self._dev(acc, g)
        n = acc.numel()
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in (acc, g))
        self._check(self._timed("grad_accumulate_kernel", 0.0, lambda: self.lib.sgg_grad_accumulate(
            _p(acc), _p(g), n, int(bool(first)), self._stream()), (8.0 if first else 12.0) * n), "sgg_grad_accumulate")

    # -- guarded updates: the decision (csrc/guard.hip, sgg_amd/guard.py); adam_guarded / adam_ema_guarded above read it ----------
    def grad_guard_workspace_bytes(self, n):
        return int(self.lib.sgg_grad_guard_workspace_bytes(int(n)))

    def grad_guard(self, grads, record, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False, ws=None, grid=0):
        """The decision of a guarded update (include/sgg_hip.h): the global norm and non-finite count of grads * grad_scale into the
        persistent fp64 record [8] (zero-filled once by the caller; sgg_amd.guard.FIELDS), which the guarded Adam passes read on the
        same stream.  ws: a uint8 buffer of grad_guard_workspace_bytes(n) (default: the stream's scratch buffer).  grid: workgroups
        of the first launch (0 = default); the record does not depend on it.  Reads grads only."""
        self._dev(grads, record, ws)
        n = grads.numel()
        assert grads.dtype == torch.float32 and grads.is_contiguous()
        assert record.dtype == torch.float64 and tuple(record.shape) == (8,) and record.is_contiguous()
        if ws is None:
            ws = self.workspace(self.grad_guard_workspace_bytes(n))
        self._check(self._timed("grad_guard(call: chunk rows + record)", 0.0, lambda: self.lib.sgg_grad_guard(
            _p(grads), n, float(grad_scale), float(max_norm), int(bool(skip_nonfinite)), int(grid), _p(ws),
            ws.numel() * ws.element_size(), _p(record), self._stream()), 4.0 * n), "sgg_grad_guard")
        return record

    # -- training diagnostics (csrc/stats.hip) ---------------------------------------------------------
    def arena_stats_chunk(self):
        """Elements per chunk of arena_stats' chunk table (a compile-time constant of the library; sgg_amd.diagnostics.CHUNK)."""
        return int(self.lib.sgg_arena_stats_chunk())

    def arena_stats_nstat(self):
        return int(self.lib.sgg_arena_stats_nstat())

    def arena_stats_workspace_bytes(self, n_chunks):
        return int(self.lib.sgg_arena_stats_workspace_bytes(int(n_chunks)))

    def arena_stats(self, params, grads, m, v, table, n_tensors, lr_t, eps, grad_scale=1.0, out=None, ws=None, grid=0):
        """Per-tensor statistics of the four arenas in one pass (include/sgg_hip.h): table int64 [n_chunks, 3] on the device
        (sgg_amd.diagnostics.chunk_table; the caller has checked it against the arenas' length, diagnostics.check_table), out fp64
        [n_tensors, 9] (default: a new tensor), ws: a uint8 buffer of arena_stats_workspace_bytes(n_chunks) (default: the stream's
        scratch buffer).  grid: workgroups of the first launch (0 = default); the result does not depend on it.  Reads only."""
        self._dev(params, grads, m, v, table, out, ws)
        n = params.numel()
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n for t in (params, grads, m, v)) and n % 4 == 0
        assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 3 and table.is_contiguous()
        n_chunks, ns = int(table.shape[0]), self.arena_stats_nstat()
        if out is None:
            out = torch.empty((n_tensors, ns), dtype=torch.float64, device=params.device)
        assert out.dtype == torch.float64 and tuple(out.shape) == (n_tensors, ns) and out.is_contiguous()
        if ws is None:
            ws = self.workspace(self.arena_stats_workspace_bytes(n_chunks))
        self._check(self._timed("arena_stats(call: chunk rows + per-tensor sum)", 0.0, lambda: self.lib.sgg_arena_stats(
            _p(params), _p(grads), _p(m), _p(v), _p(table), n_chunks, int(n_tensors), float(lr_t), float(eps), float(grad_scale),
            int(grid), _p(ws), ws.numel() * ws.element_size(), _p(out), self._stream()), 16.0 * n), "sgg_arena_stats")
        return out

    def vector_stats(self, x, threshold, out=None):
        """out fp64 [5] = (min, max, sum, count above `threshold`) over the finite elements of the fp32 vector x, and its non-finite
        count (include/sgg_hip.h); one workgroup."""
        self._dev(x, out)
        assert x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous()
        if out is None:
            out = torch.empty((5,), dtype=torch.float64, device=x.device)
        assert out.dtype == torch.float64 and tuple(out.shape) == (5,) and out.is_contiguous()
        self._check(self._timed("vector_stats_kernel", 0.0, lambda: self.lib.sgg_vector_stats(
            _p(x), x.numel(), float(threshold), _p(out), self._stream()), 4.0 * x.numel()), "sgg_vector_stats")
        return out

    def argmax_rows(self, x, out):
        """out[r] = the first index of the maximum over the non-NaN entries of row r of x [..., V] (rows may be strided); a NaN entry is
        never selected, a row without a non-NaN entry gives 0: every token is in [0, V) (oracle.sgg_oracle.argmax_tokens)."""
        self._dev(x, out)
        assert x.stride(-1) == 1 and out.dtype == torch.int64
        V = x.shape[-1]
        x2 = x.reshape(-1, V)
        self._check(self.lib.sgg_argmax_rows(_p(x2), _p(out), x2.shape[0], V, _ld(x2), self._stream()), "sgg_argmax_rows")

    def rank_triples(self, tokens, d, K, descending=False, want_sample_scores=False, vocab=None, out=None):
        """The ranked DISTINCT triples of every image (csrc/rank.hip): tokens int64 [N, nb, 3] (sample k of image j at [k, j]), d
        [N, nb, 3] or [N, nb, 3, 1] critic outputs -> dict of new device tensors: triples int64 [nb, K, 3], scores [nb, K],
        first_rank / first_sample / counts int32 [nb, K], n_distinct int32 [nb] and, on request, sample_scores [nb, N].  Score =
        fp32 mean of the three outputs; ascending (descending=True: descending), ties by sample index, NaN last; slots behind
        n_distinct hold -1 / NaN / -1 / -1 / 0.  vocab: the vocabulary size (every token in [0, vocab); default: the library's
        limit, 2^21).  out: optional dict of preallocated contiguous tensors under those names."""
        self._dev(tokens, d)
        assert tokens.dtype == torch.int64 and tokens.dim() == 3 and tokens.shape[2] == 3 and tokens.is_contiguous()
        N, nb = int(tokens.shape[0]), int(tokens.shape[1])
        assert d.dtype == torch.float32 and d.numel() == N * nb * 3 and d.is_contiguous(), "d must be contiguous [N, nb, 3]"
        K, V = max(int(K), 0), (1 << 21) if vocab is None else int(vocab)
        spec = {"triples": ((nb, K, 3), torch.int64), "scores": ((nb, K), torch.float32), "first_rank": ((nb, K), torch.int32),
                "first_sample": ((nb, K), torch.int32), "counts": ((nb, K), torch.int32), "n_distinct": ((nb,), torch.int32)}
        if want_sample_scores:
            spec["sample_scores"] = ((nb, N), torch.float32)
        res = {}
        for name, (shape, dtype) in spec.items():
            t = out[name] if out is not None else torch.empty(shape, dtype=dtype, device=tokens.device)
            self._dev(t)
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
            res[name] = t
        self._check(self.lib.sgg_rank_triples(_p(tokens), _p(d), N, nb, V, K, int(bool(descending)),
                                              _p(res["triples"]), _p(res["scores"]), _p(res["first_rank"]), _p(res["first_sample"]),
                                              _p(res["counts"]), _p(res["n_distinct"]), _p(res.get("sample_scores")),
                                              self._stream()), "sgg_rank_triples")
        return res

    def match_triples(self, ranked, n_distinct, gt, gt_count, vocab=None, out=None):
        """Where every ground-truth triple stands in its image's ranked distinct list (csrc/match.hip): ranked int64 [nb, K, 3] and
        n_distinct int32 [nb] (rank_triples' outputs), gt int64 [nb, M, 3], gt_count int32 [nb] (rows m >= gt_count[j] are padding)
        -> {"pos": int32 [nb, M], "n_gt": int32 [nb]}.  pos: the slot u >= 0 of the list that equals the row, -1 absent, -2
        duplicate of an earlier row of the image, -3 padding, -4 a token outside [0, vocab); n_gt: rows with pos >= -1.  vocab:
        default the library's limit, 2^21.  out: optional dict of preallocated contiguous tensors under those names."""
        self._dev(ranked, n_distinct, gt, gt_count)
        assert ranked.dtype == torch.int64 and ranked.dim() == 3 and ranked.shape[2] == 3 and ranked.is_contiguous()
        nb, K = int(ranked.shape[0]), int(ranked.shape[1])
        assert gt.dtype == torch.int64 and gt.dim() == 3 and gt.shape[0] == nb and gt.shape[2] == 3 and gt.is_contiguous()
        M, V = int(gt.shape[1]), (1 << 21) if vocab is None else int(vocab)
        for t in (n_distinct, gt_count):
            assert t.dtype == torch.int32 and tuple(t.shape) == (nb,) and t.is_contiguous()
        res = {}
        for name, shape in (("pos", (nb, M)), ("n_gt", (nb,))):
            t = out[name] if out is not None else torch.empty(shape, dtype=torch.int32, device=ranked.device)
            self._dev(t)
            assert tuple(t.shape) == shape and t.dtype == torch.int32 and t.is_contiguous(), name
            res[name] = t
        self._check(self.lib.sgg_match_triples(_p(ranked), _p(n_distinct), nb, K, _p(gt), _p(gt_count), M, V, _p(res["pos"]),
                                               _p(res["n_gt"]), self._stream()), "sgg_match_triples")
        return res

    @staticmethod
    def _logit_rows(logits):
        """[..., 3, V] logits whose leading dimensions are rows a fixed stride apart (Generator.sample's view of the head rows, or a
        column slice of a wider buffer) -> ([R, 3, V] view, row stride)."""
        assert logits.dtype == torch.float32 and logits.dim() >= 3 and logits.shape[-2] == 3
        V = int(logits.shape[-1])
        x = logits.reshape(-1, 3, V)
        assert x.data_ptr() == logits.data_ptr() and (x.stride(2) == 1 or V == 1) and x.stride(1) == V, "logits rows must be [3, V] contiguous"
        ld = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), 3 * V)
        return x, int(ld)

    def _out_tensors(self, spec, out, device):
        res = {}
        for name, (shape, dtype) in spec.items():
            t = out[name] if out is not None else torch.empty(shape, dtype=dtype, device=device)
            self._dev(t)
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous(), name
            res[name] = t
        return res

    def kbest_triples(self, logits, K, out=None):
        """The K most probable triples of every head row under the product of its three softmaxes (csrc/kbest.hip): logits fp32
        [..., 3, V] (R rows a fixed stride apart) -> dict of device tensors: triples int64 [R, K, 3], logp [R, K] (descending; ties by
        the slot ranks (i, j, l)), lse [R, 3].  Exact and deterministic; 1 <= K <= min(128, V^3); finite logits are a precondition.
        out: optional dict of preallocated contiguous tensors under those names."""
        self._dev(logits)
        x, ld = self._logit_rows(logits)
        R, V, K = int(x.shape[0]), int(x.shape[2]), max(int(K), 0)
        res = self._out_tensors({"triples": ((R, K, 3), torch.int64), "logp": ((R, K), torch.float32), "lse": ((R, 3), torch.float32)},
                                out, logits.device)
        self._check(self.lib.sgg_kbest_triples(_p(x), ld, R, V, K, _p(res["triples"]), _p(res["logp"]), _p(res["lse"]), self._stream()),
                    "sgg_kbest_triples")
        return res

    def kbest_merge(self, triples, logits, lse, K, out=None):
        """The K-best lists of an image's N samples merged into one ranked DISTINCT list (csrc/kbest.hip): triples int64
        [N, nb, Kc, 3] and lse [N, nb, 3] (kbest_triples' outputs on `logits`, reshaped), logits fp32 [N, nb, 3, V] -> dict of device
        tensors: triples int64 [nb, K, 3], scores [nb, K] (log-probability under the mixture of the N samples, descending; ties by
        the triple), best_sample int32 [nb, K] (the sample that gives the triple its highest probability), best_logp [nb, K] (that
        probability's log), counts int32 [nb, K] (lists that hold the triple), n_distinct int32 [nb]; slots behind n_distinct hold
        -1 / NaN / -1 / NaN / 0.  N = 1: the exact K-best list.  N > 1: the candidates are the union of the N lists, which
        approximates the mixture's own K best.  N * Kc <= 4096, 1 <= K <= N * Kc.  out: optional dict of preallocated tensors."""
        self._dev(triples, logits, lse)
        assert triples.dtype == torch.int64 and triples.dim() == 4 and triples.shape[3] == 3 and triples.is_contiguous()
        N, nb, Kc = int(triples.shape[0]), int(triples.shape[1]), int(triples.shape[2])
        assert logits.dim() == 4 and tuple(logits.shape[:3]) == (N, nb, 3), "logits must be [N, nb, 3, V]"
        x, ld = self._logit_rows(logits)
        V, K = int(x.shape[2]), max(int(K), 0)
        assert lse.dtype == torch.float32 and lse.numel() == N * nb * 3 and lse.is_contiguous(), "lse must be contiguous [N, nb, 3]"
        res = self._out_tensors({"triples": ((nb, K, 3), torch.int64), "scores": ((nb, K), torch.float32),
                                 "best_sample": ((nb, K), torch.int32), "best_logp": ((nb, K), torch.float32),
                                 "counts": ((nb, K), torch.int32), "n_distinct": ((nb,), torch.int32)}, out, triples.device)
        self._check(self.lib.sgg_kbest_merge(_p(triples), _p(x), ld, _p(lse), N, nb, Kc, V, K, _p(res["triples"]), _p(res["scores"]),
                                             _p(res["best_sample"]), _p(res["best_logp"]), _p(res["counts"]), _p(res["n_distinct"]),
                                             self._stream()), "sgg_kbest_merge")
        return res

    # -- grounded scene graphs (csrc/ground.hip; the definitions: sgg_amd/ground.py) ---------------------------
    def ground_assign(self, tokens, triples, n_distinct, vocab=None, out=None):
        """Which samples are which slot of their image's ranked list: tokens int64 [N, nb, 3], triples int64 [nb, K, 3] and n_distinct
        int32 [nb] (rank_triples' / kbest_merge's outputs) -> {"slot_of_sample": int32 [nb, N] (-1: none), "members": int32 [nb, N]
        (grouped by slot, ascending sample inside a slot, -1 in the unassigned tail), "start": int32 [nb, K + 1]}.  vocab: default
        the library's limit, 2^21.  out: optional dict of preallocated contiguous tensors under those names."""
        self._dev(tokens, triples, n_distinct)
        assert tokens.dtype == torch.int64 and tokens.dim() == 3 and tokens.shape[2] == 3 and tokens.is_contiguous()
        assert triples.dtype == torch.int64 and triples.dim() == 3 and triples.shape[2] == 3 and triples.is_contiguous()
        N, nb, K = int(tokens.shape[0]), int(tokens.shape[1]), int(triples.shape[1])
        assert triples.shape[0] == nb and n_distinct.dtype == torch.int32 and tuple(n_distinct.shape) == (nb,) and n_distinct.is_contiguous()
        V = (1 << 21) if vocab is None else int(vocab)
        res = self._out_tensors({"slot_of_sample": ((nb, N), torch.int32), "members": ((nb, N), torch.int32),
                                 "start": ((nb, K + 1), torch.int32)}, out, tokens.device)
        self._check(self.lib.sgg_ground_assign(_p(tokens), _p(triples), _p(n_distinct), N, nb, K, V, _p(res["slot_of_sample"]),
                                               _p(res["members"]), _p(res["start"]), self._stream()), "sgg_ground_assign")
        return res

    def ground_pool(self, alphas, members, start, fallback_sample, n_distinct, out=None):
        """The mean attention of every slot's members: alphas = the three fp32 [N * nb, L] attention views of the decoding steps (row
        k * nb + j; one common row stride, read in place - never a stacked copy), members int32 [nb, N] and start int32 [nb, K + 1]
        (ground_assign), fallback_sample int32 [nb, K] (the row a slot without a member takes; outside [0, N): zeros), n_distinct
        int32 [nb] -> {"maps": fp32 [nb, K, 3, L], "n_pooled": int32 [nb, K]}; slots behind n_distinct: zeros.  out: optional dict of
        preallocated contiguous tensors."""
        a0, a1, a2 = alphas
        self._dev(a0, a1, a2, members, start, fallback_sample, n_distinct)
        nb, N, K = int(members.shape[0]), int(members.shape[1]), int(start.shape[1]) - 1
        L = int(a0.shape[1])
        for a in (a0, a1, a2):
            assert a.dtype == torch.float32 and a.dim() == 2 and tuple(a.shape) == (N * nb, L) and (a.stride(1) == 1 or L == 1), \
                "alphas: three fp32 [N * nb, L] views with a contiguous last dimension"
        lda = int(_ld(a0))
        assert int(_ld(a1)) == lda and int(_ld(a2)) == lda, "alphas: one common row stride"
        for t, shape in ((members, (nb, N)), (start, (nb, K + 1)), (fallback_sample, (nb, K)), (n_distinct, (nb,))):
            assert t.dtype == torch.int32 and tuple(t.shape) == shape and t.is_contiguous()
        res = self._out_tensors({"maps": ((nb, K, 3, L), torch.float32), "n_pooled": ((nb, K), torch.int32)}, out, a0.device)
        self._check(self.lib.sgg_ground_pool(_p(a0), _p(a1), _p(a2), lda, _p(members), _p(start), _p(fallback_sample), _p(n_distinct),
                                             N, nb, K, L, _p(res["maps"]), _p(res["n_pooled"]), self._stream()), "sgg_ground_pool")
        return res

    def ground_resolve(self, maps, triples, n_distinct, n_pooled, Hf, Wf, overlap=0.5, box_frac=0.5, out=None):
        """Mentions joined into entity nodes: maps fp32 [nb, K, 3, Hf * Wf] and n_pooled int32 [nb, K] (ground_pool), triples int64
        [nb, K, 3], n_distinct int32 [nb] -> {"mention_node": int32 [nb, K, 2], "n_nodes": int32 [nb], "node_word": int64 [nb, 2K],
        "node_first" / "node_weight" / "node_mentions": int32 [nb, 2K], "node_map": fp32 [nb, 2K, L], "node_box": int32 [nb, 2K, 4]
        (y0, x0, y1, x1 inclusive), "node_center": fp32 [nb, 2K, 2] (y, x in cells)}; behind n_nodes: -1 / 0 / NaN.  overlap and
        box_frac in (0, 1]; K <= 1024.  out: optional dict of preallocated contiguous tensors."""
        self._dev(maps, triples, n_distinct, n_pooled)
        nb, K, L = int(triples.shape[0]), int(triples.shape[1]), int(Hf) * int(Wf)
        assert triples.dtype == torch.int64 and triples.dim() == 3 and triples.shape[2] == 3 and triples.is_contiguous()
        assert maps.dtype == torch.float32 and tuple(maps.shape) == (nb, K, 3, L) and maps.is_contiguous()
        for t, shape in ((n_distinct, (nb,)), (n_pooled, (nb, K))):
            assert t.dtype == torch.int32 and tuple(t.shape) == shape and t.is_contiguous()
        i32 = torch.int32
        res = self._out_tensors({"mention_node": ((nb, K, 2), i32), "n_nodes": ((nb,), i32), "node_word": ((nb, 2 * K), torch.int64),
                                 "node_first": ((nb, 2 * K), i32), "node_weight": ((nb, 2 * K), i32), "node_mentions": ((nb, 2 * K), i32),
                                 "node_map": ((nb, 2 * K, L), torch.float32), "node_box": ((nb, 2 * K, 4), i32),
                                 "node_center": ((nb, 2 * K, 2), torch.float32)}, out, maps.device)
        self._check(self.lib.sgg_ground_resolve(_p(maps), _p(triples), _p(n_distinct), _p(n_pooled), nb, K, int(Hf), int(Wf),
                                                float(overlap), float(box_frac), _p(res["mention_node"]), _p(res["n_nodes"]),
                                                _p(res["node_word"]), _p(res["node_first"]), _p(res["node_weight"]),
                                                _p(res["node_mentions"]), _p(res["node_map"]), _p(res["node_box"]),
                                                _p(res["node_center"]), self._stream()), "sgg_ground_resolve")
        return res

    # -- generator likelihood (csrc/xent.hip) ---------------------------------------------------------------
    @staticmethod
    def _rows(t, what):
        """[..., V] tensor whose rows are ONE fixed stride apart (a contiguous tensor, or a column slice of a wider 2-D buffer) ->
        ([R, V] view, row stride)."""
        assert t.dtype == torch.float32 and t.dim() >= 2, what
        V = int(t.shape[-1])
        x = t if t.dim() == 2 else t.view(-1, V)       # (raises where the rows are not one stride apart)
        assert x.stride(1) == 1 or V == 1, "%s: the last dimension must be contiguous" % what
        return x, int(_ld(x))

    @staticmethod
    def _rows_symbol(name, V, gumbel=None):
        """The row kernel behind an entry point (csrc/softmax_rows.h): resident up to V = 1024, streaming above; <gumbel> where templated."""
        return "%s_%s_kernel%s" % (name, "resident" if V <= 1024 else "stream", "" if gumbel is None else "<%s>" % ("true" if gumbel else "false"))

    def softmax_xent(self, logits, labels=None, scale=1.0, accumulate=False, dlogits=None, nll=None, lse=None, hit=None):
        """Row-wise log-softmax cross-entropy, forward and gradient in one launch (csrc/xent.hip; include/sgg_hip.h): logits fp32
        [..., V] (R rows one stride apart), labels int64 with R elements.  Outputs, each optional: dlogits (shape of logits, its own
        row stride) = scale * (softmax - onehot), stored or - accumulate - added; nll fp32 [R]; lse fp32 [R]; hit int32 [R] (1: the
        label is the row's argmax, 0: not, -1: the label is outside [0, V) and the row was skipped).  labels=None: lse only."""
        self._dev(logits, labels, dlogits, nll, lse, hit)
        x, ld = self._rows(logits, "logits")
        R, V = int(x.shape[0]), int(x.shape[1])
        ldd = 0
        if dlogits is not None:
            d, ldd = self._rows(dlogits, "dlogits")
            assert tuple(d.shape) == (R, V), "dlogits must have the logits' rows"
        if labels is not None:
            assert labels.dtype == torch.int64 and labels.numel() == R and labels.is_contiguous()
        for t, dt in ((nll, torch.float32), (lse, torch.float32), (hit, torch.int32)):
            assert t is None or (t.dtype == dt and t.numel() == R and t.is_contiguous())
        nb = 4.0 * R * V * (1 + (0 if dlogits is None else (2 if accumulate else 1)))
        self._check(self._timed(self._rows_symbol("xent_rows", V), 0.0,
                                lambda: self.lib.sgg_softmax_xent(_p(x), ld, R, V, _p(labels), float(scale), int(bool(accumulate)),
                                                                  _p(dlogits), ldd, _p(nll), _p(lse), _p(hit), self._stream()), nb),
                    "sgg_softmax_xent")

    def xent_summary(self, nll, hit, out=None):
        """out fp32 [4] = (mean nll per valid row, token accuracy, triple accuracy, valid rows) of softmax_xent's nll / hit over
        R = 3 B rows, three consecutive rows per triple (include/sgg_hip.h); one workgroup, fixed order."""
        self._dev(nll, hit, out)
        R = nll.numel()
        assert nll.dtype == torch.float32 and hit.dtype == torch.int32 and hit.numel() == R and nll.is_contiguous() and hit.is_contiguous()
        if out is None:
            out = torch.empty(4, dtype=torch.float32, device=nll.device)
        assert out.dtype == torch.float32 and out.numel() == 4 and out.is_contiguous()
        self._check(self.lib.sgg_xent_summary(_p(nll), _p(hit), R, _p(out), self._stream()), "sgg_xent_summary")
        return out

    def triple_logp(self, logits, lse, gt, gt_count, out=None):
        """The log-probability of given triples under the mixture of an image's N samples (csrc/xent.hip): logits fp32
        [N, nb, 3, V], lse fp32 [N, nb, 3], gt int64 [nb, M, 3], gt_count int32 [nb] -> dict of device tensors: mix [nb, M], mean
        [nb, M], slot [nb, M, 3], status int32 [nb, M] (0 valid, -3 padding, -4 token outside [0, V); NaN in the floats of a row that
        is not valid).  out: optional dict of preallocated contiguous tensors under those names."""
        self._dev(logits, lse, gt, gt_count)
        assert logits.dim() == 4 and logits.shape[2] == 3, "logits must be [N, nb, 3, V]"
        N, nb = int(logits.shape[0]), int(logits.shape[1])
        x, ld = self._logit_rows(logits)
        V = int(x.shape[2])
        assert lse.dtype == torch.float32 and lse.numel() == N * nb * 3 and lse.is_contiguous(), "lse must be contiguous [N, nb, 3]"
        assert gt.dtype == torch.int64 and gt.dim() == 3 and gt.shape[0] == nb and gt.shape[2] == 3 and gt.is_contiguous()
        M = int(gt.shape[1])
        assert gt_count.dtype == torch.int32 and tuple(gt_count.shape) == (nb,) and gt_count.is_contiguous()
        res = self._out_tensors({"mix": ((nb, M), torch.float32), "mean": ((nb, M), torch.float32), "slot": ((nb, M, 3), torch.float32),
                                 "status": ((nb, M), torch.int32)}, out, logits.device)
        self._check(self.lib.sgg_triple_logp(_p(x), ld, _p(lse), N, nb, V, _p(gt), _p(gt_count), M, _p(res["mix"]), _p(res["mean"]),
                                             _p(res["slot"]), _p(res["status"]), self._stream()), "sgg_triple_logp")
        return res

    # -- image retrieval by triple query (csrc/retrieve.hip; host side: sgg_amd/retrieve.py) ------------------------------
    def query_logp(self, logits, lse, tok, ucount, qidx, scores, col0=0):
        """The mixture log-probability of Q shared (partial) triples for the nb images of a batch (csrc/retrieve.hip): logits fp32
        [N, nb, 3, V], lse fp32 [N, nb, 3], tok int32 [3, U] and ucount (three host integers) - per slot the distinct tokens the
        queries use, sgg_amd.retrieve.compile_queries builds them - qidx int32 [Q, 3] (index into the slot's list; -1: wildcard)
        -> scores[q, col0 + j] for j < nb of the caller's fp32 [Q, n_columns] matrix (rows one stride apart); nothing else of it is
        written.  1 <= Q <= 4096 per launch.  Returns scores."""
        self._dev(logits, lse, tok, qidx, scores)
        assert logits.dim() == 4 and logits.shape[2] == 3, "logits must be [N, nb, 3, V]"
        N, nb = int(logits.shape[0]), int(logits.shape[1])
        x, ld = self._logit_rows(logits)
        V = int(x.shape[2])
        assert lse.dtype == torch.float32 and lse.numel() == N * nb * 3 and lse.is_contiguous(), "lse must be contiguous [N, nb, 3]"
        assert tok.dtype == torch.int32 and tok.dim() == 2 and tok.shape[0] == 3 and tok.is_contiguous(), "tok must be int32 [3, U]"
        assert qidx.dtype == torch.int32 and qidx.dim() == 2 and qidx.shape[1] == 3 and qidx.is_contiguous(), "qidx must be int32 [Q, 3]"
        U, Q = int(tok.shape[1]), int(qidx.shape[0])
        u0, u1, u2 = (int(u) for u in ucount)
        sc, lds = self._rows(scores, "scores")
        assert sc.dim() == 2 and sc.shape[0] == Q and 0 <= int(col0) and int(col0) + nb <= sc.shape[1], "scores must be [Q, >= col0 + nb]"
        self._check(self.lib.sgg_query_logp(_p(x), ld, _p(lse), N, nb, V, _p(tok), U, u0, u1, u2, _p(qidx), Q, _p(sc), lds, int(col0),
                                            self._stream()), "sgg_query_logp")
        return scores

    def retrieve_topk(self, scores, n_images, K, out=None):
        """Per query the first K images of scores[:, :n_images] (fp32 [Q, >= n_images], rows one stride apart) under (score
        descending, image index ascending; +-0 equal) -> {"idx": int32 [Q, K], "scores": fp32 [Q, K] (the inputs' bits)}; slots
        behind min(K, n_images) hold -1 / NaN.  Exact; 1 <= K <= 1024.  out: optional dict of preallocated contiguous tensors."""
        self._dev(scores)
        sc, lds = self._rows(scores, "scores")
        Q, K, n = int(sc.shape[0]), max(int(K), 0), int(n_images)
        assert sc.dim() == 2 and 1 <= n <= sc.shape[1], "scores must be [Q, >= n_images]"
        res = self._out_tensors({"idx": ((Q, K), torch.int32), "scores": ((Q, K), torch.float32)}, out, scores.device)
        self._check(self.lib.sgg_retrieve_topk(_p(sc), lds, Q, n, K, _p(res["idx"]), _p(res["scores"]), self._stream()),
                    "sgg_retrieve_topk")
        return res

    def retrieve_ranks(self, scores, n_images, rel_ptr, rel_idx, out=None):
        """Where every query's relevant images stand in the order of retrieve_topk: scores fp32 [Q, >= n_images], rel_ptr int32
        [Q + 1] and rel_idx int32 [max(1, rel_ptr[Q])] (CSR, sgg_amd.retrieve.relevance) -> {"ranks": int32 like rel_idx (1-based),
        "first_rank": int32 [Q], "ap": fp64 [Q], "status": int32 [Q] (0 valid, -3 no relevant image: first_rank 0, ap NaN)}.
        out: optional dict of preallocated contiguous tensors."""
        self._dev(scores, rel_ptr, rel_idx)
        sc, lds = self._rows(scores, "scores")
        Q, n = int(sc.shape[0]), int(n_images)
        assert sc.dim() == 2 and 1 <= n <= sc.shape[1], "scores must be [Q, >= n_images]"
        assert rel_ptr.dtype == torch.int32 and tuple(rel_ptr.shape) == (Q + 1,) and rel_ptr.is_contiguous()
        assert rel_idx.dtype == torch.int32 and rel_idx.dim() == 1 and rel_idx.numel() >= 1 and rel_idx.is_contiguous()
        res = self._out_tensors({"ranks": (tuple(rel_idx.shape), torch.int32), "first_rank": ((Q,), torch.int32),
                                 "ap": ((Q,), torch.float64), "status": ((Q,), torch.int32)}, out, scores.device)
        self._check(self.lib.sgg_retrieve_ranks(_p(sc), lds, Q, n, _p(rel_ptr), _p(rel_idx), _p(res["ranks"]), _p(res["first_rank"]),
                                                _p(res["ap"]), _p(res["status"]), self._stream()), "sgg_retrieve_ranks")
        return res

    # -- predicate classification (csrc/predcls.hip; host side and the definitions: sgg_amd/predcls.py) -----------------------
    def pair_predicate_logp(self, logits, lse, pairs, pair_count, joint=None, out=None):
        """The mixture log-probability of EVERY predicate token for given (subject, object) pairs (csrc/predcls.hip): logits fp32
        [N, nb, 3, V], lse fp32 [N, nb, 3], pairs int32 [nb, P, 2], pair_count int32 [nb] -> dict of device tensors: joint fp32
        [nb, P, V] (bit for bit triple_logp's mix of (s, v, o); `joint`: the caller's [nb, P, >= V] buffer or a column slice of it,
        rows one stride apart, only its V columns are written), marg fp32 [nb, P] (the pair with the predicate marginalised), status
        int32 [nb, P] (0 valid, -3 padding, -4 a token outside [0, V); NaN in the floats of a pair that is not valid).
        1 <= N, P <= 4096.  out: optional dict of preallocated contiguous marg / status."""
        self._dev(logits, lse, pairs, pair_count, joint)
        assert logits.dim() == 4 and logits.shape[2] == 3, "logits must be [N, nb, 3, V]"
        N, nb = int(logits.shape[0]), int(logits.shape[1])
        x, ld = self._logit_rows(logits)
        V = int(x.shape[2])
        assert lse.dtype == torch.float32 and lse.numel() == N * nb * 3 and lse.is_contiguous(), "lse must be contiguous [N, nb, 3]"
        assert pairs.dtype == torch.int32 and pairs.dim() == 3 and pairs.shape[0] == nb and pairs.shape[2] == 2 and pairs.is_contiguous(), \
            "pairs must be contiguous int32 [nb, P, 2]"
        P = int(pairs.shape[1])
        assert pair_count.dtype == torch.int32 and tuple(pair_count.shape) == (nb,) and pair_count.is_contiguous()
        if joint is None:
            joint = torch.empty((nb, P, V), dtype=torch.float32, device=logits.device)
        assert joint.dim() == 3 and tuple(joint.shape) == (nb, P, V), "joint must be [nb, P, V]"
        jv, ldj = self._rows(joint, "joint")
        res = self._out_tensors({"marg": ((nb, P), torch.float32), "status": ((nb, P), torch.int32)}, out, logits.device)
        self._check(self.lib.sgg_pair_predicate_logp(_p(x), ld, _p(lse), N, nb, V, _p(pairs), _p(pair_count), P, _p(jv), ldj,
                                                     _p(res["marg"]), _p(res["status"]), self._stream()), "sgg_pair_predicate_logp")
        res["joint"] = joint
        return res

    def predcls_pair_topk(self, joint, status, Kc, gt_pair, gt_pred, out=None):
        """Per pair the first Kc predicate tokens of its joint row under (joint descending, token ascending): joint fp32 [nb, P, V]
        (rows one stride apart) and status int32 [nb, P] of pair_predicate_logp, gt_pair int32 [nb, M] (the pair of true triple m, or
        -1), gt_pred int32 [nb, M] -> {"top_tok": int32 [nb, P, Kc], "top_score": fp32 [nb, P, Kc] (the rows' own bits; -1 / NaN
        behind min(Kc, V) and for a pair that is not valid), "gt_rank": int32 [nb, M] (1 + the tokens ahead of the true predicate in
        its pair's order; 0 without a valid pair or token)}.  1 <= Kc <= 128, 1 <= M <= 4096.  out: optional preallocated tensors."""
        self._dev(joint, status, gt_pair, gt_pred)
        assert joint.dim() == 3, "joint must be [nb, P, V]"
        nb, P, V = (int(n) for n in joint.shape)
        jv, ldj = self._rows(joint, "joint")
        assert status.dtype == torch.int32 and tuple(status.shape) == (nb, P) and status.is_contiguous()
        M, Kc = int(gt_pair.shape[1]), max(int(Kc), 0)
        for t in (gt_pair, gt_pred):
            assert t.dtype == torch.int32 and tuple(t.shape) == (nb, M) and t.is_contiguous(), "gt_pair / gt_pred must be int32 [nb, M]"
        res = self._out_tensors({"top_tok": ((nb, P, Kc), torch.int32), "top_score": ((nb, P, Kc), torch.float32),
                                 "gt_rank": ((nb, M), torch.int32)}, out, joint.device)
        self._check(self.lib.sgg_predcls_pair_topk(_p(jv), ldj, _p(status), nb, P, V, Kc, _p(gt_pair), _p(gt_pred), M, _p(res["top_tok"]),
                                                   _p(res["top_score"]), _p(res["gt_rank"]), self._stream()), "sgg_predcls_pair_topk")
        return res

    def predcls_merge(self, pairs, top_tok, top_score, marg, K, per_pair=1, conditional=False, out=None):
        """The first K (pair, predicate) candidates of every image: pairs int32 [nb, P, 2], top_tok / top_score [nb, P, Kc] of
        predcls_pair_topk, marg fp32 [nb, P]; the candidates are the slots r < per_pair of every pair with a token >= 0, scored
        top_score - marg (conditional) or top_score, ordered by (score descending, pair index ascending, r ascending) ->
        {"triples": int64 [nb, K, 3] = (s, token, o), "scores": fp32 [nb, K], "src": int32 [nb, K] = pair * per_pair + r,
        "n_distinct": int32 [nb] (the candidates; it may exceed K)}; -1 / NaN / -1 behind them: rank_triples' layout, what
        match_triples takes.  per_pair = 1: one predicate per pair (the graph constraint).  P * per_pair <= 2^21, 1 <= K <= 1024."""
        self._dev(pairs, top_tok, top_score, marg)
        assert pairs.dtype == torch.int32 and pairs.dim() == 3 and pairs.shape[2] == 2 and pairs.is_contiguous(), "pairs must be int32 [nb, P, 2]"
        nb, P = int(pairs.shape[0]), int(pairs.shape[1])
        assert top_tok.dtype == torch.int32 and top_tok.dim() == 3 and tuple(top_tok.shape[:2]) == (nb, P) and top_tok.is_contiguous()
        Kc, K = int(top_tok.shape[2]), max(int(K), 0)
        assert top_score.dtype == torch.float32 and tuple(top_score.shape) == (nb, P, Kc) and top_score.is_contiguous()
        assert marg.dtype == torch.float32 and tuple(marg.shape) == (nb, P) and marg.is_contiguous()
        res = self._out_tensors({"triples": ((nb, K, 3), torch.int64), "scores": ((nb, K), torch.float32), "src": ((nb, K), torch.int32),
                                 "n_distinct": ((nb,), torch.int32)}, out, pairs.device)
        self._check(self.lib.sgg_predcls_merge(_p(pairs), _p(top_tok), _p(top_score), _p(marg), nb, P, Kc, int(per_pair),
                                               int(bool(conditional)), K, _p(res["triples"]), _p(res["scores"]), _p(res["src"]),
                                               _p(res["n_distinct"]), self._stream()), "sgg_predcls_merge")
        return res

    # -- relaxed generator output (csrc/relax.hip) ---------------------------------------------------------------
    def relax_rows(self, x, tau, y=None, gumbel=False, seed=0, draw=0, u_out=None):
        """y = softmax((x + g) / tau) row by row (csrc/relax.hip; include/sgg_hip.h): x fp32 [..., V] (R rows one stride apart), y of
        the same rows with its own stride (default: x itself, relaxed in place).  gumbel: g = -log(-log u) drawn in the kernel from
        Philox4x32-10 keyed by the 64-bit `seed`, counter (j >> 2, row, draw): a pure function of (seed, draw, row, j); else g = 0.
        u_out (gumbel only): receives u.  Returns y."""
        if y is None:
            y = x
        self._dev(x, y, u_out)
        xv, ldx = self._rows(x, "x")
        yv, ldy = self._rows(y, "y")
        R, V = int(xv.shape[0]), int(xv.shape[1])
        assert tuple(yv.shape) == (R, V), "y must have x's rows"
        uv, ldu = None, 0
        if u_out is not None:
            uv, ldu = self._rows(u_out, "u_out")
            assert tuple(uv.shape) == (R, V), "u_out must have x's rows"
        self._check(self._timed(self._rows_symbol("relax_rows", V, gumbel), 0.0, lambda: self.lib.sgg_relax_rows(
            _p(xv), ldx, R, V, float(tau), int(bool(gumbel)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, _p(yv), ldy,
            _p(uv), ldu, self._stream()), 4.0 * R * V * 2), "sgg_relax_rows")
        return y

    def relax_rows_bwd(self, y, dy, tau, scale=1.0, dx=None):
        """dx = (scale / tau) * y * (dy - sum_k y_k dy_k) row by row: the gradient of scale * <dy, y> by the x of relax_rows (either
        mode; needs neither x nor the noise).  y, dy, dx fp32 [..., V], each with its own row stride; default dx: dy, in place."""
        if dx is None:
            dx = dy
        self._dev(y, dy, dx)
        yv, ldy = self._rows(y, "y")
        gv, lddy = self._rows(dy, "dy")
        dv, lddx = self._rows(dx, "dx")
        R, V = int(yv.shape[0]), int(yv.shape[1])
        assert tuple(gv.shape) == (R, V) and tuple(dv.shape) == (R, V), "dy and dx must have y's rows"
        self._check(self._timed(self._rows_symbol("relax_bwd", V), 0.0, lambda: self.lib.sgg_relax_rows_bwd(
            _p(yv), ldy, _p(gv), lddy, R, V, float(tau), float(scale), _p(dv), lddx, self._stream()), 4.0 * R * V * 3), "sgg_relax_rows_bwd")
        return dx

    def relax_rows_hard(self, x, y=None, tok=None, gumbel=False, seed=0, draw=0):
        """The straight-through forward (csrc/relax.hip; include/sgg_hip.h): k = the first argmax of x + g per row (g as relax_rows
        draws it, or 0), y = onehot(k) in fp32 (rows of x's shape with their own stride), tok int64 [R] = k.  y=None and tok=None:
        x itself becomes the one-hot rows; tok alone with gumbel: a Gumbel-max sample from softmax(x).  Returns (y, tok)."""
        if y is None and tok is None:
            y = x
        self._dev(x, y, tok)
        xv, ldx = self._rows(x, "x")
        R, V = int(xv.shape[0]), int(xv.shape[1])
        yv, ldy = None, 0
        if y is not None:
            yv, ldy = self._rows(y, "y")
            assert tuple(yv.shape) == (R, V), "y must have x's rows"
        assert tok is None or (tok.dtype == torch.int64 and tok.numel() == R and tok.is_contiguous()), "tok: contiguous int64, one per row"
        self._check(self._timed(self._rows_symbol("relax_hard", V, gumbel), 0.0, lambda: self.lib.sgg_relax_rows_hard(
            _p(xv), ldx, R, V, int(bool(gumbel)), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, _p(yv), ldy, _p(tok),
            self._stream()), 4.0 * R * V * (1 if y is None else 2)), "sgg_relax_rows_hard")
        return y, tok

    def relax_rows_hard_bwd(self, x, dy, tau, scale=1.0, gumbel=False, seed=0, draw=0, dx=None):
        """The straight-through backward: dx = (scale / tau) * y * (dy - sum_k y_k dy_k) with y = softmax((x + g) / tau) rebuilt from
        the logits x and the noise of (seed, draw) - the launch that made the hard rows left no y behind.  x, dy, dx fp32 [..., V],
        each with its own row stride; default dx: dy, in place (never x)."""
        if dx is None:
            dx = dy
        self._dev(x, dy, dx)
        xv, ldx = self._rows(x, "x")
        gv, lddy = self._rows(dy, "dy")
        dv, lddx = self._rows(dx, "dx")
        R, V = int(xv.shape[0]), int(xv.shape[1])
        assert tuple(gv.shape) == (R, V) and tuple(dv.shape) == (R, V), "dy and dx must have x's rows"
        self._check(self._timed(self._rows_symbol("relax_hard_bwd", V, gumbel), 0.0, lambda: self.lib.sgg_relax_rows_hard_bwd(
            _p(xv), ldx, _p(gv), lddy, R, V, float(tau), float(scale), int(bool(gumbel)), int(seed) & 0xFFFFFFFFFFFFFFFF,
            int(draw) & 0xFFFFFFFFFFFFFFFF, _p(dv), lddx, self._stream()), 4.0 * R * V * 5), "sgg_relax_rows_hard_bwd")
        return dx

    # -- score-function generator update (csrc/score.hip) -----------------------------------------------------------
    SCORE_BASELINES = {"none": 0, "rloo": 1}

    def score_advantage(self, d_out, baseline="rloo", adv=None, out2=None):
        """Rewards and advantages of B sampled triples (csrc/score.hip; include/sgg_hip.h): d_out fp32 [B, T] (rows one stride apart) =
        the critic's outputs, r_b = mean_t d_out[b, t]; adv fp32 [B] = r_b ("none") or r_b minus the mean of the other rewards
        ("rloo": needs B >= 2).  out2 (optional) fp32 [2] = (mean reward, mean advantage^2).  One workgroup.  Returns adv."""
        if baseline not in self.SCORE_BASELINES:
            raise ValueError("score_advantage: baseline must be one of %s (got %r)" % (", ".join(sorted(self.SCORE_BASELINES)), baseline))
        self._dev(d_out, adv, out2)
        assert d_out.dim() == 2, "d_out must be [B, T]"
        dv, ldd = self._rows(d_out, "d_out")
        B, T = int(dv.shape[0]), int(dv.shape[1])
        if adv is None:
            adv = torch.empty(B, dtype=torch.float32, device=d_out.device)
        assert adv.dtype == torch.float32 and adv.numel() == B and adv.is_contiguous(), "adv: contiguous fp32, one per row of d_out"
        assert out2 is None or (out2.dtype == torch.float32 and out2.numel() == 2 and out2.is_contiguous()), "out2: contiguous fp32 [2]"
        self._check(self.lib.sgg_score_advantage(_p(dv), ldd, B, T, self.SCORE_BASELINES[baseline], _p(adv), _p(out2), self._stream()),
                    "sgg_score_advantage")
        return adv

    def score_rows(self, x, tok, adv=None, group=1, coef=1.0, ent_coef=0.0, accumulate=False, dx=None, logp=None, ent=None):
        """The policy gradient of sampled tokens, row by row in one launch (csrc/score.hip; include/sgg_hip.h): x fp32 [..., V] (R rows
        one stride apart), tok int64 with R elements, adv fp32 with at least ceil(R / group) elements (None: every weight is coef).
        Outputs, each optional (not all absent): dx (x's rows, its own stride; never x itself) = coef * adv[r // group] * (softmax -
        onehot(tok)) + ent_coef * softmax * (log softmax + H), stored or - accumulate - added; logp fp32 [R] = log softmax(x)[tok];
        ent fp32 [R] = H, the row's entropy.  A token outside [0, V) skips its row (logp 0, dx zero or untouched)."""
        self._dev(x, tok, adv, dx, logp, ent)
        xv, ldx = self._rows(x, "x")
        R, V = int(xv.shape[0]), int(xv.shape[1])
        group = int(group)
        assert tok.dtype == torch.int64 and tok.numel() == R and tok.is_contiguous(), "tok: contiguous int64, one per row"
        if adv is not None:
            assert adv.dtype == torch.float32 and adv.is_contiguous(), "adv: contiguous fp32"
            assert group < 1 or adv.numel() >= -(-R // group), "adv needs ceil(R / group) = %d elements (got %d)" % (-(-R // max(group, 1)), adv.numel())
        dv, lddx = None, 0
        if dx is not None:
            dv, lddx = self._rows(dx, "dx")
            assert tuple(dv.shape) == (R, V), "dx must have x's rows"
        for t in (logp, ent):
            assert t is None or (t.dtype == torch.float32 and t.numel() == R and t.is_contiguous()), "logp, ent: contiguous fp32, one per row"
        nb = 4.0 * R * V * (1 + (0 if dx is None else (2 if accumulate else 1)))
        self._check(self._timed(self._rows_symbol("score_rows", V), 0.0, lambda: self.lib.sgg_score_rows(
            _p(xv), ldx, R, V, _p(tok), _p(adv), group, float(coef), float(ent_coef), int(bool(accumulate)), _p(dv), lddx, _p(logp), _p(ent),
            self._stream()), nb), "sgg_score_rows")
        return dx

    def score_summary(self, logp, ent, out2=None):
        """out2 fp32 [2] = (mean logp, mean ent) of score_rows' per-row outputs over their R rows; one workgroup, fp64, row order."""
        self._dev(logp, ent, out2)
        R = logp.numel()
        assert logp.dtype == torch.float32 and ent.dtype == torch.float32 and ent.numel() == R and logp.is_contiguous() and ent.is_contiguous()
        if out2 is None:
            out2 = torch.empty(2, dtype=torch.float32, device=logp.device)
        assert out2.dtype == torch.float32 and out2.numel() == 2 and out2.is_contiguous()
        self._check(self.lib.sgg_score_summary(_p(logp), _p(ent), R, _p(out2), self._stream()), "sgg_score_summary")
        return out2

    # -- S samples per row (csrc/score.hip, "S samples per row"): sample s of logits row r sits at index s * R + r ---------------
    SCORE_BASELINES_MULTI = {"none": 0, "rloo": 1, "image": 2}
    SCORE_MAX_SAMPLES = 16

    def sample_rows_multi(self, x, tok, seed=0, draw=0):
        """S Gumbel-max samples of softmax(x) per row in one launch (include/sgg_hip.h): x fp32 [..., V] (R rows one stride apart), tok
        contiguous int64 [S, ...] with S * R elements, S = tok.shape[0] in 1..16.  tok[s] is, bit for bit, the tok of
        relax_rows_hard(x, tok=..., gumbel=True, seed=seed, draw=draw | (s << 56)); draw < 2^56.  The row is read once for S <= 8 and at
        most twice above; no one-hot row is written.  Returns tok."""
        self._dev(x, tok)
        xv, ldx = self._rows(x, "x")
        R, V = int(xv.shape[0]), int(xv.shape[1])
        assert tok.dtype == torch.int64 and tok.dim() >= 1 and tok.is_contiguous(), "tok: contiguous int64 [S, ...]"
        S = int(tok.shape[0])
        assert S < 1 or tok.numel() == S * R, "tok: one token per sample and row (S * R = %d elements, got %d)" % (S * R, tok.numel())
        self._check(self._timed("sample_rows_multi_%s_kernel" % ("resident" if V <= 1024 else "stream"), 0.0,
                                lambda: self.lib.sgg_sample_rows_multi(_p(xv), ldx, R, V, S, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                                       int(draw) & 0xFFFFFFFFFFFFFFFF, _p(tok), self._stream()),
                                4.0 * R * V * (1 if S <= 8 or V <= 1024 else 2)), "sgg_sample_rows_multi")
        return tok

    def score_advantage_multi(self, d_out, samples, baseline="image", adv=None, out2=None):
        """Rewards and advantages of S = samples sampled triples per image: d_out fp32 [S * B, T] (rows one stride apart; row s * B + b
        = sample s of image b), r = the row means; adv fp32 [S * B] = r ("none"), r minus the mean of the other S * B - 1 rewards
        ("rloo"), or r[s, b] minus the mean reward of the other samples of image b ("image": S >= 2).  out2 (optional) fp32 [2] =
        (mean reward, mean advantage^2).  One workgroup.  Returns adv."""
        if baseline not in self.SCORE_BASELINES_MULTI:
            raise ValueError("score_advantage_multi: baseline must be one of %s (got %r)" % (", ".join(sorted(self.SCORE_BASELINES_MULTI)), baseline))
        self._dev(d_out, adv, out2)
        assert d_out.dim() == 2, "d_out must be [S * B, T]"
        dv, ldd = self._rows(d_out, "d_out")
        N, T, S = int(dv.shape[0]), int(dv.shape[1]), int(samples)
        assert S < 1 or N % S == 0, "d_out has %d rows: not S = %d samples of every image" % (N, S)
        if adv is None:
            adv = torch.empty(N, dtype=torch.float32, device=d_out.device)
        assert adv.dtype == torch.float32 and adv.numel() == N and adv.is_contiguous(), "adv: contiguous fp32, one per row of d_out"
        assert out2 is None or (out2.dtype == torch.float32 and out2.numel() == 2 and out2.is_contiguous()), "out2: contiguous fp32 [2]"
        self._check(self.lib.sgg_score_advantage_multi(_p(dv), ldd, N // max(S, 1), S, T, self.SCORE_BASELINES_MULTI[baseline], _p(adv),
                                                       _p(out2), self._stream()), "sgg_score_advantage_multi")
        return adv

    def score_rows_multi(self, x, tok, adv=None, group=1, coef=1.0, ent_coef=0.0, accumulate=False, dx=None, logp=None, ent=None):
        """The policy gradient of S sampled tokens per row in one launch: x fp32 [..., V] (R rows one stride apart), tok contiguous
        int64 [S, ...] (S * R elements), adv fp32 with S * (R / group) elements (None: every weight is coef; R % group == 0).  Outputs,
        each optional (not all absent): dx (x's rows, its own stride; never x itself) = (sum_s w_s) softmax - sum_s w_s onehot(tok_s)
        + ent_coef * softmax * (log softmax + H) with w_s = coef * adv[s * (R / group) + r // group], stored or - accumulate - added;
        logp fp32 [S * R] = log softmax(x)[tok_s]; ent fp32 [R] = H.  A token outside [0, V) drops that sample's term alone (logp 0)."""
        self._dev(x, tok, adv, dx, logp, ent)
        xv, ldx = self._rows(x, "x")
        R, V = int(xv.shape[0]), int(xv.shape[1])
        group = int(group)
        assert tok.dtype == torch.int64 and tok.dim() >= 1 and tok.is_contiguous(), "tok: contiguous int64 [S, ...]"
        S = int(tok.shape[0])
        assert S < 1 or tok.numel() == S * R, "tok: one token per sample and row (S * R = %d elements, got %d)" % (S * R, tok.numel())
        if adv is not None:
            assert adv.dtype == torch.float32 and adv.is_contiguous(), "adv: contiguous fp32"
            assert group < 1 or adv.numel() >= S * (R // group), "adv needs S * (R / group) = %d elements (got %d)" % (S * (R // max(group, 1)), adv.numel())
        dv, lddx = None, 0
        if dx is not None:
            dv, lddx = self._rows(dx, "dx")
            assert tuple(dv.shape) == (R, V), "dx must have x's rows"
        assert logp is None or (logp.dtype == torch.float32 and logp.numel() == S * R and logp.is_contiguous()), "logp: contiguous fp32 [S * R]"
        assert ent is None or (ent.dtype == torch.float32 and ent.numel() == R and ent.is_contiguous()), "ent: contiguous fp32, one per row"
        nb = 4.0 * R * V * (1 + (0 if dx is None else (2 if accumulate else 1)))
        self._check(self._timed("score_rows_multi_%s_kernel" % ("resident" if V <= 1024 else "stream"), 0.0,
                                lambda: self.lib.sgg_score_rows_multi(_p(xv), ldx, R, V, S, _p(tok), _p(adv), group, float(coef), float(ent_coef),
                                                                      int(bool(accumulate)), _p(dv), lddx, _p(logp), _p(ent), self._stream()),
                                nb), "sgg_score_rows_multi")
        return dx

    def score_summary_multi(self, logp, ent, out2=None):
        """out2 fp32 [2] = (mean logp, mean ent) of score_rows_multi's outputs (S * R and R values); one workgroup, fp64, index order."""
        self._dev(logp, ent, out2)
        assert logp.dtype == torch.float32 and ent.dtype == torch.float32 and logp.is_contiguous() and ent.is_contiguous()
        if out2 is None:
            out2 = torch.empty(2, dtype=torch.float32, device=logp.device)
        assert out2.dtype == torch.float32 and out2.numel() == 2 and out2.is_contiguous()
        self._check(self.lib.sgg_score_summary_multi(_p(logp), logp.numel(), _p(ent), ent.numel(), _p(out2), self._stream()),
                    "sgg_score_summary_multi")
        return out2

    def fill(self, t, value):
        self._dev(t)
        assert t.is_contiguous()
        self._check(self.lib.sgg_fill(_p(t), t.numel(), float(value), self._stream()), "sgg_fill")
