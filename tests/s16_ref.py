"""Host emulation of the pre-split ("S16") tensor format (csrc/split16.h; include/sgg_hip.h out_format / operand_format), shared by
tests/test_presplit_gpu.py and tests/test_layernorm_geometry_gpu.py (test infrastructure)."""
import math

import torch


def s16_exp(amax):
    """scale_exp_from_amax of sgg_common.h."""
    if not amax > 0.0:
        return 0
    _, k = math.frexp(amax)
    return max(-100, min(100, 14 - k))


def to_s16(x, amax):
    """Host emulation of split8<2, true> into the S16 layout: x [..., C] f32 (C % 32 == 0) -> f32-typed tensor of the same shape whose
    bytes are, per aligned 32-channel group, 32 leading fp16 pieces then 32 residual pieces of x * 2^e."""
    C = x.shape[-1]
    xs = x.float() * (2.0 ** s16_exp(amax))
    hi = xs.half()
    lo = (xs - hi.float()).half()
    out = torch.stack([hi.reshape(-1, C // 32, 32), lo.reshape(-1, C // 32, 32)], dim=2)      # [px, group, 2, 32]
    return out.contiguous().view(torch.int16).reshape(-1).view(torch.float32).reshape(x.shape)


def s16_pieces(t):
    """S16 tensor (f32-typed) -> (hi, lo) as int16 bit patterns [px, C / 32, 32]."""
    C = t.shape[-1]
    h = t.contiguous().view(torch.int16).reshape(-1, C // 32, 2, 32)
    return h[:, :, 0, :], h[:, :, 1, :]


def from_s16(t, amax):
    C = t.shape[-1]
    h = t.contiguous().view(torch.float16).reshape(-1, C // 32, 2, 32).float()
    return ((h[:, :, 0, :] + h[:, :, 1, :]) * (2.0 ** -s16_exp(amax))).reshape(t.shape)
