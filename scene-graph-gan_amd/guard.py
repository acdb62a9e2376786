"""Guarded optimiser updates: the host side (settings, the record's layout and an fp64 restatement; no device code).

Two controls of an update, both decided from one reduction over the whole gradient arena and both off by default:

    clipping by the global norm   the gradient is scaled by coef = max_norm / norm where norm = ||g * grad_scale|| exceeds max_norm;
    the non-finite skip           an update whose gradient holds an Inf or NaN is dropped: parameters, both Adam moments and the
                                  weight average keep every bit.

The device takes the decision (csrc/guard.hip, HipKernels.grad_guard) and leaves it in a record of eight doubles that the guarded
Adam pass (csrc/optim.hip) reads from device memory (HipKernels.adam_guarded / adam_ema_guarded); step.Network holds the record.
The host never reads it on the training path.

    [0] ss      sum over the finite elements of ((double)x)^2, x = g * grad_scale formed in fp32 as the Adam pass forms it
    [1] bad     number of non-finite x (they enter no sum)
    [2] norm    sqrt(ss)
    [3] coef    max_norm / norm if max_norm > 0 and norm > max_norm, else EXACTLY 1.0
    [4] s_eff   (double)(float)(grad_scale * coef): the gradient scale the Adam pass applies
    [5] apply   0.0 if skip_nonfinite and bad > 0, else 1.0
    [6] clipped updates so far (coef < 1 and applied)         [7] skipped updates so far

coef is exactly 1 while the threshold is not exceeded - not TF's clip_norm * min(1 / norm, 1 / clip_norm), which is within an ulp of
it - so a run whose threshold is never reached is bit-identical to an unguarded one.
"""
from __future__ import annotations

import math

import numpy as np

FIELDS = ("ss", "nonfinite", "norm", "coef", "s_eff", "apply", "clipped", "skipped")
NREC = len(FIELDS)


def check_settings(max_norm=0.0, skip_nonfinite=False):
    """(max_norm as float, skip_nonfinite as bool); ValueError unless max_norm is finite and >= 0 (0 = no clipping)."""
    try:
        x = float(max_norm)
    except (TypeError, ValueError):
        raise ValueError("clip norm must be a number (got %r)" % (max_norm,))
    if not math.isfinite(x) or x < 0.0 or x > float(np.finfo(np.float32).max):     # (the kernel receives it as fp32)
        raise ValueError("clip norm must be finite (in fp32) and >= 0, 0 meaning off (got %r)" % (max_norm,))
    return x, bool(skip_nonfinite)


def parse_clip_grad_norm(text):
    """--clip_grad_norm X[,Y] -> (critic's max_norm, generator's max_norm): one number applies to both networks, two numbers are the
    critic's, then the generator's; 0 means off.  ValueError for anything else (negative, NaN, Inf, three numbers, no number)."""
    if isinstance(text, (int, float)):
        parts = [text]
    else:
        parts = [p.strip() for p in str(text).split(",")]
    if not 1 <= len(parts) <= 2 or any(p == "" for p in parts):
        raise ValueError("clip_grad_norm takes X or X,Y (critic, generator); got %r" % (text,))
    vals = [check_settings(p)[0] for p in parts]
    return (vals[0], vals[-1])


def decide(ss, bad, grad_scale, max_norm, skip_nonfinite):
    """Fields [2..5] of the record from [0..1], operation for operation as the device forms them: fp64 sqrt and division (both
    correctly rounded), grad_scale and max_norm as the fp32 values the kernel receives, s_eff rounded to fp32 once.
    Returns (norm, coef, s_eff, apply) as Python floats."""
    ss, gs, mx = np.float64(ss), np.float64(np.float32(grad_scale)), np.float32(max_norm)
    norm = np.sqrt(ss)
    coef = np.float64(mx) / norm if (mx > 0 and norm > np.float64(mx)) else np.float64(1.0)
    with np.errstate(over="ignore"):
        s_eff = np.float64(np.float32(gs * coef))
    apply = 0.0 if (skip_nonfinite and bad > 0) else 1.0
    return float(norm), float(coef), float(s_eff), apply


def reference_record(g, grad_scale, max_norm, skip_nonfinite, prev=None):
    """fp64 restatement of one sgg_grad_guard call on the fp32 array g: the eight fields as a float64 array.  x = g * grad_scale is
    formed in fp32 (as the device does), squares and their sum in fp64 (NumPy's pairwise order: within n * 2^-52 * ss of any other
    order, all summands being non-negative).  prev: the record before the call (its counters [6], [7] are carried; default zeros)."""
    max_norm, skip_nonfinite = check_settings(max_norm, skip_nonfinite)
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        x = g * np.float32(grad_scale)
    finite = np.isfinite(x)
    x64 = x[finite].astype(np.float64)
    ss, bad = float(np.sum(x64 * x64)), float(x.size - int(finite.sum()))
    norm, coef, s_eff, apply = decide(ss, bad, grad_scale, max_norm, skip_nonfinite)
    rec = np.zeros(NREC, dtype=np.float64) if prev is None else np.array(prev, dtype=np.float64).reshape(NREC).copy()
    rec[:6] = (ss, bad, norm, coef, s_eff, apply)
    if coef < 1.0 and apply != 0.0:
        rec[6] += 1.0
    if apply == 0.0:
        rec[7] += 1.0
    return rec


def report(rec, max_norm, skip_nonfinite):
    """The record as a dict (Network.guard_report): counts as ints, apply as bool, plus the settings in force."""
    r = [float(x) for x in rec]
    return {"ss": r[0], "norm": r[2], "coef": r[3], "s_eff": r[4], "nonfinite": int(r[1]), "apply": bool(r[5] != 0.0), "clipped": int(r[6]),
            "skipped": int(r[7]), "max_norm": float(max_norm), "skip_nonfinite": bool(skip_nonfinite)}
