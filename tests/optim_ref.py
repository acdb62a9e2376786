"""fp64 restatement of one pass of adam_body<EMA, GUARDED> (csrc/optim.hip), its per-element fp32 error bounds, and two fp32
emulations of the device arithmetic (test infrastructure, importable without a GPU; tests/test_optim_cases_cpu.py checks all of it
from the reference alone, tests/test_optim_geometry_gpu.py holds the four kernels to it).

The update, as the kernel states it (vector loop and scalar tail alike):

    g' = g * gscale                                  m' = m * b1 + g' * (1 - b1)
    v' = v * b2 + g' * g' * (1 - b2)                 u  = lr_t * m' / (sqrtf(v') + eps)
    p' = p - u                                       e' = e - (e - p') * omd

adam_ref evaluates it in fp64 ON THE SCALARS THE KERNEL RECEIVES: lr_t, b1, b2, eps, gscale and omd are rounded to fp32 first (the
C ABI takes floats; a guarded kernel forms (float)record[4]), and 1 - b is formed from the rounded b.  1 - float32(0.9) differs from
0.1 by 2.4e-7 relative, four times the unit roundoff: a reference on the unrounded scalars would spend every bound below on that.

The bounds.  U = 2^-24 is the unit roundoff (round to nearest, results normal: tests/optim_cases.py keeps every input and every
intermediate zero or normal, so neither the denormal mode nor an underflow enters).  Every fp32 operation contributes U times the
magnitude of its own result; an error made earlier is carried along.  The library is built with -ffp-contract=fast: where a product
feeds a sum the compiler may fuse the two, which REMOVES the product's rounding and adds none, so a count made on the unfused
expression holds for every choice of fusion.  Per element, one line per rounding:

  g'   Rg    the product g * gscale: 0 where gscale is a power of two (1, 0.125: the product is exact), else 1
  1-b  r(b)  the subtraction 1.f - b: 0 for 0.5 <= b <= 1 (Sterbenz: exact; both betas of the project), else 1

  m' = A + B with A = m * b1, B = g' * (1 - b1)
       1       product A                                          on |A|
       Rg      g' inside B                                        on |B|
       r(b1)   1 - b1 inside B                                    on |B|
       1       product B                                          on |B|
       1       the sum                                            on |m'| <= |A| + |B|
       K_m = 2 + Rg + r(b1), on |A| + |B|  (A and B may cancel, so not on |m'|)                 [2 for the project's betas, gscale 1]

  v' = C + D with C = v * b2, D = (g' * g') * (1 - b2), all non-negative
       1       product C                                          on C
       2 Rg    g' twice inside D                                  on D
       1       product g' * g'                                    on D
       r(b2)   1 - b2                                             on D
       1       product with (1 - b2)                              on D
       1       the sum                                            on v'
       K_v = 3 + 2 Rg + r(b2), on v'                                                            [3 for the project's betas, gscale 1]

  u = N / den with N = lr_t * m', den = sqrtf(v') + eps, M_u = |lr_t| (|A| + |B|) / den >= |u|, w = sqrt(v') / den <= 1
       K_m     the error of m', through N                         on M_u
       1       product N                                          on M_u
       K_v/2   the error of v' through the root (d sqrt(x) / sqrt(x) = dx / 2x)        on w |u|
       R_SQRT  sqrtf                                              on w |u|
       1       the sum sqrtf(v') + eps                            on |u|
       R_DIV   the division                                       on |u|
       bound_u = U * ((K_m + 1) * M_u + ((K_v / 2 + R_SQRT) * w + 1 + R_DIV) * |u|)
       [K_u = K_m + K_v / 2 + R_SQRT + R_DIV + 2 = 9.5 on M_u where eps is invisible (w = 1), K_m + R_DIV + 2 = 6 where eps dominates]

  p' = p - u
       1       the subtraction (0 where p is 0: -u is exact)      on |p'|
       bound_p = U * |p'| + bound_u

  e' = e - (e - p') * omd, 0 <= omd <= 1
       5       the bound of tests/test_ema_gpu.py, derived in tests/test_ema_cpu.py (the difference, the product, the result; with or
               without a fused multiply-add)                      on max(|e|, |p'|)
       omd     the error of p' the update reads                   on bound_p
       bound_e = 5 * U * max(|e|, |p'|) + omd * bound_p

sqrtf and the fp32 division: the ROCm tree this suite was written against carries no HIP math-accuracy table, so each is ALLOWED
ONE ULP, R_SQRT = R_DIV = 2 (an ulp is 2^-23 relative = 2 U), although hipcc's default mode asks for the correctly rounded forms
(which would be 1 each).  Every bound is multiplied by 1 + 2^-19, which covers the second-order terms (products of at most 16
roundings: (1 + U)^16 - 1 < 16 U (1 + 2^-19)) and the fp64 roundings of the reference itself.  No K is fitted to what a device gives.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
R_SQRT = 2.0        # one ulp, in units of U
R_DIV = 2.0
SECOND_ORDER = 1.0 + 2.0 ** -19
EMA_K = 5.0         # tests/test_ema_gpu.py: ema_bound


def f32(x):
    """A host scalar as the kernel receives it: rounded to fp32, widened exactly."""
    return float(np.float32(x))


def lr_t(t, lr, b1, b2):
    """tf.train.AdamOptimizer: lr * sqrt(1 - beta2^t) / (1 - beta1^t), in double (what sgg_amd.step.tf_adam_lr_t states)."""
    return float(np.float64(lr) * np.sqrt(np.float64(1.0) - np.float64(b2) ** t) / (np.float64(1.0) - np.float64(b1) ** t))


def _f64(x):
    if x is None:
        return None
    return x.double() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


def _xp(x):
    return torch if torch.is_tensor(x) else np


def adam_terms(p, g, m, v, e, lr_t, b1, b2, eps, gscale, omd, den_of=None):
    """One step in fp64 with every intermediate the kernel forms, as a dict.  Arrays: fp32 NumPy arrays or torch tensors (widened
    exactly); e and omd may be None (the kernels without the average).  den_of: a function of v' that replaces sqrt(v') + eps - only
    for the deliberately wrong variants of tests/test_optim_cases_cpu.py."""
    xp = _xp(p)
    p, g, m, v, e = (_f64(a) for a in (p, g, m, v, e))
    lr_t, b1, b2, eps, gscale = (f32(s) for s in (lr_t, b1, b2, eps, gscale))
    t = {}
    t["g'"] = g * gscale
    t["A"], t["B"] = m * b1, t["g'"] * (1.0 - b1)
    t["m"] = t["A"] + t["B"]
    t["g'g'"] = t["g'"] * t["g'"]
    t["C"], t["D"] = v * b2, t["g'g'"] * (1.0 - b2)
    t["v"] = t["C"] + t["D"]
    t["root"] = xp.sqrt(t["v"])
    t["den"] = t["root"] + eps if den_of is None else den_of(t["v"])
    t["N"] = lr_t * t["m"]
    t["u"] = t["N"] / t["den"]
    t["p"] = p - t["u"]
    if e is not None:
        omd = f32(omd)
        t["e-p"] = e - t["p"]
        t["(e-p)omd"] = t["e-p"] * omd
        t["e"] = e - t["(e-p)omd"]
    return t


def adam_ref(p, g, m, v, e, lr_t, b1, b2, eps, gscale, omd):
    """(m', v', u, p', e') of one step in fp64 (e' is None without an average)."""
    t = adam_terms(p, g, m, v, e, lr_t, b1, b2, eps, gscale, omd)
    return t["m"], t["v"], t["u"], t["p"], t.get("e")


# ---- the bounds --------------------------------------------------------------------------------------------------------------------
def product_roundings(scale):
    """Rg: roundings of x * scale in fp32 - none where the scale is a power of two."""
    return 0 if math.frexp(f32(scale))[0] in (0.5, -0.5) else 1


def one_minus_roundings(b):
    """r(b): roundings of 1.f - b - none for 0.5 <= b <= 1 (the difference of two floats within a factor 2 of each other is exact)."""
    return 0 if 0.5 <= f32(b) <= 1.0 else 1


def k_m(b1, gscale):
    return 2 + product_roundings(gscale) + one_minus_roundings(b1)


def k_v(b2, gscale):
    return 3 + 2 * product_roundings(gscale) + one_minus_roundings(b2)


def adam_bounds(t, p, e, lr_t, b1, b2, gscale, omd):
    """Per-element bounds {"m", "v", "u", "p", "e"} on |device - reference| for the terms `t` of adam_terms (module docstring)."""
    xp = _xp(t["m"])
    p, e = _f64(p), _f64(e)
    km, kv = k_m(b1, gscale), k_v(b2, gscale)
    mag_m = xp.abs(t["A"]) + xp.abs(t["B"])
    b = {"m": km * U * mag_m, "v": kv * U * t["v"]}
    m_u = abs(f32(lr_t)) * mag_m / t["den"]
    w = t["root"] / t["den"]
    b["u"] = U * ((km + 1) * m_u + ((kv / 2.0 + R_SQRT) * w + 1.0 + R_DIV) * xp.abs(t["u"]))
    b["p"] = (p != 0) * (U * xp.abs(t["p"])) + b["u"]
    if e is not None:
        b["e"] = EMA_K * U * xp.maximum(xp.abs(e), xp.abs(t["p"])) + f32(omd) * b["p"]
    return {k: x * SECOND_ORDER for k, x in b.items()}


# ---- two fp32 emulations (NumPy, for the CPU test: both must lie inside the bounds) ------------------------------------------------
def _scalars32(*s):
    return [np.float32(x) for x in s]


def emulate_every_rounding(p, g, m, v, e, lr_t, b1, b2, eps, gscale, omd):
    """The kernel's expressions in np.float32, rounded after every operation (no contraction)."""
    lr_t, b1, b2, eps, gscale, omd = _scalars32(lr_t, b1, b2, eps, gscale, omd)
    one = np.float32(1)
    gv = g * gscale
    mv = m * b1 + gv * (one - b1)
    vv = v * b2 + gv * gv * (one - b2)
    u = lr_t * mv / (np.sqrt(vv) + eps)
    pn = p - u
    en = e - (e - pn) * omd
    assert all(a.dtype == np.float32 for a in (gv, mv, vv, u, pn, en))
    return mv, vv, u, pn, en


def emulate_fused(p, g, m, v, e, lr_t, b1, b2, eps, gscale, omd):
    """Every product that feeds a sum formed through fp64 and rounded to fp32 once with the sum (the most contraction the
    expressions allow, and more than one FMA can do for m' and v': both products unrounded).  g * gscale, lr_t * m', the root, the
    division and p - u have no sum to fuse into and are rounded as they stand."""
    lr_t, b1, b2, eps, gscale, omd = _scalars32(lr_t, b1, b2, eps, gscale, omd)
    one, d = np.float32(1), np.float64
    gv = (g * gscale).astype(d)
    mv = (m.astype(d) * d(b1) + gv * d(one - b1)).astype(np.float32)
    vv = (v.astype(d) * d(b2) + gv * gv * d(one - b2)).astype(np.float32)
    u = lr_t * mv / (np.sqrt(vv) + eps)
    pn = p - u
    en = (e.astype(d) - (e - pn).astype(d) * d(omd)).astype(np.float32)
    assert all(a.dtype == np.float32 for a in (mv, vv, u, pn, en))
    return mv, vv, u, pn, en
