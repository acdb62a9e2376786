"""The sizes and input regimes of tests/test_optim_geometry_gpu.py: the four Adam kernels of csrc/optim.hip at the geometry of the
whole-arena pass (test infrastructure, importable without a GPU; tests/test_optim_cases_cpu.py checks every property claimed here).

The launch.  adam_launch starts grid_for(n / 4 + 1, 256) workgroups of 256 threads (at most 4096); thread i0 of the grid handles
the float4s i0, i0 + stride, ... below n4 = n >> 2 with stride = grid * 256, and threads 0 .. (n & 3) - 1 of workgroup 0 handle the
last n & 3 floats.  ONE_PASS = 4 * 256 * 4096 floats is what the capped grid covers in one trip of that loop; the arenas of the
workload (34.9 M words) take more than eight.

The regimes.  Every operand is a fixed seeded array of the regime's largest size and a case of n elements is its first n: the value
at a position does not depend on n, a misplaced element meets a value of another position, and the fp64 reference of the largest
size serves every size.  Every input and every intermediate of the reference is zero or a normal fp32 number.
"""
from collections import namedtuple

import numpy as np

from tests import optim_ref as R

BLOCK, VEC, GRID_CAP = 256, 4, 4096       # blockDim.x, floats per thread and trip (f32x4), the cap of grid_for (csrc/sgg_common.h)
ONE_PASS = VEC * BLOCK * GRID_CAP
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-4, 0.5, 0.9, 1e-8      # sgg_amd/params.py (compared by the tests)
OMDS = (0.9, 1e-3)                        # one_minus_decay of the kernels that keep the average
# beta1 = 0.5 makes m * b1 + g' * (1 - b1) symmetric in b1 and 1 - b1, and 1.f - b is exact for 0.5 and 0.9: one small case each with
# betas above 0.5 that are no fp32 numbers, and with betas below 0.5 (1.f - b rounds)
OTHER_BETAS = [(0.8, 0.99), (0.3, 0.45)]
OTHER_BETAS_N = VEC * BLOCK * 3 + 3       # four workgroups and a tail


def cdiv(a, b):
    return -(-a // b)


def grid(n):
    return max(1, min(cdiv(n // VEC + 1, BLOCK), GRID_CAP))


def trips(n):
    """the most trips of the float4 loop a thread makes"""
    return cdiv(n // VEC, grid(n) * BLOCK)


def last_trip_groups(n):
    """workgroups with at least one thread on that last trip"""
    t = trips(n)
    return cdiv(n // VEC - (t - 1) * grid(n) * BLOCK, BLOCK) if t else 0


def geometry(n):
    return Size(n, grid(n), trips(n), last_trip_groups(n), n % VEC)


# n, workgroups, most trips of a thread, workgroups on the last trip, tail floats
Size = namedtuple("Size", "n grid trips last_trip_groups tail")
THIRD_TRIP = 2 * ONE_PASS + VEC * BLOCK * 5 + 1
SIZES = [
    Size(1, 1, 0, 0, 1), Size(2, 1, 0, 0, 2), Size(3, 1, 0, 0, 3),          # the tail alone
    Size(4, 1, 1, 1, 0), Size(5, 1, 1, 1, 1), Size(7, 1, 1, 1, 3),          # one float4, then a tail behind it
    Size(1023, 1, 1, 1, 3),                                                  # 255 float4s: the last thread of the only workgroup idles
    Size(1024, 2, 1, 1, 0), Size(1025, 2, 1, 1, 1), Size(1027, 2, 1, 1, 3), # n / 4 + 1 = 257: a second workgroup with no float4 - the tail must
                                                                             # still be workgroup 0's alone
    Size(ONE_PASS - 1, GRID_CAP, 1, GRID_CAP, 3),                            # the cap is reached, the grid's last thread idles
    Size(ONE_PASS, GRID_CAP, 1, GRID_CAP, 0),                                # every thread exactly one trip
    Size(ONE_PASS + 3, GRID_CAP, 1, GRID_CAP, 3),                            # ... and a tail behind a full pass: still no second trip
    Size(THIRD_TRIP, GRID_CAP, 3, 5, 1),                                     # two full trips, a third that 5 workgroups make, a tail
]
LARGEST = ONE_PASS + 3


# ---- regimes ---------------------------------------------------------------------------------------------------------------------
# name, Adam step t (lr_t = R.lr_t(t)), gradient scale of the plain kernels, record[4] of the guarded ones (a double: the kernel
# forms (float)record[4]), whether the third-trip size runs
Regime = namedtuple("Regime", "name t gscale record4 third_trip")
REGIMES = [
    Regime("a_typical", 3, 1.0, 1.0, True),            # the ranges of adam_inputs in tests/test_ema_gpu.py
    Regime("b_p_zero", 3, 1.0, 1.0, False),            # p = 0: p' = -u exactly, the update itself at a few ulps
    Regime("c_first_step", 1, 1.0, 1.0, True),         # m = v = 0, t = 1, |g| log-uniform in [1e-15, 1e2]: sqrt(v') falls through eps
    Regime("d_zeros", 3, 1.0, 1.0, False),             # g = m = v = 0 on a third of the elements: u is exactly 0 there
    Regime("e_scale_eighth", 3, 0.125, 0.125, False),  # an exact gradient scale
    Regime("e_scale_third", 3, float(np.float32(1.0 / 3.0)), 1.0 / 3.0, False),     # one more rounding; the record holds the double
    Regime("f_late_step", 1000, 1.0, 1.0, False),      # lr_t of t = 1000, v up to 1e8, |g| up to 1e4, |m| up to 1e3
]
BY_NAME = {r.name: r for r in REGIMES}
# Regime c: where the placement of eps shows.  For 1e-9 <= |g| <= 1e-6 the root sqrt(v') = 0.316 |g| lies between 0.03 eps and 32 eps:
# eps inside the root (den = sqrt(v' + eps) ~ 1e-4) and eps scaled by sqrt(1 - b2^t) = 0.316 both change u by more than 2 % of
# lr = 1e-4 there, against a bound of about 6e-8 |p'| <= 6e-8.
EPS_G_RANGE = (1e-9, 1e-6)


def largest(regime):
    return THIRD_TRIP if regime.third_trip else LARGEST


def sizes(regime):
    return [s for s in SIZES if s.n <= largest(regime)]


def hyper(regime):
    """(lr_t, b1, b2, eps) as the host passes them: doubles, rounded to fp32 at the C ABI"""
    return (R.lr_t(regime.t, ADAM_LR, ADAM_B1, ADAM_B2), ADAM_B1, ADAM_B2, ADAM_EPS)


def zero_mask(n):
    """Regime d: a seeded third of the positions, the first float4, and the last float4 and tail of every size of the list."""
    mask = np.random.RandomState(4242).rand(n) < 1.0 / 3.0
    mask[:VEC] = True
    for s in SIZES:
        if s.n <= n:
            mask[max(0, VEC * (s.n // VEC) - VEC):s.n] = True
    return mask


_master = {}


def operands(regime, n=None):
    """(p, g, m, v, e) of the regime: fp32 arrays, the first n elements of the regime's fixed arrays (views: do not write)."""
    if regime.name not in _master:
        _master.clear()                         # (one regime at a time: the largest holds 5 x 34 MB)
        _master[regime.name] = _build(regime)
    ops = _master[regime.name]
    return ops if n is None else tuple(a[:n] for a in ops)


def _build(regime):
    N = largest(regime)
    r = np.random.RandomState(1000 + REGIMES.index(regime))
    sign = lambda: np.where(r.rand(N) < 0.5, -1.0, 1.0)
    log_uniform = lambda lo, hi: 10.0 ** r.uniform(np.log10(lo), np.log10(hi), N)
    p = sign() * r.uniform(1e-3, 1.0, N)
    g = sign() * r.uniform(1e-4, 8.0, N)
    m = sign() * r.uniform(1e-6, 1e-2, N)
    v = r.uniform(1e-10, 1e-3, N)
    e = sign() * r.uniform(1e-3, 1.0, N)
    kind = regime.name[0]
    if kind == "b":
        p = np.zeros(N)
    elif kind == "c":
        g = sign() * log_uniform(1e-15, 1e2)
        m, v = np.zeros(N), np.zeros(N)
    elif kind == "d":
        z = zero_mask(N)
        g[z] = m[z] = v[z] = 0.0
    elif kind == "f":
        g = sign() * log_uniform(1e-2, 1e4)
        m = sign() * log_uniform(1e-3, 1e3)
        v = log_uniform(1e-2, 1e8)
    out = tuple(a.astype(np.float32) for a in (p, g, m, v, e))
    for a in out:
        a.setflags(write=False)
    return out


def reference(regime, n=None):
    """(terms, {omd: e' terms}, bounds, {omd: bound of e'}) of the regime in fp64 for its first n elements (default: all)."""
    p, g, m, v, e = operands(regime, n)
    lr_t, b1, b2, eps = hyper(regime)
    t = R.adam_terms(p, g, m, v, None, lr_t, b1, b2, eps, regime.gscale, None)
    b = R.adam_bounds(t, p, None, lr_t, b1, b2, regime.gscale, None)
    avg, avg_bound = {}, {}
    for omd in OMDS:
        e64 = e.astype(np.float64)
        d = e64 - t["p"]
        prod = d * R.f32(omd)
        avg[omd] = {"e-p": d, "(e-p)omd": prod, "e": e64 - prod}
        avg_bound[omd] = (R.EMA_K * R.U * np.maximum(np.abs(e64), np.abs(t["p"])) + R.f32(omd) * b["p"] / R.SECOND_ORDER) * R.SECOND_ORDER
    return t, avg, b, avg_bound
