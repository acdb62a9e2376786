"""numpy fp64 restatement of the straight-through pair of csrc/relax.hip (sgg_relax_rows_hard, sgg_relax_rows_hard_bwd; definitions in
include/sgg_hip.h) on top of tests/relax_ref.py: the one-hot row of the first argmax of x + g, and the gradient of the soft row
y = softmax((x + g) / tau) rebuilt from x and the noise.  Shared by tests/test_relax_hard_cpu.py and tests/test_relax_hard_gpu.py."""
import numpy as np

from tests import relax_ref as RR

# The forward is exact: the device's token must BE the restatement's wherever the restatement's top-2 gap of x + g is far above the
# fp32 error of that sum (|x| <= 23, g in (-2.9, 16.7): one rounding of a number below 64 is at most 2^-19 = 1.9e-6, the fp32 g is up
# to 16 ulp = 8e-6 off near u -> 1 where g is large).  The tests assert the gap on every row rather than leave rows out.
HARD_MARGIN_MIN = 1e-3
# Backward, device fp32 against this restatement, in units of max|dy| * scale / tau (absolute in that unit, as RELAX_GRAD_TOL is): the
# soft row is recomputed in fp32 inside the kernel, so the forward's error (relax_ref.RELAX_ERR_MEASURED) enters on top of the dot
# product's.  HARD_GRAD_ERR_MEASURED = the largest error measured on the MI355X over RELAX_CASES x tau in {1.0, 0.25} x both modes:
# 1.746e-7 at R = 6, V = 5125, tau 0.25 with Gumbel noise (1.58e-7 at V = 70 001, 1.45e-7 at R = 1025, V = 7, both at tau 0.25 with
# noise; without noise at most 8.6e-8, at V = 7; at tau 1 at most 1.3e-7).  The tolerance is 10 x that, rounded up - the project's
# margin (tests/tolerances.py).  A measured error above 1e-5 in that unit is a defect, not a reason for a wider tolerance.
# Against the device's own soft pair relax_rows_bwd(relax_rows(x), dy) the largest difference measured is 3.1e-8 (V = 5125; resident
# rows: 0, the same arithmetic in the same order); the tests allow twice the tolerance there.
HARD_GRAD_ERR_MEASURED = 1.8e-7
HARD_GRAD_TOL = 1.8e-6


def relax_rows_hard(x, gumbel_noise=False, seed=0, draw=0):
    """x [R, V] -> (y [R, V] fp64 one-hot, tok int64 [R], margin fp64 [R] = the top-2 gap of x + g; inf where V = 1).  The first index
    on ties (np.argmax)."""
    s = np.asarray(x, dtype=np.float64)
    if gumbel_noise:
        s = s + RR.gumbel(RR.uniforms(seed, draw, s.shape[0], s.shape[1]))
    tok = s.argmax(axis=1).astype(np.int64)
    y = np.zeros_like(s)
    y[np.arange(s.shape[0]), tok] = 1.0
    if s.shape[1] == 1:
        margin = np.full(s.shape[0], np.inf)
    else:
        top2 = np.partition(s, s.shape[1] - 2, axis=1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
    return y, tok, margin


def relax_rows_hard_bwd(x, dy, tau, scale=1.0, gumbel_noise=False, seed=0, draw=0):
    """dx_j = (scale / tau) * y_j * (dy_j - sum_k y_k dy_k) with y = softmax((x + g) / tau), fp64."""
    y, _ = RR.relax_rows(x, tau, gumbel_noise, seed, draw)
    return RR.relax_rows_bwd(y, dy, tau, scale)
