"""fp64 references and derived fp32 error bounds of tests/test_loss_geometry_gpu.py (test infrastructure, importable without a GPU).

The references are oracle/kernels_ref.py's where it has the operation (interpolate, gp_fwd, gp_bwd, wgan_losses, spatial means),
called on fp64 copies of the fp32 inputs and returning new tensors; onehot (labels outside [0, V)) and absmax are written here.
tests/test_loss_cases_cpu.py checks all of them against plain loops.

The bounds count the roundings on the longest path of the fp32 computation, U = 2^-24 each (round to nearest; the library is built
with -ffp-contract=fast, a fused multiply-add only REMOVES a rounding; sqrtf and the division are correctly rounded in the build's
default mode).  A sum of m values through `a` additions has an error of at most a * U * sum|x_i| (first order; every bound below
carries one spare U for the second-order terms).  None of them is fitted to what the kernels give.
"""
import torch

from oracle.kernels_ref import RefKernels
from tests import loss_cases as LC

U = 2.0 ** -24
F64 = torch.float64
_ref = RefKernels()


# ---- references ------------------------------------------------------------------------------------------------------------------
def onehot(labels, V):
    """tf.one_hot: a label outside [0, V) gives an all-zero row."""
    idx = torch.arange(V, dtype=torch.int64)
    return (labels.reshape(-1, 1) == idx).to(F64).reshape(*labels.shape, V)


def absmax(x, prev):
    """max(prev, max |x|) over the non-NaN elements (fmaxf returns its other operand for a NaN): fp32 values, no rounding."""
    a = x.double().abs()
    a = a[~torch.isnan(a)]
    return max(float(prev), float(a.max()) if a.numel() else 0.0)


def interpolate(real, fake, alpha):
    out = torch.empty(real.shape, dtype=F64)
    _ref.interpolate(real.double(), fake.double(), alpha.double(), out)
    return out


def gp_fwd(g):
    B = g.shape[0]
    slopes, pen = torch.empty(B, dtype=F64), torch.empty(B, dtype=F64)
    _ref.gp_fwd(g.double(), slopes, pen)
    return slopes, pen


def gp_bwd(g, slopes, pen, scale):
    v = torch.empty(g.shape, dtype=F64)
    _ref.gp_bwd(g.double(), slopes.double(), pen.double(), v, scale)
    return v


def wgan_losses(d_out, pen, lam, B, T, has_real):
    out = torch.empty(4, dtype=F64)
    _ref.wgan_losses(d_out.double(), None if pen is None else pen.double(), lam, B, T, has_real, out)
    return out


def spatial_mean_fwd(ctx, R):
    out_c, out_h = torch.empty((R, ctx.shape[2]), dtype=F64), torch.empty((R, ctx.shape[2]), dtype=F64)
    _ref.spatial_mean_fwd(ctx.double(), out_c, out_h)
    assert torch.equal(out_c, out_h)
    return out_c


def spatial_mean_bwd(dc0, dh0, dctx0, shape):
    """dctx0 None: overwrite mode; (B, L, C) = shape"""
    d = torch.zeros(shape, dtype=F64) if dctx0 is None else dctx0.double().clone()
    _ref.spatial_mean_bwd(dc0.double(), dh0.double(), d, dctx0 is not None)
    return d


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
def interpolate_bound(real, fake, alpha):
    """out = r + a * (f - r): the difference (1 rounding, relative to |f - r|), the product (1, removed by an FMA), the sum (1, relative
    to |out| <= |r| + |a| |f - r|): |d| <= U (2 |a| |f - r| + |r| + |a| |f - r|) <= 3 U (|r| + |a| |f - r|); 4 with the spare one."""
    a = alpha.double().reshape(-1, *([1] * (real.dim() - 1)))
    return 4 * U * (real.double().abs() + a.abs() * (fake.double() - real.double()).abs())


def slope_rel_bound(n):
    """sqrt(s + 1e-10), s an fp32 sum of n squares: a thread squares (1 rounding without FMA) and adds cdiv(n, 256) terms, wave_sum adds
    6 levels, block_sum_256 3 more, + 1e-10f adds once: every (non-negative) term passes through at most t + 11 roundings, t =
    cdiv(n, 256), so s is off by (t + 11) U relative; the square root halves that and rounds once; pen = slope - 1 rounds once more
    (by at most U * |pen| < U * slope), and one spare: ((t + 11) / 2 + 3) U, relative to the slope, for the slope AND, as an absolute
    bound, for pen."""
    return ((LC.block_trips(n) + 11) / 2.0 + 3) * U


GP_BWD_REL = 6 * U      # coef = scale * (2 / B) * pen / slope (a division, a product, a product, a division), then coef * g: 5 roundings + 1


def wgan_bounds(d_out, pen, lam, B, T, has_real):
    """Absolute bounds of out[0..3].  A mean of B*T values: t = cdiv(B*T, 256) additions in a thread, 6 in the wave, 3 over the waves,
    the division: (t + 10) U * mean|x|, stated on M = max(mean|fake|, mean|real|) (= max(|mf|, |mr|) for outputs of one sign, the
    critic's N(16, 1)); mf - mr adds both and rounds once (U |mf - mr| <= 2 U M).  gp = mean(pen^2): the square, tp + 9 additions,
    the division, relative to gp.  out[0] = (mf - mr) + lam * gp: the product and the sum round once each."""
    n = B * T
    flat = d_out.double().reshape(-1)
    af = float(flat[:n].abs().mean())
    ar = float(flat[n:2 * n].abs().mean()) if has_real else 0.0
    M = max(af, ar)
    t = LC.block_trips(n)
    b3 = (t + 11) * U * af
    b1 = (2 * (t + 10) + 3) * U * M if has_real else b3
    gp = float((pen.double() ** 2).mean()) if pen is not None else 0.0
    b2 = (LC.block_trips(B) + 12) * U * gp
    b0 = b1 + abs(lam) * b2 + 2 * U * (abs(lam) * gp + 2 * M)
    return [b0, b1, b2, b3]


def sm_fwd_bound(ctx):
    """mean over L: a row group adds cdiv(L, 8) rows, 7 additions over the groups, 1 / L rounds, the product rounds, one spare:
    (cdiv(L, 8) + 10) U * mean_l |ctx|, per (b, c).  Measured at L = 784 (108 U): 2.2e-8 under a bound of 5.1e-6 at that element, the
    only comparison of the file whose bound exceeds 100 x the measured error (the roundings of 98 additions do not line up); at
    L = 5 .. 196 the largest error is 0.02 .. 0.21 of the bound.  The bound stays as derived."""
    L = ctx.shape[1]
    return (LC.cdiv(L, LC.SM_RG) + 10) * U * ctx.double().abs().mean(dim=1)


def sm_bwd_bound(dc0, dh0, dctx0, shape):
    """update = (1 / L) sum_p (dc0 + dh0): each of the 2 * npass terms passes through at most npass + 1 additions, 1 / L and the product
    round once each, one spare: (npass + 4) U * A, A = (1 / L) sum_p (|dc0| + |dh0|) >= |update| (the sum may cancel, its rounding
    does not).  Accumulating rounds once more, relative to |dctx0 + update|: (npass + 5) U (|dctx0| + A).  Per element."""
    B, L, C = shape
    npass = dc0.shape[0] // B
    A = (dc0.double().abs() + dh0.double().abs()).reshape(npass, B, C).sum(dim=0)[:, None, :].expand(B, L, C) / L
    if dctx0 is None:
        return (npass + 4) * U * A
    return (npass + 5) * U * (dctx0.double().abs() + A)
