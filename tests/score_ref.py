"""numpy fp64 restatement of the three entry points of csrc/score.hip (definitions in include/sgg_hip.h, "score-function generator
update"), shared by tests/test_score_cpu.py and tests/test_score_gpu.py."""
import numpy as np

from tests.xent_ref import XENT_GRAD_TOL, XENT_TOL, lse64  # noqa: F401  (the project's bounds for the arithmetic score_rows shares with softmax_xent)

# Tolerances, device fp32 against this fp64 restatement.
#   logp = x_a - lse and the policy-gradient part of dx, w (softmax - onehot), are softmax_xent's arithmetic: XENT_TOL, and
#   XENT_GRAD_TOL in units of |w|.
#   ent and the entropy part of dx (in units of |ent_coef|) have bounds of their own: 10 x the largest error measured on the MI355X over
#   the cases of tests/test_score_gpu.py (RELAX_CASES, |x| <= 23), rounded up - the project's habit (tests/tolerances.py).  Each measured
#   value must itself lie within XENT_TOL (a reading of the fp32 arithmetic gives about 6e-6: the error of lse and of sum p x, each a few
#   ulp of a number up to 30): a larger one is a defect of the kernel, not a tolerance to widen.
#   SCORE_ENT_ERR_MEASURED = the largest |ent - H64|: 6.89e-6 at R = 6, V = 5125 (streamed rows: H = lse - sum p x, two numbers near 22
#   on the saturated row; 3.61e-6 at V = 1027, 2.93e-6 at V = 70 001); the resident rows, which take the maximum out of both terms,
#   stay below 2.2e-7.  SCORE_ENT_GRAD_ERR_MEASURED = the largest |dx - dx64| / ent_coef of the launches with coef = 0 (the entropy part
#   alone, p ((x - lse) + H)): 6.87e-6 at the same case - H's error on the saturated row, where p is 1; resident rows below 6.5e-7.
SCORE_ENT_ERR_MEASURED = 6.9e-6
SCORE_ENT_GRAD_ERR_MEASURED = 6.9e-6
SCORE_ENT_TOL = 7e-5
SCORE_ENT_GRAD_TOL = 7e-5
# score_advantage: T fp32 additions, the division, the final rounding to fp32 - relative to max(1, max|d_out|)
SCORE_ADV_TOL = 2e-6
SCORE_OUT2_TOL = 4e-6
# score_summary: fp64 sums, one rounding to fp32 - relative to max|value|
SCORE_SUMMARY_TOL = 1e-6

BASELINES = {"none": 0, "rloo": 1}


def score_advantage(d_out, baseline="rloo"):
    """d_out [B, T] -> (adv fp64 [B], out2 = [mean reward, mean adv^2]).  "none": adv = r; "rloo": r_b minus the mean of the others."""
    d = np.asarray(d_out, dtype=np.float64)
    B = d.shape[0]
    r = d.mean(axis=1)
    if BASELINES[baseline]:
        assert B >= 2, "the leave-one-out baseline needs B >= 2"
        adv = r - (r.sum() - r) / (B - 1)
    else:
        adv = r.copy()
    return adv, np.array([r.mean(), (adv * adv).mean()])


def score_rows(x, tok, adv=None, group=1, coef=1.0, ent_coef=0.0, accumulate=False, dx=None):
    """x [R, V], tok int [R], adv [ceil(R / group)] or None -> dict of dx [R, V] fp64 (stored over or - accumulate - added to the `dx`
    given; rows whose token is outside [0, V): zeros / what was there), logp [R] (0 on such rows), ent [R]."""
    x = np.asarray(x, dtype=np.float64)
    R, V = x.shape
    tok = np.asarray(tok, dtype=np.int64).reshape(R)
    valid = (tok >= 0) & (tok < V)
    safe = np.where(valid, tok, 0)
    rows = np.arange(R)
    lse = lse64(x)
    logq = x - lse[:, None]
    p = np.exp(logq)
    H = lse - (p * x).sum(axis=1)
    w = np.full(R, float(coef)) if adv is None else float(coef) * np.asarray(adv, dtype=np.float64)[rows // int(group)]
    onehot = np.zeros((R, V))
    onehot[rows, safe] = 1.0
    g = w[:, None] * (p - onehot) + float(ent_coef) * p * (logq + H[:, None])
    g = g * valid[:, None]
    if accumulate:
        assert dx is not None
        g = np.asarray(dx, dtype=np.float64) + g
    return {"dx": g, "logp": np.where(valid, x[rows, safe] - lse, 0.0), "ent": H}


def score_summary(logp, ent):
    return np.array([np.asarray(logp, dtype=np.float64).mean(), np.asarray(ent, dtype=np.float64).mean()])
