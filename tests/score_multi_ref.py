"""numpy fp64 restatement of the four multi-sample entry points of csrc/score.hip (definitions in include/sgg_hip.h, "score-function
update with S samples per row") on top of tests/relax_ref.py, tests/relax_hard_ref.py and tests/score_ref.py, shared by
tests/test_score_multi_cpu.py and tests/test_score_multi_gpu.py.  Layout everywhere: sample s of row r sits at index s * R + r."""
import numpy as np

from tests import relax_hard_ref as HR
from tests.xent_ref import lse64

MAX_SAMPLES = 16
BASELINES = {"none": 0, "rloo": 1, "image": 2}

# Tolerances, device fp32 against this fp64 restatement: 10 x the largest error measured on the MI355X over the cases of
# tests/test_score_multi_gpu.py (RELAX_CASES x S in {1, 3, 8} x group in {1, 3}, |x| <= 23), rounded up - the project's rule
# (tests/tolerances.py).  Each measured value must itself lie within the bound of the arithmetic it shares with softmax_xent and
# score_rows (XENT_GRAD_TOL, XENT_TOL, SCORE_ENT_TOL): a larger one is a defect of the kernel, not a tolerance to widen
# (test_the_measured_errors_lie_within_the_bounds_of_the_shared_arithmetic).
#   SCORE_MULTI_GRAD_ERR_MEASURED = the largest |dx - dx64| of the launches with ent_coef = 0, in units of |coef| sum_s |A_s| (the
#   row's weights taken absolutely: the one-hot terms of S samples are subtracted one by one from (sum_s w_s) p_j): 5.84e-7 at R = 5,
#   V = 1024, S = 3.
#   SCORE_MULTI_LOGP_ERR_MEASURED = the largest |logp - logp64| (absolute; x_a - lse): 1.667e-6 at R = 3, V = 70 001, S = 8 (lse's
#   error on a streamed row, met by more tokens the more samples there are).
#   SCORE_MULTI_ENT_ERR_MEASURED = the largest of |ent - H64| (6.892e-6) and of |dx - dx64| / ent_coef with coef = 0 (6.869e-6), both
#   at R = 6, V = 5125 - the saturated streamed row behind score_ref.SCORE_ENT_ERR_MEASURED: the arithmetic of H is score_rows'.
SCORE_MULTI_GRAD_ERR_MEASURED = 5.9e-7
SCORE_MULTI_LOGP_ERR_MEASURED = 1.67e-6
SCORE_MULTI_ENT_ERR_MEASURED = 6.9e-6
SCORE_MULTI_GRAD_TOL = 6e-6
SCORE_MULTI_LOGP_TOL = 1.7e-5
SCORE_MULTI_ENT_TOL = 7e-5


def sample_draw(draw, s):
    """The draw number of sample s: the sample's number in the eight bits above the caller's 56."""
    assert 0 <= int(draw) < 2 ** 56 and 0 <= int(s) < MAX_SAMPLES
    return int(draw) | (int(s) << 56)


def sample_rows_multi(x, S, seed=0, draw=0):
    """x [R, V] -> (tok int64 [S, R], margin fp64 [S, R]): sample s is relax_hard_ref.relax_rows_hard(x, True, seed, draw | (s << 56))."""
    assert 1 <= S <= MAX_SAMPLES
    res = [HR.relax_rows_hard(x, True, seed, sample_draw(draw, s)) for s in range(S)]
    return np.stack([r[1] for r in res]), np.stack([r[2] for r in res])


def score_advantage_multi(d_out, S, baseline="image"):
    """d_out [S * B, T] (row s * B + b: sample s of image b) -> (adv fp64 [S * B], out2 = [mean reward, mean adv^2])."""
    d = np.asarray(d_out, dtype=np.float64)
    N = d.shape[0]
    assert 1 <= S <= MAX_SAMPLES and N % S == 0
    B = N // S
    r = d.mean(axis=1)
    kind = BASELINES[baseline]
    if kind == 1:
        assert N >= 2, "the leave-one-out baseline needs S * B >= 2"
        adv = r - (r.sum() - r) / (N - 1)
    elif kind == 2:
        assert S >= 2, "the per-image baseline needs S >= 2"
        rs = r.reshape(S, B)
        adv = (rs - (rs.sum(axis=0, keepdims=True) - rs) / (S - 1)).reshape(N)
    else:
        adv = r.copy()
    return adv, np.array([r.mean(), (adv * adv).mean()])


def score_rows_multi(x, tok, adv=None, group=1, coef=1.0, ent_coef=0.0, accumulate=False, dx=None):
    """x [R, V], tok int [S, R], adv [S * (R / group)] or None -> dict of dx [R, V] fp64 (stored over or - accumulate - added to the
    `dx` given), logp [S, R] (0 where the token is outside [0, V): that sample's term is dropped, nothing else), ent [R], and
    unit [R] = sum_s |w_s| over the valid samples (the unit of the policy-gradient part's error)."""
    x = np.asarray(x, dtype=np.float64)
    R, V = x.shape
    tok = np.asarray(tok, dtype=np.int64)
    S = tok.shape[0]
    tok = tok.reshape(S, R)
    group = int(group)
    assert R % group == 0
    rows = np.arange(R)
    lse = lse64(x)
    logq = x - lse[:, None]
    p = np.exp(logq)
    H = lse - (p * x).sum(axis=1)
    g = float(ent_coef) * p * (logq + H[:, None])
    logp, unit = np.zeros((S, R)), np.zeros(R)
    for s in range(S):
        valid = (tok[s] >= 0) & (tok[s] < V)
        safe = np.where(valid, tok[s], 0)
        w = np.full(R, float(coef)) if adv is None else float(coef) * np.asarray(adv, dtype=np.float64)[s * (R // group) + rows // group]
        w = w * valid
        onehot = np.zeros((R, V))
        onehot[rows, safe] = 1.0
        g = g + w[:, None] * (p - onehot)
        logp[s] = np.where(valid, x[rows, safe] - lse, 0.0)
        unit += np.abs(w)
    if accumulate:
        assert dx is not None
        g = np.asarray(dx, dtype=np.float64) + g
    return {"dx": g, "logp": logp, "ent": H, "unit": unit}


def score_summary_multi(logp, ent):
    return np.array([np.asarray(logp, dtype=np.float64).mean(), np.asarray(ent, dtype=np.float64).mean()])
