"""numpy fp64 restatement of the three entry points of csrc/xent.hip (definitions in include/sgg_hip.h, "generator likelihood"),
shared by tests/test_xent_cpu.py and tests/test_xent_gpu.py."""
import numpy as np

# Tolerances, device fp32 against this fp64 restatement: 10 x the largest error measured on the MI355X over the cases of
# tests/test_xent_gpu.py, rounded up (the project's habit, tests/tolerances.py).
#   nll and lse: XENT_ERR_MEASURED = the largest |nll - ref| over the cases with |logit| <= 23: 1.33e-6 at R = 1024, V = 7 (the case
#   with the most rows; 9.70e-7 at V = 70 001; lse alone at most 8.76e-7, at V = 1003) - the 1.2e-6 of K-best's log-probabilities,
#   the same kind of sum (tests/kbest_ref.py): the lse error, its rounding (half an ulp of |lse| ~ 10 is 4.8e-7) and the rounding of
#   the subtraction.  The rows of +-80 are compared as |d| <= XENT_TOL * max(1, max|x|): measured 8.49e-6 (nll = 160.7 at V = 1000;
#   half an ulp of it is 7.6e-6).
#   gradient: XENT_GRAD_ERR_MEASURED = the largest |dlogits - ref| / scale, the error of a probability in [0, 1], over all cases, the
#   rows of +-80 included (their bound is not scaled): 6.16e-7 on the +-80 rows at V = 11, 5.65e-7 at R = 1025, V = 7 (exp(x - lse)
#   carries the lse error relatively, plus the exp's own rounding).
XENT_ERR_MEASURED = 1.33e-6
XENT_GRAD_ERR_MEASURED = 6.2e-7
XENT_TOL = 1.4e-5
XENT_GRAD_TOL = 7e-6


def lse64(x):
    """log-sum-exp over the last axis, fp64, stabilised by the maximum."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def softmax_xent(logits, labels=None, scale=1.0, accumulate=False, dlogits=None):
    """logits [R, V] (as given: float32 on the GPU side), labels int [R] or None -> dict of lse [R] and, with labels, nll [R], hit
    int32 [R] (1 / 0; -1: label outside [0, V), row skipped) and dlogits [R, V] fp64 = scale * (softmax - onehot), stored over or -
    accumulate - added to the `dlogits` given (skipped rows: zeros / what was there)."""
    x = np.asarray(logits, dtype=np.float64)
    R, V = x.shape
    lse = lse64(x)
    out = {"lse": lse}
    if labels is None:
        return out
    lab = np.asarray(labels, dtype=np.int64).reshape(R)
    valid = (lab >= 0) & (lab < V)
    safe = np.where(valid, lab, 0)
    rows = np.arange(R)
    out["nll"] = np.where(valid, lse - x[rows, safe], 0.0)
    out["hit"] = np.where(valid, (x.argmax(axis=1) == safe).astype(np.int32), -1).astype(np.int32)      # (argmax: the first maximum)
    g = np.exp(x - lse[:, None])
    g[rows, safe] -= 1.0
    g = float(scale) * g * valid[:, None]
    if accumulate:
        assert dlogits is not None
        g = np.asarray(dlogits, dtype=np.float64) + g
    out["dlogits"] = g
    return out


def xent_summary(nll, hit):
    """nll [R], hit [R] with R = 3 B, consecutive threes per triple -> [nll per valid row, token accuracy, triple accuracy, valid rows]."""
    nll, hit = np.asarray(nll, dtype=np.float64), np.asarray(hit).reshape(-1, 3)
    valid = hit >= 0
    n = int(valid.sum())
    full = valid.all(axis=1)
    return np.array([nll.reshape(-1, 3)[valid].sum() / n if n else 0.0,
                     float((hit[valid] == 1).sum()) / n if n else 0.0,
                     float((hit[full] == 1).all(axis=1).sum()) / int(full.sum()) if full.any() else 0.0,
                     float(n)])


def triple_logp(logits, lse, gt, gt_count):
    """logits [N, nb, 3, V], lse [N, nb, 3] (as given: the device's own in the GPU tests), gt int [nb, M, 3], gt_count [nb] -> dict of
    mix [nb, M], mean [nb, M], slot [nb, M, 3] (fp64; NaN where the row is not valid), status int32 [nb, M]."""
    x, z = np.asarray(logits, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    gt = np.asarray(gt, dtype=np.int64)
    N, nb, _, V = x.shape
    M = gt.shape[1]
    cnt = np.clip(np.asarray(gt_count, dtype=np.int64), 0, M)
    mix, mean = np.full((nb, M), np.nan), np.full((nb, M), np.nan)
    slot, status = np.full((nb, M, 3), np.nan), np.zeros((nb, M), dtype=np.int32)
    for j in range(nb):
        for m in range(M):
            t = gt[j, m]
            if m >= cnt[j]:
                status[j, m] = -3
            elif ((t < 0) | (t >= V)).any():
                status[j, m] = -4
            else:
                a = np.stack([x[:, j, s, t[s]] - z[:, j, s] for s in range(3)], axis=1)         # [N, 3]
                lp = (a[:, 0] + a[:, 1]) + a[:, 2]
                mx = lp.max()
                mix[j, m] = mx + (np.log(np.exp(lp - mx).sum()) - np.log(N))
                mean[j, m] = lp.mean()
                slot[j, m] = a.mean(axis=0)
    return {"mix": mix, "mean": mean, "slot": slot, "status": status}
