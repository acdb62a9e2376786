"""numpy fp64 restatement of the three entry points of csrc/retrieve.hip (definitions in include/sgg_hip.h, "image retrieval by
triple query"), shared by tests/test_retrieve_cpu.py and tests/test_retrieve_gpu.py."""
import numpy as np

# Tolerances, device fp32 against this fp64 restatement (given the DEVICE's own lse): 10 x the largest error measured on the MI355X
# over the cases of tests/test_retrieve_gpu.py, the project's habit (LP_TOL of tests/kbest_ref.py is 10 x the 1.2e-6 measured for
# the same arithmetic).  Measured |query_logp - fp64| per case (N, nb, V, Q):
#     (1, 1, 7, 1)          7.45e-7   |score| up to 16.7
#     (3, 5, 1000, 257)     2.91e-5   logits uniform in +-80, |score| up to 310 (an ulp there is 3.1e-5)
#     (65, 2, 1025, 1000)   3.90e-6   |score| up to 35.4
#     (2, 2, 70000, 64)     4.90e-6   |score| up to 66.7
#     (4, 3, 1000, 4096)    5.15e-6   |score| up to 50.5
#     (3, 2, 70000, 4096)   8.04e-6   |score| up to 73.4 (an ulp there is 7.6e-6); one sample per round, every gather slot in use
#   QLP_ERR_MEASURED   the largest of them, 2.91e-5: QLP_TOL = 2.91e-4 holds for EVERY case, the +-80 one included, unscaled.
#   QLP_SMALL_ERR_MEASURED  the largest over the cases with logits 4 N(0, 1) (|score| < 128): 8.04e-6.  Those cases, and retrieve() end
#                      to end, are held to QLP_SMALL_TOL = 8.1e-5 as well - the tighter of the two bounds where the magnitudes allow it.
#   QLP_VS_TLP_MEASURED  the largest |query_logp - triple_logp's mix| on full-triple queries over the same cases: 3.81e-6 (N = 4 and
#                      the one-sample-per-round case; 1.91e-6 at N = 65; 0 at the others, the +-80 case included): the device sum
#                      is online (rescaled when the maximum rises), the existing kernel takes two passes, so the two differ by
#                      roundings of the sum only.  One flat bound for every case.
QLP_ERR_MEASURED = 2.91e-5
QLP_SMALL_ERR_MEASURED = 8.1e-6
QLP_VS_TLP_MEASURED = 3.9e-6
QLP_TOL = 2.91e-4
QLP_SMALL_TOL = 8.1e-5
QLP_VS_TLP_TOL = 3.9e-5


def query_logp(logits, lse, ids):
    """logits [N, nb, 3, V], lse [N, nb, 3] (as given: the device's own in the GPU tests), ids int [Q, 3] (tokens; -1 for a
    wildcard) -> scores fp64 [Q, nb]: log of the mixture (over the N samples) probability of the specified slots."""
    x, z = np.asarray(logits, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 3)
    N, nb, _, V = x.shape
    a = x - z[..., None]                                         # [N, nb, 3, V]
    lp = np.zeros((ids.shape[0], N, nb))
    for s in range(3):
        spec = ids[:, s] >= 0
        lp[spec] += np.transpose(a[:, :, s, :][:, :, ids[spec, s]], (2, 0, 1))      # (a wildcard adds nothing)
    m = lp.max(axis=1)
    return m + (np.log(np.exp(lp - m[:, None, :]).sum(axis=1)) - np.log(N))


def order(row):
    """The image indices of a score row in the total order (score descending, image index ascending; +0 == -0)."""
    row = np.asarray(row)
    return np.lexsort((np.arange(row.shape[0]), -row))


def topk(scores, n_images, K):
    """scores [Q, >= n_images] -> (idx int32 [Q, K], top [Q, K] in the scores' dtype): the first K of order(); -1 / NaN behind
    min(K, n_images)."""
    scores = np.asarray(scores)
    Q = scores.shape[0]
    idx = np.full((Q, K), -1, dtype=np.int32)
    top = np.full((Q, K), np.nan, dtype=scores.dtype)
    M = min(K, n_images)
    for q in range(Q):
        o = order(scores[q, :n_images])[:M]
        idx[q, :M] = o
        top[q, :M] = scores[q, o]
    return idx, top


def ranks(scores, n_images, rel_ptr, rel_idx):
    """-> dict of ranks int32 (parallel to rel_idx; 1 + the images ahead in order()), first_rank int32 [Q], ap fp64 [Q] = mean_i
    (i + 1) / rank_(i) over the ascending ranks, status int32 [Q] (0; -3 without a relevant image: first_rank 0, ap NaN)."""
    scores = np.asarray(scores)
    rel_ptr, rel_idx = np.asarray(rel_ptr, dtype=np.int64), np.asarray(rel_idx, dtype=np.int64)
    Q = scores.shape[0]
    out = {"ranks": np.zeros(int(rel_ptr[Q]), dtype=np.int32), "first_rank": np.zeros(Q, dtype=np.int32),
           "ap": np.full(Q, np.nan), "status": np.zeros(Q, dtype=np.int32)}
    for q in range(Q):
        rel = rel_idx[rel_ptr[q]:rel_ptr[q + 1]]
        if len(rel) == 0:
            out["status"][q] = -3
            continue
        pos = np.empty(n_images, dtype=np.int64)
        pos[order(scores[q, :n_images])] = np.arange(1, n_images + 1)
        r = pos[rel]
        out["ranks"][rel_ptr[q]:rel_ptr[q + 1]] = r
        out["first_rank"][q] = r.min()
        out["ap"][q] = np.mean(np.arange(1, len(r) + 1, dtype=np.float64) / np.sort(r).astype(np.float64))
    return out
