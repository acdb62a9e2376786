"""numpy fp64 reference of K-best decoding (csrc/kbest.hip; definitions in include/sgg_hip.h), shared by tests/test_kbest_cpu.py and
tests/test_kbest_gpu.py.

Order of the tokens of a slot: (logit descending, token ascending).  Order of triples: (lp descending, then the tuple of slot ranks
(i, j, l) ascending lexicographically), lp = (a_0 + a_1) + a_2 with a_t = logit - lse_t."""
import numpy as np

# Tolerance on log-probabilities, device fp32 against this fp64 reference: 10 x the largest error measured on the MI355X over the
# cases of tests/test_kbest_gpu.py (the project's habit, tests/tolerances.py).  Measured (LP_ERR_MEASURED): 1.20e-6, logp of
# kbest_triples at R = 70, V = 40, K = 128 (1.17e-6 at V = 70 000; lse at most 6.5e-7; the scores of kbest_merge at most 1.04e-6
# against their bound of 2 x LP_TOL).  The same arithmetic in numpy fp32 on the CPU errs by at most 8e-7 on such inputs; the a-priori
# bound is three roundings of |a| <= 60 plus the lse error, about 1e-5, and whatever is measured the tolerance may not exceed
# LP_TOL_CAP for |logit| <= 22: above that the cause is a bug, not rounding.
LP_ERR_MEASURED = 1.2e-6
LP_TOL = 10 * LP_ERR_MEASURED
LP_TOL_CAP = 1e-4
assert LP_TOL <= LP_TOL_CAP


def lse64(x):
    """log-sum-exp over the last axis, fp64, stabilised by the maximum."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def slot_order(x):
    """tokens of one slot, x [V] float32, in rank order: logit descending, ties by the smaller token."""
    x = np.asarray(x)
    return np.lexsort((np.arange(x.shape[0]), -x))


def _ranked_cube(x, K, M):
    """x [3, V] float32 -> (triples [K, 3], lp [K] fp64, ranks [K, 3]) over the cube of the top M tokens of every slot."""
    x = np.asarray(x, dtype=np.float32)
    a = x.astype(np.float64) - lse64(x)[:, None]
    top = [slot_order(x[s])[:M] for s in range(3)]
    cube = (a[0, top[0]][:, None, None] + a[1, top[1]][None, :, None]) + a[2, top[2]][None, None, :]
    flat = np.argsort(-cube.ravel(), kind="stable")[:K]          # ties: flat index = lexicographic (i, j, l)
    i, j, l = np.unravel_index(flat, cube.shape)
    return np.stack([top[0][i], top[1][j], top[2][l]], axis=1).astype(np.int64), cube.ravel()[flat], np.stack([i, j, l], axis=1)


def kbest_row(x, K):
    """The K best triples of one row from the cube of its top M = min(K, V) tokens per slot (all that can take part)."""
    return _ranked_cube(x, K, min(int(K), np.asarray(x).shape[1]))


def brute_force_row(x, K):
    """The same by ranking all V^3 triples."""
    return _ranked_cube(x, K, np.asarray(x).shape[1])


def direct_candidate_count(K):
    return sum(1 for i in range(K) for j in range(K) for l in range(K) if (i + 1) * (j + 1) * (l + 1) <= K)


def pack(t):
    t = np.asarray(t, dtype=np.int64)
    return (t[..., 0] << 42) | (t[..., 1] << 21) | t[..., 2]


def merge_image(lists, logits, lse, K=None):
    """One image: lists int64 [N, Kc, 3] (the per-sample lists), logits float32 [N, 3, V], lse [N, 3] (as given: the device's own
    in the GPU tests) -> the merged ranked distinct list in fp64, cut at K (default: all): dict of triples [U, 3], scores, best_sample,
    best_logp, counts, n_distinct (before the cut), and gap2 [U]: the difference between the two largest lp_k of each triple (inf
    with one sample), which says where best_sample is decided."""
    lists = np.asarray(lists, dtype=np.int64)
    N = lists.shape[0]
    x, z = np.asarray(logits, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    keys, counts = np.unique(pack(lists.reshape(-1, 3)), return_counts=True)         # ascending packed triple
    t = np.stack([keys >> 42, (keys >> 21) & ((1 << 21) - 1), keys & ((1 << 21) - 1)], axis=1)
    lp = ((x[:, 0, t[:, 0]] - z[:, 0:1]) + (x[:, 1, t[:, 1]] - z[:, 1:2])) + (x[:, 2, t[:, 2]] - z[:, 2:3])     # [N, U]
    m = lp.max(axis=0)
    score = m + np.log(np.exp(lp - m).sum(axis=0)) - np.log(N)
    srt = np.sort(lp, axis=0)
    gap2 = srt[-1] - srt[-2] if N > 1 else np.full(m.shape, np.inf)
    order = np.argsort(-score, kind="stable")                                         # ties: packed triple ascending
    cut = order[:K]
    return {"triples": t[cut], "scores": score[cut], "best_sample": lp.argmax(axis=0)[cut].astype(np.int32), "best_logp": m[cut],
            "counts": counts[cut].astype(np.int32), "n_distinct": int(len(keys)), "gap2": gap2[cut], "all_scores": score[order]}
