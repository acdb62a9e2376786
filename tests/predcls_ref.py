"""The fp64 reference of predicate classification (sgg_amd/predcls.py states it; csrc/predcls.hip follows it) and the tolerances,
shared by tests/test_predcls_cpu.py and tests/test_predcls_gpu.py."""
import numpy as np

from sgg_amd.predcls import (candidate_pairs, gt_pair_index, merge_reference, pair_chunk, pair_predicate_reference,  # noqa: F401
                             pair_topk_reference, token_order)

# Tolerances, device fp32 against the fp64 reference (given the DEVICE's own lse, as tests/xent_ref.py and tests/retrieve_ref.py
# take it): 10 x the largest error measured on the MI355X over the cases of tests/test_predcls_gpu.py, the project's habit (LP_TOL
# of tests/kbest_ref.py).  Measured |joint - ref|, |marg - ref|, |logsumexp_v cond| per case (N, nb, V, P):
#     (1, 1, 1, 1)         0         0         0
#     (3, 2, 7, 3)         8.34e-7   1.63e-7   4.51e-7   |joint| up to 14.5
#     (65, 2, 1000, 17)    4.19e-6   1.24e-6   1.12e-6   |joint| up to 37.6
#     (5, 3, 257, 65)      5.68e-6   1.71e-6   2.03e-6   |joint| up to 44.9
#     (2, 1, 70000, 2)     1.17e-5   1.96e-6   3.83e-6   |joint| up to 73.3 (an ulp there is 7.6e-6)
#     (4, 2, 300, 20)      3.77e-5   1.49e-5   1.66e-5   logits uniform in +-80, |joint| up to 324.6 (an ulp there is 3.1e-5)
#   PCLS_ERR_MEASURED        the largest of them, 3.77e-5: PCLS_TOL = 3.77e-4 holds for EVERY case, the +-80 one included, unscaled.
#   PCLS_SMALL_ERR_MEASURED  the largest over the cases with logits 4 N(0, 1) (|joint| < 128): 1.17e-5.  Those cases, and predcls()
#                            end to end (measured there: 9.4e-7 at V = 50), are held to PCLS_SMALL_TOL = 1.17e-4 as well.
# joint is bit-equal to triple_logp's mix on all 27 010 compared triples; marg differs from query_logp on (s, ?, o) by at most
# 1.91e-6 (N = 65: the online sum of query_logp against the two walks here; 0 at the other cases), bound QLP_VS_TLP_TOL.
PCLS_ERR_MEASURED = 3.77e-5
PCLS_SMALL_ERR_MEASURED = 1.17e-5
PCLS_TOL = 10 * PCLS_ERR_MEASURED
PCLS_SMALL_TOL = 10 * PCLS_SMALL_ERR_MEASURED

def lse64(x):
    """log-sum-exp over the last axis, fp64, stabilised by the maximum."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def enumerate_triples(pairs, V):
    """pairs [n, 2] -> int64 [n * V, 3]: (s, v, o) for every pair and every predicate token v, pair-major."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    t = np.empty((len(pairs), V, 3), dtype=np.int64)
    t[:, :, 0], t[:, :, 1], t[:, :, 2] = pairs[:, 0:1], np.arange(V)[None, :], pairs[:, 1:2]
    return t.reshape(-1, 3)
