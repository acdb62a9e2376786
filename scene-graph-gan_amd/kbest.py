"""Host logic of K-best decoding (SceneGraphGAN.predict / evaluate with decode="kbest"): the width of the per-sample lists, the
number of rank tuples the kernel sorts, and the argument checks.  Pure Python: importable without a GPU.  The decoding itself is
the pair of HIP kernels of csrc/kbest.hip behind lib.HipKernels.kbest_triples and kbest_merge."""
from __future__ import annotations

MAX_K = 128             # per-row list length of sgg_kbest_triples (5136 rank tuples at K = 256 would not fit one 4096-entry sort)
MAX_POOL = 4096         # list entries per image that sgg_kbest_merge sorts
DECODES = ("samples", "kbest")
ORDERING = "descending generator log-probability (K-best of n samples)"


def list_width(n_samples, vocab):
    """Triples kept per sample: as many as the kernels take (128 per row, 4096 per image over all samples, V^3 in all)."""
    return min(MAX_K, MAX_POOL // int(n_samples), int(vocab) ** 3)


def candidate_count(K, M=None):
    """Rank tuples (i, j, l), each rank below M (default K), with (i+1)(j+1)(l+1) <= K: the only ones that can be among the K most
    probable triples of a product distribution, since a triple is preceded by every triple at componentwise smaller-or-equal ranks.
    152 / 564 / 1471 / 2045 at K = 20 / 50 / 100 / 128."""
    K = int(K)
    M = K if M is None else int(M)
    n = 0
    for i in range(1, min(M, K) + 1):
        for j in range(1, min(M, K // i) + 1):
            n += min(M, K // (i * j))
    return n


def check_decode(decode, descending=False):
    """decode is "samples" or "kbest"; the critic-score direction means nothing to K-best decoding (no critic runs)."""
    if decode not in DECODES:
        raise ValueError("decode must be one of %s (got %r)" % (", ".join(DECODES), decode))
    if decode == "kbest" and descending:
        raise ValueError("decode=\"kbest\" ranks by the generator's log-probability: descending / --predict_descending orders critic "
                         "scores and cannot be combined with it")
    return decode


def setup(who, n_samples, top_k, vocab, test_batch_size):
    """(samples per image, list width, list slots) of a K-best run.  Default n_samples: TEST_BATCH_SIZE (32 at batch 64: width 128);
    default top_k: every slot, n_samples * width."""
    N = int(n_samples) if n_samples is not None else max(1, int(test_batch_size))
    if not 1 <= N <= MAX_POOL:
        raise ValueError("%s: 1 <= n_samples <= %d with decode=\"kbest\" (got %d)" % (who, MAX_POOL, N))
    width = list_width(N, vocab)
    top_k = int(top_k) if top_k is not None else N * width
    if not 1 <= top_k <= N * width:
        raise ValueError("%s: 1 <= top_k <= n_samples * list width = %d x %d with decode=\"kbest\" (got top_k = %d)"
                         % (who, N, width, top_k))
    return N, width, top_k
