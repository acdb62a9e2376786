"""Image retrieval by triple query, host side (numpy / Python only; the kernels are csrc/retrieve.hip behind
lib.HipKernels.query_logp, retrieve_topk and retrieve_ranks).

A query is a triple (subject, predicate, object) of which any slot may be left open (a wildcard).  Given a noise draw the generator's
three decoder softmaxes are independent (sgg_amd/kbest.py), so the probability of a partial triple is the product over its
SPECIFIED slots - an open slot's softmax sums to 1 - and the score of an image is the log of that probability under the mixture of
the image's noise draws.  Images rank by (score descending, image index ascending)."""
from collections import Counter

import numpy as np

MAX_QUERIES = 4096          # queries per sgg_query_logp launch (train.SceneGraphGAN.retrieve goes in blocks of this)
MAX_RELEVANT = 4096         # relevant images per query that sgg_retrieve_ranks sorts
MAX_TOP = 1024              # images per query that sgg_retrieve_topk returns
DEFAULT_SCORE_BUDGET_BYTES = 1 << 30
WILDCARDS = (None, "?", -1)


def _is_wildcard(x):
    return x is None or (isinstance(x, str) and x == "?") or (not isinstance(x, str) and not isinstance(x, bool) and int(x) == -1)


def query_ids(query, vocab):
    """One query as three token ids, -1 for a wildcard; None when a word or id is outside the vocabulary.  vocab: word -> id."""
    if len(query) != 3:
        raise ValueError("retrieve: a query is three slots (got %r)" % (query,))
    V, out = len(vocab), []
    for x in query:
        if _is_wildcard(x):
            out.append(-1)
        elif isinstance(x, str):
            if x not in vocab:
                return None
            out.append(int(vocab[x]))
        else:
            if not 0 <= int(x) < V:
                return None
            out.append(int(x))
    return tuple(out)


def compile_queries(queries, vocab):
    """queries: id triples or word triples, None / "?" / -1 for a wildcard; vocab: word -> id (its length is V).  Returns a dict:
    ids int64 [Q, 3] (the accepted queries in the given order, -1 for a wildcard), kept (their positions in `queries`), rejected
    (positions of the queries with a word or id outside the vocabulary: reported, not scored), tok int32 [3, U] and ucount [3]
    (per slot the distinct tokens in ascending order, U = max(1, the longest list)) and qidx int32 [Q, 3] (index into the slot's
    list; -1 for a wildcard) - the operands of HipKernels.query_logp."""
    ids, kept, rejected = [], [], []
    for i, q in enumerate(queries):
        t = query_ids(q, vocab)
        if t is None:
            rejected.append(i)
        else:
            ids.append(t)
            kept.append(i)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 3)
    lists = [np.unique(ids[:, s][ids[:, s] >= 0]) for s in range(3)]
    U = max(1, max(len(l) for l in lists))
    tok = np.zeros((3, U), dtype=np.int32)
    qidx = np.full(ids.shape, -1, dtype=np.int32)
    for s, l in enumerate(lists):
        tok[s, :len(l)] = l
        spec = ids[:, s] >= 0
        qidx[spec, s] = np.searchsorted(l, ids[spec, s]).astype(np.int32)
    return {"ids": ids, "kept": kept, "rejected": rejected, "tok": tok, "ucount": [int(len(l)) for l in lists], "qidx": qidx}


def relevance(queries, gt_per_image):
    """queries: id triples with -1 for a wildcard ([Q, 3]); gt_per_image: per image its true triples.  An image is relevant to a
    query when one of its true triples equals the query on every specified slot.  Returns (rel_ptr int32 [Q + 1], rel_idx int32):
    the CSR lists, image indices ascending.  More than MAX_RELEVANT relevant images for one query raises ValueError."""
    queries = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    index = {}                                         # (pattern of specified slots, their tokens) -> images, for the patterns in use
    patterns = sorted({tuple(bool(x >= 0) for x in q) for q in queries.tolist()})
    for i, real in enumerate(gt_per_image):
        for t in real:
            t = tuple(int(x) for x in t)
            for p in patterns:
                index.setdefault((p, tuple(x for x, on in zip(t, p) if on)), set()).add(i)
    ptr, idx = [0], []
    for q in queries.tolist():
        p = tuple(x >= 0 for x in q)
        hit = sorted(index.get((p, tuple(x for x in q if x >= 0)), ()))
        if len(hit) > MAX_RELEVANT:
            raise ValueError("retrieve: query %r has %d relevant images (at most %d per query; make it more specific or evaluate "
                             "fewer images)" % (tuple(q), len(hit), MAX_RELEVANT))
        idx.extend(hit)
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32)


def summarise(first_rank, ap, status, ks):
    """The retrieval metrics over the valid queries (status 0): {"R@K": share of them whose first relevant image is within the
    first K, for K in ks; "median_rank": median first rank; "mrr": mean of 1 / first rank; "map": mean average precision;
    "n_valid"; "n_without_relevant": queries with no relevant image (status -3), excluded}.  Any other status is a ValueError: a list
    the kernel refused (-4) is not "no relevant image".  Sums in fp64; None over nothing."""
    first_rank = np.asarray(first_rank, dtype=np.int64).reshape(-1)
    ap = np.asarray(ap, dtype=np.float64).reshape(-1)
    status = np.asarray(status).reshape(-1)
    if not np.isin(status, (0, -3)).all():
        raise ValueError("summarise: status is 0 (valid) or -3 (no relevant image), got %r" % sorted(set(status.tolist())))
    ok = status == 0
    n = int(ok.sum())
    fr = first_rank[ok].astype(np.float64)
    res = {"R@%d" % k: (float((fr <= k).sum()) / n if n else None) for k in ks}
    res.update({"median_rank": float(np.median(fr)) if n else None, "mrr": float((1.0 / fr).sum() / n) if n else None,
                "map": float(ap[ok].sum() / n) if n else None, "n_valid": n, "n_without_relevant": int((~ok).sum())})
    return res


def default_queries(gt_per_image, max_queries=MAX_QUERIES):
    """The distinct true triples of the collection as queries: most frequent first (occurrences over all images' lists), ties by
    the triple ascending, cut at max_queries.  List of (s, p, o) tuples."""
    c = Counter(tuple(int(x) for x in t) for real in gt_per_image for t in real)
    return [t for t, _ in sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))][:max(0, int(max_queries))]


def score_matrix_bytes(n_queries, n_images):
    return 4 * int(n_queries) * int(n_images)
