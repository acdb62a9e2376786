"""Host side of predicate classification (SceneGraphGAN.predcls in train.py): the candidate pairs of an image, the definitions of
the three kernels of csrc/predcls.hip restated in numpy fp64, and the summary.  Pure Python and numpy: importable without a GPU.

The protocol (PredCls): the entities of an image are given; the model says which ordered pairs are related and by which predicate.
Given a noise draw the generator's three softmaxes are independent (sgg_amd/kbest.py), so under the mixture of an image's N draws

    a_t^k(x) = logits[k][t][x] - lse[k][t]
    lp_k(v)  = (a_0^k(s) + a_1^k(v)) + a_2^k(o)
    joint(v) = m + (log(sum_k exp(lp_k - m)) - log N),  m = max_k lp_k      log p(s, v, o | image): triple_logp's mix, bit for bit
    marg     = the same with a_1 = 0                                         log p(s, o | image), the predicate marginalised
    cond(v)  = joint(v) - marg                                               log p(v | s, o, image)

cond is a posterior-weighted mixture of the N predicate softmaxes: a draw that believes in the pair (a large a_0 + a_2) gets more
say.  exp(cond) sums to 1 over v up to rounding.

Order of the predicates of a pair: (joint descending, token ascending).  Order across the pairs of an image: (score descending, pair
index ascending, the predicate's rank inside its pair ascending) with score = joint (the exact ranking of the mixture restricted to
the candidates; it also down-weights unrelated pairs, for which this model has no background class) or score = cond (the
literature's PredCls score)."""
from __future__ import annotations

import numpy as np

MAX_PAIRS = 4096            # candidate pairs per image (sgg_pair_predicate_logp's P)
MAX_KC = 128                # predicates kept per pair (sgg_predcls_pair_topk's Kc)
MAX_K = 1024                # list slots per image (sgg_predcls_merge's K)
PAIR_MODES = ("all", "gt")
SCORES = ("joint", "conditional")
PADDING, INVALID = -3, -4   # status of a pair that is not valid (include/sgg_hip.h)
DEFINITION = ("predicate classification: the entities of an image are its distinct subject / object words; candidates are ordered "
              "entity pairs (pairs=all: every ordered pair of two different entities plus the true self pairs; pairs=gt: the true pairs); "
              "a candidate (s, v, o) scores log p(s, v, o | image) under the mixture of the image's noise draws (score=joint) or "
              "log p(v | s, o, image) = joint - log p(s, o | image) (score=conditional); graph_constraint lists the best predicate of "
              "every pair, no_graph_constraint up to predicates_per_pair of them; R@K, mR@K, zsR@K over distinct predictions with "
              "denominators |GT|; predicate_given_pair ranks all predicates of a true triple's own pair")


def check_args(pairs, score):
    if pairs not in PAIR_MODES:
        raise ValueError("predcls: pairs must be one of %s (got %r)" % (", ".join(PAIR_MODES), pairs))
    if score not in SCORES:
        raise ValueError("predcls: score must be one of %s (got %r)" % (", ".join(SCORES), score))


def candidate_pairs(gt, mode="all", max_pairs=MAX_PAIRS):
    """The candidate (subject, object) pairs of one image from its true triples gt = [[s, p, o], ...] -> (pairs int32 [n, 2]
    ascending by (s, o), truncated).  Entities: the distinct words in subject or object position.  mode "all": every ordered pair
    of two different entities plus every true (s, o) with s == o; "gt": the true (s, o) pairs only (predicate detection in the sense
    of Lu et al.).  More than max_pairs: the true pairs are kept, then the others in ascending order up to max_pairs (the kept set
    is again ascending), and truncated is True."""
    if mode not in PAIR_MODES:
        raise ValueError("candidate_pairs: mode must be one of %s (got %r)" % (", ".join(PAIR_MODES), mode))
    true = sorted({(int(t[0]), int(t[2])) for t in gt})
    if mode == "gt":
        cand = true
    else:
        ent = sorted({x for so in true for x in so})
        cand = sorted(set(true) | {(a, b) for a in ent for b in ent if a != b})
    truncated = len(cand) > max_pairs
    if truncated:
        keep = set(true[:max_pairs])
        for so in cand:
            if len(keep) >= max_pairs:
                break
            keep.add(so)
        cand = sorted(keep)
    return np.asarray(cand, dtype=np.int32).reshape(-1, 2), truncated


def gt_pair_index(pairs, gt):
    """int32 [len(gt)]: the index of every true triple's (s, o) among pairs [n, 2], or -1."""
    where = {(int(s), int(o)): i for i, (s, o) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist())}
    return np.asarray([where.get((int(t[0]), int(t[2])), -1) for t in gt], dtype=np.int32).reshape(-1)


def pair_chunk(P, nb, V, logits_budget_bytes):
    """(pairs per launch Pc, launches): the joint buffer [nb, Pc, V] fp32 stays within a quarter of the logits budget (one pair per
    image is the floor), the launches are as even as they can be."""
    cap = max(1, (int(logits_budget_bytes) // 4) // (int(nb) * int(V) * 4))
    n = -(-int(P) // min(cap, int(P)))
    return -(-int(P) // n), n


# ---- the kernels' definitions in fp64 ------------------------------------------------------------------------------------------
def _mix(lp):
    """lp [N, ...] -> log of the mean over axis 0 of exp(lp), stabilised by the maximum."""
    m = lp.max(axis=0)
    return m + (np.log(np.exp(lp - m).sum(axis=0)) - np.log(lp.shape[0]))


def pair_predicate_reference(logits, lse, pairs, pair_count):
    """logits [N, nb, 3, V], lse [N, nb, 3] (as given: the device's own in the GPU tests), pairs int [nb, P, 2], pair_count [nb] ->
    dict of fp64 joint [nb, P, V], marg [nb, P], cond [nb, P, V] (NaN where the pair is not valid) and status int32 [nb, P]."""
    x, z = np.asarray(logits, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64)
    N, nb, _, V = x.shape
    P = pairs.shape[1]
    cnt = np.clip(np.asarray(pair_count, dtype=np.int64), 0, P)
    joint, marg = np.full((nb, P, V), np.nan), np.full((nb, P), np.nan)
    status = np.zeros((nb, P), dtype=np.int32)
    for j in range(nb):
        a1 = x[:, j, 1, :] - z[:, j, 1:2]                                   # [N, V]
        for p in range(P):
            s, o = pairs[j, p]
            if p >= cnt[j]:
                status[j, p] = PADDING
            elif not (0 <= s < V and 0 <= o < V):
                status[j, p] = INVALID
            else:
                a0, a2 = x[:, j, 0, s] - z[:, j, 0], x[:, j, 2, o] - z[:, j, 2]
                joint[j, p] = _mix((a0[:, None] + a1) + a2[:, None])
                marg[j, p] = _mix(a0 + a2)
    return {"joint": joint, "marg": marg, "cond": joint - marg[:, :, None], "status": status}


def token_order(row):
    """The tokens of a joint row in rank order: (joint descending, token ascending; +0 == -0)."""
    row = np.asarray(row)
    return np.lexsort((np.arange(row.shape[0]), -row))


def pair_topk_reference(joint, status, Kc, gt_pair, gt_pred):
    """joint [nb, P, V] (any float dtype: the kernel's own bits in the GPU tests), status [nb, P], gt_pair / gt_pred int [nb, M] ->
    dict of top_tok int32 [nb, P, Kc], top_score [nb, P, Kc] in joint's dtype (-1 / NaN behind min(Kc, V) and where status != 0)
    and gt_rank int32 [nb, M] (1-based; 0 without a valid pair or token)."""
    joint, status = np.asarray(joint), np.asarray(status)
    gt_pair, gt_pred = np.asarray(gt_pair, dtype=np.int64), np.asarray(gt_pred, dtype=np.int64)
    nb, P, V = joint.shape
    top_tok = np.full((nb, P, Kc), -1, dtype=np.int32)
    top_score = np.full((nb, P, Kc), np.nan, dtype=joint.dtype)
    gt_rank = np.zeros(gt_pair.shape, dtype=np.int32)
    n = min(Kc, V)
    for j in range(nb):
        orders = {}
        for p in range(P):
            if status[j, p] != 0:
                continue
            orders[p] = token_order(joint[j, p])
            top_tok[j, p, :n] = orders[p][:n]
            top_score[j, p, :n] = joint[j, p, orders[p][:n]]
        for m in range(gt_pair.shape[1]):
            p, t = int(gt_pair[j, m]), int(gt_pred[j, m])
            if p in orders and 0 <= t < V:
                gt_rank[j, m] = 1 + int(np.nonzero(orders[p] == t)[0][0])
    return {"top_tok": top_tok, "top_score": top_score, "gt_rank": gt_rank}


def merge_reference(pairs, top_tok, top_score, marg, K, per_pair=1, conditional=False):
    """pairs [nb, P, 2], top_tok / top_score [nb, P, Kc], marg [nb, P] -> dict of triples int64 [nb, K, 3], scores [nb, K] (in
    top_score's dtype: fp32 inputs give the kernel's fp32 subtraction), src int32 [nb, K], n_distinct int32 [nb]; -1 / NaN / -1
    behind the candidates."""
    pairs, top_tok, top_score, marg = np.asarray(pairs), np.asarray(top_tok), np.asarray(top_score), np.asarray(marg)
    nb, P, Kc = top_tok.shape
    triples = np.full((nb, K, 3), -1, dtype=np.int64)
    scores = np.full((nb, K), np.nan, dtype=top_score.dtype)
    src = np.full((nb, K), -1, dtype=np.int32)
    n_distinct = np.zeros((nb,), dtype=np.int32)
    for j in range(nb):
        tok = top_tok[j, :, :per_pair].reshape(-1)
        sc = top_score[j, :, :per_pair]
        sc = (sc - marg[j][:, None] if conditional else sc).reshape(-1)
        cand = np.nonzero(tok >= 0)[0]
        order = cand[np.lexsort((cand, -sc[cand]))][:K]
        n = len(order)
        n_distinct[j] = len(cand)
        i = order // per_pair
        triples[j, :n] = np.stack([pairs[j, i, 0], tok[order], pairs[j, i, 1]], axis=1)
        scores[j, :n] = sc[order]
        src[j, :n] = order
    return {"triples": triples, "scores": scores, "src": src, "n_distinct": n_distinct}


# ---- the summary ---------------------------------------------------------------------------------------------------------------
class PredicateAccumulator(object):
    """Predicate accuracy GIVEN the true pair, from gt_rank (the 1-based rank of a true triple's predicate among all V predicates of
    its own pair; 0: not ranked - no candidate pair, or a token outside the vocabulary).  Duplicated true triples count once each
    time they are listed by the caller; the caller hands in the rows it wants counted."""

    def __init__(self, vocab_size):
        self.n = self.top1 = self.top5 = 0
        self.rank_sum = 0.0
        self.unranked = 0
        self.pred_n = np.zeros(int(vocab_size), dtype=np.int64)
        self.pred_top1 = np.zeros(int(vocab_size), dtype=np.int64)

    def add(self, gt_rank, gt):
        gt_rank = np.asarray(gt_rank, dtype=np.int64).reshape(-1)
        gt = np.asarray(gt, dtype=np.int64).reshape(-1, 3)
        if len(gt_rank) != len(gt):
            raise ValueError("PredicateAccumulator.add: %d ranks for %d ground-truth triples" % (len(gt_rank), len(gt)))
        ok = gt_rank >= 1
        self.unranked += int((~ok).sum())
        self.n += int(ok.sum())
        self.top1 += int((gt_rank[ok] == 1).sum())
        self.top5 += int((gt_rank[ok] <= 5).sum())
        self.rank_sum += float(gt_rank[ok].sum())
        np.add.at(self.pred_n, gt[ok, 1], 1)
        np.add.at(self.pred_top1, gt[ok, 1][gt_rank[ok] == 1], 1)

    def result(self):
        """{"top1", "top5", "mean_rank", "mean_predicate_top1" (the mean over the predicates that occur of their top-1 accuracy),
        "n_triples", "n_unranked"}; a mean over nothing is None."""
        occurs = self.pred_n > 0
        return {"top1": self.top1 / self.n if self.n else None, "top5": self.top5 / self.n if self.n else None,
                "mean_rank": self.rank_sum / self.n if self.n else None,
                "mean_predicate_top1": float((self.pred_top1[occurs] / self.pred_n[occurs]).mean()) if occurs.any() else None,
                "n_triples": self.n, "n_unranked": self.unranked}
