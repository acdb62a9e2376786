"""Host definitions of the scene-graph metrics (SceneGraphGAN.evaluate in train.py): the match of an image's ground-truth triples
against its ranked list of distinct predictions, and R@K / mR@K / zsR@K over a set of images.  Pure Python and numpy: importable
without a GPU.  The match of the product path is the HIP kernel csrc/match.hip behind lib.HipKernels.match_triples;
match_reference below states its semantics and is what the kernel is tested against."""
from __future__ import annotations

import numpy as np

ABSENT, DUPLICATE, PADDING, INVALID = -1, -2, -3, -4     # the codes of pos below a list position (include/sgg_hip.h)
MAX_VOCAB = 1 << 21
MAX_GT = 4096                                             # ground-truth rows per image the kernel sorts in LDS


def match_reference(ranked, gt, vocab=None):
    """ranked: [U, 3] distinct triples in ranked order; gt: list of [s, p, o] -> (pos int32 [len(gt)], n_gt).
    pos[m] = u where gt[m] equals ranked[u]; ABSENT (-1) where it equals none; DUPLICATE (-2) where it equals an earlier row
    gt[m'], m' < m (the first row carries the result); INVALID (-4) where a token lies outside [0, vocab) (default 2^21): such a
    row never matches and is never the earlier row of a duplicate.  n_gt = rows with pos >= -1: the distinct valid triples.
    (PADDING, -3, is the kernel's code of the rows behind an image's count in a padded batch: a list has none.)"""
    V = MAX_VOCAB if vocab is None else int(vocab)
    where = {}
    for u, t in enumerate(np.asarray(ranked, dtype=np.int64).reshape(-1, 3).tolist()):
        where.setdefault(tuple(t), u)
    pos, seen = np.empty((len(gt),), dtype=np.int32), set()
    for m, t in enumerate(gt):
        t = tuple(int(x) for x in t)
        if not all(0 <= x < V for x in t):
            pos[m] = INVALID
        elif t in seen:
            pos[m] = DUPLICATE
        else:
            seen.add(t)
            pos[m] = where.get(t, ABSENT)
    return pos, len(seen)


def zero_shot_mask(gt, train_set):
    """bool [len(gt)]: True where the triple is not in train_set (a set of (s, p, o) tuples of the training images)."""
    return np.array([tuple(int(x) for x in t) not in train_set for t in gt], dtype=bool)


class RecallAccumulator(object):
    """R@K, mR@K and zsR@K over images, from the match of every image (match_reference / HipKernels.match_triples).

    With G_i the distinct valid ground-truth triples of image i (the rows with pos >= -1) and hit_i(g, K) = (0 <= pos_i(g) < K):
      R@K   = mean over the images with |G_i| > 0 of  sum_g hit_i(g, K) / |G_i|;
      mR@K  = mean over the predicates p (token 1 of a triple) that occur in some G_i of r_p(K), where r_p(K) is the mean, over the
              images that have a triple with predicate p, of hits_{i,p}(K) / |G_{i,p}|;
      zsR@K = R@K restricted to Z_i = the triples of G_i that are not in the training set, over the images with Z_i non-empty;
              None when no image was added with a zero-shot mask, or none has such a triple.
    The predictions are DISTINCT triples (K counts distinct triples, not samples) and the denominators are |G_i|, not K.
    Sums are float64, accumulated in the order of the add() calls."""

    def __init__(self, ks, vocab_size):
        self.ks = tuple(int(k) for k in ks)
        if not self.ks or min(self.ks) < 1:
            raise ValueError("RecallAccumulator: ks must be positive integers (got %r)" % (ks,))
        self.vocab_size = int(vocab_size)
        nk = len(self.ks)
        self.images = self.skipped_images = self.invalid_triples = self.zs_images = 0
        self.zs_known = False
        self.r_sum, self.zs_sum = np.zeros(nk, dtype=np.float64), np.zeros(nk, dtype=np.float64)
        self.pred_sum = np.zeros((self.vocab_size, nk), dtype=np.float64)
        self.pred_images = np.zeros(self.vocab_size, dtype=np.int64)
        self.pred_triples = np.zeros(self.vocab_size, dtype=np.int64)

    def add(self, pos, gt, zero_shot=None):
        """One image: pos [len(gt)] (the codes of match_reference; padding rows of a batch already cut off), its ground-truth
        triples, and optionally zero_shot bool [len(gt)] (zero_shot_mask)."""
        pos = np.asarray(pos, dtype=np.int64).reshape(-1)
        gt = np.asarray(gt, dtype=np.int64).reshape(-1, 3)
        if len(pos) != len(gt):
            raise ValueError("RecallAccumulator.add: %d positions for %d ground-truth triples" % (len(pos), len(gt)))
        self.invalid_triples += int((pos == INVALID).sum())
        if zero_shot is not None:
            self.zs_known = True
        valid = pos >= ABSENT
        n = int(valid.sum())
        if n == 0:
            self.skipped_images += 1
            return
        preds = gt[:, 1]
        if int(preds[valid].max()) >= self.vocab_size or int(preds[valid].min()) < 0:
            raise ValueError("RecallAccumulator.add: a valid row has a predicate outside [0, %d) (match with vocab = vocab_size)"
                             % self.vocab_size)
        self.images += 1
        ks = np.asarray(self.ks, dtype=np.int64)
        hit = valid[:, None] & (pos[:, None] >= 0) & (pos[:, None] < ks[None, :])         # [len(gt), len(ks)]
        self.r_sum += hit.sum(axis=0) / float(n)
        for p in np.unique(preds[valid]).tolist():
            rows = valid & (preds == p)
            n_p = int(rows.sum())
            self.pred_sum[p] += hit[rows].sum(axis=0) / float(n_p)
            self.pred_images[p] += 1
            self.pred_triples[p] += n_p
        if zero_shot is not None:
            z = valid & np.asarray(zero_shot, dtype=bool).reshape(-1)
            n_z = int(z.sum())
            if n_z:
                self.zs_images += 1
                self.zs_sum += hit[z].sum(axis=0) / float(n_z)

    def result(self, reverse_vocab=None):
        """{"R@K", "mR@K", "zsR@K" for every K, "predicates": {word (or index): {"index", "images", "triples", "recall": {"K": r_p(K)}}},
        "images", "skipped_images" (|G_i| = 0), "zero_shot_images", "invalid_triples"}; a mean over nothing is None."""
        occurs = np.nonzero(self.pred_images)[0]
        r_p = self.pred_sum[occurs] / self.pred_images[occurs, None].astype(np.float64)
        res = {"images": self.images, "skipped_images": self.skipped_images, "zero_shot_images": self.zs_images,
               "invalid_triples": self.invalid_triples}
        for i, k in enumerate(self.ks):
            res["R@%d" % k] = float(self.r_sum[i] / self.images) if self.images else None
            res["mR@%d" % k] = float(r_p[:, i].mean()) if len(occurs) else None
            res["zsR@%d" % k] = float(self.zs_sum[i] / self.zs_images) if (self.zs_known and self.zs_images) else None
        word = (lambda p: str(p)) if reverse_vocab is None else (lambda p: reverse_vocab.get(p, "UNK:%d" % p))
        res["predicates"] = {word(int(p)): {"index": int(p), "images": int(self.pred_images[p]), "triples": int(self.pred_triples[p]),
                                            "recall": {str(k): float(r_p[n, i]) for i, k in enumerate(self.ks)}}
                             for n, p in enumerate(occurs)}
        return res
