"""CPU: the host definitions of the scene-graph metrics (sgg_amd/metrics.py) - the reference match of ground-truth triples against
a ranked distinct list, the zero-shot mask, and R@K / mR@K / zsR@K on a case written out by hand."""
from fractions import Fraction as F

import numpy as np
import pytest

import sgg_amd  # noqa: F401
from sgg_amd.metrics import ABSENT, DUPLICATE, INVALID, PADDING, RecallAccumulator, match_reference, zero_shot_mask


def test_match_reference_on_a_hand_written_case():
    pos, n_gt = match_reference([[4, 5, 6], [1, 2, 3], [7, 8, 9]], [[1, 2, 3], [9, 9, 9], [1, 2, 3], [7, 8, 9]])
    assert pos.dtype == np.int32 and pos.tolist() == [1, -1, -2, 2] and n_gt == 3
    assert (ABSENT, DUPLICATE, PADDING, INVALID) == (-1, -2, -3, -4)


def test_match_reference_invalid_tokens_and_empty_inputs():
    ranked = np.array([[4, 5, 6], [1, 2, 3]], dtype=np.int64)
    # a token outside [0, vocab) never matches, never merges with an equal row and is not counted
    pos, n_gt = match_reference(ranked, [[1, 2, 10], [1, 2, 10], [-5, 2, 3], [1, 2, 3], [9, 9, 9], [9, 9, 9]], vocab=10)
    assert pos.tolist() == [-4, -4, -4, 1, -1, -2] and n_gt == 2
    # the default limit is the kernel's, 2^21
    pos, n_gt = match_reference(ranked, [[1, 2, (1 << 21) - 1], [1, 2, 1 << 21]])
    assert pos.tolist() == [-1, -4] and n_gt == 1
    pos, n_gt = match_reference(np.zeros((0, 3), dtype=np.int64), [[1, 2, 3]])
    assert pos.tolist() == [-1] and n_gt == 1
    pos, n_gt = match_reference(ranked, [])
    assert pos.shape == (0,) and n_gt == 0


def test_zero_shot_mask():
    train = {(1, 2, 3), (4, 5, 6)}
    m = zero_shot_mask([[1, 2, 3], [3, 2, 1], (4, 5, 6), np.array([4, 5, 7])], train)
    assert m.dtype == bool and m.tolist() == [False, True, False, True]
    assert zero_shot_mask([], train).shape == (0,)
    assert zero_shot_mask([[1, 2, 3]], set()).tolist() == [True]


# Two images with ground truth, one without, one whose only row is invalid.  V = 20, ks = (1, 2, 5): 5 is longer than both lists.
#   image A: list [a1, a5, a2]; rows a1 (pos 0), a2 (2), a3 (absent), a1 again (duplicate), a5 (1): |G_A| = 4; nothing zero-shot
#   image B: list [b2, b1];     rows b1 (1), b2 (0), b3 (absent), one row with token 50 (invalid): |G_B| = 3; b1 and b3 zero-shot
# Predicates: 10 (A: a1, a2; B: b1), 11 (A: a3; B: b2, b3), 12 (A only: a5).
LIST_A, GT_A = [[1, 10, 2], [6, 12, 7], [1, 10, 3]], [[1, 10, 2], [1, 10, 3], [4, 11, 5], [1, 10, 2], [6, 12, 7]]
LIST_B, GT_B = [[8, 11, 9], [8, 10, 9]], [[8, 10, 9], [8, 11, 9], [3, 11, 3], [50, 11, 3]]
TRAIN = {(1, 10, 2), (1, 10, 3), (4, 11, 5), (6, 12, 7), (8, 11, 9)}
WANT = {"R@1": (F(1, 4) + F(1, 3)) / 2, "R@2": (F(2, 4) + F(2, 3)) / 2, "R@5": (F(3, 4) + F(2, 3)) / 2,
        # r_10 = mean(A: hits of {a1, a2} / 2, B: hit of b1), r_11 = mean(A: 0, B: hits of {b2, b3} / 2), r_12 = A's a5 alone
        "mR@1": ((F(1, 2) + 0) / 2 + (0 + F(1, 2)) / 2 + 0) / 3,
        "mR@2": ((F(1, 2) + 1) / 2 + (0 + F(1, 2)) / 2 + 1) / 3,
        "mR@5": ((F(2, 2) + 1) / 2 + (0 + F(1, 2)) / 2 + 1) / 3,
        # only image B has zero-shot triples: b1 (pos 1) and b3 (absent)
        "zsR@1": F(0), "zsR@2": F(1, 2), "zsR@5": F(1, 2)}
WANT_PRED = {"w10": (2, 3, [F(1, 4), F(3, 4), F(1)]), "w11": (2, 3, [F(1, 4), F(1, 4), F(1, 4)]), "w12": (1, 1, [F(0), F(1), F(1)])}


def _accumulate(with_train):
    acc = RecallAccumulator((1, 2, 5), 20)
    for ranked, gt in ((LIST_A, GT_A), (LIST_B, GT_B), (LIST_A, []), (LIST_B, [[99, 0, 0]])):
        pos, n_gt = match_reference(ranked, gt, vocab=20)
        assert n_gt == int((pos >= -1).sum())
        acc.add(pos, gt, zero_shot_mask(gt, TRAIN) if with_train else None)
    return acc


def test_recall_accumulator_on_a_hand_written_case():
    pos_a, n_a = match_reference(LIST_A, GT_A, vocab=20)
    pos_b, n_b = match_reference(LIST_B, GT_B, vocab=20)
    assert pos_a.tolist() == [0, 2, -1, -2, 1] and n_a == 4 and pos_b.tolist() == [1, 0, -1, -4] and n_b == 3
    assert zero_shot_mask(GT_A, TRAIN).tolist() == [False] * 5              # an image without zero-shot triples
    assert zero_shot_mask(GT_B, TRAIN).tolist() == [True, False, True, True]
    res = _accumulate(True).result({i: "w%d" % i for i in range(20)})
    assert (res["images"], res["skipped_images"], res["invalid_triples"], res["zero_shot_images"]) == (2, 2, 2, 1)
    for name, want in WANT.items():
        assert abs(res[name] - float(want)) <= 1e-15, (name, res[name], want)
    assert sorted(res["predicates"]) == ["w10", "w11", "w12"]
    for word, (images, triples, recall) in WANT_PRED.items():
        p = res["predicates"][word]
        assert (p["index"], p["images"], p["triples"]) == (int(word[1:]), images, triples)
        assert sorted(p["recall"]) == ["1", "2", "5"]
        for k, want in zip(("1", "2", "5"), recall):
            assert abs(p["recall"][k] - float(want)) <= 1e-15, (word, k)
    # without a reverse vocabulary the predicates are named by their index
    assert sorted(_accumulate(True).result()["predicates"]) == ["10", "11", "12"]


def test_recall_accumulator_without_training_set_or_images():
    res = _accumulate(False).result()
    assert [res["zsR@%d" % k] for k in (1, 2, 5)] == [None] * 3 and res["zero_shot_images"] == 0
    assert abs(res["R@2"] - float(WANT["R@2"])) <= 1e-15 and abs(res["mR@5"] - float(WANT["mR@5"])) <= 1e-15
    # a training set that holds every ground-truth triple: known, but no image has a zero-shot triple
    acc = RecallAccumulator((1,), 20)
    acc.add([0, 2, -1, -2, 1], GT_A, [False] * 5)
    assert acc.result()["zsR@1"] is None and acc.result()["R@1"] == 0.25
    empty = RecallAccumulator((3, 7), 20).result()
    assert empty["images"] == 0 and empty["R@3"] is None and empty["mR@7"] is None and empty["predicates"] == {}
    with pytest.raises(ValueError):
        RecallAccumulator((0,), 20)
    with pytest.raises(ValueError):
        RecallAccumulator((1,), 20).add([0, 1], GT_A)
    with pytest.raises(ValueError):         # a valid row whose predicate the accumulator has no slot for
        RecallAccumulator((1,), 5).add([0], [[1, 10, 2]])
