"""CPU: predicate classification (csrc/predcls.hip, sgg_amd/predcls.py, train.SceneGraphGAN.predcls and its command line): the
candidate pairs, known answers of the fp64 reference, the reference against tests/xent_ref.py's triple_logp, the merge's constraint
modes, the summary, parse_args and the C ABI's declarations."""
import os
import sys

import numpy as np
import pytest

import sgg_amd  # noqa: F401
from sgg_amd import lib
from sgg_amd import predcls as P
from tests import predcls_ref as PR
from tests import xent_ref as XR
from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pair_predicate_logp", "predcls_pair_topk", "predcls_merge")


# ---- candidate pairs ---------------------------------------------------------------------------------------------------------------
def test_candidate_pairs_all_and_gt():
    gt = [[5, 1, 2], [2, 9, 5], [7, 3, 7], [5, 4, 2]]
    pairs, trunc = P.candidate_pairs(gt)
    ent = [2, 5, 7]
    want = sorted({(a, b) for a in ent for b in ent if a != b} | {(7, 7)})
    assert pairs.dtype == np.int32 and pairs.tolist() == [list(x) for x in want] and not trunc
    assert (5, 5) not in want and [7, 7] in pairs.tolist(), "a self pair is a candidate only where it is true"
    assert pairs.tolist() == sorted(pairs.tolist()), "ascending by (s, o)"
    g, trunc = P.candidate_pairs(gt, "gt")
    assert g.tolist() == [[2, 5], [5, 2], [7, 7]] and not trunc
    assert P.gt_pair_index(g, gt).tolist() == [1, 0, 2, 1]
    assert P.gt_pair_index(g[:2], gt).tolist() == [1, 0, -1, 1]
    e, trunc = P.candidate_pairs([])
    assert e.shape == (0, 2) and not trunc
    with pytest.raises(ValueError):
        P.candidate_pairs(gt, "every")


def test_candidate_pairs_truncate_at_4096_and_keep_the_true_pairs():
    # 70 entities: 4830 ordered pairs; the true pairs are the LAST ones in ascending order, which a plain cut would lose
    gt = [[69, 0, i] for i in range(69)] + [[i, 0, 69] for i in range(60, 69)] + [[69, 1, 69]]
    pairs, trunc = P.candidate_pairs(gt)
    assert trunc and pairs.shape == (4096, 2) and pairs.tolist() == sorted(pairs.tolist())
    have = set(map(tuple, pairs.tolist()))
    assert len(have) == 4096 and all((t[0], t[2]) in have for t in gt), "true pairs are kept"
    rest = sorted(have - {(t[0], t[2]) for t in gt})
    every = sorted({(a, b) for a in range(70) for b in range(70) if a != b} - {(t[0], t[2]) for t in gt})
    assert rest == every[:len(rest)], "the others: ascending, up to the limit"
    assert (P.gt_pair_index(pairs, gt) >= 0).all()
    few, trunc = P.candidate_pairs(gt, max_pairs=10)
    assert trunc and len(few) == 10 and all(tuple(p) in {(t[0], t[2]) for t in gt} for p in few.tolist())


def test_pair_chunk():
    assert P.pair_chunk(380, 32, 1000, 8 << 30) == (380, 1)
    assert P.pair_chunk(12, 4, 50, 24000) == (6, 2)                 # 6000 bytes / (4 x 50 x 4) = 7 pairs: two even launches
    assert P.pair_chunk(5, 4, 50, 16) == (1, 5)                     # one pair per image is the floor
    Pc, n = P.pair_chunk(4096, 32, 70000, 8 << 30)
    assert Pc * n >= 4096 and 32 * Pc * 70000 * 4 <= (8 << 30) // 4 and (Pc - 1) * n < 4096


# ---- the reference: known answers ---------------------------------------------------------------------------------------------------
def _random(N, nb, V, seed=0, scale=4.0):
    g = np.random.RandomState(seed)
    x = (scale * g.standard_normal((N, nb, 3, V))).astype(np.float32)
    return x, PR.lse64(x)


def test_one_draw_gives_the_predicate_log_softmax():
    x, z = _random(1, 2, 9)
    pairs = np.array([[[0, 1], [8, 8], [3, 2]], [[1, 0], [2, 2], [4, 5]]])
    r = P.pair_predicate_reference(x, z, pairs, [3, 3])
    a1 = x[0, :, 1, :].astype(np.float64) - z[0, :, 1:2]
    assert (r["status"] == 0).all()
    assert np.abs(r["cond"] - a1[:, None, :]).max() <= 1e-13, "N = 1: cond = a_1 whatever the pair"
    a0, a2 = x[0].astype(np.float64)[:, 0] - z[0, :, 0:1], x[0].astype(np.float64)[:, 2] - z[0, :, 2:3]
    for j in range(2):
        for p, (s, o) in enumerate(pairs[j]):
            assert abs(r["marg"][j, p] - (a0[j, s] + a2[j, o])) <= 1e-13


def test_identical_draws_give_one_draw_and_cond_sums_to_one():
    x, z = _random(1, 2, 11, seed=1)
    pairs = np.array([[[0, 1], [2, 3]], [[10, 0], [5, 5]]])
    one = P.pair_predicate_reference(x, z, pairs, [2, 2])
    five = P.pair_predicate_reference(np.repeat(x, 5, axis=0), np.repeat(z, 5, axis=0), pairs, [2, 2])
    for name in ("joint", "marg", "cond"):
        assert np.abs(one[name] - five[name]).max() <= 1e-12, name
    x, z = _random(6, 3, 40, seed=2)
    pairs = np.random.RandomState(3).randint(0, 40, size=(3, 7, 2))
    r = P.pair_predicate_reference(x, z, pairs, [7, 7, 7])
    assert np.abs(np.exp(r["cond"]).sum(axis=2) - 1.0).max() <= 1e-12
    assert np.abs(PR.lse64(r["joint"]) - r["marg"]).max() <= 1e-12, "marg is the joint with the predicate summed out"


def test_hand_worked_two_draws_three_tokens():
    """Pair (0, 1).  Draw 0 believes in it (p(s = 0) = p(o = 1) = 0.9) and says predicate 0 (0.7, 0.2, 0.1); draw 1 does not
    (0.1 each) and says predicate 1 (0.1, 0.8, 0.1).  Posterior weights 0.81 : 0.01, so
    p(v | s, o) = (0.81 p_0(v) + 0.01 p_1(v)) / 0.82 = (0.568, 0.170, 0.082) / 0.82: predicate 0.
    The plain average of the two softmaxes is (0.4, 0.5, 0.1): predicate 1."""
    p = np.array([[[0.9, 0.05, 0.05], [0.7, 0.2, 0.1], [0.05, 0.9, 0.05]],
                  [[0.1, 0.45, 0.45], [0.1, 0.8, 0.1], [0.45, 0.1, 0.45]]])
    x = np.log(p)[:, None]                                           # [2, 1, 3, 3]; lse = 0
    r = P.pair_predicate_reference(x, np.zeros((2, 1, 3)), [[[0, 1]]], [1])
    want = np.array([0.568, 0.170, 0.082]) / 0.82
    assert np.abs(np.exp(r["cond"][0, 0]) - want).max() <= 1e-12
    assert abs(r["marg"][0, 0] - np.log(0.82 / 2)) <= 1e-12
    assert np.abs(r["joint"][0, 0] - np.log(np.array([0.568, 0.170, 0.082]) / 2)).max() <= 1e-12
    assert int(np.argmax(r["cond"][0, 0])) == 0 and int(np.argmax(p[:, 1].mean(axis=0))) == 1
    top = P.pair_topk_reference(r["joint"], r["status"], 3, [[0, 0, -1]], [[1, 2, 0]])
    assert top["top_tok"][0, 0].tolist() == [0, 1, 2] and top["gt_rank"][0].tolist() == [2, 3, 0]


def test_reference_joint_is_triple_logp_on_the_enumerated_triples():
    N, nb, V, Pn = 5, 2, 13, 6
    x, z = _random(N, nb, V, seed=4)
    pairs = np.random.RandomState(5).randint(0, V, size=(nb, Pn, 2))
    pairs[1, 2] = (V, 0)
    pairs[1, 3] = (1, -1)
    r = P.pair_predicate_reference(x, z, pairs, [Pn, 5])
    assert r["status"].tolist() == [[0] * 6, [0, 0, -4, -4, 0, -3]]
    gt = np.stack([PR.enumerate_triples(pairs[j], V) for j in range(nb)])
    t = XR.triple_logp(x, z, gt, [Pn * V, 5 * V])
    ok = r["status"] == 0
    assert np.array_equal(t["status"].reshape(nb, Pn, V)[:, :, 0], r["status"])
    assert np.isnan(r["joint"][~ok]).all() and np.isnan(r["marg"][~ok]).all()
    assert np.abs(t["mix"].reshape(nb, Pn, V)[ok] - r["joint"][ok]).max() <= 1e-12


# ---- the selection references ----------------------------------------------------------------------------------------------------
def test_topk_and_merge_reference_orders_and_constraint():
    g = np.random.RandomState(6)
    nb, Pn, V, Kc = 2, 5, 8, 4
    joint = -np.abs(g.standard_normal((nb, Pn, V))).astype(np.float32) * 3
    joint[0, 1, 6] = joint[0, 1, 2] = joint[0, 1].max() + 1          # a tie inside a pair: the smaller token first
    joint[0, 3] = joint[0, 2]                                         # two equal pairs: the smaller pair index first
    status = np.zeros((nb, Pn), dtype=np.int32)
    status[1, 4] = -3
    joint[1, 4] = np.nan
    marg = (PR.lse64(joint) + 0.0).astype(np.float32)
    pairs = np.stack([np.stack([np.arange(Pn), np.arange(Pn) + 1], axis=1)] * nb).astype(np.int32)
    gp, gv = np.array([[1, 1, 3, -1], [4, 0, 0, 9]]), np.array([[2, 6, 0, 0], [0, V, 3, 1]])
    top = P.pair_topk_reference(joint, status, Kc, gp, gv)
    assert top["top_tok"][0, 1, :2].tolist() == [2, 6] and top["gt_rank"][0].tolist()[:2] == [1, 2] and top["gt_rank"][0, 3] == 0
    assert top["gt_rank"][1].tolist()[:2] == [0, 0] and top["gt_rank"][1, 3] == 0 and top["gt_rank"][1, 2] >= 1
    assert (top["top_tok"][1, 4] == -1).all() and np.isnan(top["top_score"][1, 4]).all()
    assert np.array_equal(top["top_tok"][0, 2], top["top_tok"][0, 3])
    big = P.pair_topk_reference(joint, status, 11, gp, gv)
    assert (big["top_tok"][:, :, V:] == -1).all() and (big["top_tok"][0, :, :V] >= 0).all()
    for cond in (False, True):
        one = P.merge_reference(pairs, top["top_tok"], top["top_score"], marg, 7, 1, cond)
        assert one["n_distinct"].tolist() == [5, 4] and (one["src"][1, 4:] == -1).all() and np.isnan(one["scores"][1, 4:]).all()
        for j in range(nb):
            n = min(7, int(one["n_distinct"][j]))
            so = one["triples"][j, :n][:, [0, 2]].tolist()
            assert len({tuple(x) for x in so}) == n, "per_pair = 1 never repeats a pair"
            assert (np.diff(one["scores"][j, :n]) <= 0).all()
        i2, i3 = one["src"][0].tolist().index(2), one["src"][0].tolist().index(3)
        assert i3 == i2 + 1, "equal scores: pair index ascending"
        many = P.merge_reference(pairs, top["top_tok"], top["top_score"], marg, 64, Kc, cond)
        assert many["n_distinct"].tolist() == [20, 16] and (many["triples"][0, 20:] == -1).all()
        assert len({tuple(t) for t in many["triples"][0, :20].tolist()}) == 20
        k = many["src"][0, :20]
        tied = np.nonzero((k // Kc == 2) | (k // Kc == 3))[0]
        assert (np.diff(many["scores"][0, :20]) <= 0).all() and len(tied) == 8
        for a, b in zip(tied[0::2], tied[1::2]):
            assert b == a + 1 and k[a] // Kc == 2 and k[b] // Kc == 3 and k[a] % Kc == k[b] % Kc, "ties: pair, then rank inside the pair"


def test_predicate_accumulator():
    acc = P.PredicateAccumulator(10)
    assert acc.result()["top1"] is None
    acc.add([1, 3, 0, 6], [[0, 4, 1], [0, 4, 2], [1, 5, 1], [2, 7, 2]])
    acc.add([1], [[3, 7, 3]])
    r = acc.result()
    assert (r["n_triples"], r["n_unranked"]) == (4, 1) and r["top1"] == 0.5 and r["top5"] == 0.75 and r["mean_rank"] == 11 / 4
    assert abs(r["mean_predicate_top1"] - (0.5 + 0.5) / 2) <= 1e-15, "predicate 4: 1 of 2, predicate 7: 1 of 2; predicate 5 never ranked"
    with pytest.raises(ValueError):
        acc.add([1, 2], [[0, 0, 0]])


# ---- command line and C ABI -------------------------------------------------------------------------------------------------------
def test_parser_knows_the_flags():
    sys.path.insert(0, ROOT)
    import train as T
    a = T.parse_args([])
    assert (a.predcls_out, a.predcls_k, a.predcls_pairs, a.predcls_score) == (None, None, None, None)
    a = T.parse_args(["--predcls_out", "p.json"])
    assert a.predcls_k == (20, 50, 100) and a.predcls_pairs is None and a.predcls_score is None
    a = T.parse_args(["--predcls_out", "p.json", "--predcls_k", "5,1024", "--predcls_pairs", "gt", "--predcls_score", "conditional",
                      "--max_test_images", "4", "--predict_samples", "6", "--eval_live"])
    assert (a.predcls_out, a.predcls_k, a.predcls_pairs, a.predcls_score) == ("p.json", (5, 1024), "gt", "conditional")
    assert (a.max_test_images, a.predict_samples, a.eval_live) == (4, 6, True)
    for bad in (["--predcls_k", "5"], ["--predcls_pairs", "gt"], ["--predcls_score", "joint"],
                ["--predcls_out", "p.json", "--predcls_k", "0"], ["--predcls_out", "p.json", "--predcls_k", "1025"],
                ["--predcls_out", "p.json", "--predcls_k", "a"], ["--predcls_out", "p.json", "--predcls_k", ","],
                ["--predcls_out", "p.json", "--predcls_pairs", "none"], ["--predcls_out", "p.json", "--predcls_score", "critic"],
                ["--predcls_out", "p.json", "--metrics_out", "m.json"], ["--predcls_out", "p.json", "--retrieve_out", "r.json"],
                ["--predcls_out", "p.json", "--likelihood_out", "n.json"], ["--predcls_out", "p.json", "--predict_dir", "g"],
                ["--predcls_out", "p.json", "--saliency_dir", "s"], ["--predcls_out", "p.json", "--test_only"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_predcls_rejects_bad_arguments_before_anything_runs():
    with pytest.raises(ValueError, match="pairs"):
        P.check_args("some", "joint")
    with pytest.raises(ValueError, match="score"):
        P.check_args("all", "critic")
    P.check_args("gt", "conditional")


def test_declared_symbols_equal_the_bindings():
    names = set(declared_symbols())
    assert {"sgg_pair_predicate_logp", "sgg_predcls_pair_topk", "sgg_predcls_merge"} <= names and names == set(lib.SIGNATURES)
    for n in NEW:
        assert callable(getattr(lib.HipKernels, n))
    assert len(lib.SIGNATURES["sgg_pair_predicate_logp"][1]) == 14 and len(lib.SIGNATURES["sgg_predcls_pair_topk"][1]) == 14
    assert len(lib.SIGNATURES["sgg_predcls_merge"][1]) == 15
