"""CPU: image retrieval by triple query (csrc/retrieve.hip, sgg_amd/retrieve.py, train.SceneGraphGAN.retrieve and its command line):
known answers of the numpy fp64 restatement (tests/retrieve_ref.py), the host module on hand-made cases, the C ABI's declarations,
parse_args, and retrieve() on the reference kernel set - tests/test_xent_cpu.py's XentRefKernels carrying the three new entry points
through the restatement."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from sgg_amd import lib
from sgg_amd import retrieve as R
from tests import retrieve_ref as RR
from tests import xent_ref as XR
from tests.test_capi_symbols import declared_symbols
from sgg_amd.metrics import match_reference
from tests.test_relax_cpu import RelaxRefKernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("query_logp", "retrieve_topk", "retrieve_ranks")


class RetrieveRefKernels(RelaxRefKernels):
    """XentRefKernels (as tests/test_relax_cpu.py extends it with rank_triples, so that predict() runs) with the three entry points
    of csrc/retrieve.hip through the restatement; every call is recorded, and query_logp keeps what it was given."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.given = []

    def query_logp(self, logits, lse, tok, ucount, qidx, scores, col0=0):
        self.calls.append("query_logp")
        N, nb = logits.shape[0], logits.shape[1]
        tok, qi = tok.numpy(), qidx.numpy()
        assert all(0 <= u <= tok.shape[1] for u in ucount) and all((qi[:, s] < ucount[s]).all() for s in range(3))
        ids = np.where(qi >= 0, np.stack([tok[s][np.maximum(qi[:, s], 0)] for s in range(3)], axis=1), -1)
        self.given.append((logits.numpy().copy(), lse.reshape(N, nb, 3).numpy().copy(), ids, int(col0)))
        scores[:, col0:col0 + nb] = torch.from_numpy(RR.query_logp(logits.numpy(), lse.reshape(N, nb, 3).numpy(), ids)).to(scores.dtype)
        return scores

    def match_triples(self, ranked, n_distinct, gt, gt_count, vocab=None, out=None):
        """csrc/match.hip through sgg_amd.metrics.match_reference, so that evaluate() runs on this kernel set."""
        for j in range(ranked.shape[0]):
            pos, n_gt = match_reference(ranked[j, :min(int(n_distinct[j]), ranked.shape[1])].numpy(), gt[j, :int(gt_count[j])].tolist(), vocab)
            out["pos"][j] = -3
            out["pos"][j, :len(pos)] = torch.from_numpy(pos)
            out["n_gt"][j] = n_gt
        return out

    def retrieve_topk(self, scores, n_images, K, out=None):
        self.calls.append("retrieve_topk")
        idx, top = RR.topk(scores.numpy(), n_images, K)
        out["idx"].copy_(torch.from_numpy(idx))
        out["scores"].copy_(torch.from_numpy(top))
        return out

    def retrieve_ranks(self, scores, n_images, rel_ptr, rel_idx, out=None):
        self.calls.append("retrieve_ranks")
        r = RR.ranks(scores.numpy(), n_images, rel_ptr.numpy(), rel_idx.numpy())
        out["ranks"][:len(r["ranks"])] = torch.from_numpy(r["ranks"])
        for k in ("first_rank", "ap", "status"):
            out[k].copy_(torch.from_numpy(r[k]))
        return out


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_query_logp_known_answers():
    x = np.zeros((1, 1, 3, 2))                      # uniform logits, V = 2, N = 1
    s = RR.query_logp(x, XR.lse64(x), [[0, 1, 0], [-1, 1, -1], [-1, -1, -1]])
    assert abs(s[0, 0] + 3.0 * np.log(2.0)) < 1e-15 and abs(s[1, 0] + np.log(2.0)) < 1e-15 and s[2, 0] == 0.0
    # three wildcards score 0 for any N, and a wildcard marginalises: p(s, p, ?) = sum_o p(s, p, o)
    g = np.random.RandomState(0)
    x = 3.0 * g.randn(4, 2, 3, 5)
    z = XR.lse64(x)
    s = RR.query_logp(x, z, [[-1, -1, -1], [1, 2, -1]] + [[1, 2, o] for o in range(5)])
    assert np.abs(s[0]).max() < 1e-15 and np.abs(np.exp(s[1]) - np.exp(s[2:]).sum(axis=0)).max() < 1e-15
    # the full triple is triple_logp's mix
    t = XR.triple_logp(x, z, np.array([[[1, 2, 3]], [[1, 2, 3]]]), [1, 1])
    assert np.abs(s[2 + 3] - t["mix"][:, 0]).max() < 1e-15
    # a row of +-80 stays finite
    big = np.tile(np.array([80.0, -80.0, 80.0, -80.0]), (2, 1, 3, 1))
    sb = RR.query_logp(big, XR.lse64(big), [[1, 1, 1], [0, -1, 1]])
    assert np.isfinite(sb).all() and abs(sb[0, 0] + 3.0 * (160.0 + np.log(2.0))) < 1e-11 and abs(sb[1, 0] + 160.0 + 2.0 * np.log(2.0)) < 1e-11


def test_topk_and_ranks_known_answers():
    sc = np.array([[0.5, 2.0, 2.0, -1.0, 0.0, -0.0, 9.0]], dtype=np.float32)        # (column 6 is padding: n_images = 6)
    idx, top = RR.topk(sc, 6, 8)
    assert idx.tolist() == [[1, 2, 0, 4, 5, 3, -1, -1]], "equal scores rank by index, +0 and -0 are equal"
    assert top[0, :6].tolist() == [2.0, 2.0, 0.5, 0.0, 0.0, -1.0] and np.isnan(top[0, 6:]).all()
    assert np.signbit(top[0, 4]) and not np.signbit(top[0, 3]), "the scores are the inputs' own"
    r = RR.ranks(np.array([[5.0, 1.0, 3.0, 0.0]]), 4, [0, 2], [0, 2])
    assert r["ranks"].tolist() == [1, 2] and r["first_rank"].tolist() == [1] and r["ap"][0] == 1.0 and r["status"].tolist() == [0]
    r = RR.ranks(np.array([[5.0, 1.0, 3.0, 0.0], [1.0, 1.0, 1.0, 1.0], [1.0, 2.0, 3.0, 4.0]]), 4, [0, 2, 2, 4], [0, 1, 1, 2])
    assert r["ranks"].tolist() == [1, 3, 3, 2] and r["first_rank"].tolist() == [1, 0, 2]
    assert abs(r["ap"][0] - (1.0 + 2.0 / 3.0) / 2.0) < 1e-15 and np.isnan(r["ap"][1]) and abs(r["ap"][2] - (0.5 + 2.0 / 3.0) / 2.0) < 1e-15
    assert r["status"].tolist() == [0, -3, 0]
    tie = RR.ranks(np.array([[1.0, 1.0, 1.0]]), 3, [0, 1], [1])
    assert tie["ranks"].tolist() == [2], "an irrelevant image with the same score and a smaller index is ahead"


# ---- the host module --------------------------------------------------------------------------------------------------------------
VOCAB = {"w%d" % i: i for i in range(6)}


def test_compile_queries():
    c = R.compile_queries([("w1", "w2", "w3"), ("?", "w2", None), (4, -1, 3), ("w1", "nope", "w3"), (1, 2, 6), [5, 2, 3]], VOCAB)
    assert c["ids"].tolist() == [[1, 2, 3], [-1, 2, -1], [4, -1, 3], [5, 2, 3]] and c["kept"] == [0, 1, 2, 5] and c["rejected"] == [3, 4]
    assert c["ucount"] == [3, 1, 1] and c["tok"].shape == (3, 3) and c["tok"].dtype == np.int32 and c["qidx"].dtype == np.int32
    assert c["tok"][0].tolist() == [1, 4, 5] and c["tok"][1, 0] == 2 and c["tok"][2, 0] == 3
    assert c["qidx"].tolist() == [[0, 0, 0], [-1, 0, -1], [1, -1, 0], [2, 0, 0]]
    # the lists give the tokens back
    back = np.where(c["qidx"] >= 0, np.stack([c["tok"][s][np.maximum(c["qidx"][:, s], 0)] for s in range(3)], axis=1), -1)
    assert np.array_equal(back, c["ids"])
    e = R.compile_queries([(None, None, None)], VOCAB)
    assert e["ucount"] == [0, 0, 0] and e["tok"].shape == (3, 1) and e["qidx"].tolist() == [[-1, -1, -1]]
    assert R.compile_queries([], VOCAB)["ids"].shape == (0, 3)
    with pytest.raises(ValueError):
        R.compile_queries([(1, 2)], VOCAB)


def test_relevance_and_default_queries():
    gt = [[[1, 2, 3], [4, 2, 3]], [[1, 2, 5]], [], [[1, 2, 3], [1, 2, 3]]]
    ptr, idx = R.relevance([[1, 2, 3], [1, 2, -1], [-1, -1, 3], [0, 0, 0], [-1, -1, -1]], gt)
    assert ptr.dtype == np.int32 and idx.dtype == np.int32
    assert ptr.tolist() == [0, 2, 5, 7, 7, 10] and idx.tolist() == [0, 3, 0, 1, 3, 0, 3, 0, 1, 3]
    assert R.default_queries(gt) == [(1, 2, 3), (1, 2, 5), (4, 2, 3)] and R.default_queries(gt, 1) == [(1, 2, 3)]
    many = [[[0, 0, 0]]] * (R.MAX_RELEVANT + 1)
    with pytest.raises(ValueError, match=r"\(0, 0, -1\)"):
        R.relevance([[0, 0, -1]], many)
    assert R.relevance([[0, 0, 0]], many[:-1])[0].tolist() == [0, R.MAX_RELEVANT]


def test_summarise():
    s = R.summarise([1, 3, 0, 12], [1.0, 0.5, np.nan, 0.25], [0, 0, -3, 0], (1, 5, 10))
    assert s["R@1"] == 1.0 / 3 and s["R@5"] == 2.0 / 3 and s["R@10"] == 2.0 / 3 and s["median_rank"] == 3.0
    assert abs(s["mrr"] - (1.0 + 1.0 / 3 + 1.0 / 12) / 3) < 1e-15 and abs(s["map"] - 1.75 / 3) < 1e-15
    assert s["n_valid"] == 3 and s["n_without_relevant"] == 1
    none = R.summarise([0], [np.nan], [-3], (1,))
    assert none["R@1"] is None and none["map"] is None and none["mrr"] is None and none["n_without_relevant"] == 1
    with pytest.raises(ValueError, match="-4"):          # a list the kernel refused is not "no relevant image"
        R.summarise([1, 0], [1.0, np.nan], [0, -4], (1,))


# ---- the C ABI and the command line ----------------------------------------------------------------------------------------------
def test_declared_symbols_equal_the_bindings():
    names = set(declared_symbols())
    assert {"sgg_query_logp", "sgg_retrieve_topk", "sgg_retrieve_ranks"} <= names and names == set(lib.SIGNATURES)
    for n in NEW:
        assert callable(getattr(lib.HipKernels, n))
    assert len(lib.SIGNATURES["sgg_query_logp"][1]) == 17 and len(lib.SIGNATURES["sgg_retrieve_topk"][1]) == 8
    assert len(lib.SIGNATURES["sgg_retrieve_ranks"][1]) == 11


def test_parser_knows_the_flags():
    sys.path.insert(0, ROOT)
    import train as T
    a = T.parse_args([])
    assert (a.retrieve_out, a.retrieve_queries, a.retrieve_top, a.retrieve_max_queries) == (None, None, None, None)
    a = T.parse_args(["--retrieve_out", "r.json", "--retrieve_queries", "q.json", "--retrieve_top", "7", "--retrieve_max_queries", "100",
                      "--max_test_images", "9", "--predict_samples", "4", "--eval_live"])
    assert (a.retrieve_out, a.retrieve_queries, a.retrieve_top, a.retrieve_max_queries) == ("r.json", "q.json", 7, 100)
    for bad in (["--retrieve_queries", "q.json"], ["--retrieve_top", "7"], ["--retrieve_max_queries", "5"],
                ["--retrieve_out", "r.json", "--retrieve_top", "0"], ["--retrieve_out", "r.json", "--retrieve_top", "1025"],
                ["--retrieve_out", "r.json", "--retrieve_max_queries", "0"], ["--retrieve_out", "r.json", "--likelihood_out", "n.json"],
                ["--retrieve_out", "r.json", "--predict_dir", "g"], ["--retrieve_out", "r.json", "--metrics_out", "m.json"],
                ["--retrieve_out", "r.json", "--saliency_dir", "s"], ["--retrieve_out", "r.json", "--test_only"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


# ---- SceneGraphGAN.retrieve on the reference kernels -------------------------------------------------------------------------------
@pytest.fixture
def cpu_gan(monkeypatch, tmp_path):
    sys.path.insert(0, ROOT)
    import train as T
    from sgg_amd import api
    K = RetrieveRefKernels()
    monkeypatch.setattr(T, "kernels_for", lambda device: K)
    monkeypatch.setattr(api, "kernels_for", lambda device: K)
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    gan = T.SceneGraphGAN(str(tmp_path / "ck"), str(tmp_path / "logs"), None, None, None, None, None, batch_size=4, lambda_=10,
                          synthetic=(4, 32, 11), device="cpu", critic_iters=1, resume=False)
    return T, K, gan


KEYS = {"retrieval", "ks", "n_queries", "n_images", "n_samples", "n_without_relevant", "n_out_of_vocab", "generator_weights", "decode"}


def test_retrieve_matches_the_restatement(cpu_gan, tmp_path, monkeypatch):
    T, K, gan = cpu_gan
    monkeypatch.setattr(R, "MAX_QUERIES", 4)         # nine queries go in blocks of 4, 4 and 1
    items = gan._evaluate_items(None, 5)             # the synthetic images and triples of test(); TEST_BATCH_SIZE = 2: the last batch is padded
    gt = [real for _, _, real in items]
    queries = [tuple(gt[0][0]), tuple(gt[1][2]), ("?", "w%d" % gt[2][0][1], gt[2][0][2]), (gt[3][1][0], None, -1), tuple(gt[4][4]),
               ("w3", "w3", "nope"), tuple(gt[2][3]), (-1, -1, -1), tuple(gt[0][0][:2]) + ((gt[0][0][2] + 1) % 11,), tuple(gt[1][0])]
    ids = R.compile_queries(queries, gan.vocab)["ids"]
    assert ids.shape[0] == 9
    assert not any((np.asarray(real) == ids[7]).all(axis=1).any() for real in gt), "query 7 is meant to have no relevant image"
    out = str(tmp_path / "retrieve.json")
    res = gan.retrieve(queries=queries, max_images=5, n_samples=3, ks=(1, 2, 5), top_k=3, return_details=True, out_path=out)
    assert json.load(open(out)) == res and set(res) == KEYS | {"details"}
    assert (res["n_queries"], res["n_images"], res["n_samples"], res["n_out_of_vocab"], res["generator_weights"], res["decode"]) == \
        (9, 5, 3, 1, "live", "likelihood") and res["ks"] == [1, 2, 5]
    assert set(res["retrieval"]) == {"R@1", "R@2", "R@5", "median_rank", "mrr", "map"}
    assert K.calls.count("query_logp") == 3 * 3 and K.calls.count("retrieve_topk") == 3 and K.calls.count("retrieve_ranks") == 3
    # the logits it was given are those of the passes (same noise stream), batch after batch, every block at the batch's column
    with contextlib.closing(gan._sample_batches([(k, x) for k, x, _ in items], 3, 2)) as batches:
        passes = [(i0, n, logits.numpy().copy()) for i0, n, _, logits in batches]
    assert [g[3] for g in K.given] == [0, 0, 0, 2, 2, 2, 4, 4, 4]
    full = np.full((9, 5), np.nan)
    for b, (i0, n, x) in enumerate(passes):
        for c in range(3):
            gx, glse, gids, _ = K.given[3 * b + c]
            assert np.array_equal(gx, x) and np.array_equal(gids, ids[4 * c:4 * c + 4])
            assert np.abs(glse - XR.lse64(x)).max() < 1e-5
        full[:, i0:i0 + n] = RR.query_logp(x, XR.lse64(x), ids)[:, :n]
    # the restatement's metrics on those logits
    ptr, idx = R.relevance(ids, gt)
    ref = RR.ranks(full, 5, ptr, idx)
    assert ref["status"].tolist().count(-3) == res["n_without_relevant"] >= 1 and ref["status"][7] == -3
    assert ref["status"][6] == 0 and ref["first_rank"][6] == 1 and ptr[7] - ptr[6] == 5, "three wildcards: every image is relevant"
    want = R.summarise(ref["first_rank"], ref["ap"], ref["status"], (1, 2, 5))
    for k, v in res["retrieval"].items():
        assert abs(v - want[k]) < 1e-12, k
    tidx, ttop = RR.topk(full, 5, 3)
    for q, d in enumerate(res["details"]):
        assert d["query"] == ids[q].tolist() and d["words"] == ["?" if t < 0 else "w%d" % t for t in ids[q]]
        assert [t["image"] for t in d["top"]] == [str(i) for i in tidx[q]]
        assert np.abs(np.array([t["score"] for t in d["top"]]) - ttop[q]).max() < 1e-4      # (fp32 networks and lse on the CPU)
        ok = ref["status"][q] == 0
        assert d["first_rank"] == (int(ref["first_rank"][q]) if ok else None)
        assert (abs(d["ap"] - ref["ap"][q]) < 1e-12) if ok else d["ap"] is None
    # the default queries: the distinct true triples, every one with a relevant image
    res2 = gan.retrieve(max_images=5, n_samples=3)
    assert set(res2) == KEYS and res2["n_queries"] == len(R.default_queries(gt)) and res2["n_without_relevant"] == 0
    # a score matrix above the budget is refused with the way out
    with pytest.raises(ValueError, match="max_queries"):
        gan.retrieve(max_images=5, n_samples=3, score_budget_bytes=64)
    with pytest.raises(ValueError):
        gan.retrieve(max_images=5, n_samples=3, top_k=0)


def test_other_modes_call_nothing_new(cpu_gan, tmp_path):
    T, K, gan = cpu_gan
    gan.test(max_images=2, out_path=str(tmp_path / "recalls.txt"))
    gan.predict(max_images=2, n_samples=2)
    gan.evaluate(max_images=2, n_samples=2, ks=(1,))
    gan.likelihood(max_images=2, n_samples=2)
    assert not [c for c in K.calls if c in NEW]
    gan.retrieve(max_images=2, n_samples=2)
    assert all(n in K.calls for n in NEW)
