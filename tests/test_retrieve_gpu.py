"""-m gpu: image retrieval by triple query - the kernels of csrc/retrieve.hip (HipKernels.query_logp, retrieve_topk, retrieve_ranks)
against the numpy fp64 restatement of tests/retrieve_ref.py, query_logp against triple_logp on full triples, and
SceneGraphGAN.retrieve end to end.

query_logp runs one query per thread in tiles of T = min(512, Q rounded up to a wave) threads, at least 256 (csrc/retrieve.hip), and
gathers S = min(64, N, min(24 T, 12288) / (u0 + u1 + u2)) samples per round.  QLP_CASES holds the issue's shapes: Q = 1 and 64 (a
256-thread workgroup mostly without queries), 257 (320 threads), 1000 (two tiles of 512, the second one partly empty), 4096 (eight
tiles); one round of 1, 3, 2 and 4 samples, and four rounds of 16 and one of 1 (N = 65).  A sixth case covers the remaining shape of
a round: 4096 queries over nearly 4096 distinct tokens per slot at V = 70 000, where a round holds ONE sample (three rounds; every
gather slot in use).
retrieve_topk takes 256 threads below 1024 images and 1024 from there; retrieve_ranks sorts 64 ... 4096 keys."""
import contextlib
import json

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from sgg_amd import retrieve as R
from tests import retrieve_ref as RR
from tests import xent_ref as XR

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
SENT = 777.25


def u32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- query_logp ------------------------------------------------------------------------------------------------------------------
#            N, nb, V,     Q,    logit scale, ld - 3 V, col0, lds - (col0 + nb), token pool (0: Q / 4), queries with wildcard patterns (0: all)
QLP_CASES = [(1, 1, 7, 1, 4.0, 0, 0, 0, 0, 0), (3, 5, 1000, 257, 80.0, 8, 3, 2, 0, 0), (65, 2, 1025, 1000, 4.0, 5, 1, 4, 0, 0),
             (2, 2, 70000, 64, 4.0, 3, 0, 1, 0, 0), (4, 3, 1000, 4096, 4.0, 0, 2, 3, 0, 0),
             (3, 2, 70000, 4096, 4.0, 1, 1, 0, 70000, 64)]
_qlp = {}


def qlp_case(hip, case):
    """Once per case: logits (scale * N(0, 1), or uniform in +-80), queries over a pool of tokens a quarter of Q wide (tokens repeat
    across queries) under every wildcard pattern in turn, the kernel's scores in a sentinel-filled matrix, the restatement."""
    if case not in _qlp:
        N, nb, V, Q, scale, extra, col0, tail, npool, nwild = case
        g = np.random.RandomState(900 + N + V + Q)
        x = (scale * (g.standard_normal((N, nb, 3, V)) if scale < 50 else g.uniform(-1, 1, (N, nb, 3, V)))).astype(np.float32)
        pool = g.choice(V, size=npool or max(1, min(V, Q // 4)), replace=False)
        ids = pool[g.randint(0, len(pool), size=(Q, 3))].astype(np.int64)
        if Q > 1:
            for q in range(nwild or Q):             # pattern q % 8: bit s set = slot s open; 7 = all three open
                for s in range(3):
                    if (q % 8) >> s & 1:
                        ids[q, s] = -1
        c = R.compile_queries(ids.tolist(), {i: i for i in range(V)})
        assert np.array_equal(c["ids"], ids) and max(c["ucount"]) <= Q
        buf = torch.full((N * nb, 3 * V + extra), float("nan"), device="cuda")
        buf[:, :3 * V] = torch.from_numpy(x.reshape(N * nb, 3 * V)).cuda()
        xd = buf[:, :3 * V].unflatten(1, (3, V)).unflatten(0, (N, nb))              # rows ld = 3 V + extra apart
        lse = torch.empty((N, nb, 3), device="cuda")
        hip.softmax_xent(torch.from_numpy(x).cuda(), None, lse=lse.view(-1))
        lds = col0 + nb + tail
        scores = torch.full((Q, lds), SENT, device="cuda")
        tok, qidx = torch.from_numpy(c["tok"]).cuda(), torch.from_numpy(c["qidx"]).cuda()
        hip.query_logp(xd, lse, tok, c["ucount"], qidx, scores, col0=col0)
        torch.cuda.synchronize()
        ref = RR.query_logp(x, lse.cpu().numpy(), ids)
        _qlp[case] = dict(x=x, xd=xd, lse=lse, ids=ids, c=c, tok=tok, qidx=qidx, scores=scores, ref=ref)
    return _qlp[case]


@pytest.mark.parametrize("case", QLP_CASES, ids=["N%d-nb%d-V%d-Q%d" % c[:4] for c in QLP_CASES])
def test_query_logp_matches_fp64_restatement(hip, case):
    N, nb, V, Q, scale, extra, col0, tail, npool, nwild = case
    d = qlp_case(hip, case)
    assert N * nb == 1 or d["xd"].reshape(N * nb, 3, V).stride(0) == 3 * V + extra
    h = d["scores"].cpu().numpy()
    mask = np.ones(h.shape, dtype=bool)
    mask[:, col0:col0 + nb] = False
    assert (u32(h[mask]) == u32(np.float32(SENT))).all(), "written outside the launch's columns"
    got = h[:, col0:col0 + nb]
    assert np.isfinite(got).all()
    err = float(np.abs(got - d["ref"]).max())
    print("query_logp N %d nb %d V %d Q %d scale %g: max |d| %.3e (max |score| %.1f)" % (N, nb, V, Q, scale, err, np.abs(d["ref"]).max()))
    assert err <= RR.QLP_TOL
    if scale < 50:
        assert err <= RR.QLP_SMALL_TOL, "logits of 4 N(0, 1): the bound measured over those cases"
    if Q > 1:
        allopen = (d["ids"] < 0).all(axis=1)
        assert allopen.any() and np.abs(got[allopen]).max() <= 2.0 ** -22, "three open slots score 0 up to the rounding of log N"
        for p in range(8):
            assert ((np.arange(Q) % 8 == p) & ((d["ids"] < 0).sum(axis=1) == bin(p).count("1"))).any(), "wildcard pattern %d missing" % p
    if npool:
        assert sum(d["c"]["ucount"]) > 6144, "the lists must be long enough for one sample per round"
    # a second call gives equal bits
    again = torch.full_like(d["scores"], SENT)
    hip.query_logp(d["xd"], d["lse"], d["tok"], d["c"]["ucount"], d["qidx"], again, col0=col0)
    assert np.array_equal(u32(again), u32(d["scores"])), "two calls differ"


@pytest.mark.parametrize("case", QLP_CASES, ids=["N%d-nb%d-V%d-Q%d" % c[:4] for c in QLP_CASES])
def test_query_logp_agrees_with_triple_logp_on_full_triples(hip, case):
    N, nb, V, Q, scale, extra, col0, tail, npool, nwild = case
    d = qlp_case(hip, case)
    full = np.nonzero((d["ids"] >= 0).all(axis=1))[0]
    assert len(full) >= 1
    gt = torch.from_numpy(np.tile(d["ids"][full][None], (nb, 1, 1))).cuda()
    cnt = torch.full((nb,), len(full), dtype=I32, device="cuda")
    res = hip.triple_logp(d["xd"], d["lse"], gt, cnt)
    assert (res["status"] == 0).all()
    mix = res["mix"].cpu().numpy().T                 # [full queries, nb]
    got = d["scores"].cpu().numpy()[full, col0:col0 + nb]
    err = float(np.abs(got - mix).max())
    print("query_logp vs triple_logp N %d nb %d V %d Q %d scale %g: max |d| %.3e over %d full triples" % (N, nb, V, Q, scale, err, len(full)))
    assert err <= RR.QLP_VS_TLP_TOL
    if N == 1:
        assert np.array_equal(u32(got), u32(mix)), "one sample: no sum to order, the same bits"


def test_query_logp_rejects_bad_arguments(hip):
    d = qlp_case(hip, QLP_CASES[0])
    sc = torch.zeros((1, 4), device="cuda")
    with pytest.raises(AssertionError):
        hip.query_logp(d["xd"], d["lse"], d["tok"], d["c"]["ucount"], d["qidx"], sc, col0=4)
    with pytest.raises(Exception, match="ucount"):
        hip.query_logp(d["xd"], d["lse"], d["tok"], [2, 1, 1], d["qidx"], sc)
    lib = hip.lib
    a = [d["xd"].data_ptr(), 21, d["lse"].data_ptr(), 1, 1, 7, d["tok"].data_ptr(), 1, 1, 1, 1, d["qidx"].data_ptr(), 1, sc.data_ptr(), 4, 0, None]
    assert lib.sgg_query_logp(*a) == 0
    for pos, val, word in ((3, 4097, b"4096"), (12, 4097, b"4096"), (1, 20, b"ld"), (7, 2, b"U"), (15, 4, b"col0"), (0, None, b"null")):
        b = list(a)
        b[pos] = val
        assert lib.sgg_query_logp(*b) == -1 and word in lib.sgg_last_error(), (pos, lib.sgg_last_error())
    torch.cuda.synchronize()
    # an index outside a slot's list, or a listed token outside the vocabulary: NaN for that query, nothing read out of bounds
    qbad = torch.tensor([[0, 0, 5], [0, 0, 0]], dtype=I32, device="cuda")
    tbad = torch.tensor([[3, 0], [7, 0], [2, 0]], dtype=I32, device="cuda")
    sc2 = torch.zeros((2, 1), device="cuda")
    hip.query_logp(d["xd"], d["lse"], tbad, [1, 1, 1], qbad, sc2)
    assert torch.isnan(sc2).all()


# ---- retrieve_topk -----------------------------------------------------------------------------------------------------------------
def topk_rows(n, Q, pad):
    """[Q * 5, n + pad] fp32: per pattern Q rows - random, all equal, blocks of ties, negative, +-0 among small values - with
    garbage (NaN, +Inf, huge) in the padding columns."""
    g = np.random.RandomState(40 + n + Q)
    rows = []
    for _ in range(Q):
        rows.append(g.standard_normal(n) * 5.0)
        rows.append(np.full(n, -3.25))
        rows.append(-np.floor(g.uniform(0, max(2, n // 7), n)) * 0.5)         # ~7 images per score: ties straddle every K
        rows.append(-np.abs(g.standard_normal(n)) - g.randint(0, 2, n) * 100.0)
        z = g.choice(np.array([0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0]), n)
        rows.append(z)
    sc = np.empty((len(rows), n + pad), dtype=np.float32)
    sc[:, :n] = np.asarray(rows, dtype=np.float32)
    sc[:, n:] = np.array([np.nan, np.inf, 3e38, -np.inf])[np.arange(pad) % 4]
    return sc


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
@pytest.mark.parametrize("Q", [1, 3])
def test_retrieve_topk_is_exact(hip, n, Q):
    sc = topk_rows(n, Q, 5)
    scd = torch.from_numpy(sc).cuda()
    for K in (1, 10, 128):
        res = hip.retrieve_topk(scd, n, K)
        idx, top = res["idx"].cpu().numpy(), res["scores"].cpu().numpy()
        ridx, rtop = RR.topk(sc, n, K)
        assert np.array_equal(idx, ridx), "n %d K %d: rows %s differ" % (n, K, np.nonzero((idx != ridx).any(axis=1))[0].tolist())
        M = min(K, n)
        assert np.array_equal(u32(top[:, :M]), u32(rtop[:, :M])), "the scores are the inputs' bits"
        assert (idx[:, M:] == -1).all() and np.isnan(top[:, M:]).all()
        again = hip.retrieve_topk(scd, n, K)
        assert np.array_equal(u32(again["idx"]), u32(res["idx"])) and np.array_equal(u32(again["scores"]), u32(res["scores"]))
    if n == 5000 and Q == 3:
        res = hip.retrieve_topk(scd, n, 1024)
        assert np.array_equal(res["idx"].cpu().numpy(), RR.topk(sc, n, 1024)[0])
        lib = hip.lib
        a = [scd.data_ptr(), n + 5, 15, n, 10, res["idx"].data_ptr(), res["scores"].data_ptr(), None]
        for pos, val, word in ((4, 1025, b"1024"), (4, 0, b"1024"), (1, n - 1, b"lds"), (3, (1 << 21) + 1, b"2^21"), (0, None, b"null")):
            b = list(a)
            b[pos] = val
            assert lib.sgg_retrieve_topk(*b) == -1 and word in lib.sgg_last_error()


# ---- retrieve_ranks ----------------------------------------------------------------------------------------------------------------
def test_retrieve_ranks_are_exact(hip):
    n, pad = 5000, 3
    g = np.random.RandomState(11)
    rel = [np.array([], dtype=np.int64), np.array([4321]), np.arange(4096), np.sort(g.choice(n, 4096, replace=False)),
           np.sort(g.choice(n, 70, replace=False)), np.array([0, n - 1]), np.sort(g.choice(n, 65, replace=False)),
           np.array([], dtype=np.int64)]
    Q = len(rel)
    sc = np.empty((Q, n + pad), dtype=np.float32)
    sc[:, n:] = np.nan
    sc[:, :n] = g.standard_normal((Q, n)) * 3.0
    sc[2, :n] = np.floor(sc[2, :n])                                         # ties among relevant images
    sc[4, :n] = -np.floor(g.uniform(0, 40, n))                              # ties between relevant and irrelevant images
    sc[5, :n] = 0.0
    sc[5, 1:n:2] = -0.0                                                     # all equal (+-0): the rank is the index + 1
    sc[6, :n] = 1.5
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rel])]).astype(np.int32)
    idx = np.concatenate(rel).astype(np.int32)
    scd = torch.from_numpy(sc).cuda()
    res = hip.retrieve_ranks(scd, n, torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda())
    ref = RR.ranks(sc, n, ptr, idx)
    for name in ("ranks", "first_rank", "status"):
        assert np.array_equal(res[name].cpu().numpy(), ref[name]), name
    assert ref["status"].tolist() == [-3, 0, 0, 0, 0, 0, 0, -3] and ref["ranks"][ptr[5]:ptr[6]].tolist() == [1, n]
    assert np.array_equal(ref["ranks"][ptr[6]:ptr[7]], rel[6] + 1)
    ap = res["ap"].cpu().numpy()
    ok = ref["status"] == 0
    assert np.isnan(ap[~ok]).all() and (res["first_rank"].cpu().numpy()[~ok] == 0).all()
    err = float(np.abs(ap[ok] - ref["ap"][ok]).max())
    print("retrieve_ranks: max |AP - fp64| %.3e" % err)
    assert err <= 1e-12
    again = hip.retrieve_ranks(scd, n, torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda())
    for name in res:
        assert np.array_equal(res[name].cpu().numpy().view(np.uint8), again[name].cpu().numpy().view(np.uint8)), name
    # an all-empty relevance list; collections on both sides of the wave width and of 4096 images with EVERY image relevant
    one = hip.retrieve_ranks(scd[:2], n, torch.zeros(3, dtype=I32, device="cuda"), torch.zeros(1, dtype=I32, device="cuda"))
    assert one["status"].tolist() == [-3, -3] and one["first_rank"].tolist() == [0, 0]
    for m in (1, 63, 64, 65, 4096):
        small = np.ascontiguousarray(sc[:5, :m + 2])
        r5 = [np.arange(m), np.array([m - 1]), np.array([], dtype=np.int64), np.arange(0, m, 2), np.array([0])]
        p5 = np.concatenate([[0], np.cumsum([len(r) for r in r5])]).astype(np.int32)
        i5 = np.concatenate(r5).astype(np.int32)
        got = hip.retrieve_ranks(torch.from_numpy(small).cuda(), m, torch.from_numpy(p5).cuda(), torch.from_numpy(i5).cuda())
        want = RR.ranks(small, m, p5, i5)
        for name in ("ranks", "first_rank", "status"):
            assert np.array_equal(got[name].cpu().numpy(), want[name]), (m, name)
        okm = want["status"] == 0
        assert np.abs(got["ap"].cpu().numpy()[okm] - want["ap"][okm]).max() <= 1e-12 and want["ap"][0] == 1.0
    # a list that names an image outside the collection is refused by status, nothing is read out of bounds
    bad = hip.retrieve_ranks(scd[:1], n, torch.tensor([0, 2], dtype=I32, device="cuda"), torch.tensor([5, n], dtype=I32, device="cuda"))
    assert bad["status"].tolist() == [-4] and bad["first_rank"].tolist() == [0] and torch.isnan(bad["ap"]).all()
    long = hip.retrieve_ranks(scd[:1], n, torch.tensor([0, 4097], dtype=I32, device="cuda"), torch.arange(4097, dtype=I32, device="cuda"))
    assert long["status"].tolist() == [-4], "more than 4096 relevant images: refused by status"


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_retrieve_end_to_end(tmp_path, monkeypatch):
    """The untrained model of tests/test_predict_gpu.py, batch_size 8: TEST_BATCH_SIZE 4, 32 samples per image, five images = one full
    and one padded image batch; nine queries, one with open slots, one without a relevant image."""
    from sgg_amd.api import kernels_for
    from tests.test_eval_batched_gpu import _gan
    S, Vv = 64, 50
    gan = _gan(tmp_path, 8, S, Vv)
    g = torch.Generator().manual_seed(78)
    imgs = [torch.randn((S, S, 3), generator=g) for _ in range(5)]
    gts = [[[1, 2, 3], [4, 5, 6]], [[0, Vv - 1, 0]], [[7, 7, 7], [1, 2, 9], [8, 1, 1]], [[5, 5, 5], [1, 2, 3]], [[9, 8, 7], [6, 5, 4]]]
    items = list(zip(imgs, gts))
    queries = [("w1", "w2", "w3"), (4, 5, 6), (0, Vv - 1, 0), ("w1", "w2", "?"), (7, 7, 7), (8, 1, 1), (5, 5, 5), (9, 8, 7), (3, 3, 3)]
    K = kernels_for(gan.device)
    dumped, mats = [], []
    real_qlp, real_topk = K.query_logp, K.retrieve_topk

    def qlp(logits, lse, tok, ucount, qidx, scores, col0=0):
        dumped.append((logits.cpu().numpy().copy(), lse.cpu().numpy().copy(), col0))
        return real_qlp(logits, lse, tok, ucount, qidx, scores, col0=col0)

    def topk(scores, n_images, Kk, out=None):
        mats.append(scores.cpu().numpy().copy())
        return real_topk(scores, n_images, Kk, out=out)
    monkeypatch.setattr(K, "query_logp", qlp)
    monkeypatch.setattr(K, "retrieve_topk", topk)
    out = str(tmp_path / "retrieve.json")
    res = gan.retrieve(queries=queries, items=items, ks=(1, 2, 5), top_k=3, return_details=True, out_path=out)
    assert json.load(open(out)) == res
    assert (res["n_queries"], res["n_images"], res["n_samples"], res["n_out_of_vocab"], res["n_without_relevant"]) == (9, 5, 32, 0, 1)
    assert len(dumped) == 2 and [d[2] for d in dumped] == [0, 4] and len(mats) == 1 and mats[0].shape == (9, 8)
    ids = R.compile_queries(queries, gan.vocab)["ids"]
    dev = mats[0]
    # the score matrix against the restatement on the dumped logits (with the device's own lse)
    worst = 0.0
    for x, lse, col0 in dumped:
        n = min(4, 5 - col0)
        ref = RR.query_logp(x, lse, ids)
        worst = max(worst, float(np.abs(dev[:, col0:col0 + n] - ref[:, :n]).max()))
    print("retrieve() score matrix: max |d| %.3e" % worst)
    assert worst <= RR.QLP_SMALL_TOL <= RR.QLP_TOL
    # top-K and ranks: the restatement applied to the device's own score matrix
    ptr, idx = R.relevance(ids, gts)
    assert ptr[4] - ptr[3] == 3 and ptr[9] == ptr[8], "the query with an open slot has three relevant images, the last one none"
    rr = RR.ranks(dev, 5, ptr, idx)
    tidx, ttop = RR.topk(dev, 5, 3)
    for q, d in enumerate(res["details"]):
        assert [t["image"] for t in d["top"]] == [str(i) for i in tidx[q]] and [t["score"] for t in d["top"]] == [float(s) for s in ttop[q]]
        ok = rr["status"][q] == 0
        assert d["first_rank"] == (int(rr["first_rank"][q]) if ok else None)
        assert (abs(d["ap"] - rr["ap"][q]) <= 1e-12) if ok else d["ap"] is None
    want = R.summarise(rr["first_rank"], rr["ap"], rr["status"], (1, 2, 5))
    for k, v in res["retrieval"].items():
        assert abs(v - want[k]) <= 1e-12, k
    # a second call gives equal bits
    res2 = gan.retrieve(queries=queries, items=items, ks=(1, 2, 5), top_k=3, return_details=True)
    assert res2 == res and len(mats) == 2 and np.array_equal(u32(mats[1][:, :5]), u32(mats[0][:, :5]))
