"""-m gpu: K-best decoding - the kernels of csrc/kbest.hip (HipKernels.kbest_triples, kbest_merge) against the numpy fp64 reference
of tests/kbest_ref.py, SceneGraphGAN.predict / evaluate with decode="kbest" on the untrained model of tests/test_predict_gpu.py,
and train.py --decode kbest.

Gap condition.  Device and reference may order two triples differently only where their log-probabilities are closer than the
two errors together, 2 x LP_TOL.  Position u of a ranked list is DECIDED where the reference's gaps to both neighbours exceed that;
the identities are compared at every decided position, every stretch of undecided positions must hold the same SET of triples as
the reference's stretch, and every case asserts as an input condition (from the reference alone) that row 0 is decided throughout
and that most positions of all rows are.  (A whole case cannot be decided throughout once it has
thousands of gaps: 70 rows x 127 gaps of mean 2e-2 hold some below 2e-5.)  The VALUES are compared at every position."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sgg_amd import kbest
from sgg_amd.metrics import RecallAccumulator
from tests import kbest_ref as KR
from tests.kbest_ref import LP_TOL
from tests.test_eval_batched_gpu import _gan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 97
OFF = PAD + PAD % 2                 # (an even element offset keeps every view 8-byte aligned)
SENTINEL = {torch.int64: -777, torch.int32: -777, torch.float32: 777.25}
I64, I32, F32 = torch.int64, torch.int32, torch.float32


def guarded_outputs(shapes):
    """{name: (shape, dtype)} -> (big, out): every output inside a larger buffer filled with a sentinel."""
    big, out = {}, {}
    for name, (shape, dt) in shapes.items():
        n = int(np.prod(shape))
        big[name] = torch.full((OFF + n + PAD,), SENTINEL[dt], dtype=dt, device="cuda")
        out[name] = big[name][OFF:OFF + n].view(shape)
    return big, out


def assert_guards(big, out):
    for name, b in big.items():
        flat, n, s = b.cpu().numpy(), out[name].numel(), SENTINEL[b.dtype]
        assert (flat[:OFF] == s).all() and (flat[OFF + n:] == s).all(), "%s: written outside its extent" % name


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def decided(lp, tol2):
    """bool [K]: the reference's gaps to both neighbours exceed tol2."""
    gap = -np.diff(lp)
    ok = np.ones(lp.shape, dtype=bool)
    ok[1:] &= gap > tol2
    ok[:-1] &= gap > tol2
    return ok


def same_sets_in_undecided_stretches(got, want, ok):
    """Every maximal run of undecided positions holds the same set of triples in `got` as in `want` ([K, 3] each)."""
    u, K = 0, len(ok)
    while u < K:
        if ok[u]:
            u += 1
            continue
        v = u
        while v < K and not ok[v]:
            v += 1
        if set(map(tuple, got[u:v].tolist())) != set(map(tuple, want[u:v].tolist())):
            return False
        u = v
    return True


# ---- kbest_triples -----------------------------------------------------------------------------------------------------------
#               R, V,     K,   scale, kind,        extra row stride
TRIPLE_CASES = [(1, 1, 1, 1.0, "normal", 0), (2, 2, 8, 1.0, "normal", 0), (3, 7, 50, 2.0, "normal", 0), (70, 40, 128, 2.0, "normal", 0),
                (5, 1000, 100, 4.0, "normal", 24), (2, 4097, 128, 4.0, "normal", 0), (2, 70000, 128, 4.0, "normal", 0),
                (3, 50, 128, 2.0, "quantised", 0)]
_triple_cache = {}


def triple_case(case):
    """(logits float32 [R, 3, V], per-row reference (triples, lp, ranks)); computed once per case and shared.  At V <= 40 the
    reference is brute_force_row, the ranking of all V^3 triples (M = min(K, V) = V in those cases, so kbest_row would be the same
    call); above, kbest_row on the cube of the top M tokens, which tests/test_kbest_cpu.py holds against brute force."""
    if case not in _triple_cache:
        R, V, K, scale, kind, _ = case
        g = np.random.RandomState(4000 + V + K)
        x = (scale * g.standard_normal((R, 3, V))).astype(np.float32)
        if kind == "quantised":
            x = (np.round(x * 2.0) / 2.0).astype(np.float32)
        row = KR.brute_force_row if V <= 40 else KR.kbest_row
        _triple_cache[case] = (x, [row(x[r], K) for r in range(R)])
    return _triple_cache[case]


def strided(x, extra):
    """x [R, 3, V] on the device as a view of rows 3 V + extra floats apart (the rest NaN)."""
    R, _, V = x.shape
    buf = torch.full((R, 3 * V + extra), float("nan"), device="cuda")
    buf[:, :3 * V] = torch.from_numpy(x.reshape(R, 3 * V)).cuda()
    return buf[:, :3 * V].unflatten(1, (3, V))


@pytest.mark.parametrize("case", TRIPLE_CASES, ids=["R%d-V%d-K%d-s%g-%s-ld%d" % c for c in TRIPLE_CASES])
def test_kbest_triples_matches_fp64_reference(hip, case):
    R, V, K, scale, kind, extra = case
    x, ref = triple_case(case)
    assert float(np.abs(x).max()) <= 22.0           # (the range LP_TOL_CAP is stated for)
    xd = strided(x, extra)
    assert xd.stride(0) == 3 * V + extra
    big, out = guarded_outputs({"triples": ((R, K, 3), I64), "logp": ((R, K), F32), "lse": ((R, 3), F32)})
    res = hip.kbest_triples(xd, K, out=out)
    torch.cuda.synchronize()
    assert_guards(big, out)
    t, lp, lse = (res[n].cpu().numpy() for n in ("triples", "logp", "lse"))
    a64 = x.astype(np.float64) - KR.lse64(x)[:, :, None]
    err_lse = float(np.abs(lse - KR.lse64(x)).max())
    err_own = err_sorted = 0.0
    n_decided = 0
    for r in range(R):
        rt, rlp, _ = ref[r]
        assert ((t[r] >= 0) & (t[r] < V)).all()
        assert len({tuple(q) for q in t[r].tolist()}) == K, "row %d: repeated triple" % r
        assert (np.diff(lp[r]) <= 0).all(), "row %d: logp increases" % r
        own = (a64[r, 0, t[r, :, 0]] + a64[r, 1, t[r, :, 1]]) + a64[r, 2, t[r, :, 2]]
        err_own = max(err_own, float(np.abs(lp[r] - own).max()))
        err_sorted = max(err_sorted, float(np.abs(lp[r] - rlp).max()))
        if kind == "normal":
            ok = decided(rlp, 2 * LP_TOL)
            n_decided += int(ok.sum())
            assert r > 0 or ok.all(), "input condition: row 0 decided throughout (smallest gap %.3g)" % float((-np.diff(rlp)).min())
            assert np.array_equal(t[r][ok], rt[ok]), "row %d: triples differ from the reference at decided positions" % r
            assert same_sets_in_undecided_stretches(t[r], rt, ok), "row %d: an undecided stretch holds other triples" % r
        else:       # exact ties: neighbours with bit-equal logp stand in the order of their slot ranks (i, j, l)
            rank_of = [np.argsort(KR.slot_order(x[r, s])) for s in range(3)]
            ranks = np.stack([rank_of[s][t[r, :, s]] for s in range(3)], axis=1)
            same = np.nonzero(bits(lp[r])[1:] == bits(lp[r])[:-1])[0]
            assert r > 0 or len(same) > 10, "input condition: exact ties expected"
            for u in same.tolist():
                assert tuple(ranks[u]) < tuple(ranks[u + 1]), "row %d: tie at %d out of rank order" % (r, u)
    print("kbest_triples %s: err lse %.3g, logp against own triple %.3g, against sorted reference %.3g" % (case, err_lse, err_own, err_sorted))
    if kind == "normal":
        assert n_decided >= 0.95 * R * K, "input condition: at least 95 %% of the positions decided (%d of %d)" % (n_decided, R * K)
    assert err_lse <= LP_TOL and err_own <= LP_TOL and err_sorted <= LP_TOL, (err_lse, err_own, err_sorted)
    again = hip.kbest_triples(xd, K)                # allocated by the binding; two calls are bit-equal
    for n in ("triples", "logp", "lse"):
        assert np.array_equal(bits(again[n].cpu().numpy()), bits(res[n].cpu().numpy())), n


def test_kbest_triples_rejects_bad_arguments(hip):
    from sgg_amd.lib import SggError
    x = torch.zeros((2, 3, 50), device="cuda")
    for K in (0, 129):
        with pytest.raises(SggError, match="K"):
            hip.kbest_triples(x, K)
    with pytest.raises(SggError, match="V\\^3"):
        hip.kbest_triples(torch.zeros((2, 3, 5), device="cuda"), 126)
    lib = hip.lib
    t, lp, lse = torch.zeros((2, 8, 3), dtype=I64, device="cuda"), torch.zeros((2, 8), device="cuda"), torch.zeros((2, 3), device="cuda")
    # (V > 2^21 is refused before anything is read: no such tensor is needed)
    assert lib.sgg_kbest_triples(x.data_ptr(), 3 * ((1 << 21) + 1), 2, (1 << 21) + 1, 8, t.data_ptr(), lp.data_ptr(), lse.data_ptr(),
                                 None) == -1 and b"2^21" in lib.sgg_last_error()
    assert lib.sgg_kbest_triples(x.data_ptr(), 149, 2, 50, 8, t.data_ptr(), lp.data_ptr(), lse.data_ptr(), None) == -1
    assert b"stride" in lib.sgg_last_error()
    args = [x.data_ptr(), 150, 2, 50, 8, t.data_ptr(), lp.data_ptr(), lse.data_ptr(), None]
    for null_at in (0, 5, 6, 7):
        a = list(args)
        a[null_at] = None
        assert lib.sgg_kbest_triples(*a) == -1 and b"null" in lib.sgg_last_error()
    assert lib.sgg_kbest_triples(*args) == 0
    torch.cuda.synchronize()


# ---- kbest_merge -------------------------------------------------------------------------------------------------------------
#              N,  nb, Kc,  V,    pert
MERGE_CASES = [(1, 1, 1, 5, None), (1, 3, 128, 1000, None), (32, 2, 128, 50, 0.5), (5, 3, 7, 9, 0.5), (256, 1, 16, 1000, 0.5),
               (4, 2, 128, 1000, 0.0)]
MERGE_NAMES = ("triples", "scores", "best_sample", "best_logp", "counts", "n_distinct")
_merge_cache = {}


def merge_logits(case):
    if case not in _merge_cache:
        N, nb, Kc, V, pert = case
        g = np.random.RandomState(5000 + N + Kc + V)
        base = 3.0 * g.standard_normal((nb, 3, V))
        x = base[None] + (pert or 0.0) * g.standard_normal((N, nb, 3, V))
        _merge_cache[case] = x.astype(np.float32)
    return _merge_cache[case]


def merge_shapes(nb, K):
    return {"triples": ((nb, K, 3), I64), "scores": ((nb, K), F32), "best_sample": ((nb, K), I32), "best_logp": ((nb, K), F32),
            "counts": ((nb, K), I32), "n_distinct": ((nb,), I32)}


def run_merge(hip, lists, xd, lse, nb, K):
    big, out = guarded_outputs(merge_shapes(nb, K))
    res = hip.kbest_merge(lists, xd, lse, K, out=out)
    torch.cuda.synchronize()
    assert_guards(big, out)
    return {n: res[n].cpu().numpy() for n in MERGE_NAMES}


@pytest.mark.parametrize("case", MERGE_CASES, ids=["N%d-nb%d-Kc%d-V%d-pert%s" % c for c in MERGE_CASES])
def test_kbest_merge_matches_fp64_reference(hip, case):
    """The kernel is fed the device's own kbest_triples outputs (triples and lse) of the logits; the reference merges the same triples
    and the same lse over the same logits in fp64: only the merge is under test."""
    N, nb, Kc, V, pert = case
    x = merge_logits(case)
    xd = torch.from_numpy(x).cuda()
    per = hip.kbest_triples(xd, Kc)
    lists, lse = per["triples"].view(N, nb, Kc, 3), per["lse"].view(N, nb, 3)
    lists_h, lse_h, logp_h = lists.cpu().numpy(), lse.cpu().numpy(), per["logp"].view(N, nb, Kc).cpu().numpy()
    ref = [KR.merge_image(lists_h[:, j], x[:, j], lse_h[:, j]) for j in range(nb)]
    nd = [r["n_distinct"] for r in ref]
    for j, r in enumerate(ref):             # input conditions, from the reference alone
        n_all, n_one = int((r["counts"] == N).sum()), int((r["counts"] == 1).sum())
        print("kbest_merge %s image %d: %d distinct, %d in all lists, %d in one" % (case, j, nd[j], n_all, n_one))
        if pert == 0.5:
            assert n_all > 0 and n_one > 0, "input condition: triples in every list and triples in one list only"
    full = run_merge(hip, lists, xd, lse, nb, N * Kc)            # every slot: all distinct triples and the padding behind them
    err_score = err_best = 0.0
    for j, r in enumerate(ref):
        U = nd[j]
        assert int(full["n_distinct"][j]) == U
        got = {tuple(t): u for u, t in enumerate(full["triples"][j, :U].tolist())}
        assert len(got) == U and set(got) == set(map(tuple, r["triples"].tolist())), "image %d: another set of triples" % j
        at = np.array([got[tuple(t)] for t in r["triples"].tolist()])        # device slot of every reference entry
        assert np.array_equal(full["counts"][j, at], r["counts"])
        err_score = max(err_score, float(np.abs(full["scores"][j, at] - r["scores"]).max()))
        err_best = max(err_best, float(np.abs(full["best_logp"][j, at] - r["best_logp"]).max()))
        clear = r["gap2"] > 2 * LP_TOL
        assert np.array_equal(full["best_sample"][j, at][clear], r["best_sample"][clear])
        s = full["scores"][j, :U]
        assert (np.diff(s) <= 0).all(), "image %d: scores increase" % j
        packed = KR.pack(full["triples"][j, :U])
        tie = bits(s)[1:] == bits(s)[:-1]
        assert (packed[1:][tie] > packed[:-1][tie]).all(), "image %d: equal scores out of packed-triple order" % j
        # the padding behind the list
        assert (full["triples"][j, U:] == -1).all() and np.isnan(full["scores"][j, U:]).all() and np.isnan(full["best_logp"][j, U:]).all()
        assert (full["best_sample"][j, U:] == -1).all() and (full["counts"][j, U:] == 0).all()
        if N == 1:          # one sample: the merged list is the sample's own list
            assert U == Kc and np.array_equal(full["triples"][j, :U], lists_h[0, j]) and (full["best_sample"][j, :U] == 0).all()
            assert float(np.abs(s - logp_h[0, j]).max()) <= 2 * LP_TOL
        if pert == 0.0:     # identical samples: every list is the same list
            assert U == Kc and (full["counts"][j, :U] == N).all() and np.array_equal(full["triples"][j, :U], lists_h[0, j])
            assert float(np.abs(s - logp_h[0, j]).max()) <= 2 * LP_TOL
    print("kbest_merge %s: err scores %.3g, best_logp %.3g" % (case, err_score, err_best))
    assert err_score <= 2 * LP_TOL and err_best <= 2 * LP_TOL, (err_score, err_best)
    # K = all distinct candidates of the smallest image, and K = 20: the head of the full output, bit for bit
    for K in sorted({min(nd), min(20, min(nd))}):
        cut = run_merge(hip, lists, xd, lse, nb, K)
        for n in MERGE_NAMES[:-1]:
            assert np.array_equal(bits(cut[n]), bits(np.ascontiguousarray(full[n][:, :K]))), (K, n)
        assert np.array_equal(cut["n_distinct"], full["n_distinct"])
        for j, r in enumerate(ref):     # nothing better was left out
            kept = {tuple(t) for t in cut["triples"][j].tolist()}
            sc = {tuple(t): v for t, v in zip(r["triples"].tolist(), r["scores"].tolist())}
            worst = min(sc[t] for t in kept)
            assert all(v <= worst + 4 * LP_TOL for t, v in sc.items() if t not in kept), "image %d: a better triple was left out" % j
    again = hip.kbest_merge(lists, xd, lse, N * Kc)
    for n in MERGE_NAMES:
        assert np.array_equal(bits(again[n].cpu().numpy()), bits(full[n])), n


def test_kbest_merge_rejects_bad_arguments(hip):
    from sgg_amd.lib import SggError
    x = torch.zeros((17, 1, 3, 50), device="cuda")
    lse = torch.zeros((17, 1, 3), device="cuda")
    lists = torch.zeros((17, 1, 241, 3), dtype=I64, device="cuda")          # 17 x 241 = 4097
    with pytest.raises(SggError, match="4096"):
        hip.kbest_merge(lists, x, lse, 4)
    small = torch.zeros((17, 1, 2, 3), dtype=I64, device="cuda")
    for K in (0, 35):
        with pytest.raises(SggError, match="K"):
            hip.kbest_merge(small, x, lse, K)
    lib = hip.lib
    o = torch.zeros((64,), dtype=I64, device="cuda")
    args = [small.data_ptr(), x.data_ptr(), 150, lse.data_ptr(), 17, 1, 2, 50, 4] + [o.data_ptr()] * 6 + [None]
    for null_at in (0, 1, 3, 9, 12, 14):
        a = list(args)
        a[null_at] = None
        assert lib.sgg_kbest_merge(*a) == -1 and b"null" in lib.sgg_last_error()
    a = list(args)
    a[7] = (1 << 21) + 1
    assert lib.sgg_kbest_merge(*a) == -1 and b"2^21" in lib.sgg_last_error()


# ---- SceneGraphGAN.predict / evaluate with decode="kbest" ---------------------------------------------------------------------
S, V, N_IMG, NB, NS = 64, 50, 5, 4, 4
WIDTH = kbest.list_width(NS, V)


def _images():
    g = torch.Generator().manual_seed(77)
    return [torch.randn((S, S, 3), generator=g) for _ in range(N_IMG)]


def _untrained_gan(tmp_path):
    gan = _gan(tmp_path, 8, S, V)
    assert gan.TEST_BATCH_SIZE == NB == NS and WIDTH == 128
    return gan


def _count_trunk_forwards(gan, fn):
    from sgg_amd.trunk import Trunk
    calls = {"G": 0, "D": 0}
    orig = Trunk.forward

    def counting(self, *a, **kw):
        calls["G" if any(self is n.trunk for n in gan.g._nets.values()) else "D"] += 1
        return orig(self, *a, **kw)

    Trunk.forward = counting
    try:
        res = fn()
    finally:
        Trunk.forward = orig
    return res, calls


def _sampled_logits(gan, imgs):
    """Per image batch (logits [NS, NB, 3, V], alphas) of g.sample on the noise stream of predict(decode="kbest"): per image ONE draw
    of [TEST_BATCH_SIZE, 512] from seed + 123, the first NS rows."""
    gen = torch.Generator().manual_seed(gan.seed + 123)
    out = []
    for i0 in range(0, len(imgs), NB):
        chunk = imgs[i0:i0 + NB]
        images = torch.stack(chunk + [chunk[-1]] * (NB - len(chunk))).cuda()
        noise = torch.zeros((NS, NB, 512))
        for j in range(len(chunk)):
            noise[:, j] = torch.randn((NB, 512), generator=gen)[:NS]
        logits = gan.g.sample(images, NS, noise.cuda()).cpu().numpy()
        out.append((logits, gan.g.alphas.cpu().numpy()))
    return out


def test_predict_kbest(tmp_path):
    """Untrained model, batch_size 8: TEST_BATCH_SIZE 4 = the default sample count of this mode, list width 128; 5 images = one full
    and one padded image batch.  The reference: the fp64 K-best lists of the recomputed g.sample logits, merged in fp64."""
    gan = _untrained_gan(tmp_path)
    imgs = _images()
    before = gan.predict(items=imgs)                    # today's path, before anything else ran
    preds, calls = _count_trunk_forwards(gan, lambda: gan.predict(items=imgs, decode="kbest", with_attention=True))
    assert calls == {"G": 2, "D": 0}, calls             # two image batches, one generator encoder pass each, no critic
    assert len(preds) == N_IMG
    batches = _sampled_logits(gan, imgs)
    n_compared = 0
    for i, p in enumerate(preds):
        logits, al = batches[i // NB]
        j = i % NB
        assert sorted(p) == sorted(["image", "n_distinct", "ordering", "triples", "scores", "first_sample", "best_logp", "counts",
                                    "words", "graph", "attention"])
        assert p["ordering"] == kbest.ORDERING and p["image"] == str(i)
        nd = p["n_distinct"]
        assert nd >= WIDTH and p["triples"].shape == (nd, 3) and (np.diff(p["scores"]) <= 0).all()
        assert p["words"] == [["w%d" % t for t in row] for row in p["triples"].tolist()]
        assert [e["count"] for e in p["graph"]["edges"]] == p["counts"].tolist() and len(p["graph"]["edges"]) == nd
        # reference lists of the NS head rows; input condition: the 128th and 129th triple of every row are further apart than both errors
        rows = [KR.kbest_row(logits[k, j], WIDTH + 1) for k in range(NS)]
        edge = min(float(lp[WIDTH - 1] - lp[WIDTH]) for _, lp, _ in rows)
        assert edge > 2 * LP_TOL, "input condition: image %d: the lists' last gap is %.3g" % (i, edge)
        ref = KR.merge_image(np.stack([t[:WIDTH] for t, _, _ in rows]), logits[:, j], KR.lse64(logits[:, j]))
        assert nd == ref["n_distinct"] and set(map(tuple, p["triples"].tolist())) == set(map(tuple, ref["triples"].tolist()))
        assert float(np.abs(p["scores"] - ref["scores"]).max()) <= 2 * LP_TOL
        ok = decided(ref["scores"], 4 * LP_TOL)
        assert ok[:20].sum() >= 10, "input condition: image %d: the head of the list is decided" % i
        n_compared += int(ok.sum())
        assert np.array_equal(p["triples"][ok], ref["triples"][ok]), "image %d" % i
        assert same_sets_in_undecided_stretches(p["triples"], ref["triples"], ok), "image %d: an undecided stretch differs" % i
        clear = ok & (ref["gap2"] > 2 * LP_TOL)
        assert np.array_equal(p["first_sample"][clear], ref["best_sample"][clear]) and np.array_equal(p["counts"][ok], ref["counts"][ok])
        assert float(np.abs(p["best_logp"] - ref["best_logp"])[ok].max()) <= 2 * LP_TOL
        # attention: the sample that gives the triple its highest probability
        assert p["attention"].shape == (nd, 3, 4, 4) and p["attention"].dtype == np.float32
        assert np.array_equal(p["attention"].reshape(nd, 3, 16), al[p["first_sample"].astype(np.int64) * NB + j])
        assert float(np.abs(p["attention"].reshape(nd, 3, 16).sum(axis=-1) - 1.0).max()) <= 1e-5
    assert n_compared >= 0.8 * sum(p["n_distinct"] for p in preds), "input condition: most positions decided"
    # top_k keeps the head of the same list
    for p, q in zip(preds, gan.predict(items=imgs, decode="kbest", top_k=3)):
        assert q["n_distinct"] == p["n_distinct"] and np.array_equal(q["triples"], p["triples"][:3]) and "attention" not in q
        assert np.array_equal(bits(q["scores"]), bits(p["scores"][:3])) and len(q["graph"]["edges"]) == 3
    # the default path: same records as before, whether or not the argument is given
    for a, b, c in zip(before, gan.predict(items=imgs), gan.predict(items=imgs, decode="samples")):
        assert list(a) == list(b) == list(c) == ["image", "n_distinct", "ordering", "triples", "scores", "first_rank", "first_sample",
                                                 "counts", "words", "graph"]
        for name in a:
            same = (lambda u, v: np.array_equal(bits(u), bits(v))) if isinstance(a[name], np.ndarray) else (lambda u, v: u == v)
            assert same(a[name], b[name]) and same(a[name], c[name]), name
    with pytest.raises(ValueError, match="descending"):
        gan.predict(items=imgs, decode="kbest", descending=True)
    with pytest.raises(ValueError, match="top_k"):
        gan.predict(items=imgs, decode="kbest", top_k=NS * WIDTH + 1)


def test_evaluate_kbest(tmp_path):
    """Ground truth per image = the K-best record's 1st triple, its 60th, and a triple [t, t, t] that the image's whole list does not
    hold: positions 0, 59 and absent.  t is the largest such token: the untrained generator favours token V - 1 = 49, so
    [49, 49, 49] itself stands 5th in these lists and cannot be the absent triple."""
    gan = _untrained_gan(tmp_path)
    imgs = _images()
    preds = gan.predict(items=imgs, decode="kbest")
    items = []
    for im, p in zip(imgs, preds):
        held = set(map(tuple, p["triples"].tolist()))
        absent = next([t, t, t] for t in range(V - 1, -1, -1) if (t, t, t) not in held)
        assert p["n_distinct"] == len(held) >= 100, "input condition"
        items.append((im, [p["triples"][0].tolist(), p["triples"][59].tolist(), absent]))
    res, calls = _count_trunk_forwards(gan, lambda: gan.evaluate(items=items, decode="kbest", return_details=True))
    assert calls == {"G": 2, "D": 0}, calls
    assert res["decode"] == "kbest" and res["ordering"] == kbest.ORDERING and res["samples_per_image"] == NS and res["ks"] == [20, 50, 100]
    acc = RecallAccumulator((20, 50, 100), V)
    for d, p, (_, real) in zip(res["details"], preds, items):
        assert d["pos"] == [0, 59, -1] and d["n_gt"] == 3 and d["n_distinct"] == p["n_distinct"]
        acc.add(np.array(d["pos"]), real, None)
    assert res["R@20"] == pytest.approx(1.0 / 3.0, abs=1e-12) and res["R@50"] == res["R@20"]
    assert res["R@100"] == pytest.approx(2.0 / 3.0, abs=1e-12)
    want = acc.result(gan.reverse_vocab)
    assert {k: res[k] for k in want} == want
    assert res["mean_n_distinct"] == float(np.mean([p["n_distinct"] for p in preds])) and res["images"] == N_IMG
    assert "decode" not in gan.evaluate(items=items)
    with pytest.raises(ValueError, match="descending"):
        gan.evaluate(items=items, decode="kbest", descending=True)


def test_decode_kbest_cli(tmp_path):
    """train.py --decode kbest in fresh child processes: --predict_dir and --metrics_out write what predict(decode="kbest",
    with_attention=True) and evaluate(decode="kbest") give in-process on the loaded checkpoint."""
    script = os.path.join(ROOT, "train.py")
    common = ["--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1", "--checkpoints_dir", str(tmp_path / "ck"),
              "--summaries_dir", str(tmp_path / "logs")]
    run = lambda extra: subprocess.run([sys.executable, script] + common + extra, cwd=str(tmp_path), capture_output=True, text=True,
                                       timeout=600)
    r = run(["--max_iterations", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "out"
    r = run(["--predict_dir", str(out), "--decode", "kbest", "--max_test_images", "2"])
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = tmp_path / "m.json"
    r = run(["--metrics_out", str(metrics), "--decode", "kbest", "--max_test_images", "2"])
    assert r.returncode == 0, r.stderr[-3000:]
    r = run(["--predict_dir", str(tmp_path / "bad"), "--decode", "kbest", "--predict_descending"])
    assert r.returncode == 2 and "--predict_descending" in r.stderr and not os.path.exists(str(tmp_path / "bad"))
    gan = _gan(tmp_path, 8, 64, 50)
    assert gan.load_checkpoint()
    preds = gan.predict(max_images=2, decode="kbest", with_attention=True)
    index = json.load(open(str(out / "index.json")))
    assert sorted(index) == ["0", "1", "decode"] and index["decode"] == "kbest"
    for i, p in enumerate(preds):
        e = index[str(i)]
        assert e["file"] == "%06d.npz" % i and e["n_distinct"] == p["n_distinct"] >= 128
        assert e["graph"] == json.loads(json.dumps(p["graph"]))
        z = np.load(str(out / e["file"]))
        assert sorted(z.files) == sorted(["triples", "words", "scores", "first_sample", "best_logp", "counts", "n_distinct", "attention"])
        assert int(z["n_distinct"]) == p["n_distinct"] and z["words"].tolist() == p["words"]
        for name in ("triples", "scores", "first_sample", "best_logp", "counts", "attention"):
            assert z[name].dtype == p[name].dtype and np.array_equal(bits(z[name]), bits(p[name])), name
    written = json.load(open(str(metrics)))
    want = gan.evaluate(max_images=2, decode="kbest")
    assert written == json.loads(json.dumps(want)) and written["decode"] == "kbest" and written["images"] == 2
