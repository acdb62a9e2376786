"""-m gpu: predicate classification - the kernels of csrc/predcls.hip (HipKernels.pair_predicate_logp, predcls_pair_topk,
predcls_merge) against the fp64 reference of sgg_amd/predcls.py, against triple_logp (bit for bit) and query_logp, and
SceneGraphGAN.predcls end to end.

pair_predicate_logp's tiles (csrc/predcls.hip): a workgroup is 256 threads = 256 predicate columns (PCLS_T) by 16 pairs (PCLS_TP),
and walks the draws 64 at a time (PCLS_DK); grid (ceil(V / 256), ceil(P / 16), nb).  Per thread 2 x 16 accumulators (123 VGPRs, no
spill: four workgroups per CU); LDS 8.6 KB per workgroup (64 x 16 x (a_0, a_2) + 64 lse + the tile's tokens), far below the 160 KB
of a CU, so the registers bound the occupancy.  PPL_CASES crosses each boundary once: N = 65 (two draw chunks, the second of one
draw), P = 17 (two pair tiles, the second of one pair), V = 257 (two column tiles, the second of one column), V = 70 000 (274 column
tiles), and the smallest shape (1, 1, 1, 1).  predcls_pair_topk runs 256 threads below V = 1024 and 1024 from there; predcls_merge
256 threads below 1024 candidates and 1024 from there."""
import json

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from sgg_amd import metrics as MT
from sgg_amd import predcls as P
from sgg_amd import retrieve as R
from tests import predcls_ref as PR
from tests import retrieve_ref as RR

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
SENT = 777.25


def u32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- pair_predicate_logp ---------------------------------------------------------------------------------------------------------
#            N, nb, V,     P,  logit scale, ld - 3 V, ldj - V, special (counts below P, a pair with token V and one with -1; ties)
PPL_CASES = [(1, 1, 1, 1, 4.0, 0, 0, ""), (3, 2, 7, 3, 4.0, 2, 3, "ties"), (65, 2, 1000, 17, 4.0, 0, 0, ""),
             (5, 3, 257, 65, 4.0, 5, 1, "counts"), (2, 1, 70000, 2, 4.0, 0, 0, ""), (4, 2, 300, 20, 80.0, 3, 2, "")]
PPL_IDS = ["N%d-nb%d-V%d-P%d" % c[:4] for c in PPL_CASES]
_ppl = {}


def ppl_case(hip, case):
    """Once per case: logits (4 N(0, 1), or uniform in +-80), random pairs, the kernel's outputs in sentinel-filled buffers, the
    reference on the device's own lse.  "ties": slot 2 is a copy of slot 0, tokens 0 and 1 are equal in slots 0 and 2 (so the pairs
    (0, 1) and (1, 0) - pairs 0 and 1 - have bit-equal rows) and predicate columns 2 and 5 are equal in every draw."""
    if case not in _ppl:
        N, nb, V, Pn, scale, extra, extraj, special = case
        g = np.random.RandomState(1200 + N + V + Pn)
        x = (scale * (g.standard_normal((N, nb, 3, V)) if scale < 50 else g.uniform(-1, 1, (N, nb, 3, V)))).astype(np.float32)
        pairs = np.stack([np.stack(divmod(g.choice(V * V, Pn, replace=False) if V <= 1000 else g.randint(0, V * V, Pn), V), axis=1)
                          for _ in range(nb)]).astype(np.int32)                    # distinct pairs per image
        count = np.full((nb,), Pn, dtype=np.int32)
        if special == "ties":
            x[:, :, 0, 1] = x[:, :, 0, 0]
            x[:, :, 2, :] = x[:, :, 0, :]
            x[:, :, 1, 5] = x[:, :, 1, 2]
            pairs[:, 0], pairs[:, 1], pairs[:, 2] = (0, 1), (1, 0), (3, 4)
        if special == "counts":
            count[:] = (Pn, 40, 0)
            pairs[0, 7], pairs[0, 20], pairs[1, 39], pairs[1, 50] = (V, 3), (4, -1), (0, V - 1), (V + 5, -7)
        for j in range(nb):
            assert len({tuple(x) for x in pairs[j].tolist()}) == Pn, "the pairs of an image must be distinct"
        buf = torch.full((N * nb, 3 * V + extra), float("nan"), device="cuda")
        buf[:, :3 * V] = torch.from_numpy(x.reshape(N * nb, 3 * V)).cuda()
        xd = buf[:, :3 * V].unflatten(1, (3, V)).unflatten(0, (N, nb))              # rows ld = 3 V + extra apart
        lse = torch.empty((N, nb, 3), device="cuda")
        hip.softmax_xent(torch.from_numpy(x).cuda(), None, lse=lse.view(-1))
        jbuf = torch.full((nb * Pn, V + extraj), SENT, device="cuda")
        joint = jbuf[:, :V].unflatten(0, (nb, Pn))                                   # rows ldj = V + extraj apart
        pd, cd = torch.from_numpy(pairs).cuda(), torch.from_numpy(count).cuda()
        out = {"marg": torch.full((nb, Pn), SENT, device="cuda"), "status": torch.full((nb, Pn), -99, dtype=I32, device="cuda")}
        res = hip.pair_predicate_logp(xd, lse, pd, cd, joint=joint, out=out)
        torch.cuda.synchronize()
        ref = P.pair_predicate_reference(x, lse.cpu().numpy(), pairs, count)
        _ppl[case] = dict(x=x, xd=xd, lse=lse, pairs=pairs, count=count, pd=pd, cd=cd, jbuf=jbuf, joint=joint, res=res, ref=ref,
                          h_joint=joint.cpu().numpy(), h_marg=res["marg"].cpu().numpy(), h_status=res["status"].cpu().numpy())
    return _ppl[case]


@pytest.mark.parametrize("case", PPL_CASES, ids=PPL_IDS)
def test_pair_predicate_logp_matches_fp64_reference(hip, case):
    N, nb, V, Pn, scale, extra, extraj, special = case
    d = ppl_case(hip, case)
    assert N * nb == 1 or d["xd"].reshape(N * nb, 3, V).stride(0) == 3 * V + extra
    assert nb * Pn == 1 or d["joint"].reshape(nb * Pn, V).stride(0) == V + extraj
    assert (u32(d["jbuf"][:, V:]) == u32(np.float32(SENT))).all(), "written outside the V columns of a row"
    ref, jt, mg, st = d["ref"], d["h_joint"], d["h_marg"], d["h_status"]
    assert np.array_equal(st, ref["status"])
    ok = st == 0
    if special == "counts":
        assert (st[2] == -3).all() and (st[1, 40:] == -3).all() and st[0, 7] == st[0, 20] == -4 and st[1, 39] == 0 and st[1, 50] == -3
    else:
        assert ok.all()
    assert np.isnan(jt[~ok]).all() and np.isnan(mg[~ok]).all(), "a pair that is not valid holds NaN"
    assert np.isfinite(jt[ok]).all() and np.isfinite(mg[ok]).all()
    err_j, err_m = float(np.abs(jt[ok] - ref["joint"][ok]).max()), float(np.abs(mg[ok] - ref["marg"][ok]).max())
    cond = jt[ok].astype(np.float64) - mg[ok].astype(np.float64)[:, None]        # (exact: the fp32 subtraction is checked in the merge)
    err_c = float(np.abs(PR.lse64((jt[ok] - mg[ok][:, None]).astype(np.float32))).max())
    assert np.abs(cond - (jt[ok] - mg[ok][:, None])).max() <= 2.0 ** -17, "cond in fp32: one rounding of a value below 256"
    print("pair_predicate_logp N %d nb %d V %d P %d scale %g: max |joint - ref| %.3e  |marg - ref| %.3e  |logsumexp_v cond| %.3e "
          "(max |joint| %.1f)" % (N, nb, V, Pn, scale, err_j, err_m, err_c, np.abs(ref["joint"][ok]).max()))
    assert max(err_j, err_m, err_c) <= PR.PCLS_TOL
    if scale < 50:
        assert max(err_j, err_m, err_c) <= PR.PCLS_SMALL_TOL, "logits of 4 N(0, 1): the bound measured over those cases"
    # a second call gives equal bits
    jb2 = torch.full_like(d["jbuf"], SENT)
    again = hip.pair_predicate_logp(d["xd"], d["lse"], d["pd"], d["cd"], joint=jb2[:, :V].unflatten(0, (nb, Pn)))
    assert np.array_equal(u32(jb2), u32(d["jbuf"])) and np.array_equal(u32(again["marg"]), u32(d["res"]["marg"]))
    assert np.array_equal(again["status"].cpu().numpy(), st)


@pytest.mark.parametrize("case", PPL_CASES, ids=PPL_IDS)
def test_joint_is_bit_equal_to_triple_logp(hip, case):
    """Every (s, v, o) of every valid pair where an image has at most 4096 of them, else a sample of 4096 per image."""
    N, nb, V, Pn, scale, extra, extraj, special = case
    d = ppl_case(hip, case)
    g = np.random.RandomState(7)
    M = min(4096, Pn * V)
    gt, where = np.zeros((nb, M, 3), dtype=np.int64), np.zeros((nb, M, 2), dtype=np.int64)
    for j in range(nb):
        flat = np.arange(Pn * V) if Pn * V <= 4096 else np.sort(g.choice(Pn * V, 4096, replace=False))
        where[j] = np.stack([flat // V, flat % V], axis=1)
        gt[j] = np.stack([d["pairs"][j, where[j, :, 0], 0], where[j, :, 1], d["pairs"][j, where[j, :, 0], 1]], axis=1)
    res = hip.triple_logp(d["xd"], d["lse"], torch.from_numpy(gt).cuda(), torch.full((nb,), M, dtype=I32, device="cuda"))
    mix, st = res["mix"].cpu().numpy(), res["status"].cpu().numpy()
    n = 0
    for j in range(nb):
        ok = d["h_status"][j, where[j, :, 0]] == 0
        assert (st[j][ok] == 0).all()
        got = d["h_joint"][j, where[j, :, 0], where[j, :, 1]]
        assert np.array_equal(u32(got[ok]), u32(mix[j][ok])), "image %d: joint differs from triple_logp's mix" % j
        n += int(ok.sum())
    assert n >= 1
    print("joint == triple_logp mix, bit for bit, on %d triples" % n)


@pytest.mark.parametrize("case", PPL_CASES, ids=PPL_IDS)
def test_marg_agrees_with_query_logp(hip, case):
    N, nb, V, Pn, scale, extra, extraj, special = case
    d = ppl_case(hip, case)
    ok = d["h_status"] == 0
    uniq = sorted({(int(s), int(o)) for s, o in d["pairs"][ok].tolist()})
    ids = np.array([[s, -1, o] for s, o in uniq], dtype=np.int64)
    c = R.compile_queries(ids.tolist(), {i: i for i in range(V)})
    scores = torch.empty((len(uniq), nb), device="cuda")
    hip.query_logp(d["xd"], d["lse"], torch.from_numpy(c["tok"]).cuda(), c["ucount"], torch.from_numpy(c["qidx"]).cuda(), scores)
    q = scores.cpu().numpy()
    row = {so: i for i, so in enumerate(uniq)}
    want = np.array([[q[row[(int(s), int(o))], j] if ok[j, p] else np.nan for p, (s, o) in enumerate(d["pairs"][j])] for j in range(nb)],
                    dtype=np.float32)
    err = float(np.abs(d["h_marg"][ok] - want[ok]).max())
    print("marg vs query_logp (s, ?, o) N %d nb %d V %d P %d: max |d| %.3e" % (N, nb, V, Pn, err))
    assert err <= RR.QLP_VS_TLP_TOL
    if N == 1:
        assert np.array_equal(u32(d["h_marg"][ok]), u32(want[ok])), "one draw: no sum to order, the same bits"


def test_pair_predicate_logp_rejects_bad_arguments(hip):
    d = ppl_case(hip, PPL_CASES[0])
    lib = hip.lib
    j, m, s = torch.zeros((1, 4), device="cuda"), torch.zeros((1,), device="cuda"), torch.zeros((1,), dtype=I32, device="cuda")
    a = [d["xd"].data_ptr(), 3, d["lse"].data_ptr(), 1, 1, 1, d["pd"].data_ptr(), d["cd"].data_ptr(), 1, j.data_ptr(), 4, m.data_ptr(),
         s.data_ptr(), None]
    assert lib.sgg_pair_predicate_logp(*a) == 0
    for pos, val, word in ((3, 4097, b"4096"), (8, 4097, b"4096"), (8, 0, b"4096"), (1, 2, b"ld"), (10, 0, b"ldj"), (5, (1 << 21) + 1, b"2^21"),
                           (0, None, b"null"), (12, None, b"null")):
        b = list(a)
        b[pos] = val
        assert lib.sgg_pair_predicate_logp(*b) == -1 and word in lib.sgg_last_error(), (pos, lib.sgg_last_error())
    torch.cuda.synchronize()
    # a count outside [0, P] is clamped on the device
    big = hip.pair_predicate_logp(d["xd"], d["lse"], d["pd"], torch.tensor([9], dtype=I32, device="cuda"))
    neg = hip.pair_predicate_logp(d["xd"], d["lse"], d["pd"], torch.tensor([-2], dtype=I32, device="cuda"))
    assert big["status"].tolist() == [[0]] and neg["status"].tolist() == [[-3]] and torch.isnan(neg["joint"]).all()


# ---- predcls_pair_topk and predcls_merge --------------------------------------------------------------------------------------------
def _gt_for(d, V, Pn, nb):
    """True triples aimed at the order's ends: per image (pair 0: its best token, its worst token, its best again), a token outside the
    vocabulary, a triple without a candidate pair (-1), one whose pair index is P (outside), and the last pair's second token."""
    gp = np.zeros((nb, 7), dtype=np.int32)
    gv = np.zeros((nb, 7), dtype=np.int32)
    for j in range(nb):
        o0 = P.token_order(d["h_joint"][j, 0]) if d["h_status"][j, 0] == 0 else np.zeros(V, dtype=np.int64)
        ol = P.token_order(d["h_joint"][j, Pn - 1]) if d["h_status"][j, Pn - 1] == 0 else np.zeros(V, dtype=np.int64)
        gp[j] = (0, 0, 0, 0, -1, Pn, Pn - 1)
        gv[j] = (o0[0], o0[V - 1], o0[0], V, 0, 0, ol[min(1, V - 1)])
    return gp, gv


@pytest.mark.parametrize("case", PPL_CASES, ids=PPL_IDS)
def test_pair_topk_and_merge_are_exact(hip, case):
    """Both against the numpy reference applied to the kernel's own joint / marg bits: rounding cannot flip an order."""
    N, nb, V, Pn, scale, extra, extraj, special = case
    d = ppl_case(hip, case)
    gp, gv = _gt_for(d, V, Pn, nb)
    gpd, gvd = torch.from_numpy(gp).cuda(), torch.from_numpy(gv).cuda()
    pairs64 = d["pairs"].astype(np.int64)
    for Kc in (1, 5, 128):
        top = hip.predcls_pair_topk(d["joint"], d["res"]["status"], Kc, gpd, gvd)
        want = P.pair_topk_reference(d["h_joint"], d["h_status"], Kc, gp, gv)
        tt, ts, gr = top["top_tok"].cpu().numpy(), top["top_score"].cpu().numpy(), top["gt_rank"].cpu().numpy()
        assert np.array_equal(tt, want["top_tok"]), "Kc %d: pairs %s differ" % (Kc, np.argwhere((tt != want["top_tok"]).any(axis=2))[:5].tolist())
        assert np.array_equal(u32(ts), u32(want["top_score"])), "the scores are the rows' own bits, NaN behind them"
        assert np.array_equal(gr, want["gt_rank"])
        n = min(Kc, V)
        assert (tt[:, :, n:] == -1).all() and (tt[d["h_status"] != 0] == -1).all() and (tt[d["h_status"] == 0][:, :n] >= 0).all()
        for j in range(nb):
            if d["h_status"][j, 0] == 0:
                assert gr[j, :6].tolist() == [1, V, 1, 0, 0, 0], "rank 1, rank V, repeated, a token outside, no pair, a pair outside"
                assert gr[j, 6] == (min(2, V) if d["h_status"][j, Pn - 1] == 0 else 0)
            else:
                assert (gr[j, :4] == 0).all()
        if special == "ties":
            assert np.array_equal(u32(d["h_joint"][:, 0]), u32(d["h_joint"][:, 1])), "pairs (0, 1) and (1, 0) must tie bit for bit"
            assert np.array_equal(u32(d["h_joint"][:, :, 2]), u32(d["h_joint"][:, :, 5])), "columns 2 and 5 must tie bit for bit"
            if Kc == 128:
                for j in range(nb):
                    for p in range(Pn):
                        row = tt[j, p].tolist()
                        assert row.index(5) == row.index(2) + 1, "equal scores: the smaller token first"
        again = hip.predcls_pair_topk(d["joint"], d["res"]["status"], Kc, gpd, gvd)
        for name in top:
            assert np.array_equal(u32(again[name]), u32(top[name])), name
        for per_pair in sorted({1, Kc}):
            for cond in (False, True):
                n_cand = int((tt[:, :, :per_pair] >= 0).sum(axis=(1, 2)).max())
                for K in sorted({1, min(1024, n_cand + 3), 1024 if (Kc == 128 and cond) else 7}):
                    res = hip.predcls_merge(d["pd"], top["top_tok"], top["top_score"], d["res"]["marg"], K, per_pair=per_pair, conditional=cond)
                    ref = P.merge_reference(d["pairs"], tt, ts, d["h_marg"], K, per_pair, cond)
                    tag = "Kc %d per_pair %d conditional %s K %d" % (Kc, per_pair, cond, K)
                    tr, sc = res["triples"].cpu().numpy(), res["scores"].cpu().numpy()
                    assert np.array_equal(res["n_distinct"].cpu().numpy(), ref["n_distinct"]), tag
                    assert np.array_equal(res["src"].cpu().numpy(), ref["src"]), tag
                    assert np.array_equal(tr, ref["triples"]), tag
                    assert np.array_equal(u32(sc), u32(ref["scores"])), tag
                    for j in range(nb):
                        u = min(K, int(ref["n_distinct"][j]))
                        assert (tr[j, u:] == -1).all() and np.isnan(sc[j, u:]).all() and (tr[j, :u] >= 0).all(), tag
                        if per_pair == 1:
                            assert len({tuple(x) for x in tr[j, :u][:, [0, 2]].tolist()}) == u, tag + ": a pair is listed twice"
                    if special == "ties" and K > 2:
                        # pairs 0 and 1 tie bit for bit (under either score): equal scores are listed by candidate index
                        # pair * per_pair + rank ascending, and a slot of pair 0 stands before the same slot of pair 1
                        src, ties = res["src"].cpu().numpy(), 0
                        for j in range(nb):
                            u, s = min(K, int(ref["n_distinct"][j])), src[j].tolist()
                            for a in range(u - 1):
                                if sc[j, a] == sc[j, a + 1]:
                                    ties += 1
                                    assert s[a] < s[a + 1], tag + ": equal scores out of index order"
                            for r in range(per_pair):
                                if r in s and per_pair + r in s:
                                    assert s.index(r) < s.index(per_pair + r) and sc[j, s.index(r)] == sc[j, s.index(per_pair + r)], tag
                        assert ties >= 1, tag + ": the case must hold equal scores"
                    # the list goes through match_triples as rank_triples' does
                    gt = np.zeros((nb, 4, 3), dtype=np.int64)
                    for j in range(nb):
                        u = min(K, int(ref["n_distinct"][j]))
                        gt[j] = [tr[j, u - 1] if u else (0, 0, 0), tr[j, 0] if u else (0, 0, 0), (pairs64[j, 0, 0], V, pairs64[j, 0, 1]),
                                 tr[j, u - 1] if u else (0, 0, 0)]
                    m = hip.match_triples(res["triples"], res["n_distinct"], torch.from_numpy(gt).cuda(),
                                          torch.full((nb,), 4, dtype=I32, device="cuda"), vocab=V)
                    for j in range(nb):
                        u = min(K, int(ref["n_distinct"][j]))
                        pos, n_gt = MT.match_reference(tr[j, :u], gt[j].tolist(), V)
                        assert np.array_equal(m["pos"][j].cpu().numpy(), pos) and int(m["n_gt"][j]) == n_gt, tag
                    again = hip.predcls_merge(d["pd"], top["top_tok"], top["top_score"], d["res"]["marg"], K, per_pair=per_pair, conditional=cond)
                    for name in res:
                        assert np.array_equal(u32(again[name]), u32(res[name])), name


def test_selection_kernels_reject_bad_arguments(hip):
    d = ppl_case(hip, PPL_CASES[1])
    N, nb, V, Pn = PPL_CASES[1][:4]
    lib = hip.lib
    gp = torch.zeros((nb, 1), dtype=I32, device="cuda")
    top = hip.predcls_pair_topk(d["joint"], d["res"]["status"], 5, gp, gp)
    ldj = V + PPL_CASES[1][6]
    a = [d["joint"].data_ptr(), ldj, d["res"]["status"].data_ptr(), nb, Pn, V, 5, gp.data_ptr(), gp.data_ptr(), 1, top["top_tok"].data_ptr(),
         top["top_score"].data_ptr(), top["gt_rank"].data_ptr(), None]
    assert lib.sgg_predcls_pair_topk(*a) == 0
    for pos, val, word in ((6, 129, b"Kc"), (6, 0, b"Kc"), (9, 4097, b"4096"), (1, V - 1, b"ldj"), (4, 4097, b"4096"), (2, None, b"null")):
        b = list(a)
        b[pos] = val
        assert lib.sgg_predcls_pair_topk(*b) == -1 and word in lib.sgg_last_error(), (pos, lib.sgg_last_error())
    res = hip.predcls_merge(d["pd"], top["top_tok"], top["top_score"], d["res"]["marg"], 4)
    a = [d["pd"].data_ptr(), top["top_tok"].data_ptr(), top["top_score"].data_ptr(), d["res"]["marg"].data_ptr(), nb, Pn, 5, 1, 0, 4,
         res["triples"].data_ptr(), res["scores"].data_ptr(), res["src"].data_ptr(), res["n_distinct"].data_ptr(), None]
    assert lib.sgg_predcls_merge(*a) == 0
    for pos, val, word in ((7, 6, b"per_pair"), (7, 0, b"per_pair"), (9, 1025, b"1024"), (9, 0, b"1024"), (8, 2, b"conditional"),
                           (5, (1 << 21) + 1, b"2^21"), (3, None, b"null")):
        b = list(a)
        b[pos] = val
        assert lib.sgg_predcls_merge(*b) == -1 and word in lib.sgg_last_error(), (pos, lib.sgg_last_error())
    torch.cuda.synchronize()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
_e2e = {}


def _end_to_end(tmp_path_factory):
    """The untrained model of tests/test_eval_batched_gpu.py, batch_size 8: TEST_BATCH_SIZE 4; 10 samples per image (not a multiple of
    it), five images = one full and one padded image batch; a logits budget of 24 000 bytes keeps nb = 4 (6000 bytes per image) and
    leaves 6000 / (4 x 50 x 4) = 7 pairs per launch: the 13 pairs of the third image (four entities and a true self pair) take two
    chunks of 7."""
    if _e2e:
        return _e2e
    from sgg_amd.api import kernels_for
    from tests.test_eval_batched_gpu import _gan
    from tests.test_xent_gpu import _arenas
    tmp_path = tmp_path_factory.mktemp("predcls")
    S, Vv = 64, 50
    gan = _gan(tmp_path, 8, S, Vv)
    g = torch.Generator().manual_seed(79)
    imgs = [torch.randn((S, S, 3), generator=g) for _ in range(5)]
    gts = [[[1, 2, 3], [4, 5, 6], [1, 9, 6]], [[0, Vv - 1, 0]], [[7, 7, 7], [1, 2, 9], [8, 1, 1], [1, 2, 9]], [[5, 5, 5], [1, 2, 3], [3, 0, 5]],
           [[9, 8, 7], [6, 5, 4]]]
    items = list(zip(imgs, gts))
    before_p, before_e = gan.predict(items=items, n_samples=10), gan.evaluate(items=items, n_samples=10, ks=(1, 3))
    arenas = _arenas(gan.step)
    K = kernels_for(gan.device)
    dumped, real = [], K.pair_predicate_logp

    def ppl(logits, lse, pairs, pair_count, joint=None, out=None):
        dumped.append((logits.cpu().numpy().copy(), lse.cpu().numpy().copy(), pairs.cpu().numpy().copy(), pair_count.cpu().numpy().copy()))
        return real(logits, lse, pairs, pair_count, joint=joint, out=out)
    K.pair_predicate_logp = ppl
    try:
        runs = {}
        for pairs, score in (("all", "joint"), ("all", "conditional"), ("gt", "conditional")):
            del dumped[:]
            out = str(tmp_path / ("%s_%s.json" % (pairs, score)))
            res = gan.predcls(items=items, ks=(1, 3, 20), n_samples=10, pairs=pairs, score=score, return_details=True, out_path=out,
                              logits_budget_bytes=24000)
            assert json.load(open(out)) == res
            runs[(pairs, score)] = (res, list(dumped))
    finally:
        del K.pair_predicate_logp
    after = _arenas(gan.step)
    _e2e.update(gan=gan, items=items, gts=gts, runs=runs, arenas=(arenas, after), before=(before_p, before_e), V=Vv)
    return _e2e


def _same(a, b):
    """Two results of predict(): equal keys, equal bits of every array, equal everything else."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, torch.Tensor)):
        a, b = np.asarray(torch.as_tensor(a).cpu()), np.asarray(torch.as_tensor(b).cpu())
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def _reference_image(dumps, j_global, nb, pairs_of_image):
    """fp64 joint / marg of one image over ALL its pairs, from the recorded launches: two image batches, chunk after chunk."""
    b, j = divmod(j_global, nb)
    n_chunks = len(dumps) // 2
    joint, marg, seen = [], [], 0
    for c in range(n_chunks):
        x, lse, pairs, count = dumps[b * n_chunks + c]
        n = int(count[j])
        r = P.pair_predicate_reference(x[:, j:j + 1], lse[:, j:j + 1], pairs[j:j + 1], count[j:j + 1])
        joint.append(r["joint"][0, :n])
        marg.append(r["marg"][0, :n])
        assert (r["status"][0, :n] == 0).all() and np.array_equal(pairs[j, :n], pairs_of_image[seen:seen + n])
        seen += n
    assert seen == len(pairs_of_image)
    return np.concatenate(joint), np.concatenate(marg)


@pytest.mark.parametrize("run", [("all", "joint"), ("all", "conditional"), ("gt", "conditional")], ids=lambda r: "%s-%s" % r)
def test_predcls_end_to_end(tmp_path_factory, run):
    e = _end_to_end(tmp_path_factory)
    res, dumps = e["runs"][run]
    mode_pairs, score = run
    V, gts, nb, ks = e["V"], e["gts"], 4, (1, 3, 20)
    assert (res["ks"], res["pairs"], res["score"], res["samples_per_image"], res["predicates_per_pair"]) == ([1, 3, 20], mode_pairs, score, 10, 20)
    assert res["n_images_truncated"] == 0 and res["generator_weights"] == "live" and "definition" in res
    cands = [P.candidate_pairs(gt, mode_pairs)[0] for gt in gts]
    assert res["mean_pairs_per_image"] == np.mean([len(c) for c in cands])
    if mode_pairs == "all":
        assert max(len(c) for c in cands) == 13 and len(dumps) == 4, "two image batches x two pair chunks"
        assert dumps[0][2].shape == (4, 7, 2) and dumps[0][0].shape == (10, 4, 3, V)
    accs = {m: MT.RecallAccumulator(ks, V) for m in ("graph_constraint", "no_graph_constraint")}
    pacc = P.PredicateAccumulator(V)
    worst, decided, total = 0.0, 0, 0
    for i, d in enumerate(res["details"]):
        gt, pairs = gts[i], cands[i]
        assert d["image"] == str(i) and d["n_pairs"] == len(pairs)
        joint, marg = _reference_image(dumps, i, nb, pairs)
        sc_all = joint - marg[:, None] if score == "conditional" else joint            # [pairs, V]: every candidate there is
        where = P.gt_pair_index(pairs, gt)
        # gt_rank: the reference's rank wherever the true predicate's joint is clear of every other token of its pair
        for m, t in enumerate(gt):
            row = joint[where[m]]
            gap = np.abs(np.delete(row, t[1]) - row[t[1]]).min()
            if gap > 2 * PR.PCLS_SMALL_TOL:
                assert d["gt_rank"][m] == 1 + int((row > row[t[1]]).sum()), (i, m)
        for mode, per_pair in (("graph_constraint", 1), ("no_graph_constraint", 20)):
            got = d[mode]
            top = P.pair_topk_reference(joint[None], np.zeros((1, len(pairs)), dtype=np.int32), 20, np.zeros((1, 1)), np.zeros((1, 1)))
            ref = P.merge_reference(pairs[None], top["top_tok"], top["top_score"], marg[None], 20, per_pair, score == "conditional")
            n = min(20, int(ref["n_distinct"][0]))
            assert got["n_candidates"] == ref["n_distinct"][0] == len(pairs) * per_pair and len(got["triples"]) == n
            for u, (t, s) in enumerate(zip(got["triples"], got["scores"])):
                p = int(np.nonzero((pairs[:, 0] == t[0]) & (pairs[:, 1] == t[2]))[0][0])
                worst = max(worst, abs(s - sc_all[p, t[1]]))
                # decided: no other (pair, token) of the image scores within 2 tolerances of the reference's candidate of this slot
                total += 1
                if int((np.abs(sc_all - ref["scores"][0, u]) <= 2 * PR.PCLS_SMALL_TOL).sum()) == 1:
                    decided += 1
                    assert t == ref["triples"][0, u].tolist(), (i, mode, u)
            pos, n_gt = MT.match_reference(np.asarray(got["triples"], dtype=np.int64).reshape(-1, 3), gt, V)
            assert got["pos"] == pos.tolist() and got["n_gt"] == n_gt
            accs[mode].add(got["pos"], gt)
        keep = np.asarray(d["graph_constraint"]["pos"]) >= -1
        pacc.add(np.asarray(d["gt_rank"])[keep], np.asarray(gt)[keep])
    print("predcls() %s / %s: max |score - fp64| %.3e; %d of %d list slots decided" % (mode_pairs, score, worst, decided, total))
    assert worst <= PR.PCLS_SMALL_TOL <= PR.PCLS_TOL and decided >= 0.9 * total
    for mode, acc in accs.items():
        assert res[mode] == acc.result(e["gan"].reverse_vocab), mode
    assert res["predicate_given_pair"] == pacc.result() and res["predicate_given_pair"]["n_triples"] == 12
    if run == ("gt", "conditional"):
        # one predicate per true pair, K above the number of pairs: a true triple is hit exactly where its predicate is its pair's best
        hits = n = 0
        for i, d in enumerate(res["details"]):
            keep = np.asarray(d["graph_constraint"]["pos"]) >= -1
            hit = np.asarray(d["graph_constraint"]["pos"])[keep] >= 0
            assert np.array_equal(hit, np.asarray(d["gt_rank"])[keep] == 1), i
            hits, n = hits + int(hit.sum()), n + int(keep.sum())
        assert res["predicate_given_pair"]["top1"] == hits / n
        assert abs(res["graph_constraint"]["R@20"] - np.mean([np.mean(np.asarray(d["gt_rank"])[np.asarray(d["graph_constraint"]["pos"]) >= -1] == 1)
                                                                 for d in res["details"]])) <= 1e-15


def test_predcls_leaves_the_model_alone(tmp_path_factory):
    e = _end_to_end(tmp_path_factory)
    before, after = e["arenas"]
    for name in before:
        assert torch.equal(before[name].view(torch.int32), after[name].view(torch.int32)), name + " changed"
    gan, items = e["gan"], e["items"]
    p, m = gan.predict(items=items, n_samples=10), gan.evaluate(items=items, n_samples=10, ks=(1, 3))
    assert m == e["before"][1], "evaluate() changed"
    assert _same(p, e["before"][0]), "predict() changed"


def test_predcls_validates_before_anything_is_launched(tmp_path_factory):
    e = _end_to_end(tmp_path_factory)
    gan, img = e["gan"], e["items"][0][0]
    for bad, word in (({"pairs": "some"}, "pairs"), ({"score": "critic"}, "score"), ({"ks": (0,)}, "ks"), ({"ks": (1025,)}, "ks"),
                      ({"items": [(img, [[0, 0, e["V"]]])]}, "not three tokens"), ({"items": [(img, [[0, 0, 0]] * 4097)]}, "at most")):
        kw = dict(items=e["items"], n_samples=10)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            gan.predcls(**kw)
