"""-m gpu: the generator likelihood - the kernels of csrc/xent.hip (HipKernels.softmax_xent, xent_summary, triple_logp) against the
numpy fp64 restatement of tests/xent_ref.py, the cross-check of triple_logp with K-best decoding (same documented arithmetic: equal
bits), and GanStep.pretrain_step / generator_step(mle_weight) / generator_nll against autograd on the CPU oracle.

softmax_xent has two paths (csrc/xent.hip): rows of V <= 1024 live in the registers of one wave (one row per workgroup up to
R = 1024 rows, four above), longer rows are streamed by one 1024-thread workgroup with 16-byte accesses on the aligned body of the row and 4-byte accesses in front of
and behind it; the gradient pass falls back to 4-byte accesses where the logits row and the gradient row sit differently against a
16-byte boundary.  XENT_CASES holds the issue's shapes, both sides of the wave width (64 | 65), of the resident / streaming
threshold (1024 | 1025), of one sweep of the streaming workgroup (4096 | 4097 elements of body) and of its loop with four loads in flight (3072 | 3073 16-byte words), both sides of the row count at
which a workgroup takes four rows (R = 1024 | 1025 = one above a multiple of four), and every alignment of the two rows (element shifts sx / sd, odd strides)."""
import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd.step import GanStep
from tests import xent_ref as XR
from tests.kbest_ref import LP_TOL
from tests.test_step_gpu import check_weights_after_adam, tensor_err
from tests.tolerances import GRAD_RTOL, MARGIN_FACTOR, logit_tol, loss_tol
from tests.xent_ref import XENT_GRAD_TOL, XENT_TOL

pytestmark = pytest.mark.gpu

PAD, BASE = 97, 100                # (BASE elements = 400 bytes: a 16-byte boundary; the case's shift moves the view off it)
SENT = {torch.int32: -777, torch.float32: 777.25, torch.int64: -777}
F32, I32, I64 = torch.float32, torch.int32, torch.int64
EPS32 = 2.0 ** -23


def rows_view(R, V, ld, shift, fill, dtype=F32):
    """(big, view): a [R, V] view of rows `ld` apart, `shift` elements behind a 16-byte boundary, inside a buffer filled with `fill`."""
    big = torch.full((BASE + shift + (R - 1) * ld + V + PAD,), fill, dtype=dtype, device="cuda")
    return big, big.as_strided((R, V), (ld, 1), BASE + shift)


def assert_rows_guard(big, R, V, ld, shift, what):
    """Nothing but the R x V view was written: the gaps between rows and both ends still hold the sentinel."""
    flat = big.cpu().numpy()
    mask = np.ones(flat.shape, dtype=bool)
    for r in range(R):
        mask[BASE + shift + r * ld:BASE + shift + r * ld + V] = False
    assert (flat[mask] == SENT[big.dtype]).all(), "%s: written outside its rows" % what


def vec(n, dtype):
    big = torch.full((BASE + n + PAD,), SENT[dtype], dtype=dtype, device="cuda")
    return big, big[BASE:BASE + n]


def assert_vec_guard(big, n, what):
    flat = big.cpu().numpy()
    assert (flat[:BASE] == SENT[big.dtype]).all() and (flat[BASE + n:] == SENT[big.dtype]).all(), "%s: written outside its extent" % what


def u32(t):
    return t.cpu().numpy().view(np.uint32) if t.dtype == F32 else t.cpu().numpy()


#             R, V,     ld,    ldd,   sx, sd
XENT_CASES = [(6, 11, 11, 11, 0, 0), (1, 1, 1, 1, 0, 0), (7, 1000, 1000, 1000, 0, 0), (5, 1003, 1024, 1024, 0, 0),
              (3, 70001, 70001, 70001, 0, 0),
              (9, 64, 64, 70, 1, 0), (5, 65, 67, 65, 0, 3),                     # the wave width
              (1024, 7, 7, 9, 0, 0), (1025, 7, 8, 7, 1, 0),                      # one row per workgroup | four (R = 4 * 256 + 1)
              (5, 1024, 1024, 1030, 2, 1), (6, 1025, 1025, 1025, 0, 0),          # the resident / streaming threshold (odd stride: every head)
              (6, 1025, 1028, 1032, 0, 0),                                       # streaming, both rows aligned: no peel in front
              (6, 1027, 1027, 1028, 3, 0),                                       # rows aligned differently: the 4-byte gradient pass
              (6, 5121, 5124, 5128, 1, 1), (6, 5125, 5125, 5125, 2, 2),          # body of 4096 | 4097+ elements: one sweep | two
              (2, 12291, 12292, 12292, 0, 0), (2, 12293, 12296, 12296, 0, 0)]    # 3072 | 3073 16-byte words: pass 1's four-loads-in-flight loop not entered | entered
_cases = {}


def xent_case(case):
    """(logits float32 [R, V], labels int64 [R], reference dict); once per case.  Rows: 0 labelled 0, 1 labelled V - 1, 2 skipped
    (label V; in every second case -1), 3 all logits equal, 4 a tie at the maximum with the label on its FIRST index (hit = 1), 5
    the same with the label on its second index (hit = 0); the rest random."""
    if case not in _cases:
        R, V = case[0], case[1]
        g = np.random.RandomState(7000 + R + V)
        x = (4.0 * g.standard_normal((R, V))).astype(np.float32)
        lab = g.randint(0, V, size=R).astype(np.int64)
        lab[0] = 0
        if R > 1:
            lab[1] = V - 1
        if R > 2:
            lab[2] = V if V % 2 else -1
        if R > 3:
            x[3] = 0.5
        for r, second in ((4, False), (5, True)):
            if R > r and V >= 4:
                i, j = sorted(g.choice(V, size=2, replace=False).tolist())
                x[r, i] = x[r, j] = np.float32(x[r].max() + 1.0)
                lab[r] = j if second else i
        assert float(np.abs(x).max()) <= 23.0
        _cases[case] = (x, lab, XR.softmax_xent(x, lab, scale=0.37))
    return _cases[case]


def launch(hip, case, x, lab, accumulate, d0=None):
    R, V, ld, ldd, sx, sd = case
    bx, xv = rows_view(R, V, ld, sx, float("nan"))
    xv.copy_(torch.from_numpy(x).cuda())
    bd, dv = rows_view(R, V, ldd, sd, SENT[F32])
    if d0 is not None:
        dv.copy_(torch.from_numpy(d0).cuda())
    (bn, nll), (bl, lse), (bh, hit) = vec(R, F32), vec(R, F32), vec(R, I32)
    hip.softmax_xent(xv, torch.from_numpy(lab).cuda(), scale=0.37, accumulate=accumulate, dlogits=dv, nll=nll, lse=lse, hit=hit)
    torch.cuda.synchronize()
    assert_rows_guard(bd, R, V, ldd, sd, "dlogits")
    for b, what in ((bn, "nll"), (bl, "lse"), (bh, "hit")):
        assert_vec_guard(b, R, what)
    return xv, dv, nll, lse, hit


@pytest.mark.parametrize("case", XENT_CASES, ids=["R%d-V%d-ld%d-ldd%d-sx%d-sd%d" % c for c in XENT_CASES])
def test_softmax_xent_matches_fp64_restatement(hip, case):
    R, V, ld, ldd, sx, sd = case
    x, lab, ref = xent_case(case)
    valid = ref["hit"] >= 0
    xv, dv, nll, lse, hit = launch(hip, case, x, lab, False)
    err_nll = float(np.abs(nll.cpu().numpy() - ref["nll"]).max())
    err_lse = float(np.abs(lse.cpu().numpy() - ref["lse"]).max())
    err_g = float(np.abs(dv.cpu().numpy() - ref["dlogits"]).max()) / 0.37
    print("softmax_xent R %d V %d: max |nll - ref| %.3e  |lse - ref| %.3e  |dlogits - ref| / scale %.3e" % (R, V, err_nll, err_lse, err_g))
    # exact: hit, the skip, the zero-filled gradient row of a skipped row
    assert np.array_equal(hit.cpu().numpy(), ref["hit"])
    assert (nll.cpu().numpy()[~valid] == 0.0).all() and (dv.cpu().numpy()[~valid] == 0.0).all()
    if R > 2:
        assert ref["hit"][2] == -1
    if R > 5 and V >= 4:
        assert ref["hit"][4] == 1 and ref["hit"][5] == 0, "the tie rows do not test what they say"
    assert err_nll <= XENT_TOL and err_lse <= XENT_TOL and err_g <= XENT_GRAD_TOL
    # two launches: equal bits for every output
    _, dv2, nll2, lse2, hit2 = launch(hip, case, x, lab, False)
    for a, b, what in ((dv, dv2, "dlogits"), (nll, nll2, "nll"), (lse, lse2, "lse"), (hit, hit2, "hit")):
        assert np.array_equal(u32(a.contiguous()), u32(b.contiguous())), "%s differs between two launches" % what
    # accumulate = 1: added to what is there (one fp32 addition more), a skipped row keeps its bits
    d0 = np.random.RandomState(1).standard_normal((R, V)).astype(np.float32)
    want = XR.softmax_xent(x, lab, scale=0.37, accumulate=True, dlogits=d0)["dlogits"]
    _, dva, nlla, _, _ = launch(hip, case, x, lab, True, d0)
    got = dva.cpu().numpy()
    assert (np.abs(got - want) <= XENT_GRAD_TOL * 0.37 + EPS32 * np.abs(want)).all()
    assert np.array_equal(got[~valid].view(np.uint32), d0[~valid].view(np.uint32)), "accumulate = 1 touched a skipped row"
    assert np.array_equal(u32(nlla), u32(nll))
    # lse-only mode: the same bits, nothing else needed
    bl, lse_only = vec(R, F32)
    hip.softmax_xent(xv, None, lse=lse_only)
    torch.cuda.synchronize()
    assert_vec_guard(bl, R, "lse")
    assert np.array_equal(u32(lse_only), u32(lse))
    # outputs are optional one by one: the gradient alone
    bd, donly = rows_view(R, V, ldd, sd, SENT[F32])
    hip.softmax_xent(xv, torch.from_numpy(lab).cuda(), scale=0.37, dlogits=donly)
    torch.cuda.synchronize()
    assert np.array_equal(u32(donly.contiguous()), u32(dv.contiguous()))


@pytest.mark.parametrize("V,ld,sx", [(11, 11, 0), (1000, 1001, 1), (70001, 70001, 3)])
def test_softmax_xent_row_of_plus_minus_80_does_not_overflow(hip, V, ld, sx):
    """exp(80) overflows fp32: only the stabilised sum is finite.  nll and lse are compared as |d| <= XENT_TOL * max(1, max|x|), the
    gradient against the plain XENT_GRAD_TOL."""
    R = 2
    x = np.empty((R, V), dtype=np.float32)
    x[0] = np.where(np.arange(V) % 2 == 0, 80.0, -80.0)
    x[1] = np.where(np.arange(V) % 3 == 0, -80.0, 80.0)
    lab = np.array([V - 1, 0], dtype=np.int64)
    ref = XR.softmax_xent(x, lab)
    _, dv, nll, lse, hit = launch(hip, (R, V, ld, ld, sx, sx), x, lab, False)
    got_nll, got_lse, got_d = nll.cpu().numpy(), lse.cpu().numpy(), dv.cpu().numpy()
    assert np.isfinite(got_nll).all() and np.isfinite(got_lse).all() and np.isfinite(got_d).all()
    # (launch() scales the gradient by 0.37)
    e1, e2 = float(np.abs(got_nll - ref["nll"]).max()), float(np.abs(got_lse - ref["lse"]).max())
    e3 = float(np.abs(got_d / 0.37 - ref["dlogits"]).max())
    print("+-80 rows V %d: |nll - ref| %.3e  |lse - ref| %.3e  |dlogits - ref| / scale %.3e" % (V, e1, e2, e3))
    # (the gradient is a probability in [0, 1] whatever the logits' range: its bound is not scaled)
    assert e1 <= XENT_TOL * 80.0 and e2 <= XENT_TOL * 80.0 and e3 <= XENT_GRAD_TOL
    assert np.array_equal(hit.cpu().numpy(), ref["hit"])


def test_softmax_xent_refuses_bad_arguments(hip):
    from sgg_amd.lib import SggError
    x = torch.zeros(3, 5, device="cuda")
    lab = torch.zeros(3, dtype=I64, device="cuda")
    with pytest.raises(SggError, match="lse-only"):
        hip.softmax_xent(x, None, nll=torch.zeros(3, device="cuda"))
    with pytest.raises(SggError, match="no output"):
        hip.softmax_xent(x, lab)
    with pytest.raises(SggError, match="R = 3 B"):
        hip.xent_summary(torch.zeros(4, device="cuda"), torch.zeros(4, dtype=I32, device="cuda"))


@pytest.mark.parametrize("B", [1, 2, 100, 300])
def test_xent_summary(hip, B):
    g = np.random.RandomState(B)
    nll = (5.0 * g.random_sample(3 * B)).astype(np.float32)
    hit = g.randint(-1, 2, size=3 * B).astype(np.int32)
    if B >= 2:
        hit[:3] = 1                              # one triple whose rows all hit
        hit[3:6] = (1, 0, 1)
    want = XR.xent_summary(nll, hit)
    bo, out = vec(4, F32)
    hip.xent_summary(torch.from_numpy(nll).cuda(), torch.from_numpy(hit).cuda(), out=out)
    got = out.cpu().numpy()
    assert_vec_guard(bo, 4, "out4")
    # the sum is formed in fp64 and rounded once; the shares are ratios of integers rounded once
    assert (np.abs(got - want) <= EPS32 * np.abs(want)).all(), (got, want)
    again = hip.xent_summary(torch.from_numpy(nll).cuda(), torch.from_numpy(hit).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    # nothing valid: zeros
    none = hip.xent_summary(torch.from_numpy(nll).cuda(), torch.full((3 * B,), -1, dtype=I32, device="cuda")).cpu().numpy()
    assert none.tolist() == [0.0, 0.0, 0.0, 0.0]


# ---- triple_logp ---------------------------------------------------------------------------------------------------------------
def strided_logits(x, extra):
    """x [N, nb, 3, V] on the device as a view of head rows 3 V + extra floats apart (the rest NaN)."""
    N, nb, _, V = x.shape
    buf = torch.full((N * nb, 3 * V + extra), float("nan"), device="cuda")
    buf[:, :3 * V] = torch.from_numpy(x.reshape(N * nb, 3 * V)).cuda()
    return buf[:, :3 * V].unflatten(1, (3, V)).unflatten(0, (N, nb))


def lp_outputs(nb, M):
    shapes = {"mix": ((nb, M), F32), "mean": ((nb, M), F32), "slot": ((nb, M, 3), F32), "status": ((nb, M), I32)}
    big, out = {}, {}
    for name, (shape, dt) in shapes.items():
        n = int(np.prod(shape))
        big[name], flat = vec(n, dt)
        out[name] = flat.view(shape)
    return big, out


LP_CASES = [(1, 1, 1, 11, (1,)), (3, 2, 5, 11, (5, 0)), (4, 3, 7, 1000, (7, 3, 9))]      # (9: clamped to M on the device)


@pytest.mark.parametrize("case", LP_CASES, ids=["N%d-nb%d-M%d-V%d" % c[:4] for c in LP_CASES])
def test_triple_logp_matches_fp64_restatement(hip, case):
    N, nb, M, V, counts = case
    g = np.random.RandomState(100 + N + V)
    x = (4.0 * g.standard_normal((N, nb, 3, V))).astype(np.float32)
    gt = g.randint(0, V, size=(nb, M, 3)).astype(np.int64)
    for j in range(nb):                           # padding rows full of garbage, out-of-range tokens among it
        gt[j, min(max(counts[j], 0), M):] = g.randint(-2 ** 40, 2 ** 40, size=(M - min(max(counts[j], 0), M), 3))
    if M >= 5:
        gt[0, 1] = gt[0, 0]                       # a duplicated row: each is scored
        gt[0, 2, 1] = V                           # valid rows with a token outside [0, V)
        gt[0, 3, 0] = -1
    cnt = np.array(counts, dtype=np.int32)
    xd = strided_logits(x, 8)
    assert N * nb == 1 or xd.reshape(N * nb, 3, V).stride(0) == 3 * V + 8      # ld > 3 V
    lse = torch.empty((N, nb, 3), device="cuda")
    for k in range(N):                            # (the slot rows of a strided buffer are not ONE stride apart: one call per sample)
        for j in range(nb):
            hip.softmax_xent(xd[k, j], None, lse=lse[k, j])
    big, out = lp_outputs(nb, M)
    res = hip.triple_logp(xd, lse, torch.from_numpy(gt).cuda(), torch.from_numpy(cnt).cuda(), out=out)
    torch.cuda.synchronize()
    for name, b in big.items():
        assert_vec_guard(b, out[name].numel(), name)
    ref = XR.triple_logp(x, lse.cpu().numpy(), gt, cnt)
    st = res["status"].cpu().numpy()
    assert np.array_equal(st, ref["status"])
    ok = st == 0
    if M >= 5:
        assert st[0, 2] == -4 and st[0, 3] == -4 and st[0, 1] == 0 and (st[1, counts[1]:] == -3).all()
    for name in ("mix", "mean", "slot"):
        got = res[name].cpu().numpy()
        assert np.isnan(got[~ok]).all(), "%s: a row that is not valid must hold NaN" % name
        err = float(np.abs(got[ok] - ref[name][ok]).max()) if ok.any() else 0.0
        print("triple_logp %s N %d V %d: max |d| %.3e" % (name, N, V, err))
        assert err <= LP_TOL        # (the restatement is fed the device's own lse: the arithmetic of K-best's lp, its tolerance)
    if M >= 5:
        assert u32(res["mix"])[0, 0] == u32(res["mix"])[0, 1]
    if N == 1:
        assert np.array_equal(u32(res["mix"])[ok], u32(res["mean"])[ok]), "N = 1: mix == mean == lp"
    big2, out2 = lp_outputs(nb, M)
    res2 = hip.triple_logp(xd, lse, torch.from_numpy(gt).cuda(), torch.from_numpy(cnt).cuda(), out=out2)
    for name in res:
        assert np.array_equal(u32(res[name]), u32(res2[name])), "%s differs between two launches" % name


def test_triple_logp_equals_kbest_merge_bit_for_bit(hip):
    """The merged K-best list's triples as ground truth, K-best's own lse: mix is kbest_merge's score and max_k lp_k its best_logp -
    the same documented arithmetic on the same inputs, so no tolerance applies."""
    N, nb, V, Kc, K = 5, 3, 40, 16, 48
    x = (3.0 * np.random.RandomState(77).standard_normal((N, nb, 3, V))).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    per = hip.kbest_triples(xd, Kc)
    lse = per["lse"].view(N, nb, 3)
    merged = hip.kbest_merge(per["triples"].view(N, nb, Kc, 3), xd, lse, K)
    nd = merged["n_distinct"].clamp(max=K).to(I32)
    assert int(nd.min()) >= 20
    res = hip.triple_logp(xd, lse, merged["triples"], nd)
    torch.cuda.synchronize()
    st = res["status"].cpu().numpy()
    ok = st == 0
    assert np.array_equal(ok, np.arange(K)[None, :] < nd.cpu().numpy()[:, None])
    assert np.array_equal(u32(res["mix"])[ok], u32(merged["scores"])[ok]), "mix differs from kbest_merge's scores"
    # best_logp = max_k lp_k: every sample's lp through the N = 1 form of the same kernel (mix == lp there)
    lps = []
    for k in range(N):
        one = hip.triple_logp(xd[k:k + 1], lse[k:k + 1].contiguous(), merged["triples"], nd)
        lps.append(one["mix"].cpu().numpy())
    best = np.max(np.stack(lps), axis=0)
    assert np.array_equal(best[ok].view(np.uint32), u32(merged["best_logp"])[ok]), "max_k lp_k differs from kbest_merge's best_logp"


# ---- the step ------------------------------------------------------------------------------------------------------------------
B, S, V = 8, 64, 50


def _oracle_mle(gp, images, labels, noise, dp=None, w=1.0):
    """Autograd on the oracle: cost = [g_loss +] w * (1/B) sum_b sum_t -log softmax(logits[b, t])[labels[b, t]]."""
    for v in gp.values():
        v.requires_grad_(True)
    if dp is None:
        fake, gan = O.generator_forward(gp, images, noise), 0.0
    else:
        gan, aux = O.g_loss(gp, dp, images, noise)
        fake = aux["fake"]
    logp = torch.log_softmax(fake, dim=-1)
    xent = -logp.gather(-1, labels.unsqueeze(-1)).sum() / images.shape[0]
    grads = O._grads(gan + w * xent, gp)
    for v in gp.values():
        v.requires_grad_(False)
    return float(xent.detach()), fake.detach(), grads, (float(gan.detach()) if dp is not None else None)


def _arenas(gs):
    gs.flush()
    torch.cuda.synchronize()
    return {n + k: t.clone() for n, net in (("G", gs.G), ("D", gs.D))
            for k, t in ((".p", net.arena.flat), (".g", net.grad_flat), (".m", net.m_flat), (".v", net.v_flat))}


def test_pretrain_step_matches_oracle(hip):
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    gp0 = {k: v.clone() for k, v in gp.items()}
    images, labels, _ = O.synth_batch(B, S, V)
    noise = O.synth_noise(B, 0)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    before = _arenas(gs)
    xent, fake, grads, _ = _oracle_mle(gp, images, labels, noise)
    val = gs.generator_nll(images.cuda(), labels.cuda(), noise.cuda()).cpu()      # forward only, on the same weights: the same loss
    assert abs(float(val[0]) - xent / 3.0) <= loss_tol(xent / 3.0) and float(val[3]) == 3 * B
    ml = gs.pretrain_step(images.cuda(), labels.cuda(), noise.cuda()).cpu()
    nll_token = xent / 3.0
    print("pretrain_step: nll per token %.6f (oracle %.6f)" % (float(ml[0]), nll_token))
    assert abs(float(ml[0]) - nll_token) <= loss_tol(nll_token) and float(ml[3]) == 3 * B
    worst = max((tensor_err(gs.G.grads[n], g), n) for n, g in grads.items())
    print("pretrain_step gradients: worst rel err %.3e (%s)" % worst)
    assert worst[0] < GRAD_RTOL, "generator gradient %s: rel err %.3e" % (worst[1], worst[0])
    g_adam = O.new_adam_state(gp)
    O.tf_adam_step(gp, grads, g_adam[0], g_adam[1], 1)
    gs.flush()
    assert gs.G.adam_t == 1 and gs.D.adam_t == 0
    check_weights_after_adam(gs.G.arena.views, gp, grads, gp0, 1, "pretrain")
    margin = O.top2_margin(fake)
    if margin > MARGIN_FACTOR * logit_tol(fake.abs().max()):
        hits = (O.argmax_tokens(fake) == labels)
        assert abs(float(ml[1]) - float(hits.float().mean())) <= 1e-6
        assert abs(float(ml[2]) - float(hits.all(dim=1).float().mean())) <= 1e-6
    after = _arenas(gs)
    for k in before:
        if k.startswith("D"):
            assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), "pretrain_step touched %s" % k
    # the forward-only counterpart changes nothing
    gs.generator_nll(images.cuda(), labels.cuda(), noise.cuda())
    again = _arenas(gs)
    for k in after:
        assert torch.equal(again[k].view(torch.int32), after[k].view(torch.int32)), "generator_nll touched %s" % k
    with pytest.raises(RuntimeError, match="reuse"):
        with gs.iteration(reuse_g_encoder=True):
            gs.pretrain_step(images.cuda(), labels.cuda(), noise.cuda())


def test_generator_step_with_mle_weight_matches_oracle(hip):
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    dp["W"] = dp["W"] * 25.0
    images, labels, _ = O.synth_batch(B, S, V)
    noise = O.synth_noise(B, 1)
    img, lab, nz = images.cuda(), labels.cuda(), noise.cuda()
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    xent, _, grads, gan = _oracle_mle(gp, images, labels, noise, dp=dp, w=0.3)
    gl = gs.generator_step(img, nz, labels=lab, mle_weight=0.3).cpu()
    ml = gs.mle_losses.cpu()
    assert abs(-float(gl[3]) - gan) <= loss_tol(gan) and abs(float(ml[0]) - xent / 3.0) <= loss_tol(xent / 3.0)
    worst = max((tensor_err(gs.G.grads[n], g), n) for n, g in grads.items())
    print("generator_step(mle_weight 0.3) gradients: worst rel err %.3e (%s)" % worst)
    assert worst[0] < GRAD_RTOL, "generator gradient %s: rel err %.3e" % (worst[1], worst[0])
    # the term is in the gradient: without it the decoder bias gradient is far outside the tolerance
    plain = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    plain.generator_step(img, nz)
    assert tensor_err(plain.G.grads["decoder/bias"], grads["decoder/bias"]) > 100 * GRAD_RTOL
    # mle_weight = 0: the parent's step bit for bit, whether or not labels are handed over
    zero = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    zero.generator_step(img, nz, labels=lab, mle_weight=0.0)
    a, b = _arenas(plain), _arenas(zero)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(plain.g_losses, zero.g_losses) and float(zero.mle_losses.abs().max()) == 0.0


def test_pretrain_then_gan_iteration_two_stream_equals_serial(hip):
    """One pretrain_step then one train_iteration (two critic updates) on the two-stream schedule and on the serial one: the early
    encoder of the first critic update must not start from a state before the pretraining step's update of G."""
    Bs, Ss, Vs = 2, 32, 11
    images, labels, _ = O.synth_batch(Bs, Ss, Vs)
    img, lab = images.cuda(), labels.cuda()
    res = {}
    for overlap in (False, True):
        gp, dp = O.init_params("G", Vs, Ss, perturb=0.05), O.init_params("D", Vs, Ss, perturb=0.05)
        dp["W"] = dp["W"] * 25.0
        gs = GanStep(hip, Vs, Ss, Bs, lam=10.0, g_state=gp, d_state=dp, overlap_streams=overlap)
        gs.critic_step(img, lab, O.synth_noise(Bs, 20).cuda(), O.synth_alpha(Bs, 20).reshape(Bs).cuda())    # (leaves an event behind)
        gs.pretrain_step(img, lab, O.synth_noise(Bs, 9).cuda())
        gs.train_iteration(img, lab, [O.synth_noise(Bs, i).cuda() for i in range(3)],
                           [O.synth_alpha(Bs, i).reshape(Bs).cuda() for i in range(2)], critic_iters=2)
        res[overlap] = _arenas(gs)
        res[overlap]["mle"] = gs.mle_losses.clone()
    for k in res[False]:
        assert torch.equal(res[False][k].view(torch.int32), res[True][k].view(torch.int32)), "%s differs between the schedules" % k


def test_diagnostics_report_the_generator_alone_in_the_pretraining_phase(hip):
    Bs, Ss, Vs = 2, 32, 11
    images, labels, _ = O.synth_batch(Bs, Ss, Vs)
    gs = GanStep(hip, Vs, Ss, Bs, lam=10.0, g_state=O.init_params("G", Vs, Ss, perturb=0.05), d_state=O.init_params("D", Vs, Ss, perturb=0.05))
    gs.arm_diagnostics(True)
    gs.pretrain_step(images.cuda(), labels.cuda(), O.synth_noise(Bs, 0).cuda())
    with pytest.raises(RuntimeError, match="both networks"):
        gs.diagnostics()                              # (the GAN-phase report is what it was: it needs a step of the critic too)
    rec = gs.diagnostics(generator_only=True)
    assert set(rec) == {"G", "tensors"} and set(rec["tensors"]) == {"G"} and rec["G"]["first_nonfinite"] is None
    norm = float(gs.G.arena.live(gs.G.grad_flat).double().pow(2).sum().sqrt())
    assert abs(rec["G"]["grad_norm"] - norm) <= 1e-5 * norm


# ---- Generator.log_prob, SceneGraphGAN.likelihood, train.py --likelihood_out ------------------------------------------------------------
# Against the restatement fed with the same sample() logits and ITS OWN fp64 log-sum-exp: per triple the device differs by the three
# lse errors (XENT_TOL each) and the arithmetic of triple_logp (LP_TOL); means of such numbers differ by no more.
LIK_TOL = 3 * XENT_TOL + LP_TOL


def _lik_items(S, Vv):
    g = torch.Generator().manual_seed(77)
    imgs = [torch.randn((S, S, 3), generator=g) for _ in range(5)]
    gts = [[[1, 2, 3], [4, 5, 6], [1, 2, 3]], [[0, Vv - 1, 0]], [[7, 7, 7], [3, Vv, 2], [2, 0, 9], [8, 1, 1]], [[5, 5, 5]], [[9, 8, 7], [6, 5, 4]]]
    return list(zip(imgs, gts))


def test_log_prob_and_likelihood_match_the_restatement(tmp_path):
    """The untrained model of tests/test_predict_gpu.py, batch_size 8: TEST_BATCH_SIZE 4, 32 samples per image, five images = one full
    and one padded image batch; one true triple holds a token outside the vocabulary."""
    import json
    from tests.test_eval_batched_gpu import _gan
    S, Vv = 64, 50
    gan = _gan(tmp_path, 8, S, Vv)
    items = _lik_items(S, Vv)
    out = str(tmp_path / "nll.json")
    res = gan.likelihood(items=items, out_path=out)
    assert json.load(open(out)) == res
    assert (res["n_images"], res["n_triples"], res["n_out_of_vocab"], res["n_samples"], res["generator_weights"]) == (5, 10, 1, 32, "live")
    mix, mean, slot = [], [], []
    import contextlib
    with contextlib.closing(gan._sample_batches([(str(i), im) for i, (im, _) in enumerate(items)], 32, 4)) as batches:
        for i0, n, images, logits in batches:
            x = logits.cpu().numpy().astype(np.float64)
            for j in range(n):
                real = np.asarray(items[i0 + j][1], dtype=np.int64)[None]
                r = XR.triple_logp(x[:, j:j + 1], XR.lse64(x[:, j:j + 1]), real, [real.shape[1]])
                ok = r["status"][0] == 0
                mix.append(-r["mix"][0][ok]); mean.append(-r["mean"][0][ok]); slot.append(-r["slot"][0][ok])
    want = {"mix_micro": np.concatenate(mix).mean(), "mix_macro": np.mean([m.mean() for m in mix]),
            "mean_micro": np.concatenate(mean).mean(), "mean_macro": np.mean([m.mean() for m in mean])}
    got = {"mix_micro": res["nll_mixture"]["micro"], "mix_macro": res["nll_mixture"]["macro"],
           "mean_micro": res["nll_single"]["micro"], "mean_macro": res["nll_single"]["macro"]}
    for k in want:
        print("likelihood %s: %.7f (restatement %.7f)" % (k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= LIK_TOL, k
    assert np.abs(np.array(res["nll_slot"]) - np.concatenate(slot).mean(axis=0)).max() <= LIK_TOL
    assert abs(res["perplexity_token"] - np.exp(res["nll_single"]["micro"] / 3.0)) <= 1e-12
    assert res["nll_single"]["micro"] >= res["nll_mixture"]["micro"], "Jensen: the mixture is at least as likely as the mean draw"
    # Generator.log_prob on the first four images with a noise of its own
    noise = torch.randn((6, 4, 512), generator=torch.Generator().manual_seed(3)).cuda()
    images = torch.stack([im for im, _ in items[:4]]).cuda()
    gt = torch.zeros((4, 4, 3), dtype=torch.int64)
    cnt = torch.tensor([len(r) for _, r in items[:4]], dtype=torch.int32)
    for j, (_, real) in enumerate(items[:4]):
        gt[j, :len(real)] = torch.tensor(real)
    m, a, s, st = gan.g.log_prob(images, gt.cuda(), cnt.cuda(), 6, noise)
    x = gan.g.sample(images, 6, noise).cpu().numpy().astype(np.float64)
    ref = XR.triple_logp(x, XR.lse64(x), gt.numpy(), cnt.numpy())
    assert np.array_equal(st.cpu().numpy(), ref["status"]) and ref["status"][2, 1] == -4 and ref["status"][1, 1] == -3
    ok = ref["status"] == 0
    for name, t in (("mix", m), ("mean", a), ("slot", s)):
        h = t.cpu().numpy()
        assert np.isnan(h[~ok]).all() and float(np.abs(h[ok] - ref[name][ok]).max()) <= LIK_TOL, name


def test_likelihood_out_cli(tmp_path):
    """train.py --likelihood_out in a fresh child process: the JSON it writes is what likelihood() gives in-process on the loaded
    checkpoint."""
    import json
    import os
    import subprocess
    import sys
    from tests.test_eval_batched_gpu import _gan
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1", "--checkpoints_dir", str(tmp_path / "ck"),
              "--summaries_dir", str(tmp_path / "logs")]
    run = lambda extra: subprocess.run([sys.executable, os.path.join(root, "train.py")] + common + extra, cwd=str(tmp_path),
                                       capture_output=True, text=True, timeout=600)
    r = run(["--max_iterations", "2", "--pretrain_iterations", "1", "--log_every", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in open(str(tmp_path / "logs" / "losses.jsonl")) if l.strip()]
    assert [x.get("phase") for x in recs] == ["pretrain", None] and 0.0 < recs[0]["mle_nll_token"] < 2.0 * np.log(50)
    out = tmp_path / "nll.json"
    r = run(["--likelihood_out", str(out), "--max_test_images", "2", "--predict_samples", "8", "--pretrain_iterations", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    written = json.load(open(str(out)))
    gan = _gan(tmp_path, 8, 64, 50)
    assert gan.load_checkpoint()
    assert written == json.loads(json.dumps(gan.likelihood(max_images=2, n_samples=8)))
    assert written["n_images"] == 2 and written["n_triples"] == 10 and written["n_samples"] == 8 and written["nll_mixture"]["micro"] > 0
