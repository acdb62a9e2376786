"""-m gpu: every kernel route of the head GEMM (csrc/gemm.hip) and of the attention step (csrc/head.hip) against fp64
(oracle/kernels_ref.py, torch fp64 matmul), one case per route and operand form (tests/head_route_cases.py).

Every case (a) asserts through the library's route query that it runs the kernels it is named for, (b) compares the result with the
fp64 reference, per plane for dual numbers (close_planes: each plane against its own max|ref|), (c) lets the outputs land in
NaN-filled wider buffers and asserts that nothing outside the target was written.  Operands in the strided / offset forms sit in
NaN-filled buffers as well: an element read outside the valid range shows in the result.

Tolerances are the project's (tests/test_kernels_gpu.py): GEMM and attention forward 2e-5, attention backward 5e-5, LSTM backward
1e-4, each times the plane's max|ref|, plus 1e-6.  Every comparison prints its measured maximum error (pytest -s / -rA)."""
import functools

import pytest
import torch

import sgg_amd  # noqa: F401
from oracle.kernels_ref import RefKernels
from sgg_amd.lib import SggError
from tests import head_route_cases as RC
from tests import head_shapes as HS
from tests.test_kernels_gpu import close, close_planes, dev, rnd

pytestmark = pytest.mark.gpu

NAN = float("nan")
REF = RefKernels()


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def ceil4(n):
    return (n + 3) // 4 * 4


def guarded(shape, pad):
    """(buffer, view): a NaN-filled buffer with `pad[i]` guard elements on both sides of dimension i and the view of `shape` inside."""
    buf = nans(*[s + 2 * p for s, p in zip(shape, pad)])
    view = buf
    for i, (s, p) in enumerate(zip(shape, pad)):
        view = view.narrow(i, p, s)
    return buf, view


def untouched(buf, view, what):
    """Nothing but `view` was written in `buf` (all of it was NaN); the view itself holds no NaN."""
    assert not torch.isnan(view).any(), what + ": NaN inside the target"
    n_nan = int(torch.isnan(buf).sum())
    assert n_nan == buf.numel() - view.numel(), "%s: %d elements outside the target were written" % (what, buf.numel() - view.numel() - n_nan)


def operand(x, form):
    """x (CPU, [rows, width]) on the device in the given form; the padding is NaN."""
    rows, width = x.shape
    if form in ("plain", "bias+acc"):
        d = dev(x)
        assert d.data_ptr() % 16 == 0
        return d
    if form == "off1":
        ld = ceil4(width) + 4
        flat = nans(rows * ld + 4)
        d = flat[1:1 + rows * ld].view(rows, ld)[:, :width]
        assert d.data_ptr() % 16 == 4 and d.stride(0) % 4 == 0
    else:
        ld = width + 4 if form == "ld+4" else ceil4(width)
        d = nans(rows, ld)[:, :width]
        assert d.data_ptr() % 16 == 0 and (form != "tail2" or d.stride(0) % 4 == 0)
    d.copy_(x)
    return d


# ---- GEMM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.GEMM_CASES, ids=lambda c: "%s-%dx%dx%d-%s" % (("NN", "NT", "TN")[c[0]], c[1], c[2], c[3], c[4]))
def test_gemm_route(hip, case):
    mode, M, N, K, form, kernels = case
    assert hip.gemm_symbol(mode, M, N, K)[0] == kernels
    A, Bm = rnd((M, K), 111), rnd((K, N), 112)
    bias = rnd((N,), 113) if (mode == RC.NN and form in ("off1", "bias+acc")) else None
    accumulate = form in ("ld+4", "bias+acc")
    C0 = rnd((M, N), 114)
    ref = A.double() @ Bm.double()
    if bias is not None:
        ref = ref + bias.double()
    if accumulate:
        ref = ref + C0.double()
    buf, C = guarded((M, N), (1, 4))
    if accumulate:
        C.copy_(C0)
    if mode == RC.NN:
        hip.gemm_nn(operand(A, form), operand(Bm, form), C, None if bias is None else dev(bias), accumulate)
    elif mode == RC.NT:
        hip.gemm_nt(operand(A, form), operand(Bm.t().contiguous(), form), C, accumulate)
    else:
        hip.gemm_tn(operand(A.t().contiguous(), form), operand(Bm, form), C, accumulate)
    what = "gemm %s %s" % (case[:5], kernels)
    close(C, ref, what=what)
    untouched(buf, C, what)


# ---- attention forward ------------------------------------------------------------------------------------------------------
def attn_inputs(B, N, L, C, np_, tangent_scale=1.0):
    R = B * N
    P, ctx = rnd((B, L), 120), rnd((B, L, C), 121)
    ec, dz = rnd((np_, R, L), 122), rnd((np_, R, C), 123)
    if np_ == 2:                      # tangent inputs: the dual plane of ec, the real plane of the cotangent dz
        ec[1] *= tangent_scale
        dz[0] *= tangent_scale
    return P, ctx, ec, dz


@functools.lru_cache(maxsize=None)
def attn_fwd_ref(B, N, L, C, np_, tangent_scale=1.0):
    P, ctx, ec, _ = attn_inputs(B, N, L, C, np_, tangent_scale)
    al = torch.empty((np_, B * N, L), dtype=torch.float64)
    z = torch.empty((np_, B * N, C), dtype=torch.float64)
    REF.attn_step_fwd(P.double(), ec.double(), ctx.double(), al, z)
    return al, z


def run_attn_fwd(hip, B, N, L, C, dual, tangent_scale=1.0):
    np_, R = (2 if dual else 1), B * N
    P, ctx, ec, _ = attn_inputs(B, N, L, C, np_, tangent_scale)
    al_ref, z_ref = attn_fwd_ref(B, N, L, C, np_, tangent_scale)
    albuf, al = guarded((np_, R, L), (0, 1, 0))
    zbuf, z = guarded((np_, R, C), (0, 1, 8))
    hip.attn_step_fwd(dev(P), dev(ec), dev(ctx), al, z)
    what = "attn fwd (B %d, N %d, L %d, C %d, %s)" % (B, N, L, C, "dual" if dual else "float")
    close_planes(al, al_ref, what=what + " alpha")
    close_planes(z, z_ref, what=what + " z")
    untouched(albuf, al, what + " alpha")
    untouched(zbuf, z, what + " z")


@pytest.mark.parametrize("case", RC.ATTN_FWD_CASES, ids=lambda c: "B%d-N%d-L%d-C%d-%s" % (c[0], c[1], c[2], c[3], "dual" if c[4] else "float"))
def test_attention_forward_route(hip, case):
    B, N, L, C, dual = case
    assert hip.attn_step_fwd_symbol(B * N, B, L, C, dual) == "attn_step_fwd_kernel<%s>" % ("Dual" if dual else "float")
    run_attn_fwd(hip, B, N, L, C, dual)


# ---- attention backward -----------------------------------------------------------------------------------------------------
def attn_bwd_inputs(B, npass, L, C, np_, tangent_scale=1.0):
    """alpha: a softmax (and, dual, a tangent of one: its rows sum to 0) as float32 - the backward's input as it stands."""
    R = B * npass
    ctx, dz = rnd((B, L, C), 131), rnd((np_, R, C), 133)
    a0 = torch.softmax(rnd((R, L), 132).double(), dim=1)
    planes = [a0]
    if np_ == 2:
        t = rnd((R, L), 134).double() * tangent_scale
        planes.append(a0 * (t - (a0 * t).sum(dim=1, keepdim=True)))
        dz[0] *= tangent_scale
    return ctx, torch.stack(planes).float(), dz, rnd((B, L), 135), rnd((B, L, C), 136)


@functools.lru_cache(maxsize=None)
def attn_bwd_ref(B, npass, L, C, np_, tangent_scale=1.0):
    """(de, dP update, dctx update) in fp64: computed once per case, shared by the accumulate on / off runs."""
    ctx, al, dz, _, _ = attn_bwd_inputs(B, npass, L, C, np_, tangent_scale)
    de = torch.empty((np_, B * npass, L), dtype=torch.float64)
    dP, dctx = torch.zeros((B, L), dtype=torch.float64), torch.zeros((B, L, C), dtype=torch.float64)
    REF.attn_step_bwd(ctx.double(), al.double(), dz.double(), de, dP, dctx, False)
    return de, dP, dctx


def run_attn_bwd(hip, B, npass, L, C, dual, accumulate, tangent_scale=1.0):
    np_, R = (2 if dual else 1), B * npass
    ctx, al, dz, dP0, dctx0 = attn_bwd_inputs(B, npass, L, C, np_, tangent_scale)
    de_ref, dP_ref, dctx_ref = attn_bwd_ref(B, npass, L, C, np_, tangent_scale)
    debuf, de = guarded((np_, R, L), (0, 1, 0))
    dPbuf, dP = guarded((B, L), (1, 0))
    dcbuf, dctx = guarded((B, L, C), (1, 0, 0))
    if accumulate:
        dP.copy_(dP0)
        dctx.copy_(dctx0)
        dP_ref, dctx_ref = dP_ref + dP0.double(), dctx_ref + dctx0.double()
    hip.attn_step_bwd(dev(ctx), dev(al), dev(dz), de, dP, dctx, accumulate)
    what = "attn bwd (B %d, npass %d, L %d, C %d, %s, accumulate %d)" % (B, npass, L, C, "dual" if dual else "float", accumulate)
    close_planes(de, de_ref, rtol=5e-5, what=what + " de")
    close(dP, dP_ref, rtol=5e-5, what=what + " dP")
    close(dctx, dctx_ref, rtol=5e-5, what=what + " dctx")
    for buf, view, name in ((debuf, de, " de"), (dPbuf, dP, " dP"), (dcbuf, dctx, " dctx")):
        untouched(buf, view, what + name)


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("case", RC.ATTN_BWD_CASES, ids=lambda c: "B%d-npass%d-L%d-C%d-%s" % (c[0], c[1], c[2], c[3], "dual" if c[4] else "float"))
def test_attention_backward_route(hip, case, accumulate):
    B, npass, L, C, dual, kernels = case
    assert hip.attn_step_bwd_symbol(B * npass, B, L, C, dual) == kernels
    run_attn_bwd(hip, B, npass, L, C, dual, accumulate)


def test_attention_backward_refuses_five_rows_per_image(hip):
    B, npass, L, C = 2, 5, 16, 256
    with pytest.raises(SggError, match="at most 4 rows per image"):
        hip.attn_step_bwd_symbol(B * npass, B, L, C, False)
    ctx, al, dz, _, _ = attn_bwd_inputs(B, npass, L, C, 1)
    de, dP, dctx = nans(1, B * npass, L), nans(B, L), nans(B, L, C)
    with pytest.raises(SggError, match="at most 4 rows per image"):
        hip.attn_step_bwd(dev(ctx), dev(al), dev(dz), de, dP, dctx, False)
    torch.cuda.synchronize()
    assert torch.isnan(de).all() and torch.isnan(dP).all() and torch.isnan(dctx).all()      # nothing was launched


# ---- dual planes with small tangents, each plane held to its own scale --------------------------------------------------------
TANGENT_SCALE = 1e-3    # the tangent inputs: the dual plane of gates, c_prev, ec; the real plane of the cotangents dh, dc_new, dz


def test_attention_step_small_tangents_per_plane(hip):
    B, npass, L, C = 3, 2, 196, 512
    run_attn_fwd(hip, B, npass, L, C, True, TANGENT_SCALE)
    al_ref, _ = attn_fwd_ref(B, npass, L, C, 2, TANGENT_SCALE)
    assert float(al_ref[1].abs().max()) < 1e-2 * float(al_ref[0].abs().max())           # the planes are orders apart
    for accumulate in (False, True):
        run_attn_bwd(hip, B, npass, L, C, True, accumulate, TANGENT_SCALE)


def test_lnlstm_gates_small_tangents_per_plane(hip):
    R = 6
    gates, c_prev = rnd((2, R, 2048), 30, 1.5), rnd((2, R, 512), 31)
    ln = torch.stack([1.0 + rnd((512,), 32 + i, 0.2) if i % 2 == 0 else rnd((512,), 32 + i, 0.2) for i in range(10)])
    dh, dcn = rnd((2, R, 512), 50), rnd((2, R, 512), 51)
    for t in (gates[1], c_prev[1], dh[0], dcn[0]):
        t *= TANGENT_SCALE
    cn_ref, h_ref = (torch.empty((2, R, 512), dtype=torch.float64) for _ in range(2))
    REF.lstm_fwd(gates.double(), c_prev.double(), ln.double(), cn_ref, h_ref)
    dg_ref = torch.empty((2, R, 2048), dtype=torch.float64)
    dcp_ref = torch.empty((2, R, 512), dtype=torch.float64)
    pg_ref = torch.empty((R, 10, 512), dtype=torch.float64)
    REF.lstm_bwd(gates.double(), c_prev.double(), ln.double(), dh.double(), dcn.double(), dg_ref, dcp_ref, pg_ref)
    assert float(cn_ref[1].abs().max()) < 1e-2 * float(cn_ref[0].abs().max())
    gd, cd, lnd = dev(gates), dev(c_prev), dev(ln)
    cn = nans(2, R, 512)
    hbuf, h = guarded((2, R, 512), (0, 1, 8))
    hip.lstm_fwd(gd, cd, lnd, cn, h)
    close_planes(cn, cn_ref, what="lstm small tangents c_new")
    close_planes(h, h_ref, what="lstm small tangents h_new")
    untouched(hbuf, h, "lstm small tangents h_new")
    dg, dcp, pg = nans(2, R, 2048), nans(2, R, 512), nans(R, 10, 512)
    hip.lstm_bwd(gd, cd, lnd, dev(dh), dev(dcn), dg, dcp, pg)
    close_planes(dg, dg_ref, rtol=1e-4, what="lstm small tangents dgates")
    close_planes(dcp, dcp_ref, rtol=1e-4, what="lstm small tangents dc_prev")
    close(pg, pg_ref, rtol=1e-4, what="lstm small tangents pgrad")


# ---- column sums: the single-stage path every head call takes (rows <= 192), the 512 | 513 edge of the two-stage path -----------
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("rows", [192, 512, 513])
def test_colsum_stages(hip, rows, accumulate):
    cols, ld = 1000, 1008
    assert (hip.lib.sgg_colsum_workspace_bytes(rows, cols) > 0) == (rows > 512)
    X, out0 = rnd((rows, cols), 140), rnd((cols,), 141)
    Xd = nans(rows, ld)[:, :cols]
    Xd.copy_(X)
    buf, out = guarded((cols,), (8,))
    if accumulate:
        out.copy_(out0)
    hip.colsum(Xd, out, accumulate)
    ref = X.double().sum(0) + (out0.double() if accumulate else 0.0)
    what = "colsum rows %d accumulate %d" % (rows, accumulate)
    close(out, ref, what=what)
    untouched(buf, out, what)


# ---- tests/head_shapes.py against the real step ---------------------------------------------------------------------------------
def test_head_shapes_equal_the_recorded_step(hip, monkeypatch):
    """The _gemm / attn_step_* calls of one critic + generator step at B = 8, S = 64, V = 50 (the setup of test_step_gpu.py) are
    the launches tests/head_shapes.py lists for that size: the closure of tests/test_head_routes_cpu.py stands on that list."""
    from oracle import sgg_oracle as O
    from sgg_amd.step import GanStep
    B, S, V = 8, 64, 50
    seen = set()
    gemm, fwd, bwd = hip._gemm, hip.attn_step_fwd, hip.attn_step_bwd

    def rec_gemm(mode, M, N, K, *rest):
        seen.add(("gemm", mode, M, N, K))
        return gemm(mode, M, N, K, *rest)

    def rec_fwd(P, ec, ctx, alpha, z):
        seen.add(("attn_fwd", ec.shape[1]) + tuple(ctx.shape) + (ec.shape[0] == 2,))
        return fwd(P, ec, ctx, alpha, z)

    def rec_bwd(ctx, alpha, *rest):
        seen.add(("attn_bwd", alpha.shape[1]) + tuple(ctx.shape) + (alpha.shape[0] == 2,))
        return bwd(ctx, alpha, *rest)
    monkeypatch.setattr(hip, "_gemm", rec_gemm)
    monkeypatch.setattr(hip, "attn_step_fwd", rec_fwd)
    monkeypatch.setattr(hip, "attn_step_bwd", rec_bwd)
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    dp["W"] = dp["W"] * 25.0          # slopes > 1: the gradient penalty, and with it the dual-number pass, is active
    images, labels, _ = O.synth_batch(B, S, V)
    noise0, noise1, alpha = O.synth_noise(B, 0), O.synth_noise(B, 1), O.synth_alpha(B, 0)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    gs.critic_step(images.cuda(), labels.cuda(), noise0.cuda(), alpha.reshape(B).cuda())
    gs.generator_step(images.cuda(), noise1.cuda())
    torch.cuda.synchronize()
    # (measured, not asserted: how far apart the planes of the real gradient-penalty pass are - what close_planes is there for)
    st2 = gs.D.head.state(2, B)
    # (time step 1: at step 0 the state c0 = h0 carries no tangent, so alpha's dual plane is zero there)
    for name, t in (("alpha", st2.AL[1]), ("gates", st2.G[1]), ("z | u | h", st2.XH[2]), ("dgates", st2.dG[1]), ("de", st2.dE[1])):
        print("gradient-penalty pass, %s: max|dual plane| / max|real plane| = %.3e" % (name, float(t[1].abs().max()) / max(float(t[0].abs().max()), 1e-30)))
    listed = HS.step_launches(B, HS.feature_locations(S), V)
    assert seen == listed, "recorded but not listed: %s; listed but not recorded: %s" % (sorted(seen - listed), sorted(listed - seen))
