"""-m gpu: the LayerNorm kernels (csrc/layernorm.hip) at the launch geometry of the batch-64 step, against fp64.

The kernels take their geometry from (B, HW * C) alone (tests/ln_cases.py restates it).  At the batches of the other kernel tests
every workgroup walks ONE chunk: the chunk loops make one trip, the running (n, mean, M2, max deviation) merge of
ln_stats_partial_kernel never merges, and the sample loops of ln_bwd_finalize_body make at most one trip per lane.  The cases of
tests/ln_cases.py have B = 64 .. 256 and cpg = 2 .. 4 on planes of about 100 k elements per sample; three of them carry a valid
window whose rows leave whole workgroups empty and whole chunks skipped.

Inputs: y = 2 * randn + 0.3 plus a ramp along H and one along W, each of amplitude up to 3, with slopes that differ per sample.
Without them the chunk means agree to about 0.03 and a wrong between-chunk term of the merge moves rstd by 1e-4 of itself; with them
the means of the chunks ONE workgroup merges differ by a tenth of the standard deviation or more (the ramp along W is what separates
the two half-row chunks of a C = 512 workgroup, which the ramp along H alone leaves equal).  da = randn times a per-sample factor in [0.5, 2] (the per-sample sums the finalize reduces cannot be exchanged
between samples unnoticed); canvas pixels outside a window hold 1e6 / -1e6.

Tolerances are those of tests/test_kernels_gpu.py (test_layernorm_elu, test_layernorm_elu_valid_region): 2e-5 for a and the
statistics, 5e-5 for dy, dgamma and dbeta (fewer terms per reduction than the 448-px test that holds 5e-5), 1e-5 / 1e-4 for the
published maxima.  dbias_prev: see DBIAS_ATOL.
"""
import os

import pytest
import torch

from tests import ln_cases as L
from tests.s16_ref import s16_pieces, to_s16

pytestmark = pytest.mark.gpu
IDS = [c.id for c in L.CASES]

# dbias_prev = sum_b rstd_b * (gamma_c * A_bc - HW * s1_b - X_bc * s2_b) is a cancelling combination of per-sample sums; its f32
# error at B >= 64 had not been measured.  DBIAS_MEASURED: max|hip - fp64| per case on an MI355X with this file's inputs (the
# kernels sum in a fixed order: the figures repeat), max|dbias_ref| beside it.  atol = 10 x the largest of them (the project's
# convention for a measured tolerance), no relative part; the test also holds it under 1e-3 * max|dbias_ref| of every case - it is
# 6e-6 of the smallest.
DBIAS_MEASURED = {      # id: (max|hip - fp64|, max|dbias_ref|)
    "b64_c256": (2.804e-05, 209.0), "b70_c32": (9.117e-05, 478.0), "b256_c128": (1.164e-04, 499.4),
    "b96_c512_win": (3.875e-05, 185.6), "b96_c512_win0": (3.380e-05, 205.5), "b96_c256_win_skip": (5.294e-05, 243.0),
}
DBIAS_ATOL = 10 * max(err for err, _ in DBIAS_MEASURED.values())      # 1.164e-03


def g(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=g(seed), dtype=torch.float32) * scale


def close(hip_t, ref_t, rtol=2e-5, atol=1e-6, what=""):
    h, r = hip_t.detach().cpu().double(), ref_t.detach().cpu().double()
    assert h.shape == r.shape, (what, h.shape, r.shape)
    assert torch.isfinite(h).all(), what + ": non-finite values"
    tol = atol + rtol * float(r.abs().max())
    err = float((h - r).abs().max())
    print("%-44s max err %.3e, tol %.3e (max|ref| %.3e)" % (what, err, tol, float(r.abs().max())))
    assert err <= tol, "%s: max err %.3e > tol %.3e (max|ref| %.3e)" % (what, err, tol, float(r.abs().max()))


def inputs(case):
    """(y, da, gamma, beta) on the host, f32."""
    B, H, W, C = case.shape
    k = IDS.index(case.id)
    sample = torch.arange(B, dtype=torch.float32)
    slope = torch.where(sample % 2 == 0, 1.0, -1.0) * (0.5 + 0.5 * sample / (B - 1))      # alternating sign, |slope| 0.5 .. 1
    ramp = 3.0 * slope.view(B, 1, 1, 1) * torch.linspace(-1.0, 1.0, H).view(1, H, 1, 1)
    ramp = ramp + 3.0 * slope.flip(0).view(B, 1, 1, 1) * torch.linspace(-1.0, 1.0, W).view(1, 1, W, 1)
    y = rnd(case.shape, 7 + 100 * k, 2.0) + 0.3 + ramp
    factor = 0.5 + 1.5 * torch.rand(B, generator=g(11 + 100 * k))
    da = rnd(case.shape, 10 + 100 * k) * factor.view(B, 1, 1, 1)
    gamma, beta = 1.0 + rnd((C,), 8 + 100 * k, 0.2), rnd((C,), 9 + 100 * k, 0.2)
    if case.region is not None:
        r0, c0, hv, wv = case.region
        inside = torch.zeros((1, H, W, 1), dtype=torch.bool)
        inside[:, r0:r0 + hv, c0:c0 + wv] = True
        y = torch.where(inside, y, torch.full((), 1e6))
        da = torch.where(inside, da, torch.full((), -1e6))
    return y, da, gamma, beta


_REFS = {}


def references(case, ref, tensors=True):
    """fp64 reference of the case (oracle/kernels_ref.py), computed once: the statistics, the parameter gradients and the maxima
    stay cached for every case, the two full-size tensors a and dy (up to 184 MB each) only for the case that is used twice."""
    hit = _REFS.get(case.id)
    if hit is not None and (not tensors or hit.get("dy") is not None):
        return hit
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    B, H, W, C = case.shape
    y, da, gamma, beta = (t.double() for t in inputs(case))
    a = torch.empty(case.shape, dtype=torch.float64)
    st = torch.empty((B, 2), dtype=torch.float64)
    ref.ln_elu_fwd(y, gamma, beta, a, st, region=case.region)
    dy = torch.empty(case.shape, dtype=torch.float64)
    dg, db, dbias = (torch.empty(C, dtype=torch.float64) for _ in range(3))
    ref.ln_elu_bwd(y, da, gamma, beta, st, dy, dg, db, dbias, region=case.region)
    out = {"stats": st, "dgamma": dg, "dbeta": db, "dbias": dbias, "a": a, "dy": dy}
    _REFS[case.id] = dict(out) if case.id == L.FUSED_C3_CASE else {k: (None if k in ("a", "dy") else v) for k, v in out.items()}
    return out


def pin_geometry(hip, case):
    """The library's workspace size is a function of G: it ties the Python mirror to ln_geom without a C entry point of its own."""
    B, H, W, C = case.shape
    geo = L.ln_geometry(B, H * W, C)
    assert (geo.G, geo.cpg) == (case.G, case.cpg) and geo.cpg >= 2
    assert hip.ln_workspace_bytes(case.shape) == B * geo.G * (L.TS + 2 + 3 * C) * 4 + 256, \
        "%s: the library does not cut this shape into G = %d workgroups per sample" % (case.id, geo.G)


def outside(case):
    """[H, W] mask of the canvas pixels outside the window."""
    B, H, W, C = case.shape
    m = torch.ones((H, W), dtype=torch.bool)
    r0, c0, hv, wv = case.region
    m[r0:r0 + hv, c0:c0 + wv] = False
    return m


@pytest.mark.parametrize("case", L.CASES, ids=IDS)
def test_f32_outputs_against_fp64(hip, ref, case):
    """2a.  sgg_layernorm_hwc_elu_fwd / _bwd, f32 outputs, immediate finalize: a, stats, both published maxima, dy, dgamma, dbeta
    and dbias_prev against oracle/kernels_ref.py in float64.

    dbias_prev: measured max|hip - fp64| 2.8e-5 .. 1.16e-4 on max|ref| 186 .. 499 (DBIAS_MEASURED, per case); atol = DBIAS_ATOL =
    10 x the largest = 1.164e-3, no relative part, and never above 1e-3 * max|dbias_ref| (0.186 for the smallest case)."""
    pin_geometry(hip, case)
    B, H, W, C = case.shape
    r = references(case, ref)
    y, da, gamma, beta = (t.cuda() for t in inputs(case))
    a = torch.full(case.shape, float("nan"), device="cuda")
    st = torch.full((B, 2), float("nan"), device="cuda")
    amax = torch.zeros(2, device="cuda")
    hip.ln_elu_fwd(y, gamma, beta, a, st, amax[0:1], region=case.region)
    close(a, r["a"], what="%s a" % case.id)
    close(st, r["stats"], what="%s stats" % case.id)
    a_max = float(r["a"].abs().max())
    assert abs(float(amax[0]) - a_max) <= 1e-5 * a_max, (float(amax[0]), a_max)
    if case.region is not None:
        assert torch.equal(a.cpu() == 0, r["a"] == 0), "zeros exactly outside the window"
        assert float(a.cpu()[:, outside(case)].abs().max()) == 0.0
    del a
    dy = torch.full(case.shape, float("nan"), device="cuda")
    dg, db, dbias = (torch.full((C,), float("nan"), device="cuda") for _ in range(3))
    hip.ln_elu_bwd(y, da, gamma, beta, st, dy, dg, db, dbias, amax[1:2], region=case.region)
    close(dy, r["dy"], rtol=5e-5, what="%s dy" % case.id)
    dy_max = float(r["dy"].abs().max())
    assert abs(float(amax[1]) - dy_max) <= 1e-4 * dy_max, (float(amax[1]), dy_max)
    if case.region is not None:
        assert float(dy.cpu()[:, outside(case)].abs().max()) == 0.0
    close(dg, r["dgamma"], rtol=5e-5, what="%s dgamma" % case.id)
    close(db, r["dbeta"], rtol=5e-5, what="%s dbeta" % case.id)
    ref_max = float(r["dbias"].abs().max())
    print("%s dbias_prev: max|hip - fp64| %.3e, max|ref| %.3e, cap %.3e" % (
        case.id, float((dbias.cpu().double() - r["dbias"]).abs().max()), ref_max, 1e-3 * ref_max))
    assert DBIAS_ATOL <= 1e-3 * ref_max, "the measured tolerance exceeds 1e-3 of this case's bias gradient"
    close(dbias, r["dbias"], rtol=0.0, atol=DBIAS_ATOL, what="%s dbias_prev" % case.id)


@pytest.fixture
def mode2(hip):
    old = hip.conv_precision
    hip.conv_precision = 2
    yield hip
    hip.conv_precision = old


@pytest.mark.parametrize("case", L.CASES, ids=IDS)
def test_presplit_outputs_are_the_split_of_the_f32_outputs(mode2, case):
    """2b.  out_format 1 (what the default precision mode runs): the planes that ln_apply_elu_s16_kernel / ln_bwd_apply_s16_kernel
    write in their cpg > 1 loops - lane-pair exchange with the `in` predicate at a ragged chunk that is not the first - are bit for
    bit f16_split2 of the f32 kernels' outputs under the published bound, as tests/test_presplit_gpu.py asserts at cpg = 1."""
    hip = mode2
    pin_geometry(hip, case)
    B, H, W, C = case.shape
    y, da, gamma, beta = (t.cuda() for t in inputs(case))
    # ---- forward: a = ELU(LN(y)) ----
    a32, a16 = torch.empty_like(y), torch.full_like(y, float("nan"))
    st32, st16 = torch.empty((B, 2), device="cuda"), torch.empty((B, 2), device="cuda")
    w32, w16 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    hip.ln_elu_fwd(y, gamma, beta, a32, st32, w32, None, region=case.region)
    hip.ln_elu_fwd(y, gamma, beta, a16, st16, w16, None, region=case.region, out_s16=True)
    assert torch.allclose(st16, st32, rtol=1e-6, atol=0)
    amax, bound = float(w32), float(w16)
    print("%s forward bound / amax = %.3f" % (case.id, bound / amax))
    assert amax <= bound <= 16.0 * amax, (amax, bound)          # an upper bound, within four binades
    a32c = a32.cpu()
    exp_hi, exp_lo = s16_pieces(to_s16(a32c, bound))
    got_hi, got_lo = s16_pieces(a16.cpu())
    assert torch.equal(got_hi, exp_hi) and torch.equal(got_lo, exp_lo), "forward planes differ from f16_split2 of the f32 output"
    if case.region is not None:
        out = outside(case).reshape(-1).repeat(B)
        assert float(a32c.reshape(-1, C)[out].abs().max()) == 0.0
        assert not got_hi[out].any() and not got_lo[out].any(), "pre-split a: non-zero pieces outside the window"
    del a32, a16, a32c
    # ---- backward: dy ----
    dy32, dy16 = torch.empty_like(y), torch.full_like(y, float("nan"))
    ws = torch.empty(hip.ln_workspace_bytes(case.shape), dtype=torch.uint8, device="cuda")
    v32, v16 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    hip.ln_elu_bwd(y, da, gamma, beta, st32, dy32, None, None, None, v32, region=case.region, ws=ws)
    hip.ln_elu_bwd(y, da, gamma, beta, st32, dy16, None, None, None, v16, region=case.region, ws=ws, out_s16=True)
    amax, bound = float(v32), float(v16)
    print("%s backward bound / amax = %.3f" % (case.id, bound / amax))
    assert amax <= bound <= 64.0 * amax, (amax, bound)
    dy32c = dy32.cpu()
    exp_hi, exp_lo = s16_pieces(to_s16(dy32c, bound))
    got_hi, got_lo = s16_pieces(dy16.cpu())
    assert torch.equal(got_hi, exp_hi) and torch.equal(got_lo, exp_lo), "backward planes differ from f16_split2 of the f32 output"
    if case.region is not None:
        assert float(dy32c.reshape(-1, C)[out].abs().max()) == 0.0
        assert not got_hi[out].any() and not got_lo[out].any(), "pre-split dy: non-zero pieces outside the window"


def test_deferred_finalize_of_all_cases_in_one_launch_equals_immediate(hip):
    """2c.  Every case as one layer of ONE sgg_layernorm_hwc_bwd_finalize launch: mixed B, so the launch sizes its LDS from
    maxB = 256 while the B = 64 layer places its reduce array behind 2 * 64 floats; one layer without a bias gradient.  dy of the
    deferred call and dgamma, dbeta, dbias of the batched launch are bit-equal to the immediate path's."""
    lays, refs = [], []
    for j, case in enumerate(L.CASES):
        pin_geometry(hip, case)
        B, H, W, C = case.shape
        y, da, gamma, beta = (t.cuda() for t in inputs(case))
        a, st = torch.empty(case.shape, device="cuda"), torch.empty((B, 2), device="cuda")
        hip.ln_elu_fwd(y, gamma, beta, a, st, region=case.region)
        del a
        mk = lambda: torch.full((C,), float("nan"), device="cuda")
        dy1, dg1, db1, dbias1 = torch.empty(case.shape, device="cuda"), mk(), mk(), mk()
        hip.ln_elu_bwd(y, da, gamma, beta, st, dy1, dg1, db1, dbias1, region=case.region)
        ws = torch.empty(hip.ln_workspace_bytes(case.shape), dtype=torch.uint8, device="cuda")
        dy2, dg2, db2, dbias2 = torch.empty(case.shape, device="cuda"), mk(), mk(), (mk() if j != 1 else None)
        hip.ln_elu_bwd(y, da, gamma, beta, st, dy2, None, None, None, region=case.region, ws=ws)
        assert torch.equal(dy1, dy2), case.id
        del y, da, dy1, dy2
        lays.append({"ws": ws, "gamma": gamma, "stats": st, "dgamma": dg2, "dbeta": db2, "dbias": dbias2, "shape": case.shape,
                     "region": case.region})
        refs.append((dg1, db1, dbias1))
    assert sorted({lay["shape"][0] for lay in lays}) == [64, 70, 96, 256]
    hip.ln_bwd_finalize(hip.ln_finalize_descs(lays))
    torch.cuda.synchronize()
    for case, lay, (dg1, db1, dbias1) in zip(L.CASES, lays, refs):
        assert torch.isfinite(dg1).all() and torch.isfinite(db1).all() and torch.isfinite(dbias1).all(), case.id
        assert torch.equal(lay["dgamma"], dg1) and torch.equal(lay["dbeta"], db1), case.id
        assert lay["dbias"] is None or torch.equal(lay["dbias"], dbias1), case.id


C3_RTOL = 5e-6      # tests/test_kernels_gpu.py test_conv1_1_filter_gradient_fused_with_layernorm_backward


def test_reductions_only_entry_point_and_fused_conv1_1_gradient(hip, ref):
    """2d.  sgg_layernorm_hwc_elu_bwd_sums and ln_bwd_means_kernel with G * cpg = 24 chunks per sample at B = 70, and their consumer
    sgg_conv2d_nhwc_wgrad_c3_ln (conv1_1's filter gradient with the LayerNorm backward's apply pass inside), which had not run above
    B = 4: the workspace is byte-equal to sgg_layernorm_hwc_elu_bwd's, the published means reproduce the apply pass's dy, and the
    filter gradient holds the fp64 chain ln_elu_bwd -> conv_wgrad over 70 * 54 * 54 = 204 120 positions at the 5e-6 of the B <= 4
    test (measured: 1.25e-4 on max|ref| 556 = 2.3e-7)."""
    case = L.BY_ID[L.FUSED_C3_CASE]
    pin_geometry(hip, case)
    B, H, W, C = case.shape
    assert C == 32 and case.region is None
    r = references(case, ref)
    y, da, gamma, beta = inputs(case)
    x = rnd((B, H, W, 3), 1)
    dw_ref = torch.empty((3, 3, 3, 32), dtype=torch.float64)
    ref.conv_wgrad(x.double(), r["dy"], dw_ref, 1)
    xd, yd, dad, gd, bd = (t.cuda() for t in (x, y, da, gamma, beta))
    a, st = torch.empty(case.shape, device="cuda"), torch.empty((B, 2), device="cuda")
    hip.ln_elu_fwd(yd, gd, bd, a, st)
    ws = torch.zeros(hip.ln_workspace_bytes(case.shape), dtype=torch.uint8, device="cuda")      # (zeroed: compared as a whole below)
    means = torch.full((B, 2), float("nan"), device="cuda")
    hip.ln_elu_bwd_sums(yd, dad, gd, bd, st, means, ws)
    ws2 = torch.zeros_like(ws)
    dy = torch.empty(case.shape, device="cuda")
    hip.ln_elu_bwd(yd, dad, gd, bd, st, dy, None, None, None, ws=ws2)
    assert torch.equal(ws, ws2), "the partial sums of the reductions-only entry point differ from sgg_layernorm_hwc_elu_bwd's"
    assert bool((ws.view(torch.float32)[B * case.G * L.TS:B * case.G * (L.TS + 2 + 3 * C)] != 0).any())
    # the per-sample means are what the apply pass derives: dy recomputed on the host from them equals the apply pass's dy
    m, s = means.cpu().double(), st.cpu().double()
    xh = (y.double() - s[:, 0].view(B, 1, 1, 1)) * s[:, 1].view(B, 1, 1, 1)
    n = xh * gamma.double() + beta.double()
    dn = da.double() * torch.where(n > 0, torch.ones_like(n), torch.exp(n))
    dy_host = s[:, 1].view(B, 1, 1, 1) * (dn * gamma.double() - m[:, 0].view(B, 1, 1, 1) - xh * m[:, 1].view(B, 1, 1, 1))
    close(dy, dy_host, rtol=5e-6, what="dy from the published means vs the apply pass")
    close(dy, r["dy"], rtol=5e-5, what="dy vs fp64")
    # the fused filter gradient
    dw = torch.full((3, 3, 3, 32), float("nan"), device="cuda")
    hip.conv_c3_wgrad_ln(xd, yd, dad, gd, bd, st, means, dw)
    close(dw, dw_ref, rtol=C3_RTOL, what="fused conv1_1 filter gradient vs fp64 (B = 70)")
    dw2 = torch.empty_like(dw)
    hip.conv_c3_wgrad_ln(xd, yd, dad, gd, bd, st, means, dw2)
    assert torch.equal(dw, dw2), "two launches on the same operands differ"
