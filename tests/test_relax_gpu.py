"""-m gpu: the relaxed generator output - the kernels of csrc/relax.hip (HipKernels.relax_rows, relax_rows_bwd) against the numpy fp64
restatement of tests/relax_ref.py, and GanStep.set_relaxation / train.py --generator_output against autograd on the CPU oracle composed
with the relaxation (tests/test_relax_cpu.py).

Both kernels have two paths (csrc/relax.hip): rows of V <= 1024 live in the registers of one wave (one row per workgroup up to
R = 1024 rows, four above), longer rows are streamed by one 1024-thread workgroup with 16-byte accesses on the aligned body of the row
and 4-byte accesses in front of and behind it; a pass whose rows sit differently against a 16-byte boundary is scalar.  RELAX_CASES
holds the issue's shapes: both sides of the wave width, of the row count at which a workgroup takes four rows, of the resident /
streaming threshold, rows aligned differently, two sweeps of the streaming workgroup and a large V.  Every case runs at tau 1.0 and
0.25, in both modes, in place and out of place, the backward with dx on dy and apart."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd.step import GanStep
from tests import relax_ref as RR
from tests.relax_ref import RELAX_GRAD_TOL, RELAX_TOL
from tests.test_relax_cpu import SEED, oracle_d_cost, oracle_g_cost
from tests.test_step_gpu import check_weights_after_adam, tensor_err
from tests.test_xent_gpu import F32, SENT, assert_rows_guard, rows_view, u32
from tests.tolerances import GRAD_RTOL, loss_tol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -23

#              R, V,     ldx,   ldy,   sx, sy
RELAX_CASES = [(6, 11, 11, 11, 0, 0), (1, 1, 1, 1, 0, 0), (7, 1000, 1000, 1000, 0, 0),
               (9, 64, 64, 70, 1, 0), (5, 65, 67, 65, 0, 3),                    # the wave width
               (1025, 7, 8, 7, 1, 0),                                            # many rows: four per workgroup
               (5, 1024, 1024, 1030, 2, 1), (6, 1025, 1025, 1025, 0, 0),         # the resident / streaming threshold
               (6, 1027, 1027, 1028, 3, 0),                                      # rows aligned differently: the 4-byte pass 2
               (6, 5125, 5125, 5125, 2, 2),                                      # two sweeps of the streaming workgroup
               (3, 70001, 70001, 70001, 0, 0)]                                   # large V
TAUS = (1.0, 0.25)
_cases = {}


def relax_case(case, tau, gumbel):
    """(x float32 [R, V], dy float32 [R, V], y64, u64 or None); once per (case, tau, mode).  Row 3 holds equal logits, row 4 one
    logit far above the rest (a saturated row); the rest random."""
    key = (case, tau, gumbel)
    if key not in _cases:
        R, V = case[0], case[1]
        g = np.random.RandomState(9000 + R + V)
        x = (4.0 * g.standard_normal((R, V))).astype(np.float32)
        if R > 3:
            x[3] = 0.5
        if R > 4:
            x[4, V // 3] = 22.0
        assert float(np.abs(x).max()) <= 23.0
        dy = g.standard_normal((R, V)).astype(np.float32)
        y64, u64 = RR.relax_rows(x, tau, gumbel, SEED, 77 + R)
        _cases[key] = (x, dy, y64, u64)
    return _cases[key]


def on_device(a, R, V, ld, shift, fill):
    big, view = rows_view(R, V, ld, shift, fill)
    if a is not None:
        view.copy_(torch.from_numpy(a).cuda())
    return big, view


def run_case(hip, case, tau, gumbel):
    """Every launch of one (case, tau, mode) with its exact assertions; returns (max |y - y64|, max |dx - dx64| in units of
    max|dy| * scale / tau) for the caller to compare with the tolerances."""
    R, V, ldx, ldy, sx, sy = case
    x, dy, y64, u64 = relax_case(case, tau, gumbel)
    kw = {"gumbel": gumbel, "seed": SEED, "draw": 77 + R}
    # ---- forward, out of place ---------------------------------------------------------------------------------------------------
    bx, xv = on_device(x, R, V, ldx, sx, float("nan"))
    by, yv = on_device(None, R, V, ldy, sy, SENT[F32])
    bu, uv = on_device(None, R, V, ldy, sy, SENT[F32]) if gumbel else (None, None)
    hip.relax_rows(xv, tau, y=yv, u_out=uv, **kw)
    torch.cuda.synchronize()
    assert_rows_guard(by, R, V, ldy, sy, "y")
    assert np.array_equal(u32(xv.contiguous()), x.view(np.uint32)), "x was written"
    if gumbel:
        assert_rows_guard(bu, R, V, ldy, sy, "u_out")
        assert np.array_equal(uv.cpu().numpy().astype(np.float64), u64), "u differs from the restatement's Philox"
    y = yv.cpu().numpy()
    err_f = float(np.abs(y - y64).max())
    assert np.isfinite(y).all() and float(y.min()) >= 0.0 and float(np.abs(y.astype(np.float64).sum(axis=1) - 1.0).max()) <= max(V, 8) * EPS32
    # ---- two launches: equal bits; in place on x (same place, same stride): the bits of the launch out of place -------------------------
    by2, yv2 = on_device(None, R, V, ldy, sy, SENT[F32])
    hip.relax_rows(xv, tau, y=yv2, **kw)
    bi, xi = on_device(x, R, V, ldx, sx, SENT[F32])
    assert hip.relax_rows(xi, tau, **kw) is xi
    torch.cuda.synchronize()
    assert np.array_equal(u32(yv2.contiguous()), u32(yv.contiguous())), "y differs between two launches"
    assert_rows_guard(bi, R, V, ldx, sx, "y in place")
    assert np.array_equal(u32(xi.contiguous()), u32(yv.contiguous())), "in place differs from out of place"
    # ---- backward: y as the device made it (rows ldy, sy), dy in rows (ldx, sx), dx apart (rows ldy, sy) and on dy ------------------
    scale = 0.37
    dx64 = RR.relax_rows_bwd(y, dy, tau, scale)
    unit = float(np.abs(dy).max()) * scale / tau
    bg, gv = on_device(dy, R, V, ldx, sx, float("nan"))
    bd, dv = on_device(None, R, V, ldy, sy, SENT[F32])
    hip.relax_rows_bwd(yv, gv, tau, scale=scale, dx=dv)
    torch.cuda.synchronize()
    assert_rows_guard(bd, R, V, ldy, sy, "dx")
    assert np.array_equal(u32(gv.contiguous()), dy.view(np.uint32)) and np.array_equal(u32(yv.contiguous()), y.view(np.uint32))
    dx = dv.cpu().numpy()
    err_b = float(np.abs(dx - dx64).max()) / unit
    ba, ga = on_device(dy, R, V, ldx, sx, SENT[F32])
    assert hip.relax_rows_bwd(yv, ga, tau, scale=scale) is ga
    bd2, dv2 = on_device(None, R, V, ldy, sy, SENT[F32])
    hip.relax_rows_bwd(yv, gv, tau, scale=scale, dx=dv2)
    torch.cuda.synchronize()
    assert_rows_guard(ba, R, V, ldx, sx, "dx on dy")
    assert np.array_equal(u32(ga.contiguous()), u32(dv.contiguous())), "dx on dy differs from dx apart"
    assert np.array_equal(u32(dv2.contiguous()), u32(dv.contiguous())), "dx differs between two launches"
    return err_f, err_b


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("case", RELAX_CASES, ids=["R%d-V%d-ldx%d-ldy%d-sx%d-sy%d" % c for c in RELAX_CASES])
def test_relax_rows_match_fp64_restatement(hip, case, tau, gumbel):
    err_f, err_b = run_case(hip, case, tau, gumbel)
    print("relax_rows R %d V %d tau %g gumbel %d: max |y - y64| %.3e   max |dx - dx64| / (max|dy| scale / tau) %.3e"
          % (case[0], case[1], tau, gumbel, err_f, err_b))
    assert err_f <= RELAX_TOL and err_b <= RELAX_GRAD_TOL


DX_APART_CASE = (2, 1027, 1028, 1028, 0, 0)         # both inputs of a backward in rows of 1028 on a 16-byte boundary ...
DX_APART_SHIFT, DX_APART_TAU = 1, 0.25             # ... and dx in rows of 1028 one element behind one


def check_dx_apart(launch, dx64, unit, tol):
    """launch(dx) of a streaming backward whose inputs sit alike against 16 bytes (pass 1 on 16-byte loads), with dx one element off
    (pass 2 on 4-byte accesses) and with dx laid out like the inputs: the guard words around dx, the restatement, equal bits."""
    R, V, ld = DX_APART_CASE[:3]
    bd, dv = on_device(None, R, V, ld, DX_APART_SHIFT, SENT[F32])
    bl, dl = on_device(None, R, V, ld, 0, SENT[F32])
    launch(dv)
    launch(dl)
    torch.cuda.synchronize()
    assert_rows_guard(bd, R, V, ld, DX_APART_SHIFT, "dx")
    assert_rows_guard(bl, R, V, ld, 0, "dx like the inputs")
    err = float(np.abs(dv.cpu().numpy() - dx64).max()) / unit
    print("dx one element off the inputs' alignment: max |dx - dx64| / (max|dy| scale / tau) %.3e" % err)
    assert err <= tol
    assert np.array_equal(u32(dv.contiguous()), u32(dl.contiguous())), "dx off the inputs' alignment differs from dx laid out like them"


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
def test_backward_with_dx_alone_off_the_inputs_alignment(hip, gumbel):
    R, V, ld = DX_APART_CASE[:3]
    tau, scale = DX_APART_TAU, 0.37
    x, dy, _, _ = relax_case(DX_APART_CASE, tau, gumbel)
    _, xv = on_device(x, R, V, ld, 0, float("nan"))
    _, yv = on_device(None, R, V, ld, 0, SENT[F32])
    _, gv = on_device(dy, R, V, ld, 0, float("nan"))
    hip.relax_rows(xv, tau, y=yv, gumbel=gumbel, seed=SEED, draw=77 + R)
    check_dx_apart(lambda dx: hip.relax_rows_bwd(yv, gv, tau, scale=scale, dx=dx), RR.relax_rows_bwd(yv.cpu().numpy(), dy, tau, scale),
                   float(np.abs(dy).max()) * scale / tau, RELAX_GRAD_TOL)


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
@pytest.mark.parametrize("V,ld,sx", [(11, 11, 0), (1000, 1001, 1), (70001, 70001, 3)])
def test_rows_of_plus_minus_80_at_tau_0p1_do_not_overflow(hip, V, ld, sx, gumbel):
    """z = +-800: exp(z) overflows fp32, only the stabilised form is finite; every row still sums to 1."""
    R = 2
    x = np.empty((R, V), dtype=np.float32)
    x[0] = np.where(np.arange(V) % 2 == 0, 80.0, -80.0)
    x[1] = np.where(np.arange(V) % 3 == 0, -80.0, 80.0)
    bx, xv = on_device(x, R, V, ld, sx, float("nan"))
    by, yv = on_device(None, R, V, ld, sx, SENT[F32])
    hip.relax_rows(xv, 0.1, y=yv, gumbel=gumbel, seed=SEED, draw=5)
    torch.cuda.synchronize()
    assert_rows_guard(by, R, V, ld, sx, "y")
    y = yv.cpu().numpy()
    assert np.isfinite(y).all() and float(y.min()) >= 0.0
    assert float(np.abs(y.astype(np.float64).sum(axis=1) - 1.0).max()) <= V * EPS32
    if not gumbel:
        ref, _ = RR.relax_rows(x, 0.1)
        assert float(np.abs(y - ref).max()) <= RELAX_TOL
    dy = np.random.RandomState(2).standard_normal((R, V)).astype(np.float32)
    dx = hip.relax_rows_bwd(yv, torch.from_numpy(dy).cuda(), 0.1).cpu().numpy()
    assert np.isfinite(dx).all()
    assert float(np.abs(dx - RR.relax_rows_bwd(y, dy, 0.1)).max()) <= RELAX_GRAD_TOL * float(np.abs(dy).max()) / 0.1


def test_bad_arguments_are_refused_and_nothing_is_written(hip):
    from sgg_amd.lib import SggError
    R, V = 3, 5
    x = torch.zeros(R, V, device="cuda")
    by, y = on_device(None, R, V, V, 0, SENT[F32])
    bd, d = on_device(None, R, V, V, 0, SENT[F32])
    dy = torch.ones(R, V, device="cuda")
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(SggError, match="tau"):
            hip.relax_rows(x, tau, y=y)
        with pytest.raises(SggError, match="tau"):
            hip.relax_rows_bwd(x, dy, tau, dx=d)
    # y on x with another row stride; dx on dy with another row stride; dx on y
    wide = torch.zeros(R * (V + 1), device="cuda")
    xa, ya = wide.as_strided((R, V), (V + 1, 1), 0), wide.as_strided((R, V), (V, 1), 0)
    with pytest.raises(SggError, match="aliasing"):
        hip.relax_rows(xa, 1.0, y=ya)
    with pytest.raises(SggError, match="aliasing"):
        hip.relax_rows_bwd(x, xa, 1.0, dx=ya)
    with pytest.raises(SggError, match="alias"):
        hip.relax_rows_bwd(x, dy, 1.0, dx=x)
    # u_out without noise
    with pytest.raises(SggError, match="u_out"):
        hip.relax_rows(x, 1.0, y=y, u_out=d)
    # shapes and pointers the binding cannot produce: the C entry points themselves
    lib, st = hip.lib, hip._stream()
    big = (1 << 21) + 1
    for rc in (lib.sgg_relax_rows(x.data_ptr(), V, R, 0, 1.0, 0, 0, 0, y.data_ptr(), V, None, 0, st),
               lib.sgg_relax_rows(x.data_ptr(), big, 1, big, 1.0, 0, 0, 0, y.data_ptr(), big, None, 0, st),
               lib.sgg_relax_rows(x.data_ptr(), V, 0, V, 1.0, 0, 0, 0, y.data_ptr(), V, None, 0, st),
               lib.sgg_relax_rows(x.data_ptr(), V - 1, R, V, 1.0, 0, 0, 0, y.data_ptr(), V, None, 0, st),
               lib.sgg_relax_rows(None, V, R, V, 1.0, 0, 0, 0, y.data_ptr(), V, None, 0, st),
               lib.sgg_relax_rows(x.data_ptr(), V, R, V, 1.0, 0, 0, 0, None, V, None, 0, st),
               lib.sgg_relax_rows(x.data_ptr(), V, R, V, 1.0, 2, 0, 0, y.data_ptr(), V, None, 0, st),
               lib.sgg_relax_rows_bwd(x.data_ptr(), V, dy.data_ptr(), V, R, 0, 1.0, 1.0, d.data_ptr(), V, st),
               lib.sgg_relax_rows_bwd(x.data_ptr(), big, dy.data_ptr(), big, 1, big, 1.0, 1.0, d.data_ptr(), big, st),
               lib.sgg_relax_rows_bwd(None, V, dy.data_ptr(), V, R, V, 1.0, 1.0, d.data_ptr(), V, st),
               lib.sgg_relax_rows_bwd(x.data_ptr(), V, None, V, R, V, 1.0, 1.0, d.data_ptr(), V, st),
               lib.sgg_relax_rows_bwd(x.data_ptr(), V, dy.data_ptr(), V, R, V, 1.0, 1.0, None, V, st),
               lib.sgg_relax_rows_bwd(x.data_ptr(), V, dy.data_ptr(), V, R, V, 1.0, float("nan"), d.data_ptr(), V, st)):
        assert rc == -1 and b"sgg_relax_rows" in lib.sgg_last_error()
    torch.cuda.synchronize()
    for b in (by, bd):
        assert (b.cpu().numpy() == SENT[F32]).all(), "a refused call wrote something"
    assert float(wide.abs().max()) == 0.0 and float(x.abs().max()) == 0.0


# ---- the step ------------------------------------------------------------------------------------------------------------------
B, S, V = 8, 64, 50
STEP_TAU = 0.5


def _setup():
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    dp["W"] = dp["W"] * 25.0
    return gp, dp


def _arenas(gs):
    gs.flush()
    torch.cuda.synchronize()
    return {n + k: t.clone() for n, net in (("G", gs.G), ("D", gs.D))
            for k, t in ((".p", net.arena.flat), (".g", net.grad_flat), (".m", net.m_flat), (".v", net.v_flat))}


@pytest.mark.parametrize("mode", ["softmax", "gumbel"])
def test_generator_step_matches_oracle_through_the_relaxation(hip, mode):
    gp, dp = _setup()
    gp0 = {k: v.clone() for k, v in gp.items()}
    images, labels, _ = O.synth_batch(B, S, V)
    noise = O.synth_noise(B, 1)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    gs.set_relaxation(mode, STEP_TAU, SEED)
    cost, grads = oracle_g_cost(gp, dp, images, noise, mode, STEP_TAU, SEED, 41)
    gl = gs.generator_step(images.cuda(), noise.cuda(), draw=41).cpu()
    assert abs(-float(gl[3]) - float(cost)) <= loss_tol(cost), (gl, cost)
    worst = max((tensor_err(gs.G.grads[n], g), n) for n, g in grads.items())
    print("generator_step(%s, tau %g) gradients: worst rel err %.3e (%s)" % (mode, STEP_TAU, worst[0], worst[1]))
    assert worst[0] < GRAD_RTOL, "generator gradient %s: rel err %.3e" % (worst[1], worst[0])
    g_adam = O.new_adam_state(gp)
    O.tf_adam_step(gp, grads, g_adam[0], g_adam[1], 1)
    gs.flush()
    check_weights_after_adam(gs.G.arena.views, gp, grads, gp0, 1, "generator (%s)" % mode)
    # the relaxation is in the gradient: without it the decoder bias gradient is far outside the tolerance (the oracle alone says
    # so as well: tests/test_relax_cpu.py::test_the_relaxation_moves_the_oracles_gradient)
    plain = GanStep(hip, V, S, B, lam=10.0, g_state=gp0, d_state=dp)
    plain.generator_step(images.cuda(), noise.cuda())
    assert tensor_err(plain.G.grads["decoder/bias"], grads["decoder/bias"]) > 100 * GRAD_RTOL
    # the likelihood term still adds to the result: a function of the logits
    both = GanStep(hip, V, S, B, lam=10.0, g_state=gp0, d_state=dp)
    both.set_relaxation(mode, STEP_TAU, SEED)
    _, grads_w = oracle_g_cost(gp0, dp, images, noise, mode, STEP_TAU, SEED, 41, labels, 0.3)
    both.generator_step(images.cuda(), noise.cuda(), draw=41, labels=labels.cuda(), mle_weight=0.3)
    worst = max((tensor_err(both.G.grads[n], g), n) for n, g in grads_w.items())
    assert worst[0] < GRAD_RTOL, "generator gradient with mle_weight %s: rel err %.3e" % (worst[1], worst[0])


@pytest.mark.parametrize("mode", ["softmax", "gumbel"])
def test_critic_step_matches_oracle_on_the_relaxed_fake(hip, mode):
    gp, dp = _setup()
    dp0 = {k: v.clone() for k, v in dp.items()}
    images, labels, onehot = O.synth_batch(B, S, V)
    noise, alpha = O.synth_noise(B, 0), O.synth_alpha(B, 0)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    gs.set_relaxation(mode, STEP_TAU, SEED)
    cost, aux, grads = oracle_d_cost(gp, dp, images, onehot, noise, alpha, 10.0, mode, STEP_TAU, SEED, 7)
    grads = {n: g for n, g in grads.items() if g is not None and n != "decoder/bias"}      # (decoder/bias cancels: tests/test_step_gpu.py)
    args = (images.cuda(), labels.cuda(), noise.cuda(), alpha.reshape(B).cuda())
    val = gs.critic_loss(*args, draw=7).cpu()
    dl = gs.critic_step(*args, draw=7).cpu()
    print("critic_step(%s): disc_cost %.6f (oracle %.6f), gp %.6f (oracle %.6f)" % (mode, float(dl[0]), float(cost), float(dl[2]), float(aux["gp"])))
    assert abs(float(dl[0]) - float(cost)) <= loss_tol(cost) and abs(float(val[0]) - float(cost)) <= loss_tol(cost)
    assert abs(float(dl[2]) - float(aux["gp"])) <= 1e-5 + 1e-4 * abs(float(aux["gp"]))
    fake_rows = gs.TRI[:B].cpu()
    assert float((fake_rows.double().sum(dim=-1) - 1.0).abs().max()) <= V * EPS32 and float(fake_rows.min()) >= 0.0
    worst = max((tensor_err(gs.D.grads[n], g), n) for n, g in grads.items())
    print("critic_step(%s) gradients: worst rel err %.3e (%s)" % (mode, worst[0], worst[1]))
    assert worst[0] < GRAD_RTOL, "critic gradient %s: rel err %.3e" % (worst[1], worst[0])
    d_adam = O.new_adam_state(dp)
    O.tf_adam_step(dp, grads, d_adam[0], d_adam[1], 1)
    gs.flush()
    check_weights_after_adam(gs.D.arena.views, dp, grads, dp0, 1, "critic (%s)" % mode)


def _iteration(gs, img, lab, **kw):
    gs.train_iteration(img, lab, [O.synth_noise(gs.B, i).cuda() for i in range(3)],
                       [O.synth_alpha(gs.B, i).reshape(gs.B).cuda() for i in range(2)], critic_iters=2, **kw)


def test_mode_logits_is_the_step_without_the_option_bit_for_bit(hip):
    gp, dp = _setup()
    images, labels, _ = O.synth_batch(B, S, V)
    img, lab = images.cuda(), labels.cuda()
    res = []
    for setup in (lambda gs: None, lambda gs: gs.set_relaxation("logits"),
                  lambda gs: (gs.set_relaxation("gumbel", 0.5, 3), gs.set_relaxation("logits", 0.5, 3))):
        gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
        setup(gs)
        _iteration(gs, img, lab, **({"draws": [4, 5, 6]} if res else {}))
        res.append(_arenas(gs))
        res[-1]["losses"] = torch.cat([gs.d_losses, gs.g_losses]).clone()
    for other in res[1:]:
        for k in res[0]:
            assert torch.equal(res[0][k].view(torch.int32), other[k].view(torch.int32)), k


@pytest.mark.parametrize("mode", ["softmax", "gumbel"])
def test_relaxed_iteration_two_stream_equals_serial(hip, mode):
    Bs, Ss, Vs = 2, 32, 11
    images, labels, _ = O.synth_batch(Bs, Ss, Vs)
    img, lab = images.cuda(), labels.cuda()
    res = {}
    for overlap in (False, True):
        gp, dp = O.init_params("G", Vs, Ss, perturb=0.05), O.init_params("D", Vs, Ss, perturb=0.05)
        dp["W"] = dp["W"] * 25.0
        gs = GanStep(hip, Vs, Ss, Bs, lam=10.0, g_state=gp, d_state=dp, overlap_streams=overlap)
        gs.set_relaxation(mode, STEP_TAU, SEED)
        for it in range(2):
            _iteration(gs, img, lab, draws=[10 * it, 10 * it + 1, 10 * it + 2])
        res[overlap] = _arenas(gs)
    for k in res[False]:
        assert torch.equal(res[False][k].view(torch.int32), res[True][k].view(torch.int32)), "%s differs between the schedules" % k


def test_test_only_on_a_relaxed_checkpoint_scores_softmax_of_the_logits(tmp_path):
    """A relaxed synthetic checkpoint, then train.py --test_only in a fresh child process without the flags: the mode comes from
    the checkpoint, recalls.txt is what test() gives in-process, and the scores are the critic's on softmax(logits / tau) - against
    the oracle's critic in fp64 on the device's logits, within the score tolerance of tests/test_eval_batched_gpu.py."""
    import train as T
    from tests.test_eval_batched_gpu import _oracle_per_image
    Bc, Sc, Vc = 8, 64, 50
    mk = lambda **kw: T.SceneGraphGAN(str(tmp_path / "ck"), str(tmp_path / "logs"), None, None, None, None, None, critic_iters=1, batch_size=Bc,
                                      lambda_=10, synthetic=(Bc, Sc, Vc), **kw)
    gan = mk(resume=False, generator_output="gumbel", relax_tau="0.5,0.25,1")
    gan.train(max_iterations=1, log_every=1, test_at_end=False)
    rec = [json.loads(l) for l in open(str(tmp_path / "logs" / "losses.jsonl")) if l.strip()]
    assert rec[0]["relax"] == {"mode": "gumbel", "tau": 0.5}
    out = tmp_path / "eval"
    out.mkdir()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1",
                        "--checkpoints_dir", str(tmp_path / "ck"), "--summaries_dir", str(tmp_path / "logs"), "--test_only",
                        "--max_test_images", "2"], cwd=str(out), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = (out / "recalls.txt").read_text()
    assert '# generator_output: {"mode": "gumbel", "tau": 0.25}' in got
    ev = mk(resume=False)
    assert ev.load_checkpoint() and ev.relax_mode == "gumbel" and ev._eval_relax() == 0.25
    _, details = ev.test(max_images=2, out_path=str(tmp_path / "inproc.txt"), return_details=True)
    assert got == (tmp_path / "inproc.txt").read_text()
    # the second score_samples site: evaluate() labels its JSON (K-best decoding does not run the critic: no label)
    met = ev.evaluate(max_images=2, ks=(1, 5), out_path=str(tmp_path / "m.json"))
    assert met["generator_output"] == {"mode": "gumbel", "tau": 0.25} and json.load(open(str(tmp_path / "m.json")))["generator_output"] == met["generator_output"]
    assert "generator_output" not in ev.evaluate(max_images=2, ks=(1, 5), decode="kbest")
    # a contradicting flag is refused before anything is loaded
    with pytest.raises(ValueError, match="contradicts"):
        mk(resume=False, generator_output="softmax").load_checkpoint()
    # the reference path: the items and noise stream of test(), G's logits from the device, the oracle's critic in fp64 on their softmax
    g = torch.Generator().manual_seed(ev.seed + 99)
    items = [(torch.randn((Sc, Sc, 3), generator=g), torch.randint(0, Vc, (5, 3), generator=g).tolist()) for _ in range(2)]
    TB, n_samples = ev.TEST_BATCH_SIZE, ev.TEST_BATCH_MULTIPLIER * ev.TEST_BATCH_SIZE
    gen = torch.Generator().manual_seed(ev.seed + 123)
    noise = torch.zeros((n_samples, 2, 512))
    for j in range(2):
        for p in range(ev.TEST_BATCH_MULTIPLIER):
            noise[p * TB:(p + 1) * TB, j] = torch.randn((TB, 512), generator=gen)
    images = torch.stack([im for im, _ in items])
    logits = ev.g.sample(images.cuda(), n_samples, noise.cuda()).cpu().double()
    dp64 = {k: v.double() for k, v in ev.d.state_dict(full_names=False).items()}
    y = torch.softmax(logits / 0.25, dim=-1)
    ref = _oracle_per_image(O.discriminator_head, dp64, images.double(), [y[:, b] for b in range(2)]).mean(dim=2).reshape(n_samples, 2)
    for j in range(2):
        err = float(np.abs(details[j]["scores"] - ref[:, j].numpy()).max())
        print("image %d: max |score - fp64 reference| %.3e" % (j, err))
        assert err <= 1e-4 + 1e-4 * float(ref.abs().max())
        assert np.array_equal(details[j]["tokens"], O.argmax_tokens(logits[:, j]).numpy()), "the reported tokens are argmax(logits)"
