"""-m gpu: the straight-through (hard) relaxation - the kernels behind HipKernels.relax_rows_hard / relax_rows_hard_bwd (csrc/relax.hip)
against the numpy fp64 restatement of tests/relax_hard_ref.py, and GanStep.set_relaxation(hard=True) / train.py --relax_hard against
autograd on the CPU oracle composed with y_hard + y_soft - y_soft.detach() (tests/test_relax_hard_cpu.py).

The shapes, inputs, seed and draws are those of tests/test_relax_gpu.py (RELAX_CASES, relax_case, SEED, draw 77 + R): both sides of the
wave width, 1025 rows of 7 (four rows per workgroup), the resident / streaming threshold, rows aligned differently, two sweeps of the
streaming workgroup and V = 70 001 (the four-loads-in-flight loop of pass 1)."""
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
from tests import relax_hard_ref as HR
from tests.relax_hard_ref import HARD_GRAD_TOL, HARD_MARGIN_MIN
from tests.test_relax_cpu import SEED
from tests.test_relax_gpu import (DX_APART_CASE, DX_APART_TAU, RELAX_CASES, TAUS, _arenas, _iteration, _setup, check_dx_apart, on_device,
                                  relax_case)
from tests.test_relax_hard_cpu import oracle_d_cost_hard, oracle_g_cost_hard
from tests.test_step_gpu import check_weights_after_adam, tensor_err
from tests.test_xent_gpu import F32, SENT, assert_rows_guard, u32
from tests.tolerances import GRAD_RTOL, loss_tol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["R%d-V%d-ldx%d-ldy%d-sx%d-sy%d" % c for c in RELAX_CASES]
ONE, ZERO = 0x3F800000, 0x00000000                        # the bits of 1.0f and +0.0f
_hard = {}


def hard_ref(case, gumbel):
    """(y64, tok, margin) of the restatement on relax_case's x; once per (case, mode)."""
    key = (case, gumbel)
    if key not in _hard:
        _hard[key] = HR.relax_rows_hard(relax_case(case, 1.0, gumbel)[0], gumbel, SEED, 77 + case[0])
    return _hard[key]


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
@pytest.mark.parametrize("case", RELAX_CASES, ids=IDS)
def test_hard_rows_are_one_hot_at_the_restatements_token(hip, case, gumbel):
    R, V, ldx, ldy, sx, sy = case
    x = relax_case(case, 1.0, gumbel)[0]
    _, tok64, margin = hard_ref(case, gumbel)
    kw = {"gumbel": gumbel, "seed": SEED, "draw": 77 + R}
    bx, xv = on_device(x, R, V, ldx, sx, float("nan"))
    by, yv = on_device(None, R, V, ldy, sy, SENT[F32])
    tok = torch.full((R,), -5, dtype=torch.int64, device="cuda")
    hip.relax_rows_hard(xv, y=yv, tok=tok, **kw)
    torch.cuda.synchronize()
    assert_rows_guard(by, R, V, ldy, sy, "y")
    assert np.array_equal(u32(xv.contiguous()), x.view(np.uint32)), "x was written"
    t = tok.cpu().numpy()
    bits = u32(yv.contiguous())
    want = np.full((R, V), ZERO, dtype=np.uint32)
    want[np.arange(R), t] = ONE
    assert np.array_equal(bits, want), "a row is not bitwise one 1.0f at tok and V - 1 +0.0f"
    # the token: every row, none left out
    if gumbel:
        print("hard rows R %d V %d: smallest top-2 gap of x + g %.3e" % (R, V, float(margin.min())))
        assert float(margin.min()) >= HARD_MARGIN_MIN, "the restatement's margin does not separate fp32 from fp64 on every row"
        assert np.array_equal(t, tok64), "tok differs from the fp64 restatement's argmax of x + g"
    else:
        assert np.array_equal(t, x.argmax(axis=1)), "tok is not the first argmax of x"
        assert R <= 3 or t[3] == 0, "a row of equal logits gives index 0"
        am = torch.full((R,), -5, dtype=torch.int64, device="cuda")
        hip.argmax_rows(xv, am)
        assert torch.equal(am, tok), "tok differs from argmax_rows"
    # two launches: equal bits; in place on x: the bits of the launch out of place; tok alone and y alone agree
    by2, yv2 = on_device(None, R, V, ldy, sy, SENT[F32])
    tok2 = torch.full((R,), -5, dtype=torch.int64, device="cuda")
    hip.relax_rows_hard(xv, y=yv2, tok=tok2, **kw)
    bi, xi = on_device(x, R, V, ldx, sx, SENT[F32])
    assert hip.relax_rows_hard(xi, **kw)[0] is xi
    tok3 = torch.full((R,), -5, dtype=torch.int64, device="cuda")
    hip.relax_rows_hard(xv, tok=tok3, **kw)
    by4, yv4 = on_device(None, R, V, ldy, sy, SENT[F32])
    hip.relax_rows_hard(xv, y=yv4, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(u32(yv2.contiguous()), bits) and torch.equal(tok2, tok), "two launches differ"
    assert_rows_guard(bi, R, V, ldx, sx, "y in place")
    assert np.array_equal(u32(xi.contiguous()), bits), "in place differs from out of place"
    assert torch.equal(tok3, tok), "tok alone differs"
    assert_rows_guard(by4, R, V, ldy, sy, "y alone")
    assert np.array_equal(u32(yv4.contiguous()), bits), "y alone differs"
    assert np.array_equal(u32(xv.contiguous()), x.view(np.uint32)), "x was written"


def run_bwd(hip, case, tau, gumbel):
    """Every backward launch of one (case, tau, mode) with its exact assertions; returns (max |dx - dx64|, max |dx - the device's
    relax_rows_bwd(relax_rows(x), dy)|), both in units of max|dy| * scale / tau."""
    R, V, ldx, ldy, sx, sy = case
    x, dy, _, _ = relax_case(case, tau, gumbel)
    kw = {"gumbel": gumbel, "seed": SEED, "draw": 77 + R}
    scale = 0.37
    unit = float(np.abs(dy).max()) * scale / tau
    dx64 = HR.relax_rows_hard_bwd(x, dy, tau, scale, gumbel, SEED, 77 + R)
    # x in rows (ldx, sx), dy in rows (ldy, sy), dx apart in rows (ldx, sx) and on dy
    bx, xv = on_device(x, R, V, ldx, sx, float("nan"))
    bg, gv = on_device(dy, R, V, ldy, sy, float("nan"))
    bd, dv = on_device(None, R, V, ldx, sx, SENT[F32])
    hip.relax_rows_hard_bwd(xv, gv, tau, scale=scale, dx=dv, **kw)
    torch.cuda.synchronize()
    assert_rows_guard(bd, R, V, ldx, sx, "dx")
    assert np.array_equal(u32(xv.contiguous()), x.view(np.uint32)) and np.array_equal(u32(gv.contiguous()), dy.view(np.uint32))
    dx = dv.cpu().numpy()
    assert np.isfinite(dx).all()
    err = float(np.abs(dx - dx64).max()) / unit
    ba, ga = on_device(dy, R, V, ldy, sy, SENT[F32])
    assert hip.relax_rows_hard_bwd(xv, ga, tau, scale=scale, **kw) is ga
    bd2, dv2 = on_device(None, R, V, ldx, sx, SENT[F32])
    hip.relax_rows_hard_bwd(xv, gv, tau, scale=scale, dx=dv2, **kw)
    # the soft pair on the device: y = relax_rows(x), then relax_rows_bwd(y, dy)
    ys = torch.empty(R, V, device="cuda")
    hip.relax_rows(xv, tau, y=ys, **kw)
    soft = hip.relax_rows_bwd(ys, gv, tau, scale=scale, dx=torch.empty(R, V, device="cuda")).cpu().numpy()
    torch.cuda.synchronize()
    assert_rows_guard(ba, R, V, ldy, sy, "dx on dy")
    assert np.array_equal(u32(ga.contiguous()), u32(dv.contiguous())), "dx on dy differs from dx apart"
    assert np.array_equal(u32(dv2.contiguous()), u32(dv.contiguous())), "dx differs between two launches"
    return err, float(np.abs(dx - soft).max()) / unit


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("case", RELAX_CASES, ids=IDS)
def test_hard_backward_matches_fp64_restatement_and_the_soft_pair(hip, case, tau, gumbel):
    err, err_soft = run_bwd(hip, case, tau, gumbel)
    print("relax_rows_hard_bwd R %d V %d tau %g gumbel %d: max |dx - dx64| %.3e   max |dx - soft pair| %.3e   (units of max|dy| scale / tau)"
          % (case[0], case[1], tau, gumbel, err, err_soft))
    assert err <= HARD_GRAD_TOL and err_soft <= 2 * HARD_GRAD_TOL


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
def test_hard_backward_with_dx_alone_off_the_inputs_alignment(hip, gumbel):
    R, V, ld = DX_APART_CASE[:3]
    tau, scale = DX_APART_TAU, 0.37
    kw = {"gumbel": gumbel, "seed": SEED, "draw": 77 + R}
    x, dy, _, _ = relax_case(DX_APART_CASE, tau, gumbel)
    _, xv = on_device(x, R, V, ld, 0, float("nan"))
    _, gv = on_device(dy, R, V, ld, 0, float("nan"))
    check_dx_apart(lambda dx: hip.relax_rows_hard_bwd(xv, gv, tau, scale=scale, dx=dx, **kw),
                   HR.relax_rows_hard_bwd(x, dy, tau, scale, gumbel, SEED, 77 + R), float(np.abs(dy).max()) * scale / tau, HARD_GRAD_TOL)


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
@pytest.mark.parametrize("V,ld,sx", [(11, 11, 0), (1000, 1001, 1), (70001, 70001, 3)])
def test_rows_of_plus_minus_80_at_tau_0p1_give_finite_gradients(hip, V, ld, sx, gumbel):
    """z = +-800: exp(z) overflows fp32, only the stabilised form is finite."""
    R = 2
    x = np.empty((R, V), dtype=np.float32)
    x[0] = np.where(np.arange(V) % 2 == 0, 80.0, -80.0)
    x[1] = np.where(np.arange(V) % 3 == 0, -80.0, 80.0)
    dy = np.random.RandomState(2).standard_normal((R, V)).astype(np.float32)
    bx, xv = on_device(x, R, V, ld, sx, float("nan"))
    bd, dv = on_device(None, R, V, ld, sx, SENT[F32])
    hip.relax_rows_hard_bwd(xv, torch.from_numpy(dy).cuda(), 0.1, gumbel=gumbel, seed=SEED, draw=5, dx=dv)
    torch.cuda.synchronize()
    assert_rows_guard(bd, R, V, ld, sx, "dx")
    dx = dv.cpu().numpy()
    assert np.isfinite(dx).all()
    if not gumbel:      # (with noise at tau 0.1 the fp32 g's error is multiplied by ten before the exp: outside this tolerance's cases)
        ref = HR.relax_rows_hard_bwd(x, dy, 0.1)
        assert float(np.abs(dx - ref).max()) <= HARD_GRAD_TOL * float(np.abs(dy).max()) / 0.1
    y, tok = hip.relax_rows_hard(xv, y=torch.empty(R, V, device="cuda"), tok=torch.empty(R, dtype=torch.int64, device="cuda"),
                                 gumbel=gumbel, seed=SEED, draw=5)
    assert float(y.sum()) == R and (gumbel or tok.tolist() == [0, 1])


def test_bad_arguments_are_refused_and_nothing_is_written(hip):
    from sgg_amd.lib import SggError
    R, V = 3, 5
    x = torch.zeros(R, V, device="cuda")
    by, y = on_device(None, R, V, V, 0, SENT[F32])
    bd, d = on_device(None, R, V, V, 0, SENT[F32])
    dy = torch.ones(R, V, device="cuda")
    tok = torch.full((R,), -5, dtype=torch.int64, device="cuda")
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(SggError, match="tau"):
            hip.relax_rows_hard_bwd(x, dy, tau, dx=d)
    with pytest.raises(SggError, match="scale"):
        hip.relax_rows_hard_bwd(x, dy, 1.0, scale=float("inf"), dx=d)
    # y on x with another row stride; dx on dy with another row stride; dx on x
    wide = torch.zeros(R * (V + 1), device="cuda")
    xa, ya = wide.as_strided((R, V), (V + 1, 1), 0), wide.as_strided((R, V), (V, 1), 0)
    with pytest.raises(SggError, match="aliasing"):
        hip.relax_rows_hard(xa, y=ya)
    with pytest.raises(SggError, match="aliasing"):
        hip.relax_rows_hard_bwd(x, xa, 1.0, dx=ya)
    with pytest.raises(SggError, match="alias"):
        hip.relax_rows_hard_bwd(x, dy, 1.0, dx=x)
    # shapes and pointers the binding cannot produce: the C entry points themselves
    lib, st = hip.lib, hip._stream()
    big = (1 << 21) + 1
    xp, yp, tp, gp_, dp_ = x.data_ptr(), y.data_ptr(), tok.data_ptr(), dy.data_ptr(), d.data_ptr()
    for rc in (lib.sgg_relax_rows_hard(xp, V, R, 0, 0, 0, 0, yp, V, tp, st),
               lib.sgg_relax_rows_hard(xp, big, 1, big, 0, 0, 0, yp, big, tp, st),
               lib.sgg_relax_rows_hard(xp, V, 0, V, 0, 0, 0, yp, V, tp, st),
               lib.sgg_relax_rows_hard(xp, V - 1, R, V, 0, 0, 0, yp, V, tp, st),
               lib.sgg_relax_rows_hard(xp, V, R, V, 0, 0, 0, yp, V - 1, tp, st),
               lib.sgg_relax_rows_hard(None, V, R, V, 0, 0, 0, yp, V, tp, st),
               lib.sgg_relax_rows_hard(xp, V, R, V, 0, 0, 0, None, V, None, st),
               lib.sgg_relax_rows_hard(xp, V, R, V, 2, 0, 0, yp, V, tp, st),
               lib.sgg_relax_rows_hard(xp, V, R, V, -1, 0, 0, yp, V, tp, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, gp_, V, R, 0, 1.0, 1.0, 0, 0, 0, dp_, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, big, gp_, big, 1, big, 1.0, 1.0, 0, 0, 0, dp_, big, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, gp_, V, 0, V, 1.0, 1.0, 0, 0, 0, dp_, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, V - 1, gp_, V, R, V, 1.0, 1.0, 0, 0, 0, dp_, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, gp_, V - 1, R, V, 1.0, 1.0, 0, 0, 0, dp_, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, gp_, V, R, V, 1.0, 1.0, 0, 0, 0, dp_, V - 1, st),
               lib.sgg_relax_rows_hard_bwd(None, V, gp_, V, R, V, 1.0, 1.0, 0, 0, 0, dp_, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, None, V, R, V, 1.0, 1.0, 0, 0, 0, dp_, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, gp_, V, R, V, 1.0, 1.0, 0, 0, 0, None, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, gp_, V, R, V, 1.0, float("nan"), 0, 0, 0, dp_, V, st),
               lib.sgg_relax_rows_hard_bwd(xp, V, gp_, V, R, V, 1.0, 1.0, 2, 0, 0, dp_, V, st)):
        assert rc == -1 and b"sgg_relax_rows_hard" in lib.sgg_last_error()
    torch.cuda.synchronize()
    for b in (by, bd):
        assert (b.cpu().numpy() == SENT[F32]).all(), "a refused call wrote something"
    assert float(wide.abs().max()) == 0.0 and float(x.abs().max()) == 0.0 and tok.tolist() == [-5] * R and float((dy - 1.0).abs().max()) == 0.0


# ---- the step ------------------------------------------------------------------------------------------------------------------
# B 8, S 64, V 50, tau 0.5 as tests/test_relax_gpu.py.  The noise vectors (synth_noise 5 for the generator update, 0 for the critic's)
# and the draws (41, 7) under SEED were chosen on the CPU oracle so that the smallest top-2 gap of x + g over the 24 rows is far
# above the fp32 difference between the device's logits and the oracle's: 2.5e-2 / 3.5e-2 (generator update: softmax / gumbel) and
# 1.3e-2 / 2.8e-2 (critic update).
B, S, V = 8, 64, 50
STEP_TAU = 0.5
G_NOISE, D_NOISE = 5, 0


@pytest.mark.parametrize("mode", ["softmax", "gumbel"])
def test_generator_step_matches_oracle_through_the_straight_through_rows(hip, mode):
    gp, dp = _setup()
    gp0 = {k: v.clone() for k, v in gp.items()}
    images, labels, _ = O.synth_batch(B, S, V)
    noise = O.synth_noise(B, G_NOISE)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    gs.set_relaxation(mode, STEP_TAU, SEED, hard=True)
    cost, grads, tok, margin = oracle_g_cost_hard(gp, dp, images, noise, mode, STEP_TAU, SEED, 41)
    gl = gs.generator_step(images.cuda(), noise.cuda(), draw=41).cpu()
    print("generator_step(%s, hard): the oracle's smallest top-2 gap %.3e" % (mode, margin))
    assert margin > 1e-3
    rows = gs._relax_buf.cpu()
    assert torch.equal(rows.argmax(dim=-1), tok), "the device's tokens differ from the oracle's"
    assert torch.equal(rows, torch.nn.functional.one_hot(tok, V).float()), "D's input is not the one-hot row"
    assert abs(-float(gl[3]) - float(cost)) <= loss_tol(cost), (gl, cost)
    worst = max((tensor_err(gs.G.grads[n], g), n) for n, g in grads.items())
    print("generator_step(%s, hard, tau %g) gradients: worst rel err %.3e (%s)" % (mode, STEP_TAU, worst[0], worst[1]))
    assert worst[0] < GRAD_RTOL, "generator gradient %s: rel err %.3e" % (worst[1], worst[0])
    g_adam = O.new_adam_state(gp)
    O.tf_adam_step(gp, grads, g_adam[0], g_adam[1], 1)
    gs.flush()
    check_weights_after_adam(gs.G.arena.views, gp, grads, gp0, 1, "generator (%s, hard)" % mode)
    # the soft step is far outside the tolerance against the hard oracle: the comparison can fail
    soft = GanStep(hip, V, S, B, lam=10.0, g_state=gp0, d_state=dp)
    soft.set_relaxation(mode, STEP_TAU, SEED)
    soft.generator_step(images.cuda(), noise.cuda(), draw=41)
    assert tensor_err(soft.G.grads["decoder/bias"], grads["decoder/bias"]) > 100 * GRAD_RTOL


@pytest.mark.parametrize("mode", ["softmax", "gumbel"])
def test_critic_step_matches_oracle_on_the_hard_fake(hip, mode):
    gp, dp = _setup()
    dp0 = {k: v.clone() for k, v in dp.items()}
    images, labels, onehot = O.synth_batch(B, S, V)
    noise, alpha = O.synth_noise(B, D_NOISE), O.synth_alpha(B, 0)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    gs.set_relaxation(mode, STEP_TAU, SEED, hard=True)
    cost, aux, grads, tok, margin = oracle_d_cost_hard(gp, dp, images, onehot, noise, alpha, 10.0, mode, STEP_TAU, SEED, 7)
    grads = {n: g for n, g in grads.items() if g is not None and n != "decoder/bias"}      # (decoder/bias cancels: tests/test_step_gpu.py)
    args = (images.cuda(), labels.cuda(), noise.cuda(), alpha.reshape(B).cuda())
    val = gs.critic_loss(*args, draw=7).cpu()
    dl = gs.critic_step(*args, draw=7).cpu()
    print("critic_step(%s, hard): the oracle's smallest top-2 gap %.3e; disc_cost %.6f (oracle %.6f), gp %.6f (oracle %.6f)"
          % (mode, margin, float(dl[0]), float(cost), float(dl[2]), float(aux["gp"])))
    assert margin > 1e-3
    fake_rows = gs.TRI[:B].cpu()
    assert torch.equal(fake_rows.argmax(dim=-1), tok), "the device's tokens differ from the oracle's"
    assert torch.equal(fake_rows, torch.nn.functional.one_hot(tok, V).float()), "the fake rows are not one-hot"
    assert abs(float(dl[0]) - float(cost)) <= loss_tol(cost) and abs(float(val[0]) - float(cost)) <= loss_tol(cost)
    assert abs(float(dl[2]) - float(aux["gp"])) <= 1e-5 + 1e-4 * abs(float(aux["gp"]))
    worst = max((tensor_err(gs.D.grads[n], g), n) for n, g in grads.items())
    print("critic_step(%s, hard) gradients: worst rel err %.3e (%s)" % (mode, worst[0], worst[1]))
    assert worst[0] < GRAD_RTOL, "critic gradient %s: rel err %.3e" % (worst[1], worst[0])
    d_adam = O.new_adam_state(dp)
    O.tf_adam_step(dp, grads, d_adam[0], d_adam[1], 1)
    gs.flush()
    check_weights_after_adam(gs.D.arena.views, dp, grads, dp0, 1, "critic (%s, hard)" % mode)


@pytest.mark.parametrize("mode", ["softmax", "gumbel"])
def test_hard_iteration_two_stream_equals_serial(hip, mode):
    Bs, Ss, Vs = 2, 32, 11
    images, labels, _ = O.synth_batch(Bs, Ss, Vs)
    img, lab = images.cuda(), labels.cuda()
    res = {}
    for overlap in (False, True):
        gp, dp = O.init_params("G", Vs, Ss, perturb=0.05), O.init_params("D", Vs, Ss, perturb=0.05)
        dp["W"] = dp["W"] * 25.0
        gs = GanStep(hip, Vs, Ss, Bs, lam=10.0, g_state=gp, d_state=dp, overlap_streams=overlap)
        gs.set_relaxation(mode, STEP_TAU, SEED, hard=True)
        for it in range(2):
            _iteration(gs, img, lab, draws=[10 * it, 10 * it + 1, 10 * it + 2])
        res[overlap] = _arenas(gs)
    for k in res[False]:
        assert torch.equal(res[False][k].view(torch.int32), res[True][k].view(torch.int32)), "%s differs between the schedules" % k


def test_test_only_on_a_hard_checkpoint_scores_onehot_of_the_argmax(tmp_path):
    """A straight-through synthetic checkpoint, then train.py --test_only in a fresh child process without the flags: the option comes
    from the checkpoint, recalls.txt is what test() gives in-process, and the scores are the critic's on onehot(argmax(logits)) -
    against the oracle's critic in fp64 on the one-hot rows of the device's logits, within the score tolerance of
    tests/test_eval_batched_gpu.py."""
    import train as T
    from tests.test_eval_batched_gpu import _oracle_per_image
    Bc, Sc, Vc = 8, 64, 50
    mk = lambda **kw: T.SceneGraphGAN(str(tmp_path / "ck"), str(tmp_path / "logs"), None, None, None, None, None, critic_iters=1, batch_size=Bc,
                                      lambda_=10, synthetic=(Bc, Sc, Vc), **kw)
    gan = mk(resume=False, generator_output="gumbel", relax_tau="0.5,0.25,1", relax_hard=True)
    gan.train(max_iterations=1, log_every=1, test_at_end=False)
    rec = [json.loads(l) for l in open(str(tmp_path / "logs" / "losses.jsonl")) if l.strip()]
    assert rec[0]["relax"] == {"mode": "gumbel", "tau": 0.5, "hard": True}
    assert torch.load(gan._ckpt_path())["generator_output"] == {"mode": "gumbel", "tau": [0.5, 0.25, 1], "hard": True}
    out = tmp_path / "eval"
    out.mkdir()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1",
                        "--checkpoints_dir", str(tmp_path / "ck"), "--summaries_dir", str(tmp_path / "logs"), "--test_only",
                        "--max_test_images", "2"], cwd=str(out), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = (out / "recalls.txt").read_text()
    assert '# generator_output: {"mode": "gumbel", "tau": 0.25, "hard": true}' in got
    ev = mk(resume=False)
    assert ev.load_checkpoint() and ev.relax_mode == "gumbel" and ev.relax_hard is True
    _, details = ev.test(max_images=2, out_path=str(tmp_path / "inproc.txt"), return_details=True)
    assert got == (tmp_path / "inproc.txt").read_text()
    met = ev.evaluate(max_images=2, ks=(1, 5), out_path=str(tmp_path / "m.json"))
    assert met["generator_output"] == {"mode": "gumbel", "tau": 0.25, "hard": True}
    # the reference path: the items and noise stream of test(), G's logits from the device, the oracle's critic in fp64 on their one-hot rows
    g = torch.Generator().manual_seed(ev.seed + 99)
    items = [(torch.randn((Sc, Sc, 3), generator=g), torch.randint(0, Vc, (5, 3), generator=g).tolist()) for _ in range(2)]
    TB, n_samples = ev.TEST_BATCH_SIZE, ev.TEST_BATCH_MULTIPLIER * ev.TEST_BATCH_SIZE
    gen = torch.Generator().manual_seed(ev.seed + 123)
    noise = torch.zeros((n_samples, 2, 512))
    for j in range(2):
        for p in range(ev.TEST_BATCH_MULTIPLIER):
            noise[p * TB:(p + 1) * TB, j] = torch.randn((TB, 512), generator=gen)
    images = torch.stack([im for im, _ in items])
    logits = ev.g.sample(images.cuda(), n_samples, noise.cuda()).cpu()
    tokens = O.argmax_tokens(logits.double())
    dp64 = {k: v.double() for k, v in ev.d.state_dict(full_names=False).items()}
    y = torch.nn.functional.one_hot(tokens, Vc).double()
    ref = _oracle_per_image(O.discriminator_head, dp64, images.double(), [y[:, b] for b in range(2)]).mean(dim=2).reshape(n_samples, 2)
    for j in range(2):
        err = float(np.abs(details[j]["scores"] - ref[:, j].numpy()).max())
        print("image %d: max |score - fp64 reference on the one-hot rows| %.3e" % (j, err))
        assert err <= 1e-4 + 1e-4 * float(ref.abs().max())
        assert np.array_equal(details[j]["tokens"], tokens[:, j].numpy()), "the reported tokens are argmax(logits): the rows that were scored"
