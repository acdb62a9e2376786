"""-m gpu: the score-function generator update - the kernels behind HipKernels.score_advantage / score_rows / score_summary
(csrc/score.hip) against the numpy fp64 restatement of tests/score_ref.py, and GanStep.set_estimator("score") / train.py
--generator_gradient score against autograd on the CPU oracle's surrogate (tests/test_score_cpu.py).

The shapes of score_rows are RELAX_CASES of tests/test_relax_gpu.py with relax_case's x (|x| <= 23, a row of equal logits, a saturated
row): both sides of the wave width, 1025 rows of 7 (four rows per workgroup), the resident / streaming threshold, rows aligned
differently, two sweeps of the streaming workgroup and V = 70 001 (the four-loads-in-flight loop of pass 1).  Every case runs with group 1
and 3, ent_coef 0 and 0.4, stored and accumulated, and with each optional output absent in turn."""
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
from tests import score_ref as SR
from tests import xent_ref as XR
from tests.score_ref import (SCORE_ADV_TOL, SCORE_ENT_ERR_MEASURED, SCORE_ENT_GRAD_ERR_MEASURED, SCORE_ENT_GRAD_TOL, SCORE_ENT_TOL, SCORE_OUT2_TOL,
                             SCORE_SUMMARY_TOL)
from tests.test_relax_cpu import SEED
from tests.test_relax_gpu import RELAX_CASES, _arenas, _iteration, _setup, on_device, relax_case
from tests.test_relax_hard_gpu import G_NOISE
from tests.test_score_cpu import oracle_g_score
from tests.test_step_gpu import check_weights_after_adam, tensor_err
from tests.test_xent_gpu import EPS32, F32, I64, SENT, assert_rows_guard, assert_vec_guard, rows_view, u32, vec
from tests.tolerances import GRAD_RTOL, loss_tol
from tests.xent_ref import XENT_GRAD_TOL, XENT_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["R%d-V%d-ldx%d-ldy%d-sx%d-sy%d" % c for c in RELAX_CASES]
COEF = 0.375                                   # (exact in fp32)
ENT_COEF = float(np.float32(0.4))              # the value the entry point receives


def test_the_measured_entropy_errors_lie_within_the_likelihoods_bound():
    """The issue's condition on the two measured constants, and the tolerances as ten times them."""
    assert SCORE_ENT_ERR_MEASURED <= XENT_TOL and SCORE_ENT_GRAD_ERR_MEASURED <= XENT_TOL
    assert 10 * SCORE_ENT_ERR_MEASURED <= SCORE_ENT_TOL <= 11 * SCORE_ENT_ERR_MEASURED
    assert 10 * SCORE_ENT_GRAD_ERR_MEASURED <= SCORE_ENT_GRAD_TOL <= 11 * SCORE_ENT_GRAD_ERR_MEASURED


def rows_inputs(case, group):
    """(x, tok, adv) of a case: relax_case's x; tokens random in range, row 1 with token -1 and row 2 with token V; adv in [-2, 2]."""
    R, V = case[0], case[1]
    x = relax_case(case, 1.0, False)[0]
    g = np.random.RandomState(4000 + R + V + group)
    tok = g.randint(0, V, size=R).astype(np.int64)
    if R > 1:
        tok[1] = -1
    if R > 2:
        tok[2] = V
    adv = (4.0 * g.random_sample(-(-R // group)) - 2.0).astype(np.float32)
    return x, tok, adv


def launch_rows(hip, case, xv, tok_d, adv_d, group, coef, ent_coef, accumulate, d0=None, want=("dx", "logp", "ent")):
    R, V, ldx, ldy, sx, sy = case
    bd, dv = rows_view(R, V, ldy, sy, SENT[F32])
    if d0 is not None:
        dv.copy_(torch.from_numpy(d0).cuda())
    (bl, logp), (be, ent) = vec(R, F32), vec(R, F32)
    hip.score_rows(xv, tok_d, adv_d, group=group, coef=coef, ent_coef=ent_coef, accumulate=accumulate, dx=dv if "dx" in want else None,
                   logp=logp if "logp" in want else None, ent=ent if "ent" in want else None)
    torch.cuda.synchronize()
    assert_rows_guard(bd, R, V, ldy, sy, "dx")
    assert_vec_guard(bl, R, "logp")
    assert_vec_guard(be, R, "ent")
    if "dx" not in want:
        assert (bd.cpu().numpy() == SENT[F32]).all(), "dx absent, yet written"
    for name, b in (("logp", bl), ("ent", be)):
        if name not in want:
            assert (b.cpu().numpy() == SENT[F32]).all(), "%s absent, yet written" % name
    return dv, logp, ent


@pytest.mark.parametrize("group", [1, 3])
@pytest.mark.parametrize("case", RELAX_CASES, ids=IDS)
def test_score_rows_match_fp64_restatement(hip, case, group):
    R, V, ldx, ldy, sx, sy = case
    x, tok, adv = rows_inputs(case, group)
    valid = (tok >= 0) & (tok < V)
    w = np.abs(COEF * adv.astype(np.float64)[np.arange(R) // group])[:, None]
    bx, xv = on_device(x, R, V, ldx, sx, float("nan"))
    tok_d, adv_d = torch.from_numpy(tok).cuda(), torch.from_numpy(adv).cuda()
    d0 = np.random.RandomState(1).standard_normal((R, V)).astype(np.float32)
    worst_ent, worst_entgrad = 0.0, 0.0
    for ent_coef in (0.0, ENT_COEF):
        ref = SR.score_rows(x, tok, adv, group, COEF, ent_coef)
        dv, logp, ent = launch_rows(hip, case, xv, tok_d, adv_d, group, COEF, ent_coef, False)
        dx, lp, en = dv.cpu().numpy(), logp.cpu().numpy(), ent.cpu().numpy()
        assert np.isfinite(dx).all() and np.isfinite(lp).all() and np.isfinite(en).all()
        err_lp, err_en = float(np.abs(lp - ref["logp"]).max()), float(np.abs(en - ref["ent"]).max())
        err_dx = np.abs(dx - ref["dx"])
        worst_ent = max(worst_ent, err_en)
        print("score_rows R %d V %d group %d ent_coef %g: max |logp - ref| %.3e  |ent - ref| %.3e  |dx - ref| %.3e (in units of its bound %.3f)"
              % (R, V, group, ent_coef, err_lp, err_en, float(err_dx.max()),
                 float((err_dx / (XENT_GRAD_TOL * w + SCORE_ENT_GRAD_TOL * ent_coef + 1e-30)).max())))
        # exact: the skipped rows; the inputs
        assert (lp[~valid] == 0.0).all() and (dx[~valid] == 0.0).all(), "a skipped row: logp = 0, dx zero-filled"
        assert np.array_equal(u32(xv.contiguous()), x.view(np.uint32)), "x was written"
        assert np.array_equal(tok_d.cpu().numpy(), tok) and np.array_equal(u32(adv_d), adv.view(np.uint32)), "tok or adv was written"
        assert err_lp <= XENT_TOL and err_en <= SCORE_ENT_TOL
        assert (err_dx <= XENT_GRAD_TOL * w + SCORE_ENT_GRAD_TOL * ent_coef).all()
        # two launches: equal bits for every output
        dv2, logp2, ent2 = launch_rows(hip, case, xv, tok_d, adv_d, group, COEF, ent_coef, False)
        for a, b, what in ((dv, dv2, "dx"), (logp, logp2, "logp"), (ent, ent2, "ent")):
            assert np.array_equal(u32(a.contiguous()), u32(b.contiguous())), "%s differs between two launches" % what
        # accumulate = 1: added to what is there (one fp32 addition more), a skipped row keeps its bits
        want = SR.score_rows(x, tok, adv, group, COEF, ent_coef, accumulate=True, dx=d0)["dx"]
        dva, logpa, enta = launch_rows(hip, case, xv, tok_d, adv_d, group, COEF, ent_coef, True, d0)
        got = dva.cpu().numpy()
        assert (np.abs(got - want) <= XENT_GRAD_TOL * w + SCORE_ENT_GRAD_TOL * ent_coef + EPS32 * np.abs(want)).all()
        assert np.array_equal(got[~valid].view(np.uint32), d0[~valid].view(np.uint32)), "accumulate = 1 touched a skipped row"
        assert np.array_equal(u32(logpa), u32(logp)) and np.array_equal(u32(enta), u32(ent))
        # each optional output absent in turn: the others keep their bits
        for absent in ("dx", "logp", "ent"):
            dvo, logpo, ento = launch_rows(hip, case, xv, tok_d, adv_d, group, COEF, ent_coef, False,
                                           want=tuple(n for n in ("dx", "logp", "ent") if n != absent))
            for name, a, b in (("dx", dv, dvo), ("logp", logp, logpo), ("ent", ent, ento)):
                if name != absent:
                    assert np.array_equal(u32(a.contiguous()), u32(b.contiguous())), "%s differs without %s" % (name, absent)
    # adv = None: every weight is coef - the cross-entropy's gradient at the same scale, within its own bound
    dvn, _, _ = launch_rows(hip, case, xv, tok_d, None, group, COEF, 0.0, False)
    assert float(np.abs(dvn.cpu().numpy() - XR.softmax_xent(x, tok, COEF)["dlogits"]).max()) <= XENT_GRAD_TOL * COEF
    # the entropy part alone (coef = 0), in units of ent_coef: the figure behind SCORE_ENT_GRAD_ERR_MEASURED
    dve, _, _ = launch_rows(hip, case, xv, tok_d, adv_d, group, 0.0, ENT_COEF, False)
    worst_entgrad = float(np.abs(dve.cpu().numpy() - SR.score_rows(x, tok, adv, group, 0.0, ENT_COEF)["dx"]).max()) / ENT_COEF
    print("score_rows R %d V %d group %d: MEASURED max |ent - ref| %.3e   max |entropy part of dx - ref| / ent_coef %.3e"
          % (R, V, group, worst_ent, worst_entgrad))
    assert worst_entgrad <= SCORE_ENT_GRAD_TOL


@pytest.mark.parametrize("V,ld,sx", [(11, 11, 0), (5125, 5125, 3)])
def test_rows_of_plus_minus_80_give_finite_outputs(hip, V, ld, sx):
    R = 2
    x = np.empty((R, V), dtype=np.float32)
    x[0] = np.where(np.arange(V) % 2 == 0, 80.0, -80.0)
    x[1] = np.where(np.arange(V) % 3 == 0, -80.0, 80.0)
    tok = np.array([V - 1, 0], dtype=np.int64)                     # both sampled tokens sit at -80
    adv = np.array([1.5, -2.0], dtype=np.float32)
    case = (R, V, ld, ld, sx, sx)
    bx, xv = on_device(x, R, V, ld, sx, float("nan"))
    dv, logp, ent = launch_rows(hip, case, xv, torch.from_numpy(tok).cuda(), torch.from_numpy(adv).cuda(), 1, COEF, ENT_COEF, False)
    ref = SR.score_rows(x, tok, adv, 1, COEF, ENT_COEF)
    dx, lp, en = dv.cpu().numpy(), logp.cpu().numpy(), ent.cpu().numpy()
    assert np.isfinite(dx).all() and np.isfinite(lp).all() and np.isfinite(en).all()
    print("+-80 rows V %d: |logp - ref| %.3e  |ent - ref| %.3e  |dx - ref| %.3e" % (V, float(np.abs(lp - ref["logp"]).max()),
                                                                                   float(np.abs(en - ref["ent"]).max()), float(np.abs(dx - ref["dx"]).max())))
    assert float(np.abs(lp - ref["logp"]).max()) <= XENT_TOL * 80.0, "the likelihood's bound for these rows (tests/test_xent_gpu.py)"


@pytest.mark.parametrize("baseline", ["rloo", "none"])
@pytest.mark.parametrize("ldd", [3, 5])
@pytest.mark.parametrize("B", [2, 3, 64, 1000])
def test_score_advantage(hip, B, ldd, baseline):
    T = 3
    d = (60.0 * np.random.RandomState(B + ldd).random_sample((B, T)) - 30.0).astype(np.float32)
    adv64, out64 = SR.score_advantage(d, baseline)
    scale = max(1.0, float(np.abs(d).max()))
    bd, dv = on_device(d, B, T, ldd, 0, float("nan"))
    (ba, adv), (bo, out2) = vec(B, F32), vec(2, F32)
    assert hip.score_advantage(dv, baseline, adv=adv, out2=out2) is adv
    torch.cuda.synchronize()
    assert_vec_guard(ba, B, "adv")
    assert_vec_guard(bo, 2, "out2")
    assert np.array_equal(u32(dv.contiguous()), d.view(np.uint32)), "d_out was written"
    got, o = adv.cpu().numpy(), out2.cpu().numpy()
    e_adv, e0, e1 = float(np.abs(got - adv64).max()), abs(float(o[0]) - out64[0]), abs(float(o[1]) - out64[1])
    print("score_advantage B %d ldd %d %s: |adv - ref| %.3e  |mean r - ref| %.3e  |mean adv^2 - ref| %.3e" % (B, ldd, baseline, e_adv, e0, e1))
    assert e_adv <= SCORE_ADV_TOL * scale and e0 <= SCORE_OUT2_TOL * scale and e1 <= SCORE_OUT2_TOL * scale * scale
    # out2 is optional; two launches give the same bits
    (ba2, adv2) = vec(B, F32)
    hip.score_advantage(dv, baseline, adv=adv2)
    assert np.array_equal(u32(adv2), u32(adv))
    assert_vec_guard(ba2, B, "adv")


@pytest.mark.parametrize("R", [3, 192, 3075])
def test_score_summary(hip, R):
    g = np.random.RandomState(R)
    logp, ent = (-8.0 * g.random_sample(R)).astype(np.float32), (6.0 * g.random_sample(R)).astype(np.float32)
    want = SR.score_summary(logp, ent)
    bo, out = vec(2, F32)
    hip.score_summary(torch.from_numpy(logp).cuda(), torch.from_numpy(ent).cuda(), out2=out)
    got = out.cpu().numpy()
    assert_vec_guard(bo, 2, "out2")
    assert abs(got[0] - want[0]) <= SCORE_SUMMARY_TOL * float(np.abs(logp).max()) and abs(got[1] - want[1]) <= SCORE_SUMMARY_TOL * float(np.abs(ent).max())
    again = hip.score_summary(torch.from_numpy(logp).cuda(), torch.from_numpy(ent).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_bad_arguments_are_refused_and_nothing_is_written(hip):
    from sgg_amd.lib import SggError
    R, V, T = 3, 5, 3
    x = torch.zeros(R, V, device="cuda")
    bd, d = on_device(None, R, V, V, 0, SENT[F32])
    (bl, logp), (be, ent), (ba, adv), (bo, out2) = vec(R, F32), vec(R, F32), vec(R, F32), vec(2, F32)
    tok = torch.zeros(R, dtype=I64, device="cuda")
    dout = torch.ones(R, T, device="cuda")
    one = torch.ones(R, device="cuda")
    # the wrapper's own checks: the baseline's name, dtypes, devices, shapes, a short adv, tok's length
    with pytest.raises(ValueError, match="baseline"):
        hip.score_advantage(dout, "mean", adv=adv)
    with pytest.raises(SggError, match="B >= 2"):
        hip.score_advantage(dout[:1], "rloo", adv=adv[:1], out2=out2)
    with pytest.raises(SggError, match="not on a HIP device"):
        hip.score_rows(x, tok.cpu(), one, dx=d)
    with pytest.raises(SggError, match="not on a HIP device"):
        hip.score_advantage(dout.cpu(), "none", adv=adv)
    for bad in (lambda: hip.score_rows(x.double(), tok, one, dx=d), lambda: hip.score_rows(x, tok.int(), one, dx=d),
                lambda: hip.score_rows(x, tok, one.double(), dx=d), lambda: hip.score_rows(x, tok[:2], one, dx=d),
                lambda: hip.score_rows(x, tok, one[:2], group=1, dx=d), lambda: hip.score_rows(x, tok, one[:0], group=3, dx=d),
                lambda: hip.score_rows(x, tok, one, dx=d[:2]), lambda: hip.score_rows(x, tok, one, dx=d, logp=logp[:2]),
                lambda: hip.score_advantage(dout, "none", adv=adv[:2]), lambda: hip.score_advantage(dout.double(), "none", adv=adv),
                lambda: hip.score_summary(logp, ent[:2], out2=out2), lambda: hip.score_summary(logp, ent, out2=out2.double())):
        with pytest.raises(AssertionError):
            bad()
    with pytest.raises(SggError, match="no output"):
        hip.score_rows(x, tok, one)
    with pytest.raises(SggError, match="alias"):
        hip.score_rows(x, tok, one, dx=x)
    with pytest.raises(SggError, match="group"):
        hip.score_rows(x, tok, one, group=0, dx=d)
    for c, e in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan")), (1.0, float("-inf"))):
        with pytest.raises(SggError, match="finite"):
            hip.score_rows(x, tok, one, coef=c, ent_coef=e, dx=d, logp=logp, ent=ent)
    # shapes and pointers the binding cannot produce: the C entry points themselves
    lib, st = hip.lib, hip._stream()
    big = (1 << 21) + 1
    xp, tp, ap, dp_, lp, ep, op, gp_ = (t.data_ptr() for t in (x, tok, adv, d, logp, ent, out2, dout))
    for rc in (lib.sgg_score_rows(xp, V, 0, V, tp, ap, 1, 1.0, 0.0, 0, dp_, V, lp, ep, st),
               lib.sgg_score_rows(xp, V, R, 0, tp, ap, 1, 1.0, 0.0, 0, dp_, V, lp, ep, st),
               lib.sgg_score_rows(xp, big, 1, big, tp, ap, 1, 1.0, 0.0, 0, dp_, big, lp, ep, st),
               lib.sgg_score_rows(xp, V - 1, R, V, tp, ap, 1, 1.0, 0.0, 0, dp_, V, lp, ep, st),
               lib.sgg_score_rows(xp, V, R, V, tp, ap, 1, 1.0, 0.0, 0, dp_, V - 1, lp, ep, st),
               lib.sgg_score_rows(xp, V, R, V, tp, ap, -1, 1.0, 0.0, 0, dp_, V, lp, ep, st),
               lib.sgg_score_rows(xp, V, R, V, tp, ap, 1, 1.0, 0.0, 2, dp_, V, lp, ep, st),
               lib.sgg_score_rows(None, V, R, V, tp, ap, 1, 1.0, 0.0, 0, dp_, V, lp, ep, st),
               lib.sgg_score_rows(xp, V, R, V, None, ap, 1, 1.0, 0.0, 0, dp_, V, lp, ep, st),
               lib.sgg_score_rows(xp, V, R, V, tp, ap, 1, 1.0, 0.0, 0, None, V, None, None, st),
               lib.sgg_score_advantage(gp_, T, 0, T, 0, ap, op, st), lib.sgg_score_advantage(gp_, T, (1 << 20) + 1, T, 0, ap, op, st),
               lib.sgg_score_advantage(gp_, T, 1, T, 1, ap, op, st), lib.sgg_score_advantage(gp_, T, R, 0, 0, ap, op, st),
               lib.sgg_score_advantage(gp_, 65, R, 65, 0, ap, op, st), lib.sgg_score_advantage(gp_, T - 1, R, T, 0, ap, op, st),
               lib.sgg_score_advantage(gp_, T, R, T, 2, ap, op, st), lib.sgg_score_advantage(None, T, R, T, 0, ap, op, st),
               lib.sgg_score_advantage(gp_, T, R, T, 0, None, op, st),
               lib.sgg_score_summary(lp, ep, 0, op, st), lib.sgg_score_summary(lp, ep, (1 << 24) + 1, op, st),
               lib.sgg_score_summary(None, ep, R, op, st), lib.sgg_score_summary(lp, None, R, op, st), lib.sgg_score_summary(lp, ep, R, None, st)):
        assert rc == -1 and b"sgg_score_" in lib.sgg_last_error()
    torch.cuda.synchronize()
    for b in (bd, bl, be, ba, bo):
        assert (b.cpu().numpy() == SENT[F32]).all(), "a refused call wrote something"
    assert float(x.abs().max()) == 0.0 and tok.tolist() == [0] * R and float((dout - 1.0).abs().max()) == 0.0


# ---- the step ------------------------------------------------------------------------------------------------------------------
# B 8, S 64, V 50, _setup() weights, synth_noise(B, 5), SEED and draw 41: the inputs of the hard test's generator update
# (tests/test_relax_hard_gpu.py).  On the CPU oracle the smallest top-2 gap of x + g over the 24 rows is 3.46e-2, far above the fp32
# difference between the device's logits and the oracle's; the eight rewards span -0.19 .. 0.54 with max|A| = 0.44 = 0.82 max|r|: the
# advantages are far above the fp32 error of D's outputs.
B, S, V = 8, 64, 50


@pytest.mark.parametrize("w_ent", [0.0, 0.05])
@pytest.mark.parametrize("baseline", ["rloo", "none"])
def test_generator_step_in_score_mode_matches_the_oracle(hip, baseline, w_ent):
    gp, dp = _setup()
    gp0 = {k: v.clone() for k, v in gp.items()}
    images, labels, _ = O.synth_batch(B, S, V)
    noise = O.synth_noise(B, G_NOISE)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    gs.set_relaxation("gumbel", 1.0, SEED, hard=True)
    gs.set_estimator("score", baseline, w_ent)
    d_before = gs.D.grad_flat.clone()
    ref = oracle_g_score(gp, dp, images, noise, SEED, 41, baseline, w_ent)
    gl = gs.generator_step(images.cuda(), noise.cuda(), draw=41).cpu()
    r = ref["rewards"]
    print("generator_step(score, %s, w %g): top-2 gap %.3e, rewards %.3f .. %.3f, max|A| %.3f; numbers %s (oracle %s)"
          % (baseline, w_ent, ref["margin"], float(r.min()), float(r.max()), ref["max_adv"], gs.score_losses.cpu().tolist(), ref["numbers"]))
    assert ref["margin"] > 1e-3
    assert torch.equal(gs._score_tok.cpu(), ref["tok"]), "the device's tokens differ from the oracle's"
    assert torch.equal(gs._relax_buf.cpu(), torch.nn.functional.one_hot(ref["tok"], V).float()), "D's input is not the one-hot row"
    assert abs(float(gl[3]) - ref["d_mean"]) <= loss_tol(ref["d_mean"]), (gl, ref["d_mean"])
    for got, want, what in zip(gs.score_losses.cpu().tolist(), ref["numbers"], ("reward", "advantage^2", "logp", "entropy")):
        assert abs(got - want) <= loss_tol(want), "score_losses %s: %r against the oracle's %r" % (what, got, want)
    grads = ref["grads"]
    worst = max((tensor_err(gs.G.grads[n], g), n) for n, g in grads.items())
    print("generator_step(score, %s, w %g) gradients: worst rel err %.3e (%s)" % (baseline, w_ent, worst[0], worst[1]))
    assert worst[0] < GRAD_RTOL, "generator gradient %s: rel err %.3e" % (worst[1], worst[0])
    g_adam = O.new_adam_state(gp)
    O.tf_adam_step(gp, grads, g_adam[0], g_adam[1], 1)
    gs.flush()
    check_weights_after_adam(gs.G.arena.views, gp, grads, gp0, 1, "generator (score, %s, w %g)" % (baseline, w_ent))
    assert torch.equal(gs.D.grad_flat, d_before) and gs.D.adam_t == 0, "D's gradients were touched"
    if baseline == "rloo" and w_ent == 0.0:
        # the hard pathwise step is far outside the tolerance against the score oracle: the comparison can fail
        path = GanStep(hip, V, S, B, lam=10.0, g_state=gp0, d_state=dp)
        path.set_relaxation("gumbel", 1.0, SEED, hard=True)
        path.generator_step(images.cuda(), noise.cuda(), draw=41)
        assert tensor_err(path.G.grads["decoder/bias"], grads["decoder/bias"]) > 100 * GRAD_RTOL


def test_score_iteration_two_stream_equals_serial(hip):
    Bs, Ss, Vs = 2, 32, 11
    images, labels, _ = O.synth_batch(Bs, Ss, Vs)
    img, lab = images.cuda(), labels.cuda()
    res = {}
    for overlap in (False, True):
        gp, dp = O.init_params("G", Vs, Ss, perturb=0.05), O.init_params("D", Vs, Ss, perturb=0.05)
        dp["W"] = dp["W"] * 25.0
        gs = GanStep(hip, Vs, Ss, Bs, lam=10.0, g_state=gp, d_state=dp, overlap_streams=overlap)
        gs.set_relaxation("gumbel", 1.0, SEED, hard=True)
        gs.set_estimator("score", "rloo", 0.05)
        for it in range(2):
            _iteration(gs, img, lab, draws=[10 * it, 10 * it + 1, 10 * it + 2])
        res[overlap] = _arenas(gs)
        res[overlap]["score"] = gs.score_losses.clone()
    for k in res[False]:
        assert torch.equal(res[False][k].view(torch.int32), res[True][k].view(torch.int32)), "%s differs between the schedules" % k


def test_train_synthetic_score_run_and_test_only_on_its_checkpoint(tmp_path):
    import train as T
    Bc, Sc, Vc = 8, 64, 50
    mk = lambda **kw: T.SceneGraphGAN(str(tmp_path / "ck"), str(tmp_path / "logs"), None, None, None, None, None, critic_iters=1, batch_size=Bc,
                                      lambda_=10, synthetic=(Bc, Sc, Vc), **kw)
    gan = mk(resume=False, generator_gradient="score", entropy_weight=0.01)
    gan.train(max_iterations=3, log_every=1, test_at_end=False)
    rec = [json.loads(l) for l in open(str(tmp_path / "logs" / "losses.jsonl")) if l.strip()]
    assert len(rec) == 3
    for r in rec:
        assert r["relax"] == {"mode": "gumbel", "tau": 1.0, "hard": True}
        sc = r["score"]
        assert sc["baseline"] == "rloo" and sc["entropy_weight"] == 0.01
        assert all(np.isfinite(sc[k]) for k in ("reward", "adv_rms", "logp_token", "entropy_token")) and np.isfinite(r["gen_loss"])
        assert sc["logp_token"] < 0.0 < sc["entropy_token"] <= np.log(Vc) + 1e-5 and abs(sc["reward"] + r["gen_loss"]) <= 1e-5
    assert torch.load(gan._ckpt_path())["generator_output"] == {"mode": "gumbel", "tau": [1.0, 1.0, 0], "hard": True,
                                                                "gradient": {"kind": "score", "baseline": "rloo", "entropy_weight": 0.01}}
    out = tmp_path / "eval"
    out.mkdir()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1",
                        "--checkpoints_dir", str(tmp_path / "ck"), "--summaries_dir", str(tmp_path / "logs"), "--test_only",
                        "--max_test_images", "2"], cwd=str(out), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert '# generator_output: {"mode": "gumbel", "tau": 1.0, "hard": true, "gradient": "score"}' in (out / "recalls.txt").read_text()
