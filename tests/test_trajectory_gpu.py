"""-m gpu: the training step on the MI355X PAST its first update against the fp64 oracle - two iterations of two critic updates and one
generator update (tests/trajectory_ref.py: schedule, inputs, the oracle side and the table that justifies every bound;
tests/test_trajectory_cpu.py checks that side without a GPU).  Everything that carries state from one update to the next is on the
device's side only: the copies Trunk.refresh_weights re-derives after each Adam pass, adam_t / lr_t and non-zero moments, the G-encoder
reuse context, the early G stream and the heads' deferred gradient stream, the amax / pq words, the second gradient arena.

(a) Resynchronised (test_resynchronised_updates_match_the_oracle).  Before every update the oracle is REBUILT from the device's arenas
    (parameters, m, v, adam_t -> fp64; the test never writes to an arena and never calls refresh_weights), then both take the update:
      loss |d| <= loss_tol, penalty |d| <= 1e-5 + 1e-4 |gp|, every gradient tensor max|d| < GRAD_RTOL * max|ref| (the critic's decoder
      bias, whose gradient cancels analytically, < 1e-5 on both sides): the bounds of tests/test_step_gpu.py;
      the Adam pass: the device's parameters, m and v after the update against adam_expected on the device's OWN arenas before it and
      its own gradient arena, per element inside the bounds of tests/optim_ref.py (err / bound <= 1) - the optimiser consumed that
      gradient with the right t, lr_t, m, v and scale; adam_t advanced by one, the other network's arenas and adam_t untouched.
    A stale network moves the loss by >= 2.1e-2, stale derived copies alone by >= 2.9e-3 (loss_tol there: 2.2e-6).
(b) Free running (test_free_running_loop_is_the_resynchronised_one_bit_for_bit): GanStep.train_iteration(critic_iters=2,
    reuse_g_encoder=True) with no host read between updates; arenas and moments bit-equal to run (a), the losses each iteration leaves
    within 10 x ORACLE_F32_FREE_RUN of the free-running fp64 oracle.
(c) Accumulated (test_accumulated_updates_match_the_oracle): every update from N = 2 micro-batches of 4 rows; the oracle takes it from
    all 8 rows; the Adam check at gradient scale 1 / N; each network's second update reads an accumulator it has used before.  Then
    train_iteration_accumulated itself, bit-equal.
No second size: the weight layouts at 64 px are those of the 224 px workload layer for layer (tests/test_trajectory_cpu.py).

Measured on the MI355X (profiles/trajectory_pytest_gpu.log; worst over the six updates):

  case                           loss err / tol  gp err / tol  gradient rel err (bound 2e-4)  Adam err / bound  p / m / v  free-running loss err / tol
  f16x3, serial                  0.222           0.004         2.7e-5                         0.998 / 0.500 / 0.871       0.120
  f16x3, two streams             0.222           0.004         2.7e-5                         0.998 / 0.500 / 0.871       0.120
  native f32, serial             0.495           0.009         2.2e-5                         0.997 / 0.500 / 0.876       0.083
  f16x3, serial, 2 x 4 rows      0.186           0.004         3.0e-5                         0.997 / 0.500 / 0.878       0.071

The two-stream figures are the serial ones to every printed digit.  The Adam figures are those of the kernel itself on such data (two fp32 emulations
of it reach 0.998 / 0.500 / 0.88 on the oracle's gradients in tests/test_trajectory_cpu.py): nothing is lost between the gradient arena
and the pass.  Closest to a bound: the loss of D2 in native f32, 1.8e-5 against 3.6e-5 - where the fp32 oracle itself measures 2.0e-5.
Wall time 27 s for the file, nearly all of it the oracle on the host.
"""
import pytest
import torch

import sgg_amd  # noqa: F401
from sgg_amd.step import GanStep
from tests import trajectory_ref as T
from tests.tolerances import GRAD_RTOL, loss_tol

pytestmark = pytest.mark.gpu

OPTIONS = [(2, False), (2, True), (0, False)]            # (conv_precision, overlap_streams)
IDS = ["f16x3-serial", "f16x3-two_stream", "f32-serial"]
_RESYNC, _FREE64 = {}, {}


def snapshot(gs):
    """Parameter, m and v arenas of both networks (whole buffers, dead tail included) as they are now."""
    gs.flush()
    torch.cuda.synchronize()
    return {n + "." + q: f.clone() for n, net in (("G", gs.G), ("D", gs.D))
            for q, f in (("weights", net.arena.flat), ("m", net.m_flat), ("v", net.v_flat))}


def device_inputs(N):
    """The schedule's minibatch and per-update noise / alpha on the device, cut into N micro-batches of B / N rows."""
    Bm = T.B // N
    cut = lambda t, k: t[k * Bm:(k + 1) * Bm].contiguous().cuda()
    images, labels, onehot = T.minibatch()
    batches = [(cut(images, k), cut(labels, k)) for k in range(N)]
    noises, alphas = {}, {}
    for name, kind, it, i in T.SCHEDULE:
        noise, alpha = T.update_inputs(kind, it, i)
        noises[name] = [cut(noise, k) for k in range(N)]
        alphas[name] = None if alpha is None else [cut(alpha.reshape(T.B), k) for k in range(N)]
    return images, onehot, batches, noises, alphas


def make_step(hip, N, overlap):
    gp, dp = T.initial_states()
    return GanStep(hip, T.V, T.S, T.B // N, lam=T.LAM, g_state=gp, d_state=dp, overlap_streams=overlap)


def run_resynchronised(hip, precision, overlap, N=1):
    """Form (a) of the module docstring (N > 1: every update from N micro-batches).  Returns {"failures": messages in the order the
    assertions tripped, "worst": measured maxima per assertion, "final": snapshot, "lines"}; one run per setting for the module."""
    key = (precision, overlap, N)
    if key in _RESYNC:
        return _RESYNC[key]
    old = hip.conv_precision
    hip.conv_precision = precision
    failures, lines, worst = [], [], {}

    def check(name, quantity, value, limit, text):
        worst[quantity] = max(worst.get(quantity, 0.0), value / limit)
        line = "%s %s: %s" % (name, quantity, text)
        lines.append(line)
        if not value <= limit:                   # (a NaN fails)
            failures.append(line)

    try:
        gs = make_step(hip, N, overlap)
        images, onehot, batches, noises, alphas = device_inputs(N)
        for it in range(T.ITERS):
            with gs.iteration(reuse_g_encoder=True):
                for name, kind, _, i in [u for u in T.SCHEDULE if u[2] == it]:
                    net, other = (gs.D, gs.G) if kind == "D" else (gs.G, gs.D)
                    # ---- the oracle follows the device ----
                    gs.flush()
                    torch.cuda.synchronize()
                    (gp, g_adam, tg), (dp, d_adam, td) = T.oracle_from_device(gs.G), T.oracle_from_device(gs.D)
                    t0, t0_other = (td, tg) if kind == "D" else (tg, td)
                    n = net.arena.live_numel
                    before = [f[:n].clone() for f in (net.arena.flat, net.m_flat, net.v_flat)]
                    other_before = [f.clone() for f in (other.arena.flat, other.m_flat, other.v_flat)]
                    # ---- the device's update ----
                    for k, (img, lab) in enumerate(batches):
                        micro = {"micro": (k, N)} if N > 1 else {}
                        if kind == "D":
                            gs.critic_step(img, lab, noises[name][k], alphas[name][k], **micro)
                        else:
                            gs.generator_step(img, noises[name][k], **micro)
                    gs.flush()
                    torch.cuda.synchronize()
                    losses = (gs.d_losses_mean if kind == "D" else gs.g_losses_mean).cpu().double()
                    # ---- the oracle's, from the state the device started from ----
                    noise, alpha = T.update_inputs(kind, it, i)
                    cost, aux, grads = T.oracle_update(kind, gp, dp, d_adam if kind == "D" else g_adam, t0 + 1,
                                                       T.oracle_inputs(images, onehot, noise, alpha))
                    cost = float(cost)
                    got = float(losses[0]) if kind == "D" else -float(losses[3])
                    check(name, "loss", abs(got - cost), loss_tol(cost), "device %.7f oracle %.7f: |d| %.3e (tol %.3e)" % (
                        got, cost, abs(got - cost), loss_tol(cost)))
                    if kind == "D":
                        pen = float(aux["gp"].detach())
                        tol = 1e-5 + 1e-4 * abs(pen)
                        check(name, "gp", abs(float(losses[2]) - pen), tol, "device %.7f oracle %.7f: |d| %.3e (tol %.3e)" % (
                            float(losses[2]), pen, abs(float(losses[2]) - pen), tol))
                        bias = max(float(net.grads["decoder/bias"].abs().max()) / N, float(grads["decoder/bias"].abs().max()))
                        check(name, "decoder/bias gradient", bias, 1e-5, "max |g| on either side %.3e (bound 1e-5)" % bias)
                    # (grad_flat holds the SUM over the micro-batches)
                    err, which = max((T.tensor_err(net.grads[m] / N, g), m) for m, g in grads.items()
                                     if not (kind == "D" and m == "decoder/bias"))
                    check(name, "gradient", err, GRAD_RTOL, "worst tensor %s: rel err %.3e (bound %.0e)" % (which, err, GRAD_RTOL))
                    # ---- the Adam pass, against the device's own gradient ----
                    after = [f[:n] for f in (net.arena.flat, net.m_flat, net.v_flat)]
                    ratio = T.adam_check(name, before, net.grad_flat[:n], after, t0 + 1, 1.0 / N)
                    for q in "pmv":
                        check(name, "adam " + q, ratio[q], 1.0, "worst err / bound %.3f over %d words (t %d, lr_t %.4e, scale %g)" % (
                            ratio[q], n, t0 + 1, T.O.tf_adam_lr_t(t0 + 1), 1.0 / N))
                    moved = not torch.equal(after[0], before[0])
                    counts = (net.adam_t, other.adam_t) == (t0 + 1, t0_other) and moved
                    check(name, "step counts", 0.0 if counts else 2.0, 1.0, "adam_t %s -> %s, other %s -> %s, parameters moved: %s" % (
                        t0, net.adam_t, t0_other, other.adam_t, moved))
                    same = all(torch.equal(a, b) for a, b in zip(other_before, (other.arena.flat, other.m_flat, other.v_flat)))
                    check(name, "other network", 0.0 if same else 2.0, 1.0, "arenas of the network not updated unchanged: %s" % same)
        assert gs._g_reuse is None and not gs._g_reuse_armed
        res = {"failures": failures, "lines": lines, "worst": worst, "final": snapshot(gs), "adam_t": (gs.D.adam_t, gs.G.adam_t)}
    finally:
        hip.conv_precision = old
    _RESYNC[key] = res
    return res


def report(case, res):
    print("\n".join("trajectory %s %s" % (case, line) for line in res["lines"]))
    w = res["worst"]
    print("trajectory %s WORST: loss err / tol %.3f  gp err / tol %.3f  gradient rel err %.3e  adam err / bound p %.3f m %.3f v %.3f" % (
        case, w["loss"], w["gp"], w["gradient"] * GRAD_RTOL, w["adam p"], w["adam m"], w["adam v"]))


def free64():
    """The free-running fp64 oracle's loss per update, once for the module."""
    if not _FREE64:
        _FREE64.update({rec["name"]: rec["cost"] for rec in T.free_run(torch.float64)})
    return _FREE64


def check_free_losses(case, kept):
    """kept[it] = (d_losses, g_losses) as iteration `it` left them: the last critic update's and the generator update's."""
    ref, bad, worst = free64(), [], 0.0
    for it, (dl, gl) in enumerate(kept):
        d_name = [u[0] for u in T.SCHEDULE if u[2] == it and u[1] == "D"][-1]
        g_name = [u[0] for u in T.SCHEDULE if u[2] == it and u[1] == "G"][-1]
        for name, got in ((d_name, float(dl.cpu()[0])), (g_name, -float(gl.cpu()[3]))):
            tol = 10.0 * T.ORACLE_F32_FREE_RUN[name]
            err = abs(got - ref[name])
            worst = max(worst, err / tol)
            print("trajectory %s free-running %s: device %.7f oracle %.7f: |d| %.3e (tol %.1e)" % (case, name, got, ref[name], err, tol))
            if not err <= tol:
                bad.append((name, got, ref[name], err, tol))
    print("trajectory %s WORST free-running loss err / tol %.3f" % (case, worst))
    return bad


def differing(a, b):
    return [k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]


@pytest.mark.parametrize("precision,overlap", OPTIONS, ids=IDS)
def test_resynchronised_updates_match_the_oracle(hip, precision, overlap):
    res = run_resynchronised(hip, precision, overlap)
    report("%s/%s" % (precision, "two_stream" if overlap else "serial"), res)
    assert res["adam_t"] == (4, 2)
    assert not res["failures"], "in the order they tripped:\n" + "\n".join(res["failures"])


@pytest.mark.parametrize("precision,overlap", OPTIONS, ids=IDS)
def test_free_running_loop_is_the_resynchronised_one_bit_for_bit(hip, precision, overlap):
    want = run_resynchronised(hip, precision, overlap)["final"]
    case = "%s/%s" % (precision, "two_stream" if overlap else "serial")
    old = hip.conv_precision
    hip.conv_precision = precision
    try:
        gs = make_step(hip, 1, overlap)
        _, _, batches, noises, alphas = device_inputs(1)
        (img, lab), kept = batches[0], []
        for it in range(T.ITERS):
            names = [u[0] for u in T.SCHEDULE if u[2] == it]
            gs.train_iteration(img, lab, [noises[u][0] for u in names], [alphas[u][0] for u in names[:T.CRITIC_ITERS]],
                               critic_iters=T.CRITIC_ITERS, reuse_g_encoder=True)
            kept.append((gs.d_losses.clone(), gs.g_losses.clone()))       # (device copies on the step's stream: no host read)
        got = snapshot(gs)
        assert (gs.D.adam_t, gs.G.adam_t) == (4, 2)
    finally:
        hip.conv_precision = old
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    bad = differing(want, got)
    assert not bad, "the free-running loop differs from the resynchronised one in %s" % bad
    bad = check_free_losses(case, kept)
    assert not bad, bad


def test_accumulated_updates_match_the_oracle(hip):
    N = 2
    res = run_resynchronised(hip, 2, False, N=N)
    report("2/serial/accumulate %d" % N, res)
    assert res["adam_t"] == (4, 2)
    assert not res["failures"], "in the order they tripped:\n" + "\n".join(res["failures"])
    # the production call: bit-equal, and its loss means against the free-running oracle on all rows
    old = hip.conv_precision
    hip.conv_precision = 2
    try:
        gs = make_step(hip, N, False)
        _, _, batches, noises, alphas = device_inputs(N)
        kept = []
        for it in range(T.ITERS):
            names = [u[0] for u in T.SCHEDULE if u[2] == it]
            gs.train_iteration_accumulated(batches, [noises[u] for u in names], [alphas[u] for u in names[:T.CRITIC_ITERS]],
                                           critic_iters=T.CRITIC_ITERS, reuse_g_encoder=True)
            kept.append((gs.d_losses_mean.clone(), gs.g_losses_mean.clone()))
        got = snapshot(gs)
        assert (gs.D.adam_t, gs.G.adam_t) == (4, 2) and "acc" in gs.D.opt and "acc" in gs.G.opt
    finally:
        hip.conv_precision = old
    bad = differing(res["final"], got)
    assert not bad, "train_iteration_accumulated differs from the resynchronised updates in %s" % bad
    bad = check_free_losses("2/serial/accumulate %d" % N, kept)
    assert not bad, bad
