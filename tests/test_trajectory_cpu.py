"""CPU: the reference side of tests/test_trajectory_gpu.py meets the conditions that make that test meaningful - recomputed from the oracle
alone (tests/trajectory_ref.py has the schedule and the table these figures are recorded in).

  * the gradient penalty is active in every critic update;
  * a network that is one update stale is visible in the loss at every update from the second on, by more than 1000 x loss_tol - and so
    is one of which only the copies Trunk.refresh_weights derives are stale (the convolution kernels from conv1_2 on);
  * from the same state the fp32 oracle is inside loss_tol and GRAD_RTOL of the fp64 oracle at every update (decoder/bias of the critic
    left out as in tests/test_step_gpu.py: its gradient cancels analytically) - the bounds the GPU test applies per update;
  * free-running, the fp32 oracle stays within 5 x ORACLE_F32_FREE_RUN of the fp64 one (the GPU test allows the device 10 x);
  * two fp32 emulations of the Adam kernel, fed the oracle's own second-update state and gradient, lie inside adam_expected's bounds
    (non-zero m / v, t = 2, gradients that were not chosen to keep every intermediate normal);
  * what keeps the derived weight copies current is arena.version, not the call in Network.adam_step: with that call alone left out, the
    next forward re-derives them (host logic on the CPU reference kernels); left stale they would show as the "derived" column;
  * the weight layouts the encoder derives at 64 px are, layer for layer and direction for direction, those of the 224 px workload.

One pass over the schedule serves every test (about 25 s on 16 threads: six fp64 and twelve fp32 oracle updates, eighteen stale losses)."""
import numpy as np
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd import build, lib
from sgg_amd.params import CONV_SPECS, same_pads
from tests import optim_ref as R
from tests import trajectory_ref as T
from tests.tolerances import GRAD_RTOL, loss_tol

_TABLE = {}


def _flat(d, names):
    return torch.cat([d[n].reshape(-1) for n in names])


def table():
    """Every column of the table in tests/trajectory_ref.py, one row per update, computed once for the module."""
    if _TABLE:
        return _TABLE
    rows = {n: {} for n in T.NAMES}
    prev = {}                                    # kind -> that network's parameters before its last update (fp64)

    def before(name, kind, gp, dp, adam, t, inputs):
        row = rows[name]
        # the loss with one network one update stale (the other, and the inputs, as they are)
        row["stale"] = {"D": T.oracle_loss(kind, gp, prev["D"], inputs) if "D" in prev else None,
                        "G": T.oracle_loss(kind, prev["G"], dp, inputs) if "G" in prev else None,
                        "D derived": T.oracle_loss(kind, gp, T.derived_stale(dp, prev["D"]), inputs) if "D" in prev else None,
                        "G derived": T.oracle_loss(kind, T.derived_stale(gp, prev["G"]), dp, inputs) if "G" in prev else None}
        prev[kind] = T.to_dtype(dp if kind == "D" else gp, torch.float64)
        # the fp32 oracle from the SAME state: parameters and moments rounded to fp32, one update
        f = torch.float32
        gp32, dp32 = T.to_dtype(gp, f), T.to_dtype(dp, f)
        adam32 = (T.to_dtype(adam[0], f), T.to_dtype(adam[1], f))
        own = dp32 if kind == "D" else gp32
        names = [n for n in own if not O.is_dead(n)]
        state32 = [_flat(own, names).numpy().copy(), _flat(adam32[0], names).numpy().copy(), _flat(adam32[1], names).numpy().copy()]
        in32 = {k: (None if v is None else v.to(f)) for k, v in inputs.items()}
        cost32, _, grads32 = T.oracle_update(kind, gp32, dp32, adam32, t + 1, in32)
        row["same32"] = (float(cost32), grads32)
        if name in ("D2", "G2"):
            row["adam"] = (state32, _flat(grads32, names).numpy().copy(), t + 1)

    for rec in T.free_run(torch.float64, before):
        rows[rec["name"]].update(kind=rec["kind"], cost=rec["cost"], gp=rec["gp"], grads=rec["grads"])
    for rec in T.free_run(torch.float32):
        rows[rec["name"]]["free32"] = rec["cost"]
    print("\nupdate  fp64 loss      gp        stale D    stale G    derived D  derived G  same-state fp32: loss / worst gradient        free-running fp32: loss")
    for name in T.NAMES:
        row = rows[name]
        cost32, grads32 = row["same32"]
        row["same_loss"] = abs(cost32 - row["cost"])
        row["same_grad"] = max((T.tensor_err(grads32[n], g), n) for n, g in row["grads"].items()
                               if not (row["kind"] == "D" and n == "decoder/bias"))
        row["bias"] = max(float(g["decoder/bias"].abs().max()) for g in (grads32, row["grads"])) if row["kind"] == "D" else None
        row["free_loss"] = abs(row["free32"] - row["cost"])
        row["stale_diff"] = {k: (None if v is None else abs(v - row["cost"])) for k, v in row["stale"].items()}
        fmt = lambda x: "-        " if x is None else "%.3e" % x
        print("%-6s  %+13.7f  %s  %s  %s  %s  %s  %.3e (tol %.3e) / %.3e %-28s  %.3e (recorded %.1e)" % (
            name, row["cost"], fmt(row["gp"]), fmt(row["stale_diff"]["D"]), fmt(row["stale_diff"]["G"]), fmt(row["stale_diff"]["D derived"]),
            fmt(row["stale_diff"]["G derived"]), row["same_loss"],
            loss_tol(row["cost"]), row["same_grad"][0], row["same_grad"][1], row["free_loss"], T.ORACLE_F32_FREE_RUN[name]))
    _TABLE.update(rows)
    return _TABLE


def test_schedule_is_two_iterations_of_two_critic_updates_and_a_generator_update():
    want = []
    for it in range(T.ITERS):
        want += [("D", it, i) for i in range(T.CRITIC_ITERS)] + [("G", it, T.CRITIC_ITERS)]
    assert [u[1:] for u in T.SCHEDULE] == want and T.NAMES == ("D1", "D2", "G1", "D3", "D4", "G2")
    assert set(T.ORACLE_F32_FREE_RUN) == set(T.NAMES)
    assert [T.seed(it, i) for _, _, it, i in T.SCHEDULE] == [100, 101, 102, 103, 104, 105]
    assert (T.B, T.S, T.V, T.LAM) == (8, 64, 50, 10.0)


def test_losses_of_the_fp64_oracle_are_the_recorded_ones():
    """The first two columns of the table (to the digits it prints)."""
    rows = table()
    want = {"D1": (207.4247, 20.75, 0.005), "D2": (17.0511, 1.73, 0.005), "G1": (-0.1151, None, None), "D3": (12.5004, 1.18, 0.005),
            "D4": (0.7496, 0.052, 0.0005), "G2": (-0.5328, None, None)}          # (loss, penalty, half a unit of its last digit)
    for name, (cost, gp, half) in want.items():
        assert abs(rows[name]["cost"] - cost) <= 0.5e-4, (name, rows[name]["cost"])
        if gp is not None:
            assert abs(rows[name]["gp"] - gp) <= half, (name, rows[name]["gp"])


def test_gradient_penalty_is_active_in_every_critic_update():
    rows = table()
    for name in T.NAMES:
        if rows[name]["kind"] == "D":
            assert rows[name]["gp"] > 1e-3, (name, rows[name]["gp"])


def test_a_stale_network_is_visible_in_the_loss_from_the_second_update_on():
    rows = table()
    seen = 0
    for name in T.NAMES[1:]:
        row = rows[name]
        assert row["stale_diff"]["D"] is not None               # (the critic has been updated before every update but the first)
        assert (row["stale_diff"]["G"] is not None) == (name in ("D3", "D4", "G2"))
        assert all((row["stale_diff"][k + " derived"] is None) == (row["stale_diff"][k] is None) for k in "DG")
        for which, d in row["stale_diff"].items():
            if d is not None:
                seen += 1
                assert d > 1000.0 * loss_tol(row["cost"]), "%s with %s one update stale: the loss moves by %.3e only (loss_tol %.3e)" % (
                    name, which, d, loss_tol(row["cost"]))
    assert seen == 16


def test_same_state_fp32_oracle_is_inside_the_project_tolerances_at_every_update():
    rows = table()
    for name in T.NAMES:
        row = rows[name]
        assert row["same_loss"] <= loss_tol(row["cost"]), "%s: fp32 loss differs by %.3e (loss_tol %.3e)" % (
            name, row["same_loss"], loss_tol(row["cost"]))
        assert row["same_grad"][0] < GRAD_RTOL, "%s: gradient %s rel err %.3e" % (name, row["same_grad"][1], row["same_grad"][0])
        if row["kind"] == "D":
            assert row["bias"] < 1e-5, (name, row["bias"])


def test_free_running_fp32_oracle_is_within_half_the_gpu_tolerance():
    rows = table()
    for name in T.NAMES:
        assert rows[name]["free_loss"] <= 5.0 * T.ORACLE_F32_FREE_RUN[name], "%s: free-running fp32 loss differs by %.3e (recorded %.1e)" % (
            name, rows[name]["free_loss"], T.ORACLE_F32_FREE_RUN[name])
    # the tolerance the device gets (10 x) stays a factor 10 below the effect of a stale network at the same update, and a factor 2
    # below that of stale derived copies alone (smallest: G1, 2.9e-3 against 1.3e-3)
    for name in T.NAMES[1:]:
        for which, d in rows[name]["stale_diff"].items():
            if d is not None:
                assert 10.0 * T.ORACLE_F32_FREE_RUN[name] < d / (2.0 if "derived" in which else 10.0), (name, which, d)


def test_adam_expected_holds_for_fp32_emulations_of_the_kernel_on_second_update_state():
    """adam_expected / adam_check (the GPU test's Adam assertion) on what a step really feeds the optimiser: the fp32 oracle's state and
    gradient at each network's second update.  Both emulations of tests/optim_ref.py lie inside; one with the step count off by one,
    one with stale moments, one that ignores the gradient scale do not."""
    rows = table()
    for name in ("D2", "G2"):
        (p, m, v), g, t = rows[name]["adam"]
        assert t == 2 and np.abs(m).max() > 0 and np.abs(v).max() > 0
        tt = lambda *a: [torch.from_numpy(x) for x in a]
        lr_t = O.tf_adam_lr_t(t)
        for scale in (1.0, 0.5):
            for emulate in (R.emulate_every_rounding, R.emulate_fused):
                mv, vv, _, pn, _ = emulate(p, g, m, v, p, lr_t, O.ADAM_B1, O.ADAM_B2, O.ADAM_EPS, scale, 0.0)
                worst = T.adam_check(name, tt(p, m, v), torch.from_numpy(g), tt(pn, mv, vv), t, scale)
                print("%s gscale %g %s: worst err / bound  %s" % (name, scale, emulate.__name__, "  ".join("%s %.3f" % kv for kv in worst.items())))
                assert all(x <= 1.0 for x in worst.values()), (name, emulate.__name__, worst)
        # what the check is for
        mv, vv, _, pn, _ = R.emulate_every_rounding(p, g, m, v, p, O.tf_adam_lr_t(t - 1), O.ADAM_B1, O.ADAM_B2, O.ADAM_EPS, 1.0, 0.0)
        assert T.adam_check(name, tt(p, m, v), torch.from_numpy(g), tt(pn, mv, vv), t)["p"] > 1e3             # lr_t of the step before
        z = np.zeros_like(m)
        mv, vv, _, pn, _ = R.emulate_every_rounding(p, g, z, z, p, lr_t, O.ADAM_B1, O.ADAM_B2, O.ADAM_EPS, 1.0, 0.0)
        wrong = T.adam_check(name, tt(p, m, v), torch.from_numpy(g), tt(pn, mv, vv), t)
        assert min(wrong.values()) > 1e3, wrong                                                                    # moments lost
        mv, vv, _, pn, _ = R.emulate_every_rounding(p, g, m, v, p, lr_t, O.ADAM_B1, O.ADAM_B2, O.ADAM_EPS, 1.0, 0.0)
        assert min(T.adam_check(name, tt(p, m, v), torch.from_numpy(g), tt(pn, mv, vv), t, 0.5).values()) > 1e3   # scale 1 / N ignored


# ---- what a missing refresh would and would not do ---------------------------------------------------------------------------------
def test_derived_copies_are_rederived_through_arena_version_when_adam_step_does_not():
    """Network.adam_step bumps arena.version and then calls trunk.refresh_weights().  Leaving out the CALL alone changes no result:
    Trunk.forward / backward compare the plan's key with arena.version and re-derive first (the path of a second encoder on a shared
    arena).  The copies stay stale only if the version is not bumped either - then every convolution from conv1_2 on reads the weights
    of the update before (lib.conv_fwd passes w_fwd and the pre-split copy to the library, never the arena's tensor), the "derived"
    column of the table: 6.6e+1 on the loss of D2.  Host logic, on the CPU reference kernels (which take the HWOI transposes only)."""
    from oracle.kernels_ref import RefKernels
    from sgg_amd.step import GanStep
    dt, B, S, V = torch.float64, 2, 32, 11
    gp, dp = O.init_params("G", V, S, dtype=dt, perturb=0.1), O.init_params("D", V, S, dtype=dt, perturb=0.1)
    dp["W"] = dp["W"] * 25.0
    gs = GanStep(RefKernels(), V, S, B, lam=10.0, g_state=gp, d_state=dp, dtype=dt)
    images, labels, _ = O.synth_batch(B, S, V, dtype=dt)
    lay = gs.D.trunk.layers[3]
    stale = lambda: not torch.equal(lay["w_fwd"], lay["w"].permute(0, 1, 3, 2))
    version = gs.D.arena.version
    gs.D.trunk.refresh_weights = lambda: None            # (the plan is current throughout the update: only adam_step calls it)
    gs.critic_step(images, labels, O.synth_noise(B, 0, dt), O.synth_alpha(B, 0, dt).reshape(B))
    del gs.D.trunk.refresh_weights
    assert gs.D.adam_t == 1 and gs.D.arena.version == version + 1 and stale() and not gs.D.trunk.plan_current()
    gs.D.trunk.forward(images, False)
    assert not stale() and gs.D.trunk.plan_current()
    # ... and with the call in place nothing is left to the next forward
    gs.critic_step(images, labels, O.synth_noise(B, 1, dt), O.synth_alpha(B, 1, dt).reshape(B))
    assert gs.D.adam_t == 2 and not stale() and gs.D.trunk.plan_current()


# ---- the weight layouts of the test size cover those of the workload ---------------------------------------------------------------
def _layouts(L, S, precision):
    """{(conv index, direction): (layout, layout for a pre-split source)} for the encoder's live layers on an S x S image: the route
    query of the C ABI (no GPU), asked as trunk._query_layouts asks it - both directions with the layer's full-resolution grid, the
    dgrad with the channels swapped."""
    out, h = {}, S
    for (i, cin, cout, k, s, _, live) in CONV_SPECS:
        if not live:
            continue
        if cin != 3:                             # (conv1_1 keeps its f32 weights: nothing is derived for it)
            for direction, (a, b) in (("fwd", (cin, cout)), ("bwd", (cout, cin))):
                out[(i, direction)] = (L.sgg_conv_wsplit_layout(k, k, s, h, h, a, b, precision),
                                       L.sgg_conv_wsplit_layout_presplit(k, k, s, h, h, a, b, precision))
        h = same_pads(h, k, s)[0]
    return out


def test_layouts_at_64_px_are_those_of_the_224_px_workload():
    """refresh_weights / sgg_conv_prepare_weights derive one copy per layer and direction in the layout the routing names (1 / 2 / 3 / 4;
    0 = planes).  The layout is a function of the layer's kernel, channels and grid, not of the batch.  At 64 px every live layer and
    direction gets the layout it gets at 224 px (grids 64 .. 4 against 224 .. 14), with and without a pre-split source, in precision
    2; in precision 0 nothing is split at either size.  So 64 px alone covers the workload's weight layouts, and the GPU test needs no
    second size (section 3(d) of its plan is dropped)."""
    L = lib.load_library(build.build())
    small, work = _layouts(L, T.S, 2), _layouts(L, 224, 2)
    print("layouts at %d px, precision 2: %s" % (T.S, sorted(small.items())))
    assert len(small) == 22 and small == work, sorted(set(small.items()) ^ set(work.items()))
    assert {x for pair in work.values() for x in pair} == {1, 2, 3, 4}          # every fragment layout occurs
    assert _layouts(L, T.S, 0) == _layouts(L, 224, 0)
