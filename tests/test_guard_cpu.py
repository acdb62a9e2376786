"""CPU: guarded updates - global-norm clipping and the non-finite skip (sgg_amd/guard.py, step.Network.enable_guard) in fp64 on the
kernel-level reference: the restatement's known answers, the host logic of the step, accumulation, the data-parallel path over gloo,
the counters' round trip and the train.py flags.

What clipping can show.  Adam is invariant to a constant gradient scale: after the first step from zero state the parameters barely
depend on coef.  The observables are m (proportional to coef) and v (to coef^2) after the first update, and the parameters after a
second update taken with a different coef.

Bounds.  m and v against coef and coef^2 times the unguarded ones: both sides are a handful of fp64 operations on identical inputs,
1e-12 relative to the largest element.  Accumulated against whole batch and two ranks against one process: 1e-8, the bound and the
argument of tests/test_accumulate_cpu.py and tests/test_dp_gloo.py (the two sides differ by summation order only; the clip
coefficient is a smooth function of the gradient away from the threshold)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from oracle.kernels_ref import RefKernels
from sgg_amd import ema as E
from sgg_amd import guard as G
from sgg_amd.step import GanStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
S, V, B = 32, 11, 2
TOL, RTOL = 1e-8, 1e-12
NEW = ("grad_guard", "adam_guarded", "adam_ema_guarded")


class GuardRefKernels(RefKernels):
    """The kernel-level reference with torch versions of the guard's three entry points (csrc/guard.hip, csrc/optim.hip) in the
    arithmetic of its tensors (fp64 here: s_eff is NOT rounded to fp32), next to the others of csrc/optim.hip that the step needs;
    every call of a new entry point is recorded."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def grad_accumulate(self, acc, g, first=False):
        if first:
            acc.copy_(g)
        else:
            acc.add_(g)

    def adam_ema(self, params, grads, m, v, avg, lr_t, b1, b2, eps, grad_scale=1.0, one_minus_decay=0.0):
        self.adam(params, grads, m, v, lr_t, b1, b2, eps, grad_scale)
        avg.copy_(torch.from_numpy(E.reference_update(avg.numpy(), params.numpy(), one_minus_decay)))

    def swap(self, a, b):
        t = a.clone()
        a.copy_(b)
        b.copy_(t)

    def grad_guard(self, grads, record, grad_scale=1.0, max_norm=0.0, skip_nonfinite=False, ws=None, grid=0):
        self.calls.append("grad_guard")
        x = grads * grad_scale
        finite = torch.isfinite(x)
        ss, bad = float((x[finite] ** 2).sum()), float((~finite).sum())
        norm = ss ** 0.5
        coef = max_norm / norm if (max_norm > 0 and norm > max_norm) else 1.0
        apply = 0.0 if (skip_nonfinite and bad > 0) else 1.0
        record[:6] = torch.tensor([ss, bad, norm, coef, grad_scale * coef, apply], dtype=record.dtype)
        if coef < 1.0 and apply:
            record[6] += 1
        if not apply:
            record[7] += 1

    def adam_guarded(self, params, grads, m, v, lr_t, b1, b2, eps, record):
        self.calls.append("adam_guarded")
        if float(record[5]) != 0.0:
            self.adam(params, grads, m, v, lr_t, b1, b2, eps, float(record[4]))

    def adam_ema_guarded(self, params, grads, m, v, avg, lr_t, b1, b2, eps, record, one_minus_decay=0.0):
        self.calls.append("adam_ema_guarded")
        if float(record[5]) != 0.0:
            self.adam_ema(params, grads, m, v, avg, lr_t, b1, b2, eps, float(record[4]), one_minus_decay)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_reference_record_known_answers():
    g = np.array([3.0, -4.0], dtype=np.float32)
    above, equal, below, off = (G.reference_record(g, 1.0, mx, False) for mx in (10.0, 5.0, 2.5, 0.0))
    assert above.dtype == np.float64 and above.tolist() == [25.0, 0.0, 5.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert equal.tolist() == above.tolist() and equal[3] == 1.0, "at norm == max_norm nothing is clipped: coef is exactly 1"
    assert below.tolist() == [25.0, 0.0, 5.0, 0.5, 0.5, 1.0, 1.0, 0.0]
    assert off.tolist() == above.tolist(), "max_norm = 0 is no clipping"
    # the gradient scale enters the norm (x = g * grad_scale) and s_eff
    assert G.reference_record(g, 0.5, 1.25, True).tolist() == [6.25, 0.0, 2.5, 0.5, 0.25, 1.0, 1.0, 0.0]
    assert G.reference_record(g, -2.0, 0.0, False).tolist() == [100.0, 0.0, 10.0, 1.0, -2.0, 1.0, 0.0, 0.0]
    # s_eff is what fp32 holds of grad_scale * coef; coef itself stays fp64
    third = G.reference_record(g, 1.0, 5.0 / 3.0, False)
    assert third[3] == np.float64(np.float32(5.0 / 3.0)) / 5.0 and third[4] == np.float64(np.float32(third[3])) != third[3]


def test_reference_record_nonfinite_and_counters():
    g = np.array([3.0, np.nan, -4.0, np.inf, 0.0], dtype=np.float32)
    on, off = G.reference_record(g, 1.0, 2.5, True), G.reference_record(g, 1.0, 2.5, False)
    assert on.tolist() == [25.0, 2.0, 5.0, 0.5, 0.5, 0.0, 0.0, 1.0], "skipped, and a skipped update is not counted as clipped"
    assert off.tolist() == [25.0, 2.0, 5.0, 0.5, 0.5, 1.0, 1.0, 0.0], "skip off: the norm of the finite elements, applied"
    # a finite gradient that overflows under the scale is non-finite to the step, as the Adam pass would see it
    big = G.reference_record(np.array([3e38, 1.0], dtype=np.float32), 2.0, 0.0, True)
    assert big[:2].tolist() == [4.0, 1.0] and big[5] == 0.0
    # the counters are carried through prev, the other fields are overwritten
    rec = None
    for k, (arr, want) in enumerate([(g, (0, 1)), (g[[0, 2]], (1, 1)), (g[[0, 2]] * 0.1, (1, 1)), (g, (1, 2)), (g[[0, 2]], (2, 2))]):
        rec = G.reference_record(arr, 1.0, 2.5, True, prev=rec)
        assert (rec[6], rec[7]) == want, (k, rec)
    assert rec[:6].tolist() == [25.0, 0.0, 5.0, 0.5, 0.5, 1.0]


def test_decide_and_settings():
    assert G.decide(25.0, 0, 1.0, 10.0, True) == (5.0, 1.0, 1.0, 1.0)
    assert G.decide(25.0, 0, 1.0, 5.0, True) == (5.0, 1.0, 1.0, 1.0)
    assert G.decide(25.0, 3, 0.5, 2.5, True) == (5.0, 0.5, 0.25, 0.0)
    assert G.decide(25.0, 3, 0.5, 2.5, False) == (5.0, 0.5, 0.25, 1.0)
    assert G.decide(0.0, 0, 1.0, 1.0, True) == (0.0, 1.0, 1.0, 1.0), "a zero gradient is not clipped (no 0 / 0)"
    # grad_scale and max_norm are the fp32 values the kernel receives
    norm, coef, s_eff, _ = G.decide(2.0, 0, 0.1, 0.1, False)
    assert norm == np.sqrt(np.float64(2.0)) and coef == np.float64(np.float32(0.1)) / norm
    assert s_eff == np.float64(np.float32(np.float64(np.float32(0.1)) * coef))
    assert G.check_settings(0, 0) == (0.0, False) and G.check_settings("2.5", 1) == (2.5, True)
    for bad in (-1.0, float("nan"), float("inf"), -0.001, "x", None):
        with pytest.raises(ValueError):
            G.check_settings(bad)
    assert len(G.FIELDS) == G.NREC == 8


# ---- host logic in fp64 ---------------------------------------------------------------------------------------------------------
def _states():
    gp, dp_ = O.init_params("G", V, S, dtype=DT, perturb=0.1), O.init_params("D", V, S, dtype=DT, perturb=0.1)
    dp_["W"] = dp_["W"] * 25.0               # (the penalty is active: slopes above 1, as in tests/test_dp_gloo.py)
    return gp, dp_


def _draw(rows):
    images, labels, _ = O.synth_batch(rows, S, V, dtype=DT)
    noise = lambda seed: O.synth_noise(rows, seed, DT)
    alpha = lambda seed: O.synth_alpha(rows, seed, DT).reshape(rows)
    return images, labels, noise, alpha


def _fresh(rows=B, guard=None, K=None, decay=None, reducer=None):
    """guard: None (never enabled) or (max_norm or (critic's, generator's), skip_nonfinite)."""
    gp, dp_ = _states()
    gs = GanStep(K if K is not None else GuardRefKernels(), V, S, rows, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer)
    if decay is not None:
        gs.G.enable_averaging(decay)
    if guard is not None:
        gs.set_guard(*guard)
    return gs


def _snap(gs):
    gs.flush()
    out = {}
    for n, net in (("G", gs.G), ("D", gs.D)):
        out[n], out[n + ".m"], out[n + ".v"] = net.arena.flat.clone(), net.m_flat.clone(), net.v_flat.clone()
    out["losses"] = torch.cat([gs.d_losses, gs.g_losses]).clone()
    return out


def _iteration(gs, it=0, critic_iters=2):
    images, labels, noise, alpha = _draw(gs.B)
    gs.train_iteration(images, labels, [noise(10 * it + i) for i in range(critic_iters + 1)],
                       [alpha(10 * it + i) for i in range(critic_iters)], critic_iters=critic_iters)


_PLAIN = {}


def plain():
    """The unguarded run, once for the module: an iteration with two critic updates on the kernel set that HAS the entry points."""
    if not _PLAIN:
        gs = _fresh()
        _iteration(gs)
        _PLAIN.update(gs=gs, snap=_snap(gs), calls=list(gs.K.calls))
    return _PLAIN


def test_never_enabled_calls_none_of_the_new_entry_points():
    p = plain()
    assert p["calls"] == [], "an unguarded step called %s" % p["calls"]
    gs = p["gs"]
    assert not gs.G.has_guard and not gs.D.has_guard and "guard" not in gs.G.opt and "guard" not in gs.D.opt
    assert gs.guard_reports() == {}
    for call in (gs.G.guard_report, gs.G.guard_state, lambda: gs.G.restore_guard(1, 2)):
        with pytest.raises(RuntimeError, match="enable_guard"):
            call()


def test_a_kernel_set_without_the_entry_points_is_refused():
    gs = _fresh(K=RefKernels())
    with pytest.raises(RuntimeError, match="grad_guard"):
        gs.D.enable_guard(1.0)
    with pytest.raises(RuntimeError, match="grad_guard"):
        gs.set_guard(1.0, True)
    assert not gs.D.has_guard and not gs.G.has_guard
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _fresh().D.enable_guard(bad)


def test_unreachable_threshold_is_the_unguarded_run_bit_for_bit():
    want = plain()["snap"]
    gs = _fresh(guard=(1e30, True))
    _iteration(gs)
    got = _snap(gs)
    for key in want:
        assert torch.equal(got[key].view(torch.int64), want[key].view(torch.int64)), "%s differs from the unguarded run" % key
    # ... and it did go through the guarded kernels: one decision and one guarded pass per update
    assert gs.K.calls == ["grad_guard", "adam_guarded"] * 3
    rep = gs.guard_reports()
    for n, net in (("D", gs.D), ("G", gs.G)):
        r = rep[n]
        assert r == net.guard_report()
        assert r["coef"] == 1.0 and r["apply"] is True and r["clipped"] == r["skipped"] == r["nonfinite"] == 0 and r["norm"] > 0
        assert r["max_norm"] == 1e30 and r["skip_nonfinite"] is True
    # set_guard with both controls off puts the plain pass back
    gs.set_guard(0.0, False)
    assert not gs.D.has_guard and not gs.G.has_guard


def _first_update(which, guard=None):
    """The FIRST update of network `which` from the initial state of both (identical inputs whatever the guard), then a second
    one with other noise.  Returns (net, m, v and gradient norm after the first, parameters after the second, reports)."""
    gs = _fresh(guard=guard)
    images, labels, noise, alpha = _draw(B)
    net = gs.D if which == "D" else gs.G
    step = (lambda s: gs.critic_step(images, labels, noise(s), alpha(s))) if which == "D" else (lambda s: gs.generator_step(images, noise(s)))
    step(0)
    first = {"m": net.m_flat.clone(), "v": net.v_flat.clone(), "norm": float(net.arena.live(net.grad_flat).pow(2).sum().sqrt()),
             "report": net.guard_report() if guard is not None else None}
    step(1)
    first.update(p2=net.arena.flat.clone(), report2=net.guard_report() if guard is not None else None)
    return first


@pytest.mark.parametrize("which", ["D", "G"])
def test_active_clipping_scales_the_moments_by_coef(which):
    u = _first_update(which)
    assert u["norm"] > 0
    max_norm = u["norm"] / 4.0
    c = _first_update(which, guard=(max_norm, False))
    r = c["report"]
    assert r["apply"] is True and r["clipped"] == 1 and r["skipped"] == 0
    assert abs(r["norm"] - u["norm"]) <= RTOL * u["norm"]
    coef = r["coef"]
    assert abs(coef - 0.25) <= RTOL and r["s_eff"] == coef
    for key, factor in (("m", coef), ("v", coef * coef)):
        scale = float(u[key].abs().max())
        assert scale > 0
        err = float((c[key] - factor * u[key]).abs().max())
        print("%s %s: max |guarded - %s * unguarded| = %.3e (largest element %.3e)" % (which, key, "coef" if key == "m" else "coef^2",
                                                                                     err, scale))
        assert err <= RTOL * scale, (which, key, err, scale)
        # (unclipped moments are far outside that bound: the comparison can fail)
        assert float((c[key] - u[key]).abs().max()) > 1e3 * RTOL * scale
    # the second update meets the threshold with ANOTHER coefficient (1 where its norm is below it): now the parameters show it
    r2 = c["report2"]
    assert r2["clipped"] in (1, 2) and (r2["coef"] < 1.0) == (r2["clipped"] == 2) and abs(r2["coef"] - coef) > 1e3 * RTOL
    diff, scale = float((c["p2"] - u["p2"]).abs().max()), float(u["p2"].abs().max())
    print("%s parameters after two updates: guarded vs unguarded differ by %.3e (largest element %.3e)" % (which, diff, scale))
    assert diff > 1e3 * RTOL * scale


# ---- accumulation and data parallel -------------------------------------------------------------------------------------------------
CLIP = (2.0, 0.5)      # (critic's, generator's): below every update's norm in the runs underneath - each asserts that all were clipped


def _full(rows):
    gs = _fresh(rows, guard=(CLIP, True))
    images, labels, noise, alpha = _draw(rows)
    gs.critic_step(images, labels, noise(0), alpha(0))
    gs.generator_step(images, noise(1))
    gs.train_iteration(images, labels, [noise(10 + i) for i in range(3)], [alpha(10 + i) for i in range(2)], critic_iters=2)
    gs.flush()
    return gs, {"D": gs.D.arena.flat.clone(), "G": gs.G.arena.flat.clone(), "d1": gs.d_losses.clone(), "g1": gs.g_losses.clone()}


def _accumulated(rows, Bm, pick, reducer=None):
    N = len(pick)
    images, labels, noise, alpha = _draw(rows)
    cut = lambda t, k: t[pick[k]].contiguous()
    batches = [(cut(images, k), cut(labels, k)) for k in range(N)]
    gs = _fresh(Bm, guard=(CLIP, True), reducer=reducer)
    for k in range(N):
        gs.critic_step(batches[k][0], batches[k][1], cut(noise(0), k), cut(alpha(0), k), micro=(k, N))
    for k in range(N):
        gs.generator_step(batches[k][0], cut(noise(1), k), micro=(k, N))
    noises = [[cut(noise(10 + i), k) for k in range(N)] for i in range(3)]
    alphas = [[cut(alpha(10 + i), k) for k in range(N)] for i in range(2)]
    gs.train_iteration_accumulated(batches, noises, alphas, critic_iters=2)
    gs.flush()
    return gs, {"D": gs.D.arena.flat.clone(), "G": gs.G.arena.flat.clone(), "d1": gs.d_losses_mean.clone(), "g1": gs.g_losses_mean.clone()}


_FULL = {}


def full(rows):
    if rows not in _FULL:
        gs, out = _full(rows)
        rep = gs.guard_reports()
        assert rep["D"]["clipped"] == gs.D.adam_t == 3 and rep["G"]["clipped"] == gs.G.adam_t == 2, \
            "CLIP is not below every update's norm at %d rows: %s" % (rows, rep)
        assert rep["D"]["skipped"] == rep["G"]["skipped"] == 0
        _FULL[rows] = out
    return _FULL[rows]


def test_accumulated_clipped_update_equals_the_large_batch_clipped_update():
    pick = [list(range(k * B, (k + 1) * B)) for k in range(2)]
    gs, got = _accumulated(4, B, pick)
    want = full(4)
    for key in ("D", "G", "d1", "g1"):
        err = float((got[key] - want[key]).abs().max())
        print("%s: N = 2 x B = 2 clipped vs B = 4 clipped differ by %.3e" % (key, err))
        assert err < TOL, (key, err)
    rep = gs.guard_reports()
    assert rep["D"]["clipped"] == 3 and rep["G"]["clipped"] == 2
    # the guard saw the MEAN gradient: grad_flat holds the sum over the two micro-batches, the scale was 1 / 2
    for n, net in (("D", gs.D), ("G", gs.G)):
        host = float(net.arena.live(net.grad_flat).pow(2).sum().sqrt()) * 0.5
        assert abs(rep[n]["norm"] - host) <= RTOL * host and abs(rep[n]["s_eff"] - 0.5 * rep[n]["coef"]) <= 1e-16
    # the unclipped run is far outside the bound: the test can fail
    ugs = _fresh(4)
    images, labels, noise, alpha = _draw(4)
    ugs.critic_step(images, labels, noise(0), alpha(0))
    ugs.generator_step(images, noise(1))
    ugs.train_iteration(images, labels, [noise(10 + i) for i in range(3)], [alpha(10 + i) for i in range(2)], critic_iters=2)
    ugs.flush()
    assert float((ugs.D.arena.flat - want["D"]).abs().max()) > 1e3 * TOL


def _dp_pick(rank, world, Bm, N):
    return [list(range(k * world * Bm + rank * Bm, k * world * Bm + (rank + 1) * Bm)) for k in range(N)]


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sgg_amd  # noqa: F401
    from sgg_amd import dp
    torch.set_num_threads(2)
    dp.init_from_env(backend="gloo")
    gs, res = _accumulated(8, 2, _dp_pick(rank, world, 2, 2), reducer=dp.GradReducer())
    res["reports"] = gs.guard_reports()
    torch.save(res, out % rank)
    torch.distributed.destroy_process_group()


def test_two_ranks_take_the_same_decision_and_equal_the_single_process(tmp_path):
    out = str(tmp_path / "rank%d.pt")
    port = 35500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(r0["D"], r1["D"]) and torch.equal(r0["G"], r1["G"]), "replicas diverged"
    assert r0["reports"] == r1["reports"], "the ranks' records differ: they reduced to different bits"
    assert r0["reports"]["D"]["clipped"] == 3 and r0["reports"]["G"]["clipped"] == 2
    want = full(8)
    for key in ("D", "G"):
        err = float((r0[key] - want[key]).abs().max())
        print("%s weights: world 2 x N 2 x B 2 clipped vs 8 rows clipped differ by %.3e" % (key, err))
        assert err < TOL, (key, err)


# ---- the skip -------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int64)


@pytest.mark.parametrize("which", ["G", "D"])
def test_a_nonfinite_gradient_drops_the_update_and_the_next_one_applies(which):
    gs = _fresh(guard=(0.0, True), decay=0.9)        # (G keeps an average: its dropped update must not touch it either)
    images, labels, noise, alpha = _draw(B)
    net = gs.G if which == "G" else gs.D
    step = (lambda s: gs.critic_step(images, labels, noise(s), alpha(s))) if which == "D" else (lambda s: gs.generator_step(images, noise(s)))
    step(0)                                           # a clean update first: m and v are not zero
    assert net.guard_report()["apply"] is True and net.adam_t == 1
    avg = net.opt.get("ema")
    assert (avg is not None) == (which == "G")
    keep = [t.clone() for t in (net.arena.flat, net.m_flat, net.v_flat)] + ([avg["flat"].clone()] if avg else [])
    updates, version = (avg["updates"] if avg else None), net.arena.version
    net.grad_flat[5] = float("nan")
    net.adam_step()
    now = [net.arena.flat, net.m_flat, net.v_flat] + ([avg["flat"]] if avg else [])
    for name, a, b in zip(("arena", "m", "v", "average"), now, keep):
        assert torch.equal(_bits(a), _bits(b)), "%s changed in a dropped update" % name
    assert net.adam_t == 2 and net.arena.version == version + 1, "the dropped step consumes its number"
    if avg:
        assert avg["updates"] == updates + 1
    r = net.guard_report()
    assert r["apply"] is False and r["skipped"] == 1 and r["nonfinite"] == 1 and r["clipped"] == 0
    assert gs.K.calls[-2:] == ["grad_guard", "adam_ema_guarded" if avg else "adam_guarded"]
    step(1)                                           # the next clean update applies
    r = net.guard_report()
    assert r["apply"] is True and r["skipped"] == 1 and r["nonfinite"] == 0 and net.adam_t == 3
    assert not torch.equal(net.arena.flat, keep[0]) and not torch.equal(net.m_flat, keep[1])
    assert bool(torch.isfinite(net.arena.flat).all()) and bool(torch.isfinite(net.m_flat).all())
    if avg:
        assert not torch.equal(avg["flat"], keep[3]) and avg["updates"] == updates + 2
    # with the skip OFF the same gradient is applied, as without a guard: the NaN reaches the arena
    net.enable_guard(0.0, False)
    net.grad_flat[5] = float("nan")
    net.adam_step()
    r = net.guard_report()
    assert r["apply"] is True and r["nonfinite"] == 1 and r["skipped"] == 1 and bool(torch.isnan(net.arena.flat[5]))


def test_counters_survive_a_checkpoint_round_trip(tmp_path):
    gs = _fresh(guard=((1e-3, 0.0), True))
    images, labels, noise, alpha = _draw(B)
    gs.critic_step(images, labels, noise(0), alpha(0))
    gs.D.grad_flat[0] = float("inf")
    gs.D.adam_step()
    st = {n: net.guard_state() for n, net in (("D", gs.D), ("G", gs.G))}
    assert st == {"D": {"clipped": 1, "skipped": 1}, "G": {"clipped": 0, "skipped": 0}}
    path = str(tmp_path / "ck.pt")
    torch.save({"guard": st}, path)
    saved = torch.load(path)["guard"]
    twin = _fresh(guard=((1e-3, 0.0), True))
    twin.D.restore_guard(**saved["D"])
    twin.G.restore_guard(**saved["G"])
    assert twin.D.guard_state() == st["D"] and twin.G.guard_state() == st["G"]
    twin.critic_step(images, labels, noise(0), alpha(0))
    assert twin.D.guard_state() == {"clipped": 2, "skipped": 1}, "the restored counters do not go on counting"
    # a changed setting keeps the counters; disabling frees them
    twin.D.enable_guard(5.0, False)
    assert twin.D.guard_state() == {"clipped": 2, "skipped": 1} and twin.D.guard_report()["max_norm"] == 5.0
    twin.D.disable_guard()
    twin.D.enable_guard(5.0, False)
    assert twin.D.guard_state() == {"clipped": 0, "skipped": 0}


# ---- train.py -------------------------------------------------------------------------------------------------------------------
def test_parser_and_constructor_know_the_flags():
    sys.path.insert(0, ROOT)
    import train as T
    args = T.build_parser().parse_args([])
    assert args.clip_grad_norm == (0.0, 0.0) and args.skip_nonfinite is False
    assert T.build_parser().parse_args(["--clip_grad_norm", "5"]).clip_grad_norm == (5.0, 5.0)
    assert T.build_parser().parse_args(["--clip_grad_norm", "5,0.5", "--skip_nonfinite"]).clip_grad_norm == (5.0, 0.5)
    assert T.build_parser().parse_args(["--clip_grad_norm", "0"]).clip_grad_norm == (0.0, 0.0)
    assert T.build_parser().parse_args(["--clip_grad_norm", "0,3"]).clip_grad_norm == (0.0, 3.0)
    assert T.build_parser().parse_args(["--skip_nonfinite"]).skip_nonfinite is True
    for bad in ("-1", "nan", "1,-2", "inf", "1,2,3", "", "1,", "x"):
        with pytest.raises(SystemExit):
            T.build_parser().parse_args(["--clip_grad_norm=" + bad])
    assert G.parse_clip_grad_norm(2) == (2.0, 2.0) and G.parse_clip_grad_norm("1e-3, 4") == (1e-3, 4.0)
    for bad in (-1.0, float("nan"), (1.0, -2.0), "1,2,3"):
        with pytest.raises(ValueError, match="clip"):
            T.SceneGraphGAN("ck", "logs", None, None, None, None, None, critic_iters=1, batch_size=4, lambda_=10, resume=False,
                            synthetic=(4, 32, 11), clip_grad_norm=bad)
