"""CPU: gradient accumulation - one update from N micro-batches (step.Network.end_micro_batch, GanStep.train_iteration_accumulated) in
fp64 on the kernel-level reference, the data-parallel path over gloo, G-encoder reuse per micro-batch, the order of the example
stream and the train.py flags.

The exactness argument under test: no op couples samples and every loss term is a mean over rows, so with N micro-batches of B rows
(1 / N) * sum_k grad(micro-batch k) is the gradient of the N * B rows, and the same holds for the four loss numbers.  In fp64 the two
sides differ by summation order only: 1e-8, the bound tests/test_dp_gloo.py holds the same argument to across ranks."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from oracle.kernels_ref import RefKernels
from sgg_amd.step import GanStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
S, V = 32, 11
TOL = 1e-8


class AccRefKernels(RefKernels):
    """The kernel-level reference with the entry point of gradient accumulation: a torch add (first: a copy)."""

    def grad_accumulate(self, acc, g, first=False):
        if first:
            acc.copy_(g)
        else:
            acc.add_(g)


def _states():
    gp, dp_ = O.init_params("G", V, S, dtype=DT, perturb=0.1), O.init_params("D", V, S, dtype=DT, perturb=0.1)
    dp_["W"] = dp_["W"] * 25.0               # (the penalty is active: slopes above 1, as in tests/test_dp_gloo.py)
    return gp, dp_


def _draw(rows):
    """One seeded draw of `rows` rows: images, labels, and noise / alpha by seed."""
    images, labels, _ = O.synth_batch(rows, S, V, dtype=DT)
    noise = lambda seed: O.synth_noise(rows, seed, DT)
    alpha = lambda seed: O.synth_alpha(rows, seed, DT).reshape(rows)
    return images, labels, noise, alpha


def _full(rows, K=None):
    """The yardstick: GanStep(B = rows) on all rows - a critic step, a generator step, then an iteration with two critic updates."""
    gp, dp_ = _states()
    images, labels, noise, alpha = _draw(rows)
    gs = GanStep(K if K is not None else RefKernels(), V, S, rows, g_state=gp, d_state=dp_, dtype=DT)
    out = {}
    gs.critic_step(images, labels, noise(0), alpha(0))
    out["d0"] = gs.d_losses.clone()
    gs.generator_step(images, noise(1))
    out["g0"] = gs.g_losses.clone()
    gs.train_iteration(images, labels, [noise(10 + i) for i in range(3)], [alpha(10 + i) for i in range(2)], critic_iters=2)
    gs.flush()
    out.update(d1=gs.d_losses.clone(), g1=gs.g_losses.clone(), D=gs.D.arena.flat.clone(), G=gs.G.arena.flat.clone())
    return out


def _accumulated(rows, B, pick, reducer=None, K=None, reuse=False):
    """The same three stages from N micro-batches of B rows of the same draw; pick(k) -> the row indices of micro-batch k."""
    N = len(pick)
    gp, dp_ = _states()
    images, labels, noise, alpha = _draw(rows)
    cut = lambda t, k: t[pick[k]].contiguous()
    batches = [(cut(images, k), cut(labels, k)) for k in range(N)]
    gs = GanStep(K if K is not None else AccRefKernels(), V, S, B, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer)
    out = {}
    for k in range(N):
        gs.critic_step(batches[k][0], batches[k][1], cut(noise(0), k), cut(alpha(0), k), micro=(k, N))
    out["d0"] = gs.d_losses_mean.clone()
    for k in range(N):
        gs.generator_step(batches[k][0], cut(noise(1), k), micro=(k, N))
    out["g0"] = gs.g_losses_mean.clone()
    noises = [[cut(noise(10 + i), k) for k in range(N)] for i in range(3)]
    alphas = [[cut(alpha(10 + i), k) for k in range(N)] for i in range(2)]
    gs.train_iteration_accumulated(batches, noises, alphas, critic_iters=2, reuse_g_encoder=reuse)
    gs.flush()
    out.update(d1=gs.d_losses_mean.clone(), g1=gs.g_losses_mean.clone(), D=gs.D.arena.flat.clone(), G=gs.G.arena.flat.clone())
    return gs, out


_FULL = {}


def full(rows):
    if rows not in _FULL:
        _FULL[rows] = _full(rows)
    return _FULL[rows]


def _compare(got, want, what):
    for key in ("D", "G", "d0", "g0", "d1", "g1"):
        err = float((got[key] - want[key]).abs().max())
        assert err < TOL, "%s: %s differs by %.3e" % (what, key, err)


# ---- equivalence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(2, 2), (1, 4)], ids=["2x2", "4x1"])
def test_accumulated_update_equals_the_large_batch_update(B, N):
    """N micro-batches of B rows against GanStep(B = 4) on all four rows: every weight of both networks and the four loss means.
    (The reference kernels accept a single row: the N = 4 x B = 1 case runs.)"""
    pick = [list(range(k * B, (k + 1) * B)) for k in range(N)]
    gs, got = _accumulated(4, B, pick)
    want = full(4)
    _compare(got, want, "N = %d x B = %d" % (N, B))
    assert gs.D.adam_t == 3 and gs.G.adam_t == 2
    assert "acc" in gs.D.opt and "acc" in gs.G.opt
    # the penalty was active, the update moved the weights, and a run on HALF the rows is far outside the bound: the test can fail
    assert float(want["d0"][2]) > 1e-3, "the gradient penalty is inactive"
    half = _full(2)
    assert float((half["D"] - want["D"]).abs().max()) > 1e3 * TOL and float((half["d0"] - want["d0"]).abs().max()) > 1e3 * TOL


def test_without_accumulation_nothing_is_allocated_and_the_means_alias():
    gp, dp_ = _states()
    images, labels, noise, alpha = _draw(4)
    gs = GanStep(RefKernels(), V, S, 4, g_state=gp, d_state=dp_, dtype=DT)        # (a kernel set WITHOUT grad_accumulate)
    gs.critic_step(images, labels, noise(0), alpha(0))
    gs.generator_step(images, noise(1))
    assert gs.d_losses_mean is gs.d_losses and gs.g_losses_mean is gs.g_losses
    assert "acc" not in gs.D.opt and "acc" not in gs.G.opt and not gs._loss_acc and "pending_scale" not in gs.D.opt
    with pytest.raises(RuntimeError, match="grad_accumulate"):
        gs.critic_step(images, labels, noise(0), alpha(0), micro=(0, 2))


# ---- the new entry point with one micro-batch ---------------------------------------------------------------------------------------
def test_one_micro_batch_is_train_iteration():
    images, labels, noise, alpha = _draw(4)
    noises, alphas = [noise(10 + i) for i in range(3)], [alpha(10 + i) for i in range(2)]
    runs = []
    for accumulated in (False, True):
        gp, dp_ = _states()
        gs = GanStep(AccRefKernels(), V, S, 4, g_state=gp, d_state=dp_, dtype=DT)
        for it in range(2):
            if accumulated:
                gs.train_iteration_accumulated([(images, labels)], [[n] for n in noises], [[a] for a in alphas], critic_iters=2,
                                               reuse_g_encoder=True)
            else:
                gs.train_iteration(images, labels, noises, alphas, critic_iters=2, reuse_g_encoder=True)
        gs.flush()
        runs.append(gs)
    a, b = runs
    assert "acc" not in b.D.opt and "acc" not in b.G.opt and b.d_losses_mean is b.d_losses
    for x, y in ((a.G, b.G), (a.D, b.D)):
        assert torch.equal(x.arena.flat, y.arena.flat) and torch.equal(x.m_flat, y.m_flat) and torch.equal(x.v_flat, y.v_flat)
        assert x.adam_t == y.adam_t
    assert torch.equal(a.d_losses, b.d_losses) and torch.equal(a.g_losses, b.g_losses)


# ---- data parallel over gloo ----------------------------------------------------------------------------------------------------
def _dp_pick(rank, world, B, N):
    """Micro-batch k of the global draw is rows [k * world * B, (k + 1) * world * B); rank r takes its rows [r * B, (r + 1) * B)."""
    return [list(range(k * world * B + rank * B, k * world * B + (rank + 1) * B)) for k in range(N)]


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sgg_amd  # noqa: F401
    from sgg_amd import dp
    torch.set_num_threads(2)
    dp.init_from_env(backend="gloo")
    gs, res = _accumulated(8, 2, _dp_pick(rank, world, 2, 2), reducer=dp.GradReducer())
    torch.save(res, out % rank)
    torch.distributed.destroy_process_group()


def test_two_ranks_times_two_micro_batches_equal_the_single_process_batch(tmp_path):
    out = str(tmp_path / "rank%d.pt")
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(r0["D"], r1["D"]) and torch.equal(r0["G"], r1["G"]), "replicas diverged"
    want = full(8)
    for key in ("D", "G"):
        err = float((r0[key] - want[key]).abs().max())
        assert err < TOL, "%s weights: world 2 x N 2 x B 2 vs 8 rows differ by %.3e" % (key, err)
    # (each rank's loss means cover ITS four rows; their mean over the ranks is the number of the eight)
    for key in ("d0", "g0", "d1", "g1"):
        err = float(((r0[key] + r1[key]) / 2 - want[key]).abs().max())
        assert err < TOL, "%s: %.3e" % (key, err)


# ---- one collective and one optimiser step per update -------------------------------------------------------------------------------
class _Pending:
    def __init__(self, log, kind):
        self.log, self.kind = log, kind

    def wait(self):
        self.log.append(("wait", self.kind))
        return 1.0


def test_one_collective_per_network_per_update_after_the_last_micro_batch(monkeypatch):
    from sgg_amd import step as step_mod
    log = []
    reducer = lambda net: (log.append(("reduce", net.kind)), _Pending(log, net.kind))[1]
    orig = step_mod.Network.end_micro_batch

    def spy(self, k, N, red):
        log.append(("micro", self.kind, k, N))
        return orig(self, k, N, red)

    monkeypatch.setattr(step_mod.Network, "end_micro_batch", spy)
    N, C, I, B = 2, 2, 2, 2
    gp, dp_ = _states()
    images, labels, noise, alpha = _draw(4)
    batches = [(images[k * B:(k + 1) * B], labels[k * B:(k + 1) * B]) for k in range(N)]
    gs = GanStep(AccRefKernels(), V, S, B, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer)
    for it in range(I):
        noises = [[noise(10 * it + i)[k * B:(k + 1) * B] for k in range(N)] for i in range(C + 1)]
        alphas = [[alpha(10 * it + i)[k * B:(k + 1) * B] for k in range(N)] for i in range(C)]
        gs.train_iteration_accumulated(batches, noises, alphas, critic_iters=C)
    gs.flush()
    assert gs.D.adam_t == C * I and gs.G.adam_t == I
    assert "pending_scale" not in gs.D.opt and "pending_scale" not in gs.G.opt
    events = [e for e in log if e[0] != "wait"]
    update = lambda kind: [("micro", kind, k, N) for k in range(N)] + [("reduce", kind)]
    assert events == (update("D") * C + update("G")) * I, events
    assert sum(e == ("wait", "D") for e in log) == C * I and sum(e == ("wait", "G") for e in log) == I
    # the reducer's scale (1.0 here) reaches the Adam pass multiplied by 1 / N: the result is the one without a reducer
    twin = GanStep(AccRefKernels(), V, S, B, g_state=gp, d_state=dp_, dtype=DT)
    for it in range(I):
        noises = [[noise(10 * it + i)[k * B:(k + 1) * B] for k in range(N)] for i in range(C + 1)]
        alphas = [[alpha(10 * it + i)[k * B:(k + 1) * B] for k in range(N)] for i in range(C)]
        twin.train_iteration_accumulated(batches, noises, alphas, critic_iters=C)
    assert torch.equal(twin.D.arena.flat, gs.D.arena.flat) and torch.equal(twin.G.arena.flat, gs.G.arena.flat)


# ---- G-encoder reuse per micro-batch -----------------------------------------------------------------------------------------------
def _count_g_forwards(gs):
    calls, orig = [], gs.G.trunk.forward

    def counted(images, for_backward=True, **kw):
        calls.append(bool(for_backward))
        return orig(images, for_backward, **kw)

    gs.G.trunk.forward = counted
    return calls


def test_reuse_runs_the_generator_encoder_2n_times_and_changes_nothing():
    N, C, B = 2, 3, 2
    images, labels, noise, alpha = _draw(4)
    batches = [(images[k * B:(k + 1) * B].clone(), labels[k * B:(k + 1) * B].clone()) for k in range(N)]
    noises = [[noise(20 + i)[k * B:(k + 1) * B] for k in range(N)] for i in range(C + 1)]
    alphas = [[alpha(20 + i)[k * B:(k + 1) * B] for k in range(N)] for i in range(C)]
    res = {}
    for reuse in (False, True):
        gp, dp_ = _states()
        gs = GanStep(AccRefKernels(), V, S, B, g_state=gp, d_state=dp_, dtype=DT)
        calls = _count_g_forwards(gs)
        for it in range(2):
            del calls[:]
            gs.train_iteration_accumulated(batches, noises, alphas, critic_iters=C, reuse_g_encoder=reuse)
            assert len(calls) == (2 * N if reuse else N * (C + 1)), (reuse, calls)
            assert sum(calls) == N, "the generator update runs the encoder afresh, once per micro-batch, for its backward"
        assert not gs._g_reuse_slots and gs._g_reuse is None and not gs._g_reuse_armed
        res[reuse] = gs
    a, b = res[False], res[True]
    assert torch.equal(a.G.arena.flat, b.G.arena.flat) and torch.equal(a.D.arena.flat, b.D.arena.flat)
    assert torch.equal(a.d_losses_mean, b.d_losses_mean) and torch.equal(a.g_losses_mean, b.g_losses_mean)


def test_reuse_guard_trips_on_a_micro_batch_modified_in_place():
    N, B = 2, 2
    gp, dp_ = _states()
    images, labels, noise, alpha = _draw(4)
    batches = [(images[k * B:(k + 1) * B].clone(), labels[k * B:(k + 1) * B].clone()) for k in range(N)]
    gs = GanStep(AccRefKernels(), V, S, B, g_state=gp, d_state=dp_, dtype=DT)
    cut = lambda t, k: t[k * B:(k + 1) * B]
    with gs.iteration(reuse_g_encoder=True):
        for k in range(N):
            gs.critic_step(batches[k][0], batches[k][1], cut(noise(0), k), cut(alpha(0), k), micro=(k, N))
        gs.critic_step(batches[0][0], batches[0][1], cut(noise(1), 0), cut(alpha(1), 0), micro=(0, N))     # untouched: reused
        batches[1][0].mul_(1.5)
        with pytest.raises(AssertionError, match="micro-batch 1 was modified in place"):
            gs.critic_step(batches[1][0], batches[1][1], cut(noise(1), 1), cut(alpha(1), 1), micro=(1, N))
    assert not gs._g_reuse_slots


# ---- order of the example stream ----------------------------------------------------------------------------------------------------
def test_an_iteration_reads_a_contiguous_range_of_the_stream(tmp_path):
    sys.path.insert(0, ROOT)
    import train as T
    from sgg_amd.data import PrefetchLoader, ShuffledStream
    n, B, N, world = 37, 3, 4, 2
    mk = lambda: ShuffledStream(n, 10 * B * world, seed=5)
    st = mk()
    for it in (0, 1, 5):
        ms = list(T.micro_batch_ids(it, N))
        assert ms == [it * N + k for k in range(N)]
        got = [i for m in ms for rank in range(world) for i in st.batch(m, B, rank, world)]
        want = mk().take(it * N * B * world, N * B * world)
        assert got == want, "iteration %d does not cover stream elements [%d, %d)" % (it, it * N * B * world, (it + 1) * N * B * world)
    assert list(T.micro_batch_ids(7, 1)) == [7], "N = 1: micro-batch = iteration, the order of a run without accumulation"
    # a loader started at itr * N (a resumed run) hands out exactly those micro-batches, in order
    from PIL import Image
    rng = np.random.RandomState(1)
    files = []
    for i in range(n):
        p = os.path.join(str(tmp_path), "im%03d.jpg" % i)
        Image.fromarray((rng.rand(12, 10, 3) * 255).astype(np.uint8)).save(p)
        files.append(p)
    labels = np.arange(n * 3).reshape(n, 3)
    means, stds = np.array([120.0, 115.0, 100.0], np.float32), np.array([60.0, 58.0, 61.0], np.float32)
    itr, n_it, rank = 2, 4, 1
    loader_stream = mk()
    loader = PrefetchLoader(files, labels, B, lambda m: loader_stream.batch(m, B, rank, world), means, stds, "cpu", n_it * N,
                            start=itr * N, workers=2, side=9)
    got = [labs.numpy() for _, labs in loader]
    assert len(got) == (n_it - itr) * N
    for j, labs in enumerate(got):
        it, k = itr + j // N, j % N
        assert np.array_equal(labs, labels[st.batch(list(T.micro_batch_ids(it, N))[k], B, rank, world)])


# ---- train.py -------------------------------------------------------------------------------------------------------------------
def test_parser_and_constructor_know_accumulate():
    sys.path.insert(0, ROOT)
    import train as T
    assert T.build_parser().parse_args([]).accumulate == 1
    assert T.build_parser().parse_args(["--accumulate", "8"]).accumulate == 8
    for bad in (0, -2):
        with pytest.raises(ValueError, match="accumulate"):
            T.SceneGraphGAN("ck", "logs", None, None, None, None, None, critic_iters=1, batch_size=4, lambda_=10, resume=False,
                            synthetic=(4, 32, 11), accumulate=bad)
