"""CPU: weight averaging - the schedule and the fp64 restatement (sgg_amd/ema.py), the rounding bound the GPU tests use (checked from
the reference alone), the host logic of step.Network (enable_averaging / adam_step / averaged()) in fp64 on the kernel-level reference,
the data-parallel path over gloo, and the train.py flags.

The rounding bound.  The device forms e' = e - (e - p) * omd in fp32 with 0 <= omd <= 1 and M = max(|e|, |p|): the difference (at most
2 M) is rounded once, the product once, the final subtraction (a convex combination of e and p: at most M) once.  The first two errors
reach the result scaled by omd and 1: (2 omd + 2 omd + 1) * 2^-24 * M <= 5 * 2^-24 * M per update, with or without a fused
multiply-add (which only removes the product's rounding)."""
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
from sgg_amd.step import GanStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
BG, S, V = 4, 32, 11
DECAY, ITERS, CRITIC_ITERS = 0.999, 3, 2
U24 = 2.0 ** -24


def ema_bound(e, p):
    """5 * 2^-24 * max(|e|, |p|): the per-update bound of the module docstring (tests/test_ema_gpu.py uses the same)."""
    return 5.0 * U24 * np.maximum(np.abs(np.asarray(e, dtype=np.float64)), np.abs(np.asarray(p, dtype=np.float64)))


class EmaRefKernels(RefKernels):
    """The kernel-level reference with adam_ema and swap of csrc/optim.hip: its own adam followed by ema.reference_update, and an
    exchange through a copy."""

    def adam_ema(self, params, grads, m, v, avg, lr_t, b1, b2, eps, grad_scale=1.0, one_minus_decay=0.0):
        self.adam(params, grads, m, v, lr_t, b1, b2, eps, grad_scale)
        avg.copy_(torch.from_numpy(E.reference_update(avg.numpy(), params.numpy(), one_minus_decay)))

    def swap(self, a, b):
        t = a.clone()
        a.copy_(b)
        b.copy_(t)


# ---- schedule and restatement -------------------------------------------------------------------------------------------------
def test_tf_ema_decay_hand_values():
    assert E.tf_ema_decay(0.999, 0) == pytest.approx(0.1, abs=1e-15)
    assert E.tf_ema_decay(0.999, 90) == pytest.approx(0.91, abs=1e-15)
    assert E.tf_ema_decay(0.999, 10 ** 6) == 0.999
    assert E.tf_ema_decay(0.5, 8) == 0.5                    # (1 + 8) / (10 + 8) = 0.5: the two branches meet
    assert E.tf_ema_decay(0.05, 0) == 0.05
    assert E.one_minus_decay(0.999, 0) == pytest.approx(0.9, abs=1e-15)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            E.tf_ema_decay(bad, 3)


def test_reference_update_hand_case():
    e, p = np.array([1.0, -2.0, 0.5], dtype=np.float32), np.array([0.5, 2.0, 0.5], dtype=np.float32)
    got = E.reference_update(e, p, 0.25)
    assert got.dtype == np.float64 and got.tolist() == [0.875, -1.0, 0.5]
    assert E.reference_update(e, p, 0.0).tolist() == [1.0, -2.0, 0.5] and E.reference_update(e, p, 1.0).tolist() == [0.5, 2.0, 0.5]


def test_rounding_bound_from_the_reference_alone():
    r = np.random.RandomState(5)
    n, worst = 200000, 0.0
    for omd64 in (0.0, 1e-3, 0.05, 0.75, 0.9, 0.95, 1.0):
        omd = np.float32(omd64)
        for ratio in (1.0, 1e3, 1.0 + 1e-6):
            for flip in (1.0, -1.0):
                e = (np.where(r.rand(n) < 0.5, -1.0, 1.0) * r.uniform(1e-3, 4.0, n)).astype(np.float32)
                p = (e.astype(np.float64) * ratio * flip).astype(np.float32)
                assert (np.abs(e) >= 1.2e-38).all() and (np.abs(p) >= 1.2e-38).all(), "an input is subnormal"
                want, bound = E.reference_update(e, p, omd), ema_bound(e, p)
                d = (e - p).astype(np.float32)
                stepwise = (e - (d * omd).astype(np.float32)).astype(np.float32)                          # three fp32 roundings
                fma = (e.astype(np.float64) - d.astype(np.float64) * np.float64(omd)).astype(np.float32)   # product exact, one rounding
                for got in (stepwise, fma):
                    err = np.abs(got.astype(np.float64) - want)
                    assert (err <= bound).all(), (omd64, ratio, flip, float((err / bound).max()))
                    worst = max(worst, float((err / (bound / 5.0)).max()))
    print("worst error: %.2f units of 2^-24 * M" % worst)
    assert 0.4 < worst <= 5.0, "the inputs never came near the bound, or passed it"


# ---- host logic in fp64 ---------------------------------------------------------------------------------------------------------
def _states():
    gp, dp_ = O.init_params("G", V, S, dtype=DT, perturb=0.1), O.init_params("D", V, S, dtype=DT, perturb=0.1)
    dp_["W"] = dp_["W"] * 25.0
    return gp, dp_


def _iteration_inputs(it, shard=lambda t: t):
    noises = [shard(O.synth_noise(BG, 10 * it + i, DT)) for i in range(CRITIC_ITERS + 1)]
    alphas = [shard(O.synth_alpha(BG, 10 * it + i, DT).reshape(BG)) for i in range(CRITIC_ITERS)]
    return noises, alphas


def _run(decay, K=None, B=BG, shard=lambda t: t, reducer=None):
    """ITERS iterations of CRITIC_ITERS critic updates + one generator update; G averaged with `decay` (None: not at all)."""
    gp, dp_ = _states()
    images, labels, _ = O.synth_batch(BG, S, V, dtype=DT)
    gs = GanStep(K if K is not None else EmaRefKernels(), V, S, B, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer)
    if decay is not None:
        gs.G.enable_averaging(decay)
    snaps, losses = [gs.G.arena.flat.clone()], []
    for it in range(ITERS):
        noises, alphas = _iteration_inputs(it, shard)
        gs.train_iteration(shard(images), shard(labels), noises, alphas, critic_iters=CRITIC_ITERS)
        gs.flush()
        snaps.append(gs.G.arena.flat.clone())
        losses.append(torch.cat([gs.d_losses, gs.g_losses]).clone())
    return gs, snaps, losses


def _recurrence(snaps, decay):
    e = snaps[0].numpy().copy()
    for k, p in enumerate(snaps[1:]):
        e = e - (e - p.numpy()) * (1.0 - min(decay, (1.0 + k) / (10.0 + k)))
    return e


_RUNS = {}


def runs():
    if not _RUNS:
        _RUNS["ema"] = _run(DECAY)
        _RUNS["plain"] = _run(None, K=RefKernels())
    return _RUNS


def test_average_follows_the_recurrence_and_training_is_unchanged():
    (gs, snaps, losses), (ps, psnaps, plosses) = runs()["ema"], runs()["plain"]
    avg = gs.G.opt["ema"]
    assert gs.G.has_average and avg["updates"] == ITERS == gs.G.adam_t and avg["decay"] == DECAY and not avg["swapped"]
    assert "ema" not in gs.D.opt and not gs.D.has_average and gs.D.adam_t == ITERS * CRITIC_ITERS
    want = _recurrence(snaps, DECAY)
    assert float(np.abs(avg["flat"].numpy() - want).max()) <= 1e-15
    assert float(np.abs(want - snaps[-1].numpy()).max()) > 1e-6, "the average equals the last iterate: nothing was averaged"
    # a second call changes the decay only; the constant branch of the schedule from then on
    gs.G.enable_averaging(0.05)
    assert avg is gs.G.opt["ema"] and avg["decay"] == 0.05 and avg["updates"] == ITERS
    gs.G.enable_averaging(DECAY)
    with pytest.raises(ValueError):
        gs.G.enable_averaging(1.0)
    # training itself: bit-equal to the run that never averaged
    assert "ema" not in ps.G.opt and "ema" not in ps.D.opt
    for a, b in ((gs.G, ps.G), (gs.D, ps.D)):
        assert torch.equal(a.arena.flat, b.arena.flat) and torch.equal(a.m_flat, b.m_flat) and torch.equal(a.v_flat, b.v_flat)
    assert all(torch.equal(x, y) for x, y in zip(losses, plosses)) and all(torch.equal(x, y) for x, y in zip(snaps, psnaps))


def test_a_kernel_set_without_the_entry_points_is_refused():
    gs = runs()["plain"][0]
    with pytest.raises(RuntimeError, match="adam_ema"):
        gs.G.enable_averaging(0.9)
    for call in (gs.G.reset_average, gs.G.average_state, lambda: gs.G.state_dict(averaged=True)):
        with pytest.raises(RuntimeError, match="enable_averaging"):
            call()
    with pytest.raises(RuntimeError, match="enable_averaging"):
        with gs.G.averaged():
            pass


def test_averaged_swaps_restores_and_forbids():
    gs = runs()["ema"][0]
    G, avg = gs.G, gs.G.opt["ema"]
    live0, ema0, version0 = G.arena.flat.clone(), avg["flat"].clone(), G.arena.version
    n = G.arena.live_numel
    bits = lambda t: t.view(torch.int64)
    images, _, _ = O.synth_batch(BG, S, V, dtype=DT)
    noise = O.synth_noise(BG, 77, DT)
    before = gs.generator_forward(images, noise, for_backward=False)[0].OUT[0].clone()
    sd_avg = G.state_dict(averaged=True)
    with G.averaged() as inside:
        assert inside is G and avg["swapped"] and G.arena.version == version0 + 1
        assert torch.equal(bits(G.arena.flat[:n]), bits(ema0[:n])) and torch.equal(bits(avg["flat"][:n]), bits(live0[:n]))
        assert torch.equal(bits(G.arena.flat[n:]), bits(live0[n:])), "the dead tail is not exchanged"
        for name, call in (("adam_step", G.adam_step), ("load_state_dict", lambda: G.load_state_dict(sd_avg)),
                           ("reset_average", G.reset_average), ("state_dict", G.state_dict), ("nested", lambda: G.averaged().__enter__()),
                           ("average_state", G.average_state)):
            with pytest.raises(RuntimeError, match="averaged\\(\\)"):
                call()
        got = gs.generator_forward(images, noise, for_backward=False)[0].OUT[0].clone()
    assert not avg["swapped"] and G.arena.version == version0 + 2
    assert torch.equal(bits(G.arena.flat), bits(live0)) and torch.equal(bits(avg["flat"]), bits(ema0))
    # the forward inside is the forward of a fresh step loaded from the averaged state dict
    gp, dp_ = _states()
    fresh = GanStep(RefKernels(), V, S, BG, g_state=sd_avg, d_state=dp_, dtype=DT)
    want = fresh.generator_forward(images, noise, for_backward=False)[0].OUT[0]
    assert torch.equal(got, want) and not torch.equal(got, before)
    assert torch.equal(gs.generator_forward(images, noise, for_backward=False)[0].OUT[0], before)
    # ... also when the body raises
    with pytest.raises(KeyError):
        with G.averaged():
            raise KeyError("body")
    assert not avg["swapped"] and torch.equal(bits(G.arena.flat), bits(live0)) and torch.equal(bits(avg["flat"]), bits(ema0))
    # reset_average: the arena again, count 0 (on a copy of the state: the shared run stays as it is)
    keep = (avg["flat"].clone(), avg["updates"])
    G.reset_average()
    assert avg["updates"] == 0 and torch.equal(bits(avg["flat"]), bits(G.arena.flat))
    G.restore_average(*keep)
    assert avg["updates"] == ITERS and torch.equal(bits(avg["flat"]), bits(ema0))
    st = G.average_state()
    assert st["updates"] == ITERS and st["decay"] == DECAY and torch.equal(st["flat"], ema0)


# ---- data parallel over gloo ----------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sgg_amd  # noqa: F401
    from sgg_amd import dp
    torch.set_num_threads(2)
    dp.init_from_env(backend="gloo")
    gs, _, _ = _run(DECAY, B=BG // world, shard=lambda t: dp.shard_rows(t, rank, world), reducer=dp.GradReducer())
    torch.save({"ema": gs.G.opt["ema"]["flat"], "updates": gs.G.opt["ema"]["updates"], "G": gs.G.arena.flat}, out % rank)
    torch.distributed.destroy_process_group()


def test_two_rank_average_equals_single_process(tmp_path):
    out = str(tmp_path / "rank%d.pt")
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert r0["updates"] == r1["updates"] == ITERS
    assert torch.equal(r0["ema"].view(torch.int64), r1["ema"].view(torch.int64)) and torch.equal(r0["G"], r1["G"]), "replicas diverged"
    single = runs()["ema"][0]
    err = float((r0["ema"] - single.G.opt["ema"]["flat"]).abs().max())
    assert err < 1e-8, "average: data-parallel vs single process differ by %.3e" % err


# ---- train.py -------------------------------------------------------------------------------------------------------------------
def test_parser_knows_the_flags():
    sys.path.insert(0, ROOT)
    import train as T
    args = T.build_parser().parse_args([])
    assert args.ema_decay == 0 and args.eval_live is False
    args = T.build_parser().parse_args(["--ema_decay", "0.999", "--eval_live"])
    assert args.ema_decay == 0.999 and args.eval_live is True
