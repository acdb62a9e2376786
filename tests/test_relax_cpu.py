"""CPU: the relaxed generator output (csrc/relax.hip, GanStep.set_relaxation, train.py's --generator_output / --relax_tau) in fp64 on the
kernel-level reference: Philox and the restatement's known answers (tests/relax_ref.py), the Gumbel-max property of its noise, the
host logic of the step against autograd on the oracle composed with the relaxation, accumulation, the data-parallel path over gloo,
the guard and the weight average, G-encoder reuse, the default mode, and train.py on the reference kernels.

Bounds: those of tests/test_step_cpu.py, for the same reason - both sides are fp64 and differ by summation order only: 1e-8 on
gradients (relative to the tensor's largest element), 1e-9 on parameters after Adam, 1e-8 for accumulated against whole batch and two
ranks against one process."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd.step import GanStep
from tests import relax_ref as RR
from tests.test_step_cpu import rel_err
from tests.test_xent_cpu import XentRefKernels, cpu_train  # noqa: F401  (cpu_train: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
V, B = 11, 2
NEW = ("relax_rows", "relax_rows_bwd")
SEED = 0x1234ABCD5678EF01


class RelaxRefKernels(XentRefKernels):
    """The kernel-level reference carrying torch fp64 versions of the two entry points of csrc/relax.hip (the noise through the
    restatement's Philox); every call of them is recorded, with its arguments in `relax_log`."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.relax_log = []

    def relax_rows(self, x, tau, y=None, gumbel=False, seed=0, draw=0, u_out=None):
        self.calls.append("relax_rows")
        self.relax_log.append({"tau": float(tau), "gumbel": bool(gumbel), "seed": int(seed), "draw": int(draw), "in_place": y is None})
        assert float(tau) > 0.0
        if y is None:
            y = x
        Vx = x.shape[-1]
        z = x.reshape(-1, Vx)
        if gumbel:
            u = torch.from_numpy(RR.uniforms(seed, draw, z.shape[0], Vx)).to(z.dtype)
            if u_out is not None:
                u_out.copy_(u.reshape(u_out.shape))
            z = z - torch.log(-torch.log(u))
        y.copy_(torch.softmax(z / float(tau), dim=-1).reshape(y.shape))
        return y

    def relax_rows_bwd(self, y, dy, tau, scale=1.0, dx=None):
        self.calls.append("relax_rows_bwd")
        if dx is None:
            dx = dy
        dx.copy_((float(scale) / float(tau)) * y * (dy - (y * dy).sum(dim=-1, keepdim=True)))
        return dx

    def rank_triples(self, tokens, d, K, descending=False, want_sample_scores=False, vocab=None, out=None):
        """The documented order of csrc/rank.hip, restated for predict() / evaluate() on this kernel set: samples by the mean of
        their three critic outputs (ties by sample index), the distinct triples in that order."""
        N, nb = int(tokens.shape[0]), int(tokens.shape[1])
        sc = d.reshape(N, nb, 3).to(torch.float32).mean(dim=2).numpy()
        tok = tokens.numpy()
        res = {"triples": np.full((nb, K, 3), -1, np.int64), "scores": np.full((nb, K), np.nan, np.float32),
               "first_rank": np.full((nb, K), -1, np.int32), "first_sample": np.full((nb, K), -1, np.int32),
               "counts": np.zeros((nb, K), np.int32), "n_distinct": np.zeros((nb,), np.int32)}
        for j in range(nb):
            order = np.argsort(-sc[:, j] if descending else sc[:, j], kind="stable")
            seen = {}
            for rank, k in enumerate(order):
                t = tuple(tok[k, j])
                if t not in seen:
                    seen[t] = len(seen)
                    if seen[t] < K:
                        u = seen[t]
                        res["triples"][j, u], res["scores"][j, u] = t, sc[k, j]
                        res["first_rank"][j, u], res["first_sample"][j, u] = rank, k
                if seen[t] < K:
                    res["counts"][j, seen[t]] += 1
            res["n_distinct"][j] = len(seen)
        ret = {}
        for name, arr in res.items():
            t = torch.from_numpy(arr)
            if out is not None:
                out[name].copy_(t)
                t = out[name]
            ret[name] = t
        return ret


# ---- Philox, u, the restatement ------------------------------------------------------------------------------------------------------
def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers_and_u():
    assert _hex(RR.philox4x32((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(RR.philox4x32((ones,) * 4, (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(RR.philox4x32((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # u: 23 bits, strictly inside (0, 1), exact in fp32
    lo, hi = float(RR.u_of_word(0)), float(RR.u_of_word(2 ** 32 - 1))
    assert lo == 2.0 ** -24 and hi == 1.0 - 2.0 ** -24
    assert float(np.float32(lo)) == lo and float(np.float32(hi)) == hi and 0.0 < lo < hi < 1.0
    g = RR.gumbel(np.array([lo, hi]))
    assert -2.82 < g[0] < -2.81 and 16.63 < g[1] < 16.64
    # the counter layout: element j of row r is word j & 3 of the block (j >> 2, r, draw lo, draw hi) under the key (seed lo, seed hi)
    seed, draw = 0x299F31D0A4093822, 0x0370734413198A2E
    u = RR.uniforms(seed, draw, 1, 8, row0=0x85A308D3)
    blk = RR.philox4x32((1, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert np.array_equal(u[0, 4:], RR.u_of_word(np.array([int(w) for w in blk])))
    assert not np.array_equal(RR.uniforms(seed, draw, 2, 8)[0], RR.uniforms(seed, draw + 1, 2, 8)[0])


def test_forward_and_backward_known_answers():
    x = np.array([[0.0, 0.0, 0.0], np.log([1.0, 2.0, 3.0])])
    y, u = RR.relax_rows(x, 1.0)
    assert u is None and np.allclose(y, [[1 / 3, 1 / 3, 1 / 3], [1 / 6, 2 / 6, 3 / 6]], rtol=0, atol=1e-15)
    y2, _ = RR.relax_rows(x, 0.5)                           # z = 2 log k: y ~ k^2
    assert np.allclose(y2, [[1 / 3, 1 / 3, 1 / 3], [1 / 14, 4 / 14, 9 / 14]], rtol=0, atol=1e-15)
    dy = np.array([[1.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    dx = RR.relax_rows_bwd(y, dy, 1.0)
    assert np.allclose(dx, [[2 / 9, -1 / 9, -1 / 9], [-2 / 9, -1 / 9, 1 / 3]], rtol=0, atol=1e-15)
    assert np.allclose(RR.relax_rows_bwd(y, dy, 0.5, scale=3.0), 6.0 * dx, rtol=0, atol=1e-14)
    assert np.abs(dx.sum(axis=1)).max() < 1e-15, "a gradient row sums to zero"
    # a row of +-80 at tau 0.1 does not overflow
    big, _ = RR.relax_rows(np.array([[80.0, -80.0, 80.0]]), 0.1)
    assert np.isfinite(big).all() and np.allclose(big, [[0.5, 0.0, 0.5]], rtol=0, atol=1e-15)


@pytest.mark.parametrize("gumbel", [False, True])
@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_backward_is_the_gradient_of_the_forward(gumbel, tau):
    g = np.random.RandomState(5)
    x, dy = 2.0 * g.standard_normal((4, 7)), g.standard_normal((4, 7))
    f = lambda xx: 1.7 * (dy * RR.relax_rows(xx, tau, gumbel, SEED, 3)[0]).sum()
    y, _ = RR.relax_rows(x, tau, gumbel, SEED, 3)
    dx = RR.relax_rows_bwd(y, dy, tau, scale=1.7)
    h, num = 1e-6, np.zeros_like(x)
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            e = np.zeros_like(x)
            e[i, j] = h
            num[i, j] = (f(x + e) - f(x - e)) / (2 * h)
    err = float(np.abs(num - dx).max())
    print("central difference vs backward (gumbel %s, tau %g): %.3e" % (gumbel, tau, err))
    assert err < 1e-8        # (h^2 f''' / 6 ~ 1e-12 truncation + 1e-16 / h ~ 1e-10 rounding)


def test_gumbel_max_property_of_the_restatement():
    """argmax(x + g) is a draw from softmax(x): 20 000 rows of one 5-way distribution at distinct (row, draw)."""
    p = np.array([0.4, 0.25, 0.2, 0.1, 0.05])
    n_draws, rows = 4, 5000
    counts = np.zeros(5)
    for draw in range(n_draws):
        u = RR.uniforms(SEED, draw, rows, 5)
        counts += np.bincount((np.log(p)[None, :] + RR.gumbel(u)).argmax(axis=1), minlength=5)
    n = n_draws * rows
    freq, se = counts / n, np.sqrt(p * (1 - p) / n)
    print("Gumbel-max frequencies %s (softmax %s), in standard errors %s" % (freq, p, (freq - p) / se))
    assert (np.abs(freq - p) <= 4.0 * se).all()


def test_torch_entry_points_follow_the_restatement():
    K = RelaxRefKernels()
    g = np.random.RandomState(3)
    x, dy = 3.0 * g.standard_normal((6, 7)), g.standard_normal((6, 7))
    for gumbel in (False, True):
        y, u = torch.zeros(6, 7, dtype=DT), torch.zeros(6, 7, dtype=DT)
        K.relax_rows(torch.from_numpy(x), 0.5, y=y, gumbel=gumbel, seed=SEED, draw=9, u_out=u if gumbel else None)
        ref, uref = RR.relax_rows(x, 0.5, gumbel, SEED, 9)
        assert np.abs(y.numpy() - ref).max() < 1e-14 and (not gumbel or np.array_equal(u.numpy(), uref))
        xi = torch.from_numpy(x.copy())
        assert K.relax_rows(xi, 0.5, gumbel=gumbel, seed=SEED, draw=9) is xi and torch.equal(xi, y), "in place"
        d = torch.from_numpy(dy.copy())
        K.relax_rows_bwd(y, d, 0.5, scale=2.0)
        assert np.abs(d.numpy() - RR.relax_rows_bwd(ref, dy, 0.5, 2.0)).max() < 1e-14
    assert K.calls == ["relax_rows", "relax_rows", "relax_rows_bwd"] * 2


# ---- host logic in fp64: autograd on the oracle composed with the relaxation ----------------------------------------------------------
def _states(S):
    gp, dp_ = O.init_params("G", V, S, dtype=DT, perturb=0.1), O.init_params("D", V, S, dtype=DT, perturb=0.1)
    dp_["W"] = dp_["W"] * 25.0
    return gp, dp_


def _fresh(S=32, rows=B, reducer=None, K=None, relax=None):
    gp, dp_ = _states(S)
    gs = GanStep(K if K is not None else RelaxRefKernels(), V, S, rows, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer)
    if relax is not None:
        gs.set_relaxation(*relax)
    return gs, gp, dp_


def oracle_relax(fake, mode, tau, seed=0, draw=0):
    """The relaxation on the oracle's logits [B, 3, V] (row b * 3 + t of the launch), differentiable."""
    if mode == "logits":
        return fake
    z = fake
    if mode == "gumbel":
        u = RR.uniforms(seed, draw, fake.shape[0] * fake.shape[1], fake.shape[2]).reshape(tuple(fake.shape))
        z = z - torch.log(-torch.log(torch.from_numpy(u).to(fake.dtype)))
    return torch.softmax(z / tau, dim=-1)


def oracle_g_cost(gp, dp_, images, noise, mode, tau, seed=0, draw=0, labels=None, w=0.0):
    """generator_forward -> relaxation -> discriminator_forward [+ w * cross-entropy of the LOGITS]; returns (cost, grads of gp)."""
    gp = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    fake = O.generator_forward(gp, images, noise)
    cost = -O.discriminator_forward(dp_, oracle_relax(fake, mode, tau, seed, draw), images).mean()
    if w > 0.0:
        cost = cost + w * (-torch.log_softmax(fake, dim=-1).gather(-1, labels.unsqueeze(-1)).sum() / images.shape[0])
    return cost.detach(), O._grads(cost, gp)


def oracle_d_cost(gp, dp_, images, onehot, noise, alpha, lam, mode, tau, seed=0, draw=0):
    """d_loss's body with the relaxed fake (a constant for D); returns (cost, aux, grads of dp)."""
    dp_ = {k: v.clone().requires_grad_(True) for k, v in dp_.items()}
    with torch.no_grad():
        fake = oracle_relax(O.generator_forward(gp, images, noise), mode, tau, seed, draw)
    feat_d = O.encoder(dp_, images)
    d_fake, d_real = O.discriminator_head(dp_, feat_d, fake), O.discriminator_head(dp_, feat_d, onehot)
    gpen, slopes, _ = O.gradient_penalty(dp_, feat_d, onehot, fake, alpha)
    cost = d_fake.mean() - d_real.mean() + lam * gpen
    return cost.detach(), {"gp": gpen.detach(), "d_fake": d_fake.detach()}, O._grads(cost, dp_)


MODES = [("softmax", 1.0), ("softmax", 0.5), ("gumbel", 1.0), ("gumbel", 0.5)]


@pytest.mark.parametrize("mode,tau", MODES)
def test_generator_step_matches_autograd_through_the_relaxation(mode, tau):
    S = 32
    images, labels, _ = O.synth_batch(B, S, V, dtype=DT)
    noise = O.synth_noise(B, 1, DT)
    for w in (0.0, 0.3):
        gs, gp, dp_ = _fresh(S, relax=(mode, tau, SEED))
        kw = {"labels": labels, "mle_weight": w} if w > 0.0 else {}
        cost, grads = oracle_g_cost(gp, dp_, images, noise, mode, tau, SEED, 41, labels, w)
        gl = gs.generator_step(images, noise, draw=41, **kw)
        assert [c for c in gs.K.calls if c in NEW] == ["relax_rows", "relax_rows_bwd"]
        assert gs.K.relax_log[0] == {"tau": tau, "gumbel": mode == "gumbel", "seed": SEED, "draw": 41 if mode == "gumbel" else 0,
                                     "in_place": False}
        for name, g in grads.items():
            e = rel_err(gs.G.grads[name], g)
            assert e < 1e-8, "generator grad %s rel err %.3e (%s, tau %g, w %g)" % (name, e, mode, tau, w)
        m, v = O.new_adam_state(gp)
        O.tf_adam_step(gp, grads, m, v, 1)
        for name in gp:
            if not O.is_dead(name):
                assert rel_err(gs.G.arena.views[name], gp[name]) < 1e-9, "generator param after Adam: " + name
        if w == 0.0:
            assert abs(-float(gl[3]) - float(cost)) < 1e-9
    # the relaxation is in the gradient: the plain step is far outside the bound
    plain, _, _ = _fresh(S)
    plain.generator_step(images, noise)
    _, g0 = oracle_g_cost(*_states(S), images, noise, mode, tau, SEED, 41)
    assert rel_err(plain.G.grads["decoder/bias"], g0["decoder/bias"]) > 1e-3


@pytest.mark.parametrize("mode,tau", MODES)
def test_critic_step_and_critic_loss_match_autograd_on_the_relaxed_fake(mode, tau):
    S = 32
    gs, gp, dp_ = _fresh(S, relax=(mode, tau, SEED))
    images, labels, onehot = O.synth_batch(B, S, V, dtype=DT)
    noise, alpha = O.synth_noise(B, 0, DT), O.synth_alpha(B, 0, DT)
    cost, aux, grads = oracle_d_cost(gp, dp_, images, onehot, noise, alpha, 10.0, mode, tau, SEED, 7)
    val = gs.critic_loss(images, labels, noise, alpha.reshape(B), draw=7).clone()
    # in gumbel mode the draw matters, in softmax mode it is ignored
    other = gs.critic_loss(images, labels, noise, alpha.reshape(B), draw=8).clone()
    assert (float((other - val).abs().max()) > 1e-6) == (mode == "gumbel")
    dl = gs.critic_step(images, labels, noise, alpha.reshape(B), draw=7).clone()
    assert [c for c in gs.K.calls if c in NEW] == ["relax_rows"] * 3, "the critic's update treats y as a constant: no backward launch"
    assert abs(float(dl[0]) - float(cost)) < 1e-9 * max(1.0, abs(float(cost))) and abs(float(dl[2]) - float(aux["gp"])) < 1e-9
    assert abs(float(dl[3]) - float(aux["d_fake"].mean())) < 1e-9 and torch.allclose(val, dl, rtol=0, atol=1e-12)
    for name, g in grads.items():
        if g is None:
            continue
        e = rel_err(gs.D.grads[name], g)
        assert e < 1e-8, "critic grad %s rel err %.3e (%s, tau %g)" % (name, e, mode, tau)
    m, v = O.new_adam_state(dp_)
    O.tf_adam_step(dp_, grads, m, v, 1)
    for name in dp_:
        if not O.is_dead(name):
            assert rel_err(gs.D.arena.views[name], dp_[name]) < 1e-9, "critic param after Adam: " + name
    # the fake rows D saw lie on the simplex
    fake_rows = gs.TRI[:B]
    assert float((fake_rows.sum(dim=-1) - 1.0).abs().max()) < 1e-12 and float(fake_rows.min()) >= 0.0


def test_the_relaxation_moves_the_oracles_gradient():
    """The setting of the GPU step tests (tests/test_relax_gpu.py: B 8, S 64, V 50, W x 25, tau 0.5), on the oracle alone in fp32: the
    plain generator cost's decoder/bias gradient is more than 100 x GRAD_RTOL away from the relaxed one's, in both modes - a step that
    forgot the relaxation cannot pass there."""
    from tests.tolerances import GRAD_RTOL
    Bg, Sg, Vg = 8, 64, 50
    gp, dp_ = O.init_params("G", Vg, Sg, perturb=0.05), O.init_params("D", Vg, Sg, perturb=0.05)
    dp_["W"] = dp_["W"] * 25.0
    images, _, _ = O.synth_batch(Bg, Sg, Vg)
    noise = O.synth_noise(Bg, 1)
    _, plain = oracle_g_cost(gp, dp_, images, noise, "logits", 1.0)
    for mode in ("softmax", "gumbel"):
        _, relaxed = oracle_g_cost(gp, dp_, images, noise, mode, 0.5, SEED, 41)
        a, b = plain["decoder/bias"], relaxed["decoder/bias"]
        gap = float((a - b).abs().max() / (b.abs().max() + 1e-7))
        print("decoder/bias, plain against %s: %.3e of the relaxed gradient's maximum" % (mode, gap))
        assert gap > 100 * GRAD_RTOL


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def _pick(t, idx):
    return t[idx].contiguous()


def _iterations(rows, Bm, pick, mode, reducer=None, guard=None, decay=None, reuse=False, draws=None, seed=SEED):
    """Two GAN iterations (two critic updates each) over `rows` rows, each update from len(pick) micro-batches of Bm rows.
    draws[k]: the draw offset of micro-batch k (gumbel)."""
    S, N, C = 32, len(pick), 2
    images, labels, _ = O.synth_batch(rows, S, V, dtype=DT)
    gs, _, _ = _fresh(S, Bm, reducer=reducer, relax=(mode, 0.5, seed))
    if guard is not None:
        gs.set_guard((guard, guard), False)
    if decay is not None:
        gs.G.enable_averaging(decay)
    draws = draws if draws is not None else list(range(N))
    for it in range(2):
        noises = [[_pick(O.synth_noise(rows, 10 * it + i, DT), p) for p in pick] for i in range(C + 1)]
        alphas = [[_pick(O.synth_alpha(rows, 10 * it + i, DT).reshape(rows), p) for p in pick] for i in range(C)]
        dr = [[1000 * it + 100 * i + draws[k] for k in range(N)] for i in range(C + 1)]
        gs.train_iteration_accumulated([(_pick(images, p), _pick(labels, p)) for p in pick], noises, alphas, critic_iters=C,
                                       reuse_g_encoder=reuse, draws=dr)
    gs.flush()
    return gs, {"G": gs.G.arena.flat.clone(), "D": gs.D.arena.flat.clone(), "Gm": gs.G.m_flat.clone(), "Dm": gs.D.m_flat.clone()}


def test_accumulated_equals_the_large_batch():
    """softmax mode (the Gumbel noise of a row depends on its place in the launch, so a split batch draws other noise)."""
    _, want = _iterations(4, 4, [[0, 1, 2, 3]], "softmax")
    gs, got = _iterations(4, 2, [[0, 1], [2, 3]], "softmax")
    for key in want:
        err = float((got[key] - want[key]).abs().max())
        print("%s: N = 2 x B = 2 vs B = 4 differ by %.3e" % (key, err))
        assert err < 1e-8, (key, err)
    assert gs.G.adam_t == 2 and gs.D.adam_t == 4
    other = _iterations(4, 2, [[0, 1], [0, 1]], "softmax")[1]
    assert float((other["G"] - want["G"]).abs().max()) > 1e3 * 1e-8


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sgg_amd  # noqa: F401
    from sgg_amd import dp
    torch.set_num_threads(2)
    dp.init_from_env(backend="gloo")
    # rank r draws what micro-batch r of the single process draws: the same seed, the draw offset r
    _, res = _iterations(4, 2, [[2 * rank, 2 * rank + 1]], "gumbel", reducer=dp.GradReducer(), draws=[rank])
    torch.save(res, out % rank)
    torch.distributed.destroy_process_group()


def test_two_ranks_equal_the_single_process_in_gumbel_mode(tmp_path):
    out = str(tmp_path / "rank%d.pt")
    port = 39500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(r0["G"], r1["G"]) and torch.equal(r0["D"], r1["D"]), "replicas diverged"
    _, want = _iterations(4, 2, [[0, 1], [2, 3]], "gumbel", draws=[0, 1])
    for key in want:
        err = float((r0[key] - want[key]).abs().max())
        print("%s: world 2 x B 2 vs 2 micro-batches differ by %.3e" % (key, err))
        assert err < 1e-8, (key, err)
    # (other draws are far outside the bound: the comparison can fail)
    _, moved = _iterations(4, 2, [[0, 1], [2, 3]], "gumbel", draws=[5, 6])
    assert float((moved["G"] - want["G"]).abs().max()) > 1e3 * 1e-8


def test_guard_and_average_apply_to_the_relaxed_updates():
    twin, _, _ = _fresh(relax=("gumbel", 0.5, SEED))
    images, labels, _ = O.synth_batch(2, 32, V, dtype=DT)
    twin.generator_step(images, O.synth_noise(2, 0, DT), draw=3)
    norm = float(twin.G.arena.live(twin.G.grad_flat).pow(2).sum().sqrt())
    assert norm > 0
    first, _, _ = _fresh(relax=("gumbel", 0.5, SEED))
    first.set_guard((0.0, norm / 4.0), False)
    first.G.enable_averaging(0.9)
    init = first.G.arena.flat.clone()
    first.generator_step(images, O.synth_noise(2, 0, DT), draw=3)
    r = first.G.guard_report()
    assert r["clipped"] == 1 and abs(r["coef"] - 0.25) < 1e-12 and abs(r["norm"] - norm) < 1e-12 * norm
    assert float((first.G.m_flat - 0.25 * twin.G.m_flat).abs().max()) <= 1e-12 * float(twin.G.m_flat.abs().max())
    avg = first.G.opt["ema"]
    assert avg["updates"] == 1 and not torch.equal(avg["flat"], init) and not torch.equal(avg["flat"], first.G.arena.flat)


@pytest.mark.parametrize("mode", ["softmax", "gumbel"])
def test_with_reuse_equals_without_reuse(mode):
    a = _iterations(2, 2, [[0, 1]], mode, reuse=False)[1]
    b = _iterations(2, 2, [[0, 1]], mode, reuse=True)[1]
    for key in a:
        assert torch.equal(a[key].view(torch.int64), b[key].view(torch.int64)), key


# ---- the default mode -----------------------------------------------------------------------------------------------------------------
def _one_iteration(gs, **kw):
    images, labels, _ = O.synth_batch(B, 32, V, dtype=DT)
    gs.train_iteration(images, labels, [O.synth_noise(B, i, DT) for i in range(3)], [O.synth_alpha(B, i, DT).reshape(B) for i in range(2)],
                       critic_iters=2, **kw)
    gs.flush()
    return [t.clone() for net in (gs.G, gs.D) for t in (net.arena.flat, net.grad_flat, net.m_flat, net.v_flat)]


def test_default_mode_launches_nothing_new_and_keeps_every_bit():
    never, _, _ = _fresh(K=XentRefKernels())             # a kernel set that has never heard of the option
    want = _one_iteration(never)
    for setup in (lambda gs: None, lambda gs: gs.set_relaxation("logits"),
                  lambda gs: (gs.set_relaxation("gumbel", 0.5, 1), gs.set_relaxation("logits"))):
        gs, _, _ = _fresh()
        setup(gs)
        got = _one_iteration(gs, draws=[1, 2, 3])
        assert not [c for c in gs.K.calls if c in NEW]
        for a, b in zip(want, got):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert _fresh()[0]._relax_buf is None and _fresh()[0].relaxation is None, "no buffer unless a mode is on"
    on, _, _ = _fresh(relax=("softmax", 2.0, 0))
    assert tuple(on._relax_buf.shape) == (B, 3, V) and on.relaxation == {"mode": "softmax", "tau": 2.0, "seed": 0}
    moved = _one_iteration(on)
    assert not torch.equal(moved[0], want[0]) and not torch.equal(moved[4], want[4])


def test_a_kernel_set_without_the_entry_points_is_refused_by_name():
    bare, _, _ = _fresh(K=XentRefKernels())
    bare.set_relaxation("logits")                         # the default needs nothing
    for mode in ("softmax", "gumbel"):
        with pytest.raises(RuntimeError, match="relax_rows"):
            bare.set_relaxation(mode, 1.0)
    assert bare.relaxation is None and bare.G.adam_t == 0
    gs, _, _ = _fresh()
    with pytest.raises(ValueError, match="generator_output"):
        gs.set_relaxation("hard")
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            gs.set_relaxation("softmax", tau)


# ---- train.py on the reference kernels --------------------------------------------------------------------------------------------------
@pytest.fixture
def relax_train(cpu_train, monkeypatch):
    """cpu_train with a RelaxRefKernels behind kernels_for."""
    T, _, make = cpu_train
    from sgg_amd import api
    K = RelaxRefKernels()
    monkeypatch.setattr(T, "kernels_for", lambda device: K)
    monkeypatch.setattr(api, "kernels_for", lambda device: K)
    return T, K, make


def _records(tmp, name):
    with open(str(tmp / name / "logs" / "losses.jsonl")) as f:
        return [json.loads(l) for l in f if l.strip()]


def test_parser_knows_the_flags_and_the_schedule():
    sys.path.insert(0, ROOT)
    import train as T
    a = T.build_parser().parse_args([])
    assert a.generator_output is None and a.relax_tau is None and a.seed == 0
    a = T.parse_args(["--generator_output", "gumbel", "--relax_tau", "2,0.5,100", "--seed", "5"])
    assert (a.generator_output, a.relax_tau, a.seed) == ("gumbel", (2.0, 0.5, 100), 5)
    assert T.parse_args(["--relax_tau", "0.7"]).relax_tau == (0.7, 0.7, 0)
    for bad in (["--generator_output", "hard"], ["--relax_tau", "0"], ["--relax_tau", "1,2"], ["--relax_tau", "1,-2,10"],
                ["--relax_tau", "nan"], ["--relax_tau", "1,2,0"], ["--relax_tau", "1,2,1.5"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    spec = (2.0, 0.5, 100)
    for it, want in ((0, 2.0), (50, 1.0), (100, 0.5), (200, 0.5)):
        assert abs(T.relax_tau_at(spec, it) - want) < 1e-15, (it, T.relax_tau_at(spec, it))
    assert T.relax_tau_at((0.7, 0.7, 0), 12345) == 0.7
    # the draw numbers of an iteration's launches are distinct, and distinct from every validation's
    draws = {T.relax_draw(it, i, k, 2, 3) for it in range(4) for i in range(3) for k in range(3)}
    assert len(draws) == 36 and all(d < 2 ** 63 for d in draws) and T.relax_val_draw(0) >= 2 ** 63


def test_train_gumbel_run_resumes_bit_for_bit_and_records_the_mode(relax_train, tmp_path):
    T, K, make = relax_train
    kw = dict(generator_output="gumbel", relax_tau="2,0.5,2", critic_iters=2)
    gan = make(tmp_path, "whole", resume=False, **kw)
    gan.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    recs = [r for r in _records(tmp_path, "whole") if "triples_per_s" in r]
    assert [r["relax"] for r in recs] == [{"mode": "gumbel", "tau": 2.0}, {"mode": "gumbel", "tau": 1.0}, {"mode": "gumbel", "tau": 0.5}]
    ck = torch.load(gan._ckpt_path())
    assert ck["generator_output"] == {"mode": "gumbel", "tau": [2.0, 0.5, 2]}
    # every launch of training has a draw of its own; validation uses the training relaxation with draws keyed on its counter
    train_draws = [c["draw"] for c in K.relax_log if c["draw"] < 2 ** 63]
    val_draws = [c["draw"] for c in K.relax_log if c["draw"] >= 2 ** 63]
    assert len(train_draws) == 9 and len(set(train_draws)) == 9 and val_draws == [T.relax_val_draw(k) for k in range(3)]
    assert all(c["gumbel"] and c["seed"] == gan._relax_seed() for c in K.relax_log)
    assert [c["tau"] for c in K.relax_log if c["draw"] >= 2 ** 63] == [2.0, 1.0, 0.5]
    # stopped after one iteration and resumed WITHOUT the flags: the mode comes from the checkpoint, the same weights bit for bit
    part = make(tmp_path, "parts", resume=False, **kw)
    part.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    rest = make(tmp_path, "parts", resume=True, critic_iters=2)
    rest.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    ck2 = torch.load(rest._ckpt_path())
    assert ck2["generator_output"] == ck["generator_output"]
    for net in ("G", "D"):
        for name, t in ck[net].items():
            assert torch.equal(t, ck2[net][name]), "%s %s differs after the resume" % (net, name)
    # a contradicting flag is an error, on resume and at evaluation
    for bad in (dict(generator_output="softmax"), dict(generator_output="logits"), dict(relax_tau="1.0")):
        with pytest.raises(ValueError, match="contradicts"):
            make(tmp_path, "parts", resume=True, critic_iters=2, **bad).train(max_iterations=4, test_at_end=False)
        with pytest.raises(ValueError, match="contradicts"):
            make(tmp_path, "parts", resume=True, critic_iters=2, **bad).load_checkpoint()
    plain = make(tmp_path, "plain", resume=False)
    plain.train(max_iterations=1, log_every=1, validate_every=0, test_at_end=False)
    with pytest.raises(ValueError, match="contradicts"):
        make(tmp_path, "plain", resume=True, generator_output="softmax").load_checkpoint()


def test_train_defaults_write_the_parents_checkpoint_and_call_nothing_new(relax_train, tmp_path):
    T, K, make = relax_train
    gan = make(tmp_path, "plain", resume=False)
    gan.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    assert set(torch.load(gan._ckpt_path())) == {"itr", "G", "D", "G_adam", "D_adam", "val"}
    recs = _records(tmp_path, "plain")
    assert set(recs[0]) == {"itr", "disc_loss", "gen_loss", "gp", "triples_per_s"} and set(recs[1]) == {"itr", "val_disc_loss"}
    gan.test(max_images=1, out_path=str(tmp_path / "recalls.txt"))
    assert "generator_output" not in open(str(tmp_path / "recalls.txt")).read()
    assert "generator_output" not in gan.predict(max_images=1)[0] and not [c for c in K.calls if c in NEW]
    # an explicit --generator_output logits is the same run
    flagged = make(tmp_path, "flagged", resume=False, generator_output="logits", relax_tau="0.5")
    flagged.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    assert set(torch.load(flagged._ckpt_path())) == {"itr", "G", "D", "G_adam", "D_adam", "val"}
    fr = _records(tmp_path, "flagged")
    assert fr[0]["disc_loss"] == recs[0]["disc_loss"] and fr[1] == recs[1] and not [c for c in K.calls if c in NEW]


def test_evaluation_of_a_relaxed_checkpoint_scores_softmax_at_the_checkpoints_tau(relax_train, tmp_path):
    T, K, make = relax_train
    gan = make(tmp_path, "relaxed", resume=False, generator_output="gumbel", relax_tau="2,0.5,4")
    gan.train(max_iterations=2, log_every=1, validate_every=0, test_at_end=False)
    fresh = make(tmp_path, "relaxed", resume=False)       # an evaluation run: no flags, the mode comes from the checkpoint
    assert fresh.load_checkpoint() and fresh.relax_mode == "gumbel" and fresh.itr == 2
    tau = T.relax_tau_at((2.0, 0.5, 4), 2)
    assert abs(tau - 1.0) < 1e-15
    del K.relax_log[:]
    # site 1: test()
    out = str(tmp_path / "recalls.txt")
    fresh.test(max_images=1, out_path=out)
    assert len(K.relax_log) == 1 and K.relax_log[0] == {"tau": tau, "gumbel": False, "seed": 0, "draw": 0, "in_place": True}
    assert '# generator_output: {"mode": "gumbel", "tau": 1.0}' in open(out).read()
    # site 2: predict() / write_predictions() / evaluate()
    recs = fresh.predict(max_images=1)
    assert len(K.relax_log) == 2 and K.relax_log[1] == K.relax_log[0] and recs[0]["n_distinct"] >= 1
    index = fresh.write_predictions(str(tmp_path / "graphs"), max_images=1)
    assert index["generator_output"] == {"mode": "gumbel", "tau": 1.0}
    assert json.load(open(str(tmp_path / "graphs" / "index.json")))["generator_output"] == {"mode": "gumbel", "tau": 1.0}
    assert len(K.relax_log) == 3 and all(not c["gumbel"] and c["in_place"] for c in K.relax_log)
    # the scores are those of the critic on softmax(logits / tau): Discriminator.score_samples against its own two steps
    g = torch.Generator().manual_seed(1)
    images = torch.randn((1, 32, 32, 3), generator=g)
    logits = fresh.g.sample(images, 3, torch.randn((3, 1, 512), generator=g)).clone()
    want = fresh.d.score_samples(torch.softmax(logits / tau, dim=-1), images).clone()
    got = fresh.d.score_samples(logits, images, relax_tau=tau)
    assert float((got - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    assert float((logits.sum(dim=-1) - 1.0).abs().max()) < 1e-5, "relaxed in place"
