"""CPU: the straight-through (hard) relaxation (csrc/relax.hip's sgg_relax_rows_hard / sgg_relax_rows_hard_bwd, GanStep.set_relaxation
(hard=True), train.py --relax_hard) in fp64 on the kernel-level reference: the restatement's known answers, the host logic of the step
against autograd on the oracle composed with y_hard + y_soft - y_soft.detach(), accumulation, the data-parallel path over gloo, the
guard and the weight average, the unchanged default and soft modes, and train.py on the reference kernels.

Bounds: those of tests/test_relax_cpu.py (both sides fp64, differing by summation order): GRAD_RTOL on gradients where the issue names
it (the fp64 sides agree to 1e-8, far inside it), 1e-9 on parameters after Adam, 1e-8 for accumulated against whole batch and two ranks
against one process."""
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
from tests import relax_hard_ref as HR
from tests import relax_ref as RR
from tests.test_relax_cpu import RelaxRefKernels, SEED, _pick, _states, oracle_relax
from tests.test_step_cpu import rel_err
from tests.test_xent_cpu import XentRefKernels, cpu_train  # noqa: F401  (cpu_train: the fixture)
from tests.tolerances import GRAD_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
V, B = 11, 2
SOFT = ("relax_rows", "relax_rows_bwd")
HARD = ("relax_rows_hard", "relax_rows_hard_bwd")


class RelaxHardRefKernels(RelaxRefKernels):
    """RelaxRefKernels with torch fp64 versions of the two straight-through entry points; every call of them is recorded, with its
    arguments in `hard_log`."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.hard_log = []

    def _noisy(self, x, gumbel, seed, draw):
        z = x.reshape(-1, x.shape[-1])
        if gumbel:
            z = z - torch.log(-torch.log(torch.from_numpy(RR.uniforms(seed, draw, z.shape[0], z.shape[1])).to(z.dtype)))
        return z

    def relax_rows_hard(self, x, y=None, tok=None, gumbel=False, seed=0, draw=0):
        self.calls.append("relax_rows_hard")
        self.hard_log.append({"op": "fwd", "gumbel": bool(gumbel), "seed": int(seed), "draw": int(draw), "in_place": y is None and tok is None})
        if y is None and tok is None:
            y = x
        k = torch.argmax(self._noisy(x, gumbel, seed, draw), dim=-1)        # (the first index on ties)
        if y is not None:
            y.copy_(torch.nn.functional.one_hot(k, x.shape[-1]).to(y.dtype).reshape(y.shape))
        if tok is not None:
            tok.copy_(k.reshape(tok.shape))
        return y, tok

    def relax_rows_hard_bwd(self, x, dy, tau, scale=1.0, gumbel=False, seed=0, draw=0, dx=None):
        self.calls.append("relax_rows_hard_bwd")
        self.hard_log.append({"op": "bwd", "tau": float(tau), "gumbel": bool(gumbel), "seed": int(seed), "draw": int(draw), "in_place": dx is None})
        if dx is None:
            dx = dy
        assert dx.data_ptr() != x.data_ptr(), "dx must not alias x"
        y = torch.softmax(self._noisy(x, gumbel, seed, draw) / float(tau), dim=-1).reshape(dy.shape)
        dx.copy_((float(scale) / float(tau)) * y * (dy - (y * dy).sum(dim=-1, keepdim=True)))
        return dx


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    x = np.array([[0.0, 2.0, 2.0, -1.0], [0.5, 0.5, 0.5, 0.5], [3.0, 1.0, 0.0, 2.5]])
    y, tok, margin = HR.relax_rows_hard(x)
    assert tok.tolist() == [1, 0, 0], "the first index of the maximum"
    assert np.array_equal(y, [[0, 1, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]]) and np.allclose(margin, [0.0, 0.0, 0.5], rtol=0, atol=1e-15)
    # with noise: the argmax of x + g, and the Gumbel-max property - tok is a draw from softmax(x)
    p = np.array([0.4, 0.25, 0.2, 0.1, 0.05])
    rows = 20000
    _, tok, _ = HR.relax_rows_hard(np.tile(np.log(p), (rows, 1)), True, SEED, 5)
    freq, se = np.bincount(tok, minlength=5) / rows, np.sqrt(p * (1 - p) / rows)
    assert (np.abs(freq - p) <= 4.0 * se).all(), (freq, p)
    g = RR.gumbel(RR.uniforms(SEED, 5, 3, 4))
    assert np.array_equal(HR.relax_rows_hard(x, True, SEED, 5)[1], (x + g).argmax(axis=1))
    # the backward is relax_ref's on the recomputed soft row
    dy = np.random.RandomState(1).standard_normal(x.shape)
    for gumbel in (False, True):
        ysoft, _ = RR.relax_rows(x, 0.5, gumbel, SEED, 5)
        assert np.array_equal(HR.relax_rows_hard_bwd(x, dy, 0.5, 1.7, gumbel, SEED, 5), RR.relax_rows_bwd(ysoft, dy, 0.5, 1.7))


def test_torch_entry_points_follow_the_restatement():
    K = RelaxHardRefKernels()
    g = np.random.RandomState(3)
    x, dy = 3.0 * g.standard_normal((6, 7)), g.standard_normal((6, 7))
    for gumbel in (False, True):
        y, tok = torch.zeros(6, 7, dtype=DT), torch.zeros(6, dtype=torch.int64)
        K.relax_rows_hard(torch.from_numpy(x), y=y, tok=tok, gumbel=gumbel, seed=SEED, draw=9)
        yref, tref, _ = HR.relax_rows_hard(x, gumbel, SEED, 9)
        assert np.array_equal(y.numpy(), yref) and np.array_equal(tok.numpy(), tref)
        xi = torch.from_numpy(x.copy())
        assert K.relax_rows_hard(xi, gumbel=gumbel, seed=SEED, draw=9)[0] is xi and torch.equal(xi, y), "in place"
        d = torch.from_numpy(dy.copy())
        K.relax_rows_hard_bwd(torch.from_numpy(x), d, 0.5, scale=2.0, gumbel=gumbel, seed=SEED, draw=9)
        assert np.abs(d.numpy() - HR.relax_rows_hard_bwd(x, dy, 0.5, 2.0, gumbel, SEED, 9)).max() < 1e-14
    assert K.calls == ["relax_rows_hard", "relax_rows_hard", "relax_rows_hard_bwd"] * 2


# ---- host logic in fp64: autograd on the oracle composed with the straight-through estimator -----------------------------------------
def _fresh(S=32, rows=B, reducer=None, K=None, relax=None):
    gp, dp_ = _states(S)
    gs = GanStep(K if K is not None else RelaxHardRefKernels(), V, S, rows, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer)
    if relax is not None:
        gs.set_relaxation(*relax[:3], **({"hard": relax[3]} if len(relax) > 3 else {}))
    return gs, gp, dp_


def oracle_hard(fake, mode, tau, seed=0, draw=0):
    """(straight-through rows y_hard + y_soft - y_soft.detach() of the oracle's logits [B, 3, V], tokens [B, 3], margin of x + g)."""
    x = fake
    if mode == "gumbel":
        u = RR.uniforms(seed, draw, fake.shape[0] * fake.shape[1], fake.shape[2]).reshape(tuple(fake.shape))
        x = x - torch.log(-torch.log(torch.from_numpy(u).to(fake.dtype)))
    tok = torch.argmax(x.detach(), dim=-1)
    top2 = torch.topk(x.detach(), 2, dim=-1).values
    soft = oracle_relax(fake, mode, tau, seed, draw)
    hard = torch.nn.functional.one_hot(tok, fake.shape[-1]).to(fake.dtype)
    return hard + soft - soft.detach(), tok, float((top2[..., 0] - top2[..., 1]).min())


def oracle_g_cost_hard(gp, dp_, images, noise, mode, tau, seed=0, draw=0, labels=None, w=0.0):
    """generator_forward -> straight-through rows -> discriminator_forward [+ w * cross-entropy of the LOGITS];
    returns (cost, grads of gp, tokens, margin)."""
    gp = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    fake = O.generator_forward(gp, images, noise)
    st, tok, margin = oracle_hard(fake, mode, tau, seed, draw)
    cost = -O.discriminator_forward(dp_, st, images).mean()
    if w > 0.0:
        cost = cost + w * (-torch.log_softmax(fake, dim=-1).gather(-1, labels.unsqueeze(-1)).sum() / images.shape[0])
    return cost.detach(), O._grads(cost, gp), tok, margin


def oracle_d_cost_hard(gp, dp_, images, onehot, noise, alpha, lam, mode, tau, seed=0, draw=0):
    """d_loss's body with the hard fake (a constant for D); returns (cost, aux, grads of dp, tokens, margin)."""
    dp_ = {k: v.clone().requires_grad_(True) for k, v in dp_.items()}
    with torch.no_grad():
        st, tok, margin = oracle_hard(O.generator_forward(gp, images, noise), mode, tau, seed, draw)
        fake = torch.nn.functional.one_hot(tok, st.shape[-1]).to(st.dtype)
    feat_d = O.encoder(dp_, images)
    d_fake, d_real = O.discriminator_head(dp_, feat_d, fake), O.discriminator_head(dp_, feat_d, onehot)
    gpen, slopes, _ = O.gradient_penalty(dp_, feat_d, onehot, fake, alpha)
    cost = d_fake.mean() - d_real.mean() + lam * gpen
    return cost.detach(), {"gp": gpen.detach(), "d_fake": d_fake.detach()}, O._grads(cost, dp_), tok, margin


MODES = [("softmax", 1.0), ("softmax", 0.5), ("gumbel", 1.0), ("gumbel", 0.5)]


@pytest.mark.parametrize("mode,tau", MODES)
def test_generator_step_matches_autograd_through_the_straight_through_rows(mode, tau):
    S = 32
    images, labels, _ = O.synth_batch(B, S, V, dtype=DT)
    noise = O.synth_noise(B, 1, DT)
    for w in (0.0, 0.3):
        gs, gp, dp_ = _fresh(S, relax=(mode, tau, SEED, True))
        kw = {"labels": labels, "mle_weight": w} if w > 0.0 else {}
        cost, grads, tok, _ = oracle_g_cost_hard(gp, dp_, images, noise, mode, tau, SEED, 41, labels, w)
        gl = gs.generator_step(images, noise, draw=41, **kw)
        assert [c for c in gs.K.calls if c in SOFT + HARD] == ["relax_rows_hard", "relax_rows_hard_bwd"]
        draw = 41 if mode == "gumbel" else 0
        assert gs.K.hard_log == [{"op": "fwd", "gumbel": mode == "gumbel", "seed": SEED, "draw": draw, "in_place": False},
                                 {"op": "bwd", "tau": tau, "gumbel": mode == "gumbel", "seed": SEED, "draw": draw, "in_place": True}]
        # D's input is the one-hot row of the oracle's token
        assert torch.equal(gs._relax_buf, torch.nn.functional.one_hot(tok, V).to(DT))
        for name, g in grads.items():
            e = rel_err(gs.G.grads[name], g)
            assert e < GRAD_RTOL and e < 1e-8, "generator grad %s rel err %.3e (%s, tau %g, w %g)" % (name, e, mode, tau, w)
        m, v = O.new_adam_state(gp)
        O.tf_adam_step(gp, grads, m, v, 1)
        for name in gp:
            if not O.is_dead(name):
                assert rel_err(gs.G.arena.views[name], gp[name]) < 1e-9, "generator param after Adam: " + name
        if w == 0.0:
            assert abs(-float(gl[3]) - float(cost)) < 1e-9


@pytest.mark.parametrize("mode,tau", MODES)
def test_the_soft_step_is_far_outside_the_bound_against_the_hard_oracle(mode, tau):
    S = 32
    images, _, _ = O.synth_batch(B, S, V, dtype=DT)
    noise = O.synth_noise(B, 1, DT)
    soft, gp, dp_ = _fresh(S, relax=(mode, tau, SEED))
    soft.generator_step(images, noise, draw=41)
    _, grads, _, _ = oracle_g_cost_hard(gp, dp_, images, noise, mode, tau, SEED, 41)
    e = rel_err(soft.G.grads["decoder/bias"], grads["decoder/bias"])
    print("soft step against the hard oracle (%s, tau %g): decoder/bias rel err %.3e" % (mode, tau, e))
    assert e > 100 * GRAD_RTOL


@pytest.mark.parametrize("mode,tau", MODES)
def test_critic_step_and_critic_loss_match_autograd_on_the_hard_fake(mode, tau):
    S = 32
    gs, gp, dp_ = _fresh(S, relax=(mode, tau, SEED, True))
    images, labels, onehot = O.synth_batch(B, S, V, dtype=DT)
    noise, alpha = O.synth_noise(B, 0, DT), O.synth_alpha(B, 0, DT)
    cost, aux, grads, tok, _ = oracle_d_cost_hard(gp, dp_, images, onehot, noise, alpha, 10.0, mode, tau, SEED, 7)
    val = gs.critic_loss(images, labels, noise, alpha.reshape(B), draw=7).clone()
    dl = gs.critic_step(images, labels, noise, alpha.reshape(B), draw=7).clone()
    assert [c for c in gs.K.calls if c in SOFT + HARD] == ["relax_rows_hard"] * 2, "the critic's update treats the rows as constants"
    assert abs(float(dl[0]) - float(cost)) < 1e-9 * max(1.0, abs(float(cost))) and abs(float(dl[2]) - float(aux["gp"])) < 1e-9
    assert abs(float(dl[3]) - float(aux["d_fake"].mean())) < 1e-9 and torch.allclose(val, dl, rtol=0, atol=1e-12)
    for name, g in grads.items():
        if g is None:
            continue
        e = rel_err(gs.D.grads[name], g)
        assert e < GRAD_RTOL and e < 1e-8, "critic grad %s rel err %.3e (%s, tau %g)" % (name, e, mode, tau)
    m, v = O.new_adam_state(dp_)
    O.tf_adam_step(dp_, grads, m, v, 1)
    for name in dp_:
        if not O.is_dead(name):
            assert rel_err(gs.D.arena.views[name], dp_[name]) < 1e-9, "critic param after Adam: " + name
    assert torch.equal(gs.TRI[:B], torch.nn.functional.one_hot(tok, V).to(DT)), "the fake rows D saw are the one-hot rows"


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def _iterations(rows, Bm, pick, mode, reducer=None, guard=None, decay=None, draws=None, seed=SEED):
    """tests/test_relax_cpu.py's _iterations with the hard option: two GAN iterations (two critic updates each) over `rows` rows,
    each update from len(pick) micro-batches of Bm rows.  draws[k]: the draw offset of micro-batch k (gumbel)."""
    S, N, C = 32, len(pick), 2
    images, labels, _ = O.synth_batch(rows, S, V, dtype=DT)
    gs, _, _ = _fresh(S, Bm, reducer=reducer, relax=(mode, 0.5, seed, True))
    if guard is not None:
        gs.set_guard((guard, guard), False)
    if decay is not None:
        gs.G.enable_averaging(decay)
    draws = draws if draws is not None else list(range(N))
    for it in range(2):
        noises = [[_pick(O.synth_noise(rows, 10 * it + i, DT), p) for p in pick] for i in range(C + 1)]
        alphas = [[_pick(O.synth_alpha(rows, 10 * it + i, DT).reshape(rows), p) for p in pick] for i in range(C)]
        dr = [[1000 * it + 100 * i + draws[k] for k in range(N)] for i in range(C + 1)]
        gs.train_iteration_accumulated([(_pick(images, p), _pick(labels, p)) for p in pick], noises, alphas, critic_iters=C, draws=dr)
    gs.flush()
    return gs, {"G": gs.G.arena.flat.clone(), "D": gs.D.arena.flat.clone(), "Gm": gs.G.m_flat.clone(), "Dm": gs.D.m_flat.clone()}


def test_accumulated_equals_the_large_batch():
    """softmax + hard (without noise a row's token does not depend on its place in the launch)."""
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


def test_two_ranks_equal_the_single_process_in_gumbel_hard_mode(tmp_path):
    out = str(tmp_path / "rank%d.pt")
    port = 41500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(r0["G"], r1["G"]) and torch.equal(r0["D"], r1["D"]), "replicas diverged"
    _, want = _iterations(4, 2, [[0, 1], [2, 3]], "gumbel", draws=[0, 1])
    for key in want:
        err = float((r0[key] - want[key]).abs().max())
        print("%s: world 2 x B 2 vs 2 micro-batches differ by %.3e" % (key, err))
        assert err < 1e-8, (key, err)
    _, moved = _iterations(4, 2, [[0, 1], [2, 3]], "gumbel", draws=[5, 6])
    assert float((moved["G"] - want["G"]).abs().max()) > 1e3 * 1e-8


def test_guard_and_average_apply_to_the_hard_updates():
    twin, _, _ = _fresh(relax=("gumbel", 0.5, SEED, True))
    images, labels, _ = O.synth_batch(2, 32, V, dtype=DT)
    twin.generator_step(images, O.synth_noise(2, 0, DT), draw=3)
    norm = float(twin.G.arena.live(twin.G.grad_flat).pow(2).sum().sqrt())
    assert norm > 0
    first, _, _ = _fresh(relax=("gumbel", 0.5, SEED, True))
    first.set_guard((0.0, norm / 4.0), False)
    first.G.enable_averaging(0.9)
    init = first.G.arena.flat.clone()
    first.generator_step(images, O.synth_noise(2, 0, DT), draw=3)
    r = first.G.guard_report()
    assert r["clipped"] == 1 and abs(r["coef"] - 0.25) < 1e-12 and abs(r["norm"] - norm) < 1e-12 * norm
    assert float((first.G.m_flat - 0.25 * twin.G.m_flat).abs().max()) <= 1e-12 * float(twin.G.m_flat.abs().max())
    avg = first.G.opt["ema"]
    assert avg["updates"] == 1 and not torch.equal(avg["flat"], init) and not torch.equal(avg["flat"], first.G.arena.flat)


# ---- the option off -------------------------------------------------------------------------------------------------------------------
def _one_iteration(gs, **kw):
    images, labels, _ = O.synth_batch(B, 32, V, dtype=DT)
    gs.train_iteration(images, labels, [O.synth_noise(B, i, DT) for i in range(3)], [O.synth_alpha(B, i, DT).reshape(B) for i in range(2)],
                       critic_iters=2, **kw)
    gs.flush()
    return [t.clone() for net in (gs.G, gs.D) for t in (net.arena.flat, net.grad_flat, net.m_flat, net.v_flat)]


@pytest.mark.parametrize("relax", [None, ("logits", 1.0, 0), ("softmax", 0.5, SEED), ("gumbel", 0.5, SEED)], ids=lambda r: str(r and r[0]))
def test_hard_off_records_the_same_calls_and_keeps_every_bit(relax):
    """hard=False (given or not) and mode logits: the calls recorded and the arenas are those of a step on a kernel set that has
    never heard of the option."""
    never, _, _ = _fresh(K=RelaxRefKernels(), relax=relax)
    want = _one_iteration(never, draws=[1, 2, 3])
    for explicit in (False, True):
        gs, _, _ = _fresh(relax=(relax + (False,) if explicit else relax) if relax is not None else None)
        if relax is None and explicit:
            gs.set_relaxation("logits", hard=False)
        got = _one_iteration(gs, draws=[1, 2, 3])
        assert gs.K.calls == never.K.calls and gs.K.relax_log == never.K.relax_log and not gs.K.hard_log
        assert gs.relaxation == never.relaxation and (gs.relaxation is None or "hard" not in gs.relaxation)
        for a, b in zip(want, got):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    if relax is not None and relax[0] != "logits":
        on, _, _ = _fresh(relax=relax + (True,))
        assert on.relaxation == {"mode": relax[0], "tau": relax[1], "seed": relax[2], "hard": True}
        moved = _one_iteration(on, draws=[1, 2, 3])
        assert not torch.equal(moved[0], want[0]) and not torch.equal(moved[4], want[4])
        # switched off again: the soft step
        on2, _, _ = _fresh(relax=relax + (True,))
        on2.set_relaxation(*relax)
        back = _one_iteration(on2, draws=[1, 2, 3])
        assert "hard" not in on2.relaxation and all(torch.equal(a, b) for a, b in zip(want, back))


def test_hard_with_logits_and_a_kernel_set_without_the_entry_points_are_refused():
    gs, _, _ = _fresh()
    with pytest.raises(ValueError, match="hard"):
        gs.set_relaxation("logits", hard=True)
    assert gs.relaxation is None
    bare, _, _ = _fresh(K=RelaxRefKernels())              # the soft entry points only
    bare.set_relaxation("gumbel", 1.0)
    for mode in ("softmax", "gumbel"):
        with pytest.raises(RuntimeError, match="relax_rows_hard.*relax_rows_hard_bwd"):
            bare.set_relaxation(mode, 1.0, hard=True)
    assert bare.relaxation == {"mode": "gumbel", "tau": 1.0, "seed": 0} and bare.G.adam_t == 0


# ---- train.py on the reference kernels --------------------------------------------------------------------------------------------------
@pytest.fixture
def hard_train(cpu_train, monkeypatch):
    """cpu_train with a RelaxHardRefKernels behind kernels_for."""
    T, _, make = cpu_train
    from sgg_amd import api
    K = RelaxHardRefKernels()
    monkeypatch.setattr(T, "kernels_for", lambda device: K)
    monkeypatch.setattr(api, "kernels_for", lambda device: K)
    return T, K, make


def _records(tmp, name):
    with open(str(tmp / name / "logs" / "losses.jsonl")) as f:
        return [json.loads(l) for l in f if l.strip()]


def test_parser_and_constructor_refuse_hard_with_logits(hard_train, tmp_path):
    T, K, make = hard_train
    a = T.parse_args([])
    assert a.relax_hard is False
    assert T.parse_args(["--generator_output", "gumbel", "--relax_hard"]).relax_hard is True
    assert T.parse_args(["--generator_output", "softmax", "--relax_hard"]).relax_hard is True
    with pytest.raises(SystemExit):
        T.parse_args(["--generator_output", "logits", "--relax_hard"])
    with pytest.raises(ValueError, match="relax_hard"):
        make(tmp_path, "bad", resume=False, generator_output="logits", relax_hard=True)
    # a fresh run whose mode is the default (logits) is refused before the first update
    fresh = make(tmp_path, "bad2", resume=False, relax_hard=True)
    with pytest.raises(ValueError, match="relax_hard"):
        fresh.train(max_iterations=1, test_at_end=False)
    assert not os.path.exists(fresh._ckpt_path()) and not [c for c in K.calls if c in SOFT + HARD]


def test_train_hard_run_resumes_bit_for_bit_and_records_the_key(hard_train, tmp_path):
    T, K, make = hard_train
    kw = dict(generator_output="gumbel", relax_tau="2,0.5,2", critic_iters=2)
    gan = make(tmp_path, "whole", resume=False, relax_hard=True, **kw)
    gan.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    recs = [r for r in _records(tmp_path, "whole") if "triples_per_s" in r]
    assert [r["relax"] for r in recs] == [{"mode": "gumbel", "tau": t, "hard": True} for t in (2.0, 1.0, 0.5)]
    ck = torch.load(gan._ckpt_path())
    assert ck["generator_output"] == {"mode": "gumbel", "tau": [2.0, 0.5, 2], "hard": True}
    # nothing soft was launched; every forward has a draw of its own, and each backward takes its forward's
    assert not [c for c in K.calls if c in SOFT]
    fwd = [c for c in K.hard_log if c["op"] == "fwd" and c["draw"] < 2 ** 63]
    bwd = [c for c in K.hard_log if c["op"] == "bwd"]
    val = [c["draw"] for c in K.hard_log if c["op"] == "fwd" and c["draw"] >= 2 ** 63]
    assert len(fwd) == 9 and len({c["draw"] for c in fwd}) == 9 and val == [T.relax_val_draw(k) for k in range(3)]
    assert [c["draw"] for c in bwd] == [T.relax_draw(it, 2, 0, 2, 1) for it in range(3)] and [c["tau"] for c in bwd] == [2.0, 1.0, 0.5]
    assert all(c["gumbel"] and c["seed"] == gan._relax_seed() for c in K.hard_log)
    # stopped after one iteration and resumed WITHOUT the flags: the option comes from the checkpoint, the same weights bit for bit
    part = make(tmp_path, "parts", resume=False, relax_hard=True, **kw)
    part.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    rest = make(tmp_path, "parts", resume=True, critic_iters=2)
    rest.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    assert rest.relax_hard is True
    ck2 = torch.load(rest._ckpt_path())
    assert ck2["generator_output"] == ck["generator_output"]
    for net in ("G", "D"):
        for name, t in ck[net].items():
            assert torch.equal(t, ck2[net][name]), "%s %s differs after the resume" % (net, name)
    # the flag on a soft or plain checkpoint contradicts it: an error on resume and at evaluation, before anything is loaded
    soft = make(tmp_path, "soft", resume=False, **kw)
    soft.train(max_iterations=1, log_every=1, validate_every=0, test_at_end=False)
    ck_soft = torch.load(soft._ckpt_path())
    assert ck_soft["generator_output"] == {"mode": "gumbel", "tau": [2.0, 0.5, 2]}, "a soft run's checkpoint keeps its keys"
    assert [r["relax"] for r in _records(tmp_path, "soft") if "triples_per_s" in r] == [{"mode": "gumbel", "tau": 2.0}]
    plain = make(tmp_path, "plain", resume=False)
    plain.train(max_iterations=1, log_every=1, validate_every=0, test_at_end=False)
    for name in ("soft", "plain"):
        with pytest.raises(ValueError, match="contradicts"):
            make(tmp_path, name, resume=True, critic_iters=2, relax_hard=True).train(max_iterations=2, test_at_end=False)
        bad = make(tmp_path, name, resume=False, relax_hard=True)
        with pytest.raises(ValueError, match="contradicts"):
            bad.load_checkpoint()
        assert bad.itr == 0, "nothing was loaded"


def test_evaluation_of_a_hard_checkpoint_scores_onehot_of_the_argmax(hard_train, tmp_path):
    T, K, make = hard_train
    gan = make(tmp_path, "hard", resume=False, generator_output="gumbel", relax_tau="2,0.5,4", relax_hard=True)
    gan.train(max_iterations=2, log_every=1, validate_every=0, test_at_end=False)
    fresh = make(tmp_path, "hard", resume=False)          # an evaluation run (--test_only): no flags, everything from the checkpoint
    assert fresh.load_checkpoint() and fresh.relax_mode == "gumbel" and fresh.relax_hard is True and fresh.itr == 2
    del K.hard_log[:], K.relax_log[:]
    label = {"mode": "gumbel", "tau": 1.0, "hard": True}
    # site 1: test()
    out = str(tmp_path / "recalls.txt")
    fresh.test(max_images=1, out_path=out)
    assert K.hard_log == [{"op": "fwd", "gumbel": False, "seed": 0, "draw": 0, "in_place": True}] and not K.relax_log
    assert "# generator_output: " + json.dumps(label) in open(out).read()
    # site 2: predict() / write_predictions() / evaluate()
    recs = fresh.predict(max_images=1)
    assert len(K.hard_log) == 2 and K.hard_log[1] == K.hard_log[0] and recs[0]["n_distinct"] >= 1
    index = fresh.write_predictions(str(tmp_path / "graphs"), max_images=1)
    assert index["generator_output"] == label and json.load(open(str(tmp_path / "graphs" / "index.json")))["generator_output"] == label
    assert len(K.hard_log) == 3 and not K.relax_log
    # the scores are the critic's on onehot(argmax(logits)): Discriminator.score_samples against its own two steps
    g = torch.Generator().manual_seed(1)
    images = torch.randn((1, 32, 32, 3), generator=g)
    logits = fresh.g.sample(images, 3, torch.randn((3, 1, 512), generator=g)).clone()
    tok = torch.argmax(logits, dim=-1)
    want = fresh.d.score_samples(torch.nn.functional.one_hot(tok, logits.shape[-1]).to(logits.dtype), images).clone()
    got = fresh.d.score_samples(logits, images, relax_tau=1.0, relax_hard=True)
    assert torch.equal(got, want)
    assert torch.equal(logits, torch.nn.functional.one_hot(tok, logits.shape[-1]).to(logits.dtype)), "replaced in place"
