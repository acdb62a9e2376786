"""CPU: the generator likelihood (csrc/xent.hip, GanStep.pretrain_step / generator_step(mle_weight) / generator_nll, train.py's
--pretrain_iterations, --mle_weight, --validate_nll and likelihood()) in fp64 on the kernel-level reference: known answers of the
restatement (tests/xent_ref.py), the host logic of the step against autograd on the oracle, accumulation, the data-parallel path over
gloo, the guard and the weight average, and train.py on the reference kernels.

Bounds: those of tests/test_step_cpu.py and tests/test_guard_cpu.py, for the same reasons - both sides are fp64 and differ by
summation order only: 1e-8 on gradients (relative to the tensor's largest element), 1e-9 on parameters after Adam, 1e-8 for
accumulated against whole batch and two ranks against one process."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from oracle.kernels_ref import RefKernels
from sgg_amd import diagnostics as dg
from sgg_amd.step import GanStep
from tests import xent_ref as XR
from tests.test_guard_cpu import GuardRefKernels
from tests.test_step_cpu import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = torch.float64
V, B = 11, 2
NEW = ("softmax_xent", "xent_summary", "triple_logp")


class XentRefKernels(GuardRefKernels):
    """The kernel-level reference (with the entry points of csrc/optim.hip and csrc/guard.hip that the step needs) carrying torch
    versions of the three entry points of csrc/xent.hip in the arithmetic of their tensors; every call of them is recorded."""

    def softmax_xent(self, logits, labels=None, scale=1.0, accumulate=False, dlogits=None, nll=None, lse=None, hit=None):
        self.calls.append("softmax_xent")
        Vx = logits.shape[-1]
        x = logits.reshape(-1, Vx)
        R = x.shape[0]
        m = x.max(dim=1, keepdim=True).values
        l = (m + torch.log(torch.exp(x - m).sum(dim=1, keepdim=True)))[:, 0]
        if lse is not None:
            lse.copy_(l.reshape(lse.shape))
        if labels is None:
            assert dlogits is None and nll is None and hit is None, "labels = None is the lse-only mode"
            return
        lab = labels.reshape(-1)
        valid = (lab >= 0) & (lab < Vx)
        safe = torch.where(valid, lab, torch.zeros_like(lab))
        rows = torch.arange(R)
        if nll is not None:
            nll.copy_(torch.where(valid, l - x[rows, safe], torch.zeros_like(l)))
        if hit is not None:
            hit.copy_(torch.where(valid, (O.argmax_tokens(x) == safe).to(torch.int32), torch.full((R,), -1, dtype=torch.int32)))
        if dlogits is not None:
            g = torch.exp(x - l[:, None])
            g[rows, safe] -= 1.0
            g = scale * g
            d = dlogits.view(-1, Vx)
            if accumulate:
                d[valid] += g[valid]
            else:
                d.copy_(g * valid[:, None].to(g.dtype))

    def xent_summary(self, nll, hit, out=None):
        self.calls.append("xent_summary")
        h = hit.reshape(-1, 3)
        valid = h >= 0
        n, full = int(valid.sum()), valid.all(dim=1)
        if out is None:
            out = torch.zeros(4, dtype=nll.dtype)
        out[0] = nll.reshape(-1, 3)[valid].sum() / n if n else 0.0
        out[1] = float((h[valid] == 1).sum()) / n if n else 0.0
        out[2] = float((h[full] == 1).all(dim=1).sum()) / int(full.sum()) if bool(full.any()) else 0.0
        out[3] = float(n)
        return out

    # the statistics pass of csrc/stats.hip through its fp64 restatement (sgg_amd.diagnostics), so that train.py's
    # --diagnostics_every runs on this kernel set
    def arena_stats_chunk(self):
        return dg.CHUNK

    def arena_stats_nstat(self):
        return dg.NSTAT

    def arena_stats_workspace_bytes(self, n_chunks):
        return 8

    def arena_stats(self, params, grads, m, v, table, n_tensors, lr_t, eps, grad_scale=1.0, out=None, ws=None, grid=0):
        t = table.numpy()
        offsets = [int(t[t[:, 0] == k, 1].min()) for k in range(n_tensors)]
        numels = [int(t[t[:, 0] == k, 2].sum()) for k in range(n_tensors)]
        rows = dg.stats_reference(params.numpy(), grads.numpy(), m.numpy(), v.numpy(), offsets, numels, lr_t, eps, grad_scale)
        out.copy_(torch.from_numpy(rows))
        return out

    def vector_stats(self, x, threshold, out=None):
        out.copy_(torch.from_numpy(dg.vector_stats_reference(x.numpy(), threshold)))
        return out

    def triple_logp(self, logits, lse, gt, gt_count, out=None):
        self.calls.append("triple_logp")
        N, nb, _, Vx = logits.shape
        M = gt.shape[1]
        ref = XR.triple_logp(logits.numpy(), lse.reshape(N, nb, 3).numpy(), gt.numpy(), gt_count.numpy())
        res = {}
        for name, dt in (("mix", logits.dtype), ("mean", logits.dtype), ("slot", logits.dtype), ("status", torch.int32)):
            t = torch.from_numpy(np.asarray(ref[name])).to(dt)
            if out is not None:
                out[name].copy_(t)
                t = out[name]
            res[name] = t
        return res


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_softmax_xent_known_answers():
    r = XR.softmax_xent(np.zeros((3, 2)), [0, 1, 0], scale=2.0)
    assert np.allclose(r["nll"], np.log(2.0), rtol=0, atol=1e-15) and np.allclose(r["lse"], np.log(2.0), rtol=0, atol=1e-15)
    assert np.allclose(r["dlogits"], [[-1.0, 1.0], [1.0, -1.0], [-1.0, 1.0]], rtol=0, atol=1e-15)      # 2 * (1/2 - onehot)
    assert r["hit"].tolist() == [1, 0, 1], "on a tie the hit goes to the first index"
    # a row of +-80 does not overflow: lse = 80 + log(2 + 2 exp(-160))
    big = XR.softmax_xent(np.array([[80.0, -80.0, 80.0, -80.0]]), [1])
    assert np.isfinite(big["lse"]).all() and abs(big["lse"][0] - (80.0 + np.log(2.0))) < 1e-13 and abs(big["nll"][0] - (160.0 + np.log(2.0))) < 1e-12
    assert big["hit"].tolist() == [0]
    # an out-of-range label is skipped: nll 0, hit -1, gradient row zero (stored) or left as it was (accumulated)
    x = np.array([[1.0, 2.0, 3.0], [0.5, 0.5, 0.5], [3.0, 2.0, 1.0]])
    d0 = np.full((3, 3), 7.0)
    for lab in (3, -1):
        s = XR.softmax_xent(x, [2, lab, 0], scale=0.5)
        assert s["nll"][1] == 0.0 and s["hit"].tolist() == [1, -1, 1] and (s["dlogits"][1] == 0.0).all()
        a = XR.softmax_xent(x, [2, lab, 0], scale=0.5, accumulate=True, dlogits=d0)
        assert (a["dlogits"][1] == 7.0).all(), "accumulate = 1 leaves a skipped row untouched"
        assert np.allclose(a["dlogits"][[0, 2]], 7.0 + s["dlogits"][[0, 2]], rtol=0, atol=1e-15), "accumulate = 1 adds to what is there"
    # every gradient row sums to zero, and the lse-only mode gives the same lse
    assert np.abs(s["dlogits"].sum(axis=1)).max() < 1e-15
    assert np.array_equal(XR.softmax_xent(x)["lse"], s["lse"]) and set(XR.softmax_xent(x)) == {"lse"}


def test_xent_summary_known_answers():
    nll = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0])
    hit = np.array([1, 1, 1, 1, 0, 1, 1, -1, 1])
    assert XR.xent_summary(nll, hit).tolist() == [(45.0 - 8.0) / 8, 7.0 / 8, 0.5, 8.0]
    assert XR.xent_summary(nll, np.full(9, -1)).tolist() == [0.0, 0.0, 0.0, 0.0]


def test_triple_logp_known_answers():
    g = np.random.RandomState(0)
    x = g.standard_normal((1, 2, 3, 5))
    lse = XR.lse64(x)
    gt = np.array([[[0, 1, 2], [4, 4, 4], [9, 9, 9]], [[1, 5, 0], [0, -1, 0], [3, 3, 3]]])
    r = XR.triple_logp(x, lse, gt, [2, 3])
    assert r["status"].tolist() == [[0, 0, -3], [-4, -4, 0]], "padding rows get -3, out-of-range tokens -4"
    ok = r["status"] == 0
    assert np.isnan(r["mix"][~ok]).all() and np.isnan(r["mean"][~ok]).all() and np.isnan(r["slot"][~ok]).all()
    lp = (x[0, 0, 0, 0] - lse[0, 0, 0]) + (x[0, 0, 1, 1] - lse[0, 0, 1]) + (x[0, 0, 2, 2] - lse[0, 0, 2])
    assert abs(r["mix"][0, 0] - lp) < 1e-15 and np.array_equal(r["mix"][ok], r["mean"][ok]), "N = 1: mix == mean == lp"
    assert np.allclose(r["slot"][ok].sum(axis=1), r["mean"][ok], rtol=0, atol=1e-14)
    # two samples: the mixture is the log of the mean probability, the mean is the mean log-probability (Jensen: mix >= mean)
    x2 = g.standard_normal((2, 1, 3, 5))
    r2 = XR.triple_logp(x2, XR.lse64(x2), np.array([[[1, 2, 3]]]), [1])
    p = np.exp(x2 - XR.lse64(x2)[..., None])
    pk = p[:, 0, 0, 1] * p[:, 0, 1, 2] * p[:, 0, 2, 3]
    assert abs(r2["mix"][0, 0] - np.log(pk.mean())) < 1e-14 and abs(r2["mean"][0, 0] - np.log(pk).mean()) < 1e-14
    assert r2["mix"][0, 0] >= r2["mean"][0, 0]


def test_torch_entry_points_follow_the_restatement():
    """The torch versions the step tests run on are the restatement's arithmetic."""
    K = XentRefKernels()
    g = np.random.RandomState(3)
    x = 3.0 * g.standard_normal((6, 7))
    lab = np.array([0, 6, 7, -1, 3, 2])
    x[4, 1] = x[4, 3] = x[4].max() + 1.0          # a tie at the maximum: label 3 is its second index
    d0 = g.standard_normal((6, 7))
    for acc in (False, True):
        d, nll, lse, hit = torch.from_numpy(d0.copy()), torch.zeros(6, dtype=DT), torch.zeros(6, dtype=DT), torch.zeros(6, dtype=torch.int32)
        K.softmax_xent(torch.from_numpy(x), torch.from_numpy(lab), scale=0.25, accumulate=acc, dlogits=d, nll=nll, lse=lse, hit=hit)
        ref = XR.softmax_xent(x, lab, scale=0.25, accumulate=acc, dlogits=d0)
        assert np.abs(d.numpy() - ref["dlogits"]).max() < 1e-14 and np.abs(nll.numpy() - ref["nll"]).max() < 1e-14
        assert np.abs(lse.numpy() - ref["lse"]).max() < 1e-14 and np.array_equal(hit.numpy(), ref["hit"]) and ref["hit"][4] == 0
    got = K.xent_summary(nll, hit).numpy()
    assert np.abs(got - XR.xent_summary(ref["nll"], ref["hit"])).max() < 1e-14


# ---- host logic in fp64 ---------------------------------------------------------------------------------------------------------
def _states(S):
    gp, dp_ = O.init_params("G", V, S, dtype=DT, perturb=0.1), O.init_params("D", V, S, dtype=DT, perturb=0.1)
    dp_["W"] = dp_["W"] * 25.0
    return gp, dp_


def _fresh(S=32, rows=B, reducer=None, K=None):
    gp, dp_ = _states(S)
    return GanStep(K if K is not None else XentRefKernels(), V, S, rows, g_state=gp, d_state=dp_, dtype=DT, reducer=reducer), gp, dp_


def _oracle_mle(gp, images, labels, noise, dp_=None, w=1.0):
    """Autograd on cloned parameters: cost = [g_loss +] w * (1/B) sum_b sum_t -log_softmax(logits[b, t])[labels[b, t]]."""
    gp = {k: v.clone().requires_grad_(True) for k, v in gp.items()}
    if dp_ is None:
        fake, gan = O.generator_forward(gp, images, noise), 0.0
    else:
        gan, aux = O.g_loss(gp, dp_, images, noise)
        fake = aux["fake"]
    xent = -torch.log_softmax(fake, dim=-1).gather(-1, labels.unsqueeze(-1)).sum() / images.shape[0]
    grads = O._grads(gan + w * xent, gp)
    return float(xent.detach()), fake.detach(), grads


def _d_state(gs):
    return [t.clone() for t in (gs.D.arena.flat, gs.D.grad_flat, gs.D.m_flat, gs.D.v_flat)]


@pytest.mark.parametrize("S", [32, 29])
def test_pretrain_step_matches_autograd_and_adam(S):
    gs, gp, _ = _fresh(S)
    images, labels, _ = O.synth_batch(B, S, V, dtype=DT)
    noise = O.synth_noise(B, 0, DT)
    d_before = _d_state(gs)
    xent, fake, grads = _oracle_mle(gp, images, labels, noise)
    val = gs.generator_nll(images, labels, noise).clone()
    ml = gs.pretrain_step(images, labels, noise).clone()
    assert gs.K.calls == ["softmax_xent", "xent_summary"] * 2 and torch.equal(val, ml)
    hits = O.argmax_tokens(fake) == labels
    assert abs(float(ml[0]) - xent / 3.0) < 1e-9 and float(ml[3]) == 3 * B
    assert float(ml[1]) == float(hits.double().mean()) and float(ml[2]) == float(hits.all(dim=1).double().mean())
    for name, g in grads.items():
        assert g is not None, name
        e = rel_err(gs.G.grads[name], g)
        assert e < 1e-8, "pretrain grad %s rel err %.3e" % (name, e)
    m, v = O.new_adam_state(gp)
    O.tf_adam_step(gp, grads, m, v, 1)
    for name in gp:
        if not O.is_dead(name):
            assert rel_err(gs.G.arena.views[name], gp[name]) < 1e-9, "generator param after Adam: " + name
        else:
            assert torch.equal(gs.G.arena.views[name], gp[name])
    # D: every parameter, gradient and moment keeps its bits
    for a, b in zip(d_before, _d_state(gs)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert gs.D.adam_t == 0 and gs.G.adam_t == 1
    # a second step carries the Adam state over (moments and step count)
    noise2 = O.synth_noise(B, 1, DT)
    _, _, grads2 = _oracle_mle(gp, images, labels, noise2)
    O.tf_adam_step(gp, grads2, m, v, 2)
    gs.pretrain_step(images, labels, noise2)
    assert gs.G.adam_t == 2
    for name in gp:
        if not O.is_dead(name):
            assert rel_err(gs.G.arena.views[name], gp[name]) < 1e-8, "generator param after 2nd Adam: " + name


def test_pretrain_step_refuses_reuse_and_a_kernel_set_without_the_entry_points():
    gs, _, _ = _fresh()
    images, labels, _ = O.synth_batch(B, 32, V, dtype=DT)
    with pytest.raises(RuntimeError, match="reuse"):
        with gs.iteration(reuse_g_encoder=True):
            gs.pretrain_step(images, labels, O.synth_noise(B, 0, DT))
    bare, _, _ = _fresh(K=RefKernels())
    for call in (lambda: bare.pretrain_step(images, labels, O.synth_noise(B, 0, DT)),
                 lambda: bare.generator_nll(images, labels, O.synth_noise(B, 0, DT)),
                 lambda: bare.generator_step(images, O.synth_noise(B, 0, DT), labels=labels, mle_weight=0.5)):
        with pytest.raises(RuntimeError, match="softmax_xent"):
            call()
    assert bare.G.adam_t == 0
    with pytest.raises(ValueError, match="labels"):
        gs.generator_step(images, O.synth_noise(B, 0, DT), mle_weight=0.5)
    with pytest.raises(ValueError, match="mle_weight"):
        gs.generator_step(images, O.synth_noise(B, 0, DT), labels=labels, mle_weight=-1.0)


def test_generator_step_with_mle_weight_matches_autograd():
    S = 32
    gs, gp, dp_ = _fresh(S)
    images, labels, _ = O.synth_batch(B, S, V, dtype=DT)
    noise = O.synth_noise(B, 1, DT)
    xent, _, grads = _oracle_mle(gp, images, labels, noise, dp_=dp_, w=0.3)
    gs.generator_step(images, noise, labels=labels, mle_weight=0.3)
    assert abs(float(gs.mle_losses[0]) - xent / 3.0) < 1e-9
    for name, g in grads.items():
        e = rel_err(gs.G.grads[name], g)
        assert e < 1e-8, "generator grad %s rel err %.3e" % (name, e)
    # ... and the term matters: the plain step's gradient is far outside the bound
    plain, _, _ = _fresh(S)
    plain.generator_step(images, noise)
    assert rel_err(plain.G.grads["decoder/bias"], grads["decoder/bias"]) > 1e-3
    # mle_weight = 0: none of the new entry points is called, and the weights are those of the call without the new arguments
    zero, _, _ = _fresh(S)
    zero.generator_step(images, noise, labels=labels, mle_weight=0.0)
    assert not [c for c in zero.K.calls + plain.K.calls if c in NEW]
    for a, b in ((zero.G.arena.flat, plain.G.arena.flat), (zero.G.m_flat, plain.G.m_flat), (zero.G.grad_flat, plain.G.grad_flat)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # a whole iteration with the flags at their defaults calls none of them either
    plain.train_iteration(images, labels, [O.synth_noise(B, i, DT) for i in range(3)], [O.synth_alpha(B, i, DT).reshape(B) for i in range(2)],
                          critic_iters=2)
    assert not [c for c in plain.K.calls if c in NEW]


def _pick(t, idx):
    return t[idx].contiguous()


def _accumulated_pretrain(rows, Bm, pick, reducer=None, guard=None, decay=None):
    """Two pretraining updates of `rows` rows, each from len(pick) micro-batches of Bm rows on this process."""
    S, N = 32, len(pick)
    images, labels, _ = O.synth_batch(rows, S, V, dtype=DT)
    gs, _, _ = _fresh(S, Bm, reducer=reducer)
    if guard is not None:
        gs.set_guard((0.0, guard), False)
    if decay is not None:
        gs.G.enable_averaging(decay)
    losses = []
    for step in range(2):
        noise = O.synth_noise(rows, step, DT)
        for k in range(N):
            gs.pretrain_step(_pick(images, pick[k]), _pick(labels, pick[k]), _pick(noise, pick[k]), micro=(k, N) if N > 1 else None)
        losses.append(gs.mle_losses_mean[:3].clone())      # ([3], the valid rows, is a mean over the micro-batches too: rows per micro-batch)
    gs.flush()
    return gs, {"G": gs.G.arena.flat.clone(), "m": gs.G.m_flat.clone(), "loss0": losses[0], "loss1": losses[1]}


_FULL = {}


def full(rows):
    if rows not in _FULL:
        _FULL[rows] = _accumulated_pretrain(rows, rows, [list(range(rows))])[1]
    return _FULL[rows]


def test_accumulated_pretraining_equals_the_large_batch():
    want = full(4)
    gs, got = _accumulated_pretrain(4, 2, [[0, 1], [2, 3]])
    for key in want:
        err = float((got[key] - want[key]).abs().max())
        print("%s: N = 2 x B = 2 vs B = 4 differ by %.3e" % (key, err))
        assert err < 1e-8, (key, err)
    assert gs.G.adam_t == 2 and gs.D.adam_t == 0
    # (another batch is far outside the bound: the comparison can fail)
    other = _accumulated_pretrain(4, 2, [[0, 1], [0, 1]])[1]
    assert float((other["G"] - want["G"]).abs().max()) > 1e3 * 1e-8


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sgg_amd  # noqa: F401
    from sgg_amd import dp
    torch.set_num_threads(2)
    dp.init_from_env(backend="gloo")
    _, res = _accumulated_pretrain(4, 2, [[2 * rank, 2 * rank + 1]], reducer=dp.GradReducer())
    torch.save(res, out % rank)
    torch.distributed.destroy_process_group()


def test_two_ranks_equal_the_single_process(tmp_path):
    out = str(tmp_path / "rank%d.pt")
    port = 37500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    r0, r1 = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(r0["G"], r1["G"]), "replicas diverged"
    want = full(4)
    for key in ("G", "m"):
        err = float((r0[key] - want[key]).abs().max())
        print("%s: world 2 x B 2 vs 4 rows differ by %.3e" % (key, err))
        assert err < 1e-8, (key, err)


def test_guard_and_average_apply_to_the_pretraining_update():
    # the norm of the first update's gradient, from an unguarded twin
    twin, _, _ = _fresh()
    images, labels, _ = O.synth_batch(2, 32, V, dtype=DT)
    twin.pretrain_step(images, labels, O.synth_noise(2, 0, DT))
    norm = float(twin.G.arena.live(twin.G.grad_flat).pow(2).sum().sqrt())
    assert norm > 0
    gs, got = _accumulated_pretrain(2, 2, [[0, 1]], guard=norm / 4.0, decay=0.9)
    rep = gs.guard_reports()
    assert set(rep) == {"G"} and rep["G"]["clipped"] >= 1 and rep["G"]["skipped"] == 0 and rep["G"]["apply"] is True
    first, _, _ = _fresh()
    first.set_guard((0.0, norm / 4.0), False)
    first.pretrain_step(images, labels, O.synth_noise(2, 0, DT))
    r = first.G.guard_report()
    assert r["clipped"] == 1 and abs(r["coef"] - 0.25) < 1e-12 and abs(r["norm"] - norm) < 1e-12 * norm
    # m after the first clipped update is coef x the unclipped one (Adam's parameters barely depend on a gradient scale)
    assert float((first.G.m_flat - 0.25 * twin.G.m_flat).abs().max()) <= 1e-12 * float(twin.G.m_flat.abs().max())
    # the average moved, and differs from the live weights
    avg = gs.G.opt["ema"]
    assert avg["updates"] == 2
    init = _fresh()[0].G.arena.flat
    assert not torch.equal(avg["flat"], init) and not torch.equal(avg["flat"], gs.G.arena.flat)


def test_pretraining_then_gan_iteration_is_the_same_with_and_without_encoder_reuse():
    S = 32
    images, labels, _ = O.synth_batch(B, S, V, dtype=DT)
    res = {}
    for reuse in (False, True):
        gs, _, _ = _fresh(S)
        gs.pretrain_step(images, labels, O.synth_noise(B, 9, DT))
        gs.train_iteration(images, labels, [O.synth_noise(B, i, DT) for i in range(3)], [O.synth_alpha(B, i, DT).reshape(B) for i in range(2)],
                           critic_iters=2, reuse_g_encoder=reuse)
        gs.flush()
        res[reuse] = [t.clone() for net in (gs.G, gs.D) for t in (net.arena.flat, net.m_flat, net.v_flat)]
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


# ---- train.py on the reference kernels -----------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_train(monkeypatch):
    """train.SceneGraphGAN on the CPU: kernels_for hands out one XentRefKernels, the device is "cpu"."""
    sys.path.insert(0, ROOT)
    import train as T
    from sgg_amd import api
    K = XentRefKernels()
    monkeypatch.setattr(T, "kernels_for", lambda device: K)
    monkeypatch.setattr(api, "kernels_for", lambda device: K)
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)

    def make(tmp, name, **kw):
        kw.setdefault("critic_iters", 1)
        return T.SceneGraphGAN(str(tmp / name / "ck"), str(tmp / name / "logs"), None, None, None, None, None, batch_size=2, lambda_=10,
                               synthetic=(2, 32, 11), device="cpu", **kw)
    return T, K, make


def _records(tmp, name):
    with open(str(tmp / name / "logs" / "losses.jsonl")) as f:
        return [json.loads(l) for l in f if l.strip()]


def test_parser_knows_the_flags():
    sys.path.insert(0, ROOT)
    import train as T
    a = T.build_parser().parse_args([])
    assert a.pretrain_iterations == 0 and a.mle_weight == 0.0 and a.validate_nll is False and a.likelihood_out is None
    a = T.parse_args(["--pretrain_iterations", "5", "--mle_weight", "0.1", "--validate_nll", "--likelihood_out", "x.json"])
    assert (a.pretrain_iterations, a.mle_weight, a.validate_nll, a.likelihood_out) == (5, 0.1, True, "x.json")
    for bad in (["--pretrain_iterations", "-1"], ["--mle_weight", "-0.5"], ["--mle_weight", "nan"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_train_pretrain_phase_records_checkpoint_and_resume(cpu_train, tmp_path):
    T, K, make = cpu_train
    # --synthetic 2,32,11 --pretrain_iterations 2 --max_iterations 3 --critic_iters 1, validation at every iteration
    gan = make(tmp_path, "whole", resume=False, pretrain_iterations=2, validate_nll=True)
    gan.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    recs = _records(tmp_path, "whole")
    steps = [r for r in recs if "triples_per_s" in r]
    assert [r.get("phase") for r in steps] == ["pretrain", "pretrain", None] and [r["itr"] for r in steps] == [1, 2, 3]
    for r in steps[:2]:
        assert set(r) == {"itr", "phase", "mle_nll_token", "mle_nll_triple", "mle_token_acc", "mle_triple_acc", "triples_per_s"}
        assert r["mle_nll_triple"] == 3.0 * r["mle_nll_token"] and 0.0 < r["mle_nll_token"] < 2.0 * np.log(11)
    assert set(steps[2]) == {"itr", "disc_loss", "gen_loss", "gp", "triples_per_s"}
    # validation: the likelihood alone in the pretraining phase, beside the critic's cost afterwards
    vals = [r for r in recs if "val_nll_token" in r]
    assert [r["itr"] for r in vals] == [1, 2, 3] and all(set(r) == {"itr", "val_nll_token", "val_token_acc", "val_triple_acc"} for r in vals)
    assert [r["itr"] for r in recs if "val_disc_loss" in r] == [3] and [i for i, _ in gan.val_history] == [2]
    ck = torch.load(gan._ckpt_path())
    assert ck["pretrain_iterations"] == 2 and ck["itr"] == 3 and ck["G_adam"][2] == 3 and ck["D_adam"][2] == 1
    # stopped after one iteration and resumed: the same weights bit for bit
    part = make(tmp_path, "parts", resume=False, pretrain_iterations=2, validate_nll=True)
    part.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    assert torch.load(part._ckpt_path())["itr"] == 1
    rest = make(tmp_path, "parts", resume=True, pretrain_iterations=2, validate_nll=True)
    rest.train(max_iterations=3, log_every=1, validate_every=1, test_at_end=False)
    ck2 = torch.load(rest._ckpt_path())
    for net in ("G", "D"):
        for name, t in ck[net].items():
            assert torch.equal(t, ck2[net][name]), "%s %s differs after the resume" % (net, name)
    assert [r.get("phase") for r in _records(tmp_path, "parts") if "triples_per_s" in r] == ["pretrain", "pretrain", None]


def test_train_defaults_write_the_parents_checkpoint_and_call_nothing_new(cpu_train, tmp_path, capsys):
    T, K, make = cpu_train
    gan = make(tmp_path, "plain", resume=False)
    gan.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    assert set(torch.load(gan._ckpt_path())) == {"itr", "G", "D", "G_adam", "D_adam", "val"}
    assert not [c for c in K.calls if c in NEW]
    recs = _records(tmp_path, "plain")
    assert set(recs[0]) == {"itr", "disc_loss", "gen_loss", "gp", "triples_per_s"} and set(recs[1]) == {"itr", "val_disc_loss"}
    # --validate_nll leaves val_disc_loss its bits; --mle_weight adds the four numbers to the record
    vn = make(tmp_path, "vnll", resume=False, validate_nll=True)
    vn.train(max_iterations=1, log_every=1, validate_every=1, test_at_end=False)
    vr = _records(tmp_path, "vnll")
    assert [set(r) for r in vr] == [set(recs[0]), {"itr", "val_nll_token", "val_token_acc", "val_triple_acc"}, {"itr", "val_disc_loss"}]
    assert vr[2]["val_disc_loss"] == recs[1]["val_disc_loss"] and vr[0]["disc_loss"] == recs[0]["disc_loss"]
    flagged = make(tmp_path, "flagged", resume=False, mle_weight=0.1)
    flagged.train(max_iterations=1, log_every=1, validate_every=0, test_at_end=False)
    fr = _records(tmp_path, "flagged")
    assert set(fr[0]) == set(recs[0]) | {"mle_nll_token", "mle_nll_triple", "mle_token_acc", "mle_triple_acc"}
    assert fr[0]["disc_loss"] == recs[0]["disc_loss"], "the critic update in front of the generator's does not see the term"
    assert set(torch.load(flagged._ckpt_path())) == {"itr", "G", "D", "G_adam", "D_adam", "val"}
    # resuming with another P says so, once
    capsys.readouterr()
    again = make(tmp_path, "plain", resume=True, pretrain_iterations=4)
    again.train(max_iterations=2, log_every=1, validate_every=0, test_at_end=False)
    assert capsys.readouterr().out.count("resuming with --pretrain_iterations 4 a run saved with 0") == 1
    assert [r.get("phase") for r in _records(tmp_path, "plain") if "triples_per_s" in r] == [None, "pretrain"]


def test_train_diagnostics_across_the_phase_boundary(cpu_train, tmp_path):
    """--diagnostics_every 1 --halt_on_nonfinite --accumulate 2 with one pretraining iteration, then one GAN iteration: the
    pretraining record describes G alone (no critic rows, no slopes, no gp_slope_rows), the first GAN record is the two-network
    report it always was, and the non-finite check reads both kinds of record."""
    T, K, make = cpu_train
    gan = make(tmp_path, "diag", resume=False, pretrain_iterations=1, accumulate=2)
    gan.train(max_iterations=2, log_every=1, validate_every=0, test_at_end=False, diagnostics_every=1, halt_on_nonfinite=True)
    recs = _records(tmp_path, "diag")
    assert [r.get("phase") for r in recs] == ["pretrain", None] and all(r["accumulate"] == 2 for r in recs)
    pre, gd = recs[0]["diag"], recs[1]["diag"]
    assert set(pre) == {"G"} and pre["G"]["first_nonfinite"] is None and pre["G"]["grad_norm"] > 0 and pre["G"]["update_norm"] > 0
    assert set(gd) == {"G", "D", "gp_slope", "gp_slope_rows"} and gd["gp_slope_rows"] == 2 and gd["D"]["grad_norm"] > 0
    assert gd["G"]["grad_norm"] != pre["G"]["grad_norm"], "the GAN record still shows the pretraining step's rows"
    with open(str(tmp_path / "diag" / "logs" / "diagnostics.jsonl")) as f:
        tables = [json.loads(l) for l in f if l.strip()]
    assert [set(t["tensors"]) for t in tables] == [{"G"}, {"G", "D"}] and [t["itr"] for t in tables] == [1, 2]
    assert gan.step.G.adam_t == 2 and gan.step.D.adam_t == 1
    # the check on a record without the critic: passes when clean, names G's tensor when not
    dg.raise_if_nonfinite({"G": {"first_nonfinite": None}}, 1)
    with pytest.raises(dg.NonFiniteError, match="decoder/bias"):
        dg.raise_if_nonfinite({"G": {"first_nonfinite": {"tensor": "decoder/bias", "which": ["g"]}}}, 1)
    # a NaN in the pretraining gradient stops the run there, before the checkpoint is written
    bad = make(tmp_path, "bad", resume=False, pretrain_iterations=1)
    step = T.GanStep.pretrain_step

    def poisoned(self, images, labels, noise, micro=None):
        images = images.clone()
        images[0, 0, 0, 0] = float("nan")
        return step(self, images, labels, noise, micro)
    try:
        T.GanStep.pretrain_step = poisoned
        with pytest.raises(dg.NonFiniteError):
            bad.train(max_iterations=2, log_every=1, validate_every=0, test_at_end=False, diagnostics_every=1, halt_on_nonfinite=True)
    finally:
        T.GanStep.pretrain_step = step
    assert not os.path.exists(bad._ckpt_path())


def test_likelihood_matches_the_restatement(cpu_train, tmp_path):
    T, K, make = cpu_train
    gan = make(tmp_path, "lik", resume=False)
    g = torch.Generator().manual_seed(5)
    items = [(torch.randn((32, 32, 3), generator=g), [[1, 2, 3], [4, 5, 6], [1, 2, 3]]),
             (torch.randn((32, 32, 3), generator=g), [[0, 10, 0]]),
             (torch.randn((32, 32, 3), generator=g), [[7, 7, 7], [3, 11, 2], [2, 0, 9], [8, 1, 1]])]       # (11: outside the vocabulary)
    out = str(tmp_path / "nll.json")
    res = gan.likelihood(items=items, n_samples=3, out_path=out)
    assert json.load(open(out)) == res
    assert set(res) == {"nll_mixture", "nll_single", "nll_slot", "perplexity_token", "n_images", "n_triples", "n_out_of_vocab", "n_samples",
                        "generator_weights"}
    assert (res["n_images"], res["n_triples"], res["n_out_of_vocab"], res["n_samples"], res["generator_weights"]) == (3, 7, 1, 3, "live")
    assert K.calls.count("triple_logp") >= 1 and "softmax_xent" in K.calls
    # the restatement on the logits of the same passes (one image per pass at TEST_BATCH_SIZE = 1; same noise stream)
    mix, mean, slot = [], [], []
    with __import__("contextlib").closing(gan._sample_batches([(str(i), im) for i, (im, _) in enumerate(items)], 3, 1)) as batches:
        for i0, n, images, logits in batches:
            x = logits.numpy().astype(np.float64)
            real = np.asarray(items[i0][1], dtype=np.int64)[None]
            r = XR.triple_logp(x, XR.lse64(x), real, [real.shape[1]])
            ok = r["status"][0] == 0
            mix.append(-r["mix"][0][ok]); mean.append(-r["mean"][0][ok]); slot.append(-r["slot"][0][ok])
    tol = 1e-5          # (fp32 networks on the CPU against fp64 sums of their logits: a handful of fp32 roundings of |lp| <= 30)
    assert abs(res["nll_mixture"]["micro"] - np.concatenate(mix).mean()) < tol
    assert abs(res["nll_mixture"]["macro"] - np.mean([m.mean() for m in mix])) < tol
    assert abs(res["nll_single"]["micro"] - np.concatenate(mean).mean()) < tol
    assert abs(res["nll_single"]["macro"] - np.mean([m.mean() for m in mean])) < tol
    assert np.abs(np.array(res["nll_slot"]) - np.concatenate(slot).mean(axis=0)).max() < tol
    assert abs(res["perplexity_token"] - np.exp(res["nll_single"]["micro"] / 3.0)) < 1e-12
    assert res["nll_single"]["micro"] >= res["nll_mixture"]["micro"] and abs(sum(res["nll_slot"]) - res["nll_single"]["micro"]) < tol
    # Generator.log_prob: the same numbers for one image
    im = items[0][0][None]
    gt = torch.tensor([items[0][1]], dtype=torch.int64)
    ng = torch.Generator().manual_seed(gan.seed + 123)
    noise = torch.stack([torch.randn((1, 512), generator=ng) for _ in range(3)])        # (the draws of _sample_batches for image 0)
    m2, _, _, st = gan.g.log_prob(im, gt, torch.tensor([3], dtype=torch.int32), 3, noise)
    assert st.tolist() == [[0, 0, 0]] and np.abs(-m2.numpy()[0].astype(np.float64) - mix[0]).max() < tol
