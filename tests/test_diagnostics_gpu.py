"""-m gpu: training diagnostics - the statistics pass (csrc/stats.hip, HipKernels.arena_stats / vector_stats) against the fp64
restatement sgg_amd.diagnostics.stats_reference, its reproducibility, Network / GanStep with the pass armed (same rows by name; the
training state bit-equal to a run that was never armed) and train.py --diagnostics_every.

Tolerances (bounds, not measurements).  Counts and the maxima of g and p: equal (the same fp32 values on both sides).  Sums of squares
of g and p: relative 1e-10 - both sides are fp64 sums of exact squares, the orders differ, at most n * 2^-53 < 1e-11 for n < 1e5.
u = lr_t * m / (sqrt(v) + eps) is a few fp32 roundings per element whose placement -ffp-contract=fast may change: maxima relative
2e-6, sums of squares 1e-5 (about ten times the bound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd import diagnostics as dg
from sgg_amd.params import ADAM_EPS
from sgg_amd.step import GanStep, tf_adam_lr_t

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, SENTINEL = 64, -777.0
B, S, V = 8, 64, 50


def assert_rows(got, want, names=None):
    """got / want [T, 9] under the tolerances of the module docstring; prints the largest deviations first."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    rel = lambda c: float(np.max(np.abs(got[:, c] - want[:, c]) / np.maximum(np.abs(want[:, c]), 1e-300)))
    print("rel: g_ss %.3g p_ss %.3g u_ss %.3g u_max %.3g" % (rel(0), rel(3), rel(6), rel(7)))
    for c, name in enumerate(dg.STAT_NAMES):
        tol = {0: 1e-10, 3: 1e-10, 6: 1e-5, 7: 2e-6}.get(c, 0.0)
        bad = np.flatnonzero(~(np.abs(got[:, c] - want[:, c]) <= tol * np.abs(want[:, c])))
        assert bad.size == 0, "%s differs in tensors %s: got %r, want %r" % (
            name, [names[i] if names else int(i) for i in bad[:4]], got[bad[:4], c].tolist(), want[bad[:4], c].tolist())


# ---- kernel against the reference on crafted arenas ---------------------------------------------------------------------------
_CRAFTED = {}


def crafted():
    """Tensors of 1 .. 3 * chunk + 7 elements laid out like ParamArena (each rounded up to 4); NaN / 1e30 in every padding slot;
    +-Inf, NaN and -0.0 at the first and last positions of tensors and of chunks; tensor 8 (255 elements) has v == 0 everywhere;
    no fp32 subnormal anywhere.  Built once: (host arrays p g m v, offsets, numels, chunk table, reference rows by grad_scale)."""
    if _CRAFTED:
        return _CRAFTED
    C = dg.CHUNK
    numels = [1, 2, 3, 4, 5, 63, 64, 65, 255, 257, C - 1, C, C + 1, 3 * C + 7]
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += (n + 3) // 4 * 4
    total = off
    r = np.random.RandomState(20)
    sign = lambda: np.where(r.rand(total) < 0.5, -1.0, 1.0)
    p = (sign() * r.uniform(1e-3, 1.0, total)).astype(np.float32)
    g = (sign() * r.uniform(1e-4, 8.0, total)).astype(np.float32)
    m = (sign() * r.uniform(1e-6, 1e-2, total)).astype(np.float32)
    v = r.uniform(1e-10, 1e-3, total).astype(np.float32)
    v[offsets[8]:offsets[8] + numels[8]] = 0.0
    specials = [np.inf, -np.inf, np.nan, -0.0]
    arenas = [p, g, m, v]
    k = 0
    for t, (o, n) in enumerate(zip(offsets, numels)):
        edges = sorted({0, n - 1} | {e for c in range(C, n, C) for e in (c - 1, c)})
        for e in edges:
            arenas[(k + t) % 4][o + e] = specials[k % 4]
            k += 1
            if n >= 64:                                                # a second arena at the same element, another special
                arenas[(k + t + 1) % 4][o + e] = specials[(k + 2) % 4]
        pad = slice(o + n, o + (n + 3) // 4 * 4)
        g[pad], v[pad] = np.nan, np.nan
        p[pad], m[pad] = 1e30, 1e30
    for a in arenas:
        fin = np.isfinite(a) & (a != 0)
        assert (np.abs(a[fin]) >= 1.2e-38).all(), "an input is subnormal"
    table = dg.chunk_table(offsets, numels, C)
    dg.check_table(table, len(numels), total, C)
    lr_t = tf_adam_lr_t(3)
    want = {gs: dg.stats_reference(p, g, m, v, offsets, numels, lr_t, ADAM_EPS, gs) for gs in (1.0, 0.125)}
    # input conditions, from the reference alone: specials are counted in every arena's statistics somewhere, most rows keep finite
    # content, the v == 0 tensor has a finite update, and no padding value (1e30, NaN) shows
    w = want[1.0]
    assert (w[:, 2] > 0).any() and (w[:, 5] > 0).any() and (w[:, 8] > 0).any()
    assert (w[5:, 0] > 0).all() and (w[5:, 3] > 0).all() and (w[5:, 6] > 0).all()
    assert w[8, 6] > 0 and w[8, 7] > 1.0, "v == 0: u = lr_t * m / eps"
    assert w[:, (1, 4)].max() <= 8.0 and (w[:, (2, 5, 8)].sum(axis=1) <= np.asarray(numels)).all()
    assert w[0, (2, 5, 8)].sum() >= 1 and w[13, (2, 5, 8)].sum() >= 8
    _CRAFTED.update(dict(arr=(p, g, m, v), offsets=offsets, numels=numels, table=table, want=want, lr_t=lr_t, total=total))
    return _CRAFTED


def guarded(n, dtype):
    big = torch.full((PAD + n + PAD,), SENTINEL, dtype=dtype, device="cuda")
    return big, big[PAD:PAD + n]


def untouched(big, n):
    flat = big.cpu().numpy()
    return bool((flat[:PAD] == SENTINEL).all() and (flat[PAD + n:] == SENTINEL).all())


@pytest.mark.parametrize("grad_scale", [1.0, 0.125], ids=["scale1", "scale1_8"])
def test_arena_stats_equals_reference(hip, grad_scale):
    c = crafted()
    assert hip.arena_stats_chunk() == dg.CHUNK and hip.arena_stats_nstat() == dg.NSTAT
    dev = [torch.from_numpy(a).cuda() for a in c["arr"]]
    table = torch.from_numpy(c["table"]).cuda()
    T, n_ws = len(c["numels"]), hip.arena_stats_workspace_bytes(len(c["table"])) // 8
    big_out, out = guarded(T * dg.NSTAT, torch.float64)
    big_ws, ws = guarded(n_ws, torch.float64)
    got = hip.arena_stats(*dev, table, T, c["lr_t"], ADAM_EPS, grad_scale, out=out.view(T, dg.NSTAT), ws=ws.view(torch.uint8))
    torch.cuda.synchronize()
    assert untouched(big_out, T * dg.NSTAT) and untouched(big_ws, n_ws), "written outside the output or the workspace"
    assert all(np.array_equal(d.cpu().numpy().view(np.uint32), a.view(np.uint32)) for d, a in zip(dev, c["arr"])), "an input changed"
    assert_rows(got.cpu().numpy(), c["want"][grad_scale])
    # outputs and workspace allocated by the binding
    again = hip.arena_stats(*dev, table, T, c["lr_t"], ADAM_EPS, grad_scale)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), got.cpu().numpy().view(np.uint64))


def test_arena_stats_is_reproducible_and_grid_independent(hip):
    c = crafted()
    dev = [torch.from_numpy(a).cuda() for a in c["arr"]]
    table = torch.from_numpy(c["table"]).cuda()
    T = len(c["numels"])
    run = lambda grid: hip.arena_stats(*dev, table, T, c["lr_t"], ADAM_EPS, 0.125, grid=grid).cpu().numpy().view(np.uint64)
    first = run(0)
    assert np.isfinite(first.view(np.float64)).all()
    for grid in (0, 1, 3, 64, len(c["table"]) + 5, 5000):
        assert np.array_equal(run(grid), first), "grid %d changes the bits" % grid


def test_arena_stats_rejects_bad_arguments(hip):
    from sgg_amd.lib import SggError
    c = crafted()
    dev = [torch.from_numpy(a).cuda() for a in c["arr"]]
    table = torch.from_numpy(c["table"]).cuda()
    T = len(c["numels"])
    with pytest.raises(SggError, match="workspace"):
        hip.arena_stats(*dev, table, T, 1e-4, 1e-8, ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(SggError, match="n_tensors"):
        hip.arena_stats(*dev, table, len(c["table"]) + 1, 1e-4, 1e-8)
    with pytest.raises(SggError, match="grid"):
        hip.arena_stats(*dev, table, T, 1e-4, 1e-8, grid=70000)
    with pytest.raises(SggError, match="aligned"):
        hip.arena_stats(*[torch.cat([d, d[:4]])[1:-3] for d in dev], table, T, 1e-4, 1e-8)
    x = torch.zeros(4, device="cuda")
    assert hip.lib.sgg_vector_stats(x.data_ptr(), 0, 1.0, x.data_ptr(), None) == -1
    assert hip.lib.sgg_vector_stats(None, 4, 1.0, x.data_ptr(), None) == -1 and b"null" in hip.lib.sgg_last_error()
    torch.cuda.synchronize()


# ---- vector_stats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [(1, "plain"), (8, "at_threshold"), (63, "nan"), (64, "plain"), (65, "at_threshold"), (300, "nan")],
                         ids=lambda x: str(x))
def test_vector_stats_equals_reference(hip, n, kind):
    r = np.random.RandomState(n)
    x = r.uniform(0.25, 2.0, n).astype(np.float32)
    if kind == "at_threshold":
        x[n // 2], x[-1] = 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))        # AT the threshold: not above; one ulp over: above
    if kind == "nan":
        x[0], x[n // 2], x[-1] = np.nan, np.inf, -np.inf
    want = dg.vector_stats_reference(x, 1.0)
    if kind == "at_threshold":
        assert want[3] == float((x > 1.0).sum()) and (x == 1.0).sum() == 1
    if kind == "nan":
        assert want[4] == 3 and np.isfinite(want[:3]).all()
    big, out = guarded(5, torch.float64)
    got = hip.vector_stats(torch.from_numpy(x).cuda(), 1.0, out=out).cpu().numpy()
    assert untouched(big, 5)
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3] and got[4] == want[4], (got, want)
    # fp64 sums of the same fp32 values in two orders: each within (n - 1) * 2^-53 * sum |x| of the exact sum
    assert abs(got[2] - want[2]) <= 2 * n * 2.0 ** -53 * float(np.abs(x[np.isfinite(x)]).sum()), (got[2], want[2])
    assert np.array_equal(hip.vector_stats(torch.from_numpy(x).cuda(), 1.0).cpu().numpy().view(np.uint64), got.view(np.uint64))


def test_vector_stats_without_a_finite_element(hip):
    got = hip.vector_stats(torch.tensor([float("nan"), float("inf")], device="cuda"), 1.0).cpu().numpy()
    assert got.tolist() == [np.inf, -np.inf, 0.0, 0.0, 2.0]


# ---- Network / GanStep ------------------------------------------------------------------------------------------------------------
def _new_step(hip, **kw):
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    dp["W"] = dp["W"] * 25.0
    return GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp, **kw)


def _reference_rows(net, lr_t, grad_scale=1.0):
    names, offsets, numels = dg.live_layout(net.arena)
    host = [t.cpu().numpy() for t in (net.arena.flat, net.grad_flat, net.m_flat, net.v_flat)]
    return names, dg.stats_reference(*host, offsets, numels, lr_t, ADAM_EPS, grad_scale)


def test_network_rows_match_reference_and_name_the_nan(hip):
    images, labels, _ = O.synth_batch(B, S, V)
    img, lab = images.cuda(), labels.cuda()
    gs = _new_step(hip)
    gs.arm_diagnostics(True)
    gs.critic_step(img, lab, O.synth_noise(B, 0).cuda(), O.synth_alpha(B, 0).reshape(B).cuda())
    gs.generator_step(img, O.synth_noise(B, 1).cuda())
    diag = gs.diagnostics()
    torch.cuda.synchronize()
    for key, net in (("G", gs.G), ("D", gs.D)):
        names, want = _reference_rows(net, tf_adam_lr_t(1))
        assert list(diag["tensors"][key]) == names and net.adam_t == 1
        got = np.asarray([[diag["tensors"][key][n][s] for s in dg.STAT_NAMES] for n in names])
        assert (want[:, 0] > 0).sum() > len(names) // 2 and (want[:, 6] > 0).sum() > len(names) // 2, "the step left no gradients"
        assert_rows(got, want, names)
        s = diag[key]
        assert s["nonfinite"] == {"g": 0, "p": 0, "u": 0} and s["first_nonfinite"] is None
        assert abs(s["grad_norm"] - np.sqrt(want[:, 0].sum())) <= 1e-9 * s["grad_norm"] and s["update_ratio"] > 0
    sl = gs.slopes.cpu().numpy().astype(np.float64)
    assert diag["gp_slope"]["nonfinite"] == 0 and diag["gp_slope"]["min"] == sl.min() and diag["gp_slope"]["max"] == sl.max()
    assert abs(diag["gp_slope"]["mean"] - sl.mean()) <= 1e-12 * abs(sl.mean()) and diag["gp_slope"]["share_above_1"] == (sl > 1).mean()
    # one NaN written into a gradient buffer, the pass run again on the arenas as they are
    for key, net in (("G", gs.G), ("D", gs.D)):
        net.grads["decoder/bias"].view(-1)[0] = float("nan")
        net.arena_stats()
    again = gs.diagnostics()
    for key in ("G", "D"):
        counts = {n: r["g_nonfinite"] + r["p_nonfinite"] + r["u_nonfinite"] for n, r in again["tensors"][key].items()}
        assert counts.pop("decoder/bias") == 1 and not any(counts.values()), key
        assert again[key]["first_nonfinite"] == {"tensor": "decoder/bias", "which": ["g"]} and again[key]["nonfinite"] == {"g": 1, "p": 0, "u": 0}
    with pytest.raises(dg.NonFiniteError, match="gradient in G tensor 'decoder/bias'"):
        dg.raise_if_nonfinite(again)


def _train_state(hip, armed, overlap):
    images, labels, _ = O.synth_batch(B, S, V)
    img, lab = images.cuda(), labels.cuda()
    gs = _new_step(hip, overlap_streams=overlap)
    if armed:
        gs.arm_diagnostics(True)
    for it in range(2):
        noises = [O.synth_noise(B, 10 * it + i).cuda() for i in range(3)]
        alphas = [O.synth_alpha(B, 10 * it + i).reshape(B).cuda() for i in range(2)]
        gs.train_iteration(img, lab, noises, alphas, critic_iters=2)
    gs.flush()
    torch.cuda.synchronize()
    out = {"losses": torch.cat([gs.d_losses, gs.g_losses]).clone()}
    for key, net in (("G", gs.G), ("D", gs.D)):
        out.update({key + ".params": net.arena.flat.clone(), key + ".m": net.m_flat.clone(), key + ".v": net.v_flat.clone()})
        st = net.opt.get("diag")
        assert (st is not None and st["last"] == (tf_adam_lr_t(net.adam_t), 1.0)) if armed else (st is None and not net.opt.get("armed"))
        assert net.adam_t == (2 if key == "G" else 4)
    return out


@pytest.mark.parametrize("overlap", [True, False], ids=["two_streams", "serial"])
def test_armed_run_is_bitwise_the_unarmed_run(hip, overlap):
    ref = _train_state(hip, False, overlap)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    got = _train_state(hip, True, overlap)
    bad = [k for k in ref if not torch.equal(ref[k].view(torch.int32), got[k].view(torch.int32))]
    assert not bad, "armed diagnostics changed %s" % bad


def test_diagnostics_before_any_armed_step_is_an_error(hip):
    gs = _new_step(hip)
    with pytest.raises(RuntimeError, match="arm_diagnostics"):
        gs.diagnostics()


# ---- train.py ---------------------------------------------------------------------------------------------------------------------
def test_train_cli_writes_diagnostics(tmp_path):
    logs = tmp_path / "logs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "2",
                        "--max_iterations", "2", "--diagnostics_every", "1", "--halt_on_nonfinite", "--checkpoints_dir", str(tmp_path / "ck"),
                        "--summaries_dir", str(logs)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in open(str(logs / "losses.jsonl"))]
    diags = [x for x in recs if "diag" in x]
    assert [x["itr"] for x in diags] == [1, 2]
    from sgg_amd.params import ParamArena
    for x in diags:
        d = x["diag"]
        assert set(d) == {"G", "D", "gp_slope"}
        for key in ("G", "D"):
            assert d[key]["nonfinite"] == {"g": 0, "p": 0, "u": 0} and d[key]["first_nonfinite"] is None
            assert d[key]["grad_norm"] > 0 and d[key]["param_norm"] > 0 and d[key]["update_norm"] > 0
        assert d["gp_slope"]["nonfinite"] == 0 and 0 <= d["gp_slope"]["min"] <= d["gp_slope"]["mean"] <= d["gp_slope"]["max"]
        assert 0.0 <= d["gp_slope"]["share_above_1"] <= 1.0
    rows = [json.loads(l) for l in open(str(logs / "diagnostics.jsonl"))]
    assert [x["itr"] for x in rows] == [1, 2]
    for x in rows:
        for key in ("G", "D"):
            names = dg.live_layout(ParamArena(key, 50, 64, device="meta"))[0]
            assert list(x["tensors"][key]) == names
            assert all(t[s] == 0 for t in x["tensors"][key].values() for s in ("g_nonfinite", "p_nonfinite", "u_nonfinite"))
    assert os.path.exists(str(tmp_path / "ck" / "model.ckpt.pt"))
