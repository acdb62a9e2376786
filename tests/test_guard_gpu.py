"""-m gpu: guarded updates on the device - the reduction and the record (csrc/guard.hip) against sgg_amd.guard, the guarded Adam
kernels against the unguarded entry points bit for bit, step.Network / GanStep with a guard on the two-stream schedule, with
accumulation and with weight averaging, and train.py --clip_grad_norm / --skip_nonfinite.

Tolerances.  The non-finite count: exact.  The sum of squares: all summands are non-negative fp64 numbers (squares of fp32 values are
exact in fp64), so ANY summation order, contracted or not, lies within n * 2^-52 * ss of the exact sum; the device and NumPy each do,
and the test holds their difference to n * 2^-52 * ss.  Fields [2..5]: bit-equal to guard.decide on the device's own [0..1] (fp64
sqrt and division are correctly rounded).  Two device sums of the same elements in different orders (the guard's chunks against
arena_stats' per-tensor rows, summed over the tensors): three times that bound.  Guarded Adam against the unguarded entry point fed
(float)record[4], a dropped update, two schedules of the same kernels: bit-equal.  m against the CPU fp64 step: GRAD_RTOL *
max|ref| per tensor (tests/tolerances.py) - after the first update m is the gradient times the constant (1 - beta1) * s_eff."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd import ema as E
from sgg_amd import guard as G
from sgg_amd.lib import SggError
from sgg_amd.params import ADAM_B1, ADAM_B2, ADAM_EPS
from sgg_amd.step import GanStep, tf_adam_lr_t
from tests.test_guard_cpu import GuardRefKernels
from tests.tolerances import GRAD_RTOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAD, SENTINEL = 64, -777.0
C = 16384                                                # sgg_arena_stats_chunk() (checked against the library below)
RED_SIZES = [1, 2, 3, 4, 5, 7, 1027, C - 1, C, C + 1, 3 * C + 5, 300 * C + 3]     # the last: more chunk rows than the final workgroup has threads
# the launcher of the Adam kernels (grid_for): blocks of 256 threads, 4 floats per thread and trip, at most 4096 blocks
ONE_PASS = 4096 * 256 * 4
ADAM_SIZES = [1, 3, 4, 5, 1027, ONE_PASS + 3]
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001,
                     0x7f7fffff, 0xff7fffff, 0x00800000], dtype=np.uint32)      # +-0, subnormals, +-Inf, NaNs, +-max, min normal
U52 = 2.0 ** -52


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def guarded(host, dtype=torch.float32):
    """A device copy of `host` between two sentinel guards: (whole buffer, the view the kernel gets)."""
    n = host.size
    big = torch.full((PAD + n + PAD,), SENTINEL, dtype=dtype, device="cuda")
    big[PAD:PAD + n].copy_(torch.from_numpy(host))
    return big, big[PAD:PAD + n]


def untouched(big, n):
    return bool((big[:PAD] == SENTINEL).all() and (big[PAD + n:] == SENTINEL).all())


def same_floats(got, want):
    """Bit-equal, NaNs compared by position."""
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn]))


def test_chunk_is_the_one_of_the_statistics_pass(hip):
    assert hip.arena_stats_chunk() == C
    for n in (1, C, C + 1, 300 * C + 3):
        assert hip.grad_guard_workspace_bytes(n) == -(-n // C) * 2 * 8
    assert hip.grad_guard_workspace_bytes(0) == 0


# ---- the reduction ----------------------------------------------------------------------------------------------------------------
def reduction_input(n, special):
    r = np.random.RandomState(23 + n % 9973)
    g = (r.uniform(-4.0, 4.0, n) * 10.0 ** r.randint(-6, 4, n)).astype(np.float32).view(np.uint32).copy()
    if special:
        m = len(SPECIALS)
        for j, i in enumerate(sorted(set(range(min(n, m))) | set(range(max(0, n - m), n)))):
            g[i] = SPECIALS[j % m]
    return g.view(np.float32)


def host_sums(g, grad_scale):
    with np.errstate(over="ignore", invalid="ignore"):
        x = g * np.float32(grad_scale)
    assert x.dtype == np.float32
    fin = np.isfinite(x)
    x64 = x[fin].astype(np.float64)
    return float(np.sum(x64 * x64)), float(x.size - int(fin.sum()))


@pytest.mark.parametrize("special", [False, True], ids=["seeded", "specials"])
@pytest.mark.parametrize("n", RED_SIZES)
def test_reduction_and_record(hip, n, special):
    g = reduction_input(n, special)
    if special and n >= 1027:
        assert np.isnan(g).any() and np.isinf(g).any() and (np.abs(g[g != 0]) < 1.2e-38).any(), "the special values are missing"
    big_g, dg = guarded(g)
    rows = -(-n // C)
    big_ws, ws = guarded(np.zeros(rows * 2, dtype=np.float64), torch.float64)
    big_rec, rec = guarded(np.zeros(8, dtype=np.float64), torch.float64)
    clipped = skipped = 0
    # (grad_scale, max_norm, skip_nonfinite, grid); the first three settings are one decision for three grids
    calls = [(0.37, 1.0, True, 0), (0.37, 1.0, True, 1), (0.37, 1.0, True, 3), (0.37, 1.0, True, 0),
             (1.0, 0.0, False, 0), (0.5, 1e30, True, 0), (2.0, 1e-3, False, 3)]
    first = None
    for k, (gs, mx, skip, grid) in enumerate(calls):
        hip.grad_guard(dg, rec, gs, mx, skip, ws=ws, grid=grid)
        torch.cuda.synchronize()
        what = "n %d call %d (grad_scale %g max_norm %g skip %s grid %d)" % (n, k, gs, mx, skip, grid)
        assert untouched(big_g, n) and untouched(big_ws, rows * 2) and untouched(big_rec, 8), "written outside a buffer: " + what
        assert np.array_equal(bits(dg), g.view(np.int32)), "g changed: " + what
        got = rec.cpu().numpy()
        ss, bad = host_sums(g, gs)
        print("%s: ss %.17g (host %.17g, diff %.3e, bound %.3e), non-finite %d" % (what, got[0], ss, abs(got[0] - ss), n * U52 * ss, got[1]))
        assert got[1] == bad, "non-finite count %r, host %r: %s" % (got[1], bad, what)
        assert abs(got[0] - ss) <= n * U52 * ss, "ss %.17g, host %.17g: %s" % (got[0], ss, what)
        want = G.decide(got[0], got[1], gs, mx, skip)
        assert got[2:6].tolist() == list(want), "[2..5] = %r, guard.decide gives %r: %s" % (got[2:6].tolist(), want, what)
        clipped += int(want[1] < 1.0 and want[3] != 0.0)
        skipped += int(want[3] == 0.0)
        assert (got[6], got[7]) == (clipped, skipped), "counters %r, want %r: %s" % (got[6:].tolist(), (clipped, skipped), what)
        if k == 0:
            first = got.copy()
        elif k < 4:
            assert np.array_equal(got[:6].view(np.int64), first[:6].view(np.int64)), "the record depends on the grid or the call: " + what
    if n > 8:
        assert clipped > 0, "no call clipped"
        assert (skipped > 0) == special, "the skip did not follow the special values"
    # the whole record against the restatement, counters through prev
    ref = None
    for gs, mx, skip, _ in calls:
        ref = G.reference_record(g, gs, mx, skip, prev=ref)
    assert ref[1] == got[1] and (ref[6], ref[7]) == (clipped, skipped) and ref[5] == got[5]
    assert abs(ref[2] - got[2]) <= n * U52 * ref[2] and abs(ref[3] - got[3]) <= n * U52 * ref[3] + 2 * U52


def test_reduction_rejects_bad_arguments_without_a_launch(hip):
    n = 2 * C + 8
    base = torch.arange(n + 8, dtype=torch.float32, device="cuda")
    rec = torch.full((10,), 5.0, dtype=torch.float64, device="cuda")
    ws = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    keep = (base.clone(), rec.clone(), ws.clone())
    r8 = rec[:8]
    with pytest.raises(SggError, match="aligned"):
        hip.grad_guard(base[1:1 + n], r8, ws=ws)                    # grads offset by 4 bytes
    for mx in (-1.0, float("nan"), float("inf")):
        with pytest.raises(SggError, match="max_norm"):
            hip.grad_guard(base[:n], r8, 1.0, mx, ws=ws)
    for gs in (float("nan"), float("inf")):
        with pytest.raises(SggError, match="grad_scale"):
            hip.grad_guard(base[:n], r8, gs, 1.0, ws=ws)
    with pytest.raises(SggError, match="grid"):
        hip.grad_guard(base[:n], r8, ws=ws, grid=-1)
    with pytest.raises(SggError, match="workspace"):
        hip.grad_guard(base[:n], r8, ws=ws[:5])                     # three chunks need 48 bytes
    lib = hip.lib
    gp, rp, wp = base.data_ptr(), rec.data_ptr(), ws.data_ptr()
    assert lib.sgg_grad_guard(gp, n, 1.0, 1.0, 1, 0, wp, 128, rp + 4, None) == -1 and b"aligned" in lib.sgg_last_error()
    assert lib.sgg_grad_guard(gp, n, 1.0, 1.0, 1, 0, wp + 4, 124, rp, None) == -1 and b"aligned" in lib.sgg_last_error()
    assert lib.sgg_grad_guard(gp, 0, 1.0, 1.0, 1, 0, wp, 128, rp, None) == -1 and b"sgg_grad_guard" in lib.sgg_last_error()
    assert lib.sgg_grad_guard(gp, -4, 1.0, 1.0, 1, 0, wp, 128, rp, None) == -1
    assert lib.sgg_grad_guard(gp, n, 1.0, 1.0, 1, 0, wp, 40, rp, None) == -3
    for ptrs in ((None, wp, rp), (gp, None, rp), (gp, wp, None)):
        assert lib.sgg_grad_guard(ptrs[0], n, 1.0, 1.0, 1, 0, ptrs[1], 128, ptrs[2], None) == -1
    # the guarded Adam entry points: misaligned operands, a misaligned or missing record, n = 0
    mk = lambda: torch.full((64,), 0.5, device="cuda")
    off = lambda: torch.full((68,), 0.5, device="cuda")[1:65]
    good = torch.zeros(8, dtype=torch.float64, device="cuda")
    for k in range(5):
        ops = [mk() for _ in range(5)]
        ops[k] = off()
        with pytest.raises(SggError, match="aligned"):
            hip.adam_ema_guarded(*ops, 1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, good, 0.5)
        if k < 4:
            with pytest.raises(SggError, match="aligned"):
                hip.adam_guarded(*ops[:4], 1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, good)
    p, g_, m, v, e = (mk() for _ in range(5))
    with pytest.raises(SggError, match="overlap"):
        hip.adam_ema_guarded(p, g_, m, v, p, 1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, good, 0.5)
    with pytest.raises(SggError, match="one_minus_decay"):
        hip.adam_ema_guarded(p, g_, m, v, e, 1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, good, 1.5)
    a = [t.data_ptr() for t in (p, g_, m, v, e)]
    assert lib.sgg_adam_tf_multi_guarded(*a[:4], 64, 1e-4, 0.5, 0.9, 1e-8, good.data_ptr() + 4, None) == -1
    assert lib.sgg_adam_tf_multi_guarded(*a[:4], 64, 1e-4, 0.5, 0.9, 1e-8, None, None) == -1
    assert lib.sgg_adam_tf_multi_guarded(*a[:4], 0, 1e-4, 0.5, 0.9, 1e-8, good.data_ptr(), None) == -1
    assert lib.sgg_adam_tf_multi_ema_guarded(*a, 64, 1e-4, 0.5, 0.9, 1e-8, good.data_ptr() + 4, 0.5, None) == -1
    assert lib.sgg_adam_tf_multi_ema_guarded(*a, 0, 1e-4, 0.5, 0.9, 1e-8, good.data_ptr(), 0.5, None) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((base, rec, ws), keep)), "a rejected call wrote to a buffer"
    assert all(bool((t == 0.5).all()) for t in (p, g_, m, v, e)) and bool((good == 0).all())


# ---- the guarded Adam kernels -------------------------------------------------------------------------------------------------------
def adam_inputs(n, special=False):
    """p, g, m, v, e: seeded, no zero, no subnormal; special: NaNs with payloads, +-Inf and -0 at both ends of p, m, v and e."""
    r = np.random.RandomState(1000 + n % 9973)
    sign = lambda: np.where(r.rand(n) < 0.5, -1.0, 1.0)
    p = (sign() * r.uniform(1e-3, 1.0, n)).astype(np.float32)
    g = (sign() * r.uniform(1e-4, 8.0, n)).astype(np.float32)
    m = (sign() * r.uniform(1e-6, 1e-2, n)).astype(np.float32)
    v = r.uniform(1e-10, 1e-3, n).astype(np.float32)
    e = (sign() * r.uniform(1e-3, 1.0, n)).astype(np.float32)
    if special:
        pay = np.array([0x7fc00001, 0x7f800001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x7fffffff, 0xffc00000], dtype=np.uint32)
        for s, a in enumerate((p, m, v, e)):
            u = a.view(np.uint32)
            for k, i in enumerate(sorted(set(range(min(n, 8))) | set(range(max(0, n - 8), n)))):
                u[i] = pay[(k + s) % 8]
    return p, g, m, v, e


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_guarded_adam_is_the_unguarded_kernel_fed_s_eff(hip, n):
    host = adam_inputs(n)
    lr_t, omd, grad_scale = tf_adam_lr_t(3), 0.1, 0.5
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    hip.grad_guard(torch.from_numpy(host[1]).cuda(), rec, grad_scale, 1e-3, True)
    r = rec.cpu().numpy()
    s_eff = float(r[4])
    assert r[5] == 1.0 and r[3] < 1.0 and s_eff != grad_scale and s_eff == float(np.float32(s_eff)) and r[6] == 1.0
    plain = [torch.from_numpy(a).cuda() for a in host]
    hip.adam_ema(*plain, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, s_eff, omd)
    only = [torch.from_numpy(a).cuda() for a in host[:4]]
    hip.adam(*only, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, s_eff)
    assert not np.array_equal(bits(plain[0]), host[0].view(np.int32))
    # the scale matters at this precision: the unguarded kernel fed grad_scale itself gives other moments
    other = [torch.from_numpy(a).cuda() for a in host[:4]]
    hip.adam(*other, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, grad_scale)
    assert not np.array_equal(bits(other[2]), bits(only[2]))
    for fused in (False, True):
        pairs = [guarded(a) for a in (host if fused else host[:4])]
        bufs = [v for _, v in pairs]
        if fused:
            hip.adam_ema_guarded(*bufs, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, rec, omd)
        else:
            hip.adam_guarded(*bufs, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, rec)
        torch.cuda.synchronize()
        what = "n %d %s" % (n, "adam_ema_guarded" if fused else "adam_guarded")
        assert all(untouched(big, n) for big, _ in pairs), "written outside a buffer: " + what
        want = plain if fused else only
        for name, k in (("params", 0), ("m", 2), ("v", 3)) + ((("ema", 4),) if fused else ()):
            assert np.array_equal(bits(bufs[k]), bits(want[k])), "%s differs from the unguarded kernel fed s_eff: %s" % (name, what)
        assert np.array_equal(bits(bufs[1]), host[1].view(np.int32)), "grads changed: " + what
        assert np.array_equal(rec.cpu().numpy().view(np.int64), r.view(np.int64)), "the record changed: " + what


@pytest.mark.parametrize("n", ADAM_SIZES)
def test_guarded_adam_writes_nothing_when_the_update_is_dropped(hip, n):
    host = adam_inputs(n, special=True)
    g = host[1].copy()
    g[n // 2] = np.nan
    host = (host[0], g) + host[2:]
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    hip.grad_guard(torch.from_numpy(g).cuda(), rec, 1.0, 1e-3, True)
    r = rec.cpu().numpy()
    assert r[5] == 0.0 and r[1] == 1.0 and r[7] == 1.0 and r[6] == 0.0
    for fused in (False, True):
        pairs = [guarded(a) for a in (host if fused else host[:4])]
        bufs = [v for _, v in pairs]
        if fused:
            hip.adam_ema_guarded(*bufs, 1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, rec, 0.1)
        else:
            hip.adam_guarded(*bufs, 1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, rec)
        torch.cuda.synchronize()
        assert all(untouched(big, n) for big, _ in pairs)
        for name, buf, a in zip(("params", "grads", "m", "v", "ema"), bufs, host):
            assert np.array_equal(bits(buf), a.view(np.int32)), "%s changed in a dropped update (n %d, fused %s)" % (name, n, fused)
    # the same operands with the decision reversed by hand are written: the test can fail
    rec[5] = 1.0
    bufs = [torch.from_numpy(a).cuda() for a in host[:4]]
    hip.adam_guarded(*bufs, 1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, rec)
    assert not np.array_equal(bits(bufs[2]), host[2].view(np.int32))


# ---- step level -----------------------------------------------------------------------------------------------------------------
B, S, V = 4, 64, 50
CRITIC_ITERS = 2
_CACHE = {}


def _states(dtype=torch.float32):
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    dp["W"] = dp["W"] * 25.0
    return {k: v.to(dtype) for k, v in gp.items()}, {k: v.to(dtype) for k, v in dp.items()}


def _inputs(rows=B):
    images, labels, _ = O.synth_batch(rows, S, V)
    return images, labels, (lambda s: O.synth_noise(rows, s)), (lambda s: O.synth_alpha(rows, s).reshape(rows))


def _step(hip, guard=None, overlap=True, decay=None, armed=False):
    gp, dp = _states()
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp, overlap_streams=overlap)
    if decay is not None:
        gs.G.enable_averaging(decay)
    if guard is not None:
        gs.set_guard(*guard)
    if armed:
        gs.arm_diagnostics(True)
    return gs


def _arenas(gs):
    gs.flush()
    torch.cuda.synchronize()
    out = {}
    for n, net in (("G", gs.G), ("D", gs.D)):
        out[n + ".weights"], out[n + ".m"], out[n + ".v"] = net.arena.flat.clone(), net.m_flat.clone(), net.v_flat.clone()
    out["losses"] = torch.cat([gs.d_losses, gs.g_losses]).clone()
    return out


def _iteration(gs):
    images, labels, noise, alpha = _inputs()
    gs.train_iteration(images.cuda(), labels.cuda(), [noise(10 + i).cuda() for i in range(CRITIC_ITERS + 1)],
                       [alpha(10 + i).cuda() for i in range(CRITIC_ITERS)], critic_iters=CRITIC_ITERS)


def _host_ss(net, scale):
    x = (net.arena.live(net.grad_flat).cpu().numpy() * np.float32(scale)).astype(np.float64)
    return float(np.sum(x * x)), x.size


def unguarded(hip):
    """One critic update then one generator update WITHOUT a guard, once for the module: the arenas of an iteration besides, and the
    norms of the two first updates (the thresholds of the clipped runs are a quarter of them)."""
    if "plain" not in _CACHE:
        gs = _step(hip)
        _iteration(gs)
        it = _arenas(gs)
        assert all(bool(torch.isfinite(t).all()) for t in it.values())
        gs = _step(hip)
        images, labels, noise, alpha = _inputs()
        gs.critic_step(images.cuda(), labels.cuda(), noise(0).cuda(), alpha(0).cuda())
        gs.generator_step(images.cuda(), noise(1).cuda())
        gs.flush()
        torch.cuda.synchronize()
        norms = {n: _host_ss(net, 1.0)[0] ** 0.5 for n, net in (("D", gs.D), ("G", gs.G))}
        assert not gs.D.has_guard and gs.guard_reports() == {}
        _CACHE["plain"] = {"iteration": it, "norms": norms}
    return _CACHE["plain"]


def test_unreachable_threshold_is_the_unguarded_step_bit_for_bit(hip):
    want = unguarded(hip)["iteration"]
    gs = _step(hip, guard=(1e30, True))
    _iteration(gs)
    got = _arenas(gs)
    bad = [k for k in want if not np.array_equal(bits(got[k]), bits(want[k]))]
    assert not bad, "the guarded run with an unreachable threshold differs from the unguarded one in %s" % bad
    rep = gs.guard_reports()
    for n in ("D", "G"):
        assert rep[n]["coef"] == 1.0 and rep[n]["apply"] and rep[n]["clipped"] == rep[n]["skipped"] == rep[n]["nonfinite"] == 0
        assert rep[n]["norm"] > 0 and rep[n]["s_eff"] == 1.0


def cpu_clipped(clip):
    """The CPU fp64 step of tests/test_guard_cpu.py on the same states and inputs with the same thresholds: m of both networks after
    their first update, per tensor."""
    if "cpu" not in _CACHE:
        gp, dp = _states(torch.float64)
        gs = GanStep(GuardRefKernels(), V, S, B, lam=10.0, g_state=gp, d_state=dp, dtype=torch.float64)
        gs.set_guard(clip, False)
        images, labels, noise, alpha = _inputs()
        gs.critic_step(images.double(), labels, noise(0).double(), alpha(0).double())
        gs.generator_step(images.double(), noise(1).double())
        _CACHE["cpu"] = {n: {k: v.clone() for k, v in net.arena._make_views(net.m_flat).items()} for n, net in (("D", gs.D), ("G", gs.G))}
        _CACHE["cpu_reports"] = gs.guard_reports()
    return _CACHE["cpu"], _CACHE["cpu_reports"]


def test_active_clipping_against_host_norm_statistics_pass_and_cpu_step(hip):
    norms = unguarded(hip)["norms"]
    clip = (norms["D"] / 4.0, norms["G"] / 4.0)
    gs = _step(hip, guard=(clip, False), armed=True)
    images, labels, noise, alpha = _inputs()
    gs.critic_step(images.cuda(), labels.cuda(), noise(0).cuda(), alpha(0).cuda())
    gs.generator_step(images.cuda(), noise(1).cuda())
    diag = gs.diagnostics()
    rep = gs.guard_reports()
    assert diag["guard"] == rep
    ref_m, ref_rep = cpu_clipped(clip)
    for n, net in (("D", gs.D), ("G", gs.G)):
        r = rep[n]
        assert r["apply"] and r["clipped"] == 1 and r["skipped"] == 0 and r["nonfinite"] == 0
        ss, count = _host_ss(net, 1.0)
        print("%s: reported ss %.17g, host fp64 %.17g (diff %.3e, bound %.3e); coef %.9f (CPU fp64 step %.9f)"
              % (n, r["ss"], ss, abs(r["ss"] - ss), count * U52 * ss, r["coef"], ref_rep[n]["coef"]))
        assert abs(r["ss"] - ss) <= count * U52 * ss and r["norm"] == float(np.sqrt(np.float64(r["ss"])))
        # the statistics pass sums the same squares per tensor (the padding between tensors holds zeros) and the host sums its T rows:
        # each device sum is within count * 2^-52 * ss of the exact one, the sum over the rows adds T <= count more
        stats_ss = float(net.opt["diag"]["rows"][:, 0].sum())
        assert abs(r["ss"] - stats_ss) <= 3 * count * U52 * ss, (n, r["ss"], stats_ss)
        assert abs(diag[n]["grad_norm"] - r["norm"]) <= 3 * count * U52 * r["norm"]
        assert abs(r["coef"] - 0.25) < 1e-3, "the first update's norm is not the unguarded run's"
        assert r["s_eff"] == float(np.float32(r["coef"]))
        views = net.arena._make_views(net.m_flat)
        names = [k for k in views if not (n == "D" and k == "decoder/bias")]     # (its gradient cancels analytically: tests/test_step_gpu.py)
        worst = max((float((views[k].cpu().double() - ref_m[n][k]).abs().max() / (ref_m[n][k].abs().max() + 1e-30)), k) for k in names)
        print("%s m after the first clipped update: worst rel err %.3e (%s)" % ((n,) + worst))
        assert worst[0] < GRAD_RTOL, "%s m of %s: rel err %.3e" % (n, worst[1], worst[0])
        # m of the unclipped update is four times as large: the comparison can fail
        k = worst[1]
        assert float(views[k].abs().max()) < 0.3 * float(ref_m[n][k].abs().max()) / r["coef"]


def test_clipping_with_micro_batches_and_averaging_feeds_s_eff_to_the_fused_kernel(hip):
    N, decay = 2, 0.9
    norms = unguarded(hip)["norms"]
    gs = _step(hip, guard=((norms["D"] / 4.0, norms["G"] / 4.0), True), decay=decay)
    images, labels, noise, alpha = _inputs(N * B)
    cut = lambda t, k: t[k * B:(k + 1) * B].contiguous().cuda()
    snaps = {}
    for name, net in (("D", gs.D), ("G", gs.G)):
        def spy(scale=1.0, net=net, name=name, orig=net.adam_step):
            a = net.arena
            snaps[name] = {"scale": scale, "lr_t": tf_adam_lr_t(net.adam_t + 1),
                           "bufs": [a.live(t).clone() for t in (a.flat, net.grad_flat, net.m_flat, net.v_flat)],
                           "ema": a.live(net.opt["ema"]["flat"]).clone() if net.has_average else None}
            return orig(scale)
        net.adam_step = spy
    for k in range(N):
        gs.critic_step(cut(images, k), cut(labels, k), cut(noise(0), k), cut(alpha(0), k), micro=(k, N))
    for k in range(N):
        gs.generator_step(cut(images, k), cut(noise(1), k), micro=(k, N))
    gs.flush()
    torch.cuda.synchronize()
    rep = gs.guard_reports()
    assert gs.G.opt["ema"]["updates"] == 1 and gs.D.adam_t == gs.G.adam_t == 1
    for name, net in (("D", gs.D), ("G", gs.G)):
        sn, r, a = snaps[name], rep[name], net.arena
        assert sn["scale"] == 0.5, "the guard did not get the gradient scale 1 / N"
        ss, count = _host_ss(net, 0.5)                   # grad_flat holds the SUM over the micro-batches
        print("%s: N = 2, reported norm %.9e, host %.9e, coef %.6f, s_eff %.9g" % (name, r["norm"], ss ** 0.5, r["coef"], r["s_eff"]))
        assert abs(r["ss"] - ss) <= count * U52 * ss
        assert r["apply"] and r["clipped"] == 1 and r["coef"] < 1.0 and r["s_eff"] == float(np.float32(np.float64(np.float32(0.5)) * r["coef"]))
        bufs = sn["bufs"]
        if sn["ema"] is None:
            hip.adam(*bufs, sn["lr_t"], ADAM_B1, ADAM_B2, ADAM_EPS, r["s_eff"])
        else:
            hip.adam_ema(*bufs, sn["ema"], sn["lr_t"], ADAM_B1, ADAM_B2, ADAM_EPS, r["s_eff"], E.one_minus_decay(decay, 0))
            assert np.array_equal(bits(a.live(net.opt["ema"]["flat"])), bits(sn["ema"])), "the average is not the fused kernel's fed s_eff"
            assert not np.array_equal(bits(sn["ema"]), bits(a.live()))
        for what, got, want in zip(("weights", "m", "v"), (a.live(), a.live(net.m_flat), a.live(net.v_flat)), (bufs[0], bufs[2], bufs[3])):
            assert np.array_equal(bits(got), bits(want)), "%s %s differ from the plain kernel fed s_eff" % (name, what)
    assert (snaps["G"]["ema"] is not None) and (snaps["D"]["ema"] is None)


def test_a_nan_in_the_gradient_keeps_everything_and_the_next_step_is_clean(hip):
    gs = _step(hip, guard=(0.0, True), decay=0.9)
    images, labels, noise, alpha = _inputs()
    img, lab = images.cuda(), labels.cuda()
    gs.critic_step(img, lab, noise(0).cuda(), alpha(0).cuda())
    gs.generator_step(img, noise(1).cuda())
    gs.flush()
    for name, net in (("D", gs.D), ("G", gs.G)):
        avg = net.opt.get("ema")
        tensors = [net.arena.flat, net.m_flat, net.v_flat] + ([avg["flat"]] if avg else [])
        keep = [t.clone() for t in tensors]
        t0, version, updates = net.adam_t, net.arena.version, (avg["updates"] if avg else None)
        net.grad_flat[net.arena.live_numel // 2] = float("nan")
        net.adam_step()
        torch.cuda.synchronize()
        for what, a, b in zip(("weights", "m", "v", "average"), tensors, keep):
            assert np.array_equal(bits(a), bits(b)), "%s %s changed in a dropped update" % (name, what)
        assert net.adam_t == t0 + 1 and net.arena.version == version + 1 and (avg is None or avg["updates"] == updates + 1)
        r = net.guard_report()
        assert not r["apply"] and r["skipped"] == 1 and r["nonfinite"] == 1 and r["clipped"] == 0
    gs.critic_step(img, lab, noise(2).cuda(), alpha(2).cuda())
    gs.generator_step(img, noise(3).cuda())
    got = _arenas(gs)
    assert all(bool(torch.isfinite(t).all()) for t in got.values()), "the step after a dropped update is not clean"
    rep = gs.guard_reports()
    for name, net in (("D", gs.D), ("G", gs.G)):
        assert rep[name]["apply"] and rep[name]["skipped"] == 1 and rep[name]["nonfinite"] == 0 and net.adam_t == 3
    assert bool(torch.isfinite(gs.G.opt["ema"]["flat"]).all())


# ---- train.py -------------------------------------------------------------------------------------------------------------------
def _train(tmp_path, name, flags):
    ck, logs = tmp_path / name, tmp_path / (name + "_logs")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "4,64,50", "--critic_iters", "2", "--max_iterations", "3",
           "--log_every", "1", "--checkpoints_dir", str(ck), "--summaries_dir", str(logs)] + flags
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(str(ck / "model.ckpt.pt"), map_location="cpu"), [json.loads(l) for l in open(str(logs / "losses.jsonl"))]


def test_train_cli_logs_and_saves_the_guard(tmp_path):
    ck, recs = _train(tmp_path, "a", ["--clip_grad_norm", "1e-3,1e-4", "--skip_nonfinite"])
    assert ck["itr"] == 3 and len(recs) == 3
    for i, rec in enumerate(recs):
        gd = rec["guard"]
        assert set(gd) == {"D", "G"}
        for n, mx in (("D", 1e-3), ("G", 1e-4)):
            assert gd[n]["max_norm"] == mx and gd[n]["skip_nonfinite"] is True and gd[n]["norm"] > 0 and gd[n]["apply"] is True
            assert gd[n]["skipped"] == 0 and 0 < gd[n]["coef"] <= 1.0
        assert gd["D"]["clipped"] <= 2 * (i + 1) and gd["G"]["clipped"] <= i + 1
    last = recs[-1]["guard"]
    assert ck["guard"] == {n: {"clipped": last[n]["clipped"], "skipped": 0} for n in ("D", "G")}
    assert last["D"]["clipped"] + last["G"]["clipped"] > 0, "thresholds this small clipped nothing"


def test_train_cli_without_the_flags_writes_neither(tmp_path):
    ck, recs = _train(tmp_path, "b", [])
    assert ck["itr"] == 3 and len(recs) == 3 and "guard" not in ck and all("guard" not in r for r in recs)
