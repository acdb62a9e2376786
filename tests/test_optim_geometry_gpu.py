"""-m gpu: the four Adam kernels of csrc/optim.hip (adam_body<EMA, GUARDED> behind HipKernels.adam, adam_ema, adam_guarded and
adam_ema_guarded) per element against fp64, at the geometry of the whole-arena pass.

The sizes and input regimes are those of tests/optim_cases.py (why each exists is said there and checked without a GPU by
tests/test_optim_cases_cpu.py); the reference adam_ref and the per-element bounds on m', v', u, p' and e' are those of
tests/optim_ref.py, which counts fp32 roundings and is fitted to nothing.  Each kernel is compared with the reference on its own:
the tests that pin the kernels to each other bit for bit (tests/test_ema_gpu.py, tests/test_guard_gpu.py) say nothing about the
arithmetic all four share.  Every operand lies between sentinel guards; no element is exempt from a comparison.

Measured on one MI355X (profiles/optim_geometry_pytest_gpu.log), worst |device - reference| in units of the bound over every case:
m' 0.608 (0.792 with the other betas), v' 0.883, u 0.485, e' 0.523, and p' 0.999: where u is far below p the bound of p' is the one
rounding of p - u, which a rounding reaches.  The numbers are reported, not used: no bound was set from them.

Each comparison prints "optim-geometry <case>: worst err / bound per quantity"; the last test prints the worst of the whole file.
"""
import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd import ema as E
from sgg_amd.params import ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_LR
from sgg_amd.step import GanStep, tf_adam_lr_t
from tests import optim_cases as OC
from tests import optim_ref as R

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, -777.0          # 64 floats: the view between the guards keeps the 16-byte alignment of the allocation
KERNELS = ("adam", "adam_ema", "adam_guarded", "adam_ema_guarded")
WORST = {}                          # quantity: worst err / bound over the file


def up(a):
    return torch.from_numpy(np.array(a)).cuda()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def guarded(src, n):
    """A copy of the first n elements of the device tensor `src` between two sentinel guards: (whole buffer, the view the kernel gets)."""
    big = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    view = big[PAD:PAD + n]
    view.copy_(src[:n])
    assert view.data_ptr() % 16 == 0
    return big, view


def untouched(big, n):
    return bool((big[:PAD] == SENTINEL).all() and (big[PAD + n:] == SENTINEL).all())


def within(what, quantity, got, ref, bound):
    """|got - ref| <= bound for every element, on the device in fp64 (got: fp32; ref, bound: the fp64 arrays of the reference; a NaN
    fails; an element whose bound is 0 must be exact).  Returns the worst err / bound."""
    err = (got.double() - ref).abs()
    ok = err <= bound
    pos = bound > 0
    worst = float(torch.where(pos, err / torch.where(pos, bound, torch.ones_like(bound)), torch.zeros_like(err)).max())
    WORST[quantity] = max(WORST.get(quantity, 0.0), worst)
    if not bool(ok.all()):
        k = int((~ok).nonzero()[0])
        raise AssertionError("%s %s: %d of %d elements outside the bound, worst %.3g x; first at %d: got %.9e, reference %.17e, bound %.3e"
                             % (what, quantity, int((~ok).sum()), ok.numel(), worst, k, float(got[k]), float(ref[k]), float(bound[k])))
    return worst


# ---- the case list: every kernel, regime and size --------------------------------------------------------------------------------------
_dev = {}


def device_case(regime):
    """The regime's operands, fp64 reference and bounds on the device, for its largest size (every size is a prefix); computed once per
    regime on the host, one regime resident at a time."""
    if regime.name not in _dev:
        _dev.clear()
        torch.cuda.empty_cache()
        t, avg, b, avg_b = OC.reference(regime)
        d = {"ops": [up(a) for a in OC.operands(regime)], "ref": {k: up(t[k]) for k in "mvup"}, "bound": {k: up(b[k]) for k in "mvup"},
             "e": {omd: up(avg[omd]["e"]) for omd in OC.OMDS}, "e_bound": {omd: up(avg_b[omd]) for omd in OC.OMDS}}
        if regime.name == "d_zeros":
            d["zero"] = up(OC.zero_mask(OC.largest(regime)))
        _dev[regime.name] = d
    return _dev[regime.name]


def record(scale, apply):
    """The 8-double record of csrc/guard.hip as the guarded kernels read it: slot 4 the gradient scale, slot 5 the apply flag."""
    return torch.tensor([0.0, 0.0, 0.0, 1.0, scale, apply, 0.0, 0.0], dtype=torch.float64, device="cuda")


CASES = [(r, s) for r in OC.REGIMES for s in OC.sizes(r)]


@pytest.mark.parametrize("regime,size", CASES, ids=["%s-n%d" % (r.name, s.n) for r, s in CASES])
def test_kernels_per_element(hip, regime, size):
    n, d = size.n, device_case(regime)
    lr_t, b1, b2, eps = OC.hyper(regime)
    assert (b1, b2, eps) == (ADAM_B1, ADAM_B2, ADAM_EPS) and lr_t == tf_adam_lr_t(regime.t)
    rec = record(regime.record4, 1.0)
    rec_bits = rec.clone()
    lines = []
    for kernel in KERNELS:
        has_avg, reads_record = "ema" in kernel, "guarded" in kernel
        for omd in (OC.OMDS if has_avg else (None,)):
            pairs = [guarded(a, n) for a in d["ops"][:5 if has_avg else 4]]
            bufs = [view for _, view in pairs]
            getattr(hip, kernel)(*bufs, lr_t, b1, b2, eps, rec if reads_record else regime.gscale, *((omd,) if has_avg else ()))
            torch.cuda.synchronize()
            what = "%s n %d %s%s" % (regime.name, n, kernel, "" if omd is None else " omd %g" % omd)
            assert all(untouched(big, n) for big, _ in pairs), "written outside a buffer: " + what
            assert torch.equal(bits(bufs[1]), bits(d["ops"][1][:n])), "grads changed: " + what
            assert torch.equal(rec, rec_bits), "the record changed: " + what
            w = [within(what, q, bufs[k], d["ref"][q][:n], d["bound"][q][:n]) for q, k in (("m", 2), ("v", 3), ("p", 0))]
            if has_avg:
                w.append(within(what, "e", bufs[4], d["e"][omd][:n], d["e_bound"][omd][:n]))
            if regime.name == "b_p_zero":             # p = 0: u = p - p' = -p' exactly
                w.append(within(what, "u", -bufs[0], d["ref"]["u"][:n], d["bound"]["u"][:n]))
            if regime.name == "d_zeros":
                z = d["zero"][:n]
                assert torch.equal(bits(bufs[0])[z], bits(d["ops"][0][:n])[z]), "p changed where g = m = v = 0: " + what
                assert not bool(bufs[2][z].any()) and not bool(bufs[3][z].any())
            lines.append("optim-geometry %s: worst err / bound  %s" % (what, "  ".join("%s %.3f" % (q, x) for q, x in zip("mvpe" if has_avg else "mvp", w))
                                                                     + ("  u %.3f" % w[-1] if regime.name == "b_p_zero" else "")))
    print("optim-geometry %s n %d: grid %d, trips %d, workgroups on the last trip %d, tail %d" % (regime.name, n, size.grid, size.trips,
                                                                                                size.last_trip_groups, size.tail))
    print("\n".join(lines))


@pytest.mark.parametrize("b1,b2", OC.OTHER_BETAS)
def test_other_betas(hip, b1, b2):
    """With beta1 = 0.5 the two factors of m' are interchangeable and 1.f - b is exact for both of the project's betas: the four
    kernels once with betas that tell b from 1 - b, gradient scale 1 / 3."""
    regime, n = OC.BY_NAME["a_typical"], OC.OTHER_BETAS_N
    ops = OC.operands(regime, n)
    dev_ops = [up(a) for a in ops]
    lr_t, third, omd = OC.hyper(regime)[0], 1.0 / 3.0, 0.9
    t = R.adam_terms(*ops, lr_t, b1, b2, ADAM_EPS, third, omd)
    b = R.adam_bounds(t, ops[0], ops[4], lr_t, b1, b2, third, omd)
    ref, bound = {q: up(t[q]) for q in "mvpe"}, {q: up(b[q]) for q in "mvpe"}
    rec = record(third, 1.0)
    for kernel in KERNELS:
        has_avg = "ema" in kernel
        pairs = [guarded(a, n) for a in dev_ops[:5 if has_avg else 4]]
        bufs = [view for _, view in pairs]
        getattr(hip, kernel)(*bufs, lr_t, b1, b2, ADAM_EPS, rec if "guarded" in kernel else third, *((omd,) if has_avg else ()))
        torch.cuda.synchronize()
        what = "betas (%g, %g) n %d %s" % (b1, b2, n, kernel)
        assert all(untouched(big, n) for big, _ in pairs), "written outside a buffer: " + what
        w = [within(what, q, bufs[k], ref[q], bound[q]) for q, k in (("m", 2), ("v", 3), ("p", 0), ("e", 4))[:4 if has_avg else 3]]
        print("optim-geometry %s: worst err / bound  %s" % (what, "  ".join("%s %.3f" % qx for qx in zip("mvpe", w))))


def test_dropped_update_writes_nothing_at_the_third_trip_size(hip):
    """record[5] == 0: all five operands keep every bit (tests/test_guard_gpu.py has the sizes up to one pass)."""
    regime, n = OC.BY_NAME["a_typical"], OC.THIRD_TRIP
    d = {"ops": [up(a) for a in OC.operands(regime, n)]}
    rec = record(regime.record4, 0.0)
    for kernel in ("adam_guarded", "adam_ema_guarded"):
        has_avg = "ema" in kernel
        pairs = [guarded(a, n) for a in d["ops"][:5 if has_avg else 4]]
        bufs = [view for _, view in pairs]
        getattr(hip, kernel)(*bufs, *OC.hyper(regime), rec, *((0.9,) if has_avg else ()))
        torch.cuda.synchronize()
        assert all(untouched(big, n) for big, _ in pairs)
        for name, buf, src in zip(("params", "grads", "m", "v", "ema"), bufs, d["ops"]):
            assert torch.equal(bits(buf), bits(src[:n])), "%s changed in a dropped update (%s)" % (name, kernel)
    # the same record with the flag set is applied: the test can fail
    rec[5] = 1.0
    bufs = [guarded(a, n)[1] for a in d["ops"][:4]]
    hip.adam_guarded(*bufs, *OC.hyper(regime), rec)
    assert not torch.equal(bits(bufs[0]), bits(d["ops"][0][:n]))


# ---- twenty steps, each against the reference on the device's own state ----------------------------------------------------------------
def test_trajectory_step_by_step(hip):
    """From m = v = 0 with a fresh seeded gradient per step and the host's lr_t: every step is a pure function of its inputs, so it is
    compared with adam_ref on the state the device held before it - no accumulated bound."""
    for t in (1, 2, 3, 10, 1000):
        want = np.float64(ADAM_LR) * np.sqrt(np.float64(1.0) - np.float64(ADAM_B2) ** t) / (np.float64(1.0) - np.float64(ADAM_B1) ** t)
        assert abs(tf_adam_lr_t(t) - float(want)) <= 4 * 2.0 ** -53 * float(want), t
    assert abs(tf_adam_lr_t(1) - 1e-4 * 0.1 ** 0.5 / 0.5) < 1e-19 and abs(tf_adam_lr_t(1000) - 1e-4) < 1e-19
    n = 4 * 256 * 3 + 3                                  # four workgroups, a tail
    p0, _, _, _, e0 = OC.operands(OC.BY_NAME["a_typical"], n)
    pairs = [guarded(up(a), n) for a in (p0, p0, np.zeros(n, np.float32), np.zeros(n, np.float32), e0)]
    bufs = [view for _, view in pairs]
    worst = {}
    for t in range(1, 21):
        r = np.random.RandomState(500 + t)
        g = (np.where(r.rand(n) < 0.5, -1.0, 1.0) * r.uniform(1e-4, 8.0, n)).astype(np.float32)
        bufs[1].copy_(up(g))
        before = [b.cpu().numpy() for b in bufs]
        lr_t, omd = tf_adam_lr_t(t), E.one_minus_decay(0.999, t - 1)
        hip.adam_ema(*bufs, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0, omd)
        torch.cuda.synchronize()
        assert all(untouched(big, n) for big, _ in pairs)
        terms = R.adam_terms(*before, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0, omd)
        bound = R.adam_bounds(terms, before[0], before[4], lr_t, ADAM_B1, ADAM_B2, 1.0, omd)
        for q, k in (("m", 2), ("v", 3), ("p", 0), ("e", 4)):
            w = within("trajectory step %d" % t, q, bufs[k], up(terms[q]), up(bound[q]))
            worst[q] = max(worst.get(q, 0.0), w)
        assert not np.array_equal(bufs[0].cpu().numpy(), before[0])
    print("optim-geometry trajectory of 20 steps, n %d: worst err / bound  %s" % (n, "  ".join("%s %.3f" % kv for kv in worst.items())))


# ---- Network.adam_step: t -> lr_t, the scale, one_minus_decay and the range ------------------------------------------------------------
def test_network_adam_step_plumbing(hip):
    """Three calls of Network.adam_step(0.125) with averaging on, at the configs[0] size: every word of the live ranges of the arena,
    m_flat, v_flat and the average against adam_ref on the snapshot before the call (fp64 on the host, in chunks); every word
    outside the live ranges keeps its bits."""
    B, S, V, decay, scale = 8, 64, 50, 0.999, 0.125
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=O.init_params("G", V, S, perturb=0.05), d_state=O.init_params("D", V, S, perturb=0.05))
    net = gs.G
    net.enable_averaging(decay)
    a, n = net.arena, net.arena.live_numel
    assert 0 < n < a.flat.numel() and net.adam_t == 0
    flats = lambda: (a.flat, net.grad_flat, net.m_flat, net.v_flat, net.opt["ema"]["flat"])
    worst = {}
    for call in range(3):
        gen = torch.Generator().manual_seed(900 + call)
        g = (torch.rand(n, generator=gen) * 7.9 + 0.1) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1) * 10.0 ** -call
        net.grad_flat[:n].copy_(g.cuda())
        net.grad_flat[n:] = SENTINEL
        before = [f.cpu() for f in flats()]
        net.adam_step(scale)
        torch.cuda.synchronize()
        after = [f.cpu() for f in flats()]
        assert net.adam_t == call + 1 and net.opt["ema"]["updates"] == call + 1
        lr_t, omd = tf_adam_lr_t(call + 1), E.one_minus_decay(decay, call)
        assert omd == 1.0 - (1.0 + call) / (10.0 + call)
        for name, x, y in zip(("arena", "grads", "m_flat", "v_flat", "average"), before, after):
            assert torch.equal(bits(x[n:]), bits(y[n:])), "call %d: %s changed outside the live range" % (call, name)
        assert torch.equal(bits(before[1]), bits(after[1])), "call %d: the gradient changed" % call
        for lo in range(0, n, 1 << 22):
            hi = min(n, lo + (1 << 22))
            ops = [x[lo:hi] for x in before]
            terms = R.adam_terms(*ops, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, scale, omd)
            bound = R.adam_bounds(terms, ops[0], ops[4], lr_t, ADAM_B1, ADAM_B2, scale, omd)
            for q, k in (("p", 0), ("m", 2), ("v", 3), ("e", 4)):
                w = within("adam_step call %d words %d..%d" % (call, lo, hi), q, after[k][lo:hi], terms[q], bound[q])
                worst[q] = max(worst.get(q, 0.0), w)
        assert not torch.equal(after[0][:n], before[0][:n])
    print("optim-geometry Network.adam_step x 3, %d live words of %d: worst err / bound  %s" % (n, a.flat.numel(),
                                                                                              "  ".join("%s %.3f" % kv for kv in worst.items())))


def test_worst_errors_of_the_file():
    """(runs last) the worst err / bound per quantity over every comparison above"""
    print("optim-geometry worst err / bound over the file:  " + "  ".join("%s %.3f" % (q, WORST[q]) for q in "mvupe" if q in WORST))
    assert all(x <= 1.0 for x in WORST.values())
