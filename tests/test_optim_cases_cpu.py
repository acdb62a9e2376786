"""The cases, the fp64 restatement and the bounds of tests/test_optim_geometry_gpu.py, checked without a GPU: the launch arithmetic of
tests/optim_cases.py against the constants in csrc/optim.hip and csrc/sgg_common.h and against a walk through the grid-stride loop;
every regime's operands and reference intermediates zero or normal; two fp32 emulations of the device arithmetic (one rounding after
every operation, one with every product-plus-sum rounded once) inside every bound of tests/optim_ref.py, so the reference and the
count of roundings stand on their own; the two misplacements of eps outside the bound; known answers of adam_ref.

Each emulation prints "optim-bounds <regime> <emulation>: worst err / bound per quantity".  A ratio near 1 would mean a miscounted
rounding, not a bound in need of a margin - with one exception: where u is far below p the bound of p' is the single rounding of
p - u, U |p'|, and a single rounding reaches its bound (0.999)."""
import os

import numpy as np
import pytest

from tests import optim_cases as OC
from tests import optim_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scene-graph-gan_amd", "csrc")
MIN_NORMAL = 2.0 ** -126
MAX_F32 = float(np.finfo(np.float32).max)


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, start, end="\n}\n"):
    i = src.index(start)
    return src[i:src.index(end, i)]


# ---- launch arithmetic -------------------------------------------------------------------------------------------------------------
def test_constants_are_those_of_the_sources():
    common, optim = _source("sgg_common.h"), _source("optim.hip")
    g = _body(common, "static inline int grid_for(")
    assert "(n + block - 1) / block" in g and "if (g > %d) g = %d;" % (OC.GRID_CAP, OC.GRID_CAP) in g and "if (g < 1) g = 1;" in g
    assert "typedef float f32x4 __attribute__((ext_vector_type(%d)));" % OC.VEC in common
    launch = _body(optim, "static int adam_launch(")
    assert "const dim3 grid(grid_for(n / %d + 1, %d)), block(%d);" % (OC.VEC, OC.BLOCK, OC.BLOCK) in launch
    body = _body(optim, "void adam_body(")
    assert "const long long n4 = n >> 2;" in body and "for (long long i = i0; i < n4; i += stride) {" in body
    assert "if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {" in body and "const long long i = (n4 << 2) + threadIdx.x;" in body
    assert "if (rec[5] == 0.0) return;" in body and "gscale = (float)rec[4];" in body
    assert "#define SGG_GRID_I0 ((long long)blockIdx.x * blockDim.x + threadIdx.x)" in optim
    assert "#define SGG_GRID_STRIDE ((long long)gridDim.x * blockDim.x)" in optim
    assert OC.ONE_PASS == 4 * 256 * 4096 and OC.THIRD_TRIP == 2 * OC.ONE_PASS + 4 * 256 * 5 + 1
    # the expressions the bounds of tests/optim_ref.py count the roundings of
    for line in ("reinterpret_cast<const f32x4*>(g)[i] * gscale;", "mv = mv * b1 + gv * (1.f - b1);", "vv = vv * b2 + gv * gv * (1.f - b2);",
                 "pv[q] -= lr_t * mv[q] / (sqrtf(vv[q]) + eps);", "ev[q] -= (ev[q] - pv[q]) * omd;",
                 "const float gv = g[i] * gscale;", "const float mv = m[i] * b1 + gv * (1.f - b1);",
                 "const float vv = v[i] * b2 + gv * gv * (1.f - b2);", "pv -= lr_t * mv / (sqrtf(vv) + eps);", "e[i] = ev - (ev - pv) * omd;"):
        assert line in body, line


def test_hyperparameters_are_those_of_the_package():
    import sgg_amd  # noqa: F401
    from sgg_amd import params as P
    from sgg_amd.step import tf_adam_lr_t
    assert (OC.ADAM_LR, OC.ADAM_B1, OC.ADAM_B2, OC.ADAM_EPS) == (P.ADAM_LR, P.ADAM_B1, P.ADAM_B2, P.ADAM_EPS)
    for t in (1, 2, 3, 10, 1000):
        assert abs(tf_adam_lr_t(t) - R.lr_t(t, OC.ADAM_LR, OC.ADAM_B1, OC.ADAM_B2)) <= 4 * 2.0 ** -53 * tf_adam_lr_t(t)


def test_size_list_is_the_one_of_the_issue():
    P = OC.ONE_PASS
    assert [s.n for s in OC.SIZES] == [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, P - 1, P, P + 3, 2 * P + 4 * 256 * 5 + 1]
    assert [r.name for r in OC.REGIMES if r.third_trip] == ["a_typical", "c_first_step"]
    assert all([s.n for s in OC.sizes(r)] == [s.n for s in OC.SIZES][:14 if r.third_trip else 13] for r in OC.REGIMES)


@pytest.mark.parametrize("s", OC.SIZES, ids=lambda s: "n%d" % s.n)
def test_size_reaches_its_trips_and_tail(s):
    assert OC.geometry(s.n) == s
    assert s.grid == min(4096, (s.n // 4 + 1 + 255) // 256)


def test_size_table_covers_the_paths():
    t = OC.SIZES
    assert {s.tail for s in t if s.trips == 0} == {1, 2, 3}, "the tail alone"
    assert {s.tail for s in t if s.trips == 1 and s.grid == 1} == {0, 1, 3}
    assert any(s.grid == 2 and s.last_trip_groups == 1 and s.tail for s in t), "a workgroup other than 0 without a float4, and a tail"
    assert {s.tail for s in t if s.grid == OC.GRID_CAP and s.trips == 1} == {0, 3}
    assert any(s.trips == 3 and 1 < s.last_trip_groups < s.grid and s.tail for s in t), "a last trip that only some workgroups make"
    # the arena of the workload shares its path with the last size: the capped grid, several trips, a partial last one
    arena = OC.geometry(34_900_000 + 1)
    assert arena.grid == OC.GRID_CAP and arena.trips >= 3 and arena.last_trip_groups < arena.grid


@pytest.mark.parametrize("n", [s.n for s in OC.SIZES if s.n <= 1027] + [4 * 256 * 3 + 2])
def test_walk_through_the_loop_visits_every_element_once(n):
    """The loop and the tail as csrc/optim.hip states them, walked thread by thread for the small sizes: every float once."""
    seen = np.zeros(n, dtype=np.int64)
    grid, n4 = OC.grid(n), n >> 2
    most = 0
    for block in range(grid):
        for thread in range(OC.BLOCK):
            i, k = block * OC.BLOCK + thread, 0
            while i < n4:
                seen[4 * i:4 * i + 4] += 1
                i += grid * OC.BLOCK
                k += 1
            most = max(most, k)
            if block == 0 and thread < (n & 3):
                seen[(n4 << 2) + thread] += 1
    assert (seen == 1).all() and most == OC.trips(n)


# ---- operands, reference, bounds -----------------------------------------------------------------------------------------------------
def _normal_or_zero(a):
    a = np.abs(np.asarray(a, dtype=np.float64))
    return bool(((a == 0) | ((a >= MIN_NORMAL) & (a <= MAX_F32))).all())


def _ratios(got, want, bound):
    """worst |got - want| / bound; an element with bound 0 must be exact"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    assert not np.isnan(err).any()
    exact = bound == 0
    assert (err[exact] == 0).all(), "an element with bound 0 is not exact"
    return float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0


@pytest.mark.parametrize("regime", OC.REGIMES, ids=lambda r: r.name)
def test_regime_is_normal_and_both_emulations_are_inside_the_bounds(regime):
    """At ONE_PASS + 3 elements; the operands of every smaller size are a prefix of these (checked below), so the statement holds for
    each of them, and the worst ratio over the first 1027 is printed beside the whole."""
    n = OC.LARGEST
    ops = OC.operands(regime, n)
    assert all(a.dtype == np.float32 and a.shape == (n,) for a in ops)
    assert all(np.shares_memory(a, b) for a, b in zip(OC.operands(regime, 1027), ops)), "a smaller case is not a prefix"
    t, avg, b, avg_b = OC.reference(regime, n)
    lr_t, b1, b2, eps = OC.hyper(regime)
    assert all(_normal_or_zero(R.f32(s)) for s in (lr_t, b1, b2, eps, regime.gscale) + OC.OMDS)
    for name, a in zip("pgmve", ops):
        assert _normal_or_zero(a), "operand %s holds a subnormal or non-finite value" % name
    for name, a in list(t.items()) + [(k, x) for omd in OC.OMDS for k, x in avg[omd].items()]:
        # (the fp32 value of an intermediate lies within a few ulps of the fp64 one: a factor 2 of room on both ends)
        a = np.abs(a)
        assert bool(((a == 0) | ((a >= 2 * MIN_NORMAL) & (a <= MAX_F32 / 2))).all()), "intermediate %s leaves the normal range" % name
    if regime.name == "b_p_zero":
        assert not ops[0].any() and np.array_equal(t["p"], -t["u"]) and np.array_equal(b["p"], b["u"])
    if regime.name == "c_first_step":
        assert not ops[2].any() and not ops[3].any() and regime.t == 1
        ag = np.abs(ops[1])
        assert ag.min() < 1e-14 and ag.max() > 50.0 and (t["root"] < 1e-3 * eps).any() and (t["root"] > 1e6 * eps).any()
    if regime.name == "d_zeros":
        z = OC.zero_mask(n)
        assert 0.3 < z.mean() < 0.37 and z[:4].all()
        for s in OC.SIZES[:13]:
            assert z[max(0, 4 * (s.n // 4) - 4):s.n].all(), "last float4 and tail of n = %d" % s.n
        assert not t["u"][z].any() and not t["m"][z].any() and not t["v"][z].any() and np.array_equal(t["p"][z], ops[0][z].astype(np.float64))
        assert not b["u"][z].any() and (t["u"][~z] != 0).all()
    if regime.name == "f_late_step":
        assert ops[3].max() > 5e7 and np.abs(ops[1]).max() > 5e3 and regime.t == 1000
    small = slice(0, 1027)
    for emu in (R.emulate_every_rounding, R.emulate_fused):
        for omd in OC.OMDS:
            got = emu(*ops, lr_t, b1, b2, eps, regime.gscale, omd)
            want = (t["m"], t["v"], t["u"], t["p"], avg[omd]["e"])
            bound = (b["m"], b["v"], b["u"], b["p"], avg_b[omd])
            whole = [_ratios(x, y, z) for x, y, z in zip(got, want, bound)]
            first = [_ratios(x[small], y[small], z[small]) for x, y, z in zip(got, want, bound)]
            print("optim-bounds %s %s omd %g: worst err / bound  m %.3f  v %.3f  u %.3f  p %.3f  e %.3f   (first 1027: %s)"
                  % (regime.name, emu.__name__, omd, *whole, " ".join("%.3f" % x for x in first)))
            assert max(whole) <= 1.0, (regime.name, emu.__name__, whole)


@pytest.mark.parametrize("b1,b2", OC.OTHER_BETAS)
def test_emulations_are_inside_the_bounds_for_other_betas(b1, b2):
    regime, n = OC.BY_NAME["a_typical"], OC.OTHER_BETAS_N
    ops = OC.operands(regime, n)
    lr_t, third = OC.hyper(regime)[0], 1.0 / 3.0
    assert (R.k_m(b1, third), R.k_v(b2, third)) == ((3, 5) if b1 > 0.5 else (4, 6))
    t = R.adam_terms(*ops, lr_t, b1, b2, OC.ADAM_EPS, third, 0.9)
    b = R.adam_bounds(t, ops[0], ops[4], lr_t, b1, b2, third, 0.9)
    assert all(_normal_or_zero(a) for a in t.values())
    for emu in (R.emulate_every_rounding, R.emulate_fused):
        got = emu(*ops, lr_t, b1, b2, OC.ADAM_EPS, third, 0.9)
        ratios = [_ratios(x, t[q], b[q]) for x, q in zip(got, "mvupe")]
        print("optim-bounds betas (%g, %g) %s: worst err / bound  m %.3f  v %.3f  u %.3f  p %.3f  e %.3f" % (b1, b2, emu.__name__, *ratios))
        assert max(ratios) <= 1.0
    # the two factors of m' exchanged leave the bound (with beta1 = 0.5 they would not)
    swapped = t["m"] - (ops[2].astype(np.float64) * (1.0 - R.f32(b1)) + t["g'"] * R.f32(b1))
    assert (np.abs(swapped) > b["m"]).mean() > 0.99


def test_reference_of_the_case_list_is_adam_ref_and_adam_bounds():
    """OC.reference forms e' and its bound per omd from shared terms; adam_ref / adam_bounds with the average give the same numbers."""
    for regime in (OC.BY_NAME["a_typical"], OC.BY_NAME["e_scale_third"]):
        n = 1027
        ops = OC.operands(regime, n)
        t, avg, b, avg_b = OC.reference(regime, n)
        for omd in OC.OMDS:
            full = R.adam_terms(*ops, *OC.hyper(regime), regime.gscale, omd)
            m, v, u, p, e = R.adam_ref(*ops, *OC.hyper(regime), regime.gscale, omd)
            assert all(np.array_equal(x, y) for x, y in zip((m, v, u, p, e), (t["m"], t["v"], t["u"], t["p"], avg[omd]["e"])))
            fb = R.adam_bounds(full, ops[0], ops[4], OC.hyper(regime)[0], OC.ADAM_B1, OC.ADAM_B2, regime.gscale, omd)
            assert all(np.array_equal(fb[k], b[k]) for k in "mvup")
            assert np.allclose(fb["e"], avg_b[omd], rtol=1e-14, atol=0)


def test_rounding_counts():
    assert (R.U, R.R_SQRT, R.R_DIV, R.EMA_K) == (2.0 ** -24, 2.0, 2.0, 5.0)
    assert (R.k_m(0.5, 1.0), R.k_v(0.9, 1.0)) == (2, 3) and (R.k_m(0.5, 0.125), R.k_v(0.9, 0.125)) == (2, 3)
    third = float(np.float32(1.0 / 3.0))
    assert (R.k_m(0.5, third), R.k_v(0.9, third)) == (3, 5) and (R.k_m(0.25, 1.0), R.k_v(0.3, 1.0)) == (3, 4)
    # 1 - b is exact in fp32 for the project's betas, and 1 - float32(0.9) is not 0.1
    for b in (0.5, 0.9):
        assert float(np.float32(1) - np.float32(b)) == 1.0 - R.f32(b)
    assert abs((1.0 - R.f32(0.9)) / 0.1 - 1.0) > 2e-7
    # where eps is invisible the bound of u is 9.5 U of its magnitude, where it dominates 6 U
    one = np.ones(1, dtype=np.float32)
    for g, k in ((1.0, 9.5), (1e-14, 6.0)):
        a = (0 * one, g * one, 0 * one, 0 * one)
        t = R.adam_terms(*a, None, 1e-4, 0.5, 0.9, 1e-8, 1.0, None)
        bu = R.adam_bounds(t, a[0], None, 1e-4, 0.5, 0.9, 1.0, None)["u"]
        assert abs(float(bu[0] / (R.U * abs(t["u"][0]))) - k) < 1e-4, (g, float(bu[0] / (R.U * abs(t["u"][0]))))


# ---- eps: added to the root, outside the bias correction ------------------------------------------------------------------------------
def test_misplaced_eps_leaves_the_bound_in_regime_c():
    regime = OC.BY_NAME["c_first_step"]
    n = 4 * 256 * 3 + 3
    ops = OC.operands(regime, n)
    lr_t, b1, b2, eps = OC.hyper(regime)
    t, _, b, _ = OC.reference(regime, n)
    ag = np.abs(ops[1].astype(np.float64))
    sep = (ag >= OC.EPS_G_RANGE[0]) & (ag <= OC.EPS_G_RANGE[1])
    assert sep.sum() > n // 10
    e32 = R.f32(eps)
    variants = {"eps inside the root": lambda vn: np.sqrt(vn + e32),
                "eps times sqrt(1 - b2^t)": lambda vn: np.sqrt(vn) + e32 * np.sqrt(1.0 - R.f32(b2) ** regime.t)}
    for name, den_of in variants.items():
        w = R.adam_terms(*ops[:4], None, lr_t, b1, b2, eps, regime.gscale, None, den_of=den_of)
        ratio = np.abs(w["p"] - t["p"]) / b["p"]
        print("optim-bounds %s: |p' - reference| / bound on the %d separating elements: least %.1f, most %.3g; elements outside the "
              "bound overall: %d of %d" % (name, int(sep.sum()), float(ratio[sep].min()), float(ratio[sep].max()), int((ratio > 1).sum()), n))
        assert (ratio[sep] > 1.0).all(), name
        assert np.array_equal(w["m"], t["m"]) and np.array_equal(w["v"], t["v"])


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_adam_ref_known_answers():
    lr, b1, b2, eps = OC.ADAM_LR, OC.ADAM_B1, OC.ADAM_B2, OC.ADAM_EPS
    f = lambda *x: np.array(x, dtype=np.float32)
    # the first step with |g| >> eps moves every weight by lr * sign(g)
    g = f(3.0, -0.25, 1e-3, -40.0)
    p = f(1.0, -1.0, 0.5, 0.0)
    zero = np.zeros(4, dtype=np.float32)
    m, v, u, pn, en = R.adam_ref(p, g, zero, zero, p, R.lr_t(1, lr, b1, b2), b1, b2, eps, 1.0, 0.9)
    # (to 3e-7: lr_t is rounded to fp32, 6e-8, and sqrt(1 - float32(0.9)) is 1.2e-7 above the sqrt(0.1) in lr_t)
    assert np.allclose(u, lr * np.sign(g) * (1 - eps / (np.sqrt(0.1) * np.abs(g))), rtol=3e-7, atol=0)
    assert np.allclose(u[[0, 3]], lr * np.sign(g[[0, 3]]), rtol=3e-7, atol=0)
    assert np.allclose(m, 0.5 * g, rtol=1e-15) and np.allclose(v, (1.0 - R.f32(0.9)) * g.astype(np.float64) ** 2, rtol=1e-15)
    assert np.allclose(pn, p - u, rtol=1e-15) and np.allclose(en, p - 0.9 * (p - pn), rtol=1e-7)
    # g = 0 from zero state moves nothing, and nothing is NaN; with state, m and v decay
    m, v, u, pn, en = R.adam_ref(p, zero, zero, zero, p, 1e-4, b1, b2, eps, 1.0, 1e-3)
    assert not m.any() and not v.any() and not u.any() and np.array_equal(pn, p.astype(np.float64)) and np.array_equal(en, pn)
    m, v, u, pn, _ = R.adam_ref(p, zero, f(1, 2, 3, 4), f(4, 4, 4, 4), None, 1.0, 0.5, 0.25, 0.0, 1.0, None)
    assert m.tolist() == [0.5, 1.0, 1.5, 2.0] and v.tolist() == [1.0] * 4 and u.tolist() == [0.5, 1.0, 1.5, 2.0]
    assert pn.tolist() == [0.5, -2.0, -1.0, -2.0]
    # by hand: m' = 0.5 * 1 + 0.5 * (2 * 0.5) = 1, v' = 0.25 * 4 + 0.75 * 1 = 1.75, u = 2 * 1 / (sqrt(1.75) + 0.5)
    m, v, u, pn, en = R.adam_ref(f(1.0), f(2.0), f(1.0), f(4.0), f(3.0), 2.0, 0.5, 0.25, 0.5, 0.5, 0.5)
    assert (m[0], v[0]) == (1.0, 1.75) and abs(u[0] - 2.0 / (1.75 ** 0.5 + 0.5)) < 1e-15 and abs(en[0] - (3.0 - (3.0 - pn[0]) * 0.5)) < 1e-15
    # the scalars are taken as the kernel receives them
    m, _, _, _, _ = R.adam_ref(f(0.0), f(1.0), f(0.0), f(0.0), None, 1e-4, 0.9, 0.9, eps, 1.0, None)
    assert m[0] == 1.0 - float(np.float32(0.9)) != 0.1
    # torch tensors give the same numbers
    import torch
    a = OC.operands(OC.BY_NAME["a_typical"], 1027)
    h = OC.hyper(OC.BY_NAME["a_typical"])
    want = R.adam_ref(*a, *h, 0.125, 0.9)
    got = R.adam_ref(*(torch.from_numpy(x.copy()) for x in a), *h, 0.125, 0.9)
    assert all(np.allclose(x.numpy(), y, rtol=1e-15, atol=0) for x, y in zip(got, want))      # (the two square roots differ in the last fp64 bit)
    tb = R.adam_bounds(R.adam_terms(*(torch.from_numpy(x.copy()) for x in a), *h, 0.125, 0.9), torch.from_numpy(a[0].copy()),
                       torch.from_numpy(a[4].copy()), h[0], h[1], h[2], 0.125, 0.9)
    nb = R.adam_bounds(R.adam_terms(*a, *h, 0.125, 0.9), a[0], a[4], h[0], h[1], h[2], 0.125, 0.9)
    assert all(np.allclose(tb[k].numpy(), nb[k], rtol=1e-14, atol=0) for k in nb)
