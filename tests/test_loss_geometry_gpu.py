"""-m gpu: the loss, fill and pooling kernels (csrc/misc.hip: fill, absmax, onehot, interpolate, gp_fwd, gp_bwd, wgan_losses,
argmax_rows; csrc/head.hip: the spatial means) at the launch geometry of the batch-64 step, through HipKernels, against fp64.

The cases are those of tests/loss_cases.py (why each one exists is said there and checked without a GPU by
tests/test_loss_cases_cpu.py); the references and the error bounds are those of tests/loss_ref.py.  Every bound is per element or
per row and counts fp32 roundings; every output lies between NaN guards that must stay untouched.  Each comparison prints
"loss-geometry <kernel> <case>: max err, bound" (profiles/loss_geometry_pytest_gpu.log is the -s output of one run).
"""
import math

import numpy as np
import pytest
import torch

from oracle import np_loops as NL
from oracle import sgg_oracle as O
from tests import loss_cases as LC
from tests import loss_ref as LR

pytestmark = pytest.mark.gpu

PAD = 64                        # guard elements on both sides of a flat output (a multiple of 4: the payload keeps its alignment)
GUARD_BITS = 0x7FC0DEAD         # a NaN that no kernel produces and no test writes
NAN, INF = float("nan"), float("inf")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed), dtype=torch.float32) * scale


def dev(t):
    return t.cuda().contiguous()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def guarded(shape, pad):
    """(buffer, view): a buffer of guard NaNs with pad[i] guard elements on both sides of dimension i, and the view of `shape` inside."""
    buf = torch.full([s + 2 * p for s, p in zip(shape, pad)], GUARD_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
    view = buf
    for i, (s, p) in enumerate(zip(shape, pad)):
        view = view.narrow(i, p, s)
    return buf, view


def flat_guarded(*shape):
    """a contiguous tensor of `shape` between two guards of PAD elements"""
    n = int(np.prod(shape))
    buf, view = guarded((n,), (PAD,))
    return buf, view.view(*shape)


def untouched(buf, view, what, nan_ok=False):
    """Nothing but `view` was written in `buf`; the view holds no NaN (nan_ok: no guard NaN)."""
    torch.cuda.synchronize()
    n_guard = int((bits(buf) == GUARD_BITS).sum())
    inside = int((bits(view) == GUARD_BITS).sum())
    assert inside == 0, "%s: %d elements of the target were not written" % (what, inside)
    assert n_guard == buf.numel() - view.numel(), "%s: %d guard elements were written" % (what, buf.numel() - view.numel() - n_guard)
    assert nan_ok or not torch.isnan(view).any(), what + ": NaN inside the target"


def within(what, got, ref, bound):
    """|got - ref| <= bound for every element (bound: a number or a tensor of ref's shape); prints the largest error and its bound."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not torch.isnan(got).any(), what + ": NaN"
    err = (got - ref).abs().reshape(-1)
    bnd = (bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))).double().expand_as(ref).reshape(-1)
    k = int(torch.argmax(err - bnd))
    print("loss-geometry %s: max err %.3e (bound there %.3e), largest err / bound %.3g" %
          (what, float(err.max()), float(bnd[int(torch.argmax(err))]), float((err / bnd.clamp_min(1e-300)).max())))
    assert bool((err <= bnd).all()), "%s: element %d: err %.3e > bound %.3e (ref %.6e)" % (what, k, float(err[k]), float(bnd[k]),
                                                                                            float(ref.reshape(-1)[k]))


# ---- fill --------------------------------------------------------------------------------------------------------------------------
FILL_VALUE = {"0.0": 0.0, "-1/192": -1.0 / 192, "-0.0": -0.0, "nan": NAN}


@pytest.mark.parametrize("c", LC.FILL_CASES, ids=lambda c: "n%d_off%d" % (c.n, c.offset))
def test_fill_writes_the_value_and_nothing_else(hip, c):
    """Bit patterns: 0.0, the cotangent -1 / (B * T) of the critic's mean, -0.0 and a NaN, on the scalar path, the 16-byte path, its
    1..3-element tail launch and the scalar fallback for a start one float behind a 16-byte boundary."""
    for name in LC.FILL_VALUES:
        value = FILL_VALUE[name]
        buf = torch.full((PAD + c.offset + c.n + PAD,), GUARD_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        view = buf[PAD + c.offset:PAD + c.offset + c.n]
        assert view.data_ptr() % 16 == 4 * c.offset and view.is_contiguous()
        hip.fill(view, value)
        untouched(buf, view, "fill %s n %d" % (name, c.n), nan_ok=True)
        want = int(np.float32(value).view(np.int32))
        wrong = int((bits(view) != want).sum())
        assert wrong == 0, "fill %s n %d: %d elements differ from the value's bit pattern" % (name, c.n, wrong)
    print("loss-geometry fill n %d offset %d (%s): exact" % (c.n, c.offset, c.path))


# ---- absmax ------------------------------------------------------------------------------------------------------------------------
def amax_word(prev):
    buf, word = guarded((1,), (PAD,))
    word.fill_(prev)
    return buf, word


@pytest.mark.parametrize("c", LC.ABSMAX_CASES, ids=lambda c: "n%d" % c.n)
def test_absmax_is_exact(hip, c):
    """max |x| of negative-valued maxima in the last (tail) element, the first one and the interior; a larger word already there
    survives, a smaller one is replaced.  A maximum has no rounding: the comparison is exact."""
    base = torch.rand((c.n,), generator=gen(300 + c.n % 97), dtype=torch.float32) * 2.0 - 1.0
    for where in sorted({c.n - 1, 0, c.n // 2}):
        x = base.clone()
        x[where] = -3.75
        xd = dev(x)
        for prev, want in ((0.0, 3.75), (5.0, 5.0), (0.25, 3.75)):
            assert want == LR.absmax(x, prev)
            buf, word = amax_word(prev)
            hip.absmax(xd, word)
            untouched(buf, word, "absmax n %d" % c.n)
            assert float(word) == want, "absmax n %d, maximum at %d, word before %.2f: got %r" % (c.n, where, prev, float(word))
    print("loss-geometry absmax n %d (grid %d, trips %d, tail %d): exact" % (c.n, c.grid, c.trips, c.tail))


def test_absmax_drops_nan(hip):
    """What the code does with a NaN beside finite values: fmaxf returns its other operand, so the NaN is dropped and the word is the
    maximum of the finite elements (in the float4 body, in the tail, and for an input of NaNs only: the word stays)."""
    n = 1027
    x = torch.rand((n,), generator=gen(310), dtype=torch.float32)
    x[0] = x[5] = x[6] = x[7] = x[600] = x[n - 1] = x[n - 3] = NAN
    x[4], x[n - 2] = -2.5, -2.0
    for t, prev, want in ((x, 0.0, 2.5), (x[n - 3:].clone(), 0.0, 2.0), (torch.full((9,), NAN), 0.5, 0.5)):
        assert LR.absmax(t, prev) == want
        buf, word = amax_word(prev)
        hip.absmax(dev(t), word)
        untouched(buf, word, "absmax with NaN")
        assert float(word) == want


# ---- onehot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.ONEHOT_CASES, ids=lambda c: "V%d" % c.V)
def test_onehot_rows(hip, c):
    """192 rows from a [B, T] label tensor; a label equal to V and a negative one give all-zero rows (tf.one_hot)."""
    labels = torch.randint(0, c.V, (c.B, c.T), generator=gen(320 + c.V))
    labels[0, 0], labels[1, 2], labels[2, 1], labels[3, 0], labels[c.B - 1, c.T - 1] = c.V, -1, c.V - 1, 0, c.V - 1
    buf, out = flat_guarded(c.B, c.T, c.V)
    hip.onehot(labels.cuda(), out)
    untouched(buf, out, "onehot V %d" % c.V)
    want = LR.onehot(labels, c.V)
    assert float(want[0, 0].sum()) == 0.0 and float(want[1, 2].sum()) == 0.0 and float(want.sum()) == c.B * c.T - 2
    assert torch.equal(out.cpu().double(), want)
    print("loss-geometry onehot V %d (trips %d): exact" % (c.V, c.trips))


# ---- interpolate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LC.INTERP_CASES, ids=lambda c: "n%d" % c.n)
@pytest.mark.parametrize("real_kind", ["dense", "onehot"])
def test_interpolate_per_element(hip, c, real_kind):
    """x_hat = real + alpha (fake - real) with alpha = 0 (real, bit for bit), 1 and values between; real dense, and one-hot rows as
    in the step."""
    T, V = 3, c.n // 3
    if real_kind == "dense":
        real = rnd((c.B, T, V), 330 + V)
    else:
        real = LR.onehot(torch.randint(0, V, (c.B, T), generator=gen(331 + V)), V).float()
    fake = rnd((c.B, T, V), 332 + V, 3.0)
    alpha = torch.tensor([0.0, 1.0, 0.3, 0.77, 0.999], dtype=torch.float32)[:c.B]
    buf, out = flat_guarded(c.B, T, V)
    hip.interpolate(dev(real), dev(fake), dev(alpha), out)
    untouched(buf, out, "interpolate n %d" % c.n)
    within("interpolate %s n %d (grid %d, second trip %s)" % (real_kind, c.n, c.grid, c.second_grid_trip), out,
           LR.interpolate(real, fake, alpha), LR.interpolate_bound(real, fake, alpha))
    assert torch.equal(bits(out[0]).cpu(), bits(real[0])), "alpha = 0 does not give real bit for bit"


# ---- gradient penalty --------------------------------------------------------------------------------------------------------------
_gp = {}


def gp_case(B, n):
    """(g, fp64 slopes, fp64 pens): rows with slopes well below 1 (0.3, 0.05), well above (3, 40), an all-zero row and a row whose only
    nonzero is its last element; once per shape."""
    if (B, n) not in _gp:
        g = torch.zeros((B, n), dtype=torch.float32)
        for b in range(B):
            kind = b % 6
            if kind == 2:
                continue
            if kind == 3:
                g[b, n - 1] = 2.5
                continue
            g[b] = rnd((n,), 340 + 7 * n + b) * ({0: 0.3, 1: 3.0, 4: 40.0, 5: 0.05}[kind] / math.sqrt(n))
        slopes, pen = LR.gp_fwd(g)
        bound = LR.slope_rel_bound(n) * slopes
        assert bool(((slopes - 1.0).abs() > 10 * bound).all()), "a row's slope lies within 10 bounds of 1"
        _gp[(B, n)] = (g, slopes, pen)
    return _gp[(B, n)]


@pytest.mark.parametrize("c", LC.GP_CASES, ids=lambda c: "n%d" % c.n)
def test_gp_fwd_per_row(hip, c):
    """Slopes relative per row.  pen = max(slope - 1, 0) CANCELS, so it is held to its row's slope bound as an ABSOLUTE bound (a
    relative one on pen would ask for digits the fp32 slope does not have), and it is 0.0 exactly wherever the slope is below 1."""
    g, slopes, pen = gp_case(c.B, c.n)
    bs, sl = flat_guarded(c.B)
    bp, pn = flat_guarded(c.B)
    hip.gp_fwd(dev(g).view(c.B, 3, c.n // 3) if c.n % 3 == 0 else dev(g), sl, pn)
    untouched(bs, sl, "slopes"), untouched(bp, pn, "pen")
    bound = LR.slope_rel_bound(c.n) * slopes
    what = "n %d (trips %d, waves %d)" % (c.n, c.trips, c.waves_with_data)
    within("gp_fwd slopes " + what, sl, slopes, bound)
    within("gp_fwd pen " + what, pn, pen, bound)
    below = slopes < 1.0
    assert int(below.sum()) >= 3 and bool((pn.cpu()[below] == 0.0).all()), "pen is not exactly 0 under a slope below 1"
    assert bool((pn.cpu()[~below] > 0.0).all())
    assert float(slopes[2]) == math.sqrt(1e-10) and float(pn[2]) == 0.0, "the all-zero row"


@pytest.mark.parametrize("c", LC.GP_BWD_CASES, ids=lambda c: "B%d_n%d" % (c.B, c.n))
def test_gp_bwd_per_element(hip, c):
    """Fed with the reference's slopes and pens rounded to fp32: the error is the kernel's own, five roundings per element (+ one
    subnormal step should a product underflow).  Rows without a penalty are exact zeros."""
    g, slopes, pen = gp_case(c.B, c.n)
    s32, p32 = slopes.float(), pen.float()
    ref = LR.gp_bwd(g, s32, p32, 10.0)
    buf, v = flat_guarded(c.B, c.n)
    hip.gp_bwd(dev(g), dev(s32), dev(p32), v, 10.0)
    untouched(buf, v, "gp_bwd")
    within("gp_bwd B %d n %d (grid %d, second trip %s)" % (c.B, c.n, c.grid, c.second_grid_trip), v, ref,
           LR.GP_BWD_REL * ref.abs() + 2.0 ** -149)
    zero = p32 == 0.0
    assert int(zero.sum()) >= 3 and bool((v.cpu()[zero] == 0.0).all()), "a row with pen == 0 is not exactly zero"
    assert bool((v.cpu()[~zero].abs().sum(dim=1) > 0.0).all())


# ---- wgan_losses -------------------------------------------------------------------------------------------------------------------
def wgan_inputs(B, T, late_only):
    d = 16.0 + rnd((2 * B, T), 350 + B)
    pen = torch.clamp(rnd((B,), 351 + B, 1.5), min=0.0)
    if late_only:       # everything a lane of wave 0 reads is zero: waves 1..3 carry the whole result
        d.view(2, B * T)[:, :LC.WAVE] = 0.0
        pen[:LC.WAVE] = 0.0
    return d, pen


def check_wgan(hip, B, T, form, late_only, what):
    d, pen = wgan_inputs(B, T, late_only)
    has_real = form != "generator"
    if not has_real:
        d = d[:B].clone()
    p = pen if form == "real+pen" else None
    ref = LR.wgan_losses(d, p, 10.0, B, T, has_real)
    buf, out = flat_guarded(4)
    hip.wgan_losses(dev(d), None if p is None else dev(p), 10.0, B, T, has_real, out)
    untouched(buf, out, what)
    within(what, out, ref, torch.tensor(LR.wgan_bounds(d, p, 10.0, B, T, has_real), dtype=torch.float64))
    o = out.cpu()
    if form == "generator":
        assert torch.equal(bits(o[1:2]), bits(o[3:4])) and float(o[2]) == 0.0 and float(o[0]) == float(o[3]), "the generator form"
    if form == "real":
        assert float(o[2]) == 0.0 and float(o[0]) == float(o[1])
    if form == "real+pen":
        assert float(ref[2]) > 0.1 or late_only and B <= LC.WAVE


@pytest.mark.parametrize("form", LC.WGAN_FORMS)
@pytest.mark.parametrize("c", LC.WGAN_CASES, ids=lambda c: "B%d_T%d" % (c.B, c.T))
def test_wgan_losses_forms(hip, c, form):
    """Critic outputs N(16, 1) (tests/tolerances.py): mean(fake) - mean(real) cancels, so the bounds are absolute and stated on the
    means' magnitude, not on the difference."""
    check_wgan(hip, c.B, c.T, form, False, "wgan_losses B %d T %d %s (waves %d, trips %d, pen trips %d)" %
               (c.B, c.T, form, c.waves_with_data, c.trips, c.pen_trips))


@pytest.mark.parametrize("form", LC.WGAN_FORMS)
@pytest.mark.parametrize("B,T", [(64, 3), (300, 1)])
def test_wgan_losses_from_waves_1_to_3_only(hip, B, T, form):
    """Only elements with i >= 64 are nonzero: a block sum that loses waves 1..3 gives zeros."""
    check_wgan(hip, B, T, form, True, "wgan_losses B %d T %d %s, i >= 64 only" % (B, T, form))


# ---- argmax_rows -------------------------------------------------------------------------------------------------------------------
def argmax_input(c):
    """x [rows, V] and {row: token the construction decides}.  Row r takes kind (r + V + rows) % 12."""
    V = c.V
    x = rnd((c.rows, V), 360 + V + c.rows)
    want = {}
    for r in range(c.rows):
        kind = (r + V + c.rows) % 12
        if kind == 1:                                   # a tie inside one lane: index 0 and its next trip (V <= 64: two lanes)
            a, b = (0, 64) if V > 64 else (3, 40)
            x[r, a] = x[r, b] = 100.0
            want[r] = a
        elif kind == 2 and V > 70:                      # lane 6's second trip against lane 3's first
            x[r, 70] = x[r, 3] = 50.0
            want[r] = 3
        elif kind == 3 and V > 64:                      # a LATER trip of a low lane against the first trip of a higher one:
            a, b = (3 + 64 * 5, 5) if V > 323 else (64, 7)   # only argmax_merge's index comparison makes the first index win
            x[r, a] = x[r, b] = 75.0
            want[r] = b
        elif kind == 4:
            x[r] = 0.25
            want[r] = 0
        elif kind == 5:
            x[r] = -INF
            want[r] = 0
        elif kind == 6:
            x[r, V - 1] = 9.0
            want[r] = V - 1
        elif kind == 7:                                 # NaNs beside numbers are never selected
            x[r, 0] = x[r, V // 2] = x[r, V - 1] = NAN
            x[r, 11] = 9.0
            want[r] = 11
        elif kind == 8:                                 # no non-NaN entry
            x[r] = NAN
            want[r] = 0
        elif kind == 9:                                 # the non-NaN maximum is -inf: its first index, not the NaN in front of it
            x[r] = -INF
            x[r, 0] = NAN
            want[r] = 1
        elif kind == 10:
            x[r, ::3] = NAN
            x[r, V - 1] = INF
            x[r, 1] = INF if V > 64 else x[r, 1]
            want[r] = 1 if V > 64 else V - 1
    return x, want


@pytest.mark.parametrize("c", LC.ARGMAX_CASES, ids=lambda c: "R%d_V%d_pad%d" % (c.rows, c.V, c.pad))
def test_argmax_rows_exact(hip, c):
    """The first index of the maximum over the non-NaN entries, 0 for a row without one, always in [0, V): against
    oracle.sgg_oracle.argmax_tokens, the plain loop of oracle/np_loops.py and the tokens the constructions decide.  pad: the rows are a
    column slice of a wider buffer whose padding is +inf (a read past V would win)."""
    x, want = argmax_input(c)
    wide = torch.full((c.rows, c.V + c.pad), INF, device="cuda")
    xv = wide[:, :c.V]
    xv.copy_(x)
    assert xv.is_contiguous() == (c.pad == 0 or c.rows == 1)
    buf = torch.full((PAD + c.rows + PAD,), -5, dtype=torch.int64, device="cuda")
    out = buf[PAD:PAD + c.rows]
    hip.argmax_rows(xv, out)
    torch.cuda.synchronize()
    assert bool((buf[:PAD] == -5).all()) and bool((buf[PAD + c.rows:] == -5).all()), "written outside the tokens"
    got = out.cpu()
    assert bool(((got >= 0) & (got < c.V)).all()), "a token outside [0, V)"
    ref = O.argmax_tokens(x)
    assert ref.tolist() == NL.argmax_first(x.numpy()).tolist()
    for r, k in want.items():
        assert int(ref[r]) == k, "row %d (kind %d): the oracle gives %d, the construction %d" % (r, (r + c.V + c.rows) % 12, int(ref[r]), k)
    bad = (got != ref).nonzero().reshape(-1).tolist()
    assert not bad, "rows %s (kinds %s): got %s, want %s" % (bad[:8], [(r + c.V + c.rows) % 12 for r in bad[:8]], got[bad[:8]].tolist(),
                                                            ref[bad[:8]].tolist())
    print("loss-geometry argmax_rows rows %d V %d ld %d (trips %d, idle waves %d): exact" % (c.rows, c.V, c.V + c.pad, c.trips, c.idle_waves))


# ---- spatial means -----------------------------------------------------------------------------------------------------------------
SM_IDS = ["B%d_P%d_L%d_C%d" % (c.B, c.npass, c.L, c.C) for c in LC.SM_CASES]
SM_COLS = 160                   # guard columns of the strided operands (more than the 128 channels of a forward workgroup)


def device_ctx(ctx):
    """ctx on the device with NaNs behind its last element (a read past channel C of the last row comes back as NaN)"""
    flat = torch.full((ctx.numel() + 256,), NAN, device="cuda")
    flat[:ctx.numel()].copy_(ctx.reshape(-1))
    return flat[:ctx.numel()].view(ctx.shape)


@pytest.mark.parametrize("c", LC.SM_CASES, ids=SM_IDS)
def test_spatial_mean_fwd_per_element(hip, c):
    """c0 = h0 = mean over L, into column slices of wider buffers as the step does (XH[:, ind:]); rows r and r + B are the same bits."""
    R = c.B * c.npass
    ctx = rnd((c.B, c.L, c.C), 370 + c.L)
    bc, oc = guarded((R, c.C), (1, SM_COLS))
    bh, oh = guarded((R, c.C), (2, SM_COLS + 4))
    hip.spatial_mean_fwd(device_ctx(ctx), oc, oh)
    untouched(bc, oc, "c0"), untouched(bh, oh, "h0")
    ref, bound = LR.spatial_mean_fwd(ctx, R), LR.sm_fwd_bound(ctx).repeat(c.npass, 1)
    within("spatial_mean_fwd %s (empty groups %d, ragged %s, c guard %s)" % (SM_IDS[LC.SM_CASES.index(c)], c.empty_groups,
                                                                             c.ragged_groups, c.c_guard), oc, ref, bound)
    assert torch.equal(bits(oc), bits(oh)), "c0 and h0 differ"
    for p in range(1, c.npass):
        assert torch.equal(bits(oc[:c.B]), bits(oc[p * c.B:(p + 1) * c.B])), "rows r and r + B differ"


@pytest.mark.parametrize("accumulate", [True, False], ids=["accumulate", "overwrite"])
@pytest.mark.parametrize("c", LC.SM_CASES, ids=SM_IDS)
def test_spatial_mean_bwd_per_element(hip, c, accumulate):
    """dctx (+)= (1 / L) sum over the passes of (dc0 + dh0); overwrite mode starts from a dctx of NaNs and must leave none."""
    R, shape = c.B * c.npass, (c.B, c.L, c.C)
    dc0, dh0 = rnd((R, c.C), 380 + c.L), rnd((R, c.C), 381 + c.L)
    dctx0 = rnd(shape, 382 + c.L) if accumulate else None
    _, dc = guarded((R, c.C), (0, SM_COLS))
    _, dh = guarded((R, c.C), (0, 8))
    dc.copy_(dc0), dh.copy_(dh0)
    buf, d = flat_guarded(*shape)
    d.copy_(dctx0) if accumulate else d.fill_(NAN)
    hip.spatial_mean_bwd(dc, dh, d, accumulate)
    untouched(buf, d, "dctx")
    within("spatial_mean_bwd %s %s (gy %d, y trips %d, ragged %s)" % (SM_IDS[LC.SM_CASES.index(c)], "accumulate" if accumulate else
                                                                      "overwrite", c.gy, c.y_trips, c.ragged_y), d,
           LR.spatial_mean_bwd(dc0, dh0, dctx0, shape), LR.sm_bwd_bound(dc0, dh0, dctx0, shape))


# ---- the wrappers refuse views they would read wrongly -------------------------------------------------------------------------------
def test_wrappers_refuse_non_contiguous_tensors(hip):
    """onehot, interpolate, gp_fwd, gp_bwd and wgan_losses pass raw pointers: a transposed view raises instead of computing on the
    wrong elements (and nothing is written)."""
    B, T, V = 4, 3, 8
    tr = lambda *s: torch.zeros(tuple(reversed(s)), device="cuda").t() if len(s) == 2 else torch.zeros((s[0], s[2], s[1]), device="cuda").transpose(1, 2)
    ok = lambda *s: torch.zeros(s, device="cuda")
    lab = torch.zeros((B, T), dtype=torch.int64, device="cuda")
    assert not tr(B, V).is_contiguous() and not tr(B, T, V).is_contiguous() and tr(B, T, V).shape == (B, T, V)
    calls = [
        lambda: hip.onehot(lab, tr(B, T, V)),
        lambda: hip.onehot(torch.zeros((T, B), dtype=torch.int64, device="cuda").t(), ok(B, T, V)),
        lambda: hip.interpolate(tr(B, T, V), ok(B, T, V), ok(B), ok(B, T, V)),
        lambda: hip.interpolate(ok(B, T, V), tr(B, T, V), ok(B), ok(B, T, V)),
        lambda: hip.interpolate(ok(B, T, V), ok(B, T, V), ok(B), tr(B, T, V)),
        lambda: hip.gp_fwd(tr(B, T, V), ok(B), ok(B)),
        lambda: hip.gp_bwd(tr(B, T, V), ok(B), ok(B), ok(B, T, V), 10.0),
        lambda: hip.gp_bwd(ok(B, T, V), ok(B), ok(B), tr(B, T, V), 10.0),
        lambda: hip.gp_bwd(ok(B, T, V), ok(2 * B)[::2], ok(B), ok(B, T, V), 10.0),
        lambda: hip.wgan_losses(tr(2 * B, T), ok(B), 10.0, B, T, True, ok(4)),
        lambda: hip.wgan_losses(ok(2 * B, T), ok(2 * B)[::2], 10.0, B, T, True, ok(4)),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("call %d went through" % i)
    # the same calls on contiguous tensors go through
    hip.onehot(lab, ok(B, T, V))
    hip.interpolate(ok(B, T, V), ok(B, T, V), ok(B), ok(B, T, V))
    hip.gp_fwd(ok(B, T, V), ok(B), ok(B))
    hip.gp_bwd(ok(B, T, V), ok(B) + 1.0, ok(B), ok(B, T, V), 10.0)
    hip.wgan_losses(ok(2 * B, T), ok(B), 10.0, B, T, True, ok(4))
    torch.cuda.synchronize()
