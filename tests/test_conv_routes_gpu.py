"""-m gpu: every convolution kernel instance the library can route a launch to, run once against fp64 - the cases of
tests/conv_route_cases.py, whose closure over the routing tables tests/test_conv_routes_cpu.py proves without a GPU.

Each case is launched through the C ABI with exactly its scalars (the route query must name the case's kernels first), on seeded
Gaussian operands, into NaN-filled outputs; pre-split operands are made by sgg_presplit16 against their sgg_absmax words; an LN
prologue gets its statistics from sgg_layernorm_hwc_finalize over tile partials (as test_layernorm_prologue_fwd_wgrad does) and is
compared with the convolution of ELU(LN(y)) in fp64 (tests/conv_ref64.py).

Error metric: max|hip - ref| / max|ref| - per tap slice dw[kh, kw] for filter gradients (a wrong tap-parity class of a 5x5 stride-2
launch cannot hide under the other three), per tensor for y and dx.  Bounds: those of tests/test_kernels_gpu.py for the same
arithmetic (CONV_TOL: 2e-5 in precisions 0, 2, 6; 1e-4 in 3; ONE_PIECE_TOL in 1 and 4; the per-tap filter-gradient kernels run 1 / 4 as
2 / 3 and are held to those).  A filter gradient runs in a workspace of exactly the reported bytes with a canary behind it; tile
statistics, where the case asks for them, must give the LayerNorm statistics of the kernel's own y."""
import functools
import math

import pytest
import torch

from tests import conv_ref64 as R64
from tests import conv_route_cases as RC
from tests.test_kernels_gpu import CONV_TOL, ONE_PIECE_TOL, close, dev, rnd

pytestmark = pytest.mark.gpu

CANARY = 4096


def _ln_params(C):
    return 1.0 + rnd((C,), 32, 0.3), rnd((C,), 33, 0.3)


@functools.lru_cache(maxsize=4)
def _pre_ln(shape):
    """(y0, ELU(LN(y0)) in fp64, tile partials [B, 4, 4]): the producing layer's pre-LayerNorm output, samples with different statistics."""
    from oracle.kernels_ref import RefKernels
    B, H, W, C = shape
    y0 = rnd(shape, 31, 2.0) + 0.7
    y0[0] *= 3.0
    gamma, beta = _ln_params(C)
    a_ref = torch.empty(shape, dtype=torch.float64)
    RefKernels().ln_elu_fwd(y0.double(), gamma.double(), beta.double(), a_ref, torch.empty((B, 2), dtype=torch.float64))
    flat = y0.reshape(B, 4, -1).double()
    ts = torch.empty((B, 4, 4), dtype=torch.float64)
    ts[:, :, 0] = flat.shape[2]
    ts[:, :, 1] = flat.mean(dim=2)
    ts[:, :, 2] = ((flat - flat.mean(dim=2, keepdim=True)) ** 2).sum(dim=2)
    ts[:, :, 3] = (flat - flat.mean(dim=2, keepdim=True)).abs().amax(dim=2)
    return y0, a_ref, ts.float()


def _ln_prologue(hip, shape, precision):
    """Device operands of an LN prologue: (y0, (stats, gamma, beta), amax word of ELU(LN(y0)) as the finalize publishes it)."""
    y0, _, ts = _pre_ln(shape)
    gamma, beta = (dev(t) for t in _ln_params(shape[3]))
    stats = torch.full((shape[0], 2), float("nan"), device="cuda")
    am = torch.zeros(1, device="cuda")
    hip.ln_finalize(dev(ts), gamma, beta, stats, am if precision == 2 else None, shape[1] * shape[2])
    return dev(y0), (stats, gamma, beta), am


def _source(hip, t, presplit):
    """(device tensor - pre-split in place where asked -, its amax word)."""
    d = dev(t)
    am = torch.zeros(1, device="cuda")
    hip.absmax(d, am)
    if presplit:
        hip.presplit16(d, d, am)
    return d, am


@functools.lru_cache(maxsize=2)
def _wgrad_operands(shape, ln):
    """(x | pre-LN y0, dy, dw in fp64) of a filter-gradient shape: shared by the precisions and formats that run on it."""
    B, H, W, Ci, Co, k, s = shape
    Ho, Wo = RC.same_pads(H, k, s)[0], RC.same_pads(W, k, s)[0]
    dy = rnd((B, Ho, Wo, Co), 6)
    if ln:
        x, a_ref, _ = _pre_ln((B, H, W, Ci))
    else:
        x = rnd((B, H, W, Ci), 5)
        a_ref = x.double()
    return x, dy, R64.conv_wgrad64(a_ref, dy.double(), k, s)


def _wgrad_id(case):
    return "%s-p%d-a%d-ln%d-f%d" % ("x".join(map(str, case[:7])), *case[7:11])


@pytest.mark.parametrize("case", RC.WGRAD_CASES, ids=_wgrad_id)
def test_filter_gradient_kernels_against_fp64(hip, case):
    from sgg_amd.lib import _p
    shape, (precision, algo, ln, fmt), symbols = case[:7], case[7:11], case[11]
    B, H, W, Ci, Co, k, s = shape
    L, dims = hip.lib, RC.conv_dims(*shape)
    got, need = RC.wgrad_query(L, case)
    assert got == symbols
    x, dy, dw_ref = _wgrad_operands(shape, ln)
    if ln:
        assert not fmt & 1
        xd, (ln_s, ln_g, ln_b), am_x = _ln_prologue(hip, (B, H, W, Ci), precision)
    else:
        (xd, am_x), ln_s, ln_g, ln_b = _source(hip, x, fmt & 1), None, None, None
    dyd, am_dy = _source(hip, dy, fmt & 2)
    ws = torch.empty(need + CANARY, dtype=torch.uint8, device="cuda")
    ws[:need] = 0xff             # (NaN patterns where a slab is not written)
    ws[need:] = 0x5a
    dw = torch.full((k, k, Ci, Co), float("nan"), device="cuda")
    rc = L.sgg_conv2d_nhwc_wgrad(_p(xd), _p(dyd), _p(dw), *dims, precision, algo, _p(am_x), _p(am_dy), _p(ln_s), _p(ln_g), _p(ln_b), fmt,
                                 _p(ws), need, hip._stream())
    assert rc == 0, L.sgg_last_error()
    per_tap = symbols.startswith(("conv_wgrad_kernel", "conv_wgrad_tr_kernel"))
    tol = CONV_TOL[{1: 2, 4: 3}[precision] if per_tap and precision in ONE_PIECE_TOL else precision]
    h = dw.cpu().double()
    assert bool(torch.isfinite(h).all()), "NaN left in dw: %d elements" % int((~torch.isfinite(h)).sum())
    assert bool((ws[need:] == 0x5a).all()), "the launch wrote past the workspace it reported"
    errs = ((h - dw_ref).abs().amax(dim=(2, 3)) / dw_ref.abs().amax(dim=(2, 3)))
    worst = int(errs.argmax())
    print("%s: worst tap (%d, %d) err %.3e, tol %.3e, workspace %d" % (symbols.split(";")[0], worst // k, worst % k, float(errs.max()), tol, need))
    assert float(errs.max()) <= tol, "tap (%d, %d): %.3e > %.3e; per tap:\n%s" % (worst // k, worst % k, float(errs.max()), tol, errs)


def _weights(hip, case, w, am_w):
    """(the launch's f32 weight operand, its pre-split copy in the case's layout or None)."""
    direction, precision, layout, k = case[:4]
    Ci, Co, has_split = case[8], case[9], case[10]
    wd = dev(w)
    if Ci == 3:
        return wd, None
    hip.absmax(wd, am_w)
    wf = torch.empty((k, k, Co, Ci), device="cuda")
    hip.hwio_to_hwoi(wd, wf)
    launch = wf if direction == "fwd" else wd
    if not has_split:
        return launch, None
    src = launch
    if layout == 3:      # conv1_3 over the space-to-depth view: the 9-tap kernel (its HWOI transpose for the forward)
        src = torch.empty((3, 3, 4 * Ci, Co), device="cuda")
        hip.s2d_weights(wd, src)
        if direction == "fwd":
            w3 = src
            src = torch.empty((3, 3, Co, 4 * Ci), device="cuda")
            hip.hwio_to_hwoi(w3, src)
    ws = torch.zeros((3, w.numel()), dtype=torch.int16, device="cuda")
    old = hip.conv_precision
    hip.conv_precision = precision
    try:
        hip.split_weights(src, ws, am_w, layout)
    finally:
        hip.conv_precision = old
    return launch, ws


@functools.lru_cache(maxsize=2)
def _fd_operands(direction, shape, ln):
    """(x | y0 | dy, w, bias, reference in fp64) of a forward / dgrad shape."""
    B, H, W, Ci, Co, k, s = shape
    Ho, Wo = RC.same_pads(H, k, s)[0], RC.same_pads(W, k, s)[0]
    w, b = rnd((k, k, Ci, Co), 12, 1.0 / math.sqrt(k * k * Ci)), rnd((Co,), 13, 0.1)
    if direction == "dgrad":
        dy = rnd((B, Ho, Wo, Co), 14)
        return dy, w, b, R64.conv_dgrad64(dy.double(), w.double(), (H, W), s)
    if ln:
        x, a_ref, _ = _pre_ln((B, H, W, Ci))
    else:
        x = rnd((B, H, W, Ci), 11)
        a_ref = x.double()
    return x, w, b, R64.conv_fwd64(a_ref, w.double(), b.double(), s)


def _fd_id(case):
    return "%s-p%d-l%d-%s-ws%d-ts%d-ln%d-f%d" % (case[0], case[1], case[2], "x".join(map(str, case[5:10] + case[3:5])), *case[10:14])


@pytest.mark.parametrize("case", RC.FWD_DGRAD_CASES, ids=_fd_id)
def test_forward_and_dgrad_kernels_against_fp64(hip, case):
    from sgg_amd.lib import _p
    direction, precision, layout, k, s, B, H, W, Ci, Co, has_split, has_stats, ln, fmt, symbol = case
    L, dims = hip.lib, RC.conv_dims(B, H, W, Ci, Co, k, s)
    Ho, Wo = dims[4], dims[5]
    assert RC.fwd_dgrad_query(L, case) == symbol
    src, w, b, ref64 = _fd_operands(direction, (B, H, W, Ci, Co, k, s), ln)
    am_w = torch.zeros(1, device="cuda")
    wl, ws = _weights(hip, case, w, am_w)
    tol = CONV_TOL[precision]
    if direction == "dgrad":
        dyd, am_dy = _source(hip, src, fmt & 1)
        out = torch.full((B, H, W, Ci), float("nan"), device="cuda")
        rc = L.sgg_conv2d_nhwc_dgrad(_p(dyd), _p(wl), _p(ws), _p(out), *dims, precision, layout, _p(am_dy), _p(am_w), fmt, hip._stream())
        assert rc == 0, L.sgg_last_error()
        close(out, ref64, rtol=tol, atol=0.0, what="%s dx" % symbol)
        return
    if ln:
        assert not fmt & 1
        xd, (ln_s, ln_g, ln_b), am_x = _ln_prologue(hip, (B, H, W, Ci), precision)
    else:
        (xd, am_x), ln_s, ln_g, ln_b = _source(hip, src, fmt & 1), None, None, None
    ts = None
    if has_stats:
        nts = L.sgg_conv2d_nhwc_fwd_tile_stats(Ho, Wo, Ci, Co, k, k, s, precision, layout)
        assert nts > 0
        ts = torch.full((B, nts, 4), float("nan"), device="cuda")
    y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
    rc = L.sgg_conv2d_nhwc_fwd(_p(xd), _p(wl), _p(ws), _p(dev(b)), _p(y), *dims, precision, layout, _p(am_x), _p(am_w), _p(ts), _p(ln_s), _p(ln_g),
                               _p(ln_b), fmt, hip._stream())
    assert rc == 0, L.sgg_last_error()
    close(y, ref64, rtol=tol, atol=0.0, what="%s y" % symbol)
    if ts is not None:       # the epilogue's partials give the LayerNorm statistics of the kernel's own y
        assert bool(torch.isfinite(ts).all()), "NaN left in the tile statistics"
        assert abs(float(ts[:, :, 0].double().sum()) - y.numel()) < 0.5
        gamma, beta = dev(1.0 + rnd((Co,), 15, 0.2)), dev(rnd((Co,), 16, 0.2))
        a1, a2 = torch.empty_like(y), torch.empty_like(y)
        st1, st2 = torch.empty((B, 2), device="cuda"), torch.empty((B, 2), device="cuda")
        hip.ln_elu_fwd(y, gamma, beta, a1, st1, tile_stats=ts)
        hip.ln_elu_fwd(y, gamma, beta, a2, st2)
        close(st1, st2.cpu(), rtol=1e-6, what="%s: statistics from the epilogue vs statistics pass" % symbol)
        close(a1, a2.cpu(), rtol=1e-6, what="%s: LN output" % symbol)
