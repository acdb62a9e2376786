"""-m gpu: the persistent convolution kernels beyond one tile per workgroup.

conv_halo3_kernel (csrc/conv_halo.hip), conv_halo3_pc_kernel (csrc/conv_halo_pc.hip) and conv_s2_kernel (csrc/conv_s2.hip) walk the
tiles (bands) of their XCD's range in a loop and carry state from one trip to the next: block coordinates advanced by increments with
carries, the prefetched first patch of the next tile, patch-buffer and register-set parity, the producer / consumer barrier phase,
the accumulators zeroed by the epilogue, dead blocks of a ragged last tile.  Every other kernel-level case of the suite gives a
workgroup at most one tile (tests/test_persistent_plan.py pins that), so this file is where the second trip is checked.

  * Forward: the launch hint cu_cap (operand_format bits 8 .. 13 of sgg_conv2d_nhwc_fwd) shrinks the grid without changing the work
    decomposition - include/sgg_hip.h promises bit-identical results.  With cu_cap = 1 a 75-block problem gives every workgroup 2 to
    5 tiles; with cu_cap = 0 one each (tests/persistent_plan.py).  So y under every cap must EQUAL y without one, bit for bit, tile
    statistics included; y without a cap is checked against fp64 at the bounds of tests/test_kernels_gpu.py (2e-5 of max|ref| in
    mode 2, 1e-4 in mode 3, ONE_PIECE_TOL in mode 1).  Cap 28, the product's value (option g_early_cus), is run for every case.
  * Dgrad: the C ABI has no cap for it, so the shapes are just large enough that some workgroups walk two tiles; against fp64, and
    bit for bit against the same launch over sub-batches small enough for one tile per workgroup.
  * Encoder: every layer of G's trunk at (B = 8, S = 64) with the operand formats, LN fusion and tile statistics the product's plan
    composes, under caps 1, 3, 28 against no cap, bit for bit.
"""
import math

import pytest
import torch

from tests import conv_ref64 as R64
from tests import persistent_plan as PP
from tests.test_kernels_gpu import ONE_PIECE_TOL

pytestmark = pytest.mark.gpu

TOL = {2: 2e-5, 3: 1e-4, **ONE_PIECE_TOL}


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


_DATA = {}


def _data(ref, case, ln):
    """Seeded operands and the fp64 reference of a case, computed once and shared by its variants and modes (CPU tensors, read-only).
    ln: x is a pre-LayerNorm tensor; the reference convolves ELU(LN(x))."""
    key = (case.name, ln)
    if key not in _DATA:
        B, H, W, Ci, Co = case.shape
        k, s = case.k, case.stride
        w, b = rnd((k, k, Ci, Co), 12, 1.0 / math.sqrt(k * k * Ci)), rnd((Co,), 13, 0.1)
        d = {"w": w, "b": b}
        if ln:
            x = rnd((B, H, W, Ci), 31, 2.0) + 0.7
            x[0] *= 3.0                                       # samples with different statistics
            d["gamma"], d["beta"] = 1.0 + rnd((Ci,), 32, 0.3), rnd((Ci,), 33, 0.3)
            a = torch.empty((B, H, W, Ci), dtype=torch.float64)
            ref.ln_elu_fwd(x.double(), d["gamma"].double(), d["beta"].double(), a, torch.empty((B, 2), dtype=torch.float64))
        else:
            x = rnd((B, H, W, Ci), 11)
            a = x.double()
        d["x"] = x
        d["y_ref"] = R64.conv_fwd64(a, w.double(), b.double(), s)
        _DATA[key] = d
    return _DATA[key]


def _first_bad_blocks(a, b, n=6):
    """8x8 output blocks (flat index over [B][H/8][W/8]: two or four consecutive ones form a tile of the 3x3 kernels) where a != b."""
    B, H, W, _ = a.shape
    bad = (a != b).any(dim=3)
    if H % 8 or W % 8:
        return bad.reshape(-1).nonzero().flatten()[:n].tolist()
    blk = bad.view(B, H // 8, 8, W // 8, 8).any(dim=4).any(dim=2).reshape(-1)
    return blk.nonzero().flatten()[:n].tolist()


def _forward_weights(hip, case, wd):
    """(w_fwd, pre-split weights) of the case's layout, as tests/test_kernels_gpu.py prepares them."""
    k = case.k
    Ci, Co = case.shape[3], case.shape[4]
    wf = torch.empty((k, k, Co, Ci), device="cuda")
    hip.hwio_to_hwoi(wd, wf)
    ws = torch.empty((3, wd.numel()), dtype=torch.int16, device="cuda")
    src = wf
    if case.layout == 3:        # conv1_3 over the space-to-depth view: the HWOI transpose of the 9-tap kernel
        w3, src = torch.empty((3, 3, 4 * Ci, Co), device="cuda"), torch.empty((3, 3, Co, 4 * Ci), device="cuda")
        hip.s2d_weights(wd, w3)
        hip.hwio_to_hwoi(w3, src)
    hip.split_weights(src, ws, layout=case.layout)
    return wf, ws


@pytest.mark.parametrize("run", PP.RUNS, ids=["%s-%s-mode%d" % r for r in PP.RUNS])
def test_forward_under_cu_caps_is_bit_identical(hip, ref, run):
    name, variant, mode = run
    case = PP.CASE[name]
    B, H, W, Ci, Co = case.shape
    Ho, Wo = PP.out_hw(case)
    lay, s = case.layout, case.stride
    old = hip.conv_precision
    hip.conv_precision = mode
    try:
        d = _data(ref, case, variant == "ln")
        xd, wd, bd = d["x"].cuda(), d["w"].cuda(), d["b"].cuda()
        wf, ws = _forward_weights(hip, case, wd)
        kw = {}
        if variant == "ln":
            assert hip.ln_prologue_fwd_ok(case.k, s, H, W, Ci, Co)
            gd, btd = d["gamma"].cuda(), d["beta"].cuda()
            st, am = torch.empty((B, 2), device="cuda"), torch.zeros(1, device="cuda")
            hip.ln_elu_fwd(xd, gd, btd, torch.empty_like(xd), st, am)      # the sample statistics and the bound of max|ELU(LN(x))|
            kw = {"amax_x": am, "ln": (st, gd, btd)}
        elif case.x_s16 or variant == "s16":
            assert mode == 2
            am = torch.zeros(1, device="cuda")
            hip.absmax(xd, am)
            x16 = torch.empty_like(xd)
            hip.presplit16(xd, x16, am)
            xd, kw = x16, {"amax_x": am, "x_s16": True}
            if lay == 4 and Co % 128:
                assert hip.conv_wsplit_layout_presplit(case.k, s, H, W, Ci, Co) == 4
        nts = hip.conv_tile_stats_count((B, Ho, Wo, Co), Ci, case.k, s, lay) if variant == "stats" else 0
        assert nts > 0 or variant != "stats"

        def launch(cap):
            y = torch.full((B, Ho, Wo, Co), float("nan"), device="cuda")
            ts = torch.full((B, nts, 4), float("nan"), device="cuda") if nts else None
            hip.conv_fwd(xd, wd, wf, bd, y, s, ws, tile_stats=ts, w_split_layout=lay, cu_cap=cap, **kw)
            return y, ts

        y0, ts0 = launch(0)
        for cap in case.caps + (PP.PRODUCT_CAP,):
            plan = PP.forward_plan(case, cap, variant)
            yc, tsc = launch(cap)
            if not torch.equal(yc, y0):
                blocks = _first_bad_blocks(yc, y0)
                unit = blocks[0] // plan.info.get("nb", 1) if plan.form != "s2" else -1
                raise AssertionError("%s %s mode %d: y under cu_cap %d differs from cu_cap 0 in %d elements (max |d| %.3e); first 8x8 blocks %s; tile %d "
                                     "is trip %s of workgroup %s (tiles per workgroup %s)" %
                                     (name, variant, mode, cap, int((yc != y0).sum()), float((yc - y0).abs().nan_to_num(float("inf")).max()), blocks, unit,
                                      [t for _, t in PP.owner(plan, unit)] if unit >= 0 else "?", [g for g, _ in PP.owner(plan, unit)] if unit >= 0 else "?",
                                      sorted(set(PP.busy(plan)))))
            if nts:
                assert torch.equal(tsc, ts0), "%s %s: tile statistics under cu_cap %d differ from cu_cap 0" % (name, variant, cap)
        y_ref = d["y_ref"]
        h = y0.cpu().double()
        assert torch.isfinite(h).all(), "%s %s: non-finite output without a cap" % (name, variant)
        if nts:
            assert torch.isfinite(ts0).all()
        scale = float(y_ref.abs().max())
        err = float((h - y_ref).abs().max())
        print("%s %s mode %d: err vs fp64 %.3e of max|ref| (bound %.1e)" % (name, variant, mode, err / scale, TOL[mode]))
        assert err <= TOL[mode] * scale, "%s %s mode %d vs fp64: %.3e > %.1e of max|ref|" % (name, variant, mode, err / scale, TOL[mode])
    finally:
        hip.conv_precision = old


_DGRAD = {}


def _dgrad_data(case):
    if case.name not in _DGRAD:
        B, H, W, Ci, Co = case.shape
        k, s = case.k, case.stride
        w, dy = rnd((k, k, Ci, Co), 22, 1.0 / math.sqrt(k * k * Co)), rnd((B, PP.cdiv(H, s), PP.cdiv(W, s), Co), 14)
        _DGRAD[case.name] = {"w": w, "dy": dy, "dx_ref": R64.conv_dgrad64(dy.double(), w.double(), (H, W), s)}
    return _DGRAD[case.name]


@pytest.mark.parametrize("run", PP.DGRAD_RUNS, ids=["%s-mode%d" % r for r in PP.DGRAD_RUNS])
def test_dgrad_with_two_tiles_per_workgroup(hip, run):
    """sgg_conv2d_nhwc_dgrad takes no cap: shapes whose plan gives some workgroups two tiles (tests/test_persistent_plan.py).

    Against fp64 at the bounds of tests/test_kernels_gpu.py.  In mode 2 that check is blind to one kind of carry: the epilogue
    multiplies the accumulators by 2^-(ea + eb), the inverse of the operands' fp16 scales (about 2^-26 here), so a value left in them
    from the previous tile arrives in the next output at 1e-8 of its size - below fp32 resolution of most elements, far below any
    tolerance.  Hence also EXACTLY against the same launch over sub-batches that give each workgroup one tile at most (same amax
    words, hence the same pieces, products and summation order per block), and in mode 3, which has no such scaling."""
    name, mode = run
    case = PP.DGRAD_CASE[name]
    B, H, W, Ci, Co = case.shape
    k, s, lay = case.k, case.stride, case.layout
    assert max(PP.dgrad_plan(case).per_wg) >= 2 and max(PP.dgrad_plan(case, case.chunk).per_wg) <= 1
    old = hip.conv_precision
    hip.conv_precision = mode
    try:
        want = hip.conv_wsplit_layout_presplit(k, s, H, W, Co, Ci) if case.dy_s16 else hip.conv_wsplit_layout(k, s, H, W, Co, Ci)
        assert want == lay, (want, lay)
        d = _dgrad_data(case)
        wd, dyd = d["w"].cuda(), d["dy"].cuda()
        am = torch.zeros(2, device="cuda")
        hip.absmax(dyd, am[0:1])
        hip.absmax(wd, am[1:2])
        ws = torch.empty((2, wd.numel()), dtype=torch.int16, device="cuda")
        hip.split_weights(wd, ws, am[1:2], layout=lay)
        kw = {"amax_dy": am[0:1], "amax_w": am[1:2], "w_split_layout": lay}
        if case.dy_s16:
            dy16 = torch.empty_like(dyd)
            hip.presplit16(dyd, dy16, am[0:1])
            dyd, kw["dy_s16"] = dy16, True
        dx = torch.full((B, H, W, Ci), float("nan"), device="cuda")
        hip.conv_dgrad(dyd, wd, dx, s, ws, **kw)
        assert torch.isfinite(dx).all(), "dgrad %s: non-finite output" % name
        for b0 in range(0, B, case.chunk):
            b1 = min(B, b0 + case.chunk)
            sub = torch.full((b1 - b0, H, W, Ci), float("nan"), device="cuda")
            hip.conv_dgrad(dyd[b0:b1], wd, sub, s, ws, **kw)
            if not torch.equal(dx[b0:b1], sub):
                ne = dx[b0:b1] != sub
                raise AssertionError("dgrad %s mode %d: samples %d..%d differ from the one-tile-per-workgroup launch in %d elements (max |d| %.3e); "
                                     "first 8x8 blocks (flat) %s" % (name, mode, b0, b1 - 1, int(ne.sum()),
                                                                     float((dx[b0:b1] - sub).abs().nan_to_num(float("inf")).max()),
                                                                     [b0 * (H // 8) * (W // 8) + i for i in _first_bad_blocks(dx[b0:b1], sub)]))
        dx_ref = d["dx_ref"]
        scale = float(dx_ref.abs().max())
        err = float((dx.cpu().double() - dx_ref).abs().max())
        print("dgrad %s mode %d: err vs fp64 %.3e of max|ref| (bound %.1e)" % (name, mode, err / scale, TOL[mode]))
        assert err <= TOL[mode] * scale, "dgrad %s mode %d vs fp64: %.3e > %.1e of max|ref|" % (name, mode, err / scale, TOL[mode])
    finally:
        hip.conv_precision = old


def test_encoder_forward_under_cu_caps_is_bit_identical(hip):
    """G's trunk at (B = 8, S = 64, V = 50): conv1_2 alone has 512 blocks, 8 tiles per workgroup under cap 1.  Both kinds of pass
    (followed by a backward or not: different LN fusion), every layer's output and the features, bit for bit against no cap."""
    import sgg_amd  # noqa: F401
    from oracle import sgg_oracle as O
    from sgg_amd.step import GanStep
    B, S, V = 8, 64, 50
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp)
    images = O.synth_batch(B, S, V)[0].cuda()
    T = gs.G.trunk
    assert any(lay["ws_layout"] in (1, 4) for lay in T.layers) and any(lay["ws_layout"] in (2, 3) for lay in T.layers)
    for fb in (True, False):
        got = {}
        for c in (0, 1, 3, 28):
            feat = T.forward(images, for_backward=fb, cu_cap=c).clone()
            torch.cuda.synchronize()
            got[c] = [lay["y"].clone() for lay in T.layers] + [feat]
        assert all(torch.isfinite(t).all() for t in got[0])
        for c in (1, 3, 28):
            bad = [j for j, (a, b) in enumerate(zip(got[c], got[0])) if not torch.equal(a, b)]
            assert not bad, "for_backward=%s, cu_cap %d: outputs of layers %s (index %d = features) differ from cu_cap 0" % (fb, c, bad, len(T.layers))
