"""How the persistent convolution kernels cut their work: a Python restatement of the launchers' grid sizing (test infrastructure).

The 3x3 halo-resident kernel, its producer / consumer forms and the band-resident 5x5 stride-2 kernel are persistent: XCD k of the 8
owns a contiguous eighth of the work units - M-tiles of NB 8x8 blocks, or bands of 224 output positions - and its `gx` workgroups
walk that range with `for (unit = begin; unit < end; unit += tstride)`.  This module mirrors, line by line,

  * csrc/conv_halo.hip     sgg_halo_route (NB = 2; N % 128 / N % 64 / N % 32 tilings on 4 / 4 / 2 waves,
                           slots = cus * 8 / (WGM * WGN)) and the range arithmetic at the head of conv_halo3_kernel;
  * csrc/conv_halo_pc.hip  sgg_halo_pc_route (two blocks x 128 columns, or four blocks x 64 columns where N % 128 != 0; slots = cus)
                           and the head of conv_halo3_pc_kernel;
  * csrc/conv_s2.hip       sgg_s2_route (`wide`, `small_` / ksplit, slots = (wide ? 1 : 2) * cus, ntn = (N / bn) * ksplit) and the
                           head of conv_s2_kernel;
  * csrc/conv_halo.h       sgg_persist_gx (workgroups per XCD from units, ntn and slots: _walk below), sgg_persist_cus (cu_cap
                           1 .. 31 caps the CUs of an XCD, anything else means all 32);
  * csrc/conv_gather.hip   sgg_conv2d_nhwc_fwd / _dgrad for the unit counts (nblk = B * H/8 * W/8; M = B * Ho * Wo; the dgrad swaps
                           C and N and never passes a cap).

A change to any of them needs the same change here: tests/test_persistent_plan.py pins which cases of the suite walk more than one
unit per workgroup, and tests/test_persistent_tiles_gpu.py relies on it to know that its cases do.

CASES is the table of forward cases of tests/test_persistent_tiles_gpu.py, DGRAD_CASES the uncapped dgrad shapes, RUNS the
(case, variant, mode) launches that file makes.
"""
from collections import namedtuple

XCDS = 8
CUS_PER_XCD = 32          # SGG_PERSIST_CUS_PER_XCD
S2_BAND = 224
S2_SMALL_ITEMS = 256


def cdiv(a, b):
    return -(-a // b)


def persist_cus(cu_cap):
    return cu_cap if 0 < cu_cap < CUS_PER_XCD else CUS_PER_XCD


# units: M-tiles or bands; ntn: (n-tile [, channel half]) pairs per unit; gx: workgroups per XCD; tstride: units between two trips of a
# workgroup; ranges: (begin, end) of each XCD; per_wg: units walked by workgroup id 0 .. 8 * gx - 1 (id & 7 = XCD, as the hardware deals
# them); info: what else the launcher decided (nb, bn, wide, ksplit)
Plan = namedtuple("Plan", "form units ntn gx tstride ranges per_wg info")


def _walk(form, units, ntn, slots, info):
    per_xcd = cdiv(units, XCDS) * ntn
    gx = min(per_xcd, slots)
    gx = cdiv(gx, ntn) * ntn
    tstride = gx // ntn
    ranges = [((k * units) >> 3, ((k + 1) * units) >> 3) for k in range(XCDS)]
    per_wg = []
    for wg in range(XCDS * gx):
        xcd, jx = wg & 7, wg >> 3
        begin, end = ranges[xcd][0] + jx // ntn, ranges[xcd][1]
        per_wg.append(max(0, cdiv(end - begin, tstride)))
    return Plan(form, units, ntn, gx, tstride, ranges, per_wg, info)


def halo_plan(nblk, N, cu_cap=0):
    """sgg_halo_route (launches without frag16): conv_halo3_kernel<2, BN, WGM, WGN>."""
    bn, waves = (128, 4) if N % 128 == 0 else ((64, 4) if N % 64 == 0 else (32, 2))
    return _walk("halo", cdiv(nblk, 2), N // bn, persist_cus(cu_cap) * 8 // waves, {"nb": 2, "bn": bn})


def pc_plan(nblk, N, cu_cap=0):
    """sgg_halo_pc_route: two-block tiles of 128 columns, four-block tiles of 64 columns where N % 128 != 0."""
    nb = 4 if N % 128 != 0 else 2
    bn = 256 // nb
    return _walk("pc%d" % nb, cdiv(nblk, nb), N // bn, persist_cus(cu_cap), {"nb": nb, "bn": bn})


def s2_plan(M, N, C, cu_cap=0, presplit=False, stats=False, ln=False):
    """sgg_s2_route in the two-piece fp16 mode (precision 2; presplit only exists there): M = B * Ho * Wo output positions (dgrad:
    positions of dy), N output columns, C contraction channels."""
    nbands = cdiv(M, S2_BAND)
    dmap = presplit and not ln
    wide = dmap and N % 256 == 0 and nbands * (N // 256) > S2_SMALL_ITEMS // 2
    bn = 256 if wide else 128
    small = not wide and not stats and not ln and nbands * (N // bn) <= S2_SMALL_ITEMS
    ksplit = 2 if (small and (C >> 4) % 4 == 0) else 1
    return _walk("s2", nbands, (N // bn) * ksplit, (1 if wide else 2) * persist_cus(cu_cap), {"bn": bn, "wide": wide, "ksplit": ksplit})


def owner(plan, unit):
    """(workgroup id, trip) of the workgroups that compute `unit` (one per n-tile / channel half): for mapping a wrong output tile
    back to the loop iteration that produced it."""
    out = []
    for wg in range(XCDS * plan.gx):
        xcd, jx = wg & 7, wg >> 3
        begin, end = plan.ranges[xcd][0] + jx // plan.ntn, plan.ranges[xcd][1]
        if begin <= unit < end and (unit - begin) % plan.tstride == 0:
            out.append((wg, (unit - begin) // plan.tstride))
    return out


def busy(plan):
    """Units walked by the workgroups that have any."""
    return [t for t in plan.per_wg if t > 0]


def ragged(plan):
    return len(set(busy(plan))) > 1


# ---- the cases of tests/test_persistent_tiles_gpu.py -----------------------------------------------------------------------------
# shape: x (B, H, W, Cin) and Cout, NHWC; layout: w_split_layout of the launch (1 four-wave 3x3, 4 producer / consumer 3x3, 3 conv1_3
# through the space-to-depth view, 2 band-resident 5x5 stride 2); x_s16: the case only exists with a pre-split x; caps: the caps that
# make its workgroups walk several units (cap 28, the product's value, is run on top of these for every case); expect: units per
# busy workgroup under each cap, where the table of the issue states them.
Case = namedtuple("Case", "name shape k stride layout x_s16 caps expect")

CASES = [
    Case("halo32_onechunk", (6, 40, 48, 32, 32), 3, 1, 1, False, (1, 2), {1: {2, 3}, 2: {1, 2}}),      # bw = 6: advance (1 row, 2 columns), column carry
    Case("halo32_multichunk", (6, 40, 48, 64, 32), 3, 1, 1, False, (1, 2), {1: {2, 3}, 2: {1, 2}}),
    Case("halo64_c32", (5, 40, 24, 32, 64), 3, 1, 1, False, (1, 2), {1: {2, 3}, 2: {1, 2}}),
    Case("halo64_c64", (5, 40, 24, 64, 64), 3, 1, 1, False, (1, 2), {1: {2, 3}, 2: {1, 2}}),
    Case("halo128_c32", (5, 40, 24, 32, 128), 3, 1, 1, False, (1, 2), {1: {2, 3}, 2: {1, 2}}),          # not producer / consumer eligible
    Case("halo128_fourwave", (5, 40, 24, 64, 128), 3, 1, 1, False, (1, 2), {1: {2, 3}, 2: {1, 2}}),     # eligible, kept on the four-wave kernel
    Case("pc2", (5, 40, 24, 64, 128), 3, 1, 4, False, (1, 2, 3), {1: {4, 5}, 2: {2, 3}, 3: {1, 2}}),
    Case("pc2_two_ntiles", (5, 24, 24, 128, 256), 3, 1, 4, False, (1, 3), {1: {2, 3}, 3: {1, 2}}),
    Case("pc4_presplit", (7, 40, 24, 64, 64), 3, 1, 4, True, (1, 2), {1: {3, 4}, 2: {1, 2}}),          # 105 blocks: three dead blocks in the last tile
    Case("s2d_conv1_3", (6, 80, 96, 32, 32), 5, 2, 3, False, (1,), {1: {2, 3}}),                        # view (6, 40, 48, 128) -> 32
    Case("s2", (24, 112, 112, 32, 128), 5, 2, 2, False, (1, 2), {1: {21}, 2: {10, 11}}),
    # (9, 56, 56, 64, 256) has 32 bands: the launcher splits the channel chunks (ksplit 2) and every workgroup walks 4 (cap 1) or 2 (cap 3)
    # bands - not ragged; with B = 10 there are 35 bands, 4 or 5 per XCD
    Case("s2_two_ntiles", (10, 56, 56, 64, 256), 5, 2, 2, False, (1, 3), {1: {4, 5}, 3: {2, 3}}),
    # eight-wave workgroups of 256 columns: pre-split x, more than 128 (band, 256-column) items - at 28 x 28 outputs from B = 37 on (130 bands)
    Case("s2_wide", (37, 56, 56, 64, 256), 5, 2, 2, True, (1,), {1: {16, 17}}),
]
CASE = {c.name: c for c in CASES}
PRODUCT_CAP = 28          # DEFAULT_OPTIONS["g_early_cus"]


def out_hw(case):
    B, H, W, Ci, Co = case.shape
    return cdiv(H, case.stride), cdiv(W, case.stride)


def forward_plan(case, cu_cap, variant="plain"):
    """Plan of the forward launch of `case` in precision 2 / 3; variant: plain, stats, ln (LN prologue), s16 (pre-split x)."""
    B, H, W, Ci, Co = case.shape
    Ho, Wo = out_hw(case)
    if case.layout in (1, 3):
        return halo_plan(B * (Ho // 8) * (Wo // 8), Co, cu_cap)
    if case.layout == 4:
        return pc_plan(B * (H // 8) * (W // 8), Co, cu_cap)
    return s2_plan(B * Ho * Wo, Co, Ci, cu_cap, presplit=case.x_s16 or variant == "s16", stats=variant == "stats", ln=variant == "ln")


# (case, variant, precision mode) of every forward test: each case plain in mode 2; the variants on the smallest case of a form that
# has them; modes 3 and 1 (other template instantiations of the same loops) on one case each
RUNS = [(c.name, "plain", 2) for c in CASES] + [
    ("halo32_onechunk", "stats", 2), ("halo64_c64", "stats", 2), ("halo128_fourwave", "stats", 2), ("pc2", "stats", 2), ("pc4_presplit", "stats", 2),
    ("s2d_conv1_3", "stats", 2), ("s2", "stats", 2),
    ("halo32_onechunk", "ln", 2), ("halo64_c64", "ln", 2), ("pc2", "ln", 2), ("s2_two_ntiles", "ln", 2), ("s2d_conv1_3", "ln", 2),
    ("halo64_c64", "s16", 2), ("pc2", "s16", 2), ("s2_two_ntiles", "s16", 2),
    ("halo64_c64", "plain", 3), ("halo64_c64", "plain", 1), ("halo64_c32", "plain", 1), ("pc2", "plain", 3), ("pc2", "ln", 3),
    ("s2_two_ntiles", "plain", 3), ("s2_two_ntiles", "ln", 3),
]

# ---- dgrad: no cap in the C ABI, so the shapes are large enough that some workgroups walk two units -------------------------------
# shape (B, H, W, Cin, Cout) of the LAYER: the launch contracts over Cout and produces N = Cin columns
# chunk: samples per sub-batch of the exact comparison - the same launch over `chunk` samples at a time gives every workgroup at most
# one unit and, since a block's (band's) products and their order do not depend on how the units are dealt out, the same bits.  (An even
# number of samples of the 28 x 28 grid is a whole number of bands: 2 * 784 = 7 * 224.)
DgradCase = namedtuple("DgradCase", "name shape k stride layout dy_s16 chunk")
DGRAD_CASES = [
    DgradCase("halo32", (3, 224, 224, 32, 32), 3, 1, 1, False, 1),          # 1176 tiles, 147 per XCD on 128 workgroups
    DgradCase("halo64", (6, 112, 112, 64, 64), 3, 1, 1, False, 3),          # 588 tiles, 73 / 74 per XCD on 64
    DgradCase("pc2", (9, 64, 64, 128, 64), 3, 1, 4, False, 4),              # N = Cin = 128: 288 tiles, 36 per XCD on 32
    DgradCase("pc4_presplit", (17, 64, 64, 64, 64), 3, 1, 4, True, 8),      # 272 four-block tiles, 34 per XCD on 32
    # more than 512 bands (8 XCDs x 64 slots) at Cin = 128, Cout = 32: B * Ho * Wo > 114 688; on the 28 x 28 grid (bands cross images in
    # the middle of a row, ragged last band) that is B = 147: 515 bands, 64 / 65 per XCD
    DgradCase("s2", (147, 56, 56, 128, 32), 5, 2, 2, False, 80),
]
DGRAD_CASE = {c.name: c for c in DGRAD_CASES}
# (case, precision mode): mode 2 everywhere; mode 3 where the form has it (the four-block form is precision 2 only) - without the fp16
# scaling a value carried from one tile into the next arrives at full size, so there the fp64 check alone sees it
DGRAD_RUNS = [(c.name, 2) for c in DGRAD_CASES] + [("halo32", 3), ("halo64", 3), ("pc2", 3), ("s2", 3)]


def dgrad_plan(case, samples=None):
    """Plan of the dgrad launch of `case`, or of the same launch over `samples` samples."""
    B, H, W, Ci, Co = case.shape
    B = B if samples is None else samples
    Ho, Wo = cdiv(H, case.stride), cdiv(W, case.stride)
    if case.layout == 1:
        return halo_plan(B * (H // 8) * (W // 8), Ci, 0)
    if case.layout == 4:
        return pc_plan(B * (H // 8) * (W // 8), Ci, 0)
    return s2_plan(B * Ho * Wo, Ci, Co, 0, presplit=case.dy_s16)
