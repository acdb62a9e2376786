"""CPU: which cases of the suite make a persistent convolution workgroup walk more than one tile (tests/persistent_plan.py).

The state a persistent workgroup carries from one tile to the next - block coordinates advanced by increments, the prefetched first
patch of the next tile, buffer and register-set parity, the producer / consumer barrier phase, the zeroed accumulators, dead blocks of
a ragged last tile - is only exercised where the launch plan gives a workgroup at least two tiles.  These tests state, from the
launch rules alone, that

  * every forward case of tests/test_persistent_tiles_gpu.py does so under its caps, and that without a cap it gives each workgroup
    at most ONE tile - the bitwise comparison of that file is "several tiles per workgroup" against "one tile per workgroup";
  * its dgrad shapes (no cap exists for the dgrad) do so uncapped, and the sub-batches they are compared with bit for bit do not;
  * the kernel-level cases of tests/test_kernels_gpu.py and the B = 2 layer shapes of tests/test_fullsize_conv_gpu.py do NOT: they
    check one trip of the loop.  If someone enlarges those, the last test of this file says which comment can change.

What is asserted per (case, cap): some workgroup walks at least two units, and the units per workgroup are the sets the case table
states.  Per case: under at least one of its caps some workgroup walks three or more units AND the workgroups differ in their
number of trips (a ragged walk: both parities of the one-chunk kernel's paired loop, a last trip that some workgroups do not make).
The caps 2 and 3 of the table give {1, 2} units - two, not three - and cap 1 of the 336-band stride-2 case gives 21 to every workgroup,
so "three or more, and ragged" cannot hold for every single cap; it holds for every case.
"""
import pytest

from tests import persistent_plan as PP


def _id(run):
    return "%s-%s-mode%d" % run


@pytest.mark.parametrize("run", PP.RUNS, ids=_id)
def test_forward_cases_walk_several_tiles_under_their_caps(run):
    name, variant, mode = run
    case = PP.CASE[name]
    deep = False
    for cap in case.caps:
        plan = PP.forward_plan(case, cap, variant)
        busy = PP.busy(plan)
        assert max(busy) >= 2, (name, variant, cap, sorted(set(busy)))
        deep |= max(busy) >= 3 and PP.ragged(plan)
    assert deep, "%s (%s): no cap gives a ragged walk of three or more tiles" % (name, variant)


@pytest.mark.parametrize("case", PP.CASES, ids=[c.name for c in PP.CASES])
def test_forward_case_table_values(case):
    """The units per workgroup the table states for each cap (plain launches)."""
    for cap, want in case.expect.items():
        assert set(PP.busy(PP.forward_plan(case, cap))) == want, (case.name, cap)
    assert set(case.expect) == set(case.caps)


@pytest.mark.parametrize("run", PP.RUNS, ids=_id)
def test_forward_cases_uncapped_are_one_tile_per_workgroup(run):
    name, variant, _ = run
    for cap in (0, PP.PRODUCT_CAP, 32):
        assert max(PP.forward_plan(PP.CASE[name], cap, variant).per_wg) <= 1, (name, variant, cap)


def test_forward_cases_take_the_kernel_forms_they_name():
    info = lambda name, variant="plain": PP.forward_plan(PP.CASE[name], 1, variant).info
    assert PP.forward_plan(PP.CASE["pc2"], 1).form == "pc2" and PP.forward_plan(PP.CASE["pc4_presplit"], 1).form == "pc4"
    assert PP.forward_plan(PP.CASE["pc2_two_ntiles"], 1).ntn == 2
    assert info("s2") == {"bn": 128, "wide": False, "ksplit": 1}
    assert info("s2_two_ntiles") == {"bn": 128, "wide": False, "ksplit": 2}                # few items: channel chunks split
    assert info("s2_two_ntiles", "s16") == {"bn": 128, "wide": False, "ksplit": 2}         # 35 (band, 256-column) items: not wide
    assert info("s2_two_ntiles", "ln") == {"bn": 128, "wide": False, "ksplit": 1}          # the prologue is not split
    assert info("s2_wide") == {"bn": 256, "wide": True, "ksplit": 1}
    # the smallest batch of that shape which is wide, and the smallest of the two-n-tile shape whose split walk is ragged
    B, H, W, Ci, Co = PP.CASE["s2_wide"].shape
    assert not PP.s2_plan((B - 1) * (H // 2) * (W // 2), Co, Ci, 1, presplit=True).info["wide"]
    B, H, W, Ci, Co = PP.CASE["s2_two_ntiles"].shape
    assert not PP.ragged(PP.s2_plan((B - 1) * (H // 2) * (W // 2), Co, Ci, 1)) and not PP.ragged(PP.s2_plan((B - 1) * (H // 2) * (W // 2), Co, Ci, 3))
    # the last tile of the four-block case has dead blocks, the 32-column case advances by (1 row, 2 columns) of its 6-column block grid
    B, H, W, Ci, Co = PP.CASE["pc4_presplit"].shape
    assert (B * (H // 8) * (W // 8)) % 4 == 1
    p = PP.forward_plan(PP.CASE["halo32_onechunk"], 1)
    assert (p.tstride * 2) // 6 == 1 and (p.tstride * 2) % 6 == 2


@pytest.mark.parametrize("case", PP.DGRAD_CASES, ids=[c.name for c in PP.DGRAD_CASES])
def test_dgrad_cases_walk_two_tiles_uncapped(case):
    plan = PP.dgrad_plan(case)
    assert max(plan.per_wg) >= 2 and PP.ragged(plan), (case.name, sorted(set(plan.per_wg)))
    assert min(plan.per_wg) >= 1
    # the sub-batches of the exact comparison: one unit per workgroup at most, the same kernel variant (tile form, channel split), and
    # for the band kernel sub-batches that start on a band boundary
    B, H, W, Ci, Co = case.shape
    for n in {case.chunk, B % case.chunk or case.chunk}:
        sub = PP.dgrad_plan(case, n)
        assert max(sub.per_wg) <= 1 and sub.info == plan.info and sub.form == plan.form, (case.name, n)
    if case.layout == 2:
        assert (case.chunk * (H // 2) * (W // 2)) % PP.S2_BAND == 0


def test_dgrad_case_details():
    p = PP.dgrad_plan(PP.DGRAD_CASES[0])
    assert p.units == 1176 and p.gx == 128 and {e - b for b, e in p.ranges} == {147}
    s2 = [c for c in PP.DGRAD_CASES if c.name == "s2"][0]
    B, H, W, Ci, Co = s2.shape
    assert PP.dgrad_plan(s2).units > 512 and (B - 1) * (H // 2) * (W // 2) <= 512 * PP.S2_BAND      # the smallest such batch


def test_encoder_level_conv1_2_walks_eight_tiles_under_cap_1():
    """GanStep(B = 8, S = 64): conv1_2 has 8 * 8 * 8 = 512 blocks = 256 tiles, 32 per XCD on 4 two-wave workgroups."""
    plan = PP.halo_plan(8 * 8 * 8, 32, 1)
    assert set(plan.per_wg) == {8} and plan.gx == 4
    assert set(PP.halo_plan(8 * 8 * 8, 32, 3).per_wg) == {2, 3}
    assert max(PP.halo_plan(8 * 8 * 8, 32, 0).per_wg) == 1 and max(PP.halo_plan(8 * 8 * 8, 32, PP.PRODUCT_CAP).per_wg) == 1


def test_owner_inverts_the_walk():
    for plan in (PP.forward_plan(PP.CASE["halo32_onechunk"], 1), PP.forward_plan(PP.CASE["pc2_two_ntiles"], 3), PP.forward_plan(PP.CASE["s2_two_ntiles"], 3)):
        trips = [0] * (PP.XCDS * plan.gx)
        for unit in range(plan.units):
            own = PP.owner(plan, unit)
            assert len(own) == plan.ntn, (plan.form, unit, own)
            for wg, _ in own:
                trips[wg] += 1
        assert trips == plan.per_wg


def test_the_kernel_level_cases_elsewhere_stay_at_one_tile_per_workgroup():
    """HALO_CASES, S2_CASES (tests/test_kernels_gpu.py) and the conv1_2 shape of test_configs1_layer_shapes_b2
    (tests/test_fullsize_conv_gpu.py) plan to at most one tile (band) per workgroup in both directions.  If this fails because one of
    them was enlarged, its comment may say "several tiles per workgroup" again - and this pin moves."""
    from tests.test_kernels_gpu import HALO_CASES, S2_CASES
    for B, H, W, Ci, Co in HALO_CASES:
        nblk = B * (H // 8) * (W // 8)
        plans = [PP.halo_plan(nblk, Co), PP.halo_plan(nblk, Ci)]                                      # forward, dgrad (N = Cin)
        plans += [PP.pc_plan(nblk, n) for n, c in ((Co, Ci), (Ci, Co)) if n % 128 == 0 and c % 64 == 0]
        assert max(max(p.per_wg) for p in plans) <= 1, (B, H, W, Ci, Co)
    assert max(PP.halo_plan(75, 32).per_wg) == 1 and PP.halo_plan(75, 32).units == 38               # "(5, 40, 24, 32, 32): 75 blocks"
    for B, H, Ci, Co in S2_CASES:
        M = B * (H // 2) * (H // 2)
        plans = [PP.s2_plan(M, Co, Ci, stats=st, ln=ln) for st in (False, True) for ln in (False, True)]
        if Ci % 128 == 0:
            plans.append(PP.s2_plan(M, Ci, Co))
        assert max(max(p.per_wg) for p in plans) <= 1, (B, H, Ci, Co)
    assert PP.s2_plan(24 * 56 * 56, 128, 32).units == 336 and PP.s2_plan(24 * 56 * 56, 128, 32).gx == 42   # 42 bands per XCD on 64 slots
    # conv1_2 at B = 2, 224 x 224: 1568 blocks = 784 tiles, 98 per XCD against 128 two-wave workgroups - the largest B = 2 layer
    p = PP.halo_plan(2 * 28 * 28, 32)
    assert p.units == 784 and p.gx == 98 and max(p.per_wg) == 1
    from tests.test_fullsize_conv_gpu import LAYERS
    for name, H, Ci, Co, k, s in LAYERS:
        if k == 3:
            nblk = 2 * (H // 8) * (H // 8)
            plans = [PP.halo_plan(nblk, Co), PP.halo_plan(nblk, Ci)] + [PP.pc_plan(nblk, n) for n in (Co, Ci) if n % 128 == 0]
        elif Ci == 32 and Co == 32:
            nblk = 2 * (H // 16) * (H // 16)
            plans = [PP.halo_plan(nblk, 32), PP.halo_plan(nblk, 128)]                                 # space-to-depth view: dgrad has 128 columns
        else:
            M = 2 * (H // 2) * (H // 2)
            plans = [PP.s2_plan(M, Co, Ci), PP.s2_plan(M, Ci, Co)]
        assert max(max(p.per_wg) for p in plans) <= 1, name
