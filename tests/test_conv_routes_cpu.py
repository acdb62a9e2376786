"""CPU: the closure of the convolution GPU cases (tests/conv_route_cases.py, run against fp64 by tests/test_conv_routes_gpu.py) over
every kernel instance the routing tables know.  The library's own queries (sgg_conv2d_nhwc_wgrad_symbol, _fwd_symbol, _dgrad_symbol: the
launch's validation and route, no GPU) name the kernels of every case; their union must be

  * the 137 filter-gradient kernels that make up the symbol strings of tests/golden/wgrad_routes.json, and
  * the 78 forward / dgrad symbols of tests/golden/conv_symbols.json

(tests/test_wgrad_route_cpu.py and tests/test_conv_route_cpu.py pin those tables against the library).  A kernel the library can route
a launch to and that no case runs against fp64 fails here; so does a case taken out of the lists (their lengths are pinned)."""
import json
import os

import sgg_amd  # noqa: F401
from sgg_amd import build, lib

from tests import conv_route_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _library():
    return lib.load_library(build.build())


def _table_kernels():
    wgrad = {k for s in json.load(open(os.path.join(GOLDEN, "wgrad_routes.json")))["symbols"] for k in s.split(";")}
    fd = set(json.load(open(os.path.join(GOLDEN, "conv_symbols.json")))["symbols"])
    return wgrad, fd


def test_every_case_reaches_the_kernels_it_is_named_for():
    L = _library()
    assert RC.same_pads(13, 5, 2) == lib.same_pads(13, 5, 2) and RC.same_pads(16, 3, 1) == lib.same_pads(16, 3, 1)
    for case in RC.WGRAD_CASES:
        symbols, need = RC.wgrad_query(L, case)
        assert symbols == case[11], (case[:11], symbols)
        assert symbols.count(";") == (3 if case[6] == 2 else 0)       # (every stride-2 case runs on the resident kernels: four tap classes)
        assert need % 16 == 0 and need <= L.sgg_conv2d_nhwc_wgrad_workspace_bytes(*RC.conv_dims(*case[:7])[:9])
    for case in RC.FWD_DGRAD_CASES:
        assert RC.fwd_dgrad_query(L, case) == case[14], case
        if case[11]:        # tile statistics are asked for only where the kernel emits them
            d = RC.conv_dims(*case[5:10], *case[3:5])
            assert L.sgg_conv2d_nhwc_fwd_tile_stats(d[4], d[5], d[3], d[6], d[7], d[8], d[9], case[1], case[2]) > 0, case


def test_cases_close_over_every_routable_kernel():
    """Closure: every filter-gradient kernel and every forward / dgrad symbol of the routing tables is the kernel of a GPU case."""
    L = _library()
    assert (len(RC.WGRAD_PER_TAP), len(RC.WGRAD_RESIDENT), len(RC.FWD_DGRAD_CASES)) == (44, 38, 78)
    assert len(set(RC.WGRAD_CASES)) == 82 and len(set(RC.FWD_DGRAD_CASES)) == 78
    table_wgrad, table_fd = _table_kernels()
    wgrad, fd = RC.case_symbols(L)
    assert len(table_wgrad) == 137 and len(table_fd) == 78
    assert wgrad == table_wgrad, "filter-gradient kernels no GPU case reaches: %s; unknown to the table: %s" % (
        sorted(table_wgrad - wgrad), sorted(wgrad - table_wgrad))
    assert fd == table_fd, "forward / dgrad symbols no GPU case reaches: %s; unknown to the table: %s" % (sorted(table_fd - fd), sorted(fd - table_fd))
    assert len(wgrad) == 137 and len(fd) == 78
    # one row per forward / dgrad symbol
    assert len({c[14] for c in RC.FWD_DGRAD_CASES}) == 78


def test_closure_notices_a_missing_kernel(monkeypatch):
    """The closure above is not vacuous: without its cases, conv_wgrad_tr_kernel<2,true> shows up as missing."""
    L = _library()
    monkeypatch.setattr(RC, "WGRAD_CASES", [c for c in RC.WGRAD_CASES if c[11] != "conv_wgrad_tr_kernel<2,true>"])
    assert len(RC.WGRAD_CASES) == 80
    wgrad, _ = RC.case_symbols(L)
    assert _table_kernels()[0] - wgrad == {"conv_wgrad_tr_kernel<2,true>"}


def _older_wgrad_launches():
    """The filter-gradient launches of the kernel-level GPU tests that compare with fp64 and predate these cases, assumed generously
    (every list in every mode its test can run): (shape, precision, algo, ln, operand_format)."""
    from tests import test_fullsize_conv_gpu as TF
    from tests import test_kernels_gpu as TK
    from tests import test_presplit_gpu as TP
    rows = [(c, p, 0, 0, 0) for c in TK.CONV_CASES for p in (0, 2, 6, 3, 1, 4)] + [((4, 48, 48, 32, 32, 3, 1), 2, 0, 0, 0)]
    rows += [(c + (3, 1), p, 0, 0, 0) for c in TK.HALO_CASES for p in (2, 3, 1, 4)]
    rows += [(c + (3, 1), p, 0, ln, 0) for c in TK.LNP_CASES for p in (2, 3) for ln in (0, 1)]
    rows += [(c + (32, 32, 5, 2), p, 0, ln, 0) for c in TK.S2D_CASES for p in (2, 3) for ln in (0, 1)]
    rows += [(c, 2, 0, 0, fmt) for c in TP.DMA_CASES for fmt in (3, 1)]
    rows += [(c, 2, 0, 0, fmt) for c in TP.WGRAD_BAND_CASES for fmt in (0, 1, 2, 3)]
    for B, layers in ((2, TF.LAYERS), (64, [TF.LAYERS[0], TF.LAYERS[5], TF.LAYERS[9]])):
        rows += [((B, H, H, Ci, Co, k, s), p, 0, 0, fmt) for (_, H, Ci, Co, k, s) in layers for (p, fmt) in ((0, 0), (2, 0), (2, 3))]
    return rows


def test_kernels_the_older_case_lists_reach():
    """Informational: how many of the 137 filter-gradient kernels the case lists of tests/test_kernels_gpu.py (CONV_CASES in all six
    modes, the split-K shape, HALO_CASES, LNP_CASES, S2D_CASES), tests/test_presplit_gpu.py (DMA_CASES, WGRAD_BAND_CASES) and
    tests/test_fullsize_conv_gpu.py reach by themselves: 102.  The other 35 ran against fp64 nowhere before tests/test_conv_routes_gpu.py:
    the per-tap split forms on 64+ channel tiles and conv_wgrad_tr_kernel<2,*>, the LN prologue in the stride-2 tap classes except
    conv1_3's, and the 64-column LDS-DMA kernel under 5x5 stride 2."""
    L = _library()
    reached = set()
    for shape, precision, algo, ln, fmt in _older_wgrad_launches():
        reached.update(RC.wgrad_query(L, shape + (precision, algo, ln, fmt))[0].split(";"))
    table_wgrad, _ = _table_kernels()
    assert reached <= table_wgrad
    missing = table_wgrad - reached
    assert (len(reached), len(missing)) == (102, 35)
    fam = lambda prefix: {k for k in missing if k.startswith(prefix)}
    assert fam("conv_wgrad_tr_kernel") == {"conv_wgrad_tr_kernel<2,true>", "conv_wgrad_tr_kernel<2,false>"}
    assert fam("conv_wgrad_dma_kernel") == {"conv_wgrad_dma_kernel<2,2,2>", "conv_wgrad_dma_kernel<2,2,3>", "conv_wgrad_dma_kernel<2,3,2>"}
    assert len(fam("conv_wgrad_kernel<")) == 18 and len(fam("conv_wgrad_halo3_kernel<")) == 12
    assert all(k.endswith(",true,0,false>") and ",3,3," not in k for k in fam("conv_wgrad_halo3_kernel<"))        # LN prologue, classes 2,2 | 2,3 | 3,2
