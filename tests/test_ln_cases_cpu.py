"""The cases of tests/test_layernorm_geometry_gpu.py stay on the code paths they were built for (no GPU): the launch geometry of
csrc/layernorm.hip restated in tests/ln_cases.py, checked against the constants in the source and against the case table."""
import os
import re

import pytest

from tests import ln_cases as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scene-graph-gan_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_those_of_the_source():
    ln, common = _source("layernorm.hip"), _source("sgg_common.h")
    assert int(re.search(r"constexpr int SGG_LN_WGS = (\d+);", ln).group(1)) == L.LN_WGS
    assert int(re.search(r"#define LN_CHUNK (\d+)", ln).group(1)) == L.LN_CHUNK
    assert int(re.search(r"#define LNF_BL (\d+)", ln).group(1)) == L.LNF_BL
    assert int(re.search(r"#define SGG_TS (\d+)", common).group(1)) == L.TS


def test_geometry_of_the_timed_step():
    """conv1's LayerNorm of the batch-64 step, and the one multi-chunk shape of the older kernel tests."""
    g = L.ln_geometry(64, 224 * 224, 32)
    assert (g.nchunks, g.G, g.cpg, g.last, g.tail) == (392, 24, 17, 1, 0)
    g = L.ln_geometry(2, 448 * 448, 32)
    assert (g.G, g.cpg) == (523, 3)
    assert L.ln_geometry(2, 8 * 8, 32).cpg == 1 and L.ln_geometry(1, 1, 4) == L.Geometry(1, 1, 1, 1, 4)


EXPECT = {      # id: (nchunks, chunks of the last workgroup, N % LN_CHUNK)
    "b64_c256": (25, 1, 3072), "b70_c32": (23, 1, 3200), "b256_c128": (22, 2, 3584), "b96_c512_win": (32, 2, 0),
    "b96_c512_win0": (32, 2, 0), "b96_c256_win_skip": (32, 2, 0),
}


@pytest.mark.parametrize("case", L.CASES, ids=[c.id for c in L.CASES])
def test_case_reaches_the_batch64_paths(case):
    B, H, W, C = case.shape
    g = L.ln_geometry(B, H * W, C)
    assert g.cpg >= 2, "the chunk loops and the running merge need more than one chunk per workgroup"
    assert (g.G, g.cpg) == (case.G, case.cpg), (case.id, g)
    assert (g.nchunks, g.last, g.tail) == EXPECT[case.id], (case.id, g)
    assert B > L.LNF_BL, "the finalize's sample loop needs more than one trip per lane"
    assert L.LN_CHUNK % C == 0 and C % 32 == 0      # (whole pixels per chunk; the pre-split output needs 32-channel groups)
    census = L.chunk_census(case.shape, case.region)
    assert len(census) == g.G and sum(len(r) for r in census) == g.nchunks
    if case.region is None:
        assert sum(map(sum, census)) == H * W * C and census[-1][-1] == (g.tail or L.LN_CHUNK)
        return
    y0, x0, hv, wv = case.region
    assert sum(map(sum, census)) == hv * wv * C
    assert any(sum(r) == 0 for r in census), "no workgroup lies wholly outside the window (empty partial)"
    assert any(0 < n < L.LN_CHUNK for r in census for n in r), "no chunk is partly inside the window"
    assert any(n == 0 for r in census if sum(r) for n in r) == (case.id == "b96_c256_win_skip")


def test_empty_partials_and_skipped_chunks_where_the_table_says():
    by = L.BY_ID
    empty = lambda c: [g for g, r in enumerate(L.chunk_census(c.shape, c.region)) if sum(r) == 0]
    assert empty(by["b96_c512_win"]) == [0, 1, 15]
    assert empty(by["b96_c512_win0"]) == [15]
    census = L.chunk_census(by["b96_c256_win_skip"].shape, by["b96_c256_win_skip"].region)
    assert empty(by["b96_c256_win_skip"]) == [0]
    assert census[1][0] == 0 and census[1][1] > 0, "workgroup 1: its first valid chunk follows a skipped one"
    assert census[15][0] > 0 and census[15][1] == 0, "workgroup 15: a skipped chunk after a valid one"


def test_finalize_trips_per_lane():
    trips = lambda B: sorted({len(range(bl, B, L.LNF_BL)) for bl in range(L.LNF_BL)})
    assert trips(64) == [2] and trips(256) == [8] and trips(96) == [3]
    assert trips(70) == [2, 3], "B = 70: lanes 0 .. 5 make three trips, the others two"
    assert max(c.shape[0] for c in L.CASES) == 256      # maxB of the batched finalize launch


def test_workspace_formula():
    assert L.ln_workspace_bytes(64, 18 * 22, 256) == 64 * 13 * (4 + 2 + 768) * 4 + 256
