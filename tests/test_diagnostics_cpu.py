"""CPU: the host side of the training diagnostics (sgg_amd/diagnostics.py): the chunk table the device pass walks, the summary and
NonFiniteError, the fp64 reference on a hand-computed case, and train.py's flags."""
import math

import numpy as np
import pytest

import sgg_amd  # noqa: F401
from sgg_amd import diagnostics as dg
from sgg_amd import lib
from sgg_amd.params import ParamArena, is_dead


def _check_cover(table, offsets, numels, chunk, arena_numel):
    """Every element of every tensor exactly once, no chunk across two tensors, no padding element, rows sorted by tensor."""
    cover = np.zeros(arena_numel, dtype=np.int32)
    owner = np.full(arena_numel, -1, dtype=np.int64)
    for t, (o, n) in enumerate(zip(offsets, numels)):
        owner[o:o + n] = t
    assert (np.diff(table[:, 0]) >= 0).all()
    for t, first, count in table.tolist():
        assert 1 <= count <= chunk and first % 4 == 0
        assert (owner[first:first + count] == t).all(), "chunk (%d, %d, %d) leaves its tensor" % (t, first, count)
        cover[first:first + count] += 1
    assert (cover[owner >= 0] == 1).all() and (cover[owner < 0] == 0).all()
    assert sorted(set(table[:, 0].tolist())) == list(range(len(offsets)))
    dg.check_table(table, len(offsets), arena_numel, chunk)


def test_chunk_constant_is_the_librarys():
    so = lib.load_library()
    assert so.sgg_arena_stats_chunk() == dg.CHUNK and dg.CHUNK % 4 == 0
    assert so.sgg_arena_stats_nstat() == dg.NSTAT == len(dg.STAT_NAMES)
    assert so.sgg_arena_stats_workspace_bytes(7) == 7 * dg.NSTAT * 8


@pytest.mark.parametrize("kind", ["G", "D"])
def test_chunk_table_on_real_config1_layout(kind):
    arena = ParamArena(kind, 1000, 224, device="meta")
    names, offsets, numels = dg.live_layout(arena)
    assert names == [n for n in arena.shapes if not is_dead(n)] and not any(is_dead(n) for n in names)
    assert len(names) == len(arena.shapes) - 8                          # conv3_3 / conv3_4: kernel, bias, gamma, beta each
    assert sum(numels) == arena.live_param_count()
    table = dg.chunk_table(offsets, numels)
    _check_cover(table, offsets, numels, dg.CHUNK, arena.total_numel)
    # nothing of the dead tail: every chunk ends inside the live range
    assert int((table[:, 1] + table[:, 2]).max()) <= arena.live_numel < arena.total_numel
    # the balance the chunking is for: the attention perceptron is most of the table, a conv bias is one row
    att = names.index("attention_perceptron/kernel")
    assert (table[:, 0] == att).sum() == -(-numels[att] // dg.CHUNK) > len(table) // 2
    assert (table[:, 0] == names.index("conv2d/bias")).sum() == 1


def test_chunk_table_on_a_crafted_layout():
    chunk = 8
    numels = [1, 2, 3, 4, 5, 7, 8, 9, 3 * 8 + 7]
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += (n + 3) // 4 * 4
    offsets[5:] = [o + 12 for o in offsets[5:]]                         # a gap between two tensors: never covered
    total = off + 12
    table = dg.chunk_table(offsets, numels, chunk)
    _check_cover(table, offsets, numels, chunk, total)
    assert table[table[:, 0] == 8].tolist() == [[8, offsets[8], 8], [8, offsets[8] + 8, 8], [8, offsets[8] + 16, 8], [8, offsets[8] + 24, 7]]
    assert len(table) == 5 + 1 + 1 + 2 + 4
    for bad in (dict(offsets=[0, 2], numels=[1, 1]), dict(offsets=[0, 4], numels=[5, 1]), dict(offsets=[0], numels=[0])):
        with pytest.raises(ValueError):
            dg.chunk_table(chunk=chunk, **bad)
    with pytest.raises(ValueError):
        dg.chunk_table([0], [4], chunk=6)
    with pytest.raises(ValueError):
        dg.check_table(table, len(numels), total - 4, chunk)            # the last chunk's float4 would leave the arena


def test_stats_reference_hand_computed():
    """Three tensors of 3, 1 and 5 elements (offsets 0, 4, 8); the padding slots hold values that must not show."""
    nan, inf = float("nan"), float("inf")
    p = np.array([3, -4, 0, 99,        2, 99, 99, 99,     1, nan, -2, 2, -inf, 99, 99, 99], dtype=np.float32)
    g = np.array([8, -16, 24, nan,     inf, 7, 7, 7,      0, 0, -0.0, 0, 0, 1e30, 1e30, 1e30], dtype=np.float32)
    m = np.array([1, 2, -2, 5,         3, 5, 5, 5,        0, 1, 1, nan, 4, 5, 5, 5], dtype=np.float32)
    v = np.array([4, 16, 0, 5,         -1, 5, 5, 5,       0, 0, 1, 1, 4, 5, 5, 5], dtype=np.float32)
    rows = dg.stats_reference(p, g, m, v, [0, 4, 8], [3, 1, 5], lr_t=0.5, eps=0.25, grad_scale=0.125)
    # tensor 0: g = (1, -2, 3); p = (3, -4, 0); u = 0.5 * (1, 2, -2) / ((2, 4, 0) + 0.25) = (2/9, 4/17, -4)
    u0 = np.array([0.5 / 2.25, 1.0 / 4.25, -4.0], dtype=np.float32).astype(np.float64)
    assert rows[0, :6].tolist() == [14.0, 3.0, 0.0, 25.0, 4.0, 0.0]
    assert abs(rows[0, 6] - float((u0 * u0).sum())) <= 1e-6 and rows[0, 7] == 4.0 and rows[0, 8] == 0.0
    # tensor 1: g = Inf (counted, not accumulated); p = 2; v = -1: sqrt is NaN -> u non-finite
    assert rows[1].tolist() == [0.0, 0.0, 1.0, 4.0, 2.0, 0.0, 0.0, 0.0, 1.0]
    # tensor 2: g all (signed) zero; p = (1, NaN, -2, 2, -Inf): two non-finite, sum 9, max 2;
    #           u = 0.5 * (0, 1, 1, NaN, 4) / ((0, 0, 1, 1, 2) + 0.25) = (0, 2, 0.4, NaN, 8/9): v == 0 is finite through eps
    u2 = np.array([0.0, 2.0, 0.5 / 1.25, 2.0 / 2.25], dtype=np.float32).astype(np.float64)
    assert rows[2, :6].tolist() == [0.0, 0.0, 0.0, 9.0, 2.0, 2.0]
    assert abs(rows[2, 6] - float((u2 * u2).sum())) <= 1e-6 and rows[2, 7] == 2.0 and rows[2, 8] == 1.0
    # grad_scale is applied in float32 before the square
    one = dg.stats_reference(p, g, m, v, [0], [3], 0.5, 0.25, 1.0)
    assert one[0, :3].tolist() == [64.0 + 256.0 + 576.0, 24.0, 0.0]
    vs = dg.vector_stats_reference([0.5, 1.0, 1.5, nan, -inf, 3.0], 1.0)
    assert vs.tolist() == [0.5, 3.0, 6.0, 2.0, 2.0]                      # the value AT the threshold is not above it


def _rows(spec):
    """rows [T, 9] from per-tensor (g_ss, g_max, g_bad, p_ss, p_max, p_bad, u_ss, u_max, u_bad)."""
    return np.asarray(spec, dtype=np.float64)


def test_summarise_and_nonfinite_error():
    names, numels = ["a/kernel", "a/bias", "b/kernel", "b/bias"], [12, 4, 100, 2]
    rows = _rows([[9.0, 2.0, 0, 16.0, 3.0, 0, 1.0, 0.5, 0],
                  [16.0, 4.0, 0, 0.0, 0.0, 0, 4.0, 2.0, 0],            # a zero-norm weight: no ratio, no division by zero
                  [144.0, 6.0, 0, 9.0, 1.0, 0, 0.0, 0.0, 0],
                  [0.0, 0.0, 0, 0.25, 0.5, 0, 0.25, 0.5, 0]])
    s = dg.summarise(rows, names, numels)
    assert s["grad_norm"] == 13.0 and s["param_norm"] == math.sqrt(25.25) and s["update_norm"] == math.sqrt(5.25)
    assert s["update_ratio"] == math.sqrt(5.25) / math.sqrt(25.25)
    assert s["nonfinite"] == {"g": 0, "p": 0, "u": 0} and s["first_nonfinite"] is None
    assert s["max_grad_norm"] == {"tensor": "b/kernel", "value": 12.0}
    assert s["max_update_ratio"] == {"tensor": "b/bias", "value": 1.0}     # 0.5 / 0.5; a/bias (weight norm 0) is left out
    assert s["grad_absmax"] == 6.0 and s["elements"] == 118
    dg.raise_if_nonfinite({"G": s, "D": s})                              # nothing to raise
    # non-finite counts in tensors 3 (g) and 1 (p and u): tensor 1 is first in arena order
    rows2 = rows.copy()
    rows2[3, 2], rows2[1, 5], rows2[1, 8] = 2, 1, 3
    s2 = dg.summarise(rows2, names, numels)
    assert s2["nonfinite"] == {"g": 2, "p": 1, "u": 3}
    assert s2["first_nonfinite"] == {"tensor": "a/bias", "which": ["p", "u"]}
    with pytest.raises(dg.NonFiniteError) as e:
        dg.raise_if_nonfinite({"G": s, "D": s2}, itr=7)
    assert (e.value.network, e.value.tensor, e.value.which, e.value.itr) == ("D", "a/bias", ["p", "u"], 7)
    assert "parameter / update" in str(e.value) and "'a/bias'" in str(e.value) and "D" in str(e.value) and "7" in str(e.value)
    assert isinstance(e.value, ArithmeticError)
    # every weight zero: ratios are None, not an exception
    z = rows.copy()
    z[:, 3] = 0.0
    sz = dg.summarise(z, names, numels)
    assert sz["update_ratio"] is None and sz["max_update_ratio"] == {"tensor": None, "value": None}
    t = dg.tensor_rows(rows2, names)
    assert list(t) == names and t["b/bias"]["g_nonfinite"] == 2 and isinstance(t["b/bias"]["g_nonfinite"], int)
    assert t["a/kernel"]["g_sumsq"] == 9.0 and set(t["a/kernel"]) == set(dg.STAT_NAMES)


def test_train_flags_parse_and_default_to_off():
    import train as T
    p = T.build_parser()
    off = p.parse_args([])
    assert off.diagnostics_every == 0 and off.halt_on_nonfinite is False
    on = p.parse_args(["--diagnostics_every", "25", "--halt_on_nonfinite"])
    assert on.diagnostics_every == 25 and on.halt_on_nonfinite is True
    text = p.format_help()
    assert "last good" in " ".join(text.split()) and "--diagnostics_every" in text


def test_armed_network_without_the_kernel_is_an_error():
    """No quiet fallback: a kernel set without arena_stats (the CPU reference kernels) cannot be armed."""
    from oracle.kernels_ref import RefKernels
    from sgg_amd.step import Network
    net = Network.__new__(Network)
    net.K, net.opt = RefKernels(), {"t": 0, "pending": None}
    with pytest.raises(RuntimeError, match="arena_stats"):
        net.arm_diagnostics(True)
    net.arm_diagnostics(False)                                            # disarming needs nothing
    assert net.opt["armed"] is False
