"""Training diagnostics: per-tensor gradient / parameter / update norms and non-finite counts (host side; pure Python + NumPy).

The device pass is csrc/stats.hip (HipKernels.arena_stats / vector_stats): one read of a network's four arenas (parameters,
gradients, Adam m and v) behind an optimiser step gives, per tensor, the sum of squares, the largest magnitude and the non-finite
count of
    g = grad * grad_scale                     the gradient the step consumed,
    p                                         the parameter after the step,
    u = lr_t * m / (sqrt(v) + eps)            the delta the step applied (up to its sign).
This module builds the chunk table that pass walks, restates both kernels in fp64 NumPy (the yardstick of the GPU tests) and turns
the rows into what a person reads: global norms, the update / weight ratio, the first tensor that went non-finite.
"""
from __future__ import annotations

import math

import numpy as np

CHUNK = 16384          # elements per chunk of the table: the library's compile-time constant (sgg_arena_stats_chunk; checked in the tests)
NSTAT = 9
STAT_NAMES = ("g_sumsq", "g_absmax", "g_nonfinite", "p_sumsq", "p_absmax", "p_nonfinite", "u_sumsq", "u_absmax", "u_nonfinite")
KINDS = (("g", "gradient"), ("p", "parameter"), ("u", "update"))
VECTOR_STAT_NAMES = ("min", "max", "sum", "above", "nonfinite")


class NonFiniteError(FloatingPointError):
    """A reported iteration found Inf or NaN: names the network, the first such tensor in arena order and which of gradient (g),
    parameter (p) and applied update (u) it was found in."""

    def __init__(self, network, tensor, which, itr=None):
        self.network, self.tensor, self.which, self.itr = network, tensor, which, itr
        what = " / ".join(dict(KINDS)[k] for k in which)
        super().__init__("non-finite %s in %s tensor %r%s" % (what, network, tensor, "" if itr is None else " at iteration %d" % itr))


def live_layout(arena):
    """(names, offsets, numels) of an arena's live tensors in arena order (params.ParamArena lays the dead conv3_3 / conv3_4 branch
    out behind them: it is not part of the pass)."""
    from .params import is_dead
    names = [n for n in arena.offsets if not is_dead(n)]
    return names, [int(arena.offsets[n]) for n in names], [int(math.prod(arena.shapes[n])) for n in names]


def chunk_table(offsets, numels, chunk=CHUNK):
    """int64 [n_chunks, 3] rows (tensor, first arena element, count): every tensor cut into pieces of at most `chunk` elements, in
    the order given; a chunk never spans two tensors and covers no padding.  offsets: the tensors' first arena elements (multiples
    of 4, ascending, each tensor's extent rounded up to 4 ends at or before the next offset); numels: their element counts."""
    chunk = int(chunk)
    if chunk < 4 or chunk % 4:
        raise ValueError("chunk_table: the chunk length must be a positive multiple of 4 (got %d)" % chunk)
    rows, end = [], 0
    for t, (off, n) in enumerate(zip(offsets, numels)):
        off, n = int(off), int(n)
        if off % 4 or off < end or n < 1:
            raise ValueError("chunk_table: tensor %d at offset %d with %d elements (offsets are ascending multiples of 4 behind the "
                             "previous tensor's padded extent %d; tensors are not empty)" % (t, off, n, end))
        end = off + (n + 3) // 4 * 4
        for s in range(0, n, chunk):
            rows.append((t, off + s, min(chunk, n - s)))
    return np.asarray(rows, dtype=np.int64).reshape(-1, 3)


def check_table(table, n_tensors, arena_numel, chunk=CHUNK):
    """The conditions the device pass relies on without checking them (include/sgg_hip.h): raises ValueError if a chunk would read
    outside an arena of `arena_numel` elements."""
    t = np.asarray(table)
    ok = (t.ndim == 2 and t.shape[1] == 3 and len(t) >= 1 and (t[:, 1] >= 0).all() and (t[:, 1] % 4 == 0).all()
          and (t[:, 2] >= 1).all() and (t[:, 2] <= chunk).all() and ((t[:, 1] + (t[:, 2] + 3) // 4 * 4) <= arena_numel).all()
          and (np.diff(t[:, 0]) >= 0).all() and t[0, 0] >= 0 and t[-1, 0] < n_tensors)
    if not ok:
        raise ValueError("chunk table does not fit an arena of %d elements and %d tensors" % (arena_numel, n_tensors))


def _three(x):
    """(sum of squares in fp64, max |x|, non-finite count) over the finite elements of the fp32 array x."""
    fin = np.isfinite(x)
    xf = x[fin].astype(np.float64)
    return [float(np.sum(xf * xf)), float(np.max(np.abs(xf))) if xf.size else 0.0, float(x.size - xf.size)]


def stats_reference(params, grads, m, v, offsets, numels, lr_t, eps, grad_scale=1.0):
    """fp64 NumPy restatement of arena_stats: [T, NSTAT] rows for the tensors at `offsets` / `numels` of the four flat fp32 arrays.
    g = grads * grad_scale and u = lr_t * m / (sqrt(v) + eps) are taken in float32 first (as the optimiser kernel forms them), the
    squares in float64 (exact for fp32 values)."""
    f32 = np.float32
    arr = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (params, grads, m, v)]
    out = np.zeros((len(offsets), NSTAT), dtype=np.float64)
    with np.errstate(all="ignore"):
        for t, (off, n) in enumerate(zip(offsets, numels)):
            p, g, mm, vv = (a[int(off):int(off) + int(n)] for a in arr)
            gs = g * f32(grad_scale)
            u = (f32(lr_t) * mm) / (np.sqrt(vv) + f32(eps))
            assert gs.dtype == np.float32 and u.dtype == np.float32
            out[t] = _three(gs) + _three(p) + _three(u)
    return out


def vector_stats_reference(x, threshold):
    """fp64 restatement of vector_stats: (min, max, sum, count above the threshold) over the finite elements, non-finite count."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    xf = x[np.isfinite(x)]
    return np.asarray([xf.min() if xf.size else np.inf, xf.max() if xf.size else -np.inf, xf.astype(np.float64).sum(),
                       float((xf > np.float32(threshold)).sum()), float(x.size - xf.size)], dtype=np.float64)


def _ratio(u, p):
    """update / weight norm; None for a zero-norm weight (a freshly zero-initialised bias)."""
    return float(u / p) if p > 0.0 else None


def tensor_rows(rows, names):
    """{name: {stat name: value}} of arena_stats' rows."""
    rows = np.asarray(rows, dtype=np.float64).reshape(len(names), NSTAT)
    return {n: {k: (int(x) if k.endswith("nonfinite") else float(x)) for k, x in zip(STAT_NAMES, r)} for n, r in zip(names, rows)}


def summarise(rows, names, numels):
    """What one reads first of a network's rows [T, NSTAT] (tensors `names` in arena order, `numels` elements each): the global L2
    norms of gradient, parameter and applied update (root of the summed squares, finite elements), update / weight ratio, total
    non-finite counts, the first tensor in arena order with a non-finite gradient, parameter or update (and which), and the tensors
    with the largest gradient norm and the largest update / weight ratio."""
    rows = np.asarray(rows, dtype=np.float64).reshape(len(names), NSTAT)
    assert len(numels) == len(names)
    gn, pn, un = (math.sqrt(float(rows[:, c].sum())) for c in (0, 3, 6))
    bad = rows[:, (2, 5, 8)]
    first = None
    for t in np.flatnonzero(bad.sum(axis=1) > 0)[:1]:
        first = {"tensor": names[t], "which": [k for (k, _), c in zip(KINDS, bad[t]) if c > 0]}
    tg = int(np.argmax(rows[:, 0]))
    ratios = [(_ratio(math.sqrt(r[6]), math.sqrt(r[3])), n) for r, n in zip(rows, names)]
    ratios = [(x, n) for x, n in ratios if x is not None]
    top_ratio = max(ratios) if ratios else (None, None)
    return {"grad_norm": gn, "param_norm": pn, "update_norm": un, "update_ratio": _ratio(un, pn),
            "grad_absmax": float(rows[:, 1].max()), "elements": int(sum(numels)),
            "nonfinite": {k: int(bad[:, i].sum()) for i, (k, _) in enumerate(KINDS)},
            "first_nonfinite": first,
            "max_grad_norm": {"tensor": names[tg], "value": math.sqrt(float(rows[tg, 0]))},
            "max_update_ratio": {"tensor": top_ratio[1], "value": top_ratio[0]}}


def raise_if_nonfinite(diag, itr=None):
    """NonFiniteError for the first network ("G", then "D") of a GanStep.diagnostics() record whose summary counts a non-finite
    gradient, parameter or update."""
    for net in ("G", "D"):
        if net not in diag:                 # (the G-only record of the pretraining phase)
            continue
        first = diag[net]["first_nonfinite"]
        if first is not None:
            raise NonFiniteError(net, first["tensor"], first["which"], itr)
