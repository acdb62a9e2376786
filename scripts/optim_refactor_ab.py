"""optim_refactor_ab.py - the optimiser's whole-arena passes of one library against another's, in one process: bits, then time.

    python scripts/optim_refactor_ab.py --parent PATH [--new PATH] [--repeats 20] [--vocab 1000] [--size 224] [--out FILE]

Both libraries are loaded with ctypes (the entry points below are bound directly, so a library built from another commit loads too;
--new defaults to the tree's own libsgg_hip.so).

  bits    the four Adam forms (plain, with the average, guarded, guarded with the average), swap, grad_accumulate (first and not first),
          grad_guard (workspace and record) and arena_stats (workspace and rows) on the same seeded inputs, for n = 1, 3, 4, 5, 1027 and
          4 * 256 * 4096 + 5 (the scalar tail alone, the vector body, a second trip of the grid-stride loop), gradient scales 1 and
          0.125, one_minus_decay 0.9, and two records made by each library's own grad_guard: an applied one (clipped, coef 0.5) and a
          dropped one (a NaN in the gradient, the skip armed).  Reported: the number of differing BITS per output, summed over the
          cases.  Required: zero everywhere.
  timing  the legs adam, adam_ema, grad_guard + adam_guarded, grad_guard + adam_ema_guarded, swap and grad_accumulate on the live
          arena of G (vocab 1000, 224 x 224), as scripts/bench_guard.py times them: bursts of launches between two device events,
          parent and new alternating (the one that goes first changes with every repetition), --repeats repetitions.  Required: the median of the new library does not exceed the parent's
          slowest repetition of the same leg (the parent's own spread in the same run is the noise).

Prints ONE JSON line (with --out also into FILE); exit status 1 unless both requirements hold.  Needs the GPU; reads nothing outside the
repository except the two libraries."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = (1, 3, 4, 5, 1027, 4 * 256 * 4096 + 5)
SCALES = (1.0, 0.125)
OMD = 0.9
LEGS = ("adam", "adam_ema", "guard_adam_guarded", "guard_adam_ema_guarded", "swap", "grad_accumulate")


class Lib:
    """The entry points under comparison, on raw device tensors (current stream = the null stream)."""

    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        vp, i, ll, sz, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_float
        L.sgg_last_error.restype = ctypes.c_char_p
        for name, args in (("sgg_adam_tf_multi", [vp] * 4 + [ll] + [f] * 5 + [vp]),
                           ("sgg_adam_tf_multi_ema", [vp] * 5 + [ll] + [f] * 6 + [vp]),
                           ("sgg_adam_tf_multi_guarded", [vp] * 4 + [ll] + [f] * 4 + [vp, vp]),
                           ("sgg_adam_tf_multi_ema_guarded", [vp] * 5 + [ll] + [f] * 4 + [vp, f, vp]),
                           ("sgg_swap_f32", [vp, vp, ll, vp]), ("sgg_grad_accumulate", [vp, vp, ll, i, vp]),
                           ("sgg_grad_guard", [vp, ll, f, f, i, i, vp, sz, vp, vp]),
                           ("sgg_arena_stats", [vp] * 5 + [i, i, f, f, f, i, vp, sz, vp, vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = i, args
        L.sgg_grad_guard_workspace_bytes.restype, L.sgg_grad_guard_workspace_bytes.argtypes = sz, [ll]
        L.sgg_arena_stats_workspace_bytes.restype, L.sgg_arena_stats_workspace_bytes.argtypes = sz, [i]
        L.sgg_arena_stats_chunk.restype = L.sgg_arena_stats_nstat.restype = i

    def call(self, name, *args):
        rc = getattr(self.L, name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], None)
        if rc != 0:
            raise RuntimeError("%s: %d %s" % (name, rc, self.L.sgg_last_error().decode()))


def diff_bits(a, b):
    wa, wb = (t.contiguous().view(torch.uint8) for t in (a, b))
    x = wa ^ wb
    return int(np.unpackbits(x[x != 0].cpu().numpy()).sum())


def inputs(n, seed, dev):
    """p, g, m, v, e (and a second gradient-like arena) of n elements, each in an allocation rounded up to whole float4s."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    pad = (n + 3) // 4 * 4
    t = {k: (torch.randn(pad, generator=gen, device=dev) * s)[:n] for k, s in (("p", 0.05), ("g", 1e-3), ("m", 1e-3), ("e", 0.05), ("a", 1e-3))}
    t["v"] = (torch.rand(pad, generator=gen, device=dev) * 1e-6)[:n]
    return t


def storage(t):
    """The whole allocation behind a view made by inputs(): what a pass wrote behind element n - 1 is compared too."""
    return t.as_strided(((t.numel() + 3) // 4 * 4,), (1,))


def bits_leg(libs, dev, hyper):
    from sgg_amd import diagnostics
    out, cases = {}, 0

    def run(what, n, seed, fn, keys):
        """fn(lib, tensors) on a fresh copy of the same inputs per library; the tensors named in `keys` are compared."""
        nonlocal cases
        res = []
        for lib in libs:
            t = inputs(n, seed, dev)
            extra = fn(lib, t) or {}
            torch.cuda.synchronize()
            res.append(dict({k: storage(t[k]) for k in keys}, **extra))
        for k in res[0]:
            out["%s.%s" % (what, k)] = out.get("%s.%s" % (what, k), 0) + diff_bits(res[0][k], res[1][k])
        cases += 1

    def guard(lib, t, n, scale, dropped):
        """The record of the library's own grad_guard: clipped to half the norm; dropped = a NaN in the gradient, the skip armed."""
        if dropped:
            t["g"][n // 2] = float("nan")
        ws = torch.zeros(max(8, lib.L.sgg_grad_guard_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        rec = torch.zeros(8, dtype=torch.float64, device=dev)
        finite = torch.nan_to_num(t["g"].double() * scale, nan=0.0)
        lib.call("sgg_grad_guard", t["g"], n, scale, 0.5 * float(finite.norm()), 1, 0, ws, ws.numel(), rec)
        return ws, rec

    for n in SIZES:
        for scale in SCALES:
            seed = 1000 + n % 977
            run("adam", n, seed, lambda lib, t: lib.call("sgg_adam_tf_multi", t["p"], t["g"], t["m"], t["v"], n, *hyper, scale), "pgmv")
            run("adam_ema", n, seed, lambda lib, t: lib.call("sgg_adam_tf_multi_ema", t["p"], t["g"], t["m"], t["v"], t["e"], n, *hyper,
                                                             scale, OMD), "pgmve")
            for dropped in (False, True):
                def guarded(lib, t, with_ema):
                    ws, rec = guard(lib, t, n, scale, dropped)
                    if with_ema:
                        lib.call("sgg_adam_tf_multi_ema_guarded", t["p"], t["g"], t["m"], t["v"], t["e"], n, *hyper, rec, OMD)
                    else:
                        lib.call("sgg_adam_tf_multi_guarded", t["p"], t["g"], t["m"], t["v"], n, *hyper, rec)
                    assert float(rec[5]) == (0.0 if dropped else 1.0), rec.tolist()
                    return {"workspace": ws, "record": rec}
                tag = "dropped" if dropped else "applied"
                run("grad_guard+adam_guarded[%s]" % tag, n, seed, lambda lib, t: guarded(lib, t, False), "pgmv")
                run("grad_guard+adam_ema_guarded[%s]" % tag, n, seed, lambda lib, t: guarded(lib, t, True), "pgmve")

            def stats(lib, t):
                chunk, ns = lib.L.sgg_arena_stats_chunk(), lib.L.sgg_arena_stats_nstat()
                h = (n // 2) // 4 * 4                     # two tensors where the range is long enough
                offsets, numels = ([0, h], [h, n - h]) if h else ([0], [n])
                table = torch.from_numpy(diagnostics.chunk_table(offsets, numels, chunk)).to(dev)
                ws = torch.zeros(max(8, lib.L.sgg_arena_stats_workspace_bytes(len(table))), dtype=torch.uint8, device=dev)
                rows = torch.zeros((len(offsets), ns), dtype=torch.float64, device=dev)
                lib.call("sgg_arena_stats", t["p"], t["g"], t["m"], t["v"], table, len(table), len(offsets), hyper[0], hyper[3], scale, 0,
                         ws, ws.numel(), rows)
                return {"workspace": ws, "rows": rows}
            run("arena_stats", n, seed, stats, "pgmv")
        run("swap", n, 7 + n % 977, lambda lib, t: lib.call("sgg_swap_f32", t["p"], t["e"], n), "pe")
        for first in (1, 0):
            run("grad_accumulate[%s]" % ("first" if first else "add"), n, 9 + n % 977,
                lambda lib, t: lib.call("sgg_grad_accumulate", t["a"], t["g"], n, first), "ag")
    return {"sizes": list(SIZES), "grad_scales": list(SCALES), "one_minus_decay": OMD, "cases": cases, "differing_bits": out,
            "ok": not any(out.values())}


def timing_leg(libs, names, dev, hyper, V, S, repeats, burst=10):
    from sgg_amd.params import ParamArena
    n = ParamArena("G", V, S, device="meta").live_numel
    t = inputs(n, 7, dev)
    rec = torch.zeros(8, dtype=torch.float64, device=dev)
    ws = torch.empty(max(8, libs[0].L.sgg_grad_guard_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    max_norm = 0.5 * float(t["g"].double().norm())
    arenas = (t["p"], t["g"], t["m"], t["v"])

    def legs(lib):
        guard = lambda: lib.call("sgg_grad_guard", t["g"], n, 1.0, max_norm, 1, 0, ws, ws.numel(), rec)
        return {"adam": lambda: lib.call("sgg_adam_tf_multi", *arenas, n, *hyper, 1.0),
                "adam_ema": lambda: lib.call("sgg_adam_tf_multi_ema", *arenas, t["e"], n, *hyper, 1.0, 1e-3),
                "guard_adam_guarded": lambda: (guard(), lib.call("sgg_adam_tf_multi_guarded", *arenas, n, *hyper, rec)),
                "guard_adam_ema_guarded": lambda: (guard(), lib.call("sgg_adam_tf_multi_ema_guarded", *arenas, t["e"], n, *hyper, rec, 1e-3)),
                "swap": lambda: lib.call("sgg_swap_f32", t["p"], t["e"], n),
                "grad_accumulate": lambda: lib.call("sgg_grad_accumulate", t["a"], t["g"], n, 0)}

    res = {"vocab": V, "parameters": int(n), "burst": burst, "repeats": repeats,
           "order": "%s first in even repetitions, %s first in odd ones" % tuple(names),
           "legs": alternating_bursts([legs(lib) for lib in libs], LEGS, names, repeats, burst)}
    res["ok"] = all(v["new_median_within_parent_max"] for v in res["legs"].values())
    return res


def alternating_bursts(fns, legs, names, repeats, burst=10):
    """fns[0] (parent) and fns[1] (new): {leg: a function that enqueues one call}.  Per leg and repetition one burst of each between
    two device events, parent and new alternating -> {leg: medians, extremes, every time, and the criterion}."""
    for f in fns:
        for fn in f.values():
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    ms = [{k: [] for k in legs} for _ in fns]
    for r in range(repeats):
        for k in legs:
            # the second burst of a pair starts on the cache state (dirty lines of the same arenas) the first one left, the first on
            # that of another leg: which library goes first changes with every repetition
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):
                f = fns[which]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(burst):
                    f[k]()
                e1.record()
                e1.synchronize()
                ms[which][k].append(e0.elapsed_time(e1) / burst)
    res = {}
    for k in legs:
        par, new = ms[0][k], ms[1][k]
        res[k] = {names[0]: {"median": round(float(np.median(par)), 5), "min": round(min(par), 5), "max": round(max(par), 5)},
                  names[1]: {"median": round(float(np.median(new)), 5), "min": round(min(new), 5), "max": round(max(new), 5)},
                  "new_median_within_parent_max": bool(np.median(new) <= max(par)),
                  "ms_all": {names[0]: [round(x, 5) for x in par], names[1]: [round(x, 5) for x in new]}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=None)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.build import LIB_PATH
    from sgg_amd.params import ADAM_B1, ADAM_B2, ADAM_EPS
    from sgg_amd.step import tf_adam_lr_t
    dev = torch.device("cuda:0")
    libs = [Lib(args.parent), Lib(args.new or LIB_PATH)]
    hyper = (tf_adam_lr_t(100), ADAM_B1, ADAM_B2, ADAM_EPS)
    rec = {"metric": "optim_refactor_ab", "parent": os.path.basename(args.parent), "new": os.path.basename(args.new or LIB_PATH),
           "bits": bits_leg(libs, dev, hyper), "timing": timing_leg(libs, ("parent", "new"), dev, hyper, args.vocab, args.size, args.repeats),
           "device": torch.cuda.get_device_name(0)}
    rec["ok"] = rec["bits"]["ok"] and rec["timing"]["ok"]
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if rec["ok"] else 1)


if __name__ == "__main__":
    main()
