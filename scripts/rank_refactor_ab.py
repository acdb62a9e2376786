"""rank_refactor_ab.py - the sort-and-select kernels (csrc/rank.hip, match.hip, kbest.hip, ground.hip, retrieve.hip) of one library
against another's, in one process: bits, then time.

    python scripts/rank_refactor_ab.py --parent PATH [--new PATH] [--repeats 20] [--out FILE]

Both libraries are loaded with ctypes (--new defaults to the tree's own libsgg_hip.so) and each is put behind the product binding
(HipKernels with its `lib` replaced: the C ABI of the two is the same), so the tests' input builders and the benchmarks' set-up code
serve both.  diff_bits, the library wrapper and the alternating burst timing are those of scripts/optim_refactor_ab.py.

  bits    sgg_rank_triples, sgg_match_triples, sgg_kbest_triples, sgg_kbest_merge, sgg_ground_assign, sgg_ground_resolve,
          sgg_retrieve_topk and sgg_retrieve_ranks on the cases of tests/test_predict_gpu.py, test_metrics_gpu.py, test_kbest_gpu.py,
          test_ground_gpu.py and test_retrieve_gpu.py: the reference tests of those files are CALLED, over their own parameter lists,
          with a stand-in for their `hip` fixture that hands every call of the eight to both libraries on the same inputs - into the
          caller's buffers for the parent (zeroed ones where the binding would allocate; the test goes on with the parent's results),
          into a copy of the whole allocations for the new one.  The WHOLE buffer around every output is compared, guard words and
          the slots that no kernel writes included.  Reported: the number of differing BITS per
          output, summed over the calls.  Required: zero everywhere.
  timing  rank_triples as rank_alone of scripts/bench_predict.py sets it up (32 images, 256 and 4096 samples), match_triples as
          match_alone of bench_metrics.py (100 slots against 64 rows, 4096 against 4096), kbest_triples and kbest_merge as
          kernels_alone of bench_kbest.py (V = 1000 and V = 70 000), ground_assign and ground_resolve as kernels_alone of
          bench_ground.py, retrieve_topk and retrieve_ranks as ranking_leg of bench_retrieve.py (Q = 4096, n = 5000): those functions
          run once on the parent and the call they time is taken from them.  Bursts between two device events, parent and new
          alternating, --repeats repetitions.  Required: the median of the new library does not exceed the parent's slowest
          repetition of the same leg (the parent's own spread in the same run is the noise).

Prints ONE JSON line (with --out also into FILE); exit status 1 unless both requirements hold.  Needs the GPU; reads nothing outside the
repository except the two libraries."""
import argparse
import contextlib
import ctypes
import itertools
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import optim_refactor_ab as AB  # noqa: E402

ENTRY_POINTS = ("rank_triples", "match_triples", "kbest_triples", "kbest_merge", "ground_assign", "ground_resolve", "retrieve_topk",
                "retrieve_ranks")
TB = 32             # TEST_BATCH_SIZE at the benchmarks' batch size of 64: the images of a batch, and the samples of K-best decoding
BURST = 50          # launches per pair of events, as the benchmarks above time these kernels


class Lib(AB.Lib):
    """A library behind the product binding: `hip` is a HipKernels whose calls go to this library.  Every declared entry point is
    bound from the binding's own table (sgg_last_error included), so the inherited call() serves too."""

    def __init__(self, path):
        from sgg_amd.lib import SIGNATURES, HipKernels
        L = self.L = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        self.hip = HipKernels("cuda:0")
        self.hip.lib = L


class Tap:
    """Stands in for a HipKernels: a call of one of ENTRY_POINTS goes to on_call(name, args, kwargs), whose result the caller gets;
    everything else is the parent's binding."""

    def __init__(self, parent, on_call):
        self._parent, self._on_call = parent, on_call

    def __getattr__(self, name):
        if name not in ENTRY_POINTS:
            return getattr(self._parent.hip, name)
        return lambda *args, **kwargs: self._on_call(name, args, kwargs)


def whole(t):
    """The allocation t is a view of, as one flat tensor."""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def twin(t):
    """t's view in a copy of its whole allocation."""
    return whole(t).clone().as_strided(t.shape, t.stride(), t.storage_offset())


def parameter_grid(test):
    """The argument sets of a test's own pytest.mark.parametrize decorators."""
    marks = [m for m in getattr(test, "pytestmark", []) if m.name == "parametrize"]
    for values in itertools.product(*[m.args[1] for m in marks]):
        yield dict(zip([m.args[0] for m in marks], values))


def bits_leg(libs):
    from tests import test_ground_gpu, test_kbest_gpu, test_metrics_gpu, test_predict_gpu, test_retrieve_gpu
    tests = (test_predict_gpu.test_rank_triples_matches_numpy_reference, test_metrics_gpu.test_match_triples_equals_reference,
             test_kbest_gpu.test_kbest_triples_matches_fp64_reference, test_kbest_gpu.test_kbest_merge_matches_fp64_reference,
             test_ground_gpu.test_ground_kernels_match_reference, test_retrieve_gpu.test_retrieve_topk_is_exact,
             test_retrieve_gpu.test_retrieve_ranks_are_exact)
    out, calls = {}, {name: 0 for name in ENTRY_POINTS}

    def both(name, args, kwargs):
        given = kwargs.get("out")
        if given is None:       # the binding would allocate: zeroed buffers of those shapes, so that what no kernel writes is equal
            given = {k: torch.zeros_like(v) for k, v in getattr(libs[0].hip, name)(*args, **kwargs).items()}
        copy = {k: twin(v) for k, v in given.items()}
        res = [getattr(lib.hip, name)(*args, **dict(kwargs, out=o)) for lib, o in zip(libs, (given, copy))]
        torch.cuda.synchronize()
        for k in res[0]:
            out["%s.%s" % (name, k)] = out.get("%s.%s" % (name, k), 0) + AB.diff_bits(whole(res[0][k]), whole(res[1][k]))
        calls[name] += 1
        return res[0]

    tap, cases = Tap(libs[0], both), {}
    for test in tests:
        for params in parameter_grid(test):
            test(tap, **params)
            cases[test.__name__] = cases.get(test.__name__, 0) + 1
    return {"test_cases": cases, "launch_pairs": calls, "differing_bits": out,
            "ok": all(calls.values()) and not any(out.values())}


def timing_leg(libs, names, repeats):
    import bench_ground
    import bench_kbest
    import bench_metrics
    import bench_predict
    import bench_retrieve
    dev = libs[0].hip.device
    fns = [{} for _ in libs]

    def take(label, keep, setup):
        """setup(K) runs a benchmark's kernel leg on the parent; the last call it makes of every entry point in `keep` - the one it
        times, with its preallocated outputs - becomes the leg label/entry point of both libraries."""
        last = {}

        def note(name, args, kwargs):
            last[name] = (args, kwargs)
            return getattr(libs[0].hip, name)(*args, **kwargs)
        setup(Tap(libs[0], note))
        torch.cuda.synchronize()
        for name in keep:
            args, kwargs = last[name]
            for lib, f in zip(libs, fns):
                o = kwargs["out"] if lib is libs[0] else {k: torch.empty_like(v) for k, v in kwargs["out"].items()}
                f["%s/%s" % (name, label)] = lambda lib=lib, name=name, args=args, kw=dict(kwargs, out=o): getattr(lib.hip, name)(*args, **kw)

    host = types.SimpleNamespace(device=dev, recalls=lambda *a: None)      # (rank_alone's host loop is not what is taken from it)
    for N in (256, 4096):
        take("N%d" % N, ("rank_triples",), lambda K, N=N: bench_predict.rank_alone(host, K, TB, N, 1000, 1))
    for top_k, M in ((100, 64), (4096, 4096)):
        take("K%d-M%d" % (top_k, M), ("match_triples",), lambda K, top_k=top_k, M=M: bench_metrics.match_alone(K, TB, top_k, M, 1000, 1, burst=1))
    for nb, V in ((TB, 1000), (2, 70000)):
        take("V%d" % V, ("kbest_triples", "kbest_merge"), lambda K, nb=nb, V=V: bench_kbest.kernels_alone(K, dev, TB, nb, V, 1))
    take("N256-14x14", ("ground_assign", "ground_resolve"), lambda K: bench_ground.kernels_alone(K, dev, 8 * TB, TB, 1000, 14))
    take("Q4096-n5000", ("retrieve_topk", "retrieve_ranks"), lambda K: bench_retrieve.ranking_leg(K, 1, 1))
    legs = list(fns[0])
    res = {"burst": BURST, "repeats": repeats, "order": "%s first in even repetitions, %s first in odd ones" % tuple(names),
           "legs": AB.alternating_bursts(fns, legs, names, repeats, BURST)}
    res["ok"] = all(v["new_median_within_parent_max"] for v in res["legs"].values())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.build import LIB_PATH
    libs = [Lib(args.parent), Lib(args.new or LIB_PATH)]
    with contextlib.redirect_stdout(sys.stderr):        # (the tests and the benchmarks' legs print as they go)
        bits, timing = bits_leg(libs), timing_leg(libs, ("parent", "new"), args.repeats)
    rec = {"metric": "rank_refactor_ab", "parent": os.path.basename(args.parent), "new": os.path.basename(args.new or LIB_PATH),
           "bits": bits, "timing": timing, "device": torch.cuda.get_device_name(0)}
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
