"""bench_augment.py - what training-time augmentation costs (csrc/augment.hip, sgg_amd/augment.py, PrefetchLoader(augment=...)):

  kernels   on one packed batch of 64 random 640 x 480 images -> 221 x 221, in one run, the legs alternating:
              resize      HipKernels.resize_bilinear_tf1, the launch a run without --augment makes
              crop        augment_plan + augment_resize with crop=0.5,flip=0.5 (no colour stage, no grey sum)
              all         augment_plan + augment_resize with every stage on (plan, grey sum, grey mean, resize)
            bursts of calls between two device events; ms per call, and GB/s of the 12 bytes written per output pixel;
  loader    batches/s of PrefetchLoader on generated Visual-Genome-sized JPEGs (as scripts/loader_rate.py) with augmentation off and
            on, the two alternating;
  step      ms per G+D iteration (one critic update + one generator update, two streams) fed by that loader, off and on, alternating.

    python scripts/bench_augment.py [--repeats 20] [--loader-repeats 3] [--step-repeats 5] [--steps 10] [--images 256] [--out FILE]

Warm-up first; medians with the range of every leg and every repetition.  Prints ONE JSON line and, with --out, writes it to FILE
(profiles/augment_bench.json is such a file).  Needs the GPU; reads nothing outside the repository."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SPEC_CROP = "crop=0.5,flip=0.5"
SPEC_ALL = "crop=0.5,flip=0.5,brightness=0.2,contrast=0.2,saturation=0.2"
MEANS, STDS = [120.0, 115.0, 100.0], [60.0, 58.0, 61.0]


def spread(xs):
    return round(100.0 * (max(xs) - min(xs)) / float(np.median(xs)), 2)


def kernel_leg(K, repeats, B=64, H=480, W=640, side=221, burst=10):
    from sgg_amd.augment import AugmentSpec
    dev = K.device
    g = torch.Generator(device=dev).manual_seed(3)
    packed = torch.randint(0, 256, (B * H * W * 3,), generator=g, device=dev, dtype=torch.uint8)
    offs = (torch.arange(B, device=dev, dtype=torch.int64) * (H * W * 3)).contiguous()
    hs, ws = torch.full((B,), H, dtype=torch.int32, device=dev), torch.full((B,), W, dtype=torch.int32, device=dev)
    labels = torch.zeros((B, 3), dtype=torch.int64, device=dev)
    swap = torch.arange(8, dtype=torch.int32, device=dev)
    out = torch.empty((B, side, side, 3), device=dev)
    box, fac, lab = torch.empty((B, 6), dtype=torch.int32, device=dev), torch.empty((B, 4), device=dev), torch.empty_like(labels)
    means, stds = torch.tensor(MEANS, device=dev), torch.tensor(STDS, device=dev)
    draw = [0]

    def augmented(spec):
        spec = AugmentSpec.parse(spec)

        def fn():
            draw[0] += B
            K.augment_plan(packed, offs, hs, ws, labels, swap, spec.quantised(), 1, draw[0], box, fac, lab)
            K.augment_resize(packed, offs, hs, ws, box, fac, spec.stages, out, means, stds)
        return fn
    legs = {"resize": lambda: K.resize_bilinear_tf1(packed, offs, hs, ws, out, means, stds), "crop": augmented(SPEC_CROP),
            "all": augmented(SPEC_ALL)}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / burst)
    med = {k: float(np.median(x)) for k, x in ms.items()}
    written = 12.0 * B * side * side
    return {"batch": B, "source": [H, W], "side": side, "burst": burst, "repeats": repeats, "specs": {"crop": SPEC_CROP, "all": SPEC_ALL},
            "ms": {k: round(x, 5) for k, x in med.items()}, "written_GBps": {k: round(written / med[k] / 1e6, 1) for k in legs},
            "source_bytes": B * H * W * 3, "written_bytes": int(written),
            "range_ms": {k: [round(min(x), 5), round(max(x), 5)] for k, x in ms.items()},
            "spread_pct": {k: spread(x) for k, x in ms.items()}, "ms_all": {k: [round(y, 5) for y in x] for k, x in ms.items()}}


def make_files(n):
    from PIL import Image
    d = tempfile.mkdtemp(prefix="augment_bench_")
    rng = np.random.RandomState(0)
    files = []
    for i in range(n):
        arr = (rng.rand(375, 500, 3) * 255).astype(np.uint8)          # a typical Visual Genome frame (scripts/loader_rate.py)
        arr = (0.5 * arr + 0.5 * np.roll(arr, 1, axis=0)).astype(np.uint8)
        p = os.path.join(d, "im%04d.jpg" % i)
        Image.fromarray(arr).save(p, quality=90)
        files.append(p)
    return files, rng.randint(0, 1000, (n, 3))


def make_loader(files, labels, B, iters, spec, workers):
    from sgg_amd.data import PrefetchLoader
    n = len(files)
    kw = {} if spec is None else {"augment": spec, "seed": 1, "swap": np.arange(1000, dtype=np.int32)}
    return PrefetchLoader(files, labels, B, lambda it: [(it * B + j) % n for j in range(B)], MEANS, STDS, "cuda:0", iters, workers=workers,
                          **kw)


def loader_leg(files, labels, repeats, B=64, iters=22, workers=16):
    legs = {"off": None, "on": SPEC_ALL}
    rate = {k: [] for k in legs}
    for _ in range(repeats):
        for k, spec in legs.items():
            with make_loader(files, labels, B, iters, spec, workers) as loader:
                next(loader); next(loader)                             # first batches: worker start-up
                t0, n = time.perf_counter(), 0
                for _images, _labels in loader:
                    n += 1
                torch.cuda.synchronize()
                rate[k].append(n / (time.perf_counter() - t0))
    med = {k: float(np.median(x)) for k, x in rate.items()}
    return {"batch": B, "batches_timed": iters - 2, "workers": workers, "host_cores": len(os.sched_getaffinity(0)), "spec": SPEC_ALL,
            "batches_per_s": {k: round(x, 2) for k, x in med.items()}, "ms_per_batch": {k: round(1e3 / x, 2) for k, x in med.items()},
            "range": {k: [round(min(x), 2), round(max(x), 2)] for k, x in rate.items()},
            "all": {k: [round(y, 2) for y in x] for k, x in rate.items()}}


def step_leg(K, files, labels, steps, repeats, B=64, S=221, V=1000, workers=16):
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), overlap_streams=True)
    g = torch.Generator().manual_seed(11)
    noises = [torch.randn((B, 512), generator=g).to(K.device) for _ in range(2)]
    alphas = [torch.rand((B,), generator=g).to(K.device)]

    def run(spec):
        with make_loader(files, labels, B, steps + 2, spec, workers) as loader:
            for _ in range(2):                                         # worker start-up, and the step's own warm-up
                images, labs = next(loader)
                gs.train_iteration(images, labs, noises, alphas, critic_iters=1)
            gs.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for images, labs in loader:
                gs.train_iteration(images, labs, noises, alphas, critic_iters=1)
            gs.flush()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / steps
    legs = {"off": None, "on": SPEC_ALL}
    for spec in legs.values():
        run(spec)
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, spec in legs.items():
            ms[k].append(run(spec))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    diff, noise = med["on"] - med["off"], max(max(x) - min(x) for x in ms.values())
    return {"critic_iters": 1, "steps_per_repetition": steps, "alternations": repeats, "schedule": "two streams", "batch": B, "size": S,
            "vocab": V, "fed_by": "PrefetchLoader, %d decode threads" % workers, "spec": SPEC_ALL,
            "ms_per_iteration": {k: round(x, 3) for k, x in med.items()}, "on_minus_off_ms": round(diff, 3),
            "largest_range_of_a_leg_ms": round(noise, 3), "difference_inside_the_spread": abs(diff) <= noise,
            "spread_pct": {k: spread(x) for k, x in ms.items()}, "ms_all": {k: [round(y, 3) for y in x] for k, x in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loader-repeats", type=int, default=3)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.lib import HipKernels
    K = HipKernels("cuda:0")

    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r
    files, labels = make_files(args.images)
    rec = {"metric": "augment_ms", "kernels": part(kernel_leg, K, args.repeats),
           "loader": part(loader_leg, files, labels, args.loader_repeats, 64, 22, args.workers),
           "step": part(step_leg, K, files, labels, args.steps, args.step_repeats, 64, 221, 1000, args.workers),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for p in files:
        os.remove(p)
    os.rmdir(os.path.dirname(files[0]))


if __name__ == "__main__":
    main()
