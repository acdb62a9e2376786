"""bench_ema.py - what averaging the generator's weights costs (csrc/optim.hip, sgg_amd/ema.py, step.Network.enable_averaging):

  kernels     on G's live arena for vocab 1000 and vocab 70 000 at 224 x 224, in one run, the legs alternating:
                adam           HipKernels.adam (adam_kernel)                                  7 n words
                adam_ema       HipKernels.adam_ema, the fused step                            9 n words
                adam_then_ema  HipKernels.adam followed by a separate averaging pass          10 n words moved, rated at 9 n
                               (torch's one-launch elementwise e.lerp_(p, 1 - decay) as the stand-in for such a kernel)
                swap           HipKernels.swap (Network.averaged())                           4 n words
              bursts of launches between two device events; ms per call and GB/s from the words above;
  step        ms per G+D iteration (critic_iters critic updates + one generator update, the two-stream schedule) with averaging off
              and on, the two alternating in one process on one GanStep.

    python scripts/bench_ema.py [--batch-size 64] [--size 224] [--vocab 1000] [--big-vocab 70000] [--repeats 20] [--step-repeats 5]
                                [--steps 10] [--out FILE]

Warm-up first; medians are reported with the spread (max - min over the median, per cent) and every repetition.  Prints ONE JSON line
and, with --out, writes it to FILE (profiles/ema_bench.json is such a file).  Needs the GPU; reads nothing outside the repository.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORDS = {"adam": 7, "adam_ema": 9, "adam_then_ema": 9, "swap": 4}


def spread(xs):
    return round(100.0 * (max(xs) - min(xs)) / float(np.median(xs)), 2)


def kernel_leg(K, V, S, repeats, burst=10):
    from sgg_amd.params import ADAM_B1, ADAM_B2, ADAM_EPS, ParamArena
    from sgg_amd.step import tf_adam_lr_t
    n = ParamArena("G", V, S, device="meta").live_numel
    g = torch.Generator(device=K.device).manual_seed(7)
    p, gr, m, e = (torch.randn(n, generator=g, device=K.device) * s for s in (0.05, 1e-3, 1e-3, 0.05))
    v = torch.rand(n, generator=g, device=K.device) * 1e-6
    other = torch.randn(n, generator=g, device=K.device)
    lr_t, omd = tf_adam_lr_t(100), 1e-3
    adam = lambda: K.adam(p, gr, m, v, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0)

    def adam_then_ema():
        adam()
        e.lerp_(p, omd)

    legs = {"adam": adam, "adam_ema": lambda: K.adam_ema(p, gr, m, v, e, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0, omd),
            "adam_then_ema": adam_then_ema, "swap": lambda: K.swap(e, other)}
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
    return {"vocab": V, "parameters": int(n), "burst": burst, "repeats": repeats,
            "ms": {k: round(x, 5) for k, x in med.items()},
            "GBps": {k: round(4.0 * WORDS[k] * n / med[k] / 1e6, 1) for k in legs},
            "fused_over_adam": round(med["adam_ema"] / med["adam"], 4),
            "fused_over_separate": round(med["adam_ema"] / med["adam_then_ema"], 4),
            "fused_faster_than_separate": med["adam_ema"] < med["adam_then_ema"],
            "spread_pct": {k: spread(x) for k, x in ms.items()}, "ms_all": {k: [round(y, 5) for y in x] for k, x in ms.items()}}


def step_leg(K, B, S, V, critic_iters, steps, repeats, decay=0.999):
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), overlap_streams=True)
    g = torch.Generator().manual_seed(11)
    images = torch.randn((B, S, S, 3), generator=g).to(K.device)
    labels = torch.randint(0, V, (B, 3), generator=g, dtype=torch.int64).to(K.device)
    noises = [torch.randn((B, 512), generator=g).to(K.device) for _ in range(critic_iters + 1)]
    alphas = [torch.rand((B,), generator=g).to(K.device) for _ in range(critic_iters)]

    def run(on):
        if on:                          # (the buffer is allocated and freed outside the timed region)
            gs.G.enable_averaging(decay)
        else:
            gs.G.disable_averaging()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            gs.train_iteration(images, labels, noises, alphas, critic_iters=critic_iters)
        gs.flush()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    legs = {"off": False, "on": True}
    for on in legs.values():
        run(on)
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, on in legs.items():
            ms[k].append(run(on))
    gs.G.disable_averaging()
    med = {k: float(np.median(x)) for k, x in ms.items()}
    diff = med["on"] - med["off"]
    noise = max(max(x) - min(x) for x in ms.values())
    return {"critic_iters": critic_iters, "steps_per_repetition": steps, "alternations": repeats, "schedule": "two streams", "decay": decay,
            "ms_per_iteration": {k: round(x, 4) for k, x in med.items()}, "on_minus_off_ms": round(diff, 4),
            "largest_range_of_a_leg_ms": round(noise, 4), "difference_inside_the_spread": abs(diff) <= noise,
            "spread_pct": {k: spread(x) for k, x in ms.items()}, "ms_all": {k: [round(y, 4) for y in x] for k, x in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--big-vocab", type=int, default=70000)
    ap.add_argument("--critic-iters", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.lib import HipKernels
    K = HipKernels("cuda:0")
    B, S, V = args.batch_size, args.size, args.vocab

    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r

    rec = {"metric": "adam_ema_ms", "batch_size": B, "size": S, "vocab": V,
           "kernels": [part(kernel_leg, K, v, S, args.repeats) for v in (V, args.big_vocab)],
           "step": part(step_leg, K, B, S, V, args.critic_iters, args.steps, args.step_repeats),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
