"""bench_relax_hard.py - what the straight-through (hard) relaxation costs (csrc/relax.hip, step.GanStep.set_relaxation(hard=True)):

  kernels     HipKernels.relax_rows_hard and relax_rows_hard_bwd, plain and with Gumbel noise, at (R, V) = (192, 1000), (192, 70 000)
              and (24 576, 1000) - the shapes of scripts/bench_relax.py - BESIDE the soft kernels in the same run, the legs
              alternating: relax_rows in both modes and relax_rows_bwd are the yardstick, not a fixed number.  The harness of
              scripts/bench_xent.py: `burst` (50) back-to-back launches between two device events, 20 alternating repetitions;
              microseconds per launch (median, min .. max) and the ALGORITHMIC bytes per second: forwards 8 R V (x read once, y
              written), soft backward 12 R V (y, dy read, dx written), hard backward 12 R V (x, dy read, dx written; its second
              read of both rows at V > 1024 is not counted, as for the soft kernels).
              One condition follows from the work done and is evaluated here ("hard_gumbel_forward_within_soft"): at (192, 70 000)
              with noise the hard forward draws once and takes no exp where the soft one draws twice, so its median must not exceed
              the soft Gumbel forward's by more than that leg's own range (max - min).
  step        ms per G+D iteration (critic_iters 1, two-stream schedule) with generator_output gumbel soft and gumbel hard,
              alternating five times in one process on one GanStep.

    python scripts/bench_relax_hard.py [--batch-size 64] [--size 224] [--vocab 1000] [--repeats 20] [--step-repeats 5] [--steps 10]
                                       [--out FILE]

Prints ONE JSON line and, with --out, writes it to FILE (profiles/relax_hard_bench.json is such a file).  Needs the GPU; reads nothing
outside the repository.  Whether hard rows improve recall is not measured here or anywhere.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_xent import COPY_TBPS, stats, timed_legs  # noqa: E402


def kernel_leg(K, repeats, burst=50, eval_rows=24576):
    g = torch.Generator(device=K.device).manual_seed(7)
    out = {"burst": burst, "repeats": repeats, "copy_TBps": COPY_TBPS}
    for R, V in ((192, 1000), (192, 70000), (eval_rows, 1000)):
        x = 4.0 * torch.randn((R, V), generator=g, device=K.device)
        dy = torch.randn((R, V), generator=g, device=K.device)
        y, d = torch.empty_like(x), torch.empty_like(x)
        ys = K.relax_rows(x, 0.5, y=torch.empty_like(x), gumbel=True, seed=11, draw=5)
        nz = {"gumbel": True, "seed": 11, "draw": 5}
        legs = {"soft_softmax": lambda: K.relax_rows(x, 0.5, y=y),
                "soft_gumbel": lambda: K.relax_rows(x, 0.5, y=y, **nz),
                "soft_bwd": lambda: K.relax_rows_bwd(ys, dy, 0.5, scale=1.0, dx=d),
                "hard_softmax": lambda: K.relax_rows_hard(x, y=y),
                "hard_gumbel": lambda: K.relax_rows_hard(x, y=y, **nz),
                "hard_bwd_softmax": lambda: K.relax_rows_hard_bwd(x, dy, 0.5, scale=1.0, dx=d),
                "hard_bwd_gumbel": lambda: K.relax_rows_hard_bwd(x, dy, 0.5, scale=1.0, dx=d, **nz)}
        nbytes = {k: (12.0 if "bwd" in k else 8.0) * R * V for k in legs}
        us = timed_legs(legs, repeats, burst)
        rec = {}
        for k, xs in us.items():
            tbps = nbytes[k] / float(np.median(xs)) / 1e6
            rec[k] = dict(stats(xs), us="per launch", bytes=int(nbytes[k]), TBps=round(tbps, 3), share_of_copy_pct=round(100.0 * tbps / COPY_TBPS, 1))
        for hard, soft in (("hard_softmax", "soft_softmax"), ("hard_gumbel", "soft_gumbel"), ("hard_bwd_softmax", "soft_bwd"),
                           ("hard_bwd_gumbel", "soft_bwd")):
            rec[hard]["time_over_" + soft] = round(rec[hard]["median"] / rec[soft]["median"], 3)
        rec["hard_bwd_gumbel"]["time_over_soft_gumbel"] = round(rec["hard_bwd_gumbel"]["median"] / rec["soft_gumbel"]["median"], 3)
        out["R%d_V%d" % (R, V)] = rec
    big = out["R192_V70000"]
    soft = big["soft_gumbel"]
    spread = soft["min_max"][1] - soft["min_max"][0]
    out["hard_gumbel_forward_within_soft"] = {"shape": "R192_V70000", "hard_median_us": big["hard_gumbel"]["median"],
                                              "soft_median_us": soft["median"], "soft_range_us": round(spread, 3),
                                              "holds": bool(big["hard_gumbel"]["median"] <= soft["median"] + spread)}
    return out


def step_leg(K, B, S, V, steps, repeats):
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), overlap_streams=True)
    g = torch.Generator().manual_seed(11)
    images = torch.randn((B, S, S, 3), generator=g).to(K.device)
    labels = torch.randint(0, V, (B, 3), generator=g, dtype=torch.int64).to(K.device)
    noises = [torch.randn((B, 512), generator=g).to(K.device) for _ in range(2)]
    alphas = [torch.rand((B,), generator=g).to(K.device)]
    count = [0]

    def iteration(hard):
        gs.set_relaxation("gumbel", 0.5, 3, hard=hard)
        count[0] += 1
        gs.train_iteration(images, labels, noises, alphas, critic_iters=1, draws=[2 * count[0], 2 * count[0] + 1])

    def run(hard):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            iteration(hard)
        gs.flush()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    modes = (("gumbel_soft", False), ("gumbel_hard", True))
    for _, h in modes:
        run(h)
    ms = {m: [] for m, _ in modes}
    for _ in range(repeats):
        for m, h in modes:
            ms[m].append(run(h))
    med = {m: float(np.median(x)) for m, x in ms.items()}
    return {"critic_iters": 1, "steps_per_repetition": steps, "alternations": repeats, "schedule": "two streams", "tau": 0.5,
            "ms_per_iteration": {m: stats(x, 4) for m, x in ms.items()},
            "hard_minus_soft_ms": round(med["gumbel_hard"] - med["gumbel_soft"], 4),
            "largest_range_of_a_leg_ms": round(max(max(x) - min(x) for x in ms.values()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--eval-rows", type=int, default=24576)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="skip the step legs")
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.lib import HipKernels
    K = HipKernels("cuda:0")
    B, S, V = args.batch_size, args.size, args.vocab

    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r

    rec = {"metric": "relax_rows_hard_us", "batch_size": B, "size": S, "vocab": V,
           "kernels": part(kernel_leg, K, args.repeats, 50, args.eval_rows),
           "step": None if args.kernels_only else part(step_leg, K, B, S, V, args.steps, args.step_repeats),
           "recall": "not measured", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
