"""bench_accumulate.py - what gradient accumulation costs (csrc/optim.hip: grad_accumulate_kernel; step.Network.end_micro_batch,
GanStep.train_iteration_accumulated):

  kernels     on G's live arena for vocab 1000 and vocab 70 000 at 224 x 224, in one run, the legs alternating:
                adam              HipKernels.adam (adam_kernel)                                 7 n words
                accumulate        HipKernels.grad_accumulate(acc, g)         acc += g           3 n words
                accumulate_first  HipKernels.grad_accumulate(acc, g, True)   acc  = g           2 n words
              bursts of launches between two device events; ms per call and GB/s from the words above.  The pass moves 3 streams
              against Adam's 7: it must take less time than adam_kernel in the same run (`accumulate_faster_than_adam`).
  iterations  ms per iteration and triples/s (B * N rows per iteration) of (B, N) = (64, 1), (32, 2), (64, 2), (64, 8) at 224 x 224,
              vocab 1000, critic_iters 1 and 10, G-encoder reuse on and off, on the two-stream schedule, the legs alternating; and
              the share of an iteration spent in the accumulate pass: the device time of its launches from the timing hook
              (HipKernels.timing, label grad_accumulate_kernel) over one separately run iteration, against the untimed median.

    python scripts/bench_accumulate.py [--size 224] [--vocab 1000] [--big-vocab 70000] [--repeats 20] [--step-repeats 3] [--steps 1]
                                       [--critic-iters 1,10] [--configs 64x1,32x2,64x2,64x8] [--out FILE]

One device: the figures say what N micro-batches cost on it, they are no scaling curve.  Warm-up first; medians with every
repetition.  Prints ONE JSON line and writes it to --out (default profiles/accumulate_bench.json).  Needs the GPU; reads nothing
outside the repository.
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

WORDS = {"adam": 7, "accumulate": 3, "accumulate_first": 2}


def spread(xs):
    return round(100.0 * (max(xs) - min(xs)) / float(np.median(xs)), 2)


def kernel_leg(K, V, S, repeats, burst=10):
    from sgg_amd.params import ADAM_B1, ADAM_B2, ADAM_EPS, ParamArena
    from sgg_amd.step import tf_adam_lr_t
    n = ParamArena("G", V, S, device="meta").live_numel
    g = torch.Generator(device=K.device).manual_seed(7)
    p, gr, m, acc = (torch.randn(n, generator=g, device=K.device) * s for s in (0.05, 1e-3, 1e-3, 1e-3))
    v = torch.rand(n, generator=g, device=K.device) * 1e-6
    lr_t = tf_adam_lr_t(100)
    legs = {"adam": lambda: K.adam(p, gr, m, v, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0),
            "accumulate": lambda: K.grad_accumulate(acc, gr), "accumulate_first": lambda: K.grad_accumulate(acc, gr, first=True)}
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
            "accumulate_over_adam": round(med["accumulate"] / med["adam"], 4),
            "accumulate_faster_than_adam": max(ms["accumulate"]) < min(ms["adam"]),
            "spread_pct": {k: spread(x) for k, x in ms.items()}, "ms_all": {k: [round(y, 5) for y in x] for k, x in ms.items()}}


def iteration_legs(K, S, V, configs, critic_iters, steps, repeats):
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    g = torch.Generator().manual_seed(11)
    steps_by_B, legs = {}, {}
    for B, N in configs:
        if B not in steps_by_B:
            steps_by_B[B] = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S),
                                    overlap_streams=True)
        batches = [(torch.randn((B, S, S, 3), generator=g).to(K.device),
                    torch.randint(0, V, (B, 3), generator=g, dtype=torch.int64).to(K.device)) for _ in range(N)]
        noises = [[torch.randn((B, 512), generator=g).to(K.device) for _ in range(N)] for _ in range(critic_iters + 1)]
        alphas = [[torch.rand((B,), generator=g).to(K.device) for _ in range(N)] for _ in range(critic_iters)]
        for reuse in (True, False):
            legs[(B, N, reuse)] = (steps_by_B[B], batches, noises, alphas)

    def run(key, n_steps):
        gs, batches, noises, alphas = legs[key]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            gs.train_iteration_accumulated(batches, noises, alphas, critic_iters=critic_iters, reuse_g_encoder=key[2])
        gs.flush()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n_steps

    for key in legs:
        run(key, 1)
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for key in legs:
            ms[key].append(run(key, steps))
    # the accumulate pass's device time over one iteration of each leg, from the timing hook (every launch is then bracketed by
    # events: this iteration is not one of the timed ones)
    acc_ms = {}
    for key in legs:
        K.timing, K.timing_conv_only = [], False
        try:
            run(key, 1)
            acc_ms[key] = sum(e0.elapsed_time(e1) for sym, _, _, e0, e1 in K.timing if sym == "grad_accumulate_kernel")
            acc_n = sum(sym == "grad_accumulate_kernel" for sym, _, _, _, _ in K.timing)
        finally:
            K.timing = None
        acc_ms[key] = (acc_ms[key], acc_n)
    out = []
    for (B, N, reuse), x in ms.items():
        med = float(np.median(x))
        out.append({"B": B, "N": N, "rows_per_update": B * N, "reuse_g_encoder": reuse, "critic_iters": critic_iters,
                    "ms_per_iteration": round(med, 3), "triples_per_s": round(1e3 * B * N / med, 1),
                    "accumulate_pass_ms": round(acc_ms[(B, N, reuse)][0], 4), "accumulate_launches": acc_ms[(B, N, reuse)][1],
                    "accumulate_share_pct": round(100.0 * acc_ms[(B, N, reuse)][0] / med, 3),
                    "spread_pct": spread(x), "ms_all": [round(y, 3) for y in x]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--big-vocab", type=int, default=70000)
    ap.add_argument("--critic-iters", default="1,10")
    ap.add_argument("--configs", default="64x1,32x2,64x2,64x8", help="BxN pairs")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_bench.json"))
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.lib import HipKernels
    K = HipKernels("cuda:0")
    S, V = args.size, args.vocab
    configs = [tuple(int(x) for x in c.split("x")) for c in args.configs.split(",") if c.strip()]

    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r

    rec = {"metric": "grad_accumulate_ms", "size": S, "vocab": V, "schedule": "two streams", "scope": "one device; not a scaling curve",
           "kernels": [part(kernel_leg, K, v, S, args.repeats) for v in (V, args.big_vocab)],
           "iterations": [r for ci in args.critic_iters.split(",") if ci.strip()
                          for r in part(iteration_legs, K, S, V, configs, int(ci), args.steps, args.step_repeats)],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
