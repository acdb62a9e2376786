"""bench_diagnostics.py - what the training diagnostics cost (csrc/stats.hip, sgg_amd/diagnostics.py) at the benchmark shape:

  kernel      HipKernels.arena_stats over G's four arenas (16 bytes per parameter) against HipKernels.adam on the same arenas (28 bytes
              per parameter) in the same run: bursts of launches between two HIP events, the two alternating;
  host_loop   the alternative without the kernel: torch norms of every gradient and parameter tensor in a host loop (two small
              launches per tensor) and one copy of the stacked results; wall clock round a device synchronise;
  step        ms per G+D iteration (critic_iters critic updates + one generator update, the two-stream schedule) never armed, armed
              on every iteration, and armed with GanStep.diagnostics() read after every iteration (what train.py --diagnostics_every 1
              does); the legs alternate in one process.

    python scripts/bench_diagnostics.py [--batch-size 64] [--size 224] [--vocab 1000] [--repeats 7] [--steps 10] [--out FILE]

Warm-up first; medians are reported, every repetition is kept.  Prints ONE JSON line and, with --out, writes it to FILE
(profiles/diagnostics_bench.json is such a file).  Needs the GPU; reads nothing outside the repository.
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


def spread(xs):
    return round(100.0 * (max(xs) - min(xs)) / float(np.median(xs)), 2)


def kernel_leg(K, V, S, repeats, burst=20):
    from sgg_amd import diagnostics as dg
    from sgg_amd.params import ADAM_B1, ADAM_B2, ADAM_EPS, ParamArena
    from sgg_amd.step import tf_adam_lr_t
    arena = ParamArena("G", V, S, device=K.device)
    names, offsets, numels = dg.live_layout(arena)
    n = arena.live_numel
    g = torch.Generator(device=K.device).manual_seed(7)
    p, gr, m = (torch.randn(n, generator=g, device=K.device) * s for s in (0.05, 1e-3, 1e-3))
    v = torch.rand(n, generator=g, device=K.device) * 1e-6
    table_h = dg.chunk_table(offsets, numels, K.arena_stats_chunk())
    dg.check_table(table_h, len(names), n, K.arena_stats_chunk())
    table = torch.from_numpy(table_h).to(K.device)
    ws = torch.empty(K.arena_stats_workspace_bytes(len(table_h)), dtype=torch.uint8, device=K.device)
    out = torch.empty((len(names), K.arena_stats_nstat()), dtype=torch.float64, device=K.device)
    lr_t = tf_adam_lr_t(100)
    legs = {"arena_stats": lambda: K.arena_stats(p, gr, m, v, table, len(names), lr_t, ADAM_EPS, 1.0, out=out, ws=ws),
            "adam": lambda: K.adam(p, gr, m, v, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0)}
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
    # the host loop on the same arenas: gradient and parameter norm per tensor, one copy
    views = [(gr[o:o + c], p[o:o + c]) for o, c in zip(offsets, numels)]

    def host_loop():
        return torch.stack([x.norm() for pair in views for x in pair]).cpu()

    host_loop()
    legs["arena_stats"]()           # (the rows of the arenas as the host loop sees them)
    host = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        norms = host_loop()
        host.append(1e3 * (time.perf_counter() - t0))
    rows = out.cpu().numpy()
    same = bool(np.allclose(np.sqrt(rows[:, 3]), norms.numpy()[1::2].astype(np.float64), rtol=1e-4))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    return {"tensors": len(names), "chunks": int(len(table_h)), "parameters": int(n), "burst": burst,
            "arena_stats_ms": round(med["arena_stats"], 5), "adam_ms": round(med["adam"], 5),
            "arena_stats_GBps": round(16.0 * n / med["arena_stats"] / 1e6, 1), "adam_GBps": round(28.0 * n / med["adam"] / 1e6, 1),
            "arena_stats_over_adam": round(med["arena_stats"] / med["adam"], 4), "arena_stats_not_slower": med["arena_stats"] <= med["adam"],
            "spread_pct": {k: spread(x) for k, x in ms.items()}, "ms_all": {k: [round(y, 5) for y in x] for k, x in ms.items()},
            "host_loop": {"what": "torch .norm() of every gradient and parameter tensor + one stacked copy (2 of the 9 statistics)",
                          "launches": 2 * len(names) + 1, "ms_wall": round(float(np.median(host)), 4), "ms_all": [round(x, 4) for x in host],
                          "param_norms_agree": same}}


def step_leg(K, B, S, V, critic_iters, steps, repeats):
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), overlap_streams=True)
    g = torch.Generator().manual_seed(11)
    images = torch.randn((B, S, S, 3), generator=g).to(K.device)
    labels = torch.randint(0, V, (B, 3), generator=g, dtype=torch.int64).to(K.device)
    noises = [torch.randn((B, 512), generator=g).to(K.device) for _ in range(critic_iters + 1)]
    alphas = [torch.rand((B,), generator=g).to(K.device) for _ in range(critic_iters)]

    def run(armed, read):
        gs.arm_diagnostics(armed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            gs.train_iteration(images, labels, noises, alphas, critic_iters=critic_iters)
            if read:
                gs.diagnostics()
        gs.flush()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    legs = {"never_armed": (False, False), "armed": (True, False), "armed_and_read": (True, True)}
    for a in legs.values():
        run(*a)
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, a in legs.items():
            ms[k].append(run(*a))
    gs.arm_diagnostics(False)
    med = {k: float(np.median(x)) for k, x in ms.items()}
    return {"critic_iters": critic_iters, "steps_per_repetition": steps, "schedule": "two streams",
            "ms_per_iteration": {k: round(x, 4) for k, x in med.items()},
            "armed_minus_never_ms": round(med["armed"] - med["never_armed"], 4),
            "armed_and_read_minus_never_ms": round(med["armed_and_read"] - med["never_armed"], 4),
            "spread_pct": {k: spread(x) for k, x in ms.items()}, "ms_all": {k: [round(y, 4) for y in x] for k, x in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--critic-iters", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=7)
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

    rec = {"metric": "arena_stats_ms", "batch_size": B, "size": S, "vocab": V, "repeats": args.repeats,
           "kernel": part(kernel_leg, K, V, S, args.repeats), "step": part(step_leg, K, B, S, V, args.critic_iters, args.steps, args.repeats),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
