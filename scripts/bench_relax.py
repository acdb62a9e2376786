"""bench_relax.py - what the relaxed generator output costs (csrc/relax.hip, step.GanStep.set_relaxation):

  kernels     HipKernels.relax_rows, plain and with Gumbel noise, at (R, V) = (192, 1000) and (192, 70 000) - the 3 x 64 decoder rows
              of a batch-64 step at the two vocabularies - and in place at (24 576, 1000), the 256 samples x 32 images x 3 rows of an
              evaluation pass at batch 64; HipKernels.relax_rows_bwd at the first two shapes.  The harness of scripts/bench_xent.py:
              `burst` back-to-back launches between two device events, the legs alternating; microseconds per launch (median,
              min .. max) and the ALGORITHMIC bytes per second: forward 8 R V (x read once, y written), backward 12 R V (y and dy read
              once, dx written).  At V > 1024 both kernels read their inputs a second time, from a cache or from HBM (not measured
              which); that read is not counted.  The yardstick is softmax_xent at the same shapes in the same run, its legs
              alternating with these: with the gradient (8 R V) and forward only (4 R V) - not a fixed number.
  step        ms per G+D iteration (critic_iters 1, two-stream schedule) with generator_output logits / softmax / gumbel, alternating
              in one process on one GanStep.  The logits leg launches nothing new; --parent-bench FILE takes the JSON line that
              scripts/bench_xent.py of the PARENT commit printed in the same session and puts its "gd_mle0" figure - the same
              iteration - beside it.

    python scripts/bench_relax.py [--batch-size 64] [--size 224] [--vocab 1000] [--repeats 20] [--step-repeats 5] [--steps 10]
                                  [--parent-bench FILE] [--out FILE]

Prints ONE JSON line and, with --out, writes it to FILE (profiles/relax_bench.json is such a file).  Needs the GPU; reads nothing
outside the repository.  Whether the relaxation improves recall is not measured here or anywhere.
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
    for R, V, train in ((192, 1000, True), (192, 70000, True), (eval_rows, 1000, False)):
        x = 4.0 * torch.randn((R, V), generator=g, device=K.device)
        lab = torch.randint(0, V, (R,), generator=g, device=K.device, dtype=torch.int64)
        y, d = torch.empty_like(x), torch.empty_like(x)
        nll, hit = torch.empty(R, device=K.device), torch.empty(R, dtype=torch.int32, device=K.device)
        K.relax_rows(x, 0.5, y=y)
        dy = torch.randn((R, V), generator=g, device=K.device)
        legs = {"xent_with_gradient": lambda: K.softmax_xent(x, lab, scale=1.0 / 64, dlogits=d, nll=nll, hit=hit),
                "xent_forward_only": lambda: K.softmax_xent(x, lab, nll=nll, hit=hit)}
        nbytes = {"xent_with_gradient": 8.0 * R * V, "xent_forward_only": 4.0 * R * V}
        if train:
            legs["relax_softmax"] = lambda: K.relax_rows(x, 0.5, y=y)
            legs["relax_gumbel"] = lambda: K.relax_rows(x, 0.5, y=y, gumbel=True, seed=11, draw=5)
            legs["relax_bwd"] = lambda: K.relax_rows_bwd(y, dy, 0.5, scale=1.0, dx=d)
            nbytes.update(relax_softmax=8.0 * R * V, relax_gumbel=8.0 * R * V, relax_bwd=12.0 * R * V)
        else:
            # in place, as the evaluation does; a relaxed row is a valid input again (softmax of values in [0, 1])
            z = x.clone()
            legs["relax_softmax_in_place"] = lambda: K.relax_rows(z, 0.5)
            nbytes["relax_softmax_in_place"] = 8.0 * R * V
        us = timed_legs(legs, repeats, burst)
        rec = {}
        for k, xs in us.items():
            tbps = nbytes[k] / float(np.median(xs)) / 1e6
            rec[k] = dict(stats(xs), us="per launch", bytes=int(nbytes[k]), TBps=round(tbps, 3), share_of_copy_pct=round(100.0 * tbps / COPY_TBPS, 1))
        for k in rec:
            if k.startswith("relax"):
                rec[k]["rate_over_xent_with_gradient"] = round(rec[k]["TBps"] / rec["xent_with_gradient"]["TBps"], 3)
        out["R%d_V%d" % (R, V)] = rec
    return out


def step_leg(K, B, S, V, steps, repeats, parent=None):
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), overlap_streams=True)
    g = torch.Generator().manual_seed(11)
    images = torch.randn((B, S, S, 3), generator=g).to(K.device)
    labels = torch.randint(0, V, (B, 3), generator=g, dtype=torch.int64).to(K.device)
    noises = [torch.randn((B, 512), generator=g).to(K.device) for _ in range(2)]
    alphas = [torch.rand((B,), generator=g).to(K.device)]
    count = [0]

    def iteration(mode):
        gs.set_relaxation(mode, 0.5, 3)
        count[0] += 1
        gs.train_iteration(images, labels, noises, alphas, critic_iters=1, draws=[2 * count[0], 2 * count[0] + 1])

    def run(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            iteration(mode)
        gs.flush()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    modes = ("logits", "softmax", "gumbel")
    for m in modes:
        run(m)
    ms = {m: [] for m in modes}
    for _ in range(repeats):
        for m in modes:
            ms[m].append(run(m))
    med = {m: float(np.median(x)) for m, x in ms.items()}
    noise = max(max(x) - min(x) for x in ms.values())
    rec = {"critic_iters": 1, "steps_per_repetition": steps, "alternations": repeats, "schedule": "two streams", "tau": 0.5,
           "ms_per_iteration": {m: stats(x, 4) for m, x in ms.items()},
           "softmax_minus_logits_ms": round(med["softmax"] - med["logits"], 4),
           "gumbel_minus_logits_ms": round(med["gumbel"] - med["logits"], 4),
           "largest_range_of_a_leg_ms": round(noise, 4)}
    if parent is not None:
        p = parent["step"]["ms_per_iteration"]["gd_mle0"]
        rec["parent_commit_gd_ms"] = p
        rec["logits_minus_parent_ms"] = round(med["logits"] - p["median"], 4)
        lo = min(min(ms["logits"]), p["min_max"][0])
        hi = max(max(ms["logits"]), p["min_max"][1])
        rec["logits_median_inside_parents_range"] = p["min_max"][0] <= med["logits"] <= p["min_max"][1]
        rec["ranges_overlap"] = not (min(ms["logits"]) > p["min_max"][1] or max(ms["logits"]) < p["min_max"][0])
        rec["joint_range_ms"] = [round(lo, 4), round(hi, 4)]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--eval-rows", type=int, default=24576)
    ap.add_argument("--parent-bench", default=None, help="the JSON line of the parent commit's scripts/bench_xent.py from the same session")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="skip the step legs")
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.lib import HipKernels
    K = HipKernels("cuda:0")
    B, S, V = args.batch_size, args.size, args.vocab
    parent = None
    if args.parent_bench:
        with open(args.parent_bench) as f:
            parent = json.loads(f.readline())

    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r

    rec = {"metric": "relax_rows_us", "batch_size": B, "size": S, "vocab": V,
           "kernels": part(kernel_leg, K, args.repeats, 50, args.eval_rows),
           "step": None if args.kernels_only else part(step_leg, K, B, S, V, args.steps, args.step_repeats, parent),
           "recall": "not measured", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
