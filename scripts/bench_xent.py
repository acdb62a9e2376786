"""bench_xent.py - what the generator likelihood costs (csrc/xent.hip, step.GanStep.pretrain_step / generator_step(mle_weight)):

  kernels     HipKernels.softmax_xent at (R, V) = (192, 1000) and (192, 70 000) - the 3 x 64 decoder rows of a batch-64 step at the two
              vocabularies - with the gradient (nll + hit + dlogits stored) and without (nll + hit only), `burst` back-to-back
              launches between two device events, the legs alternating; microseconds per launch (median, min .. max) and the bytes
              the algorithm moves per second: 4 R V read once, plus 4 R V written with the gradient.  These are ALGORITHMIC bytes:
              at V > 1024 the gradient pass reads the row a second time, from a cache or from HBM (not measured which), and that
              read is not counted - with it the kernel itself moves 12 R V.  Beside it the share of 6.29 TB/s, the float4-copy rate measured
              on this device (the bound of a kernel that streams from HBM; at these sizes the operands fit the Infinity Cache, so a
              share above 100 % is possible and a low one means launch / latency-bound).
              HipKernels.triple_logp at N = 64, nb = 32, M = 64 (V = 1000), the same way.
  pretrain    ms per pretraining iteration (one pretrain_step) against ms per G+D iteration (critic_iters 1), alternating in one
              process on one GanStep (two-stream schedule).
  mle_weight  ms per G+D iteration with mle_weight 0 against 0.1, alternating the same way.

    python scripts/bench_xent.py [--batch-size 64] [--size 224] [--vocab 1000] [--repeats 20] [--step-repeats 5] [--steps 10] [--out FILE]

Warm-up first; medians are reported with min .. max, the spread (max - min over the median, per cent) and every repetition.  Prints
ONE JSON line and, with --out, writes it to FILE (profiles/xent_bench.json is such a file).  Needs the GPU; reads nothing outside the
repository.
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

COPY_TBPS = 6.29            # float4 copy measured on the MI355X (the HBM bound of a streaming kernel)


def spread(xs):
    return round(100.0 * (max(xs) - min(xs)) / float(np.median(xs)), 2)


def stats(xs, digits=3):
    return {"median": round(float(np.median(xs)), digits), "min_max": [round(min(xs), digits), round(max(xs), digits)],
            "spread_pct": spread(xs), "all": [round(x, digits) for x in xs]}


def timed_legs(legs, repeats, burst):
    """{name: fn} -> {name: [us per launch] * repeats}: warm-up, then the legs alternating, `burst` launches per pair of events."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            e1.synchronize()
            us[k].append(1e3 * e0.elapsed_time(e1) / burst)
    return us


def kernel_leg(K, repeats, burst=50):
    g = torch.Generator(device=K.device).manual_seed(7)
    out = {"burst": burst, "repeats": repeats, "copy_TBps": COPY_TBPS}
    for R, V in ((192, 1000), (192, 70000)):
        x = 4.0 * torch.randn((R, V), generator=g, device=K.device)
        lab = torch.randint(0, V, (R,), generator=g, device=K.device, dtype=torch.int64)
        d = torch.empty_like(x)
        nll, hit = torch.empty(R, device=K.device), torch.empty(R, dtype=torch.int32, device=K.device)
        legs = {"with_gradient": lambda: K.softmax_xent(x, lab, scale=1.0 / 64, dlogits=d, nll=nll, hit=hit),
                "forward_only": lambda: K.softmax_xent(x, lab, nll=nll, hit=hit)}
        us = timed_legs(legs, repeats, burst)
        nbytes = {"with_gradient": 8.0 * R * V, "forward_only": 4.0 * R * V}
        rec = {}
        for k, xs in us.items():
            tbps = nbytes[k] / float(np.median(xs)) / 1e6
            rec[k] = dict(stats(xs), us="per launch", bytes=int(nbytes[k]), TBps=round(tbps, 3), share_of_copy_pct=round(100.0 * tbps / COPY_TBPS, 1))
        out["softmax_xent_R%d_V%d" % (R, V)] = rec
    N, nb, M, V = 64, 32, 64, 1000
    x = 4.0 * torch.randn((N, nb, 3, V), generator=g, device=K.device)
    lse = torch.empty((N, nb, 3), device=K.device)
    K.softmax_xent(x, None, lse=lse.view(-1))
    gt = torch.randint(0, V, (nb, M, 3), generator=g, device=K.device, dtype=torch.int64)
    cnt = torch.full((nb,), M, dtype=torch.int32, device=K.device)
    res = K.triple_logp(x, lse, gt, cnt)
    us = timed_legs({"triple_logp": lambda: K.triple_logp(x, lse, gt, cnt, out=res)}, repeats, burst)
    out["triple_logp_N%d_nb%d_M%d_V%d" % (N, nb, M, V)] = dict(stats(us["triple_logp"]), us="per launch",
                                                              gathered_words=2 * 6 * N * nb * M)
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

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        gs.flush()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    legs = {"pretrain": lambda: gs.pretrain_step(images, labels, noises[0]),
            "gd_mle0": lambda: gs.train_iteration(images, labels, noises, alphas, critic_iters=1),
            "gd_mle0.1": lambda: gs.train_iteration(images, labels, noises, alphas, critic_iters=1, mle_weight=0.1)}
    for fn in legs.values():
        run(fn)
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ms[k].append(run(fn))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    noise = max(max(x) - min(x) for x in ms.values())
    diff = med["gd_mle0.1"] - med["gd_mle0"]
    return {"critic_iters": 1, "steps_per_repetition": steps, "alternations": repeats, "schedule": "two streams",
            "ms_per_iteration": {k: stats(x, 4) for k, x in ms.items()},
            "pretrain_over_gd": round(med["pretrain"] / med["gd_mle0"], 4),
            "mle_weight_on_minus_off_ms": round(diff, 4), "largest_range_of_a_leg_ms": round(noise, 4),
            "difference_inside_the_spread": abs(diff) <= noise,
            "last_mle_losses": [round(float(x), 6) for x in gs.mle_losses.cpu().tolist()]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step-repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="skip the step legs (for a run under a kernel trace)")
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.lib import HipKernels
    K = HipKernels("cuda:0")
    B, S, V = args.batch_size, args.size, args.vocab

    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r

    rec = {"metric": "softmax_xent_us", "batch_size": B, "size": S, "vocab": V,
           "kernels": part(kernel_leg, K, args.repeats),
           "step": None if args.kernels_only else part(step_leg, K, B, S, V, args.steps, args.step_repeats),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
