"""bench_score.py - what the score-function generator update costs (csrc/score.hip, step.GanStep.set_estimator("score")):

  kernels     HipKernels.score_rows with ent_coef 0 and 0.01 at (R, V) = (192, 1000), (192, 70 000) and (24 576, 1000) - the shapes of
              scripts/bench_relax_hard.py - BESIDE softmax_xent with its gradient in the same run, the legs alternating: the
              likelihood's launch is the yardstick, not a fixed number.  score_advantage and score_summary at B = 64 (192 rows).  The
              harness of scripts/bench_xent.py: `burst` (50) back-to-back launches between two device events, 20 alternating
              repetitions; microseconds per launch (median, min .. max) and the ALGORITHMIC bytes per second, 8 R V (x read once, dx
              written; the gradient pass's second read of a streamed row is not counted, as for softmax_xent).
              One condition follows from the work done and is evaluated here ("score_rows_within_softmax_xent"): at (192, 70 000)
              score_rows with ent_coef = 0 moves the bytes of softmax_xent with its gradient and adds one FMA per element, so its
              median must not exceed the likelihood's by more than that leg's own range (max - min).
  step        ms per G+D iteration (critic_iters 1, two-stream schedule) with generator_output gumbel hard and the pathwise update, and
              with the score update at entropy weight 0 and 0.01, alternating five times in one process on one GanStep.  The second
              condition ("score_iteration_within_pathwise"): the score iteration launches strictly less of D (no head backward, no
              gemm_nt, no relax_rows_hard_bwd), so its median must not exceed the pathwise one's by more than that leg's range.

    python scripts/bench_score.py [--batch-size 64] [--size 224] [--vocab 1000] [--repeats 20] [--step-repeats 5] [--steps 10] [--out FILE]

Prints ONE JSON line and, with --out, writes it to FILE (profiles/score_bench.json is such a file).  Needs the GPU; reads nothing
outside the repository.  Whether the estimator trains better is not measured here or anywhere.
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


def kernel_leg(K, repeats, burst=50, eval_rows=24576, B=64):
    g = torch.Generator(device=K.device).manual_seed(7)
    out = {"burst": burst, "repeats": repeats, "copy_TBps": COPY_TBPS}
    for R, V in ((192, 1000), (192, 70000), (eval_rows, 1000)):
        x = 4.0 * torch.randn((R, V), generator=g, device=K.device)
        tok = torch.randint(0, V, (R,), generator=g, device=K.device, dtype=torch.int64)
        adv = torch.randn((R // 3,), generator=g, device=K.device)
        d = torch.empty_like(x)
        nll, hit = torch.empty(R, device=K.device), torch.empty(R, dtype=torch.int32, device=K.device)
        logp, ent = torch.empty(R, device=K.device), torch.empty(R, device=K.device)
        legs = {"softmax_xent_grad": lambda: K.softmax_xent(x, tok, scale=1.0 / 64, dlogits=d, nll=nll, hit=hit),
                "score_rows": lambda: K.score_rows(x, tok, adv, group=3, coef=1.0 / 64, dx=d, logp=logp, ent=ent),
                "score_rows_entropy": lambda: K.score_rows(x, tok, adv, group=3, coef=1.0 / 64, ent_coef=0.01 / 64, dx=d, logp=logp, ent=ent),
                "score_rows_no_dx": lambda: K.score_rows(x, tok, adv, group=3, logp=logp, ent=ent)}
        nbytes = {k: (4.0 if k.endswith("no_dx") else 8.0) * R * V for k in legs}
        us = timed_legs(legs, repeats, burst)
        rec = {}
        for k, xs in us.items():
            tbps = nbytes[k] / float(np.median(xs)) / 1e6
            rec[k] = dict(stats(xs), us="per launch", bytes=int(nbytes[k]), TBps=round(tbps, 3), share_of_copy_pct=round(100.0 * tbps / COPY_TBPS, 1))
        for k in ("score_rows", "score_rows_entropy"):
            rec[k]["time_over_softmax_xent_grad"] = round(rec[k]["median"] / rec["softmax_xent_grad"]["median"], 3)
        out["R%d_V%d" % (R, V)] = rec
    # the two one-workgroup launches of a step at batch B
    d_out = torch.randn((B, 3), generator=g, device=K.device)
    adv, out2 = torch.empty(B, device=K.device), torch.empty(2, device=K.device)
    logp, ent = torch.randn(3 * B, generator=g, device=K.device), torch.rand(3 * B, generator=g, device=K.device)
    us = timed_legs({"score_advantage_rloo": lambda: K.score_advantage(d_out, "rloo", adv=adv, out2=out2),
                     "score_advantage_none": lambda: K.score_advantage(d_out, "none", adv=adv, out2=out2),
                     "score_summary": lambda: K.score_summary(logp, ent, out2=out2)}, repeats, burst)
    out["B%d" % B] = {k: dict(stats(xs), us="per launch") for k, xs in us.items()}
    big = out["R192_V70000"]
    xe = big["softmax_xent_grad"]
    spread = xe["min_max"][1] - xe["min_max"][0]
    out["score_rows_within_softmax_xent"] = {"shape": "R192_V70000", "score_rows_median_us": big["score_rows"]["median"],
                                             "softmax_xent_grad_median_us": xe["median"], "softmax_xent_grad_range_us": round(spread, 3),
                                             "holds": bool(big["score_rows"]["median"] <= xe["median"] + spread)}
    return out


def step_leg(K, B, S, V, steps, repeats):
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), overlap_streams=True)
    gs.set_relaxation("gumbel", 1.0, 3, hard=True)
    g = torch.Generator().manual_seed(11)
    images = torch.randn((B, S, S, 3), generator=g).to(K.device)
    labels = torch.randint(0, V, (B, 3), generator=g, dtype=torch.int64).to(K.device)
    noises = [torch.randn((B, 512), generator=g).to(K.device) for _ in range(2)]
    alphas = [torch.rand((B,), generator=g).to(K.device)]
    count = [0]

    def iteration(mode):
        if mode is None:
            gs.set_estimator("pathwise")
        else:
            gs.set_estimator("score", "rloo", mode)
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

    modes = (("hard_pathwise", None), ("score", 0.0), ("score_entropy_0p01", 0.01))
    for _, m in modes:
        run(m)
    ms = {n: [] for n, _ in modes}
    for _ in range(repeats):
        for n, m in modes:
            ms[n].append(run(m))
    med = {n: float(np.median(x)) for n, x in ms.items()}
    path = ms["hard_pathwise"]
    spread = max(path) - min(path)
    return {"critic_iters": 1, "steps_per_repetition": steps, "alternations": repeats, "schedule": "two streams", "baseline": "rloo",
            "ms_per_iteration": {n: stats(x, 4) for n, x in ms.items()},
            "score_minus_pathwise_ms": round(med["score"] - med["hard_pathwise"], 4),
            "score_entropy_minus_pathwise_ms": round(med["score_entropy_0p01"] - med["hard_pathwise"], 4),
            "score_iteration_within_pathwise": {"score_median_ms": round(med["score"], 4), "pathwise_median_ms": round(med["hard_pathwise"], 4),
                                                "pathwise_range_ms": round(spread, 4), "holds": bool(med["score"] <= med["hard_pathwise"] + spread)}}


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

    rec = {"metric": "score_rows_us", "batch_size": B, "size": S, "vocab": V,
           "kernels": part(kernel_leg, K, args.repeats, 50, args.eval_rows, B),
           "step": None if args.kernels_only else part(step_leg, K, B, S, V, args.steps, args.step_repeats),
           "training_quality": "not measured", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
