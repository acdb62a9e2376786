"""bench_score_multi.py - what S sampled triples per image cost in the score-function update (csrc/score.hip's multi-sample entry
points, step.GanStep.set_estimator("score", samples=S)):

  kernels     at (R, V) = (192, 1000), (192, 70 000) and (24 576, 1000) - the shapes of scripts/bench_score.py - and S in {1, 2, 4, 8}:
              HipKernels.sample_rows_multi BESIDE S launches of relax_rows_hard(tok only, gumbel) in the same run, and
              score_rows_multi BESIDE score_rows, the legs alternating: the existing launches are the yardsticks, never the new code
              itself.  The harness of scripts/bench_xent.py: `burst` (50) back-to-back launches between two device events, 20
              alternating repetitions; microseconds per launch (the S separate launches count as one).  Two conditions follow from
              the work done and are evaluated here per shape and S:
                "sample_rows_multi_within_separate_launches"  the one launch reads the row once instead of S times and draws the same
                    noise, so its median must not exceed the S launches' by more than that leg's own range (max - min).  The draw is
                    VALU-bound: the gain may be small, it is reported as a ratio.
                "score_rows_multi_s1_within_score_rows"       at S = 1 the launch does score_rows' work: its median must not exceed
                    score_rows' by more than that leg's range.
  step        ms per G+D iteration at critic_iters 1 on the two-stream schedule with the score update at S = 1 (baseline rloo) and
              S = 4 and 8 (baseline image), alternating five times in one process on one GanStep.  The difference is the S * B-row
              forward of D's head plus the wider launches; it is reported, not bounded.

    python scripts/bench_score_multi.py [--batch-size 64] [--size 224] [--vocab 1000] [--repeats 20] [--step-repeats 5] [--steps 10] [--out FILE]

Prints ONE JSON line and, with --out, writes it to FILE (profiles/score_multi_bench.json is such a file).  Needs the GPU; reads nothing
outside the repository.  Whether S > 1 trains better is not measured here or anywhere.
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

from bench_xent import stats, timed_legs  # noqa: E402

SAMPLES = (1, 2, 4, 8)


def kernel_leg(K, repeats, burst=50, eval_rows=24576):
    g = torch.Generator(device=K.device).manual_seed(7)
    out = {"burst": burst, "repeats": repeats, "samples": list(SAMPLES)}
    ok_sample, ok_rows = [], []
    for R, V in ((192, 1000), (192, 70000), (eval_rows, 1000)):
        x = 4.0 * torch.randn((R, V), generator=g, device=K.device)
        d = torch.empty_like(x)
        rec = {}
        for S in SAMPLES:
            tok = torch.zeros((S, R), dtype=torch.int64, device=K.device)
            one = torch.zeros(R, dtype=torch.int64, device=K.device)
            adv = torch.randn((S * (R // 3),), generator=g, device=K.device)
            logp, ent, logp1 = torch.empty(S * R, device=K.device), torch.empty(R, device=K.device), torch.empty(R, device=K.device)
            K.sample_rows_multi(x, tok, seed=3, draw=5)

            def separate(S=S, one=one):
                for s in range(S):
                    K.relax_rows_hard(x, tok=one, gumbel=True, seed=3, draw=5 | (s << 56))

            legs = {"relax_rows_hard_x_S": separate,
                    "sample_rows_multi": lambda tok=tok: K.sample_rows_multi(x, tok, seed=3, draw=5),
                    "score_rows": lambda tok=tok, adv=adv, logp1=logp1, ent=ent: K.score_rows(x, tok[0], adv, group=3, coef=1.0 / 64, dx=d, logp=logp1, ent=ent),
                    "score_rows_multi": lambda tok=tok, adv=adv, logp=logp, ent=ent: K.score_rows_multi(x, tok, adv, group=3, coef=1.0 / (64 * S), dx=d,
                                                                                                         logp=logp, ent=ent)}
            us = timed_legs(legs, repeats, burst)
            r = {k: dict(stats(xs), us="per launch" if k != "relax_rows_hard_x_S" else "per %d launches" % S) for k, xs in us.items()}
            sep, mul = r["relax_rows_hard_x_S"], r["sample_rows_multi"]
            spread = sep["min_max"][1] - sep["min_max"][0]
            r["sample_rows_multi_within_separate_launches"] = {"separate_range_us": round(spread, 3), "time_over_separate": round(mul["median"] / sep["median"], 3),
                                                               "holds": bool(mul["median"] <= sep["median"] + spread)}
            ok_sample.append(r["sample_rows_multi_within_separate_launches"]["holds"])
            one_, many = r["score_rows"], r["score_rows_multi"]
            r["score_rows_multi"]["time_over_score_rows"] = round(many["median"] / one_["median"], 3)
            if S == 1:
                spread = one_["min_max"][1] - one_["min_max"][0]
                r["score_rows_multi_s1_within_score_rows"] = {"score_rows_range_us": round(spread, 3), "holds": bool(many["median"] <= one_["median"] + spread)}
                ok_rows.append(r["score_rows_multi_s1_within_score_rows"]["holds"])
            rec["S%d" % S] = r
        out["R%d_V%d" % (R, V)] = rec
    out["sample_rows_multi_within_separate_launches"] = {"holds": bool(all(ok_sample)), "legs": len(ok_sample)}
    out["score_rows_multi_s1_within_score_rows"] = {"holds": bool(all(ok_rows)), "legs": len(ok_rows)}
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

    def run(n):
        gs.set_estimator("score", "rloo" if n == 1 else "image", 0.0, samples=n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            count[0] += 1
            gs.train_iteration(images, labels, noises, alphas, critic_iters=1, draws=[2 * count[0], 2 * count[0] + 1])
        gs.flush()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    modes = (1, 4, 8)
    for n in modes:
        run(n)
    ms = {n: [] for n in modes}
    for _ in range(repeats):
        for n in modes:
            ms[n].append(run(n))
    med = {n: float(np.median(x)) for n, x in ms.items()}
    return {"critic_iters": 1, "steps_per_repetition": steps, "alternations": repeats, "schedule": "two streams",
            "ms_per_iteration": {"S%d" % n: stats(x, 4) for n, x in ms.items()},
            "S4_minus_S1_ms": round(med[4] - med[1], 4), "S8_minus_S1_ms": round(med[8] - med[1], 4),
            "note": "the difference is the S * B-row forward of D's head and the wider launches: reported, not bounded"}


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

    rec = {"metric": "score_multi_us", "batch_size": B, "size": S, "vocab": V,
           "kernels": part(kernel_leg, K, args.repeats, 50, args.eval_rows),
           "step": None if args.kernels_only else part(step_leg, K, B, S, V, args.steps, args.step_repeats),
           "training_quality": "not measured", "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
