"""bench_retrieve.py - what image retrieval by triple query costs (csrc/retrieve.hip, train.SceneGraphGAN.retrieve):

  query_logp  HipKernels.query_logp at V = 1000 and V = 70 000 for Q = 64 and Q = 4096 shared full-triple queries, nb = 32 images and
              N = 256 samples (the evaluation's defaults), beside HipKernels.triple_logp covering the SAME (image, query) pairs -
              the queries replicated per image as its ground-truth list [nb, Q, 3] - in the same run: `burst` back-to-back launches
              between two device events, the four legs of a vocabulary alternating, `repeats` times; microseconds per launch
              (median, min .. max), the ratio of the medians and whether the two ranges overlap.  Their results are compared first.
  ranking     HipKernels.retrieve_topk (K = 10) and retrieve_ranks (10 relevant images per query) on a [4096, 5000] score matrix,
              the same way.
  retrieve    SceneGraphGAN.retrieve() beside likelihood() on the same synthetic items (an untrained model; --images of them, the
              default queries): images per second of each, alternating, host clock around calls that end in a copy to the host.

    python scripts/bench_retrieve.py [--repeats 20] [--burst 50] [--images 64] [--batch-size 64] [--size 224] [--out FILE]
                                     [--skip-v70000] [--kernels-only]

Prints ONE JSON line and, with --out, writes it to FILE (profiles/retrieve_bench.json is such a file).  Needs the GPU; reads nothing
outside the repository.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_xent import stats, timed_legs  # noqa: E402  (the house method: bursts between device events, alternating legs)


def overlap(a, b):
    return not (max(a) < min(b) or max(b) < min(a))


def query_leg(K, V, repeats, burst, N=256, nb=32, Qs=(64, 4096)):
    from sgg_amd import retrieve as R
    g = torch.Generator(device=K.device).manual_seed(7 + V)
    x = torch.empty((N, nb, 3, V), device=K.device)
    for k in range(N):                                # (sample by sample: no second copy of a 6.9 GB tensor at V = 70 000)
        x[k] = 4.0 * torch.randn((nb, 3, V), generator=g, device=K.device)
    lse = torch.empty((N, nb, 3), device=K.device)
    K.softmax_xent(x, None, lse=lse.view(-1))
    legs, check, out = {}, {}, {"N": N, "nb": nb, "V": V, "burst": burst, "repeats": repeats}
    rng = np.random.RandomState(V)
    for Q in Qs:
        ids = rng.randint(0, V, size=(Q, 3)).astype(np.int64)
        c = R.compile_queries(ids.tolist(), {i: i for i in range(V)})
        tok, qidx = torch.from_numpy(c["tok"]).to(K.device), torch.from_numpy(c["qidx"]).to(K.device)
        scores = torch.empty((Q, nb), device=K.device)
        gt = torch.from_numpy(np.tile(ids[None], (nb, 1, 1))).to(K.device)
        cnt = torch.full((nb,), Q, dtype=torch.int32, device=K.device)
        res = K.triple_logp(x, lse, gt, cnt)
        K.query_logp(x, lse, tok, c["ucount"], qidx, scores)
        check["Q%d" % Q] = float((scores.t() - res["mix"]).abs().max())
        out["Q%d_list_lengths" % Q] = c["ucount"]
        legs["query_logp_Q%d" % Q] = (lambda tok=tok, u=c["ucount"], qidx=qidx, scores=scores: K.query_logp(x, lse, tok, u, qidx, scores))
        legs["triple_logp_Q%d" % Q] = (lambda gt=gt, cnt=cnt, res=res: K.triple_logp(x, lse, gt, cnt, out=res))
    us = timed_legs(legs, repeats, burst)
    for Q in Qs:
        q, t = us["query_logp_Q%d" % Q], us["triple_logp_Q%d" % Q]
        out["Q%d" % Q] = {"query_logp": dict(stats(q), us="per launch"), "triple_logp_same_pairs": dict(stats(t), us="per launch"),
                          "triple_logp_over_query_logp": round(float(np.median(t)) / float(np.median(q)), 2),
                          "ranges_overlap": overlap(q, t), "max_abs_difference_of_results": check["Q%d" % Q],
                          "terms": N * nb * Q}
    return out


def ranking_leg(K, repeats, burst, Q=4096, n=5000, top=10, n_rel=10):
    g = torch.Generator(device=K.device).manual_seed(3)
    scores = -10.0 * torch.rand((Q, n), generator=g, device=K.device)
    rng = np.random.RandomState(3)
    rel = np.sort(np.stack([rng.choice(n, n_rel, replace=False) for _ in range(Q)]), axis=1).astype(np.int32).reshape(-1)
    ptr = torch.arange(0, Q * n_rel + 1, n_rel, dtype=torch.int32, device=K.device)
    idx = torch.from_numpy(rel).to(K.device)
    t = K.retrieve_topk(scores, n, top)
    r = K.retrieve_ranks(scores, n, ptr, idx)
    us = timed_legs({"retrieve_topk": lambda: K.retrieve_topk(scores, n, top, out=t),
                     "retrieve_ranks": lambda: K.retrieve_ranks(scores, n, ptr, idx, out=r)}, repeats, burst)
    return {"Q": Q, "n_images": n, "K": top, "relevant_per_query": n_rel, "burst": burst, "repeats": repeats,
            "retrieve_topk": dict(stats(us["retrieve_topk"]), us="per launch"),
            "retrieve_ranks": dict(stats(us["retrieve_ranks"]), us="per launch")}


def end_to_end_leg(B, S, V, n_images, repeats):
    import train as T
    tmp = tempfile.mkdtemp(prefix="bench_retrieve_")
    gan = T.SceneGraphGAN(os.path.join(tmp, "ck"), os.path.join(tmp, "logs"), None, None, None, None, None, critic_iters=1, batch_size=B,
                          lambda_=10, resume=False, synthetic=(B, S, V))
    items = [(x, real) for _, x, real in gan._evaluate_items(None, n_images)]

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return n_images / (time.perf_counter() - t0), res
    legs = {"retrieve": lambda: gan.retrieve(items=items), "likelihood": lambda: gan.likelihood(items=items)}
    last = {}
    for k, fn in legs.items():
        run(fn)
    rate = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            r, last[k] = run(fn)
            rate[k].append(r)
    return {"batch_size": B, "size": S, "vocab": V, "images": n_images, "n_samples": last["retrieve"]["n_samples"],
            "n_queries": last["retrieve"]["n_queries"], "alternations": repeats, "model": "untrained (synthetic items)",
            "images_per_s": {k: stats(v) for k, v in rate.items()},
            "retrieve_over_likelihood": round(float(np.median(rate["retrieve"])) / float(np.median(rate["likelihood"])), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--e2e-repeats", type=int, default=3)
    ap.add_argument("--skip-v70000", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import sgg_amd  # noqa: F401
    from sgg_amd.api import kernels_for
    K = kernels_for("cuda:0")

    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        return r

    rec = {"metric": "query_logp_us", "query_logp_V1000": part(query_leg, K, 1000, args.repeats, args.burst),
           "query_logp_V70000": None if args.skip_v70000 else part(query_leg, K, 70000, args.repeats, args.burst),
           "ranking": part(ranking_leg, K, args.repeats, args.burst),
           "retrieve": None if args.kernels_only else part(end_to_end_leg, args.batch_size, args.size, args.vocab, args.images,
                                                           args.e2e_repeats),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
