"""bench_predcls.py - what predicate classification costs (csrc/predcls.hip, train.SceneGraphGAN.predcls):

  pair_logp   HipKernels.pair_predicate_logp at N = 256 draws for P = 64 and P = 380 pairs (20 entities), at V = 1000 with nb = 32
              images and at V = 70 000 with one image, beside HipKernels.triple_logp on the largest enumeration of the SAME
              (pair, v) triples it accepts - 4096 rows per image, the first ones in pair-major order - in the same run: `burst`
              back-to-back launches between two device events, the legs of a vocabulary alternating, `repeats` times; microseconds
              per launch (median, min .. max), nanoseconds per triple of each and their ratio.  The results are compared first (the
              bits must be equal).
  selection   HipKernels.predcls_pair_topk (Kc = 100) on the [32, 380, 1000] joint buffer and predcls_merge (K = 100; one
              predicate per pair, and 100), the same way.
  predcls     SceneGraphGAN.predcls() beside likelihood() on the same synthetic items (an untrained model; --images of them):
              images per second of each, alternating, host clock around calls that end in a copy to the host.

    python scripts/bench_predcls.py [--repeats 20] [--burst 50] [--images 64] [--batch-size 64] [--size 224] [--out FILE]
                                    [--skip-v70000] [--kernels-only]

Prints ONE JSON line and, with --out, writes it to FILE (profiles/predcls_bench.json is such a file).  Needs the GPU; reads nothing
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


def _logits(K, N, nb, V):
    g = torch.Generator(device=K.device).manual_seed(11 + V)
    x = torch.empty((N, nb, 3, V), device=K.device)
    for k in range(N):
        x[k] = 4.0 * torch.randn((nb, 3, V), generator=g, device=K.device)
    lse = torch.empty((N, nb, 3), device=K.device)
    K.softmax_xent(x, None, lse=lse.view(-1))
    return x, lse


def _pairs(V, nb, P, entities=20):
    """Per image the first P ordered pairs of `entities` random distinct tokens (380 at 20 entities)."""
    rng = np.random.RandomState(V + P)
    out = np.empty((nb, P, 2), dtype=np.int32)
    for j in range(nb):
        e = np.sort(rng.choice(V, entities, replace=False))
        out[j] = [(a, b) for a in e for b in e if a != b][:P]
    return out


def pair_leg(K, V, nb, repeats, burst, N=256, Ps=(64, 380), keep=None):
    x, lse = _logits(K, N, nb, V)
    legs, out, check = {}, {"N": N, "nb": nb, "V": V, "burst": burst, "repeats": repeats}, {}
    for P in Ps:
        pairs = _pairs(V, nb, P)
        pd = torch.from_numpy(pairs).to(K.device)
        cnt = torch.full((nb,), P, dtype=torch.int32, device=K.device)
        jt = torch.empty((nb, P, V), device=K.device)
        res = K.pair_predicate_logp(x, lse, pd, cnt, joint=jt)
        # the largest enumeration triple_logp takes: the first 4096 (pair, v) of every image, pair-major
        M = min(4096, P * V)
        flat = np.arange(M)
        gt = np.stack([np.stack([pairs[j, flat // V, 0], flat % V, pairs[j, flat // V, 1]], axis=1) for j in range(nb)]).astype(np.int64)
        gtd = torch.from_numpy(gt).to(K.device)
        gcnt = torch.full((nb,), M, dtype=torch.int32, device=K.device)
        tl = K.triple_logp(x, lse, gtd, gcnt)
        mine = jt.reshape(nb, P * V)[:, :M]
        check[P] = bool(torch.equal(mine.contiguous().view(torch.int32), tl["mix"].view(torch.int32)))
        legs["pair_predicate_logp_P%d" % P] = (lambda pd=pd, cnt=cnt, jt=jt, res=res: K.pair_predicate_logp(
            x, lse, pd, cnt, joint=jt, out={"marg": res["marg"], "status": res["status"]}))
        legs["triple_logp_P%d" % P] = (lambda gtd=gtd, gcnt=gcnt, tl=tl: K.triple_logp(x, lse, gtd, gcnt, out=tl))
        if keep is not None and P == max(Ps):
            keep.update(joint=jt, status=res["status"], marg=res["marg"], pairs=pd)
    us = timed_legs(legs, repeats, burst)
    for P in Ps:
        a, t = us["pair_predicate_logp_P%d" % P], us["triple_logp_P%d" % P]
        M = min(4096, P * V)
        ns_a, ns_t = float(np.median(a)) * 1e3 / (nb * P * V), float(np.median(t)) * 1e3 / (nb * M)
        out["P%d" % P] = {"pair_predicate_logp": dict(stats(a), us="per launch", triples=nb * P * V, ns_per_triple=round(ns_a, 4)),
                          "triple_logp_4096_rows_per_image": dict(stats(t), us="per launch", triples=nb * M, ns_per_triple=round(ns_t, 4)),
                          "triple_logp_over_pair_predicate_logp_per_triple": round(ns_t / ns_a, 1),
                          "bits_equal_on_the_enumerated_triples": check[P]}
    return out


def selection_leg(K, kept, repeats, burst, Kc=100, top=100, M=16):
    joint, status, marg, pairs = kept["joint"], kept["status"], kept["marg"], kept["pairs"]
    nb, P, V = (int(n) for n in joint.shape)
    g = torch.Generator().manual_seed(5)
    gp = torch.randint(0, P, (nb, M), generator=g, dtype=torch.int32).to(K.device)
    gv = torch.randint(0, V, (nb, M), generator=g, dtype=torch.int32).to(K.device)
    t = K.predcls_pair_topk(joint, status, Kc, gp, gv)
    one = K.predcls_merge(pairs, t["top_tok"], t["top_score"], marg, top, per_pair=1)
    many = K.predcls_merge(pairs, t["top_tok"], t["top_score"], marg, top, per_pair=Kc, conditional=True)
    us = timed_legs({"predcls_pair_topk": lambda: K.predcls_pair_topk(joint, status, Kc, gp, gv, out=t),
                     "predcls_merge_per_pair_1": lambda: K.predcls_merge(pairs, t["top_tok"], t["top_score"], marg, top, per_pair=1, out=one),
                     "predcls_merge_per_pair_Kc": lambda: K.predcls_merge(pairs, t["top_tok"], t["top_score"], marg, top, per_pair=Kc,
                                                                          conditional=True, out=many)}, repeats, burst)
    out = {"nb": nb, "P": P, "V": V, "Kc": Kc, "K": top, "true_triples_per_image": M, "burst": burst, "repeats": repeats}
    out.update({k: dict(stats(v), us="per launch") for k, v in us.items()})
    return out


def end_to_end_leg(B, S, V, n_images, repeats):
    import train as T
    tmp = tempfile.mkdtemp(prefix="bench_predcls_")
    gan = T.SceneGraphGAN(os.path.join(tmp, "ck"), os.path.join(tmp, "logs"), None, None, None, None, None, critic_iters=1, batch_size=B,
                          lambda_=10, resume=False, synthetic=(B, S, V))
    items = [(x, real) for _, x, real in gan._evaluate_items(None, n_images)]

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return n_images / (time.perf_counter() - t0), res
    legs = {"predcls": lambda: gan.predcls(items=items), "likelihood": lambda: gan.likelihood(items=items)}
    last = {}
    for k, fn in legs.items():
        run(fn)
    rate = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            r, last[k] = run(fn)
            rate[k].append(r)
    return {"batch_size": B, "size": S, "vocab": V, "images": n_images, "n_samples": last["predcls"]["samples_per_image"],
            "mean_pairs_per_image": last["predcls"]["mean_pairs_per_image"], "alternations": repeats,
            "model": "untrained (synthetic items)", "images_per_s": {k: stats(v) for k, v in rate.items()},
            "predcls_over_likelihood": round(float(np.median(rate["predcls"])) / float(np.median(rate["likelihood"])), 4)}


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

    def part(fn, *a, **kw):     # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a, **kw)
        print(json.dumps(r), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        return r

    kept = {}
    rec = {"metric": "pair_predicate_logp_us", "pair_logp_V1000": part(pair_leg, K, 1000, 32, args.repeats, args.burst, keep=kept),
           "selection": part(selection_leg, K, kept, args.repeats, args.burst)}
    kept.clear()
    rec.update({"pair_logp_V70000": None if args.skip_v70000 else part(pair_leg, K, 70000, 1, args.repeats, args.burst),
                "predcls": None if args.kernels_only else part(end_to_end_leg, args.batch_size, args.size, args.vocab, args.images,
                                                               args.e2e_repeats),
                "device": torch.cuda.get_device_name(0)})
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
