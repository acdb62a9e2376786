"""bench_ground.py - grounded scene graphs: SceneGraphGAN.predict(ground=True) (csrc/ground.hip: the entity instances of an image
resolved on the device from the pooled attention of its samples) against SceneGraphGAN.predict(with_attention=True) - what a user
had to run before to see any attention at all - and against plain predict(), same seeded weights and images; the three kernels alone
(50 back-to-back launches per pair of HIP events) on a synthetic batch of the default evaluation shape; and
sgg_amd.ground.ground_reference, the numpy fp64 statement of the same definitions, per image of that batch on the host.

    python scripts/bench_ground.py [--batch-size 64] [--size 224] [--vocab 1000] [--images 64] [--repeats 10] [--out FILE]

One process, warm-up first; the legs alternate, `repeats` times each; medians and ranges are reported and every repetition is kept.
Prints ONE JSON line and, with --out, writes it to FILE (profiles/ground_bench.json is such a file).  The model is untrained: the
line says nothing about whether the attention localises entities.
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

LAUNCHES = 50       # per pair of events: the queue stays full, so the host's time to submit a call (asserts, ctypes) is not in the figure
KERNEL_REPEATS = 20


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def event_us(fn, repeats):
    """us per launch: LAUNCHES back-to-back launches between two HIP events, `repeats` times."""
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
    return out


def stats(us):
    return {"median": round(float(np.median(us)), 2), "min": round(float(np.min(us)), 2), "max": round(float(np.max(us)), 2)}


def kernels_alone(K, device, N, nb, V, side, words=10):
    """The three kernels on a synthetic batch: tokens from `words` words (so that triples repeat and words share mentions), random
    critic scores ranked by rank_triples, attention rows = softmax of a blob around one of three centres per word plus noise.
    Returns the timings and the host reference's time per image on the same batch."""
    from sgg_amd import ground
    g = np.random.RandomState(8)
    L = side * side
    vocab = np.sort(g.choice(V, size=words, replace=False))
    tokens = vocab[g.randint(0, words, size=(N, nb, 3))].astype(np.int64)
    yy, xx = np.mgrid[0:side, 0:side]
    cy, cx = g.randint(0, side, size=(V, 3)), g.randint(0, side, size=(V, 3))
    pick = g.randint(0, 3, size=(N, nb, 3))
    z = -0.125 * ((yy[None, None, None] - cy[tokens, pick][..., None, None]) ** 2 + (xx[None, None, None] - cx[tokens, pick][..., None, None]) ** 2)
    z = z + g.uniform(-0.5, 0.5, size=z.shape)
    e = np.exp(z - z.max(axis=(-1, -2), keepdims=True)).reshape(N * nb, 3, L)
    alphas = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    tok = torch.from_numpy(tokens).to(device)
    d = torch.from_numpy(g.standard_normal((N, nb, 3)).astype(np.float32)).to(device)
    al = [torch.from_numpy(np.ascontiguousarray(alphas[:, t])).to(device) for t in range(3)]
    ranked = K.rank_triples(tok, d, N, vocab=V)
    a = K.ground_assign(tok, ranked["triples"], ranked["n_distinct"], vocab=V)
    p = K.ground_pool(al, a["members"], a["start"], ranked["first_sample"], ranked["n_distinct"])
    r = K.ground_resolve(p["maps"], ranked["triples"], ranked["n_distinct"], p["n_pooled"], side, side)
    torch.cuda.synchronize()
    us = {"ground_assign": event_us(lambda: K.ground_assign(tok, ranked["triples"], ranked["n_distinct"], vocab=V, out=a), KERNEL_REPEATS),
          "ground_pool": event_us(lambda: K.ground_pool(al, a["members"], a["start"], ranked["first_sample"], ranked["n_distinct"], out=p),
                                  KERNEL_REPEATS),
          "ground_resolve": event_us(lambda: K.ground_resolve(p["maps"], ranked["triples"], ranked["n_distinct"], p["n_pooled"], side,
                                                              side, out=r), KERNEL_REPEATS)}
    host = {k: v.cpu().numpy() for k, v in ranked.items()}
    t0 = time.perf_counter()
    ref = ground.ground_reference(tokens, host["triples"], host["n_distinct"], host["first_sample"], alphas, side, side, vocab=V)
    host_s = time.perf_counter() - t0
    same = all(np.array_equal(ref[k], v.cpu().numpy()) for k, v in r.items() if v.dtype != torch.float32)
    rows_bytes = 3.0 * N * nb * L * 4
    pool_us = float(np.median(us["ground_pool"]))
    return {"samples_per_image": N, "images": nb, "slots": N, "cells": L, "vocab": V, "words": words,
            "us_per_launch_hip_events": {k: stats(v) for k, v in us.items()},
            "us_per_launch_all": {k: [round(x, 2) for x in v] for k, v in us.items()},
            "three_kernels_us_median_sum": round(float(sum(np.median(v) for v in us.values())), 2),
            "ground_pool_attention_bytes": rows_bytes, "ground_pool_GBps_of_attention_rows": round(rows_bytes / pool_us / 1e3, 1),
            "mean_n_distinct": round(float(host["n_distinct"].mean()), 2), "mean_n_nodes": round(float(ref["n_nodes"].mean()), 2),
            "host_reference_ms_per_image": round(1e3 * host_s / nb, 3), "host_reference_ms_per_batch": round(1e3 * host_s, 2),
            "device_discrete_outputs_equal_reference": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--workdir", default="/tmp/sgg_bench_ground")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import train as T
    from sgg_amd.api import kernels_for
    B, S, V = args.batch_size, args.size, args.vocab
    gan = T.SceneGraphGAN(os.path.join(args.workdir, "ck"), os.path.join(args.workdir, "logs"), None, None, None, None, None,
                          critic_iters=1, batch_size=B, lambda_=10, resume=False, synthetic=(B, S, V))
    K = kernels_for(gan.device)
    g = torch.Generator().manual_seed(4242)
    items = [torch.randn((S, S, 3), generator=g) for _ in range(args.images)]
    TB, N = gan.TEST_BATCH_SIZE, gan.TEST_BATCH_MULTIPLIER * gan.TEST_BATCH_SIZE
    legs = {"ground": lambda: gan.predict(items=items, ground=True),
            "with_attention": lambda: gan.predict(items=items, with_attention=True),
            "plain": lambda: gan.predict(items=items)}
    times = {k: [] for k in legs}
    for fn in legs.values():            # warm-up: the networks and their buffers at the test batch size, every leg once
        fn()
    for _ in range(args.repeats):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    preds = legs["ground"]()
    side = int(preds[0]["grounding"]["pooled_attention"].shape[-1])
    ips = {k: args.images / float(np.median(v)) for k, v in times.items()}
    ms = {k: 1e3 * float(np.median(v)) for k, v in times.items()}
    rec = {"metric": "ground_predict_images_per_s", "batch_size": B, "size": S, "vocab": V, "test_batch_size": TB, "samples_per_image": N,
           "images": args.images, "repeats": args.repeats, "feature_cells": side * side,
           "images_per_s": {k: round(v, 2) for k, v in ips.items()},
           "ms_per_call_median": {k: round(v, 3) for k, v in ms.items()},
           "ms_per_call_range": {k: [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in times.items()},
           "ms_per_call_all": {k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
           "ground_over_with_attention_time": round(ms["ground"] / ms["with_attention"], 4),
           "ground_over_plain_time": round(ms["ground"] / ms["plain"], 4),
           "ground_minus_plain_ms_per_image": round((ms["ground"] - ms["plain"]) / args.images, 4),
           "mean_n_distinct": round(float(np.mean([p["n_distinct"] for p in preds])), 2),
           "mean_n_nodes": round(float(np.mean([len(p["grounded_graph"]["nodes"]) for p in preds])), 2),
           "launches_per_event_pair": LAUNCHES, "kernel_repeats": KERNEL_REPEATS,
           "kernels_alone": kernels_alone(K, gan.device, N, TB, V, side),
           "thresholds": {"overlap": 0.5, "box_frac": 0.5, "tuned": False},
           "localisation_on_a_trained_model": "not measured",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
