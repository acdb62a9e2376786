"""bench_predict.py - scene-graph prediction throughput: SceneGraphGAN.predict() (ranked distinct triples, ranking on the device:
csrc/rank.hip) against SceneGraphGAN.test() (the same sampling and scoring passes, tokens and scores copied to the host, per-image
Python ranking), same seeded weights, images and noise; and the ranking alone: HipKernels.rank_triples (HIP events) against the
host loop it replaces (SceneGraphGAN.recalls per image, on arrays already on the host; wall clock).

    python scripts/bench_predict.py [--batch-size 64] [--size 224] [--vocab 1000] [--images 64] [--repeats 10] [--out FILE]

One process, warm-up first; the legs of a comparison alternate, `repeats` times each; medians are reported and every repetition is
kept.  Prints ONE JSON line and, with --out, writes it to FILE (profiles/predict_bench_v1000.json is such a file).
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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def rank_alone(gan, K, nb, N, V, repeats):
    """rank_triples on [N, nb] samples between two HIP events (outputs preallocated) against recalls() per image on the host copies."""
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, V, (N, nb, 3), generator=g, dtype=torch.int64)
    tokens[N // 2:] = tokens[:N - N // 2]                  # every triple twice: duplicates as a sampler produces them
    d = torch.randn((N, nb, 3), generator=g)
    tok_d, d_d = tokens.to(gan.device), d.to(gan.device)
    out = K.rank_triples(tok_d, d_d, N, vocab=V)            # warm-up (and the output buffers of the timed calls)
    torch.cuda.synchronize()
    kern = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.rank_triples(tok_d, d_d, N, vocab=V, out=out)
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1))
    tok_h, score_h = tokens.numpy(), d.numpy().reshape(N, nb, 3, 1).mean(axis=2).reshape(N, nb)
    real = [[0, 0, 0]]
    host = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for j in range(nb):
            gan.recalls(tok_h[:, j].copy(), score_h[:, j].copy(), real)
        host.append(1e3 * (time.perf_counter() - t0))
    return {"images": nb, "samples_per_image": N, "rank_triples_ms_hip_events": round(float(np.median(kern)), 4),
            "host_recalls_loop_ms_wall": round(float(np.median(host)), 4), "kernel_faster": float(np.median(kern)) < float(np.median(host)),
            "rank_triples_ms_all": [round(x, 4) for x in kern], "host_ms_all": [round(x, 4) for x in host]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--workdir", default="/tmp/sgg_bench_predict")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import train as T
    from sgg_amd.api import kernels_for
    B, S, V = args.batch_size, args.size, args.vocab
    gan = T.SceneGraphGAN(os.path.join(args.workdir, "ck"), os.path.join(args.workdir, "logs"), None, None, None, None, None,
                          critic_iters=1, batch_size=B, lambda_=10, resume=False, synthetic=(B, S, V))
    K = kernels_for(gan.device)
    g = torch.Generator().manual_seed(4242)
    items = [(torch.randn((S, S, 3), generator=g), [[0, 0, 0]]) for _ in range(args.images)]
    TB, N = gan.TEST_BATCH_SIZE, gan.TEST_BATCH_MULTIPLIER * gan.TEST_BATCH_SIZE
    quiet = open(os.devnull, "w")
    legs = {"test": lambda: gan.test(items=items, out_path=None),
            "predict": lambda: gan.predict(items=items),
            "predict_with_attention": lambda: gan.predict(items=items, with_attention=True)}
    times = {k: [] for k in legs}
    stdout = sys.stdout
    sys.stdout = quiet                  # (test() prints its result line)
    try:
        for fn in legs.values():        # warm-up: both networks and their buffers at the test batch size, every leg once
            fn()
        for _ in range(args.repeats):
            for k, fn in legs.items():
                times[k].append(timed(fn))
        # agreement: the distinct triples of predict() are those of test()'s samples
        _, det = gan.test(items=items, out_path=None, return_details=True)
        pred = gan.predict(items=items)
    finally:
        sys.stdout = stdout
    same = all(set(map(tuple, p["triples"].tolist())) == set(map(tuple, d["tokens"].tolist())) and
               p["scores"][0] == d["scores"].min() for p, d in zip(pred, det))
    ips = {k: args.images / float(np.median(v)) for k, v in times.items()}
    rec = {"metric": "predict_images_per_s", "batch_size": B, "size": S, "vocab": V, "test_batch_size": TB, "samples_per_image": N,
           "images": args.images, "repeats": args.repeats,
           "images_per_s": {k: round(v, 2) for k, v in ips.items()},
           "ms_per_call_median": {k: round(1e3 * float(np.median(v)), 3) for k, v in times.items()},
           "ms_per_call_all": {k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
           "predict_over_test": round(ips["predict"] / ips["test"], 4),
           "predict_not_slower_than_test_by_more_than_5_percent": ips["predict"] >= 0.95 * ips["test"],
           "predict_triples_equal_test_samples": bool(same),
           "mean_distinct_triples": round(float(np.mean([p["n_distinct"] for p in pred])), 2),
           "ranking_alone": [rank_alone(gan, K, 32, 256, V, args.repeats), rank_alone(gan, K, 32, 4096, V, args.repeats)],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
