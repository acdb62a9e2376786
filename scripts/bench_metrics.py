"""bench_metrics.py - scene-graph metrics throughput: SceneGraphGAN.evaluate() (ground truth matched on the device: csrc/match.hip,
a few ints per ground-truth triple reach the host) against SceneGraphGAN.predict() followed by the host match
(sgg_amd.metrics.match_reference + RecallAccumulator per image), same seeded weights, images, noise and ground truth, at the default
N = 8 x TEST_BATCH_SIZE samples per image and at N = 4096; and the match alone: HipKernels.match_triples (HIP events round a burst of
launches) against the host loop over one batch (match_reference per image on arrays already on the host; wall clock).

    python scripts/bench_metrics.py [--batch-size 64] [--size 224] [--vocab 1000] [--images 64] [--repeats 7] [--large-samples 4096] [--out FILE]

One process, warm-up first; the legs of a comparison alternate, `repeats` times each; medians are reported and every repetition is
kept.  Prints ONE JSON line and, with --out, writes it to FILE (profiles/metrics_bench.json is such a file).
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

KS = (20, 50, 100)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def host_metrics(gan, items, n_samples, train):
    """The host path: predict() cut at max(KS), then the reference match and the accumulator per image."""
    from sgg_amd.metrics import RecallAccumulator, match_reference, zero_shot_mask
    V = len(gan.vocab)
    preds = gan.predict(items=items, n_samples=n_samples, top_k=min(max(KS), n_samples))
    acc, pos_all = RecallAccumulator(KS, V), []
    for p, (_, real) in zip(preds, items):
        pos, _ = match_reference(p["triples"], real, vocab=V)
        acc.add(pos, real, zero_shot_mask(real, train))
        pos_all.append(pos.tolist())
    return acc.result(gan.reverse_vocab), pos_all


def end_to_end(gan, images, n_samples, repeats):
    from sgg_amd.metrics import match_reference  # noqa: F401  (imported before the timed region)
    V = len(gan.vocab)
    g = np.random.RandomState(11)
    first = gan.predict(items=images, n_samples=n_samples, top_k=min(max(KS), n_samples))       # (also the warm-up of this shape)
    items = []
    for im, p in zip(images, first):        # ground truth: 8 triples of the image's own list and 8 random ones
        L = p["triples"].tolist()
        items.append((im, L[::max(1, len(L) // 8)][:8] + g.randint(0, V, size=(8, 3)).tolist()))
    train = {tuple(p["triples"][0].tolist()) for p in first}
    legs = {"evaluate": lambda: gan.evaluate(items=items, ks=KS, n_samples=n_samples, train_triples=train),
            "predict_then_host_match": lambda: host_metrics(gan, items, n_samples, train)}
    times = {k: [] for k in legs}
    for fn in legs.values():
        fn()
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    got = gan.evaluate(items=items, ks=KS, n_samples=n_samples, train_triples=train, return_details=True)
    want, want_pos = host_metrics(gan, items, n_samples, train)
    close = lambda a, b: (a is None and b is None) or (a is not None and b is not None and abs(a - b) <= 1e-12)
    same = [d["pos"] for d in got["details"]] == want_pos and all(
        close(got[n % k], want[n % k]) for k in KS for n in ("R@%d", "mR@%d", "zsR@%d"))
    ips = {k: len(images) / float(np.median(v)) for k, v in times.items()}
    return {"samples_per_image": n_samples, "images": len(images), "ground_truth_triples_per_image": 16,
            "images_per_s": {k: round(v, 2) for k, v in ips.items()},
            "ms_per_image": {k: round(1e3 / v, 4) for k, v in ips.items()},
            "evaluate_over_host_path": round(ips["evaluate"] / ips["predict_then_host_match"], 4),
            "evaluate_faster": ips["evaluate"] > ips["predict_then_host_match"],
            "ms_per_call_all": {k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
            "results_equal": bool(same), "R@100": got["R@100"], "mean_n_distinct": got["mean_n_distinct"]}


def match_alone(K, nb, top_k, M, V, repeats, burst=20):
    """match_triples on one batch between two HIP events (a burst of launches, outputs preallocated) against match_reference per image
    on the host copies."""
    from sgg_amd.metrics import match_reference
    g = torch.Generator().manual_seed(5)
    N = top_k
    tokens = torch.randint(0, V, (N, nb, 3), generator=g, dtype=torch.int64)
    ranked = K.rank_triples(tokens.cuda(), torch.randn((N, nb, 3), generator=g).cuda(), top_k, vocab=V)
    lists = ranked["triples"].cpu()
    nd = ranked["n_distinct"].cpu().numpy()
    gt = torch.randint(0, V, (nb, M, 3), generator=g, dtype=torch.int64)
    gt[:, ::2] = lists[:, torch.randint(0, top_k, (len(range(0, M, 2)),), generator=g)]     # every other row is in the list
    count = torch.full((nb,), M, dtype=torch.int32)
    gt_d, count_d = gt.cuda(), count.cuda()
    out = K.match_triples(ranked["triples"], ranked["n_distinct"], gt_d, count_d, vocab=V)    # warm-up, and the timed calls' outputs
    torch.cuda.synchronize()
    kern = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            K.match_triples(ranked["triples"], ranked["n_distinct"], gt_d, count_d, vocab=V, out=out)
        e1.record()
        e1.synchronize()
        kern.append(e0.elapsed_time(e1) / burst)
    lists_h, gt_h = lists.numpy(), gt.numpy()
    host, pos_h = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        pos_h = [match_reference(lists_h[j, :min(int(nd[j]), top_k)], gt_h[j].tolist(), vocab=V)[0] for j in range(nb)]
        host.append(1e3 * (time.perf_counter() - t0))
    return {"images": nb, "list_slots": top_k, "ground_truth_rows": M,
            "match_triples_ms_hip_events": round(float(np.median(kern)), 5), "host_match_loop_ms_wall": round(float(np.median(host)), 4),
            "kernel_faster": float(np.median(kern)) < float(np.median(host)),
            "results_equal": bool(np.array_equal(out["pos"].cpu().numpy(), np.stack(pos_h))),
            "match_triples_ms_all": [round(x, 5) for x in kern], "host_ms_all": [round(x, 4) for x in host]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--large-samples", type=int, default=4096, help="samples per image of the second end-to-end shape (0: skip it)")
    ap.add_argument("--workdir", default="/tmp/sgg_bench_metrics")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import train as T
    from sgg_amd.api import kernels_for
    B, S, V = args.batch_size, args.size, args.vocab
    gan = T.SceneGraphGAN(os.path.join(args.workdir, "ck"), os.path.join(args.workdir, "logs"), None, None, None, None, None,
                          critic_iters=1, batch_size=B, lambda_=10, resume=False, synthetic=(B, S, V))
    K = kernels_for(gan.device)
    g = torch.Generator().manual_seed(4242)
    images = [torch.randn((S, S, 3), generator=g) for _ in range(args.images)]
    TB = gan.TEST_BATCH_SIZE
    def part(fn, *a):           # (every part is also reported on stderr as soon as it is measured)
        r = fn(*a)
        print(json.dumps(r), file=sys.stderr, flush=True)
        return r

    rec = {"metric": "evaluate_images_per_s", "batch_size": B, "size": S, "vocab": V, "test_batch_size": TB, "ks": list(KS),
           "repeats": args.repeats,
           "match_alone": [part(match_alone, K, TB, 100, 64, V, args.repeats), part(match_alone, K, TB, 4096, 4096, V, args.repeats)],
           "end_to_end": [part(end_to_end, gan, images, n, args.repeats) for n in (gan.TEST_BATCH_MULTIPLIER * TB, args.large_samples) if n],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
