"""bench_kbest.py - K-best decoding: SceneGraphGAN.predict(decode="kbest") at its defaults (TEST_BATCH_SIZE samples per image, the
sgg_amd.kbest.list_width most probable triples of each, merged by mixture log-probability; no critic pass: csrc/kbest.hip) against
SceneGraphGAN.predict() at its defaults (8 x TEST_BATCH_SIZE argmax samples per image ranked by critic score), same seeded weights
and images, and against predict(decode="kbest", top_k=256) - the same device work with host records of 256 triples per image in
place of every slot, which separates the record building from the rest; and the two kernels alone (50 back-to-back launches per
pair of HIP events) at V = 1000 and V = 70 000.

    python scripts/bench_kbest.py [--batch-size 64] [--size 224] [--vocab 1000] [--images 64] [--repeats 10] [--out FILE]

One process, warm-up first; the legs alternate, `repeats` times each; medians are reported and every repetition is kept.  Prints
ONE JSON line and, with --out, writes it to FILE (profiles/kbest_bench.json is such a file).  The model is untrained: the line says
nothing about recall.
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


LAUNCHES = 50       # per pair of events: the queue stays full, so the host's time to submit a call (asserts, ctypes) is not in the figure


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


def kernels_alone(K, device, N, nb, V, repeats):
    """kbest_triples on N x nb head rows and kbest_merge of their lists (outputs preallocated): us per launch over LAUNCHES
    back-to-back launches between two HIP events."""
    from sgg_amd import kbest
    width = kbest.list_width(N, V)
    g = torch.Generator().manual_seed(6)
    base = 3.0 * torch.randn((1, nb, 3, V), generator=g)
    logits = (base + 0.5 * torch.randn((N, nb, 3, V), generator=g)).to(device)
    per = K.kbest_triples(logits, width)                    # warm-up (and the output buffers of the timed calls)
    lists, lse = per["triples"].view(N, nb, width, 3), per["lse"]
    merged = K.kbest_merge(lists, logits, lse, N * width)
    torch.cuda.synchronize()
    t_us = event_us(lambda: K.kbest_triples(logits, width, out=per), repeats)
    m_us = event_us(lambda: K.kbest_merge(lists, logits, lse, N * width, out=merged), repeats)
    return {"vocab": V, "samples_per_image": N, "images": nb, "head_rows": N * nb, "list_width": width,
            "kbest_triples_us_hip_events": round(float(np.median(t_us)), 2), "kbest_merge_us_hip_events": round(float(np.median(m_us)), 2),
            "mean_n_distinct": round(float(merged["n_distinct"].float().mean()), 2),
            "kbest_triples_us_all": [round(x, 2) for x in t_us], "kbest_merge_us_all": [round(x, 2) for x in m_us]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--vocab", type=int, default=1000)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--workdir", default="/tmp/sgg_bench_kbest")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import train as T
    from sgg_amd import kbest
    from sgg_amd.api import kernels_for
    B, S, V = args.batch_size, args.size, args.vocab
    gan = T.SceneGraphGAN(os.path.join(args.workdir, "ck"), os.path.join(args.workdir, "logs"), None, None, None, None, None,
                          critic_iters=1, batch_size=B, lambda_=10, resume=False, synthetic=(B, S, V))
    K = kernels_for(gan.device)
    g = torch.Generator().manual_seed(4242)
    items = [torch.randn((S, S, 3), generator=g) for _ in range(args.images)]
    TB = gan.TEST_BATCH_SIZE
    # kbest_top256: the same device work as kbest, but the host builds records of 256 triples per image, not of every slot - what
    # separates the record building from the generator pass and the kernels
    legs = {"kbest": lambda: gan.predict(items=items, decode="kbest"),
            "kbest_top256": lambda: gan.predict(items=items, decode="kbest", top_k=256),
            "samples": lambda: gan.predict(items=items)}
    times = {k: [] for k in legs}
    for fn in legs.values():            # warm-up: the networks and their buffers at the test batch size, every leg once
        fn()
    for _ in range(args.repeats):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    preds = {k: fn() for k, fn in legs.items()}
    ips = {k: args.images / float(np.median(v)) for k, v in times.items()}
    rec = {"metric": "kbest_predict_images_per_s", "batch_size": B, "size": S, "vocab": V, "test_batch_size": TB, "images": args.images,
           "repeats": args.repeats,
           "samples_per_image": {"kbest": TB, "kbest_top256": TB, "samples": gan.TEST_BATCH_MULTIPLIER * TB}, "list_width": kbest.list_width(TB, V),
           "images_per_s": {k: round(v, 2) for k, v in ips.items()},
           "ms_per_call_median": {k: round(1e3 * float(np.median(v)), 3) for k, v in times.items()},
           "ms_per_call_all": {k: [round(1e3 * x, 3) for x in v] for k, v in times.items()},
           "kbest_over_samples": round(ips["kbest"] / ips["samples"], 4),
           "kbest_top256_over_samples": round(ips["kbest_top256"] / ips["samples"], 4),
           "launches_per_event_pair": LAUNCHES,
           "mean_n_distinct": {k: round(float(np.mean([p["n_distinct"] for p in v])), 2) for k, v in preds.items()},
           "kernels_alone": [kernels_alone(K, gan.device, TB, TB, 1000, args.repeats), kernels_alone(K, gan.device, TB, 2, 70000, args.repeats)],
           "recall_on_a_trained_model": "not measured",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
