"""xent_trace_summary.py - per-dispatch durations of the likelihood kernels (csrc/xent.hip) from a rocprofv3 kernel trace of
scripts/bench_xent.py, split by the benchmark's legs.  At V = 1000 the benchmark's bursts measure the host's enqueue rate; the trace
has the kernels' own times.  A run of its own (tracing slows the host):

    rocprofv3 --kernel-trace -d DIR -o xent --output-format csv -- python scripts/bench_xent.py --kernels-only --repeats 4
    python scripts/xent_trace_summary.py DIR/xent_kernel_trace.csv [--repeats 4] [--out FILE]

The legs are recovered from the order of the dispatches: per shape 3 warm-up launches of each leg, then `repeats` x (50 with the
gradient, 50 forward only); triple_logp: one call, 3 warm-ups, `repeats` x 50.  Prints ONE JSON line (profiles/xent_kernel_trace.json
is such a line): microseconds, median and min .. max over the dispatches of a leg.
"""
import argparse
import csv
import json

import numpy as np

BURST, WARM = 50, 3


def leg(d):
    return {"n": len(d), "median_us": round(float(np.median(d)), 3), "min_max": [round(min(d), 3), round(max(d), 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with open(args.trace) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda key: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r["Kernel_Name"]]
    out = {"source": "rocprofv3 --kernel-trace of scripts/bench_xent.py --kernels-only --repeats %d" % args.repeats, "burst": BURST}
    for key, shape in (("xent_rows_resident_kernel", "R192_V1000"), ("xent_rows_stream_kernel", "R192_V70000")):
        d = us(key)[2 * WARM:2 * WARM + 2 * BURST * args.repeats]
        assert len(d) == 2 * BURST * args.repeats, (key, len(d))
        legs = {"with_gradient": [], "forward_only": []}
        for c in range(0, len(d), 2 * BURST):
            legs["with_gradient"] += d[c:c + BURST]
            legs["forward_only"] += d[c + BURST:c + 2 * BURST]
        out["%s_%s" % (key, shape)] = {k: leg(v) for k, v in legs.items()}
    d = us("triple_logp_kernel")[1 + WARM:]
    assert len(d) == BURST * args.repeats, len(d)
    out["triple_logp_kernel_N64_nb32_M64_V1000"] = leg(d)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
