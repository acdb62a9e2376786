"""Is the kernel symbol the library reports for a convolution launch the one that ran?   python scripts/conv_route_trace_check.py [outdir]

One rocprofv3 --kernel-trace of the small step of tests/test_step_gpu.py::test_step_runs_the_kernels_the_routing_names (B 8, S 64,
V 50, ln_fusion 2, one critic and one generator update) with the timing hook on: the set of conv_gather* / conv_halo* / conv_s2* /
conv_c3_fwd* kernel names in the trace (spaces stripped, argument list dropped) must equal the set of symbols the hook collected in
the same process (sgg_conv2d_nhwc_fwd_symbol / _dgrad_symbol).  The same for the filter gradients: the conv_wgrad* / conv_c3_wgrad*
names in the trace against the symbols sgg_conv2d_nhwc_wgrad_symbol reported for the step's conv_wgrad calls (the hook itself gets a
label per kernel family there; the fused conv1_1 entry point sgg_conv2d_nhwc_wgrad_c3_ln has one kernel, conv_c3_wgrad_kernel<true>).
Prints the sets; exit status 1 if they differ.  No counters are collected; the traced program runs as a child of rocprofv3 under a
time limit of its own.  (--step FILE: that child.)"""
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAMILIES = ("conv_gather", "conv_halo", "conv_s2", "conv_c3_fwd")
WGRAD_FAMILIES = ("conv_wgrad", "conv_c3_wgrad")


def step(out_path):
    import torch
    import sgg_amd  # noqa: F401
    from oracle import sgg_oracle as O
    from sgg_amd.lib import HipKernels
    from sgg_amd.step import GanStep
    B, S, V = 8, 64, 50
    hip = HipKernels("cuda:0")
    hip.ln_fusion = 2
    images, labels, _ = O.synth_batch(B, S, V)
    noise0, noise1, alpha = O.synth_noise(B, 0), O.synth_noise(B, 1), O.synth_alpha(B, 0)
    hip.timing, hip.timing_conv_only = [], False          # every call is bracketed: the conv1_1 forward as well
    wgrad, query = set(), hip._conv_symbol

    def recording_query(entry, *args, **kw):              # what conv_wgrad asks the library before it picks its label
        symbols = query(entry, *args, **kw)
        if entry == "sgg_conv2d_nhwc_wgrad_symbol":
            wgrad.update(symbols.split(";"))
        return symbols
    hip._conv_symbol = recording_query
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=O.init_params("G", V, S, perturb=0.05), d_state=O.init_params("D", V, S, perturb=0.05))
    gs.critic_step(images.cuda(), labels.cuda(), noise0.cuda(), alpha.reshape(B).cuda())
    gs.generator_step(images.cuda(), noise1.cuda())
    gs.flush()
    torch.cuda.synchronize()
    syms = sorted({t[0] for t in hip.timing if t[0].startswith(FAMILIES)})
    if any(t[0].startswith("conv_c3_wgrad_ln(") for t in hip.timing):
        wgrad.add("conv_c3_wgrad_kernel<true>")
    hip.timing = None
    with open(out_path, "w") as f:
        json.dump({"fwd_dgrad": syms, "wgrad": sorted(wgrad)}, f)


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    hook_path = os.path.join(outdir, "hook_symbols.json")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", os.path.join(outdir, "trace"), "-o", "t", "--",
           "timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--step", hook_path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-4000:])
        return r.returncode
    traces = glob.glob(os.path.join(outdir, "trace", "**", "*kernel_trace.csv"), recursive=True)
    assert len(traces) == 1, traces
    rows = list(csv.DictReader(open(traces[0])))
    reported = json.load(open(hook_path))
    print("# rocprofv3 --kernel-trace of one critic + one generator update (B 8, S 64, V 50, ln_fusion 2)")
    equal = True
    for what, families, hook in (("forward / dgrad convolution", FAMILIES, set(reported["fwd_dgrad"])),
                                 ("filter gradient", WGRAD_FAMILIES, set(reported["wgrad"]))):
        pat = re.compile(r"^(?:void)?((?:%s)\w*(?:<[^>]*>)?)" % "|".join(families))
        names = [m.group(1) for m in (pat.match(row["Kernel_Name"].replace(" ", "")) for row in rows) if m]
        traced = set(names)
        print("%s: %d launches, %d kernels in the trace:" % (what, len(names), len(traced)))
        for s in sorted(traced):
            print("  " + s)
        print("symbols the library reported (%d):" % len(hook))
        for s in sorted(hook):
            print("  " + s)
        if "conv_c3_wgrad_kernel<true>" in hook:
            print("  (conv_c3_wgrad_kernel<true> is not reported by the library: this script adds it for the conv_c3_wgrad_ln calls the hook saw)")
        print("only in the trace: %s" % sorted(traced - hook))
        print("only reported:     %s" % sorted(hook - traced))
        equal &= traced == hook and len(traced) > 0
    print("RESULT: %s" % ("the sets are equal" if equal else "THE SETS DIFFER"))
    return 0 if equal else 1


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        step(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "_prof", "conv_route_trace")))
