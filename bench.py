"""bench.py - triples/sec of the WGAN-GP "G+D step" (one critic update + one generator update on one minibatch,
train.py:362-368 with CRITIC_ITERS = 1) on N MI355X GPUs of one node.

  python bench.py --gpus 1 --steps K --warmup W [--config {1,3,4}] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Default workload = BASELINE.json configs[1]: batch 64 per GPU, 224x224 synthetic images, vocab 1000, length-3 triples
(weak scaling: the global batch is 64*N, sharded by rows of one seeded global draw; the only exchange is the
gradient all-reduce over RCCL).  Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line:

  value / ms_per_step   the timed region: the product's default schedule (train.py: two HIP streams - D's encoder beside G's forward,
                        filter gradients beside the dgrad -> LayerNorm-backward chain - and a third for the recurrent heads' deferred
                        parameter-gradient work; bit-identical to the serial order), default conv
                        contraction mode (see DTYPE_NAME); config.schedule says so.  --single-stream times the serial order instead

A plain run does only this: set-up, W warm-up steps, the K timed steps, the outputs of the last timed step written to DIR
(--dump-outputs, see timed_path_outputs), the line.  Every record below is measured in --full runs only:

  serial                the same workload in the serial launch order, right after the timed region (kernels of two streams share the
                        chip, so only serial steps give per-kernel durations): its steps bracket the dominant convolution kernel's launches
  roofline              dominant convolution kernel against the MFMA peak (live HIP events around its launches in the `serial` steps;
                        which kernel that is comes from one serial step before them, where every convolution launch is bracketed)
  roofline_hbm          the memory-bound kernels (conv1_1, LSTM gates, attention, attention product, LayerNorm, Adam) against HBM peak,
                        from HIP events around every such call in two extra serial steps (the `serial` steps bracket only the dominant
                        kernel's launches: an event pair costs ~ 5 us); kernel_tflops_extra_steps holds the TFLOP/s of every other
                        matrix kernel from the same two steps
  native_f32            the same workload re-timed in the same run with native f32 MFMA arithmetic (mode 0)
  parity                same-run checks: default mode vs native f32 (logits, tokens); both vs the CPU oracle with the GPU side ON THE TIMED
                        SCHEDULE (losses, logits, tokens, every parameter-gradient tensor; tolerances ~10x the measured errors, and the
                        oracle's top-2 logit margin must exceed 4x the logit tolerance); two_stream_bitwise_at_full_size: two iterations of
                        two critic updates + one generator update at the timed size, serial launch order vs the timed multi-stream
                        schedule, parameter and Adam arenas bit-equal
  other_configs         (N = 1, default workload only) short legs of the other single-GPU configs of BASELINE.json - configs[3] (vocab
                        70 000) and configs[4] (batch 32, 448x448) -: value, ms_per_step, default mode vs native f32 on logits / tokens,
                        and one G+D step of the CPU oracle on --other-oracle-rows rows at the config's FULL shape vs the GPU
  critic_iters_10       secondary line: the loop body with the reference flag's nominal CRITIC_ITERS = 10 (train.py:408)
  cpu_baseline          the CPU oracle timed on this box's host cores (same run, N = 1 only)
  rccl                  (N > 1) what the collective layer saw and how much of the all-reduce is exposed
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

MFMA_F32_PEAK_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, chip table: Peak FP32 (matrix)
MFMA_BF16_PEAK_TFLOPS = 2500.0    # same table: Peak BF16 MFMA, dense (f16 MFMA runs at the bf16 rate)
HBM_PEAK_GBPS = 8000.0            # same table: HBM3E
SUSTAINED_F16_MFMA_TFLOPS = 1635.0   # measured, random operands (profiles/r01_ubench_mfma16_peak.log)
DTYPE_NAME = {0: "f32 (native f32 MFMA)",
              2: "f32 (conv operands scaled per tensor and split into 2 fp16 pieces, round-to-nearest = 23 significant bits, "
                 "3 fp16 MFMAs per product, f32 accumulate; native-f32 figure and parity in the same line)",
              6: "f32 (conv operands split into 3 bf16 pieces, 6 bf16 MFMAs per product, f32 accumulate)",
              3: "f32 storage, conv operands split into 2 bf16 pieces (3 bf16 MFMAs per product, f32 accumulate)",
              1: "f32 storage, conv operands scaled per tensor and ROUNDED TO ONE fp16 PIECE (11 significant bits, one fp16 MFMA per "
                 "product, f32 accumulate): mixed-precision mode, NOT the reference's arithmetic (SURVEY.md 8 row f4)",
              4: "f32 storage, conv operands rounded to ONE bf16 piece (8 significant bits, one bf16 MFMA per product, f32 accumulate): "
                 "mixed-precision mode, NOT the reference's arithmetic (SURVEY.md 8 row f4)"}
# BASELINE.json configs[i] that fit one GPU: rows per GPU, image side, vocabulary
CONFIGS = {1: (64, 224, 1000), 3: (64, 224, 70000), 4: (32, 448, 1000)}
# Same-run parity tolerances, ~10x what is measured (round 4: losses 1.9e-6 .. 3.8e-6 on |16.1|, logits 1.4e-6 .. 1.7e-6 on |1.2|, worst
# parameter-gradient tensor 1.4e-5 of its maximum) - the same numbers as tests/tolerances.py.  The arg-maxed tokens are guaranteed by
# the TOLERANCE, not only by the measured error: the record is ok only if the oracle's minimum top-2 logit margin exceeds 4x the
# logit tolerance (two logits may move towards each other by one tolerance each, with a factor 2 to spare).
LOSS_ATOL = LOSS_RTOL = 2e-6
LOGIT_ATOL = LOGIT_RTOL = 1e-5
GRAD_RTOL = 2e-4                  # per-tensor: max|d| <= GRAD_RTOL * max|ref| (train.py:265-266: what optimizer.minimize differentiates)
MARGIN_FACTOR = 4.0
CONFIG_NOTE = {1: "1xMI355X, batch 64, 224x224, vocab 1000", 3: "Visual-Genome-scale vocab 70k", 4: "large image, batch 32, 448x448"}


def workload_name(B, S, V, CI):
    tail = "batch %d per GPU, %dx%d synthetic images, vocab %d, 3-token triples, %d critic update%s + 1 generator update per step " \
           "(WGAN-GP lambda=10, TF-Adam)" % (B, S, S, V, CI, "" if CI == 1 else "s")
    for i, cfg in CONFIGS.items():
        if cfg == (B, S, V):
            return "BASELINE.json configs[%d] (%s): %s" % (i, CONFIG_NOTE[i], tail)
    return "custom (not a BASELINE.json config): " + tail


def conv_flops_per_step(B, S):
    """8*F_fwd - 2*f1: G-conv fwd x2, D-conv fwd x2, one backward (dgrad+wgrad, no image dgrad) each."""
    from sgg_amd.params import CONV_SPECS, same_pads
    h, f_fwd, f1 = S, 0.0, 0.0
    for (i, cin, cout, k, s, _, live) in CONV_SPECS:
        if not live:
            continue
        ho = same_pads(h, k, s)[0]
        f = 2.0 * B * ho * ho * cout * k * k * cin
        f_fwd += f
        if i == 0:
            f1 = f
        h = ho
    return 8 * f_fwd - 2 * f1


def synth_inputs(B_global, S, V, n_draws, rank, world, device):
    """images N(0,1) seed 0, labels randint seed 1, noise N(0,1) seed 2+k, alpha U[0,1) seed 1000+k,
    drawn for the GLOBAL batch on a CPU generator and sliced by rank."""
    B = B_global // world
    sl = slice(rank * B, (rank + 1) * B)
    g = torch.Generator().manual_seed(0)
    images = torch.randn((B_global, S, S, 3), generator=g)[sl].contiguous().to(device)
    g = torch.Generator().manual_seed(1)
    labels = torch.randint(0, V, (B_global, 3), generator=g, dtype=torch.int64)[sl].contiguous().to(device)
    noises, alphas = [], []
    for k in range(n_draws):
        g = torch.Generator().manual_seed(2 + k)
        noises.append(torch.randn((B_global, 512), generator=g)[sl].contiguous().to(device))
        g = torch.Generator().manual_seed(1000 + k)
        alphas.append(torch.rand((B_global,), generator=g)[sl].contiguous().to(device))
    return images, labels, noises, alphas


# --dump-outputs: an array is written whole up to this many elements and as a fixed seeded sample of this many above it (seven
# arrays, five of which can be this large: at most 40 MiB in all)
DUMP_MAX_ELEMS = 1 << 21


def dump_sample(t, seed=0):
    """t flattened to float32 on the host: whole up to DUMP_MAX_ELEMS elements, else the elements at DUMP_MAX_ELEMS sorted positions
    drawn with replacement by a CPU generator seeded with `seed` - the same positions for every array of the same length."""
    t = t.detach().reshape(-1)
    if t.numel() > DUMP_MAX_ELEMS:
        idx = torch.randint(t.numel(), (DUMP_MAX_ELEMS,), generator=torch.Generator().manual_seed(seed)).sort().values
        t = t[idx.to(t.device)]
    return t.float().cpu().numpy()


def timed_path_outputs(gs):
    """What a caller of the timed path holds after its last step, as {name: float32 array}: the losses of the last critic and the
    last generator update (step.py: d_losses, g_losses), the generator's logits [B,3,V] of the last generator update, and per network
    the parameters after its last Adam step and the gradients that step applied (every live tensor, in sorted TF-name order, so that
    the arrays do not depend on the arena layout)."""
    from sgg_amd.params import is_dead
    out = {"d_losses": gs.d_losses, "g_losses": gs.g_losses, "fake_logits": gs.G.head.state(1, gs.B).OUT[0]}
    for tag, net in (("G", gs.G), ("D", gs.D)):
        names = sorted(n for n in net.arena.views if not is_dead(n))
        out[tag + "_params"] = torch.cat([net.arena.views[n].reshape(-1) for n in names])
        out[tag + "_grads"] = torch.cat([net.grads[n].reshape(-1) for n in names])
    return {k: dump_sample(v) for k, v in out.items()}


def summarise_timing(timing):
    per = {}
    for sym, fl, nb, e0, e1 in timing:
        a = per.setdefault(sym, [0, 0.0, 0.0, 0.0])
        a[0] += 1
        a[1] += fl
        a[2] += nb
        a[3] += e0.elapsed_time(e1) * 1e-3
    return per


def conv_roofline(per, precision, dt):
    """Roofline record of the dominant convolution kernel (largest summed duration among the forward/dgrad kernels)."""
    conv = [s for s in per if s.startswith(("conv_gather", "conv_halo", "conv_s2"))]
    if not conv:
        return None
    dom = max(conv, key=lambda s: per[s][3])
    n, fl, _, sec = per[dom]
    traffic = None
    tpath = os.path.join(ROOT, "profiles", "roofline_traffic.json")
    if os.path.exists(tpath):
        traffic = json.load(open(tpath)).get(dom)
    nprod = {0: 1, 1: 1, 4: 1, 2: 3, 3: 3, 6: 6}[precision]
    peak = MFMA_BF16_PEAK_TFLOPS / nprod if precision else MFMA_F32_PEAK_TFLOPS
    note = ("dense %s MFMA peak %.0f TFLOP/s / %d MFMA products per algorithmic f32 product"
            % ("f16" if precision in (1, 2) else "bf16", MFMA_BF16_PEAK_TFLOPS, nprod) if precision else "f32 matrix peak")
    r = {"bound": "mfma", "kernel": dom, "achieved": fl / sec / 1e12, "peak": peak, "peak_note": note, "unit": "TFLOP/s",
         "frac": fl / sec / 1e12 / peak, "traffic": traffic, "mfma_tflops_issued": nprod * fl / sec / 1e12,
         "vs_native_f32_mfma_peak": fl / sec / 1e12 / MFMA_F32_PEAK_TFLOPS, "launches": n, "avg_launch_ms": 1e3 * sec / n,
         "flop_per_launch": fl / n, "share_of_step_time": sec / dt}
    targs = dom[dom.index("<") + 1:-1].split(",") if "<" in dom else []
    if (dom.startswith("conv_halo3_kernel") and len(targs) > 7 and targs[7] == "true") or \
            (dom.startswith("conv_halo3_pc_kernel") and len(targs) > 1 and targs[1] == "true") or \
            (dom.startswith("conv_s2_kernel") and len(targs) > 4 and targs[4] == "true"):
        r["kernel_note"] = ("this instantiation also applies the producing layer's LayerNorm + ELU while staging its patches (LN prologue: "
                            "that work replaces a separate HBM pass and is not counted in `achieved`); the plain instantiation is in kernel_tflops_extra_steps")
    if dom.startswith("conv_halo3_pc_kernel") and len(targs) > 2 and targs[2] == "true":
        r["kernel_note"] = ("producer / consumer 3x3 kernel on a pre-split source: weight fragments AND the activation patch are staged by "
                            "LDS-DMA (buffer_load ... lds), the MFMA waves issue LDS reads, v_mfma_f32_16x16x32_f16 and stores only")
    if precision in (1, 2, 3, 4):
        # a register-only loop of v_mfma_f32_32x32x16_f16 on random operands sustains 1.56-1.71 PFLOP/s: the chip clocks down
        # under matrix load (2.46 PFLOP/s only with all-zero operands) -> / 3 products
        r["sustained_mfma_peak_measured"] = SUSTAINED_F16_MFMA_TFLOPS / nprod
        r["frac_of_sustained"] = fl / sec / 1e12 / (SUSTAINED_F16_MFMA_TFLOPS / nprod)
    return r


def hbm_rooflines(per, steps):
    """The memory-bound calls against the HBM peak: algorithmic bytes (sgg_amd/lib.py) / event-measured time."""
    out = []
    for sym, (n, _, nb, sec) in sorted(per.items(), key=lambda kv: -kv[1][3]):
        if nb <= 0 or sec <= 0:
            continue
        gbps = nb / sec / 1e9
        out.append({"kernel": sym, "launches_per_step": round(n / steps, 2), "bytes": nb / n, "avg_us": 1e6 * sec / n,
                    "GBps": gbps, "frac_of_8TBps": gbps / HBM_PEAK_GBPS, "ms_per_step": 1e3 * sec / steps})
    return out


def loss_tol(ref):
    return LOSS_ATOL + LOSS_RTOL * abs(float(ref))


def logit_tol(max_abs_ref):
    return LOGIT_ATOL + LOGIT_RTOL * abs(float(max_abs_ref))


TOLERANCE_NOTE = ("losses |d| <= %g + %g*|ref|; logits |d| <= %g + %g*max|ref|; every parameter-gradient tensor max|d| <= %g * max|ref| "
                  "(train.py:265-266: what optimizer.minimize differentiates); tokens exact, and the oracle's top-2 logit margin must exceed "
                  "%g x the logit tolerance" % (LOSS_ATOL, LOSS_RTOL, LOGIT_ATOL, LOGIT_RTOL, GRAD_RTOL, MARGIN_FACTOR))


def parity_and_cpu_baseline(K, S, V, rows, threads, precisions, two_stream=True, head_side_stream=None):
    """One full G+D step of the CPU oracle (oracle/sgg_oracle.py, the restatement of the reference) on `rows` rows of the
    workload, timed on this box's host cores = cpu_baseline; the same step on the GPU (same weights, inputs, noise) in
    each of `precisions` = the same-run parity record.

    The GPU side runs the schedule that `value` is timed on (train.py:362-368's loop body as GanStep enqueues it by default):
    overlap_streams / head_side_stream as in the timed region, and - the critic and the generator update see ONE device tensor of
    images, as in the timed loop - G's encoder forward of the generator update early on its own stream (option g_early); the record
    says which of these were in force (`schedule`)."""
    from oracle import sgg_oracle as O
    from sgg_amd.step import GanStep
    torch.set_num_threads(threads)
    gp, dp = O.init_params("G", V, S), O.init_params("D", V, S)
    gp0, dp0 = {k: v.clone() for k, v in gp.items()}, {k: v.clone() for k, v in dp.items()}
    images, labels, onehot = O.synth_batch(rows, S, V)
    noise0, noise1, alpha = O.synth_noise(rows, 0), O.synth_noise(rows, 1), O.synth_alpha(rows, 0)
    d_adam, g_adam = O.new_adam_state(dp), O.new_adam_state(gp)
    t0 = time.time()
    cost, aux, dgrads = O.d_step(gp, dp, d_adam, 1, images, onehot, noise0, alpha)
    gcost, gaux, ggrads = O.g_step(gp, dp, g_adam, 1, images, noise1)
    dt = time.time() - t0
    cpu = {"value": rows / dt, "unit": "triples/sec", "cores": threads, "kind": "port",
           "sample": "1 full G+D step on %d rows of the workload (%dx%d, vocab %d), oracle/sgg_oracle.py fp32 (PyTorch CPU "
                     "restatement of the reference; the reference itself cannot run here), %d torch threads, %.1f s"
                     % (rows, S, S, V, threads, dt)}
    ref_toks = O.argmax_tokens(gaux["fake"])
    margin = O.top2_margin(gaux["fake"].detach())
    dev = K.device
    old = K.conv_precision
    par = {"rows": rows, "tolerance": TOLERANCE_NOTE, "top2_logit_margin": margin}

    def worst_grad(grads, ref, skip=()):
        # per tensor: max|d| / max|ref| (tests/test_configs34_gpu.py); the critic's decoder bias gradient is identically
        # mean - mean = 0 in exact arithmetic (the penalty does not see the bias) and has no scale to be relative to
        errs = [(float((grads[n].cpu() - g).abs().max() / (g.abs().max() + 1e-7)), n) for n, g in ref.items() if n not in skip]
        return max(errs)
    images_d, labels_d = images.to(dev), labels.to(dev)
    noise0_d, noise1_d, alpha_d = noise0.to(dev), noise1.to(dev), alpha.reshape(rows).to(dev)
    try:
        for prec in precisions:
            K.conv_precision = prec
            gs = GanStep(K, V, S, rows, lam=10.0, g_state=gp0, d_state=dp0, overlap_streams=two_stream, head_side_stream=head_side_stream)
            dl = gs.critic_step(images_d, labels_d, noise0_d, alpha_d).cpu()
            wd = worst_grad(gs.D.grads, dgrads, skip=("decoder/bias",))
            logit_err = float((gs.G.head.state(1, rows).OUT[0].cpu() - aux["fake"]).abs().max())
            # the generator step is compared on identical critic weights (the first Adam step is sign-like: gradient
            # elements at fp32 noise level move by +-lr in either implementation; DESIGN.md, Parity)
            gs.D.arena.load_state_dict(dp)
            gs.D.trunk.refresh_weights()
            gl = gs.generator_step(images_d, noise1_d).cpu()
            toks = gs.argmax_tokens(gs.G.head.state(1, rows).OUT[0]).cpu()
            wg = worst_grad(gs.G.grads, ggrads)
            max_logit = float(aux["fake"].abs().max())
            rec = {"disc_cost": float(dl[0]), "disc_cost_oracle": float(cost), "gp": float(dl[2]), "gp_oracle": float(aux["gp"]),
                   "gen_cost": -float(gl[3]), "gen_cost_oracle": float(gcost),
                   "loss_err_vs_oracle": max(abs(float(dl[0]) - float(cost)), abs(-float(gl[3]) - float(gcost))),
                   "max_logit_err_vs_oracle": logit_err, "max_abs_logit_oracle": max_logit, "logit_tolerance": logit_tol(max_logit),
                   "margin_over_logit_tolerance": margin / logit_tol(max_logit),
                   "tokens_equal_oracle": bool(torch.equal(toks, ref_toks)),
                   "worst_grad_rel_err_D": wd[0], "worst_grad_tensor_D": wd[1], "grad_tensors_D": len(dgrads) - 1,
                   "worst_grad_rel_err_G": wg[0], "worst_grad_tensor_G": wg[1], "grad_tensors_G": len(ggrads),
                   "schedule": {"overlap_streams": gs.side is not None, "head_side_stream": gs.head_side is not None,
                                "g_early_fired": getattr(gs, "xs", None) is not None}}
            rec["ok"] = bool(abs(float(dl[0]) - float(cost)) <= loss_tol(cost) and abs(-float(gl[3]) - float(gcost)) <= loss_tol(gcost)
                             and logit_err <= logit_tol(max_logit) and rec["tokens_equal_oracle"]
                             and margin > MARGIN_FACTOR * logit_tol(max_logit)
                             and wd[0] <= GRAD_RTOL and wg[0] <= GRAD_RTOL)
            par["precision%d_vs_oracle" % prec] = rec
            del gs
            torch.cuda.empty_cache()
    finally:
        K.conv_precision = old
    return cpu, par


def two_stream_bitwise_leg(K, B, S, V, iterations=2, critic_iters=2):
    """The schedule `value` is timed on against the serial launch order AT THE TIMED SIZE: from one initialisation, `iterations`
    iterations of train.py:362-368's loop body with `critic_iters` critic updates each, once on one HIP stream and once on the
    product's multi-stream schedule (overlap_streams, the heads' deferred stream, g_early); both parameter arenas, both Adam moment
    arenas and the last losses must be EQUAL bit for bit (tests/test_concurrency_gpu.py asserts the same)."""
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    dev = K.device
    g0, d0 = init_state_dict("G", V, S), init_state_dict("D", V, S)
    n_draw = iterations * (critic_iters + 1)
    images, labels, noises, alphas = synth_inputs(B, S, V, n_draw, 0, 1, dev)

    def run(two):
        gs = GanStep(K, V, S, B, lam=10.0, g_state=g0, d_state=d0, overlap_streams=two)
        gp_first = None
        for it in range(iterations):            # (GanStep.train_iteration's loop body, train.py:362-368)
            o = it * (critic_iters + 1)
            for i in range(critic_iters):
                gs.critic_step(images, labels, noises[o + i], alphas[o + i])
                if gp_first is None:
                    gp_first = gs.d_losses[2:3].clone()      # (the penalty, i.e. the second-order path, is active in the first update)
            gs.generator_step(images, noises[o + critic_iters])
        gs.flush()
        torch.cuda.synchronize(dev)
        snap = {"G.weights": gs.G.arena.flat.clone(), "D.weights": gs.D.arena.flat.clone(), "G.adam_m": gs.G.m_flat.clone(),
                "D.adam_m": gs.D.m_flat.clone(), "G.adam_v": gs.G.v_flat.clone(), "D.adam_v": gs.D.v_flat.clone(),
                "losses": torch.cat([gs.d_losses, gs.g_losses, gp_first]).clone()}
        fired = getattr(gs, "xs", None) is not None
        del gs
        torch.cuda.empty_cache()
        return snap, fired
    ref, _ = run(False)
    got, fired = run(True)
    bad = [k for k in ref if not torch.equal(ref[k], got[k])]
    finite = all(bool(torch.isfinite(v).all()) for v in got.values())
    return {"equal": not bad and finite, "differing": bad, "finite": finite, "iterations": iterations, "critic_iters": critic_iters,
            "g_early_fired": fired, "gp_first_update": float(got["losses"][8]), "gp_last_update": float(got["losses"][2]),
            "compared": "flat parameter arenas, Adam m and v arenas of G and D, last losses: torch.equal, serial vs multi-stream schedule, "
                        "batch %d, %dx%d, vocab %d" % (B, S, S, V)}


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a FRESH child (`python -m torch.distributed.run`, one
    process per GPU, the command line the driver itself uses) and relay rank 0's JSON line and the child's exit code.  This
    process never touches the GPU (no HIP call, no torch.cuda.is_available()) and never replaces itself (no os.exec*): the
    reference selects one device per process (train.py:417-418); the N-process layout is this build's."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    # --standalone: the launcher's own c10d rendezvous on a port the OS picks when it binds (no pre-picked port that another
    # bench started at the same moment could take); --local-addr: the container hostname may not resolve
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node", str(n),
           os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)      # stderr passes through
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    js = [l for l in lines if l.lstrip().startswith("{")]
    for l in lines:
        if not js or l is not js[-1]:
            print(l, file=sys.stderr)
    if js:
        print(js[-1])
        sys.stdout.flush()
    elif r.returncode == 0:
        print("bench.py: the %d-rank child printed no JSON line" % n, file=sys.stderr)
        return 1
    return exit_code_from(r.returncode, js[-1] if js else None)


def exit_code_from(child_rc, line):
    """torch.distributed.run collapses any rank failure to exit code 1, so the parity verdict travels in the JSON line: 3 when rank 0
    printed a line whose same-run parity record is not ok (the code a single-process run returns itself), else the child's own."""
    if line is not None:
        try:
            if json.loads(line).get("parity", {}).get("ok") is False:
                return 3
        except ValueError:
            pass
    return child_rc


def rendezvous_only(args):
    """The N > 1 launch path without a workload: process group from the launcher's environment (sgg_amd/dp.py), one all-reduce of a
    gradient-bucket-sized tensor through the same GradReducer the step uses, barrier, rank 0 prints the line."""
    import types
    import torch.distributed as dist
    import sgg_amd  # noqa: F401
    from sgg_amd import dp as dpmod
    rank, world, local = dpmod.init_from_env()
    assert world == args.gpus, "WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus)
    dev = torch.device("cuda:%d" % local) if dist.get_backend() == "nccl" else torch.device("cpu")
    reducer = dpmod.GradReducer(bucket_bytes=1 << 20)
    flat = torch.full((3 * reducer.bucket_elems + 5,), float(rank + 1), device=dev)
    net = types.SimpleNamespace(arena=types.SimpleNamespace(live=lambda t: t), grad_flat=flat)
    scale = reducer(net).wait()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    ok = bool(torch.all(flat * scale == (world + 1) / 2.0))
    dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "triples/sec (G+D step)", "value": None, "unit": "triples/sec", "n_gpus": world, "steps": 0, "warmup": 0,
                          "ms_per_step": None, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "data": "none (--rendezvous-only)",
                          "rccl": {"nranks": dist.get_world_size(), "backend": dist.get_backend(), "bucket_bytes": reducer.bucket_elems * 4,
                                   "allreduce_mean_ok": ok}}))
    dist.barrier()
    dist.destroy_process_group()
    return 0 if ok else 1


def other_config_leg(K, cfg, steps, warmup=1, oracle_rows=0, threads=16):
    """A short leg of another single-GPU config of BASELINE.json on the product's default schedule: `steps` timed G+D steps, then the
    generator's logits / tokens in the default arithmetic against native f32 MFMA on the same weights, then (oracle_rows > 0) one
    G+D step of the CPU oracle on a few rows at the config's full shape against the GPU.  The networks are built here and freed."""
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    B, S, V = CONFIGS[cfg]
    dev = K.device
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), overlap_streams=True)
    images, labels, noises, alphas = synth_inputs(B, S, V, 2 * (warmup + steps), 0, 1, dev)

    def one(k):
        gs.critic_step(images, labels, noises[2 * k], alphas[2 * k])
        gs.generator_step(images, noises[2 * k + 1])
    for k in range(warmup):
        one(k)
    gs.flush()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        one(k)
    gs.flush()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    rec = {"workload": workload_name(B, S, V, 1), "value": B * steps / dt, "unit": "triples/sec", "steps": steps, "warmup": warmup,
           "ms_per_step": 1e3 * dt / steps, "schedule": "two-stream", "conv_tflops_whole_step": conv_flops_per_step(B, S) * steps / dt / 1e12}
    main_prec = K.conv_precision
    if main_prec != 0:
        from oracle import sgg_oracle as O          # (top-2 margin helper only: the checker, never the thing measured)
        st, _ = gs.generator_forward(images, noises[0])
        logits_main = st.OUT[0].clone()
        toks_main = gs.argmax_tokens(logits_main).clone()
        try:
            K.conv_precision = 0
            gs.G.trunk.refresh_weights()
            st, _ = gs.generator_forward(images, noises[0])
            logits_f32 = st.OUT[0].clone()
            toks_f32 = gs.argmax_tokens(logits_f32).clone()
        finally:
            K.conv_precision = main_prec
        err, margin = float((logits_main - logits_f32).abs().max()), O.top2_margin(logits_f32.cpu())
        equal = bool(torch.equal(toks_main, toks_f32))
        # (post-training weights: the margin is not a property of the seeds; a flip only counts when the margin is resolvable)
        forgiven = bool(not equal and margin < 8.0 * err)
        rec["parity"] = {"mode%d_vs_native_f32" % main_prec: {"max_logit_err": err, "max_abs_logit": float(logits_f32.abs().max()),
                                                             "tokens_equal": equal, "top2_logit_margin": margin,
                                                             "token_flip_forgiven": forgiven},
                         "ok": bool(err <= logit_tol(logits_f32.abs().max()) and (equal or forgiven))}
    del gs
    torch.cuda.empty_cache()
    if oracle_rows > 0:
        # the CPU oracle on `oracle_rows` rows at the FULL shape of this config (image side, feature-map locations, vocabulary): one
        # G+D step, the GPU side on the timed schedule - losses, logits, tokens, every parameter-gradient tensor
        _, par = parity_and_cpu_baseline(K, S, V, oracle_rows, threads, [K.conv_precision], two_stream=True)
        orec = par["precision%d_vs_oracle" % K.conv_precision]
        orec["rows"], orec["top2_logit_margin"] = oracle_rows, par["top2_logit_margin"]
        rec.setdefault("parity", {"ok": True})["vs_oracle_at_full_shape"] = orec
        rec["parity"]["ok"] = bool(rec["parity"]["ok"] and orec["ok"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", type=int, default=1, choices=sorted(CONFIGS), help="BASELINE.json configs[i] preset (default 1)")
    ap.add_argument("--batch", type=int, default=None, help="rows per GPU (overrides the preset)")
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--vocab", type=int, default=None)
    ap.add_argument("--critic-iters", type=int, default=1)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last timed step to DIR/<name>.npy (float32; timed_path_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure and check everything else the line can hold: serial leg, roofline, "
                         "roofline_hbm, native_f32, critic_iters_10, cpu_baseline, parity, other_configs, rccl.  --cpu-rows, --f32-steps, "
                         "--ci10-steps, --no-kernel-timing, --per-shape, --serial-steps, --other-configs, --other-oracle-rows and "
                         "--bitwise-iters shape these legs and act in --full runs only")
    ap.add_argument("--cpu-rows", type=int, default=None, help="rows of the cpu_baseline / oracle-parity step (0 = skip; default: the "
                                                               "whole per-GPU batch up to 224x224, 16 rows at 448x448)")
    ap.add_argument("--f32-steps", type=int, default=10, help="steps of the native-f32 leg (0 = skip)")
    ap.add_argument("--ci10-steps", type=int, default=2, help="iterations of the critic_iters = 10 secondary leg (0 = skip)")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--per-shape", action="store_true", help="add per-layer conv timings (from the serial steps) to the JSON line")
    ap.add_argument("--serial-steps", type=int, default=5,
                    help="steps of the serial-order leg that follows the timed region; `roofline` is measured in them (0 = skip: no roofline)")
    ap.add_argument("--single-stream", action="store_true",
                    help="time the serial launch order as the headline (default: the product's two-stream schedule; per-kernel event "
                         "durations always come from serial steps, where no two kernels share the chip)")
    ap.add_argument("--other-configs", type=int, default=5,
                    help="timed steps of the configs[3] / configs[4] legs appended to the default workload's line at N = 1 (0 = skip)")
    ap.add_argument("--other-oracle-rows", type=int, default=4,
                    help="rows of the CPU-oracle step at the full configs[3] / configs[4] shape inside their legs (0 = skip)")
    ap.add_argument("--bitwise-iters", type=int, default=2,
                    help="iterations (2 critic updates + 1 generator update each) of the serial-vs-multi-stream bit-identity leg at the "
                         "timed size, parity.two_stream_bitwise_at_full_size (0 = skip)")
    ap.add_argument("--conv-precision", type=int, default=None, choices=[0, 1, 2, 3, 4, 6],
                    help="conv contraction: 2 = scaled fp16 pieces, 3 products (default), 6 = bf16 pieces, 6 products, "
                         "0 = native f32 MFMA, 3 = bf16 pieces, 3 products (within the 1e-4 tolerance); 1 / 4 = ONE fp16 / bf16 piece, one product "
                         "(mixed precision: not the reference's arithmetic, not a headline)")
    ap.add_argument("--head-side-stream", type=int, default=None, choices=[0, 1],
                    help="A/B switch: the heads' parameter-gradient work deferred to a stream of its own (sgg_amd/head.py; bit-identical "
                         "results); default: on with the two-stream schedule, off with --single-stream")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="N > 1: the ranks only meet (process group, one bucket-sized all-reduce through sgg_amd.dp, barrier) and rank 0 "
                         "prints the `rccl` record with value null - the launch path without a workload (CPU rehearsal over gloo)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))

    if args.rendezvous_only:
        sys.exit(rendezvous_only(args))

    import sgg_amd  # noqa: F401
    from sgg_amd import dp as dpmod
    from sgg_amd.lib import HipKernels
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep

    rank, world, local = dpmod.init_from_env()
    assert world == args.gpus, "WORLD_SIZE (%d) != --gpus (%d)" % (world, args.gpus)
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (there is no CPU fallback for the product path)"
    torch.cuda.set_device(local)
    dev = torch.device("cuda:%d" % local)
    K = HipKernels(dev)
    if args.conv_precision is not None:
        K.conv_precision = args.conv_precision
    B0, S0, V0 = CONFIGS[args.config]
    B = args.batch if args.batch is not None else B0
    S = args.size if args.size is not None else S0
    V = args.vocab if args.vocab is not None else V0
    CI = args.critic_iters
    two_stream = not args.single_stream
    reducer = dpmod.GradReducer() if world > 1 else None
    gs = GanStep(K, V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S), reducer=reducer,
                 overlap_streams=two_stream, head_side_stream=None if args.head_side_stream is None else bool(args.head_side_stream))
    side_stream, head_stream = gs.side, gs.head_side
    kt = not args.no_kernel_timing
    full = args.full
    # (the draws are seeded per step index: the timed steps see the same inputs with and without --full)
    extra = ((args.serial_steps + 2) + (2 if kt else 0) + (args.f32_steps + 1 if K.conv_precision != 0 else 0) + (4 if world > 1 else 0)
             if full else 0)
    total_steps = args.warmup + args.steps
    images, labels, noises, alphas = synth_inputs(B * world, S, V, (total_steps + extra) * (CI + 1), rank, world, dev)

    def set_schedule(two):
        """Two-stream (the product's default, GanStep(overlap_streams=True)) or serial launch order; same kernels, same results."""
        gs.side = side_stream if two else None
        gs.G.trunk.enable_wgrad_overlap(gs.side)
        gs.D.trunk.enable_wgrad_overlap(gs.side)
        gs.head_side = head_stream if two else None      # (the heads' deferred parameter-gradient work: head.py)
        gs.G.head.enable_side_stream(gs.head_side)
        gs.D.head.enable_side_stream(gs.head_side)

    def one_step(k):
        base = k * (CI + 1)
        for i in range(CI):
            gs.critic_step(images, labels, noises[base + i], alphas[base + i])
        gs.generator_step(images, noises[base + CI])

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    def timed(k0, n, with_events, conv_only=True):
        """n steps bracketed by barrier + synchronize on both sides; max over ranks."""
        barrier()
        K.timing = [] if with_events else None
        K.timing_conv_only = conv_only
        t0 = time.perf_counter()
        for k in range(k0, k0 + n):
            one_step(k)
        gs.flush()
        barrier()
        dt = time.perf_counter() - t0
        timing, K.timing = K.timing, None
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t.item())
        return dt, timing

    # ---- the timed region: W warm-up steps, then exactly K steps of the product's default schedule, no event inside -------------
    for k in range(args.warmup):
        one_step(k)
    gs.flush()
    dt, _ = timed(args.warmup, args.steps, False)
    d_losses, g_losses = gs.d_losses.cpu().tolist(), gs.g_losses.cpu().tolist()
    next_k = total_steps
    if args.dump_outputs and rank == 0:       # (before any leg of --full changes the networks)
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in timed_path_outputs(gs).items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)

    # ---- the same workload in the serial launch order: per-kernel durations (kernels of two streams would share the chip).  One
    # step brackets every forward / dgrad convolution launch and names the dominant kernel (largest summed duration); the serial
    # steps then bracket only that kernel's launches (an event pair costs ~ 5 us); two more steps bracket every call.
    dt_ser, timing, timing_hbm, hbm_steps, dominant = None, None, None, 2, None
    if full and args.serial_steps > 0:
        set_schedule(False)
        if kt:
            torch.cuda.synchronize(dev)
            K.timing, K.timing_conv_only, K.timing_symbols = [], True, None
        one_step(next_k)
        gs.flush()
        if kt:
            torch.cuda.synchronize(dev)
            wt, K.timing = K.timing, None
            per_w = summarise_timing(wt)
            conv_w = [s_ for s_ in per_w if s_.startswith(("conv_gather", "conv_halo", "conv_s2"))]
            dominant = max(conv_w, key=lambda s_: per_w[s_][3]) if conv_w else None
            K.timing_symbols = {dominant} if (dominant and not args.per_shape) else None
        dt_ser, timing = timed(next_k + 1, args.serial_steps, kt, conv_only="mfma" if args.per_shape else True)
        K.timing_symbols = None
        next_k += args.serial_steps + 1
        if kt:
            _, timing_hbm = timed(next_k, hbm_steps, True, conv_only=False)
            next_k += hbm_steps
        set_schedule(two_stream)

    out = None
    if rank == 0:
        value = B * world * args.steps / dt
        sched = ("two-stream; per-kernel figures from serial steps" if two_stream else "serial (--single-stream)")
        out = {
            "metric": "triples/sec (G+D step)", "value": value, "unit": "triples/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE_NAME[K.conv_precision], "data": "synthetic",
            "config": {"workload": workload_name(B, S, V, CI), "global_batch": B * world, "critic_iters": CI,
                       "parallelism": "dp%d" % world, "conv_precision_mode": K.conv_precision, "schedule": sched},
            "losses": {"disc_cost": d_losses[0], "gp": d_losses[2], "gen_cost": -g_losses[3]},
        }
        flops_step = conv_flops_per_step(B, S) * (CI + 1) / 2.0 if CI == 1 else None
        if flops_step:
            out["conv_tflops_whole_step_per_gpu"] = flops_step * args.steps / dt / 1e12
        if dt_ser is not None:
            out["serial"] = {"value": B * world * args.serial_steps / dt_ser, "unit": "triples/sec", "steps": args.serial_steps,
                             "ms_per_step": 1e3 * dt_ser / args.serial_steps,
                             "schedule": "serial launch order (one HIP stream): same kernels, same results; `roofline` is measured here"}
        if timing:
            per = summarise_timing(timing)
            out["roofline"] = conv_roofline(per, K.conv_precision, dt_ser)
            out["roofline"]["measured_in"] = "the `serial` leg (%d steps, %.2f ms per step)" % (args.serial_steps, 1e3 * dt_ser / args.serial_steps)
            out["roofline"]["launches_per_step"] = out["roofline"]["launches"] / args.serial_steps
            out["roofline_hbm"] = hbm_rooflines(summarise_timing(timing_hbm), hbm_steps)
            out["kernel_time_s"] = {s_: round(v[3], 4) for s_, v in sorted(per.items(), key=lambda kv: -kv[1][3])}
            out["kernel_tflops"] = {s_: round(v[1] / v[3] / 1e12, 2) for s_, v in per.items() if v[3] > 0 and v[1] > 0}
            # every other matrix kernel (the other convolution instantiations, filter gradients, conv1_1, attention product) is
            # bracketed in the two extra steps only
            per_x = summarise_timing(timing_hbm)
            out["kernel_tflops_extra_steps"] = {s_: round(v[1] / v[3] / 1e12, 2) for s_, v in per_x.items()
                                                if v[3] > 0 and v[1] > 0 and s_ not in per}
            if dominant:
                conv_x = {s_: v[3] for s_, v in per_x.items() if s_.startswith(("conv_gather", "conv_halo", "conv_s2"))}
                out["roofline"]["dominant_selected_in"] = ("one serial step before the `serial` leg (every forward / dgrad convolution launch "
                                                           "bracketed); largest summed duration in the extra steps: %s" % max(conv_x, key=conv_x.get))
            if args.per_shape:     # per (kernel, FLOPs per launch) = per layer and direction
                shp = {}
                for sym, fl, nb, e0, e1 in timing:
                    if fl <= 0:
                        continue
                    a_ = shp.setdefault("%s @ %.1f GF" % (sym, fl / 1e9), [0, 0.0])
                    a_[0] += 1
                    a_[1] += e0.elapsed_time(e1) * 1e-3
                out["per_shape"] = {k_: {"launches": v[0], "ms_per_step": round(1e3 * v[1] / args.serial_steps, 3),
                                         "tflops": round(float(k_.split("@")[1].split()[0]) * 1e9 * v[0] / v[1] / 1e12, 1)}
                                    for k_, v in sorted(shp.items(), key=lambda kv: -kv[1][1])}

    # ---- N > 1: what RCCL saw, and how much of the gradient all-reduce is exposed (same ranks, reducer off) --------------
    if full and world > 1:
        import torch.distributed as dist
        gs.reducer = None
        one_step(next_k)
        dt_off, _ = timed(next_k + 1, 3, False)
        next_k += 4
        gs.reducer = reducer
        if rank == 0:
            ms_on, ms_off = 1e3 * dt / args.steps, 1e3 * dt_off / 3
            out["rccl"] = {"nranks": dist.get_world_size(), "backend": dist.get_backend(), "bucket_bytes": reducer.bucket_elems * 4,
                           "allreduce_bytes_per_step": 4 * (gs.G.arena.live_numel + CI * gs.D.arena.live_numel),
                           "ms_per_step_without_allreduce": ms_off, "allreduce_ms_exposed": ms_on - ms_off}

    # ---- the same workload in native f32 MFMA arithmetic, same run, same schedule (the reference arithmetic is IEEE fp32) ------
    if full and K.conv_precision != 0 and args.f32_steps > 0:
        main_prec = K.conv_precision
        st, _ = gs.generator_forward(images, noises[0])
        logits_main = st.OUT[0].clone()
        toks_main = gs.argmax_tokens(logits_main).clone()
        K.conv_precision = 0
        gs.G.trunk.refresh_weights()
        gs.D.trunk.refresh_weights()
        st, _ = gs.generator_forward(images, noises[0])
        logits_f32 = st.OUT[0].clone()
        toks_f32 = gs.argmax_tokens(logits_f32).clone()
        one_step(next_k)
        dt32, _ = timed(next_k + 1, args.f32_steps, False)
        next_k += args.f32_steps + 1
        timing32 = None
        if kt:      # its own roofline from two serial steps with every forward / dgrad convolution launch bracketed
            set_schedule(False)
            _, timing32 = timed(next_k - 2, 2, True, conv_only=True)
            set_schedule(two_stream)
        K.conv_precision = main_prec
        gs.G.trunk.refresh_weights()
        gs.D.trunk.refresh_weights()
        if rank == 0:
            out["native_f32"] = {"value": B * world * args.f32_steps / dt32, "unit": "triples/sec", "steps": args.f32_steps,
                                 "ms_per_step": 1e3 * dt32 / args.f32_steps, "dtype": DTYPE_NAME[0], "schedule": out["config"]["schedule"]}
            if timing32:
                out["native_f32"]["roofline"] = conv_roofline(summarise_timing(timing32), 0, dt32)
            from oracle import sgg_oracle as O
            out["parity"] = {"mode%d_vs_native_f32" % main_prec: {
                "max_logit_err": float((logits_main - logits_f32).abs().max()), "max_abs_logit": float(logits_f32.abs().max()),
                "tokens_equal": bool(torch.equal(toks_main, toks_f32)), "top2_logit_margin": O.top2_margin(logits_f32.cpu()),
                "on": "generator logits [%d,3,%d] of the timed workload after the timed steps, same weights" % (B, V)}}

    # ---- secondary line: the reference flag's nominal CRITIC_ITERS = 10 (train.py:408): 10 critic updates + 1 generator update -----
    if full and CI == 1 and args.ci10_steps > 0:
        def iteration10(j):
            for i in range(10):
                gs.critic_step(images, labels, noises[(j + i) % len(noises)], alphas[(j + i) % len(alphas)])
            gs.generator_step(images, noises[(j + 10) % len(noises)])
        iteration10(0)
        gs.flush()
        barrier()
        t0 = time.perf_counter()
        for j in range(args.ci10_steps):
            iteration10(j + 1)
        gs.flush()
        barrier()
        dt10 = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt10], dtype=torch.float64, device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt10 = float(t.item())
        if rank == 0:
            out["critic_iters_10"] = {"value": B * world * args.ci10_steps / dt10, "unit": "triples/sec (one iteration = 10 critic updates + 1 "
                                      "generator update on one minibatch)", "iterations": args.ci10_steps,
                                      "ms_per_iteration": 1e3 * dt10 / args.ci10_steps}

    rc = 0
    if rank == 0:
        rows = args.cpu_rows if args.cpu_rows is not None else (B if S <= 224 else min(B, 16))
        default_workload = (B, S, V, CI) == CONFIGS[1] + (1,)
        del gs
        torch.cuda.empty_cache()
        if full and world == 1 and rows > 0:
            try:
                ncpu = len(os.sched_getaffinity(0))
            except AttributeError:
                ncpu = os.cpu_count() or 1
            precs = sorted({K.conv_precision, 0})
            # (the GPU side of the record runs the schedule `value` was timed on)
            cpu, par = parity_and_cpu_baseline(K, S, V, rows, min(ncpu, 16), precs, two_stream=two_stream,   # a 1-GPU box grants 16 host cores
                                               head_side_stream=None if args.head_side_stream is None else bool(args.head_side_stream))
            out["cpu_baseline"] = cpu
            out.setdefault("parity", {}).update(par)
        if full and world == 1 and two_stream and args.bitwise_iters > 0:
            bw = two_stream_bitwise_leg(K, B, S, V, iterations=args.bitwise_iters)
            out.setdefault("parity", {})["two_stream_bitwise_at_full_size"] = bw["equal"]
            out["parity"]["two_stream_bitwise_detail"] = bw
        # ---- the other single-GPU configs of BASELINE.json, observed in the same line (networks built and freed one after the other) --
        if full and world == 1 and default_workload and args.other_configs > 0:
            try:
                ncpu = len(os.sched_getaffinity(0))
            except AttributeError:
                ncpu = os.cpu_count() or 1
            out["other_configs"] = {"configs[%d]" % c: other_config_leg(K, c, args.other_configs, oracle_rows=args.other_oracle_rows,
                                                                        threads=min(ncpu, 16)) for c in (3, 4)}
        # same-run parity is ENFORCED: the line is printed either way, the exit code says whether the
        # arithmetic mode that was timed agrees with the oracle (and with native f32 on the timed workload's tokens)
        par = out.get("parity")
        if par is not None:
            checks = [par[k]["ok"] for k in par if k.endswith("_vs_oracle")]
            for k in [k for k in par if k.endswith("_vs_native_f32")]:
                # (the weights of this comparison are those after the timed steps, so its top-2 margin is not a fixed property of the
                # seeds: a token flip only counts when the margin is resolvable, i.e. above 8x the logit difference itself)
                r = par[k]
                r["token_flip_forgiven"] = bool(not r["tokens_equal"] and r["top2_logit_margin"] < 8.0 * r["max_logit_err"])
                r["ok"] = bool(r["tokens_equal"] or r["token_flip_forgiven"])
                checks.append(r["ok"])
            if "two_stream_bitwise_at_full_size" in par:
                checks.append(bool(par["two_stream_bitwise_at_full_size"]))
            checks += [leg["parity"]["ok"] for leg in out.get("other_configs", {}).values() if "parity" in leg]
            par["ok"] = bool(all(checks))
            head = par.get("precision%d_vs_oracle" % K.conv_precision)
            if (head is not None and not head["ok"]) or not all(par[k]["ok"] for k in par if k.endswith("_vs_native_f32")) or \
                    par.get("two_stream_bitwise_at_full_size") is False:
                rc = 3
        print(json.dumps(out))
        sys.stdout.flush()
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main())
