"""CPU: the parts of bench.py that do not need a GPU - the workload naming (BASELINE.json configs), the algorithmic FLOP
accounting of SURVEY.md 8d and the record builders - so that the driver-facing JSON contract cannot drift silently."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_workload_names_follow_the_arguments():
    assert bench.workload_name(64, 224, 1000, 1).startswith("BASELINE.json configs[1]")
    assert bench.workload_name(64, 224, 70000, 1).startswith("BASELINE.json configs[3]")
    assert bench.workload_name(32, 448, 1000, 1).startswith("BASELINE.json configs[4]")
    assert bench.workload_name(8, 64, 50, 1).startswith("custom")           # the rehearsal size is NOT configs[1]
    assert "10 critic updates" in bench.workload_name(64, 224, 1000, 10)
    cfgs = json.load(open(os.path.join(ROOT, "BASELINE.json")))["configs"]
    assert "batch 64" in cfgs[1] and "448" in cfgs[4] and "70k" in cfgs[3]


def test_conv_flops_per_step_matches_the_survey():
    # 8*F_fwd - 2*f1 = 12 489.5 GFLOP at configs[1], 127.4 at configs[0], 24 979 at configs[4]
    assert abs(bench.conv_flops_per_step(64, 224) / 1e9 - 12489.5) < 1.0
    assert abs(bench.conv_flops_per_step(8, 64) / 1e9 - 127.4) < 0.1
    assert abs(bench.conv_flops_per_step(32, 448) / 1e9 - 24979.0) < 2.0


class _Ev:
    def __init__(self, t):
        self.t = t

    def elapsed_time(self, other):
        return other.t - self.t


def test_roofline_records_from_event_timings():
    timing = [("conv_halo3_kernel<2,128,2,2,true,true,false,false>", 236.8e9, 0.0, _Ev(0.0), _Ev(0.6)),
              ("conv_halo3_kernel<2,128,2,2,true,true,false,false>", 236.8e9, 0.0, _Ev(1.0), _Ev(1.6)),
              ("conv_s2_kernel<false,true,7>", 328.8e9, 0.0, _Ev(2.0), _Ev(2.9)),
              ("adam_kernel", 0.0, 967e6, _Ev(3.0), _Ev(3.16))]
    per = bench.summarise_timing(timing)
    r = bench.conv_roofline(per, 2, dt=0.01)
    assert r["kernel"].startswith("conv_halo3_kernel") and r["bound"] == "mfma" and r["unit"] == "TFLOP/s"
    assert abs(r["achieved"] - 2 * 236.8e9 / 1.2e-3 / 1e12) < 1e-6 and abs(r["peak"] - 2500.0 / 3) < 1e-9
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["launches"] == 2
    f32 = bench.conv_roofline(per, 0, dt=0.01)
    assert f32["peak"] == 157.3
    hbm = bench.hbm_rooflines(per, steps=1)
    assert [h["kernel"] for h in hbm] == ["adam_kernel"]
    assert abs(hbm[0]["GBps"] - 967e6 / 0.16e-3 / 1e9) < 1e-6 and abs(hbm[0]["frac_of_8TBps"] - hbm[0]["GBps"] / 8000.0) < 1e-12


def test_exit_code_travels_in_the_json_line():
    """torch.distributed.run collapses a rank's exit code to 1: the parent derives the parity code 3 from rank 0's line."""
    assert bench.exit_code_from(0, json.dumps({"parity": {"ok": True}})) == 0
    assert bench.exit_code_from(1, json.dumps({"parity": {"ok": False}})) == 3
    assert bench.exit_code_from(0, json.dumps({"parity": {"ok": False}})) == 3
    assert bench.exit_code_from(1, None) == 1 and bench.exit_code_from(1, "not json") == 1 and bench.exit_code_from(0, json.dumps({"value": 1})) == 0


def test_dump_outputs_are_the_last_step_and_fit_the_budget():
    """--dump-outputs: float32 arrays of what the timed path holds after its last step (here one G+D step through the CPU reference
    kernels); an array above DUMP_MAX_ELEMS elements becomes the same seeded sample every time, and all of them fit 64 MB at any size."""
    import numpy as np
    import torch
    import sgg_amd  # noqa: F401
    from oracle.kernels_ref import RefKernels
    from sgg_amd.params import init_state_dict
    from sgg_amd.step import GanStep
    B, S, V = 2, 32, 11
    gs = GanStep(RefKernels(), V, S, B, lam=10.0, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S))
    images, labels, noises, alphas = bench.synth_inputs(B, S, V, 2, 0, 1, "cpu")
    gs.critic_step(images, labels, noises[0], alphas[0])
    gs.generator_step(images, noises[1])
    gs.flush()
    out = bench.timed_path_outputs(gs)
    assert sorted(out) == ["D_grads", "D_params", "G_grads", "G_params", "d_losses", "fake_logits", "g_losses"]
    assert all(a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all() for a in out.values())
    assert np.array_equal(out["d_losses"], gs.d_losses.numpy()) and np.array_equal(out["g_losses"], gs.g_losses.numpy())
    assert np.array_equal(out["fake_logits"], gs.G.head.state(1, B).OUT[0].reshape(-1).numpy())
    assert len(out["G_params"]) == len(out["D_grads"]) == bench.DUMP_MAX_ELEMS < gs.G.arena.live_param_count()
    assert float(np.abs(out["G_grads"]).max()) > 0 and float(np.abs(out["D_grads"]).max()) > 0
    again = bench.timed_path_outputs(gs)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    t = torch.arange(1000, dtype=torch.float32)
    assert np.array_equal(bench.dump_sample(t), t.numpy())
    # losses whole, the other five arrays at most DUMP_MAX_ELEMS float32 each
    assert 2 * 4 * 4 + 5 * bench.DUMP_MAX_ELEMS * 4 <= 64e6


def test_cli_contract_flags_exist():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--config", "--critic-iters", "--cpu-rows", "--f32-steps", "--serial-steps", "--single-stream",
                 "--other-configs", "--other-oracle-rows", "--bitwise-iters", "--full", "--dump-outputs"):
        assert flag in out.stdout


def test_gpus_n_starts_its_own_ranks_over_gloo():
    """`python bench.py --gpus 2` with no launcher on the command line and no WORLD_SIZE in the environment (the form the driver
    may use): bench.py starts `python -m torch.distributed.run` as a child, the two ranks meet over gloo (SGG_DP_BACKEND; "nccl" =
    RCCL on a GPU node), all-reduce a bucket through sgg_amd.dp.GradReducer, and the parent relays rank 0's ONE JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SGG_DP_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rendezvous-only"], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl"]["nranks"] == 2 and rec["rccl"]["backend"] == "gloo" and rec["rccl"]["allreduce_mean_ok"]


def test_self_launch_relays_the_exit_code_of_the_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SGG_DP_BACKEND"] = "gloo"
    # without --rendezvous-only the ranks need MI355X GPUs: on a CPU box they must fail loudly (no CPU fallback), and so must the parent
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "2",
                          "--size", "32", "--vocab", "11", "--cpu-rows", "0"], capture_output=True, text=True, timeout=600, env=env)
    import torch
    if not torch.cuda.is_available():
        assert out.returncode != 0 and not [l for l in out.stdout.splitlines() if l.startswith("{")]


import pytest  # noqa: E402


@pytest.mark.gpu
def test_bench_line_names_its_schedule_and_measures_the_roofline_in_serial_steps():
    """The headline is the product's default (two-stream) schedule and says so; `roofline` comes from the serial leg, whose dominant
    kernel's launches per step times their average duration must fit inside a serial step (a rehearsal-sized workload)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "4", "--size", "64",
                          "--vocab", "50", "--cpu-rows", "4", "--f32-steps", "1", "--ci10-steps", "0", "--serial-steps", "2", "--full"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["config"]["schedule"] == "two-stream; per-kernel figures from serial steps"
    assert rec["config"]["workload"].startswith("custom") and rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["serial"]["steps"] == 2 and rec["serial"]["ms_per_step"] > 0 and "other_configs" not in rec      # (not the default workload)
    r = rec["roofline"]
    assert r["bound"] == "mfma" and r["launches_per_step"] * r["avg_launch_ms"] <= rec["serial"]["ms_per_step"]
    assert any(h["kernel"].startswith("conv_c3") for h in rec["roofline_hbm"]), [h["kernel"] for h in rec["roofline_hbm"]]
    assert rec["parity"]["ok"] is True and rec["cpu_baseline"]["kind"] == "port" and rec["native_f32"]["steps"] == 1
    # the oracle record is about the schedule that was timed, and that schedule is bit-identical to the serial one at the timed size
    sch = rec["parity"]["precision2_vs_oracle"]["schedule"]
    assert sch["overlap_streams"] and sch["head_side_stream"] and sch["g_early_fired"], sch
    assert rec["parity"]["two_stream_bitwise_at_full_size"] is True and rec["parity"]["two_stream_bitwise_detail"]["g_early_fired"]
    assert rec["parity"]["precision2_vs_oracle"]["margin_over_logit_tolerance"] > 4.0
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--batch", "4", "--size", "64",
                          "--vocab", "50", "--cpu-rows", "0", "--f32-steps", "0", "--ci10-steps", "0", "--serial-steps", "0", "--single-stream"],
                         capture_output=True, text=True, timeout=900)
    assert one.returncode == 0, one.stderr[-3000:]
    rec1 = json.loads([l for l in one.stdout.splitlines() if l.startswith("{")][-1])
    assert rec1["config"]["schedule"].startswith("serial") and "roofline" not in rec1


@pytest.mark.gpu
def test_plain_run_times_only_and_dumps_its_last_step(tmp_path):
    """Without --full the line holds the timed region only, even with every leg's option at its default; --dump-outputs writes the
    outputs of the last timed step, and two runs with the same arguments (same seeded inputs) write the same arrays."""
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4", "--size", "64", "--vocab", "50"]
    recs = []
    for run in ("a", "b"):
        out = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        recs.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
    rec = recs[0]
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["higher_is_better"] is True
    assert rec["metric"] == "triples/sec (G+D step)" and rec["unit"] == "triples/sec" and rec["dtype"] == bench.DTYPE_NAME[2]
    assert not set(rec) & {"serial", "roofline", "roofline_hbm", "native_f32", "critic_iters_10", "cpu_baseline", "parity", "other_configs",
                           "rccl"}, sorted(rec)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(k + ".npy" for k in ("d_losses", "g_losses", "fake_logits", "G_params", "G_grads", "D_params", "D_grads"))
    total = 0
    for f in names:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64e6
    d, g = np.load(str(tmp_path / "a" / "d_losses.npy")), np.load(str(tmp_path / "a" / "g_losses.npy"))
    assert d[0] == np.float32(rec["losses"]["disc_cost"]) and -g[3] == np.float32(rec["losses"]["gen_cost"])
    assert np.load(str(tmp_path / "a" / "fake_logits.npy")).shape == (4 * 3 * 50,)
