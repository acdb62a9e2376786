"""-m gpu: gradient accumulation on the device - the accumulate kernel (csrc/optim.hip) against NumPy fp32, an update from N micro-batches
against the CPU oracle on all N * B rows, the plumbing bit for bit, the two-stream schedule, G-encoder reuse per micro-batch,
diagnostics, weight averaging and train.py --accumulate.

Tolerances.  The kernel: one correctly rounded fp32 addition per element has one answer - bit-equal to NumPy (NaNs by position).
Against the oracle: the tolerances of tests/test_step_gpu.py (tests/tolerances.py) - the accumulated update IS the update of the
N * B rows, only the summation order differs.  Everything that compares two schedules of the same kernels: bit-equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd.lib import SggError
from sgg_amd.step import GanStep
from tests.tolerances import GRAD_RTOL, loss_tol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PAD, SENTINEL = 64, -777.0
# the launcher of csrc/optim.hip (grid_for): blocks of BLOCK threads, VEC floats per thread and trip, at most GRID_CAP blocks
GRID_CAP, BLOCK, VEC = 4096, 256, 4
ONE_PASS = GRID_CAP * BLOCK * VEC                       # elements one trip of the capped grid covers
SIZES = [1, 2, 3, 4, 5, 7, 1027, ONE_PASS + 3, ONE_PASS + VEC * BLOCK + 2]      # (the last: a second trip of the loop AND a tail)
SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001,
                     0x7f7fffff, 0xff7fffff, 0x00800000], dtype=np.uint32)      # +-0, subnormals, +-Inf, NaNs, +-max, min normal


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def guarded(host):
    """A device copy of `host` between two sentinel guards: (whole buffer, the view the kernel gets)."""
    n = host.size
    big = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    big[PAD:PAD + n].copy_(torch.from_numpy(host.view(np.float32)))
    return big, big[PAD:PAD + n]


def untouched(big, n):
    return bool((big[:PAD] == SENTINEL).all() and (big[PAD + n:] == SENTINEL).all())


def kernel_inputs(n):
    """acc and g: seeded finite values with every pairing of the special values at both ends (so that the vector body and the scalar
    tail both meet them), among them Inf + -Inf and -0 + +0."""
    r = np.random.RandomState(11 + n % 9973)
    a = r.uniform(-4.0, 4.0, n).astype(np.float32).view(np.uint32).copy()
    g = (r.uniform(-4.0, 4.0, n) * 10.0 ** r.randint(-6, 3, n)).astype(np.float32).view(np.uint32).copy()
    m = len(SPECIALS)
    where = sorted(set(range(min(n, m * m))) | set(range(max(0, n - m * m), n)))
    for j, i in enumerate(where):
        a[i], g[i] = SPECIALS[j % m], SPECIALS[(j // m + j) % m]
    return a.view(np.float32), g.view(np.float32)


def same_floats(got, want):
    """Bit-equal, NaNs compared by position."""
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn]))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_one_fp32_addition_per_element(hip, n):
    a, g = kernel_inputs(n)
    if n >= 1027:
        assert np.isnan(a).any() and np.isinf(g).any() and (np.abs(a[a != 0]) < 1.2e-38).any(), "the special values are missing"
    with np.errstate(invalid="ignore", over="ignore"):
        want_sum = (a + g).astype(np.float32)           # (float32 + float32 in NumPy: one correctly rounded addition)
    assert want_sum.dtype == np.float32
    if n >= 1027:
        assert np.isnan(want_sum[~(np.isnan(a) | np.isnan(g))]).any(), "no Inf + -Inf among the inputs"
    for first, want in ((False, want_sum), (True, g)):
        (big_a, da), (big_g, dg) = guarded(a), guarded(g)
        hip.grad_accumulate(da, dg, first=first)
        torch.cuda.synchronize()
        assert untouched(big_a, n) and untouched(big_g, n), "written outside a buffer: n %d first %s" % (n, first)
        assert np.array_equal(bits(dg), g.view(np.int32)), "g changed: n %d first %s" % (n, first)
        got = da.cpu().numpy()
        assert same_floats(got, want), "n %d first %s: %d elements differ" % (
            n, first, int((got.view(np.int32) != want.view(np.int32)).sum()))
        if first and n > 8:
            assert not same_floats(a, g), "a non-zero acc equal to g: the overwrite would not show"


def test_kernel_rejects_bad_arguments_without_a_launch(hip):
    n = 64
    base = torch.arange(2 * n + 8, dtype=torch.float32, device="cuda")
    other = torch.full((n + 4,), 3.0, device="cuda")
    keep_base, keep_other = base.clone(), other.clone()
    with pytest.raises(SggError, match="aligned"):
        hip.grad_accumulate(base[1:1 + n], other[:n])              # acc offset by 4 bytes
    with pytest.raises(SggError, match="aligned"):
        hip.grad_accumulate(other[:n], base[1:1 + n])              # g offset by 4 bytes
    for shift in (0, 4, -4, n - 4):
        with pytest.raises(SggError, match="overlap"):
            hip.grad_accumulate(base[8:8 + n], base[8 + shift:8 + shift + n])
        with pytest.raises(SggError, match="overlap"):
            hip.grad_accumulate(base[8:8 + n], base[8 + shift:8 + shift + n], first=True)
    lib = hip.lib
    assert lib.sgg_grad_accumulate(base.data_ptr(), other.data_ptr(), 0, 0, None) == -1 and b"sgg_grad_accumulate" in lib.sgg_last_error()
    assert lib.sgg_grad_accumulate(base.data_ptr(), other.data_ptr(), -4, 1, None) == -1
    assert lib.sgg_grad_accumulate(None, other.data_ptr(), 4, 0, None) == -1 and lib.sgg_grad_accumulate(base.data_ptr(), None, 4, 0, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(base, keep_base) and torch.equal(other, keep_other), "a rejected call wrote to a buffer"
    hip.grad_accumulate(base[:n], base[n:2 * n])                   # adjacent ranges are not overlapping ones
    torch.cuda.synchronize()
    assert torch.equal(base[:n], keep_base[:n] + keep_base[n:2 * n]) and torch.equal(base[n:], keep_base[n:])


# ---- against the oracle on all rows -------------------------------------------------------------------------------------------------
BT, S, V = 8, 64, 50
_ORACLE = {}


def check_weights_after_adam(views, ref_params, ref_grads, old_params, t, what):
    """The rule of tests/test_step_gpu.py.  First-step Adam is sign-like: update = lr_t*g/(|g|*c + eps'), so an element whose gradient
    is at the fp32 rounding-noise level may legitimately move by +-lr_t in either implementation.  Assert (a) every element moved by
    at most the Adam bound, (b) elements with a significant gradient (>= 1% of the tensor's max) got the oracle's update within 1%
    of lr_t."""
    lr_t = O.tf_adam_lr_t(t)
    bound = 1.05 * lr_t * (1 - O.ADAM_B1) / (1 - O.ADAM_B2) ** 0.5
    for n, g in ref_grads.items():
        w_hip, w_ref, w_old = views[n].cpu(), ref_params[n], old_params[n]
        assert float((w_hip - w_old).abs().max()) <= bound, "%s %s: update exceeds the Adam bound" % (what, n)
        sig = g.abs() >= 1e-2 * g.abs().max()
        if sig.any():
            d = ((w_hip - w_old) - (w_ref - w_old))[sig].abs().max()
            assert float(d) <= 1e-2 * lr_t, "%s %s: update differs by %.3e (lr_t %.3e)" % (what, n, float(d), lr_t)


def tensor_err(a, b):
    return float((a.cpu() - b).abs().max() / (b.abs().max() + 1e-7))


def oracle():
    """O.d_step and O.g_step on all 8 rows, once for the module (left unchanged by the tests)."""
    if not _ORACLE:
        gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
        dp["W"] = dp["W"] * 25.0
        gp0, dp0 = {k: v.clone() for k, v in gp.items()}, {k: v.clone() for k, v in dp.items()}
        images, labels, onehot = O.synth_batch(BT, S, V)
        noise0, noise1, alpha = O.synth_noise(BT, 0), O.synth_noise(BT, 1), O.synth_alpha(BT, 0)
        cost, aux, dgrads = O.d_step(gp, dp, O.new_adam_state(dp), 1, images, onehot, noise0, alpha)
        assert float(aux["gp"]) > 1e-3, "the gradient penalty is inactive"
        dp1 = {k: v.clone() for k, v in dp.items()}
        gcost, _, ggrads = O.g_step(gp, dp, O.new_adam_state(gp), 1, images, noise1)
        _ORACLE.update(gp0=gp0, dp0=dp0, dp1=dp1, gp1=gp, cost=float(cost), gp=float(aux["gp"]), dgrads=dgrads, gcost=float(gcost),
                       ggrads=ggrads, images=images, labels=labels, noise0=noise0, noise1=noise1, alpha=alpha.reshape(BT))
    return _ORACLE


@pytest.mark.parametrize("N,B", [(2, 4), (4, 2)], ids=["2x4", "4x2"])
def test_accumulated_update_matches_the_oracle_on_all_rows(hip, N, B):
    R = oracle()
    cut = lambda t, k: t[k * B:(k + 1) * B].contiguous().cuda()
    gs = GanStep(hip, V, S, B, lam=10.0, g_state={k: v.clone() for k, v in R["gp0"].items()},
                 d_state={k: v.clone() for k, v in R["dp0"].items()})
    for k in range(N):
        gs.critic_step(cut(R["images"], k), cut(R["labels"], k), cut(R["noise0"], k), cut(R["alpha"], k), micro=(k, N))
    dl = gs.d_losses_mean.cpu()
    print("N %d x B %d: disc_cost %.7f (oracle %.7f), gp %.7f (oracle %.7f)" % (N, B, float(dl[0]), R["cost"], float(dl[2]), R["gp"]))
    assert abs(float(dl[0]) - R["cost"]) <= loss_tol(R["cost"]), (dl, R["cost"])
    assert abs(float(dl[2]) - R["gp"]) <= 1e-5 + 1e-4 * abs(R["gp"]), (dl, R["gp"])      # (the penalty's bound in tests/test_step_gpu.py)
    assert gs.D.adam_t == 1 and gs.G.adam_t == 0
    # grad_flat holds the SUM over the micro-batches; the decoder bias gradient cancels analytically (tests/test_step_gpu.py)
    dgrads = {n: g for n, g in R["dgrads"].items() if n != "decoder/bias"}
    assert float(gs.D.grads["decoder/bias"].abs().max()) / N < 1e-5
    worst = max((tensor_err(gs.D.grads[n] / N, g), n) for n, g in dgrads.items())
    print("critic gradients: worst rel err %.3e (%s)" % worst)
    assert worst[0] < GRAD_RTOL, "critic gradient %s: rel err %.3e" % (worst[1], worst[0])
    check_weights_after_adam(gs.D.arena.views, R["dp1"], dgrads, R["dp0"], 1, "critic")
    # the generator update on IDENTICAL critic weights, as tests/test_step_gpu.py does
    gs.D.arena.load_state_dict(R["dp1"])
    gs.D.trunk.refresh_weights()
    for k in range(N):
        gs.generator_step(cut(R["images"], k), cut(R["noise1"], k), micro=(k, N))
    gl = gs.g_losses_mean.cpu()
    print("gen_cost %.7f (oracle %.7f)" % (-float(gl[3]), R["gcost"]))
    assert abs(-float(gl[3]) - R["gcost"]) <= loss_tol(R["gcost"])
    worst = max((tensor_err(gs.G.grads[n] / N, g), n) for n, g in R["ggrads"].items())
    print("generator gradients: worst rel err %.3e (%s)" % worst)
    assert worst[0] < GRAD_RTOL, "generator gradient %s: rel err %.3e" % (worst[1], worst[0])
    check_weights_after_adam(gs.G.arena.views, R["gp1"], R["ggrads"], R["gp0"], 1, "generator")
    assert gs.G.adam_t == 1


# ---- schedules of the same kernels: bit for bit -------------------------------------------------------------------------------------
B4 = 4
ITERS, CRITIC_ITERS = 2, 2


def _states():
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    dp["W"] = dp["W"] * 25.0
    return gp, dp


def _weights(gs):
    gs.flush()
    torch.cuda.synchronize()
    out = {}
    for n, net in (("G", gs.G), ("D", gs.D)):
        out[n + ".weights"], out[n + ".m"], out[n + ".v"] = net.arena.flat.clone(), net.m_flat.clone(), net.v_flat.clone()
    out["losses"] = torch.cat([gs.d_losses_mean, gs.g_losses_mean]).clone()
    return out


def _differing(a, b):
    return [k for k in a if not np.array_equal(bits(a[k]), bits(b[k]))]


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "two_stream"])
def test_the_same_micro_batch_twice_is_the_plain_step_bit_for_bit(hip, overlap):
    """N = 2 fed the same micro-batch, noise and alpha twice: g + g and (2 g) * 0.5 are exact in fp32, so weights, Adam moments and
    loss means equal the plain step's bit for bit - the plumbing (zeroing, the two passes, the scale, the step count) adds nothing."""
    images, labels, _ = O.synth_batch(B4, S, V)
    img, lab = images.cuda(), labels.cuda()
    res = {}
    for N in (1, 2):
        gp, dp = _states()
        gs = GanStep(hip, V, S, B4, lam=10.0, g_state=gp, d_state=dp, overlap_streams=overlap)
        for it in range(ITERS):
            noises = [[O.synth_noise(B4, 10 * it + i).cuda()] * N for i in range(CRITIC_ITERS + 1)]
            alphas = [[O.synth_alpha(B4, 10 * it + i).reshape(B4).cuda()] * N for i in range(CRITIC_ITERS)]
            gs.train_iteration_accumulated([(img, lab)] * N, noises, alphas, critic_iters=CRITIC_ITERS)
        res[N] = _weights(gs)
        assert gs.D.adam_t == ITERS * CRITIC_ITERS and gs.G.adam_t == ITERS and ("acc" in gs.D.opt) == (N == 2)
    assert all(bool(torch.isfinite(t).all()) for t in res[1].values())
    bad = _differing(res[1], res[2])
    assert not bad, "accumulating the same micro-batch twice differs from the plain step: %s" % bad


_RUNS = {}


def run_accumulated(hip, overlap=False, reuse=True, ln_fusion=None, armed=False, decay=None):
    """ITERS iterations of CRITIC_ITERS critic updates + a generator update, every update from N = 2 distinct micro-batches of 4
    rows (the two halves of one 8-row draw); one run per setting for the module unless it is a repetition."""
    images, labels, _ = O.synth_batch(2 * B4, S, V)
    batches = [(images[k * B4:(k + 1) * B4].contiguous().cuda(), labels[k * B4:(k + 1) * B4].contiguous().cuda()) for k in range(2)]
    cut = lambda t, k: t[k * B4:(k + 1) * B4].contiguous().cuda()
    old = hip.ln_fusion
    if ln_fusion is not None:
        hip.ln_fusion = ln_fusion
    try:
        gp, dp = _states()
        gs = GanStep(hip, V, S, B4, lam=10.0, g_state=gp, d_state=dp, overlap_streams=overlap)
        if decay is not None:
            gs.G.enable_averaging(decay)
        if armed:
            gs.arm_diagnostics(True)
        calls, fwd = [], gs.G.trunk.forward
        gs.G.trunk.forward = lambda *a, **k: (calls.append(1), fwd(*a, **k))[1]
        for it in range(ITERS):
            noises = [[cut(O.synth_noise(2 * B4, 10 * it + i), k) for k in range(2)] for i in range(CRITIC_ITERS + 1)]
            alphas = [[cut(O.synth_alpha(2 * B4, 10 * it + i).reshape(2 * B4), k) for k in range(2)] for i in range(CRITIC_ITERS)]
            gs.train_iteration_accumulated(batches, noises, alphas, critic_iters=CRITIC_ITERS, reuse_g_encoder=reuse)
        snap = _weights(gs)
    finally:
        hip.ln_fusion = old
    return gs, snap, len(calls)


def reference_run(hip):
    if "ref" not in _RUNS:
        _RUNS["ref"] = run_accumulated(hip)
    return _RUNS["ref"]


def test_two_stream_schedule_is_bitwise_the_serial_one_under_accumulation(hip):
    gs, ref, calls = reference_run(hip)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())
    assert calls == ITERS * 2 * 2 and gs.D.adam_t == ITERS * CRITIC_ITERS and gs.G.adam_t == ITERS
    for rep in range(3):
        _, got, _ = run_accumulated(hip, overlap=True)
        bad = _differing(ref, got)
        assert not bad, "repetition %d: %s differ from the serial schedule" % (rep, bad)


@pytest.mark.parametrize("ln_fusion", [0, 2])
def test_reuse_equals_recompute_bit_for_bit(hip, ln_fusion):
    """The kept ctx is the output of the same forward-only schedule on the same weights: bit-equal in every ln_fusion mode (unlike the
    single-batch reuse, whose critic updates read the with-backward schedule)."""
    _, a, calls_a = run_accumulated(hip, reuse=True, ln_fusion=ln_fusion)
    _, b, calls_b = run_accumulated(hip, reuse=False, ln_fusion=ln_fusion)
    assert calls_a == ITERS * 2 * 2 and calls_b == ITERS * 2 * (CRITIC_ITERS + 1)
    bad = _differing(a, b)
    assert not bad, "ln_fusion %d: reuse differs from recompute in %s" % (ln_fusion, bad)


def test_diagnostics_read_the_mean_gradient_and_change_nothing(hip):
    _, ref, _ = reference_run(hip)
    gs, got, _ = run_accumulated(hip, armed=True)
    bad = _differing(ref, got)
    assert not bad, "the armed run differs from the unarmed one in %s" % bad
    diag = gs.diagnostics()
    for key, net in (("G", gs.G), ("D", gs.D)):
        live = net.arena.live(net.grad_flat).double()          # the SUM over the N = 2 micro-batches of the last update
        want = float(live.pow(2).sum().sqrt()) * 1.0 / 2
        print("%s: reported gradient norm %.9e, ||grad_flat|| * scale / N = %.9e" % (key, diag[key]["grad_norm"], want))
        assert want > 0 and abs(diag[key]["grad_norm"] - want) <= 1e-6 * want
        assert diag[key]["nonfinite"] == {"g": 0, "p": 0, "u": 0}
        assert net.opt["diag"]["last"][1] == 0.5, "the statistics pass did not get the gradient scale 1 / N"


def test_one_average_update_per_optimiser_step(hip):
    _, ref, _ = reference_run(hip)
    gs, got, _ = run_accumulated(hip, decay=0.9)
    assert gs.G.opt["ema"]["updates"] == ITERS == gs.G.adam_t and "ema" not in gs.D.opt
    bad = _differing(ref, got)
    assert not bad, "averaging changed the training state: %s" % bad
    n = gs.G.arena.live_numel
    assert not np.array_equal(bits(gs.G.opt["ema"]["flat"])[:n], bits(gs.G.arena.flat)[:n])


# ---- train.py -------------------------------------------------------------------------------------------------------------------
def _train(tmp_path, name, n_it, resume=False, logs=None):
    ck, logs = tmp_path / name, tmp_path / (logs or name + "_logs")
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--synthetic", "4,64,50", "--accumulate", "2", "--critic_iters", "2",
           "--max_iterations", str(n_it), "--diagnostics_every", "1", "--ema_decay", "0.9", "--checkpoints_dir", str(ck),
           "--summaries_dir", str(logs)] + (["--resume"] if resume else [])
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(str(ck / "model.ckpt.pt"), map_location="cpu"), [json.loads(l) for l in open(str(logs / "losses.jsonl"))]


def _finite(x):
    if isinstance(x, dict):
        return all(_finite(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(_finite(v) for v in x)
    return not isinstance(x, float) or np.isfinite(x)


def test_train_cli_accumulates_and_resumes_bit_for_bit(tmp_path):
    ck2, recs = _train(tmp_path, "a", 2)
    assert ck2["itr"] == 2 and ck2["D_adam"][2] == 4 and ck2["G_adam"][2] == 2 and ck2["accumulate"] == 2
    assert ck2["G_ema"]["updates"] == 2
    assert len(recs) == 2 and all("diag" in r for r in recs) and _finite(recs)
    for r in recs:
        assert r["diag"]["gp_slope_rows"] == 4 and r["diag"]["G"]["grad_norm"] > 0 and r["diag"]["D"]["grad_norm"] > 0
    ck3, _ = _train(tmp_path, "a", 3, resume=True, logs="a_logs_resumed")
    whole, _ = _train(tmp_path, "b", 3)
    assert ck3["itr"] == whole["itr"] == 3 and ck3["accumulate"] == whole["accumulate"] == 2
    for key in ("G", "D"):
        assert all(torch.equal(ck3[key][n].view(torch.int32), whole[key][n].view(torch.int32)) for n in whole[key]), key
        adam = key + "_adam"
        assert ck3[adam][2] == whole[adam][2] and all(torch.equal(ck3[adam][j], whole[adam][j]) for j in (0, 1)), adam
    assert torch.equal(ck3["G_ema"]["flat"], whole["G_ema"]["flat"]) and ck3["G_ema"]["updates"] == whole["G_ema"]["updates"] == 3
    assert not all(torch.equal(ck2["G"][n], whole["G"][n]) for n in whole["G"]), "the third iteration changed nothing"
