"""The oracle side of the multi-update trajectory tests (test infrastructure, importable without a GPU; no test functions):
tests/test_trajectory_cpu.py checks from the oracle alone that the conditions below hold, tests/test_trajectory_gpu.py holds the device
training step to them past its first update.

The schedule: two iterations of two critic updates and one generator update on ONE minibatch of B, S, V = 8, 64, 50 (train.py:362-368
with CRITIC_ITERS = 2), from O.init_params(perturb=0.05) with the critic's embedding scaled by 25 (slopes > 1: the gradient penalty and
its second-order path are active), lam = 10, noise / alpha seeds 100 + 3 * iteration + i: the inputs of
tests/test_split_bf16_gpu.py::test_training_trajectory_default_mode_tracks_native_f32.  Update names: D1 D2 G1 D3 D4 G2.

Measured on the CPU with the oracle alone (tests/test_trajectory_cpu.py recomputes every column and asserts the conditions).  The fp32
columns move with the thread count's summation order: each figure is the largest of runs with 16, 8 and 5 threads.

  update  fp64 loss   gp      loss, one network one update stale      ... only its derived copies stale  fp32 vs fp64, same state  fp32 vs fp64,
                              critic / generator                      critic's / generator's             loss / worst grad tensor  free-running: loss
  D1      207.4247    20.75   -      / -                              -      / -                         1.1e-4 / 1.5e-5           1.1e-4
  D2       17.0511     1.73   1.0e+2 / -                              6.6e+1 / -                         2.0e-5 / 1.3e-5           2.1e-4
  G1       -0.1151     -      2.1e-2 / -                              2.9e-3 / -                         1.2e-7 / 7.9e-6           1.3e-4
  D3       12.5004     1.18   1.6e+1 / 7.2                            1.3e+1 / 7.2                       8.7e-6 / 9.6e-6           1.5e-4
  D4        0.7496     0.052  3.5    / 1.2                            2.1    / 1.2                       4.6e-7 / 3.3e-5           3.5e-5
  G2       -0.5328     -      7.7e-2 / 2.2e-1                         1.8e-2 / 1.5e-1                    7.3e-8 / 7.1e-6           2.7e-4

  * a network that is one update stale moves the loss by at least 2.1e-2 (G1, critic stale): 9e3 x loss_tol there (2.2e-6);
  * "derived copies stale": a network's convolution kernels from conv1_2 on one update stale, everything else current - what the
    device computes when the copies Trunk.refresh_weights derives from the arena (HWOI transposes, pre-split planes and fragments; the
    convolutions read nothing else, conv1_1 and the head read the arena itself) are not re-derived after an Adam pass: at least
    2.9e-3 (G1), 1.3e3 x loss_tol;
  * from the same state a correct fp32 implementation stays inside tests/tolerances.py at every update: losses within loss_tol with a
    factor >= 1.8 to spare (D2: 2.0e-5 against 3.6e-5), gradient tensors at most 3.3e-5 of their maximum against GRAD_RTOL = 2e-4 - no
    update needs a bound of its own;
  * two correct implementations that are NOT resynchronised drift apart through Adam (a first step is sign-like): ORACLE_F32_FREE_RUN
    is that drift of the fp32 oracle per update, the scale of the free-running tolerance (GPU: 10 x, the project's convention for a
    measured tolerance; the CPU test holds the fp32 oracle itself to 5 x).
"""
from collections import OrderedDict

import torch

from oracle import sgg_oracle as O
from tests import optim_ref as R

# ---- the schedule, as data ---------------------------------------------------------------------------------------------------------
B, S, V, LAM = 8, 64, 50, 10.0
PERTURB, EMB_SCALE = 0.05, 25.0
ITERS, CRITIC_ITERS = 2, 2
# (name, network updated, iteration, update within the iteration)
SCHEDULE = (("D1", "D", 0, 0), ("D2", "D", 0, 1), ("G1", "G", 0, 2), ("D3", "D", 1, 0), ("D4", "D", 1, 1), ("G2", "G", 1, 2))
NAMES = tuple(u[0] for u in SCHEDULE)

# |loss of the free-running fp32 oracle - loss of the free-running fp64 oracle| per update: the larger of two runs with
# torch.set_num_threads(16) and (5) (the last column of the table above; tests/test_trajectory_cpu.py re-measures it)
ORACLE_F32_FREE_RUN = {"D1": 1.1e-4, "D2": 2.1e-4, "G1": 1.3e-4, "D3": 1.5e-4, "D4": 3.5e-5, "G2": 2.7e-4}


def seed(it, i):
    return 100 + 3 * it + i


def initial_states(V=V, S=S):
    """(G's, D's) fp32 state dicts in the oracle's names: what the device is loaded with and what the free-running oracle starts from
    (widened exactly where it runs in fp64)."""
    gp, dp = O.init_params("G", V, S, perturb=PERTURB), O.init_params("D", V, S, perturb=PERTURB)
    dp["W"] = dp["W"] * EMB_SCALE
    return gp, dp


def minibatch(B=B, S=S, V=V):
    """(images, labels, onehot) in fp32: the one minibatch every update of the schedule sees."""
    return O.synth_batch(B, S, V)


def update_inputs(kind, it, i, B=B):
    """(noise [B, 512], alpha [B, 1, 1] or None) of update i of iteration it, fp32."""
    return O.synth_noise(B, seed(it, i)), (O.synth_alpha(B, seed(it, i)) if kind == "D" else None)


def oracle_inputs(images, onehot, noise, alpha, dtype=torch.float64):
    return {"images": images.to(dtype), "onehot": onehot.to(dtype), "noise": noise.to(dtype),
            "alpha": None if alpha is None else alpha.to(dtype)}


def to_dtype(d, dtype):
    return OrderedDict((k, v.detach().to(dtype).clone()) for k, v in d.items())


# ---- the oracle follows the device ---------------------------------------------------------------------------------------------------
def oracle_from_device(net):
    """fp64 host copies of a sgg_amd.step.Network's training state, in the oracle's form: (parameters by name, (m, v) by name without
    the dead branch - as O.new_adam_state makes them -, t = net.adam_t).  Reads only; the caller has applied pending updates."""
    assert net.pending is None, "oracle_from_device: an optimiser step is still pending (GanStep.flush first)"
    a = net.arena
    host = lambda flat: a._make_views(flat.detach().cpu().double())
    params = OrderedDict((n, v.clone()) for n, v in host(a.flat).items())
    m = {n: v.clone() for n, v in host(net.m_flat).items() if not O.is_dead(n)}
    v = {n: x.clone() for n, x in host(net.v_flat).items() if not O.is_dead(n)}
    assert set(m) == set(O.new_adam_state(params)[0])
    return params, (m, v), int(net.adam_t)


def oracle_update(kind, gp, dp, adam, t, inputs):
    """One O.d_step / O.g_step (update number t of the network `kind`, whose Adam moments are `adam`) in the dtype of its operands.
    Returns (cost, aux, gradients by name); the updated parameters and moments are left in place."""
    if kind == "D":
        return O.d_step(gp, dp, adam, t, inputs["images"], inputs["onehot"], inputs["noise"], inputs["alpha"], lam=LAM)
    return O.g_step(gp, dp, adam, t, inputs["images"], inputs["noise"])


def derived_stale(now, prev):
    """The parameters `now` with every tensor the encoder reads through a DERIVED copy taken from `prev`: the convolution kernels
    from conv1_2 on (Trunk.refresh_weights: conv1_1 has three input channels and is read from the arena, as are biases, LayerNorm
    parameters and the head)."""
    return OrderedDict((k, (prev[k] if (k.startswith("conv2d_") and k.endswith("/kernel")) else v)) for k, v in now.items())


def oracle_loss(kind, gp, dp, inputs):
    """The loss of update `kind` without an update: disc_cost / gen_cost as a float."""
    if kind == "D":
        return float(O.d_loss(gp, dp, inputs["images"], inputs["onehot"], inputs["noise"], inputs["alpha"], LAM)[0].detach())
    with torch.no_grad():
        return float(O.g_loss(gp, dp, inputs["images"], inputs["noise"])[0])


def free_run(dtype, before=None, B=B, S=S, V=V, schedule=SCHEDULE):
    """The schedule on the oracle alone in `dtype`, never resynchronised.  before(name, kind, gp, dp, adam, t, inputs), if given, sees
    the state each update starts from (adam, t: those of the network it updates).  Returns one record per update:
    {"name", "kind", "cost", "gp" (critic updates), "grads"}."""
    gp, dp = (to_dtype(d, dtype) for d in initial_states(V, S))
    adam = {"G": O.new_adam_state(gp), "D": O.new_adam_state(dp)}
    t = {"G": 0, "D": 0}
    images, _, onehot = minibatch(B, S, V)
    out = []
    for name, kind, it, i in schedule:
        inputs = oracle_inputs(images, onehot, *update_inputs(kind, it, i, B), dtype=dtype)
        if before is not None:
            before(name, kind, gp, dp, adam[kind], t[kind], inputs)
        t[kind] += 1
        cost, aux, grads = oracle_update(kind, gp, dp, adam[kind], t[kind], inputs)
        out.append({"name": name, "kind": kind, "cost": float(cost), "gp": float(aux["gp"].detach()) if kind == "D" else None, "grads": grads})
    return out


def tensor_err(a, b):
    """max|a - b| relative to max|b| (the gradient measure of tests/test_step_gpu.py)."""
    return float((a.detach().cpu().double() - b.double()).abs().max() / (b.double().abs().max() + 1e-7))


# ---- one Adam pass over flat arenas ------------------------------------------------------------------------------------------------
# tests/optim_ref.py derives its bounds for results that are zero or normal; the gradients of a training step are not chosen that way.
# An fp32 result below the smallest normal number is rounded on the denormal grid or flushed to zero, either way within 2^-126 of the
# exact value: m' and v' get that much room, and u (so p') what an error of that size in m', v', the product lr_t * m' or u itself
# can cause through the division by sqrt(v') + eps >= eps (lr_t < 1): 2^-126 * (2 / eps + 1).  A floor of 1e-30 at most, next to
# parameters and updates of 1e-1 .. 1e-6: it decides nothing an optimiser fault could hide behind.
TINY = 2.0 ** -126


def adam_expected(p, g, m, v, t, gscale=1.0):
    """One pass of the project's Adam (csrc/optim.hip) number t over flat fp32 arenas of any device: the fp64 result and the
    per-element bounds on |device - result|, both from tests/optim_ref.py (adam_terms = adam_ref with its intermediates, adam_bounds) on the
    oracle's lr_t and constants.  Returns ({"p", "m", "v"}, {"p", "m", "v"})."""
    lr_t = O.tf_adam_lr_t(t)
    terms = R.adam_terms(p, g, m, v, None, lr_t, O.ADAM_B1, O.ADAM_B2, O.ADAM_EPS, gscale, None)
    bound = R.adam_bounds(terms, p, None, lr_t, O.ADAM_B1, O.ADAM_B2, gscale, None)
    floor = {"m": TINY, "v": TINY, "p": TINY * (2.0 / R.f32(O.ADAM_EPS) + 1.0)}
    return {q: terms[q] for q in "pmv"}, {q: bound[q] + floor[q] for q in "pmv"}


def adam_check(what, before, grad, after, t, gscale=1.0, chunk=1 << 22):
    """before / after = (p, m, v) flat fp32 arenas around one pass that read `grad`: the worst |after - expected| / bound per quantity
    {"p", "m", "v"} (<= 1: inside), in chunks, on the tensors' device.  A NaN counts as outside (inf)."""
    worst = {q: 0.0 for q in "pmv"}
    n = before[0].numel()
    for lo in range(0, n, chunk):
        s = slice(lo, min(n, lo + chunk))
        ref, bound = adam_expected(before[0][s], grad[s], before[1][s], before[2][s], t, gscale)
        for q, got in zip("pmv", after):
            ratio = (got[s].double() - ref[q]).abs() / bound[q]
            ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
            worst[q] = max(worst[q], float(ratio.max()))
    return worst
