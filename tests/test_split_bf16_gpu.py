"""-m gpu: the three conv contraction modes agree at the full configs[1] layer shapes (224x224, all 12 layers):
generator logits and critic outputs of the split-bf16 modes against the native f32-MFMA mode on the same weights
and inputs.  Tolerances: mode 6 (6 products) 2e-5 + 2e-5*|ref| (its error vs fp64 equals native f32's);
mode 3 (3 products, drops 2^-17 cross terms) the path's stated 1e-4 + 1e-4*|ref|.  Tokens must be identical."""
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd.params import init_state_dict
from sgg_amd.step import GanStep

pytestmark = pytest.mark.gpu


def test_modes_agree_at_full_layer_shapes(hip):
    B, S, V = 4, 224, 1000
    images, labels, onehot = O.synth_batch(B, S, V)
    noise = O.synth_noise(B, 0)
    old = hip.conv_precision
    outs = {}
    try:
        gs = GanStep(hip, V, S, B, g_state=init_state_dict("G", V, S), d_state=init_state_dict("D", V, S))
        for mode in (0, 2, 6, 3):
            hip.conv_precision = mode
            gs.G.trunk.refresh_weights(); gs.D.trunk.refresh_weights()
            st, _ = gs.generator_forward(images.cuda(), noise.cuda())
            logits = st.OUT[0].clone()
            toks = gs.argmax_tokens(logits).clone()
            ctx = gs.D.trunk.forward(images.cuda())
            gs.D.head.precompute(ctx)
            dst = gs.D.head.state(1, B, "g")
            gs.D.head.forward(dst, ctx, [onehot.cuda()])
            outs[mode] = (logits, toks, dst.OUT[0].clone())
    finally:
        hip.conv_precision = old
    ref_logits, ref_toks, ref_d = outs[0]
    margin = O.top2_margin(ref_logits.cpu())
    for mode, tol in ((2, 2e-5), (6, 2e-5), (3, 1e-4)):
        lg, tk, dd = outs[mode]
        e1 = float((lg - ref_logits).abs().max())
        e2 = float((dd - ref_d).abs().max())
        print("mode %d: logits err %.3e, critic err %.3e (top-2 margin %.3e)" % (mode, e1, e2, margin))
        assert e1 <= tol + tol * float(ref_logits.abs().max())
        assert e2 <= tol + tol * float(ref_d.abs().max())
        assert torch.equal(tk, ref_toks) or margin < 10 * e1


def test_training_trajectory_default_mode_tracks_native_f32(hip):
    """Ten G+D iterations (critic_iters = 2, fresh noise / alpha per update) from the same weights in the default f16x3 mode and in
    native f32 MFMA arithmetic: the loss trajectories stay together (Adam amplifies rounding differences step by step: the bound
    grows with the iteration).  configs[0] shapes; the penalty is active (embedding scaled).  Both sides are the library: past the first
    update against the fp64 oracle: tests/test_trajectory_gpu.py."""
    B, S, V, iters, ci = 8, 64, 50, 10, 2
    images, labels, _ = O.synth_batch(B, S, V)
    gsd, dsd = init_state_dict("G", V, S), init_state_dict("D", V, S)
    dsd["W"] = dsd["W"] * 25.0
    old = hip.conv_precision
    traj = {}
    try:
        for mode in (0, 2):
            hip.conv_precision = mode
            gs = GanStep(hip, V, S, B, g_state=gsd, d_state=dsd)
            rows = []
            for it in range(iters):
                noises = [O.synth_noise(B, 100 + 3 * it + i).cuda() for i in range(ci + 1)]
                alphas = [O.synth_alpha(B, 100 + 3 * it + i).reshape(B).cuda() for i in range(ci)]
                gs.train_iteration(images.cuda(), labels.cuda(), noises, alphas, critic_iters=ci)
                rows.append(gs.d_losses.cpu().tolist()[:3] + [-float(gs.g_losses[3])])
            gs.flush()
            traj[mode] = torch.tensor(rows, dtype=torch.float64)
    finally:
        hip.conv_precision = old
    assert torch.isfinite(traj[2]).all() and float(traj[0][:, 2].max()) > 1e-3, "the run should exercise the gradient penalty"
    scale = traj[0].abs().max(dim=0).values + 1e-3
    err = ((traj[2] - traj[0]).abs() / scale).max(dim=1).values
    print("relative loss difference per iteration:", ["%.1e" % e for e in err.tolist()])
    assert float(err[0]) < 1e-4 and float(err[-1]) < 5e-3      # measured 6e-6 ... 7e-5
