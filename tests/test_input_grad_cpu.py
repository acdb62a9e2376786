"""CPU: input gradients (sgg_amd/grad.py) - the data-only backward of both networks continued into conv1_1's input gradient - with
the kernel-level reference injected in place of the HIP binding, against torch.autograd through the fp64 oracle.  Pins the schedule
(every head row feeds dP / dctx, the attention product's data path, the encoder backward past layer 1, the canvas crop of odd
sizes) and that nothing of the parameter, gradient or Adam arenas is written."""
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from oracle.kernels_ref import RefKernels
from sgg_amd import grad
from sgg_amd.step import Network

DT = torch.float64


class InputGradRefKernels(RefKernels):
    """RefKernels plus conv1_1's input-gradient entry points of the HIP backend (csrc/conv_dgrad_c3.hip), in torch."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def conv_c3_dgrad(self, dy, w_hwio, dx):
        assert dy.shape[3] == 32 and dx.shape[3] == 3
        self.calls.append("conv_c3_dgrad")
        self.conv_dgrad(dy, w_hwio, dx, 1)

    def conv_c3_dgrad_ln(self, y, da, gamma, beta, stats, means, w_hwio, dx):
        self.calls.append("conv_c3_dgrad_ln")
        mean, rstd = stats[:, 0, None, None, None], stats[:, 1, None, None, None]
        m1, m2 = means[:, 0, None, None, None], means[:, 1, None, None, None]
        xh = (y - mean) * rstd
        n = xh * gamma + beta
        dy = rstd * (da * torch.where(n > 0, torch.ones_like(n), torch.exp(n)) * gamma - m1 - xh * m2)
        self.conv_dgrad(dy, w_hwio, dx, 1)


def rel_err(a, b, floor=1e-30):
    return float((a - b).abs().max() / (b.abs().max() + floor))


def arenas(net):
    return [t.clone() for t in (net.arena.flat, net.grad_flat, net.m_flat, net.v_flat)]


def poison(net):
    # non-zero gradient / Adam slots, so that a stray write of zeros would show as well
    g = torch.Generator().manual_seed(5)
    for t in (net.grad_flat, net.m_flat, net.v_flat):
        t.copy_(torch.randn(t.shape, generator=g, dtype=t.dtype))


@pytest.fixture(scope="module", params=[32, 29])     # 29: odd maps on even canvases (trunk.plan_canvas)
def setup(request):
    B, S, V = 2, request.param, 11
    gp = O.init_params("G", V, S, dtype=DT, perturb=0.1)
    dp = O.init_params("D", V, S, dtype=DT, perturb=0.1)
    images, labels, onehot = O.synth_batch(B, S, V, dtype=DT)
    K = InputGradRefKernels()
    G = Network(K, "G", V, S, B, dtype=DT, state_dict=gp)
    D = Network(K, "D", V, S, B, dtype=DT, state_dict=dp)
    poison(G)
    poison(D)
    return dict(B=B, S=S, V=V, gp=gp, dp=dp, images=images, onehot=onehot, K=K, G=G, D=D)


def test_generator_image_gradient_matches_autograd(setup):
    s = setup
    B, S, V = s["B"], s["S"], s["V"]
    noise = O.synth_noise(B, 0, DT)
    d_logits = torch.randn((B, 3, V), generator=torch.Generator().manual_seed(11), dtype=DT)
    before = arenas(s["G"])
    s["K"].calls.clear()
    dimg, st, _ = grad.generator_image_gradient(s["G"], s["images"], noise, d_logits)
    assert "conv_c3_dgrad" in s["K"].calls
    img = s["images"].clone().requires_grad_(True)
    logits = O.generator_forward(s["gp"], img, noise)
    (ref,) = torch.autograd.grad(logits, img, d_logits)
    assert rel_err(st.OUT[0], logits.detach()) < 1e-10
    assert rel_err(dimg, ref) < 1e-9, rel_err(dimg, ref)
    for a, b in zip(before, arenas(s["G"])):
        assert torch.equal(a, b), "an arena changed"


def test_discriminator_input_gradients_match_autograd(setup):
    s = setup
    B, V = s["B"], s["V"]
    gen = torch.Generator().manual_seed(12)
    for triples in (s["onehot"], torch.randn((B, 3, V), generator=gen, dtype=DT)):     # one-hot real triples / generator logits
        d_scores = torch.randn((B, 3, 1), generator=gen, dtype=DT)
        before = arenas(s["D"])
        d_tri, d_img, _, _ = grad.discriminator_input_gradients(s["D"], triples.contiguous(), s["images"], d_scores)
        tri = triples.clone().requires_grad_(True)
        img = s["images"].clone().requires_grad_(True)
        out = O.discriminator_forward(s["dp"], tri, img)
        ref_tri, ref_img = torch.autograd.grad(out, (tri, img), d_scores)
        assert rel_err(d_tri, ref_tri) < 1e-9, rel_err(d_tri, ref_tri)
        assert rel_err(d_img, ref_img) < 1e-9, rel_err(d_img, ref_img)
        for a, b in zip(before, arenas(s["D"])):
            assert torch.equal(a, b), "an arena changed"


def test_generator_saliency_definition(setup):
    s = setup
    B, S = s["B"], s["S"]
    noise = O.synth_noise(B, 1, DT)
    before = arenas(s["G"])
    tokens, grads, st, _ = grad.generator_saliency(s["G"], s["images"], noise)
    img = s["images"].clone().requires_grad_(True)
    logits = O.generator_forward(s["gp"], img, noise)
    assert torch.equal(tokens, O.argmax_tokens(logits.detach()))
    for t in range(3):
        # logit[b, t, token_bt] of image b depends on image b only: one autograd call over the batch gives every image's gradient
        sel = logits[torch.arange(B), t, tokens[:, t]].sum()
        (ref,) = torch.autograd.grad(sel, img, retain_graph=True)
        assert rel_err(grads[t], ref) < 1e-9, (t, rel_err(grads[t], ref))
        sal = grads[t].abs().amax(dim=-1)
        assert sal.shape == (B, S, S)
        assert rel_err(sal, ref.abs().amax(dim=-1)) < 1e-9
    for a, b in zip(before, arenas(s["G"])):
        assert torch.equal(a, b), "an arena changed"


def test_fused_dy_formula_matches_layernorm_backward():
    """conv_c3_dgrad_ln's dy (the formula the HIP kernel uses) equals the LayerNorm backward of the reference kernels."""
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 5, 7
    y = torch.randn((B, H, W, 32), generator=g, dtype=DT)
    da = torch.randn((B, H, W, 32), generator=g, dtype=DT)
    gamma = 1 + 0.1 * torch.randn(32, generator=g, dtype=DT)
    beta = 0.1 * torch.randn(32, generator=g, dtype=DT)
    w = torch.randn((3, 3, 3, 32), generator=g, dtype=DT)
    K = InputGradRefKernels()
    a, stats = torch.empty_like(y), torch.empty((B, 2), dtype=DT)
    K.ln_elu_fwd(y, gamma, beta, a, stats)
    dy = torch.empty_like(y)
    K.ln_elu_bwd(y, da, gamma, beta, stats, dy, torch.empty(32, dtype=DT), torch.empty(32, dtype=DT), None)
    xh = (y - stats[:, 0, None, None, None]) * stats[:, 1, None, None, None]
    n = xh * gamma + beta
    dxh = da * torch.where(n > 0, torch.ones_like(n), torch.exp(n)) * gamma
    means = torch.stack([dxh.mean(dim=(1, 2, 3)), (dxh * xh).mean(dim=(1, 2, 3))], dim=1)
    dx_fused, dx_plain = torch.empty((B, H, W, 3), dtype=DT), torch.empty((B, H, W, 3), dtype=DT)
    K.conv_c3_dgrad_ln(y, da, gamma, beta, stats, means, w, dx_fused)
    K.conv_c3_dgrad(dy, w, dx_plain)
    assert rel_err(dx_fused, dx_plain) < 1e-12
