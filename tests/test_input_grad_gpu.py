"""-m gpu: input gradients on the MI355X - conv1_1's input-gradient kernels (csrc/conv_dgrad_c3.hip, plain and LayerNorm-fused)
against fp64, the data-only backward of both networks end to end against the fp64 oracle's autograd, non-interference with the
training step, the per-word saliency maps and train.py --saliency_dir."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from tests.tolerances import GRAD_RTOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(hip_t, ref_t, rtol=2e-5, atol=1e-6, what=""):
    h = hip_t.detach().cpu().double()
    r = ref_t.detach().cpu().double()
    assert h.shape == r.shape, (what, h.shape, r.shape)
    assert torch.isfinite(h).all(), what + ": non-finite values"
    tol = atol + rtol * float(r.abs().max())
    err = float((h - r).abs().max())
    assert err <= tol, "%s: max err %.3e > tol %.3e (max|ref| %.3e)" % (what, err, tol, float(r.abs().max()))


def dgrad64(dy, w):
    """Conv2DBackpropInput of a 3x3 stride-1 SAME convolution in fp64 on the host: dy [B,H,W,32], w [3,3,3,32] -> [B,H,W,3]."""
    dy, w = dy.detach().cpu().double(), w.detach().cpu().double()
    x0 = torch.zeros(dy.shape[:3] + (3,), dtype=torch.float64, requires_grad=True)
    y = O.conv2d_same(x0, w, torch.zeros(32, dtype=torch.float64), 1)
    (g,) = torch.autograd.grad(y, x0, dy)
    return g


def ln_operands(hip, B, H, W, seed):
    """Device (y, da, gamma, beta, w, stats, means, dy): stats from the LayerNorm forward, dy and means from its backward (the apply
    pass / the reduction-only call on the same operands)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.randn((B, H, W, 32), generator=g, device="cuda") * 0.7 + 0.2
    da = torch.randn((B, H, W, 32), generator=g, device="cuda")
    gamma = 1.0 + 0.2 * torch.randn(32, generator=g, device="cuda")
    beta = 0.2 * torch.randn(32, generator=g, device="cuda")
    w = torch.randn((3, 3, 3, 32), generator=g, device="cuda") * 0.1
    a, stats = torch.empty_like(y), torch.empty((B, 2), device="cuda")
    hip.ln_elu_fwd(y, gamma, beta, a, stats)
    nws = hip.ln_workspace_bytes(y.shape)
    dy, means = torch.empty_like(y), torch.empty((B, 2), device="cuda")
    hip.ln_elu_bwd(y, da, gamma, beta, stats, dy, None, None, None, ws=torch.empty(nws, dtype=torch.uint8, device="cuda"))
    hip.ln_elu_bwd_sums(y, da, gamma, beta, stats, means, torch.empty(nws, dtype=torch.uint8, device="cuda"))
    return y, da, gamma, beta, w, stats, means, dy


def fused_dy64(y, da, gamma, beta, stats, means):
    y, da, gamma, beta, stats, means = (t.detach().cpu().double() for t in (y, da, gamma, beta, stats, means))
    xh = (y - stats[:, 0, None, None, None]) * stats[:, 1, None, None, None]
    n = xh * gamma + beta
    dn = da * torch.where(n > 0, torch.ones_like(n), torch.exp(n))
    return stats[:, 1, None, None, None] * (dn * gamma - means[:, 0, None, None, None] - xh * means[:, 1, None, None, None])


# ---- kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 224, 224), (2, 221, 221), (2, 29, 45), (2, 8, 33), (3, 17, 5)])
def test_c3_dgrad_kernels_vs_fp64(hip, B, H, W):
    y, da, gamma, beta, w, stats, means, dy = ln_operands(hip, B, H, W, seed=H * 1000 + W)
    dx = torch.empty((B, H, W, 3), device="cuda")
    hip.conv_c3_dgrad(dy, w, dx)
    close(dx, dgrad64(dy, w), what="conv_c3_dgrad %s" % ((B, H, W),))
    dxf = torch.empty_like(dx)
    hip.conv_c3_dgrad_ln(y, da, gamma, beta, stats, means, w, dxf)
    close(dxf, dgrad64(fused_dy64(y, da, gamma, beta, stats, means), w), rtol=1e-4, what="conv_c3_dgrad_ln %s" % ((B, H, W),))
    # the fused form = the LayerNorm backward's apply pass followed by the plain form
    close(dxf, dx, rtol=1e-4, what="fused vs apply + plain")
    # fixed summation order: two calls are bit-equal
    dx2, dxf2 = torch.empty_like(dx), torch.empty_like(dx)
    hip.conv_c3_dgrad(dy, w, dx2)
    hip.conv_c3_dgrad_ln(y, da, gamma, beta, stats, means, w, dxf2)
    assert torch.equal(dx, dx2) and torch.equal(dxf, dxf2)


def test_c3_dgrad_kernels_batch64(hip):
    """The production shape (no fp64 oracle at this size): fused = apply + plain, and bit-equal repeats."""
    B, H, W = 64, 224, 224
    y, da, gamma, beta, w, stats, means, dy = ln_operands(hip, B, H, W, seed=64)
    dx, dxf = torch.empty((B, H, W, 3), device="cuda"), torch.empty((B, H, W, 3), device="cuda")
    hip.conv_c3_dgrad(dy, w, dx)
    hip.conv_c3_dgrad_ln(y, da, gamma, beta, stats, means, w, dxf)
    close(dxf, dx, rtol=1e-4, what="batch 64: fused vs apply + plain")
    dx2, dxf2 = torch.empty_like(dx), torch.empty_like(dx)
    hip.conv_c3_dgrad(dy, w, dx2)
    hip.conv_c3_dgrad_ln(y, da, gamma, beta, stats, means, w, dxf2)
    assert torch.equal(dx, dx2) and torch.equal(dxf, dxf2)


def test_c3_dgrad_argument_errors(hip):
    from sgg_amd.lib import SggError
    dy, w = torch.zeros((1, 8, 8, 32), device="cuda"), torch.zeros((3, 3, 3, 32), device="cuda")
    with pytest.raises(SggError):
        hip.conv_c3_dgrad(dy, w, torch.empty((1, 8, 8, 4), device="cuda"))
    rc = hip.lib.sgg_conv2d_nhwc_dgrad_c3(dy.data_ptr(), w.data_ptr(), dy.data_ptr(), 1, 8, 8, 0, 1, None)
    assert rc != 0 and b"bad dims" in hip.lib.sgg_last_error()


# ---- end to end against the fp64 oracle ------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_case(B, S, V):
    key = (B, S, V)
    if key not in _ORACLE:
        gp, dp = O.init_params("G", V, S), O.init_params("D", V, S)
        images, _, onehot = O.synth_batch(B, S, V)
        noise = O.synth_noise(B, 0)
        g = torch.Generator().manual_seed(21)
        d_logits, d_scores = torch.randn((B, 3, V), generator=g), torch.randn((B, 3, 1), generator=g)
        triples = torch.randn((B, 3, V), generator=g)
        p64 = lambda p: {k: v.double() for k, v in p.items()}
        img = images.double().requires_grad_(True)
        (g_img,) = torch.autograd.grad(O.generator_forward(p64(gp), img, noise.double()), img, d_logits.double())
        tri, img = triples.double().requires_grad_(True), images.double().requires_grad_(True)
        d_tri, d_img = torch.autograd.grad(O.discriminator_forward(p64(dp), tri, img), (tri, img), d_scores.double())
        _ORACLE[key] = dict(gp=gp, dp=dp, images=images, noise=noise, d_logits=d_logits, d_scores=d_scores, triples=triples,
                            g_img=g_img, d_tri=d_tri, d_img=d_img)
    return _ORACLE[key]


def grad_close(got, ref, what):
    err = float((got.detach().cpu().double() - ref).abs().max())
    assert err <= GRAD_RTOL * float(ref.abs().max()), "%s: max|d| %.3e > %.1e * max|ref| %.3e" % (what, err, GRAD_RTOL, float(ref.abs().max()))


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("B,S,V", [(2, 64, 50), (2, 224, 1000), (2, 221, 1000)])
def test_input_gradients_match_oracle(hip, B, S, V, mode):
    from sgg_amd import grad
    from sgg_amd.step import Network
    c = oracle_case(B, S, V)
    old = hip.conv_precision
    hip.conv_precision = mode
    try:
        G = Network(hip, "G", V, S, B, state_dict=c["gp"])
        D = Network(hip, "D", V, S, B, state_dict=c["dp"])
        before = [t.clone() for n in (G, D) for t in (n.arena.flat, n.grad_flat, n.m_flat, n.v_flat)]
        g_img, _, _ = grad.generator_image_gradient(G, c["images"].cuda(), c["noise"].cuda(), c["d_logits"].cuda())
        d_tri, d_img, _, _ = grad.discriminator_input_gradients(D, c["triples"].cuda(), c["images"].cuda(), c["d_scores"].cuda())
        torch.cuda.synchronize()
        grad_close(g_img, c["g_img"], "G image gradient (mode %d)" % mode)
        grad_close(d_tri, c["d_tri"], "D triple gradient (mode %d)" % mode)
        grad_close(d_img, c["d_img"], "D image gradient (mode %d)" % mode)
        after = [t for n in (G, D) for t in (n.arena.flat, n.grad_flat, n.m_flat, n.v_flat)]
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "a parameter / gradient / Adam arena changed"
    finally:
        hip.conv_precision = old


# ---- public interface ------------------------------------------------------------------------------------------------------------
def _arenas(h):
    n = h.net
    return [t.clone() for t in (n.arena.flat, n.grad_flat, n.m_flat, n.v_flat)]


def test_api_non_interference():
    """Generator.image_gradient / Discriminator.input_gradients leave every arena bit-equal, and a GanStep critic + generator step
    on the same objects gives bit-identical losses and weights whether or not they ran before it (two-stream schedule)."""
    from architectures.generator_with_attention import Generator
    from architectures.discriminator_with_attention import Discriminator
    from sgg_amd.api import kernels_for
    from sgg_amd.step import GanStep
    B, S, V = 2, 64, 50
    images, labels, onehot = (t.cuda() for t in O.synth_batch(B, S, V))
    emb = torch.rand((V, 300), generator=torch.Generator().manual_seed(3)) * 0.2 - 0.1
    gen = torch.Generator().manual_seed(8)
    noises = [torch.randn((B, 512), generator=gen).cuda() for _ in range(4)]
    alphas = [torch.rand((B,), generator=gen).cuda() for _ in range(2)]
    d_logits, d_scores = torch.randn((B, 3, V), generator=gen).cuda(), torch.randn((B, 3, 1), generator=gen).cuda()

    def run(with_grads):
        g, d = Generator(V), Discriminator(V, emb.clone())
        gs = GanStep(kernels_for(images.device), V, S, B, G=g._ensure(images), D=d._ensure(images), overlap_streams=True)
        gs.critic_step(images, labels, noises[0], alphas[0])
        if with_grads:
            gs.flush()
            before = _arenas(g) + _arenas(d)
            dimg = g.image_gradient(images, d_logits, noises[3])
            d_tri, d_img = d.input_gradients(onehot, images, d_scores)
            assert tuple(dimg.shape) == (B, S, S, 3) and tuple(d_tri.shape) == (B, 3, V) and tuple(d_img.shape) == (B, S, S, 3)
            assert tuple(g.alphas.shape) == (B, 3, 16) and torch.equal(g.alphas[:, 2], g.alpha)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(before, _arenas(g) + _arenas(d))), "an arena changed"
        gs.critic_step(images, labels, noises[1], alphas[1])
        gs.generator_step(images, noises[2])
        gs.flush()
        torch.cuda.synchronize()
        return [gs.d_losses.clone(), gs.g_losses.clone()] + _arenas(g) + _arenas(d)

    plain, with_grads = run(False), run(True)
    for a, b in zip(plain, with_grads):
        assert torch.equal(a, b), "the training step changed after an input-gradient call"


def test_saliency_equals_separate_image_gradients():
    from architectures.generator_with_attention import Generator
    B, S, V = 2, 64, 50
    images = O.synth_batch(B, S, V)[0].cuda()
    noise = O.synth_noise(B, 2).cuda()
    g = Generator(V)
    tokens, grads, used = g.saliency_gradients(images, noise)
    assert torch.equal(used, noise)
    logits = g.build_generator(images, noise=noise)
    toks = torch.empty((B, 3), dtype=torch.int64, device="cuda")
    g._last.K.argmax_rows(logits, toks.view(-1))
    assert torch.equal(tokens, toks)
    for t in range(3):
        cot = torch.zeros((B, 3, V), device="cuda")
        cot[torch.arange(B), t, tokens[:, t]] = 1.0
        ig = g.image_gradient(images, cot, noise)
        close(grads[t], ig, rtol=1e-6, atol=0.0, what="saliency word %d vs image_gradient" % t)


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
def test_saliency_cli(tmp_path):
    import train as T
    script = os.path.join(ROOT, "train.py")
    common = ["--synthetic", "2,64,50", "--batch_size", "2", "--critic_iters", "1", "--checkpoints_dir", str(tmp_path / "ck"),
              "--summaries_dir", str(tmp_path / "logs")]
    run = lambda extra: subprocess.run([sys.executable, script] + common + extra, cwd=str(tmp_path), capture_output=True, text=True,
                                       timeout=600)
    r = run(["--max_iterations", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(str(tmp_path / "ck" / "model.ckpt.pt"))
    out = tmp_path / "maps"
    r = run(["--saliency_dir", str(out), "--max_test_images", "3"])
    assert r.returncode == 0, r.stderr[-3000:]
    index = json.loads((out / "index.json").read_text())
    assert sorted(index) == ["0", "1", "2"]
    gan = T.SceneGraphGAN(str(tmp_path / "ck"), str(tmp_path / "logs2"), None, None, None, None, None, critic_iters=1, batch_size=2,
                          lambda_=10, resume=False, synthetic=(2, 64, 50))
    assert gan.load_checkpoint()
    for key, image in gan._saliency_items(3):
        rec = np.load(str(out / index[key]["file"]))
        noise = torch.from_numpy(rec["noise"]).cuda()[None]
        res = gan.saliency(image[None].cuda(), noise)
        assert index[key]["words"] == res["words"][0] == list(rec["words"])
        assert np.array_equal(rec["tokens"], res["tokens"][0].cpu().numpy())
        assert rec["saliency"].shape == (3, 64, 64) and rec["attention"].shape == (3, 4, 4)
        np.testing.assert_allclose(rec["saliency"], res["saliency"][0].cpu().numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(rec["attention"], res["attention"][0].cpu().numpy(), rtol=1e-5, atol=1e-7)
    empty = tmp_path / "none"
    r = subprocess.run([sys.executable, script, "--synthetic", "2,64,50", "--batch_size", "2", "--saliency_dir", str(empty / "maps"),
                        "--checkpoints_dir", str(empty / "ck"), "--summaries_dir", str(empty / "logs")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "no checkpoint" in r.stderr
