"""Input gradients of the two networks: vector-Jacobian products with respect to the images (both networks) and the input triples
(critic), and per-word saliency maps - what `tf.gradients(fake_inputs, images)` / `tf.gradients(disc_fake, images)` give a user of
the reference graph (train.py:269-272).

A DATA-ONLY backward: the encoder forward (for_backward=True), the head forward, the head backward with every row feeding dP /
dctx and no parameter gradient (Head.backward(..., param_grads=False)), the data path of the attention product
(Head.finish_backward(..., param_grads=False)) and the encoder backward continued into conv1_1's input gradient
(Trunk.backward(..., param_grads=False, dimages=...)).  The parameter, gradient and Adam arenas are never written and no collective
is called; everything runs on the current stream.  Backend-agnostic: the same functions run on the HIP kernels and on the CPU
reference kernels (tests/test_input_grad_cpu.py).
"""
from __future__ import annotations

import torch

from .params import FEAT_C, T_STEPS


def _state(net, B):
    # (a head state of its own: never shared with a training pass)
    return net.head.state(1, B, "input-grad")


def _data_backward(net, st, ctx, dimages):
    net.head.backward(st, ctx, None, R_w=st.R, param_grads=False)
    dctx = net.head.finish_backward(ctx, param_grads=False)
    net.trunk.backward(dctx, param_grads=False, dimages=dimages)


def _forward(net, images):
    net.data_passes = getattr(net, "data_passes", 0) + 1      # (GanStep: G's encoder buffers were used since its last update)
    ctx = net.trunk.forward(images, for_backward=True)
    net.head.precompute(ctx)
    return ctx


def generator_image_gradient(net, images, noise, d_logits, dimages=None):
    """d <d_logits, G(images, noise)> / d images: images [B,S,S,3] (standardised), noise [B,512], d_logits [B,3,V] -> [B,S,S,3].
    Returns (dimages, head state, ctx) - the state holds the forward's logits (OUT) and attention (AL)."""
    B = int(images.shape[0])
    assert net.kind == "G" and tuple(d_logits.shape) == (B, T_STEPS, net.arena.V), d_logits.shape
    ctx = _forward(net, images)
    st = _state(net, B)
    net.head.forward(st, ctx, noise)
    st.dOUT[0].copy_(d_logits)
    if dimages is None:
        dimages = torch.empty_like(images)
    _data_backward(net, st, ctx, dimages)
    return dimages, st, ctx


def discriminator_input_gradients(net, triples, images, d_scores):
    """Gradients of <d_scores, D(triples, images)> with respect to the triples [B,3,V] (one-hot or logits) and the images [B,S,S,3]:
    d_scores [B,3,1] -> (d_triples [B,3,V], d_images [B,S,S,3], head state, ctx)."""
    B, K = int(images.shape[0]), net.K
    assert net.kind == "D" and tuple(d_scores.shape) == (B, T_STEPS, 1) and tuple(triples.shape) == (B, T_STEPS, net.arena.V)
    ctx = _forward(net, images)
    st = _state(net, B)
    net.head.forward(st, ctx, [triples])
    st.dOUT[0].copy_(d_scores)
    d_images = torch.empty_like(images)
    _data_backward(net, st, ctx, d_images)
    d_triples = torch.empty_like(triples)
    ind = net.head.in_dim
    for t in range(T_STEPS):
        # u_t = triples[:, t] @ W (discriminator_with_attention.py:87): d triples[:, t] = d u_t @ W^T
        K.gemm_nt(st.dXH[t][0][:, FEAT_C:ind], net.head.W_emb, d_triples[:, t, :])
    return d_triples, d_images, st, ctx


def generator_saliency(net, images, noise):
    """Per-word saliency of the generator's argmax triple (Simonyan et al. 2014): one forward, then for each of the three words t
    the image gradient of logit[b, t, token_bt] - three data-only backwards from that ONE forward (same noise, same activations; the
    dP / dctx accumulators are re-zeroed between them).  Returns (tokens [B,3] int64, grads [3,B,S,S,3], head state, ctx)."""
    B, K, V = int(images.shape[0]), net.K, net.arena.V
    assert net.kind == "G"
    ctx = _forward(net, images)
    st = _state(net, B)
    net.head.forward(st, ctx, noise)
    tokens = torch.empty((B, T_STEPS), dtype=torch.int64, device=images.device)
    K.argmax_rows(st.OUT[0], tokens.view(-1))
    onehot = torch.empty((B, T_STEPS, V), dtype=images.dtype, device=images.device)
    K.onehot(tokens, onehot)
    grads = torch.empty((T_STEPS,) + tuple(images.shape), dtype=images.dtype, device=images.device)
    for t in range(T_STEPS):
        if t:
            K.fill(net.head.dP, 0.0)
            K.fill(net.head.dctx, 0.0)
        K.fill(st.dOUT, 0.0)
        st.dOUT[0][:, t, :].copy_(onehot[:, t, :])
        _data_backward(net, st, ctx, grads[t])
    return tokens, grads, st, ctx
