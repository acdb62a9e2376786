"""Drop-in for the reference's architectures/generator_with_attention.py (class Generator), MI355X-native.

Same import path, constructor and method signatures as the reference (generator_with_attention.py:8-91):
    Generator(vocab_size)
    Generator.build_generator(images, is_training=True) -> logits [B, 3, vocab]      (raw logits, no softmax)
    Generator.attentionMechanism(cell_state)            -> z_hat  [B, 512]           (cell_state = (c, h), c is used)
    attributes after a build: downsampled, flattened_context, partially_flattened_context, alpha
Added (evaluation): Generator.sample(images, num_samples, noise=None) -> logits [N, B, 3, vocab] on one encoder pass.
Added (input gradients): Generator.image_gradient(images, d_logits, noise=None) -> [B, S, S, 3], the vector-Jacobian product of
build_generator with respect to the images (what tf.gradients(fake_inputs, images, d_logits) gives in the reference graph).
Added (likelihood): Generator.log_prob(images, triples, counts, num_samples, noise=None) -> the log-probability of given triples
under the mixture of num_samples noise draws (the product of the three softmaxes per draw).
In the reference these methods add TensorFlow ops to a graph; here they run eagerly on the GPU: every arithmetic
op is a hand-written HIP kernel behind the C ABI of libsgg_hip.so (include/sgg_hip.h).  Repeated builds share one
set of weights, as `reuse=tf.AUTO_REUSE` does (train.py:86).  `is_training` is accepted and ignored, as in the
reference (no dropout / batch-norm).  There is no CPU fallback.
"""
import os
import sys

sys.path.append(os.getcwd())
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import torch  # noqa: E402

import sgg_amd  # noqa: E402,F401
from sgg_amd import grad  # noqa: E402
from sgg_amd.api import NetworkHandle  # noqa: E402


class Generator(NetworkHandle):

    def __init__(self, vocab_size):
        NetworkHandle.__init__(self, "G", vocab_size)

    def attentionMechanism(self, cell_state):
        return self._attention(cell_state)

    def build_generator(self, images, is_training=True, noise=None):
        """images: float32 NHWC [B, S, S, 3], already standardised (train.py:172).  `noise` [B, 512] replaces the
        in-graph tf.random_normal of the reference (generator_with_attention.py:81); drawn with torch.randn if None."""
        net = self._ensure(images)
        if noise is None:
            noise = torch.randn((images.shape[0], 512), device=images.device, dtype=torch.float32)
        ctx = net.trunk.forward(images.contiguous())
        net.head.precompute(ctx)
        st = net.head.state(1, images.shape[0])
        net.head.forward(st, ctx, noise)
        self._publish(ctx, st)
        return st.OUT[0]

    def sample(self, images, num_samples, noise=None):
        """num_samples generator samples of each image on ONE encoder pass: images [B, S, S, 3] (standardised) -> logits
        [N, B, 3, vocab].  Sample k of image b is head row k*B + b (the returned tensor is a view of the head's rows; the next
        call overwrites it).  `noise` [N, B, 512] (torch.randn if None)."""
        net = self._ensure(images)
        B, N = int(images.shape[0]), int(num_samples)
        if noise is None:
            noise = torch.randn((N, B, 512), device=images.device, dtype=torch.float32)
        assert tuple(noise.shape) == (N, B, 512), noise.shape
        ctx = net.trunk.forward(images.contiguous(), for_backward=False)
        net.head.precompute(ctx)
        st = net.head.sample_state(N * B)
        net.head.forward(st, ctx, noise.contiguous().view(N * B, 512))
        self._publish(ctx, st)
        return st.OUT[0].view(N, B, 3, self.vocab_size)

    def log_prob(self, images, triples, counts, num_samples, noise=None):
        """The log-probability the generator assigns to given triples: images [B, S, S, 3] (standardised), triples int64 [B, M, 3],
        counts int32 [B] (rows m >= counts[b] are padding), num_samples noise draws per image (`noise` [N, B, 512], torch.randn if
        None).  Returns (mix [B, M], mean [B, M], slot [B, M, 3], status int32 [B, M]): the log-probability under the mixture of
        the N draws, the mean over the draws of the per-draw log-probability, that mean per slot, and 0 / -3 (padding) / -4 (a
        token outside the vocabulary; the floats of such rows are NaN).  sample(), then the log-sum-exp of every decoder row
        (softmax_xent without labels), then triple_logp (csrc/xent.hip).  Touches no weights."""
        logits = self.sample(images, num_samples, noise)
        K = self._last.K
        N, B = int(logits.shape[0]), int(logits.shape[1])
        lse = torch.empty((N, B, 3), device=logits.device, dtype=logits.dtype)
        K.softmax_xent(logits, None, lse=lse.view(-1))
        res = K.triple_logp(logits, lse, triples.contiguous(), counts.contiguous())
        return res["mix"], res["mean"], res["slot"], res["status"]

    def image_gradient(self, images, d_logits, noise=None):
        """d <d_logits, build_generator(images, noise)> / d images: images [B, S, S, 3] (standardised), d_logits [B, 3, vocab] ->
        [B, S, S, 3] (a new tensor).  `noise` [B, 512] as in build_generator (torch.randn if None).  A data-only backward
        (sgg_amd/grad.py): the weights, their gradients and the optimiser state are not touched.  The build's attributes
        (downsampled, alpha, alphas) are published as by build_generator."""
        net = self._ensure(images)
        B = int(images.shape[0])
        if noise is None:
            noise = torch.randn((B, 512), device=images.device, dtype=torch.float32)
        assert tuple(d_logits.shape) == (B, 3, self.vocab_size), d_logits.shape
        dimages, st, ctx = grad.generator_image_gradient(net, images.contiguous(), noise.contiguous(), d_logits.contiguous())
        self._publish(ctx, st)
        return dimages

    def saliency_gradients(self, images, noise=None):
        """The generator's argmax triple and, per word t, d logit[b, t, token_bt] / d image[b] - three data-only backwards from ONE
        forward (one noise draw for all three words).  Returns (tokens [B, 3] int64, grads [3, B, S, S, 3], noise); the attention of
        the three steps is published in `alphas`."""
        net = self._ensure(images)
        if noise is None:
            noise = torch.randn((images.shape[0], 512), device=images.device, dtype=torch.float32)
        tokens, grads, st, ctx = grad.generator_saliency(net, images.contiguous(), noise.contiguous())
        self._publish(ctx, st)
        return tokens, grads, noise
