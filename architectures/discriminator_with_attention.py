"""Drop-in for the reference's architectures/discriminator_with_attention.py (class Discriminator), MI355X-native.

Same import path, constructor and method signatures as the reference (discriminator_with_attention.py:7-93):
    Discriminator(vocab_size, embedding_matrix)
    Discriminator.build_discriminator(input_triples, images, is_training=True) -> critic logits [B, 3, 1]
    Discriminator.attentionMechanism(cell_state) -> z_hat [B, 512]
Added (evaluation): Discriminator.score_samples(input_triples [N, B, 3, vocab], images) -> [N, B, 3, 1] on one encoder pass.
Added (input gradients): Discriminator.input_gradients(input_triples, images, d_scores [B, 3, 1]) -> (d_triples [B, 3, vocab],
d_images [B, S, S, 3]), the vector-Jacobian product of build_discriminator (tf.gradients(disc_fake, [inputs, images], d_scores)).
`input_triples` is float32 [B, 3, vocab]: one-hot real triples or raw generator logits (train.py:173, 242).
`embedding_matrix` [vocab, 300] is created by the trainer and trained by the critic's optimiser
(train.py:68-72, 263); here its storage moves into the critic's parameter arena and `self.embedding_matrix`
is the live view of it.  Every arithmetic op is a HIP kernel behind libsgg_hip.so; no CPU fallback.
"""
import os
import sys

sys.path.append(os.getcwd())
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import sgg_amd  # noqa: E402,F401
from sgg_amd import grad  # noqa: E402
from sgg_amd.api import NetworkHandle  # noqa: E402
from sgg_amd.step import need_kernels  # noqa: E402


class Discriminator(NetworkHandle):

    def __init__(self, vocab_size, embedding_matrix):
        NetworkHandle.__init__(self, "D", vocab_size)
        self.embedding_matrix = embedding_matrix

    def attentionMechanism(self, cell_state):
        return self._attention(cell_state)

    def build_discriminator(self, input_triples, images, is_training=True):
        net = self._ensure(images)
        B = images.shape[0]
        ctx = net.trunk.forward(images.contiguous())
        net.head.precompute(ctx)
        st = net.head.state(1, B, "api")
        net.head.forward(st, ctx, [input_triples.contiguous()])
        self._publish(ctx, st)
        return st.OUT[0]

    def score_samples(self, input_triples, images, relax_tau=None, relax_hard=False):
        """Critic outputs of N triples per image on ONE encoder pass: input_triples [N, B, 3, vocab] (one-hots or generator
        logits, e.g. Generator.sample's output), images [B, S, S, 3] -> [N, B, 3, 1].  Row k*B + b reads image b; the returned
        tensor is a view of the head's rows (the next call overwrites it).
        relax_tau = tau > 0: the critic of a run with a relaxed generator output - input_triples are logits and are replaced IN PLACE
        by softmax(logits / tau) before the critic reads them (one launch, csrc/relax.hip; a contiguous input_triples is the
        caller's own tensor: take its argmax first).
        relax_hard: the critic of a straight-through run - the logits are replaced IN PLACE by onehot(argmax(logits)) instead, without
        noise and whatever the temperature: the scored row is the token argmax_rows reports."""
        net = self._ensure(images)
        B = int(images.shape[0])
        N = int(input_triples.shape[0])
        assert tuple(input_triples.shape) == (N, B, 3, self.vocab_size), input_triples.shape
        rows = input_triples.contiguous().view(N * B, 3, self.vocab_size)
        if relax_hard:
            need_kernels(net.K, "score_samples(relax_hard)", "relax_rows_hard")
            net.K.relax_rows_hard(rows)
        elif relax_tau is not None:
            need_kernels(net.K, "score_samples(relax_tau)", "relax_rows")
            net.K.relax_rows(rows, float(relax_tau))
        ctx = net.trunk.forward(images.contiguous(), for_backward=False)
        net.head.precompute(ctx)
        st = net.head.sample_state(N * B)
        net.head.forward(st, ctx, [rows])
        self._publish(ctx, st)
        return st.OUT[0].view(N, B, 3, 1)

    def input_gradients(self, input_triples, images, d_scores):
        """Gradients of <d_scores, build_discriminator(input_triples, images)>: input_triples [B, 3, vocab] (one-hots or logits),
        images [B, S, S, 3], d_scores [B, 3, 1] -> (d_triples [B, 3, vocab], d_images [B, S, S, 3]), new tensors.  A data-only
        backward (sgg_amd/grad.py): the weights, their gradients and the optimiser state are not touched."""
        net = self._ensure(images)
        B = int(images.shape[0])
        assert tuple(input_triples.shape) == (B, 3, self.vocab_size), input_triples.shape
        assert tuple(d_scores.shape) == (B, 3, 1), d_scores.shape
        d_tri, d_img, st, ctx = grad.discriminator_input_gradients(net, input_triples.contiguous(), images.contiguous(),
                                                                   d_scores.contiguous())
        self._publish(ctx, st)
        return d_tri, d_img
