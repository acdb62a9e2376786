"""Entry point mirroring the reference's train.py (class SceneGraphGAN + the same CLI flags), MI355X-native.

    python train.py --synthetic 64,224,1000 --max_iterations 20           # no Visual Genome files needed
    python train.py --checkpoints_dir ckpt --saliency_dir maps             # per-word saliency maps of the test split
    python train.py --checkpoints_dir ckpt --predict_dir graphs            # ranked scene graph of every test image
    python train.py --checkpoints_dir ckpt --predict_dir graphs --ground   # ... with subjects / objects resolved to entity instances
    python train.py --checkpoints_dir ckpt --metrics_out metrics.json      # R@K, mR@K, zsR@K of the test split
    python train.py --ema_decay 0.999 ...                                  # keep an average of G's weights; evaluation then uses it
    python train.py --batch_size 64 --accumulate 8 ...                     # every update from 8 micro-batches: the batch-512 update
    python train.py --clip_grad_norm 5,50 --skip_nonfinite ...             # clip D / G updates by global norm, drop non-finite ones
    python train.py --pretrain_iterations 2000 --mle_weight 0.1 --validate_nll ...  # maximum-likelihood warm start of G, held-out NLL
    python train.py --checkpoints_dir ckpt --likelihood_out nll.json       # NLL of the test split's true triples under G
    python train.py --generator_output gumbel --relax_tau 2,0.5,20000 ...  # the critic sees Gumbel-softmax rows, tau annealed
    python train.py --generator_output gumbel --relax_tau 1 --relax_hard ...  # straight-through: one-hot rows to the critic, soft gradient
    python train.py --generator_gradient score --entropy_weight 0.01 ...   # REINFORCE on sampled triples: no gradient through the critic
    python train.py --generator_gradient score --score_samples 4 ...       # ... with 4 sampled triples per image and a per-image baseline
    python train.py --path_to_ims_to_triples ... --path_to_vocab ... --path_to_word_embeddings ...

Reference: train.py:17-422.  Kept: constructor signature (:23-24), `_Generator` / `_Discriminator` wrappers with
shared weights (:85-93), the loss / optimiser definition (:239-266) and the loop body (:362-368: CRITIC_ITERS critic
updates then one generator update on the same minibatch, fresh noise / alpha per update).  The TensorFlow graph /
tfgan / tf.data machinery is replaced by sgg_amd.step.GanStep (hand-written HIP kernels behind libsgg_hip.so).
Deviations, all documented in SURVEY.md Appendix C: flags are passed by keyword (the reference swaps batch_size and
critic_iters, C-2); the checkpoint directory is not wiped when resuming and checkpoints are actually written (C-5);
evaluation uses the trained weights (C-4).  Multi-GPU: launch with torch.distributed.run, one process per GPU.
"""
import os, sys
sys.path.append(os.getcwd())

import argparse
import contextlib
import json
import math
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from architectures.generator_with_attention import Generator
from architectures.discriminator_with_attention import Discriminator

import sgg_amd  # noqa: F401
from sgg_amd import dp as dpmod
from sgg_amd import ground as groundmod
from sgg_amd import guard as guardmod
from sgg_amd import kbest as kbestmod
from sgg_amd import predcls as pclsmod
from sgg_amd import retrieve as retrmod
from sgg_amd.api import kernels_for
from sgg_amd.augment import AugmentSpec, flip_swap_table
from sgg_amd.data import PrefetchLoader, ShuffledStream, parse_image
from sgg_amd.diagnostics import raise_if_nonfinite
from sgg_amd.params import EMBED_DIM
from sgg_amd.metrics import MAX_GT, RecallAccumulator, zero_shot_mask
from sgg_amd.predict import DEFAULT_LOGITS_BUDGET_BYTES, images_per_pass, scene_graph
from sgg_amd.step import GanStep, need_kernels


class ValidationEarlyStop(object):
    """The convergence test of train.py:358-384: `last_loss = inf; convergence_count = 0`, then per validation
    `if last_loss < loss: count += 1 else: count = 0; if count == 3: break; last_loss = loss`."""

    def __init__(self, patience=3):
        self.patience, self.count, self.last = int(patience), 0, float("inf")

    def update(self, loss):
        """True = stop training now."""
        self.count = self.count + 1 if self.last < loss else 0
        if self.count == self.patience:
            return True
        self.last = loss
        return False


def micro_batch_ids(it, N):
    """The micro-batches of the example stream that iteration `it` consumes with --accumulate N: m = it * N + k, k = 0 .. N - 1.
    Micro-batch m is what iteration m of a run without accumulation reads (ShuffledStream.batch(m, B, rank, world)), so the update
    of iteration `it` covers stream elements [it * N * B * world, (it + 1) * N * B * world)."""
    return range(it * N, (it + 1) * N)


RELAX_MODES = GanStep.RELAX_MODES


def parse_relax_tau(spec):
    """--relax_tau: "T" or "T0,T1,N" (or a number, or three of them) -> (T0, T1, N), the temperature schedule
    tau(it) = T0 * (T1 / T0) ^ (min(it, N) / N); a constant T is (T, T, 0).  T0, T1 finite and > 0, N a whole number >= 0."""
    parts = [p for p in spec.split(",")] if isinstance(spec, str) else (list(spec) if isinstance(spec, (tuple, list)) else [spec])
    try:
        if len(parts) == 1:
            t0 = t1 = float(parts[0])
            n = 0
        elif len(parts) == 3:
            t0, t1, n = float(parts[0]), float(parts[1]), int(parts[2])
            if n != float(parts[2]):
                raise ValueError
        else:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("relax_tau takes T or T0,T1,N (got %r)" % (spec,))
    if not (np.isfinite(t0) and np.isfinite(t1) and t0 > 0.0 and t1 > 0.0 and n >= 0) or (n == 0 and t0 != t1):
        raise ValueError("relax_tau: temperatures must be finite and > 0, N >= 1 for a schedule (got %r)" % (spec,))
    return (t0, t1, n)


def relax_tau_at(spec, it):
    """tau(it) of the schedule (T0, T1, N), in double on the host."""
    t0, t1, n = spec
    if n == 0:
        return float(t0)
    return float(t0) * (float(t1) / float(t0)) ** (min(int(it), n) / float(n))


def relax_draw(it, update, micro, critic_iters, accumulate):
    """The 64-bit Gumbel draw number of one relaxation launch of training: a function of the iteration, the update within it (critic
    updates first, the generator update last) and the micro-batch - a stopped and resumed run repeats its draws with nothing saved."""
    return ((int(it) * (int(critic_iters) + 1) + int(update)) * int(accumulate) + int(micro)) & 0x7FFFFFFFFFFFFFFF


GRADIENTS = ("pathwise", "score")
SCORE_BASELINES = ("rloo", "none", "image")
SCORE_MAX_SAMPLES = 16


def check_score_flags(generator_gradient, score_baseline, entropy_weight, generator_output, relax_tau, score_samples=None):
    """The combinations of --generator_gradient / --score_baseline / --entropy_weight / --score_samples with each other and with the
    relaxation's flags that are refused (ValueError); returns (generator_gradient, score_baseline, entropy_weight, score_samples) as
    given (None: not given)."""
    if generator_gradient is not None and generator_gradient not in GRADIENTS:
        raise ValueError("generator_gradient must be one of %s (got %r)" % (", ".join(GRADIENTS), generator_gradient))
    if score_baseline is not None and score_baseline not in SCORE_BASELINES:
        raise ValueError("score_baseline must be one of %s (got %r)" % (", ".join(SCORE_BASELINES), score_baseline))
    if entropy_weight is not None:
        entropy_weight = float(entropy_weight)
        if not (0.0 <= entropy_weight < float("inf")):
            raise ValueError("entropy_weight must be a finite number >= 0 (got %r)" % entropy_weight)
    if score_samples is not None:
        if isinstance(score_samples, bool) or int(score_samples) != score_samples or not 1 <= int(score_samples) <= SCORE_MAX_SAMPLES:
            raise ValueError("score_samples must be an integer in 1..%d (got %r)" % (SCORE_MAX_SAMPLES, score_samples))
        score_samples = int(score_samples)
    if generator_gradient != "score":
        if score_baseline is not None or entropy_weight is not None:
            raise ValueError("score_baseline and entropy_weight belong to generator_gradient score")
        if score_samples is not None:
            raise ValueError("score_samples belongs to generator_gradient score")
    else:
        if score_baseline == "image" and (score_samples or 1) < 2:
            raise ValueError("score_baseline image compares the samples of one image: it needs score_samples >= 2")
        if generator_output in ("logits", "softmax"):
            raise ValueError("generator_gradient score implies generator_output gumbel with relax_hard: the critic must see samples of "
                             "softmax(logits) (got generator_output %s)" % generator_output)
        if relax_tau is not None:
            raise ValueError("relax_tau has no meaning with generator_gradient score: no temperature enters either update")
    return generator_gradient, score_baseline, entropy_weight, score_samples


def relax_val_draw(k):
    """... and of validation number k: the top bit set, so that no training launch shares it."""
    return (1 << 63) | (int(k) & 0x7FFFFFFFFFFFFFFF)


class SceneGraphGAN(object):

    ############################################################
    ## All init methods
    ############################################################
    def __init__(self, checkpoints_dir, summaries_dir, path_to_ims_to_triples, path_to_vocab, path_to_word_embeddings,
                 path_to_image_means, path_to_image_stds, critic_iters, batch_size, lambda_, resume,
                 synthetic=None, device=None, seed=0, two_streams=True, reuse_g_encoder=True, shuffle_buffer=True,
                 ema_decay=0.0, eval_live=False, accumulate=1, clip_grad_norm=0.0, skip_nonfinite=False,
                 pretrain_iterations=0, mle_weight=0.0, validate_nll=False, generator_output=None, relax_tau=None, relax_hard=False,
                 generator_gradient=None, score_baseline=None, entropy_weight=None, score_samples=None, augment=None):
        # Hyperparameters (train.py:26-32)
        self.CRITIC_ITERS = int(critic_iters)
        self.BATCH_SIZE = int(batch_size)
        self.VAL_BATCH_SIZE = self.BATCH_SIZE // 2
        self.TEST_BATCH_SIZE = self.BATCH_SIZE // 2
        self.TEST_BATCH_MULTIPLIER = 8
        self.LAMBDA = float(lambda_)
        self.resume = bool(resume)
        # two-stream schedule of step.GanStep (D's encoder beside G's forward, filter gradients beside the dgrad -> LayerNorm
        # chain): same kernels, bit-identical results (tests/test_concurrency_gpu.py), +4 % triples/s
        self.two_streams = bool(two_streams)
        self.reuse_g_encoder = bool(reuse_g_encoder)
        # ema_decay > 0: an exponential moving average of G's weights (tf.train.ExponentialMovingAverage with its warm-up schedule) is
        # updated inside every generator step (step.Network.enable_averaging).  Training, the validation loss and sample_triples use
        # the live weights; evaluation - test(), saliency(), predict(), evaluate() - runs G on the average whenever one exists
        # (enabled here or restored from the checkpoint) unless eval_live.  The critic is never averaged.
        self.ema_decay = float(ema_decay or 0.0)
        if self.ema_decay < 0.0 or self.ema_decay >= 1.0:
            raise ValueError("ema_decay must be 0 (off) or lie strictly between 0 and 1 (got %r)" % (ema_decay,))
        self.eval_live = bool(eval_live)
        self._in_eval = False
        # accumulate = N > 1: every optimiser step is taken from N micro-batches of BATCH_SIZE rows (GanStep.train_iteration_accumulated:
        # the mean of their gradients is the gradient of the N * BATCH_SIZE rows - every loss term is a mean over rows and no op couples
        # samples); iteration `it` consumes micro-batches it * N .. it * N + N - 1 of the example stream (micro_batch_ids)
        self.ACCUMULATE = int(accumulate)
        if self.ACCUMULATE < 1:
            raise ValueError("accumulate must be a positive number of micro-batches per update (got %r)" % (accumulate,))
        # clip_grad_norm = X or (critic's, generator's) or "X[,Y]", 0 = off: each network's update is scaled down to that global norm
        # where its gradient exceeds it; skip_nonfinite: an update whose gradient holds an Inf or NaN is dropped.  Both are decided on
        # the device inside the optimiser step (step.Network.enable_guard; the host learns of it through the record it logs)
        self.clip_norms = tuple(guardmod.check_settings(x)[0] for x in clip_grad_norm) if isinstance(clip_grad_norm, (tuple, list)) \
            else guardmod.parse_clip_grad_norm(clip_grad_norm)
        if len(self.clip_norms) != 2:
            raise ValueError("clip_grad_norm takes one number or (critic's, generator's) (got %r)" % (clip_grad_norm,))
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.skip_nonfinite or any(x > 0.0 for x in self.clip_norms)
        # pretrain_iterations = P > 0: iterations itr < P of the run are maximum-likelihood updates of G on the minibatch's true triples
        # (GanStep.pretrain_step, no critic update); the phase is a function of itr and P, so --resume needs no counter of its own.
        # mle_weight = w > 0: the same cross-entropy as an auxiliary term of the generator's cost in the GAN phase.  validate_nll:
        # validation also logs the held-out negative log-likelihood (GanStep.generator_nll).  All off by default: nothing is launched.
        self.PRETRAIN = int(pretrain_iterations or 0)
        if self.PRETRAIN < 0:
            raise ValueError("pretrain_iterations must be >= 0 (got %r)" % (pretrain_iterations,))
        self.mle_weight = float(mle_weight or 0.0)
        if not (0.0 <= self.mle_weight < float("inf")):
            raise ValueError("mle_weight must be a finite number >= 0 (got %r)" % (mle_weight,))
        self.validate_nll = bool(validate_nll)
        # generator_output = "softmax" | "gumbel": the critic sees y = softmax((logits [+ Gumbel noise]) / tau) instead of G's raw
        # decoder logits, and the generator's update differentiates through y (GanStep.set_relaxation); relax_tau = T or (T0, T1, N),
        # tau(it) = T0 (T1 / T0)^(min(it, N) / N).  None = not given: a fresh run is "logits" at tau 1 (nothing launched, nothing
        # written), a resumed run or an evaluation takes both from the checkpoint; a given value that contradicts the checkpoint is
        # an error (_loadModel).
        if generator_output is not None and generator_output not in RELAX_MODES:
            raise ValueError("generator_output must be one of %s (got %r)" % (", ".join(RELAX_MODES), generator_output))
        # generator_gradient = "score": the generator's update is the score-function (REINFORCE) estimator on the sampled triples
        # (GanStep.set_estimator) - it implies generator_output gumbel with relax_hard (the critic sees Gumbel-max samples of
        # softmax(logits) in both updates) and takes no temperature; score_baseline "rloo" (default) | "none", entropy_weight >= 0.
        # score_samples = S in 1..16 (default 1): S triples per image in the generator's update, score_baseline "image" (the default
        # for S > 1) = against the other samples of the same image; the dict carries "samples" only when S > 1.
        # None = not given: pathwise for a fresh run; a resumed run or an evaluation takes all four from the checkpoint.
        self._score_flags = check_score_flags(generator_gradient, score_baseline, entropy_weight, generator_output, relax_tau, score_samples)
        self.score = None
        if generator_gradient == "score":
            generator_output, relax_hard = "gumbel", True
            S = self._score_flags[3] or 1
            self.score = {"kind": "score", "baseline": score_baseline or ("image" if S > 1 else "rloo"),
                          "entropy_weight": float(entropy_weight or 0.0)}
            if S > 1:
                self.score["samples"] = S
        self._relax_flags = (generator_output, None if relax_tau is None else parse_relax_tau(relax_tau))
        self.relax_mode = generator_output or "logits"
        # relax_hard: the straight-through estimator on top of "softmax" or "gumbel" - the critic sees onehot(argmax(logits [+ noise])),
        # the generator's update takes the soft row's gradient.  False = not given: taken from the checkpoint like the mode.
        self.relax_hard = bool(relax_hard)
        if self.relax_hard and generator_output == "logits":
            raise ValueError("relax_hard needs generator_output softmax or gumbel (got logits)")
        self.relax_tau = self._relax_flags[1] or (1.0, 1.0, 0)
        # augment = "crop=0.5,flip=0.5,brightness=0.2,contrast=0.2,saturation=0.2" (sgg_amd/augment.py): random crop / mirror / colour
        # jitter of the TRAINING batches, drawn and applied inside the loader's input kernel (csrc/augment.hip); validation and every
        # evaluation mode read the plain pixels.  None = not given: off for a fresh run, the checkpoint's for a resumed one; a given
        # spec that contradicts the checkpoint is an error (_loadModel).
        self._augment_flag = None if augment is None else AugmentSpec.parse(augment)
        if self._augment_flag is not None and synthetic is not None:
            raise ValueError("augment works on decoded source pixels: synthetic batches have none (drop --augment or --synthetic)")
        self.augment = self._augment_flag
        self.shuffle_buffer = bool(shuffle_buffer)      # tf.data shuffle(buffer_size = 10 * batch) on the repeated stream (train.py:176-179)
        self.checkpoints_dir, self.summaries_dir = checkpoints_dir, summaries_dir
        self.rank, self.world, local = dpmod.init_from_env()
        self.device = torch.device(device if device is not None else "cuda:%d" % local)
        torch.cuda.set_device(self.device)
        if self.rank == 0:
            os.makedirs(checkpoints_dir, exist_ok=True)
            os.makedirs(summaries_dir, exist_ok=True)
        self.seed = seed
        if synthetic is not None:
            B, S, V = synthetic
            self.BATCH_SIZE, self.image_size = B, S
            self.vocab = {"w%d" % i: i for i in range(V)}
            g = torch.Generator().manual_seed(3)
            self.embeddings = (torch.rand((V, EMBED_DIM), generator=g) * 0.2 - 0.1).numpy()   # map_files_to_triples.py:24
            self.dataset = None
        else:
            self.image_size = 221                                           # train.py:171
            with open(path_to_ims_to_triples, "r") as f:
                self.ims_to_triples = json.load(f)
            with open(path_to_vocab, "r") as f:
                self.vocab = json.load(f)
            self.embeddings = np.load(path_to_word_embeddings)
            self._loadImageMeans(path_to_image_means, path_to_image_stds)
            self.dataset = self._gatherFiles()
        self._createStringMappings()
        self.g = Generator(len(self.vocab))
        self.d = Discriminator(len(self.vocab), torch.as_tensor(self.embeddings, dtype=torch.float32))
        self.step = None
        self.val_step = None
        self.itr = 0

    def _createStringMappings(self):
        self.reverse_vocab = {y: x for x, y in self.vocab.items()}                          # train.py:76-80

    def _loadImageMeans(self, path_means, path_stds):
        with open(path_means) as f:
            self.image_means = torch.tensor([float(l.strip()) for l in f if l.strip()])
        with open(path_stds) as f:
            self.image_stds = torch.tensor([float(l.strip()) for l in f if l.strip()])

    def _Generator(self, images, is_training=True):
        return self.g.build_generator(images, is_training)

    def _Discriminator(self, triple_input, images, is_training=True):
        return self.d.build_discriminator(triple_input, images, is_training)

    ############################################################
    ## Data (train.py:114-226); synthetic mode needs no files
    ############################################################
    def _gatherFiles(self):
        keys = list(self.ims_to_triples.keys())
        train_keys = keys[:int(0.9 * len(keys))]
        self.test_items = [(k, self.ims_to_triples[k]) for k in keys[int(0.9 * len(keys)):] if len(self.ims_to_triples[k])]
        files, labels = [], []
        for k in train_keys:
            for t in self.ims_to_triples[k]:
                files.append(k)
                labels.append(t)
        perm = np.random.RandomState(self.seed).permutation(len(files))
        files, labels = [files[i] for i in perm], np.asarray(labels, dtype=np.int64)[perm]
        thr = int(0.88 * len(files))
        self.max_iterations = 5 * thr                                       # train.py:159
        self.write_iterations = 10                                          # train.py:161
        self.validate_iterations = max(1, int(thr / 50))                    # train.py:162
        return {"train": (files[:thr], labels[:thr]), "val": (files[thr:], labels[thr:])}

    def _streams(self):
        """The example order of the reference's datasets (train.py:176-179): the shuffled list repeated for ever, through a rolling
        shuffle buffer of 10 batches (sgg_amd.data.ShuffledStream).  One stream per consumer (the prefetching loader's producer
        thread, the synchronous path, validation): same seed -> same order."""
        if getattr(self, "_stream_cache", None) is None:
            B, VB = self.BATCH_SIZE, self._val_rows()
            n_tr = len(self.dataset["train"][0]) if self.dataset is not None else 0
            n_va = len(self.dataset["val"][0]) if self.dataset is not None else 0
            mk = lambda n, b, salt: ShuffledStream(n, 10 * b * self.world, seed=self.seed + salt) if (n and self.shuffle_buffer) else None
            self._stream_cache = {"loader": mk(n_tr, B, 11), "sync": mk(n_tr, B, 11), "val": mk(n_va, VB, 12)}
        return self._stream_cache

    def _val_rows(self):
        """VAL_BATCH_SIZE = BATCH_SIZE / 2 (train.py:30, Python-2 integer division); the model objects take any batch size on one
        set of weights (sgg_amd/api.py), so the validation batch runs at its own size, as in the reference graph."""
        return max(1, self.BATCH_SIZE // 2)

    def _parseFunction(self, filename):
        """JPEG decode -> tf.image.resize_images([221, 221]) (TF-1.x bilinear, align_corners=False, no antialiasing) ->
        (x - mean) / std (train.py:167-172), on the host: sgg_amd/data.py."""
        return torch.from_numpy(parse_image(filename, self.image_means.numpy(), self.image_stds.numpy()))

    def _batch_indices(self, it, stream="sync"):
        """Example indices of iteration `it` on this rank (rank r takes rows [r*B, (r+1)*B) of the global batch): batch `it` of the
        repeated + buffer-shuffled stream (train.py:176-179), or of the plain cyclic walk with shuffle_buffer=False."""
        B, n = self.BATCH_SIZE, len(self.dataset["train"][0])
        st = self._streams()[stream]
        if st is not None:
            return st.batch(it, B, self.rank, self.world)
        return [(it * B * self.world + self.rank * B + j) % n for j in range(B)]

    def _next_batch(self, it):
        B = self.BATCH_SIZE
        if self.dataset is None:
            g = torch.Generator().manual_seed(self.seed + 17 * it + 1000 * self.rank)
            images = torch.randn((B, self.image_size, self.image_size, 3), generator=g)
            labels = torch.randint(0, len(self.vocab), (B, 3), generator=g, dtype=torch.int64)
        else:
            files, labs = self.dataset["train"]
            idx = self._batch_indices(it)
            images = torch.stack([self._parseFunction(files[i]) for i in idx])
            labels = torch.from_numpy(labs[idx])
        return images.to(self.device), labels.to(self.device)

    def _val_batch(self, k):
        """Validation batch k (the live validation iterator of train.py:199-203): VAL_BATCH_SIZE examples of the validation split in
        its own repeated + shuffled order."""
        VB = self._val_rows()
        if self.dataset is None:
            g = torch.Generator().manual_seed(self.seed + 5000 + 17 * k + 1000 * self.rank)
            images = torch.randn((VB, self.image_size, self.image_size, 3), generator=g)
            labels = torch.randint(0, len(self.vocab), (VB, 3), generator=g, dtype=torch.int64)
        else:
            files, labs = self.dataset["val"]
            st = self._streams()["val"]
            idx = st.batch(k, VB, self.rank, self.world) if st is not None else \
                [(k * VB * self.world + self.rank * VB + j) % len(files) for j in range(VB)]
            images = torch.stack([self._parseFunction(files[i]) for i in idx])
            labels = torch.from_numpy(labs[idx])
        return images.to(self.device), labels.to(self.device)

    def validation_loss(self, k, gen):
        """np.mean(sess.run(self.disc_cost, feed_dict = {handle: val_handle})) (train.py:377): the critic's cost on validation batch k with
        fresh noise / alpha, no update; averaged over the data-parallel ranks so that every rank takes the same early-stop decision."""
        images, labels = self._val_batch(k)
        VB = self._val_rows()
        noise = torch.randn((VB, 512), generator=gen).to(self.device)
        alpha = torch.rand((VB,), generator=gen).to(self.device)
        self._ensure_val_step(images)
        self.step.flush()           # (a deferred optimiser step of the training networks changes the weights validation reads)
        relax = {}
        if self.relaxed:            # the training relaxation at the temperature of the iteration just run, draws keyed on k
            self._set_relaxation(self.val_step, max(self.itr - 1, 0))
            relax = {"draw": relax_val_draw(k)}
        loss = self.val_step.critic_loss(images, labels, noise, alpha, **relax)[0:1].clone()
        if self.world > 1:
            torch.distributed.all_reduce(loss)
            loss /= self.world
        return float(loss.item())

    # ---- relaxed generator output (GanStep.set_relaxation, csrc/relax.hip) ------------------------------------
    relaxed = property(lambda self: self.relax_mode != "logits")

    def _relax_seed(self):
        """The 64-bit key of the Gumbel noise: --seed in the high word, the rank in the low one."""
        return ((int(self.seed) & 0xFFFFFFFF) << 32) | (int(self.rank) & 0xFFFFFFFF)

    def _set_relaxation(self, step, it):
        """Put `step` into the run's mode at the temperature of iteration `it`; returns that temperature."""
        tau = relax_tau_at(self.relax_tau, it)
        step.set_relaxation(self.relax_mode, tau, self._relax_seed(), hard=self.relax_hard)
        return tau

    def _eval_relax(self):
        """What the critic is shown at evaluation: None (logits) or the temperature of softmax(logits / tau) at the checkpoint's
        iteration - in both modes without Gumbel noise (the samples' diversity comes from the noise vector)."""
        return relax_tau_at(self.relax_tau, self.itr) if self.relaxed else None

    def _eval_relax_kw(self):
        """score_samples' keywords at evaluation: nothing (logits), the temperature, or - a straight-through run - the hard option:
        the critic scores onehot(argmax(logits)), the row of the token that is reported."""
        if not self.relaxed:
            return {}
        return dict({"relax_tau": self._eval_relax()}, **({"relax_hard": True} if self.relax_hard else {}))

    def _hard_key(self):
        """{"hard": True} for a straight-through run, else nothing: a soft run's checkpoint, logs and labels keep their keys."""
        return {"hard": True} if self.relax_hard else {}

    def _relax_label(self):
        """The "generator_output" entry of an evaluation's JSON output."""
        return dict({"mode": self.relax_mode, "tau": relax_tau_at(self.relax_tau, self.itr)}, **self._hard_key(),
                    **({"gradient": "score"} if self.score else {}),
                    **({"samples": self.score["samples"]} if self.score and self.score.get("samples", 1) > 1 else {}))

    def _ensure_val_step(self, images):
        if self.val_step is None:
            # the same variables at the validation batch size (train.py:199-203 feeds the validation iterator through the same graph)
            self.val_step = GanStep(kernels_for(self.device), len(self.vocab), self.image_size, self._val_rows(), lam=self.LAMBDA,
                                    G=self.g._ensure(images), D=self.d._ensure(images))

    def validation_nll(self, k, gen):
        """The held-out negative log-likelihood of validation batch k's true tokens under the generator (GanStep.generator_nll, no
        update): {"val_nll_token" (nats per token), "val_token_acc", "val_triple_acc"}, averaged over the data-parallel ranks as
        validation_loss is.  `gen` is a noise generator of its own, so that validation_loss draws what it draws without this."""
        images, labels = self._val_batch(k)
        noise = torch.randn((self._val_rows(), 512), generator=gen).to(self.device)
        self._ensure_val_step(images)
        self.step.flush()
        out = self.val_step.generator_nll(images, labels, noise)[0:3].clone()
        if self.world > 1:
            torch.distributed.all_reduce(out)
            out /= self.world
        v = out.cpu().tolist()
        return {"val_nll_token": v[0], "val_token_acc": v[1], "val_triple_acc": v[2]}

    def _prefetcher(self, start, stop, workers=16):
        """tf.contrib.data.map_and_batch + prefetch (train.py:181-187) as decode threads + a pinned double buffer whose
        host-to-device copy runs on its own stream while the previous batch trains.  start / stop count (micro-)batches."""
        files, labs = self.dataset["train"]
        return PrefetchLoader(files, labs, self.BATCH_SIZE, lambda it: self._batch_indices(it, "loader"), self.image_means.numpy(),
                              self.image_stds.numpy(), self.device, stop, start=start, workers=workers, processes=workers > 2,
                              **self._augment_kw())

    def _augment_kw(self):
        """The loader's augmentation arguments - nothing for a run without --augment.  The key is --seed alone: every data-parallel
        layout of a global batch draws the same parameters for the same stream position."""
        if self.augment is None:
            return {}
        return {"augment": self.augment, "seed": self.seed, "rank": self.rank, "world": self.world, "swap": flip_swap_table(self.vocab)}

    ############################################################
    ## Saving
    ############################################################
    def _ckpt_path(self):
        return os.path.join(self.checkpoints_dir, "model.ckpt.pt")

    def _saveModel(self):
        self.step.flush()
        if self.rank == 0:
            stopper = getattr(self, "_stopper", None)
            ck = {"itr": self.itr, "G": self.g.state_dict(), "D": self.d.state_dict(),
                  "G_adam": (self.step.G.m_flat.cpu(), self.step.G.v_flat.cpu(), self.step.G.adam_t),
                  "D_adam": (self.step.D.m_flat.cpu(), self.step.D.v_flat.cpu(), self.step.D.adam_t),
                  # the validation state of the loop (train.py:358-384): last loss, consecutive increases, batches consumed
                  "val": {"last": stopper.last if stopper else float("inf"), "count": stopper.count if stopper else 0,
                          "history": list(getattr(self, "val_history", []))}}
            if self.ACCUMULATE > 1:         # (only a run that accumulates writes the key)
                ck["accumulate"] = self.ACCUMULATE
            if self.PRETRAIN > 0:           # (only a run with a pretraining phase writes the key)
                ck["pretrain_iterations"] = self.PRETRAIN
            if self.relaxed:                # (only a run with a relaxed generator output writes the key)
                ck["generator_output"] = dict({"mode": self.relax_mode, "tau": list(self.relax_tau)}, **self._hard_key())
                if self.score:              # (only a run with the score-function update writes the key)
                    ck["generator_output"]["gradient"] = dict(self.score)
            if self.augment is not None:    # (only a run that augments writes the key)
                ck["augment"] = self.augment.as_dict()
            if self.step.D.has_guard or self.step.G.has_guard:      # (only a guarded run writes the key: the clipped / skipped counts)
                ck["guard"] = {n: net.guard_state() for n, net in (("D", self.step.D), ("G", self.step.G)) if net.has_guard}
            if self.step.G.has_average:     # (only a run that averages writes these keys: without it the checkpoint is what it was)
                ck["G_ema"] = self.step.G.average_state()
            # ... and where the noise stream stands, so that a resumed run continues the stream: its average is the one of the
            # uninterrupted run, and a run with a pretraining phase, stopped and resumed, ends on the same weights (single process
            # only: every rank draws from a stream of its own, rank 0 writes)
            gen = getattr(self, "_noise_gen", None)
            if (self.step.G.has_average or self.PRETRAIN > 0 or self.relaxed) and gen is not None and self.world == 1:
                ck["noise_rng"] = gen.get_state()
            torch.save(ck, self._ckpt_path())

    def _loadModel(self, for_training=False):
        ck = torch.load(self._ckpt_path(), map_location="cpu")
        # the generator output the run was trained with is the checkpoint's: a flag that says otherwise is an error, before anything is loaded
        saved_relax = ck.get("generator_output") or {"mode": "logits", "tau": [1.0, 1.0, 0]}
        saved_mode, saved_tau = saved_relax["mode"], (float(saved_relax["tau"][0]), float(saved_relax["tau"][1]), int(saved_relax["tau"][2]))
        flag_mode, flag_tau = self._relax_flags
        saved_score = saved_relax.get("gradient")
        flag_kind, flag_base, flag_ent, flag_samples = self._score_flags
        if flag_kind is not None and flag_kind != (saved_score or {"kind": "pathwise"})["kind"]:
            raise ValueError("--generator_gradient %s contradicts the checkpoint, which was trained with the %s update"
                             % (flag_kind, (saved_score or {"kind": "pathwise"})["kind"]))
        if saved_score and flag_base is not None and flag_base != saved_score["baseline"]:
            raise ValueError("--score_baseline %s contradicts the checkpoint's %s" % (flag_base, saved_score["baseline"]))
        if saved_score and flag_ent is not None and float(flag_ent) != float(saved_score["entropy_weight"]):
            raise ValueError("--entropy_weight %g contradicts the checkpoint's %g" % (flag_ent, saved_score["entropy_weight"]))
        if saved_score and flag_samples is not None and flag_samples != int(saved_score.get("samples", 1)):
            raise ValueError("--score_samples %d contradicts the checkpoint's %d" % (flag_samples, int(saved_score.get("samples", 1))))
        if flag_mode is not None and flag_mode != saved_mode:
            raise ValueError("--generator_output %s contradicts the checkpoint, which was trained with %s" % (flag_mode, saved_mode))
        if flag_tau is not None and saved_mode != "logits" and flag_tau != saved_tau:
            raise ValueError("--relax_tau %s contradicts the checkpoint's %s" % (",".join(str(x) for x in flag_tau),
                                                                                 ",".join(str(x) for x in saved_tau)))
        if self.relax_hard and not saved_relax.get("hard"):
            raise ValueError("--relax_hard contradicts the checkpoint, which was trained %s"
                             % ("on the raw logits" if saved_mode == "logits" else "with soft %s rows" % saved_mode))
        saved_augment = AugmentSpec.parse(ck["augment"]) if ck.get("augment") else None
        if self._augment_flag is not None and self._augment_flag != saved_augment:
            raise ValueError("--augment %s contradicts the checkpoint, which was trained %s"
                             % (self._augment_flag, "with %s" % saved_augment if saved_augment is not None else "without augmentation"))
        self.augment = saved_augment
        self.relax_mode, self.relax_tau, self.relax_hard = saved_mode, saved_tau, bool(saved_relax.get("hard"))
        self.score = dict(saved_score) if saved_score else None
        self.g.load_state_dict(ck["G"])
        self.d.load_state_dict(ck["D"])
        for net, key in ((self.step.G, "G_adam"), (self.step.D, "D_adam")):
            net.m_flat.copy_(ck[key][0]); net.v_flat.copy_(ck[key][1]); net.adam_t = ck[key][2]
        saved, G = ck.get("G_ema"), self.step.G
        if self.ema_decay > 0.0:            # (_constructOps enabled averaging with the decay of this run: it wins over the saved one)
            if saved is not None:
                G.restore_average(saved["flat"], saved["updates"])
            else:
                G.reset_average()           # the average starts from the loaded weights
        elif saved is not None:
            if for_training:
                if self.rank == 0:
                    print("resuming without --ema_decay: the checkpoint's average of the generator weights is dropped")
            else:                           # evaluation-only modes use the checkpoint's average without the flag
                G.enable_averaging(saved["decay"])
                G.restore_average(saved["flat"], saved["updates"])
        saved_guard = ck.get("guard")
        if saved_guard is not None and for_training:
            kept = [n for n, net in (("D", self.step.D), ("G", self.step.G)) if net.has_guard and n in saved_guard]
            for n in kept:
                getattr(self.step, n).restore_guard(saved_guard[n]["clipped"], saved_guard[n]["skipped"])
            if len(kept) < len(saved_guard) and self.rank == 0:
                print("resuming without --clip_grad_norm / --skip_nonfinite for %s: the checkpoint's clipped / skipped counts are dropped"
                      % ", ".join(n for n in saved_guard if n not in kept))
        self.itr = ck["itr"]
        if for_training and int(ck.get("accumulate", 1)) != self.ACCUMULATE and self.rank == 0:
            print("resuming with --accumulate %d a run saved with %d: the data stream continues at micro-batch itr * %d = %d"
                  % (self.ACCUMULATE, int(ck.get("accumulate", 1)), self.ACCUMULATE, self.itr * self.ACCUMULATE))
        if for_training and int(ck.get("pretrain_iterations", 0)) != self.PRETRAIN and self.rank == 0:
            print("resuming with --pretrain_iterations %d a run saved with %d: iterations below %d are pretraining iterations from "
                  "here on (the run stands at iteration %d)" % (self.PRETRAIN, int(ck.get("pretrain_iterations", 0)), self.PRETRAIN, self.itr))
        self._resumed_val = ck.get("val")
        self._resumed_rng = ck.get("noise_rng") if (for_training and (self.ema_decay > 0.0 or self.PRETRAIN > 0 or self.relaxed)
                                                    and self.world == 1) else None

    @property
    def evaluates_average(self):
        """True if evaluation runs G on the average of its weights (one exists and eval_live is off)."""
        return (not self.eval_live) and self.step is not None and self.step.G.has_average

    @contextlib.contextmanager
    def _eval_weights(self):
        """The weights evaluation runs on: inside, G's arena holds the average where evaluates_average (Network.averaged: exchanged
        on entry, exchanged back on exit), else nothing changes.  Yields "ema" or "live".  Re-entrant (write_saliency -> saliency)."""
        if self.step is None:               # (an untrained model: the networks are built here, as the evaluation entry points do)
            images, _ = self._next_batch(0)
            self._constructOps(images)
        if self._in_eval or not self.evaluates_average:
            yield "ema" if self._in_eval else "live"
            return
        self.step.flush()
        self._in_eval = True
        try:
            with self.g.averaged():
                yield "ema"
        finally:
            self._in_eval = False

    ############################################################
    ## Training (train.py:341-388)
    ############################################################
    def _constructOps(self, images):
        """Build both networks for this static shape and wire the WGAN-GP step (train.py:231-266)."""
        B, S, V = images.shape[0], images.shape[1], len(self.vocab)
        g_net, d_net = self.g._ensure(images), self.d._ensure(images)
        reducer = dpmod.GradReducer() if self.world > 1 else None
        self.step = GanStep(kernels_for(self.device), V, S, B, lam=self.LAMBDA, G=g_net, D=d_net, reducer=reducer,
                            overlap_streams=self.two_streams)
        if self.ema_decay > 0.0:            # G only: the critic keeps its live weights everywhere
            self.step.G.enable_averaging(self.ema_decay)
        if self.guarded:                    # (never called otherwise: an unguarded run launches what it always did)
            self.step.set_guard(self.clip_norms, self.skip_nonfinite)

    def _accumulated_iteration(self, batches, gen):
        """One iteration with every update taken from the N = len(batches) micro-batches: noise and alpha are drawn from `gen` in
        the order (update, micro-batch) - with N = 1 the stream of the plain loop - and each update runs all micro-batches before
        its one optimiser step (GanStep.train_iteration_accumulated)."""
        B, C, N = self.BATCH_SIZE, self.CRITIC_ITERS, len(batches)
        noises, alphas = [], []
        for i in range(C + 1):
            noises.append([])
            alphas.append([])
            for _ in range(N):
                noises[i].append(torch.randn((B, 512), generator=gen).to(self.device))
                if i < C:
                    alphas[i].append(torch.rand((B,), generator=gen).to(self.device))
        mle = {"mle_weight": self.mle_weight} if self.mle_weight > 0.0 else {}
        if self.relax_mode == "gumbel":
            mle["draws"] = [[relax_draw(self.itr, i, k, C, N) for k in range(N)] for i in range(C + 1)]
        self.step.train_iteration_accumulated(batches, noises, alphas[:C], critic_iters=C, reuse_g_encoder=self.reuse_g_encoder, **mle)

    def load_checkpoint(self):
        """Build both networks and load the checkpoint in checkpoints_dir (weights, Adam state, iteration) as --resume does;
        False if there is none."""
        if not os.path.exists(self._ckpt_path()):
            return False
        if self.step is None:
            images, _ = self._next_batch(0)
            self._constructOps(images)
        self._loadModel()
        return True

    def train(self, max_iterations=None, log_every=10, save_every=0, validate_every=None, test_at_end=None, patience=3,
              test_max_images=None, diagnostics_every=0, halt_on_nonfinite=False):
        """train.py:341-388.  Every `validate_every` iterations (default: the reference's len(train) / 50 on real data, off in
        synthetic mode) the critic's cost on a validation batch is compared with the previous one: `patience` (3) consecutive
        increases end the training (train.py:375-384); afterwards the model is evaluated (`print "Testing"; self.test(sess)`,
        train.py:387-388) - by default on real data only.

        diagnostics_every = N > 0: iterations N, 2N, ... run with the statistics pass armed for their whole length
        (GanStep.arm_diagnostics: per-tensor gradient / parameter / update norms and non-finite counts behind every optimiser step,
        read-only); their summary goes into losses.jsonl under "diag" (into that iteration's record, or one of its own) and the
        per-tensor table into summaries_dir/diagnostics.jsonl (rank 0).  halt_on_nonfinite: such an iteration that counts an Inf or
        NaN raises diagnostics.NonFiniteError before anything else happens - no checkpoint is written on the way out (neither
        save_every's nor the final one), so the last good checkpoint survives."""
        images, labels = self._next_batch(0)
        self._constructOps(images)
        if self.resume and os.path.exists(self._ckpt_path()):
            self._loadModel(for_training=True)
        if self.relax_hard and not self.relaxed:
            raise ValueError("relax_hard needs generator_output softmax or gumbel (a fresh run's default is logits)")
        n_it = max_iterations if max_iterations is not None else getattr(self, "max_iterations", 1000)
        if validate_every is None:
            validate_every = getattr(self, "validate_iterations", 0) if self.dataset is not None else 0
        if test_at_end is None:
            test_at_end = self.dataset is not None
        gen = self._noise_gen = torch.Generator().manual_seed(self.seed + 7 + self.rank)
        if getattr(self, "_resumed_rng", None) is not None:
            gen.set_state(self._resumed_rng)
            self._resumed_rng = None
        vgen = torch.Generator().manual_seed(self.seed + 70007 + self.rank)
        ngen = None                 # noise of the held-out likelihood (validation_nll): seed + 90009 + rank, made at its first use
        log = open(os.path.join(self.summaries_dir, "losses.jsonl"), "a") if self.rank == 0 else None
        if log is not None and self.augment is not None:        # once per run (a resumed run writes it again, with its start)
            log.write(json.dumps({"itr": self.itr, "augment": self.augment.as_dict()}) + "\n"); log.flush()
        B, t0, itr0, N = self.BATCH_SIZE, time.time(), self.itr, self.ACCUMULATE
        loader = self._prefetcher(self.itr * N, n_it * N) if self.dataset is not None else None
        stopper, self.stopped_early, self.val_history = ValidationEarlyStop(patience), False, []
        rv = getattr(self, "_resumed_val", None)
        if rv is not None:          # a resumed run carries on with the validation iterator and the early-stop counters where it stopped
            stopper.last, stopper.count, self.val_history = rv["last"], rv["count"], [tuple(x) for x in rv["history"]]
            self._resumed_val = None
        self._stopper = stopper
        diagnostics_every = int(diagnostics_every or 0)
        diag_log = open(os.path.join(self.summaries_dir, "diagnostics.jsonl"), "a") if (self.rank == 0 and diagnostics_every > 0) else None
        try:
            while self.itr < n_it:
                if N == 1:
                    images, labels = next(loader) if loader is not None else self._next_batch(self.itr)
                else:                       # all N micro-batches stay on the device for the whole iteration: every update reads all of them
                    batches = [next(loader) if loader is not None else self._next_batch(m) for m in micro_batch_ids(self.itr, N)]
                report = diagnostics_every > 0 and (self.itr + 1) % diagnostics_every == 0
                if diagnostics_every > 0:
                    self.step.arm_diagnostics(report)
                # every update of an iteration sees the same minibatch (train.py:175-190) and G's weights change only at its end: G's
                # encoder runs once per iteration (exact; 10 of 11 encoder forwards of G saved at CRITIC_ITERS = 10)
                pre = self.itr < self.PRETRAIN          # a pretraining iteration: one maximum-likelihood update of G, no critic update
                C = self.CRITIC_ITERS
                # relaxed generator output: this iteration's temperature, and per launch a draw number made of (itr, update, micro-batch)
                tau = self._set_relaxation(self.step, self.itr) if (self.relaxed and not pre) else None
                if self.score and not pre:  # (behind the relaxation it needs; a pathwise run never calls it)
                    self.step.set_estimator("score", self.score["baseline"], self.score["entropy_weight"],
                                            **({"samples": self.score["samples"]} if self.score.get("samples", 1) > 1 else {}))
                draw = (lambda i: {"draw": relax_draw(self.itr, i, 0, C, 1)}) if self.relax_mode == "gumbel" else (lambda i: {})
                if pre:
                    for k, (im, lb) in enumerate(batches if N > 1 else [(images, labels)]):
                        noise = torch.randn((B, 512), generator=gen).to(self.device)    # one fresh draw per micro-batch
                        self.step.pretrain_step(im, lb, noise, micro=(k, N) if N > 1 else None)
                elif N > 1:
                    self._accumulated_iteration(batches, gen)
                else:
                    with self.step.iteration(reuse_g_encoder=self.reuse_g_encoder):
                        for i in range(C):                                              # train.py:364-365
                            noise = torch.randn((B, 512), generator=gen).to(self.device)
                            alpha = torch.rand((B,), generator=gen).to(self.device)
                            self.step.critic_step(images, labels, noise, alpha, **draw(i))
                        noise = torch.randn((B, 512), generator=gen).to(self.device)
                        if self.mle_weight > 0.0:
                            self.step.generator_step(images, noise, labels=labels, mle_weight=self.mle_weight, **draw(C))
                        else:
                            self.step.generator_step(images, noise, **draw(C))          # train.py:368
                itr = self.itr                                                          # the reference's 0-based loop variable
                self.itr += 1
                diag = self.step.diagnostics(generator_only=pre) if report else None
                tensors = diag.pop("tensors") if diag is not None else None
                if diag is not None and N > 1 and not pre:
                    diag["gp_slope_rows"] = B       # the slopes are those of the last micro-batch of the last critic update
                if log is not None and self.itr % log_every == 0:
                    rate = B * N * self.world * (self.itr - itr0) / (time.time() - t0)  # of this run (a resumed run starts at itr0 > 0)
                    if pre or self.mle_weight > 0.0:
                        m = self.step.mle_losses_mean.cpu().tolist()
                        mle = {"mle_nll_token": m[0], "mle_nll_triple": 3.0 * m[0], "mle_token_acc": m[1], "mle_triple_acc": m[2]}
                    if pre:
                        rec = dict({"itr": self.itr, "phase": "pretrain"}, **mle)
                        rec["triples_per_s"] = rate
                    else:
                        d, g = self.step.d_losses_mean.cpu().tolist(), self.step.g_losses_mean.cpu().tolist()   # (N = 1: d_losses / g_losses)
                        rec = {"itr": self.itr, "disc_loss": d[0], "gen_loss": -g[3], "gp": d[2], "triples_per_s": rate}
                        if self.mle_weight > 0.0:
                            rec.update(mle)
                        if tau is not None:
                            rec["relax"] = dict({"mode": self.relax_mode, "tau": tau}, **self._hard_key())
                        if self.score:
                            sc = self.step.score_losses_mean.cpu().tolist()
                            rec["score"] = {"reward": sc[0], "adv_rms": math.sqrt(max(sc[1], 0.0)), "logp_token": sc[2], "entropy_token": sc[3],
                                            "baseline": self.score["baseline"], "entropy_weight": self.score["entropy_weight"]}
                            if self.score.get("samples", 1) > 1:        # (only a run with several samples per image writes the key)
                                rec["score"]["samples"] = self.score["samples"]
                    if N > 1:
                        rec["accumulate"] = N
                    if self.guarded:        # the records of each network's last update and the clipped / skipped counts so far
                        rec["guard"] = self.step.guard_reports()
                    if diag is not None:
                        rec["diag"] = diag
                    log.write(json.dumps(rec) + "\n"); log.flush()
                    print(rec)
                elif log is not None and diag is not None:
                    log.write(json.dumps({"itr": self.itr, "diag": diag}) + "\n"); log.flush()
                if diag_log is not None and tensors is not None:
                    diag_log.write(json.dumps({"itr": self.itr, "tensors": tensors}) + "\n"); diag_log.flush()
                if diag is not None and halt_on_nonfinite:
                    # every rank sees the same network rows (the gradients are all-reduced), so every rank raises here; the exception
                    # passes the checkpoint writes below and the final one behind the loop
                    raise_if_nonfinite(diag, self.itr)
                if save_every and self.itr % save_every == 0:
                    self._saveModel()
                if validate_every and itr % validate_every == 0 and pre:
                    # pretraining phase: the held-out likelihood only - the critic is untrained, its cost says nothing yet, and the
                    # early stop's counters and validation iterator wait for the GAN phase (batch: the validation's ordinal)
                    if ngen is None:
                        ngen = torch.Generator().manual_seed(self.seed + 90009 + self.rank)
                    nll = self.validation_nll(itr // validate_every, ngen)
                    if log is not None:
                        log.write(json.dumps(dict({"itr": self.itr}, **nll)) + "\n"); log.flush()
                elif validate_every and itr % validate_every == 0:                      # train.py:375-384
                    if self.validate_nll:       # on the batch validation_loss is about to read, noise from a generator of its own
                        if ngen is None:
                            ngen = torch.Generator().manual_seed(self.seed + 90009 + self.rank)
                        nll = self.validation_nll(len(self.val_history), ngen)
                        if log is not None:
                            log.write(json.dumps(dict({"itr": self.itr}, **nll)) + "\n"); log.flush()
                    loss = self.validation_loss(len(self.val_history), vgen)
                    self.val_history.append((itr, loss))
                    if log is not None:
                        log.write(json.dumps({"itr": self.itr, "val_disc_loss": loss}) + "\n"); log.flush()
                    if stopper.update(loss):
                        self.stopped_early = True
                        break
        finally:
            if loader is not None:
                loader.close()
            if diag_log is not None:
                diag_log.close()
        self._saveModel()
        if test_at_end:
            print("Testing")                                                            # train.py:387-388
            return self.test(max_images=test_max_images)

    ############################################################
    ## Testing (train.py:294-335)
    ############################################################
    def _recall(self, fake, real, N):
        return float(len(set(map(tuple, fake)).intersection(set(map(tuple, real))))) / N

    @staticmethod
    def _rank(scores, reference_literal=False):
        """Order of the sampled triples for R@k (train.py:321-323).  Intended semantics (default): ascending mean critic
        score over the three steps.  reference_literal=True reproduces what the reference's code does: its score array has
        shape [N, 1] (np.mean(disc_scores, axis=1) of [B, 3, 1], train.py:315), so `argsort()` sorts the length-1 last axis
        and returns zeros - every "top-k" entry is sample 0 (reference quirk C-11)."""
        scores = np.asarray(scores, dtype=np.float64).reshape(-1)
        if reference_literal:
            return np.zeros(len(scores), dtype=np.int64)
        return np.argsort(scores, kind="stable")

    def recalls(self, fake, scores, real, reference_literal=False):
        """(R@50, R@100) of one image: fake [N,3] sampled token triples, scores [N] mean critic outputs, real [M,3] true
        triples.  Set semantics of train.py:294-295: duplicates collapse, the denominators are the constants 50 and 100."""
        order = self._rank(scores, reference_literal)
        fake, real = np.asarray(fake), np.asarray(real, dtype=np.int64).reshape(-1, 3)
        return self._recall(fake[order[:50]], real, 50.0), self._recall(fake[order[:100]], real, 100.0)

    def test(self, max_images=None, out_path="recalls.txt", reference_literal=False, items=None, return_details=False):
        """R@50 / R@100 (train.py:297-335): per test image TEST_BATCH_MULTIPLIER x TEST_BATCH_SIZE generator samples, each scored by
        the mean critic output over the three steps (`np.mean(disc_scores, axis=1)`, :315), ordered by score, the first 50 / 100
        compared as sets with the image's true triples (:294-295, :325-326), averaged over the images, written to recalls.txt.

        ORDERING.  Default (reference_literal=False): ascending mean critic score - what `score_accumulator.argsort()` (:321) is
        written to mean.  This is NOT what the reference's code computes: its score array has shape [N, 1], so argsort sorts the
        length-1 axis and every selected index is 0 (sample 0 repeated).  reference_literal=True reproduces
        that literally.  The mode in force is written into recalls.txt (third line) and returned with the details.
        Uses the trained weights (the reference's test ops use an untrained copy).
        items: optional list of (image [S,S,3] float tensor, true triples [[s,p,o], ...]) replacing the test split.
        return_details: also return, per image, the sampled tokens [N,3], their scores [N] and the two recalls.

        Schedule: TEST_BATCH_SIZE distinct images per encoder pass (the last batch padded with its last image, whose results are
        dropped), all N samples of those images as one head pass of N x TEST_BATCH_SIZE rows (Generator.sample ->
        Discriminator.score_samples), tokens and critic outputs copied to the host once per batch.  Same samples as the reference's
        protocol: sample k = pass * TEST_BATCH_SIZE + j of an image uses row j of that image's pass-th [TEST_BATCH_SIZE, 512] noise
        draw, drawn image after image.  Test-split images are decoded by a thread pool while the previous batch runs.

        With an average of G's weights (ema_decay, or one restored from the checkpoint) and eval_live off, G runs on the average."""
        with self._eval_weights():
            return self._test(max_images, out_path, reference_literal, items, return_details)

    def _test(self, max_images, out_path, reference_literal, items, return_details):
        if self.step is None:
            images, _ = self._next_batch(0)
            self._constructOps(images)
        self.step.flush()
        K = kernels_for(self.device)
        TB = max(1, self.TEST_BATCH_SIZE)
        passes = self.TEST_BATCH_MULTIPLIER
        n_samples = passes * TB
        decode = None
        if items is not None:
            items = list(items)[:max_images]
        elif self.dataset is None:
            g = torch.Generator().manual_seed(self.seed + 99)
            items = [(torch.randn((self.image_size, self.image_size, 3), generator=g),
                      torch.randint(0, len(self.vocab), (5, 3), generator=g).tolist()) for _ in range(max_images or 2)]
        else:
            items, decode = list(self.test_items[:max_images]), self._parseFunction
        nb = min(TB, len(items))                        # images per encoder pass
        pool = ThreadPoolExecutor(max_workers=min(16, nb)) if decode is not None else None

        def fetch(i0):
            chunk = items[i0:i0 + nb]
            return [pool.submit(decode, k) for k, _ in chunk] if pool is not None else [im for im, _ in chunk]

        gen = torch.Generator().manual_seed(self.seed + 123)
        toks = torch.empty((n_samples, nb, 3), dtype=torch.int64, device=self.device)
        relax = self._eval_relax_kw()       # the critic scores what it was trained on
        r50, r100, details = [], [], []
        try:
            pending = fetch(0) if items else None
            for i0 in range(0, len(items), nb):
                imgs = [f.result() for f in pending] if pool is not None else pending
                pending = fetch(i0 + nb) if i0 + nb < len(items) else None
                n = len(imgs)
                images = torch.stack(imgs + [imgs[-1]] * (nb - n)).to(self.device)
                noise = torch.zeros((n_samples, nb, 512))
                for j in range(n):
                    for p in range(passes):
                        noise[p * TB:(p + 1) * TB, j] = torch.randn((TB, 512), generator=gen)
                logits = self.g.sample(images, n_samples, noise.to(self.device))
                K.argmax_rows(logits, toks.view(-1))
                d = self.d.score_samples(logits, images, **relax)   # (relaxed: in place on the logits, behind the argmax)
                tok_h, d_h = toks.cpu().numpy(), d.cpu().numpy()
                score_h = d_h.mean(axis=2).reshape(n_samples, nb)
                for j in range(n):
                    fake, score = tok_h[:, j].copy(), score_h[:, j].copy()
                    a, b = self.recalls(fake, score, items[i0 + j][1], reference_literal)
                    r50.append(a)
                    r100.append(b)
                    details.append({"tokens": fake, "scores": score, "r50": a, "r100": b})
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)
        res = (float(np.mean(r50)), float(np.mean(r100)))
        ordering = "reference_literal ([N,1] argsort: sample 0 repeated)" if reference_literal else "ascending mean critic score"
        if self.rank == 0 and out_path:
            with open(out_path, "w") as f:
                f.write("{}\n{}\n# ordering: {}\n".format(res[0], res[1], ordering))
                if self.relaxed:
                    f.write("# generator_output: {}\n".format(json.dumps(self._relax_label())))
        if self.rank == 0:
            summary = {"R@50": res[0], "R@100": res[1], "ordering": ordering, "images": len(items), "samples_per_image": n_samples}
            if self.relaxed:
                summary["generator_output"] = self._relax_label()
            print(summary)
        return (res, details) if return_details else res

    def sample_triples(self, images, noise=None):
        """tf.argmax(fake_inputs, -1) -> words (train.py:269-275), with the trained weights."""
        logits = self._Generator(images, False) if noise is None else self.g.build_generator(images, False, noise)
        toks = torch.empty((images.shape[0], 3), dtype=torch.int64, device=images.device)
        kernels_for(images.device).argmax_rows(logits, toks.view(-1))
        return toks, [[self.reverse_vocab.get(int(i), "UNK") for i in row] for row in toks.cpu()]

    ############################################################
    ## Saliency (input gradients, sgg_amd/grad.py)
    ############################################################
    def saliency(self, images, noise=None):
        """Which pixels drove each word of the generator's triple: images [B, S, S, 3] (standardised), noise [B, 512] (torch.randn if
        None).  Returns a dict of device tensors: tokens [B, 3] (argmax, as sample_triples), words, attention [B, 3, Hf, Wf] (the
        attention of each step), saliency [B, 3, S, S] = max over channels of |d logit[b, t, token_bt] / d image[b]| (Simonyan et
        al. 2014), and the noise used.  All three words share one noise draw and one forward pass; each word's gradient is its own
        data-only backward from that pass (Generator.saliency_gradients).  The weights and optimiser state are not touched.  With an
        average of G's weights and eval_live off, G runs on the average."""
        if self.step is not None:
            self.step.flush()
        with self._eval_weights() if self.evaluates_average else contextlib.nullcontext():      # (no networks are built here)
            tokens, grads, noise = self.g.saliency_gradients(images, noise)
        B, S = int(images.shape[0]), int(images.shape[1])
        al = self.g.alphas
        side = int(round(al.shape[-1] ** 0.5))
        words = [[self.reverse_vocab.get(int(i), "UNK") for i in row] for row in tokens.cpu()]
        return {"tokens": tokens, "words": words, "attention": al.view(B, 3, side, side),
                "saliency": grads.abs().amax(dim=-1).permute(1, 0, 2, 3).contiguous(), "noise": noise}

    def _saliency_items(self, max_images=None):
        """(key, image or path) of the images --saliency_dir covers: the test split, or with --synthetic the synthetic test images of
        test() (same seed)."""
        if self.dataset is None:
            g = torch.Generator().manual_seed(self.seed + 99)
            out = []
            for i in range(max_images or 2):
                out.append((str(i), torch.randn((self.image_size, self.image_size, 3), generator=g)))
                torch.randint(0, len(self.vocab), (5, 3), generator=g)      # (test()'s true triples: same image sequence)
            return out
        return [(k, k) for k, _ in self.test_items[:max_images]]

    def write_saliency(self, out_dir, max_images=None):
        """Saliency maps of the test images, TEST_BATCH_SIZE images per call, seeded noise: one <index>.npz per image (tokens, words,
        attention, saliency, noise) and index.json (image path or index -> npz file and words)."""
        os.makedirs(out_dir, exist_ok=True)
        items = self._saliency_items(max_images)
        nb = max(1, min(self.TEST_BATCH_SIZE, len(items)))
        gen = torch.Generator().manual_seed(self.seed + 321)
        index = {}
        with self._eval_weights() as weights:
            for i0 in range(0, len(items), nb):
                chunk = items[i0:i0 + nb]
                imgs = [self._parseFunction(x) if isinstance(x, str) else x for _, x in chunk]
                n = len(imgs)
                images = torch.stack(imgs + [imgs[-1]] * (nb - n)).to(self.device)      # (the last batch padded with its last image)
                noise = torch.randn((nb, 512), generator=gen).to(self.device)
                r = self.saliency(images, noise)
                tok, att, sal, nz = (r[k].cpu().numpy() for k in ("tokens", "attention", "saliency", "noise"))
                for j in range(n):
                    name = "%06d.npz" % (i0 + j)
                    np.savez(os.path.join(out_dir, name), tokens=tok[j], words=np.array(r["words"][j]), attention=att[j], saliency=sal[j],
                             noise=nz[j])
                    index[chunk[j][0]] = {"file": name, "words": r["words"][j]}
        if weights == "ema":
            index["generator_weights"] = "ema"
        with open(os.path.join(out_dir, "index.json"), "w") as f:
            json.dump(index, f, indent=1)
        if self.rank == 0:
            print({"saliency_dir": out_dir, "images": len(items)})
        return index

    ############################################################
    ## Prediction: the ranked distinct triples of an image (csrc/rank.hip, sgg_amd/predict.py)
    ############################################################
    def _predict_items(self, items=None, max_images=None):
        """[(key, image tensor or path)]: items may hold standardised [S,S,3] tensors, image paths or (image, anything) pairs; the
        default is the test split, or with --synthetic the synthetic images of test() (same seed, same sequence).  key = the path,
        or the index for a tensor."""
        if items is None:
            return self._saliency_items(max_images)
        out = []
        for i, it in enumerate(list(items)[:max_images]):
            x = it[0] if isinstance(it, (tuple, list)) else it
            out.append((x if isinstance(x, str) else str(i), x))
        return out

    def _sampling_setup(self, who, n_samples, top_k, decode="samples"):
        """(kernels, V, TEST_BATCH_SIZE, samples per image, list slots) of predict() / evaluate(); builds the networks if needed.
        decode="kbest": the defaults and limits of sgg_amd.kbest.setup."""
        if self.step is None:
            images, _ = self._next_batch(0)
            self._constructOps(images)
        self.step.flush()
        TB = max(1, self.TEST_BATCH_SIZE)
        if decode == "kbest":
            N, _, top_k = kbestmod.setup(who, n_samples, top_k, len(self.vocab), TB)
            return kernels_for(self.device), len(self.vocab), TB, N, top_k
        N = int(n_samples) if n_samples is not None else self.TEST_BATCH_MULTIPLIER * TB
        top_k = int(top_k) if top_k is not None else N
        if not 1 <= top_k <= N <= 4096:
            raise ValueError("%s: 1 <= top_k <= n_samples <= 4096 (got top_k = %d, n_samples = %d)" % (who, top_k, N))
        return kernels_for(self.device), len(self.vocab), TB, N, top_k

    def _device_pack(self, parts, device):
        """ONE uint8 buffer on `device` carved into the tensors `parts` = [(name, numpy dtype, shape)] (8-byte aligned), so that they
        cross the bus as one copy: (buffer, {name: tensor view}, views(buffer on the other side as numpy) -> {name: array})."""
        offs, total = {}, 0
        for name, dt, shape in parts:
            offs[name] = total
            total += -(-int(np.prod(shape)) * np.dtype(dt).itemsize // 8) * 8
        packed = torch.empty((total,), dtype=torch.uint8, device=device)
        tdt = {np.int64: torch.int64, np.float32: torch.float32, np.int32: torch.int32, np.float64: torch.float64}
        size = lambda dt, shape: int(np.prod(shape)) * np.dtype(dt).itemsize
        out = {name: packed[offs[name]:offs[name] + size(dt, shape)].view(tdt[dt]).view(shape) for name, dt, shape in parts}
        views = lambda host: {name: host[offs[name]:offs[name] + size(dt, shape)].view(dt).reshape(shape) for name, dt, shape in parts}
        return packed, out, views

    def _sample_batches(self, items, N, nb):
        """The generator passes both decoding modes share.  items: [(key, image tensor or path)]; per batch of nb images (the last
        one padded with its last image): Generator.sample; yields (i0, n, images, logits) = first item and number of real images of
        the batch, its images and its logits [N, nb, 3, V] (a view of the head rows: the next batch overwrites it).  Noise: per
        image ceil(N / TEST_BATCH_SIZE) draws of [TEST_BATCH_SIZE, 512] from seed + 123, image after image."""
        TB = max(1, self.TEST_BATCH_SIZE)
        passes = -(-N // TB)
        load = lambda x: self._parseFunction(x) if isinstance(x, str) else x
        pool = ThreadPoolExecutor(max_workers=min(16, nb)) if any(isinstance(x, str) for _, x in items) else None
        fetch = lambda i0: [pool.submit(load, x) if pool is not None else x for _, x in items[i0:i0 + nb]]
        gen = torch.Generator().manual_seed(self.seed + 123)
        try:
            pending = fetch(0)
            for i0 in range(0, len(items), nb):
                imgs = [f.result() for f in pending] if pool is not None else pending
                pending = fetch(i0 + nb) if i0 + nb < len(items) else None
                n = len(imgs)
                images = torch.stack(imgs + [imgs[-1]] * (nb - n)).to(self.device)      # (the last batch padded with its last image)
                noise = torch.zeros((passes * TB, nb, 512))
                for j in range(n):
                    for p in range(passes):
                        noise[p * TB:(p + 1) * TB, j] = torch.randn((TB, 512), generator=gen)
                yield i0, n, images, self.g.sample(images, N, noise[:N].to(self.device))
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)

    def _ranked_batches(self, K, items, N, nb, top_k, descending, out, toks=None):
        """The sampling passes predict() and evaluate() share: per batch of _sample_batches, argmax_rows ->
        Discriminator.score_samples -> rank_triples into `out`; yields (i0, n) with `out` (and self.g.alphas) holding the batch's
        results.  toks: an int64 [N, nb, 3] tensor of the caller's that receives the sample tokens (grounding reads them)."""
        V = len(self.vocab)
        if toks is None:
            toks = torch.empty((N, nb, 3), dtype=torch.int64, device=self.device)
        relax = self._eval_relax_kw()       # the critic scores what it was trained on
        with contextlib.closing(self._sample_batches(items, N, nb)) as batches:
            for i0, n, images, logits in batches:
                K.argmax_rows(logits, toks.view(-1))
                d = self.d.score_samples(logits, images, **relax)   # (relaxed: in place on the logits, behind the argmax)
                K.rank_triples(toks, d.view(N, nb, 3), top_k, descending=descending, vocab=V, out=out)
                yield i0, n

    def _kbest_batches(self, K, items, N, nb, top_k, out, toks=None):
        """K-best decoding of the same passes: per batch of _sample_batches, kbest_triples (the list_width most probable triples of
        every head row) -> kbest_merge into `out`.  The discriminator is not run.  toks: an int64 [N, nb, 3] tensor of the caller's;
        given, one argmax_rows of the logits fills it with the sample tokens (grounding reads them)."""
        width = kbestmod.list_width(N, len(self.vocab))
        lists = {"triples": torch.empty((N * nb, width, 3), dtype=torch.int64, device=self.device),
                 # (the per-row logp is an output the binding requires; nothing here reads it: the merge scores every triple anew
                 #  over all N samples)
                 "logp": torch.empty((N * nb, width), dtype=torch.float32, device=self.device),
                 "lse": torch.empty((N * nb, 3), dtype=torch.float32, device=self.device)}
        with contextlib.closing(self._sample_batches(items, N, nb)) as batches:
            for i0, n, images, logits in batches:
                if toks is not None:
                    K.argmax_rows(logits, toks.view(-1))
                K.kbest_triples(logits, width, out=lists)
                K.kbest_merge(lists["triples"].view(N, nb, width, 3), logits, lists["lse"], top_k, out=out)
                yield i0, n

    def _predict_iter(self, items=None, max_images=None, n_samples=None, top_k=None, descending=False, with_attention=False,
                      logits_budget_bytes=DEFAULT_LOGITS_BUDGET_BYTES, decode="samples", ground=False,
                      ground_overlap=groundmod.DEFAULT_OVERLAP, ground_box_frac=groundmod.DEFAULT_BOX_FRAC):
        """predict(), one image at a time (write_predictions streams it to disk)."""
        kbest = kbestmod.check_decode(decode, descending) == "kbest"
        if ground:
            ground_overlap, ground_box_frac = groundmod.check_ground_args(ground_overlap, ground_box_frac)
        K, V, TB, N, top_k = self._sampling_setup("predict", n_samples, top_k, decode)
        if ground:
            groundmod.check_ground_args(ground_overlap, ground_box_frac, top_k)
            need_kernels(K, "predict(ground=True)", "ground_assign", "ground_pool", "ground_resolve")
        items = self._predict_items(items, max_images)
        if not items:
            return
        nb = images_per_pass(N, V, TB, len(items), logits_budget_bytes)
        ordering = kbestmod.ORDERING if kbest else "%s mean critic score" % ("descending" if descending else "ascending")
        # the ranked outputs of a batch live in ONE device buffer (carved into the kernel's output tensors): one copy to the host
        # (K-best: the kernel's best_sample is the record's first_sample, the sample that gives the triple its highest probability)
        fields = [("scores", np.float32), ("best_sample", np.int32), ("best_logp", np.float32), ("counts", np.int32)] if kbest else \
                 [("scores", np.float32), ("first_rank", np.int32), ("first_sample", np.int32), ("counts", np.int32)]
        parts = [("triples", np.int64, (nb, top_k, 3))] + [(f, dt, (nb, top_k)) for f, dt in fields] + [("n_distinct", np.int32, (nb,))]
        sample_of = "best_sample" if kbest else "first_sample"
        toks = gbuf = None
        if ground:
            # grounding (csrc/ground.hip): its outputs join the packed buffer, except the node maps, of which only the rows in front
            # of the batch's largest n_nodes are copied; the sample tokens and the three intermediate arrays never leave the device
            L, S = int(self.g.net.trunk.L), int(self.g.net.trunk.S)
            Hf = Wf = int(round(L ** 0.5))
            i32, dev = torch.int32, self.device
            parts += [("mention_node", np.int32, (nb, top_k, 2)), ("n_pooled", np.int32, (nb, top_k)),
                      ("maps", np.float32, (nb, top_k, 3, L)), ("n_nodes", np.int32, (nb,)), ("node_word", np.int64, (nb, 2 * top_k)),
                      ("node_first", np.int32, (nb, 2 * top_k)), ("node_weight", np.int32, (nb, 2 * top_k)),
                      ("node_mentions", np.int32, (nb, 2 * top_k)), ("node_box", np.int32, (nb, 2 * top_k, 4)),
                      ("node_center", np.float32, (nb, 2 * top_k, 2))]
            toks = torch.empty((N, nb, 3), dtype=torch.int64, device=dev)
            gbuf = {"slot_of_sample": torch.empty((nb, N), dtype=i32, device=dev), "members": torch.empty((nb, N), dtype=i32, device=dev),
                    "start": torch.empty((nb, top_k + 1), dtype=i32, device=dev),
                    "node_map": torch.empty((nb, 2 * top_k, L), dtype=torch.float32, device=dev)}
        packed, out, views = self._device_pack(parts, self.device)
        col = torch.arange(nb, device=self.device).view(nb, 1)
        batches = self._kbest_batches(K, items, N, nb, top_k, out, toks) if kbest else \
            self._ranked_batches(K, items, N, nb, top_k, descending, out, toks)
        for i0, n in batches:
            if ground:              # right behind the ranking, on the attention of the same g.sample call (score_samples ran D's head)
                K.ground_assign(toks, out["triples"], out["n_distinct"], vocab=V, out=gbuf)
                K.ground_pool([a[0] for a in self.g._alphas], gbuf["members"], gbuf["start"], out[sample_of], out["n_distinct"], out=out)
                res_names = ("mention_node", "n_nodes", "node_word", "node_first", "node_weight", "node_mentions", "node_box",
                             "node_center")
                K.ground_resolve(out["maps"], out["triples"], out["n_distinct"], out["n_pooled"], Hf, Wf, ground_overlap,
                                 ground_box_frac, out=dict({k: out[k] for k in res_names}, node_map=gbuf["node_map"]))
            if with_attention:      # the attention of every triple's first-occurrence sample: head row first_sample * nb + j
                rows = out[sample_of].long().clamp_(min=0) * nb + col
                al = self.g.alphas
                side = int(round(al.shape[-1] ** 0.5))
                att_h = al[rows.view(-1)].view(nb, top_k, 3, side, side).cpu().numpy()
            h = views(packed.cpu().numpy())
            if ground:
                most = int(h["n_nodes"][:n].max())
                node_map_h = gbuf["node_map"][:, :most].cpu().numpy()
            for j in range(n):
                nd = int(h["n_distinct"][j])
                U = min(nd, top_k)
                r = {"image": items[i0 + j][0], "n_distinct": nd, "ordering": ordering}
                for name in ["triples"] + [f for f, _ in fields]:
                    r["first_sample" if name == "best_sample" else name] = h[name][j, :U].copy()
                r["words"] = [[self.reverse_vocab.get(int(i), "UNK") for i in row] for row in r["triples"]]
                r["graph"] = scene_graph(r["triples"], r["scores"], r["counts"], self.reverse_vocab)
                if with_attention:
                    r["attention"] = att_h[j, :U].copy()
                if ground:
                    nn = int(h["n_nodes"][j])
                    nodes = {f: h["node_" + f][j, :nn].copy() for f in groundmod.NODE_FIELDS if f != "map"}
                    nodes["map"] = node_map_h[j, :nn].reshape(nn, Hf, Wf).copy()
                    r["grounding"] = {"mention_node": h["mention_node"][j, :U].copy(), "n_pooled": h["n_pooled"][j, :U].copy(),
                                      "pooled_attention": h["maps"][j, :U].reshape(U, 3, Hf, Wf).copy(), "nodes": nodes}
                    r["grounded_graph"] = groundmod.grounded_scene_graph(r["triples"], r["scores"], r["counts"], self.reverse_vocab,
                                                                         r["grounding"]["mention_node"], nodes, S)
                yield r

    def predict(self, items=None, max_images=None, n_samples=None, top_k=None, descending=False, with_attention=False,
                logits_budget_bytes=DEFAULT_LOGITS_BUDGET_BYTES, decode="samples", ground=False,
                ground_overlap=groundmod.DEFAULT_OVERLAP, ground_box_frac=groundmod.DEFAULT_BOX_FRAC):
        """The scene graph of every image: its n_samples generator samples (default TEST_BATCH_MULTIPLIER x TEST_BATCH_SIZE) scored by
        the critic as in test(), reduced on the device to the DISTINCT triples in ranked order (K.rank_triples: ascending mean
        critic score - the order of test() - or descending=True for the highest score first; ties by sample index), the first top_k
        of them kept (default: all).

        items: list of standardised [S,S,3] tensors, image paths or (image, anything) pairs; default: the test split, or with
        --synthetic the synthetic images of test().  Returns one dict per image: triples [U,3] int64, words, scores [U] (of each
        triple's best-ranked sample), first_rank [U] (position of that sample among the n_samples ordered ones), first_sample [U],
        counts [U] (samples that were this triple), n_distinct (before top_k), graph (sgg_amd.predict.scene_graph), ordering, image
        (path or index) and, with with_attention, attention [U,3,Hf,Wf]: the generator's attention of each triple's first_sample.

        Schedule: sgg_amd.predict.images_per_pass images per encoder pass (TEST_BATCH_SIZE unless the [n_samples, nb, 3, V] logits
        exceed logits_budget_bytes; the last batch padded with its last image), Generator.sample -> argmax_rows ->
        Discriminator.score_samples -> rank_triples, one copy of the ranked outputs to the host per batch (tokens and scores of the
        samples stay on the device).  Noise: per image ceil(n_samples / TEST_BATCH_SIZE) draws of [TEST_BATCH_SIZE, 512] from seed
        + 123, image after image, the first n_samples rows used - with the defaults the stream of test(), sample for sample.
        Touches no weights and no optimiser state; usable on an untrained model, as test() is.

        decode="kbest" (default "samples": everything above): no tokens are sampled and the critic is not run.  The generator's three
        softmaxes are independent given the noise, so each of the n_samples head rows (default here: TEST_BATCH_SIZE) yields its
        sgg_amd.kbest.list_width most probable triples exactly (K.kbest_triples), and K.kbest_merge ranks the distinct triples of an
        image's lists by their log-probability under the mixture of its n_samples noise draws, highest first (ties by the triple).
        Same batches, padding, noise stream (the first n_samples rows are the same draws) and weights.  The record then holds
        triples, words, scores [U] (the mixture log-probability), first_sample [U] (the sample that gives the triple its highest
        probability: with_attention shows that sample's attention), best_logp [U] (that probability's log), counts [U] (lists that
        hold the triple), n_distinct, graph, ordering and image, and no first_rank.  top_k <= n_samples x list width (default: all
        of them); descending=True is rejected.  With one sample the list is the exact K-best list; with more, the candidates are the
        union of the per-sample lists, which approximates the mixture's own K best.

        ground=True (either decoding mode; top_k <= 1024): the subjects and objects of the ranked triples are resolved to entity
        INSTANCES from the generator's attention (sgg_amd/ground.py states the definitions; csrc/ground.hip).  Right behind the
        ranking, on the attention of the same Generator.sample call: K.ground_assign (which samples are which triple; under
        decode="kbest" the sample tokens come from one argmax_rows of the logits) -> K.ground_pool (per triple and decoding step
        the mean attention of its samples; a K-best triple that is no sample's argmax takes its first_sample's row) ->
        K.ground_resolve (two mentions of one word are one node when their pooled maps overlap by ground_overlap or more, sum of
        the cell-wise minimum; per node the weighted mean map, the cell box of everything at or above ground_box_frac of its
        maximum, and the centre of mass).  The outputs ride in the same packed copy; of the node maps only the rows in front of the
        batch's largest node count are copied.  The record gains "grounding": mention_node [U, 2], n_pooled [U], pooled_attention
        [U, 3, Hf, Wf] and nodes (word, first, weight, mentions [n], map [n, Hf, Wf], box [n, 4] as y0, x0, y1, x1 inclusive cells,
        center [n, 2] as y, x in cells), and "grounded_graph" (sgg_amd.ground.grounded_scene_graph: boxes and centres in input
        pixels); "graph" stays the word-merged graph.  Both thresholds default to 0.5 and are untuned, and whether the attention
        of a trained model localises entities has not been measured.  With ground=False nothing of this is allocated or launched."""
        kbestmod.check_decode(decode, descending)
        with self._eval_weights():
            return list(self._predict_iter(items, max_images, n_samples, top_k, descending, with_attention, logits_budget_bytes,
                                           decode, ground, ground_overlap, ground_box_frac))

    def write_predictions(self, out_dir, max_images=None, n_samples=None, top_k=None, descending=False, items=None, decode="samples",
                          ground=False, ground_overlap=groundmod.DEFAULT_OVERLAP, ground_box_frac=groundmod.DEFAULT_BOX_FRAC):
        """predict(with_attention=True) of the test images to disk: one <index>.npz per image (triples, words, scores, first_rank,
        first_sample, counts, n_distinct, attention) and index.json (image path or index -> npz file, n_distinct and the graph).
        decode="kbest": the arrays of that record (best_logp in place of first_rank), and index.json says "decode": "kbest".
        ground=True: predict(ground=True); the .npz gains ground_mention_node, ground_n_pooled, ground_pooled_attention and
        ground_node_word / _first / _weight / _mentions / _map / _box / _center, every image of index.json gains "grounded_graph",
        and index.json says "ground": {"overlap", "box_frac"}."""
        kbestmod.check_decode(decode, descending)
        if ground:
            ground_overlap, ground_box_frac = groundmod.check_ground_args(ground_overlap, ground_box_frac)
        os.makedirs(out_dir, exist_ok=True)
        index = {}
        extra = "best_logp" if decode == "kbest" else "first_rank"
        with self._eval_weights() as weights:
            for i, r in enumerate(self._predict_iter(items, max_images, n_samples, top_k, descending, with_attention=True,
                                                     decode=decode, ground=ground, ground_overlap=ground_overlap,
                                                     ground_box_frac=ground_box_frac)):
                name = "%06d.npz" % i
                arrays = {extra: r[extra]}
                if ground:
                    gr = r["grounding"]
                    arrays.update({"ground_" + k: gr[k] for k in ("mention_node", "n_pooled", "pooled_attention")})
                    arrays.update({"ground_node_" + k: v for k, v in gr["nodes"].items()})
                np.savez(os.path.join(out_dir, name), triples=r["triples"], words=np.array(r["words"], dtype=str).reshape(-1, 3),
                         scores=r["scores"], first_sample=r["first_sample"], counts=r["counts"],
                         n_distinct=np.int32(r["n_distinct"]), attention=r["attention"], **arrays)
                index[r["image"]] = {"file": name, "n_distinct": r["n_distinct"], "graph": r["graph"]}
                if ground:
                    index[r["image"]]["grounded_graph"] = r["grounded_graph"]
        n_images = len(index)
        if weights == "ema":
            index["generator_weights"] = "ema"
        if decode == "kbest":
            index["decode"] = "kbest"
        elif self.relaxed:                  # (the critic ranked softmax(logits / tau); K-best decoding does not run it)
            index["generator_output"] = self._relax_label()
        if ground:
            index["ground"] = {"overlap": ground_overlap, "box_frac": ground_box_frac}
        with open(os.path.join(out_dir, "index.json"), "w") as f:
            json.dump(index, f, indent=1)
        if self.rank == 0:
            print({"predict_dir": out_dir, "images": n_images})
        return index


    ############################################################
    ## Metrics: R@K, mR@K, zsR@K over distinct predictions (csrc/match.hip, sgg_amd/metrics.py)
    ############################################################
    def _evaluate_items(self, items=None, max_images=None):
        """[(key, image tensor or path, [[s, p, o], ...])]: the given (image, triples) pairs, else the test split with its true
        triples, or with --synthetic the synthetic images and triples of test() (same seed)."""
        if items is not None:
            return [(x if isinstance(x, str) else str(i), x, [list(map(int, t)) for t in real])
                    for i, (x, real) in enumerate(list(items)[:max_images])]
        if self.dataset is None:
            g = torch.Generator().manual_seed(self.seed + 99)
            return [(str(i), torch.randn((self.image_size, self.image_size, 3), generator=g),
                     torch.randint(0, len(self.vocab), (5, 3), generator=g).tolist()) for i in range(max_images or 2)]
        return [(k, k, real) for k, real in self.test_items[:max_images]]

    def evaluate(self, items=None, max_images=None, ks=(20, 50, 100), n_samples=None, descending=False, train_triples=None,
                 return_details=False, out_path=None, logits_budget_bytes=DEFAULT_LOGITS_BUDGET_BYTES, decode="samples"):
        """R@K, mR@K and zsR@K of the model (sgg_amd.metrics.RecallAccumulator has the definitions): per image the ranked list of
        DISTINCT triples of predict() - same passes, same noise stream, same order - cut at max(ks), and the image's true triples
        matched against it on the device (K.match_triples).  Distinct predictions, denominators |GT|: not the protocol of test(),
        whose top 50 / 100 are samples (duplicates use up the budget) and whose denominators are the constants 50 and 100.

        items: list of (standardised [S,S,3] tensor or image path, [[s, p, o], ...]); default: the test split, or with --synthetic
        the synthetic images and triples of test().  train_triples: set of (s, p, o) tuples that zsR@K counts as seen; default:
        every triple of the training images (the train and val label arrays, both from the 90 % image split), or None with
        --synthetic (zsR@K is then None).  Returns RecallAccumulator.result() plus ks, samples_per_image, ordering, mean_n_distinct,
        definition and, with return_details, details: per image {"image", "pos", "n_gt", "n_distinct"}; rank 0 writes the dict as
        JSON to out_path.  A ground-truth list of more than 4096 triples or a token outside the vocabulary raises ValueError
        before anything is launched.

        Schedule: the batches of predict(); per batch one copy to the device (the padded ground truth and its counts) and one
        copy back (pos, n_gt, n_distinct).  Ranked triples, tokens and scores stay on the device.  Touches no weights and no
        optimiser state; usable on an untrained model, as test() and predict() are.

        With an average of G's weights and eval_live off, G runs on the average and the result says "generator_weights": "ema".

        decode="kbest": the ranked list is that of predict(decode="kbest") - the K-best triples of n_samples head rows (default
        TEST_BATCH_SIZE) merged by mixture log-probability, no critic pass - cut at min(max(ks), n_samples x list width); the
        result says "decode": "kbest".  descending=True is rejected."""
        kbestmod.check_decode(decode, descending)
        with self._eval_weights() as weights:
            return self._evaluate(items, max_images, ks, n_samples, descending, train_triples, return_details, out_path,
                                  logits_budget_bytes, weights, decode)

    def _evaluate(self, items, max_images, ks, n_samples, descending, train_triples, return_details, out_path, logits_budget_bytes,
                  weights, decode="samples"):
        kbest = decode == "kbest"
        ks = tuple(sorted(set(int(k) for k in ks)))
        if not ks or ks[0] < 1:
            raise ValueError("evaluate: ks must be positive integers (got %r)" % (ks,))
        items = self._evaluate_items(items, max_images)
        V = len(self.vocab)
        for key, _, real in items:
            if len(real) > MAX_GT:
                raise ValueError("evaluate: image %s has %d ground-truth triples (at most %d per image)" % (key, len(real), MAX_GT))
            for t in real:
                if len(t) != 3 or not all(0 <= x < V for x in t):
                    raise ValueError("evaluate: image %s: ground-truth triple %r is not three tokens in [0, %d)" % (key, list(t), V))
        if train_triples is None and self.dataset is not None:
            train_triples = set(map(tuple, np.concatenate([self.dataset["train"][1], self.dataset["val"][1]]).tolist()))
        K, V, TB, N, slots = self._sampling_setup("evaluate", n_samples, None, decode)
        top_k = min(max(ks), slots)
        acc = RecallAccumulator(ks, V)
        details, nd_all = [], []
        if items:
            nb = images_per_pass(N, V, TB, len(items), logits_budget_bytes)
            M = max(1, max(len(real) for _, _, real in items))
            ranked = {name: torch.empty(shape, dtype=dt, device=self.device) for name, shape, dt in
                      [("triples", (nb, top_k, 3), torch.int64), ("scores", (nb, top_k), torch.float32)] +
                      ([("best_sample", (nb, top_k), torch.int32), ("best_logp", (nb, top_k), torch.float32)] if kbest else
                       [("first_rank", (nb, top_k), torch.int32), ("first_sample", (nb, top_k), torch.int32)]) +
                      [("counts", (nb, top_k), torch.int32)]}
            packed, back, views = self._device_pack([("pos", np.int32, (nb, M)), ("n_gt", np.int32, (nb,)),
                                                     ("n_distinct", np.int32, (nb,))], self.device)
            ranked["n_distinct"] = back["n_distinct"]
            gt_parts = [("gt", np.int64, (nb, M, 3)), ("gt_count", np.int32, (nb,))]
            gt_host, _, gt_views = self._device_pack(gt_parts, "cpu")
            gt_h = gt_views(gt_host.numpy())                    # (numpy views of the host buffer: filled in place)
            gt_packed, gt_d, _ = self._device_pack(gt_parts, self.device)
            plain = [(key, x) for key, x, _ in items]
            batches = self._kbest_batches(K, plain, N, nb, top_k, ranked) if kbest else \
                self._ranked_batches(K, plain, N, nb, top_k, descending, ranked)
            for i0, n in batches:
                gt_h["gt"][:] = 0
                gt_h["gt_count"][:] = 0                  # (the padded images of the last batch: no ground truth)
                for j in range(n):
                    real = items[i0 + j][2]
                    gt_h["gt"][j, :len(real)] = np.asarray(real, dtype=np.int64).reshape(-1, 3)
                    gt_h["gt_count"][j] = len(real)
                gt_packed.copy_(gt_host)
                K.match_triples(ranked["triples"], ranked["n_distinct"], gt_d["gt"], gt_d["gt_count"], vocab=V, out=back)
                h = views(packed.cpu().numpy())
                for j in range(n):
                    key, _, real = items[i0 + j]
                    pos = h["pos"][j, :len(real)].copy()
                    acc.add(pos, real, None if train_triples is None else zero_shot_mask(real, train_triples))
                    nd_all.append(int(h["n_distinct"][j]))
                    if return_details:
                        details.append({"image": key, "pos": pos.tolist(), "n_gt": int(h["n_gt"][j]), "n_distinct": nd_all[-1]})
        res = acc.result(self.reverse_vocab)
        res.update({"ks": list(ks), "samples_per_image": N,
                    "ordering": kbestmod.ORDERING if kbest else "%s mean critic score" % ("descending" if descending else "ascending"),
                    "mean_n_distinct": float(np.mean(nd_all)) if nd_all else None,
                    "definition": "distinct predictions, denominators |GT|: R@K = mean over images of hits in the first K distinct "
                                  "triples / |GT|; mR@K = mean over predicates of the per-predicate mean over images; zsR@K = R@K on "
                                  "the triples absent from the training set"})
        if return_details:
            res["details"] = details
        if weights == "ema":
            res["generator_weights"] = "ema"
        if kbest:
            res["decode"] = "kbest"
        elif self.relaxed:
            res["generator_output"] = self._relax_label()
        if self.rank == 0 and out_path:
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)
        return res


    ############################################################
    ## Likelihood: held-out NLL of the true triples under the generator's softmaxes (csrc/xent.hip)
    ############################################################
    def likelihood(self, items=None, max_images=None, n_samples=None, out_path=None, logits_budget_bytes=DEFAULT_LOGITS_BUDGET_BYTES):
        """The negative log-likelihood the generator assigns to the true triples of the test images - threshold-free, and comparable
        between checkpoints and between live and averaged weights.  Given a noise draw the three decoder softmaxes are independent
        (sgg_amd/kbest.py), so a triple's probability under the image's n_samples draws (default TEST_BATCH_MULTIPLIER x
        TEST_BATCH_SIZE) is the mixture of per-draw products.  Per batch of _sample_batches (the passes and the noise stream of
        predict() / evaluate()): the log-sum-exp of every decoder row (K.softmax_xent without labels), then K.triple_logp on the
        padded ground truth in the form evaluate() builds; one copy back per batch, sums in fp64 on the host.

        items: as evaluate().  Returns (rank 0 writes it as JSON to out_path): nll_mixture {"micro": mean over all valid true triples
        of -log p_mixture, "macro": mean over images of the image's mean}, nll_single (the same two means of the per-draw
        log-probability averaged over the draws: what one noise vector gives, >= nll_mixture by Jensen), nll_slot (its three slots:
        subject, predicate, object; micro), perplexity_token = exp(nll_single micro / 3), n_images, n_triples (valid ones),
        n_out_of_vocab (true triples with a token outside the vocabulary: counted, not scored), n_samples, generator_weights."""
        with self._eval_weights() as weights:
            items = self._evaluate_items(items, max_images)
            for key, _, real in items:
                if len(real) > MAX_GT:
                    raise ValueError("likelihood: image %s has %d ground-truth triples (at most %d per image)" % (key, len(real), MAX_GT))
            K, V, TB, N, _ = self._sampling_setup("likelihood", n_samples, None)
            tot = np.zeros(5, dtype=np.float64)             # sums over valid triples of -mix, -mean, -slot[0..2]
            per_image, n_valid, n_oov = [], 0, 0
            if items:
                nb = images_per_pass(N, V, TB, len(items), logits_budget_bytes)
                M = max(1, max(len(real) for _, _, real in items))
                packed, out, views = self._device_pack([("mix", np.float32, (nb, M)), ("mean", np.float32, (nb, M)),
                                                        ("slot", np.float32, (nb, M, 3)), ("status", np.int32, (nb, M))], self.device)
                gt_parts = [("gt", np.int64, (nb, M, 3)), ("gt_count", np.int32, (nb,))]
                gt_host, _, gt_views = self._device_pack(gt_parts, "cpu")
                gt_h = gt_views(gt_host.numpy())
                gt_packed, gt_d, _ = self._device_pack(gt_parts, self.device)
                lse = torch.empty((N, nb, 3), dtype=torch.float32, device=self.device)
                with contextlib.closing(self._sample_batches([(key, x) for key, x, _ in items], N, nb)) as batches:
                    for i0, n, images, logits in batches:
                        gt_h["gt"][:] = 0
                        gt_h["gt_count"][:] = 0             # (the padded images of the last batch: no ground truth)
                        for j in range(n):
                            real = items[i0 + j][2]
                            gt_h["gt"][j, :len(real)] = np.asarray(real, dtype=np.int64).reshape(-1, 3)
                            gt_h["gt_count"][j] = len(real)
                        gt_packed.copy_(gt_host)
                        K.softmax_xent(logits, None, lse=lse.view(-1))
                        K.triple_logp(logits, lse, gt_d["gt"], gt_d["gt_count"], out=out)
                        h = views(packed.cpu().numpy())
                        for j in range(n):
                            ok = h["status"][j] == 0
                            n_oov += int((h["status"][j] == -4).sum())
                            if not ok.any():
                                continue
                            row = np.concatenate([-h["mix"][j][ok].astype(np.float64)[:, None], -h["mean"][j][ok].astype(np.float64)[:, None],
                                                  -h["slot"][j][ok].astype(np.float64)], axis=1)
                            tot += row.sum(axis=0)
                            n_valid += int(ok.sum())
                            per_image.append(row[:, :2].mean(axis=0))
            micro = tot / n_valid if n_valid else np.full(5, np.nan)
            macro = np.mean(per_image, axis=0) if per_image else np.full(2, np.nan)
            num = lambda x: float(x) if np.isfinite(x) else None
            res = {"nll_mixture": {"micro": num(micro[0]), "macro": num(macro[0])},
                   "nll_single": {"micro": num(micro[1]), "macro": num(macro[1])},
                   "nll_slot": [num(x) for x in micro[2:5]],
                   "perplexity_token": num(np.exp(micro[1] / 3.0)) if n_valid else None,
                   "n_images": len(items), "n_triples": n_valid, "n_out_of_vocab": n_oov, "n_samples": N,
                   "generator_weights": weights}
            if self.rank == 0 and out_path:
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
            return res

    ############################################################
    ## Retrieval: images ranked by the generator's likelihood of a (partial) triple (csrc/retrieve.hip, sgg_amd/retrieve.py)
    ############################################################
    def retrieve(self, queries=None, items=None, max_images=None, n_samples=None, ks=(1, 5, 10), top_k=10, max_queries=retrmod.MAX_QUERIES,
                 return_details=False, out_path=None, logits_budget_bytes=DEFAULT_LOGITS_BUDGET_BYTES,
                 score_budget_bytes=retrmod.DEFAULT_SCORE_BUDGET_BYTES):
        """The other direction of likelihood(): given triples - whole ("man riding horse") or with open slots ("? riding horse") -
        rank the IMAGES of a collection by the probability the generator gives the query.  score(query, image) = log of the
        probability of the query's specified slots under the mixture of the image's n_samples noise draws (default
        TEST_BATCH_MULTIPLIER x TEST_BATCH_SIZE); an open slot is marginalised exactly (sgg_amd/retrieve.py).

        queries: list of triples as words or token ids, None / "?" / -1 for an open slot; default: sgg_amd.retrieve.default_queries
        of the evaluated images (their distinct true triples, most frequent first, at most max_queries).  A query with a word or id
        outside the vocabulary is counted (n_out_of_vocab) and not scored.  items: as evaluate(); an image is RELEVANT to a query
        when one of its true triples equals the query on every specified slot.

        Schedule: the passes and the noise stream of likelihood().  Per batch K.softmax_xent (lse only), then K.query_logp per block
        of 4096 queries, which writes the batch's columns of a device-resident [n_queries, n_images] score matrix (nothing is read
        back per batch; the padded images of the last batch land in columns behind n_images that nothing reads).  Behind the last
        batch one K.retrieve_topk and one K.retrieve_ranks per query block, one copy back, the sums in fp64 on the host
        (sgg_amd.retrieve.summarise).  A score matrix above score_budget_bytes raises ValueError before anything is launched.

        Returns (rank 0 writes it as JSON to out_path): retrieval {"R@K" for K in ks: share of the queries with a relevant image
        whose best-ranked relevant image is within the first K; median_rank; mrr; map}, ks, n_queries (scored), n_images,
        n_samples, n_without_relevant (scored queries without a relevant image: excluded from the metrics), n_out_of_vocab,
        generator_weights, decode ("likelihood": the generator alone ranks, the critic is not run) and, with return_details,
        details: per scored query {"query" (ids), "words", "top": [{"image", "score"}] (the first top_k images), "first_rank",
        "ap"} (None where there is no relevant image).  Touches no weights and no optimiser state."""
        with self._eval_weights() as weights:
            ks = tuple(sorted(set(int(k) for k in ks)))
            if not ks or ks[0] < 1:
                raise ValueError("retrieve: ks must be positive integers (got %r)" % (ks,))
            if not 1 <= int(top_k) <= retrmod.MAX_TOP:
                raise ValueError("retrieve: 1 <= top_k <= %d (got %r)" % (retrmod.MAX_TOP, top_k))
            top_k = int(top_k)
            items = self._evaluate_items(items, max_images)
            gt = [real for _, _, real in items]
            if queries is None:
                queries = retrmod.default_queries(gt, max_queries)
            queries = list(queries)[:max(0, int(max_queries))]
            cq = retrmod.compile_queries(queries, self.vocab)
            ids, Q, n_img = cq["ids"], int(cq["ids"].shape[0]), len(items)
            rel_ptr, rel_idx = retrmod.relevance(ids, gt)
            K, V, TB, N, _ = self._sampling_setup("retrieve", n_samples, None)
            first_rank, ap, status = np.zeros(Q, dtype=np.int32), np.full(Q, np.nan), np.full(Q, -3, dtype=np.int32)
            details = []
            if items and Q:
                need_kernels(K, "retrieve", "query_logp", "retrieve_topk", "retrieve_ranks")
                nb = images_per_pass(N, V, TB, n_img, logits_budget_bytes)
                cols = -(-n_img // nb) * nb                   # (the last batch's padded images get columns of their own)
                if retrmod.score_matrix_bytes(Q, cols) > score_budget_bytes:
                    raise ValueError("retrieve: the score matrix of %d queries x %d images takes %d bytes, above the budget of %d: "
                                     "pass fewer queries (max_queries / --retrieve_max_queries), fewer images (max_images / "
                                     "--max_test_images) or a larger score_budget_bytes"
                                     % (Q, cols, retrmod.score_matrix_bytes(Q, cols), score_budget_bytes))
                dev, QB = self.device, retrmod.MAX_QUERIES
                scores = torch.empty((Q, cols), dtype=torch.float32, device=dev)
                blocks = []                                   # per block of 4096 queries: its own token lists and indices
                for b0 in range(0, Q, QB):
                    c = retrmod.compile_queries(ids[b0:b0 + QB].tolist(), self.vocab)
                    blocks.append((b0, torch.from_numpy(c["tok"]).to(dev), c["ucount"], torch.from_numpy(c["qidx"]).to(dev)))
                lse = torch.empty((N, nb, 3), dtype=torch.float32, device=dev)
                with contextlib.closing(self._sample_batches([(key, x) for key, x, _ in items], N, nb)) as batches:
                    for i0, n, images, logits in batches:
                        K.softmax_xent(logits, None, lse=lse.view(-1))
                        for b0, tok, ucount, qidx in blocks:
                            K.query_logp(logits, lse, tok, ucount, qidx, scores[b0:b0 + qidx.shape[0]], col0=i0)
                top_w = min(top_k, n_img)
                # (the CSR arrays carry one spare entry: a block without a relevant image still hands the kernel an allocated one)
                parts = [("ap", np.float64, (Q,)), ("idx", np.int32, (Q, top_k)), ("scores", np.float32, (Q, top_k)),
                         ("ranks", np.int32, (len(rel_idx) + 1,)), ("first_rank", np.int32, (Q,)), ("status", np.int32, (Q,))]
                packed, out, views = self._device_pack(parts, dev)
                ptr_h = rel_ptr.astype(np.int64)
                idx_d = torch.from_numpy(np.concatenate([rel_idx, np.zeros(1, dtype=np.int32)])).to(dev)
                for b0, _, _, qidx in blocks:
                    b1 = b0 + int(qidx.shape[0])
                    K.retrieve_topk(scores[b0:b1], n_img, top_k, out={"idx": out["idx"][b0:b1], "scores": out["scores"][b0:b1]})
                    r0, r1 = int(ptr_h[b0]), int(ptr_h[b1])
                    ptr_d = torch.from_numpy((ptr_h[b0:b1 + 1] - r0).astype(np.int32)).to(dev)
                    K.retrieve_ranks(scores[b0:b1], n_img, ptr_d, idx_d[r0:max(r1, r0 + 1)],
                                     out={"ranks": out["ranks"][r0:max(r1, r0 + 1)], "first_rank": out["first_rank"][b0:b1],
                                          "ap": out["ap"][b0:b1], "status": out["status"][b0:b1]})
                h = views(packed.cpu().numpy())
                first_rank, status, ap = h["first_rank"].copy(), h["status"].copy(), h["ap"].copy()
                if return_details:
                    for q in range(Q):
                        ok = int(status[q]) == 0
                        details.append({"query": [int(x) for x in ids[q]],
                                        "words": ["?" if x < 0 else self.reverse_vocab.get(int(x), "UNK") for x in ids[q]],
                                        "top": [{"image": items[int(i)][0], "score": float(s)}
                                                for i, s in zip(h["idx"][q, :top_w], h["scores"][q, :top_w])],
                                        "first_rank": int(first_rank[q]) if ok else None, "ap": float(ap[q]) if ok else None})
            summ = retrmod.summarise(first_rank, ap, status, ks)      # (raises on a status other than 0 / -3: a refused list is a bug)
            res = {"retrieval": {k: v for k, v in summ.items() if k not in ("n_valid", "n_without_relevant")},
                   "ks": list(ks), "n_queries": Q, "n_images": n_img, "n_samples": N, "n_without_relevant": summ["n_without_relevant"],
                   "n_out_of_vocab": len(cq["rejected"]), "generator_weights": weights, "decode": "likelihood"}
            if return_details:
                res["details"] = details
            if self.rank == 0 and out_path:
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
            return res

    ############################################################
    ## Predicate classification: predicates ranked per entity pair (csrc/predcls.hip, sgg_amd/predcls.py)
    ############################################################
    def predcls(self, items=None, max_images=None, ks=(20, 50, 100), n_samples=None, pairs="all", score="joint", train_triples=None,
                return_details=False, out_path=None, logits_budget_bytes=DEFAULT_LOGITS_BUDGET_BYTES):
        """The PredCls protocol of the scene-graph literature: the ENTITIES of an image are given (the distinct subject / object words
        of its true triples), the model says which ordered pairs are related and by which predicate.  Every candidate (s, v, o) is
        scored exactly by the likelihood of likelihood() / retrieve() - the mixture over the image's n_samples noise draws (default
        TEST_BATCH_MULTIPLIER x TEST_BATCH_SIZE) - for ALL V predicates of every candidate pair; sgg_amd/predcls.py has the
        definitions.  The critic is not run.

        items, train_triples: as evaluate().  pairs: "all" (every ordered pair of two different entities plus the true self pairs) or
        "gt" (the true pairs only: predicate detection).  score: "joint" (log p(s, v, o | image): the exact ranking of the mixture
        over the candidates) or "conditional" (log p(v | s, o, image), the literature's score).  ks: at most 1024.

        Schedule: the passes and the noise stream of likelihood().  Per batch one copy to the device (pairs, counts, the padded
        ground truth, each true triple's pair index and predicate); K.softmax_xent (lse only); per chunk of pairs - the joint
        buffer [nb, Pc, V] stays within a quarter of the logits budget - K.pair_predicate_logp and K.predcls_pair_topk; then
        K.predcls_merge and K.match_triples once per constraint mode (one predicate per pair / up to predicates_per_pair =
        min(128, V, max(ks)) of them: exact while max(ks) <= 128), and one copy back.

        Returns (rank 0 writes it as JSON to out_path): graph_constraint and no_graph_constraint (each a RecallAccumulator.result():
        R@K, mR@K, zsR@K), predicate_given_pair (top1, top5, mean_rank and mean_predicate_top1 of the true predicate among all V
        predicates of its own pair, over the distinct valid true triples), ks, pairs, score, samples_per_image, predicates_per_pair,
        mean_pairs_per_image, n_images_truncated (images with more than 4096 candidate pairs: the true pairs are kept),
        generator_weights, definition and, with return_details, details: per image {"image", "n_pairs", "gt_rank", and per mode
        "triples", "scores", "pos", "n_gt", "n_candidates"}.  A ground-truth list of more than 4096 triples or a token outside the
        vocabulary raises ValueError before anything is launched.  Touches no weights and no optimiser state."""
        pclsmod.check_args(pairs, score)
        with self._eval_weights() as weights:
            ks = tuple(sorted(set(int(k) for k in ks)))
            if not ks or ks[0] < 1 or ks[-1] > pclsmod.MAX_K:
                raise ValueError("predcls: ks must be integers in 1..%d (got %r)" % (pclsmod.MAX_K, ks))
            items = self._evaluate_items(items, max_images)
            V = len(self.vocab)
            for key, _, real in items:
                if len(real) > MAX_GT:
                    raise ValueError("predcls: image %s has %d ground-truth triples (at most %d per image)" % (key, len(real), MAX_GT))
                for t in real:
                    if len(t) != 3 or not all(0 <= x < V for x in t):
                        raise ValueError("predcls: image %s: ground-truth triple %r is not three tokens in [0, %d)" % (key, list(t), V))
            if train_triples is None and self.dataset is not None:
                train_triples = set(map(tuple, np.concatenate([self.dataset["train"][1], self.dataset["val"][1]]).tolist()))
            K, V, TB, N, _ = self._sampling_setup("predcls", n_samples, None)
            modes = ("graph_constraint", "no_graph_constraint")
            acc = {mode: RecallAccumulator(ks, V) for mode in modes}
            pacc = pclsmod.PredicateAccumulator(V)
            top_k, Kc = max(ks), min(pclsmod.MAX_KC, V, max(ks))
            cand = [pclsmod.candidate_pairs(real, pairs) for _, _, real in items]
            details = []
            if items:
                need_kernels(K, "predcls", "pair_predicate_logp", "predcls_pair_topk", "predcls_merge", "match_triples")
                dev = self.device
                nb = images_per_pass(N, V, TB, len(items), logits_budget_bytes)
                M = max(1, max(len(real) for _, _, real in items))
                P = max(1, max(len(c) for c, _ in cand))
                Pc, n_chunks = pclsmod.pair_chunk(P, nb, V, logits_budget_bytes)
                Pp = Pc * n_chunks                              # (the pairs behind an image's count are padding: status -3)
                per_pair = {"graph_constraint": 1, "no_graph_constraint": Kc}
                in_parts = [("gt", np.int64, (nb, M, 3)), ("pairs", np.int32, (nb, Pp, 2)), ("pairs_c", np.int32, (n_chunks, nb, Pc, 2)),
                            ("count_c", np.int32, (n_chunks, nb)), ("gt_count", np.int32, (nb,)),
                            ("gt_pair_c", np.int32, (n_chunks, nb, M)), ("gt_pred", np.int32, (nb, M))]
                in_host, _, in_views = self._device_pack(in_parts, "cpu")
                h_in = in_views(in_host.numpy())                # (numpy views of the host buffer: filled in place)
                in_packed, d_in, _ = self._device_pack(in_parts, dev)
                back_parts = [("gt_rank", np.int32, (nb, M))]
                for mode in modes:
                    back_parts += [(mode + "/triples", np.int64, (nb, top_k, 3)), (mode + "/scores", np.float32, (nb, top_k)),
                                   (mode + "/src", np.int32, (nb, top_k)), (mode + "/n_distinct", np.int32, (nb,)),
                                   (mode + "/pos", np.int32, (nb, M)), (mode + "/n_gt", np.int32, (nb,))]
                packed, back, views = self._device_pack(back_parts, dev)
                joint = torch.empty((nb, Pc, V), dtype=torch.float32, device=dev)
                full = {"marg": torch.empty((nb, Pp), dtype=torch.float32, device=dev),
                        "top_tok": torch.empty((nb, Pp, Kc), dtype=torch.int32, device=dev),
                        "top_score": torch.empty((nb, Pp, Kc), dtype=torch.float32, device=dev)}
                status = torch.empty((nb, Pc), dtype=torch.int32, device=dev)
                part = full if n_chunks == 1 else {"marg": torch.empty((nb, Pc), dtype=torch.float32, device=dev),
                                                   "top_tok": torch.empty((nb, Pc, Kc), dtype=torch.int32, device=dev),
                                                   "top_score": torch.empty((nb, Pc, Kc), dtype=torch.float32, device=dev),
                                                   "gt_rank": torch.empty((nb, M), dtype=torch.int32, device=dev)}
                lse = torch.empty((N, nb, 3), dtype=torch.float32, device=dev)
                with contextlib.closing(self._sample_batches([(key, x) for key, x, _ in items], N, nb)) as batches:
                    for i0, n, images, logits in batches:
                        for a in h_in.values():
                            a[...] = 0
                        h_in["gt_pair_c"][...] = -1             # (the padded images of the last batch: no pairs, no ground truth)
                        for j in range(n):
                            real, (pr, _) = items[i0 + j][2], cand[i0 + j]
                            if not len(real):
                                continue
                            g = np.asarray(real, dtype=np.int64).reshape(-1, 3)
                            h_in["gt"][j, :len(g)] = g
                            h_in["gt_count"][j] = len(g)
                            h_in["gt_pred"][j, :len(g)] = g[:, 1]
                            h_in["pairs"][j, :len(pr)] = pr
                            where = pclsmod.gt_pair_index(pr, real)
                            for c in range(n_chunks):
                                own = pr[c * Pc:(c + 1) * Pc]
                                h_in["pairs_c"][c, j, :len(own)] = own
                                h_in["count_c"][c, j] = len(own)
                                h_in["gt_pair_c"][c, j, :len(g)] = np.where((where >= c * Pc) & (where < (c + 1) * Pc), where - c * Pc, -1)
                        in_packed.copy_(in_host)
                        K.softmax_xent(logits, None, lse=lse.view(-1))
                        for c in range(n_chunks):
                            K.pair_predicate_logp(logits, lse, d_in["pairs_c"][c], d_in["count_c"][c], joint=joint,
                                                  out={"marg": part["marg"], "status": status})
                            K.predcls_pair_topk(joint, status, Kc, d_in["gt_pair_c"][c], d_in["gt_pred"],
                                                out={"top_tok": part["top_tok"], "top_score": part["top_score"],
                                                     "gt_rank": back["gt_rank"] if n_chunks == 1 else part["gt_rank"]})
                            if n_chunks > 1:                    # (a true triple's pair lies in one chunk: the others report rank 0)
                                for name in full:
                                    full[name][:, c * Pc:(c + 1) * Pc].copy_(part[name])
                                if c == 0:
                                    back["gt_rank"].copy_(part["gt_rank"])
                                else:
                                    back["gt_rank"].add_(part["gt_rank"])
                        for mode in modes:
                            out = {name: back[mode + "/" + name] for name in ("triples", "scores", "src", "n_distinct")}
                            K.predcls_merge(d_in["pairs"], full["top_tok"], full["top_score"], full["marg"], top_k,
                                            per_pair=per_pair[mode], conditional=score == "conditional", out=out)
                            K.match_triples(out["triples"], out["n_distinct"], d_in["gt"], d_in["gt_count"], vocab=V,
                                            out={"pos": back[mode + "/pos"], "n_gt": back[mode + "/n_gt"]})
                        h = views(packed.cpu().numpy())
                        for j in range(n):
                            key, _, real = items[i0 + j]
                            zs = None if train_triples is None else zero_shot_mask(real, train_triples)
                            rank = h["gt_rank"][j, :len(real)].copy()
                            for mode in modes:
                                acc[mode].add(h[mode + "/pos"][j, :len(real)], real, zs)
                            keep = h[modes[0] + "/pos"][j, :len(real)] >= -1       # (the distinct valid true triples, as R@K counts them)
                            pacc.add(rank[keep], np.asarray(real, dtype=np.int64).reshape(-1, 3)[keep])
                            if return_details:
                                d = {"image": key, "n_pairs": int(len(cand[i0 + j][0])), "gt_rank": rank.tolist()}
                                for mode in modes:
                                    u = min(int(h[mode + "/n_distinct"][j]), top_k)
                                    d[mode] = {"triples": h[mode + "/triples"][j, :u].tolist(),
                                               "scores": [float(s) for s in h[mode + "/scores"][j, :u]],
                                               "pos": h[mode + "/pos"][j, :len(real)].tolist(), "n_gt": int(h[mode + "/n_gt"][j]),
                                               "n_candidates": int(h[mode + "/n_distinct"][j])}
                                details.append(d)
            res = {mode: acc[mode].result(self.reverse_vocab) for mode in modes}
            res.update({"predicate_given_pair": pacc.result(), "ks": list(ks), "pairs": pairs, "score": score, "samples_per_image": N,
                        "predicates_per_pair": Kc,
                        "mean_pairs_per_image": float(np.mean([len(c) for c, _ in cand])) if cand else None,
                        "n_images_truncated": int(sum(t for _, t in cand)), "generator_weights": weights,
                        "definition": pclsmod.DEFINITION})
            if return_details:
                res["details"] = details
            if self.rank == 0 and out_path:
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
            return res


def _str2bool(v):
    """--resume of the reference is `type=bool` (train.py:410), which makes every non-empty string - "False" included - true."""
    if isinstance(v, bool):
        return v
    if str(v).strip().lower() in ("1", "true", "t", "yes", "y", "on"):
        return True
    if str(v).strip().lower() in ("0", "false", "f", "no", "n", "off", ""):
        return False
    raise argparse.ArgumentTypeError("expected a boolean, got %r" % (v,))


def _clip_arg(text):
    try:
        return guardmod.parse_clip_grad_norm(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--checkpoints_dir", help="Where to save the checkpoints", default="./checkpoints")
    parser.add_argument("--summaries_dir", help="Where to write the logs", default="./logs")
    parser.add_argument("--path_to_ims_to_triples", default="./dataset_creation/ims_to_triples.json")
    parser.add_argument("--path_to_vocab", default="./dataset_creation/vocab.json")
    parser.add_argument("--path_to_word_embeddings", default="./dataset_creation/word_embeddings.npy")
    parser.add_argument("--path_to_image_means", default="./dataset_creation/image_means.txt")
    parser.add_argument("--path_to_image_stds", default="./dataset_creation/image_stds.txt")
    parser.add_argument("--batch_size", default=64, help="Batch size defaults", type=int)
    parser.add_argument("--critic_iters", default=10, help="Number of critic iterations per generator iteration", type=int)
    parser.add_argument("--lambda", default=10, help="WGAN Lipschitz Penalty", type=float)
    parser.add_argument("--resume", default=False, nargs="?", const=True, type=_str2bool,
                        help="Resume from the last checkpoint (--resume, --resume True, --resume False)")
    parser.add_argument("--GPU", default="0", help="Which GPU to use (single-process runs)")
    parser.add_argument("--synthetic", default=None, help="B,S,V: train on synthetic tensors of that shape (no dataset files)")
    parser.add_argument("--max_iterations", default=None, type=int)
    parser.add_argument("--single_stream", action="store_true", help="serial launch order (default: two HIP streams)")
    parser.add_argument("--no_shuffle_buffer", action="store_true", help="walk the shuffled example list in order (default: through the "
                                                                         "reference's rolling shuffle buffer of 10 batches, train.py:178)")
    parser.add_argument("--validate_every", default=None, type=int, help="iterations between validation-loss checks (default: "
                                                                         "len(train) / 50 on real data as train.py:162, off with --synthetic)")
    parser.add_argument("--recompute_generator_encoder", action="store_true",
                        help="run G's encoder in every update like the reference graph (default: once per iteration, same result)")
    parser.add_argument("--test_only", action="store_true",
                        help="load the checkpoint in --checkpoints_dir, compute R@50 / R@100 (recalls.txt) and exit; no training")
    parser.add_argument("--max_test_images", default=None, type=int, help="evaluate the first N test images only")
    parser.add_argument("--saliency_dir", default=None,
                        help="load the checkpoint in --checkpoints_dir, write per-word saliency maps of the test images (one .npz per "
                             "image + index.json) to this directory and exit; no training")
    parser.add_argument("--predict_dir", default=None,
                        help="load the checkpoint in --checkpoints_dir, write the ranked scene graph of the test images (one .npz per "
                             "image + index.json) to this directory and exit; no training")
    parser.add_argument("--predict_samples", default=None, type=int,
                        help="generator samples per image for --predict_dir / --metrics_out (default: 8 x the test batch size, as the evaluation)")
    parser.add_argument("--top_k", default=None, type=int, help="keep the first K distinct triples per image (default: all)")
    parser.add_argument("--predict_descending", action="store_true",
                        help="highest critic score first (default: ascending, the order of the evaluation)")
    parser.add_argument("--decode", default="samples", choices=kbestmod.DECODES,
                        help="how --predict_dir / --metrics_out draw an image's candidate triples: samples = the argmax triple of each "
                             "noise sample, ranked by critic score (the default); kbest = the K most probable triples of each sample's "
                             "three softmaxes, merged and ranked by the generator's log-probability, no critic pass (--predict_samples "
                             "then defaults to the test batch size; not with --predict_descending)")
    parser.add_argument("--ground", action="store_true",
                        help="with --predict_dir: resolve the subjects and objects of the ranked triples to entity instances from the "
                             "generator's pooled attention (nodes with boxes and centres; \"grounded_graph\" in index.json)")
    parser.add_argument("--ground_overlap", default=groundmod.DEFAULT_OVERLAP, type=float,
                        help="with --ground: two mentions of one word are one entity when their pooled attention maps overlap by at "
                             "least this much, in (0, 1] (default 0.5; untuned)")
    parser.add_argument("--ground_box_frac", default=groundmod.DEFAULT_BOX_FRAC, type=float,
                        help="with --ground: an entity's box holds every cell at or above this fraction of its map's maximum, in "
                             "(0, 1] (default 0.5; untuned)")
    parser.add_argument("--metrics_out", default=None,
                        help="load the checkpoint in --checkpoints_dir, write R@K, mR@K and zsR@K of the test images (distinct "
                             "predictions, denominators |GT|) as JSON to this file and exit; no training")
    parser.add_argument("--metrics_k", default="20,50,100", help="the K values of --metrics_out, comma-separated")
    parser.add_argument("--predcls_out", default=None,
                        help="load the checkpoint in --checkpoints_dir, write predicate classification (PredCls: the entities of an "
                             "image given, predicates ranked per entity pair by the generator's likelihood; R@K, mR@K, zsR@K with and "
                             "without the graph constraint, predicate accuracy given the true pair) of the test images as JSON to this "
                             "file and exit; no training (--max_test_images, --predict_samples and --eval_live apply)")
    parser.add_argument("--predcls_k", default=None, help="with --predcls_out: the K values, comma-separated in 1..1024 (default 20,50,100)")
    parser.add_argument("--predcls_pairs", default=None, choices=pclsmod.PAIR_MODES,
                        help="with --predcls_out: all = every ordered pair of two different entities (default); gt = the true pairs only")
    parser.add_argument("--predcls_score", default=None, choices=pclsmod.SCORES,
                        help="with --predcls_out: joint = log p(s, v, o | image) (default); conditional = log p(v | s, o, image)")
    parser.add_argument("--diagnostics_every", default=0, type=int,
                        help="every N iterations, report per-tensor gradient / parameter / update norms and non-finite counts of both "
                             "networks and the critic's gradient-penalty slopes: summary under \"diag\" in losses.jsonl, per-tensor table in "
                             "<summaries_dir>/diagnostics.jsonl (default 0: off, nothing is launched; read-only when on)")
    parser.add_argument("--halt_on_nonfinite", action="store_true",
                        help="with --diagnostics_every: stop with NonFiniteError (network, tensor, gradient / parameter / update) on "
                             "the first reported iteration that counts an Inf or NaN; no checkpoint is written on the way out, so the "
                             "last good one in --checkpoints_dir survives")
    parser.add_argument("--ema_decay", default=0.0, type=float,
                        help="D in (0, 1): keep an exponential moving average of the generator's weights (decay min(D, (1 + k) / (10 + k)) "
                             "at its k-th update, as tf.train.ExponentialMovingAverage), updated inside the generator's optimiser pass "
                             "and saved in the checkpoint; evaluation (the test after training, --test_only, --saliency_dir, "
                             "--predict_dir, --metrics_out) then runs the generator on the average (default 0: off)")
    parser.add_argument("--accumulate", default=1, type=int,
                        help="N >= 1: take every optimiser step from N micro-batches of --batch_size rows (gradients summed on the "
                             "device, scaled by 1 / N inside the Adam pass): the update of N x batch_size rows per GPU; iteration "
                             "i reads micro-batches i * N .. i * N + N - 1 of the example stream (default 1: off)")
    parser.add_argument("--clip_grad_norm", default=(0.0, 0.0), type=_clip_arg, metavar="X[,Y]",
                        help="clip every update to this global gradient norm (the gradient is scaled by X / norm where its norm "
                             "exceeds X; decided on the device inside the optimiser step): one number applies to both networks, two "
                             "are the critic's, then the generator's; 0 means off (default 0)")
    parser.add_argument("--skip_nonfinite", action="store_true",
                        help="drop an update whose gradient holds an Inf or NaN: parameters, Adam moments and the weight average keep "
                             "every bit (decided on the device; the step count still advances); the counts of clipped and skipped "
                             "updates are logged under \"guard\" in losses.jsonl and saved in the checkpoint")
    parser.add_argument("--pretrain_iterations", default=0, type=int,
                        help="P >= 0: the first P iterations of the run (itr < P; --max_iterations is the total) are maximum-likelihood "
                             "updates of the generator on the minibatch's true triples - softmax cross-entropy over its three decoder "
                             "outputs, one fresh noise draw per (micro-)batch, no critic update; its Adam state carries over into the "
                             "GAN phase; the checkpoint then also holds \"pretrain_iterations\" and, in a single-process run, the "
                             "noise generator's state (\"noise_rng\"), so that a stopped and resumed run ends on the same weights - "
                             "with several ranks a resumed run restarts its noise streams (default 0: off)")
    parser.add_argument("--mle_weight", default=0.0, type=float,
                        help="W >= 0: add W x the same cross-entropy to the generator's cost in the GAN phase; losses.jsonl then also "
                             "carries mle_nll_token / mle_nll_triple / mle_token_acc / mle_triple_acc (default 0: off, nothing is launched)")
    parser.add_argument("--validate_nll", action="store_true",
                        help="whenever validation runs, also log the held-out negative log-likelihood of the validation batch's true "
                             "tokens under the generator (val_nll_token, val_token_acc, val_triple_acc); its noise comes from a "
                             "generator of its own, so val_disc_loss keeps its bits")
    parser.add_argument("--generator_output", default=None, choices=list(RELAX_MODES),
                        help="what the critic is shown of the generator's decoder rows x: logits = x itself; softmax = "
                             "y = softmax(x / tau); gumbel = y = softmax((x + g) / tau) with Gumbel noise g drawn on the device from "
                             "--seed, the rank and (iteration, update, micro-batch).  The generator's update differentiates through y.  "
                             "The checkpoint records the mode; a resumed run and every evaluation mode take it from there (where "
                             "the critic scores softmax(x / tau) without noise), and a flag that contradicts it is an error "
                             "(default: logits for a fresh run)")
    parser.add_argument("--relax_hard", action="store_true",
                        help="with --generator_output softmax|gumbel: the straight-through estimator - the critic is shown "
                             "onehot(argmax(x + g)) in both updates and the generator's update takes the gradient of the soft row, rebuilt "
                             "from the logits and the same noise.  Recorded in the checkpoint and taken from there on --resume and at "
                             "evaluation, where the critic scores onehot(argmax(x)): the row of the reported token")
    parser.add_argument("--generator_gradient", default=None, choices=list(GRADIENTS),
                        help="how the generator's update gets its gradient: pathwise = through the critic's gradient of its input; "
                             "score = the score-function (REINFORCE) estimator on triples sampled from softmax(x) - unbiased, no "
                             "gradient through the critic.  score implies --generator_output gumbel --relax_hard and takes no "
                             "--relax_tau.  Recorded in the checkpoint and taken from there on --resume and at evaluation "
                             "(default: pathwise for a fresh run)")
    parser.add_argument("--score_baseline", default=None, choices=list(SCORE_BASELINES),
                        help="with --generator_gradient score: rloo = each sample's reward minus the mean reward of the other samples "
                             "of its (micro-)batch; none = the reward itself; image (needs --score_samples >= 2) = minus the mean "
                             "reward of the other samples of the same image (default rloo; image with --score_samples >= 2)")
    parser.add_argument("--score_samples", default=None, type=int, metavar="S",
                        help="with --generator_gradient score: S in 1..16 triples are sampled per image in the generator's update "
                             "from one set of logits, the critic's head scores all S x batch of them against the batch's feature "
                             "maps; the encoders run once either way.  The critic's updates keep one sample.  Recorded in the "
                             "checkpoint when S > 1 (default 1)")
    parser.add_argument("--entropy_weight", default=None, type=float, metavar="W",
                        help="with --generator_gradient score: W >= 0 adds W x the mean entropy of the decoder rows to what the "
                             "generator maximises (default 0)")
    parser.add_argument("--seed", default=0, type=int,
                        help="the run's seed: the example stream, the noise streams and the Gumbel noise's key derive from it (default 0)")
    parser.add_argument("--augment", default=None, metavar="SPEC",
                        help="training-time augmentation of the real-data batches, drawn and applied on the device inside the input "
                             "kernel: crop=LO (smallest side fraction of a random crop box, (0, 1]), flip=P (mirror with probability P; "
                             "left / right words of the triple are exchanged), brightness=A, contrast=A, saturation=A (factor in "
                             "[1 - A, 1 + A], A in [0, 1)), comma-separated, e.g. crop=0.5,flip=0.5,brightness=0.2,contrast=0.2,"
                             "saturation=0.2.  Validation and evaluation never augment.  Stored in the checkpoint: --resume continues "
                             "with it, a contradicting flag is an error.  Not with --synthetic (default: off)")
    parser.add_argument("--relax_tau", default=None, metavar="T | T0,T1,N",
                        help="the relaxation's temperature: a constant T, or the schedule tau(it) = T0 (T1 / T0)^(min(it, N) / N) "
                             "(default 1)")
    parser.add_argument("--likelihood_out", default=None,
                        help="load the checkpoint in --checkpoints_dir, write the negative log-likelihood of the test images' true "
                             "triples under the generator (mixture over --predict_samples noise draws, per draw, per slot; token "
                             "perplexity) as JSON to this file and exit; no training")
    parser.add_argument("--retrieve_out", default=None,
                        help="load the checkpoint in --checkpoints_dir, rank the test images for a list of triple queries by the "
                             "generator's likelihood (mixture over --predict_samples noise draws), write R@K, median rank, MRR and mAP "
                             "as JSON to this file and exit; no training")
    parser.add_argument("--retrieve_queries", default=None,
                        help="with --retrieve_out: a JSON file holding a list of triples as words or token ids, \"?\" or null for an "
                             "open slot (default: the distinct true triples of the evaluated images, most frequent first)")
    parser.add_argument("--retrieve_top", default=None, type=int,
                        help="with --retrieve_out: the JSON lists the first K images of every query (1..1024; default 10)")
    parser.add_argument("--retrieve_max_queries", default=None, type=int,
                        help="with --retrieve_out: score at most Q queries (default 4096)")
    parser.add_argument("--log_every", default=10, type=int, help="iterations between the loss records of losses.jsonl (default 10)")
    parser.add_argument("--eval_live", action="store_true",
                        help="evaluate the generator's live weights even where an average exists (from --ema_decay or the checkpoint)")
    return parser


def parse_args(argv=None):
    """The command line, with the combinations no single option can reject."""
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        kbestmod.check_decode(args.decode, args.predict_descending)
    except ValueError as e:
        parser.error(str(e))
    if args.ground:
        if not args.predict_dir:
            parser.error("--ground needs --predict_dir")
        try:
            groundmod.check_ground_args(args.ground_overlap, args.ground_box_frac, args.top_k)
        except ValueError as e:
            parser.error(str(e))
    for flag in ("retrieve_queries", "retrieve_top", "retrieve_max_queries"):
        if getattr(args, flag) is not None and not args.retrieve_out:
            parser.error("--%s needs --retrieve_out" % flag)
    if args.retrieve_out:
        for flag in ("likelihood_out", "saliency_dir", "predict_dir", "metrics_out", "test_only"):
            if getattr(args, flag):
                parser.error("--retrieve_out is a run of its own: not together with --%s" % flag)
    for flag in ("predcls_k", "predcls_pairs", "predcls_score"):
        if getattr(args, flag) is not None and not args.predcls_out:
            parser.error("--%s needs --predcls_out" % flag)
    if args.predcls_out:
        for flag in ("retrieve_out", "likelihood_out", "saliency_dir", "predict_dir", "metrics_out", "test_only"):
            if getattr(args, flag):
                parser.error("--predcls_out is a run of its own: not together with --%s" % flag)
        try:
            args.predcls_k = tuple(int(k) for k in (args.predcls_k or "20,50,100").split(",") if k.strip())
        except ValueError:
            parser.error("--predcls_k must be comma-separated integers (got %r)" % args.predcls_k)
        if not args.predcls_k or min(args.predcls_k) < 1 or max(args.predcls_k) > pclsmod.MAX_K:
            parser.error("--predcls_k must be integers in 1..%d" % pclsmod.MAX_K)
    if args.retrieve_top is not None and not 1 <= args.retrieve_top <= retrmod.MAX_TOP:
        parser.error("--retrieve_top must be in 1..%d" % retrmod.MAX_TOP)
    if args.retrieve_max_queries is not None and args.retrieve_max_queries < 1:
        parser.error("--retrieve_max_queries must be >= 1")
    if args.pretrain_iterations < 0:
        parser.error("--pretrain_iterations must be >= 0")
    if not (0.0 <= args.mle_weight < float("inf")):
        parser.error("--mle_weight must be a finite number >= 0")
    if args.relax_hard and args.generator_output == "logits":
        parser.error("--relax_hard needs --generator_output softmax or gumbel")
    try:
        check_score_flags(args.generator_gradient, args.score_baseline, args.entropy_weight, args.generator_output, args.relax_tau,
                          args.score_samples)
    except ValueError as e:
        parser.error("--" + str(e))
    if args.generator_gradient == "score":
        args.generator_output, args.relax_hard = "gumbel", True
    if args.augment is not None:
        if args.synthetic:
            parser.error("--augment works on decoded source pixels: not together with --synthetic")
        try:
            AugmentSpec.parse(args.augment)
        except ValueError as e:
            parser.error("--" + str(e))
    if args.relax_tau is not None:
        try:
            args.relax_tau = parse_relax_tau(args.relax_tau)
        except ValueError as e:
            parser.error("--" + str(e))
    return args


if __name__ == "__main__":
    args = parse_args()
    params = vars(args)

    if "LOCAL_RANK" not in os.environ:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", "{}".format(params["GPU"]))
    synthetic = tuple(int(x) for x in params["synthetic"].split(",")) if params["synthetic"] else None
    gan = SceneGraphGAN(checkpoints_dir=params["checkpoints_dir"], summaries_dir=params["summaries_dir"],
                        path_to_ims_to_triples=params["path_to_ims_to_triples"], path_to_vocab=params["path_to_vocab"],
                        path_to_word_embeddings=params["path_to_word_embeddings"],
                        path_to_image_means=params["path_to_image_means"], path_to_image_stds=params["path_to_image_stds"],
                        critic_iters=params["critic_iters"], batch_size=params["batch_size"], lambda_=params["lambda"],
                        resume=params["resume"], synthetic=synthetic, two_streams=not params["single_stream"],
                        reuse_g_encoder=not params["recompute_generator_encoder"], shuffle_buffer=not params["no_shuffle_buffer"],
                        ema_decay=params["ema_decay"], eval_live=params["eval_live"], accumulate=params["accumulate"],
                        clip_grad_norm=params["clip_grad_norm"], skip_nonfinite=params["skip_nonfinite"],
                        pretrain_iterations=params["pretrain_iterations"], mle_weight=params["mle_weight"],
                        validate_nll=params["validate_nll"], generator_output=params["generator_output"],
                        relax_tau=params["relax_tau"], relax_hard=params["relax_hard"], seed=params["seed"],
                        generator_gradient=params["generator_gradient"], score_baseline=params["score_baseline"],
                        entropy_weight=params["entropy_weight"], score_samples=params["score_samples"], augment=params["augment"])
    if params["retrieve_out"]:
        if not gan.load_checkpoint():
            print("--retrieve_out: no checkpoint at %s (train first, or pass the run's --checkpoints_dir)" % gan._ckpt_path(),
                  file=sys.stderr)
            sys.exit(2)
        queries = None
        if params["retrieve_queries"]:
            with open(params["retrieve_queries"]) as f:
                queries = json.load(f)
        res = gan.retrieve(queries=queries, max_images=params["max_test_images"], n_samples=params["predict_samples"],
                           top_k=params["retrieve_top"] or 10, max_queries=params["retrieve_max_queries"] or retrmod.MAX_QUERIES,
                           return_details=True, out_path=params["retrieve_out"])
        if gan.rank == 0:
            print({k: v for k, v in res.items() if k != "details"})
    elif params["predcls_out"]:
        if not gan.load_checkpoint():
            print("--predcls_out: no checkpoint at %s (train first, or pass the run's --checkpoints_dir)" % gan._ckpt_path(),
                  file=sys.stderr)
            sys.exit(2)
        res = gan.predcls(max_images=params["max_test_images"], ks=params["predcls_k"], n_samples=params["predict_samples"],
                          pairs=params["predcls_pairs"] or "all", score=params["predcls_score"] or "joint", return_details=True,
                          out_path=params["predcls_out"])
        if gan.rank == 0:
            print({k: ({a: b for a, b in v.items() if a != "predicates"} if isinstance(v, dict) else v)
                   for k, v in res.items() if k not in ("details", "definition")})
    elif params["likelihood_out"]:
        if not gan.load_checkpoint():
            print("--likelihood_out: no checkpoint at %s (train first, or pass the run's --checkpoints_dir)" % gan._ckpt_path(),
                  file=sys.stderr)
            sys.exit(2)
        res = gan.likelihood(max_images=params["max_test_images"], n_samples=params["predict_samples"], out_path=params["likelihood_out"])
        if gan.rank == 0:
            print(res)
    elif params["saliency_dir"]:
        if not gan.load_checkpoint():
            print("--saliency_dir: no checkpoint at %s (train first, or pass the run's --checkpoints_dir)" % gan._ckpt_path(),
                  file=sys.stderr)
            sys.exit(2)
        gan.write_saliency(params["saliency_dir"], max_images=params["max_test_images"])
    elif params["predict_dir"]:
        if not gan.load_checkpoint():
            print("--predict_dir: no checkpoint at %s (train first, or pass the run's --checkpoints_dir)" % gan._ckpt_path(),
                  file=sys.stderr)
            sys.exit(2)
        gan.write_predictions(params["predict_dir"], max_images=params["max_test_images"], n_samples=params["predict_samples"],
                              top_k=params["top_k"], descending=params["predict_descending"], decode=params["decode"],
                              ground=params["ground"], ground_overlap=params["ground_overlap"],
                              ground_box_frac=params["ground_box_frac"])
    elif params["metrics_out"]:
        if not gan.load_checkpoint():
            print("--metrics_out: no checkpoint at %s (train first, or pass the run's --checkpoints_dir)" % gan._ckpt_path(),
                  file=sys.stderr)
            sys.exit(2)
        m = gan.evaluate(max_images=params["max_test_images"], ks=tuple(int(k) for k in params["metrics_k"].split(",") if k.strip()),
                         n_samples=params["predict_samples"], descending=params["predict_descending"], out_path=params["metrics_out"],
                         decode=params["decode"])
        if gan.rank == 0:
            print({k: v for k, v in m.items() if k != "predicates" and k != "definition"})
    elif params["test_only"]:
        if not gan.load_checkpoint():
            print("--test_only: no checkpoint at %s (train first, or pass the run's --checkpoints_dir)" % gan._ckpt_path(),
                  file=sys.stderr)
            sys.exit(2)
        gan.test(max_images=params["max_test_images"])
    else:
        gan.train(max_iterations=params["max_iterations"], log_every=max(1, params["log_every"]), validate_every=params["validate_every"],
                  test_max_images=params["max_test_images"], diagnostics_every=params["diagnostics_every"],
                  halt_on_nonfinite=params["halt_on_nonfinite"])
