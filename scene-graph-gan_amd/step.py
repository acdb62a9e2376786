"""WGAN-GP critic step and generator step (one "G+D step" = critic_iters critic updates + one generator update).

Reference: train.py:239-266 (tfgan gan_model / gan_loss with wasserstein losses + one-sided gradient penalty,
two Adam optimisers, variable partition by name prefix) and the loop body train.py:362-368.

Critic step:   G forward (fake logits, constant for D) -> D encoder forward ONCE (fake / real / interpolated share
               the images) -> critic head on the 3B-row super-batch -> first-order backward (parameter gradients
               from the fake and real rows; g = d sum(D(x_hat)) / d x_hat from the interpolated rows) -> penalty
               and v = lambda * dGP/dg -> dual-number head pass on the interpolated rows (JVP along v, then the same
               backward evaluated on duals = gradient of the penalty) -> encoder backward -> [all-reduce] -> TF-Adam.
Generator step: G forward -> D forward with the updated critic -> backward through the critic head to the fake
               logits -> generator head + encoder backward -> [all-reduce] -> TF-Adam.
No autograd tape is used anywhere in this path; every arithmetic op is a HIP kernel behind the C ABI.
"""
from __future__ import annotations

import math

import contextlib
from collections import OrderedDict

import torch

from . import diagnostics, ema
from . import guard as guardmod
from .head import Head
from .lib import option
from .params import ADAM_B1, ADAM_B2, ADAM_EPS, ADAM_LR, EMBED_DIM, FEAT_C, NUM_UNITS, T_STEPS, ParamArena, tf_variable_name
from .trunk import Trunk


def tf_adam_lr_t(t, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2):
    """tf.train.AdamOptimizer: lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)."""
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def need_kernels(K, what, *kernels):
    """`what` needs these methods of the kernel set K.  A set without one of them (the CPU reference kernels, a stub in a test) is
    refused by name: an error before anything is launched, never a fall-back."""
    missing = [n for n in kernels if not hasattr(K, n)]
    if missing:
        raise RuntimeError("%s needs the kernels %s; the %r kernel set lacks %s"
                           % (what, ", ".join(kernels), getattr(K, "name", K), ", ".join(missing)))


class Network:
    """Parameters (+ gradient / Adam arenas), encoder and head of one network for ONE batch size.

    share=<Network>: the variables of the reference graph exist once however many times build_* runs (tf.AUTO_REUSE, train.py:86,91;
    the graph is batch-dynamic: generator_with_attention.py:74-75 reshape to [-1, ...], train.py:29-30,199-203,297-298 feed B, B/2
    and B/2 x 8 rows through the same ops).  A Network built with `share` uses the other one's parameter, gradient and Adam arenas
    and optimiser step count, and owns only the activation buffers of its own batch size."""

    def __init__(self, K, kind, V, S, B, E=EMBED_DIM, device=None, dtype=torch.float32, state_dict=None, share=None):
        self.K, self.kind = K, kind
        device = device if device is not None else K.device
        if share is not None:
            assert state_dict is None and (share.kind, share.arena.V, share.arena.S, share.arena.E) == (kind, V, S, E)
            self.arena, self.grad_flat, self.grads = share.arena, share.grad_flat, share.grads
            self.m_flat, self.v_flat, self.opt = share.m_flat, share.v_flat, share.opt
        else:
            self.arena = ParamArena(kind, V, S, E, device=device, dtype=dtype)
            if state_dict is not None:
                self.arena.load_state_dict(state_dict)
            self.grad_flat, self.grads = self.arena.like()
            self.m_flat, _ = self.arena.like()
            self.v_flat, _ = self.arena.like()
            # t: Adam step count; pending: in-flight gradient all-reduce (dp.PendingReduce) whose Adam step is deferred
            self.opt = {"t": 0, "pending": None}
        self.trunk = Trunk(K, self.arena, self.grads, B, S)
        self.head = Head(K, kind, self.arena, self.grads, B, self.trunk.L)
        self.data_passes = 0                 # input-gradient passes on this network's buffers (sgg_amd/grad.py; GanStep._g_early_stream)

    adam_t = property(lambda self: self.opt["t"], lambda self, v: self.opt.__setitem__("t", v))
    pending = property(lambda self: self.opt["pending"], lambda self, v: self.opt.__setitem__("pending", v))

    def zero_grads(self):
        assert self.pending is None
        self.K.fill(self.arena.live(self.grad_flat), 0.0)

    def update(self, reducer, grad_scale=1.0):
        """Gradients are complete: start their all-reduce (if data parallel) and defer the Adam step until the
        weights are next needed (finish_update), so the collective overlaps with the other network's encoder.
        grad_scale: 1 / N after N accumulated micro-batches (end_micro_batch); multiplies the reducer's scale."""
        if reducer is None:
            self.adam_step(grad_scale)
        else:
            self.pending = reducer(self)
            if grad_scale != 1.0:
                self.opt["pending_scale"] = grad_scale

    def finish_update(self):
        if self.pending is not None:
            scale = self.pending.wait()
            self.pending = None
            extra = self.opt.pop("pending_scale", None)
            self.adam_step(scale if extra is None else scale * extra)

    # ---- gradient accumulation (csrc/optim.hip: grad_accumulate_kernel) ----------------------------------
    def _acc_flat(self):
        """The second gradient arena: allocated the first time an update spans more than one micro-batch, state of the ARENA."""
        acc = self.opt.get("acc")
        if acc is None:
            need_kernels(self.K, "gradient accumulation", "grad_accumulate")
            acc = self.opt["acc"] = self.arena.like()[0]
        return acc

    def end_micro_batch(self, k, N, reducer):
        """The gradients of micro-batch k of N are complete in grad_flat (every filter-gradient kernel overwrites its range, so each
        micro-step starts from zero_grads as a whole step does).  k < N - 1: they are added to the second arena (k = 0: copied) and
        nothing else happens - no optimiser step, no collective.  k = N - 1 > 0: the sum so far is added to grad_flat, which then
        holds the sum over all N, and update() runs with the gradient scale 1 / N: the reducer, both Adam passes and the statistics
        pass read the MEAN gradient, which is the gradient of the N * B rows (every loss term is a mean over rows, no op couples
        samples).  N = 1: update(reducer), call for call.  On the current stream, behind the step's last gradient kernel."""
        assert 0 <= k < N
        if N == 1:
            return self.update(reducer)
        a, acc = self.arena, self._acc_flat()
        if k < N - 1:
            self.K.grad_accumulate(a.live(acc), a.live(self.grad_flat), first=(k == 0))
            return
        self.K.grad_accumulate(a.live(self.grad_flat), a.live(acc))
        self.update(reducer, 1.0 / N)

    def adam_step(self, grad_scale=1.0):
        self._not_swapped("adam_step")
        self.adam_t += 1
        a = self.arena
        lr_t = tf_adam_lr_t(self.adam_t)
        # One Adam pass (csrc/optim.hip), K.adam[_ema][_guarded]: the same arithmetic with two optional operands.
        avg, gd = self.opt.get("ema"), self.opt.get("guard")
        arenas, scale, tail = [a.live(), a.live(self.grad_flat), a.live(self.m_flat), a.live(self.v_flat)], grad_scale, []
        if avg is not None:                  # the shadow update of the average in the same pass
            arenas.append(a.live(avg["flat"]))
            tail = [ema.one_minus_decay(avg["decay"], avg["updates"])]
        if gd is not None:                   # the decision on the device (csrc/guard.hip), then the pass reads its scale from the record
            self.K.grad_guard(a.live(self.grad_flat), gd["record"], grad_scale, gd["max_norm"], gd["skip_nonfinite"], ws=gd["ws"])
            scale = gd["record"]
        kernel = getattr(self.K, "adam" + ("_ema" if avg is not None else "") + ("_guarded" if gd is not None else ""))
        kernel(*arenas, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, scale, *tail)
        if avg is not None:
            avg["updates"] += 1              # (also for a step the guard dropped: the host does not know)
        if self.opt.get("armed"):            # diagnostics: one read-only pass directly behind the step, on its stream
            self.arena_stats(lr_t, grad_scale)
        a.version += 1                       # (encoders of other batch sizes on this arena re-derive their operand formats lazily)
        self.trunk.refresh_weights()

    # ---- guarded updates (sgg_amd/guard.py, csrc/guard.hip) -----------------------------------------------
    # opt["guard"] = {"record": fp64 [8] on the device, "ws": the reduction's workspace, "max_norm", "skip_nonfinite"}: state of the
    # ARENA, like ema / diag.  What the host does NOT learn: whether a step was dropped - so a dropped step still advances adam_t
    # (it consumes its number in the bias correction: with beta = (0.5, 0.9) the correction is within 1e-3 of 1 after about 60
    # steps), the average's update count and arena.version.  The statistics pass describes the UNCLIPPED g * grad_scale, and an
    # update delta that a dropped step did not apply; the record says which it was.
    has_guard = property(lambda self: self.opt.get("guard") is not None)

    def enable_guard(self, max_norm=0.0, skip_nonfinite=False):
        """From now on every optimiser step of this arena is guarded: one reduction over the scaled gradient (grad_guard), then the
        Adam pass reading the decision from device memory - clipped to the global norm max_norm (0: no clipping) and, with
        skip_nonfinite, dropped as a whole where the gradient holds an Inf or NaN.  The first call allocates the record (zeroed)
        and the workspace; a later call changes the settings only and keeps the counters."""
        max_norm, skip_nonfinite = guardmod.check_settings(max_norm, skip_nonfinite)
        gd = self.opt.get("guard")
        if gd is None:
            need_kernels(self.K, "a guarded update", "grad_guard", "adam_guarded", "adam_ema_guarded")
            dev = self.arena.flat.device
            nbytes = self.K.grad_guard_workspace_bytes(self.arena.live_numel) if hasattr(self.K, "grad_guard_workspace_bytes") else 0
            gd = self.opt["guard"] = {"record": torch.zeros(guardmod.NREC, dtype=torch.float64, device=dev),
                                      "ws": torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dev)}
        gd["max_norm"], gd["skip_nonfinite"] = max_norm, skip_nonfinite

    def disable_guard(self):
        """Stop guarding and free the record (its counters with it): the next optimiser step is the plain one again."""
        self.finish_update()
        self.opt.pop("guard", None)

    def _guard(self, what):
        gd = self.opt.get("guard")
        if gd is None:
            raise RuntimeError("%s: this network's updates are not guarded (enable_guard first)" % what)
        return gd

    def guard_report(self):
        """The record of the LAST guarded step as a dict (guard.report: norm, coef, s_eff, nonfinite, apply, and the cumulative
        clipped / skipped counts; all zero before the first step).  Applies a pending update first; one device read."""
        gd = self._guard("guard_report")
        self.finish_update()
        return guardmod.report(gd["record"].cpu().tolist(), gd["max_norm"], gd["skip_nonfinite"])

    def guard_state(self):
        """What a checkpoint keeps of the guard: the two cumulative counters {"clipped", "skipped"}."""
        r = self.guard_report()
        return {"clipped": r["clipped"], "skipped": r["skipped"]}

    def restore_guard(self, clipped, skipped):
        """Put saved counters back (guard_state; the settings in force stay)."""
        gd = self._guard("restore_guard")
        self.finish_update()
        gd["record"][6:8] = torch.tensor([float(int(clipped)), float(int(skipped))], dtype=torch.float64)

    # ---- weight averaging (sgg_amd/ema.py, csrc/optim.hip) -----------------------------------------------
    # opt["ema"] = {"flat": buffer of the arena's layout, "decay", "updates": shadow updates applied, "swapped"}: state of the ARENA,
    # like t / pending / diag - every Network on it sees the same average.
    has_average = property(lambda self: self.opt.get("ema") is not None)

    def _not_swapped(self, what):
        avg = self.opt.get("ema")
        if avg is not None and avg["swapped"]:
            raise RuntimeError("%s inside averaged(): the arena holds the averaged weights until the context exits" % what)

    def enable_averaging(self, decay):
        """Keep tf.train.ExponentialMovingAverage(decay, num_updates) of this arena's parameters: from now on every optimiser step
        also updates the average (one fused pass).  The first call allocates the buffer as a bit copy of the whole arena (dead tail
        included) with update count 0; a later call changes the decay only."""
        ema.tf_ema_decay(decay, 0)           # (ValueError unless 0 < decay < 1)
        avg = self.opt.get("ema")
        if avg is not None:
            avg["decay"] = float(decay)
            return
        need_kernels(self.K, "weight averaging", "adam_ema", "swap")
        self.finish_update()
        self.opt["ema"] = {"flat": self.arena.flat.clone(), "decay": float(decay), "updates": 0, "swapped": False}

    def disable_averaging(self):
        """Stop averaging and free the buffer: the next optimiser step is the plain one again."""
        self._not_swapped("disable_averaging")
        self.opt.pop("ema", None)

    def reset_average(self):
        """Restart the average from the arena as it is now (after a load_state_dict): bit copy, update count 0."""
        avg = self._average("reset_average")
        self._not_swapped("reset_average")
        self.finish_update()
        avg["flat"].copy_(self.arena.flat)
        avg["updates"] = 0

    def average_state(self):
        """What a checkpoint keeps of the average: {"flat": the whole buffer on the host, "updates", "decay"}."""
        avg = self._average("average_state")
        self._not_swapped("average_state")
        self.finish_update()
        return {"flat": avg["flat"].cpu(), "updates": int(avg["updates"]), "decay": float(avg["decay"])}

    def restore_average(self, flat, updates):
        """Put a saved buffer and update count back (average_state; the decay in force stays)."""
        avg = self._average("restore_average")
        self._not_swapped("restore_average")
        flat = torch.as_tensor(flat)
        if tuple(flat.shape) != tuple(avg["flat"].shape):
            raise ValueError("saved average has %d elements, this network's arena %d" % (flat.numel(), avg["flat"].numel()))
        avg["flat"].copy_(flat)
        avg["updates"] = int(updates)

    def _average(self, what):
        avg = self.opt.get("ema")
        if avg is None:
            raise RuntimeError("%s: this network keeps no weight average (enable_averaging first)" % what)
        return avg

    def _exchange_average(self):
        a = self.arena
        self.K.swap(a.live(), a.live(self.opt["ema"]["flat"]))
        a.version += 1                       # as adam_step after writing the parameters
        self.trunk.refresh_weights()

    @contextlib.contextmanager
    def averaged(self):
        """Run with the AVERAGED weights in the arena: the live ranges of the arena and of the average are exchanged on entry and
        exchanged back on exit, bit for bit.  Addresses never change - every view, weight descriptor and pre-split copy of every
        Network on the arena stays valid and is re-derived through arena.version, as after an optimiser step.  Applies a pending
        update first.  Not re-entrant; adam_step, load_state_dict, reset_average and state_dict raise inside.  For use between
        iterations (outside GanStep.iteration())."""
        avg = self._average("averaged()")
        self._not_swapped("a nested averaged()")
        self.finish_update()
        self._exchange_average()
        avg["swapped"] = True
        try:
            yield self
        finally:
            avg["swapped"] = False
            self._exchange_average()

    def state_dict(self, full_names=False, averaged=False):
        """The parameters (averaged=True: the average) by TF name, on the host; a pending update is applied first."""
        self._not_swapped("state_dict")
        self.finish_update()
        if not averaged:
            return self.arena.state_dict(full_names)
        views = self.arena._make_views(self._average("state_dict(averaged=True)")["flat"])
        return OrderedDict(((tf_variable_name(self.kind, n) if full_names else n), v.detach().clone().cpu()) for n, v in views.items())

    def load_state_dict(self, sd, strict=True):
        """arena.load_state_dict + the encoder's operand formats.  The average, if any, is left alone (reset_average restarts it)."""
        self._not_swapped("load_state_dict")
        self.arena.load_state_dict(sd, strict)
        self.trunk.refresh_weights()

    # ---- diagnostics (sgg_amd/diagnostics.py, csrc/stats.hip) -------------------------------------------
    def _diag_state(self):
        """Chunk table, workspace and stats buffer of this ARENA: built once, kept in `opt` (every Network on the arena sees them)."""
        st = self.opt.get("diag")
        if st is None:
            need_kernels(self.K, "the diagnostics pass", "arena_stats")
            chunk = self.K.arena_stats_chunk()
            names, offsets, numels = diagnostics.live_layout(self.arena)
            table = diagnostics.chunk_table(offsets, numels, chunk)
            diagnostics.check_table(table, len(names), self.arena.live_numel, chunk)
            dev = self.arena.flat.device
            st = self.opt["diag"] = {
                "names": names, "offsets": offsets, "numels": numels, "table": torch.from_numpy(table).to(dev),
                "ws": torch.empty(self.K.arena_stats_workspace_bytes(len(table)), dtype=torch.uint8, device=dev),
                "rows": torch.full((len(names), self.K.arena_stats_nstat()), float("nan"), dtype=torch.float64, device=dev),
                "last": None}                # (lr_t, grad_scale) of the pass the rows are from; None: no pass yet
        return st

    def arm_diagnostics(self, on=True):
        """While armed, every optimiser step on this arena is followed by the statistics pass (its rows overwrite the buffer)."""
        if on:
            self._diag_state()
        self.opt["armed"] = bool(on)

    def arena_stats(self, lr_t=None, grad_scale=None):
        """Launch the statistics pass on the current stream into the arena's buffer; default: with the lr_t and gradient scale of the
        last pass (re-reading the arenas as they are now).  Returns the device rows [T, 9]."""
        st = self._diag_state()
        if lr_t is None:
            assert st["last"] is not None, "arena_stats(): no optimiser step has been recorded yet"
            lr_t, grad_scale = st["last"]
        a = self.arena
        self.K.arena_stats(a.live(), a.live(self.grad_flat), a.live(self.m_flat), a.live(self.v_flat), st["table"], len(st["names"]),
                           lr_t, ADAM_EPS, grad_scale, out=st["rows"], ws=st["ws"])
        st["last"] = (lr_t, grad_scale)
        return st["rows"]


class GanStep:
    """The training hot path for a fixed (B, S, V). `reducer(network)` (optional) all-reduces network.grad_flat
    across data-parallel ranks and returns the scale to apply to the gradient (1/world_size)."""

    def __init__(self, K, V, S, B, lam=10.0, E=EMBED_DIM, g_state=None, d_state=None, dtype=torch.float32, reducer=None,
                 G=None, D=None, overlap_streams=False, head_side_stream=None):
        self.K, self.V, self.S, self.B, self.lam = K, V, S, B, float(lam)
        self.G = G if G is not None else Network(K, "G", V, S, B, E, dtype=dtype, state_dict=g_state)
        self.D = D if D is not None else Network(K, "D", V, S, B, E, dtype=dtype, state_dict=d_state)
        self.reducer = reducer
        dev = self.G.arena.flat.device
        z = lambda *s: torch.zeros(s, device=dev, dtype=dtype)
        self.TRI = z(3 * B, T_STEPS, V)          # rows: fake | real (one-hot) | interpolated
        self.gbuf = z(B, T_STEPS, V)             # g = d sum(D(x_hat)) / d x_hat
        self.vbuf = z(B, T_STEPS, V)             # lambda * dGP/dg
        self.slopes, self.pen = z(B), z(B)
        self.dfake = z(1, B, T_STEPS, V)
        self.d_losses, self.g_losses = z(4), z(4)
        self.tokens = torch.zeros((B, T_STEPS), dtype=torch.int64, device=dev)
        # Optional second HIP stream: the two encoders are independent until the critic head needs the fake triples,
        # so D's encoder forward can run next to G's forward (the HBM-bound LayerNorm passes of one network overlap
        # the MFMA-bound convolutions of the other, launch tails are filled).  Measured +3 % triples/s; off by
        # default because concurrent kernels make per-kernel durations (the roofline measurement) meaningless.
        self._g_reuse, self._g_reuse_armed = None, False       # (images, ctx) of G's encoder within one train_iteration
        self._g_reuse_slots = {}                 # accumulation: micro-batch k -> (images, copy of ctx, guard) (generator_forward)
        self._loss_acc, self._loss_n = {}, {"d": 1, "g": 1, "m": 1, "s": 1}    # sums of the four loss numbers over the micro-batches of an update
        # generator likelihood (pretrain_step, generator_step(mle_weight > 0), generator_nll): (nll per token, token accuracy, triple
        # accuracy, valid rows) of the last cross-entropy; the per-row buffers behind it are allocated at the first use (_xent_rows)
        self.mle_losses = z(4)
        self._xent_buf = None
        # relaxed generator output (set_relaxation; csrc/relax.hip): None = the critic sees the raw decoder logits
        self._relax, self._relax_buf = None, None
        # score-function generator update (set_estimator; csrc/score.hip): None = the pathwise update, nothing of it is launched or allocated
        self._estimator, self._score_bufs, self._score_multi_bufs = None, None, {}
        # (option side_priority: priority of the side streams - everything on them is off the critical chain of the main stream)
        prio = int(option(K, "side_priority"))
        self.side = torch.cuda.Stream(device=dev, priority=prio) if (overlap_streams and dev.type == "cuda") else None
        if self.side is not None:
            # backward: filter gradients beside the dgrad -> LayerNorm-backward chain (trunk.enable_wgrad_overlap)
            self.G.trunk.enable_wgrad_overlap(self.side)
            self.D.trunk.enable_wgrad_overlap(self.side)
        # The recurrent heads are chains of short dependent launches.  Their parameter-gradient work (95 of the ~330 launches per step:
        # every weight-gradient GEMM and column sum) is off that chain: with a stream of its own the backward pass DEFERS it there
        # behind one fork per pass (head.py; bit-identical results), and nothing waits for it until head.join() in front of the
        # optimiser - the chain, and the encoder backward after it, no longer carry those launches: 44.32 / 44.32 / 44.39 against
        # 45.12 / 45.01 / 45.20 ms per step (same box, interleaved; profiles/r04_head_deferred_grads_ab.log).  Part of the two-stream
        # schedule by default (head_side_stream=None follows overlap_streams).  Round 3's form - a fork per time step and a join at
        # the end of every pass - measured equal to none.
        if head_side_stream is None:
            head_side_stream = overlap_streams
        self.head_side = torch.cuda.Stream(device=dev, priority=prio) if (head_side_stream and dev.type == "cuda") else None
        self.G.head.enable_side_stream(self.head_side)
        self.D.head.enable_side_stream(self.head_side)

    # ------------------------------------------------------------------------------------------------
    def _g_early_stream(self, images, N=1):
        """Option g_early (default on, two-stream schedule): G's encoder forward of THIS update depends on nothing the previous update
        still computes once that update's G head has run (a critic update leaves G's weights alone): it may start on a stream of its
        own right there - beside the critic's heads, which are a chain of short launches that leaves the chip idle, and its encoder
        backward.  Returns that stream (already waiting for the event), or None.  Same kernels, same operands: bit-identical;
        43.17 / 43.15 against 43.60 / 43.73 ms per step (profiles/r04_g_early_ab.log)."""
        ev, ev_images = getattr(self, "_ev_g_free", None), getattr(self, "_ev_g_images", None)
        self._ev_g_free = self._ev_g_images = None
        if self.side is None or ev is None or not option(self.K, "g_early") or self.G.pending is not None or self._g_reuse is not None:
            return None
        if N > 1 and self._g_reuse_armed:        # accumulation with reuse: G's encoder output is kept per micro-batch on the main stream
            return None
        # only for the minibatch tensor the critic update ran on, unmodified (train.py:175-190 repeats each batch for every update of an
        # iteration): the early stream waits for nothing the main stream enqueued after that update's G head, so a tensor produced there
        # since (another batch, an augmentation in place) would be read too early
        if ev_images is None or ev_images[0] is not images or ev_images[1] != images._version:
            return None
        # ... and only for the parameters that critic update left: a state-dict load or an optimiser step through another batch size's
        # Network on the shared arena since then would make trunk.forward re-derive the weight formats (refresh_weights) on the early
        # stream, unordered against the main stream's writes - as would an option of K changed since the encoder made its plan
        if ev_images[2] != (self.G.arena.version, self.G.adam_t) or not self.G.trunk.plan_current():
            return None
        # ... and only if no input-gradient pass (sgg_amd/grad.py) has used G's encoder buffers on the main stream since then
        if ev_images[3] != self.G.data_passes:
            return None
        if getattr(self, "xs", None) is None:
            self.xs = torch.cuda.Stream(device=images.device)
        self.xs.wait_event(ev)
        return self.xs

    def generator_forward(self, images, noise, for_backward=True, early=None, micro=None):
        """Generator.build_generator: fake logits [B,3,V] (a view of the critic's input slab).

        Inside train_iteration(..., reuse_g_encoder=True) G's ENCODER runs once per iteration: every update of an iteration sees
        the same minibatch (train.py:175-190 repeats each batch CRITIC_ITERS + 1 times) and G's weights only change at its end, so
        the encoder output, the step-invariant attention product and the activations kept for G's backward are those of the first
        call; only the recurrent head (fresh noise) is re-run.  bench.py never does this (every update recomputes everything)."""
        G = self.G
        k, N = micro if micro is not None else (0, 1)
        if N > 1:
            # An update over N micro-batches (train_iteration_accumulated).  With reuse armed, the critic updates (forward-only
            # passes) of an iteration share G's encoder output per micro-batch: the first one keeps a COPY of ctx (the trunk's output
            # buffer is overwritten by the next micro-batch's forward), later ones re-run only the step-invariant attention product
            # (the head has one P buffer) and the head.  Same forward-only schedule on the same weights: bit-equal to recomputing.
            # The generator update (for_backward) always runs the encoder afresh: there is one set of backward activations.
            guard = (images.data_ptr(), images._version, G.adam_t)
            slot = self._g_reuse_slots.get(k) if (self._g_reuse_armed and not for_backward) else None
            if slot is not None:
                assert slot[0] is images and slot[2] == guard, \
                    "G-encoder reuse: micro-batch %d was modified in place or replaced (or G was updated) inside one iteration" % k
                ctx = slot[1]
                G.head.precompute(ctx)
            elif early is not None:
                ctx = self._encode(G, images, for_backward, early, int(option(self.K, "g_early_cus")))
                torch.cuda.current_stream().wait_stream(early)
            else:
                ctx = self._encode(G, images, for_backward)
                if self._g_reuse_armed and not for_backward:
                    self._g_reuse_slots[k] = (images, ctx.clone(), guard)
        elif self._g_reuse is not None and self._g_reuse[0] is images:
            # the kept encoder output is only valid for the tensor's contents at the first call: an in-place write to the minibatch
            # (augmentation, a loader refilling its device buffer) or an optimiser step of G since then would silently train on stale
            # activations.  (Invariant of the schedule: no G.head.backward runs between the first generator_forward of an iteration
            # and generator_step, so the dP / dctx accumulators head.precompute cleared are still zero there.)
            assert self._g_reuse[2] == (images.data_ptr(), images._version, G.adam_t), \
                "G-encoder reuse: the minibatch tensor was modified in place (or G was updated) inside one iteration"
            ctx = self._g_reuse[1]
        else:
            keep = for_backward or self._g_reuse_armed
            if early is not None:        # (the caller made `early` wait for everything this forward depends on)
                ctx = self._encode(G, images, keep, early, int(option(self.K, "g_early_cus")))
                torch.cuda.current_stream().wait_stream(early)
            else:
                ctx = self._encode(G, images, keep)
            if self._g_reuse_armed:
                self._g_reuse = (images, ctx, (images.data_ptr(), images._version, G.adam_t))
        st = G.head.state(1, self.B)
        G.head.forward(st, ctx, noise)
        return st, ctx

    @staticmethod
    def _encode(net, images, for_backward, stream=None, cu_cap=0):
        """Run this network's encoder: trunk forward (for_backward, cu_cap: Trunk.forward) and the step-invariant attention product of
        its head, on `stream` when one is given (the caller orders it); returns ctx."""
        kw = {"cu_cap": cu_cap} if cu_cap else {}
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            ctx = net.trunk.forward(images, for_backward, **kw)
            net.head.precompute(ctx)
        return ctx

    def _d_encoder_on_side_stream(self, images, zero_grads, for_backward=True):
        """D.finish_update (pending all-reduce + Adam), D's encoder forward and the step-invariant attention product,
        enqueued on the side stream (where there is one); returns ctx. Call _join_side() before anything on the main stream reads them."""
        D, cap = self.D, 0
        if self.side is not None:
            self.side.wait_stream(torch.cuda.current_stream())
            cap = int(option(self.K, "d_side_cus"))                 # (option d_side_cus: as g_early_cus, for D's forward beside G's forward and head)
        with torch.cuda.stream(self.side) if self.side is not None else contextlib.nullcontext():
            D.finish_update()
            if zero_grads:
                D.zero_grads()
            return self._encode(D, images, for_backward, cu_cap=cap)

    def _join_side(self):
        if self.side is not None:
            torch.cuda.current_stream().wait_stream(self.side)

    # ---- relaxed generator output (csrc/relax.hip) --------------------------------------------------------
    RELAX_MODES = ("logits", "softmax", "gumbel")

    def set_relaxation(self, mode, tau=1.0, seed=0, hard=False):
        """What the critic sees of G's decoder rows x: "logits" (default) = x itself, nothing launched; "softmax" = y = softmax(x / tau);
        "gumbel" = y = softmax((x + g) / tau) with g drawn on the device from (seed, draw, row, column) - `draw` is the 64-bit number
        each step takes.  The generator's update differentiates through y (one launch in front of D, one behind the critic's gradient
        of its input); the critic's update treats y as a constant, as it treats the logits.  tau may be changed between steps by
        another call (a schedule); the [B, 3, V] buffer of the generator update is allocated the first time a mode is on.
        hard (straight-through, with "softmax" or "gumbel"): the critic sees onehot(argmax(x + g)) in both updates, and the generator's
        update takes the gradient of the soft row y, rebuilt from the logits and the same draw behind the critic's input gradient."""
        if mode not in self.RELAX_MODES:
            raise ValueError("generator_output must be one of %s (got %r)" % (", ".join(self.RELAX_MODES), mode))
        if hard and mode == "logits":
            raise ValueError("the straight-through (hard) output needs generator_output softmax or gumbel: raw logits have no one-hot form")
        if mode == "logits":
            self._relax = None
            return
        tau = float(tau)
        if not (math.isfinite(tau) and tau > 0.0):
            raise ValueError("the relaxation's temperature must be a finite number > 0 (got %r)" % tau)
        if hard:
            need_kernels(self.K, "generator_output=%s, hard" % mode, "relax_rows_hard", "relax_rows_hard_bwd")
        else:
            need_kernels(self.K, "generator_output=%s" % mode, "relax_rows", "relax_rows_bwd")
        self._relax = {"mode": mode, "tau": tau, "seed": int(seed) & 0xFFFFFFFFFFFFFFFF}
        if hard:
            self._relax["hard"] = True
        if self._relax_buf is None:
            self._relax_buf = torch.zeros_like(self.TRI[:self.B])

    relaxation = property(lambda self: None if self._relax is None else dict(self._relax))

    def _relax_fwd(self, logits, out, draw):
        """out = the relaxed rows of `logits` [B,3,V] in the mode in force (one launch)."""
        rx = self._relax
        gumbel = rx["mode"] == "gumbel"
        draw = int(draw or 0) if gumbel else 0
        if rx.get("hard"):
            self.K.relax_rows_hard(logits, y=out, gumbel=gumbel, seed=rx["seed"], draw=draw)
        else:
            self.K.relax_rows(logits, rx["tau"], y=out, gumbel=gumbel, seed=rx["seed"], draw=draw)
        return out

    # ---- score-function generator update (csrc/score.hip) ---------------------------------------------------
    ESTIMATORS = ("pathwise", "score")
    SCORE_BASELINES = ("rloo", "none", "image")
    SCORE_MAX_SAMPLES = 16

    def _check_score_relaxation(self):
        rx = self._relax
        if rx is None or rx["mode"] != "gumbel" or not rx.get("hard"):
            have = "logits" if rx is None else "%s, hard=%s" % (rx["mode"], bool(rx.get("hard")))
            raise ValueError("generator_gradient=score needs generator_output=gumbel with hard=True - the critic must see Gumbel-max "
                             "samples of softmax(logits) in both updates (the relaxation in force is generator_output=%s)" % have)

    def set_estimator(self, kind="pathwise", baseline=None, entropy_weight=0.0, samples=1):
        """How the generator's update gets its gradient.  "pathwise" (default): through the critic's gradient of its input, as
        set_relaxation describes - today's path, nothing new launched.  "score": the score-function (REINFORCE) estimator.  The critic
        scores the sampled one-hot rows (the relaxation must be "gumbel" with hard=True: tok is then an exact sample of
        softmax(logits)), its head is NOT differentiated, and the logits receive the gradient of
            -(1/B) sum_b A_b sum_t log p(a_bt) - (entropy_weight / B) sum_{b,t} H(p_bt)
        with A_b a constant: the reward r_b = mean_t D(sample b)[t], minus - baseline "rloo" - the mean reward of the OTHER samples of
        the (micro-)batch, which leaves the estimator unbiased; "none": r_b itself.  entropy_weight >= 0: an entropy bonus on the
        policy.  Four numbers of the update land in score_losses.
        samples = S >= 2 (at most 16): S triples per image are drawn from the one set of logits (draw numbers draw | (s << 56)), D's head
        scores the S * B of them against the B feature maps, and the first term becomes
            -(1/(B S)) sum_{b,s} A_sb sum_t log p(a_sbt).
        baseline "image" (the default there; refused at S = 1): r_sb minus the mean reward of the other samples of the SAME image, which
        takes the image's own difficulty out of the advantage and exists at B = 1; "rloo": minus the mean of the other S * B - 1 rewards.
        The critic's updates keep one sample per image.  samples = 1 is the path above, call for call."""
        if kind not in self.ESTIMATORS:
            raise ValueError("generator_gradient must be one of %s (got %r)" % (", ".join(self.ESTIMATORS), kind))
        if kind == "pathwise":
            self._estimator = None
            return
        S = int(samples)
        if S != samples or not 1 <= S <= self.SCORE_MAX_SAMPLES:
            raise ValueError("score_samples must be an integer in 1..%d (got %r)" % (self.SCORE_MAX_SAMPLES, samples))
        if baseline is None:
            baseline = "image" if S > 1 else "rloo"
        if baseline not in self.SCORE_BASELINES:
            raise ValueError("score_baseline must be one of %s (got %r)" % (", ".join(self.SCORE_BASELINES), baseline))
        entropy_weight = float(entropy_weight)
        if not (math.isfinite(entropy_weight) and entropy_weight >= 0.0):
            raise ValueError("entropy_weight must be a finite number >= 0 (got %r)" % entropy_weight)
        self._check_score_relaxation()
        if S == 1:
            need_kernels(self.K, "generator_gradient=score", "score_advantage", "score_rows", "score_summary", "relax_rows_hard")
        else:
            need_kernels(self.K, "generator_gradient=score with score_samples > 1", "sample_rows_multi", "score_advantage_multi",
                         "score_rows_multi", "score_summary_multi")
        if baseline == "image" and S < 2:
            raise ValueError("score_baseline=image compares each sample with the other samples of its image: it needs score_samples >= 2 "
                             "(got %d)" % S)
        if baseline == "rloo" and S * self.B < 2:
            raise ValueError("score_baseline=rloo compares each sample with the others of its batch: it needs B >= 2 (got B = %d)" % self.B)
        dev, dt, R = self.g_losses.device, self.g_losses.dtype, self.B * T_STEPS
        if S == 1 and self._score_bufs is None:
            self._score_bufs = {"tok": torch.zeros((self.B, T_STEPS), dtype=torch.int64, device=dev), "adv": torch.zeros(self.B, dtype=dt, device=dev),
                                "logp": torch.zeros(R, dtype=dt, device=dev), "ent": torch.zeros(R, dtype=dt, device=dev)}
        if S > 1 and self._score_multi_bufs.get("S") != S:
            self._score_multi_bufs = {"S": S, "tok": torch.zeros((S, self.B, T_STEPS), dtype=torch.int64, device=dev),
                                      "adv": torch.zeros(S * self.B, dtype=dt, device=dev), "logp": torch.zeros(S * R, dtype=dt, device=dev),
                                      "ent": torch.zeros(R, dtype=dt, device=dev)}
        if getattr(self, "score_losses", None) is None:
            self.score_losses = torch.zeros(4, dtype=dt, device=dev)
        self._estimator = {"kind": "score", "baseline": baseline, "entropy_weight": entropy_weight}
        if S > 1:
            self._estimator["samples"] = S

    estimator = property(lambda self: {"kind": "pathwise"} if self._estimator is None else dict(self._estimator))
    _score_now = property(lambda self: self._score_multi_bufs if (self._estimator or {}).get("samples", 1) > 1 else self._score_bufs)
    _score_tok = property(lambda self: self._score_now["tok"])
    _score_adv = property(lambda self: self._score_now["adv"])

    def critic_step(self, images, labels, noise, alpha, micro=None, draw=None):
        """One disc_train_op (train.py:365). labels int64 [B,3]; noise [B,512]; alpha [B]. Returns self.d_losses
        = (disc_cost, wasserstein term, gradient penalty, mean D(fake)) as a device tensor.
        micro = (k, N): this is micro-batch k of an update over N (Network.end_micro_batch); None = (0, 1), the whole update.
        draw: the 64-bit number of this launch's Gumbel noise (set_relaxation; ignored unless the mode is "gumbel")."""
        K, B, V, D = self.K, self.B, self.V, self.D
        mk, mN = micro if micro is not None else (0, 1)
        if mN > 1:
            D._acc_flat()                         # (raises before anything is launched if the kernel set cannot accumulate)
        fake_rows, real_rows, hat_rows = self.TRI[:B], self.TRI[B:2 * B], self.TRI[2 * B:]
        # Data parallel: the network WITHOUT a gradient all-reduce in flight goes first, so that its encoder forward
        # runs under the other network's collective before anything waits for it (critic_iters = 1: G's reduce from the
        # last generator step hides under D's encoder; critic_iters > 1: D's reduce from the previous critic update
        # hides under G's forward).  With a side stream the wait is enqueued there and never blocks the main stream.
        if D.pending is None or self.side is not None:
            early = self._g_early_stream(images, mN)  # (critic_iters > 1: after another critic update)
            ctx = self._d_encoder_on_side_stream(images, zero_grads=True)
            self.G.finish_update()
            gst, _ = self.generator_forward(images, noise, for_backward=False, early=early, micro=micro)     # the critic update never differentiates G
        else:
            self.G.finish_update()
            gst, _ = self.generator_forward(images, noise, for_backward=False, micro=micro)
            ctx = self._d_encoder_on_side_stream(images, zero_grads=True)
        if self.side is not None and option(K, "g_early"):
            # G's encoder buffers are free from here on, and this critic update does not touch G's weights (_g_early_stream)
            self._ev_g_free = torch.cuda.Event()
            self._ev_g_free.record()
            self._ev_g_images = (images, images._version, (self.G.arena.version, self.G.adam_t), self.G.data_passes)
        self._join_side()
        if self._relax is None:
            fake_rows.copy_(gst.OUT[0])
        else:
            self._relax_fwd(gst.OUT[0], fake_rows, draw)      # (the launch writes y where the copy wrote the logits)
        K.onehot(labels, real_rows)
        K.interpolate(real_rows, fake_rows, alpha, hat_rows)
        # ---- first-order pass on the 3B-row super-batch ------------------------------------------------
        st = D.head.state(1, 3 * B)
        D.head.forward(st, ctx, [self.TRI], labels, (B, 2 * B))
        inv = 1.0 / (B * T_STEPS)
        K.fill(st.dOUT[0][:B], inv)               # d mean(D(fake))
        K.fill(st.dOUT[0][B:2 * B], -inv)         # d -mean(D(real))
        K.fill(st.dOUT[0][2 * B:], 1.0)           # d sum(D(x_hat)) -> g
        D.head.backward(st, ctx, [self.TRI], R_w=2 * B, labels=labels, label_rows=(B, 2 * B))
        ind = D.head.in_dim
        for t in range(T_STEPS):
            K.gemm_nt(st.dXH[t][0][2 * B:, FEAT_C:ind], D.head.W_emb, self.gbuf[:, t, :])
        K.gp_fwd(self.gbuf, self.slopes, self.pen)
        K.gp_bwd(self.gbuf, self.slopes, self.pen, self.vbuf, self.lam)
        K.wgan_losses(st.OUT[0].view(3 * B, T_STEPS), self.pen, self.lam, B, T_STEPS, True, self.d_losses)
        # ---- gradient of lambda*GP: dual-number pass on the interpolated rows ------------------------------
        st2 = D.head.state(2, B)
        u2 = [hat_rows, self.vbuf]
        D.head.forward(st2, ctx, u2)
        K.fill(st2.dOUT[0], 1.0)                  # cotangent of the tangent output (= d(lambda*GP)/d JVP)
        K.fill(st2.dOUT[1], 0.0)
        D.head.backward(st2, ctx, u2, R_w=B)
        # W enters g = delta_e @ W^T directly as well: handled by the tangent input v @ W above (u2[1])
        dctx = D.head.finish_backward(ctx)
        D.trunk.backward(dctx)
        D.head.join()
        self._sum_losses("d", self.d_losses, mk, mN)
        D.end_micro_batch(mk, mN, self.reducer)
        return self.d_losses

    def critic_loss(self, images, labels, noise, alpha, out=None, draw=None):
        """disc_cost of a minibatch WITHOUT an update: what `sess.run(self.disc_cost, feed_dict = {handle: val_handle})` evaluates
        for the validation-loss early stop (train.py:375-377).  Same forward as critic_step; the head backward runs only as far as
        g = d sum(D(x_hat)) / d x_hat needs it (no parameter gradient is touched, R_w = 0), no encoder backward, no Adam.
        Returns (disc_cost, wasserstein term, gradient penalty, mean D(fake)) in `out` (default: a buffer of its own)."""
        K, B, V, D = self.K, self.B, self.V, self.D
        assert self._g_reuse is None and not self._g_reuse_armed, "critic_loss inside an iteration with G-encoder reuse"
        if out is None:
            if getattr(self, "val_losses", None) is None:
                self.val_losses = torch.zeros_like(self.d_losses)
            out = self.val_losses
        fake_rows, real_rows, hat_rows = self.TRI[:B], self.TRI[B:2 * B], self.TRI[2 * B:]
        self.flush()
        ctx = self._encode(D, images, False)
        gst, _ = self.generator_forward(images, noise, for_backward=False)
        if self._relax is None:
            fake_rows.copy_(gst.OUT[0])
        else:
            self._relax_fwd(gst.OUT[0], fake_rows, draw)
        K.onehot(labels, real_rows)
        K.interpolate(real_rows, fake_rows, alpha, hat_rows)
        st = D.head.state(1, 3 * B)
        D.head.forward(st, ctx, [self.TRI], labels, (B, 2 * B))
        K.fill(st.dOUT[0][:2 * B], 0.0)
        K.fill(st.dOUT[0][2 * B:], 1.0)           # d sum(D(x_hat)) -> g
        D.head.backward(st, ctx, [self.TRI], R_w=0)
        ind = D.head.in_dim
        for t in range(T_STEPS):
            K.gemm_nt(st.dXH[t][0][2 * B:, FEAT_C:ind], D.head.W_emb, self.gbuf[:, t, :])
        K.gp_fwd(self.gbuf, self.slopes, self.pen)
        K.wgan_losses(st.OUT[0].view(3 * B, T_STEPS), self.pen, self.lam, B, T_STEPS, True, out)
        return out

    def generator_step(self, images, noise, micro=None, labels=None, mle_weight=0.0, draw=None):
        """One gen_train_op (train.py:368). Returns self.g_losses; g_losses[3] = mean D(fake) = -gen_cost.  micro: as critic_step.
        mle_weight = w > 0 (with labels int64 [B,3]): the auxiliary likelihood term, gen_cost' = -mean D(G(x)) + w * xent with xent
        the loss of pretrain_step - one softmax_xent launch that ADDS w / B * (softmax - onehot) to the critic's gradient of the fake
        logits, and the summary into self.mle_losses.  w = 0 (default): nothing of it is launched.
        With a relaxation on (set_relaxation) D's input is y = relax(logits) in a buffer of its own, and the critic's gradient of y is
        turned into the gradient of the logits in place (relax_rows_bwd) before the likelihood term - a function of the logits - adds
        to it.  With the hard option D's input is the one-hot row and the second launch is relax_rows_hard_bwd on the logits.
        With the score-function estimator (set_estimator) D's head is not differentiated: _score_logits_gradient.
        draw: as critic_step."""
        K, B, G, D = self.K, self.B, self.G, self.D
        mk, mN = micro if micro is not None else (0, 1)
        mle_weight = float(mle_weight)
        if not (mle_weight >= 0.0 and math.isfinite(mle_weight)):
            raise ValueError("mle_weight must be a finite number >= 0 (got %r)" % mle_weight)
        if mle_weight > 0.0:
            if labels is None:
                raise ValueError("generator_step: mle_weight > 0 needs the labels of the minibatch")
            self._need_xent("generator_step(mle_weight > 0)")
        score = self._estimator
        if score is not None:
            self._check_score_relaxation()        # (set_relaxation may have been called since set_estimator)
        if mN > 1:
            G._acc_flat()
        G.finish_update()
        G.zero_grads()
        if D.pending is None or self.side is not None:
            early = self._g_early_stream(images, mN)
            ctx = self._d_encoder_on_side_stream(images, zero_grads=False, for_backward=False)   # independent of G's forward
            gst, gctx = self.generator_forward(images, noise, early=early, micro=micro)
        else:
            # the critic-gradient all-reduce launched at the end of critic_step runs under G's forward; only then does
            # D.finish_update() wait for it
            gst, gctx = self.generator_forward(images, noise, micro=micro)
            ctx = self._d_encoder_on_side_stream(images, zero_grads=False, for_backward=False)   # only D's head is differentiated here
        fake = gst.OUT[0]
        self._join_side()
        if score is not None:
            self._score_logits_gradient(score, gst, ctx, draw)
        else:
            d_in = fake if self._relax is None else self._relax_fwd(fake, self._relax_buf, draw)
            st = D.head.state(1, B, "g")
            D.head.forward(st, ctx, [d_in])
            K.wgan_losses(st.OUT[0].view(B, T_STEPS), None, 0.0, B, T_STEPS, False, self.g_losses)
            K.fill(st.dOUT[0], -1.0 / (B * T_STEPS))  # gen_cost = -mean(D(G(x)))
            D.head.backward(st, ctx, [d_in], R_w=0)
            ind = D.head.in_dim
            for t in range(T_STEPS):
                K.gemm_nt(st.dXH[t][0][:, FEAT_C:ind], D.head.W_emb, gst.dOUT[0][:, t, :])
            if self._relax is not None and self._relax.get("hard"):
                # straight-through: d_in holds the one-hot rows; the soft row's gradient from the logits and the forward's draw, in place
                gumbel = self._relax["mode"] == "gumbel"
                K.relax_rows_hard_bwd(fake, gst.dOUT[0], self._relax["tau"], gumbel=gumbel, seed=self._relax["seed"],
                                      draw=(int(draw or 0) if gumbel else 0))
            elif self._relax is not None:
                K.relax_rows_bwd(d_in, gst.dOUT[0], self._relax["tau"])        # d cost / d y -> d cost / d logits, in place
        if mle_weight > 0.0:
            self._xent(fake, labels, mle_weight / B, gst.dOUT[0], accumulate=True, out=self.mle_losses)
            self._sum_losses("m", self.mle_losses, mk, mN)
        G.head.backward(gst, gctx, None, R_w=B)
        dctx = G.head.finish_backward(gctx)
        G.trunk.backward(dctx)
        G.head.join()
        self._sum_losses("g", self.g_losses, mk, mN)
        if score is not None:
            self._sum_losses("s", self.score_losses, mk, mN)
        G.end_micro_batch(mk, mN, self.reducer)
        return self.g_losses

    def _score_logits_gradient(self, score, gst, ctx, draw):
        """The middle of generator_step with the score-function estimator (set_estimator): D's head runs forward only, on the sampled
        one-hot rows, into g_losses; the gradient of the logits (G's dOUT) comes from the samples' log-probabilities weighted by their
        advantages, and the update's four numbers go into score_losses."""
        K, B, D = self.K, self.B, self.D
        if score.get("samples", 1) > 1:
            return self._score_logits_gradient_multi(score, gst, ctx, draw)
        fake, bufs, rx = gst.OUT[0], self._score_bufs, self._relax
        # one launch: the one-hot rows D scores and the tokens they are the rows of - Gumbel-max samples of softmax(fake)
        K.relax_rows_hard(fake, y=self._relax_buf, tok=bufs["tok"], gumbel=True, seed=rx["seed"], draw=int(draw or 0))
        st = D.head.state(1, B, "g")
        D.head.forward(st, ctx, [self._relax_buf])
        K.wgan_losses(st.OUT[0].view(B, T_STEPS), None, 0.0, B, T_STEPS, False, self.g_losses)
        K.score_advantage(st.OUT[0].view(B, T_STEPS), score["baseline"], adv=bufs["adv"], out2=self.score_losses[0:2])
        K.score_rows(fake, bufs["tok"].view(-1), bufs["adv"], group=T_STEPS, coef=1.0 / B, ent_coef=score["entropy_weight"] / B,
                     dx=gst.dOUT[0], logp=bufs["logp"], ent=bufs["ent"])
        K.score_summary(bufs["logp"], bufs["ent"], out2=self.score_losses[2:4])

    def _score_logits_gradient_multi(self, score, gst, ctx, draw):
        """_score_logits_gradient with S = score["samples"] >= 2 triples per image: one launch draws them all from G's logits, D's head
        runs forward only on S * B rows against the B feature maps (row s * B + b reads image b) and takes the tokens as a row gather of
        its embedding - no one-hot row exists -, and one launch turns the S * B advantages into the gradient of the B * 3 logits rows."""
        K, B, D, S = self.K, self.B, self.D, score["samples"]
        fake, bufs, rx = gst.OUT[0], self._score_multi_bufs, self._relax
        assert bufs.get("S") == S
        K.sample_rows_multi(fake, bufs["tok"], seed=rx["seed"], draw=int(draw or 0))
        st = D.head.sample_state(S * B)
        D.head.forward(st, ctx, [None], bufs["tok"].view(S * B, T_STEPS), (0, S * B))
        K.wgan_losses(st.OUT[0].view(S * B, T_STEPS), None, 0.0, S * B, T_STEPS, False, self.g_losses)
        K.score_advantage_multi(st.OUT[0].view(S * B, T_STEPS), S, score["baseline"], adv=bufs["adv"], out2=self.score_losses[0:2])
        K.score_rows_multi(fake, bufs["tok"], bufs["adv"], group=T_STEPS, coef=1.0 / (B * S), ent_coef=score["entropy_weight"] / B,
                           dx=gst.dOUT[0], logp=bufs["logp"], ent=bufs["ent"])
        K.score_summary_multi(bufs["logp"], bufs["ent"], out2=self.score_losses[2:4])

    # ---- generator likelihood (csrc/xent.hip) -------------------------------------------------------------
    def _need_xent(self, what):
        need_kernels(self.K, what, "softmax_xent", "xent_summary")

    def _xent(self, logits, labels, scale, dlogits, accumulate, out):
        """softmax_xent of the B * 3 decoder rows `logits` [B,3,V] against labels int64 [B,3] (gradient into dlogits unless None),
        then its summary into `out` (4 floats)."""
        if self._xent_buf is None:
            dev, R = self.mle_losses.device, self.B * T_STEPS
            self._xent_buf = (torch.zeros(R, dtype=self.mle_losses.dtype, device=dev), torch.zeros(R, dtype=torch.int32, device=dev))
        nll, hit = self._xent_buf
        assert tuple(labels.shape) == (self.B, T_STEPS) and labels.dtype == torch.int64
        self.K.softmax_xent(logits, labels.reshape(-1), scale=scale, accumulate=accumulate, dlogits=dlogits, nll=nll, hit=hit)
        return self.K.xent_summary(nll, hit, out=out)

    def pretrain_step(self, images, labels, noise, micro=None):
        """One maximum-likelihood update of G: loss = (1/B) * sum_b sum_t -log softmax(logits[b,t])[labels[b,t]] - the likelihood
        K-best decoding ranks by, as a supervised objective.  G's forward as in generator_step, the cross-entropy and its gradient
        (scale 1/B) in one launch into the head's dOUT, then G's backward and end_micro_batch: accumulation (micro), the data-parallel
        all-reduce, the guard, the weight average and the diagnostics apply as to any update of G; its Adam moments and step count
        are those of the GAN phase.  D is never touched.  Returns self.mle_losses = (nll per token, token accuracy, triple accuracy,
        valid rows) as a device tensor."""
        B, G = self.B, self.G
        if self._g_reuse_armed or self._g_reuse is not None:
            raise RuntimeError("pretrain_step inside an iteration with G-encoder reuse: the step updates G, the kept encoder output "
                               "would be stale")
        self._need_xent("pretrain_step")
        mk, mN = micro if micro is not None else (0, 1)
        if mN > 1:
            G._acc_flat()
        # G's weights change here without a critic update in front: an early encoder forward (_g_early_stream) must not start from an
        # event recorded before this step (its guard on (arena.version, adam_t) refuses it as well)
        self._ev_g_free = self._ev_g_images = None
        G.finish_update()
        G.zero_grads()
        gst, gctx = self.generator_forward(images, noise, micro=micro)
        self._xent(gst.OUT[0], labels, 1.0 / B, gst.dOUT[0], accumulate=False, out=self.mle_losses)
        G.head.backward(gst, gctx, None, R_w=B)
        dctx = G.head.finish_backward(gctx)
        G.trunk.backward(dctx)
        G.head.join()
        self._sum_losses("m", self.mle_losses, mk, mN)
        G.end_micro_batch(mk, mN, self.reducer)
        return self.mle_losses

    def generator_nll(self, images, labels, noise, out=None):
        """The four numbers of pretrain_step for a minibatch WITHOUT an update (the forward-only counterpart of critic_loss): the
        held-out negative log-likelihood of the ground-truth tokens under G(images, noise).  Returns them in `out` (default: a buffer
        of its own)."""
        assert self._g_reuse is None and not self._g_reuse_armed, "generator_nll inside an iteration with G-encoder reuse"
        self._need_xent("generator_nll")
        if out is None:
            if getattr(self, "val_nll", None) is None:
                self.val_nll = torch.zeros_like(self.mle_losses)
            out = self.val_nll
        self.flush()
        self._ev_g_free = self._ev_g_images = None      # (G's encoder buffers are rewritten on this stream)
        gst, _ = self.generator_forward(images, noise, for_backward=False)
        return self._xent(gst.OUT[0], labels, 1.0, None, accumulate=False, out=out)

    # ---- loss numbers of an update over N micro-batches --------------------------------------------------
    def _sum_losses(self, which, losses, k, N):
        """Every loss number is a mean over rows: the mean over N equal micro-batches is the number of the N * B rows.  The sum is
        kept on the device by the accumulate kernel (k = 0: copy), the division by N happens on read.  N = 1: nothing is launched."""
        self._loss_n[which] = N
        if N == 1:
            return
        acc = self._loss_acc.get(which)
        if acc is None:
            acc = self._loss_acc[which] = torch.zeros_like(losses)
        self.K.grad_accumulate(acc, losses, first=(k == 0))

    def _losses_mean(self, which, losses):
        n = self._loss_n[which]
        return losses if n == 1 else self._loss_acc[which] / n

    # (disc_cost, wasserstein term, gradient penalty, mean D(fake)) / (-, -, -, mean D(fake)) of the LAST update as means over its
    # micro-batches; without accumulation d_losses / g_losses themselves
    d_losses_mean = property(lambda self: self._losses_mean("d", self.d_losses))
    g_losses_mean = property(lambda self: self._losses_mean("g", self.g_losses))
    # (nll per token, token accuracy, triple accuracy, valid rows) of the last cross-entropy of a training step, the same way
    mle_losses_mean = property(lambda self: self._losses_mean("m", self.mle_losses))
    # (mean reward, mean advantage^2, mean log-probability per sampled token, mean entropy per token) of the last score-function update
    score_losses_mean = property(lambda self: self._losses_mean("s", self.score_losses))

    def flush(self):
        """Apply any deferred optimiser update (before reading weights / at the end of the timed region)."""
        self.D.finish_update()
        self.G.finish_update()

    # ---- diagnostics ---------------------------------------------------------------------------------
    def arm_diagnostics(self, on=True):
        """Arm (or disarm) both networks: while armed, each of their optimiser steps is followed by the statistics pass over its
        arenas (Network.adam_step).  Read-only: the training state is bit-identical to a run that was never armed."""
        self.G.arm_diagnostics(on)
        self.D.arm_diagnostics(on)

    # ---- guarded updates ---------------------------------------------------------------------------
    def set_guard(self, max_norm=0.0, skip_nonfinite=False):
        """Guard the updates of both networks (Network.enable_guard).  max_norm: one number for both, or (critic's, generator's);
        0 = no clipping.  A network with neither control on is left - or put back - on the plain Adam pass."""
        d_norm, g_norm = max_norm if isinstance(max_norm, (tuple, list)) else (max_norm, max_norm)
        for net, mx in ((self.D, d_norm), (self.G, g_norm)):
            mx, skip = guardmod.check_settings(mx, skip_nonfinite)
            if mx > 0.0 or skip:
                net.enable_guard(mx, skip)
            else:
                net.disable_guard()

    def guard_reports(self):
        """{"D": Network.guard_report(), "G": ...} of the guarded networks (empty: no guard is on).  ONE device read for both."""
        self.flush()
        nets = [(n, net) for n, net in (("D", self.D), ("G", self.G)) if net.has_guard]
        if not nets:
            return {}
        host = torch.cat([net.opt["guard"]["record"] for _, net in nets]).cpu().tolist()
        return {n: guardmod.report(host[i * guardmod.NREC:(i + 1) * guardmod.NREC], net.opt["guard"]["max_norm"],
                                   net.opt["guard"]["skip_nonfinite"]) for i, (n, net) in enumerate(nets)}

    def diagnostics(self, generator_only=False):
        """The statistics of each network's LAST optimiser step while armed, and of the critic's per-row slopes
        ||d sum(D(x_hat)) / d x_hat|| that the last critic update's gradient penalty left on the device:
            {"G": summary, "D": summary,                            diagnostics.summarise
             "gp_slope": {min, mean, max, share_above_1, nonfinite},
             "tensors": {"G": {name: row}, "D": {name: row}}}       diagnostics.tensor_rows (short TF names)
        Applies any deferred optimiser step first (data parallel: the step just taken is the one reported; gradients are identical
        across ranks after the all-reduce, so every rank sees the same network rows).  One device-to-host copy.
        generator_only=True: the report of the pretraining phase, where only G takes optimiser steps - {"G": summary,
        "tensors": {"G": ...}} (and "guard" with G's record where G is guarded); the critic is not read."""
        self.flush()
        if generator_only:
            gd = self.G.opt.get("diag")
            if gd is None or gd["last"] is None:
                raise RuntimeError("diagnostics(generator_only=True): no optimiser step of G has run while armed (arm_diagnostics first)")
            host = gd["rows"].view(-1).cpu().numpy()
            out = {"G": diagnostics.summarise(host, gd["names"], gd["numels"]), "tensors": {"G": diagnostics.tensor_rows(host, gd["names"])}}
            if self.G.has_guard:
                out["guard"] = {"G": self.G.guard_report()}
            return out
        gd, dd = self.G.opt.get("diag"), self.D.opt.get("diag")
        if gd is None or dd is None or gd["last"] is None or dd["last"] is None:
            raise RuntimeError("diagnostics(): no optimiser step of both networks has run while armed (arm_diagnostics first)")
        if getattr(self, "_slope_stats", None) is None:
            self._slope_stats = torch.empty(5, dtype=torch.float64, device=self.slopes.device)
        self.K.vector_stats(self.slopes, 1.0, out=self._slope_stats)
        host = torch.cat([gd["rows"].view(-1), dd["rows"].view(-1), self._slope_stats]).cpu().numpy()
        ng, nd = gd["rows"].numel(), dd["rows"].numel()
        rows = {"G": host[:ng], "D": host[ng:ng + nd]}
        mn, mx, total, above, bad = (float(x) for x in host[ng + nd:])
        finite = self.B - int(bad)
        out = {n: diagnostics.summarise(rows[n], st["names"], st["numels"]) for n, st in (("G", gd), ("D", dd))}
        out["gp_slope"] = {"min": mn if finite else None, "mean": total / finite if finite else None, "max": mx if finite else None,
                           "share_above_1": above / finite if finite else None, "nonfinite": int(bad)}
        out["tensors"] = {n: diagnostics.tensor_rows(rows[n], st["names"]) for n, st in (("G", gd), ("D", dd))}
        if self.G.has_guard or self.D.has_guard:
            # the rows above describe the unclipped gradient, and an update delta that a dropped step did not apply: the records say
            out["guard"] = self.guard_reports()
        return out

    def train_iteration(self, images, labels, noises, alphas, critic_iters=1, reuse_g_encoder=False, mle_weight=0.0, draws=None):
        """Loop body of train.py:362-368: critic_iters critic updates then one generator update on one minibatch,
        fresh noise / alpha per update.  reuse_g_encoder: G's encoder forward once per iteration (generator_forward).
        mle_weight > 0: the generator update carries the auxiliary likelihood term on `labels` (generator_step).
        draws[i]: the Gumbel draw number of update i (critic updates first, the generator update last; set_relaxation)."""
        mle = {"labels": labels, "mle_weight": mle_weight} if mle_weight > 0.0 else {}
        dr = (lambda i: {}) if draws is None else (lambda i: {"draw": draws[i]})
        with self.iteration(reuse_g_encoder):
            for i in range(critic_iters):
                self.critic_step(images, labels, noises[i], alphas[i], **dr(i))
            self.generator_step(images, noises[critic_iters], **mle, **dr(critic_iters))

    def train_iteration_accumulated(self, batches, noises, alphas, critic_iters=1, reuse_g_encoder=False, mle_weight=0.0, draws=None):
        """train_iteration with every update taken from N = len(batches) micro-batches of B rows: the update of the N * B rows.
        batches: [(images, labels)] * N, all resident on the device for the whole iteration (every update reads all of them);
        noises[i][k] / alphas[i][k]: update i (critic updates first, the generator update last), micro-batch k.  Order: per critic
        update all N micro-batches, then ONE optimiser step; then the generator update the same way.  reuse_g_encoder: G's encoder
        runs 2 N times per iteration instead of N * (critic_iters + 1) (generator_forward).  N = 1 is train_iteration.  draws[i][k]: as noises (train_iteration)."""
        N = len(batches)
        if N == 1:
            return self.train_iteration(batches[0][0], batches[0][1], [n[0] for n in noises], [a[0] for a in alphas],
                                        critic_iters, reuse_g_encoder, mle_weight, None if draws is None else [d[0] for d in draws])
        dr = (lambda i, k: {}) if draws is None else (lambda i, k: {"draw": draws[i][k]})
        with self.iteration(reuse_g_encoder):
            for i in range(critic_iters):
                for k, (images, labels) in enumerate(batches):
                    self.critic_step(images, labels, noises[i][k], alphas[i][k], micro=(k, N), **dr(i, k))
            for k, (images, labels) in enumerate(batches):
                mle = {"labels": labels, "mle_weight": mle_weight} if mle_weight > 0.0 else {}
                self.generator_step(images, noises[critic_iters][k], micro=(k, N), **mle, **dr(critic_iters, k))

    @contextlib.contextmanager
    def iteration(self, reuse_g_encoder=False):
        """The updates of ONE minibatch (train.py:362-368), or of one group of micro-batches.  reuse_g_encoder: see generator_forward."""
        self._g_reuse, self._g_reuse_armed = None, bool(reuse_g_encoder)
        self._g_reuse_slots = {}
        try:
            yield self
        finally:
            self._g_reuse, self._g_reuse_armed = None, False
            self._g_reuse_slots = {}

    def argmax_tokens(self, logits):
        """tf.argmax(fake_inputs, -1) (train.py:270)."""
        self.K.argmax_rows(logits, self.tokens.view(-1))
        return self.tokens
