"""Exponential moving average of a network's weights: the host side (schedule and fp64 restatement; no device code).

tf.train.ExponentialMovingAverage(decay, num_updates) keeps for every variable a shadow with

    shadow -= (shadow - variable) * (1 - min(decay, (1 + num_updates) / (10 + num_updates)))

after every optimiser step.  The warm-up of the schedule lets the first updates follow the variable closely (the first one with
decay 0.1) so that the initial weights, which the shadow starts from, fade out quickly; it is always on here.  The device applies
the update inside the optimiser pass (csrc/optim.hip, HipKernels.adam_ema); step.Network holds the buffer and the update count.
"""
from __future__ import annotations

import numpy as np


def tf_ema_decay(decay, num_updates):
    """The decay of the update that follows `num_updates` applied ones: min(decay, (1 + num_updates) / (10 + num_updates))."""
    decay, num_updates = float(decay), int(num_updates)
    if not 0.0 < decay < 1.0:
        raise ValueError("ema decay must lie strictly between 0 and 1 (got %r)" % (decay,))
    if num_updates < 0:
        raise ValueError("num_updates must not be negative (got %r)" % (num_updates,))
    return min(decay, (1.0 + num_updates) / (10.0 + num_updates))


def one_minus_decay(decay, num_updates):
    """1 - tf_ema_decay(...) in double: what the host passes to the kernel (which receives it rounded to fp32)."""
    return 1.0 - tf_ema_decay(decay, num_updates)


def reference_update(e, p_new, one_minus_decay):
    """fp64 restatement of one shadow update: e - (e - p_new) * one_minus_decay with every operation in double.  To compare with the
    device, pass what the device sees: e, p_new as fp32 arrays (the average before, the parameters after the optimiser step) and
    one_minus_decay rounded to fp32 (np.float32(...)); the inputs are widened exactly, nothing is rounded here."""
    e64, p64 = np.asarray(e).astype(np.float64), np.asarray(p_new).astype(np.float64)
    return e64 - (e64 - p64) * np.float64(one_minus_decay)
