"""Training-time image augmentation: the host side of csrc/augment.hip (definitions: include/sgg_hip.h, "training-time augmentation").

    AugmentSpec          the five amplitudes of --augment, parsed, validated and quantised to the 16-bit fixed point the library takes
    plan                 the per-example parameter table (box, factors, remapped labels) in numpy: integer arithmetic on Philox4x32-10
                         words and one int64 -> fp32 conversion per factor, the same bits as sgg_augment_plan
    augment_image        the fp32 host path of the CPU loader: crop, TF-1.x resize, mirror, colour, standardise for one table row
    flip_swap_table      word id -> id of the word with `left` and `right` exchanged (a mirrored image turns one into the other)

The reference has no augmentation (train.py:167-172); without a spec nothing here runs."""
from __future__ import annotations

import re

import numpy as np

from .data import IMAGE_SIDE, resize_bilinear_tf1

KEYS = ("crop", "flip", "brightness", "contrast", "saturation")
STAGE_SATURATION, STAGE_CONTRAST, STAGE_BRIGHTNESS = 1, 2, 4
KEY1 = 0x41554731                                  # "AUG1", xor-ed into the high key word: no relaxation launch shares the key
M32 = 0xFFFFFFFF
_U = np.uint64


class AugmentSpec:
    """crop = smallest side fraction of the crop box in (0, 1] (1 = off), flip = probability of a mirror in [0, 1] (0 = off),
    brightness / contrast / saturation = amplitude a in [0, 1): factor in [1 - a, 1 + a] (0 = off)."""

    def __init__(self, crop=1.0, flip=0.0, brightness=0.0, contrast=0.0, saturation=0.0):
        self.crop, self.flip = float(crop), float(flip)
        self.brightness, self.contrast, self.saturation = float(brightness), float(contrast), float(saturation)
        if not (0.0 < self.crop <= 1.0):
            raise ValueError("augment: crop must lie in (0, 1] (got %r)" % (crop,))
        if not (0.0 <= self.flip <= 1.0):
            raise ValueError("augment: flip must lie in [0, 1] (got %r)" % (flip,))
        for key in KEYS[2:]:
            a = getattr(self, key)
            if not (0.0 <= a < 1.0) or int(round(a * 65536)) > 65535:
                raise ValueError("augment: %s must lie in [0, 1) (got %r)" % (key, a))

    @classmethod
    def parse(cls, text):
        """"crop=0.5,flip=0.5,brightness=0.2,contrast=0.2,saturation=0.2" (any subset, any order) -> AugmentSpec; an AugmentSpec or a
        dict of the keys passes through."""
        if isinstance(text, cls):
            return text
        if isinstance(text, dict):
            items = list(text.items())
        else:
            items = []
            for part in str(text).split(","):
                key, eq, val = part.partition("=")
                if not eq or not key.strip() or not val.strip():
                    raise ValueError("augment: expected key=value, got %r" % (part,))
                items.append((key.strip(), val.strip()))
        kw = {}
        for key, val in items:
            if key not in KEYS:
                raise ValueError("augment: unknown key %r (known: %s)" % (key, ", ".join(KEYS)))
            if key in kw:
                raise ValueError("augment: %s given twice" % key)
            try:
                kw[key] = float(val)
            except (TypeError, ValueError):
                raise ValueError("augment: %s needs a number (got %r)" % (key, val))
            if not np.isfinite(kw[key]):
                raise ValueError("augment: %s needs a finite number (got %r)" % (key, val))
        return cls(**kw)

    def quantised(self):
        """(crop_q, flip_q, brightness_q, contrast_q, saturation_q): q = round(a * 65536), crop at least 1."""
        return (max(1, int(round(self.crop * 65536))),) + tuple(int(round(getattr(self, k) * 65536)) for k in KEYS[1:])

    @property
    def stages(self):
        """The stage mask of sgg_augment_resize: a stage whose quantised amplitude is 0 is not executed."""
        _, _, b, c, s = self.quantised()
        return (STAGE_SATURATION if s else 0) | (STAGE_CONTRAST if c else 0) | (STAGE_BRIGHTNESS if b else 0)

    def as_dict(self):
        return {k: getattr(self, k) for k in KEYS}

    def __eq__(self, other):
        return isinstance(other, AugmentSpec) and self.quantised() == other.quantised()

    def __hash__(self):
        return hash(self.quantised())

    def __str__(self):
        return ",".join("%s=%s" % (k, repr(getattr(self, k))) for k in KEYS)

    __repr__ = lambda self: "AugmentSpec(%s)" % self


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words -> four uint64 arrays."""
    c = [np.asarray(w, dtype=_U) & _U(M32) for w in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & M32, int(k1) & M32
    for _ in range(10):
        p0, p1 = _U(0xD2511F53) * c[0], _U(0xCD9E8D57) * c[2]
        c = [(p1 >> _U(32)) ^ c[1] ^ _U(k0), p1 & _U(M32), (p0 >> _U(32)) ^ c[3] ^ _U(k1), p0 & _U(M32)]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def _interval(n, lo_q, w_len, w_pos):
    n = np.asarray(n, dtype=np.int64)
    mn = np.maximum(1, (n * np.int64(lo_q) + 65535) >> 16)
    length = mn + (((n - mn + 1) * (w_len >> _U(8)).astype(np.int64)) >> 24)
    start = ((n - length + 1) * (w_pos >> _U(8)).astype(np.int64)) >> 24
    return start, length


def _factor(a_q, w):
    t = 2 * (w >> _U(9)).astype(np.int64) + 1 - (1 << 23)
    f = ((1 << 39) + np.int64(a_q) * t).astype(np.float32) * np.float32(2.0 ** -39)
    return f if a_q else np.ones_like(f)


def grey_mean(rgb, box_row):
    """The contrast pivot of one example: the integer sum of 77 R + 150 G + 29 B over the box / (256 ch cw) in fp64 -> fp32."""
    y0, x0, ch, cw = (int(v) for v in box_row[:4])
    px = np.asarray(rgb)[y0:y0 + ch, x0:x0 + cw].astype(np.int64)
    total = int((px * np.array([77, 150, 29], dtype=np.int64)).sum())
    return np.float32(np.float64(total) / np.float64(256 * ch * cw))


def plan(spec, seed, draws, heights, widths, labels=None, swap=None, images=None):
    """The table of sgg_augment_plan: box int32 [B, 6], factors float32 [B, 4], labels_out int64 [B, 3] (None without labels).
    draws: the examples' 64-bit stream positions.  swap: flip_swap_table(...) - with labels given, an example whose triple holds a
    word without a mirrored counterpart is not mirrored.  images: the uint8 arrays - needed for the grey mean when contrast is on."""
    crop_q, flip_q, bright_q, contrast_q, sat_q = AugmentSpec.parse(spec).quantised()
    seed = int(seed) & (2 ** 64 - 1)
    d = np.array([int(x) & (2 ** 64 - 1) for x in np.atleast_1d(draws)], dtype=_U)
    k0, k1 = seed & M32, (seed >> 32) ^ KEY1
    zero = np.zeros_like(d)
    w = philox4x32(zero, zero, d & _U(M32), d >> _U(32), k0, k1) + philox4x32(zero + _U(1), zero, d & _U(M32), d >> _U(32), k0, k1)
    y0, ch = _interval(heights, crop_q, w[0], w[1])
    x0, cw = _interval(widths, crop_q, w[2], w[3])
    flip = (w[4] >> _U(16)).astype(np.int64) < flip_q
    labels_out = None
    if labels is not None:
        labels = np.asarray(labels, dtype=np.int64).reshape(len(d), 3)
        swap = np.asarray(swap, dtype=np.int64)
        inside = (labels >= 0) & (labels < len(swap))
        mapped = np.where(inside, swap[np.where(inside, labels, 0)], -1)
        flip = flip & ((mapped >= 0) & (mapped < len(swap))).all(axis=1)
        labels_out = np.where(flip[:, None], mapped, labels)
    box = np.stack([y0, x0, ch, cw, flip.astype(np.int64), np.zeros_like(y0)], axis=1).astype(np.int32)
    factors = np.stack([_factor(bright_q, w[5]), _factor(contrast_q, w[6]), _factor(sat_q, w[7]),
                        np.zeros(len(d), np.float32)], axis=1).astype(np.float32)
    if contrast_q and images is not None:
        for b, img in enumerate(images):
            factors[b, 3] = grey_mean(img, box[b])
    return box, factors, labels_out


def clamp_box(box_row, H, W):
    """A table row clamped into its image, as every kernel that reads the table does: (y0, x0, ch, cw, flip)."""
    ch, cw = min(max(int(box_row[2]), 1), H), min(max(int(box_row[3]), 1), W)
    return min(max(int(box_row[0]), 0), H - ch), min(max(int(box_row[1]), 0), W - cw), ch, cw, int(box_row[4]) != 0


def augment_image(rgb, box_row, factors_row, stages, means, stds, side=IMAGE_SIDE):
    """One example of sgg_augment_resize on the host in fp32: rgb uint8 [H, W, 3] -> float32 [side, side, 3]."""
    rgb = np.asarray(rgb)
    y0, x0, ch, cw, flip = clamp_box(box_row, rgb.shape[0], rgb.shape[1])
    v = resize_bilinear_tf1(rgb[y0:y0 + ch, x0:x0 + cw], side, side)
    if flip:
        v = v[:, ::-1]
    if stages:
        bright, contrast, sat, mean = (np.float32(f) for f in factors_row)
        if stages & STAGE_SATURATION:
            g = (np.float32(0.299) * v[..., 0] + np.float32(0.587) * v[..., 1] + np.float32(0.114) * v[..., 2])[..., None]
            v = g + sat * (v - g)
        if stages & STAGE_CONTRAST:
            v = mean + contrast * (v - mean)
        if stages & STAGE_BRIGHTNESS:
            v = bright * v
        v = np.clip(v, np.float32(0.0), np.float32(255.0))
    return ((v - np.asarray(means, dtype=np.float32)) / np.asarray(stds, dtype=np.float32)).astype(np.float32)


def augment_example(rgb, spec, seed, draw, label, swap, means, stds, side=IMAGE_SIDE):
    """Plan + augment_image of one decoded example at stream position `draw`: (float32 [side, side, 3], int64 [3])."""
    spec = AugmentSpec.parse(spec)
    box, factors, labels_out = plan(spec, seed, [draw], [rgb.shape[0]], [rgb.shape[1]], [label], swap, images=[rgb])
    return augment_image(rgb, box[0], factors[0], spec.stages, means, stds, side), labels_out[0]


_SIDE_WORD = re.compile(r"(?<![A-Za-z0-9])(left|right)(?![A-Za-z0-9])")


def mirror_word(word):
    """`word` with the tokens left and right exchanged ("to the left of" -> "to the right of")."""
    return _SIDE_WORD.sub(lambda m: "right" if m.group(1) == "left" else "left", word)


def flip_swap_table(words):
    """int32 [V]: entry i = the id of word i with the tokens `left` / `right` exchanged; i itself for a word without them; -1 where
    the exchanged word is not in the vocabulary.  words: a {word: id} dict with ids 0 .. V - 1, or the words in id order."""
    vocab = dict(words) if isinstance(words, dict) else {w: i for i, w in enumerate(words)}
    table = np.full(len(vocab), -1, dtype=np.int32)
    if sorted(vocab.values()) != list(range(len(vocab))):
        raise ValueError("flip_swap_table: the ids must be 0 .. V - 1, each once")
    for word, i in vocab.items():
        table[i] = vocab.get(mirror_word(str(word)), -1)
    return table
