"""numpy restatement of csrc/augment.hip (definitions in include/sgg_hip.h, "training-time augmentation"): the integer plan on
tests/relax_ref.philox4x32, then crop, resample, mirror, colour and standardise in fp64.  Shared by tests/test_augment_cpu.py and
tests/test_augment_gpu.py; independent of sgg_amd/augment.py, which the CPU tests compare with it."""
import numpy as np

from tests.relax_ref import philox4x32

# Tolerance of the device's fp32 output against this fp64 restatement, on the 0..255 scale (means 0, stds 1); with other constants the
# error is brought back to that scale with the smallest std.  AUG_TOL = 10 x the largest error measured on the MI355X over the cases of
# tests/test_augment_gpu.py::test_all_stages_against_fp64 (nine images, three crop amplitudes, jitter amplitudes 0.2 and 0.999,
# hand-written factors at the ends of the range, output sizes 9x11, 17x33 and 221x221, both sets of constants), rounded up - the
# project's margin everywhere (tests/tolerances.py, tests/relax_ref.py).
#   AUG_ERR_MEASURED = 2.096e-4: image 7 (300 x 260) at 221 x 221 with all three factors at 1.999 and the dataset constants - values of
#   up to 2 x 255 before the clamp, each stage a fused multiply-add of such values (an fp32 ulp of 512 is 6.1e-5).
AUG_ERR_MEASURED = 2.1e-4
AUG_TOL = 2.1e-3

KEY1 = 0x41554731
M32 = 0xFFFFFFFF
DATASET_MEANS = (119.6, 115.1, 106.1)            # the dataset constants of tests/test_f1_f3_gpu.py, 0..255 scale
DATASET_STDS = (30.4, 30.5, 36.7)


def quantise(a):
    return int(round(float(a) * 65536))


def words(seed, draw):
    """The eight Philox words of one example: counters (0, 0, draw lo, draw hi) and (1, 0, draw lo, draw hi)."""
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    key = (seed & M32, ((seed >> 32) ^ KEY1) & M32)
    out = []
    for block in (0, 1):
        out += [int(w) for w in philox4x32((block, 0, draw & M32, draw >> 32), key)]
    return out


def interval(n, lo_q, w_len, w_pos):
    mn = max(1, (n * lo_q + 65535) >> 16)
    length = mn + (((n - mn + 1) * (w_len >> 8)) >> 24)
    return ((n - length + 1) * (w_pos >> 8)) >> 24, length, mn


def factor(a_q, w):
    if a_q == 0:
        return np.float32(1.0)
    return np.float32(np.int64((1 << 39) + a_q * (2 * (w >> 9) + 1 - (1 << 23)))) * np.float32(2.0 ** -39)


def grey_mean(img, y0, x0, ch, cw):
    px = np.asarray(img)[y0:y0 + ch, x0:x0 + cw].astype(object)          # Python integers: no width to overflow
    total = int((77 * px[..., 0] + 150 * px[..., 1] + 29 * px[..., 2]).sum())
    return np.float32(np.float64(total) / np.float64(256 * ch * cw))


def plan(spec, seed, draw0, images, labels, swap):
    """spec = (crop, flip, brightness, contrast, saturation) as real amplitudes -> box int32 [B,6], factors fp32 [B,4], labels int64 [B,3];
    plain Python integers, one example after the other."""
    crop_q, flip_q, bright_q, contrast_q, sat_q = (quantise(a) for a in spec)
    crop_q = max(crop_q, 1)
    B, V = len(images), len(swap)
    box, factors, out = np.zeros((B, 6), np.int32), np.zeros((B, 4), np.float32), np.array(labels, dtype=np.int64).reshape(B, 3)
    for b, img in enumerate(images):
        H, W = img.shape[:2]
        w = words(seed, (int(draw0) + b) & (2 ** 64 - 1))
        y0, ch, _ = interval(H, crop_q, w[0], w[1])
        x0, cw, _ = interval(W, crop_q, w[2], w[3])
        flip = (w[4] >> 16) < flip_q
        mapped = [int(swap[l]) if 0 <= l < V else -1 for l in out[b]]
        flip = flip and all(0 <= m < V for m in mapped)
        if flip:
            out[b] = mapped
        box[b] = (y0, x0, ch, cw, int(flip), 0)
        factors[b] = (factor(bright_q, w[5]), factor(contrast_q, w[6]), factor(sat_q, w[7]),
                      grey_mean(img, y0, x0, ch, cw) if contrast_q else 0.0)
    return box, factors, out


def axis_grid(n, out):
    """The legacy TF-1.x grid on n source pixels: positions in fp32 as the definition states them (scale = (float)n / out, every
    product rounded to fp32), so that floor() picks the pixels the kernels pick -> (lower, upper, weight as fp64)."""
    scale = np.float32(n) / np.float32(out)
    pos = (np.arange(out, dtype=np.float32) * scale).astype(np.float32)
    lo = np.floor(pos).astype(np.int64)
    return lo, np.minimum(lo + 1, n - 1), (pos - lo.astype(np.float32)).astype(np.float64)


def augment(img, box_row, factors_row, stages, oh, ow, means=(0.0, 0.0, 0.0), stds=(1.0, 1.0, 1.0)):
    """fp64 [oh, ow, 3] of one example for a VALID table row: crop, resample on the box, mirror, colour, clamp, standardise."""
    y0, x0, ch, cw, flip = (int(v) for v in box_row[:5])
    px = np.asarray(img)[y0:y0 + ch, x0:x0 + cw].astype(np.float64)
    ylo, yhi, wy = axis_grid(ch, oh)
    xlo, xhi, wx = axis_grid(cw, ow)
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = px[ylo][:, xlo] + (px[ylo][:, xhi] - px[ylo][:, xlo]) * wx
    bot = px[yhi][:, xlo] + (px[yhi][:, xhi] - px[yhi][:, xlo]) * wx
    v = top + (bot - top) * wy
    if flip:
        v = v[:, ::-1]
    if stages:
        bright, contrast, sat, mean = (np.float64(f) for f in factors_row)
        if stages & 1:
            g = (0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2])[..., None]
            v = g + sat * (v - g)
        if stages & 2:
            v = mean + contrast * (v - mean)
        if stages & 4:
            v = bright * v
        v = np.clip(v, 0.0, 255.0)
    return (v - np.asarray(means, np.float64)) / np.asarray(stds, np.float64)


def stage_mask(spec):
    return (1 if quantise(spec[4]) else 0) | (2 if quantise(spec[3]) else 0) | (4 if quantise(spec[2]) else 0)


# ---- the images of the GPU plan / resize tests: one-pixel sides, odd sizes, more than one block; pixels from a seed ------------------------
SIZES = ((1, 7), (40, 1), (5, 5), (13, 9), (37, 53), (50, 75), (221, 221), (300, 260), (700, 520))


def ref_images(seed=2024, sizes=SIZES):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]


def pack(images):
    """(packed uint8 [n], offsets int64 [B], heights int32 [B], widths int32 [B]) as the loader packs a batch."""
    offs = np.cumsum([0] + [im.size for im in images[:-1]]).astype(np.int64)
    return (np.concatenate([im.reshape(-1) for im in images]), offs, np.array([im.shape[0] for im in images], np.int32),
            np.array([im.shape[1] for im in images], np.int32))


# a vocabulary with a mirrored pair, an unrelated word and a `left` without its `right`
TEST_WORDS = ["man", "to the left of", "tree", "to the right of", "on left side", "dog", "next to"]
