"""GPU: csrc/augment.hip against tests/augment_ref.py and against the existing resize kernel (include/sgg_hip.h, "training-time
augmentation").  The plan is compared bit for bit with the numpy restatement; the crop-only output bit for bit with
sgg_resize_bilinear_tf1 on packed copies of the cropped pixels (the existing kernel is the oracle); a flip with the mirrored output; the
colour stages with the fp64 restatement within AUG_TOL.  Outputs start as NaN, with a canary behind dst and behind both tables."""
import ctypes

import numpy as np
import pytest
import torch

from tests import augment_ref as R

pytestmark = pytest.mark.gpu

SIZES_SMALL = ((9, 11), (17, 33))
BIG = (221, 221)
BIG_IMAGES = (7, 8)                     # the two images resized to 221 x 221: (300, 260) and (700, 520)
LABELS = np.array([[0, 1, 2], [5, 3, 0], [0, 4, 2], [2, 6, 5], [0, 1, 5], [2, 3, 2], [5, 4, 0], [0, 6, 2], [5, 1, 0]], np.int64)
CANARY = 64


@pytest.fixture(scope="module")
def images():
    return R.ref_images()


@pytest.fixture(scope="module")
def swap():
    import sgg_amd  # noqa: F401
    from sgg_amd.augment import flip_swap_table
    return flip_swap_table(R.TEST_WORDS)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _packed(imgs):
    return tuple(_cuda(x) for x in R.pack(imgs))


class Guarded:
    """A device array of `shape` followed by a canary: floats start as NaN, integers as a sentinel no kernel writes."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.fill = float("nan") if dtype.is_floating_point else -123456789
        self.mark = 7.5 if dtype.is_floating_point else 987654321
        self.buf = torch.full((n + CANARY,), self.fill, dtype=dtype, device="cuda")
        self.buf[n:] = self.mark
        self.t = self.buf[:n].view(shape)
        self.n = n

    def intact(self):
        return bool((self.buf[self.n:] == self.mark).all())

    def untouched(self):
        return bool(torch.isnan(self.t).all()) if self.t.dtype.is_floating_point else bool((self.t == self.fill).all())


def _tables(B):
    return Guarded((B, 6), torch.int32), Guarded((B, 4), torch.float32), Guarded((B, 3), torch.int64)


def _device_plan(hip, pk, spec, seed, draw0, swap, labels=LABELS):
    import sgg_amd  # noqa: F401
    from sgg_amd.augment import AugmentSpec
    B = pk[1].shape[0]
    box, fac, lab = _tables(B)
    hip.augment_plan(pk[0], pk[1], pk[2], pk[3], _cuda(labels[:B]), _cuda(swap), AugmentSpec(*spec).quantised(), seed, draw0, box.t, fac.t,
                     lab.t)
    torch.cuda.synchronize()
    assert box.intact() and fac.intact() and lab.intact(), "the plan wrote behind a table"
    return box.t, fac.t, lab.t


def _resize(hip, pk, box, fac, stages, oh, ow, means=(0.0, 0.0, 0.0), stds=(1.0, 1.0, 1.0)):
    B = pk[1].shape[0]
    out = Guarded((B, oh, ow, 3), torch.float32)
    hip.augment_resize(pk[0], pk[1], pk[2], pk[3], box if torch.is_tensor(box) else _cuda(np.asarray(box, np.int32)),
                       fac if torch.is_tensor(fac) else _cuda(np.asarray(fac, np.float32)), stages, out.t,
                       _cuda(np.asarray(means, np.float32)), _cuda(np.asarray(stds, np.float32)))
    torch.cuda.synchronize()
    assert out.intact(), "the resize wrote behind dst"
    assert not bool(torch.isnan(out.t).any()), "an output pixel was not written"
    return out.t


def _oracle(hip, imgs, boxes, oh, ow, means=(0.0, 0.0, 0.0), stds=(1.0, 1.0, 1.0)):
    """sgg_resize_bilinear_tf1 on packed copies of the cropped pixels."""
    crops = [np.ascontiguousarray(im[y0:y0 + ch, x0:x0 + cw]) for im, (y0, x0, ch, cw) in zip(imgs, [b[:4] for b in boxes])]
    pk = _packed(crops)
    out = torch.full((len(imgs), oh, ow, 3), float("nan"), device="cuda")
    hip.resize_bilinear_tf1(pk[0], pk[1], pk[2], pk[3], out, _cuda(np.asarray(means, np.float32)), _cuda(np.asarray(stds, np.float32)))
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,flip", [(1.0, 0.5), (0.3, 1.0), (1.0 / 65536, 0.5)])
def test_plan_equals_the_restatement(hip, images, swap, lo, flip):
    spec = (lo, flip, 0.2, 0.3, 0.999)
    draw0, seed = 2 ** 32 - 3, 11                        # rows 3.. cross the carry into the counter's high word
    pk = _packed(images)
    box, fac, lab = _device_plan(hip, pk, spec, seed, draw0, swap)
    wbox, wfac, wlab = R.plan(spec, seed, draw0, images, LABELS, swap)
    assert np.array_equal(box.cpu().numpy(), wbox), (box.cpu().numpy(), wbox)
    assert np.array_equal(fac.cpu().numpy().view(np.uint32), wfac.view(np.uint32)), (fac.cpu().numpy(), wfac)
    assert np.array_equal(lab.cpu().numpy(), wlab)
    if flip == 1.0:                                      # a blocked flip (word 4 has no mirror image) and remapped triples
        assert wbox[:, 4].tolist() == [0 if 4 in row else 1 for row in LABELS]
        assert wlab[0].tolist() == [0, 3, 2] and wlab[2].tolist() == LABELS[2].tolist()
    if lo == 1.0:
        assert all(wbox[b, :4].tolist() == [0, 0, im.shape[0], im.shape[1]] for b, im in enumerate(images))
    # with every jitter off the factors are exactly 1, the mean is not computed and no workspace is asked for
    box1, fac1, _ = _device_plan(hip, pk, (lo, flip, 0.0, 0.0, 0.0), seed, draw0, swap)
    assert np.array_equal(box1.cpu().numpy(), wbox) and fac1.cpu().numpy().tolist() == [[1.0, 1.0, 1.0, 0.0]] * len(images)


# ---- crop only: the existing kernel is the oracle ------------------------------------------------------------------------------------------
def _hand_boxes(imgs):
    """Four tables: a 1x1 box in the bottom-right corner, a one-row full-width box, a one-column full-height box, box = image."""
    return [[[im.shape[0] - 1, im.shape[1] - 1, 1, 1, 0, 0] for im in imgs],
            [[im.shape[0] // 2, 0, 1, im.shape[1], 0, 0] for im in imgs],
            [[0, im.shape[1] // 3, im.shape[0], 1, 0, 0] for im in imgs],
            [[0, 0, im.shape[0], im.shape[1], 0, 0] for im in imgs]]


@pytest.mark.parametrize("size", SIZES_SMALL + (BIG,))
def test_crop_only_equals_the_existing_kernel_on_the_cropped_pixels(hip, images, swap, size):
    oh, ow = size
    imgs = [images[i] for i in BIG_IMAGES] if size == BIG else images
    pk = _packed(imgs)
    means, stds = R.DATASET_MEANS, R.DATASET_STDS
    plan_box = _device_plan(hip, pk, (0.3, 0.0, 0.0, 0.0, 0.0), 5, 17, swap)[0].cpu().numpy().tolist()
    assert any(b[2] < im.shape[0] for b, im in zip(plan_box, imgs))
    ones = np.tile(np.array([1, 1, 1, 0], np.float32), (len(imgs), 1))
    for boxes in [plan_box] + _hand_boxes(imgs):
        got = _resize(hip, pk, boxes, ones, 0, oh, ow, means, stds)
        want = _oracle(hip, imgs, boxes, oh, ow, means, stds)
        assert torch.equal(_bits(got), _bits(want)), (size, boxes, float((got - want).abs().max()))


# ---- flip ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [0, 7])
def test_flip_is_the_mirrored_output(hip, images, swap, stages):
    pk = _packed(images)
    box, fac, _ = R.plan((0.3, 0.0, 0.2, 0.3, 0.4), 9, 100, images, LABELS, swap)
    flipped = box.copy()
    flipped[:, 4] = 1
    for oh, ow in SIZES_SMALL:
        plain = _resize(hip, pk, box, fac, stages, oh, ow, R.DATASET_MEANS, R.DATASET_STDS)
        mirrored = _resize(hip, pk, flipped, fac, stages, oh, ow, R.DATASET_MEANS, R.DATASET_STDS)
        assert torch.equal(_bits(mirrored), _bits(torch.flip(plain, dims=[2])))


# ---- all stages against fp64 -----------------------------------------------------------------------------------------------------------
def _cases(images, swap):
    """(label, box, factors, also at 221 x 221): the plan's tables for three crop amplitudes and jitter amplitudes 0.2 / 0.999, and hand-written
    factors at the ends of the range (amplitude 0.999), where the clamp works at both ends."""
    for lo in (1.0, 0.3, 1.0 / 65536):
        for amp in (0.2, 0.999):
            box, fac, _ = R.plan((lo, 0.5, amp, amp, amp), 21, 2 ** 32 - 3, images, LABELS, swap)
            yield "lo %g amp %g" % (lo, amp), box, fac, lo == 0.3
    lo_f, hi_f = np.float32(1.0 - 0.999), np.float32(1.0 + 0.999)
    box = np.array([[0, 0, im.shape[0], im.shape[1], b & 1, 0] for b, im in enumerate(images)], np.int32)
    for row in ([hi_f, hi_f, hi_f], [lo_f, hi_f, hi_f], [hi_f, lo_f, lo_f], [lo_f, lo_f, hi_f]):
        fac = np.array([row + [R.grey_mean(im, 0, 0, im.shape[0], im.shape[1])] for im in images], np.float32)
        yield "ends %s" % ([float(f) for f in row],), box, fac, row[1] == hi_f and row[0] == hi_f


def test_all_stages_against_fp64(hip, images, swap):
    """The largest error on the 0..255 scale is printed (AUG_ERR_MEASURED of tests/augment_ref.py is this figure on the MI355X)."""
    worst = (0.0, None)
    for means, stds in (((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (R.DATASET_MEANS, R.DATASET_STDS)):
        for label, box, fac, big in _cases(images, swap):
            for size in SIZES_SMALL + (BIG,):
                sel = list(BIG_IMAGES) if size == BIG else list(range(len(images)))
                if size == BIG and not big:
                    continue                                # (221 x 221: two images, three tables)
                imgs = [images[i] for i in sel]
                got = _resize(hip, _packed(imgs), box[sel], fac[sel], 7, size[0], size[1], means, stds).cpu().numpy().astype(np.float64)
                for k, im in enumerate(imgs):
                    want = R.augment(im, box[sel][k], fac[sel][k], 7, size[0], size[1], means, stds)
                    err = float(np.abs(got[k] - want).max()) * min(stds)          # on the 0..255 scale
                    if err > worst[0]:
                        worst = (err, (label, size, sel[k], stds))
    print("augment_resize: largest |device - fp64| on the 0..255 scale %.3e at %s" % worst)
    assert worst[0] <= R.AUG_TOL, worst


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_launches_give_equal_bits(hip, images, swap):
    pk = _packed(images)
    spec = (0.3, 0.5, 0.2, 0.3, 0.4)
    a, b = _device_plan(hip, pk, spec, 3, 2 ** 32 - 3, swap), _device_plan(hip, pk, spec, 3, 2 ** 32 - 3, swap)
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(a[2], b[2])
    x, y = (_resize(hip, pk, a[0], a[1], 7, 17, 33, R.DATASET_MEANS, R.DATASET_STDS) for _ in range(2))
    assert torch.equal(_bits(x), _bits(y))


# ---- the loader ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpegs(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("augment_jpegs")
    rng = np.random.RandomState(12)
    sizes = [(40, 60), (33, 21), (700, 520), (64, 64), (25, 90), (48, 30), (120, 80), (57, 57)]        # one above 640 x 480
    out = []
    for i, (h, w) in enumerate(sizes):
        arr = np.kron(rng.randint(0, 256, size=(-(-h // 4), -(-w // 4), 3)), np.ones((4, 4, 1)))[:h, :w].astype(np.uint8)
        p = str(d / ("im%d.jpg" % i))
        Image.fromarray(arr[..., 0] if i in (1, 5) else arr).save(p, quality=92)                      # two grayscale files
        out.append(p)
    return out


def test_prefetch_loader_on_the_device(hip, jpegs, swap):
    import sgg_amd  # noqa: F401
    from sgg_amd import augment as A
    from sgg_amd.data import PrefetchLoader, decode_rgb
    B, side, n_it = 3, 37, 7
    labels = LABELS[:len(jpegs)]
    means, stds = np.array(R.DATASET_MEANS, np.float32), np.array(R.DATASET_STDS, np.float32)
    spec = A.AugmentSpec.parse("crop=0.4,flip=0.5,brightness=0.3,contrast=0.3,saturation=0.3")
    idx = lambda it: [(it * B + j) % len(jpegs) for j in range(B)]

    def run():
        with PrefetchLoader(jpegs, labels, B, idx, means, stds, "cuda", n_it, workers=4, depth=2, side=side, augment=spec, seed=5,
                            swap=swap) as loader:
            out = [(im.cpu().numpy(), lb.cpu().numpy()) for im, lb in loader]
        return out
    first, second = run(), run()
    assert len(first) == n_it
    rgbs = [decode_rgb(p) for p in jpegs]
    flips = 0
    for it, (im, lb) in enumerate(first):
        assert np.array_equal(im.view(np.uint32), second[it][0].view(np.uint32)) and np.array_equal(lb, second[it][1])
        ids = idx(it)
        box, fac, lab = A.plan(spec, 5, [it * B + j for j in range(B)], [rgbs[i].shape[0] for i in ids], [rgbs[i].shape[1] for i in ids],
                               labels[ids], swap, images=[rgbs[i] for i in ids])
        assert np.array_equal(lb, lab)
        flips += int(box[:, 4].sum())
        for j, i in enumerate(ids):
            want = R.augment(rgbs[i], box[j], fac[j], 7, side, side, means, stds)
            assert np.abs(im[j] - want).max() <= R.AUG_TOL / stds.min(), (it, j)
    assert 0 < flips < n_it * B


# ---- argument errors -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_the_error_code_and_launch_nothing(hip, images, swap):
    from sgg_amd.lib import SggError
    pk = _packed(images[:3])
    B = 3
    box, fac, lab = _tables(B)
    lab_in, d_swap = _cuda(LABELS[:B]), _cuda(swap)
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(src=p(pk[0]), offsets=p(pk[1]), heights=p(pk[2]), widths=p(pk[3]), labels_in=p(lab_in), swap=p(d_swap), V=len(swap), B=B,
                crop_q=32768, flip_q=32768, bright_q=1000, contrast_q=1000, sat_q=1000, seed=1, draw0=0, box=p(box.t), factors=p(fac.t),
                labels_out=p(lab.t), ws=p(ws), ws_bytes=512, stream=None)
    bad = [dict(src=None), dict(box=None), dict(labels_out=None), dict(swap=None), dict(B=0), dict(V=0), dict(crop_q=0), dict(crop_q=65537),
           dict(flip_q=-1), dict(flip_q=65537), dict(bright_q=65536), dict(contrast_q=-1), dict(sat_q=1 << 20), dict(ws=None),
           dict(ws_bytes=8)]
    for change in bad:
        a = dict(good, **change)
        rc = hip.lib.sgg_augment_plan(*a.values())
        assert rc == -1 and b"sgg_augment_plan" in hip.lib.sgg_last_error(), change
    out = Guarded((B, 9, 11, 3), torch.float32)
    ms = _cuda(np.ones(3, np.float32))
    rgood = dict(src=p(pk[0]), offsets=p(pk[1]), heights=p(pk[2]), widths=p(pk[3]), box=p(box.t), factors=p(fac.t), stages=7, dst=p(out.t),
                 B=B, oh=9, ow=11, means=p(ms), stds=p(ms), stream=None)
    for change in (dict(src=None), dict(box=None), dict(factors=None), dict(dst=None), dict(B=0), dict(oh=0), dict(ow=-1), dict(stages=8),
                   dict(stages=-1), dict(means=None)):
        rc = hip.lib.sgg_augment_resize(*dict(rgood, **change).values())
        assert rc == -1 and b"sgg_augment_resize" in hip.lib.sgg_last_error(), change
    torch.cuda.synchronize()
    assert box.untouched() and fac.untouched() and lab.untouched() and out.untouched(), "a refused call launched something"
    assert box.intact() and fac.intact() and lab.intact() and out.intact()
    with pytest.raises(SggError):
        hip.augment_plan(pk[0], pk[1], pk[2], pk[3], lab_in, d_swap, (32768, 32768, 65536, 0, 0), 1, 0, box.t, fac.t, lab.t)
