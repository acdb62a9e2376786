"""CPU: training-time augmentation (include/sgg_hip.h "training-time augmentation", sgg_amd/augment.py, tests/augment_ref.py).

The integer plan is pinned and checked for its invariants; the host fp32 path is compared bit for bit with the existing resize where the
definition promises it and with the fp64 restatement elsewhere; the CPU loader, the spec's parsing and train.py's flag are exercised."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from sgg_amd import augment as A
from sgg_amd.data import PrefetchLoader, resize_bilinear_tf1
from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS, STDS = np.array(R.DATASET_MEANS, np.float32), np.array(R.DATASET_STDS, np.float32)
ZERO, ONE = np.zeros(3, np.float32), np.ones(3, np.float32)
# the fp32 host path against fp64 on the 0..255 scale: a dozen fp32 roundings of values up to 2 * 255 (factor 1.999 before the clamp),
# each at most 2^-24 relative -> 12 * 510 * 6e-8 = 3.7e-4; the positions are the same fp32 numbers on both sides
HOST_TOL = 4e-4


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_pinned_table_rows():
    """Literal rows for fixed (seed, draw, H, W, spec): the restatement and the package's plan both give them."""
    spec = (0.3, 0.5, 0.2, 0.25, 0.999)
    cases = [(7, 0, 480, 640), (7, 2 ** 32 - 1, 480, 640), (7, 2 ** 32, 333, 500), (2 ** 40 + 5, 123456789012, 1, 7)]
    want_box = [[224, 40, 206, 478, 1, 0], [36, 330, 362, 210, 1, 0], [86, 121, 164, 342, 1, 0], [0, 2, 1, 5, 1, 0]]
    want_bits = [[0x3f8e8fa0, 0x3f8c3a38, 0x3e96166a, 0], [0x3f8d0c0e, 0x3f5982c4, 0x3e630236, 0],
                 [0x3f6e670c, 0x3f7fb68c, 0x3fda9991, 0], [0x3f8b697a, 0x3f877f87, 0x3fd30871, 0]]
    swap = np.arange(4)
    for (seed, draw, H, W), wb, wf in zip(cases, want_box, want_bits):
        img = np.zeros((H, W, 3), np.uint8)
        box, fac, _ = R.plan(spec, seed, draw, [img], [[0, 1, 2]], swap)
        assert box[0].tolist() == wb, (seed, draw, box[0].tolist())
        assert _bits(fac[0]).tolist() == wf, (seed, draw, [hex(v) for v in _bits(fac[0])])
        box2, fac2, _ = A.plan(A.AugmentSpec(*spec), seed, [draw], [H], [W], [[0, 1, 2]], swap, images=[img])
        assert np.array_equal(box2, box) and np.array_equal(_bits(fac2), _bits(fac))


def test_package_plan_equals_the_restatement_bit_for_bit():
    images = R.ref_images()
    B = len(images)
    words = R.TEST_WORDS
    swap = A.flip_swap_table(words)
    labels = np.array([[0, 1, 2], [5, 3, 0], [0, 4, 2], [2, 6, 5], [0, 1, 5], [2, 3, 2], [5, 4, 0], [0, 6, 2], [5, 1, 0]])
    for lo in (1.0, 0.3, 1.0 / 65536):
        spec = (lo, 0.9, 0.2, 0.3, 0.999)
        draw0 = 2 ** 32 - 3
        box, fac, lab = R.plan(spec, 11, draw0, images, labels, swap)
        box2, fac2, lab2 = A.plan(A.AugmentSpec(*spec), 11, [draw0 + b for b in range(B)], [im.shape[0] for im in images],
                                  [im.shape[1] for im in images], labels, swap, images=images)
        assert np.array_equal(box, box2) and np.array_equal(_bits(fac), _bits(fac2)) and np.array_equal(lab, lab2)
        if lo == 1.0:
            assert all(box[b, :4].tolist() == [0, 0, im.shape[0], im.shape[1]] for b, im in enumerate(images))
        # rows with the unmirrorable word (id 4) are never flipped and keep their labels; flipped rows exchange ids 1 and 3
        for b in range(B):
            if 4 in labels[b]:
                assert box[b, 4] == 0 and lab[b].tolist() == labels[b].tolist()
            elif box[b, 4]:
                assert lab[b].tolist() == [{1: 3, 3: 1}.get(int(l), int(l)) for l in labels[b]]
        assert box[:, 4].sum() >= 2 and any(box[b, 4] and (1 in labels[b] or 3 in labels[b]) for b in range(B))


def test_box_invariants_over_random_sizes():
    """10^5 random (H, W, lo) with the edge values forced in: the box lies inside the image, ch >= hmin, lo = 1 gives the image."""
    n = 100000
    rng = np.random.RandomState(3)
    H, W = rng.randint(1, 5000, n), rng.randint(1, 5000, n)
    lo_q = rng.randint(1, 65537, n)
    H[:2000], W[1000:3000] = 1, 1
    lo_q[::7], lo_q[3::11] = 65536, 1
    H[-3:], W[-3:] = 2 ** 31 - 1, 2 ** 31 - 1              # the largest sizes an int32 holds: 64-bit products
    draws = np.arange(n, dtype=np.uint64) + np.uint64(2 ** 32 - n // 2)
    zero = np.zeros(n, np.uint64)
    w = A.philox4x32(zero, zero, draws & np.uint64(A.M32), draws >> np.uint64(32), 5, A.KEY1)
    # extreme words as well: every quantity at both ends of its range
    for arr, val in ((w[0], 0), (w[1], A.M32), (w[2], A.M32), (w[3], 0)):
        arr[::13] = val
    for lq in np.unique(lo_q[:64]).tolist() + [1, 65536]:
        sel = lo_q == lq
        if not sel.any():
            continue
        y0, ch = A._interval(H[sel], lq, w[0][sel], w[1][sel])
        x0, cw = A._interval(W[sel], lq, w[2][sel], w[3][sel])
        hmin = np.maximum(1, (H[sel].astype(np.int64) * lq + 65535) >> 16)
        assert (y0 >= 0).all() and (ch >= hmin).all() and (y0 + ch <= H[sel]).all()
        assert (x0 >= 0).all() and (cw >= 1).all() and (x0 + cw <= W[sel]).all()
        if lq == 65536:
            assert (y0 == 0).all() and (x0 == 0).all() and (ch == H[sel]).all() and (cw == W[sel]).all()
    # the whole set through the scalar restatement's formula (vectorised over lo_q)
    Hl, Wl = H.astype(np.int64), W.astype(np.int64)
    hmin = np.maximum(1, (Hl * lo_q + 65535) >> 16)
    ch = hmin + (((Hl - hmin + 1) * (w[0] >> np.uint64(8)).astype(np.int64)) >> 24)
    y0 = ((Hl - ch + 1) * (w[1] >> np.uint64(8)).astype(np.int64)) >> 24
    assert (y0 >= 0).all() and (ch >= hmin).all() and (y0 + ch <= Hl).all()
    full = lo_q == 65536
    assert (ch[full] == Hl[full]).all() and (y0[full] == 0).all()
    for i in (0, 1500, 2500, n - 1, 13, 26):              # ... and single rows against the Python-integer restatement
        s, l, mn = R.interval(int(H[i]), int(lo_q[i]), int(w[0][i]), int(w[1][i]))
        assert (s, l) == (int(y0[i]), int(ch[i])) and l >= mn


def test_factors_stay_in_range_and_off_is_exactly_one():
    w = np.array([0, 1 << 9, A.M32, 0x80000000, 0x7fffffff], np.uint64)
    for a in (0.2, 0.999, 1.0 / 65536):
        q = R.quantise(a)
        f = A._factor(q, w)
        assert (f >= np.float32(1.0 - a)).all() and (f <= np.float32(1.0 + a)).all() and f.dtype == np.float32
        assert [R.factor(q, int(x)) for x in w] == f.tolist()
    assert A._factor(0, w).tolist() == [1.0] * 5 and R.factor(0, 12345) == 1.0


# ---- the host fp32 path -------------------------------------------------------------------------------------------------------------
def _img(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def test_all_off_equals_resize_and_standardise():
    img = _img(37, 53)
    got = A.augment_image(img, [0, 0, 37, 53, 0, 0], [1, 1, 1, 0], 0, MEANS, STDS, side=21)
    want = (resize_bilinear_tf1(img, 21, 21) - MEANS) / STDS
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))


def test_crop_equals_resize_of_the_slice_and_flip_mirrors():
    img = _img(50, 75, 1)
    for box in ([7, 11, 30, 41], [49, 74, 1, 1], [12, 0, 1, 75], [0, 40, 50, 1], [0, 0, 50, 75]):
        y0, x0, ch, cw = box
        got = A.augment_image(img, box + [0, 0], [1, 1, 1, 0], 0, MEANS, STDS, side=17)
        want = (resize_bilinear_tf1(np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw]), 17, 17) - MEANS) / STDS
        assert np.array_equal(_bits(got), _bits(want)), box
        flipped = A.augment_image(img, box + [1, 0], [1, 1, 1, 0], 0, MEANS, STDS, side=17)
        assert np.array_equal(_bits(flipped), _bits(np.flip(got, axis=1))), box
        assert np.abs(got.astype(np.float64) - R.augment(img, box + [0], [1, 1, 1, 0], 0, 17, 17, MEANS, STDS)).max() <= HOST_TOL / STDS.min()


def test_colour_stage_identities_and_clamp():
    img = _img(20, 24, 2)
    box = [0, 0, 20, 24, 0, 0]
    grey = A.augment_image(img, box, [1, 1, 0, 0], A.STAGE_SATURATION, ZERO, ONE, side=9)
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 1], grey[..., 2])
    m = A.grey_mean(img, box)
    flat = A.augment_image(img, box, [1, 0, 1, m], A.STAGE_CONTRAST, ZERO, ONE, side=9)
    assert (flat == m).all()
    hot = A.augment_image(img, box, [1.999, 1.999, 1.999, m], 7, ZERO, ONE, side=9)
    cold = A.augment_image(img, box, [0.001, 1.999, 1.999, m], 7, ZERO, ONE, side=9)
    assert hot.max() == 255.0 and hot.min() >= 0.0 and cold.min() == 0.0 and cold.max() <= 255.0
    assert (hot == 255.0).sum() > 10 and (A.augment_image(img, box, [1, 1.999, 1.999, m], 3, ZERO, ONE, side=9) == 0.0).sum() > 10


def test_grey_mean_is_the_integer_sum():
    img = _img(13, 9, 4)
    box = [2, 1, 10, 7, 0, 0]
    total = sum(77 * int(p[0]) + 150 * int(p[1]) + 29 * int(p[2]) for row in img[2:12, 1:8] for p in row)
    want = np.float32(np.float64(total) / np.float64(256 * 10 * 7))
    assert _bits(A.grey_mean(img, box)) == _bits(want) == _bits(R.grey_mean(img, 2, 1, 10, 7))


@pytest.mark.parametrize("amp", [0.2, 0.999])
def test_host_path_matches_the_fp64_restatement(amp):
    images = R.ref_images()
    swap = np.arange(3)
    labels = np.zeros((len(images), 3), np.int64)
    for lo in (1.0, 0.3, 1.0 / 65536):
        spec = (lo, 0.5, amp, amp, amp)
        box, fac, _ = R.plan(spec, 21, 2 ** 32 - 3, images, labels, swap)
        for means, stds in ((ZERO, ONE), (MEANS, STDS)):
            for b, img in enumerate(images):
                got = A.augment_image(img, box[b], fac[b], 7, means, stds, side=17)
                want = R.augment(img, box[b], fac[b], 7, 17, 17, means, stds)
                assert np.abs(got - want).max() <= HOST_TOL / stds.min(), (lo, b)
    # the ends of the factor range (amplitude 0.999), where the clamp works at both ends
    lo_f, hi_f = np.float32(1.0 - 0.999), np.float32(1.0 + 0.999)
    for row in ([hi_f, hi_f, hi_f], [lo_f, hi_f, hi_f], [hi_f, lo_f, lo_f], [lo_f, lo_f, hi_f]):
        for b, img in enumerate(images[3:6]):
            f = row + [A.grey_mean(img, [0, 0, img.shape[0], img.shape[1]])]
            got = A.augment_image(img, [0, 0, img.shape[0], img.shape[1], b & 1, 0], f, 7, ZERO, ONE, side=17)
            want = R.augment(img, [0, 0, img.shape[0], img.shape[1], b & 1], f, 7, 17, 17)
            assert np.abs(got - want).max() <= HOST_TOL, (row, b)


def test_bad_table_row_is_clamped():
    img = _img(10, 12, 5)
    ok = A.augment_image(img, [0, 0, 10, 12, 0, 0], [1, 1, 1, 0], 0, ZERO, ONE, side=7)
    for bad in ([-5, -9, 99, 1 << 30, 0, 0], [0, 0, 10 ** 9, 10 ** 9, 0, 0]):
        assert np.array_equal(A.augment_image(img, bad, [1, 1, 1, 0], 0, ZERO, ONE, side=7), ok)
    corner = A.augment_image(img, [1 << 30, 1 << 30, 0, -3, 0, 0], [1, 1, 1, 0], 0, ZERO, ONE, side=7)
    assert np.array_equal(corner, np.broadcast_to(img[9, 11].astype(np.float32), (7, 7, 3)))
    assert A.clamp_box([3, 4, 20, 20, 2, 0], 10, 12) == (0, 0, 10, 12, True)


# ---- labels under a flip ------------------------------------------------------------------------------------------------------------
def test_flip_swap_table():
    words = R.TEST_WORDS
    t = A.flip_swap_table(words)
    assert t.dtype == np.int32 and t.tolist() == [0, 3, 2, 1, -1, 5, 6]
    assert A.flip_swap_table({w: i for i, w in enumerate(words)}).tolist() == t.tolist()
    assert A.flip_swap_table(["left", "cat"]).tolist() == [-1, 1]
    assert A.flip_swap_table(["leftover", "upright", "left_hand", "right_hand", "copyright"]).tolist() == [0, 1, 3, 2, 4]
    with pytest.raises(ValueError):
        A.flip_swap_table({"a": 0, "b": 2})
    # "left" alone: a certain flip is cleared, the labels stay untouched
    img = _img(8, 8)
    box, _, lab = A.plan(A.AugmentSpec(flip=1.0), 0, [0, 1], [8, 8], [8, 8], [[1, 0, 1], [1, 1, 1]], A.flip_swap_table(["left", "cat"]),
                         images=[img, img])
    assert box[:, 4].tolist() == [0, 1] and lab.tolist() == [[1, 0, 1], [1, 1, 1]]


# ---- the spec ---------------------------------------------------------------------------------------------------------------------------
def test_spec_parsing_and_errors():
    s = A.AugmentSpec.parse("crop=0.5,flip=0.5,brightness=0.2,contrast=0.2,saturation=0.2")
    assert s.quantised() == (32768, 32768, 13107, 13107, 13107) and s.stages == 7
    assert A.AugmentSpec.parse(str(s)) == s and A.AugmentSpec.parse(s.as_dict()) == s and A.AugmentSpec.parse(s) is s
    d = A.AugmentSpec.parse("flip=1")
    assert d.quantised() == (65536, 65536, 0, 0, 0) and d.stages == 0
    assert A.AugmentSpec.parse(" saturation = 0.999 ").stages == A.STAGE_SATURATION
    for bad in ("", "crop", "crop=", "=1", "rotate=0.5", "crop=0", "crop=1.5", "crop=-1", "flip=1.1", "flip=-0.1", "brightness=1",
                "contrast=-0.2", "saturation=1.0", "brightness=0.9999999", "crop=abc", "crop=nan", "crop=0.5,crop=0.6", "crop=0.5;flip=1"):
        with pytest.raises(ValueError, match="augment"):
            A.AugmentSpec.parse(bad)


# ---- the CPU loader -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("augment_images")
    rng = np.random.RandomState(8)
    out = []
    for i in range(10):
        h, w = 9 + 3 * i, 30 - 2 * i
        p = str(d / ("im%02d.%s" % (i, "png" if i % 2 else "jpg")))
        arr = (rng.rand(h, w, 3) * 255).astype(np.uint8)
        Image.fromarray(arr if i != 4 else arr[..., 0]).save(p)        # (one grayscale file)
        out.append(p)
    return out


SPEC = "crop=0.4,flip=0.5,brightness=0.3,contrast=0.3,saturation=0.3"
LABELS = np.array([[0, 1, 2], [5, 3, 0], [0, 4, 2], [2, 6, 5], [0, 1, 5], [2, 3, 2], [5, 4, 0], [0, 6, 2], [5, 1, 0], [2, 1, 2]])


def _loader(files, B, n_it, start=0, rank=0, world=1, **kw):
    idx = lambda it: [((it * world + rank) * B + j) % len(files) for j in range(B)]
    if kw.get("augment") is not None:
        kw.update(rank=rank, world=world)
    return PrefetchLoader(files, LABELS, B, idx, MEANS, STDS, "cpu", n_it, start=start, workers=2, side=13, **kw)


def _batches(loader):
    with loader:
        return [(im.numpy().copy(), lb.numpy().copy()) for im, lb in loader]


def test_cpu_loader_is_deterministic_resumable_and_layout_independent(files):
    swap = A.flip_swap_table(R.TEST_WORDS)
    kw = dict(augment=SPEC, seed=3, swap=swap)
    a, b = _batches(_loader(files, 4, 5, **kw)), _batches(_loader(files, 4, 5, **kw))
    assert len(a) == 5
    for (ia, la), (ib, lb) in zip(a, b):
        assert np.array_equal(_bits(ia), _bits(ib)) and np.array_equal(la, lb)
    # the batches are what plan + augment_image give at draws it * B + j, the labels the plan's
    from sgg_amd.data import decode_rgb
    spec = A.AugmentSpec.parse(SPEC)
    flips = 0
    for it, (im, lb) in enumerate(a):
        for j in range(4):
            i = (it * 4 + j) % len(files)
            rgb = decode_rgb(files[i])
            box, fac, lab = A.plan(spec, 3, [it * 4 + j], [rgb.shape[0]], [rgb.shape[1]], [LABELS[i]], swap, images=[rgb])
            assert np.array_equal(_bits(im[j]), _bits(A.augment_image(rgb, box[0], fac[0], spec.stages, MEANS, STDS, side=13)))
            assert np.array_equal(lb[j], lab[0])
            assert np.abs(im[j] - R.augment(rgb, box[0], fac[0], 7, 13, 13, MEANS, STDS)).max() <= HOST_TOL / STDS.min()
            flips += int(box[0, 4])
    assert 0 < flips < 20 and not np.array_equal(np.concatenate([l for _, l in a]), LABELS[[k % 10 for k in range(20)]])
    # start = k gives batch k
    tail = _batches(_loader(files, 4, 5, start=3, **kw))
    assert len(tail) == 2 and all(np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1]) for x, y in zip(tail, a[3:]))
    # world 1 with B = 4 gives the rows of world 2 with B = 2
    halves = [_batches(_loader(files, 2, 5, rank=r, world=2, **kw)) for r in range(2)]
    for it in range(5):
        both_i, both_l = np.concatenate([halves[0][it][0], halves[1][it][0]]), np.concatenate([halves[0][it][1], halves[1][it][1]])
        assert np.array_equal(_bits(both_i), _bits(a[it][0])) and np.array_equal(both_l, a[it][1])
    # another seed draws other parameters
    other = _batches(_loader(files, 4, 1, augment=SPEC, seed=4, swap=swap))
    assert not np.array_equal(other[0][0], a[0][0])


def test_cpu_loader_without_augment_is_the_loader_as_it_was(files):
    plain, none = _batches(_loader(files, 3, 4)), _batches(_loader(files, 3, 4, augment=None, seed=9, rank=0, world=1))
    from sgg_amd.data import parse_image
    for it, ((ia, la), (ib, lb)) in enumerate(zip(plain, none)):
        assert np.array_equal(_bits(ia), _bits(ib)) and np.array_equal(la, lb)
        assert np.array_equal(la, LABELS[[(it * 3 + j) % 10 for j in range(3)]])
        assert np.array_equal(_bits(ia[0]), _bits(parse_image(files[(it * 3) % 10], MEANS, STDS, 13)))


def test_cpu_loader_with_worker_processes(files):
    kw = dict(augment=SPEC, seed=3, swap=A.flip_swap_table(R.TEST_WORDS))
    threads = _batches(_loader(files, 4, 1, **kw))
    idx = lambda it: [(it * 4 + j) % len(files) for j in range(4)]
    with PrefetchLoader(files, LABELS, 4, idx, MEANS, STDS, "cpu", 1, workers=2, side=13, processes=True, **kw) as loader:
        procs = [(im.numpy().copy(), lb.numpy().copy()) for im, lb in loader]
    assert np.array_equal(_bits(procs[0][0]), _bits(threads[0][0])) and np.array_equal(procs[0][1], threads[0][1])


# ---- train.py ---------------------------------------------------------------------------------------------------------------------------
def _train_module():
    sys.path.insert(0, ROOT)
    import train as T
    return T


def test_flag_is_parsed_and_rejected_with_synthetic():
    T = _train_module()
    assert T.build_parser().parse_args([]).augment is None
    assert T.parse_args(["--augment", SPEC]).augment == SPEC
    for bad in (["--augment", SPEC, "--synthetic", "2,32,11"], ["--augment", "rotate=1"], ["--augment", "crop=2"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    with pytest.raises(ValueError, match="synthetic"):
        T.SceneGraphGAN("ck", "logs", None, None, None, None, None, critic_iters=1, batch_size=2, lambda_=10, resume=False,
                        synthetic=(2, 32, 11), device="cpu", augment=SPEC)


@pytest.fixture
def real_train(files, tmp_path, monkeypatch):
    """train.SceneGraphGAN on ten small image files, on the CPU reference kernels, at 32 pixels (the constructor's 221 is the
    reference's; nothing below depends on the size) with a two-thread loader whose arguments are recorded."""
    from oracle.kernels_ref import RefKernels
    from sgg_amd import api
    T = _train_module()
    K = RefKernels()
    monkeypatch.setattr(T, "kernels_for", lambda device: K)
    monkeypatch.setattr(api, "kernels_for", lambda device: K)
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: None)
    seen = []

    def loader(*a, **kw):
        seen.append({k: kw.get(k) for k in ("augment", "seed", "rank", "world", "swap", "start")})
        kw.update(workers=2, processes=False, side=32)
        return PrefetchLoader(*a, **kw)
    monkeypatch.setattr(T, "PrefetchLoader", loader)
    words = R.TEST_WORDS + ["w%d" % i for i in range(4)]
    d = tmp_path / "data"
    d.mkdir()
    triples = {f: [LABELS[i].tolist(), LABELS[(i + 1) % 10].tolist()] for i, f in enumerate(files)}
    (d / "triples.json").write_text(json.dumps(triples))
    (d / "vocab.json").write_text(json.dumps({w: i for i, w in enumerate(words)}))
    np.save(str(d / "emb.npy"), (np.random.RandomState(0).rand(len(words), 300) * 0.2 - 0.1).astype(np.float32))
    (d / "means.txt").write_text("\n".join(str(x) for x in R.DATASET_MEANS) + "\n")
    (d / "stds.txt").write_text("\n".join(str(x) for x in R.DATASET_STDS) + "\n")

    def make(name, **kw):
        gan = T.SceneGraphGAN(str(tmp_path / name / "ck"), str(tmp_path / name / "logs"), str(d / "triples.json"), str(d / "vocab.json"),
                              str(d / "emb.npy"), str(d / "means.txt"), str(d / "stds.txt"), critic_iters=1, batch_size=2, lambda_=10,
                              device="cpu", **kw)
        gan.image_size = 32
        from sgg_amd.data import parse_image
        gan._parseFunction = lambda f: torch.from_numpy(parse_image(f, gan.image_means.numpy(), gan.image_stds.numpy(), 32))
        return gan
    return T, make, seen, words


def test_checkpoint_round_trip_and_contradicting_flag(real_train, tmp_path):
    T, make, seen, words = real_train
    gan = make("run", resume=False, augment=SPEC, seed=6)
    gan.train(max_iterations=1, log_every=1, validate_every=0, test_at_end=False)
    spec = A.AugmentSpec.parse(SPEC)
    assert seen[-1]["augment"] == spec and seen[-1]["seed"] == 6 and (seen[-1]["rank"], seen[-1]["world"]) == (0, 1)
    assert seen[-1]["swap"].tolist() == A.flip_swap_table(words).tolist()
    ck = torch.load(gan._ckpt_path())
    assert ck["augment"] == spec.as_dict()
    with open(str(tmp_path / "run" / "logs" / "losses.jsonl")) as f:
        recs = [json.loads(l) for l in f if l.strip()]
    assert [r for r in recs if "augment" in r] == [{"itr": 0, "augment": spec.as_dict()}]
    # resumed without the flag: the stored spec, the loader starts at the checkpoint's iteration
    rest = make("run", resume=True, seed=6)
    assert rest.augment is None
    rest.train(max_iterations=2, log_every=1, validate_every=0, test_at_end=False)
    assert rest.augment == spec and seen[-1]["augment"] == spec and seen[-1]["start"] == 1
    assert torch.load(rest._ckpt_path())["augment"] == spec.as_dict()
    same = make("run", resume=True, augment=SPEC, seed=6)
    assert same.load_checkpoint() and same.augment == spec
    # a contradicting flag is an error, on resume and at load
    with pytest.raises(ValueError, match="contradicts"):
        make("run", resume=True, augment="crop=0.5", seed=6).train(max_iterations=3, test_at_end=False)
    with pytest.raises(ValueError, match="contradicts"):
        make("run", resume=True, augment="flip=0.5", seed=6).load_checkpoint()
    # validation never augments: its batches are the plain pixels
    from sgg_amd.data import parse_image
    vi, _ = rest._val_batch(0)
    vf = rest.dataset["val"][0]
    st = rest._streams()["val"]
    j = st.batch(0, rest._val_rows(), 0, 1)[0]
    assert np.array_equal(vi[0].numpy(), parse_image(vf[j], rest.image_means.numpy(), rest.image_stds.numpy(), 32))


def test_run_without_the_flag_writes_no_key_and_refuses_it_later(real_train, tmp_path):
    T, make, seen, _ = real_train
    gan = make("plain", resume=False)
    gan.train(max_iterations=1, log_every=1, validate_every=0, test_at_end=False)
    assert seen[-1]["augment"] is None and seen[-1]["swap"] is None
    assert "augment" not in torch.load(gan._ckpt_path())
    assert "augment" not in open(str(tmp_path / "plain" / "logs" / "losses.jsonl")).read()
    with pytest.raises(ValueError, match="contradicts"):
        make("plain", resume=True, augment=SPEC).load_checkpoint()
