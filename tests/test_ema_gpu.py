"""-m gpu: weight averaging on the device - the fused Adam + average kernel and the swap (csrc/optim.hip) against HipKernels.adam and
sgg_amd.ema.reference_update, step.Network with averaging on the two-stream schedule, averaged() (other batch sizes included) and
train.py --ema_decay / --eval_live.

Tolerances.  params, m, v, and everything the swap moves: bit-equal.  The average: 5 * 2^-24 * max(|e|, |p_new|) per update (three
fp32 roundings - the difference, at most 2 M; the product; the result, at most M - give (4 omd + 1) * 2^-24 * M; derived and checked
from the reference alone in tests/test_ema_cpu.py).  After k updates: k times that bound with M the largest magnitude among the
parameter snapshots so far (the average is a convex combination of them, and an earlier error is carried on scaled by decay <= 1)."""
import shutil

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from oracle import sgg_oracle as O
from sgg_amd import ema as E
from sgg_amd.lib import SggError
from sgg_amd.params import ADAM_B1, ADAM_B2, ADAM_EPS
from sgg_amd.step import GanStep, tf_adam_lr_t

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, -777.0
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4 * 256 * 4096 + 5]     # the last: a second trip of the grid-stride loop (4096 blocks)
U24 = 2.0 ** -24


def ema_bound(e, p):
    return 5.0 * U24 * np.maximum(np.abs(np.asarray(e, dtype=np.float64)), np.abs(np.asarray(p, dtype=np.float64)))


def guarded(host):
    """A device copy of `host` between two sentinel guards: (whole buffer, the view the kernel gets)."""
    n = host.size
    big = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    big[PAD:PAD + n].copy_(torch.from_numpy(host.view(np.float32)))
    return big, big[PAD:PAD + n]


def untouched(big, n):
    return bool((big[:PAD] == SENTINEL).all() and (big[PAD + n:] == SENTINEL).all())


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


# ---- fused kernel ---------------------------------------------------------------------------------------------------------------
def adam_inputs(n):
    """p, g, m, v, e: seeded, no zero, no subnormal."""
    r = np.random.RandomState(1000 + n % 9973)
    sign = lambda: np.where(r.rand(n) < 0.5, -1.0, 1.0)
    p = (sign() * r.uniform(1e-3, 1.0, n)).astype(np.float32)
    g = (sign() * r.uniform(1e-4, 8.0, n)).astype(np.float32)
    m = (sign() * r.uniform(1e-6, 1e-2, n)).astype(np.float32)
    v = r.uniform(1e-10, 1e-3, n).astype(np.float32)
    e = (sign() * r.uniform(1e-3, 1.0, n)).astype(np.float32)
    for a in (p, g, m, v, e):
        assert (np.abs(a) >= 1.2e-38).all(), "an input is zero or subnormal"
    return p, g, m, v, e


@pytest.mark.parametrize("n", SIZES)
def test_adam_ema_equals_adam_and_reference(hip, n):
    host = adam_inputs(n)
    lr_t = tf_adam_lr_t(3)
    for grad_scale in (1.0, 0.125):
        plain = [torch.from_numpy(a).cuda() for a in host[:4]]
        hip.adam(*plain, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, grad_scale)
        p_new = plain[0].cpu().numpy()
        assert not np.array_equal(p_new, host[0]) and np.array_equal(bits(plain[1]), host[1].view(np.int32))
        for omd in (0.9, 1e-3, 1.0, 0.0):
            pairs = [guarded(a) for a in host]
            bufs = [v for _, v in pairs]
            hip.adam_ema(*bufs, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, grad_scale, omd)
            torch.cuda.synchronize()
            what = "n %d grad_scale %g one_minus_decay %g" % (n, grad_scale, omd)
            assert all(untouched(big, n) for big, _ in pairs), "written outside a buffer: " + what
            for name, got, want in zip(("params", "m", "v"), (bufs[0], bufs[2], bufs[3]), (plain[0], plain[2], plain[3])):
                assert np.array_equal(bits(got), bits(want)), "%s differs from adam_kernel: %s" % (name, what)
            assert np.array_equal(bits(bufs[1]), host[1].view(np.int32)), "grads changed: " + what
            got = bufs[4].cpu().numpy()
            if omd == 0.0:
                assert np.array_equal(got.view(np.int32), host[4].view(np.int32)), "one_minus_decay 0 changed the average: " + what
            want = E.reference_update(host[4], p_new, np.float32(omd))
            err, bound = np.abs(got.astype(np.float64) - want), ema_bound(host[4], p_new)
            print("%s: worst %.2f units of 2^-24 * M" % (what, float((err / (bound / 5.0)).max())))
            assert (err <= bound).all(), "average outside the bound (%.2f x): %s" % (float((err / bound).max()), what)


def test_adam_ema_rejects_misaligned_and_overlapping_operands(hip):
    n = 64
    mk = lambda: torch.full((n,), 0.5, device="cuda")
    args = (1e-4, ADAM_B1, ADAM_B2, ADAM_EPS, 1.0, 0.5)
    off = lambda: torch.full((n + 4,), 0.5, device="cuda")[1:1 + n]
    for k in range(5):
        ops = [mk() for _ in range(5)]
        ops[k] = off()
        with pytest.raises(SggError, match="aligned"):
            hip.adam_ema(*ops, *args)
    for k in range(4):                                  # the average inside, behind and in front of every other operand
        for shift in (0, 4, -4):
            base = torch.full((2 * n + 8,), 0.5, device="cuda")
            ops = [mk() for _ in range(4)]
            ops[k] = base[8:8 + n]
            with pytest.raises(SggError, match="overlap"):
                hip.adam_ema(*ops, base[8 + shift:8 + shift + n], *args)
    ops = [mk() for _ in range(5)]
    with pytest.raises(SggError, match="one_minus_decay"):
        hip.adam_ema(*ops, *args[:5], 1.5)
    assert hip.lib.sgg_adam_tf_multi_ema(None, None, None, None, None, 4, 1e-4, 0.5, 0.9, 1e-8, 1.0, 0.5, None) == -1
    # adjacent ranges are not overlapping ones
    base = torch.full((2 * n,), 0.5, device="cuda")
    ops = [mk() for _ in range(3)]
    hip.adam_ema(base[:n], *ops, base[n:], *args)
    torch.cuda.synchronize()


# ---- swap -----------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x7fc00001, 0x7f800001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x7fffffff, 0xffc00000], dtype=np.uint32)


def swap_inputs(n):
    """Two int32 bit patterns of finite floats with NaNs of distinct payloads (quiet and signalling), +-Inf and -0.0 at both ends."""
    r = np.random.RandomState(7 + n % 9973)
    a = r.uniform(-4.0, 4.0, n).astype(np.float32).view(np.uint32).copy()
    b = r.uniform(-4.0, 4.0, n).astype(np.float32).view(np.uint32).copy()
    for k, i in enumerate(sorted(set(range(min(n, 8))) | set(range(max(0, n - 8), n)))):
        a[i], b[i] = SPECIALS[k % 8], SPECIALS[(k + 3) % 8]
    b[a == b] ^= 1                                      # (two draws that met: every element must change hands visibly)
    assert (a != b).all()
    return a.view(np.int32), b.view(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bit_for_bit(hip, n):
    a, b = swap_inputs(n)
    if n >= 16:
        assert all((a.view(np.uint32) == s).any() or (b.view(np.uint32) == s).any() for s in SPECIALS)
    (big_a, da), (big_b, db) = guarded(a), guarded(b)
    hip.swap(da, db)
    torch.cuda.synchronize()
    assert untouched(big_a, n) and untouched(big_b, n), "written outside a buffer"
    assert np.array_equal(bits(da), b) and np.array_equal(bits(db), a), "not exchanged exactly"
    hip.swap(da, db)
    torch.cuda.synchronize()
    assert np.array_equal(bits(da), a) and np.array_equal(bits(db), b), "twice is not the identity"
    assert untouched(big_a, n) and untouched(big_b, n)


def test_swap_rejects_overlap_and_misalignment(hip):
    n = 64
    base = torch.zeros(2 * n + 8, device="cuda")
    for shift in (0, 4, -4, n - 4):
        with pytest.raises(SggError, match="overlap"):
            hip.swap(base[8:8 + n], base[8 + shift:8 + shift + n])
    with pytest.raises(SggError, match="aligned"):
        hip.swap(base[1:1 + n], torch.zeros(n, device="cuda"))
    with pytest.raises(SggError, match="aligned"):
        hip.swap(torch.zeros(n, device="cuda"), base[3:3 + n])
    assert hip.lib.sgg_swap_f32(None, base.data_ptr(), 4, None) == -1 and hip.lib.sgg_swap_f32(base.data_ptr(), base.data_ptr(), 0, None) == -1
    hip.swap(base[:n], base[n:2 * n])                   # adjacent: fine
    torch.cuda.synchronize()


# ---- Network on the two-stream schedule -------------------------------------------------------------------------------------------
B, S, V = 4, 64, 50
ITERS, CRITIC_ITERS = 3, 2
_RUNS = {}


def _states():
    gp, dp = O.init_params("G", V, S, perturb=0.05), O.init_params("D", V, S, perturb=0.05)
    dp["W"] = dp["W"] * 25.0
    return gp, dp


def run(hip, decay):
    """ITERS iterations, G averaged with `decay` (None: never enabled): the step, G's snapshots (before, after each iteration), the
    average after each iteration and the losses.  One run per decay for the whole module."""
    if decay in _RUNS:
        return _RUNS[decay]
    gp, dp = _states()
    gs = GanStep(hip, V, S, B, lam=10.0, g_state=gp, d_state=dp, overlap_streams=True)
    if decay is not None:
        gs.G.enable_averaging(decay)
    images, labels, _ = O.synth_batch(B, S, V)
    img, lab = images.cuda(), labels.cuda()
    snaps, avgs, losses = [gs.G.arena.flat.cpu().numpy()], [], []
    for it in range(ITERS):
        noises = [O.synth_noise(B, 10 * it + i).cuda() for i in range(CRITIC_ITERS + 1)]
        alphas = [O.synth_alpha(B, 10 * it + i).reshape(B).cuda() for i in range(CRITIC_ITERS)]
        gs.train_iteration(img, lab, noises, alphas, critic_iters=CRITIC_ITERS)
        gs.flush()
        torch.cuda.synchronize()
        snaps.append(gs.G.arena.flat.cpu().numpy())
        losses.append(torch.cat([gs.d_losses, gs.g_losses]).cpu().numpy())
        if decay is not None:
            avgs.append(gs.G.opt["ema"]["flat"].cpu().numpy())
    _RUNS[decay] = (gs, snaps, avgs, losses)
    return _RUNS[decay]


@pytest.mark.parametrize("decay", [0.999, 0.05], ids=["warmup_branch", "constant_branch"])
def test_network_average_follows_the_recurrence_and_training_is_unchanged(hip, decay):
    gs, snaps, avgs, losses = run(hip, decay)
    twin, tsnaps, _, tlosses = run(hip, None)
    assert gs.G.opt["ema"]["updates"] == ITERS == gs.G.adam_t and "ema" not in gs.D.opt and "ema" not in twin.G.opt
    assert E.tf_ema_decay(decay, 0) == (0.1 if decay == 0.999 else 0.05)
    e, M = snaps[0].astype(np.float64), np.abs(snaps[0]).astype(np.float64)
    assert np.array_equal(avgs[0][gs.G.arena.live_numel:].view(np.int32), snaps[0][gs.G.arena.live_numel:].view(np.int32)), "dead tail"
    for k in range(1, ITERS + 1):
        assert not np.array_equal(snaps[k], snaps[k - 1]), "iteration %d left G's weights alone" % k
        e = E.reference_update(e, snaps[k], np.float32(E.one_minus_decay(decay, k - 1)))
        M = np.maximum(M, np.abs(snaps[k]).astype(np.float64))
        err, bound = np.abs(avgs[k - 1].astype(np.float64) - e), k * 5.0 * U24 * M
        print("decay %g, after iteration %d: worst %.2f of the bound" % (decay, k, float((err[bound > 0] / bound[bound > 0]).max())))
        assert (err <= bound).all(), "average after iteration %d outside %d x the bound" % (k, k)
    assert float(np.abs(e - snaps[-1]).max()) > 1e-6, "the average equals the last iterate"
    # training itself: bit-equal to the twin that never averaged
    for a, b in ((gs.G, twin.G), (gs.D, twin.D)):
        for name in ("m_flat", "v_flat"):
            assert np.array_equal(bits(getattr(a, name)), bits(getattr(b, name))), "%s.%s" % (a.kind, name)
        assert np.array_equal(bits(a.arena.flat), bits(b.arena.flat)), a.kind + " weights"
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(losses, tlosses))
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(snaps, tsnaps))
    assert all(np.isfinite(x).all() for x in losses)


def test_averaged_on_the_device(hip):
    from architectures.generator_with_attention import Generator
    trained = run(hip, 0.999)[0]
    images, _, _ = O.synth_batch(B, S, V)
    img = images.cuda()
    noise = O.synth_noise(B, 77).cuda()
    # the trained state under the model objects (NetworkHandle): weights and average of the run above
    g = Generator(V)
    net = g._ensure(img)
    g.load_state_dict(trained.G.state_dict())
    assert not g.has_average
    net.enable_averaging(0.999)
    net.restore_average(trained.G.opt["ema"]["flat"], ITERS)
    assert g.has_average
    n = net.arena.live_numel
    live0, ema0 = bits(net.arena.flat).copy(), bits(net.opt["ema"]["flat"]).copy()
    assert not np.array_equal(live0[:n], ema0[:n])
    before = g.build_generator(img, False, noise).clone()
    sd_avg = g.state_dict(full_names=True, averaged=True)
    assert all(k.startswith("Generator/Generator/") for k in sd_avg)
    gp, dp = _states()
    fresh = GanStep(hip, V, S, B, lam=10.0, g_state=sd_avg, d_state=dp)
    want = fresh.generator_forward(img, noise)[0].OUT[0].clone()
    half = img[:2].contiguous()
    with g.averaged():
        assert np.array_equal(bits(net.arena.flat)[:n], ema0[:n]) and np.array_equal(bits(net.opt["ema"]["flat"])[:n], live0[:n])
        inside = g.build_generator(img, False, noise).clone()
        small = g.build_generator(half, False, noise[:2].contiguous()).clone()      # a batch size first used inside the context
        with pytest.raises(RuntimeError, match="averaged"):
            g.state_dict()
    torch.cuda.synchronize()
    assert np.array_equal(bits(inside), bits(want)), "the forward inside averaged() is not the forward on the averaged state dict"
    assert not np.array_equal(bits(inside), bits(before))
    fresh2 = GanStep(hip, V, S, 2, lam=10.0, g_state=sd_avg, d_state=dp)
    want2 = fresh2.generator_forward(half, noise[:2].contiguous())[0].OUT[0]
    assert np.array_equal(bits(small), bits(want2)), "a batch size first used inside averaged() did not see the averaged weights"
    assert np.array_equal(bits(net.arena.flat), live0) and np.array_equal(bits(net.opt["ema"]["flat"]), ema0), "not restored bit for bit"
    assert np.array_equal(bits(g.build_generator(img, False, noise)), bits(before)), "the forward after exit differs"
    live_small = g.build_generator(half, False, noise[:2].contiguous())
    assert not np.array_equal(bits(live_small), bits(small)), "the other batch size kept the averaged weights after exit"


# ---- train.py -------------------------------------------------------------------------------------------------------------------
def _gan(T, ck, logs, **kw):
    return T.SceneGraphGAN(str(ck), str(logs), None, None, None, None, None, critic_iters=2, batch_size=8, lambda_=10,
                           synthetic=(8, 64, 50), **kw)


def _lists(preds):
    return [(p["triples"].tolist(), p["scores"].view(np.int32).tolist(), p["counts"].tolist()) for p in preds]


def test_train_resume_and_evaluation_with_the_average(tmp_path, capsys):
    import json
    import train as T
    logs = tmp_path / "logs"
    # 3 iterations, save, resume, one more == 4 uninterrupted ones
    first = _gan(T, tmp_path / "ck", logs, resume=False, ema_decay=0.5)
    first.train(max_iterations=3)
    ck3 = torch.load(first._ckpt_path(), map_location="cpu")
    assert set(ck3["G_ema"]) == {"flat", "updates", "decay"} and ck3["G_ema"]["updates"] == 3 and ck3["G_ema"]["decay"] == 0.5
    assert "ema" not in first.step.D.opt and not first.step.D.has_average
    resumed = _gan(T, tmp_path / "ck", logs, resume=True, ema_decay=0.5)
    resumed.train(max_iterations=4)
    whole = _gan(T, tmp_path / "ck_whole", logs, resume=False, ema_decay=0.5)
    whole.train(max_iterations=4)
    torch.cuda.synchronize()
    assert resumed.itr == whole.itr == 4
    for key in ("G", "D"):
        a, b = getattr(resumed.step, key), getattr(whole.step, key)
        assert np.array_equal(bits(a.arena.flat), bits(b.arena.flat)), key + " weights differ after the resume"
        assert np.array_equal(bits(a.m_flat), bits(b.m_flat)) and np.array_equal(bits(a.v_flat), bits(b.v_flat)) and a.adam_t == b.adam_t
    ra, wa = resumed.step.G.opt["ema"], whole.step.G.opt["ema"]
    assert ra["updates"] == wa["updates"] == 4 and np.array_equal(bits(ra["flat"]), bits(wa["flat"])), "the average differs after the resume"
    n = whole.step.G.arena.live_numel
    assert not np.array_equal(bits(wa["flat"])[:n], bits(whole.step.G.arena.flat)[:n]), "the average equals the live weights"
    sd_avg = whole.g.state_dict(averaged=True)
    del first, resumed
    # a fresh instance without the flag evaluates the averaged checkpoint ...
    plain = _gan(T, tmp_path / "ck_whole", logs, resume=False)
    assert plain.load_checkpoint() and plain.evaluates_average and plain.step.G.opt["ema"]["updates"] == 4
    got = plain.predict(max_images=2)
    met = plain.evaluate(max_images=2, ks=(1, 5), out_path=str(tmp_path / "m.json"))
    assert met["generator_weights"] == "ema" and json.load(open(str(tmp_path / "m.json")))["generator_weights"] == "ema"
    graphs = plain.write_predictions(str(tmp_path / "graphs"), max_images=1)
    assert graphs["generator_weights"] == "ema" and sorted(graphs) == ["0", "generator_weights"]
    index = plain.write_saliency(str(tmp_path / "maps"), max_images=1)
    assert index["generator_weights"] == "ema" and json.load(open(str(tmp_path / "maps" / "index.json")))["generator_weights"] == "ema"
    assert np.array_equal(bits(plain.step.G.arena.flat), bits(whole.step.G.arena.flat)), "evaluation left the averaged weights in the arena"
    # ... as an instance whose live weights ARE the average does
    as_live = _gan(T, tmp_path / "ck_whole", logs, resume=False, eval_live=True)
    assert as_live.load_checkpoint() and not as_live.evaluates_average
    live = as_live.predict(max_images=2)
    live_met = as_live.evaluate(max_images=2, ks=(1, 5))
    assert "generator_weights" not in live_met and "generator_weights" not in as_live.write_saliency(str(tmp_path / "maps_live"), max_images=1)
    as_live.g.load_state_dict(sd_avg)
    want = as_live.predict(max_images=2)
    assert _lists(got) == _lists(want), "evaluation on the average differs from evaluation of the averaged state dict"
    assert _lists(live) != _lists(got), "live and averaged weights predict the same lists"
    # with eval_live the results are the live ones: those of the trained object's live weights, average ignored
    whole.eval_live = True
    assert _lists(whole.predict(max_images=2)) == _lists(live)
    whole.eval_live = False
    assert _lists(whole.predict(max_images=2)) == _lists(got)
    # a training run resumed without the flag drops the average, says so once, and writes a checkpoint without the key
    shutil.copytree(str(tmp_path / "ck_whole"), str(tmp_path / "ck_drop"))
    capsys.readouterr()
    dropped = _gan(T, tmp_path / "ck_drop", logs, resume=True)
    dropped.train(max_iterations=4)
    out = capsys.readouterr().out
    assert out.count("average of the generator weights is dropped") == 1 and not dropped.step.G.has_average
    ck = torch.load(dropped._ckpt_path(), map_location="cpu")
    assert "G_ema" not in ck and "noise_rng" not in ck and ck["itr"] == 4
    assert np.array_equal(bits(dropped.step.G.arena.flat), bits(whole.step.G.arena.flat))


def test_checkpoint_without_the_flag_has_no_average(tmp_path):
    import train as T
    gan = _gan(T, tmp_path / "ck", tmp_path / "logs", resume=False)
    gan.train(max_iterations=1)
    ck = torch.load(gan._ckpt_path(), map_location="cpu")
    assert set(ck) == {"itr", "G", "D", "G_adam", "D_adam", "val"} and not gan.step.G.has_average and not gan.evaluates_average
    assert "generator_weights" not in gan.evaluate(max_images=1, ks=(1,))
