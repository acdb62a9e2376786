"""-m gpu: the batched evaluation path - the attention kernel for many rows per image (csrc/head.hip attn_step_fwd_rows_kernel),
Generator.sample / Discriminator.score_samples (one encoder pass per image batch, N x B head rows), SceneGraphGAN.test() on them
and train.py --test_only.  References: oracle/kernels_ref.py (fp64), oracle/sgg_oracle.py, oracle/eval_ref.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import eval_ref as ER
from oracle import sgg_oracle as O
from tests.test_kernels_gpu import close, rnd
from tests.tolerances import MARGIN_FACTOR, logit_tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ratio_threshold():
    src = open(os.path.join(ROOT, "scene-graph-gan_amd", "csrc", "head.hip")).read()
    return int(re.search(r"#define ATTN_ROWS_MIN_RATIO (\d+)", src).group(1))


THR = _ratio_threshold()
ATTN_CASES = [(1, 256, 196, 1.0), (3, 64, 196, 1.0), (32, 256, 196, 1.0), (2, 32, 784, 1.0), (4, 16, 16, 1.0), (4, 64, 16, 1.0),
              (3, THR - 1, 196, 1.0), (3, THR, 196, 1.0), (5, 40, 196, 30.0)]


@pytest.mark.parametrize("case", ATTN_CASES, ids=["B%d-N%d-L%d-s%g" % c for c in ATTN_CASES])
def test_attention_step_many_rows_per_image(hip, ref, case):
    """Rows r = b + k*B of B images (N per image): alpha and z (into a column slice of a wider NaN-filled buffer) against fp64."""
    B, N, L, scale = case
    C, R = 512, B * N
    P, ctx = rnd((B, L), 30, scale), rnd((B, L, C), 31)
    ec = rnd((1, R, L), 32, scale)
    al_ref = torch.empty((1, R, L), dtype=torch.float64)
    z_ref = torch.empty((1, R, C), dtype=torch.float64)
    for b in range(B):                  # per image (rows b, b + B, ...): the reference gathers ctx per row
        a = torch.empty((1, N, L), dtype=torch.float64)
        zz = torch.empty((1, N, C), dtype=torch.float64)
        ref.attn_step_fwd(P[b:b + 1].double(), ec[:, b::B].double(), ctx[b:b + 1].double(), a, zz)
        al_ref[:, b::B], z_ref[:, b::B] = a, zz
    al = torch.full((1, R, L), float("nan"), device="cuda")
    zbuf = torch.full((1, R, C + 40), float("nan"), device="cuda")
    hip.attn_step_fwd(P.cuda(), ec.cuda(), ctx.cuda(), al, zbuf[:, :, :C])
    close(al, al_ref, what="alpha")
    close(zbuf[:, :, :C], z_ref, what="z")
    assert torch.isnan(zbuf[:, :, C:]).all(), "z written outside its column slice"


def _oracle_per_image(fn, p, images, per_image):
    """fn(p, feature map of N copies of image b, per_image[b]) for every image b (one oracle encoder pass per image)."""
    feat = O.encoder(p, images)
    out = []
    for b in range(images.shape[0]):
        n = per_image[b].shape[0]
        out.append(fn(p, feat[b:b + 1].expand(n, *feat.shape[1:]).contiguous(), per_image[b]))
    return torch.stack(out, dim=1)                       # [N, B, ...]


def test_generator_sample_matches_oracle():
    from architectures.generator_with_attention import Generator
    from sgg_amd.trunk import Trunk
    S, V, B, N = 64, 50, 3, 16
    gp = O.init_params("G", V, S)
    g = Generator(V)
    # the owner network at batch 4 (build_generator), sample() at batch 3 on the same weights
    im4, _, _ = O.synth_batch(4, S, V, seed_img=7)
    n4 = O.synth_noise(4, 5)
    close_logits = lambda a, r, what: _close_tol(a, r, logit_tol(float(r.abs().max())), what)
    close_logits(g.build_generator(im4.cuda(), True, noise=n4.cuda()), O.generator_forward(gp, im4, n4), "build_generator at B = 4")
    images, _, _ = O.synth_batch(B, S, V, seed_img=11)
    noise = torch.randn((N, B, 512), generator=torch.Generator().manual_seed(12))
    calls = []
    orig = Trunk.forward
    Trunk.forward = lambda self, *a, **kw: calls.append(kw.get("for_backward", a[1] if len(a) > 1 else True)) or orig(self, *a, **kw)
    try:
        logits = g.sample(images.cuda(), N, noise.cuda())
    finally:
        Trunk.forward = orig
    assert calls == [False], "one forward-only encoder pass expected, got %s" % calls
    assert tuple(logits.shape) == (N, B, 3, V)
    ref = _oracle_per_image(O.generator_head, gp, images, [noise[:, b] for b in range(B)])
    close_logits(logits, ref, "Generator.sample")
    assert tuple(g.alpha.shape) == (N * B, 16) and tuple(g.downsampled.shape) == (B, 4, 4, 512)
    # tokens: exact wherever the oracle's top-2 margin is resolved (MARGIN_FACTOR x the logit tolerance)
    toks = torch.empty((N, B, 3), dtype=torch.int64, device="cuda")
    g.net.K.argmax_rows(logits, toks.view(-1))
    top = ref.topk(2, dim=-1).values
    ok = (top[..., 0] - top[..., 1]) > MARGIN_FACTOR * logit_tol(float(ref.abs().max()))
    assert int(ok.sum()) >= 0.9 * ok.numel()
    assert torch.equal(toks.cpu()[ok], O.argmax_tokens(ref)[ok])
    # the head state of the sample rows carries no cotangent buffers and is not a training state
    st = g.net.head if g._last is None else g._last.head
    fo = [s for k, s in st._states.items() if k[2] == "forward-only"]
    assert len(fo) == 1 and fo[0].R == N * B and not hasattr(fo[0], "dOUT") and not hasattr(fo[0], "pgrad")
    # build_generator at batch 4 is unchanged afterwards
    close_logits(g.build_generator(im4.cuda(), True, noise=n4.cuda()), O.generator_forward(gp, im4, n4), "build_generator after sample")


def _close_tol(a, r, tol, what):
    err = float((a.detach().cpu().double() - r.double()).abs().max())
    assert err <= tol, "%s: %.3e > %.3e" % (what, err, tol)


@pytest.mark.parametrize("V,N", [(50, 16), (70000, 2)])
def test_discriminator_score_samples_matches_oracle(V, N):
    from architectures.discriminator_with_attention import Discriminator
    S, B = 64, 3 if V < 1000 else 2
    dp = O.init_params("D", V, S)
    d = Discriminator(V, dp["W"].clone())
    images, _, _ = O.synth_batch(B, S, V, seed_img=13)
    logits = torch.randn((N, B, 3, V), generator=torch.Generator().manual_seed(14))
    labels = torch.randint(0, V, (N, B, 3), generator=torch.Generator().manual_seed(15))
    onehot = torch.nn.functional.one_hot(labels, V).float()
    for what, x in (("logits", logits), ("one-hots", onehot)):
        out = d.score_samples(x.cuda(), images.cuda())
        assert tuple(out.shape) == (N, B, 3, 1)
        ref = _oracle_per_image(O.discriminator_head, dp, images, [x[:, b] for b in range(B)])
        _close_tol(out, ref, 1e-4 + 1e-4 * float(ref.abs().max()), "Discriminator.score_samples(%s, V = %d)" % (what, V))
    if V < 1000:       # G's own logits through the critic, as test() does
        from architectures.generator_with_attention import Generator
        g = Generator(V)
        gl = g.sample(images.cuda(), N, torch.randn((N, B, 512), generator=torch.Generator().manual_seed(16)).cuda())
        out = d.score_samples(gl, images.cuda())
        ref = _oracle_per_image(O.discriminator_head, dp, images, [gl[:, b].cpu() for b in range(B)])
        _close_tol(out, ref, 1e-4 + 1e-4 * float(ref.abs().max()), "Discriminator.score_samples(G.sample)")


def _gan(tmp_path, B, S, V):
    import train as T
    return T.SceneGraphGAN(str(tmp_path / "ck"), str(tmp_path / "logs"), None, None, None, None, None, critic_iters=1, batch_size=B,
                           lambda_=10, resume=False, synthetic=(B, S, V))


def test_batched_test_matches_per_image_oracle(tmp_path):
    """batch_size 8: TEST_BATCH_SIZE 4, N = 32 samples per image; 5 images = one full image batch and one padded one."""
    from sgg_amd.trunk import Trunk
    S, V = 64, 50
    gan = _gan(tmp_path, 8, S, V)
    assert gan.TEST_BATCH_SIZE == 4 and gan.TEST_BATCH_MULTIPLIER == 8
    gan.train(max_iterations=1, log_every=1000, test_at_end=False)
    gp, dp = gan.g.state_dict(full_names=False), gan.d.state_dict(full_names=False)
    g = torch.Generator().manual_seed(77)
    imgs = [torch.randn((S, S, 3), generator=g) for _ in range(5)]
    gen = torch.Generator().manual_seed(gan.seed + 123)           # today's stream: per image, 8 draws of [TEST_BATCH_SIZE, 512]
    noises = [[torch.randn((4, 512), generator=gen) for _ in range(8)] for _ in imgs]
    pre = [ER.evaluate_image(gp, dp, im, [[0, 0, 0]], ns) for im, ns in zip(imgs, noises)]
    items = []
    for im, p in zip(imgs, pre):
        order = np.argsort(p["scores"], kind="stable")
        items.append((im, [p["tokens"][order[0]].tolist(), p["tokens"][order[-1]].tolist(), [V - 1, V - 1, V - 1]]))
    calls = {"G": 0, "D": 0}
    orig = Trunk.forward

    def counting(self, *a, **kw):
        calls["G" if any(self is n.trunk for n in gan.g._nets.values()) else "D"] += 1
        return orig(self, *a, **kw)

    for literal in (False, True):
        calls.update(G=0, D=0)
        Trunk.forward = counting
        try:
            (r50, r100), details = gan.test(items=items, out_path=str(tmp_path / "recalls.txt"), reference_literal=literal,
                                            return_details=True)
        finally:
            Trunk.forward = orig
        assert calls == {"G": 2, "D": 2}, calls                   # two image batches, one encoder pass per network each
        assert len(details) == 5
        for d, p, (im, real), ns in zip(details, pre, items, noises):
            e = ER.evaluate_image(gp, dp, im, real, ns, literal=literal)
            assert np.array_equal(d["tokens"], e["tokens"])
            assert float(np.abs(d["scores"] - e["scores"]).max()) <= 1e-4 + 1e-4 * float(np.abs(e["scores"]).max())
            assert (d["r50"], d["r100"]) == (e["r50"], e["r100"])
        assert r50 == float(np.mean([d["r50"] for d in details])) and r100 == float(np.mean([d["r100"] for d in details]))
        lines = open(str(tmp_path / "recalls.txt")).read().splitlines()
        assert float(lines[0]) == r50 and float(lines[1]) == r100 and lines[2].startswith("# ordering:")
        assert ("reference_literal" in lines[2]) == literal


def test_test_only_cli(tmp_path):
    """train.py --test_only in fresh child processes: the recalls.txt it writes is what test() gives in-process on the loaded
    checkpoint; without a checkpoint it exits non-zero."""
    script = os.path.join(ROOT, "train.py")
    common = ["--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1", "--checkpoints_dir", str(tmp_path / "ck"),
              "--summaries_dir", str(tmp_path / "logs")]
    run = lambda extra, cwd: subprocess.run([sys.executable, script] + common + extra, cwd=str(cwd), capture_output=True, text=True,
                                            timeout=600)
    r = run(["--max_iterations", "1"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(str(tmp_path / "ck" / "model.ckpt.pt"))
    out = tmp_path / "eval"
    out.mkdir()
    r = run(["--test_only", "--max_test_images", "2"], out)
    assert r.returncode == 0, r.stderr[-3000:]
    got = (out / "recalls.txt").read_text()
    gan = _gan(tmp_path, 8, 64, 50)
    assert gan.load_checkpoint()
    gan.test(max_images=2, out_path=str(tmp_path / "inproc.txt"))
    assert got == (tmp_path / "inproc.txt").read_text()
    empty = tmp_path / "none"
    r = subprocess.run([sys.executable, script, "--synthetic", "8,64,50", "--batch_size", "8", "--test_only", "--checkpoints_dir",
                        str(empty / "ck"), "--summaries_dir", str(empty / "logs")], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "no checkpoint" in r.stderr
