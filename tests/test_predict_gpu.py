"""-m gpu: scene-graph prediction - the ranking kernel (csrc/rank.hip, HipKernels.rank_triples) against a numpy reference of the
host ranking it replaces (stable argsort of the mean critic score, first occurrences, counts), SceneGraphGAN.predict against
test(return_details=True) on the same model, the attention of the ranked triples, and train.py --predict_dir."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import eval_ref as ER
from tests.test_eval_batched_gpu import _gan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("triples", "scores", "first_rank", "first_sample", "counts", "n_distinct", "sample_scores")


# ---- numpy reference ---------------------------------------------------------------------------------------------------------
def ref_scores(d):
    """d float32 [N, nb, 3] -> [N, nb]: the host path's `d_h.mean(axis=2)` of the [N, nb, 3, 1] critic outputs, in numpy float32."""
    N, nb = d.shape[:2]
    return d.reshape(N, nb, 3, 1).mean(axis=2).reshape(N, nb)


def ref_order(score, descending):
    """Ascending: SceneGraphGAN._rank's np.argsort(kind="stable").  Descending: the stable argsort of the negated scores (ties by the
    smaller sample index; a NaN stays a NaN, and numpy sorts NaN behind every number)."""
    return np.argsort(-score if descending else score, kind="stable")


def ref_rank_image(tokens, score, K, descending=False):
    """tokens [N, 3] int64, score [N] float32 -> the ranked distinct triples of one image, padded to K slots as the kernel pads."""
    order = ref_order(score, descending)
    first, count = {}, {}
    for r, k in enumerate(order):
        t = tuple(int(x) for x in tokens[k])
        if t not in first:
            first[t] = (r, int(k))
        count[t] = count.get(t, 0) + 1
    ranked = sorted(first.items(), key=lambda kv: kv[1][0])
    out = {"triples": np.full((K, 3), -1, dtype=np.int64), "scores": np.full((K,), np.nan, dtype=np.float32),
           "first_rank": np.full((K,), -1, dtype=np.int32), "first_sample": np.full((K,), -1, dtype=np.int32),
           "counts": np.zeros((K,), dtype=np.int32), "n_distinct": np.int32(len(ranked))}
    for u, (t, (r, k)) in enumerate(ranked[:K]):
        out["triples"][u], out["scores"][u], out["first_rank"][u], out["first_sample"][u], out["counts"][u] = t, score[k], r, k, count[t]
    return out


def ref_rank(tokens, d, K, descending=False):
    """tokens [N, nb, 3], d [N, nb, 3] -> dict of the kernel's outputs ([nb, ...])."""
    score = ref_scores(d)
    per = [ref_rank_image(tokens[:, j], score[:, j], K, descending) for j in range(tokens.shape[1])]
    out = {name: np.stack([p[name] for p in per]) for name in NAMES[:-1]}
    out["sample_scores"] = np.ascontiguousarray(score.T)
    return out


def test_reference_on_a_hand_written_case():
    tokens = np.array([[1, 2, 3], [4, 5, 6], [1, 2, 3], [7, 8, 9], [4, 5, 6], [1, 2, 3]], dtype=np.int64)
    score = np.array([0.5, -1.0, 0.25, np.nan, -1.0, 0.25], dtype=np.float32)
    r = ref_rank_image(tokens, score, 4)            # order: 1, 4 (tie: index), 2, 5, 0, 3 (NaN last)
    assert r["n_distinct"] == 3
    assert r["triples"].tolist() == [[4, 5, 6], [1, 2, 3], [7, 8, 9], [-1, -1, -1]]
    assert r["first_rank"].tolist() == [0, 2, 5, -1] and r["first_sample"].tolist() == [1, 2, 3, -1]
    assert r["counts"].tolist() == [2, 3, 1, 0]
    r = ref_rank_image(tokens, score, 2, descending=True)      # order: 0, 2, 5, 1, 4, 3 (NaN still last)
    assert r["n_distinct"] == 3 and r["triples"].tolist() == [[1, 2, 3], [4, 5, 6]]
    assert r["first_rank"].tolist() == [0, 3] and r["first_sample"].tolist() == [0, 1] and r["counts"].tolist() == [3, 2]


# ---- kernel ------------------------------------------------------------------------------------------------------------------
PAD = 97
SENTINEL = {torch.int64: -777, torch.int32: -777, torch.float32: 777.25}


def guarded_outputs(nb, N, K):
    """The kernel's outputs, each inside a larger buffer filled with a sentinel."""
    shapes = {"triples": ((nb, K, 3), torch.int64), "scores": ((nb, K), torch.float32), "first_rank": ((nb, K), torch.int32),
              "first_sample": ((nb, K), torch.int32), "counts": ((nb, K), torch.int32), "n_distinct": ((nb,), torch.int32),
              "sample_scores": ((nb, N), torch.float32)}
    big, out = {}, {}
    for name, (shape, dt) in shapes.items():
        n = int(np.prod(shape))
        off = PAD + (-PAD) % 2          # (an even element offset keeps every view 8-byte aligned)
        big[name] = torch.full((off + n + PAD,), SENTINEL[dt], dtype=dt, device="cuda")
        out[name] = big[name][off:off + n].view(shape)
    return big, out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def make_case(nb, N, V, kind, seed):
    g = np.random.RandomState(seed)
    tokens = g.randint(0, V, size=(N, nb, 3)).astype(np.int64)
    if kind == "one-triple":
        tokens[:] = np.array([V - 1, 0, V // 2], dtype=np.int64)
    if kind == "normal":
        d = g.standard_normal((N, nb, 3)).astype(np.float32)
    else:       # multiples of 0.75 in a small range: the three-step mean is exact and ties are frequent
        d = (0.75 * g.randint(-4, 5, size=(N, nb, 3))).astype(np.float32)
    if kind == "nan":
        for j in range(nb):
            rows = g.choice(N, size=min(N, 5), replace=False)
            d[rows, j, g.randint(0, 3, size=len(rows))] = np.nan
    return tokens, d


CASES = [(1, 1, 5, 1, "quant"), (3, 256, 50, 256, "quant"), (32, 256, 1000, 100, "quant"), (5, 100, 50, 100, "quant"),
         (2, 4096, 70000, 4096, "quant"), (4, 1000, 7, 50, "quant"), (3, 256, 50, 256, "one-triple"), (2, 1, 5, 1, "one-triple"),
         (3, 256, 50, 256, "normal"), (4, 1000, 7, 50, "nan"), (2, 300, 1000, 300, "nan")]


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("case", CASES, ids=["nb%d-N%d-V%d-K%d-%s" % c for c in CASES])
def test_rank_triples_matches_numpy_reference(hip, case, descending):
    nb, N, V, K, kind = case
    tokens, d = make_case(nb, N, V, kind, seed=1000 + N + nb)
    want = ref_rank(tokens, d, K, descending)
    if kind == "quant":         # input conditions of the case (from the reference alone)
        score = ref_scores(d)
        assert N < 8 or all(len(np.unique(score[:, j])) < N for j in range(nb)), "ties expected"
        if V == 7:
            assert int(want["n_distinct"].min()) > K and int(want["counts"].max()) > 1
    if kind == "one-triple":
        assert want["n_distinct"].tolist() == [1] * nb and want["counts"][:, 0].tolist() == [N] * nb
    if kind == "nan":
        assert np.isnan(want["sample_scores"]).any(axis=1).all()
    tok_d, d_d = torch.from_numpy(tokens).cuda(), torch.from_numpy(d).cuda()
    big, out = guarded_outputs(nb, N, K)
    res = hip.rank_triples(tok_d, d_d, K, descending=descending, want_sample_scores=True, vocab=V, out=out)
    torch.cuda.synchronize()
    for name in NAMES:
        got = res[name].cpu().numpy()
        assert np.array_equal(bits(got), bits(want[name])), "%s differs (%s)" % (name, case,)
        flat = big[name].cpu().numpy()
        n = got.size
        off = PAD + (-PAD) % 2
        s = SENTINEL[big[name].dtype]
        assert (flat[:off] == s).all() and (flat[off + n:] == s).all(), "%s: written outside its extent" % name
    # the scores are the host path's float32 mean, bit for bit
    assert np.array_equal(res["sample_scores"].cpu().numpy().view(np.uint32),
                          np.ascontiguousarray(d.reshape(N, nb, 3, 1).mean(axis=2).reshape(N, nb).T).view(np.uint32))
    # allocated by the binding, without sample_scores: same results; two calls are bit-equal
    again = hip.rank_triples(tok_d, d_d, K, descending=descending, vocab=V)
    assert "sample_scores" not in again
    for name in NAMES[:-1]:
        assert np.array_equal(bits(again[name].cpu().numpy()), bits(res[name].cpu().numpy())), name


def test_rank_triples_rejects_bad_arguments(hip):
    from sgg_amd.lib import SggError
    tok = torch.zeros((8, 2, 3), dtype=torch.int64, device="cuda")
    d = torch.zeros((8, 2, 3), device="cuda")
    for K in (0, 9):
        with pytest.raises(SggError, match="K"):
            hip.rank_triples(tok, d, K)
    with pytest.raises(SggError, match="V"):
        hip.rank_triples(tok, d, 8, vocab=(1 << 21) + 1)
    big = torch.zeros((4097, 1, 3), dtype=torch.int64, device="cuda")
    with pytest.raises(SggError, match="4096"):
        hip.rank_triples(big, torch.zeros((4097, 1, 3), device="cuda"), 4)
    lib = hip.lib
    args = [tok.data_ptr(), d.data_ptr(), 8, 2, 50, 8, 0] + [tok.data_ptr()] * 6 + [None, None]
    for null_at in (0, 1, 7, 12):
        a = list(args)
        a[null_at] = None
        assert lib.sgg_rank_triples(*a) == -1 and b"null" in lib.sgg_last_error()
    a = list(args)
    a[6] = 2
    assert lib.sgg_rank_triples(*a) == -1 and b"descending" in lib.sgg_last_error()


# ---- SceneGraphGAN.predict ------------------------------------------------------------------------------------------------------
S, V, N_IMG = 64, 50, 5


def _images():
    g = torch.Generator().manual_seed(77)
    return [torch.randn((S, S, 3), generator=g) for _ in range(N_IMG)]


def _untrained_gan(tmp_path):
    gan = _gan(tmp_path, 8, S, V)
    assert gan.TEST_BATCH_SIZE == 4 and gan.TEST_BATCH_MULTIPLIER == 8
    return gan


def _count_trunk_forwards(gan, fn):
    from sgg_amd.trunk import Trunk
    calls = {"G": 0, "D": 0}
    orig = Trunk.forward

    def counting(self, *a, **kw):
        calls["G" if any(self is n.trunk for n in gan.g._nets.values()) else "D"] += 1
        return orig(self, *a, **kw)

    Trunk.forward = counting
    try:
        res = fn()
    finally:
        Trunk.forward = orig
    return res, calls


def test_predict_matches_test_details(tmp_path):
    """Untrained model, batch_size 8: TEST_BATCH_SIZE 4, N = 32 samples per image; 5 images = one full and one padded image batch.
    The samples and scores of test() (the existing path: host copies, per-image Python ranking) through the numpy reference must
    give exactly what predict() returns: both run the same kernels on the same rows, so the scores are expected bit-equal.

    Input condition (asserted): every image has >= 2 distinct triples and at least one duplicated triple among its 32 samples.  On
    the CPU oracle with the default initial weights these images and this noise stream give 26, 26, 27, 26 and 30 distinct triples
    of 32 and gaps of 7e-6 .. 7.6e-4 between adjacent scores (no ties)."""
    gan = _untrained_gan(tmp_path)
    imgs = _images()
    gan._constructOps(gan._next_batch(0)[0])           # (builds both networks with their initial weights: no training)
    gp, dp = gan.g.state_dict(full_names=False), gan.d.state_dict(full_names=False)
    gen = torch.Generator().manual_seed(gan.seed + 123)
    noises = [[torch.randn((4, 512), generator=gen) for _ in range(8)] for _ in imgs]
    items = []
    for im, ns in zip(imgs, noises):        # real triples as in test_batched_test_matches_per_image_oracle: best, worst, absent
        p = ER.evaluate_image(gp, dp, im, [[0, 0, 0]], ns)
        order = np.argsort(p["scores"], kind="stable")
        items.append((im, [p["tokens"][order[0]].tolist(), p["tokens"][order[-1]].tolist(), [V - 1, V - 1, V - 1]]))
    (_, _), details = gan.test(items=items, out_path=str(tmp_path / "recalls.txt"), return_details=True)
    preds, calls = _count_trunk_forwards(gan, lambda: gan.predict(items=items))
    assert calls == {"G": 2, "D": 2}, calls             # two image batches, one encoder pass per network each
    assert len(preds) == N_IMG == len(details)
    for i, (p, dt, (_, real)) in enumerate(zip(preds, details, items)):
        want = ref_rank_image(dt["tokens"], dt["scores"], 32)
        nd = int(want["n_distinct"])
        print("image %d: n_distinct %d (predict %d), r50 %g r100 %g" % (i, nd, p["n_distinct"], dt["r50"], dt["r100"]))
        assert 2 <= nd < 32, "input condition: >= 2 distinct triples and a duplicate among the 32 samples (got %d)" % nd
        assert p["n_distinct"] == nd and p["image"] == str(i) and p["ordering"] == "ascending mean critic score"
        for name in ("triples", "first_rank", "first_sample", "counts", "scores"):
            assert p[name].shape[0] == nd
            assert np.array_equal(bits(p[name]), bits(want[name][:nd])), "image %d: %s" % (i, name)
        assert p["words"] == [["w%d" % t for t in row] for row in p["triples"].tolist()]
        assert [e["count"] for e in p["graph"]["edges"]] == p["counts"].tolist() and len(p["graph"]["edges"]) == nd
        realset = set(map(tuple, real))
        for k, key in ((50, "r50"), (100, "r100")):
            hit = {tuple(t) for t, r in zip(p["triples"].tolist(), p["first_rank"].tolist()) if r < k}
            assert len(hit & realset) / float(k) == dt[key]
        assert dt["r50"] > 0.0
    # top_k keeps the head of the same list
    top = gan.predict(items=items, top_k=3)
    for p, q in zip(preds, top):
        assert q["n_distinct"] == p["n_distinct"] and np.array_equal(q["triples"], p["triples"][:3])
        assert np.array_equal(bits(q["scores"]), bits(p["scores"][:3])) and len(q["graph"]["edges"]) == 3


def test_predict_descending(tmp_path):
    gan = _untrained_gan(tmp_path)
    items = _images()                                   # plain tensors
    _, details = gan.test(items=[(im, [[0, 0, 0]]) for im in items], out_path=None, return_details=True)
    preds = gan.predict(items=items, descending=True)
    for i, (p, dt) in enumerate(zip(preds, details)):
        want = ref_rank_image(dt["tokens"], dt["scores"], 32, descending=True)
        nd = int(want["n_distinct"])
        assert p["n_distinct"] == nd and p["ordering"] == "descending mean critic score"
        for name in ("triples", "first_rank", "first_sample", "counts", "scores"):
            assert np.array_equal(bits(p[name]), bits(want[name][:nd])), "image %d: %s" % (i, name)
        assert (np.diff(p["scores"]) <= 0).all()


def test_predict_attention(tmp_path):
    """attention[u] is the generator's attention of triple u's first-occurrence sample: rows first_sample * nb + j of g.alphas right
    after an identical g.sample call; every map is a softmax (sums to 1)."""
    gan = _untrained_gan(tmp_path)
    imgs = _images()
    preds = gan.predict(items=imgs, with_attention=True)
    plain = gan.predict(items=imgs)
    gen = torch.Generator().manual_seed(gan.seed + 123)
    nb, N = 4, 32
    for i0 in (0, 4):
        chunk = imgs[i0:i0 + nb]
        n = len(chunk)
        images = torch.stack(chunk + [chunk[-1]] * (nb - n)).cuda()
        noise = torch.zeros((N, nb, 512))
        for j in range(n):
            for p in range(8):
                noise[p * 4:(p + 1) * 4, j] = torch.randn((4, 512), generator=gen)
        gan.g.sample(images, N, noise.cuda())
        al = gan.g.alphas.cpu().numpy()                 # [N * nb, 3, L]
        assert al.shape == (N * nb, 3, 16)
        for j in range(n):
            p = preds[i0 + j]
            U = min(p["n_distinct"], N)
            assert p["attention"].shape == (U, 3, 4, 4) and p["attention"].dtype == np.float32
            rows = p["first_sample"].astype(np.int64) * nb + j
            assert np.array_equal(p["attention"].reshape(U, 3, 16), al[rows])
            assert float(np.abs(p["attention"].reshape(U, 3, 16).sum(axis=-1) - 1.0).max()) <= 1e-5
            assert np.array_equal(p["triples"], plain[i0 + j]["triples"]) and "attention" not in plain[i0 + j]


def test_predict_dir_cli(tmp_path):
    """train.py --predict_dir in fresh child processes: the files it writes are what predict() gives in-process on the loaded
    checkpoint; without a checkpoint it exits non-zero."""
    script = os.path.join(ROOT, "train.py")
    common = ["--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1", "--checkpoints_dir", str(tmp_path / "ck"),
              "--summaries_dir", str(tmp_path / "logs")]
    run = lambda extra, cwd: subprocess.run([sys.executable, script] + common + extra, cwd=str(cwd), capture_output=True, text=True,
                                            timeout=600)
    r = run(["--max_iterations", "1"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "out"
    r = run(["--predict_dir", str(out), "--max_test_images", "2"], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    index = json.load(open(str(out / "index.json")))
    assert sorted(index) == ["0", "1"]
    gan = _gan(tmp_path, 8, 64, 50)
    assert gan.load_checkpoint()
    preds = gan.predict(max_images=2, with_attention=True)
    assert len(preds) == 2
    for i, p in enumerate(preds):
        e = index[str(i)]
        assert e["file"] == "%06d.npz" % i and e["n_distinct"] == p["n_distinct"] and len(e["graph"]["edges"]) == e["n_distinct"]
        assert e["graph"] == json.loads(json.dumps(p["graph"]))
        z = np.load(str(out / e["file"]))
        assert int(z["n_distinct"]) == p["n_distinct"] and z["words"].tolist() == p["words"]
        for name in ("triples", "scores", "first_rank", "first_sample", "counts", "attention"):
            assert z[name].dtype == p[name].dtype and np.array_equal(bits(z[name]), bits(p[name])), name
    # the new flags: 16 samples per image, the best 3 triples, highest score first
    out2 = tmp_path / "out2"
    r = run(["--predict_dir", str(out2), "--max_test_images", "2", "--predict_samples", "16", "--top_k", "3", "--predict_descending"],
            tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    want = gan.predict(max_images=2, n_samples=16, top_k=3, descending=True)
    index2 = json.load(open(str(out2 / "index.json")))
    for i, p in enumerate(want):
        z = np.load(str(out2 / index2[str(i)]["file"]))
        assert z["triples"].shape[0] <= 3 and np.array_equal(z["triples"], p["triples"])
        assert np.array_equal(bits(z["scores"]), bits(p["scores"])) and index2[str(i)]["n_distinct"] == p["n_distinct"]
    empty = tmp_path / "none"
    r = subprocess.run([sys.executable, script, "--synthetic", "8,64,50", "--batch_size", "8", "--predict_dir", str(empty / "out"),
                        "--checkpoints_dir", str(empty / "ck"), "--summaries_dir", str(empty / "logs")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "no checkpoint" in r.stderr
    assert not os.path.exists(str(empty / "out" / "index.json"))
