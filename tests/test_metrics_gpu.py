"""-m gpu: scene-graph metrics - the matching kernel (csrc/match.hip, HipKernels.match_triples) against the dict-lookup reference
sgg_amd.metrics.match_reference, SceneGraphGAN.evaluate against predict() + match_reference + RecallAccumulator on the same model,
and train.py --metrics_out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sgg_amd.metrics import RecallAccumulator, match_reference, zero_shot_mask
from tests.test_eval_batched_gpu import _gan
from tests.test_predict_gpu import N_IMG, V, _count_trunk_forwards, _images, _untrained_gan, bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, SENTINEL = 98, -777


# ---- kernel ------------------------------------------------------------------------------------------------------------------
def guarded_outputs(nb, M):
    """pos and n_gt, each inside a larger buffer filled with a sentinel."""
    big, out = {}, {}
    for name, shape in (("pos", (nb, M)), ("n_gt", (nb,))):
        n = int(np.prod(shape))
        big[name] = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        out[name] = big[name][PAD:PAD + n].view(shape)
    return big, out


def ranked_lists(hip, nb, N, K, vocab, kind, seed):
    """The lists of a case from hip.rank_triples on random tokens (real -1 padding behind n_distinct): (device outputs cut at K, host
    copy of the FULL ranked list [nb, N, 3], n_distinct [nb])."""
    g = np.random.RandomState(seed)
    tokens = g.randint(0, vocab, size=(N, nb, 3)).astype(np.int64)
    if kind == "edges" and N >= 2:          # the packing edges: tokens 0 and V - 1 in all three slots
        tokens[0], tokens[1] = 0, vocab - 1
    elif kind in ("plain", "empty", "invalid"):
        tokens[N // 2:] = tokens[:N - N // 2]               # every triple twice: the lists are shorter than N
    d = (0.75 * g.randint(-4, 5, size=(N, nb, 3))).astype(np.float32)
    tok_d, d_d = torch.from_numpy(tokens).cuda(), torch.from_numpy(d).cuda()
    cut = hip.rank_triples(tok_d, d_d, K, vocab=vocab)
    full = hip.rank_triples(tok_d, d_d, N, vocab=vocab)
    return cut, full["triples"].cpu().numpy(), full["n_distinct"].cpu().numpy()


def build_ground_truth(g, full, nd, K, M, vocab, kind, empty):
    """One image's rows [M, 3] and its count, by construction (random triples at V = 50 almost never coincide with a prediction): a
    third from the image's own list at random positions, duplicates of earlier rows, the rest absent from the list, and behind the
    count a padding row that equals the image's top prediction.  kind "invalid": a row with token V and one with -5; "behind": one
    triple ranked behind K; "edges": the all-0 and all-(V - 1) triples."""
    U = min(int(nd), K)
    listed = set(map(tuple, full[:U].tolist()))
    count = 0 if empty else (M - 1 if M >= 2 else 1)
    rows = []
    if kind == "edges":
        rows += [[0, 0, 0], [vocab - 1] * 3]
    if kind == "behind":
        rows.append(full[K].tolist())
    if kind == "invalid":
        rows += [[1, 2, vocab], [3, -5, 4]]
    n_dup = 0 if count < 4 else (1 if count < 8 else 2)
    n_present = min(max(1, count // 3), U, max(0, count - n_dup - len(rows)))
    rows += full[g.choice(U, size=n_present, replace=False)].tolist()
    while len(rows) < count - n_dup:
        t = tuple(g.randint(0, vocab, size=3).tolist())
        if t not in listed:
            rows.append(list(t))
    rows = [rows[i] for i in g.permutation(len(rows))][:count]
    for _ in range(n_dup if rows else 0):
        src = int(g.choice([m for m, t in enumerate(rows) if all(0 <= x < vocab for x in t)]))
        rows.insert(int(g.randint(src + 1, len(rows) + 1)), list(rows[src]))
    assert len(rows) == count
    gt = np.empty((M, 3), dtype=np.int64)
    gt[:count] = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    gt[count:] = full[0]                    # padding that equals the top prediction: must be ignored
    return gt, count


# (nb, N, K, M, V, kind); kind "empty": the last image has gt_count = 0
CASES = [(1, 1, 1, 1, 5, "plain"), (3, 32, 32, 5, 50, "empty"), (4, 100, 37, 37, 50, "plain"), (2, 256, 100, 130, 1000, "invalid"),
         (5, 1000, 50, 64, 7, "behind"), (2, 300, 300, 9, 1 << 21, "edges"), (2, 4096, 4096, 4096, 70000, "plain")]


@pytest.mark.parametrize("case", CASES, ids=["nb%d-N%d-K%d-M%d-V%d-%s" % c for c in CASES])
def test_match_triples_equals_reference(hip, case):
    nb, N, K, M, vocab, kind = case
    cut, full, nd = ranked_lists(hip, nb, N, K, vocab, kind, seed=2000 + N + M)
    g = np.random.RandomState(7 + M)
    gts, counts = zip(*[build_ground_truth(g, full[j], nd[j], K, M, vocab, kind, empty=(kind == "empty" and j == nb - 1))
                        for j in range(nb)])
    gt, gt_count = np.stack(gts), np.asarray(counts, dtype=np.int32)
    want_pos, want_n = np.full((nb, M), -3, dtype=np.int32), np.zeros((nb,), dtype=np.int32)
    for j in range(nb):
        U = min(int(nd[j]), K)
        want_pos[j, :counts[j]], want_n[j] = match_reference(full[j, :U], gt[j, :counts[j]].tolist(), vocab=vocab)
    # input conditions of the case, from the reference alone
    if M >= 5:
        for code in (-1, -2, -3):
            assert (want_pos == code).any(), "the case has no row with code %d" % code
        assert (want_pos >= 0).any() and (want_pos[:, -1] == -3).all()
    if kind == "empty" or M == 4096:
        assert (nd < K).all(), "lists shorter than K: real -1 padding behind them"
    if kind == "empty":
        assert counts[-1] == 0 and want_n[-1] == 0
    if kind == "invalid":
        assert ((want_pos == -4).sum(axis=1) == 2).all()
    else:
        assert not (want_pos == -4).any()
    if kind == "behind":
        assert int(nd.min()) > K
        for j in range(nb):
            m = gt[j, :counts[j]].tolist().index(full[j, K].tolist())
            assert want_pos[j, m] == -1, "a triple ranked behind K counts as absent"
    if kind == "edges":
        for j in range(nb):
            rows = gt[j, :counts[j]].tolist()
            assert want_pos[j, rows.index([0, 0, 0])] >= 0 and want_pos[j, rows.index([vocab - 1] * 3)] >= 0
    assert np.array_equal(cut["triples"].cpu().numpy(), full[:, :K]) and (full[:, 0] >= 0).all()
    assert (cut["triples"].cpu().numpy() == -1).any() == bool((nd < K).any())       # (real -1 padding where a list is short)

    big, out = guarded_outputs(nb, M)
    gt_d, cnt_d = torch.from_numpy(gt).cuda(), torch.from_numpy(gt_count).cuda()
    res = hip.match_triples(cut["triples"], cut["n_distinct"], gt_d, cnt_d, vocab=vocab, out=out)
    torch.cuda.synchronize()
    got_pos, got_n = res["pos"].cpu().numpy(), res["n_gt"].cpu().numpy()
    assert np.array_equal(got_n, want_n), (got_n, want_n)
    assert np.array_equal(got_pos, want_pos), "pos differs in %d rows" % int((got_pos != want_pos).sum())
    for name, n in (("pos", nb * M), ("n_gt", nb)):
        flat = big[name].cpu().numpy()
        assert (flat[:PAD] == SENTINEL).all() and (flat[PAD + n:] == SENTINEL).all(), "%s: written outside its extent" % name
    again = hip.match_triples(cut["triples"], cut["n_distinct"], gt_d, cnt_d, vocab=vocab)       # outputs allocated by the binding
    assert np.array_equal(again["pos"].cpu().numpy(), got_pos) and np.array_equal(again["n_gt"].cpu().numpy(), got_n)


def test_match_triples_rejects_bad_arguments(hip):
    from sgg_amd.lib import SggError
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")
    for M, what in ((0, "M"), (4097, "4096")):
        with pytest.raises(SggError, match=what):
            hip.match_triples(i64(2, 8, 3), i32(2), i64(2, M, 3), i32(2))
    for K, what in ((0, "K"), (4097, "4096")):
        with pytest.raises(SggError, match=what):
            hip.match_triples(i64(2, K, 3), i32(2), i64(2, 4, 3), i32(2))
    with pytest.raises(SggError, match="V"):
        hip.match_triples(i64(2, 8, 3), i32(2), i64(2, 4, 3), i32(2), vocab=(1 << 21) + 1)
    lib = hip.lib
    ranked, nd, gt, cnt, pos, n_gt = i64(2, 8, 3), i32(2), i64(2, 4, 3), i32(2), i32(2, 4), i32(2)
    args = [ranked.data_ptr(), nd.data_ptr(), 2, 8, gt.data_ptr(), cnt.data_ptr(), 4, 50, pos.data_ptr(), n_gt.data_ptr(), None]
    for null_at in (0, 1, 4, 5, 8, 9):
        a = list(args)
        a[null_at] = None
        assert lib.sgg_match_triples(*a) == -1 and b"null" in lib.sgg_last_error()
    assert lib.sgg_match_triples(*args) == 0
    torch.cuda.synchronize()


# ---- SceneGraphGAN.evaluate ----------------------------------------------------------------------------------------------------
KS = (1, 10, 20, 32)


def _expected(preds, items, train):
    """match_reference + RecallAccumulator on predict()'s lists: (pos per image, metrics)."""
    acc, pos_all = RecallAccumulator(KS, V), []
    for p, (_, real) in zip(preds, items):
        pos, n_gt = match_reference(p["triples"][:max(KS)], real, vocab=V)
        acc.add(pos, real, zero_shot_mask(real, train))
        pos_all.append((pos.tolist(), n_gt))
    return pos_all, acc.result({i: "w%d" % i for i in range(V)})


def _same_metrics(got, want):
    for k in KS:
        for name in ("R@%d" % k, "mR@%d" % k, "zsR@%d" % k):
            assert got[name] is not None and abs(got[name] - want[name]) <= 1e-12, (name, got[name], want[name])
    assert sorted(got["predicates"]) == sorted(want["predicates"])
    for w, p in want["predicates"].items():
        q = got["predicates"][w]
        assert (q["index"], q["images"], q["triples"]) == (p["index"], p["images"], p["triples"])
        assert all(abs(q["recall"][k] - p["recall"][k]) <= 1e-12 for k in p["recall"])
    for name in ("images", "skipped_images", "invalid_triples", "zero_shot_images"):
        assert got[name] == want[name], name


def test_evaluate_matches_predict_and_reference(tmp_path):
    """Untrained model, batch_size 8: TEST_BATCH_SIZE 4, N = 32 samples per image, 5 images = one full and one padded image batch.
    Ground truth per image from predict() on the same model (the existing path): its best, worst and middle triple, the triple
    [V-1, V-1, V-1], the best once more, and a triple that is absent from the image's list by construction; the training set = the
    best triple of every image.

    [V-1, V-1, V-1] was meant as the absent row, but this model predicts it: the lists have 26, 26, 27, 26 and 30 triples and hold
    [49, 49, 49] at positions 21, 15, 9, 0 (the best triple of image 3: the row is a duplicate of row 0 there) and 12.  The row stays
    (its code is checked like any other), and the sixth row - the first [V-1, V-1, c], c = V-2, V-3, ..., that the list does not hold -
    carries the condition "the absent triple is absent in every image".  Ascending, the other picked positions are 0, nd - 1
    (25 .. 29) and nd // 2 (13 .. 15): R@1 = 0.21, R@20 = 0.54, R@32 = 0.79, zsR@32 = 2/3."""
    gan = _untrained_gan(tmp_path)
    imgs = _images()
    before = gan.predict(items=imgs)
    items = []
    for im, p in zip(imgs, before):
        L = p["triples"].tolist()
        absent = next([V - 1, V - 1, c] for c in range(V - 2, -1, -1) if [V - 1, V - 1, c] not in L)
        items.append((im, [L[0], L[-1], L[len(L) // 2], [V - 1, V - 1, V - 1], L[0], absent]))
    train = {tuple(p["triples"][0].tolist()) for p in before}
    want_pos, want = _expected(before, items, train)
    print("lists", [p["n_distinct"] for p in before], "expected", want_pos, {k: want[k] for k in want if "@" in k})
    # input conditions, from the expected values
    assert all(pos[5] == -1 and pos[4] == -2 and pos[3] >= -2 for pos, n in want_pos), "the absent triple is absent in every image"
    assert all(n == 4 + (pos[3] != -2) for pos, n in want_pos)
    assert want["R@1"] < want["R@20"] <= want["R@32"] < 1.0, want
    assert any(p["images"] >= 2 for p in want["predicates"].values())
    assert want["zsR@32"] is not None and want["zsR@32"] != want["R@32"]
    out_path = str(tmp_path / "metrics.json")
    got, calls = _count_trunk_forwards(gan, lambda: gan.evaluate(items=items, ks=KS, train_triples=train, return_details=True,
                                                                 out_path=out_path))
    assert calls == {"G": 2, "D": 2}, calls             # two image batches, one encoder pass per network each
    print({k: got[k] for k in got if "@" in k}, [d["n_distinct"] for d in got["details"]])
    assert len(got["details"]) == N_IMG
    for i, (d, (pos, n_gt), p) in enumerate(zip(got["details"], want_pos, before)):
        assert d["pos"] == pos and d["n_gt"] == n_gt and d["n_distinct"] == p["n_distinct"] and d["image"] == str(i), (i, d, pos)
    _same_metrics(got, want)
    assert got["ks"] == list(KS) and got["samples_per_image"] == 32 and got["ordering"] == "ascending mean critic score"
    assert abs(got["mean_n_distinct"] - np.mean([p["n_distinct"] for p in before])) <= 1e-12
    assert "distinct predictions, denominators |GT|" in got["definition"]
    assert json.load(open(out_path)) == json.loads(json.dumps(got))
    # without a training set zsR@K is None; without return_details no per-image record
    plain = gan.evaluate(items=items, ks=KS)
    assert "details" not in plain and plain["zsR@32"] is None and plain["R@20"] == got["R@20"]
    # descending: the reference on predict(descending=True), same ground truth
    desc = gan.predict(items=imgs, descending=True)
    dpos, dwant = _expected(desc, items, train)
    dgot = gan.evaluate(items=items, ks=KS, train_triples=train, return_details=True, descending=True)
    assert [(d["pos"], d["n_gt"]) for d in dgot["details"]] == dpos and dgot["ordering"] == "descending mean critic score"
    _same_metrics(dgot, dwant)
    assert [d["pos"] for d in dgot["details"]] != [d["pos"] for d in got["details"]]
    # predict() is what it was
    after = gan.predict(items=imgs)
    for p, q in zip(before, after):
        assert p["n_distinct"] == q["n_distinct"]
        for name in ("triples", "scores", "first_rank", "first_sample", "counts"):
            assert np.array_equal(bits(p[name]), bits(q[name])), name
    with pytest.raises(ValueError, match=r"\[0, 0, 50\]"):
        gan.evaluate(items=[(imgs[0], [[1, 2, 3], [0, 0, V]])], ks=KS)
    with pytest.raises(ValueError, match="4097"):
        gan.evaluate(items=[(imgs[0], [[0, 0, 0]]), (imgs[1], [[1, 2, 3]] * 4097)], ks=KS)


def test_metrics_out_cli(tmp_path):
    """train.py --metrics_out in fresh child processes: the JSON it writes is what evaluate() gives in-process on the loaded
    checkpoint; without a checkpoint it exits non-zero and writes nothing."""
    script = os.path.join(ROOT, "train.py")
    common = ["--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1", "--checkpoints_dir", str(tmp_path / "ck"),
              "--summaries_dir", str(tmp_path / "logs")]
    run = lambda extra: subprocess.run([sys.executable, script] + common + extra, cwd=str(tmp_path), capture_output=True, text=True,
                                       timeout=600)
    r = run(["--max_iterations", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "m.json"
    r = run(["--metrics_out", str(out), "--max_test_images", "2", "--metrics_k", "1,5"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "R@5" in r.stdout
    written = json.load(open(str(out)))
    gan = _gan(tmp_path, 8, 64, 50)
    assert gan.load_checkpoint()
    want = gan.evaluate(max_images=2, ks=(1, 5))
    assert written == json.loads(json.dumps(want))
    assert written["images"] == 2 and written["ks"] == [1, 5] and written["zsR@5"] is None and "R@1" in written and "mR@5" in written
    empty = tmp_path / "none"
    r = subprocess.run([sys.executable, script, "--synthetic", "8,64,50", "--batch_size", "8", "--metrics_out", str(empty / "m.json"),
                        "--checkpoints_dir", str(empty / "ck"), "--summaries_dir", str(empty / "logs")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "no checkpoint" in r.stderr
    assert not os.path.exists(str(empty / "m.json"))
