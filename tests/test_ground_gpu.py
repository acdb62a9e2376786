"""-m gpu: grounded scene graphs - the three kernels of csrc/ground.hip (HipKernels.ground_assign / ground_pool / ground_resolve)
against the fp64 statement of their definitions (sgg_amd.ground.ground_reference), SceneGraphGAN.predict(ground=True) against the
same reference fed with the attention of an identical Generator.sample call, and train.py --predict_dir --ground.

Discrete outputs are compared exactly.  That is only meaningful when no decision of the reference sits at fp32 rounding distance
from its threshold, so every case asserts ON THE REFERENCE ALONE, before the GPU is touched: with margin = 8 (L + N + 2) 2^-24 no
same-token overlap lies within margin of `overlap`, and no cell of a node map lies within margin * max of box_frac * max.  The case
generator redraws its seed (at most 20 times) until both hold; no pair and no cell is ever left out of a comparison.

Float outputs, relative to the fp64 value: maps within 4 (n_pooled + 2) 2^-24 (sequential fp32 summation of non-negative terms),
node_map within 4 (node_weight + 2) 2^-24, node_center within 4 (L + 2) 2^-24."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sgg_amd  # noqa: F401
from sgg_amd import ground as G
from tests.test_eval_batched_gpu import _gan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
PAD = 98            # (even: every guarded view stays 8-byte aligned)
SENTINEL = {torch.int64: -777, torch.int32: -777, torch.float32: 777.25}
INT_NAMES = ("slot_of_sample", "members", "start", "n_pooled", "mention_node", "n_nodes", "node_word", "node_first", "node_weight",
             "node_mentions", "node_box")
FLOAT_NAMES = ("maps", "node_map", "node_center")


def shapes(nb, N, K, L):
    i32, i64, f32 = torch.int32, torch.int64, torch.float32
    return {"slot_of_sample": ((nb, N), i32), "members": ((nb, N), i32), "start": ((nb, K + 1), i32), "maps": ((nb, K, 3, L), f32),
            "n_pooled": ((nb, K), i32), "mention_node": ((nb, K, 2), i32), "n_nodes": ((nb,), i32), "node_word": ((nb, 2 * K), i64),
            "node_first": ((nb, 2 * K), i32), "node_weight": ((nb, 2 * K), i32), "node_mentions": ((nb, 2 * K), i32),
            "node_map": ((nb, 2 * K, L), f32), "node_box": ((nb, 2 * K, 4), i32), "node_center": ((nb, 2 * K, 2), f32)}


def guarded(nb, N, K, L):
    """Every output inside a larger buffer filled with a sentinel."""
    big, out = {}, {}
    for name, (shape, dt) in shapes(nb, N, K, L).items():
        n = int(np.prod(shape))
        big[name] = torch.full((PAD + n + PAD,), SENTINEL[dt], dtype=dt, device="cuda")
        out[name] = big[name][PAD:PAD + n].view(shape)
    return big, out


def sentinels_intact(big, out):
    for name, t in big.items():
        flat, n, s = t.cpu().numpy(), out[name].numel(), SENTINEL[t.dtype]
        assert (flat[:PAD] == s).all() and (flat[PAD + n:] == s).all(), "%s: written outside its extent" % name


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def draw_case(nb, N, K, Hf, Wf, V, kind, seed):
    """tokens [N, nb, 3], triples [nb, K, 3], n_distinct [nb], fallback [nb, K], alphas fp32 [N * nb, 3, L].

    Tokens come from at most four words, so duplicates abound.  Every distinct triple of an image has, per decoding step, one centre
    out of four candidates of its word: three in a row of adjacent cells and one far away.  A row is the softmax of a Gaussian blob
    (sigma 1 cell) around that centre plus noise, so the pooled maps of two triples overlap by about 0.95 (same centre), 0.6
    (adjacent: joined at 0.5), 0.3 (two apart: joined only through the one between - a chain) or ~0 (far: a split).  The list is
    the distinct triples in order of first appearance, cut at K.  The blob is floored at e^-40 of its peak: every value stays a
    normal fp32 number (the relative error bounds of this file presume that nothing underflows; a subnormal has no relative precision)."""
    g = np.random.RandomState(seed)
    L = Hf * Wf
    words = np.sort(g.choice(V, size=min(V, 4), replace=False)).astype(np.int64)
    if kind == "one-word":
        tokens = np.empty((N, nb, 3), np.int64)
        tokens[..., 0] = tokens[..., 2] = words[1]
        tokens[..., 1] = g.randint(0, V, size=(N, nb))
    else:
        sample_words = words[:-1] if kind == "kbest" and len(words) > 1 else words
        tokens = sample_words[g.randint(0, len(sample_words), size=(N, nb, 3))]
    yy, xx = np.mgrid[0:Hf, 0:Wf]
    alphas = np.empty((N * nb, 3, L), np.float32)
    triples = np.full((nb, K, 3), -1, np.int64)
    n_distinct, fallback = np.zeros((nb,), np.int32), np.full((nb, K), -1, np.int32)
    for j in range(nb):
        base = {int(w): (g.randint(0, Hf), g.randint(1, max(2, Wf - 1))) for w in words}
        far = {int(w): ((base[int(w)][0] + Hf // 2) % Hf, (base[int(w)][1] + Wf // 2) % Wf) for w in words}
        centre_of, first = {}, {}
        for k in range(N):
            t = tuple(int(x) for x in tokens[k, j])
            if t not in first:
                first[t] = k
                centre_of[t] = g.randint(0, 4, size=3)
            for s in range(3):
                c, (by, bx) = centre_of[t][s], base[t[s]]
                cy, cx = far[t[s]] if c == 3 else (by, min(max(bx + c - 1, 0), Wf - 1))
                z = np.maximum(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2), -40.0) + g.uniform(-0.1, 0.1, size=(Hf, Wf))
                e = np.exp(z - z.max())
                alphas[k * nb + j, s] = (e / e.sum()).ravel()
        ranked = sorted(first.items(), key=lambda kv: kv[1])
        n_distinct[j] = len(ranked)
        for u, (t, k) in enumerate(ranked[:K]):
            triples[j, u], fallback[j, u] = t, k
        if kind == "kbest":             # a third of the slots hold a triple that is no sample's: they pool their fallback row
            for u in range(0, min(len(ranked), K), 3):
                triples[j, u, 1] = words[-1]
                fallback[j, u] = g.randint(0, N)
        if kind == "one-word":          # V = 3 allows three distinct triples: the list REPEATS them (the smallest slot owns the samples,
            n_distinct[j] = K           # every other slot pools the row of a random sample)
            for u in range(K):
                triples[j, u] = (words[1], u % V, words[1])
                fallback[j, u] = g.randint(0, N)
    return tokens, triples, n_distinct, fallback, alphas


def margins_ok(ref, n_distinct, L, N, overlap, box_frac):
    margin = 8.0 * (L + N + 2) * EPS
    for ov in ref["overlaps"]:
        if len(ov) and np.abs(ov[:, 2] - overlap).min() <= margin:
            return False
    for j in range(len(n_distinct)):
        a = ref["node_map"][j, :int(ref["n_nodes"][j])]
        mx = a.max(axis=1, keepdims=True) if a.size else a
        if a.size and (np.abs(a - box_frac * mx) <= margin * mx).any():
            return False
    return True


_CASES = {}


def make_case(case, overlap=0.5, box_frac=0.5):
    """The case and its reference, drawn once per session; the seed is redrawn until the input condition holds."""
    if case not in _CASES:
        nb, N, K, Hf, Wf, V, kind = case
        for attempt in range(20):
            inputs = draw_case(nb, N, K, Hf, Wf, V, kind, seed=4000 + 97 * attempt + N + K)
            ref = G.ground_reference(*inputs, Hf, Wf, overlap, box_frac, vocab=V)
            if margins_ok(ref, inputs[2], Hf * Wf, N, overlap, box_frac):
                break
        else:
            pytest.fail("input error: no seed in 20 keeps every overlap and every cell off its threshold (%s)" % (case,))
        _CASES[case] = (inputs, ref)
    return _CASES[case]


def run_kernels(hip, inputs, Hf, Wf, V, overlap, box_frac, out, strided=False):
    tokens, triples, n_distinct, fallback, alphas = inputs
    L = Hf * Wf
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if strided:                     # the three steps as column slices of one wider buffer: row stride 3 (L + 5)
        buf = torch.full((alphas.shape[0], 3, L + 5), 9.0, device="cuda")
        buf[:, :, :L] = dev(alphas)
        views = [buf[:, t, :L] for t in range(3)]
        assert views[0].stride(0) == 3 * (L + 5) > L
    else:
        views = [dev(alphas[:, t]) for t in range(3)]
    tok, tri, nd, fb = dev(tokens), dev(triples), dev(n_distinct), dev(fallback)
    hip.ground_assign(tok, tri, nd, vocab=V, out=out)
    hip.ground_pool(views, out["members"], out["start"], fb, nd, out=out)
    hip.ground_resolve(out["maps"], tri, nd, out["n_pooled"], Hf, Wf, overlap, box_frac, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def rel_err(got, want, count):
    """max over the elements of |got - want| / (4 (count + 2) 2^-24 |want|): <= 1 is inside the bound."""
    bound = 4.0 * (count + 2.0) * EPS * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def compare(got, ref, L):
    for name in INT_NAMES:
        assert np.array_equal(got[name], ref[name]), name
    r_maps = rel_err(got["maps"], ref["maps"], ref["n_pooled"][:, :, None, None].astype(np.float64))
    r_node = rel_err(got["node_map"], ref["node_map"], np.maximum(ref["node_weight"], 0)[:, :, None].astype(np.float64))
    assert np.array_equal(np.isnan(got["node_center"]), np.isnan(ref["node_center"]))
    ok = ~np.isnan(ref["node_center"])
    r_cen = rel_err(got["node_center"][ok], ref["node_center"][ok], float(L))
    print("error / bound: maps %.3f  node_map %.3f  node_center %.3f" % (r_maps, r_node, r_cen))
    assert r_maps <= 1.0 and r_node <= 1.0 and r_cen <= 1.0, (r_maps, r_node, r_cen)


def splits_and_merges(ref, triples, n_distinct):
    """(an image where one word owns two nodes, an image where a node has two mentions)"""
    split = merge = False
    for j in range(len(n_distinct)):
        n = int(ref["n_nodes"][j])
        w = ref["node_word"][j, :n].tolist()
        split |= len(set(w)) < len(w)
        merge |= bool((ref["node_mentions"][j, :n] > 1).any())
    return split, merge


# (nb, N, K, Hf, Wf, V, kind)
CASES = [(1, 1, 1, 1, 1, 5, "plain"), (3, 32, 32, 4, 4, 50, "plain"), (2, 300, 50, 3, 4, 7, "plain"), (2, 256, 256, 14, 14, 1000, "plain"),
         (1, 64, 16, 28, 28, 50, "plain"), (1, 2048, 1024, 14, 14, 3, "one-word"), (2, 96, 40, 5, 7, 50, "strided"),
         (2, 128, 64, 6, 6, 50, "kbest")]


@pytest.mark.parametrize("case", CASES, ids=["nb%d-N%d-K%d-%dx%d-V%d-%s" % c for c in CASES])
def test_ground_kernels_match_reference(hip, case):
    nb, N, K, Hf, Wf, V, kind = case
    inputs, ref = make_case(case)
    tokens, triples, n_distinct, fallback, alphas = inputs
    L = Hf * Wf
    # input conditions of the case, from the reference alone
    if (N, K) != (1, 1):
        split, merge = splits_and_merges(ref, triples, n_distinct)
        assert split and merge, "the case must hold a word with two nodes and a node with two mentions (%s, %s)" % (split, merge)
    if kind == "kbest":
        U = np.minimum(n_distinct, K)
        empty = sum(int((ref["n_pooled"][j, :U[j]] == 0).sum()) for j in range(nb))
        assert empty * 3 >= int(U.sum()) and (ref["n_pooled"] > 1).any()
    if kind == "one-word":
        assert int(n_distinct[0]) == K == 1024 and len(ref["overlaps"][0]) == 2048 * 2047 // 2      # one group of 2048 mentions
    if K < N and kind == "plain" and V == 7:
        assert (n_distinct > K).all() and (ref["slot_of_sample"] == -1).any()                       # the cut by K drops samples
    big, out = guarded(nb, N, K, L)
    got = run_kernels(hip, inputs, Hf, Wf, V, 0.5, 0.5, out, strided=(kind == "strided"))
    sentinels_intact(big, out)
    compare(got, ref, L)
    # two launches into fresh buffers are bit-equal
    big2, out2 = guarded(nb, N, K, L)
    again = run_kernels(hip, inputs, Hf, Wf, V, 0.5, 0.5, out2, strided=(kind == "strided"))
    sentinels_intact(big2, out2)
    for name in INT_NAMES + FLOAT_NAMES:
        a, b = got[name], again[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), "%s differs between two launches" % name


def test_ground_bindings_allocate_their_outputs(hip):
    case = CASES[1]
    nb, N, K, Hf, Wf, V, _ = case
    inputs, ref = make_case(case)
    tokens, triples, n_distinct, fallback, alphas = inputs
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = hip.ground_assign(dev(tokens), dev(triples), dev(n_distinct), vocab=V)
    p = hip.ground_pool([dev(alphas[:, t]) for t in range(3)], a["members"], a["start"], dev(fallback), dev(n_distinct))
    r = hip.ground_resolve(p["maps"], dev(triples), dev(n_distinct), p["n_pooled"], Hf, Wf)
    got = {k: v.cpu().numpy() for d in (a, p, r) for k, v in d.items()}
    assert sorted(got) == sorted(shapes(nb, N, K, Hf * Wf))
    compare(got, ref, Hf * Wf)


def test_ground_kernels_reject_bad_arguments(hip):
    from sgg_amd.lib import SggError
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    nb, N, K, L = 1, 8, 4, 4
    tri, nd = z((nb, K, 3), torch.int64), z((nb,), torch.int32)
    maps, npool = z((nb, K, 3, L), torch.float32), z((nb, K), torch.int32)
    for kw in ({"overlap": 0.0}, {"overlap": 1.5}, {"overlap": float("nan")}):
        with pytest.raises(SggError, match="overlap"):
            hip.ground_resolve(maps, tri, nd, npool, 2, 2, **kw)
    with pytest.raises(SggError, match="box_frac"):
        hip.ground_resolve(maps, tri, nd, npool, 2, 2, box_frac=0.0)
    Kb = 1025
    with pytest.raises(SggError, match="1024"):
        hip.ground_resolve(z((nb, Kb, 3, 1), torch.float32), z((nb, Kb, 3), torch.int64), nd, z((nb, Kb), torch.int32), 1, 1)
    with pytest.raises(SggError, match="4096"):
        hip.ground_assign(z((4097, 1, 3), torch.int64), tri, nd)
    with pytest.raises(SggError, match="V"):
        hip.ground_assign(z((N, nb, 3), torch.int64), tri, nd, vocab=(1 << 21) + 1)
    lib, p = hip.lib, tri.data_ptr()
    args = [p, p, p, N, nb, K, 50, p, p, p, None]
    for null_at in (0, 1, 2, 7, 8, 9):
        a = list(args)
        a[null_at] = None
        assert lib.sgg_ground_assign(*a) == -1 and b"null" in lib.sgg_last_error()
    args = [p, p, p, L, p, p, p, p, N, nb, K, L, p, p, None]
    for null_at in (0, 2, 4, 6, 12, 13):
        a = list(args)
        a[null_at] = None
        assert lib.sgg_ground_pool(*a) == -1 and b"null" in lib.sgg_last_error()
    a = list(args)
    a[3] = L - 1
    assert lib.sgg_ground_pool(*a) == -1 and b"lda" in lib.sgg_last_error()
    args = [p, p, p, p, nb, K, 2, 2, 0.5, 0.5] + [p] * 9 + [None]
    for null_at in (0, 3, 10, 16, 18):
        a = list(args)
        a[null_at] = None
        assert lib.sgg_ground_resolve(*a) == -1 and b"null" in lib.sgg_last_error()
    a = list(args)
    a[5] = 1025
    assert lib.sgg_ground_resolve(*a) == -1 and b"1024" in lib.sgg_last_error()


# ---- SceneGraphGAN.predict(ground=True) ---------------------------------------------------------------------------------------------
S, V, N_IMG, NB, NS, HF = 64, 50, 5, 4, 32, 4
PARENT_KEYS = {"image", "n_distinct", "ordering", "triples", "scores", "first_rank", "first_sample", "counts", "words", "graph"}


def _images():
    g = torch.Generator().manual_seed(77)
    return [torch.randn((S, S, 3), generator=g) for _ in range(N_IMG)]


def _untrained_gan(tmp_path):
    gan = _gan(tmp_path, 8, S, V)
    assert gan.TEST_BATCH_SIZE == NB and gan.TEST_BATCH_MULTIPLIER == 8
    return gan


def _sampled(gan, imgs, N):
    """Per image: (argmax tokens [N, 3], attention [N, 3, L]) of Generator.sample calls identical to predict()'s (the noise stream of
    SceneGraphGAN._sample_batches: per image 8 draws of [4, 512], the first N rows used)."""
    gen = torch.Generator().manual_seed(gan.seed + 123)
    res = []
    for i0 in range(0, len(imgs), NB):
        chunk = imgs[i0:i0 + NB]
        n = len(chunk)
        images = torch.stack(chunk + [chunk[-1]] * (NB - n)).cuda()
        passes = -(-N // NB)
        noise = torch.zeros((passes * NB, NB, 512))
        for j in range(n):
            for p in range(passes):
                noise[p * NB:(p + 1) * NB, j] = torch.randn((NB, 512), generator=gen)
        logits = gan.g.sample(images, N, noise[:N].cuda())
        toks = logits.argmax(dim=-1).cpu().numpy()          # [N, NB, 3]
        al = gan.g.alphas.cpu().numpy()                     # [N * NB, 3, L]
        for j in range(n):
            res.append((toks[:, j], al[j::NB]))
    return res


def _reference(p, tokens, al, overlap, box_frac=0.5):
    """ground_reference of one predicted image: the record's ranked list, the given sample tokens and attention rows."""
    U = len(p["triples"])
    K = max(U, 1)
    tri = np.full((1, K, 3), -1, np.int64)
    tri[0, :U] = p["triples"]
    fb = np.full((1, K), -1, np.int32)
    fb[0, :U] = p["first_sample"]
    return G.ground_reference(tokens.reshape(-1, 1, 3), tri, np.array([U], np.int32), fb, al, HF, HF, overlap, box_frac, vocab=V)


def _check_record(p, ref, N, overlap):
    gr, U, n = p["grounding"], len(p["triples"]), int(ref["n_nodes"][0])
    L = HF * HF
    assert margins_ok(ref, [U], L, N, overlap, 0.5), "input condition: an overlap or a cell at rounding distance of its threshold"
    assert np.array_equal(gr["mention_node"], ref["mention_node"][0, :U]) and np.array_equal(gr["n_pooled"], ref["n_pooled"][0, :U])
    nodes = gr["nodes"]
    assert sorted(nodes) == sorted(G.NODE_FIELDS)
    for f in ("word", "first", "weight", "mentions", "box"):
        assert nodes[f].shape[0] == n and np.array_equal(nodes[f], ref["node_" + f][0, :n]), f
    assert gr["pooled_attention"].shape == (U, 3, HF, HF) and nodes["map"].shape == (n, HF, HF)
    assert rel_err(gr["pooled_attention"].reshape(U, 3, L), ref["maps"][0, :U], ref["n_pooled"][0, :U, None, None].astype(np.float64)) <= 1.0
    assert rel_err(nodes["map"].reshape(n, L), ref["node_map"][0, :n], ref["node_weight"][0, :n, None].astype(np.float64)) <= 1.0
    assert rel_err(nodes["center"], ref["node_center"][0, :n], float(L)) <= 1.0
    sums = gr["pooled_attention"].reshape(U, 3, L).sum(axis=-1)
    assert float(np.abs(sums[:, [0, 2]] - 1.0).max()) <= 1e-5
    gg = p["grounded_graph"]
    assert len(gg["nodes"]) == n and [(e["subject"], e["object"]) for e in gg["edges"]] == [tuple(x) for x in gr["mention_node"].tolist()]
    assert [e["count"] for e in gg["edges"]] == p["counts"].tolist()
    assert [x["word"] for x in gg["nodes"]] == ["w%d" % w for w in nodes["word"]]
    for x, box in zip(gg["nodes"], nodes["box"].tolist()):
        assert x["box"] == [box[1] * 16.0, box[0] * 16.0, (box[3] + 1) * 16.0, (box[2] + 1) * 16.0]


def test_predict_ground_matches_reference(tmp_path):
    """Untrained 64 px model, V 50: N = 32 samples, 4 images per pass, five images, L = 16.  An untrained model's attention is
    near-uniform, so at the default overlap everything of one word merges; the second run puts the threshold into the widest gap
    among the reference's same-token overlaps, where one word must own two nodes in some image."""
    gan = _untrained_gan(tmp_path)
    imgs = _images()
    _, details = gan.test(items=[(im, [[0, 0, 0]]) for im in imgs], out_path=None, return_details=True)
    plain = gan.predict(items=imgs)
    preds = gan.predict(items=imgs, ground=True)
    sampled = _sampled(gan, imgs, NS)
    overlaps = []
    for p, q, dt, (toks, al) in zip(preds, plain, details, sampled):
        assert np.array_equal(toks, dt["tokens"])
        assert set(q) == PARENT_KEYS and set(p) == PARENT_KEYS | {"grounding", "grounded_graph"}
        assert np.array_equal(p["triples"], q["triples"]) and p["graph"] == q["graph"]
        ref = _reference(p, dt["tokens"], al, 0.5)
        _check_record(p, ref, NS, 0.5)
        overlaps.append(ref["overlaps"][0][:, 2])
    ov = np.unique(np.concatenate(overlaps))
    assert len(ov) >= 2, "input condition: same-token pairs exist"
    i = int(np.argmax(np.diff(ov)))
    mid = float(0.5 * (ov[i] + ov[i + 1]))
    print("same-token overlaps %.6f .. %.6f; widest gap %.3e at %.6f" % (ov[0], ov[-1], ov[i + 1] - ov[i], mid))
    preds = gan.predict(items=imgs, ground=True, ground_overlap=mid)
    owns_two = False
    for p, dt, (toks, al) in zip(preds, details, sampled):
        ref = _reference(p, dt["tokens"], al, mid)
        _check_record(p, ref, NS, mid)
        w = p["grounding"]["nodes"]["word"].tolist()
        owns_two |= len(set(w)) < len(w)
    assert owns_two, "at the mid-gap threshold one word must own two nodes in some image"


def test_predict_ground_kbest(tmp_path):
    gan = _untrained_gan(tmp_path)
    imgs = _images()
    preds = gan.predict(items=imgs, decode="kbest", ground=True)
    N = NB                                                  # K-best decoding defaults to TEST_BATCH_SIZE samples
    sampled = _sampled(gan, imgs, N)
    plain = gan.predict(items=imgs, decode="kbest")
    fallbacks = 0
    for p, q, (toks, al) in zip(preds, plain, sampled):
        assert np.array_equal(p["triples"], q["triples"]) and set(p) == set(q) | {"grounding", "grounded_graph"}
        ref = _reference(p, toks, al, 0.5)
        _check_record(p, ref, N, 0.5)
        fallbacks += int((p["grounding"]["n_pooled"] == 0).sum())
    assert fallbacks > 0, "K-best lists hold triples that are no sample's argmax: they pool their best sample's row"


def test_predict_without_ground_launches_nothing_new(tmp_path):
    from sgg_amd.lib import HipKernels
    gan = _untrained_gan(tmp_path)
    imgs = _images()[:2]
    calls = []
    names = ("ground_assign", "ground_pool", "ground_resolve")
    orig = {n: getattr(HipKernels, n) for n in names}

    def wrap(n):
        def f(self, *a, **kw):
            calls.append(n)
            return orig[n](self, *a, **kw)
        return f

    for n in names:
        setattr(HipKernels, n, wrap(n))
    try:
        preds = gan.predict(items=imgs)
        assert calls == [] and all(set(p) == PARENT_KEYS for p in preds)
        att = gan.predict(items=imgs, with_attention=True)
        assert calls == [] and all(set(p) == PARENT_KEYS | {"attention"} for p in att)
        gan.predict(items=imgs, ground=True)
        assert calls == list(names)                         # one batch: one launch of each, in this order
    finally:
        for n in names:
            setattr(HipKernels, n, orig[n])
    for kw in ({"ground_overlap": 0.0}, {"ground_box_frac": 1.5}):
        with pytest.raises(ValueError):
            gan.predict(items=imgs, ground=True, **kw)


def test_predict_dir_ground_cli(tmp_path):
    """train.py --predict_dir D --ground writes the grounding arrays and the "ground" entry; without the flag neither; --ground
    without --predict_dir is a usage error."""
    script = os.path.join(ROOT, "train.py")
    common = ["--synthetic", "8,64,50", "--batch_size", "8", "--critic_iters", "1", "--checkpoints_dir", str(tmp_path / "ck"),
              "--summaries_dir", str(tmp_path / "logs")]
    run = lambda extra: subprocess.run([sys.executable, script] + common + extra, cwd=str(tmp_path), capture_output=True, text=True,
                                       timeout=600)
    r = run(["--ground"])
    assert r.returncode == 2 and "--ground needs --predict_dir" in r.stderr
    r = run(["--max_iterations", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "out"
    r = run(["--predict_dir", str(out), "--max_test_images", "2", "--ground", "--ground_overlap", "0.75"])
    assert r.returncode == 0, r.stderr[-3000:]
    index = json.load(open(str(out / "index.json")))
    assert index["ground"] == {"overlap": 0.75, "box_frac": 0.5}
    new = ["ground_mention_node", "ground_n_pooled", "ground_pooled_attention"] + ["ground_node_" + f for f in G.NODE_FIELDS]
    for i in range(2):
        e = index[str(i)]
        z = np.load(str(out / e["file"]))
        U = z["triples"].shape[0]
        assert all(k in z.files for k in new)
        assert z["ground_mention_node"].shape == (U, 2) and z["ground_pooled_attention"].shape == (U, 3, HF, HF)
        n = z["ground_node_word"].shape[0]
        assert n == int(z["ground_mention_node"].max()) + 1 == len(e["grounded_graph"]["nodes"])
        assert z["ground_node_map"].shape == (n, HF, HF) and len(e["grounded_graph"]["edges"]) == U == len(e["graph"]["edges"])
    out2 = tmp_path / "out2"
    r = run(["--predict_dir", str(out2), "--max_test_images", "2"])
    assert r.returncode == 0, r.stderr[-3000:]
    index2 = json.load(open(str(out2 / "index.json")))
    assert "ground" not in index2 and "grounded_graph" not in index2["0"]
    assert not [k for k in np.load(str(out2 / index2["0"]["file"])).files if k.startswith("ground")]
