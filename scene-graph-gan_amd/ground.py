"""Grounded scene graphs: entity instances resolved from the generator's pooled attention (SceneGraphGAN.predict(ground=True)).

The numpy fp64 reference below STATES the definitions; the kernels of csrc/ground.hip (HipKernels.ground_assign / ground_pool /
ground_resolve) implement them on the device.  Pure Python and numpy: importable without a GPU.

Per image j of a prediction batch: the ranked distinct triples triples[j, u], u < U = min(n_distinct[j], K); the sample tokens
tokens[k, j], k < N; the generator's attention alpha_t[k * nb + j, :] of decoding step t (0 subject, 1 predicate, 2 object) over
the L = Hf x Wf feature cells.

  1. Members of slot u: the samples whose three tokens equal triples[j, u], in ascending sample index.  A sample that equals
     no kept slot (cut by top_k, or holding a token outside [0, V)) belongs to none; should two kept slots hold the same triple
     (a list that is not distinct), the smaller slot owns the samples.  A slot without a member pools the single row
     fallback_sample[j, u] (K-best decoding: a triple need not be any sample's argmax); with a fallback outside [0, N) its maps
     are all zero.  n_pooled = number of members (0 when the fallback was used); the slot's weight is w = max(n_pooled, 1).
  2. maps[j, u, t, :] = mean of the member rows of alpha_t.
  3. Mention m = 2u + r (r = 0 subject, 1 object): token triples[j, u, 2r], map maps[j, u, 2r].
  4. ov(m, m') = sum_l min(a_l, b_l) (both maps sum to 1: one minus the total-variation distance).  Two mentions are joined
     when their tokens are equal (the index, not the word string) and ov >= overlap; nodes are the connected components.  The
     two mentions of one triple are no special case: an edge whose ends land in one node is a self-loop.
  5. A node's id is the number of nodes whose smallest mention is smaller than its own (order of first appearance).
  6. node_map = sum_m w_m map_m / sum_m w_m over the node's mentions (the mean attention of all samples behind the node),
     node_weight = sum_m w_m, node_mentions = the number of mentions.
  7. node_box = the smallest cell rectangle [y0, x0, y1, x1] (inclusive) holding every cell with a >= box_frac * max(a).
  8. node_center = (sum a (y + 0.5), sum a (x + 0.5)) / sum a, in cell units.

overlap and box_frac default to 0.5.  Neither has been tuned, and whether this model's attention localises entities on a trained
checkpoint has not been measured: this module is the tool that makes the question answerable."""
from __future__ import annotations

import numpy as np

DEFAULT_OVERLAP = 0.5
DEFAULT_BOX_FRAC = 0.5
MAX_TOP_K = 1024            # 2 * top_k mentions per image; the pair work of an all-one-word image is quadratic in it

NODE_FIELDS = ("word", "first", "weight", "mentions", "map", "box", "center")


def check_ground_args(overlap=DEFAULT_OVERLAP, box_frac=DEFAULT_BOX_FRAC, top_k=None):
    """The parameter ranges of grounding, checked on the host before anything is launched: overlap and box_frac in (0, 1],
    top_k <= 1024.  Returns (overlap, box_frac) as floats."""
    overlap, box_frac = float(overlap), float(box_frac)
    if not 0.0 < overlap <= 1.0:          # (NaN fails both comparisons)
        raise ValueError("ground: overlap must be in (0, 1] (got %r)" % overlap)
    if not 0.0 < box_frac <= 1.0:
        raise ValueError("ground: box_frac must be in (0, 1] (got %r)" % box_frac)
    if top_k is not None and not 1 <= int(top_k) <= MAX_TOP_K:
        raise ValueError("ground: 1 <= top_k <= %d list slots per image (got %d): an image's 2 * top_k mentions are compared "
                         "pairwise" % (MAX_TOP_K, int(top_k)))
    return overlap, box_frac


def _planes(alphas):
    """[R, 3, L] (NetworkHandle.alphas) or three [R, L] arrays -> [3, R, L] float64."""
    if isinstance(alphas, (tuple, list)):
        return np.stack([np.asarray(a, dtype=np.float64) for a in alphas])
    a = np.asarray(alphas, dtype=np.float64)
    assert a.ndim == 3 and a.shape[1] == 3, a.shape
    return np.ascontiguousarray(a.transpose(1, 0, 2))


def _box_center(a, Hf, Wf, box_frac):
    a2 = a.reshape(Hf, Wf)
    ys, xs = np.nonzero(a2 >= box_frac * a2.max())
    box = [int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())]
    tot = a2.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        cy = (a2.sum(axis=1) * (np.arange(Hf) + 0.5)).sum() / tot
        cx = (a2.sum(axis=0) * (np.arange(Wf) + 0.5)).sum() / tot
    return box, [cy, cx]


def ground_reference(tokens, triples, n_distinct, fallback_sample, alphas, Hf, Wf, overlap=DEFAULT_OVERLAP,
                     box_frac=DEFAULT_BOX_FRAC, vocab=None):
    """Every output of the three grounding kernels for one batch, in fp64 (the definitions of the module docstring).

    tokens int64 [N, nb, 3], triples int64 [nb, K, 3], n_distinct int32 [nb], fallback_sample int32 [nb, K], alphas [N * nb, 3, L]
    or three [N * nb, L] arrays (row k * nb + j), L = Hf * Wf; vocab: the vocabulary size V (default: no upper limit).
    Returns a dict, padded as the kernels pad: slot_of_sample [nb, N], members [nb, N], start [nb, K + 1], n_pooled [nb, K],
    maps [nb, K, 3, L], mention_node [nb, K, 2], n_nodes [nb], node_word / node_first / node_weight / node_mentions [nb, 2K],
    node_map [nb, 2K, L], node_box [nb, 2K, 4], node_center [nb, 2K, 2]; and "overlaps": per image an array [P, 3] of
    (m, m', ov) for EVERY pair m < m' of same-token mentions, so that a test can check its margins."""
    overlap, box_frac = check_ground_args(overlap, box_frac)
    tokens, triples = np.asarray(tokens, dtype=np.int64), np.asarray(triples, dtype=np.int64)
    N, nb = tokens.shape[:2]
    K, L = triples.shape[1], int(Hf) * int(Wf)
    al = _planes(alphas)
    assert al.shape == (3, N * nb, L), (al.shape, N, nb, L)
    fallback_sample = np.asarray(fallback_sample).reshape(nb, K)
    V = None if vocab is None else int(vocab)
    out = {"slot_of_sample": np.full((nb, N), -1, np.int32), "members": np.full((nb, N), -1, np.int32),
           "start": np.zeros((nb, K + 1), np.int32), "n_pooled": np.zeros((nb, K), np.int32), "maps": np.zeros((nb, K, 3, L)),
           "mention_node": np.full((nb, K, 2), -1, np.int32), "n_nodes": np.zeros((nb,), np.int32),
           "node_word": np.full((nb, 2 * K), -1, np.int64), "node_first": np.full((nb, 2 * K), -1, np.int32),
           "node_weight": np.full((nb, 2 * K), -1, np.int32), "node_mentions": np.full((nb, 2 * K), -1, np.int32),
           "node_map": np.zeros((nb, 2 * K, L)), "node_box": np.full((nb, 2 * K, 4), -1, np.int32),
           "node_center": np.full((nb, 2 * K, 2), np.nan), "overlaps": []}
    in_vocab = lambda t: all(x >= 0 and (V is None or x < V) for x in t)
    for j in range(nb):
        U = min(max(int(n_distinct[j]), 0), K)
        # 1. members
        slot_of = {}
        for u in range(U):
            t = tuple(int(x) for x in triples[j, u])
            if in_vocab(t):
                slot_of.setdefault(t, u)
        groups = [[] for _ in range(U)]
        for k in range(N):
            t = tuple(int(x) for x in tokens[k, j])
            u = slot_of.get(t, -1) if in_vocab(t) else -1
            out["slot_of_sample"][j, k] = u
            if u >= 0:
                groups[u].append(k)
        pos = 0
        for u in range(U):
            out["start"][j, u] = pos
            out["members"][j, pos:pos + len(groups[u])] = groups[u]
            pos += len(groups[u])
        out["start"][j, U:] = pos
        # 2. pooled maps
        w = np.ones((U,), np.int64)
        for u in range(U):
            n = len(groups[u])
            out["n_pooled"][j, u] = n
            if n:
                rows = np.asarray(groups[u], np.int64) * nb + j
                out["maps"][j, u] = al[:, rows].sum(axis=1) / n
                w[u] = n
            else:
                fb = int(fallback_sample[j, u])
                if 0 <= fb < N:
                    out["maps"][j, u] = al[:, fb * nb + j]
        # 3. mentions and 4. joining
        M = 2 * U
        tok = triples[j, :U][:, [0, 2]].reshape(M)
        mp = out["maps"][j, :U][:, [0, 2]].reshape(M, L)
        wm = np.repeat(w, 2)
        parent = list(range(M))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        pairs = []
        for m in range(M - 1):
            same = np.nonzero(tok[m + 1:] == tok[m])[0] + m + 1
            if not len(same):
                continue
            ov = np.minimum(mp[m], mp[same]).sum(axis=1)
            pairs.append(np.stack([np.full(len(same), m, np.float64), same.astype(np.float64), ov], axis=1))
            for m2 in same[ov >= overlap]:
                a, b = find(m), find(int(m2))
                if a != b:
                    parent[max(a, b)] = min(a, b)
        out["overlaps"].append(np.concatenate(pairs) if pairs else np.zeros((0, 3)))
        # 5. node ids in order of first appearance (the root of a component is its smallest mention)
        root = [find(m) for m in range(M)]
        ids = {}
        for m in range(M):
            if root[m] == m:
                ids[m] = len(ids)
        out["n_nodes"][j] = len(ids)
        out["mention_node"][j, :U] = np.asarray([ids[r] for r in root], np.int32).reshape(U, 2)
        # 6. - 8. node maps, boxes, centres
        root = np.asarray(root, np.int64)
        for m0, n in ids.items():
            ms = np.nonzero(root == m0)[0]
            wsum = int(wm[ms].sum())
            a = (wm[ms, None] * mp[ms]).sum(axis=0) / wsum
            out["node_word"][j, n], out["node_first"][j, n] = tok[m0], m0
            out["node_weight"][j, n], out["node_mentions"][j, n] = wsum, len(ms)
            out["node_map"][j, n] = a
            out["node_box"][j, n], out["node_center"][j, n] = _box_center(a, Hf, Wf, box_frac)
    return out


def grounded_scene_graph(triples, scores, counts, reverse_vocab, mention_node, nodes, image_size):
    """{"nodes": [...], "edges": [...]} of a ranked list of triples whose subjects and objects have been resolved to entity
    instances.  mention_node [U, 2]: the node of each triple's subject and object; nodes: dict of arrays over the image's n nodes
    (word [n], weight [n], mentions [n], box [n, 4] as [y0, x0, y1, x1] inclusive cells, center [n, 2] as (y, x) in cells, map
    [n, Hf, Wf]: the grid is read from it); image_size: the side S of the square input in pixels.

    Node: {"word", "box": [x0, y0, x1, y1], "center": [x, y], "weight", "mentions"}, box and centre in input pixels on the uniform
    grid of S / Wf by S / Hf pixel cells: cell column x covers x * S / Wf up to (x + 1) * S / Wf, so an inclusive cell box
    [y0, x0, y1, x1] is x0 * S / Wf to (x1 + 1) * S / Wf, and likewise in y.  The receptive field of a feature cell (far larger
    than its grid cell, and overlapping its neighbours') is NOT modelled.  Edge, in ranked order: {"subject": node index,
    "predicate": word, "object": node index, "score", "count"}; subject == object is a self-loop and is kept."""
    word = lambda i: reverse_vocab.get(int(i), "UNK")
    Hf, Wf = np.asarray(nodes["map"]).shape[-2:]
    sy, sx = float(image_size) / Hf, float(image_size) / Wf
    lst = lambda a, dt: np.asarray(a, dtype=dt).tolist()         # (Python scalars in one pass: the records are built per image)
    out_nodes = [{"word": word(w), "box": [x0 * sx, y0 * sy, (x1 + 1) * sx, (y1 + 1) * sy], "center": [cx * sx, cy * sy],
                  "weight": wt, "mentions": nm}
                 for w, (y0, x0, y1, x1), (cy, cx), wt, nm in zip(lst(nodes["word"], np.int64), lst(nodes["box"], np.int64),
                                                                  lst(nodes["center"], np.float64), lst(nodes["weight"], np.int64),
                                                                  lst(nodes["mentions"], np.int64))]
    edges = [{"subject": s, "predicate": word(t[1]), "object": o, "score": sc, "count": c}
             for t, sc, c, (s, o) in zip(lst(triples, np.int64), lst(scores, np.float64), lst(counts, np.int64),
                                         lst(np.asarray(mention_node).reshape(-1, 2), np.int64))]
    return {"nodes": out_nodes, "edges": edges}
