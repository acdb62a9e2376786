"""Host logic of scene-graph prediction (SceneGraphGAN.predict in train.py): how many images share one sampling pass, and the
graph of an image's ranked distinct triples.  Pure Python: importable without a GPU.  The ranking itself is the HIP kernel
csrc/rank.hip behind lib.HipKernels.rank_triples."""
from __future__ import annotations

DEFAULT_LOGITS_BUDGET_BYTES = 8 << 30


def images_per_pass(n_samples, vocab, test_batch_size, n_items, logits_budget_bytes=DEFAULT_LOGITS_BUDGET_BYTES):
    """Images per encoder pass.  Generator.sample materialises the logits of all samples of a pass, [n_samples, nb, 3, vocab] float32:
    the largest nb <= min(test_batch_size, n_items) whose slab fits the budget, and at least 1 (one image's slab is the floor: it
    may exceed the budget).  The default evaluation shape (N = 256, TEST_BATCH_SIZE = 32, V = 1000: 98 MB) gives TEST_BATCH_SIZE, the
    passes of test()."""
    per_image = int(n_samples) * 3 * int(vocab) * 4
    cap = min(int(test_batch_size), int(n_items))
    return max(1, min(cap, int(logits_budget_bytes) // per_image))


def scene_graph(triples, scores, counts, reverse_vocab):
    """{"nodes": [...], "edges": [...]} of a ranked list of (subject, predicate, object) index triples.  Nodes: the distinct subject
    and object words in order of first appearance (a word is one node, whichever role it appears in).  Edges, in ranked order:
    {"subject": node index, "predicate": word, "object": node index, "score": critic score, "count": samples that were this triple}.
    Indices missing from reverse_vocab map to "UNK", as in SceneGraphGAN.sample_triples."""
    word = lambda i: reverse_vocab.get(int(i), "UNK")
    nodes, where, edges = [], {}, []

    def node(w):
        if w not in where:
            where[w] = len(nodes)
            nodes.append(w)
        return where[w]

    for (s, p, o), sc, c in zip(triples, scores, counts):
        i = node(word(s))
        j = node(word(o))
        edges.append({"subject": i, "predicate": word(p), "object": j, "score": float(sc), "count": int(c)})
    return {"nodes": nodes, "edges": edges}
