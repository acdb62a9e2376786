"""CPU: the host logic of scene-graph prediction (sgg_amd/predict.py) - the graph of a ranked triple list and the number of images
per sampling pass."""
import sgg_amd  # noqa: F401
from sgg_amd.predict import DEFAULT_LOGITS_BUDGET_BYTES, images_per_pass, scene_graph


def test_scene_graph_nodes_edges_and_unknown_words():
    rv = {0: "man", 1: "on", 2: "horse", 3: "wears", 4: "hat", 5: "field"}
    triples = [[0, 1, 2], [0, 3, 4], [2, 1, 5], [0, 1, 2], [4, 1, 99]]
    scores = [-1.5, -0.25, 0.0, 0.5, 2.0]
    counts = [3, 1, 2, 1, 7]
    g = scene_graph(triples, scores, counts, rv)
    # a word is one node however often it is subject or object; order of first appearance; index 99 is unknown
    assert g["nodes"] == ["man", "horse", "hat", "field", "UNK"]
    assert g["edges"] == [
        {"subject": 0, "predicate": "on", "object": 1, "score": -1.5, "count": 3},
        {"subject": 0, "predicate": "wears", "object": 2, "score": -0.25, "count": 1},
        {"subject": 1, "predicate": "on", "object": 3, "score": 0.0, "count": 2},
        {"subject": 0, "predicate": "on", "object": 1, "score": 0.5, "count": 1},
        {"subject": 2, "predicate": "on", "object": 4, "score": 2.0, "count": 7},
    ]
    assert all(type(e["score"]) is float and type(e["count"]) is int for e in g["edges"])
    g = scene_graph([[7, 8, 7]], [1.0], [1], rv)           # unknown predicate; subject and object share the unknown node
    assert g == {"nodes": ["UNK"], "edges": [{"subject": 0, "predicate": "UNK", "object": 0, "score": 1.0, "count": 1}]}
    assert scene_graph([], [], [], rv) == {"nodes": [], "edges": []}


def test_scene_graph_takes_numpy_arrays():
    import numpy as np
    g = scene_graph(np.array([[1, 0, 2]], dtype=np.int64), np.array([0.5], dtype=np.float32), np.array([4], dtype=np.int32),
                    {0: "a", 1: "b", 2: "c"})
    assert g == {"nodes": ["b", "c"], "edges": [{"subject": 0, "predicate": "a", "object": 1, "score": 0.5, "count": 4}]}


def test_images_per_pass():
    assert DEFAULT_LOGITS_BUDGET_BYTES == 8 << 30
    # the default evaluation shape runs the passes of test()
    assert images_per_pass(256, 1000, 32, 10 ** 6) == 32
    assert images_per_pass(256, 1000, 32, 10 ** 6, DEFAULT_LOGITS_BUDGET_BYTES) == 32
    # V = 70 000, N = 4096: the slab [N, nb, 3, V] float32 stays inside the budget
    nb = images_per_pass(4096, 70000, 32, 1000)
    slab = lambda n: 4096 * n * 3 * 70000 * 4
    assert 1 <= nb <= 32 and slab(nb) <= DEFAULT_LOGITS_BUDGET_BYTES < slab(nb + 1)
    # never more than the items, never less than one (one image's slab is the floor even where it exceeds the budget)
    for n_items in (1, 2, 5, 31, 32, 33):
        assert images_per_pass(256, 1000, 32, n_items) == min(32, n_items)
    assert images_per_pass(4096, 70000, 32, 1) == 1
    assert images_per_pass(4096, 70000, 32, 7, logits_budget_bytes=1) == 1
    assert images_per_pass(32, 50, 4, 5) == 4
    assert images_per_pass(256, 1000, 32, 100, logits_budget_bytes=5 * 256 * 3 * 1000 * 4) == 5
