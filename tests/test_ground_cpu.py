"""CPU: the definitions of grounded scene graphs (sgg_amd/ground.py) on hand-written cases - ground_reference, the fp64 statement
the kernels of csrc/ground.hip are tested against, grounded_scene_graph and check_ground_args."""
import numpy as np
import pytest

import sgg_amd  # noqa: F401
from sgg_amd import ground as G


def onehot(L, *cells):
    a = np.zeros((L,))
    for c in cells:
        a[c] = 1.0 / len(cells)
    return a


def run(sample_triples, sample_maps, triples, fallback=None, Hf=2, Wf=2, n_distinct=None, **kw):
    """One image.  sample_triples [N][3]; sample_maps [N] of (subject map, object map) over L cells (the predicate's map is uniform);
    triples [K][3]."""
    N, K, L = len(sample_triples), len(triples), Hf * Wf
    tokens = np.asarray(sample_triples, np.int64).reshape(N, 1, 3)
    al = np.zeros((N, 3, L))
    for k, (s, o) in enumerate(sample_maps):
        al[k, 0], al[k, 1], al[k, 2] = s, np.full((L,), 1.0 / L), o
    fb = np.full((1, K), -1, np.int32) if fallback is None else np.asarray(fallback, np.int32).reshape(1, K)
    nd = np.asarray([K if n_distinct is None else n_distinct], np.int32)
    return G.ground_reference(tokens, np.asarray(triples, np.int64).reshape(1, K, 3), nd, fb, al, Hf, Wf, **kw)


A, B, C, D = (onehot(4, c) for c in range(4))


def test_two_same_word_mentions_with_disjoint_maps_are_two_nodes():
    r = run([[1, 5, 2], [1, 6, 3]], [(A, B), (C, D)], [[1, 5, 2], [1, 6, 3]])
    assert r["n_nodes"][0] == 4 and r["mention_node"][0].tolist() == [[0, 1], [2, 3]]
    assert r["node_word"][0, :4].tolist() == [1, 2, 1, 3]
    ov = r["overlaps"][0]
    assert ov.tolist() == [[0.0, 2.0, 0.0]]          # the one same-token pair: mentions 0 and 2, disjoint


def test_identical_maps_are_one_node():
    r = run([[1, 5, 2], [1, 6, 3]], [(A, B), (A, D)], [[1, 5, 2], [1, 6, 3]])
    assert r["n_nodes"][0] == 3 and r["mention_node"][0].tolist() == [[0, 1], [0, 2]]
    assert r["node_mentions"][0, :3].tolist() == [2, 1, 1] and r["node_first"][0, :3].tolist() == [0, 1, 3]
    assert r["overlaps"][0].tolist() == [[0.0, 2.0, 1.0]]


def test_a_chain_is_one_node():
    """a ~ b, b ~ c, a !~ c: the transitive closure joins all three."""
    a, b, c = onehot(4, 0, 1), onehot(4, 1, 2), onehot(4, 2, 3)
    r = run([[1, 5, 7], [1, 6, 8], [1, 4, 9]], [(a, D), (b, D), (c, D)], [[1, 5, 7], [1, 6, 8], [1, 4, 9]], overlap=0.5)
    ov = {(int(m), int(n)): v for m, n, v in r["overlaps"][0]}
    assert ov[(0, 2)] == 0.5 and ov[(2, 4)] == 0.5 and ov[(0, 4)] == 0.0
    assert r["mention_node"][0].tolist() == [[0, 1], [0, 2], [0, 3]] and r["n_nodes"][0] == 4
    assert r["node_mentions"][0, 0] == 3
    assert np.allclose(r["node_map"][0, 0], [1 / 6, 1 / 3, 1 / 3, 1 / 6])


def test_identical_maps_with_different_tokens_are_two_nodes():
    r = run([[1, 5, 2]], [(A, A)], [[1, 5, 2]])
    assert r["n_nodes"][0] == 2 and r["mention_node"][0].tolist() == [[0, 1]] and len(r["overlaps"][0]) == 0


def test_a_self_loop_is_kept():
    r = run([[1, 5, 1]], [(A, A)], [[1, 5, 1]])
    assert r["n_nodes"][0] == 1 and r["mention_node"][0].tolist() == [[0, 0]]
    nodes = {k: r["node_" + k][0, :1] for k in G.NODE_FIELDS}
    nodes["map"] = nodes["map"].reshape(1, 2, 2)
    g = G.grounded_scene_graph([[1, 5, 1]], [0.25], [1], {1: "man", 5: "beside"}, r["mention_node"][0, :1], nodes, 64)
    assert g["edges"] == [{"subject": 0, "predicate": "beside", "object": 0, "score": 0.25, "count": 1}]
    assert len(g["nodes"]) == 1 and g["nodes"][0]["word"] == "man" and g["nodes"][0]["mentions"] == 2


def test_a_slot_without_member_uses_its_fallback_row_with_weight_one():
    # K-best-like: slot 1's triple is no sample's; it pools sample 2's row.  Slot 2 has no fallback either: zeros.
    r = run([[1, 5, 2], [1, 5, 2], [3, 3, 3]], [(A, B), (A, B), (C, D)], [[1, 5, 2], [1, 6, 2], [4, 4, 4]], fallback=[0, 2, -1])
    assert r["n_pooled"][0].tolist() == [2, 0, 0]
    assert np.array_equal(r["maps"][0, 1, 0], C) and np.array_equal(r["maps"][0, 1, 2], D)
    assert not r["maps"][0, 2].any()
    assert r["slot_of_sample"][0].tolist() == [0, 0, -1] and r["members"][0].tolist() == [0, 1, -1]
    assert r["start"][0].tolist() == [0, 2, 2, 2]
    # mentions 2 (word 1, map C) and 0 (word 1, map A) stay apart; the fallback node weighs 1
    assert r["mention_node"][0].tolist() == [[0, 1], [2, 3], [4, 5]]
    assert r["node_weight"][0, :6].tolist() == [2, 2, 1, 1, 1, 1]
    assert np.isnan(r["node_center"][0, 4]).all() and r["node_box"][0, 4].tolist() == [0, 0, 1, 1]      # an all-zero map


def test_a_sample_cut_by_top_k_is_in_no_slot():
    r = run([[1, 5, 2], [3, 6, 4], [1, 5, 2]], [(A, B), (C, D), (A, B)], [[1, 5, 2], [3, 6, 4]], n_distinct=1)
    assert r["slot_of_sample"][0].tolist() == [0, -1, 0] and r["members"][0].tolist() == [0, 2, -1]
    assert r["start"][0].tolist() == [0, 2, 2] and r["n_pooled"][0].tolist() == [2, 0]
    assert r["mention_node"][0].tolist() == [[0, 1], [-1, -1]] and r["n_nodes"][0] == 2
    # a token outside the vocabulary is in no slot either
    r = run([[1, 5, 9]], [(A, B)], [[1, 5, 9]], vocab=9)
    assert r["slot_of_sample"][0].tolist() == [-1] and r["n_pooled"][0].tolist() == [0]


def test_node_ids_follow_first_appearance():
    # mentions: 0 (w1, A)  1 (w2, B)  2 (w2, B)  3 (w1, C)  4 (w1, C)  5 (w1, A)
    r = run([[1, 5, 2], [2, 5, 1], [1, 5, 1]], [(A, B), (B, C), (C, A)], [[1, 5, 2], [2, 5, 1], [1, 5, 1]])
    assert r["mention_node"][0].tolist() == [[0, 1], [1, 2], [2, 0]]
    assert r["node_first"][0, :3].tolist() == [0, 1, 3] and r["node_word"][0, :3].tolist() == [1, 2, 1]
    assert (r["node_first"][0, 3:] == -1).all() and (r["node_word"][0, 3:] == -1).all()
    assert not r["node_map"][0, 3:].any() and np.isnan(r["node_center"][0, 3:]).all()


def test_node_map_weights():
    """A node of two mentions with n_pooled 3 and 1: its map is (3 a + 1 b) / 4."""
    a, b = np.array([0.7, 0.1, 0.1, 0.1]), np.array([0.4, 0.4, 0.1, 0.1])
    r = run([[1, 5, 2]] * 3 + [[1, 6, 3]], [(a, C)] * 3 + [(b, D)], [[1, 5, 2], [1, 6, 3]])
    assert r["n_pooled"][0].tolist() == [3, 1] and r["mention_node"][0].tolist() == [[0, 1], [0, 2]]
    assert r["node_weight"][0, :3].tolist() == [4, 3, 1]
    assert np.allclose(r["node_map"][0, 0], (3 * a + b) / 4, rtol=0, atol=1e-15)
    assert np.allclose(r["overlaps"][0], [[0.0, 2.0, 0.7]])


def test_box_and_centre():
    a = np.zeros((3, 4))
    a[1, 2], a[0, 0], a[2, 3] = 0.5, 0.3, 0.2
    kw = dict(Hf=3, Wf=4)
    r = run([[1, 5, 2]], [(a.ravel(), a.ravel())], [[1, 5, 2]], box_frac=1.0, **kw)
    assert r["node_box"][0, 0].tolist() == [1, 2, 1, 2]                  # the argmax cell
    r = run([[1, 5, 2]], [(a.ravel(), a.ravel())], [[1, 5, 2]], box_frac=0.5, **kw)
    assert r["node_box"][0, 0].tolist() == [0, 0, 1, 2]                  # 0.3 >= 0.25, 0.2 is not
    u = np.full((12,), 1.0 / 12) + np.linspace(-1e-3, 1e-3, 12) * np.array([1, -1] * 6)
    r = run([[1, 5, 2]], [(u / u.sum(), a.ravel())], [[1, 5, 2]], box_frac=1e-6, **kw)
    assert r["node_box"][0, 0].tolist() == [0, 0, 2, 3]                  # a tiny fraction: the whole grid
    assert np.allclose(r["node_center"][0, 1], [0.3 * 0.5 + 0.5 * 1.5 + 0.2 * 2.5, 0.3 * 0.5 + 0.5 * 2.5 + 0.2 * 3.5])


def test_pixel_mapping_on_a_non_square_grid():
    nodes = {"word": np.array([7]), "first": np.array([0]), "weight": np.array([5]), "mentions": np.array([2]),
             "map": np.zeros((1, 2, 4)), "box": np.array([[0, 1, 1, 2]]), "center": np.array([[0.5, 3.0]])}
    g = G.grounded_scene_graph(np.array([[7, 3, 7]]), [1.5], [4], {7: "dog"}, np.array([[0, 0]]), nodes, 64)
    # S = 64, Hf = 2, Wf = 4: cells are 16 px wide and 32 px high
    assert g["nodes"] == [{"word": "dog", "box": [16.0, 0.0, 48.0, 64.0], "center": [48.0, 16.0], "weight": 5, "mentions": 2}]
    assert g["edges"] == [{"subject": 0, "predicate": "UNK", "object": 0, "score": 1.5, "count": 4}]


def test_check_ground_args():
    assert G.check_ground_args() == (0.5, 0.5)
    assert G.check_ground_args(1.0, 1.0, 1024) == (1.0, 1.0)
    for bad in (0.0, -0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="overlap"):
            G.check_ground_args(overlap=bad)
        with pytest.raises(ValueError, match="box_frac"):
            G.check_ground_args(box_frac=bad)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="top_k"):
            G.check_ground_args(top_k=bad)
    with pytest.raises(ValueError, match="overlap"):
        run([[1, 5, 2]], [(A, B)], [[1, 5, 2]], overlap=0.0)


def test_command_line(capsys):
    import train as T
    a = T.parse_args([])
    assert a.ground is False and a.ground_overlap == 0.5 and a.ground_box_frac == 0.5
    a = T.parse_args(["--predict_dir", "x", "--ground", "--ground_overlap", "0.7", "--ground_box_frac", "0.25", "--decode", "kbest"])
    assert a.ground and a.ground_overlap == 0.7 and a.ground_box_frac == 0.25
    for argv, word in ((["--ground"], "--predict_dir"), (["--predict_dir", "x", "--ground", "--ground_overlap", "0"], "overlap"),
                       (["--predict_dir", "x", "--ground", "--ground_box_frac", "1.5"], "box_frac"),
                       (["--predict_dir", "x", "--ground", "--top_k", "1025"], "top_k")):
        with pytest.raises(SystemExit) as e:
            T.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_predict_refuses_a_kernel_set_without_the_grounding_kernels():
    """need_kernels guards the path: a kernel set that lacks the three kernels is refused by name, never replaced."""
    from sgg_amd.step import need_kernels

    class Stub:
        name = "stub"

        def ground_assign(self):
            pass

    with pytest.raises(RuntimeError, match="ground_pool, ground_resolve"):
        need_kernels(Stub(), "predict(ground=True)", "ground_assign", "ground_pool", "ground_resolve")
