"""CPU: the host logic of K-best decoding (sgg_amd/kbest.py), the command line, and the numpy reference of tests/kbest_ref.py
against brute force over all V^3 triples."""
import numpy as np
import pytest

import sgg_amd  # noqa: F401
from sgg_amd import kbest
from sgg_amd.predict import scene_graph
from tests import kbest_ref as R


@pytest.mark.parametrize("kind", ["normal", "quantised"])
@pytest.mark.parametrize("V", [1, 2, 3, 7, 12])
def test_top_m_cube_equals_brute_force(V, kind):
    """Only the top min(K, V) tokens of a slot, and only rank tuples with (i+1)(j+1)(l+1) <= K, can be among the K best: the cube of
    the top M against all V^3 triples, every valid K, random logits and logits on a 0.5 grid (exact ties everywhere)."""
    g = np.random.RandomState(100 + V)
    x = (2.0 * g.standard_normal((3, V))).astype(np.float32)
    if kind == "quantised":
        x = (np.round(x * 2.0) / 2.0).astype(np.float32)
        assert V < 7 or any(len(np.unique(x[s])) < V for s in range(3)), "ties expected"
    for K in range(1, min(kbest.MAX_K, V ** 3) + 1):
        t, lp, ranks = R.kbest_row(x, K)
        tb, lpb, ranksb = R.brute_force_row(x, K)
        assert np.array_equal(t, tb) and np.array_equal(lp, lpb) and np.array_equal(ranks, ranksb), (V, K)
        assert len({tuple(r) for r in t.tolist()}) == K and (np.diff(lp) <= 0).all()
        assert ((ranks + 1).prod(axis=1) <= K).all(), "a rank tuple outside the candidate set was selected"


def test_candidate_count():
    want = {20: 152, 50: 564, 100: 1471, 128: 2045}
    r = np.arange(1, 129)
    cube = np.multiply.outer(np.multiply.outer(r, r), r)          # (i+1)(j+1)(l+1) of every rank tuple below 128
    for K in range(1, 129):
        n = kbest.candidate_count(K)
        assert n == int((cube[:K, :K, :K] <= K).sum()), K           # the direct count, every K
        assert K <= n <= 2045
    for K in (1, 2, 7, 20):                                         # the cube itself against the plain triple loop
        assert int((cube[:K, :K, :K] <= K).sum()) == R.direct_candidate_count(K)
    for K, n in want.items():
        assert kbest.candidate_count(K) == n
    assert kbest.candidate_count(256) == 5136 > kbest.MAX_POOL            # why 128 is the limit
    # ranks capped by a small vocabulary
    assert kbest.candidate_count(8, 2) == 8 and kbest.candidate_count(128, 1) == 1
    assert kbest.candidate_count(100, 3) == sum(1 for i in range(3) for j in range(3) for l in range(3) if (i + 1) * (j + 1) * (l + 1) <= 100)


def test_list_width_and_argument_checks():
    assert kbest.list_width(32, 1000) == 128 and kbest.list_width(1, 70000) == 128          # the defaults at batch 64
    assert kbest.list_width(4, 50) == 128 and kbest.list_width(64, 1000) == 64 and kbest.list_width(256, 1000) == 16
    assert kbest.list_width(4096, 1000) == 1 and kbest.list_width(5, 1000) == 128 and kbest.list_width(33, 1000) == 124
    assert kbest.list_width(1, 1) == 1 and kbest.list_width(2, 2) == 8 and kbest.list_width(1, 5) == 125
    # defaults: TEST_BATCH_SIZE samples, every slot
    assert kbest.setup("predict", None, None, 1000, 32) == (32, 128, 4096)
    assert kbest.setup("predict", None, None, 50, 4) == (4, 128, 512)
    assert kbest.setup("predict", 1, 20, 70000, 32) == (1, 128, 20)
    assert kbest.setup("evaluate", 4096, None, 1000, 32) == (4096, 1, 4096)
    for n in (0, -1, 4097):
        with pytest.raises(ValueError, match="n_samples"):
            kbest.setup("predict", n, None, 1000, 32)
    for n, k in ((4, 0), (4, 513), (1, 129), (4096, 4097)):
        with pytest.raises(ValueError, match="top_k"):
            kbest.setup("predict", n, k, 1000, 32)
    assert kbest.check_decode("samples") == "samples" and kbest.check_decode("samples", True) == "samples"
    assert kbest.check_decode("kbest") == "kbest"
    with pytest.raises(ValueError, match="descending"):
        kbest.check_decode("kbest", True)
    with pytest.raises(ValueError, match="decode"):
        kbest.check_decode("beam")


def test_command_line(capsys):
    import train as T
    assert T.build_parser().parse_args([]).decode == "samples"
    assert T.build_parser().parse_args(["--decode", "kbest"]).decode == "kbest"
    assert T.parse_args(["--decode", "kbest", "--predict_dir", "x"]).decode == "kbest"
    assert T.parse_args(["--predict_descending"]).decode == "samples"
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--decode", "beam"])
    with pytest.raises(SystemExit) as e:
        T.parse_args(["--decode", "kbest", "--predict_descending", "--predict_dir", "x"])
    assert e.value.code == 2 and "--predict_descending" in capsys.readouterr().err


def test_scene_graph_of_a_kbest_record():
    """The record of predict(decode="kbest"): the edge's score is the mixture log-probability, its count the lists holding the triple."""
    x = np.array([[0.0, 2.0, 1.0], [3.0, 0.0, 0.0], [0.0, 0.0, 1.5]], dtype=np.float32)
    t, lp, _ = R.kbest_row(x, 4)
    m = R.merge_image(t[None], x[None], R.lse64(x)[None])
    assert m["n_distinct"] == 4 and np.array_equal(m["triples"], t) and np.allclose(m["scores"], lp, rtol=0, atol=1e-12)
    assert m["counts"].tolist() == [1] * 4 and m["best_sample"].tolist() == [0] * 4
    g = scene_graph(m["triples"], m["scores"].astype(np.float32), m["counts"], {0: "man", 1: "on", 2: "horse"})
    assert t.tolist() == [[1, 0, 2], [2, 0, 2], [1, 0, 0], [1, 0, 1]]
    assert g["nodes"] == ["on", "horse", "man"]
    assert [(e["subject"], e["predicate"], e["object"], e["count"]) for e in g["edges"]] == \
        [(0, "man", 1, 1), (1, "man", 1, 1), (0, "man", 2, 1), (0, "man", 0, 1)]
    assert all(type(e["score"]) is float and e["score"] < 0 for e in g["edges"])
    assert [e["score"] for e in g["edges"]] == sorted((e["score"] for e in g["edges"]), reverse=True)
