"""The exact oracles of ``tree_oracle`` on values worked out by hand, and the tree engine's CPU
branches against them on every case the GPU module (``test_tree_kernels_gpu.py``) uses — so the
oracles, the case data and the CPU rule are checked before any kernel is."""
from fractions import Fraction

import numpy as np
import pytest

import tree_cases as C
import tree_oracle as O

CPU = "cpu"


# ---------------------------------------------------------------------------------------------- the oracles

def test_oracle_bin_codes_by_hand():
    thr = np.array([[0.1, 0.5, 0.9], [0.0, np.inf, np.inf], [np.inf] * 3])
    x = np.array([[0.1, -0.0, 7.0], [np.nextafter(0.1, 1), np.nextafter(0.0, 1), -np.inf], [np.nan] * 3,
                  [np.inf, -np.inf, np.inf], [0.9, 0.0, 0.0]])
    assert O.bin_codes(x, thr, [3, 1, 0]).tolist() == [[0, 0, 0], [1, 1, 0], [3, 1, 0], [3, 0, 0], [2, 0, 0]]


def test_oracle_histogram_by_hand():
    bins = np.array([[0, 1], [1, 1], [1, 0], [0, 0]])
    node_of = np.array([[0, 0, -1, 1]], dtype=np.int32)
    wt = np.array([[2.0, 0.5, 1.0, 0.0]], dtype=np.float32)
    h = O.histogram(bins, node_of, wt, np.array([3.0, -2.0, 9.0, 9.0]), 3, 2, [4.0, 2.0, 1.0], 2)
    assert h.shape == (1, 2, 2, 2, 3) and not h[0, 1].any()          # row 3 has weight 0, row 2 is retired
    assert h[0, 0, 0].tolist() == [[8, 12, 18], [2, -2, 2]] and h[0, 0, 1].tolist() == [[0, 0, 0], [10, 10, 20]]
    hc = O.histogram(bins, node_of, wt, np.array([1, 0, 1, 1], dtype=np.int32), 2, 2, [4.0, 1.0, 1.0], 2)
    assert hc[0, 0, 0].tolist() == [[0, 8], [2, 0]]
    # round half to even
    assert O.histogram(bins[:1], node_of[:, :1], np.array([[2.5]], dtype=np.float32), np.array([0], dtype=np.int32),
                       1, 1, [1.0, 1.0, 1.0], 2)[0, 0, 0, 0, 0] == 2


def test_oracle_best_split_by_hand():
    # y = 0, 0, 4, 4 in bins 0..3 of feature 1; feature 0 puts every row in bin 0
    h = np.zeros((2, 4, 3), dtype=np.int64)
    h[0, 0] = [4, 8, 32]
    h[1] = [[1, 0, 0], [1, 0, 0], [1, 4, 16], [1, 4, 16]]
    o = O.best_split(h, [1.0, 1.0, 1.0], "variance", [1, 1], [3, 3], 1, 0.0, 0.0)
    gains = {(f, b): g for f, b, g, *_ in o["candidates"]}
    assert gains[(0, 0)] is None                                      # nothing on the right
    assert gains[(1, 0)] == Fraction(4, 3) and gains[(1, 1)] == 4 and gains[(1, 2)] == Fraction(4, 3)
    assert (o["feature"], o["bin"], o["gain"]) == (1, 1, 4) and o["left_i"] == [2, 0, 0] and o["right_i"] == [2, 8, 32]
    assert o["err"] == 32 * 2.0 ** -53 * 8 and not o["ambiguous"]
    assert O.best_split(h, [1.0] * 3, "variance", [1, 1], [3, 3], 2, 0.0, 0.0)["feature"] == 1
    assert O.best_split(h, [1.0] * 3, "variance", [1, 1], [3, 3], 3, 0.0, 0.0)["feature"] == -1
    assert O.best_split(h, [1.0] * 3, "variance", [1, 1], [3, 3], 1, 0.3, 0.0)["bin"] == 1
    assert O.best_split(h, [1.0] * 3, "variance", [1, 0], [3, 3], 1, 0.0, 0.0)["feature"] == -1
    assert O.best_split(h, [1.0] * 3, "variance", [1, 1], [3, 1], 1, 0.0, 0.0)["bin"] == 0
    assert O.best_split(h, [1.0] * 3, "variance", [1, 1], [3, 3], 1, 0.0, 4.5)["feature"] == -1
    # two classes, 4 rows each; the split after bin 0 separates them: gini 1/2 -> 0, entropy 1 -> 0
    hc = np.array([[[4, 0], [0, 4]], [[2, 2], [2, 2]]], dtype=np.int64)
    g = O.best_split(hc, [2.0, 1.0, 1.0], "gini", [1, 1], [1, 1], 1, 0.0, 0.0)
    assert (g["feature"], g["gain"]) == (0, Fraction(1, 2)) and g["candidates"][1][2] == 0
    e = O.best_split(hc, [2.0, 1.0, 1.0], "entropy", [1, 1], [1, 1], 1, 0.0, 0.0)
    assert (e["feature"], e["gain"]) == (0, 1) and e["candidates"][1][2] == 0
    # a tie within TIE_REL of the maximum goes to the first candidate; beyond it, to the larger gain
    # (gain = const + (s1l^2 / wl + s1r^2 / wr) / W: moving k / 2^20 of sum(w y) to the right child
    # raises feature 1's gain by 3.8e-17 * k of itself)
    def tie(k):
        ht = np.zeros((2, 2, 3), dtype=np.int64)
        for f, dk in ((0, 0), (1, k)):
            ht[f] = [[10 ** 4, -dk, 10 ** 4], [10 ** 4, 10 ** 11 * 2 ** 20 + dk, 2 * 10 ** 18 - 10 ** 4]]
        o = O.best_split(ht, [1.0, 2.0 ** 20, 1.0], "variance", [1, 1], [1, 1], 1, 0.0, 0.0)
        g0, g1 = o["candidates"][0][2], o["candidates"][1][2]
        return o["feature"], float((g1 - g0) / g0)
    f, rel = tie(10000)
    assert f == 0 and 3e-13 < rel < 5e-13
    f, rel = tie(200000)
    assert f == 1 and 7e-12 < rel < 8e-12


def test_oracle_route_and_predict_by_hand():
    bins = np.array([[3, 0], [4, 9], [0, 0], [9, 9]])
    node_of = np.array([[0, 0, 1, -1]], dtype=np.int32)
    out = O.route(bins, node_of, np.array([[0, -1]]), np.array([[3, 0]]), np.array([[5, 0]]), np.array([[6, 0]]))
    assert out.tolist() == [[5, 6, -1, -1]]
    leaf = lambda *v: {"value": list(v)}                                              # noqa: E731
    tree = {"f": 0, "thr": 1.0, "left": leaf(1.0, 0.0), "right": {"f": 1, "thr": 0.0, "left": leaf(0.5, 0.5),
                                                                     "right": leaf(0.0, 1.0)}}
    x = np.array([[1.0, 5.0], [np.nan, 0.0], [2.0, np.nan], [-np.inf, np.nan], [np.inf, -np.inf]])
    one = O.predict([tree], x, 2, average=True)
    assert one.tolist() == [[1, 0], [.5, .5], [0, 1], [1, 0], [.5, .5]]
    three = O.predict([tree, leaf(0.25, 0.75), tree], x, 2, average=True)
    assert three[0].tolist() == [2.25 / 3, 0.75 / 3] and three[2].tolist() == [0.25 / 3, 2.75 / 3]


# ---------------------------------------------------------------------------------------------- the CPU branches

@pytest.mark.parametrize("name", list(C.BINIZE_SHAPES))
def test_cpu_binize_matches_oracle(name):
    c = C.binize_case(name)
    assert c["nan_mask"].any() and np.isnan(c["x"][c["nan_mask"]]).all()
    assert (c["expected"][c["nan_mask"]] == np.broadcast_to(c["nsplit"], c["x"].shape)[c["nan_mask"]]).all()
    assert np.array_equal(C.run_binize(CPU, c), c["expected"])


@pytest.mark.parametrize("name", list(C.HIST_CASES))
def test_cpu_histogram_matches_oracle(name):
    import torch
    c = C.hist_case(name)
    eng, wt = C.hist_engine(CPU, c)
    assert np.array_equal(eng.fixed_point_scales(wt), c["scales"])    # the documented scales
    (h,) = C.run_hist(CPU, c)
    assert h.dtype == torch.int64 and torch.equal(h, torch.as_tensor(c["expected"]))


@pytest.mark.parametrize("name", list(C.SPLIT_CASES))
def test_cpu_best_split_matches_oracle(name):
    C.check_best_splits(CPU, name)


def test_split_cases_are_what_they_claim():
    """The data of the K19 cases does what their descriptions say, by the oracle alone."""
    for name in C.SPLIT_CASES:
        c, orc = C.split_case(name), C.split_oracle(name)
        for o, w in zip(orc, c.get("winners", [])):
            assert (o["feature"], o["bin"]) == w, (name, o["feature"], o["bin"], w)
    for name in ("planted_variance", "gini_S16", "entropy_S3"):
        o = C.split_oracle(name)[0]       # the negated copy, the original and the duplicate tie exactly
        g = {(f, b): v for f, b, v, *_ in o["candidates"]}
        assert g[(1, 3)] == g[(2, 3)] == g[(4, 3)] == o["G"]
    none = C.split_oracle("gates_none")[0]
    assert (none["feature"], none["bin"]) == (0, 0)
    assert none["left_i"][0] == 6 * int(C.split_case("gates_none")["scales"][0])     # six rows on the left
    for name in ("gates_min_instances", "gates_min_weight_fraction", "gates_min_gain_below",
                 "gates_fractional_weights"):
        o = C.split_oracle(name)[0]
        want = (0, 0) if name == "gates_min_gain_below" else (1, 3)
        assert (o["feature"], o["bin"]) == want, name
    assert C.split_oracle("gates_min_gain_above")[0]["feature"] == -1
    empty, pure, one_bin = C.split_oracle("degenerate_gini")
    assert empty["feature"] == -1 and not any(empty["tot_i"])
    assert (pure["feature"], pure["gain"], pure["err"]) == (1, 0, 0.0) and one_bin["feature"] == -1
    assert pure["bin"] == int(np.nonzero(C.split_case("degenerate_gini")["hist"][0, 1, 1].sum(-1))[0][0])
    assert [o["feature"] for o in C.split_oracle("degenerate_variance")] == [-1, -1]
    absent = C.split_case("entropy_absent_classes")["hist"][0, 0, 0].sum(0)
    assert sorted(np.nonzero(absent)[0]) == [0, 3, 7]
    assert len(C.split_oracle("nodes_3x64")) == 192


@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_cpu_route_matches_oracle(name):
    c = C.route_case(name)
    assert np.array_equal(C.run_route(CPU, c), c["expected"])


@pytest.mark.parametrize("name", list(C.PREDICT_CASES))
def test_cpu_predict_matches_oracle(name):
    c = C.predict_case(name)
    assert C.same_bits(C.run_predict(CPU, c), c["expected"])


@pytest.mark.parametrize("name", list(C.FIT_SETS))
def test_cpu_fit_routes_training_rows_like_prediction(name):
    """No oracle grows whole trees; what can be checked without one: every leaf of a fit holds the
    rows that prediction sends to it — NaN cells included, which go right in both."""
    eng, trees, pred = C.run_fit(CPU, name)
    assert np.isfinite(pred).all() and any(not t.is_leaf for t in trees)
    if name == "gates_and_weights":
        C.check_leaf_weights(trees[0], C.fit_data())
