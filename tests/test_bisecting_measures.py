"""BisectingKMeans: weightCol (weights equal row repetition, weight-0 rows, bad weights), distanceMeasure="cosine"
(unit centres, cost, heights, scale invariance, zero rows, save / load) and the reference form of one iteration
against the chunked euclidean form."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import session
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import bisecting as B
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import (BisectingKMeans,
                                                                                      BisectingKMeansModel)
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.feature import VectorAssembler
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import bisect_ops as BO
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops.silhouette_ops import ZERO_ROW

# level-wise splitting (Spark): root -> two pairs -> four blobs (tests/test_bisecting.py)
CENTERS = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 30.0], [4.0, 30.0]])


def _blobs(n=600, seed=0):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 4, n)
    return CENTERS[lab] + rs.randn(n, 2) * 0.5, lab, rs.randint(1, 4, n).astype(np.float64)


def _frame(X, w=None):
    cols = {"features": torch.as_tensor(np.ascontiguousarray(X, dtype=np.float64))}
    if w is not None:
        cols["w"] = torch.as_tensor(np.asarray(w, dtype=np.float64))
    return session().createDataFrameFromTensors(cols)


def _pred(m, f):
    return np.asarray(m.transform(f).toPandas().prediction)


def _shape(m):
    """The tree as nested (index, [children]) tuples."""
    def walk(nd):
        return (nd.index, [walk(ch) for ch in nd.children])
    return walk(m._root)


def _leaf_sizes(m):
    return [int(round(nd.size)) for nd in m._leaves]


def test_integer_weights_equal_row_repetition():
    X, _, w = _blobs()
    fa = _frame(X, w)
    rep = np.repeat(np.arange(len(X)), w.astype(int))
    fb = _frame(X[rep])
    a = BisectingKMeans(k=4, seed=3, minDivisibleClusterSize=1.0, weightCol="w").fit(fa)
    b = BisectingKMeans(k=4, seed=3, minDivisibleClusterSize=1.0).fit(fb)
    np.testing.assert_allclose(np.stack(a.clusterCenters()), np.stack(b.clusterCenters()), rtol=1e-12)
    np.testing.assert_allclose(a.trainingCost, b.trainingCost, rtol=1e-9)
    assert _shape(a) == _shape(b) and len(a.clusterCenters()) == 4
    # sizes are row counts: A's are the counts of its rows, B's the repeated counts
    pa = _pred(a, fa)
    assert _leaf_sizes(a) == [int((pa == j).sum()) for j in range(4)]
    assert _leaf_sizes(b) == [int(w[pa == j].sum()) for j in range(4)]
    assert a._root.size == len(X) and b._root.size == int(w.sum())
    assert a.summary.clusterSizes == _leaf_sizes(a)


def test_weight_zero_rows_count_but_do_not_move_anything():
    X, lab, w = _blobs()
    rs = np.random.RandomState(5)
    zl = rs.randint(0, 4, 150)
    Z = CENTERS[zl] + rs.randn(150, 2) * 0.5
    a = BisectingKMeans(k=4, seed=3, weightCol="w").fit(_frame(X, w))
    fz = _frame(np.r_[X, Z], np.r_[w, np.zeros(150)])
    z = BisectingKMeans(k=4, seed=3, weightCol="w").fit(fz)
    np.testing.assert_allclose(np.stack(z.clusterCenters()), np.stack(a.clusterCenters()), rtol=1e-12)
    np.testing.assert_allclose(z.trainingCost, a.trainingCost, rtol=1e-12)
    np.testing.assert_allclose([nd.cost for nd in z._nodes()], [nd.cost for nd in a._nodes()], rtol=1e-12)
    pz = _pred(z, fz)
    assert _leaf_sizes(z) == [int((pz == j).sum()) for j in range(4)]
    assert sum(_leaf_sizes(z)) == 750 and z._root.size == 750 and a._root.size == 600
    assert z.summary.clusterSizes == _leaf_sizes(z)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), None])
def test_bad_weights_raise(bad):
    X, _, w = _blobs(40)
    rows = [(float(r[0]), float(r[1]), float(v)) for r, v in zip(X, w)]
    rows[7] = (rows[7][0], rows[7][1], bad)
    df = session().createDataFrame(rows, "a DOUBLE, b DOUBLE, w DOUBLE")
    f = VectorAssembler(inputCols=["a", "b"], outputCol="features").transform(df)
    with pytest.raises(ValueError):
        BisectingKMeans(k=2, seed=3, weightCol="w").fit(f)


DIRS = np.array([[1.0, 0.15, 0.0], [1.0, -0.15, 0.0], [0.0, 0.15, 1.0], [0.0, -0.15, 1.0]])


def _cones(n=400, seed=2):
    """Four directions in 3 dimensions with small angular noise, row lengths spread over 0.1 .. 100."""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 4, n)
    u = DIRS[lab] / np.linalg.norm(DIRS[lab], axis=1, keepdims=True) + rs.randn(n, 3) * 0.01
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u * (10.0 ** rs.uniform(-1, 2, n))[:, None], lab


def _cos_dist(a, b):
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def test_cosine_fit(tmp_path):
    X, lab = _cones()
    f = _frame(X)
    m = BisectingKMeans(k=4, seed=3, distanceMeasure="cosine").fit(f)
    cs = np.stack(m.clusterCenters())
    assert cs.shape == (4, 3)
    for nd in m._nodes():
        assert abs(np.linalg.norm(nd.center) - 1.0) <= 1e-12
    pred = _pred(m, f)
    for c in range(4):
        assert len(np.unique(pred[lab == c])) == 1
    assert len(np.unique(pred)) == 4
    want = float(_cos_dist(X, cs[pred]).sum())
    np.testing.assert_allclose(m.trainingCost, want, rtol=1e-9)
    np.testing.assert_allclose(m.computeCost(f), want, rtol=1e-6)
    # scaling every row by a positive factor changes no prediction
    scale = np.random.RandomState(9).uniform(0.01, 50.0, len(X))[:, None]
    np.testing.assert_array_equal(_pred(m, _frame(X * scale)), pred)
    assert m.predict(X[0] * 7.0) == pred[0]
    internal = [nd for nd in m._nodes() if nd.children]
    assert len(internal) == 3
    for nd in internal:
        far = max(float(_cos_dist(nd.center, ch.center)) for ch in nd.children)
        assert abs(nd.height - far) <= 1e-12
    # save / load: the loaded model predicts with the saved measure
    p = str(tmp_path / "bkm_cos")
    m.write().overwrite().save(p)
    with open(os.path.join(p, "data", "metadata", "part-00000")) as fh:
        assert json.loads(fh.readline())["distanceMeasure"] == "cosine"
    back = BisectingKMeansModel.load(p)
    assert back.getDistanceMeasure() == "cosine"
    np.testing.assert_array_equal(_pred(back, _frame(X * scale)), pred)


def test_cosine_zero_row_raises():
    X, _ = _cones(50)
    X[11] = 0.0
    with pytest.raises(ValueError, match=ZERO_ROW[:30]):
        BisectingKMeans(k=2, seed=3, distanceMeasure="cosine").fit(_frame(X))


def test_unknown_measure_raises():
    X, _ = _cones(20)
    with pytest.raises(ValueError, match="distanceMeasure"):
        BisectingKMeans(k=2, distanceMeasure="manhattan").fit(_frame(X))


class _Capture:
    """Stands in for the communicator of one rank and keeps the summed statistics."""

    def allreduce_(self, t, op="sum"):
        self.t = t.clone()
        return t


def test_reference_step_matches_chunked_form():
    rs = np.random.RandomState(4)
    n, d = 700, 5
    node = rs.choice([4, 5, 6, 7], n)  # 7 is not divided on this level
    x = torch.as_tensor(rs.randn(n, d) + 5.0 + node[:, None])
    idx = torch.as_tensor(node.astype(np.int64))
    dvi = [4, 5, 6]
    centers = {c: rs.randn(d) * 0.5 + 5.0 + c // 2 for c in (8, 9, 10, 11, 12)}  # 13: a dead child
    child_idx = B._update_assignments(x, idx, dvi, centers)
    cap = _Capture()
    keys = [c for i in dvi for c in (2 * i, 2 * i + 1)]
    B._summarize(x, child_idx, keys, cap)
    tab = np.zeros((3, 2, d))
    alive = np.zeros((3, 2), dtype=bool)
    for j, i in enumerate(dvi):
        for h in (0, 1):
            if 2 * i + h in centers:
                tab[j, h], alive[j, h] = centers[2 * i + h], True
    slot = torch.as_tensor(np.where(node == 7, -1, node - 4))
    choice, stats = BO.bisect_step_reference(x, slot, torch.as_tensor(tab), torch.as_tensor(alive), chunk=256)
    want = torch.where(slot >= 0, 2 * idx + choice.to(torch.int64), idx)
    assert torch.equal(want, child_idx)
    assert set(child_idx.tolist()) == {7, 8, 9, 10, 11, 12}
    old = cap.t.numpy()  # [S | n | Q]
    new = stats.numpy()  # [S | W | Q | N]
    np.testing.assert_allclose(new[:, :d], old[:, :d], rtol=1e-13)
    np.testing.assert_allclose(new[:, d + 1], old[:, d + 1], rtol=1e-13)
    np.testing.assert_array_equal(new[:, d], old[:, d])
    np.testing.assert_array_equal(new[:, d + 2], old[:, d])
    assert not new[5].any() and new[4, d + 2] == (node == 6).sum()
    # the choices alone
    only, none = BO.bisect_step_reference(x, slot, torch.as_tensor(tab), torch.as_tensor(alive), want_sums=False)
    assert none is None and torch.equal(only, choice)
