"""ClusteringEvaluator on CPU frames: distanceMeasure (squaredEuclidean / cosine), weightCol, the error
cases and the chunked reference form, against sklearn (unweighted) and a numpy oracle written from the
definition (weighted mean distance to every cluster from the cluster statistics)."""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.evaluation import ClusteringEvaluator
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import silhouette_ops as SO
from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession


def oracle(X, lab, w=None, cosine=False, K=None):
    """(silhouette, per-row s) in numpy f64, dense n x K."""
    X = np.asarray(X, np.float64)
    n = len(X)
    w = np.ones(n) if w is None else np.asarray(w, np.float64)
    if cosine:
        X = X / np.linalg.norm(X, axis=1, keepdims=True)
    K = int(lab.max()) + 1 if K is None else K
    W = np.bincount(lab, w, K)
    S = np.zeros((K, X.shape[1]))
    np.add.at(S, lab, X * w[:, None])
    mu = S / np.maximum(W, 1e-300)[:, None]
    if cosine:
        D = 1.0 - X @ mu.T
    else:
        q = np.bincount(lab, w * (X * X).sum(1), K) / np.maximum(W, 1e-300)
        D = (X * X).sum(1)[:, None] - 2 * X @ mu.T + q[None]
    D[:, W == 0] = np.inf
    own = D[np.arange(n), lab]
    D[np.arange(n), lab] = np.inf
    b = D.min(1)
    Wl = W[lab]
    single = Wl == w
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(single, 0.0, own * Wl / np.where(single, 1.0, Wl - w))
        s = np.where(a < b, 1 - a / b, np.where(a > b, b / a - 1, 0.0))
    s = np.where(single, 0.0, s)
    return (s * w).sum() / w.sum(), s


@pytest.fixture(scope="module")
def spark():
    return SparkSession.builder.master("local[1]").getOrCreate()


@pytest.fixture(scope="module")
def blobs():
    rs = np.random.RandomState(0)
    k, d, n = 5, 8, 600
    true = rs.randn(k, d) * 3 + 4
    lab = rs.randint(0, k, n)
    X = true[lab] + rs.randn(n, d)
    flip = rs.rand(n) < 0.1
    lab = np.where(flip, rs.randint(0, k, n), lab)
    return X, lab.astype(np.int32)


def _frame(spark, X, lab, w=None):
    cols = {"features": torch.as_tensor(X), "prediction": torch.as_tensor(lab)}
    if w is not None:
        cols["w"] = torch.as_tensor(w)
    return spark.createDataFrameFromTensors(cols)


@pytest.mark.parametrize("measure,metric", [("squaredEuclidean", "sqeuclidean"), ("cosine", "cosine")])
def test_sklearn_parity(spark, blobs, measure, metric):
    from sklearn.metrics import silhouette_score
    X, lab = blobs
    got = ClusteringEvaluator(distanceMeasure=measure).evaluate(_frame(spark, X, lab))
    assert abs(got - silhouette_score(X, lab, metric=metric)) <= 1e-12
    assert abs(got - oracle(X, lab, cosine=measure == "cosine")[0]) <= 1e-12


def test_default_is_squared_euclidean(spark, blobs):
    X, lab = blobs
    df = _frame(spark, X, lab)
    assert ClusteringEvaluator().evaluate(df) == ClusteringEvaluator(distanceMeasure="squaredEuclidean").evaluate(df)
    assert abs(ClusteringEvaluator().evaluate(df) - ClusteringEvaluator(distanceMeasure="cosine").evaluate(df)) > 1e-3


@pytest.mark.parametrize("measure", ["squaredEuclidean", "cosine"])
def test_weights(spark, blobs, measure):
    """Weights in {0, 1, 2, 3}, a weight-0 row, a singleton cluster (id 6) and an unused id (5)."""
    X, lab = blobs
    rs = np.random.RandomState(1)
    w = rs.randint(0, 4, len(lab)).astype(np.float64)
    lab = lab.copy()
    lab[17] = 6
    w[17] = 2.0
    w[3] = 0.0
    assert (lab == 5).sum() == 0 and (lab == 6).sum() == 1 and (w == 0).sum() > 1
    cos = measure == "cosine"
    want, s = oracle(X, lab, w, cos)
    assert s[17] == 0.0
    got = ClusteringEvaluator(distanceMeasure=measure, weightCol="w").evaluate(_frame(spark, X, lab, w))
    assert abs(got - want) <= 1e-12
    # the weights matter, and integer weights are not row replication (the W / (W - w) factor)
    assert abs(got - oracle(X, lab, None, cos)[0]) > 1e-5
    rep = np.repeat(np.arange(len(lab)), w.astype(int))
    assert abs(got - oracle(X[rep], lab[rep], None, cos, K=7)[0]) > 1e-6


def test_reference_rows(blobs):
    X, lab = blobs
    w = np.random.RandomState(2).randint(0, 4, len(lab)).astype(np.float64)
    for cos in (False, True):
        want, s = oracle(X, lab, w, cos)
        part, own, b, nb, sr = SO.silhouette_reference(torch.as_tensor(X), torch.as_tensor(lab), 5,
                                                       torch.as_tensor(w), cos, rows=True)
        assert abs(float(part[0] / part[1]) - want) <= 1e-12
        assert np.abs(sr.numpy() - s).max() <= 1e-12
        assert ((nb.numpy() != lab) & (nb.numpy() >= 0)).all() and (b >= 0).all() and own.shape == b.shape


def test_chunking(blobs):
    X, lab = blobs
    x, g = torch.as_tensor(X), torch.as_tensor(lab)
    w = torch.as_tensor(np.random.RandomState(3).randint(0, 4, len(lab)).astype(np.float64))
    for cos in (False, True):
        full = SO.silhouette_reference(x, g, 5, w, cos, rows=True, chunk=1 << 16)
        small = SO.silhouette_reference(x, g, 5, w, cos, rows=True, chunk=7)
        assert torch.allclose(SO.cluster_stats_reference(x, g, 5, w, cos, chunk=7),
                              SO.cluster_stats_reference(x, g, 5, w, cos), rtol=0, atol=1e-10)
        assert abs(float(full[0][0] / full[0][1]) - float(small[0][0] / small[0][1])) <= 1e-13
        for a, b in zip(full[1:], small[1:]):
            assert a.shape == b.shape and float((a.double() - b.double()).abs().max()) <= 1e-11


@pytest.mark.parametrize("bad", [-1.0, float("inf"), float("nan")])
def test_bad_weights_raise(spark, blobs, bad):
    X, lab = blobs
    w = np.ones(len(lab))
    w[5] = bad
    with pytest.raises(ValueError, match="weights must be finite and non-negative"):
        ClusteringEvaluator(weightCol="w").evaluate(_frame(spark, X, lab, w))


def test_null_weights_raise(spark, blobs):
    X, lab = blobs
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.feature import VectorAssembler
    rows = [(float(X[i, 0]), float(X[i, 1]), int(lab[i]), None if i == 2 else 1.0) for i in range(20)]
    df = spark.createDataFrame(rows, ["f0", "f1", "prediction", "w"])
    df = VectorAssembler(inputCols=["f0", "f1"], outputCol="features").transform(df)
    with pytest.raises(ValueError, match="contains nulls"):
        ClusteringEvaluator(weightCol="w").evaluate(df)


def test_zero_row_cosine_raises(spark, blobs):
    X, lab = blobs
    X = X.copy()
    X[11] = 0.0
    df = _frame(spark, X, lab)
    with pytest.raises(ValueError, match="Cosine distance is not defined for zero-length vectors."):
        ClusteringEvaluator(distanceMeasure="cosine").evaluate(df)
    assert np.isfinite(ClusteringEvaluator().evaluate(df))  # fine for squaredEuclidean


def test_unknown_measure_and_negative_labels_raise(spark, blobs):
    X, lab = blobs
    with pytest.raises(ValueError, match="distanceMeasure"):
        ClusteringEvaluator(distanceMeasure="manhattan").evaluate(_frame(spark, X, lab))
    neg = lab.copy()
    neg[0] = -1
    with pytest.raises(ValueError, match="negative"):
        ClusteringEvaluator().evaluate(_frame(spark, X, neg))
