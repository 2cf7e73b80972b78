"""NaiveBayes(modelType="complement") against sklearn's ComplementNB(norm=False), a loop transcription of Spark's
formulas, and the model's own surface (save / load, predict, thresholds, the checks)."""
import math

import numpy as np
import pytest
from sklearn.naive_bayes import ComplementNB

from helpers import session
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import NaiveBayes, NaiveBayesModel
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.feature import VectorAssembler
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.linalg import Vectors


def _frame(X, y, w=None):
    spark = session()
    names = [f"x{j}" for j in range(X.shape[1])]
    w = np.ones(len(y)) if w is None else w
    rows = [tuple(map(float, r)) + (float(t), float(u)) for r, t, u in zip(X, y, w)]
    df = spark.createDataFrame(rows, ", ".join(f"{c} DOUBLE" for c in names) + ", label DOUBLE, w DOUBLE")
    return VectorAssembler(inputCols=names, outputCol="features").transform(df)


def _col(df, name):
    return np.stack(df.toPandas()[name].map(lambda v: v.toArray()))


def _counts():
    rs = np.random.RandomState(0)
    y = rs.randint(0, 3, 1500)
    X = rs.poisson(1.0 + 2.0 * np.eye(3)[y] @ rs.rand(3, 5))
    return X, y, rs.uniform(0.2, 3.0, 1500)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("lam", [1.0, 0.7])
def test_complement_matches_sklearn(weighted, lam):
    X, y, w = _counts()
    f = _frame(X, y, w)
    nb = NaiveBayes(modelType="complement", smoothing=lam)
    if weighted:
        nb = nb.setWeightCol("w")
    else:
        w = np.ones(len(y))
    m = nb.fit(f)
    sk = ComplementNB(alpha=lam, norm=False).fit(X, y, sample_weight=w)
    np.testing.assert_allclose(m.theta.toArray(), sk.feature_log_prob_, rtol=1e-10)
    n_c = np.bincount(y, weights=w)
    np.testing.assert_allclose(m.pi.toArray(), np.log(n_c + lam) - math.log(n_c.sum() + 3 * lam), rtol=1e-12)
    assert m.sigma.toArray().size == 0 and m.numClasses == 3 and m.numFeatures == 5
    out = m.transform(f)
    raw, prob = _col(out, "rawPrediction"), _col(out, "probability")
    np.testing.assert_array_equal(np.asarray(out.toPandas().prediction), sk.predict(X))
    np.testing.assert_allclose(np.log(np.exp(raw).sum(1)), 0.0, atol=1e-12)
    np.testing.assert_allclose(prob, np.exp(raw), rtol=1e-12)
    np.testing.assert_allclose(prob.sum(1), 1.0, rtol=1e-12)


def test_complement_against_the_formulas_written_out():
    X = np.array([[1.0, 0.0, 2.0], [0.0, 3.0, 1.0], [2.0, 1.0, 0.0], [0.0, 0.0, 4.0]])
    y = np.array([0, 1, 0, 1])
    w = np.array([1.0, 2.0, 0.5, 1.5])
    lam, C, d = 0.7, 2, 3
    S = [[0.0] * d for _ in range(C)]
    n = [0.0] * C
    for r in range(4):
        n[y[r]] += w[r]
        for i in range(d):
            S[y[r]][i] += w[r] * X[r, i]
    theta = [[0.0] * d for _ in range(C)]
    pi = [0.0] * C
    for c in range(C):
        comp = [sum(S[k][i] for k in range(C)) - S[c][i] for i in range(d)]
        for i in range(d):
            theta[c][i] = -(math.log(comp[i] + lam) - math.log(sum(comp) + d * lam))
        pi[c] = math.log(n[c] + lam) - math.log(sum(n) + C * lam)
    f = _frame(X, y, w)
    m = NaiveBayes(modelType="complement", smoothing=lam, weightCol="w").fit(f)
    np.testing.assert_allclose(m.theta.toArray(), theta, rtol=1e-13)
    np.testing.assert_allclose(m.pi.toArray(), pi, rtol=1e-13)
    out = m.transform(f)
    raw = _col(out, "rawPrediction")
    for r in range(4):
        s = [sum(theta[c][i] * X[r, i] for i in range(d)) for c in range(C)]  # pi is not added
        top = max(s)
        lse = top + math.log(sum(math.exp(v - top) for v in s))
        np.testing.assert_allclose(raw[r], [v - lse for v in s], rtol=1e-12, atol=1e-14)
        assert out.toPandas().prediction[r] == float(np.argmax(s))
        assert m.predict(Vectors.dense(X[r])) == float(np.argmax(s))


def test_complement_save_load_predict_and_thresholds(tmp_path):
    X, y, _ = _counts()
    f = _frame(X, y)
    m = NaiveBayes(modelType="complement").fit(f)
    out = m.transform(f)
    p = str(tmp_path / "cnb")
    m.write().overwrite().save(p)
    m2 = NaiveBayesModel.load(p)
    assert m2.getModelType() == "complement"
    np.testing.assert_array_equal(m2.theta.toArray(), m.theta.toArray())
    np.testing.assert_array_equal(m2.pi.toArray(), m.pi.toArray())
    assert m2.sigma.toArray().size == 0
    np.testing.assert_allclose(_col(m2.transform(f), "probability"), _col(out, "probability"), rtol=1e-12)
    pred = np.asarray(out.toPandas().prediction)
    for r in (0, 7, 300):
        assert m.predict(Vectors.dense(X[r].astype(float))) == pred[r]
    # thresholds: argmax of probability / threshold, as the other types do it
    thr = [0.1, 0.6, 0.3]
    mt = NaiveBayes(modelType="complement", thresholds=thr).fit(f)
    outt = mt.transform(f)
    prob = _col(outt, "probability")
    np.testing.assert_array_equal(np.asarray(outt.toPandas().prediction), np.argmax(prob / np.array(thr), 1))
    assert (np.asarray(outt.toPandas().prediction) != pred).any()


def test_complement_checks():
    X, y, _ = _counts()
    Xn = X.astype(float).copy()
    Xn[3, 1] = -1.0
    with pytest.raises(ValueError, match="non-negative feature values"):
        NaiveBayes(modelType="complement").fit(_frame(Xn, y))
    with pytest.raises(ValueError) as e:
        NaiveBayes(modelType="poisson").fit(_frame(X, y))
    for name in ("multinomial", "bernoulli", "gaussian", "complement"):
        assert name in str(e.value)
    assert "complement" in NaiveBayes().explainParam("modelType")
