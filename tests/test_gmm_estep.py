"""GaussianMixture's E-step in its reference form (``ops/gmm_ops.py``) against a dense numpy / scipy evaluation
of the definitions, the weight validation of the estimator, and the untouched dense path of CPU frames."""
import math

import numpy as np
import pytest
import torch
from scipy.stats import multivariate_normal

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import gmm as G
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import GaussianMixture
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.feature import VectorAssembler
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import gmm_ops as GO

N, D, K = 1001, 5, 3
_cache = {}


@pytest.fixture(scope="module")
def spark():
    """A host session of this module's own, beside whichever session is active (on a GPU machine the shared
    session may be a device one, and these tests are about CPU frames); the modules that follow find the active
    session as they would without this one."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    s = SparkSession({"spark.master": "local", "spark.app.name": "gmm-cpu"})
    assert s.device.type == "cpu"
    yield s
    s.stop()


def _case():
    """Rows, integer weights in {0..3}, mixture parameters and the dense oracle (made once, never modified)."""
    if _cache:
        return _cache
    rs = np.random.RandomState(5)
    cen = rs.uniform(-4.0, 4.0, (K, D))
    x = cen[rs.randint(0, K, N)] + rs.randn(N, D)
    w = rs.randint(0, 4, N).astype(np.float64)
    pi = np.array([0.2, 0.5, 0.3])
    mus = cen + 0.3 * rs.randn(K, D)
    covs = np.stack([(lambda B: B @ B.T / D + 0.5 * np.eye(D))(rs.randn(D, D)) for _ in range(K)])
    A, c = G._estep_tables(pi, covs)
    lp = np.stack([np.log(pi[j]) + multivariate_normal.logpdf(x, mus[j], covs[j]) for j in range(K)], 1)
    m = lp.max(1)
    lse = m + np.log(np.exp(lp - m[:, None]).sum(1))
    p = np.exp(lp - lse[:, None])
    _cache.update(x=x, w=w, A=A, mu=mus, c=c, lp=lp, lse=lse, p=p)
    return _cache


def _dense(C, w):
    r = C["p"] * w[:, None]
    x = C["x"]
    S2 = np.einsum("nk,na,nb->kab", r, x, x)
    stats = np.concatenate([r.sum(0)[:, None], r.T @ x, S2.reshape(K, D * D)], 1)
    return stats, np.array([(w * C["lse"]).sum(), w.sum()])


def test_tables_are_the_definition():
    rs = np.random.RandomState(1)
    B = rs.randn(D, D)
    cov = B @ B.T + np.eye(D)
    A, c = G._estep_tables(np.array([0.25, 0.75]), np.stack([cov, 2.0 * cov]))
    L = np.linalg.cholesky(cov)
    np.testing.assert_allclose(A[0] @ L, np.eye(D), atol=1e-13)
    assert not np.triu(A[0], 1).any()
    want = math.log(0.25) - 0.5 * (D * math.log(2.0 * math.pi) + np.linalg.slogdet(cov)[1])
    np.testing.assert_allclose(c[0], want, rtol=1e-13)


@pytest.mark.parametrize("chunk", [7, 4096])
@pytest.mark.parametrize("weighted", [False, True])
def test_estep_reference_against_dense(chunk, weighted):
    C = _case()
    w = C["w"] if weighted else np.ones(N)
    want_s, want_t = _dense(C, w)
    stats, tail = GO.estep_reference(torch.as_tensor(C["x"]), D, torch.as_tensor(w) if weighted else None,
                                     C["A"], C["mu"], C["c"], chunk=chunk)
    assert stats.shape == (K, 1 + D + D * D) and tail.shape == (2,)
    np.testing.assert_allclose(stats.numpy(), want_s, rtol=1e-11)
    np.testing.assert_allclose(tail.numpy(), want_t, rtol=1e-11)
    S2 = stats[:, 1 + D:].reshape(K, D, D)
    assert torch.equal(S2, S2.transpose(1, 2))
    prob, label = GO.predict_reference(torch.as_tensor(C["x"]), D, None, C["A"], C["mu"], C["c"], chunk=chunk)
    np.testing.assert_allclose(prob.numpy(), C["p"], rtol=1e-11, atol=1e-300)
    assert label.dtype == torch.int32 and np.array_equal(label.numpy(), C["lp"].argmax(1))


def test_zero_weight_rows_change_nothing():
    C = _case()
    keep = C["w"] > 0
    assert 0 < keep.sum() < N
    full = GO.estep_reference(torch.as_tensor(C["x"]), D, torch.as_tensor(C["w"]), C["A"], C["mu"], C["c"], chunk=N)
    some = GO.estep_reference(torch.as_tensor(C["x"][keep]), D, torch.as_tensor(C["w"][keep]), C["A"], C["mu"],
                              C["c"], chunk=N)
    mass = _dense(dict(C, x=np.abs(C["x"])), C["w"])[0]
    assert (np.abs(full[0].numpy() - some[0].numpy()) <= 1e-12 * mass).all()
    np.testing.assert_allclose(full[1].numpy(), some[1].numpy(), rtol=1e-12)


def test_integer_weights_are_repeated_rows():
    C = _case()
    rep = np.repeat(C["x"], C["w"].astype(np.int64), axis=0)
    a = GO.estep_reference(torch.as_tensor(C["x"]), D, torch.as_tensor(C["w"]), C["A"], C["mu"], C["c"], chunk=300)
    b = GO.estep_reference(torch.as_tensor(rep), D, None, C["A"], C["mu"], C["c"], chunk=300)
    mass = _dense(dict(C, x=np.abs(C["x"])), C["w"])[0]
    assert (np.abs(a[0].numpy() - b[0].numpy()) <= 1e-12 * mass).all()
    assert abs(a[1][0].item() - b[1][0].item()) <= 1e-12 * (C["w"] * np.abs(C["lse"])).sum()
    assert a[1][1].item() == b[1][1].item() == C["w"].sum()


def test_reference_takes_low_precision_rows_and_pad_columns():
    """bf16 and e4m3 rows are widened chunk by chunk; columns past d are never read."""
    C = _case()
    nan = torch.full((N, 3), float("nan"), dtype=torch.float32)
    for dt in (torch.bfloat16, torch.float8_e4m3fn):
        wide = torch.as_tensor(C["x"]).to(torch.float32).to(dt).to(torch.float32)
        low = torch.cat([wide, nan], 1).to(dt)
        a = GO.estep_reference(low, D, None, C["A"], C["mu"], C["c"], chunk=100)
        b = GO.estep_reference(wide.to(torch.float64), D, None, C["A"], C["mu"], C["c"], chunk=100)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.isfinite(a[0]).all()


def _blobs(n=600, seed=2):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 2, n)
    x = np.where(lab[:, None] == 0, [-5.0, 0.0, 2.0], [5.0, 1.0, -2.0]) + 0.5 * rs.randn(n, 3)
    return x, lab, rs.randint(1, 4, n).astype(np.float64)


def test_cpu_frames_keep_the_dense_path(spark, monkeypatch):
    """A CPU f64 frame and a CPU bf16 frame fit with every gmm_ops entry raising."""
    def boom(*a, **k):
        raise AssertionError("the dense path must not call into gmm_ops")
    for name in ("estep", "predict", "estep_reference", "predict_reference", "kernel_enabled", "kernel_supported",
                 "gather_rows", "column_moments"):
        monkeypatch.setattr(GO, name, boom)
    x, lab, w = _blobs()
    for feats in (torch.as_tensor(x), torch.as_tensor(x).to(torch.bfloat16)):
        df = spark.createDataFrameFromTensors({"features": feats, "w": torch.as_tensor(w)})
        assert not df._feature_matrix("features").is_cuda
        m = GaussianMixture(k=2, seed=1, maxIter=20, weightCol="w").fit(df)
        mus = np.stack([g[0].toArray() for g in m.gaussians])
        assert sorted(np.round(mus[:, 0]).tolist()) == [-5.0, 5.0]
        pred = m.transform(df)._column_data("prediction").values.numpy()
        assert max((pred == lab).mean(), (pred != lab).mean()) > 0.99


@pytest.mark.parametrize("bad", [-1.0, float("nan"), None])
def test_bad_weight_raises(spark, bad):
    x, _, w = _blobs(60)
    rows = [tuple(float(v) for v in r) + (float(wi),) for r, wi in zip(x, w)]
    rows[7] = rows[7][:3] + (bad,)
    df = spark.createDataFrame(rows, "a DOUBLE, b DOUBLE, c DOUBLE, w DOUBLE")
    df = VectorAssembler(inputCols=["a", "b", "c"], outputCol="features").transform(df)
    with pytest.raises(ValueError, match="weight"):
        GaussianMixture(k=2, seed=1, maxIter=3, weightCol="w").fit(df)


def test_weighted_fit_recovers_blobs(spark):
    x, lab, w = _blobs()
    df = spark.createDataFrameFromTensors({"features": torch.as_tensor(x), "w": torch.as_tensor(w)})
    m = GaussianMixture(k=2, seed=1, maxIter=50, tol=1e-6, weightCol="w").fit(df)
    order = np.argsort([g[0].toArray()[0] for g in m.gaussians])
    mus = np.stack([m.gaussians[i][0].toArray() for i in order])
    np.testing.assert_allclose(mus, [[-5.0, 0.0, 2.0], [5.0, 1.0, -2.0]], atol=0.15)
    share = np.array([w[lab == 0].sum(), w[lab == 1].sum()]) / w.sum()
    np.testing.assert_allclose(np.array(m.weights)[order], share, atol=1e-3)
