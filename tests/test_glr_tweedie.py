"""GeneralizedLinearRegression: family="tweedie" (variancePower, linkPower), offsetCol, and the reference form of the
fused IRLS step (``ops/glr_ops.py``), against sklearn, the named families, identities that hold in real arithmetic and
the formulas written out in numpy."""
import numpy as np
import pytest
import torch
from sklearn.linear_model import TweedieRegressor

from helpers import session
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import (
    GeneralizedLinearRegression, GeneralizedLinearRegressionModel)
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import glr_ops as GO

GLR = GeneralizedLinearRegression


@pytest.fixture(scope="module", autouse=True)
def _own_session():
    """A session made by this module is stopped with it: later modules choose their own."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    act = SparkSession.getActiveSession()
    mine = act is None or act._stopped
    yield
    now = SparkSession.getActiveSession()
    if mine and now is not None and not now._stopped:
        now.stop()


def _frame(X, y, **cols):
    data = {"features": torch.as_tensor(np.asarray(X, dtype=np.float64)), "label": torch.as_tensor(np.asarray(y, float))}
    data.update({k: torch.as_tensor(np.asarray(v, float)) for k, v in cols.items()})
    return session().createDataFrameFromTensors(data)


def _coef(m):
    return np.r_[m.coefficients.toArray(), m.intercept]


@pytest.fixture(scope="module")
def X():
    rs = np.random.RandomState(0)
    return rs.randn(3000, 3) * [0.5, 0.3, 0.8]


@pytest.fixture(scope="module")
def cost(X):
    """Compound Poisson-gamma labels (tweedie p = 1.5, dispersion 0.8) with a log mean: about 7 % exact zeros."""
    rs = np.random.RandomState(7)
    p, phi = 1.5, 0.8
    mu = np.exp(X @ [0.4, -0.3, 0.2] + 1.0)
    cnt = rs.poisson(mu ** (2 - p) / (phi * (2 - p)))
    y = np.where(cnt > 0, rs.gamma(np.maximum(cnt, 1) * (2 - p) / (p - 1), phi * (p - 1) * mu ** (p - 1)), 0.0)
    assert 0 < (y == 0).sum() < len(y) / 2
    return y


@pytest.fixture(scope="module")
def counts(X):
    rs = np.random.RandomState(2)
    e = rs.uniform(0.5, 3.0, len(X))
    return rs.poisson(e * np.exp(X @ [0.4, -0.3, 0.2] + 0.5)).astype(float), e


def _np_poisson(A, y, off, iters=100):
    """Poisson / log IRLS on the design A (an intercept is a column of ones) with an offset, in numpy."""
    b = np.zeros(A.shape[1])
    mu = np.maximum(y, 0.1)
    eta = np.log(mu)
    for _ in range(iters):
        z = eta - off + (y - mu) / mu
        nb = np.linalg.solve(A.T @ (A * mu[:, None]), A.T @ (mu * z))
        done = np.abs(nb - b).max() < 1e-14
        b = nb
        eta = A @ b + off
        mu = np.exp(eta)
        if done:
            break
    return b


def test_tweedie_log_matches_sklearn(X, cost):
    m = GLR(family="tweedie", variancePower=1.5, linkPower=0.0, tol=1e-10).fit(_frame(X, cost))
    sk = TweedieRegressor(power=1.5, alpha=0, link="log", tol=1e-12, max_iter=10000).fit(X, cost)
    np.testing.assert_allclose(m.coefficients.toArray(), sk.coef_, rtol=1e-5, atol=1e-6)
    assert abs(m.intercept - sk.intercept_) < 1e-6
    assert 2 < m.summary.numIterations <= 25


def test_tweedie_equals_the_named_families(X, cost, counts):
    rs = np.random.RandomState(3)
    lin = X @ [1.0, -2.0, 0.5] + 3 + 0.1 * rs.randn(len(X))
    pos = rs.gamma(2.0, 1.0 / (2.0 * (X @ [0.3, 0.1, -0.2] + 2.0)))
    for p, lp, family, y in ((0.0, 1.0, "gaussian", lin), (1.0, 0.0, "poisson", counts[0]), (2.0, -1.0, "gamma", pos)):
        f = _frame(X, y)
        a = GLR(family="tweedie", variancePower=p, linkPower=lp, tol=1e-12).fit(f)
        b = GLR(family=family, tol=1e-12).fit(f)
        np.testing.assert_allclose(_coef(a), _coef(b), rtol=1e-9, err_msg=family)
        np.testing.assert_allclose(a.summary.deviance, b.summary.deviance, rtol=1e-9, err_msg=family)
        np.testing.assert_allclose(a.summary.nullDeviance, b.summary.nullDeviance, rtol=1e-9, err_msg=family)


def test_default_link_power_is_one_minus_p(X, cost):
    f = _frame(X, cost)
    a = GLR(family="tweedie", variancePower=1.5, tol=1e-12).fit(f)
    b = GLR(family="tweedie", variancePower=1.5, linkPower=-0.5, tol=1e-12).fit(f)
    c = GLR(family="tweedie", variancePower=1.5, linkPower=0.0, tol=1e-12).fit(f)
    assert a._family_link() == ("tweedie", -0.5)
    np.testing.assert_array_equal(_coef(a), _coef(b))
    assert np.abs(_coef(a) - _coef(c)).max() > 0.1
    # link="log" is ignored for tweedie
    d = GLR(family="tweedie", variancePower=1.5, link="log", tol=1e-12).fit(f)
    np.testing.assert_array_equal(_coef(a), _coef(d))
    mu = (X @ a.coefficients.toArray() + a.intercept) ** -2.0
    np.testing.assert_allclose(a.transform(f)._column_data("prediction").values.numpy(), mu, rtol=1e-12)


def test_deviance_and_dispersion(X, cost):
    y, p = cost, 1.5
    rs = np.random.RandomState(5)
    w = rs.uniform(0.5, 2.0, len(y))
    m = GLR(family="tweedie", variancePower=p, linkPower=0.0, weightCol="w", tol=1e-12).fit(_frame(X, y, w=w))
    mu = np.exp(X @ m.coefficients.toArray() + m.intercept)

    def dev(mu):
        y1 = np.maximum(y, 0.1)
        return np.sum(2 * w * (y * (y1 ** (1 - p) - mu ** (1 - p)) / (1 - p) - (y ** (2 - p) - mu ** (2 - p)) / (2 - p)))
    s = m.summary
    np.testing.assert_allclose(s.deviance, dev(mu), rtol=1e-10)
    np.testing.assert_allclose(s.nullDeviance, dev(np.full_like(y, np.sum(w * y) / np.sum(w))), rtol=1e-10)
    assert s.residualDegreeOfFreedom == len(y) - 4 and s.residualDegreeOfFreedomNull == len(y) - 1
    np.testing.assert_allclose(s.dispersion, np.sum(w * (y - mu) ** 2 / mu ** p) / (len(y) - 4), rtol=1e-10)
    assert s.deviance < s.nullDeviance


def test_rate_identity(X, counts):
    """poisson on counts with offset log(e) = poisson on the rates y / e with weight e."""
    y, e = counts
    a = GLR(family="poisson", offsetCol="off", tol=1e-12).fit(_frame(X, y, off=np.log(e)))
    b = GLR(family="poisson", weightCol="e", tol=1e-12).fit(_frame(X, y / e, e=e))
    np.testing.assert_allclose(a.coefficients.toArray(), b.coefficients.toArray(), rtol=1e-9)
    np.testing.assert_allclose(a.intercept, b.intercept, rtol=1e-9)
    assert a.summary.dispersion == 1.0


def test_constant_offset_moves_the_intercept(X, counts):
    y, _ = counts
    c = 0.7
    a = GLR(family="poisson", offsetCol="off", tol=1e-12).fit(_frame(X, y, off=np.full(len(y), c)))
    b = GLR(family="poisson", tol=1e-12).fit(_frame(X, y))
    np.testing.assert_allclose(a.coefficients.toArray(), b.coefficients.toArray(), rtol=1e-9)
    np.testing.assert_allclose(a.intercept, b.intercept - c, rtol=1e-9)
    np.testing.assert_allclose(a.summary.deviance, b.summary.deviance, rtol=1e-9)


def test_offset_without_intercept(X, counts):
    y, e = counts
    off = np.log(e) + 0.5
    m = GLR(family="poisson", offsetCol="off", fitIntercept=False, tol=1e-12).fit(_frame(X, y, off=off))
    want = _np_poisson(X, y, off)
    assert m.intercept == 0.0
    np.testing.assert_allclose(m.coefficients.toArray(), want, rtol=1e-8)
    mu0 = np.exp(off)  # the null model of a fit without intercept is the offset alone
    nd = 2 * np.sum(np.where(y > 0, y * np.log(np.where(y > 0, y, 1) / mu0), 0) - (y - mu0))
    np.testing.assert_allclose(m.summary.nullDeviance, nd, rtol=1e-10)
    assert m.summary.residualDegreeOfFreedomNull == len(y)


def test_null_deviance_with_offset_and_intercept(X, counts):
    y, e = counts
    off = np.log(e)
    m = GLR(family="poisson", offsetCol="off", tol=1e-12).fit(_frame(X, y, off=off))
    c = _np_poisson(np.ones((len(y), 1)), y, off)[0]
    np.testing.assert_allclose(c, np.log(y.sum() / e.sum()), rtol=1e-12)  # the closed form of this scalar problem
    mu0 = np.exp(off + c)
    nd = 2 * np.sum(np.where(y > 0, y * np.log(np.where(y > 0, y, 1) / mu0), 0) - (y - mu0))
    np.testing.assert_allclose(m.summary.nullDeviance, nd, rtol=1e-9)
    assert m.summary.deviance < m.summary.nullDeviance


def test_rejections(X, cost):
    with pytest.raises(ValueError):
        GLR(family="tweedie", variancePower=0.5).fit(_frame(X, cost))
    with pytest.raises(ValueError):
        GLR(family="tweedie", variancePower=-1.0).fit(_frame(X, cost))
    with pytest.raises(ValueError):
        GLR(family="tweedie", variancePower=1.5).fit(_frame(X, cost - 1.0))
    with pytest.raises(ValueError):
        GLR(family="tweedie", variancePower=2.0).fit(_frame(X, cost))  # zero labels
    with pytest.raises(ValueError):
        GLR(family="nope", offsetCol="off").fit(_frame(X, cost, off=cost))


def test_model_save_load_transform_predict(X, cost, tmp_path):
    rs = np.random.RandomState(9)
    off = rs.uniform(-0.3, 0.3, len(X))
    f = _frame(X, cost, off=off)
    m = GLR(family="tweedie", variancePower=1.5, linkPower=0.0, offsetCol="off", linkPredictionCol="eta",
            tol=1e-10).fit(f)
    beta, b0 = m.coefficients.toArray(), m.intercept
    out = m.transform(f)
    np.testing.assert_allclose(out._column_data("eta").values.numpy(), X @ beta + b0 + off, rtol=1e-12)
    np.testing.assert_allclose(out._column_data("prediction").values.numpy(), np.exp(X @ beta + b0 + off), rtol=1e-12)
    assert m.predict(X[0], 0.25) == pytest.approx(np.exp(X[0] @ beta + b0 + 0.25), rel=1e-12)
    assert m.predict(X[0]) == pytest.approx(np.exp(X[0] @ beta + b0), rel=1e-12)
    p = str(tmp_path / "glr")
    m.write().overwrite().save(p)
    back = GeneralizedLinearRegressionModel.load(p)
    assert back.getFamily() == "tweedie" and back.getVariancePower() == 1.5 and back.getLinkPower() == 0.0
    assert back.getOffsetCol() == "off" and back._family_link() == ("tweedie", 0.0)
    np.testing.assert_array_equal(back.transform(f)._column_data("prediction").values.numpy(),
                                  out._column_data("prediction").values.numpy())
    # without an offset column: tweedie alone, and the default link power after a load
    g = _frame(X, cost)
    m2 = GLR(family="tweedie", variancePower=1.5, tol=1e-10).fit(g)
    pred = m2.transform(g)._column_data("prediction").values.numpy()
    np.testing.assert_allclose(pred, (X @ m2.coefficients.toArray() + m2.intercept) ** -2.0, rtol=1e-12)
    assert m2.predict(X[0], 5.0) == pytest.approx(pred[0], rel=1e-12)  # no offsetCol: the offset is not used
    p2 = str(tmp_path / "glr2")
    m2.write().overwrite().save(p2)
    np.testing.assert_array_equal(GeneralizedLinearRegressionModel.load(p2).transform(g)._column_data(
        "prediction").values.numpy(), pred)


# ------------------------------------------------------------------------------------------ the reference step
def _dense_step(x, y, w, off, coef, p, lp, logit, init):
    """[X 1 z]^T diag(wt) [X 1 z] and the four stats, written out in numpy for tweedie (p, lp) and binomial / logit."""
    n, d = x.shape
    if init:
        mu = (w * y + 0.5) / (w + 1.0) if logit else np.where((y == 0) & (1 <= p < 2), 0.1, y)
        eta = np.log(mu / (1 - mu)) if logit else (np.log(mu) if lp == 0 else mu ** lp)
    else:
        eta = x @ coef[:d] + coef[d] + off
        with np.errstate(over="ignore"):
            mu = 1 / (1 + np.exp(-eta)) if logit else (np.exp(eta) if lp == 0 else eta ** (1 / lp))
        mu = np.clip(mu, 1e-16, 1 - 1e-16 if logit else np.finfo(float).max)
    with np.errstate(all="ignore"):
        gp = 1 / (mu * (1 - mu)) if logit else (1 / mu if lp == 0 else lp * mu ** (lp - 1))
        V = mu * (1 - mu) if logit else mu ** p
        z = eta - off + (y - mu) * gp
        wt = w / (gp * gp * V)
        if logit:
            dev = 2 * (np.where(y > 0, y * np.log(np.where(y > 0, y, 1) / mu), 0)
                       + np.where(y < 1, (1 - y) * np.log(np.where(y < 1, 1 - y, 1) / (1 - mu)), 0))
        else:
            def yp(a, e):
                return np.log(a / mu) if e == 0 else (a ** e - mu ** e) / e
            dev = 2 * (y * yp(np.maximum(y, 0.1) if 1 <= p < 2 else y, 1 - p) - yp(y, 2 - p))
        pe = (y - mu) ** 2 / V
    live = w != 0
    z, wt = np.where(live, z, 0.0), np.where(live, wt, 0.0)
    A = np.c_[x, np.ones(n), z]
    stats = np.array([np.sum(np.where(live, w * dev, 0.0)), np.sum(np.where(live, w * pe, 0.0)),
                      np.sum(np.where(live, w * y, 0.0)), w.sum()])
    return A.T @ (A * wt[:, None]), stats


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
def test_step_reference_against_dense_numpy(dtype, monkeypatch):
    monkeypatch.setattr(GO, "CHUNK", 100)
    rs = np.random.RandomState(12)
    n, d = 250, 5  # chunks of 100, 100 and 50 rows
    xt = torch.as_tensor(rs.randn(n, d)).to(dtype)
    x = xt.to(torch.float64).numpy()
    w = rs.rand(n)
    w[rs.rand(n) < 0.1] = 0.0
    off = rs.uniform(-0.3, 0.3, n)
    dead = np.flatnonzero(w == 0)
    assert len(dead) > 5
    off[dead[:5]] = 1e4
    coef = np.r_[0.3 * rs.randn(d) / np.sqrt(d), 2.0]
    ypos = rs.gamma(2.0, 1.0, n)
    ycp = np.where(rs.rand(n) < 0.2, 0.0, ypos)
    ybin = (rs.rand(n) < 0.5).astype(float)
    cases = [(GO.spec("tweedie", None, 1.5, 0.0), ycp, 1.5, 0.0, False),
             (GO.spec("tweedie", None, 1.5, None), ycp, 1.5, -0.5, False),
             (GO.spec("tweedie", None, 2.5, 0.0), ypos, 2.5, 0.0, False),
             (GO.spec("tweedie", None, 0.0, None), ypos - 1.0, 0.0, 1.0, False),
             (GO.spec("binomial", "logit"), ybin, 0.0, 0.0, True)]
    T = torch.as_tensor
    for s, y, p, lp, logit in cases:
        for init in (True, False):
            G, st = GO.step_reference(xt, d, T(y), T(w), T(off), coef, s, init)
            wantG, wantst = _dense_step(x, y, w, off, coef, p, lp, logit, init)
            assert G.dtype == torch.float64 and G.shape == (d + 2, d + 2) and torch.equal(G, G.T)
            assert torch.isfinite(G).all() and torch.isfinite(st).all()
            np.testing.assert_allclose(G.numpy(), wantG, rtol=1e-11, atol=1e-11 * np.abs(wantG).max())
            np.testing.assert_allclose(st.numpy(), wantst, rtol=1e-11)
            # rows of weight 0 are ignored, whatever they hold
            live = w != 0
            G2, st2 = GO.step_reference(xt[live], d, T(y[live]), T(w[live]), T(off[live]), coef, s, init)
            np.testing.assert_allclose(G.numpy(), G2.numpy(), rtol=1e-11, atol=1e-11 * np.abs(wantG).max())
            np.testing.assert_allclose(st.numpy(), st2.numpy(), rtol=1e-11)
    # no weight and no offset: ones and zeros
    s = cases[0][0]
    G, st = GO.step_reference(xt, d, T(ycp), None, None, coef, s, False)
    wantG, wantst = _dense_step(x, ycp, np.ones(n), np.zeros(n), coef, 1.5, 0.0, False, False)
    np.testing.assert_allclose(G.numpy(), wantG, rtol=1e-11, atol=1e-11 * np.abs(wantG).max())
    np.testing.assert_allclose(st.numpy(), wantst, rtol=1e-11)
    eta, mu = GO.rows_reference(xt, d, T(off), coef, s)
    np.testing.assert_allclose(eta.numpy(), x @ coef[:d] + coef[d] + off, rtol=1e-13)
    live = w != 0
    np.testing.assert_allclose(mu.numpy()[live], np.exp(eta.numpy()[live]), rtol=1e-13)
