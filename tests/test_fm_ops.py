"""``ops/fm_ops.py``: the chunked reference form of the factorisation machine's loss, gradient and scores against
autograd over the estimator's dense expression, row lists, the limits of K32, and the estimator on the reference
form."""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import fm as FM
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import fm_ops as FO

N = 4099
SHAPES = [(3, 2), (17, 15), (40, 31)]
LOSSES = ["squared", "logistic"]
_cache = {}


def _case(d, f):
    """Rows, labels for both losses and parameters with |s| of a few units; made once per shape, never modified."""
    if (d, f) in _cache:
        return _cache[(d, f)]
    rs = np.random.RandomState(100 * d + f)
    x = torch.as_tensor(rs.randn(N, d))
    y = {"squared": torch.as_tensor(rs.randn(N)), "logistic": torch.as_tensor((rs.rand(N) < 0.5).astype(np.float64))}
    p = torch.as_tensor(np.concatenate([[0.3], rs.randn(d) / np.sqrt(d), 0.5 * rs.randn(d * f) / np.sqrt(d)]))
    _cache[(d, f)] = (x, y, p)
    return _cache[(d, f)]


def _autograd(x, y, p, d, f, loss):
    """The estimator's dense expression: ``[grad | loss]``."""
    pt = p.clone().requires_grad_(True)
    s = FM._fm_scores(x, pt[0], pt[1:1 + d], pt[1 + d:].reshape(d, f))
    if loss == "logistic":
        total = (torch.logaddexp(torch.zeros_like(s), s) - y * s).sum()
    else:
        total = 0.5 * ((s - y) ** 2).sum()
    g, = torch.autograd.grad(total, pt)
    return torch.cat([g, total.detach().reshape(1)]).numpy()


def _bound(x, y, p, d, f, loss):
    """M per message entry: the sum of the absolute terms (the kernel test's bound)."""
    b, w, V = p[0], p[1:1 + d], p[1 + d:].reshape(d, f)
    s = FM._fm_scores(x, b, w, V)
    ax = x.abs()
    Tf = ax @ V.abs()
    A = b.abs() + ax @ w.abs() + 0.5 * ((Tf * Tf).sum(1) + (x * x) @ (V * V).sum(1))
    if loss == "logistic":
        r, l = torch.sigmoid(s) - y, torch.logaddexp(torch.zeros_like(s), s) - y * s
    else:
        r, l = s - y, 0.5 * (s - y) ** 2
    R = r.abs() + A
    MV = (ax * R[:, None]).T @ Tf + V.abs() * ((x * x) * R[:, None]).sum(0)[:, None]
    return torch.cat([R.sum().reshape(1), (ax * R[:, None]).sum(0), MV.reshape(-1),
                      (l.abs() + r.abs() * A).sum().reshape(1)]).numpy()


def _close(got, want):
    """rtol 1e-10 on the entries that are not a cancellation to near zero."""
    big = np.abs(want) > 1e-6 * np.abs(want[:-1]).max()
    big[-1] = True
    np.testing.assert_allclose(got[big], want[big], rtol=1e-10)
    assert np.abs(got - want)[~big].max(initial=0.0) <= 1e-10 * np.abs(want[:-1]).max()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d,f", SHAPES)
def test_reference_equals_autograd(d, f, loss):
    x, y, p = _case(d, f)
    got = FO.loss_grad_reference(x, None, d, y[loss], p, f, loss)
    assert got.dtype == torch.float64 and got.shape == (FO.size(d, f) + 1,)
    _close(got.numpy(), _autograd(x, y[loss], p, d, f, loss))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d,f", SHAPES)
def test_low_precision_rows_are_widened_exactly(d, f, loss, dtype):
    x, y, p = _case(d, f)
    xl = x.to(torch.float32).to(dtype)
    xl = torch.cat([xl, torch.zeros(N, 5).to(dtype)], 1)  # wider than d: the columns past d are not read
    wide = xl[:, :d].to(torch.float32).to(torch.float64)
    got = FO.loss_grad_reference(xl, None, d, y[loss], p, f, loss, chunk=1000)
    _close(got.numpy(), _autograd(wide, y[loss], p, d, f, loss))
    s = FO.scores_reference(xl, d, p, f, 1000)
    want = FM._fm_scores(wide, p[0], p[1:1 + d], p[1 + d:].reshape(d, f))
    np.testing.assert_allclose(s.numpy(), want.numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d,f", SHAPES)
def test_chunk_invariance(d, f, loss):
    x, y, p = _case(d, f)
    M = _bound(x, y[loss], p, d, f, loss)
    whole = FO.loss_grad_reference(x, None, d, y[loss], p, f, loss, chunk=8192).numpy()
    for chunk in (1000, 1):
        got = FO.loss_grad_reference(x, None, d, y[loss], p, f, loss, chunk=chunk).numpy()
        assert (np.abs(got - whole) <= 1e-11 * M).all()


@pytest.mark.parametrize("loss", LOSSES)
def test_row_lists(loss):
    d, f = 17, 15
    x, y, p = _case(d, f)
    xb = x.to(torch.float32).to(torch.bfloat16)
    third = torch.cat([torch.arange(0, N - 1, 3), torch.tensor([N - 1])])
    for rows in (third, torch.tensor([1234]), torch.arange(N)):
        got = FO.loss_grad_reference(xb, rows, d, y[loss], p, f, loss, chunk=1000)
        want = FO.loss_grad_reference(xb[rows], None, d, y[loss][rows], p, f, loss, chunk=1000)
        assert torch.equal(got, want)
    e4 = x.to(torch.float32).to(torch.float8_e4m3fn)
    got = FO.loss_grad_reference(e4, third, d, y[loss], p, f, loss)
    want = FO.loss_grad_reference(e4.to(torch.float32)[third], None, d, y[loss][third], p, f, loss)
    assert torch.equal(got, want)
    empty = FO.loss_grad_reference(xb, torch.zeros(0, dtype=torch.int64), d, y[loss], p, f, loss)
    assert empty.shape == (FO.size(d, f) + 1,) and not empty.any()
    none = FO.loss_grad_reference(xb[:0], None, d, y[loss][:0], p, f, loss)
    assert none.shape == (FO.size(d, f) + 1,) and not none.any()


@pytest.mark.parametrize("d,f", SHAPES)
def test_scores_reference(d, f):
    x, _, p = _case(d, f)
    want = FM._fm_scores(x, p[0], p[1:1 + d], p[1 + d:].reshape(d, f))
    for chunk in (1000, 8192):
        s = FO.scores_reference(x, d, p, f, chunk)
        assert s.dtype == torch.float64 and s.shape == (N,)
        np.testing.assert_allclose(s.numpy(), want.numpy(), rtol=1e-10, atol=1e-12)
    assert FO.scores_reference(x[:0], d, p, f).shape == (0,)


def test_logistic_loss_does_not_overflow():
    """|s| about 700: softplus and sigmoid through exp(-|s|)."""
    x = torch.tensor([[700.0], [-700.0]], dtype=torch.float64)
    y = torch.tensor([0.0, 1.0], dtype=torch.float64)
    p = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    out = FO.loss_grad_reference(x, None, 1, y, p, 1, "logistic")
    assert torch.isfinite(out).all()
    np.testing.assert_allclose(out[-1].item(), 1400.0, rtol=1e-15)
    np.testing.assert_allclose(out[0].item(), 0.0, atol=1e-300)


def test_argument_checks():
    x, y, p = _case(3, 2)
    with pytest.raises(ValueError):
        FO.loss_grad_reference(x, None, 3, y["squared"], p[:-1], 2, "squared")
    with pytest.raises(ValueError):
        FO.loss_grad_reference(x, None, 3, y["squared"][:-1], p, 2, "squared")
    with pytest.raises(ValueError):
        FO.loss_grad_reference(x, None, 3, y["squared"], p, 2, "hinge")
    with pytest.raises(ValueError):
        FO.loss_grad_reference(x, torch.arange(5, dtype=torch.int32), 3, y["squared"], p, 2, "squared")
    with pytest.raises(ValueError):
        FO.scores_reference(x, 4, p, 2)
    # the kernel wrappers take device rows only
    xb = torch.zeros(64, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        FO.loss_grad(xb, None, 3, torch.zeros(64, dtype=torch.float64), p, 2, "squared")
    with pytest.raises(ValueError):
        FO.scores(xb, 3, p, 2)


def test_kernel_enabled(monkeypatch):
    monkeypatch.delenv("CML_FM_KERNEL", raising=False)
    assert FO.kernel_enabled()
    monkeypatch.setenv("CML_FM_KERNEL", "0")
    assert not FO.kernel_enabled()


def test_kernel_supported():
    bf = torch.bfloat16
    for dp in (16, 32, 64, 128, 256, 512):
        for f in (1, 15, 16, 31, 32):
            hp = 16 if f <= 15 else 32
            dpt = max(dp, 64)
            formula = 8 * (hp * dpt + dpt + 66 * hp + 8) + 128 * (dpt + 8)  # the docstring of lds_bytes
            inside = f <= 31 and formula <= 160 * 1024
            assert FO.kernel_supported(bf, dp, f) == inside, (dp, f)
            assert FO.lds_bytes(dp, f) == (formula if inside else 0), (dp, f)
            assert inside == (f <= (15 if dp == 512 else 31))
            assert not FO.kernel_supported(torch.float32, dp, f)
            assert not FO.kernel_supported(torch.float8_e4m3fn, dp, f)
    assert FO.lds_bytes(256, 31) == 118336 and FO.lds_bytes(512, 15) == 144704
    for dp, f in ((8, 4), (1024, 4), (48, 4), (64, 0)):
        assert not FO.kernel_supported(bf, dp, f)
    assert FO.size(10, 8) == 91


# ------------------------------------------------------------------------------------------------- estimator
def _planted(n=600, d=4, f=2):
    rs = np.random.RandomState(5)
    X = torch.as_tensor(rs.normal(size=(n, d))).to(torch.float32).to(torch.bfloat16)
    Xw = X.to(torch.float64).numpy()
    V = rs.normal(scale=0.7, size=(d, f))
    w = np.array([0.5, -0.3, 0.0, 0.2])
    y = 1.0 + Xw @ w + 0.5 * (((Xw @ V) ** 2) - (Xw ** 2) @ (V ** 2)).sum(1) + 0.05 * rs.normal(size=n)
    return X, Xw, y


def test_estimator_on_the_reference_form(monkeypatch):
    """A CPU bf16 frame, routed as a bf16 device column is with the kernel off. The host session is this test's
    own, beside whichever session is active, and is stopped at the end: the modules that follow find the active
    session as they would without this one."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession({"spark.master": "local[2]", "spark.app.name": "fm_ops"})
    assert spark.device.type == "cpu"
    try:
        _estimator_on_the_reference_form(spark, monkeypatch)
    finally:
        spark.stop()


def _estimator_on_the_reference_form(spark, monkeypatch):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import FMRegressor
    X, Xw, y = _planted()
    calls = []
    real = FO.loss_grad_reference
    monkeypatch.setattr(FO, "loss_grad_reference", lambda *a, **k: (calls.append(a[1]), real(*a, **k))[1])
    monkeypatch.setattr(FO, "kernel_enabled", lambda: False)
    monkeypatch.setattr(FM, "_low_precision", lambda x: x.dtype in (torch.bfloat16, torch.float8_e4m3fn))
    monkeypatch.setattr(torch.autograd, "grad", lambda *a, **k: pytest.fail("the dense form ran"))
    df = spark.createDataFrameFromTensors({"features": X, "label": torch.as_tensor(y)})
    m = FMRegressor(factorSize=2, stepSize=0.05, maxIter=400, seed=3).fit(df)
    assert len(calls) == m._iters and all(c is None for c in calls)
    pred = m.transform(df)._column_data("prediction").values.numpy()
    assert np.mean((pred - y) ** 2) < 0.1 * np.var(y)
    W, Vm = m.linear.toArray(), m.factors.toArray()
    ref = m.intercept + Xw @ W + 0.5 * (((Xw @ Vm) ** 2) - (Xw ** 2) @ (Vm ** 2)).sum(1)
    np.testing.assert_allclose(pred, ref, rtol=1e-10, atol=1e-12)
    del calls[:]
    half = FMRegressor(factorSize=2, stepSize=0.05, maxIter=20, tol=0.0, seed=3, miniBatchFraction=0.5).fit(df)
    assert len(calls) == 20 and all(c is not None and 0 < c.numel() < len(y) for c in calls)
    assert np.isfinite(half.linear.toArray()).all() and np.isfinite(half.factors.toArray()).all()
    assert np.isfinite(half.intercept) and np.isfinite(half._hist).all()
