"""K32 (``_native/csrc/fm.hip``): the factorisation machine's loss, gradient and scores on bf16 rows against the
reference form on the same values (CPU f64), and the estimators on the kernel against their own reference form.

Op-level data: 4099 rows (the last 16-row group and the last tile are partial) of bf16 ``randn`` values, b = 0.3,
w ~ N(0, 1/d), V ~ N(0, 0.25/d), so that |s| stays a few units; labels ``randn`` for the squared loss and 0/1 for
the logistic loss. For d < dp the pad columns of the device rows hold bf16 NaN bits.

Bound per entry: |g - g_ref| <= 1e-10 M with, per row, T_f = sum_i |x_i||V_if|,
A = |b| + sum_i |x_i||w_i| + 1/2 (sum_f T_f^2 + sum_i x_i^2 sv_i), R = |r| + A, and
M(db) = sum_rows R, M(dw_i) = sum_rows |x_i| R, M(dV_if) = sum_rows |x_i| T_f R + |V_if| sum_rows x_i^2 R,
M(loss) = sum_rows (|l| + |r| A). The order of an n-term f64 sum costs at most n 2^-53 of the absolute terms, a
dp-term dot product dp 2^-53, taken twice through t_f^2: about 6e-13 M at n = 4099, dp = 512. 1e-10 leaves two
orders. Scores: |s - s_ref| <= 1e-10 A per row. Decisions: rows with |s_ref| <= 1e-9 A are the band that is left
out (at most 0.1 % of the rows); the sign of s agrees on all others.
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import fm as FM
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import fm_ops as FO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
N = 4099
SHAPES = [(3, 2), (10, 8), (17, 15), (40, 16), (100, 31), (256, 31), (512, 15)]
IDS = [f"{d}-{f}" for d, f in SHAPES]
LOSSES = ["squared", "logistic"]
_cache = {}


def _case(d, f):
    """bf16 rows (host and device, NaN bits in the pad columns), labels and parameters; made once per shape and
    shared, never modified."""
    if (d, f) in _cache:
        return _cache[(d, f)]
    rs = np.random.RandomState(1000 * d + f)
    xb = torch.as_tensor(rs.randn(N, d)).to(torch.float32).to(torch.bfloat16)
    y = {"squared": torch.as_tensor(rs.randn(N)), "logistic": torch.as_tensor((rs.rand(N) < 0.5).astype(np.float64))}
    p = torch.as_tensor(np.concatenate([[0.3], rs.randn(d) / np.sqrt(d), 0.5 * rs.randn(d * f) / np.sqrt(d)]))
    xd = to_device_matrix(xb.to(DEV), d).clone()
    dp = int(xd.shape[1])
    if d < dp:
        xd.view(torch.int16)[:, d:] = 0x7fc0
    out = dict(d=d, f=f, dp=dp, xb=xb, xd=xd, y=y, yd={k: v.to(DEV) for k, v in y.items()}, p=p)
    _cache[(d, f)] = out
    return out


def _terms(x, p, d, f):
    """Per row: the scores, t's absolute-term sums T [n, f] and A [n] (CPU f64)."""
    b, w, V = p[0], p[1:1 + d], p[1 + d:].reshape(d, f)
    ax = x.abs()
    T = ax @ V.abs()
    A = b.abs() + ax @ w.abs() + 0.5 * ((T * T).sum(1) + (x * x) @ (V * V).sum(1))
    return T, A


def _reference(C, loss, rows):
    """The reference form on the listed rows (a slice or an index tensor; CPU f64): the message and M per entry."""
    key = ("ref", loss, rows if isinstance(rows, int) else tuple(rows.tolist()))
    if key in C:
        return C[key]
    d, f, p = C["d"], C["f"], C["p"]
    sel = slice(0, rows) if isinstance(rows, int) else rows
    xb, y = C["xb"][sel], C["y"][loss][sel]
    want = FO.loss_grad_reference(xb, None, d, y, p, f, loss)
    x = xb.to(torch.float64)
    V = p[1 + d:].reshape(d, f)
    s = FO.scores_reference(xb, d, p, f)
    T, A = _terms(x, p, d, f)
    if loss == "logistic":
        r, l = torch.sigmoid(s) - y, torch.logaddexp(torch.zeros_like(s), s) - y * s
    else:
        r, l = s - y, 0.5 * (s - y) ** 2
    R = r.abs() + A
    ax = x.abs()
    MV = (ax * R[:, None]).T @ T + V.abs() * ((x * x) * R[:, None]).sum(0)[:, None]
    M = torch.cat([R.sum().reshape(1), (ax * R[:, None]).sum(0), MV.reshape(-1), (l.abs() + r.abs() * A).sum().reshape(1)])
    C[key] = (want.numpy(), M.numpy())
    return C[key]


def _check(got, want, M, what):
    g = got.cpu().numpy()
    assert got.dtype == torch.float64 and g.shape == want.shape and np.isfinite(g).all()
    ratio = np.abs(g - want) / M
    print(f"{what}: max |g - g_ref| / M = {ratio[:-1].max():.3e}, loss {ratio[-1]:.3e}, min M {M.min():.3e}")
    assert (np.abs(g - want) <= 1e-10 * M).all()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d,f", SHAPES, ids=IDS)
def test_loss_grad_against_reference(d, f, loss):
    C = _case(d, f)
    assert FO.kernel_supported(torch.bfloat16, C["dp"], f)
    for n in (N, 15, 1):
        want, M = _reference(C, loss, n)
        got = FO.loss_grad(C["xd"][:n], None, d, C["yd"][loss][:n], C["p"], f, loss)
        again = FO.loss_grad(C["xd"][:n], None, d, C["yd"][loss][:n], C["p"], f, loss)
        torch.cuda.synchronize()
        assert torch.equal(got, again)  # the same bits
        _check(got, want, M, f"d={d} f={f} {loss} n={n}")


@pytest.mark.parametrize("d,f", [s for s in SHAPES if s[0] not in (256, 512)], ids=IDS[:5])
def test_pad_columns_are_masked(d, f):
    """NaN bits in the pad columns change nothing: the same bits as zero padding."""
    C = _case(d, f)
    assert torch.isnan(C["xd"][:, d:].to(torch.float32)).all() and C["dp"] > d
    clean = to_device_matrix(C["xb"].to(DEV), d)
    for loss in LOSSES:
        a = FO.loss_grad(C["xd"], None, d, C["yd"][loss], C["p"], f, loss)
        b = FO.loss_grad(clean, None, d, C["yd"][loss], C["p"], f, loss)
        assert torch.equal(a, b) and torch.isfinite(a).all()
    sa = FO.scores(C["xd"], d, C["p"], f)
    sb = FO.scores(clean, d, C["p"], f)
    assert torch.equal(sa, sb) and torch.isfinite(sa).all()


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("d,f", SHAPES, ids=IDS)
def test_row_lists(d, f, loss):
    C = _case(d, f)
    xd, yd, p = C["xd"], C["yd"][loss], C["p"]
    third = torch.cat([torch.arange(0, N - 1, 3), torch.tensor([N - 1])])
    want, M = _reference(C, loss, third)
    _check(FO.loss_grad(xd, third.to(DEV), d, yd, p, f, loss), want, M, f"d={d} f={f} {loss} every third row")
    one = torch.tensor([N - 2])
    want, M = _reference(C, loss, one)
    _check(FO.loss_grad(xd, one, d, yd, p, f, loss), want, M, f"d={d} f={f} {loss} one listed row")
    every = FO.loss_grad(xd, torch.arange(N, device=DEV), d, yd, p, f, loss)
    assert torch.equal(every, FO.loss_grad(xd, None, d, yd, p, f, loss))
    empty = FO.loss_grad(xd, torch.zeros(0, dtype=torch.int64, device=DEV), d, yd, p, f, loss)
    torch.cuda.synchronize()
    assert empty.shape == (FO.size(d, f) + 1,) and not empty.any()


@pytest.mark.parametrize("d,f", SHAPES, ids=IDS)
def test_scores_against_reference(d, f):
    C = _case(d, f)
    xd, p = C["xd"], C["p"]
    want = FO.scores_reference(C["xb"], d, p, f).numpy()
    _, A = _terms(C["xb"].to(torch.float64), p, d, f)
    A = A.numpy()
    for n in (N, 15, 1):
        s = FO.scores(xd[:n], d, p, f)
        assert s.dtype == torch.float64 and s.shape == (n,)
        got = s.cpu().numpy()
        band = np.abs(want[:n]) <= 1e-9 * A[:n]
        print(f"d={d} f={f} n={n}: max |s - s_ref| / A = {(np.abs(got - want[:n]) / A[:n]).max():.3e}, rows in the "
              f"band {int(band.sum())}, min |s_ref| / A = {(np.abs(want[:n]) / A[:n]).min():.3e}")
        assert (np.abs(got - want[:n]) <= 1e-10 * A[:n]).all()
        assert band.mean() <= 0.001
        assert np.array_equal(got[~band] > 0, want[:n][~band] > 0)
    # the fit form's s where it is observable: the squared loss with y = 0 and one row has db = r = s
    s = FO.scores(xd, d, p, f)
    zeros = torch.zeros(N, dtype=torch.float64, device=DEV)
    for i in (0, 17, 2049, N - 1):
        alone = FO.loss_grad(xd[i:i + 1], None, d, zeros[:1], p, f, "squared")
        listed = FO.loss_grad(xd, torch.tensor([i], device=DEV), d, zeros, p, f, "squared")
        assert alone[0] == s[i] and listed[0] == s[i]
        assert FO.scores(xd[i:i + 1], d, p, f)[0] == s[i]


def test_edge_cases():
    C = _case(3, 2)
    xd, yd, p = C["xd"], C["yd"]["squared"], C["p"]
    g = FO.loss_grad(xd[:0], None, 3, yd[:0], p, 2, "squared")
    s = FO.scores(xd[:0], 3, p, 2)
    torch.cuda.synchronize()
    assert g.shape == (p.numel() + 1,) and not g.any() and s.shape == (0,)
    with pytest.raises(ValueError):
        FO.loss_grad(xd.to(torch.float32), None, 3, yd, p, 2, "squared")
    with pytest.raises(ValueError):
        FO.loss_grad(xd.T.contiguous().T, None, 3, yd, p, 2, "squared")
    with pytest.raises(ValueError):
        FO.loss_grad(xd, None, 3, yd, p[:-1], 2, "squared")
    with pytest.raises(ValueError):
        FO.scores(xd, 3, p[:-1], 2)
    with pytest.raises(ValueError):
        FO.loss_grad(xd, None, 3, yd, torch.zeros(FO.size(3, 32), dtype=torch.float64), 32, "squared")
    with pytest.raises(ValueError):
        FO.loss_grad(xd, torch.arange(5, dtype=torch.int32, device=DEV), 3, yd, p, 2, "squared")
    with pytest.raises(ValueError):
        FO.loss_grad(xd, None, 3, yd[:-1], p, 2, "squared")
    with pytest.raises(ValueError):
        FO.loss_grad(xd, None, 3, yd, p, 2, "hinge")
    wide = torch.zeros(64, 512, dtype=torch.bfloat16, device=DEV)  # dp = 512 with f = 16: 218 688 B of LDS
    assert not FO.kernel_supported(torch.bfloat16, 512, 16)
    with pytest.raises(ValueError):
        FO.scores(wide, 512, torch.zeros(FO.size(512, 16), dtype=torch.float64), 16)
    with pytest.raises(ValueError):
        FO.loss_grad(wide, None, 512, torch.zeros(64, dtype=torch.float64, device=DEV),
                     torch.zeros(FO.size(512, 16), dtype=torch.float64), 16, "logistic")


# ------------------------------------------------------------------------------------------------- estimator
@pytest.fixture(scope="module")
def spark():
    """A GPU session of this module's own, beside whichever session is active: a host session left active by
    another module would keep the frames on the CPU, where no kernel runs, and the modules that follow find the
    active session as they would without this one."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    s = SparkSession({"spark.master": "mi355x", "spark.app.name": "fm"})
    assert s.device.type == "cuda"
    yield s
    s.stop()


def _labelled(n, d, f=3, seed=0):
    """bf16 rows on the device and the labels of a planted factorisation machine with noise (f64): the response
    and the side of its interaction term's median."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=DEV).to(torch.bfloat16)
    xw = x.to(torch.float64)
    w = torch.randn(d, generator=g, device=DEV, dtype=torch.float64) / d ** 0.5
    V = 0.7 * torch.randn(d, f, generator=g, device=DEV, dtype=torch.float64) / d ** 0.5
    inter = 0.5 * (((xw @ V) ** 2) - (xw * xw) @ (V * V)).sum(1)
    y = 1.0 + xw @ w + inter + 0.05 * torch.randn(n, generator=g, device=DEV, dtype=torch.float64)
    return x, y, (inter > inter.median()).to(torch.float64)


def _flat(m):
    return np.concatenate([[m.intercept], m.linear.toArray(), m._V.reshape(-1)])


@pytest.mark.parametrize("frac", [1.0, 0.5])
@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_estimator_kernel_equals_reference(spark, monkeypatch, kind, frac):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import FMClassifier
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import FMRegressor
    x, yr, yc = _labelled(20_000, 12)
    df = spark.createDataFrameFromTensors({"features": x, "label": yr if kind == "regressor" else yc})
    cls = FMRegressor if kind == "regressor" else FMClassifier
    est = cls(factorSize=4, maxIter=5, tol=0.0, stepSize=0.05, seed=3, miniBatchFraction=frac)
    calls = []
    real, real_ref = FO.loss_grad, FO.loss_grad_reference

    def counted(*a, **k):
        calls.append(a[1])
        return real(*a, **k)
    monkeypatch.setattr(FO, "loss_grad", counted)
    fast = est.fit(df)
    out_fast = fast.transform(df)
    assert len(calls) >= 5
    assert all(c is None for c in calls) if frac == 1.0 else all(0 < c.numel() < 20_000 for c in calls)
    del calls[:]
    monkeypatch.setenv("CML_FM_KERNEL", "0")
    slow = est.fit(df)
    out_slow = slow.transform(df)
    monkeypatch.setattr(FO, "loss_grad_reference", lambda *a, **k: real_ref(*a, chunk=1000, **k))
    slow2 = est.fit(df)
    assert not calls
    assert fast._iters == slow._iters == 5
    np.testing.assert_allclose(fast._hist, slow._hist, rtol=1e-9)
    pf, ps, ps2 = _flat(fast), _flat(slow), _flat(slow2)
    D = np.abs(ps - ps2).max()
    diff = np.abs(pf - ps).max()
    print(f"{kind} frac={frac}: reference chunk 8192 vs 1000 D = {D:.3e}, kernel vs reference {diff:.3e}, "
          f"max |p| = {np.abs(ps).max():.3e}")
    assert diff <= 100.0 * D + 1e-12 * np.abs(ps).max()
    # predictions: the kernel's scores of its own model within the scores' bound, decisions outside the band
    xb = x.cpu()
    _, A = _terms(xb.to(torch.float64), torch.as_tensor(pf), 12, 4)
    A = A.numpy()
    s_own = FO.scores_reference(xb, 12, torch.as_tensor(pf), 4).numpy()
    s_ref = FO.scores_reference(xb, 12, torch.as_tensor(ps), 4).numpy()
    if kind == "regressor":
        got = out_fast._column_data("prediction").values.cpu().numpy()
        assert (np.abs(got - s_own) <= 1e-10 * A).all()
        assert (np.abs(out_slow._column_data("prediction").values.cpu().numpy() - s_ref) <= 1e-10 * A).all()
    else:
        raw = out_fast._column_data("rawPrediction").values.cpu().numpy()
        assert (np.abs(raw[:, 1] - s_own) <= 1e-10 * A).all() and np.array_equal(raw[:, 0], -raw[:, 1])
        band = np.abs(s_ref) <= 1e-9 * A
        lf = out_fast._column_data("prediction").values.cpu().numpy()
        ls = out_slow._column_data("prediction").values.cpu().numpy()
        print(f"rows in the band {int(band.sum())}, min |s_ref| / A = {(np.abs(s_ref) / A).min():.3e}")
        assert band.mean() <= 0.001 and np.array_equal(lf[~band], ls[~band])
        assert len(np.unique(ls)) == 2
        prob = out_fast._column_data("probability").values.cpu().numpy()
        np.testing.assert_allclose(prob.sum(1), 1.0, rtol=1e-15)


def test_other_columns_take_the_other_forms(spark, monkeypatch):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import FMClassifier
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import FMRegressor

    def boom(*a, **k):
        raise AssertionError("outside the kernel's limits: another form is expected")
    monkeypatch.setattr(FO, "loss_grad", boom)
    monkeypatch.setattr(FO, "scores", boom)
    x12, yr12, yc12 = _labelled(2000, 12)
    x256, yr256, _ = _labelled(2000, 256)
    for feats, y, f, cls in ((x12, yc12, 40, FMClassifier),
                             (x256.cpu().to(torch.float32).to(torch.float8_e4m3fn), yr256, 8, FMRegressor)):
        df = spark.createDataFrameFromTensors({"features": feats, "label": y})
        m = cls(factorSize=f, seed=3, maxIter=3, miniBatchFraction=0.7).fit(df)
        assert np.isfinite(_flat(m)).all() and np.isfinite(m._hist).all() and m._V.shape[1] == f
        pred = m.transform(df)._column_data("prediction").values
        assert pred.shape == (2000,) and torch.isfinite(pred).all()
    for name in ("loss_grad_reference", "scores_reference", "kernel_enabled", "kernel_supported", "lds_bytes"):
        monkeypatch.setattr(FO, name, boom)
    df = spark.createDataFrameFromTensors({"features": x12.to(torch.float32), "label": yr12})  # f32: the dense form
    m = FMRegressor(factorSize=4, seed=3, maxIter=3).fit(df)
    assert m.transform(df)._column_data("prediction").values.shape == (2000,)


@pytest.mark.parametrize("kind", ["regressor", "classifier"])
def test_fit_and_transform_memory(spark, kind):
    """Peak allocation during fit stays below half of X: the per-workgroup partials and the parameter images; no
    f64 copy, no x * x, no n x f activations. During transform it stays below the outputs plus a quarter of X: the
    f64 scores, and for the classifier the probability and rawPrediction columns."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import FMClassifier
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import FMRegressor
    n = 2_000_000
    x, yr, yc = _labelled(n, 32)
    df = spark.createDataFrameFromTensors({"features": x, "label": yr if kind == "regressor" else yc})
    del yr, yc
    est = (FMRegressor if kind == "regressor" else FMClassifier)(factorSize=8, seed=3, maxIter=3)
    xbytes = x.numel() * x.element_size()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = est.fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"{kind}: fit peak rise {rise / n:.1f} B/row = {100.0 * rise / xbytes:.1f} % of X")
    assert rise < 0.5 * xbytes
    assert m._V.shape == (32, 8) and m._iters == 3
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m.transform(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    outputs = 8 * n if kind == "regressor" else 8 * n + 2 * 16 * n
    print(f"{kind}: transform peak rise {rise / n:.1f} B/row, outputs {outputs / n:.0f} B/row, X {xbytes / n:.0f} B/row")
    assert rise < outputs + 0.25 * xbytes
    assert out._column_data("prediction").values.shape == (n,)
