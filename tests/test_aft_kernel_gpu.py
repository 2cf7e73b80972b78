"""K35 (``_native/csrc/aft.hip``): the fused AFT loss-gradient pass over bf16 rows of padded width 16 .. 512 against
the reference form (CPU f64, ``ops/aft_ops.py``), never against itself, and the routing of AFTSurvivalRegression.

Op-level data: 4099 rows (the last 64-row tile is partial, several slabs) of bf16 ``randn`` values in the
``to_device_matrix`` layout with bf16 NaN bits (0x7fc0) in the pad columns and 70 NaN rows behind the view;
``beta = 0.3 randn / sqrt(d)``, ``logt = x . beta + 0.7 log(Exp(1))``, 30 % of the rows censored with t scaled by
U(0.3, 1); evaluated at a perturbed ``coef`` with ``b = 0.8``, ``sigma = 0.9``, where -20 < eps < 5 (asserted).

Bounds (``u = 2^-53``):
(a) eta of the rows form: ``|eta_k - eta_ref| <= 2 (d + 2) u (sum_i |x_i beta_i| + |b|)``.
(b) r, s, l of the rows form against ``row_terms`` in torch on the CPU at the kernel's own eta, in units of
    ``u scale`` with ``scale_r = (delta + ee) / sigma``, ``scale_s = delta + (delta + ee) |eps|``,
    ``scale_l = delta |ls| + delta |eps| + ee``. D is the same quantity between torch on the GPU and torch on the CPU
    (two ``exp`` libraries on identical input); the kernel must stay within ``max(4 D, 16)`` units: a handful of
    roundings and one library call.
    Measured maxima on an MI355X over all widths and row counts (units; kernel / D):
      r 3.42 / 3.42, s 3.11 / 3.11, l 1.97 / 1.97 (the bits of torch on the GPU everywhere)
(c) gradient of the fit form: with r_k read from the rows form, ``|g - X^T r_k|[i] <= 2 (n + 2) u (|X|^T |r_k|)[i]``;
    entries whose bound is 0 are exactly 0.
(d) ``sum r, sum s, sum l``: within ``(2 (n + 2) + 64) u`` of the CPU sums of the rows form's vectors, scaled by the
    sums of their absolute values.
(e) two calls give the same bits, a row-offset view works, NaN in the pad columns and in the rows behind the view
    changes nothing, ``n = 0`` gives zeros, the eta-only mode of the rows form equals its with-terms eta bit for bit,
    ``cml_aft_lds(dp) == lds_bytes(dp)``.

Estimator: the gap D between the GPU reference form and a CPU frame over the same values is the spread of the
arithmetic before K35; the kernel may be 10 D from the CPU frame (the convention of ``test_gram_kernel_gpu.py``).
Measured on an MI355X (D, then the kernel's gap): model 3.5e-17 / 3.5e-17, prediction 3.6e-15 / 3.6e-15, quantiles
7.1e-15 / 7.1e-15; the f32 frame's model is within 2.9e-15 relative of the bf16 frame's; the fit's peak rise 0.065 x X.
Memory: a fit of 2M x 64 bf16 holds at most four f64 n-vectors (t, delta, logt, a temporary: 0.25 x the bytes of X)
and the partials, so its peak rise stays below 0.5 x; the dense form's is at least 4 x.
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd import _native
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import AFTSurvivalRegression
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import aft_ops as AO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
N = 4099
TAIL = 70  # rows behind the view, NaN
WIDTHS = [1, 15, 16, 17, 40, 100, 128, 300, 512]
ROWS = [N, 64, 63, 1]
BIG_N = 70_001  # more 64-row tiles than a launch has workgroups
U = 2.0 ** -53
_cache = {}
_worst = {}


def host_case(d, N=N):
    """The host side of a width's data; made once and shared, never modified."""
    rs = np.random.RandomState(2000 + d + (N - 4099))  # one seed per width and row count
    xb = torch.as_tensor(rs.randn(N, d)).to(torch.float32).to(torch.bfloat16)
    beta = 0.3 * rs.randn(d) / np.sqrt(d)
    t = np.exp(xb.to(torch.float64).numpy() @ beta + 0.7 * np.log(rs.exponential(1.0, N)))
    cens = rs.rand(N) < 0.3
    t = np.where(cens, t * rs.uniform(0.3, 1.0, N), t)
    coef = np.r_[beta + 0.05 * rs.randn(d) / np.sqrt(d), 0.8, np.log(0.9)]
    return dict(d=d, xb=xb, logt=torch.as_tensor(np.log(t)), delta=torch.as_tensor((~cens).astype(np.float64)),
                coef=torch.as_tensor(coef))


def _case(d, N=N):
    if (d, N) in _cache:
        return _cache[(d, N)]
    C = host_case(d, N)
    clean = to_device_matrix(C["xb"].to(DEV), d)
    dp = int(clean.shape[1])
    big = torch.full((N + TAIL, dp), float("nan"), dtype=torch.bfloat16, device=DEV)
    big[:N] = clean
    if d < dp:
        big.view(torch.int16)[:, d:] = 0x7fc0
    C.update(dp=dp, xd=big[:N], logtd=C["logt"].to(DEV), deltad=C["delta"].to(DEV))
    _cache[(d, N)] = C
    return C


def _units(got, want, scale):
    return float(((got - want).abs() / (U * scale).clamp(min=1e-300)).max()) if got.numel() else 0.0


def _check(C, n, xd=None, lo=0):
    """One evaluation on rows lo .. lo + n of the case: bounds (a) to (e)."""
    d, coef = C["d"], C["coef"]
    sl = slice(lo, lo + n)
    xd = C["xd"][sl] if xd is None else xd
    xb, logt, delta = C["xb"][sl], C["logt"][sl], C["delta"][sl]
    logtd, deltad = C["logtd"][sl], C["deltad"][sl]
    ls = float(coef[d + 1])
    out = AO.loss_grad(xd, d, logtd, deltad, coef)
    out2 = AO.loss_grad(xd, d, logtd, deltad, coef)
    ek, rk, sk, lk = (v.cpu() for v in AO.rows(xd, d, coef, logtd, deltad))
    e2 = AO.rows(xd, d, coef).cpu()
    torch.cuda.synchronize()
    assert out.shape == (d + 3,) and out.dtype == torch.float64 and torch.isfinite(out).all()
    assert torch.equal(out, out2) and torch.equal(ek, e2) and ek.shape == (n,)                 # (e)
    x64 = xb.to(torch.float64)
    eta_ref = AO.rows_reference(xb, d, coef)                                                   # (a)
    bound = 2.0 * (d + 2) * U * ((x64.abs() @ coef[:d].abs()) + coef[d].abs())
    assert ((ek - eta_ref).abs() <= bound).all()
    # (b): the row terms at the kernel's own eta, torch CPU against the kernel and against torch on the GPU
    cpu = AO.row_terms(ek, logt, delta, ls)
    gpu = {k: v.cpu() for k, v in AO.row_terms(ek.to(DEV), logtd, deltad, ls).items()}
    eps, ee, sigma = cpu["eps"], cpu["ee"], float(np.exp(ls))
    assert float(eps.min()) > -20.0 and float(eps.max()) < 5.0
    scales = {"r": (delta + ee) / sigma, "s": delta + (delta + ee) * eps.abs(),
              "l": delta * abs(ls) + delta * eps.abs() + ee}
    for k, got in (("r", rk), ("s", sk), ("l", lk)):
        mine, D = _units(got, cpu[k], scales[k]), _units(gpu[k], cpu[k], scales[k])
        _worst[k] = max(_worst.get(k, (0.0, 0.0)), (mine, D))
        assert mine <= max(4.0 * D, 16.0), (k, d, n, mine, D)
    # (c)
    g = out[:d].cpu()
    want = x64.T @ rk
    M = x64.abs().T @ rk.abs()
    assert (g[M == 0] == 0).all()
    assert ((g - want).abs() <= 2.0 * (n + 2) * U * M).all(), (d, n)
    # (d)
    ref = torch.stack([rk.sum(), sk.sum(), lk.sum()])
    sb = (2.0 * (n + 2) + 64.0) * U * torch.stack([rk.abs().sum(), sk.abs().sum(), lk.abs().sum()])
    assert ((out[d:].cpu() - ref).abs() <= sb).all(), (d, n, out[d:].cpu(), ref, sb)
    return out


@pytest.mark.parametrize("d", WIDTHS)
def test_pass_against_reference(d):
    C = _case(d)
    assert AO.kernel_supported(torch.bfloat16, C["dp"])
    for n in ROWS:
        _check(C, n)
    print(f"(b) up to d = {d}: " + ", ".join(f"{k} {m:.2f} / {D:.2f}" for k, (m, D) in sorted(_worst.items())))


@pytest.mark.parametrize("d", [40, 300])
def test_several_tiles_per_workgroup(d):
    """70 001 rows are 1094 tiles: more than a launch has workgroups at d = 300 (two per CU) and a little more than
    it has at d = 40 (four per CU), so workgroups run their tile loop (the loads one tile ahead, the barriers)
    several times; at 4099 rows each has one tile."""
    _check(_case(d, BIG_N), BIG_N)


@pytest.mark.parametrize("d", [17, 100, 512])
def test_views_pad_columns_and_rows_behind_the_view(d):
    """A row-offset view works; NaN bits in the pad columns and NaN rows behind the view change nothing: the same
    bits as a clean buffer of exactly n rows."""
    C = _case(d)
    _check(C, N - 3, xd=C["xd"][3:], lo=3)
    _check(C, 63, xd=C["xd"][5:68], lo=5)
    clean = to_device_matrix(C["xb"].to(DEV), d)
    assert d == C["dp"] or torch.isnan(C["xd"][:, d:].to(torch.float32)).all()
    a = AO.loss_grad(C["xd"], d, C["logtd"], C["deltad"], C["coef"])
    b = AO.loss_grad(clean, d, C["logtd"], C["deltad"], C["coef"])
    assert torch.equal(a, b)
    for u, v in zip(AO.rows(C["xd"], d, C["coef"], C["logtd"], C["deltad"]),
                    AO.rows(clean, d, C["coef"], C["logtd"], C["deltad"])):
        assert torch.equal(u, v)


def test_empty_errors_and_lds():
    C = _case(17)
    d, xd, logt, delta, coef = 17, C["xd"], C["logtd"], C["deltad"], C["coef"]
    e = AO.loss_grad(xd[:0], d, logt[:0], delta[:0], coef)
    assert e.shape == (d + 3,) and e.is_cuda and not e.any()
    assert AO.rows(xd[:0], d, coef).shape == (0,)
    assert all(v.shape == (0,) for v in AO.rows(xd[:0], d, coef, logt[:0], delta[:0]))
    with pytest.raises(ValueError):
        AO.loss_grad(xd.to(torch.float32), d, logt, delta, coef)
    with pytest.raises(ValueError):
        AO.loss_grad(xd, d, logt[:-1], delta, coef)
    with pytest.raises(ValueError):
        AO.loss_grad(xd, d, logt, delta, coef[:-1])
    with pytest.raises(ValueError):
        AO.loss_grad(C["xb"], d, C["logt"], C["delta"], coef)  # host rows
    with pytest.raises(ValueError):
        AO.rows(xd, d, coef, logt=logt)
    lib = _native.kernels()
    for dp in (16, 32, 64, 128, 256, 512):
        assert int(lib.cml_aft_lds(dp)) == AO.lds_bytes(dp)
    assert int(lib.cml_aft_lds(48)) == 0 and int(lib.cml_aft_lds(1024)) == 0


# ------------------------------------------------------------------------------------------------ estimator
@pytest.fixture(scope="module")
def sessions():
    """A GPU session and a host session of this module's own, beside whichever session is active."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    gpu = SparkSession({"spark.master": "mi355x", "spark.app.name": "aft"})
    assert gpu.device.type == "cuda"
    host = SparkSession({"spark.master": "local", "spark.app.name": "aft-host"})
    assert host.device.type == "cpu"
    yield gpu, host
    host.stop()
    gpu.stop()


def _counted(monkeypatch):
    calls = {}
    for name in ("loss_grad", "loss_grad_reference", "rows", "rows_reference"):
        def wrap(*a, _f=getattr(AO, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(AO, name, wrap)
    return calls


def _table(n=3000, d=40):
    """bf16 rows, a Weibull duration whose log is linear in them, 30 % censored."""
    rs = np.random.RandomState(17)
    xb = torch.as_tensor(rs.randn(n, d)).to(torch.float32).to(torch.bfloat16)
    beta = 0.3 * rs.randn(d) / np.sqrt(d)
    t = np.exp(xb.to(torch.float64).numpy() @ beta + 1.0 + 0.7 * np.log(rs.exponential(1.0, n)))
    cens = rs.rand(n) < 0.3
    t = np.where(cens, t * rs.uniform(0.3, 1.0, n), t)
    return xb, torch.as_tensor(t), torch.as_tensor((~cens).astype(np.float64))


def _fit(df):
    m = AFTSurvivalRegression(maxIter=30, quantileProbabilities=[0.1, 0.5, 0.9], quantilesCol="q").fit(df)
    out = m.transform(df)
    return np.r_[m.coefficients.toArray(), m.intercept, m.scale], \
        out._column_data("prediction").values.cpu().numpy(), out._column_data("q").values.cpu().numpy()


def test_estimator_kernel_reference_and_host(sessions, monkeypatch):
    gpu, host = sessions
    xb, t, c = _table()
    dfg = gpu.createDataFrameFromTensors({"features": xb.to(DEV), "label": t.to(DEV), "censor": c.to(DEV)})
    dfh = host.createDataFrameFromTensors({"features": xb.to(torch.float64), "label": t, "censor": c})
    assert dfg._feature_matrix("features").dtype == torch.bfloat16 and not dfh._feature_matrix("features").is_cuda
    monkeypatch.delenv("CML_AFT_KERNEL", raising=False)
    calls = _counted(monkeypatch)
    fast = _fit(dfg)
    assert set(calls) == {"loss_grad", "rows"} and calls["loss_grad"] > 5 and calls["rows"] == 1
    evals = calls["loss_grad"]
    calls.clear()
    monkeypatch.setenv("CML_AFT_KERNEL", "0")
    slow = _fit(dfg)
    assert calls == {"loss_grad_reference": evals, "rows_reference": 1}
    calls.clear()
    cpu = _fit(dfh)
    assert not calls                                                       # a host frame keeps the dense form
    for what, a, b, c_ in zip(("model", "prediction", "quantiles"), fast, slow, cpu):
        D, gap = np.abs(b - c_).max(), np.abs(a - c_).max()
        print(f"{what}: reference form vs host frame D = {D:.3e}, kernel vs host frame {gap:.3e}, "
              f"max |value| = {np.abs(c_).max():.3e}")
        assert np.isfinite(a).all() and gap <= 10.0 * D


def test_estimator_routes(sessions, monkeypatch):
    gpu, _ = sessions
    monkeypatch.delenv("CML_AFT_KERNEL", raising=False)
    calls = _counted(monkeypatch)
    xb, t, c = _table()
    model = _fit(gpu.createDataFrameFromTensors({"features": xb.to(DEV), "label": t.to(DEV), "censor": c.to(DEV)}))[0]
    calls.clear()
    # e4m3 rows take the reference form
    df8 = gpu.createDataFrameFromTensors({"features": xb.to(torch.float8_e4m3fn).to(DEV), "label": t.to(DEV),
                                          "censor": c.to(DEV)})
    assert df8._feature_matrix("features").dtype == torch.float8_e4m3fn
    assert np.isfinite(_fit(df8)[0]).all()
    assert set(calls) == {"loss_grad_reference", "rows_reference"} and calls["rows_reference"] == 1
    calls.clear()
    # an f32 frame keeps the dense form, and gives the bf16 frame's model (the same values)
    df32 = gpu.createDataFrameFromTensors({"features": xb.to(torch.float32).to(DEV), "label": t.to(DEV),
                                           "censor": c.to(DEV)})
    m32 = _fit(df32)[0]
    assert not calls
    print(f"f32 frame vs bf16 frame: max rel diff {np.abs((m32 - model) / model).max():.3e}")
    np.testing.assert_allclose(m32, model, rtol=1e-8)
    # the label and censor checks stand before either form
    with pytest.raises(ValueError, match="must be positive"):
        AFTSurvivalRegression().fit(gpu.createDataFrameFromTensors(
            {"features": xb.to(DEV), "label": (-t).to(DEV), "censor": c.to(DEV)}))
    with pytest.raises(ValueError, match="0 or 1"):
        AFTSurvivalRegression().fit(gpu.createDataFrameFromTensors(
            {"features": xb.to(DEV), "label": t.to(DEV), "censor": (2.0 * c).to(DEV)}))


def test_fit_memory(sessions, monkeypatch):
    """2M x 64 bf16: the kernel path allocates the f64 n-vectors logt and a temporary of the label checks, the
    per-workgroup partials and nothing of size n x d; the dense form's rise is more than 4 x the bytes of X."""
    gpu, _ = sessions
    monkeypatch.delenv("CML_AFT_KERNEL", raising=False)
    n, d = 2_000_000, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32).to(torch.bfloat16)
    t = torch.exp(0.5 * torch.randn(n, device=DEV, generator=g, dtype=torch.float64))
    c = (torch.rand(n, device=DEV, generator=g) < 0.7).to(torch.float64)
    df = gpu.createDataFrameFromTensors({"features": x, "label": t, "censor": c})
    assert df._feature_matrix("features").dtype == torch.bfloat16
    xbytes = n * d * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = AFTSurvivalRegression(maxIter=5).fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"fit of 2M x 64 bf16: peak rise {rise / 2 ** 20:.1f} MiB = {rise / xbytes:.3f} x X")
    assert m.numFeatures == d and rise < 0.5 * xbytes
