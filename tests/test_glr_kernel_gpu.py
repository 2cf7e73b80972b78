"""K33 (``_native/csrc/glr.hip``): the fused IRLS step of bf16 rows with 1 <= d <= 128 on the f64 MFMA against the
reference form (CPU f64, ``ops/glr_ops.py``), never against itself, and the routing of GeneralizedLinearRegression.

Op-level data: 4099 rows (the last 64-row tile is partial, several slabs) of bf16 ``randn`` values in the
``to_device_matrix`` layout with bf16 NaN bits (0x7fc0) in the pad columns and 70 NaN rows behind the view;
``w = rand`` with about 5 % exact zeros, five of the zero-weight rows with offset 1e4; ``off = U(-0.3, 0.3)``,
``beta = 0.3 randn / sqrt(d)``, ``b0 = 2``, so that eta lies in (0.25, 4) on the live rows (asserted) and every power
link stays inside its domain.

Bounds:
(a) eta: ``|eta_k - eta_ref| <= 2 (d + 3) 2^-53 (sum_i |x_i beta_i| + |b0| + |off|)``, a (d + 2)-term f64 sum on
    both sides.
(b) eta (init form), mu, z, wt of the rows form against ``row_terms`` in torch on the CPU at the kernel's own eta,
    in units of ``2^-53 scale`` with ``scale_mu = |mu|``, ``scale_wt = |wt|``,
    ``scale_z = |eta| + |off| + (|y| + |mu|) |g'(mu)|``. D is the same quantity between torch on the GPU and torch on
    the CPU (two math libraries on identical input); the kernel must stay within ``max(4 D, 16)`` units: at most six
    roundings and three library calls of at most 2 ulp each.
    Measured maxima on an MI355X over all widths and row counts (units; kernel / D; quantities not listed are 0 / 0,
    the same bits on all three):
      tweedie(1.5, log)          init eta 1.98 / 1.98, z 1.26 / 1.26, wt 4.37 / 4.37; coef mu 1.98 / 1.98,
                                 z 1.28 / 1.28, wt 5.67 / 5.67
      tweedie(1.5, default -0.5) init eta 2.72 / 2.18, z 3.37 / 1.88, wt 7.98 / 7.98; coef mu 2.84 / 0.00,
                                 z 5.59 / 2.73, wt 9.61 / 7.85 (the only spec on pow, where the kernel and torch on
                                 the GPU differ; all within the floor of 16)
      tweedie(0, identity)       all 0 / 0
      tweedie(1, log)            coef mu 1.98 / 1.98, z 1.26 / 1.26, wt 6.31 / 6.31
      tweedie(2, inverse)        all 0 / 0
      tweedie(3, 0.5)            init eta 1.99 / 1.99, z 1.74 / 1.74, wt 6.17 / 6.17
      binomial / logit           init eta 2.00 / 2.00, z 3.30 / 3.30; coef mu 2.70 / 2.70, z 24.99 / 24.99,
                                 wt 31.82 / 31.82 (above the floor, but the bits of torch on the GPU: 1 - mu loses
                                 digits as mu nears 1, in both libraries alike)
(c) G: with z_k, wt_k read from the rows form, ``|G - gram_reference(x, d, z_k, wt_k)|[i][j] <= 2 (n + 2) 2^-53
    M[i][j]``, ``M = |A|^T diag(|wt|) |A|`` (K31's bound); entries with ``M == 0`` are exactly 0; G is exactly
    symmetric.
(d) stats: each within ``(2 (n + 2) + 64) 2^-53`` times the sum over the rows of the absolute values of the leaf
    terms of its formula, evaluated on the CPU at the kernel's mu. Leaves: ``w y^a / a`` and ``w mu^a / a`` of every
    power difference (times ``|y|`` where the formula multiplies by y), ``|log q| + 1`` for a logarithm of a quotient
    (the quotient's rounding is an absolute error of 2^-53 in the log), ``(|y| + |mu|)^2`` for ``(y - mu)^2``: a
    row's addend made of k roundings is within ``k 2^-53`` of that sum, 64 covers k and the library calls, and the
    n-term sum adds ``(n + 2) 2^-53`` on each side.
(e) two calls give the same bits, a row-offset view and ``w = None`` / ``off = None`` work, the ``gram=False`` stats
    are the ``gram=True`` stats bit for bit.

Estimator: the gap D between the GPU reference form and a CPU frame over the same values is the spread of the
arithmetic before K33; the kernel may be 10 D from the CPU frame (the convention of ``test_gram_kernel_gpu.py``).
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import GeneralizedLinearRegression
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import glr_ops as GO
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import gram_ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
N = 4099
TAIL = 70  # rows behind the view, NaN
WIDTHS = [1, 15, 16, 17, 40, 100, 128]
ROWS = [N, 64, 63, 1]
BIG_N = 70_001  # more 64-row tiles than a launch has workgroups
U = 2.0 ** -53
SPECS = {  # name: (spec, label kind)
    "tweedie(1.5, log)": (GO.spec("tweedie", None, 1.5, 0.0), "cp"),
    "tweedie(1.5, default -0.5)": (GO.spec("tweedie", None, 1.5, None), "cp"),
    "tweedie(0, identity)": (GO.spec("tweedie", None, 0.0, 1.0), "real"),
    "tweedie(1, log)": (GO.spec("tweedie", None, 1.0, 0.0), "count"),
    "tweedie(2, inverse)": (GO.spec("tweedie", None, 2.0, -1.0), "pos"),
    "tweedie(3, 0.5)": (GO.spec("tweedie", None, 3.0, 0.5), "pos"),
    "binomial / logit": (GO.spec("binomial", "logit"), "bin"),
}
_cache = {}
_worst = {}


def host_case(d, N=N):
    """The host side of a width's data; made once and shared, never modified."""
    rs = np.random.RandomState(1000 + d + (N - 4099))  # one seed per width and row count
    xb = torch.as_tensor(rs.randn(N, d)).to(torch.float32).to(torch.bfloat16)
    w = torch.as_tensor(rs.rand(N))
    w[rs.rand(N) < 0.05] = 0.0
    off = torch.as_tensor(rs.uniform(-0.3, 0.3, N))
    dead = torch.nonzero(w == 0).reshape(-1)
    off[dead[1:6]] = 1e4
    coef = torch.as_tensor(np.r_[0.3 * rs.randn(d) / np.sqrt(d), 2.0])
    pos = rs.gamma(2.0, 1.0, N) + 1e-3
    y = {"pos": pos, "cp": np.where(rs.rand(N) < 0.2, 0.0, pos), "real": rs.randn(N) + 2.0,
         "count": rs.poisson(3.0, N).astype(np.float64), "bin": (rs.rand(N) < 0.6).astype(np.float64)}
    return dict(d=d, xb=xb, w=w, off=off, coef=coef, y={k: torch.as_tensor(v) for k, v in y.items()})


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
    C.update(dp=dp, xd=big[:N], wd=C["w"].to(DEV), offd=C["off"].to(DEV), yd={k: v.to(DEV) for k, v in C["y"].items()})
    _cache[(d, N)] = C
    return C


def _units(got, want, scale):
    return float(((got - want).abs() / (U * scale).clamp(min=1e-300)).max()) if got.numel() else 0.0


def _abs_addends(s, y, w, mu):
    """Per stat, the sum over the rows of the absolute leaf terms of its formula (bound (d) of the module)."""
    live = w != 0
    if s.var == 1:
        def lg(a, b):
            return torch.where(a > 0, a.abs() * (torch.log(a / b).abs() + 1.0), torch.zeros_like(a))
        dev = 2.0 * (lg(y, mu) + lg(1.0 - y, 1.0 - mu))
        V = mu * (1.0 - mu)
    else:
        def yp(a, e):
            if e == 0.0:
                return torch.where(a > 0, torch.log(a / mu).abs() + 1.0, torch.zeros_like(a))
            return (a.abs() ** e + mu.abs() ** e) / abs(e)
        y1 = y.clamp(min=0.1) if 1.0 <= s.p < 2.0 else y
        first = yp(y1, 1.0 - s.p)
        dev = 2.0 * (torch.where(y != 0, y.abs() * first, torch.zeros_like(y)) + yp(y, 2.0 - s.p))
        V = mu ** s.p
    z = torch.zeros_like(y)
    rows = [w * dev, w * (y.abs() + mu.abs()) ** 2 / V, (w * y).abs(), w.abs()]
    return torch.stack([torch.where(live, r, z).sum() for r in rows[:3]] + [rows[3].sum()])


def _check(C, name, n, init, xd=None, lo=0, weighted=True, offset=True):
    """One step on rows lo .. lo + n of the case: bounds (a) to (e)."""
    s, kind = SPECS[name]
    d = C["d"]
    sl = slice(lo, lo + n)
    xd = C["xd"][sl] if xd is None else xd
    xb, y, coef = C["xb"][sl], C["y"][kind][sl], C["coef"]
    w = C["w"][sl] if weighted else torch.ones(n, dtype=torch.float64)
    off = C["off"][sl] if offset else torch.zeros(n, dtype=torch.float64)
    yd = C["yd"][kind][sl]
    wd = C["wd"][sl] if weighted else None
    offd = C["offd"][sl] if offset else None
    live = w != 0
    ck = None if init else coef
    G, st = GO.step(xd, d, yd, wd, offd, coef, s, init)
    G2, st2 = GO.step(xd, d, yd, wd, offd, coef, s, init)
    st3 = GO.step(xd, d, yd, wd, offd, coef, s, init, gram=False)
    ek, mk, zk, wk = (v.cpu() for v in GO.rows(xd, d, yd, wd, offd, ck, s))
    torch.cuda.synchronize()
    assert torch.equal(G, G2) and torch.equal(st, st2) and torch.equal(st, st3)           # (e)
    assert G.shape == (d + 2, d + 2) and G.dtype == torch.float64 and torch.equal(G, G.T)
    assert torch.isfinite(G).all() and torch.isfinite(st).all()
    x64 = xb.to(torch.float64)
    if not init:                                                                           # (a)
        eta_ref, _ = GO.rows_reference(xb, d, off, coef, s)
        assert not live.any() or (float(eta_ref[live].min()) > 0.25 and float(eta_ref[live].max()) < 4.0)
        bound = 2.0 * (d + 3) * U * ((x64.abs() @ coef[:d].abs()) + coef[d].abs() + off.abs())
        assert ((ek - eta_ref).abs() <= bound).all(), name
    # (b): the row terms at the kernel's own eta, torch CPU against the kernel and against torch on the GPU
    cpu = GO.row_terms(None if init else ek, y, w, off, s)
    gpu = {k: v.cpu() for k, v in GO.row_terms(None if init else ek.to(DEV), y.to(DEV), w.to(DEV), off.to(DEV), s).items()}
    assert (zk[~live] == 0).all() and (wk[~live] == 0).all()
    gp = GO.link_deriv(s, cpu["mu"])
    scales = {"mu": cpu["mu"].abs(), "wt": cpu["wt"].abs(),
              "z": cpu["eta"].abs() + off.abs() + (y.abs() + cpu["mu"].abs()) * gp.abs()}
    got = {"mu": mk, "z": zk, "wt": wk}
    if init:
        scales["eta"], got["eta"] = cpu["eta"].abs(), ek
    for k in got:
        mine = _units(got[k][live], cpu[k][live], scales[k][live])
        D = _units(gpu[k][live], cpu[k][live], scales[k][live])
        key = (name, "init" if init else "coef", k)
        _worst[key] = max(_worst.get(key, (0.0, 0.0)), (mine, D))
        assert mine <= max(4.0 * D, 16.0), (name, k, mine, D)
    # (c)
    want = gram_ops.gram_reference(xb, d, zk, wk)
    A = torch.cat([x64, torch.ones(n, 1, dtype=torch.float64), zk[:, None]], 1).abs()
    M = A.T @ (A * wk.abs()[:, None])
    g = G.cpu()
    assert (g[M == 0] == 0).all()
    assert ((g - want).abs() <= 2.0 * (n + 2) * U * M).all(), name
    # (d)
    t = GO.row_terms(None if init else ek, y, w, off, s)
    zero = torch.zeros_like(y)
    V = GO.variance(s, mk)
    r = y - mk
    ref = torch.stack([torch.where(live, w * GO.unit_deviance(s, y, mk), zero).sum(),
                       torch.where(live, (w * (r * r)) / V, zero).sum(), t["wy"].sum(), w.sum()])
    bound = (2.0 * (n + 2) + 64.0) * U * _abs_addends(s, y, w, mk)
    assert ((st.cpu() - ref).abs() <= bound).all(), (name, st.cpu(), ref, bound)


@pytest.mark.parametrize("d", WIDTHS)
def test_step_against_reference(d):
    C = _case(d)
    assert GO.kernel_supported(torch.bfloat16, C["dp"])
    for name in SPECS:
        for init in (True, False):
            for n in ROWS:
                _check(C, name, n, init)
    for name in SPECS:  # (b): the maxima so far (this width and the ones before it), kernel / D, zeros left out
        row = ", ".join(f"{form} {k} {_worst[(name, form, k)][0]:.2f} / {_worst[(name, form, k)][1]:.2f}"
                        for form in ("init", "coef") for k in ("eta", "mu", "z", "wt")
                        if _worst.get((name, form, k), (0.0, 0.0)) != (0.0, 0.0))
        print(f"(b) up to d = {d}, {name}: {row or 'all 0 / 0'}")


@pytest.mark.parametrize("d", [40, 128])
def test_several_tiles_per_workgroup(d):
    """70 001 rows are 1094 tiles: more than two workgroups per CU take, so every workgroup runs its tile loop (the
    loads one tile ahead, the four barriers per tile) several times; at 4099 rows each has one tile."""
    C = _case(d, BIG_N)
    for name in ("tweedie(1.5, log)", "binomial / logit"):
        for init in (True, False):
            _check(C, name, BIG_N, init)


@pytest.mark.parametrize("d", [17, 100])
def test_views_and_missing_columns(d):
    C = _case(d)
    name = "tweedie(1.5, log)"
    _check(C, name, N - 3, False, xd=C["xd"][3:], lo=3)             # a row-offset view
    _check(C, name, N, False, weighted=False, offset=False)          # w = None, off = None
    _check(C, name, N, True, weighted=False, offset=False)
    _check(C, "binomial / logit", 63, False, xd=C["xd"][5:68], lo=5, weighted=True, offset=False)


def test_pad_columns_rows_behind_the_view_and_dead_rows():
    """NaN bits in the pad columns and NaN rows behind the view change nothing, and rows of weight 0 add nothing
    whatever they hold: the same bits as a clean buffer of exactly n rows."""
    C = _case(40)
    s, kind = SPECS["tweedie(1.5, log)"]
    d, y, w, off, coef = 40, C["yd"][kind], C["wd"], C["offd"], C["coef"]
    clean = to_device_matrix(C["xb"].to(DEV), d)
    assert C["dp"] > d and torch.isnan(C["xd"][:, d:].to(torch.float32)).all()
    for init in (True, False):
        a = GO.step(C["xd"], d, y, w, off, coef, s, init)
        b = GO.step(clean, d, y, w, off, coef, s, init)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        dead = w == 0
        x2, y2, off2 = clean.clone(), y.clone(), off.clone()
        x2[dead] = 7.0
        y2[dead] = 3.5e4
        off2[dead] = -50.0
        c = GO.step(x2, d, y2, w, off2, coef, s, init)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_errors():
    C = _case(17)
    s, kind = SPECS["tweedie(1.5, log)"]
    y = C["yd"][kind]
    e = GO.step(C["xd"][:0], 17, y[:0], None, None, C["coef"], s, False)
    assert e[0].shape == (19, 19) and not e[0].any() and not e[1].any()
    with pytest.raises(ValueError):
        GO.step(C["xd"].to(torch.float32), 17, y, None, None, C["coef"], s, False)
    with pytest.raises(ValueError):
        GO.step(C["xd"], 17, y[:-1], None, None, C["coef"], s, False)
    with pytest.raises(ValueError):
        GO.step(C["xd"], 17, y, None, None, C["coef"][:-1], s, False)
    with pytest.raises(ValueError):
        GO.step(C["xb"], 17, C["y"][kind], None, None, C["coef"], s, False)  # host rows
    assert not GO.kernel_supported(torch.bfloat16, 256) and not GO.kernel_supported(torch.float32, 64)


# ------------------------------------------------------------------------------------------------ estimator
@pytest.fixture(scope="module")
def sessions():
    """A GPU session and a host session of this module's own, beside whichever session is active."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    gpu = SparkSession({"spark.master": "mi355x", "spark.app.name": "glr"})
    assert gpu.device.type == "cuda"
    host = SparkSession({"spark.master": "local", "spark.app.name": "glr-host"})
    assert host.device.type == "cpu"
    yield gpu, host
    host.stop()
    gpu.stop()


def _table():
    """3000 x 40 bf16 rows (independent columns of scale 1 .. 40 under a fixed orthogonal mix), a log exposure, a
    compound Poisson-gamma cost whose mean is log-linear in the first latent columns, and a poisson count."""
    rs = np.random.RandomState(13)
    n, d = 3000, 40
    latent = rs.randn(n, d)
    q, _ = np.linalg.qr(rs.randn(d, d))
    x = torch.as_tensor((latent * np.arange(1, d + 1)) @ q).to(torch.float32).to(torch.bfloat16)
    off = np.log(rs.uniform(0.5, 2.0, n))
    mu = np.exp(0.5 + 0.2 * latent[:, :5].sum(1) + off)
    cnt = rs.poisson(2.0 * np.sqrt(mu))
    cost = np.where(cnt > 0, rs.gamma(np.maximum(cnt, 1), 0.5 * np.sqrt(mu)), 0.0)
    return x, torch.as_tensor(cost), torch.as_tensor(off), torch.as_tensor(rs.poisson(mu).astype(np.float64))


def _counted(monkeypatch):
    calls = {"kernel": 0, "reference": 0}
    real, real_ref = GO.step, GO.step_reference

    def kernel(*a, **k):
        calls["kernel"] += 1
        return real(*a, **k)

    def reference(*a, **k):
        calls["reference"] += 1
        return real_ref(*a, **k)
    monkeypatch.setattr(GO, "step", kernel)
    monkeypatch.setattr(GO, "step_reference", reference)
    return calls


def _fit(df):
    m = GeneralizedLinearRegression(labelCol="cost", family="tweedie", variancePower=1.5, linkPower=0.0,
                                    offsetCol="off").fit(df)
    s = m.summary
    return np.r_[m.coefficients.toArray(), m.intercept], np.array([s.deviance, s.nullDeviance, s.dispersion]), \
        s.numIterations


def test_estimator_kernel_reference_and_host(sessions, monkeypatch):
    gpu, host = sessions
    x, cost, off, cnt = _table()
    dfg = gpu.createDataFrameFromTensors({"features": x.to(DEV), "cost": cost.to(DEV), "off": off.to(DEV),
                                          "count": cnt.to(DEV)})
    dfh = host.createDataFrameFromTensors({"features": x.to(torch.float64), "cost": cost, "off": off, "count": cnt})
    assert dfg._feature_matrix("features").dtype == torch.bfloat16 and not dfh._feature_matrix("features").is_cuda
    monkeypatch.delenv("CML_GLR_KERNEL", raising=False)
    calls = _counted(monkeypatch)
    fast, sum_fast, it_fast = _fit(dfg)
    assert calls["kernel"] == it_fast + 1 and calls["reference"] == 0
    calls["kernel"] = 0
    monkeypatch.setenv("CML_GLR_KERNEL", "0")
    slow, sum_slow, it_slow = _fit(dfg)
    assert calls["kernel"] == 0 and calls["reference"] == it_slow + 1
    calls["reference"] = 0
    cpu, sum_cpu, it_cpu = _fit(dfh)
    assert calls["kernel"] == 0 and calls["reference"] == it_cpu + 1
    assert it_fast == it_slow == it_cpu and it_fast > 2
    for what, a, b, c in (("coefficients", fast, slow, cpu), ("summary", sum_fast, sum_slow, sum_cpu)):
        D = np.abs(b - c).max()
        gap = np.abs(a - c).max()
        print(f"{what}: reference form vs host frame D = {D:.3e}, kernel vs host frame {gap:.3e}, "
              f"max |value| = {np.abs(c).max():.3e}")
        assert np.isfinite(a).all()
        if what == "coefficients":
            assert gap <= 10.0 * D
    # the four named families without an offset keep their path: K33 is not launched
    monkeypatch.delenv("CML_GLR_KERNEL", raising=False)
    calls["kernel"] = calls["reference"] = 0
    GeneralizedLinearRegression(labelCol="count", family="poisson").fit(dfg)
    assert calls["kernel"] == 0 and calls["reference"] == 0
    # transform takes the rows form and agrees with the host frame
    m = GeneralizedLinearRegression(labelCol="cost", family="tweedie", variancePower=1.5, linkPower=0.0,
                                    offsetCol="off").fit(dfg)
    pg = m.transform(dfg)._column_data("prediction").values.cpu()
    ph = m.transform(dfh)._column_data("prediction").values
    torch.testing.assert_close(pg, ph, rtol=1e-12, atol=0.0)
