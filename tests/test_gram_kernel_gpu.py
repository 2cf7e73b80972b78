"""K31 (``_native/csrc/gram.hip``): the Gram matrix ``[X 1 z]^T W [X 1 z]`` of bf16 rows with 31 <= d <= 512 on the
f64 MFMA against the reference form on the same values (CPU f64), the routing of ``glm_ops.gram``, and the four
estimators that take their statistics from it.

Op-level data: 4099 rows (the last 16-row group and the last 64-row tile are partial, several slabs) of bf16
``randn`` values, ``z = 1e3 randn`` in f64 (not representable in bf16), ``w = rand`` with about 5 % exact zeros. The
device rows are in the ``to_device_matrix`` layout with bf16 NaN bits (0x7fc0) in the pad columns.

Bound per entry: ``|G - G_ref|[i][j] <= 2 (n + 2) 2^-53 M[i][j]`` with ``M[i][j] = sum_r |w_r a_ri a_rj|``: an n-term
f64 sum of once-rounded products in any order is within ``(n + 2) 2^-53 M`` of the exact value, and both sides carry
that error. Entries with ``M = 0`` must be exactly 0.

Estimators: the gap D between the GPU reference form and a CPU frame over the same values is the spread of the
arithmetic before K31 (summation order, placement of ``sqrt(w)``); the kernel may be 10 D from the CPU frame.
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import feature_extra as FE
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import (GeneralizedLinearRegression,
                                                                                        LinearRegression)
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.stat import Correlation
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import glm_ops
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import gram_ops as GO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
N = 4099
TAIL = 70  # rows behind the view, NaN
WIDTHS = [31, 48, 100, 128, 129, 257, 512]
ROWS = [N, 64, 63, 1]
_cache = {}


def _nan_pads(xd, d):
    if d < xd.shape[1]:
        xd.view(torch.int16)[:, d:] = 0x7fc0
    return xd


def _case(d):
    """bf16 rows (host; device with NaN bits in the pad columns and NaN rows behind row N), z and w; made once per
    width and shared, never modified."""
    if d in _cache:
        return _cache[d]
    rs = np.random.RandomState(31 * d)
    xb = torch.as_tensor(rs.randn(N, d)).to(torch.float32).to(torch.bfloat16)
    z = torch.as_tensor(1e3 * rs.randn(N))
    w = torch.as_tensor(rs.rand(N))
    w[rs.rand(N) < 0.05] = 0.0
    clean = to_device_matrix(xb.to(DEV), d)
    dp = int(clean.shape[1])
    big = torch.full((N + TAIL, dp), float("nan"), dtype=torch.bfloat16, device=DEV)
    big[:N] = clean
    _nan_pads(big, d)
    out = dict(d=d, dp=dp, xb=xb, z=z, w=w, clean=clean, xd=big[:N], zd=z.to(DEV), wd=w.to(DEV))
    _cache[d] = out
    return out


def _reference(C, n, weighted):
    key = ("ref", n, weighted)
    if key not in C:
        d = C["d"]
        w = C["w"][:n] if weighted else None
        want = GO.gram_reference(C["xb"][:n], d, C["z"][:n], w)
        A = torch.cat([C["xb"][:n].to(torch.float64), torch.ones(n, 1, dtype=torch.float64), C["z"][:n, None]], 1).abs()
        M = A.T @ (A * (w[:, None] if weighted else 1.0))
        C[key] = (want, M)
    return C[key]


@pytest.mark.parametrize("d", WIDTHS)
def test_against_reference(d):
    C = _case(d)
    assert GO.kernel_supported(torch.bfloat16, d)
    for n in ROWS:
        for weighted in (False, True):
            want, M = _reference(C, n, weighted)
            wd = C["wd"][:n] if weighted else None
            got = GO.gram(C["xd"][:n], d, C["zd"][:n], wd)
            again = GO.gram(C["xd"][:n], d, C["zd"][:n], wd)
            torch.cuda.synchronize()
            assert torch.equal(got, again)  # the same bits
            assert got.dtype == torch.float64 and got.shape == (d + 2, d + 2)
            assert torch.isfinite(got).all() and torch.equal(got, got.T)
            g = got.cpu()
            err = (g - want).abs()
            bound = 2.0 * (n + 2) * 2.0 ** -53 * M
            ratio = float((err / bound.clamp(min=1e-300)).max())
            print(f"d={d} n={n} weighted={weighted}: max |G - G_ref| / bound = {ratio:.3e}")
            assert (g[M == 0] == 0).all()
            assert (err <= bound).all()


@pytest.mark.parametrize("d", [31, 100, 129, 257])
def test_pad_columns_and_rows_behind_the_view_are_masked(d):
    """NaN bits in the pad columns and NaN rows behind the view change nothing: the same bits as zero padding in a
    buffer of exactly n rows."""
    C = _case(d)
    assert C["dp"] > d and torch.isnan(C["xd"][:, d:].to(torch.float32)).all()
    for n in (N, 63):
        a = GO.gram(C["xd"][:n], d, C["zd"][:n], C["wd"][:n])
        b = GO.gram(C["clean"][:n].clone(), d, C["zd"][:n].clone(), C["wd"][:n].clone())
        assert torch.equal(a, b) and torch.isfinite(a).all()


def test_rows_of_weight_zero_add_nothing():
    C = _case(100)
    dead = C["wd"] == 0
    assert 0 < int(dead.sum()) < N
    x2, z2 = C["clean"].clone(), C["zd"].clone()
    x2[dead] = 7.0
    z2[dead] = -3.5e4
    a = GO.gram(C["xd"], 100, C["zd"], C["wd"])
    b = GO.gram(x2, 100, z2, C["wd"])
    assert torch.equal(a, b)
    live = ~dead
    c = GO.gram(C["clean"][live], 100, C["zd"][live], C["wd"][live]).cpu()
    want, M = _reference(C, N, True)
    assert ((c - want).abs() <= 2.0 * (N + 2) * 2.0 ** -53 * M).all()


def test_other_layouts_and_errors():
    """Rows whose pitch is no multiple of 16 bytes (d = 31 as given, no pad columns) and f32 z / w go through the
    wrapper's own copies; anything outside the limits is an error, never another path."""
    C = _case(31)
    want, M = _reference(C, N, True)
    got = GO.gram(C["xb"].to(DEV), 31, C["zd"], C["wd"]).cpu()
    assert ((got - want).abs() <= 2.0 * (N + 2) * 2.0 ** -53 * M).all()
    e = GO.gram(C["xd"][:0], 31, C["zd"][:0], None)
    assert e.shape == (33, 33) and not e.any()
    with pytest.raises(ValueError):
        GO.gram(C["xd"].to(torch.float32), 31, C["zd"], None)
    with pytest.raises(ValueError):
        GO.gram(C["xd"], 30, C["zd"], None)
    with pytest.raises(ValueError):
        GO.gram(C["xd"], 31, C["zd"][:-1], None)
    with pytest.raises(ValueError):
        GO.gram(C["xb"], 31, C["z"], None)  # host rows


# --------------------------------------------------------------------------------------------------- routing
def _counted(monkeypatch):
    calls = {"kernel": 0, "reference": 0}
    real, real_ref = GO.gram, GO.gram_reference

    def kernel(*a, **k):
        calls["kernel"] += 1
        return real(*a, **k)

    def reference(*a, **k):
        calls["reference"] += 1
        return real_ref(*a, **k)
    monkeypatch.setattr(GO, "gram", kernel)
    monkeypatch.setattr(GO, "gram_reference", reference)
    return calls


def test_routing(monkeypatch):
    monkeypatch.delenv("CML_GRAM_KERNEL", raising=False)
    calls = _counted(monkeypatch)
    g = torch.Generator(device=DEV).manual_seed(5)
    n = 2000
    x = torch.randn(n, 600, generator=g, device=DEV)
    z = torch.randn(n, generator=g, device=DEV, dtype=torch.float64)
    w = torch.rand(n, generator=g, device=DEV, dtype=torch.float64)
    xb = x.to(torch.bfloat16)

    seen = []
    for rows, d, want in ((xb[:, :40].contiguous(), 40, (1, 0)),     # bf16 d = 40: K31
                          (xb[:, :12].contiguous(), 12, (0, 0)),     # bf16 d = 12: K15 as before
                          (xb, 600, (0, 1)),                          # bf16 d = 600: the reference form
                          (x[:, :40].contiguous(), 40, (0, 1))):     # f32 d = 40: the reference form
        calls["kernel"] = calls["reference"] = 0
        G = glm_ops.gram(rows, d, z, w)
        assert (calls["kernel"], calls["reference"]) == want
        assert G.shape == (d + 2, d + 2) and G.dtype == torch.float64 and torch.equal(G, G.T)
        seen.append(G)
    monkeypatch.setenv("CML_GRAM_KERNEL", "0")
    calls["kernel"] = calls["reference"] = 0
    off = glm_ops.gram(xb[:, :40].contiguous(), 40, z, w)
    assert (calls["kernel"], calls["reference"]) == (0, 1)
    # the kernel and the reference form of the same column agree within the bound of the op-level test
    A = torch.cat([xb[:, :40].to(torch.float64), torch.ones(n, 1, dtype=torch.float64, device=DEV), z[:, None]], 1).abs()
    M = A.T @ (A * w[:, None])
    assert ((seen[0] - off).abs() <= 2.0 * (n + 2) * 2.0 ** -53 * M).all()
    # host rows and empty shards keep the dense form
    calls["kernel"] = calls["reference"] = 0
    glm_ops.gram(xb[:, :40].cpu(), 40, z.cpu(), w.cpu())
    glm_ops.gram(xb[:0, :40], 40, z[:0], None)
    assert (calls["kernel"], calls["reference"]) == (0, 0)


# ------------------------------------------------------------------------------------------------ estimators
@pytest.fixture(scope="module")
def sessions():
    """A GPU session and a host session of this module's own, beside whichever session is active."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    gpu = SparkSession({"spark.master": "mi355x", "spark.app.name": "gram"})
    assert gpu.device.type == "cuda"
    host = SparkSession({"spark.master": "local", "spark.app.name": "gram-host"})
    assert host.device.type == "cpu"
    yield gpu, host
    host.stop()
    gpu.stop()


def _table():
    """3000 x 40 bf16 rows: independent columns of scale 1 .. 40 under a fixed orthogonal mix (a well separated
    covariance spectrum), a linear label with noise and a poisson count."""
    rs = np.random.RandomState(11)
    n, d = 3000, 40
    latent = rs.randn(n, d)
    q, _ = np.linalg.qr(rs.randn(d, d))
    x = torch.as_tensor((latent * np.arange(1, d + 1)) @ q).to(torch.float32).to(torch.bfloat16)
    y = latent[:, :6] @ np.array([2.0, -1.0, 0.5, 3.0, -2.0, 1.0]) + 0.3 * rs.randn(n) + 4.0
    cnt = rs.poisson(np.exp(0.5 + 0.2 * latent[:, :5].sum(1))).astype(np.float64)
    return x, torch.as_tensor(y), torch.as_tensor(cnt)


def _fits(df):
    pca = FE.PCA(k=3, inputCol="features", outputCol="p").fit(df)
    lr = LinearRegression(labelCol="label", solver="normal", regParam=0.1).fit(df)
    glr = GeneralizedLinearRegression(labelCol="count", family="poisson").fit(df)
    corr = Correlation.corr(df, "features").head()[0].toArray()
    return {"pca": np.r_[pca.pc.toArray().reshape(-1), pca.explainedVariance.toArray()],
            "lr": np.r_[lr.coefficients.toArray(), lr.intercept],
            "glr": np.r_[glr.coefficients.toArray(), glr.intercept],
            "corr": corr.reshape(-1)}, glr.summary.numIterations


def test_estimators_kernel_reference_and_host(sessions, monkeypatch):
    gpu, host = sessions
    x, y, cnt = _table()
    cols = {"features": x, "label": y, "count": cnt}
    dfg = gpu.createDataFrameFromTensors({k: v.to(DEV) for k, v in cols.items()})
    dfh = host.createDataFrameFromTensors({"features": x.to(torch.float64), "label": y, "count": cnt})
    assert dfg._feature_matrix("features").dtype == torch.bfloat16 and not dfh._feature_matrix("features").is_cuda
    monkeypatch.delenv("CML_GRAM_KERNEL", raising=False)
    calls = _counted(monkeypatch)
    fast, it_fast = _fits(dfg)
    assert calls["kernel"] >= 4 and calls["reference"] == 0
    calls["kernel"] = 0
    monkeypatch.setenv("CML_GRAM_KERNEL", "0")
    slow, it_slow = _fits(dfg)
    assert calls["kernel"] == 0 and calls["reference"] >= 4
    cpu, it_cpu = _fits(dfh)
    assert it_fast == it_slow == it_cpu and it_fast > 1
    for name in ("pca", "lr", "glr", "corr"):
        D = np.abs(slow[name] - cpu[name]).max()
        gap = np.abs(fast[name] - cpu[name]).max()
        print(f"{name}: reference form vs host frame D = {D:.3e}, kernel vs host frame {gap:.3e}, "
              f"max |value| = {np.abs(cpu[name]).max():.3e}")
        assert np.isfinite(fast[name]).all()
        assert gap <= 10.0 * D


def test_pca_memory(sessions, monkeypatch):
    """PCA on 200 000 x 256 bf16 (102 MB): the fit's peak rise stays within the size of the bf16 column (the slab
    partials of K31; the dense form's f64 copy alone is 413 MB), the transform's within its (n, 8) f64 output plus one
    chunk: the f64 copy of ``_TRANSFORM_CHUNK`` rows and the (d, 8) f64 components it is multiplied by."""
    gpu, _ = sessions
    monkeypatch.delenv("CML_GRAM_KERNEL", raising=False)
    n, d, k = 200_000, 256, 8
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(n, d, generator=g, device=DEV).to(torch.bfloat16)
    df = gpu.createDataFrameFromTensors({"features": x})
    est = FE.PCA(k=k, inputCol="features", outputCol="p")
    xbytes = x.numel() * x.element_size()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = est.fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"fit peak rise {rise / 1e6:.1f} MB of the column's {xbytes / 1e6:.1f} MB")
    assert rise <= xbytes
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = m.transform(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    allowed = n * k * 8 + FE._TRANSFORM_CHUNK * d * 8 + d * k * 8
    print(f"transform peak rise {rise / 1e6:.1f} MB, allowed {allowed / 1e6:.1f} MB")
    assert rise <= allowed
    p = out._column_data("p").values
    assert p.shape == (n, k) and p.dtype == torch.float64
    want = x[:1000].to(torch.float64) @ torch.as_tensor(m.pc.toArray(), device=DEV)
    torch.testing.assert_close(p[:1000], want, rtol=1e-12, atol=1e-12)
