"""K30 (``_native/csrc/mlp.hip``): the MLP loss, gradient and forward pass on bf16 rows against the reference form
on the same values (CPU f64), and the estimator on the kernel against its own reference form.

Op-level data: 4099 rows (the last 16-row group and the last tile are partial) of bf16 ``randn`` values, labels
uniform over the classes, parameters uniform in Spark's init range +-sqrt(6 / (in + out)). For d < dp the pad
columns of the device rows hold bf16 NaN bits.

Bound per gradient entry: |g - g_ref| <= 1e-9 M with M = sum_rows |a_{l-1,i}| (n for a bias), and for the loss
1e-9 sum_rows (|lse| + |z_y|). The order of an n-term f64 sum costs at most n 2^-53 = 4.6e-13 of the absolute
terms; a 512-term dot product 5.7e-14 of its absolute terms, which puts z_L off by at most about 1e-11 on this
data (init-range weights, |x| a few units, sigmoid' <= 1/4); delta's error is absolute, hence M with |delta| taken
as 1 (|delta_L| <= 1). 1e-9 leaves two orders over that worst case.
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import classification_more as CM
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import mlp_ops as MO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
N = 4099
SHAPES = [(3, [3, 5, 2]), (10, [10, 16, 3]), (17, [17, 17, 5]), (40, [40, 8, 4, 17]), (100, [100, 32, 32, 32]),
          (256, [256, 32, 2]), (512, [512, 16, 3])]
IDS = ["-".join(map(str, s[1])) for s in SHAPES]
_cache = {}


def _case(d, layers, labels=None):
    """bf16 rows (host and device, NaN bits in the pad columns), labels and parameters; made once per shape and
    shared, never modified."""
    key = (tuple(layers), labels)
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(1000 * d + len(layers))
    xb = torch.as_tensor(rs.randn(N, d)).to(torch.float32).to(torch.bfloat16)
    y = torch.as_tensor(rs.randint(0, layers[-1], N) if labels is None else np.full(N, labels)).to(torch.int32)
    p = torch.as_tensor(np.concatenate([rs.uniform(-np.sqrt(6.0 / (a + b)), np.sqrt(6.0 / (a + b)), a * b + b)
                                        for a, b in zip(layers[:-1], layers[1:])]))
    xd = to_device_matrix(xb.to(DEV), d).clone()
    dp = int(xd.shape[1])
    if d < dp:
        xd.view(torch.int16)[:, d:] = 0x7fc0
    out = dict(d=d, layers=layers, dp=dp, xb=xb, xd=xd, y=y, yd=y.to(DEV), p=p)
    _cache[key] = out
    return out


def _reference(C, n):
    """The reference form on the first n rows (CPU f64): the message, the bound's M per entry, the scores and
    the largest sum of absolute terms of a score."""
    key = ("ref", n)
    if key in C:
        return C[key]
    layers, p, d = C["layers"], C["p"], C["d"]
    x, y = C["xb"][:n].to(torch.float64), C["y"][:n].to(torch.int64)
    want = MO.loss_grad_reference(C["xb"][:n], d, C["y"][:n], layers, p)
    z = MO.forward_reference(C["xb"][:n], d, layers, p)
    params = CM._mlp_unpack(p, layers)
    acts = [x]
    for W, b in params[:-1]:
        acts.append(torch.sigmoid(acts[-1] @ W.T + b))
    M = [torch.cat([a.abs().sum(0)[:, None].expand(a.shape[1], W.shape[0]).reshape(-1),
                    torch.full((W.shape[0],), float(n), dtype=torch.float64)]) for a, (W, _) in zip(acts, params)]
    zy = z.gather(1, y[:, None])[:, 0]
    M.append((torch.logsumexp(z, 1).abs() + zy.abs()).sum().reshape(1))
    WL, bL = params[-1]
    zterms = float((acts[-1].abs() @ WL.abs().T + bL.abs()).max())
    C[key] = (want.numpy(), torch.cat(M).numpy(), z.numpy(), zterms)
    return C[key]


@pytest.mark.parametrize("d,layers", SHAPES, ids=IDS)
def test_loss_grad_against_reference(d, layers):
    C = _case(d, layers)
    assert MO.kernel_supported(torch.bfloat16, C["dp"], layers)
    for n in (N, 15, 1):
        want, M, _, _ = _reference(C, n)
        got = MO.loss_grad(C["xd"][:n], d, C["yd"][:n], layers, C["p"])
        again = MO.loss_grad(C["xd"][:n], d, C["yd"][:n], layers, C["p"])
        torch.cuda.synchronize()
        assert torch.equal(got, again)  # the same bits
        g = got.cpu().numpy()
        assert got.dtype == torch.float64 and g.shape == want.shape and np.isfinite(g).all()
        ratio = np.abs(g - want) / np.maximum(M, 1e-300)
        print(f"layers={layers} n={n}: max |g - g_ref| / M = {ratio[:-1].max():.3e}, loss {ratio[-1]:.3e}")
        assert (np.abs(g - want) <= 1e-9 * M).all()


@pytest.mark.parametrize("d,layers", [s for s in SHAPES if s[0] not in (256, 512)], ids=IDS[:5])
def test_pad_columns_are_masked(d, layers):
    """NaN bits in the pad columns change nothing: the same bits as zero padding."""
    C = _case(d, layers)
    assert torch.isnan(C["xd"][:, d:].to(torch.float32)).all() and C["dp"] > d
    clean = to_device_matrix(C["xb"].to(DEV), d)
    a = MO.loss_grad(C["xd"], d, C["yd"], layers, C["p"])
    b = MO.loss_grad(clean, d, C["yd"], layers, C["p"])
    assert torch.equal(a, b) and torch.isfinite(a).all()
    za = MO.forward(C["xd"], d, layers, C["p"])
    zb = MO.forward(clean, d, layers, C["p"])
    assert torch.equal(za, zb) and torch.isfinite(za).all()


@pytest.mark.parametrize("d,layers", SHAPES, ids=IDS)
def test_forward_against_reference(d, layers):
    C = _case(d, layers)
    for n in (N, 15, 1):
        _, _, want, zterms = _reference(C, n)
        z = MO.forward(C["xd"][:n], d, layers, C["p"])
        assert z.dtype == torch.float64 and z.shape == (n, layers[-1])
        got = z.cpu().numpy()
        top2 = np.sort(want, 1)[:, -2:]
        band = (top2[:, 1] - top2[:, 0]) <= 1e-9
        print(f"layers={layers} n={n}: max |z - z_ref| = {np.abs(got - want).max():.3e} of {zterms:.3e}, "
              f"rows in the label band {int(band.sum())}")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * zterms)
        assert band.mean() <= 0.001
        assert np.array_equal(got.argmax(1)[~band], want.argmax(1)[~band])


def test_pad_classes_and_pad_units():
    """3 of 16 class slots and 17 of 32 unit slots are real. A class that never occurs has delta = +softmax."""
    C = _case(10, [10, 16, 3], labels=2)
    want, M, _, _ = _reference(C, N)
    g = MO.loss_grad(C["xd"], 10, C["yd"], [10, 16, 3], C["p"]).cpu().numpy()
    assert np.isfinite(g).all() and (np.abs(g - want) <= 1e-9 * M).all()
    last = g[10 * 16 + 16:-1]
    W2, b2 = last[:16 * 3].reshape(16, 3), last[16 * 3:]
    assert (W2[:, :2] > 0).all() and (b2[:2] > 0).all() and (W2[:, 2] < 0).all() and b2[2] < 0
    C = _case(17, [17, 17, 5])
    want, M, _, _ = _reference(C, N)
    g = MO.loss_grad(C["xd"], 17, C["yd"], [17, 17, 5], C["p"]).cpu().numpy()
    assert np.isfinite(g).all() and (np.abs(g - want) <= 1e-9 * M).all()


def test_edge_cases():
    C = _case(3, [3, 5, 2])
    xd, yd, p = C["xd"], C["yd"], C["p"]
    g = MO.loss_grad(xd[:0], 3, yd[:0], [3, 5, 2], p)
    z = MO.forward(xd[:0], 3, [3, 5, 2], p)
    torch.cuda.synchronize()
    assert g.shape == (p.numel() + 1,) and not g.any() and z.shape == (0, 2)
    with pytest.raises(ValueError):
        MO.loss_grad(xd.to(torch.float32), 3, yd, [3, 5, 2], p)
    with pytest.raises(ValueError):
        MO.loss_grad(xd.T.contiguous().T, 3, yd, [3, 5, 2], p)
    with pytest.raises(ValueError):
        MO.loss_grad(xd, 3, yd, [3, 5, 2], p[:-1])
    with pytest.raises(ValueError):
        MO.forward(xd, 3, [3, 5, 3], p)
    with pytest.raises(ValueError):
        MO.loss_grad(xd, 3, yd.to(torch.int64), [3, 5, 2], p)
    with pytest.raises(ValueError):
        MO.forward(xd, 3, [3, 2], p[:8])


# ------------------------------------------------------------------------------------------------- estimator
@pytest.fixture(scope="module")
def spark():
    """A GPU session of this module's own, beside whichever session is active: a host session left active by
    another module would keep the frames on the CPU, where no kernel runs, and the modules that follow find the
    active session as they would without this one."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    s = SparkSession({"spark.master": "mi355x", "spark.app.name": "mlp"})
    assert s.device.type == "cuda"
    yield s
    s.stop()


def _labelled(n, d, k, seed=0):
    """f32 rows on the device and the labels of a planted linear rule with noise (f64)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=DEV)
    w = torch.randn(d, k, generator=g, device=DEV)
    y = torch.argmax(x @ w + 0.5 * torch.randn(n, k, generator=g, device=DEV), 1)
    return x, y.to(torch.float64)


def test_estimator_kernel_equals_reference(spark, monkeypatch):
    x, y = _labelled(20_000, 12, 3)
    df = spark.createDataFrameFromTensors({"features": x.to(torch.bfloat16), "label": y})
    est = CM.MultilayerPerceptronClassifier(layers=[12, 8, 3], seed=3, maxIter=5, tol=0.0)
    calls = []
    real, real_ref = MO.loss_grad, MO.loss_grad_reference

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(MO, "loss_grad", counted)
    fast = est.fit(df)
    out_fast = fast.transform(df)
    assert len(calls) >= 5
    del calls[:]
    monkeypatch.setenv("CML_MLP_KERNEL", "0")
    slow = est.fit(df)
    out_slow = slow.transform(df)
    monkeypatch.setattr(MO, "loss_grad_reference", lambda *a, **k: real_ref(*a, chunk=1000, **k))
    slow2 = est.fit(df)
    assert not calls
    assert fast.summary.totalIterations == slow.summary.totalIterations == 5
    np.testing.assert_allclose(fast.summary.objectiveHistory, slow.summary.objectiveHistory, rtol=1e-9)
    wf, ws, ws2 = (m.weights.toArray() for m in (fast, slow, slow2))
    D = np.abs(ws - ws2).max()
    diff = np.abs(wf - ws).max()
    print(f"weights: reference chunk 8192 vs 1000 D = {D:.3e}, kernel vs reference {diff:.3e}, "
          f"max |w| = {np.abs(ws).max():.3e}")
    assert diff <= 100.0 * D + 1e-12 * np.abs(ws).max()
    z = out_slow._column_data("rawPrediction").values.cpu().numpy()
    top2 = np.sort(z, 1)[:, -2:]
    band = (top2[:, 1] - top2[:, 0]) <= 1e-9
    pf = out_fast._column_data("prediction").values.cpu().numpy()
    ps = out_slow._column_data("prediction").values.cpu().numpy()
    assert band.mean() <= 0.001 and np.array_equal(pf[~band], ps[~band])
    assert len(np.unique(ps)) == 3


def test_other_columns_take_the_other_forms(spark, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("outside the kernel's limits: another form is expected")
    monkeypatch.setattr(MO, "loss_grad", boom)
    monkeypatch.setattr(MO, "forward", boom)
    x40, y40 = _labelled(2000, 40, 2)
    x256, y256 = _labelled(2000, 256, 2)
    x12, y12 = _labelled(2000, 12, 3)
    for feats, y, layers in ((x40.to(torch.bfloat16), y40, [40, 40, 2]),
                             (x256.cpu().to(torch.float8_e4m3fn), y256, [256, 8, 2]),
                             (x12.to(torch.bfloat16), y12, [12, 3])):
        df = spark.createDataFrameFromTensors({"features": feats, "label": y})
        m = CM.MultilayerPerceptronClassifier(layers=layers, seed=3, maxIter=3).fit(df)
        assert np.isfinite(m.weights.toArray()).all() and np.isfinite(m.summary.objectiveHistory).all()
        assert m.transform(df)._column_data("probability").values.shape == (2000, layers[-1])
    for name in ("loss_grad_reference", "forward_reference", "kernel_enabled", "kernel_supported", "lds_bytes"):
        monkeypatch.setattr(MO, name, boom)
    df = spark.createDataFrameFromTensors({"features": x12, "label": y12})  # f32: the dense form
    m = CM.MultilayerPerceptronClassifier(layers=[12, 8, 3], seed=3, maxIter=3).fit(df)
    assert m.transform(df)._column_data("prediction").values.shape == (2000,)


def test_fit_memory(spark):
    """Peak allocation during fit stays below half of X: the int32 labels (4 B per row against 64 B of X), the
    per-workgroup partials and the parameter images; no f64 copy, no one-hot matrix, no n x h activations."""
    x, y = _labelled(2_000_000, 32, 4)
    x = x.to(torch.bfloat16)
    df = spark.createDataFrameFromTensors({"features": x, "label": y})
    est = CM.MultilayerPerceptronClassifier(layers=[32, 16, 4], seed=3, maxIter=3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = est.fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    xbytes = x.numel() * x.element_size()
    print(f"fit peak rise {rise / x.shape[0]:.1f} B/row = {100.0 * rise / xbytes:.1f} % of X")
    assert rise < 0.5 * xbytes
    assert m.weights.toArray().shape == (32 * 16 + 16 + 16 * 4 + 4,)
