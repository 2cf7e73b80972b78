"""K34 (``_native/csrc/nb.hip``): the naive Bayes moments and scores of bf16 rows on the f64 MFMA against the
reference forms of ``ops/nb_ops.py`` evaluated in f64 on the CPU, never against the kernel itself, and the routing of
NaiveBayes.

Op-level data: 4099 rows in the ``to_device_matrix`` layout with bf16 NaN bits (0x7fc0) in the pad columns and 70 NaN
rows behind the view; the row counts 4099, 64, 63, 1 are prefixes of it, and one case has 70 001 rows (more tiles than
workgroups). Integer counts 0 .. 8 (exact in bf16) and a ``randn`` column; ``w = rand`` with about 5 % exact zeros.

Bounds (u = 2^-53; cnt_c the rows of class c):
(a) moments, unweighted counts: ``n_c``, ``S1``, ``S2`` and ``bad`` are the reference's bit for bit (every partial sum
    is an integer below 2^53).
(b) moments, weighted and shifted: ``|S1 - ref|[c][i] <= 2 (cnt_c + 2) u sum |w (x_i - m_ci)|``, ``|S2 - ref|[c][i]
    <= (2 (cnt_c + 2) + 8) u sum w (x_i - m_ci)^2``, ``|n_c - ref| <= 2 (cnt_c + 2) u sum w``: a cnt-term f64 sum on
    both sides, the subtraction and the square in between. Entries whose bound is 0 are exactly 0; ``bad`` is exact.
(c) raw before the lse: linear / complement ``2 (d + 3) u (sum_i |x_i W_ci| + |b_c|)``, gaussian
    ``(2 (d + 3) + 8) u (1/2 sum_i (x_i - W_ci)^2 iv_ci + |b_c|)``. Complement's raw is ``s - lse``: the log-sum-exp
    moves by at most the largest change of an ``s_c``, and its own evaluation (a max, C exp, a sum, a log, an add, on
    both sides) is within ``16 u (1 + |lse|)``, so its bound is ``bound_c + max_c' bound_c' + 16 u (1 + |lse|)``.
(d) prob and the lse against torch on the CPU at the kernel's own ``s`` (complement: ``exp`` of the kernel's own raw),
    in units of ``u (1 + |s - lse|) prob``; D is the same quantity between torch on the GPU and torch on the CPU; the
    kernel stays within ``max(4 D, 16)`` units.
    Measured maxima on an MI355X over all widths, class counts and row counts (units; kernel / D):
      linear 4.23 / 3.99, complement 1.18 / 1.18, gaussian 4.02 / 4.02 (all within the floor of 16)
(e) pred is the lowest-index argmax of the kernel's own raw on every row, and the reference's prediction on every row
    whose reference top-2 margin exceeds twice the row's largest raw bound; at most 1 % of the rows may be left out
    (asserted of the reference alone).

Estimator: the gap D between the GPU reference form and a CPU frame over the same values is the spread of the
arithmetic before K34; the kernel may be 10 D from the CPU frame (the convention of ``test_gram_kernel_gpu.py``).
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd import _native
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import NaiveBayes
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import nb_ops as NO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
N = 4099
TAIL = 70  # rows behind the view, NaN
WIDTHS = [1, 15, 16, 17, 40, 100, 128, 300, 512]
ROWS = [N, 64, 63, 1]
BIG_N = 70_001
CLASSES = [1, 2, 3, 16, 17, 32]
U = 2.0 ** -53
_cache = {}
_worst = {}


def _layout(xb, d):
    """The device rows of a host bf16 matrix: NaN bits in the pad columns, NaN rows behind the view."""
    n = xb.shape[0]
    clean = to_device_matrix(xb.to(DEV), d)
    dp = int(clean.shape[1])
    big = torch.full((n + TAIL, dp), float("nan"), dtype=torch.bfloat16, device=DEV)
    big[:n] = clean
    if d < dp:
        big.view(torch.int16)[:, d:] = 0x7fc0
    return big[:n], dp


def _case(d, n=N):
    """The data of a width; made once and shared, never modified."""
    if (d, n) in _cache:
        return _cache[(d, n)]
    rs = np.random.RandomState(2000 + d + (n - N))
    cnt = torch.as_tensor(rs.randint(0, 9, (n, d)).astype(np.float32)).to(torch.bfloat16)
    real = torch.as_tensor(rs.randn(n, d).astype(np.float32)).to(torch.bfloat16)
    near = torch.as_tensor((1000.0 + 4.0 * rs.randint(-2, 3, (n, d))).astype(np.float32)).to(torch.bfloat16)
    w = torch.as_tensor(rs.rand(n))
    w[rs.rand(n) < 0.05] = 0.0
    C = dict(d=d, n=n, cnt=cnt, real=real, near=near, w=w, wd=w.to(DEV), u=rs.rand(n),
             W=rs.randn(32, d), b=rs.randn(32), iv=rs.uniform(0.5, 2.0, (32, d)), shift=0.5 * rs.randn(32, d))
    for k in ("cnt", "real", "near"):
        C[k + "_d"], C["dp"] = _layout(C[k], d)
    assert (C["near"].to(torch.float64) - 1000.0).abs().max() <= 8.0
    _cache[(d, n)] = C
    return C


def _labels(C, k, n):
    return torch.as_tensor(np.floor(C["u"][:n] * k).astype(np.int64))


# --------------------------------------------------------------------------------------------------- moments
def _check_counts(C, k, n):
    """(a): unweighted integer counts, bit for bit."""
    d, lab = C["d"], _labels(C, k, n)
    want, wbad = NO.moments_reference(C["cnt"][:n], d, lab, None, k)
    got, gbad = NO.moments(C["cnt_d"][:n], d, lab.to(DEV), None, k)
    assert torch.equal(got.cpu(), want) and torch.equal(gbad.cpu(), wbad), (d, k, n)
    first, fbad = NO.moments(C["cnt_d"][:n], d, lab.to(DEV), None, k, second=False)
    assert torch.equal(first[:, :1 + d], got[:, :1 + d]) and not first[:, 1 + d:].any() and torch.equal(fbad, gbad)
    assert float(wbad[0]) == 0.0 and float(want[:, 0].sum()) == n


def _check_weighted(C, k, n, shifted=True, weighted=True, xd=None, lo=0):
    """(b): weighted, shifted moments of the randn column."""
    d = C["d"]
    sl = slice(lo, lo + n)
    lab = _labels(C, k, lo + n)[sl]
    w = C["w"][sl] if weighted else None
    shift = C["shift"][:k] if shifted else None
    xd = C["real_d"][sl] if xd is None else xd
    want, wbad = NO.moments_reference(C["real"][sl], d, lab, w, k, shift)
    got, gbad = NO.moments(xd, d, lab.to(DEV), C["wd"][sl] if weighted else None, k, shift)
    again, abad = NO.moments(xd, d, lab.to(DEV), C["wd"][sl] if weighted else None, k, shift)
    assert torch.equal(got, again) and torch.equal(gbad, abad)           # two calls, the same bits
    got = got.cpu()
    assert torch.equal(gbad.cpu(), wbad) and (n * d < 64 or float(wbad[0]) > 0)
    x = C["real"][sl].to(torch.float64)
    wv = torch.ones(n, dtype=torch.float64) if w is None else w
    m = torch.zeros(k, d, dtype=torch.float64) if shift is None else torch.as_tensor(shift)
    for c in range(k):
        sel = lab == c
        cntc = int(sel.sum())
        dev = x[sel] - m[c]
        b1 = 2.0 * (cntc + 2) * U * (wv[sel, None] * dev).abs().sum(0)
        b2 = (2.0 * (cntc + 2) + 8.0) * U * (wv[sel, None] * dev * dev).sum(0)
        b0 = 2.0 * (cntc + 2) * U * wv[sel].sum()
        e1 = (got[c, 1:1 + d] - want[c, 1:1 + d]).abs()
        e2 = (got[c, 1 + d:] - want[c, 1 + d:]).abs()
        assert (e1 <= b1).all() and (e2 <= b2).all() and abs(float(got[c, 0] - want[c, 0])) <= float(b0), (d, k, n, c)
        assert (got[c, 1:1 + d][b1 == 0] == 0).all() and (got[c, 1 + d:][b2 == 0] == 0).all()
        assert float(b0) > 0 or float(got[c, 0]) == 0.0


@pytest.mark.parametrize("d", WIDTHS)
def test_moments_against_reference(d):
    C = _case(d)
    assert NO.kernel_supported(torch.bfloat16, C["dp"], (32, False))
    for k in CLASSES:
        # a shift table goes with the gaussian limits: 17 classes at the padded width 512
        ks = k if NO.kernel_supported(torch.bfloat16, C["dp"], (k, True)) else 17
        assert ks == k or (C["dp"], k) == (512, 32)
        for n in ROWS:
            _check_counts(C, k, n)
            _check_weighted(C, ks, n)
            _check_weighted(C, k, n, shifted=False)


@pytest.mark.parametrize("d", [40, 300])
def test_moments_several_tiles_per_workgroup(d):
    """70 001 rows are more tiles than a launch has workgroups, so every workgroup runs its tile loop (the loads one
    tile ahead, the two barriers per tile) several times."""
    C = _case(d, BIG_N)
    for k in (3, 17):
        _check_counts(C, k, BIG_N)
        _check_weighted(C, k, BIG_N)


@pytest.mark.parametrize("d", [17, 100])
def test_moments_views_missing_weights_and_foreign_labels(d):
    C = _case(d)
    _check_weighted(C, 3, N - 3, xd=C["real_d"][3:], lo=3)               # a row-offset view
    _check_weighted(C, 17, 63, xd=C["real_d"][5:68], lo=5)
    _check_weighted(C, 3, N, weighted=False)                             # weights = None
    _check_weighted(C, 3, N, weighted=False, shifted=False)
    # labels >= C (and negative ones) add nothing: the same bits as with weight 0 on those rows
    k = 3
    lab = _labels(C, k, N)
    odd = lab.clone()
    odd[:40] = torch.as_tensor([k, k + 1, 31, 32, 1000, -1, -7, 2 ** 31 - 1] * 5)
    w0 = C["w"].clone()
    w0[:40] = 0.0
    for shift in (None, C["shift"][:k]):
        a = NO.moments(C["real_d"], d, odd.to(DEV), C["wd"], k, shift)
        b = NO.moments(C["real_d"], d, lab.to(DEV), w0.to(DEV), k, shift)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        want, _ = NO.moments_reference(C["real"], d, odd, C["w"], k, shift)
        torch.testing.assert_close(a[0].cpu(), want, rtol=1e-11, atol=1e-11)


def test_pad_columns_and_rows_behind_the_view():
    """NaN bits in the pad columns and NaN rows behind the view change nothing: the bits of a clean buffer."""
    C = _case(40)
    d, k = 40, 3
    lab = _labels(C, k, N).to(DEV)
    clean = to_device_matrix(C["real"].to(DEV), d)
    assert C["dp"] > d and torch.isnan(C["real_d"][:, d:].to(torch.float32)).all()
    a = NO.moments(C["real_d"], d, lab, C["wd"], k, C["shift"][:k])
    b = NO.moments(clean, d, lab, C["wd"], k, C["shift"][:k])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for kind in NO.KINDS:
        iv = C["iv"][:k] / d if kind == "gaussian" else None
        for p, q in zip(NO.scores(C["real_d"], d, kind, C["W"][:k], C["b"][:k], iv),
                        NO.scores(clean, d, kind, C["W"][:k], C["b"][:k], iv)):
            assert torch.equal(p, q) and torch.isfinite(p).all()


def test_no_rows_limits_and_errors():
    C = _case(17)
    lab = _labels(C, 3, N).to(DEV)
    calls = []
    lib = _native.kernels()

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(lib, name)
    real = _native.kernels
    _native.kernels = lambda: Spy()
    try:
        m, bad = NO.moments(C["real_d"][:0], 17, lab[:0], None, 3)
        r, p, y = NO.scores(C["real_d"][:0], 17, "linear", C["W"][:3], C["b"][:3])
    finally:
        _native.kernels = real
    assert not calls                                                       # n = 0 launches nothing
    assert m.shape == (3, 35) and not m.any() and not bad.any() and r.shape == (0, 3) and y.shape == (0,)
    for dp in NO.WIDTHS:
        for k in range(1, 33):
            for g in (False, True):
                lds = int(lib.cml_nb_lds(dp, k, int(g)))
                assert lds == (NO.lds_bytes(dp, k, g) if NO.kernel_supported(torch.bfloat16, dp, (k, g)) else 0)
    assert int(lib.cml_nb_lds(512, 33, 0)) == 0 and int(lib.cml_nb_lds(48, 2, 0)) == 0
    with pytest.raises(ValueError):
        NO.moments(C["real_d"].to(torch.float32), 17, lab, None, 3)
    with pytest.raises(ValueError):
        NO.moments(C["real"], 17, lab, None, 3)                           # host rows
    with pytest.raises(ValueError):
        NO.moments(C["real_d"], 17, lab[:-1], None, 3)
    with pytest.raises(ValueError):
        NO.moments(C["real_d"], 17, lab, None, 33)
    with pytest.raises(ValueError):
        NO.scores(C["real_d"], 17, "gaussian", C["W"][:3], C["b"][:3])    # no iv
    wide = _case(512)
    with pytest.raises(ValueError):
        NO.scores(wide["real_d"], 512, "gaussian", wide["W"][:18], wide["b"][:18], wide["iv"][:18])
    with pytest.raises(ValueError):
        NO.moments(wide["real_d"], 512, _labels(wide, 18, N).to(DEV), None, 18, wide["shift"][:18])


# ---------------------------------------------------------------------------------------------------- scores
def _units(got, want, scale):
    return float(((got - want).abs() / (U * scale).clamp(min=1e-300)).max()) if got.numel() else 0.0


def _check_scores(C, kind, k, n, col="real"):
    d = C["d"]
    xb, xd = C[col][:n], C[col + "_d"][:n]
    x = xb.to(torch.float64)
    if kind == "gaussian":
        W = C["W"][:k] * 0.3 + (1000.0 if col == "near" else 0.0)
        iv = C["iv"][:k] / d * (0.05 if col == "near" else 1.0)
    else:
        W, iv = C["W"][:k] * (0.3 / np.sqrt(d)), None
    b = C["b"][:k]
    Wt, bt = torch.as_tensor(W), torch.as_tensor(b)
    ref = NO.scores_reference(xb, d, kind, W, b, iv)
    raw, prob, pred = (v.cpu() for v in NO.scores(xd, d, kind, W, b, iv))
    again = NO.scores(xd, d, kind, W, b, iv)
    assert torch.equal(again[0].cpu(), raw) and torch.equal(again[1].cpu(), prob) and torch.equal(again[2].cpu(), pred)
    assert raw.shape == (n, k) and prob.shape == (n, k) and pred.shape == (n,) and raw.dtype == torch.float64
    # (c)
    if kind == "gaussian":
        ivt = torch.as_tensor(iv)
        quad = torch.stack([0.5 * ((x - Wt[c]) ** 2 * ivt[c]).sum(1) for c in range(k)], 1)
        bound = (2.0 * (d + 3) + 8.0) * U * (quad + bt.abs())
    else:
        bound = 2.0 * (d + 3) * U * (x.abs() @ Wt.abs().T + (bt.abs() if kind == "linear" else 0.0))
    if kind == "complement":
        lse = torch.logsumexp(x @ Wt.T, 1, keepdim=True)
        bound = bound + bound.max(1, keepdim=True).values + 16.0 * U * (1.0 + lse.abs())
    assert ((raw - ref[0]).abs() <= bound).all(), (kind, d, k, n, float(((raw - ref[0]).abs() / bound).max()))
    # (d)
    if kind == "complement":
        t_cpu, t_gpu = raw, raw.to(DEV)
        p_cpu, p_gpu = torch.exp(t_cpu), torch.exp(t_gpu).cpu()
        assert (torch.logsumexp(raw, 1).abs() <= 16.0 * U * k).all()
    else:
        t_cpu = raw - torch.logsumexp(raw, 1, keepdim=True)
        p_cpu = torch.exp(t_cpu)
        rg = raw.to(DEV)
        p_gpu = torch.exp(rg - torch.logsumexp(rg, 1, keepdim=True)).cpu()
    scale = (1.0 + t_cpu.abs()) * p_cpu
    mine, D = _units(prob, p_cpu, scale), _units(p_gpu, p_cpu, scale)
    _worst[kind] = max(_worst.get(kind, (0.0, 0.0)), (mine, D))
    assert mine <= max(4.0 * D, 16.0), (kind, d, k, n, mine, D)
    # (e)
    ar = torch.arange(k)
    own = torch.where(raw == raw.max(1, keepdim=True).values, ar, k).min(1).values.to(torch.float64)
    assert torch.equal(pred, own)
    if k > 1:
        top = torch.topk(ref[0], 2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > 2.0 * bound.max(1).values
        assert int((~clear).sum()) <= 0.01 * n or n < 100, (kind, d, k, n)  # the reference alone: few close calls
        assert torch.equal(pred[clear], ref[2][clear])
    else:
        assert not pred.any()


@pytest.mark.parametrize("d", WIDTHS)
def test_scores_against_reference(d):
    C = _case(d)
    for kind in NO.KINDS:
        for k in CLASSES:
            if not NO.kernel_supported(torch.bfloat16, C["dp"], (k, kind == "gaussian")):
                assert (C["dp"], kind, k) == (512, "gaussian", 32)
                k = 17  # the last class count the table takes at this width
            for n in ROWS:
                _check_scores(C, kind, k, n)
    print("(d) up to d = %d: " % d + ", ".join(f"{kd} {m:.2f} / {D:.2f}" for kd, (m, D) in sorted(_worst.items())))


@pytest.mark.parametrize("d", [16, 100, 512])
def test_gaussian_scores_where_the_mean_sits(d):
    """x = 1000 + {0, +-4, +-8} and theta = 1000 + small: ``x^2 iv - 2 x theta iv + theta^2 iv`` loses every digit of
    the quadratic (its terms are 1e6 iv d), the centred form none."""
    C = _case(d)
    for k in (3, 17):
        _check_scores(C, "gaussian", k, N, col="near")


@pytest.mark.parametrize("d", [40, 300])
def test_scores_several_tiles_per_workgroup(d):
    C = _case(d, BIG_N)
    for kind in NO.KINDS:
        _check_scores(C, kind, 3, BIG_N)
    _check_scores(C, "linear", 17, BIG_N)


# ------------------------------------------------------------------------------------------------ estimator
@pytest.fixture(scope="module")
def sessions():
    """A GPU session and a host session of this module's own, beside whichever session is active."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    gpu = SparkSession({"spark.master": "mi355x", "spark.app.name": "nb"})
    assert gpu.device.type == "cuda"
    host = SparkSession({"spark.master": "local", "spark.app.name": "nb-host"})
    assert host.device.type == "cpu"
    yield gpu, host
    host.stop()
    gpu.stop()


def _counted(monkeypatch):
    calls = {}
    for name in ("moments", "moments_reference", "scores", "scores_reference"):
        def wrap(*a, _f=getattr(NO, name), _n=name, **kw):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a, **kw)
        monkeypatch.setattr(NO, name, wrap)
    return calls


def _table(mt, n=3000, d=40, k=3):
    rs = np.random.RandomState(21)
    y = rs.randint(0, k, n)
    if mt == "gaussian":
        x = rs.randn(n, d) + (y[:, None] * np.linspace(-1.0, 1.0, d))
    elif mt == "bernoulli":
        x = (rs.rand(n, d) < 0.2 + 0.2 * (y[:, None] == np.arange(d)[None] % k)).astype(np.float64)
    else:
        x = rs.poisson(1.0 + 2.0 * (y[:, None] == np.arange(d)[None] % k)).astype(np.float64)
    xb = torch.as_tensor(x).to(torch.float32).to(torch.bfloat16)
    return xb, torch.as_tensor(y.astype(np.float64)), torch.as_tensor(rs.uniform(0.5, 2.0, n))


def _fit(df, mt):
    m = NaiveBayes(modelType=mt, weightCol="w", smoothing=0.7).fit(df)
    out = m.transform(df)
    return m, np.r_[m.pi.toArray(), m.theta.toArray().reshape(-1), m.sigma.toArray().reshape(-1)], \
        out._column_data("probability").values.cpu().numpy(), out._column_data("prediction").values.cpu().numpy()


@pytest.mark.parametrize("mt", ["multinomial", "bernoulli", "gaussian", "complement"])
def test_estimator_kernel_reference_and_host(sessions, monkeypatch, mt):
    gpu, host = sessions
    xb, y, w = _table(mt)
    dfg = gpu.createDataFrameFromTensors({"features": xb.to(DEV), "label": y.to(DEV), "w": w.to(DEV)})
    dfh = host.createDataFrameFromTensors({"features": xb.to(torch.float64), "label": y, "w": w})
    assert dfg._feature_matrix("features").dtype == torch.bfloat16 and not dfh._feature_matrix("features").is_cuda
    monkeypatch.delenv("CML_NB_KERNEL", raising=False)
    calls = _counted(monkeypatch)
    passes = 2 if mt == "gaussian" else 1
    _, fast, pf, yf = _fit(dfg, mt)
    assert calls == {"moments": passes, "scores": 1}
    calls.clear()
    monkeypatch.setenv("CML_NB_KERNEL", "0")
    _, slow, ps, ys = _fit(dfg, mt)
    assert calls == {"moments_reference": passes, "scores_reference": 1}
    calls.clear()
    _, cpu, pc, yc = _fit(dfh, mt)
    assert not calls                                                       # a host frame keeps the dense form
    for what, a, b, c in (("model", fast, slow, cpu), ("probability", pf, ps, pc)):
        D, gap = np.abs(b - c).max(), np.abs(a - c).max()
        print(f"{mt} {what}: reference form vs host frame D = {D:.3e}, kernel vs host frame {gap:.3e}, "
              f"max |value| = {np.abs(c).max():.3e}")
        assert np.isfinite(a).all() and gap <= 10.0 * D
    assert (yf == yc).mean() >= 0.999 and (ys == yc).mean() >= 0.999


def test_estimator_routes(sessions, monkeypatch):
    gpu, _ = sessions
    monkeypatch.delenv("CML_NB_KERNEL", raising=False)
    calls = _counted(monkeypatch)
    xb, y, w = _table("multinomial")
    # e4m3 rows take the reference form
    df8 = gpu.createDataFrameFromTensors({"features": xb.to(torch.float8_e4m3fn), "label": y, "w": w})
    assert df8._feature_matrix("features").dtype == torch.float8_e4m3fn
    m8, t8, _, _ = _fit(df8, "multinomial")
    assert calls == {"moments_reference": 1, "scores_reference": 1}
    calls.clear()
    # ... and so do 40 classes
    y40 = torch.as_tensor(np.arange(len(y)) % 40.0)
    df40 = gpu.createDataFrameFromTensors({"features": xb.to(DEV), "label": y40.to(DEV), "w": w.to(DEV)})
    m40 = _fit(df40, "complement")[0]
    assert m40.numClasses == 40 and calls == {"moments_reference": 1, "scores_reference": 1}
    calls.clear()
    # an f32 frame keeps the dense form, and gives the bf16 frame's model (the same values)
    df32 = gpu.createDataFrameFromTensors({"features": xb.to(torch.float32).to(DEV), "label": y.to(DEV),
                                           "w": w.to(DEV)})
    t32 = _fit(df32, "multinomial")[1]
    assert not calls
    np.testing.assert_allclose(t8, t32, rtol=1e-12)
    # the feature checks, from the counts of pass 1
    dfb = gpu.createDataFrameFromTensors({"features": xb.to(DEV), "label": y.to(DEV)})
    with pytest.raises(ValueError, match="0/1 feature values"):
        NaiveBayes(modelType="bernoulli").fit(dfb)
    neg = xb.clone()
    neg[17, 3] = -1.0
    dfn = gpu.createDataFrameFromTensors({"features": neg.to(DEV), "label": y.to(DEV)})
    for mt in ("multinomial", "complement"):
        with pytest.raises(ValueError, match="non-negative feature values"):
            NaiveBayes(modelType=mt).fit(dfn)
    NaiveBayes(modelType="gaussian").fit(dfn)


def test_fit_memory(sessions, monkeypatch):
    """2M x 64 bf16, C = 4, gaussian: the kernel path allocates int32 labels, per-workgroup partials and nothing of
    size n x d; the dense form's rise is more than 8 x the bytes of X."""
    gpu, _ = sessions
    monkeypatch.delenv("CML_NB_KERNEL", raising=False)
    n, d = 2_000_000, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(n, d, device=DEV, generator=g, dtype=torch.float32).to(torch.bfloat16)
    y = torch.randint(0, 4, (n,), device=DEV, generator=g).to(torch.float64)
    df = gpu.createDataFrameFromTensors({"features": x, "label": y})
    assert df._feature_matrix("features").dtype == torch.bfloat16
    xbytes = n * d * 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = NaiveBayes(modelType="gaussian").fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"fit of 2M x 64 bf16, gaussian, C = 4: peak rise {rise / 2 ** 20:.1f} MiB = {rise / xbytes:.3f} x X")
    assert m.numClasses == 4 and rise < 0.5 * xbytes
