"""K29 (``_native/csrc/lda.hip``): the LDA E-step on bf16 rows against the reference form on the same values (on
the CPU), and the estimator on the kernel against its own reference form.

Op-level data: the planted-topic corpus of ``tests/test_lda_estep.py``, restated here. Topics ~ Dirichlet(0.1)
over V terms, document mixtures ~ Dirichlet(0.3), length ~ Poisson(m) + 1, lambda = Gamma(100, 0.01) + 50 topics,
alpha = 1 / k, gamma0 ~ Gamma(100, 0.01); 130 documents (two 64-document tiles and a partial 16-document group).
Each case asserts on the CPU reference that every count is at most 256 (exact in bf16) and that no active sweep's
change lies within 1e-9 of the 1e-3 threshold: two f64 summation orders move a change by about 1e-15 of gamma,
so with that margin the sweep counts of two correct evaluations are equal, and are compared exactly.

Bounds: gamma elementwise at rtol 1e-10 (the project's bound between two f64 evaluations of the E-step,
``tests/test_lda_pic.py``); every sstats entry, a sum of like-signed terms, within 1e-9 of the reference entry
(one decade over the bound its terms inherit from gamma; an entry that is 0 in the reference is exactly 0);
logphat within 1e-9 of its sum of absolute terms.
"""
import numpy as np
import pytest
import torch
from scipy.special import digamma

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import lda as L
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import lda_ops as LO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
B = 130
SHAPES = [(6, 3, 12), (16, 2, 8), (24, 10, 40), (100, 16, 120), (256, 32, 300), (512, 16, 300), (40, 17, 60)]
_cache = {}


def _case(V, k, m, nb=B):
    """bf16 rows (host, and device with NaN bits in the pad columns) and the E-step's inputs on both sides; made
    once per shape and shared, never modified."""
    key = (V, k, m, nb)
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(1000 * V + k)
    topics = rs.dirichlet(np.full(V, 0.1), k)
    X = np.zeros((nb, V))
    for i in range(nb):
        p = rs.dirichlet(np.full(k, 0.3)) @ topics
        X[i] = rs.multinomial(rs.poisson(m) + 1, p / p.sum())
    assert X.max() <= 256
    lam = rs.gamma(100.0, 0.01, (k, V)) + 50.0 * topics
    e_beta = torch.as_tensor(np.exp(digamma(lam) - digamma(lam.sum(1, keepdims=True))))
    alpha = torch.full((k,), 1.0 / k, dtype=torch.float64)
    gamma0 = torch.as_tensor(rs.gamma(100.0, 0.01, (nb, k)))
    xb = torch.as_tensor(X).to(torch.bfloat16)
    assert np.array_equal(xb.to(torch.float64).numpy(), X)
    clean = to_device_matrix(xb.to(DEV), V)
    xd = clean.clone()
    dp = int(xd.shape[1])
    if V < dp:
        xd.view(torch.int16)[:, V:] = 0x7fc0
    out = dict(V=V, k=k, dp=dp, X=X, xb=xb, xd=xd, clean=clean, e_beta=e_beta, alpha=alpha, gamma0=gamma0,
               dev=(e_beta.to(DEV), alpha.to(DEV), gamma0.to(DEV)))
    _cache[key] = out
    return out


def _reference(C, n):
    """The reference form on the first n documents (CPU f64), with its margin, and logphat's sum of |terms|."""
    key = ("ref", n)
    if key not in C:
        gam, ss, lph, sw, margin = LO.estep_reference(C["xb"][:n], None, C["V"], C["e_beta"], C["alpha"],
                                                      C["gamma0"][:n], with_margin=True)
        M = L.dirichlet_expectation(gam).abs().sum(0)
        C[key] = (gam.numpy(), ss.numpy(), lph.numpy(), sw.numpy(), margin, M.numpy())
    return C[key]


@pytest.mark.parametrize("V,k,m", SHAPES)
def test_estep_against_reference(V, k, m):
    C = _case(V, k, m)
    assert LO.kernel_supported(torch.bfloat16, C["dp"], k)
    e_beta, alpha, gamma0 = C["dev"]
    for n in (B, 15, 1):
        want_g, want_s, want_l, want_w, margin, M = _reference(C, n)
        assert margin >= 1e-9  # a shape that misses this gets another seed, never another bound
        gam, ss, lph, sw = LO.estep(C["xd"][:n], None, V, e_beta, alpha, gamma0[:n])
        torch.cuda.synchronize()
        assert gam.shape == (n, k) and ss.shape == (k, V) and lph.shape == (k,) and sw.shape == (n,)
        assert gam.dtype == ss.dtype == lph.dtype == torch.float64 and sw.dtype == torch.int32
        g, s, lp, w = gam.cpu().numpy(), ss.cpu().numpy(), lph.cpu().numpy(), sw.cpu().numpy()
        eg = np.abs(g - want_g) / np.abs(want_g)
        es = np.abs(s - want_s)[want_s != 0] / np.abs(want_s[want_s != 0])
        el = np.abs(lp - want_l) / M
        print(f"V={V} k={k} n={n}: sweeps {want_w.min()}..{want_w.max()} (differ: {int((w != want_w).sum())}), "
              f"margin {margin:.2e}, worst gamma {eg.max():.3e}, sstats {es.max() if es.size else 0.0:.3e}, "
              f"logphat {el.max():.3e}")
        assert np.array_equal(w, want_w)
        np.testing.assert_allclose(g, want_g, rtol=1e-10, atol=0)
        assert (np.abs(s - want_s) <= 1e-9 * np.abs(want_s)).all()  # a reference 0 is exactly 0
        assert (np.abs(lp - want_l) <= 1e-9 * M).all()
    w_all = _reference(C, B)[3]
    assert w_all.min() >= 1 and w_all.max() > w_all.min()  # documents that stop at different sweeps


def test_lds_budget_is_the_kernels():
    lib = LO._native.kernels()
    for dp in (16, 32, 64, 128, 256, 512, 1024):
        for k in (1, 2, 16, 17, 32, 33):
            assert int(lib.cml_lda_lds(dp, k)) == LO.lds_bytes(dp, k)


@pytest.mark.parametrize("V,k,m", [(6, 3, 12), (24, 10, 40), (100, 16, 120), (40, 17, 60)])
def test_pad_columns_are_masked(V, k, m):
    """NaN bits in the pad columns change nothing: the same bits as zero padding."""
    C = _case(V, k, m)
    assert C["dp"] > V and torch.isnan(C["xd"][:, V:].to(torch.float32)).all()
    e_beta, alpha, gamma0 = C["dev"]
    a = LO.estep(C["xd"], None, V, e_beta, alpha, gamma0)
    b = LO.estep(C["clean"], None, V, e_beta, alpha, gamma0)
    for u, v in zip(a, b):
        assert torch.equal(u, v) and torch.isfinite(u.to(torch.float64)).all()


def test_determinism_row_lists_and_infer():
    V, k, m = 24, 10, 40
    C = _case(V, k, m, nb=300)
    e_beta, alpha, gamma0 = C["dev"]
    rs = np.random.RandomState(5)
    rows = torch.as_tensor(np.sort(rs.choice(300, 141, replace=False))).to(DEV)
    a = LO.estep(C["xd"], rows, V, e_beta, alpha, gamma0[rows])
    again = LO.estep(C["xd"], rows, V, e_beta, alpha, gamma0[rows])
    packed = LO.estep(C["xd"][rows].contiguous(), None, V, e_beta, alpha, gamma0[rows])
    gi, si = LO.infer(C["xd"], rows, V, e_beta, alpha, gamma0[rows])
    torch.cuda.synchronize()
    for u, v, w in zip(a, again, packed):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert torch.equal(gi, a[0]) and torch.equal(si, a[3])
    assert int(a[3].min()) >= 1 and torch.isfinite(a[0]).all() and bool(a[1].any())
    # against the reference form on the device, through the same row list
    want = LO.estep_reference(C["xd"], rows, V, e_beta, alpha, gamma0[rows], with_margin=True)
    assert want[4] >= 1e-9
    assert torch.equal(want[3], a[3])
    np.testing.assert_allclose(a[0].cpu().numpy(), want[0].cpu().numpy(), rtol=1e-10)


def test_no_document_is_no_launch_and_wrong_rows_raise():
    C = _case(6, 3, 12)
    e_beta, alpha, gamma0 = C["dev"]
    gam, ss, lph, sw = LO.estep(C["xd"][:0], None, 6, e_beta, alpha, gamma0[:0])
    g2, s2 = LO.infer(C["xd"], torch.zeros(0, dtype=torch.int64, device=DEV), 6, e_beta, alpha, gamma0[:0])
    torch.cuda.synchronize()
    assert gam.shape == (0, 3) and ss.shape == (3, 6) and not ss.any() and lph.shape == (3,) and not lph.any()
    assert sw.shape == (0,) and g2.shape == (0, 3) and s2.shape == (0,)
    with pytest.raises(ValueError):
        LO.estep(C["xd"].to(torch.float32), None, 6, e_beta, alpha, gamma0)
    with pytest.raises(ValueError):
        LO.estep(C["xd"][:, :8], None, 6, e_beta, alpha, gamma0)  # not the kernels' layout
    with pytest.raises(ValueError):
        LO.infer(C["xb"], None, 6, e_beta, alpha, gamma0)  # host rows
    with pytest.raises(ValueError):
        LO.estep(C["xd"], None, 6, e_beta, alpha, gamma0[:5])


def test_digamma():
    """The kernel's psi against scipy: 64 ulp max(1, |psi|) = 1.4e-14 max(1, |psi|). About 20 roundings stand
    behind a value (at most 10 recurrence terms, the log, the series with remainder below 1e-15): a factor 3."""
    x = np.concatenate([np.logspace(-3, 7, 4001), [1.0 / 32, 1.0, 1.4616321449683623, 2.0, 100.0]])
    got = LO.digamma(torch.as_tensor(x, device=DEV)).cpu().numpy()
    want = digamma(x)
    ratio = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"digamma: worst |err| / max(1, |psi|) = {ratio.max():.3e} at x = {x[ratio.argmax()]:.6g}")
    assert (ratio <= 64 * 2.0 ** -52).all()


# ------------------------------------------------------------------------------------------------- estimator
@pytest.fixture(scope="module")
def spark():
    """A GPU session of this module's own, beside whichever session is active: a host session left active by
    another module would keep the frames on the CPU, where no kernel runs."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    s = SparkSession({"spark.master": "mi355x", "spark.app.name": "lda"})
    assert s.device.type == "cuda"
    yield s
    s.stop()


def _corpus(n, k=6, block=8, seed=1, length=40):
    """Planted blocks as in tests/test_lda_pic.py: document i draws its tokens almost only from block i mod k."""
    rs = np.random.RandomState(seed)
    V = k * block
    X = np.zeros((n, V), dtype=np.float32)
    for t in range(k):
        p = np.full(V, 0.01)
        p[t * block:(t + 1) * block] = 1.0
        idx = np.arange(t, n, k)
        X[idx] = rs.multinomial(length, p / p.sum(), size=len(idx))
    return torch.as_tensor(X), V


def _fitted(m, df):
    return (m.topicsMatrix().toArray(), np.array(m.estimatedDocConcentration()),
            m.transform(df)._column_data("topicDistribution").values.cpu().numpy(), m.logLikelihood(df))


def test_estimator_kernel_equals_reference(spark, monkeypatch):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import LDA
    x, V = _corpus(20_000)
    df = spark.createDataFrameFromTensors({"features": x.to(DEV).to(torch.bfloat16)})
    est = LDA(k=6, seed=7, maxIter=5, subsamplingRate=0.5)
    calls = []
    real = LO.estep

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(LO, "estep", counted)
    monkeypatch.delenv("CML_LDA_KERNEL", raising=False)
    fast = est.fit(df)
    assert len(calls) == 5
    got = _fitted(fast, df)
    assert fast.logPerplexity(df) == pytest.approx(-got[3] / float(20_000 * 40), rel=1e-12)
    del calls[:]
    monkeypatch.setenv("CML_LDA_KERNEL", "0")
    slow = est.fit(df)
    want = _fitted(slow, df)
    assert not calls
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=1e-9)
    assert got[0].shape == (V, 6) and got[2].shape == (20_000, 6)
    np.testing.assert_allclose(got[2].sum(1), 1.0, rtol=1e-12)
    assert np.isfinite(got[3]) and got[3] < 0


def test_longer_fit_recovers_the_planted_blocks(spark, monkeypatch):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import LDA
    monkeypatch.delenv("CML_LDA_KERNEL", raising=False)
    x, V = _corpus(20_000)
    df = spark.createDataFrameFromTensors({"features": x.to(DEV).to(torch.bfloat16)})
    m = LDA(k=6, seed=7, maxIter=40, subsamplingRate=0.5, learningOffset=8.0).fit(df)
    lam = m.topicsMatrix().toArray().T  # [k, V]
    norm = lam / lam.sum(1, keepdims=True)
    top = np.argsort(-norm, 1)[:, :8]
    blocks = [set((row // 8).tolist()) for row in top]
    assert all(len(b) == 1 for b in blocks)  # each topic = one planted block
    assert sorted(next(iter(b)) for b in blocks) == list(range(6))
    td = m.transform(df)._column_data("topicDistribution").values.cpu().numpy()
    lab = td.argmax(1)
    for t in range(6):
        _, cnt = np.unique(lab[t::6], return_counts=True)
        assert cnt.max() / cnt.sum() > 0.95


def test_other_columns_take_the_other_forms(spark, monkeypatch):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import LDA
    monkeypatch.delenv("CML_LDA_KERNEL", raising=False)

    def boom(*a, **k):
        raise AssertionError("outside the kernel's limits: another form is expected")
    monkeypatch.setattr(LO, "estep", boom)
    monkeypatch.setattr(LO, "infer", boom)
    seen = []
    real = LO.estep_reference

    def counted(*a, **k):
        seen.append(1)
        return real(*a, **k)
    monkeypatch.setattr(LO, "estep_reference", counted)
    wide = _corpus(600, k=6, block=100)[0]  # V = 600: padded width 1024
    narrow = torch.clamp(_corpus(600)[0], max=16.0)
    for feats in (wide.to(DEV).to(torch.bfloat16), narrow.to(torch.float8_e4m3fn)):
        del seen[:]
        df = spark.createDataFrameFromTensors({"features": feats})
        m = LDA(k=3, seed=7, maxIter=3, subsamplingRate=0.5).fit(df)
        assert len(seen) == 3
        td = m.transform(df)._column_data("topicDistribution").values
        assert td.shape == (600, 3) and np.isfinite(m.logLikelihood(df)) and np.isfinite(m.logPerplexity(df))
        assert len(seen) == 6
    for name in ("estep_reference", "kernel_enabled", "kernel_supported", "gather_rows", "row_sums"):
        monkeypatch.setattr(LO, name, boom)
    df = spark.createDataFrameFromTensors({"features": _corpus(600)[0].to(DEV)})  # f32: the dense form
    m = LDA(k=3, seed=7, maxIter=3, subsamplingRate=0.5).fit(df)
    assert m.transform(df)._column_data("topicDistribution").values.shape == (600, 3)
    assert np.isfinite(m.logLikelihood(df)) and np.isfinite(m.logPerplexity(df))


def test_fit_memory(spark, monkeypatch):
    """Peak allocation during fit stays below half of X (the f64 copy this replaces is four times X): the row
    sums' one widened chunk, per-row ids / draws / masks, the mini-batch's row list and gamma, and the
    per-workgroup partials; nothing of the size of X or of the mini-batch's rows."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import LDA
    monkeypatch.delenv("CML_LDA_KERNEL", raising=False)
    n, V = 1_000_000, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.empty(n, V, dtype=torch.bfloat16, device=DEV)
    rate = torch.full((1 << 16, V), 0.25, device=DEV)
    for st in range(0, n, 1 << 16):
        x[st:st + (1 << 16)] = torch.poisson(rate[:n - st], generator=g).to(torch.bfloat16)
    del rate
    df = spark.createDataFrameFromTensors({"features": x})
    est = LDA(k=10, seed=3, maxIter=3, subsamplingRate=0.05)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = est.fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    xbytes = x.numel() * x.element_size()
    print(f"fit peak rise {rise / n:.1f} B/row = {100.0 * rise / xbytes:.1f} % of X")
    assert rise < 0.5 * xbytes
    assert m.topicsMatrix().numRows == V and m.topicsMatrix().numCols == 10
