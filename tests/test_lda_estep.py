"""The reference form of the LDA E-step (``ops/lda_ops.py: estep_reference``) on low-precision CPU tensors, against
``ml.lda.e_step`` on the gathered, widened rows and against a per-document numpy loop, and the limits of K29.

Data: a planted-topic corpus. Topics ~ Dirichlet(0.1) over V terms, document mixtures ~ Dirichlet(0.3), length
~ Poisson(m) + 1, lambda = Gamma(100, 0.01) + 50 topics, alpha = 1 / k and gamma0 ~ Gamma(100, 0.01). Counts stay
small integers, so they are exact in bf16 (and the ones used for e4m3, at most 16, in e4m3). Every case asserts on
the reference that no active sweep's change lies within 1e-9 of the 1e-3 threshold: a document closer to it than
f64 reordering can resolve could legitimately stop one sweep apart in two correct evaluations.
"""
import numpy as np
import pytest
import torch
from scipy.special import digamma

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.lda import e_step
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import lda_ops as LO

RTOL = 1e-10  # the project's bound between two f64 evaluations of the E-step (tests/test_lda_pic.py)


def make_case(V, k, m, B, seed=0, cap=None):
    rs = np.random.RandomState(seed)
    topics = rs.dirichlet(np.full(V, 0.1), k)
    X = np.zeros((B, V))
    for i in range(B):
        p = rs.dirichlet(np.full(k, 0.3)) @ topics
        X[i] = rs.multinomial(rs.poisson(m) + 1, p / p.sum())
    if cap is not None:
        X = np.minimum(X, cap)
    lam = rs.gamma(100.0, 0.01, (k, V)) + 50.0 * topics
    e_beta = np.exp(digamma(lam) - digamma(lam.sum(1, keepdims=True)))
    return dict(X=X, e_beta=e_beta, alpha=np.full(k, 1.0 / k), gamma0=rs.gamma(100.0, 0.01, (B, k)))


def doc_loop(x, e_beta, alpha, g0):
    """One document, as Spark's variationalTopicInference runs it: (gamma, sstats term, sweeps)."""
    g = g0.copy()
    e = np.exp(digamma(g) - digamma(g.sum()))
    ph = e @ e_beta + 1e-100
    for it in range(1, 1001):
        last = g
        g = e * ((x / ph) @ e_beta.T) + alpha
        e = np.exp(digamma(g) - digamma(g.sum()))
        ph = e @ e_beta + 1e-100
        if not np.abs(g - last).mean() > 1e-3:
            break
    return g, np.outer(e, x / ph), it


@pytest.mark.parametrize("dtype,V,k,m,cap", [(torch.bfloat16, 24, 10, 40, None), (torch.bfloat16, 6, 3, 12, None),
                                             (torch.float8_e4m3fn, 24, 10, 40, 16), (torch.float8_e4m3fn, 16, 2, 8, 16)])
def test_reference_form_on_low_precision_rows(dtype, V, k, m, cap):
    C = make_case(V, k, m, 60, seed=3, cap=cap)
    assert C["X"].max() <= 256
    x = torch.as_tensor(C["X"]).to(torch.float32).to(dtype)
    assert np.array_equal(x.to(torch.float32).numpy(), C["X"])  # exact in this dtype
    rows = torch.as_tensor(np.array([0, 1, 2, 5, 7, 8, 13, 21, 22, 34, 55, 59]))
    e_beta, alpha = torch.as_tensor(C["e_beta"]), torch.as_tensor(C["alpha"])
    g0 = torch.as_tensor(C["gamma0"])[rows]
    gam, ss, lph, sw, margin = LO.estep_reference(x, rows, V, e_beta, alpha, g0, with_margin=True)
    assert margin >= 1e-9
    assert gam.shape == (12, k) and ss.shape == (k, V) and lph.shape == (k,) and sw.dtype == torch.int32
    # ml.lda.e_step on the gathered, widened rows
    g1, ss1, _, _ = e_step(torch.as_tensor(C["X"])[rows], e_beta, alpha, g0)
    np.testing.assert_allclose(gam.numpy(), g1.numpy(), rtol=RTOL)
    np.testing.assert_allclose(ss.numpy(), ss1.numpy(), rtol=RTOL)
    # the per-document loop
    ref_ss, ref_lp = np.zeros((k, V)), np.zeros(k)
    for i, r in enumerate(rows.tolist()):
        gi, si, it = doc_loop(C["X"][r], C["e_beta"], C["alpha"], C["gamma0"][r])
        np.testing.assert_allclose(gam[i].numpy(), gi, rtol=RTOL)
        assert int(sw[i]) == it
        ref_ss += si
        ref_lp += digamma(gi) - digamma(gi.sum())
    np.testing.assert_allclose(ss.numpy(), ref_ss, rtol=RTOL)
    np.testing.assert_allclose(lph.numpy(), ref_lp, rtol=RTOL)
    assert int(sw.min()) >= 1 and int(sw.max()) > int(sw.min())


def test_chunks_and_row_lists():
    V, k = 24, 10
    C = make_case(V, k, 40, 60, seed=3)
    x = torch.as_tensor(C["X"]).to(torch.bfloat16)
    e_beta, alpha, g0 = (torch.as_tensor(C[key]) for key in ("e_beta", "alpha", "gamma0"))
    one = LO.estep_reference(x, None, V, e_beta, alpha, g0, with_margin=True)
    assert one[4] >= 1e-9
    small = LO.estep_reference(x, None, V, e_beta, alpha, g0, chunk=7)
    listed = LO.estep_reference(x, torch.arange(60), V, e_beta, alpha, g0)
    for other in (small, listed):
        assert torch.equal(other[3], one[3])
        for a, b in zip(other[:3], one[:3]):
            np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=RTOL)
    for a, b in zip(listed, one[:4]):
        assert torch.equal(a, b)  # the same chunks: the same bits
    # columns past d are ignored
    wide = torch.cat([x, torch.full((60, 3), float("nan"), dtype=torch.bfloat16)], 1)
    for a, b in zip(LO.estep_reference(wide, None, V, e_beta, alpha, g0), one[:4]):
        assert torch.equal(a, b)
    none = LO.estep_reference(x, torch.zeros(0, dtype=torch.int64), V, e_beta, alpha, g0[:0])
    assert none[0].shape == (0, k) and not none[1].any() and not none[2].any() and none[3].shape == (0,)


def test_row_sums():
    C = make_case(16, 2, 8, 50, seed=1, cap=16)
    for dtype in (torch.bfloat16, torch.float8_e4m3fn, torch.float64):
        x = torch.as_tensor(C["X"]).to(torch.float32).to(dtype)
        s = LO.row_sums(x, 16, chunk=7)
        assert s.dtype == torch.float64 and np.array_equal(s.numpy(), C["X"].sum(1))
        assert np.array_equal(LO.row_sums(x, 5).numpy(), C["X"][:, :5].sum(1))


def test_limits():
    bf = torch.bfloat16
    assert LO.kernel_supported(bf, 512, 16) and not LO.kernel_supported(bf, 512, 17)
    assert LO.kernel_supported(bf, 256, 32) and not LO.kernel_supported(bf, 256, 33)
    assert not LO.kernel_supported(bf, 1024, 2)
    assert not LO.kernel_supported(torch.float8_e4m3fn, 256, 2)
    assert not LO.kernel_supported(bf, 16, 1)
    assert LO.kernel_supported(bf, 16, 2) and LO.kernel_supported(bf, 16, 32)
    assert not LO.kernel_supported(torch.float32, 64, 4)
    # the LDS sum behind them: inside 160 KB at both corners
    assert LO.lds_bytes(512, 16) == 141440 and LO.lds_bytes(256, 32) == 117504
    assert 0 < max(LO.lds_bytes(dp, k) for dp in (16, 32, 64, 128, 256, 512) for k in range(2, 33)) <= 160 * 1024


def test_kernel_switch(monkeypatch):
    monkeypatch.delenv("CML_LDA_KERNEL", raising=False)
    assert LO.kernel_enabled()
    monkeypatch.setenv("CML_LDA_KERNEL", "0")
    assert not LO.kernel_enabled()
