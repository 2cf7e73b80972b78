"""``ops/aft_ops.py`` on the CPU: the chunked f64 reference form of the AFT loss and gradient against torch autograd of
``sum l`` on the widened rows, for bf16, e4m3 and f32 rows, and the limits and argument checks of the kernel wrappers.

Data: ``x = randn`` in the stored dtype, ``beta = 0.3 randn / sqrt(d)``, ``logt = x . beta + 0.7 log(Exp(1))``, 30 % of
the rows censored with t scaled by U(0.3, 1); evaluated at a perturbed ``coef`` with ``b = 0.8``, ``sigma = 0.9``.

Bounds (``u = 2^-53``):
* gradient: ``|g - g_autograd|[i] <= 2 (n + 2) u (|X|^T |r|)[i]``: an n-term f64 sum on both sides;
* ``sum r, sum s, sum l``: within ``(2 (n + 2) + 64) u`` times the sum over the rows of the absolute leaf terms
  ``(delta + ee) / sigma``, ``delta + (delta + ee) |eps|``, ``delta |ls| + delta |eps| + ee``: a row's addend is a
  handful of roundings and one ``exp`` (64 covers them), the n-term sum adds ``(n + 2) u`` on each side;
* eta of ``rows_reference``: ``<= 2 (d + 2) u (sum_i |x_i beta_i| + |b|)``.
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import aft_ops as AO

U = 2.0 ** -53
DTYPES = {"bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn, "f32": torch.float32}


def make_case(n, d, dtype, seed):
    """Rows in the stored dtype, log times, censors and the parameters of the module docstring (CPU, f64)."""
    rs = np.random.RandomState(seed)
    x = torch.as_tensor(rs.randn(n, d)).to(torch.float32)
    x = (x.to(torch.bfloat16) if dtype == torch.float8_e4m3fn else x).to(dtype)
    xw = AO.widen(x)
    beta = 0.3 * rs.randn(d) / np.sqrt(d)
    t = np.exp(xw.numpy() @ beta + 0.7 * np.log(rs.exponential(1.0, n)))
    cens = rs.rand(n) < 0.3
    t = np.where(cens, t * rs.uniform(0.3, 1.0, n), t)
    coef = np.r_[beta + 0.05 * rs.randn(d) / np.sqrt(d), 0.8, np.log(0.9)]
    return x, torch.as_tensor(np.log(t)), torch.as_tensor((~cens).astype(np.float64)), torch.as_tensor(coef)


def leaf_sums(t, delta, ls):
    """Per scalar of the message, the sum over the rows of the absolute leaf terms of its formula."""
    sigma, eps, ee = float(np.exp(float(ls))), t["eps"].abs(), t["ee"]
    return torch.stack([((delta + ee) / sigma).sum(), (delta + (delta + ee) * eps).sum(),
                        (delta * abs(float(ls)) + delta * eps + ee).sum()])


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("chunk", [7, 8192])
@pytest.mark.parametrize("n", [50, 1, 0])
@pytest.mark.parametrize("d", [1, 15, 17, 40])
def test_loss_grad_reference_against_autograd(d, n, chunk, name):
    x, logt, delta, coef = make_case(n, d, DTYPES[name], 100 * d + n)
    got = AO.loss_grad_reference(x, d, logt, delta, coef, chunk=chunk)
    assert got.shape == (d + 3,) and got.dtype == torch.float64
    if n == 0:
        assert not got.any()
        return
    xw = AO.widen(x)
    p = coef.clone().requires_grad_(True)
    t = AO.row_terms(xw @ p[:d] + p[d], logt, delta, p[d + 1])
    loss = t["l"].sum()
    loss.backward()
    t = {k: v.detach() for k, v in t.items()}
    assert float(t["eps"].min()) > -20.0 and float(t["eps"].max()) < 5.0
    gb = 2.0 * (n + 2) * U * (xw.abs().T @ t["r"].abs())
    assert ((got[:d] - p.grad[:d]).abs() <= gb).all(), ((got[:d] - p.grad[:d]).abs() / gb).max()
    want = torch.stack([p.grad[d], p.grad[d + 1], loss.detach()])
    sb = (2.0 * (n + 2) + 64.0) * U * leaf_sums(t, delta, coef[d + 1])
    assert ((got[d:] - want).abs() <= sb).all(), (got[d:], want, sb)


def test_reference_ignores_columns_past_d_and_takes_any_chunk():
    d, n = 17, 50
    x, logt, delta, coef = make_case(n, d, torch.bfloat16, 7)
    wide = torch.full((n, d + 7), float("nan"), dtype=torch.bfloat16)
    wide[:, :d] = x
    a = AO.loss_grad_reference(x, d, logt, delta, coef)
    assert torch.equal(a, AO.loss_grad_reference(wide, d, logt, delta, coef))
    assert torch.equal(AO.rows_reference(x, d, coef, chunk=7), AO.rows_reference(wide, d, coef, chunk=7))
    assert torch.isfinite(a).all()
    # another chunk is another order of the same sums: within the bounds of the module docstring, not the same bits
    b = AO.loss_grad_reference(x, d, logt, delta, coef, chunk=7)
    xw = AO.widen(x)
    t = AO.row_terms(xw @ coef[:d] + coef[d], logt, delta, coef[d + 1])
    assert ((a[:d] - b[:d]).abs() <= 2.0 * (n + 2) * U * (xw.abs().T @ t["r"].abs())).all()
    assert ((a[d:] - b[d:]).abs() <= (2.0 * (n + 2) + 64.0) * U * leaf_sums(t, delta, coef[d + 1])).all()


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("d", [1, 15, 17, 40])
def test_rows_reference(d, name):
    for n in (50, 1, 0):
        x, _, _, coef = make_case(n, d, DTYPES[name], 100 * d + n)
        xw = AO.widen(x)
        for chunk in (7, None):
            eta = AO.rows_reference(x, d, coef, chunk=chunk)
            assert eta.shape == (n,) and eta.dtype == torch.float64
            bound = 2.0 * (d + 2) * U * (xw.abs() @ coef[:d].abs() + coef[d].abs())
            assert ((eta - (xw @ coef[:d] + coef[d])).abs() <= bound).all()


def test_row_terms_are_the_formulas():
    eta = torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64)
    logt = torch.tensor([0.1, 0.4, -3.0], dtype=torch.float64)
    delta = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)
    ls = float(np.log(0.9))
    t = AO.row_terms(eta, logt, delta, ls)
    sigma = torch.exp(torch.tensor(ls, dtype=torch.float64))
    eps = (logt - eta) / sigma
    ee = torch.exp(eps)
    assert torch.equal(t["r"], (delta - ee) / sigma)
    assert torch.equal(t["s"], delta + (delta - ee) * eps)
    assert torch.equal(t["l"], delta * ls - delta * eps + ee)


def test_kernel_limits():
    for dp in (16, 32, 64, 128, 256, 512):
        assert AO.kernel_supported(torch.bfloat16, dp)
        assert not AO.kernel_supported(torch.float8_e4m3fn, dp) and not AO.kernel_supported(torch.float32, dp)
    assert not AO.kernel_supported(torch.bfloat16, 1024) and not AO.kernel_supported(torch.bfloat16, 8)
    # the tile at a pitch of dp + 16 bf16, beta, the tile's r, the two folds; two launches of the widest fit a CU
    assert AO.lds_bytes(512) == 64 * 528 * 2 + 512 * 8 + 64 * 8 + 512 * 8 + 64 * 3 * 8 == 77824
    assert 2 * AO.lds_bytes(512) <= 160 * 1024
    assert AO.lds_bytes(16) == 10368


def test_argument_errors():
    d, n = 17, 50
    x, logt, delta, coef = make_case(n, d, torch.bfloat16, 3)
    for bad in (lambda: AO.loss_grad_reference(x, d, logt[:-1], delta, coef),
                lambda: AO.loss_grad_reference(x, d, logt, delta[:-1], coef),
                lambda: AO.loss_grad_reference(x, d, logt, delta, coef[:-1]),
                lambda: AO.loss_grad_reference(x, d + 1, logt, delta, coef),
                lambda: AO.loss_grad_reference(x[0], d, logt, delta, coef),
                lambda: AO.rows_reference(x, d, coef[:-1]),
                lambda: AO.loss_grad(x, d, logt, delta, coef),            # host rows
                lambda: AO.loss_grad(x, d, None, delta, coef),
                lambda: AO.rows(x, d, coef),
                lambda: AO.rows(x, d, coef, logt=logt),                    # log times without censors
                lambda: AO.rows(x[0], d, coef)):
        with pytest.raises(ValueError):
            bad()
