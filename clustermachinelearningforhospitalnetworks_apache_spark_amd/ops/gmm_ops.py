"""One E-step of a full-covariance Gaussian mixture: the reference form and the host wrappers of K28
(``_native/csrc/gmm.hip``).

The caller (``ml/gmm.py``) hands over, per component j, ``A_j = L_j^-1`` (``L_j`` the Cholesky factor of the
covariance, so ``A_j`` is lower triangular), the mean ``mu_j`` and the constant
``c_j = log(max(pi_j, 1e-300)) - (d log 2pi + 2 sum log diag L_j) / 2``. Per row, in f64:

* ``z_j = A_j (x - mu_j)`` (the subtraction first), ``lp_j = c_j - |z_j|^2 / 2``
* ``lse`` the max-subtracted log-sum-exp of ``lp`` over j, ``r_j = w exp(lp_j - lse)``

and the E-step returns ``stats`` f64 ``[k, 1 + d + d*d]`` = ``[S0_j | S1_j | S2_j]`` (``sum r``, ``sum r x``,
``sum r x x^T``; S2 in full and exactly symmetric) and ``tail`` f64 ``[2]`` = ``[sum w lse, sum w]``: the message
the fit all-reduces once per iteration.

``estep_reference`` / ``predict_reference`` evaluate this in f64 torch chunk by chunk on any device and dtype
(no copy of the rows, no n x k or n x d temporary): the path of e4m3 rows, d > 32 and k past the kernel's
limits, and the oracle of the kernel. ``estep`` / ``predict`` are the gfx950 kernel for bf16 rows in the
``to_device_matrix`` layout (``kernel_supported``): one launch reads every row once, a small second launch adds
the per-workgroup partials in workgroup order. ``CML_GMM_KERNEL=0`` keeps the estimator on the reference form.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from ._fused import check_matrix, env_enabled, gather_rows, ncu, widen  # gather_rows: a public name here

_native.register_kernel_sigs({
    "cml_gmm_lds": (c_ll, [c_int, c_int]),
    "cml_gmm_grid": (c_int, [c_ll, c_int, c_int, c_int, c_int]),
    "cml_gmm_estep": (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp]),
    "cml_gmm_predict": (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp]),
})

CHUNK = 1 << 16


def kernel_enabled() -> bool:
    return env_enabled("CML_GMM_KERNEL")


def kernel_supported(dtype: torch.dtype, dp: int, k: int) -> bool:
    """Whether K28 takes rows of this dtype and padded width with k components (anything else: the reference
    form). bf16 rows only; ``2 <= k <= 32`` at dp = 16 and ``2 <= k <= 16`` at dp = 32: the f64 ``A_j^T`` tables
    (k dp^2 values, at most 128 KB), ``mu``, ``c``, the 2048-value f64 row tile and the ``[rows, k]``
    responsibility tile together stay inside one CU's 160 KB of LDS (158 KB at dp = 32, k = 16)."""
    if dtype != torch.bfloat16:
        return False
    return (dp == 16 and 2 <= k <= 32) or (dp == 32 and 2 <= k <= 16)


# ---------------------------------------------------------------------------------------------- reference form
def _params(A, mu, c, dev):
    A = torch.as_tensor(np.asarray(A, dtype=np.float64), device=dev)
    mu = torch.as_tensor(np.asarray(mu, dtype=np.float64), device=dev)
    c = torch.as_tensor(np.asarray(c, dtype=np.float64), device=dev)
    return A, mu, c


def _chunk_lp(v, A, mu, c):
    """[rows, k] lp of one widened chunk; one ``rows x d`` temporary per component."""
    lp = torch.empty(v.shape[0], A.shape[0], dtype=torch.float64, device=v.device)
    for j in range(A.shape[0]):
        z = (v - mu[j]) @ A[j].T
        lp[:, j] = c[j] - 0.5 * (z * z).sum(1)
    return lp


def estep_reference(x: torch.Tensor, d: int, weights: Optional[torch.Tensor], A, mu, c, chunk: int = CHUNK):
    """``(stats, tail)`` of this rank's rows. ``x`` ``[n, >= d]`` of any dtype (columns past ``d`` are ignored),
    ``weights`` f64 ``[n]`` or None, ``A`` ``[k, d, d]``, ``mu`` ``[k, d]``, ``c`` ``[k]``. No host read."""
    n, dev = int(x.shape[0]), x.device
    A, mu, c = _params(A, mu, c, dev)
    k = int(A.shape[0])
    S0 = torch.zeros(k, dtype=torch.float64, device=dev)
    S1 = torch.zeros(k, d, dtype=torch.float64, device=dev)
    S2 = torch.zeros(k, d, d, dtype=torch.float64, device=dev)
    tail = torch.zeros(2, dtype=torch.float64, device=dev)
    for st in range(0, n, chunk):
        v = widen(x[st:st + chunk, :d])
        lp = _chunk_lp(v, A, mu, c)
        lse = torch.logsumexp(lp, 1)
        r = torch.exp(lp - lse[:, None])
        if weights is None:
            tail[0] += lse.sum()
            tail[1] += float(v.shape[0])
        else:
            w = weights[st:st + chunk].to(device=dev, dtype=torch.float64)
            r = r * w[:, None]
            tail[0] += (w * lse).sum()
            tail[1] += w.sum()
        S0 += r.sum(0)
        S1 += r.T @ v
        for j in range(k):
            S2[j] += (r[:, j:j + 1] * v).T @ v
    low = torch.tril(S2)
    S2 = low + torch.tril(S2, -1).transpose(1, 2)  # one triangle, mirrored: symmetric bit for bit
    return torch.cat([S0[:, None], S1, S2.reshape(k, d * d)], 1), tail


def predict_reference(x: torch.Tensor, d: int, weights: Optional[torch.Tensor], A, mu, c, chunk: int = CHUNK):
    """``(prob f64 [n, k], label int32 [n])``: ``prob = exp(lp - lse)``, ``label`` the lowest index among the
    maxima of ``lp``. ``weights`` is accepted for the common signature and not used."""
    n, dev = int(x.shape[0]), x.device
    A, mu, c = _params(A, mu, c, dev)
    k = int(A.shape[0])
    prob = torch.empty(n, k, dtype=torch.float64, device=dev)
    label = torch.empty(n, dtype=torch.int32, device=dev)
    ar = torch.arange(k, device=dev)
    for st in range(0, n, chunk):
        lp = _chunk_lp(widen(x[st:st + chunk, :d]), A, mu, c)
        prob[st:st + chunk] = torch.exp(lp - torch.logsumexp(lp, 1)[:, None])
        top = lp == lp.max(1, keepdim=True).values
        label[st:st + chunk] = torch.where(top, ar, torch.full_like(ar, k)).min(1).values.to(torch.int32)
    return prob, label


def column_moments(x: torch.Tensor, d: int, weights: Optional[torch.Tensor], chunk: int = CHUNK) -> torch.Tensor:
    """f64 ``[1 + 2d]`` = ``[sum w | sum w x | sum w x^2]`` by chunked sums (no n x d f64 product)."""
    dev = x.device
    out = torch.zeros(1 + 2 * d, dtype=torch.float64, device=dev)
    for st in range(0, int(x.shape[0]), chunk):
        v = widen(x[st:st + chunk, :d])
        if weights is None:
            out[0] += float(v.shape[0])
            out[1:1 + d] += v.sum(0)
            out[1 + d:] += (v * v).sum(0)
        else:
            w = weights[st:st + chunk].to(device=dev, dtype=torch.float64)
            wv = w[:, None] * v
            out[0] += w.sum()
            out[1:1 + d] += wv.sum(0)
            out[1 + d:] += (wv * v).sum(0)
    return out


# ---------------------------------------------------------------------------------------------------- kernel
def _check(xd: torch.Tensor, d: int, k: int, what: str):
    check_matrix(xd, d, lambda dtype, dp: kernel_supported(dtype, dp, k), what,
                 "16 or 32, with k inside the kernel's limits")


def _tables(A, mu, c, d: int, dp: int, dev) -> torch.Tensor:
    """``[A_j^T in 16-column blocks | mu | c]`` zero padded to dp, f64 on the device: ``Bt[j][cb][t][col] =
    A_j[16 cb + col][t]``, so that the 32 lanes of a half wave read 32 consecutive doubles."""
    A = np.asarray(A, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    k = A.shape[0]
    if A.shape != (k, d, d) or mu.shape != (k, d) or c.shape != (k,):
        raise ValueError("gmm tables: A [k, d, d], mu [k, d] and c [k] do not fit")
    Ap = np.zeros((k, dp, dp))
    Ap[:, :d, :d] = np.tril(A)
    mp = np.zeros((k, dp))
    mp[:, :d] = mu
    bt = Ap.reshape(k, dp // 16, 16, dp).transpose(0, 1, 3, 2)
    return torch.as_tensor(np.concatenate([bt.reshape(-1), mp.reshape(-1), c]), device=dev)


def estep(xd: torch.Tensor, d: int, weights: Optional[torch.Tensor], A, mu, c):
    """K28, fit form: ``(stats, tail)`` as ``estep_reference`` returns them. All arithmetic after the exact
    bf16 -> f64 widening is f64 (the products on the f64 MFMA); pad columns are masked by ``d``. No atomics;
    two calls return the same bits."""
    k = int(np.asarray(c).shape[0])
    _check(xd, d, k, "gmm estep")
    n, dp, dev = int(xd.shape[0]), int(xd.shape[1]), xd.device
    cs = 1 + d + d * d
    out = torch.zeros(k * cs + 2, dtype=torch.float64, device=dev)
    if n:
        if weights is not None:
            weights = weights.to(device=dev, dtype=torch.float64).contiguous()
            if weights.shape[0] != n:
                raise ValueError("gmm estep: the weights differ in length from the rows")
        tab = _tables(A, mu, c, d, dp, dev)
        lib, cus = _native.kernels(), ncu(dev)
        grid = int(lib.cml_gmm_grid(n, dp, k, cus, 0))
        part = torch.empty(grid * (k * cs + 2), dtype=torch.float64, device=dev)
        _native.check(lib.cml_gmm_estep(xd.data_ptr(), n, dp, d, k, _native.ptr(weights), tab.data_ptr(),
                                        part.data_ptr(), grid, out.data_ptr(), cus,
                                        torch.cuda.current_stream(dev).cuda_stream), "gmm_estep")
    return out[:k * cs].view(k, cs), out[k * cs:]


def predict(xd: torch.Tensor, d: int, A, mu, c):
    """K28, predict form: ``(prob f64 [n, k], label int32 [n])`` as ``predict_reference`` returns them."""
    k = int(np.asarray(c).shape[0])
    _check(xd, d, k, "gmm predict")
    n, dp, dev = int(xd.shape[0]), int(xd.shape[1]), xd.device
    prob = torch.empty(n, k, dtype=torch.float64, device=dev)
    label = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        tab = _tables(A, mu, c, d, dp, dev)
        _native.check(_native.kernels().cml_gmm_predict(xd.data_ptr(), n, dp, d, k, tab.data_ptr(),
                                                        prob.data_ptr(), label.data_ptr(), ncu(dev),
                                                        torch.cuda.current_stream(dev).cuda_stream), "gmm_predict")
    return prob, label
