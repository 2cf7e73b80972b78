"""The variational E-step of online LDA: the reference form and the host wrappers of K29
(``_native/csrc/lda.hip``).

The caller (``ml/lda.py``) hands over ``e_beta = exp(E[log beta])`` f64 ``[k, d]``, the prior ``alpha`` f64
``[k]`` and, per listed document, the initial ``gamma0`` f64 ``[B, k]``. Per document x, in f64:

* ``e = exp(psi(gamma) - psi(sum gamma))``, ``phinorm_w = sum_j e_j beta_jw + 1e-100``
* one sweep: ``gamma' = alpha + e * sum_w (x_w / phinorm_w) beta_jw``, ``change = mean_j |gamma'_j - gamma_j|``,
  ``gamma <- gamma'``, then ``e`` and ``phinorm`` again
* the document stops after the sweep whose change is not ``> 1e-3``, at the latest after 1000 sweeps

and the E-step returns ``gamma`` ``[B, k]``, ``sstats`` ``[k, d]`` = ``sum_docs e_j x_w / phinorm_w`` (final ``e``
and ``phinorm``), ``logphat`` ``[k]`` = ``sum_docs (psi(gamma_j) - psi(sum gamma))`` and the sweep counts int32
``[B]``: ``ml.lda.e_step`` exactly, per document.

``estep_reference`` evaluates this in f64 torch chunk by chunk on any device and dtype (one chunk of the rows in
f64 at a time): the path of e4m3 rows and of bf16 rows outside the kernel's limits, and the oracle of the kernel.
``estep`` / ``infer`` are the gfx950 kernel for bf16 rows in the ``to_device_matrix`` layout (``kernel_supported``):
one launch reads every listed row once and sweeps it to convergence in LDS, a small second launch adds the
per-workgroup partials in workgroup order. ``CML_LDA_KERNEL=0`` keeps the estimator on the reference form.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from ._fused import check_matrix, env_enabled, gather_rows, ncu, row_list, widen  # gather_rows: a public name here

_native.register_kernel_sigs({
    "cml_lda_lds": (c_ll, [c_int, c_int]),
    "cml_lda_grid": (c_int, [c_ll, c_int, c_int, c_int]),
    "cml_lda_estep": (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_vp, c_ll, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int,
                              c_vp, c_int, c_int, c_vp]),
    "cml_lda_digamma": (c_int, [c_vp, c_vp, c_ll, c_vp]),
})

CHUNK = 8192
_TILE = 64


def kernel_enabled() -> bool:
    return env_enabled("CML_LDA_KERNEL")


def lds_bytes(dp: int, k: int) -> int:
    """LDS bytes of K29 (what ``cml_lda_lds`` returns), 0 outside the limits. With kp = k rounded up to 16:
    the f64 image of beta ``kp * max(dp, 32)``, the f64 ``e`` tile ``64 * (kp + 1)``, alpha ``kp`` and the
    logphat fold ``4 * kp`` doubles, plus the 64-document bf16 row tile ``64 * (dp + 8)`` values:
    ``8 * (kp * max(dp, 32) + 64 * (kp + 1) + 5 * kp) + 128 * (dp + 8)`` bytes. That is 141 440 B (138 KB) at
    k = 16, dp = 512 and 117 504 B (115 KB) at k = 32, dp = 256, inside one CU's 160 KB; k = 32 at dp = 512
    would need 211 KB, and dp = 1024 at kp = 16 266 KB."""
    if dp < 16 or dp > 512 or dp & (dp - 1) or k < 2 or k > 32 or (k > 16 and dp > 256):
        return 0
    kp = 16 if k <= 16 else 32
    b = 8 * (kp * max(dp, 32) + _TILE * (kp + 1) + 5 * kp) + 2 * _TILE * (dp + 8)
    return b if b <= 160 * 1024 else 0


def kernel_supported(dtype: torch.dtype, dp: int, k: int) -> bool:
    """Whether K29 takes rows of this dtype and padded width with k topics (anything else: the reference form).
    bf16 rows of padded width 16..512 with ``2 <= k <= 16``, and ``17 <= k <= 32`` up to width 256: see
    ``lds_bytes`` for the sum that sets these limits."""
    return dtype == torch.bfloat16 and lds_bytes(int(dp), int(k)) > 0


# ---------------------------------------------------------------------------------------------- reference form
def row_sums(x: torch.Tensor, d: int, chunk: int = 1 << 16) -> torch.Tensor:
    """f64 ``[n]`` row sums over the first ``d`` columns, one widened chunk at a time."""
    n = int(x.shape[0])
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    for st in range(0, n, chunk):
        out[st:st + chunk] = widen(x[st:st + chunk, :d]).sum(1)
    return out


def estep_reference(x: torch.Tensor, rows: Optional[torch.Tensor], d: int, e_beta: torch.Tensor, alpha: torch.Tensor,
                    gamma0: torch.Tensor, chunk: int = CHUNK, with_margin: bool = False):
    """``(gamma [B, k], sstats [k, d], logphat [k], sweeps int32 [B])`` of the listed rows (``rows`` an ascending
    int64 index tensor, None for all rows; ``gamma0`` aligned with it). ``x`` ``[n, >= d]`` of any dtype and
    device. ``with_margin`` adds the smallest ``|change - 1e-3|`` seen while a document was active (a float)."""
    from ..ml.lda import dirichlet_expectation, e_step_counted
    dev = x.device
    e_beta = e_beta.to(device=dev, dtype=torch.float64)
    alpha = alpha.to(device=dev, dtype=torch.float64)
    gamma0 = gamma0.to(device=dev, dtype=torch.float64)
    k = int(e_beta.shape[0])
    B = int(x.shape[0]) if rows is None else int(rows.shape[0])
    if gamma0.shape != (B, k) or e_beta.shape[1] != d:
        raise ValueError("lda estep: gamma0 [B, k] and e_beta [k, d] do not fit the rows")
    gamma = torch.empty(B, k, dtype=torch.float64, device=dev)
    sweeps = torch.zeros(B, dtype=torch.int32, device=dev)
    sstats = torch.zeros(k, d, dtype=torch.float64, device=dev)
    logphat = torch.zeros(k, dtype=torch.float64, device=dev)
    margin = float("inf")
    for st in range(0, B, chunk):
        if rows is None:
            v = widen(x[st:st + chunk, :d])
        else:
            v = gather_rows(x, rows[st:st + chunk].to(dev), d)
        g, ss, _, _, sw, mg = e_step_counted(v, e_beta, alpha, gamma0[st:st + chunk], with_margin=with_margin)
        gamma[st:st + chunk] = g
        sweeps[st:st + chunk] = sw
        sstats += ss
        logphat += dirichlet_expectation(g).sum(0)
        if with_margin:
            margin = min(margin, float(mg))
    out = (gamma, sstats, logphat, sweeps)
    return out + (margin,) if with_margin else out


# ---------------------------------------------------------------------------------------------------- kernel
def _launch(xd, rows, d, e_beta, alpha, gamma0, fit: bool, what: str):
    if not torch.is_tensor(xd) or xd.dim() != 2:
        raise ValueError(f"{what}: rows must be a 2-d tensor")
    k = int(e_beta.shape[0])
    dp = int(xd.shape[1])
    check_matrix(xd, d, lambda dtype, dp: (kernel_supported(dtype, dp, k) and e_beta.shape[1] == d
                                           and alpha.shape == (k,)), what,
                 "16..512, with e_beta [k, d], alpha [k] and k inside the kernel's limits")
    n, dev = int(xd.shape[0]), xd.device
    if rows is not None:
        rows = row_list(rows, dev, what)
    B = n if rows is None else int(rows.shape[0])
    if gamma0.shape != (B, k):
        raise ValueError(f"{what}: gamma0 must be [B, k]")
    gamma = torch.zeros(B, k, dtype=torch.float64, device=dev)
    sweeps = torch.zeros(B, dtype=torch.int32, device=dev)
    out = torch.zeros(k * d + k, dtype=torch.float64, device=dev) if fit else None
    if B:
        kp = 16 if k <= 16 else 32
        tab = torch.zeros(kp, dp, dtype=torch.float64, device=dev)
        tab[:k, :d] = e_beta.to(device=dev, dtype=torch.float64)
        al = torch.zeros(kp, dtype=torch.float64, device=dev)
        al[:k] = alpha.to(device=dev, dtype=torch.float64)
        g0 = gamma0.to(device=dev, dtype=torch.float64).contiguous()
        lib, cus = _native.kernels(), ncu(dev)
        grid = int(lib.cml_lda_grid(B, dp, k, cus))
        part = torch.empty(grid * (kp * dp + kp), dtype=torch.float64, device=dev) if fit else None
        _native.check(lib.cml_lda_estep(xd.data_ptr(), n, dp, d, k, _native.ptr(rows), B, tab.data_ptr(),
                                        al.data_ptr(), g0.data_ptr(), gamma.data_ptr(), sweeps.data_ptr(),
                                        _native.ptr(part), grid, _native.ptr(out), 1 if fit else 0, cus,
                                        torch.cuda.current_stream(dev).cuda_stream), what)
    return gamma, sweeps, out


def estep(xd: torch.Tensor, rows: Optional[torch.Tensor], d: int, e_beta: torch.Tensor, alpha: torch.Tensor,
          gamma0: torch.Tensor):
    """K29, fit form: ``(gamma, sstats, logphat, sweeps)`` as ``estep_reference`` returns them. All arithmetic
    after the exact bf16 -> f64 widening is f64 (the products on the f64 MFMA); pad columns are masked by ``d``.
    No atomics, no host read; two calls return the same bits."""
    gamma, sweeps, out = _launch(xd, rows, d, e_beta, alpha, gamma0, True, "lda estep")
    k = int(e_beta.shape[0])
    return gamma, out[:k * d].view(k, d), out[k * d:], sweeps


def infer(xd: torch.Tensor, rows: Optional[torch.Tensor], d: int, e_beta: torch.Tensor, alpha: torch.Tensor,
          gamma0: torch.Tensor):
    """K29 without the statistics: ``(gamma, sweeps)``, bit for bit the fit form's."""
    gamma, sweeps, _ = _launch(xd, rows, d, e_beta, alpha, gamma0, False, "lda infer")
    return gamma, sweeps


def digamma(t: torch.Tensor) -> torch.Tensor:
    """The kernel's device psi on an f64 device tensor (for testing)."""
    if not t.is_cuda or t.dtype != torch.float64:
        raise ValueError("lda digamma: an f64 device tensor is expected")
    t = t.contiguous()
    out = torch.empty_like(t)
    _native.check(_native.kernels().cml_lda_digamma(t.data_ptr(), out.data_ptr(), t.numel(),
                                                    torch.cuda.current_stream(t.device).cuda_stream), "lda_digamma")
    return out
