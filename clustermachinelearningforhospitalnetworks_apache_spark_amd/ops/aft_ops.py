"""Loss and gradient of the Weibull accelerated-failure-time model: the reference form and the host wrappers of K35
(``_native/csrc/aft.hip``).

For a row with ``logt = log t``, censor ``delta`` in {0, 1} and the parameters ``coef = (beta[0..d), b, ls)`` with
``sigma = exp(ls)``, in f64 after the exact widening of the stored row:

* ``eta = x . beta + b``
* ``eps = (logt - eta) / sigma``, ``ee = exp(eps)``
* ``r = (delta - ee) / sigma`` (d loss / d eta), ``s = delta + (delta - ee) * eps`` (d loss / d ls)
* ``l = delta * ls - delta * eps + ee`` (the row's negative log-likelihood)

One L-BFGS evaluation of ``AFTSurvivalRegression`` needs ``[X^T r | sum r | sum s | sum l]``, ``d + 3`` doubles per
shard: the caller all-reduces them.

``row_terms`` is the per-row arithmetic in plain f64 torch; ``loss_grad_reference`` / ``rows_reference`` evaluate it
chunk by chunk on any device and stored dtype (one chunk of ``CHUNK`` rows in f64 at a time, never an ``n x d``
copy): the path of every column the kernel does not take and the oracle of the kernel. ``loss_grad`` / ``rows`` are
the gfx950 kernel for bf16 device rows in the ``to_device_matrix`` layout of padded width 16..512
(``kernel_supported``): one launch reads every row once, a small second launch adds the slabs in slab order.
``CML_AFT_KERNEL=0`` keeps the estimator on the reference form.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from ._fused import check_matrix, env_enabled, ncu, widen

_native.register_kernel_sigs({
    "cml_aft_slabs": (c_int, [c_ll, c_int, c_int]),
    "cml_aft_part": (c_ll, [c_int]),
    "cml_aft_lds": (c_ll, [c_int]),
    "cml_aft_pass": (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int, c_vp]),
})

CHUNK = 8192
MIN_DP, MAX_DP = 16, 512
_TILE = 64     # rows of a staged tile
_FOLD = 512    # doubles of the kernel's gradient fold


def kernel_enabled() -> bool:
    return env_enabled("CML_AFT_KERNEL")


def kernel_supported(dtype: torch.dtype, dp: int, arg=None) -> bool:
    """Whether K35 takes rows of this dtype and padded width (anything else: the reference form). ``arg`` is the
    place of the other modules' limit (k, the factor size) in ``_fused.use_kernel``; K35 has none."""
    dp = int(dp)
    return dtype == torch.bfloat16 and MIN_DP <= dp <= MAX_DP and dp & (dp - 1) == 0


def lds_bytes(dp: int) -> int:
    """Bytes of LDS of a launch at the padded width ``dp``: the 64-row tile at a pitch of ``dp + 16`` bf16, beta as
    f64, the tile's ``r``, the gradient fold and the fold of the three scalars."""
    dp = int(dp)
    return 2 * _TILE * (dp + 16) + 8 * dp + 8 * _TILE + 8 * _FOLD + 8 * 3 * _TILE


# ---------------------------------------------------------------------------------------------- reference form
def row_terms(eta: torch.Tensor, logt: torch.Tensor, delta: torch.Tensor, ls) -> dict:
    """The f64 per-row terms ``r, s, l`` (and ``eps, ee``) at the linear predictor ``eta``. The operations and their
    order are those of ``aft_row_terms`` in ``aft.hip``; ``sigma = exp(ls)`` is made on the device of ``eta``."""
    ls = torch.as_tensor(ls, dtype=torch.float64).to(eta.device).reshape(())  # a float would become f32 otherwise
    sigma = torch.exp(ls)
    eps = (logt - eta) / sigma
    ee = torch.exp(eps)
    return {"eps": eps, "ee": ee,
            "r": (delta - ee) / sigma,
            "s": delta + (delta - ee) * eps,
            "l": delta * ls - delta * eps + ee}


def _coef(coef, d: int, dev, what: str) -> torch.Tensor:
    c = torch.as_tensor(coef, dtype=torch.float64).to(dev).reshape(-1).contiguous()
    if c.numel() != d + 2:
        raise ValueError(f"{what}: {c.numel()} parameters, d = {d} needs {d + 2} (beta, b, log sigma)")
    return c


def _check_rows(x, d: int, logt, delta, what: str) -> int:
    if not torch.is_tensor(x) or x.dim() != 2 or d < 0 or x.shape[1] < d:
        raise ValueError(f"{what}: rows [n, >= d] are expected")
    n = int(x.shape[0])
    for v in (logt, delta):
        if v is not None and (not torch.is_tensor(v) or v.numel() != n):
            raise ValueError(f"{what}: one log time and censor per row are expected")
    return n


def _vec(v: torch.Tensor, dev) -> torch.Tensor:
    return v.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()


def loss_grad_reference(x: torch.Tensor, d: int, logt: torch.Tensor, delta: torch.Tensor, coef,
                        chunk: Optional[int] = None) -> torch.Tensor:
    """``[X^T r | sum r | sum s | sum l]``, ``d + 3`` doubles, of the rows ``x`` ``[n, >= d]`` (any dtype and device)
    at ``coef`` = (beta, b, log sigma): one widened chunk of rows at a time."""
    d = int(d)
    n, dev = _check_rows(x, d, logt, delta, "aft loss_grad"), x.device
    if logt is None or delta is None:
        raise ValueError("aft loss_grad: one log time and censor per row are expected")
    chunk = int(CHUNK if chunk is None else chunk)
    c = _coef(coef, d, dev, "aft loss_grad")
    logt, delta = _vec(logt, dev), _vec(delta, dev)
    out = torch.zeros(d + 3, dtype=torch.float64, device=dev)
    for st in range(0, n, chunk):
        en = min(n, st + chunk)
        xw = widen(x[st:en, :d])
        t = row_terms(xw @ c[:d] + c[d], logt[st:en], delta[st:en], c[d + 1])
        out[:d] += xw.T @ t["r"]
        out[d:] += torch.stack([t["r"].sum(), t["s"].sum(), t["l"].sum()])
    return out


def rows_reference(x: torch.Tensor, d: int, coef, chunk: Optional[int] = None) -> torch.Tensor:
    """f64 ``eta`` ``[n]`` of the rows ``x`` ``[n, >= d]`` of any dtype and device."""
    d = int(d)
    n, dev = _check_rows(x, d, None, None, "aft rows"), x.device
    chunk = int(CHUNK if chunk is None else chunk)
    c = _coef(coef, d, dev, "aft rows")
    eta = torch.empty(n, dtype=torch.float64, device=dev)
    for st in range(0, n, chunk):
        en = min(n, st + chunk)
        eta[st:en] = widen(x[st:en, :d]) @ c[:d] + c[d]
    return eta


# ---------------------------------------------------------------------------------------------------- kernel
def _launch(xd, d, logt, delta, coef, mode: int, what: str) -> torch.Tensor:
    if not torch.is_tensor(xd) or xd.dim() != 2:
        raise ValueError(f"{what}: rows must be a 2-d tensor")
    d, dp = int(d), int(xd.shape[1])
    check_matrix(xd, d, kernel_supported, what, "16..512")
    n, dev = _check_rows(xd, d, logt, delta, what), xd.device
    if mode != 2:
        logt, delta = _vec(logt, dev), _vec(delta, dev)
    c = _coef(coef, d, dev, what)
    out = torch.zeros((d + 3, 4 * n, n)[mode], dtype=torch.float64, device=dev)
    if n:
        lib, cus = _native.kernels(), ncu(dev)
        slabs = int(lib.cml_aft_slabs(n, d, cus))
        part = torch.empty(slabs * int(lib.cml_aft_part(d)), dtype=torch.float64, device=dev) if mode == 0 else None
        _native.check(lib.cml_aft_pass(xd.data_ptr(), n, dp, dp, d, _native.ptr(logt), _native.ptr(delta),
                                       c.data_ptr(), mode, _native.ptr(part), slabs, out.data_ptr(), cus,
                                       torch.cuda.current_stream(dev).cuda_stream), what)
    return out


def loss_grad(xd: torch.Tensor, d: int, logt: torch.Tensor, delta: torch.Tensor, coef) -> torch.Tensor:
    """K35, fit form: ``[X^T r | sum r | sum s | sum l]`` as ``loss_grad_reference`` returns it, for bf16 device rows
    in the ``to_device_matrix`` layout. All arithmetic after the exact bf16 -> f64 widening is f64; pad columns are
    masked by ``d``; nothing of size n is written. No atomics, no host read; two calls return the same bits."""
    if logt is None or delta is None:
        raise ValueError("aft loss_grad: one log time and censor per row are expected")
    return _launch(xd, d, logt, delta, coef, 0, "aft loss_grad")


def rows(xd: torch.Tensor, d: int, coef, logt: Optional[torch.Tensor] = None, delta: Optional[torch.Tensor] = None):
    """K35, rows form: the f64 device vector ``eta`` of every row; with ``logt`` and ``delta`` the tuple
    ``(eta, r, s, l)``, bit for bit what the fit form summed."""
    if (logt is None) != (delta is None):
        raise ValueError("aft rows: log times and censors come together")
    n = int(xd.shape[0]) if torch.is_tensor(xd) and xd.dim() == 2 else 0
    if logt is None:
        return _launch(xd, d, None, None, coef, 2, "aft rows")
    out = _launch(xd, d, logt, delta, coef, 1, "aft rows")
    return out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n:]
