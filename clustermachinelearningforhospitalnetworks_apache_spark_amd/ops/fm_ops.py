"""Loss, gradient and scores of the second-order factorisation machine: the reference form and the host wrappers
of K32 (``_native/csrc/fm.hip``).

The parameters ``p`` are ``ml.fm``'s flat vector ``[b | w (d) | V (d x f, row-major)]``. For a row x with label y,
in f64 after the exact widening:

* ``t_u = sum_i x_i V_iu``, ``sv_i = sum_u V_iu^2``
* ``s = b + sum_i w_i x_i + 1/2 (sum_u t_u^2 - sum_i x_i^2 sv_i)``
* squared loss: ``l = 1/2 (s - y)^2``, ``r = s - y``; logistic loss: ``l = softplus(s) - y s``,
  ``r = sigmoid(s) - y``, both through ``exp(-|s|)`` so that neither overflows
* ``db = sum_rows r``, ``dw_i = sum_rows r x_i``, ``u_i = sum_rows r x_i^2``,
  ``dV_iu = sum_rows x_i (r t_u) - V_iu u_i``

The sums are not divided by the number of rows: the caller divides after its all-reduce. The message of a shard is
the f64 vector ``[grad in the flat layout | loss]``. The second-order term needs no matrix of squares: its forward
part is one dot product per row against ``sv``, its backward part the one vector ``u``.

``loss_grad_reference`` / ``scores_reference`` evaluate this in f64 torch chunk by chunk on any device and dtype
(one chunk of the rows in f64 at a time, no autograd graph): the path of e4m3 rows and of bf16 rows outside the
kernel's limits, and the oracle of the kernel. ``loss_grad`` / ``scores`` are the gfx950 kernel for bf16 rows in
the ``to_device_matrix`` layout (``kernel_supported``): one launch reads every listed row once, a small second
launch adds the per-workgroup partials in workgroup order. ``CML_FM_KERNEL=0`` keeps the estimator on the
reference form.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from ._fused import check_matrix, env_enabled, gather_rows, ncu, row_list, widen

_native.register_kernel_sigs({
    "cml_fm_lds": (c_ll, [c_int, c_int]),
    "cml_fm_grid": (c_int, [c_ll, c_int, c_int, c_int]),
    "cml_fm_pass": (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_vp, c_ll, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_int,
                            c_int, c_vp]),
})

CHUNK = 8192
_TILE = 64
LOSSES = ("squared", "logistic")


def kernel_enabled() -> bool:
    return env_enabled("CML_FM_KERNEL")


def size(d: int, f: int) -> int:
    """Length of the flat parameter vector ``[b | w | V]``."""
    return 1 + d + d * f


def lds_bytes(dp: int, f: int) -> int:
    """LDS bytes of K32 (what ``cml_fm_lds`` returns), 0 outside the limits. With the parameter image
    ``[V^T ; w ; 0 ..]`` padded to hp = 16 (f <= 15) or 32 (f <= 31) units and the compiled width class
    dpt = max(dp, 64): the f64 image ``hp * dpt``, ``sv`` ``dpt``, the staging buffer of D^T ``hp * 66`` and the
    fold of db and the loss ``8`` doubles, plus the 64-row bf16 tile ``64 * (dpt + 8)`` values:
    ``8 * (hp dpt + dpt + 66 hp + 8) + 128 * (dpt + 8)`` bytes. That is 118 336 B at dp = 256, hp = 32 and
    144 704 B at dp = 512, hp = 16, inside one CU's 160 KB = 163 840 B; dp = 512 with hp = 32 would need
    218 688 B."""
    dp, f = int(dp), int(f)
    if dp < 16 or dp > 512 or dp & (dp - 1) or f < 1 or f > 31:
        return 0
    hp = 16 if f <= 15 else 32
    dpt = max(dp, 64)
    b = 8 * (hp * dpt + dpt + hp * 66 + 8) + 2 * _TILE * (dpt + 8)
    return b if b <= 160 * 1024 else 0


def kernel_supported(dtype: torch.dtype, dp: int, f: int) -> bool:
    """Whether K32 takes rows of this dtype and padded width with this factor size (anything else: the reference
    form). bf16 rows of padded width 16..512 with ``1 <= f <= 31``, as far as the LDS sum of ``lds_bytes`` allows:
    widths up to 256 take all of these, width 512 ``f <= 15``."""
    return dtype == torch.bfloat16 and lds_bytes(dp, f) > 0


# ---------------------------------------------------------------------------------------------- reference form
def _params(x, d: int, p, f: int, what: str):
    d, f = int(d), int(f)
    if not torch.is_tensor(x) or x.dim() != 2 or d < 1 or x.shape[1] < d or f < 1:
        raise ValueError(f"{what}: rows [n, >= d] with d >= 1 and a factor size >= 1 are expected")
    p = torch.as_tensor(p).to(device=x.device, dtype=torch.float64)
    if p.dim() != 1 or p.numel() != size(d, f):
        raise ValueError(f"{what}: {p.numel()} parameters, d = {d} and factor size {f} need {size(d, f)}")
    return p[0], p[1:1 + d], p[1 + d:].reshape(d, f)


def _scores_chunk(v, b, w, V, sv):
    t = v @ V
    return t, b + v @ w + 0.5 * ((t * t).sum(1) - (v * v) @ sv)


def loss_grad_reference(x: torch.Tensor, rows: Optional[torch.Tensor], d: int, y: torch.Tensor, p, f: int, loss: str,
                        chunk: int = CHUNK) -> torch.Tensor:
    """f64 ``[size(d, f) + 1]`` = ``[grad in the flat layout | loss]`` of the listed rows of ``x`` ``[n, >= d]``
    (any dtype and device; ``rows`` an ascending int64 index tensor, None for all rows) with labels ``y`` f64
    ``[n]`` indexed by row id, one widened chunk of rows at a time."""
    what = "fm loss_grad"
    b, w, V = _params(x, d, p, f, what)
    if loss not in LOSSES:
        raise ValueError(f"{what}: loss must be 'squared' or 'logistic'")
    n, dev = int(x.shape[0]), x.device
    if not torch.is_tensor(y) or y.shape != (n,):
        raise ValueError(f"{what}: one label per row of x is expected")
    y = y.to(device=dev, dtype=torch.float64)
    if rows is not None:
        rows = row_list(rows, dev, what)
    B = n if rows is None else int(rows.shape[0])
    sv = (V * V).sum(1)
    db = torch.zeros((), dtype=torch.float64, device=dev)
    dw = torch.zeros(d, dtype=torch.float64, device=dev)
    u = torch.zeros(d, dtype=torch.float64, device=dev)
    dV = torch.zeros(d, f, dtype=torch.float64, device=dev)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for st in range(0, B, chunk):
        v = widen(x[st:st + chunk, :d]) if rows is None else gather_rows(x, rows[st:st + chunk], d)
        yc = y[st:st + chunk] if rows is None else y[rows[st:st + chunk]]
        t, s = _scores_chunk(v, b, w, V, sv)
        if loss == "logistic":
            e = torch.exp(-s.abs())
            r = torch.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e)) - yc
            total += ((torch.clamp(s, min=0.0) + torch.log1p(e)) - yc * s).sum()
        else:
            r = s - yc
            total += (0.5 * r * r).sum()
        db += r.sum()
        rv = v * r[:, None]
        dw += rv.sum(0)
        u += (rv * v).sum(0)
        dV += rv.T @ t
    return torch.cat([db.reshape(1), dw, (dV - V * u[:, None]).reshape(-1), total.reshape(1)])


def scores_reference(x: torch.Tensor, d: int, p, f: int, chunk: int = CHUNK) -> torch.Tensor:
    """f64 ``[n]`` scores ``s`` of the rows ``x`` ``[n, >= d]`` of any dtype and device."""
    b, w, V = _params(x, d, p, f, "fm scores")
    sv = (V * V).sum(1)
    n = int(x.shape[0])
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    for st in range(0, n, chunk):
        out[st:st + chunk] = _scores_chunk(widen(x[st:st + chunk, :d]), b, w, V, sv)[1]
    return out


# ---------------------------------------------------------------------------------------------------- kernel
def _pack(p: torch.Tensor, d: int, f: int, dp: int) -> torch.Tensor:
    """The kernel's parameter image: ``[hp, dp]`` with rows 0 .. f - 1 = V^T and row f = w, zero padded, then b."""
    hp = 16 if f <= 15 else 32
    img = torch.zeros(hp * dp + 1, dtype=torch.float64, device=p.device)
    m = img[:hp * dp].view(hp, dp)
    m[:f, :d] = p[1 + d:].view(d, f).T
    m[f, :d] = p[1:1 + d]
    img[hp * dp] = p[0]
    return img


def _launch(xd, rows, d, y, p, f, loss, fit: bool, what: str):
    if not torch.is_tensor(xd) or xd.dim() != 2:
        raise ValueError(f"{what}: rows must be a 2-d tensor")
    dp, d, f = int(xd.shape[1]), int(d), int(f)
    check_matrix(xd, d, lambda dtype, dp: kernel_supported(dtype, dp, f), what,
                 "16..512 and the factor size inside the kernel's limits")
    n, dev = int(xd.shape[0]), xd.device
    p = torch.as_tensor(p)
    if p.dim() != 1 or p.numel() != size(d, f):
        raise ValueError(f"{what}: {p.numel()} parameters, d = {d} and factor size {f} need {size(d, f)}")
    if fit:
        if loss not in LOSSES:
            raise ValueError(f"{what}: loss must be 'squared' or 'logistic'")
        if (not torch.is_tensor(y) or y.dtype != torch.float64 or y.shape != (n,) or y.device != dev
                or not y.is_contiguous()):
            raise ValueError(f"{what}: the labels must be a contiguous f64 device vector, one per row of the matrix")
        if rows is not None:
            rows = row_list(rows, dev, what)
    B = n if rows is None else int(rows.shape[0])
    out = torch.zeros(size(d, f) + 1, dtype=torch.float64, device=dev) if fit else torch.empty(
        n, dtype=torch.float64, device=dev)
    if B:
        hp = 16 if f <= 15 else 32
        wp = _pack(p.to(device=dev, dtype=torch.float64), d, f, dp)
        lib, cus = _native.kernels(), ncu(dev)
        grid = int(lib.cml_fm_grid(B, dp, f, cus))
        part = torch.empty(grid * (hp * dp + dp + 2), dtype=torch.float64, device=dev) if fit else None
        _native.check(lib.cml_fm_pass(xd.data_ptr(), n, dp, d, f, _native.ptr(rows), B, _native.ptr(y if fit else None),
                                      wp.data_ptr(), _native.ptr(part), grid, out.data_ptr(), 1 if fit else 0,
                                      1 if loss == "logistic" else 0, cus,
                                      torch.cuda.current_stream(dev).cuda_stream), what)
    return out


def loss_grad(xd: torch.Tensor, rows: Optional[torch.Tensor], d: int, y: torch.Tensor, p, f: int,
              loss: str) -> torch.Tensor:
    """K32, fit form: the f64 device vector ``[grad | loss]`` as ``loss_grad_reference`` returns it. All arithmetic
    after the exact bf16 -> f64 widening is f64 (the products on the f64 MFMA); pad columns are masked by ``d``;
    with a row list every listed row is read once and no row is copied. No atomics, no host read; two calls return
    the same bits."""
    return _launch(xd, rows, d, y, p, f, loss, True, "fm loss_grad")


def scores(xd: torch.Tensor, d: int, p, f: int) -> torch.Tensor:
    """K32 without the backward pass: f64 ``[n]`` scores, bit for bit the fit form's ``s``."""
    return _launch(xd, None, d, None, p, f, None, False, "fm scores")
