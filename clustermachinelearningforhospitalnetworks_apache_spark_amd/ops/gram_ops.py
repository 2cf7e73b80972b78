"""The Gram matrix ``[X 1 z]^T W [X 1 z]`` of feature columns wider than K15 takes (d > 30): the reference form and
the host wrapper of K31 (``_native/csrc/gram.hip``).

With ``a_r = [x_r[:d], 1, z_r]``, ``m = d + 2`` and ``w_r = 1`` when no weight is given, in f64 after the exact
widening of the stored values:

    ``G[i][j] = sum_r a_ri * (w_r * a_rj)``

The weight goes on one side (there is no ``sqrt(w)``). The result is ``(m, m)`` f64 and exactly symmetric: the upper
triangle is computed and mirrored. The sums are per shard and not normalised: the caller all-reduces.

``gram_reference`` evaluates this in f64 torch chunk by chunk on any device and stored dtype (one chunk of ``CHUNK``
rows in f64 at a time, never an ``n x m`` copy): the path of every column the kernel does not take, and the oracle of
the kernel. ``gram`` is the gfx950 kernel for bf16 rows with ``31 <= d <= 512`` (``kernel_supported``): one launch
computes the 16 x 16 blocks of the upper triangle per row slab on the f64 MFMA, a small second launch adds the slabs
in slab order and mirrors. ``CML_GRAM_KERNEL=0`` keeps every such column on the reference form.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from ._fused import env_enabled, ncu, widen

_native.register_kernel_sigs({
    "cml_gram_mfma_slabs": (c_int, [c_ll, c_int, c_int]),
    "cml_gram_mfma_part": (c_ll, [c_int]),
    "cml_gram_mfma": (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp]),
})

CHUNK = 8192
MIN_D = 31
MAX_D = 512


def kernel_enabled() -> bool:
    return env_enabled("CML_GRAM_KERNEL")


def kernel_supported(dtype: torch.dtype, d: int) -> bool:
    """Whether K31 takes rows of this dtype with ``d`` feature columns (anything else: the reference form)."""
    return dtype == torch.bfloat16 and MIN_D <= int(d) <= MAX_D


# ---------------------------------------------------------------------------------------------- reference form
def _mirror(g: torch.Tensor) -> torch.Tensor:
    return torch.triu(g) + torch.triu(g, 1).T


def gram_reference(x: torch.Tensor, d: int, z: torch.Tensor, w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f64 ``(d + 2, d + 2)`` Gram matrix of the rows ``x`` ``[n, >= d]`` (any dtype and device) with the f64-widened
    column ``z`` ``[n]`` and the optional weights ``w`` ``[n]``, one widened chunk of ``CHUNK`` rows at a time."""
    n, dev = int(x.shape[0]), x.device
    d = int(d)
    if x.dim() != 2 or x.shape[1] < d or z.numel() != n or (w is not None and w.numel() != n):
        raise ValueError("gram: rows [n, >= d], one z and (optionally) one weight per row are expected")
    m = d + 2
    z = z.reshape(-1)
    w = w.reshape(-1) if w is not None else None
    g = torch.zeros((m, m), dtype=torch.float64, device=dev)
    chunk = int(CHUNK)
    for st in range(0, n, chunk):
        en = min(n, st + chunk)
        a = torch.empty((en - st, m), dtype=torch.float64, device=dev)
        a[:, :d] = widen(x[st:en, :d])
        a[:, d] = 1.0
        a[:, d + 1] = z[st:en].to(device=dev, dtype=torch.float64)
        if w is None:
            g += a.T @ a
        else:
            g += a.T @ (a * w[st:en].to(device=dev, dtype=torch.float64)[:, None])
    return _mirror(g)


# ---------------------------------------------------------------------------------------------------- kernel
def _readable_cols(xx: torch.Tensor) -> int:
    """Columns of a row that the kernel's 16-byte loads may touch: the width rounded up to 8 where the row pitch and
    the storage behind the last row cover it, else 0."""
    wc = (xx.shape[1] + 7) // 8 * 8
    if wc == xx.shape[1]:
        return wc
    end = xx.storage_offset() + (xx.shape[0] - 1) * xx.stride(0) + wc
    if xx.stride(0) >= wc and end * xx.element_size() <= xx.untyped_storage().nbytes():
        return wc
    return 0


def gram(x: torch.Tensor, d: int, z: torch.Tensor, w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K31: the f64 device matrix that ``gram_reference`` returns, for bf16 device rows with ``31 <= d <= 512``.
    All arithmetic after the exact bf16 -> f64 widening is f64 (the products on the f64 MFMA); ``z`` and ``w`` are
    read as f64; pad columns (``>= d``) and rows past ``n`` never reach a product. No atomics, no host read; two
    calls return the same bits."""
    from .glm_ops import _prep
    d = int(d)
    if not torch.is_tensor(x) or x.dim() != 2 or not x.is_cuda or x.shape[1] < d or not kernel_supported(x.dtype, d):
        raise ValueError("gram: the kernel takes bf16 device rows [n, >= d] with 31 <= d <= 512")
    n, dev = int(x.shape[0]), x.device
    if z.numel() != n or (w is not None and w.numel() != n):
        raise ValueError("gram: one z and (optionally) one weight per row are expected")
    m = d + 2
    out = torch.zeros((m, m), dtype=torch.float64, device=dev)
    if n == 0:
        return out
    xx = _prep(x)
    wc = _readable_cols(xx)
    if wc == 0:  # a width that is no multiple of 8 at the very end of its storage: pad the rows once
        buf = torch.zeros((n, (xx.shape[1] + 7) // 8 * 8), dtype=xx.dtype, device=dev)
        buf[:, :xx.shape[1]] = xx
        xx, wc = buf, int(buf.shape[1])
    zz = z.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    ww = w.reshape(-1).to(device=dev, dtype=torch.float64).contiguous() if w is not None else None
    lib, cus = _native.kernels(), ncu(dev)
    slabs = int(lib.cml_gram_mfma_slabs(n, d, cus))
    part = torch.empty(slabs * int(lib.cml_gram_mfma_part(d)), dtype=torch.float64, device=dev)
    _native.check(lib.cml_gram_mfma(xx.data_ptr(), n, xx.stride(0), wc, d, zz.data_ptr(), _native.ptr(ww),
                                    part.data_ptr(), slabs, out.data_ptr(), cus,
                                    torch.cuda.current_stream(dev).cuda_stream), "gram")
    return out
