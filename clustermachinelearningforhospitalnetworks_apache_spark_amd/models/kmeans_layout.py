"""Row layouts of the KMeans kernels and the per-tensor caches that ride on a feature matrix."""
from __future__ import annotations

import math
from typing import Optional

import torch

from ..ops import kmeans_ops as K
from ..parallel.comm import Communicator
from ..utils.device import padded_dim


def padded_dim_fp8(d: int) -> int:
    """fp8 rows: >= 256 bytes, power of two (16-B loads covering two MFMA k-steps, sort-regime lanes)."""
    return max(256, 1 << max(0, (d - 1).bit_length()))


def to_device_matrix(x: torch.Tensor, d: Optional[int] = None) -> torch.Tensor:
    """Zero-padded GPU copy of a feature matrix in the kernels' layout: bf16 [n, padded_dim(d)], or
    OCP e4m3fn [n, padded_dim_fp8(d)] when the features already are fp8 (SURVEY config 5)."""
    d = x.shape[1] if d is None else d
    if x.dtype == torch.float8_e4m3fn:
        dp = padded_dim_fp8(d)
        if x.shape[1] == dp and x.is_contiguous():
            return x
        out = torch.zeros((x.shape[0], dp), dtype=torch.uint8, device=x.device)
        out[:, :d] = x[:, :d].view(torch.uint8)
        return out.view(torch.float8_e4m3fn)
    dp = padded_dim(d)
    if x.dtype == torch.bfloat16 and x.shape[1] == dp and x.is_contiguous():
        return x
    out = torch.zeros((x.shape[0], dp), dtype=torch.bfloat16, device=x.device)
    step = 1 << 22
    for s in range(0, x.shape[0], step):
        out[s:s + step, :d] = x[s:s + step, :d].to(torch.bfloat16)
    return out


def host_layout(x: torch.Tensor, d: Optional[int] = None) -> torch.Tensor:
    """The pinned host copy of an out-of-core feature matrix in the kernels' layout (bf16
    [n, padded_dim(d)], or e4m3fn [n, padded_dim_fp8(d)] for fp8 rows), written straight into page-locked
    memory chunk by chunk (no unpinned intermediate) and cached on ``x`` while it is unmodified, so the
    fits and transforms of one column share one copy — and, through it, the cached row norms and stream
    buffers (every transform used to make a new bf16 copy plus a pinned copy of it). A matrix
    already in that layout and pinned is used as is."""
    from ..utils.hoststream import pinned_rows
    d = x.shape[1] if d is None else d
    fp8 = x.dtype == torch.float8_e4m3fn
    dp = padded_dim_fp8(d) if fp8 else padded_dim(d)
    want = torch.float8_e4m3fn if fp8 else torch.bfloat16
    layout = x.dtype == want and x.shape[1] == dp and x.is_contiguous()
    if layout and (x.is_pinned() or not torch.cuda.is_available()):
        return x
    ent = getattr(x, "_cml_hostlayout", None)
    if ent is not None and ent[0] == x._version and ent[1] == d:
        return ent[2]
    pin = torch.cuda.is_available()
    n = x.shape[0]
    if layout:
        out = pinned_rows(x)
    elif fp8:
        out = torch.zeros((n, dp), dtype=torch.uint8, pin_memory=pin)
        out[:, :d] = x[:, :d].view(torch.uint8)
        out = out.view(torch.float8_e4m3fn)
    else:
        out = torch.zeros((n, dp), dtype=torch.bfloat16, pin_memory=pin)
        step = 1 << 20
        for s in range(0, n, step):
            out[s:s + step, :d] = x[s:s + step, :d].to(torch.bfloat16)
    try:
        x._cml_hostlayout = (x._version, d, out)
    except (AttributeError, RuntimeError):
        pass
    return out


def unit_rows(x: torch.Tensor, d: Optional[int] = None, exact: Optional[bool] = None) -> torch.Tensor:
    """Rows scaled to unit length (cosine KMeans). bf16 on the GPU's MFMA path (computed in f32; fp8
    inputs widen to bf16: unit components need more than e4m3's 3 mantissa bits), f64 on the CPU and
    on the GPU's source-precision path (``exact``, default: f32/f64 input). Spark rejects zero-length
    vectors for the cosine measure, and so does this."""
    d = x.shape[1] if d is None else d
    if exact is None:
        exact = (not x.is_cuda) or x.dtype in (torch.float32, torch.float64)
    out_dtype = torch.float64 if exact else torch.bfloat16
    work = torch.float64 if exact else torch.float32
    out = torch.empty((x.shape[0], d), dtype=out_dtype, device=x.device)
    step = 1 << 22
    for s in range(0, x.shape[0], step):
        v = x[s:s + step, :d].to(work)
        nrm = v.norm(dim=1, keepdim=True)
        if bool((nrm == 0).any()):
            raise ValueError("Cosine distance is not defined for zero-length vectors.")
        out[s:s + step] = (v / nrm).to(out_dtype)
    return out


def dd_sums_exact(x: torch.Tensor, d: int, comm: Communicator) -> bool:
    """Whether double-double sums of the f64 rows are exact in any order (so incremental, chunked and
    rank-folded sums agree bit for bit): a value is a multiple of 2^(e_min - 52) and a total of n of them
    stays below 2^(e_max + 1 + log2 n), which a double-double (2 x 53 bits) holds while
    e_max - e_min + 53 + log2(n) <= 104 (2 bits of margin). One pass over the rows (cached on the tensor
    while it is unmodified); the span and the row count are agreed over every rank (a collective)."""
    ent = getattr(x, "_cml_f64span", None)
    if ent is not None and ent[0] == x._version and ent[1] == d:
        lo, hi = ent[2], ent[3]
    else:
        lo, hi = math.inf, -math.inf
        step = max(1, (1 << 24) // max(d, 1))
        for r0 in range(0, int(x.shape[0]), step):
            a = x[r0:r0 + step, :d].abs()
            mx = float(a.max()) if a.numel() else 0.0
            if mx > 0:
                mn = float(torch.where(a > 0, a, torch.full_like(a, math.inf)).min())
                hi = max(hi, math.frexp(mx)[1])
                lo = min(lo, math.frexp(mn)[1])
        try:
            x._cml_f64span = (x._version, d, lo, hi)
        except (AttributeError, RuntimeError):
            pass
    v = torch.tensor([-lo if lo != math.inf else -1e9, hi if hi != -math.inf else -1e9, float(x.shape[0])],
                     dtype=torch.float64, device=comm.device)
    if comm.is_distributed:
        comm.allreduce_(v[:2], op="max")
        comm.allreduce_(v[2:], op="sum")
    lo_g, hi_g, n_g = -float(v[0]), float(v[1]), float(v[2])
    if hi_g < -1e8:  # every value is zero
        return True
    return (hi_g - lo_g) + 53 + math.ceil(math.log2(n_g + 1)) <= 104


def cached_row_norms(x: torch.Tensor, n: int, dp: int):
    """The ``_cml_xnorm`` entry of ``x`` (written by cached_row_sqnorm and the engine's row pass) while the tensor
    is unmodified: (||x||² f32, bf16 exponent range of X, ||x||² summed in f64), else None."""
    ent = getattr(x, "_cml_xnorm", None)
    if ent is not None and ent[0] == x._version and ent[1] == (n, dp):
        return ent[2], ent[3], ent[4]
    return None


def cached_row_sqnorm(x: torch.Tensor, n: int, dp: int) -> torch.Tensor:
    """||x_i||² of the device matrix's rows, kept on the tensor itself while it is unmodified.

    Spark caches point norms with the vectors (reference KMeans uses VectorWithNorm); here the cache
    rides on the feature tensor, so a fit followed by ``KMeansModel.transform``/``computeCost`` on the
    same features reads the matrix once for its norms instead of once per call. The entry is keyed by
    the tensor's version counter: any in-place write invalidates it."""
    ent = cached_row_norms(x, n, dp)
    if ent is not None:
        return ent[0]
    xn = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)
    xn64 = torch.empty(max(n, 1), dtype=torch.float64, device=x.device)
    er = torch.tensor([2 ** 31 - 1, -1], dtype=torch.int32, device=x.device)
    if n:
        K.row_pass(x, n, dp, xn, erange=er, xn64=xn64)
    try:
        x._cml_xnorm = (x._version, (n, dp), xn, er, xn64)
    except (AttributeError, RuntimeError):
        pass
    return xn
