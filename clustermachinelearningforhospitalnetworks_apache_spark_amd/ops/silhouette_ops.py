"""Silhouette from cluster statistics (Spark's ClusteringEvaluator): the reference form and the host
wrappers of K26 (``_native/csrc/silhouette.hip``).

With ``W_c = Σ w_i``, ``μ_c`` and ``q_c`` of every cluster (``cluster_stats*``: ``[S | W | Q]``, summed over
ranks by the caller) the mean distance from a row to the rows of cluster ``c`` is

* squaredEuclidean: ``D_c(x) = |x|² − 2 x·μ_c + q_c``, ``μ_c = Σ w x / W_c``, ``q_c = Σ w |x|² / W_c``
* cosine: ``D_c(x) = 1 − x·μ_c / |x|``, ``μ_c = Σ w x/|x| / W_c``

and per row ``own = D_l(x)``, ``b = min over live c ≠ l of D_c(x)``, ``a = own·W_l / (W_l − w)``,
``s = 1 − a/b`` (a < b), ``b/a − 1`` (a > b), 0 otherwise and for a cluster of one row's weight (``W_l == w``).

``silhouette_reference`` / ``cluster_stats_reference`` evaluate this in f64 torch, chunk by chunk, on any
device and dtype: the CPU path, the path of f32 / f64 columns on the GPU and the oracle of the kernels.
``silhouette_score`` / ``cluster_stats_device`` are the gfx950 kernels for bf16 / e4m3 rows in the
``to_device_matrix`` layout (``kernel_supported``).
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from .._native import c_int, c_ll, c_vp

_native.register_kernel_sigs({
    "cml_row_sqnorm_f64": (c_int, [c_vp, c_ll, c_ll, c_int, c_vp, c_vp]),
    "cml_label_wsum": (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp,
                               c_vp, c_vp, c_vp]),
    "cml_silhouette_rows_per_block": (c_int, [c_int]),
    "cml_silhouette_score": (c_int, [c_vp, c_ll, c_ll, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int,
                                     c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
})

CHUNK = 1 << 16
ZERO_ROW = "Cosine distance is not defined for zero-length vectors."
_DTYPE_CODE = {torch.bfloat16: 0, torch.float8_e4m3fn: 3}
K_MAX = 1024


# ---------------------------------------------------------------------------------------------- reference form
def has_zero_rows(x: torch.Tensor, chunk: int = CHUNK) -> bool:
    """Whether a row of ``x`` has length 0 (cosine is undefined there), chunk by chunk in f64."""
    for s in range(0, x.shape[0], chunk):
        v = x[s:s + chunk].to(torch.float64)
        if bool(((v * v).sum(1) == 0).any()):
            return True
    return False


def cluster_stats_reference(x: torch.Tensor, labels: torch.Tensor, K: int, weights: Optional[torch.Tensor] = None,
                            cosine: bool = False, chunk: int = CHUNK) -> torch.Tensor:
    """``[S | W | Q]`` as one f64 ``[K, d + 2]`` tensor: ``S_c = Σ w x`` (cosine: ``Σ w x/|x|``), ``W_c = Σ w``,
    ``Q_c = Σ w |x|²`` (cosine: 0) over this rank's rows of cluster ``c``. A zero-length row raises for cosine."""
    n, d = int(x.shape[0]), int(x.shape[1])
    out = torch.zeros(K, d + 2, dtype=torch.float64, device=x.device)
    for s in range(0, n, chunk):
        v = x[s:s + chunk].to(torch.float64)
        g = labels[s:s + chunk].to(torch.int64)
        w = (torch.ones(v.shape[0], dtype=torch.float64, device=x.device) if weights is None
             else weights[s:s + chunk].to(torch.float64))
        xx = (v * v).sum(1)
        if cosine:
            if bool((xx == 0).any()):
                raise ValueError(ZERO_ROW)
            v = v / xx.sqrt()[:, None]
            xx = torch.zeros_like(xx)
        out.index_add_(0, g, torch.cat([v * w[:, None], w[:, None], (w * xx)[:, None]], 1))
    return out


def _row_silhouette(own, b, Wl, w):
    """s from own, b (f64), the own cluster's weight and the row's weight."""
    single = Wl == w
    a = own * Wl / torch.where(single, torch.ones_like(Wl), Wl - w)
    s = torch.where(a < b, 1.0 - a / b, torch.where(a > b, b / a - 1.0, torch.zeros_like(a)))
    return torch.where(single, torch.zeros_like(s), s), a


def silhouette_reference(x: torch.Tensor, labels: torch.Tensor, K: int, weights: Optional[torch.Tensor] = None,
                         cosine: bool = False, rows: bool = False, stats: Optional[torch.Tensor] = None,
                         chunk: int = CHUNK):
    """This rank's partial sums ``(Σ w s, Σ w)`` as an f64 ``[2]`` tensor, for the cluster statistics ``stats``
    (``[K, d + 2]``, already summed over ranks; default: this rank's own). f64 torch in row chunks: never more
    than ``chunk x K`` distances. ``rows=True`` also returns the per-row ``own``, ``b`` (f64), ``nb`` (the
    arg-min cluster, -1 where no other cluster is live) and ``s``."""
    n, d = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    if stats is None:
        stats = cluster_stats_reference(x, labels, K, weights, cosine, chunk)
    S, W, Q = stats[:, :d], stats[:, d], stats[:, d + 1]
    live = W > 0
    Wsafe = torch.where(live, W, torch.ones_like(W))
    mu = S / Wsafe[:, None]
    q = Q / Wsafe
    inf = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
    dead = torch.where(live, torch.zeros_like(inf), inf)
    part = torch.zeros(2, dtype=torch.float64, device=dev)
    per = [[], [], [], []]
    for st in range(0, n, chunk):
        v = x[st:st + chunk].to(torch.float64)
        g = labels[st:st + chunk].to(torch.int64)
        w = (torch.ones(v.shape[0], dtype=torch.float64, device=dev) if weights is None
             else weights[st:st + chunk].to(torch.float64))
        xx = (v * v).sum(1)
        if cosine:
            D = 1.0 - (v @ mu.T) / xx.sqrt()[:, None]
        else:
            D = xx[:, None] - 2.0 * (v @ mu.T) + q[None, :]
        D = D + dead[None, :]
        own = D.gather(1, g[:, None]).squeeze(1)
        D.scatter_(1, g[:, None], float("inf"))
        b, nb = D.min(1)
        s, _ = _row_silhouette(own, b, W[g], w)
        part += torch.stack([(w * s).sum(), w.sum()])
        if rows:
            nb = torch.where(torch.isinf(b), torch.full_like(nb, -1), nb)
            for lst, t in zip(per, (own, b, nb, s)):
                lst.append(t)
    if not rows:
        return part
    if not per[0]:
        z = torch.zeros(0, dtype=torch.float64, device=dev)
        return part, z, z.clone(), torch.zeros(0, dtype=torch.int64, device=dev), z.clone()
    return (part,) + tuple(torch.cat(p) for p in per)


# ---------------------------------------------------------------------------------------------------- kernels
def kernel_supported(dtype: torch.dtype, dp: int, K: int) -> bool:
    """Whether K26 takes rows of this dtype and padded width with K clusters (anything else: the reference
    form). bf16: 16 <= dp <= 512; e4m3: dp in {256, 512}; 2 <= K <= 1024."""
    if not 2 <= K <= K_MAX:
        return False
    if dtype == torch.bfloat16:
        return dp in (16, 32, 64, 128, 256, 512)
    if dtype == torch.float8_e4m3fn:
        return dp in (256, 512)
    return False


def _check_layout(xd: torch.Tensor) -> int:
    if not xd.is_cuda or xd.dtype not in _DTYPE_CODE or xd.dim() != 2 or not xd.is_contiguous():
        raise ValueError("silhouette kernels: rows must be a contiguous bf16 / e4m3 device matrix")
    dp = int(xd.shape[1])
    if not kernel_supported(xd.dtype, dp, 2):
        raise ValueError(f"silhouette kernels: unsupported padded width {dp} for {xd.dtype}")
    return dp


def _labels32(labels: torch.Tensor, K: int, n: int) -> torch.Tensor:
    lab = (labels if labels.dtype == torch.int32 else labels.to(torch.int32)).contiguous()
    if lab.shape[0] != n:
        raise ValueError("silhouette kernels: rows and labels differ in length")
    if n:
        lo, hi = torch.aminmax(lab)
        if int(lo) < 0 or int(hi) >= K:  # the kernels index [K] arrays by label: never launch out of range
            raise ValueError(f"silhouette kernels: labels outside [0, {K})")
    return lab


def row_sqnorm(xd: torch.Tensor) -> torch.Tensor:
    """f64 ``|x_i|²`` per row (exact products, f64 sums)."""
    _check_layout(xd)
    n = int(xd.shape[0])
    out = torch.empty(n, dtype=torch.float64, device=xd.device)
    if n:
        stream = torch.cuda.current_stream(xd.device).cuda_stream
        _native.check(_native.kernels().cml_row_sqnorm_f64(xd.data_ptr(), n, xd.shape[1], _DTYPE_CODE[xd.dtype],
                                                       out.data_ptr(), stream), "row_sqnorm")
    return out


def label_wsum(xd: torch.Tensor, labels: torch.Tensor, K: int, omega: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f64 ``[K, dp]``: ``S[c] = Σ_{l_i = c} ω_i x_i`` (``ω`` f64 per row, None = 1). Deterministic: the rows
    are taken in label order (a stable sort) and every addition has a fixed place; no atomics."""
    dp = _check_layout(xd)
    n = int(xd.shape[0])
    if K < 1:
        raise ValueError("label_wsum: K must be positive")
    lab = _labels32(labels, K, n)
    S = torch.zeros(K, dp, dtype=torch.float64, device=xd.device)
    if n == 0:
        return S
    if omega is not None:
        omega = omega.to(torch.float64).contiguous()
        if omega.shape[0] != n:
            raise ValueError("label_wsum: rows and factors differ in length")
    slab, perm = torch.sort(lab, stable=True)
    off = torch.searchsorted(slab, torch.arange(K + 1, dtype=torch.int32, device=xd.device)).to(torch.int64)
    L = 256 if n < (1 << 20) else 1024
    nunits = -(-n // L)
    head = torch.empty(nunits, dp, dtype=torch.float64, device=xd.device)
    tail = torch.empty(nunits, dp, dtype=torch.float64, device=xd.device)
    hl = torch.empty(nunits, 2, dtype=torch.int32, device=xd.device)
    stream = torch.cuda.current_stream(xd.device).cuda_stream
    _native.check(_native.kernels().cml_label_wsum(
        xd.data_ptr(), n, dp, dp, _DTYPE_CODE[xd.dtype], slab.data_ptr(), perm.data_ptr(), off.data_ptr(),
        _native.ptr(omega), K, L, S.data_ptr(), head.data_ptr(), tail.data_ptr(), hl.data_ptr(), stream),
        "label_wsum")
    return S


def cluster_stats_device(xd: torch.Tensor, labels: torch.Tensor, K: int, weights: Optional[torch.Tensor] = None,
                         cosine: bool = False):
    """(``[S | W | Q]`` f64 ``[K, dp + 2]``, zero-row flag) of this rank's rows through the kernels: one pass
    for the row norms, one gather pass for S; W and Q are scalar-per-row group sums (K25). The flag (a 0-d
    bool tensor) says a row has length 0; the caller agrees it over ranks before raising for cosine, and S is
    then meaningless."""
    from .group_ops import group_reduce
    dp = _check_layout(xd)
    n = int(xd.shape[0])
    out = torch.zeros(K, dp + 2, dtype=torch.float64, device=xd.device)
    if n == 0:
        return out, torch.zeros((), dtype=torch.bool, device=xd.device)
    lab = _labels32(labels, K, n)
    w = None if weights is None else weights.to(torch.float64).contiguous()
    nrm2 = row_sqnorm(xd)
    zero = (nrm2 == 0).any()
    if cosine:
        inv = torch.rsqrt(nrm2.clamp_(min=torch.finfo(torch.float64).tiny))
        omega = inv if w is None else inv.mul_(w)
        qv = None
    else:
        omega = w
        qv = nrm2 if w is None else nrm2.mul_(w)
    out[:, :dp] = label_wsum(xd, lab, K, omega)
    if w is None:
        out[:, dp] = torch.bincount(lab, minlength=K).to(torch.float64)
    else:
        out[:, dp] = group_reduce(lab, w, K, "sum", ids_in_range=True)
    if qv is not None:
        out[:, dp + 1] = group_reduce(lab, qv, K, "sum", ids_in_range=True)
    return out, zero


def _split3(v32: torch.Tensor):
    hi = v32.to(torch.bfloat16)
    r1 = v32 - hi.to(torch.float32)
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.to(torch.float32)).to(torch.bfloat16)
    return hi, mid, lo


def score_operands(stats: torch.Tensor, dp: int, cosine: bool):
    """The kernel's centre-side operands from the global ``[S | W | Q]`` (k x d work in f64): the three-term
    bf16 table of ν ``[KT, 3, 16, dpk]``, κ f32 ``[16 KT]`` (+inf: dead cluster or padding), the shift m f32
    ``[dpk]`` and ``W`` f64 ``[K]``. squaredEuclidean is taken about the weighted global mean (rounded to f32,
    the value the kernel subtracts): ν = μ − m, κ = q − 2 m·μ + |m|² + 2 m·ν; cosine: ν = μ, κ = 0, m = 0."""
    K = int(stats.shape[0])
    dev = stats.device
    S, W, Q = stats[:, :dp], stats[:, dp].contiguous(), stats[:, dp + 1]
    live = W > 0
    Wsafe = torch.where(live, W, torch.ones_like(W))
    mu = S / Wsafe[:, None]
    dpk = max(32, dp)
    KT = -(-K // 16)
    if cosine:
        m = torch.zeros(dp, dtype=torch.float64, device=dev)
        nu = mu
        kap = torch.zeros(K, dtype=torch.float64, device=dev)
    else:
        tot = W.sum()
        m = S.sum(0) / torch.where(tot > 0, tot, torch.ones_like(tot))
        m = m.to(torch.float32).to(torch.float64)
        nu = mu - m[None, :]
        kap = Q / Wsafe - 2.0 * (mu @ m) + m @ m + 2.0 * (nu @ m)
    nu = torch.where(live[:, None], nu, torch.zeros_like(nu))
    kappa = torch.full((16 * KT,), float("inf"), dtype=torch.float32, device=dev)
    kappa[:K] = torch.where(live, kap, torch.full_like(kap, float("inf"))).to(torch.float32)
    nu32 = torch.zeros(16 * KT, dpk, dtype=torch.float32, device=dev)
    nu32[:K, :dp] = nu.to(torch.float32)
    tab = torch.stack(_split3(nu32)).view(3, KT, 16, dpk).permute(1, 0, 2, 3).contiguous()
    mean = torch.zeros(dpk, dtype=torch.float32, device=dev)
    mean[:dp] = m.to(torch.float32)
    return tab, kappa, mean, W, KT, dpk


def silhouette_score(xd: torch.Tensor, labels: torch.Tensor, stats: torch.Tensor,
                     weights: Optional[torch.Tensor] = None, cosine: bool = False, rows: bool = False):
    """K26: this rank's ``(Σ w s, Σ w)`` (f64 ``[2]``) for the global statistics ``stats`` ``[K, dp + 2]``, in
    one read of ``xd``. ``rows=True`` also returns the kernel's per-row ``own``, ``b`` (f32), ``nb`` (i32, -1:
    no other live cluster) and ``s`` (f32)."""
    dp = _check_layout(xd)
    n, K = int(xd.shape[0]), int(stats.shape[0])
    if not kernel_supported(xd.dtype, dp, K) or stats.shape[1] != dp + 2:
        raise ValueError(f"silhouette_score: unsupported shape (dp = {dp}, K = {K})")
    dev = xd.device
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    per = None
    if rows:
        per = (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
               torch.full((n,), -1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev))
    if n == 0:
        return (out,) + per if rows else out
    lab = _labels32(labels, K, n)
    w = None if weights is None else weights.to(torch.float64).contiguous()
    if w is not None and w.shape[0] != n:
        raise ValueError("silhouette_score: rows and weights differ in length")
    tab, kappa, mean, W, KT, dpk = score_operands(stats.to(torch.float64), dp, cosine)
    lib = _native.kernels()
    rpb = int(lib.cml_silhouette_rows_per_block(dpk))
    partial = torch.empty(-(-n // rpb), 2, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pp = [t.data_ptr() for t in per] if rows else [None] * 4
    _native.check(lib.cml_silhouette_score(
        xd.data_ptr(), n, dp, _DTYPE_CODE[xd.dtype], lab.data_ptr(), _native.ptr(w), tab.data_ptr(),
        kappa.data_ptr(), mean.data_ptr(), W.data_ptr(), KT, dpk, 1 if cosine else 0, partial.data_ptr(),
        out.data_ptr(), *pp, stream), "silhouette_score")
    return (out,) + per if rows else out
