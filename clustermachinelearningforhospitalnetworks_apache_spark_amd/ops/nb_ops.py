"""The two row passes of naive Bayes: the reference forms and the host wrappers of K34 (``_native/csrc/nb.hip``).

**Moments.** With labels ``l``, weights ``w`` (1 without any) and a shift table ``m`` ``[C, d]`` (0 without one), in
f64 after the exact widening of the stored row, ``moments`` is f64 ``[C, 1 + 2 d]``::

    [ n_c = sum_{l = c} w | sum_{l = c} w (x - m_c) | sum_{l = c} w (x - m_c)^2 ]

and ``bad`` is f64 ``[2]`` = ``[# of x_i < 0, # of x_i not in {0, 1}]`` over the ``d`` live columns of every row: the
message a fit all-reduces. A row whose label is outside ``0 .. C-1`` adds nothing to ``moments`` (it still counts
towards ``bad``).

**Scores.** ``(raw, prob, pred)`` = f64 ``[n, C]``, ``[n, C]``, ``[n]`` of a table ``kind``:

* ``"linear"``: ``s = x W^T + b``, ``raw = s``
* ``"complement"``: ``s = x W^T``, ``raw = s - lse``
* ``"gaussian"``: ``s_c = b_c - 1/2 sum_i (x_i - W_ci)^2 iv_ci`` (the centred form, never the expanded one),
  ``raw = s``

with ``lse`` the max-subtracted log-sum-exp of ``s``, ``prob = exp(s - lse)`` and ``pred`` the lowest index among the
maxima of ``raw`` (0 where there is none: a row of NaN).

``moments_reference`` / ``scores_reference`` evaluate this in f64 torch chunk by chunk on any device and stored dtype
(never an ``n x d`` copy, no host read): the path of every column the kernel does not take, of CPU frames' callers that
want it, and the oracle of the kernel. ``moments`` / ``scores`` are the gfx950 kernel for bf16 device rows in the
``to_device_matrix`` layout (``kernel_supported``): one launch reads every row once; the moments form writes
per-workgroup partials that a small second launch adds in a fixed order (no atomics, the same bits on every call).
``CML_NB_KERNEL=0`` keeps the estimator on the reference form.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from ._fused import check_matrix, env_enabled, ncu, widen

_native.register_kernel_sigs({
    "cml_nb_lds": (c_ll, [c_int, c_int, c_int]),
    "cml_nb_grid": (c_int, [c_ll, c_int, c_int, c_int]),
    "cml_nb_part": (c_ll, [c_int, c_int, c_int, c_int]),
    "cml_nb_moments": (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_int,
                               c_vp]),
    "cml_nb_scores": (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
})

CHUNK = 1 << 16
KINDS = ("linear", "complement", "gaussian")
WIDTHS = (16, 32, 64, 128, 256, 512)
MAX_C = 32
LDS_PER_CU = 160 * 1024


def kernel_enabled() -> bool:
    return env_enabled("CML_NB_KERNEL")


def tile_rows(dp: int) -> int:
    """Rows of a K34 tile at this padded width."""
    return min(256, 8192 // int(dp))


def lds_bytes(dp: int, C: int, gaussian: bool) -> int:
    """LDS bytes K34 needs for a model of padded width ``dp`` with ``C`` classes: the larger of

    * the moments form: the bf16 row tile ``TR (dp + 16) 2``, the weights and labels ``12 TR`` and, for gaussian
      (the shifted second pass), the f64 shift table ``8 C dp``;
    * the scores form: the row tile ``TR (dp + 4) 2``, the f64 table (``[W | b]`` with the classes padded to a
      multiple of 16: ``8 (C16 dp + C16)``; gaussian ``[theta | iv | b]`` with the odd pitch:
      ``8 (2 C (dp + 1) + C)``; rounded up to 16 bytes) and the f64 score tile ``8 TR (C | 1)``,

    with ``TR = min(256, 8192 / dp)`` rows per tile. ``cml_nb_lds`` is the same sum."""
    dp, C = int(dp), int(C)
    tr = tile_rows(dp)
    mom = tr * (dp + 16) * 2 + tr * 12 + (C * dp * 8 if gaussian else 0)
    c16 = (C + 15) // 16 * 16
    tab = 2 * C * (dp + 1) + C if gaussian else c16 * dp + c16
    tab += tab & 1
    return max(mom, tr * (dp + 4) * 2 + tab * 8 + tr * (C | 1) * 8)


def kernel_supported(dtype: torch.dtype, dp: int, arg) -> bool:
    """Whether K34 takes rows of this dtype and padded width for ``arg = (C, gaussian)`` (anything else: the
    reference form): bf16 rows of padded width 16, 32, 64, 128, 256 or 512, ``1 <= C <= 32``, and ``lds_bytes``
    within one CU's 160 KB (163 840 B). The exact table: every such width and class count is taken, but for gaussian
    at width 512 with more than 17 classes (C = 17 needs 158 368 B, C = 18 166 832 B: two ``C x 513`` f64 tables
    beside the 16 512 B row tile). The widest other cases: multinomial / bernoulli / complement at 512 x 32,
    152 064 B; gaussian at 256 x 32, 156 928 B."""
    C, gaussian = arg
    return (dtype == torch.bfloat16 and int(dp) in WIDTHS and 1 <= int(C) <= MAX_C
            and lds_bytes(dp, C, bool(gaussian)) <= LDS_PER_CU)


# ---------------------------------------------------------------------------------------------- reference form
def _f64(v, dev) -> torch.Tensor:
    if torch.is_tensor(v):
        return v.to(device=dev, dtype=torch.float64)
    return torch.as_tensor(np.asarray(v, dtype=np.float64), device=dev)


def _check_rows(x, d: int, what: str) -> int:
    if not torch.is_tensor(x) or x.dim() != 2 or d < 0 or x.shape[1] < d:
        raise ValueError(f"{what}: rows [n, >= d] are expected")
    return int(x.shape[0])


_BLOCK = 512


def _class_sums(oh: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """``oh^T v`` ``[C, d]`` of a chunk. A chunk of whole 512-row blocks is one batched GEMM and a sum over the
    blocks in block order: a single GEMM with 2 .. 32 output rows walks the whole chunk in one workgroup."""
    m = int(oh.shape[0])
    if m > _BLOCK and m % _BLOCK == 0:
        a = oh.reshape(-1, _BLOCK, oh.shape[1]).transpose(1, 2)
        return torch.bmm(a, v.reshape(-1, _BLOCK, v.shape[1])).sum(0)
    return oh.T @ v


def moments_reference(x: torch.Tensor, d: int, labels: torch.Tensor, weights: Optional[torch.Tensor], C: int,
                      shift=None, chunk: int = CHUNK, second: bool = True):
    """``(moments, bad)`` of the rows ``x`` ``[n, >= d]`` of any dtype and device, one widened chunk at a time. The
    class sums are a chunk-sized one-hot GEMM ``onehot(w)^T v`` (no ``index_add_``: its f64 atomics do not give the
    same bits twice). With ``second=False`` the second moments are not computed and come back as 0."""
    d, C, chunk = int(d), int(C), int(chunk)
    n, dev = _check_rows(x, d, "nb moments"), x.device
    if labels.numel() != n or (weights is not None and weights.numel() != n):
        raise ValueError("nb moments: one label and weight per row are expected")
    labels = labels.reshape(-1).to(dev)
    w = None if weights is None else weights.reshape(-1).to(device=dev, dtype=torch.float64)
    m = None if shift is None else _f64(shift, dev).reshape(C, d)
    out = torch.zeros((C, 1 + 2 * d), dtype=torch.float64, device=dev)
    bad = torch.zeros(2, dtype=torch.float64, device=dev)
    ar = torch.arange(C, device=dev)
    for st in range(0, n, chunk):
        en = min(n, st + chunk)
        v = widen(x[st:en, :d])
        bad[0] += (v < 0).sum()
        bad[1] += ((v != 0) & (v != 1)).sum()
        lab = labels[st:en].long()
        hot = lab[:, None] == ar[None]
        oh = hot.to(torch.float64) if w is None else torch.where(hot, w[st:en, None], 0.0)
        if m is not None:
            inside = (lab >= 0) & (lab < C)
            v = v - torch.where(inside[:, None], m[lab.clamp(0, C - 1)], 0.0)
        out[:, 0] += oh.sum(0)
        out[:, 1:1 + d] += _class_sums(oh, v)
        if second:
            out[:, 1 + d:] += _class_sums(oh, v * v)
    return out, bad


def _lowest_argmax(r: torch.Tensor) -> torch.Tensor:
    C = r.shape[1]
    ar = torch.arange(C, device=r.device)
    idx = torch.where(r == r.max(1, keepdim=True).values, ar, torch.full_like(ar, C)).min(1).values
    return torch.where(idx == C, torch.zeros_like(idx), idx).to(torch.float64)


def finish_scores(s: torch.Tensor, kind: str):
    """``(raw, prob, pred)`` of the f64 scores ``s`` ``[rows, C]``."""
    dl = s - torch.logsumexp(s, 1, keepdim=True)
    raw = dl if kind == "complement" else s
    return raw, torch.exp(dl), _lowest_argmax(raw)


def _tables(kind: str, W, b, iv, d: int, dev):
    if kind not in KINDS:
        raise ValueError(f"nb scores: kind must be one of {KINDS}, got {kind!r}")
    W = _f64(W, dev)
    if W.dim() != 2 or W.shape[1] != d or W.shape[0] < 1:
        raise ValueError("nb scores: W [C, d] is expected")
    C = int(W.shape[0])
    b = torch.zeros(C, dtype=torch.float64, device=dev) if b is None or kind == "complement" \
        else _f64(b, dev).reshape(-1)
    if b.numel() != C:
        raise ValueError("nb scores: b [C] is expected")
    if kind == "gaussian":
        if iv is None:
            raise ValueError("nb scores: the gaussian kind needs iv = 1 / sigma")
        iv = _f64(iv, dev)
        if iv.shape != W.shape:
            raise ValueError("nb scores: iv [C, d] is expected")
    return W, b, iv, C


def scores_reference(x: torch.Tensor, d: int, kind: str, W, b, iv=None, chunk: int = CHUNK):
    """``(raw, prob, pred)`` of the rows ``x`` ``[n, >= d]`` of any dtype and device, one widened chunk at a time. The
    gaussian form loops over the classes with one ``chunk x d`` temporary: never ``n x C x d``."""
    d, chunk = int(d), int(chunk)
    n, dev = _check_rows(x, d, "nb scores"), x.device
    W, b, iv, C = _tables(kind, W, b, iv, d, dev)
    raw = torch.empty((n, C), dtype=torch.float64, device=dev)
    prob = torch.empty((n, C), dtype=torch.float64, device=dev)
    pred = torch.empty(n, dtype=torch.float64, device=dev)
    for st in range(0, n, chunk):
        en = min(n, st + chunk)
        v = widen(x[st:en, :d])
        if kind == "gaussian":
            s = torch.empty((en - st, C), dtype=torch.float64, device=dev)
            for c in range(C):
                t = v - W[c]
                s[:, c] = b[c] - 0.5 * t.mul_(t).mul_(iv[c]).sum(1)
        else:
            s = v @ W.T + b
        raw[st:en], prob[st:en], pred[st:en] = finish_scores(s, kind)
    return raw, prob, pred


# ---------------------------------------------------------------------------------------------------- kernel
_DETAIL = "16..512, with the classes inside the kernel's limits"


def moments(xd: torch.Tensor, d: int, labels: torch.Tensor, weights: Optional[torch.Tensor], C: int, shift=None,
            second: bool = True):
    """K34, moments form: ``(moments, bad)`` as ``moments_reference`` returns them, for bf16 device rows in the
    ``to_device_matrix`` layout. With ``second=False`` the second moments are not computed and come back as 0. All
    arithmetic after the exact bf16 -> f64 widening is f64 (the sums on the f64 MFMA); pad columns are masked by
    ``d``. Nothing of size n is written; no atomics, no host read; two calls return the same bits."""
    if not torch.is_tensor(xd) or xd.dim() != 2:
        raise ValueError("nb moments: rows must be a 2-d tensor")
    d, C = int(d), int(C)
    check_matrix(xd, d, lambda dtype, dp: kernel_supported(dtype, dp, (C, shift is not None)), "nb moments", _DETAIL)
    n, dp, dev = int(xd.shape[0]), int(xd.shape[1]), xd.device
    if not torch.is_tensor(labels) or labels.numel() != n or (weights is not None and weights.numel() != n):
        raise ValueError("nb moments: one label and weight per row are expected")
    cs = 1 + 2 * d
    out = torch.zeros(C * cs + 2, dtype=torch.float64, device=dev)
    if n:
        lab = labels.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        w = None if weights is None else weights.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
        m = None if shift is None else _f64(shift, dev).reshape(C, d).contiguous()
        lib, cus = _native.kernels(), ncu(dev)
        grid = int(lib.cml_nb_grid(n, dp, C, cus))
        part = torch.empty(int(lib.cml_nb_part(dp, C, d, grid)), dtype=torch.float64, device=dev)
        _native.check(lib.cml_nb_moments(xd.data_ptr(), n, dp, d, C, lab.data_ptr(), _native.ptr(w), _native.ptr(m),
                                         1 if second else 0, part.data_ptr(), grid, out.data_ptr(), cus,
                                         torch.cuda.current_stream(dev).cuda_stream), "nb_moments")
    return out[:C * cs].view(C, cs), out[C * cs:]


def scores(xd: torch.Tensor, d: int, kind: str, W, b, iv=None):
    """K34, scores form: ``(raw, prob, pred)`` as ``scores_reference`` returns them, for bf16 device rows in the
    ``to_device_matrix`` layout; each output is written once."""
    if not torch.is_tensor(xd) or xd.dim() != 2:
        raise ValueError("nb scores: rows must be a 2-d tensor")
    d = int(d)
    dev = xd.device
    W, b, iv, C = _tables(kind, W, b, iv, d, dev)
    gaussian = kind == "gaussian"
    check_matrix(xd, d, lambda dtype, dp: kernel_supported(dtype, dp, (C, gaussian)), "nb scores", _DETAIL)
    n, dp = int(xd.shape[0]), int(xd.shape[1])
    raw = torch.empty((n, C), dtype=torch.float64, device=dev)
    prob = torch.empty((n, C), dtype=torch.float64, device=dev)
    pred = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        if gaussian:  # [theta | iv | b], the columns zero padded to dp
            tab = torch.zeros(2 * C * dp + C, dtype=torch.float64, device=dev)
            tab[:C * dp].view(C, dp)[:, :d] = W
            tab[C * dp:2 * C * dp].view(C, dp)[:, :d] = iv
            tab[2 * C * dp:] = b
        else:         # [W | b], the classes zero padded to a multiple of 16 too
            c16 = (C + 15) // 16 * 16
            tab = torch.zeros(c16 * dp + c16, dtype=torch.float64, device=dev)
            tab[:c16 * dp].view(c16, dp)[:C, :d] = W
            tab[c16 * dp:c16 * dp + C] = b
        _native.check(_native.kernels().cml_nb_scores(xd.data_ptr(), n, dp, d, C, KINDS.index(kind), tab.data_ptr(),
                                                      raw.data_ptr(), prob.data_ptr(), pred.data_ptr(), ncu(dev),
                                                      torch.cuda.current_stream(dev).cuda_stream), "nb_scores")
    return raw, prob, pred
