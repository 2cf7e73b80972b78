"""One restricted 2-means iteration of BisectingKMeans: the reference form and the host wrapper of K27
(``_native/csrc/bisect.hip``).

A level divides ``m`` nodes together. Every row of a divided node (its ``slot``, 0 <= slot < m; -1: the row's node
is not divided and the row is never read) chooses between the two children of its own node:

* euclidean: ``d_h(x) = |x − c_h|²``; cosine: ``d_h(x) = 1 − x·c_h / |x|`` (unit-length ``c_h``)
* right iff ``d_R < d_L`` (left on ties); a child that is not ``alive`` is at ``+inf``; a node without a live
  child keeps its rows (choice 0, no statistics)

and the children collect ``[S | W | Q | N]`` as one f64 ``[2m, d + 3]`` tensor (row ``2·slot + child``):
``S = Σ ω x`` with ``ω = w`` (cosine: ``w / |x|``), ``W = Σ w``, ``Q = Σ w |x|²`` (cosine: 0) and ``N`` the number
of rows (a row of weight 0 counts 1).

``bisect_step_reference`` evaluates this in f64 torch, chunk by chunk, on any device and dtype: the path of CPU
frames, f32 / f64 columns, host-resident columns and unsupported widths, and the oracle of the kernel.
``bisect_step`` is the gfx950 kernel for bf16 / e4m3 rows in the ``to_device_matrix`` layout
(``kernel_supported``): one launch reads every listed row once, a small second launch adds the partials of the
nodes that span several units. ``CML_BISECT_KERNEL=0`` keeps the estimator on the reference form.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from . import silhouette_ops as SO
from ._fused import env_enabled

_native.register_kernel_sigs({
    "cml_bisect_step": (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_ll, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
})

CHUNK = 1 << 16
M_MAX = 1 << 20  # nodes divided on one level (k - 1 at the most)


def kernel_enabled() -> bool:
    return env_enabled("CML_BISECT_KERNEL")


def kernel_supported(dtype: torch.dtype, dp: int) -> bool:
    """Whether K27 takes rows of this dtype and padded width (anything else: the reference form).
    bf16: 16 <= dp <= 512; e4m3: dp in {256, 512}."""
    if dtype == torch.bfloat16:
        return dp in (16, 32, 64, 128, 256, 512)
    if dtype == torch.float8_e4m3fn:
        return dp in (256, 512)
    return False


# ---------------------------------------------------------------------------------------------- reference form
def bisect_step_reference(x: torch.Tensor, slot: torch.Tensor, centres: torch.Tensor, alive: torch.Tensor,
                          weights: Optional[torch.Tensor] = None, cosine: bool = False, want_sums: bool = True,
                          chunk: int = CHUNK):
    """One iteration over this rank's rows: ``(choice, stats)``. ``slot`` ``[n]`` integer (-1: not listed),
    ``centres`` ``[m, 2, d]`` (a dead child's row is ignored), ``alive`` ``[m, 2]`` bool, ``weights`` f64 per row
    or None. ``choice`` is int8 ``[n]`` (0 where the row is not listed), ``stats`` f64 ``[2m, d + 3]`` (None
    when ``want_sums`` is false). A zero-length row is the caller's to refuse for cosine. No host read: rows that
    are not listed are masked, not skipped."""
    n, d = int(x.shape[0]), int(x.shape[1])
    m = int(centres.shape[0])
    dev = x.device
    C = torch.nan_to_num(centres.to(device=dev, dtype=torch.float64))
    al = alive.to(device=dev, dtype=torch.bool)
    choice = torch.zeros(n, dtype=torch.int8, device=dev)
    stats = torch.zeros(2 * m, d + 3, dtype=torch.float64, device=dev) if want_sums else None
    if m == 0:
        return choice, stats
    inf = float("inf")
    for st in range(0, n, chunk):
        sl = slot[st:st + chunk].to(torch.int64)
        listed = sl >= 0
        s = sl.clamp(min=0)
        v = x[st:st + chunk].to(torch.float64)
        v = torch.where(listed[:, None], v, torch.zeros_like(v))
        xx = (v * v).sum(1)
        if cosine:
            nrm = torch.where(xx > 0, xx.sqrt(), torch.ones_like(xx))
            dl = 1.0 - (v * C[s, 0]).sum(1) / nrm
            dr = 1.0 - (v * C[s, 1]).sum(1) / nrm
        else:
            dl = ((v - C[s, 0]) ** 2).sum(1)
            dr = ((v - C[s, 1]) ** 2).sum(1)
        dl = torch.where(al[s, 0], dl, torch.full_like(dl, inf))
        dr = torch.where(al[s, 1], dr, torch.full_like(dr, inf))
        act = listed & (al[s, 0] | al[s, 1])
        go = (dr < dl) & act
        choice[st:st + chunk] = go.to(torch.int8)
        if not want_sums:
            continue
        w = (torch.ones_like(xx) if weights is None else weights[st:st + chunk].to(device=dev, dtype=torch.float64))
        w = torch.where(act, w, torch.zeros_like(w))
        if cosine:
            feat = v * (w / nrm)[:, None]
            q = torch.zeros_like(xx)
        else:
            feat = v * w[:, None]
            q = w * xx
        part = torch.cat([feat, w[:, None], q[:, None], act.to(torch.float64)[:, None]], 1)
        stats.index_add_(0, torch.where(act, 2 * s + go.to(torch.int64), torch.zeros_like(s)), part)
    return choice, stats


# ---------------------------------------------------------------------------------------------------- kernel
class BisectPlan:
    """The rows of one level in (node slot, row) order: ``perm`` i64 ``[npos]`` (the row of every position),
    ``pslot`` i32 ``[npos]`` (its node slot, ascending) and ``off`` i64 ``[m + 1]`` (the first position of every
    slot). Built once per level (``make_plan``); rows of undivided nodes are not in it."""

    __slots__ = ("perm", "pslot", "off", "m", "npos", "n", "L")

    def __init__(self, perm, pslot, off, m, n):
        self.perm, self.pslot, self.off, self.m, self.n = perm, pslot, off, m, n
        self.npos = int(perm.shape[0])
        self.L = 256 if self.npos < (1 << 20) else 1024


def make_plan(slot: torch.Tensor, m: int) -> BisectPlan:
    """The plan of a level from the per-row node slot (integer ``[n]``, -1: not divided on this level). A
    stable sort by slot keeps the rows of a node in row order, so the order of every sum is fixed by the data."""
    n = int(slot.shape[0])
    if not 0 < m <= M_MAX:
        raise ValueError(f"bisect plan: m = {m} outside (0, {M_MAX}]")
    if n:
        hi = int(slot.max())  # the kernel indexes [m] tables by slot: never launch out of range
        if hi >= m:
            raise ValueError(f"bisect plan: slots outside [-1, {m})")
    pos = torch.nonzero(slot >= 0).flatten()
    ps, order = torch.sort(slot[pos].to(torch.int32), stable=True)
    perm = pos[order].contiguous()
    off = torch.searchsorted(ps, torch.arange(m + 1, dtype=torch.int32, device=slot.device)).to(torch.int64)
    return BisectPlan(perm, ps.contiguous(), off.contiguous(), m, n)


def bisect_step(xd: torch.Tensor, plan: BisectPlan, centres: torch.Tensor, alive: torch.Tensor,
                omega: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None,
                nrm2: Optional[torch.Tensor] = None, cosine: bool = False, want_sums: bool = True):
    """K27: ``(choice, stats)`` of one iteration. ``choice`` is uint8 per POSITION of the plan (``plan.perm``
    names the row), ``stats`` f64 ``[2m, dp + 3]`` (None when ``want_sums`` is false). ``centres`` ``[m, 2, dp]``
    f64, zero padded; ``alive`` ``[m, 2]``; per ROW (f64 ``[n]``): ``omega`` the factor of S (None = 1),
    ``weights`` (None = 1) and ``nrm2 = |x|²`` (``silhouette_ops.row_sqnorm``; needed for euclidean sums).
    The decision is the single dot product ``2 x·(c_R − c_L) > |c_R|² − |c_L|²`` (cosine: ``x·(c_R − c_L) > 0``),
    in f64 on the exact values of the rows. No atomics; two calls return the same bits."""
    if not xd.is_cuda or xd.dim() != 2 or not xd.is_contiguous() or not kernel_supported(xd.dtype, int(xd.shape[1])):
        raise ValueError("bisect_step: rows must be a contiguous bf16 / e4m3 device matrix of a supported width")
    n, dp = int(xd.shape[0]), int(xd.shape[1])
    m, npos = plan.m, plan.npos
    dev = xd.device
    if plan.n != n or tuple(centres.shape) != (m, 2, dp) or tuple(alive.shape) != (m, 2):
        raise ValueError("bisect_step: plan, centres and alive do not fit the rows")
    choice = torch.zeros(npos, dtype=torch.uint8, device=dev)
    stats = torch.zeros(2 * m, dp + 3, dtype=torch.float64, device=dev) if want_sums else None
    if npos == 0:
        return choice, stats
    per_row = []
    for t in (omega, weights, nrm2):
        if t is not None:
            t = t.to(device=dev, dtype=torch.float64).contiguous()
            if t.shape[0] != n:
                raise ValueError("bisect_step: a per-row factor differs in length from the rows")
        per_row.append(t)
    omega, weights, nrm2 = per_row
    if want_sums and not cosine and nrm2 is None:
        raise ValueError("bisect_step: euclidean sums need the row norms")
    C = centres.to(device=dev, dtype=torch.float64)
    al = alive.to(device=dev, dtype=torch.int32).contiguous()
    live = al.to(torch.bool)
    C = torch.where(live[:, :, None], torch.nan_to_num(C), torch.zeros_like(C))
    delta = (C[:, 1] - C[:, 0]).contiguous()
    thr = (torch.zeros(m, dtype=torch.float64, device=dev) if cosine
           else ((C[:, 1] * C[:, 1]).sum(1) - (C[:, 0] * C[:, 0]).sum(1)).contiguous())
    L = plan.L
    nunits = -(-npos // L)
    if want_sums:
        head = torch.empty(nunits, 2, dp + 3, dtype=torch.float64, device=dev)
        tail = torch.empty(nunits, 2, dp + 3, dtype=torch.float64, device=dev)
        hl = torch.empty(nunits, 2, dtype=torch.int32, device=dev)
    else:
        head = tail = hl = None
    stream = torch.cuda.current_stream(dev).cuda_stream
    _native.check(_native.kernels().cml_bisect_step(
        xd.data_ptr(), n, dp, dp, SO._DTYPE_CODE[xd.dtype], npos, plan.perm.data_ptr(), plan.pslot.data_ptr(),
        plan.off.data_ptr(), _native.ptr(omega), _native.ptr(weights), _native.ptr(nrm2), delta.data_ptr(),
        thr.data_ptr(), al.data_ptr(), m, L, 1 if cosine else 0, 1 if want_sums else 0, choice.data_ptr(),
        _native.ptr(stats), _native.ptr(head), _native.ptr(tail), _native.ptr(hl), stream), "bisect_step")
    return choice, stats
