"""The host-synchronised (torch-form) pruned Lloyd step of a LloydEngine: what host rows use, and device rows
without a K9r plan. Functions over the engine; the state lives in ``eng._pst`` (and ``eng._xn64`` for host rows).
``_PRUNE_TAU`` / ``_PRUNE_CAP`` stay class attributes of the engine and are read through it at call time."""
from __future__ import annotations

import math
import os
import types
from typing import Optional

import torch

from ..ops import kmeans_ops as K
from ..ops.group_ops import group_reduce
from ..utils.trace import trace

def _prune_init(eng) -> None:
    eng._ensure_norms()
    n, k, d, dev = eng.n, eng.k, eng.d, eng.device
    bdt = torch.float32 if eng.gpu else torch.float64
    idt = torch.int32 if eng.gpu else torch.int64
    st = types.SimpleNamespace(valid=False, last=(True, 0), history=[])
    st.ub = torch.full((max(n, 1),), float("inf"), dtype=bdt, device=dev)  # >= |x_i - c_label(i)|
    st.lb = torch.zeros(max(n, 1), dtype=bdt, device=dev)  # <= distance to the nearest other centre
    st.dmax = torch.zeros(3, dtype=bdt, device=dev)  # [largest drift, second largest, its index]
    st.cand = torch.zeros(max(n, 1), dtype=idt, device=dev)
    st.count = torch.zeros(1, dtype=idt, device=dev)
    st.L = torch.zeros(k * d + 2 * k, dtype=torch.float64, device=dev)  # local [Σx | count | Σ|x|²] per centre
    st.G = torch.zeros_like(st.L)  # all ranks' L summed (kept by adding the all-reduced deltas)
    st.drift = torch.zeros(k, dtype=bdt, device=dev)
    st.thr = torch.zeros(k, dtype=bdt, device=dev)
    if eng.gpu:
        xn = eng.xnorm[:n]
    else:
        eng._xn64 = (eng.x * eng.x).sum(1)
        xn = eng._xn64
    st.mx = eng.comm.max_scalar(float(xn.max()) if n else 0.0)
    if not eng.gpu and eng.labels is None:
        eng.labels = torch.zeros(max(n, 1), dtype=torch.int64)
    eng._pst = st


def _assign_centres64(eng) -> torch.Tensor:
    """The centres the assignment compares against (bf16-rounded on the GPU), as f64."""
    return eng.cb[: eng.k, : eng.d].to(torch.float64) if eng.gpu else eng.centers


def _prune_centre_stats(eng, old: Optional[torch.Tensor] = None) -> None:
    """drift[j] = |c_j - old_j| (rounded up) and thr[j] = half the distance from c_j to its nearest
    other centre less the slack that keeps a pruned row's label strictly best under the full
    assign's rounding: |x - c_j'|² - |x - c_j|² >= 4·s_j·(s_j - ub) >= 2·tau·(max|x|² + max|c|²)."""
    st = eng._pst
    c = _assign_centres64(eng)
    cn = (c * c).sum(1)
    st.cn = cn
    st.mc = float(cn.max()) if eng.k else 0.0
    st.c2 = 2.0 * eng._tau * (st.mx + st.mc)
    if old is not None:
        dr = (c - old).pow(2).sum(1).sqrt() * (1.0 + 1e-6)
        st.drift.copy_(dr)
        top = torch.topk(dr, min(2, eng.k))
        st.dmax.copy_(torch.stack([top.values[0], top.values[-1],
                                   top.indices[0].to(torch.float64)]).to(st.dmax.dtype))
    if eng.k > 1:
        d2 = (cn[:, None] + cn[None, :] - 2.0 * (c @ c.T)).clamp_(min=0.0)
        d2.fill_diagonal_(float("inf"))
        half = 0.5 * d2.min(1).values.sqrt()
        slack = eng._tau * (st.mx + st.mc) / (2.0 * half)
        thr = torch.where(half > 0, (half - slack) * (1.0 - 1e-6), torch.full_like(half, -math.inf))
    else:
        thr = torch.full((eng.k,), math.inf, dtype=torch.float64, device=eng.device)
    st.thr.copy_(thr)


def _prune_bound(eng, best: torch.Tensor, xn: torch.Tensor) -> torch.Tensor:
    """Upper bound on the exact distance from the assign's squared distance (rounded up)."""
    return (best.clamp(min=0) + eng._tau * (xn + eng._pst.mc)).sqrt() * (1.0 + 1e-6)


def _prune_lower(eng, xg: torch.Tensor, xng: torch.Tensor, lab: torch.Tensor, out: torch.Tensor,
                 chunk: Optional[int] = None) -> None:
    """out[i] = lower bound on the distance from row i to its nearest centre other than lab[i].
    GPU: one bf16 GEMM against the centres with f32 accumulation and f32 output (hipBLASLt), the
    label's column masked, min over centres; its rounding is that of the full assign, covered
    by subtracting tau·(|x|² + max|c|²) before the square root. CPU: the same in f64."""
    st, k = eng._pst, eng.k
    if eng.gpu:
        cbt = eng.cb[:k].t()
        cn = st.cn.to(torch.float32)
    else:
        cbt = eng.centers.t()
        cn = st.cn
    if chunk is None:  # [chunk, k] f32 blocks (CML_PRUNE_CHUNK_MB, default 512 MiB)
        chunk = max(1024, (int(os.environ.get("CML_PRUNE_CHUNK_MB", 512)) << 20) // (4 * max(k, 1)))
    for s0 in range(0, xg.shape[0], chunk):
        xc = xg[s0:s0 + chunk]
        xn = xng[s0:s0 + chunk].to(cn.dtype)
        if k > 1:
            if eng.gpu:
                if xc.dtype != torch.bfloat16:
                    xc = xc.to(torch.bfloat16)
                # |c_j|² - 2 x·c_j with the bias and scale in the GEMM epilogue (one f32 write)
                dist = torch.addmm(cn, xc, cbt, out_dtype=torch.float32, alpha=-2.0)
                if k % 4 == 0 and out.dtype == torch.float32:  # masked row min + bound in one pass
                    labc = lab[s0:s0 + chunk]
                    labc = labc if labc.dtype == torch.int32 else labc.to(torch.int32)
                    K.prune_lower(dist, labc.contiguous(), xn.contiguous(), st.mc, eng._tau,
                                  out[s0:s0 + chunk])
                    continue
            else:
                dist = torch.addmm(cn, xc, cbt, alpha=-2.0)
            dist.scatter_(1, lab[s0:s0 + chunk].long()[:, None], math.inf)
            sec = dist.min(1).values + xn
        else:
            sec = torch.full_like(xn, math.inf)
        lo = (sec - eng._tau * (xn + st.mc)).clamp_(min=0.0).sqrt_().mul_(1.0 - 1e-6)
        out[s0:s0 + chunk] = lo.to(out.dtype)


def _moved_sums(delta: torch.Tensor, k: int, d: int, xs: torch.Tensor, xq: torch.Tensor, new: torch.Tensor,
                old: torch.Tensor, chunk: int = 1 << 17, split: int = 64) -> None:
    """delta += the per-centre [Σx | count | Σ|x|²] change of rows moving old -> new: an f64 GEMM of
    a {-1, 0, +1} move matrix with [x | 1 | |x|²] (sums of bf16 / fp8 rows are exact in f64, so the
    result does not depend on the summation order; scatter-add atomics onto k rows serialise). The
    row dimension is split into ``split`` batches so the tiny k x (d + 2) output still spreads over
    every CU (one plain GEMM ran 4 workgroups: 14 ms per 128K rows)."""
    kd = k * d
    for s0 in range(0, xs.shape[0], chunk):
        nw, o = new[s0:s0 + chunk], old[s0:s0 + chunk]
        c = nw.shape[0]
        b = max(1, min(split, c // 256))
        cp = -(-c // b) * b
        w = torch.zeros((cp, k), dtype=torch.float64, device=xs.device)
        ar = torch.arange(c, device=xs.device)
        w[ar, nw] = 1.0
        w[ar, o] = -1.0
        v = torch.zeros((cp, d + 2), dtype=torch.float64, device=xs.device)
        v[:c, :d] = xs[s0:s0 + chunk]
        v[:c, d] = 1.0
        v[:c, d + 1] = xq[s0:s0 + chunk]
        part = torch.bmm(w.view(b, cp // b, k).transpose(1, 2), v.view(b, cp // b, d + 2)).sum(0)
        delta[:kd].view(k, d).add_(part[:, :d])
        delta[kd:kd + k].add_(part[:, d])
        delta[kd + k:].add_(part[:, d + 1])


def _step_prune(eng) -> None:
    """One exact Lloyd iteration: bounds pass (K9p), the rows it cannot prove are gathered and
    assigned against every centre (K9), the per-centre sums move by the rows whose label changed,
    and the deltas are all-reduced. A rank whose candidates exceed _PRUNE_CAP of its rows, or
    whose bounds are stale (first step, set_centers), assigns all of its rows instead; the
    collective sequence is the same either way."""
    if eng._pst is None:
        _prune_init(eng)
        _prune_centre_stats(eng)
    st = eng._pst
    n, k, d = eng.n, eng.k, eng.d
    full, m = not st.valid, n
    if not full and n:
        with trace("prune.bounds"):
            K.prune_bounds(eng.labels[:n], st.ub, st.lb, st.drift, st.dmax, st.thr, st.c2, k, st.cand,
                           st.count)
            m = int(st.count[0].item())
        full = m > eng._PRUNE_CAP * n
    with trace("prune.full" if full else "prune.candidates"):
        delta = _prune_local_full(eng) if full else _prune_local_cands(eng, m)
    st.last = (full, m)
    st.history.append((bool(full), int(m)))
    with trace("prune.allreduce_update"):
        _prune_apply(eng, delta)


def _prune_apply(eng, delta: torch.Tensor) -> None:
    st = eng._pst
    k, d = eng.k, eng.d
    eng.comm.allreduce_(delta)
    st.G += delta
    kd = k * d
    c = _assign_centres64(eng)
    s_, cnt, q = st.G[:kd].view(k, d), st.G[kd:kd + k], st.G[kd + k:]
    # cost of this assignment: Σ_j Σ_{i in j} |x_i - c_j|² = Σ_j (Q_j - 2 c_j·S_j + n_j |c_j|²)
    cost = (q.sum() - 2.0 * (c * s_).sum() + (cnt * st.cn).sum()).clamp(min=0.0)
    msg = torch.cat([st.G[:kd + k], cost.reshape(1)])
    old = c.clone()
    if eng.gpu:
        eng._cb_cost.copy_(eng.cb)  # exact cost on first read (the expanded form above cancels)
        eng._update_gpu(msg.view(1, -1))
        eng._cost_fn = eng._exact_cost
    else:
        eng._update_cpu(msg)
    st.valid = True
    with trace("prune.centre_stats"):
        _prune_centre_stats(eng, old)


def _prune_local_full(eng) -> torch.Tensor:
    st = eng._pst
    n, k, d = eng.n, eng.k, eng.d
    kd = k * d
    new = torch.zeros_like(st.L)
    if n and eng.gpu:
        msg, xc, lab, best = eng.msgs[0], eng.x[:n], eng.labels[:n], eng.best[:n]
        if eng.cplan.mode == "priv":
            K.assign_bf16(xc, n, eng.dp, eng.cb, eng.cnorm, eng.aplan, lab, best, eng.cost_part,
                          xnorm=eng.xnorm[:n])
            K.accumulate_priv(xc, n, lab, k, eng.cplan, eng.slab, eng.cslab)
            K.reduce_slabs(eng.slab, eng.cslab, eng.cost_part, eng.aplan.grid, k, d, eng.cplan, msg)
        else:
            rank = eng.rank[:n]
            K.assign_bf16(xc, n, eng.dp, eng.cb, eng.cnorm, eng.aplan, lab, best, eng.cost_part,
                          eng.hist, rank, xnorm=eng.xnorm[:n])
            K.accumulate_sort(xc, n, eng.dp, d, lab, rank, eng.hist, eng.aplan, k, eng.cost_part,
                              eng.off, eng.seg, eng.perm, eng.cplan, msg, eng.slots)
        new[:kd + k] = msg[:kd + k]
        new[kd + k:] = group_reduce(lab, eng.xnorm[:n], k, "sum")
        st.ub[:n] = _prune_bound(eng, best, eng.xnorm[:n])
        _prune_lower(eng, xc, eng.xnorm[:n], lab, st.lb)
    elif n:
        lab, best = K.assign_reference(eng.x, eng.centers)
        eng.labels = lab
        sums, counts = K.sums_reference(eng.x, lab, k)
        new[:kd] = sums.reshape(-1)
        new[kd:kd + k] = counts
        new[kd + k:].index_add_(0, lab, eng._xn64)
        st.ub[:n] = _prune_bound(eng, best, eng._xn64)
        _prune_lower(eng, eng.x, eng._xn64, lab, st.lb)
    delta = new - st.L
    st.L = new
    return delta


def _prune_local_cands(eng, m: int) -> torch.Tensor:
    st = eng._pst
    k, d = eng.k, eng.d
    delta = torch.zeros_like(st.L)
    if m == 0:
        return delta
    cand = st.cand[:m].long()
    with trace("prune.gather_assign"):
        xg, xng, labg, bestg = _prune_assign_rows(eng, cand, m)
    old = eng.labels[cand]
    labg = labg.to(old.dtype)
    eng.labels[cand] = labg
    st.ub[cand] = _prune_bound(eng, bestg, xng).to(st.ub.dtype)
    lo = torch.empty(m, dtype=st.lb.dtype, device=eng.device)
    with trace("prune.lower"):
        _prune_lower(eng, xg, xng, labg, lo)
    st.lb[cand] = lo
    with trace("prune.delta"):
        ch = torch.nonzero(labg != old).flatten()
        if ch.numel():
            o, nw = old[ch].long(), labg[ch].long()
            _moved_sums(delta, k, d, xg[ch, :d].to(torch.float64), xng[ch].to(torch.float64), nw, o)
    st.L += delta
    return delta


def _prune_assign_rows(eng, cand: torch.Tensor, m: int):
    """Gathered candidate rows, their |x|², labels and squared distances against every centre."""
    k = eng.k
    if eng.gpu:
        fp8 = K.is_fp8(eng.x)
        xg = eng.x.view(torch.uint8)[cand].view(eng.x.dtype) if fp8 else eng.x[cand]
        xng = eng.xnorm[cand]
        labg = torch.empty(m, dtype=torch.int32, device=eng.device)
        bestg = torch.empty(m, dtype=torch.float32, device=eng.device)
        plan = K.plan_assign(m, eng.dp, k, eng.device.index or 0, fp8=fp8)
        K.assign_bf16(xg, m, eng.dp, eng.cb, eng.cnorm, plan, labg, bestg, None, xnorm=xng)
    else:
        xg, xng = eng.x[cand], eng._xn64[cand]
        labg, bestg = K.assign_reference(xg, eng.centers)
    return xg, xng, labg, bestg
