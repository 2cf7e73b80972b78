"""k-means|| initialisation of a LloydEngine (and Spark's initMode="random"): functions over the engine.

What the init leaves for the fit stays on the engine: ``_seed`` (labels / costs that seed the first pruned
step's bounds), ``k_effective``, ``_gn`` (global row count), ``_init_prune_history`` and the candidate passes'
scratch ``_iscr`` (allocated once per engine)."""
from __future__ import annotations

import math
import os
import types

import numpy as np
import torch

from ..ops import kmeans_ops as K
from ..utils import rng
from ..utils.device import round_up
from ..utils.trace import trace

def init_random(eng, seed: int) -> np.ndarray:
    """Spark initMode="random": k distinct rows sampled uniformly without replacement."""
    ids = eng.row_ids()
    u = rng.uniform(ids, seed, stream=11)
    take = min(eng.k, eng.n)
    loc_u, loc_i = torch.topk(-u, take) if take > 0 else (u[:0], ids[:0].long())
    cand_u = -loc_u
    rows = _rows_f64(eng, loc_i)
    all_u = eng.comm.allgather_cat(cand_u.to(torch.float64))
    all_rows = eng.comm.allgather_cat(rows)
    order = torch.argsort(all_u)[: eng.k]
    return all_rows[order].cpu().numpy()


def _rows_f64(eng, idx: torch.Tensor) -> torch.Tensor:
    if eng._hs is not None:  # host rows
        return eng.x[idx.long().cpu(), : eng.d].to(torch.float64).to(eng.device)
    if eng.gpu:
        return eng.x[idx.long(), : eng.d].to(torch.float64)
    return eng.x[idx.long()].to(torch.float64)  # (the screen keeps f32 source rows)


def _min_dist_idx(eng, cands: torch.Tensor):
    """(squared distance to the nearest of `cands` as f64, its index) of every local row."""
    if eng._screen:
        return eng._screen_min_dist(cands)
    if not eng.gpu:
        lab, best = K.assign_reference(eng.x, cands)
        return best, lab
    eng._ensure_norms()
    lab, best = eng._assign_all(cands)
    return best.to(torch.float64), lab.long()


def init_kmeans_parallel(eng, seed: int, steps: int = 2, as_device: bool = False):
    """k-means|| (Bahmani et al.), Spark's default initMode (initSteps rounds sampling each row with
    probability 2k·cost/Σcost), then weighted local k-means++ + Lloyd on the distinct candidates.

    GPU ranks stay on the device: the first pass over X computes the row norms and the costs
    against the first centre together (K12 row pass), a round samples with one kernel over the
    costs, the new candidates' distances run on K9r in chunks of at most 256 centres merged into
    (cost, nearest candidate), and the local k-means runs as HIP kernels. The nearest candidate of
    every row is carried across rounds (strict improvement keeps the earlier candidate: argmin's
    first-index rule over the concatenated list), so the candidate weights need no extra pass.
    The GPU path reads the host only where a size decides the next launches: once per round (the
    sampled counts of every rank, one fixed-size all-gather) plus the pruned pass's row counts, the
    distinct-candidate count and the result — the first centre, Σcost and the sampling rate, the
    candidate weights and the local Lloyd's convergence stay on the device (~11 ms of
    init at the 8-GPU shard was mostly host round trips).
    The CPU path runs the same algorithm in f64, with the same distinct-candidate order (sorted
    rows) and the bitwise-identical local k-means (host twin of the kernels). ``as_device``: return
    the centres as the f64 device tensor (GPU engines; set_centers takes it without a host copy)."""
    if eng.gpu:
        with trace("kinit.gpu"):
            return _init_kmeans_parallel_gpu(eng, seed, steps, as_device)
    k = eng.k
    ids = eng.row_ids()
    gn = eng.global_n
    if gn == 0:
        raise ValueError("KMeans on an empty dataset")
    # first centre: one uniformly drawn global row (same draw on every rank)
    u = rng.uniform(ids, seed, stream=1)
    lu, li = (torch.min(u, 0) if eng.n else (torch.tensor(2.0, device=eng.device), torch.tensor(0)))
    first_u = eng.comm.allgather_cat(lu.reshape(1).to(torch.float64))
    owner = int(torch.argmin(first_u).item())
    row = (_rows_f64(eng, li.reshape(1)) if eng.n
           else torch.zeros((1, eng.d), dtype=torch.float64, device=eng.device))
    row = eng.comm.allgather(row)[owner] if eng.comm.is_distributed else row
    centers = [row.reshape(1, eng.d)]
    if eng.n:
        costs, nearest = _min_dist_idx(eng, centers[0])
    else:
        costs = torch.zeros(0, dtype=torch.float64, device=eng.device)
        nearest = torch.zeros(0, dtype=torch.int64, device=eng.device)
    ncand = 1
    for step in range(steps):
        local = float(costs[: eng.n].sum(dtype=torch.float64).item()) if eng.n else 0.0
        sum_cost = eng.comm.sum_scalar(local)
        if sum_cost <= 0:
            break
        us = rng.uniform(ids, seed, stream=100 + step)  # the sample kernel's test: u < scale·cost
        chosen = torch.nonzero(us < (2.0 * k / sum_cost) * costs).flatten()
        new = (_rows_f64(eng, chosen) if chosen.numel()
               else torch.zeros((0, eng.d), dtype=torch.float64, device=eng.device))
        new = eng.comm.allgather_cat(new)
        if new.shape[0] == 0:
            continue
        centers.append(new)
        if eng.n:
            d_new, i_new = _min_dist_idx(eng, new)
            better = d_new < costs
            costs = torch.where(better, d_new, costs)
            nearest = torch.where(better, i_new + ncand, nearest)
        ncand += new.shape[0]
    return _init_finish(eng, seed, centers, costs, nearest, as_device=False)


def _init_kmeans_parallel_gpu(eng, seed: int, steps: int, as_device: bool):
    k, n, d, dev, comm = eng.k, eng.n, eng.d, eng.device, eng.comm
    ids = eng.row_ids()
    ids64 = ids if ids.dtype == torch.int64 and ids.is_contiguous() else ids.to(torch.int64).contiguous()
    # first centre: the global row with the smallest counter uniform — one fixed-size all-gather of
    # [u_min, local rows, row] per rank, picked on the device (no host read)
    u = rng.uniform(ids, seed, stream=1)
    if n:
        lu, li = torch.min(u, 0)
        row = _rows_f64(eng, li.reshape(1)).reshape(-1)
    else:
        lu = torch.full((), 2.0, dtype=torch.float64, device=dev)
        row = torch.zeros(d, dtype=torch.float64, device=dev)
    hdr = torch.cat([lu.reshape(1).to(torch.float64),
                     torch.full((1,), float(n), dtype=torch.float64, device=dev), row])
    g = comm.allgather_fixed(hdr)
    gn_dev = g[:, 1].sum()
    # every candidate of every round lands in one f64 buffer, in Spark's order (first centre, then each
    # round's rows by rank and row id): the rounds and the finish read views of it, no concatenations
    cap = min(max(n, 1), max(4096, 8 * k))
    cands = torch.empty((1 + steps * 2 * cap if comm.is_distributed else 1 + steps * cap, d), dtype=torch.float64,
                        device=dev) if steps <= 4 else None
    if cands is None or cands.shape[0] > 65536:  # (many init steps: grow on demand instead)
        cands = torch.empty((1 + 4 * k + 1024, d), dtype=torch.float64, device=dev)
    cands[0].copy_(g[torch.argmin(g[:, 0]), 2:])
    c0 = cands[0:1]
    costs, nearest = _init_first_pass(eng, c0)
    xmax = eng._xmax_dev()
    ncand = 1
    two_k = eng._const([0.0, 2.0 * k], torch.float64)
    out = torch.empty(cap, dtype=torch.int32, device=dev)
    send = torch.empty((cap, d), dtype=torch.float64, device=dev) if comm.is_distributed else None
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    head = torch.empty(2, dtype=torch.float64, device=dev)
    for step in range(steps):
        with trace(f"kinit.round{step}"):
            # Σcost over every rank and the rate 2k / Σcost stay on the device (the sample kernel forms it)
            # (Σcost as integer limbs on the grid of 5·max||x||² — a row's squared distance to a candidate row is
            # at most 4·max||x||², plus the bf16 / MX rounding of the candidate — so the rate is the same bits
            # for any split of the rows over ranks: exactsum.hip)
            scale = two_k.clone()
            limbs = torch.zeros(2, dtype=torch.int64, device=dev)
            if n:
                K.fixsum(costs, n, xmax, 5.0, limbs=limbs)
            comm.allreduce_(limbs)
            K.fixsum_finalize(limbs, 1, xmax, 5.0, out=scale[0:1])
            cnt.zero_()
            if cands.shape[0] < ncand + (cap if send is None else 0):
                cands = _grow_cands(cands, ncand, ncand + cap)
            gathered = False
            if n:
                K.init_sample(costs, ids64, n, rng.key(seed, 100 + step), scale, out, cnt)
                # the sampled rows in row order, widened to f64, before the host read (device count)
                if eng._hs is None:  # (host rows of an out-of-core engine: the gather below)
                    gathered = K.gather_rank_rows(eng.x, out, cnt, cap, d, cands[ncand:] if send is None else send)
            # the one host read of the round: every rank's sampled count (and, once, the global row count)
            head[0:1].copy_(cnt)
            head[1:2].copy_(gn_dev.reshape(1))
            hv = comm.allgather_fixed(head).cpu()
            counts = [int(v) for v in hv[:, 0].tolist()]
            if step == 0:
                eng._gn = int(hv[0, 1].item())
                if eng._gn == 0:
                    raise ValueError("KMeans on an empty dataset")
            m = counts[comm.rank]
            if m > cap:  # rare: more than the expected ~2k·(share of the cost) rows; sample again with room
                out = torch.empty(m, dtype=torch.int32, device=dev)
                cnt.zero_()
                K.init_sample(costs, ids64, n, rng.key(seed, 100 + step), scale, out, cnt)
                cap, gathered = m, False
            mt = sum(counts)
            if cands.shape[0] < ncand + mt:
                cands = _grow_cands(cands, ncand, ncand + mt)
            dst = send if send is not None else cands[ncand:]
            if m and not gathered:
                chosen = torch.sort(out[:m]).values.long()
                if send is not None and send.shape[0] < m:
                    send = dst = torch.empty((m, d), dtype=torch.float64, device=dev)
                dst[:m].copy_(_rows_f64(eng, chosen))
            if send is not None:
                pad = max(max(counts), 1)
                if send.shape[0] < pad:  # (a small shard's buffer is sized by its own rows: every rank sends pad)
                    grown = torch.zeros((pad, d), dtype=torch.float64, device=dev)
                    grown[:m].copy_(send[:m])
                    send = grown
                gath = comm.allgather_fixed(send[:pad])
                at = ncand
                for r in range(comm.world_size):
                    if counts[r]:
                        cands[at:at + counts[r]].copy_(gath[r, :counts[r]])
                    at += counts[r]
            if mt == 0:
                continue
            new = cands[ncand:ncand + mt]
            # bf16 copies and norms of every new candidate in one K11 launch; each K9r chunk is a view of them
            # (rows past mt: zero centres with +inf norms, which no row takes)
            dp = eng.dp
            kp_all = round_up(mt, 64)
            cbn = torch.empty((kp_all, dp), dtype=torch.bfloat16, device=dev)
            cnn = torch.empty(kp_all, dtype=torch.float32, device=dev)
            K.update_centers(None, mt, d, new, cbn, dp, kp_all, cnn, None, snap=eng._mx)
            # once most rows sit near a candidate, only the new candidates close to a row's nearest one
            # can take it over (_init_candidate_pass_pruned): the second round at once; in the first
            # round (only the first centre so far) everything after the first K9r chunk
            first = _first_chunk(eng, mt) if step == 0 else 0
            if first:
                _init_candidate_pass(eng, first, cbn, cnn, 0, costs, nearest, ncand)
            if mt > first and not _init_candidate_pass_pruned(
                    eng, cands[:ncand + first], new[first:], cbn, cnn, first, costs, nearest, ncand + first):
                _init_candidate_pass(eng, mt - first, cbn, cnn, first, costs, nearest, ncand + first)
            ncand += mt
    with trace("kinit.finish"):
        return _init_finish(eng, seed, cands[:ncand], costs, nearest, as_device=as_device)


def _grow_cands(cands: torch.Tensor, used: int, need: int) -> torch.Tensor:
    out = torch.empty((max(need, 2 * cands.shape[0]), cands.shape[1]), dtype=cands.dtype, device=cands.device)
    out[:used].copy_(cands[:used])
    return out


def _init_finish(eng, seed: int, centers: list, costs: torch.Tensor, nearest: torch.Tensor, as_device: bool):
    """Distinct candidates, their weights (rows per candidate, all-reduced) and the local k-means."""
    k = eng.k
    cand = centers if torch.is_tensor(centers) else torch.cat(centers, 0)
    # distinct candidates in sorted-row order (np.unique's order; identical on every device)
    uniq, inverse = K.unique_rows(cand) if cand.is_cuda else torch.unique(cand, dim=0, return_inverse=True)
    if uniq.shape[0] <= k:
        out = uniq
    else:
        if eng.n and eng.w is not None:
            # summed row weights per candidate (deterministic f64 sums, as the Lloyd sums)
            w = K.sums_reference(eng.w[:, None], inverse.reshape(-1)[nearest[: eng.n].long()],
                                 uniq.shape[0])[0][:, 0].contiguous()
        elif eng.n:
            # rows per candidate (an int32 histogram of the nearest ids: integer counts, exact in any
            # order), folded onto the distinct candidates
            if eng.gpu or nearest.is_cuda:  # device rows (bf16 path or the screen): no bincount sync
                per_i = torch.zeros(cand.shape[0], dtype=torch.int32, device=eng.device)
                near32 = nearest if nearest.dtype == torch.int32 else nearest[: eng.n].to(torch.int32)
                K.int_hist(near32.contiguous(), eng.n, cand.shape[0], per_i)
                per = per_i.to(torch.float64)
            else:
                per = torch.bincount(nearest[: eng.n], minlength=cand.shape[0]).to(torch.float64)
            w = torch.zeros(uniq.shape[0], dtype=torch.float64, device=eng.device)
            w.index_add_(0, inverse.reshape(-1), per)
        else:
            w = torch.zeros(uniq.shape[0], dtype=torch.float64, device=eng.device)
        eng.comm.allreduce_(w)
        # unweighted: the weights are row counts summing to the global row count, which is positive
        # (the candidates are rows), so local_kmeans skips its clamp and all-zero fallback
        out = K.local_kmeans(uniq, w, k, seed, max_iter=30, spherical=eng.spherical, counts=eng.w is None)
        if eng.comm.is_distributed:
            # every rank ran the same local k-means on the same candidates and weights; rank 0's
            # result is taken verbatim (one source of truth for the centres every rank starts from)
            out = eng.comm.broadcast_(out.contiguous(), 0)
    nk = int(out.shape[0])
    if nk < k:
        # Spark may return fewer centres when there are < k distinct points; pad by repetition so the
        # device buffers keep their shape, and record the real count.
        eng.k_effective = nk
        out = torch.cat([out, out[-1:].expand(k - nk, -1)], 0)
    else:
        eng.k_effective = k
    out = out.to(torch.float64).contiguous()
    if eng._pdev and eng.n and eng.k_effective == k and os.environ.get("CML_KMEANS_SEED_BOUNDS", "1") != "0":
        # what the first Lloyd step needs to start from bounds instead of a full pass (set_centers)
        eng._seed = types.SimpleNamespace(nearest=nearest, costs=costs, inverse=inverse, uniq=uniq, out=out,
                                           out_np=None)
    if as_device and eng.gpu:
        return out
    res = out.cpu().numpy()
    if eng._seed is not None and eng._seed.out is out:
        eng._seed.out_np = res
    return res


def _init_first_pass(eng, c0: torch.Tensor):
    """(cost f32, nearest i32) of every local row against the first centre, from the row pass that
    also fills the norms (one read of X; a second read only if the norms were cached already). The
    centre's bf16 norm reaches the kernel on the device."""
    n, d, dp, dev = eng.n, eng.d, eng.dp, eng.device
    # K11 writes every row of the 32-row block (zero rows, +inf norms past the first) and rewrites the
    # f64 centre with its own value: no clears, no copy of c0
    cb0 = torch.empty((32, dp), dtype=torch.bfloat16, device=dev)
    cn0 = torch.empty(32, dtype=torch.float32, device=dev)
    c0 = c0.reshape(1, d)
    if c0.dtype != torch.float64 or not c0.is_contiguous():
        c0 = c0.to(torch.float64).contiguous()
    K.update_centers(None, 1, d, c0, cb0, dp, 32, cn0, None, snap=eng._mx)
    alloc = torch.empty if n else torch.zeros  # (the row pass writes every row's cost and nearest)
    costs = alloc(max(n, 1), dtype=torch.float32, device=dev)
    nearest = alloc(max(n, 1), dtype=torch.int32, device=dev)
    eng._row_pass(cb0[0].to(torch.float32).contiguous(), 0.0, costs, nearest, c0n_dev=cn0[0:1])
    return costs, nearest


def _init_scratch(eng):
    """Per-engine scratch of the k-means|| candidate passes (allocated once; the K9r passes write every
    entry they read back, so nothing is cleared per round)."""
    sc = eng._iscr
    if sc is None:
        n, dev = eng.n, eng.device
        tr = eng.aplan.round_rows
        sc = types.SimpleNamespace()
        sc.lab = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        sc.best = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        sc.list_a = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
        # list B is read in whole K9r tiles: entries past the count must be valid row ids (zeros once)
        sc.list_b = torch.zeros(n + tr, dtype=torch.int32, device=dev)
        sc.cxn = torch.zeros(n + tr, dtype=torch.float32, device=dev)
        sc.lab_in = torch.full((n + tr,), -1, dtype=torch.int32, device=dev)
        sc.cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        eng._iscr = sc
    return sc


def _init_candidate_pass(eng, m: int, cbn: torch.Tensor, cnn: torch.Tensor, c_off: int, costs: torch.Tensor,
                         nearest: torch.Tensor, off: int) -> None:
    """Merge the distances to the candidates cbn[c_off : c_off + m] (bf16 copies, norms cnn; K9r, at
    most 320 centres per launch) into (cost, nearest); candidate i is global index off + i."""
    n, dp, dev = eng.n, eng.dp, eng.device
    if n == 0:
        return
    sc = _init_scratch(eng)
    lab, best = sc.lab[:n], sc.best[:n]
    xn = eng.xnorm
    parts, c0 = [], 0
    for size in _candidate_chunks(eng, m):
        kp = round_up(size, 32)
        parts.append((c0, size, cbn[c_off + c0:c_off + c0 + kp], cnn[c_off + c0:c_off + c0 + kp]))
        c0 += size
    # rows outer (one read of X per pass, streamed out of core), candidate chunks inner: the merges
    # of a row run in candidate order either way
    for _, r0, r1, xc in eng._x_chunks(whole=True):
        mm = r1 - r0
        if mm == 0:
            continue
        for c0, kc, cb, cn in parts:
            plan = K.plan_assign(mm, dp, kc, dev.index or 0, fp8=K.is_fp8(eng.x))
            K.assign_bf16(xc, mm, dp, cb, cn, plan, lab[r0:r1], best[r0:r1], None, xnorm=xn[r0:r1])
            K.init_merge(costs[r0:r1], nearest[r0:r1], best[r0:r1], lab[r0:r1], off + c0, mm)


_INIT_LMAX = 8  # relevant new candidates a row may have to take the per-row path (else the K9r pass)


def _init_candidate_pass_pruned(eng, prev: torch.Tensor, new: torch.Tensor, cbn: torch.Tensor,
                                cnn: torch.Tensor, c_off: int, costs: torch.Tensor, nearest: torch.Tensor,
                                off: int) -> bool:
    """A k-means|| candidate pass that skips what the triangle inequality rules out: a row at distance
    r from its nearest candidate p can only move to a new candidate y with |p - y| < 2r. With the
    distances from every existing candidate to the new ones sorted (a small f64 table), each row
    counts its relevant candidates (kmeans init_classify); rows with none are done, rows with at
    most _INIT_LMAX get those distances from a per-row kernel, the rest run the K9r candidate pass
    over their positions (mode 2). Same nearest candidates as the full pass up to the rounding of
    near-ties. No host read: the list sizes stay on the device (the launches are sized by capacity).
    ``new`` (f64) are the candidates whose bf16 copies / norms are cbn / cnn[c_off:]; candidate i is
    global index off + i. Returns False (nothing changed) when the pruned pass does not apply (host rows,
    pruning off)."""
    n, d, dp, dev = eng.n, eng.d, eng.dp, eng.device
    # default on up to Dp = 256; at Dp = 512 the per-row path reads 1 KiB of candidate per listed
    # candidate and the gathered K9r pass loses to the streaming one: the config-5 pipeline's init
    # (125M x 512 fp8, k = 128) ran 120 ms pruned vs 97.5 ms full (profiles/r4/pipeline_init_ab.log)
    mode = os.environ.get("CML_KMEANS_INIT_PRUNE", "auto")
    if mode == "0" or (mode == "auto" and dp > 256):
        return False
    if not eng._pdev or not K.rr_max_chunk(eng.dp, K.is_fp8(eng.x)):
        return False
    if n == 0:
        return True
    m = int(new.shape[0])
    tab = K.init_table(prev, new)  # one launch: direct-difference distances, sorted in LDS
    if tab is not None:
        tab_v, tab_j, pn32 = tab
    else:
        P = prev.to(device=dev, dtype=torch.float64)
        Y = new.to(device=dev, dtype=torch.float64)
        pn, yn = (P * P).sum(1), (Y * Y).sum(1)
        d2 = pn[:, None] + yn[None, :] - 2.0 * (P @ Y.T)
        eps = 1e-12 * (pn.max() + yn.max())  # device scalar (no host read)
        vals, order = torch.sort((d2 - eps).clamp_(min=0.0).sqrt_().mul_(1.0 - 1e-6), dim=1)
        tab_v = vals.to(torch.float32).contiguous()
        tab_j = order.to(torch.int32).contiguous()
        pn32 = (pn * (1.0 + 1e-6)).to(torch.float32).contiguous()
    tau = 2.0 * eng._tau
    sc = _init_scratch(eng)
    list_a, list_b, cnt = sc.list_a, sc.list_b, sc.cnt
    cnt.zero_()
    # per-row path limit: each listed candidate costs the row a read of its dp-wide bf16 copy from L2
    # (1 KiB at dp = 512), so wide rows hand longer lists to the MFMA pass sooner
    lmax = int(os.environ.get("CML_KMEANS_INIT_LMAX", _INIT_LMAX if dp <= 256 else 4))
    lmax = max(0, min(_INIT_LMAX, lmax))
    K.init_classify(costs, nearest, eng.xnorm, pn32, tab_v, tau, n, lmax, list_a, cnt[0:1], list_b, cnt[1:2])
    # no host read of the list sizes: the per-row kernel and the K9r candidate pass take them from the
    # device and size their grids by the capacity (dead tiles exit at once); the new candidates' bf16
    # rows are the K11 copies the K9r chunks use
    K.init_near_list(eng.x, dp, costs, nearest, eng.xnorm, pn32, tab_v, tab_j, cbn[c_off:c_off + m], off, tau,
                     list_a, cnt[0:1], n)
    st = eng._pst
    cxn = sc.cxn
    torch.index_select(eng.xnorm[:n], 0, list_b[:n], out=cxn[:n])  # entries past the count: row 0's, unread
    c0 = 0
    for size in _candidate_chunks(eng, m):
        kp = round_up(size, 32)
        cbk, cnk = cbn[c_off + c0:c_off + c0 + kp], cnn[c_off + c0:c_off + c0 + kp]
        plan = K.plan_assign(n, dp, size, dev.index or 0, fp8=K.is_fp8(eng.x))
        mc = cnk[:size].max().reshape(1)
        K.assign_rr_ext(2, eng.x, n, dp, cbk, cnk, plan, cxn, eng.labels, None, st.ub, st.lb, mc,
                        eng._tau, idx=list_b, n_dev=cnt[1:2], lab_in=sc.lab_in, merge_cost=costs,
                        merge_near=nearest, merge_off=off + c0)
        c0 += size
    if eng.track_prune:
        ca, cb = (int(v) for v in cnt.tolist())
        eng._init_prune_history.append((n, ca, cb))
    return True


# Time of one K9r pass over 20M x 256 bf16 rows by centre tiles per compute wave (64 centres each),
# ms, measured on MI355X (profiles/r3/mb_rr_modes.log): CT <= 2 is HBM-bound, then the MFMA work
# grows with CT (under the power-limited clock, not linearly).
_CT_COST = {1: 1.72, 2: 1.78, 3: 2.06, 4: 2.45, 5: 2.78}


def _first_chunk(eng, m: int) -> int:
    """Candidates of the first k-means|| round that take a full K9r pass before the rest are pruned
    against them (CML_KMEANS_INIT_FIRST caps it, a multiple of 64; default: the first chunk of
    _candidate_chunks)."""
    first = _candidate_chunks(eng, m)[0]
    cap = os.environ.get("CML_KMEANS_INIT_FIRST")
    if cap:
        first = min(first, max(64, int(cap) // 64 * 64), m)
    return first


def _candidate_chunks(eng, m: int) -> list:
    """Split m candidate centres into K9r launches (multiples of 64, at most 256 — 320 where CT = 5
    exists) minimising the summed pass cost: 520 candidates run as 256 + 264 (two passes, ~27.5)
    rather than 256 + 256 + 8 (three, ~34)."""
    big = K.rr_max_chunk(eng.dp, K.is_fp8(eng.x)) or 256  # 256: K9 launches (no K9r plan at this width)
    units = -(-m // 64)
    best = [0.0] + [math.inf] * units  # best[u]: cheapest cover of u units of 64
    pick = [0] * (units + 1)
    for u in range(1, units + 1):
        for c in range(1, big // 64 + 1):
            v = best[max(0, u - c)] + _CT_COST.get(c, 20.0)
            if v < best[u]:
                best[u], pick[u] = v, c
    sizes, u = [], units
    while u > 0:
        sizes.append(pick[u] * 64)
        u = max(0, u - pick[u])
    sizes.sort(reverse=True)
    sizes[-1] -= sum(sizes) - m  # the last chunk takes the remainder
    return [s for s in sizes if s > 0]
