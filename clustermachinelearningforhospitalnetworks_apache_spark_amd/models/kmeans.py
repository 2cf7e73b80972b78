"""Distributed Lloyd engine for KMeans (the north-star workload, BASELINE.json).

The reference contains no KMeans; semantics follow Spark MLlib's
KMeans defaults: k-means|| initialisation with initSteps=2,
maxIter=20, tol=1e-4 (converged when every centre moved ≤ tol), empty clusters
keep their previous centre, trainingCost = cost of the last iteration's
assignment.

Per iteration on each rank (E5 in SURVEY.md §3):

    for chunk c of the local HBM-resident shard:
        K9  assign  (MFMA distance GEMM + argmin, centres LDS-resident)
        K10 accumulate (LDS-privatised per-cluster sums) -> K10b reduce -> msg[c]
        RCCL all-reduce(msg[c]) enqueued asynchronously — it runs on the
        process group's stream while chunk c+1's distance GEMM runs
    K11 update from Σ_c msg[c]  (the only exposed collective is the last chunk's)

Incremental sums (default on the sort regime): the per-cluster sums of the current labels are kept
across steps; a step re-reads only the rows whose label changed (new sums = old + moved in − moved
out, exact in f64 for bf16/fp8 rows), falling back to the full accumulate on the first step and
whenever more than 1/4 of the rows changed (CML_KMEANS_DELTA_CAP). Every step still assigns every row against every centre.

Pruned steps (``prune=True`` / ``CML_KMEANS_PRUNE=1``, opt-in): the exact bound-pruned form of the
same iteration (``_step_prune_dev``; ``kmeans_prune_host._step_prune``). Spark's own findClosest skips centres the triangle inequality rules
out (mllib/clustering/DistanceMeasure.scala); here a per-row upper bound on the distance to the
assigned centre is carried across iterations (Hamerly), so rows whose bound proves the label are not
read at all and only the others are re-assigned against every centre. Labels, sums and centres are
those of the full step (tests/test_kmeans_prune.py); the headline bench keeps the full assignment.

Weighted fits (``weights``, Spark's weightCol) run the source-precision path by default; with
``precision="bf16"`` device rows stay bf16 / e4m3 and the step is K9 / K9r, the counting sort and the
weighted double-double sums of ``kmeans_weighted.hip`` (``_step_weighted``): unpruned, full steps, one
row chunk. Its sums are the exact sums of the rounded products fl64(w·x), correctly rounded, so they do
not depend on the order, the slicing or the number of ranks while the products of a column span fewer
than about 106 - 53 - ceil(log2 n) binary orders (the source-precision weighted sums' own contract);
beyond that the result is still deterministic for a fixed partition.

CPU tensors run the same algorithm with torch float64 ops (``local[n]`` mode and
the numerical oracle).

Where the parts live: this module holds ``LloydEngine`` — the constructor, the step dispatch, the MFMA steps
(full, weighted, screened exact, device pruned with its launch replay), the graph wrapper, the CPU step and the
cost readers. ``kmeans_route.py`` decides the path from the constructor's arguments (``resolve_route``, a pure
function; the plan-dependent second stage is the block at the top of ``_alloc_gpu``); ``kmeans_init.py`` is
k-means|| and the random init; ``kmeans_prune_host.py`` the host-synchronised pruned step (host rows, device rows
without a K9r plan); ``kmeans_layout.py`` the row layouts and per-tensor caches. The three are plain functions
over the engine; their names are re-exported here.
"""
from __future__ import annotations

import math
import os
import types
from typing import List, Optional

import numpy as np
import torch

from .. import _native
from ..ops import kmeans_ops as K
from ..ops.group_ops import group_reduce
from ..parallel.comm import Communicator, local_comm
from ..utils.device import padded_dim, round_up
from ..utils.fault import maybe_fail
from ..utils.trace import trace
from . import kmeans_init, kmeans_prune_host
from .kmeans_layout import (cached_row_norms, cached_row_sqnorm, dd_sums_exact, host_layout,  # noqa: F401
                            padded_dim_fp8, to_device_matrix, unit_rows)
from .kmeans_route import resolve_route


class LloydEngine:
    """Rank-local shard + distributed Lloyd iterations."""

    def __init__(self, x: torch.Tensor, d: int, k: int, comm: Optional[Communicator] = None,
                 row_ids: Optional[torch.Tensor] = None, row_chunks: Optional[int] = None,
                 accum_mode: Optional[str] = None, use_graph: Optional[bool] = None,
                 incremental: Optional[bool] = None, spherical: bool = False, prune: Optional[bool] = None,
                 precision: Optional[str] = None, weights: Optional[torch.Tensor] = None,
                 refresh_interval: Optional[int] = None, device: Optional[torch.device] = None,
                 stream_chunk_rows: Optional[int] = None):
        self.comm = comm or local_comm()
        # out-of-core rows (utils/hoststream.py): host rows with a GPU `device` stay in pinned host memory
        # and every pass over X streams them through two device buffers (full steps; the per-row state —
        # norms, labels, k-means|| costs — lives on the device)
        self._hs = None
        streamed = device is not None and torch.device(device).type == "cuda" and not x.is_cuda
        screen_ok = (x.is_cuda and x.dtype in (torch.float32, torch.float64) and not streamed and weights is None
                     and not spherical and self.screen_applies(d, k))
        # every decision taken before the rows are prepared (kmeans_route.py; dd_sums_exact is a collective)
        rt = resolve_route(on_device=x.is_cuda, dtype=x.dtype, streamed=streamed, weighted=weights is not None,
                           spherical=bool(spherical), precision=precision, prune=prune, incremental=incremental,
                           use_graph=use_graph, row_chunks=row_chunks, accum_mode=accum_mode,
                           refresh_interval=refresh_interval, screen_ok=screen_ok,
                           dd_exact=lambda: dd_sums_exact(x, d, self.comm), env=os.environ)
        self.precision, self.prune, self.gpu = rt.precision, rt.prune, rt.gpu
        self._wfast, self._screen = rt.wfast, rt.screen
        self._accum_mode, self._incremental = rt.accum_mode, rt.incremental
        self.use_graph, self.refresh_interval, row_chunks = rt.use_graph, rt.refresh_interval, rt.row_chunks
        if streamed:
            # the pinned bf16/fp8 padded copy, made once per column and reused by every later fit and
            # transform of it (with its cached norms and its stream buffers)
            x = host_layout(x, d)
        if rt.to_f32:
            x = x.to(torch.float32)
        # spherical = Spark's distanceMeasure="cosine": rows are scaled to unit length once, centres
        # are renormalised after every update (CosineDistanceMeasure.centroid), and on unit vectors
        # ||x - c||² = 2·(1 - cos), so the euclidean K9/K10 path computes the cosine assignment;
        # costs and the convergence test are converted back (cost / 2, shift² <= 2·tol).
        self.spherical = bool(spherical)
        if self.spherical:
            x = unit_rows(x, d, exact=(rt.precision == "exact"))
        self.track_prune = False  # record (full?, re-assigned rows) of every pruned step (host reads)
        self._pdev = False  # the device pruned step (_step_prune_dev) is in use, decided in _alloc_gpu
        self._graph = None
        self.k = int(k)
        self.d = int(d)
        self.n = int(x.shape[0])
        self.device = torch.device(device) if streamed else x.device
        self._scr = None  # screen state (precision "screen"), see _screen_state
        if streamed:
            from ..utils.hoststream import HostRowStream, cached_stream
            self.x = x
            self.dp = self.x.shape[1]
            if stream_chunk_rows is None:  # ~1 GiB per buffer
                stream_chunk_rows = max(1024, (1 << 30) // (self.dp * self.x.element_size()))
            bounds = HostRowStream.chunk_bounds(self.n, stream_chunk_rows)
            row_chunks = len(bounds) - 1
            self._hs = cached_stream(self.x, bounds[1] - bounds[0] if self.n else 1, self.device)
            self._hs_bounds = bounds  # (re-deriving them from the first chunk's size splits a lone short chunk)
        elif self.gpu:
            self.x = to_device_matrix(x, d)
            self.dp = self.x.shape[1]
        elif self._screen:
            # source rows kept as given (f32 / f64): the exact kernels read them, the screen its bf16 copy
            # (the tensor itself when it is already [n, d]: the screen's bf16 copy and norms are cached on
            # it, and a fresh view would drop them between the fit and the model's transforms)
            self.x = x if (x.shape[1] == d and x.is_contiguous()) else (
                x[:, :d] if x[:, :d].is_contiguous() else x[:, :d].contiguous())
            self.dp = d
        else:
            self.x = x[:, :d].to(torch.float64)
            self.dp = d
        self._row_ids = row_ids
        self.w = self._wx = None
        if weights is not None:
            w = torch.as_tensor(weights, dtype=torch.float64, device=self.device).reshape(-1)
            if w.shape[0] != self.n:
                raise ValueError(f"{w.shape[0]} weights for {self.n} rows")
            self.w = w.contiguous()
            if self._wfast:  # K10w reads the rows as they are: no f64 copy of X, no [w·x | w]
                fp8 = K.is_fp8(self.x)
                # (K10w itself takes e4m3 rows up to 1024 columns; the assign kernels stop at 512)
                if (fp8 and not 256 <= self.dp <= 512) or (not fp8 and self.dp > 512):
                    raise ValueError(
                        f"weighted KMeans with precision 'bf16' assigns on the MFMA kernels and sums in the sort "
                        f"regime: padded width {self.dp} is outside their limit (bf16 rows Dp <= 512, e4m3 rows "
                        f"256 <= Dp <= 512); use precision 'auto' for the source-precision path")
            else:
                self._wx = torch.cat([self.x * w[:, None], w[:, None]], 1)  # [w·x | w]: one sums pass
        # error allowance of the assign's squared distances (pruning bounds), scaled with the padded
        # width: the f32 accumulation error grows with D; f64 rows keep the fixed floor
        # fp8 rows: the K9r passes run MX-scaled fp8 MFMAs against an exact e4m3 split of the centres, which
        # stay on the MX grid (kmeans_mx.hip mx_snap after every update); the allowance is doubled for the MX
        # instruction's own sums (measured within 2^-17 of Σ|terms| per 128 products)
        self._mx = self.gpu and K.mx_applies(self.x)
        self._tau = self.prune_tau(self.dp) if self.gpu else self._PRUNE_TAU
        if self._mx:
            self._tau *= 2.0
        if row_chunks is None:
            row_chunks = 2 if (self.comm.is_distributed and self.n >= (1 << 20)) else 1
        self.row_chunks = max(1, min(int(row_chunks), max(1, self.n)))
        if self._hs is not None:
            self.row_chunks = len(bounds) - 1
        self.centers = torch.zeros((self.k, self.d), dtype=torch.float64, device=self.device)
        self.iterations = 0
        self._cost_fn = None
        self.last_cost = None
        self._shift2 = None
        self._conv_lim = None  # squared-move limit of a tol > 0 fit's device convergence latch (_fit_lagged)
        self.delta = None  # incremental-sums state (GPU sort regime), see _alloc_gpu
        self._pst = None  # pruned-step state: _pdev_alloc, or kmeans_prune_host._prune_init
        # sum grid of the device sort-regime accumulates (_sum_grid): qscale 0 / unit 1 = plain f64 sums
        self._qscale, self._unit, self._grid_done = 0.0, 1.0, False
        self.sum_grid = None  # the grid step when the rows are summed on a grid
        # lazily filled state, declared here so every later read is a plain attribute read
        self.labels = None  # per-row labels: _alloc_gpu, or the first host / exact step
        self._gn = None  # global row count (global_n)
        self._gxmax = None  # max ||x||² over every rank (_xmax_dev)
        self._seed = None  # labels / costs of this engine's k-means|| init (seeds the first step's bounds)
        self._seeded = False  # the next step is _step_seeded
        self._consumed = False  # the fit's final assignment took over the step state
        self._er_event = None  # exponent range prefetched behind the row pass (_prefetch_erange)
        self._graph_warm = False
        self._scr_scratch = None
        self._shift_pair = None
        self._iscr = None  # scratch of the k-means|| candidate passes (kmeans_init._init_scratch)
        self._xn64 = None  # ||x||² of host rows in f64 (kmeans_prune_host._prune_init)
        self.k_effective = self.k  # distinct centres the k-means|| init found (kmeans_init._init_finish)
        self._wst = None  # buffers of the weighted MFMA step (_step_weighted)
        self._init_prune_history = []  # (rows, per-row path, K9r pass) of the pruned k-means|| rounds (track_prune)
        if self.gpu:
            self._alloc_gpu()

    # ------------------------------------------------------------------ setup
    def _alloc_gpu(self):
        dev = self.device
        k, d, dp, n = self.k, self.d, self.dp, self.n
        self.kp = round_up(k, 32)
        if self._hs is not None:
            bounds = self._hs_bounds
        else:
            bounds = [round(i * n / self.row_chunks) for i in range(self.row_chunks + 1)]
            # keep chunk boundaries on 32-row tiles
            bounds = [min(n, round_up(b, 32)) if 0 < i < self.row_chunks else b for i, b in enumerate(bounds)]
        self.bounds = bounds
        maxn = max(bounds[i + 1] - bounds[i] for i in range(self.row_chunks)) if n else 0
        fp8 = K.is_fp8(self.x)
        self.aplan = K.plan_assign(max(maxn, 1), dp, k, dev.index or 0, fp8=fp8)
        self.cplan = K.plan_accum(max(maxn, 1), dp, k, dev.index or 0, force=self._accum_mode, fp8=fp8)
        # the second stage of the route (kmeans_route.py), which depends on the plans:
        # - the device pruned step needs the K9r assign (every centre in one launch) and the sort-regime sums;
        #   pruned steps without them take the torch form (kmeans_prune_host.py: host-synchronised, never
        #   captured, its own sums and a per-row distance scratch)
        # - incremental sums need the sort regime with the centres in one LDS chunk (labels are final after one
        #   launch); the device pruned step allocates its own, larger change lists in _pdev_alloc
        # - distance scratch otherwise only when the centres need several LDS chunks (running min through HBM)
        one_launch = self.aplan.kc == self.aplan.kp
        self._pdev = self.prune and self.aplan.rr_ct > 0 and one_launch and self.cplan.mode == "sort"
        torch_prune = self.prune and not self._pdev
        if torch_prune:
            self.use_graph = False
        want_delta = self._incremental and self.cplan.mode == "sort" and one_launch and not self.prune
        want_best = not one_launch or torch_prune
        self.labels = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        self.best = torch.zeros(max(n, 1), dtype=torch.float32, device=dev) if want_best else None
        # ||x||² are constant over the fit, like Spark's cached point norms: reused from the feature
        # tensor's cache, else computed lazily (_ensure_norms) — k-means|| init fuses them into its
        # first pass over X
        # (_erange: bf16 exponent range of X — exactness of the f64 sums; _xnorm64: ||x||² summed in f64 — the
        # training cost; both from the row pass)
        ent = cached_row_norms(self.x, n, dp)
        if ent is not None:
            (self._xnorm, self._erange, self._xnorm64), self._norms_ready = ent, True
        else:
            self._xnorm, self._norms_ready = torch.empty(max(n, 1), dtype=torch.float32, device=dev), False
            self._erange = None
            self._xnorm64 = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        self.cost_part = torch.zeros(self.aplan.grid, dtype=torch.float64, device=dev)
        if self.cplan.mode == "priv":
            self.slab = torch.empty(self.cplan.nsl * self.cplan.gx * k * self.cplan.dw, dtype=torch.float32,
                                    device=dev)
            self.cslab = torch.empty(self.cplan.gx * k, dtype=torch.int32, device=dev)
        else:
            self.hist = torch.zeros(self.aplan.grid * self.aplan.kp, dtype=torch.int32, device=dev)
            self.rank = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            self.off = torch.zeros(max(k * self.aplan.grid, 1), dtype=torch.int32, device=dev)
            self.seg = torch.zeros(K.seg_buffer_ints(k), dtype=torch.int32, device=dev)
            self.perm = torch.zeros(max(maxn, 1), dtype=torch.int32, device=dev)
            self.slots = K.seg_slots(self.cplan, d, dev)
        self.msg_len = k * d + k + 1
        self.delta = (K.DeltaState(max(maxn, 1), k, d, dp, self.row_chunks, self.msg_len, dev, self.aplan.grid,
                                   fp8=fp8) if want_delta else None)
        self.msgs = torch.zeros((self.row_chunks, self.msg_len), dtype=torch.float64, device=dev)
        self.cb = torch.zeros((self.kp, dp), dtype=torch.bfloat16, device=dev)
        self._cb_cost = torch.zeros_like(self.cb)  # centres of the last full/torch-pruned step's assignment
        self.cnorm = torch.zeros(self.kp, dtype=torch.float32, device=dev)
        self.shift2 = torch.zeros(k, dtype=torch.float64, device=dev)
        self._prev_centers = torch.zeros((k, d), dtype=torch.float64, device=dev) if self.spherical else None
        if self._pdev:
            self._pdev_alloc()

    def _set_mx(self) -> None:
        """Device max ||x||² over every rank (pruning slack), from the cached norms."""
        st = self._pst
        if self.n:
            st.mx.copy_(self._xnorm[: self.n].max().reshape(1))
        else:
            st.mx.zero_()
        if self.comm.is_distributed:
            self.comm.allreduce_(st.mx, op="max")

    def _row_pass(self, c0: Optional[torch.Tensor] = None, c0n: float = 0.0, cost=None, near=None,
                  c0n_dev: Optional[torch.Tensor] = None) -> None:
        """The one pass over X that fills the norms (and max norm, exponent range; with c0 the first
        k-means|| costs), then caches the norms on the feature tensor."""
        n, dp = self.n, self.dp
        self._erange = self._const([2 ** 31 - 1, -1], torch.int32)
        mxv = self._pst.mx if self._pdev else None
        if mxv is not None:
            mxv.zero_()
        if n:
            for _, r0, r1, xc in self._x_chunks(whole=True):
                K.row_pass(xc, r1 - r0, dp, self._xnorm[r0:r1], c0, c0n, None if cost is None else cost[r0:r1],
                           None if near is None else near[r0:r1], xn_max=mxv, erange=self._erange,
                           xn64=self._xnorm64[r0:r1], c0n_dev=c0n_dev)
        if mxv is not None and self.comm.is_distributed:
            self.comm.allreduce_(mxv, op="max")
        self._prefetch_erange()
        self._norms_ready = True
        try:
            self.x._cml_xnorm = (self.x._version, (n, dp), self._xnorm, self._erange, self._xnorm64)
        except (AttributeError, RuntimeError):
            pass

    def _prefetch_erange(self) -> None:
        """Enqueue the rank-agreed exponent range of X (_sum_grid) right behind the row pass and copy it to
        pinned memory: the first Lloyd step then reads it without waiting for the whole init (a blocking read
        there drained the queue between the init and step 1)."""
        if not self.gpu or self._erange is None or K.is_fp8(self.x) or self.cplan.mode != "sort":
            return
        er = self._erange.to(torch.int64)
        if self.comm.is_distributed:
            self.comm.allreduce_(er[0:1], op="min")
            self.comm.allreduce_(er[1:2], op="max")
        self._er_host = torch.empty(2, dtype=torch.int64, pin_memory=True)
        self._er_host.copy_(er, non_blocking=True)
        self._er_event = torch.cuda.Event()
        self._er_event.record()

    def _x_chunks(self, whole: bool = False):
        """(chunk, r0, r1, device rows) over the row chunks: slices of the resident matrix (one slice of
        every row with ``whole``), or the host rows streamed through the double buffer."""
        if self._hs is not None:
            yield from self._hs.chunks(self.bounds)
        elif whole:
            yield 0, 0, self.n, self.x
        else:
            for c in range(self.row_chunks):
                yield c, self.bounds[c], self.bounds[c + 1], self.x[self.bounds[c]:self.bounds[c + 1]]

    def _ensure_norms(self) -> None:
        if self.gpu and not self._norms_ready:
            self._row_pass()

    @property
    def xnorm(self) -> torch.Tensor:
        """||x||² of the device rows (f32), computed on first use unless the k-means|| init's first
        pass over X already produced them."""
        self._ensure_norms()
        return self._xnorm

    @property
    def global_n(self) -> int:
        if self._gn is None:
            self._gn = int(self.comm.sum_scalar(float(self.n)))
        return self._gn

    def row_ids(self) -> torch.Tensor:
        if self._row_ids is None:
            counts = self.comm.allgather_object(self.n)
            off = sum(counts[: self.comm.rank])
            self._row_ids = torch.arange(off, off + self.n, dtype=torch.int64, device=self.device)
        return self._row_ids

    def set_centers(self, centers) -> None:
        """New centres (numpy / list, or a device tensor: no host copy) — the k-means|| result of this
        engine seeds the first step's bounds (_seed_from_init)."""
        self._ensure_norms()
        if torch.is_tensor(centers):
            c = centers.to(device=self.device, dtype=torch.float64)
        else:
            c = torch.as_tensor(np.asarray(centers, dtype=np.float64), device=self.device)
        if c.shape != (self.k, self.d):
            raise ValueError(f"centers shape {tuple(c.shape)} != {(self.k, self.d)}")
        if self.centers.shape == c.shape and self.centers.dtype == c.dtype:
            self.centers.copy_(c)  # in place: a captured step graph keeps reading this buffer
        else:
            self.centers = c.contiguous().clone()
        if self.gpu:
            K.update_centers(None, self.k, self.d, self.centers, self.cb, self.dp, self.kp, self.cnorm, None,
                             snap=self._mx)
        if self._scr is not None and getattr(self._scr, "cert", None) is not None:
            self._scr.cert.valid = False  # the certified step restarts from a screened full assignment
        self._shift_pair = None
        seed, self._seed = self._seed, None
        if self._pdev:  # bounds and incremental sums were relative to the old centres: a full step next
            st = self._pst
            K.centre_stats(self.cb, None, self.k, self.d, st.mx, st.tau, st.cn, st.half, st.drift, st.thr, st.dmax,
                           st.mc, st.c2, st.count, st.force)
            st.backoff.zero_()
            self.delta.invalidate()
            # centres straight from this engine's k-means|| init: the first step starts from bounds the
            # init already implies (no full assign pass); anything else takes a full step
            self._seeded = seed is not None and seed.out.shape == tuple(c.shape) and (
                centers is seed.out or (seed.out_np is not None and not torch.is_tensor(centers) and
                                        np.array_equal(seed.out_np, np.asarray(centers, dtype=np.float64))))
            if self._seeded:
                self._seed_from_init(seed)
            else:
                st.force.fill_(1)
        elif self._pst is not None:  # bounds were relative to the old centres
            self._pst.valid = False
            kmeans_prune_host._prune_centre_stats(self)

    # ------------------------------------------------------------------ iteration
    def step(self) -> None:
        """One Lloyd iteration over the global dataset (all ranks participate)."""
        if self._consumed:
            raise RuntimeError("LloydEngine: the fit's final assignment consumed this engine's step state")
        self._ensure_norms()
        self._sum_grid()
        if (self.delta is not None and self.refresh_interval and self.iterations
                and self.iterations % self.refresh_interval == 0):
            self.delta.invalidate()  # device flag: graph replays take the full accumulate too
            if self._pdev:  # a pruned step has no counting-sort ranks of every row: a full step
                self._pst.force.fill_(1)
        if self._pdev:
            if self._seeded:
                self._seeded = False
                self._step_seeded()
            elif self.use_graph:
                self._step_graph()
            else:
                self._step_prune_dev()
            if self.track_prune:
                self._pst.history.append(self._pdev_last())
        elif self.prune:
            kmeans_prune_host._step_prune(self)
        elif self._wfast:
            self._step_weighted()
        elif self.gpu and self.use_graph and not self.comm.is_distributed:
            self._step_graph()
        elif self.gpu:
            self._step_gpu()
        else:
            self._step_cpu()
        self.iterations += 1

    def _sum_grid(self) -> None:
        """Exactness of the device f64 sums (once per fit, a collective). The incremental sums are only
        equal to a full re-accumulation while every f64 sum is exact: a bf16 row value is a multiple of
        2^(emin - 134) below 2^(emax - 126) (biased exponents over the data, from the row pass), so
        n of them sum exactly while log2(n) + (emax - emin) + 8 <= 53. When the data's exponent span
        breaks that (tiny values beside large ones), every value is summed on the grid
        g = 2^(emax - 126 + ceil(log2(n + 1)) - 52) instead — scaled by 1/g and rounded to an integer, so
        the sums are exact integers in any order and K11 scales them back. The rounding (at most g/2
        per value, at the headline scale 2^-20 against values up to 2^5) happens once per value and in
        the same way on every path, so full, incremental, pruned and multi-rank sums stay equal bit for
        bit. fp8 rows (multiples of 2^-9 below 2^9) are always exact."""
        if self._grid_done:
            return
        self._grid_done = True
        if not self.gpu or K.is_fp8(self.x) or self.cplan.mode != "sort" or (self.prune and not self._pdev):
            return
        if self._wfast:  # double-double sums of the products need no grid
            return
        if self._er_event is not None:  # prefetched behind the row pass (_prefetch_erange)
            self._er_event.synchronize()
            lo, hi = int(self._er_host[0]), int(self._er_host[1])
            self._er_event = None
        else:
            lo_t = self._erange[0:1].to(torch.int64).clone()
            hi_t = self._erange[1:2].to(torch.int64).clone()
            if self.comm.is_distributed:
                self.comm.allreduce_(lo_t, op="min")
                self.comm.allreduce_(hi_t, op="max")
            lo, hi = int(lo_t.item()), int(hi_t.item())
        gn = self.global_n
        if hi < 0 or gn == 0:  # every value is zero
            return
        lg = math.ceil(math.log2(gn + 1))
        if lg + (hi - max(lo, 1)) + 8 <= 53:
            return  # plain f64 sums are exact
        g = (hi - 126) + lg - 52
        self._qscale, self._unit, self.sum_grid = 2.0 ** -g, 2.0 ** g, 2.0 ** g

    def _step_graph(self):
        """Replay the captured step (captured on the first call after one eager warm-up step,
        which also settles every lazily allocated buffer). All step state lives in buffers the
        graph reads in place: new centres from set_centers/update are picked up by the replay."""
        split = self._pdev and self.comm.is_distributed  # graph | all-reduce | graph
        if self._graph is None:
            if not self._graph_warm:
                self._graph_warm = True
                (self._step_prune_dev if self._pdev else self._step_gpu)()
                return
            torch.cuda.synchronize(self.device)
            if split:
                ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(ga):
                    self._pdev_pre()
                with torch.cuda.graph(gb):
                    self._pdev_post()
                self._graph = (ga, gb)
            else:
                g = torch.cuda.CUDAGraph()
                body = self._step_prune_dev if self._pdev else self._step_gpu
                with torch.cuda.graph(g):
                    body()
                self._graph = g
        if split:
            self._graph[0].replay()
            self.comm.allreduce_async(self.msgs[0]).wait()
            self._graph[1].replay()
        else:
            self._graph.replay()
        self._cost_fn = self._device_cost if self.cplan.mode != "priv" else self._exact_cost

    def _best(self, r0: int, r1: int):
        return None if self.best is None else self.best[r0:r1]

    def _step_gpu(self):
        handles = []
        for c, r0, r1, xc in self._x_chunks():
            nrow = r1 - r0
            msg = self.msgs[c]
            if nrow > 0:
                lab, dl = self.labels[r0:r1], self.delta
                # (the sort regime's assign also emits the counting sort's histogram and ranks, and with
                # incremental sums logs the label changes)
                sort = self.cplan.mode != "priv"
                rank = self.rank[r0:r1] if sort else None
                K.assign_bf16(xc, nrow, self.dp, self.cb, self.cnorm, self.aplan, lab, self._best(r0, r1),
                              self.cost_part, self.hist if sort else None, rank, xnorm=self.xnorm[r0:r1], delta=dl)
                if not sort:
                    K.accumulate_priv(xc, nrow, lab, self.k, self.cplan, self.slab, self.cslab)
                    K.reduce_slabs(self.slab, self.cslab, self.cost_part, self.aplan.grid, self.k, self.d,
                                   self.cplan, msg)
                elif dl is not None:
                    # label changes logged by the assign; the gate picks the full or the delta accumulate
                    # on the device (no host sync, graph-capturable), both update delta.acc[c] -> msg
                    dl.gate(c)
                    K.accumulate_sort(xc, nrow, self.dp, self.d, lab, rank, self.hist, self.aplan, self.k,
                                      self.cost_part, self.off, self.seg, self.perm, self.cplan, dl.acc[c],
                                      self.slots, gate=dl.mode[c], qscale=self._qscale)
                    dl.accumulate(xc, self.dp, lab, c, self.cost_part, self.aplan.grid, msg, qscale=self._qscale)
                else:
                    K.accumulate_sort(xc, nrow, self.dp, self.d, lab, rank, self.hist, self.aplan, self.k,
                                      self.cost_part, self.off, self.seg, self.perm, self.cplan, msg, self.slots,
                                      qscale=self._qscale)
            else:
                msg.zero_()
            handles.append(self.comm.allreduce_async(msg))
        for h in handles:
            h.wait()
        # the cost of this assignment is evaluated on first read against a copy of the centres it was made
        # with: from the exact f64 sums (_device_cost), or — the private-LDS regime sums in f32 — by the
        # exact cost pass (resident rows) / the assign's per-row distances (streamed rows)
        self._cb_cost.copy_(self.cb)
        if self.cplan.mode != "priv":
            self._cost_fn = self._device_cost
        elif self._hs is None:
            self._cost_fn = self._exact_cost
        else:
            self.last_cost = self.msgs[:, -1].sum()
        self._update_gpu(self.msgs)

    def _update_gpu(self, msgs: torch.Tensor) -> None:
        """K11 from the all-reduced [sums | counts | cost] rows (one per chunk)."""
        if self.spherical:
            self._prev_centers.copy_(self.centers)
        K.update_centers(msgs, self.k, self.d, self.centers, self.cb, self.dp, self.kp, self.cnorm,
                         self.shift2, unit=self._unit, snap=self._mx)
        if self.spherical:  # unit-length centres (empty clusters keep their old, already unit, centre)
            self.centers.div_(self.centers.norm(dim=1, keepdim=True).clamp_(min=1e-300))
            torch.sum((self.centers - self._prev_centers) ** 2, dim=1, out=self.shift2)
            K.update_centers(None, self.k, self.d, self.centers, self.cb, self.dp, self.kp, self.cnorm, None,
                             snap=self._mx)
        self._shift2 = self.shift2

    def _step_weighted(self):
        """One weighted Lloyd iteration on the MFMA path (weights with precision "bf16"): the unweighted
        step's assign (K9 / K9r with the counting sort's hist / rank) and sort, then K10w instead of the f64
        segmented sums: per cluster Σ fl64(w·x), Σ w and Σ fl64(w·||x||²) in double-double, read from the
        bf16 / e4m3 rows as they are. Several ranks gather [S | S_lo] and fold them in rank order
        (_exact_global's scheme), so the message — and every centre — is the one-rank bits for any split of
        the rows. K11 runs unchanged on [Σw·x | Σw | 0]: it divides by the count slot, here W_j, and keeps
        the centre of a cluster with W_j = 0. The cost is evaluated on first read from the same sums
        (_weighted_cost), with no pass over X."""
        n, k, d, dev = self.n, self.k, self.d, self.device
        st = self._wst
        if st is None:
            f64 = dict(dtype=torch.float64, device=dev)
            st = self._wst = types.SimpleNamespace(
                S=torch.zeros((k, d + 2), **f64), S_lo=torch.zeros((k, d + 2), **f64),
                tail=torch.zeros(k + 1, **f64), q=torch.zeros(k, **f64),
                slots=K.wseg_slots(self.cplan, d, dev))
        if n:
            K.assign_bf16(self.x, n, self.dp, self.cb, self.cnorm, self.aplan, self.labels, self._best(0, n),
                          self.cost_part, self.hist, self.rank, xnorm=self.xnorm[:n])
            K.sort_perm(self.labels, self.rank, self.hist, self.aplan, n, k, self.off, self.seg, self.perm,
                        tail=st.tail)
            K.weighted_sums(self.x, n, self.dp, d, self.w, self._norms64(), k, self.perm, self.seg, self.cplan,
                            out=(st.S, st.S_lo), slots=st.slots)
        S = st.S
        if self.comm.is_distributed:
            m = S.numel()
            g = self.comm.allgather_fixed(torch.cat([st.S.reshape(-1), st.S_lo.reshape(-1)]))
            S = K.dd_fold(g[:, :m], g[:, m:]).reshape(k, d + 2)
        msg = self.msgs[0]
        msg[:k * d].view(k, d).copy_(S[:, :d])
        msg[k * d:k * d + k].copy_(S[:, d])
        msg[k * d + k:].zero_()
        st.q.copy_(S[:, d + 1])
        self._cb_cost.copy_(self.cb)
        self._cost_fn = self._weighted_cost
        self._update_gpu(self.msgs)

    def _weighted_cost(self) -> torch.Tensor:
        """Σ w_i |x_i - c_label(i)|² of the last weighted step's assignment, from its sums alone:
        Σ_j (Q_j - 2 c_j·S_j + W_j |c_j|²) with Q_j = Σ fl64(w_i ||x_i||²), S_j and W_j the (rank-folded)
        weighted sums and c_j the bf16 centres the assignment compared with. No collective: every rank
        holds the folded sums."""
        return K.cost_combine(self._wst.q, self.msgs, self.k, self.d, 1.0, self._cb_cost)

    # ------------------------------------------------------------------ MFMA-screened exact assignment
    @staticmethod
    def screen_applies(d: int, k: int) -> bool:
        """A K9r plan (every centre in one launch) exists for the bf16 copy of d-wide rows and k centres."""
        dp = padded_dim(d)
        if dp not in (128, 256, 512):
            return False
        p = K.plan_assign(1, dp, k)
        return p.rr_ct > 0 and p.kc == p.kp

    def _screen_state(self):
        """The screen's buffers: the bf16 copy of the rows with each row's rounding error (cached on the
        source tensor while it is unmodified), its f32 norms, bf16 centres, bounds, candidate list."""
        if self._scr is not None:
            return self._scr
        n, d, dev = self.n, self.d, self.device
        # split screen when three segments of the row fit one K9r row (d <= 170): x·c to ~2^-16, so the
        # certificate leaves only real near-ties for the f64 re-check (CML_KMEANS_SCREEN_SPLIT=0: plain)
        ds = round_up(d, 8)
        split = (3 * ds <= 512 and os.environ.get("CML_KMEANS_SCREEN_SPLIT", "1") != "0"
                 and K.plan_assign(1, 512, self.k).rr_ct > 0)
        dp = 512 if split else padded_dim(d)
        key = ("split", ds) if split else ("plain", dp)
        ent = getattr(self.x, "_cml_screen", None)
        if ent is not None and ent[0] == self.x._version and ent[1] == (n, d) and ent[2] == key:
            parts = ent[3]
        else:
            parts = K.to_bf16_split(self.x, d, ds, dp) if split else K.to_bf16_err(self.x, d, dp)
            try:
                self.x._cml_screen = (self.x._version, (n, d), key, parts)
            except (AttributeError, RuntimeError):
                pass
        if split:
            xb, ea, eb, en, xn = parts
            # the K9r slack of 3·ds non-zero products (the zero tail adds no rounding); the lo·hi products
            # are 2^-8 of the hi·hi ones, so their magnitudes sum to at most 1.02x the plain row's
            st = types.SimpleNamespace(xb=xb, ea=ea, eb=eb, en=en, ex=None, dp=dp, ds=ds, split=True,
                                       tau=1.02 * self.prune_tau(3 * ds))
            st.xn = xn
        else:
            xb, ex = parts
            st = types.SimpleNamespace(xb=xb, ex=ex, dp=dp, split=False, tau=self.prune_tau(dp))
            st.xn = cached_row_sqnorm(xb, n, dp) if n else torch.zeros(1, dtype=torch.float32, device=dev)
        st.rr_max = K.rr_max_chunk(dp)
        kp = round_up(max(st.rr_max, self.k), 32)
        st.cb = torch.zeros((kp, dp), dtype=torch.bfloat16, device=dev)
        st.cn = torch.zeros(kp, dtype=torch.float32, device=dev)
        st.ub = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
        st.lb = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
        st.lst = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        st.cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        st.rechecked = []  # uncertified rows per screened pass, read only when track_prune is set
        self._scr = st
        return st

    def _screen_labels(self, C: torch.Tensor, lab: torch.Tensor, best: Optional[torch.Tensor] = None) -> None:
        """Exact f64 argmin labels (lowest index on ties) of every local row against the f64 centres C
        (at most one K9r launch of them), screened on MFMA: K9r mode 1 on the bf16 copy gives each row's
        bf16 label with bounds ub >= its distance and lb <= every other distance (f32 rounding inside);
        the exact distances differ from the bf16 ones by at most ||x - bf16(x)|| + ||c - bf16(c)||, so a row
        with lb - ub > 2·(err_x + max err_c) has that label exactly; the others are re-assigned in f64
        (exact_top2 over the listed rows: exact_assign's fold, same bits). Afterwards st.ub / st.lb hold
        f32 bounds of every row's real distance to its label / to every other centre (the certified
        step's starting bounds). ``best`` (f64 [n], optional) receives the exact squared distance to the
        label (exact_dist: the exact kernel's fold, the same bits)."""
        st = self._screen_state()
        n, d, kc = self.n, self.d, int(C.shape[0])
        if n == 0:
            return
        C = C.to(device=self.device, dtype=torch.float64).contiguous()
        kp = round_up(kc, 32)
        if st.split:  # one launch: the layout, the norms, the certificate's constants and max |c|²
            if getattr(st, "cst", None) is None:
                st.cst = torch.zeros(3, dtype=torch.float64, device=self.device)
                st.mc = torch.zeros(1, dtype=torch.float32, device=self.device)
            K.split_centres_dev(C, st.ds, st.cb[:kp], st.cn[:kp], st.cst, mc=st.mc)
            cst, mc = st.cst, st.mc
        else:
            st.cb[:kp].zero_()
            st.cn[:kp].zero_()
            K.update_centers(None, kc, d, C.clone(), st.cb[:kp], st.dp, kp, st.cn[:kp], None)
            ecmax = ((C - st.cb[:kc, :d].to(torch.float64)) ** 2).sum(1).max().sqrt().reshape(1) * (1.0 + 1e-9)
            mc = st.cn[:kc].max().reshape(1)
        plan = K.plan_assign(n, st.dp, kc)
        K.assign_rr_ext(1, st.xb, n, st.dp, st.cb[:kp], st.cn[:kp], plan, st.xn, lab, None, st.ub, st.lb, mc, st.tau)
        st.cnt.zero_()
        if st.split:
            K.screen_cert_split(st.ub, st.lb, st.ea, st.eb, st.en, cst, n, st.lst, st.cnt, st.ub, st.lb)
        else:
            K.screen_cert(st.ub, st.lb, st.ex, ecmax, n, st.lst, st.cnt, u_out=st.ub, l_out=st.lb)
        if best is not None:
            K.exact_dist(self.x, C, lab, best)
        K.exact_top2(self.x, C, lab, st.ub, st.lb, idx=st.lst, n_dev=st.cnt, best=best)
        if self.track_prune:
            st.rechecked.append(int(st.cnt.item()))

    def screen_assign(self, centers, want_dist: bool = True):
        """(labels int64, exact f64 squared distance or None) of every local row against ``centers`` on the
        MFMA screen — exact_assign's labels and distances bit for bit (``KMeansModel.transform`` /
        ``computeCost`` on f32/f64 device rows; VERDICT r4: they ran the scalar f64 kernel, ~300 ms per
        pass at 10M x 128). Rank-local: no collective."""
        st = self._screen_state()
        n, dev = self.n, self.device
        C = torch.as_tensor(centers).to(device=dev, dtype=torch.float64).contiguous()
        kc = int(C.shape[0])
        if n == 0:
            return (torch.zeros(0, dtype=torch.int64, device=dev),
                    torch.zeros(0, dtype=torch.float64, device=dev) if want_dist else None)
        if kc > st.rr_max:  # several K9r launches merged in candidate order (the first index on ties)
            best, lab = self._screen_min_dist(C)
            return lab, (best if want_dist else None)
        lab = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        best = self._scr_best() if want_dist else None
        self._screen_labels(C, lab, best)
        return lab[:n].long(), (best[:n].clone() if want_dist else None)

    def _scr_best(self) -> torch.Tensor:
        if self._scr_scratch is None:
            self._scr_scratch = torch.empty(max(self.n, 1), dtype=torch.float64, device=self.device)
        return self._scr_scratch

    def _screen_min_dist(self, cands: torch.Tensor):
        """_min_dist_idx of the screen: (exact f64 squared distance to the nearest candidate, its index) of
        every local row, candidates in K9r-sized chunks merged in order with strict < (the first index on
        ties, as one exact assignment over the whole list)."""
        st = self._screen_state()
        n, dev = self.n, self.device
        cands = cands.to(device=dev, dtype=torch.float64)
        if int(cands.shape[0]) == 1:  # one candidate: every label is 0, the distance one exact fold
            lab1 = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
            b1 = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
            if n:
                K.exact_dist(self.x, cands.contiguous(), lab1, b1)
            return b1[:n], lab1[:n].long()
        best = torch.full((max(n, 1),), math.inf, dtype=torch.float64, device=dev)
        lab = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        lab_c = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        best_c = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        step = max(1, st.rr_max)
        for c0 in range(0, int(cands.shape[0]), step):
            C = cands[c0:c0 + step]
            if int(C.shape[0]) <= 8:
                # a short leftover chunk (e.g. 2 of a round's 130 candidates): the exact fold over every
                # row reads X once and yields the distances too — cheaper than a screened pass over the
                # wide split copy plus exact_dist
                K.exact_top2(self.x, C, lab_c, st.ub, st.lb, best=best_c)
            else:
                self._screen_labels(C, lab_c, best_c)
            better = best_c[:n] < best[:n]
            best[:n] = torch.where(better, best_c[:n], best[:n])
            lab[:n] = torch.where(better, lab_c[:n].long() + c0, lab[:n])
        return best[:n], lab[:n]

    def _cert_state(self):
        """Buffers of the certified pruned step (kmeans_cert.hip): labels, row lists, moves, the move
        sort, and the double-double cluster sums of the current labels (S_hi + S_lo, int32 counts)."""
        st = self._screen_state()
        c = getattr(st, "cert", None)
        if c is not None:
            return c
        n, k, d, dev = self.n, self.k, self.d, self.device
        m = max(n, 1)
        i32 = dict(dtype=torch.int32, device=dev)
        c = types.SimpleNamespace(valid=False, history=[])
        c.lab = torch.zeros(m, **i32)
        c.ctr = torch.zeros(4 + 2 * k, **i32)  # [list A, list B, moves, -, move histogram (2k)]
        c.la, c.lbl = torch.empty(m, **i32), torch.empty(m, **i32)
        c.mvr, c.mvo, c.mvn = torch.empty(m, **i32), torch.empty(m, **i32), torch.empty(m, **i32)
        c.seg, c.cursor, c.perm = torch.empty(2 * k + 1, **i32), torch.empty(2 * k, **i32), torch.empty(2 * m, **i32)
        c.s = torch.empty(k, dtype=torch.float32, device=dev)
        c.drift = torch.empty(k, dtype=torch.float32, device=dev)
        c.dtop = torch.zeros(4, dtype=torch.float32, device=dev)
        ns = K.cert_slices(k)
        c.P_hi = torch.empty(ns * k * d, dtype=torch.float64, device=dev)
        c.P_lo = torch.empty(ns * k * d, dtype=torch.float64, device=dev)
        c.S_hi = c.S_lo = c.cnt = c.C_cur = None
        if st.split and n:
            # list B goes through the split-screen K9r candidate pass first: whole K9r tiles of valid rows
            c.plan = K.plan_assign(n, st.dp, k)
            pad = n + c.plan.round_rows
            c.lbl = torch.zeros(pad, **i32)
            c.bxn = torch.zeros(pad, dtype=torch.float32, device=dev)
            c.blab = torch.zeros(pad, **i32)
            c.lc = torch.empty(m, **i32)
            c.cst = torch.zeros(3, dtype=torch.float64, device=dev)
            c.mc = torch.zeros(1, dtype=torch.float32, device=dev)
            c.kp = round_up(k, 32)
        # one-rank centre updates land in two alternating buffers (the update kernel writes the next
        # centres beside the current ones; no per-step host work)
        c.cbuf = [torch.empty((k, d), dtype=torch.float64, device=dev) for _ in range(2)]
        st.cert = c
        return c

    def _exact_global(self, S: torch.Tensor, S_lo: torch.Tensor, counts: Optional[torch.Tensor],
                      cost: torch.Tensor):
        """(sums, counts, cost) over every rank: each rank's double-double sums folded in rank order — the
        one-rank bits for any partitioning of the rows (an f64 all-reduce would round per rank)."""
        if not self.comm.is_distributed:
            return S, counts, cost
        m, k = S.numel(), self.k
        parts = [S.reshape(-1), S_lo.reshape(-1)]
        if counts is not None:
            parts.append(counts.to(torch.float64))
        parts.append(cost.reshape(1).to(torch.float64))
        g = self.comm.allgather_fixed(torch.cat(parts))
        S = K.dd_fold(g[:, :m], g[:, m:2 * m]).reshape(S.shape)
        counts = g[:, 2 * m:2 * m + k].sum(0) if counts is not None else None
        return S, counts, g[:, -1].sum()

    def _step_screen(self):
        """One exact Lloyd iteration on the source rows (the exact path's labels, sums and centres bit for
        bit). The first assigns every row through the MFMA screen (_screen_labels) and sums from scratch
        (double-double, exact_sums); later ones are certified pruned steps (kmeans_cert.hip): Hamerly
        bounds on the real distances, moved by the centre drifts, prove most labels unchanged; the rest
        are tightened, re-assigned by the exact fold when still unproven, and the label moves update the
        double-double sums incrementally (exactly the from-scratch sums). The cost of the assignment is
        evaluated on first read (exact_dist)."""
        n, k, d = self.n, self.k, self.d
        c = self._cert_state()
        st = self._scr
        f64 = dict(dtype=torch.float64, device=self.device)
        if not c.valid:
            if n:
                self._screen_labels(self.centers, c.lab)
                c.S_hi, c.cnt, c.S_lo = K.exact_sums(self.x, c.lab[:n], k, with_lo=True, counts_int=True)
            else:
                c.S_hi, c.S_lo = torch.zeros((k, d), **f64), torch.zeros((k, d), **f64)
                c.cnt = torch.zeros(k, dtype=torch.int32, device=self.device)
            c.valid = True
        elif n:
            K.cert_stats(self.centers, c.C_cur, c.s, c.drift, c.dtop, zero=c.ctr)
            K.cert_bounds(c.lab, st.ub, st.lb, c.drift, c.dtop, c.s, n, c.la, c.ctr[0:1])
            moves = (c.mvr, c.mvo, c.mvn, c.ctr[2:3])
            if st.split:
                # list B: the split-screen K9r candidate pass, its certificate, the exact fold for the rest
                K.cert_tighten(self.x, self.centers, c.lab, st.ub, st.lb, c.s, c.la, c.ctr[0:1], c.lbl, c.ctr[1:2],
                               xn=st.xn, bxn=c.bxn, blab=c.blab)
                K.split_centres_dev(self.centers, st.ds, st.cb[:c.kp], st.cn[:c.kp], c.cst, mc=c.mc)
                K.assign_rr_ext(2, st.xb, n, st.dp, st.cb[:c.kp], st.cn[:c.kp], c.plan, c.bxn, c.lab, None, st.ub,
                                st.lb, c.mc, st.tau, idx=c.lbl, n_dev=c.ctr[1:2], lab_in=c.blab)
                K.cert_list(c.lbl, c.ctr[1:2], n, c.blab, c.lab, st.ub, st.lb, st.ea, st.eb, st.en, c.cst, c.lc,
                            c.ctr[3:4], moves)
                K.exact_top2(self.x, self.centers, c.lab, st.ub, st.lb, idx=c.lc, n_dev=c.ctr[3:4], moves=moves)
            else:
                K.cert_tighten(self.x, self.centers, c.lab, st.ub, st.lb, c.s, c.la, c.ctr[0:1], c.lbl, c.ctr[1:2])
                K.exact_top2(self.x, self.centers, c.lab, st.ub, st.lb, idx=c.lbl, n_dev=c.ctr[1:2], moves=moves)
            fast = not self.comm.is_distributed  # one rank: the update kernel writes the next centres
            nxt = None
            if fast:
                nxt = c.cbuf[1] if self.centers.data_ptr() == c.cbuf[0].data_ptr() else c.cbuf[0]
            K.cert_moves(self.x, k, c.mvr, c.mvo, c.mvn, c.ctr[2:3], c.ctr[4:], c.seg, c.cursor, c.perm, c.P_hi,
                         c.P_lo, c.S_hi, c.S_lo, c.cnt, C_cur=self.centers if fast else None, C_next=nxt)
            if self.track_prune:  # (list A, list B, moves, list C: exact re-assignments after the screen)
                c.history.append(tuple(int(v) for v in c.ctr[:4].tolist()))
            if fast:
                # the exact path's update bits (S / count in IEEE f64, empty clusters keep their centre);
                # the shift and the cost are evaluated on demand against these two buffers, which the
                # next step's update (the other buffer) leaves intact
                c.C_cur, c_used, lab_used = self.centers, self.centers, c.lab[:n]
                self._shift2, self._shift_pair = None, (nxt, self.centers)
                self.centers = nxt
                self.labels = c.lab[:n]
                self._cost_fn = lambda: self._screen_cost(c_used, lab_used)
                return
        c.C_cur = self.centers.clone()  # the centres of this assignment (set_centers writes in place)
        S, counts, _ = self._exact_global(c.S_hi, c.S_lo, c.cnt.to(torch.float64), torch.zeros(1, **f64))
        msg = torch.cat([S.reshape(-1), counts, torch.zeros(1, **f64)])
        c_used, lab_used = c.C_cur, c.lab[:n].clone()
        self._shift_pair = None
        self._update_cpu(msg)
        self.labels = c.lab[:n]
        self._cost_fn = lambda: self._screen_cost(c_used, lab_used)

    def _screen_cost(self, C: torch.Tensor, lab: torch.Tensor) -> torch.Tensor:
        """Cost of an exact assignment: Σ of every row's f64 fold against its label's centre, over ranks."""
        n = self.n
        b = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        if n:
            K.exact_dist(self.x, C, lab, b)
        tot = K.sum_exact(b[:n]).reshape(1) if n else torch.zeros(1, dtype=torch.float64, device=self.device)
        self.comm.allreduce_(tot)
        return tot[0]

    def _step_cpu(self):
        if self._screen:
            return self._step_screen()
        labels, best = K.assign_reference(self.x, self.centers)
        # the cost: a correctly rounded sum too (host and device sessions report the same bits)
        if self.w is not None:  # weighted rows: [w·x | w] summed in double-double, the weight column too
            aug, _, aug_lo = K.sums_reference(self._wx, labels, self.k, with_lo=True)
            aug, _, cost = self._exact_global(aug, aug_lo, None, K.sum_exact(best * self.w))
            sums, counts = aug[:, : self.d], aug[:, self.d]
        else:
            sums, counts, sums_lo = K.sums_reference(self.x, labels, self.k, with_lo=True)
            sums, counts, cost = self._exact_global(sums, sums_lo, counts, K.sum_exact(best))
        msg = torch.cat([sums.reshape(-1), counts, cost.reshape(1)])
        self._update_cpu(msg)
        self.labels = labels

    def _update_cpu(self, msg: torch.Tensor) -> None:
        kd = self.k * self.d
        sums = msg[:kd].reshape(self.k, self.d)
        counts = msg[kd:kd + self.k]
        new = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], self.centers)
        if self.spherical:
            new = torch.where(counts[:, None] > 0, new / new.norm(dim=1, keepdim=True).clamp(min=1e-300), new)
        self._shift2 = ((new - self.centers) ** 2).sum(1)
        self.centers = new
        self.last_cost = msg[-1]

    # ------------------------------------------------------------------ device pruned step
    @staticmethod
    def prune_tau(dp: int) -> float:
        """Error allowance of the assign's squared distances, relative to |x|² + max|c|²: the f32
        accumulation of dp exact bf16 products (dp·2^-25 of Σ|x_j c_j| <= (|x|² + |c|²)/2 each way)
        plus the key truncation of the K9r argmin (2^-18 of a distance <= 2(|x|² + |c|²)), doubled."""
        return max(3e-5, 2.0 * (dp * 2.0 ** -25 + 2.0 ** -17))

    def _pdev_alloc(self) -> None:
        """State of the device pruned step (_step_prune_dev): per-row bounds, candidate lists sized for
        _PRUNE_CAP of the rows, centre statistics, and incremental sums whose change lists can hold
        every candidate of a workgroup (a candidate pass never overflows into a full re-accumulation)."""
        n, k, d, dev, ap = self.n, self.k, self.d, self.device, self.aplan
        tr = ap.round_rows
        st = types.SimpleNamespace(history=[])
        cap = float(os.environ.get("CML_KMEANS_PRUNE_CAP", self._PRUNE_CAP))  # A/B knob (bench --prune-cap)
        st.cap_m = max(tr, int(math.ceil(cap * n)))
        st.tau = self._tau
        per_wg = -(-(-(-st.cap_m // tr)) // ap.grid) * tr
        pad = round_up(st.cap_m, tr) + tr
        # the candidate lists and the small per-step state: views of one zeroed block (one fill instead of
        # sixteen). pmode = [full pass?, re-assigned rows]; mx = max ||x||² over all ranks (_ensure_norms)
        lazy = k <= 4096
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        (st.cand, st.cand_lab, st.cand_xn, st.count, st.pmode, st.backoff, st.drift, st.thr, st.dmax, st.cn, st.half,
         st.mc, st.c2, st.mx, cum, st.ctr) = K.zeros_block(dev, [
             (pad, i32), (pad, i32), (pad, f32), (1, i32), (2, i32), (1, i32), (k, f32), (k, f32), (3, f32),
             (k, f64), (k, f64), (1, f32), (1, f32), (1, f32), (2 * k if lazy else 0, f32), (2, i32)])
        # step flags [force, done]: force = bounds invalid (a full pass next); done = converged (tol > 0
        # fits, _fit_lagged): every later step is a frozen no-op until the host reads the flag
        st.flags = self._const([1, 0], torch.int32)
        st.force, st.done = st.flags[0:1], st.flags[1:2]
        # steps left that skip the bounds after one went over the cap (data the bounds do not prune);
        # CML_KMEANS_PRUNE_BACKOFF=0 retries the bounds every step
        st.nback = int(os.environ.get("CML_KMEANS_PRUNE_BACKOFF", "2"))
        st.ub = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
        st.lb = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
        st.cb_old = torch.zeros_like(self.cb)
        st.cb_cost = torch.zeros_like(self.cb)  # centres of the last live step's assignment (training cost)
        # offset-form bounds (kmeans_prune.hip bound_lazy): ub/lb hold ub - cu[label] / lb + cl[label]
        # against these cumulative drifts [cu | cl], so the bounds pass only reads the rows whose label
        # holds; k > 4096 keeps the absolute bounds rewritten every step
        st.cum = cum if lazy else None
        # completion counters of the fused launches (gate in the bounds pass, stats in the half pass); each
        # launch leaves its counter at zero (st.ctr)
        st.half_every = int(os.environ.get("CML_KMEANS_HALF_EVERY", "4"))
        # recorded launch sequences of the step variants (_pdev_pre / _pdev_post); None: always the wrappers
        st.replay = {} if os.environ.get("CML_KMEANS_REPLAY", "1") != "0" else None
        st.replay_refused = None  # why a recording was not replayable (_replay), for tests and diagnostics
        # the gate's full-pass flag, stored by the device into pinned host memory and read by the host with no
        # synchronisation (a few steps stale): steps enqueue the full-accumulate launches while the device keeps
        # picking full passes (data the bounds do not prune: many label changes), lean steps otherwise
        st.pm_host = torch.zeros(1, dtype=torch.int32, pin_memory=True) if self.gpu else None
        self._pst = st
        if self._norms_ready:  # norms cached on the feature tensor by an earlier engine
            self._set_mx()
        # lean steps (CML_KMEANS_LEAN_STEP, eager steps only: a captured graph must hold the full path for forced
        # replays): change lists sized for every row of a workgroup, so an unforced step enqueues only the delta
        # launches — the full re-accumulation's six gated launches ran (as no-ops) in every steady step before
        lean = os.environ.get("CML_KMEANS_LEAN_STEP", "1") != "0" and not self.use_graph
        per_wg_all = -(-(-(-max(n, 1) // tr)) // ap.grid) * tr
        self.delta = K.DeltaState(max(n, 1), k, d, self.dp, 1, self.msg_len, dev, ap.grid, fp8=K.is_fp8(self.x),
                                  cap=max(st.cap_m, 1024), pcap=max(per_wg_all if lean else per_wg, 64), lean=lean)

    def _step_prune_dev(self) -> None:
        """One exact Lloyd iteration with no host synchronisation (HIP-graph capturable):
        K9p moves every row's bounds by the centre drifts and compacts the rows they no longer prove
        (label, norm beside each); a one-thread gate picks the full pass (bounds invalid, or more than
        _PRUNE_CAP of the rows are candidates) or the candidate pass; both K9r launches are enqueued
        and the device runs one — mode 1 over every row, mode 2 over the candidate positions, each
        writing new labels and top-2 bounds and logging label changes; the incremental sums move by
        the changed rows (exact f64 sums, as the full path); all-reduce; K11; centre statistics for
        the next step's bounds."""
        self._pdev_pre()
        self.comm.allreduce_async(self.msgs[0]).wait()
        self._pdev_post()

    def _pdev_pre(self) -> None:
        """The device pruned step up to its all-reduce (bounds, gate, K9r passes, sums -> msg)."""
        st, dl = self._pst, self.delta
        hint_full = int(st.pm_host[0]) != 0
        lean = dl.lean_step() and not hint_full
        if self._replay_ok():
            # the launch sequence of this variant, recorded once (fixed buffers and scalars): replayed without
            # the Python wrappers — the shard's steps were bound by ~25 us of host time per launch
            if self._replay(("pre", lean), lambda: self._pdev_pre_launches(lean)):
                dl.host_forced = False  # what the recorded gate does on the host
                return
        self._pdev_pre_launches(lean)

    def _replay(self, key, launches) -> bool:
        """Replay the recorded launch sequence ``key`` of the current stream, recording it first (or again,
        after a buffer it reads was re-allocated: _native.ReplayGuard). False — nothing ran, the caller runs
        the wrappers — when the sequence cannot be recorded safely (temporaries or torch ops inside)."""
        st = self._pst
        stream = _native.stream_ptr(None)
        k = (key, stream)  # the recording froze the stream: one per stream
        ent = st.replay.get(k)
        if ent is not None and ent[1].valid():
            ent[0]()
            return True
        if ent is not None and not ent[1].ok:
            return False
        with _native.recording() as rec:
            launches()
        guard = _native.ReplayGuard(rec, (self, st, self.delta, self.aplan, self.cplan), stream)
        st.replay[k] = (_native.Recorded(rec.calls), guard)
        if not guard.ok:
            st.replay_refused = guard.why
            return False
        st.replay[k][0]()
        return True

    def _pdev_pre_launches(self, lean: bool) -> None:
        st, dl = self._pst, self.delta
        n, k, d, ap = self.n, self.k, self.d, self.aplan
        x, lab, msg = self.x, self.labels, self.msgs[0]
        # bounds pass + gate in one launch
        K.prune_bounds_gated(lab[:n], st.ub, st.lb, st.drift, st.dmax, st.thr, st.c2, k, st.cand, st.count,
                             self.xnorm, st.cand_lab, st.cand_xn, st.flags, st.cum, st.pmode, st.cap_m,
                             st.backoff if st.nback > 0 else None, st.nback, st.ctr[0:1], mode_host=st.pm_host)
        K.assign_rr_ext(1, x, n, self.dp, self.cb, self.cnorm, ap, self.xnorm, lab, self.cost_part, st.ub, st.lb,
                        st.mc, st.tau, hist=self.hist, rank=self.rank, delta=dl, gate=st.pmode, want=1, cum=st.cum)
        K.assign_rr_ext(2, x, st.cap_m, self.dp, self.cb, self.cnorm, ap, st.cand_xn, lab, self.cost_part, st.ub,
                        st.lb, st.mc, st.tau, delta=dl, idx=st.cand, n_dev=st.count, lab_in=st.cand_lab,
                        gate=st.pmode, want=0, cum=st.cum)
        dl.gate(0, lean=lean)
        if not lean:  # a forced step: the full re-accumulation may run (lean steps never pick it)
            K.accumulate_sort(x, n, self.dp, d, lab, self.rank, self.hist, ap, k, self.cost_part, self.off, self.seg,
                              self.perm, self.cplan, dl.acc[0], self.slots, gate=dl.mode[0], qscale=self._qscale)
        dl.accumulate(x, self.dp, lab, 0, self.cost_part, ap.grid, msg, qscale=self._qscale)

    def _replay_ok(self) -> bool:
        """Recorded launch sequences for the device pruned step: eager steps (a captured graph already
        replays its launches), the sum regime settled (the first step's _sum_grid); CML_KMEANS_REPLAY=0: off."""
        st = self._pst
        return (not self.use_graph and self._grid_done and st.replay is not None
                and not torch.cuda.is_current_stream_capturing())

    def _pdev_post(self) -> None:
        """The device pruned step after its all-reduce: K11, the centre statistics of the next bounds and,
        in a tol > 0 fit, the device convergence latch (flags[1])."""
        st = self._pst
        exact = self.use_graph or st.half_every <= 1 or self.iterations % st.half_every == 0
        if not (self._replay_ok() and not self.spherical and self.dp <= 2048
                and self._replay(("post", exact, self._conv_lim), lambda: self._pdev_post_launches(exact))):
            self._pdev_post_launches(exact)
        self._shift2 = self.shift2
        self._cost_fn = self._device_cost

    def _pdev_post_launches(self, exact: bool) -> None:
        st, k, d = self._pst, self.k, self.d
        if not self.spherical and self.dp <= 2048:
            # K11 + cb_old / cb_cost copies + norms + drifts in one launch, then the centre statistics in one
            K.update_pdev(self.msgs, k, d, self.centers, self.cb, self.dp, self.kp, self.cnorm, self.shift2,
                          self._unit, st.cb_old, st.cb_cost, st.flags, st.cn, st.drift, snap=self._mx)
            # the nearest-centre half distances are recomputed every st.half_every steps (and in captured graphs);
            # between, they are lowered by the drifts (a valid, slightly looser bound: one small launch)
            if exact:
                K.centre_half_stats(self.cb, k, self.dp, st.cn, st.half, st.drift, st.mx, st.tau, st.thr, st.dmax,
                                    st.mc, st.c2, st.count, st.force, st.cum, st.backoff if st.nback > 0 else None,
                                    st.ctr[1:2])
            else:
                K.centre_decay_stats(k, st.cn, st.half, st.drift, st.mx, st.tau, st.thr, st.dmax, st.mc, st.c2,
                                     st.count, st.force, st.cum, st.backoff if st.nback > 0 else None)
        else:
            # cb_old <- cb, and cb_cost <- cb unless converged (frozen steps keep the last live step's centres)
            K.cond_copy(st.cb_cost, self.cb, st.flags, dst_always=st.cb_old)
            self._update_gpu(self.msgs)
            K.centre_stats(self.cb, st.cb_old, k, d, st.mx, st.tau, st.cn, st.half, st.drift, st.thr, st.dmax,
                           st.mc, st.c2, st.count, st.force, cum=st.cum, backoff=st.backoff if st.nback > 0 else None)
        if self._conv_lim is not None:
            K.converge_latch(self.shift2, k, self._conv_lim, st.flags)

    def _seed_from_init(self, sd) -> None:
        """Labels and bounds of every row from the k-means|| init (kmeans_seed_bounds): row x's nearest
        candidate p is within r = sqrt(cost + slack) of it (the candidate pass's f32 distance, slack for
        its rounding), and p's nearest / second-nearest bf16 centre lie at d1 / d2 (f64, rounded
        outward), so the label is a(p) with ub = r + d1 and lb = d2 - r. The first pruned step then
        re-assigns only the rows these bounds do not prove (_step_seeded)."""
        st, n, k, d = self._pst, self.n, self.k, self.d
        if n == 0:
            return
        U = sd.uniq.to(device=self.device, dtype=torch.float64)
        # one launch: per distinct candidate its nearest / second-nearest bf16 centre by direct differences
        # (rounded outward) and its norm rounded up (kmeans_init_fast.hip; was an f64 GEMM + top-k + ~25 ops)
        a, d1, d2, pn32 = K.seed_table(U, self.cb, k)
        qmap = sd.inverse.reshape(-1).to(torch.int32).contiguous()
        if st.cum is not None:
            st.cum.zero_()  # every row's bounds are written here: offsets against zero drift
        K.seed_bounds(sd.nearest[:n], sd.costs[:n], self.xnorm[:n], qmap, a, d1, d2, pn32, 2.0 * self._tau, n,
                      self.labels[:n], st.ub[:n], st.lb[:n])

    def _step_seeded(self) -> None:
        """First Lloyd step after _seed_from_init: the bounds pass (no drift yet) lists the rows the
        init's bounds leave open, the K9r candidate pass re-assigns them, and the sums of every row's
        label are accumulated in full (counting-sort ranks from the labels; the incremental sums start
        from them). Same labels and centres as a full step; more than _PRUNE_CAP candidates on a rank
        fall back to the full pass there (the collectives are the same either way)."""
        st, dl = self._pst, self.delta
        n, k, d, ap = self.n, self.k, self.d, self.aplan
        x, lab, msg = self.x, self.labels, self.msgs[0]
        if n:
            # the gate picks the candidate pass (+ counting-sort ranks of the labels) or, past _PRUNE_CAP
            # candidates, the full pass (which ranks every row itself) — decided on the device
            K.prune_bounds(lab, st.ub, st.lb, st.drift, st.dmax, st.thr, st.c2, k, st.cand, st.count,
                           xn=self.xnorm, cand_lab=st.cand_lab, cand_xn=st.cand_xn, zero_count=True, cum=st.cum)
            K.prune_gate(st.count, st.cap_m, st.flags, st.pmode)
            K.assign_rr_ext(1, x, n, self.dp, self.cb, self.cnorm, ap, self.xnorm, lab, self.cost_part, st.ub, st.lb,
                            st.mc, st.tau, hist=self.hist, rank=self.rank, delta=dl, gate=st.pmode, want=1,
                            cum=st.cum)
            K.assign_rr_ext(2, x, st.cap_m, self.dp, self.cb, self.cnorm, ap, st.cand_xn, lab, None, st.ub, st.lb,
                            st.mc, st.tau, delta=dl, idx=st.cand, n_dev=st.count, lab_in=st.cand_lab, gate=st.pmode,
                            want=0, cum=st.cum)
            K.label_hist(lab, n, ap, self.hist, self.rank, gate=st.pmode, want=0)
        self.cost_part.zero_()
        dl.invalidate()
        dl.gate(0)
        # the seeded upper bounds (r + d1) are loose; the accumulate streams every row anyway and leaves
        # the exact one, |x - c_label| rounded up, so the next step's bounds prove as many rows as after a
        # full pass (the seeded lower bounds stay: d2 - r is far below what they are compared with)
        K.accumulate_sort(x, n, self.dp, d, lab, self.rank, self.hist, ap, k, self.cost_part, self.off, self.seg,
                          self.perm, self.cplan, dl.acc[0], self.slots, gate=dl.mode[0],
                          ub_centres=self.cb, ub=st.ub, qscale=self._qscale, cum=st.cum)
        dl.accumulate(x, self.dp, lab, 0, self.cost_part, ap.grid, msg, qscale=self._qscale)
        self.comm.allreduce_async(msg).wait()
        self._pdev_post()

    def _norms64(self) -> torch.Tensor:
        """||x||² of the device rows summed in f64 (from the row pass, or the feature tensor's cache)."""
        self._ensure_norms()
        return self._xnorm64

    def _device_cost(self) -> torch.Tensor:
        """Cost of the last step's assignment (Spark's per-iteration trainingCost) from what the step
        already holds: Σ_j (Q_j - 2 c_j·S_j + n_j|c_j|²) with S/n the all-reduced f64 sums of that
        assignment, c_j the bf16 centres it compared against (the pruned step's cb_old, else the copy
        _step_gpu keeps) and Q_j = Σ_{i in j} ||x_i||² from the row pass's f64 norms (one deterministic
        group-sum over the labels, all-reduced) — ~1e-11 relative even far from the origin, where the
        f32 norms lost percents, and no pass over X. Collective: every rank reads
        it together. (With the sum grid active — _sum_grid — S holds the gridded values, and the cost
        is that of the values the centres were computed from.)"""
        k, d, n = self.k, self.d, self.n
        cb = self._pst.cb_cost if self._pdev else self._cb_cost
        if k <= 4096:
            # Q_j as integer limbs on the grid of the global max ||x||² (exactsum.hip): they add exactly, so Q —
            # and the cost — are the same bits for any split of the rows over ranks (the scaling curve fits one
            # problem at every N; an f64 all-reduce of per-rank sums rounded once per rank)
            bound = self._xmax_dev()
            limbs = torch.zeros(2 * k, dtype=torch.int64, device=self.device)
            if n:
                lab = self.labels[:n]
                lab = lab if lab.dtype == torch.int32 and lab.is_contiguous() else lab.to(torch.int32).contiguous()
                K.fixsum(self._norms64()[:n], n, bound, 1.0, lab=lab, k=k, limbs=limbs)
            self.comm.allreduce_(limbs)
            q = K.fixsum_finalize(limbs, k, bound, 1.0)
        else:
            if n:
                # (engine labels are always in [0, k): no range check, no host read)
                q = group_reduce(self.labels[:n], self._norms64()[:n], k, "sum",
                                 ids_in_range=True).to(torch.float64).contiguous()
            else:
                q = torch.zeros(k, dtype=torch.float64, device=self.device)
            self.comm.allreduce_(q)
        return K.cost_combine(q, self.msgs, k, d, self._unit, cb)

    def _xmax_dev(self) -> torch.Tensor:
        """Device f32 max ||x||² over every rank: the grid bound of the partition-invariant sums (K.fixsum).
        The device pruned step keeps it (st.mx); other engines reduce it once (the norms are fixed)."""
        self._ensure_norms()
        if self._pdev:
            return self._pst.mx
        mx = self._gxmax
        if mx is None:
            mx = (self._xnorm[: self.n].max().reshape(1) if self.n
                  else torch.zeros(1, dtype=torch.float32, device=self.device))
            if self.comm.is_distributed:
                self.comm.allreduce_(mx, op="max")
            self._gxmax = mx
        return mx

    def _exact_cost(self) -> torch.Tensor:
        """Cost of the last step's assignment (Spark's per-iteration cost) on the device rows: one exact
        pass Σ_i |x_i - c_lab(i)|² (f64 differences and squares, K.cost_pass) against the bf16 centres that
        assignment compared with (the pruned step's cb_old, else the copy _step_gpu keeps), all-reduced.
        Read lazily — a fit whose cost is never read never pays the pass. The expanded per-centre form
        Σ(Q_j - 2c_j·S_j + n_j|c_j|²) it replaces lost percents for data far from the origin (|x|² >> cost)."""
        cb = self._pst.cb_old if self._pdev else self._cb_cost
        if self.n:
            cost = K.cost_pass(self.x, self.n, self.dp, self.labels, cb)
        else:
            cost = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.comm.allreduce_(cost)
        return cost[0]

    def _pdev_last(self) -> tuple:
        """(full pass?, re-assigned rows) of the last device pruned step (synchronises)."""
        pm = self._pst.pmode.cpu().tolist()
        return (bool(pm[0]), int(self.n if pm[0] else pm[1]))

    # ------------------------------------------------------------------ pruned (exact) steps
    # Error allowance of a squared distance from the full assign, relative to |x|² + |c|²: f32
    # accumulation of exact bf16 products is within D·2^-24·Σ|x_j c_j| <= 0.77e-5·(|x|² + |c|²) at D = 256.
    _PRUNE_TAU = 3e-5
    _PRUNE_CAP = 0.3  # a rank re-assigns all of its rows when more than this fraction are candidates


    def prune_stats(self) -> dict:
        """Last pruned step: whether this rank re-assigned all rows, and how many it re-assigned."""
        if self._pst is None:
            return {}
        full, m = self._pdev_last() if self._pdev else self._pst.last
        return {"full": bool(full), "reassigned_rows": int(m), "rows": self.n}

    def prune_history(self) -> list:
        """(full step?, re-assigned rows) of every pruned step of this engine, rank-local."""
        return [] if self._pst is None else list(self._pst.history)

    def converged(self, tol: float) -> bool:
        """Spark's rule: converged iff every centre moved at most tol (euclidean)."""
        if self._shift2 is None and self._shift_pair is not None:
            new, old = self._shift_pair  # the screen's one-rank update: the exact path's expression, on demand
            self._shift2 = ((new - old) ** 2).sum(1)
        if self._shift2 is None:
            return False
        lim = 2.0 * tol if self.spherical else tol * tol  # cosine: 1 - cos = ||a - b||² / 2 on unit vectors
        return bool((self._shift2 <= lim).all().item())

    def fit(self, max_iter: int, tol: float, start_iter: int = 0, on_iter=None) -> int:
        """Lloyd iterations until every centre moves <= tol or max_iter. ``start_iter`` resumes a
        checkpointed fit; ``on_iter(it)`` runs after each iteration (checkpoint hook)."""
        # (a refresh interval re-accumulates from counting-sort ranks that a frozen step does not rebuild:
        # such fits take the synchronous loop — ADVICE r4)
        if (tol > 0 and self._pdev and on_iter is None and not self.refresh_interval
                and os.environ.get("CML_KMEANS_LAGGED_TOL", "1") != "0"):
            return self._fit_lagged(max_iter, tol, start_iter)
        it = start_iter
        while it < max_iter:
            maybe_fail("kmeans.iteration", it)  # crash point (SURVEY.md §5.3 "mid-iteration k")
            with trace("kmeans.step"):
                self.step()
            it += 1
            if on_iter is not None:
                on_iter(it)
            if tol > 0 and self.converged(tol):
                break
            # the weighted MFMA step at tol = 0: a step that moved no centre is a fixed point (the next
            # assignment compares with the same bf16 centres, and the sums are order-free), so every later
            # step would give the same centres, cost and labels — Spark's rule (moved <= tol) stops here
            if tol == 0 and self._wfast and self.converged(0.0):
                break
        return it

    def _fit_lagged(self, max_iter: int, tol: float, start_iter: int = 0, window: int = 2) -> int:
        """A tol > 0 fit with no per-step host synchronisation: every step latches Spark's convergence
        test on the device (kmeans_converge_latch: all centres moved <= tol) and a converged engine's
        later steps are frozen no-ops (kmeans_prune_gate: no row re-assigned, so sums and centres stay
        bit for bit). The flag of each step is copied to pinned memory behind its work; the host reads
        it ``window`` steps late (waiting only for that older step's event, so the GPU always has queued
        work) and stops at the first converged step — the same iteration count, centres, labels and
        cost as the synchronous loop, plus at most ``window`` frozen steps of a few small kernels."""
        st = self._pst
        self._conv_lim = 2.0 * tol if self.spherical else tol * tol
        st.done.zero_()
        total = max(0, max_iter - start_iter)
        flags = torch.zeros(max(total, 1), dtype=torch.int32, pin_memory=True)
        events = []
        stop, checked, it = None, 0, start_iter
        try:
            while it < max_iter:
                maybe_fail("kmeans.iteration", it)
                with trace("kmeans.step"):
                    self.step()
                i = it - start_iter
                flags[i:i + 1].copy_(st.done, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                events.append(ev)
                it += 1
                while checked <= i - window:  # the step `window` back: its flag is (nearly) ready
                    events[checked].synchronize()
                    if int(flags[checked]) != 0:
                        stop = start_iter + checked + 1
                        break
                    checked += 1
                if stop is not None:
                    break
            while stop is None and checked < len(events):
                events[checked].synchronize()
                if int(flags[checked]) != 0:
                    stop = start_iter + checked + 1
                checked += 1
        finally:
            self._conv_lim = None
            st.done.zero_()  # later steps of this engine (more iterations, assigns) run live again
        return stop if stop is not None else it

    # ------------------------------------------------------------------ prediction / cost
    def final_labels(self, in_place: bool = False) -> torch.Tensor:
        """Labels of every local row against the current (final) centres — what ``transform`` with the
        fitted model predicts (Spark's summary.clusterSizes counts these). After device pruned steps this is
        one pruned assign: the bounds pass against the last update's drifts lists the rows the bounds no
        longer prove, and K9r re-assigns only those (the full pass when there are too many), on copies of
        the labels and bounds — the engine's own step state is untouched. Other paths run a full assign."""
        n, k = self.n, self.k
        c = getattr(self._scr, "cert", None) if self._scr is not None else None
        if self._screen and n and c is not None and c.valid:
            # certified pruned assign on copies: the bounds moved by the last update's drifts prove most
            # labels; the rest are tightened and re-assigned by the exact fold (same labels as a full pass)
            st = self._scr
            lab, u, l = c.lab.clone(), st.ub.clone(), st.lb.clone()
            ctr = torch.zeros(4 + 2 * k, dtype=torch.int32, device=self.device)
            la, lbl = torch.empty_like(c.la), torch.empty_like(c.lbl)
            s_, drift, dtop = torch.empty_like(c.s), torch.empty_like(c.drift), torch.zeros_like(c.dtop)
            K.cert_stats(self.centers, c.C_cur, s_, drift, dtop, zero=ctr)
            K.cert_bounds(lab, u, l, drift, dtop, s_, n, la, ctr[0:1])
            K.cert_tighten(self.x, self.centers, lab, u, l, s_, la, ctr[0:1], lbl, ctr[1:2])
            K.exact_top2(self.x, self.centers, lab, u, l, idx=lbl, n_dev=ctr[1:2])
            return lab[:n]
        if not (self._pdev and n):
            return self.assign()[0]
        st, ap = self._pst, self.aplan
        if in_place:
            # the fit's last use of this engine (cluster_sizes_async(consume=True)): the pass updates the step's
            # own labels, bounds and candidate lists instead of copies (at 100M rows the three copies moved
            # 2.4 GB); the engine is marked consumed, so no later step runs on the now mismatched state
            self._consumed = True
            lab, ub, lb = self.labels, st.ub, st.lb
            cand, cand_lab, cand_xn, count = st.cand, st.cand_lab, st.cand_xn, st.count
            flags, pmode = K.zeros_block(self.device, [(2, torch.int32), (2, torch.int32)])
            count.zero_()
        else:
            lab, ub, lb = self.labels.clone(), st.ub.clone(), st.lb.clone()
            pad, i32 = st.cand.shape[0], torch.int32
            cand, cand_lab, cand_xn, count, flags, pmode = K.zeros_block(self.device, [
                (pad, i32), (pad, i32), (pad, torch.float32), (1, i32), (2, i32), (2, i32)])
        K.prune_bounds(lab, ub, lb, st.drift, st.dmax, st.thr, st.c2, k, cand, count, xn=self.xnorm, cand_lab=cand_lab,
                       cand_xn=cand_xn, zero_count=False, cum=st.cum)
        K.prune_gate(count, st.cap_m, flags, pmode)
        K.assign_rr_ext(1, self.x, n, self.dp, self.cb, self.cnorm, ap, self.xnorm, lab, None, ub, lb, st.mc, st.tau,
                        gate=pmode, want=1, cum=st.cum)
        K.assign_rr_ext(2, self.x, st.cap_m, self.dp, self.cb, self.cnorm, ap, cand_xn, lab, None, ub, lb, st.mc,
                        st.tau, idx=cand, n_dev=count, lab_in=cand_lab, gate=pmode, want=0, cum=st.cum)
        return lab[:n]

    def cluster_sizes(self) -> List[int]:
        """Global row count of every cluster under the final centres (a collective)."""
        return self.cluster_sizes_async()()

    def cluster_sizes_async(self, consume: bool = False):
        """Enqueue the final-centre counts of every cluster and their all-reduce (no host read) and return
        a zero-argument reader of the result. Every rank calls this together (at the end of ``fit``);
        the reader itself is no collective — one rank alone may read it — and it holds only the k-long
        count buffer, not the engine (a lazy collective deadlocked ``if rank == 0: print(
        summary.clusterSizes)`` and kept every per-row buffer of the fit alive)."""
        k, n = self.k, self.n
        if n and self.device.type == "cuda":
            lab = self.final_labels(in_place=consume)
            cnt = torch.zeros(k, dtype=torch.int32, device=self.device)
            K.int_hist(lab.to(torch.int32).contiguous(), n, k, cnt)  # integer counts: no bincount host sync
            sizes = cnt.to(torch.int64)
        elif n:
            sizes = torch.bincount(self.final_labels().long(), minlength=k).to(torch.int64)
        else:
            sizes = torch.zeros(k, dtype=torch.int64, device=self.device)
        h = self.comm.allreduce_async(sizes)

        def read() -> List[int]:
            return [int(v) for v in h.wait().cpu().tolist()]
        return read

    def assign(self, centers: Optional[torch.Tensor] = None):
        """(labels, squared distance) of every local row against `centers` (default: current)."""
        if centers is not None:
            centers = torch.as_tensor(centers, dtype=torch.float64, device=self.device)
        if not self.gpu:
            return K.assign_reference(self.x, self.centers if centers is None else centers)
        self._ensure_norms()
        return self._assign_all(self.centers if centers is None else centers)

    def _assign_all(self, centers: torch.Tensor):
        """(labels, distances) of every local row on the MFMA path (streamed chunk by chunk out of core)."""
        if self._hs is None:
            return assign_gpu(self.x, self.dp, self.d, centers, self.xnorm)
        lab = torch.empty(max(self.n, 1), dtype=torch.int32, device=self.device)
        best = torch.empty(max(self.n, 1), dtype=torch.float32, device=self.device)
        for _, r0, r1, xc in self._x_chunks():
            if r1 > r0:
                lc, bc = assign_gpu(xc, self.dp, self.d, centers, self._xnorm[r0:r1])
                lab[r0:r1], best[r0:r1] = lc, bc
        return lab[: self.n], best[: self.n]

    @property
    def last_cost(self):
        """Cost of the last step's assignment (a device scalar); the device pruned step evaluates it
        on first access (a collective: every rank reads it together)."""
        if self._cost_fn is not None:
            fn, self._cost_fn = self._cost_fn, None
            self._last_cost = fn()
        return self._last_cost

    @last_cost.setter
    def last_cost(self, v) -> None:
        self._cost_fn = None
        self._last_cost = v

    def training_cost(self) -> float:
        """Spark's trainingCost: sum of squared distances, or of cosine distances (spherical)."""
        if self.last_cost is None:
            return float("nan")
        c = float(self.last_cost.item())
        return c / 2.0 if self.spherical else c

    # ------------------------------------------------------------------ initialisation
    def init_random(self, seed: int) -> np.ndarray:
        return kmeans_init.init_random(self, seed)

    def init_kmeans_parallel(self, seed: int, steps: int = 2, as_device: bool = False):
        return kmeans_init.init_kmeans_parallel(self, seed, steps, as_device)

    def _const(self, values, dtype) -> torch.Tensor:
        """A small device tensor of host values without a blocking copy (pinned staging, non_blocking): a
        torch.tensor(..., device=cuda) is a pageable copy that waits for every queued kernel, which in the
        fit's hot path stalled the host behind the row pass (profiles/r5/shard/)."""
        h = torch.tensor(values, dtype=dtype, pin_memory=self.device.type == "cuda")
        return h.to(self.device, non_blocking=True)


def assign_gpu(x: torch.Tensor, dp: int, d: int, centers: torch.Tensor, xnorm: Optional[torch.Tensor] = None):
    """K9 against an arbitrary centre set (used for transform, cost and k-means||)."""
    k = centers.shape[0]
    kp = round_up(max(k, 1), 32)
    dev = x.device
    n = x.shape[0]
    cb = torch.zeros((kp, dp), dtype=torch.bfloat16, device=dev)
    cn = torch.zeros(kp, dtype=torch.float32, device=dev)
    cent = centers.to(device=dev, dtype=torch.float64).contiguous().clone()
    K.update_centers(None, k, d, cent, cb, dp, kp, cn, None, snap=K.mx_applies(x))
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    best = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    if n:
        if xnorm is None:
            xnorm = cached_row_sqnorm(x, n, dp)
        plan = K.plan_assign(n, dp, k, dev.index or 0, fp8=K.is_fp8(x))
        K.assign_bf16(x, n, dp, cb, cn, plan, labels, best, None, xnorm=xnorm)
    return labels[:n], best[:n]


def local_kmeans_pp(points: np.ndarray, weights: np.ndarray, k: int, seed: int, max_iter: int = 30,
                    spherical: bool = False) -> np.ndarray:
    """Weighted k-means++ seeding + weighted Lloyd on the candidate set (host, float64): the native
    host twin of the device kernels (``ops.kmeans_ops.local_kmeans``). ``spherical``: centres are
    renormalised after every mean (cosine KMeans)."""
    return K.local_kmeans(torch.as_tensor(np.ascontiguousarray(points, dtype=np.float64)),
                          torch.as_tensor(np.ascontiguousarray(weights, dtype=np.float64)), k, seed,
                          max_iter=max_iter, spherical=spherical).numpy()


def local_kmeans_pp_device(points: torch.Tensor, weights: torch.Tensor, k: int, seed: int,
                           max_iter: int = 30, spherical: bool = False) -> np.ndarray:
    """local_kmeans_pp on ``points.device`` (HIP kernels on a GPU tensor); bitwise the host result."""
    return K.local_kmeans(points, weights, k, seed, max_iter=max_iter, spherical=spherical).cpu().numpy()
