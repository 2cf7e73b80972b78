"""BisectingKMeans (Spark ``org.apache.spark.ml.clustering.BisectingKMeans``).

Divisive hierarchical clustering for segmenting hospitals / admissions when the number of
natural groups is unknown (the reference's feature table, ref.py:134-136).  The algorithm is
Spark's ``mllib.clustering.BisectingKMeans.runWithWeight`` step for step:

* nodes carry Spark's raw indices (root 1, children 2i and 2i+1); a level works on the
  ACTIVE set only — the clusters created on the previous level.  Every active cluster leaves
  the active set at the end of the level, divided or not: an undivided one is a permanent leaf.
* divisible: ``size >= minSize`` and ``cost > EPSILON * size``, where ``minSize`` is
  ``ceil(minDivisibleClusterSize)`` (or ``ceil(fraction * n)`` below 1.0) and EPSILON is the
  double machine epsilon (MLUtils.EPSILON).  When more clusters are divisible than leaves are
  still needed, the LARGEST (by size) are divided.
* each divided cluster is seeded by ``splitCenter``: centre ∓ 1e-4·‖centre‖·u with u uniform
  [0, 1)^d drawn from ``java.util.Random(seed)`` (reimplemented bit-exactly, ``JavaRandom``),
  then ALL divided clusters of the level run exactly ``maxIter`` restricted 2-means iterations
  together (each row chooses between its own cluster's two children, the left one on ties; a
  child that attracts no row drops out, as in Spark's updateAssignments).  One iteration is one
  pass over the local rows plus ONE all-reduce of every child's (Σx, count, Σ‖x‖²).
* summaries are Spark's ClusterSummary: centre Σx/n, cost max(Σ‖x‖² − n‖c‖², 0).
* the tree (buildTree): internal iff the left child exists; leaves are numbered 0.. in
  left-first depth order, internal nodes -1, -2, ...; height = max distance centre -> child.
* ``weightCol`` (weights w >= 0, finite, not null): a summary holds S = Σ w x, W = Σ w, Q = Σ w‖x‖²
  and N, the number of ROWS (a row of weight 0 counts 1). Centre S / W, cost max(Q − W‖c‖², 0),
  size N: ``minDivisibleClusterSize``, "largest first", ``cost > EPSILON·size``, the saved node
  sizes and ``summary.clusterSizes`` all count rows. A child with W == 0 drops out like a child
  without a row.
* ``distanceMeasure="cosine"`` (CosineDistanceMeasure): a zero-length row raises on every rank;
  S = Σ w x/‖x‖, the centre is S / W scaled to unit length, the cost max(W − S·c, 0); both split
  centres are scaled to unit length; rows compare 1 − x·c/‖x‖; ``computeCost`` is Σ (1 − cos) and a
  node's height the largest cosine distance to a child centre.

One iteration runs, per column: the K27 kernel (``ops/bisect_ops.py``, ``_native/csrc/bisect.hip``)
on bf16 / e4m3 device columns of a supported width, for both measures and with or without weights
(``CML_BISECT_KERNEL=0``: off); the chunked torch form below for euclidean unweighted fits on
everything else; ``bisect_step_reference`` for the rest (cosine or weighted fits on CPU frames, f32 /
f64, host-resident and wide columns).

Parity notes (pyspark is not importable here, so parity is unpinned by fixture): Spark divides
the clusters of a level in its Map's iteration order when drawing the split noise; here they are
drawn in ascending node-index order.  Prediction walks the tree from the root, taking the
closer child at every level (``ClusteringTreeNode.predict``).  Save: ml metadata under
``path/metadata`` and the mllib ``BisectingKMeansModel`` (SaveLoadV3_0: JSON metadata with
rootId, k, distanceMeasure, trainingCost + one parquet row per node) under ``path/data``.
"""
from __future__ import annotations

import json
import math
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from ..ops import bisect_ops as BO
from ..ops import silhouette_ops as SO
from ..ops.group_ops import group_sum_rows

from ..sql import types as T
from ..sql.column import ColumnData
from . import util as U
from .util import java_hash
from .base import Estimator, Model
from .feature import _replace_col
from .util import JavaRandom  # noqa: F401 (re-exported)
from .linalg import as_array

EPSILON = np.finfo(np.float64).eps  # MLUtils.EPSILON: 2.220446049250313e-16
LEVEL_LIMIT = 63                    # log2(Long.MaxValue): raw indices stay below 2^63
_CHUNK = 1 << 24                    # elements per f64 row chunk (bounded temporaries)


class _Node:
    def __init__(self, center: np.ndarray, size: float, cost: float, index: int = -1, height: float = 0.0):
        self.center, self.size, self.cost = np.asarray(center, dtype=np.float64), size, cost
        self.children: List["_Node"] = []
        self.index = index
        self.height = height


class _Summary:
    def __init__(self, size: int, center: np.ndarray, cost: float):
        self.size, self.center, self.cost = size, center, cost


def _summarize(x: torch.Tensor, idx: torch.Tensor, keys: List[int], comm) -> Dict[int, _Summary]:
    """Spark ``summarize`` restricted to the clusters ``keys``: per cluster (Σx, n, Σ‖x‖²),
    all-reduced in one message; clusters with no row anywhere are absent from the result."""
    d = int(x.shape[1])
    m = len(keys)
    acc = torch.zeros((m, d + 2), dtype=torch.float64, device=x.device)
    if m and x.shape[0]:
        kt = torch.as_tensor(sorted(keys), dtype=torch.int64, device=x.device)
        step = max(1, _CHUNK // max(d, 1))
        for r0 in range(0, int(x.shape[0]), step):
            ii = idx[r0:r0 + step]
            slot = torch.searchsorted(kt, ii).clamp(max=m - 1)
            sel = kt[slot] == ii
            if not bool(sel.any()):
                continue
            xs = x[r0:r0 + step][sel].to(torch.float64)
            part = torch.cat([xs, torch.ones((xs.shape[0], 1), dtype=torch.float64, device=x.device),
                              (xs * xs).sum(1, keepdim=True)], 1)
            acc += group_sum_rows(slot[sel], part, m)  # K25 per-cluster column sums on the GPU
    comm.allreduce_(acc)
    a = acc.cpu().numpy()
    out = {}
    for j, key in enumerate(sorted(keys)):
        n = a[j, d]
        if n <= 0:
            continue
        c = a[j, :d] / n
        out[key] = _Summary(int(round(n)), c, max(float(a[j, d + 1]) - n * float(c @ c), 0.0))
    return out


def _update_assignments(x: torch.Tensor, idx: torch.Tensor, divisible: List[int],
                        centers: Dict[int, np.ndarray]) -> torch.Tensor:
    """Spark ``updateAssignments``: rows of a divided cluster i move to the closer of its
    children 2i / 2i+1 that still exist (left on ties); every other row keeps its index."""
    out = idx.clone()
    if not divisible or x.shape[0] == 0:
        return out
    d = int(x.shape[1])
    dv = torch.as_tensor(sorted(divisible), dtype=torch.int64, device=x.device)
    m = dv.numel()
    inf = float("inf")
    lc = np.full((m, d), np.nan)
    rc = np.full((m, d), np.nan)
    for j, i in enumerate(sorted(divisible)):
        if 2 * i in centers:
            lc[j] = centers[2 * i]
        if 2 * i + 1 in centers:
            rc[j] = centers[2 * i + 1]
    L = torch.as_tensor(lc, device=x.device)
    R = torch.as_tensor(rc, device=x.device)
    has_l = ~torch.isnan(L[:, 0])
    has_r = ~torch.isnan(R[:, 0])
    step = max(1, _CHUNK // max(d, 1))
    for r0 in range(0, int(x.shape[0]), step):
        ii = idx[r0:r0 + step]
        slot = torch.searchsorted(dv, ii).clamp(max=m - 1)
        sel = (dv[slot] == ii) & (has_l[slot] | has_r[slot])
        if not bool(sel.any()):
            continue
        rows = torch.nonzero(sel).flatten()
        s = slot[rows]
        xs = x[r0:r0 + step][rows].to(torch.float64)
        dl = torch.where(has_l[s], ((xs - torch.nan_to_num(L[s])) ** 2).sum(1), torch.full_like(xs[:, 0], inf))
        dr = torch.where(has_r[s], ((xs - torch.nan_to_num(R[s])) ** 2).sum(1), torch.full_like(xs[:, 0], inf))
        child = 2 * ii[rows] + (dr < dl).to(torch.int64)
        out[r0 + rows] = child
    return out


def _split_center(center: np.ndarray, rnd: JavaRandom):
    level = 1e-4 * float(np.linalg.norm(center))
    noise = np.array([rnd.next_double() for _ in range(center.size)])
    return center - level * noise, center + level * noise


def _unit(v: np.ndarray) -> np.ndarray:
    nrm = float(np.linalg.norm(v))
    return v / nrm if nrm > 0 else v


def _split_center_cosine(center: np.ndarray, rnd: JavaRandom):
    left, right = _split_center(center, rnd)
    return _unit(left), _unit(right)


def _summaries(a: np.ndarray, keys: List[int], d: int, cosine: bool) -> Dict[int, _Summary]:
    """Spark's ClusterSummary of every key from the all-reduced ``[S | W | Q | N]`` rows (``S`` may be zero
    padded beyond ``d``): size N (rows, whatever their weights), centre S / W (cosine: scaled to unit length),
    cost max(Q - W|c|^2, 0) (cosine: max(W - S.c, 0)). A cluster of no row or no weight is absent."""
    out = {}
    for j, key in enumerate(keys):
        S, W, Q, N = a[j, :d], float(a[j, -3]), float(a[j, -2]), a[j, -1]
        if N <= 0 or W <= 0:
            continue
        c = S / W
        if cosine:
            c = _unit(c)
            cost = max(W - float(S @ c), 0.0)
        else:
            cost = max(Q - W * float(c @ c), 0.0)
        out[key] = _Summary(int(round(N)), c, cost)
    return out


class _ChunkedStep:
    """The euclidean unweighted iteration in chunked f64 torch (``_update_assignments`` + ``_summarize``)."""

    def __init__(self, x, comm):
        self.x, self.comm = x, comm
        self.idx = torch.ones(x.shape[0], dtype=torch.int64, device=x.device)  # ROOT_INDEX = 1

    def root(self):
        return _summarize(self.x, self.idx, [1], self.comm)

    def begin(self, dvi):
        self.dvi = dvi

    def iterate(self, centers):
        child_idx = _update_assignments(self.x, self.idx, self.dvi, centers)
        return _summarize(self.x, child_idx, [c for i in self.dvi for c in (2 * i, 2 * i + 1)], self.comm)

    def finish(self, centers):
        self.idx = _update_assignments(self.x, self.idx, self.dvi, centers)


class _StatStep:
    """One iteration as ``ops.bisect_ops`` evaluates it, for either measure and with row weights: the K27
    kernel on bf16 / e4m3 device columns (``kernel=True``: a plan of the level's rows once per level, the row
    norms and the factor of S once per fit), the reference form on everything else. Either way an iteration is
    one pass over the rows of the divided nodes and ONE all-reduce of the ``[2m, d + 3]`` statistics."""

    def __init__(self, x, d, comm, weights, cosine, kernel):
        self.d, self.comm, self.w, self.cosine, self.kernel = d, comm, weights, cosine, kernel
        self.idx = torch.ones(x.shape[0], dtype=torch.int64, device=x.device)
        self.omega = self.nrm2 = None
        if kernel:
            from ..models.kmeans import to_device_matrix
            self.x = to_device_matrix(x, d)  # a copy only when the layout is not already the kernels'
            self.nrm2 = SO.row_sqnorm(self.x)
            self.zero = (self.nrm2 == 0).any() if cosine else False
            if cosine:
                nrm = torch.sqrt(self.nrm2.clamp_(min=torch.finfo(torch.float64).tiny))
                self.omega = torch.reciprocal(nrm) if weights is None else weights / nrm
                self.nrm2 = None  # Q is not kept for cosine
            else:
                self.omega = weights
        else:
            self.x = x
            self.zero = cosine and SO.has_zero_rows(x)
        self.width = int(self.x.shape[1])

    def _run(self, centers, want_sums):
        m = len(self.dvi)
        tab = np.zeros((m, 2, self.width))
        alive = np.zeros((m, 2), dtype=bool)
        for j, i in enumerate(self.dvi):
            for h in (0, 1):
                if 2 * i + h in centers:
                    tab[j, h, :self.d] = centers[2 * i + h]
                    alive[j, h] = True
        dev = self.x.device
        tab, alive = torch.as_tensor(tab, device=dev), torch.as_tensor(alive, device=dev)
        if self.kernel:
            choice, stats = BO.bisect_step(self.x, self.plan, tab, alive, self.omega, self.w, self.nrm2,
                                           self.cosine, want_sums)
        else:
            choice, stats = BO.bisect_step_reference(self.x, self.slot, tab, alive, self.w, self.cosine, want_sums)
        return choice, stats, alive

    def _reduce(self, stats, keys):
        stats = self.comm.allreduce_(stats.to(self.comm.device))
        return _summaries(stats.cpu().numpy(), keys, self.d, self.cosine)

    def root(self):
        """The root's summary: one node whose only live child is the left one takes every row."""
        self.begin([0])
        _, stats, _ = self._run({0: np.zeros(self.d)}, True)
        return {1: s for s in self._reduce(stats[:1], [0]).values()}

    def begin(self, dvi):
        self.dvi = dvi
        dv = torch.as_tensor(dvi, dtype=torch.int64, device=self.idx.device)
        if dvi == [0]:
            slot = torch.zeros_like(self.idx)
        else:
            slot = torch.searchsorted(dv, self.idx).clamp_(max=len(dvi) - 1)
            slot = torch.where(dv[slot] == self.idx, slot, torch.full_like(slot, -1))
        if self.kernel:
            self.plan = BO.make_plan(slot, len(dvi))
        else:
            self.slot = slot

    def iterate(self, centers):
        _, stats, _ = self._run(centers, True)
        return self._reduce(stats, [c for i in self.dvi for c in (2 * i, 2 * i + 1)])

    def finish(self, centers):
        choice, _, alive = self._run(centers, False)
        moves = alive.any(1)
        if self.kernel:
            rows = self.plan.perm
            move = moves[self.plan.pslot.to(torch.int64)]
            old = self.idx[rows]
            self.idx[rows] = torch.where(move, 2 * old + choice.to(torch.int64), old)
        else:
            move = (self.slot >= 0) & moves[self.slot.clamp(min=0)]
            self.idx = torch.where(move, 2 * self.idx + choice.to(torch.int64), self.idx)


class BisectingKMeans(Estimator):
    _params = {
        "featuresCol": ("features", "features column name", str),
        "predictionCol": ("prediction", "prediction column name", str),
        "k": (4, "the desired number of leaf clusters (> 1)", int),
        "maxIter": (20, "max number of iterations of every 2-means split (>= 0)", int),
        "seed": (java_hash("org.apache.spark.ml.clustering.BisectingKMeans"), "random seed", int),
        "minDivisibleClusterSize": (1.0, "minimum points (>= 1.0) or fraction (< 1.0) of a divisible cluster", float),
        "distanceMeasure": ("euclidean", "'euclidean' or 'cosine'", str),
        "weightCol": (None, "weight column name", None),
    }

    def __init__(self, featuresCol=None, predictionCol=None, k=None, maxIter=None, seed=None,
                 minDivisibleClusterSize=None, distanceMeasure=None, weightCol=None):
        super().__init__(featuresCol=featuresCol, predictionCol=predictionCol, k=k, maxIter=maxIter, seed=seed,
                         minDivisibleClusterSize=minDivisibleClusterSize, distanceMeasure=distanceMeasure,
                         weightCol=weightCol)
        self._defaultParamMap.pop("weightCol", None)

    def _stepper(self, df, x, cosine):
        """The iteration of this column: K27 for bf16 / e4m3 device columns of a supported width, the chunked
        torch form for euclidean unweighted fits on everything else, the reference form for the rest."""
        from .clustering import _weights
        comm = df._comm
        weights = None
        if self.isSet("weightCol") and self.getOrDefault("weightCol"):
            weights = _weights(df, self.getOrDefault("weightCol"), x.device)
        d = int(x.shape[1])
        kernel = False
        if x.is_cuda and x.dtype in (torch.bfloat16, torch.float8_e4m3fn) and BO.kernel_enabled():
            from ..models.kmeans import padded_dim_fp8
            from ..utils.device import padded_dim
            dp = padded_dim_fp8(d) if x.dtype == torch.float8_e4m3fn else padded_dim(d)
            kernel = BO.kernel_supported(x.dtype, dp)
        if not cosine and weights is None and not kernel:
            return _ChunkedStep(x, comm)
        step = _StatStep(x, d, comm, weights, cosine, kernel)
        if cosine:
            # a zero-length row on one rank makes every rank raise (nobody is left in the collectives below)
            flag = torch.tensor([1.0 if bool(step.zero) else 0.0], dtype=torch.float64, device=comm.device)
            comm.allreduce_(flag, op="max")
            if flag.item() > 0:
                raise ValueError(SO.ZERO_ROW)
        return step

    def _fit(self, df):
        measure = self.getDistanceMeasure()
        if measure not in ("euclidean", "cosine"):
            raise ValueError(f"distanceMeasure must be 'euclidean' or 'cosine', got {measure!r}")
        cosine = measure == "cosine"
        k = self.getK()
        if k < 2:
            raise ValueError("k must be > 1")
        max_iter = self.getMaxIter()
        x = df._feature_matrix(self.getFeaturesCol())
        step = self._stepper(df, x, cosine)
        split = _split_center_cosine if cosine else _split_center
        active = step.root()
        if not active:
            raise ValueError("BisectingKMeans needs at least one row")
        n = active[1].size
        mds = self.getMinDivisibleClusterSize()
        min_size = math.ceil(mds) if mds >= 1.0 else math.ceil(mds * n)
        inactive: Dict[int, _Summary] = {}
        rnd = JavaRandom(self.getSeed())
        needed, level = k - 1, 1
        while active and needed > 0 and level < LEVEL_LIMIT:
            div = {i: s for i, s in active.items() if s.size >= min_size and s.cost > EPSILON * s.size}
            if len(div) > needed:  # take the larger ones (stable by index on equal sizes)
                div = dict(sorted(div.items(), key=lambda kv: (-kv[1].size, kv[0]))[:needed])
            if not div:
                inactive.update(active)
                active = {}
                break
            dvi = sorted(div)
            centers: Dict[int, np.ndarray] = {}
            for i in dvi:
                centers[2 * i], centers[2 * i + 1] = split(div[i].center, rnd)
            step.begin(dvi)
            new = {}
            for _ in range(max(max_iter, 1)):
                new = step.iterate(centers)
                centers = {c: s.center for c, s in new.items()}
            step.finish(centers)
            inactive.update(active)
            active = new
            needed -= len(div)
            level += 1
        clusters = {**inactive, **active}
        root = _build_tree(clusters, cosine)
        m = BisectingKMeansModel(root)
        self._copyValues(m)
        m._training_cost = float(sum(nd.cost for nd in m._leaves))
        m._summary = BisectingKMeansSummary(m, df, len(m._leaves), max_iter, m._training_cost)
        return m


def _centre_distance(a: np.ndarray, b: np.ndarray, cosine: bool) -> float:
    if cosine:
        return float(1.0 - (a @ b) / (np.linalg.norm(a) * np.linalg.norm(b)))
    return float(np.linalg.norm(a - b))


def _build_tree(clusters: Dict[int, _Summary], cosine: bool = False) -> _Node:
    """Spark ``buildTree``: internal iff the left child exists; leaf indices 0.. in left-first
    depth order, internal indices -1, -2, ...; height = max distance (of the fit's measure) to a
    child centre."""
    counters = {"leaf": 0, "internal": -1}

    def build(raw: int) -> _Node:
        s = clusters[raw]
        if 2 * raw in clusters:
            node = _Node(s.center, s.size, s.cost, counters["internal"])
            counters["internal"] -= 1
            kids = [c for c in (2 * raw, 2 * raw + 1) if c in clusters]
            node.height = max(_centre_distance(s.center, clusters[c].center, cosine) for c in kids)
            node.children = [build(c) for c in kids]
            return node
        node = _Node(s.center, s.size, s.cost, counters["leaf"])
        counters["leaf"] += 1
        return node

    return build(1)


class BisectingKMeansSummary:
    def __init__(self, model, df, k, num_iter, cost):
        self._model, self._df = model, df
        self.k, self.numIter, self.trainingCost = k, num_iter, cost
        self.featuresCol = model.getFeaturesCol()
        self.predictionCol = model.getPredictionCol()

    @property
    def predictions(self):
        return self._model.transform(self._df)

    @property
    def cluster(self):
        return self.predictions.select(self.predictionCol)

    @property
    def clusterSizes(self) -> List[int]:
        lab = self._model._predict_tensor(self._df._feature_matrix(self.featuresCol))
        sizes = torch.bincount(lab, minlength=self.k).to(torch.float64)
        self._df._comm.allreduce_(sizes)
        return [int(v) for v in sizes.cpu().tolist()]


class BisectingKMeansModel(Model):
    _params = BisectingKMeans._params

    def __init__(self, root: Optional[_Node] = None):
        super().__init__()
        self._root = root
        self._training_cost = float("nan")
        self._leaves: List[_Node] = []
        self._summary = None
        if root is not None:
            self._index()

    def _index(self):
        self._leaves = []

        def walk(nd):
            if not nd.children:
                self._leaves.append(nd)
            for ch in nd.children:
                walk(ch)
        walk(self._root)
        self._leaves.sort(key=lambda nd: nd.index)

    def clusterCenters(self) -> List[np.ndarray]:
        return [nd.center.copy() for nd in self._leaves]

    @property
    def numFeatures(self) -> int:
        return int(self._root.center.size)

    @property
    def trainingCost(self) -> float:
        return self._training_cost

    @property
    def hasSummary(self) -> bool:
        return self._summary is not None

    @property
    def summary(self) -> BisectingKMeansSummary:
        if self._summary is None:
            raise RuntimeError("No training summary available for this BisectingKMeansModel")
        return self._summary

    @property
    def _cosine(self) -> bool:
        return self.getDistanceMeasure() == "cosine"

    def _predict_tensor(self, x: torch.Tensor) -> torch.Tensor:
        out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
        step = max(1, _CHUNK // max(int(x.shape[1]), 1))
        cosine = self._cosine

        def walk(nd, rows, xs):
            if rows.numel() == 0:
                return
            if not nd.children:
                out[rows] = nd.index
                return
            cs = torch.as_tensor(np.stack([ch.center for ch in nd.children]), device=x.device)
            if cosine:  # xs has unit rows: 1 - x.c / |x| against the unit-length children, the first on ties
                go = torch.argmin(1.0 - xs @ cs.T, 1)
            else:
                go = torch.argmin(((xs[:, None, :] - cs[None]) ** 2).sum(-1), 1)
            for h, ch in enumerate(nd.children):
                sel = go == h
                walk(ch, rows[sel], xs[sel])
        for r0 in range(0, int(x.shape[0]), step):
            xs = x[r0:r0 + step].to(torch.float64)
            if cosine:
                xs = xs / torch.linalg.norm(xs, dim=1, keepdim=True)
            walk(self._root, torch.arange(r0, r0 + xs.shape[0], device=x.device), xs)
        return out

    def predict(self, value) -> int:
        return int(self._predict_tensor(torch.as_tensor(as_array(value)).reshape(1, -1))[0])

    def computeCost(self, dataset) -> float:
        x = dataset._feature_matrix(self.getFeaturesCol())
        lab = self._predict_tensor(x)
        cs = torch.as_tensor(np.stack([nd.center for nd in self._leaves]), device=x.device)
        c = torch.zeros(1, dtype=torch.float64, device=x.device)
        step = max(1, _CHUNK // max(int(x.shape[1]), 1))
        for r0 in range(0, int(x.shape[0]), step):
            xs = x[r0:r0 + step].to(torch.float64)
            if self._cosine:  # sum of 1 - cos, not squared
                c += (1.0 - (xs * cs[lab[r0:r0 + step]]).sum(1) / torch.linalg.norm(xs, dim=1)).sum()
                continue
            c += ((xs - cs[lab[r0:r0 + step]]) ** 2).sum()
        dataset._comm.allreduce_(c)
        return float(c[0])

    def _transform(self, df):
        lab = self._predict_tensor(df._feature_matrix(self.getFeaturesCol())).to(torch.int32)
        return _replace_col(df, self.getPredictionCol(), ColumnData(lab, None, T.IntegerType()))

    def _nodes(self) -> List[_Node]:
        nodes = []

        def walk(nd):
            nodes.append(nd)
            for ch in nd.children:
                walk(ch)
        walk(self._root)
        return nodes

    def _save_impl(self, path):
        import pyarrow as pa
        U.write_metadata(self, path)
        data = os.path.join(path, "data")
        md = {"class": "org.apache.spark.mllib.clustering.BisectingKMeansModel", "version": "3.0",
              "rootId": int(self._root.index), "k": len(self._leaves),
              "distanceMeasure": self.getDistanceMeasure(), "trainingCost": self._training_cost}
        os.makedirs(os.path.join(data, "metadata"), exist_ok=True)
        with open(os.path.join(data, "metadata", "part-00000"), "w") as fh:
            fh.write(json.dumps(md, separators=(",", ":")) + "\n")
        open(os.path.join(data, "metadata", "_SUCCESS"), "w").close()
        rows = [{"index": int(nd.index), "size": int(round(nd.size)), "center": U.vector_struct(nd.center),
                 "norm": float(np.linalg.norm(nd.center)), "cost": float(nd.cost), "height": float(nd.height),
                 "children": [int(ch.index) for ch in nd.children]} for nd in self._nodes()]
        U.write_parquet(data, "data", pa.Table.from_pylist(rows, schema=pa.schema([
            pa.field("index", pa.int32(), nullable=False), pa.field("size", pa.int64(), nullable=False),
            ("center", U.vector_arrow_type()), pa.field("norm", pa.float64(), nullable=False),
            pa.field("cost", pa.float64(), nullable=False), pa.field("height", pa.float64(), nullable=False),
            ("children", pa.list_(pa.field("element", pa.int32(), nullable=False)))])))

    @classmethod
    def _load_impl(cls, path, md):
        data = os.path.join(path, "data")
        with open(os.path.join(data, "metadata", "part-00000")) as fh:
            dmd = json.loads(fh.readline())
        rows = {r["index"]: r for r in U.read_parquet(data, "data").to_pylist()}
        nodes = {i: _Node(U.vector_from_struct(r["center"]), float(r["size"]), r["cost"], int(i), r["height"])
                 for i, r in rows.items()}
        for i, r in rows.items():
            nodes[i].children = [nodes[ch] for ch in r["children"]]
        m = cls(nodes[int(dmd["rootId"])])
        m._training_cost = float(dmd.get("trainingCost", float("nan")))
        U.apply_params(m, md)
        return m
