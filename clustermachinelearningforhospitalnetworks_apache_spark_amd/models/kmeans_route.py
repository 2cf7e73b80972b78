"""Which path a LloydEngine takes: everything its constructor decides before it prepares rows or allocates,
as one pure function of flags and dtypes (tests/test_kmeans_route.py pins the whole table)."""
from __future__ import annotations

import dataclasses
from typing import Callable, Mapping, Optional

import torch

_SOURCE = (torch.float32, torch.float64)


@dataclasses.dataclass(frozen=True)
class Route:
    precision: str  # "bf16" (MFMA path), "exact" (f64 reference algorithm) or "screen" (exact, MFMA-screened)
    prune: bool  # exact bound-pruned steps (device form or torch form: decided from the plans in _alloc_gpu)
    incremental: bool
    use_graph: bool
    row_chunks: Optional[int]  # None: the constructor's default (by rank count and rows)
    accum_mode: Optional[str]
    refresh_interval: int
    wfast: bool  # weighted fit on the MFMA path (_step_weighted)
    screen: bool
    gpu: bool  # the MFMA kernels run (bf16 path on device or streamed rows)
    to_f32: bool  # weighted bf16 / fp8 device rows are first widened to f32 (source-precision path)


def resolve_route(*, on_device: bool, dtype: torch.dtype, streamed: bool, weighted: bool, spherical: bool,
                  precision: Optional[str], prune: Optional[bool], incremental: Optional[bool],
                  use_graph: Optional[bool], row_chunks: Optional[int], accum_mode: Optional[str],
                  refresh_interval: Optional[int], screen_ok: bool, dd_exact: Callable[[], bool],
                  env: Mapping[str, str]) -> Route:
    """The decisions, in the order in which each overrides the earlier ones: streamed, weights, precision,
    screen, prune, graph. ``screen_ok``: unweighted euclidean f32/f64 device rows with a K9r plan at this width.
    ``dd_exact()`` (dd_sums_exact: a collective) is called at most once, and only for "auto" precision on f64
    device rows with ``screen_ok`` and CML_KMEANS_SCREEN not "0"."""
    # out-of-core rows: full unpruned steps on the MFMA path, one chunk per stream buffer
    if streamed:
        if weighted or spherical:
            raise ValueError("streamed (out-of-core) KMeans supports unweighted euclidean fits")
        precision, prune, incremental, use_graph = "bf16", False, False, False
    # full re-accumulation of the incremental sums every refresh_interval steps (0 = never: the sum
    # grid of _sum_grid already keeps incremental == full bit for bit; conf
    # cml.ml.kmeans.refreshInterval / env CML_KMEANS_REFRESH turn on the belt-and-braces refresh)
    if refresh_interval is None:
        refresh_interval = int(env.get("CML_KMEANS_REFRESH", "0") or 0)
    # weights (Spark's weightCol, KMeans.scala runAlgorithm): centre = Σ w·x / Σ w, cost = Σ w·d²,
    # k-means|| candidates weighted by the summed weight of their rows. Weighted fits run the
    # source-precision path (f64 rows, deterministic f64 sums of [w·x | w]) unless precision "bf16" is
    # asked for (argument, conf cml.ml.kmeans.precision, env CML_KMEANS_PRECISION): device rows then
    # stay bf16 / e4m3 on the MFMA path (_step_weighted: K9 / K9r assign, the counting sort, the
    # double-double weighted sums of K10w — the same correctly rounded Σ fl64(w·x) the source-precision
    # path forms, with no f64 copy of X). "auto" keeps the source-precision routing; host rows with
    # "bf16" take the host path, as an unweighted "bf16" request on host rows does.
    wfast = to_f32 = False
    if weighted:
        req = str(precision or env.get("CML_KMEANS_PRECISION") or "auto").lower()
        if req == "bf16" and on_device:
            wfast = True
            precision, prune, incremental, use_graph = "bf16", False, False, False
            row_chunks, accum_mode = 1, "sort"
        else:
            precision, prune = "exact", False
            if on_device and dtype not in _SOURCE:
                to_f32, dtype = True, torch.float32
    # precision (cml.ml.kmeans.precision): "bf16" = the MFMA path (bf16 rows in the distance GEMM,
    # exact f64 sums of those rows); "exact" = the f64 reference algorithm on the rows as given
    # (kmeans_exact.hip on the GPU); "auto" = exact for f32/f64 device rows — the reference's f64
    # feature vectors (ref.py:134-136) are not silently rounded to 8 mantissa bits — and the MFMA
    # path for bf16 / fp8 rows; "screen" = the exact algorithm's results bit for bit, with the
    # assignments screened on MFMA (_screen_labels: a bf16 K9r pass with top-2 bounds, a certificate
    # covering the bf16 rounding of rows and centres, an f64 re-assignment of the uncertified rows) —
    # what "auto" picks for wide f32/f64 device rows where K9r applies (CML_KMEANS_SCREEN=0: exact).
    precision = (precision or env.get("CML_KMEANS_PRECISION") or "auto").lower()
    if precision not in ("auto", "bf16", "exact", "screen"):
        raise ValueError(f"KMeans precision must be 'auto', 'bf16', 'exact' or 'screen', got {precision!r}")
    if precision == "auto":
        precision = "exact" if (not on_device or dtype in _SOURCE) else "bf16"
        if precision == "exact" and screen_ok and env.get("CML_KMEANS_SCREEN", "1") != "0":
            # the screen's incremental double-double sums equal the exact path's only while every
            # coordinate sum fits 106 bits: f32 rows always; f64 rows when their exponent span allows
            #  — otherwise the plain exact kernels
            if dtype != torch.float64 or dd_exact():
                precision = "screen"
    if streamed:
        precision = "bf16"
    if precision in ("exact", "screen") and on_device and dtype not in _SOURCE:
        raise ValueError(f"precision {precision!r} needs f32/f64 rows, got {dtype}")
    if precision == "screen" and not screen_ok:
        precision = "exact"  # (weights, cosine, or no K9r plan at this width: the plain exact kernels)
    if on_device and precision in ("exact", "screen"):
        prune = False  # the reference algorithm (the torch bounds form would need host syncs anyway)
    if prune is None:  # default on GPU rows: exact pruned steps (CML_KMEANS_PRUNE=0 turns them off)
        knob = env.get("CML_KMEANS_PRUNE")
        prune = (knob != "0") if knob is not None else on_device
    if prune:  # one row chunk; the device form keeps incremental sums, the torch form its own
        row_chunks = 1
    # One Lloyd step = ~8-15 kernel launches; with use_graph it is replayed as a captured HIP graph
    # (single rank: one graph; multi-rank: the device pruned step as two graphs around its
    # all-reduce, the RCCL call eager between the replays; the chunked full step stays eager).
    # Measured on MI355X (profiles/r3/graph_ab/): the pruned step has no host synchronisation, so eager
    # launches run ahead of the GPU and a 20-step fit is as fast eagerly (100.9 vs 102.6 ms at 100M
    # rows, 19.6 vs 20.9 ms at the 8-GPU shard of 12.5M) — the capture costs more than the replays
    # save. Default eager; CML_KMEANS_GRAPH=1 (or use_graph=True) captures.
    if use_graph is None:
        use_graph = env.get("CML_KMEANS_GRAPH") == "1"
    return Route(precision=precision, prune=bool(prune), incremental=True if incremental is None else bool(incremental),
                 use_graph=bool(use_graph), row_chunks=row_chunks, accum_mode=accum_mode,
                 refresh_interval=max(0, int(refresh_interval)), wfast=wfast, screen=precision == "screen",
                 gpu=(on_device or streamed) and precision == "bf16", to_f32=to_f32)
