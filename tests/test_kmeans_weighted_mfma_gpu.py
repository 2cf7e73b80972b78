"""Weighted KMeans on the bf16 / e4m3 MFMA path (``precision="bf16"`` with weights).

K10w (``kmeans_weighted.hip``) against the project's own correctly rounded sums (``sums_reference`` on the
materialised f64 products — the existing double-double kernel, not the code under test), bit for bit in ``S``
and ``S_lo``, through both front ends (the counting sort of a real assign, and the stable-sort convenience
form); the engine against the source-precision weighted engine, the unweighted bf16 engine (unit weights),
duplicated rows (integer weights) and dropped rows (zero weights), bit for bit on lattice data whose sums are
exact; the lazy cost against an f64 oracle; cosine against a torch f64 weighted spherical Lloyd; the public
API (conf, fit, transform, summary, save / load); two gloo ranks against one; and the refusals."""
import json
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import (LloydEngine, padded_dim,
                                                                                     to_device_matrix)
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import kmeans_ops as K

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
DEV = torch.device("cuda", 0)
KW = 37  # clusters of the kernel cases; 0, 5 and 36 stay empty


# ------------------------------------------------------------------------------------------ K10w alone

def _rows(dtype, n, d, seed, skew=False):
    """Device rows in the kernels' layout and their weights: uniform in [0, 4), every 17th exactly 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g) * (2.0 if dtype == FP8 else 3.0)
    if skew:  # > 90 % of the rows around one point: one cluster spans many wave slices
        m = (n * 93) // 100
        x[:m] = 6.0 + 0.25 * torch.randn(m, d, generator=g)
    x = torch.where(x.abs() < 2.0 ** -8, torch.zeros(()), x)  # (bounds the exponent span of the products)
    w = torch.rand(n, generator=g, dtype=torch.float64) * 4
    w[::17] = 0.0
    return to_device_matrix(x.to(dtype).to(DEV), d), w.to(DEV)


def _assign_sort(x, n, d, k, seed, skew=False):
    """A real K9 / K9r assign with the counting sort's hist / rank, then the sort-only front end."""
    dp, fp8 = x.shape[1], K.is_fp8(x)
    g = torch.Generator().manual_seed(seed + 1)
    first = (n * 93) // 100 if skew else 0  # (skew: centres from the rows outside the dense group ...)
    cent = x[torch.randint(first, n, (k,), generator=g).to(DEV), :d].to(torch.float32).to(torch.float64)
    cent += 0.01 * torch.randn(k, d, generator=g, dtype=torch.float64).to(DEV)
    if skew:
        cent[7] = 6.0  # (... and one at its middle)
    cent[[0, 5, k - 1]] = 200.0  # far from every row: these clusters stay empty
    cplan = K.plan_accum(n, dp, k, 0, force="sort", fp8=fp8)
    i32 = dict(dtype=torch.int32, device=DEV)
    xn = torch.empty(n, dtype=torch.float32, device=DEV)
    xn64 = torch.empty(n, dtype=torch.float64, device=DEV)
    K.row_pass(x, n, dp, xn, xn64=xn64)
    if fp8 and dp > 512:
        # the assign kernels stop at 512 e4m3 columns (K10w's CPL 16 path does not): labels from the f64
        # reference assign, and in place of the counting sort a grouping permutation that is NOT the stable
        # sort's (rows of a cluster in descending order)
        lab = K.assign_reference(x[:, :d].to(torch.float32), cent)[0].to(torch.int32)
        order = torch.argsort(lab.long() * n + (n - 1 - torch.arange(n, device=DEV)))
        seg = torch.zeros(k + 1, **i32)
        seg[1:] = torch.cumsum(torch.bincount(lab.long(), minlength=k), 0)
        return lab, order.to(torch.int32), seg, xn64, cplan, None
    aplan = K.plan_assign(n, dp, k, 0, fp8=fp8)
    cb = torch.zeros((aplan.kp, dp), dtype=torch.bfloat16, device=DEV)
    cn = torch.zeros(aplan.kp, dtype=torch.float32, device=DEV)
    K.update_centers(None, k, d, cent.contiguous(), cb, dp, aplan.kp, cn, None, snap=K.mx_applies(x))
    lab, rank, perm = (torch.zeros(n, **i32) for _ in range(3))
    hist = torch.zeros(aplan.grid * aplan.kp, **i32)
    off = torch.zeros(k * aplan.grid, **i32)
    seg = torch.zeros(K.seg_buffer_ints(k), **i32)
    best = torch.zeros(n, dtype=torch.float32, device=DEV)
    cost_part = torch.zeros(aplan.grid, dtype=torch.float64, device=DEV)
    K.assign_bf16(x, n, dp, cb, cn, aplan, lab, best, cost_part, hist, rank, xnorm=xn)
    tail = K.sort_perm(lab, rank, hist, aplan, n, k, off, seg, perm)
    return lab, perm, seg, xn64, cplan, tail


def _oracle(x, n, d, w, xn64, lab, k):
    x64 = x[:n, :d].to(torch.float32).to(torch.float64)
    cols = torch.cat([x64 * w[:, None], w[:, None], (w * xn64)[:, None]], 1)
    S, _, S_lo = K.sums_reference(cols, lab, k, with_lo=True)
    return S, S_lo


def _check_k10w(dtype, n, d, skew=False):
    x, w = _rows(dtype, n, d, seed=1000 * d + n, skew=skew)
    dp = x.shape[1]
    lab, perm, seg, xn64, cplan, tail = _assign_sort(x, n, d, KW, seed=n + d, skew=skew)
    cnt = torch.bincount(lab.long(), minlength=KW)
    assert int(cnt[0]) == 0 and int(cnt[5]) == 0 and int(cnt[KW - 1]) == 0
    assert (tail is None or torch.equal(tail[:KW], cnt.to(torch.float64))) and int(seg[KW]) == n
    assert torch.equal(torch.sort(perm.long()).values, torch.arange(n, device=DEV))
    assert bool((lab[perm.long()][1:] >= lab[perm.long()][:-1]).all())
    R, R_lo = _oracle(x, n, d, w, xn64, lab, KW)
    S, S_lo = K.weighted_sums(x, n, dp, d, w, xn64, KW, perm, seg, cplan)
    T, T_lo = K.weighted_sums_labels(x, n, dp, d, w, xn64, lab, KW)
    assert S.shape == (KW, d + 2)
    assert torch.equal(S, R) and torch.equal(S_lo, R_lo)
    assert torch.equal(T, R) and torch.equal(T_lo, R_lo)
    assert not S[[0, 5, KW - 1]].any() and not S_lo[[0, 5, KW - 1]].any()
    return cnt


# (dtype, d): bf16 Dp 32 / 128 / 256 / 512 (CPL 2 / 2 / 4 / 8; Dp 32 leaves lanes inactive) and d = 250 < Dp 256;
# e4m3 Dp 256 / 512 / 1024 (CPL 4 / 8 / 16) and d = 200 < Dp 256
_SHAPES = [(torch.bfloat16, 32), (torch.bfloat16, 128), (torch.bfloat16, 256), (torch.bfloat16, 512),
           (torch.bfloat16, 250), (FP8, 256), (FP8, 512), (FP8, 1024), (FP8, 200)]


@pytest.mark.parametrize("n", [1, 130, 4099])
@pytest.mark.parametrize("dtype,d", _SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_k10w_equals_the_correctly_rounded_sums(dtype, d, n):
    _check_k10w(dtype, n, d)


@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 128), (FP8, 256)], ids=lambda v: str(v).replace("torch.", ""))
def test_k10w_one_cluster_over_many_slices(dtype, d):
    cnt = _check_k10w(dtype, 4099, d, skew=True)
    assert int(cnt.max()) > 0.9 * 4099


# ------------------------------------------------------------------------------------------ engine

def _lattice(n, d, k, seed, fp8=False):
    """Blobs on a lattice: centres on a grid spaced 8 apart, offsets within ±1 in multiples of 1/8 (integers
    for e4m3) — every coordinate is exact in the storage dtype and every sum of them exact in f64; blobs are
    at least 8 apart in (nearly) every coordinate, so no label is near a tie. Returns (rows f32 [n, d], blob of
    every row, one row per blob for set_centers)."""
    g = torch.Generator().manual_seed(seed)
    span = 1 if fp8 else 2
    cen = 8.0 * torch.randint(-span, span + 1, (k, d), generator=g).float()
    blob = torch.randint(0, k, (n,), generator=g)
    blob[:k] = torch.arange(k)
    offs = (torch.randint(-1, 2, (n, d), generator=g).float() if fp8
            else torch.randint(-8, 9, (n, d), generator=g).float() / 8.0)
    x = cen[blob] + offs
    dt = FP8 if fp8 else torch.bfloat16
    assert torch.equal(x.to(dt).float(), x)
    return x, blob, x[:k].clone()


def _engine(x, d, k, init, steps, **kw):
    eng = LloydEngine(x, d, k, **kw)
    eng.set_centers(init.double().numpy())
    for _ in range(steps):
        eng.step()
    return eng


def _weights(n, seed, lo=0.25):
    g = torch.Generator().manual_seed(seed)
    return (lo + 3.0 * torch.rand(n, generator=g, dtype=torch.float64)).to(DEV)


@pytest.mark.parametrize("fp8,d", [(False, 24), (True, 256)], ids=["bf16-24", "e4m3-256"])
def test_engine_equals_source_precision_engine(fp8, d):
    n, k = 5000, 6
    x, blob, init = _lattice(n, d, k, seed=3, fp8=fp8)
    w = _weights(n, 7)
    assert float(torch.zeros(k, dtype=torch.float64, device=DEV).index_add_(0, blob.to(DEV), w).min()) >= 1.0
    xd = x.to(FP8 if fp8 else torch.bfloat16).to(DEV)
    a = _engine(xd, d, k, init, 5, weights=w, precision="bf16")
    b = _engine(xd.float(), d, k, init, 5, weights=w)
    assert a.gpu and a.precision == "bf16" and a._wx is None and a.x.dtype == xd.dtype
    assert b.precision == "exact"
    assert np.array_equal(a.centers.cpu().numpy(), b.centers.cpu().numpy())
    assert torch.equal(a.labels[:n].long().cpu(), blob)


def test_unit_weights_equal_unweighted_bf16_fit():
    n, d, k = 5000, 24, 6
    x, _, init = _lattice(n, d, k, seed=4)
    xd = x.to(torch.bfloat16).to(DEV)
    a = _engine(xd, d, k, init, 5, weights=torch.ones(n, dtype=torch.float64, device=DEV), precision="bf16")
    b = _engine(xd, d, k, init, 5, precision="bf16")
    assert np.array_equal(a.centers.cpu().numpy(), b.centers.cpu().numpy())
    assert a.cluster_sizes() == b.cluster_sizes()


def test_integer_weights_equal_duplicated_rows():
    n, d, k = 3000, 24, 5
    x, _, init = _lattice(n, d, k, seed=5)
    reps = torch.randint(1, 4, (n,), generator=torch.Generator().manual_seed(6))
    xd = x.to(torch.bfloat16).to(DEV)
    a = _engine(xd, d, k, init, 4, weights=reps.double().to(DEV), precision="bf16")
    b = _engine(torch.repeat_interleave(xd, reps.to(DEV), 0), d, k, init, 4, precision="bf16")
    assert np.array_equal(a.centers.cpu().numpy(), b.centers.cpu().numpy())


def test_zero_weights_equal_dropped_rows():
    n, d, k = 3000, 24, 5
    x, _, init = _lattice(n, d, k, seed=8)
    w = _weights(n, 9)
    keep = torch.rand(n, generator=torch.Generator().manual_seed(10)) < 0.7
    keep[:k] = True
    w = torch.where(keep.to(DEV), w, torch.zeros((), dtype=torch.float64, device=DEV))
    xd = x.to(torch.bfloat16).to(DEV)
    a = _engine(xd, d, k, init, 4, weights=w, precision="bf16")
    b = _engine(xd[keep.to(DEV)].contiguous(), d, k, init, 4, weights=w[keep.to(DEV)].contiguous(), precision="bf16")
    assert np.array_equal(a.centers.cpu().numpy(), b.centers.cpu().numpy())
    assert a.training_cost() == b.training_cost()


def _cost_oracle(x64, w, lab, cb64):
    """(Σ w_i |x_i - c_label|² in f64, the tolerance (d + 8)·2^-52·Σ w_i (|x_i| + max_j |c_j|)²): every term of
    the expanded form Σ_j (Q_j - 2 c_j·S_j + W_j |c_j|²) is an f64 quantity with at most d + O(1) roundings and
    a magnitude bounded by that sum."""
    d = x64.shape[1]
    want = float((w * ((x64 - cb64[lab]) ** 2).sum(1)).sum())
    cmax = float(cb64.norm(dim=1).max())
    tol = (d + 8) * 2.0 ** -52 * float((w * (x64.norm(dim=1) + cmax) ** 2).sum())
    return want, tol


@pytest.mark.parametrize("fp8,d", [(False, 24), (True, 256)], ids=["bf16-24", "e4m3-256"])
def test_training_cost_from_the_sums(fp8, d):
    n, k = 4000, 6
    g = torch.Generator().manual_seed(11)
    cen = torch.randn(k, d, generator=g) * 3
    x = (cen[torch.randint(0, k, (n,), generator=g)] + 0.5 * torch.randn(n, d, generator=g)).to(
        FP8 if fp8 else torch.bfloat16).to(DEV)
    w = _weights(n, 12, lo=0.0)
    eng = LloydEngine(x, d, k, weights=w, precision="bf16")
    eng.set_centers((cen + 0.1).double().numpy())
    cb64 = eng.cb[:k, :d].to(torch.float64).clone()  # the bf16 centres the step's assignment compares with
    eng.step()
    got = eng.training_cost()
    want, tol = _cost_oracle(x[:, :d].float().double(), w, eng.labels[:n].long(), cb64)
    print(f"cost {got!r} oracle {want!r} |diff| {abs(got - want):.3e} tol {tol:.3e}")
    assert want > 0 and abs(got - want) <= tol


def test_cosine_with_weights():
    n, d, k = 2000, 48, 5
    g = torch.Generator().manual_seed(13)
    dirs = torch.zeros(k, d)
    for j in range(k):  # separated directions: disjoint blocks of coordinates
        dirs[j, 8 * j: 8 * j + 8] = 1.0 + torch.rand(8, generator=g)
    x = (dirs[torch.randint(0, k, (n,), generator=g)] * (1.0 + torch.rand(n, 1, generator=g))
         + 0.05 * torch.randn(n, d, generator=g)).to(torch.bfloat16).to(DEV)
    w = _weights(n, 14, lo=0.0)
    eng = LloydEngine(x, d, k, weights=w, precision="bf16", spherical=True)
    init = dirs / dirs.norm(dim=1, keepdim=True)
    eng.set_centers(init.double().numpy())
    xu = eng.x[:, :d].to(torch.float64)  # the engine's bf16 unit rows
    c = init.double().to(DEV)
    for _ in range(4):
        cb64 = eng.cb[:k, :d].to(torch.float64).clone()
        eng.step()
        lab = (xu @ c.T).argmax(1)
        s = torch.zeros(k, d, dtype=torch.float64, device=DEV).index_add_(0, lab, xu * w[:, None])
        c = s / s.norm(dim=1, keepdim=True)
        assert torch.equal(eng.labels[:n].long(), lab)
    np.testing.assert_allclose(eng.centers.cpu().numpy(), c.cpu().numpy(), rtol=1e-12, atol=0)
    # the cosine cost: Σ w (1 - cos) = Σ w |x - c|² / 2 on unit vectors, against the last step's bf16 centres
    want, tol = _cost_oracle(xu, w, lab, cb64)
    assert abs(eng.training_cost() - want / 2.0) <= tol / 2.0


# ------------------------------------------------------------------------------------------ public API

def _api_data(n=5000, d=24, k=6):
    x, blob, _ = _lattice(n, d, k, seed=21)
    return x, blob, _weights(n, 22).cpu()


def _api_fit(spark, x, w, k, lo=0, hi=None):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import KMeans
    hi = x.shape[0] if hi is None else hi
    df = spark.createDataFrameFromTensors({"features": x[lo:hi].to(torch.bfloat16).to(spark._device),
                                           "w": w[lo:hi].to(spark._device)})
    return df, KMeans(k=k, seed=5, weightCol="w", tol=0.0, maxIter=50).fit(df)


def test_public_api_weighted_bf16_fit(tmp_path):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import KMeansModel
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    n, d, k = 5000, 24, 6
    x, _, w = _api_data(n, d, k)
    spark.conf.set("cml.ml.kmeans.precision", "bf16")
    try:
        df, m = _api_fit(spark, x, w, k)  # (a) does not raise
        assert m.summary.numIter < 50  # (b)
        L = m.transform(df)._numeric("prediction").long()
        x64, wd = x.double().to(DEV), w.to(DEV)
        S, _ = K.sums_reference(torch.cat([x64 * wd[:, None], wd[:, None]], 1), L, k)
        got = np.array(m.clusterCenters())
        assert float(S[:, d].min()) > 0
        Sh = S.cpu().numpy()
        assert np.array_equal(got, Sh[:, :d] / Sh[:, d:d + 1])  # (c): fl(fl(Σ w·x) / fl(Σ w))
        assert m.summary.clusterSizes == torch.bincount(L, minlength=k).tolist()  # (d)
        cb64 = torch.as_tensor(got, device=DEV).to(torch.bfloat16).to(torch.float64)
        want, tol = _cost_oracle(x64, wd, L, cb64)
        print(f"trainingCost {m.summary.trainingCost!r} oracle {want!r} tol {tol:.3e}")
        assert abs(m.summary.trainingCost - want) <= tol  # (e)
        p = str(tmp_path / "wkm")
        m.write().overwrite().save(p)
        assert np.array_equal(np.array(KMeansModel.load(p).clusterCenters()), got)  # (f)
    finally:
        spark.conf.unset("cml.ml.kmeans.precision")


# ------------------------------------------------------------------------------------------ two gloo ranks

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, out_path):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": "0",
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "CML_COMM_BACKEND": "gloo"})
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    spark.conf.set("cml.ml.kmeans.precision", "bf16")
    x, _, w = _api_data()
    n = x.shape[0]
    _, m = _api_fit(spark, x, w, 6, rank * n // world, (rank + 1) * n // world)
    res = {"centers": [[v.hex() for v in c.tolist()] for c in m.clusterCenters()],
           "cost": float(m.summary.trainingCost).hex(), "iters": int(m.summary.numIter),
           "sizes": m.summary.clusterSizes}
    spark._comm.barrier()
    if rank == 0:
        with open(out_path, "w") as fh:
            json.dump(res, fh)
    spark.stop()


def _run_world(world, tmp_path, limit=240.0):
    out = str(tmp_path / f"wmfma_w{world}.json")
    ctx = mp.start_processes(_rank_main, args=(world, _free_port(), out), nprocs=world, join=False,
                             start_method="spawn")
    t0 = time.monotonic()
    while not ctx.join(timeout=2.0):  # (raises when a child failed)
        if time.monotonic() - t0 > limit:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"world {world}: a rank did not finish within {limit:.0f} s")
    with open(out) as fh:
        return json.load(fh)


def test_two_gloo_ranks_equal_one_rank(tmp_path):
    r1, r2 = _run_world(1, tmp_path), _run_world(2, tmp_path)
    assert r2["centers"] == r1["centers"]
    assert r2["cost"] == r1["cost"]
    assert r2["sizes"] == r1["sizes"] and r2["iters"] == r1["iters"] < 50


# ------------------------------------------------------------------------------------------ refusals

def test_refusals():
    w = torch.ones(64, dtype=torch.float64, device=DEV)
    wide = torch.zeros((64, 600), dtype=torch.bfloat16, device=DEV)  # padded width 1024 > 512
    assert padded_dim(600) > 512
    with pytest.raises(ValueError, match="512"):
        LloydEngine(wide, 600, 2, weights=w, precision="bf16")
    host = torch.zeros((64, 16), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="unweighted"):
        LloydEngine(host, 16, 2, weights=w.cpu(), precision="bf16", device=DEV)
