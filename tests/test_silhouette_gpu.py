"""K26 (``_native/csrc/silhouette.hip``) and the ClusteringEvaluator paths on the GPU.

The kernels are checked against a dense f64 oracle written here from the definition, on the f64 values of
the same rows and labels, with the derived error model of the kernel's header (u = 2^-24, 3·dp exact
products accumulated in f32):

    squaredEuclidean  E_i = u·[(6·dp + 12)·|x_i|·max_c|ν_c| + (dp + 6)·r_i + 4·max_c|κ_c|]
    cosine            E_i = u·(6·dp + 16)

    |own − own_ref| <= E_i, |b − b_ref| <= E_i, nb == nb_ref where best and second best differ by > 2·E_i,
    |s − s(own, b)| <= 1e-6 (the epilogue, recomputed in f64 from the kernel's own outputs),
    |silhouette − ref| <= Σ w·((W/(W−w) + 1)·E/max(a_ref, b_ref) + 1e-6) / Σ w, which must be < 2e-3.
"""
import functools

import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import silhouette_ops as SO

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _data(n, d, k, fp8, scale, offset, seed=5):
    """Blobs (tests/test_kmeans_api_gpu.py:_blobs) in the kernels' layout, labels 90 % true / 10 % random
    (both branches of s occur), integer weights in {0, 1, 2, 3}."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    g = torch.Generator(device=DEV).manual_seed(seed)
    cen = torch.randn(k, d, generator=g, device=DEV) * scale
    true = torch.randint(0, k, (n,), generator=g, device=DEV)
    x = cen[true] + torch.randn(n, d, generator=g, device=DEV) + offset
    x = x.to(torch.float8_e4m3fn if fp8 else torch.bfloat16)
    rnd = torch.randint(0, k, (n,), generator=g, device=DEV)
    lab = torch.where(torch.rand(n, generator=g, device=DEV) < 0.9, true, rnd).to(torch.int32)
    w = torch.randint(0, 4, (n,), generator=g, device=DEV).to(torch.float64)
    return to_device_matrix(x, d), lab, w


def _x64(xd, d):
    return xd[:, :d].to(torch.float32).to(torch.float64)


def _stats(x64, lab, K, w, cosine):
    """[S | W | Q] by the f64 index_add_ oracle."""
    n, d = x64.shape
    w = torch.ones(n, dtype=torch.float64, device=DEV) if w is None else w
    g = lab.long()
    xx = (x64 * x64).sum(1)
    v = x64 / xx.sqrt()[:, None] if cosine else x64
    S = torch.zeros(K, d, dtype=torch.float64, device=DEV).index_add_(0, g, v * w[:, None])
    W = torch.zeros(K, dtype=torch.float64, device=DEV).index_add_(0, g, w)
    Q = torch.zeros(K, dtype=torch.float64, device=DEV).index_add_(0, g, torch.zeros_like(xx) if cosine else w * xx)
    return S, W, Q


def _oracle(x64, lab, K, w, cosine, dpk):
    """Dense f64 oracle: own, b, nb, second best, s, a, E per row and the silhouette."""
    n, d = x64.shape
    w = torch.ones(n, dtype=torch.float64, device=DEV) if w is None else w
    g = lab.long()
    S, W, Q = _stats(x64, lab, K, w, cosine)
    live = W > 0
    Ws = torch.where(live, W, torch.ones_like(W))
    mu = S / Ws[:, None]
    xx = (x64 * x64).sum(1)
    if cosine:
        D = 1.0 - (x64 @ mu.T) / xx.sqrt()[:, None]
        E = torch.full((n,), U * (6 * dpk + 16), dtype=torch.float64, device=DEV)
    else:
        q = Q / Ws
        D = xx[:, None] - 2.0 * (x64 @ mu.T) + q[None, :]
        m = S.sum(0) / W.sum()
        nu = (mu - m)[live]
        kap = (q - 2.0 * (mu @ m) + m @ m + 2.0 * ((mu - m) @ m))[live]
        r = ((x64 - m) ** 2).sum(1)
        E = U * ((6 * dpk + 12) * xx.sqrt() * nu.norm(dim=1).max() + (dpk + 6) * r + 4 * kap.abs().max())
    D[:, ~live] = float("inf")
    own = D.gather(1, g[:, None]).squeeze(1)
    D.scatter_(1, g[:, None], float("inf"))
    two = D.topk(min(2, K), dim=1, largest=False)
    b, nb = two.values[:, 0], two.indices[:, 0]
    second = two.values[:, 1] if K > 2 else torch.full_like(b, float("inf"))
    Wl = W[g]
    single = Wl == w
    a = own * Wl / torch.where(single, torch.ones_like(Wl), Wl - w)
    s = torch.where(a < b, 1 - a / b, torch.where(a > b, b / a - 1, torch.zeros_like(a)))
    s = torch.where(single, torch.zeros_like(s), s)
    sil = float((w * s).sum() / w.sum())
    amp = torch.where(single, torch.zeros_like(Wl), (Wl / torch.where(single, torch.ones_like(Wl), Wl - w) + 1.0)
                      * E / torch.maximum(a, b))
    bound = float((w * torch.where(single, torch.zeros_like(amp), amp + 1e-6)).sum() / w.sum())
    return dict(own=own, b=b, nb=nb, second=second, s=s, a=a, E=E, sil=sil, bound=bound, W=W, single=single,
                stats=torch.cat([S, W[:, None], Q[:, None]], 1))


def _host_s(own, b, Wl, w):
    single = Wl == w
    a = own * Wl / torch.where(single, torch.ones_like(Wl), Wl - w)
    s = torch.where(a < b, 1 - a / b, torch.where(a > b, b / a - 1, torch.zeros_like(a)))
    return torch.where(single, torch.zeros_like(s), s)


# ------------------------------------------------------------------------------------------------ label_wsum
WSUM = [(5, 20, 2, False), (4099, 128, 17, False), (70001, 256, 257, False), (30000, 512, 100, True)]


@pytest.mark.parametrize("n,d,K,fp8", WSUM)
@pytest.mark.parametrize("factor", ["none", "weights", "cosine"])
def test_label_wsum(n, d, K, fp8, factor):
    xd, lab, w = _data(n, d, K, fp8, 3.0, 0.0)
    x64 = _x64(xd, xd.shape[1])
    omega = {"none": None, "weights": w, "cosine": w / x64.norm(dim=1)}[factor]
    got = SO.label_wsum(xd, lab, K, omega)
    om = torch.ones(n, dtype=torch.float64, device=DEV) if omega is None else omega
    ref = torch.zeros(K, xd.shape[1], dtype=torch.float64, device=DEV).index_add_(0, lab.long(), x64 * om[:, None])
    mag = torch.zeros_like(ref).index_add_(0, lab.long(), (x64 * om[:, None]).abs())
    err = (got - ref).abs()
    print(f"label_wsum n={n} d={d} K={K} {factor}: max err / (1e-12 Σ|ωx|) = "
          f"{float((err / (1e-12 * mag).clamp(min=1e-300)).max()):.3g}")
    assert bool((err <= 1e-12 * mag).all())
    assert torch.equal(got, SO.label_wsum(xd, lab, K, omega))  # same bits
    assert got.shape == (K, xd.shape[1]) and bool((got[:, d:] == 0).all())


def test_label_wsum_empty():
    xd, lab, w = _data(4099, 128, 17, False, 3.0, 0.0)
    got = SO.label_wsum(xd, lab, 19, w)  # ids 17, 18 unused
    assert bool((got[17:] == 0).all()) and bool((got[:17] != 0).any())
    lab2 = torch.where(lab == 3, torch.full_like(lab, 4), lab)  # an empty cluster in the middle
    got2 = SO.label_wsum(xd, lab2, 17, None)
    assert bool((got2[3] == 0).all())
    ref = torch.zeros(17, 128, dtype=torch.float64, device=DEV).index_add_(0, lab2.long(), _x64(xd, 128))
    assert torch.allclose(got2, ref, rtol=1e-12, atol=1e-9)
    z = SO.label_wsum(xd[:0], lab[:0], 17, None)
    assert z.shape == (17, 128) and bool((z == 0).all())


# ------------------------------------------------------------------------------------------ silhouette_score
#        n      d    K   fp8   scale offset
SCORE = [(5, 20, 2, False, 3.0, 0.0),       # dp = 32
         (4099, 128, 3, False, 3.0, 0.0),
         (4099, 128, 17, False, 3.0, 5.0),  # one past a 16-centre tile
         (70001, 256, 64, False, 12.0, 20.0),  # cosine at +20 needs the wide blobs for the 2e-3 condition
         (20000, 512, 100, False, 2.0, 0.0),
         (20000, 256, 257, False, 3.0, 0.0),
         (20000, 256, 64, True, 3.0, 0.0),
         (20000, 512, 64, True, 3.0, 0.0)]


def _check_score(xd, d, lab, K, w, cosine, tag):
    dpk = max(32, xd.shape[1])
    o = _oracle(_x64(xd, d), lab, K, w, cosine, dpk)
    stats = torch.zeros(K, xd.shape[1] + 2, dtype=torch.float64, device=DEV)
    stats[:, :d] = o["stats"][:, :d]
    stats[:, xd.shape[1]:] = o["stats"][:, d:]
    part, own, b, nb, s = SO.silhouette_score(xd, lab, stats, w, cosine, rows=True)
    ww = torch.ones(len(lab), dtype=torch.float64, device=DEV) if w is None else w
    E = o["E"]
    fin = torch.isfinite(o["b"])
    fo = torch.isfinite(o["own"])  # own is +inf on a weight-0 row whose cluster holds no weight
    e_own = ((own.double() - o["own"]).abs()[fo] / E[fo]).max()
    e_b = ((b.double() - o["b"]).abs()[fin] / E[fin]).max() if bool(fin.any()) else 0.0
    sure = (o["second"] - o["b"]) > 2 * E
    s_host = _host_s(own.double(), b.double(), o["W"][lab.long()], ww)
    e_s = (s.double() - s_host).abs().max()
    sil = float(part[0] / part[1])
    print(f"{tag}: |own-ref|/E={float(e_own):.3f} |b-ref|/E={float(e_b):.3f} |s-s(own,b)|={float(e_s):.2e} "
          f"|sil-ref|={abs(sil - o['sil']):.3e} bound={o['bound']:.3e} sil={sil:.6f} "
          f"s<0: {float((o['s'] < 0).double().mean()):.3f}")
    assert o["bound"] < 2e-3  # the last assertion below cannot pass vacuously
    assert float(e_own) <= 1.0 and float(e_b) <= 1.0
    assert bool((b[~fin] == float("inf")).all()) and bool((nb[~fin] == -1).all())
    assert bool((own[~fo] == float("inf")).all())
    assert bool((nb.long()[sure] == o["nb"][sure]).all())
    assert float(e_s) <= 1e-6
    assert abs(float(part[1]) - float(ww.sum())) <= 1e-9 * max(1.0, float(ww.sum()))
    assert abs(sil - o["sil"]) <= o["bound"]
    # the reference form agrees with the dense oracle
    ref = SO.silhouette_reference(_x64(xd, d), lab, K, w, cosine, stats=o["stats"])
    assert abs(float(ref[0] / ref[1]) - o["sil"]) <= 1e-9
    return o


@pytest.mark.parametrize("n,d,K,fp8,scale,offset", SCORE)
@pytest.mark.parametrize("cosine", [False, True], ids=["sqeuclid", "cosine"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_silhouette_score(n, d, K, fp8, scale, offset, cosine, weighted):
    xd, lab, w = _data(n, d, K, fp8, scale, offset)
    o = _check_score(xd, d, lab, K, w if weighted else None, cosine, f"n={n} d={d} K={K} fp8={fp8}")
    if n > 1000:
        assert bool((o["s"] < 0).any()) and bool((o["s"] > 0).any())  # both branches of s


@pytest.mark.parametrize("cosine", [False, True], ids=["sqeuclid", "cosine"])
def test_silhouette_score_dead_and_singleton(cosine):
    xd, lab, w = _data(4099, 128, 17, False, 3.0, 5.0)
    lab = lab.clone()
    w = w.clone()
    lab[7] = 18  # a singleton cluster; id 17 stays unused (dead)
    w[7] = 2.0
    o = _check_score(xd, 128, lab, 19, w, cosine, "dead + singleton")
    assert float(o["s"][7]) == 0.0 and float(o["W"][17]) == 0.0
    o = _check_score(xd, 128, lab, 19, None, cosine, "dead + singleton, unit weights")
    assert bool((o["nb"] != 17).all())


def test_silhouette_score_empty():
    xd, lab, w = _data(4099, 128, 3, False, 3.0, 0.0)
    stats = torch.cat([SO.cluster_stats_device(xd, lab, 3, None, False)[0]])
    part = SO.silhouette_score(xd[:0], lab[:0], stats, None, False)
    assert part.tolist() == [0.0, 0.0]
    st0, zero = SO.cluster_stats_device(xd[:0], lab[:0], 3, None, True)
    assert bool((st0 == 0).all()) and not bool(zero)


def test_cluster_stats_device_matches_reference():
    xd, lab, w = _data(4099, 128, 17, False, 3.0, 5.0)
    for cosine in (False, True):
        got, zero = SO.cluster_stats_device(xd, lab, 17, w, cosine)
        ref = SO.cluster_stats_reference(_x64(xd, 128), lab, 17, w, cosine)
        assert not bool(zero)
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-9)
    xz = xd.clone()
    xz[5] = 0
    assert bool(SO.cluster_stats_device(xz, lab, 17, None, True)[1])


# --------------------------------------------------------------------------------------------------- public API
@pytest.fixture(scope="module")
def spark():
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    return SparkSession.builder.master("mi355x").getOrCreate()


@pytest.fixture(scope="module")
def api_frame(spark):
    n, d, k = 250_000, 256, 32
    g = torch.Generator(device=DEV).manual_seed(21)
    cen = torch.randn(k, d, generator=g, device=DEV) * 2.0
    x = (cen[torch.randint(0, k, (n,), generator=g, device=DEV)] + torch.randn(n, d, generator=g, device=DEV))
    x = x.to(torch.bfloat16)
    w = torch.randint(0, 4, (n,), generator=g, device=DEV).to(torch.float64)
    return x, w, spark.createDataFrameFromTensors({"features": x, "w": w})


@pytest.mark.parametrize("measure,weighted", [("squaredEuclidean", False), ("cosine", False),
                                               ("squaredEuclidean", True)])
def test_evaluator_bf16_frame(api_frame, monkeypatch, measure, weighted):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import KMeans
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.evaluation import ClusteringEvaluator
    x, w, df = api_frame
    kw = {"weightCol": "w"} if weighted else {}
    fit_measure = "cosine" if measure == "cosine" else "euclidean"  # KMeans names its default measure so
    pred = KMeans(k=32, seed=9, maxIter=4, tol=0.0, distanceMeasure=fit_measure, **kw).fit(df).transform(df)
    calls = []
    real = SO.silhouette_score
    monkeypatch.setattr(SO, "silhouette_score", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = ClusteringEvaluator(distanceMeasure=measure, **kw).evaluate(pred)
    assert calls == [1]  # the kernel path
    lab = pred._numeric("prediction").to(torch.int32)
    K = int(lab.max()) + 1
    o = _oracle(x.double(), lab, K, w if weighted else None, measure == "cosine", 256)
    print(f"evaluate {measure} weighted={weighted}: {got:.6f} ref {o['sil']:.6f} bound {o['bound']:.2e}")
    assert o["bound"] < 2e-3
    assert abs(got - o["sil"]) <= o["bound"]


def test_evaluator_f32_frame_takes_reference(api_frame, spark, monkeypatch):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.evaluation import ClusteringEvaluator
    x, w, _ = api_frame
    n = 50_000
    xf = x[:n].float()
    lab = torch.randint(0, 32, (n,), device=DEV, dtype=torch.int32)
    df = spark.createDataFrameFromTensors({"features": xf, "prediction": lab, "w": w[:n]})

    def boom(*a, **k):
        raise AssertionError("f32 rows must not take the bf16 kernel")
    monkeypatch.setattr(SO, "silhouette_score", boom)
    monkeypatch.setattr(SO, "label_wsum", boom)
    for cosine in (False, True):
        got = ClusteringEvaluator(distanceMeasure="cosine" if cosine else "squaredEuclidean",
                                  weightCol="w").evaluate(df)
        cpu = SO.silhouette_reference(xf.cpu(), lab.cpu(), 32, w[:n].cpu(), cosine)
        assert abs(got - float(cpu[0] / cpu[1])) <= 1e-9


def test_evaluator_memory(spark):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.evaluation import ClusteringEvaluator
    xd, lab, w = _data(400_000, 256, 64, False, 3.0, 0.0)
    df = spark.createDataFrameFromTensors({"features": xd, "prediction": lab})
    ev = ClusteringEvaluator()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    val = ev.evaluate(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    xbytes = xd.numel() * xd.element_size()
    print(f"evaluate peak rise {rise / xd.shape[0]:.1f} B/row = {100.0 * rise / xbytes:.1f} % of X")
    assert rise < 0.25 * xbytes
    assert 0.0 < val < 1.0


@pytest.mark.parametrize("n,d,K", [(6000, 32, 1500), (3000, 600, 8)])
def test_evaluator_routing_outside_limits(spark, monkeypatch, n, d, K):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.evaluation import ClusteringEvaluator
    g = torch.Generator(device=DEV).manual_seed(3)
    cen = torch.randn(K, d, generator=g, device=DEV) * 3
    lab = torch.randint(0, K, (n,), generator=g, device=DEV)
    lab[0] = K - 1
    x = (cen[lab] + torch.randn(n, d, generator=g, device=DEV)).to(torch.bfloat16)
    lab = lab.to(torch.int32)
    df = spark.createDataFrameFromTensors({"features": x, "prediction": lab})

    def boom(*a, **k):
        raise AssertionError("outside the kernel's limits: the reference form is expected")
    monkeypatch.setattr(SO, "silhouette_score", boom)
    got = ClusteringEvaluator().evaluate(df)
    cpu = SO.silhouette_reference(x.cpu().double(), lab.cpu(), K)
    assert abs(got - float(cpu[0] / cpu[1])) <= 1e-9
