"""K27 (``_native/csrc/bisect.hip``): one BisectingKMeans iteration on bf16 / e4m3 rows against an f64 oracle
written from the definition, and the estimator on the kernel against its own reference form.

Op-level data: 4099 listed rows (the last unit and the last batch are partial) in m = 3 nodes of 5, 3000 and
1094 rows (a node boundary inside a unit, a node that spans many units, the last node with a dead right child)
plus 64 rows of no divided node, which hold NaN and must never be read. x = node centre + N(0, 1) with centre
components of magnitude 6 .. 10, so every |x| stays far above 2^-10 and every euclidean partial sum of integer
weights is exactly representable in f64; children = node centre -+ 0.25 · a random direction (cosine: scaled to
unit length), so the choices are about balanced and many rows sit near the boundary.

Choice band (u = 2^-53 on dp-term recursive sums, for either form of the decision): the kernel may differ from
the oracle only where |d_L - d_R| <= 8 (dp + 3) u (|x|^2 + |c_L|^2 + |c_R|^2) (euclidean) or 8 (dp + 4) u
(cosine); at most 0.1 % of the rows may lie in that band (0 are expected).
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import bisect_ops as BO
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import silhouette_ops as SO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
U = 2.0 ** -53
SIZES = (5, 3000, 1094)
EXTRA = 64
CASES = [(torch.bfloat16, 10), (torch.bfloat16, 64), (torch.bfloat16, 500), (torch.float8_e4m3fn, 256)]
_cache = {}


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _data(dtype, d, cosine):
    """Rows in the kernels' layout, the per-row slot, the children, alive, integer weights and the f64 oracle
    (made once per case and shared, never modified)."""
    key = (dtype, d, cosine)
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(1000 + d + (7 if cosine else 0))
    n = sum(SIZES) + EXTRA
    slot = np.repeat(np.arange(-1, 3), (EXTRA,) + SIZES)
    rs.shuffle(slot)
    cen = rs.uniform(6.0, 10.0, (3, d)) * rs.choice([-1.0, 1.0], (3, d))
    x = cen[np.maximum(slot, 0)] + rs.randn(n, d)
    xh = to_device_matrix(torch.as_tensor(x).to(torch.float32).to(dtype), d).clone()
    dp = int(xh.shape[1])
    fp8 = dtype == torch.float8_e4m3fn
    xh.view(torch.uint8 if fp8 else torch.int16)[torch.as_tensor(slot < 0)] = 0x7f if fp8 else 0x7fc0  # NaN
    xd = xh.to(DEV)
    u = _unit(rs.randn(3, d))
    ch = np.zeros((3, 2, dp))
    ch[:, 0, :d], ch[:, 1, :d] = cen - 0.25 * u, cen + 0.25 * u
    if cosine:
        ch = _unit(ch)
    alive = np.array([[1, 1], [1, 1], [1, 0]], dtype=bool)
    w = rs.randint(0, 4, n).astype(np.float64)
    v = xh.to(torch.float32).to(torch.float64).numpy()
    v[slot < 0] = 0.0
    s = np.maximum(slot, 0)
    xx = (v * v).sum(1)
    nrm = np.sqrt(np.where(slot >= 0, xx, 1.0))
    if cosine:
        dl = 1.0 - (v * ch[s, 0]).sum(1) / nrm
        dr = 1.0 - (v * ch[s, 1]).sum(1) / nrm
        band = np.full(n, 8.0 * (dp + 4) * U)
    else:
        dl = ((v - ch[s, 0]) ** 2).sum(1)
        dr = ((v - ch[s, 1]) ** 2).sum(1)
        band = 8.0 * (dp + 3) * U * (xx + (ch[s, 0] ** 2).sum(1) + (ch[s, 1] ** 2).sum(1))
    close = np.abs(dl - dr) <= band
    go = np.where(alive[s, 1], np.where(alive[s, 0], dr < dl, True), False)
    out = dict(xd=xd, dp=dp, n=n, slot=slot, ch=ch, alive=alive, w=w, v=v, xx=xx, nrm=nrm, go=go,
               close=close & alive[s].all(1) & (slot >= 0), listed=slot >= 0)
    _cache[key] = out
    return out


def _oracle_stats(D, weighted, cosine):
    """[S | W | Q | N] of the oracle's own choices: dense f64 index_add_ from the definition."""
    dp, lst = D["dp"], D["listed"]
    w = D["w"] if weighted else np.ones(D["n"])
    om = w / D["nrm"] if cosine else w
    q = np.zeros(D["n"]) if cosine else w * D["xx"]
    part = np.concatenate([D["v"] * om[:, None], w[:, None], q[:, None], np.ones((D["n"], 1))], 1)[lst]
    row = torch.as_tensor((2 * D["slot"] + D["go"])[lst].astype(np.int64))
    stats = torch.zeros(6, dp + 3, dtype=torch.float64).index_add_(0, row, torch.as_tensor(part))
    mass = torch.zeros(6, dp, dtype=torch.float64).index_add_(0, row, torch.as_tensor(np.abs(part[:, :dp])))
    return stats.numpy(), mass.numpy()


def _run(D, weighted, cosine, want_sums=True):
    xd = D["xd"]
    plan = BO.make_plan(torch.as_tensor(D["slot"], device=DEV), 3)
    w = torch.as_tensor(D["w"], device=DEV) if weighted else None
    nrm2 = SO.row_sqnorm(xd)
    if cosine:
        nrm = torch.sqrt(nrm2)
        omega, nrm2 = (torch.reciprocal(nrm) if w is None else w / nrm), None
    else:
        omega = w
    choice, stats = BO.bisect_step(xd, plan, torch.as_tensor(D["ch"], device=DEV),
                                   torch.as_tensor(D["alive"], device=DEV), omega, w, nrm2, cosine, want_sums)
    return plan, choice, stats


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("dtype,d", CASES)
def test_step_against_oracle(dtype, d, cosine, weighted):
    D = _data(dtype, d, cosine)
    dp = D["dp"]
    plan, choice, stats = _run(D, weighted, cosine)
    torch.cuda.synchronize()
    perm = plan.perm.cpu().numpy()
    assert plan.npos == sum(SIZES) and choice.shape == (plan.npos,) and D["listed"][perm].all()
    assert np.array_equal(D["slot"][perm], np.repeat(np.arange(3), SIZES))
    got = choice.cpu().numpy().astype(bool)
    nband = int(D["close"][perm].sum())
    differ = got != D["go"][perm]
    print(f"{dtype} d={d} cosine={cosine} weighted={weighted}: rows in the band {nband}, "
          f"choices that differ {int(differ.sum())}, right {int(got.sum())} of {plan.npos}")
    assert nband <= 0.001 * plan.npos
    assert not (differ & ~D["close"][perm]).any()
    two = got[D["slot"][perm] == 1]
    assert 0.3 < two.mean() < 0.7            # about balanced
    assert not got[D["slot"][perm] == 2].any()  # the dead right child attracts nobody
    want, mass = _oracle_stats(D, weighted, cosine)
    S = stats.cpu().numpy()
    assert np.isfinite(S).all()              # the NaN rows of no divided node were never read
    assert not differ.any()                  # the sums below are those of the oracle's choices
    np.testing.assert_array_equal(S[:, dp + 2], want[:, dp + 2])  # N counts rows, weight 0 included
    np.testing.assert_array_equal(S[:, dp], want[:, dp])          # W
    assert not S[5].any() and S[4, dp + 2] == SIZES[2]            # a dead child's statistics are zero
    if cosine:
        assert not S[:, dp + 1].any()
        bound = 2.0 * want[:, dp + 2][:, None] * U * mass
        err = np.abs(S[:, :dp] - want[:, :dp])
        print(f"  cosine sums: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
    else:
        np.testing.assert_array_equal(S, want)  # every partial sum is exact: bit for bit
    # the same bits again, and the choices alone
    _, choice2, stats2 = _run(D, weighted, cosine)
    assert torch.equal(choice2, choice) and torch.equal(stats2, stats)
    _, choice3, none = _run(D, weighted, cosine, want_sums=False)
    assert none is None and torch.equal(choice3, choice)


def test_reference_form_agrees_on_device():
    """The reference form on the same device rows (the estimator's fallback) makes the oracle's choices."""
    D = _data(torch.bfloat16, 64, False)
    x = D["xd"].clone()
    x[torch.as_tensor(~D["listed"], device=DEV)] = 0
    choice, stats = BO.bisect_step_reference(x, torch.as_tensor(D["slot"], device=DEV),
                                             torch.as_tensor(D["ch"], device=DEV),
                                             torch.as_tensor(D["alive"], device=DEV),
                                             torch.as_tensor(D["w"], device=DEV))
    assert np.array_equal(choice.cpu().numpy().astype(bool)[D["listed"]], D["go"][D["listed"]])
    want, _ = _oracle_stats(D, True, False)
    np.testing.assert_array_equal(stats.cpu().numpy(), want)


def test_exact_tie_goes_left():
    rs = np.random.RandomState(3)
    n, dp = 300, 16
    x = rs.randint(-4, 5, (n, dp)).astype(np.float64)
    x[:, 0] = 1.0        # |x - 0|^2 == |x - 2 e_0|^2 exactly
    x[200:, 0] = 2.0     # strictly closer to the right child
    xd = torch.as_tensor(x).to(torch.bfloat16).to(DEV)
    ch = np.zeros((1, 2, dp))
    ch[0, 1, 0] = 2.0
    plan = BO.make_plan(torch.zeros(n, dtype=torch.int64, device=DEV), 1)
    choice, stats = BO.bisect_step(xd, plan, torch.as_tensor(ch, device=DEV),
                                   torch.ones(1, 2, dtype=torch.bool, device=DEV), nrm2=SO.row_sqnorm(xd))
    got = choice.cpu().numpy()
    assert not got[:200].any() and got[200:].all()
    assert stats[0, dp + 2].item() == 200 and stats[1, dp + 2].item() == 100


def test_no_position_is_no_launch():
    xd = torch.ones(40, 16, dtype=torch.bfloat16, device=DEV)
    plan = BO.make_plan(torch.full((40,), -1, dtype=torch.int64, device=DEV), 2)
    choice, stats = BO.bisect_step(xd, plan, torch.zeros(2, 2, 16, dtype=torch.float64, device=DEV),
                                   torch.ones(2, 2, dtype=torch.bool, device=DEV), nrm2=SO.row_sqnorm(xd))
    torch.cuda.synchronize()
    assert choice.numel() == 0 and stats.shape == (4, 19) and not stats.any()


# ------------------------------------------------------------------------------------------------- estimator
@pytest.fixture(scope="module")
def spark():
    """A GPU session of this module's own, beside whichever session is active: a host session left active by
    another module would keep the frames on the CPU, where no kernel runs, and the modules that follow find the
    active session as they would without this one."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    s = SparkSession({"spark.master": "mi355x", "spark.app.name": "bisect"})
    assert s.device.type == "cuda"
    yield s
    s.stop()


def _blobs(n, d, seed=0):
    """Four blobs in two pairs (root -> two pairs -> four), f32 on the device, and integer weights."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = torch.randn(2, d, generator=g, device=DEV) * 4.0 + 3.0
    cen = torch.cat([a, a + 1.5 * torch.randn(2, d, generator=g, device=DEV).sign()])[[0, 2, 1, 3]]
    lab = torch.randint(0, 4, (n,), generator=g, device=DEV)
    x = cen[lab] + 0.3 * torch.randn(n, d, generator=g, device=DEV)
    return x, torch.randint(0, 4, (n,), generator=g, device=DEV).to(torch.float64)


def _tree(m):
    return [(nd.index, int(round(nd.size)), [c.index for c in nd.children]) for nd in m._nodes()]


@pytest.mark.parametrize("measure,weighted", [("euclidean", False), ("euclidean", True), ("cosine", True)])
def test_estimator_kernel_equals_reference(spark, monkeypatch, measure, weighted):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import BisectingKMeans
    x, w = _blobs(20_000, 64)
    df = spark.createDataFrameFromTensors({"features": x.to(torch.bfloat16), "w": w})
    est = BisectingKMeans(k=4, seed=3, maxIter=5, distanceMeasure=measure)
    if weighted:
        est = est.setWeightCol("w")
    calls = []
    real = BO.bisect_step

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(BO, "bisect_step", counted)
    fast = est.fit(df)
    assert len(calls) >= 1 + 2 * 6  # the root, then 5 iterations and the final assignment of two levels
    del calls[:]
    monkeypatch.setenv("CML_BISECT_KERNEL", "0")
    slow = est.fit(df)
    assert not calls
    assert _tree(fast) == _tree(slow) and len(fast.clusterCenters()) == 4
    np.testing.assert_allclose(np.stack(fast.clusterCenters()), np.stack(slow.clusterCenters()), rtol=1e-12)
    np.testing.assert_allclose(fast.trainingCost, slow.trainingCost, rtol=1e-9)
    assert fast.summary.clusterSizes == [nd.size for nd in fast._leaves]


def test_other_columns_take_the_reference_form(spark, monkeypatch):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import BisectingKMeans

    def boom(*a, **k):
        raise AssertionError("outside the kernel's limits: the reference form is expected")
    monkeypatch.setattr(BO, "bisect_step", boom)
    x, w = _blobs(3000, 64)
    for feats in (x, _blobs(3000, 1000)[0].to(torch.bfloat16)):  # f32 rows; bf16 rows of padded width 1024
        df = spark.createDataFrameFromTensors({"features": feats, "w": w})
        for est in (BisectingKMeans(k=4, seed=3, maxIter=3),
                    BisectingKMeans(k=4, seed=3, maxIter=3, distanceMeasure="cosine", weightCol="w")):
            assert len(est.fit(df).clusterCenters()) == 4


def test_fit_memory(spark):
    """Peak allocation during fit stays below half of X: per-row scalars only (index, perm, slot, choice, norm,
    factor, sort scratch: roughly 80 B per row against 512 B of a 256-wide bf16 row), no n x d temporary."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import BisectingKMeans
    x, _ = _blobs(400_000, 256)
    x = x.to(torch.bfloat16)
    df = spark.createDataFrameFromTensors({"features": x})
    est = BisectingKMeans(k=4, seed=3, maxIter=3)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = est.fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    xbytes = x.numel() * x.element_size()
    print(f"fit peak rise {rise / x.shape[0]:.1f} B/row = {100.0 * rise / xbytes:.1f} % of X")
    assert rise < 0.5 * xbytes
    assert len(m.clusterCenters()) == 4
