"""Weighted KMeans on the bf16 / e4m3 MFMA path, the host side: the host twin of the weighted sums
(``ops.kmeans_ops.weighted_sums`` / ``weighted_sums_labels`` on host tensors) is the correctly rounded
exact sum of the rounded products fl64(w·x) — checked against ``math.fsum`` — whatever the row order, and
a ``local[1]`` session with ``cml.ml.kmeans.precision=bf16`` fits a weighted KMeans on the host path
(the same bits as without the conf) instead of refusing it."""
import math

import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import kmeans_ops as K


def _host_case(seed=0, n=211, d=5, k=7):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, 8, generator=g) * 3).to(torch.bfloat16)  # padded width 8 > d: columns past d are ignored
    w = torch.rand(n, generator=g, dtype=torch.float64) * 4
    w[::17] = 0.0
    xn64 = (x[:, :d].double() ** 2).sum(1)
    lab = torch.randint(0, k, (n,), generator=g)
    lab[lab == 3] = 4  # an empty cluster
    return x, w, xn64, lab, n, d, k


def test_host_weighted_sums_equal_fsum_of_rounded_products():
    x, w, xn64, lab, n, d, k = _host_case()
    S, S_lo = K.weighted_sums_labels(x, n, 8, d, w, xn64, lab, k)
    assert S.shape == (k, d + 2) and S_lo.shape == (k, d + 2)
    xs, ws, qs, ls = x[:, :d].double().tolist(), w.tolist(), xn64.tolist(), lab.tolist()
    for c in range(k):
        rows = [i for i in range(n) if ls[i] == c]
        for j in range(d):
            assert S[c, j].item() == math.fsum(ws[i] * xs[i][j] for i in rows), (c, j)
        assert S[c, d].item() == math.fsum(ws[i] for i in rows)
        assert S[c, d + 1].item() == math.fsum(ws[i] * qs[i] for i in rows)
    assert not S[3].any() and not S_lo[3].any()
    # the remainders: S + S_lo is the exact sum, so S_lo is what fsum leaves after taking S out
    for c in (0, 6):
        rows = [i for i in range(n) if ls[i] == c]
        assert S_lo[c, 0].item() == math.fsum([ws[i] * xs[i][0] for i in rows] + [-S[c, 0].item()])


def test_host_weighted_sums_do_not_depend_on_the_row_order():
    x, w, xn64, lab, n, d, k = _host_case(seed=1)
    S, S_lo = K.weighted_sums_labels(x, n, 8, d, w, xn64, lab, k)
    p = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    S2, S2_lo = K.weighted_sums_labels(x[p].contiguous(), n, 8, d, w[p].contiguous(), xn64[p].contiguous(), lab[p], k)
    assert torch.equal(S, S2) and torch.equal(S_lo, S2_lo)
    # the perm / seg form on host tensors: any permutation that groups the labels
    order = torch.argsort(lab[p], stable=True)
    seg = torch.zeros(k + 1, dtype=torch.int32)
    seg[1:] = torch.cumsum(torch.bincount(lab, minlength=k), 0)
    S3, S3_lo = K.weighted_sums(x[p].contiguous(), n, 8, d, w[p].contiguous(), xn64[p].contiguous(), k,
                                order.to(torch.int32), seg)
    assert torch.equal(S, S3) and torch.equal(S_lo, S3_lo)


def test_weighted_sums_validate_their_operands():
    x, w, xn64, lab, n, d, k = _host_case()
    with pytest.raises(ValueError):
        K.weighted_sums(x, n, 8, d, w.float(), xn64, k, torch.zeros(n, dtype=torch.int32),
                        torch.zeros(k + 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        K.weighted_sums(x, n, 8, d, w, xn64[: n - 1].contiguous(), k, torch.zeros(n, dtype=torch.int32),
                        torch.zeros(k + 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        K.weighted_sums(x, n, 8, d, w, xn64, k, torch.zeros(n, dtype=torch.int64),
                        torch.zeros(k + 1, dtype=torch.int32))


def test_local_session_weighted_fit_with_bf16_conf_equals_the_fit_without_it():
    """Host rows with precision "bf16" take the host weighted path (as an unweighted "bf16" request on host
    rows does): centres, cost and sizes are those of the fit without the conf, bit for bit."""
    import pandas as pd
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import KMeans
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.feature import VectorAssembler
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    rs = np.random.RandomState(4)
    cen = rs.randn(4, 3) * 6
    x = cen[rs.randint(0, 4, 900)] + rs.randn(900, 3)
    pdf = pd.DataFrame(x, columns=["a", "b", "c"])
    pdf["w"] = rs.uniform(0.0, 3.0, len(x))
    df = VectorAssembler(inputCols=["a", "b", "c"], outputCol="features").transform(spark.createDataFrame(pdf))
    assert spark.conf.get("cml.ml.kmeans.precision", None) is None
    m0 = KMeans(k=4, seed=2, weightCol="w").fit(df)
    spark.conf.set("cml.ml.kmeans.precision", "bf16")
    try:
        m1 = KMeans(k=4, seed=2, weightCol="w").fit(df)
    finally:
        spark.conf.unset("cml.ml.kmeans.precision")
    assert np.array_equal(np.array(m1.clusterCenters()), np.array(m0.clusterCenters()))
    assert m1.summary.trainingCost == m0.summary.trainingCost
    assert m1.summary.clusterSizes == m0.summary.clusterSizes
