"""GeneralizedLinearRegression with family="tweedie" and offsetCol over 2 gloo ranks on the CPU: the all-reduced
``[G | stats]`` of the shards gives the one-rank model, summary included."""
import json
import os
import socket

import numpy as np
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dataset():
    rs = np.random.RandomState(6)
    n = 600
    x = rs.randn(n, 3) * [0.5, 0.3, 0.8]
    e = rs.uniform(0.5, 2.0, n)
    mu = e * np.exp(x @ [0.4, -0.3, 0.2] + 1.0)
    cnt = rs.poisson(2.0 * np.sqrt(mu))
    y = np.where(cnt > 0, rs.gamma(np.maximum(cnt, 1), 0.5 * np.sqrt(mu)), 0.0)
    return x, y, np.log(e), rs.uniform(0.5, 2.0, n)


def _fit(spark, rank, world):
    import torch
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import GeneralizedLinearRegression
    x, y, off, w = _dataset()
    idx = np.arange(len(y)) if world == 1 else np.array_split(np.arange(len(y)), world)[rank]
    df = spark.createDataFrameFromTensors({"features": torch.as_tensor(x[idx]), "label": torch.as_tensor(y[idx]),
                                           "off": torch.as_tensor(off[idx]), "w": torch.as_tensor(w[idx])})
    m = GeneralizedLinearRegression(family="tweedie", variancePower=1.5, linkPower=0.0, offsetCol="off", weightCol="w",
                                    tol=1e-12).fit(df)
    s = m.summary
    return {"coef": m.coefficients.toArray().tolist(), "b0": m.intercept, "it": s.numIterations,
            "summary": [s.deviance, s.nullDeviance, s.dispersion, s.residualDegreeOfFreedom]}


def _rank_main(rank, world, port, out_path):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "CML_FORCE_CPU": "1"})
    import torch
    torch.set_num_threads(1)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    assert spark.world_size == world
    res = _fit(spark, rank, world)
    spark._comm.barrier()
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump(res, fh)
    spark.stop()


def test_two_ranks_give_the_one_rank_model(tmp_path, monkeypatch):
    monkeypatch.setenv("CML_FORCE_CPU", "1")
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    act = SparkSession.getActiveSession()
    mine = act is None or act._stopped  # a session made here is stopped here: later modules choose their own
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    try:
        one = _fit(spark, 0, 1)
    finally:
        if mine:
            spark.stop()
    assert one["it"] > 2
    out = str(tmp_path / "glr")
    mp.start_processes(_rank_main, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    for rank in range(2):
        with open(f"{out}.{rank}") as fh:
            res = json.load(fh)
        assert res["it"] == one["it"]
        np.testing.assert_allclose(res["coef"], one["coef"], rtol=1e-9)
        np.testing.assert_allclose(res["b0"], one["b0"], rtol=1e-9)
        np.testing.assert_allclose(res["summary"], one["summary"], rtol=1e-9)
