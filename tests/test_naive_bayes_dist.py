"""NaiveBayes over 2 gloo ranks on the CPU: the all-reduced class sums of the shards give the one-rank model
(complement and gaussian), and a feature that fails the check on one rank only raises on both ranks."""
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
    rs = np.random.RandomState(4)
    n = 600
    y = rs.randint(0, 3, n)
    counts = rs.poisson(1.0 + 2.0 * np.eye(3)[y] @ rs.rand(3, 4)).astype(np.float64)
    real = rs.randn(n, 4) + y[:, None] * [1.0, -0.5, 0.0, 0.3]
    return counts, real, y.astype(np.float64), rs.uniform(0.5, 2.0, n)


def _fit(spark, rank, world):
    import torch
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import NaiveBayes
    counts, real, y, w = _dataset()
    idx = np.arange(len(y)) if world == 1 else np.array_split(np.arange(len(y)), world)[rank]
    res = {}
    for mt, x in (("complement", counts), ("gaussian", real)):
        df = spark.createDataFrameFromTensors({"features": torch.as_tensor(x[idx]), "label": torch.as_tensor(y[idx]),
                                               "w": torch.as_tensor(w[idx])})
        m = NaiveBayes(modelType=mt, weightCol="w", smoothing=0.7).fit(df)
        res[mt] = {"pi": m.pi.toArray().tolist(), "theta": m.theta.toArray().tolist(),
                   "sigma": m.sigma.toArray().tolist()}
    # a negative count on the last row of the last rank only
    bad = counts[idx].copy()
    if rank == world - 1:
        bad[-1, 2] = -1.0
    df = spark.createDataFrameFromTensors({"features": torch.as_tensor(bad), "label": torch.as_tensor(y[idx])})
    try:
        NaiveBayes(modelType="complement").fit(df)
        res["raised"] = ""
    except ValueError as e:
        res["raised"] = str(e)
    return res


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


def test_two_ranks_give_the_one_rank_model_and_raise_together(tmp_path, monkeypatch):
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
    assert "non-negative feature values" in one["raised"]
    assert np.asarray(one["gaussian"]["sigma"]).shape == (3, 4) and np.asarray(one["complement"]["sigma"]).size == 0
    out = str(tmp_path / "nb")
    mp.start_processes(_rank_main, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    for rank in range(2):
        with open(f"{out}.{rank}") as fh:
            res = json.load(fh)
        assert res["raised"] == one["raised"]
        for mt in ("complement", "gaussian"):
            for k in ("pi", "theta", "sigma"):
                np.testing.assert_allclose(np.asarray(res[mt][k]), np.asarray(one[mt][k]), rtol=1e-10, atol=1e-13)
