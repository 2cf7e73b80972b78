"""GaussianMixture over 2 gloo ranks on the CPU: a bad weight on rank 1 only makes both ranks raise the same
ValueError before the first collective of the fit (nobody is left waiting), and a valid weighted fit returns the
one-rank model on both."""
import json
import os
import socket

import numpy as np
import torch.multiprocessing as mp

MODES = ("good", "negative", "nan")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dataset():
    rs = np.random.RandomState(4)
    n = 400
    lab = rs.randint(0, 2, n)
    x = np.where(lab[:, None] == 0, [-4.0, 1.0, 0.0], [4.0, -1.0, 2.0]) + 0.5 * rs.randn(n, 3)
    return x, rs.randint(0, 4, n).astype(np.float64)


def _fit(spark, mode, rank, world):
    import torch
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import GaussianMixture
    x, w = _dataset()
    idx = np.arange(len(w)) if world == 1 else np.array_split(np.arange(len(w)), world)[rank]
    x, w = x[idx], w[idx].copy()
    if mode != "good" and rank == world - 1:
        w[5] = -1.0 if mode == "negative" else float("nan")
    df = spark.createDataFrameFromTensors({"features": torch.as_tensor(x), "w": torch.as_tensor(w)})
    try:
        m = GaussianMixture(k=2, seed=3, maxIter=5, tol=0.0, weightCol="w").fit(df)
    except ValueError as e:
        return {"error": str(e)}
    return {"weights": m.weights, "mus": [g[0].toArray().tolist() for g in m.gaussians],
            "ll": m.summary.logLikelihood}


def _rank_main(rank, world, port, out_path):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "CML_FORCE_CPU": "1"})
    import torch
    torch.set_num_threads(1)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    assert spark.world_size == world
    res = {m: _fit(spark, m, rank, world) for m in MODES}
    spark._comm.barrier()
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump(res, fh)
    spark.stop()


def test_bad_weight_on_one_rank_raises_on_both(tmp_path, monkeypatch):
    monkeypatch.setenv("CML_FORCE_CPU", "1")
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    act = SparkSession.getActiveSession()
    mine = act is None or act._stopped  # a session made here is stopped here: later modules choose their own
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    try:
        one = _fit(spark, "good", 0, 1)
    finally:
        if mine:
            spark.stop()
    assert "error" not in one
    out = str(tmp_path / "gmm")
    mp.start_processes(_rank_main, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    for rank in range(2):
        with open(f"{out}.{rank}") as fh:
            res = json.load(fh)
        for mode in ("negative", "nan"):
            assert res[mode] == {"error": "weights must be finite and non-negative (column 'w')"}, (rank, res)
        np.testing.assert_allclose(res["good"]["weights"], one["weights"], rtol=1e-9)
        np.testing.assert_allclose(res["good"]["mus"], one["mus"], rtol=1e-9)
        np.testing.assert_allclose(res["good"]["ll"], one["ll"], rtol=1e-10)
