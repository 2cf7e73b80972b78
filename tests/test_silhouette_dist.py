"""ClusteringEvaluator over 2 gloo ranks on the CPU: cosine with weights, a cluster that lives on rank 1
only, a rank without rows, and a zero-length row on one rank (every rank raises, nobody is left waiting in a
collective). Both ranks return the one-rank value."""
import json
import os
import socket

import numpy as np
import torch.multiprocessing as mp

MODES = ("split", "empty0", "zero")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dataset():
    rs = np.random.RandomState(7)
    n, d, k = 900, 8, 5
    cen = rs.randn(k, d) * 3 + 2
    lab = rs.randint(0, k, n)
    x = cen[lab] + rs.randn(n, d)
    lab = np.where(rs.rand(n) < 0.1, rs.randint(0, k, n), lab).astype(np.int32)
    w = rs.randint(0, 4, n).astype(np.float64)
    return x, lab, w


def _shard(mode, rank, world):
    """Row indices of ``rank``: cluster 4 lives on the last rank only; ``empty0``: rank 0 holds nothing."""
    x, lab, w = _dataset()
    idx = np.arange(len(lab))
    if world == 1:
        return idx
    if mode == "empty0":
        return idx[:0] if rank == 0 else idx
    rest = idx[lab != 4]
    return rest[: len(rest) // 2] if rank == 0 else np.concatenate([rest[len(rest) // 2:], idx[lab == 4]])


def _evaluate(spark, mode, rank, world):
    import torch
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.evaluation import ClusteringEvaluator
    x, lab, w = _dataset()
    idx = _shard(mode, rank, world)
    x, lab, w = x[idx].copy(), lab[idx], w[idx]
    if mode == "zero" and rank == world - 1:
        x[3] = 0.0
    df = spark.createDataFrameFromTensors({"features": torch.as_tensor(x).reshape(-1, 8),
                                           "prediction": torch.as_tensor(lab), "w": torch.as_tensor(w)})
    try:
        return {"value": ClusteringEvaluator(distanceMeasure="cosine", weightCol="w").evaluate(df)}
    except ValueError as e:
        return {"error": str(e)}


def _rank_main(rank, world, port, out_path):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "CML_FORCE_CPU": "1"})
    import torch
    torch.set_num_threads(1)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    assert spark.world_size == world
    res = {m: _evaluate(spark, m, rank, world) for m in MODES}
    spark._comm.barrier()
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump(res, fh)
    spark.stop()


def test_two_ranks_match_one(tmp_path, monkeypatch):
    monkeypatch.setenv("CML_FORCE_CPU", "1")
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    one = _evaluate(spark, "split", 0, 1)["value"]
    assert 0.0 < one < 1.0
    lab = _dataset()[1]
    assert set(lab[_shard("split", 0, 2)]) == {0, 1, 2, 3} and 4 in set(lab[_shard("split", 1, 2)])
    assert len(_shard("empty0", 0, 2)) == 0
    out = str(tmp_path / "sil")
    mp.start_processes(_rank_main, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    for rank in range(2):
        with open(f"{out}.{rank}") as fh:
            res = json.load(fh)
        assert abs(res["split"]["value"] - one) <= 1e-12, (rank, res)
        assert abs(res["empty0"]["value"] - one) <= 1e-12, (rank, res)
        assert res["zero"] == {"error": "Cosine distance is not defined for zero-length vectors."}, (rank, res)
