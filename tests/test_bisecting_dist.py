"""BisectingKMeans over 2 gloo ranks on the CPU: a weighted cosine fit with a blob that lives on rank 1 only, a
rank without rows, and a zero-length row on one rank (every rank raises, nobody is left waiting in a
collective). Both ranks return the one-rank model."""
import json
import os
import socket

import numpy as np
import torch.multiprocessing as mp

MODES = ("split", "empty0", "zero")
DIRS = np.array([[1.0, 0.15, 0.0], [1.0, -0.15, 0.0], [0.0, 0.15, 1.0], [0.0, -0.15, 1.0]])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dataset():
    rs = np.random.RandomState(11)
    n = 480
    lab = rs.randint(0, 4, n)
    u = DIRS[lab] / np.linalg.norm(DIRS[lab], axis=1, keepdims=True) + rs.randn(n, 3) * 0.01
    x = u * (10.0 ** rs.uniform(-1, 2, n))[:, None]
    w = rs.randint(0, 4, n).astype(np.float64)
    return x, lab, w


def _shard(mode, rank, world):
    """Row indices of ``rank``: blob 3 lives on the last rank only; ``empty0``: rank 0 holds nothing."""
    x, lab, w = _dataset()
    idx = np.arange(len(lab))
    if world == 1:
        return idx
    if mode == "empty0":
        return idx[:0] if rank == 0 else idx
    rest = idx[lab != 3]
    return rest[: len(rest) // 2] if rank == 0 else np.concatenate([rest[len(rest) // 2:], idx[lab == 3]])


def _fit(spark, mode, rank, world):
    import torch
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import BisectingKMeans
    x, lab, w = _dataset()
    idx = _shard(mode, rank, world)
    x, w = x[idx].copy(), w[idx]
    if mode == "zero" and rank == world - 1:
        x[3] = 0.0
    df = spark.createDataFrameFromTensors({"features": torch.as_tensor(x).reshape(-1, 3), "w": torch.as_tensor(w)})
    try:
        m = BisectingKMeans(k=4, seed=3, distanceMeasure="cosine", weightCol="w").fit(df)
    except ValueError as e:
        return {"error": str(e)}
    nodes = m._nodes()
    return {"centers": [nd.center.tolist() for nd in nodes], "index": [nd.index for nd in nodes],
            "sizes": [int(round(nd.size)) for nd in nodes], "cost": m.trainingCost}


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


def test_two_ranks_match_one(tmp_path, monkeypatch):
    monkeypatch.setenv("CML_FORCE_CPU", "1")
    for v in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    act = SparkSession.getActiveSession()
    mine = act is None or act._stopped  # a session made here is stopped here: later modules choose their own
    spark = SparkSession.builder.master("local[1]").getOrCreate()
    try:
        one = _fit(spark, "split", 0, 1)
    finally:
        if mine:
            spark.stop()
    assert one["index"] == [-1, -2, 0, 1, -3, 2, 3] and one["sizes"][0] == 480
    lab = _dataset()[1]
    assert set(lab[_shard("split", 0, 2)]) == {0, 1, 2} and 3 in set(lab[_shard("split", 1, 2)])
    assert len(_shard("empty0", 0, 2)) == 0
    out = str(tmp_path / "bkm")
    mp.start_processes(_rank_main, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    for rank in range(2):
        with open(f"{out}.{rank}") as fh:
            res = json.load(fh)
        for mode in ("split", "empty0"):
            got = res[mode]
            assert got["index"] == one["index"] and got["sizes"] == one["sizes"], (rank, mode, got)
            np.testing.assert_allclose(got["centers"], one["centers"], rtol=1e-10)
            np.testing.assert_allclose(got["cost"], one["cost"], rtol=1e-9)
        assert res["zero"] == {"error": "Cosine distance is not defined for zero-length vectors."}, (rank, res)
