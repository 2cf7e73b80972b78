"""Fits of every route of the Lloyd engine against the records of tests/golden/kmeans_fits.json (written by
scripts/record_kmeans_golden.py at the commit before the engine was split into modules): the same init, centres,
labels and cost. GPU routes are deterministic and compare bit for bit; host routes compare labels exactly and
centres / cost at rtol 1e-12 (another host CPU may pick another BLAS kernel for the f64 matmuls)."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_kmeans_golden",
                                                  os.path.join(ROOT, "scripts", "record_kmeans_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(os.path.join(ROOT, "tests", "golden", "kmeans_fits.json"), encoding="utf-8") as _fh:
    GOLDEN = {r["name"]: r for r in json.load(_fh)}


def _arr(hexed, shape):
    return np.frombuffer(bytes.fromhex(hexed), dtype=np.float64).reshape(shape)


def test_every_route_is_recorded():
    assert sorted(GOLDEN) == sorted(c[0] for c in REC.CASES)
    # the device pruned step (and its seeded first step) is among the recorded routes
    assert GOLDEN["gpu_bf16_pruned_dev"]["pdev"] and not GOLDEN["gpu_bf16_incremental"]["pdev"]
    assert GOLDEN["gpu_bf16_incremental"]["delta"]


@pytest.mark.parametrize("case", [c for c in REC.CASES if not REC.needs_gpu(c)], ids=lambda c: c[0])
def test_host_fit_matches_record(case):
    want = GOLDEN[case[0]]
    got = REC.run_case(case)
    init, centres, labels, cost = got.pop("_arrays")
    for f in ("precision", "pdev", "delta", "labels_sha1"):
        assert got[f] == want[f], f
    np.testing.assert_allclose(init, _arr(want["init"], init.shape), rtol=1e-12, atol=0)
    np.testing.assert_allclose(centres, _arr(want["centres"], centres.shape), rtol=1e-12, atol=0)
    np.testing.assert_allclose(cost, float.fromhex(want["cost"]), rtol=1e-12, atol=0)
    assert hashlib.sha1(labels.tobytes()).hexdigest() == want["labels_sha1"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in REC.CASES if REC.needs_gpu(c)], ids=lambda c: c[0])
def test_gpu_fit_matches_record_bit_for_bit(case):
    want = GOLDEN[case[0]]
    got = REC.run_case(case)
    got.pop("_arrays")
    for f in ("precision", "pdev", "delta", "labels_sha1", "cost", "init", "centres"):
        assert got[f] == want[f], f
