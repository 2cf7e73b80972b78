"""Record tests/golden/kmeans_fits.json: one small KMeans fit per route of the Lloyd engine.

Run at the commit whose behaviour is to be pinned (tests/test_kmeans_golden.py replays the same sequence and
compares): ``python scripts/record_kmeans_golden.py [--out FILE] [--only cpu|gpu]``. Host cases run anywhere,
GPU cases need a device; records of cases that were not run are kept from the existing file. Every case runs
twice on freshly made rows, and a case whose two runs differ in any recorded field is refused (named on
stderr, exit status 1) instead of written.

The sequence of a case: ``LloydEngine(...)``, the k-means|| init with seed 7, ``set_centers``, ``fit(5, 0.0)``,
``final_labels()``, ``training_cost()``.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "kmeans_fits.json")

# name, rows ("host" or the device dtype), n, d, k, engine arguments; "weights" / "streamed" are expanded in build()
CASES = [
    ("cpu_exact_noprune", "host", 300, 5, 6, dict(prune=False)),
    ("cpu_exact_prune", "host", 300, 5, 6, dict(prune=True)),
    ("cpu_cosine", "host", 300, 5, 6, dict(spherical=True)),
    ("cpu_weighted", "host", 300, 5, 6, dict(weights=True)),
    # (the device pruned step needs a K9r plan: padded width 128 is the narrowest that has one; narrower device
    # rows take the torch-form pruned step)
    ("gpu_bf16_pruned_dev", "bf16", 4096, 128, 8, dict()),
    ("gpu_bf16_pruned_torch_form", "bf16", 4096, 16, 8, dict()),
    ("gpu_bf16_incremental", "bf16", 4096, 16, 8, dict(prune=False, incremental=True)),
    ("gpu_bf16_two_chunks", "bf16", 4096, 16, 8, dict(row_chunks=2, prune=False)),
    ("gpu_e4m3", "e4m3", 2048, 256, 8, dict()),
    ("gpu_f32_screen", "f32", 2048, 128, 8, dict(precision="screen")),
    ("gpu_f32_exact", "f32", 1024, 5, 6, dict(precision="exact")),
    ("gpu_weighted_source", "f64", 1024, 5, 6, dict(weights=True)),
    ("gpu_weighted_bf16", "bf16", 1024, 16, 8, dict(weights=True, precision="bf16")),
    ("gpu_cosine_bf16", "bf16", 1024, 16, 8, dict(spherical=True)),
    ("gpu_streamed_host_rows", "host", 4096, 16, 8, dict(streamed=True, stream_chunk_rows=1024)),
]
_DTYPES = {"bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn, "f32": torch.float32, "f64": torch.float64}


def needs_gpu(case) -> bool:
    return case[1] != "host" or bool(case[5].get("streamed"))


def build(case):
    """(rows, d, k, engine keyword arguments) of a case, on freshly generated data: default_rng(3) normals plus
    3 * integers(0, 4) per row (separated clusters: no label hangs on a last-bit tie)."""
    _, rows, n, d, k, kw = case
    kw = dict(kw)
    g = np.random.default_rng(3)
    x = torch.from_numpy(g.standard_normal((n, d)) + 3.0 * g.integers(0, 4, size=(n, 1)))
    if kw.pop("weights", False):
        kw["weights"] = torch.from_numpy(g.uniform(0.5, 2.0, size=n))
    if kw.pop("streamed", False):
        x, kw["device"] = x.to(torch.float32), torch.device("cuda", 0)
    elif rows != "host":
        dev = torch.device("cuda", 0)
        x = x.to(dev).to(torch.float32).to(_DTYPES[rows]) if rows != "f64" else x.to(dev)
        if "weights" in kw:
            kw["weights"] = kw["weights"].to(dev)
    return x, d, k, kw


def run_case(case) -> dict:
    """The pinned sequence; returns the record plus the raw arrays (under "_arrays") for tolerance compares."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import LloydEngine
    x, d, k, kw = build(case)
    eng = LloydEngine(x, d, k, **kw)
    init = np.ascontiguousarray(eng.init_kmeans_parallel(seed=7), dtype=np.float64)
    eng.set_centers(init)
    eng.fit(5, 0.0)
    labels = eng.final_labels().cpu().numpy().astype(np.int64)
    centres = np.ascontiguousarray(eng.centers.cpu().numpy(), dtype=np.float64)
    cost = float(eng.training_cost())
    return {"name": case[0], "init": init.tobytes().hex(), "centres": centres.tobytes().hex(),
            "labels_sha1": hashlib.sha1(labels.tobytes()).hexdigest(), "cost": cost.hex(),
            "precision": eng.precision, "pdev": bool(eng._pdev), "delta": eng.delta is not None,
            "_arrays": (init, centres, labels, cost)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--only", choices=["cpu", "gpu"], default=None)
    args = ap.parse_args()
    records = {}
    if os.path.exists(args.out):
        with open(args.out, encoding="utf-8") as fh:
            records = {r["name"]: r for r in json.load(fh)}
    refused = []
    for case in CASES:
        gpu = needs_gpu(case)
        if (gpu and (args.only == "cpu" or not torch.cuda.is_available())) or (not gpu and args.only == "gpu"):
            continue
        a, b = run_case(case), run_case(case)
        a.pop("_arrays"), b.pop("_arrays")
        if a != b:
            refused.append(case[0])
            print(f"refused (two runs differ): {case[0]}: {[f for f in a if a[f] != b[f]]}", file=sys.stderr)
            continue
        records[case[0]] = a
        print(f"recorded {case[0]}: precision={a['precision']} pdev={a['pdev']} delta={a['delta']} cost={a['cost']}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump([records[c[0]] for c in CASES if c[0] in records], fh, indent=0)
        fh.write("\n")
    return 1 if refused else 0


if __name__ == "__main__":
    sys.exit(main())
