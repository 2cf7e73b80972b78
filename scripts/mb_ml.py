"""Estimator-kernel microbenchmarks (GLM family and trees): one driver, one subcommand per experiment.

    python scripts/mb_ml.py glm [--scale S]
        K7 moments, K8 scale_apply, K13 logreg_grad, K24 linear_predict (and K15 gram for narrow rows) on five
        shapes from 20M x 512 fp8 to 20M x 4 f64; best-of-5 ms and TB/s
    python scripts/mb_ml.py glm-fp8 [--rows 50000000]
        fp8 x 512 GLM kernels by streaming layout (chunks per lane: auto, 2, 4) with the gradient's relative diff
    python scripts/mb_ml.py logreg [--scale S] [--out FILE.json]
        K13 logreg_grad by batch size (16K rows .. the whole shard; small batches replayed from one HIP graph so
        launch cost does not hide the kernel), partial_colsum, and K7 moments
    python scripts/mb_ml.py multinomial [--rows 100000000] [--dim 256]
        K13m multinomial loss + gradient passes over bf16 rows for C = 4, 8 (VALU kernel), 16, 32, 64 (MFMA kernel):
        best-of-3 ms, HBM TB/s of the row bytes, and the MFMA-form FLOP rate
    python scripts/mb_ml.py trees [--scale S]
        ForestEngine fits (20 trees, depth 5, 32 bins) with the phase split, cold and warm; GBT fits (20 iterations)
    python scripts/mb_ml.py tree-transform [--rows 2000000]
        the reference workflow's tree fits and transforms (ref.py:130-160) through the public API, each between
        device syncs; the first RF-regression transform also under cProfile

    python scripts/mb_ml.py silhouette [--rows 20000000] [--dim 256] [--k 256] [--dtype bf16|fp8] [--measure M]
        K26 ClusteringEvaluator kernels on blobs with 90 % true labels: the stats pass (row norms, label sort,
        label_wsum, W / Q group sums) and the score pass (one MFMA pass over X) separately, best-of-5 ms; M is
        squaredEuclidean, cosine or both; --evaluate also times ClusteringEvaluator.evaluate end to end

    python scripts/mb_ml.py bisecting [--rows 20000000] [--dim 256] [--k 8] [--max-iter 20] [--dtype bf16|fp8]
                                      [--measure euclidean|cosine] [--weighted]
        BisectingKMeans.fit end to end on blobs (seconds, ms per pass over the rows) and, where K27 takes the
        column, the step kernel alone on all rows with and without the sums; CML_BISECT_KERNEL=0 times the
        torch forms instead

    python scripts/mb_ml.py gmm [--rows 20000000] [--dim 32] [--k 8] [--max-iter 10] [--form kernel|reference|dense]
        GaussianMixture.fit end to end on overlapping bf16 blobs (seconds, ms per EM iteration, peak allocation
        rise) in one of three forms: the K28 kernel, the chunked reference form (CML_GMM_KERNEL=0), or the dense
        f64 form on an f64 copy of the same values; for the kernel also estep and predict alone

    python scripts/mb_ml.py lda [--rows 4000000] [--terms 256] [--k 10] [--subsampling 0.05] [--max-iter 10]
                                [--length 100] [--form kernel|reference|dense]
        LDA.fit (online optimizer) end to end on a planted-topic bf16 corpus (seconds, ms per iteration, peak
        allocation rise) in one of three forms: the K29 kernel, the chunked reference form (CML_LDA_KERNEL=0), or
        the dense f64 form on an f64 copy of the same values; for the kernel also the E-step alone on one
        mini-batch with its issued f64 MFMA rate, and the sweep histogram of that mini-batch

    python scripts/mb_ml.py mlp [--rows 20000000] [--layers 64,16,4] [--max-iter 10] [--form kernel|reference|dense]
                                [--pass-only]
        MultilayerPerceptronClassifier.fit end to end on bf16 rows labelled by a noisy linear rule (seconds, ms
        per loss + gradient evaluation, peak allocation rise) in one of three forms: the K30 kernel, the chunked
        reference form (CML_MLP_KERNEL=0), or the dense autograd form on an f64 copy of the same values; for the
        kernel also loss_grad and forward alone with the issued f64 MFMA rate. --pass-only skips the fit

    python scripts/mb_ml.py gram [--rows 4000000] [--dim 256] [--rounds 3] [--fits] [--pass-only]
        the Gram matrix [X 1 z]^T W [X 1 z] of wide bf16 rows (d > 30, which ``glm`` skips) in three forms,
        interleaved round by round: the K31 kernel, the chunked reference form, and the dense form on an
        n x (d + 2) f64 copy (ms, peak allocation rise); --fits adds PCA, LinearRegression(normal) and a 5-step
        poisson GeneralizedLinearRegression fit on all three; --pass-only times K31 alone with its f64 MFMA rate,
        for sizes at which the dense form does not fit

    python scripts/mb_ml.py fm [--rows 20000000] [--dim 64] [--factor-size 8] [--max-iter 10] [--rounds 2]
                               [--loss squared|logistic] [--pass-only]
        one loss + gradient evaluation of the factorisation machine and an FMRegressor / FMClassifier fit on bf16
        rows in three forms, interleaved round by round in one process: the K32 kernel, the chunked reference form
        (CML_FM_KERNEL=0), and the dense autograd form on an f64 copy of the same values (ms or s, peak allocation
        rise); then K32's loss_grad and scores alone with the issued f64 MFMA rate. --pass-only times K32 alone,
        for sizes at which the dense form does not fit

    python scripts/mb_ml.py glr_step [--rows 10000000] [--dim 64] [--rounds 3]
        one IRLS step of a poisson / log model on bf16 rows in two forms, interleaved round by round: the fused K33
        step (tweedie p = 1, log link: the same math) and one iteration of the loop the four named families keep
        (K24 linear predictor, the torch element-wise passes, K31 weighted Gram); ms, bytes read or written and TB/s

    python scripts/mb_ml.py nb [--rows 10000000] [--dim 64] [--classes 2 16] [--rounds 2] [--ops-only]
        the two row passes of naive Bayes on bf16 rows, K34 against the chunked reference form (ms, bytes, TB/s), then
        NaiveBayes fit and transform (multinomial and gaussian) in three forms, interleaved round by round: the
        kernel, the reference form (CML_NB_KERNEL=0) and the dense form on an f32 frame of the same values (ms, peak
        allocation rise); dense steps whose f64 temporaries would not fit are skipped

    python scripts/mb_ml.py aft [--shapes 10000000x64 4000000x256] [--rounds 3] [--dense-limit-gb 24]
        one L-BFGS evaluation of AFTSurvivalRegression on bf16 rows in three forms, interleaved round by round: the
        K35 kernel, the chunked reference form and the dense form of f32 / f64 columns (two GEMVs on an f64 copy
        of the rows and the element-wise passes between them; skipped where the copy would not fit); then K35's rows
        form; ms, bytes read and their rate against the 6.3 TB/s copy rate

``--scale`` multiplies every row count (e.g. 0.05 for a quick check).
"""
import argparse
import cProfile
import io
import json
import os
import pstats
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import glm_ops  # noqa: E402


def best_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e))
    return best


def graph_ms(fn, reps=20):
    """ms per call with the calls captured into one HIP graph and replayed (best of 5 replays)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        g.replay()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / reps)
    return min(ts)


def rows_x(n, d, dt):
    x = torch.randn(n, d, device="cuda")
    return (x.to(torch.bfloat16) if dt == torch.float8_e4m3fn else x).to(dt)


def glm_inputs(n, d):
    y = (torch.rand(n, device="cuda") > 0.5).double()
    return y, torch.randn(d + 1, device="cuda", dtype=torch.float64) * 0.05


def cmd_glm(argv):
    ap = argparse.ArgumentParser(prog="mb_ml.py glm")
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args(argv)
    shapes = [(20_000_000, 512, torch.float8_e4m3fn), (20_000_000, 256, torch.bfloat16),
              (10_000_000, 256, torch.float32), (20_000_000, 4, torch.float64), (20_000_000, 512, torch.bfloat16)]
    for n, d, dt in shapes:
        n = int(n * a.scale)
        x = rows_x(n, d, dt)
        y, coef = glm_inputs(n, d)
        gb = x.numel() * x.element_size() / 1e9
        mean = torch.zeros(d, dtype=torch.float64, device="cuda")
        inv = torch.ones(d, dtype=torch.float64, device="cuda")
        ops = [("moments", lambda: glm_ops.moments(x, d), 1),
               ("scale_apply", lambda: glm_ops.scale_apply(x, d, mean, inv, True, dt), 2),
               ("logreg_grad", lambda: glm_ops.logreg_grad(x, d, y, coef, None), 1),
               ("linear_predict", lambda: glm_ops.linear_predict(x, d, coef, "logistic"), 1)]
        if d <= 30:
            ops.append(("gram", lambda: glm_ops.gram(x, d, y, None), 1))
        for name, fn, passes in ops:
            t = best_ms(fn)
            print(f"n={n} d={d} {dt}: {name} {t:.3f} ms {passes * gb / t:.2f} TB/s{' (r+w)' if passes == 2 else ''}",
                  flush=True)
        del x, y
        torch.cuda.empty_cache()


def cmd_glm_fp8(argv):
    ap = argparse.ArgumentParser(prog="mb_ml.py glm-fp8")
    ap.add_argument("--rows", type=int, default=50_000_000)
    a = ap.parse_args(argv)
    n, d = a.rows, 512
    x = rows_x(n, d, torch.float8_e4m3fn)
    y, coef = glm_inputs(n, d)
    gb = x.numel() / 1e9
    ref = None
    for nch in (0, 2, 4):
        glm_ops.set_fp8_nch(nch)
        g = glm_ops.logreg_grad(x, d, y, coef, None)
        ref = g.clone() if ref is None else ref
        err = float((g - ref).abs().max() / ref.abs().max())
        t = best_ms(lambda: glm_ops.logreg_grad(x, d, y, coef, None))
        tm = best_ms(lambda: glm_ops.moments(x, d))
        tp = best_ms(lambda: glm_ops.linear_predict(x, d, coef, "logistic"))
        print(f"fp8 nch={nch or 'auto'}: logreg_grad {t:.3f} ms {gb / t:.2f} TB/s (rel diff {err:.1e}); "
              f"moments {gb / tm:.2f} TB/s; linear_predict {gb / tp:.2f} TB/s", flush=True)
    glm_ops.set_fp8_nch(0)


def cmd_logreg(argv):
    ap = argparse.ArgumentParser(prog="mb_ml.py logreg")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--unroll", type=int, default=1, help="K13 rows in flight per wave (1, 2; 0 = automatic)")
    a = ap.parse_args(argv)
    res = []
    glm_ops.set_logreg_unroll(a.unroll)
    for d, dt in ((256, torch.bfloat16), (512, torch.float8_e4m3fn), (256, torch.float32)):
        n = int((25_000_000 if dt == torch.float32 else 50_000_000) * a.scale)
        x = rows_x(n, d, dt)
        y, coef = glm_inputs(n, d)
        base = torch.zeros((), dtype=torch.int64, device="cuda")
        for b in sorted({min(b, n) for b in (16384, 131072, 1048576, n)}):
            t = graph_ms(lambda: glm_ops.logreg_grad(x, d, y, coef, None, batch=b, row_base=base),
                         reps=20 if b < n else 3)
            r = {"dtype": str(dt), "d": d, "U": a.unroll, "rows": b, "ms": round(t, 4),
                 "TB/s": round(b * d * x.element_size() / 1e9 / t, 2)}
            res.append(r)
            print(json.dumps(r), flush=True)
        part = torch.randn(1024, d + 3, dtype=torch.float64, device="cuda")
        t = graph_ms(lambda: glm_ops.partial_colsum(part))
        print(json.dumps({"op": "partial_colsum", "shape": [1024, d + 3], "us": round(t * 1e3, 2)}), flush=True)
        ts = sorted(best_ms(lambda: glm_ops.moments(x, d), 1) for _ in range(5))
        t = ts[2]
        r = {"dtype": str(dt), "d": d, "op": "moments", "rows": n, "ms": round(t, 3),
             "TB/s": round(n * d * x.element_size() / 1e9 / t, 2)}
        res.append(r)
        print(json.dumps(r), flush=True)
        del x, y
        torch.cuda.empty_cache()
    glm_ops.set_logreg_unroll(0)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


def cmd_trees(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models import trees as TR
    ap = argparse.ArgumentParser(prog="mb_ml.py trees")
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args(argv)

    def data(n, d):
        g = torch.Generator(device="cuda")
        g.manual_seed(0)
        x = torch.randn(n, d, device="cuda", dtype=torch.float64, generator=g)
        return x, 0.1 * torch.randn(n, device="cuda", dtype=torch.float64, generator=g)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    for n, d, task in ((10_000_000, 4, "regression"), (10_000_000, 4, "classification"), (2_000_000, 64, "regression")):
        n = int(n * a.scale)
        x, noise = data(n, d)
        if task == "regression":
            y, imp = 2 * x[:, 0] + (x[:, 1 % d] > 0).double() + noise, "variance"
        else:
            y, imp = ((x[:, 0] + 0.5 * x[:, 2 % d]) > 0).double(), "gini"
        p = TR.TreeParams(task=task, num_classes=2, impurity=imp, num_trees=20, seed=1, feature_subset="auto")
        times = {}
        eng = TR.ForestEngine(x, y, p)
        for name in ("find_splits", "binize", "histogram", "best_splits", "route"):
            def wrap(*args, _fn=getattr(eng, name), _name=name, **kw):
                t, r = timed(lambda: _fn(*args, **kw))
                times[_name] = times.get(_name, 0.0) + t
                return r
            setattr(eng, name, wrap)
        for rep in ("cold", "warm"):  # the first fit of a process also loads every kernel it launches
            times.clear()
            t, trees = timed(eng.fit)
            nodes = sum(TR.num_nodes(r) for r in trees)
            print(f"RF{task[:5]} n={n} d={d} ({rep}): fit {t:.3f} s ({nodes} nodes) " +
                  " ".join(f"{k}={v:.3f}s" for k, v in times.items()), flush=True)
        del x, y, eng
        torch.cuda.empty_cache()
    # gradient boosting: 20 iterations of depth-5 regression trees (GBTRegressor defaults) / logistic loss
    for n, d, loss in ((10_000_000, 4, "squared"), (10_000_000, 4, "logistic"), (2_000_000, 64, "squared")):
        n = int(n * a.scale)
        x, noise = data(n, d)
        y = torch.sin(2 * x[:, 0]) + (x[:, 1 % d] > 0).double() + noise
        if loss == "logistic":
            y = torch.where(y > 0.5, 1.0, -1.0).double()
        t, (trees, tw) = timed(lambda: TR.fit_gbt(x, y, TR.TreeParams(max_depth=5, seed=1), 20, 0.1, loss))
        f = TR.predict_forest(trees, x, "variance", 1, False, False, tw)[:, 0]
        err = float(TR.gbt_loss(loss, f, y).mean())
        print(f"GBT-{loss} n={n} d={d}: fit {t:.3f} s for {len(trees)} trees ({t / len(trees) * 1e3:.1f} ms/tree), "
              f"train loss {err:.4f}", flush=True)
        del x, y
        torch.cuda.empty_cache()


def cmd_tree_transform(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import (
        DecisionTreeClassifier, RandomForestClassifier)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.feature import VectorAssembler
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import (
        DecisionTreeRegressor, RandomForestRegressor)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    ap = argparse.ArgumentParser(prog="mb_ml.py tree-transform")
    ap.add_argument("--rows", type=int, default=int(os.environ.get("MB_ROWS", 2_000_000)))
    a = ap.parse_args(argv)
    n = a.rows
    spark = SparkSession.builder.master("mi355x" if torch.cuda.is_available() else "local[4]").getOrCreate()
    dev = spark._device
    g = torch.Generator(device=dev).manual_seed(0)
    cols = {c: torch.randint(0, 100, (n,), generator=g, device=dev).to(torch.int32)
            for c in ("admission_count", "current_occupancy", "emergency_visits")}
    cols["seasonality_index"] = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    los = (cols["admission_count"].double() * 0.05 + cols["seasonality_index"] * 3
           + torch.rand(n, generator=g, device=dev, dtype=torch.float64))
    cols["length_of_stay"] = los
    cols["LOS_binary"] = (los > 5.0).to(torch.int32)
    df = spark.createDataFrameFromTensors(cols)
    feats = ["admission_count", "current_occupancy", "emergency_visits", "seasonality_index"]

    def sync():
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def timed(name, fn):
        sync()
        t = time.perf_counter()
        out = fn()
        sync()
        print(f"{name:36s} {1000 * (time.perf_counter() - t):9.2f} ms", flush=True)
        return out

    va = VectorAssembler(inputCols=feats, outputCol="features")
    tr, te = va.transform(df).select("features", "length_of_stay").randomSplit([0.7, 0.3], seed=42)
    dt = timed("DecisionTreeRegressor.fit",
               lambda: DecisionTreeRegressor(featuresCol="features", labelCol="length_of_stay").fit(tr))
    timed("DecisionTreeRegressionModel.transform", lambda: dt.transform(te))
    rf = timed("RandomForestRegressor.fit",
               lambda: RandomForestRegressor(featuresCol="features", labelCol="length_of_stay").fit(tr))
    print("rf trees", len(rf._trees), "nodes", rf.totalNumNodes, "depths", [rf.trees[i].depth for i in range(3)])
    pr = cProfile.Profile()
    sync()
    pr.enable()
    timed("RandomForestRegressionModel.transform", lambda: rf.transform(te))
    pr.disable()
    s = io.StringIO()
    pstats.Stats(pr, stream=s).sort_stats("cumulative").print_stats(25)
    print(s.getvalue())
    for _ in range(2):
        timed("RandomForestRegressionModel.transform", lambda: rf.transform(te))
    ctr, cte = va.transform(df).select("features", "LOS_binary").randomSplit([0.7, 0.3], seed=42)
    rfc = timed("RandomForestClassifier.fit",
                lambda: RandomForestClassifier(featuresCol="features", labelCol="LOS_binary").fit(ctr))
    timed("RandomForestClassificationModel.transform", lambda: rfc.transform(cte))
    dtc = timed("DecisionTreeClassifier.fit",
                lambda: DecisionTreeClassifier(featuresCol="features", labelCol="LOS_binary").fit(ctr))
    timed("DecisionTreeClassificationModel.transform", lambda: dtc.transform(cte))


def _mode_run(mode, x, d, y, coef, C, cp, dp):
    prev = glm_ops.set_multinomial_mfma_mode(mode)
    try:
        lib = glm_ops._native.kernels()
        code = glm_ops._CODE[x.dtype]
        cp, dp = lib.cml_multinomial_mfma_supported(d, code, C), lib.cml_multinomial_mfma_dpad(d, C)
        if cp <= 0:
            return None
        return glm_ops._multinomial_mfma(x, d, y, coef, None, C, cp, dp)
    finally:
        glm_ops.set_multinomial_mfma_mode(prev)


def cmd_multinomial(argv):
    ap = argparse.ArgumentParser(prog="mb_ml.py multinomial")
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"], help="row storage (fp8: OCP e4m3)")
    ap.add_argument("--classes", default="4,8,16,32,64")
    a = ap.parse_args(argv)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.utils import synth
    dev = torch.device("cuda", 0)
    n, d = a.rows, a.dim
    x = synth.synth_rows(0, n, d, seed=3, dtype=torch.bfloat16, device=dev)
    code, esz = 0, 2
    if a.dtype == "fp8":
        x = x.to(torch.float8_e4m3fn)
        code, esz = 3, 1
    lib = __import__("clustermachinelearningforhospitalnetworks_apache_spark_amd._native",
                     fromlist=["kernels"]).kernels()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for C in (int(c) for c in a.classes.split(",")):
        y = torch.randint(0, C, (n,), generator=g, device=dev).to(torch.float64)
        coef = torch.randn(C, d + 1, generator=g, device=dev, dtype=torch.float64) * 0.05
        # MFMA form: margins + gradient on the padded class tile (16, 32 or 64 classes)
        flop = 4.0 * n * d * (16 if C <= 16 else 32 if C <= 32 else 64)  # (mode 2: 32 for C <= 16 too)
        runs = []
        if lib.cml_multinomial_supported(d, code, C) > 0:
            runs.append(("valu", lambda: glm_ops.multinomial_grad(x, d, y, coef, prefer_valu=True)))
        cp = lib.cml_multinomial_mfma_supported(d, code, C)
        if cp > 0:  # both MFMA forms (mode 0, the first, is the default route)
            dp = lib.cml_multinomial_mfma_dpad(d, C)
            for mode, name in ((0, "mfma-bf16x3"), (2, "mfma-bf16x3-regsplit")):
                if code == 3 and mode == 2:  # (e4m3 rows: the default split only)
                    continue
                runs.append((name, (lambda m: lambda: _mode_run(m, x, d, y, coef, C, cp, dp))(mode)))
        if not runs:
            runs.append(("torch-chunks", lambda: glm_ops.multinomial_grad(x, d, y, coef)))
        if code == 0 and lib.cml_multinomial_predict_lds(d, 0, C) > 0:  # K13t: transform (raw + probability, f64 [n, C] each)
            ms = best_ms(lambda: glm_ops.multinomial_predict(x, d, coef), reps=3)
            byts = n * d * 2 + 2 * n * C * 8
            print(f"multinomial transform {n}x{d} bf16 C={C:2d} [K13t f64 mfma]: {ms:8.3f} ms, "
                  f"{byts / ms / 1e9:6.2f} TB/s (rows in + raw/prob out)", flush=True)
        for name, fn in runs:
            ms = best_ms(fn, reps=3)
            print(f"multinomial {n}x{d} {a.dtype} C={C:2d} [{name}]: {ms:8.3f} ms, {n * d * esz / ms / 1e9:6.2f} TB/s rows"
                  + (f", {flop / ms / 1e9:7.1f} useful TFLOP/s" if name.startswith("mfma") else ""), flush=True)
        del y


def cmd_silhouette(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import silhouette_ops as SO
    ap = argparse.ArgumentParser(prog="mb_ml.py silhouette")
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--measure", choices=["squaredEuclidean", "cosine", "both"], default="both")
    ap.add_argument("--evaluate", action="store_true", help="also time ClusteringEvaluator.evaluate end to end")
    a = ap.parse_args(argv)
    n, d, k = a.rows, a.dim, a.k
    dt = torch.float8_e4m3fn if a.dtype == "fp8" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(1)
    cen = torch.randn(k, d, generator=g, device="cuda") * 3.0
    true = torch.randint(0, k, (n,), generator=g, device="cuda")
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # blobs in chunks: no n x d f32 temporary
        t = true[s0:s0 + step]
        x[s0:s0 + step] = (cen[t] + torch.randn(len(t), d, generator=g, device="cuda")).to(torch.bfloat16)
    xd = to_device_matrix(x.to(dt) if dt != torch.bfloat16 else x, d)
    del x
    rnd = torch.randint(0, k, (n,), generator=g, device="cuda")
    lab = torch.where(torch.rand(n, generator=g, device="cuda") < 0.9, true, rnd).to(torch.int32)
    del true, rnd
    gb = xd.numel() * xd.element_size() / 1e9
    for measure in (("squaredEuclidean", "cosine") if a.measure == "both" else (a.measure,)):
        cos = measure == "cosine"
        stats, _ = SO.cluster_stats_device(xd, lab, k, None, cos)
        ts = best_ms(lambda: SO.cluster_stats_device(xd, lab, k, None, cos))
        tw = best_ms(lambda: SO.label_wsum(xd, lab, k, None))
        tn = best_ms(lambda: SO.row_sqnorm(xd))
        tsc = best_ms(lambda: SO.silhouette_score(xd, lab, stats, None, cos))
        part = SO.silhouette_score(xd, lab, stats, None, cos)
        flop = 6.0 * n * max(32, xd.shape[1]) * 16 * (-(-k // 16))  # three bf16 MFMA terms per product
        print(f"silhouette {n}x{d} {a.dtype} k={k} {measure}: stats pass {ts:.3f} ms (label_wsum with its sort "
              f"{tw:.3f} ms, row norms {tn:.3f} ms); score pass {tsc:.3f} ms, {gb / tsc:.2f} TB/s rows, "
              f"{flop / tsc / 1e9:.1f} TFLOP/s bf16 MFMA; silhouette {float(part[0] / part[1]):.6f}", flush=True)
    if a.evaluate:
        from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.evaluation import ClusteringEvaluator
        from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
        spark = SparkSession.builder.master("mi355x").getOrCreate()
        df = spark.createDataFrameFromTensors({"features": xd, "prediction": lab})
        for measure in (("squaredEuclidean", "cosine") if a.measure == "both" else (a.measure,)):
            ev = ClusteringEvaluator(distanceMeasure=measure)
            ev.evaluate(df)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = ev.evaluate(df)
            torch.cuda.synchronize()
            print(f"evaluate {n}x{d} {a.dtype} k={k} {measure}: {(time.perf_counter() - t0) * 1e3:.1f} ms end to end, "
                  f"silhouette {v:.6f}", flush=True)


def cmd_bisecting(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import BisectingKMeans
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import bisect_ops as BO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import silhouette_ops as SO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    ap = argparse.ArgumentParser(prog="mb_ml.py bisecting")
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--measure", choices=["euclidean", "cosine"], default="euclidean")
    ap.add_argument("--weighted", action="store_true")
    a = ap.parse_args(argv)
    n, d, k = a.rows, a.dim, a.k
    dt = torch.float8_e4m3fn if a.dtype == "fp8" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(1)
    cen = torch.randn(k, d, generator=g, device="cuda") * 3.0
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # blobs in chunks: no n x d f32 temporary
        t = torch.randint(0, k, (min(step, n - s0),), generator=g, device="cuda")
        x[s0:s0 + step] = (cen[t] + torch.randn(len(t), d, generator=g, device="cuda")).to(torch.bfloat16)
    xd = to_device_matrix(x.to(dt) if dt != torch.bfloat16 else x, d)
    del x
    cols = {"features": xd}
    if a.weighted:
        cols["w"] = torch.randint(0, 4, (n,), generator=g, device="cuda").to(torch.float64)
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    df = spark.createDataFrameFromTensors(cols)
    est = BisectingKMeans(k=k, seed=3, maxIter=a.max_iter, distanceMeasure=a.measure)
    if a.weighted:
        est = est.setWeightCol("w")
    small = spark.createDataFrameFromTensors({c: v[:50_000] for c, v in cols.items()})
    est.fit(small)  # loads the kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = est.fit(df)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0

    def levels(nd):
        return 1 + max((levels(c) for c in nd.children), default=0)
    nlev = levels(m._root) - 1
    iters = nlev * (max(a.max_iter, 1) + 1) + 1  # per level: the iterations and the final assignment; the root
    form = "K27" if BO.kernel_enabled() and BO.kernel_supported(xd.dtype, xd.shape[1]) else "torch"
    print(f"bisecting {n}x{d} {a.dtype} k={k} maxIter={a.max_iter} {a.measure}{' weighted' if a.weighted else ''} "
          f"[{form}]: fit {fit_s:.3f} s, {len(m.clusterCenters())} leaves on {nlev} levels, "
          f"{1e3 * fit_s / iters:.2f} ms per pass ({iters} passes), trainingCost {m.trainingCost:.6e}", flush=True)
    if form == "K27":  # the step alone: every row listed (level 1), two live children
        cosine = a.measure == "cosine"
        plan = BO.make_plan(torch.zeros(n, dtype=torch.int64, device="cuda"), 1)
        c0 = torch.as_tensor(m._root.center, device="cuda")
        ch = torch.zeros(1, 2, xd.shape[1], dtype=torch.float64, device="cuda")
        ch[0, 0, :d], ch[0, 1, :d] = c0 * 0.999, c0 * 1.001
        alive = torch.ones(1, 2, dtype=torch.bool, device="cuda")
        w = cols.get("w")
        nrm2 = SO.row_sqnorm(xd)
        omega = (w if not cosine else (torch.reciprocal(nrm2.sqrt()) if w is None else w / nrm2.sqrt()))
        for sums in (True, False):
            ms = best_ms(lambda: BO.bisect_step(xd, plan, ch, alive, omega, w, None if cosine else nrm2, cosine, sums))
            gb = xd.numel() * xd.element_size() / 1e9
            print(f"  bisect_step want_sums={int(sums)}: {ms:.3f} ms, {gb / ms:.2f} TB/s rows", flush=True)


def cmd_gmm(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import gmm as G
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import GaussianMixture
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import gmm_ops as GO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    ap = argparse.ArgumentParser(prog="mb_ml.py gmm")
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--form", choices=["kernel", "reference", "dense"], default="kernel")
    a = ap.parse_args(argv)
    n, d, k = a.rows, a.dim, a.k
    os.environ["CML_GMM_KERNEL"] = "1" if a.form == "kernel" else "0"
    g = torch.Generator(device="cuda").manual_seed(1)
    cen = torch.randn(k, d, generator=g, device="cuda") * 1.5
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # overlapping blobs in chunks: no n x d f32 temporary
        t = torch.randint(0, k, (min(step, n - s0),), generator=g, device="cuda")
        x[s0:s0 + step] = (cen[t] + torch.randn(len(t), d, generator=g, device="cuda")).to(torch.bfloat16)
    xd = to_device_matrix(x, d)
    del x
    # dense: an f64 copy of the same values, the dense path's column (its conversion is not timed)
    feats = xd[:, :d].to(torch.float64) if a.form == "dense" else xd
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    df = spark.createDataFrameFromTensors({"features": feats})
    est = GaussianMixture(k=k, seed=3, maxIter=a.max_iter, tol=0.0)
    est.fit(spark.createDataFrameFromTensors({"features": feats[:50_000]}))  # loads the kernels
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    m = est.fit(df)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    rise = torch.cuda.max_memory_allocated() - base
    xbytes = xd.numel() * xd.element_size()
    its = m.summary.numIter
    print(f"gmm {n}x{d} bf16 k={k} maxIter={a.max_iter} [{a.form}]: fit {fit_s:.3f} s, {its} iterations, "
          f"{1e3 * fit_s / max(its, 1):.2f} ms per iteration, logLikelihood {m.summary.logLikelihood:.9e}, "
          f"peak rise {rise / 2**20:.0f} MiB = {rise / xbytes:.2f} x the bf16 rows", flush=True)
    if a.form == "kernel" and GO.kernel_supported(xd.dtype, xd.shape[1], k):
        A, c = G._estep_tables(m._w, m._cov)
        ms = best_ms(lambda: GO.estep(xd, d, None, A, m._mu, c))
        dp = xd.shape[1]
        flops = 2.0 * n * k * dp * dp * (0.75 if dp == 32 else 1.0) * 2  # MFMAs issued: both phases, lower blocks
        print(f"  estep alone: {ms:.3f} ms, {flops / ms / 1e9:.1f} TF/s f64 issued "
              f"({4.0 * n * k * d * d / ms / 1e9:.1f} TF/s of 4 n k d^2), {xbytes / ms / 1e9:.3f} TB/s rows",
              flush=True)
        ms = best_ms(lambda: GO.predict(xd, d, A, m._mu, c))
        print(f"  predict alone: {ms:.3f} ms ({n * k * 8 / ms / 1e9:.2f} TB/s of prob written)", flush=True)


def cmd_lda(argv):
    import numpy as np
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import lda as L
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.clustering import LDA
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import lda_ops as LO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.utils import rng as R
    ap = argparse.ArgumentParser(prog="mb_ml.py lda")
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--subsampling", type=float, default=0.05)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--length", type=float, default=100.0, help="mean tokens per document")
    ap.add_argument("--form", choices=["kernel", "reference", "dense"], default="kernel")
    a = ap.parse_args(argv)
    n, V, k = a.rows, a.terms, a.k
    os.environ["CML_LDA_KERNEL"] = "1" if a.form == "kernel" else "0"
    g = torch.Generator(device="cuda").manual_seed(1)
    # planted topics ~ Dirichlet(0.1), document mixtures ~ Dirichlet(0.3) (normalised Gamma draws); the counts
    # of a document are Poisson(length * p_w), in chunks: no n x V f32 temporary
    conc = torch.distributions.Gamma(torch.tensor(0.1, device="cuda"), torch.tensor(1.0, device="cuda"))
    torch.manual_seed(1)
    topics = conc.sample((k, V)) + 1e-30
    topics = topics / topics.sum(1, keepdim=True)
    mixc = torch.distributions.Gamma(torch.tensor(0.3, device="cuda"), torch.tensor(1.0, device="cuda"))
    x = torch.empty(n, V, dtype=torch.bfloat16, device="cuda")
    step = 1 << 20
    for s0 in range(0, n, step):
        m = min(step, n - s0)
        th = mixc.sample((m, k)) + 1e-30
        p = (th / th.sum(1, keepdim=True)) @ topics
        x[s0:s0 + m] = torch.poisson(p * a.length, generator=g).clamp(max=256.0).to(torch.bfloat16)
    xd = to_device_matrix(x, V)
    del x
    # dense: an f64 copy of the same values, the dense path's column (its conversion is not timed)
    feats = xd[:, :V].to(torch.float64) if a.form == "dense" else xd
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    df = spark.createDataFrameFromTensors({"features": feats})
    est = LDA(k=k, seed=3, maxIter=a.max_iter, subsamplingRate=a.subsampling)
    est.fit(spark.createDataFrameFromTensors({"features": feats[:50_000]}))  # loads the kernels
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    m = est.fit(df)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    rise = torch.cuda.max_memory_allocated() - base
    xbytes = xd.numel() * xd.element_size()
    print(f"lda {n}x{V} bf16 k={k} subsampling={a.subsampling} maxIter={a.max_iter} [{a.form}]: fit {fit_s:.3f} s, "
          f"{1e3 * fit_s / max(a.max_iter, 1):.2f} ms per iteration, alpha[0] {m.estimatedDocConcentration()[0]:.9e}, "
          f"peak rise {rise / 2**20:.0f} MiB = {rise / xbytes:.2f} x the bf16 rows", flush=True)
    dp = xd.shape[1]
    if a.form == "kernel" and LO.kernel_supported(xd.dtype, dp, k):
        # the E-step alone on the last iteration's mini-batch with the fitted topics
        ids = df._row_ids
        rows = torch.nonzero((LO.row_sums(xd, V) > 0) & (R.uniform(ids, 3, 1_000_003 + a.max_iter) < a.subsampling))
        rows = rows.reshape(-1)
        lam = torch.as_tensor(m._topics.T, device="cuda")
        e_beta = torch.exp(L.dirichlet_expectation(lam))
        alpha = torch.as_tensor(m._alpha, device="cuda")
        g0 = L._gamma_init(ids[rows], k, 3)
        out = []
        ms = best_ms(lambda: out.append(LO.estep(xd, rows, V, e_beta, alpha, g0)), reps=3)
        sw = out[-1][3].to(torch.float64)
        nb = int(rows.shape[0])
        pad = (-nb) % 16
        grp = torch.cat([sw, torch.zeros(pad, dtype=sw.dtype, device=sw.device)]).reshape(-1, 16).max(1).values
        kp = 16 if k <= 16 else 32
        per_block = (kp // 2) * 2048.0  # f64 flops of the MFMAs issued per 16 documents x 16 terms, either phase
        flops = (float(grp.sum()) + 4.0 * ((nb + 63) // 64)) * (dp // 16) * per_block
        q = np.percentile(sw.cpu().numpy(), [0, 50, 99, 100])
        print(f"  estep alone on {nb} documents: {ms:.3f} ms, {flops / ms / 1e9:.2f} TF/s f64 MFMA issued, "
              f"{nb * dp * 2 / ms / 1e9:.4f} TB/s rows", flush=True)
        print(f"  sweeps min / median / p99 / max = {q[0]:.0f} / {q[1]:.0f} / {q[2]:.0f} / {q[3]:.0f}, mean "
              f"{float(sw.mean()):.1f}; mean over 16-document groups of the group's maximum / mean sweeps = "
              f"{float(grp.mean()) / float(sw.mean()):.2f}", flush=True)


def cmd_mlp(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification_more import (
        MultilayerPerceptronClassifier)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import mlp_ops as MO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    ap = argparse.ArgumentParser(prog="mb_ml.py mlp")
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--layers", default="64,16,4")
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--form", choices=["kernel", "reference", "dense"], default="kernel")
    ap.add_argument("--pass-only", action="store_true", help="no fit: one loss + gradient pass of the kernel")
    a = ap.parse_args(argv)
    layers = [int(v) for v in a.layers.split(",")]
    n, d, C = a.rows, layers[0], layers[-1]
    os.environ["CML_MLP_KERNEL"] = "1" if a.form == "kernel" else "0"
    g = torch.Generator(device="cuda").manual_seed(1)
    w = torch.randn(d, C, generator=g, device="cuda")
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # a planted linear rule with noise, in chunks: no n x d f32 temporary
        v = torch.randn(min(step, n - s0), d, generator=g, device="cuda")
        x[s0:s0 + step] = v.to(torch.bfloat16)
        y[s0:s0 + step] = torch.argmax(v @ w + 0.5 * torch.randn(len(v), C, generator=g, device="cuda"), 1)
        del v
    xd = to_device_matrix(x, d)
    del x
    xbytes = xd.numel() * xd.element_size()

    def kernel_alone(p):
        y32 = y.to(torch.int32)
        ms = best_ms(lambda: MO.loss_grad(xd, d, y32, layers, p))
        nl, t = len(layers) - 1, 1 if max(layers[1:]) <= 16 else 2
        # MFMAs issued per 64-row tile: layer 1 forward and dW_1 16 t dp/16 each; per upper layer the forward
        # and backward 16 t^2 each and the 16 of each of its t^2 gradient blocks
        flops = ((n + 63) // 64) * (2 * 16 * t * (xd.shape[1] // 16) + (nl - 1) * 48 * t * t) * 2048.0
        print(f"  loss_grad alone at {n}x{d} {layers}: {ms:.3f} ms, {flops / ms / 1e9:.2f} TF/s f64 MFMA issued, "
              f"{xbytes / ms / 1e9:.3f} TB/s rows", flush=True)
        ms = best_ms(lambda: MO.forward(xd, d, layers, p))
        print(f"  forward alone: {ms:.3f} ms ({n * C * 8 / ms / 1e9:.2f} TB/s of scores written)", flush=True)

    if a.pass_only:
        import numpy as np
        rs = np.random.RandomState(3)
        kernel_alone(torch.as_tensor(np.concatenate([rs.uniform(-1, 1, i * o + o) * np.sqrt(6.0 / (i + o))
                                                     for i, o in zip(layers[:-1], layers[1:])]), device="cuda"))
        return
    # dense: an f64 copy of the same values, the dense path's column (its conversion is not timed)
    feats = xd[:, :d].to(torch.float64) if a.form == "dense" else xd
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    df = spark.createDataFrameFromTensors({"features": feats, "label": y})
    est = MultilayerPerceptronClassifier(layers=layers, seed=3, maxIter=a.max_iter, tol=0.0)
    est.fit(spark.createDataFrameFromTensors({"features": feats[:50_000], "label": y[:50_000]}))  # loads the kernels
    evals = []
    real, real_ref = MO.loss_grad, MO.loss_grad_reference
    MO.loss_grad = lambda *aa, **kk: (evals.append(1), real(*aa, **kk))[1]
    MO.loss_grad_reference = lambda *aa, **kk: (evals.append(1), real_ref(*aa, **kk))[1]
    real_grad = torch.autograd.grad  # the dense form's evaluations
    torch.autograd.grad = lambda *aa, **kk: (evals.append(1), real_grad(*aa, **kk))[1]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    m = est.fit(df)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    MO.loss_grad, MO.loss_grad_reference, torch.autograd.grad = real, real_ref, real_grad
    rise = torch.cuda.max_memory_allocated() - base
    hist = m.summary.objectiveHistory
    ne = len(evals) if evals else None
    per = f", {ne} evaluations, {1e3 * fit_s / ne:.2f} ms per evaluation" if ne else ""
    print(f"mlp {n}x{d} bf16 layers={layers} maxIter={a.max_iter} [{a.form}]: fit {fit_s:.3f} s, "
          f"{m.summary.totalIterations} iterations{per}, final loss {hist[-1]:.12e}, peak rise {rise / 2**20:.0f} MiB = {rise / xbytes:.2f} x the bf16 rows",
          flush=True)
    if a.form == "kernel" and MO.kernel_supported(xd.dtype, xd.shape[1], layers):
        kernel_alone(torch.as_tensor(m.weights.toArray(), device="cuda"))


def cmd_fm(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import fm as FM
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import FMRegressor
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import fm_ops as FO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    ap = argparse.ArgumentParser(prog="mb_ml.py fm")
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--factor-size", type=int, default=8)
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--loss", choices=["squared", "logistic"], default="squared")
    ap.add_argument("--pass-only", action="store_true", help="K32 alone (sizes at which the dense form does not fit)")
    a = ap.parse_args(argv)
    n, d, f = a.rows, a.dim, a.factor_size
    g = torch.Generator(device="cuda").manual_seed(1)
    w = torch.randn(d, generator=g, device="cuda") / d ** 0.5
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # a planted linear rule with noise, in chunks: no n x d f32 temporary
        v = torch.randn(min(step, n - s0), d, generator=g, device="cuda")
        x[s0:s0 + step] = v.to(torch.bfloat16)
        y[s0:s0 + step] = v @ w + 0.5 * torch.randn(len(v), generator=g, device="cuda")
        del v
    if a.loss == "logistic":
        y = (y > 0).to(torch.float64)
    xd = to_device_matrix(x, d)
    del x
    dp = int(xd.shape[1])
    xbytes = xd.numel() * xd.element_size()
    import numpy as np
    rs = np.random.RandomState(3)
    p = torch.as_tensor(np.concatenate([[0.3], rs.randn(d) / np.sqrt(d), 0.5 * rs.randn(d * f) / np.sqrt(d)]),
                        device="cuda")
    hp = 16 if f <= 15 else 32
    # MFMAs issued per 64-row tile: the forward and the blocks of dP, hp / 16 * dp / 16 * 16 each
    flops = ((n + 63) // 64) * 2 * 16 * (hp // 16) * (dp // 16) * 2048.0

    def timed(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base, out

    FO.loss_grad(xd[:4096], None, d, y[:4096], p, f, a.loss)  # loads the kernels
    if a.pass_only:
        ms = best_ms(lambda: FO.loss_grad(xd, None, d, y, p, f, a.loss), reps=3)
        print(f"K32 loss_grad at {n}x{d} bf16 factorSize={f} {a.loss}: {ms:.2f} ms, {flops / ms / 1e9:.2f} TF/s f64 MFMA "
              f"issued, {xbytes / ms / 1e9:.3f} TB/s rows", flush=True)
        ms = best_ms(lambda: FO.scores(xd, d, p, f), reps=3)
        print(f"K32 scores: {ms:.2f} ms, {xbytes / ms / 1e9:.3f} TB/s rows", flush=True)
        return
    x64 = xd[:, :d].to(torch.float64)  # the dense form's column (its conversion is not timed)

    def dense():
        pt = p.clone().requires_grad_(True)
        s = FM._fm_scores(x64, pt[0], pt[1:1 + d], pt[1 + d:].reshape(d, f))
        loss = (torch.nn.functional.softplus(s) - y * s).sum() if a.loss == "logistic" else 0.5 * ((s - y) ** 2).sum()
        grad, = torch.autograd.grad(loss, pt)
        return torch.cat([grad, loss.detach().reshape(1)])

    forms = {"kernel": lambda: FO.loss_grad(xd, None, d, y, p, f, a.loss),
             "reference": lambda: FO.loss_grad_reference(xd, None, d, y, p, f, a.loss), "dense": dense}
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    frames = {"kernel": spark.createDataFrameFromTensors({"features": xd[:, :d], "label": y}),
              "dense": spark.createDataFrameFromTensors({"features": x64, "label": y})}
    frames["reference"] = frames["kernel"]
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import FMClassifier
    est = (FMClassifier if a.loss == "logistic" else FMRegressor)(factorSize=f, seed=3, maxIter=a.max_iter, tol=0.0,
                                                                   stepSize=0.05)
    want = None
    for r in range(a.rounds):
        for name, fn in forms.items():
            fn()
            s, rise, out = timed(fn)
            want = out if want is None else want
            print(f"round {r} fm {n}x{d} factorSize={f} {a.loss} one iteration [{name}]: {1e3 * s:.2f} ms, peak rise "
                  f"{rise / 2**20:.0f} MiB = {rise / xbytes:.2f} x the bf16 rows, max rel diff to the first "
                  f"{float(((out - want).abs() / want.abs().clamp(min=1e-300)).max()):.2e}", flush=True)
            del out
        for name in forms:
            os.environ["CML_FM_KERNEL"] = "1" if name == "kernel" else "0"
            s, rise, m = timed(lambda: est.fit(frames[name]))
            print(f"round {r} fm {n}x{d} factorSize={f} {a.loss} fit maxIter={a.max_iter} [{name}]: {s:.3f} s, final "
                  f"loss {m._hist[-1]:.12e}, peak rise {rise / 2**20:.0f} MiB = {rise / xbytes:.2f} x the bf16 rows",
                  flush=True)
    os.environ.pop("CML_FM_KERNEL", None)
    ms = best_ms(forms["kernel"], reps=3)
    print(f"K32 loss_grad alone: {ms:.2f} ms, {flops / ms / 1e9:.2f} TF/s f64 MFMA issued, {xbytes / ms / 1e9:.3f} TB/s "
          f"rows", flush=True)
    ms = best_ms(lambda: FO.scores(xd, d, p, f), reps=3)
    print(f"K32 scores alone: {ms:.2f} ms, {xbytes / ms / 1e9:.3f} TB/s rows", flush=True)


def cmd_gram(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.feature_extra import PCA
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.regression import (
        GeneralizedLinearRegression, LinearRegression)
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import gram_ops as GO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    ap = argparse.ArgumentParser(prog="mb_ml.py gram")
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pass-only", action="store_true", help="K31 alone (sizes at which the dense form does not fit)")
    ap.add_argument("--fits", action="store_true", help="also PCA, LinearRegression and a 5-step poisson GLR fit")
    a = ap.parse_args(argv)
    n, d = a.rows, a.dim
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # in chunks: no n x d f32 temporary
        x[s0:s0 + step] = torch.randn(min(step, n - s0), d, generator=g, device="cuda").to(torch.bfloat16)
    z = torch.randn(n, generator=g, device="cuda", dtype=torch.float64)
    w = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    xbytes = x.numel() * x.element_size()
    nt = (d + 15) // 16
    flops = 512.0 * ((nt + 1) * (nt + 2) // 2) * n  # 16 x 16 x 4 MFMAs of the upper triangle of (NT + 1)^2 blocks

    def dense(xx, dd, y, weight=None):  # the form before K31: an n x (d + 2) f64 copy (two with weights)
        aa = torch.cat([xx[:, :dd].to(torch.float64), torch.ones((xx.shape[0], 1), dtype=torch.float64, device=xx.device),
                        y.to(torch.float64).reshape(-1, 1)], 1)
        if weight is not None:
            aa = aa * weight.to(torch.float64).sqrt().reshape(-1, 1)
        return aa.T @ aa

    def timed(fn, reps=1):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, torch.cuda.max_memory_allocated() - base, out

    GO.gram(x[:4096], d, z[:4096], w[:4096])  # loads the kernels
    if a.pass_only:
        for wt in (None, w):
            ms = best_ms(lambda: GO.gram(x, d, z, wt), reps=3)
            print(f"K31 at {n}x{d} bf16{' weighted' if wt is not None else ''}: {ms:.2f} ms, "
                  f"{flops / ms / 1e9:.2f} TF/s f64 MFMA, {xbytes / ms / 1e9:.3f} TB/s rows", flush=True)
        return
    forms = {"kernel": GO.gram, "reference": GO.gram_reference, "dense": dense}
    for fn in forms.values():
        fn(x[:100_000], d, z[:100_000], w[:100_000])
    want = None
    for r in range(a.rounds):
        for name, fn in forms.items():
            s, rise, G = timed(lambda: fn(x, d, z, w))
            want = G if want is None else want
            print(f"round {r} gram {n}x{d} weighted [{name}]: {1e3 * s:.2f} ms, peak rise {rise / 2**20:.0f} MiB = "
                  f"{rise / xbytes:.2f} x the bf16 rows, max rel diff to the first "
                  f"{float(((G - want).abs() / want.abs().clamp(min=1e-300)).max()):.2e}", flush=True)
            del G
    if not a.fits:
        return
    spark = SparkSession.builder.master("mi355x").getOrCreate()
    cnt = torch.poisson(torch.exp(0.3 * x[:, :4].to(torch.float64).sum(1))).to(torch.float64)
    df = spark.createDataFrameFromTensors({"features": x, "label": z, "count": cnt})
    small = spark.createDataFrameFromTensors({"features": x[:50_000], "label": z[:50_000], "count": cnt[:50_000]})
    fits = {"PCA(k=8)": lambda f: PCA(k=8, inputCol="features", outputCol="p").fit(f),
            "LinearRegression(normal)": lambda f: LinearRegression(solver="normal", regParam=0.1).fit(f),
            "GLR(poisson, 5 steps)": lambda f: GeneralizedLinearRegression(labelCol="count", family="poisson", maxIter=5,
                                                                           tol=0.0).fit(f)}
    real = glm_ops.gram
    for r in range(a.rounds):
        for form in ("kernel", "reference", "dense"):
            os.environ["CML_GRAM_KERNEL"] = "1" if form == "kernel" else "0"
            glm_ops.gram = dense if form == "dense" else real
            try:
                for name, fit in fits.items():
                    fit(small)
                    s, rise, _ = timed(lambda: fit(df))
                    print(f"round {r} {name} {n}x{d} [{form}]: fit {s:.3f} s, peak rise {rise / 2**20:.0f} MiB",
                          flush=True)
            finally:
                glm_ops.gram = real
    os.environ.pop("CML_GRAM_KERNEL", None)


def cmd_glr_step(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml import glr as GLR
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import glr_ops as GO
    ap = argparse.ArgumentParser(prog="mb_ml.py glr_step")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args(argv)
    n, d = a.rows, a.dim
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # in chunks: no n x d f32 temporary
        x[s0:s0 + step] = torch.randn(min(step, n - s0), d, generator=g, device="cuda").to(torch.bfloat16)
    coef = torch.cat([0.3 * torch.randn(d, generator=g, device="cuda", dtype=torch.float64) / d ** 0.5,
                      torch.ones(1, dtype=torch.float64, device="cuda")])
    y = torch.poisson(torch.exp(glm_ops.linear_predict(x, d, coef)))
    w = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    xd = to_device_matrix(x, d)
    spec = GO.spec("tweedie", None, 1.0, 0.0)
    xbytes = x.numel() * x.element_size()

    def fused():
        return GO.step(xd, d, y, w, None, coef, spec, False)

    def loop():  # one iteration of ml/glr.py's loop for family="poisson": eta, mu, z, wt, then the Gram
        eta = glm_ops.linear_predict(x, d, coef)
        mu = GLR._project("poisson", GLR._unlink("log", eta))
        dmu = GLR._deriv("log", mu)
        z = eta + (y - mu) * dmu
        wt = w / (dmu * dmu * GLR._variance("poisson", mu))
        return glm_ops.gram(x, d, z, wt)

    # bytes: K33 reads the rows once and y, w; the loop reads the rows twice and writes / reads the n-vectors of its
    # 9 element-wise kernels (3 with one operand, 6 with two, one result each: 24 vector passes) besides K24's eta and
    # K31's z, wt
    fused_bytes = xbytes + 2 * 8 * n
    loop_bytes = 2 * xbytes + (1 + 24 + 2) * 8 * n
    Gf, Gl = fused()[0], loop()
    print(f"max rel diff of G between the two forms: "
          f"{float(((Gf - Gl).abs() / Gl.abs().clamp(min=1e-300)).max()):.2e}", flush=True)
    for r in range(a.rounds):
        for name, fn, nbytes in (("K33 step", fused, fused_bytes), ("K24 + torch + K31", loop, loop_bytes)):
            ms = best_ms(fn, reps=3)
            print(f"round {r} glr step {n}x{d} bf16 [{name}]: {ms:.2f} ms, {nbytes / 1e9:.2f} GB, "
                  f"{nbytes / ms / 1e9:.3f} TB/s ({xbytes / ms / 1e9:.3f} TB/s counting the rows once)", flush=True)


def cmd_nb(argv):
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification import NaiveBayes
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import nb_ops as NO
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.sql import SparkSession
    ap = argparse.ArgumentParser(prog="mb_ml.py nb")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 16])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--ops-only", action="store_true", help="time the two passes alone, not the estimator")
    ap.add_argument("--dense-limit-gb", type=float, default=24.0,
                    help="skip a dense-form step whose largest f64 temporary would pass this size")
    a = ap.parse_args(argv)
    n, d = a.rows, a.dim
    spark = SparkSession({"spark.master": "mi355x", "spark.app.name": "mb-nb"})
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
    step = 1 << 22
    for s0 in range(0, n, step):  # counts 0 .. 8 in chunks: exact in bf16, and valid for every model type but bernoulli
        x[s0:s0 + step] = torch.randint(0, 9, (min(step, n - s0), d), generator=g, device="cuda").to(torch.bfloat16)
    xd = to_device_matrix(x, d)
    xbytes = x.numel() * x.element_size()

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    for C in a.classes:
        y = torch.randint(0, C, (n,), generator=g, device="cuda").to(torch.float64)
        lab = y.to(torch.int32)
        shift = torch.rand(C, d, generator=g, device="cuda", dtype=torch.float64) * 8.0
        W = torch.randn(C, d, generator=g, device="cuda", dtype=torch.float64) * 0.05
        b = torch.zeros(C, dtype=torch.float64, device="cuda")
        iv = torch.full((C, d), 0.2 / d, dtype=torch.float64, device="cuda")
        ops = (("moments, pass 1", lambda: NO.moments(xd, d, lab, None, C, None, False),
                lambda: NO.moments_reference(x, d, lab, None, C), xbytes + 4 * n),
               ("moments, pass 2 (shift, second)", lambda: NO.moments(xd, d, lab, None, C, shift, True),
                lambda: NO.moments_reference(x, d, lab, None, C, shift), xbytes + 4 * n),
               ("scores, linear", lambda: NO.scores(xd, d, "linear", W, b),
                lambda: NO.scores_reference(x, d, "linear", W, b), xbytes + (2 * C + 1) * 8 * n),
               ("scores, gaussian", lambda: NO.scores(xd, d, "gaussian", shift, b, iv),
                lambda: NO.scores_reference(x, d, "gaussian", shift, b, iv), xbytes + (2 * C + 1) * 8 * n))
        for name, kern, ref, nbytes in ops:
            for r in range(a.rounds):
                km, rm = best_ms(kern, reps=3), best_ms(ref, reps=2)
                print(f"round {r} nb {n}x{d} bf16 C={C} [{name}]: K34 {km:.2f} ms ({nbytes / 1e9:.2f} GB, "
                      f"{nbytes / km / 1e9:.3f} TB/s), reference form {rm:.2f} ms", flush=True)
        if a.ops_only:
            continue
        frames = {"bf16": spark.createDataFrameFromTensors({"features": x, "label": y}),
                  "f32": None}
        for mt in ("multinomial", "gaussian"):
            for r in range(a.rounds):
                for form in ("kernel", "reference", "dense f32"):
                    os.environ["CML_NB_KERNEL"] = "0" if form == "reference" else "1"
                    if form == "dense f32":
                        if 4 * n * d * 8 / 1e9 > a.dense_limit_gb:
                            print(f"round {r} nb {mt} C={C} [{form}]: skipped (fit temporaries)", flush=True)
                            continue
                        if frames["f32"] is None:
                            frames["f32"] = spark.createDataFrameFromTensors({"features": x.to(torch.float32),
                                                                              "label": y})
                    df = frames["f32" if form == "dense f32" else "bf16"]
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    fit_ms, m = wall(lambda: NaiveBayes(modelType=mt).fit(df))
                    rise = torch.cuda.max_memory_allocated() - base
                    if form == "dense f32" and mt == "gaussian" and n * C * d * 8 / 1e9 > a.dense_limit_gb:
                        tr = "transform skipped (n x C x d f64)"
                    else:
                        tr_ms, out = wall(lambda: m.transform(df)._column_data("prediction").values)
                        tr = f"transform {tr_ms:.1f} ms"
                        del out
                    print(f"round {r} nb {mt} {n}x{d} C={C} [{form}]: fit {fit_ms:.1f} ms "
                          f"(peak rise {rise / xbytes:.2f} x the bf16 rows), {tr}", flush=True)
        os.environ.pop("CML_NB_KERNEL", None)
        del frames
    spark.stop()


def cmd_aft(argv):
    import math

    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import to_device_matrix
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import aft_ops as AO
    ap = argparse.ArgumentParser(prog="mb_ml.py aft")
    ap.add_argument("--shapes", nargs="+", default=["10000000x64", "4000000x256"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dense-limit-gb", type=float, default=24.0, help="skip the dense form above this f64 copy")
    a = ap.parse_args(argv)
    copy_rate = 6.3e12  # B/s, the copy rate PARITY.md measures against
    for shape in a.shapes:
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.empty(n, d, dtype=torch.bfloat16, device="cuda")
        step = 1 << 22
        for s0 in range(0, n, step):  # in chunks: no n x d f32 temporary
            x[s0:s0 + step] = torch.randn(min(step, n - s0), d, generator=g, device="cuda").to(torch.bfloat16)
        beta = 0.3 * torch.randn(d, generator=g, device="cuda", dtype=torch.float64) / d ** 0.5
        ls = math.log(0.9)
        coef = torch.cat([beta, torch.tensor([0.8, ls], dtype=torch.float64, device="cuda")])
        logt = AO.rows_reference(x, d, coef) - 0.8 + 0.7 * torch.log(
            -torch.log1p(-torch.rand(n, generator=g, device="cuda", dtype=torch.float64)))
        delta = (torch.rand(n, generator=g, device="cuda") < 0.7).to(torch.float64)
        xd = to_device_matrix(x, d)
        xbytes = x.numel() * x.element_size()
        x64 = x.to(torch.float64) if 8 * n * d / 1e9 <= a.dense_limit_gb else None

        def dense():  # fg of the f32 / f64 columns in ml/regression_more.py
            sigma = math.exp(ls)
            m = x64 @ beta + 0.8
            eps = (logt - m) / sigma
            ee = torch.exp(eps)
            loss = (delta * ls - delta * eps + ee).sum()
            r = (delta - ee) / sigma
            return torch.cat([x64.T @ r, r.sum().reshape(1), (delta + (delta - ee) * eps).sum().reshape(1),
                              loss.reshape(1)])

        # bytes: K35 and the reference form read the rows once and logt, delta; the dense form reads its f64 copy twice
        # and the n-vectors of its 11 element-wise and 3 sum kernels (34 vector passes) besides the two GEMVs' m and r
        forms = [("K35 loss_grad", lambda: AO.loss_grad(xd, d, logt, delta, coef), xbytes + 16 * n),
                 ("reference form", lambda: AO.loss_grad_reference(x, d, logt, delta, coef), xbytes + 16 * n)]
        if x64 is not None:
            forms.append(("dense f64", dense, 2 * 8 * n * d + (34 + 2) * 8 * n))
            ref = dense()
            got = forms[0][1]()
            print(f"aft {n}x{d}: max rel diff of the message, K35 vs dense: "
                  f"{float(((got - ref).abs() / ref.abs().clamp(min=1e-300)).max()):.2e}", flush=True)
        forms.append(("K35 rows, eta only", lambda: AO.rows(xd, d, coef), xbytes + 8 * n))
        forms.append(("K35 rows with terms", lambda: AO.rows(xd, d, coef, logt, delta), xbytes + 48 * n))
        for r in range(a.rounds):
            for name, fn, nbytes in forms:
                ms = best_ms(fn, reps=3)
                print(f"round {r} aft {n}x{d} bf16 [{name}]: {ms:.2f} ms, {nbytes / 1e9:.2f} GB, "
                      f"{nbytes / ms / 1e9:.3f} TB/s = {100 * nbytes / (ms * 1e-3) / copy_rate:.0f} % of the copy rate "
                      f"(floor {1e3 * nbytes / copy_rate:.2f} ms)", flush=True)
        del x, xd, x64, logt, delta, forms


COMMANDS = {"aft": cmd_aft, "nb": cmd_nb, "glr_step": cmd_glr_step, "fm": cmd_fm, "gram": cmd_gram, "mlp": cmd_mlp, "lda": cmd_lda, "gmm": cmd_gmm, "bisecting": cmd_bisecting, "silhouette": cmd_silhouette,"multinomial": cmd_multinomial, "glm": cmd_glm, "glm-fp8": cmd_glm_fp8, "logreg": cmd_logreg, "trees": cmd_trees,
            "tree-transform": cmd_tree_transform}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in COMMANDS:
        print(__doc__)
        sys.exit(2)
    COMMANDS[sys.argv[1]](sys.argv[2:])
