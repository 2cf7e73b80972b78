"""The route of a LloydEngine — which precision, pruning, sums and step its constructor arguments end in — as
a table: models/kmeans_route.resolve_route against tests/golden/kmeans_routes.json, the decisions the engine's
constructor took at the commit before it was split up (recorded by driving that constructor itself; rows it
rejected hold the exception's message). On a GPU, real engines are checked against the same lines."""
import json
import os

import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans_route import Route, resolve_route

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "kmeans_routes.json"), encoding="utf-8") as _fh:
    TABLE = json.load(_fh)
DTYPES = {"host": torch.float64, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn, "f32": torch.float32,
          "f64": torch.float64}
ARGS = dict(incremental=None, use_graph=None, row_chunks=None, accum_mode=None, refresh_interval=None)


def _lines():
    for row in TABLE["rows"]:
        line = dict(zip(TABLE["inputs"], row))
        line["want"], line["dd_calls"] = row[len(TABLE["inputs"])], row[len(TABLE["inputs"]) + 1]
        yield line


def test_table_covers_the_cross_product():
    assert TABLE["fields"] == [f.name for f in Route.__dataclass_fields__.values()]
    plain = {(ln["rows"], ln["streamed"], ln["weights"], ln["spherical"], ln["precision"], ln["prune"])
             for ln in _lines() if not ln["env"] and not ln["args"]}
    # every constructible combination (streamed rows are host rows by definition)
    assert len(plain) == (5 + 1) * 2 * 2 * 5 * 3
    assert {ln["screen_ok"] for ln in _lines() if ln["rows"] in ("f32", "f64")} == {True, False}
    knobs = {(k, v) for ln in _lines() for k, v in ln["env"].items()}
    assert {("CML_KMEANS_SCREEN", "0"), ("CML_KMEANS_PRUNE", "0"), ("CML_KMEANS_PRUNE", "1"),
            ("CML_KMEANS_PRECISION", "bf16"), ("CML_KMEANS_GRAPH", "1"), ("CML_KMEANS_REFRESH", "3")} <= knobs
    assert any(not ln["dd_exact"] and ln["dd_calls"] for ln in _lines())


def test_resolve_route_equals_the_recorded_constructor():
    for ln in _lines():
        calls = []

        def dd_exact():
            calls.append(1)
            return ln["dd_exact"]
        kw = dict(ARGS, **ln["args"])
        kw.update(on_device=ln["rows"] != "host", dtype=DTYPES[ln["rows"]], streamed=ln["streamed"],
                  weighted=ln["weights"], spherical=ln["spherical"], precision=ln["precision"], prune=ln["prune"],
                  screen_ok=ln["screen_ok"], dd_exact=dd_exact, env=ln["env"])
        if isinstance(ln["want"], str):
            with pytest.raises(ValueError) as err:
                resolve_route(**kw)
            assert str(err.value) == ln["want"], ln
        else:
            got = resolve_route(**kw)
            for name, want in zip(TABLE["fields"], ln["want"]):
                assert getattr(got, name) == want and type(getattr(got, name)) is type(want), (name, ln)
        assert len(calls) == ln["dd_calls"], ln  # dd_sums_exact is a collective: the same calls, no more


@pytest.mark.gpu
def test_real_engines_take_the_recorded_routes(monkeypatch):
    """Engines on device rows (n = 64, d = 8, k = 4, where no K9r plan exists: the lines with screen_ok false),
    and one f32 engine at d = 128, k = 8, where the screen applies."""
    from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import LloydEngine
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    base = torch.randn(64, 8, generator=g, dtype=torch.float64)
    w = (torch.rand(64, generator=g, dtype=torch.float64) + 0.5).to(dev)
    data = {r: base.to(dev).to(torch.float32).to(DTYPES[r]) if r != "f64" else base.to(dev)
            for r in ("bf16", "e4m3", "f32", "f64")}
    assert not LloydEngine.screen_applies(8, 4) and LloydEngine.screen_applies(128, 8)
    checked = 0
    for ln in _lines():
        if ln["rows"] == "host" or ln["streamed"] or ln["screen_ok"]:
            continue
        for name in ("CML_KMEANS_SCREEN", "CML_KMEANS_PRUNE", "CML_KMEANS_PRECISION", "CML_KMEANS_GRAPH",
                     "CML_KMEANS_REFRESH"):
            monkeypatch.delenv(name, raising=False)
        for name, v in ln["env"].items():
            monkeypatch.setenv(name, v)
        kw = dict(ln["args"], spherical=ln["spherical"], precision=ln["precision"], prune=ln["prune"],
                  weights=w if ln["weights"] else None)
        if isinstance(ln["want"], str):
            with pytest.raises(ValueError) as err:
                LloydEngine(data[ln["rows"]], 8, 4, **kw)
            assert str(err.value) == ln["want"], ln
        else:
            _check(LloydEngine(data[ln["rows"]], 8, 4, **kw), dict(zip(TABLE["fields"], ln["want"])), ln)
        checked += 1
    assert checked > 200
    for name in ("CML_KMEANS_SCREEN", "CML_KMEANS_PRECISION"):
        monkeypatch.delenv(name, raising=False)
    wide = torch.randn(64, 128, generator=g, dtype=torch.float32).to(dev)
    for ln in _lines():
        if (ln["rows"], ln["screen_ok"], ln["env"], ln["args"], ln["weights"], ln["spherical"]) == (
                "f32", True, {}, {}, False, False):
            eng = LloydEngine(wide, 128, 8, precision=ln["precision"], prune=ln["prune"])
            _check(eng, dict(zip(TABLE["fields"], ln["want"])), ln)
            checked += 1
    assert checked > 215


def _check(eng, want, ln):
    assert (eng.precision, eng.prune, eng._wfast, eng._screen, eng.gpu) == (
        want["precision"], want["prune"], want["wfast"], want["screen"], want["gpu"]), ln
    # the second stage (_alloc_gpu): pruned steps without a K9r plan take the torch form, which is never captured
    assert eng.use_graph == (want["use_graph"] and not (eng.gpu and eng.prune and not eng._pdev)), ln
    assert eng.row_chunks == min(want["row_chunks"] or 1, eng.n), ln  # (one rank, few rows: the default is 1)
