"""The tree kernels K17-K21 (``_native/csrc/trees.hip``), kernel by kernel, against the exact oracles
of ``tree_oracle`` — the cases of ``tree_cases``, which ``test_tree_oracle.py`` has checked on the
CPU first.  Whole fits on a device frame are reached by test_gpu_glm_trees.py and test_tree_bins.py;
here every kernel meets the shapes, types and edges of its own: the four binize instantiations on
either side of the LDS limit, NaN cells, every LDS chunking of the histogram, exact ties and gates
in the split search, and the second iteration of every grid-stride loop.

K19: the worst |gain - exact| / err printed on an MI355X is 0.0636 (case nodes_3x64; err is the bound
derived in ``tree_oracle.best_split``, not a measurement).
"""
import functools

import numpy as np
import pytest
import torch

import tree_cases as C
from clustermachinelearningforhospitalnetworks_apache_spark_amd import _native
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models import trees as TR

pytestmark = pytest.mark.gpu
GPU = "cuda"


# ---------------------------------------------------------------------------------------------- K17

@functools.lru_cache(maxsize=None)
def _binize(name):
    return C.run_binize(GPU, C.binize_case(name))


@pytest.mark.parametrize("name", list(C.BINIZE_SHAPES))
def test_binize_codes_equal_oracle(name):
    """Every cell that holds a number: thresholds met exactly and missed by one ulp, +-inf, -0.0."""
    c = C.binize_case(name)
    keep = ~c["nan_mask"]
    assert np.array_equal(_binize(name)[keep], c["expected"][keep])


@pytest.mark.parametrize("name", list(C.BINIZE_SHAPES))
def test_binize_nan_takes_the_last_bin(name):
    """NaN sorts above every threshold: bin nsplit[f], the side K21 and the host predictor send it to."""
    c = C.binize_case(name)
    m = c["nan_mask"]
    assert np.array_equal(_binize(name)[m], c["expected"][m])
    assert np.array_equal(c["expected"][m], np.broadcast_to(c["nsplit"], m.shape)[m])


def test_binize_row_strided_view():
    """ld = d + 3: the engine always passes a contiguous frame, the kernel's contract is wider."""
    c = C.binize_case("lds_u8", nan=False)
    n, d, ms = c["n"], c["d"], c["ms"]
    base = torch.full((n, d + 3), float("nan"), dtype=torch.float64, device=GPU)
    base[:, :d] = torch.as_tensor(c["x"])
    view = base[:, :d]
    assert view.stride(0) == d + 3
    thr = torch.as_tensor(c["thr"]).to(GPU).contiguous()
    ns = torch.as_tensor(c["nsplit"]).to(GPU).contiguous()
    out = torch.empty((n, d), dtype=torch.uint8, device=GPU)
    st = _native.kernels().cml_tree_binize(view.data_ptr(), n, view.stride(0), d, thr.data_ptr(), ms, ns.data_ptr(),
                                           out.data_ptr(), 1, _native.stream_ptr())
    _native.check(st, "tree_binize")
    assert np.array_equal(C.codes_of(out), c["expected"])


# ---------------------------------------------------------------------------------------------- K18

@pytest.mark.parametrize("name", list(C.HIST_CASES))
def test_histogram_equals_oracle(name):
    c = C.hist_case(name)
    first, second = C.run_hist(GPU, c, repeat=2)
    assert first.dtype == torch.int64 and torch.equal(first, second)     # the same bits, run after run
    assert torch.equal(first, torch.as_tensor(c["expected"]))


# ---------------------------------------------------------------------------------------------- K19

@pytest.mark.parametrize("name", list(C.SPLIT_CASES))
def test_best_split_equals_oracle(name):
    """The histogram is the oracle's own.  First the case's answer is shown to be unique (no gain
    within 2 err of the tie threshold or of a gate), then feature, bin and statistics must be the
    oracle's and the gain within err of the exact gain.  gini_S17 is wider than the kernel and takes
    the host rule."""
    C.check_best_splits(GPU, name)


# ---------------------------------------------------------------------------------------------- K20

@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_route_equals_oracle(name):
    c = C.route_case(name)
    assert np.array_equal(C.run_route(GPU, c), c["expected"])


# ---------------------------------------------------------------------------------------------- K21

@pytest.mark.parametrize("name", list(C.PREDICT_CASES))
def test_predict_equals_oracle(name):
    c = C.predict_case(name)
    assert C.same_bits(C.run_predict(GPU, c), c["expected"])


# ---------------------------------------------------------------------------------------------- whole fits

@functools.lru_cache(maxsize=None)
def _cpu_fit(name):
    return C.run_fit("cpu", name)


@pytest.mark.parametrize("name", list(C.FIT_SETS))
def test_small_fit_matches_cpu(name):
    """Gates, sample weights, subsampling with and without bootstrap, 5 and 17 classes, on columns
    with few distinct values, a duplicate, a negated copy, a constant and NaN cells."""
    ce, cpu, cpu_pred = _cpu_fit(name)
    ge, gpu, gpu_pred = C.run_fit(GPU, name)
    assert torch.equal(ge.bins.cpu(), ce.bins)
    assert len(cpu) == len(gpu)
    for a, b in zip(cpu, gpu):
        na, nb = TR.preorder(a), TR.preorder(b)
        assert len(na) == len(nb)
        for u, v in zip(na, nb):
            assert (u.feature, u.split_bin) == (v.feature, v.split_bin)
            assert np.array_equal(u.stats, v.stats)
    assert C.same_bits(cpu_pred, gpu_pred)
    if name == "gates_and_weights":
        C.check_leaf_weights(gpu[0], C.fit_data())
