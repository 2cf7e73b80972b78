"""``ops/_fused.py``: the helpers that the host wrappers of the fused f64-MFMA kernels share, and the public names
that the six ops modules keep."""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import (_fused as F, bisect_ops, fm_ops, gmm_ops,
                                                                            gram_ops, lda_ops, mlp_ops)

N, D, WIDTH = 37, 17, 20


def _matrix(dtype):
    rs = np.random.RandomState(7)
    return torch.as_tensor(rs.randn(N, WIDTH)).to(torch.float32).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn])
def test_gather_rows_equals_indexing_the_widened_matrix(dtype):
    x = _matrix(dtype)
    wide = x.to(torch.float32).to(torch.float64)
    idx = torch.as_tensor(np.random.RandomState(3).permutation(N)[:23].astype(np.int64))
    for mod_gather in (F.gather_rows, gmm_ops.gather_rows, lda_ops.gather_rows):
        got = mod_gather(x, None, D)
        assert got.dtype == torch.float64 and torch.equal(got, wide[:, :D])
        got = mod_gather(x, idx, D)
        assert got.dtype == torch.float64 and torch.equal(got, wide[idx][:, :D])


def test_widen_of_e4m3_goes_through_f32(monkeypatch):
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7f) != 0x7f]  # every e4m3 value but the two NaNs
    x = codes.view(torch.float8_e4m3fn)
    want = x.to(torch.float32).to(torch.float64)
    seen, to = [], torch.Tensor.to

    def spy(self, *a, **k):
        seen.append(a[0] if a else k.get("dtype"))
        return to(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "to", spy)
    got = F.widen(x)
    monkeypatch.undo()
    assert seen == [torch.float32, torch.float64]
    assert got.dtype == torch.float64 and torch.equal(got, want)
    b = _matrix(torch.bfloat16)
    assert torch.equal(F.widen(b), b.to(torch.float64))


def test_row_list_takes_a_1d_int64_tensor_only():
    dev = torch.device("cpu")
    rows = torch.arange(6, dtype=torch.int64)[::2]
    got = F.row_list(rows, dev, "t")
    assert got.is_contiguous() and torch.equal(got, rows)
    for bad in (torch.arange(5, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int64), [0, 1, 2]):
        with pytest.raises(ValueError, match="t: the row list"):
            F.row_list(bad, dev, "t")


def test_check_matrix_keeps_each_modules_message():
    x = _matrix(torch.bfloat16)  # not a device matrix
    with pytest.raises(ValueError, match="^w: rows must be a contiguous bf16 device matrix of padded width 16 or 32, x$"):
        F.check_matrix(x, D, lambda dtype, dp: True, "w", "16 or 32, x")


PUBLIC = {
    gmm_ops: ["CHUNK", "kernel_enabled", "kernel_supported", "estep_reference", "predict_reference", "gather_rows",
              "column_moments", "estep", "predict"],
    lda_ops: ["CHUNK", "kernel_enabled", "kernel_supported", "lds_bytes", "gather_rows", "row_sums", "estep_reference",
              "estep", "infer", "digamma"],
    mlp_ops: ["CHUNK", "kernel_enabled", "kernel_supported", "lds_bytes", "size", "loss_grad_reference",
              "forward_reference", "loss_grad", "forward"],
    fm_ops: ["CHUNK", "LOSSES", "kernel_enabled", "kernel_supported", "lds_bytes", "size", "loss_grad_reference",
             "scores_reference", "loss_grad", "scores"],
    gram_ops: ["CHUNK", "MIN_D", "MAX_D", "kernel_enabled", "kernel_supported", "gram_reference", "gram"],
    bisect_ops: ["CHUNK", "kernel_enabled", "kernel_supported", "bisect_step_reference", "make_plan", "bisect_step"],
}
SWITCH = {gmm_ops: "CML_GMM_KERNEL", lda_ops: "CML_LDA_KERNEL", mlp_ops: "CML_MLP_KERNEL", fm_ops: "CML_FM_KERNEL",
          gram_ops: "CML_GRAM_KERNEL", bisect_ops: "CML_BISECT_KERNEL"}


@pytest.mark.parametrize("mod", list(PUBLIC), ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_ops_modules_keep_their_public_names_and_switch(mod, monkeypatch):
    for name in PUBLIC[mod]:
        assert hasattr(mod, name), name
    monkeypatch.delenv(SWITCH[mod], raising=False)
    assert mod.kernel_enabled()
    monkeypatch.setenv(SWITCH[mod], "0")
    assert not mod.kernel_enabled()


@pytest.mark.parametrize("mod,arg", [(gmm_ops, 4), (lda_ops, 4), (mlp_ops, [D, 8, 3]), (fm_ops, 4)],
                         ids=["gmm", "lda", "mlp", "fm"])
def test_use_kernel_reads_the_module_at_call_time(mod, arg, monkeypatch):
    monkeypatch.delenv(SWITCH[mod], raising=False)
    x = _matrix(torch.bfloat16)[:, :D]
    assert F.use_kernel(mod, x, arg)
    assert not F.use_kernel(mod, x.to(torch.float8_e4m3fn), arg)
    monkeypatch.setattr(mod, "kernel_enabled", lambda: False)
    assert not F.use_kernel(mod, x, arg)
    monkeypatch.undo()
    monkeypatch.setattr(mod, "kernel_supported", lambda dtype, dp, a: False)
    assert not F.use_kernel(mod, x, arg)
