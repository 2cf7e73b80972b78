"""``ops/gram_ops.py``: the chunked reference form of the Gram matrix ``[X 1 z]^T W [X 1 z]`` against the one-shot f64
formula ``A.T @ (w[:, None] * A)``, and the limits of K31.

Bound per entry: both sides are n-term f64 sums of once-rounded products (``w_r a_rj`` rounded, then the product
with ``a_ri`` accumulated), each within ``(n + 2) 2^-53 M[i][j]`` of the exact value, ``M[i][j] = sum_r |w_r a_ri
a_rj|``; hence ``|G - G_one_shot| <= 2 (n + 2) 2^-53 M``.
"""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import gram_ops as GO

N, D = 5000, 40
DTYPES = [torch.float64, torch.float32, torch.bfloat16, torch.float8_e4m3fn]


def _stored(dtype):
    rs = np.random.RandomState(7)
    x = torch.as_tensor(rs.randn(N, D + 3))  # three more columns than d: they must not be read
    x = x.to(torch.float32).to(dtype) if dtype == torch.float8_e4m3fn else x.to(dtype)
    z = torch.as_tensor(1e3 * rs.randn(N))
    w = torch.as_tensor(rs.rand(N))
    w[rs.rand(N) < 0.05] = 0.0
    return x, z, w


def _widen(x):
    return (x.to(torch.float32) if x.dtype == torch.float8_e4m3fn else x).to(torch.float64)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32", "bf16", "e4m3"])
def test_reference_against_one_shot(dtype, weighted, monkeypatch):
    monkeypatch.setattr(GO, "CHUNK", 777)  # 5000 = 6 * 777 + 338
    x, z, w = _stored(dtype)
    ww = w if weighted else torch.ones(N, dtype=torch.float64)
    A = torch.cat([_widen(x[:, :D]), torch.ones(N, 1, dtype=torch.float64), z[:, None]], 1)
    want = A.T @ (ww[:, None] * A)
    M = A.abs().T @ (ww[:, None] * A.abs())
    G = GO.gram_reference(x, D, z, w if weighted else None)
    assert G.dtype == torch.float64 and G.shape == (D + 2, D + 2) and torch.isfinite(G).all()
    assert torch.equal(G, G.T)
    bound = 2.0 * (N + 2) * 2.0 ** -53 * M
    err = (G - want).abs()
    print(f"{dtype} weighted={weighted}: max |G - G1| / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all()
    sw = float(ww.sum())
    assert abs(float(G[D, D]) - sw) <= 2.0 * (N + 2) * 2.0 ** -53 * sw
    xtw = _widen(x[:, :D]).T @ ww
    assert ((G[:D, D] - xtw).abs() <= bound[:D, D]).all()


def test_reference_chunk_larger_than_n_and_empty():
    x, z, w = _stored(torch.bfloat16)
    a = GO.gram_reference(x[:100], D, z[:100], w[:100])
    assert a.shape == (D + 2, D + 2) and torch.equal(a, a.T)
    e = GO.gram_reference(x[:0], D, z[:0], None)
    assert e.shape == (D + 2, D + 2) and not e.any()
    with pytest.raises(ValueError):
        GO.gram_reference(x, D, z[:-1], None)
    with pytest.raises(ValueError):
        GO.gram_reference(x, D + 4, z, None)


def test_kernel_supported_truth_table():
    for d, want in ((30, False), (31, True), (512, True), (513, False)):
        assert GO.kernel_supported(torch.bfloat16, d) is want
    for dt in (torch.float64, torch.float32, torch.float16, torch.float8_e4m3fn):
        for d in (30, 31, 40, 512, 513):
            assert GO.kernel_supported(dt, d) is False


def test_kernel_enabled_switch(monkeypatch):
    monkeypatch.delenv("CML_GRAM_KERNEL", raising=False)
    assert GO.kernel_enabled()
    monkeypatch.setenv("CML_GRAM_KERNEL", "0")
    assert not GO.kernel_enabled()
    monkeypatch.setenv("CML_GRAM_KERNEL", "1")
    assert GO.kernel_enabled()
