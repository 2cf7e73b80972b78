"""``ops/nb_ops.py`` on the CPU: the chunked reference forms against dense numpy, and the routing of K34."""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import _fused
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import nb_ops as NO

N = 53


def _data(d, C, seed=0, dtype=torch.float64):
    rs = np.random.RandomState(seed + 10 * d + C)
    x = rs.randint(-1, 4, (N, d + 2)).astype(np.float64)      # two columns past d, to be ignored
    x[:, d:] = np.nan
    xt = torch.as_tensor(x).to(torch.float32).to(dtype)
    lab = rs.randint(0, C, N)
    w = rs.uniform(0.1, 2.0, N)
    w[rs.rand(N) < 0.1] = 0.0
    shift = rs.randn(C, d)
    return xt, xt[:, :d].to(torch.float32).to(torch.float64).numpy(), lab, w, shift


def _dense_moments(x, lab, w, C, shift):
    n, d = x.shape
    out = np.zeros((C, 1 + 2 * d))
    for c in range(C):
        sel = lab == c
        v = x[sel] - (shift[c] if shift is not None else 0.0)
        out[c, 0] = w[sel].sum()
        out[c, 1:1 + d] = (w[sel, None] * v).sum(0)
        out[c, 1 + d:] = (w[sel, None] * v * v).sum(0)
    return out, np.array([(x < 0).sum(), ((x != 0) & (x != 1)).sum()], dtype=np.float64)


@pytest.mark.parametrize("d", [1, 17])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shifted", [False, True])
def test_moments_reference_against_dense_numpy(d, C, weighted, shifted):
    xt, x, lab, w, shift = _data(d, C)
    wn = w if weighted else np.ones(N)
    want, bad = _dense_moments(x, lab, wn, C, shift if shifted else None)
    for chunk in (7, 52, 1 << 16):  # 53 rows: uneven splits, a last chunk of one row, one chunk
        got, gbad = NO.moments_reference(xt, d, torch.as_tensor(lab), torch.as_tensor(w) if weighted else None, C,
                                         shift if shifted else None, chunk=chunk)
        assert got.dtype == torch.float64 and got.shape == (C, 1 + 2 * d)
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(gbad.numpy(), bad)
    assert bad[0] > 0 and bad[1] > bad[0]


def test_moments_reference_e4m3_labels_outside_and_no_rows():
    d, C = 17, 3
    xt, x, lab, w, shift = _data(d, C, dtype=torch.float8_e4m3fn)
    want, bad = _dense_moments(x, lab, w, C, shift)
    got, gbad = NO.moments_reference(xt, d, torch.as_tensor(lab, dtype=torch.float64), torch.as_tensor(w), C, shift,
                                     chunk=10)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(gbad.numpy(), bad)
    # labels outside 0 .. C-1 add nothing to the moments; their rows still count towards bad
    lab2 = lab.copy()
    lab2[:5] = [C, C + 7, -1, -3, 1000]
    keep = np.ones(N, bool)
    keep[:5] = False
    want2, _ = _dense_moments(x[keep], lab2[keep], w[keep], C, shift)
    got2, gbad2 = NO.moments_reference(xt, d, torch.as_tensor(lab2), torch.as_tensor(w), C, shift, chunk=10)
    np.testing.assert_allclose(got2.numpy(), want2, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(gbad2.numpy(), bad)
    e, ebad = NO.moments_reference(xt[:0], d, torch.zeros(0), None, C)
    assert e.shape == (C, 1 + 2 * d) and not e.any() and not ebad.any()
    with pytest.raises(ValueError):
        NO.moments_reference(xt, d, torch.as_tensor(lab[:-1]), None, C)


def test_moments_reference_whole_blocks_and_first_moments_only():
    """A chunk of whole 512-row blocks takes the batched GEMM; ``second=False`` leaves the second moments 0."""
    rs = np.random.RandomState(9)
    n, d, C = 1536 + 5, 7, 3
    x = rs.randint(0, 5, (n, d)).astype(np.float64)
    lab, w, shift = rs.randint(0, C, n), rs.uniform(0.1, 2.0, n), rs.randn(C, d)
    want, bad = _dense_moments(x, lab, w, C, shift)
    xt = torch.as_tensor(x).to(torch.bfloat16)
    for chunk in (1024, 1536, 512):
        got, gbad = NO.moments_reference(xt, d, torch.as_tensor(lab), torch.as_tensor(w), C, shift, chunk=chunk)
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(gbad.numpy(), bad)
    first, _ = NO.moments_reference(xt, d, torch.as_tensor(lab), torch.as_tensor(w), C, shift, chunk=1024, second=False)
    np.testing.assert_allclose(first[:, :1 + d].numpy(), want[:, :1 + d], rtol=1e-12, atol=1e-12)
    assert not first[:, 1 + d:].any()


def _dense_scores(x, kind, W, b, iv):
    if kind == "gaussian":
        s = b[None] - 0.5 * (((x[:, None, :] - W[None]) ** 2) * iv[None]).sum(2)
    elif kind == "complement":
        s = x @ W.T
    else:
        s = x @ W.T + b
    top = s.max(1, keepdims=True)
    lse = top + np.log(np.exp(s - top).sum(1, keepdims=True))
    raw = s - lse if kind == "complement" else s
    return raw, np.exp(s - lse), np.argmax(raw, 1).astype(np.float64)


@pytest.mark.parametrize("d", [1, 17])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", NO.KINDS)
def test_scores_reference_against_dense_numpy(d, C, kind):
    xt, x, _, _, W = _data(d, C, seed=3)
    rs = np.random.RandomState(d + C)
    b, iv = rs.randn(C), rs.uniform(0.5, 2.0, (C, d))
    want = _dense_scores(x, kind, W, b, iv)
    for chunk in (7, 52, 1 << 16):
        got = NO.scores_reference(xt, d, kind, W, b, iv if kind == "gaussian" else None, chunk=chunk)
        assert got[0].shape == (N, C) and got[1].shape == (N, C) and got[2].shape == (N,)
        for g, w_ in zip(got, want):
            assert g.dtype == torch.float64
            np.testing.assert_allclose(g.numpy(), w_, rtol=1e-11, atol=1e-11)
    e = NO.scores_reference(xt[:0], d, kind, W, b, iv if kind == "gaussian" else None)
    assert e[0].shape == (0, C) and e[2].shape == (0,)


def test_scores_reference_e4m3_ties_and_errors():
    xt, x, _, _, W = _data(17, 3, seed=5, dtype=torch.float8_e4m3fn)
    b = np.array([0.3, -0.2, 0.1])
    want = _dense_scores(x, "linear", W, b, None)
    got = NO.scores_reference(xt, 17, "linear", W, b, chunk=9)
    for g, w_ in zip(got, want):
        np.testing.assert_allclose(g.numpy(), w_, rtol=1e-11, atol=1e-11)
    # equal scores: the lowest index among the maxima
    tie = NO.scores_reference(torch.ones(4, 2), 2, "linear", np.ones((3, 2)), np.zeros(3))
    assert (tie[2] == 0).all()
    with pytest.raises(ValueError):
        NO.scores_reference(xt, 17, "gaussian", W, b)          # no iv
    with pytest.raises(ValueError):
        NO.scores_reference(xt, 17, "softmax", W, b)
    with pytest.raises(ValueError):
        NO.scores_reference(xt, 17, "linear", W[:, :5], b)


def test_kernel_limits():
    bf = torch.bfloat16
    for dp in NO.WIDTHS:
        for C in (1, 2, 16, 17, 32):
            assert NO.kernel_supported(bf, dp, (C, False)), (dp, C)
            assert NO.kernel_supported(bf, dp, (C, True)) == (dp < 512 or C <= 17), (dp, C)
        assert not NO.kernel_supported(bf, dp, (0, False)) and not NO.kernel_supported(bf, dp, (33, False))
    for dp in (8, 24, 48, 1024):
        assert not NO.kernel_supported(bf, dp, (2, False))
    for dt in (torch.float32, torch.float64, torch.float16, torch.float8_e4m3fn):
        assert not NO.kernel_supported(dt, 64, (2, False))
    # the edges of the LDS sum, to the byte
    assert NO.lds_bytes(512, 17, True) == 158368 <= NO.LDS_PER_CU < NO.lds_bytes(512, 18, True) == 166832
    assert NO.lds_bytes(512, 32, False) == 152064 and NO.lds_bytes(256, 32, True) == 156928
    assert NO.lds_bytes(16, 1, False) == 256 * 32 * 2 + 256 * 12   # the moments form is the larger one here
    assert NO.tile_rows(16) == 256 and NO.tile_rows(64) == 128 and NO.tile_rows(512) == 16


def test_switch_is_honoured(monkeypatch):
    class Rows:  # what use_kernel looks at
        dtype = torch.bfloat16
        shape = (10, 40)
    monkeypatch.delenv("CML_NB_KERNEL", raising=False)
    assert NO.kernel_enabled() and _fused.use_kernel(NO, Rows, (2, True))
    monkeypatch.setenv("CML_NB_KERNEL", "0")
    assert not NO.kernel_enabled() and not _fused.use_kernel(NO, Rows, (2, True))
    monkeypatch.setenv("CML_NB_KERNEL", "1")
    assert _fused.use_kernel(NO, Rows, (2, False)) and not _fused.use_kernel(NO, Rows, (40, False))
    Rows.dtype = torch.float8_e4m3fn
    assert not _fused.use_kernel(NO, Rows, (2, False))
