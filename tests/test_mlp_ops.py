"""``ops/mlp_ops.py``: the chunked reference form of the MLP loss, gradient and forward pass against the
estimator's autograd expression, and the limits of K30."""
import numpy as np
import pytest
import torch

from clustermachinelearningforhospitalnetworks_apache_spark_amd.ml.classification_more import (
    _mlp_forward, _mlp_size, _mlp_unpack)
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import mlp_ops as MO

N = 4099
TOPOLOGIES = [[3, 5, 2], [10, 16, 3], [12, 7, 4, 17], [4, 3]]


def _case(layers, seed=0):
    rs = np.random.RandomState(seed + 7 * len(layers) + layers[0])
    x = torch.as_tensor(rs.randn(N, layers[0]))
    y = torch.as_tensor(rs.randint(0, layers[-1], N))
    p = np.concatenate([rs.uniform(-np.sqrt(6.0 / (a + b)), np.sqrt(6.0 / (a + b)), a * b + b)
                        for a, b in zip(layers[:-1], layers[1:])])
    return x, y, torch.as_tensor(p)


def _autograd(x, y, layers, p):
    """The estimator's dense expression: ``[grad | loss]``."""
    pt = p.clone().requires_grad_(True)
    z = _mlp_forward(x, _mlp_unpack(pt, layers))
    Y = torch.nn.functional.one_hot(y.to(torch.int64), layers[-1]).to(torch.float64)
    loss = (torch.logsumexp(z, 1) - (z * Y).sum(1)).sum()
    g, = torch.autograd.grad(loss, pt)
    return torch.cat([g, loss.detach().reshape(1)]).numpy()


@pytest.mark.parametrize("chunk", [1000, 8192])
@pytest.mark.parametrize("layers", TOPOLOGIES)
def test_reference_equals_autograd(layers, chunk):
    x, y, p = _case(layers)
    got = MO.loss_grad_reference(x, layers[0], y, layers, p, chunk=chunk)
    assert got.dtype == torch.float64 and got.shape == (_mlp_size(layers) + 1,)
    np.testing.assert_allclose(got.numpy(), _autograd(x, y, layers, p), rtol=1e-12)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn])
@pytest.mark.parametrize("layers", TOPOLOGIES)
def test_low_precision_rows_are_widened_exactly(layers, dtype):
    x, y, p = _case(layers)
    xl = x.to(torch.float32).to(dtype)
    wide = xl.to(torch.float32).to(torch.float64)
    got = MO.loss_grad_reference(xl, layers[0], y.to(torch.int32), layers, p, chunk=1000)
    np.testing.assert_allclose(got.numpy(), _autograd(wide, y, layers, p), rtol=1e-12)
    z = MO.forward_reference(xl, layers[0], layers, p, 1000)
    np.testing.assert_allclose(z.numpy(), _mlp_forward(wide, _mlp_unpack(p, layers)).numpy(), rtol=1e-12)


@pytest.mark.parametrize("layers", TOPOLOGIES)
def test_forward_reference(layers):
    x, _, p = _case(layers)
    want = _mlp_forward(x, _mlp_unpack(p, layers))
    for chunk in (1000, 8192):
        z = MO.forward_reference(x, layers[0], layers, p, chunk)
        assert z.dtype == torch.float64 and z.shape == (N, layers[-1])
        np.testing.assert_allclose(z.numpy(), want.numpy(), rtol=1e-12)
    assert MO.forward_reference(x[:0], layers[0], layers, p, 1000).shape == (0, layers[-1])


def _abs_terms(x, y, layers, p):
    """The sum of the absolute terms of every message entry: ``sum_rows |delta_l| |a_{l-1}|``, ``sum_rows
    |delta_l|`` and ``sum_rows (|lse| + |z_y|)``."""
    params = _mlp_unpack(p, layers)
    acts = [x]
    for l, (W, b) in enumerate(params):
        z = acts[-1] @ W.T + b
        acts.append(torch.sigmoid(z) if l < len(params) - 1 else z)
    z = acts[-1]
    delta = torch.softmax(z, 1)
    delta[torch.arange(len(y)), y.to(torch.int64)] -= 1.0
    out = [None] * len(params)
    for l in range(len(params) - 1, -1, -1):
        out[l] = torch.cat([(delta.abs().T @ acts[l].abs()).T.reshape(-1), delta.abs().sum(0)])
        if l:
            delta = (delta @ params[l][0]) * (acts[l] * (1.0 - acts[l]))
    zy = z.gather(1, y.to(torch.int64)[:, None])[:, 0]
    return torch.cat(out + [(torch.logsumexp(z, 1).abs() + zy.abs()).sum().reshape(1)]).numpy()


@pytest.mark.parametrize("layers", TOPOLOGIES)
def test_two_shards_add_up(layers):
    x, y, p = _case(layers)
    cut = 1777
    whole = MO.loss_grad_reference(x, layers[0], y, layers, p).numpy()
    parts = (MO.loss_grad_reference(x[:cut], layers[0], y[:cut], layers, p)
             + MO.loss_grad_reference(x[cut:], layers[0], y[cut:], layers, p)).numpy()
    assert (np.abs(parts - whole) <= 1e-12 * _abs_terms(x, y, layers, p)).all()


def test_argument_checks():
    x, y, p = _case([3, 5, 2])
    with pytest.raises(ValueError):
        MO.loss_grad_reference(x, 3, y, [3, 5, 2], p[:-1])
    with pytest.raises(ValueError):
        MO.loss_grad_reference(x, 3, y, [4, 5, 2], p)
    with pytest.raises(ValueError):
        MO.forward_reference(x, 3, [3, 5, 3], p)
    out = MO.loss_grad_reference(x[:0], 3, y[:0], [3, 5, 2], p)
    assert out.shape == (p.numel() + 1,) and not out.any()


def test_kernel_enabled(monkeypatch):
    monkeypatch.delenv("CML_MLP_KERNEL", raising=False)
    assert MO.kernel_enabled()
    monkeypatch.setenv("CML_MLP_KERNEL", "0")
    assert not MO.kernel_enabled()


def test_kernel_supported():
    bf = torch.bfloat16
    for dp in (16, 32, 64, 128, 256):  # one hidden layer of 1..32 units, 2..32 classes
        for h, c in ((1, 2), (16, 16), (17, 2), (32, 32), (1, 32), (32, 2)):
            assert MO.kernel_supported(bf, dp, [dp - 3, h, c]), (dp, h, c)
            assert 0 < MO.lds_bytes(dp, [dp - 3, h, c]) <= 160 * 1024
    for h, c in ((1, 2), (16, 16), (7, 3)):  # width 512: up to 16 units and 16 classes
        assert MO.kernel_supported(bf, 512, [512, h, c]) and MO.lds_bytes(512, [512, h, c]) <= 160 * 1024
    for dp in (16, 32, 64, 128):  # two hidden layers of 1..32 units
        for h1, h2, c in ((1, 1, 2), (32, 32, 32), (8, 4, 17), (32, 1, 2)):
            assert MO.kernel_supported(bf, dp, [dp, h1, h2, c]), (dp, h1, h2, c)
    assert not MO.kernel_supported(torch.float32, 64, [64, 16, 3])
    assert not MO.kernel_supported(torch.float8_e4m3fn, 256, [256, 16, 3])
    assert not MO.kernel_supported(bf, 1024, [1024, 16, 3])
    assert not MO.kernel_supported(bf, 64, [64, 33, 3])
    assert not MO.kernel_supported(bf, 64, [64, 16, 33])
    assert not MO.kernel_supported(bf, 64, [64, 3])
    assert not MO.kernel_supported(bf, 64, [64, 8, 8, 8, 3])   # more than two hidden layers
    assert not MO.kernel_supported(bf, 512, [512, 32, 2])      # 251 424 B of LDS
    assert not MO.kernel_supported(bf, 256, [256, 32, 32, 2])  # 171 808 B of LDS
    assert MO.lds_bytes(256, [256, 32, 2]) == 153120 and MO.lds_bytes(512, [512, 16, 3]) == 154912
