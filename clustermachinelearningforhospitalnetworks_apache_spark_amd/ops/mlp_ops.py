"""Loss, gradient and forward pass of the multilayer perceptron classifier: the reference form and the host
wrappers of K30 (``_native/csrc/mlp.hip``).

The parameters ``p`` are Spark's flat vector, as ``ml.classification_more._mlp_unpack`` reads it: per layer ``W``
(out x in, column-major), then ``b``. For ``layers = [d, h_1, .., C]`` with L weight layers and a row x with label
y, in f64 after the exact widening:

* ``a_0 = x``, ``z_l = W_l a_{l-1} + b_l``, ``a_l = 1 / (1 + exp(-z_l))`` for ``l < L``
* ``loss = logsumexp(z_L) - z_L[y]`` (the row maximum subtracted inside), ``delta_L = softmax(z_L) - onehot(y)``
* ``delta_l = (W_{l+1}^T delta_{l+1}) * a_l (1 - a_l)``, ``dW_l = sum_rows delta_l a_{l-1}^T``,
  ``db_l = sum_rows delta_l``

The sums are not divided by the number of rows: the caller divides after its all-reduce. The message of a shard is
the f64 vector ``[grad in the flat layout | loss]``.

``loss_grad_reference`` / ``forward_reference`` evaluate this in f64 torch chunk by chunk on any device and dtype
(one chunk of the rows in f64 at a time, manual backprop, no autograd graph): the path of e4m3 rows and of bf16
rows outside the kernel's limits, and the oracle of the kernel. ``loss_grad`` / ``forward`` are the gfx950 kernel
for bf16 rows in the ``to_device_matrix`` layout (``kernel_supported``): one launch reads every row once, a small
second launch adds the per-workgroup partials in workgroup order. ``CML_MLP_KERNEL=0`` keeps the estimator on the
reference form.
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from .. import _native
from .._native import c_int, c_ll, c_vp
from ._fused import check_matrix, env_enabled, ncu, widen

_native.register_kernel_sigs({
    "cml_mlp_lds": (c_ll, [c_int, c_int, c_int]),
    "cml_mlp_grid": (c_int, [c_ll, c_int, c_int, c_int, c_int]),
    "cml_mlp_pass": (c_int, [c_vp, c_ll, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp,
                             c_int, c_int, c_vp]),
})

CHUNK = 8192
_TILE = 64


def kernel_enabled() -> bool:
    return env_enabled("CML_MLP_KERNEL")


def size(layers: Sequence[int]) -> int:
    """Length of the flat parameter vector of a topology."""
    return sum(a * b + b for a, b in zip(layers[:-1], layers[1:]))


def lds_bytes(dp: int, layers: Sequence[int]) -> int:
    """LDS bytes of K30 (what ``cml_mlp_lds`` returns), 0 outside the limits. With L = len(layers) - 1 = 2 or 3
    weight layers, every non-input layer padded to hp = 16 (widest of them <= 16) or 32 units and the compiled
    width class dpt = max(dp, 64): the f64 image of W_1 ``hp * dpt``, the upper layers in both orientations
    ``2 (L - 1) hp (hp + 2)``, the biases ``L hp``, the two staging buffers of delta^T and a^T ``2 * hp * 66``
    and the fold of db and the loss ``4 (L hp + 1)`` doubles, plus the 64-row bf16 tile ``64 * (dpt + 8)`` values:
    ``8 * (hp dpt + 2 (L - 1) hp (hp + 2) + L hp + 132 hp + 4 (L hp + 1)) + 128 * (dpt + 8)`` bytes. That is
    153 120 B (150 KB) at dp = 256, hp = 32, L = 2, 154 912 B at dp = 512, hp = 16, L = 2, 160 160 B at dp = 512,
    hp = 16, L = 3 and 122 656 B at dp = 128, hp = 32, L = 3, inside one CU's 160 KB = 163 840 B; dp = 256 with
    hp = 32 and L = 3 would need 171 808 B, dp = 512 with hp = 32 and L = 2 251 424 B."""
    layers = [int(v) for v in layers]
    nl = len(layers) - 1
    if nl < 2 or nl > 3 or dp < 16 or dp > 512 or dp & (dp - 1):
        return 0
    if min(layers[1:]) < 1 or max(layers[1:]) > 32 or layers[-1] < 2:
        return 0
    hp = 16 if max(layers[1:]) <= 16 else 32
    dpt = max(dp, 64)
    b = 8 * (hp * dpt + 2 * (nl - 1) * hp * (hp + 2) + nl * hp + 2 * hp * 66 + 4 * (nl * hp + 1)) + 2 * _TILE * (dpt + 8)
    return b if b <= 160 * 1024 else 0


def kernel_supported(dtype: torch.dtype, dp: int, layers: Sequence[int]) -> bool:
    """Whether K30 takes rows of this dtype and padded width with this topology (anything else: the reference
    form). bf16 rows of padded width 16..512, one or two hidden layers, every hidden layer of 1..32 units and
    2..32 classes, as far as the LDS sum of ``lds_bytes`` allows: widths up to 128 take all of these, width 256
    everything but two hidden layers with a layer wider than 16, width 512 layers of at most 16 units."""
    return dtype == torch.bfloat16 and lds_bytes(int(dp), layers) > 0


# ---------------------------------------------------------------------------------------------- reference form
def _unpack(p: torch.Tensor, layers: Sequence[int]):
    out, off = [], 0
    for a, b in zip(layers[:-1], layers[1:]):
        W = p[off:off + a * b].reshape(a, b).T  # column-major [out, in]
        off += a * b
        out.append((W, p[off:off + b]))
        off += b
    return out


def _params(x: torch.Tensor, d: int, layers: Sequence[int], p, what: str):
    layers = [int(v) for v in layers]
    if len(layers) < 2 or layers[0] != d or x.dim() != 2 or x.shape[1] < d:
        raise ValueError(f"{what}: layers must start with the d columns of the rows")
    p = torch.as_tensor(p).to(device=x.device, dtype=torch.float64)
    if p.dim() != 1 or p.numel() != size(layers):
        raise ValueError(f"{what}: {p.numel()} parameters, the topology needs {size(layers)}")
    return layers, p


def _forward_chunk(v: torch.Tensor, params) -> List[torch.Tensor]:
    """``[a_0, .., a_{L-1}, z_L]`` of one widened chunk."""
    acts = [v]
    for l, (W, b) in enumerate(params):
        z = acts[-1] @ W.T + b
        acts.append(torch.sigmoid(z) if l < len(params) - 1 else z)
    return acts


def loss_grad_reference(x: torch.Tensor, d: int, y: torch.Tensor, layers: Sequence[int], p,
                        chunk: int = CHUNK) -> torch.Tensor:
    """f64 ``[len(p) + 1]`` = ``[grad in the flat layout | loss]`` of the rows ``x`` ``[n, >= d]`` (any dtype and
    device) with integer labels ``y`` ``[n]``, one widened chunk of rows at a time."""
    layers, p = _params(x, d, layers, p, "mlp loss_grad")
    n, dev = int(x.shape[0]), x.device
    if y.shape != (n,):
        raise ValueError("mlp loss_grad: one label per row is expected")
    params = _unpack(p, layers)
    gW = [torch.zeros(W.shape, dtype=torch.float64, device=dev) for W, _ in params]
    gb = [torch.zeros(b.shape, dtype=torch.float64, device=dev) for _, b in params]
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    for st in range(0, n, chunk):
        acts = _forward_chunk(widen(x[st:st + chunk, :d]), params)
        yc = y[st:st + chunk].to(device=dev, dtype=torch.int64)[:, None]
        z = acts[-1]
        m = z.max(1, keepdim=True).values
        e = torch.exp(z - m)
        s = e.sum(1, keepdim=True)
        loss += ((m + torch.log(s)) - z.gather(1, yc)).sum()
        delta = e / s
        delta.scatter_add_(1, yc, torch.full_like(yc, -1, dtype=torch.float64))
        for l in range(len(params) - 1, -1, -1):
            gW[l] += delta.T @ acts[l]
            gb[l] += delta.sum(0)
            if l:
                delta = (delta @ params[l][0]) * (acts[l] * (1.0 - acts[l]))
    return torch.cat([t for W, b in zip(gW, gb) for t in (W.T.reshape(-1), b)] + [loss.reshape(1)])


def forward_reference(x: torch.Tensor, d: int, layers: Sequence[int], p, chunk: int = CHUNK) -> torch.Tensor:
    """f64 ``[n, C]`` raw scores ``z_L`` of the rows ``x`` ``[n, >= d]`` of any dtype and device."""
    layers, p = _params(x, d, layers, p, "mlp forward")
    params = _unpack(p, layers)
    n = int(x.shape[0])
    out = torch.empty(n, layers[-1], dtype=torch.float64, device=x.device)
    for st in range(0, n, chunk):
        out[st:st + chunk] = _forward_chunk(widen(x[st:st + chunk, :d]), params)[-1]
    return out


# ---------------------------------------------------------------------------------------------------- kernel
def _pack(p: torch.Tensor, layers: List[int], dp: int) -> torch.Tensor:
    """The kernel's parameter image: W_1 ``[hp, dp]``, W_l ``[hp out, hp in]`` for the upper layers, then the
    biases ``[L, hp]``, zero padded."""
    nl = len(layers) - 1
    hp = 16 if max(layers[1:]) <= 16 else 32
    params = _unpack(p, layers)
    w1 = torch.zeros(hp, dp, dtype=torch.float64, device=p.device)
    w1[:layers[1], :layers[0]] = params[0][0]
    wu = torch.zeros(nl - 1, hp, hp, dtype=torch.float64, device=p.device)
    bs = torch.zeros(nl, hp, dtype=torch.float64, device=p.device)
    for l, (W, b) in enumerate(params):
        if l:
            wu[l - 1, :W.shape[0], :W.shape[1]] = W
        bs[l, :b.shape[0]] = b
    return torch.cat([w1.reshape(-1), wu.reshape(-1), bs.reshape(-1)])


def _launch(xd, d, y32, layers, p, fit: bool, what: str):
    if not torch.is_tensor(xd) or xd.dim() != 2:
        raise ValueError(f"{what}: rows must be a 2-d tensor")
    dp = int(xd.shape[1])
    layers = [int(v) for v in layers]
    check_matrix(xd, d, lambda dtype, dp: kernel_supported(dtype, dp, layers) and layers[0] == d, what,
                 "16..512 and layers [d, ..] a topology inside the kernel's limits")
    n, dev = int(xd.shape[0]), xd.device
    p = torch.as_tensor(p)
    if p.dim() != 1 or p.numel() != size(layers):
        raise ValueError(f"{what}: {p.numel()} parameters, the topology needs {size(layers)}")
    if fit and (not torch.is_tensor(y32) or y32.dtype != torch.int32 or y32.shape != (n,) or y32.device != dev
                or not y32.is_contiguous()):
        raise ValueError(f"{what}: the labels must be a contiguous int32 device vector, one per row")
    np_ = size(layers)
    C = layers[-1]
    out = torch.zeros(np_ + 1, dtype=torch.float64, device=dev) if fit else torch.empty(
        n, C, dtype=torch.float64, device=dev)
    if n:
        nl, hmax = len(layers) - 1, max(layers[1:])
        hp = 16 if hmax <= 16 else 32
        wp = _pack(p.to(device=dev, dtype=torch.float64), layers, dp)
        lib, cus = _native.kernels(), ncu(dev)
        grid = int(lib.cml_mlp_grid(n, dp, hmax, nl, cus))
        part = torch.empty(grid * (hp * dp + (nl - 1) * hp * hp + nl * hp + 1), dtype=torch.float64,
                           device=dev) if fit else None
        s = layers[1:] + [0] * (4 - len(layers))
        _native.check(lib.cml_mlp_pass(xd.data_ptr(), n, dp, d, nl, s[0], s[1], s[2], _native.ptr(y32 if fit else None),
                                       wp.data_ptr(), _native.ptr(part), grid, out.data_ptr(), 1 if fit else 0, cus,
                                       torch.cuda.current_stream(dev).cuda_stream), what)
    return out


def loss_grad(xd: torch.Tensor, d: int, y32: torch.Tensor, layers: Sequence[int], p) -> torch.Tensor:
    """K30, fit form: the f64 device vector ``[grad | loss]`` as ``loss_grad_reference`` returns it. All arithmetic
    after the exact bf16 -> f64 widening is f64 (the products on the f64 MFMA); pad columns are masked by ``d``.
    No atomics, no host read; two calls return the same bits."""
    return _launch(xd, d, y32, layers, p, True, "mlp loss_grad")


def forward(xd: torch.Tensor, d: int, layers: Sequence[int], p) -> torch.Tensor:
    """K30 without the backward pass: f64 ``[n, C]`` raw scores, bit for bit the fit form's ``z_L``."""
    return _launch(xd, d, None, layers, p, False, "mlp forward")
