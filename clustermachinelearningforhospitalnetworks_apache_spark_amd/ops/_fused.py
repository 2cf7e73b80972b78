"""What the host wrappers of the fused f64-MFMA kernels (K27 .. K32: ``bisect_ops``, ``gmm_ops``, ``lda_ops``,
``mlp_ops``, ``gram_ops``, ``fm_ops``) share: the exact widening of low-precision rows, the row gather, the CU
count of a device, the ``CML_*_KERNEL`` switch, the argument checks of a launch and the estimators' choice between
the kernel and the reference form. The ops modules import these names; their own public names stay where they are."""
from __future__ import annotations

import os
from typing import Callable, Optional

import torch


def widen(v: torch.Tensor) -> torch.Tensor:
    """Exact f64 copy of rows of any dtype (e4m3 goes through f32)."""
    if v.dtype == torch.float8_e4m3fn:
        v = v.to(torch.float32)
    return v.to(torch.float64)


def gather_rows(x: torch.Tensor, idx: Optional[torch.Tensor], d: int) -> torch.Tensor:
    """Rows ``idx`` (None: all) of a column of any dtype, widened to f64 (e4m3 rows are gathered as bytes)."""
    if idx is None:
        return widen(x[:, :d])
    if x.dtype == torch.float8_e4m3fn:
        return widen(x.view(torch.uint8)[idx].view(torch.float8_e4m3fn)[:, :d])
    return widen(x[idx][:, :d])


def ncu(dev: torch.device) -> int:
    """CUs of the device a tensor lives on; a device without an index is the current one."""
    from ..utils.device import num_cus
    return num_cus(dev.index if dev.index is not None else torch.cuda.current_device())


def env_enabled(name: str) -> bool:
    """A kernel's switch: on unless the variable is ``0``."""
    return os.environ.get(name, "1") != "0"


def row_list(rows, dev, what: str) -> torch.Tensor:
    """The row list of a launch on ``dev``; the caller keeps None (all rows) to itself."""
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1:
        raise ValueError(f"{what}: the row list must be a 1-d int64 tensor")
    return rows.to(dev).contiguous()


def check_matrix(xd: torch.Tensor, d: int, supported: Callable[[torch.dtype, int], bool], what: str, detail: str):
    """The rows of a launch: a contiguous 2-d device matrix that ``supported(dtype, dp)`` takes, with
    ``1 <= d <= dp``. ``detail`` ends the message: the module's widths and what else ``supported`` looks at."""
    if (not xd.is_cuda or xd.dim() != 2 or not xd.is_contiguous() or not 1 <= d <= int(xd.shape[1])
            or not supported(xd.dtype, int(xd.shape[1]))):
        raise ValueError(f"{what}: rows must be a contiguous bf16 device matrix of padded width {detail}")


def use_kernel(ops, x: torch.Tensor, arg) -> bool:
    """Whether an estimator takes the kernel of the module ``ops`` for the bf16 rows ``x``: the module's switch and
    its limits (``arg``: k, the topology, the factor size) at the width ``to_device_matrix`` will pad to. Both are
    read through the module at call time."""
    from ..utils.device import padded_dim
    return (x.dtype == torch.bfloat16 and ops.kernel_enabled()
            and ops.kernel_supported(x.dtype, padded_dim(int(x.shape[1])), arg))
