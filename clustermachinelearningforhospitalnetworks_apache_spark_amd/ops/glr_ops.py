"""One IRLS step of a generalized linear model with an offset: the reference form and the host wrappers of K33
(``_native/csrc/glr.hip``).

A step is described by a ``Spec``: the variance kind (``mu^p``, or the binomial ``mu (1 - mu)``), ``p``, the link kind
(the power link ``mu^lp``, ``log`` at ``lp == 0``; or logit), ``lp``, and the family whose initialisation,
projection and deviance apply (``spec`` builds one from the estimator's params). For a row with label ``y``,
weight ``w`` (1 without one) and offset ``off`` (0 without one), in f64 after the exact widening of the stored row:

* ``eta = x . beta + b0 + off``; the init form takes ``mu`` from the family's initialisation and ``eta = g(mu)``
* ``mu = project(g^-1(eta))``, ``z = eta - off + (y - mu) g'(mu)``, ``wt = w / (g'(mu)^2 V(mu))``
* ``G = [X 1 z]^T diag(wt) [X 1 z]``, ``(d + 2, d + 2)`` in K31's layout, exactly symmetric
* ``stats = [sum w dev(y, mu), sum w (y - mu)^2 / V(mu), sum w y, sum w]``

A row with ``w == 0`` contributes exactly 0 to everything (``z = 0``, ``wt = 0``, stats 0), whatever its ``eta``.
The sums are per shard: the caller all-reduces ``[G | stats]``.

``row_terms`` is the per-row arithmetic in plain f64 torch; ``step_reference`` / ``rows_reference`` evaluate a step
chunk by chunk on any device and stored dtype (one chunk of ``CHUNK`` rows in f64 at a time, never an ``n x d``
copy): the path of every column the kernel does not take, of CPU frames, and the oracle of the kernel. ``step`` /
``rows`` are the gfx950 kernel for bf16 device rows in the ``to_device_matrix`` layout of padded width 16..128
(``kernel_supported``): one launch reads every row once and makes ``eta``, ``mu``, ``z`` and ``wt`` in flight, a
small second launch adds the slabs in slab order and mirrors. ``CML_GLR_KERNEL=0`` keeps the estimator on the
reference form.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .. import _native
from .._native import c_dbl, c_int, c_ll, c_vp
from ._fused import check_matrix, env_enabled, ncu, widen

_native.register_kernel_sigs({
    "cml_glr_slabs": (c_int, [c_ll, c_int, c_int]),
    "cml_glr_part": (c_ll, []),
    "cml_glr_pass": (c_int, [c_vp, c_ll, c_ll, c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_dbl, c_dbl,
                             c_int, c_vp, c_int, c_vp, c_int, c_vp]),
})

CHUNK = 8192
MAX_DP = 128
FAMILIES = ("gaussian", "binomial", "poisson", "gamma", "tweedie")
_LINK_POWER = {"identity": 1.0, "log": 0.0, "inverse": -1.0, "sqrt": 0.5}
_FAMILY_POWER = {"gaussian": 0.0, "poisson": 1.0, "gamma": 2.0}
_EPS = 1e-16
_BIG = 1.7976931348623157e308


class Spec(NamedTuple):
    fam: int    # index into FAMILIES: whose initialisation, projection and deviance
    var: int    # 0: V = mu^p, 1: V = mu (1 - mu)
    link: int   # 0: g = mu^lp (log at 0), 1: logit
    p: float
    lp: float


def spec(family: str, link: Optional[str] = None, variance_power: float = 0.0,
         link_power: Optional[float] = None) -> Spec:
    """The spec of a family and link by name; for ``tweedie`` the link is ``link_power`` (None: ``1 - p``)."""
    fam = FAMILIES.index(family)
    if family == "tweedie":
        p = float(variance_power)
        if p != 0.0 and p < 1.0:
            raise ValueError(f"variancePower must be 0 or >= 1, got {p}")
        return Spec(fam, 0, 0, p, float(1.0 - p if link_power is None else link_power))
    if link != "logit" and link not in _LINK_POWER:
        raise ValueError(f"unsupported link {link!r}")
    logit = link == "logit"
    return Spec(fam, 1 if family == "binomial" else 0, 1 if logit else 0, _FAMILY_POWER.get(family, 0.0),
                0.0 if logit else _LINK_POWER[link])


def kernel_enabled() -> bool:
    return env_enabled("CML_GLR_KERNEL")


def kernel_supported(dtype: torch.dtype, dp: int, arg=None) -> bool:
    """Whether K33 takes rows of this dtype and padded width (anything else: the reference form). ``arg`` is the
    place of the other modules' limit (k, the factor size) in ``_fused.use_kernel``; K33 has none."""
    return dtype == torch.bfloat16 and 16 <= int(dp) <= MAX_DP


# ---------------------------------------------------------------------------------------------- reference form
def _pow(x: torch.Tensor, a: float) -> torch.Tensor:
    if a == 1.0:
        return x
    if a == 2.0:
        return x * x
    if a == 3.0:
        return x * x * x
    if a == -1.0:
        return 1.0 / x
    if a == -2.0:
        return 1.0 / (x * x)
    if a == 0.5:
        return torch.sqrt(x)
    if a == -0.5:
        return 1.0 / torch.sqrt(x)
    if a == 0.0:
        return torch.ones_like(x)
    return torch.pow(x, a)


def link(s: Spec, mu: torch.Tensor) -> torch.Tensor:
    if s.link == 1:
        return torch.log(mu / (1.0 - mu))
    if s.lp == 1.0:
        return mu
    if s.lp == 0.0:
        return torch.log(mu)
    if s.lp == -1.0:
        return 1.0 / mu
    if s.lp == 0.5:
        return torch.sqrt(mu)
    return torch.pow(mu, s.lp)


def unlink(s: Spec, eta: torch.Tensor) -> torch.Tensor:
    if s.link == 1:
        return 1.0 / (1.0 + torch.exp(-eta))
    if s.lp == 1.0:
        return eta
    if s.lp == 0.0:
        return torch.exp(eta)
    if s.lp == -1.0:
        return 1.0 / eta
    if s.lp == 0.5:
        return eta * eta
    return torch.pow(eta, 1.0 / s.lp)


def link_deriv(s: Spec, mu: torch.Tensor) -> torch.Tensor:
    if s.link == 1:
        return 1.0 / (mu * (1.0 - mu))
    if s.lp == 1.0:
        return torch.ones_like(mu)
    if s.lp == 0.0:
        return 1.0 / mu
    if s.lp == -1.0:
        return -1.0 / (mu * mu)
    if s.lp == 0.5:
        return 0.5 / torch.sqrt(mu)
    return s.lp * torch.pow(mu, s.lp - 1.0)


def variance(s: Spec, mu: torch.Tensor) -> torch.Tensor:
    return mu * (1.0 - mu) if s.var == 1 else _pow(mu, s.p)


def project(s: Spec, mu: torch.Tensor) -> torch.Tensor:
    fam = FAMILIES[s.fam]
    if fam == "binomial":
        return mu.clamp(_EPS, 1.0 - _EPS)
    if fam == "gaussian" or (fam == "tweedie" and s.p == 0.0):  # Spark takes tweedie with p = 0 as gaussian
        return mu
    return mu.clamp(_EPS, _BIG)


def init_mu(s: Spec, y: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    fam = FAMILIES[s.fam]
    if fam == "binomial":
        return (w * y + 0.5) / (w + 1.0)
    if fam == "poisson":
        return y.clamp(min=0.1)
    if fam == "tweedie" and 1.0 <= s.p < 2.0:
        return torch.where(y == 0.0, torch.full_like(y, 0.1), y)
    return y.clone()


def _ylogy(a, b):
    return torch.where(a > 0, a * torch.log(a / b), torch.zeros_like(a))


def _yp(y, mu, a: float):
    return torch.log(y / mu) if a == 0.0 else (_pow(y, a) - _pow(mu, a)) / a


def unit_deviance(s: Spec, y: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
    fam = FAMILIES[s.fam]
    r = y - mu
    if fam == "gaussian":
        return r * r
    if fam == "binomial":
        return 2.0 * (_ylogy(y, mu) + _ylogy(1.0 - y, 1.0 - mu))
    if fam == "poisson":
        return 2.0 * (_ylogy(y, mu) - r)
    if fam == "gamma":
        return 2.0 * (-torch.log(y / mu) + r / mu)
    y1 = y.clamp(min=0.1) if 1.0 <= s.p < 2.0 else y
    return 2.0 * (y * _yp(y1, mu, 1.0 - s.p) - _yp(y, mu, 2.0 - s.p))


def row_terms(eta: Optional[torch.Tensor], y: torch.Tensor, w: torch.Tensor, off: torch.Tensor, s: Spec) -> dict:
    """The f64 per-row terms ``eta, mu, z, wt`` and the stat addends ``dev, pearson, wy, sw`` at the linear predictor
    ``eta`` (offset included), or at the family's initialisation when ``eta`` is None. The operations and their
    order are those of ``glr_row_terms`` in ``glr.hip``."""
    if eta is None:
        mu = init_mu(s, y, w)
        eta = link(s, mu)
    else:
        mu = project(s, unlink(s, eta))
    gp = link_deriv(s, mu)
    V = variance(s, mu)
    r = y - mu
    live = w != 0
    zero = torch.zeros_like(y)
    return {"eta": eta, "mu": mu,
            "z": torch.where(live, (eta - off) + r * gp, zero),
            "wt": torch.where(live, w / ((gp * gp) * V), zero),
            "dev": torch.where(live, w * unit_deviance(s, y, mu), zero),
            "pearson": torch.where(live, (w * (r * r)) / V, zero),
            "wy": torch.where(live, w * y, zero),
            "sw": w}


def _vec(v, n: int, dev, fill: float) -> torch.Tensor:
    if v is None:
        return torch.full((n,), fill, dtype=torch.float64, device=dev)
    return v.reshape(-1).to(device=dev, dtype=torch.float64)


def _coef(coef, d: int, dev, what: str) -> torch.Tensor:
    c = torch.as_tensor(coef).to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    if c.numel() != d + 1:
        raise ValueError(f"{what}: {c.numel()} coefficients, d = {d} needs {d + 1} (beta, b0)")
    return c


def _check_rows(x, d: int, y, w, off, what: str) -> int:
    if not torch.is_tensor(x) or x.dim() != 2 or d < 0 or x.shape[1] < d:
        raise ValueError(f"{what}: rows [n, >= d] are expected")
    n = int(x.shape[0])
    for v in (y, w, off):
        if v is not None and v.numel() != n:
            raise ValueError(f"{what}: one label, weight and offset per row are expected")
    return n


def step_reference(x: torch.Tensor, d: int, y: torch.Tensor, w: Optional[torch.Tensor], off: Optional[torch.Tensor],
                   coef, s: Spec, init: bool, chunk: Optional[int] = None):
    """``(G, stats)`` of the rows ``x`` ``[n, >= d]`` (any dtype and device) at the coefficients ``coef`` = (beta, b0)
    or, with ``init``, at the family's initialisation: one widened chunk of rows at a time."""
    d = int(d)
    n, dev = _check_rows(x, d, y, w, off, "glr step"), x.device
    chunk = int(CHUNK if chunk is None else chunk)
    c = None if init else _coef(coef, d, dev, "glr step")
    y, w, off = _vec(y, n, dev, 0.0), _vec(w, n, dev, 1.0), _vec(off, n, dev, 0.0)
    m = d + 2
    g = torch.zeros((m, m), dtype=torch.float64, device=dev)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    for st in range(0, n, chunk):
        en = min(n, st + chunk)
        a = torch.empty((en - st, m), dtype=torch.float64, device=dev)
        a[:, :d] = widen(x[st:en, :d])
        a[:, d] = 1.0
        eta = None if init else (a[:, :d] @ c[:d] + c[d]) + off[st:en]
        t = row_terms(eta, y[st:en], w[st:en], off[st:en], s)
        a[:, d + 1] = t["z"]
        g += a.T @ (a * t["wt"][:, None])
        stats += torch.stack([t["dev"].sum(), t["pearson"].sum(), t["wy"].sum(), t["sw"].sum()])
    return torch.triu(g) + torch.triu(g, 1).T, stats


def rows_reference(x: torch.Tensor, d: int, off: Optional[torch.Tensor], coef, s: Spec, chunk: Optional[int] = None):
    """f64 ``eta, mu`` ``[n]`` of the rows ``x`` ``[n, >= d]`` of any dtype and device."""
    d = int(d)
    n, dev = _check_rows(x, d, None, None, off, "glr rows"), x.device
    chunk = int(CHUNK if chunk is None else chunk)
    c = _coef(coef, d, dev, "glr rows")
    off = _vec(off, n, dev, 0.0)
    eta = torch.empty(n, dtype=torch.float64, device=dev)
    for st in range(0, n, chunk):
        en = min(n, st + chunk)
        eta[st:en] = (widen(x[st:en, :d]) @ c[:d] + c[d]) + off[st:en]
    return eta, project(s, unlink(s, eta))


# ---------------------------------------------------------------------------------------------------- kernel
def _arg(v, n: int, dev, what: str):
    if v is None:
        return None
    if not torch.is_tensor(v) or v.numel() != n:
        raise ValueError(f"{what}: one label, weight and offset per row are expected")
    return v.reshape(-1).to(device=dev, dtype=torch.float64).contiguous()


def _launch(xd, d, y, w, off, coef, s: Spec, mode: int, what: str):
    if not torch.is_tensor(xd) or xd.dim() != 2:
        raise ValueError(f"{what}: rows must be a 2-d tensor")
    d, dp = int(d), int(xd.shape[1])
    check_matrix(xd, d, kernel_supported, what, "16..128")
    n, dev = int(xd.shape[0]), xd.device
    y, w, off = _arg(y, n, dev, what), _arg(w, n, dev, what), _arg(off, n, dev, what)
    c = None if coef is None else _coef(coef, d, dev, what)
    m = d + 2
    out = torch.zeros(4 * n if mode == 2 else m * m + 4, dtype=torch.float64, device=dev)
    if n:
        lib, cus = _native.kernels(), ncu(dev)
        slabs = int(lib.cml_glr_slabs(n, d, cus))
        part = torch.empty(slabs * int(lib.cml_glr_part()), dtype=torch.float64, device=dev) if mode != 2 else None
        _native.check(lib.cml_glr_pass(xd.data_ptr(), n, dp, dp, d, _native.ptr(y), _native.ptr(w), _native.ptr(off),
                                       _native.ptr(c), s.fam, s.var, s.link, float(s.p), float(s.lp), mode,
                                       _native.ptr(part), slabs, out.data_ptr(), cus,
                                       torch.cuda.current_stream(dev).cuda_stream), what)
    return out


def step(xd: torch.Tensor, d: int, y: torch.Tensor, w: Optional[torch.Tensor], off: Optional[torch.Tensor], coef,
         s: Spec, init: bool, gram: bool = True):
    """K33, step form: ``(G, stats)`` as ``step_reference`` returns them, for bf16 device rows in the
    ``to_device_matrix`` layout. With ``gram=False`` the products are skipped and only ``stats`` is returned. All
    arithmetic after the exact bf16 -> f64 widening is f64; pad columns are masked by ``d``; nothing of size n is
    written. No atomics, no host read; two calls return the same bits."""
    out = _launch(xd, d, y, w, off, None if init else coef, s, 0 if gram else 1, "glr step")
    m = int(d) + 2
    return (out[:m * m].view(m, m), out[m * m:]) if gram else out[m * m:]


def rows(xd: torch.Tensor, d: int, y: Optional[torch.Tensor], w: Optional[torch.Tensor], off: Optional[torch.Tensor],
         coef, s: Spec):
    """K33, rows form: the f64 device vectors ``eta, mu, z, wt`` of every row, bit for bit the step form's
    (``coef`` None: the init form's)."""
    n = int(xd.shape[0]) if torch.is_tensor(xd) and xd.dim() == 2 else 0
    out = _launch(xd, d, y, w, off, coef, s, 2, "glr rows")
    return out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n:]
