"""GaussianMixture (pyspark.ml.clustering): soft clustering of hospital feature vectors.

KMeans (the [NS] flagship) gives hard hospital-regime assignments; a Gaussian mixture gives
per-regime covariances and membership probabilities. Design, MI355X-first: one EM iteration is,
per component, a triangular solve of the shard against the component's Cholesky factor (device
TRSM), a log-sum-exp over components for the responsibilities, and the weighted moments
R_kᵀ·X and (R_k ∘ X)ᵀ·X as device GEMMs (hipBLASLt) — all k·(1 + d + d²) sufficient statistics
plus the log-likelihood go into ONE all-reduce per iteration. The M-step (k small d×d matrices)
runs on the host in float64.

bf16 / e4m3 device columns never become an f64 copy: their E-step is ``ops/gmm_ops.py`` (the K28 kernel for bf16
rows of d <= 32, the chunked reference form otherwise), which returns the same all-reduced message; the M-step is
shared. f32 / f64 columns and CPU frames keep the dense form above.

Spark semantics: k=2, maxIter=100, tol=0.01 (stop when the log-likelihood improves by less than
tol), init = means of k disjoint groups of ``nSamples`` = 5 rows sampled with replacement from the
data (seeded) and the diagonal of the data variance as every initial covariance, uniform weights.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch

from ..sql import types as T
from ..sql.column import ColumnData
from ..ops._fused import use_kernel
from . import util as U
from .base import Estimator, Model
from .feature import _replace_col
from .linalg import DenseMatrix, DenseVector

_GMM_PARAMS = {
    "featuresCol": ("features", "features column name", str),
    "predictionCol": ("prediction", "prediction column name", str),
    "probabilityCol": ("probability", "column name for predicted class conditional probabilities", str),
    "k": (2, "number of independent Gaussians in the mixture model (> 1)", int),
    "maxIter": (100, "max number of iterations (>= 0)", int),
    "seed": (None, "random seed", None),
    "tol": (0.01, "convergence tolerance for iterative algorithms (>= 0)", float),
    "aggregationDepth": (2, "suggested depth for treeAggregate (>= 2)", int),
    "weightCol": (None, "weight column name", None),
}

_LOG2PI = math.log(2.0 * math.pi)


def _chol(cov: np.ndarray) -> np.ndarray:
    """Cholesky factor, with a growing ridge for (near-)singular covariances."""
    d = cov.shape[0]
    ridge = 0.0
    scale = max(float(np.trace(cov)) / max(d, 1), 1e-300)
    for _ in range(12):
        try:
            return np.linalg.cholesky(cov + ridge * np.eye(d))
        except np.linalg.LinAlgError:
            ridge = scale * 1e-10 if ridge == 0.0 else ridge * 10.0
    raise np.linalg.LinAlgError("GaussianMixture: covariance is not positive definite")


def _log_pdf(x: torch.Tensor, mus: np.ndarray, covs: np.ndarray) -> torch.Tensor:
    """[n, k] log N(x | mu_j, Sigma_j) via device triangular solves."""
    n, d = x.shape
    out = torch.empty((n, len(mus)), dtype=torch.float64, device=x.device)
    for j, (mu, cov) in enumerate(zip(mus, covs)):
        L = _chol(cov)
        Lt = torch.as_tensor(L, device=x.device)
        z = torch.linalg.solve_triangular(Lt, (x - torch.as_tensor(mu, device=x.device)).T, upper=False)
        logdet = 2.0 * float(np.log(np.diag(L)).sum())
        out[:, j] = -0.5 * (d * _LOG2PI + logdet + (z * z).sum(0))
    return out


def _inv_lower(L: np.ndarray) -> np.ndarray:
    """L^-1 of a lower triangular matrix by forward substitution (exactly lower triangular)."""
    d = L.shape[0]
    A = np.zeros((d, d))
    for i in range(d):
        A[i, :i] = -(L[i, :i] @ A[:i, :i]) / L[i, i]
        A[i, i] = 1.0 / L[i, i]
    return A


def _estep_tables(weights: np.ndarray, covs: np.ndarray):
    """``(A [k, d, d], c [k])`` of ``ops/gmm_ops.py``: A_j = L_j^-1 and the constant of lp_j."""
    d = covs.shape[1]
    Ls = [_chol(cov) for cov in covs]
    A = np.stack([_inv_lower(L) for L in Ls])
    logdet = np.array([2.0 * float(np.log(np.diag(L)).sum()) for L in Ls])
    return A, np.log(np.clip(weights, 1e-300, None)) - 0.5 * (d * _LOG2PI + logdet)


def _low_precision(x: torch.Tensor) -> bool:
    """bf16 and e4m3 device columns: the path without an f64 copy. Every other column keeps the dense form."""
    return x.is_cuda and x.dtype in (torch.bfloat16, torch.float8_e4m3fn)


def _m_step(o: np.ndarray, k: int, d: int):
    """``(weights, mus, covs, ll)`` from the all-reduced message [S0 | S1 | S2 | sum w lse | sum w]."""
    s0 = o[:k]
    s1 = o[k:k + k * d].reshape(k, d)
    s2 = o[k + k * d:k + k * d + k * d * d].reshape(k, d, d)
    ll, wt = float(o[-2]), float(o[-1])
    s0c = np.clip(s0, 1e-300, None)
    mus = s1 / s0c[:, None]
    covs = s2 / s0c[:, None, None] - np.einsum("ki,kj->kij", mus, mus)
    covs = 0.5 * (covs + np.transpose(covs, (0, 2, 1)))
    return s0 / wt, mus, covs, ll


class GaussianMixture(Estimator):
    _params = _GMM_PARAMS

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        for k in ("seed", "weightCol"):
            self._defaultParamMap.pop(k, None)

    def _init(self, df, x: torch.Tensor, w, k: int, seed: int, lowp: bool = False):
        """Initial (weights, means, covariances). ``lowp``: ``x`` is a bf16 / e4m3 device column and ``w`` may be
        None; the sampled rows are widened after the gather and the variance comes from chunked sums."""
        comm = df._comm
        d = x.shape[1]
        n_samples = 5
        counts = comm.allgather_object(int(x.shape[0]))
        total = sum(counts)
        if total < k:
            raise ValueError(f"GaussianMixture: {total} rows < k = {k}")
        rng = np.random.default_rng(seed & 0xFFFFFFFF)
        picks = rng.integers(0, total, size=k * n_samples)  # global row ids, drawn order kept
        off = sum(counts[:comm.rank])
        pos = np.nonzero((picks >= off) & (picks < off + x.shape[0]))[0]
        idx = torch.as_tensor(picks[pos] - off, dtype=torch.int64, device=x.device)
        if lowp:
            from ..ops import gmm_ops as GO
            rows = GO.gather_rows(x, idx, d).cpu().numpy()
        else:
            rows = x[idx].cpu().numpy()
        samp = np.zeros((k * n_samples, d))
        for p_, r_ in comm.allgather_object((pos, rows)):
            samp[p_] = r_
        mus = samp.reshape(k, n_samples, d).mean(1)
        # diagonal of the (weighted) data variance
        if lowp:
            msg = GO.column_moments(x, d, w)
        else:
            W = w.sum()
            s1 = (w[:, None] * x).sum(0)
            s2 = (w[:, None] * x * x).sum(0)
            msg = torch.cat([W.reshape(1), s1, s2])
        comm.allreduce_(msg)
        o = msg.cpu().numpy()
        mean = o[1:1 + d] / o[0]
        var = np.clip(o[1 + d:] / o[0] - mean * mean, 1e-12, None)
        covs = np.stack([np.diag(var)] * k)
        return np.full(k, 1.0 / k), mus, covs

    def _fit(self, df):
        from .clustering import _weights
        from .tree_models import _default_seed
        x = df._feature_matrix(self.getFeaturesCol())
        k = self.getK()
        if k < 2:
            raise ValueError("GaussianMixture: k must be > 1")
        # Spark's non-negative-weight check, agreed over the ranks before the first collective of the fit
        w = _weights(df, self.getOrDefault("weightCol"), x.device) \
            if self.isSet("weightCol") and self.getOrDefault("weightCol") else None
        seed = int(self.getOrDefault("seed")) if self.isSet("seed") else _default_seed(U.jvm_class(self))
        comm = df._comm
        if _low_precision(x):
            return self._fit_low_precision(df, x, w, k, seed)
        x = x.to(torch.float64)
        n, d = x.shape
        if w is None:
            w = torch.ones(n, dtype=torch.float64, device=x.device)
        weights, mus, covs = self._init(df, x, w, k, seed)
        ll_prev, ll = -np.inf, -np.inf
        it = 0
        for it in range(1, self.getMaxIter() + 1):
            lp = _log_pdf(x, mus, covs) + torch.as_tensor(np.log(np.clip(weights, 1e-300, None)), device=x.device)
            lse = torch.logsumexp(lp, 1)
            R = torch.exp(lp - lse[:, None]) * w[:, None]  # weighted responsibilities [n, k]
            S0 = R.sum(0)
            S1 = R.T @ x
            S2 = torch.stack([(R[:, j:j + 1] * x).T @ x for j in range(k)])
            msg = torch.cat([S0, S1.reshape(-1), S2.reshape(-1), (w * lse).sum().reshape(1), w.sum().reshape(1)])
            comm.allreduce_(msg)
            weights, mus, covs, ll = _m_step(msg.cpu().numpy(), k, d)
            if abs(ll - ll_prev) < self.getTol():
                break
            ll_prev = ll
        return self._model(df, weights, mus, covs, ll, it)

    def _model(self, df, weights, mus, covs, ll, it):
        model = GaussianMixtureModel(weights, mus, covs)
        self._copyValues(model)
        model._attach_summary(GaussianMixtureSummary(model, df, ll, it))
        return model

    def _fit_low_precision(self, df, x: torch.Tensor, w: Optional[torch.Tensor], k: int, seed: int):
        """bf16 / e4m3 device rows: the same EM with the E-step of ``ops/gmm_ops.py`` on the rows as they are."""
        from ..ops import gmm_ops as GO
        d = int(x.shape[1])
        comm = df._comm
        kernel = use_kernel(GO, x, k)
        weights, mus, covs = self._init(df, x, w, k, seed, lowp=True)
        if kernel:
            from ..models.kmeans import to_device_matrix
            x = to_device_matrix(x, d)  # a copy only when the layout is not already the kernel's
        ll_prev, ll = -np.inf, -np.inf
        it = 0
        for it in range(1, self.getMaxIter() + 1):
            A, c = _estep_tables(weights, covs)
            stats, tail = (GO.estep if kernel else GO.estep_reference)(x, d, w, A, mus, c)
            msg = torch.cat([stats[:, 0], stats[:, 1:1 + d].reshape(-1), stats[:, 1 + d:].reshape(-1), tail])
            comm.allreduce_(msg)
            weights, mus, covs, ll = _m_step(msg.cpu().numpy(), k, d)
            if abs(ll - ll_prev) < self.getTol():
                break
            ll_prev = ll
        return self._model(df, weights, mus, covs, ll, it)


class GaussianMixtureModel(Model):
    _params = _GMM_PARAMS

    def __init__(self, weights=None, mus=None, covs=None):
        super().__init__()
        self._w = np.asarray(weights if weights is not None else [], dtype=np.float64)
        self._mu = np.asarray(mus if mus is not None else np.zeros((0, 0)), dtype=np.float64)
        self._cov = np.asarray(covs if covs is not None else np.zeros((0, 0, 0)), dtype=np.float64)
        self._summary = None

    @property
    def weights(self) -> List[float]:
        return self._w.tolist()

    @property
    def gaussians(self):
        return [(DenseVector(m), DenseMatrix(c.shape[0], c.shape[1], c.T.reshape(-1))) for m, c in
                zip(self._mu, self._cov)]

    @property
    def gaussiansDF(self):
        from ..sql.builder import rows_round_robin
        schema = T.StructType([T.StructField("mean", T.VectorUDT(), False), T.StructField("cov", T.MatrixUDT(), False)])
        sess = self._session()
        return rows_round_robin(sess, schema, [[m, c] for m, c in self.gaussians])

    @staticmethod
    def _session():
        from ..sql.session import SparkSession
        return SparkSession.builder.getOrCreate()

    def _probs_labels(self, x: torch.Tensor):
        """``(prob [n, k], label int32 [n])``; bf16 / e4m3 device rows go through ``ops/gmm_ops.py``."""
        if not _low_precision(x):
            p = self._probs(x)
            return p, torch.argmax(p, 1).to(torch.int32)
        from ..ops import gmm_ops as GO
        d = int(x.shape[1])
        A, c = _estep_tables(self._w, self._cov)
        if use_kernel(GO, x, len(self._w)):
            from ..models.kmeans import to_device_matrix
            return GO.predict(to_device_matrix(x, d), d, A, self._mu, c)
        return GO.predict_reference(x, d, None, A, self._mu, c)

    def _probs(self, x: torch.Tensor) -> torch.Tensor:
        if _low_precision(x):
            return self._probs_labels(x)[0]
        lp = _log_pdf(x.to(torch.float64), self._mu, self._cov) + torch.as_tensor(
            np.log(np.clip(self._w, 1e-300, None)), device=x.device)
        return torch.softmax(lp, 1)

    def _transform(self, df):
        p, lab = self._probs_labels(df._feature_matrix(self.getFeaturesCol()))
        out = df
        if self.getProbabilityCol():
            out = _replace_col(out, self.getProbabilityCol(), ColumnData(p.contiguous(), None, T.VectorUDT()))
        return _replace_col(out, self.getPredictionCol(),
                            ColumnData(lab, None, T.IntegerType()))

    def predict(self, value) -> int:
        from .linalg import as_array
        return int(torch.argmax(self._probs(torch.as_tensor(as_array(value), dtype=torch.float64)[None, :]), 1)[0])

    def predictProbability(self, value) -> DenseVector:
        from .linalg import as_array
        return DenseVector(self._probs(torch.as_tensor(as_array(value), dtype=torch.float64)[None, :])[0].numpy())

    def _save_impl(self, path):
        import pyarrow as pa
        U.write_metadata(self, path)
        U.write_parquet(path, "data", pa.Table.from_pylist(
            [{"weights": self._w.tolist(), "mus": [U.vector_struct(m) for m in self._mu],
              "sigmas": [U.matrix_struct(c) for c in self._cov]}],
            schema=pa.schema([("weights", pa.list_(pa.float64())), ("mus", pa.list_(U.vector_arrow_type())),
                              ("sigmas", pa.list_(U.matrix_arrow_type()))])))

    @classmethod
    def _load_impl(cls, path, md):
        r = U.read_parquet(path, "data").to_pylist()[0]
        m = cls(r["weights"], np.stack([U.vector_from_struct(v) for v in r["mus"]]),
                np.stack([U.matrix_from_struct(s) for s in r["sigmas"]]))
        U.apply_params(m, md)
        return m


class GaussianMixtureSummary:
    def __init__(self, model, df, ll, iters):
        self._model, self._df = model, df
        self.logLikelihood = float(ll)
        self.numIter = int(iters)
        self.k = len(model._w)
        self.featuresCol = model.getFeaturesCol()
        self.predictionCol = model.getPredictionCol()
        self.probabilityCol = model.getProbabilityCol()
        self._pred = None

    @property
    def predictions(self):
        if self._pred is None:
            self._pred = self._model.transform(self._df)
        return self._pred

    @property
    def cluster(self):
        return self.predictions.select(self.predictionCol)

    @property
    def probability(self):
        return self.predictions.select(self.probabilityCol)

    @property
    def clusterSizes(self) -> List[int]:
        pred = self.predictions._column_data(self.predictionCol).values.to(torch.int64)
        c = torch.bincount(pred, minlength=self.k).to(torch.float64)
        self._df._comm.allreduce_(c)
        return [int(v) for v in c.cpu().tolist()]


__all__ = ["GaussianMixture", "GaussianMixtureModel", "GaussianMixtureSummary"]
