"""Exact oracles for the tree kernels K17-K21 (``_native/csrc/trees.hip``).

Plain numpy and Python: nothing here imports the package, so a mistake shared by the engine's GPU
and CPU branches cannot hide in these forms.  ``tests/test_tree_oracle.py`` checks the CPU branches
against them, ``tests/test_tree_kernels_gpu.py`` the kernels.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53          # unit roundoff of f64
TIE_REL = Fraction(1, 10 ** 12)   # the documented tie tolerance of K19 (kTreeTieRel)
KINDS = ("variance", "gini", "entropy")


# ---------------------------------------------------------------------------------------------- K17

def bin_codes(x, thr, nsplit):
    """Bin code of every cell: the number of the feature's thresholds below the value.

    ``thr`` is [d, max_splits] (only the first ``nsplit[f]`` entries of row f count).  numpy orders
    NaN above every number, so a NaN cell gets ``nsplit[f]``; -0.0 equals a threshold of 0.0."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    out = np.zeros((n, d), dtype=np.int64)
    for f in range(d):
        out[:, f] = np.searchsorted(np.asarray(thr[f, :nsplit[f]], dtype=np.float64), x[:, f], side="left")
    return out


# ---------------------------------------------------------------------------------------------- K18

def fixed_point_scales(n, wmax, ymax, variance):
    """The scales 2^e the engine documents: the largest e for which n * max w * max|y|^s fits 2^61."""
    out = np.ones(3)
    for s in range(3):
        bound = n * wmax * (ymax ** s if variance else 1.0)
        out[s] = 2.0 ** (61 - math.ceil(math.log2(bound)))
    return out


def histogram(bins, node_of, wt, y_or_cls, S, nodes, scales, nbins):
    """int64 [T, nodes, d, nbins, S] fixed-point statistics.

    ``y_or_cls`` of an integer type holds class indices (statistic c = weight of class c, scale 0);
    a float type holds regression labels (statistics w, w*y, w*y*y with scales 0, 1, 2).  Every row's
    statistic is the f64 product, times an exact power of two, rounded half to even.  Rows with
    ``node_of < 0`` or weight 0 contribute nothing.  ``wt`` is [T, n] float32 or None (weight 1)."""
    bins = np.asarray(bins).astype(np.int64)
    node_of = np.asarray(node_of)
    T, n = node_of.shape
    d = bins.shape[1]
    out = np.zeros((T, nodes, d, nbins, S), dtype=np.int64)
    classes = np.issubdtype(np.asarray(y_or_cls).dtype, np.integer)
    feat = np.arange(d)
    for t in range(T):
        w = np.ones(n) if wt is None else np.asarray(wt[t]).astype(np.float64)
        rows = np.nonzero((node_of[t] >= 0) & (w != 0.0))[0]
        if rows.size == 0:
            continue
        w = w[rows]
        nd = node_of[t][rows].astype(np.int64)
        b = bins[rows]
        if classes:
            q = np.rint(w * scales[0]).astype(np.int64)
            c = np.asarray(y_or_cls)[rows].astype(np.int64)
            np.add.at(out[t], (nd[:, None], feat[None, :], b, c[:, None]), q[:, None])
        else:
            y = np.asarray(y_or_cls, dtype=np.float64)[rows]
            wy = w * y
            for s, v in enumerate((w, wy, wy * y)):
                q = np.rint(v * scales[s]).astype(np.int64)
                np.add.at(out[t], (nd[:, None], feat[None, :], b, s), q[:, None])
    return out


# ---------------------------------------------------------------------------------------------- K19

def _frac_stats(ints, scales, kind):
    sc = scales[:len(ints)] if kind == "variance" else [scales[0]] * len(ints)
    return [Fraction(int(v)) / Fraction(float(s)) for v, s in zip(ints, sc)]


def _count(st, kind):
    return st[0] if kind == "variance" else sum(st)


def _variance(st):
    if st[0] <= 0:
        return Fraction(0)
    m = st[1] / st[0]
    return max(st[2] / st[0] - m * m, Fraction(0))


def _gini(st):
    tot = sum(st)
    if tot <= 0:
        return Fraction(0)
    return 1 - sum((c / tot) ** 2 for c in st)


def _entropy_terms(st, wtot):
    """The terms of (w / wtot) * H(st) = -sum_c (c / wtot) * log2(c / w)."""
    w = sum(st)
    return [-float(c / wtot) * math.log2(float(c / w)) for c in st if c > 0]


def gain_error_bound(kind, S, tot, pure):
    """``err`` of best_split; see there."""
    if kind == "variance":
        return 32.0 * U * (float(tot[2] / tot[0]) if tot[0] > 0 else 0.0)
    if pure:
        return 0.0
    if kind == "gini":
        return (8 * S + 16) * U
    H = max(1.0, math.log2(S))
    return (3 * (S + 2) + H * (6 * S + 14) + 6 * H + 4) * U


def best_split(hist_node, scales, kind, mask, nsplit, min_inst, min_wfrac, min_gain):
    """K19's rule on one node, in exact arithmetic.

    ``hist_node`` is the node's int64 [d, nbins, S] histogram.  Child and total statistics are
    ``int / scale`` as exact rationals; variance and gini gains are exact ``Fraction``s, entropy gains
    one ``math.fsum`` over the ``math.log2`` terms of the parent and both children (symmetric in the
    children).  A candidate (f, b) needs mask[f], b < nsplit[f], both children of positive weight and
    of at least max(min_inst, min_wfrac * w_total), and gain >= min_gain.  The answer is the first
    (f, b) in (feature, bin) order whose gain is at least G - TIE_REL * |G|, G the largest admissible
    gain; feature -1 when there is no candidate.

    ``err`` bounds |computed gain - exact gain| for any f64 evaluation of

        imp(tot) - (wl / wtot) * imp(left) - (wr / wtot) * imp(right)

    from statistics that are each one rounding (u = 2^-53, the int64 -> f64 conversion; the division
    by the power-of-two scale is exact) away from ``int / scale``.  First order in u, constants
    rounded up:

    * variance, imp = s2/w - (s1/w)^2 clamped at 0.  With A = s2/w: s1/w carries 3u (two inputs, one
      division), its square 7u, A carries 3u, the subtraction adds u of a result that is at most A,
      so |d imp| <= (3 + 7 + 1) u A = 11 u A, because (s1/w)^2 <= A; the clamp does not increase it.
      wl/wtot carries 3u and the product one more: each child term errs by at most
      (wl/wtot) * 15 u A_child, and sum_child (w_child/wtot) A_child = A_tot exactly (sum of w*y*y is
      additive).  The two final subtractions add 2 u A_tot at most.  Total (11 + 15 + 2) u A_tot,
      stated as 32 u A_tot: relative to sum(w y^2) / sum(w), the largest intermediate, NOT to the
      impurity (y = 1e6 + noise has A ~ 1e12 and impurity ~ 1).  A contraction of the subtraction
      into an fma only removes a rounding.
    * gini, imp = 1 - sum p_c^2, p_c = s_c / tot.  tot is S - 1 additions of rounded inputs: S u;
      p_c (S + 2) u; p_c^2 (2S + 5) u; the S subtractions from 1 stay within [0, 1]: S u.
      |d imp| <= (3S + 5) u.  A child term is (ratio, (2S + 1) u) * imp + u:
      (w_child/wtot) * (5S + 7) u, together (5S + 7) u; plus the parent's (3S + 5) u and 2u for the
      final subtractions: (8S + 14) u, stated as (8S + 16) u (largest intermediate: 1).
    * entropy, imp = -sum p_c log2 p_c <= H = log2 S.  log2 within 2 ulp; the error of p moves
      log2 p by (S + 2) u / ln 2 < 1.45 (S + 2) u.  Per impurity: 1.45 (S + 2) u + H (S + 5) u for the
      terms and S H u for the accumulation; a gain is two such (parent, children weighted to one)
      plus the ratios' (2S + 2) u H and 2 u H for the subtractions: < [3 (S + 2) + H (6S + 14)] u.
      This oracle's own float terms (three roundings each, sum of |terms| <= 2H, argument of log2
      rounded) add (6H + 4) u, included.  H is taken as at least 1.
    * a classification node with a single class present: every operation is exact (sums with 0,
      x / x = 1, 1 - 1 * 1 = 0, log2 1 = 0, products with 0), so err = 0 and the gain is exactly 0.
    """
    h = np.asarray(hist_node)
    d, nbins, S = h.shape
    tot_i = [int(v) for v in h[0].sum(axis=0)]            # feature 0 covers every row once
    tot = _frac_stats(tot_i, scales, kind)
    wtot = _count(tot, kind)
    pure = kind != "variance" and sum(1 for v in tot_i if v != 0) <= 1
    err = gain_error_bound(kind, S, tot, pure)
    min_w = max(Fraction(min_inst), Fraction(float(min_wfrac)) * wtot)
    mg = Fraction(float(min_gain))
    if kind == "entropy":
        parent_terms = _entropy_terms(tot, wtot) if wtot > 0 else []
    else:
        imp_tot = _variance(tot) if kind == "variance" else _gini(tot)
    cands = []      # (f, b, gain, wl, wr, weight gates ok, admissible)
    for f in range(d):
        if not mask[f]:
            continue
        cum = [0] * S
        for b in range(int(nsplit[f])):
            cum = [c + int(v) for c, v in zip(cum, h[f, b])]
            ls = _frac_stats(cum, scales, kind)
            rs = _frac_stats([t - c for t, c in zip(tot_i, cum)], scales, kind)
            wl, wr = _count(ls, kind), _count(rs, kind)
            w_ok = wl >= min_w and wr >= min_w and wl > 0 and wr > 0
            if not (wl > 0 and wr > 0):
                cands.append((f, b, None, wl, wr, False, False))
                continue
            if kind == "variance":
                gain = imp_tot - (wl / wtot) * _variance(ls) - (wr / wtot) * _variance(rs)
            elif kind == "gini":
                gain = imp_tot - (wl / wtot) * _gini(ls) - (wr / wtot) * _gini(rs)
            else:
                gain = Fraction(math.fsum(parent_terms + [-v for v in _entropy_terms(ls, wtot)]
                                          + [-v for v in _entropy_terms(rs, wtot)]))
            cands.append((f, b, gain, wl, wr, w_ok, w_ok and gain >= mg))
    adm = [c for c in cands if c[6]]
    res = {"err": err, "candidates": cands, "tot_i": tot_i, "min_w": min_w, "G": None,
           "feature": -1, "bin": -1, "gain": None, "left_i": [0] * S, "right_i": list(tot_i)}
    # what would make the answer depend on rounding: a gate or the tie threshold within reach of a value
    amb = []
    for f, b, gain, wl, wr, w_ok, ok in cands:
        if gain is None:
            continue
        for w in (wl, wr):
            if w != min_w and abs(w - min_w) <= Fraction(1, 10 ** 9) * max(min_w, Fraction(1)):
                amb.append((f, b, "weight gate"))
        if w_ok and abs(gain - mg) < 2 * err:
            amb.append((f, b, "min_gain"))
    if adm:
        G = max(c[2] for c in adm)
        thr = G - TIE_REL * abs(G)
        amb += [(c[0], c[1], "tie") for c in adm if abs(c[2] - thr) < 2 * err]
        f, b, gain = next((c[0], c[1], c[2]) for c in adm if c[2] >= thr)
        left_i = [int(v) for v in h[f, :b + 1].sum(axis=0)]
        res.update(G=G, feature=f, bin=b, gain=gain, left_i=left_i,
                   right_i=[t - c for t, c in zip(tot_i, left_i)], tie_margin=float(TIE_REL * abs(G)))
    res["ambiguous"] = amb
    return res


def stats_f64(ints, scales, kind):
    """``int / scale`` in f64: the integer rounded to f64, divided by the power-of-two scale."""
    sc = np.asarray(scales[:len(ints)] if kind == "variance" else [scales[0]] * len(ints), dtype=np.float64)
    return np.array([float(v) for v in ints], dtype=np.float64) / sc


# ---------------------------------------------------------------------------------------------- K20

def route(bins, node_of, split_feat, split_bin, left_id, right_id):
    """New [T, n] node ids: a row at a node with split_feat < 0 retires (-1), a retired row stays
    retired, any other goes left when its bin code of the split feature is <= split_bin, else right.
    The split arrays are [T, nodes]."""
    bins = np.asarray(bins).astype(np.int64)
    node_of = np.asarray(node_of)
    out = node_of.copy()
    rows = np.arange(bins.shape[0])
    for t in range(node_of.shape[0]):
        act = node_of[t] >= 0
        k = node_of[t][act]
        f = split_feat[t][k]
        code = bins[rows[act], np.maximum(f, 0)]
        new = np.where(code <= split_bin[t][k], left_id[t][k], right_id[t][k])
        out[t][act] = np.where(f < 0, -1, new)
    return out


# ---------------------------------------------------------------------------------------------- K21

def predict(trees, x, S, average):
    """[n, S] sum of the leaf values each row reaches, tree by tree in order, then one true division
    by the tree count when ``average`` (and more than one tree).  A tree is a dict: a leaf
    ``{"value": [S floats]}`` or a split ``{"f", "thr", "left", "right"}``; a row goes left when
    ``x[f] <= thr`` (so NaN goes right)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((x.shape[0], S), dtype=np.float64)

    def descend(node, idx):
        if idx.size == 0:
            return
        if "value" in node:
            out[idx] += np.asarray(node["value"], dtype=np.float64)
            return
        with np.errstate(invalid="ignore"):
            go = x[idx, node["f"]] <= node["thr"]
        descend(node["left"], idx[go])
        descend(node["right"], idx[~go])

    for t in trees:
        descend(t, np.arange(x.shape[0]))
    if average and len(trees) > 1:
        out = out / np.float64(len(trees))
    return out
