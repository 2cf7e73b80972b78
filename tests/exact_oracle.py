"""Exact oracles and checkers for the source-precision KMeans kernels (``_native/csrc/kmeans_exact.hip``).

Plain numpy and Python (``fractions.Fraction``): nothing here imports the package.  The helpers of
``cert_oracle`` (directed roundings, the rational window, the row-list check, bf16 rounding, exact
cluster sums) are imported, not copied.  ``tests/test_exact_oracle.py`` checks these oracles against
the host twin and shows that every checker fails on a mutated output;
``tests/test_kmeans_exact_kernels_gpu.py`` feeds the kernels' outputs to the same checkers.

Rules (those of ``cert_oracle``).  Bit equality is asked only where every device operation is one IEEE
operation, an explicit ``__fma_rn`` or an explicit rounding: the distance fold (``fma_fold``), labels,
lists, counts, the bf16 layouts, the double-double sums of exactly summable rows.  Everything else is
checked for soundness with no tolerance and for tightness inside a window written down from the code's
constants, in rational arithmetic:

  W            2^-23 + 3e-10 (cert_oracle): the outward f32 rounding, kFoldMargin = 1e-10 and the f64
               fold error, for ub / lb of exact_top2 and u_out / l_out of screen_cert;
  W_ERR        to_bf16_err's last line, err = (float)(sqrt(e2) * (1 + 1e-6)) + 1e-30f: the factor
               1 + 1e-6, the f32 roundings to nearest of the product and of the sum (2^-23 together)
               and the absolute term 1e-30, rounded with the sum: err <= true (1 + 1e-6)(1 + 2^-23) +
               1e-30 (1 + 2^-23);
  W_SPLIT      ea / eb / en = f32_up(sqrt(fold) * (1 + 1e-6)): 1e-6 + 2^-23 (one directed rounding)
               + ROOM = 1e-12 (the f64 fold of at most 11 fmas per lane, the 4-step 16-lane
               reduction, the square root and the product: < 20 roundings of 2^-53 = 2.3e-15); eb
               has the absolute term 1e-300 inside f32_up, which the check subtracts from eb (times 1 + 2^-23) first;
  xn           (float) of the f64 fold: one rounding to nearest, 2^-24, plus the same ROOM.
"""
import math
from fractions import Fraction

import numpy as np

from cert_oracle import (C1E6, C101, F32_EPS, FOLD_MARGIN, GAP, W, W_LIST, bf16_bits, bf16_value, bits32,  # noqa: F401
                         bits64, check_row_list, check_window, dd_rel, exact_cluster_sums, f32_dn, f32_up, fr,
                         fsum_clusters, is_dyadic, list_slack, sqdist_fraction)

ROOM = Fraction(1, 10 ** 12)
W_ERR = (1 + Fraction(1, 10 ** 6)) * (1 + F32_EPS) - 1
ERR_ABS = Fraction(1, 10 ** 30) * (1 + F32_EPS)
W_SPLIT = Fraction(1, 10 ** 6) + F32_EPS + ROOM
W_XN = Fraction(1, 2 ** 24) + ROOM


# ---------------------------------------------------------------------------------------------- the fold

def fma_fold(x, c):
    """acc = fma(e, e, acc) with e = x_t - c_t in f64, t ascending from 0.0: the kernels' fold.
    float(Fraction) is correctly rounded, so each step is one fma exactly."""
    acc = 0.0
    for a, b in zip(np.asarray(x, dtype=np.float64).tolist(), np.asarray(c, dtype=np.float64).tolist()):
        e = Fraction(a - b)
        acc = float(e * e + Fraction(acc))
    return acc


def argmin_top2(vals):
    """(index of the smallest with strict < in index order, smallest, second smallest; +inf for one)."""
    bi, bd, sd = 0, math.inf, math.inf
    for j, v in enumerate(vals):
        if v < bd:
            sd, bd, bi = bd, v, j
        elif v < sd:
            sd = v
    return bi, bd, sd


def assign_fold(X, C, rows=None):
    """The fold assignment of the given rows (all by default): labels, best, second as arrays."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    out = [argmin_top2([fma_fold(X[r], c) for c in C]) for r in rows]
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.float64))


def is_lattice(*arrays):
    """is_dyadic, or half-integers of size <= 512 in rows of at most 4096 entries (the d > 1024 cases,
    which is_dyadic's row length refuses): differences are multiples of 1/2 below 2^10, squares
    multiples of 1/4 below 2^20, a row of them sums below 2^32 — 34 bits, exact in f64 in any order."""
    if is_dyadic(*arrays):
        return True
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        if a.size and (a.shape[-1] > 4096 or not np.all(np.abs(a) <= 512.0) or not np.array_equal(np.floor(a * 2), a * 2)):
            return False
    return True


def assign_lattice(X, C, chunk=1 << 15):
    """Exact (labels, best, second) on lattice data in plain numpy: every squared distance is exact in
    f64, so it is the fold's value too, whatever the order."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    assert is_lattice(X, C)
    n, k = X.shape[0], C.shape[0]
    lab, bd, sd = np.empty(n, dtype=np.int64), np.empty(n), np.full(n, np.inf)
    for s in range(0, n, chunk):
        xb = X[s:s + chunk]
        D2 = np.stack([((xb - c) ** 2).sum(axis=1) for c in C], axis=1)
        lab[s:s + chunk] = np.argmin(D2, axis=1)          # the first of equal minima: strict < in index order
        if k > 1:
            part = np.partition(D2, 1, axis=1)
            bd[s:s + chunk], sd[s:s + chunk] = part[:, 0], part[:, 1]
        else:
            bd[s:s + chunk] = D2[:, 0]
    return lab, bd, sd


def check_assign(ref_lab, ref_best, labels, best, rows=None, lab0=None, best0=None, changed=None, where=None):
    """labels / best of the rows ``rows`` (all by default) equal the oracle's bit for bit — ``ref_*``
    are indexed like ``where`` (the rows the oracle was computed for; all by default) —, every other
    row keeps what it held before (``lab0`` / ``best0``), and ``changed`` counts the labels that
    differ from ``lab0``."""
    labels = np.asarray(labels).astype(np.int64)
    n = labels.size
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    where = np.arange(n) if where is None else np.asarray(where, dtype=np.int64)
    pos = np.full(n, -1, dtype=np.int64)
    pos[where] = np.arange(where.size)
    listed = np.zeros(n, dtype=bool)
    listed[rows] = True
    sel = where[listed[where]]
    assert sel.size or not rows.size or not where.size
    bad = sel[labels[sel] != np.asarray(ref_lab)[pos[sel]]]
    assert bad.size == 0, f"labels differ from the oracle's argmin at rows {bad[:5]}"
    if best is not None:
        bad = sel[bits64(np.asarray(best)[sel]) != bits64(np.asarray(ref_best)[pos[sel]])]
        assert bad.size == 0, f"best differs in bits from the t-ascending fma fold at rows {bad[:5]}"
    if lab0 is not None:
        assert np.array_equal(labels[~listed], np.asarray(lab0)[~listed]), "an unlisted row's label changed"
        if best is not None and best0 is not None:
            assert np.array_equal(bits64(np.asarray(best)[~listed]), bits64(np.asarray(best0)[~listed])), \
                "an unlisted row's best changed"
        if changed is not None:
            want = int((labels[rows] != np.asarray(lab0)[rows]).sum())
            assert int(changed) == want, f"changed = {int(changed)}, {want} labels differ from the earlier ones"


def tight_up(q):
    """The least f32 whose square is >= the Fraction q."""
    f = np.float32(math.sqrt(float(q)))
    while fr(f) ** 2 < q:
        f = np.nextafter(f, np.float32(np.inf))
    while f > 0 and fr(np.nextafter(f, np.float32(0))) ** 2 >= q:
        f = np.nextafter(f, np.float32(0))
    return np.float32(f)


def tight_dn(q):
    """The largest f32 whose square is <= the Fraction q."""
    f = np.float32(math.sqrt(float(q)))
    while fr(f) ** 2 > q:
        f = np.nextafter(f, np.float32(0))
    while fr(np.nextafter(f, np.float32(np.inf))) ** 2 <= q:
        f = np.nextafter(f, np.float32(np.inf))
    return np.float32(f)


def exact_top2_fraction(X, C, rows):
    """Per row: the exact squared distances (Fractions) to the nearest centre and to the nearest of all
    others (None for k = 1)."""
    out1, out2 = [], []
    for r in rows:
        q = sorted(sqdist_fraction(X[r], c) for c in C)
        out1.append(q[0])
        out2.append(q[1] if len(q) > 1 else None)
    return out1, out2


def check_top2_bounds(ub, lb, D1, D2, rows):
    """ub[rows] / lb[rows] against the exact squared distances D1 (nearest) and D2 (second nearest; None or
    +inf for k = 1, where lb must be +inf): sound, inside W, exactly 0 on a true 0.  D1 / D2 are exact f64
    arrays (lattice) or lists of Fractions.  Returns (worst ub/true - 1, worst 1 - lb/true)."""
    rows = np.asarray(rows, dtype=np.int64)
    ub, lb = np.asarray(ub, dtype=np.float32)[rows], np.asarray(lb, dtype=np.float32)[rows]
    if rows.size == 0:
        return 0.0, 0.0
    wu = check_window(ub, D1, upper=True)
    one = (D2 is None) or (isinstance(D2, np.ndarray) and D2.size and np.all(np.isinf(D2))) or \
        (not isinstance(D2, np.ndarray) and len(D2) and D2[0] is None)
    if one:
        assert np.all(lb == np.inf), "k = 1: lb must be +inf"
        return wu, 0.0
    return wu, check_window(lb, D2, upper=False)


def check_moves(mv, lst, old, new, m0=0, fill=-1):
    """The move log (rows, old, new, count) holds {(r, old[r], new[r]) : old != new} of the listed rows as
    a set, after the ``m0`` entries it held before, with the right count and nothing past it."""
    mr, mo, mn, mc = (np.asarray(a) for a in mv)
    m1 = int(mc.reshape(-1)[0])
    lst = np.asarray(lst, dtype=np.int64)
    old, new = np.asarray(old), np.asarray(new)
    want = sorted((int(r), int(old[r]), int(new[r])) for r in lst if old[r] != new[r])
    assert m1 - m0 == len(want), f"{m1 - m0} moves logged, {len(want)} expected"
    got = sorted(zip(mr[m0:m1].tolist(), mo[m0:m1].tolist(), mn[m0:m1].tolist()))
    assert got == want, "the logged moves differ from the oracle's"
    for a in (mr, mo, mn):
        assert np.all(a[m1:] == fill), "the move log was written past its count"


def check_list(lst, count, expected, fill=-1, what="list"):
    """check_row_list, and the sentinel in every entry past the count."""
    check_row_list(lst, count, expected, what)
    assert np.all(np.asarray(lst)[int(count):] == fill), f"{what} was written past its count"


# ---------------------------------------------------------------------------------------------- bf16 copies

def _sumsq_fraction(row):
    return sum((fr(v) ** 2 for v in row), Fraction(0))


def err_oracle(X, d, ldo):
    """(bf16 bits [n, ldo] of f64 -> f32 -> bf16 with zero padding, the rounding errors x - bf16(x) as
    f64: exact, the bf16 value holds leading bits of x)."""
    X = np.asarray(X, dtype=np.float64)[:, :d]
    out = np.zeros((X.shape[0], ldo), dtype=np.uint16)
    hb = bf16_bits(X.astype(np.float32))
    out[:, :d] = hb
    return out, X - bf16_value(hb).astype(np.float64)


def check_bf16_err(X, d, ldo, out_bits, err):
    """to_bf16_err's outputs; returns the worst err/true - 1 over the rows whose true error is not 0."""
    want, e = err_oracle(X, d, ldo)
    out_bits = np.asarray(out_bits)
    assert out_bits.shape == want.shape
    assert not out_bits[:, d:].any(), "a padding element is not zero"
    assert np.array_equal(out_bits, want), "the bf16 copy differs from f64 -> f32 -> bf16 (nearest even)"
    err = np.asarray(err, dtype=np.float32)
    assert not np.any(np.isnan(err))
    worst = 0.0
    dy = is_dyadic(e * 2.0 ** 16) if e.size else True   # errors of dyadic data: exact squares and sums
    for r in range(e.shape[0]):
        q = fr((e[r] * e[r]).sum()) if dy else _sumsq_fraction(e[r])
        v = fr(err[r])
        assert v > 0 and v ** 2 >= q, f"row {r}: err² = {float(v) ** 2!r} is below the exact {float(q)!r}"
        # err <= true (1 + W_ERR) + ERR_ABS, on squares: (err - ERR_ABS)² <= q (1 + W_ERR)²
        assert v <= ERR_ABS or (v - ERR_ABS) ** 2 <= q * (1 + W_ERR) ** 2, f"row {r}: err = {err[r]!r} is loose"
        if q > 0:
            worst = max(worst, float(v) / math.sqrt(float(q)) - 1.0)
    return worst


def split_rows_oracle(X, d, ds, ldo):
    """[hi | lo | hi] as uint16 [n, ldo] (hi = bf16(f32(x)), lo = bf16(f32(x - hi)), zero elsewhere), and
    the parts lo and x - hi - lo as f64 (both subtractions are exact)."""
    X = np.asarray(X, dtype=np.float64)[:, :d]
    hb = bf16_bits(X.astype(np.float32))
    r1 = X - bf16_value(hb).astype(np.float64)
    lb = bf16_bits(r1.astype(np.float32))
    lo = bf16_value(lb).astype(np.float64)
    out = np.zeros((X.shape[0], ldo), dtype=np.uint16)
    out[:, :d] = hb
    out[:, ds:ds + d] = lb
    out[:, 2 * ds:2 * ds + d] = hb
    return out, lo, r1 - lo


def _check_norm(v, q, w, what, r, abs_term=Fraction(0)):
    """f32 ``v`` is a sound upper bound of sqrt(q) and v - abs_term within (1 + w) of it; 0 for 0."""
    v = fr(v)
    assert v >= 0 and v ** 2 >= q, f"row {r}: {what}² is below the exact {float(q)!r}"
    if q == 0 and abs_term == 0:
        assert v == 0, f"row {r}: {what} of a true 0 must be 0"
        return 0.0
    assert v <= abs_term or (v - abs_term) ** 2 <= q * (1 + w) ** 2, f"row {r}: {what} = {float(v)!r} is loose"
    return float(v) / math.sqrt(float(q)) - 1.0 if q > 0 else 0.0


def check_split_rows(X, d, ds, ldo, out_bits, ea, eb, en, xn, rows=None):
    """to_bf16_split's outputs: the layout bit for bit on every row; the four norms on ``rows`` (all by
    default) in rationals.  Returns the worst (ea, eb, en) / true - 1 and the worst |xn / true - 1|."""
    want, lo, rx = split_rows_oracle(X, d, ds, ldo)
    out_bits = np.asarray(out_bits)
    assert out_bits.shape == want.shape
    pad = np.ones(ldo, dtype=bool)
    for s in (0, ds, 2 * ds):
        pad[s:s + d] = False
    assert not out_bits[:, pad].any(), "a padding element is not zero"
    assert np.array_equal(out_bits[:, ds:ds + d], want[:, ds:ds + d]), \
        "the lo segment differs from bf16(f32(x - hi)) (the remainder is rounded through f32)"
    assert np.array_equal(out_bits, want), "the layout [hi | lo | hi] differs"
    X = np.asarray(X, dtype=np.float64)[:, :d]
    rows = range(X.shape[0]) if rows is None else rows
    wa = wb = wn = wx = 0.0
    tiny = Fraction(1e-300) * (1 + F32_EPS)
    for r in rows:
        wa = max(wa, _check_norm(ea[r], _sumsq_fraction(lo[r]), W_SPLIT, "ea", r))
        qb = _sumsq_fraction(rx[r])
        v = fr(eb[r])
        assert v > 0, f"row {r}: eb carries the absolute term 1e-300 and is never 0"
        if qb == 0:   # f32_up(1e-300): the smallest positive f32
            assert np.float32(eb[r]) == np.nextafter(np.float32(0), np.float32(1)), f"row {r}: eb of a true 0"
        else:
            wb = max(wb, _check_norm(eb[r], qb, W_SPLIT, "eb", r, abs_term=tiny))
        q = _sumsq_fraction(X[r])
        wn = max(wn, _check_norm(en[r], q, W_SPLIT, "en", r))
        assert abs(fr(xn[r]) - q) <= q * W_XN, f"row {r}: xn = {xn[r]!r} is more than an f32 rounding off"
        if q > 0:
            wx = max(wx, abs(float(fr(xn[r]) / q) - 1.0))
    return wa, wb, wn, wx


# ---------------------------------------------------------------------------------------------- screen_cert

def cert_decision(ub, lb, err, ecmax):
    """(listed, on the line, margin): listed = not (lb - ub > 2 (err + ecmax)) exactly — the data is
    dyadic, so f64 is exact —; margin = (lb - ub) / (2 e) - 1 for the rows above the line."""
    ub, lb, err = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (ub, lb, err))
    e2 = 2.0 * (err + float(ecmax))
    gap = lb - ub
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(gap > e2, gap / e2 - 1.0, 0.0)
    return ~(gap > e2), gap == e2, margin


def cert_case_is_exact(ub, lb, err, ecmax):
    """Every value is a multiple of 2^-8 below 2^10: ub + e, lb - e and their squares are exact in f64."""
    for a in (ub, lb, err, [ecmax]):
        a = np.asarray(a, dtype=np.float64)
        if not (np.all(np.abs(a) < 1024.0) and np.array_equal(np.floor(a * 256.0), a * 256.0)):
            return False
    return True


def check_screen_cert(case, lst, count, u_out=None, l_out=None, fill=-1):
    """``case`` = dict(ub, lb, err, ecmax) of dyadic values whose rows are on the line, at least GAP above
    it or below it (test_exact_oracle.py proves that).  Returns (worst u/true - 1, 1 - l/true)."""
    listed, _, _ = cert_decision(case["ub"], case["lb"], case["err"], case["ecmax"])
    check_list(lst, count, np.nonzero(listed)[0], fill, "the uncertified list")
    if u_out is None:
        return 0.0, 0.0
    ub, lb, err = (np.asarray(case[n], dtype=np.float32).astype(np.float64) for n in ("ub", "lb", "err"))
    e = err + float(case["ecmax"])
    wu = check_window(u_out, (ub + e) ** 2, upper=True)
    wl = check_window(l_out, np.maximum(lb - e, 0.0) ** 2, upper=False)
    return wu, wl


def check_screen_cert_split(case, lst, count, u_out, l_out, fill=-1):
    """``case`` = dict(ub, lb, ea, eb, en, cst).  The list is {i : not (u_out[i] < l_out[i])} from the
    outputs' own bits; u_out² >= ub² + E and l_out² <= max(lb² - E, 0) with E = 2 (ea c0 + eb c1 + 1.01 en
    c2) in rationals; inside W_LIST of the code's e = E (1 + 1e-6) (the premise |lb² - e| >= 1e-3 lb² is
    the cases', proven on the CPU); lb² < E gives 0 and a listed row.  Plain f64 decides the rows that
    stay 1e-11 inside both edges, Fractions the rest.  Returns (worst uu/true - 1, 1 - ll/true)."""
    u_out, l_out = np.asarray(u_out, dtype=np.float32), np.asarray(l_out, dtype=np.float32)
    assert not np.any(np.isnan(u_out)) and not np.any(np.isnan(l_out))
    check_list(lst, count, np.nonzero(~(u_out < l_out))[0], fill, "the uncertified list")
    on = np.zeros(u_out.size, dtype=bool)
    on[np.asarray(lst)[:int(count)].astype(np.int64)] = True
    ub, lb, ea, eb, en = (np.asarray(case[n], dtype=np.float32).astype(np.float64) for n in ("ub", "lb", "ea", "eb", "en"))
    c0, c1, c2 = (float(v) for v in case["cst"])
    e = 2.0 * (ea * c0 + eb * c1 + 1.01 * en * c2) * (1.0 + 1e-6)
    U2, L2 = ub * ub, lb * lb
    uu2, ll2 = u_out.astype(np.float64) ** 2, l_out.astype(np.float64) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        ru, rl = uu2 / (U2 + e), ll2 / (L2 - e)
    hi, lo = float((1 + W_LIST) ** 2), float((1 - W_LIST) ** 2)
    below = (L2 < e * (1 - 1e-11)) & (l_out == 0)              # lb² < E for sure: 0, and therefore listed
    assert np.all(on[below])
    sure = (ru >= 1 + 1e-11) & (ru <= hi * (1 - 1e-11)) & \
        (below | ((rl <= 1 - 1e-11) & (rl >= lo * (1 + 1e-11)) & (L2 > e)))
    wu = float(np.sqrt(ru[sure].max()) - 1.0) if sure.any() else 0.0
    live = sure & ~below
    wl = float(1.0 - np.sqrt(rl[live].min())) if live.any() else 0.0
    for r in np.nonzero(~sure)[0]:
        E, ec = list_slack(case, r)
        Uq, Lq, u2, l2 = fr(ub[r]) ** 2, fr(lb[r]) ** 2, fr(u_out[r]) ** 2, fr(l_out[r]) ** 2
        assert ec >= E and u2 >= Uq + E, f"row {r}: u_out is below sqrt(ub² + E)"
        assert u2 <= (Uq + ec) * (1 + W_LIST) ** 2, f"row {r}: u_out is loose"
        assert l2 <= max(Lq - E, 0), f"row {r}: l_out is above sqrt(max(lb² - E, 0))"
        if Lq < E:
            assert l_out[r] == 0 and on[r], f"row {r}: lb² < E must give l_out = 0 and a listed row"
        elif Lq > ec:
            assert l2 >= (Lq - ec) * (1 - W_LIST) ** 2, f"row {r}: l_out is loose"
            wl = max(wl, 1.0 - math.sqrt(float(l2 / (Lq - ec))))
        if Uq + ec > 0:
            wu = max(wu, math.sqrt(float(u2 / (Uq + ec))) - 1.0)
    return wu, wl


# ---------------------------------------------------------------------------------------------- sums

def check_sums(X, L, k, S, S_lo, cnt, exact_rows, cols=None, f32_rows=False):
    """exact_sums' outputs.  ``exact_rows``: the rows' exponents span far less than 2^80, so S is the
    correctly rounded exact sum bit for bit (math.fsum) and S + S_lo the exact sum (Fractions, on the
    columns ``cols``; all by default); otherwise (generic f64 rows) S + S_lo lies within the
    double-double error dd_rel(n + 32) of the summed sizes.  Returns that worst relative error."""
    X, L = np.asarray(X, dtype=np.float64), np.asarray(L, dtype=np.int64)
    n, d = X.shape
    S, S_lo = np.asarray(S, dtype=np.float64), np.asarray(S_lo, dtype=np.float64)
    assert np.array_equal(np.asarray(cnt).astype(np.int64), np.bincount(L, minlength=k)), "counts differ from bincount"
    assert np.array_equal(bits64(S + S_lo), bits64(S)), "S / S_lo are not normalised (fl(S + S_lo) != S)"
    want, _ = fsum_clusters(X, L, k)
    if exact_rows or f32_rows:
        assert np.array_equal(S, want), "S differs from the correctly rounded exact sums"
    cols = range(d) if cols is None else cols
    exact, mag = exact_cluster_sums(X[:, list(cols)], L, k)
    worst = 0.0
    for j in range(k):
        for i, t in enumerate(cols):
            err = abs(fr(S[j, t]) + fr(S_lo[j, t]) - exact[j][i])
            if exact_rows or f32_rows:
                assert err == 0, f"S + S_lo is not the exact sum at ({j}, {t})"
            else:
                assert err <= mag[j][i] * dd_rel(n + 32), f"S + S_lo is off the exact sum at ({j}, {t})"
                assert abs(fr(S[j, t]) - exact[j][i]) <= abs(exact[j][i]) * Fraction(1, 2 ** 53) + mag[j][i] * dd_rel(n + 32), \
                    f"S is not the rounded sum at ({j}, {t})"
                if mag[j][i]:
                    worst = max(worst, float(err / mag[j][i]))
    return worst


def check_sum_exact(v, out):
    """sum_exact's result is math.fsum's (the correctly rounded exact sum) bit for bit."""
    want = math.fsum(np.asarray(v, dtype=np.float64).tolist())
    assert float(out) == want and math.copysign(1.0, float(out) + 0.0) == math.copysign(1.0, want + 0.0), \
        f"sum_exact = {float(out)!r}, math.fsum = {want!r}"
