"""Exact oracles and checkers for the certified pruned Lloyd step (``_native/csrc/kmeans_cert.hip``).

Plain numpy and Python (``fractions.Fraction``): nothing here imports the package, so a mistake in the
kernels cannot hide in these forms.  ``tests/test_cert_oracle.py`` checks the oracles and shows that
every checker fails on a mutated output; ``tests/test_kmeans_cert_kernels_gpu.py`` feeds the kernels'
outputs to the same checkers.

Rules.  The device code may contract ``a * b + c`` into one fma, so bit equality is asked only where
every operation is one IEEE operation or an explicit rounding (cert_bounds, the bf16 layout, integer
outputs, double-double sums of exactly summable data).  Every other bound is checked on both sides of
a window in exact rational arithmetic, on squares (no square root):

  soundness   u² >= D² (upper bounds), l² <= D² (lower bounds, half-separations): no tolerance;
  tightness   within the relative width W = 2^-23 + 3e-10: one f32 ulp of the outward rounding
              (2^-23 relative at most), kFoldMargin = 1e-10 of exact_util.h, and the f64 fold error
              (d + 6 roundings of 2^-53: < 1e-13 for d <= 512), with room to 3e-10.  A true value of 0
              must give exactly 0.
"""
import math
from fractions import Fraction

import numpy as np

F32_EPS = Fraction(1, 2 ** 23)
W = F32_EPS + Fraction(3, 10 ** 10)
FOLD_MARGIN = 1e-10       # kFoldMargin (exact_util.h)
KBUF = 2048               # kBuf (exact_util.h): the LDS list buffer of cert_bounds / cert_tighten
GAP = 4.0 * 2.0 ** -23    # list cases: test value and threshold are equal or this far apart (relative)


# ---------------------------------------------------------------------------------------------- numbers

def f32_up(v):
    """f64 -> f32 rounded towards +inf (NaN stays NaN)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.array(v.astype(np.float32), ndmin=1)
        m = f.astype(np.float64) < v.reshape(f.shape)
        f[m] = np.nextafter(f[m], np.float32(np.inf))
    return f.reshape(v.shape)


def f32_dn(v):
    """f64 -> f32 rounded towards 0 for positive values; everything that is not > 0 (NaN too) gives 0."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.array(v.astype(np.float32), ndmin=1)
        vv = v.reshape(f.shape)
        m = f.astype(np.float64) > vv
        f[m] = np.nextafter(f[m], np.float32(0))
        f[~(vv > 0)] = 0
    return f.reshape(v.shape)


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits32(a, b):
    """Bit equality of f32 arrays; a NaN matches any NaN (the payload of a converted NaN is free)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits32(a) == bits32(b)) | (np.isnan(a) & np.isnan(b))))


def is_dyadic(*arrays):
    """Multiples of 2^-8 below 2^10 in rows of at most 2^10 entries: differences are multiples of 2^-8
    below 2^11, their squares multiples of 2^-16 below 2^22, a row of them sums below 2^32 — 48 bits, so
    plain f64 differences, squares and sums of such data are exact (sums of up to 2^20 values too)."""
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        if a.size == 0:
            continue
        if a.shape[-1] > 1024 or not np.all(np.isfinite(a)) or not np.all(np.abs(a) < 1024.0):
            return False
        if not np.array_equal(np.floor(a * 256.0), a * 256.0):
            return False
    return True


def fr(x):
    return Fraction(float(x))


def sqdist_fraction(x, c):
    return sum(((fr(a) - fr(b)) ** 2 for a, b in zip(x, c)), Fraction(0))


def sqdist_rows(X, C, lab):
    """Exact squared distance of every row X[r] to C[lab[r]]: an exact f64 array on dyadic data, else a
    list of Fractions."""
    X, C, lab = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64), np.asarray(lab)
    if is_dyadic(X, C):
        e = X - C[lab]
        return (e * e).sum(axis=1)
    return [sqdist_fraction(X[r], C[lab[r]]) for r in range(X.shape[0])]


def sumsq_rows(A):
    """Exact squared norm of every row: exact f64 on dyadic data, else Fractions."""
    A = np.asarray(A, dtype=np.float64)
    if is_dyadic(A):
        return (A * A).sum(axis=1)
    return [sum((fr(v) ** 2 for v in row), Fraction(0)) for row in A]


# ---------------------------------------------------------------------------------------------- windows

def _window_one(v, D2, upper, w):
    v = float(v)
    assert not math.isnan(v), "NaN bound"
    D2 = D2 if isinstance(D2, Fraction) else fr(D2)
    if D2 == 0:
        assert v == 0.0, f"true value 0 must give exactly 0, got {v!r}"
        return 0.0
    V2 = fr(v) ** 2
    if upper:
        assert v > 0 and V2 >= D2, f"unsound upper bound {v!r}: its square is below the exact {float(D2)!r}"
        assert V2 <= D2 * (1 + w) ** 2, f"loose upper bound {v!r} for {float(D2) ** 0.5!r}"
        return math.sqrt(float(V2 / D2)) - 1.0
    assert v >= 0 and V2 <= D2, f"unsound lower bound {v!r}: its square is above the exact {float(D2)!r}"
    assert V2 >= D2 * (1 - w) ** 2, f"loose lower bound {v!r} for {float(D2) ** 0.5!r}"
    return 1.0 - math.sqrt(float(V2 / D2))


def check_window(vals, D2, upper, w=W):
    """Every f32 ``vals[i]`` is a sound bound of sqrt(D2[i]) (upper: >=, else <=) and within the
    relative width ``w`` of it; exactly 0 where D2 is 0.  ``D2`` is an exact f64 array (dyadic data:
    the squares of f32 values are exact in f64 too, so the soundness comparison is exact and only the
    rows near the edge of the tightness window go through Fractions) or a list of Fractions.
    Returns the worst observed u/true - 1 (upper) or 1 - l/true (lower)."""
    vals = np.asarray(vals, dtype=np.float32).reshape(-1)
    if not isinstance(D2, np.ndarray):
        assert len(D2) == vals.size
        return max([_window_one(v, q, upper, w) for v, q in zip(vals, D2)], default=0.0)
    D2 = D2.reshape(-1)
    assert D2.size == vals.size and not np.any(np.isnan(vals))
    v2 = vals.astype(np.float64) ** 2  # exact: 24-bit significands
    zero = D2 == 0
    assert np.all(vals[zero] == 0), "true value 0 must give exactly 0"
    nz = ~zero
    if upper:
        bad = nz & ~(v2 >= D2)
        assert not bad.any(), f"unsound upper bound at {np.nonzero(bad)[0][:5]}"
    else:
        bad = nz & ~((v2 <= D2) & (vals >= 0))
        assert not bad.any(), f"unsound lower bound at {np.nonzero(bad)[0][:5]}"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(nz, v2 / np.where(nz, D2, 1.0), 1.0)
    lim = float((1 + w) ** 2) if upper else float((1 - w) ** 2)
    edge = nz & ((ratio > lim * (1 - 1e-12)) if upper else (ratio < lim * (1 + 1e-12)))
    for i in np.nonzero(edge)[0]:
        _window_one(vals[i], D2[i], upper, w)
    worst = float(np.max(np.sqrt(ratio)) - 1.0) if upper else float(1.0 - np.min(np.sqrt(ratio)))
    return max(worst, 0.0)


def check_row_list(lst, count, expected, what="list"):
    """A device row list (unordered) holds exactly the expected rows, each once."""
    count = int(count)
    exp = np.sort(np.asarray(expected, dtype=np.int64))
    assert count == exp.size, f"{what}: {count} rows listed, {exp.size} expected"
    got = np.sort(np.asarray(lst)[:count].astype(np.int64))
    assert np.array_equal(got, exp), f"{what}: the listed rows differ from the oracle's"


# ---------------------------------------------------------------------------------------------- cert_stats

def stats_truth(C, Cold):
    """(sep2, dr2): the exact squared half-distance of every centre to the nearest other one (None for
    k = 1) and the exact squared drift — exact f64 arrays on dyadic data, else lists of Fractions."""
    C, Cold = np.asarray(C, dtype=np.float64), np.asarray(Cold, dtype=np.float64)
    k = C.shape[0]
    if is_dyadic(C, Cold):
        dr2 = ((C - Cold) ** 2).sum(axis=1)
        if k == 1:
            return None, dr2
        sep2 = np.empty(k)
        for j in range(k):
            g = ((C - C[j]) ** 2).sum(axis=1)
            g[j] = np.inf
            sep2[j] = g.min() / 4.0  # a power-of-two scaling: exact
        return sep2, dr2
    dr2 = [sqdist_fraction(C[j], Cold[j]) for j in range(k)]
    if k == 1:
        return None, dr2
    sep2 = [min(sqdist_fraction(C[j], C[i]) for i in range(k) if i != j) / 4 for j in range(k)]
    return sep2, dr2


def check_stats(C, Cold, s, drift, dtop, zero=None):
    """cert_stats' outputs; returns (worst drift/true - 1, worst 1 - s/true)."""
    s, drift, dtop = (np.asarray(a, dtype=np.float32) for a in (s, drift, dtop))
    k = np.asarray(C).shape[0]
    sep2, dr2 = stats_truth(C, Cold)
    if sep2 is None:
        assert s[0] == np.inf, "k = 1: the half-separation is +inf"
        lo = 0.0
    else:
        lo = check_window(s[:k], sep2, upper=False)
    up = check_window(drift[:k], dr2, upper=True)
    order = np.sort(drift[:k].astype(np.float64))
    top, second = order[-1], (order[-2] if k > 1 else 0.0)
    assert float(dtop[0]) == top, f"dtop[0] = {dtop[0]!r} is not the largest drift {top!r}"
    assert float(dtop[1]) == second, f"dtop[1] = {dtop[1]!r} is not the second largest drift {second!r}"
    i1 = float(dtop[2])
    assert i1 == int(i1) and 0 <= int(i1) < k, f"dtop[2] = {i1!r} is no centre index"
    assert float(drift[int(i1)]) == top, f"dtop[2] = {int(i1)} does not hold the largest drift"
    if zero is not None:
        assert not np.any(np.asarray(zero)), "the zero buffer is not all zero"
    return up, lo


# ---------------------------------------------------------------------------------------------- cert_bounds

def bounds_oracle(lab, u, l, drift, dtop, s):
    """(u', l', listed rows) of cert_bounds: single IEEE operations and explicit roundings only."""
    lab = np.asarray(lab, dtype=np.int64)
    u, l, drift, dtop, s = (np.asarray(a, dtype=np.float32) for a in (u, l, drift, dtop, s))
    d1, d2, i1 = float(dtop[0]), float(dtop[1]), int(dtop[2])
    with np.errstate(invalid="ignore"):
        un = f32_up(u.astype(np.float64) + drift[lab].astype(np.float64))
        ln = f32_dn(l.astype(np.float64) - np.where(lab == i1, d2, d1))
        thr = np.where(np.isnan(ln) | (ln < s[lab]), s[lab], ln)  # fmaxf
        listed = np.nonzero(~(un < thr))[0]
    return un, ln, listed


def check_bounds(inp, u_out, l_out, lst, count, fill=-1):
    """``inp`` = dict(lab, u, l, drift, dtop, s); ``lst`` is the whole list buffer, which was filled
    with ``fill`` before the call: entries past the count stay untouched."""
    un, ln, listed = bounds_oracle(inp["lab"], inp["u"], inp["l"], inp["drift"], inp["dtop"], inp["s"])
    assert same_bits32(u_out, un), "u' differs from f32_up(f64(u) + f64(drift[lab]))"
    assert same_bits32(l_out, ln), "l' differs from f32_dn(f64(l) - (lab == i1 ? d2 : d1))"
    check_row_list(lst, count, listed, "list A")
    assert np.all(np.asarray(lst)[int(count):] == fill), "list A was written past its count"
    return listed


# ---------------------------------------------------------------------------------------------- cert_tighten

def tighten_oracle(X, C, lab, l, s, la):
    """For the rows of list A: the exact squared distance to the label's centre, the kernel's formula
    in numpy (u_or = f32_up(sqrt(D2) * (1 + kFoldMargin)); the device value may differ in the last
    places where the square root is inexact), the threshold max(l, s[lab]) and the rows that stay
    unproven by u_or."""
    la = np.asarray(la, dtype=np.int64)
    lab = np.asarray(lab, dtype=np.int64)
    Xa = np.asarray(X, dtype=np.float64)[la]
    D2 = sqdist_rows(Xa, C, lab[la])
    D2f = D2 if isinstance(D2, np.ndarray) else np.array([float(q) for q in D2])
    u_or = f32_up(np.sqrt(D2f) * (1.0 + FOLD_MARGIN))
    thr = np.maximum(np.asarray(l, dtype=np.float32)[la], np.asarray(s, dtype=np.float32)[lab[la]])
    listed = la[~(u_or < thr)]
    return D2, u_or, thr, listed


def gap_holds(value, thr):
    """Every test value equals its threshold or lies GAP (relative, >= 4 f32 ulps) away from it."""
    value, thr = np.asarray(value, dtype=np.float64), np.asarray(thr, dtype=np.float64)
    big = np.maximum(np.abs(value), np.abs(thr))
    return bool(np.all((value == thr) | (np.abs(value - thr) >= GAP * big) | np.isinf(thr)))


def check_tighten(case, u_after, lbst, nb, bxn=None, blab=None, fill=-1):
    """``case`` = dict(X, C, lab, u, l, s, la, xn); returns the worst u/true - 1 over list A."""
    la = np.asarray(case["la"], dtype=np.int64)[:case["na"]]
    u0, u1 = np.asarray(case["u"], dtype=np.float32), np.asarray(u_after, dtype=np.float32)
    D2, _, _, listed = tighten_oracle(case["X"], case["C"], case["lab"], case["l"], case["s"], la)
    rest = np.ones(u0.size, dtype=bool)
    rest[la] = False
    assert np.array_equal(bits32(u0[rest]), bits32(u1[rest])), "a row outside list A changed its u"
    worst = check_window(u1[la], D2, upper=True) if la.size else 0.0
    check_row_list(lbst, nb, listed, "list B")
    assert np.all(np.asarray(lbst)[int(nb):] == fill), "list B was written past its count"
    if bxn is not None:
        rows = np.asarray(lbst)[:int(nb)].astype(np.int64)
        assert np.array_equal(bits32(np.asarray(bxn)[:int(nb)]), bits32(np.asarray(case["xn"])[rows])), "bxn"
        assert np.array_equal(np.asarray(blab)[:int(nb)], np.asarray(case["lab"])[rows]), "blab"
    return worst


# ---------------------------------------------------------------------------------------------- split_centres

def bf16_bits(f):
    """bf16 bit pattern (uint16) of f32 values, round to nearest even (finite inputs)."""
    b = bits32(f).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_oracle(C, kp, ds, ldc):
    """The layout [c_hi | c_hi | c_lo] as uint16 [kp, ldc] (f64 -> f32 -> bf16, each to nearest even),
    and the parts c_lo and c - c_hi - c_lo as f64 (the subtractions are exact: Sterbenz-like, the bf16
    parts are leading bits of the value)."""
    C = np.asarray(C, dtype=np.float64)
    k, d = C.shape
    hb = bf16_bits(C.astype(np.float32))
    r1 = C - bf16_value(hb).astype(np.float64)
    lb = bf16_bits(r1.astype(np.float32))
    lo = bf16_value(lb).astype(np.float64)
    rc = r1 - lo
    cb = np.zeros((kp, ldc), dtype=np.uint16)
    cb[:k, :d] = hb
    cb[:k, ds:ds + d] = hb
    cb[:k, 2 * ds:2 * ds + d] = lb
    return cb, lo, rc


def _max_fraction(q):
    return max((fr(v) if not isinstance(v, Fraction) else v) for v in q)


def check_split(C, kp, ds, cb_bits, cn, cst, mc):
    """split_centres' outputs (``cb_bits``: the bf16 buffer as uint16 [kp, ldc])."""
    C = np.asarray(C, dtype=np.float64)
    k, d = C.shape
    cb_bits = np.asarray(cb_bits)
    exp, lo, rc = split_oracle(C, kp, ds, cb_bits.shape[1])
    assert np.array_equal(cb_bits[:k, ds:2 * ds], exp[:k, ds:2 * ds]), "the second segment is not c_hi"
    assert np.array_equal(cb_bits, exp), "the bf16 layout [c_hi | c_hi | c_lo] differs"
    cn = np.asarray(cn, dtype=np.float32)
    assert np.all(cn[k:] == np.inf), "padding rows need an infinite norm"
    n2 = sumsq_rows(C)
    for j in range(k):  # within one f32 ulp of ||c||²: (float) of an f64 fold that is ~1e-14 off
        q = n2[j] if isinstance(n2[j], Fraction) else fr(n2[j])
        assert abs(fr(cn[j]) - q) <= q * F32_EPS, f"cn[{j}] = {cn[j]!r} is more than an f32 ulp off"
    # cst = sqrt(f64 fold) * (1 + 1e-9): the fold of d fmas and a 6-step wave sum is within (d + 6) 2^-53
    # of the exact sum (< 1e-13 for d <= 512), the square root halves it and adds 2^-53, the product one
    # more: the value lies in [true * (1 + 1e-9 - 1e-12), true * (1 + 1e-9 + 1e-12)] — above the truth
    # (soundness, no tolerance) and within the code's factor (tightness).
    cst = np.asarray(cst, dtype=np.float64)
    for i, q in enumerate((_max_fraction(sumsq_rows(lo)), _max_fraction(n2), _max_fraction(sumsq_rows(rc)))):
        v2 = fr(cst[i]) ** 2
        assert v2 >= q, f"cst[{i}] is below the true maximum"
        assert v2 <= q * (1 + Fraction(1, 10 ** 9) + Fraction(1, 10 ** 12)) ** 2, f"cst[{i}] is loose"
        if q == 0:
            assert cst[i] == 0.0
    if mc is not None:
        assert float(np.asarray(mc).reshape(-1)[0]) == float(cn[:k].max()), "mc is not the largest cn"


# ---------------------------------------------------------------------------------------------- cert_list

C101, C1E6 = Fraction(1.01), Fraction(1.0 + 1e-6)   # the kernel's double constants, as it holds them
# tightness of cert_list's bounds: W, plus the f64 rounding of e (8 operations, < 1e-15 relative) as it
# reaches the result: the cases keep |l² - e| >= 1e-3 l² (or e > l² by as much), so the cancellation
# amplifies it by at most 1e3 — 1e-12, with room to 1e-11
W_LIST = W + Fraction(1, 10 ** 11)


def list_oracle(case):
    """Per list entry: (uu, ll, bad) by the kernel's formula in plain f64 (unfused)."""
    lst = np.asarray(case["lst"], dtype=np.int64)[:case["cnt"]]
    ea, eb, en = (np.asarray(case[n], dtype=np.float32).astype(np.float64)[lst] for n in ("ea", "eb", "en"))
    c0, c1, c2 = (float(v) for v in case["cst"])
    e = 2.0 * (ea * c0 + eb * c1 + 1.01 * en * c2) * (1.0 + 1e-6)
    ub = np.asarray(case["u"], dtype=np.float32).astype(np.float64)[lst]
    lb = np.asarray(case["l"], dtype=np.float32).astype(np.float64)[lst]
    uu = f32_up(np.sqrt(ub * ub + e) * (1.0 + FOLD_MARGIN))
    ll = f32_dn(np.sqrt(np.maximum(lb * lb - e, 0.0)) * (1.0 - FOLD_MARGIN))
    return uu, ll, ~(uu < ll)


def list_slack(case, r):
    """(E_true, e_code) of row r as Fractions: the certificate's slack 2 (ea c0 + eb c1 + en c2) and
    the code's inflated form of it, 2 (ea c0 + eb c1 + 1.01 en c2) (1 + 1e-6)."""
    a, b, n = fr(case["ea"][r]), fr(case["eb"][r]), fr(case["en"][r])
    c0, c1, c2 = (fr(v) for v in case["cst"])
    return 2 * (a * c0 + b * c1 + n * c2), 2 * (a * c0 + b * c1 + C101 * n * c2) * C1E6


def check_list(case, lab, u, l, lc, nc, moves):
    """``case`` = dict(lst, cnt, blab, lab, u, l, ea, eb, en, cst, mv0 = the move log before the call
    (rows, old, new, count)); ``moves`` the log afterwards.  Returns (worst uu/true - 1, 1 - ll/true)
    against the code's own slack e."""
    cnt = case["cnt"]
    lst = np.asarray(case["lst"], dtype=np.int64)[:cnt]
    blab = np.asarray(case["blab"])[:cnt]
    lab0, u0, l0 = np.asarray(case["lab"]), np.asarray(case["u"], np.float32), np.asarray(case["l"], np.float32)
    lab, u, l = np.asarray(lab), np.asarray(u, np.float32), np.asarray(l, np.float32)
    _, _, bad = list_oracle(case)
    rest = np.ones(lab0.size, dtype=bool)
    rest[lst] = False
    assert np.array_equal(lab[rest], lab0[rest]) and np.array_equal(bits32(u[rest]), bits32(u0[rest])) \
        and np.array_equal(bits32(l[rest]), bits32(l0[rest])), "a row outside the list changed"
    check_row_list(lc, nc, lst[bad], "list C")
    rb, rg = lst[bad], lst[~bad]
    assert np.array_equal(lab[rb], blab[bad]), "an uncertified row did not get its old label back"
    assert np.array_equal(bits32(u[rb]), bits32(u0[rb])) and np.array_equal(bits32(l[rb]), bits32(l0[rb])), \
        "an uncertified row's bounds changed"
    assert np.array_equal(lab[rg], lab0[rg]), "a certified row lost its screened label"
    wu = wl = 0.0
    # plain f64 first: e, u² + e and l² - e carry at most 2e-12 of relative rounding there (the premise
    # |l² - e| >= 1e-3 l² again), so a row whose ratios stay 1e-11 inside both edges of its windows is
    # decided; every other row goes through Fractions
    ea, eb, en = (np.asarray(case[n], np.float32).astype(np.float64) for n in ("ea", "eb", "en"))
    c0, c1, c2 = (float(v) for v in case["cst"])
    e_r = 2.0 * (ea[rg] * c0 + eb[rg] * c1 + 1.01 * en[rg] * c2) * (1.0 + 1e-6)
    U2, L2 = u0[rg].astype(np.float64) ** 2, l0[rg].astype(np.float64) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        ru = u[rg].astype(np.float64) ** 2 / (U2 + e_r)
        rl = l[rg].astype(np.float64) ** 2 / (L2 - e_r)
    hi, lo = float((1 + W_LIST) ** 2), float((1 - W_LIST) ** 2)
    sure = (ru >= 1 + 1e-11) & (ru <= hi * (1 - 1e-11)) & (rl <= 1 - 1e-11) & (rl >= lo * (1 + 1e-11)) & (L2 > e_r)
    if sure.any():
        wu, wl = float(np.sqrt(ru[sure].max()) - 1.0), float(1.0 - np.sqrt(rl[sure].min()))
    for r in rg[~sure]:
        E, e = list_slack(case, r)
        U2, L2, uu2, ll2 = fr(u0[r]) ** 2, fr(l0[r]) ** 2, fr(u[r]) ** 2, fr(l[r]) ** 2
        # the code's e carries ~1e-15 of f64 rounding, far inside the 1e-10 margin applied after it: the
        # results are sound against the exact value of the code's own formula, a fortiori against E <= e
        assert e >= E and uu2 >= U2 + e, f"row {r}: the new u is below sqrt(u² + e)"
        assert uu2 <= (U2 + e) * (1 + W_LIST) ** 2, f"row {r}: the new u is loose"
        assert ll2 <= max(L2 - e, 0), f"row {r}: the new l is above sqrt(l² - e)"
        assert L2 - e > 0 and ll2 >= (L2 - e) * (1 - W_LIST) ** 2, f"row {r}: the new l is loose"
        wu = max(wu, math.sqrt(float(uu2 / (U2 + e))) - 1.0)
        wl = max(wl, 1.0 - math.sqrt(float(ll2 / (L2 - e))))
    r0, o0, n0, m0 = case["mv0"]
    mr, mo, mn, mc = moves
    m0, m1 = int(m0), int(np.asarray(mc).reshape(-1)[0])
    for a, b in ((mr, r0), (mo, o0), (mn, n0)):
        assert np.array_equal(np.asarray(a)[:m0], np.asarray(b)[:m0]), "earlier moves were overwritten"
    want = sorted((int(r), int(o), int(lab0[r])) for r, o, g in zip(lst, blab, ~bad) if g and lab0[r] != o)
    got = sorted(zip(np.asarray(mr)[m0:m1].tolist(), np.asarray(mo)[m0:m1].tolist(), np.asarray(mn)[m0:m1].tolist()))
    assert m1 - m0 == len(want), f"{m1 - m0} moves logged, {len(want)} expected"
    assert got == want, "the logged moves differ from the oracle's"
    return wu, wl


# ---------------------------------------------------------------------------------------------- cert_moves

def apply_moves(L0, rows, new):
    L1 = np.array(L0, dtype=np.int64)
    L1[np.asarray(rows, dtype=np.int64)] = np.asarray(new, dtype=np.int64)
    return L1


def dd_rel(adds):
    """Error of a double-double sum after ``adds`` additions, relative to the sum M of the sizes of
    the values: every dd_add splits exactly (TwoSum), so only the plain f64 additions into the low part
    round.  The low part is a sum of at most ``adds`` remainders of at most 2^-53 M each, so each of
    its additions rounds by at most 2^-53 * adds * 2^-53 M, and there are ``adds`` of them (the rows of
    the from-scratch sum, both ends of every move, the lanes, slices and normalisations)."""
    return Fraction(adds * adds, 2 ** 106)


def exact_cluster_sums(X, L, k):
    """Per cluster and column: the exact sum and the sum of the sizes, as Fractions."""
    X = np.asarray(X, dtype=np.float64)
    exact, mag = [], []
    for j in range(k):
        cols = [[Fraction(v) for v in col] for col in X[np.asarray(L) == j].T.tolist()]
        exact.append([sum(c, Fraction(0)) for c in cols])
        mag.append([sum((abs(v) for v in c), Fraction(0)) for c in cols])
    return exact, mag


def fsum_clusters(X, L, k):
    """S[j, t] = math.fsum of X[r, t] over the rows with L[r] = j (the correctly rounded exact sum), and
    the counts."""
    X = np.asarray(X, dtype=np.float64)
    d = X.shape[1]
    S = np.zeros((k, d))
    order = np.argsort(L, kind="stable")
    cnt = np.bincount(L, minlength=k)
    pos = np.concatenate([[0], np.cumsum(cnt)])
    for j in range(k):
        rows = X[order[pos[j]:pos[j + 1]]]
        for t in range(d):
            S[j, t] = math.fsum(rows[:, t].tolist())
    return S, cnt


def check_moves(case, S_hi, S_lo, cnt, seg, perm, C_next=None, shift2=None):
    """``case`` = dict(X, k, L0, rows, old, new, C_cur); the sums started from the from-scratch sums of
    L0.  Returns the worst relative error of shift2 (0 without it)."""
    X, k = np.asarray(case["X"], dtype=np.float64), case["k"]
    rows, old, new = (np.asarray(case[n], dtype=np.int64) for n in ("rows", "old", "new"))
    m = rows.size
    L1 = apply_moves(case["L0"], rows, new)
    S, c = fsum_clusters(X, L1, k)
    assert np.array_equal(np.asarray(cnt, dtype=np.int64), c), "cnt differs from bincount(L1)"
    assert np.array_equal(bits64(S_hi), bits64(S)), "S_hi differs from the correctly rounded sums of L1"
    hi, lo = np.asarray(S_hi, dtype=np.float64), np.asarray(S_lo, dtype=np.float64)
    assert np.array_equal(bits64(hi + lo), bits64(hi)), "S_hi / S_lo are not normalised (fl(hi + lo) != hi)"
    if is_dyadic(X) and not case.get("f32_rows"):
        # every partial sum is exact in f64 (is_dyadic), so no step of the double-double chain has a
        # remainder: the low parts are exactly 0
        assert not lo.any(), "S_lo is not 0 on exactly summable rows"
    else:
        exact, mag = exact_cluster_sums(X, L1, k)
        for j in range(k):
            for t in range(X.shape[1]):
                err = abs(fr(hi[j, t]) + fr(lo[j, t]) - exact[j][t])
                if case.get("f32_rows"):   # exponents span far less than 2^80: hi + lo is the exact sum
                    assert err == 0, f"S_hi + S_lo is not the exact sum at ({j}, {t})"
                else:                      # f64 rows: the double-double error, 2^-100 of the summed sizes
                    assert err <= mag[j][t] * dd_rel(X.shape[0] + 2 * m + 32), \
                        f"S_hi + S_lo is off the exact sum at ({j}, {t})"
    seg, perm = np.asarray(seg, dtype=np.int64), np.asarray(perm, dtype=np.int64)
    assert seg[0] == 0 and seg[2 * k] == 2 * m, f"seg[2k] = {seg[2 * k]}, 2m = {2 * m}"
    for b in range(2 * k):
        want = np.sort(rows[new == b]) if b < k else np.sort(rows[old == b - k])
        assert np.array_equal(np.sort(perm[seg[b]:seg[b + 1]]), want), f"perm: bin {b} holds the wrong rows"
    worst = 0.0
    if C_next is not None:
        Cc = np.asarray(case["C_cur"], dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where((c > 0)[:, None], S / np.maximum(c, 1)[:, None].astype(np.float64), Cc)
        assert np.array_equal(bits64(C_next), bits64(want)), "C_next differs from S_hi / cnt (empty: C_cur)"
        if shift2 is not None:
            # shift2[j] = f64 sum of (c - c_cur)² over d terms: every term is non-negative, so the
            # relative error is at most (roundings per term + depth of the sum) 2^-53 — 2 per term (the
            # difference, doubled by the square), 1 for the square, ceil(d / 256) + 8 additions: below
            # 20 * 2^-53 = 2.3e-15 for d <= 2048.  1e-12 leaves room and still fails any wrong term.
            e = want - Cc
            for j in range(k):
                ref = math.fsum((e[j] * e[j]).tolist())
                got = float(np.asarray(shift2)[j])
                if ref == 0.0:
                    assert got == 0.0
                else:
                    rel = abs(got - ref) / ref
                    assert rel <= 1e-12, f"shift2[{j}] = {got!r}, f64 value {ref!r}"
                    worst = max(worst, rel)
    return worst


# ---------------------------------------------------------------------------------------------- the chained step

def check_step_bounds(X, C, lab, u, l):
    """After a certified step: u >= the exact distance of every row to its own centre and l <= the exact
    distance to the nearest other centre, for every row.  The f64 squared distances, summed from the
    differences, are within (d + 2) 2^-53 < 1e-13 of the exact ones; a bound that clears the f64 value
    by 1e-12 is decided (the kernels' own margin is 1e-10, so fresh bounds clear it too), and every
    other row — ties, a row on its centre, anything close — goes through Fractions against its own
    centre and every other centre within 1e-9 of the nearest.  Returns the number of such rows."""
    X, C = np.asarray(X, dtype=np.float64), np.asarray(C, dtype=np.float64)
    lab = np.asarray(lab, dtype=np.int64)
    n, k = X.shape[0], C.shape[0]
    u, l = np.asarray(u, dtype=np.float32), np.asarray(l, dtype=np.float32)
    assert not np.any(np.isnan(u)) and not np.any(np.isnan(l)) and np.all(u >= 0) and np.all(l >= 0)
    D2 = np.stack([((X - c) ** 2).sum(axis=1) for c in C], axis=1)
    rows = np.arange(n)
    own = D2[rows, lab]
    u2, l2 = u.astype(np.float64) ** 2, l.astype(np.float64) ** 2
    exact_u = ~(u2 >= own * (1 + 1e-12)) | (own == 0)
    for r in rows[exact_u]:
        assert fr(u[r]) ** 2 >= sqdist_fraction(X[r], C[lab[r]]), \
            f"row {r}: u = {u[r]!r} is below the exact distance to its centre"
    if k == 1:
        assert np.all(l == np.inf)
        return int(exact_u.sum())
    D2[rows, lab] = np.inf
    other = D2.min(axis=1)
    exact_l = ~(l2 <= other * (1 - 1e-12))
    for r in rows[exact_l]:
        cand = np.nonzero(D2[r] <= other[r] * (1 + 1e-9))[0]
        q = min(sqdist_fraction(X[r], C[j]) for j in cand)
        assert np.isfinite(l[r]) and fr(l[r]) ** 2 <= q, \
            f"row {r}: l = {l[r]!r} is above the exact distance to the nearest other centre"
    return int(exact_u.sum() + exact_l.sum())


def hamerly_update(u, l, lab, drift, dtop):
    """The Hamerly bound update of cert_bounds on its own (no list)."""
    un, ln, _ = bounds_oracle(lab, u, l, drift, dtop, np.zeros(np.asarray(drift).shape, dtype=np.float32))
    return un, ln
