"""The oracles and checkers of ``exact_oracle`` / ``exact_cases`` on the CPU: the Fraction fold against
the host twin (``cml_exact_assign_host`` / ``cml_exact_sums_host``), the properties the cases promise
(exactness of the lattice rows, ties, gaps of the certificate rows), and for every checker a correct
output built by the oracle (passes) and mutants of it (each must fail) — the proof that
``test_kmeans_exact_kernels_gpu.py`` can fail."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import exact_cases as C
import exact_oracle as E
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import kmeans_ops as K

F32, F64 = np.float32, np.float64


def ulp(a, target):
    return np.nextafter(np.asarray(a, dtype=F32), F32(target)).astype(F32)


def fails(fn, *args, match=None, **kw):
    with pytest.raises(AssertionError, match=match):
        fn(*args, **kw)


def fold_desc(x, c):
    return E.fma_fold(np.asarray(x)[::-1], np.asarray(c)[::-1])


def fold_halves(x, c):
    h = len(x) // 2
    return E.fma_fold(x[:h], c[:h]) + E.fma_fold(x[h:], c[h:])


# ---------------------------------------------------------------------------------------------- the fold and the host twin

def test_fma_fold_is_one_fma_per_term():
    """On values where the product is inexact the fma and the two-step form differ; the fold keeps the
    fma's.  A changed order changes the bits of most random rows."""
    a, b = 1.0 + 2.0 ** -30, 0.0
    assert E.fma_fold([a, 3.0], [b, 1.0]) == float(Fraction(a) ** 2 + 4)
    assert E.fma_fold([1.5, 2.0], [0.25, 1.0]) == 2.5625
    rng = np.random.default_rng(5)
    X, c = rng.standard_normal((60, 37)) * 50, rng.standard_normal(37) * 50
    ref = np.array([E.fma_fold(x, c) for x in X])
    assert np.mean(ref != ((X - c) ** 2).sum(axis=1)) > 0.3           # plain numpy is another fold
    assert np.mean(ref != np.array([fold_desc(x, c) for x in X])) > 0.3
    assert np.mean(ref != np.array([fold_halves(x, c) for x in X])) > 0.3
    assert np.allclose(ref, ((X - c) ** 2).sum(axis=1), rtol=1e-14)
    assert E.argmin_top2([3.0, 1.0, 1.0, 2.0]) == (1, 1.0, 1.0)
    assert E.argmin_top2([4.0]) == (0, 4.0, math.inf)


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("n,d,k", [(60, 37, 20), (40, 4, 9), (6, 300, 5)])
def test_host_twin_equals_the_fraction_fold(n, d, k, f64):
    """K.assign_reference on CPU tensors: labels and distances bit for bit, for f64 rows and for f32 rows
    widened to f64 — after this the GPU module may take the host twin for the rows Fractions cannot reach."""
    rng = np.random.default_rng(n * d + k)
    X, Cn = rng.standard_normal((n, d)) * 50, rng.standard_normal((k, d)) * 50
    if not f64:
        X = X.astype(F32).astype(F64)
    assert not E.is_dyadic(X)
    lab, best = C.host_twin_assign(X, Cn)
    want_lab, want_best, _ = E.assign_fold(X, Cn)
    assert np.array_equal(lab, want_lab)
    assert np.array_equal(E.bits64(best), E.bits64(want_best))
    E.check_assign(want_lab, want_best, lab, best)


def test_host_twin_breaks_ties_to_the_lowest_index():
    for form in ("kg16_d17_k9", "dreg16_d16_k513"):
        c = C.assign_lattice_case(form, 257, True)
        lab, best = C.host_twin_assign(c["X"], c["C"])
        E.check_assign(c["lab"], c["bd"], lab, best)


def test_host_twin_sums_are_the_exact_cluster_sums():
    for c in (C.sums_case("forty_in_one_chunk", 1), C.sums_case("empties", 65), C.sums_case("single_row"),
              C.sums_cancel_case()):
        S, cnt, S_lo = C.host_twin_sums(c["X"], c["L"], c["k"])
        exact, _ = E.exact_cluster_sums(c["X"], c["L"], c["k"])
        for j in range(c["k"]):
            for t in range(c["X"].shape[1]):
                assert Fraction(float(S[j, t])) == exact[j][t] and S_lo[j, t] == 0    # representable sums
        E.check_sums(c["X"], c["L"], c["k"], S, S_lo, cnt, exact_rows=True)
    g = C.sums_generic_case()
    S, cnt, S_lo = C.host_twin_sums(g["X"], g["L"], g["k"])
    assert np.any(S_lo != 0)
    E.check_sums(g["X"], g["L"], g["k"], S, S_lo, cnt, exact_rows=False)
    for n in C.SUM_N[:2]:
        E.check_sum_exact(C.sum_case(n), K.sum_exact(torch.as_tensor(C.sum_case(n))).item())


# ---------------------------------------------------------------------------------------------- what the cases promise

@pytest.mark.parametrize("form", list(C.ASSIGN_FORMS))
def test_assign_lattice_cases_hold_their_edges(form):
    d, k = C.ASSIGN_FORMS[form]
    for n in C.ASSIGN_N:
        for dup in (False, True):
            c = C.assign_lattice_case(form, n, dup)
            X, Cn = c["X"], c["C"]
            assert E.is_lattice(X, Cn) and (d > 1024 or E.is_dyadic(X, Cn))
            assert np.array_equal(X.astype(F32).astype(F64), X)             # the same rows as f32
            assert c["bd"][0] == 0 and np.array_equal(X[0], Cn[k - 1])      # row 0 sits on the last centre
            if k == 1:
                assert np.all(np.isinf(c["sd"]))
                continue
            assert c["lab"][0] == (0 if dup else k - 1)                     # ... which loses to centre 0 if it repeats it
            if dup:
                assert np.all(c["lab"] != k - 1) and np.array_equal(Cn[0], Cn[k - 1])
            if n > 1:
                assert np.sum(c["bd"] == c["sd"]) >= n // 16                 # rows on bisectors / duplicates
                assert len(set(c["lab"].tolist())) >= min(k - dup * (1 if k < 4 else 2), 3)
    for r in (0, 1, 100):                                                    # plain numpy is the Fractions' value
        assert Fraction(float(c["bd"][r])) == min(E.sqdist_fraction(X[r], cj) for cj in Cn)


def test_assign_generic_cases_have_no_ties():
    for form, f64 in (("dreg16_d5", True), ("kg4_d17_k3", False), ("kg16_d17_k9", True)):
        c = C.assign_generic_case(form, f64)
        assert not E.is_dyadic(c["X"]) and np.all(c["sd"] > c["bd"] * (1 + 1e-9))
        assert {0, c["n"] - 1, 255, 256} <= set(c["sub"].tolist())
        if not f64:
            assert np.array_equal(c["X"].astype(F32).astype(F64), c["X"])
    b = C.BIG_IDX
    assert b["n"] > 4096 * 256 and b["n"] * b["d"] * 4 < 72e6


@pytest.mark.parametrize("name", list(C.CERT_CASES))
def test_screen_cert_cases_have_the_gap(name):
    """Every row is on the line lb - ub = 2 (err + ecmax), at least GAP (relative) above it — the kernel's
    factor is 1 + 1e-9 —, or below it; the data is dyadic, so the decision is exact in f64."""
    c = C.cert_case(name)
    assert E.cert_case_is_exact(c["ub"], c["lb"], c["err"], c["ecmax"])
    listed, on_line, margin = E.cert_decision(c["ub"], c["lb"], c["err"], c["ecmax"])
    assert np.array_equal(on_line, c["kind"] == 0) and np.array_equal(listed, c["kind"] != 1)
    assert np.all(margin[~listed] >= E.GAP) and E.GAP > 100 * 1e-9
    pattern = C.CERT_CASES[name][1]
    if pattern == "mixed" and c["n"] > 100:
        assert all(np.any(c["kind"] == v) for v in (0, 1, 2)) and np.any(c["err"] == 0)
    if pattern == "wave":
        assert listed.sum() == -(-c["n"] // 64)
    assert (pattern != "all" or listed.all()) and (pattern != "none" or not listed.any())


@pytest.mark.parametrize("name", list(C.SPLIT_CERT_CASES))
def test_screen_cert_split_cases_hold_the_premise(name):
    c = C.split_cert_case(name)
    ub, lb, ea, eb, en = (c[m].astype(F64) for m in ("ub", "lb", "ea", "eb", "en"))
    e = 2.0 * (ea * C.CST[0] + eb * C.CST[1] + 1.01 * en * C.CST[2]) * (1.0 + 1e-6)
    assert np.all(np.abs(lb * lb - e) >= 1.001e-3 * lb * lb)                  # the premise of W_LIST
    for r in range(0, c["n"], max(1, c["n"] // 20)):
        assert abs(float(E.list_slack(c, r)[1]) - e[r]) <= 1e-14 * e[r]
    pattern = C.SPLIT_CERT_CASES[name][1]
    if pattern == "all":
        assert np.all(lb * lb < e)
    if pattern == "mixed" and c["n"] > 100:
        assert np.any(lb * lb < e) and np.any(e == 0) and np.any((e > 0) & (e < lb * lb))
    if name == "flush":   # block 0 visits 8 tiles of 256 rows, all listed: more than kBuf - 256 after the 8th
        assert -(-c["n"] // (2048 * 256)) * 256 > 2048 - 256


def test_sums_cases_hold_their_edges():
    for name, sizes in C.SUMS_LAYOUTS.items():
        assert sum(sizes) == 3073
        c = C.sums_case(name, 1)
        assert E.is_dyadic(c["X"]) and np.array_equal(np.bincount(c["L"], minlength=c["k"]), sizes)
        assert np.array_equal(c["X"].astype(F32).astype(F64), c["X"])
    ends = np.cumsum(C.SUMS_LAYOUTS["ends_on_edges"])
    assert 1024 in ends and 2048 in ends
    s = np.cumsum(C.SUMS_LAYOUTS["spans_three_chunks"])
    assert s[0] < 1024 and s[1] > 2048
    f = np.cumsum(C.SUMS_LAYOUTS["forty_in_one_chunk"])
    assert f[0] > 0 and f[40] < 1024
    z = C.sums_cancel_case()
    assert np.array_equal(z["X"].astype(F32).astype(F64), z["X"]) and not np.any(z["X"][z["L"] == 1].sum(axis=0))
    assert C.SUM_N[2] > 1024 * 4096 and C.SUM_N[1] > 4096


# ---------------------------------------------------------------------------------------------- mutants: assign

def test_check_assign_passes_the_oracle_and_fails_its_mutants():
    c = C.assign_generic_case("kg4_d17_k3", True)
    X, Cn, sub = c["X"], c["C"], c["sub"]
    n, k = c["n"], c["k"]
    lab, best = C.host_twin_assign(X, Cn)
    E.check_assign(c["lab"], c["bd"], lab, best, where=sub)
    for mutant, why in ((fold_desc, "a fold in descending t"), (fold_halves, "a fold in two halves")):
        m = best.copy()
        m[sub] = [mutant(X[r], Cn[lab[r]]) for r in sub]
        assert np.any(m != best), why
        fails(E.check_assign, c["lab"], c["bd"], lab, m, where=sub, match="t-ascending")
    # a tie broken to the higher index
    t = C.assign_lattice_case("kg16_d17_k9", 257, True)
    E.check_assign(t["lab"], t["bd"], t["lab"], t["bd"])
    high = t["lab"].copy()
    on_dup = np.all(t["X"] == t["C"][t["k"] - 1], axis=1)
    assert on_dup.any()
    high[on_dup] = t["k"] - 1
    fails(E.check_assign, t["lab"], t["bd"], high, t["bd"], match="argmin")
    # idx mode: unlisted rows keep their sentinel, changed counts the differing labels
    rows = np.arange(0, n, 2)
    lab0 = C.other_labels(lab, k)
    out, b0 = lab0.copy(), np.full(n, -1.0)
    out[rows] = lab[rows]
    bo = b0.copy()
    bo[rows] = best[rows]
    ch = int((out[rows] != lab0[rows]).sum())
    assert ch > 0
    E.check_assign(lab, best, out, bo, rows=rows, lab0=lab0, best0=b0, changed=ch)
    fails(E.check_assign, lab, best, out, bo, rows=rows, lab0=lab0, best0=b0, changed=ch + 1, match="changed")
    touched = out.copy()
    touched[1] = (touched[1] + 1) % k
    fails(E.check_assign, lab, best, touched, bo, rows=rows, lab0=lab0, best0=b0, match="unlisted")
    tb = bo.copy()
    tb[1] = 0.0
    fails(E.check_assign, lab, best, out, tb, rows=rows, lab0=lab0, best0=b0, match="unlisted")


def test_check_top2_bounds_passes_the_tightest_bounds_and_fails_their_mutants():
    c = C.assign_generic_case("kg4_d17_k3", True)
    sub = c["sub"]
    D1, D2 = E.exact_top2_fraction(c["X"], c["C"], sub)
    n = c["n"]
    ub, lb = np.zeros(n, F32), np.zeros(n, F32)
    ub[sub] = [E.tight_up(q) for q in D1]
    lb[sub] = [E.tight_dn(q) for q in D2]
    E.check_top2_bounds(ub, lb, D1, D2, sub)
    # the kernel's formula passes too
    ku, kl = ub.copy(), lb.copy()
    ku[sub] = E.f32_up(np.sqrt(c["bd"]) * (1 + E.FOLD_MARGIN))
    kl[sub] = E.f32_dn(np.sqrt(c["sd"]) * (1 - E.FOLD_MARGIN))
    wu, wl = E.check_top2_bounds(ku, kl, D1, D2, sub)
    assert 0 < wu < float(E.W) and 0 < wl < float(E.W)
    for i in (0, len(sub) - 1):
        m = ub.copy()
        m[sub[i]] = ulp(m[sub[i]], 0)
        fails(E.check_top2_bounds, m, lb, D1, D2, sub, match="unsound upper")     # ub one f32 ulp low
        m = lb.copy()
        m[sub[i]] = ulp(m[sub[i]], np.inf)
        fails(E.check_top2_bounds, ub, m, D1, D2, sub, match="unsound lower")     # lb one ulp high
        m = ub.copy()
        m[sub[i]] = ulp(ulp(m[sub[i]], np.inf), np.inf)
        fails(E.check_top2_bounds, m, lb, D1, D2, sub, match="loose upper")
    # lattice: a row on its centre gives exactly 0; k = 1 gives lb = +inf
    t = C.assign_lattice_case("kg4_d17_k3", 255, False)
    rows = np.arange(255)
    tu = E.f32_up(np.sqrt(t["bd"]) * (1 + E.FOLD_MARGIN))
    tl = E.f32_dn(np.sqrt(t["sd"]) * (1 - E.FOLD_MARGIN))
    E.check_top2_bounds(tu, tl, t["bd"], t["sd"], rows)
    m = tu.copy()
    m[0] = F32(1e-30)
    fails(E.check_top2_bounds, m, tl, t["bd"], t["sd"], rows, match="exactly 0")
    one = C.assign_lattice_case("kg4_d24_k1", 255, False)
    ou = E.f32_up(np.sqrt(one["bd"]) * (1 + E.FOLD_MARGIN))
    E.check_top2_bounds(ou, np.full(255, np.inf, F32), one["bd"], one["sd"], rows)
    fails(E.check_top2_bounds, ou, np.full(255, 3e38, F32), one["bd"], one["sd"], rows, match=r"\+inf")


def test_check_moves_and_check_list_fail_their_mutants():
    rng = np.random.default_rng(9)
    n = 300
    old, new = rng.integers(0, 5, n), rng.integers(0, 5, n)
    lst = rng.permutation(n)[:200]
    moved = [r for r in lst if old[r] != new[r]]
    m = len(moved)

    def log(rows, count):
        mv = [np.full(n, -1, np.int32) for _ in range(3)]
        mv[0][:len(rows)], mv[1][:len(rows)], mv[2][:len(rows)] = rows, old[rows], new[rows]
        return (*mv, np.array([count], np.int32))

    E.check_moves(log(moved, m), lst, old, new)
    fails(E.check_moves, log(moved, m - 1), lst, old, new, match="expected")                 # a wrong count
    fails(E.check_moves, log(moved + moved[:1], m), lst, old, new, match="past its count")   # a write past the count
    fails(E.check_moves, log(moved[:-1] + moved[:1], m), lst, old, new, match="differ")      # a duplicate for a missing row
    unl = [r for r in range(n) if r not in set(lst.tolist()) and old[r] != new[r]][:1]
    fails(E.check_moves, log(moved + unl, m + 1), lst, old, new, match="expected")           # a move of an unlisted row
    wrong = log(moved, m)
    wrong[2][0] = (wrong[2][0] + 1) % 5
    fails(E.check_moves, wrong, lst, old, new, match="differ")

    exp = np.sort(lst[:50])
    buf = np.full(n, -1, np.int32)
    buf[:50] = exp[::-1]
    E.check_list(buf, 50, exp)
    fails(E.check_list, buf, 49, exp, match="expected")                                      # a wrong count
    d = buf.copy()
    d[1] = d[0]
    fails(E.check_list, d, 50, exp, match="differ")                                          # a duplicate (and a missing row)
    p = buf.copy()
    p[50] = 7
    fails(E.check_list, p, 50, exp, match="past its count")                                  # a write past the count
    E.check_list(np.full(n, -1, np.int32), 0, [])


# ---------------------------------------------------------------------------------------------- mutants: bf16 copies

def _tight_err(X, d, ldo):
    out, e = E.err_oracle(X, d, ldo)
    err = np.array([max(E.tight_up(sum((Fraction(float(v)) ** 2 for v in row), Fraction(0))), F32(1e-30)) for row in e], F32)
    return out, err


def test_check_bf16_err_passes_the_oracle_and_fails_its_mutants():
    for f64 in (True, False):
        X = C.rows_case(5, 63, f64)
        out, err = _tight_err(X, 63, 64)
        assert np.array_equal(out[:, :63], C.torch_bf16_bits(X, f64))                       # torch's own rounding
        E.check_bf16_err(X, 63, 64, out, err)
        k = E.f32_up(np.sqrt(((X - E.bf16_value(out[:, :63]).astype(F64)) ** 2).sum(axis=1)) * (1 + 1e-6)) + F32(1e-30)
        w = E.check_bf16_err(X, 63, 64, out, k.astype(F32))                                 # the kernel's formula
        assert 1e-6 - 1e-9 < w < float(E.W_ERR)
        m = out.copy()
        m[3, 63] = 1
        fails(E.check_bf16_err, X, 63, 64, m, err, match="padding")                         # a nonzero padding element
        m = err.copy()
        m[0] = ulp(m[0], 0)
        fails(E.check_bf16_err, X, 63, 64, out, m, match="below the exact")
        m = err.copy()
        m[0] = F32(m[0] * (1 + 2e-6))
        fails(E.check_bf16_err, X, 63, 64, out, m, match="loose")
        trunc = (E.bits32(X[:, :63].astype(F32)) >> 16).astype(np.uint16)                   # truncation, not nearest even
        m = out.copy()
        m[:, :63] = trunc
        assert np.any(m != out)
        fails(E.check_bf16_err, X, 63, 64, m, err, match="nearest even")
    fails(E.check_bf16_err, X, 63, 64, out, np.zeros(5, F32))                               # a zero row still has err > 0


def _direct_bf16(v):
    """f64 -> bf16 in one rounding (nearest even): the mutant's ``lo``."""
    out = np.empty(v.shape, np.uint16)
    for i, x in np.ndenumerate(v):
        lo = np.uint16(E.bits32(F32(x))[0] >> 16) if x == 0 else None
        if lo is None:
            b = int(E.bits32(np.array(abs(x), F32).reshape(1))[0]) >> 16
            cand = [b - 1, b, b + 1]
            val = [Fraction(float(E.bf16_value(np.array([c], np.uint16))[0])) for c in cand]
            dist = [abs(q - Fraction(abs(float(x)))) for q in val]
            best = min(range(3), key=lambda j: (dist[j], cand[j] & 1))
            lo = np.uint16(cand[best] | (0x8000 if x < 0 else 0))
        out[i] = lo
    return out


def _tight_split(X, d, ds, ldo):
    out, lo, rx = E.split_rows_oracle(X, d, ds, ldo)
    sq = lambda A: [sum((Fraction(float(v)) ** 2 for v in row), Fraction(0)) for row in A]   # noqa: E731
    tiny = np.nextafter(F32(0), F32(1))
    ea = np.array([E.tight_up(q) for q in sq(lo)], F32)
    eb = np.array([max(E.tight_up(q), tiny) for q in sq(rx)], F32)
    en = np.array([E.tight_up(q) for q in sq(X[:, :d])], F32)
    xn = np.array([float(q) for q in sq(X[:, :d])]).astype(F32)
    return out, ea, eb, en, xn


def test_f64_rows_tell_the_rounding_through_f32_from_one_rounding():
    """Row 4 of the f64 rows: hi (first value) and lo (second value) differ between f64 -> f32 -> bf16, which
    torch and the oracle apply, and a single rounding from f64."""
    for d in (1, 63, 130):
        X = C.rows_case(5, d, True)
        hi = E.bf16_bits(X[4].astype(F32))
        assert _direct_bf16(X[4, :1])[0] != hi[0] and np.array_equal(hi, C.torch_bf16_bits(X[4:5], True)[0])
        if d > 1:
            r1 = X[4, 1:2] - E.bf16_value(hi[1:2]).astype(F64)
            assert _direct_bf16(r1)[0] != E.bf16_bits(r1.astype(F32))[0]


def test_check_split_rows_passes_the_oracle_and_fails_its_mutants():
    d, ds, ldo = 130, 136, 512
    X = C.rows_case(17, d, True).copy()
    # lo through f32: x - hi = 2^-10 (1 + 2^-8 + 2^-40) rounds to the bf16 midpoint in f32 first, then to even
    # (down); one rounding from f64 goes up
    X[5, 0] = 1.0 + 2.0 ** -10 + 2.0 ** -18 + 2.0 ** -50
    out, ea, eb, en, xn = _tight_split(X, d, ds, ldo)
    assert np.array_equal(out, C.torch_split_layout(X, True, d, ds, ldo))                   # torch's own rounding
    E.check_split_rows(X, d, ds, ldo, out, ea, eb, en, xn)
    assert ea[1] == 0 and ea[2] == 0 and en[2] == 0 and xn[2] == 0 and eb[3] == np.nextafter(F32(0), F32(1))
    hi = E.bf16_value(out[:, :d]).astype(F64)
    m = out.copy()
    m[:, ds:ds + d] = _direct_bf16(X - hi)
    assert m[5, ds] != out[5, ds]
    fails(E.check_split_rows, X, d, ds, ldo, m, ea, eb, en, xn, match="through f32")        # lo rounded from f64
    for col in (d, ds + d, 2 * ds + d, 3 * ds, ldo - 1):
        m = out.copy()
        m[4, col] = 0x3F80
        fails(E.check_split_rows, X, d, ds, ldo, m, ea, eb, en, xn, match="padding")        # a nonzero padding element
    for i, (name, arr) in enumerate((("ea", ea), ("eb", eb), ("en", en))):
        lowm, loose = [a.copy() for a in (ea, eb, en)], [a.copy() for a in (ea, eb, en)]
        lowm[i][0] = ulp(arr[0], 0)
        fails(E.check_split_rows, X, d, ds, ldo, out, *lowm, xn, match=f"{name}² is below")
        loose[i][0] = F32(arr[0] * (1 + 2e-6))
        fails(E.check_split_rows, X, d, ds, ldo, out, *loose, xn, match="loose")
    m = xn.copy()
    m[0] = ulp(ulp(m[0], np.inf), np.inf)
    fails(E.check_split_rows, X, d, ds, ldo, out, ea, eb, en, m, match="xn")
    m = eb.copy()
    m[3] = 0
    fails(E.check_split_rows, X, d, ds, ldo, out, ea, m, en, xn, match="eb")
    # the kernel's formulas stay inside the windows
    lo, rx = E.split_rows_oracle(X, d, ds, ldo)[1:]
    kf = lambda A, t=0.0: E.f32_up(np.sqrt((A * A).sum(axis=1)) * (1 + 1e-6) + t)           # noqa: E731
    wa, wb, wn, wx = E.check_split_rows(X, d, ds, ldo, out, kf(lo), kf(rx, 1e-300), kf(X), (X * X).sum(axis=1).astype(F32))
    assert max(wa, wb, wn) < float(E.W_SPLIT) and wx <= float(E.W_XN)


# ---------------------------------------------------------------------------------------------- mutants: the certificates

def _cert_outputs(c):
    listed, _, _ = E.cert_decision(c["ub"], c["lb"], c["err"], c["ecmax"])
    e = c["err"].astype(F64) + c["ecmax"]
    u = E.f32_up((c["ub"].astype(F64) + e) * (1 + E.FOLD_MARGIN))
    l = E.f32_dn((c["lb"].astype(F64) - e) * (1 - E.FOLD_MARGIN))
    rows = np.nonzero(listed)[0]
    lst = np.full(c["n"], -1, np.int32)
    lst[:rows.size] = rows[::-1]
    return lst, rows.size, u, l


def test_check_screen_cert_passes_the_oracle_and_fails_its_mutants():
    c = C.cert_case("n1025")
    lst, cnt, u, l = _cert_outputs(c)
    wu, wl = E.check_screen_cert(c, lst, cnt, u, l)
    assert 0 < wu < float(E.W) and 0 < wl < float(E.W)
    E.check_screen_cert(c, lst, cnt)
    on_line = np.nonzero(c["kind"] == 0)[0]
    m = np.full(c["n"], -1, np.int32)
    keep = lst[:cnt][lst[:cnt] != on_line[0]]
    m[:keep.size] = keep
    fails(E.check_screen_cert, c, m, cnt - 1, u, l, match="expected")                        # >= instead of a strict >
    above = np.nonzero(c["kind"] == 1)[0]
    m = lst.copy()
    m[cnt] = above[0]
    fails(E.check_screen_cert, c, m, cnt + 1, u, l, match="expected")                        # a certified row listed
    fails(E.check_screen_cert, c, m, cnt, u, l, match="past its count")
    m = lst.copy()
    m[0] = m[1]
    fails(E.check_screen_cert, c, m, cnt, u, l, match="differ")
    tu = E.f32_up(c["ub"].astype(F64) + c["err"].astype(F64) + c["ecmax"])                   # the tightest bounds pass
    tl = E.f32_dn(c["lb"].astype(F64) - c["err"].astype(F64) - c["ecmax"])
    E.check_screen_cert(c, lst, cnt, tu, tl)
    m = tu.copy()
    m[3] = ulp(m[3], 0)
    fails(E.check_screen_cert, c, lst, cnt, m, tl, match="unsound upper")
    m = tl.copy()
    m[3] = ulp(m[3], np.inf)
    fails(E.check_screen_cert, c, lst, cnt, tu, m, match="unsound lower")
    m = tu.copy()
    m[3] = ulp(ulp(m[3], np.inf), np.inf)
    fails(E.check_screen_cert, c, lst, cnt, m, tl, match="loose upper")


def _split_outputs(c):
    ub, lb, ea, eb, en = (c[m].astype(F64) for m in ("ub", "lb", "ea", "eb", "en"))
    e = 2.0 * (ea * C.CST[0] + eb * C.CST[1] + 1.01 * en * C.CST[2]) * (1.0 + 1e-6)
    u = E.f32_up(np.sqrt(ub * ub + e) * (1 + E.FOLD_MARGIN))
    l = E.f32_dn(np.sqrt(np.maximum(lb * lb - e, 0.0)) * (1 - E.FOLD_MARGIN))
    rows = np.nonzero(~(u < l))[0]
    lst = np.full(c["n"], -1, np.int32)
    lst[:rows.size] = rows
    return lst, rows.size, u, l, e


def test_check_screen_cert_split_passes_the_oracle_and_fails_its_mutants():
    c = C.split_cert_case("n257")
    lst, cnt, u, l, e = _split_outputs(c)
    wu, wl = E.check_screen_cert_split(c, lst, cnt, u, l)
    assert 0 < wu < float(E.W_LIST) and 0 < wl < float(E.W_LIST)
    lb2 = c["lb"].astype(F64) ** 2
    below = np.nonzero(lb2 < e)[0]
    good = np.nonzero((e > 0) & (e < lb2 * 0.9))[0]
    assert below.size and good.size and np.all(l[below] == 0)
    m = np.full(c["n"], -1, np.int32)
    keep = lst[:cnt][lst[:cnt] != below[0]]
    m[:keep.size] = keep
    fails(E.check_screen_cert_split, c, m, cnt - 1, u, l, match="expected")                  # a row with lb² < E not listed
    r = good[0]
    m = u.copy()
    m[r] = E.f32_dn(np.float64(c["ub"][r]))                                                  # u_out without the slack E
    fails(E.check_screen_cert_split, c, *_relist(c, m, l), m, l, match="below sqrt")
    m = l.copy()
    m[r] = c["lb"][r]                                                                        # l_out without the slack
    fails(E.check_screen_cert_split, c, *_relist(c, u, m), u, m, match="above sqrt")
    m = u.copy()
    m[r] = F32(m[r] * (1 + 1e-6))
    fails(E.check_screen_cert_split, c, *_relist(c, m, l), m, l, match="loose")
    m = l.copy()
    m[r] = F32(m[r] * (1 - 1e-6))
    fails(E.check_screen_cert_split, c, *_relist(c, u, m), u, m, match="loose")
    m = l.copy()
    m[below[0]] = F32(1e-3)
    fails(E.check_screen_cert_split, c, *_relist(c, u, m), u, m, match="above sqrt")


def _relist(c, u, l):
    rows = np.nonzero(~(u < l))[0]
    lst = np.full(c["n"], -1, np.int32)
    lst[:rows.size] = rows
    return lst, rows.size


# ---------------------------------------------------------------------------------------------- mutants: sums

def test_check_sums_and_check_sum_exact_fail_their_mutants():
    z = C.sums_cancel_case()
    S, cnt, S_lo = C.host_twin_sums(z["X"], z["L"], z["k"])
    E.check_sums(z["X"], z["L"], z["k"], S, S_lo, cnt, exact_rows=True)
    plain = np.zeros_like(S)
    for x, j in zip(z["X"], z["L"]):
        plain[j] += x                                                                        # plain f64, in row order
    assert np.any(plain != S) and not np.any(S[1])
    fails(E.check_sums, z["X"], z["L"], z["k"], plain, S_lo, cnt, exact_rows=True)           # not correctly rounded
    m = cnt.copy()
    m[0] += 1
    fails(E.check_sums, z["X"], z["L"], z["k"], S, S_lo, m, exact_rows=True, match="counts")
    g = C.sums_generic_case()
    S, cnt, S_lo = C.host_twin_sums(g["X"], g["L"], g["k"])
    E.check_sums(g["X"], g["L"], g["k"], S, S_lo, cnt, exact_rows=False)
    fails(E.check_sums, g["X"], g["L"], g["k"], S, np.zeros_like(S_lo), cnt, exact_rows=False, match="off the exact")
    fails(E.check_sums, g["X"], g["L"], g["k"], S, S_lo * 1.5 + 1e-9, cnt, exact_rows=False)
    c = C.sums_case("ends_on_edges", 65)
    S, cnt, S_lo = C.host_twin_sums(c["X"], c["L"], c["k"])
    E.check_sums(c["X"], c["L"], c["k"], S, S_lo, cnt, exact_rows=True, cols=(0, 64))
    m = S.copy()
    m[1, 64] += c["X"][0, 64] if c["X"][0, 64] else 1.0                                     # one row in the wrong cluster
    fails(E.check_sums, c["X"], c["L"], c["k"], m, S_lo, cnt, exact_rows=True)
    v = C.sum_case(4097)
    E.check_sum_exact(v, math.fsum(v.tolist()))
    seq = 0.0
    for x in np.sort(v).tolist():
        seq += x
    assert seq != math.fsum(v.tolist())
    fails(E.check_sum_exact, v, seq)
