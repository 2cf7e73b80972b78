"""The eleven kernels of the source-precision KMeans path (``_native/csrc/kmeans_exact.hip``), kernel by
kernel through the wrappers of ``ops/kmeans_ops.py``, against the exact oracles of ``exact_oracle`` —
the cases of ``exact_cases``, whose promises and whose checkers ``test_exact_oracle.py`` has tested on
the CPU first.  The other GPU modules take ``K.exact_assign`` as their reference; here it is the
subject: the two narrow forms and the six wide forms of ``launch_wide_any`` each meet lattice rows
(exact in plain numpy: rows on their centre, on bisectors, on duplicate centres, winners in every LDS
tile and accumulator group) and generic rows whose labels and distances must equal the Fraction fold
(a subset of rows) and the host twin (all rows) bit for bit — so wide, narrow and host are the same
bits by way of the oracle, not by way of each other.

Figures.  Every test prints what it measured and the worst value so far (``-s`` shows them); the
windows are asserted inside the checkers.  A run of this whole module on an MI355X printed the worst
values below, each beside the window it had to stay within (derived in ``exact_oracle`` /
``cert_oracle`` from the code's constants, not from a run):

  exact_top2         ub/true - 1          1.192e-07   measured on an MI355X   (window 1.195e-07 = 2^-23 + 3e-10)
  exact_top2         1 - lb/true          1.192e-07   measured on an MI355X   (window 1.195e-07)
  screen_cert        u_out/true - 1       1.192e-07   measured on an MI355X   (window 1.195e-07)
  screen_cert        1 - l_out/true       1.192e-07   measured on an MI355X   (window 1.195e-07)
  screen_cert_split  u_out/true - 1       1.192e-07   measured on an MI355X   (window 1.195e-07, + 1e-11 for e)
  screen_cert_split  1 - l_out/true       1.192e-07   measured on an MI355X   (window 1.195e-07, + 1e-11 for e)
  to_bf16_err        err/true - 1         1.059e-06   measured on an MI355X   (window 1.119e-06 = (1 + 1e-6)(1 + 2^-23) - 1,
                                                                               and 1e-30 (1 + 2^-23) absolute)
  to_bf16_split      ea/true - 1          1.108e-06   measured on an MI355X   (window 1.119e-06 = 1e-6 + 2^-23 + 1e-12)
  to_bf16_split      eb/true - 1          1.111e-06   measured on an MI355X   (window 1.119e-06, and 1e-300 absolute)
  to_bf16_split      en/true - 1          1.106e-06   measured on an MI355X   (window 1.119e-06)
  to_bf16_split      |xn/true - 1|        5.198e-08   measured on an MI355X   (window 5.961e-08 = 2^-24 + 1e-12)
  exact_sums         |S + S_lo - exact|   0           measured on an MI355X   (bound 1.2e-25 of the summed sizes,
                                                                               dd_rel(n + 32); generic f64 rows)

The fold (labels, best, exact_dist), every list, count and move, the bf16 layouts and the sums of
exactly summable rows are compared bit for bit and have no figure.  The worst bound slack is one f32
ulp just above a power of two (2^-23).

A finding of these tests: for f64 rows the two bf16 kernels rounded x (and x - hi) to bf16 in one step from
f64, not through f32 as their comments and the host forms say — the compiler folds (__bf16)(float)v — which
gives the other neighbour where the f32 value falls on a bf16 tie (about 2^-17 of random values: the 131 075
x 8 case met it first; row 4 of the f64 rows now holds such values on purpose).  ``f64_to_bf16_via_f32``
(exact_util.h) keeps the f32 step.

One shape differs from the issue that asked for these tests: screen_cert_split's LDS buffer (2048
entries) flushes in mid-loop only once a block has gathered more than 2048 - 256 entries, which takes
eight all-listed tiles per block, n > 7 * 2048 * 256 (the "flush" case); n = 4100, all listed, is run
too.
"""
import numpy as np
import pytest
import torch

import exact_cases as C
import exact_oracle as E
from clustermachinelearningforhospitalnetworks_apache_spark_amd import _native
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import kmeans_ops as K

pytestmark = pytest.mark.gpu
GPU = "cuda"
WORST = {}
TYPES = pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    print(f"[exact figures] {key} = {value:.3e} (worst so far {WORST[key]:.3e})")


# ---------------------------------------------------------------------------------------------- exact_assign / exact_top2

def _lists(n, rng):
    """Row lists for the idx mode: count 0 and 1 for one row; else a count below the capacity and a full,
    permuted list."""
    if n == 1:
        return [np.zeros(0, np.int32), np.zeros(1, np.int32)]
    p = rng.permutation(n).astype(np.int32)
    return [p[:2 * n // 3], p]


def _check_top2(c, o, rows, lab0, D1, D2, where=None):
    """Labels and best of the listed rows, sentinels elsewhere, the bounds, the move log."""
    n = o["labels"].size
    E.check_assign(c["lab"], c["bd"], o["labels"], o["best"], rows=rows, lab0=lab0, best0=np.full(n, -1.0), where=where)
    rest = np.ones(n, dtype=bool)
    rest[rows] = False
    assert np.all(o["ub"][rest] == -7) and np.all(o["lb"][rest] == -7), "an unlisted row's bounds changed"
    E.check_moves(o["mv"], rows, lab0, o["labels"], fill=C.FILL)
    return E.check_top2_bounds(o["ub"], o["lb"], D1, D2, rows if where is None else where)


def _assign_lattice(form, f64, top2):
    d, k = C.ASSIGN_FORMS[form]
    rng = np.random.default_rng(d * 1000 + k)
    layouts = C.LAYOUTS if form in C.LAYOUT_FORMS else ("contig",)
    for n in C.ASSIGN_N:
        for dup in ((False, True) if k > 1 else (False,)):
            c = C.assign_lattice_case(form, n, dup)
            lab0 = C.other_labels(c["lab"], k)
            for layout in layouts:
                o = C.run_assign(GPU, c["X"], c["C"], f64, layout, lab0=lab0)
                E.check_assign(c["lab"], c["bd"], o["labels"], o["best"], lab0=lab0, changed=o["changed"])
            for lst in _lists(n, rng):
                o = C.run_assign(GPU, c["X"], c["C"], f64, layouts[-1], lab0=lab0, lst=lst)
                E.check_assign(c["lab"], c["bd"], o["labels"], o["best"], rows=lst, lab0=lab0,
                               best0=np.full(n, -1.0), changed=o["changed"])
                if top2:
                    o = C.run_assign(GPU, c["X"], c["C"], f64, layouts[-1], lab0=lab0, lst=lst, top2=True)
                    rows = lst.astype(np.int64)
                    wu, wl = _check_top2(c, o, rows, lab0, c["bd"][rows], c["sd"][rows])
                    note("exact_top2 ub/true - 1", wu)
                    note("exact_top2 1 - lb/true", wl)
                    if rows.size and 0 in rows:
                        assert o["ub"][0] == 0          # row 0 sits on its centre


def _assign_generic(form, f64, top2):
    d, k = C.ASSIGN_FORMS[form]
    c = C.assign_generic_case(form, f64)
    n, sub = c["n"], c["sub"]
    hl, hb = C.host_twin_assign(c["X"], c["C"])
    E.check_assign(c["lab"], c["bd"], hl, hb, where=sub)              # host twin == Fraction fold, here too
    lab0 = C.other_labels(hl, k)
    for layout in (("contig", "slice") if form in C.LAYOUT_FORMS else ("contig",)):
        o = C.run_assign(GPU, c["X"], c["C"], f64, layout, lab0=lab0)
        E.check_assign(c["lab"], c["bd"], o["labels"], o["best"], where=sub)
        E.check_assign(hl, hb, o["labels"], o["best"], lab0=lab0, changed=o["changed"])
    lst = np.concatenate([sub[::-1], np.setdiff1d(np.arange(0, n, 3), sub)]).astype(np.int32)
    o = C.run_assign(GPU, c["X"], c["C"], f64, lab0=lab0, lst=lst)
    E.check_assign(c["lab"], c["bd"], o["labels"], o["best"], rows=lst, where=sub)
    E.check_assign(hl, hb, o["labels"], o["best"], rows=lst, lab0=lab0, best0=np.full(n, -1.0), changed=o["changed"])
    if top2:
        D1, D2 = E.exact_top2_fraction(c["X"], c["C"], sub)
        for rows in (np.arange(n), lst.astype(np.int64)):
            o = C.run_assign(GPU, c["X"], c["C"], f64, lab0=lab0, lst=(None if rows.size == n else lst), top2=True)
            wu, wl = _check_top2(c, o, rows, lab0, D1, D2, where=sub)
            E.check_assign(hl, hb, o["labels"], o["best"], rows=rows)
            note("exact_top2 ub/true - 1", wu)
            note("exact_top2 1 - lb/true", wl)


@TYPES
@pytest.mark.parametrize("form", list(C.NARROW_FORMS))
def test_narrow_assign_on_lattice_rows(form, f64):
    """exact_assign_kernel<T, 4> / <T, 16>: labels and best exact on rows that sit on centres, bisectors
    and duplicates (k = 513: in the second LDS tile), the change counter, the idx mode's sentinels."""
    _assign_lattice(form, f64, top2=False)


@TYPES
@pytest.mark.parametrize("form", list(C.NARROW_FORMS))
def test_narrow_assign_equals_the_fraction_fold(form, f64):
    _assign_generic(form, f64, top2=False)


@TYPES
@pytest.mark.parametrize("form", list(C.WIDE_FORMS))
def test_wide_assign_and_top2_on_lattice_rows(form, f64):
    """One form of exact_assign_wide_kernel per case: ties across tiles and accumulator groups go to the
    lowest index; ub / lb are sound and inside W, 0 for a row on its centre, +inf for k = 1; the moves
    are the set of changed labels of the listed rows."""
    _assign_lattice(form, f64, top2=True)


@TYPES
@pytest.mark.parametrize("form", list(C.WIDE_FORMS))
def test_wide_assign_and_top2_equal_the_fraction_fold(form, f64):
    _assign_generic(form, f64, top2=True)


def test_wide_idx_mode_reaches_a_second_grid_stride_pass():
    """More listed rows than 4096 blocks of 256: the permuted full list of 1 048 876 lattice f32 rows."""
    c = C.big_idx_case()
    lab0 = C.other_labels(c["lab"], c["k"], every=997)
    o = C.run_assign(GPU, c["X"], c["C"], False, lab0=lab0, lst=c["lst"], top2=True)
    rows = np.arange(c["n"])
    wu, wl = _check_top2(c, o, rows, lab0, c["bd"], c["sd"])
    note("exact_top2 ub/true - 1", wu)
    note("exact_top2 1 - lb/true", wl)


# ---------------------------------------------------------------------------------------------- exact_dist

@TYPES
@pytest.mark.parametrize("k", C.DIST_K)
@pytest.mark.parametrize("d", C.DIST_D)
def test_exact_dist_equals_the_fold(d, k, f64):
    """best[r] is the fold against the label's own centre bit for bit: every load path (d), centres from
    LDS (k <= 256) and from global memory, with and without a label offset."""
    for n in C.DIST_N:
        for lattice in ((True, False) if n == 600 else (True,)):
            c = C.dist_case(d, k, n, f64, lattice)
            for off in ((0, 5) if n == 257 else ((5,) if lattice else (0,))):
                best = C.run_dist(GPU, c, f64, off)
                bad = c["sub"][E.bits64(best[c["sub"]]) != E.bits64(c["want"])]
                assert bad.size == 0, f"n={n} lab_off={off}: best differs from the fold at rows {bad[:5]}"


# ---------------------------------------------------------------------------------------------- bf16 copies

@TYPES
@pytest.mark.parametrize("d,ldo", C.ERR_SHAPES)
def test_to_bf16_err(d, ldo, f64):
    """The copy is torch's own rounding (through f32), every padding element 0 in a buffer that held
    0xFFFF, err sound and inside W_ERR."""
    for n in (1, 5):
        X = C.rows_case(n, d, f64)
        out, err = C.run_bf16_err(GPU, X, f64, d, ldo)
        assert np.array_equal(out[:, :d], C.torch_bf16_bits(X, f64))
        note("to_bf16_err err/true - 1", E.check_bf16_err(X, d, ldo, out, err))


@TYPES
def test_to_bf16_err_reaches_a_second_pass(f64):
    n, d, ldo = C.ERR_BIG
    X = C.rows_case(n, d, f64)
    out, err = C.run_bf16_err(GPU, X, f64, d, ldo)
    assert np.array_equal(out[:, :d], C.torch_bf16_bits(X, f64))
    note("to_bf16_err err/true - 1", E.check_bf16_err(X, d, ldo, out, err))


def _note_split(w):
    for key, v in zip(("ea", "eb", "en"), w[:3]):
        note(f"to_bf16_split {key}/true - 1", v)
    note("to_bf16_split |xn/true - 1|", w[3])


@TYPES
@pytest.mark.parametrize("d,ds,ldo", C.SPLIT_SHAPES)
def test_to_bf16_split(d, ds, ldo, f64):
    """[hi | lo | hi] and every padding position bit for bit (torch's rounding of x and of x - hi, through
    f32); ea, eb, en sound and inside W_SPLIT, xn within one f32 rounding; x = hi rows, rows of zeros."""
    for n in (1, 17):
        X = C.rows_case(n, d, f64)
        out, ea, eb, en, xn = C.run_bf16_split(GPU, X, f64, d, ds, ldo)
        assert np.array_equal(out, C.torch_split_layout(X, f64, d, ds, ldo))
        _note_split(E.check_split_rows(X, d, ds, ldo, out, ea, eb, en, xn))
        if n > 3:
            assert ea[1] == 0 and ea[2] == 0 and en[2] == 0 and xn[2] == 0


@TYPES
def test_to_bf16_split_reaches_a_second_round(f64):
    n, d, ds, ldo = C.SPLIT_BIG
    X = C.rows_case(n, d, f64)
    out, ea, eb, en, xn = C.run_bf16_split(GPU, X, f64, d, ds, ldo)
    assert np.array_equal(out, C.torch_split_layout(X, f64, d, ds, ldo))
    rows = list(range(0, n, 4099)) + list(range(n - 5, n))
    _note_split(E.check_split_rows(X, d, ds, ldo, out, ea, eb, en, xn, rows=rows))
    assert not np.any(np.isnan(ea)) and not np.any(np.isnan(eb)) and not np.any(np.isnan(en)) and not np.any(np.isnan(xn))


# ---------------------------------------------------------------------------------------------- the certificates

@pytest.mark.parametrize("name,outs", [(name, outs) for name in C.CERT_CASES for outs in ("separate", "aliased", "none")
                                       if name != "second_pass" or outs == "separate"])   # the large case runs once
def test_screen_cert(name, outs):
    """Rows on the line are listed (a strict >), rows GAP above it are not, rows below it are; the list is
    a set with its count and a sentinel behind it; u_out / l_out sound and inside W."""
    c = C.cert_case(name)
    lst, count, u, l = C.run_screen_cert(GPU, c, outs)
    wu, wl = E.check_screen_cert(c, lst, count, u, l, fill=C.FILL)
    if u is not None:
        note("screen_cert u_out/true - 1", wu)
        note("screen_cert 1 - l_out/true", wl)


@pytest.mark.parametrize("name", list(C.SPLIT_CERT_CASES))
def test_screen_cert_split(name):
    """The list is {i : not (u_out[i] < l_out[i])} from the outputs' own bits; u_out² >= ub² + E and l_out²
    <= max(lb² - E, 0) in rationals, inside W_LIST; lb² < E gives 0 and a listed row."""
    c = C.split_cert_case(name)
    lst, count, u, l = C.run_screen_cert_split(GPU, c)
    wu, wl = E.check_screen_cert_split(c, lst, count, u, l, fill=C.FILL)
    note("screen_cert_split u_out/true - 1", wu)
    note("screen_cert_split 1 - l_out/true", wl)
    pattern = C.SPLIT_CERT_CASES[name][1]
    assert (pattern != "all" or count == c["n"]) and (pattern != "none" or count == 0)


# ---------------------------------------------------------------------------------------------- sums

def _check_exact_sums(c, f64, cols=None):
    S, S_lo, cnt = C.run_sums(GPU, c, f64)
    E.check_sums(c["X"], c["L"], c["k"], S, S_lo, cnt, exact_rows=True, cols=cols)
    hS, hcnt, hlo = C.host_twin_sums(c["X"], c["L"], c["k"])
    assert np.array_equal(E.bits64(S), E.bits64(hS)) and np.array_equal(cnt, hcnt.astype(np.int64))
    return S, S_lo


@TYPES
@pytest.mark.parametrize("d", C.SUMS_D)
@pytest.mark.parametrize("name", list(C.SUMS_LAYOUTS))
def test_exact_sums_at_the_chunk_edges(name, d, f64):
    """exact_seg_partial / exact_seg_fix with cluster ends on the 1024-position chunk edges: S is the
    exact sum of the dyadic rows bit for bit, S_lo 0, the counts int32."""
    cols = None if d <= 65 else (0, 127, 128, 255, 256)
    S, S_lo = _check_exact_sums(C.sums_case(name, d), f64, cols)
    assert not S_lo.any()


@TYPES
@pytest.mark.parametrize("name", list(C.SUMS_SMALL))
def test_exact_sums_single_row_and_single_cluster(name, f64):
    _check_exact_sums(C.sums_case(name), f64)


@TYPES
def test_exact_sums_under_cancellation(f64):
    S, _ = _check_exact_sums(C.sums_cancel_case(), f64)
    assert not S[1].any()


def test_exact_sums_generic_rows_within_the_double_double_error():
    c = C.sums_generic_case()
    S, S_lo, cnt = C.run_sums(GPU, c, True)
    note("exact_sums |S + S_lo - exact| / sum of sizes", E.check_sums(c["X"], c["L"], c["k"], S, S_lo, cnt, exact_rows=False))
    hS, _, _ = C.host_twin_sums(c["X"], c["L"], c["k"])
    assert np.array_equal(E.bits64(S), E.bits64(hS))


@pytest.mark.parametrize("n", C.SUM_N)
def test_sum_exact(n):
    """sum_dd_partial / sum_dd_final: math.fsum's bits and the host's, up to the 1024-block cap."""
    v = C.sum_case(n)
    out = K.sum_exact(C.dev(v, GPU)).item()
    E.check_sum_exact(v, out)
    assert out == K.sum_exact(torch.as_tensor(v)).item()


# ---------------------------------------------------------------------------------------------- argument checks

def test_argument_checks_return_before_any_launch():
    """By return code only (hipErrorInvalidValue = 1), with n > 0: d = 0, ldo < d, ds % 8, idx without
    n_dev.  Every pointer is a real buffer, none is touched."""
    lib, s = _native.kernels(), _native.stream_ptr(None)
    x = torch.zeros(4, 8, dtype=torch.float64, device=GPU)
    c = torch.zeros(3, 8, dtype=torch.float64, device=GPU)
    i32 = torch.zeros(8, dtype=torch.int32, device=GPU)
    f64 = torch.zeros(8, dtype=torch.float64, device=GPU)
    f32 = [torch.zeros(8, dtype=torch.float32, device=GPU) for _ in range(4)]
    out = torch.zeros(4, 64, dtype=torch.int16, device=GPU)
    p = lambda t: t.data_ptr()   # noqa: E731
    assert lib.cml_kmeans_exact_assign(p(x), 1, 4, 8, 0, p(c), 3, p(i32), p(f64), 0, 0, 0, s) == 1
    assert lib.cml_kmeans_exact_assign(p(x), 1, 4, 8, 8, p(c), 3, p(i32), p(f64), 0, p(i32), 0, s) == 1
    assert lib.cml_kmeans_exact_dist(p(x), 1, 4, 8, 0, p(c), 3, p(i32), 0, p(f64), s) == 1
    assert lib.cml_kmeans_to_bf16_err(p(x), 1, 4, 8, 0, p(out), 64, p(f32[0]), s) == 1
    assert lib.cml_kmeans_to_bf16_err(p(x), 1, 4, 8, 8, p(out), 7, p(f32[0]), s) == 1
    assert lib.cml_kmeans_to_bf16_split(p(x), 1, 4, 8, 0, 8, p(out), 64, *(p(t) for t in f32), s) == 1
    assert lib.cml_kmeans_to_bf16_split(p(x), 1, 4, 8, 8, 12, p(out), 64, *(p(t) for t in f32), s) == 1
    torch.cuda.synchronize()
    assert not out.any() and not i32.any() and not f64.any()
