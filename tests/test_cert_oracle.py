"""The oracles and checkers of ``cert_oracle`` / ``cert_cases`` on the CPU: their own invariants, the
properties the cases promise (gaps of the list cases, exactness of the dyadic data), and for every
checker a correct output built by the oracle (passes) and mutants of it (each must fail) — the proof
that ``test_kmeans_cert_kernels_gpu.py`` can fail."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import cert_cases as C
import cert_oracle as O

F32 = np.float32


def ulp_toward(a, target):
    return np.nextafter(np.asarray(a, dtype=F32), F32(target)).astype(F32)


# ---------------------------------------------------------------------------------------------- the oracle itself

def test_directed_roundings_never_round_inward():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-30, 30, 2000), [0.0, 1.0, 1 + 2.0 ** -30,
                        1 - 2.0 ** -30, 2.0 ** -140, 3e38, 16777217.0, -1.0, -2.0 ** -30]])
    up, dn = O.f32_up(v), O.f32_dn(v)
    for x, a, b in zip(v, up, dn):
        assert Fraction(float(a)) >= Fraction(float(x))                      # never below
        assert a == -np.inf or Fraction(float(np.nextafter(a, F32(-np.inf)))) < Fraction(float(x))  # the least such
        if x > 0:
            assert 0 <= Fraction(float(b)) <= Fraction(float(x))
            assert Fraction(float(np.nextafter(b, F32(np.inf)))) > Fraction(float(x))
        else:
            assert b == 0
    assert np.isnan(O.f32_up(np.array([np.nan])))[0] and O.f32_dn(np.array([np.nan]))[0] == 0
    assert O.f32_up(np.array([np.inf]))[0] == np.inf


def test_bf16_rounding_is_torchs():
    rng = np.random.default_rng(2)
    f = np.concatenate([rng.standard_normal(5000) * 10.0 ** rng.integers(-10, 10, 5000),
                        [1.00390625, 1.01171875, 1.0 + 2.0 ** -8, 0.0, -0.0]]).astype(F32)
    want = torch.as_tensor(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(O.bf16_bits(f), want)
    assert np.array_equal(O.bf16_value(want), torch.as_tensor(f).to(torch.bfloat16).float().numpy())
    for name in ("k3_kp32_d5_ds8_wide", "k40_kp64_d170_ds176_tight", "random_f64"):
        c = C.split_case(name)
        assert np.array_equal(O.split_oracle(c["C"], c["kp"], c["ds"], c["ldc"])[0], C.split_layout_torch(c))


def test_dyadic_data_is_exact_in_f64():
    """The fast paths (plain f64 on dyadic data) give the Fractions' values."""
    rng = np.random.default_rng(3)
    X, Cn = C.dyadic(rng, (40, 130), span=512), C.dyadic(rng, (3, 130), span=512)
    lab = rng.integers(0, 3, 40)
    fast = O.sqdist_rows(X, Cn, lab)
    assert isinstance(fast, np.ndarray)
    assert all(Fraction(float(f)) == O.sqdist_fraction(X[r], Cn[lab[r]]) for r, f in enumerate(fast))
    assert not O.is_dyadic(X + 2.0 ** -9) and not O.is_dyadic(X * 4) and not O.is_dyadic(np.zeros((2, 1025)))
    assert not isinstance(O.sqdist_rows(X + 1e-3, Cn, lab), np.ndarray)
    for name in C.STATS_CASES:
        c = C.stats_case(name)
        assert O.is_dyadic(c["C"], c["Cold"]) == (name != "random_f64")
    for name in C.TIGHTEN_CASES:
        c = C.tighten_case(name)
        assert O.is_dyadic(c["X"], c["C"]) == (name != "random_f64")
    for name in C.SPLIT_CASES:
        c = C.split_case(name)
        _, lo, rc = O.split_oracle(c["C"], c["kp"], c["ds"], c["ldc"])
        assert O.is_dyadic(c["C"], lo, rc) == (name != "random_f64")
        assert np.any(lo != 0) and (c["k"] * c["d"] < 100 or np.any(rc != 0))   # all three constants are live
    for name in ("k5_d63", "big", "strided"):
        c = C.moves_case(name)
        assert O.is_dyadic(c["X"]) and c["X"].shape[0] < 2 ** 20
        if not c["f64"]:
            assert np.array_equal(c["X"].astype(F32).astype(np.float64), c["X"])


@pytest.mark.parametrize("name", list(C.TIGHTEN_CASES))
def test_tighten_cases_have_the_gap(name):
    """Every list-A row's u and its threshold are equal or 4 f32 ulps apart: no row is ambiguous."""
    c = C.tighten_case(name)
    rows = c["la"][:c["na"]].astype(np.int64)
    assert np.unique(rows).size == rows.size
    _, u_or, thr, listed = O.tighten_oracle(c["X"], c["C"], c["lab"], c["l"], c["s"], rows)
    assert O.gap_holds(u_or, thr)
    if c["na"] >= 17:
        assert np.any(u_or == thr) or name == "random_f64"       # the equality rows are there
        assert 0 < listed.size
        assert (listed.size == rows.size) == (name == "flush")
        assert np.any(u_or == 0) or name == "random_f64"
    if name == "flush":                                          # the busiest block overruns kBuf - 256
        assert -(-c["na"] // (1024 * 16)) * 16 > O.KBUF - 256


@pytest.mark.parametrize("name", list(C.LIST_CASES))
def test_list_cases_have_the_gap(name):
    c = C.list_case(name)
    uu, ll, bad = O.list_oracle(c)
    assert O.gap_holds(uu, ll)
    rows = c["lst"][:c["cnt"]].astype(np.int64)
    l2 = c["l"][rows].astype(np.float64) ** 2
    ea, eb, en = (c[n][rows].astype(np.float64) for n in ("ea", "eb", "en"))
    e = 2.0 * (ea * c["cst"][0] + eb * c["cst"][1] + 1.01 * en * c["cst"][2]) * (1.0 + 1e-6)   # ~1e-15 off
    assert np.all(np.abs(l2 - e) >= 1.001e-3 * l2)               # the premise of W_LIST, on every row
    for i, r in enumerate(rows[:50]):                            # the f64 form is the Fractions' value
        assert abs(float(O.list_slack(c, r)[1]) - e[i]) <= 1e-14 * e[i]
    if c["cnt"] >= 255:
        assert np.any(uu == ll) and np.any(bad) and np.any(~bad)
        assert np.any((l2 < e) & (e > 0)) and np.any(e == 0)


def test_bounds_cases_hold_their_edges():
    c = C.bounds_case("n262145")
    un, ln, listed = O.bounds_oracle(c["lab"], c["u"], c["l"], c["drift"], c["dtop"], c["s"])
    on = np.zeros(c["n"], dtype=bool)
    on[listed] = True
    eq = (c["lab"] == C.I_EQ) & np.isfinite(c["u"])
    assert eq.any() and np.all(un[eq] == c["s"][C.I_EQ]) and on[eq].all()
    assert on[np.isnan(c["u"])].all() and on[np.isinf(c["u"])].all()
    inf_s = (c["lab"] == C.I_INF) & np.isfinite(c["u"])
    assert inf_s.any() and not on[inf_s].any()
    assert np.any((ln == 0) & (c["l"] > 0)) and np.any(c["lab"] == C.I_TOP) and 0 < listed.size < c["n"]
    assert O.bounds_oracle(*[C.bounds_case("none_listed")[n] for n in ("lab", "u", "l", "drift", "dtop", "s")])[2].size == 0
    f = C.bounds_case("flush")
    assert O.bounds_oracle(*[f[n] for n in ("lab", "u", "l", "drift", "dtop", "s")])[2].size == f["n"]
    assert (-(-f["n"] // (1024 * 256)) - 1) * 256 > O.KBUF - 256  # full before the last iteration


@pytest.mark.parametrize("name", ["k5_d2", "k300_d17"])
def test_hamerly_update_keeps_the_lattice_bounds_sound(name):
    """Exact first assignment, the means as new centres, the drifts by the kernel's formula, the
    Hamerly update of the oracle: the moved bounds still hold against the Fractions' distances."""
    c = C.chain_case(name)
    X, C0, k = c["X"], c["C0"], c["k"]
    D2 = C.numpy_sqdist(X, C0)                                       # integers: exact
    lab = D2.argmin(axis=1)
    own = D2[np.arange(len(X)), lab]
    D2[np.arange(len(X)), lab] = np.inf
    other = D2.min(axis=1)
    assert int((own == other).sum()) >= 50                           # rows exactly on a bisector
    u, l = O.f32_up(np.sqrt(own) * (1 + 1e-10)), O.f32_dn(np.sqrt(other) * (1 - 1e-10))
    cnt = np.bincount(lab, minlength=k)
    S = np.stack([np.bincount(lab, weights=X[:, t], minlength=k) for t in range(X.shape[1])], axis=1)
    C1 = np.where((cnt > 0)[:, None], S / np.maximum(cnt, 1)[:, None], C0)
    _, drift, dtop, _ = C.stats_oracle_output(dict(C=C1, Cold=C0))
    un, ln = O.hamerly_update(u, l, lab, drift, dtop)
    O.check_step_bounds(X, C1, lab, un, ln)
    # the checker fails on a bound that is 1e-6 (8 f32 ulps) on the wrong side of the f64 distance
    r = int(np.argmax(own > 0))
    D1 = np.sqrt(C.numpy_sqdist(X[r:r + 1], C1)[0])
    bad_u, bad_l = un.copy(), ln.copy()
    bad_u[r] = F32(D1[lab[r]] * (1 - 1e-6))
    bad_l[r] = F32(np.delete(D1, lab[r]).min() * (1 + 1e-6))
    with pytest.raises(AssertionError):
        O.check_step_bounds(X[r:r + 1], C1, lab[r:r + 1], bad_u[r:r + 1], ln[r:r + 1])
    with pytest.raises(AssertionError):
        O.check_step_bounds(X[r:r + 1], C1, lab[r:r + 1], un[r:r + 1], bad_l[r:r + 1])
    # the case's own promises: the gadget's middle cluster owns rows now and none after the next step
    e = c["emptied"]
    assert cnt[e] == 2
    lab1 = C.numpy_sqdist(X, C1).argmin(axis=1)
    assert np.bincount(lab1, minlength=k)[e] == 0
    if c["dup"]:
        assert np.array_equal(C0[c["dup"][0]], C0[c["dup"][1]]) and cnt[c["dup"][1]] == 0 < cnt[c["dup"][0]]


# ---------------------------------------------------------------------------------------------- checkers and mutants

@pytest.mark.parametrize("name", ["k3_d7", "k257_d130", "top_ge_256", "same_stride_rev", "tie", "all_zero_k1",
                                  "random_f64"])
def test_check_stats_passes_the_oracle_and_fails_mutants(name):
    c = C.stats_case(name)
    s, drift, dtop, zero = C.stats_oracle_output(c)
    O.check_stats(c["C"], c["Cold"], s, drift, dtop, zero)
    if c.get("top"):
        assert int(dtop[2]) in c["top"] and {int(np.argsort(drift)[-1]), int(np.argsort(drift)[-2])} == set(c["top"])
    k = len(s)
    if name == "all_zero_k1":
        assert dtop[1] == 0 and s[0] == np.inf
        with pytest.raises(AssertionError):
            O.check_stats(c["C"], c["Cold"], np.array([3e38], dtype=F32), drift, dtop, zero)
        return
    # only the entries whose true value is not 0 move, so each mutant fails on the soundness comparison
    # it names, not on "a true value of 0 gives exactly 0"
    assert np.any(drift > 0) and np.any(s > 0)
    with pytest.raises(AssertionError, match="unsound upper bound"):      # u one f32 ulp low
        O.check_stats(c["C"], c["Cold"], s, np.where(drift > 0, ulp_toward(drift, -np.inf), drift), dtop, zero)
    with pytest.raises(AssertionError, match="unsound lower bound"):      # l one ulp high
        O.check_stats(c["C"], c["Cold"], np.where(s > 0, ulp_toward(s, np.inf), s), drift, dtop, zero)
    if np.any(drift == 0):
        with pytest.raises(AssertionError, match="exactly 0"):            # an unmoved centre with a drift
            O.check_stats(c["C"], c["Cold"], s, np.where(drift == 0, F32(1e-30), drift), dtop, zero)
    with pytest.raises(AssertionError):                                   # a loose bound
        O.check_stats(c["C"], c["Cold"], s, drift * F32(1 + 2.0 ** -21), dtop * np.array([1 + 2.0 ** -21, 1 + 2.0 ** -21, 1, 1], dtype=F32), zero)
    if not c.get("tie"):
        with pytest.raises(AssertionError):                               # dtop[0] / dtop[1] swapped
            O.check_stats(c["C"], c["Cold"], s, drift, dtop[[1, 0, 2, 3]], zero)
    for step in (-1, 1):                                                  # dtop[2] off by one
        with pytest.raises(AssertionError):
            O.check_stats(c["C"], c["Cold"], s, drift, dtop + np.array([0, 0, step, 0], dtype=F32), zero)
    with pytest.raises(AssertionError):
        O.check_stats(c["C"], c["Cold"], s, drift, dtop, np.where(np.arange(zero.size) == 5, 1, zero))


@pytest.mark.parametrize("name", ["n257", "n262145", "all_listed", "none_listed"])
def test_check_bounds_passes_the_oracle_and_fails_mutants(name):
    c = C.bounds_case(name)
    un, ln, lst, cnt = C.bounds_oracle_output(c)
    O.check_bounds(c, un, ln, lst, cnt)
    with pytest.raises(AssertionError):                                   # u one ulp low
        O.check_bounds(c, np.where(np.arange(c["n"]) == 7, ulp_toward(un, -np.inf), un), ln, lst, cnt)
    with pytest.raises(AssertionError):                                   # l one ulp high
        O.check_bounds(c, un, np.where(np.arange(c["n"]) == 9, ulp_toward(ln, np.inf), ln), lst, cnt)
    if name != "none_listed":                                             # d1 used where d2 is due
        top = c["lab"] == C.I_TOP
        l_wrong = np.where(top, O.f32_dn(c["l"].astype(np.float64) - float(c["dtop"][0])), ln)
        assert top.any() and np.any(O.bits32(l_wrong) != O.bits32(ln))
        with pytest.raises(AssertionError):
            O.check_bounds(c, un, l_wrong, lst, cnt)
        with pytest.raises(AssertionError):                               # one row missing
            O.check_bounds(c, un, ln, np.concatenate([lst[1:cnt], [-1], lst[cnt:]]), cnt - 1)
        with pytest.raises(AssertionError):                               # one row listed twice
            O.check_bounds(c, un, ln, np.concatenate([lst[:cnt - 1], lst[:1], lst[cnt:]]), cnt)
    else:
        with pytest.raises(AssertionError):                               # the list was touched
            O.check_bounds(c, un, ln, np.where(np.arange(c["n"]) == 0, 3, lst), cnt)
    if name == "n262145":                                                 # the equality rows left out
        eq = (c["lab"] == C.I_EQ) & np.isfinite(c["u"])
        keep = lst[:cnt][~eq[lst[:cnt]]]
        short = np.full(c["n"], -1, dtype=np.int32)
        short[:keep.size] = keep
        with pytest.raises(AssertionError):
            O.check_bounds(c, un, ln, short, keep.size)


@pytest.mark.parametrize("name", ["d17_f32", "d129_f64", "strided", "random_f64", "na0", "na1"])
def test_check_tighten_passes_the_oracle_and_fails_mutants(name):
    c = C.tighten_case(name)
    u, lbst, nb, bxn, blab = C.tighten_oracle_output(c)
    O.check_tighten(c, u, lbst, nb, bxn, blab)
    if c["na"] == 0:
        with pytest.raises(AssertionError):
            O.check_tighten(c, np.where(np.arange(c["n"]) == 3, F32(1.0), u), lbst, nb)
        return
    rows = c["la"][:c["na"]].astype(np.int64)
    on = np.zeros(c["n"], dtype=bool)
    on[rows] = True
    with pytest.raises(AssertionError, match="unsound upper bound"):      # u one ulp low where it is not 0
        O.check_tighten(c, np.where(on & (u > 0), ulp_toward(u, -np.inf), u), lbst, nb)
    if np.any(on & (u == 0)):
        with pytest.raises(AssertionError, match="exactly 0"):            # a row on its centre with u > 0
            O.check_tighten(c, np.where(on & (u == 0), F32(1e-30), u), lbst, nb)
    with pytest.raises(AssertionError, match="loose upper bound"):        # three ulps high
        O.check_tighten(c, np.where(on & (u > 0), ulp_toward(ulp_toward(ulp_toward(u, np.inf), np.inf), np.inf), u), lbst, nb)
    off = np.nonzero(~on)[0][0]
    with pytest.raises(AssertionError):                                   # a row outside list A written
        O.check_tighten(c, np.where(np.arange(c["n"]) == off, ulp_toward(u, np.inf), u), lbst, nb)
    if nb >= 2:
        with pytest.raises(AssertionError):                               # one row missing
            O.check_tighten(c, u, np.concatenate([lbst[1:nb], [-1], lbst[nb:]]), nb - 1)
        with pytest.raises(AssertionError):                               # one row twice
            O.check_tighten(c, u, np.concatenate([lbst[:nb - 1], lbst[:1], lbst[nb:]]), nb)
        _, u_or, thr, _ = O.tighten_oracle(c["X"], c["C"], c["lab"], c["l"], c["s"], rows)
        eq = set(rows[u_or == thr].tolist())
        if eq:                                                            # the equality rows left out
            keep = np.array([r for r in lbst[:nb] if r not in eq], dtype=np.int32)
            short = np.full(c["n"], -1, dtype=np.int32)
            short[:keep.size] = keep
            with pytest.raises(AssertionError):
                O.check_tighten(c, u, short, keep.size)
        if c["ext"]:
            with pytest.raises(AssertionError):
                O.check_tighten(c, u, lbst, nb, np.roll(bxn, 1), blab)
            with pytest.raises(AssertionError):
                O.check_tighten(c, u, lbst, nb, bxn, np.where(np.arange(c["n"]) == 1, blab + 1, blab))


@pytest.mark.parametrize("name", ["k3_kp32_d5_ds8_wide", "k40_kp64_d170_ds176_tight", "k1_kp32_d128_ds128_tight",
                                  "random_f64"])
def test_check_split_passes_the_oracle_and_fails_mutants(name):
    c = C.split_case(name)
    cb, cn, cst, mc = C.split_oracle_output(c)
    k, d, ds = c["k"], c["d"], c["ds"]
    O.check_split(c["C"], c["kp"], ds, cb, cn, cst, mc)
    swapped = cb.copy()                                                   # c_lo placed in the second segment
    swapped[:, ds:2 * ds], swapped[:, 2 * ds:3 * ds] = cb[:, 2 * ds:3 * ds], cb[:, ds:2 * ds]
    with pytest.raises(AssertionError):
        O.check_split(c["C"], c["kp"], ds, swapped, cn, cst, mc)
    for col in (d if d < ds else None, 3 * ds if c["ldc"] > 3 * ds else None):
        if col is not None:                                               # padding columns not zero
            dirty = cb.copy()
            dirty[0, col] = 0x3F80
            with pytest.raises(AssertionError):
                O.check_split(c["C"], c["kp"], ds, dirty, cn, cst, mc)
    flip = cb.copy()
    flip[0, 0] ^= 1                                                       # one bf16 ulp
    with pytest.raises(AssertionError):
        O.check_split(c["C"], c["kp"], ds, flip, cn, cst, mc)
    with pytest.raises(AssertionError):                                   # padding norm finite
        O.check_split(c["C"], c["kp"], ds, cb, np.where(np.arange(c["kp"]) == k, F32(0), cn), cst, mc)
    with pytest.raises(AssertionError):                                   # cn two ulps off
        O.check_split(c["C"], c["kp"], ds, cb, np.where(np.arange(c["kp"]) == 0, ulp_toward(ulp_toward(cn, np.inf), np.inf), cn), cst, mc)
    for i in range(3):
        for f in (1 - 1.5e-9, 1 + 1e-8):                                  # below the maximum; loose
            if cst[i] == 0:
                continue
            bad = cst.copy()
            bad[i] *= f
            with pytest.raises(AssertionError):
                O.check_split(c["C"], c["kp"], ds, cb, cn, bad, mc)
    with pytest.raises(AssertionError):
        O.check_split(c["C"], c["kp"], ds, cb, cn, cst, ulp_toward(mc, 0))


@pytest.mark.parametrize("name", ["cnt1", "cnt257"])
def test_check_list_passes_the_oracle_and_fails_mutants(name):
    c = C.list_case(name)
    lab, u, l, lc, nc, mv = C.list_oracle_output(c)
    O.check_list(c, lab, u, l, lc, nc, mv)
    rows = c["lst"][:c["cnt"]].astype(np.int64)
    _, _, bad = O.list_oracle(c)
    good = np.zeros(c["n"], dtype=bool)
    good[rows[~bad]] = True
    with pytest.raises(AssertionError):                                   # u one ulp low
        O.check_list(c, lab, np.where(good, ulp_toward(u, -np.inf), u), l, lc, nc, mv)
    with pytest.raises(AssertionError):                                   # l one ulp high
        O.check_list(c, lab, u, np.where(good, ulp_toward(l, np.inf), l), lc, nc, mv)
    with pytest.raises(AssertionError):                                   # loose
        O.check_list(c, lab, u * np.where(good, F32(1 + 2.0 ** -21), F32(1)), l, lc, nc, mv)
    if name == "cnt1":
        return
    with pytest.raises(AssertionError):                                   # an uncertified row kept the new label
        r = rows[bad][np.nonzero(c["lab"][rows[bad]] != c["blab"][:c["cnt"]][bad])[0][0]]
        O.check_list(c, np.where(np.arange(c["n"]) == r, c["lab"], lab), u, l, lc, nc, mv)
    with pytest.raises(AssertionError):                                   # one row missing from list C
        O.check_list(c, lab, u, l, np.concatenate([lc[1:nc], [-1], lc[nc:]]), nc - 1, mv)
    with pytest.raises(AssertionError):                                   # one row twice
        O.check_list(c, lab, u, l, np.concatenate([lc[:nc - 1], lc[:1], lc[nc:]]), nc, mv)
    eq = set(rows[(c["u"][rows] == 1.0) & (c["ea"][rows] == 0)].tolist())  # the equality rows left out
    keep = np.array([r for r in lc[:nc] if r not in eq], dtype=np.int32)
    assert 0 < keep.size < nc
    with pytest.raises(AssertionError):
        O.check_list(c, lab, u, l, np.concatenate([keep, np.full(c["n"] - keep.size, -1, np.int32)]), keep.size, mv)
    m1 = mv[3]
    assert m1 > C.LIST_M0 + 2
    with pytest.raises(AssertionError):                                   # one move dropped
        O.check_list(c, lab, u, l, lc, nc, (mv[0], mv[1], mv[2], m1 - 1))
    with pytest.raises(AssertionError):                                   # old and new swapped
        O.check_list(c, lab, u, l, lc, nc, (mv[0], mv[2], mv[1], m1))
    with pytest.raises(AssertionError):                                   # the earlier entries overwritten
        O.check_list(c, lab, u, l, lc, nc, (np.where(np.arange(mv[0].size) == 0, 1, mv[0]), mv[1], mv[2], m1))


@pytest.mark.parametrize("name", ["k2_d1", "k5_d63", "k64_d65", "no_moves", "one_move", "k2_emptied", "random_f64",
                                  "random_f32"])
def test_check_moves_passes_the_oracle_and_fails_mutants(name):
    c = C.moves_case(name)
    o = C.moves_oracle_output(c)
    O.check_moves(c, **o)
    k = c["k"]

    def mutated(**kw):
        with pytest.raises(AssertionError):
            O.check_moves(c, **{**o, **kw})

    S = o["S_hi"].copy()
    S[k - 1, 0] = np.nextafter(S[k - 1, 0], np.inf)                       # S_hi one ulp off
    mutated(S_hi=S)
    cnt = o["cnt"].copy()
    cnt[0] += 1                                                           # cnt off by one
    mutated(cnt=cnt)
    if "random" in name:                                                  # the low parts are live
        assert not O.is_dyadic(c["X"]) and np.count_nonzero(o["S_lo"]) > o["S_lo"].size // 2
        mutated(S_lo=np.zeros_like(o["S_lo"]))                            # S_lo dropped
        mutated(S_lo=o["S_lo"] * (1 + 2.0 ** -20))                        # S_lo perturbed
        lo = o["S_lo"].copy()
        lo[k - 1, 0] += np.abs(o["S_hi"][k - 1, 0]) * 2.0 ** -70          # one remainder lost on the way
        mutated(S_lo=lo)
        mutated(S_lo=o["S_hi"] * 2.0 ** -40)                              # not normalised
    else:
        lo = o["S_lo"].copy()
        lo[0, 0] = 2.0 ** -60                                             # exactly summable rows: S_lo is 0
        mutated(S_lo=lo)
    Cn = o["C_next"].copy()
    Cn[0, 0] = np.nextafter(Cn[0, 0], np.inf)
    mutated(C_next=Cn)
    sh = o["shift2"].copy()
    sh[0] *= 1 + 1e-11
    mutated(shift2=sh)
    m = c["rows"].size
    if m:
        seg = o["seg"].copy()
        seg[-1] -= 1
        mutated(seg=seg)
        perm = o["perm"].copy()
        perm[0] = perm[0] + 1 if perm[0] + 1 < c["n"] else perm[0] - 1    # a wrong row in a bin
        mutated(perm=perm)
        # one move dropped: the sums and counts of the labels without it
        short = dict(c, rows=c["rows"][1:], old=c["old"][1:], new=c["new"][1:])
        o2 = C.moves_oracle_output(short)
        mutated(S_hi=o2["S_hi"], cnt=o2["cnt"], C_next=o2["C_next"], shift2=o2["shift2"])
        mutated(S_hi=o2["S_hi"], cnt=o2["cnt"], C_next=o2["C_next"], shift2=o2["shift2"], seg=o2["seg"], perm=o2["perm"])
    if name == "k5_d63":
        L1 = O.apply_moves(c["L0"], c["rows"], c["new"])
        got, lost = np.bincount(c["new"], minlength=k), np.bincount(c["old"], minlength=k)
        assert got[0] == 3 and got[1] % 4 and lost[1] and np.bincount(L1, minlength=k)[3] == 0 < lost[3]
