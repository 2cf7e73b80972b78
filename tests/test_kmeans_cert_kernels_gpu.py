"""The ten kernels of the certified pruned Lloyd step (``_native/csrc/kmeans_cert.hip``), kernel by
kernel through the wrappers of ``ops/kmeans_ops.py``, against the exact oracles of ``cert_oracle`` —
the cases of ``cert_cases``, whose promises (gaps, exactness) and whose checkers ``test_cert_oracle.py``
has tested on the CPU first.  Whole fits on Gaussian blobs are in test_kmeans_screen_gpu.py; there
almost every row is far from its bisectors, so an unsound certificate still gives the exact fit.  Here
every kernel meets the edges of its own: bounds on both sides of a rational window, strict ``<`` on
rows that sit exactly on the threshold, the top two drifts wherever they fall in a thread's stride,
list flushes in mid-loop, the second iteration of every grid-stride loop, slices of cert_delta with
fewer rows than slices — and a chained step on lattice rows that lie on bisectors.

Figures.  Every test prints what it measured and the worst value so far (``-s`` shows them); the
windows are asserted inside the checkers.  A run of this whole module on an MI355X printed the worst
values below, each beside the window it had to stay within (derived in ``cert_oracle`` from the
code's constants, not from a run):

  cert_stats     drift/true - 1   1.192e-07   measured on an MI355X   (window 1.195e-07 = 2^-23 + 3e-10)
  cert_stats     1 - s/true       1.187e-07   measured on an MI355X   (window 1.195e-07)
  cert_tighten   u/true - 1       1.192e-07   measured on an MI355X   (window 1.195e-07)
  cert_list      uu/true - 1      1.192e-07   measured on an MI355X   (window 1.195e-07, + 1e-11 for e)
  cert_list      1 - ll/true      1.192e-07   measured on an MI355X   (window 1.195e-07, + 1e-11 for e)
  cert_moves     shift2 rel. err  2.194e-16   measured on an MI355X   (bound 1e-12)

cert_bounds, the bf16 layout, every list, count and move, and the double-double sums are compared bit
for bit and have no figure.  The worst bound slack is one f32 ulp just above a power of two (2^-23).
"""
import numpy as np
import pytest
import torch

import cert_cases as C
import cert_oracle as O
from clustermachinelearningforhospitalnetworks_apache_spark_amd import _native
from clustermachinelearningforhospitalnetworks_apache_spark_amd.models.kmeans import LloydEngine
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import kmeans_ops as K

pytestmark = pytest.mark.gpu
GPU = "cuda"
WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    print(f"[cert figures] {key} = {value:.3e} (worst so far {WORST[key]:.3e})")


# ---------------------------------------------------------------------------------------------- cert_stats

@pytest.mark.parametrize("name", C.STATS_CASES)
def test_cert_stats(name):
    """s below and drift above the exact values within the window, exactly 0 / +inf where due; dtop the
    top two of the returned drifts bit for bit, with the index of the largest; the counters zeroed."""
    c = C.stats_case(name)
    s, drift, dtop, zero = C.run_stats(GPU, c)
    up, lo = O.check_stats(c["C"], c["Cold"], s, drift, dtop, zero)
    note("cert_stats drift/true - 1", up)
    note("cert_stats 1 - s/true", lo)
    if c.get("top"):
        assert int(dtop[2]) in (c["top"] if c.get("tie") else c["top"][:1])
    if "zero" in name:
        assert dtop[0] == 0 and dtop[1] == 0 and not drift.any()


def test_cert_stats_without_zero_buffer():
    c = C.stats_case("k257_d7")
    s, drift, dtop, _ = C.run_stats(GPU, c, with_zero=False)
    O.check_stats(c["C"], c["Cold"], s, drift, dtop)


# ---------------------------------------------------------------------------------------------- cert_bounds

@pytest.mark.parametrize("name", list(C.BOUNDS_CASES))
def test_cert_bounds(name):
    """u' and l' bit for bit on every row, list A as a set with its count, nothing written past it."""
    c = C.bounds_case(name)
    u, l, lst, count = C.run_bounds(GPU, c)
    listed = O.check_bounds(c, u, l, lst, count)
    if name == "none_listed":
        assert count == 0 and np.all(lst == -1)
    if name in ("all_listed", "flush"):
        assert listed.size == c["n"]


# ---------------------------------------------------------------------------------------------- cert_tighten

@pytest.mark.parametrize("name", list(C.TIGHTEN_CASES))
def test_cert_tighten(name):
    """Only list A's rows change u; the new u is the distance to the label's centre within the window
    (0 for a row on its centre); list B is the oracle's set; bxn / blab sit beside it."""
    c = C.tighten_case(name)
    u, lbst, nb, bxn, blab = C.run_tighten(GPU, c)
    note("cert_tighten u/true - 1", O.check_tighten(c, u, lbst, nb, bxn, blab))


# ---------------------------------------------------------------------------------------------- split_centres

@pytest.mark.parametrize("name", list(C.SPLIT_CASES))
def test_split_centres(name):
    """[c_hi | c_hi | c_lo] by torch's own f64 -> f32 -> bf16 rounding, zero padding, the norms and the
    certificate's constants."""
    c = C.split_case(name)
    cb, cn, cst, mc = C.run_split(GPU, c)
    assert np.array_equal(cb, C.split_layout_torch(c))
    O.check_split(c["C"], c["kp"], c["ds"], cb, cn, cst, mc)


# ---------------------------------------------------------------------------------------------- cert_list

@pytest.mark.parametrize("name", list(C.LIST_CASES))
def test_cert_list(name):
    c = C.list_case(name)
    lab, u, l, lc, nc, mv = C.run_list(GPU, c)
    wu, wl = O.check_list(c, lab, u, l, lc, nc, mv)
    note("cert_list uu/true - 1", wu)
    note("cert_list 1 - ll/true", wl)


# ---------------------------------------------------------------------------------------------- cert_moves

@pytest.mark.parametrize("name", list(C.MOVES_CASES))
def test_cert_moves(name):
    """hist, scan, scatter, delta and apply together: the sums and counts of the moved labels are the
    from-scratch ones bit for bit, seg / perm hold every bin's rows, C_next = S_hi / cnt."""
    c = C.moves_case(name)
    out = C.run_moves(GPU, c)
    note("cert_moves shift2 relative error", O.check_moves(c, **out))


def test_cert_moves_refuses_an_oversized_k():
    """4 k ints of dynamic LDS for k > 4096 pass the 64 KiB default limit: refused before any launch
    (the return code alone: no pointer is touched)."""
    st = _native.kernels().cml_kmeans_cert_moves(0, 0, 0, 1, 2, 4097, *([0] * 16), _native.stream_ptr(None))
    assert st == 1  # hipErrorInvalidValue


# ---------------------------------------------------------------------------------------------- the chained step

def _check_chain_state(ch, c):
    """The labels are exact_assign's, both bounds hold for every row, the sums, counts and the next
    centres are the from-scratch ones bit for bit; returns the counts."""
    ref, _ = K.exact_assign(ch.x, ch.C_used)
    assert torch.equal(ch.lab, ref)
    O.check_step_bounds(c["X"], C.host(ch.C_used), C.host(ch.lab), C.host(ch.u), C.host(ch.l))
    S, cnt, S_lo = K.exact_sums(ch.x, ch.lab, c["k"], with_lo=True, counts_int=True)
    assert torch.equal(ch.cnt, cnt)
    assert np.array_equal(O.bits64(C.host(ch.S_hi)), O.bits64(C.host(S)))
    assert np.array_equal(O.bits64(C.host(ch.S_lo)), O.bits64(C.host(S_lo)))
    want = torch.where((cnt > 0)[:, None], S / cnt.clamp(min=1).to(torch.float64)[:, None], ch.C_used)
    assert np.array_equal(O.bits64(C.host(ch.C)), O.bits64(C.host(want)))
    return C.host(cnt).copy()


@pytest.mark.parametrize("name", list(C.CHAIN_CASES))
def test_chained_certified_steps_on_a_lattice(name):
    """cert_stats, cert_bounds, cert_tighten, exact_top2 with moves, cert_moves, as _step_screen chains
    them, for 6 steps on lattice rows: after every step the labels are exact_assign's, both bounds hold
    for every row, and the sums are the from-scratch ones.  The first assignment (a full exact_top2)
    meets the rows that lie on bisectors of the integer centres; a seventh, certified step back to
    those integer centres puts the same ties in front of cert_bounds and cert_tighten, which must
    leave every one of them to the exact fold."""
    c = C.chain_case(name)
    k, n = c["k"], c["n"]
    ch = C.Chain(GPU, c, f64=(c["d"] > 2))
    lab0 = ch.lab.clone()
    counts = [C.host(ch.cnt).copy()]
    pruned = moved = 0
    for _ in range(6):
        a, b, m = ch.step()
        assert b <= a <= n
        pruned += n - a
        moved += m
        counts.append(_check_chain_state(ch, c))
    assert pruned > 0 and moved > 0                       # the certificate proved rows, and labels moved
    if c["emptied"] is not None:
        e = c["emptied"]
        assert counts[0][e] == 2 and counts[1][e] == 0 and counts[-1][e] == 0
    if c["dup"]:
        assert counts[0][c["dup"][1]] == 0 < counts[0][c["dup"][0]]
    # back to the integer centres in one certified step: the tied rows cannot be proven (u >= l for them)
    D2 = np.sort(C.numpy_sqdist(c["X"], c["C0"]), axis=1)                 # integers: exact
    ties = int((D2[:, 0] == D2[:, 1]).sum())
    assert ties >= 50
    a, b, m = ch.restart(c["C0"])
    assert ties <= b <= a <= n
    assert np.array_equal(_check_chain_state(ch, c), counts[0]) and torch.equal(ch.lab, lab0)


def test_engine_screen_equals_exact_on_the_lattice():
    """The same lattice rows through LloydEngine: precision "screen" (split layout) against "exact",
    labels and centres after every step."""
    c = C.chain_case(C.ENGINE_CASE)
    x = C.rows_tensor(c["X"], True, GPU)
    eng = {}
    for prec in ("exact", "screen"):
        e = LloydEngine(x, c["d"], c["k"], precision=prec)
        assert e.precision == prec
        e.set_centers(c["C0"].copy())
        eng[prec] = e
    for step in range(6):
        for e in eng.values():
            e.step()
        assert eng["screen"]._scr.split
        assert torch.equal(eng["exact"].labels[:c["n"]].long(), eng["screen"].labels[:c["n"]].long()), step
        assert np.array_equal(O.bits64(C.host(eng["exact"].centers)), O.bits64(C.host(eng["screen"].centers))), step
    assert eng["screen"]._scr.cert.valid                   # the later steps were certified ones
