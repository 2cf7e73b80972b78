"""Named, seeded cases for the kernels of ``_native/csrc/kmeans_exact.hip`` and the runners that put
them through the wrappers of ``ops/kmeans_ops.py``, shared by ``test_exact_oracle.py`` (the oracle and
the checkers, any machine) and ``test_kmeans_exact_kernels_gpu.py`` (the kernels).  Builders return
plain numpy; every case is built once per process and never modified.

Two kinds of rows.  *Lattice* rows (``exact_oracle.is_lattice``: integers and half-integers) make every
squared distance exact in f64, so plain numpy is the oracle at any size, and rows can sit exactly on
their centre, on a bisector or on a duplicate centre.  *Generic* rows are random and non-dyadic: the
Fraction fold decides a subset of them bit for bit, the host twin (which ``test_exact_oracle.py`` has
compared with the Fraction fold) the rest.
"""
import functools

import numpy as np
import torch

import exact_oracle as E
from cert_cases import _seed, dev, dyadic, host
from clustermachinelearningforhospitalnetworks_apache_spark_amd import _native
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import kmeans_ops as K

F32, F64 = np.float32, np.float64
FILL = -1

# ---------------------------------------------------------------------------------------------- assign

# name -> (d, k).  Narrow: exact_assign_kernel<T, 4> (d <= 4) and <T, 16> (d <= 16); kt = min(k, 8192 / d),
# so (16, 513) puts centre 512 in a second LDS tile.
NARROW_FORMS = {"dreg4_d1": (1, 7), "dreg4_d4": (4, 7), "dreg16_d5": (5, 7), "dreg16_d16": (16, 7),
                "dreg16_d16_k513": (16, 513)}
# Wide: one per branch of launch_wide_any, in one LDS tile and in more than one (tiles in the comment).
WIDE_FORMS = {
    "kg4_d17_k3": (17, 3),            # KG 4, one tile
    "kg4_d24_k1": (24, 1),            # KG 4, k = 1: lb = +inf
    "kg8_d40_k7": (40, 7),            # KG 8 (k <= 8), one tile
    "kg8w_d520_k9": (520, 9),         # KG 8 (512 < dpad <= 1024), tiles of 8 and 1
    "kg32_d24_k33": (24, 33),         # KG 32, one tile of 64
    "kg32_d256_k33": (256, 33),       # KG 32, tiles of 32 and 1
    "kg16_d17_k9": (17, 9),           # KG 16, one tile
    "kg16_d264_k17": (264, 17),       # KG 16, tiles of 16 and 1
    "kg1_d1032_k5": (1032, 5),        # KG 1, one tile
    "kg1_d1032_k9": (1032, 9),        # KG 1, tiles of 7 and 2
}
ASSIGN_FORMS = {**NARROW_FORMS, **WIDE_FORMS}
ASSIGN_N = (1, 255, 257)
# the loads: d % 8 != 0 (a partial last chunk), a column slice (unaligned base, pitch != d), a padded pitch
# (vector loads with a partial last chunk); a contiguous d = 17 f32 matrix has an odd pitch by itself
LAYOUT_FORMS = ("kg4_d17_k3", "kg8_d40_k7", "kg16_d264_k17", "dreg16_d5")
LAYOUTS = ("contig", "slice", "padded")
BIG_IDX = dict(n=1_048_576 + 300, d=17, k=3)   # idx mode: 4096 blocks of 256 rows, then a second pass


def lattice_centres(rng, d, k, dup):
    """Integer centres, distinct in the first coordinate; ``dup``: the last centre repeats centre 0 (it
    must lose to the lower index) and, from k = 4, centre k // 2 repeats centre 1."""
    C = rng.integers(-8, 8, size=(k, d)).astype(F64)
    C[:, 0] = rng.permutation(k) - k // 2
    if dup and k > 1:
        C[k - 1] = C[0]
        if k >= 4:
            C[k // 2] = C[1]
    return C


def lattice_rows(rng, C, n):
    """Row 0 sits on the last centre; then a third of the rows sit on centres (every tile and group),
    a third on the midpoint of a centre and its nearest neighbour (bisectors), the rest are random integers."""
    k, d = C.shape
    X = rng.integers(-8, 8, size=(n, d)).astype(F64)
    X[:, 0] = rng.integers(-(k // 2) - 1, k - k // 2 + 1, size=n)
    on = np.arange(0, n, 3)
    X[on] = C[(k - 1 - np.arange(on.size) * max(1, k // 7)) % k]
    mid = np.arange(1, n, 3)
    a = (k - 1 - np.arange(mid.size) * 5) % k
    G = ((C[:, None, :] - C[None]) ** 2).sum(axis=2)
    G[np.arange(k), np.arange(k)] = np.inf
    X[mid] = (C[a] + C[np.argmin(G, axis=1)[a]]) / 2.0     # between a centre and its nearest neighbour
    return X


@functools.lru_cache(maxsize=None)
def assign_lattice_case(form, n, dup):
    d, k = ASSIGN_FORMS[form]
    rng = np.random.default_rng(_seed(f"{form}/{n}/{dup}"))
    C = lattice_centres(rng, d, k, dup)
    X = lattice_rows(rng, C, n)
    lab, bd, sd = E.assign_lattice(X, C)
    return dict(X=X, C=C, lab=lab, bd=bd, sd=sd, n=n, d=d, k=k)


def fraction_rows(n, d, k, budget=60_000):
    """The rows that go through Fractions: the first, the last, both sides of the block edge and a few
    between, as many as ``budget`` fold terms allow (at least 2)."""
    m = max(2, min(16, budget // (k * d)))
    rows = [0, n - 1, min(255, n - 1), min(256, n - 1)]
    rows += [r for r in np.linspace(0, n - 1, 16).astype(int).tolist() if r not in rows]
    return np.array(sorted(set(rows[:m])), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def assign_generic_case(form, f64, n=257):
    """Random rows and centres; ``sub`` = the rows decided by the Fraction fold (``lab``, ``bd``, ``sd``
    are indexed like it)."""
    d, k = ASSIGN_FORMS[form]
    rng = np.random.default_rng(_seed(f"{form}/generic/{f64}"))
    X = rng.standard_normal((n, d)) * 50.0
    if not f64:
        X = X.astype(F32).astype(F64)
    C = rng.standard_normal((k, d)) * 50.0
    sub = fraction_rows(n, d, k)
    lab, bd, sd = E.assign_fold(X, C, sub)
    return dict(X=X, C=C, sub=sub, lab=lab, bd=bd, sd=sd, n=n, d=d, k=k)


def host_twin_assign(X, C):
    """K.assign_reference on CPU tensors: cml_exact_assign_host (f32 rows widened to f64)."""
    lab, best = K.assign_reference(torch.as_tensor(np.ascontiguousarray(X, dtype=F64)), torch.as_tensor(np.ascontiguousarray(C)))
    return lab.numpy(), best.numpy()


def host_twin_sums(X, L, k):
    S, cnt, S_lo = K.sums_reference(torch.as_tensor(np.ascontiguousarray(X, dtype=F64)), torch.as_tensor(np.asarray(L, dtype=np.int64)),
                                    k, with_lo=True)
    return S.numpy(), cnt.numpy(), S_lo.numpy()


def place(X, f64, device, layout="contig"):
    """The rows on the device in the given layout; the elements around a view hold 1e6, so a read outside
    the row shows in the distance."""
    t = torch.as_tensor(np.ascontiguousarray(X)).to(torch.float64 if f64 else torch.float32)
    n, d = t.shape
    if layout == "contig":
        return t.to(device).contiguous()
    width = d + 3 if layout == "slice" else (d + 7) // 8 * 8 + 8
    off = 1 if layout == "slice" else 0
    wide = torch.full((n, width), 1e6, dtype=t.dtype)
    wide[:, off:off + d] = t
    v = wide.to(device)[:, off:off + d]
    assert v.stride(0) == width and v.stride(1) == 1
    return v


def other_labels(lab, k, every=3):
    """Pre-filled labels: the oracle's, with every third one moved to another centre (k > 1)."""
    lab0 = np.asarray(lab, dtype=np.int64).copy()
    if k > 1:
        lab0[::every] = (lab0[::every] + 1) % k
    return lab0


def run_assign(device, X, C, f64, layout="contig", lab0=None, lst=None, top2=False):
    """exact_assign (or exact_top2) on every row, or on the rows ``lst`` (idx / n_dev mode: the list has
    the capacity n, the count sits on the device).  Labels start from ``lab0``, best from -1, ub / lb
    from -7, the move log from FILL.  Returns numpy outputs."""
    x = place(X, f64, device, layout)
    n = x.shape[0]
    c = dev(C, device)
    lab = dev(np.zeros(n) if lab0 is None else lab0, device, torch.int32)
    best = torch.full((n,), -1.0, dtype=torch.float64, device=device)
    idx = n_dev = None
    if lst is not None:
        full = np.zeros(n, dtype=np.int32)
        full[:len(lst)] = lst
        idx, n_dev = dev(full, device), dev(np.array([len(lst)], dtype=np.int32), device)
    out = {}
    if top2:
        ub = torch.full((n,), -7.0, dtype=torch.float32, device=device)
        lb = torch.full((n,), -7.0, dtype=torch.float32, device=device)
        mv = tuple(torch.full((n,), FILL, dtype=torch.int32, device=device) for _ in range(3)) + \
            (torch.zeros(1, dtype=torch.int32, device=device),)
        K.exact_top2(x, c, lab, ub, lb, idx=idx, n_dev=n_dev, best=best, moves=mv)
        out.update(ub=host(ub), lb=host(lb), mv=tuple(host(m) for m in mv))
    else:
        changed = torch.zeros(1, dtype=torch.int32, device=device)
        K.exact_assign(x, c, labels=lab, changed=changed, idx=idx, n_dev=n_dev, best=best)
        out.update(changed=int(host(changed)[0]))
    out.update(labels=host(lab), best=host(best))
    return out


@functools.lru_cache(maxsize=None)
def big_idx_case():
    """Lattice f32 rows for the idx mode's second grid-stride pass, with a permuted full list."""
    n, d, k = BIG_IDX["n"], BIG_IDX["d"], BIG_IDX["k"]
    rng = np.random.default_rng(_seed("big_idx"))
    C = lattice_centres(rng, d, k, dup=True)
    X = rng.integers(-8, 8, size=(n, d)).astype(F32)
    X[:, 0] = rng.integers(-2, 3, size=n)
    X[::1000] = C[2]                                # on the duplicate of centre 0
    X[1::1000] = (C[0] + C[1]) / 2.0                # on a bisector
    lab, bd, sd = E.assign_lattice(X, C, chunk=1 << 17)
    return dict(X=X, C=C, lab=lab, bd=bd, sd=sd, lst=rng.permutation(n).astype(np.int32), n=n, d=d, k=k)


# ---------------------------------------------------------------------------------------------- exact_dist

# d: 16 and 48 pipelined (without / with a prefetch), 40 chunks of 16, 16, 8, 37 (f32: unaligned), 130;
# k: 256 centres fill the 32 KiB of LDS, 257 are read from global memory
DIST_D = (16, 48, 40, 37, 130)
DIST_K = (3, 256, 257)
DIST_N = (1, 257, 600)


@functools.lru_cache(maxsize=None)
def dist_case(d, k, n, f64, lattice):
    rng = np.random.default_rng(_seed(f"dist/{d}/{k}/{n}/{f64}/{lattice}"))
    if lattice:
        C = lattice_centres(rng, d, k, dup=False)
        X = lattice_rows(rng, C, n)
    else:
        X, C = rng.standard_normal((n, d)) * 50.0, rng.standard_normal((k, d)) * 50.0
        if not f64:
            X = X.astype(F32).astype(F64)
    lab = rng.integers(0, k, size=n)
    lab[:min(n, 2)] = (k - 1, 0)[:min(n, 2)]
    if lattice:
        want = ((X - C[lab]) ** 2).sum(axis=1)
        sub = np.arange(n)
    else:
        sub = np.unique(np.concatenate([np.arange(0, n, 5), [n - 1, min(255, n - 1), min(256, n - 1)]]))
        want = np.array([E.fma_fold(X[r], C[lab[r]]) for r in sub])
    return dict(X=X, C=C, lab=lab, sub=sub, want=want)


def run_dist(device, c, f64, lab_off):
    """The centres are passed as the slice the offset implies: rows lab_off .. of a taller matrix."""
    x = place(c["X"], f64, device)
    tall = np.concatenate([np.full((lab_off, c["C"].shape[1]), 1e6), c["C"]])
    best = torch.full((x.shape[0],), -1.0, dtype=torch.float64, device=device)
    K.exact_dist(x, dev(tall, device)[lab_off:], dev(c["lab"] + lab_off, device, torch.int32), best, lab_off=lab_off)
    return host(best)


# ---------------------------------------------------------------------------------------------- bf16 copies

ERR_SHAPES = ((1, 8), (63, 64), (65, 256), (130, 256))
ERR_BIG = (32_768 + 5, 3, 8)            # the grid is capped at 8192 blocks of 4 rows: a second pass
SPLIT_SHAPES = ((1, 8, 24), (128, 128, 384), (130, 136, 512), (170, 176, 640))
SPLIT_BIG = (131_072 + 3, 8, 8, 24)     # 8192 blocks of 16 rows: a second round with dead lanes


@functools.lru_cache(maxsize=None)
def rows_case(n, d, f64, kind="generic"):
    """Rows for the bf16 copies: random values over a few decades; row 1 (if any) holds bf16 values
    (x = hi exactly), row 2 zeros, row 3 values with a 16-bit significand (x = hi + lo exactly), row 4 of
    f64 rows two values that tell the rounding through f32 from one rounding."""
    rng = np.random.default_rng(_seed(f"rows/{n}/{d}/{f64}/{kind}"))
    X = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-2, 3, size=(n, 1))
    if not f64:
        X = X.astype(F32).astype(F64)
    if n > 1:
        X[1] = rng.integers(-127, 128, size=d)
    if n > 2:
        X[2] = 0.0
    if n > 3:
        X[3] = rng.integers(-32767, 32768, size=d) / 256.0
    if n > 4 and f64:
        # f32(x) falls on a bf16 tie that x itself is above: through f32 the tie goes to even (down), one
        # rounding from f64 goes up — in hi (first value) and in lo (second value)
        X[4, 0] = 1.0 + 2.0 ** -8 + 2.0 ** -40
        X[4, min(1, d - 1)] = 1.0 + 2.0 ** -10 + 2.0 ** -18 + 2.0 ** -50 if d > 1 else X[4, 0]
    return X


def run_bf16_err(device, X, f64, d, ldo):
    """The C entry point, so that ``out`` starts as 0xFFFF everywhere (the wrapper allocates its own)."""
    x = place(X, f64, device)
    n = x.shape[0]
    out = torch.full((n, ldo), -1, dtype=torch.int16, device=device)
    err = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    _native.check(_native.kernels().cml_kmeans_to_bf16_err(x.data_ptr(), int(f64), n, x.stride(0), d, out.data_ptr(), ldo,
                                                           err.data_ptr(), _native.stream_ptr(None)), "to_bf16_err")
    return host(out).view(np.uint16), host(err)


def run_bf16_split(device, X, f64, d, ds, ldo):
    x = place(X, f64, device)
    n = x.shape[0]
    out = torch.full((n, ldo), -1, dtype=torch.int16, device=device)
    ea, eb, en, xn = (torch.full((n,), float("nan"), dtype=torch.float32, device=device) for _ in range(4))
    _native.check(_native.kernels().cml_kmeans_to_bf16_split(
        x.data_ptr(), int(f64), n, x.stride(0), d, ds, out.data_ptr(), ldo, ea.data_ptr(), eb.data_ptr(), en.data_ptr(),
        xn.data_ptr(), _native.stream_ptr(None)), "to_bf16_split")
    return host(out).view(np.uint16), host(ea), host(eb), host(en), host(xn)


def torch_bf16_bits(X, f64):
    """torch's own rounding on the CPU, through f32: f64 -> f32 -> bf16."""
    t = torch.as_tensor(np.ascontiguousarray(X)).to(torch.float64 if f64 else torch.float32)
    return t.to(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def torch_split_layout(X, f64, d, ds, ldo):
    t = torch.as_tensor(np.ascontiguousarray(X)).to(torch.float64)
    hi = t.to(torch.float32).to(torch.bfloat16)
    lo = (t - hi.to(torch.float64)).to(torch.float32).to(torch.bfloat16)
    out = torch.zeros((t.shape[0], ldo), dtype=torch.bfloat16)
    out[:, :d], out[:, ds:ds + d], out[:, 2 * ds:2 * ds + d] = hi, lo, hi
    return out.view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------- screen_cert

ECMAX = 0.75
STEP = 2.0 ** -8          # rows above the line clear it by this much: >= GAP * 2 e, since 2 e < 6
# name -> (n, pattern)
CERT_CASES = {
    "n1_on_line": (1, "line"), "n1_above": (1, "none"), "n1023": (1023, "mixed"), "n1025": (1025, "mixed"),
    "all": (1025, "all"), "none": (1025, "none"), "one_per_wave": (1025, "wave"),
    "second_pass": (2048 * 1024 + 5, "mixed"),       # the grid is capped at 2048 blocks of 1024 rows
}


@functools.lru_cache(maxsize=None)
def cert_case(name):
    """Dyadic ub, err, ecmax; lb on the line lb - ub = 2 (err + ecmax) (listed: the test is a strict >),
    STEP above it (certified) or STEP below it (listed)."""
    n, pattern = CERT_CASES[name]
    rng = np.random.default_rng(_seed("screen_cert/" + name))
    ub = (rng.integers(8 * 256, 64 * 256, size=n) / 256.0).astype(F32)
    err = (rng.integers(0, 2 * 256, size=n) / 256.0).astype(F32)
    err[::5] = 0.0
    kind = {"line": np.zeros(n, int), "none": np.ones(n, int), "all": rng.integers(0, 2, size=n) * 2,
            "mixed": rng.integers(0, 3, size=n)}.get(pattern)
    if kind is None:                                     # one listed row per wave, at a moving lane
        kind = np.ones(n, int)
        w = np.arange(0, n, 64)
        kind[np.minimum(w + (w // 64 * 7) % 64, n - 1)] = 0
    line = ub.astype(F64) + 2.0 * (err.astype(F64) + ECMAX)
    lb = (line + STEP * np.array([0.0, 1.0, -1.0])[kind]).astype(F32)
    return dict(ub=ub, lb=lb, err=err, ecmax=ECMAX, n=n, kind=kind)


def run_screen_cert(device, c, outs="separate"):
    """``outs``: "separate" bound outputs, "aliased" (u_out is ub, l_out is lb) or "none"."""
    n = c["n"]
    ub, lb, err = (dev(c[m], device) for m in ("ub", "lb", "err"))
    ec = dev(np.array([c["ecmax"]]), device)
    lst = torch.full((n,), FILL, dtype=torch.int32, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    u = l = None
    if outs == "separate":
        u = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
        l = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    elif outs == "aliased":
        u, l = ub, lb
    K.screen_cert(ub, lb, err, ec, n, lst, count, u_out=u, l_out=l)
    if outs != "aliased":   # the inputs are untouched
        assert np.array_equal(host(ub), c["ub"]) and np.array_equal(host(lb), c["lb"])
    return host(lst), int(host(count)[0]), (host(u) if u is not None else None), (host(l) if l is not None else None)


CST = (0.5, 2.0, 0.25)
# name -> (n, pattern)
SPLIT_CERT_CASES = {
    "n1": (1, "mixed"), "n255": (255, "mixed"), "n257": (257, "mixed"), "none": (1000, "none"),
    "all_n4100": (4100, "all"),
    "flush": (7 * 2048 * 256 + 300, "all"),   # the first blocks gather 8 x 256 entries: a flush in mid-loop
    "second_pass": (2048 * 256 + 7, "mixed"),
}


@functools.lru_cache(maxsize=None)
def split_cert_case(name):
    """Random f32 bounds and slacks; the code's e is 0, well below lb² or well above it (|lb² - e| >=
    1e-2 lb²: the premise of W_LIST), shared among ea, eb and en."""
    n, pattern = SPLIT_CERT_CASES[name]
    rng = np.random.default_rng(_seed("screen_cert_split/" + name))
    lb = (1.0 + 9.0 * rng.random(n)).astype(F32)
    ub = (lb * (0.05 + rng.random(n))).astype(F32)
    f = np.where(rng.random(n) < 0.5, 0.01 + 0.89 * rng.random(n), 1.1 + 2.0 * rng.random(n))
    f[::7] = 0.0
    if pattern == "none":
        ub, f = (lb * F32(0.25)).astype(F32), 0.2 * rng.random(n)
    elif pattern == "all":
        f = 1.1 + 2.0 * rng.random(n)
    e_t = f * lb.astype(F64) ** 2 / (1.0 + 1e-6)
    share = rng.dirichlet((1.0, 1.0, 1.0), size=n)
    ea = (share[:, 0] * e_t / (2.0 * CST[0])).astype(F32)
    eb = (share[:, 1] * e_t / (2.0 * CST[1])).astype(F32)
    en = (share[:, 2] * e_t / (2.0 * 1.01 * CST[2])).astype(F32)
    return dict(ub=ub, lb=lb, ea=ea, eb=eb, en=en, cst=np.array(CST), n=n)


def run_screen_cert_split(device, c):
    n = c["n"]
    t = {m: dev(c[m], device) for m in ("ub", "lb", "ea", "eb", "en", "cst")}
    lst = torch.full((n,), FILL, dtype=torch.int32, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    u = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    l = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    K.screen_cert_split(t["ub"], t["lb"], t["ea"], t["eb"], t["en"], t["cst"], n, lst, count, u, l)
    return host(lst), int(host(count)[0]), host(u), host(l)


# ---------------------------------------------------------------------------------------------- sums

# name -> cluster sizes in label order (n = 3073 = three chunks of 1024 positions and one more row)
SUMS_LAYOUTS = {
    "ends_on_edges": [1024, 1024, 500, 525, 0],                  # clusters end exactly at 1024 and at 2048
    "spans_three_chunks": [100, 2500, 473],
    "forty_in_one_chunk": [100] + [20] * 40 + [1000, 1173],
    "empties": [0, 0, 1000, 0, 0, 1500, 573, 0, 0],              # empty first, in the middle and last
}
SUMS_D = (1, 65, 257)     # 65: a 128-thread block; 257: two column blocks
SUMS_SMALL = {"single_row": ([0, 0, 1, 0], 3), "single_cluster": ([2500], 5)}


def _labels(rng, sizes):
    lab = np.repeat(np.arange(len(sizes)), sizes)
    return lab[rng.permutation(lab.size)]


@functools.lru_cache(maxsize=None)
def sums_case(name, d=None):
    """Exactly summable rows (dyadic, f32-exact) under the named label layout."""
    sizes, d = (SUMS_LAYOUTS[name], d) if name in SUMS_LAYOUTS else SUMS_SMALL[name]
    rng = np.random.default_rng(_seed(f"sums/{name}/{d}"))
    L = _labels(rng, sizes)
    return dict(X=dyadic(rng, (L.size, d)), L=L, k=len(sizes), exact=True)


@functools.lru_cache(maxsize=None)
def sums_cancel_case():
    """Cluster 0: large +- pairs (m 2^40, m < 2^20) and small remainders (j 2^-10); cluster 1: pairs
    only, its sum is exactly 0; cluster 2: dyadic rows.  Top to bottom the values span 2^70, so hi + lo
    holds every partial sum exactly, in any order."""
    rng = np.random.default_rng(_seed("sums/cancel"))
    d, pairs = 2, 700
    big = rng.integers(1, 2 ** 20, size=(pairs, d)).astype(F64) * 2.0 ** 40
    small = rng.integers(-1023, 1024, size=(300, d)).astype(F64) * 2.0 ** -10
    z = rng.integers(1, 2 ** 20, size=(400, d)).astype(F64) * 2.0 ** 30
    X = np.concatenate([big, -big, small, z, -z, dyadic(rng, (473, d))])
    L = np.concatenate([np.zeros(2 * pairs + 300, int), np.ones(800, int), np.full(473, 2)])
    p = rng.permutation(L.size)
    return dict(X=X[p], L=L[p], k=3, exact=True)


@functools.lru_cache(maxsize=None)
def sums_generic_case():
    rng = np.random.default_rng(_seed("sums/generic"))
    L = _labels(rng, [1024, 1500, 0, 549])
    return dict(X=rng.standard_normal((L.size, 3)) * 1e3, L=L, k=4, exact=False)


def run_sums(device, c, f64):
    x = place(c["X"], f64, device)
    S, cnt, S_lo = K.exact_sums(x, dev(c["L"], device, torch.int32), c["k"], with_lo=True, counts_int=True)
    return host(S), host(S_lo), host(cnt)


SUM_N = (1, 4097, 4_194_304 + 4097)   # 1024 blocks of 4096 values, then the cap: longer ranges per block


@functools.lru_cache(maxsize=None)
def sum_case(n):
    """Spread exponents (2^-20 .. 2^20 times a 20-bit integer: 2^60 top to bottom, well inside 2^80) in
    cancelling pairs, with a small remainder."""
    rng = np.random.default_rng(_seed(f"sum/{n}"))
    v = rng.integers(1, 2 ** 20, size=n).astype(F64) * 2.0 ** rng.integers(-20, 21, size=n)
    h = n // 2
    v[1:2 * h:2] = -v[0:2 * h:2]
    v[n // 2] += 3.0 * 2.0 ** -20
    return v
