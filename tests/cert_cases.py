"""Named, seeded cases for the kernels of ``_native/csrc/kmeans_cert.hip`` and the runners that put
them through the wrappers of ``ops/kmeans_ops.py``, shared by ``test_cert_oracle.py`` (the oracle and
the checkers, any machine) and ``test_kmeans_cert_kernels_gpu.py`` (the kernels).  Builders return
plain numpy; every case is built once per process and never modified.

Data is dyadic (multiples of 2^-8 below 2^10, see ``cert_oracle.is_dyadic``) wherever plain f64 is
then exact; one case per kernel holds unrestricted random f64 values and goes through Fractions.
"""
import functools

import numpy as np
import torch

import cert_oracle as O
from clustermachinelearningforhospitalnetworks_apache_spark_amd.ops import kmeans_ops as K

F32, F64 = np.float32, np.float64


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def dyadic(rng, shape, span=64):
    """Random multiples of 2^-8 in [-span, span)."""
    return rng.integers(-span * 256, span * 256, size=shape).astype(F64) / 256.0


def dev(a, device, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device).contiguous()


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- cert_stats

STATS_GRID = {f"k{k}_d{d}": (k, d) for k in (1, 2, 3, 255, 256, 257, 600) for d in (1, 7, 130)}
# name -> (k, d, (index of the largest drift, index of the second largest) or a keyword)
STATS_SPECIAL = {
    "top_at_0": (257, 7, (0, 200)),
    "top_ge_256": (600, 7, (515, 3)),
    "same_stride": (600, 1, (40, 296)),        # both in thread 40's stride, the largest first
    "same_stride_rev": (600, 7, (296, 40)),    # ... the largest second
    "same_stride_3rd": (600, 7, (552, 296)),   # third and second visit of one thread
    "tie": (300, 7, "tie"),
    "tie_same_stride": (600, 1, "tie_stride"),
    "all_zero_k257": (257, 7, "zero"),
    "all_zero_k1": (1, 7, "zero"),
    "random_f64": (3, 7, "random"),
}
STATS_CASES = list(STATS_GRID) + list(STATS_SPECIAL)


@functools.lru_cache(maxsize=None)
def stats_case(name):
    rng = np.random.default_rng(_seed(name))
    if name in STATS_GRID:
        k, d = STATS_GRID[name]
        C = dyadic(rng, (k, d))
        if k >= 3:
            C[2] = C[0]                       # duplicate centres: half-separation exactly 0
        Cold = C + dyadic(rng, (k, d), span=2)
        Cold[::3] = C[::3]                    # unmoved centres: drift exactly 0
        if k > 1:
            Cold[k - 1] = C[k - 1] + 1.0
        return dict(C=C, Cold=Cold, top=None)
    k, d, how = STATS_SPECIAL[name]
    if how == "random":
        C = rng.standard_normal((k, d)) * 1e3
        return dict(C=C, Cold=C + rng.standard_normal((k, d)), top=None)
    C = dyadic(rng, (k, d))
    if how == "zero":
        return dict(C=C, Cold=C.copy(), top=None)
    Cold = C + dyadic(rng, (k, d), span=1)    # |offset| < 1 per coordinate: drift < sqrt(d) <= 2.7
    if how in ("tie", "tie_stride"):
        i, j = (299, 50) if how == "tie" else (40, 296)
        Cold[i], Cold[j] = C[i], C[j]
        Cold[i, 0] += 90.0
        Cold[j, 0] -= 90.0                    # the same drift, bit for bit
        return dict(C=C, Cold=Cold, top=(i, j), tie=True)
    i, j = how
    Cold[i], Cold[j] = C[i], C[j]
    Cold[i, 0] += 100.0
    Cold[j, d - 1] -= 99.0
    return dict(C=C, Cold=Cold, top=(i, j))


def run_stats(device, c, with_zero=True):
    C, Cold = dev(c["C"], device), dev(c["Cold"], device)
    k = C.shape[0]
    s = torch.full((k,), -7.0, dtype=torch.float32, device=device)
    drift = torch.full((k,), -7.0, dtype=torch.float32, device=device)
    dtop = torch.full((4,), -7.0, dtype=torch.float32, device=device)
    zero = torch.full((4 + 2 * k,), 9, dtype=torch.int32, device=device) if with_zero else None
    K.cert_stats(C, Cold, s, drift, dtop, zero=zero)
    return host(s), host(drift), host(dtop), (host(zero) if with_zero else None)


# ---------------------------------------------------------------------------------------------- cert_bounds

BOUNDS_K = 7
I_TOP, I_INF, I_EQ = 2, 5, 6     # the top-drift centre, the centre with s = +inf, the equality centre
# name -> (n, mode)
BOUNDS_CASES = {
    "n1": (1, "mixed"), "n255": (255, "mixed"), "n256": (256, "mixed"), "n257": (257, "mixed"),
    "n262145": (262_145, "mixed"),            # the grid is capped at 1024 x 256 rows: a second iteration
    "none_listed": (1000, "none"), "all_listed": (1000, "all"),
    "flush": (2_100_000, "all"),              # 9 iterations of 256 listed rows per block: a flush at 2048
}


@functools.lru_cache(maxsize=None)
def bounds_case(name):
    n, mode = BOUNDS_CASES[name]
    rng = np.random.default_rng(_seed(name))
    k = BOUNDS_K
    drift = (rng.random(k) * 0.5).astype(F32)
    drift[I_TOP] = F32(0.75)
    drift[3] = F32(0.625)                     # the second largest
    dtop = np.array([drift[I_TOP], drift[3], I_TOP, 0], dtype=F32)
    s = (rng.random(k) * 2.0).astype(F32)
    lab = rng.integers(0, k, size=n).astype(np.int32)
    u = (rng.random(n) * 4.0).astype(F32)
    l = (rng.random(n) * 6.0).astype(F32)
    if mode == "none":
        lab[lab == I_EQ] = 0
        u = (rng.random(n) * 0.5).astype(F32)
        l = (4.0 + rng.random(n)).astype(F32)
    elif mode == "all":
        u = (5.0 + rng.random(n)).astype(F32)
        l = (rng.random(n) * 2.0).astype(F32)  # around the top drifts: some go negative and clamp to 0
    else:
        s[I_INF] = np.inf
        eq = lab == I_EQ                       # u' == max(l', s) exactly: listed (the test is a strict <)
        u[eq], l[eq] = F32(3.25), F32(0.0)
        s[I_EQ] = O.f32_up(np.float64(F32(3.25)) + np.float64(drift[I_EQ]))
        l[::11] = F32(0.25)                    # goes negative: clamps to 0
        u[::13] = np.inf
        u[5::17] = np.nan
    return dict(n=n, k=k, lab=lab, u=u, l=l, drift=drift, dtop=dtop, s=s)


def run_bounds(device, c):
    n = c["n"]
    lab, u, l = dev(c["lab"], device), dev(c["u"], device), dev(c["l"], device)
    lst = torch.full((n,), -1, dtype=torch.int32, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    K.cert_bounds(lab, u, l, dev(c["drift"], device), dev(c["dtop"], device), dev(c["s"], device), n, lst, count)
    return host(u), host(l), host(lst), int(count.item())


# ---------------------------------------------------------------------------------------------- cert_tighten

# name -> dict(d, f64 rows, n, na, and flags)
TIGHTEN_CASES = {f"d{d}_{'f64' if f else 'f32'}": dict(d=d, f64=f, n=200, na=150)
                 for d in (1, 15, 16, 17, 127, 128, 129, 300) for f in (False, True)}
TIGHTEN_CASES.update({
    "na0": dict(d=15, f64=False, n=40, na=0),
    "na1": dict(d=15, f64=True, n=40, na=1),
    "na17": dict(d=15, f64=False, n=40, na=17, ext=True),
    "na16385": dict(d=3, f64=True, n=16_400, na=16_385, ext=True),   # 1024 blocks x 16 rows: a second iteration
    "flush": dict(d=1, f64=False, n=1_900_000, na=1_900_000, unproven=True),  # 1855 rows per block > kBuf - 256
    "strided": dict(d=17, f64=True, n=200, na=150, strided=True, ext=True),
    "random_f64": dict(d=7, f64=True, n=64, na=17, random=True),
})


@functools.lru_cache(maxsize=None)
def tighten_case(name):
    p = TIGHTEN_CASES[name]
    d, n, na = p["d"], p["n"], p["na"]
    rng = np.random.default_rng(_seed(name))
    k = 3
    lab = rng.integers(0, k, size=n).astype(np.int32)
    if p.get("random"):
        C = rng.standard_normal((k, d)) * 3.0
        X = rng.standard_normal((n, d)) * 3.0
        exact_root = np.zeros(n, dtype=bool)
    else:
        C = dyadic(rng, (k, d), span=8)
        X = dyadic(rng, (n, d), span=8)
        X[::5] = C[lab[::5]]                                  # the row is its centre: u exactly 0
        m = rng.integers(1, 20, size=n).astype(F64)
        X[1::5] = C[lab[1::5]]
        X[1::5, 0] += m[1::5]                                 # distance exactly m: the square root is exact
        exact_root = np.zeros(n, dtype=bool)
        exact_root[::5] = exact_root[1::5] = True
        if d == 1:
            exact_root[:] = True
    la = np.zeros(n, dtype=np.int32)
    la[:na] = rng.permutation(n)[:na].astype(np.int32)
    u = (rng.random(n) * 50.0).astype(F32)
    l = (rng.random(n) * 50.0).astype(F32)
    s = np.zeros(k, dtype=F32)
    if not p.get("unproven"):
        s[2] = F32(2048.0)                                    # proves every row of centre 2 on its own
    rows = la[:na].astype(np.int64)
    _, u_or, _, _ = O.tighten_oracle(X, C, lab, l, s, rows)
    kind = np.arange(na) % 3                                  # 0: equal (listed), 1: proven, 2: listed
    if p.get("unproven"):
        kind = np.where(kind == 1, 2, kind)
    kind = np.where((kind == 0) & ~exact_root[rows], 2, kind)
    t = np.where(kind == 0, u_or, np.where(kind == 1, u_or * F32(1 + 2.0 ** -19), u_or * F32(1 - 2.0 ** -19)))
    t = np.where((u_or == 0) & (kind == 1), F32(2.0 ** -10), t).astype(F32)
    l[rows] = t
    xn = (rng.random(n) * 100.0).astype(F32)
    return dict(X=X, C=C, lab=lab, u=u, l=l, s=s, la=la, na=na, n=n, d=d, xn=xn, f64=p["f64"],
                strided=bool(p.get("strided")), ext=bool(p.get("ext")))


def rows_tensor(X, f64, device, strided=False):
    """The rows as an f32 / f64 device tensor; ``strided``: a view with ld = d + 3 and NaN in the padding."""
    dt = torch.float64 if f64 else torch.float32
    x = dev(X, device, dt)
    if not strided:
        return x
    n, d = x.shape
    base = torch.full((n, d + 3), float("nan"), dtype=dt, device=device)
    base[:, :d] = x
    view = base[:, :d]
    assert view.stride(0) == d + 3
    return view


def run_tighten(device, c):
    n = c["n"]
    x = rows_tensor(c["X"], c["f64"], device, c["strided"])
    u = dev(c["u"], device)
    lab = dev(c["lab"], device)
    lbst = torch.full((n,), -1, dtype=torch.int32, device=device)
    ctr = torch.zeros(2, dtype=torch.int32, device=device)
    ctr[0] = c["na"]
    ext = {}
    if c["ext"]:
        ext = dict(xn=dev(c["xn"], device), bxn=torch.full((n,), -1.0, dtype=torch.float32, device=device),
                   blab=torch.full((n,), -1, dtype=torch.int32, device=device))
    K.cert_tighten(x, dev(c["C"], device), lab, u, dev(c["l"], device), dev(c["s"], device), dev(c["la"], device),
                   ctr[0:1], lbst, ctr[1:2], **ext)
    return (host(u), host(lbst), int(ctr[1].item()), host(ext["bxn"]) if ext else None,
            host(ext["blab"]) if ext else None)


# ---------------------------------------------------------------------------------------------- split_centres

SPLIT_CASES = {f"k{k}_kp{kp}_d{d}_ds{ds}_{'wide' if wide else 'tight'}": (k, kp, d, ds, wide)
               for k, kp in ((1, 32), (3, 32), (40, 64), (64, 64), (300, 320))
               for d, ds in ((5, 8), (128, 128), (170, 176)) for wide in (False, True)}
SPLIT_CASES["random_f64"] = (3, 32, 5, 8, True)


@functools.lru_cache(maxsize=None)
def split_case(name):
    k, kp, d, ds, wide = SPLIT_CASES[name]
    rng = np.random.default_rng(_seed(name))
    C = rng.standard_normal((k, d)) * 1e3 if name == "random_f64" else dyadic(rng, (k, d), span=1024)
    return dict(C=C, k=k, kp=kp, d=d, ds=ds, ldc=3 * ds + (40 if wide else 0))


def run_split(device, c):
    kp, ldc = c["kp"], c["ldc"]
    cb = torch.full((kp, ldc), 1.5, dtype=torch.bfloat16, device=device)
    cn = torch.full((kp,), -1.0, dtype=torch.float32, device=device)
    cst = torch.full((3,), -1.0, dtype=torch.float64, device=device)
    mc = torch.full((1,), -1.0, dtype=torch.float32, device=device)
    K.split_centres_dev(dev(c["C"], device), c["ds"], cb, cn, cst, mc=mc)
    return host(cb.view(torch.int16)).view(np.uint16), host(cn), host(cst), host(mc)


def split_layout_torch(c):
    """The layout by torch's own f64 -> f32 -> bf16 rounding (the oracle of the split row layout's test)."""
    C = torch.as_tensor(c["C"])
    k, d, ds = c["k"], c["d"], c["ds"]
    ch = C.to(torch.float32).to(torch.bfloat16)
    cl = (C - ch.to(torch.float64)).to(torch.float32).to(torch.bfloat16)
    cb = torch.zeros((c["kp"], c["ldc"]), dtype=torch.bfloat16)
    cb[:k, :d], cb[:k, ds:ds + d], cb[:k, 2 * ds:2 * ds + d] = ch, ch, cl
    return cb.view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------- cert_list

LIST_CASES = {"cnt0": 0, "cnt1": 1, "cnt255": 255, "cnt257": 257,
              "cnt131100": 131_100}               # 512 blocks x 256 entries: a second iteration, cap = n
LIST_K, LIST_M0 = 6, 5


@functools.lru_cache(maxsize=None)
def list_case(name):
    cnt = LIST_CASES[name]
    rng = np.random.default_rng(_seed(name))
    n = max(cnt + 13, 64)
    lst = np.zeros(n, dtype=np.int32)
    lst[:cnt] = rng.permutation(n)[:cnt].astype(np.int32)
    rows = lst[:cnt].astype(np.int64)
    blab = rng.integers(0, LIST_K, size=n).astype(np.int32)      # beside the list: the old labels
    lab = rng.integers(0, LIST_K, size=n).astype(np.int32)       # at the rows: the screened labels
    keep = np.arange(cnt) % 2 == 0
    lab[rows[keep]] = blab[:cnt][keep]                            # half of the listed rows did not move
    cst = np.array([1.3 * 2.0 ** -9, 37.7, 0.9 * 2.0 ** -17], dtype=F64)
    ea = (rng.random(n) * 0.1).astype(F32)
    eb = (rng.random(n) * 2.0 ** -16).astype(F32)
    en = (rng.random(n) * 100.0).astype(F32)
    u = (1.0 + rng.random(n) * 9.0).astype(F32)
    l = (rng.random(n) * 9.0).astype(F32)
    kind = (np.arange(cnt) % 5) if cnt > 1 else np.array([2] * cnt, dtype=np.int64)
    z = rows[(kind == 0) | (kind == 1)]
    ea[z] = eb[z] = en[z] = 0                                     # e = 0
    e = 2.0 * (ea.astype(F64) * cst[0] + eb.astype(F64) * cst[1] + 1.01 * en.astype(F64) * cst[2]) * (1 + 1e-6)
    r0, r1, r2, r3, r4 = (rows[kind == i] for i in range(5))
    u[r0], l[r0] = F32(1.0), F32(1.0 + 2.0 ** -22)               # uu == ll == 1 + 2^-23 exactly: uncertified
    l[r1] = (u[r1].astype(F64) * (1 + 2.0 ** -18)).astype(F32)   # certified, 2^-18 apart
    l[r2] = (1.5 * np.sqrt(u[r2].astype(F64) ** 2 + 2 * e[r2])).astype(F32)   # certified
    l[r3] = (0.5 * np.sqrt(e[r3])).astype(F32)                   # l² - e < 0: ll = 0, uncertified
    l[r4] = (u[r4].astype(F64) * (1 - 2.0 ** -10)).astype(F32)   # uncertified
    mv0 = (np.full(LIST_M0, 70_000, np.int32), np.full(LIST_M0, 71, np.int32), np.full(LIST_M0, 72, np.int32),
           LIST_M0)
    return dict(n=n, cnt=cnt, lst=lst, blab=blab, lab=lab, u=u, l=l, ea=ea, eb=eb, en=en, cst=cst, mv0=mv0)


def run_list(device, c):
    n = c["n"]
    lab, u, l = dev(c["lab"], device), dev(c["u"], device), dev(c["l"], device)
    lc = torch.full((n,), -1, dtype=torch.int32, device=device)
    ctr = torch.zeros(3, dtype=torch.int32, device=device)
    ctr[0], ctr[2] = c["cnt"], LIST_M0
    mv = [torch.full((n + LIST_M0,), -1, dtype=torch.int32, device=device) for _ in range(3)]
    for t, a in zip(mv, c["mv0"][:3]):
        t[:LIST_M0] = dev(a, device)
    K.cert_list(dev(c["lst"], device), ctr[0:1], n, dev(c["blab"], device), lab, u, l, dev(c["ea"], device),
                dev(c["eb"], device), dev(c["en"], device), dev(c["cst"], device), lc, ctr[1:2],
                (mv[0], mv[1], mv[2], ctr[2:3]))
    return host(lab), host(u), host(l), host(lc), int(ctr[1].item()), tuple(host(t) for t in mv) + (int(ctr[2].item()),)


# ---------------------------------------------------------------------------------------------- cert_moves

MOVES_CASES = {f"k{k}_d{d}": dict(k=k, d=d, f64=bool((i + j) % 2), how="standard")
               for i, k in enumerate((2, 5, 64, 256)) for j, d in enumerate((1, 63, 64, 65, 130))}
MOVES_CASES.update({
    "no_moves": dict(k=5, d=7, f64=False, how="none"),
    "one_move": dict(k=5, d=7, f64=True, how="one"),
    "all_into_one": dict(k=5, d=7, f64=False, how="into_one"),
    "k2_emptied": dict(k=2, d=3, f64=False, how="empty2"),
    # 131 100 moves: cert_hist (256 blocks x 256) and cert_scatter (512 x 256) iterate twice, and every
    # slice of cert_delta holds more rows than its 4 lanes x 8 loads take at once
    "big": dict(k=5, d=2, f64=True, how="big", n=140_000),
    "strided": dict(k=5, d=17, f64=True, how="standard", strided=True),
    "d300": dict(k=5, d=300, f64=False, how="standard"),   # cert_apply's 256 threads loop over d
    # unrestricted rows over twelve decades: the low parts of the double-double sums are live
    "random_f64": dict(k=5, d=7, f64=True, how="standard", random=True),
    "random_f32": dict(k=5, d=7, f64=False, how="standard", random=True),
    "random_f64_k64": dict(k=64, d=65, f64=True, how="standard", random=True),
})


def _take(pool, j, m):
    """m rows of cluster j from the pool of rows that have not moved yet."""
    rows = pool[j][:m]
    assert len(rows) == m, "the case needs more rows per cluster"
    pool[j] = pool[j][m:]
    return rows


@functools.lru_cache(maxsize=None)
def moves_case(name):
    p = MOVES_CASES[name]
    k, d, how = p["k"], p["d"], p["how"]
    rng = np.random.default_rng(_seed(name))
    n = p.get("n", max(40 * k, 200))
    X = dyadic(rng, (n, d))
    if p.get("random"):
        X = rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-4, 8, size=(n, d))
        if not p["f64"]:
            X = X.astype(F32).astype(F64)
    L0 = rng.integers(0, k, size=n).astype(np.int32)
    L0[:k * 30] = np.repeat(np.arange(k), 30)                    # at least 30 rows in every cluster
    pool = {j: list(np.nonzero(L0 == j)[0]) for j in range(k)}
    mv = []                                                       # (rows, new cluster)
    if how == "standard":
        mv.append((_take(pool, 1, 3), 0))                        # 3 rows into cluster 0: fewer than the slices
        src = 2 if k >= 3 else 0
        mv.append((_take(pool, src, 19), 1))                     # 19 into 1 (which also lost 3): no multiple of 4
        if k >= 5:
            mv.append((_take(pool, 3, len(pool[3])), 4))         # cluster 3 loses every row
        if k >= 64:
            for j in range(5, k - 1, 3):
                mv.append((_take(pool, j, 1 + j % 7), j + 1))
    elif how == "one":
        mv.append((_take(pool, 2, 1), 4))
    elif how == "into_one":
        for j in (0, 1, 2, 4):
            mv.append((_take(pool, j, 11 + j), 3))
    elif how == "empty2":
        mv.append((_take(pool, 1, len(pool[1])), 0))
    elif how == "big":
        rows = np.arange(131_100)
        mv.append((rows, None))
    if mv and mv[0][1] is None:
        rows = mv[0][0].astype(np.int32)
        new = ((L0[rows] + 1) % k).astype(np.int32)
    else:
        rows = np.array([r for rr, _ in mv for r in rr], dtype=np.int32)
        new = np.array([j for rr, j in mv for _ in rr], dtype=np.int32)
    perm = rng.permutation(rows.size)
    rows, new = rows[perm], new[perm]
    old = L0[rows].astype(np.int32)
    assert np.all(old != new) and np.unique(rows).size == rows.size
    C_cur = dyadic(rng, (k, d))
    return dict(X=X, k=k, d=d, n=n, L0=L0, rows=rows, old=old, new=new, C_cur=C_cur, f64=p["f64"],
                f32_rows=not p["f64"], strided=bool(p.get("strided")))


def run_moves(device, c):
    k, d, n = c["k"], c["d"], c["n"]
    x = rows_tensor(c["X"], c["f64"], device, c["strided"])
    L0 = dev(c["L0"], device)
    S_hi, cnt, S_lo = K.exact_sums(x, L0, k, with_lo=True, counts_int=True)
    m = c["rows"].size
    i32 = dict(dtype=torch.int32, device=device)
    mv = [torch.zeros(n, **i32) for _ in range(3)]
    for t, a in zip(mv, (c["rows"], c["old"], c["new"])):
        t[:m] = dev(a, device)
    m_dev = torch.tensor([m], **i32)
    hist = torch.zeros(2 * k, **i32)                               # cert_stats zeroes it in the engine
    seg, cursor, perm = torch.full((2 * k + 1,), -1, **i32), torch.full((2 * k,), -1, **i32), torch.full((2 * n,), -1, **i32)
    ns = K.cert_slices(k)
    assert ns == (4 if k >= 256 else 8 if k >= 64 else 16)
    P_hi = torch.full((ns * k * d,), float("nan"), dtype=torch.float64, device=device)
    P_lo = torch.full((ns * k * d,), float("nan"), dtype=torch.float64, device=device)
    C_cur = dev(c["C_cur"], device)
    C_next = torch.full((k, d), float("nan"), dtype=torch.float64, device=device)
    shift2 = torch.full((k,), float("nan"), dtype=torch.float64, device=device)
    K.cert_moves(x, k, mv[0], mv[1], mv[2], m_dev, hist, seg, cursor, perm, P_hi, P_lo, S_hi, S_lo, cnt,
                 C_cur=C_cur, C_next=C_next, shift2=shift2)
    return dict(S_hi=host(S_hi), S_lo=host(S_lo), cnt=host(cnt), seg=host(seg), perm=host(perm),
                C_next=host(C_next), shift2=host(shift2))


def moves_oracle_output(c):
    """What a correct cert_moves returns, built by the oracle alone (for the checkers' own tests)."""
    k, rows, old, new = c["k"], c["rows"].astype(np.int64), c["old"].astype(np.int64), c["new"].astype(np.int64)
    L1 = O.apply_moves(c["L0"], rows, new)
    S, cnt = O.fsum_clusters(c["X"], L1, k)
    bins = [rows[new == b] if b < k else rows[old == b - k] for b in range(2 * k)]
    seg = np.concatenate([[0], np.cumsum([len(b) for b in bins])])
    perm = np.full(2 * c["n"], -1, dtype=np.int64)
    perm[:seg[-1]] = np.concatenate(bins) if rows.size else []
    with np.errstate(divide="ignore", invalid="ignore"):
        C_next = np.where((cnt > 0)[:, None], S / np.maximum(cnt, 1)[:, None].astype(F64), c["C_cur"])
    shift2 = ((C_next - c["C_cur"]) ** 2).sum(axis=1)
    S_lo = np.zeros_like(S)
    if not O.is_dyadic(c["X"]):   # the remainder of the exact sum, rounded (exact for f32 rows)
        exact, _ = O.exact_cluster_sums(c["X"], L1, k)
        S_lo = np.array([[float(exact[j][t] - O.fr(S[j, t])) for t in range(S.shape[1])] for j in range(k)])
    return dict(S_hi=S, S_lo=S_lo, cnt=cnt, seg=seg, perm=perm, C_next=C_next, shift2=shift2)


# ---------------------------------------------------------------------------------------------- the chained step

CHAIN_CASES = {f"k{k}_d{d}": (k, d) for k in (2, 5, 300) for d in (2, 17)}
ENGINE_CASE = "k5_d65"   # LloydEngine's screen needs a K9r row width (d > 64); its split layout d <= 170
R = 31              # the lattice: every integer point of [-R, R]² in the first two coordinates
GADGET_Y = 1000.0   # the emptying gadget lives far away, on the line y = GADGET_Y


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """Rows on an integer lattice, integer centres with even coordinates: the first assignment meets
    rows exactly on the bisector of two centres (ties go to the lowest index, as K.exact_assign has
    it).  From k = 5 on, a gadget of three centres A < B < E on a far line: B = 10 owns the rows 6 and
    14 and stays their mean, while A = 0 (rows 3, 4, 5; 5 ties with B) moves to 4 and E = 20 (rows 16,
    17, 18) to 17, so both rows leave B at the first certified step: a cluster that empties.
    k = 300 also holds two duplicate centres (k = 5 has no room for them beside the gadget, k = 2 for
    neither)."""
    k, d = (5, 65) if name == ENGINE_CASE else CHAIN_CASES[name]
    rng = np.random.default_rng(_seed(name))
    g = np.arange(-R, R + 1)
    X = np.zeros(((2 * R + 1) ** 2, d))
    X[:, 0], X[:, 1] = np.repeat(g, g.size), np.tile(g, g.size)
    if d > 2:
        X[:, 2:] = rng.integers(-1, 2, size=(X.shape[0], d - 2))
    emptied = dup = None
    if k == 2:
        C = np.zeros((2, d))
        C[0, :2], C[1, :2] = (-30, -30), (-26, -30)   # the 63 rows with x = -28 lie on the bisector
    else:
        nl = k - 3
        even = np.array([(a, b) for a in range(-R + 1, R, 2) for b in range(-R + 1, R, 2)], dtype=F64)
        pick = even[rng.permutation(len(even))[:nl]]
        if k == 5:
            pick = np.array([(-30, -30), (-26, -30)], dtype=F64)
        C = np.zeros((k, d))
        C[:nl, :2] = pick
        if k == 300:
            C[200] = C[10]
            dup = (10, 200)
        ga = np.zeros((3, d))
        ga[:, 0], ga[:, 1] = (0, 10, 20), GADGET_Y
        C[nl:] = ga
        rows = np.zeros((8, d))
        rows[:, 0], rows[:, 1] = (3, 4, 5, 6, 14, 16, 17, 18), GADGET_Y
        X = np.concatenate([X, rows])
        emptied = nl + 1
    return dict(X=X, C0=C, k=k, d=d, n=X.shape[0], emptied=emptied, dup=dup)


def numpy_sqdist(X, C):
    """f64 squared distances [n, k], centre by centre in the plain order (exact on integer data)."""
    return np.stack([((X - c) ** 2).sum(axis=1) for c in C], axis=1)


class Chain:
    """The non-split chain of LloydEngine._step_screen, kernel by kernel."""

    def __init__(self, device, c, f64=True):
        self.c, self.k, self.n, self.d = c, c["k"], c["n"], c["d"]
        k, n, d = self.k, self.n, self.d
        self.x = rows_tensor(c["X"], f64, device)
        i32 = dict(dtype=torch.int32, device=device)
        f32 = dict(dtype=torch.float32, device=device)
        self.lab, self.u, self.l = torch.zeros(n, **i32), torch.empty(n, **f32), torch.empty(n, **f32)
        self.C_cur = dev(c["C0"], device)
        K.exact_top2(self.x, self.C_cur, self.lab, self.u, self.l)
        self.S_hi, self.cnt, self.S_lo = K.exact_sums(self.x, self.lab, k, with_lo=True, counts_int=True)
        self.cbuf = [torch.empty((k, d), dtype=torch.float64, device=device) for _ in range(2)]
        self.C = self.cbuf[0]
        self.C.copy_(torch.where((self.cnt > 0)[:, None], self.S_hi / self.cnt.clamp(min=1).to(torch.float64)[:, None],
                                 self.C_cur))
        self.ctr = torch.zeros(4 + 2 * k, **i32)
        self.la, self.lbl = torch.empty(n, **i32), torch.empty(n, **i32)
        self.mv = [torch.empty(n, **i32) for _ in range(3)]
        self.seg, self.cursor, self.perm = torch.empty(2 * k + 1, **i32), torch.empty(2 * k, **i32), torch.empty(2 * n, **i32)
        self.s, self.drift, self.dtop = torch.empty(k, **f32), torch.empty(k, **f32), torch.zeros(4, **f32)
        ns = K.cert_slices(k)
        self.P_hi = torch.empty(ns * k * d, dtype=torch.float64, device=device)
        self.P_lo = torch.empty(ns * k * d, dtype=torch.float64, device=device)

    def step(self):
        """One certified step against self.C; afterwards self.C_used holds the centres the labels and
        bounds refer to and self.C the next ones (the kernel's own update)."""
        x, k, n, ctr = self.x, self.k, self.n, self.ctr
        K.cert_stats(self.C, self.C_cur, self.s, self.drift, self.dtop, zero=ctr)
        K.cert_bounds(self.lab, self.u, self.l, self.drift, self.dtop, self.s, n, self.la, ctr[0:1])
        moves = (self.mv[0], self.mv[1], self.mv[2], ctr[2:3])
        K.cert_tighten(x, self.C, self.lab, self.u, self.l, self.s, self.la, ctr[0:1], self.lbl, ctr[1:2])
        K.exact_top2(x, self.C, self.lab, self.u, self.l, idx=self.lbl, n_dev=ctr[1:2], moves=moves)
        nxt = self.cbuf[1] if self.C.data_ptr() == self.cbuf[0].data_ptr() else self.cbuf[0]
        K.cert_moves(x, k, self.mv[0], self.mv[1], self.mv[2], ctr[2:3], ctr[4:], self.seg, self.cursor, self.perm,
                     self.P_hi, self.P_lo, self.S_hi, self.S_lo, self.cnt, C_cur=self.C, C_next=nxt)
        self.C_cur = self.C_used = self.C
        self.C = nxt
        return tuple(int(v) for v in ctr[:3].tolist())

    def restart(self, centres):
        """As set_centers between steps: the pending centres are replaced, then one certified step runs
        from the bounds of the last assignment."""
        self.C.copy_(dev(centres, self.C.device))
        return self.step()


# ---------------------------------------------------------------------------------------------- oracle-built outputs
# What a correct kernel returns, by the kernels' formulas in plain numpy: the checkers' own tests
# (test_cert_oracle.py) pass these and fail their mutants.

def stats_oracle_output(c):
    C, Cold = np.asarray(c["C"], dtype=F64), np.asarray(c["Cold"], dtype=F64)
    k = C.shape[0]
    dr2 = ((C - Cold) ** 2).sum(axis=1)
    drift = np.where(dr2 > 0, O.f32_up(np.sqrt(dr2) * (1 + O.FOLD_MARGIN)), F32(0)).astype(F32)
    s = np.full(k, np.inf, dtype=F32)
    if k > 1:
        D2 = numpy_sqdist(C, C)
        D2[np.arange(k), np.arange(k)] = np.inf
        s = O.f32_dn(0.5 * np.sqrt(D2.min(axis=1)) * (1 - O.FOLD_MARGIN))
    i1 = int(np.argmax(drift))
    rest = np.delete(drift, i1)
    dtop = np.array([drift[i1], rest.max() if k > 1 else 0.0, i1, 0.0], dtype=F32)
    return s, drift, dtop, np.zeros(4 + 2 * k, dtype=np.int32)


def bounds_oracle_output(c):
    un, ln, listed = O.bounds_oracle(c["lab"], c["u"], c["l"], c["drift"], c["dtop"], c["s"])
    lst = np.full(c["n"], -1, dtype=np.int32)
    lst[:listed.size] = listed[::-1]
    return un, ln, lst, listed.size


def tighten_oracle_output(c):
    rows = c["la"][:c["na"]].astype(np.int64)
    _, u_or, _, listed = O.tighten_oracle(c["X"], c["C"], c["lab"], c["l"], c["s"], rows)
    u = c["u"].copy()
    u[rows] = u_or
    lbst = np.full(c["n"], -1, dtype=np.int32)
    lbst[:listed.size] = listed
    bxn = np.full(c["n"], -1.0, dtype=F32)
    blab = np.full(c["n"], -1, dtype=np.int32)
    bxn[:listed.size], blab[:listed.size] = c["xn"][listed], c["lab"][listed]
    return u, lbst, listed.size, bxn, blab


def split_oracle_output(c):
    C = np.asarray(c["C"], dtype=F64)
    cb, lo, rc = O.split_oracle(C, c["kp"], c["ds"], c["ldc"])
    cn = np.full(c["kp"], np.inf, dtype=F32)
    cn[:c["k"]] = (C * C).sum(axis=1).astype(F32)
    cst = np.array([np.sqrt((a * a).sum(axis=1)).max() for a in (lo, C, rc)]) * (1 + 1e-9)
    return cb, cn, cst, np.array([cn[:c["k"]].max()], dtype=F32)


def list_oracle_output(c):
    cnt, n = c["cnt"], c["n"]
    rows = c["lst"][:cnt].astype(np.int64)
    uu, ll, bad = O.list_oracle(c)
    lab, u, l = c["lab"].copy(), c["u"].copy(), c["l"].copy()
    lab[rows[bad]] = c["blab"][:cnt][bad]
    u[rows[~bad]], l[rows[~bad]] = uu[~bad], ll[~bad]
    lc = np.full(n, -1, dtype=np.int32)
    lc[:int(bad.sum())] = rows[bad]
    mv = [np.full(n + LIST_M0, -1, dtype=np.int32) for _ in range(3)]
    for t, a in zip(mv, c["mv0"][:3]):
        t[:LIST_M0] = a
    moved = ~bad & (c["lab"][rows] != c["blab"][:cnt])
    m1 = LIST_M0 + int(moved.sum())
    mv[0][LIST_M0:m1], mv[1][LIST_M0:m1], mv[2][LIST_M0:m1] = rows[moved], c["blab"][:cnt][moved], c["lab"][rows[moved]]
    return lab, u, l, lc, int(bad.sum()), (mv[0], mv[1], mv[2], m1)
