"""CPU: the hostile inputs of tests/hostile_inputs.py are what they claim to be.

* every branch the header names, and every data class, occurs in the arrays the GPU tests run (a condition on the
  generators, printed as a table with -s);
* check_bits sees the sign of a zero and the position of a NaN;
* sgn(NaN) = 0: the header's statement, the restatement's `sgn`, and what follows for Pchip's end formula;
* the restatement on the finite hostile classes still agrees with scipy;
* mutants of the restatement -- the subtle ways a kernel could be wrong -- are told apart by at least one hostile array;
* the hostile Bicubic grids (tests/test_gpu_bicubic_hostile.py): finite where they claim to be, subnormal where they claim to
  be, non-finite in the planted lanes only, with queries that tell a left-sided cell search from the right-sided one;
* the same grids under the eight partial derivatives (tests/test_gpu_bicubic_partial_hostile.py): a top-scale and a subnormal
  lane per order, each exponent found by search and recorded, the subnormal lane judged by a flush-to-zero mutant, six
  mutants of H1 / H2 told apart, and the cases that claim nothing named in literals;
* the same grids made periodic (tests/test_gpu_bicubic_periodic_hostile.py): every family on a wrapping axis under every
  periodic-axes setting, hostile wrapped queries whose wrapped coordinates are never NaN and never below k0, finite tables
  and rows in every lane that claims them, a +0 / -0 seam lane, and the periodic top-scale exponents searched and recorded;
* the arrangement with a query per lane (tests/test_gpu_lanewise2d_hostile.py): every lane a permutation of the list, the
  lanes of a row in different places, every finite lane's reference at least 90 % finite in range and with extrapolation,
  and the top-scale exponents it needs searched and recorded;
* the Trilinear window cases (tests/test_gpu_trilinear_hostile.py): planted differences and spacings exactly on the edges of
  the division window and one float either side, every reference output finite, vectors inside and outside the window in
  every lane table by a restatement of the kernel's test; the hostile axes strictly rising and at least 75 % finite.
"""
import os

import numpy as np
import pytest

import derivative_ref
import hermite_ref
import hostile_inputs as hostile
from conftest import GOLDEN, ROOT
from hostile_inputs import check_bits

# the (n, L) grid of tests/test_gpu_cubic_hostile.py
NS = (2, 3, 4, 5, 6, 64, 301)
LS = (1, 3, 8, 130)
DTYPES = (np.float64, np.float32)


# ---- the comparer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32, np.float16])
def test_check_bits(dt):
    a = np.array([1.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 2.0], dt)
    check_bits(a, a.copy(), "same")
    b = a.copy(); b[1] = -0.0
    assert np.array_equal(a, b, equal_nan=True)                      # what check_equal would accept
    with pytest.raises(AssertionError, match=r"1 of 7 elements differ \(zero sign only: 1, NaN position: 0, value: 0\); first at \(1,\)"):
        check_bits(b, a, "zero")
    # another NaN payload and sign is the same NaN; a NaN that moved is not
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize]
    c = a.copy(); cv = c.view(u); cv[3] = cv[3] ^ u(1) ^ (u(1) << u(8 * np.dtype(dt).itemsize - 1))
    assert np.isnan(c[3]) and c.view(u)[3] != a.view(u)[3]
    check_bits(c, a, "payload")
    d = a.copy(); d[3] = 1.0; d[0] = np.nan
    with pytest.raises(AssertionError, match=r"2 of 7 elements differ \(zero sign only: 0, NaN position: 2, value: 0\)"):
        check_bits(d, a, "moved")
    e = a.copy(); e[6] = np.nextafter(dt(2.0), dt(3.0))
    with pytest.raises(AssertionError, match=r"value: 1\); first at \(6,\): got .* = 0x[0-9a-f]+, ref .* = 0x[0-9a-f]+"):
        check_bits(e, a, "one ulp")
    with pytest.raises(AssertionError, match="dtype"):
        check_bits(a.astype(np.float64), a.astype(np.float32), "dtype")
    with pytest.raises(AssertionError, match="shape"):
        check_bits(a[:3], a[:4], "shape")


# ---- the generators' self-check -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", hostile.RULES)
def test_every_branch_and_class_occurs(rule):
    """A condition on the generators: every count > 0 for every (rule, dtype, n >= 3, L) the GPU tests use."""
    print()
    for dt in DTYPES:
        for n in NS:
            if n < 3:
                continue
            worst = None
            for L in LS:
                t = hostile.branch_table(rule, dt, n, L)
                missing = [name for name in hostile.expected_branches(rule, n) if t[name] <= 0]
                assert not missing, (rule, np.dtype(dt).name, n, L, missing)
                worst = t if worst is None else {k: min(worst[k], t[k]) for k in t}
            print(f"{rule} {np.dtype(dt).name} n={n}: smallest count over L in {LS}")
            for name in hostile.expected_branches(rule, n):
                print(f"    {worst[name]:8d}  {name}")


def test_generators_are_seeded_and_shaped():
    for rule in hostile.RULES:
        for n, L in ((2, 3), (3, 1), (64, 8)):
            if rule == "akima" and n < 3:
                continue
            one = list(hostile.cases(rule, np.float32, n, L))
            two = list(hostile.cases(rule, np.float32, n, L))
            assert len(one) == len(two) >= 5
            for (t1, x1, y1, k1), (t2, x2, y2, k2) in zip(one, two):
                assert t1 == t2 and x1.dtype == y1.dtype == np.float32 and y1.shape == (n, L) and np.all(x1[1:] > x1[:-1])
                check_bits(x1, x2, t1); check_bits(y1, y2, t1)
                assert (k1 is None) == (rule != "hermite")
                if k1 is not None:
                    check_bits(k1, k2, t1)
    # the knot families
    for dt in DTYPES:
        x = hostile.knots("adjacent", dt, 9)
        assert np.all(np.nextafter(x[:-1], dt(np.inf)) == x[1:]) and hostile.has_adjacent(x)
        x = hostile.knots("huge", dt, 301)
        assert np.all(np.isfinite(x)) and np.all(np.diff(x) >= 0.99 * hostile.big_step(dt)) and not hostile.has_adjacent(x)
        x = hostile.knots("mixed", dt, 6)
        assert x[1] == np.nextafter(x[0], dt(np.inf)) and x[-1] - x[-2] >= 0.99 * hostile.big_step(dt)
        q = hostile.queries(hostile.knots("uneven", dt, 5))
        assert q.dtype == np.dtype(dt) and np.isinf(q).sum() == 2 and not np.isnan(q).any() and len(q) == 5 + 4 + 8 + 4 + 2


# ---- sgn(NaN) -----------------------------------------------------------------------------------------------------------
def test_sgn_of_the_specification():
    """include/ndinterp.h: sgn(v) = (v > 0) - (v < 0), so sgn(NaN) = 0.  A NaN slope at an end makes that end's k NaN unless
    sgn(d) != sgn(m0) has already decided."""
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert "sgn(v) = (v > 0) - (v < 0)" in header and "sgn(NaN) = 0" in header
    nan, inf = np.nan, np.inf
    v = np.array([nan, -nan, inf, -inf, 0.0, -0.0, 5e-324, -5e-324, 1.0, -2.0])
    assert hermite_ref.sgn(v).tolist() == [0, 0, 1, -1, 0, 0, 1, -1, 1, -1]
    assert hermite_ref.sgn(v.astype(np.float32)).tolist() == [0, 0, 1, -1, 0, 0, 0, 0, 1, -1]      # (5e-324 is 0 in f32)
    # invisible on finite data: equal to np.sign on every finite value of the goldens
    seen = 0
    for name in ("hermite_scipy.npz", "derivative_scipy.npz"):
        g = np.load(os.path.join(GOLDEN, name))
        for key in g.files:
            arr = g[key]
            if arr.dtype.kind == "f":
                f = arr[np.isfinite(arr)]
                assert np.array_equal(hermite_ref.sgn(f), np.sign(f).astype(np.int8)), (name, key)
                seen += f.size
    assert seen > 10_000
    # the end formula as a table: x, y -> k (pchip_k); the first two rows are the examples of the open question
    x = np.array([0.0, 1.0, 2.5, 3.0, 4.5])
    table = [
        ([1, 1, nan, 2, 3], {0: nan}),            # m0 = 0, m1 = NaN: d = NaN, sgn all 0 -> d
        ([1, 2, 3, nan, 5], {4: nan}),            # right end: m0 = NaN
        ([nan, 1, 2, 3, 4], {0: nan}),            # m0 = NaN itself
        ([1, 2, nan, 3, 4], {0: 0.0}),            # m0 = 1, m1 = NaN: d = NaN, sgn(d) = 0 != sgn(m0) = 1 decides first: +0
        ([1, 2, 3, 4, nan], {4: nan, 3: 0.0}),    # right end m0 = NaN; the interior knot before it: (2 > 0) != (NaN > 0), +0
        ([1, 1, 3, 4, 5], {0: 0.0}),              # m0 = 0, m1 != 0: sgn(d) = -1 != sgn(m0) = 0: +0
        ([1, 2, -13, 4, 5], {0: 3.0}),            # m0 = 1, m1 = -10: d = (3.5 + 10) / 2.5 > 3: 3 m0
        ([1, 2, 8, 9, 10], {0: 0.0}),             # m0 = 1, m1 = 4: d = (3.5 - 4) / 2.5 < 0: +0
        ([1, 2, inf, 3, 4], {0: 0.0}),            # m0 = 1, m1 = inf: d = -inf: +0
        ([inf, 2, 3, 4, 5], {0: -inf}),           # m0 = -inf, m1 = 2/3: d = -inf, same sign, |d| > 3 |m0| is false: d
        ([-0.0, -0.0, -0.0, 1, 2], {0: 0.0, 1: 0.0}),     # flat run of -0: +0, never -0
    ]
    for y, want in table:
        for dt in DTYPES:
            with np.errstate(all="ignore"):
                k = hermite_ref.pchip_k(x.astype(dt), np.array(y, dt)[:, None]).ravel()
            for i, v in want.items():
                check_bits(k[i:i + 1], np.array([v], dt), f"y = {y}: k_{i}")
    # and what the first example does to the table next to the NaN row: a_0 = k_0 h_0 - dy is NaN, no longer 0
    with np.errstate(all="ignore"):
        a, b = hermite_ref.build("pchip", x, np.array([1, 1, nan, 2, 3.0])[:, None])
    assert np.isnan(a[0, 0]) and b[0, 0] == 0 and np.isnan(a[1, 0])      # (k_1 = +0: delta_0 == 0 decides before the NaN)


# ---- the restatement on finite hostile data against scipy ---------------------------------------------------------------
def _finite_case(x, y):
    return np.all(np.isfinite(y))


@pytest.mark.parametrize("rule", ["pchip", "akima"])
@pytest.mark.parametrize("dt", DTYPES)
def test_restatement_on_finite_hostile_data_matches_scipy(rule, dt):
    """The bound of tests/test_hermite_abi.py: 4 x the deviation stored in tests/golden/hermite_scipy.npz, relative to
    max|y| + 1; scipy computes in f64 from the same (f32 or f64) inputs.

    Left to the bit comparison alone, because scipy's rule differs there or scipy itself leaves the finite range:
    * lanes whose f64 slopes or tables overflow the dtype (the "dy overflows", "3 (b - a) overflows" and "all exponents"
      recipes, the huge / adjacent / mixed axes): the restatement has inf or NaN where scipy, in f64, has finite numbers,
      or both overflow;
    * f32 lanes with subnormal differences on their own are kept: scipy sees the same inputs, and the deviation is far
      below the bound, which is relative to max|y| + 1;
    * Akima lanes with some s below scipy's threshold (1e-9 of the largest s of the lane) other than exact zeros: scipy
      averages there, the header does not.  Lanes where every s is either exactly 0 or above the threshold are kept."""
    scipy_interpolate = pytest.importorskip("scipy.interpolate")
    g = np.load(os.path.join(GOLDEN, "hermite_scipy.npz"))
    bound = 4.0 * float(g[f"deviation/{np.dtype(dt).name}/{rule}"])
    seen, worst = 0, 0.0
    for n in (3, 4, 5, 6, 64):
        for tag, x, y, _ in hostile.cases(rule, dt, n, 130, classes=("branch", "zero", "scale"), kinds=("even", "uneven")):
            ra, rb = hostile.reference(rule, x, y)
            q = hostile.queries(x, extrapolate=False)
            with np.errstate(all="ignore"):
                got = hermite_ref.evaluate(x, y, ra, rb, q).astype(np.float64)
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            for l in range(y.shape[1]):
                if not (np.all(np.isfinite(y[:, l])) and np.all(np.isfinite(ra[:, l])) and np.all(np.isfinite(rb[:, l]))
                        and np.all(np.isfinite(got[:, l]))):
                    continue
                if np.abs(y64[:, l]).max() > 1e-3 * float(np.finfo(dt).max):
                    continue
                if rule == "akima":
                    with np.errstate(all="ignore"):
                        s = hermite_ref.akima_k(x64, y64[:, l:l + 1])[1].ravel()
                    if np.any((s > 0) & (s <= 1e-6 * s.max())):
                        continue
                    want = scipy_interpolate.Akima1DInterpolator(x64, y64[:, l])(q.astype(np.float64))
                else:
                    want = scipy_interpolate.PchipInterpolator(x64, y64[:, l])(q.astype(np.float64))
                dev = float(np.abs(got[:, l] - want).max() / (np.abs(y64[:, l]).max() + 1))
                worst = max(worst, dev)
                seen += 1
                assert dev <= bound, (tag, l, dev, bound)
    assert seen >= 300, seen
    print(f"{rule} {np.dtype(dt).name}: {seen} finite hostile lanes, largest deviation from scipy {worst:.3e}, bound {bound:.3e}")


# ---- mutants ----------------------------------------------------------------------------------------------------------------
def entry_build(rule, x, y, dydx=None, mutant=None):
    """The build as the kernel is organised (csrc/hermite_kernels.hpp): one table entry per interval i, the window of rows
    around it, k_i and k_{i+1} formed per entry -- in numpy over the lanes.  `mutant` switches in one subtle error."""
    T = y.dtype.type
    n = len(x)
    zero = T(-0.0) if mutant == "flat branch returns -0" else T(0)
    sgn = (lambda v: np.sign(v)) if mutant == "np.sign for NaN" else hermite_ref.sgn

    def interior(hp, hc, dp, dc):
        flat = (dp == 0) | (dc == 0) | ((dp > 0) != (dc > 0))
        w1 = (hc + hc) + hp
        w2 = hc + (hp + hp)
        return np.where(flat, zero, (w1 + w2) / (w1 / dp + w2 / dc))

    def edge(h0, h1, m0, m1):
        d = (((h0 + h0) + h1) * m0 - h0 * m1) / (h0 + h1)
        opp = sgn(d) != sgn(m0)
        big = (sgn(m0) != sgn(m1)) & (np.abs(d) > T(3) * np.abs(m0))
        return np.where(opp, T(0), np.where(big, T(3) * m0, d))

    def akima(mm2, mm1, m0, mp1):
        w1 = np.abs(mp1 - m0)
        w2 = np.abs(mm1 - mm2)
        s = w1 + w2
        return np.where(s == 0, T(0.5) * (mm1 + m0), (w1 * mm1 + w2 * m0) / s)
    halo = {"pchip": 1, "akima": 2, "hermite": 0}[rule]
    a = np.empty((n - 1, y.shape[1]), y.dtype)
    b = np.empty_like(a)
    with np.errstate(all="ignore"):
        for i in range(n - 1):
            rows = [y[i + w - halo] if 0 <= i + w - halo < n else np.zeros(y.shape[1], y.dtype) for w in range(2 + 2 * halo)]
            xs = [x[i + w - halo] if 0 <= i + w - halo < n else T(0) for w in range(2 + 2 * halo)]
            hi = xs[halo + 1] - xs[halo]
            dy = rows[halo + 1] - rows[halo]
            if rule == "hermite":
                k0, k1 = dydx[i], dydx[i + 1]
            else:
                h = [xs[w + 1] - xs[w] for w in range(len(xs) - 1)]
                dl = [(rows[w + 1] - rows[w]) / h[w] for w in range(len(xs) - 1)]
                if rule == "pchip":
                    if n == 2:
                        k0 = k1 = dl[1]
                    else:
                        k0 = edge(h[1], h[2], dl[1], dl[2]) if i == 0 else interior(h[0], h[1], dl[0], dl[1])
                        k1 = edge(h[1], h[0], dl[1], dl[0]) if i + 2 == n else interior(h[1], h[2], dl[1], dl[2])
                else:
                    m = list(dl)
                    if i + 1 < 2: m[1] = (m[2] + m[2]) - m[3]
                    if i + 0 < 2: m[0] = (m[1] + m[1]) - m[2]
                    if (i + 3 >= n) if mutant == "akima extension i + 3 >= n" else (i + 3 > n): m[3] = (m[2] + m[2]) - m[1]
                    if i + 4 > n: m[4] = (m[3] + m[3]) - m[2]
                    k0 = akima(m[0], m[1], m[2], m[3])
                    k1 = akima(m[1], m[2], m[3], m[4])
            a[i] = k0 * hi - dy
            b[i] = dy - k1 * hi
    return a, b


def _flush(v):
    out = v.copy()
    out[(out != 0) & (np.abs(out) < np.finfo(v.dtype).tiny)] = 0
    return out


@pytest.mark.parametrize("rule", hostile.RULES)
@pytest.mark.parametrize("dt", DTYPES)
def test_entry_formulation_equals_the_restatement(rule, dt):
    """The per-entry organisation of the kernel and the whole-array restatement are the same numbers, bit for bit, on every
    hostile array of the small shapes: the stand-in the mutants are applied to is right before it is made wrong."""
    for n in NS[:6]:
        if rule == "akima" and n < 3:
            continue
        for tag, x, y, k in hostile.cases(rule, dt, n, 130):
            ra, rb = hostile.reference(rule, x, y, k)
            ea, eb = entry_build(rule, x, y, k)
            check_bits(ea, ra, tag + ": a"); check_bits(eb, rb, tag + ": b")


MUTANTS = [("pchip", "flat branch returns -0"), ("pchip", "np.sign for NaN"), ("akima", "akima extension i + 3 >= n"),
           ("pchip", "flushed subnormals"), ("akima", "flushed subnormals"), ("hermite", "flushed subnormals"),
           ("pchip", "derivative 3 (a - b)"), ("akima", "derivative 3 (a - b)"), ("hermite", "derivative 3 (a - b)")]


@pytest.mark.parametrize("rule,mutant", MUTANTS)
@pytest.mark.parametrize("dt", DTYPES)
def test_hostile_inputs_tell_a_mutant_from_the_restatement(rule, mutant, dt):
    """Each mutant is one subtle error a kernel could have; check_bits against the unmodified restatement must fail on at
    least one hostile array of EVERY (n, L) of the small shapes (n >= 3), so no lane mapping depends on another's luck."""
    print()
    for n in (3, 4, 5, 6, 64):
        for L in LS:
            caught = []
            for tag, x, y, k in hostile.cases(rule, dt, n, L):
                ra, rb = hostile.reference(rule, x, y, k)
                if mutant == "derivative 3 (a - b)":
                    ref = hostile.derivative_reference(x, y, ra, rb)
                    with np.errstate(all="ignore"):
                        got = (ref[0], (y.dtype.type(3) * (ra - rb)) / (x[1:] - x[:-1])[:, None])
                    ref = ref[:2]
                elif mutant == "flushed subnormals":
                    got = tuple(_flush(t) for t in entry_build(rule, x, _flush(y), None if k is None else _flush(k)))
                    ref = (ra, rb)
                else:
                    got = entry_build(rule, x, y, k, mutant)
                    ref = (ra, rb)
                try:
                    for g, r in zip(got, ref):
                        check_bits(g, r, tag)
                except AssertionError as e:
                    caught.append(str(e))
            assert caught, f"{mutant}: no hostile array of {rule} {np.dtype(dt).name} n={n} L={L} notices"
            if (n, L) == (64, 130):
                print(f"{mutant} / {rule} {np.dtype(dt).name}: {len(caught)} arrays notice, e.g. {caught[0][:230]}")


def test_derivative_restatement_keeps_its_order():
    """3 (b - a) and not 3 (a - b); (dy + a) / dx on the left and (dy - b) / dx at the last knot -- on numbers where each
    choice shows."""
    x = np.array([0.0, 2.0, 3.0]); y = np.array([[1.0], [4.0], [2.0]]); a = np.array([[0.5], [-1.0]]); b = np.array([[2.0], [3.0]])
    Y, A, B = derivative_ref.derive(x, y, a, b)
    assert Y.ravel().tolist() == [1.75, -3.0, -5.0] and A.ravel().tolist() == [2.25, 12.0] and np.array_equal(A, B)


# ---- the hostile Bicubic grids ----------------------------------------------------------------------------------------------
BICUBIC_FINITE = [i for i, n in enumerate(hostile.BICUBIC_RECIPES) if n not in ("inf node", "nan node")]
BICUBIC_CASES = [(dt, fx, fy) for dt in DTYPES for fx, fy in hostile.bicubic_pairs(dt)]


def _bicubic_case(dt, fx, fy, nx, ny, bc, finite_only=False, side="right"):
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    z, names = hostile.bicubic_nodes(dt, nx, ny, len(hostile.BICUBIC_RECIPES), 0, hostile.bicubic_top_exponent(dt, fx, fy),
                                    finite_only=finite_only)
    qx, qy = hostile.bicubic_queries(x, y)
    tabs, rows = hostile.bicubic_reference(x, y, z, bc, qx, qy, side=side)
    return x, y, z, names, qx, qy, tabs, rows


@pytest.mark.parametrize("dt,fx,fy", BICUBIC_CASES, ids=[f"{np.dtype(c[0]).name}-{c[1]}-{c[2]}" for c in BICUBIC_CASES])
def test_bicubic_hostile_grids_are_what_they_claim(dt, fx, fy):
    """Every (family pair, dtype) of the GPU tests, all recipes side by side in one array of nine lanes (lanes are independent,
    and bicubic_nodes gives a recipe the same lane whatever the array it sits in -- the last test below), both grids, both end
    sets, so that the device comparison is not NaN against NaN:
    * tables and rows of the finite recipes are at least 90 % finite on every grid and end set;
    * the subnormal lane's rows are at least 30 % subnormal with the default ends (MIXED prescribes an end slope of 0.75 on
      x, which no scaling of the data makes subnormal: rows near that end are of the order 1).  The share is pooled over
      the rows of both grids, one figure per (family pair, dtype).  Taken per grid it is printed below; its smallest values
      are 23 % on mixed2 x mixed2 and 34 % on mixed2 x adjacent, both on 6 x 7 in either dtype, and about 40 % or more
      everywhere else -- so every grid of every pair has subnormal rows for a flush to zero to show in: at least 20 % on
      each grid is asserted as well, a floor under those figures that still leaves hundreds of rows for a flush to show in;
    * the top-scale lane counts among the finite recipes: its exponent is found per family pair (the last test but one);
    * the inf and the NaN lane have non-finite rows, and every other lane has the bits it has without them;
    * evaluating with searchsorted(side="left") changes the bits of at least one row over the two grids: the queries at the
      nodes see the difference (a Hermite patch gives the node value from either side, so only the sign of a zero result
      can tell -- the "-0 among integers" lane is there for that)."""
    tiny = np.finfo(dt).tiny
    sub, total, left_differs, per_grid = 0, 0, 0, {}
    for nx, ny in hostile.BICUBIC_GRIDS:
        for bi, bc in enumerate(hostile.bicubic_ends()):
            x, y, z, names, qx, qy, tabs, rows = _bicubic_case(dt, fx, fy, nx, ny, bc)
            what = f"{np.dtype(dt).name} {fx} x {fy} {nx}x{ny} ends {bi}"
            assert names == list(hostile.BICUBIC_RECIPES)
            for l in BICUBIC_FINITE:
                assert hostile.finite_share(*[t[:, :, l] for t in tabs]) >= 0.9, (what, names[l], "tables")
                assert hostile.finite_share(rows[:, l]) >= 0.9, (what, names[l], "rows")
            if bc is None:
                l = names.index("subnormal")
                here = int(np.count_nonzero((rows[:, l] != 0) & (np.abs(rows[:, l]) < tiny)))
                per_grid[f"{nx}x{ny}"] = round(here / len(rows), 2)
                assert here >= 0.2 * len(rows), (what, "subnormal rows on this grid", per_grid)
                sub += here
                total += len(rows)
            _, _, _, _, _, _, ftabs, frows = _bicubic_case(dt, fx, fy, nx, ny, bc, finite_only=True)
            for l, name in enumerate(names):
                if l in hostile.BICUBIC_NONFINITE:
                    assert not np.all(np.isfinite(rows[:, l])), (what, name)
                    assert hostile.finite_share(frows[:, l]) >= 0.9, (what, name)
                else:
                    for a, b in zip(tabs + (rows,), ftabs + (frows,)):
                        check_bits(a[..., l], b[..., l], f"{what}: lane {name} beside the non-finite lanes")
            left = _bicubic_case(dt, fx, fy, nx, ny, bc, side="left")[-1]
            same = ((rows == left) & (np.signbit(rows) == np.signbit(left))) | (np.isnan(rows) & np.isnan(left))
            left_differs += int(np.count_nonzero(~same.all(axis=1)))
    assert sub >= 0.3 * total, (sub, total)
    assert left_differs >= 1
    print(f"{np.dtype(dt).name} {fx} x {fy}: subnormal rows {sub / total:.2f} {per_grid}, rows a left-sided search changes {left_differs}")


@pytest.mark.parametrize("dt", DTYPES)
def test_bicubic_top_scale_is_the_largest(dt):
    """The "top scale" lane: integers times 2^e with the largest e that keeps tables and rows 90 % finite on both grids and
    both end sets, found for every family pair (the knot spacings divide into it); e + 1 does not.  That the lane, as it sits
    in the arrays, is 90 % finite on every pair is part of test_bicubic_hostile_grids_are_what_they_claim."""
    found = {}
    for fx, fy in hostile.bicubic_pairs(dt):
        e = found[fx, fy] = hostile.bicubic_top_exponent(dt, fx, fy)
        assert hostile.bicubic_top_ok(dt, fx, fy, e) and not hostile.bicubic_top_ok(dt, fx, fy, e + 1), (fx, fy, e)
    print(f"{np.dtype(dt).name}: top scales 2^e, e = {found}")


def test_bicubic_generators_are_seeded_and_shaped():
    for dt in DTYPES:
        T = np.dtype(dt).type
        for fam in hostile.BICUBIC_FAMILIES:
            for n in (5, 6, 7, 65):
                k = hostile.bicubic_knots(fam, dt, n)
                assert k.dtype == np.dtype(dt) and k.shape == (n,) and np.all(np.isfinite(k)) and np.all(k[1:] > k[:-1])
                assert (0.0 in k) == (fam in ("big", "small"))
                assert hostile.has_adjacent(k) == (fam in ("adjacent", "mixed2"))
                # the query set: every knot, and both neighbours of every knot that lie in range; both zeros where 0.0 is a knot
                for ext in (False, True):
                    q = hostile.bicubic_axis_queries(k, ext)
                    assert q.dtype == np.dtype(dt) and not np.isnan(q).any()
                    have = set(q.tolist())
                    for v in k:
                        assert v in have
                        for nb in (np.nextafter(v, T(-np.inf)), np.nextafter(v, T(np.inf))):
                            assert nb in have or not (k[0] <= nb <= k[-1])
                    for a, b in zip(k[:-1], k[1:]):
                        assert a + (b - a) / T(2) in have
                    if 0.0 in k:
                        z = q[q == 0]
                        assert np.signbit(z).any() and not np.signbit(z).all()
                    w = k[-1] - k[0]
                    outside = q[(q < k[0]) | (q > k[-1])]
                    assert len(outside) == (10 if ext else 0)
                    if ext:
                        assert np.isinf(outside).sum() == 2 and k[0] - np.ldexp(w, 20) in have and k[-1] + w in have
        # a recipe's lane does not depend on the array it sits in: what the nine-lane self-check shows holds for every
        # (lanes, part) of the GPU tests; and every recipe occurs for every lane count
        nx, ny = hostile.BICUBIC_GRIDS[0]
        top = hostile.bicubic_top_exponent(dt)
        full, names = hostile.bicubic_nodes(dt, nx, ny, len(hostile.BICUBIC_RECIPES), 0, top)
        assert full.shape == (nx, ny, 9) and np.isinf(full[..., 5]).sum() == 1 and np.isnan(full[..., 6]).sum() == 1
        assert np.isinf(full[nx // 2, ny // 2, 5]) and np.isnan(full[nx // 2, ny // 2, 6])
        assert np.all(np.signbit(full[..., 4])) and not np.signbit(full[..., 3]).any() and np.signbit(full[..., 8][full[..., 8] == 0]).all()
        for C in hostile.BICUBIC_LANES:
            seen = []
            for part in range(hostile.bicubic_parts(C)):
                z, nm = hostile.bicubic_nodes(dt, nx, ny, C, part, top)
                z2, _ = hostile.bicubic_nodes(dt, nx, ny, C, part, top)
                check_bits(z, z2, "seeded")
                for l, name in enumerate(nm):
                    check_bits(z[..., l], full[..., names.index(name)], f"C={C} part={part} lane {l}")
                seen += nm
            assert set(seen) == set(hostile.BICUBIC_RECIPES), (C, seen)
        x, y = hostile.bicubic_grid("big", "uneven", dt, nx, ny)
        qx, qy = hostile.bicubic_queries(x, y)
        ax, ay = hostile.bicubic_axis_queries(x), hostile.bicubic_axis_queries(y)
        assert len(qx) == len(qy) == len(ax) * len(ay) + 2000 and qx.dtype == qy.dtype == np.dtype(dt)
        assert x[0] <= qx.min() and qx.max() <= x[-1] and y[0] <= qy.min() and qy.max() <= y[-1]


# ---- the hostile Bicubic grids under partial derivatives (tests/test_gpu_bicubic_partial_hostile.py) ------------------------------
import hashlib                                     # noqa: E402
import bicubic_partial_ref as partial_ref          # noqa: E402

ORDERS = partial_ref.ORDERS
ALL_MUTANTS = partial_ref.MUTANTS + partial_ref.ROUNDING_MUTANTS
# The integer lane's rows of these orders are less than 90 % finite on a grid (the smallest share beside each): a slope of the
# order 2^40 / 2^400 divided twice more by 2^-40 / 2^-400 -- genuine overflows of the contract's arithmetic.  These cases run
# on the device like every other; they make no finiteness claim, and their top-scale lane repeats the integers (exponent 0).
INTEGERS_OVERFLOW = {
    np.float32: {("adjacent", "small", (2, 2)): 0.08, ("small", "adjacent", (2, 2)): 0.08, ("small", "small", (2, 2)): 0.0,
                 ("small", "mixed2", (2, 2)): 0.6, ("mixed2", "small", (2, 2)): 0.55},
    np.float64: {("small", "small", (0, 2)): 0.0, ("small", "small", (1, 2)): 0.0, ("small", "small", (2, 1)): 0.0,
                 ("small", "small", (2, 2)): 0.0},
}
# ... and those the MIXED ends add (an end slope of 0.75 prescribed on x, which no scaling of the data changes)
INTEGERS_OVERFLOW_MIXED_ENDS = {np.float32: {}, np.float64: {}}
# No exponent in the whole range at which a flush to zero changes a row of that order on every grid: none.
NO_FLUSH_SHOWS = {np.float32: [], np.float64: []}
# On the pairs drawn from {uneven, big}^2 at least 20 % of the subnormal lane's rows of every order are subnormal on each
# grid, but for: f64 big x big (2, 2), whose rows are nodes times 2^-1600 while the tables overflow from nodes of 2^219 on
# (bicubic_top_exponent: 218) -- every such row is below the smallest subnormal, 2^-1074, whatever the exponent.
NO_SUBNORMAL_ROW_POSSIBLE = {np.float32: [], np.float64: [("big", "big", (2, 2))]}
_PARTIAL = {}


def _spacings(family, dt):
    return np.concatenate([np.diff(hostile.bicubic_knots(family, dt, n, seed)) for n in (5, 6, 7, 65) for seed in (0, 1)])


def mutant_can_show(variant, dt, fx, fy, order):
    """False where the mutant is the restatement itself, as a function, on every axis on which it changes the form that
    `order` uses: no node data can tell the two apart on those knots.  That is so for the three mutants that are about the
    rounding of a product or quotient with h, on an axis whose every spacing is a power of two (computed from the knots:
    adjacent, big, small, and mixed2, whose coarse steps round to 2^10 / 2^100 exactly): kl * h is exact, so rounding
    kl * h - d once is rounding it twice; 1 / h is exact, so x * (1 / h) is x / h; and x / h / h has an exact first quotient.
    (Exact but for a product or quotient that lands in the subnormal range, where the arithmetic is fixed-point and the
    second rounding changes a result only on a tie; nothing is claimed there.)  Such an axis cannot tell these mutants
    whatever lanes it carries: the pairs with an `uneven` axis under the mutated form are the ones that can.
    "contracted" is defined for f32 alone."""
    fams = [f for nu, f in zip(order, (fx, fy)) if nu in partial_ref.mutant_orders(variant)]
    if not fams:
        return False
    if variant in ("reciprocal", "h2_two_divisions", "contracted"):
        if variant == "contracted" and np.dtype(dt) != np.float32:
            return False
        return not all(bool(np.all(np.frexp(_spacings(f, dt))[0] == 0.5)) for f in fams)
    return True


def _partial_arrays(dt, fx, fy, bc):
    for nx, ny in hostile.BICUBIC_GRIDS:
        x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
        z, lanes = hostile.bicubic_partial_nodes(dt, nx, ny, fx, fy)
        qx, qy = hostile.bicubic_queries(x, y, True, n_random=300)       # the outside points included: s beyond [0, 1]
        yield x, y, z, lanes, qx, qy, hostile.bicubic_reference(x, y, z, bc)[0]


def partial_table(dt, fx, fy):
    """Everything the self-check says about one (dtype, pair), per order: computed once, asserted below."""
    key = (np.dtype(dt), fx, fy)
    if key in _PARTIAL:
        return _PARTIAL[key]
    out = {}
    arrays = {bi: list(_partial_arrays(dt, fx, fy, bc)) for bi, bc in enumerate(hostile.bicubic_ends())}
    for order in ORDERS:
        r = out[order] = {}
        r["integer share"] = [hostile.bicubic_integer_share(dt, fx, fy, order, bc) for bc in hostile.bicubic_ends()]
        e = r["top"] = hostile.bicubic_top_exponent(dt, fx, fy, order, recorded=False)
        r["top ok"] = (hostile.bicubic_top_ok(dt, fx, fy, e, order), hostile.bicubic_top_ok(dt, fx, fy, e + 1, order))
        s = r["sub"] = hostile.bicubic_sub_exponent(dt, fx, fy, order, recorded=False)
        r["recorded"] = hostile.bicubic_recorded_exponents(dt, fx, fy, order)
        sub, changed = hostile.bicubic_sub_scan(dt, fx, fy, order, [s])
        r["sub rows"], r["flush changes"] = sub[0].tolist(), changed[0].tolist()
        r["rows"] = [len(a[4]) for a in arrays[0]]
        # the mutants, on the arrays of the device test: the small grid first, the large one and the MIXED ends only if needed
        caught = {}
        for bi in arrays:
            for x, y, z, lanes, qx, qy, tabs in arrays[bi]:
                todo = [m for m in ALL_MUTANTS if m not in caught and mutant_can_show(m, dt, fx, fy, order)]
                if not todo:
                    break
                _, want = hostile.bicubic_reference(x, y, z, None, qx, qy, tabs=tabs, order=order)
                for m in todo:
                    _, got = hostile.bicubic_reference(x, y, z, None, qx, qy, tabs=tabs, order=order, variant=m)
                    n = hostile.changed_rows(got, want)
                    if n:
                        caught[m] = n
        r["caught"] = caught
        r["expected"] = [m for m in ALL_MUTANTS if mutant_can_show(m, dt, fx, fy, order)]
    _PARTIAL[key] = out
    return out


BICUBIC_PARTIAL_CASES = [(dt, fx, fy) for dt in DTYPES for fx, fy in hostile.bicubic_partial_pairs(dt)]


@pytest.mark.parametrize("dt,fx,fy", BICUBIC_PARTIAL_CASES, ids=[f"{np.dtype(c[0]).name}-{c[1]}-{c[2]}" for c in BICUBIC_PARTIAL_CASES])
def test_bicubic_partial_lanes_are_what_they_claim(dt, fx, fy):
    """Every (family pair, dtype) of tests/test_gpu_bicubic_partial_hostile.py and every order, so that the device comparison
    is not NaN against NaN or 0 against 0 in the lanes that matter.  Printed per order (-s): the top exponent, the subnormal
    exponent, the subnormal rows and the rows a flush to zero changes on each grid, the rows each mutant changes.
    * Finite share: the integer lane and the order's top-scale lane are at least 90 % finite in the rows of the order on both
      grids and both end sets, and one exponent more is not -- but for the cases of INTEGERS_OVERFLOW (9 of 440).
    * The subnormal lane is judged by a flush-to-zero mutant of the restatement (operands, tables, t, u and the result of
      every operation of H flushed): it changes at least one row of the order on each grid, in every case -- the search over
      the whole exponent range found no case without such an exponent (0 of 440; NO_FLUSH_SHOWS).  In 84 of 224 f32 cases and
      89 of 216 f64 cases no exponent gives a subnormal row on either grid -- rows of a derivative on adjacent, small or
      mixed2 axes would need nodes below the smallest subnormal -- and the lane found is the one whose subnormal operands
      (nodes, kl * h, pr - pl) a flush changes in the most rows.  On the pairs from {uneven, big}^2 every grid has at least
      20 % subnormal rows (a floor under measured figures of 94 % and more), but for the one case of NO_SUBNORMAL_ROW_POSSIBLE.
    * Mutants of H1 / H2 (bicubic_partial_ref.MUTANTS and ROUNDING_MUTANTS): each is told from the restatement on at least
      one row of some hostile array of the pair, for every order it can affect.  It cannot where it is the restatement (mutant_can_show):
      "reciprocal", "h2_two_divisions" and "contracted" on axes whose spacings are powers of two, which is every hostile
      family of the value tests; the `triple` axis of the three further pairs is there for them."""
    T = partial_table(dt, fx, fy)
    name = np.dtype(dt).name
    for (nx, ny) in hostile.BICUBIC_GRIDS:          # the lanes in the arrays are the lanes the searches ran on
        z, lanes = hostile.bicubic_partial_nodes(dt, nx, ny, fx, fy, 28)
        assert lanes[:9] == [(r, (0, 0)) for r in hostile.BICUBIC_RECIPES] and lanes[25:] == lanes[:3] and len(lanes) == 28
        check_bits(z[..., :9], hostile.bicubic_nodes(dt, nx, ny, 9, 0, hostile.bicubic_top_exponent(dt, fx, fy))[0], "the nine recipes")
        check_bits(z[..., 25:], z[..., :3], "lanes past 25 repeat")
        for k, order in enumerate(ORDERS):
            assert lanes[9 + 2 * k:11 + 2 * k] == [("top scale", order), ("subnormal", order)]
            ints = [hostile.bicubic_lane("integers", dt, nx, ny, np.random.default_rng([0, nx, ny, r])) for r in (7, 1)]
            with np.errstate(over="ignore"):
                check_bits(z[..., 9 + 2 * k], (ints[0] * np.ldexp(dt(1), T[order]["top"])).astype(dt), f"top lane {order}")
                check_bits(z[..., 10 + 2 * k], (ints[1] * np.ldexp(dt(1), T[order]["sub"])).astype(dt), f"subnormal lane {order}")
        zf, lf = hostile.bicubic_partial_nodes(dt, nx, ny, fx, fy, 28, finite_only=True)
        for l in range(28):
            if l in hostile.BICUBIC_NONFINITE:
                assert lf[l] == ("integers", (0, 0)) and np.all(np.isfinite(zf[..., l])) and not np.all(np.isfinite(z[..., l]))
            else:
                check_bits(zf[..., l], z[..., l], f"finite_only, lane {l}")
    for order in ORDERS:
        r = T[order]
        what = f"{name} {fx} x {fy} {order}"
        print(f"{what}: top 2^{r['top']}, subnormal lane 2^{r['sub']}: subnormal rows {r['sub rows']} and rows a flush changes "
              f"{r['flush changes']} of {r['rows']}, integer lane finite {[round(v, 2) for v in r['integer share']]}, mutants {r['caught']}")
        assert r["recorded"] == [r["top"], r["sub"]], (what, "the recorded exponents are not what the searches find", r["recorded"])
        listed = (fx, fy, order) in INTEGERS_OVERFLOW[dt] or (fx, fy, order) in INTEGERS_OVERFLOW_MIXED_ENDS[dt]
        if listed:
            assert r["top"] == 0, what
        else:
            assert min(r["integer share"]) >= 0.9, (what, r["integer share"])
            assert r["top ok"] == (True, False), (what, r["top"], r["top ok"])
        if (fx, fy, order) not in NO_FLUSH_SHOWS[dt]:
            assert all(c >= 1 for c in r["flush changes"]), (what, "a flush to zero changes no row on a grid", r["flush changes"])
        if fx in ("uneven", "big") and fy in ("uneven", "big") and (fx, fy, order) not in NO_SUBNORMAL_ROW_POSSIBLE[dt]:
            assert all(s >= 0.2 * n for s, n in zip(r["sub rows"], r["rows"])), (what, r["sub rows"], r["rows"])
        missed = [m for m in r["expected"] if m not in r["caught"]]
        assert not missed, f"{what}: no hostile array notices {missed}"


@pytest.mark.parametrize("dt", DTYPES)
def test_bicubic_partial_exclusions_are_the_listed_ones(dt):
    """The cases that make no finiteness claim, no flush claim or no subnormal-row claim are computed, and are the literal
    lists above: nothing is left out of a claim by a rule nobody can read."""
    default, mixed = hostile.bicubic_integer_overflows(dt, None), hostile.bicubic_integer_overflows(dt, hostile.bicubic_ends()[1])
    assert default == INTEGERS_OVERFLOW[dt], default
    assert {k: v for k, v in mixed.items() if k not in default} == INTEGERS_OVERFLOW_MIXED_ENDS[dt], mixed
    no_flush, no_sub = [], []
    for fx, fy in hostile.bicubic_partial_pairs(dt):
        T = partial_table(dt, fx, fy)
        for order in ORDERS:
            if not all(c >= 1 for c in T[order]["flush changes"]):
                no_flush.append((fx, fy, order))
            if fx in ("uneven", "big") and fy in ("uneven", "big") and sum(T[order]["sub rows"]) == 0:
                no_sub.append((fx, fy, order))
    assert no_flush == NO_FLUSH_SHOWS[dt] and no_sub == NO_SUBNORMAL_ROW_POSSIBLE[dt], (no_flush, no_sub)
    none = sum(1 for fx, fy in hostile.bicubic_partial_pairs(dt) for o in ORDERS if sum(partial_table(dt, fx, fy)[o]["sub rows"]) == 0)
    print(f"{np.dtype(dt).name}: {none} of {len(hostile.bicubic_partial_pairs(dt)) * len(ORDERS)} cases have no subnormal row at any exponent")


# sha256 of the nine-recipe array (6 x 7 x 9, top exponent 5) made with the default arguments, before the order argument
DEFAULT_BITS = {np.float32: "420ed827be92a8ec7103ed0ee8e01dbba435f5a9ce233b16810205ffb26e6ab8",
                np.float64: "6ec54fbda447ba55934ecca634a7f2540f6f5fc2915266a4fde5550b6170a10b"}


@pytest.mark.parametrize("dt", DTYPES)
def test_default_arguments_give_the_bits_they_gave(dt):
    """order=(0, 0) is the default and changes nothing: every recipe has the bits it had before the scaled recipes took an
    order (a digest of them, recorded then), and naming the default explicitly is the same lane."""
    z, _ = hostile.bicubic_nodes(dt, 6, 7, 9, 0, 5)
    assert hashlib.sha256(np.ascontiguousarray(z).tobytes()).hexdigest() == DEFAULT_BITS[dt]
    for r in range(len(hostile.BICUBIC_RECIPES)):
        a = hostile.bicubic_lane(r, dt, 6, 7, np.random.default_rng([0, 6, 7, r]), 5)
        b = hostile.bicubic_lane(r, dt, 6, 7, np.random.default_rng([0, 6, 7, r]), 5, order=(0, 0), pair=("small", "small"))
        check_bits(a, z[..., r], f"recipe {r}"); check_bits(b, a, f"recipe {r}, the default named")
    x, y = hostile.bicubic_grid("uneven", "mixed2", dt, 6, 7)
    qx, qy = hostile.bicubic_queries(x, y)
    tabs, rows = hostile.bicubic_reference(x, y, z, None, qx, qy)
    check_bits(hostile.bicubic_reference(x, y, z, None, qx, qy, tabs=tabs, order=(0, 0))[1], rows, "order (0, 0) is the surface")
    with np.errstate(all="ignore"):
        check_bits(partial_ref.evaluate(x, y, z, *tabs, qx, qy, 0, 0), rows, "the partial restatement at (0, 0)")
        for o in ORDERS:
            check_bits(hostile.bicubic_reference(x, y, z, None, qx, qy, tabs=tabs, order=o)[1],
                       partial_ref.evaluate(x, y, z, *tabs, qx, qy, *o), f"order {o}")


# ---- the hostile Bicubic grids with periodic axes (tests/test_gpu_bicubic_periodic_hostile.py) ---------------------------------
import bicubic_periodic_ref as periodic_ref        # noqa: E402

PERIODIC_FINITE = [n for n in hostile.BICUBIC_RECIPES + (hostile.SEAM_LANE,) if n not in ("inf node", "nan node", "top scale")]


def test_the_periodic_configurations_put_every_family_on_a_wrapping_axis():
    """Every knot family sits on a wrapping axis under each of the three periodic-axes settings at both grid sizes, in
    both dtypes; either end set of the other axis occurs beside x and beside y; the configurations are bicubic_pairs."""
    for dt in DTYPES:
        for gi in range(len(hostile.BICUBIC_GRIDS)):
            cases = hostile.bicubic_periodic_cases(dt, gi)
            assert [c[:2] for c in cases] == hostile.bicubic_pairs(dt)
            for fam in hostile.BICUBIC_FAMILIES:
                assert any(fx == fam for fx, fy, a, m in cases if a == "x"), (dt, gi, fam, "x")
                assert any(fy == fam for fx, fy, a, m in cases if a == "y"), (dt, gi, fam, "y")
                assert any(fx == fam for fx, fy, a, m in cases if a == "xy") and any(fy == fam for fx, fy, a, m in cases if a == "xy")
            for a in ("x", "y"):
                assert {m for fx, fy, s, m in cases if s == a} == {False, True}, (dt, gi, a)


def test_bicubic_wrapped_queries_are_what_they_claim():
    """The hostile set of a wrapping axis, on 3, 4, 6 and 65 knots of the five families and of `triple` and on the past-the-end
    axis of tests/test_gpu_bicubic_periodic_plans.py: the named points are in it, no wrapped coordinate is NaN and none is
    below k0 -- so a finite lane has finite rows; a wrapped coordinate may exceed kn, and on the past-the-end axis one does."""
    for dt in DTYPES:
        T = np.dtype(dt).type
        f = np.finfo(dt)
        axes = [hostile.bicubic_knots(fam, dt, n) for fam in hostile.BICUBIC_FAMILIES + ("triple",) for n in (3, 4, 6, 65)]
        k0, kn = T(-10) / T(7), T(3 if dt == np.float32 else 1)
        past = [np.concatenate([[k0], (float(k0) + (float(kn) - float(k0)) * np.arange(1, n - 1) / (n - 1)).astype(dt), [kn]]).astype(dt)
                for n in (3, 8, 65, 1000)]
        for k in axes + past:
            q = hostile.bicubic_wrap_axis_queries(k)
            assert q.dtype == np.dtype(dt) and np.all(np.isfinite(q))
            p = k[-1] - k[0]
            have = set(q.tolist())
            for v in (np.nextafter(k[0], T(-np.inf)), np.nextafter(k[-1], T(np.inf)), k[0] - f.tiny, k[0] - f.smallest_subnormal, f.max,
                      -f.max, k[0] - T(2**20) * p, k[-1] + T(2**20) * p, k[1] + T(2) * p, k[1] - p):
                assert v in have
            w = periodic_ref.wrap(k, q)
            assert not np.isnan(w).any() and not (w < k[0]).any(), k[:3]
        for k in past:
            assert T((k[-1] - k[0]) + k[0]) == np.nextafter(k[-1], T(np.inf))
            w = periodic_ref.wrap(k, hostile.bicubic_wrap_axis_queries(k))
            assert (w > k[-1]).any() and w.max() == np.nextafter(k[-1], T(np.inf))


@pytest.mark.parametrize("dt", DTYPES)
def test_bicubic_periodic_lanes_are_what_they_claim(dt):
    """Conditions on the restatement, for every pair, both grids and all three periodic-axes settings with the default ends
    (and with the ends the device test gives the case): every lane but `inf node`, `nan node` and `top scale` has
    all-finite tables and all-finite rows on the hostile wrapped queries; the inf and NaN lanes do not, their non-finite
    node is off the seam, and the other lanes have the bits they have without them; the seam lane is +0 in the first and
    -0 in the last row / column of a periodic axis, which the mismatch test (==) accepts; lanes 0 .. C - 2 are
    bicubic_nodes' made periodic."""
    for gi, (nx, ny) in enumerate(hostile.BICUBIC_GRIDS):
        mixed_of = {c[:3]: c[3] for c in hostile.bicubic_periodic_cases(dt, gi)}
        for fx, fy in hostile.bicubic_pairs(dt):
            x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
            for axes, a in hostile.PERIODIC_AXES.items():
                top = hostile.bicubic_periodic_top_exponent(dt, fx, fy, axes)
                z, names = hostile.bicubic_periodic_nodes(dt, nx, ny, 10, a, 0, top)
                zf, _ = hostile.bicubic_periodic_nodes(dt, nx, ny, 10, a, 0, top, finite_only=True)
                what = f"{np.dtype(dt).name} {fx} x {fy} {nx}x{ny} periodic {axes}"
                assert names == list(hostile.BICUBIC_RECIPES) + [hostile.SEAM_LANE]
                plain = periodic_ref.make_periodic(hostile.bicubic_nodes(dt, nx, ny, 9, 0, top)[0], a)
                check_bits(z[..., :9], plain, f"{what}: the nine recipes made periodic")
                s = z[..., 9]
                if a & 1:
                    assert np.all(z[0] == z[-1]) and not np.isnan(z[0]).any(), what
                    assert np.all(s[0, 1:-1] == 0) and not np.signbit(s[0, 1:-1]).any() and np.signbit(s[-1, 1:-1]).all(), what
                if a & 2:
                    assert np.all(z[:, 0] == z[:, -1]) and not np.isnan(z[:, 0]).any(), what
                    assert np.all(s[1:-1, 0] == 0) and not np.signbit(s[1:-1, 0]).any() and np.signbit(s[1:-1, -1]).all(), what
                qx, qy = hostile.bicubic_periodic_queries(x, y, a)
                for mixed in sorted({False, mixed_of.get((fx, fy, axes), False)}):
                    bc = hostile.bicubic_periodic_ends(a, mixed)
                    tabs, rows = hostile.bicubic_periodic_reference(x, y, z, bc, a, qx, qy)
                    ftabs, frows = hostile.bicubic_periodic_reference(x, y, zf, bc, a, qx, qy)
                    for l, name in enumerate(names):
                        if name in PERIODIC_FINITE:
                            assert all(np.isfinite(t[..., l]).all() for t in tabs), (what, mixed, name, "tables")
                            assert np.isfinite(rows[:, l]).all(), (what, mixed, name, "rows")
                        if l in hostile.BICUBIC_NONFINITE:
                            assert not np.isfinite(rows[:, l]).all() and np.isfinite(frows[:, l]).all(), (what, mixed, name)
                        else:
                            for u, v in zip(tabs + (rows,), ftabs + (frows,)):
                                check_bits(u[..., l], v[..., l], f"{what}: lane {name} beside the non-finite lanes")


@pytest.mark.parametrize("dt", DTYPES)
def test_bicubic_periodic_top_scale_is_the_largest(dt):
    """The "top scale" lane of a periodic build: integers times 2^e with the largest e at which the periodic restatement's
    three tables and its rows on the hostile wrapped queries are ALL finite on both grids and with both end sets of the other
    axis -- searched again here for every (pair, setting), equal to the recorded value
    (tests/golden/bicubic_periodic_exponents.json), and one step up is not all-finite.  Printed beside the exponents of the
    not-a-knot build (90 % finite, in-range queries), which overflow under a periodic build on some pairs."""
    found = {}
    for fx, fy in hostile.bicubic_pairs(dt):
        for axes in hostile.PERIODIC_AXES:
            e = hostile.bicubic_periodic_top_exponent(dt, fx, fy, axes, recorded=False)
            assert e == hostile.bicubic_periodic_recorded(dt, fx, fy, axes), (fx, fy, axes, e)
            assert hostile.bicubic_periodic_top_ok(dt, fx, fy, axes, e) and not hostile.bicubic_periodic_top_ok(dt, fx, fy, axes, e + 1)
            found[fx, fy, axes] = (e, hostile.bicubic_top_exponent(dt, fx, fy))
    below = {k: v for k, v in found.items() if v[0] < v[1]}
    print(f"{np.dtype(dt).name}: periodic top scales 2^e (beside the not-a-knot build's) = {found}; below it: {below}")


# ---- a query per lane (tests/test_gpu_lanewise2d_hostile.py) ------------------------------------------------------------------
def test_lanewise_arrangement_is_what_it_claims():
    """lane l holds the list rotated by l s with s prime to N: every lane meets every query once, and (L <= N) no two lanes of
    a row hold the same list position"""
    for N, L in ((1, 1), (7, 3), (12, 5), (625, 9), (2057, 25)):
        qx, qy = np.arange(N, dtype=np.float64), -np.arange(N, dtype=np.float64)
        xs, ys, s = hostile.lanewise_arrangement(qx, qy, L)
        assert xs.shape == ys.shape == (N, L) and np.gcd(s, N) == 1
        check_bits(ys, -xs, "the two coordinates stay paired")
        for l in range(L):
            assert np.array_equal(np.sort(xs[:, l]), qx) and xs[0, l] == (l * s) % N
        if L <= N:
            assert all(len(set(row)) == L for row in xs)
    with pytest.raises(AssertionError):
        hostile.lanewise_arrangement(np.arange(6.0), np.arange(6.0), 2, s=3)


@pytest.mark.parametrize("dt", DTYPES)
def test_bicubic_lanewise_lanes_are_what_they_claim(dt):
    """The arrays of the lane-wise hostile tests, nine recipes side by side: with a query per lane (lanewise_arrangement of the
    thinned list, in range and with extrapolation) the restatement's reference of every lane outside the planted inf / NaN
    lanes is at least 90 % finite, on both grids and with both end sets; so are the tables.  The top-scale exponent is
    searched again for every pair and equals the recorded one (tests/golden/bicubic_lanewise_exponents.json): the row-wise
    exponent where that holds the share on these lists, else the largest below it that does."""
    lowered = {}
    for fx, fy in hostile.bicubic_pairs(dt):
        e = hostile.bicubic_lanewise_top_exponent(dt, fx, fy, recorded=False)
        row = hostile.bicubic_top_exponent(dt, fx, fy)
        assert e == hostile.bicubic_lanewise_recorded(dt, fx, fy) and 0 <= e <= row, (fx, fy, e, row)
        assert hostile.bicubic_lanewise_top_ok(dt, fx, fy, e), (fx, fy, e)
        if e < row:
            lowered[fx, fy] = (e, row)
            assert not hostile.bicubic_lanewise_top_ok(dt, fx, fy, e + 1), (fx, fy, e)
        for nx, ny in hostile.BICUBIC_GRIDS:
            x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
            z, names = hostile.bicubic_nodes(dt, nx, ny, len(hostile.BICUBIC_RECIPES), 0, e)
            for bi, bc in enumerate(hostile.bicubic_ends()):
                tabs, _ = hostile.bicubic_reference(x, y, z, bc)
                for ext in (False, True):
                    xs, ys = hostile.bicubic_lanewise_queries(x, y, ext, len(names))
                    rows = hostile.bicubic_lanewise_reference(x, y, z, bc, xs, ys, tabs)
                    what = f"{np.dtype(dt).name} {fx} x {fy} {nx}x{ny} ends {bi} ext={ext}"
                    assert not np.array_equal(xs[:, 0], xs[:, 1])
                    for l in BICUBIC_FINITE:
                        assert hostile.finite_share(*[t[:, :, l] for t in tabs]) >= 0.9, (what, names[l], "tables")
                        assert hostile.finite_share(rows[:, l]) >= 0.9, (what, names[l], hostile.finite_share(rows[:, l]))
                    for l in hostile.BICUBIC_NONFINITE:
                        assert not np.all(np.isfinite(rows[:, l])), (what, names[l])
    print(f"{np.dtype(dt).name}: lane-wise top scales below the row-wise ones (e, row-wise e) = {lowered}")


BICUBIC_LANEWISE_PARTIAL_CASES = [(dt, fx, fy) for dt in DTYPES for fx, fy in hostile.bicubic_partial_pairs(dt)]


@pytest.mark.parametrize("dt,fx,fy", BICUBIC_LANEWISE_PARTIAL_CASES,
                         ids=[f"{np.dtype(c[0]).name}-{c[1]}-{c[2]}" for c in BICUBIC_LANEWISE_PARTIAL_CASES])
def test_bicubic_lanewise_partial_lanes_are_what_they_claim(dt, fx, fy):
    """The partial-order cases of the lane-wise hostile tests (hostile.LANEWISE_PARTIAL_ORDERS on the 25 lanes of
    bicubic_lanewise_partial_nodes), as test_bicubic_partial_lanes_are_what_they_claim has the row-wise sets: with a query per
    lane, in range and with extrapolation, on both grids, the integer lane and the order's own top-scale lane are at least
    90 % finite in the rows of the order, and so are their tables -- but for the cases of INTEGERS_OVERFLOW, whose lane repeats
    the integers (exponent 0) and claims nothing; that those are the only cases in which the integers fall short on these
    lists is asserted.  The exponent of every order is searched again and equals the recorded one: the row-wise exponent of
    that order where it holds the share on these lists, else the largest below it that does (one step up does not)."""
    name = np.dtype(dt).name
    found = {}
    for order in hostile.LANEWISE_PARTIAL_ORDERS:
        what = f"{name} {fx} x {fy} {order}"
        e = found[order] = hostile.bicubic_lanewise_partial_top_exponent(dt, fx, fy, order, recorded=False)
        row = hostile.bicubic_top_exponent(dt, fx, fy, order)
        assert e == hostile.bicubic_lanewise_recorded(dt, fx, fy, order) and 0 <= e <= row, (what, e, row)
        listed = (fx, fy, order) in INTEGERS_OVERFLOW[dt]
        falls_short = hostile.bicubic_lanewise_integer_share(dt, fx, fy, order) < 0.9 or \
            not hostile.bicubic_lanewise_partial_top_ok(dt, fx, fy, order, 0)
        assert falls_short == listed, (what, "the integers on the lane-wise lists", falls_short)
        if listed:
            assert e == 0, what
            continue
        assert hostile.bicubic_lanewise_partial_top_ok(dt, fx, fy, order, e), (what, e)
        if e < row:
            assert not hostile.bicubic_lanewise_partial_top_ok(dt, fx, fy, order, e + 1), (what, e)
    for nx, ny in hostile.BICUBIC_GRIDS:          # ... and on the arrays and the arrangement the device test runs
        x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
        z, lanes = hostile.bicubic_lanewise_partial_nodes(dt, nx, ny, fx, fy)
        zr, lanes_r = hostile.bicubic_partial_nodes(dt, nx, ny, fx, fy)
        zf, lanes_f = hostile.bicubic_lanewise_partial_nodes(dt, nx, ny, fx, fy, finite_only=True)
        assert lanes == lanes_r and len(lanes) == 25
        tabs, _ = hostile.bicubic_reference(x, y, z, None)
        for l, (recipe, o) in enumerate(lanes):
            if l in hostile.BICUBIC_NONFINITE:
                assert lanes_f[l] == ("integers", (0, 0)) and np.all(np.isfinite(zf[..., l])) and not np.all(np.isfinite(z[..., l]))
            else:
                check_bits(zf[..., l], z[..., l], f"finite_only, lane {l}")
            if recipe == "top scale" and o in found:
                ints = hostile.bicubic_lane("integers", dt, nx, ny, np.random.default_rng([0, nx, ny, 7]))
                with np.errstate(over="ignore"):
                    check_bits(z[..., l], (ints * np.ldexp(dt(1), found[o])).astype(dt), f"top lane {o}")
            elif not (recipe == "top scale" and o == (0, 0)):
                check_bits(z[..., l], zr[..., l], f"lane {l} is the row-wise array's")
        for order in hostile.LANEWISE_PARTIAL_ORDERS:
            if (fx, fy, order) in INTEGERS_OVERFLOW[dt]:
                continue
            sel = [lanes.index(("integers", (0, 0))), lanes.index(("top scale", order))]
            for ext in (False, True):
                xs, ys = hostile.bicubic_lanewise_queries(x, y, ext, len(lanes))
                rows = hostile.bicubic_lanewise_reference(x, y, np.ascontiguousarray(z[..., sel]), None, np.ascontiguousarray(xs[:, sel]),
                                                          np.ascontiguousarray(ys[:, sel]), tuple(t[..., sel] for t in tabs), order=order)
                for k, l in enumerate(sel):
                    what = f"{name} {fx} x {fy} {nx}x{ny} {order} ext={ext} lane {lanes[l]}"
                    assert hostile.finite_share(*[t[:, :, l] for t in tabs]) >= 0.9, (what, "tables")
                    assert hostile.finite_share(rows[:, k]) >= 0.9, (what, hostile.finite_share(rows[:, k]))
    print(f"{name} {fx} x {fy}: lane-wise top scales per order {found}")


# ---- an x axis per lane (tests/test_gpu_lane_axes_hostile.py) -------------------------------------------------------------------
LANE_AXES_L = 15
LANE_AXES_NS = (2, 3, 4, 5, 6, 33)
LANE_AXES_TWIN = ("branch", "zero", "scale")
LANE_AXES_RULE_NS = [(rule, n) for rule in hostile.RULES for n in LANE_AXES_NS if not (rule == "akima" and n < 3)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rule,n", LANE_AXES_RULE_NS)
def test_lane_axes_cases_are_seeded_and_shaped(dt, rule, n):
    """lane_axes_cases: the same call gives the same bits; x, y (and dydx for CubicHermite) are (n, L); every column is
    strictly rising; column l of part p is knots(KNOT_KINDS[(l + p) % 5], seed=l), so with 15 lanes every array holds every
    knot kind three times, neighbouring lanes never share a kind, and the kind in a lane position moves on by one with the
    part: over P parts a position sees min(P, 5) kinds (the recipe lists give 2 to 5 parts); y and dydx are generate()'s of
    that part on the even axis."""
    L = LANE_AXES_L
    for classes in (hostile.CLASSES, LANE_AXES_TWIN):
        first = list(hostile.lane_axes_cases(rule, dt, n, L, classes))
        again = list(hostile.lane_axes_cases(rule, dt, n, L, classes))
        P = hostile.parts(rule, n, L, classes)
        assert len(first) == len(again) == P >= 2
        kinds_at = [set() for _ in range(L)]
        for part, ((tag, x, y, k), (tag2, x2, y2, k2)) in enumerate(zip(first, again)):
            assert tag == tag2 and f"part={part}" in tag
            assert x.shape == y.shape == (n, L) and x.dtype == y.dtype == np.dtype(dt) and x.flags.c_contiguous
            assert (k is None) == (rule != "hermite") and (k is None or (k.shape == (n, L) and k.dtype == np.dtype(dt)))
            check_bits(x2, x, tag + ": x again")
            check_bits(y2, y, tag + ": y again")
            if k is not None:
                check_bits(k2, k, tag + ": dydx again")
            assert np.all(x[1:] > x[:-1]) and np.all(np.isfinite(x)), tag
            _, gy, gk = hostile.generate(rule, dt, n, L, classes, "even", part)
            check_bits(y, gy, tag + ": y is generate()'s")
            seen = set()
            for l in range(L):
                kind = hostile.KNOT_KINDS[(l + part) % 5]
                check_bits(x[:, l], hostile.knots(kind, dt, n, seed=l), f"{tag}: column {l} is the {kind} axis")
                kinds_at[l].add(kind)
                seen.add(kind)
            assert seen == set(hostile.KNOT_KINDS), tag
            if n > 2:          # (two knots: `adjacent` and `mixed` are the same two floats apart from the step)
                assert all(not np.array_equal(x[:, l], x[:, l + 1]) for l in range(L - 1)), tag
        assert all(len(s) == min(P, 5) for s in kinds_at), (rule, n, classes, [len(s) for s in kinds_at])
    q = hostile.lane_axes_queries(first[0][1])
    assert q.shape[1] == L and q.dtype == np.dtype(dt)
    for l in range(L):
        own = hostile.queries(np.ascontiguousarray(first[0][1][:, l]))
        check_bits(q[:len(own), l], own, f"lane {l}: its own query list first")
        assert np.all(q[len(own):, l] == own[-1]) or np.isnan(own[-1])


def lane_axes_finite_share(rule, x, y, k):
    """the share of finite elements among the oracle's rows, lane by lane on the lane's own in-range queries, evaluated on
    the restatement's tables -- nothing of the library is in it"""
    import oracle
    finite = total = 0
    for l in range(x.shape[1]):
        xc, yc = np.ascontiguousarray(x[:, l]), np.ascontiguousarray(y[:, l:l + 1])
        a, b = hostile.reference(rule, xc, yc, None if k is None else np.ascontiguousarray(k[:, l:l + 1]))
        q = hostile.queries(xc, extrapolate=False)
        assert np.all((q >= xc[0]) & (q <= xc[-1]))
        st, _, rows = oracle.interp1d_cubic(xc, yc, a, b, q)
        assert st == oracle.OK
        finite += int(np.count_nonzero(np.isfinite(rows)))
        total += rows.size
    return finite / total


def test_lane_axes_twin_arrays_are_mostly_finite():
    """The twin arrays (classes branch, zero, scale: no planted inf or NaN) on the knot tables of lane_axes_cases: the rows of
    every array are at least 75 % finite.  The huge and mixed columns overflow the slopes of ordinary data and the scale
    recipes overflow on any column, so the share is well below 1; what the floor keeps out is an arrangement whose rows are
    mostly inf and NaN, on which a bit-for-bit comparison says little.  80 arrays; measured worst 79.2 %."""
    shares = {}
    for dt in DTYPES:
        for rule, n in LANE_AXES_RULE_NS:
            for tag, x, y, k in hostile.lane_axes_cases(rule, dt, n, LANE_AXES_L, LANE_AXES_TWIN):
                shares[tag] = lane_axes_finite_share(rule, x, y, k)
    worst = min(shares, key=shares.get)
    print(f"lane-axes twin arrays: {len(shares)}, worst finite share {shares[worst]:.3f} ({worst})")
    assert len(shares) == 80
    low = {t: round(s, 3) for t, s in shares.items() if s < 0.75}
    assert not low, low


# ---- Trilinear: window edges and hostile axes (tests/test_gpu_trilinear_hostile.py) ---------------------------------------------
from fractions import Fraction                     # noqa: E402

import trilinear_ref as tr                         # noqa: E402


def vector_in_window(n, dt):
    """nums_in_window of csrc/kernels.hpp on one 16-byte vector (4 x f32 / 2 x f64), restated: the smallest magnitude >= N_LO
    and the sum of the magnitudes, formed in the dtype as the kernel forms it -- (|x| + |y|) + (|z| + |w|) in f32, |x| + |y|
    in f64 -- <= N_HI.  A NaN or an infinity fails the sum test."""
    w = hostile.trilinear_window(dt)
    m = np.abs(np.asarray(n, dt))
    with np.errstate(all="ignore"):
        s = (m[0] + m[1]) + (m[2] + m[3]) if m.size == 4 else m[0] + m[1]
        return bool(np.fmin.reduce(m) >= w["N_LO"]) and bool(s <= w["N_HI"])


def scalar_in_window(n, dt):
    w = hostile.trilinear_window(dt)
    return bool(w["N_LO"] <= abs(n) <= w["N_HI"])


def divisor_in_window(d, dt):
    w = hostile.trilinear_window(dt)
    return bool(w["D_LO"] <= d <= w["D_HI"])


@pytest.mark.parametrize("dt", DTYPES)
def test_trilinear_window_cases_are_what_they_claim(dt):
    """27 cases: every planted difference is the intended edge value, every spacing of the varying axis the intended divisor
    edge, both reference forms agree, every reference output is finite (27 000 of 27 000), and every lane table holds a
    vector inside the window and one outside it -- and lanes that are inside on their own in a vector that is outside, so
    that the scalar and the 16-byte form take different paths for the same lane."""
    T = np.dtype(dt).type
    w = hostile.trilinear_window(dt)
    prev, nxt = hostile._prev, hostile._next
    W = 16 // np.dtype(dt).itemsize
    assert [w[k] for k in ("N_LO", "N_HI", "D_LO", "D_HI")] == ([2.0 ** -60, 2.0 ** 60, 2.0 ** -40, 2.0 ** 40] if dt == np.float32 else
                                                                 [2.0 ** -500, 2.0 ** 500, 2.0 ** -400, 2.0 ** 400])
    cases = list(hostile.trilinear_window_cases(dt))
    assert len(cases) == 27 and len({c["tag"] for c in cases}) == 27
    assert {(c["vary"], c["table"], c["kind"]) for c in cases} == {(v, t, k) for v in range(3) for t in hostile.TRILINEAR_WINDOW_TABLES
                                                                     for k in hostile.TRILINEAR_WINDOW_AXES}
    # the lane tables, value by value
    a, b = hostile.trilinear_lane_table("low edge", dt)
    assert list(a[[0, 4, 5]]) == [prev(w["N_LO"]), w["N_LO"], nxt(w["N_LO"])] and a[0] < w["N_LO"] < a[5]
    assert np.array_equal(b, np.roll(a, 4))
    a, b = hostile.trilinear_lane_table("sum edge", dt)
    H = w["N_HI"] / T(W)
    assert np.all(a[:W] == H) and sum(Fraction(float(e)) for e in a[:W]) == Fraction(float(w["N_HI"]))       # exactly N_HI
    assert np.all(a[W:2 * W - 1] == H) and a[2 * W - 1] == nxt(H)
    assert np.all(b[:W - 1] == H) and b[W - 1] > nxt(H)
    a, b = hostile.trilinear_lane_table("scalar edge", dt)
    assert list(a[[2, 3, 4]]) == [w["N_HI"], w["N_LO"], nxt(w["N_HI"])] and a[0] == a[1] == b[4] == b[5] == w["N_HI"] / T(2)
    finite = total = 0
    for c in cases:
        tag, v, data, axes = c["tag"], c["vary"], c["data"], c["axes"]
        assert data.shape == (3, 3, 3, 8) and data.dtype == np.dtype(dt) and data.flags.c_contiguous, tag
        assert len(c["q"]) == 3 and all(q.size == 125 and q.dtype == np.dtype(dt) for q in c["q"]), tag
        # the data varies along one axis only; there the two differences are exactly (a, b), computed in the dtype
        d = np.moveaxis(data, v, 0)
        assert np.all(d == d[:, :1, :1, :]), tag
        col = d[:, 0, 0, :]
        check_bits(col[1] - col[0], c["a"], tag + ": the lower difference")
        check_bits(col[2] - col[1], c["b"], tag + ": the upper difference")
        assert np.all(col[1] == 0) and not np.any(np.signbit(col[1])), tag
        # the spacings of the varying axis, computed in the dtype, are the intended divisor edges
        k = axes[v]
        want = {"plain": None, "low divisor": [prev(w["D_LO"]), w["D_LO"]], "high divisor": [nxt(w["D_HI"]), w["D_HI"]]}[c["kind"]]
        sp = k[1:] - k[:-1]
        if want is None:
            assert all(divisor_in_window(s, dt) for s in sp), tag
        else:
            assert list(sp) == want and not divisor_in_window(sp[0], dt) and divisor_in_window(sp[1], dt), tag
        for o in range(3):
            if o != v:
                assert all(divisor_in_window(s, dt) for s in axes[o][1:] - axes[o][:-1]), tag
        # both forms of the reference, and every output finite
        r1 = tr.trilinear_ref(*axes, data, *c["q"])
        r2 = tr.trilinear_direct(*axes, data, *c["q"])
        assert r1[:2] == r2[:2] == (None, None), tag
        check_bits(r1[2], r2[2], tag + ": the two reference forms")
        assert np.array_equal(tr.bits(r1[2]), tr.bits(r2[2])), tag
        finite += int(np.count_nonzero(np.isfinite(r1[2])))
        total += r1[2].size
        assert np.isfinite(r1[2]).all(), tag
        # the calc_frac steps of the two constant axes return y1: at the knots of the varying axis the rows are the column
        on = [np.full(3, axes[o][1], dt) if o != v else k for o in range(3)]
        check_bits(tr.trilinear_ref(*axes, data, *on)[2][:2], col[:2], tag + ": rows on the knots of the varying axis")
        # the differing-path claim, per lane table (the numerators of both cells of the varying axis)
        vecs = [n[i:i + W] for n in (c["a"], c["b"]) for i in range(0, 8, W)]
        inside = [vector_in_window(n, dt) for n in vecs]
        assert any(inside) and not all(inside), (tag, inside)
        assert any(not vector_in_window(n, dt) and any(scalar_in_window(e, dt) for e in n) for n in vecs), tag
    print(f"trilinear window cases {np.dtype(dt).name}: finite {finite} of {total}")
    assert (finite, total) == (27_000, 27_000)
    # what the sum edge claims, by the restatement: N_HI exactly is inside; one float more in one lane is a tie that rounds back
    # to N_HI (inside as the kernel sums it, although the exact sum is above); four floats more is outside
    a, b = hostile.trilinear_lane_table("sum edge", dt)
    assert vector_in_window(a[:W], dt) and vector_in_window(a[W:2 * W], dt) and not vector_in_window(b[:W], dt)
    assert sum(Fraction(float(e)) for e in a[W:2 * W]) > Fraction(float(w["N_HI"]))
    # the nonfinite table: inside by its smallest magnitude, outside by the sum alone
    for c in hostile.trilinear_nonfinite_lane_cases(dt):
        col = np.moveaxis(c["data"], c["vary"], 0)[:, 0, 0, :]
        assert np.isfinite(c["data"]).all(), c["tag"]
        with np.errstate(over="ignore"):
            low = col[1] - col[0]
        assert low[1] == np.inf and low[6] == -np.inf, c["tag"]
        vecs = [low[i:i + W] for i in range(0, 8, W)]
        bad = [n for n in vecs if not np.isfinite(n).all()]
        assert len(bad) == 2 and all(np.abs(n).min() >= w["N_LO"] and not vector_in_window(n, dt) for n in bad), c["tag"]
        r1, r2 = tr.trilinear_ref(*c["axes"], c["data"], *c["q"]), tr.trilinear_direct(*c["axes"], c["data"], *c["q"])
        assert np.array_equal(tr.bits(r1[2]), tr.bits(r2[2])), c["tag"]
        # an infinite row survives where the planted division is the last one (z); after x or y the next level's difference of
        # two equal infinities is NaN
        assert np.isinf(r1[2]).any() == (c["vary"] == 2) and np.isnan(r1[2][:, [1, 6]]).any(), c["tag"]
        assert np.isfinite(r1[2][:, [0, 2, 3, 4, 5, 7]]).all(), c["tag"]


@pytest.mark.parametrize("dt", DTYPES)
def test_trilinear_axis_cases_are_what_they_claim(pkg, dt):
    """18 cases: every axis strictly rising (infinite end knots included: the builder's scan accepts them), adjacent floats
    where intended, -0.0 a knot and both zeros queries where intended, both reference forms agree, and at least 75 % of the
    reference's outputs are finite in every case, in range and extrapolating (NaN only where an infinite knot bounds the
    cell; measured: 0.8 on an axis with infinite ends -- 8 of its 10 queries -- and 1.0 everywhere else).  The reference's
    search cannot place a query strictly between infinite end knots: that is asserted here, and is why those cases keep
    the end knots and the queries of the inner cells only (hostile_inputs.trilinear_axis_reference)."""
    from ndarray_interp_amd.vector_extensions import Monotonic, monotonic_prop
    cases = list(hostile.trilinear_axis_cases(dt))
    assert len(cases) == 18 and len({c["tag"] for c in cases}) == 18
    shares = {}
    for c in cases:
        tag, h, axes, data = c["tag"], c["hostile"], c["axes"], c["data"]
        assert data.shape == (5, 5, 5, 4) and data.dtype == np.dtype(dt) and np.isfinite(data).all(), tag
        for o, k in enumerate(axes):
            assert k.shape == (5,) and k.dtype == np.dtype(dt) and np.all(k[1:] > k[:-1]), tag
            assert monotonic_prop(k) == Monotonic.Rising(True), tag
            assert hostile.has_adjacent(k) == (o == h and c["kind"] in ("adjacent", "mixed")), tag
            assert np.isfinite(k).all() == (not (o == h and c["kind"] == "infinite ends")), tag
        k = axes[h]
        if c["kind"] == "minus zero":
            assert k[2] == 0 and np.signbit(k[2]), tag
        if c["kind"] == "infinite ends":
            assert k[0] == -np.inf and k[-1] == np.inf, tag
        for ext in (False, True):
            q = c["q"][ext]
            per = hostile.trilinear_axis_queries(k, ext)
            if c["kind"] == "infinite ends":        # the end knots, and every point of the list inside the inner cells
                assert list(per[:2]) == [-np.inf, np.inf] and np.all((per[2:] >= k[1]) & (per[2:] < k[3])) and per.size == 10, tag
                assert {k[1], k[2], np.nextafter(k[1], dt(np.inf)), np.nextafter(k[3], dt(-np.inf))} <= set(per), tag
                import oracle                                # an interior query on the whole axis: the reference's guess is NaN
                assert list(oracle.get_lower_index(k, np.array([-np.inf, 0.25, np.inf], dt))) == [0, -1, 3], tag
            else:
                assert set(tr.bits(k)) <= set(tr.bits(per)), tag                               # every knot is a query
                assert set(tr.bits(np.nextafter(k[1:-1], dt(np.inf)))) | set(tr.bits(np.nextafter(k[1:-1], dt(-np.inf)))) <= set(tr.bits(per)), tag
            if c["kind"] in ("minus zero", "huge"):
                z = per[per == 0]
                assert np.signbit(z).any() and not np.signbit(z).all(), tag
            outside = (per < k[0]) | (per > k[-1])
            assert outside.sum() == (2 if ext and c["kind"] != "infinite ends" else 0), tag
            r1 = hostile.trilinear_axis_reference(c, ext)
            r2 = hostile.trilinear_axis_reference(c, ext, tr.trilinear_direct)
            assert r1[:2] == r2[:2] == (None, None), tag
            assert np.array_equal(tr.bits(r1[2]), tr.bits(r2[2])), tag
            shares[tag, ext] = hostile.finite_share(r1[2])
            if c["kind"] == "subnormal spacing":        # the reciprocal of the spacing overflows, many numerators are in the window
                W = 16 // np.dtype(dt).itemsize
                with np.errstate(over="ignore"):
                    assert np.isinf(dt(1) / (k[1:] - k[:-1])).all(), tag
                n = np.diff(data, axis=h).reshape(-1, W)
                assert np.mean([vector_in_window(v, dt) for v in n]) > 0.5, tag
            if c["kind"] != "infinite ends":
                assert shares[tag, ext] == 1.0, (tag, ext, shares[tag, ext])
    worst = min(shares, key=shares.get)
    print(f"trilinear axis cases {np.dtype(dt).name}: {len(shares)} query sets, worst finite share {shares[worst]:.3f} {worst}")
    low = {t: round(s, 3) for t, s in shares.items() if s < 0.75}
    assert not low, low
