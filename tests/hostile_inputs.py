"""Hostile inputs for the Pchip / Akima / CubicHermite build and the derivative build, and a bit-level comparer; further
down the hostile grids, lanes and queries of the 2-D Bicubic strategy and of its partial derivatives; at the end of the file
the window-edge and hostile-axis cases of the 3-D Trilinear strategy.

The rules (include/ndinterp.h, ndi_strategy1d / ndi_interp1d_derivative) have data-dependent branches and rest on plain
IEEE arithmetic: correctly rounded division, nothing fused, f32 subnormals kept.  The generators here plant every branch
the header names, zeros of both signs, subnormal / overflowing scales and non-finite values at chosen knots, each in a
lane of its own, so one (n, L) array carries many cases; lanes beyond the planted ones get seeded draws from the same
recipes.  `cases()` cuts the recipe list into as many arrays as L needs, so every lane mapping sees every recipe;
`lane_axes_cases()` puts the same arrays over a knot TABLE whose columns cycle through the knot kinds (handles with an x
axis per lane, tests/test_gpu_lane_axes_hostile.py).

`classify()` is the generators' self-check: it evaluates the header's conditions knot by knot (its own code, not
hermite_ref.pchip_k / akima_k) and counts how often each branch and data class occurs.
"""
import collections

import numpy as np

import derivative_ref
import hermite_ref

RULES = ("pchip", "akima", "hermite")
CLASSES = ("branch", "zero", "scale", "nonfinite")
KNOT_KINDS = ("even", "uneven", "adjacent", "huge", "mixed")


# ---- the comparer -------------------------------------------------------------------------------------------------------
def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_bits(got, ref, what):
    """Same dtype, same shape; every non-NaN element equal as its bit pattern (-0.0 != +0.0); NaN at the same positions
    (payload and sign of a NaN are not compared)."""
    got = np.ascontiguousarray(got); ref = np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.dtype.kind == "f", f"{what}: dtype {got.dtype} against {ref.dtype}"
    assert got.shape == ref.shape, f"{what}: shape {got.shape} against {ref.shape}"
    gn, rn = np.isnan(got), np.isnan(ref)
    gb, rb = _bits(got), _bits(ref)
    nanpos = gn != rn
    bad = nanpos | (~gn & ~rn & (gb != rb))
    if not bad.any():
        return
    zero = bad & ~nanpos & (got == 0) & (ref == 0)
    value = bad & ~nanpos & ~zero
    i = tuple(int(v) for v in np.argwhere(bad)[0])
    w = 2 * got.dtype.itemsize
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.size} elements differ (zero sign only: {int(zero.sum())}, NaN position: "
        f"{int(nanpos.sum())}, value: {int(value.sum())}); first at {i}: got {got[i]!r} = 0x{int(gb[i]):0{w}x}, "
        f"ref {ref[i]!r} = 0x{int(rb[i]):0{w}x}")


# ---- knots --------------------------------------------------------------------------------------------------------------
def big_step(dtype):
    return np.dtype(dtype).type(1e30 if np.dtype(dtype) == np.float32 else 1e300)


def knots(kind, dtype, n, seed=0):
    """even: 0, 1, 2 ... (slopes of integer data are exact); uneven: the well-conditioned axis of the other tests;
    adjacent: neighbouring floats from 1.0 up; huge: steps of 1e30 (f32) / 1e300 (f64) around 0; mixed: both spacings."""
    T = np.dtype(dtype).type
    if kind == "even":
        return np.arange(n).astype(dtype)
    if kind == "uneven":
        return np.cumsum(np.random.default_rng(1234 + seed).uniform(0.1, 2.0, n)).astype(dtype)
    if kind == "huge":
        return ((np.arange(n) - n // 2).astype(dtype) * big_step(dtype)).astype(dtype)
    x = np.empty(n, dtype)
    x[0] = 1.0
    near = n if kind == "adjacent" else (n + 1) // 2
    for i in range(1, n):
        x[i] = np.nextafter(x[i - 1], T(np.inf)) if i < near else x[i - 1] + big_step(dtype)
    assert kind in ("adjacent", "mixed") and np.all(x[1:] > x[:-1])
    return x


def has_adjacent(x):
    return bool(np.any(np.nextafter(x[:-1], x.dtype.type(np.inf)) == x[1:]))


# ---- lane recipes: f(n, T, rng) -> y column, or (y, dydx) columns -------------------------------------------------------------
def _bg(n, rng):
    """background slopes on the unit grid: small integers, zero included"""
    return rng.integers(-3, 4, n - 1).astype(np.float64)


def _col(sl, T, y0=1.0):
    return np.concatenate([[y0], y0 + np.cumsum(sl)]).astype(T)


def _slopes(plant):
    """a recipe from {slope index (negative: from the end): value}; planted where the index exists, the rest background"""
    def f(n, T, rng):
        sl = _bg(n, rng)
        if all(-(n - 1) <= j < n - 1 for j in plant):
            # an index may be named from both ends at small n: the later entry wins, as in a dict
            for j, v in plant.items():
                sl[j] = v
        return _col(sl, T)
    return f


def _mid(pattern):
    """slopes `pattern` centred so that pattern[len // 2 - 1], pattern[len // 2] are delta_{p-1}, delta_p, p = n // 2"""
    def f(n, T, rng):
        sl = _bg(n, rng)
        p = n // 2
        lo = p - len(pattern) // 2
        if lo >= 0 and lo + len(pattern) <= n - 1:
            sl[lo:lo + len(pattern)] = pattern
        return _col(sl, T)
    return f


def _random_lane(n, T, rng):
    return rng.normal(size=n).astype(T)


def _rounded_lane(n, T, rng):
    return np.round(rng.normal(size=n)).astype(T)


def branch_recipes(rule):
    r = [("random", _random_lane), ("rounded", _rounded_lane)]
    if rule == "pchip":
        r += [("int d0=0", _mid([0, 2])), ("int d1=0", _mid([2, 0])), ("int both 0", _mid([0, 0])),
              ("int + -", _mid([2, -1])), ("int - +", _mid([-1, 2])), ("int hm ++", _mid([1, 3])), ("int hm --", _mid([-1, -3])),
              # ends on the unit grid: d = (3 m0 - m1) / 2
              ("left opp", _slopes({0: 1, 1: 5})), ("left clamp", _slopes({0: 1, 1: -5})), ("left pass", _slopes({0: 2, 1: 1})),
              ("left m0=0", _slopes({0: 0, 1: 3})),
              ("right opp", _slopes({-1: 1, -2: 5})), ("right clamp", _slopes({-1: 1, -2: -5})), ("right pass", _slopes({-1: 2, -2: 1})),
              ("right m0=0", _slopes({-1: 0, -2: -3}))]
    elif rule == "akima":
        r += [("ramp", lambda n, T, rng: (3.0 * np.arange(n) - 7.0).astype(T)),
              ("flat", lambda n, T, rng: np.full(n, 2.5, T)),
              ("ramp left", _slopes({0: 2, 1: 2, 2: 2})), ("ramp right", _slopes({-1: -2, -2: -2, -3: -2})),
              ("ramp mid", _mid([1, 1, 1, 1, 1, 1])), ("flat mid", _mid([0, 0, 0, 0])),
              ("w1=0 low", _slopes({0: 1, 1: 3, 2: 3})), ("w2=0 high", _slopes({-3: 3, -2: 3, -1: 1})),
              ("w1=0 mid", _mid([1, 3, 2, 2])), ("w2=0 mid", _mid([2, 2, 3, 1]))]
    return r


def zero_recipes(rule):
    def runs(n, T, rng):
        return np.where((np.arange(n) // 3) % 2 == 0, T(-0.0), T(0.0)).astype(T)

    def alternating(n, T, rng):
        return np.where(np.arange(n) % 2 == 0, T(0.0), T(-0.0)).astype(T)

    def plateau(sign, level):
        def f(n, T, rng):     # level, level, then a plateau of signed zeros, then back: falling and rising steps onto 0
            y = np.full(n, level, T)
            y[n // 3:max(n // 3 + 1, 2 * n // 3)] = T(sign * 0.0)
            return y
        return f
    r = [("all -0", lambda n, T, rng: np.full(n, -0.0, T)), ("runs of -0 / +0", runs), ("alternating 0", alternating),
         ("plateau -0 below 1", plateau(-1.0, 1.0)), ("plateau +0 above -1", plateau(1.0, -1.0)), ("plateau -0 above -1", plateau(-1.0, -1.0))]
    if rule == "hermite":
        z = [(name, (lambda f: lambda n, T, rng: (f(n, T, rng), np.full(n, -0.0, T)))(f)) for name, f in r[:3]]
        r = z + [("dydx +0", lambda n, T, rng: (_rounded_lane(n, T, rng), np.zeros(n, T))),
                 ("dydx -0", lambda n, T, rng: (_rounded_lane(n, T, rng), np.full(n, -0.0, T))),
                 ("dydx alternating 0", lambda n, T, rng: (runs(n, T, rng), alternating(n, T, rng)))] + r[3:]
    return r


def scale_recipes(rule):
    def sub_values(n, T, rng):      # the values themselves subnormal: every difference is (the flush-to-zero detector)
        return (rng.integers(-4, 5, n).astype(T) * np.finfo(T).smallest_subnormal).astype(T)

    def sub_diffs(n, T, rng):       # normal values one or a few ulps apart at the bottom of the normal range
        return (np.finfo(T).tiny * (T(1) + rng.integers(0, 9, n).astype(T) * np.finfo(T).eps)).astype(T)

    def half_max(n, T, rng):        # opposite signs near max / 2 .. max: dy overflows
        s = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 if rng.integers(0, 2) else -1.0)
        return (s * rng.uniform(0.55, 0.95, n) * float(np.finfo(T).max)).astype(T)

    def tenth_max(n, T, rng):       # dy, a, b finite; 3 (b - a) of the derivative rule not
        return (rng.choice([-1.0, 1.0], n) * rng.uniform(0.05, 0.12, n) * float(np.finfo(T).max)).astype(T)

    def zigzag(n, T, rng):          # +-0.2 max: every interior Pchip k is +0, b - a = 2 dy = 0.8 max, 3 (b - a) overflows
        return (np.where(np.arange(n) % 2 == 0, 0.2, -0.2) * float(np.finfo(T).max)).astype(T)

    def w1_over_sub(n, T, rng):     # delta_{p-1} subnormal beside delta_p = 1: w1 / delta_{p-1} = inf, k_p = (w1 + w2) / inf = 0
        y = _col(np.abs(_bg(n, rng)) + 1.0, T, 0.0)
        p = n // 2
        if p >= 1 and p + 1 < n:
            y[:p] = 0; y[p] = np.finfo(T).smallest_subnormal; y[p + 1:] = y[p + 1:] - y[p + 1] + T(1)
        return y

    def w2_over_sub(n, T, rng):
        return (-w1_over_sub(n, T, rng)[::-1]).astype(T)

    def exponents(n, T, rng):       # the whole exponent range in one lane
        lim = 37 if T == np.float32 else 300
        with np.errstate(over="ignore"):
            return (rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-lim - 8, lim, n)).astype(T)
    r = [("subnormal values", sub_values), ("subnormal differences", sub_diffs), ("dy overflows", half_max),
         ("3 (b - a) overflows", tenth_max), ("zigzag 0.2 max", zigzag), ("w1 / delta = inf", w1_over_sub), ("w2 / delta = inf", w2_over_sub),
         ("all exponents", exponents)]
    if rule == "hermite":
        def steep(n, T, rng):       # flat data, k = -0.2 max: a = -0.2 max h, b = 0.2 max h, 3 (b - a) overflows on the unit grid
            return np.zeros(n, T), np.full(n, -0.2 * float(np.finfo(T).max), T)
        r = [(name, (lambda f: lambda n, T, rng: (f(n, T, rng), exponents(n, T, rng)))(f)) for name, f in r]

        def all_sub(n, T, rng):     # subnormal data and derivatives: subnormal tables (a_0 = 5 - 1 = 4 units on the unit grid)
            u = np.finfo(T).smallest_subnormal
            return (np.cumsum(np.arange(n)).astype(T) * u).astype(T), np.full(n, T(5) * u, T)
        r += [("dydx -0.2 max", steep), ("dydx subnormal", lambda n, T, rng: (_random_lane(n, T, rng), sub_values(n, T, rng))),
              ("y and dydx subnormal", all_sub)]
    return r


def nonfinite_rows(n):
    return sorted({r for r in (0, 1, 2, n // 2, n - 3, n - 2, n - 1) if 0 <= r < n})


def nonfinite_recipes(rule, n):
    def one(row, v, into_k):
        def f(n, T, rng):
            y, k = _random_lane(n, T, rng), _random_lane(n, T, rng)
            (k if into_k else y)[row] = v
            return (y, k) if rule == "hermite" else y
        return f

    def pair(v0, v1, into_k):
        def f(n, T, rng):
            y, k = _random_lane(n, T, rng), _random_lane(n, T, rng)
            p = min(n // 2, n - 2)
            (k if into_k else y)[p:p + 2] = [v0, v1]
            return (y, k) if rule == "hermite" else y
        return f
    def flat_end(right):
        def f(n, T, rng):      # a finite flat end interval beside a NaN row: m0 = 0, m1 = NaN, where sgn(NaN) = 0 shows in a / b
            y, k = _random_lane(n, T, rng), _random_lane(n, T, rng)
            if n >= 3:
                y[:3] = [y[0], y[0], np.nan]
                if right:
                    y = y[::-1].copy()
            return (y, k) if rule == "hermite" else y
        return f
    r = [("flat left end, then NaN", flat_end(False)), ("NaN, then flat right end", flat_end(True))]
    for into_k in ((False, True) if rule == "hermite" else (False,)):
        tag = "dydx" if into_k else "y"
        for v in (np.nan, np.inf, -np.inf):
            r += [(f"{tag}[{row}] = {v}", one(row, v, into_k)) for row in nonfinite_rows(n)]
        r += [(f"{tag} pair {v0} {v1}", pair(v0, v1, into_k)) for v0, v1 in ((np.inf, np.inf), (np.inf, -np.inf), (-np.inf, np.inf),
                                                                            (-np.inf, -np.inf))]
    return r


def recipes(rule, n, classes=CLASSES):
    r = []
    for c in classes:
        r += {"branch": lambda: branch_recipes(rule), "zero": lambda: zero_recipes(rule), "scale": lambda: scale_recipes(rule),
              "nonfinite": lambda: nonfinite_recipes(rule, n)}[c]()
    return r


# ---- the arrays ---------------------------------------------------------------------------------------------------------
def generate(rule, dtype, n, L, classes=CLASSES, kind="even", part=0, seed=0):
    """(x, y, dydx): x of `kind`, y (n, L), dydx (n, L) for rule "hermite" else None.  Lane l carries recipe part * L + l of
    recipes(rule, n, classes); lanes past the end of the list carry seeded random draws from it."""
    T = np.dtype(dtype).type
    rec = recipes(rule, n, classes)
    rng = np.random.default_rng([seed, n, L, part, KNOT_KINDS.index(kind), RULES.index(rule)])
    y = np.empty((n, L), dtype)
    k = np.empty((n, L), dtype)
    for l in range(L):
        j = part * L + l
        f = rec[j][1] if j < len(rec) else rec[int(rng.integers(0, len(rec)))][1]
        col = f(n, T, rng)
        if isinstance(col, tuple):
            y[:, l], k[:, l] = col
        else:
            y[:, l] = col
            k[:, l] = rng.normal(size=n)
    return knots(kind, dtype, n, seed), y, (k if rule == "hermite" else None)


def parts(rule, n, L, classes=CLASSES):
    return -(-len(recipes(rule, n, classes)) // L)


def cases(rule, dtype, n, L, classes=CLASSES, kinds=KNOT_KINDS):
    """Every array a test of this (rule, dtype, n, L) runs: (tag, x, y, dydx).  Every recipe on the even and the uneven axis;
    the scale recipes once more on each of the hostile axes."""
    for kind in kinds:
        cl = tuple(classes) if kind in ("even", "uneven") else tuple(c for c in classes if c == "scale")
        if not cl:
            continue
        for part in range(parts(rule, n, L, cl)):
            x, y, k = generate(rule, dtype, n, L, cl, kind, part)
            yield f"{rule} {np.dtype(dtype).name} n={n} L={L} knots={kind} part={part}", x, y, k


def lane_axes_table(dtype, n, L, part=0):
    """x[n][L] for a handle with an x axis per lane: column l is knots(KNOT_KINDS[(l + part) % 5], dtype, n, seed=l), so every
    array of five lanes or more holds every knot kind, neighbouring lanes never share a spacing, and the kind in a lane
    position moves on with the part."""
    x = np.stack([knots(KNOT_KINDS[(l + part) % len(KNOT_KINDS)], dtype, n, seed=l) for l in range(L)], axis=1)
    assert np.all(x[1:] > x[:-1])
    return np.ascontiguousarray(x)


def lane_axes_cases(rule, dtype, n, L, classes=CLASSES):
    """Every array the lane-axes tests of this (rule, dtype, n, L) run: (tag, x[n][L], y, dydx).  y and dydx are generate()'s
    on the even axis for every part of the recipe list (the recipes are slopes on the unit grid: on another column they are
    the same values over other spacings, which is the point); x is lane_axes_table of that part."""
    for part in range(parts(rule, n, L, classes)):
        _, y, k = generate(rule, dtype, n, L, classes, "even", part)
        yield f"{rule} {np.dtype(dtype).name} n={n} L={L} lane axes part={part}", lane_axes_table(dtype, n, L, part), y, k


def lane_axes_reference(rule, x, y, dydx=None):
    """(a, b) of a lane-axes table, column by column: reference() of (x[:, l], y[:, l]) alone"""
    cols = [reference(rule, np.ascontiguousarray(x[:, l]), np.ascontiguousarray(y[:, l:l + 1]),
                      None if dydx is None else np.ascontiguousarray(dydx[:, l:l + 1])) for l in range(x.shape[1])]
    return np.concatenate([c[0] for c in cols], axis=1), np.concatenate([c[1] for c in cols], axis=1)


def lane_axes_queries(x, extrapolate=True):
    """(Q, L): queries(x[:, l], extrapolate) per lane, padded to one length by repeating the lane's last query"""
    cols = [queries(np.ascontiguousarray(x[:, l]), extrapolate) for l in range(x.shape[1])]
    Q = max(len(c) for c in cols)
    return np.stack([np.concatenate([c, np.full(Q - len(c), c[-1], x.dtype)]) for c in cols], axis=1)


def reference(rule, x, y, dydx=None):
    """the restatement's (a, b) with numpy's floating-point warnings off: overflow and inf - inf are the point here"""
    with np.errstate(all="ignore"):
        return hermite_ref.build(rule, x, y, dydx)


def derivative_reference(x, y, a, b, nu=1):
    with np.errstate(all="ignore"):
        return derivative_ref.derive_nu(x, np.ascontiguousarray(y).reshape(len(x), -1), a, b, nu)


def queries(x, extrapolate=True):
    """every knot, nextafter of every knot in both directions (not where knots are adjacent floats), the interval midpoints;
    with extrapolation a point half an end interval outside on each side and +-inf"""
    T = x.dtype.type
    q = [x, x[:-1] + (x[1:] - x[:-1]) / T(2)]
    if not has_adjacent(x):
        q += [np.nextafter(x[:-1], T(np.inf)), np.nextafter(x[1:], T(-np.inf))]
    if extrapolate:
        q += [np.array([x[0] - (x[1] - x[0]) / T(2), x[-1] + (x[-1] - x[-2]) / T(2), np.inf, -np.inf], x.dtype)]
        if not has_adjacent(x):
            q += [np.array([np.nextafter(x[0], T(-np.inf)), np.nextafter(x[-1], T(np.inf))], x.dtype)]
    q = np.concatenate(q).astype(x.dtype)
    return q[np.isfinite(q) | extrapolate]


# ---- the self-check -------------------------------------------------------------------------------------------------------
def _s(v):
    return np.where(v > 0, 1, np.where(v < 0, -1, 0))


def _n(mask):
    return int(np.count_nonzero(mask))


def expected_branches(rule, n):
    """the names classify() must count at least once for `n` knots"""
    if rule == "pchip":
        names = ["pchip interior: delta_{i-1} == 0 only", "pchip interior: delta_i == 0 only", "pchip interior: both 0",
                 "pchip interior: + then -", "pchip interior: - then +", "pchip interior: harmonic mean, both +",
                 "pchip interior: harmonic mean, both -"]
        for side in ("left", "right"):
            names += [f"pchip {side} end: sgn(d) != sgn(m0)", f"pchip {side} end: 3 m0", f"pchip {side} end: d",
                      f"pchip {side} end: m0 == 0, m1 != 0", f"pchip {side} end: m0 == 0, m1 NaN: k NaN"]
        names += ["scale: w / delta = inf"]
    elif rule == "akima":
        names = ["akima s == 0 at i = 0", "akima s == 0 at i = 1", "akima s == 0 at i = n-2", "akima s == 0 at i = n-1", "akima s > 0"]
        if n >= 5:
            names += ["akima s == 0 at an interior knot"]
        if n >= 4:
            names += ["akima s > 0, w1 == 0 only", "akima s > 0, w2 == 0 only"]
    else:
        names = ["dydx: -0", "dydx: +0", "dydx: NaN", "dydx: +inf", "dydx: -inf", "dydx: subnormal"]
    names += ["zero: -0 in y", "zero: dy == 0 between zeros of different sign", "scale: subnormal dy", "scale: dy overflows",
              "nonfinite: NaN in y", "nonfinite: +inf in y", "nonfinite: -inf in y", "nonfinite: inf - inf", "tables: -0",
              "tables: subnormal"]
    # a and b near max / 3 with b - a finite: CubicHermite takes them from dydx; Pchip's k lies between 0 and 3 delta, so it
    # needs an interval between two interior knots whose k are both 0; Akima's own products w m overflow long before
    # (|y| >= sqrt(max)), so its tables are never that large and finite
    if rule == "hermite" or (rule == "pchip" and n >= 4):
        names += ["derivative: 3 (b - a) overflows, b - a finite"]
    return names


def classify(rule, x, y, dydx=None):
    """Counter of branch / data-class name -> occurrences over the knots and lanes of one array (n >= 3)."""
    c = collections.Counter()
    n = len(x)
    y = np.ascontiguousarray(y).reshape(n, -1)
    T = y.dtype.type
    tiny = np.finfo(T).tiny
    with np.errstate(all="ignore"):
        h = x[1:] - x[:-1]
        dy = y[1:] - y[:-1]
        dl = dy / h[:, None]
        if rule == "pchip":
            for i in range(1, n - 1):
                d0, d1 = dl[i - 1], dl[i]
                z0, z1 = d0 == 0, d1 == 0
                c["pchip interior: delta_{i-1} == 0 only"] += _n(z0 & ~z1)
                c["pchip interior: delta_i == 0 only"] += _n(~z0 & z1)
                c["pchip interior: both 0"] += _n(z0 & z1)
                c["pchip interior: + then -"] += _n((d0 > 0) & (d1 < 0))
                c["pchip interior: - then +"] += _n((d0 < 0) & (d1 > 0))
                c["pchip interior: harmonic mean, both +"] += _n((d0 > 0) & (d1 > 0))
                c["pchip interior: harmonic mean, both -"] += _n((d0 < 0) & (d1 < 0))
                w1 = (h[i] + h[i]) + h[i - 1]
                same = ((d0 > 0) & (d1 > 0)) | ((d0 < 0) & (d1 < 0))
                w2 = h[i] + (h[i - 1] + h[i - 1])
                c["scale: w / delta = inf"] += _n(same & np.isfinite(d0) & np.isfinite(d1) & (np.isinf(w1 / d0) | np.isinf(w2 / d1)))
            for side, h0, h1, m0, m1 in (("left", h[0], h[1], dl[0], dl[1]), ("right", h[-1], h[-2], dl[-1], dl[-2])):
                d = (((h0 + h0) + h1) * m0 - h0 * m1) / (h0 + h1)
                opp = _s(d) != _s(m0)
                clamp = ~opp & (_s(m0) != _s(m1)) & (np.abs(d) > T(3) * np.abs(m0))
                c[f"pchip {side} end: sgn(d) != sgn(m0)"] += _n(opp)
                c[f"pchip {side} end: 3 m0"] += _n(clamp)
                c[f"pchip {side} end: d"] += _n(~opp & ~clamp & ~np.isnan(d))
                c[f"pchip {side} end: m0 == 0, m1 != 0"] += _n((m0 == 0) & (m1 != 0) & ~np.isnan(m1))
                c[f"pchip {side} end: m0 == 0, m1 NaN: k NaN"] += _n(~opp & ~clamp & (m0 == 0) & np.isnan(m1))
        elif rule == "akima":
            m = {j: dl[j] for j in range(n - 1)}
            m[-1] = (m[0] + m[0]) - m[1]
            m[-2] = (m[-1] + m[-1]) - m[0]
            m[n - 1] = (m[n - 2] + m[n - 2]) - m[n - 3]
            m[n] = (m[n - 1] + m[n - 1]) - m[n - 2]
            for i in range(n):
                w1 = np.abs(m[i + 1] - m[i])
                w2 = np.abs(m[i - 1] - m[i - 2])
                s0 = (w1 + w2) == 0
                for name, at in (("i = 0", i == 0), ("i = 1", i == 1), ("i = n-2", i == n - 2), ("i = n-1", i == n - 1),
                                 ("an interior knot", 2 <= i <= n - 3)):
                    if at:
                        c[f"akima s == 0 at {name}"] += _n(s0)
                c["akima s > 0"] += _n((w1 + w2) > 0)
                c["akima s > 0, w1 == 0 only"] += _n((w1 == 0) & (w2 > 0))
                c["akima s > 0, w2 == 0 only"] += _n((w2 == 0) & (w1 > 0))
        else:
            k = np.ascontiguousarray(dydx).reshape(n, -1)
            c["dydx: -0"] += _n((k == 0) & np.signbit(k))
            c["dydx: +0"] += _n((k == 0) & ~np.signbit(k))
            c["dydx: NaN"] += _n(np.isnan(k))
            c["dydx: +inf"] += _n(k == np.inf)
            c["dydx: -inf"] += _n(k == -np.inf)
            c["dydx: subnormal"] += _n((k != 0) & (np.abs(k) < tiny))
        c["zero: -0 in y"] += _n((y == 0) & np.signbit(y))
        c["zero: dy == 0 between zeros of different sign"] += _n((dy == 0) & (np.signbit(y[1:]) != np.signbit(y[:-1])))
        c["scale: subnormal dy"] += _n((dy != 0) & (np.abs(dy) < tiny))
        c["scale: dy overflows"] += _n(np.isinf(dy) & np.isfinite(y[1:]) & np.isfinite(y[:-1]))
        c["nonfinite: NaN in y"] += _n(np.isnan(y))
        c["nonfinite: +inf in y"] += _n(y == np.inf)
        c["nonfinite: -inf in y"] += _n(y == -np.inf)
        c["nonfinite: inf - inf"] += _n(np.isinf(y[1:]) & (y[1:] == y[:-1]))
        a, b = hermite_ref.build(rule, x, y, dydx)
        c["derivative: 3 (b - a) overflows, b - a finite"] += _n(np.isfinite(b - a) & np.isinf(T(3) * (b - a)))
        c["tables: -0"] += _n(((a == 0) & np.signbit(a)) | ((b == 0) & np.signbit(b)))
        c["tables: subnormal"] += _n(((a != 0) & (np.abs(a) < tiny)) | ((b != 0) & (np.abs(b) < tiny)))
    return c


def branch_table(rule, dtype, n, L):
    total = collections.Counter({name: 0 for name in expected_branches(rule, n)})
    for _, x, y, k in cases(rule, dtype, n, L):
        total.update(classify(rule, x, y, k))
    return total


# ---- Bicubic: hostile grids (tests/test_gpu_bicubic_hostile.py, self-check in tests/test_hostile_inputs.py) ---------------
# The spline build squares the knot spacings, so the `huge` / `mixed` axes above (and subnormal spacings) leave no finite
# table entry; these families stay inside the range where the restatement (tests/bicubic_ref.py) is finite on integer data.
BICUBIC_FAMILIES = ("uneven", "adjacent", "big", "small", "mixed2")
BICUBIC_GRIDS = ((6, 7), (65, 5))
BICUBIC_LANES = (1, 4, 5, 9)
BICUBIC_RECIPES = ("integers", "subnormal", "constant", "+0", "-0", "inf node", "nan node", "top scale", "-0 among integers")
BICUBIC_NONFINITE = (5, 6)        # positions of the two non-finite recipes in BICUBIC_RECIPES
_BICUBIC_EXP = {np.dtype(np.float32): dict(step=40, coarse=10, sub=-135), np.dtype(np.float64): dict(step=400, coarse=100, sub=-1050)}


def bicubic_knots(family, dtype, n, seed=0):
    """uneven / adjacent: knots() above.  big / small: steps of 2^40 / 2^-40 (f32), 2^400 / 2^-400 (f64), centred so that 0.0
    is a knot.  mixed2: adjacent floats from 1.0 for the first half, then steps of 2^10 (f32) / 2^100 (f64).  triple (the
    partial-derivative tests only, bicubic_partial_pairs): every third float from 1.0 up."""
    T = np.dtype(dtype).type
    e = _BICUBIC_EXP[np.dtype(dtype)]
    if family in ("uneven", "adjacent"):
        return knots(family, dtype, n, seed)
    if family in ("big", "small"):
        step = np.ldexp(T(1), e["step"] if family == "big" else -e["step"])
        x = ((np.arange(n) - n // 2).astype(dtype) * step).astype(dtype)
    elif family == "triple":      # three floats apart from 1.0 up: as close as `adjacent`, but no spacing is a power of two
        x = (T(1) + T(3) * np.finfo(dtype).eps * np.arange(n).astype(dtype)).astype(dtype)
    else:
        assert family == "mixed2", family
        x = np.empty(n, dtype)
        x[0] = 1.0
        for i in range(1, n):
            x[i] = np.nextafter(x[i - 1], T(np.inf)) if i < (n + 1) // 2 else x[i - 1] + np.ldexp(T(1), e["coarse"])
    assert np.all(np.isfinite(x)) and np.all(x[1:] > x[:-1])
    return x


def bicubic_ends():
    """The two end-condition sets of the Bicubic tests: the default (None) and the MIXED ends of tests/test_gpu_bicubic.py."""
    import bicubic_ref
    return (None, bicubic_ref.MIXED_BC)


def bicubic_grid(fx, fy, dtype, nx, ny):
    return bicubic_knots(fx, dtype, nx, 0), bicubic_knots(fy, dtype, ny, 1)


def bicubic_pairs(dtype):
    """The (x family, y family) pairs the tests run.  f64 small x big is left out: its cross table zxy is a slope of the
    order 2^400 divided once more by 2^-400, which overflows with the default ends (tests/test_hostile_inputs.py shows it)."""
    return [(fx, fy) for fx in BICUBIC_FAMILIES for fy in BICUBIC_FAMILIES
            if not (np.dtype(dtype) == np.float64 and (fx, fy) == ("small", "big"))]


# Every spacing of adjacent, big, small and mixed2 is a power of two, on which a product or quotient with h is exact: a
# reciprocal for a division, x / h / h for x / (h * h) or a fused kl * h - d are the same function there, whatever the nodes
# (tests/test_hostile_inputs.py, mutant_can_show).  The partial-derivative tests, whose forms H1 and H2 have those divisions,
# therefore run three pairs more, on an axis as fine as `adjacent` whose spacing of 3 ulps is not.
BICUBIC_PARTIAL_EXTRA = (("triple", "triple"), ("triple", "uneven"), ("uneven", "triple"))


def bicubic_partial_pairs(dtype):
    return bicubic_pairs(dtype) + list(BICUBIC_PARTIAL_EXTRA)


def bicubic_lane(recipe, dtype, nx, ny, rng, top_exp=0, order=(0, 0), pair=None):
    """One lane (nx, ny) of node data.  `rng` is consumed the same way by every recipe, so the integer background of two
    arrays made with the same seed is the same lane by lane.  The two scaled recipes ("subnormal", "top scale") take the
    partial-derivative order whose rows they are for: with the default (0, 0) the fixed subnormal exponent and `top_exp`, with
    any other order the exponents found for it on the knot families `pair` (bicubic_sub_exponent, bicubic_top_exponent)."""
    T = np.dtype(dtype).type
    ints = rng.integers(-3, 5, (nx, ny)).astype(dtype)
    name = BICUBIC_RECIPES[recipe] if isinstance(recipe, int) else recipe
    order = tuple(order)
    if name == "integers":
        return ints
    if name == "subnormal":       # the flush-to-zero detector: every node value is subnormal or zero
        e = _BICUBIC_EXP[np.dtype(dtype)]["sub"] if order == (0, 0) else bicubic_sub_exponent(dtype, pair[0], pair[1], order)
        with np.errstate(over="ignore"):
            return (ints * np.ldexp(T(1), e)).astype(dtype)
    if name == "constant":
        return np.full((nx, ny), 2.5, dtype)
    if name == "+0":
        return np.zeros((nx, ny), dtype)
    if name == "-0":
        return np.full((nx, ny), -0.0, dtype)
    if name in ("inf node", "nan node"):      # one interior node
        ints[nx // 2, ny // 2] = np.inf if name == "inf node" else np.nan
        return ints
    if name == "top scale":
        if order != (0, 0):
            top_exp = bicubic_top_exponent(dtype, pair[0], pair[1], order)
        with np.errstate(over="ignore"):
            return (ints * np.ldexp(T(1), top_exp)).astype(dtype)
    assert name == "-0 among integers", name
    ints[ints == 0] = -0.0
    return ints


def bicubic_nodes(dtype, nx, ny, C, part=0, top_exp=0, seed=0, finite_only=False):
    """(z, names): z (nx, ny, C); lane l carries recipe (part * C + l) mod len(BICUBIC_RECIPES).  `finite_only` puts the
    integer lane where the inf / NaN recipes would go and changes nothing else (the lane-independence check)."""
    z = np.empty((nx, ny, C), dtype)
    names = []
    for l in range(C):
        r = (part * C + l) % len(BICUBIC_RECIPES)
        rng = np.random.default_rng([seed, nx, ny, r])
        if finite_only and r in BICUBIC_NONFINITE:
            r = 0
        names.append(BICUBIC_RECIPES[r])
        z[:, :, l] = bicubic_lane(r, dtype, nx, ny, rng, top_exp)
    return z, names


def bicubic_parts(C):
    return -(-len(BICUBIC_RECIPES) // C)


BICUBIC_PARTIAL_LANES = (25, 28)     # every lane once, scalar form (odd); the same and three more, 16-byte vectors in f32 and f64


def bicubic_partial_recipes():
    """The lanes of the partial-derivative arrays: the nine recipes, then for each of the eight orders a top-scale and a
    subnormal lane scaled for the rows of that order: (recipe name, order) for each of 25 lanes."""
    import bicubic_partial_ref
    return [(r, (0, 0)) for r in BICUBIC_RECIPES] + [(r, o) for o in bicubic_partial_ref.ORDERS for r in ("top scale", "subnormal")]


def bicubic_partial_nodes(dtype, nx, ny, fx, fy, C=25, seed=0, finite_only=False):
    """(z, lanes): z (nx, ny, C); lane l carries entry l mod 25 of bicubic_partial_recipes().  One array per grid serves the
    handles of all eight orders: a lane scaled for another order is mostly inf or 0 there, which still compares bit for bit.
    `finite_only` as in bicubic_nodes.  The integer background of a recipe is the one it has in bicubic_nodes, whatever the
    order (the exponents were searched on it)."""
    rec = bicubic_partial_recipes()
    top = bicubic_top_exponent(dtype, fx, fy)
    z = np.empty((nx, ny, C), dtype)
    lanes = []
    for l in range(C):
        name, order = rec[l % len(rec)]
        r = BICUBIC_RECIPES.index(name)
        rng = np.random.default_rng([seed, nx, ny, r])
        if finite_only and r in BICUBIC_NONFINITE:
            name = BICUBIC_RECIPES[0]
        lanes.append((name, order))
        z[:, :, l] = bicubic_lane(name, dtype, nx, ny, rng, top, order, (fx, fy))
    return z, lanes


def bicubic_axis_queries(k, extrapolate=False):
    """One axis: every knot, the float just above and just below each knot (clipped into range), every midpoint, both
    zeros where 0.0 is a knot; with `extrapolate` points up to a full axis width outside, points 2^20 widths outside and
    +-inf."""
    T = k.dtype.type
    q = [k, np.nextafter(k, T(np.inf)), np.nextafter(k, T(-np.inf)), k[:-1] + (k[1:] - k[:-1]) / T(2)]
    if np.any(k == 0):
        q.append(np.array([-0.0, 0.0], k.dtype))
    q = np.clip(np.concatenate(q).astype(k.dtype), k[0], k[-1])      # (np.clip keeps the sign of a zero)
    if extrapolate:
        w = k[-1] - k[0]
        far = np.ldexp(w, 20)
        q = np.concatenate([q, np.array([k[0] - w, k[0] - w / T(3), np.nextafter(k[0], T(-np.inf)), np.nextafter(k[-1], T(np.inf)),
                                         k[-1] + w / T(3), k[-1] + w, k[0] - far, k[-1] + far, -np.inf, np.inf], k.dtype)])
    return q


def bicubic_queries(x, y, extrapolate=False, seed=0, n_random=2000, thin=1):
    """(qx, qy): the cross product of the two axes' sets, then `n_random` points spread over the cells (a random cell and a
    random position inside it on each axis, so the wide cells of a mixed axis do not take them all).  `thin`: every thin-th
    pair of the cross product only; with `thin` prime to the length of the y set every point of either axis' set still occurs."""
    ax, ay = bicubic_axis_queries(x, extrapolate), bicubic_axis_queries(y, extrapolate)
    gx, gy = np.meshgrid(ax, ay, indexing="ij")
    if thin > 1:
        assert np.gcd(thin, len(ay)) == 1 and len(ax) >= thin, (thin, len(ax), len(ay))
        gx, gy = gx.ravel()[::thin], gy.ravel()[::thin]
    rng = np.random.default_rng([seed, len(x), len(y)])

    def spread(k):
        i = rng.integers(0, len(k) - 1, n_random)
        return np.clip(k[i] + (k[i + 1] - k[i]) * rng.uniform(0, 1, n_random).astype(k.dtype), k[0], k[-1]).astype(k.dtype)
    return np.concatenate([gx.ravel(), spread(x)]), np.concatenate([gy.ravel(), spread(y)])


def bicubic_reference(x, y, z, bc=None, qx=None, qy=None, tabs=None, side="right", order=(0, 0), variant=None):
    """(tables, rows) of the restatement with numpy's floating-point warnings off.  `tabs`: evaluate on these tables (the
    device's own) instead of the restatement's; `side="left"`: the wrong cell search, for the self-check.  `order`: rows of
    that partial derivative (tests/bicubic_partial_ref.py), `variant` one of its deliberately wrong forms."""
    import bicubic_ref
    with np.errstate(all="ignore"):
        if tabs is None:
            tabs = bicubic_ref.tables(x, y, z, bc or bicubic_ref.DEFAULT_BC)
        if qx is None:
            return tabs, None
        if tuple(order) == (0, 0) and variant is None:
            return tabs, bicubic_ref.evaluate(x, y, z, *tabs, qx, qy, side=side)
        import bicubic_partial_ref
        assert side == "right"
        return tabs, bicubic_partial_ref.evaluate(x, y, z, *tabs, qx, qy, order[0], order[1], variant)


def finite_share(*arrays):
    return float(np.mean(np.concatenate([np.isfinite(a).ravel() for a in arrays])))


_TOP = {}
_SUB = {}
_SEARCH = {}


def bicubic_recorded_exponents(dtype, fx, fy, order):
    """(top, sub) of tests/golden/bicubic_partial_exponents.json: what the two searches below found for the orders other than
    (0, 0), recorded so that the device tests do not search again (880 searches); tests/test_hostile_inputs.py runs every
    search and holds the file to the results."""
    import json
    import os
    if "recorded" not in _SEARCH:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicubic_partial_exponents.json")) as f:
            _SEARCH["recorded"] = json.load(f)
    return _SEARCH["recorded"].get(np.dtype(dtype).name, {}).get(f"{fx} {fy}", {}).get(f"{order[0]},{order[1]}")


def bicubic_top_exponent(dtype, fx="uneven", fy="uneven", order=(0, 0), recorded=True):
    """The largest e for which integer nodes times 2^e keep tables and rows of the restatement at least 90 % finite on this
    pair of knot families, on every grid of BICUBIC_GRIDS and both end sets -- found, not guessed.  The divisions by the knot
    spacings move it a long way: 2^118 / 2^1014 on uneven x uneven, far less on adjacent or small axes, so one exponent for
    all pairs would leave the lane all inf and NaN on most of them.  Bisection: tables and rows are linear in the nodes and a
    power of two scales them exactly, so what overflows at e overflows at e + 1 (tests/test_hostile_inputs.py holds the
    result to ok(e) and not ok(e + 1) for every pair).  `recorded=False` searches whatever the recorded file says.  `order`: the rows are those of that partial derivative (the tables do
    not depend on it).  Where the integer lane itself is not 90 % finite in the rows of an order -- a slope divided once or
    twice more by a spacing of 2^-40 / 2^-400, bicubic_integer_overflows -- there is no such e: the answer is 0, the lane
    repeats the integers and claims nothing."""
    order = tuple(order)
    key = (np.dtype(dtype), fx, fy, order)
    if recorded and order != (0, 0) and bicubic_recorded_exponents(dtype, fx, fy, order):
        return bicubic_recorded_exponents(dtype, fx, fy, order)[0]
    if key not in _TOP:
        lo, hi = 0, np.finfo(dtype).maxexp      # ok(lo): the integer lane itself; 2^maxexp is inf
        if order == (0, 0):
            assert bicubic_top_ok(dtype, fx, fy, lo), key
        elif not bicubic_top_ok(dtype, fx, fy, lo, order):
            hi = 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if bicubic_top_ok(dtype, fx, fy, mid, order) else (lo, mid)
        _TOP[key] = lo
    return _TOP[key]


def bicubic_top_ok(dtype, fx, fy, e, order=(0, 0)):
    return all(_top_ok(dtype, fx, fy, e, nx, ny, bc, order) for nx, ny in BICUBIC_GRIDS for bc in bicubic_ends())


def _top_ok(dtype, fx, fy, e, nx, ny, bc, order=(0, 0)):
    x, y = bicubic_grid(fx, fy, dtype, nx, ny)
    z = bicubic_lane("top scale", dtype, nx, ny, np.random.default_rng([0, nx, ny, 7]), e)[:, :, None]
    qx, qy = bicubic_queries(x, y)
    tabs, rows = bicubic_reference(x, y, z, bc, qx, qy, order=order)
    return finite_share(*tabs) >= 0.9 and finite_share(rows) >= 0.9


def bicubic_integer_share(dtype, fx, fy, order, bc=None):
    """the smallest finite share, over the grids, of the integer lane's rows of `order` with the ends `bc`"""
    shares = []
    for nx, ny in BICUBIC_GRIDS:
        x, y = bicubic_grid(fx, fy, dtype, nx, ny)
        z = bicubic_lane("integers", dtype, nx, ny, np.random.default_rng([0, nx, ny, 0]))[:, :, None]
        shares.append(finite_share(bicubic_reference(x, y, z, bc, *bicubic_queries(x, y), order=order)[1]))
    return min(shares)


def bicubic_integer_overflows(dtype, bc=None):
    """{(fx, fy, order): share}: the cases in which the integer lane's rows of a partial derivative are less than 90 % finite
    on a grid, with the smallest share.  Genuine overflows of the contract's arithmetic, not defects."""
    import bicubic_partial_ref
    out = {}
    for fx, fy in bicubic_partial_pairs(dtype):
        for order in bicubic_partial_ref.ORDERS:
            share = bicubic_integer_share(dtype, fx, fy, order, bc)
            if share < 0.9:
                out[fx, fy, order] = round(share, 2)
    return out


def subnormal_count(a):
    return int(np.count_nonzero((a != 0) & (np.abs(a) < np.finfo(a.dtype).tiny)))


def changed_rows(a, b):
    """the number of rows (first axis) in which a and b differ in what check_bits compares"""
    same = ((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))
    return int(np.count_nonzero(~same.reshape(len(a), -1).all(axis=1)))


def bicubic_sub_scan(dtype, fx, fy, order, exps, grids=BICUBIC_GRIDS, thin=1):
    """For every exponent e of `exps`: (subnormal non-zero rows of `order`, rows a flush to zero changes), each with one
    column per grid of `grids`, for the subnormal recipe's integers times 2^e as one lane, default ends.  All exponents go
    through the restatement at once, as lanes of one array.  `thin`: every thin-th query only (the search)."""
    import bicubic_partial_ref
    T = np.dtype(dtype).type
    exps = np.asarray(exps)
    sub, changed = [], []
    for nx, ny in grids:
        x, y = bicubic_grid(fx, fy, dtype, nx, ny)
        ints = bicubic_lane("integers", dtype, nx, ny, np.random.default_rng([0, nx, ny, 1]))
        with np.errstate(over="ignore"):
            z = (ints[:, :, None] * np.ldexp(T(1), exps)[None, None, :]).astype(dtype)
        qx, qy = bicubic_queries(x, y, n_random=300)
        qx, qy = qx[::thin], qy[::thin]
        tabs, rows = bicubic_reference(x, y, z, None, qx, qy, order=order)
        _, flushed = bicubic_reference(x, y, z, None, qx, qy, tabs=tabs, order=order, variant=bicubic_partial_ref.FLUSHED)
        sub.append(np.count_nonzero((rows != 0) & (np.abs(rows) < np.finfo(dtype).tiny), axis=0))
        same = ((rows == flushed) & (np.signbit(rows) == np.signbit(flushed))) | (np.isnan(rows) & np.isnan(flushed))
        changed.append(np.count_nonzero(~same, axis=0))
    return np.stack(sub, 1), np.stack(changed, 1)


def bicubic_sub_range(dtype):
    """the exponents at which integers 1 .. 4 times 2^e are non-zero and finite"""
    f = np.finfo(dtype)
    return f.minexp - f.nmant, f.maxexp - 3


SUB_STEP = 4


def bicubic_sub_exponent(dtype, fx, fy, order, recorded=True):
    """The exponent e for which integers times 2^e give the most subnormal, non-zero rows of the partial derivative `order`,
    pooled over both grids with the default ends -- found by search, not guessed.  The count is not monotone in e (rows
    underflow to zero below a window, are normal above it, and the build's products underflow before its quotients do), so
    the whole range in which the scaled integers are non-zero is scanned: every 4th exponent on a third of the queries of
    the small grid and a ninth of the large one's, then every exponent within 4 of the best.  The rows of a derivative are
    node differences divided by spacings, so the best e moves with the knot families by hundreds; it may make the nodes
    themselves subnormal, which puts subnormal operands into kl * h and pr - pl.  An exponent at which a flush to zero
    (bicubic_partial_ref.FLUSHED) changes a row on every grid goes before one at which it does not; ties in the count go to
    the exponent at which the flush changes more rows, then to the smaller one: where no exponent gives a subnormal row (the
    rows would need nodes below the smallest subnormal) the lane is the one whose operands a flush changes most.  Where the
    two stages find no exponent at which the flush changes a row on every grid, every exponent of the range is tried."""
    key = (np.dtype(dtype), fx, fy, tuple(order))
    if recorded and bicubic_recorded_exponents(dtype, fx, fy, order):
        return bicubic_recorded_exponents(dtype, fx, fy, order)[1]
    if key not in _SUB:
        lo, hi = bicubic_sub_range(dtype)

        def scan(exps):
            best = None
            for thin, grids in ((3, BICUBIC_GRIDS[:1]), (9, BICUBIC_GRIDS[1:])):
                r = bicubic_sub_scan(dtype, fx, fy, order, exps, grids, thin)
                sub, changed = (r[0], r[1]) if thin == 3 else (np.concatenate([sub, r[0]], 1), np.concatenate([changed, r[1]], 1))
            for k, e in enumerate(exps):
                cand = (bool(np.all(changed[k] > 0)), int(sub[k].sum()), int(changed[k].sum()), -int(e))
                best = cand if best is None or cand > best else best
            return best
        best = scan(np.arange(lo, hi + 1, SUB_STEP))
        best = scan(np.arange(max(lo, -best[3] - SUB_STEP), min(hi, -best[3] + SUB_STEP) + 1))
        if not best[0]:
            best = scan(np.arange(lo, hi + 1))
        _SUB[key] = -best[3]
    return _SUB[key]


# ---- Bicubic with periodic axes: hostile grids and wrapped queries (tests/test_gpu_bicubic_periodic_hostile.py and
# tests/test_gpu_bicubic_periodic_plans.py; self-check in tests/test_hostile_inputs.py) ----------------------------------------
PERIODIC_AXES = {"x": 1, "y": 2, "xy": 3}
SEAM_LANE = "+0 / -0 seam"
WRAP_PERIODS = (1, 2, 3, 1000, 2**20)


def bicubic_wrap_axis_queries(k):
    """The hostile queries of one wrapping axis, p = kn - k0 (every operation in k's dtype): every knot and the float either
    side of it -- not clipped, so one ulp outside either end is a query; every knot shifted by m p, m in -2, -1, 1, 2;
    k0 - m p and kn + m p and the float either side of each for m in 1, 2, 3, 1000, 2^20; k0 less the smallest normal and
    less the smallest subnormal (a tiny negative remainder: r + |p| rounds to p); +-max, max / 4, +-1e30."""
    T = k.dtype.type
    f = np.finfo(k.dtype)
    lo, hi = T(-np.inf), T(np.inf)
    k0, kn = k[0], k[-1]
    p = kn - k0
    q = [k, np.nextafter(k, lo), np.nextafter(k, hi)]
    q += [k + T(m) * p for m in (-2, -1, 1, 2)]
    far = np.array([e for m in WRAP_PERIODS for e in (k0 - T(m) * p, kn + T(m) * p)], k.dtype)
    q += [far, np.nextafter(far, lo), np.nextafter(far, hi)]
    q.append(np.array([k0 - f.tiny, k0 - f.smallest_subnormal, f.max, -f.max, f.max / T(4), 1e30, -1e30], k.dtype))
    q = np.concatenate(q).astype(k.dtype)
    assert np.all(np.isfinite(q))
    return q


def bicubic_periodic_queries(x, y, axes, seed=0, n_random=300):
    """(qx, qy) for a handle that wraps on `axes` (bit 0: x, bit 1: y): the cross product of bicubic_wrap_axis_queries on a
    wrapping axis and bicubic_axis_queries (in range) on the other, then `n_random` points up to 3.5 periods outside on a
    wrapping axis and in range on the other."""
    ax = bicubic_wrap_axis_queries(x) if axes & 1 else bicubic_axis_queries(x)
    ay = bicubic_wrap_axis_queries(y) if axes & 2 else bicubic_axis_queries(y)
    gx, gy = np.meshgrid(ax, ay, indexing="ij")
    rng = np.random.default_rng([seed, len(x), len(y), axes])

    def draws(k, wraps):
        p = k[-1] - k[0]
        u = rng.uniform(-3.5 if wraps else 0.0, 4.5 if wraps else 1.0, n_random).astype(k.dtype)
        r = (k[0] + u * p).astype(k.dtype)
        return r if wraps else np.clip(r, k[0], k[-1])
    return np.concatenate([gx.ravel(), draws(x, axes & 1)]), np.concatenate([gy.ravel(), draws(y, axes & 2)])


def bicubic_periodic_ends(axes, mixed):
    """the four ends of a periodic case: not-a-knot (not read) on a periodic axis, the default or MIXED_BC's on the other"""
    import bicubic_ref
    bc = list(bicubic_ref.MIXED_BC if mixed else bicubic_ref.DEFAULT_BC)
    if axes & 1:
        bc[0] = bc[1] = bicubic_ref.NOT_A_KNOT
    if axes & 2:
        bc[2] = bc[3] = bicubic_ref.NOT_A_KNOT
    return tuple(bc)


def bicubic_periodic_cases(dtype, grid_index):
    """(fx, fy, axes, mixed) for every pair of bicubic_pairs: the periodic-axes setting cycles x, y, xy over the pairs (one
    step on for the second grid), the other axis takes the default ends on even pairs and MIXED_BC's on odd ones."""
    names = tuple(PERIODIC_AXES)
    return [(fx, fy, names[(i + grid_index) % 3], i % 2 == 1) for i, (fx, fy) in enumerate(bicubic_pairs(dtype))]


def bicubic_periodic_parts(C):
    return -(-len(BICUBIC_RECIPES) // (C - 1))


def bicubic_periodic_nodes(dtype, nx, ny, C, axes, part=0, top_exp=0, seed=0, finite_only=False):
    """(z, names): z (nx, ny, C), periodic along `axes`.  Lanes 0 .. C - 2 are bicubic_nodes' (recipe
    (part * (C - 1) + l) mod 9, the same lane as there) followed by make_periodic: the last row / column repeats the first.  A
    planted NaN that this leaves on a seam row or column moves one node inwards (a NaN on the seam is a refusal, not a
    case).  Lane C - 1 is the seam lane: the integer background made periodic, then +0 in the first row and -0 in the last
    along each periodic axis -- equal under ==, so the build accepts it, and not the same bits."""
    import bicubic_periodic_ref
    z = np.empty((nx, ny, C), dtype)
    names = []
    for l in range(C - 1):
        r = (part * (C - 1) + l) % len(BICUBIC_RECIPES)
        rng = np.random.default_rng([seed, nx, ny, r])
        if finite_only and r in BICUBIC_NONFINITE:
            r = 0
        names.append(BICUBIC_RECIPES[r])
        z[:, :, l] = bicubic_lane(r, dtype, nx, ny, rng, top_exp)
    z[:, :, C - 1] = bicubic_lane("integers", dtype, nx, ny, np.random.default_rng([seed, nx, ny, len(BICUBIC_RECIPES)]))
    names.append(SEAM_LANE)
    for i, j, l in np.argwhere(np.isnan(z)):      # NaN off the seam: swapped with the node one step inwards, then the copy
        i2 = min(max(i, 1), nx - 2) if axes & 1 else i
        j2 = min(max(j, 1), ny - 2) if axes & 2 else j
        z[i, j, l], z[i2, j2, l] = z[i2, j2, l], z[i, j, l]
    z = bicubic_periodic_ref.make_periodic(z, axes)
    s = z[:, :, C - 1]
    if axes & 1:
        s[0], s[-1] = 0.0, -0.0
    if axes & 2:
        s[:, 0], s[:, -1] = 0.0, -0.0
    return z, names


def bicubic_periodic_reference(x, y, z, bc, axes, qx=None, qy=None, tabs=None, wrap=True, order=(0, 0)):
    """(tables, rows) of the periodic restatement (tests/bicubic_periodic_ref.py) with numpy's warnings off.  `tabs`: evaluate
    on these tables; `wrap=False`: the handle built without extrapolate, which does not wrap."""
    import bicubic_periodic_ref
    with np.errstate(all="ignore"):
        if tabs is None:
            tabs = bicubic_periodic_ref.tables(x, y, z, bc, axes)
        if qx is None:
            return tabs, None
        return tabs, bicubic_periodic_ref.evaluate_partial(x, y, z, *tabs, qx, qy, order[0], order[1], axes if wrap else 0)


def bicubic_periodic_recorded(dtype, fx, fy, axes):
    """tests/golden/bicubic_periodic_exponents.json: what bicubic_periodic_top_exponent found, recorded so that the device
    tests do not search again; tests/test_hostile_inputs.py runs every search and holds the file to the results."""
    import json
    import os
    if "periodic" not in _SEARCH:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicubic_periodic_exponents.json")) as f:
            _SEARCH["periodic"] = json.load(f)
    return _SEARCH["periodic"].get(np.dtype(dtype).name, {}).get(f"{fx} {fy}", {}).get(axes)


def bicubic_periodic_top_ok(dtype, fx, fy, axes, e):
    """integers times 2^e: the periodic restatement's three tables and its rows on the hostile wrapped queries are ALL finite,
    on both grids and with both end sets of the other axis"""
    a = PERIODIC_AXES[axes]
    for nx, ny in BICUBIC_GRIDS:
        x, y = bicubic_grid(fx, fy, dtype, nx, ny)
        import bicubic_periodic_ref
        z = bicubic_periodic_ref.make_periodic(
            bicubic_lane("top scale", dtype, nx, ny, np.random.default_rng([0, nx, ny, 7]), e)[:, :, None], a)
        qx, qy = bicubic_periodic_queries(x, y, a)
        for mixed in (False, True):
            try:
                tabs, rows = bicubic_periodic_reference(x, y, z, bicubic_periodic_ends(a, mixed), a, qx, qy)
            except ValueError:       # zx overflowed to NaN on the seam of y: the cross pass refuses it, as the build would
                return False
            if not (all(np.isfinite(t).all() for t in tabs) and np.isfinite(rows).all()):
                return False
    return True


def bicubic_periodic_top_exponent(dtype, fx, fy, axes, recorded=True):
    """bicubic_top_exponent for a build periodic along `axes` ("x", "y", "xy") whose handle wraps: the largest e, in steps
    of one, at which bicubic_periodic_top_ok holds -- measured on the restatement alone, never on a device.  The exponents
    of bicubic_top_exponent were found for not-a-knot builds and in-range queries at a 90 % finite share; the cyclic system
    and the end cells under wrapped queries overflow earlier on some pairs.  Bisection, as there."""
    if recorded and bicubic_periodic_recorded(dtype, fx, fy, axes) is not None:
        return bicubic_periodic_recorded(dtype, fx, fy, axes)
    key = (np.dtype(dtype), fx, fy, axes)
    if key not in _TOP:
        lo, hi = 0, np.finfo(dtype).maxexp
        assert bicubic_periodic_top_ok(dtype, fx, fy, axes, lo), key
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if bicubic_periodic_top_ok(dtype, fx, fy, axes, mid) else (lo, mid)
        _TOP[key] = lo
    return _TOP[key]


# ---- a query per lane (tests/test_gpu_lanewise2d_hostile.py; self-check in tests/test_hostile_inputs.py) -----------------------
def lanewise_arrangement(qx, qy, L, s=None):
    """(xs, ys, s): the query list (qx, qy) of length N as (N, L) arrays for a call with a query per lane: lane l holds the
    list rotated by l s, s prime to N (by default the first such s from N // L up, so the lanes start about evenly spread over
    the list).  Every lane meets every query exactly once -- its reference elements are a permutation of that lane's column of
    the row-wise reference -- and the lanes of a row sit s list positions apart, in different cells wherever the list moves."""
    N = len(qx)
    assert N >= 1 and len(qy) == N and L >= 1
    if s is None:
        s = max(1, N // L)
        while np.gcd(s, N) != 1:
            s += 1
    assert np.gcd(s, N) == 1, (s, N)
    at = (np.arange(N)[:, None] + s * np.arange(L)[None, :]) % N
    return np.ascontiguousarray(qx[at]), np.ascontiguousarray(qy[at]), s


def bicubic_lanewise_reference(x, y, z, bc, xs, ys, tabs, order=(0, 0), periodic=None, wrap=True):
    """(N, L): column l is the restatement's lane l on the queries (xs[:, l], ys[:, l]), evaluated on the tables `tabs` --
    bicubic_reference, or bicubic_periodic_reference for a build periodic along `periodic` (a bit set)."""
    N, L = xs.shape
    assert z.shape[2] == L
    out = np.empty((N, L), z.dtype)
    for l in range(L):
        one = tuple(np.ascontiguousarray(t[:, :, l:l + 1]) for t in tabs)
        zl = np.ascontiguousarray(z[:, :, l:l + 1])
        qx, qy = np.ascontiguousarray(xs[:, l]), np.ascontiguousarray(ys[:, l])
        if periodic:
            out[:, l] = bicubic_periodic_reference(x, y, zl, bc, periodic, qx, qy, tabs=one, wrap=wrap, order=order)[1][:, 0]
        else:
            out[:, l] = bicubic_reference(x, y, zl, bc, qx, qy, tabs=one, order=order)[1][:, 0]
    return out


LANEWISE_THIN = 11      # every 11th pair of the cross product: 11 is prime to the length of every y set of BICUBIC_GRIDS (19 .. 39)


def bicubic_lanewise_queries(x, y, extrapolate, L):
    """(xs, ys) of shape (N, L): bicubic_queries with every LANEWISE_THIN-th pair of the cross product (every point of either
    axis' set still occurs) and all its spread points, arranged by lanewise_arrangement."""
    qx, qy = bicubic_queries(x, y, extrapolate, thin=LANEWISE_THIN)
    return lanewise_arrangement(qx, qy, L)[:2]


def bicubic_lanewise_recorded(dtype, fx, fy, order=(0, 0)):
    """tests/golden/bicubic_lanewise_exponents.json: what bicubic_lanewise_top_exponent (order (0, 0)) and
    bicubic_lanewise_partial_top_exponent (LANEWISE_PARTIAL_ORDERS) found, recorded so that the device tests do not search
    again; tests/test_hostile_inputs.py runs every search and holds the file to the results.  The file is a held record of
    EVERY pair and order, also where the exponent is the row-wise one (most of them): the two functions return the recorded
    value before they consult bicubic_top_exponent, so the self-check is what ties the file to it."""
    import json
    import os
    if "lanewise" not in _SEARCH:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bicubic_lanewise_exponents.json")) as f:
            _SEARCH["lanewise"] = json.load(f)
    return _SEARCH["lanewise"].get(np.dtype(dtype).name, {}).get(f"{fx} {fy}", {}).get(f"{order[0]},{order[1]}")


def bicubic_lanewise_top_ok(dtype, fx, fy, e):
    """integers times 2^e: tables and rows of the restatement are at least 90 % finite on the query lists of
    bicubic_lanewise_queries -- in range and with extrapolation -- on both grids and with both end sets.  (A lane of the
    arrangement holds a permutation of the list, so the share of a lane is the share of the list.)"""
    for nx, ny in BICUBIC_GRIDS:
        x, y = bicubic_grid(fx, fy, dtype, nx, ny)
        z = bicubic_lane("top scale", dtype, nx, ny, np.random.default_rng([0, nx, ny, 7]), e)[:, :, None]
        for bc in bicubic_ends():
            for ext in (False, True):
                qx, qy = bicubic_queries(x, y, ext, thin=LANEWISE_THIN)
                tabs, rows = bicubic_reference(x, y, z, bc, qx, qy)
                if finite_share(*tabs) < 0.9 or finite_share(rows) < 0.9:
                    return False
    return True


def bicubic_lanewise_top_exponent(dtype, fx, fy, recorded=True):
    """The exponent of the "top scale" lane in the lane-wise tests: bicubic_top_exponent where bicubic_lanewise_top_ok holds
    for it, else the largest smaller e for which it does (bisection, as there: what overflows at e overflows at e + 1).  The
    row-wise exponent was found on the whole cross product in range; the thinned list has a larger share of spread points,
    which fall into the wide cells of a mixed axis, and the extrapolating list reaches 2^20 widths outside."""
    if recorded and bicubic_lanewise_recorded(dtype, fx, fy) is not None:
        return bicubic_lanewise_recorded(dtype, fx, fy)
    key = (np.dtype(dtype), fx, fy, "lanewise")
    if key not in _TOP:
        hi = bicubic_top_exponent(dtype, fx, fy)
        if bicubic_lanewise_top_ok(dtype, fx, fy, hi):
            _TOP[key] = hi
        else:
            lo = 0
            assert bicubic_lanewise_top_ok(dtype, fx, fy, lo), key
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if bicubic_lanewise_top_ok(dtype, fx, fy, mid) else (lo, mid)
            _TOP[key] = lo
    return _TOP[key]


LANEWISE_PARTIAL_ORDERS = ((1, 1), (2, 0), (0, 2))      # the orders tests/test_gpu_lanewise2d_hostile.py runs on the partial arrays


def bicubic_lanewise_shares(dtype, fx, fy, order, z_of):
    """the finite shares of the tables and of the rows of `order`, for the single lane z_of(nx, ny), on every list of
    bicubic_lanewise_queries: both grids, in range and with extrapolation, default ends (the partial cases build those)"""
    out = []
    for nx, ny in BICUBIC_GRIDS:
        x, y = bicubic_grid(fx, fy, dtype, nx, ny)
        z = z_of(nx, ny)[:, :, None]
        for ext in (False, True):
            qx, qy = bicubic_queries(x, y, ext, thin=LANEWISE_THIN)
            tabs, rows = bicubic_reference(x, y, z, None, qx, qy, order=order)
            out.append((finite_share(*tabs), finite_share(rows)))
    return out


def bicubic_lanewise_integer_share(dtype, fx, fy, order):
    """the smallest finite share of the integer lane's rows of `order` over those lists"""
    return min(s[1] for s in bicubic_lanewise_shares(
        dtype, fx, fy, order, lambda nx, ny: bicubic_lane("integers", dtype, nx, ny, np.random.default_rng([0, nx, ny, 0]))))


def bicubic_lanewise_partial_top_ok(dtype, fx, fy, order, e):
    return all(min(s) >= 0.9 for s in bicubic_lanewise_shares(
        dtype, fx, fy, order, lambda nx, ny: bicubic_lane("top scale", dtype, nx, ny, np.random.default_rng([0, nx, ny, 7]), e)))


def bicubic_lanewise_partial_top_exponent(dtype, fx, fy, order, recorded=True):
    """The exponent of the ("top scale", order) lane in the lane-wise tests of the partial orders: bicubic_top_exponent of
    that order where bicubic_lanewise_partial_top_ok holds for it, else the largest smaller e for which it does (bisection,
    as there); 0 where not even the integers pass (the row-wise case of bicubic_integer_overflows: the lane repeats the
    integers and claims nothing)."""
    order = tuple(order)
    if recorded and bicubic_lanewise_recorded(dtype, fx, fy, order) is not None:
        return bicubic_lanewise_recorded(dtype, fx, fy, order)
    key = (np.dtype(dtype), fx, fy, order, "lanewise")
    if key not in _TOP:
        hi = bicubic_top_exponent(dtype, fx, fy, order)
        if bicubic_lanewise_partial_top_ok(dtype, fx, fy, order, hi):
            _TOP[key] = hi
        elif not bicubic_lanewise_partial_top_ok(dtype, fx, fy, order, 0):
            _TOP[key] = 0
        else:
            lo = 0
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if bicubic_lanewise_partial_top_ok(dtype, fx, fy, order, mid) else (lo, mid)
            _TOP[key] = lo
    return _TOP[key]


def bicubic_lanewise_partial_nodes(dtype, nx, ny, fx, fy, C=25, seed=0, finite_only=False):
    """bicubic_partial_nodes with the top-scale lanes of the lane-wise tests: the ("top scale", order) lane of each order of
    LANEWISE_PARTIAL_ORDERS at bicubic_lanewise_partial_top_exponent, and the ("top scale", (0, 0)) lane at
    bicubic_lanewise_top_exponent where the pair is one of bicubic_pairs.  Every other lane is that function's."""
    z, lanes = bicubic_partial_nodes(dtype, nx, ny, fx, fy, C, seed, finite_only)
    T = np.dtype(dtype).type
    for l, (name, order) in enumerate(lanes):
        if name != "top scale":
            continue
        if order in LANEWISE_PARTIAL_ORDERS:
            e = bicubic_lanewise_partial_top_exponent(dtype, fx, fy, order)
        elif order == (0, 0) and (fx, fy) in bicubic_pairs(dtype):
            e = bicubic_lanewise_top_exponent(dtype, fx, fy)
        else:
            continue
        ints = bicubic_lane("integers", dtype, nx, ny, np.random.default_rng([seed, nx, ny, BICUBIC_RECIPES.index("top scale")]))
        with np.errstate(over="ignore"):
            z[:, :, l] = (ints * np.ldexp(T(1), e)).astype(dtype)
    return z, lanes


# ---- Trilinear: the edges of the division window and hostile axes (tests/test_gpu_trilinear_hostile.py; self-check in
# tests/test_hostile_inputs.py) ---------------------------------------------------------------------------------------------
# The exponent window of the shared-divisor division, restated from the comment above DivWindow in csrc/kernels.hpp: the
# reciprocal path is taken when the divisor lies in [D_LO, D_HI], the smallest numerator magnitude of a vector is >= N_LO
# and the sum of the vector's magnitudes is <= N_HI; everything else is the IEEE division.
TRILINEAR_WINDOW = {np.dtype(np.float32): dict(N_LO=-60, N_HI=60, D_LO=-40, D_HI=40),
                    np.dtype(np.float64): dict(N_LO=-500, N_HI=500, D_LO=-400, D_HI=400)}
TRILINEAR_WINDOW_TABLES = ("low edge", "sum edge", "scalar edge")
TRILINEAR_WINDOW_AXES = ("plain", "low divisor", "high divisor")
TRILINEAR_LANES = 8


def trilinear_window(dtype):
    """{N_LO, N_HI, D_LO, D_HI} as values of `dtype`"""
    T = np.dtype(dtype).type
    return {k: np.ldexp(T(1), e) for k, e in TRILINEAR_WINDOW[np.dtype(dtype)].items()}


def _prev(v):
    return np.nextafter(v, v.dtype.type(-np.inf))


def _next(v):
    return np.nextafter(v, v.dtype.type(np.inf))


def trilinear_lane_table(table, dtype):
    """(a, b): the two planted differences of each of the 8 lanes (two 16-byte vectors in f32, four in f64).
    low edge:    prev(N_LO), N_LO and next(N_LO) beside in-window lanes: one lane below the edge puts the whole vector on the
                 IEEE path, the lanes on and above it stay inside.
    sum edge:    with H = N_HI / (lanes of a vector): a vector of H alone (the sum is exactly N_HI: inside); the same with one
                 lane next(H) (the exact sum lies above N_HI and the sum as the kernel forms it rounds back to N_HI, ties to
                 even: inside); the same with one lane four floats above H (the rounded sum lies above N_HI: outside).
    scalar edge: N_HI and N_HI / 2 lanes, each inside on its own, in vectors whose sum is above N_HI; next(N_HI), outside in
                 either form; N_HI / 2 twice in an f64 vector (sum exactly N_HI).
    nonfinite:   (not one of the 27 finite cases) plain lanes; _trilinear_window_case then plants nodes of -+0.75 max in lanes
                 1 and 6, whose difference overflows: +inf and -inf as the lower numerator of one lane each, inside vectors
                 that are otherwise in the window -- only the sum test sends them to the IEEE division."""
    T = np.dtype(dtype).type
    W = 16 // np.dtype(dtype).itemsize
    w = trilinear_window(dtype)
    lo, hi = w["N_LO"], w["N_HI"]
    one = lambda *v: np.array(v, dtype)   # noqa: E731
    if table == "low edge":
        a = one(_prev(lo), 1.0, 3.0, 0.75, lo, _next(lo), 1.5, 2.0)
        b = np.roll(a, 4)
    elif table == "sum edge":
        H = hi / T(W)
        exact = [H] * W
        tie = [H] * (W - 1) + [_next(H)]
        above = [H] * (W - 1) + [H + T(4) * (_next(H) - H)]
        if W == 4:
            a, b = one(*exact, *tie), one(*above, *exact)
        else:
            a, b = one(*exact, *tie, *above, *exact), one(*above, *exact, *exact, *tie)
    elif table == "scalar edge":
        a = one(hi / T(2), hi / T(2), hi, lo, _next(hi), 1.0, 1.5, 2.0)
        b = one(1.0, 3.0, 0.75, 1.5, hi / T(2), hi / T(2), lo, lo)
    else:
        assert table == "nonfinite", table
        a = one(1.0, 3.0, 0.75, 1.5, 2.0, 1.25, 0.5, 1.0)
        b = one(1.5, 2.5, 2.0, 1.0, 3.0, 0.75, 0.25, 1.25)
    assert a.shape == b.shape == (TRILINEAR_LANES,)
    return a, b


def trilinear_plain_axis(dtype, seed):
    return np.cumsum(np.random.default_rng(4321 + seed).uniform(0.5, 1.5, 3)).astype(dtype)


def trilinear_window_axis(kind, dtype, seed=0):
    """Three knots whose two spacings are computed exactly: plain; [-prev(D_LO), 0, D_LO] (one float below the window, and
    its lower edge); [-next(D_HI), 0, D_HI] (one float above it, and its upper edge)."""
    w = trilinear_window(dtype)
    if kind == "plain":
        return trilinear_plain_axis(dtype, seed)
    if kind == "low divisor":
        return np.array([-_prev(w["D_LO"]), 0.0, w["D_LO"]], dtype)
    assert kind == "high divisor", kind
    return np.array([-_next(w["D_HI"]), 0.0, w["D_HI"]], dtype)


def _trilinear_window_case(dtype, vary, table, kind):
    a, b = trilinear_lane_table(table, dtype)
    col = np.stack([-a, np.zeros_like(a), b])                       # (3, 8): the column along the varying axis
    if table == "nonfinite":        # finite nodes whose difference overflows: the lower numerator of lanes 1 and 6 is +-inf
        big = np.dtype(dtype).type(0.75) * np.finfo(dtype).max
        col[:2, 1] = [-big, big]
        col[:2, 6] = [big, -big]
    shape = [1, 1, 1, TRILINEAR_LANES]
    shape[vary] = 3
    reps = [3, 3, 3, 1]
    reps[vary] = 1
    data = np.ascontiguousarray(np.tile(col.reshape(shape), reps))  # constant along the two other axes
    axes = [trilinear_window_axis(kind if ax == vary else "plain", dtype, seed=ax) for ax in range(3)]
    import trilinear_ref
    km = [trilinear_ref.knots_and_midpoints(k) for k in axes]
    q = [np.ascontiguousarray(g.ravel()) for g in np.meshgrid(*km, indexing="ij")]
    return dict(tag=f"{np.dtype(dtype).name} varying {'xyz'[vary]}, {table}, {kind} axis", vary=vary, table=table, kind=kind,
                axes=axes, data=data, q=q, a=a, b=b)


def trilinear_window_cases(dtype):
    """The 27 cases of one dtype: the varying axis (x, y, z: the division level whose numerators are planted) x the lane table
    x the kind of the varying axis.  3 x 3 x 3 x 8 data that varies along ONE axis, where its column is [-a, 0, b] per lane:
    both differences are exactly a and b, the calc_frac steps of the two other axes return y1 exactly (0 / d = 0,
    0 * t + y1 = y1), so (a, b) are the numerators of that level's division -- d100 - d000 for x, c10 - c00 for y, c1 - c0
    for z.  Queries: the full product of every axis' knots and midpoints, 125.  Each case is a dict: tag, vary, table, kind,
    axes, data, q, a, b."""
    for vary in range(3):
        for table in TRILINEAR_WINDOW_TABLES:
            for kind in TRILINEAR_WINDOW_AXES:
                yield _trilinear_window_case(dtype, vary, table, kind)


def trilinear_nonfinite_lane_cases(dtype):
    """Three cases more, one per varying axis on plain axes: the `nonfinite` lane table.  Their rows hold inf and NaN by
    construction, so they are no part of the all-finite claim of trilinear_window_cases."""
    for vary in range(3):
        yield _trilinear_window_case(dtype, vary, "nonfinite", "plain")


TRILINEAR_AXIS_KINDS = ("adjacent", "mixed", "huge", "minus zero", "infinite ends", "subnormal spacing")
_TRILINEAR_SUB_DATA = {np.dtype(np.float32): -50, np.dtype(np.float64): -60}


def trilinear_hostile_axis(kind, dtype):
    """Five knots: knots() of the kind; an axis with -0.0 as its middle knot; an axis with -inf and +inf as end knots; an axis
    whose spacing is three times the smallest subnormal (its reciprocal overflows: the divisor is far below the window)."""
    if kind == "minus zero":
        return np.array([-2.0, -0.75, -0.0, 1.0, 2.5], dtype)
    if kind == "infinite ends":
        return np.array([-np.inf, -1.0, 0.5, 2.0, np.inf], dtype)
    if kind == "subnormal spacing":
        return (np.array([-6, -3, 0, 3, 6], dtype) * np.finfo(dtype).smallest_subnormal).astype(dtype)
    return knots(kind, dtype, 5)


def trilinear_axis_queries(k, extrapolate):
    """One axis: every knot, every cell midpoint, the float either side of every interior knot; both zeros where a zero is a
    knot; with extrapolation one point a cell width below and one above.
    An axis with infinite end knots has no outside, and the reference's search cannot place a query strictly between infinite
    ends (its first guess is calc_frac over the whole axis: 0 * inf).  There the queries are the two end knots, which the
    reference places without a guess, and the points of the list that lie in [k[1], k[n-2]): the cells with finite knots on
    both sides, which trilinear_axis_reference evaluates on the finite part of the grid.  The queries inside the two end
    cells are left out."""
    T = k.dtype.type
    mid = ((k[:-1].astype(np.float64) + k[1:].astype(np.float64)) / 2).astype(k.dtype)
    q = [k, mid, np.nextafter(k[1:-1], T(-np.inf)), np.nextafter(k[1:-1], T(np.inf))]
    if np.any(k == 0):
        q.append(np.array([0.0, -0.0], k.dtype))
    if np.isinf(k[0]) or np.isinf(k[-1]):
        q = np.concatenate(q).astype(k.dtype)
        return np.concatenate([k[[0, -1]], q[(q >= k[1]) & (q < k[-2])]])
    if extrapolate:
        q.append(np.array([k[0] - (k[1] - k[0]), k[-1] + (k[-1] - k[-2])], k.dtype))
    return np.concatenate(q).astype(k.dtype)


def trilinear_axis_cases(dtype):
    """The 18 hostile-axis cases of one dtype: each of x, y, z in turn is one of TRILINEAR_AXIS_KINDS, the two others are
    knots("uneven") with a seed of their own; 5 x 5 x 5 x 4 uniform data in [-1, 1] (over the subnormal spacing: integers in
    [-4, 4] times 2^-50 / 2^-60 -- differences inside the numerator window whose slopes along that axis are finite, over a
    divisor whose reciprocal is not).  Each case is a dict: tag, hostile (the
    axis index), kind, axes, data, and q[extrapolate]: the full product of trilinear_axis_queries of the three axes."""
    for hostile in range(3):
        for kind in TRILINEAR_AXIS_KINDS:
            axes = [trilinear_hostile_axis(kind, dtype) if ax == hostile else knots("uneven", dtype, 5, seed=ax) for ax in range(3)]
            rng = np.random.default_rng([77, hostile, TRILINEAR_AXIS_KINDS.index(kind)])
            if kind == "subnormal spacing":
                data = np.ldexp(rng.integers(-4, 5, (5, 5, 5, 4)).astype(dtype), _TRILINEAR_SUB_DATA[np.dtype(dtype)]).astype(dtype)
            else:
                data = rng.uniform(-1, 1, (5, 5, 5, 4)).astype(dtype)
            q = {}
            for ext in (False, True):
                per = [trilinear_axis_queries(k, ext) for k in axes]
                q[ext] = [np.ascontiguousarray(g.ravel()) for g in np.meshgrid(*per, indexing="ij")]
            yield dict(tag=f"{np.dtype(dtype).name} {kind} on {'xyz'[hostile]}", hostile=hostile, kind=kind, axes=axes, data=data, q=q)


def trilinear_axis_reference(case, extrapolate, form=None):
    """(fail, axis, out) of tests/trilinear_ref.py (`form`: trilinear_ref by default, or trilinear_direct) for one case.  On
    an axis with infinite end knots the rows are the reference's in two parts: the queries on the end knots on the whole
    grid, and the queries in [k[1], k[n-2]) on the grid without its two end planes along that axis -- by the value rule
    (include/ndinterp3d.h) their cells have all eight corners there, and on that grid the reference's search works."""
    import trilinear_ref
    form = form or trilinear_ref.trilinear_ref
    axes, data, q, h = case["axes"], case["data"], case["q"][extrapolate], case["hostile"]
    if case["kind"] != "infinite ends":
        return form(*axes, data, *q, extrapolate)
    ends = np.isinf(q[h])
    out = np.zeros((q[0].size, data.shape[3]), data.dtype)
    fail, axis, rows = form(*axes, data, *[a[ends] for a in q], extrapolate)
    assert fail is None
    out[ends] = rows
    inner_axes = [k[1:-1] if ax == h else k for ax, k in enumerate(axes)]
    inner = np.ascontiguousarray(np.take(data, np.arange(1, data.shape[h] - 1), axis=h))
    fail, axis, rows = form(*inner_axes, inner, *[a[~ends] for a in q], extrapolate)
    assert fail is None
    out[~ends] = rows
    return None, None, out

