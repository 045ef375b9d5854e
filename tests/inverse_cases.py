"""The arrays of the inverse tests (ndi_interp1d_inverse), shared by the CPU tests (tests/test_inverse_ref.py), the GPU
tests (tests/test_gpu_inverse.py) and the generator of tests/golden/inverse_scipy.npz (tools/gen_inverse_golden.py): knots,
monotone data per source, the host-side tables of a source from the project's restatements, and queries.

Sources: "linear", "pchip", "akima", "spline" (natural; lane 0 is a step that the spline overshoots), "dpchip" (the
derivative handle of a Pchip on convex / concave data), "anti_pchip" and "anti_linear" (the antiderivative of non-negative
data with runs of zeros: flat runs in P).  Lanes alternate rising / falling where the source allows a common range for both
(an antiderivative starts at +0 in every lane, so its lanes all rise).  Increments are spread over four decades, about one
interval in six is flat, and every lane spans a little more than [-1, 1] (antiderivatives: [0, the smallest total]), so the
range common to all lanes is not empty.
"""
import numpy as np

import antiderivative_ref
import derivative_ref
import hermite_ref
import hostile_inputs
import inverse_ref
import oracle

SOURCES = ("linear", "pchip", "akima", "spline", "dpchip", "anti_pchip", "anti_linear")
CLASS_OF = {"linear": "linear", "pchip": "cubic", "akima": "cubic", "spline": "cubic", "dpchip": "cubic",
            "anti_pchip": "anti_cubic", "anti_linear": "anti_linear"}
# (n, lanes, Q): every n of {2, 3, 5, 257}, every lane count of {1, 3, 4, 64, 65} (rows that are and are not whole 16-byte
# groups; 64: one wavefront per row; 65: a row ends inside a wavefront) and every Q of {1, 63, 65, 4097} at least once
SHAPES = ((2, 1, 1), (3, 3, 63), (5, 4, 65), (257, 64, 4097), (257, 65, 63), (5, 1, 4097), (3, 65, 1), (257, 4, 65))
MIN_N = {"akima": 3, "spline": 3, "dpchip": 3}
# the shapes whose returned abscissae are evaluated forward again (the round trip): the cases of tests/golden/inverse_scipy.npz
TRIP_SHAPES = ((3, 3, 63), (5, 4, 65), (257, 4, 65))
# The restatement's worst |f_scipy(x) - v| / (eps_T max(|nl|, |nr|)) per (dtype, source) over tests/golden/inverse_scipy.npz,
# as tools/gen_inverse_golden.py measured and printed it; the tests allow 2 x each (the device does the identical
# arithmetic on other inputs).  DESIGN.md 4.18 repeats the table.
MEASURED = {
    ("float32", "akima"): 260.2,      # float32_akima_n257_L4
    ("float32", "anti_linear"): 4.166,      # float32_anti_linear_n257_L4
    ("float32", "anti_pchip"): 4.729,      # float32_anti_pchip_n257_L4
    ("float32", "dpchip"): 40.01,      # float32_dpchip_n257_L4
    ("float32", "linear"): 518.8,      # float32_linear_n257_L4
    ("float32", "pchip"): 531.3,      # float32_pchip_n257_L4
    ("float32", "spline"): 105.7,      # float32_spline_n257_L4
    ("float64", "akima"): 462.7,      # float64_akima_n257_L4
    ("float64", "anti_linear"): 9.897,      # float64_anti_linear_n3_L3
    ("float64", "anti_pchip"): 12.35,      # float64_anti_pchip_n257_L4
    ("float64", "dpchip"): 367.2,      # float64_dpchip_n257_L4
    ("float64", "linear"): 668,      # float64_linear_n257_L4
    ("float64", "pchip"): 307.2,      # float64_pchip_n257_L4
    ("float64", "spline"): 507.4,      # float64_spline_n257_L4
}
# the largest iteration count of the restatement over every array the GPU tests use (tests/test_inverse_ref.py asserts it
# and that it is below K = 128 / 64); DESIGN.md 4.18 states it
LARGEST_COUNT = {"float64": 58, "float32": 28}
HOSTILE_KNOTS = ("uneven", "adjacent", "mixed")
HOSTILE_DATA = ("subnormal", "offset", "infinite")


def shapes_of(source):
    return tuple(s for s in SHAPES if s[0] >= MIN_N.get(source, 2))


def knots(rng, n, dt):
    """uneven steps from 0, one in five of them twenty times shorter (clusters)"""
    step = rng.uniform(0.5, 2.0, n)
    step[rng.random(n) < 0.2] *= 0.05
    x = np.cumsum(step) - step[0]
    x = x.astype(dt)
    assert np.all(np.diff(x) > 0)
    return x


def _increments(rng, n, L, flat):
    """(n - 1, L) non-negative, over four decades, a share `flat` of them zero, at least one positive per lane"""
    inc = 10.0 ** rng.uniform(-4, 0, (n - 1, L))
    zero = rng.random((n - 1, L)) < flat
    zero[rng.integers(0, n - 1, L), np.arange(L)] = False
    return np.where(zero, 0.0, inc)


def _directions(L, mixed):
    return np.where((np.arange(L) % 2 == 1) & mixed, -1.0, 1.0)


def data(source, rng, x, L, dt):
    """y (n, L) of the source on the knots x"""
    n = len(x)
    x64 = x.astype(np.float64)
    if source in ("anti_pchip", "anti_linear"):
        y = 10.0 ** rng.uniform(-3, 0, (n, L))
        zero = rng.random((n, L)) < 0.3
        if n >= 5:
            zero[1:3, :] = True                      # a run of zeros: a zero interval, a flat run in P
        zero[0, :] = False
        return np.where(zero, 0.0, y).astype(dt)
    if source == "dpchip":
        # slopes rising from 0.1 to about 3 (convex data) or falling the same way (concave): the Pchip derivative at the
        # knots lies between neighbouring slopes, so the derivative handle's node table is monotone
        s = 0.1 + np.cumsum(10.0 ** rng.uniform(-2, 0, (n - 1, L)), axis=0)
        s = 0.1 + (s - 0.1) * (2.9 / (s[-1] - 0.1))
        s = np.where(_directions(L, True) > 0, s, s[::-1])
        y = np.concatenate([np.zeros((1, L)), np.cumsum(s * np.diff(x64)[:, None], axis=0)])
        return y.astype(dt)
    inc = _increments(rng, n, L, 1.0 / 6.0)
    if source == "spline" and n >= 5:
        inc[:, 0] = 0.0
        inc[(n - 1) // 2, 0] = 1.0                    # a step between two flat runs: the spline overshoots beside it
    c = np.concatenate([np.zeros((1, L)), np.cumsum(inc, axis=0)])
    pad0, pad1 = rng.uniform(0.0, 0.25, L), rng.uniform(0.0, 0.25, L)
    y = (-1.0 - pad0) + c / c[-1] * (2.0 + pad0 + pad1)
    return (y * _directions(L, True)).astype(dt)


def tables(source, x, y):
    """(cls, N, y, a, b) of the source from the project's restatements, in y's dtype: what inverse_ref.solve takes"""
    cls = CLASS_OF[source]
    if source == "linear":
        return cls, y, None, None, None
    if source == "anti_linear":
        return cls, antiderivative_ref.prefix(x, y), y, None, None
    if source == "spline":
        st, a, b = oracle.cubic_build(x, y, left=(oracle.BC_NATURAL, 0.0), right=(oracle.BC_NATURAL, 0.0))
        assert st == oracle.OK
    else:
        a, b = hermite_ref.build("akima" if source == "akima" else "pchip", x, y)
    if source == "dpchip":
        Y, A, B = derivative_ref.derive(x, y, a, b)
        return cls, Y, None, A, B
    if source == "anti_pchip":
        return cls, antiderivative_ref.prefix(x, y, a, b), y, a, b
    return cls, y, None, a, b


def queries(rng, N, Q):
    """Q values in the common range: Lo and Hi, node values and their neighbours one ulp inside, random values between"""
    dt = N.dtype
    lo, hi = inverse_ref.common_range(N)
    assert lo <= hi
    nodes = np.unique(N[(N >= lo) & (N <= hi)])
    if len(nodes) > Q // 4:
        nodes = rng.choice(nodes, max(Q // 4, 1), replace=False)
    near = np.concatenate([np.nextafter(nodes, dt.type(np.inf)), np.nextafter(nodes, dt.type(-np.inf))])
    special = np.concatenate([[hi, lo], nodes, near]).astype(dt)
    special = special[(special >= lo) & (special <= hi)][:Q]
    fill = rng.uniform(lo, hi, Q - len(special)).astype(dt)
    q = np.clip(np.concatenate([special, fill]), lo, hi).astype(dt)
    return np.ascontiguousarray(rng.permutation(q) if Q > 2 else q)


def case(source, dt, n, L, Q):
    """(x, y, q) of one seeded case; q from the host-side tables' node table"""
    rng = np.random.default_rng([SOURCES.index(source), n, L, Q, np.dtype(dt).itemsize])
    x = knots(rng, n, dt)
    y = data(source, rng, x, L, dt)
    return x, y, queries(rng, tables(source, x, y)[1], Q)


def hostile_sources(kind, recipe):
    """Linear and Pchip; the antiderivative only of the offset data on the uneven knots (elsewhere P underflows or
    overflows to a constant); the infinite nodes only under Linear (a Pchip of them has NaN tables, on which the
    iteration runs to its cap K -- it terminates, but the tests' arrays never reach K)"""
    if recipe == "infinite":
        return ("linear",)
    return ("linear", "pchip") + (("anti_pchip",) if (kind, recipe) == ("uneven", "offset") else ())


# ---- hostile monotone data (tests/hostile_inputs.py knots) ------------------------------------------------------------------
def hostile(kind, recipe, dt, n, L):
    """(x, y): y = base + m * unit with integer m, so every sum is exact and all lanes have the same two end values.
    subnormal: base 0, unit the smallest subnormal; offset: base 2^20 (f32: 2^10), unit its spacing; infinite: the offset
    data with the first node of lane 0 at -inf and of lane 1 at +inf (the start value in that interval is inf / inf: only
    the final min keeps the NaN out of x).  Lanes alternate rising / falling; the increments are a permutation of one
    multiset per lane (zeros among them)."""
    T = np.dtype(dt).type
    rng = np.random.default_rng([HOSTILE_KNOTS.index(kind), HOSTILE_DATA.index(recipe), n, L])
    x = hostile_inputs.knots(kind, dt, n)
    steps = np.concatenate([[0, 0, 1, 1, 2, 3, 5, 40], rng.integers(0, 1000, max(n - 1, 8))])[:n - 1] if n > 2 else np.array([7])
    if steps.sum() == 0:
        steps[0] = 3
    m = np.stack([np.concatenate([[0], np.cumsum(rng.permutation(steps))]) for _ in range(L)], axis=1)
    m = np.where(np.arange(L) % 2 == 1, m[-1] - m, m)
    if recipe == "subnormal":
        base, unit = T(0), np.nextafter(T(0), T(1))
    else:
        base = T(2.0 ** 20 if np.dtype(dt) == np.float64 else 2.0 ** 10)
        unit = np.spacing(base)
    y = (base + m.astype(dt) * unit).astype(dt)
    assert np.array_equal((y - base) / unit, m)
    if recipe == "infinite":
        y[0, 0] = -np.inf
        if L > 1:
            y[0, 1] = np.inf
    return x, y
