"""Test-side restatement of the inverse rule (include/ndinterp.h, ndi_interp1d_inverse): for values `v` the abscissa `x`
with `f_l(x) = v` per lane, in numpy, in exactly the operation order the header specifies -- the search over the node
values of the lane, the start value, the bracketed Newton iteration on the interval's polynomial in `t`, the finish.

Every line is one IEEE operation per element in the tables' own dtype T (numpy does not fuse; every operand is a T array
or a T scalar, which `solve` asserts), so the device kernel -- compiled without contraction, same order -- gives the same
bits.  `x`: (n,), `N`: (n, lanes) node table, `v`: (Q,).  Classes:
    "linear"       N = y                                   closed form
    "cubic"        N = y, tables a, b (n - 1, lanes)       Newton on the cubic evaluation's expression
    "anti_cubic"   N = P, the source's y, a, b             Newton on the antiderivative's quartic
    "anti_linear"  N = P, the source's y                   Newton on its quadratic
`solve` returns `(x, iterations)`, both (Q, lanes): `iterations` counts the evaluations of p(t) per element (0 where the
start value finishes: v == nl, Linear).  The elements are independent, so the iteration runs on all of them at once with
those that have stopped masked out.  `mutant` switches ONE rule off so that a test can show its arrays tell the variants
apart: "search_lt" (< for <= in the search), "no_shortcut" (no v == nl start), "no_eps_stop" (no |step| <= eps stop),
"no_min" (no final min).
"""
import numpy as np

K = {np.dtype(np.float64): 128, np.dtype(np.float32): 64}
EPS = {np.dtype(np.float64): np.float64(2.0 ** -52), np.dtype(np.float32): np.float32(2.0 ** -23)}
CLASSES = ("linear", "cubic", "anti_cubic", "anti_linear")
MUTANTS = ("search_lt", "no_shortcut", "no_eps_stop", "no_min")


def search(N, v, mutant=None):
    """(i, rising): the interval per element (Q, lanes) and the direction per lane"""
    n, L = N.shape
    Q = len(v)
    rising = N[n - 1] >= N[0]
    lane = np.broadcast_to(np.arange(L), (Q, L))
    V = np.broadcast_to(v[:, None], (Q, L))
    lo = np.zeros((Q, L), dtype=np.int64)
    hi = np.full((Q, L), n - 1, dtype=np.int64)
    while True:
        act = hi - lo > 1
        if not act.any():
            break
        mid = (lo + hi) >> 1
        cm = N[mid, lane]
        if mutant == "search_lt":
            pred = np.where(rising, cm < V, cm > V)
        else:
            pred = np.where(rising, cm <= V, cm >= V)
        lo = np.where(act & pred, mid, lo)
        hi = np.where(act & ~pred, mid, hi)
    return lo, rising


def _poly(cls, T, yl, yr, a, b, p0, dx):
    """(p, dp): the interval's polynomial in t as the forward evaluation forms it, and its derivative in t"""
    if cls == "cubic":
        dy = yr - yl
        d0 = dy + a
        e = b - (a + a)
        e2 = e + e
        g = T(3) * (b - a)

        def p(t, m):
            u = T(1) - t
            return (u * yl[m] + t * yr[m]) + (t * u) * (a[m] * u + b[m] * t)

        def dp(t, m):
            return d0[m] + t * (e2[m] - g[m] * t)
        return p, dp
    if cls == "anti_cubic":
        dy = yr - yl
        c1 = (dy + a) * T(0.5)
        c2 = (b - (a + a)) / T(3)
        c3 = (b - a) * T(0.25)

        def p(t, m):
            return p0[m] + dx[m] * (t * (yl[m] + t * (c1[m] + t * (c2[m] - t * c3[m]))))

        def dp(t, m):
            return dx[m] * (yl[m] + t * ((c1[m] + c1[m]) + t * (T(3) * c2[m] - (T(4) * c3[m]) * t)))
        return p, dp
    assert cls == "anti_linear"
    c1 = (yr - yl) * T(0.5)

    def p(t, m):
        return p0[m] + dx[m] * (t * (yl[m] + t * c1[m]))

    def dp(t, m):
        return dx[m] * (yl[m] + t * (c1[m] + c1[m]))
    return p, dp


def solve(cls, x, N, v, y=None, a=None, b=None, mutant=None, cap=None):
    """(x, iterations), both (Q, lanes).  `cap`: another iteration limit than K (a test's own)."""
    assert cls in CLASSES and mutant in (None,) + MUTANTS
    dt = N.dtype
    T = dt.type
    assert dt in K and x.dtype == dt and v.dtype == dt and N.ndim == 2 and len(x) == N.shape[0] >= 2 and v.ndim == 1
    for tab, rows in ((y, len(x)), (a, len(x) - 1), (b, len(x) - 1)):
        assert tab is None or (tab.dtype == dt and tab.shape == (rows, N.shape[1]))
    assert (a is None) == (cls in ("linear", "anti_linear")) and (y is None) == (cls in ("linear", "cubic"))
    Q, L = len(v), N.shape[1]
    i, rising = search(N, v, mutant)
    i, lane = i.reshape(-1), np.broadcast_to(np.arange(L), (Q, L)).reshape(-1)
    rising = np.broadcast_to(rising, (Q, L)).reshape(-1)
    V = np.broadcast_to(v[:, None], (Q, L)).reshape(-1)
    nl, nr = N[i, lane], N[i + 1, lane]
    xl, xr = x[i], x[i + 1]
    dx = xr - xl
    go = np.ones(Q * L, dtype=bool) if mutant == "no_shortcut" else ~(V == nl)
    with np.errstate(all="ignore"):
        t = np.where(go, (V - nl) / (nr - nl), T(0))
        iters = np.zeros(Q * L, dtype=np.int64)
        if cls != "linear":
            src = N if cls == "cubic" else y
            yl, yr = src[i, lane], src[i + 1, lane]
            ai = a[i, lane] if a is not None else None
            bi = b[i, lane] if b is not None else None
            p, dp = _poly(cls, T, yl, yr, ai, bi, nl, dx)
            tl, th, dprev = np.zeros(Q * L, dtype=dt), np.ones(Q * L, dtype=dt), np.ones(Q * L, dtype=dt)
            alive = np.nonzero(go)[0]
            for _ in range(K[dt] if cap is None else cap):
                if alive.size == 0:
                    break
                m = alive
                tm = t[m]
                f = p(tm, m) - V[m]
                iters[m] += 1
                run = ~(f == 0)
                m, tm, f = m[run], tm[run], f[run]
                below = np.where(rising[m], f < 0, f > 0)
                tl[m] = np.where(below, tm, tl[m])
                th[m] = np.where(below, th[m], tm)
                d = dp(tm, m)
                s = f / d
                tn = tm - s
                bisect = ~((tn > tl[m]) & (tn < th[m])) | ~(np.abs(s + s) <= np.abs(dprev[m]))
                tn = np.where(bisect, tl[m] + T(0.5) * (th[m] - tl[m]), tn)
                step = tn - tm
                dprev[m] = step
                t[m] = tn
                alive = m if mutant == "no_eps_stop" else m[~(np.abs(step) <= EPS[dt])]
        w = xl + t * dx
        if mutant != "no_min":
            w = np.where(w < xr, w, xr)
        out = np.where(t == 1, xr, w)
    assert out.dtype == dt and t.dtype == dt
    return out.reshape(Q, L), iters.reshape(Q, L)


def intervals(N, v):
    """(i, nl, nr) per element, (Q, lanes): the interval the contract's search takes and its node values"""
    i, _ = search(N, v)
    lane = np.broadcast_to(np.arange(N.shape[1]), i.shape)
    return i, N[i, lane], N[i + 1, lane]


def common_range(N):
    """(Lo, Hi): the value range common to all lanes, from the first and last rows of N"""
    lo = np.minimum(N[0], N[-1]).max()
    hi = np.maximum(N[0], N[-1]).min()
    return lo, hi
