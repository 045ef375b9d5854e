"""CPU: the numpy restatement of the inverse rule (tests/inverse_ref.py, what the GPU tests compare the device against bit
for bit) -- against scipy through tests/golden/inverse_scipy.npz (tools/gen_inverse_golden.py), its structural
properties, its iteration counts on every array the GPU tests use, and the mutants those arrays must tell apart."""
import os

import numpy as np
import pytest

import inverse_cases as ic
import inverse_ref as ir
from conftest import GOLDEN

DTYPES = [np.float64, np.float32]


def golden():
    return np.load(os.path.join(GOLDEN, "inverse_scipy.npz"))


def ppoly_eval(c, xk, X):
    """scipy's PPoly in f64 from ITS coefficients c (k, n - 1, lanes) on the knots xk: sum_j c[j] (x - xk[i])^(k-1-j), at
    X (Q, lanes), lane l of the polynomial at column l.  (A PPoly is continuous here, so the interval at a knot is free.)"""
    X = np.asarray(X, dtype=np.float64)
    i = np.clip(np.searchsorted(xk, X, side="right") - 1, 0, len(xk) - 2)
    lane = np.broadcast_to(np.arange(X.shape[1]), X.shape)
    s = X - xk[i]
    r = np.zeros_like(X)
    for j in range(c.shape[0]):
        r = r * s + c[j][i, lane]
    return r


def residual_ratio(c, x, N, q, X):
    """|f_scipy(x) - v| / (eps_T max(|nl|, |nr|)) per element; where the scale is zero the residual must be zero"""
    f = ppoly_eval(c, x.astype(np.float64), X)
    _, nl, nr = ir.intervals(N, q)
    scale = np.maximum(np.abs(nl), np.abs(nr)).astype(np.float64) * float(np.finfo(N.dtype).eps)
    err = np.abs(f - q[:, None].astype(np.float64))
    assert np.all(err[scale == 0] == 0)
    return np.where(scale == 0, 0.0, err / np.where(scale == 0, 1.0, scale))


# ---- agreement with scipy ---------------------------------------------------------------------------------------------
def test_golden_covers_the_cases_and_its_evaluation_is_scipys():
    g = golden()
    cases = list(g["cases"])
    assert len(cases) == 2 * 3 * len(ic.SOURCES)
    for cid in cases:
        x, y, q, c = (g[cid + "/" + k] for k in ("x", "y", "q", "c"))
        assert x.dtype == y.dtype == q.dtype and c.dtype == np.float64 and c.shape[1:] == (len(x) - 1, y.shape[1])
        dt, source = cid.split("_n")[0].split("_", 1)
        assert c.shape[0] == {"linear": 2, "dpchip": 3, "anti_linear": 3, "anti_pchip": 5}.get(source, 4)
        xc, fc = g[cid + "/xc"], g[cid + "/fc"]
        assert np.allclose(ppoly_eval(c, x.astype(np.float64), xc[:, None] * np.ones(y.shape[1])), fc, rtol=1e-12, atol=1e-300)
        x2, y2, q2 = ic.case(source, np.dtype(dt), len(x), y.shape[1], len(q))      # the file's arrays are inverse_cases'
        assert np.array_equal(x, x2) and np.array_equal(y, y2) and np.array_equal(q, q2)
    assert os.path.getsize(os.path.join(GOLDEN, "inverse_scipy.npz")) <= 640 * 1024


@pytest.mark.parametrize("dt,source", sorted(ic.MEASURED))
def test_residual_against_scipy(dt, source):
    """|f_scipy(x) - v| <= 2 x MEASURED x eps_T x max(|nl|, |nr|) for every x the restatement returns on the golden cases:
    f_scipy is scipy's f64 PPoly of the source.  |x - x_scipy| is NOT bounded: where f' -> 0 (Pchip's flat ends) the
    inverse is ill-conditioned by construction."""
    g = golden()
    m = ic.MEASURED[(dt, source)]
    assert abs(float(g[f"measured/{dt}/{source}"]) - m) <= 1e-3 * m
    worst, seen = 0.0, 0
    for cid in g["cases"]:
        if not cid.startswith(f"{dt}_{source}_n"):
            continue
        x, y, q, c = (g[cid + "/" + k] for k in ("x", "y", "q", "c"))
        cls, N, ys, a, b = ic.tables(source, x, y)
        X, iters = ir.solve(cls, x, N, q, ys, a, b)
        assert X.dtype == np.dtype(dt) and iters.max() < ir.K[np.dtype(dt)]
        r = float(residual_ratio(c, x, N, q, X).max())
        worst = max(worst, r)
        assert r <= 2.0 * m, (cid, r, 2.0 * m)
        seen += 1
    assert seen == 3
    print(f"{dt} {source}: largest |f_scipy(x) - v| / (eps max(|nl|, |nr|)) = {worst:.4g}, bound {2.0 * m:.4g}")


# ---- structure ---------------------------------------------------------------------------------------------------------
def gpu_arrays():
    """every (what, source, x, y, q) the GPU tests evaluate (tests/test_gpu_inverse.py), hostile ones included"""
    for dt in DTYPES:
        for source in ic.SOURCES:
            for n, L, Q in ic.shapes_of(source):
                yield (f"{source} {n} x {L} Q = {Q} {np.dtype(dt).name}", source) + ic.case(source, dt, n, L, Q)
        rng = np.random.default_rng(3)
        for kind in ic.HOSTILE_KNOTS:
            for recipe in ic.HOSTILE_DATA:
                for n, L, Q in ((33, 5, 257), (4, 4, 63)):
                    x, y = ic.hostile(kind, recipe, dt, n, L)
                    for source in ic.hostile_sources(kind, recipe):
                        yy = y if source != "anti_pchip" else np.abs(y[:, ::2])
                        q = ic.queries(rng, ic.tables(source, x, yy)[1], Q)
                        yield f"hostile {kind} {recipe} {source} {n} {np.dtype(dt).name}", source, x, yy, q


def test_structure_and_iteration_counts_on_the_gpu_arrays():
    """x in [xl, xr]; a query at a node returns the node, or the right end of its flat run (the left end of the LAST
    interval where the run reaches the last node); the iteration count stays below K.  The largest count goes to
    DESIGN.md 4.18."""
    most = {np.dtype(d): 0 for d in DTYPES}
    total = {np.dtype(d): [0, 0] for d in DTYPES}
    overshoot = runs = 0
    for what, source, x, y, q in gpu_arrays():
        cls, N, ys, a, b = ic.tables(source, x, y)
        X, iters = ir.solve(cls, x, N, q, ys, a, b)
        dt = N.dtype
        assert iters.max() < ir.K[dt], what
        most[dt] = max(most[dt], int(iters.max()))
        if cls != "linear":
            total[dt][0] += int(iters.sum()); total[dt][1] += iters.size
        i, nl, nr = ir.intervals(N, q)
        assert np.all((X >= x[i]) & (X <= x[i + 1])) and not np.isnan(X).any(), what
        n = len(x)
        at = q[:, None] == nl                                   # the search's interval starts at a node with this value
        assert np.all(X[at] == x[i][at]), what
        V = np.broadcast_to(q[:, None], i.shape)
        assert np.all((nr[at] != V[at]) | (i[at] == n - 2)), what          # ... and it is the run's last node
        lane = np.broadcast_to(np.arange(N.shape[1]), i.shape)
        runs += int((at & (i > 0) & (N[np.maximum(i - 1, 0), lane] == V)).sum())     # nodes hit at the end of a flat run
        hit_right = (q[:, None] == nr) & (i == n - 2) & ~at
        assert np.all(X[hit_right] == x[n - 1]), what
        if source == "spline" and n >= 5:                       # lane 0: a root exists although p leaves [nl, nr]
            t = np.linspace(0, 1, 33)[:, None]
            k = (n - 1) // 2 + 1                                # the flat interval right of the step
            yl, yr, ak, bk = (v.astype(np.float64) for v in (N[k, 0], N[k + 1, 0], a[k, 0], b[k, 0]))
            p = (1 - t) * yl + t * yr + t * (1 - t) * (ak * (1 - t) + bk * t)
            overshoot += int(p.max() > max(yl, yr) + 1e-3)
    assert overshoot >= 2 and runs >= 100
    for dt in most:
        print(f"{dt.name}: largest iteration count {most[dt]} (K = {ir.K[dt]}), mean over the Newton classes "
              f"{total[dt][0] / total[dt][1]:.2f}")
    assert most[np.dtype(np.float64)] == ic.LARGEST_COUNT["float64"] and most[np.dtype(np.float32)] == ic.LARGEST_COUNT["float32"]


# ---- mutants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ir.MUTANTS)
def test_the_gpu_arrays_tell_the_mutants_apart(mutant):
    """a restatement with one rule switched off returns other bits on at least one array the GPU tests compare"""
    caught = []
    for what, source, x, y, q in gpu_arrays():
        if len(q) > 300 and caught:
            continue
        cls, N, ys, a, b = ic.tables(source, x, y)
        if mutant == "no_eps_stop" and cls == "linear":
            continue
        X, _ = ir.solve(cls, x, N, q, ys, a, b)
        M, _ = ir.solve(cls, x, N, q, ys, a, b, mutant=mutant)
        same = (X.view(np.uint64 if X.itemsize == 8 else np.uint32) == M.view(np.uint64 if X.itemsize == 8 else np.uint32)) \
            | (np.isnan(X) & np.isnan(M))
        if not same.all():
            caught.append(what)
    print(f"{mutant}: told apart by {len(caught)} arrays, first {caught[:3]}")
    assert caught, mutant


def test_the_trailing_flat_run_needs_the_shortcut():
    """without `v == nl -> t = 0` the start value on a flat run that reaches the last node is 0 / 0"""
    for dt in DTYPES:
        x = np.arange(5).astype(dt)
        N = np.array([[0.0], [1.0], [2.0], [2.0], [2.0]], dtype=dt)
        a = b = np.zeros((4, 1), dtype=dt)
        v = np.array([2.0], dtype=dt)
        X, it = ir.solve("cubic", x, N, v, None, a, b)
        assert X[0, 0] == 3.0 and it[0, 0] == 0
        M, itm = ir.solve("cubic", x, N, v, None, a, b, mutant="no_shortcut")
        assert itm[0, 0] == ir.K[np.dtype(dt)] and M[0, 0] != 3.0          # t is NaN to the end: the cap, and another x
        assert ir.solve("linear", x, N, v)[0][0, 0] == 3.0
