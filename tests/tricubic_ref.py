"""Test-side restatement of the Tricubic contract (include/ndinterp3d_cubic.h) in numpy, in exactly the operation order the
header specifies and in the arrays' own dtype (the implementation never imports it).

The seven node-derivative tables come from `bicubic_ref.knot_derivatives` -- the Bicubic pass: the reference-order spline
build with the true not-a-knot right row, then the derivative rule's Y -- on reshaped / transposed columns; the evaluation
is the 21 Hermite forms `bicubic_ref.hermite`, z first, then y, then x.  Every line is one IEEE operation per element
(numpy does not fuse), so the device kernel -- compiled without contraction, same order -- gives the same bits.

`x`: (nx,), `y`: (ny,), `z`: (nz,), `f`: (nx, ny, nz, C), one float dtype.  `bc`: six (kind, value) pairs, x-left, x-right,
y-left, y-right, z-left, z-right.  The tables are (fx, fy, fz, fxy, fxz, fyz, fxyz), ndi_interp3d_tables' order.

Deliberately wrong variants, for the mutant tests (`variant=`):
  "fxyz_zero"     the triple cross table zeroed
  "fxyz_from_x"   fxyz derived as D_x of fyz instead of D_z of fxy (the passes are linear maps along different axes, so this
                  is the same table mathematically for every set of ends: it differs in rounding only, in most entries)
  "x_first"       the 21 forms evaluated x first, then y, then z (the same polynomial, other roundings)
and `side="left"`: the wrong search (a query on a knot falls into the cell below; a Hermite patch gives the node value from
either side, so on finite tables only the cell differs, and with it the nodes that reach the row)."""
import numpy as np

import bicubic_ref
import oracle
from bicubic_ref import hermite
from trilinear_ref import bits, first_failure  # noqa: F401  (re-exported for the tests)

NOT_A_KNOT = bicubic_ref.NOT_A_KNOT
DEFAULT_BC = (NOT_A_KNOT,) * 6
# one end condition of every other kind, a non-zero end value on each axis: the second end set of the Tricubic tests
MIXED_BC = ((oracle.BC_NATURAL, 0.0), (oracle.BC_FIRST_DERIV, 0.75), (oracle.BC_SECOND_DERIV, -0.5), (oracle.BC_CLAMPED, 0.0),
            (oracle.BC_FIRST_DERIV, -1.25), (oracle.BC_NOT_A_KNOT, 0.0))


def derive(k, g, axis, left, right):
    """D_axis g: the knot derivatives of the 1-D splines through g (nx, ny, nz, C) along `axis`, of g's shape."""
    moved = np.ascontiguousarray(np.moveaxis(g, axis, 0))
    cols = moved.reshape(moved.shape[0], -1)
    with np.errstate(all="ignore"):      # hostile data overflow on purpose
        out = bicubic_ref.knot_derivatives(k, cols, left, right).reshape(moved.shape)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def tables(x, y, z, f, bc=DEFAULT_BC, variant=None):
    """(fx, fy, fz, fxy, fxz, fyz, fxyz), each of f's shape."""
    assert x.dtype == y.dtype == z.dtype == f.dtype and f.shape[:3] == (len(x), len(y), len(z)) and f.ndim == 4
    zero = lambda e: (e[0], 0.0)   # noqa: E731  a pass on a derivative table: the same end kinds with value 0
    fx = derive(x, f, 0, bc[0], bc[1])
    fy = derive(y, f, 1, bc[2], bc[3])
    fz = derive(z, f, 2, bc[4], bc[5])
    fxy = derive(y, fx, 1, zero(bc[2]), zero(bc[3]))
    fxz = derive(z, fx, 2, zero(bc[4]), zero(bc[5]))
    fyz = derive(z, fy, 2, zero(bc[4]), zero(bc[5]))
    fxyz = derive(z, fxy, 2, zero(bc[4]), zero(bc[5]))
    if variant == "fxyz_zero":
        fxyz = np.zeros_like(fxyz)
    elif variant == "fxyz_from_x":
        fxyz = derive(x, fyz, 0, zero(bc[0]), zero(bc[1]))
    return fx, fy, fz, fxy, fxz, fyz, fxyz


def cells(x, y, z, qx, qy, qz, side="right"):
    """The largest index with knot <= q, clamped to [0, n - 2], on each axis (`side="left"`: the wrong search)."""
    return tuple(np.clip(np.searchsorted(k, q, side=side) - 1, 0, len(k) - 2) for k, q in ((x, qx), (y, qy), (z, qz)))


def evaluate(x, y, z, f, tabs, qx, qy, qz, variant=None, side="right"):
    """Rows (Q, C) of the tricubic Hermite patches at (qx, qy, qz); every query is evaluated (the end patch continues)."""
    fx, fy, fz, fxy, fxz, fyz, fxyz = tabs
    i, j, k = cells(x, y, z, qx, qy, qz, side)
    with np.errstate(all="ignore"):
        hx = x[i + 1] - x[i]
        t = ((qx - x[i]) / hx)[:, None]
        hy = y[j + 1] - y[j]
        u = ((qy - y[j]) / hy)[:, None]
        hz = z[k + 1] - z[k]
        w = ((qz - z[k]) / hz)[:, None]
        hx, hy, hz = hx[:, None], hy[:, None], hz[:, None]
        if variant == "x_first":
            def alongx(P, Px, jj, kk):
                return hermite(P[i, jj, kk], P[i + 1, jj, kk], Px[i, jj, kk], Px[i + 1, jj, kk], hx, t)
            val, der = [], []
            for kk in (k, k + 1):
                X = {n: [alongx(P, Px, jj, kk) for jj in (j, j + 1)] for n, (P, Px) in
                     {"f": (f, fx), "fy": (fy, fxy), "fz": (fz, fxz), "fyz": (fyz, fxyz)}.items()}
                val.append(hermite(X["f"][0], X["f"][1], X["fy"][0], X["fy"][1], hy, u))
                der.append(hermite(X["fz"][0], X["fz"][1], X["fyz"][0], X["fyz"][1], hy, u))
            return hermite(val[0], val[1], der[0], der[1], hz, w)

        def alongz(P, Pz, ii, jj):
            return hermite(P[ii, jj, k], P[ii, jj, k + 1], Pz[ii, jj, k], Pz[ii, jj, k + 1], hz, w)
        val, der = [], []
        for ii in (i, i + 1):
            Z = {n: [alongz(P, Pz, ii, jj) for jj in (j, j + 1)] for n, (P, Pz) in
                 {"f": (f, fz), "fx": (fx, fxz), "fy": (fy, fyz), "fxy": (fxy, fxyz)}.items()}
            val.append(hermite(Z["f"][0], Z["f"][1], Z["fy"][0], Z["fy"][1], hy, u))
            der.append(hermite(Z["fx"][0], Z["fx"][1], Z["fxy"][0], Z["fxy"][1], hy, u))
        return hermite(val[0], val[1], der[0], der[1], hx, t)


def interp(x, y, z, f, qx, qy, qz, bc=DEFAULT_BC, variant=None, side="right"):
    return evaluate(x, y, z, f, tables(x, y, z, f, bc, variant), qx, qy, qz, variant, side)
