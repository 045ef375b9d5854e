"""Test-side restatement of the periodic Bicubic contract (include/ndinterp.h, ndi_interp2d_create_bicubic_periodic) in
numpy, in exactly the operation order the header specifies and in the arrays' own dtype.

A pass along a periodic axis is the oracle's CubicSpline build with periodic = True (the bit-faithful restatement of the
reference: the closed form on 3 knots, the cyclic system otherwise) followed by the derivative rule's Y
(tests/derivative_ref.py) with the last row a copy of the first; a pass along a non-periodic axis is tests/bicubic_ref.py's, the true not-a-knot row included.
The wrap is the reference's rem_euclid (cubic_spline.rs:805-809), applied to out-of-range coordinates only; evaluation is
bicubic_ref's / bicubic_partial_ref's on the wrapped coordinates.  `periodic_axes`: bit 0 is x, bit 1 is y.
"""
import numpy as np

import bicubic_partial_ref
import bicubic_ref
import derivative_ref
import oracle

PERIODIC_X, PERIODIC_Y = 1, 2


def knot_derivatives(k, cols, left, right, periodic):
    """The spline's derivative at every knot: `cols` (n, lanes) on knots `k` (n,)."""
    if not periodic:
        return bicubic_ref.knot_derivatives(k, cols, left, right)
    st, a, b = oracle.cubic_build(k, cols, periodic=True)
    if st != oracle.OK:
        raise ValueError(oracle.STATUS_NAMES[st])
    Y = derivative_ref.derive(k, cols, a, b)[0]
    Y[-1] = Y[0]          # a copy: the rule's two end rows are two roundings of the same knot derivative k[n-1] = k[0]
    return Y


def tables(x, y, z, bc=bicubic_ref.DEFAULT_BC, periodic_axes=0):
    """(zx, zy, zxy), each of z's shape.  The two `bc` entries of a periodic axis are not read."""
    nx, ny, C = z.shape
    assert x.dtype == y.dtype == z.dtype and x.shape == (nx,) and y.shape == (ny,)
    per_x, per_y = bool(periodic_axes & PERIODIC_X), bool(periodic_axes & PERIODIC_Y)

    def along_x(f):
        return knot_derivatives(x, np.ascontiguousarray(f.reshape(nx, ny * C)), bc[0], bc[1], per_x).reshape(nx, ny, C)

    def along_y(f, left, right):
        ft = np.ascontiguousarray(f.transpose(1, 0, 2).reshape(ny, nx * C))
        return np.ascontiguousarray(knot_derivatives(y, ft, left, right, per_y).reshape(ny, nx, C).transpose(1, 0, 2))

    zx = along_x(z)
    # the cross pass: the periodic pass on zx, or zx's own end condition along y (the same kinds with value 0)
    return zx, along_y(z, bc[2], bc[3]), along_y(zx, (bc[2][0], 0.0), (bc[3][0], 0.0))


def wrap(k, q):
    """The five lines of the header on the out-of-range entries of q (knots k), in q's dtype; in-range entries and NaN stay."""
    q = np.asarray(q)
    k0, kn = k[0], k[-1]
    out = q.copy()
    m = ~((k0 <= q) & (q <= kn))
    with np.errstate(invalid="ignore"):
        d = q[m] - k0
        p = kn - k0
        r = np.fmod(d, p)
        r = np.where(r < 0, r + np.abs(p), r)
        out[m] = r + k0
    return out


def wrapped(x, y, qx, qy, wrap_axes):
    return (wrap(x, qx) if wrap_axes & PERIODIC_X else qx), (wrap(y, qy) if wrap_axes & PERIODIC_Y else qy)


def evaluate(x, y, z, zx, zy, zxy, qx, qy, wrap_axes):
    """Rows (Q, C) of a handle that wraps on `wrap_axes` (the periodic axes of a handle built with extrapolate)."""
    return bicubic_ref.evaluate(x, y, z, zx, zy, zxy, *wrapped(x, y, qx, qy, wrap_axes))


def evaluate_partial(x, y, z, zx, zy, zxy, qx, qy, nu_x, nu_y, wrap_axes):
    return bicubic_partial_ref.evaluate(x, y, z, zx, zy, zxy, *wrapped(x, y, qx, qy, wrap_axes), nu_x, nu_y)


def evaluate_jet(x, y, z, zx, zy, zxy, qx, qy, parts, wrap_axes):
    """One array per (nu_x, nu_y) of `parts`."""
    return [evaluate_partial(x, y, z, zx, zy, zxy, qx, qy, nx_, ny_, wrap_axes) for nx_, ny_ in parts]


def make_periodic(z, periodic_axes):
    """A copy of z whose last row / column repeats the first along each periodic axis: x first, then y, so the corners agree."""
    z = z.copy()
    if periodic_axes & PERIODIC_X:
        z[-1] = z[0]
    if periodic_axes & PERIODIC_Y:
        z[:, -1] = z[:, 0]
    return z


def interp(x, y, z, qx, qy, bc=bicubic_ref.DEFAULT_BC, periodic_axes=0, nu=(0, 0)):
    zx, zy, zxy = tables(x, y, z, bc, periodic_axes)
    return evaluate_partial(x, y, z, zx, zy, zxy, qx, qy, nu[0], nu[1], periodic_axes)
