"""Test-side restatement of the Bicubic contract (include/ndinterp.h, ndi_interp2d_create_bicubic) in numpy, in exactly
the operation order the header specifies and in the arrays' own dtype.

The 1-D solves go through the oracle's spline build (the reference operation order) on the reshaped / transposed columns,
followed by the derivative rule's Y (tests/derivative_ref.py).  One case cannot: a not-a-knot right end on more than three
knots.  The reference's last row carries dx[n-2] on the diagonal where the not-a-knot condition has dx[n-3]
(cubic_spline.rs:635), which is the same number only when the last two intervals are equal; Bicubic builds the true row,
so that its default ends are scipy's spline on any knots.  `cubic_build` below restates the reference's general build line
by line with that one entry selectable; with the reference's entry it equals oracle.cubic_build bit for bit
(tests/test_bicubic_abi.py holds it to that), so the two differ in that entry and in nothing else.  Every evaluation line is one IEEE operation per element
(numpy does not fuse), so the device kernel -- compiled without contraction, same order -- gives the same bits.
`x`: (nx,), `y`: (ny,), `z`: (nx, ny, C), one float dtype.  `bc`: four (kind, value) pairs, x-left, x-right, y-left, y-right.
"""
import numpy as np

import derivative_ref
import oracle

NOT_A_KNOT = (oracle.BC_NOT_A_KNOT, 0.0)
DEFAULT_BC = (NOT_A_KNOT,) * 4
# one end condition of every other kind, a nonzero value among them: the second end set of the Bicubic tests
MIXED_BC = ((oracle.BC_NATURAL, 0.0), (oracle.BC_FIRST_DERIV, 0.75), (oracle.BC_CLAMPED, 0.0), (oracle.BC_CLAMPED, 0.0))


def _specialize(end):
    kind, val = end
    if kind == oracle.BC_NATURAL:
        return oracle.BC_SECOND_DERIV, 0.0
    if kind == oracle.BC_CLAMPED:
        return oracle.BC_FIRST_DERIV, 0.0
    return kind, val


def cubic_build(x, data, left, right, reference_row=False):
    """(a, b), each (n - 1, lanes): the reference's general (non-periodic, not the 3-point parabola) spline build in its
    operation order -- rows, right-hand sides, CubicSpline::thomas, then a / b -- in the arrays' dtype.  The last diagonal
    entry of a not-a-knot right end is dx[n-3]; `reference_row` puts the reference's dx[n-2] there."""
    T = x.dtype.type
    n = len(x)
    two, three = T(2), T(3)
    (lk, lv), (rk, rv) = _specialize(left), _specialize(right)
    assert n >= 3 and not (n == 3 and lk == rk == oracle.BC_NOT_A_KNOT)
    y = data
    dx = x[1:] - x[:-1]
    up, mid, low = (np.zeros(n, x.dtype) for _ in range(3))
    up[1:-1] = dx[:-1]
    mid[1:-1] = two * (dx[1:] + dx[:-1])
    low[1:-1] = dx[1:]
    rhs = np.zeros_like(y)
    dxn, dxn_1 = dx[1:, None], dx[:-1, None]
    rhs[1:-1] = three * (dxn * (y[1:-1] - y[:-2]) / dxn_1 + dxn_1 * (y[2:] - y[1:-1]) / dxn)
    dx0, dx1, dx_1, dx_2 = dx[0], dx[1], dx[-1], dx[-2]
    if lk == oracle.BC_NOT_A_KNOT:
        mid[0] = dx1
        d = x[2] - x[0]
        up[0] = d
        tmp1 = (dx0 + two * d) * dx1
        rhs[0] = (tmp1 * (y[1] - y[0]) / dx0 + (dx0 * dx0) * (y[2] - y[1]) / dx1) / d
    elif lk == oracle.BC_FIRST_DERIV:
        mid[0] = T(1)
        rhs[0] = T(lv)
    else:
        up[0], mid[0] = dx0, two * dx0
        rhs[0] = three * (y[1] - y[0]) - T(lv) * (dx0 * dx0) / two
    if rk == oracle.BC_NOT_A_KNOT:
        mid[-1] = dx_1 if reference_row else dx_2
        d = x[-1] - x[-3]
        low[-1] = d
        tmp1 = (two * d + dx_1) * dx_2
        rhs[-1] = ((dx_1 * dx_1) * (y[-2] - y[-3]) / dx_2 + tmp1 * (y[-1] - y[-2]) / dx_1) / d
    elif rk == oracle.BC_FIRST_DERIV:
        mid[-1] = T(1)
        rhs[-1] = T(rv)
    else:
        mid[-1], low[-1] = two * dx_1, dx_1
        rhs[-1] = three * (y[-1] - y[-2]) + T(rv) * (dx_1 * dx_1) / two
    for i in range(1, n):
        w = low[i] / mid[i - 1]
        mid[i] = mid[i] - w * up[i - 1]
        rhs[i] = rhs[i] - w * rhs[i - 1]
    k = np.empty_like(y)
    k[-1] = rhs[-1] / mid[-1]
    for i in range(n - 2, -1, -1):
        k[i] = (rhs[i] - up[i] * k[i + 1]) / mid[i]
    dy = y[1:] - y[:-1]
    return k[:-1] * dx[:, None] - dy, dy - k[1:] * dx[:, None]


def knot_derivatives(k, cols, left, right):
    """The spline's derivative at every knot: `cols` (n, lanes) on knots `k` (n,)."""
    if right[0] == oracle.BC_NOT_A_KNOT and not (len(k) == 3 and left[0] == oracle.BC_NOT_A_KNOT):
        a, b = cubic_build(k, cols, left, right)
    else:
        st, a, b = oracle.cubic_build(k, cols, left=left, right=right)
        assert st == oracle.OK, st
    return derivative_ref.derive(k, cols, a, b)[0]


def tables(x, y, z, bc=DEFAULT_BC):
    """(zx, zy, zxy), each of z's shape."""
    nx, ny, C = z.shape
    assert x.dtype == y.dtype == z.dtype and x.shape == (nx,) and y.shape == (ny,)

    def along_x(f):
        return knot_derivatives(x, np.ascontiguousarray(f.reshape(nx, ny * C)), bc[0], bc[1]).reshape(nx, ny, C)

    def along_y(f, left, right):
        ft = np.ascontiguousarray(f.transpose(1, 0, 2).reshape(ny, nx * C))
        return np.ascontiguousarray(knot_derivatives(y, ft, left, right).reshape(ny, nx, C).transpose(1, 0, 2))

    zx = along_x(z)
    # the cross pass: zx's end condition along y is the x-derivative of z's, the same kinds with value 0
    return zx, along_y(z, bc[2], bc[3]), along_y(zx, (bc[2][0], 0.0), (bc[3][0], 0.0))


def hermite(pl, pr, kl, kr, h, s, variant=None):
    """H of the header; h, s broadcast over the lanes.  `variant`: a deliberately wrong form for the mutant tests."""
    one = pl.dtype.type(1)
    d = pr - pl
    a = kl * h - d
    b = d - (kl if variant == "b_from_kl" else kr) * h
    c0 = one - s
    return c0 * pl + s * pr + (s * c0) * (a * c0 + b * s)


def cells(x, y, qx, qy, side="right"):
    """get_lower_index on each axis: clamped to the end cells, so queries outside continue the end patch.  `side="left"` is
    the wrong search (a query at a knot falls into the cell below), for the self-check of the hostile query sets."""
    i = np.clip(np.searchsorted(x, qx, side=side) - 1, 0, len(x) - 2)
    j = np.clip(np.searchsorted(y, qy, side=side) - 1, 0, len(y) - 2)
    return i, j


def evaluate(x, y, z, zx, zy, zxy, qx, qy, variant=None, side="right"):
    """Rows (Q, C) of the bicubic Hermite patches at (qx, qy)."""
    i, j = cells(x, y, qx, qy, side)
    hx = (x[i + 1] - x[i])
    t = ((qx - x[i]) / hx)[:, None]
    hy = (y[j + 1] - y[j])
    u = ((qy - y[j]) / hy)[:, None]
    hx, hy = hx[:, None], hy[:, None]
    if variant == "zxy_zero":
        zxy = np.zeros_like(zxy)
    p0 = hermite(z[i, j], z[i, j + 1], zy[i, j], zy[i, j + 1], hy, u, variant)
    p1 = hermite(z[i + 1, j], z[i + 1, j + 1], zy[i + 1, j], zy[i + 1, j + 1], hy, u, variant)
    d0 = hermite(zx[i, j], zx[i, j + 1], zxy[i, j], zxy[i, j + 1], hy, u, variant)
    d1 = hermite(zx[i + 1, j], zx[i + 1, j + 1], zxy[i + 1, j], zxy[i + 1, j + 1], hy, u, variant)
    return hermite(p0, p1, d0, d1, hx, t, variant)


def interp(x, y, z, qx, qy, bc=DEFAULT_BC, variant=None):
    zx, zy, zxy = tables(x, y, z, bc)
    return evaluate(x, y, z, zx, zy, zxy, qx, qy, variant)
