"""Test-side restatement of the partial-derivative contract of Bicubic (include/ndinterp.h, ndi_interp2d_partial) in numpy, in
exactly the operation order the header specifies and in the arrays' own dtype: the forms H0, H1, H2 and the evaluation with
the forms swapped.  The node tables and the cell search are the surface's (tests/bicubic_ref.py: `tables`, `cells`); with
orders (0, 0) `evaluate` is `bicubic_ref.evaluate`.  Every line is one IEEE operation per element (numpy does not fuse), so
the device kernel -- compiled without contraction, same order -- gives the same bits.

`variant`: a deliberately wrong form for the self-check of the goldens --
  "h1_over_hh"   H1 divided by h * h (the chain rule applied once too often)
  "h2_three"     3 where H2 has 6 (the second derivative of s^3 taken as 3 s)
"""
import numpy as np

import bicubic_ref

ORDERS = tuple((nx, ny) for nx in range(3) for ny in range(3) if (nx, ny) != (0, 0))
MUTANTS = ("h1_over_hh", "h2_three")


def hermite_nu(nu, pl, pr, kl, kr, h, s, variant=None):
    """H_nu of the header; h, s broadcast over the lanes."""
    if nu == 0:
        return bicubic_ref.hermite(pl, pr, kl, kr, h, s)
    T = pl.dtype.type
    d = pr - pl
    a = kl * h - d
    b = d - kr * h
    c2 = b - (a + a)
    c3 = b - a
    if nu == 1:
        c1 = d + a
        return (c1 + s * ((c2 + c2) - (T(3) * c3) * s)) / ((h * h) if variant == "h1_over_hh" else h)
    assert nu == 2, nu
    return ((c2 + c2) - (T(3 if variant == "h2_three" else 6) * c3) * s) / (h * h)


def evaluate(x, y, z, zx, zy, zxy, qx, qy, nu_x, nu_y, variant=None):
    """Rows (Q, C) of d^(nu_x + nu_y) / dx^nu_x dy^nu_y of the bicubic Hermite patches at (qx, qy)."""
    i, j = bicubic_ref.cells(x, y, qx, qy)
    hx = (x[i + 1] - x[i])
    t = ((qx - x[i]) / hx)[:, None]
    hy = (y[j + 1] - y[j])
    u = ((qy - y[j]) / hy)[:, None]
    hx, hy = hx[:, None], hy[:, None]
    p0 = hermite_nu(nu_y, z[i, j], z[i, j + 1], zy[i, j], zy[i, j + 1], hy, u, variant)
    p1 = hermite_nu(nu_y, z[i + 1, j], z[i + 1, j + 1], zy[i + 1, j], zy[i + 1, j + 1], hy, u, variant)
    d0 = hermite_nu(nu_y, zx[i, j], zx[i, j + 1], zxy[i, j], zxy[i, j + 1], hy, u, variant)
    d1 = hermite_nu(nu_y, zx[i + 1, j], zx[i + 1, j + 1], zxy[i + 1, j], zxy[i + 1, j + 1], hy, u, variant)
    return hermite_nu(nu_x, p0, p1, d0, d1, hx, t, variant)


def interp(x, y, z, qx, qy, nu_x, nu_y, bc=bicubic_ref.DEFAULT_BC, variant=None):
    zx, zy, zxy = bicubic_ref.tables(x, y, z, bc)
    return evaluate(x, y, z, zx, zy, zxy, qx, qy, nu_x, nu_y, variant)
