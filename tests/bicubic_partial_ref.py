"""Test-side restatement of the partial-derivative contract of Bicubic (include/ndinterp.h, ndi_interp2d_partial) in numpy, in
exactly the operation order the header specifies and in the arrays' own dtype: the forms H0, H1, H2 and the evaluation with
the forms swapped.  The node tables and the cell search are the surface's (tests/bicubic_ref.py: `tables`, `cells`); with
orders (0, 0) `evaluate` is `bicubic_ref.evaluate`.  Every line is one IEEE operation per element (numpy does not fuse), so
the device kernel -- compiled without contraction, same order -- gives the same bits.

`variant`: a deliberately wrong form for the self-check of the goldens --
  "h1_over_hh"   H1 divided by h * h (the chain rule applied once too often)
  "h2_three"     3 where H2 has 6 (the second derivative of s^3 taken as 3 s)
  "reciprocal"   H1's x / h as x * (1 / h)
  "h2_two_divisions"  H2's x / (h * h) as x / h / h
  "three_c3_s"   3 * (c3 * s) for (3 * c3) * s, and likewise with 6
  "contracted"   a = kl h - d and b = d - kr h of H1 and H2 rounded once (a fused multiply-add; it shows in f32 only, where
                 float64 holds the product exactly)
  "flushed"      subnormal operands and results of every operation read and written as zero
"""
import numpy as np

import bicubic_ref

ORDERS = tuple((nx, ny) for nx in range(3) for ny in range(3) if (nx, ny) != (0, 0))
MUTANTS = ("h1_over_hh", "h2_three")          # wrong formulas: they miss the scipy goldens (tests/test_bicubic_partial_abi.py)
# the right formulas rounded differently: a last bit here and there, which only a bit-for-bit comparison on inputs chosen
# for it can see (tests/test_hostile_inputs.py holds the hostile grids to telling each of the six)
ROUNDING_MUTANTS = ("reciprocal", "h2_two_divisions", "three_c3_s", "contracted")
FLUSHED = "flushed"       # not in MUTANTS: the judge of the subnormal lanes (tests/test_hostile_inputs.py)


def mutant_orders(variant):
    """the forms a variant changes: a partial of order nu on an axis goes through H_nu on that axis"""
    return {"h1_over_hh": (1,), "reciprocal": (1,), "h2_three": (2,), "h2_two_divisions": (2,)}.get(variant, (1, 2))


def flush(v):
    """subnormals to zero, the sign kept, as a flushing device would"""
    v = np.asarray(v)
    return np.where((v != 0) & (np.abs(v) < np.finfo(v.dtype).tiny), np.copysign(v.dtype.type(0), v), v)


def _once(f, *v):
    """f on the float64 of the operands, rounded once to their own type: what a fused chain would give"""
    return f(*[np.asarray(w, np.float64) for w in v]).astype(np.asarray(v[0]).dtype)


def hermite_nu(nu, pl, pr, kl, kr, h, s, variant=None):
    """H_nu of the header; h, s broadcast over the lanes."""
    if variant == FLUSHED:
        return _hermite_nu_flushed(nu, pl, pr, kl, kr, h, s)
    if nu == 0:
        return bicubic_ref.hermite(pl, pr, kl, kr, h, s)
    T = pl.dtype.type
    d = pr - pl
    if variant == "contracted":
        a = _once(lambda k, w, e: k * w - e, kl, h, d)
        b = _once(lambda e, k, w: e - k * w, d, kr, h)
    else:
        a = kl * h - d
        b = d - kr * h
    c2 = b - (a + a)
    c3 = b - a
    if nu == 1:
        c1 = d + a
        top = c1 + s * ((c2 + c2) - (T(3) * (c3 * s) if variant == "three_c3_s" else (T(3) * c3) * s))
        if variant == "reciprocal":
            return top * (T(1) / h)
        return top / ((h * h) if variant == "h1_over_hh" else h)
    assert nu == 2, nu
    six = T(3 if variant == "h2_three" else 6)
    top = (c2 + c2) - (six * (c3 * s) if variant == "three_c3_s" else (six * c3) * s)
    return top / h / h if variant == "h2_two_divisions" else top / (h * h)


def _hermite_nu_flushed(nu, pl, pr, kl, kr, h, s):
    """The same operations with the result of each one flushed (the operands are flushed by the caller)."""
    F = flush
    T = pl.dtype.type
    d = F(pr - pl)
    a = F(F(kl * h) - d)
    b = F(d - F(kr * h))
    if nu == 0:
        c0 = F(T(1) - s)
        return F(F(F(c0 * pl) + F(s * pr)) + F(F(s * c0) * F(F(a * c0) + F(b * s))))
    c2 = F(b - F(a + a))
    c3 = F(b - a)
    if nu == 1:
        c1 = F(d + a)
        return F(F(c1 + F(s * F(F(c2 + c2) - F(F(T(3) * c3) * s)))) / h)
    return F(F(F(c2 + c2) - F(F(T(6) * c3) * s)) / F(h * h))


def evaluate(x, y, z, zx, zy, zxy, qx, qy, nu_x, nu_y, variant=None):
    """Rows (Q, C) of d^(nu_x + nu_y) / dx^nu_x dy^nu_y of the bicubic Hermite patches at (qx, qy)."""
    i, j = bicubic_ref.cells(x, y, qx, qy)
    hx = (x[i + 1] - x[i])
    t = ((qx - x[i]) / hx)[:, None]
    hy = (y[j + 1] - y[j])
    u = ((qy - y[j]) / hy)[:, None]
    hx, hy = hx[:, None], hy[:, None]
    if variant == FLUSHED:
        z, zx, zy, zxy, hx, hy = (flush(v) for v in (z, zx, zy, zxy, hx, hy))
        t, u = flush(flush(flush(qx - x[i])[:, None] / hx)), flush(flush(flush(qy - y[j])[:, None] / hy))
    p0 = hermite_nu(nu_y, z[i, j], z[i, j + 1], zy[i, j], zy[i, j + 1], hy, u, variant)
    p1 = hermite_nu(nu_y, z[i + 1, j], z[i + 1, j + 1], zy[i + 1, j], zy[i + 1, j + 1], hy, u, variant)
    d0 = hermite_nu(nu_y, zx[i, j], zx[i, j + 1], zxy[i, j], zxy[i, j + 1], hy, u, variant)
    d1 = hermite_nu(nu_y, zx[i + 1, j], zx[i + 1, j + 1], zxy[i + 1, j], zxy[i + 1, j + 1], hy, u, variant)
    return hermite_nu(nu_x, p0, p1, d0, d1, hx, t, variant)


def interp(x, y, z, qx, qy, nu_x, nu_y, bc=bicubic_ref.DEFAULT_BC, variant=None):
    zx, zy, zxy = bicubic_ref.tables(x, y, z, bc)
    return evaluate(x, y, z, zx, zy, zxy, qx, qy, nu_x, nu_y, variant)
