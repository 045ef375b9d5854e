"""Test-side restatement of the node derivatives of a Bicubic handle built from a local rule (include/ndinterp.h,
ndi_interp2d_create_bicubic_local) in numpy: the 1-D rule of tests/hermite_ref.py composed along the axes, in the arrays'
own dtype.  Every line of the rule is one IEEE operation per element (numpy does not fuse), and the three views below only
move columns, so the device kernel -- compiled without contraction, same order -- gives the same bits.

Evaluation has no restatement of its own: the surface, its partials, F and the rectangle integral are
bicubic_ref.evaluate, bicubic_partial_ref.evaluate and bicubic_integral_ref.tables / evaluate / rectangle on these tables.
`x`: (nx,), `y`: (ny,), `z`: (nx, ny, C), one float dtype.  `rule`: "pchip" or "akima".
"""
import numpy as np

import hermite_ref

RULES = ("pchip", "akima")
MINIMUM = {"pchip": 2, "akima": 3, "hermite": 2}


def rule_k(rule, knots, cols):
    """k = RULE(knots, columns): cols (n, lanes) -> (n, lanes)."""
    if rule == "pchip":
        return hermite_ref.pchip_k(knots, cols)
    assert rule == "akima", rule
    return hermite_ref.akima_k(knots, cols)[0]


def tables(rule, x, y, z):
    """(zx, zy, zxy), each of z's shape: zx = RULE(x, .) on z viewed as (nx, ny C); zy = RULE(y, .) on each z[i] viewed as
    (ny, C); zxy = RULE(y, .) on each zx[i]."""
    nx, ny, C = z.shape
    assert x.dtype == y.dtype == z.dtype and x.shape == (nx,) and y.shape == (ny,)

    def along_y(f):
        ft = np.ascontiguousarray(f.transpose(1, 0, 2).reshape(ny, nx * C))
        return np.ascontiguousarray(rule_k(rule, y, ft).reshape(ny, nx, C).transpose(1, 0, 2))

    with np.errstate(all="ignore"):
        zx = rule_k(rule, x, np.ascontiguousarray(z.reshape(nx, ny * C))).reshape(nx, ny, C)
        return zx, along_y(z), along_y(zx)
