"""Test-side restatement of the 2-D antiderivative rule of Bicubic (include/ndinterp.h, ndi_interp2d_antiderivative): the
five prefix tables of an integral handle from the source's node tables {z, zx, zy, zxy}, F(qx, qy) and the rectangle
integral, in numpy, in exactly the operation order the header specifies.

Built on bicubic_ref (the cells, t, u) and antiderivative_ref.prefix (the fixed blocked sum, B = 256).  Every line is one
IEEE operation per element in the arrays' own dtype, so the device kernels -- compiled without contraction, same order --
give the same bits.  `x`: (nx,), `y`: (ny,), the node tables (nx, ny, C), one float dtype.  The keyword arguments name
deliberately wrong forms for the mutant tests.
"""
import numpy as np

import antiderivative_ref
import bicubic_ref


def hermite_ab(knots, p, k):
    """H's lines on (n, lanes) Hermite data: a, b, each (n - 1, lanes)"""
    h = (knots[1:] - knots[:-1])[:, None]
    d = p[1:] - p[:-1]
    return k[:-1] * h - d, d - k[1:] * h


def prefix_axis(knots, p, k, block=antiderivative_ref.B, serial=False, no_third=False):
    """The blocked prefix sum along axis 0 of the interval integrals of Hermite data (values p, slopes k), (n, lanes)"""
    a, b = hermite_ab(knots, p, k)
    if no_third:   # mutant: c2 without the / 3
        return _prefix_no_third(knots, p, a, b)
    return antiderivative_ref.prefix(knots, p, a, b, block=block, serial=serial)


def _prefix_no_third(knots, p, a, b):
    T = p.dtype.type
    dx = (knots[1:] - knots[:-1])[:, None]
    d = p[1:] - p[:-1]
    c1 = (d + a) * T(0.5)
    c2 = b - (a + a)
    c3 = (b - a) * T(0.25)
    I = dx * (p[:-1] + (c1 + (c2 - c3)))
    out = np.zeros_like(p)
    out[1:] = np.cumsum(I, axis=0)
    return out


def tables(x, y, z, zx, zy, zxy, pp_along_y=False, **kw):
    """(PP, Qz, Qzy, Pz, Pzx), each of z's shape"""
    nx, ny, C = z.shape
    assert x.dtype == y.dtype == z.dtype == zx.dtype == zy.dtype == zxy.dtype

    def along_x(p, k):
        flat = lambda f: np.ascontiguousarray(f.reshape(nx, ny * C))   # noqa: E731
        return prefix_axis(x, flat(p), flat(k), **kw).reshape(nx, ny, C)

    def along_y(p, k):
        flat = lambda f: np.ascontiguousarray(f.transpose(1, 0, 2).reshape(ny, nx * C))   # noqa: E731
        return np.ascontiguousarray(prefix_axis(y, flat(p), flat(k), **kw).reshape(ny, nx, C).transpose(1, 0, 2))

    Qz, Qzy = along_x(z, zx), along_x(zy, zxy)
    Pz, Pzx = along_y(z, zy), along_y(zx, zxy)
    PP = along_y(Qz, Qzy) if pp_along_y else along_x(Pz, Pzx)
    return PP, Qz, Qzy, Pz, Pzx


def G(pl, pr, kl, kr, h, s, no_third=False):
    """The header's G in Hermite form; h, s broadcast over the lanes"""
    T = pl.dtype.type
    d = pr - pl
    a = kl * h - d
    b = d - kr * h
    c1 = (d + a) * T(0.5)
    c2 = (b - (a + a)) if no_third else (b - (a + a)) / T(3)
    c3 = (b - a) * T(0.25)
    return s * (pl + s * (c1 + s * (c2 - s * c3)))


def evaluate(x, y, nodes, tabs, qx, qy, no_third=False):
    """F(qx, qy), rows (Q, C).  nodes = (z, zx, zy, zxy), tabs = (PP, Qz, Qzy, Pz, Pzx)"""
    z, zx, zy, zxy = nodes
    PP, Qz, Qzy, Pz, Pzx = tabs
    i, j = bicubic_ref.cells(x, y, qx, qy)
    hx = x[i + 1] - x[i]
    t = ((qx - x[i]) / hx)[:, None]
    hy = y[j + 1] - y[j]
    u = ((qy - y[j]) / hy)[:, None]
    hx, hy = hx[:, None], hy[:, None]
    g = lambda *args: G(*args, no_third=no_third)   # noqa: E731
    w0 = Pz[i, j] + hy * g(z[i, j], z[i, j + 1], zy[i, j], zy[i, j + 1], hy, u)
    w1 = Pz[i + 1, j] + hy * g(z[i + 1, j], z[i + 1, j + 1], zy[i + 1, j], zy[i + 1, j + 1], hy, u)
    v0 = Pzx[i, j] + hy * g(zx[i, j], zx[i, j + 1], zxy[i, j], zxy[i, j + 1], hy, u)
    v1 = Pzx[i + 1, j] + hy * g(zx[i + 1, j], zx[i + 1, j + 1], zxy[i + 1, j], zxy[i + 1, j + 1], hy, u)
    e = PP[i, j] + hy * g(Qz[i, j], Qz[i, j + 1], Qzy[i, j], Qzy[i, j + 1], hy, u)
    return e + hx * g(w0, w1, v0, v1, hx, t)


def rectangle(x, y, nodes, tabs, xa, xb, ya, yb, other_association=False, **kw):
    """(F(xb, yb) - F(xa, yb)) - (F(xb, ya) - F(xa, ya)), rows (Q, C)"""
    F = lambda qx, qy: evaluate(x, y, nodes, tabs, qx, qy, **kw)   # noqa: E731
    if other_association:   # mutant
        return ((F(xb, yb) - F(xa, yb)) - F(xb, ya)) + F(xa, ya)
    return (F(xb, yb) - F(xa, yb)) - (F(xb, ya) - F(xa, ya))


def integral(x, y, z, xa, xb, ya, yb, bc=bicubic_ref.DEFAULT_BC, **kw):
    """The whole chain from the data: Bicubic's node tables, the prefix tables, the rectangle rows"""
    zx, zy, zxy = bicubic_ref.tables(x, y, z, bc)
    nodes = (z, zx, zy, zxy)
    tab_kw = {k: v for k, v in kw.items() if k in ("pp_along_y", "block", "serial", "no_third")}
    tabs = tables(x, y, *nodes, **tab_kw)
    return rectangle(x, y, nodes, tabs, xa, xb, ya, yb, other_association=kw.get("other_association", False),
                     no_third=kw.get("no_third", False))
