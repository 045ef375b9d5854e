"""Test-side restatement of the derivative rule (include/ndinterp.h, ndi_interp1d_derivative): the tables {Y, A, B} of a
derivative handle from the source handle's {y, a, b}, in numpy, in exactly the operation order the header specifies.

Every line is one IEEE operation per element in the array's own dtype (numpy does not fuse), so the device kernel --
compiled without contraction, same order -- gives the same bits.  `x`: (n,), `y`: (n, lanes), `a`, `b`: (n - 1, lanes),
one float dtype.  Evaluation of the result is tests/hermite_ref.evaluate (or the oracle's interp1d_cubic).
"""
import numpy as np


def derive(x, y, a, b):
    """(Y, A, B): Y[i] the derivative at the left end of interval i, Y[n-1] at the last knot, A == B."""
    T = y.dtype.type
    assert x.dtype == y.dtype == a.dtype == b.dtype and y.ndim == 2 and a.shape == b.shape == (len(x) - 1, y.shape[1])
    dx = (x[1:] - x[:-1])[:, None]
    dy = y[1:] - y[:-1]
    Y = np.empty_like(y)
    Y[:-1] = (dy + a) / dx
    Y[-1] = (dy[-1] - b[-1]) / dx[-1]
    A = (T(3) * (b - a)) / dx
    return Y, A, A.copy()


def derive_nu(x, y, a, b, nu):
    """The rule applied `nu` times."""
    for _ in range(nu):
        y, a, b = derive(x, y, a, b)
    return y, a, b
