"""Test-side restatement of the antiderivative rule (include/ndinterp.h, ndi_interp1d_antiderivative): the prefix table P
of an antiderivative handle from the source handle's {y, a, b}, its evaluation and the definite integral, in numpy, in
exactly the operation order the header specifies.

Every line is one IEEE operation per element in the array's own dtype (numpy does not fuse), so the device kernels --
compiled without contraction, same order -- give the same bits.  `x`: (n,), `y`: (n, lanes), `a`, `b`: (n - 1, lanes),
one float dtype; Linear sources pass `a = b = None`.  The prefix table is the header's FIXED blocked sum (B = 256 knots
per block); `block` and `serial` exist so that a test can show that other summation orders give other bits.
"""
import numpy as np

B = 256


def _g_coefficients(yl, yr, a, b):
    """(c1, c2, c3) of the cubic class, or (c1, None, None) of Linear"""
    T = yl.dtype.type
    if a is None:
        return (yr - yl) * T(0.5), None, None
    dy = yr - yl
    c1 = (dy + a) * T(0.5)
    c2 = (b - (a + a)) / T(3)
    c3 = (b - a) * T(0.25)
    return c1, c2, c3


def intervals(x, y, a=None, b=None):
    """I[i], (n - 1, lanes): the integral over interval i"""
    assert x.dtype == y.dtype and y.ndim == 2
    assert (a is None) == (b is None)
    if a is not None:
        assert a.dtype == b.dtype == y.dtype and a.shape == b.shape == (len(x) - 1, y.shape[1])
    dx = (x[1:] - x[:-1])[:, None]
    yl, yr = y[:-1], y[1:]
    c1, c2, c3 = _g_coefficients(yl, yr, a, b)
    if a is None:
        return dx * (yl + c1)
    return dx * (yl + (c1 + (c2 - c3)))


def prefix(x, y, a=None, b=None, block=B, serial=False):
    """P, (n, lanes).  `serial`: one running sum over all intervals (a mutant); `block`: another block length (a mutant)."""
    I = intervals(x, y, a, b)
    n, lanes = y.shape
    if serial:
        block = n
    nblk = (n + block - 1) // block
    Ipad = np.zeros((nblk * block, lanes), dtype=y.dtype)      # (the padding is never added into a value that is kept)
    Ipad[:n - 1] = I
    Ipad = Ipad.reshape(nblk, block, lanes)
    S = np.empty((nblk, block, lanes), dtype=y.dtype)
    run = np.zeros((nblk, lanes), dtype=y.dtype)               # +0: the local sums, every block at once, serially inside
    for j in range(block):
        S[:, j] = run
        run = run + Ipad[:, j]
    tot = run                                                  # the running sum taken over the block's end
    O = np.empty((nblk, lanes), dtype=y.dtype)
    acc = np.zeros(lanes, dtype=y.dtype)
    for k in range(nblk):                                      # the block offsets, serially
        O[k] = acc
        acc = acc + tot[k]
    P = (O[:, None, :] + S).reshape(nblk * block, lanes)[:n]
    assert P.dtype == y.dtype
    return np.ascontiguousarray(P)


def lower_index(x, q):
    """get_lower_index of the reference for finite queries, clamped to [0, n - 2]"""
    return np.clip(np.searchsorted(x, q, side="right") - 1, 0, len(x) - 2)


def evaluate(x, y, a, b, P, idx, q):
    """F(q), (len(q), lanes): interval `idx` per query (the oracle's get_lower_index), t the cubic evaluation's"""
    i = np.asarray(idx, dtype=np.int64)
    dx = x[i + 1] - x[i]
    t = ((q - x[i]) / dx)[:, None]
    dx = dx[:, None]
    yl, yr = y[i], y[i + 1]
    if a is None:
        c1, _, _ = _g_coefficients(yl, yr, None, None)
        G = t * (yl + t * c1)
    else:
        c1, c2, c3 = _g_coefficients(yl, yr, a[i], b[i])
        G = t * (yl + t * (c1 + t * (c2 - t * c3)))
    return P[i] + dx * G


def integrate(x, y, a, b, P, idx_lo, lo, idx_hi, hi):
    """F(hi) - F(lo), one subtraction"""
    return evaluate(x, y, a, b, P, idx_hi, hi) - evaluate(x, y, a, b, P, idx_lo, lo)


# the Linear variant: the same functions without coefficient tables
def prefix_linear(x, y, **kw):
    return prefix(x, y, None, None, **kw)


def evaluate_linear(x, y, P, idx, q):
    return evaluate(x, y, None, None, P, idx, q)


def integrate_linear(x, y, P, idx_lo, lo, idx_hi, hi):
    return integrate(x, y, None, None, P, idx_lo, lo, idx_hi, hi)
