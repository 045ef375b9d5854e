"""Test-side restatement of the Pchip / Akima / CubicHermite build (include/ndinterp.h, ndi_strategy1d): the knot
derivatives and the {a, b} tables in numpy, in exactly the operation order the header specifies.

Every line is one IEEE operation per element in the array's own dtype (numpy does not fuse), so the device kernel --
compiled without contraction, same order -- gives the same bits.  `x`: (n,), `y`: (n, lanes), one float dtype.
"""
import numpy as np


def _col(x):
    return (x[1:] - x[:-1])[:, None]


def sgn(v):
    """The header's sgn: -1, 0 or 1, formed from the two comparisons (v > 0) - (v < 0) -- so sgn(NaN) = 0 and
    sgn(-0) = sgn(+0) = 0.  (np.sign gives NaN for NaN, and NaN != NaN would read as a sign change.)"""
    return (v > 0).astype(np.int8) - (v < 0).astype(np.int8)


def pchip_k(x, y):
    """Fritsch-Butland derivatives with the three-point shape-preserving end formula (scipy's PchipInterpolator)."""
    T = y.dtype.type
    n = len(x)
    h = _col(x)
    dl = (y[1:] - y[:-1]) / h
    k = np.zeros_like(y)
    if n == 2:
        k[0] = dl[0]
        k[1] = dl[0]
        return k
    h0, h1 = h[:-1], h[1:]            # h_{i-1}, h_i       for interior knot i
    d0, d1 = dl[:-1], dl[1:]          # delta_{i-1}, delta_i
    w1 = (h1 + h1) + h0
    w2 = h1 + (h0 + h0)
    with np.errstate(divide="ignore", invalid="ignore"):
        hm = (w1 + w2) / (w1 / d0 + w2 / d1)
    flat = (d0 == 0) | (d1 == 0) | ((d0 > 0) != (d1 > 0))
    k[1:-1] = np.where(flat, T(0), hm)

    def edge(h0, h1, m0, m1):
        d = (((h0 + h0) + h1) * m0 - h0 * m1) / (h0 + h1)
        opp = sgn(d) != sgn(m0)
        big = (sgn(m0) != sgn(m1)) & (np.abs(d) > T(3) * np.abs(m0))
        return np.where(opp, T(0), np.where(big, T(3) * m0, d))
    k[0] = edge(h[0], h[1], dl[0], dl[1])
    k[-1] = edge(h[-1], h[-2], dl[-1], dl[-2])
    return k


def akima_k(x, y):
    """Akima (1970) derivatives, n >= 3.  Returns (k, s): s = w1 + w2 per knot -- the golden generator uses it to keep
    its inputs away from scipy's relative threshold, which the specification replaces by an exact `s == 0`."""
    T = y.dtype.type
    n = len(x)
    h = _col(x)
    dl = (y[1:] - y[:-1]) / h
    m = np.empty((n + 3,) + y.shape[1:], y.dtype)      # m[j + 2] = m_j, j = -2 .. n
    m[2:-2] = dl
    m[1] = (m[2] + m[2]) - m[3]
    m[0] = (m[1] + m[1]) - m[2]
    m[-2] = (m[-3] + m[-3]) - m[-4]
    m[-1] = (m[-2] + m[-2]) - m[-3]
    w1 = np.abs(m[3:] - m[2:-1])        # |m_{i+1} - m_i|
    w2 = np.abs(m[1:-2] - m[:-3])       # |m_{i-1} - m_{i-2}|
    s = w1 + w2
    with np.errstate(divide="ignore", invalid="ignore"):
        kk = (w1 * m[1:-2] + w2 * m[2:-1]) / s
    return np.where(s == 0, T(0.5) * (m[1:-2] + m[2:-1]), kk), s


def tables(x, y, k):
    """cubic_spline.rs:362-363 with the strategy's own k."""
    dx = _col(x)
    dy = y[1:] - y[:-1]
    return k[:-1] * dx - dy, dy - k[1:] * dx


def build(rule, x, y, dydx=None):
    """(a, b) of a strategy: rule in {"pchip", "akima", "hermite"}; y of any trailing shape (flattened to lanes)."""
    y2 = np.ascontiguousarray(y).reshape(len(x), -1)
    if rule == "pchip":
        k = pchip_k(x, y2)
    elif rule == "akima":
        k = akima_k(x, y2)[0]
    else:
        k = np.ascontiguousarray(dydx, dtype=y2.dtype).reshape(y2.shape)
    return tables(x, y2, k)


def evaluate(x, y, a, b, q):
    """cubic_spline.rs:811-828 (what the evaluation kernels and the oracle's interp1d_cubic compute); queries outside
    the knots continue the first / last interval's polynomial."""
    i = np.clip(np.searchsorted(x, q, side="right") - 1, 0, len(x) - 2)
    t = ((q - x[i]) / (x[i + 1] - x[i]))[:, None]
    one = y.dtype.type(1)
    return (one - t) * y[i] + t * y[i + 1] + t * (one - t) * (a[i] * (one - t) + b[i] * t)
