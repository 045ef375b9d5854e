"""The reference of the Trilinear tests (the implementation never imports it).

`trilinear_ref` is the value rule of include/ndinterp3d.h in its slab form: the oracle's Bilinear on the two slabs
data[:, :, k] and data[:, :, k + 1], then one calc_frac along z in numpy (numpy does not fuse).  `trilinear_direct` is an
independent second form: the seven calc_frac steps straight from the eight gathered corners.  The two must agree bit for
bit (tests/test_trilinear_abi.py).

Both return (fail, axis, out): the lowest failing query (None: none) and its axis -- x before y before z within a query --
and out[Q, lanes], of which only the rows before `fail` are evaluated (the others are zero)."""
import numpy as np

import oracle


def first_failure(x, y, z, qx, qy, qz, extrapolate):
    """Without extrapolation a coordinate outside [k[0], k[n-1]] fails (a NaN fails that test too); with it only a NaN."""
    bad = []
    for k, q in ((x, qx), (y, qy), (z, qz)):
        bad.append(np.isnan(q) if extrapolate else ~((k[0] <= q) & (q <= k[-1])))
    anyb = bad[0] | bad[1] | bad[2]
    if not anyb.any():
        return None, None
    f = int(np.argmax(anyb))
    return f, 0 if bad[0][f] else 1 if bad[1][f] else 2


def _prep(x, y, z, data, qx, qy, qz):
    data = np.ascontiguousarray(data)
    dt = data.dtype
    x, y, z = (np.ascontiguousarray(k, dtype=dt) for k in (x, y, z))
    qx, qy, qz = (np.ascontiguousarray(q, dtype=dt).ravel() for q in (qx, qy, qz))
    lanes = int(np.prod(data.shape[3:], dtype=np.int64))
    return x, y, z, data.reshape(data.shape[:3] + (lanes,)), qx, qy, qz, lanes


def trilinear_ref(x, y, z, data, qx, qy, qz, extrapolate=False):
    x, y, z, d, qx, qy, qz, lanes = _prep(x, y, z, data, qx, qy, qz)
    fail, axis = first_failure(x, y, z, qx, qy, qz, extrapolate)
    good = qx.size if fail is None else fail
    out = np.zeros((qx.size, lanes), dtype=d.dtype)
    kz = oracle.get_lower_index(z, qz[:good])
    with np.errstate(all="ignore"):
        for k in np.unique(kz):
            rows = np.nonzero(kz == k)[0]
            slabs = []
            for kk in (k, k + 1):
                st, _, _, b = oracle.interp2d_bilinear(x, y, np.ascontiguousarray(d[:, :, kk]), qx[rows], qy[rows], extrapolate)
                assert st == 0, st
                slabs.append(b)
            z1, z2 = z[k], z[k + 1]
            out[rows] = ((slabs[1] - slabs[0]) / (z2 - z1)) * (qz[rows] - z1)[:, None] + slabs[0]
    return fail, axis, out


def _calc_frac(x1, y1, x2, y2, x):
    """linear.rs:29-36, one IEEE operation per step in the arrays' dtype."""
    return ((y2 - y1) / (x2 - x1)[:, None]) * (x - x1)[:, None] + y1


def trilinear_direct(x, y, z, data, qx, qy, qz, extrapolate=False):
    x, y, z, d, qx, qy, qz, lanes = _prep(x, y, z, data, qx, qy, qz)
    fail, axis = first_failure(x, y, z, qx, qy, qz, extrapolate)
    good = qx.size if fail is None else fail
    out = np.zeros((qx.size, lanes), dtype=d.dtype)
    gx, gy, gz = qx[:good], qy[:good], qz[:good]
    i, j, k = (oracle.get_lower_index(kn, q) for kn, q in ((x, gx), (y, gy), (z, gz)))
    with np.errstate(all="ignore"):
        x1, x2, y1, y2, z1, z2 = x[i], x[i + 1], y[j], y[j + 1], z[k], z[k + 1]
        c00 = _calc_frac(x1, d[i, j, k], x2, d[i + 1, j, k], gx)
        c01 = _calc_frac(x1, d[i, j, k + 1], x2, d[i + 1, j, k + 1], gx)
        c10 = _calc_frac(x1, d[i, j + 1, k], x2, d[i + 1, j + 1, k], gx)
        c11 = _calc_frac(x1, d[i, j + 1, k + 1], x2, d[i + 1, j + 1, k + 1], gx)
        c0 = _calc_frac(y1, c00, y2, c10, gy)
        c1 = _calc_frac(y1, c01, y2, c11, gy)
        out[:good] = _calc_frac(z1, c0, z2, c1, gz)
    return fail, axis, out


def knots_and_midpoints(k):
    """Every knot and every cell midpoint of an axis, in the axis' dtype."""
    k = np.asarray(k)
    return np.concatenate([k, ((k[:-1].astype(np.float64) + k[1:].astype(np.float64)) / 2).astype(k.dtype)])


def bits(a):
    """The integer view bits are compared on, NaN equal to NaN (every NaN is mapped to one pattern)."""
    a = np.ascontiguousarray(a)
    v = a.view(np.int32 if a.dtype == np.float32 else np.int64).copy()
    v[np.isnan(a)] = -1
    return v
