"""GPU: periodic axes of the Bicubic strategy against the numpy restatement of the contract
(tests/bicubic_periodic_ref.py), bit for bit -- the node tables and their seam, rows on in-range and on wrapped queries,
the eight partial handles and the jet on wrapped queries, the error semantics (Bilinear's without extrapolation, the
periodic 1-D CubicSpline's with it), the mismatch refusal, and every other handle surface at one small shape."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bicubic_integral_ref
import bicubic_periodic_ref as ref
import bicubic_ref
from conftest import ROOT
from hostile_inputs import check_bits

pytestmark = pytest.mark.gpu

SHAPES = [(3, 3), (3, 4), (4, 3), (4, 4), (5, 7), (64, 48)]
LANES = [1, 2, 3, 4, 5, 64, 65]
NQS = [1, 63, 64, 65, 10007]
AXES = {"x": 1, "y": 2, "xy": 3}
NK = bicubic_ref.NOT_A_KNOT
DTYPES = pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])


def ends_for(axes, mixed):
    """the contract's four ends: the default pair on a periodic axis, bicubic_ref.MIXED_BC's (or the default) on the other"""
    bc = list(bicubic_ref.MIXED_BC if mixed else bicubic_ref.DEFAULT_BC)
    if axes & 1:
        bc[0] = bc[1] = NK
    if axes & 2:
        bc[2] = bc[3] = NK
    return tuple(bc)


def make_grid(rng, nx, ny, C, dt, axes):
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
    return x, y, ref.make_periodic(rng.normal(size=(nx, ny, C)).astype(dt), axes)


def strategy(pkg, axes, bc, extrapolate=False):
    s, sb = pkg.Bicubic.new(), pkg.SingleBoundary
    if axes & 1:
        s.periodic_x()
    elif bc[:2] != (NK, NK):
        s.boundary_x(pkg.RowBoundary.Mixed(sb(*bc[0]), sb(*bc[1])))
    if axes & 2:
        s.periodic_y()
    elif bc[2:] != (NK, NK):
        s.boundary_y(pkg.RowBoundary.Mixed(sb(*bc[2]), sb(*bc[3])))
    return s.extrapolate(extrapolate)


def build(pkg, x, y, z, axes, bc=bicubic_ref.DEFAULT_BC, device_inputs=False, extrapolate=False):
    import torch
    if device_inputs:
        x, y, z = (torch.as_tensor(a, device="cuda:0") for a in (x, y, z))
    return pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(strategy(pkg, axes, bc, extrapolate)).build()


def dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


def in_range_queries(rng, x, y, nq):
    """random in-range queries, then (as far as nq allows) the four corners and every node"""
    dt = x.dtype
    ii, jj = np.meshgrid(np.arange(len(x)), np.arange(len(y)), indexing="ij")
    sx = np.concatenate([[x[0], x[0], x[-1], x[-1]], x[ii.ravel()]])
    sy = np.concatenate([[y[0], y[-1], y[0], y[-1]], y[jj.ravel()]])
    k = min(len(sx), nq)
    qx = np.concatenate([sx[:k], rng.uniform(x[0], x[-1], nq - k)]).astype(dt)
    qy = np.concatenate([sy[:k], rng.uniform(y[0], y[-1], nq - k)]).astype(dt)
    return np.clip(qx, x[0], x[-1]), np.clip(qy, y[0], y[-1])


def wrapped_queries(rng, x, y, nq, axes):
    """3.5 periods either side on a wrapping axis, with exactly k0 - p, kn + p, kn, k0; one width either side on the other"""
    def one(k, wraps):
        p = k[-1] - k[0]
        if not wraps:
            return rng.uniform(k[0] - p, k[-1] + p, nq).astype(k.dtype)
        q = rng.uniform(k[0] - 3.5 * p, k[-1] + 3.5 * p, nq).astype(k.dtype)
        m = min(4, nq)
        q[:m] = [k[0] - p, k[-1] + p, k[-1], k[0]][:m]
        return rng.permutation(q)
    return one(x, axes & 1), one(y, axes & 2)


def check_seam(tabs, axes, what):
    for name, t in zip(("zx", "zy", "zxy"), tabs):
        if axes & 1:
            check_bits(t[-1], t[0], f"{what}: {name}, the x seam")
        if axes & 2:
            check_bits(np.ascontiguousarray(t[:, -1]), np.ascontiguousarray(t[:, 0]), f"{what}: {name}, the y seam")


# Every lane class meets every periodic-axes setting; the shapes, the other axis' ends and the memory space of the inputs
# cycle through, so that every value of every list appears (a reduced cross product).
CONFIGS = [(SHAPES[(3 * a + l) % len(SHAPES)], C, name, (a + l) % 2 == 1, (a + l) % 3 == 0)
           for a, name in enumerate(AXES) for l, C in enumerate(LANES)]


def test_the_configurations_cover_every_value():
    assert {c[0] for c in CONFIGS} == set(SHAPES) and {c[3] for c in CONFIGS} == {c[4] for c in CONFIGS} == {False, True}
    assert {(c[1], c[2]) for c in CONFIGS} == {(C, a) for C in LANES for a in AXES}
    for a in ("x", "y"):
        assert {c[3] for c in CONFIGS if c[2] == a} == {False, True}, a


@pytest.mark.parametrize("shape,C,axes,mixed,device_inputs", CONFIGS,
                         ids=[f"{s[0]}x{s[1]}x{C}-p{a}-{'mixed' if m else 'default'}-{'dev' if d else 'host'}"
                              for s, C, a, m, d in CONFIGS])
@DTYPES
def test_tables_and_rows_are_bit_exact(pkg, dt, shape, C, axes, mixed, device_inputs):
    axes = AXES[axes]
    rng = np.random.default_rng(hash((shape, C, axes)) % 2**32)
    x, y, z = make_grid(rng, shape[0], shape[1], C, dt, axes)
    bc = ends_for(axes, mixed)
    it = build(pkg, x, y, z, axes, bc, device_inputs)
    got = it.strategy.tables()
    for name, g, r in zip(("zx", "zy", "zxy"), got, ref.tables(x, y, z, bc, axes)):
        check_bits(g, r, name)
    check_seam(got, axes, "device tables")
    zx, zy, zxy = got                       # rows: the restatement's evaluation on the device's own tables
    for nq in NQS:
        qx, qy = in_range_queries(rng, x, y, nq)
        want = bicubic_ref.evaluate(x, y, z, zx, zy, zxy, qx, qy)
        for path in (pkg.PATH_AUTO, pkg.PATH_GATHER):
            it.strategy.path = path
            check_bits(it.interp_array(qx, qy), want, f"host queries nq={nq} path={path}")
            check_bits(it.interp_array(dev(qx), dev(qy)).cpu().numpy(), want, f"device queries nq={nq} path={path}")


@DTYPES
def test_no_periodic_axis_is_the_plain_handle(pkg, dt):
    """periodic_axes == 0 through the new symbol builds, bit for bit, what ndi_interp2d_create_bicubic builds"""
    import ctypes as C
    from test_bicubic_abi import desc_for
    cap = pkg._capi
    rng = np.random.default_rng(8)
    x, y, z = make_grid(rng, 5, 7, 3, dt, 0)
    sb = [(k, v) for k, v in bicubic_ref.MIXED_BC]
    bc = (cap.Boundary * 4)(*[cap.Boundary(int(k), float(v)) for k, v in sb])
    tabs = []
    for create in (lambda d, h: cap.lib().ndi_interp2d_create_bicubic_periodic(C.byref(d), bc, 0, C.byref(h)),
                   lambda d, h: cap.lib().ndi_interp2d_create_bicubic(C.byref(d), bc, C.byref(h))):
        h = C.c_void_p()
        assert create(desc_for(cap, x, y, z, cap.F32 if dt == np.float32 else cap.F64), h) == cap.OK, cap.last_error()
        out = [np.empty_like(z) for _ in range(3)]
        assert cap.lib().ndi_interp2d_tables(h, *[o.ctypes.data for o in out], cap.MEM_HOST) == cap.OK
        cap.lib().ndi_interp2d_destroy(h)
        tabs.append(out)
    for a, b, r in zip(tabs[0], tabs[1], bicubic_ref.tables(x, y, z, bicubic_ref.MIXED_BC)):
        check_bits(a, b, "periodic_axes = 0 against the plain call")
        check_bits(a, r, "periodic_axes = 0 against the restatement")


WRAP_CASES = [((5, 7), 3, "x", True), ((4, 4), 4, "y", True), ((3, 3), 1, "xy", False), ((64, 48), 5, "xy", False),
              ((9, 7), 65, "x", False)]


@pytest.mark.parametrize("shape,C,axes,mixed", WRAP_CASES, ids=[f"{s[0]}x{s[1]}x{C}-p{a}" for s, C, a, m in WRAP_CASES])
@DTYPES
def test_wrapped_rows(pkg, dt, shape, C, axes, mixed):
    import torch
    axes = AXES[axes]
    rng = np.random.default_rng(hash((shape, C, axes, 1)) % 2**32)
    x, y, z = make_grid(rng, shape[0], shape[1], C, dt, axes)
    it = build(pkg, x, y, z, axes, ends_for(axes, mixed), extrapolate=True)
    tabs = it.strategy.tables()
    nq = 4001
    qx, qy = wrapped_queries(rng, x, y, nq, axes)
    want = ref.evaluate(x, y, z, *tabs, qx, qy, axes)
    assert np.isfinite(want).all()
    check_bits(it.interp_array(qx, qy), want, "fresh output, host queries")
    check_bits(it.interp_array(dev(qx), dev(qy)).cpu().numpy(), want, "fresh output, device queries")
    host = np.full((nq, C), -7.0, dt)
    it.interp_array_into(qx, qy, host)
    check_bits(host, want, "caller-owned host buffer")
    buf = torch.full((nq, C), -7.0, dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda:0")
    it.interp_array_into(dev(qx), dev(qy), buf)
    check_bits(buf.cpu().numpy(), want, "caller-owned device buffer")
    # a handle of the same build that does not extrapolate does not wrap: the same queries are out of range
    with pytest.raises(pkg.InterpolateError.OutOfBounds):
        build(pkg, x, y, z, axes, ends_for(axes, mixed)).interp_array(qx, qy)


@pytest.mark.parametrize("axes", list(AXES))
@DTYPES
def test_partials_and_jet_on_wrapped_queries(pkg, dt, axes):
    axes = AXES[axes]
    rng = np.random.default_rng(31 + axes)
    x, y, z = make_grid(rng, 9, 7, 3, dt, axes)
    it = build(pkg, x, y, z, axes, ends_for(axes, True), extrapolate=True)
    tabs = it.strategy.tables()
    qx, qy = wrapped_queries(rng, x, y, 2003, axes)
    rows = {(0, 0): it.interp_array(qx, qy)}
    check_bits(rows[(0, 0)], ref.evaluate(x, y, z, *tabs, qx, qy, axes), "the surface")
    for nu in [(a, b) for a in range(3) for b in range(3) if (a, b) != (0, 0)]:
        part = it.partial(*nu)
        assert part.strategy.wraps == axes
        rows[nu] = part.interp_array(qx, qy)
        check_bits(rows[nu], ref.evaluate_partial(x, y, z, *tabs, qx, qy, nu[0], nu[1], axes), f"partial {nu}")
        check_bits(part.interp_array(dev(qx), dev(qy)).cpu().numpy(), rows[nu], f"partial {nu}, device queries")
    for order in (1, 2):
        parts = pkg.interp2d.JET_PARTS[order]
        for q in ((qx, qy), (dev(qx), dev(qy))):
            got = it.jet(*q, order)
            assert len(got) == len(parts)
            for nu, g in zip(parts, got):
                check_bits(g if isinstance(g, np.ndarray) else g.cpu().numpy(), rows[nu], f"jet order {order}, part {nu}")
    z0, gx, gy = it.value_and_gradient(qx, qy)
    check_bits(gx, rows[(1, 0)], "value_and_gradient: d/dx")
    check_bits(gy, rows[(0, 1)], "value_and_gradient: d/dy")


@pytest.fixture(scope="module")
def small(pkg):
    """64 x 48 x 5 f64 periodic on both axes: the handle that wraps, the one that does not, Bilinear, queries, rows"""
    rng = np.random.default_rng(11)
    x, y, z = make_grid(rng, 64, 48, 5, np.float64, 3)
    wrap = build(pkg, x, y, z, 3, extrapolate=True)
    plain = build(pkg, x, y, z, 3)
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    tabs = wrap.strategy.tables()
    qx, qy = wrapped_queries(rng, x, y, 10007, 3)
    ix, iy = in_range_queries(rng, x, y, 10007)
    return dict(x=x, y=y, z=z, wrap=wrap, plain=plain, bil=bil, tabs=tabs, qx=qx, qy=qy, ix=ix, iy=iy,
                want=ref.evaluate(x, y, z, *tabs, qx, qy, 3), iwant=bicubic_ref.evaluate(x, y, z, *tabs, ix, iy))


def failure(it, qx, qy, into=None):
    with pytest.raises(Exception) as e:
        if into is not None:
            it.interp_array_into(qx, qy, into)
        else:
            it.interp_array(qx, qy)
    v = e.value
    return type(v).__name__, str(v), getattr(v, "index", None), getattr(v, "value", None), getattr(v, "axis", None)


@pytest.mark.parametrize("kind", ["x_low", "x_high", "y_low", "y_high", "both"])
def test_without_extrapolation_out_of_range_is_bilinears(pkg, small, kind):
    import torch
    x, y, nq = small["x"], small["y"], len(small["ix"])
    pos = nq // 2
    qx, qy = small["ix"].copy(), small["iy"].copy()
    if kind in ("x_low", "both"):
        qx[pos] = x[0] - 0.25
    if kind == "x_high":
        qx[pos] = x[-1] + 0.25
    if kind == "y_low":
        qy[pos] = y[0] - 0.25
    if kind in ("y_high", "both"):
        qy[pos] = y[-1] + 0.5
    qy[pos + 7] = np.nan                       # a later failure must not be the one reported
    exp = failure(small["bil"], qx, qy)
    assert exp[2] == pos and exp[4] == (1 if kind.startswith("y") else 0)
    assert failure(small["plain"], qx, qy) == exp
    assert failure(small["plain"], dev(qx), dev(qy)) == exp
    for mk in (lambda: np.full((nq, 5), -7.0), lambda: torch.full((nq, 5), -7.0, dtype=torch.float64, device="cuda:0")):
        buf = mk()
        q = (qx, qy) if isinstance(buf, np.ndarray) else (dev(qx), dev(qy))
        assert failure(small["plain"], *q, into=buf) == exp
        rows = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
        check_bits(rows[:pos], small["iwant"][:pos], "rows before the failure")
        assert np.all(rows[pos:] == -7.0), "rows from the failure on keep the sentinel"


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_with_wrap_nan_and_inf_fail_as_the_periodic_1d_spline(pkg, small, bad):
    import torch
    x, y, z, nq = small["x"], small["y"], small["z"], len(small["qx"])
    col = np.ascontiguousarray(z[:, 0, :])
    one_d = pkg.Interp1DBuilder.new(col).x(x).strategy(
        pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Periodic).extrapolate(True)).build()
    pos = 4321
    for axis in (0, 1):
        qx, qy = small["qx"].copy(), small["qy"].copy()
        (qx, qy)[axis][pos] = bad
        (qx, qy)[1 - axis][pos + 3] = np.nan           # a later failure must not be the one reported
        with pytest.raises(Exception) as e:
            one_d.interp_array(np.where(np.arange(nq) == pos, bad, small["qx"]))
        exp = (type(e.value).__name__, str(e.value), e.value.index)
        assert exp[0] == "Panic" and exp[2] == pos
        assert failure(small["wrap"], qx, qy)[:3] == exp
        assert failure(small["wrap"], dev(qx), dev(qy))[:3] == exp
        for mk in (lambda: np.full((nq, 5), -7.0), lambda: torch.full((nq, 5), -7.0, dtype=torch.float64, device="cuda:0")):
            buf = mk()
            q = (qx, qy) if isinstance(buf, np.ndarray) else (dev(qx), dev(qy))
            assert failure(small["wrap"], *q, into=buf)[:3] == exp
            rows = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
            check_bits(rows[:pos], small["want"][:pos], "rows before the failure")
            assert np.all(rows[pos:] == -7.0), "rows from the failure on keep the sentinel"
    # x before y for the same query
    qx, qy = small["qx"].copy(), small["qy"].copy()
    qx[pos] = qy[pos] = bad
    assert failure(small["wrap"], qx, qy)[2] == pos


def test_with_wrap_on_x_only_a_y_outside_is_not_an_error(pkg):
    rng = np.random.default_rng(5)
    x, y, z = make_grid(rng, 9, 7, 3, np.float64, 1)
    it = build(pkg, x, y, z, 1, extrapolate=True)
    qx, qy = wrapped_queries(rng, x, y, 500, 1)
    assert np.sum((qy < y[0]) | (qy > y[-1])) > 100 and np.sum((qx < x[0]) | (qx > x[-1])) > 100
    want = ref.evaluate(x, y, z, *it.strategy.tables(), qx, qy, 1)
    check_bits(it.interp_array(qx, qy), want, "y continues the end patch, x wraps")
    for inf in (np.inf, -np.inf):                   # an infinite y is not NaN: no error on the axis that does not wrap
        qy2 = qy.copy()
        qy2[7] = inf
        rows = it.interp_array(qx, qy2)
        check_bits(np.delete(rows, 7, axis=0), np.delete(want, 7, axis=0), "the other rows")
    qx2 = qx.copy()
    qx2[7] = np.inf
    with pytest.raises(pkg.Panic, match="NaN"):
        it.interp_array(qx2, qy)


@DTYPES
def test_a_mismatch_is_a_value_error_naming_the_axis(pkg, dt):
    rng = np.random.default_rng(2)
    for axes, axis, where in ((1, "x", (-1, 3, 1)), (2, "y", (2, -1, 0)), (3, "x", (-1, 2, 2)), (3, "y", (3, -1, 1))):
        x, y, z = make_grid(rng, 6, 5, 3, dt, axes)
        for value in (z[where] + dt(1), dt(np.nan)):
            bad = z.copy()
            bad[where] = value            # one lane of one column (both axes periodic: the x pass runs first)
            for device_inputs in (False, True):
                with pytest.raises(pkg.BuilderError.ValueError, match=f"Bicubic: the {axis} axis is periodic"):
                    build(pkg, x, y, bad, axes, device_inputs=device_inputs)
        assert build(pkg, x, y, z, axes).strategy._periodic == axes        # the periodic data builds
    x, y, z = make_grid(rng, 6, 5, 3, dt, 1)
    z[0, 2, 1] = z[-1, 2, 1] = np.nan                                      # NaN in the seam row: NaN != NaN
    with pytest.raises(pkg.BuilderError.ValueError, match="Bicubic: the x axis is periodic"):
        build(pkg, x, y, z, 1)


def test_clone_ring_sharded_and_integrals(pkg, small):
    import torch
    wrap, plain, want, nq = small["wrap"], small["plain"], small["want"], len(small["qx"])
    x, y, z = small["x"], small["y"], small["z"]
    dqx, dqy = dev(small["qx"]), dev(small["qy"])
    out = torch.empty((nq, 5), dtype=torch.float64, device="cuda:0")
    wrap.interp_array_into(dqx, dqy, out, async_launch=True)                     # async_launch + finish
    wrap.strategy.finish()
    check_bits(out.cpu().numpy(), want, "async_launch + finish")
    rep = wrap.replicate([0])[0]                                                 # clone: the bits travel
    assert rep.strategy.wraps == 3
    for a, b in zip(rep.strategy.tables(), small["tabs"]):
        check_bits(a, b, "clone: tables")
    check_bits(rep.interp_array(small["qx"], small["qy"]), want, "clone: rows")
    got = np.zeros_like(want)                                                    # ring: 2 slots, 1000 does not divide 10 007
    ring = pkg.striped_ring(1000, 5, 2, np.float64, 0)

    def consumer(c, rows):
        got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
    wrap.interp_array_ring(dqx, dqy, 1000, consumer, slots=ring)
    check_bits(got, want, "ring")
    got = np.full_like(want, -1.0)                                               # sharded: two replicas on one device
    pkg.sharding.interp_array_sharded([wrap, rep], small["qx"], small["qy"], out=got)
    check_bits(got, want, "sharded")
    other = build(pkg, x, y, z, 1, extrapolate=True)                             # other periodic bits: not a replica
    with pytest.raises(Exception, match="replicas of one interpolator"):
        pkg.sharding.interp_array_sharded([wrap, other], small["qx"], small["qy"], out=got)
    # integrals: refused for the handle that wraps (by the mirror, and by the library itself)
    with pytest.raises(TypeError, match="antiderivative of a wrapping strategy is not provided"):
        wrap.antiderivative()
    import ctypes as C
    cap = pkg._capi
    h = C.c_void_p(1234)
    assert cap.lib().ndi_interp2d_antiderivative(wrap.strategy._h, C.byref(h)) == cap.BAD_ARG and h.value is None
    assert "wraps queries on x and y" in cap.last_error() and "Bicubic" in cap.last_error()
    # ... and today's code for the periodic build that does not: the full rectangle against the restatement on that table
    F = plain.antiderivative()
    nodes = (z,) + tuple(small["tabs"])
    tabs = bicubic_integral_ref.tables(x, y, *nodes)
    r = [np.array([v]) for v in (x[0], x[-1], y[0], y[-1])]
    check_bits(F.integral(*r), bicubic_integral_ref.rectangle(x, y, nodes, tabs, *r), "the integral over the full rectangle")


def test_wrapped_rows_under_the_bounds_checked_library():
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import bicubic_periodic_ref as ref, test_gpu_bicubic_periodic as t\n"
        "from hostile_inputs import check_bits\n"
        "pkg = load_product_package(); rng = np.random.default_rng(5)\n"
        "for dt in (np.float32, np.float64):\n"
        "    for (nx, ny), C, axes in (((3, 4), 1, 3), ((64, 48), 65, 1)):\n"
        "        x, y, z = t.make_grid(rng, nx, ny, C, dt, axes)\n"
        "        bc = t.ends_for(axes, True)\n"
        "        it = t.build(pkg, x, y, z, axes, bc, extrapolate=True)\n"
        "        tabs = it.strategy.tables()\n"
        "        for a, b in zip(tabs, ref.tables(x, y, z, bc, axes)): check_bits(a, b, 'tables')\n"
        "        for nq in (1, 65, 10007):\n"
        "            qx, qy = t.wrapped_queries(rng, x, y, nq, axes)\n"
        "            want = ref.evaluate(x, y, z, *tabs, qx, qy, axes)\n"
        "            check_bits(it.interp_array(qx, qy), want, 'host')\n"
        "            d = it.interp_array(torch.as_tensor(qx, device='cuda:0'), torch.as_tensor(qy, device='cuda:0'))\n"
        "            check_bits(d.cpu().numpy(), want, 'device')\n"
        "            buf = np.zeros_like(want); it.interp_array_into(qx, qy, buf); check_bits(buf, want, 'into')\n"
        "            for g, nu in zip(it.jet(qx, qy, 1), ((0, 0), (1, 0), (0, 1))):\n"
        "                check_bits(g, ref.evaluate_partial(x, y, z, *tabs, qx, qy, nu[0], nu[1], axes), 'jet')\n"
        "print('checked OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDI_LIB=lib), timeout=600)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
