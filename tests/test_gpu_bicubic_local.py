"""GPU: Bicubic handles whose node derivatives come from a local rule (Pchip, Akima) or from the caller
(ndi_interp2d_create_bicubic_local, ndi_interp2d_create_bicubic_hermite) against the numpy restatement
(tests/bicubic_local_ref.py), bit for bit: the node tables read through ndi_interp2d_tables, evaluated rows, the partial
handles, the jet, the antiderivative and the rectangle integral (the existing kernels, on two-point axes for the first
time), the grid-line identity against a 1-D handle on the device, hostile data, the handle plumbing at one shape, the build
shapes under the bounds-checked library, and one grid whose table passes 2^32 elements."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bicubic_integral_ref
import bicubic_local_ref
import bicubic_partial_ref
import bicubic_ref
import hostile_inputs
from conftest import ROOT
from hostile_inputs import check_bits

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
RULES = ("pchip", "akima", "hermite")
# (nx, ny, C), the axes: uneven throughout, one evenly spaced case; "offset": device-resident data one element off a 16-byte
# boundary, so the scalar fallback runs on lanes the vector form would take
SHAPES = [((2, 2, 1), "uneven"), ((2, 5, 1), "uneven"), ((3, 3, 1), "uneven"), ((4, 3, 2), "uneven"), ((5, 6, 3), "uneven"),
          ((7, 5, 4), "uneven"), ((7, 5, 4), "even"), ((33, 17, 8), "uneven"), ((4, 4, 129), "uneven"), ((5, 5, 4), "offset")]
DEEP = [(2, 2, 1), (4, 3, 2), (7, 5, 4)]         # partials, jet and integrals


def rules_for(shape):
    return [r for r in RULES if min(shape[:2]) >= bicubic_local_ref.MINIMUM[r]]


def make_grid(rng, shape, dt, axes="uneven"):
    nx, ny, C = shape
    if axes == "even":
        x, y = (np.arange(nx) * 0.5 - 1.0).astype(dt), (np.arange(ny) * 0.25).astype(dt)
    else:
        x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
        y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
    return x, y, rng.normal(size=shape).astype(dt)


def given_tables(rng, z):
    """caller-given derivatives: any arrays will do, no rule is applied"""
    return tuple(rng.normal(size=z.shape).astype(z.dtype) for _ in range(3))


def reference_tables(rule, x, y, z, given=None):
    return given if rule == "hermite" else bicubic_local_ref.tables(rule, x, y, z)


def on_device(a, offset=False):
    import torch
    t = torch.as_tensor(a, device="cuda:0")
    if not offset:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda:0")
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def build(pkg, rule, x, y, z, given=None, device_inputs=False, extrapolate=False, offset=False):
    if device_inputs:
        x, y, z = on_device(x), on_device(y), on_device(z, offset)
        given = None if given is None else tuple(on_device(t, offset) for t in given)
    s = {"pchip": pkg.Bicubic.pchip, "akima": pkg.Bicubic.akima, "hermite": lambda: pkg.Bicubic.hermite(*given)}[rule]()
    return pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(s.extrapolate(extrapolate)).build()


def queries(rng, x, y, extra=40, outside=True):
    """every node (so every grid line and both ends of each), random points on every grid line of either family, interior
    points, and -- `outside` -- points up to one end interval outside on every side"""
    dt = x.dtype
    ii, jj = np.meshgrid(np.arange(len(x)), np.arange(len(y)), indexing="ij")
    qx = [x[ii.ravel()], np.repeat(x, 3), rng.uniform(x[0], x[-1], 3 * len(y)), rng.uniform(x[0], x[-1], extra)]
    qy = [y[jj.ravel()], rng.uniform(y[0], y[-1], 3 * len(x)), np.repeat(y, 3), rng.uniform(y[0], y[-1], extra)]
    if outside:
        wx0, wx1, wy0, wy1 = x[1] - x[0], x[-1] - x[-2], y[1] - y[0], y[-1] - y[-2]
        qx += [[x[0] - wx0, x[-1] + wx1, x[0] - 0.5 * wx0, x[-1] + 0.5 * wx1, x[0], x[-1], x[0] - wx0, x[-1] + wx1]]
        qy += [[y[0] - wy0, y[-1] + wy1, y[0], y[-1], y[0] - 0.5 * wy0, y[-1] + 0.5 * wy1, y[-1] + wy1, y[0] - wy0]]
    qx, qy = np.concatenate(qx).astype(dt), np.concatenate(qy).astype(dt)
    if not outside:
        qx, qy = np.clip(qx, x[0], x[-1]), np.clip(qy, y[0], y[-1])
    return qx, qy


def dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


# ---- tables and rows, every shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,axes", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_tables_and_rows_are_bit_exact(pkg, dt, shape, axes):
    rng = np.random.default_rng([shape[0], shape[1], shape[2], len(axes)])
    x, y, z = make_grid(rng, shape, dt, axes)
    given = given_tables(rng, z)
    qx, qy = queries(rng, x, y)
    for rule in rules_for(shape):
        ref = reference_tables(rule, x, y, z, given)
        want = bicubic_ref.evaluate(x, y, z, *ref, qx, qy)
        for device_inputs in ((True,) if axes == "offset" else (False, True)):
            it = build(pkg, rule, x, y, z, given, device_inputs, extrapolate=True, offset=axes == "offset")
            for name, g, r in zip(("zx", "zy", "zxy"), it.strategy.tables(), ref):
                check_bits(g, r, f"{rule} {name} device_inputs={device_inputs}")
            for name, g, r in zip(("zx", "zy", "zxy"), it.strategy.tables(on_device=True), ref):
                check_bits(g.cpu().numpy(), r, f"{rule} {name} to the device, device_inputs={device_inputs}")
            for path in (pkg.PATH_AUTO, pkg.PATH_GATHER):
                it.strategy.path = path
                check_bits(it.interp_array(qx, qy), want, f"{rule} rows, host queries, path={path}")
                check_bits(it.interp_array(dev(qx), dev(qy)).cpu().numpy(), want, f"{rule} rows, device queries, path={path}")


# ---- the existing kernels on these tables: partials, jet, integrals ------------------------------------------------------
@pytest.mark.parametrize("shape,rule", [(s, r) for s in DEEP for r in rules_for(s)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_partials_jet_and_integrals_are_bit_exact(pkg, dt, shape, rule):
    rng = np.random.default_rng([7, shape[0], shape[1], shape[2]])
    x, y, z = make_grid(rng, shape, dt)
    given = given_tables(rng, z)
    ref = reference_tables(rule, x, y, z, given)
    qx, qy = queries(rng, x, y)
    it = build(pkg, rule, x, y, z, given, extrapolate=True)
    with np.errstate(all="ignore"):
        rows = {o: bicubic_partial_ref.evaluate(x, y, z, *ref, qx, qy, *o) for o in bicubic_partial_ref.ORDERS}
        rows[(0, 0)] = bicubic_ref.evaluate(x, y, z, *ref, qx, qy)
    for o in bicubic_partial_ref.ORDERS:                                         # all eight orders stay allowed
        p = it.partial(*o)
        check_bits(p.interp_array(qx, qy), rows[o], f"partial {o}, host queries")
        check_bits(p.interp_array(dev(qx), dev(qy)).cpu().numpy(), rows[o], f"partial {o}, device queries")
    for order in (1, 2):
        parts = it.jet(qx, qy, order)
        dparts = it.jet(dev(qx), dev(qy), order)
        for o, a, b in zip(pkg.JET_PARTS[order], parts, dparts):
            check_bits(a, rows[o], f"jet order {order} part {o}, host")
            check_bits(b.cpu().numpy(), rows[o], f"jet order {order} part {o}, device")
    F = it.antiderivative()
    tabs = bicubic_integral_ref.tables(x, y, z, *ref)
    for name, g, r in zip(("PP", "Qz", "Qzy", "Pz", "Pzx"), F.strategy.integral_tables(), tabs):
        check_bits(g, r, f"prefix table {name}")
    nodes = (z,) + tuple(ref)
    check_bits(F.interp_array(qx, qy), bicubic_integral_ref.evaluate(x, y, nodes, tabs, qx, qy), "F, host queries")
    check_bits(F.interp_array(dev(qx), dev(qy)).cpu().numpy(), bicubic_integral_ref.evaluate(x, y, nodes, tabs, qx, qy),
               "F, device queries")
    n = len(qx) // 2
    xa, xb, ya, yb = qx[:n].copy(), qx[n:2 * n].copy(), qy[:n].copy(), qy[n:2 * n].copy()
    xb[:4] = xa[:4]                                                               # equal bounds: exactly 0
    yb[4:8] = ya[4:8]
    xa[8:12], xb[8:12] = np.maximum(xa[8:12], xb[8:12]) + 0, np.minimum(xa[8:12], xb[8:12]) + 0   # reversed
    want = bicubic_integral_ref.rectangle(x, y, nodes, tabs, xa, xb, ya, yb)
    got = F.integral(xa, xb, ya, yb)
    check_bits(got, want, "rectangles, host bounds")
    check_bits(F.integral(dev(xa), dev(xb), dev(ya), dev(yb)).cpu().numpy(), want, "rectangles, device bounds")
    assert np.all(got[:8] == 0)
    swapped = F.integral(xb, xa, ya, yb)
    check_bits(swapped, bicubic_integral_ref.rectangle(x, y, nodes, tabs, xb, xa, ya, yb), "rectangles, x bounds swapped")
    assert np.array_equal(swapped[8:], -got[8:], equal_nan=True), "swapped bounds negate"


# ---- the grid-line identity against a 1-D handle on the device ------------------------------------------------------------
@pytest.mark.parametrize("rule", ["pchip", "akima"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_grid_lines_are_the_1d_handles_rows(pkg, dt, rule):
    """On x = x[i] the surface is what a 1-D Pchip / Akima handle of the column z[i][:] evaluates (t == 0; t == 1 on the
    last line), and likewise along y: the 2-D stencil and the 1-D build choose the same bits."""
    strat1d = {"pchip": pkg.Pchip, "akima": pkg.Akima}[rule]
    rng = np.random.default_rng(19)
    for shape in ((2, 5, 1), (4, 3, 2), (7, 5, 4)):
        if rule not in rules_for(shape):
            continue
        x, y, z = make_grid(rng, shape, dt)
        it = build(pkg, rule, x, y, z)
        qy = np.sort(np.concatenate([rng.uniform(y[0], y[-1], 50).astype(dt), y]))
        qx = np.sort(np.concatenate([rng.uniform(x[0], x[-1], 50).astype(dt), x]))
        for i in range(shape[0]):
            line = pkg.Interp1DBuilder.new(np.ascontiguousarray(z[i])).x(y).strategy(strat1d.new()).build()
            check_bits(it.interp_array(np.full(len(qy), x[i], dt), qy), line.interp_array(qy), f"{shape}: line x[{i}]")
        for j in range(shape[1]):
            line = pkg.Interp1DBuilder.new(np.ascontiguousarray(z[:, j])).x(x).strategy(strat1d.new()).build()
            check_bits(it.interp_array(qx, np.full(len(qx), y[j], dt)), line.interp_array(qx), f"{shape}: line y[{j}]")


# ---- hostile data -----------------------------------------------------------------------------------------------------------
def subnormal_axis(n, dt):
    """spacings that are subnormal numbers (3, 5, 3, 5 ... units of the smallest subnormal from 0)"""
    steps = np.where(np.arange(n) % 2 == 0, 3.0, 5.0)
    return (np.concatenate([[0.0], np.cumsum(steps[:n - 1])]) * float(np.finfo(dt).smallest_subnormal)).astype(dt)


HOSTILE_N, HOSTILE_OTHER, HOSTILE_C = 7, 6, 4


def hostile_grids(rule, dt):
    """(tag, x, y, z): the 1-D hostile recipes of tests/hostile_inputs.py -- NaN and +-inf nodes, flat runs and signed zeros,
    sign changes, exact s == 0 for Akima, the scale recipes on every knot kind -- laid along x, then along y, of a
    7 x 6 x 4 / 6 x 7 x 4 grid; and both on an axis of subnormal spacings."""
    n, m, C = HOSTILE_N, HOSTILE_OTHER, HOSTILE_C
    other = hostile_inputs.knots("uneven", dt, m, seed=3)
    for tag, k, cols, _ in hostile_inputs.cases(rule, dt, n, m * C):
        yield tag + " along x", k, other, np.ascontiguousarray(cols.reshape(n, m, C))
        yield tag + " along y", other, k, np.ascontiguousarray(cols.reshape(n, m, C).transpose(1, 0, 2))
    k, cols, _ = hostile_inputs.generate(rule, dt, n, m * C, ("branch", "zero"), "even", 0)
    sub = subnormal_axis(n, dt)
    yield "subnormal spacings along x", sub, other, np.ascontiguousarray(cols.reshape(n, m, C))
    yield "subnormal spacings along y", other, sub, np.ascontiguousarray(cols.reshape(n, m, C).transpose(1, 0, 2))
    yield "subnormal spacings on both axes", sub, subnormal_axis(m, dt), np.ascontiguousarray(cols.reshape(n, m, C))


@pytest.mark.parametrize("rule", ["pchip", "akima"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_hostile_data_gives_the_restatements_tables(pkg, dt, rule):
    seen = 0
    for tag, x, y, z in hostile_grids(rule, dt):
        with np.errstate(all="ignore"):
            ref = bicubic_local_ref.tables(rule, x, y, z)
        it = build(pkg, rule, x, y, z)
        for name, g, r in zip(("zx", "zy", "zxy"), it.strategy.tables(), ref):
            check_bits(g, r, f"{tag}: {name}")            # bitwise; NaN compared as positions
        seen += 1
    assert seen >= 20


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_hostile_given_tables_come_back_bit_for_bit(pkg, dt):
    """No rule is applied to the caller's tables: NaN payloads, infinities, signed zeros and subnormals included, the bytes
    that went in come out, from host and from device arrays."""
    rng = np.random.default_rng(23)
    x, y, z = make_grid(rng, (5, 6, 3), dt)
    given = list(given_tables(rng, z))
    T = np.dtype(dt).type
    given[0][1, 2] = [np.nan, np.inf, -np.inf]
    given[1][0, 0] = [-0.0, 0.0, np.finfo(dt).smallest_subnormal]
    given[2][4, 5] = [np.finfo(dt).max, -np.finfo(dt).tiny, T(np.nan)]
    bits = given[0].view({4: np.uint32, 8: np.uint64}[np.dtype(dt).itemsize])
    bits[3, 3, 0] = bits[1, 2, 0] | 0x5A5                                       # a NaN with a payload
    assert np.isnan(given[0][3, 3, 0])
    for device_inputs in (False, True):
        it = build(pkg, "hermite", x, y, z, tuple(given), device_inputs)
        for name, g, r in zip(("zx", "zy", "zxy"), it.strategy.tables(), given):
            assert g.tobytes() == r.tobytes(), f"{name} device_inputs={device_inputs}"
    qx, qy = queries(rng, x, y, outside=False)
    with np.errstate(all="ignore"):
        want = bicubic_ref.evaluate(x, y, z, *given, qx, qy)
    check_bits(it.interp_array(qx, qy), want, "rows on hostile given tables")


# ---- the handle is wired: clone, trim, ring, sharded, the error semantics -------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_clone_trim_ring_sharded_and_first_error(pkg, rule):
    import torch
    rng = np.random.default_rng(31)
    shape, dt = (33, 17, 8), np.float64
    x, y, z = make_grid(rng, shape, dt)
    given = given_tables(rng, z)
    ref = reference_tables(rule, x, y, z, given)
    qx, qy = queries(rng, x, y, extra=2000, outside=False)
    nq = len(qx)
    want = bicubic_ref.evaluate(x, y, z, *ref, qx, qy)
    it = build(pkg, rule, x, y, z, given)
    rep = it.replicate([0])[0]                                                   # clone: the table is copied, no rebuild
    for a, b in zip(rep.strategy.tables(), ref):
        check_bits(a, b, "clone: tables")
    check_bits(rep.interp_array(qx, qy), want, "clone: rows")
    it.strategy.trim()
    check_bits(it.interp_array(qx, qy), want, "rows after trim")
    got = np.zeros_like(want)                                                    # ring: 2 slots, 1000 does not divide nq
    ring = pkg.striped_ring(1000, shape[2], 2, dt, 0)

    def consumer(c, rows):
        got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
    it.interp_array_ring(dev(qx), dev(qy), 1000, consumer, slots=ring)
    check_bits(got, want, "ring")
    reps = [it, build(pkg, rule, x, y, z, given)]                                # sharded: two replicas on one device
    got = np.full_like(want, -1.0)
    pkg.sharding.interp_array_sharded(reps, qx, qy, out=got)
    check_bits(got, want, "sharded")
    spline = pkg.Interp2DBuilder.new(z).x(x).y(y).strategy(pkg.Bicubic.new()).build()
    got = np.full_like(want, -1.0)                                               # the rule is not part of the signature
    pkg.sharding.interp_array_sharded([it, spline], qx[:8], qy[:8], out=got[:8])
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    with pytest.raises(Exception, match="replicas of one interpolator"):
        pkg.sharding.interp_array_sharded([it, bil], qx, qy, out=got)
    it.strategy.path = pkg.PATH_BUCKETED
    try:
        with pytest.raises(Exception, match="Bicubic has no tile-grouped evaluation form"):
            it.interp_array(qx, qy)
    finally:
        it.strategy.path = pkg.PATH_AUTO
    # first error, and the rows before it: Bilinear's report on the same queries
    pos = nq // 2
    bx, by = qx.copy(), qy.copy()
    by[pos] = y[-1] + 0.5
    bx[pos + 3] = np.nan                                                         # a later failure is not the one reported
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e_bil:
        bil.interp_array(bx, by)
    for q in ((bx, by), (dev(bx), dev(by))):
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array(*q)
        assert (str(e.value), e.value.index, e.value.axis) == (str(e_bil.value), pos, 1)
    for buf in (np.full((nq, shape[2]), -7.0), torch.full((nq, shape[2]), -7.0, dtype=torch.float64, device="cuda:0")):
        q = (bx, by) if isinstance(buf, np.ndarray) else (dev(bx), dev(by))
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array_into(*q, buf)
        assert e.value.index == pos
        rows = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
        check_bits(rows[:pos], want[:pos], "rows before the failure")
        assert np.all(rows[pos:] == -7.0), "rows from the failure on keep the sentinel"


# ---- the bounds-checked library -------------------------------------------------------------------------------------------
def test_build_shapes_run_clean_under_the_bounds_checked_library():
    """Every NDI_CHK of the stencil, on every build shape and both dtypes, in a fresh child process that loads the checked
    library: a violation would come back as a DeviceError from the create call."""
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import bicubic_ref, test_gpu_bicubic_local as t\n"
        "from hostile_inputs import check_bits\n"
        "pkg = load_product_package()\n"
        "assert pkg._capi.LIB_PATH.endswith('libndinterp_hip_dbg.so'), pkg._capi.LIB_PATH\n"
        "for dt in t.DTYPES:\n"
        "    for shape, axes in t.SHAPES:\n"
        "        rng = np.random.default_rng(shape)\n"
        "        x, y, z = t.make_grid(rng, shape, dt, axes)\n"
        "        given = t.given_tables(rng, z)\n"
        "        qx, qy = t.queries(rng, x, y)\n"
        "        for rule in t.rules_for(shape):\n"
        "            ref = t.reference_tables(rule, x, y, z, given)\n"
        "            it = t.build(pkg, rule, x, y, z, given, device_inputs=True, extrapolate=True, offset=axes == 'offset')\n"
        "            for a, b in zip(it.strategy.tables(), ref): check_bits(a, b, 'tables')\n"
        "            check_bits(it.interp_array(qx, qy), bicubic_ref.evaluate(x, y, z, *ref, qx, qy), 'rows')\n"
        "print('checked OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDI_LIB=lib), timeout=600)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- indices beyond 32 bits ---------------------------------------------------------------------------------------------------
def test_table_beyond_2_to_32_elements(pkg):
    """3 x 3 x 2^27 f32 with Akima: the grid is 4.8 GB, the node table 19 GB -- the stencil takes its 64-bit index branch and
    record offsets pass 2^32 elements.  Lanes are independent, so the restatement runs on a sample of lanes only."""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    assert free > 90 * 2**30, "the test needs 90 GB of free device memory"
    C = 1 << 27
    x = np.array([0.0, 1.0, 2.5], np.float32)
    y = np.array([-1.0, 0.5, 1.0], np.float32)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    z = torch.rand((3, 3, C), dtype=torch.float32, device="cuda:0", generator=g)
    m = (1 << 32) // 36
    lanes = np.array([0, 1, 2, 3] + list(range(m - 2, m + 3)) + list(range(C - 4, C)))
    sel = torch.as_tensor(lanes, device="cuda:0")
    it = pkg.Interp2DBuilder.new(z).x(dev(x)).y(dev(y)).strategy(pkg.Bicubic.akima()).build()
    zs = z[:, :, sel].cpu().numpy()
    del z
    tabs = it.strategy.tables(on_device=True)
    got = [t[:, :, sel].cpu().numpy() for t in tabs]
    del tabs
    ref = bicubic_local_ref.tables("akima", x, y, zs)
    for name, a, b in zip(("zx", "zy", "zxy"), got, ref):
        check_bits(a, b, name)
    rng = np.random.default_rng(2)
    qx, qy = queries(rng, x, y, extra=4, outside=False)
    rows = it.interp_array(dev(qx[:16]), dev(qy[:16]))
    check_bits(rows[:, sel].cpu().numpy(), bicubic_ref.evaluate(x, y, zs, *ref, qx[:16], qy[:16]), "rows")
    del rows
    it.strategy.release()
    torch.cuda.empty_cache()
