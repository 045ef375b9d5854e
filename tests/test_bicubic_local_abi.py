"""CPU: Bicubic with Pchip / Akima / caller-given node derivatives at the boundary -- the two new entry points in the
header, the ctypes binding, the built library, the Rust declarations and the C++ mirror; every refusal that needs no device;
the numpy restatement (tests/bicubic_local_ref.py, what the GPU tests compare the device against bit for bit) against scipy
through tests/golden/bicubic_local_scipy.npz (tests/golden/gen_bicubic_local_golden.py); and the properties the header
states, on the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bicubic_integral_ref
import bicubic_local_ref
import bicubic_partial_ref
import bicubic_ref
import hermite_ref
from conftest import GOLDEN, ROOT
from hostile_inputs import check_bits

DTYPES = [np.float64, np.float32]
# shapes of the grid-line identity: the smallest grid of each rule up to 33 x 17 x 4
SHAPES = [(2, 2, 1), (2, 5, 1), (5, 2, 2), (3, 3, 1), (4, 3, 2), (5, 6, 3), (7, 5, 4), (33, 17, 4)]


def golden():
    return np.load(os.path.join(GOLDEN, "bicubic_local_scipy.npz"))


def make_grid(rng, nx, ny, Cn, dt):
    x = np.cumsum(rng.uniform(0.5, 1.5, nx)).astype(dt)
    y = np.cumsum(rng.uniform(0.5, 1.5, ny)).astype(dt)
    return x, y, rng.normal(size=(nx, ny, Cn)).astype(dt)


def desc_for(cap, x, y, z, dtype=None):
    d = cap.Interp2DDesc()
    d.dtype = cap.F64 if dtype is None else dtype
    d.memspace = cap.MEM_HOST
    d.nx, d.ny, d.lanes = z.shape
    d.x_len, d.y_len = len(x), len(y)
    d.x, d.y, d.data = x.ctypes.data, y.ctypes.data, z.ctypes.data
    d.validate = 1
    return d


def grid(nx=4, ny=5, Cn=2, dt=np.float64):
    return np.arange(nx, dtype=dt), np.arange(ny, dtype=dt), np.zeros((nx, ny, Cn), dt)


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_library_rust_and_docs_carry_both_symbols(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert ("ndi_status ndi_interp2d_create_bicubic_local(const ndi_interp2d_desc* desc, int32_t rule, ndi_interp2d** out);"
            in header)
    assert ("ndi_status ndi_interp2d_create_bicubic_hermite(const ndi_interp2d_desc* desc, const void* zx, const void* zy,\n"
            "                                               const void* zxy, ndi_interp2d** out);") in header
    for text in ("zx  = RULE(x, .) on z viewed as (nx, ny C)", "zy  = RULE(y, .) on each z[i] viewed as (ny, C)",
                 "zxy = RULE(y, .) on each zx[i] viewed as (ny, C)", "Grid-line property", "Monotonicity INSIDE a cell is NOT promised",
                 "C1, not C2", "Pchip 2, Akima 3, caller-given 2"):
        assert text in header, text
    assert "Pchip / Akima node derivatives" not in header          # no longer under "Not provided"
    lib = C.CDLL(cap.LIB_PATH)
    for name in ("ndi_interp2d_create_bicubic_local", "ndi_interp2d_create_bicubic_hermite"):
        assert name in cap.SYMBOLS and hasattr(lib, name), name
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp2d_create_bicubic_local(" in rust and "pub fn ndi_interp2d_create_bicubic_hermite(" in rust
    assert cap.lib().ndi_version() == (0 << 16) | 5     # two new symbols, no new enumerator: no version change
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "ndi_interp2d_create_bicubic_local" in text and "ndi_interp2d_create_bicubic_hermite" in text, doc
    B = pkg.Bicubic
    assert (B.pchip().MINIMUM_DATA_LENGHT, B.akima().MINIMUM_DATA_LENGHT, B.MINIMUM_DATA_LENGHT) == (2, 3, 3)
    z = np.zeros((2, 2))
    assert B.hermite(z, z, z).MINIMUM_DATA_LENGHT == 2 and B.new().rule is None
    assert all(isinstance(s, B) for s in (B.pchip(), B.akima(), B.hermite(z, z, z)))   # one class: partial, jet ... are shared


def test_refusals_come_back_without_a_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    x, y, z = grid()
    local, herm = lib.ndi_interp2d_create_bicubic_local, lib.ndi_interp2d_create_bicubic_hermite
    h = C.c_void_p(1234)
    assert local(None, cap.PCHIP, C.byref(h)) == cap.BAD_ARG and cap.last_error() == "null argument"
    assert local(C.byref(desc_for(cap, x, y, z)), cap.PCHIP, None) == cap.BAD_ARG and cap.last_error() == "null argument"
    assert herm(None, z.ctypes.data, z.ctypes.data, z.ctypes.data, C.byref(h)) == cap.BAD_ARG
    assert herm(C.byref(desc_for(cap, x, y, z)), z.ctypes.data, z.ctypes.data, z.ctypes.data, None) == cap.BAD_ARG
    for rule in (cap.LINEAR, cap.CUBIC_SPLINE, cap.CUBIC_HERMITE, -1, 99):
        h = C.c_void_p(1234)
        assert local(C.byref(desc_for(cap, x, y, z)), rule, C.byref(h)) == cap.BAD_ARG
        assert "Bicubic" in cap.last_error() and "NDI_PCHIP or NDI_AKIMA" in cap.last_error() and f"got {rule}" in cap.last_error()
        assert h.value is None                                                   # *out is cleared
    for name, rule in (("Pchip", cap.PCHIP), ("Akima", cap.AKIMA)):
        for dtype in (cap.I32, cap.I64, cap.F16, cap.BF16):
            h = C.c_void_p(1234)
            assert local(C.byref(desc_for(cap, x, y, z, dtype)), rule, C.byref(h)) == cap.BAD_ARG
            assert cap.last_error().startswith(f"Bicubic ({name}) needs") and h.value is None
    for dtype in (cap.I32, cap.I64, cap.F16, cap.BF16):
        assert herm(C.byref(desc_for(cap, x, y, z, dtype)), z.ctypes.data, z.ctypes.data, z.ctypes.data, C.byref(h)) == cap.BAD_ARG
        assert cap.last_error().startswith("Bicubic (Hermite) needs")
    for k, name in enumerate(("zx", "zy", "zxy")):
        tabs = [z.ctypes.data] * 3
        tabs[k] = None
        h = C.c_void_p(1234)
        assert herm(C.byref(desc_for(cap, x, y, z)), *tabs, C.byref(h)) == cap.BAD_ARG
        assert cap.last_error().startswith("Bicubic (Hermite) needs all three") and f"{name} is null" in cap.last_error()
        assert h.value is None
    # fewer points than the rule needs: the message gives the rule, the need and the shape
    for (nx, ny) in ((2, 5), (5, 2), (2, 2)):
        x2, y2, z2 = grid(nx, ny)
        assert local(C.byref(desc_for(cap, x2, y2, z2)), cap.AKIMA, C.byref(h)) == cap.NOT_ENOUGH_DATA
        assert cap.last_error() == f"Bicubic (Akima) needs at least 3 data points on each axis (got {nx} x {ny})"
    x1, y1, z1 = grid(1, 5)
    d = desc_for(cap, x1, y1, z1)
    d.validate = 0
    assert local(C.byref(d), cap.PCHIP, C.byref(h)) == cap.NOT_ENOUGH_DATA
    assert cap.last_error() == "Bicubic (Pchip) needs at least 2 data points on each axis (got 1 x 5)"
    assert herm(C.byref(d), z1.ctypes.data, z1.ctypes.data, z1.ctypes.data, C.byref(h)) == cap.NOT_ENOUGH_DATA
    assert cap.last_error() == "Bicubic (Hermite) needs at least 2 data points on each axis (got 1 x 5)"
    # validate behaves as in ndi_interp2d_create_bicubic: the builder's own errors, before the strategy's
    xb = np.array([0.0, 2.0, 1.0, 3.0])
    assert local(C.byref(desc_for(cap, xb, y, z)), cap.PCHIP, C.byref(h)) == cap.MONOTONIC
    assert lib.ndi_interp2d_create_bicubic(C.byref(desc_for(cap, xb, y, z)), None, C.byref(h)) == cap.MONOTONIC


def test_the_python_mirror_refuses_before_the_library(pkg):
    B, IB = pkg.Bicubic, pkg.Interp2DBuilder
    z = np.zeros((4, 5, 2))
    for s in (B.pchip(), B.akima(), B.hermite(z, z, z)):
        for call in (s.boundary, s.boundary_x, s.boundary_y):
            with pytest.raises(TypeError, match="takes no boundary conditions: ends are a spline notion"):
                call(pkg.BoundaryCondition.Natural)
    B.new().boundary(pkg.BoundaryCondition.Natural)                  # the spline keeps them
    for shape, dim in (((2, 5), 0), ((5, 2), 1)):
        with pytest.raises(pkg.BuilderError.NotEnoughData, match=f"The {dim}-dimension has not enough data.*Provided: 2, Reqired: 3"):
            IB.new(np.zeros(shape)).strategy(B.akima()).build()
    with pytest.raises(pkg.BuilderError.NotEnoughData, match="Provided: 1, Reqired: 2"):
        IB.new(np.zeros((1, 5))).strategy(B.pchip()).build()
    with pytest.raises(pkg.BuilderError.NotEnoughData, match="Provided: 2, Reqired: 3"):
        IB.new(np.zeros((2, 5))).strategy(B.new()).build()           # the spline's minimum stays 3
    for dt in (np.int32, np.int64, np.float16):
        for s in (B.pchip(), B.akima(), B.hermite(np.zeros((3, 3), dt), np.zeros((3, 3), dt), np.zeros((3, 3), dt))):
            with pytest.raises(TypeError, match="Bicubic covers float32/float64 only"):
                IB.new(np.zeros((3, 3), dt)).strategy(s).build()
    for k, name in enumerate(("zx", "zy", "zxy")):
        tabs = [np.zeros((4, 5, 2))] * 3
        tabs[k] = np.zeros((4, 5, 3))
        with pytest.raises(pkg.BuilderError.ShapeError, match=rf"{name} has wrong shape. Expected: \[4, 5, 2\], got: \[4, 5, 3\]"):
            IB.new(z).strategy(B.hermite(*tabs)).build()
        tabs[k] = np.zeros((4, 5, 2), np.float32)
        with pytest.raises(TypeError, match=f"Bicubic.hermite: {name} has element type float32, the data is float64"):
            IB.new(z).strategy(B.hermite(*tabs)).build()
        tabs[k] = [[0.0]]
        with pytest.raises(TypeError, match=f"Bicubic.hermite: {name} is a numpy array or a tensor, got list"):
            IB.new(z).strategy(B.hermite(*tabs)).build()


def test_building_without_a_gpu_is_a_loud_device_error(pkg):
    z = np.zeros((4, 4))
    for s in (pkg.Bicubic.pchip, pkg.Bicubic.akima, lambda: pkg.Bicubic.hermite(z, z, z)):
        build = pkg.Interp2DBuilder.new(z).strategy(s()).build
        if pkg.device_count() > 0:      # with a device the same call builds (tests/test_gpu_bicubic_local.py has the rest)
            assert isinstance(build().strategy, pkg.Bicubic)
            continue
        with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
            build()


def test_cpp_mirror_compiles_and_refuses_the_same(pkg, tmp_path):
    libdir = os.path.join(ROOT, "ndarray-interp_amd")
    exe = str(tmp_path / "test_bicubic_local_mirror")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "test_bicubic_local_mirror.cpp"), "-L", libdir, "-lndinterp_hip",
                        "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "OK" in run.stdout, run.stdout + run.stderr


# ---- the restatement against scipy --------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", bicubic_local_ref.RULES)
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_restatement_matches_scipy(rule, dt):
    """Tolerance as test_restatement_matches_scipy of tests/test_hermite_abi.py: 4 x the largest deviation the generator
    measured over the file (relative to max|z| + 1); the bound itself stays below 1e-13 (f64) / 2e-5 (f32)."""
    g = golden()
    name = np.dtype(dt).name
    bound = 4.0 * float(g[f"deviation/{name}/{rule}"])
    assert bound < (1e-13 if dt == np.float64 else 2e-5)
    worst, seen, shapes = 0.0, 0, set()
    for cid in g["cases"]:
        if not cid.startswith(name) or f"{cid}/{rule}/z" not in g:
            continue
        x, y, z = g[cid + "/x"], g[cid + "/y"], g[f"{cid}/{rule}/z"]
        got = bicubic_local_ref.tables(rule, x, y, z)
        scale = np.abs(z.astype(np.float64)).max() + 1
        for tab, t in zip(("zx", "zy", "zxy"), got):
            assert t.dtype == np.dtype(dt) and t.shape == z.shape
            dev = float(np.abs(t.astype(np.float64) - g[f"{cid}/{rule}/{tab}"]).max() / scale)
            worst = max(worst, dev)
            assert dev <= bound, (cid, tab, dev, bound)
        seen += 1
        shapes.add(z.shape)
    assert seen == (8 if rule == "pchip" else 5) and (33, 17, 4) in shapes
    assert (rule == "pchip") == ((2, 2, 1) in shapes)
    print(f"{name} {rule}: largest deviation from scipy {worst:.3e}, bound {bound:.3e}")
    assert os.path.getsize(os.path.join(GOLDEN, "bicubic_local_scipy.npz")) <= 512 * 1024


def test_the_golden_tells_a_wrong_composition_from_the_contract():
    """The cross table is RULE(y, .) of zx.  A nonlinear rule does not commute with itself across the axes: RULE(x, .) of zy
    -- the same number for the spline -- misses the golden zxy by orders of magnitude more than the bound, and so does
    zxy = 0."""
    g = golden()
    cid = "float64_33x17x4"
    x, y, z = g[cid + "/x"], g[cid + "/y"], g[cid + "/pchip/z"]
    bound = 4.0 * float(g["deviation/float64/pchip"])
    assert np.abs(g[cid + "/pchip/zxy"]).max() / (np.abs(z).max() + 1) > 1e6 * bound
    zx, zy, zxy = bicubic_local_ref.tables("pchip", x, y, z)
    other = hermite_ref.pchip_k(x, zy.reshape(33, -1)).reshape(z.shape)      # along x of zy: another composition
    assert np.abs(other - g[cid + "/pchip/zxy"]).max() / (np.abs(z).max() + 1) > 1e6 * bound


# ---- properties on the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", bicubic_local_ref.RULES)
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_grid_lines_are_the_1d_strategy_bit_for_bit(rule, dt):
    """On x = x[i] the surface is the 1-D strategy's interpolant of z[i][:], and likewise along y: t == 0 on every line but
    the last, t == 1 there."""
    rng = np.random.default_rng(77)
    for nx, ny, Cn in SHAPES:
        if min(nx, ny) < bicubic_local_ref.MINIMUM[rule]:
            continue
        x, y, z = make_grid(rng, nx, ny, Cn, dt)
        zx, zy, zxy = bicubic_local_ref.tables(rule, x, y, z)
        qy = np.sort(np.concatenate([rng.uniform(y[0], y[-1], 40).astype(dt), y]))
        qx = np.sort(np.concatenate([rng.uniform(x[0], x[-1], 40).astype(dt), x]))
        for i in range(nx):
            a, b = hermite_ref.build(rule, y, z[i])
            got = bicubic_ref.evaluate(x, y, z, zx, zy, zxy, np.full(len(qy), x[i], dt), qy)
            check_bits(got, hermite_ref.evaluate(y, z[i], a, b, qy), f"{rule} {nx}x{ny}x{Cn}: line x[{i}]")
        for j in range(ny):
            col = np.ascontiguousarray(z[:, j])
            a, b = hermite_ref.build(rule, x, col)
            got = bicubic_ref.evaluate(x, y, z, zx, zy, zxy, qx, np.full(len(qx), y[j], dt))
            check_bits(got, hermite_ref.evaluate(x, col, a, b, qx), f"{rule} {nx}x{ny}x{Cn}: line y[{j}]")


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_pchip_on_a_monotone_step_table(dt):
    """A table that rises in steps with plateaus along both axes: along every grid line the Pchip surface stays monotone
    and inside the line's range, and the node derivatives on the plateaus are +0."""
    steps = np.array([0, 0, 0, 1, 1, 1, 5, 5, 6, 6], dtype=dt)
    x = np.cumsum(np.array([1, 0.5, 2, 1, 1, 0.25, 3, 1, 1, 2], dtype=dt))
    y = np.arange(10).astype(dt)
    z = (steps[:, None] + 2 * steps[None, :])[:, :, None].astype(dt)
    zx, zy, zxy = bicubic_local_ref.tables("pchip", x, y, z)
    # every knot of `steps` has a zero slope on one side at least: every k is +0
    for t in (zx, zy, zxy):
        assert np.all(t == 0) and not np.any(np.signbit(t)), "+0 derivatives on plateaus"
    # "No overshoot" is a property of the polynomial; the evaluated form rounds.  On a grid line the outer form is exact
    # (t == 0: 1 * p0 + 0 * p1 + 0), the inner one is five roundings of numbers no larger than max|z| -- (1-s) pl, s pr, their
    # sum, the correction, the last sum -- half an ulp each: 4 ulp of max|z| covers it.
    slack = 4 * np.finfo(dt).eps * np.abs(z).max()

    def monotone_inside(v, line, what):
        assert np.all(np.diff(v) >= -slack) and v.min() >= line.min() - slack and v.max() <= line.max() + slack, what
    q = np.linspace(0, 1, 401)
    for i in range(10):
        qy = (y[0] + q * (y[-1] - y[0])).astype(dt)
        monotone_inside(bicubic_ref.evaluate(x, y, z, zx, zy, zxy, np.full(len(qy), x[i], dt), qy)[:, 0], z[i], f"line x[{i}]")
        qx = (x[0] + q * (x[-1] - x[0])).astype(dt)
        monotone_inside(bicubic_ref.evaluate(x, y, z, zx, zy, zxy, qx, np.full(len(qx), y[i], dt))[:, 0], z[:, i], f"line y[{i}]")
    # a table with strict rises between the plateaus: interior derivatives are non-negative, plateau nodes +0
    ramp = np.array([0, 0, 1, 3, 3, 4, 7, 7, 7, 9], dtype=dt)
    z2 = (ramp[:, None] + ramp[None, :])[:, :, None].astype(dt)
    zx, zy, zxy = bicubic_local_ref.tables("pchip", x, y, z2)
    assert np.all(zx >= 0) and np.all(zy >= 0) and not np.any(np.signbit(zx)) and not np.any(np.signbit(zy))
    assert np.all(zx[[0, 1, 3, 4, 6, 7, 8]] == 0) and np.all(zy[:, [0, 1, 3, 4, 6, 7, 8]] == 0)
    for i in range(10):
        qy = (y[0] + q * (y[-1] - y[0])).astype(dt)
        slack = 4 * np.finfo(dt).eps * np.abs(z2).max()
        monotone_inside(bicubic_ref.evaluate(x, y, z2, zx, zy, zxy, np.full(len(qy), x[i], dt), qy)[:, 0], z2[i], f"ramp: line x[{i}]")


def test_hermite_tables_of_a_bicubic_polynomial_reproduce_it():
    """p(x, y) bicubic: with its own zx, zy, zxy at the nodes every cell's Hermite patch IS p -- the value, the partials
    and the rectangle integral, to rounding."""
    x = np.array([0.0, 0.7, 1.1, 2.0])
    y = np.array([-1.0, -0.2, 1.0])
    X, Y = x[:, None], y[None, :]
    p = lambda u, v: u ** 3 - 2.0 * u * v * v + v ** 3 * u * u + 1.0               # noqa: E731
    px = lambda u, v: 3.0 * u ** 2 - 2.0 * v * v + 2.0 * v ** 3 * u               # noqa: E731
    py = lambda u, v: -4.0 * u * v + 3.0 * v ** 2 * u * u                          # noqa: E731
    pxy = lambda u, v: -4.0 * v + 6.0 * v ** 2 * u                                 # noqa: E731
    P = lambda u, v: u ** 4 * v / 4.0 - u * u * v ** 3 / 3.0 + u ** 3 * v ** 4 / 12.0 + u * v   # noqa: E731
    z, zx, zy, zxy = (np.ascontiguousarray((f(X, Y) + 0.0 * X * Y)[:, :, None]) for f in (p, px, py, pxy))
    rng = np.random.default_rng(5)
    qx, qy = rng.uniform(x[0], x[-1], 500), rng.uniform(y[0], y[-1], 500)
    assert np.abs(bicubic_ref.evaluate(x, y, z, zx, zy, zxy, qx, qy)[:, 0] - p(qx, qy)).max() <= 1e-13
    assert np.abs(bicubic_partial_ref.evaluate(x, y, z, zx, zy, zxy, qx, qy, 1, 0)[:, 0] - px(qx, qy)).max() <= 1e-12
    assert np.abs(bicubic_partial_ref.evaluate(x, y, z, zx, zy, zxy, qx, qy, 0, 1)[:, 0] - py(qx, qy)).max() <= 1e-12
    assert np.abs(bicubic_partial_ref.evaluate(x, y, z, zx, zy, zxy, qx, qy, 1, 1)[:, 0] - pxy(qx, qy)).max() <= 1e-12
    tabs = bicubic_integral_ref.tables(x, y, z, zx, zy, zxy)
    xa, xb, ya, yb = qx[:250], qx[250:], qy[:250], qy[250:]
    want = (P(xb, yb) - P(xa, yb)) - (P(xb, ya) - P(xa, ya))
    got = bicubic_integral_ref.rectangle(x, y, (z, zx, zy, zxy), tabs, xa, xb, ya, yb)[:, 0]
    assert np.abs(got - want).max() <= 1e-13
