"""CPU: the Bicubic strategy at the boundary -- the two new entry points in the header, the ctypes binding, the built
library and the Rust declarations; the builder errors and the refusals that need no device; and the accuracy of the
numerical contract's numpy restatement (tests/bicubic_ref.py, what the GPU tests compare the device against bit for bit)
against scipy through tests/golden/bicubic_scipy.npz (tests/golden/gen_bicubic_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import bicubic_ref
import oracle
from conftest import GOLDEN, ROOT

# class -> the contract's four ends (the generator's CLASSES)
NK = (oracle.BC_NOT_A_KNOT, 0.0)
ENDS = {
    "nat": ((oracle.BC_NATURAL, 0.0),) * 4,
    "cl": ((oracle.BC_CLAMPED, 0.0),) * 4,
    "mix": ((oracle.BC_FIRST_DERIV, 0.3), (oracle.BC_SECOND_DERIV, -0.2), (oracle.BC_FIRST_DERIV, 0.7),
            (oracle.BC_SECOND_DERIV, 0.4)),
    "n3": (NK,) * 4,
    "nk": (NK,) * 4,
}

# Largest error of the restatement against f64 scipy over the golden file, max abs error / (max |z| + 1), as
# tests/golden/gen_bicubic_golden.py measured and printed it; the bar is 2 x each (the project's margin in
# test_derivative_abi.py: it covers a numpy build that orders an operation differently, not algorithmic drift).
MEASURED = {
    ("float64", "nk"): 6.739e-14, ("float64", "nat"): 1.512e-14, ("float64", "cl"): 1.360e-14,
    ("float64", "mix"): 1.512e-14, ("float64", "n3"): 2.432e-15,
    ("float32", "nk"): 3.283e-06, ("float32", "nat"): 3.283e-06, ("float32", "cl"): 3.283e-06,
    ("float32", "mix"): 3.283e-06, ("float32", "n3"): 4.718e-07,
}


def golden():
    return np.load(os.path.join(GOLDEN, "bicubic_scipy.npz"))


def grid(nx=4, ny=5, C=2, dt=np.float64):
    return np.arange(nx, dtype=dt), np.arange(ny, dtype=dt), np.zeros((nx, ny, C), dt)


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_library_and_rust_carry_both_symbols(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert "ndi_status ndi_interp2d_create_bicubic(const ndi_interp2d_desc* desc, const ndi_boundary* bc, ndi_interp2d** out);" in header
    assert "ndi_status ndi_interp2d_tables(const ndi_interp2d* h, void* zx, void* zy, void* zxy, int32_t memspace);" in header
    for text in ("zx[i]    = (dz + a[i]) / dx", "zx[nx-1] = (dz - b[nx-2]) / dx", "result = H(p0, p1, d0, d1, hx, t)",
                 "d = pr - pl;  a = kl h - d;  b = d - kr h;", "REFERENCE operation order", "T[nx][ny][4][C]"):
        assert text in header, text
    lib = C.CDLL(cap.LIB_PATH)
    for name in ("ndi_interp2d_create_bicubic", "ndi_interp2d_tables"):
        assert name in cap.SYMBOLS and hasattr(lib, name), name
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp2d_create_bicubic(" in rust and "bc: *const ndi_boundary," in rust
    assert "pub fn ndi_interp2d_tables(" in rust
    assert cap.lib().ndi_version() == (0 << 16) | 5     # two new symbols, no new enumerator: no version change
    assert pkg.Bicubic.MINIMUM_DATA_LENGHT == 3
    assert issubclass(pkg.Bicubic, pkg.Interp2DStrategyBuilder) and issubclass(pkg.Bicubic, pkg.Interp2DStrategy)
    for m in ("interp_array_into", "finish", "clone", "interp_array_ring", "interp_into", "trim"):   # shared, not copied
        assert getattr(pkg.Bicubic, m) is getattr(pkg.Bilinear, m), m
    assert callable(pkg.Bicubic.tables) and "Bicubic" in pkg.__all__


def test_builder_errors_come_through_the_2d_builder(pkg):
    B = pkg.Interp2DBuilder
    for shape, dim in (((2, 5), 0), ((5, 2), 1)):
        with pytest.raises(pkg.BuilderError.NotEnoughData, match=f"The {dim}-dimension has not enough data.*Provided: 2, Reqired: 3"):
            B.new(np.zeros(shape)).strategy(pkg.Bicubic.new()).build()
    B.new(np.zeros((2, 5)))                                      # (Bilinear's minimum stays 2)
    with pytest.raises(pkg.BuilderError.Monotonic, match="x-axis"):
        B.new(np.zeros((3, 3))).x(np.array([0.0, 2.0, 1.0])).strategy(pkg.Bicubic.new()).build()
    with pytest.raises(pkg.BuilderError.Monotonic, match="y-axis"):
        B.new(np.zeros((3, 3))).y(np.array([0.0, 1.0, 1.0])).strategy(pkg.Bicubic.new()).build()
    with pytest.raises(pkg.BuilderError.ShapeError, match="x-axis and data-0-axis"):
        B.new(np.zeros((3, 3))).x(np.arange(4.0)).strategy(pkg.Bicubic.new()).build()
    with pytest.raises(pkg.BuilderError.ShapeError, match="at least 2"):
        B.new(np.zeros(3)).strategy(pkg.Bicubic.new()).build()


def desc_for(cap, x, y, z, dtype=None):
    d = cap.Interp2DDesc()
    d.dtype = cap.F64 if dtype is None else dtype
    d.memspace = cap.MEM_HOST
    d.nx, d.ny, d.lanes = z.shape
    d.x_len, d.y_len = len(x), len(y)
    d.x, d.y, d.data = x.ctypes.data, y.ctypes.data, z.ctypes.data
    d.validate = 1
    return d


def test_refusals_come_back_without_a_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    x, y, z = grid()
    h = C.c_void_p(1234)
    for dtype in (cap.I32, cap.I64, cap.F16, cap.BF16):
        assert lib.ndi_interp2d_create_bicubic(C.byref(desc_for(cap, x, y, z, dtype)), None, C.byref(h)) == cap.BAD_ARG
        assert cap.last_error().startswith("Bicubic needs") and h.value is None      # *out is cleared
    for bad in (-1, 5, 99):      # no periodic / per-lane encoding: every kind outside ndi_bc_kind
        for end in range(4):
            bc = (cap.Boundary * 4)()
            bc[end].kind = bad
            assert lib.ndi_interp2d_create_bicubic(C.byref(desc_for(cap, x, y, z)), bc, C.byref(h)) == cap.BAD_ARG
            assert "Bicubic" in cap.last_error() and "periodic and per-lane boundaries are not provided" in cap.last_error()
    x2, y2, z2 = grid(2, 5)
    assert lib.ndi_interp2d_create_bicubic(C.byref(desc_for(cap, x2, y2, z2)), None, C.byref(h)) == cap.NOT_ENOUGH_DATA
    assert lib.ndi_interp2d_create_bicubic(None, None, C.byref(h)) == cap.BAD_ARG and cap.last_error() == "null argument"
    assert lib.ndi_interp2d_tables(None, None, None, None, cap.MEM_HOST) == cap.BAD_ARG and cap.last_error() == "null handle"
    # the mirror says the same before it reaches the library
    bic = pkg.Bicubic.new
    with pytest.raises(TypeError, match="Bicubic has no periodic ends"):
        bic().boundary(pkg.BoundaryCondition.Periodic)
    rows = np.array([[pkg.RowBoundary.Natural, pkg.RowBoundary.Clamped]], dtype=object)
    with pytest.raises(TypeError, match="Bicubic takes no per-lane"):
        bic().boundary_y(pkg.BoundaryCondition.Individual(rows))
    for dt in (np.int32, np.int64, np.float16):
        with pytest.raises(TypeError, match="Bicubic covers float32/float64 only"):
            pkg.Interp2DBuilder.new(np.zeros((3, 3), dt)).strategy(bic()).build()
    b = bic().boundary(pkg.BoundaryCondition.Natural).boundary_x(
        pkg.RowBoundary.Mixed(pkg.SingleBoundary.Natural, pkg.SingleBoundary.FirstDeriv(0.5)))
    assert (b._bc_x.right.kind, b._bc_x.right.value, b._bc_y.left.kind) == (cap.BC_FIRST_DERIV, 0.5, cap.BC_NATURAL)


def test_building_without_a_gpu_is_a_loud_device_error(pkg):
    build = pkg.Interp2DBuilder.new(np.zeros((4, 4))).strategy(pkg.Bicubic.new()).build
    if pkg.device_count() > 0:      # with a device the same call builds (tests/test_gpu_bicubic.py has the rest)
        assert isinstance(build().strategy, pkg.Bicubic)
        return
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        build()


# ---- the restatement against scipy --------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_specification_names():
    g = golden()
    cases = list(g["cases"])
    assert len(cases) == 20 and sum(c.startswith("float32") for c in cases) == 10
    shapes, lanes, fams, labels = set(), set(), set(), set()
    for cid in cases:
        x, y, z, qx, qy = (g[f"{cid}/{k}"] for k in ("x", "y", "z", "qx", "qy"))
        assert x.dtype == y.dtype == z.dtype == qx.dtype == qy.dtype and z.shape[:2] == (len(x), len(y))
        assert g[cid + "/expect"].shape == (len(g[cid + "/labels"]), len(qx), z.shape[2]) and g[cid + "/expect"].dtype == np.float64
        assert np.all((qx >= x[0]) & (qx <= x[-1]) & (qy >= y[0]) & (qy <= y[-1]))
        assert np.sum(np.isin(qx, x) & np.isin(qy, y)) >= 5 and (qx[16], qy[16]) == (x[-1], y[-1])   # nodes; the last corner
        assert qx[17] == x[-1] and qy[18] == y[-1]                       # the last knot on each axis alone
        shapes.add(z.shape[:2]); lanes.add(z.shape[2]); fams |= set(cid.split("_")[-2:]); labels |= set(g[cid + "/labels"])
    assert {(3, 3), (3, 4), (4, 3), (64, 48)} <= shapes and lanes == {1, 2, 3}
    assert fams == {"even", "random", "geometric", "jittered"} and labels == set(ENDS)
    assert os.path.getsize(os.path.join(GOLDEN, "bicubic_scipy.npz")) <= 200 * 1024


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_the_restated_build_is_the_oracles_but_for_the_not_a_knot_row(dt):
    """bicubic_ref.cubic_build with the reference's last-row entry equals oracle.cubic_build bit for bit, on every knot
    family and every pair of ends: the build Bicubic uses for a not-a-knot right end differs from the reference's in that
    entry alone; where the last two intervals are equal it is the reference's build outright."""
    import itertools

    T = np.dtype(dt).type
    rng = np.random.default_rng(4131)

    def knots(fam, n):
        if fam == "even":
            return (np.arange(n) * 0.5 - 1.0).astype(dt)
        if fam == "geometric":
            return np.cumsum(1.3 ** np.arange(n) * 0.01).astype(dt)
        gaps = rng.uniform(0.05, 1.0, n) if fam == "random" else 1.0 + rng.uniform(-0.3, 0.3, n)
        return np.cumsum(gaps).astype(dt)

    ends = [NK, (oracle.BC_NATURAL, 0.0), (oracle.BC_CLAMPED, 0.0), (oracle.BC_FIRST_DERIV, 0.7), (oracle.BC_SECOND_DERIV, -0.4)]
    for fam, n in itertools.product(("even", "random", "geometric", "jittered"), (3, 4, 5, 9, 64)):
        x = knots(fam, n)
        assert np.all(np.diff(x) > T(0))
        y = rng.normal(size=(n, 3)).astype(dt)
        for left, right in itertools.product(ends, ends):
            if n == 3 and left == right == NK:
                continue                      # the parabola branch: not the general build
            st, a, b = oracle.cubic_build(x, y, left=left, right=right)
            a2, b2 = bicubic_ref.cubic_build(x, y, left, right, reference_row=True)
            assert st == oracle.OK and a2.dtype == b2.dtype == np.dtype(dt)
            assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes(), (fam, n, left, right)
            if fam == "even" and right == NK:     # equal last intervals: the true row is the reference's
                a3, b3 = bicubic_ref.cubic_build(x, y, left, right)
                assert a.tobytes() == a3.tobytes() and b.tobytes() == b3.tobytes(), (n, left)


@pytest.mark.parametrize("dt,cls", sorted(MEASURED))
def test_contract_matches_scipy(dt, cls):
    """max abs error / (max |z| + 1) per (dtype, boundary class) over every golden case of that pair, against 2 x the value
    the generator measured (MEASURED above; DESIGN.md 4.13 repeats the table)."""
    g = golden()
    bound = 2.0 * MEASURED[(dt, cls)]
    assert abs(float(g[f"measured/{dt}/{cls}"]) - MEASURED[(dt, cls)]) <= 1e-3 * MEASURED[(dt, cls)]
    worst, seen = 0.0, 0
    for cid in g["cases"]:
        if not cid.startswith(dt) or cls not in g[cid + "/labels"]:
            continue
        x, y, z, qx, qy = (g[f"{cid}/{k}"] for k in ("x", "y", "z", "qx", "qy"))
        got = bicubic_ref.interp(x, y, z, qx, qy, ENDS[cls])
        assert got.dtype == np.dtype(dt)
        expect = g[cid + "/expect"][list(g[cid + "/labels"]).index(cls)]
        err = float(np.abs(got.astype(np.float64) - expect).max() / (np.abs(z.astype(np.float64)).max() + 1))
        worst, seen = max(worst, err), seen + 1
        assert err <= bound, (cid, cls, err, bound)
    assert seen == {"nat": 10, "cl": 10, "mix": 10, "n3": 3, "nk": 7}[cls]
    print(f"{dt} {cls}: largest error against scipy {worst:.3e}, bound {bound:.3e}")


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_nodes_and_the_last_corner_are_exact(dt):
    g = golden()
    for cid in g["cases"]:
        if not cid.startswith(dt):
            continue
        x, y, z = (g[f"{cid}/{k}"] for k in ("x", "y", "z"))
        for ends in (ENDS["nk"], ENDS["mix"]):
            zx, zy, zxy = bicubic_ref.tables(x, y, z, ends)
            ii, jj = np.meshgrid(np.arange(len(x)), np.arange(len(y)), indexing="ij")
            got = bicubic_ref.evaluate(x, y, z, zx, zy, zxy, x[ii.ravel()], y[jj.ravel()])
            assert np.array_equal(got, z.reshape(-1, z.shape[2])), cid      # every node, the last row / column included
            assert np.array_equal(got[-1], z[-1, -1])


@pytest.mark.parametrize("variant", ["zxy_zero", "b_from_kl"])
def test_the_goldens_tell_a_mutant_from_the_contract(variant):
    """A restatement with zxy taken as 0, or with b = d - kl h, misses the goldens by orders of magnitude more than the
    bound: the goldens pin the cross term and the Hermite form."""
    g = golden()
    worst = 0.0
    for cid in g["cases"]:
        if not cid.startswith("float64"):
            continue
        x, y, z, qx, qy = (g[f"{cid}/{k}"] for k in ("x", "y", "z", "qx", "qy"))
        for k, cls in enumerate(g[cid + "/labels"]):
            got = bicubic_ref.interp(x, y, z, qx, qy, ENDS[cls], variant=variant)
            worst = max(worst, float(np.abs(got - g[cid + "/expect"][k]).max() / (np.abs(z).max() + 1)))
    assert worst > 1e6 * max(v for (dt, _), v in MEASURED.items() if dt == "float64"), worst
