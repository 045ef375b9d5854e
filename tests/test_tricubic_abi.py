"""CPU: the Tricubic restatement (tests/tricubic_ref.py) against scipy through tests/golden/tricubic_scipy.npz
(tests/golden/gen_tricubic_golden.py), polynomial exactness, the mutants, the ABI of include/ndinterp3d_cubic.h (symbols,
strict C99) and the refusals and builder errors that are decided before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import tricubic_ref as tc
from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "ndinterp3d_cubic.h")
NEW = ["ndi_interp3d_create_tricubic", "ndi_interp3d_tables"]

# Largest error of the restatement against f64 scipy over the golden file, max abs error / (max |f| + 1), per (dtype, class
# of ends) as tests/golden/gen_tricubic_golden.py measured and printed it; the bar is 2 x each (DESIGN.md 4.13's rule: the
# restatement's rounding differs from scipy's by operation order only).  DESIGN.md 4.27 repeats the table.
MEASURED = {
    ("float64", "nk"): 3.488e-13, ("float64", "mix"): 5.349e-16, ("float64", "n3"): 1.261e-15,
    ("float32", "nk"): 2.486e-06, ("float32", "mix"): 2.255e-07, ("float32", "n3"): 9.045e-07,
}


def golden():
    return np.load(os.path.join(GOLDEN, "tricubic_scipy.npz"))


def case(g, cid):
    return [g[f"{cid}/{k}"] for k in ("x", "y", "z", "f", "qx", "qy", "qz", "expect")] + [str(g[cid + "/class"])]


def bc_of(cls):
    return tc.MIXED_BC if cls == "mix" else tc.DEFAULT_BC


# ---- the restatement against scipy -----------------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_specification_names():
    g = golden()
    cases = [str(c) for c in g["cases"]]
    assert 10 <= len(cases) <= 16
    shapes = {tuple(g[c + "/f"].shape) for c in cases}
    assert (4, 4, 4, 1) in shapes and (17, 9, 12, 1) in shapes
    assert {s[3] for s in shapes} == {1, 2, 3}
    assert {str(g[c + "/class"]) for c in cases} == {"nk", "mix", "n3"}
    for fam in ("even", "random", "geometric", "clustered"):
        assert any(fam in c for c in cases), fam
    assert any(min(g[c + "/f"].shape[:3]) == 3 for c in cases if str(g[c + "/class"]) == "n3")
    assert all(v != 0.0 for _, v in (tc.MIXED_BC[1], tc.MIXED_BC[2], tc.MIXED_BC[4]))    # a non-zero end value on each axis
    assert os.path.getsize(os.path.join(GOLDEN, "tricubic_scipy.npz")) <= 300 * 1024


@pytest.mark.parametrize("dt,cls", sorted(MEASURED))
def test_restatement_against_scipy(dt, cls):
    """max abs error / (max |f| + 1) per (dtype, class of ends) over every golden case of that pair, against 2 x the value
    the generator measured (MEASURED above)."""
    g = golden()
    bound = 2.0 * MEASURED[(dt, cls)]
    assert abs(float(g[f"measured/{dt}/{cls}"]) - MEASURED[(dt, cls)]) <= 1e-3 * MEASURED[(dt, cls)]
    seen = 0
    for cid in (str(c) for c in g["cases"]):
        x, y, z, f, qx, qy, qz, expect, c = case(g, cid)
        if f.dtype.name != dt or c != cls:
            continue
        seen += 1
        got = tc.interp(x, y, z, f, qx, qy, qz, bc_of(cls)).astype(np.float64)
        err = float(np.abs(got - expect).max() / (np.abs(f.astype(np.float64)).max() + 1))
        print(f"{cid}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (cid, err, bound)
    assert seen >= 1


# ---- polynomial exactness ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_a_cubic_polynomial_with_exact_first_derivative_ends_is_reproduced(dt):
    """f = p(x) q(y) r(z) + a(x) + b(y) + c(z), p, q, r cubics with zero slope at both ends of their axis and a, b, c any
    cubics: the normal derivative on each end face is one number, so first-derivative ends state it exactly, and the spline
    with those ends IS the polynomial.  Bound: 64 ulp of max |f| + 1 -- an evaluation is three nested Hermite forms of about
    ten roundings each on top of three nested solves on at most 7 knots of spacing ratio below 2, whose tridiagonal systems
    are diagonally dominant (factor 2), so a few tens of roundings of values of the size of f in all."""
    rng = np.random.default_rng(5)
    ax = [np.array(k, dtype=dt) for k in ([0.0, 0.25, 0.5, 0.625, 0.875, 1.0], [0.0, 0.5, 0.75, 1.0],
                                          [0.0, 0.125, 0.375, 0.5, 0.625, 0.875, 1.0])]
    flat = lambda s: 3.0 * s * s - 2.0 * s ** 3                                     # noqa: E731  zero slope at 0 and at 1
    co = [(0.5, -1.0, 2.0, 1.5), (1.0, 0.75, -0.5, 0.25), (-0.25, 2.0, 1.0, -1.0)]    # a, b, c: c0 + c1 s + c2 s^2 + c3 s^3
    cubic = lambda c, s: c[0] + c[1] * s + c[2] * s * s + c[3] * s ** 3             # noqa: E731
    slope = lambda c, s: c[1] + 2.0 * c[2] * s + 3.0 * c[3] * s * s                 # noqa: E731

    def poly(x, y, z):
        return flat(x) * flat(y) * flat(z) + cubic(co[0], x) + cubic(co[1], y) + cubic(co[2], z)
    a64 = [k.astype(np.float64) for k in ax]
    f = poly(a64[0][:, None, None], a64[1][None, :, None], a64[2][None, None, :]).astype(dt)[..., None]
    bc = tuple((oracle.BC_FIRST_DERIV, slope(co[a], end)) for a in range(3) for end in (0.0, 1.0))
    q = [rng.uniform(0.0, 1.0, 400).astype(dt) for _ in range(3)]
    got = tc.interp(*ax, f, *q, bc)[:, 0].astype(np.float64)
    want = poly(*[v.astype(np.float64) for v in q])
    # the data were rounded to dt once: half an ulp of f, carried through an interpolant whose weights sum to 1 in size
    err = float(np.abs(got - want).max() / (np.abs(want).max() + 1))
    print(f"{np.dtype(dt).name}: polynomial reproduced to {err / np.finfo(dt).eps:.2f} ulp of max |f| + 1")
    assert err <= 64 * np.finfo(dt).eps


# ---- mutants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fxyz_zero", "fxyz_from_x", "x_first", "left"])
def test_every_mutant_differs_from_the_rule_on_the_tests_own_queries(variant):
    """The wrong variants of tests/tricubic_ref.py on the golden queries of the mixed-ends case (plus queries ON knots for the
    wrong search): the value mutants miss scipy by far more than the bound, the order and search mutants give other bits."""
    g = golden()
    cid = next(str(c) for c in g["cases"] if str(g[str(c) + "/class"]) == "mix" and "float64" in str(c))
    x, y, z, f, qx, qy, qz, expect, _ = case(g, cid)
    bound = 2.0 * MEASURED[("float64", "mix")]
    scale = np.abs(f).max() + 1
    right = tc.interp(x, y, z, f, qx, qy, qz, tc.MIXED_BC)
    assert float(np.abs(right - expect).max() / scale) <= bound
    if variant == "fxyz_zero":
        wrong = tc.interp(x, y, z, f, qx, qy, qz, tc.MIXED_BC, variant=variant)
        assert float(np.abs(wrong - expect).max() / scale) > 1e6 * bound
    elif variant == "fxyz_from_x":
        # The passes are linear maps along different axes and the end values of a pass on a derivative table are 0, so
        # D_x D_z D_y f and D_z D_y D_x f are ONE table mathematically, for every set of ends: this mutant can differ in
        # rounding only.  It does, in most entries -- which is what the bit-for-bit table tests on the device hold.
        a, b = tc.tables(x, y, z, f, tc.MIXED_BC)[6], tc.tables(x, y, z, f, tc.MIXED_BC, variant=variant)[6]
        assert np.allclose(a, b, rtol=0, atol=1e-9 * np.abs(a).max())
        assert (tc.bits(a) != tc.bits(b)).mean() > 0.25
    elif variant == "x_first":
        wrong = tc.interp(x, y, z, f, qx, qy, qz, tc.MIXED_BC, variant=variant)
        assert float(np.abs(wrong - expect).max() / scale) <= 4 * bound            # the same polynomial ...
        assert (tc.bits(wrong) != tc.bits(right)).mean() > 0.25                      # ... in other bits
    else:
        kx, ky, kz = (np.ascontiguousarray(a.ravel()) for a in np.meshgrid(x[1:-1], y[1:-1], z[1:-1], indexing="ij"))
        tabs = tc.tables(x, y, z, f, tc.MIXED_BC)
        # A Hermite patch gives the node value from either side (s == 0 and s == 1 are both exact), so on finite tables the
        # wrong search is the same VALUE on every knot; what it changes is the cell, and with it which nodes reach the row.
        right_cells, left_cells = tc.cells(x, y, z, kx, ky, kz), tc.cells(x, y, z, kx, ky, kz, side="left")
        assert all(np.all(r == l + 1) for r, l in zip(right_cells, left_cells))
        a = tc.evaluate(x, y, z, f, tabs, kx, ky, kz)
        assert np.array_equal(a, f[1:-1, 1:-1, 1:-1].reshape(a.shape))           # on a knot, s == 0: the data exactly
        assert np.array_equal(a, tc.evaluate(x, y, z, f, tabs, kx, ky, kz, side="left"))
        # a NaN planted in one node derivative reaches exactly the rows whose cell holds the node: node (3, 2, 2) is a corner
        # of the cell of the knot query (2, 1, 1) by the rule, and of no cell the wrong search picks for a knot below it
        poisoned = [t.copy() for t in tabs]
        poisoned[6][3, 2, 2] = np.nan
        row = np.ravel_multi_index((1, 0, 0), (len(x) - 2, len(y) - 2, len(z) - 2))        # the query on knot (2, 1, 1)
        a = tc.evaluate(x, y, z, f, poisoned, kx, ky, kz)
        b = tc.evaluate(x, y, z, f, poisoned, kx, ky, kz, side="left")
        assert np.isnan(a[row]).all() and np.isfinite(b[row]).all()


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ndi_[a-z0-9_]+)\s*\(", text)))


def test_new_header_declares_exactly_the_two_functions_and_they_are_bound(pkg):
    assert _declared(HEADER) == NEW
    lib = C.CDLL(pkg._capi.LIB_PATH)
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert sorted(pkg._capi.SYMBOLS3D_CUBIC) == NEW
    bound = pkg._capi.lib()
    for n in NEW:
        assert getattr(bound, n).argtypes == pkg._capi.SYMBOLS3D_CUBIC[n][1]
    assert '#include "ndinterp3d.h"' in open(HEADER).read()
    assert pkg._capi.lib().ndi_version() == (0 << 16) | 5


def test_the_frozen_headers_still_declare_exactly_their_tables(pkg):
    assert _declared(os.path.join(ROOT, "include", "ndinterp3d.h")) == sorted(pkg._capi.SYMBOLS3D) == \
        ["ndi_interp3d_clone", "ndi_interp3d_create", "ndi_interp3d_destroy", "ndi_interp3d_eval"]
    assert _declared(os.path.join(ROOT, "include", "ndinterp.h")) == sorted(pkg._capi.SYMBOLS)
    assert not (set(pkg._capi.SYMBOLS) | set(pkg._capi.SYMBOLS3D)) & set(NEW)
    assert "Tricubic" in pkg.__all__ and pkg.Tricubic.MINIMUM_DATA_LENGHT == 3


def test_header_and_example_are_plain_c99(pkg, tmp_path):
    src = tmp_path / "only_header.c"
    src.write_text('#include "ndinterp3d_cubic.h"\nint main(void) { ndi_boundary b[6]; (void)b; '
                   'return (int)sizeof(ndi_interp3d_desc) - 112; }\n')
    flags = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include")]
    r = subprocess.run(flags + [str(src), "-o", str(tmp_path / "only_header")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "only_header")]).returncode == 0
    exe = tmp_path / "c_abi_tricubic"
    r = subprocess.run(flags + [os.path.join(ROOT, "examples", "c_abi_tricubic.c"), "-L", os.path.join(ROOT, "ndarray-interp_amd"),
                                "-lndinterp_hip", "-Wl,-rpath," + os.path.join(ROOT, "ndarray-interp_amd"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if pkg._capi.lib().ndi_device_count() == 0:      # (with a GPU the example runs in tests/test_gpu_tricubic.py)
        run = subprocess.run([str(exe)], capture_output=True, text=True)
        assert run.returncode == 1 and "no CPU fallback" in run.stderr      # loud failure without a GPU


# ---- refusals and builder errors: no device needed -------------------------------------------------------------------------------
def host_desc(pkg, x, y, z, data, validate=1):
    cap = pkg._capi
    d = cap.Interp3DDesc()
    d.dtype = cap.F64 if data.dtype == np.float64 else cap.F32
    d.memspace, d.validate = cap.MEM_HOST, validate
    d.nx, d.ny, d.nz = data.shape[:3]
    d.lanes = int(np.prod(data.shape[3:], dtype=np.int64))
    for name, k in (("x", x), ("y", y), ("z", z)):
        if k is not None:
            setattr(d, name, k.ctypes.data)
            setattr(d, name + "_len", k.size)
    d.data = data.ctypes.data
    return d


def test_create_and_tables_refusals_need_no_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    data = np.zeros((3, 3, 3))
    k = np.array([0.0, 1.0, 2.0])
    h = C.c_void_p(0xdead)
    assert lib.ndi_interp3d_create_tricubic(None, None, C.byref(h)) == cap.BAD_ARG and h.value is None      # *out cleared
    d = host_desc(pkg, k, k, k, data)
    assert lib.ndi_interp3d_create_tricubic(C.byref(d), None, None) == cap.BAD_ARG
    for dtype in (cap.I32, cap.I64, cap.F16, cap.BF16, 7, -1):
        d = host_desc(pkg, k, k, k, data)
        d.dtype = dtype
        h = C.c_void_p(0xdead)
        assert lib.ndi_interp3d_create_tricubic(C.byref(d), None, C.byref(h)) == cap.BAD_ARG and h.value is None
        assert "Tricubic takes f32 / f64" in cap.last_error()
    d = host_desc(pkg, k, k, k, data)
    d.reserved = 1
    h = C.c_void_p(0xdead)
    assert lib.ndi_interp3d_create_tricubic(C.byref(d), None, C.byref(h)) == cap.BAD_ARG and h.value is None
    assert "reserved" in cap.last_error()
    for end in range(6):                     # an unknown boundary kind, at each end
        for kind in (5, -1):
            bc = (cap.Boundary * 6)(*[cap.Boundary(cap.BC_NOT_A_KNOT, 0.0) for _ in range(6)])
            bc[end].kind = kind
            d = host_desc(pkg, k, k, k, data)
            h = C.c_void_p(0xdead)
            assert lib.ndi_interp3d_create_tricubic(C.byref(d), bc, C.byref(h)) == cap.BAD_ARG and h.value is None
            assert "Tricubic takes one non-periodic boundary kind" in cap.last_error()
            assert ("x-left", "x-right", "y-left", "y-right", "z-left", "z-right")[end] in cap.last_error()
    none = (C.c_void_p * 7)()
    assert lib.ndi_interp3d_tables(None, none, cap.MEM_HOST) == cap.BAD_ARG and "null handle" in cap.last_error()


def test_validation_on_host_axes_in_the_builders_order_with_three_knots(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    h = C.c_void_p()
    up = lambda n: np.arange(float(n))   # noqa: E731

    def create(x, y, z, shape):
        d = host_desc(pkg, x, y, z, np.zeros(shape))
        return lib.ndi_interp3d_create_tricubic(C.byref(d), None, C.byref(h)), cap.last_error()
    bad = np.array([0.0, 2.0, 1.0, 3.0])
    for a, shape in enumerate([(2, 2, 2), (3, 2, 2), (3, 3, 2)]):     # n = 2 on each axis in turn, every other defect present
        assert create(up(5), up(5), bad, shape) == (cap.NOT_ENOUGH_DATA, f"The {a}-dimension has not enough data for the chosen "
                                                    "interpolation strategy. Provided: 2, Reqired: 3")
    assert create(up(5), up(5), bad, (3, 3, 3)) == (cap.SHAPE, "Lenghts of x-axis and data-0-axis need to match. Got x: 5, data-0: 3")
    assert create(up(3), up(5), bad, (3, 3, 3)) == (cap.SHAPE, "Lenghts of y-axis and data-1-axis need to match. Got y: 5, data-1: 3")
    assert create(up(3), up(3), bad, (3, 3, 3)) == (cap.SHAPE, "Lenghts of z-axis and data-2-axis need to match. Got z: 4, data-2: 3")
    assert create(up(3), up(3), bad, (3, 3, 4)) == (cap.MONOTONIC, "The z-axis needs to be strictly monotonic rising")
    assert create(bad, up(3), bad, (4, 3, 4)) == (cap.MONOTONIC, "The x-axis needs to be strictly monotonic rising")
    assert create(up(3), bad, bad, (3, 4, 4)) == (cap.MONOTONIC, "The y-axis needs to be strictly monotonic rising")
    assert create(None, None, np.array([0.0, 1.0, 1.0]), (3, 3, 3))[0] == cap.MONOTONIC      # a NULL axis is 0..n and passes
    # Trilinear keeps 2
    d = host_desc(pkg, up(5), up(5), bad, np.zeros((1, 2, 2)))
    assert lib.ndi_interp3d_create(C.byref(d), C.byref(h)) == cap.NOT_ENOUGH_DATA and cap.last_error().endswith("Provided: 1, Reqired: 2")


def test_mirror_errors(pkg):
    E, BC = pkg.BuilderError, pkg.BoundaryCondition
    up = lambda n: np.arange(float(n))   # noqa: E731

    def build(x, y, z, shape, dt=np.float64):
        return pkg.Interp3D.builder(np.zeros(shape, dtype=dt)).x(x).y(y).z(z).strategy(pkg.Tricubic.new()).build()
    for a, shape in enumerate([(2, 3, 3), (3, 2, 3), (3, 3, 2)]):
        with pytest.raises(E.NotEnoughData, match=f"The {a}-dimension has not enough data .* Provided: 2, Reqired: 3"):
            build(up(3), up(3), up(3), shape)
    with pytest.raises(E.ShapeError, match="Lenghts of y-axis and data-1-axis need to match"):
        build(up(3), up(4), up(3), (3, 3, 3))
    with pytest.raises(E.Monotonic, match="The z-axis needs"):
        build(up(3), up(3), np.array([0.0, 2.0, 1.0]), (3, 3, 3))
    for dt in (np.int32, np.int64, np.float16):
        with pytest.raises(TypeError, match="Tricubic takes float32 / float64"):
            build(up(3), up(3), up(3), (3, 3, 3), dt)
    with pytest.raises(TypeError, match="Tricubic has no periodic ends"):
        pkg.Tricubic.new().boundary(BC.Periodic)
    with pytest.raises(TypeError, match="Tricubic takes no per-lane"):
        pkg.Tricubic.new().boundary_z(BC.Individual([[pkg.RowBoundary.Natural]]))
    with pytest.raises(TypeError, match="Tricubic boundaries are"):
        pkg.Tricubic.new().boundary_x("natural")
    s = pkg.Tricubic.new().boundary(BC.Natural).boundary_y(pkg.RowBoundary.Mixed(pkg.SingleBoundary.Clamped, pkg.SingleBoundary.NotAKnot))
    assert [int(e.kind) for a in s._bc for e in (a.left, a.right)] == [1, 1, 2, 0, 1, 1]


def test_no_device_means_loud_failure(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        pkg.Interp3D.builder(np.zeros((3, 3, 3))).strategy(pkg.Tricubic.new()).build()
