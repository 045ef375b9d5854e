"""CPU: periodic axes of the Bicubic strategy at the boundary -- the new entry point in the header, the ctypes binding, the
built library and the Rust declarations; the refusals that need no device and the mirror's TypeErrors; the accuracy of the
contract's numpy restatement (tests/bicubic_periodic_ref.py, what the GPU tests compare the device against bit for bit)
against scipy through tests/golden/bicubic_periodic_scipy.npz (tests/golden/gen_bicubic_periodic_golden.py); and the
restatement's own properties, bit for bit: the seam, the period, and periodic_axes = 0."""
import ctypes as C
import os

import numpy as np
import pytest

import bicubic_periodic_ref as ref
import bicubic_ref
import oracle
from conftest import GOLDEN, ROOT
from test_bicubic_abi import desc_for, grid

NK = (oracle.BC_NOT_A_KNOT, 0.0)
# the generator's ENDS: the contract's four ends per class (the pair of a periodic axis is not read)
ENDS = {
    "nk": (NK,) * 4,
    "nat": ((oracle.BC_NATURAL, 0.0),) * 4,
    "mix": ((oracle.BC_FIRST_DERIV, 0.3), (oracle.BC_SECOND_DERIV, -0.2), (oracle.BC_FIRST_DERIV, 0.7),
            (oracle.BC_SECOND_DERIV, 0.4)),
}

# Largest error of the restatement against f64 scipy over the golden file, max abs error / (max |z| + 1), per (dtype,
# periodic axes, total order of the partial), as tests/golden/gen_bicubic_periodic_golden.py measured and printed it; the
# bar is 2 x each (the project's margin in test_bicubic_abi.py: it covers a numpy build that orders an operation
# differently, not algorithmic drift).  The queries lie up to 3.5 periods outside the range, so the figures include the
# rounding of the wrap itself (a few ulp of the coordinate times the slope of the part), which grows with the order.
MEASURED = {
    ("float64", "x", 0): 3.979e-15, ("float64", "x", 1): 1.744e-13, ("float64", "x", 2): 1.429e-10,
    ("float64", "y", 0): 7.702e-15, ("float64", "y", 1): 6.293e-13, ("float64", "y", 2): 4.296e-10,
    ("float64", "xy", 0): 2.546e-14, ("float64", "xy", 1): 6.517e-12, ("float64", "xy", 2): 4.290e-09,
    ("float32", "x", 0): 2.183e-05, ("float32", "x", 1): 4.800e-04, ("float32", "x", 2): 3.154e-01,
    ("float32", "y", 0): 1.154e-04, ("float32", "y", 1): 1.618e-02, ("float32", "y", 2): 6.913e+02,
    ("float32", "xy", 0): 1.099e-05, ("float32", "xy", 1): 5.055e-03, ("float32", "xy", 2): 3.723e+00,
}


def golden():
    return np.load(os.path.join(GOLDEN, "bicubic_periodic_scipy.npz"))


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_library_and_rust_carry_the_symbol(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert ("ndi_status ndi_interp2d_create_bicubic_periodic(const ndi_interp2d_desc* desc, const ndi_boundary* bc,\n"
            "                                                int32_t periodic_axes, ndi_interp2d** out);") in header
    for text in ("d = q - k0", "p = kn - k0", "r = fmod(d, p)", "if (r < 0) r = r + |p|", "qs = r + k0",
                 "periodic = 1 in the REFERENCE operation", "BIT FOR BIT", "bit 0 is x, bit 1 is y", "NDI_VALUE",
                 "Not provided: periodic local rules"):
        assert text in header, text
    name = "ndi_interp2d_create_bicubic_periodic"
    assert name in cap.SYMBOLS and hasattr(C.CDLL(cap.LIB_PATH), name)
    assert cap.SYMBOLS[name][1][2] is C.c_int32 and len(cap.SYMBOLS[name][1]) == 4
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp2d_create_bicubic_periodic(" in rust and "periodic_axes: i32," in rust
    assert cap.lib().ndi_version() == (0 << 16) | 5     # a new symbol, no new enumerator: no version change
    for m in ("periodic_x", "periodic_y", "periodic"):
        assert callable(getattr(pkg.Bicubic, m)), m


def test_refusals_come_back_without_a_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    create = lib.ndi_interp2d_create_bicubic_periodic
    x, y, z = grid()
    h = C.c_void_p(1234)
    for bits in (-1, 4, 7, 1 << 20):
        h = C.c_void_p(1234)
        assert create(C.byref(desc_for(cap, x, y, z)), None, bits, C.byref(h)) == cap.BAD_ARG
        assert "periodic_axes" in cap.last_error() and "Bicubic" in cap.last_error() and h.value is None   # *out is cleared
    for bits, ends, axis in ((1, (0, 1), "x"), (2, (2, 3), "y"), (3, (0, 1, 2, 3), None)):
        for end in ends:
            for kind, value in ((cap.BC_NATURAL, 0.0), (cap.BC_FIRST_DERIV, 0.5), (cap.BC_NOT_A_KNOT, 0.25), (5, 0.0)):
                bc = (cap.Boundary * 4)()
                bc[end].kind, bc[end].value = kind, value
                h = C.c_void_p(1234)
                assert create(C.byref(desc_for(cap, x, y, z)), bc, bits, C.byref(h)) == cap.BAD_ARG
                msg = cap.last_error()
                assert "Bicubic" in msg and f"the {axis or 'xy'[end // 2]} axis is periodic" in msg and h.value is None
                assert "a periodic end has no kind" in msg
    # the other axis keeps ndi_bc_kind, and its refusal
    bc = (cap.Boundary * 4)()
    bc[2].kind = 5
    assert create(C.byref(desc_for(cap, x, y, z)), bc, 1, C.byref(h)) == cap.BAD_ARG
    assert "periodic and per-lane boundaries are not provided" in cap.last_error()
    for dtype in (cap.I32, cap.I64, cap.F16, cap.BF16):
        h = C.c_void_p(1234)
        assert create(C.byref(desc_for(cap, x, y, z, dtype)), None, 3, C.byref(h)) == cap.BAD_ARG
        assert cap.last_error().startswith("Bicubic needs") and h.value is None
    for shape in ((2, 5), (5, 2)):
        x2, y2, z2 = grid(*shape)
        assert create(C.byref(desc_for(cap, x2, y2, z2)), None, 3, C.byref(h)) == cap.NOT_ENOUGH_DATA
        assert "at least 3 data points on each axis" in cap.last_error()
    assert create(None, None, 1, C.byref(h)) == cap.BAD_ARG and cap.last_error() == "null argument"
    assert create(C.byref(desc_for(cap, x, y, z)), None, 1, None) == cap.BAD_ARG and cap.last_error() == "null argument"


def test_the_mirror_refuses_before_it_reaches_the_library(pkg):
    bic, BC, RB, SB = pkg.Bicubic.new, pkg.BoundaryCondition, pkg.RowBoundary, pkg.SingleBoundary
    z = np.zeros((4, 5))
    with pytest.raises(TypeError, match=r"Bicubic has no periodic ends.*periodic_x\(\) / \.periodic_y\(\)"):
        bic().boundary(BC.Periodic)
    with pytest.raises(TypeError, match="Bicubic has no periodic ends"):
        bic().periodic_x().boundary_y(BC.Periodic)
    mixed = RB.Mixed(SB.Natural, SB.FirstDeriv(0.5))
    for strat, axis in ((bic().periodic_x().boundary_x(BC.Natural), "x"), (bic().boundary_y(mixed).periodic_y(), "y"),
                        (bic().periodic_x().boundary(BC.Clamped), "x"), (bic().boundary(BC.Natural).periodic(), "x"),
                        (bic().periodic_y().boundary(mixed), "y")):
        with pytest.raises(TypeError, match=f"the {axis} axis is periodic and takes no boundary condition"):
            pkg.Interp2DBuilder.new(z).strategy(strat).build()
    for local in (pkg.Bicubic.pchip, pkg.Bicubic.akima, lambda: pkg.Bicubic.hermite(z, z, z)):
        for m in ("periodic_x", "periodic_y", "periodic"):
            with pytest.raises(TypeError, match="takes no boundary conditions: ends are a spline notion"):
                getattr(local(), m)()
    # the chain: the other axis keeps its ends, extrapolate decides the wrap
    s = bic().periodic_x().boundary_y(mixed).extrapolate(True)
    assert (s._periodic, s.wraps, s._bc_y.right.value) == (1, 1, 0.5)
    assert (bic().periodic().wraps, bic().periodic().extrapolate(True).wraps, bic().extrapolate(True).wraps) == (0, 3, 0)
    assert bic().periodic_y().boundary(BC.NotAKnot)._periodic == 2          # the default kind is no boundary condition
    with pytest.raises(TypeError, match="wraps queries on x and y.*antiderivative of a wrapping strategy is not provided"):
        bic().periodic().extrapolate(True).antiderivative()
    with pytest.raises(TypeError, match="wraps queries on y"):
        bic().periodic_y().extrapolate(True).antiderivative()


def test_building_without_a_gpu_is_a_loud_device_error(pkg):
    z = ref.make_periodic(np.random.default_rng(0).normal(size=(4, 5, 2)), 3)
    build = pkg.Interp2DBuilder.new(z).strategy(pkg.Bicubic.new().periodic()).build
    if pkg.device_count() > 0:      # with a device the same call builds (tests/test_gpu_bicubic_periodic.py has the rest)
        assert build().strategy._periodic == 3
        return
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        build()


# ---- the restatement against scipy --------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_specification_names():
    g = golden()
    cases = list(g["cases"])
    assert len(cases) == 24 and sum(c.startswith("float32") for c in cases) == 12
    assert [tuple(p) for p in g["parts"]] == [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)]
    shapes, lanes, fams, combos = set(), set(), set(), set()
    for cid in cases:
        x, y, z, qx, qy = (g[f"{cid}/{k}"] for k in ("x", "y", "z", "qx", "qy"))
        axes, ends = int(g[cid + "/axes"]), str(g[cid + "/ends"])
        assert x.dtype == y.dtype == z.dtype == qx.dtype == qy.dtype and z.shape[:2] == (len(x), len(y))
        assert g[cid + "/expect"].shape == (6, len(qx), z.shape[2]) and g[cid + "/expect"].dtype == np.float64
        assert np.array_equal(z, ref.make_periodic(z, axes))                 # the data is periodic, corners included
        for bit, k, q in ((1, x, qx), (2, y, qy)):
            p = k[-1] - k[0]
            if axes & bit:      # up to 3.5 periods outside, and exactly k0 - p, kn + p, kn, k0
                assert q.min() < k[0] - p and q.max() > k[-1] + p and np.all((q >= k[0] - 3.5 * p) & (q <= k[-1] + 3.5 * p))
                assert all(v in q for v in (k[0] - p, k[-1] + p, k[-1], k[0]))
            else:
                assert np.all((q >= k[0]) & (q <= k[-1])) and k[-1] in q
        shapes.add(z.shape[:2]); lanes.add(z.shape[2]); fams |= set(cid.split("_")[2:4]); combos.add((axes, ends))
    assert {(3, 4), (4, 3), (3, 3), (4, 4), (33, 24)} <= shapes and lanes == {1, 2, 3}
    assert fams == {"even", "random", "geometric", "jittered"}
    assert combos == {(1, "nk"), (2, "nk"), (3, "nk"), (1, "nat"), (2, "nat"), (1, "mix"), (2, "mix")}
    assert os.path.getsize(os.path.join(GOLDEN, "bicubic_periodic_scipy.npz")) <= 200 * 1024


@pytest.mark.parametrize("dt,axes,order", sorted(MEASURED))
def test_contract_matches_scipy(dt, axes, order):
    """max abs error / (max |z| + 1) per (dtype, periodic axes, total order) over every golden case and part of that class,
    against 2 x the value the generator measured (MEASURED above; DESIGN.md 4.20 repeats the table)."""
    g = golden()
    m = MEASURED[(dt, axes, order)]
    bound = 2.0 * m
    assert abs(float(g[f"measured/{dt}/{axes}/{order}"]) - m) <= 1e-3 * m
    bits = {"x": 1, "y": 2, "xy": 3}[axes]
    worst, seen = 0.0, 0
    for cid in g["cases"]:
        if not cid.startswith(dt) or int(g[cid + "/axes"]) != bits:
            continue
        x, y, z, qx, qy = (g[f"{cid}/{k}"] for k in ("x", "y", "z", "qx", "qy"))
        zx, zy, zxy = ref.tables(x, y, z, ENDS[str(g[cid + "/ends"])], bits)
        for k, (nu_x, nu_y) in enumerate(g["parts"]):
            if nu_x + nu_y != order:
                continue
            got = ref.evaluate_partial(x, y, z, zx, zy, zxy, qx, qy, int(nu_x), int(nu_y), bits)
            assert got.dtype == np.dtype(dt)
            err = float(np.abs(got.astype(np.float64) - g[cid + "/expect"][k]).max() / (np.abs(z.astype(np.float64)).max() + 1))
            worst, seen = max(worst, err), seen + 1
            assert err <= bound, (cid, (nu_x, nu_y), err, bound)
    assert seen == {"x": 4, "y": 4, "xy": 4}[axes] * {0: 1, 1: 2, 2: 3}[order]
    print(f"{dt} periodic {axes}, order {order}: largest error against scipy {worst:.3e}, bound {bound:.3e}")


def test_measured_covers_every_class():
    assert sorted(MEASURED) == sorted((dt, ax, o) for dt in ("float32", "float64") for ax in ("x", "y", "xy") for o in range(3))


# ---- properties of the restatement, bit for bit -------------------------------------------------------------------
def cases(dt):
    g = golden()
    for cid in g["cases"]:
        if cid.startswith(dt):
            yield (cid, int(g[cid + "/axes"]), ENDS[str(g[cid + "/ends"])]) + tuple(g[f"{cid}/{k}"] for k in ("x", "y", "z"))


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_the_seam_is_the_same_bits(dt):
    """index 0 equals index n-1 of each table along each periodic axis"""
    for cid, axes, ends, x, y, z in cases(dt):
        for name, t in zip(("zx", "zy", "zxy"), ref.tables(x, y, z, ends, axes)):
            assert t.dtype == np.dtype(dt)
            if axes & 1:
                assert t[0].tobytes() == t[-1].tobytes(), (cid, name, "x")
            if axes & 2:
                assert np.ascontiguousarray(t[:, 0]).tobytes() == np.ascontiguousarray(t[:, -1]).tobytes(), (cid, name, "y")


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_a_query_whole_periods_away_is_its_wrapped_query(dt):
    """evaluate(q + m period) is evaluate(wrap(q + m period)): the wrap happens once, before the search, and nothing else
    knows about it; in range the wrap is the identity, and +-inf and NaN come out NaN."""
    rng = np.random.default_rng(77)
    for cid, axes, ends, x, y, z in cases(dt):
        tabs = ref.tables(x, y, z, ends, axes)
        qx, qy = rng.uniform(x[0], x[-1], 40).astype(dt), rng.uniform(y[0], y[-1], 40).astype(dt)
        assert ref.wrap(x, qx).tobytes() == qx.tobytes() and ref.wrap(y, qy).tobytes() == qy.tobytes()
        base = ref.evaluate(x, y, z, *tabs, qx, qy, axes)
        assert base.tobytes() == bicubic_ref.evaluate(x, y, z, *tabs, qx, qy).tobytes()
        for m in (1, -1, 3, -3):
            sx = (qx + x.dtype.type(m) * (x[-1] - x[0])) if axes & 1 else qx
            sy = (qy + y.dtype.type(m) * (y[-1] - y[0])) if axes & 2 else qy
            got = ref.evaluate(x, y, z, *tabs, sx, sy, axes)
            wx, wy = ref.wrapped(x, y, sx, sy, axes)
            assert np.all((wx >= x[0]) & (wy >= y[0]))
            assert got.tobytes() == bicubic_ref.evaluate(x, y, z, *tabs, wx, wy).tobytes(), (cid, m)
    k =np.array([1.0, 2.0, 4.0], dt)
    w = ref.wrap(k, np.array([np.inf, -np.inf, np.nan, 4.0, 1.0, 7.5, -2.5, 0.0], dt))
    assert np.isnan(w[:3]).all() and w[3:].tolist() == [4.0, 1.0, 1.5, 3.5, 3.0]


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_no_periodic_axis_is_the_plain_restatement(dt):
    for cid, axes, ends, x, y, z in cases(dt):
        for a, b in zip(ref.tables(x, y, z, ends, 0), bicubic_ref.tables(x, y, z, ends)):
            assert a.tobytes() == b.tobytes(), cid


def test_a_mismatch_is_a_value_error_of_the_restatement_too():
    for cid, axes, ends, x, y, z in cases("float64"):
        bad = z.copy()
        bad[-1 if axes & 1 else 0, -1 if axes & 2 else 0, 0] += 1.0
        with pytest.raises(ValueError, match="VALUE"):
            ref.tables(x, y, bad, ends, axes)
