"""CPU: partial-derivative handles of Bicubic at the boundary -- the new entry point in the header, the ctypes binding, the
built library and the Rust declarations; the refusals that need no device, the library's and the mirror's; and the accuracy
of the contract's numpy restatement (tests/bicubic_partial_ref.py, what the GPU tests compare the device against bit for bit)
against scipy through tests/golden/bicubic_partial_scipy.npz (tests/golden/gen_bicubic_partial_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import bicubic_partial_ref
import bicubic_ref
from conftest import GOLDEN, ROOT
from test_bicubic_abi import ENDS

ORDERS = bicubic_partial_ref.ORDERS

# Largest error of the restatement against f64 scipy over the golden file, max abs error / (max |expected| + 1) per (dtype,
# class, nu_x, nu_y), as tests/golden/gen_bicubic_partial_golden.py measured and printed it; the bar is 2 x each (the
# project's margin in test_bicubic_abi.py / test_derivative_abi.py: it covers a numpy build that orders an operation
# differently, not algorithmic drift).
MEASURED = {
    ("float32", "mix", 0, 1): 1.394e-07, ("float32", "mix", 0, 2): 4.014e-07, ("float32", "mix", 1, 0): 3.345e-07,
    ("float32", "mix", 1, 1): 3.051e-07, ("float32", "mix", 1, 2): 6.530e-07, ("float32", "mix", 2, 0): 3.312e-07,
    ("float32", "mix", 2, 1): 8.971e-07, ("float32", "mix", 2, 2): 1.946e-06,
    ("float32", "n3", 0, 1): 1.969e-07, ("float32", "n3", 0, 2): 6.088e-07, ("float32", "n3", 1, 0): 4.452e-07,
    ("float32", "n3", 1, 1): 4.000e-07, ("float32", "n3", 1, 2): 6.769e-07, ("float32", "n3", 2, 0): 5.719e-07,
    ("float32", "n3", 2, 1): 7.684e-07, ("float32", "n3", 2, 2): 2.590e-06,
    ("float32", "nk", 0, 1): 4.025e-07, ("float32", "nk", 0, 2): 7.074e-07, ("float32", "nk", 1, 0): 8.093e-07,
    ("float32", "nk", 1, 1): 1.084e-06, ("float32", "nk", 1, 2): 1.692e-06, ("float32", "nk", 2, 0): 1.073e-06,
    ("float32", "nk", 2, 1): 1.585e-06, ("float32", "nk", 2, 2): 2.563e-06,
    ("float64", "mix", 0, 1): 3.264e-15, ("float64", "mix", 0, 2): 4.302e-15, ("float64", "mix", 1, 0): 3.871e-15,
    ("float64", "mix", 1, 1): 3.185e-15, ("float64", "mix", 1, 2): 4.318e-15, ("float64", "mix", 2, 0): 5.604e-16,
    ("float64", "mix", 2, 1): 3.976e-14, ("float64", "mix", 2, 2): 1.146e-13,
    ("float64", "n3", 0, 1): 7.600e-16, ("float64", "n3", 0, 2): 5.276e-15, ("float64", "n3", 1, 0): 8.190e-16,
    ("float64", "n3", 1, 1): 5.551e-16, ("float64", "n3", 1, 2): 5.296e-15, ("float64", "n3", 2, 0): 2.148e-15,
    ("float64", "n3", 2, 1): 2.783e-15, ("float64", "n3", 2, 2): 2.348e-14,
    ("float64", "nk", 0, 1): 4.623e-15, ("float64", "nk", 0, 2): 6.863e-15, ("float64", "nk", 1, 0): 3.188e-15,
    ("float64", "nk", 1, 1): 5.146e-15, ("float64", "nk", 1, 2): 7.122e-15, ("float64", "nk", 2, 0): 3.478e-15,
    ("float64", "nk", 2, 1): 1.337e-14, ("float64", "nk", 2, 2): 2.485e-14,
}
# cases per (dtype, class): the ten shapes, less the f32 copies of the two 64 x 48 cases (the file's size limit)
SEEN = {("float64", "mix"): 10, ("float64", "n3"): 3, ("float64", "nk"): 7,
        ("float32", "mix"): 8, ("float32", "n3"): 3, ("float32", "nk"): 5}


def golden():
    return np.load(os.path.join(GOLDEN, "bicubic_partial_scipy.npz"))


def case(g, cid):
    x, y, z, q = (g[f"{cid}/{k}"] for k in ("x", "y", "z", "q"))
    return x, y, z, q[0], q[1]


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_library_and_rust_carry_the_symbol(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert "ndi_status ndi_interp2d_partial(const ndi_interp2d* h, int32_t nu_x, int32_t nu_y, ndi_interp2d** out);" in header
    for text in ("c1 = d + a          c2 = b - (a + a)          c3 = b - a",
                 "H1(pl, pr, kl, kr, h, s) = (c1 + s * ((c2 + c2) - (3 * c3) * s)) / h",
                 "H2(pl, pr, kl, kr, h, s) = ((c2 + c2) - (6 * c3) * s) / (h * h)",
                 "result = H_{nu_x}(p0, p1, d0, d1, hx, t)", "C2 in each variable", "get_lower_index"):
        assert text in header, text
    assert "partial-derivative and integral handles" not in header          # moved out of *Not provided*
    lib = C.CDLL(cap.LIB_PATH)
    assert "ndi_interp2d_partial" in cap.SYMBOLS and hasattr(lib, "ndi_interp2d_partial")
    res, args = cap.SYMBOLS["ndi_interp2d_partial"]
    assert res is C.c_int and args[1:3] == [C.c_int32, C.c_int32] and len(args) == 4
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp2d_partial(h: *const ndi_interp2d, nu_x: i32, nu_y: i32, out: *mut *mut ndi_interp2d) -> i32;" in rust
    assert cap.lib().ndi_version() == (0 << 16) | 5     # a new symbol, no new enumerator: no version change
    for m in ("interp_array_into", "finish", "clone", "interp_array_ring", "interp_into", "trim"):   # shared, not copied
        assert getattr(pkg.Bicubic, m) is getattr(pkg.Bilinear, m), m
    assert callable(pkg.Bicubic.partial) and callable(pkg.Interp2D.partial)
    assert pkg.Bicubic.orders == (0, 0)


def test_null_arguments_are_refused_without_a_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    h = C.c_void_p(1234)
    assert lib.ndi_interp2d_partial(None, 1, 0, C.byref(h)) == cap.BAD_ARG
    assert cap.last_error() == "null handle" and h.value is None            # *out is cleared
    assert lib.ndi_interp2d_partial(None, 1, 0, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"


def test_the_mirror_refuses_before_the_library(pkg):
    """Non-integer orders, orders out of range, (0, 0) and a call on Bilinear: decided on an UNBUILT strategy, so no
    library call can have been made."""
    bic = pkg.Bicubic.new()
    for bad in ((1.0, 0), (0, "1"), (None, 1), (1, 0.5)):
        with pytest.raises(TypeError, match=r"Bicubic\.partial: the orders are integers"):
            bic.partial(*bad)
    for bad in ((-1, 0), (0, -1), (-2, -2), (1, -1)):
        with pytest.raises(ValueError, match=r"Bicubic\.partial: an order below 0"):
            bic.partial(*bad)
    for bad in ((3, 0), (0, 3), (2, 7), (3, 3)):
        with pytest.raises(ValueError, match=r"Bicubic\.partial: the third derivative of a cubic spline jumps"):
            bic.partial(*bad)
    for call in (lambda: bic.partial(), lambda: bic.partial(0, 0), lambda: bic.partial(nu_x=0), lambda: bic.partial(nu_y=0)):
        with pytest.raises(ValueError, match=r"Bicubic\.partial: orders \(0, 0\) are the strategy itself"):
            call()
    assert bic.partial.__func__ is pkg.Bicubic.partial
    with pytest.raises(TypeError, match="Bilinear has no partial derivatives"):
        pkg.Bilinear.new().partial(1, 0)
    # through Interp2D: the strategy's refusal, and a strategy that is no device strategy at all
    it = pkg.Interp2D.new_unchecked(np.arange(3.0), np.arange(3.0), np.zeros((3, 3)), pkg.Bilinear.new())
    with pytest.raises(TypeError, match="Bilinear has no partial derivatives"):
        it.partial(1, 0)
    it = pkg.Interp2D.new_unchecked(np.arange(3.0), np.arange(3.0), np.zeros((3, 3)), pkg.Interp2DStrategy())
    with pytest.raises(TypeError, match="partial needs a built Bicubic strategy.*Interp2DStrategy"):
        it.partial(1, 0)
    # numpy integers are integers
    with pytest.raises(pkg.DeviceError):
        bic.partial(np.int64(1), np.int32(0))


def test_partial_without_a_gpu_is_a_loud_device_error(pkg):
    """An unbuilt strategy holds no device handle: partial() says so with a DeviceError, as building without a GPU does;
    with a device, build + partial gives a built Bicubic of the summed orders."""
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        pkg.Bicubic.new().partial(1, 0)
    build = pkg.Interp2DBuilder.new(np.zeros((4, 4))).strategy(pkg.Bicubic.new()).build
    if pkg.device_count() > 0:      # (tests/test_gpu_bicubic_partial.py has the rest)
        p = build().partial(1, 0).partial(0, 2)
        assert isinstance(p.strategy, pkg.Bicubic) and p.strategy.orders == (1, 2)
        return
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        build().partial(1, 0)


# ---- the restatement against scipy --------------------------------------------------------------------------------
def test_golden_covers_the_orders_and_classes_the_specification_names():
    g = golden()
    cases = list(g["cases"])
    assert [tuple(o) for o in g["orders"]] == list(ORDERS) and len(ORDERS) == 8 and (0, 0) not in ORDERS
    assert len(cases) == 18 and sum(c.startswith("float32") for c in cases) == 8
    shapes, lanes, fams, seen = set(), set(), set(), {}
    for cid in cases:
        x, y, z, qx, qy = case(g, cid)
        nx, ny = z.shape[:2]
        labels = list(g[cid + "/labels"])
        assert labels == ["mix", "n3" if min(nx, ny) == 3 else "nk"], cid      # mix on every case; nk where nx, ny >= 4
        assert x.dtype == y.dtype == z.dtype == qx.dtype and z.shape[:2] == (len(x), len(y))
        assert g[cid + "/expect"].shape == (2, 8, len(qx), z.shape[2]) and g[cid + "/expect"].dtype == np.float64
        assert len(qx) == 19 and np.all((qx >= x[0]) & (qx <= x[-1]) & (qy >= y[0]) & (qy <= y[-1]))
        assert np.sum(np.isin(qx, x) & np.isin(qy, y)) >= 5 and (qx[16], qy[16]) == (x[-1], y[-1])   # nodes; the last corner
        assert qx[17] == x[-1] and qy[18] == y[-1]                       # the last knot on each axis alone
        shapes.add((nx, ny)); lanes.add(z.shape[2]); fams |= set(cid.split("_")[-2:])
        for cls in labels:
            key = (cid.split("_")[0], cls)
            seen[key] = seen.get(key, 0) + 1
    assert {(3, 3), (3, 4), (4, 3), (64, 48)} <= shapes and lanes == {1, 2, 3}
    assert fams == {"even", "random", "geometric", "jittered"} and seen == SEEN
    assert os.path.getsize(os.path.join(GOLDEN, "bicubic_partial_scipy.npz")) <= 200 * 1024


@pytest.mark.parametrize("dt,cls", sorted(SEEN))
def test_contract_matches_scipy(dt, cls):
    """max abs error / (max |expected| + 1) per (dtype, class, order) over every golden case of that pair, against 2 x the
    value the generator measured (MEASURED above; DESIGN.md 4.14 repeats the table)."""
    g = golden()
    stored = g[f"measured/{dt}/{cls}"]
    worst, seen = dict.fromkeys(ORDERS, 0.0), 0
    for k, o in enumerate(ORDERS):
        assert abs(float(stored[k]) - MEASURED[(dt, cls) + o]) <= 1e-3 * MEASURED[(dt, cls) + o], (o, stored[k])
    for cid in g["cases"]:
        if not cid.startswith(dt) or cls not in g[cid + "/labels"]:
            continue
        x, y, z, qx, qy = case(g, cid)
        tabs = bicubic_ref.tables(x, y, z, ENDS[cls])
        expect = g[cid + "/expect"][list(g[cid + "/labels"]).index(cls)]
        seen += 1
        for k, (nu_x, nu_y) in enumerate(ORDERS):
            got = bicubic_partial_ref.evaluate(x, y, z, *tabs, qx, qy, nu_x, nu_y)
            assert got.dtype == np.dtype(dt)
            err = float(np.abs(got.astype(np.float64) - expect[k]).max() / (np.abs(expect[k]).max() + 1))
            worst[(nu_x, nu_y)] = max(worst[(nu_x, nu_y)], err)
            print(f"{cid} {cls} ({nu_x}, {nu_y}): {err:.3e}, bound {2.0 * MEASURED[(dt, cls, nu_x, nu_y)]:.3e}")
            assert err <= 2.0 * MEASURED[(dt, cls, nu_x, nu_y)], (cid, cls, nu_x, nu_y, err)
    assert seen == SEEN[(dt, cls)]
    print(f"{dt} {cls}: largest errors against scipy {worst}")


@pytest.mark.parametrize("variant", bicubic_partial_ref.MUTANTS)
def test_the_goldens_tell_a_mutant_from_the_contract(variant):
    """H1 divided by h * h, or 3 for the 6 of H2: over the orders the mutant touches it misses the goldens by at least
    1e6 x the largest f64 bound."""
    g = golden()
    touched = [k for k, o in enumerate(ORDERS) if (1 if variant == "h1_over_hh" else 2) in o]
    worst = 0.0
    for cid in g["cases"]:
        if not cid.startswith("float64"):
            continue
        x, y, z, qx, qy = case(g, cid)
        for c, cls in enumerate(g[cid + "/labels"]):
            tabs = bicubic_ref.tables(x, y, z, ENDS[cls])
            for k in touched:
                got = bicubic_partial_ref.evaluate(x, y, z, *tabs, qx, qy, *ORDERS[k], variant=variant)
                e = g[cid + "/expect"][c][k]
                worst = max(worst, float(np.abs(got - e).max() / (np.abs(e).max() + 1)))
    assert worst >= 1e6 * 2.0 * max(v for k, v in MEASURED.items() if k[0] == "float64"), worst


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_orders_zero_are_the_surface_bit_for_bit(dt):
    g = golden()
    for cid in g["cases"]:
        if not cid.startswith(dt):
            continue
        x, y, z, qx, qy = case(g, cid)
        for ends in (ENDS["nk"], ENDS["mix"]):
            tabs = bicubic_ref.tables(x, y, z, ends)
            a = bicubic_partial_ref.evaluate(x, y, z, *tabs, qx, qy, 0, 0)
            b = bicubic_ref.evaluate(x, y, z, *tabs, qx, qy)
            assert a.dtype == b.dtype == np.dtype(dt) and a.tobytes() == b.tobytes(), cid
