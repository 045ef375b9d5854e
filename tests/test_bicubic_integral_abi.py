"""CPU: 2-D antiderivative handles and rectangle integrals of Bicubic at the boundary -- the three new entry points in the
header, the ctypes binding, the built library and the Rust declarations; the refusals that need no device, the library's and
the mirror's; and the accuracy of the contract's numpy restatement (tests/bicubic_integral_ref.py, what the GPU tests compare
the device against bit for bit) against scipy through tests/golden/bicubic_integral_scipy.npz
(tests/golden/gen_bicubic_integral_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import bicubic_integral_ref as ref
import bicubic_ref
from conftest import GOLDEN, ROOT
from test_bicubic_abi import ENDS

# Largest error of the restatement against f64 scipy over the golden file, max abs error / (max |expected| + 1) per (dtype,
# class), as tests/golden/gen_bicubic_integral_golden.py measured and printed it; the bar is 2 x each (the project's margin
# in test_bicubic_abi.py / test_bicubic_partial_abi.py).
MEASURED = {
    ("float32", "mix"): 2.664e-07,
    ("float32", "n3"): 1.650e-07,
    ("float32", "nk"): 1.703e-07,
    ("float64", "mix"): 6.372e-16,
    ("float64", "n3"): 1.014e-16,
    ("float64", "nk"): 8.082e-14,
}
SEEN = {("float64", "mix"): 11, ("float64", "n3"): 3, ("float64", "nk"): 8,
        ("float32", "mix"): 11, ("float32", "n3"): 3, ("float32", "nk"): 8}
MUTANTS = ({"pp_along_y": True}, {"serial": True}, {"block": 128}, {"no_third": True}, {"other_association": True})


def golden():
    return np.load(os.path.join(GOLDEN, "bicubic_integral_scipy.npz"))


def case(g, cid):
    return tuple(g[f"{cid}/{k}"] for k in ("x", "y", "z", "r"))


def rel_err(got, expect):
    return float(np.abs(got.astype(np.float64) - expect).max() / (np.abs(expect).max() + 1))


# ---- the boundary ------------------------------------------------------------------------------------------------
def test_header_capi_library_and_rust_carry_the_symbols(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    for text in ("ndi_status ndi_interp2d_antiderivative(const ndi_interp2d* h, ndi_interp2d** out);",
                 "ndi_status ndi_interp2d_integral(const ndi_interp2d* h, const void* xa, const void* xb, const void* ya, "
                 "const void* yb,",
                 "ndi_status ndi_interp2d_integral_tables(const ndi_interp2d* h, void* pp, void* qz, void* qzy, void* pz, "
                 "void* pzx,",
                 "c1 = (d + a) * 0.5;  c2 = (b - (a + a)) / 3;  c3 = (b - a) * 0.25",
                 "s * (pl + s * (c1 + s * (c2 - s * c3)))", "I = h * (pl + (c1 + (c2 - c3)))",
                 "PP  = prefix along x of (values Pz, slopes Pzx)", "F  = e + hx * G(w0, w1, v0, v1, hx, t)",
                 "out = (F(xb, yb) - F(xa, yb)) - (F(xb, ya) - F(xa, ya))", "async_launch != 0 is NDI_UNSUPPORTED"):
        assert text in header, text
    assert "Pchip / Akima node derivatives, integral handles" not in header      # moved out of *Not provided*
    lib = C.CDLL(cap.LIB_PATH)
    for name, nargs in (("ndi_interp2d_antiderivative", 2), ("ndi_interp2d_integral", 10), ("ndi_interp2d_integral_tables", 7)):
        assert name in cap.SYMBOLS and hasattr(lib, name), name
        res, args = cap.SYMBOLS[name]
        assert res is C.c_int and len(args) == nargs, name
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp2d_antiderivative(h: *const ndi_interp2d, out: *mut *mut ndi_interp2d) -> i32;" in rust
    assert "pub fn ndi_interp2d_integral(" in rust and "pub fn ndi_interp2d_integral_tables(" in rust
    assert cap.lib().ndi_version() == (0 << 16) | 5     # new symbols, no new enumerator: no version change
    for m in ("antiderivative", "integral", "integral_tables"):
        assert callable(getattr(pkg.Bicubic, m)), m
    assert callable(pkg.Interp2D.antiderivative) and callable(pkg.Interp2D.integral)
    assert pkg.Bicubic.is_integral is False


def test_argument_validation_needs_no_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    h = C.c_void_p(1234)
    assert lib.ndi_interp2d_antiderivative(None, C.byref(h)) == cap.BAD_ARG
    assert cap.last_error() == "null handle" and h.value is None            # *out is cleared
    assert lib.ndi_interp2d_antiderivative(None, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"
    buf = np.zeros(4)
    p = buf.ctypes.data
    assert lib.ndi_interp2d_integral(None, p, p, p, p, 1, p, 1, None, None) == cap.BAD_ARG and cap.last_error() == "null handle"
    assert lib.ndi_interp2d_integral_tables(None, p, None, None, None, None, cap.MEM_HOST) == cap.BAD_ARG
    assert cap.last_error() == "null handle"


def test_the_mirror_refuses_before_the_library(pkg):
    """Decided on UNBUILT strategies, so no library call can have been made."""
    with pytest.raises(TypeError, match="Bilinear has no antiderivative handle"):
        pkg.Bilinear.new().antiderivative()
    with pytest.raises(TypeError, match="Bilinear has no rectangle integral"):
        pkg.Bilinear.new().integral(0, 1, 0, 1, None)
    k = np.arange(3.0)
    it = pkg.Interp2D.new_unchecked(k, k, np.zeros((3, 3)), pkg.Bilinear.new())
    with pytest.raises(TypeError, match="Bilinear has no antiderivative handle"):
        it.antiderivative()
    with pytest.raises(TypeError, match="Interp2D.integral needs the antiderivative of a Bicubic interpolator, got Bilinear"):
        it.integral(0.0, 1.0, 0.0, 1.0)
    it = pkg.Interp2D.new_unchecked(k, k, np.zeros((3, 3)), pkg.Interp2DStrategy())
    with pytest.raises(TypeError, match="antiderivative needs a built Bicubic strategy.*Interp2DStrategy"):
        it.antiderivative()
    bic = pkg.Interp2D.new_unchecked(k, k, np.zeros((3, 3)), pkg.Bicubic.new())
    with pytest.raises(TypeError, match="this is a Bicubic interpolator of the surface.*antiderivative\\(\\) first"):
        bic.integral(0.0, 1.0, 0.0, 1.0)
    with pytest.raises(TypeError, match="Bicubic.integral needs the integral strategy"):
        pkg.Bicubic.new().integral(k, k, k, k, np.zeros((3, 1)))
    # an integral strategy (marked by hand: there is no device here): mismatched bounds, partials, a second antiderivative
    s = pkg.Bicubic.new()
    s.is_integral = True
    fake = pkg.Interp2D.new_unchecked(k, k, np.zeros((3, 3)), s)
    with pytest.raises(ValueError, match="Bicubic integral: the bound shapes do not broadcast"):
        fake.integral(np.zeros(3), np.zeros(4), 0.0, 1.0)
    with pytest.raises(ValueError, match="Bicubic.partial: an integral strategy has no partial derivatives.*y-integral"):
        s.partial(1, 0)
    with pytest.raises(ValueError, match="Bicubic.antiderivative: this strategy is already an integral"):
        s.antiderivative()
    p = pkg.Bicubic.new()
    p.orders = (1, 0)
    with pytest.raises(ValueError, match="Bicubic.antiderivative: a partial-derivative strategy"):
        p.antiderivative()


def test_antiderivative_without_a_gpu_is_a_loud_device_error(pkg):
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        pkg.Bicubic.new().antiderivative()
    build = pkg.Interp2DBuilder.new(np.zeros((4, 4))).strategy(pkg.Bicubic.new()).build
    if pkg.device_count() > 0:      # (tests/test_gpu_bicubic_integral.py has the rest)
        F = build().antiderivative()
        assert isinstance(F.strategy, pkg.Bicubic) and F.strategy.is_integral
        return
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        build().antiderivative()


# ---- the restatement against scipy --------------------------------------------------------------------------------
def test_golden_covers_the_cases_the_specification_names():
    g = golden()
    cases = list(g["cases"])
    assert len(cases) == 22 and sum(c.startswith("float32") for c in cases) == 11
    shapes, lanes, fams, seen = set(), set(), set(), {}
    for cid in cases:
        x, y, z, r = case(g, cid)
        nx, ny = z.shape[:2]
        labels = list(g[cid + "/labels"])
        assert labels == ["mix", "n3" if min(nx, ny) == 3 else "nk"], cid      # mix on every case; nk where nx, ny >= 4
        assert x.dtype == y.dtype == z.dtype == r.dtype and z.shape[:2] == (len(x), len(y)) and r.shape == (4, 12)
        assert g[cid + "/expect"].shape == (2, 12, z.shape[2]) and g[cid + "/expect"].dtype == np.float64
        xa, xb, ya, yb = r
        assert (xa[0], xb[0], ya[0], yb[0]) == (x[0], x[-1], y[0], y[-1])                    # the whole domain
        assert xa[1] == xb[1] and ya[2] == yb[2] and xa[3] == xb[3] and ya[3] == yb[3]       # degenerate ones
        assert xa[4] >= xb[4] and ya[4] <= yb[4] and xa[5] >= xb[5] and ya[5] >= yb[5]       # reversed bounds
        assert np.all(np.isin(np.concatenate([xa[6:8], xb[6:8]]), x)) and np.all(np.isin(np.concatenate([ya[6:8], yb[6:8]]), y))
        assert np.all((r[:2] >= x[0]) & (r[:2] <= x[-1])) and np.all((r[2:] >= y[0]) & (r[2:] <= y[-1]))
        shapes.add((nx, ny)); lanes.add(z.shape[2]); fams |= set(cid.split("_")[-2:])
        for cls in labels:
            key = (cid.split("_")[0], cls)
            seen[key] = seen.get(key, 0) + 1
    # 3 points on an axis; axes that cross the block edges 256 / 257 (x), 512 / 513 (x and y)
    assert {(3, 3), (3, 4), (4, 3), (257, 5), (5, 513), (513, 4)} <= shapes and lanes == {1, 2, 3}
    assert fams == {"even", "random", "geometric", "jittered"} and seen == SEEN
    assert os.path.getsize(os.path.join(GOLDEN, "bicubic_integral_scipy.npz")) <= 200 * 1024


@pytest.mark.parametrize("dt,cls", sorted(SEEN))
def test_contract_matches_scipy(dt, cls):
    """max abs error / (max |expected| + 1) per (dtype, class) over every golden case of that pair, against 2 x the value
    the generator measured (MEASURED above; DESIGN.md 4.15 repeats the table)."""
    g = golden()
    stored = float(g[f"measured/{dt}/{cls}"])
    assert abs(stored - MEASURED[(dt, cls)]) <= 1e-3 * MEASURED[(dt, cls)], stored
    worst, seen = 0.0, 0
    for cid in g["cases"]:
        if not cid.startswith(dt) or cls not in g[cid + "/labels"]:
            continue
        x, y, z, r = case(g, cid)
        got = ref.integral(x, y, z, *r, ENDS[cls])
        assert got.dtype == np.dtype(dt)
        expect = g[cid + "/expect"][list(g[cid + "/labels"]).index(cls)]
        err = rel_err(got, expect)
        print(f"{cid} {cls}: {err:.3e}, bound {2.0 * MEASURED[(dt, cls)]:.3e}")
        assert err <= 2.0 * MEASURED[(dt, cls)], (cid, cls, err)
        worst, seen = max(worst, err), seen + 1
    assert seen == SEEN[(dt, cls)]
    print(f"{dt} {cls}: largest error against scipy {worst:.3e}")


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: next(iter(m)))
def test_mutants_miss_the_goldens_or_give_other_bits(mutant):
    """A wrong rule (c2 without the / 3) misses the f64 goldens by 1e6 x the bound.  Another summation order (PP along y,
    one serial sum, B = 128) or the other association of the rectangle is the same number mathematically: it stays inside
    the bound and gives OTHER BITS, in every case that can tell (an axis longer than the block for the block mutants)."""
    g = golden()
    worst, differ, total = 0.0, 0, 0
    for cid in g["cases"]:
        if not cid.startswith("float64"):
            continue
        x, y, z, r = case(g, cid)
        for c, cls in enumerate(g[cid + "/labels"]):
            got = ref.integral(x, y, z, *r, ENDS[cls], **mutant)
            worst = max(worst, rel_err(got, g[cid + "/expect"][c]))
            if "block" in mutant and max(z.shape[:2]) <= 128:
                continue                                    # one block either way: the same bits by construction
            total += 1
            differ += got.tobytes() != ref.integral(x, y, z, *r, ENDS[cls]).tobytes()
    if "no_third" in mutant:
        assert worst >= 1e6 * 2.0 * max(v for k, v in MEASURED.items() if k[0] == "float64"), worst
        return
    assert worst <= 2.0 * max(v for k, v in MEASURED.items() if k[0] == "float64"), worst     # the same number ...
    print(f"{mutant}: other bits in {differ} of {total} cases")
    if "block" in mutant or "serial" in mutant:
        assert differ >= 1, (mutant, differ, total)
    else:
        assert differ >= total // 2, (mutant, differ, total)                                  # ... in other bits


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_degenerate_rectangles_are_exact_zeros_and_reversed_ones_negate(dt):
    g = golden()
    for cid in g["cases"]:
        if not cid.startswith(dt):
            continue
        x, y, z, (xa, xb, ya, yb) = case(g, cid)
        for ends in (ENDS["nk"], ENDS["mix"]):
            rows = ref.integral(x, y, z, xa, xb, ya, yb, ends)
            assert np.all(rows[1:4] == 0), cid                              # xa == xb, ya == yb, both: 0 - 0 or d - d
            assert np.any(rows[0] != 0)
            swapped = ref.integral(x, y, z, xb, xa, ya, yb, ends)           # x bounds exchanged: the exact negative
            assert np.array_equal(swapped, -rows), cid
            both = ref.integral(x, y, z, xb, xa, yb, ya, ends)
            assert np.allclose(both, rows, rtol=0, atol=(1e-12 if dt == "float64" else 1e-4) * (np.abs(rows).max() + 1)), cid


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_a_bicubic_polynomial_integrates_to_its_closed_form(dt):
    """Not-a-knot ends reproduce f(x, y) = x^3 - 2 x y^2 + x^2 y^3 + 1, so the rectangle integral is that of the
    polynomial: a few ulps of the largest antiderivative value."""
    rng = np.random.default_rng(7)
    x = np.cumsum(rng.uniform(0.2, 0.4, 9)).astype(dt)
    y = (np.cumsum(rng.uniform(0.2, 0.4, 7)) - 1.0).astype(dt)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    z = (x64[:, None] ** 3 - 2.0 * x64[:, None] * y64[None, :] ** 2 + x64[:, None] ** 2 * y64[None, :] ** 3 + 1.0)
    z = z.astype(dt)[:, :, None]

    def anti(u, v):
        return u ** 4 / 4 * v - u * u * v ** 3 / 3 + u ** 3 / 3 * v ** 4 / 4 + u * v

    xa, xb = rng.uniform(x[0], x[-1], 50).astype(dt), rng.uniform(x[0], x[-1], 50).astype(dt)
    ya, yb = rng.uniform(y[0], y[-1], 50).astype(dt), rng.uniform(y[0], y[-1], 50).astype(dt)
    xa[0], xb[0], ya[0], yb[0] = x[0], x[-1], y[0], y[-1]
    a, b, c, d = (q.astype(np.float64) for q in (xa, xb, ya, yb))
    want = (anti(b, d) - anti(a, d)) - (anti(b, c) - anti(a, c))
    got = ref.integral(x, y, z, xa, xb, ya, yb)[:, 0].astype(np.float64)
    scale = max(abs(anti(u, v)) for u in (x64[0], x64[-1]) for v in (y64[0], y64[-1])) + 1
    bound = 64 * np.finfo(dt).eps * scale       # z itself is rounded to dt: a few ulps of the largest term per operation
    print(f"{np.dtype(dt).name}: largest deviation from the closed form {np.abs(got - want).max():.3e}, bound {bound:.3e}")
    assert np.abs(got - want).max() <= bound
