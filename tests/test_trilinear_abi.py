"""CPU: the Trilinear reference (tests/trilinear_ref.py) against itself and against scipy, the ABI of include/ndinterp3d.h
(symbols, struct layout, strict C99), the refusals and builder errors that are decided before any device work, and the loud
failure without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import trilinear_ref as tr
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ndinterp3d.h")
GRIDS = [(2, 2, 2), (3, 2, 4), (5, 4, 3)]
DTYPES = [np.float32, np.float64]


def axis(rng, n, dt):
    """a non-uniform strictly rising axis"""
    return np.cumsum(rng.uniform(0.5, 1.5, n)).astype(dt)


def product_queries(x, y, z, outside):
    """every knot and every cell midpoint of each axis (the full product), `outside` appended on each axis"""
    per = [np.concatenate([tr.knots_and_midpoints(k), np.asarray(o, k.dtype)]) for k, o in zip((x, y, z), outside)]
    g = np.meshgrid(*per, indexing="ij")
    return [np.ascontiguousarray(a.ravel()) for a in g]


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", GRIDS)
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("extrapolate", [False, True])
def test_the_two_reference_forms_agree(dt, shape, lanes, extrapolate):
    rng = np.random.default_rng(7)
    x, y, z = (axis(rng, n, dt) for n in shape)
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    far = [[k[0] - 3, k[-1] + 2.5] for k in (x, y, z)]
    if extrapolate:
        qx, qy, qz = product_queries(x, y, z, far)               # the end cells continue
    else:
        qx, qy, qz = product_queries(x, y, z, [[], [], []])
        qx, qy, qz = (np.concatenate([q, np.asarray(o, dt)]) for q, o in zip((qx, qy, qz), far))   # two failing queries last
    a = tr.trilinear_ref(x, y, z, data, qx, qy, qz, extrapolate)
    b = tr.trilinear_direct(x, y, z, data, qx, qy, qz, extrapolate)
    assert a[:2] == b[:2] == ((None, None) if extrapolate else (qx.size - 2, 0))
    assert np.array_equal(tr.bits(a[2]), tr.bits(b[2]))
    assert np.isfinite(a[2]).all() and np.abs(a[2][:qx.size - 2]).max() > 0
    # on the knots the interpolant is the data (three nested calc_frac, each three roundings of magnitudes below 4)
    kx, ky, kz = np.meshgrid(x, y, z, indexing="ij")
    on = tr.trilinear_ref(x, y, z, data, kx.ravel(), ky.ravel(), kz.ravel(), extrapolate)[2]
    assert np.allclose(on, data.reshape(-1, lanes), rtol=0, atol=3 * 3 * 4 * np.finfo(dt).eps)


def test_first_failure_order():
    x = y = z = np.array([0.0, 1.0, 2.0])
    q = np.array([0.5, 0.5, 0.5, 0.5])
    assert tr.first_failure(x, y, z, q, q, q, False) == (None, None)
    qz = q.copy(); qz[1] = 9.0
    qx = q.copy(); qx[2] = -1.0
    assert tr.first_failure(x, y, z, qx, q, qz, False) == (1, 2)      # the lower index wins, on z
    qx[1] = np.nan
    assert tr.first_failure(x, y, z, qx, q, qz, False) == (1, 0)      # x before z within a query; NaN fails the range test
    assert tr.first_failure(x, y, z, qx, q, qz, True) == (1, 0)       # extrapolating: only the NaN fails
    qx[1] = 0.5
    assert tr.first_failure(x, y, z, qx, q, qz, True) == (None, None)


@pytest.mark.parametrize("dt", DTYPES)
def test_reference_against_scipy(dt):
    """scipy forms the eight weights and sums, another order of the same handful of operations: 8 ulp of 1.0 for data in
    [-1, 1], four times the 3.9e-16 (f64) / 1.6e-7 (f32) first measured on a 5 x 4 x 3 x 3 grid with 2000 queries.  Measured
    maximum on this case (the same shape, seed 11): 4.44e-16 (f64, 2 ulp), 1.91e-7 (f32, 1.6 ulp)."""
    interpolate = pytest.importorskip("scipy.interpolate")
    rng = np.random.default_rng(11)
    shape = (5, 4, 3)
    x, y, z = (axis(rng, n, dt) for n in shape)
    data = rng.uniform(-1, 1, shape + (3,)).astype(dt)
    qx, qy, qz = (rng.uniform(k[0], k[-1], 2000).astype(dt) for k in (x, y, z))
    qx, qy, qz = (np.clip(q, k[0], k[-1]) for q, k in zip((qx, qy, qz), (x, y, z)))
    fail, _, got = tr.trilinear_ref(x, y, z, data, qx, qy, qz)
    assert fail is None
    want = interpolate.RegularGridInterpolator((x, y, z), data, method="linear")(np.stack([qx, qy, qz], axis=1))
    err = np.abs(got.astype(np.float64) - np.asarray(want, np.float64)).max()
    print(f"trilinear_ref against scipy, {np.dtype(dt)}: max abs difference {err:.3g}")
    assert err <= 8 * np.finfo(dt).eps


@pytest.mark.parametrize("dt", DTYPES)
def test_reference_slab_property(dt):
    """at qz = z[k], k < nz - 1, the row is the slab's Bilinear row exactly"""
    import oracle
    rng = np.random.default_rng(12)
    shape = (5, 4, 3)
    x, y, z = (axis(rng, n, dt) for n in shape)
    data = rng.uniform(-1, 1, shape + (3,)).astype(dt)
    qx, qy = (np.clip(rng.uniform(k[0], k[-1], 200).astype(dt), k[0], k[-1]) for k in (x, y))
    for k in range(shape[2] - 1):
        got = tr.trilinear_ref(x, y, z, data, qx, qy, np.full(200, z[k], dt))[2]
        slab = oracle.interp2d_bilinear(x, y, np.ascontiguousarray(data[:, :, k]), qx, qy)[3]
        assert np.array_equal(tr.bits(got), tr.bits(slab))


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def _header_text(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    return sorted(set(re.findall(r"\b(ndi_[a-z0-9_]+)\s*\(", _header_text(path))))


def test_header_symbols_are_exported_and_bound(pkg):
    names = _declared()
    assert names == ["ndi_interp3d_clone", "ndi_interp3d_create", "ndi_interp3d_destroy", "ndi_interp3d_eval"]
    lib = C.CDLL(pkg._capi.LIB_PATH)
    assert not [n for n in names if not hasattr(lib, n)]
    assert sorted(pkg._capi.SYMBOLS3D) == names                       # the 3-D table binds exactly the 3-D header
    bound = pkg._capi.lib()
    for n in names:
        assert getattr(bound, n).argtypes == pkg._capi.SYMBOLS3D[n][1]


def test_main_header_still_declares_exactly_the_main_table(pkg):
    """no 3-D symbol may slip into include/ndinterp.h or into SYMBOLS"""
    main = _declared(os.path.join(ROOT, "include", "ndinterp.h"))
    assert sorted(pkg._capi.SYMBOLS) == main
    assert not [n for n in main if "3d" in n] and not set(main) & set(pkg._capi.SYMBOLS3D)
    assert pkg._capi.lib().ndi_version() == (0 << 16) | 5


def test_desc_matches_the_header_field_by_field(pkg):
    text = _header_text()
    body = re.search(r"typedef struct ndi_interp3d_desc \{(.*?)\} ndi_interp3d_desc;", text, flags=re.S).group(1)
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "const void*": C.c_void_p}
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(int32_t|uint64_t|const void\s?\*)\s*(.*)", decl)
        assert m, decl
        t = ctype[m.group(1).replace(" *", "*")]
        for name in m.group(2).split(","):
            name = name.strip()
            assert re.fullmatch(r"[a-z_]+", name), decl     # (`const void *x, *y` would bind the star to the name)
            fields.append((name, t))
    got = [(n, t) for n, t in pkg._capi.Interp3DDesc._fields_]
    assert [n for n, _ in got] == [n for n, _ in fields]
    assert [C.sizeof(t) for _, t in got] == [C.sizeof(t) for _, t in fields]
    off = 0
    for name, t in fields:                                   # natural alignment, as the C compiler lays it out
        off = (off + C.sizeof(t) - 1) // C.sizeof(t) * C.sizeof(t)
        assert getattr(pkg._capi.Interp3DDesc, name).offset == off, name
        off += C.sizeof(t)
    assert C.sizeof(pkg._capi.Interp3DDesc) == (off + 7) // 8 * 8 == 112


def test_header_and_example_are_plain_c99(pkg, tmp_path):
    src = tmp_path / "only_header.c"
    src.write_text('#include "ndinterp3d.h"\nint main(void) { ndi_interp3d_desc d; (void)d; return (int)sizeof(ndi_interp3d_desc) - 112; }\n')
    flags = ["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include")]
    r = subprocess.run(flags + [str(src), "-o", str(tmp_path / "only_header")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "only_header")]).returncode == 0      # sizeof as ctypes has it
    exe = tmp_path / "c_abi_trilinear"
    r = subprocess.run(flags + [os.path.join(ROOT, "examples", "c_abi_trilinear.c"), "-L", os.path.join(ROOT, "ndarray-interp_amd"),
                                "-lndinterp_hip", "-Wl,-rpath," + os.path.join(ROOT, "ndarray-interp_amd"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    if pkg._capi.lib().ndi_device_count() == 0:
        assert run.returncode == 1 and "no CPU fallback" in run.stderr      # loud failure without a GPU
    else:
        assert run.returncode == 0, run.stdout + run.stderr
        f = lambda x, y, z: 1 + 2 * x - 3 * y + 0.5 * z   # noqa: E731
        pts = zip((0.0, 0.5, 2.0, 3.0, 1.25), (-1.0, -0.5, 0.25, 0.5, 0.0), (0.0, 1.0, 3.0, 4.0, 2.5))
        assert [float(v) for v in run.stdout.split()] == [f(*p) for p in pts]


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


def test_create_and_eval_refusals_need_no_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    data = np.zeros((2, 2, 2))
    k = np.array([0.0, 1.0])
    h = C.c_void_p(0xdead)
    assert lib.ndi_interp3d_create(None, C.byref(h)) == cap.BAD_ARG and h.value is None      # *out cleared
    d = host_desc(pkg, k, k, k, data)
    assert lib.ndi_interp3d_create(C.byref(d), None) == cap.BAD_ARG
    for dtype in (cap.I32, cap.I64, cap.F16, cap.BF16, 7, -1):
        d = host_desc(pkg, k, k, k, data)
        d.dtype = dtype
        h = C.c_void_p(0xdead)
        assert lib.ndi_interp3d_create(C.byref(d), C.byref(h)) == cap.BAD_ARG and h.value is None
        assert "f32 / f64" in cap.last_error()
    d = host_desc(pkg, k, k, k, data)
    d.reserved = 1
    assert lib.ndi_interp3d_create(C.byref(d), C.byref(h)) == cap.BAD_ARG and "reserved" in cap.last_error()
    assert lib.ndi_interp3d_clone(None, 0, C.byref(h)) == cap.BAD_ARG
    lib.ndi_interp3d_destroy(None)                                                          # a no-op
    # ndi_interp3d_eval: what is decided from the options alone comes before the handle is looked at
    assert lib.ndi_interp3d_eval(None, None, None, None, 0, None, 0, None, None) == cap.BAD_ARG
    assert "null handle" in cap.last_error()
    for field, value, status, text in (("flags", 4, cap.BAD_ARG, "unknown bits"), ("reserved", 1, cap.BAD_ARG, "reserved"),
                                       ("path", cap.PATH_BUCKETED, cap.BAD_ARG, "NDI_PATH_BUCKETED"),
                                       ("async_launch", 1, cap.UNSUPPORTED, "async_launch")):
        opts = cap.EvalOpts()
        setattr(opts, field, value)
        assert lib.ndi_interp3d_eval(None, None, None, None, 0, None, 0, C.byref(opts), None) == status, field
        assert text in cap.last_error(), (field, cap.last_error())


def test_validation_on_host_axes_in_the_builders_order(pkg):
    """validate != 0 with host axes: the builder's errors, interp2d/mod.rs:480-509's order with a third axis, before the
    device is asked for"""
    cap, lib = pkg._capi, pkg._capi.lib()
    h = C.c_void_p()
    up = lambda n: np.arange(float(n))   # noqa: E731

    def create(x, y, z, shape):
        d = host_desc(pkg, x, y, z, np.zeros(shape))
        return lib.ndi_interp3d_create(C.byref(d), C.byref(h)), cap.last_error()
    bad = np.array([0.0, 2.0, 1.0])
    # every defect at once: the length of axis 0 is reported; then 1, 2; then the three shapes; then x, y, z not rising
    assert create(up(5), up(5), bad, (1, 1, 1)) == (cap.NOT_ENOUGH_DATA, "The 0-dimension has not enough data for the chosen "
                                                    "interpolation strategy. Provided: 1, Reqired: 2")
    assert create(up(5), up(5), bad, (2, 1, 1))[1].startswith("The 1-dimension has not enough data")
    st, msg = create(up(5), up(5), bad, (2, 2, 1))
    assert st == cap.NOT_ENOUGH_DATA and msg.startswith("The 2-dimension has not enough data")
    assert create(up(5), up(5), bad, (2, 2, 2)) == (cap.SHAPE, "Lenghts of x-axis and data-0-axis need to match. Got x: 5, data-0: 2")
    assert create(up(2), up(5), bad, (2, 2, 2)) == (cap.SHAPE, "Lenghts of y-axis and data-1-axis need to match. Got y: 5, data-1: 2")
    assert create(up(2), up(2), bad, (2, 2, 2)) == (cap.SHAPE, "Lenghts of z-axis and data-2-axis need to match. Got z: 3, data-2: 2")
    assert create(up(2), up(2), bad, (2, 2, 3)) == (cap.MONOTONIC, "The z-axis needs to be strictly monotonic rising")     # z alone
    assert create(bad, up(2), bad, (3, 2, 3)) == (cap.MONOTONIC, "The x-axis needs to be strictly monotonic rising")       # x and z
    assert create(up(3), bad, bad, (3, 3, 3)) == (cap.MONOTONIC, "The y-axis needs to be strictly monotonic rising")
    tie = np.array([0.0, 1.0, 1.0])
    assert create(None, None, tie, (2, 2, 3))[0] == cap.MONOTONIC         # a NULL axis is 0..n and passes
    assert create(None, None, np.array([0.0, np.nan, 2.0]), (2, 2, 3))[0] == cap.MONOTONIC


def test_mirror_builder_errors_in_order(pkg):
    B, E = pkg.Interp3DBuilder, pkg.BuilderError
    up = lambda n: np.arange(float(n))   # noqa: E731
    bad = np.array([0.0, 2.0, 1.0])

    def build(x, y, z, shape):
        return pkg.Interp3D.builder(np.zeros(shape)).x(x).y(y).z(z).strategy(pkg.Trilinear.new()).build()
    with pytest.raises(E.ShapeError, match="data dimension needs to be at least 3"):
        B.new(np.zeros((4, 4))).build()
    for a, shape in enumerate([(1, 1, 1), (2, 1, 1), (2, 2, 1)]):
        with pytest.raises(E.NotEnoughData, match=f"The {a}-dimension has not enough data .* Provided: 1, Reqired: 2"):
            build(up(5), up(5), bad, shape)
    for a, (name, axes) in enumerate(zip("xyz", [(up(5), up(5), bad), (up(2), up(5), bad), (up(2), up(2), bad)])):
        with pytest.raises(E.ShapeError, match=f"Lenghts of {name}-axis and data-{a}-axis need to match"):
            build(*axes, (2, 2, 2))
    with pytest.raises(E.Monotonic, match="The z-axis needs"):
        build(up(2), up(2), bad, (2, 2, 3))
    with pytest.raises(E.Monotonic, match="The x-axis needs"):
        build(bad, up(2), bad, (3, 2, 3))
    with pytest.raises(E.Monotonic, match="The y-axis needs"):
        build(up(3), bad, bad, (3, 3, 3))


def test_mirror_type_and_value_errors(pkg):
    with pytest.raises(TypeError, match="Trilinear takes float32 / float64"):
        pkg.Interp3DBuilder.new(np.zeros((2, 2, 2), dtype=np.int32)).build()
    with pytest.raises(TypeError, match="Trilinear"):
        pkg.Interp3DBuilder.new(np.zeros((2, 2, 2), dtype=np.float16)).build()
    k = np.array([0.0, 1.0])
    it = pkg.Interp3D.new_unchecked(k, k, k, np.zeros((2, 2, 2, 5)), None)
    with pytest.raises(ValueError, match="equal shapes"):
        it.interp_array(np.zeros(3), np.zeros(3), np.zeros(4))
    with pytest.raises(ValueError, match="equal shapes"):
        it.interp_array_into(np.zeros((2, 3)), np.zeros((3, 2)), np.zeros((2, 3)), np.zeros((2, 3, 5)))
    with pytest.raises(TypeError, match="interp_scalar needs 3-D data"):
        it.interp_scalar(0.5, 0.5, 0.5)
    assert it.get_buffer_shape((4, 2)) == (4, 2, 5)
    assert it.is_in_x_range(0.5) and not it.is_in_y_range(1.5) and not it.is_in_z_range(float("nan"))
    assert it.index_point(1, 0, 1)[:3] == (1.0, 0.0, 1.0) and it.index_point(1, 0, 1)[3].shape == (5,)


def test_no_device_means_loud_failure(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.DeviceError, match="no CPU fallback"):
        pkg.Interp3DBuilder.new(np.zeros((2, 2, 2))).build()
