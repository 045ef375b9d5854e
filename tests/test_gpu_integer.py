"""i32 / i64 Linear and Bilinear on the device (.device(0) or GPU tensors): bit-exact against the reference's integer
semantics (generic_host: truncating division, a panic on any intermediate that overflows T), first-error precedence,
and every evaluation entry point."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
INFO = {np.int32: np.iinfo(np.int32), np.int64: np.iinfo(np.int64)}


def _vec():
    with open(os.path.join(GOLDEN, "reference_integer_vectors.json")) as f:
        return json.load(f)


def _lin(pkg, x, data, extrapolate=False, device=True):
    s = pkg.Linear.new().extrapolate(extrapolate)
    if device:
        s = s.device(0)
    b = pkg.Interp1DBuilder.new(data)
    if x is not None:
        b = b.x(x)
    interp = b.strategy(s).build()
    if device and np.dtype(data.dtype) in (np.dtype(np.int32), np.dtype(np.int64)):
        assert type(interp.strategy).__name__ == "Linear" and interp.strategy._h is not None   # the device strategy
    return interp


def _bil(pkg, x, y, data, extrapolate=False, device=True):
    s = pkg.Bilinear.new().extrapolate(extrapolate)
    if device:
        s = s.device(0)
    b = pkg.Interp2DBuilder.new(data)
    if x is not None:
        b = b.x(x)
    if y is not None:
        b = b.y(y)
    interp = b.strategy(s).build()
    if device and np.dtype(data.dtype) in (np.dtype(np.int32), np.dtype(np.int64)):
        assert type(interp.strategy).__name__ != "HostBilinear" and interp.strategy._h is not None
    return interp


def _trunc_div(a, b):
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) == (b < 0), q, -q)


def _lin_ref(x, data, q):
    """Vectorised Linear in exact i64 (valid for data / queries whose intermediates fit i32)."""
    x = x.astype(np.int64); d2 = data.reshape(len(x), -1).astype(np.int64); q = q.astype(np.int64)
    i = np.clip(np.searchsorted(x, q, side="right") - 1, 0, len(x) - 2)
    y1, y2 = d2[i], d2[i + 1]
    m = _trunc_div(y2 - y1, (x[i + 1] - x[i])[:, None])
    return m * (q - x[i])[:, None] + y1


def _bil_ref(x, y, g, qx, qy):
    x = x.astype(np.int64); y = y.astype(np.int64); g3 = g.reshape(len(x), len(y), -1).astype(np.int64)
    qx = qx.astype(np.int64); qy = qy.astype(np.int64)
    xi = np.clip(np.searchsorted(x, qx, side="right") - 1, 0, len(x) - 2)
    yi = np.clip(np.searchsorted(y, qy, side="right") - 1, 0, len(y) - 2)
    dx = (x[xi + 1] - x[xi])[:, None]; dy = (y[yi + 1] - y[yi])[:, None]
    z11, z12, z21, z22 = g3[xi, yi], g3[xi, yi + 1], g3[xi + 1, yi], g3[xi + 1, yi + 1]
    ddx = (qx - x[xi])[:, None]
    z1 = _trunc_div(z21 - z11, dx) * ddx + z11
    z2 = _trunc_div(z22 - z12, dx) * ddx + z12
    return _trunc_div(z2 - z1, dy) * (qy - y[yi])[:, None] + z1


def test_reference_integer_vectors_on_the_device(pkg):
    v = _vec()
    for case in v["interp2d_scalar"]:
        for dt in (np.int32, np.int64):
            x = np.array(case["x"], dtype=dt) if case["x"] is not None else None
            interp = _bil(pkg, x, None, np.array(case["data"], dtype=dt))
            q = np.array(case["queries"], dtype=dt)
            res = interp.interp_array(q[:, 0], q[:, 1])
            assert res.dtype == dt and res.tolist() == case["expect"], case["src"]
    oob = v["interp2d_out_of_bounds"]
    interp = _bil(pkg, None, None, np.array(oob["data"], dtype=np.int32))
    for (qx, qy), axis in zip(oob["queries"], oob["axis"]):
        with pytest.raises(pkg.InterpolateError.OutOfBounds, match=rf"^{axis} = {qx if axis == 'x' else qy} is not in range$"):
            interp.interp_array(np.array([qx], np.int32), np.array([qy], np.int32))
    for case in v["derived_linear_i32"]:
        for dt in (np.int32, np.int64):
            interp = _lin(pkg, np.array(case["x"], dtype=dt), np.array(case["data"], dtype=dt))
            res = interp.interp_array(np.array(case["queries"], dtype=dt))
            assert res.dtype == dt and res.tolist() == case["expect"], case["why"]
    for case in v["derived_integer_overflow"]:
        dt = np.dtype(case["dtype"])
        interp = _lin(pkg, np.array(case["x"], dtype=dt), np.array(case["data"], dtype=dt),
                      extrapolate=case.get("extrapolate", False))
        if dt.kind == "u":    # unsigned stays on the generic path
            assert type(interp.strategy).__name__ == "HostLinear"
        q = np.array([case["query"]], dtype=dt)
        if "panic" in case:
            with pytest.raises(pkg.Panic, match=f"^{case['panic']}$"):
                interp.interp_array(q)
        else:
            assert interp.interp_array(q).tolist() == [case["expect"]]


@pytest.mark.parametrize("dt", [np.int32, np.int64])
@pytest.mark.parametrize("n", [2, 3, 17, 100, 4096])
def test_linear_randomized_sweep(pkg, dt, n):
    import torch
    rng = np.random.default_rng(n * 7 + (dt == np.int64))
    for lanes in (1, 2, 3, 5, 8, 16, 64, 4096):
        if n * lanes > 2_000_000:
            continue
        x = np.cumsum(rng.integers(1, 50, n)).astype(dt) - 300
        data = rng.integers(-10000, 10000, (n, lanes)).astype(dt)
        for extrap in (False, True):
            interp = _lin(pkg, x, data if lanes > 1 else data[:, 0], extrapolate=extrap)
            lo, hi = (int(x[0]), int(x[-1])) if not extrap else (int(x[0]) - 100, int(x[-1]) + 100)
            q = rng.integers(lo, hi + 1, (7, 5)).astype(dt)
            want = _lin_ref(x, data, q.reshape(-1)).reshape((7, 5) + ((lanes,) if lanes > 1 else ()))
            got = interp.interp_array(q)
            assert got.dtype == dt and np.array_equal(got, want), (n, lanes, extrap)
            gd = interp.interp_array(torch.as_tensor(q, device="cuda:0"))
            assert gd.dtype == torch.from_numpy(np.zeros(1, dt)).dtype and np.array_equal(gd.cpu().numpy(), want)
            if lanes > 1:   # strided output view
                big = np.zeros((7, 5, lanes * 2), dtype=dt)
                interp.interp_array_into(q, big[:, :, ::2])
                assert np.array_equal(big[:, :, ::2], want)
            if dt == np.int64:   # sampled rows against the generic per-query path
                ref = _lin(pkg, x, data if lanes > 1 else data[:, 0], extrapolate=extrap, device=False)
                assert np.array_equal(ref.interp_array(q[0]), got[0])


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_bilinear_randomized_sweep(pkg, dt):
    rng = np.random.default_rng(11 + (dt == np.int64))
    for nx, ny, lanes in ((2, 2, 1), (3, 17, 2), (17, 5, 3), (100, 100, 5), (33, 40, 64), (5, 4, 100)):
        x = np.cumsum(rng.integers(1, 20, nx)).astype(dt)
        y = np.cumsum(rng.integers(1, 20, ny)).astype(dt) - 100
        g = rng.integers(-3000, 3000, (nx, ny, lanes)).astype(dt)
        for extrap in (False, True):
            interp = _bil(pkg, x, y, g if lanes > 1 else g[:, :, 0], extrapolate=extrap)
            pad = 30 if extrap else 0
            qx = rng.integers(int(x[0]) - pad, int(x[-1]) + pad + 1, (9, 4)).astype(dt)
            qy = rng.integers(int(y[0]) - pad, int(y[-1]) + pad + 1, (9, 4)).astype(dt)
            want = _bil_ref(x, y, g, qx.reshape(-1), qy.reshape(-1)).reshape((9, 4) + ((lanes,) if lanes > 1 else ()))
            got = interp.interp_array(qx, qy)
            assert got.dtype == dt and np.array_equal(got, want), (nx, ny, lanes, extrap)
            if dt == np.int64:
                ref = _bil(pkg, x, y, g if lanes > 1 else g[:, :, 0], extrapolate=extrap, device=False)
                assert np.array_equal(ref.interp_array(qx[0], qy[0]), got[0])


def _first_error_cases(dt):
    info = INFO[dt]
    mx, mn = int(info.max), int(info.min)
    x = np.array([0, 1, 2], dt)
    # interval 0 is harmless at x = 0; lane 1 of interval 1 overflows: subtract (dy), multiply (m * d), add (m * d + y1)
    return [
        ("subtract", x, np.array([[0, 0], [1, mn], [2, mx]], dt), False, 2),
        ("multiply", x, np.array([[0, 0], [1, 0], [2, mx // 2 + 10]], dt), True, 5),
        ("add", x, np.array([[0, 0], [1, mx - 1], [2, mx]], dt), True, 4),
    ]


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_overflow_panics_like_the_serial_loop(pkg, dt):
    for op, x, data, extrap, bad_q in _first_error_cases(dt):
        dev = _lin(pkg, x, data, extrapolate=extrap)
        host = _lin(pkg, x, data, extrapolate=extrap, device=False)
        q = np.array([0, 0, bad_q, 0, bad_q], dtype=dt)
        with pytest.raises(pkg.Panic) as eh:
            host.interp_array_into(q, np.zeros((5, 2), dt))
        assert str(eh.value) == f"attempt to {op} with overflow", (op, str(eh.value))
        for flags in ({}, {"rows_after_error_unspecified": True}):
            buf = np.full((5, 2), 77, dtype=dt)
            with pytest.raises(pkg.Panic) as ed:
                dev.interp_array_into(q, buf, **flags)
            assert str(ed.value) == str(eh.value) and ed.value.index == 2
            assert np.array_equal(buf[:2], data[[0, 0]]), op
            if not flags:
                assert (buf[2:] == 77).all()
        with pytest.raises(pkg.Panic, match=f"^attempt to {op} with overflow$"):
            dev.interp_array(q)
    # Bilinear: the y step overflows (z2 - z1)
    info = INFO[dt]
    g = np.array([[0, int(info.max)], [0, int(info.min) + 1]], dtype=dt)
    dev = _bil(pkg, None, None, g)
    host = _bil(pkg, None, None, g, device=False)
    qx = np.array([0, 1], dt); qy = np.array([0, 1], dt)
    with pytest.raises(pkg.Panic) as eh:
        host.interp_array(qx, qy)
    with pytest.raises(pkg.Panic) as ed:
        dev.interp_array(qx, qy)
    assert str(ed.value) == str(eh.value)


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_first_error_precedence(pkg, dt):
    info = INFO[dt]
    x = np.array([0, 1, 2], dt)
    data = np.array([[0, 0], [1, int(info.max)], [2, 0]], dt)    # interval 0 lane 1: m = MAX, x - x1 = 1 fits
    interp = _lin(pkg, x, data)
    # no query overflows here (q = 1 and q = 2 evaluate): a plain out-of-bounds error at index 1
    q = np.array([0, 5, 1, 2], dt)
    with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^x = 5 is not in range$") as e:
        interp.interp_array(q)
    assert e.value.index == 1
    big = np.array([[0, int(info.min)], [1, int(info.max)], [2, 0]], dt)  # interval 0: dy overflows
    interp = _lin(pkg, x, big)
    buf = np.full((4, 2), 9, dt)
    with pytest.raises(pkg.Panic, match="^attempt to subtract with overflow$") as e:
        interp.interp_array_into(np.array([2, 0, 7, 1], dt), buf)
    assert e.value.index == 1 and (buf[1:] == 9).all()
    # out of bounds at a lower index than a later overflow: the out-of-bounds query wins, in both output modes
    for flags in ({}, {"rows_after_error_unspecified": True}):
        buf = np.full((4, 2), 9, dt)
        with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^x = -3 is not in range$") as e:
            interp.interp_array_into(np.array([2, -3, 0, 7], dt), buf, **flags)
        assert e.value.index == 1 and np.array_equal(buf[0], [2, 0])
        if not flags:
            assert (buf[1:] == 9).all()
    gb = np.array([[0, 0], [1, int(info.max)], [2, int(info.min)]], dt).reshape(3, 1, 2).repeat(2, axis=1)
    b2 = _bil(pkg, None, None, gb)          # x interval 1 (xi = 1): dz = MIN - MAX overflows
    with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^y = 5 is not in range$") as e:
        b2.interp_array(np.array([0, 0, 2], dt), np.array([0, 5, 0], dt))
    assert e.value.index == 1
    with pytest.raises(pkg.Panic, match="^attempt to subtract with overflow$") as e:
        b2.interp_array(np.array([0, 2, 0], dt), np.array([0, 0, 5], dt))
    assert e.value.index == 1
    # 2-D: x before y within a query, the lowest failing query across kinds
    g = np.arange(12, dtype=dt).reshape(3, 4)
    b = _bil(pkg, None, None, g)
    with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^x = -1 is not in range$") as e:
        b.interp_array(np.array([0, -1, 1], dt), np.array([0, 9, -3], dt))
    assert e.value.index == 1 and e.value.axis == 0
    with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^y = 4 is not in range$") as e:
        b.interp_array(np.array([0, 1], dt), np.array([0, 4], dt))
    assert e.value.index == 1


def test_ring_sharded_async_locator(pkg):
    import torch
    rng = np.random.default_rng(5)
    for dt in (np.int32, np.int64):
        x = np.cumsum(rng.integers(1, 9, 50)).astype(dt)
        data = rng.integers(-500, 500, (50, 6)).astype(dt)
        interp = _lin(pkg, x, data)
        q = rng.integers(int(x[0]), int(x[-1]) + 1, 1000).astype(dt)
        want = _lin_ref(x, data, q)
        qd = torch.as_tensor(q, device="cuda:0")
        got = []
        interp.strategy.interp_array_ring(qd, 128, lambda c, v: got.append(v.clone()),
                                          slots=[torch.empty((128, 6), dtype=qd.dtype, device="cuda:0") for _ in range(2)])
        torch.cuda.synchronize()
        assert np.array_equal(torch.cat(got).cpu().numpy(), want)
        out = torch.empty((1000, 6), dtype=qd.dtype, device="cuda:0")
        interp.strategy.interp_array_into(interp, qd, out, async_launch=True)
        interp.strategy.finish()
        assert np.array_equal(out.cpu().numpy(), want)
        # sharded, one device
        lib = pkg._capi.lib()
        import ctypes as C
        outh = np.zeros((1000, 6), dt)
        io = (pkg._capi.ShardIO * 1)()
        io[0].out = outh.ctypes.data
        hs = (C.c_void_p * 1)(interp.strategy._h)
        info = pkg._capi.OobInfo()
        st = lib.ndi_interp1d_eval_sharded(hs, 1, q.ctypes.data, 1000, io, 6, None, C.byref(info))
        assert st == pkg._capi.OK and np.array_equal(outh, want)
        qbad = q.copy(); qbad[600] = int(x[-1]) + 1
        outh[:] = 3
        st = lib.ndi_interp1d_eval_sharded(hs, 1, qbad.ctypes.data, 1000, io, 6, None, C.byref(info))
        assert st == pkg._capi.OUT_OF_BOUNDS and info.index == 600
        assert np.array_equal(outh[:600], want[:600]) and (outh[600:] == 3).all()
        # locator on integer knots
        idx = np.zeros(1000, np.int64)
        assert lib.ndi_get_lower_index_batch(pkg._capi.I32 if dt == np.int32 else pkg._capi.I64, 0, x.ctypes.data,
                                             50, q.ctypes.data, 1000, idx.ctypes.data, pkg._capi.MEM_HOST) == 0
        from ndarray_interp_amd.generic_host import lower_index
        assert idx.tolist() == [lower_index([int(v) for v in x], int(v), True) for v in q]
        # path rules
        interp.strategy.path = pkg._capi.PATH_BUCKETED
        with pytest.raises(Exception, match="UNSUPPORTED"):
            interp.interp_array(q)


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_out_of_range_queries_are_refused_like_the_generic_path(pkg, dt):
    import torch
    x = np.array([0, 10], dt)
    data = np.array([0, 100], dt)
    dev, host = _lin(pkg, x, data), _lin(pkg, x, data, device=False)
    bads = [np.array([1, 2**63 + 5], np.uint64), np.array([1.0, 2.5]), np.array([1.0, np.nan])]
    if dt == np.int32:
        bads.append(np.array([1, 2**32 + 1], np.int64))
    for q in bads:
        with pytest.raises(TypeError) as eh:
            host.interp_array(q)
        with pytest.raises(TypeError) as ed:
            dev.interp_array(q)
        assert str(ed.value) == str(eh.value), (q, str(ed.value), str(eh.value))
        if q.dtype != np.uint64:
            with pytest.raises(TypeError) as et:
                dev.interp_array(torch.as_tensor(q, device="cuda:0"))
            assert str(et.value) == str(eh.value)
    # in-range values of a wider integer type and integral floats are accepted, as on the generic path
    assert dev.interp_array(np.array([3, 10], np.int64)).tolist() == host.interp_array(np.array([3, 10], np.int64)).tolist()
    assert dev.interp_array(np.array([3.0, 10.0])).tolist() == [30, 100]


def test_error_paths_under_the_forced_wave_mapping():
    """The overflow / first-error tests use 1-2 lanes, i.e. the per-element mapping: run them again with the
    one-query-per-wavefront kernels forced (NDI_INT_MAP=2 is read once per process, hence a child process)."""
    env = dict(os.environ, NDI_INT_MAP="2")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-k", "overflow or precedence or ring_sharded", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


def test_integer_file_under_the_checked_library():
    if os.environ.get("NDI_LIB"):
        pytest.skip("already running under another library")
    subprocess.run(["make", "-C", os.path.join(ROOT, "ndarray-interp_amd", "csrc"), "debug"], check=True,
                   capture_output=True)
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-k", "not checked_library and not forced_wave_mapping", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
