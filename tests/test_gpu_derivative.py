"""GPU: derivative handles (ndi_interp1d_derivative, Interp1D.derivative) on the device, bit for bit.

The build kernel (csrc/derivative_kernels.hpp) follows the header's rule operation by operation, so a derivative handle's
data / a / b tables equal tests/derivative_ref.derive of the SOURCE HANDLE'S OWN tables (read back through
ndi_interp1d_data and coefficients(): that keeps the blocked spline build's few-ulp freedom out of the comparison)
exactly; evaluation is the spline's, so rows equal the CPU oracle's interp1d_cubic fed with those tables exactly.  The
rule itself is checked against scipy in tests/test_derivative_abi.py."""
import os

import numpy as np
import pytest

import derivative_ref
import oracle
from test_gpu_parity import SHAPES_1D, check_equal, knots

pytestmark = pytest.mark.gpu

SOURCES = ["nk", "nat", "cl", "per", "lanes", "pchip", "akima", "hermite"]
SPLINES = ("nk", "nat", "cl", "per", "lanes")
SHAPES = [(3, 1), (3, 5), (100, 5), (257, 130), (1000, 6), (64, 4096), (100_000, 8), (1_000_000, 1), (4096, 4096)]


def strategy(pkg, source, y, extrapolate=False):
    """the strategy builder of a source; `lanes`: a different boundary pair per lane (BoundaryCondition.Individual)"""
    if source in ("pchip", "akima"):
        s = (pkg.Pchip if source == "pchip" else pkg.Akima).new()
    elif source == "hermite":
        yh = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
        s = pkg.CubicHermite.new(np.cos(3.0 * yh).astype(yh.dtype))     # any derivatives: no rule is applied to them
    else:
        s = pkg.CubicSpline.new()
        if source == "lanes":
            L = int(np.prod(y.shape[1:], dtype=np.int64)) if len(y.shape) > 1 else 1
            SB, RB = pkg.SingleBoundary, pkg.RowBoundary
            kinds = [RB.NotAKnot, RB.Natural, RB.Mixed(SB.FirstDeriv(0.5), SB.SecondDeriv(-1.0)), RB.Clamped]
            rows = np.empty((1,) + tuple(y.shape[1:]), dtype=object)
            rows.reshape(-1)[:] = [kinds[l % 4] for l in range(L)]
            s = s.boundary(pkg.BoundaryCondition.Individual(rows))
        else:
            s = s.boundary({"nk": pkg.BoundaryCondition.NotAKnot, "nat": pkg.BoundaryCondition.Natural,
                            "cl": pkg.BoundaryCondition.Clamped, "per": pkg.BoundaryCondition.Periodic}[source])
    return s.extrapolate(extrapolate)


def data(rng, source, n, L, dt, scalar=False):
    """uneven knots, values with sign changes; the periodic source gets equal end rows; Pchip's two-knot case for n = 2"""
    x = np.cumsum(rng.uniform(0.5, 2.0, n)).astype(dt)     # (steps of 0.5 and more stay distinct in f32 at 1e6 knots)
    assert np.all(np.diff(x) > 0)
    y = rng.normal(size=(n, L)).astype(dt)
    if source == "per":
        y[-1] = y[0]
    return x, (y.reshape(n) if scalar and L == 1 else y)


def make(pkg, source, x, y, extrapolate=False):
    return pkg.Interp1D.builder(y).x(x).strategy(strategy(pkg, source, y, extrapolate)).build()


def tables_of(interp):
    """the handle's OWN {y, a, b}, each (n, lanes), on the host"""
    a, b = interp.strategy.coefficients()
    return interp.strategy.data_table(), a, b


def check_derivative(interp, x, nu, what):
    """derivative(nu) of `interp` against the rule applied to interp's own tables; returns (handle, Y, A, B)"""
    y, a, b = tables_of(interp)
    Y, A, B = derivative_ref.derive_nu(x, y, a, b, nu)
    d = interp.derivative(nu)
    gy, ga, gb = tables_of(d)
    check_equal(gy, Y, what + ": data"); check_equal(ga, A, what + ": a"); check_equal(gb, B, what + ": b")
    dd = d.data.cpu().numpy() if hasattr(d.data, "cpu") else d.data
    assert tuple(d.data.shape) == tuple(interp.data.shape) and np.array_equal(dd.reshape(Y.shape), Y), what + ": Interp1D.data"
    assert d.x is interp.x
    return d, Y, A, B


def max_order(source):
    return 2 if source in SPLINES else 1


# ---- tables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n,L", SHAPES)
def test_tables_host_and_device_built(pkg, dt, source, n, L):
    import torch
    rng = np.random.default_rng(n + 7 * L)
    shapes = [(n, L)] + ([(2, 1)] if (n, L) == (3, 1) and source in ("pchip", "hermite") else [])
    for nn, LL in shapes:
        x, y = data(rng, source, nn, LL, dt, scalar=True)
        host = make(pkg, source, x, y)
        dev = make(pkg, source, torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0"))
        for interp, where in ((host, "host-built"), (dev, "device-built")):
            for nu in range(1, max_order(source) + 1):
                d, Y, A, B = check_derivative(interp, x, nu, f"{source} {nn} x {LL} {where} nu={nu}")
                assert isinstance(d.strategy, pkg.DerivativeStrategy) and d.strategy.order == nu
                assert (hasattr(d.data, "is_cuda") and d.data.is_cuda) == (where == "device-built")
                if nu == 2:   # equals derivative().derivative(), and the coefficient tables vanish
                    d11 = interp.derivative().derivative()
                    assert d11.strategy.order == 2
                    for got, ref in zip(tables_of(d11), (Y, A, B)):
                        check_equal(got, ref, f"{source} {nn} x {LL} {where} derivative().derivative()")
                    assert np.all(A == 0) and np.all(B == 0)
        # the source is untouched and still evaluates
        q = x[:2].copy()
        check_equal(host.interp_array(q).reshape(-1), np.asarray(y).reshape(nn, -1)[:2].reshape(-1), "source after derivative")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("L", [1, 3, 7, 8, 64])
def test_lane_mappings(pkg, dt, L):
    """L = 1 (consecutive threads on consecutive knots), odd L (one lane per thread), L a multiple of the vector width
    (16-byte vectors) -- and that last one built from a device data pointer that is not 16-byte aligned."""
    import torch
    rng = np.random.default_rng(L)
    n = 301
    for source in ("nk", "pchip"):
        x, y = data(rng, source, n, L, dt)
        check_derivative(make(pkg, source, x, y), x, 1, f"{source} L={L}")
        yd = torch.empty(n * L + 1, dtype=torch.as_tensor(y).dtype, device="cuda:0")[1:].view(n, L)
        yd.copy_(torch.as_tensor(y))
        assert yd.data_ptr() % 16 != 0
        off = make(pkg, source, torch.as_tensor(x, device="cuda:0"), yd)
        d, Y, A, B = check_derivative(off, x, 1, f"{source} L={L} offset device data")
        # ... and Y goes back into a caller's unaligned device buffer through ndi_interp1d_data
        buf = torch.empty(n * L + 1, dtype=yd.dtype, device="cuda:0")[1:]
        assert pkg._capi.lib().ndi_interp1d_data(d.strategy._h, buf.data_ptr(), pkg._capi.MEM_DEVICE) == pkg._capi.OK
        check_equal(buf.cpu().numpy().reshape(n, L), Y, "ndi_interp1d_data into an offset device buffer")


# ---- evaluation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("source,nu", [("nk", 1), ("nk", 2), ("pchip", 1), ("akima", 1)])
@pytest.mark.parametrize("n,L,Q", SHAPES_1D)
def test_eval_bit_exact_every_path(pkg, dt, source, nu, n, L, Q):
    rng = np.random.default_rng(n * 7919 + L)
    x = knots("rand", n, rng, dt)
    y = rng.uniform(-1.0, 1.0, (n, L)).astype(dt)
    q = rng.uniform(x[0], x[-1], Q).astype(dt)
    q[:3] = [x[0], x[-1], x[n // 2]]
    d, Y, A, B = check_derivative(make(pkg, source, x, y), x, nu, f"{source} nu={nu} n={n} L={L}")
    _, _, ref = oracle.interp1d_cubic(x, Y, A, B, q)
    for path in (pkg.PATH_GATHER, pkg.PATH_BUCKETED, pkg.PATH_AUTO):
        d.strategy.path = path
        check_equal(d.interp_array(q), ref, f"{source} nu={nu} n={n} L={L} path={path}")
    # at the knots: Y itself (an interior knot carries the value of the interval to its right)
    d.strategy.path = pkg.PATH_AUTO
    check_equal(d.interp_array(x), Y, f"{source} nu={nu} n={n} L={L} at the knots")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("source,nu,n,L", [("nk", 1, 100, 1), ("nk", 2, 100, 1), ("per", 1, 100, 1), ("per", 2, 100, 5),
                                           ("pchip", 1, 100, 5), ("akima", 1, 100, 1), ("pchip", 1, 2, 1), ("hermite", 1, 2, 7),
                                           ("nat", 2, 3, 2), ("akima", 1, 3, 2)])
def test_eval_short_rows_device_batches(pkg, dt, source, nu, n, L):
    """Scalar / short-row data with 1e6 device queries (random, and sorted: the interval-sorted plan): the forms that keep
    the tables in LDS; with extrapolation, and with the periodic wrap for the periodic spline."""
    import torch
    rng = np.random.default_rng(n + 31 * L)
    x, y = data(rng, source, n, L, dt, scalar=True)
    for extrapolate in (False, True):
        d, Y, A, B = check_derivative(make(pkg, source, x, y, extrapolate), x, nu, f"{source} nu={nu} n={n} L={L}")
        span = x[-1] - x[0]
        lo, hi = (x[0], x[-1]) if not extrapolate else \
            ((x[0] - 2.5 * span, x[-1] + 2.5 * span) if source == "per" else (x[0] - 0.5 * (x[1] - x[0]), x[-1] + 0.5 * (x[-1] - x[-2])))
        mode = oracle.EXTRAPOLATE_NO if not extrapolate else (oracle.EXTRAPOLATE_PERIODIC if source == "per" else oracle.EXTRAPOLATE_YES)
        q = rng.uniform(lo, hi, 1_000_000).astype(dt)
        for qq, order in ((q, "random"), (np.sort(q), "sorted")):
            _, _, ref = oracle.interp1d_cubic(x, Y, A, B, qq, mode)
            qd = torch.as_tensor(qq, device="cuda:0")
            for path in (pkg.PATH_AUTO, pkg.PATH_GATHER):
                d.strategy.path = path
                got = d.interp_array(qd).cpu().numpy()
                check_equal(got.reshape(ref.shape), ref, f"{source} nu={nu} n={n} L={L} extrapolate={extrapolate} {order} path={path}")
            check_equal(d.interp_array(qq).reshape(ref.shape), ref, f"{source} nu={nu} n={n} L={L} host batch {order}")


# ---- semantics carried over ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,nu", [("nk", 1), ("nk", 2), ("pchip", 1)])
def test_first_error_ring_clone_sharded(pkg, source, nu):
    import torch
    rng = np.random.default_rng(5)
    n, L, Q = 20, 1024, 4099
    x, y = data(rng, source, n, L, np.float64)
    src = make(pkg, source, x, y)
    d, Y, A, B = check_derivative(src, x, nu, f"{source} nu={nu}")
    q = rng.uniform(x[0], x[-1], Q)
    _, _, ref = oracle.interp1d_cubic(x, Y, A, B, q)
    # OutOfBounds: the reference's message and first-error semantics -- rows before the failure written, later ones untouched
    qbad = q.copy(); qbad[317] = x[0] - 0.1; qbad[500] = x[-1] + 99.0
    for path in (pkg.PATH_GATHER, pkg.PATH_BUCKETED):
        d.strategy.path = path
        buf = np.full((Q, L), -7.0)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as ei:
            d.interp_array_into(qbad, buf)
        assert ei.value.index == 317 and str(ei.value).startswith("x = ") and str(ei.value).endswith(" is not in range")
        assert np.array_equal(buf[:317], ref[:317]) and np.all(buf[317:] == -7.0)
    d.strategy.path = pkg.PATH_AUTO
    # single queries through the mirror
    check_equal(d.interp(q[5]), ref[5], "interp")
    assert d.index_point(3)[0] == x[3] and np.array_equal(d.index_point(3)[1], Y[3])
    # ring: the whole batch, and the cut at the first error
    qd = torch.as_tensor(q, device="cuda:0")
    got = np.zeros_like(ref)
    ring = pkg.striped_ring(1024, L, 2, np.float64, 0)
    seen = []

    def consumer(c, rows):
        got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
        seen.append((c.q_begin, c.q_count))
    d.interp_array_ring(qd, 1024, consumer, slots=ring)
    check_equal(got, ref, "ring")
    seen.clear(); got[...] = -3.0
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as ei:
        d.interp_array_ring(torch.as_tensor(qbad, device="cuda:0"), 128, consumer, slots=pkg.striped_ring(128, L, 2, np.float64, 0))
    assert ei.value.index == 317 and sum(c for _, c in seen) == 317 and seen[-1] == (256, 61)
    assert np.array_equal(got[:317], ref[:317]) and np.all(got[317:] == -3.0)
    # clone on the same device: tables copied, nothing rebuilt, order carried
    rep = d.replicate([0])[0]
    assert isinstance(rep.strategy, pkg.DerivativeStrategy) and rep.strategy.order == nu
    for g, r in zip(tables_of(rep), (Y, A, B)):
        check_equal(g, r, "clone tables")
    check_equal(rep.interp_array(q), ref, "clone rows")
    if nu == 1 and source == "nk":     # the origin and order travel with the replica: the second derivative follows from it
        check_equal(tables_of(rep.derivative())[0], derivative_ref.derive(x, Y, A, B)[0], "derivative of a clone")
        with pytest.raises(ValueError, match="third derivative"):
            rep.derivative(2)
    # one sharded call over derivative replicas
    got = np.full_like(ref, -1.0)
    pkg.sharding.interp_array_sharded([d, rep], q, out=got)
    check_equal(got, ref, "sharded")
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as ei:
        pkg.sharding.interp_array_sharded([d, rep], qbad, out=got)
    assert ei.value.index == 317
    # a function and its derivative are not one interpolator; nor are two orders
    with pytest.raises(pkg.DeviceError, match="same knots, strategy"):
        pkg.sharding.interp_array_sharded([src, d], q, out=got)
    if nu == 2:
        with pytest.raises(pkg.DeviceError, match="same knots, strategy"):
            pkg.sharding.interp_array_sharded([src.derivative(1), d], q, out=got)
    d.strategy.trim()
    check_equal(d.interp_array(q), ref, "after trim")
    # library-owned output (ndi_output_alloc) as the target
    own = pkg.output_zeros((Q, L), np.float64, 0)
    d.interp_array_into(qd, own)
    check_equal(own.cpu().numpy(), ref, "library-owned output")


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_with_a_real_handle(pkg):
    import torch
    cap, lib = pkg._capi, pkg._capi.lib()
    import ctypes as C
    x = np.arange(6.0); y = np.sin(x)
    out = C.c_void_p(99)
    lin = pkg.Interp1D.builder(y).x(x).build()
    assert lib.ndi_interp1d_derivative(lin.strategy._h, 1, C.byref(out)) == cap.BAD_ARG and out.value is None
    assert cap.last_error().startswith("Linear has no derivative handle: its slope jumps at the knots")
    with pytest.raises(ValueError, match="Linear has no derivative handle"):
        lin.derivative()
    xi = torch.arange(6, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="an integer handle is a Linear interpolator"):
        pkg.Interp1D.builder(xi * 3).x(xi).build().derivative()
    xh = torch.arange(6, dtype=torch.float16, device="cuda:0")
    with pytest.raises(ValueError, match="an f16 / bf16 handle is a Linear interpolator"):
        pkg.Interp1D.builder(xh * 0.5).x(xh).build().derivative()
    for source, name in (("pchip", "Pchip"), ("akima", "Akima"), ("hermite", "CubicHermite")):
        it = make(pkg, source, x, y)
        assert lib.ndi_interp1d_derivative(it.strategy._h, 2, C.byref(out)) == cap.BAD_ARG
        assert cap.last_error().startswith(f"{name}: the second derivative of a C1 interpolant jumps at the knots")
        with pytest.raises(ValueError, match=f"{name}: the second derivative of a C1 interpolant jumps at the knots"):
            it.derivative(2)
        with pytest.raises(ValueError, match=f"{name}: the second derivative .* of its first derivative"):
            it.derivative().derivative()
    sp = make(pkg, "nat", x, y)
    d2 = sp.derivative(2)
    for bad in (d2.derivative, lambda: sp.derivative().derivative(2)):
        with pytest.raises(ValueError, match="CubicSpline: the third derivative of a cubic spline jumps at the knots"):
            bad()
    for nu, text in ((0, "nu = 0: the derivative order must be 1 or 2"), (3, "nu = 3: the third and higher derivatives")):
        with pytest.raises(ValueError, match=text):
            sp.derivative(nu)
    with pytest.raises(TypeError):
        sp.derivative(1.5)
    assert lib.ndi_interp1d_derivative(sp.strategy._h, 1, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"
    # ndi_interp1d_data serves every 1-D handle: the data as given
    assert np.array_equal(lin.strategy.data_table().reshape(-1), y)
    it = pkg.Interp1D.builder(xi * 3).x(xi).build()
    assert np.array_equal(it.strategy.data_table().reshape(-1), np.arange(6, dtype=np.int32) * 3)
    ih = pkg.Interp1D.builder(xh * 0.5).x(xh).build()
    assert np.array_equal(ih.strategy.data_table().reshape(-1), (np.arange(6) * 0.5).astype(np.float16))


# ---- AUTO ---------------------------------------------------------------------------------------------------------------
def _plans(pkg, capfd, interp, qd):
    os.environ["NDI_TRACE_PLAN"] = "1"
    try:
        capfd.readouterr()
        pkg.profile_enable(True); pkg.profile_read(reset=True)
        interp.interp_array(qd)
        prof = pkg.profile_read(reset=True)
        return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[ndi plan]")], prof
    finally:
        pkg.profile_enable(False)
        os.environ.pop("NDI_TRACE_PLAN", None)


def test_auto_plans(pkg, capfd):
    import torch
    rng = np.random.default_rng(11)
    # 1024 knots x 8 lanes of f64, 9.4e6 device queries (a shape tests/test_gpu_short_rows.py pins): the source kept k and
    # AUTO gives it the {y, k} LDS form ({y, a, b} does not fit beside as many waves); its derivative has no k and takes a
    # form that reads a / b
    x = knots("rand", 1024, rng, np.float64)
    y = rng.normal(size=(1024, 8))
    src = make(pkg, "nk", torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0"))
    qd = torch.as_tensor(rng.uniform(x[0], x[-1], 600_000_000 // 64), device="cuda:0")
    ps, _ = _plans(pkg, capfd, src, qd)
    assert ps and "tables=lds{y,k}" in ps[0], ps
    for nu in (1, 2):
        pd, _ = _plans(pkg, capfd, src.derivative(nu), qd)
        assert pd and "lds{y,k}" not in pd[0] and ("tables=lds{y,a,b}" in pd[0] or "tables=memory" in pd[0] or "sorted" in pd[0]), pd
    # 4096 x 4096: the same plan as the source
    x, y = data(rng, "nk", 4096, 4096, np.float64)
    src = make(pkg, "nk", x, y)
    qd = torch.as_tensor(rng.uniform(x[0], x[-1], 20_000), device="cuda:0")
    ps, fs = _plans(pkg, capfd, src, qd)
    pd, fd = _plans(pkg, capfd, src.derivative(), qd)
    assert ps == pd, (ps, pd)
    for key in ("last_path", "eval_launches", "locate_launches", "group_launches"):
        assert fs[key] == fd[key], (key, fs, fd)


# ---- the bounds-checked build -------------------------------------------------------------------------------------------
def test_checked_build_runs_the_new_kernel_clean(pkg):
    """One pass of the table test under the bounds-checked build of the library (make debug), in a child process: a
    violation would turn the call into NDI_HIP_ERROR."""
    import subprocess
    import sys
    from conftest import ROOT
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import derivative_ref\n"
        "pkg = load_product_package(); rng = np.random.default_rng(1)\n"
        "for n, L in ((2, 3), (3, 1), (3, 5), (100, 5), (257, 130), (1000, 6), (64, 4096), (100000, 8)):\n"
        "    x = np.cumsum(rng.uniform(0.1, 2.0, n)); y = rng.normal(size=(n, L)); q = rng.uniform(x[0], x[-1], 5000)\n"
        "    for s, top in ((pkg.CubicSpline.new(), 2), (pkg.Pchip.new(), 1), (pkg.Akima.new(), 1), (pkg.CubicHermite.new(y), 1)):\n"
        "        if n < 3 and not isinstance(s, (pkg.Pchip, pkg.CubicHermite)): continue\n"
        "        it = pkg.Interp1D.builder(y).x(x).strategy(s).build()\n"
        "        a, b = it.strategy.coefficients(); t = (it.strategy.data_table(), a, b)\n"
        "        for nu in range(1, top + 1):\n"
        "            d = it.derivative(nu); ga, gb = d.strategy.coefficients()\n"
        "            Y, A, B = derivative_ref.derive_nu(x, *t, nu)\n"
        "            assert np.array_equal(d.data, Y) and np.array_equal(ga, A) and np.array_equal(gb, B), (type(s).__name__, n, L, nu)\n"
        "            d.interp_array(q)\n"
        "print('checked OK')\n" % (os.path.join(ROOT, "tests"), ROOT))
    env = dict(os.environ, NDI_LIB=lib)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout + r.stderr
