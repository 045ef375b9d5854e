"""GPU: antiderivative handles (ndi_interp1d_antiderivative, ndi_interp1d_integrate).  The prefix table, evaluated rows and
definite integrals are compared BIT FOR BIT with the numpy restatement of the header's rule (tests/antiderivative_ref.py)
applied to the SOURCE HANDLE'S OWN tables, read back through data_table() / coefficients(); intervals come from the CPU
oracle's get_lower_index.  Shapes: the smallest at which each build mapping can go wrong (one block, a block edge with an
odd lane count, the vector path, 3907 blocks of scalar data, many lanes with few blocks).  The three largest shapes run two
sources each (one cubic, Linear: the kernels' two template variants); 1e6 x 1 and 4096 x 4096 host-built only."""
import ctypes as C
import os

import numpy as np
import pytest

import antiderivative_ref as ar
import hostile_inputs
import oracle
from test_gpu_derivative import data, make, strategy
from test_gpu_parity import check_equal

pytestmark = pytest.mark.gpu

SOURCES = ["nk", "nat", "per", "lanes", "pchip", "akima", "hermite", "linear", "dnat"]
SHAPES = [(2, 1), (3, 5), (100, 5), (257, 130), (258, 3), (1000, 6), (64, 4096), (100_000, 8), (1_000_000, 1), (4096, 4096)]
BIG = {(100_000, 8): ("nat", "linear"), (1_000_000, 1): ("pchip", "linear"), (4096, 4096): ("akima", "linear")}


def build(pkg, source, x, y, extrapolate=False):
    """the source interpolator: a strategy of test_gpu_derivative's, Linear, or derivative(1) of a natural spline"""
    if source == "linear":
        return pkg.Interp1D.builder(y).x(x).strategy(pkg.Linear.new().extrapolate(extrapolate)).build()
    if source == "dnat":
        return make(pkg, "nat", x, y, extrapolate).derivative(1)
    return make(pkg, source, x, y, extrapolate)


def tables_of(interp):
    """the handle's OWN {y, a, b}, each (n, lanes), on the host; Linear: a = b = None"""
    y = interp.strategy.data_table()
    if type(interp.strategy).__name__ == "Linear":
        return y, None, None
    a, b = interp.strategy.coefficients()
    return y, a, b


def host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def queries(rng, x, count, extrapolate):
    """every knot (or `count` of them), both ends, the neighbours of knots, random points; outside points with extrapolate"""
    dt = x.dtype
    kn = x if len(x) <= count else np.concatenate([x[:2], x[-2:], rng.choice(x, count)])
    near = np.concatenate([np.nextafter(kn[1:], dt.type(-np.inf)), np.nextafter(kn[:-1], dt.type(np.inf))])
    q = np.concatenate([kn, near, rng.uniform(x[0], x[-1], count).astype(dt)])
    q = q[(q >= x[0]) & (q <= x[-1])]
    if extrapolate:
        span = x[-1] - x[0]
        q = np.concatenate([q, (x[0] - rng.uniform(0, 0.3, 8) * span).astype(dt), (x[-1] + rng.uniform(0, 0.3, 8) * span).astype(dt)])
    return np.ascontiguousarray(rng.permutation(q).astype(dt))


def reference(x, t, P, q):
    return ar.evaluate(x, *t, P, oracle.get_lower_index(x, q), q)


def sources_for(n, L):
    if (n, L) in BIG:
        return BIG[(n, L)]
    if n == 2:
        return ("pchip", "linear")
    return SOURCES


# ---- tables and rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n,L", SHAPES)
def test_tables_and_rows_bit_for_bit(pkg, dt, n, L):
    import torch
    rng = np.random.default_rng([n, L])
    nq = 64 if n * L > 4_000_000 else 1000
    for source in sources_for(n, L):
        x, y = data(rng, "per" if source == "per" else "nat", n, L, dt)
        for where in (("host", "device") if n * L <= 1_000_000 else ("host",)):    # (1e5 x 8: device-built, 391 blocks)
            xx, yy = (x, y) if where == "host" else (torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0"))
            for extrapolate in ((False, True) if source != "per" and n * L <= 1_000_000 else (False,)):
                what = f"{source} {n} x {L} {np.dtype(dt).name} {where} extrapolate={extrapolate}"
                src = build(pkg, source, xx, yy, extrapolate)
                t = tables_of(src)
                P = ar.prefix(x, *t)
                F = src.antiderivative()
                assert isinstance(F.strategy, pkg.AntiderivativeStrategy) and F.x is src.x
                assert tuple(F.data.shape) == tuple(src.data.shape)
                assert (hasattr(F.data, "is_cuda") and F.data.is_cuda) == (where == "device")
                got = F.strategy.data_table()
                check_equal(got, P, what + ": prefix table")
                hostile_inputs.check_bits(got, P, what + ": prefix table, signs of zero")
                assert np.array_equal(host(F.data).reshape(P.shape), P)
                q = queries(rng, x, nq, extrapolate)
                ref = reference(x, t, P, q)
                check_equal(F.interp_array(q).reshape(ref.shape), ref, what + ": host rows")
                qd = torch.as_tensor(q, device="cuda:0")
                check_equal(F.interp_array(qd).cpu().numpy().reshape(ref.shape), ref, what + ": device rows")
                # the source is untouched and still evaluates
                check_equal(src.strategy.data_table(), t[0], what + ": source data after antiderivative()")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("source,n,L", [("nat", 300, 7), ("linear", 300, 7), ("pchip", 40, 1024), ("linear", 40, 1024),
                                         ("akima", 600, 4)])
def test_output_forms_async_and_clone(pkg, dt, source, n, L):
    import torch
    rng = np.random.default_rng([n, L, 1])
    x, y = data(rng, source, n, L, dt)
    src = build(pkg, source, x, y, True)
    t = tables_of(src)
    P = ar.prefix(x, *t)
    F = src.antiderivative()
    q = queries(rng, x, 500, True)
    ref = reference(x, t, P, q)
    qd = torch.as_tensor(q, device="cuda:0")
    tdt = torch.float64 if dt == np.float64 else torch.float32
    # a strided view out[:, :lanes] of a wider device buffer: the pad columns stay untouched
    wide = torch.full((len(q), L + 3), 7.0, dtype=tdt, device="cuda:0")
    F.strategy.interp_array_into(F, qd, wide[:, :L])
    check_equal(wide[:, :L].cpu().numpy(), ref, "strided device rows")
    assert bool((wide[:, L:] == 7.0).all())
    # out[1:] (rows that start off a 16-byte boundary when the lane count is odd)
    off = torch.full((len(q) + 1, L), 7.0, dtype=tdt, device="cuda:0")
    F.strategy.interp_array_into(F, qd, off[1:])
    check_equal(off[1:].cpu().numpy(), ref, "out[1:]")
    assert bool((off[0] == 7.0).all())
    # host queries into a strided host buffer
    hw = np.full((len(q), L + 2), 7.0, dtype=dt)
    F.strategy.interp_array_into(F, q, hw[:, :L])
    check_equal(hw[:, :L], ref, "strided host rows")
    assert np.all(hw[:, L:] == 7.0)
    # async_launch + finish
    out = torch.empty((len(q), L), dtype=tdt, device="cuda:0")
    F.strategy.interp_array_into(F, qd, out, async_launch=True)
    F.strategy.finish()
    check_equal(out.cpu().numpy(), ref, "async rows")
    # a clone on the same device, then trim
    rep = pkg.Interp1D(F.x, F.data, F.strategy.clone(0))
    check_equal(rep.strategy.data_table(), P, "clone table")
    check_equal(rep.interp_array(q).reshape(ref.shape), ref, "clone rows")
    F.strategy.trim()
    check_equal(F.interp_array(q).reshape(ref.shape), ref, "after trim")
    check_equal(F.interp(q[3]).reshape(-1), ref[3], "interp")


# ---- integrate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("source,n,L", [("nat", 1000, 6), ("linear", 1000, 6), ("pchip", 3000, 1), ("akima", 40, 1024),
                                         ("linear", 40, 1024)])
def test_integrate_bit_for_bit(pkg, dt, source, n, L):
    import torch
    rng = np.random.default_rng([n, L, 2])
    x, y = data(rng, source, n, L, dt)
    src = build(pkg, source, x, y, True)
    t = tables_of(src)
    P = ar.prefix(x, *t)
    F = src.antiderivative()
    q = queries(rng, x, 400, True)
    lo, hi = q.copy(), rng.permutation(q)                      # pairs across many blocks, either order
    m = min(50, n - 1)
    lo[:m] = rng.uniform(x[:m], x[1:m + 1]).astype(dt)         # the same interval
    hi[:m] = rng.uniform(x[:m], x[1:m + 1]).astype(dt)
    hi[50:80] = lo[50:80]                                      # lo == hi
    assert np.any(lo > hi) and np.any(lo < hi)
    gl = oracle.get_lower_index
    ref = ar.integrate(x, *t, P, gl(x, lo), lo, gl(x, hi), hi)
    assert np.all(ref[50:80] == 0) and not np.any(np.signbit(ref[50:80]))      # F - F = +0
    got = F.integrate(lo, hi)
    check_equal(got.reshape(ref.shape), ref, "host pairs")
    hostile_inputs.check_bits(got.reshape(ref.shape), ref, "host pairs, signs of zero")
    lod, hid = torch.as_tensor(lo, device="cuda:0"), torch.as_tensor(hi, device="cuda:0")
    gd = F.integrate(lod, hid)
    assert gd.is_cuda and tuple(gd.shape) == (len(lo),) + tuple(F.data.shape[1:])
    check_equal(gd.cpu().numpy().reshape(ref.shape), ref, "device pairs")
    check_equal(F.integrate(hi, lo).reshape(ref.shape), ar.integrate(x, *t, P, gl(x, hi), hi, gl(x, lo), lo), "swapped")
    # the source interpolator builds its antiderivative once and gives the same bits
    check_equal(src.integrate(lo, hi).reshape(ref.shape), ref, "Interp1D.integrate on the source")
    kept = src._antiderivative
    src.integrate(lo[:3], hi[:3])
    assert src._antiderivative is kept
    # query rank 2
    check_equal(F.integrate(lo[:12].reshape(3, 4), hi[:12].reshape(3, 4)).reshape(12, -1), ref[:12], "rank 2")
    check_equal(F.integrate([float(v) for v in lo[:5]], [float(v) for v in hi[:5]]).reshape(5, -1), ref[:5], "plain lists")
    with pytest.raises(pkg.Panic, match="incompatible shapes"):
        F.integrate(lo[:3], hi[:4])


# ---- errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,L", [("nat", 5), ("linear", 5), ("pchip", 512)])
def test_first_error_semantics(pkg, source, L):
    import torch
    rng = np.random.default_rng([L, 3])
    n = 300
    x, y = data(rng, source, n, L, np.float64)
    src = build(pkg, source, x, y)
    F = src.antiderivative()
    t = tables_of(src)
    P = ar.prefix(x, *t)
    q = rng.uniform(x[0], x[-1], 700)
    k = int(rng.integers(100, 600))
    bad = q.copy(); bad[k] = x[-1] + 1.0; bad[k + 40] = x[0] - 1.0
    ref = reference(x, t, P, q)
    for dev in (False, True):
        qq = torch.as_tensor(bad, device="cuda:0") if dev else bad
        out = torch.full((700, L), 7.0, dtype=torch.float64, device="cuda:0") if dev else np.full((700, L), 7.0)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            F.interp_array_into(qq, out)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as es:
            src.interp_array_into(qq, torch.empty_like(out) if dev else np.empty_like(out))
        assert e.value.index == es.value.index == k and str(e.value) == str(es.value)
        o = host(out)
        check_equal(o[:k], ref[:k], "rows before the failure")
        assert np.all(o[k:] == 7.0), "rows at / after the failure are untouched"
    # a NaN query: without extrapolation a range failure naming NaN, with it the search's panic -- as the source
    nanq = q.copy(); nanq[k] = np.nan
    for extrapolate in (False, True):
        s2 = build(pkg, source, x, y, extrapolate)
        F2 = s2.antiderivative()
        errs = []
        for it in (F2, s2):
            with pytest.raises((pkg.InterpolateError.OutOfBounds, pkg.Panic)) as e:
                it.interp_array(nanq)
            errs.append((type(e.value), str(e.value), e.value.index))
        assert errs[0] == errs[1] and errs[0][2] == k
    # integrate: lo is tested before hi at the same index; hi alone reports axis 1
    lo, hi = q.copy(), q[::-1].copy()
    out = np.full((700, L), 7.0)
    lo2, hi2 = lo.copy(), hi.copy(); lo2[k] = x[-1] + 2.0; hi2[k] = x[0] - 3.0
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        F.strategy.integrate_into(lo2, hi2, out)
    assert (e.value.index, e.value.axis, e.value.value) == (k, 0, x[-1] + 2.0)
    gl = oracle.get_lower_index
    refI = ar.integrate(x, *t, P, gl(x, lo), lo, gl(x, hi), hi)
    check_equal(out[:k], refI[:k], "integrate: rows before the failure")
    assert np.all(out[k:] == 7.0)
    hi3 = hi.copy(); hi3[k] = x[0] - 3.0; lo3 = lo.copy(); lo3[k + 1] = x[-1] + 2.0
    outd = torch.full((700, L), 7.0, dtype=torch.float64, device="cuda:0")
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        F.strategy.integrate_into(torch.as_tensor(lo3, device="cuda:0"), torch.as_tensor(hi3, device="cuda:0"), outd)
    assert (e.value.index, e.value.axis, e.value.value) == (k, 1, x[0] - 3.0)
    check_equal(outd[:k].cpu().numpy(), refI[:k], "integrate on the device: rows before the failure")
    assert bool((outd[k:] == 7.0).all())


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_with_a_real_handle(pkg):
    import torch
    cap, lib = pkg._capi, pkg._capi.lib()
    x = np.arange(8.0); y = np.sin(x)[:, None] * np.ones((1, 2))
    out = C.c_void_p(99)
    xi = torch.arange(6, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="antiderivative: an integer handle"):
        pkg.Interp1D.builder(xi * 3).x(xi).build().antiderivative()
    xh = torch.arange(6, dtype=torch.float16, device="cuda:0")
    with pytest.raises(ValueError, match="antiderivative: an f16 / bf16 handle"):
        pkg.Interp1D.builder(xh * 0.5).x(xh).build().antiderivative()
    yp = y.copy(); yp[-1] = yp[0]
    per = make(pkg, "per", x, yp, True)       # periodic boundary + extrapolate: the Periodic mode
    assert lib.ndi_interp1d_antiderivative(per.strategy._h, C.byref(out)) == cap.BAD_ARG and out.value is None
    assert cap.last_error().startswith("CubicSpline: the Periodic extrapolation mode has no antiderivative handle")
    with pytest.raises(ValueError, match="CubicSpline: the Periodic extrapolation mode"):
        per.antiderivative()
    sp = make(pkg, "nat", x, y)
    assert lib.ndi_interp1d_antiderivative(sp.strategy._h, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"
    q = np.array([0.5, 1.5]); buf = np.zeros((2, 2))
    assert lib.ndi_interp1d_integrate(sp.strategy._h, q.ctypes.data, q.ctypes.data, 2, buf.ctypes.data, 2, None, None) == cap.BAD_ARG
    assert cap.last_error().startswith("integrate takes an antiderivative handle")
    for source, name in (("nat", "CubicSpline"), ("pchip", "Pchip"), ("akima", "Akima"), ("hermite", "CubicHermite"),
                         ("linear", "Linear"), ("dnat", "CubicSpline")):
        F = build(pkg, source, x, y).antiderivative()
        with pytest.raises(ValueError, match=f"antiderivative: this handle is already the antiderivative of {name}"):
            F.antiderivative()
        with pytest.raises(ValueError, match=f"derivative: the antiderivative of {name} is a piecewise quartic"):
            F.derivative()
        with pytest.raises(ValueError, match=f"coefficients: the antiderivative of {name} is a piecewise quartic"):
            F.strategy.coefficients()
    F = sp.antiderivative()
    s = F.strategy
    # the ring, the bucketed path, the sharded calls: NDI_UNSUPPORTED with a message
    ring = cap.RingDesc(); ring.chunk_queries = 2; ring.n_slots = 2; ring.row_stride = 2
    opts = cap.EvalOpts(); opts.q_memspace = cap.MEM_HOST; opts.out_memspace = cap.MEM_DEVICE
    info = cap.OobInfo()
    assert lib.ndi_interp1d_eval_ring(s._h, q.ctypes.data, 2, C.byref(ring), C.cast(None, cap.RING_CONSUMER), None,
                                      C.byref(opts), C.byref(info)) == cap.UNSUPPORTED
    assert "no ring evaluation" in cap.last_error()
    opts = cap.EvalOpts(); opts.q_memspace = cap.MEM_HOST; opts.out_memspace = cap.MEM_HOST; opts.path = cap.PATH_BUCKETED
    assert lib.ndi_interp1d_eval(s._h, q.ctypes.data, 2, buf.ctypes.data, 2, C.byref(opts), C.byref(info)) == cap.UNSUPPORTED
    assert cap.last_error().startswith("NDI_PATH_BUCKETED: an antiderivative handle")
    assert lib.ndi_interp1d_integrate(s._h, q.ctypes.data, q.ctypes.data, 2, buf.ctypes.data, 2, C.byref(opts), C.byref(info)) == cap.UNSUPPORTED
    rep = s.clone(0)
    with pytest.raises(Exception, match="do not take antiderivative handles"):
        pkg.sharding.interp_array_sharded([pkg.Interp1D(x, F.data, s), pkg.Interp1D(x, F.data, rep)], np.linspace(0.0, 7.0, 64))
    with pytest.raises(Exception, match="must be replicas of one interpolator"):
        pkg.sharding.interp_array_sharded([sp, pkg.Interp1D(x, F.data, rep)], np.linspace(0.0, 7.0, 64))
    assert s.clone(0)._h is not None and lib.ndi_interp1d_scratch_sets(s._h) >= 0


# ---- hostile data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule", ["pchip", "akima", "hermite"])
def test_hostile_inputs_through_the_build(pkg, dt, rule):
    """infinities, NaN, signed zeros, denormals and huge ratios in the data: the table equals the restatement as bit patterns
    (NaN positions included), and no index depends on a data value -- the build and the evaluation complete and the rows of
    finite lanes equal the restatement's."""
    n, L = 300, 6
    x, y, k = hostile_inputs.generate(rule, dt, n, L)
    s = pkg.CubicHermite.new(k) if rule == "hermite" else (pkg.Pchip if rule == "pchip" else pkg.Akima).new()
    src = pkg.Interp1D.builder(y).x(x).strategy(s.extrapolate(True)).build()
    t = (src.strategy.data_table(),) + tuple(src.strategy.coefficients())
    with np.errstate(all="ignore"):
        P = ar.prefix(x, *t)
        F = src.antiderivative()
        hostile_inputs.check_bits(F.strategy.data_table(), P, f"{rule} hostile table")
        q = hostile_inputs.queries(x)
        q = q[np.isfinite(q)]
        ref = reference(x, t, P, q)
        hostile_inputs.check_bits(F.interp_array(q).reshape(ref.shape), ref, f"{rule} hostile rows")
        sL = pkg.Interp1D.builder(y).x(x).strategy(pkg.Linear.new().extrapolate(True)).build()
        PL = ar.prefix_linear(x, sL.strategy.data_table())
        hostile_inputs.check_bits(sL.antiderivative().strategy.data_table(), PL, "linear hostile table")


# ---- the bounds-checked build -------------------------------------------------------------------------------------------
def test_checked_build_runs_the_new_kernels_clean(pkg):
    """One pass of the table and row checks under the bounds-checked build of the library (make debug), in a child process:
    a violation would turn the call into NDI_HIP_ERROR.  The shapes of this file, and those of
    test_gpu_antiderivative_plans.py whose kernels or index forms no shape here reaches."""
    import subprocess
    import sys
    from conftest import ROOT
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import antiderivative_ref as ar, oracle\n"
        "pkg = load_product_package(); rng = np.random.default_rng(1)\n"
        "shapes = [(n, L, 2000) for n, L in ((2, 3), (3, 5), (100, 5), (257, 130), (258, 3), (1000, 6), (64, 4096), (100000, 8), (300000, 1))]\n"
        "# test_gpu_antiderivative_plans.py's plans: two and five chains per workgroup, the per-lane offsets kernel (scalar and\n"
        "# 16-byte add), one full block; evaluation: a ragged last segment of long rows (257 vectors), scalar rows of 513 lanes\n"
        "shapes += [(4095 * 256, 1, 2000), (10236 * 256 + 100, 3, 2000), (4353, 33, 2000), (4353, 36, 2000), (256, 5, 2000),\n"
        "           (5, 514, 300), (7, 513, 300)]\n"
        "for n, L, nq in shapes:\n"
        "    x = np.cumsum(rng.uniform(0.5, 2.0, n)); y = rng.normal(size=(n, L)); q = rng.uniform(x[0], x[-1], nq)\n"
        "    for s in (pkg.Pchip.new(), pkg.Linear.new()):\n"
        "        it = pkg.Interp1D.builder(y).x(x).strategy(s).build()\n"
        "        t = (it.strategy.data_table(),) + (tuple(it.strategy.coefficients()) if isinstance(s, pkg.Pchip) else (None, None))\n"
        "        P = ar.prefix(x, *t); F = it.antiderivative()\n"
        "        assert np.array_equal(F.strategy.data_table(), P), (type(s).__name__, n, L)\n"
        "        i = oracle.get_lower_index(x, q)\n"
        "        assert np.array_equal(F.interp_array(q).reshape(len(q), L), ar.evaluate(x, *t, P, i, q)), (type(s).__name__, n, L)\n"
        "        assert np.array_equal(F.integrate(q, q[::-1].copy()).reshape(len(q), L), ar.integrate(x, *t, P, i, q, i[::-1], q[::-1])), (n, L)\n"
        "print('checked OK')\n" % (os.path.join(ROOT, "tests"), ROOT))
    env = dict(os.environ, NDI_LIB=lib)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout + r.stderr
