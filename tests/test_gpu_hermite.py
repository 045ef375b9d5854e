"""GPU: the Pchip / Akima / CubicHermite strategies on the device, bit for bit.

The build kernel (csrc/hermite_kernels.hpp) follows the header's numerical specification operation by operation, so its
a / b tables equal the numpy restatement's (tests/hermite_ref.py, checked against scipy in tests/test_hermite_abi.py)
exactly; evaluation is the spline's, so rows equal the CPU oracle's interp1d_cubic fed with those tables exactly."""
import os

import numpy as np
import pytest

import hermite_ref
import oracle
from conftest import GOLDEN
from test_gpu_parity import SHAPES_1D, check_equal, knots

pytestmark = pytest.mark.gpu

RULES = ["pchip", "akima"]


def builder(pkg, rule, dydx=None):
    return {"pchip": pkg.Pchip.new, "akima": pkg.Akima.new}[rule]() if rule != "hermite" else pkg.CubicHermite.new(dydx)


def make(pkg, rule, x, y, dydx=None, extrapolate=False):
    return pkg.Interp1D.builder(y).x(x).strategy(builder(pkg, rule, dydx).extrapolate(extrapolate)).build()


def check_tables(interp, x, y, rule, what, dydx=None):
    a, b = interp.strategy.coefficients()
    ra, rb = hermite_ref.build(rule, x, y, dydx)
    check_equal(a, ra, what + ": a")
    check_equal(b, rb, what + ": b")
    return ra, rb


def data(rng, n, L, dt, rounded=False):
    """uneven knots; values with sign changes (rounded: flat runs and zeros too, the branches of the Pchip rule)"""
    x = np.cumsum(rng.uniform(0.1, 2.0, n)).astype(dt)
    assert np.all(np.diff(x) > 0)
    y = rng.normal(size=(n, L))
    return x, (np.round(y) if rounded else y).astype(dt)


# ---- 3. the tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", RULES)
def test_tables_of_the_golden_cases(pkg, rule):
    g = np.load(os.path.join(GOLDEN, "hermite_scipy.npz"))
    seen = 0
    for cid in g["cases"]:
        if cid + "/" + rule not in g:
            continue
        x, q = g[cid + "/x"], g[cid + "/q"]
        y = g[cid + ("/y_akima" if rule == "akima" else "/y")]
        interp = make(pkg, rule, x, y, extrapolate=True)
        a, b = check_tables(interp, x, y, rule, f"{rule} {cid}")
        # ... and the rows: the oracle's evaluation of those tables, which is within the stored bound of scipy
        _, _, ref = oracle.interp1d_cubic(x, y, a, b, q, oracle.EXTRAPOLATE_YES)
        got = interp.interp_array(q)
        check_equal(got.reshape(ref.shape), ref, f"{rule} {cid} rows")
        name = x.dtype.name
        dev = np.abs(ref.astype(np.float64) - g[cid + "/" + rule]).max() / (np.abs(y.astype(np.float64)).max() + 1)
        assert dev <= 4.0 * float(g[f"deviation/{name}/{rule}"]), (cid, dev)
        seen += 1
    assert seen == (44 if rule == "pchip" else 36)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule,n", [(r, n) for r in RULES for n in (2, 3, 4, 5, 6) if not (r == "akima" and n == 2)])
@pytest.mark.parametrize("L", [1, 5, 64, 100, 4096])
def test_tables_small_n_every_lane_mapping(pkg, dt, rule, n, L):
    rng = np.random.default_rng(1000 * n + L)
    for rounded in (False, True):
        x, y = data(rng, n, L, dt, rounded)
        check_tables(make(pkg, rule, x, y), x, y, rule, f"{rule} n={n} L={L} rounded={rounded}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("n,L", [(1_000_000, 1), (4096, 4096), (100_000, 8), (100, 5), (257, 130), (1000, 6)])
def test_tables_large_host_and_device_inputs(pkg, dt, rule, n, L):
    import torch
    rng = np.random.default_rng(n + L)
    x, y = data(rng, n, L, dt, rounded=(L == 1))
    if L == 1:
        y = y.reshape(n)
    ra, rb = check_tables(make(pkg, rule, x, y), x, y, rule, f"{rule} {n} x {L} host arrays")
    yd = torch.as_tensor(y, device="cuda:0"); xd = torch.as_tensor(x, device="cuda:0")
    dev = pkg.Interp1D.builder(yd).x(xd).strategy(builder(pkg, rule)).build()
    a, b = dev.strategy.coefficients()
    check_equal(a, ra, "device tensors: a"); check_equal(b, rb, "device tensors: b")


# ---- 4. evaluation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("n,L,Q", SHAPES_1D)
def test_eval_bit_exact_every_path(pkg, dt, rule, n, L, Q):
    rng = np.random.default_rng(n * 7919 + L)
    x = knots("rand", n, rng, dt)
    y = rng.uniform(-1.0, 1.0, (n, L)).astype(dt)
    q = rng.uniform(x[0], x[-1], Q).astype(dt)
    q[:3] = [x[0], x[-1], x[n // 2]]
    interp = make(pkg, rule, x, y)
    a, b = check_tables(interp, x, y, rule, f"{rule} n={n} L={L}")
    _, _, ref = oracle.interp1d_cubic(x, y, a, b, q)
    for path in (pkg.PATH_GATHER, pkg.PATH_BUCKETED, pkg.PATH_AUTO):
        interp.strategy.path = path
        check_equal(interp.interp_array(q), ref, f"{rule} n={n} L={L} path={path}")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule,n,L", [("pchip", 100, 1), ("akima", 100, 1), ("pchip", 100, 5), ("akima", 100, 5),
                                      ("pchip", 2, 1), ("pchip", 2, 7), ("pchip", 3, 2), ("akima", 3, 2)])
def test_eval_short_rows_device_batches(pkg, dt, rule, n, L):
    """Scalar / short-row data with 1e6 device queries: the forms that keep the tables (or {y, k}) in LDS; also the
    two-knot tables the spline never had."""
    import torch
    rng = np.random.default_rng(n + 31 * L)
    x, y = data(rng, n, L, dt)
    yy = y.reshape(n) if L == 1 else y
    for extrapolate in (False, True):
        interp = make(pkg, rule, x, yy, extrapolate=extrapolate)
        a, b = hermite_ref.build(rule, x, y)
        lo, hi = (x[0], x[-1]) if not extrapolate else (x[0] - 0.5 * (x[1] - x[0]), x[-1] + 0.5 * (x[-1] - x[-2]))
        q = rng.uniform(lo, hi, 1_000_000).astype(dt)
        _, _, ref = oracle.interp1d_cubic(x, y, a, b, q, oracle.EXTRAPOLATE_YES if extrapolate else oracle.EXTRAPOLATE_NO)
        qd = torch.as_tensor(q, device="cuda:0")
        for path in (pkg.PATH_AUTO, pkg.PATH_GATHER):
            interp.strategy.path = path
            got = interp.interp_array(qd).cpu().numpy()
            check_equal(got.reshape(ref.shape), ref, f"{rule} n={n} L={L} extrapolate={extrapolate} path={path}")
            check_equal(interp.interp_array(q).reshape(ref.shape), ref, f"{rule} n={n} L={L} host batch path={path}")


@pytest.mark.parametrize("rule", RULES)
def test_first_error_ring_sharded_clone(pkg, rule):
    import torch
    rng = np.random.default_rng(5)
    n, L, Q = 20, 1024, 4099
    x, y = data(rng, n, L, np.float64)
    interp = make(pkg, rule, x, y)
    a, b = check_tables(interp, x, y, rule, rule)
    q = rng.uniform(x[0], x[-1], Q)
    _, _, ref = oracle.interp1d_cubic(x, y, a, b, q)
    # OutOfBounds: the reference's message and first-error semantics -- rows before the failure written, later ones untouched
    qbad = q.copy(); qbad[317] = x[0] - 0.1; qbad[500] = x[-1] + 99.0
    for path in (pkg.PATH_GATHER, pkg.PATH_BUCKETED):
        interp.strategy.path = path
        buf = np.full((Q, L), -7.0)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as ei:
            interp.interp_array_into(qbad, buf)
        assert ei.value.index == 317 and str(ei.value).startswith("x = ") and str(ei.value).endswith(" is not in range")
        assert np.array_equal(buf[:317], ref[:317]) and np.all(buf[317:] == -7.0)
    interp.strategy.path = pkg.PATH_AUTO
    # ring
    qd = torch.as_tensor(q, device="cuda:0")
    got = np.zeros_like(ref)
    ring = pkg.striped_ring(1024, L, 2, np.float64, 0)

    def consumer(c, rows):
        got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
    interp.interp_array_ring(qd, 1024, consumer, slots=ring)
    check_equal(got, ref, "ring")
    # clone: tables copied, nothing rebuilt; then one sharded call over the original and the replica
    rep = interp.replicate([0])[0]
    ca, cb = rep.strategy.coefficients()
    check_equal(ca, a, "clone a"); check_equal(cb, b, "clone b")
    check_equal(rep.interp_array(q), ref, "clone rows")
    got = np.full_like(ref, -1.0)
    pkg.sharding.interp_array_sharded([interp, rep], q, out=got)
    check_equal(got, ref, "sharded")
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as ei:
        pkg.sharding.interp_array_sharded([interp, rep], qbad, out=got)
    assert ei.value.index == 317
    # replicas of different strategies over the same knots are not one interpolator
    other = make(pkg, "akima" if rule == "pchip" else "pchip", x, y)
    with pytest.raises(pkg.DeviceError, match="same knots, strategy"):
        pkg.sharding.interp_array_sharded([interp, other], q, out=got)
    interp.strategy.trim()


# ---- 5. CubicHermite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n,L", [(2, 1), (3, 5), (100, 5), (64, 4096), (1000, 64), (50_000, 1)])
def test_cubic_hermite(pkg, dt, n, L):
    import torch
    rng = np.random.default_rng(n * 3 + L)
    x, y = data(rng, n, L, dt)
    # with Pchip's own derivatives: the Pchip handle's tables, bit for bit -- host and device dydx
    k = hermite_ref.pchip_k(x, y)
    pa, pb = make(pkg, "pchip", x, y).strategy.coefficients()
    ha, hb = make(pkg, "hermite", x, y, k).strategy.coefficients()
    check_equal(ha, pa, "hermite(pchip_k) a"); check_equal(hb, pb, "hermite(pchip_k) b")
    yd, xd, kd = (torch.as_tensor(v, device="cuda:0") for v in (y, x, k))
    dev = pkg.Interp1D.builder(yd).x(xd).strategy(pkg.CubicHermite.new(kd)).build()
    da, db = dev.strategy.coefficients()
    check_equal(da, pa, "hermite(device pchip_k) a"); check_equal(db, pb, "hermite(device pchip_k) b")
    # device derivatives at an address that is not 16-byte aligned (read in place: the one-lane form takes over)
    kv = torch.empty(n * L + 1, dtype=kd.dtype, device="cuda:0")[1:].view(n, L)
    kv.copy_(kd)
    va, vb = pkg.Interp1D.builder(yd).x(xd).strategy(pkg.CubicHermite.new(kv)).build().strategy.coefficients()
    check_equal(va, pa, "hermite(offset device pchip_k) a"); check_equal(vb, pb, "hermite(offset device pchip_k) b")
    # random derivatives: the restatement's tables, and rows through every path
    k = rng.normal(size=(n, L)).astype(dt)
    interp = make(pkg, "hermite", x, y, k, extrapolate=True)
    a, b = check_tables(interp, x, y, "hermite", f"hermite n={n} L={L}", k)
    q = rng.uniform(x[0] - 0.5 * (x[1] - x[0]), x[-1] + 0.5 * (x[-1] - x[-2]), 3000).astype(dt)
    _, _, ref = oracle.interp1d_cubic(x, y, a, b, q, oracle.EXTRAPOLATE_YES)
    for path in (pkg.PATH_GATHER, pkg.PATH_BUCKETED, pkg.PATH_AUTO):
        interp.strategy.path = path
        check_equal(interp.interp_array(q), ref, f"hermite n={n} L={L} path={path}")
        check_equal(interp.interp_array(torch.as_tensor(q, device="cuda:0")).cpu().numpy(), ref, f"hermite device batch path={path}")


# ---- 6. the same evaluation form as a spline of that shape ------------------------------------------------------------------
@pytest.mark.parametrize("n,L,Q", [(100, 1, 1_000_000), (100, 5, 200_000), (4096, 4096, 20_000)])
def test_auto_takes_the_splines_evaluation_form(pkg, n, L, Q):
    import torch
    rng = np.random.default_rng(n + L)
    x, y = data(rng, n, L, np.float64)
    yy = y.reshape(n) if L == 1 else y
    qd = torch.as_tensor(rng.uniform(x[0], x[-1], Q), device="cuda:0")
    taken = {}
    for name, strat in (("spline", pkg.CubicSpline.new()), ("pchip", pkg.Pchip.new()), ("akima", pkg.Akima.new())):
        interp = pkg.Interp1D.builder(yy).x(x).strategy(strat).build()
        pkg.profile_enable(True); pkg.profile_read(reset=True)
        try:
            interp.interp_array(qd)
            taken[name] = pkg.profile_read(reset=True)
        finally:
            pkg.profile_enable(False)
    for name in ("pchip", "akima"):
        for key in ("last_path", "eval_launches", "locate_launches", "group_launches"):
            assert taken[name][key] == taken["spline"][key], (name, key, taken)


def test_checked_build_runs_the_new_kernel_clean(pkg):
    """The bounds-checked build of the library (make debug) on the new handles, in a child process."""
    import subprocess
    import sys
    from conftest import ROOT
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import hermite_ref\n"
        "pkg = load_product_package(); rng = np.random.default_rng(1)\n"
        "for n, L in ((2, 3), (3, 1), (7, 130), (500, 64)):\n"
        "    x = np.cumsum(rng.uniform(0.1, 2.0, n)); y = rng.normal(size=(n, L)); q = rng.uniform(x[0], x[-1], 5000)\n"
        "    for rule, s in (('pchip', pkg.Pchip.new()), ('akima', pkg.Akima.new()), ('hermite', pkg.CubicHermite.new(y))):\n"
        "        if rule == 'akima' and n < 3: continue\n"
        "        it = pkg.Interp1D.builder(y).x(x).strategy(s).build()\n"
        "        a, b = it.strategy.coefficients(); ra, rb = hermite_ref.build(rule, x, y, y)\n"
        "        assert np.array_equal(a, ra) and np.array_equal(b, rb), (rule, n, L)\n"
        "        it.interp_array(q)\n"
        "print('checked OK')\n" % (os.path.join(ROOT, "tests"), ROOT))
    env = dict(os.environ, NDI_LIB=lib)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout + r.stderr
