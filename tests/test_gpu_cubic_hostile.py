"""GPU: the Pchip / Akima / CubicHermite build and the derivative build on hostile inputs, bit for bit.

tests/hostile_inputs.py plants every branch of the rules, zeros of both signs, subnormal and overflowing scales, adjacent
and 1e30-apart knots, NaN and infinities (tests/test_hostile_inputs.py checks on the CPU that it does, and that such arrays
tell a subtly wrong build from a right one).  Here they go through the device: the tables against the numpy restatements
(tests/hermite_ref.py, tests/derivative_ref.py), the rows against the CPU oracle's interp1d_cubic fed with the restatement's
tables -- compared with check_bits, which sees the sign of a zero and the position of a NaN.  None of these inputs may
fault: they are ordinary floating-point values, and the kernels index by knot and lane only.
"""
import os

import numpy as np
import pytest

import hostile_inputs as hostile
import oracle
from hostile_inputs import check_bits
from test_gpu_hermite import make
from test_gpu_short_rows import knobs

pytestmark = pytest.mark.gpu

NS = (2, 3, 4, 5, 6, 64, 301)
LS = (1, 3, 8, 130)


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _offset(v):
    """a device copy whose address is one element past a 16-byte boundary"""
    import torch
    t = torch.as_tensor(np.ascontiguousarray(v))
    d = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda:0")[1:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 != 0
    return d


def check_handle(pkg, interp, x, y, a, b, what, paths):
    """tables {y, a, b} of a handle against the reference tables, then its rows at hostile.queries through `paths`"""
    ga, gb = interp.strategy.coefficients()
    check_bits(interp.strategy.data_table(), y, what + ": data")
    check_bits(ga, a, what + ": a")
    check_bits(gb, b, what + ": b")
    q = hostile.queries(x)
    _, _, ref = oracle.interp1d_cubic(x, y, a, b, q, oracle.EXTRAPOLATE_YES)
    for path in paths:
        interp.strategy.path = path
        check_bits(_np(interp.interp_array(q)).reshape(ref.shape), ref, f"{what}: rows, path={path}")
    interp.strategy.path = pkg.PATH_AUTO


def run_case(pkg, rule, x, y, k, what, offset=False):
    """one hostile array: the strategy's handle and its first derivative"""
    import torch
    n, L = y.shape
    paths = (pkg.PATH_GATHER, pkg.PATH_BUCKETED, pkg.PATH_AUTO)
    if offset:
        interp = make(pkg, rule, torch.as_tensor(x, device="cuda:0"), _offset(y), None if k is None else _offset(k), extrapolate=True)
    else:       # scalar data as a 1-D array: the shape a caller with one lane has
        interp = make(pkg, rule, x, y.reshape(n) if L == 1 else y, k if k is None or L > 1 else k.reshape(n), extrapolate=True)
    a, b = hostile.reference(rule, x, y, k)
    check_handle(pkg, interp, x, y, a, b, what, paths)
    Y, A, B = hostile.derivative_reference(x, y, a, b)
    check_handle(pkg, interp.derivative(), x, Y, A, B, what + " derivative", paths)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule,n", [(r, n) for r in hostile.RULES for n in NS if not (r == "akima" and n < 3)])
@pytest.mark.parametrize("L", LS)
def test_hostile_tables_and_rows(pkg, dt, rule, n, L):
    """L = 1: scalar data, consecutive threads on consecutive knots; L = 3 (and 130 in f32): one lane per thread; L = 8 (and
    130 in f64): 16-byte vectors -- and those once more from device pointers one element off a 16-byte boundary, which must
    take the one-lane form."""
    vector = L % (16 // np.dtype(dt).itemsize) == 0
    seen = 0
    for tag, x, y, k in hostile.cases(rule, dt, n, L):
        run_case(pkg, rule, x, y, k, tag)
        if vector:
            run_case(pkg, rule, x, y, k, tag + " offset device pointers", offset=True)
        seen += 1
    assert seen >= 5


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("source", ["nk", "nat", "per"])
@pytest.mark.parametrize("n,L", [(3, 1), (5, 3), (64, 8), (301, 130)])
def test_derivative_of_a_spline_on_hostile_scales(pkg, dt, source, n, L):
    """CubicSpline sources: y from the scale recipes, so the derivative rule gets {y, a, b} that overflow, underflow or are
    not finite.  The spline's own build on such data is not under test: its tables are read back and the rule is applied
    to those, first and second derivative."""
    from test_gpu_derivative import make as make_spline, tables_of
    paths = (pkg.PATH_GATHER, pkg.PATH_BUCKETED, pkg.PATH_AUTO)
    seen = 0
    for tag, x, y, _ in hostile.cases("pchip", dt, n, L, classes=("scale",)):
        if source == "per":
            y = y.copy(); y[-1] = y[0]
        src = make_spline(pkg, source, x, y.reshape(n) if L == 1 else y, extrapolate=(source != "per"))
        sy, sa, sb = tables_of(src)
        check_bits(sy, y, tag + ": the spline's data")
        for nu in (1, 2):
            Y, A, B = hostile.derivative_reference(x, sy, sa, sb, nu)
            d = src.derivative(nu)
            if source == "per":      # (no extrapolation: the queries inside the axis)
                ga, gb = d.strategy.coefficients()
                check_bits(d.strategy.data_table(), Y, f"{tag} {source} nu={nu}: data"); check_bits(ga, A, f"{tag} {source} nu={nu}: a")
                check_bits(gb, B, f"{tag} {source} nu={nu}: b")
                q = hostile.queries(x, extrapolate=False)
                _, _, ref = oracle.interp1d_cubic(x, Y, A, B, q)
                for path in paths:
                    d.strategy.path = path
                    check_bits(_np(d.interp_array(q)).reshape(ref.shape), ref, f"{tag} {source} nu={nu}: rows, path={path}")
            else:
                check_handle(pkg, d, x, Y, A, B, f"{tag} {source} nu={nu}", paths)
        seen += 1
    assert seen >= 5


# ---- large device batches: the forms that keep the tables, or {y, k}, in LDS ---------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("rule", hostile.RULES)
@pytest.mark.parametrize("n,L", [(100, 1), (100, 5)])
def test_hostile_large_device_batches(pkg, capfd, dt, rule, n, L):
    """1e6 device queries on the shapes that open the LDS forms.  The {y, k} form evaluates from the kept k table (`kout` of
    the build kernel) and not from a / b: a k that differs from the restatement's shows here while the tables agree.  The
    runs are PATH_AUTO, PATH_GATHER, and PATH_GATHER with the {y, k} form pinned; the plan trace must show that form."""
    import torch
    rng = np.random.default_rng(n + 31 * L)
    plans = []
    for tag, x, y, k in hostile.cases(rule, dt, n, L, classes=("zero", "scale", "nonfinite"), kinds=("even", "uneven")):
        dev = [torch.as_tensor(v, device="cuda:0") for v in (x, y.reshape(n) if L == 1 else y)]
        kd = None if k is None else torch.as_tensor(k.reshape(n) if L == 1 else k, device="cuda:0")
        interp = make(pkg, rule, dev[0], dev[1], kd, extrapolate=True)
        a, b = hostile.reference(rule, x, y, k)
        ga, gb = interp.strategy.coefficients()
        check_bits(ga, a, tag + ": a"); check_bits(gb, b, tag + ": b")
        q = rng.uniform(x[0] - 0.5 * (x[1] - x[0]), x[-1] + 0.5 * (x[-1] - x[-2]), 1_000_000).astype(dt)
        q[:n] = x
        _, _, ref = oracle.interp1d_cubic(x, y, a, b, q, oracle.EXTRAPOLATE_YES)
        qd = torch.as_tensor(q, device="cuda:0")
        os.environ["NDI_TRACE_PLAN"] = "1"
        try:
            for path, pin in ((pkg.PATH_AUTO, {}), (pkg.PATH_GATHER, {}), (pkg.PATH_GATHER, dict(NDI_SHORT_MODE=2, NDI_FUSED_LDS=2))):
                interp.strategy.path = path
                capfd.readouterr()
                with knobs(**pin):
                    got = interp.interp_array(qd).cpu().numpy()
                plan = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[ndi plan]")]
                plans += plan
                check_bits(got.reshape(ref.shape), ref, f"{tag}: path={path} {pin} {plan}")
        finally:
            os.environ.pop("NDI_TRACE_PLAN", None)
    if L > 2:        # (1-2 lanes take the one-thread-per-query kernels, which have no {y, k} form)
        assert any("tables=lds{y,k}" in p for p in plans), sorted(set(plans))
    assert plans


# ---- the bounds-checked build ----------------------------------------------------------------------------------------------
def test_checked_build_runs_hostile_inputs_clean(pkg):
    """One pass of the table and row checks under the bounds-checked build of the library (make debug), in a child process:
    a violation would turn the call into NDI_HIP_ERROR."""
    import subprocess
    import sys
    from conftest import ROOT
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import hostile_inputs as hostile, test_gpu_cubic_hostile as t\n"
        "pkg = load_product_package(); seen = 0\n"
        "for dt in (np.float64, np.float32):\n"
        "    for rule in hostile.RULES:\n"
        "        for n, L in ((2, 3), (3, 1), (5, 8), (64, 130)):\n"
        "            if rule == 'akima' and n < 3: continue\n"
        "            for tag, x, y, k in hostile.cases(rule, dt, n, L):\n"
        "                t.run_case(pkg, rule, x, y, k, tag); seen += 1\n"
        "                if L == 8: t.run_case(pkg, rule, x, y, k, tag + ' offset', offset=True)\n"
        "print('checked OK', seen)\n" % (os.path.join(ROOT, "tests"), ROOT))
    env = dict(os.environ, NDI_LIB=lib)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- the 64-bit index mapping of the two build kernels -----------------------------------------------------------------------
def _hash_rows(xp, rows, L):
    """y[i, l] from an integer hash of (i, l): int64 arithmetic with wrap-around masked to 31 bits -- the same numbers from
    torch on the device and from numpy.  Values are small integers / 8 in [-512, 512): exact in f32, with flat runs rare."""
    i = rows.reshape(-1, 1)
    l = xp.arange(L, dtype=xp.int64).reshape(1, -1) if xp is np else xp.arange(L, dtype=xp.int64, device=rows.device).reshape(1, -1)
    h = (i * 1_000_003 + l * 7_919 + 12_345) & 0x7fffffff
    h = (h * 1_103_515_245 + 12_345) & 0x7fffffff
    h = (h ^ (h >> 13)) & 0x7fffffff
    h = (h * 214_013 + 2_531_011) & 0x7fffffff
    return ((h >> 9) & 0x1fff) - 4096


def test_build_kernels_64_bit_index_mapping(pkg):
    """total = (n - 1) * lanes > 0xffffffff selects the 64-bit `e / LV` of hermite_build_kernel and derivative_build_kernel:
    f32, n = L = 65537 (odd: one lane per thread), 17.2 GB per table.  Nothing that large goes to the host: y comes from an
    integer hash on the device, and rows are compared in about 200 sampled intervals -- the first, the last, those around the
    2^32-th entry (it lies in the last interval) -- with the oracle's evaluation of restatement tables computed for each interval's window i-2 .. i+3.  A
    wrong i or lv in the 64-bit path gives the rows of another interval or lane.  Skips only for lack of device memory."""
    import torch
    n = L = 65537
    dt = np.float32
    need = 9 * n * L * 4 + (8 << 30)      # y (torch) + the handle's {y, a, b, k} + the derivative's {Y, A, B} + working room
    free, total = torch.cuda.mem_get_info(0)
    print(f"\n64-bit mapping: {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB, needs {need / 2**30:.1f} GiB")
    if free < need:
        pytest.skip(f"needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")
    assert (n - 1) * L > 0xffffffff
    dev = torch.device("cuda:0")
    yd = torch.empty((n, L), dtype=torch.float32, device=dev)
    step = 2048
    for r0 in range(0, n, step):
        rows = torch.arange(r0, min(n, r0 + step), dtype=torch.int64, device=dev)
        yd[r0:r0 + len(rows)] = _hash_rows(torch, rows, L).to(torch.float32) * 0.125
    x = np.cumsum(np.random.default_rng(7).uniform(0.5, 2.0, n)).astype(dt)
    assert np.all(np.diff(x) > 0)
    # sampled intervals: both ends, the entries around e = 2^32 (interval e // L, lanes on both sides of e % L), random ones
    # (entry 2^32 = interval 65535, lane 1: the last interval holds it, lane 0 below and the lanes from 1 on above it; every
    # entry of the launch takes the 64-bit division, so every sampled interval checks it)
    edge = (1 << 32) // L
    assert edge == n - 2 and (1 << 32) - edge * L == 1
    rng = np.random.default_rng(11)
    iv = sorted({0, 1, 2, edge - 3, edge - 2, edge - 1, edge} | {int(v) for v in rng.integers(0, n - 1, 190)})
    assert iv[0] == 0 and iv[-1] == n - 2
    T = dt
    q = np.concatenate([[x[i], x[i] + (x[i + 1] - x[i]) / T(2), np.nextafter(x[i + 1], T(-np.inf))] for i in iv] + [[x[-1]]]).astype(dt)
    owner = np.concatenate([[i, i, i] for i in iv] + [[n - 2]])
    assert np.all((np.searchsorted(x, q, side="right") - 1).clip(0, n - 2) == owner)
    # the windows' rows on the host, checked against the numpy form of the hash
    windows = {}
    for i in iv:
        lo, hi = max(0, i - 2), min(n - 1, i + 3)
        yw = yd[lo:hi + 1].cpu().numpy()
        assert np.array_equal(yw, (_hash_rows(np, np.arange(lo, hi + 1, dtype=np.int64), L).astype(np.float32) * np.float32(0.125)))
        windows[i] = (lo, yw)
    src = pkg.Interp1D.builder(yd).x(torch.as_tensor(x, device=dev)).strategy(pkg.Akima.new()).build()
    del yd
    torch.cuda.empty_cache()
    qd = torch.as_tensor(q, device=dev)

    def compare(interp, tables, what):
        got = interp.interp_array(qd).cpu().numpy().reshape(len(q), L)
        for i in iv:
            lo, yw = windows[i]
            xw = x[lo:lo + len(yw)]
            tw = tables(xw, yw)
            sel = np.flatnonzero(owner == i)
            _, _, ref = oracle.interp1d_cubic(xw, tw[0], tw[1], tw[2], q[sel])
            check_bits(got[sel], ref.reshape(len(sel), L), f"{what}: interval {i} (entry {i * L} .. {i * L + L - 1})")

    def akima_tables(xw, yw):
        a, b = hostile.reference("akima", xw, yw)
        return yw, a, b
    compare(src, akima_tables, "Akima 65537 x 65537")
    src.strategy.trim()
    d = src.derivative()
    del src
    torch.cuda.empty_cache()
    # the derivative's window tables: Y[i] needs a_i and y_i, y_{i+1} only, so the window serves as it is -- except that a
    # window cut short of the axis' end must not take its own last row for the last knot: only intervals are compared
    compare(d, lambda xw, yw: hostile.derivative_reference(xw, *akima_tables(xw, yw)), "its derivative")
