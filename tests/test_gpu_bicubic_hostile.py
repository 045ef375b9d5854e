"""GPU: the Bicubic build and evaluation on hostile grids (tests/hostile_inputs.py, bicubic_*; self-check in
tests/test_hostile_inputs.py) against the numpy restatement, bit for bit with zero signs and NaN positions: adjacent-float
knots, knot steps of 2^+-40 / 2^+-400, subnormal results, zeros of both signs, an inf and a NaN node, the largest scale that
stays finite on each pair of knot families, queries at every knot and one ulp either side of it, and under extrapolation points far outside and +-inf.
The evaluation has its own divisions and five Hermite forms: a flushed subnormal, a fused multiply-add or an approximate
division shows here first."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_inputs as hostile
from conftest import ROOT
from hostile_inputs import check_bits
from test_gpu_bicubic import build

pytestmark = pytest.mark.gpu

CASES = [(dt, g, fx, fy) for dt in (np.float32, np.float64) for g in hostile.BICUBIC_GRIDS for fx, fy in hostile.bicubic_pairs(dt)]


def rows_of(it, qx, qy, on_device):
    import torch
    if on_device:
        return it.interp_array(torch.as_tensor(qx, device="cuda:0"), torch.as_tensor(qy, device="cuda:0")).cpu().numpy()
    return it.interp_array(qx, qy)


def run_case(pkg, dt, nx, ny, fx, fy, bc, C, part, what):
    """One array: tables against the restatement, rows on the device's own tables for host and device queries, without and
    with extrapolation; where the array has the inf / NaN lanes, a second build without them must leave every other lane's
    tables and rows bit-identical."""
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    top = hostile.bicubic_top_exponent(dt, fx, fy)
    z, names = hostile.bicubic_nodes(dt, nx, ny, C, part, top)
    ref, _ = hostile.bicubic_reference(x, y, z, bc)
    planted = [l for l, n in enumerate(names) if n in ("inf node", "nan node")]
    keep = [l for l in range(C) if l not in planted]
    for ext in (False, True):
        qx, qy = hostile.bicubic_queries(x, y, ext)
        it = build(pkg, x, y, z, bc, extrapolate=ext)
        tabs = it.strategy.tables()
        for name, g, r in zip(("zx", "zy", "zxy"), tabs, ref):
            check_bits(g, r, f"{what} ext={ext} {name}")
        _, want = hostile.bicubic_reference(x, y, z, bc, qx, qy, tabs=tabs)
        got = [rows_of(it, qx, qy, on_device) for on_device in (False, True)]
        for g, where in zip(got, ("host", "device")):
            check_bits(g, want, f"{what} ext={ext} {where} queries")
        if planted and keep:
            zf, _ = hostile.bicubic_nodes(dt, nx, ny, C, part, top, finite_only=True)
            itf = build(pkg, x, y, zf, bc, extrapolate=ext)
            for name, a, b in zip(("zx", "zy", "zxy"), itf.strategy.tables(), tabs):
                check_bits(a[..., keep], b[..., keep], f"{what} ext={ext} {name}: lanes beside the non-finite ones")
            check_bits(rows_of(itf, qx, qy, True)[:, keep], got[1][:, keep], f"{what} ext={ext} rows: lanes beside the non-finite ones")


@pytest.mark.parametrize("dt,grid,fx,fy", CASES, ids=[f"{np.dtype(c[0]).name}-{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}" for c in CASES])
def test_hostile_grids_are_bit_exact(pkg, dt, grid, fx, fy):
    for bi, bc in enumerate(hostile.bicubic_ends()):
        for C in hostile.BICUBIC_LANES:
            for part in range(hostile.bicubic_parts(C)):
                run_case(pkg, dt, grid[0], grid[1], fx, fy, bc, C, part,
                         f"{np.dtype(dt).name} {grid[0]}x{grid[1]} {fx} x {fy} ends={bi} C={C} part={part}")


def test_infinite_queries_need_extrapolation(pkg):
    """include/ndinterp.h: range and errors are Bilinear's -- +-inf is out of range without extrapolation, and a query like
    any other with it (NaN alone is refused then): its row has the restatement's bits, like the +-inf queries of every
    extrapolating case above."""
    for dt in (np.float32, np.float64):
        x, y = hostile.bicubic_grid("uneven", "big", dt, 6, 7)
        z, _ = hostile.bicubic_nodes(dt, 6, 7, 4)
        q = np.array([x[1], np.inf], dt), np.array([y[1], y[2]], dt)
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            build(pkg, x, y, z).interp_array(*q)
        assert e.value.index == 1
        it = build(pkg, x, y, z, extrapolate=True)
        rows = it.interp_array(*q)
        assert rows.shape == (2, 4) and np.all(np.isfinite(rows[0])) and not np.all(np.isfinite(rows[1]))
        check_bits(rows, hostile.bicubic_reference(x, y, z, None, *q, tabs=it.strategy.tables())[1], "an infinite query")


def test_hostile_subset_under_the_bounds_checked_library():
    """adjacent, big and mixed2 axes at 5 and 9 lanes, and one grid whose knots stay in global memory, in a process that loads
    the bounds-checked build: a device-side index out of range fails the call."""
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import os, sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import hostile_inputs as hostile\n"
        "import test_gpu_bicubic_hostile as t, test_gpu_bicubic_plans as p\n"
        "from hostile_inputs import check_bits\n"
        "pkg = load_product_package()\n"
        "fams = ('adjacent', 'big', 'mixed2')\n"
        "for dt in (np.float32, np.float64):\n"
        "    for nx, ny in hostile.BICUBIC_GRIDS:\n"
        "        for fx in fams:\n"
        "            for fy in fams:\n"
        "                for C in (5, 9):\n"
        "                    for part in range(hostile.bicubic_parts(C)):\n"
        "                        t.run_case(pkg, dt, nx, ny, fx, fy, None, C, part, f'{dt.__name__} {nx}x{ny} {fx} x {fy} C={C} part={part}')\n"
        "rng = np.random.default_rng(9)\n"
        "w = p.Wide(pkg, rng, p.uneven(rng, 40_000, np.float32), p.uneven(rng, 5, np.float32), 5)\n"
        "qx, qy = p.sweep(rng, w.x, w.y, 10_000)\n"
        "want = w.rows(qx, qy)\n"
        "os.environ['NDI_TRACE_PLAN'] = '1'\n"
        "for lo, hi in ((0, 4), (0, 5)):\n"
        "    it = w.handle(lo, hi, 'global knots')\n"
        "    check_bits(it.interp_array(qx, qy), want[:, lo:hi], 'global knots, host queries')\n"
        "    check_bits(t.rows_of(it, qx, qy, True), want[:, lo:hi], 'global knots, device queries')\n"
        "print('checked OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDI_LIB=lib), timeout=600)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    plans = [l for l in r.stderr.splitlines() if l.startswith("[ndi plan] bicubic")]
    assert plans and all(" klds=0 " in l for l in plans), plans[:4]
    assert any(" vec=1 " in l for l in plans) and any(" vec=0 " in l for l in plans)
