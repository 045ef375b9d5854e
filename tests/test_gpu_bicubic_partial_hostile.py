"""GPU: the partial-derivative handles of Bicubic on the hostile grids (tests/hostile_inputs.py, bicubic_partial_nodes; self-check
in tests/test_hostile_inputs.py) against the numpy restatement (tests/bicubic_partial_ref.py), bit for bit with zero signs and
NaN positions.  H1 and H2 divide by h and by h * h, a product found nowhere else in the kernel, four times along y and once
along x: an approximate or reciprocal division, a flushed subnormal or a contracted kl * h - d shows on adjacent-float knots,
on steps of 2^+-40 / 2^+-400, and in the lanes scaled per order -- the largest scale whose rows of that order stay finite, and
the scale that makes most of them subnormal.  One array of 25 lanes per (grid, pair, ends) serves all eight orders: every
handle shares the one node table, and every lane is compared under every order (a lane scaled for another order is mostly
inf or 0 there, which still compares)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bicubic_partial_ref as ref
import hostile_inputs as hostile
from conftest import ROOT
from hostile_inputs import check_bits
from test_gpu_bicubic import build
from test_gpu_bicubic_plans import dev, sentinel_buffer, to_np

pytestmark = pytest.mark.gpu

CASES = [(dt, g, fx, fy) for dt in (np.float32, np.float64) for g in hostile.BICUBIC_GRIDS for fx, fy in hostile.bicubic_partial_pairs(dt)]
N_RANDOM = 300
# every point of each axis' query set with a quarter of the other axis' on the 65 x 5 grid (7801 pairs otherwise, eight orders)
THIN = {6: 1, 65: 4}
INTO = ((1, 2), (2, 1))       # the orders that also go through interp_array_into (the pre-pass plan), once per dtype each


def rows_of(p, qx, qy, on_device):
    return to_np(p.interp_array(dev(qx), dev(qy))) if on_device else p.interp_array(qx, qy)


def run_case(pkg, dt, nx, ny, fx, fy, bc, what, orders=ref.ORDERS, lanes=hostile.BICUBIC_PARTIAL_LANES, into=()):
    """One (grid, pair, ends): without and with extrapolation, 25 lanes (scalar form) and 28 (16-byte vectors); the tables
    against the restatement, then the rows of every order on the device's own tables for host and device queries; a second
    build without the inf / NaN lanes must leave every other lane's rows of every order bit-identical."""
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    C = max(lanes)
    z, names = hostile.bicubic_partial_nodes(dt, nx, ny, fx, fy, C)
    zf, _ = hostile.bicubic_partial_nodes(dt, nx, ny, fx, fy, C, finite_only=True)
    ref_tabs, _ = hostile.bicubic_reference(x, y, z, bc)
    keep = [l for l, (n, _) in enumerate(names) if n not in ("inf node", "nan node")]
    for ext in (False, True):
        qx, qy = hostile.bicubic_queries(x, y, ext, n_random=N_RANDOM, thin=THIN[nx])
        want = {}
        for Cn in lanes:
            w = f"{what} ext={ext} C={Cn}"
            it = build(pkg, x, y, np.ascontiguousarray(z[:, :, :Cn]), bc, extrapolate=ext)
            tabs = it.strategy.tables()
            for name, g, r in zip(("zx", "zy", "zxy"), tabs, ref_tabs):
                check_bits(g, r[:, :, :Cn], f"{w} {name}")
            itf = build(pkg, x, y, np.ascontiguousarray(zf[:, :, :Cn]), bc, extrapolate=ext)
            k = [l for l in keep if l < Cn]
            for order in orders:
                if order not in want:      # lanes are independent and the tables are the restatement's, bit for bit (held
                    # just above for each build): the rows of the widest array, cut to Cn lanes, are the reference of each
                    want[order] = hostile.bicubic_reference(x, y, z, bc, qx, qy, tabs=ref_tabs, order=order)[1]
                p = it.partial(*order)
                got = [rows_of(p, qx, qy, on_device) for on_device in (False, True)]
                for g, where in zip(got, ("host", "device")):
                    check_bits(g, want[order][:, :Cn], f"{w} order {order} {where} queries")
                check_bits(rows_of(itf.partial(*order), qx, qy, True)[:, k], got[1][:, k],
                           f"{w} order {order}: lanes beside the non-finite ones")
                if order in into:
                    for on_device in (False, True):
                        buf = sentinel_buffer((len(qx), Cn), dt, on_device)
                        q = (dev(qx), dev(qy)) if on_device else (qx, qy)
                        p.interp_array_into(*q, buf)
                        check_bits(to_np(buf), want[order][:, :Cn], f"{w} order {order} into a sentinel buffer, device={on_device}")


@pytest.mark.parametrize("dt,grid,fx,fy", CASES, ids=[f"{np.dtype(c[0]).name}-{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}" for c in CASES])
def test_hostile_grids_are_bit_exact_for_every_order(pkg, dt, grid, fx, fy):
    # interp_array_into on the pair whose spacings differ most on the two axes, one case per dtype and grid
    into = INTO if (fx, fy) == ("adjacent", "big") else ()
    for bi, bc in enumerate(hostile.bicubic_ends()):
        run_case(pkg, dt, grid[0], grid[1], fx, fy, bc, f"{np.dtype(dt).name} {grid[0]}x{grid[1]} {fx} x {fy} ends={bi}", into=into)


def test_hostile_partials_under_the_bounds_checked_library():
    """adjacent, big and mixed2 axes, orders (1, 0), (1, 2), (2, 1), (2, 2), and one grid whose knots stay in global memory, in
    a process that loads the bounds-checked build: a device-side index out of range fails the call."""
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import os, sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import hostile_inputs as hostile\n"
        "import bicubic_partial_ref as ref, test_gpu_bicubic_partial_hostile as t, test_gpu_bicubic_plans as p\n"
        "from hostile_inputs import check_bits\n"
        "pkg = load_product_package()\n"
        "fams = ('adjacent', 'big', 'mixed2')\n"
        "orders = ((1, 0), (1, 2), (2, 1), (2, 2))\n"
        "for dt in (np.float32, np.float64):\n"
        "    for nx, ny in hostile.BICUBIC_GRIDS:\n"
        "        for fx in fams:\n"
        "            for fy in fams:\n"
        "                t.run_case(pkg, dt, nx, ny, fx, fy, None, f'{dt.__name__} {nx}x{ny} {fx} x {fy}', orders, into=t.INTO)\n"
        "rng = np.random.default_rng(9)\n"
        "w = p.Wide(pkg, rng, p.uneven(rng, 40_000, np.float32), p.uneven(rng, 5, np.float32), 5)\n"
        "qx, qy = p.sweep(rng, w.x, w.y, 2_000)\n"
        "os.environ['NDI_TRACE_PLAN'] = '1'\n"
        "with np.errstate(all='ignore'):\n"
        "    want = {o: ref.evaluate(w.x, w.y, w.z, *w.tabs, qx, qy, *o) for o in orders}\n"
        "for lo, hi in ((0, 4), (0, 5)):\n"
        "    it = w.handle(lo, hi, 'global knots')\n"
        "    for order in orders:\n"
        "        h = it.partial(*order)\n"
        "        check_bits(h.interp_array(qx, qy), want[order][:, lo:hi], f'global knots, order {order}, host queries')\n"
        "        check_bits(t.rows_of(h, qx, qy, True), want[order][:, lo:hi], f'global knots, order {order}, device queries')\n"
        "print('checked OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDI_LIB=lib), timeout=600)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    plans = [l for l in r.stderr.splitlines() if l.startswith("[ndi plan] bicubic")]
    assert len(plans) >= 16 and all(" klds=0 " in l for l in plans), plans[:4]
    assert any(" vec=1 " in l for l in plans) and any(" vec=0 " in l for l in plans)
    assert {l.rsplit("nu=", 1)[1].strip() for l in plans} == {"1,0", "1,2", "2,1", "2,2"}, plans[:4]
