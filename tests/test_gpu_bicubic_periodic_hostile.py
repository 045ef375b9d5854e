"""GPU: the periodic Bicubic build and the wrapping evaluation on hostile grids (tests/hostile_inputs.py, bicubic_periodic_*;
self-check in tests/test_hostile_inputs.py) against the numpy restatement of the periodic contract
(tests/bicubic_periodic_ref.py), bit for bit with zero signs and NaN positions: adjacent-float knots, knot steps of 2^+-40 /
2^+-400, subnormal nodes, zeros of both signs -- on the seam too, +0 in the first row and -0 in the last -- an inf and a NaN
node off the seam, the largest scale at which the periodic restatement stays finite, and the hostile wrapped queries: one ulp
outside either end, whole periods out to 2^20, a tiny negative remainder, +-max.

The configurations (hostile_inputs.bicubic_periodic_cases): both dtypes, both grids, every pair of knot families, the
periodic-axes setting cycling x, y, xy and the other axis' ends alternating default / MIXED over the pairs; 4 and 9 lanes,
every part."""
import numpy as np
import pytest

import hostile_inputs as hostile
from hostile_inputs import check_bits
from test_gpu_bicubic_periodic import build, check_seam

pytestmark = pytest.mark.gpu

LANES = (4, 9)
CASES = [(dt, g) + c for dt in (np.float32, np.float64) for gi, g in enumerate(hostile.BICUBIC_GRIDS)
         for c in hostile.bicubic_periodic_cases(dt, gi)]
HIDDEN = ("inf node", "nan node", "top scale")      # the lanes the finiteness conditions do not speak of


def rows_of(h, qx, qy, on_device):
    import torch
    if on_device:
        return h.interp_array(torch.as_tensor(qx, device="cuda:0"), torch.as_tensor(qy, device="cuda:0")).cpu().numpy()
    return h.interp_array(qx, qy)


def run_case(pkg, dt, nx, ny, fx, fy, axes, mixed, C, part, what, thin=1):
    """One array: tables against the restatement, and the seam; rows on the device's own tables for host and device queries --
    the handle that wraps on the hostile wrapped queries, the same build without extrapolate on in-range queries; where the
    array has the inf / NaN lanes, a second build without them must leave every other lane's tables and rows bit-identical;
    the (1, 1) partial and the order-2 jet on the same queries."""
    import torch
    a = hostile.PERIODIC_AXES[axes]
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    top = hostile.bicubic_periodic_top_exponent(dt, fx, fy, axes)
    z, names = hostile.bicubic_periodic_nodes(dt, nx, ny, C, a, part, top)
    bc = hostile.bicubic_periodic_ends(a, mixed)
    ref, _ = hostile.bicubic_periodic_reference(x, y, z, bc, a)
    planted = [l for l, n in enumerate(names) if n in ("inf node", "nan node")]
    keep = [l for l in range(C) if l not in planted]
    finite = [l for l, n in enumerate(names) if n not in HIDDEN]
    assert all(np.isfinite(t[..., finite]).all() for t in ref), f"{what}: the tables of the finite lanes are finite"
    for ext in (False, True):
        qx, qy = hostile.bicubic_periodic_queries(x, y, a) if ext else hostile.bicubic_queries(x, y, n_random=300)
        qx, qy = qx[::thin], qy[::thin]          # (thin > 1: the run under the bounds-checked library, every thin-th query)
        dq = torch.as_tensor(qx, device="cuda:0"), torch.as_tensor(qy, device="cuda:0")
        it = build(pkg, x, y, z, a, bc, extrapolate=ext)
        assert it.strategy.wraps == (a if ext else 0)
        tabs = it.strategy.tables()
        for name, g, r in zip(("zx", "zy", "zxy"), tabs, ref):
            check_bits(g, r, f"{what} ext={ext} {name}")
        check_seam(tabs, a, f"{what} ext={ext}")
        _, want = hostile.bicubic_periodic_reference(x, y, z, bc, a, qx, qy, tabs=tabs, wrap=ext)
        assert np.isfinite(want[:, finite]).all(), f"{what} ext={ext}: the rows of the finite lanes are finite"
        got = [rows_of(it, qx, qy, on_device) for on_device in (False, True)]
        for g, where in zip(got, ("host", "device")):
            check_bits(g, want, f"{what} ext={ext} {where} queries")
        if planted and keep:
            zf, _ = hostile.bicubic_periodic_nodes(dt, nx, ny, C, a, part, top, finite_only=True)
            itf = build(pkg, x, y, zf, a, bc, extrapolate=ext)
            for name, u, v in zip(("zx", "zy", "zxy"), itf.strategy.tables(), tabs):
                check_bits(u[..., keep], v[..., keep], f"{what} ext={ext} {name}: lanes beside the non-finite ones")
            check_bits(rows_of(itf, qx, qy, True)[:, keep], got[1][:, keep], f"{what} ext={ext} rows: lanes beside the non-finite ones")
        parts = {nu: hostile.bicubic_periodic_reference(x, y, z, bc, a, qx, qy, tabs=tabs, wrap=ext, order=nu)[1]
                 for nu in pkg.JET_PARTS[2][1:]}
        parts[0, 0] = want
        check_bits(rows_of(it.partial(1, 1), qx, qy, True), parts[1, 1], f"{what} ext={ext} partial (1, 1)")
        for nu, g in zip(pkg.JET_PARTS[2], it.jet(*dq, 2)):
            check_bits(g.cpu().numpy(), parts[nu], f"{what} ext={ext} jet part {nu}")


@pytest.mark.parametrize("dt,grid,fx,fy,axes,mixed", CASES,
                         ids=[f"{np.dtype(c[0]).name}-{c[1][0]}x{c[1][1]}-{c[2]}-{c[3]}-p{c[4]}-{'mixed' if c[5] else 'default'}" for c in CASES])
def test_hostile_periodic_grids_are_bit_exact(pkg, dt, grid, fx, fy, axes, mixed):
    for C in LANES:
        for part in range(hostile.bicubic_periodic_parts(C)):
            run_case(pkg, dt, grid[0], grid[1], fx, fy, axes, mixed, C, part,
                     f"{np.dtype(dt).name} {grid[0]}x{grid[1]} {fx} x {fy} periodic {axes} mixed={mixed} C={C} part={part}")
