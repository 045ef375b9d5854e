"""GPU: the 2-D lane-wise kernel (ndi_interp2d_eval_lanewise, csrc/lanewise2d_kernels.hpp) on the hostile grids of
tests/hostile_inputs.py (bicubic_*; self-check in tests/test_hostile_inputs.py): adjacent-float knots, knot steps of 2^+-40 /
2^+-400, subnormal results, zeros of both signs, an inf and a NaN node, the largest scale that stays finite on each pair of
knot families, queries at every knot and one ulp either side of it, under extrapolation points far outside and +-inf, and on
periodic builds the hostile wrapped queries (one ulp outside, whole periods out to 2^20, the tiny negative remainder, +-max).

The kernel keeps its own t, u, hx, hy per thread and calls the scalar hermite_nu where the row-wise kernel uses vector forms,
and its Bilinear point divides plainly where the tile path uses div_shared: a contraction, a flushed subnormal or a reordered
product shows on these inputs first.  The yardstick is the numpy restatement evaluated on the device's own tables (which
tests/test_gpu_bicubic_hostile.py and its siblings hold the row-wise kernel to), lane by lane
(hostile_inputs.bicubic_lanewise_reference), bit for bit with zero signs and NaN positions; every case is compared with
per_lane of tests/test_gpu_lanewise2d.py -- the row-wise handle -- first, so that a disagreement says which side moved.

The queries: hostile_inputs.lanewise_arrangement -- lane l holds the query list rotated by l s, s prime to its length, so
every lane meets every query and the lanes of a row sit in different cells.  Every call runs through `run` of
tests/test_gpu_lanewise2d.py: host arrays and device tensors, the output-owning call (check=1) and a caller's buffer
(check=0), NDI_LANEWISE2D_RECORDS 0 and 1, with the plan line asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_inputs as hostile
import oracle
from conftest import ROOT
from hostile_inputs import check_bits
from test_gpu_bicubic import build
from test_gpu_bicubic_periodic import build as build_periodic
from test_gpu_lanewise2d import SENTINEL, expect, per_lane, raw_call, run, surface, tdt, traced

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
LANES = (5, 9)
CASES = [(dt, g, fx, fy) for dt in DTYPES for g in hostile.BICUBIC_GRIDS for fx, fy in hostile.bicubic_pairs(dt)]
PARTIAL_CASES = [(dt, g, fx, fy) for dt in DTYPES for g in hostile.BICUBIC_GRIDS for fx, fy in hostile.bicubic_partial_pairs(dt)]
PERIODIC_CASES = [(dt, g) + c for dt in DTYPES for gi, g in enumerate(hostile.BICUBIC_GRIDS)
                  for c in hostile.bicubic_periodic_cases(dt, gi)]
PLANTED = ("inf node", "nan node")      # every other lane of a periodic array is finite in every row: the periodic top exponent
#                                         was searched for all-finite rows on the whole list, of which the lists here are a part


def ids(cases):
    return [f"{np.dtype(c[0]).name}-{c[1][0]}x{c[1][1]}-" + "-".join(str(v) for v in c[2:]) for c in cases]


def lane_run(pkg, monkeypatch, capfd, it, xs, ys, want, what, **fields):
    """the row-wise handle against the restatement first (per_lane), then the lane-wise call in all its forms"""
    check_bits(per_lane(it, xs, ys), want, f"{what}: the ROW-WISE handle against the restatement")
    run(pkg, monkeypatch, capfd, it, xs, ys, want, what, stage=1, **fields)


def beside_the_planted_lanes(itf, xs, ys, want, names, what):
    """a handle built without the inf / NaN lanes gives every other lane the same bits"""
    import torch
    keep = [l for l, n in enumerate(names) if n not in ("inf node", "nan node")]
    if len(keep) == len(names) or not keep:
        return
    got = itf.interp_lanewise(torch.as_tensor(xs, device="cuda:0"), torch.as_tensor(ys, device="cuda:0")).cpu().numpy()
    check_bits(got[:, keep], want[:, keep], f"{what}: lanes beside the non-finite ones")


def run_case(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, bc, C, part, what):
    """one array of nodes, without and with extrapolation, order (0, 0)"""
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    top = hostile.bicubic_lanewise_top_exponent(dt, fx, fy)
    z, names = hostile.bicubic_nodes(dt, nx, ny, C, part, top)
    for ext in (False, True):
        it = build(pkg, x, y, z, bc, extrapolate=ext)
        xs, ys = hostile.bicubic_lanewise_queries(x, y, ext, C)
        want = hostile.bicubic_lanewise_reference(x, y, z, bc, xs, ys, it.strategy.tables())
        lane_run(pkg, monkeypatch, capfd, it, xs, ys, want, f"{what} ext={ext}", wrap="none")
        if any(n in ("inf node", "nan node") for n in names):
            zf, _ = hostile.bicubic_nodes(dt, nx, ny, C, part, top, finite_only=True)
            beside_the_planted_lanes(build(pkg, x, y, zf, bc, extrapolate=ext), xs, ys, want, names, f"{what} ext={ext}")


def run_bilinear(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, C, part, what):
    """Bilinear on the same knots and nodes: per_lane, and the CPU oracle's Bilinear lane by lane"""
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    top = hostile.bicubic_lanewise_top_exponent(dt, fx, fy)
    z, names = hostile.bicubic_nodes(dt, nx, ny, C, part, top)
    for ext in (False, True):
        it = surface(pkg, "bilinear", x, y, z, extrapolate=ext)
        xs, ys = hostile.bicubic_lanewise_queries(x, y, ext, C)
        want = np.empty(xs.shape, dt)
        for l in range(C):
            r = oracle.interp2d_bilinear(x, y, np.ascontiguousarray(z[:, :, l:l + 1]), np.ascontiguousarray(xs[:, l]),
                                         np.ascontiguousarray(ys[:, l]), ext)
            assert r[0] == oracle.OK, (what, ext, l, r[:3])
            want[:, l] = r[3].reshape(-1)
        lane_run(pkg, monkeypatch, capfd, it, xs, ys, want, f"{what} bilinear ext={ext}", wrap="none")
        if any(n in ("inf node", "nan node") for n in names):
            zf, _ = hostile.bicubic_nodes(dt, nx, ny, C, part, top, finite_only=True)
            beside_the_planted_lanes(surface(pkg, "bilinear", x, y, zf, extrapolate=ext), xs, ys, want, names, f"{what} bilinear ext={ext}")


@pytest.mark.parametrize("dt,grid,fx,fy", CASES, ids=ids(CASES))
def test_hostile_grids_are_bit_exact(pkg, monkeypatch, capfd, dt, grid, fx, fy):
    """every pair of knot families, both grids, both end sets, 5 and 9 lanes with every part of the nine recipes at the recorded
    top exponent; Bilinear on the same grids and nodes"""
    for bi, bc in enumerate(hostile.bicubic_ends()):
        for C in LANES:
            for part in range(hostile.bicubic_parts(C)):
                what = f"{np.dtype(dt).name} {grid[0]}x{grid[1]} {fx} x {fy} ends={bi} C={C} part={part}"
                run_case(pkg, monkeypatch, capfd, dt, grid[0], grid[1], fx, fy, bc, C, part, what)
                if bi == 0:
                    run_bilinear(pkg, monkeypatch, capfd, dt, grid[0], grid[1], fx, fy, C, part, what)


def run_partials(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, shift, what):
    """the orders (1, 1), (2, 0) and (0, 2) on the 25 lanes of bicubic_lanewise_partial_nodes (a top-scale and a subnormal
    lane per order, the top-scale lanes at the exponents found for these query lists); order k runs without extrapolation or
    with it, alternating with k + shift; a handle built without the inf / NaN lanes gives every other lane the same bits"""
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    z, lanes = hostile.bicubic_lanewise_partial_nodes(dt, nx, ny, fx, fy)
    zf, _ = hostile.bicubic_lanewise_partial_nodes(dt, nx, ny, fx, fy, finite_only=True)
    names = [n for n, _ in lanes]
    assert "inf node" in names and "nan node" in names
    C = z.shape[2]
    for k, nu in enumerate(hostile.LANEWISE_PARTIAL_ORDERS):
        ext = bool((k + shift) % 2)
        src = build(pkg, x, y, z, None, extrapolate=ext)
        xs, ys = hostile.bicubic_lanewise_queries(x, y, ext, C)
        want = hostile.bicubic_lanewise_reference(x, y, z, None, xs, ys, src.strategy.tables(), order=nu)
        lane_run(pkg, monkeypatch, capfd, src.partial(*nu), xs, ys, want, f"{what} partial {nu} ext={ext}", wrap="none",
                 nu_x=nu[0], nu_y=nu[1])
        beside_the_planted_lanes(build(pkg, x, y, zf, None, extrapolate=ext).partial(*nu), xs, ys, want, names,
                                 f"{what} partial {nu} ext={ext}")


@pytest.mark.parametrize("dt,grid,fx,fy", PARTIAL_CASES, ids=ids(PARTIAL_CASES))
def test_hostile_partials_are_bit_exact(pkg, monkeypatch, capfd, dt, grid, fx, fy):
    """the scalar hermite_nu<1> and <2> of the lane-wise kernel: H1 and H2 have the divisions by h and h * h, so the pairs
    include the `triple` axes, whose spacing of 3 ulps is no power of two"""
    shift = hostile.bicubic_partial_pairs(dt).index((fx, fy)) + hostile.BICUBIC_GRIDS.index(grid)
    run_partials(pkg, monkeypatch, capfd, dt, grid[0], grid[1], fx, fy, shift,
                 f"{np.dtype(dt).name} {grid[0]}x{grid[1]} {fx} x {fy}")


def run_periodic(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, axes, mixed, C, part, what, thin=5):
    """a periodic build whose handle wraps, on the hostile wrapped queries (every thin-th pair of their cross product); then
    +-inf on the wrapping axis, which wraps to NaN and is refused: index, axis and value of the report with the pre-pass and
    without it"""
    import torch
    cap = pkg._capi
    a = hostile.PERIODIC_AXES[axes]
    x, y = hostile.bicubic_grid(fx, fy, dt, nx, ny)
    top = hostile.bicubic_periodic_top_exponent(dt, fx, fy, axes)
    z, names = hostile.bicubic_periodic_nodes(dt, nx, ny, C, a, part, top)
    bc = hostile.bicubic_periodic_ends(a, mixed)
    it = build_periodic(pkg, x, y, z, a, bc, extrapolate=True)
    assert it.strategy.wraps == a
    qx, qy = hostile.bicubic_periodic_queries(x, y, a)
    xs, ys, _ = hostile.lanewise_arrangement(qx[::thin], qy[::thin], C)
    for k, q, wraps in ((x, xs, a & 1), (y, ys, a & 2)):      # the stride keeps every point of either axis' set
        axis_set = hostile.bicubic_wrap_axis_queries(k) if wraps else hostile.bicubic_axis_queries(k)
        assert all(np.isin(axis_set, q[:, l]).all() for l in range(C)), f"{what}: thin = {thin} drops a query of an axis' set"
    want = hostile.bicubic_lanewise_reference(x, y, z, bc, xs, ys, it.strategy.tables(), periodic=a)
    finite = [l for l, n in enumerate(names) if n not in PLANTED]
    assert hostile.SEAM_LANE in names
    assert np.isfinite(want[:, finite]).all(), f"{what}: the rows of the finite lanes, the top-scale lane among them, are finite"
    lane_run(pkg, monkeypatch, capfd, it, xs, ys, want, what, wrap=axes)
    if any(n in ("inf node", "nan node") for n in names):
        zf, _ = hostile.bicubic_periodic_nodes(dt, nx, ny, C, a, part, top, finite_only=True)
        beside_the_planted_lanes(build_periodic(pkg, x, y, zf, a, bc, extrapolate=True), xs, ys, want, names, what)
    N = len(xs)
    j0, l0 = N // 3, C - 1
    for axis, first, later in ((0, np.inf, -np.inf), (1, -np.inf, np.inf)):
        if not a & (1 << axis):
            continue
        b = [xs.copy(), ys.copy()]
        b[axis][j0, l0] = first
        b[axis][j0 + 5, 0] = later
        dx, dy = (torch.as_tensor(q, device="cuda:0") for q in b)
        for flags in (0, cap.EVAL_FRESH_OUTPUT):
            out = torch.full((N, C), SENTINEL, dtype=tdt(dt), device="cuda:0")
            with traced(capfd) as t:
                st, info = raw_call(pkg, it, dx, dy, N, C, out, C, q_dev=True, out_dev=True, flags=flags)
            w = f"{what}: {first} on axis {axis}, flags = {flags}"
            expect(t.plans, w, n=1, wrap=axes, check=int(flags != 0))
            assert (st, info.index, info.axis, info.value) == (cap.NAN_QUERY, j0 * C + l0, axis, float(first)), \
                (w, st, info.index, info.axis, info.value, cap.last_error())
            o = out.cpu().numpy()
            check_bits(o[:j0], want[:j0], w + ": rows before the failing row")
            if not flags:
                assert np.all(o[j0:] == SENTINEL), w


@pytest.mark.parametrize("dt,grid,fx,fy,axes,mixed", PERIODIC_CASES, ids=ids(PERIODIC_CASES))
def test_hostile_periodic_grids_are_bit_exact(pkg, monkeypatch, capfd, dt, grid, fx, fy, axes, mixed):
    """hostile_inputs.bicubic_periodic_cases: the periodic-axes setting cycles x, y, xy over the pairs; 9 lanes in both parts
    (every recipe and the +0 / -0 seam lane) and 5 lanes"""
    for C, part in ((9, 0), (9, 1), (5, 0)):
        run_periodic(pkg, monkeypatch, capfd, dt, grid[0], grid[1], fx, fy, axes, mixed, C, part,
                     f"{np.dtype(dt).name} {grid[0]}x{grid[1]} {fx} x {fy} periodic {axes} mixed={mixed} C={C} part={part}")


# ---- under the bounds-checked library -----------------------------------------------------------------------------------------
CHECKED_FAMILIES = ("adjacent", "big", "mixed2")


def test_checked_subset(pkg, monkeypatch, capfd):
    """what runs again under the bounds-checked library (below): adjacent, big and mixed2 axes in every pairing, at 5 and 9
    lanes, the grid and the dtype alternating over the pairs; order (0, 0), one partial order and a periodic build each"""
    for i, fx in enumerate(CHECKED_FAMILIES):
        for j, fy in enumerate(CHECKED_FAMILIES):
            dt = DTYPES[(i + j) % 2]
            nx, ny = hostile.BICUBIC_GRIDS[(i + 2 * j) % 2]
            what = f"checked {np.dtype(dt).name} {nx}x{ny} {fx} x {fy}"
            for C in LANES:
                run_case(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, None, C, 0, f"{what} C={C}")
                run_periodic(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, ("x", "y", "xy")[(i + j) % 3], False, C, 0,
                             f"{what} periodic C={C}", thin=11)
            run_bilinear(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, 5, 0, what)
            run_partials(pkg, monkeypatch, capfd, dt, nx, ny, fx, fy, i + j, what)


def test_the_bounds_checked_library_runs_clean():
    """NDI_CHK on both cell indices: a cell index past the grid from a search that hostile knots mislead fails the call"""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lanewise2d_hostile.py"), "-m", "gpu", "-x",
                        "-q", "-k", "test_checked_subset"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
