"""GPU: 2-D antiderivative handles and rectangle integrals of Bicubic (ndi_interp2d_antiderivative, ndi_interp2d_integral,
ndi_interp2d_integral_tables) against the numpy restatement of their contract (tests/bicubic_integral_ref.py) applied to the
device's own node tables, bit for bit, f32 and f64: the five prefix tables on every build plan, F rows and rectangle rows on
every branch of the evaluation kernel at the smallest shapes that reach it (each held to its plan line), the error
semantics of the four bounds, the life of the handles, the bounds-checked library, and the value and partial paths as
they were."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bicubic_integral_ref as ref
import bicubic_partial_ref
import bicubic_ref
import hostile_inputs
from conftest import ROOT
from hostile_inputs import check_bits
from test_gpu_bicubic import build, make_grid
from test_gpu_bicubic_plans import PLAN, SENTINEL, dev, sentinel_buffer, to_np, uneven, vn

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
EVAL = re.compile(r"\[ndi plan\] bicubic integral rect=(\d+) vec=(\d+) lv=(\d+) klds=(\d+) grid=(\d+) x (\d+) lds=(\d+) "
                  r"prepass=(\d+)\n")
EVAL_FIELDS = ("rect", "vec", "lv", "klds", "gx", "gy", "lds", "prepass")
BUILD = re.compile(r"\[ndi plan\] bicubic integral build nx=(\d+) ny=(\d+) lanes=(\d+) xview=(\d+) yview=(\d+) passes=5\n")
PASS = re.compile(r"\[ndi plan\] antiderivative build linear=0 staged=(\d+) kb=\d+ vec=\d+ vec_local=\d+ nblk=(\d+) single=(\d+) "
                  r"fuse=(\d+) grid=\d+\n")


def trace(capfd, call):
    """(result, stderr) of the call under NDI_TRACE_PLAN"""
    capfd.readouterr()
    before = os.environ.get("NDI_TRACE_PLAN")
    os.environ["NDI_TRACE_PLAN"] = "1"
    try:
        r = call()
    finally:
        if before is None:
            del os.environ["NDI_TRACE_PLAN"]
        else:
            os.environ["NDI_TRACE_PLAN"] = before
    return r, capfd.readouterr().err


def traced(capfd, call, what, **fields):
    """the call's result; every integral plan line it printed (at least one) carries `fields`"""
    r, err = trace(capfd, call)
    plans = [dict(zip(EVAL_FIELDS, (int(v) for v in m.groups()))) for m in EVAL.finditer(err)]
    assert plans, f"{what}: no integral plan line in: {err[-500:]}"
    for p in plans:
        assert {k: p[k] for k in fields} == fields, f"{what}: plan {p} where {fields} was expected"
    return r


def setup(pkg, x, y, z, **kw):
    """(surface, integral, node tables of the device, its prefix tables)"""
    it = build(pkg, x, y, z, **kw)
    F = it.antiderivative()
    return it, F, (z,) + tuple(it.strategy.tables()), F.strategy.integral_tables()


def f_rows(x, y, nodes, tabs, qx, qy):
    with np.errstate(all="ignore"):
        return ref.evaluate(x, y, nodes, tabs, qx, qy)


def r_rows(x, y, nodes, tabs, r):
    with np.errstate(all="ignore"):
        return ref.rectangle(x, y, nodes, tabs, *r)


def rectangles(qx, qy, rng):
    """(xa, xb, ya, yb) from a query set: each point against a shuffled partner, so reversed bounds come by themselves;
    the first three (where there are that many) are degenerate in x, in y and in both"""
    k = rng.permutation(len(qx))
    xa, xb, ya, yb = qx.copy(), qx[k].copy(), qy.copy(), qy[k].copy()
    if len(qx) >= 3:
        xb[0], yb[1], xb[2], yb[2] = xa[0], ya[1], xa[2], ya[2]
    return xa, xb, ya, yb


def rect_both_ways(F, r, want, what, capfd=None, **fields):
    out = [F.integral(*r), to_np(F.integral(*[dev(b) for b in r]))] if capfd is None else \
        [traced(capfd, lambda: F.integral(*r), what, rect=1, **fields),
         to_np(traced(capfd, lambda: F.integral(*[dev(b) for b in r]), what, rect=1, **fields))]
    check_bits(out[0], want, f"{what}: host bounds")
    check_bits(out[1], want, f"{what}: device bounds")


def f_both_ways(F, qx, qy, want, what, capfd=None, **fields):
    if capfd is None:
        out = [F.interp_array(qx, qy), to_np(F.interp_array(dev(qx), dev(qy)))]
    else:
        out = [traced(capfd, lambda: F.interp_array(qx, qy), what, rect=0, **fields),
               to_np(traced(capfd, lambda: F.interp_array(dev(qx), dev(qy)), what, rect=0, **fields))]
    check_bits(out[0], want, f"{what}: host queries")
    check_bits(out[1], want, f"{what}: device queries")


# ---- the five tables, every build plan ----------------------------------------------------------------------------------------
SHAPES = [(5, 7, 3), (9, 6, 8), (257, 5, 3), (5, 513, 2), (258, 257, 1), (4354, 3, 1), (3, 4354, 2), (4354, 3, 12)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_tables_are_bit_exact_on_every_build_plan(pkg, capfd, dt, shape):
    """The prefix tables against the restatement on the device's own node tables, and the build held to its plan lines:
    one line of the 2-D build, then the five 1-D prefix builds in the order Qz, Qzy (along x), Pz, Pzx (along y), PP (along
    x), each staged through LDS or not by the width of its view (<= 32 lanes), in one block, with the offsets fused into the
    add (<= 17 blocks) or in a pass of their own.  5 x 7 x 3 and 257 x 5 x 3: views narrower than 32; 9 x 6 x 8 and
    4354 x 3 x 12: wider; 257 / 258 / 513: the block edges; 4354: 18 blocks, past the fused offsets."""
    nx, ny, Cn = shape
    rng = np.random.default_rng(nx * 1000 + ny)
    x, y = uneven(rng, nx, dt), uneven(rng, ny, dt)
    z = rng.normal(size=shape).astype(dt)
    it = build(pkg, x, y, z)
    F, err = trace(capfd, lambda: it.antiderivative())
    assert [tuple(map(int, m.groups())) for m in BUILD.finditer(err)] == [(nx, ny, Cn, ny * Cn, nx * Cn)], err[-800:]
    want_pass = []
    for n, view in ((nx, ny * Cn), (nx, ny * Cn), (ny, nx * Cn), (ny, nx * Cn), (nx, ny * Cn)):
        nblk = (n + 255) // 256
        want_pass.append((int(view <= 32), nblk, int(nblk == 1), int(nblk > 1 and nblk <= 17)))
    assert [tuple(map(int, m.groups())) for m in PASS.finditer(err)] == want_pass, err[-1500:]
    nodes = (z,) + tuple(it.strategy.tables())
    got = F.strategy.integral_tables()
    for name, g, w in zip(("PP", "Qz", "Qzy", "Pz", "Pzx"), got, ref.tables(x, y, *nodes)):
        check_bits(g, w, name)
    for g, d in zip(got, F.strategy.integral_tables(on_device=True)):
        check_bits(to_np(d), g, "tables handed back in device memory")
    for a, b in zip(F.strategy.tables(), nodes[1:]):           # ndi_interp2d_tables of an integral handle: the origin's
        check_bits(a, b, "node tables of the integral handle")
    assert np.all(got[0][0] == 0) and np.all(got[0][:, 0] == 0) and np.all(got[1][0] == 0) and np.all(got[3][:, 0] == 0)
    # rows on these tables: the whole domain, nodes, random rectangles
    qx = np.clip(np.concatenate([[x[0], x[-1], x[-1], x[nx // 2]], rng.uniform(x[0], x[-1], 60)]).astype(dt), x[0], x[-1])
    qy = np.clip(np.concatenate([[y[0], y[-1], y[0], y[-1]], rng.uniform(y[0], y[-1], 60)]).astype(dt), y[0], y[-1])
    f_both_ways(F, qx, qy, f_rows(x, y, nodes, got, qx, qy), "F")
    r = rectangles(qx, qy, rng)
    r[0][3], r[1][3], r[2][3], r[3][3] = x[0], x[-1], y[0], y[-1]
    rect_both_ways(F, r, r_rows(x, y, nodes, got, r), "rectangles")


# ---- F and rectangle rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("even", [False, True], ids=["uneven", "even"])
@pytest.mark.parametrize("shape", [(5, 7, 3), (9, 6, 8)], ids=["5x7x3-scalar", "9x6x8-vectors"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_rows_on_the_hostile_queries(pkg, capfd, dt, shape, even):
    """Every node, the last knots, one ulp either side of every grid line, midpoints, 300 random points
    (tests/hostile_inputs.py, bicubic_queries), as F queries and as corners of rectangles."""
    nx, ny, Cn = shape
    rng = np.random.default_rng(nx * 100 + ny + even)
    x = np.arange(nx).astype(dt) if even else uneven(rng, nx, dt)
    y = (np.arange(ny) * 0.5).astype(dt) if even else uneven(rng, ny, dt)
    z = rng.normal(size=shape).astype(dt)
    it, F, nodes, tabs = setup(pkg, x, y, z)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=300)
    vec = int(Cn % vn(dt) == 0)
    fields = dict(vec=vec, lv=Cn // vn(dt) if vec else Cn, klds=1, gy=1)
    f_both_ways(F, qx, qy, f_rows(x, y, nodes, tabs, qx, qy), "F", capfd, **fields)
    r = rectangles(qx, qy, rng)
    want = r_rows(x, y, nodes, tabs, r)
    assert np.all(want[:3] == 0) and np.any(want[3:] > 0) and np.any(want[3:] < 0)       # degenerate; both signs
    rect_both_ways(F, r, want, "rectangles", capfd, **fields)
    neg, nz = F.integral(r[1], r[0], r[2], r[3]), want != 0
    check_bits(neg[nz], -want[nz], "x bounds exchanged: the exact negative")
    assert np.all(neg[~nz] == 0)                              # (d - d is +0 either way round)
    # broadcasting: one rectangle against a (2, 3) block of upper corners, shape ++ trailing data shape
    got = F.integral(x[0], r[1][:6].reshape(2, 3), y[0], r[3][:6].reshape(2, 3))
    assert got.shape == (2, 3, Cn)
    full = np.broadcast_to
    check_bits(got.reshape(6, Cn), r_rows(x, y, nodes, tabs, (full(x[0], 6), r[1][:6], full(y[0], 6), r[3][:6])), "broadcast")


@pytest.fixture(scope="module", params=DTYPES, ids=DT_IDS)
def wide(pkg, request):
    """4 x 5 x (VN * 65), 65 queries (a wave's second batch of one query): one grid, handles on slices of its lanes"""
    dt = request.param
    rng = np.random.default_rng(65)
    x, y = uneven(rng, 4, dt), uneven(rng, 5, dt)
    z = rng.normal(size=(4, 5, vn(dt) * 65)).astype(dt)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=0)
    pick = rng.permutation(len(qx))[:65]
    return dict(dt=dt, x=x, y=y, z=z, qx=qx[pick], qy=qy[pick], r=rectangles(qx[pick], qy[pick], rng))


@pytest.mark.parametrize("lv", [1, 2, 63, 64, 65])
def test_row_lengths(pkg, capfd, wide, lv):
    """lv vectors per row: 1 (no division), 2 and 63 (the magic division, several queries per trip), 64 (one full trip per
    query), 65 (a trip and a tail) -- in the vector form at lanes = VN * lv and, where the lanes do not divide, the scalar
    form at lanes = lv.  65 queries; then the empty batch."""
    dt, x, y = wide["dt"], wide["x"], wide["y"]
    for Cn, vec in ((vn(dt) * lv, 1), (lv, 0)):
        if not vec and lv % vn(dt) == 0:
            continue
        z = np.ascontiguousarray(wide["z"][:, :, :Cn])
        it, F, nodes, tabs = setup(pkg, x, y, z)
        fields = dict(vec=vec, lv=lv, gy=1, klds=1)
        f_both_ways(F, wide["qx"], wide["qy"], f_rows(x, y, nodes, tabs, wide["qx"], wide["qy"]), f"F lv={lv} vec={vec}", capfd, **fields)
        rect_both_ways(F, wide["r"], r_rows(x, y, nodes, tabs, wide["r"]), f"rect lv={lv} vec={vec}", capfd, **fields)
        e = np.empty(0, dt)
        assert F.interp_array(e, e).shape == (0, Cn) and F.integral(e, e, e, e).shape == (0, Cn)
        assert tuple(F.integral(dev(e), dev(e), dev(e), dev(e)).shape) == (0, Cn)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_row_cut_into_pieces_and_caller_owned_buffers(pkg, capfd, dt):
    """3 x 3 x 513, scalar lanes: two pieces along blockIdx.y, the second of one element; fresh outputs (the kernel's own
    range test) and caller-owned ones (the pre-pass), contiguous, strided and offset by one element"""
    rng = np.random.default_rng(513)
    x, y = uneven(rng, 3, dt), uneven(rng, 3, dt)
    z = rng.normal(size=(3, 3, 513)).astype(dt)
    it, F, nodes, tabs = setup(pkg, x, y, z)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=20)
    nq = len(qx)
    r = rectangles(qx, qy, rng)
    wf, wr = f_rows(x, y, nodes, tabs, qx, qy), r_rows(x, y, nodes, tabs, r)
    check_bits(to_np(traced(capfd, lambda: F.interp_array(dev(qx), dev(qy)), "F", rect=0, vec=0, lv=513, gy=2, prepass=0)), wf, "F pieces")
    check_bits(to_np(traced(capfd, lambda: F.integral(*[dev(b) for b in r]), "rect", rect=1, vec=0, lv=513, gy=2, prepass=0)), wr,
               "rect pieces")
    for on_device in (True, False):
        q = [dev(b) for b in r] if on_device else list(r)
        buf = sentinel_buffer((nq, 513), dt, on_device)
        traced(capfd, lambda: F.strategy.integral(*q, buf), "rect into", rect=1, vec=0, lv=513, gy=2, prepass=1)
        check_bits(to_np(buf), wr, f"rect, caller-owned buffer, device={on_device}")
    for name, stride, base in (("lanes + 3", 516, 0), ("base + 1", 513, 1)):
        flat = sentinel_buffer((nq * stride + base + 1,), dt, True)
        view = flat[base:base + nq * stride].view(nq, stride)[:, :513]
        for call, want in ((lambda: F.strategy.integral(*[dev(b) for b in r], view), wr),
                           (lambda: F.strategy.interp_array_into(F, dev(qx), dev(qy), view), wf)):
            flat.fill_(SENTINEL)
            call()
            h = to_np(flat)
            check_bits(h[base:base + nq * stride].reshape(nq, stride)[:, :513], want, name)
            gaps = np.ones(h.shape, bool)
            gaps[base:base + nq * stride].reshape(nq, stride)[:, :513] = False
            assert np.all(h[gaps] == SENTINEL), f"{name}: gap elements were written"
    host = np.full((nq, 520), SENTINEL, dt)                   # strided host rows
    F.strategy.integral(*r, host[:, :513])
    check_bits(host[:, :513], wr, "strided host rows")
    assert np.all(host[:, 513:] == SENTINEL)


def test_knots_in_global_memory(pkg, capfd):
    """17 880 x 3 x 1 f64: one knot past what fits LDS beside the value kernel's strips (tests/test_gpu_bicubic_plans.py
    derives the number; the integral's strips are no smaller): the searches read the knots from global memory"""
    rng = np.random.default_rng(17_880)
    x, y = uneven(rng, 17_880, np.float64), uneven(rng, 3, np.float64)
    z = rng.normal(size=(17_880, 3, 1))
    it, F, nodes, tabs = setup(pkg, x, y, z)
    near = np.concatenate([x[:40], np.nextafter(x[1:40], -np.inf), x[-40:], np.nextafter(x[-40:], -np.inf)])
    qx = np.concatenate([near, rng.uniform(x[0], x[-1], 2000)])
    qy = np.clip(np.resize(np.concatenate([y, np.nextafter(y, -np.inf), np.nextafter(y, np.inf)]), len(qx)), y[0], y[-1])
    f_both_ways(F, qx, qy, f_rows(x, y, nodes, tabs, qx, qy), "F, global knots", capfd, klds=0, vec=0, lv=1)
    r = rectangles(qx, qy, rng)
    rect_both_ways(F, r, r_rows(x, y, nodes, tabs, r), "rect, global knots", capfd, klds=0, vec=0, lv=1)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_extrapolation_continues_the_end_cells(pkg, dt):
    rng = np.random.default_rng(3)
    x, y, z = make_grid(rng, 9, 7, 3, dt)
    it, F, nodes, tabs = setup(pkg, x, y, z, extrapolate=True)
    wx, wy = x[-1] - x[0], y[-1] - y[0]
    qx = rng.uniform(x[0] - wx, x[-1] + wx, 1000).astype(dt)
    qy = rng.uniform(y[0] - wy, y[-1] + wy, 1000).astype(dt)
    qx[:8] = [x[0] - wx, x[0] - wx, x[-1] + wx, x[-1] + wx, x[0] - wx, x[-1] + wx, x[3], x[4]]      # corners, sides
    qy[:8] = [y[0] - wy, y[-1] + wy, y[0] - wy, y[-1] + wy, y[2], y[3], y[0] - wy, y[-1] + wy]
    assert np.any(qx < x[0]) and np.any(qx > x[-1]) and np.any(qy < y[0]) and np.any(qy > y[-1])
    f_both_ways(F, qx, qy, f_rows(x, y, nodes, tabs, qx, qy), "F, extrapolate")
    r = rectangles(qx, qy, rng)
    rect_both_ways(F, r, r_rows(x, y, nodes, tabs, r), "rect, extrapolate")
    nan = np.array([x[1], np.nan], dt)
    ok = np.array([x[1], x[2]], dt)
    with pytest.raises(pkg.Panic, match="NaN") as e:
        F.interp_array(nan, np.array([y[1], y[1]], dt))
    assert e.value.index == 1
    for k in range(4):                                        # NaN in each bound: the search's failure, query 1
        b = [ok.copy() for _ in range(4)]
        b[k] = nan
        with pytest.raises(pkg.Panic, match="NaN") as e:
            F.integral(*b)
        assert e.value.index == 1, k


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def rect_failure(pkg, F, r, into=None, fresh=False):
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        if into is None:
            F.integral(*r)
        else:
            F.strategy.integral(*r, into, fresh=fresh)
    v = e.value
    return str(v), v.index, v.value, v.axis


def test_out_of_range_bounds_lowest_index_and_precedence(pkg):
    """Without `extrapolate`.  One bad bound at a time: its letter, its value, its index.  Several bad bounds in one
    rectangle: xa before xb before ya before yb.  Two bad rectangles: the lower index, whatever the bound.  Rows before the
    failing index are written; rows from it on keep the sentinel of a caller-owned buffer (with NDI_EVAL_FRESH_OUTPUT they
    are unspecified and not looked at).  NaN is out of range."""
    import torch
    rng = np.random.default_rng(8)
    x, y, z = make_grid(rng, 9, 7, 5, np.float64)
    it, F, nodes, tabs = setup(pkg, x, y, z)
    nq = 300
    good = [rng.uniform(x[0], x[-1], nq), rng.uniform(x[0], x[-1], nq), rng.uniform(y[0], y[-1], nq), rng.uniform(y[0], y[-1], nq)]
    want = r_rows(x, y, nodes, tabs, good)
    bad_of = [x[-1] + 0.25, x[0] - 0.5, y[0] - 0.25, y[-1] + 1.0]
    letter = ["x", "x", "y", "y"]

    def check(r, pos, k):
        v = bad_of[k]
        exp = (f"{letter[k]} = {float(v)!r} is not in range", pos, float(v), k // 2)
        dr = [dev(b) for b in r]
        assert rect_failure(pkg, F, r) == exp and rect_failure(pkg, F, dr) == exp, (pos, k)     # fresh outputs
        for on_device in (False, True):
            for fresh in (False, True):
                buf = sentinel_buffer((nq, 5), np.float64, on_device)
                assert rect_failure(pkg, F, dr if on_device else r, into=buf, fresh=fresh) == exp, (pos, k, on_device, fresh)
                rows = to_np(buf)
                check_bits(rows[:pos], want[:pos], "rows before the failure")
                if not fresh:
                    assert np.all(rows[pos:] == SENTINEL), "rows from the failure on keep the sentinel"

    for pos in (0, 131, nq - 1):
        for k in range(4):                                    # one bad bound
            r = [b.copy() for b in good]
            r[k][pos] = bad_of[k]
            if pos + 7 < nq:
                r[(k + 1) % 4][pos + 7] = np.nan              # a later failure must not be the one reported
            check(r, pos, k)
    for ks in ((0, 1, 2, 3), (1, 2, 3), (2, 3), (1, 3), (0, 3)):   # several in one rectangle: the first in the order wins
        r = [b.copy() for b in good]
        for k in ks:
            r[k][77] = bad_of[k]
        check(r, 77, ks[0])
    r = [b.copy() for b in good]                              # yb fails at 40, xa at 41: the lower index wins
    r[3][40], r[0][41] = bad_of[3], bad_of[0]
    check(r, 40, 3)
    r = [b.copy() for b in good]
    r[2][200] = np.nan                                        # NaN without extrapolation: "is not in range"
    msg, index, value, axis = rect_failure(pkg, F, r)
    assert msg == "y = NaN is not in range" and index == 200 and axis == 1 and np.isnan(value)
    check_bits(F.integral(*good), want, "the handle evaluates after the failures")
    # finish() after a failing async batch of F
    qx, qy = good[0].copy(), good[2].copy()
    qx[150] = x[-1] + 2.0
    out = torch.full((nq, 5), SENTINEL, dtype=torch.float64, device="cuda:0")
    dqx, dqy = dev(qx), dev(qy)
    F.interp_array_into(dqx, dqy, out, async_launch=True)
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        F.strategy.finish()
    assert e.value.index == 150 and e.value.axis == 0
    rows = to_np(out)
    check_bits(rows[:150], f_rows(x, y, nodes, tabs, qx[:150], qy[:150]), "async: rows before the failure")
    assert np.all(rows[150:] == SENTINEL)


# ---- the life of the handles ----------------------------------------------------------------------------------------------------
def test_either_handle_may_go_first_and_the_node_table_is_shared(pkg):
    """512 x 256 x 4 f64: a grid of 4 MiB, a node table of 16 MiB.  The integral handle costs its five prefix tables and two
    knot axes, not a copy of the node table: less than 7 grids (a copy would make it 9)."""
    import torch
    rng = np.random.default_rng(512)
    x, y = uneven(rng, 512, np.float64), uneven(rng, 256, np.float64)
    z = rng.normal(size=(512, 256, 4))
    it = build(pkg, x, y, z)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    F = it.antiderivative()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    print(f"the integral handle took {free0 - free1} bytes of device memory; one grid is {z.nbytes}")
    assert 5 * z.nbytes <= free0 - free1 < 7 * z.nbytes, (free0 - free1, z.nbytes)
    nodes, tabs = (z,) + tuple(it.strategy.tables()), F.strategy.integral_tables()
    qx, qy = rng.uniform(x[0], x[-1], 500), rng.uniform(y[0], y[-1], 500)
    r = rectangles(qx, qy, rng)
    wf, wr = f_rows(x, y, nodes, tabs, qx, qy), r_rows(x, y, nodes, tabs, r)
    G = it.antiderivative()                                   # a second integral of the same surface
    it.strategy.release()                                     # the source goes first
    f_both_ways(F, qx, qy, wf, "F after the source is gone")
    rect_both_ways(F, r, wr, "rect after the source is gone")
    F.strategy.release()
    rect_both_ways(G, r, wr, "the second integral after both are gone")
    G.strategy.release()
    it2 = build(pkg, x, y, z)                                 # the other way round
    F2 = it2.antiderivative()
    F2.strategy.release()
    check_bits(it2.interp_array(qx, qy), bicubic_ref.evaluate(x, y, *nodes, qx, qy), "the surface after its integral is gone")


def test_clone_ring_sharded_trim_and_refusals(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    rng = np.random.default_rng(33)
    x, y, z = make_grid(rng, 33, 20, 5, np.float64)
    it, F, nodes, tabs = setup(pkg, x, y, z)
    nq = 2007
    qx, qy = rng.uniform(x[0], x[-1], nq), rng.uniform(y[0], y[-1], nq)
    r = rectangles(qx, qy, rng)
    wf, wr = f_rows(x, y, nodes, tabs, qx, qy), r_rows(x, y, nodes, tabs, r)
    dqx, dqy = dev(qx), dev(qy)
    rep = F.replicate([0])[0]                                 # clone: the tables copied, the flag kept
    assert rep.strategy.is_integral and rep.strategy._h.value != F.strategy._h.value
    for a, b in zip(rep.strategy.integral_tables(), tabs):
        check_bits(a, b, "clone: prefix tables")
    for a, b in zip(rep.strategy.tables(), nodes[1:]):
        check_bits(a, b, "clone: node tables")
    check_bits(rep.interp_array(qx, qy), wf, "clone: F")
    check_bits(rep.integral(*r), wr, "clone: rectangles")
    got = np.zeros_like(wf)                                   # ring: two chunks of F
    ring = pkg.striped_ring(1500, 5, 2, np.float64, 0)
    chunks = []

    def consumer(c, rows):
        chunks.append(c.q_count)
        got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
    F.interp_array_ring(dqx, dqy, 1500, consumer, slots=ring)
    assert chunks == [1500, 507]
    check_bits(got, wf, "ring")
    got = np.full_like(wf, -1.0)                              # sharded: two replicas on one device
    pkg.sharding.interp_array_sharded([F, rep], qx, qy, out=got)
    check_bits(got, wf, "sharded")
    for other in (it, it.partial(1, 0)):                      # the integral bit is part of the signature
        with pytest.raises(Exception, match="replicas of one interpolator"):
            pkg.sharding.interp_array_sharded([F, other], qx, qy, out=got)
    F.strategy.trim()
    check_bits(F.integral(*r), wr, "after trim")
    check_bits(F.interp_array(qx, qy), wf, "after trim")
    # refusals, the library's own whatever the mirror knows
    h = C.c_void_p(77)
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    part = it.partial(1, 0)
    for src, text in ((bil, "Bilinear has no antiderivative handle"), (part, "Bicubic: a partial-derivative handle"),
                      (F, "Bicubic: this handle is already an integral handle")):
        assert lib.ndi_interp2d_antiderivative(src.strategy._h, C.byref(h)) == cap.BAD_ARG
        assert cap.last_error().startswith(text) and h.value is None, cap.last_error()
    assert lib.ndi_interp2d_partial(F.strategy._h, 1, 0, C.byref(h)) == cap.BAD_ARG
    assert "y-integral" in cap.last_error() and cap.last_error().startswith("Bicubic") and h.value is None
    out = np.zeros((4, 5))
    b4 = [np.ascontiguousarray(b[:4]) for b in r]
    p4 = [b.ctypes.data for b in b4]
    for src, name in ((bil, "Bilinear"), (it, "Bicubic surface"), (part, "Bicubic partial-derivative")):
        assert lib.ndi_interp2d_integral(src.strategy._h, *p4, 4, out.ctypes.data, 5, None, None) == cap.BAD_ARG
        assert "takes an integral handle" in cap.last_error() and name in cap.last_error(), cap.last_error()
        assert lib.ndi_interp2d_integral_tables(src.strategy._h, out.ctypes.data, None, None, None, None, cap.MEM_HOST) == cap.BAD_ARG
        assert "takes an integral handle" in cap.last_error()
    opts = cap.EvalOpts()
    opts.q_memspace, opts.out_memspace = cap.MEM_HOST, cap.MEM_HOST
    assert lib.ndi_interp2d_integral(F.strategy._h, *p4, 4, out.ctypes.data, 5, C.byref(opts), None) == cap.OK
    check_bits(out, wr[:4], "through the C ABI")
    opts.async_launch = 1
    assert lib.ndi_interp2d_integral(F.strategy._h, *p4, 4, out.ctypes.data, 5, C.byref(opts), None) == cap.UNSUPPORTED
    assert "async_launch" in cap.last_error()
    opts.async_launch, opts.path = 0, cap.PATH_BUCKETED
    assert lib.ndi_interp2d_integral(F.strategy._h, *p4, 4, out.ctypes.data, 5, C.byref(opts), None) == cap.BAD_ARG
    assert "Bicubic has no tile-grouped evaluation form" in cap.last_error()
    assert lib.ndi_interp2d_integral(F.strategy._h, *p4, 4, out.ctypes.data, 4, None, None) == cap.BAD_ARG     # stride < lanes
    F.strategy.path = pkg.PATH_BUCKETED
    with pytest.raises(Exception, match="Bicubic has no tile-grouped evaluation form"):
        F.interp_array(qx, qy)
    F.strategy.path = pkg.PATH_AUTO
    with pytest.raises(ValueError, match="y-integral"):
        F.partial(1, 0)
    with pytest.raises(ValueError, match="already an integral"):
        F.antiderivative()
    with pytest.raises(ValueError, match="partial-derivative strategy"):
        part.antiderivative()
    with pytest.raises(TypeError, match="antiderivative\\(\\) first"):
        it.integral(*r)
    check_bits(F.integral(*r), wr, "the refused handle still evaluates")


# ---- the bounds-checked library --------------------------------------------------------------------------------------------------
def test_compact_pass_under_the_bounds_checked_library():
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import bicubic_integral_ref as ref, test_gpu_bicubic as t\n"
        "import test_gpu_bicubic_integral as ti\n"
        "from hostile_inputs import check_bits\n"
        "pkg = load_product_package(); rng = np.random.default_rng(5)\n"
        "for dt in (np.float32, np.float64):\n"
        "    for (nx, ny), C in (((3, 3), 1), ((5, 7), 3), ((9, 6), 8), ((4, 5), 260), ((3, 3), 513), ((600, 3), 5), ((3, 4354), 2)):\n"
        "        x, y, z = t.make_grid(rng, nx, ny, C, dt)\n"
        "        it, F, nodes, tabs = ti.setup(pkg, x, y, z)\n"
        "        for a, b in zip(tabs, ref.tables(x, y, *nodes)): check_bits(a, b, 'tables')\n"
        "        for nq in (1, 65, 1003):\n"
        "            qx, qy = t.queries(rng, x, y, nq)\n"
        "            r = ti.rectangles(qx, qy, rng)\n"
        "            check_bits(F.interp_array(qx, qy), ti.f_rows(x, y, nodes, tabs, qx, qy), 'F host')\n"
        "            d = F.interp_array(torch.as_tensor(qx, device='cuda:0'), torch.as_tensor(qy, device='cuda:0'))\n"
        "            check_bits(d.cpu().numpy(), ti.f_rows(x, y, nodes, tabs, qx, qy), 'F device')\n"
        "            check_bits(F.integral(*r), ti.r_rows(x, y, nodes, tabs, r), 'rect host')\n"
        "            d = F.integral(*[torch.as_tensor(b, device='cuda:0') for b in r])\n"
        "            check_bits(d.cpu().numpy(), ti.r_rows(x, y, nodes, tabs, r), 'rect device')\n"
        "print('checked OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDI_LIB=lib), timeout=600)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the value and partial paths as they were -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_value_and_partial_paths_are_unchanged(pkg, capfd, dt):
    """A value and a partial evaluated before and after an integral handle exists give the same bits (the restatement's, on
    the same node tables), and the `bicubic` plan line keeps its fields; an integral evaluation prints no such line."""
    for shape in ((5, 7, 3), (9, 6, 8)):
        rng = np.random.default_rng(shape[0])
        x, y, z = make_grid(rng, *shape, dt)
        it = build(pkg, x, y, z)
        p = it.partial(1, 1)
        qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=300)
        before = to_np(it.interp_array(dev(qx), dev(qy))), to_np(p.interp_array(dev(qx), dev(qy)))
        tabs0 = it.strategy.tables()
        F = it.antiderivative()
        _, err = trace(capfd, lambda: F.interp_array(dev(qx), dev(qy)))
        assert len(EVAL.findall(err)) == 1 and not PLAN.findall(err), err[-400:]
        for h, b, order in ((it, before[0], (0, 0)), (p, before[1], (1, 1))):
            rows, err = trace(capfd, lambda: h.interp_array(dev(qx), dev(qy)))
            check_bits(to_np(rows), b, f"order {order} after the integral handle exists")
            assert len(PLAN.findall(err)) == 1 and not EVAL.findall(err) and f"nu={order[0]},{order[1]}\n" in err, err[-400:]
        for a, b in zip(it.strategy.tables(), tabs0):
            check_bits(a, b, "node tables after the integral build")
        with np.errstate(all="ignore"):
            check_bits(before[0], bicubic_ref.evaluate(x, y, z, *tabs0, qx, qy), "the surface itself")
            check_bits(before[1], bicubic_partial_ref.evaluate(x, y, z, *tabs0, qx, qy, 1, 1), "the mixed partial")
