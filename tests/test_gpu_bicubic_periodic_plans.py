"""GPU: every form the Bicubic launch planner (csrc/bicubic_host.hpp, bicubic_launch_eval; csrc/bicubic_jet_host.hpp) can
choose for a handle that WRAPS -- a periodic axis of a handle built with extrapolate -- each against the numpy restatement
of the periodic contract (tests/bicubic_periodic_ref.py) bit for bit AND against the plan line the library prints under
NDI_TRACE_PLAN.  tests/test_gpu_bicubic_plans.py is the pattern; its helpers are imported.  The plan regex here also takes
`nu=a,b` and the trailing ` wrap=x|y|xy`, and every run asserts the wrap field, so no case can silently fall back to the
instance that does not wrap (hence a tracer of this file's own: the other file's parses with its regex):

  knots in global memory (the KLDS = false WRAP instances, and the periodic build on 20 000 and 40 000 knots), the O(1) index
  guess on a wrapping axis, a wrapped coordinate one ulp past the last knot, one- and two-level pyramids, every short-row
  width class, long rows cut along blockIdx.y with the first-error rule across pieces, a wave's second batch, strided and
  misaligned caller buffers, the empty batch, and the eight partial handles and the jet across those forms.

The queries are hostile_inputs.bicubic_wrap_axis_queries on a wrapping axis: one ulp outside either end, whole periods out
to 2^20, a tiny negative remainder, +-max.  No wrapped coordinate of them is NaN, so every expected row is finite, which is
asserted before every comparison: NaN on both sides cannot pass for agreement."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bicubic_partial_ref
import bicubic_periodic_ref as ref
import hostile_inputs as hostile
from conftest import ROOT
from hostile_inputs import check_bits
from test_gpu_bicubic_periodic import build, check_seam, ends_for, failure
from test_gpu_bicubic_plans import (GLOBAL_SHAPES, SENTINEL, SLICES_145, dev, expect_plan, guess_axes, guess_of, near,
                                    sentinel_buffer, to_np, uneven, vn)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
PLAN = re.compile(r"\[ndi plan\] bicubic vec=(\d+) lv=(\d+) klds=(\d+) grid=(\d+) x (\d+) lds=(\d+) prepass=(\d+) "
                  r"guess=(\d+),(\d+) levels=(\d+),(\d+) nu=(\d+),(\d+)(?: wrap=(xy|x|y))?\n")
FIELDS = ("vec", "lv", "klds", "gx", "gy", "lds", "prepass", "guess_x", "guess_y", "levels_x", "levels_y", "nu_x", "nu_y", "wrap")
JET = re.compile(r"\[ndi plan\] bicubic_jet order=(\d) vec=(\d+) lv=(\d+) klds=(\d+) grid=(\d+) x (\d+) lds=(\d+) prepass=(\d+)"
                 r"(?: wrap=(xy|x|y))?\n")
JET_FIELDS = ("order", "vec", "lv", "klds", "gx", "gy", "lds", "prepass", "wrap")
WRAP = {1: "x", 2: "y", 3: "xy"}
ORDERS = bicubic_partial_ref.ORDERS
JET_PARTS = {1: ((0, 0), (1, 0), (0, 1)), 2: ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))}


def wtraced(capfd, call, jet=False):
    """(result, plans): the call under NDI_TRACE_PLAN and the fields of every Bicubic (or jet) plan line it printed, `wrap`
    as text ("" for a line without the field).  `capfd` None (the child process of the last test): the call alone."""
    if capfd is None:
        return call(), []
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
    err = capfd.readouterr().err
    rx, names = (JET, JET_FIELDS) if jet else (PLAN, FIELDS)
    plans = [{k: (v or "") if k == "wrap" else int(v) for k, v in zip(names, m.groups())} for m in rx.finditer(err)]
    assert plans, f"no {'jet' if jet else 'Bicubic'} plan line in: {err[-500:]}"
    if jet:
        assert "[ndi plan] bicubic vec=" not in err, "a jet call launched the value kernel"
    return r, plans


def wrap_sweep(rng, x, y, axes, n_random):
    """On a wrapping axis the hostile set of hostile_inputs.bicubic_wrap_axis_queries and draws up to 3.5 periods outside;
    on the other axis every knot and its neighbours (clipped into range) and draws up to one width outside (the handle
    extrapolates there).  Each axis' set in turn, the other coordinate walking through its own, then the draws."""
    def one(k, wraps):
        p = float(k[-1]) - float(k[0])
        out = 3.5 * p if wraps else p
        return (hostile.bicubic_wrap_axis_queries(k) if wraps else near(k)), rng.uniform(k[0] - out, k[-1] + out, n_random)
    (sx, rx), (sy, ry) = one(x, axes & 1), one(y, axes & 2)
    qx = np.concatenate([sx, np.resize(sx, len(sy)), rx]).astype(x.dtype)
    qy = np.concatenate([np.resize(sy, len(sx)), sy, ry]).astype(y.dtype)
    return qx, qy


def run_all(it, qx, qy, want, capfd, what, axes, nu=(0, 0), fresh_device=None, **fields):
    """host and device queries x fresh output and caller-owned buffer: bits, and `fields`, the orders and the wrap field in
    every launch's plan.  A caller-owned buffer is where the range pre-pass of a wrapping handle runs."""
    assert np.isfinite(want).all(), f"{what}: the expected rows of a finite lane are finite"
    fields = dict(fields, wrap=WRAP[axes], nu_x=nu[0], nu_y=nu[1])
    C = want.shape[1]
    plans = []
    for on_device in (False, True):
        q = (dev(qx), dev(qy)) if on_device else (qx, qy)
        rows, plans = wtraced(capfd, lambda: it.interp_array(*q))
        more = fresh_device if on_device and fresh_device else {}
        expect_plan(plans, f"{what} fresh device={on_device}", **fields, **more)
        check_bits(to_np(rows), want, f"{what} fresh device={on_device}")
        buf = sentinel_buffer((len(qx), C), want.dtype, on_device)
        _, plans = wtraced(capfd, lambda: it.interp_array_into(*q, buf))
        expect_plan(plans, f"{what} into device={on_device}", **fields, **(dict(prepass=1) if on_device else {}))
        check_bits(to_np(buf), want, f"{what} into device={on_device}")
    return plans[-1] if plans else None


def run_unaligned(it, qx, qy, want, capfd, what, axes, **fields):
    """a caller-owned device buffer whose base is one element past a 16-byte boundary: the scalar form at any width"""
    assert np.isfinite(want).all(), what
    nq, C = want.shape
    flat = sentinel_buffer((nq * C + 2,), want.dtype, True)
    view = flat[1:1 + nq * C].view(nq, C)
    _, plans = wtraced(capfd, lambda: it.strategy.interp_array_into(it, dev(qx), dev(qy), view))
    expect_plan(plans, what, vec=0, lv=C, wrap=WRAP[axes], **fields)
    h = to_np(flat)
    check_bits(h[1:1 + nq * C].reshape(nq, C), want, what)
    assert h[0] == SENTINEL and h[-1] == SENTINEL, f"{what}: the elements around the buffer were written"


def run_jet(it, want6, qx, qy, capfd, what, axes, **fields):
    """Orders 1 and 2 through `jet` (fresh parts) and `jet_into` (device parts, host parts, strided device parts), each part
    against the restatement's partial, the wrap suffix in every jet plan line.  `want6`: the six parts of order 2."""
    dt = want6[0].dtype
    nq, C = want6[0].shape
    V = vn(dt)
    fields = dict(fields, wrap=WRAP[axes])
    for order in (1, 2):
        nus = JET_PARTS[order]
        K = len(nus)
        assert all(np.isfinite(w).all() for w in want6[:K]), what
        for on_device in (False, True):
            q = (dev(qx), dev(qy)) if on_device else (qx, qy)
            tag = f"{what} order {order} device={on_device}"
            got, plans = wtraced(capfd, lambda: it.jet(*q, order), jet=True)
            expect_plan(plans, tag, order=order, **fields, **(dict(prepass=0) if on_device else {}))
            assert len(got) == K
            for g, w, nu in zip(got, want6, nus):
                check_bits(to_np(g), w, f"{tag}: jet, part {nu}")
            bufs = [sentinel_buffer((nq, C), dt, on_device) for _ in nus]
            _, plans = wtraced(capfd, lambda: it.jet_into(*q, bufs), jet=True)
            expect_plan(plans, tag, order=order, **fields, **(dict(prepass=1) if on_device else {}))
            for b, w, nu in zip(bufs, want6, nus):
                check_bits(to_np(b), w, f"{tag}: jet_into, part {nu}")
        stride = C + V                                         # strided device parts: planar, rows of lanes + VN
        flat = sentinel_buffer((K * nq * stride + 1,), dt, True)
        parts = [flat[:K * nq * stride].view(K, nq, stride)[k][:, :C] for k in range(K)]
        _, plans = wtraced(capfd, lambda: it.strategy.jet_into(dev(qx), dev(qy), parts), jet=True)
        expect_plan(plans, f"{what} order {order} strided", order=order, prepass=1, **fields)
        h = to_np(flat)
        body = h[:K * nq * stride].reshape(K, nq, stride)
        for k, nu in enumerate(nus):
            check_bits(body[k][:, :C], want6[k], f"{what} order {order} strided: part {nu}")
        assert np.all(body[:, :, C:] == SENTINEL) and h[-1] == SENTINEL, f"{what} order {order} strided: gap elements were written"


class WideP:
    """One wide grid, periodic along `axes`, and the restatement's tables; `handle(lo, hi)` builds with extrapolate (so it
    wraps on `axes`) on the lanes lo..hi and holds the device's tables to the restatement's and the seam to itself; `rows` /
    `part` evaluate once for all lanes."""

    def __init__(self, pkg, rng, x, y, C, axes, mixed=False):
        self.pkg, self.x, self.y, self.axes = pkg, x, y, axes
        self.bc = ends_for(axes, mixed)
        self.z = ref.make_periodic(rng.normal(size=(len(x), len(y), C)).astype(x.dtype), axes)
        with np.errstate(all="ignore"):
            self.tabs = ref.tables(x, y, self.z, self.bc, axes)

    def handle(self, lo, hi, what):
        it = build(self.pkg, self.x, self.y, np.ascontiguousarray(self.z[:, :, lo:hi]), self.axes, self.bc, extrapolate=True)
        got = it.strategy.tables()
        for name, g, r in zip(("zx", "zy", "zxy"), got, self.tabs):
            check_bits(g, r[:, :, lo:hi], f"{what} lanes {lo}:{hi} {name}")
        check_seam(got, self.axes, f"{what} lanes {lo}:{hi}")
        assert it.strategy.wraps == self.axes
        return it

    def part(self, qx, qy, nu=(0, 0)):
        with np.errstate(all="ignore"):
            if tuple(nu) == (0, 0):
                rows = ref.evaluate(self.x, self.y, self.z, *self.tabs, qx, qy, self.axes)
            else:
                rows = ref.evaluate_partial(self.x, self.y, self.z, *self.tabs, qx, qy, nu[0], nu[1], self.axes)
        assert np.isfinite(rows).all(), f"partial {nu}: every wrapped coordinate is finite, so every row is"
        return rows

    rows = part


def form_of(C, dt):
    vec = int(C % vn(dt) == 0)
    return dict(vec=vec, lv=C // vn(dt) if vec else C)


# ---- knots in global memory -------------------------------------------------------------------------------------------------
GLOBAL_CASES = [(dt, nx, ny, "xy") for dt, nx, ny in GLOBAL_SHAPES] + [(np.float64, 20_000, 3, "y"), (np.float32, 5, 40_000, "x")]


def run_global(pkg, capfd, dt, nx, ny, axes, even, slices=SLICES_145, n_random=2000, thin=1):
    rng = np.random.default_rng(nx * 7 + ny + axes)
    mk = (lambda n: np.arange(n).astype(dt)) if even else (lambda n: uneven(rng, n, dt))
    w = WideP(pkg, rng, mk(nx), mk(ny), 10, axes)
    qx, qy = wrap_sweep(rng, w.x, w.y, axes, n_random)
    qx, qy = qx[::thin], qy[::thin]                     # (thin > 1: the run under the bounds-checked library)
    want = w.rows(qx, qy)
    for lo, hi in slices:
        it = w.handle(lo, hi, "global knots")
        run_all(it, qx, qy, want[:, lo:hi], capfd, f"global knots {nx}x{ny} C={hi - lo} even={even} wrap={WRAP[axes]}", axes, klds=0,
                guess_x=int(even), guess_y=int(even), levels_x=1 + (nx > 64), levels_y=1 + (ny > 64), **form_of(hi - lo, dt))
    return w, qx, qy


@pytest.mark.parametrize("even", [False, True], ids=["uneven", "even"])
@pytest.mark.parametrize("dt,nx,ny,axes", GLOBAL_CASES, ids=[f"{np.dtype(s[0]).name}-{s[1]}x{s[2]}-p{s[3]}" for s in GLOBAL_CASES])
def test_knots_in_global_memory(pkg, capfd, dt, nx, ny, axes, even):
    """The pyramids and the strips pass the LDS limit: the KLDS = false WRAP instances, whose search reads `const T*`, with the
    guess (exactly even knots) and without; and the periodic build with its seam on 20 000 and 40 000 knots.  Periodic on
    both axes, and on the short axis alone (the long axis' search then meets extrapolated coordinates)."""
    run_global(pkg, capfd, dt, nx, ny, hostile.PERIODIC_AXES[axes], even)


# ---- the index guess on a wrapping axis ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("n", [3, 64, 65, 1000])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_index_guess_on_a_wrapping_axis(pkg, capfd, dt, n, axis):
    """guess_axes of the plans file on the periodic axis, which wraps: the guess of locate_index is formed from the WRAPPED
    coordinate, accepted and rejected."""
    rng = np.random.default_rng(n + axis)
    other = uneven(rng, 4, dt)
    axes = 1 << axis
    for name, k in guess_axes(n, dt):
        assert np.all(k[1:] > k[:-1]) and guess_of(k) == 1
        x, y = (k, other) if axis == 0 else (other, k)
        w = WideP(pkg, rng, x, y, 5, axes)
        qx, qy = wrap_sweep(rng, x, y, axes, 3000)
        want = w.rows(qx, qy)
        for lo, hi in ((0, 1), (1, 5)):
            it = w.handle(lo, hi, f"guess {name}")
            run_all(it, qx, qy, want[:, lo:hi], capfd, f"guess {name} n={n} axis={axis} C={hi - lo}", axes, klds=1,
                    guess_x=int(axis == 0), guess_y=int(axis == 1), vec=int(hi - lo == 4))


# ---- a wrapped coordinate past the last knot ----------------------------------------------------------------------------------
def past_end_axis(rng, n, dt, even):
    """k0 = -10 / 7, kn = 3 (f32) or 1 (f64): fl(fl(kn - k0) + k0) is one ulp above kn, and nextafter(k0, -inf) wraps to it.
    Evenly spaced with both ends set exactly, or with uneven interior knots."""
    T = np.dtype(dt).type
    k0, kn = T(-10) / T(7), T(3 if np.dtype(dt) == np.float32 else 1)
    while True:
        f = np.arange(n) / (n - 1) if even else np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, n - 1))])
        k = (float(k0) + (float(kn) - float(k0)) * f / f[-1]).astype(dt)
        k[0], k[-1] = k0, kn
        if np.all(k[1:] > k[:-1]) and guess_of(k) == int(even):
            return k


def run_past_end(pkg, capfd, dt, n, even, axis, partials=True):
    T = np.dtype(dt).type
    rng = np.random.default_rng(n * 4 + 2 * even + axis)
    k, other = past_end_axis(rng, n, dt, even), uneven(rng, 4, dt)
    assert T((k[-1] - k[0]) + k[0]) == np.nextafter(k[-1], T(np.inf))
    axes = 1 << axis
    x, y = (k, other) if axis == 0 else (other, k)
    w = WideP(pkg, rng, x, y, 5, axes)
    qx, qy = wrap_sweep(rng, x, y, axes, 300)
    past = ref.wrap(k, (qx, qy)[axis]) > k[-1]
    assert past.any() and not np.isnan(ref.wrap(k, (qx, qy)[axis])).any(), "the case is about a wrapped coordinate past kn"
    want = {nu: w.part(qx, qy, nu) for nu in ((0, 0),) + ORDERS}
    g = {"guess_x" if axis == 0 else "guess_y": int(even)}
    for lo, hi in ((0, 1), (1, 5)):
        what = f"past the end n={n} even={even} axis={axis} C={hi - lo}"
        it = w.handle(lo, hi, what)
        run_all(it, qx, qy, want[0, 0][:, lo:hi], capfd, what, axes, klds=1, **g, **form_of(hi - lo, dt))
        if partials:
            for nu in ORDERS:
                run_all(it.partial(*nu), qx, qy, want[nu][:, lo:hi], capfd, f"{what} partial {nu}", axes, nu=nu, klds=1, **g,
                        **form_of(hi - lo, dt))
        run_jet(it, [want[nu][:, lo:hi] for nu in JET_PARTS[2]], qx, qy, capfd, what, axes, klds=1, **form_of(hi - lo, dt))
    return int(past.sum())


@pytest.mark.parametrize("even", [True, False], ids=["even", "uneven"])
@pytest.mark.parametrize("n", [3, 8, 65, 1000])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_wrapped_coordinate_past_the_last_knot(pkg, capfd, dt, n, even):
    """fl(r + k0) can land one ulp past kn; the search clamps to the last cell and t is just over 1.  With the
    guess (even) and through the search (uneven), the surface, the eight partial handles and the jet, on each axis."""
    for axis in (0, 1):
        assert run_past_end(pkg, capfd, dt, n, even, axis) >= 1


# ---- pyramid levels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("n", [64, 65, 129, 4097])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_pyramid_levels_on_a_wrapping_axis(pkg, capfd, dt, n, axis):
    """one level (64), a second level with a last block of one knot (65: blocks of 2; 129: of 4; 4097: of 128)"""
    rng = np.random.default_rng(n * 2 + axis)
    k, other = uneven(rng, n, dt), uneven(rng, 3, dt)
    axes = 1 << axis
    x, y = (k, other) if axis == 0 else (other, k)
    w = WideP(pkg, rng, x, y, 5, axes)
    qx, qy = wrap_sweep(rng, x, y, axes, 500)
    want = w.rows(qx, qy)
    lv = {"levels_x" if axis == 0 else "levels_y": 1 if n <= 64 else 2, "levels_y" if axis == 0 else "levels_x": 1}
    for lo, hi in ((0, 1), (1, 5)):
        it = w.handle(lo, hi, "levels")
        run_all(it, qx, qy, want[:, lo:hi], capfd, f"levels n={n} axis={axis} C={hi - lo}", axes, klds=1, guess_x=0, guess_y=0,
                vec=int(hi - lo == 4), **lv)


# ---- short and long rows ------------------------------------------------------------------------------------------------------
SHORT_LANES = list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130]
LONG_LV = [64, 65, 513, 1025]


def small_grid(pkg, dt, C):
    """4 x 5 x C periodic on both axes and 200 hostile queries in a seeded order: the first 130 are the short rows' two waves"""
    rng = np.random.default_rng(1025)
    w = WideP(pkg, rng, uneven(rng, 4, dt), uneven(rng, 5, dt), C, 3)
    qx, qy = wrap_sweep(rng, w.x, w.y, 3, 63)
    assert len(qx) == 200
    order = rng.permutation(200)
    return w, qx[order], qy[order]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_short_rows(pkg, capfd, dt):
    """130 queries (two waves, the second partial).  Aligned buffers give the vector form wherever the lanes divide; a
    misaligned caller buffer runs those widths through the scalar form as well."""
    w, qx, qy = small_grid(pkg, dt, 130)
    qx, qy = qx[:130], qy[:130]
    want = w.rows(qx, qy)
    for C in SHORT_LANES:
        it = w.handle(0, C, "short rows")
        run_all(it, qx, qy, want[:, :C], capfd, f"short rows C={C}", 3, gx=1, gy=1, klds=1, **form_of(C, dt))
        if C % vn(dt) == 0:
            run_unaligned(it, qx, qy, want[:, :C], capfd, f"short rows C={C} unaligned", 3, gx=1, gy=1)


def make_long(pkg, dt):
    w, qx, qy = small_grid(pkg, dt, vn(dt) * 1025)
    return dict(dt=dt, w=w, qx=qx, qy=qy, want=w.rows(qx, qy))


@pytest.fixture(scope="module", params=DTYPES, ids=DT_IDS)
def long_rows(pkg, request):
    """4 x 5 x (VN * 1025), periodic on both axes, and 200 queries: the restatement once per dtype"""
    return make_long(pkg, request.param)


def run_long(pkg, capfd, lr, lv, nqs=(1, 65, 200)):
    dt, w = lr["dt"], lr["w"]
    gy = -(-lv // 512)
    for C, vec in ((vn(dt) * lv, 1), (lv, 0)):
        it = w.handle(0, C, f"long rows lv={lv}")
        for nq in nqs:
            qx, qy, want = lr["qx"][:nq], lr["qy"][:nq], lr["want"][:nq, :C]
            what = f"long rows lv={lv} vec={vec} nq={nq}"
            if vec or lv % 2:
                # a fresh device output is checked in the kernel, on the wrapped coordinates, by the piece blockIdx.y == 0 alone
                run_all(it, qx, qy, want, capfd, what, 3, fresh_device=dict(prepass=0) if gy > 1 else None,
                        vec=vec, lv=lv, gx=1, gy=gy, klds=1)
            else:
                run_unaligned(it, qx, qy, want, capfd, what, 3, gx=1, gy=gy, klds=1)


@pytest.mark.parametrize("lv", LONG_LV)
def test_long_rows_and_pieces_along_y(pkg, capfd, long_rows, lv):
    """lv >= 64: one query at a time; rows of more than 512 vectors are cut along blockIdx.y with a last piece of one vector
    (513, 1025).  The vector form at lanes = VN * lv; the scalar form at lanes = lv (even lv: a misaligned caller buffer)."""
    assert -(-lv // 512) == {64: 1, 65: 1, 513: 2, 1025: 3}[lv]
    run_long(pkg, capfd, long_rows, lv)


def periodic_spline_report(pkg, k, col, q):
    """the first-error report of the periodic 1-D CubicSpline with extrapolate on the queries q"""
    one_d = pkg.Interp1DBuilder.new(col).x(k).strategy(
        pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Periodic).extrapolate(True)).build()
    with pytest.raises(Exception) as e:
        one_d.interp_array(q)
    return type(e.value).__name__, str(e.value), e.value.index


@pytest.mark.parametrize("lv", [513, 1025])
def test_first_error_across_pieces(pkg, long_rows, lv):
    """gridDim.y > 1: only blockIdx.y == 0 range-checks a fresh output, and every piece of a caller-owned buffer stops at the
    first failing query.  NaN, +inf and -inf on the wrapping axis (+-inf wraps to NaN), NaN on the other (which
    extrapolates: NaN alone fails there); the report is the periodic 1-D CubicSpline's on the same queries."""
    import torch
    dt, w = long_rows["dt"], long_rows["w"]
    x, y, nq = w.x, w.y, 200
    tdt = torch.float32 if dt == np.float32 else torch.float64
    for C in (vn(dt) * lv, lv):
        z = np.ascontiguousarray(w.z[:, :, :C])
        for axes in (1, 2):
            it = build(pkg, x, y, z, axes, extrapolate=True)
            rng = np.random.default_rng(lv + axes)
            qx0, qy0 = wrap_sweep(rng, x, y, axes, 200)          # (the fixture's queries are hostile on both axes)
            pick = rng.permutation(len(qx0))[:nq]
            qx0, qy0 = qx0[pick], qy0[pick]
            want = ref.evaluate(x, y, z, *it.strategy.tables(), qx0, qy0, axes)
            assert np.isfinite(want).all()
            wa = 0 if axes == 1 else 1
            for axis, bad in ((wa, np.nan), (wa, np.inf), (wa, -np.inf), (1 - wa, np.nan)):
                for pos in (0, nq // 2, nq - 1):
                    qx, qy = qx0.copy(), qy0.copy()
                    (qx, qy)[axis][pos] = bad
                    if pos + 7 < nq:
                        (qx, qy)[1 - axis][pos + 7] = np.nan   # a later failure must not be the one reported
                    what = f"lv={lv} C={C} wrap={WRAP[axes]} {bad} on axis {axis} at {pos}"
                    exp = periodic_spline_report(pkg, x, np.ascontiguousarray(z[:, 0, :1]),
                                                 np.where(np.arange(nq) == pos, dt(bad), qx0))
                    assert exp[0] == "Panic" and exp[2] == pos, what
                    dqx, dqy = dev(qx), dev(qy)
                    assert failure(it, qx, qy)[:3] == exp and failure(it, dqx, dqy)[:3] == exp, what
                    for mk in (lambda: np.full((nq, C), SENTINEL, dt), lambda: torch.full((nq, C), SENTINEL, dtype=tdt, device="cuda:0")):
                        buf = mk()
                        q = (qx, qy) if isinstance(buf, np.ndarray) else (dqx, dqy)
                        assert failure(it, *q, into=buf)[:3] == exp, what
                        rows = to_np(buf)
                        check_bits(rows[:pos], want[:pos], f"{what}: rows before the failure")
                        assert np.all(rows[pos:] == SENTINEL), f"{what}: rows from the failure on keep the sentinel in every piece"


# ---- a wave's second batch ----------------------------------------------------------------------------------------------------
NQ_SECOND = 3 * 2**20 + 71


@pytest.mark.parametrize("C", [1, 4])
def test_second_batch_of_a_wave(pkg, capfd, C):
    """f32 9 x 7, wrapping on both axes, more queries than gridDim.x * 256: waves come round and wrap their second batch.  Then
    +inf on x inside the second batch: the periodic 1-D spline's report, rows before it, the sentinel from it on."""
    import torch
    dt = np.float32
    rng = np.random.default_rng(9 + C)
    w = WideP(pkg, rng, uneven(rng, 9, dt), uneven(rng, 7, dt), C, 3)
    it = w.handle(0, C, "second batch")
    qx, qy = wrap_sweep(rng, w.x, w.y, 3, 0)
    more = wrap_sweep(rng, w.x, w.y, 3, NQ_SECOND - len(qx))
    qx, qy = more[0][-NQ_SECOND:], more[1][-NQ_SECOND:]
    assert len(qx) == NQ_SECOND
    want = w.rows(qx, qy)
    p = run_all(it, qx, qy, want, capfd, f"second batch C={C}", 3, klds=1, gy=1, vec=int(C == 4))
    assert NQ_SECOND > p["gx"] * 256, p
    pos = p["gx"] * 256 + 1000                             # the first error, found by a wave in its second batch
    assert pos + 7 < NQ_SECOND
    qx[pos] = np.inf
    qy[pos + 7] = np.nan
    exp = periodic_spline_report(pkg, w.x, np.ascontiguousarray(w.z[:, 0, :1]), qx)
    assert exp[0] == "Panic" and exp[2] == pos
    dqx, dqy = dev(qx), dev(qy)
    assert failure(it, dqx, dqy)[:3] == exp
    buf = torch.full((NQ_SECOND, C), SENTINEL, dtype=torch.float32, device="cuda:0")
    assert failure(it, dqx, dqy, into=buf)[:3] == exp
    rows = to_np(buf)
    check_bits(rows[:pos], want[:pos], "rows before the failure")
    assert np.all(rows[pos:] == SENTINEL), "rows from the failure on keep the sentinel"


# ---- strided and misaligned caller buffers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 5, 64])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_strided_and_misaligned_buffers(pkg, capfd, dt, C):
    """64 x 48 periodic on both axes, 1000 queries into a view of a larger sentinel-filled buffer: a row stride of lanes + VN
    (the vector form when the lanes divide), of lanes + 1, and of lanes from a base one element in (both scalar).  Every gap
    element keeps the sentinel.  Device views with device queries, and the same strides as host views with host queries."""
    rng = np.random.default_rng(C)
    w = WideP(pkg, rng, uneven(rng, 64, dt), uneven(rng, 48, dt), C, 3)
    it = w.handle(0, C, "strided")
    qx, qy = wrap_sweep(rng, w.x, w.y, 3, 200)
    pick = rng.permutation(len(qx))[:1000]
    qx, qy = qx[pick], qy[pick]
    nq = len(qx)
    assert nq == 1000
    want = w.rows(qx, qy)
    V = vn(dt)
    for name, stride, base, vec in (("lanes + VN", C + V, 0, int(C % V == 0)), ("lanes + 1", C + 1, 0, 0), ("base + 1", C, 1, 0)):
        for on_device in (True, False):
            flat = sentinel_buffer((nq * stride + base + 1,), dt, on_device)
            body = flat[base:base + nq * stride]
            view = (body.view(nq, stride) if on_device else body.reshape(nq, stride))[:, :C]
            q = (dev(qx), dev(qy)) if on_device else (qx, qy)
            _, plans = wtraced(capfd, lambda: it.strategy.interp_array_into(it, *q, view))
            what = f"{name} C={C} device={on_device}"
            expect_plan(plans, what, wrap="xy")
            if on_device:
                expect_plan(plans, what, vec=vec, lv=C // V if vec else C, prepass=1)
            h = to_np(flat)
            check_bits(h[base:base + nq * stride].reshape(nq, stride)[:, :C], want, what)
            gaps = np.ones(h.shape, bool)
            gaps[base:base + nq * stride].reshape(nq, stride)[:, :C] = False
            assert np.all(h[gaps] == SENTINEL), f"{what}: {int((h[gaps] != SENTINEL).sum())} gap elements were written"


# ---- the empty batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_empty_batch(pkg, capfd, dt):
    import torch
    rng = np.random.default_rng(0)
    for C in (1, 4, 5):
        w = WideP(pkg, rng, uneven(rng, 4, dt), uneven(rng, 5, dt), C, 3)
        it = w.handle(0, C, "empty")
        e = np.empty(0, dt)
        rows = it.interp_array(e, e)
        assert rows.shape == (0, C) and rows.dtype == np.dtype(dt)
        rows = it.interp_array(dev(e), dev(e))
        assert tuple(rows.shape) == (0, C)
        it.interp_array_into(e, e, np.empty((0, C), dt))
        it.interp_array_into(dev(e), dev(e), torch.empty((0, C), dtype=rows.dtype, device="cuda:0"))
        for order in (1, 2):
            assert all(tuple(g.shape) == (0, C) for g in it.jet(dev(e), dev(e), order))
        p = float(w.x[-1]) - float(w.x[0])                      # and the handle still evaluates: one query, a period out
        q = np.array([w.x[1] + dt(p)], dt), np.array([w.y[2]], dt)
        rows, plans = wtraced(capfd, lambda: it.interp_array(*q))
        expect_plan(plans, "after the empty batches", wrap="xy", **form_of(C, dt))
        check_bits(rows, w.rows(*q), "after the empty batches")


# ---- partials and the jet across the forms ------------------------------------------------------------------------------------
def run_partials_and_jet(it, w, lo, hi, qx, qy, capfd, what, **fields):
    want = {nu: w.part(qx, qy, nu)[:, lo:hi] for nu in ((0, 0),) + ORDERS}
    for nu in ORDERS:
        part = it.partial(*nu)
        assert part.strategy.wraps == w.axes
        run_all(part, qx, qy, want[nu], capfd, f"{what} partial {nu}", w.axes, nu=nu, **fields)
    run_jet(it, [want[nu] for nu in JET_PARTS[2]], qx, qy, capfd, what, w.axes,
            **{k: v for k, v in fields.items() if k in JET_FIELDS})


def test_partials_and_jet_with_knots_in_global_memory(pkg, capfd):
    """f64 20 000 x 3 periodic on both axes, 4 lanes: the KLDS = false WRAP instances of the eight partial orders and of the jet"""
    dt = np.float64
    rng = np.random.default_rng(20_000)
    w = WideP(pkg, rng, uneven(rng, 20_000, dt), uneven(rng, 3, dt), 4, 3)
    it = w.handle(0, 4, "global knots, partials")
    qx, qy = wrap_sweep(rng, w.x, w.y, 3, 1000)
    pick = np.sort(np.concatenate([np.arange(0, len(qx), 37), np.arange(len(qx) - 1500, len(qx))]))   # every 37th, the far set, the draws
    run_partials_and_jet(it, w, 0, 4, qx[pick], qy[pick], capfd, "global knots", klds=0, vec=1, lv=2, levels_x=2, levels_y=1)


@pytest.mark.parametrize("vec", [1, 0], ids=["vectors", "scalar"])
def test_partials_and_jet_on_rows_cut_into_pieces(pkg, capfd, long_rows, vec):
    """lv = 513: two pieces along blockIdx.y.  Caller-owned buffers are where bicubic_wrap_check_kernel runs for a partial
    handle; a fresh device output is range-checked in the kernel by the first piece."""
    dt, w = long_rows["dt"], long_rows["w"]
    C = vn(dt) * 513 if vec else 513
    it = w.handle(0, C, "pieces, partials")
    run_partials_and_jet(it, w, 0, C, long_rows["qx"][:65], long_rows["qy"][:65], capfd, f"pieces vec={vec}", vec=vec, lv=513, gy=2, klds=1)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_partials_and_jet_on_short_rows(pkg, capfd, dt):
    """1, 4 and 5 lanes of the small grid, 200 queries"""
    w, qx, qy = small_grid(pkg, dt, 10)
    for lo, hi in SLICES_145:
        it = w.handle(lo, hi, "short rows, partials")
        run_partials_and_jet(it, w, lo, hi, qx, qy, capfd, f"short rows C={hi - lo}", klds=1, gy=1, **form_of(hi - lo, dt))


def jet_failure(it, qx, qy, order=1, into=None):
    with pytest.raises(Exception) as e:
        if into is not None:
            it.jet_into(qx, qy, into)
        else:
            it.jet(qx, qy, order)
    return type(e.value).__name__, str(e.value), getattr(e.value, "index", None)


@pytest.mark.parametrize("form", ["short", "pieces"])
def test_jet_first_error_on_a_wrapping_handle(pkg, long_rows, form):
    """NaN and +-inf on a wrapping axis with a later failure of the other axis: the report is the value call's (the periodic
    1-D spline's, test_first_error_across_pieces), rows before it are bit-exact in all K parts, rows from it on keep the
    sentinel in all K parts.  5 lanes, and 513 lanes in two pieces."""
    import torch
    dt, w = long_rows["dt"], long_rows["w"]
    C = 5 if form == "short" else 513
    nq = 200
    it = w.handle(0, C, "jet first error")
    tdt = torch.float32 if dt == np.float32 else torch.float64
    want6 = [w.part(long_rows["qx"], long_rows["qy"], nu)[:, :C] for nu in JET_PARTS[2]]
    for order in (1, 2):
        K = len(JET_PARTS[order])
        for axis in (0, 1):
            for bad in (np.nan, np.inf, -np.inf):
                for pos in (0, nq // 2, nq - 1):
                    qx, qy = long_rows["qx"].copy(), long_rows["qy"].copy()
                    (qx, qy)[axis][pos] = bad
                    if pos + 7 < nq:
                        (qx, qy)[1 - axis][pos + 7] = np.nan
                    what = f"jet {form} order {order}: {bad} on axis {axis} at {pos}"
                    exp = failure(it, qx, qy)[:3]
                    assert exp[0] == "Panic" and exp[2] == pos, what
                    dqx, dqy = dev(qx), dev(qy)
                    assert jet_failure(it, qx, qy, order) == exp and jet_failure(it, dqx, dqy, order) == exp, what
                    for mk in (lambda: np.full((nq, C), SENTINEL, dt), lambda: torch.full((nq, C), SENTINEL, dtype=tdt, device="cuda:0")):
                        bufs = [mk() for _ in range(K)]
                        q = (qx, qy) if isinstance(bufs[0], np.ndarray) else (dqx, dqy)
                        assert jet_failure(it, *q, into=bufs) == exp, what
                        for k, b in enumerate(bufs):
                            rows = to_np(b)
                            check_bits(rows[:pos], want6[k][:pos], f"{what}: part {k}, rows before the failure")
                            assert np.all(rows[pos:] == SENTINEL), f"{what}: part {k}, rows from the failure on keep the sentinel"


# ---- under the bounds-checked library -----------------------------------------------------------------------------------------
def test_wrapping_forms_under_the_bounds_checked_library():
    """The f32 40 000 x 5 KLDS = false wrapping case, lv = 513 in both forms, the past-the-end axis with the jet, and the
    adjacent / big / mixed2 hostile pairs at 5 and 9 lanes, in a fresh child process that loads the bounds-checked build: a
    device-side index out of range (cell, strip, table) fails the call."""
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import os, sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package\n"
        "import test_gpu_bicubic_periodic_plans as p, test_gpu_bicubic_periodic_hostile as t\n"
        "pkg = load_product_package()\n"
        "os.environ['NDI_TRACE_PLAN'] = '1'\n"
        "p.run_global(pkg, None, np.float32, 40_000, 5, 3, False, slices=((1, 5), (5, 10)), thin=9)\n"
        "print('[global done]', file=sys.stderr, flush=True)\n"
        "for dt in (np.float32, np.float64):\n"
        "    p.run_long(pkg, None, p.make_long(pkg, dt), 513, nqs=(65,))\n"
        "    for even in (True, False):\n"
        "        p.run_past_end(pkg, None, dt, 65, even, 0, partials=False)\n"
        "print('[forms done]', file=sys.stderr, flush=True)\n"
        "for dt in (np.float32, np.float64):\n"
        "    for gi, (nx, ny) in enumerate(t.hostile.BICUBIC_GRIDS):\n"
        "        for i, fx in enumerate(('adjacent', 'big', 'mixed2')):\n"
        "            for j, fy in enumerate(('adjacent', 'big', 'mixed2')):\n"
        "                for C in (5, 9):\n"
        "                    for part in range(t.hostile.bicubic_periodic_parts(C)):\n"
        "                        t.run_case(pkg, dt, nx, ny, fx, fy, ('x', 'y', 'xy')[(i + j + gi) %% 3], (i + j) %% 2 == 1, C, part,\n"
        "                                   f'checked {dt.__name__} {nx}x{ny} {fx} x {fy} C={C} part={part}', thin=7)\n"
        "print('checked OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDI_LIB=lib), timeout=900)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stderr.splitlines()

    def plans_of(seg):
        return [l for l in seg if l.startswith("[ndi plan] bicubic vec=") or l.startswith("[ndi plan] bicubic_jet")]
    g, f = lines.index("[global done]"), lines.index("[forms done]")
    head, forms, hostile_lines = plans_of(lines[:g]), plans_of(lines[g:f]), plans_of(lines[f:])
    assert head and all(" klds=0 " in l and l.endswith(" wrap=xy") for l in head), head[:4]
    assert any(" vec=1 " in l for l in head) and any(" vec=0 " in l for l in head)
    assert forms and all(" klds=1 " in l and (l.endswith(" wrap=xy") or l.endswith(" wrap=x")) for l in forms), forms[:4]
    assert any(l.startswith("[ndi plan] bicubic_jet") and l.endswith(" wrap=x") for l in forms)
    for vec in (0, 1):
        assert any(f" vec={vec} lv=513 " in l and " grid=1 x 2 " in l and l.endswith(" wrap=xy") for l in forms), vec
    # the hostile cases build every array twice: with extrapolate (it wraps) and without (it does not)
    for a in ("x", "y", "xy"):
        assert any(l.endswith(f" wrap={a}") for l in hostile_lines if l.startswith("[ndi plan] bicubic vec=")), a
        assert any(l.endswith(f" wrap={a}") for l in hostile_lines if l.startswith("[ndi plan] bicubic_jet")), a
