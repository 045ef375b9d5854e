"""GPU: partial-derivative handles of Bicubic (ndi_interp2d_partial, Bicubic.partial) against the numpy restatement of their
contract (tests/bicubic_partial_ref.py) on the device's own node tables, bit for bit, f32 and f64: all eight orders on the
hostile 2-D query set, the kernel's row-length branches at the smallest shapes that reach them (the ones
tests/test_gpu_bicubic_plans.py found for the value kernel, each held to its plan line), extrapolation, the error semantics
against Bilinear's, the shared node table and its lifetime, every other surface of a handle, and the value path as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bicubic_partial_ref as ref
import bicubic_ref
import hostile_inputs
from hostile_inputs import check_bits
from test_gpu_bicubic import build, failure, make_grid
from test_gpu_bicubic_plans import PLAN, SENTINEL, dev, expect_plan, sentinel_buffer, to_np, traced, uneven, vn

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
ORDERS = ref.ORDERS
FOUR = ((1, 0), (0, 1), (1, 1), (2, 2))
NU = re.compile(r"\[ndi plan\] bicubic vec=\d+ lv=\d+ klds=\d+ grid=\d+ x \d+ lds=\d+ prepass=\d+ guess=\d+,\d+ levels=\d+,\d+ "
                r"nu=(\d),(\d)\n")


def rows_of(it, x, y, z, qx, qy, order, tabs=None):
    """the restatement on the device's own tables, floating-point warnings off"""
    tabs = it.strategy.tables() if tabs is None else tabs
    with np.errstate(all="ignore"):
        return ref.evaluate(x, y, z, *tabs, qx, qy, *order)


def both_ways(p, qx, qy, want, what):
    check_bits(p.interp_array(qx, qy), want, f"{what}: host queries")
    check_bits(to_np(p.interp_array(dev(qx), dev(qy))), want, f"{what}: device queries")


# ---- all eight orders -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("even", [False, True], ids=["uneven", "even"])
@pytest.mark.parametrize("shape", [(5, 7, 3), (9, 6, 8)], ids=["5x7x3-scalar", "9x6x8-vectors"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_all_orders_on_the_hostile_queries(pkg, capfd, dt, shape, even):
    """5 x 7 x 3: scalar lanes, several queries per trip; 9 x 6 x 8: 16-byte vectors.  Queries: every node, the last knots, one
    ulp either side of every grid line, midpoints, 300 random points (tests/hostile_inputs.py, bicubic_queries)."""
    nx, ny, Cn = shape
    rng = np.random.default_rng(nx * 100 + ny + even)
    x = np.arange(nx).astype(dt) if even else uneven(rng, nx, dt)
    y = (np.arange(ny) * 0.5).astype(dt) if even else uneven(rng, ny, dt)
    z = rng.normal(size=shape).astype(dt)
    it = build(pkg, x, y, z)
    tabs = it.strategy.tables()
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=300)
    vec = int(Cn % vn(dt) == 0)
    for order in ORDERS:
        p = it.partial(*order)
        assert p.strategy.orders == order and isinstance(p.strategy, pkg.Bicubic) and p.x is it.x and p.y is it.y
        want = rows_of(it, x, y, z, qx, qy, order, tabs)
        rows, plans = traced(capfd, lambda: p.interp_array(dev(qx), dev(qy)))
        expect_plan(plans, f"order {order}", vec=vec, lv=Cn // vn(dt) if vec else Cn, klds=1)
        check_bits(to_np(rows), want, f"order {order}: device queries")
        check_bits(p.interp_array(qx, qy), want, f"order {order}: host queries")
    for a, b in zip(p.strategy.tables(), tabs):          # ndi_interp2d_tables of a partial: the origin's zx, zy, zxy
        check_bits(a, b, "tables of a partial handle")


# ---- row lengths ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=DTYPES, ids=DT_IDS)
def wide(pkg, request):
    """4 x 5 x (VN * 65), 65 queries (a wave's second batch of one query): one grid, handles on slices of its lanes"""
    dt = request.param
    rng = np.random.default_rng(65)
    x, y = uneven(rng, 4, dt), uneven(rng, 5, dt)
    z = rng.normal(size=(4, 5, vn(dt) * 65)).astype(dt)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=0)
    pick = rng.permutation(len(qx))[:65]
    return dict(dt=dt, x=x, y=y, z=z, qx=qx[pick], qy=qy[pick])


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
        it = build(pkg, x, y, z)
        tabs = it.strategy.tables()
        for order in FOUR:
            p = it.partial(*order)
            want = rows_of(it, x, y, z, wide["qx"], wide["qy"], order, tabs)
            for q in ((wide["qx"], wide["qy"]), (dev(wide["qx"]), dev(wide["qy"]))):
                rows, plans = traced(capfd, lambda: p.interp_array(*q))
                expect_plan(plans, f"lv={lv} vec={vec} {order}", vec=vec, lv=lv, gy=1, klds=1)
                check_bits(to_np(rows), want, f"lv={lv} vec={vec} order {order}")
            e = np.empty(0, dt)
            assert p.interp_array(e, e).shape == (0, Cn) and tuple(p.interp_array(dev(e), dev(e)).shape) == (0, Cn)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_row_cut_into_pieces(pkg, capfd, dt):
    """3 x 3 x 513, scalar lanes: two pieces along blockIdx.y, the second of one element"""
    rng = np.random.default_rng(513)
    x, y = uneven(rng, 3, dt), uneven(rng, 3, dt)
    z = rng.normal(size=(3, 3, 513)).astype(dt)
    it = build(pkg, x, y, z)
    tabs = it.strategy.tables()
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=20)
    for order in FOUR:
        p = it.partial(*order)
        want = rows_of(it, x, y, z, qx, qy, order, tabs)
        rows, plans = traced(capfd, lambda: p.interp_array(dev(qx), dev(qy)))
        expect_plan(plans, f"pieces {order}", vec=0, lv=513, gy=2)
        check_bits(to_np(rows), want, f"pieces, order {order}")
        buf = sentinel_buffer((len(qx), 513), dt, True)
        _, plans = traced(capfd, lambda: p.interp_array_into(dev(qx), dev(qy), buf))
        expect_plan(plans, f"pieces into {order}", vec=0, lv=513, gy=2, prepass=1)
        check_bits(to_np(buf), want, f"pieces, caller-owned buffer, order {order}")


def test_knots_in_global_memory(pkg, capfd):
    """17 880 x 3 x 1 f64: one knot past what fits LDS beside the strips (tests/test_gpu_bicubic_plans.py derives the
    number): the searches read the knots from global memory"""
    rng = np.random.default_rng(17_880)
    x, y = uneven(rng, 17_880, np.float64), uneven(rng, 3, np.float64)
    z = rng.normal(size=(17_880, 3, 1))
    it = build(pkg, x, y, z)
    tabs = it.strategy.tables()
    near = np.concatenate([x[:40], np.nextafter(x[1:40], -np.inf), x[-40:], np.nextafter(x[-40:], -np.inf)])
    qx = np.concatenate([near, rng.uniform(x[0], x[-1], 2000)])
    qy = np.clip(np.resize(np.concatenate([y, np.nextafter(y, -np.inf), np.nextafter(y, np.inf)]), len(qx)), y[0], y[-1])
    for order in FOUR:
        p = it.partial(*order)
        want = rows_of(it, x, y, z, qx, qy, order, tabs)
        rows, plans = traced(capfd, lambda: p.interp_array(dev(qx), dev(qy)))
        expect_plan(plans, f"global knots {order}", klds=0, vec=0, lv=1, lds=10_240)
        check_bits(to_np(rows), want, f"global knots, order {order}")


# ---- extrapolation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_extrapolation_continues_the_end_patches(pkg, dt):
    rng = np.random.default_rng(3)
    x, y, z = make_grid(rng, 9, 7, 3, dt)
    it = build(pkg, x, y, z, extrapolate=True)
    tabs = it.strategy.tables()
    wx, wy = x[-1] - x[0], y[-1] - y[0]
    qx = rng.uniform(x[0] - wx, x[-1] + wx, 1000).astype(dt)
    qy = rng.uniform(y[0] - wy, y[-1] + wy, 1000).astype(dt)
    qx[:8] = [x[0] - wx, x[0] - wx, x[-1] + wx, x[-1] + wx, x[0] - wx, x[-1] + wx, x[3], x[4]]      # corners, sides
    qy[:8] = [y[0] - wy, y[-1] + wy, y[0] - wy, y[-1] + wy, y[2], y[3], y[0] - wy, y[-1] + wy]
    assert np.any(qx < x[0]) and np.any(qx > x[-1]) and np.any(qy < y[0]) and np.any(qy > y[-1])
    for order in ORDERS:
        p = it.partial(*order)
        both_ways(p, qx, qy, rows_of(it, x, y, z, qx, qy, order, tabs), f"extrapolate, order {order}")
    with pytest.raises(pkg.Panic, match="NaN"):
        p.interp_array(np.array([x[1], np.nan], dt), np.array([y[1], y[1]], dt))


# ---- errors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["x_high", "y_low", "both"])
def test_out_of_range_is_bilinears(pkg, kind):
    """Without `extrapolate`: the first-error report (x before y, the lowest index) is Bilinear's on the same queries; rows
    before the failing query are written, rows from it on keep the sentinel of a caller-owned buffer; a fresh output raises."""
    import torch
    rng = np.random.default_rng(8)
    x, y, z = make_grid(rng, 9, 7, 5, np.float64)
    it = build(pkg, x, y, z)
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    tabs = it.strategy.tables()
    nq = 300
    qx0, qy0 = rng.uniform(x[0], x[-1], nq), rng.uniform(y[0], y[-1], nq)
    for order in ((1, 0), (2, 1)):
        p = it.partial(*order)
        want = rows_of(it, x, y, z, qx0, qy0, order, tabs)
        for pos in (0, 131, nq - 1):
            qx, qy = qx0.copy(), qy0.copy()
            if kind in ("x_high", "both"):
                qx[pos] = x[-1] + 0.25
            if kind in ("y_low", "both"):
                qy[pos] = y[0] - 0.25
            if pos + 7 < nq:
                qy[pos + 7] = np.nan                       # a later failure must not be the one reported
            exp = failure(bil, qx, qy)
            assert exp[2] == pos and exp[4] == (1 if kind == "y_low" else 0)
            dqx, dqy = dev(qx), dev(qy)
            assert failure(p, qx, qy) == exp and failure(p, dqx, dqy) == exp            # fresh outputs
            for mk in (lambda: np.full((nq, 5), SENTINEL), lambda: torch.full((nq, 5), SENTINEL, dtype=torch.float64, device="cuda:0")):
                buf = mk()
                q = (qx, qy) if isinstance(buf, np.ndarray) else (dqx, dqy)
                assert failure(p, *q, into=buf) == exp
                rows = to_np(buf)
                check_bits(rows[:pos], want[:pos], "rows before the failure")
                assert np.all(rows[pos:] == SENTINEL), "rows from the failure on keep the sentinel"


# ---- sharing and lifetime -----------------------------------------------------------------------------------------------------
def test_partials_share_the_table_and_outlive_the_source(pkg):
    """1024 x 512 x 4 f64: a grid of 16 MiB, a node table of 64 MiB.  Two partial handles cost less device memory than one
    grid (four knot-axis allocations, no table), and evaluate after the source is destroyed."""
    import torch
    rng = np.random.default_rng(1024)
    x, y = uneven(rng, 1024, np.float64), uneven(rng, 512, np.float64)
    z = rng.normal(size=(1024, 512, 4))
    it = build(pkg, x, y, z)
    tabs = it.strategy.tables()
    qx, qy = rng.uniform(x[0], x[-1], 500), rng.uniform(y[0], y[-1], 500)
    qx[:4], qy[:4] = [x[0], x[-1], x[5], x[-1]], [y[-1], y[-1], y[7], y[0]]
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    px, py = it.partial(1, 0), it.partial(0, 1)
    free1, _ = torch.cuda.mem_get_info(0)
    print(f"two partial handles took {free0 - free1} bytes of device memory; one grid is {z.nbytes}")
    assert free0 - free1 < z.nbytes, (free0 - free1, z.nbytes)
    it.strategy.release()                                  # the source goes first
    both_ways(px, qx, qy, ref.evaluate(x, y, z, *tabs, qx, qy, 1, 0), "d/dx after the source is gone")
    both_ways(py, qx, qy, ref.evaluate(x, y, z, *tabs, qx, qy, 0, 1), "d/dy after the source is gone")
    pxy = px.partial(0, 1)                                 # a partial of a partial whose origin is gone
    px.strategy.release()
    both_ways(pxy, qx, qy, ref.evaluate(x, y, z, *tabs, qx, qy, 1, 1), "d2/dxdy after both are gone")
    pxy.strategy.release()
    py.strategy.release()
    free2, _ = torch.cuda.mem_get_info(0)
    assert free2 - free1 >= 2 * z.nbytes, "the table (four grids) goes with the last handle"


def test_orders_add_and_third_orders_are_refused(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    rng = np.random.default_rng(21)
    x, y, z = make_grid(rng, 9, 6, 8, np.float32)
    it = build(pkg, x, y, z)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=100)
    a, b = it.partial(1, 0).partial(0, 1), it.partial(1, 1)
    assert a.strategy.orders == b.strategy.orders == (1, 1)
    check_bits(a.interp_array(qx, qy), b.interp_array(qx, qy), "partial(1, 0).partial(0, 1) against partial(1, 1)")
    check_bits(it.partial(1, 0).partial(1, 2).interp_array(qx, qy), rows_of(it, x, y, z, qx, qy, (2, 2)), "(1, 0) + (1, 2)")
    p20 = it.partial(2, 0)
    with pytest.raises(ValueError, match="Bicubic.*third derivative"):
        p20.partial(1, 0)
    h = C.c_void_p(77)                                     # and the library itself, whatever the mirror knows
    for src, nux, nuy, text in ((p20, 1, 0, "third derivative"), (it, 0, 3, "third derivative"), (it, 0, 0, "(0, 0)"),
                                (p20, 0, 0, "(0, 0)"), (it, -1, 1, "below 0"), (p20, -2, 0, "below 0")):
        assert lib.ndi_interp2d_partial(src.strategy._h, nux, nuy, C.byref(h)) == cap.BAD_ARG, (nux, nuy)
        assert cap.last_error().startswith("Bicubic") and text in cap.last_error() and h.value is None, cap.last_error()
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    assert lib.ndi_interp2d_partial(bil.strategy._h, 1, 0, C.byref(h)) == cap.BAD_ARG
    assert cap.last_error().startswith("Bilinear has no partial-derivative handle") and h.value is None
    with pytest.raises(TypeError, match="Bilinear has no partial derivatives"):
        bil.partial(1, 0)
    check_bits(p20.interp_array(qx, qy), rows_of(it, x, y, z, qx, qy, (2, 0)), "the refused source still evaluates")


# ---- everything a handle takes --------------------------------------------------------------------------------------------------
def test_clone_ring_sharded_async_and_strided_rows(pkg):
    import torch
    rng = np.random.default_rng(33)
    x, y, z = make_grid(rng, 33, 20, 5, np.float64)
    it = build(pkg, x, y, z)
    p = it.partial(1, 1)
    nq = 2007
    qx, qy = rng.uniform(x[0], x[-1], nq), rng.uniform(y[0], y[-1], nq)
    want = rows_of(it, x, y, z, qx, qy, (1, 1))
    dqx, dqy = dev(qx), dev(qy)
    out = torch.empty((nq, 5), dtype=torch.float64, device="cuda:0")
    p.interp_array_into(dqx, dqy, out, async_launch=True)                        # async_launch + finish
    p.strategy.finish()
    check_bits(to_np(out), want, "async_launch + finish")
    rep = p.replicate([0])[0]                                                    # clone: the table copied, the orders kept
    assert rep.strategy.orders == (1, 1) and rep.strategy._h.value != p.strategy._h.value
    for a, b in zip(rep.strategy.tables(), it.strategy.tables()):
        check_bits(a, b, "clone: tables")
    check_bits(rep.interp_array(qx, qy), want, "clone: rows")
    check_bits(rep.partial(0, 1).interp_array(qx, qy), rows_of(it, x, y, z, qx, qy, (1, 2)), "a partial of the clone")
    got = np.zeros_like(want)                                                    # ring: two chunks
    ring = pkg.striped_ring(1500, 5, 2, np.float64, 0)
    chunks = []

    def consumer(c, rows):
        chunks.append(c.q_count)
        got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
    p.interp_array_ring(dqx, dqy, 1500, consumer, slots=ring)
    assert chunks == [1500, 507]
    check_bits(got, want, "ring")
    got = np.full_like(want, -1.0)                                               # sharded: two replicas on one device
    pkg.sharding.interp_array_sharded([p, rep], qx, qy, out=got)
    check_bits(got, want, "sharded")
    for other in (it, it.partial(1, 0)):                                         # the orders are part of the signature
        with pytest.raises(Exception, match="replicas of one interpolator"):
            pkg.sharding.interp_array_sharded([p, other], qx, qy, out=got)
    p.strategy.trim()
    check_bits(p.interp_array(qx, qy), want, "after trim")
    for name, stride, base in (("lanes + 1", 6, 0), ("base + 1", 5, 1)):          # strided and misaligned rows, C = 5
        flat = sentinel_buffer((nq * stride + base + 1,), np.float64, True)
        view = flat[base:base + nq * stride].view(nq, stride)[:, :5]
        p.strategy.interp_array_into(p, dqx, dqy, view)
        h = to_np(flat)
        check_bits(h[base:base + nq * stride].reshape(nq, stride)[:, :5], want, name)
        gaps = np.ones(h.shape, bool)
        gaps[base:base + nq * stride].reshape(nq, stride)[:, :5] = False
        assert np.all(h[gaps] == SENTINEL), f"{name}: gap elements were written"
    p.strategy.path = pkg.PATH_BUCKETED
    with pytest.raises(Exception, match="Bicubic has no tile-grouped evaluation form"):
        p.interp_array(qx, qy)


# ---- the value path and the trace line ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_value_path_is_unchanged_and_the_plan_line_carries_the_orders(pkg, capfd, dt):
    for shape in ((5, 7, 3), (9, 6, 8)):
        rng = np.random.default_rng(shape[0])
        x, y, z = make_grid(rng, *shape, dt)
        it = build(pkg, x, y, z)
        tabs = it.strategy.tables()
        qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=300)
        capfd.readouterr()
        rows, plans = traced(capfd, lambda: it.interp_array(dev(qx), dev(qy)))
        vec = int(shape[2] % vn(dt) == 0)
        expect_plan(plans, "value", vec=vec, lv=shape[2] // vn(dt) if vec else shape[2], klds=1, prepass=0, gy=1)
        with np.errstate(all="ignore"):
            check_bits(to_np(rows), bicubic_ref.evaluate(x, y, z, *tabs, qx, qy), "the surface itself")
        for order in ((0, 0), (1, 2), (2, 0)):
            h = it if order == (0, 0) else it.partial(*order)
            before = os.environ.get("NDI_TRACE_PLAN")
            os.environ["NDI_TRACE_PLAN"] = "1"
            try:
                h.interp_array(dev(qx), dev(qy))
            finally:
                if before is None:
                    del os.environ["NDI_TRACE_PLAN"]
                else:
                    os.environ["NDI_TRACE_PLAN"] = before
            err = capfd.readouterr().err
            assert [m.groups() for m in NU.finditer(err)] == [(str(order[0]), str(order[1]))], err[-300:]
            assert len(PLAN.findall(err)) == 1                      # the old fields, names and order as they were
