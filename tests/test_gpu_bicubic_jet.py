"""GPU: the fused value-and-gradient (jet) evaluation of Bicubic (ndi_interp2d_eval_jet, Bicubic.jet_into, Interp2D.jet)
against the numpy restatement of the partial-derivative contract (tests/bicubic_partial_ref.py; tests/bicubic_ref.py for part
0) on the device's own node tables, bit for bit, f32 and f64 -- and, where a case says so, against the separate partial
handles evaluated on the device.  Both orders on the hostile query set, the kernel's row-length branches at the smallest
shapes that reach them (each held to the plan line `[ndi plan] bicubic_jet ...`), the output layouts one stride and K bases
can express, extrapolation, the first-error semantics in EVERY part against Bilinear's report, a wave's second batch, the
host-output staging chunks, the hostile grids, every refusal of the library, and the surroundings as they were."""
import ctypes as C
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import bicubic_partial_ref as ref
import bicubic_ref
import hostile_inputs
from conftest import ROOT
from hostile_inputs import check_bits
from test_gpu_bicubic import build, failure, make_grid
from test_gpu_bicubic_partial import wide  # noqa: F401  (the 4 x 5 x (VN * 65) fixture of the partial handles' row lengths)
from test_gpu_bicubic_partial_hostile import THIN
from test_gpu_bicubic_plans import SENTINEL, dev, sentinel_buffer, to_np, traced, uneven, vn

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
JET = re.compile(r"\[ndi plan\] bicubic_jet order=(\d) vec=(\d+) lv=(\d+) klds=(\d+) grid=(\d+) x (\d+) lds=(\d+) prepass=(\d+)\n")
JET_FIELDS = ("order", "vec", "lv", "klds", "gx", "gy", "lds", "prepass")
STAGE_BYTES = 256 << 20          # the host-output staging size of the library (csrc/bicubic_jet_host.hpp)


def parts_of(pkg, order):
    return pkg.JET_PARTS[order]


def jet_traced(capfd, call):
    """(result, plans): the call under NDI_TRACE_PLAN and the fields of every jet plan line it printed"""
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
    plans = [dict(zip(JET_FIELDS, (int(v) for v in m.groups()))) for m in JET.finditer(err)]
    assert plans, f"no jet plan line in: {err[-500:]}"
    assert "[ndi plan] bicubic vec=" not in err, "a jet call launched the value kernel"
    return r, plans


def expect_jet(plans, what, **fields):
    for p in plans:
        got = {k: p[k] for k in fields}
        assert got == fields, f"{what}: plan {p} where {fields} was expected"


def want_parts(x, y, z, tabs, qx, qy, nus):
    """the restatement's rows of each part on the given tables, floating-point warnings off"""
    with np.errstate(all="ignore"):
        return [bicubic_ref.evaluate(x, y, z, *tabs, qx, qy) if nu == (0, 0) else ref.evaluate(x, y, z, *tabs, qx, qy, *nu)
                for nu in nus]


def check_parts(got, want, what, nus):
    assert len(got) == len(want) == len(nus), what
    for g, w, nu in zip(got, want, nus):
        check_bits(to_np(g), w, f"{what}: part {nu}")


def jet_failure(it, qx, qy, order=1, into=None):
    """test_gpu_bicubic.failure for the jet calls"""
    with pytest.raises(Exception) as e:
        if into is not None:
            it.jet_into(qx, qy, into)
        else:
            it.jet(qx, qy, order)
    v = e.value
    return type(v).__name__, str(v), getattr(v, "index", None), getattr(v, "value", None), getattr(v, "axis", None)


# ---- 1: both orders on the hostile queries ----------------------------------------------------------------------------------
def run_hostile_queries(pkg, dt, shape, even, capfd=None):
    nx, ny, Cn = shape
    rng = np.random.default_rng(nx * 100 + ny + even)
    x = np.arange(nx).astype(dt) if even else uneven(rng, nx, dt)
    y = (np.arange(ny) * 0.5).astype(dt) if even else uneven(rng, ny, dt)
    z = rng.normal(size=shape).astype(dt)
    it = build(pkg, x, y, z)
    tabs = it.strategy.tables()
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=300)
    vec = int(Cn % vn(dt) == 0)
    want6 = want_parts(x, y, z, tabs, qx, qy, parts_of(pkg, 2))
    handles = [it if nu == (0, 0) else it.partial(*nu) for nu in parts_of(pkg, 2)]
    for order in (1, 2):
        nus = parts_of(pkg, order)
        want = want6[:len(nus)]
        for on_device in (True, False):
            q = (dev(qx), dev(qy)) if on_device else (qx, qy)
            if capfd is None:
                got = it.jet(*q, order)
            else:
                got, plans = jet_traced(capfd, lambda: it.jet(*q, order))
                expect_jet(plans, f"order {order} device={on_device}", order=order, vec=vec, lv=Cn // vn(dt) if vec else Cn,
                           klds=1, prepass=0 if on_device else 1)
            assert len(got) == len(nus) and all(tuple(g.shape) == (len(qx), Cn) for g in got)
            assert all(isinstance(g, np.ndarray) != on_device for g in got)
            check_parts(got, want, f"order {order} device={on_device}", nus)
            for g, h, nu in zip(got, handles, nus):                    # and the separate handles on the same queries
                check_bits(to_np(g), to_np(h.interp_array(*q)), f"order {order} device={on_device}: part {nu} against its handle")
    got = it.value_and_gradient(dev(qx), dev(qy))
    check_parts(got, want6[:3], "value_and_gradient", parts_of(pkg, 1))


@pytest.mark.parametrize("even", [False, True], ids=["uneven", "even"])
@pytest.mark.parametrize("shape", [(5, 7, 3), (9, 6, 8)], ids=["5x7x3-scalar", "9x6x8-vectors"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_both_orders_on_the_hostile_queries(pkg, capfd, dt, shape, even):
    """5 x 7 x 3: scalar lanes, several queries per trip; 9 x 6 x 8: 16-byte vectors.  Queries: every node, the last knots, one
    ulp either side of every grid line, midpoints, 300 random points (tests/hostile_inputs.py, bicubic_queries)."""
    run_hostile_queries(pkg, dt, shape, even, capfd)


# ---- 2: row lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lv", [1, 2, 63, 64, 65])
def test_row_lengths(pkg, capfd, wide, lv):  # noqa: F811
    """lv vectors per row: 1 (no division), 2 and 63 (the magic division, several queries per trip), 64 (one full trip per
    query), 65 (a trip and a tail) -- in the vector form at lanes = VN * lv and, where the lanes do not divide, the scalar
    form at lanes = lv.  65 queries (a wave's second batch of one query), both orders; then the empty batch."""
    dt, x, y = wide["dt"], wide["x"], wide["y"]
    for Cn, vec in ((vn(dt) * lv, 1), (lv, 0)):
        if not vec and lv % vn(dt) == 0:
            continue
        z = np.ascontiguousarray(wide["z"][:, :, :Cn])
        it = build(pkg, x, y, z)
        want6 = want_parts(x, y, z, it.strategy.tables(), wide["qx"], wide["qy"], parts_of(pkg, 2))
        for order in (1, 2):
            nus = parts_of(pkg, order)
            for q in ((wide["qx"], wide["qy"]), (dev(wide["qx"]), dev(wide["qy"]))):
                got, plans = jet_traced(capfd, lambda: it.jet(*q, order))
                expect_jet(plans, f"lv={lv} vec={vec} order {order}", order=order, vec=vec, lv=lv, gy=1, klds=1)
                check_parts(got, want6[:len(nus)], f"lv={lv} vec={vec} order {order}", nus)
            e = np.empty(0, dt)
            for q in ((e, e), (dev(e), dev(e))):
                got = it.jet(*q, order)
                assert len(got) == len(nus) and all(tuple(g.shape) == (0, Cn) for g in got)
        check_bits(it.jet(wide["qx"][:1], wide["qy"][:1])[1], want6[1][:1], "after the empty batches")


# ---- 3: pieces along blockIdx.y ---------------------------------------------------------------------------------------------
def run_pieces(pkg, dt, capfd=None):
    rng = np.random.default_rng(513)
    x, y = uneven(rng, 3, dt), uneven(rng, 3, dt)
    z = rng.normal(size=(3, 3, 513)).astype(dt)
    it = build(pkg, x, y, z)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=20)
    want6 = want_parts(x, y, z, it.strategy.tables(), qx, qy, parts_of(pkg, 2))
    for order in (1, 2):
        nus = parts_of(pkg, order)
        bufs = [sentinel_buffer((len(qx), 513), dt, True) for _ in nus]
        if capfd is None:
            got = it.jet(dev(qx), dev(qy), order)
            it.jet_into(dev(qx), dev(qy), bufs)
        else:
            got, plans = jet_traced(capfd, lambda: it.jet(dev(qx), dev(qy), order))
            expect_jet(plans, f"pieces order {order}", order=order, vec=0, lv=513, gy=2, prepass=0)
            _, plans = jet_traced(capfd, lambda: it.jet_into(dev(qx), dev(qy), bufs))
            expect_jet(plans, f"pieces into order {order}", order=order, vec=0, lv=513, gy=2, prepass=1)
        check_parts(got, want6[:len(nus)], f"pieces, fresh output, order {order}", nus)
        check_parts(bufs, want6[:len(nus)], f"pieces, caller-owned buffers, order {order}", nus)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_row_cut_into_pieces(pkg, capfd, dt):
    """3 x 3 x 513, scalar lanes: two pieces along blockIdx.y, the second of one element; a fresh output (the range test on
    blockIdx.y == 0 only) and caller-owned buffers (the pre-pass)"""
    run_pieces(pkg, dt, capfd)


# ---- 4: knots in global memory ----------------------------------------------------------------------------------------------
def test_knots_in_global_memory(pkg, capfd):
    """17 880 x 3 x 1 f64: one knot past what fits LDS beside the strips (tests/test_gpu_bicubic_plans.py derives the
    number): the searches read the knots from global memory"""
    rng = np.random.default_rng(17_880)
    x, y = uneven(rng, 17_880, np.float64), uneven(rng, 3, np.float64)
    z = rng.normal(size=(17_880, 3, 1))
    it = build(pkg, x, y, z)
    near = np.concatenate([x[:40], np.nextafter(x[1:40], -np.inf), x[-40:], np.nextafter(x[-40:], -np.inf)])
    qx = np.concatenate([near, rng.uniform(x[0], x[-1], 2000)])
    qy = np.clip(np.resize(np.concatenate([y, np.nextafter(y, -np.inf), np.nextafter(y, np.inf)]), len(qx)), y[0], y[-1])
    want6 = want_parts(x, y, z, it.strategy.tables(), qx, qy, parts_of(pkg, 2))
    for order in (1, 2):
        nus = parts_of(pkg, order)
        got, plans = jet_traced(capfd, lambda: it.jet(dev(qx), dev(qy), order))
        expect_jet(plans, f"global knots order {order}", order=order, klds=0, vec=0, lv=1, lds=10_240)
        check_parts(got, want6[:len(nus)], f"global knots, order {order}", nus)


# ---- 5: layouts -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=DTYPES, ids=DT_IDS)
def grid64(pkg, request):
    """64 x 48 x 5 and 1000 queries: the restatement of all six parts once per dtype (lanes are independent: the handle on the
    first four lanes has the first four columns)"""
    dt = request.param
    rng = np.random.default_rng(64)
    x, y = uneven(rng, 64, dt), uneven(rng, 48, dt)
    z = rng.normal(size=(64, 48, 5)).astype(dt)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=1000)
    pick = rng.permutation(len(qx))[:1000]
    qx, qy = qx[pick], qy[pick]
    with np.errstate(all="ignore"):
        tabs = bicubic_ref.tables(x, y, z)
    return dict(dt=dt, x=x, y=y, z=z, qx=qx, qy=qy, tabs=tabs, want=want_parts(x, y, z, tabs, qx, qy, pkg.JET_PARTS[2]))


@pytest.mark.parametrize("Cn", [4, 5])
@pytest.mark.parametrize("order", [1, 2])
def test_layouts(pkg, capfd, grid64, order, Cn):
    """Into views of larger sentinel-filled buffers: planar with stride lanes, planar with stride lanes + VN (the vector form
    where the lanes divide), interleaved (nq, K, lanes) with stride K * lanes, and one part's base one element past a 16-byte
    boundary with the others aligned (all parts scalar).  Every element outside the parts keeps the sentinel.  Device buffers
    with device queries, and the same views as host arrays with host queries."""
    dt, x, y, qx, qy = (grid64[k] for k in ("dt", "x", "y", "qx", "qy"))
    z = np.ascontiguousarray(grid64["z"][:, :, :Cn])
    it = build(pkg, x, y, z)
    for name, g, r in zip(("zx", "zy", "zxy"), it.strategy.tables(), grid64["tabs"]):
        check_bits(g, r[:, :, :Cn], f"tables {name}")
    nus = parts_of(pkg, order)
    K, nq, V = len(nus), len(qx), vn(dt)
    want = [w[:, :Cn] for w in grid64["want"][:K]]
    divides = int(Cn % V == 0)

    def planar(stride):
        def views(flat):
            body = flat[:K * nq * stride]
            body = body.view(K, nq, stride) if not isinstance(body, np.ndarray) else body.reshape(K, nq, stride)
            return [body[k][:, :Cn] for k in range(K)]
        return K * nq * stride + 1, views

    def interleaved(flat):
        body = flat[:nq * K * Cn]
        body = body.view(nq, K, Cn) if not isinstance(body, np.ndarray) else body.reshape(nq, K, Cn)
        return [body[:, k, :] for k in range(K)]

    slot = (nq * Cn + V + V - 1) // V * V          # elements per part, a whole number of vectors, with room for the shift

    def one_misaligned(flat):
        out = []
        for k in range(K):
            base = k * slot + (1 if k == 1 else 0)
            body = flat[base:base + nq * Cn]
            out.append(body.view(nq, Cn) if not isinstance(body, np.ndarray) else body.reshape(nq, Cn))
        return out

    layouts = (("planar, stride lanes", *planar(Cn), divides),
               ("planar, stride lanes + VN", *planar(Cn + V), divides),
               ("interleaved", nq * K * Cn + 1, interleaved, divides),
               ("one part misaligned", K * slot, one_misaligned, 0))
    for name, total, views, vec in layouts:
        for on_device in (True, False):
            flat = sentinel_buffer((total,), dt, on_device)
            parts = views(flat)
            q = (dev(qx), dev(qy)) if on_device else (qx, qy)
            what = f"{name} C={Cn} order={order} device={on_device}"
            _, plans = jet_traced(capfd, lambda: it.strategy.jet_into(*q, parts))
            if on_device:
                assert parts[0].data_ptr() % 16 == 0
                expect_jet(plans, what, order=order, vec=vec, lv=Cn // V if vec else Cn, prepass=1)
            check_parts(parts, want, what, nus)
            h = to_np(flat)
            written = np.zeros(h.shape, bool)
            for p in views(written):
                p[...] = True
            assert written.sum() == K * nq * Cn
            assert np.all(h[~written] == SENTINEL), f"{what}: {int((h[~written] != SENTINEL).sum())} gap elements were written"
    with pytest.raises(ValueError, match="share one row stride.*got row strides"):
        it.strategy.jet_into(qx, qy, [np.zeros((nq, Cn + (k == 1)), dt)[:, :Cn] for k in range(K)])
    with pytest.raises(TypeError, match="one memory space"):
        it.strategy.jet_into(qx, qy, [np.zeros((nq, Cn), dt)] * (K - 1) + [sentinel_buffer((nq, Cn), dt, True)])
    with pytest.raises(pkg.Panic, match="do not match"):
        it.jet(qx, qy[:-1], order)


# ---- 6: extrapolation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_extrapolation_continues_the_end_patches(pkg, dt):
    rng = np.random.default_rng(3)
    x, y, z = make_grid(rng, 9, 7, 3, dt)
    it = build(pkg, x, y, z, extrapolate=True)
    wx, wy = x[-1] - x[0], y[-1] - y[0]
    qx = rng.uniform(x[0] - wx, x[-1] + wx, 1000).astype(dt)
    qy = rng.uniform(y[0] - wy, y[-1] + wy, 1000).astype(dt)
    qx[:8] = [x[0] - wx, x[0] - wx, x[-1] + wx, x[-1] + wx, x[0] - wx, x[-1] + wx, x[3], x[4]]      # corners, sides
    qy[:8] = [y[0] - wy, y[-1] + wy, y[0] - wy, y[-1] + wy, y[2], y[3], y[0] - wy, y[-1] + wy]
    assert np.any(qx < x[0]) and np.any(qx > x[-1]) and np.any(qy < y[0]) and np.any(qy > y[-1])
    want6 = want_parts(x, y, z, it.strategy.tables(), qx, qy, parts_of(pkg, 2))
    for order in (1, 2):
        nus = parts_of(pkg, order)
        check_parts(it.jet(qx, qy, order), want6[:len(nus)], f"extrapolate, order {order}, host queries", nus)
        check_parts(it.jet(dev(qx), dev(qy), order), want6[:len(nus)], f"extrapolate, order {order}, device queries", nus)
    bad = np.array([x[1], np.nan], dt), np.array([y[1], y[1]], dt)
    exp = failure(it, *bad)
    assert exp[0] == "Panic" and "NaN" in exp[1]
    for order in (1, 2):
        assert jet_failure(it, *bad, order) == exp and jet_failure(it, dev(bad[0]), dev(bad[1]), order) == exp


# ---- 7: the first error -----------------------------------------------------------------------------------------------------
def first_error_case(pkg, it, bil, x, y, qx0, qy0, want, order, kind, pos, dt, what):
    import torch
    nq, Cn = len(qx0), want[0].shape[1]
    K = len(parts_of(pkg, order))
    qx, qy = qx0.copy(), qy0.copy()
    if kind in ("x_high", "both"):
        qx[pos] = x[-1] + dt(0.25)
    if kind in ("y_low", "both"):
        qy[pos] = y[0] - dt(0.25)
    if pos + 7 < nq:
        qy[pos + 7] = np.nan                       # a later failure must not be the one reported
    exp = failure(bil, qx, qy)
    assert exp[2] == pos and exp[4] == (1 if kind == "y_low" else 0), what
    dqx, dqy = dev(qx), dev(qy)
    assert jet_failure(it, qx, qy, order) == exp and jet_failure(it, dqx, dqy, order) == exp, what      # fresh outputs
    tdt = torch.float32 if np.dtype(dt) == np.float32 else torch.float64
    for mk in (lambda: np.full((nq, Cn), SENTINEL, dt), lambda: torch.full((nq, Cn), SENTINEL, dtype=tdt, device="cuda:0")):
        bufs = [mk() for _ in range(K)]
        q = (qx, qy) if isinstance(bufs[0], np.ndarray) else (dqx, dqy)
        assert jet_failure(it, *q, into=bufs) == exp, what
        for k, b in enumerate(bufs):
            rows = to_np(b)
            check_bits(rows[:pos], want[k][:pos], f"{what}: part {k}, rows before the failure")
            assert np.all(rows[pos:] == SENTINEL), f"{what}: part {k}, rows from the failure on keep the sentinel"


@pytest.mark.parametrize("kind", ["x_high", "y_low", "both"])
def test_first_error_is_bilinears_in_every_part(pkg, kind):
    """Without `extrapolate`: the first-error report (x before y, the lowest index) is Bilinear's on the same queries; rows
    before the failing query are written in each part, rows from it on keep the sentinel in each part."""
    rng = np.random.default_rng(8)
    x, y, z = make_grid(rng, 9, 7, 5, np.float64)
    it = build(pkg, x, y, z)
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    nq = 300
    qx0, qy0 = rng.uniform(x[0], x[-1], nq), rng.uniform(y[0], y[-1], nq)
    want6 = want_parts(x, y, z, it.strategy.tables(), qx0, qy0, parts_of(pkg, 2))
    for order in (1, 2):
        for pos in (0, 131, nq - 1):
            first_error_case(pkg, it, bil, x, y, qx0, qy0, want6, order, kind, pos, np.float64, f"order {order} {kind} at {pos}")


def test_first_error_across_pieces(pkg):
    """The same with gridDim.y > 1, on 4 x 5 x 513 scalar lanes (tests/test_gpu_bicubic_plans.py,
    test_first_error_across_pieces): only blockIdx.y == 0 range-checks a fresh output, and every piece of every caller-owned
    part stops at the first failing query."""
    dt = np.float32
    rng = np.random.default_rng(1537)
    x, y = uneven(rng, 4, dt), uneven(rng, 5, dt)
    z = rng.normal(size=(4, 5, 513)).astype(dt)
    it = build(pkg, x, y, z)
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    nq = 200
    qx0 = rng.uniform(x[0], x[-1], nq).astype(dt).clip(x[0], x[-1])
    qy0 = rng.uniform(y[0], y[-1], nq).astype(dt).clip(y[0], y[-1])
    want3 = want_parts(x, y, z, it.strategy.tables(), qx0, qy0, parts_of(pkg, 1))
    for kind in ("x_high", "y_low"):
        for pos in (0, nq // 2, nq - 1):
            first_error_case(pkg, it, bil, x, y, qx0, qy0, want3, 1, kind, pos, dt, f"pieces {kind} at {pos}")


# ---- 8: a wave's second batch -----------------------------------------------------------------------------------------------
def test_second_batch_of_a_wave(pkg, capfd):
    """More queries than gridDim.x * 256 (3 * 2^20 + 71 on 9 x 7 x 1 f32, the value kernel's test): waves come round and
    rewrite their strip after the closing wave barrier.  Expected rows: the three separate handles on the device (the
    restatement is too slow at this size)."""
    dt, nq = np.float32, 3 * 2**20 + 71
    rng = np.random.default_rng(10)
    x, y = uneven(rng, 9, dt), uneven(rng, 7, dt)
    z = rng.normal(size=(9, 7, 1)).astype(dt)
    it = build(pkg, x, y, z)
    qx = dev(rng.uniform(x[0], x[-1], nq).astype(dt).clip(x[0], x[-1]))
    qy = dev(rng.uniform(y[0], y[-1], nq).astype(dt).clip(y[0], y[-1]))
    got, plans = jet_traced(capfd, lambda: it.jet(qx, qy, 1))
    expect_jet(plans, "second batch", order=1, vec=0, lv=1, klds=1, gy=1, prepass=0)
    assert len(plans) == 1 and nq > plans[0]["gx"] * 256, plans
    for g, nu in zip(got, parts_of(pkg, 1)):
        h = it if nu == (0, 0) else it.partial(*nu)
        check_bits(to_np(g), to_np(h.interp_array(qx, qy)), f"second batch: part {nu} against its handle")


# ---- 9: host output across the staging chunk ----------------------------------------------------------------------------------
def test_host_output_across_the_staging_chunk(pkg, capfd):
    """f32, 4 lanes, order 1: the three staging slices hold (256 MiB / 3, rounded down to 16 bytes) / 16 B queries; 1000 more
    enter a second chunk, and query 500 of it is out of range.  Rows before it equal the separate handles' rows, rows from it
    on keep the sentinel, the error is Bilinear's with the index of the whole batch."""
    dt, Cn = np.float32, 4
    chunk = ((STAGE_BYTES // 3) & ~15) // (Cn * 4)
    nq, pos = chunk + 1000, chunk + 500
    rng = np.random.default_rng(256)
    x, y = uneven(rng, 9, dt), uneven(rng, 7, dt)
    z = rng.normal(size=(9, 7, Cn)).astype(dt)
    it = build(pkg, x, y, z)
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    qx = rng.uniform(x[0], x[-1], nq).astype(dt).clip(x[0], x[-1])
    qy = rng.uniform(y[0], y[-1], nq).astype(dt).clip(y[0], y[-1])
    dqx, dqy = dev(qx[:pos]), dev(qy[:pos])
    want = [to_np((it if nu == (0, 0) else it.partial(*nu)).interp_array(dqx, dqy)) for nu in parts_of(pkg, 1)]
    qx[pos] = x[-1] + dt(0.25)
    qy[pos + 7] = np.nan
    exp = failure(bil, qx[chunk:], qy[chunk:])
    assert exp[2] == 500 and exp[4] == 0
    bufs = [np.full((nq, Cn), SENTINEL, dt) for _ in range(3)]
    got, plans = jet_traced(capfd, lambda: jet_failure(it, qx, qy, into=bufs))
    assert [p["prepass"] for p in plans] == [1, 1], plans                     # two chunks, the second entered
    expect_jet(plans, "staging chunks", order=1, vec=1, lv=1, klds=1)
    assert got[0] == exp[0] and got[1] == exp[1] and got[2] == pos and got[3:] == exp[3:], (got, exp)
    for k, b in enumerate(bufs):
        check_bits(b[:pos], want[k], f"part {k}: rows before the failure, both chunks")
        assert np.all(b[pos:] == SENTINEL), f"part {k}: rows from the failure on keep the sentinel"


# ---- 10: hostile grids ------------------------------------------------------------------------------------------------------
HOSTILE_PAIRS = (("triple", "uneven"), ("small", "mixed2"))
HOSTILE = [(dt, g, p) for dt in DTYPES for g in hostile_inputs.BICUBIC_GRIDS for p in HOSTILE_PAIRS]


@pytest.mark.parametrize("dt,grid,pair", HOSTILE, ids=[f"{np.dtype(c[0]).name}-{c[1][0]}x{c[1][1]}-{c[2][0]}-{c[2][1]}" for c in HOSTILE])
def test_hostile_grids_are_bit_exact_in_every_part(pkg, dt, grid, pair):
    """The grid and lane builders of tests/test_gpu_bicubic_partial_hostile.py: a spacing of 3 ulps (no power of two: a
    reciprocal for a division or a contracted kl * h - d shows) against an uneven axis, and steps of 2^-40 / 2^-400 against
    adjacent floats followed by steps of 2^10 / 2^100 (subnormal operands); 25 lanes (scalar) and 28 (vectors) of the nine
    recipes and the per-order top-scale and subnormal lanes; both end sets, extrapolation off and on, both orders."""
    (nx, ny), (fx, fy) = grid, pair
    x, y = hostile_inputs.bicubic_grid(fx, fy, dt, nx, ny)
    lanes = hostile_inputs.BICUBIC_PARTIAL_LANES
    z, _ = hostile_inputs.bicubic_partial_nodes(dt, nx, ny, fx, fy, max(lanes))
    for bi, bc in enumerate(hostile_inputs.bicubic_ends()):
        for ext in (False, True):
            qx, qy = hostile_inputs.bicubic_queries(x, y, ext, n_random=300, thin=THIN[nx])
            for Cn in lanes:
                zc = np.ascontiguousarray(z[:, :, :Cn])
                it = build(pkg, x, y, zc, bc, extrapolate=ext)
                want6 = want_parts(x, y, zc, it.strategy.tables(), qx, qy, parts_of(pkg, 2))
                for order in (1, 2):
                    nus = parts_of(pkg, order)
                    what = f"{fx} x {fy} ends={bi} ext={ext} C={Cn} order={order}"
                    check_parts(it.jet(dev(qx), dev(qy), order), want6[:len(nus)], what + " device queries", nus)
                    check_parts(it.jet(qx, qy, order), want6[:len(nus)], what + " host queries", nus)


# ---- 11: refusals through the library ---------------------------------------------------------------------------------------
def test_refusals_through_the_library(pkg):
    import torch
    cap, lib = pkg._capi, pkg._capi.lib()
    rng = np.random.default_rng(21)
    x, y, z = make_grid(rng, 9, 6, 8, np.float32)
    it = build(pkg, x, y, z)
    bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
    par, integ = it.partial(1, 0), it.antiderivative()
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=100)
    nq = len(qx)
    before = it.interp_array(qx, qy)
    dqx, dqy = dev(qx), dev(qy)
    bufs = [torch.full((nq, 8), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(6)]

    def call(h, order, ptrs, stride=8, n=nq, path=cap.PATH_AUTO, async_launch=0, qxp=dqx.data_ptr()):
        opts = cap.EvalOpts()
        opts.q_memspace = opts.out_memspace = cap.MEM_DEVICE
        opts.path, opts.async_launch = path, async_launch
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        info = cap.OobInfo()
        return lib.ndi_interp2d_eval_jet(h.strategy._h, order, qxp, dqy.data_ptr(), n, arr, stride, C.byref(opts), C.byref(info))

    p = [b.data_ptr() for b in bufs]
    cases = (("Bilinear handle", lambda: call(bil, 1, p[:3]), cap.BAD_ARG, "Bilinear has no value-and-gradient"),
             ("partial handle", lambda: call(par, 1, p[:3]), cap.BAD_ARG, "Bicubic: a partial-derivative handle (orders (1, 0))"),
             ("integral handle", lambda: call(integ, 1, p[:3]), cap.BAD_ARG, "Bicubic: an integral handle"),
             ("order 0", lambda: call(it, 0, p), cap.BAD_ARG, "Bicubic: ndi_interp2d_eval_jet takes order 1"),
             ("order 3", lambda: call(it, 3, p), cap.BAD_ARG, "Bicubic: ndi_interp2d_eval_jet takes order 1"),
             ("a null part", lambda: call(it, 2, p[:4] + [None] + p[5:]), cap.BAD_ARG, "Bicubic: ndi_interp2d_eval_jet: outs[4] is null"),
             ("two equal parts", lambda: call(it, 1, [p[0], p[1], p[0]]), cap.BAD_ARG, "outs[0] and outs[2] are the same pointer"),
             ("stride below lanes", lambda: call(it, 1, p[:3], stride=7), cap.BAD_ARG, "out_row_stride (7) < lanes (8)"),
             ("a null query pointer", lambda: call(it, 1, p[:3], qxp=None), cap.BAD_ARG, "null query pointer"),
             ("NDI_PATH_BUCKETED", lambda: call(it, 1, p[:3], path=cap.PATH_BUCKETED), cap.BAD_ARG,
              "Bicubic has no tile-grouped evaluation form"),
             ("async_launch", lambda: call(it, 1, p[:3], async_launch=1), cap.UNSUPPORTED, "ndi_interp2d_partial"))
    for what, f, status, text in cases:
        assert f() == status, (what, cap.last_error())
        msg = cap.last_error()
        assert text in msg and msg.startswith(("Bicubic", "Bilinear")), (what, msg)
        torch.cuda.synchronize()
        assert all(bool((b == SENTINEL).all()) for b in bufs), f"{what}: a refused call wrote"
        check_bits(it.interp_array(qx, qy), before, f"{what}: the source still evaluates")
    # an empty batch touches nothing, whatever the part pointers are
    assert call(it, 1, [None, None, None], n=0) == cap.OK and call(it, 2, [p[0]] * 6, n=0) == cap.OK
    assert call(it, 2, p) == cap.OK                                              # and the accepted call is right
    torch.cuda.synchronize()
    check_parts(bufs, want_parts(x, y, z, it.strategy.tables(), qx, qy, parts_of(pkg, 2)), "after the refusals", parts_of(pkg, 2))
    with pytest.raises(TypeError, match="Bilinear has no value-and-gradient"):
        bil.jet(qx, qy)
    with pytest.raises(ValueError, match="partial-derivative strategy"):
        par.jet(qx, qy)
    with pytest.raises(ValueError, match="integral strategy"):
        integ.value_and_gradient(qx, qy)
    check_bits(par.interp_array(qx, qy), ref.evaluate(x, y, z, *it.strategy.tables(), qx, qy, 1, 0), "the partial still evaluates")


# ---- 12: the surroundings are as they were ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_value_and_partial_paths_are_unchanged(pkg, capfd, dt):
    rng = np.random.default_rng(12)
    x, y, z = make_grid(rng, 9, 6, 8, dt)
    it = build(pkg, x, y, z)
    p = it.partial(1, 1)
    qx, qy = hostile_inputs.bicubic_queries(x, y, n_random=300)
    dqx, dqy = dev(qx), dev(qy)
    v0, plans_v0 = traced(capfd, lambda: it.interp_array(dqx, dqy))
    p0, plans_p0 = traced(capfd, lambda: p.interp_array(dqx, dqy))
    tabs = it.strategy.tables()
    want6 = want_parts(x, y, z, tabs, qx, qy, parts_of(pkg, 2))
    check_bits(to_np(v0), want6[0], "the surface before")
    check_bits(to_np(p0), want6[4], "the (1, 1) partial before")
    for order in (1, 2, 1):
        check_parts(it.jet(dqx, dqy, order), want6[:len(parts_of(pkg, order))], f"jet order {order}", parts_of(pkg, order))
        check_parts(it.jet(qx, qy, order), want6[:len(parts_of(pkg, order))], f"jet order {order}, host", parts_of(pkg, order))
    v1, plans_v1 = traced(capfd, lambda: it.interp_array(dqx, dqy))
    p1, plans_p1 = traced(capfd, lambda: p.interp_array(dqx, dqy))
    check_bits(to_np(v1), to_np(v0), "the surface after jet calls")
    check_bits(to_np(p1), to_np(p0), "the (1, 1) partial after jet calls")
    assert plans_v1 == plans_v0 and plans_p1 == plans_p0 and len(plans_v0) == len(plans_p0) == 1


def test_two_host_threads_on_one_handle(pkg):
    rng = np.random.default_rng(2)
    x, y, z = make_grid(rng, 33, 20, 5, np.float64)
    it = build(pkg, x, y, z)
    tabs = it.strategy.tables()
    jobs = []
    for t in range(2):
        qx, qy = rng.uniform(x[0], x[-1], 5000 + 7 * t), rng.uniform(y[0], y[-1], 5000 + 7 * t)
        jobs.append(dict(qx=qx, qy=qy, order=1 + t, want=want_parts(x, y, z, tabs, qx, qy, parts_of(pkg, 1 + t)), got=[], err=[]))

    def work(j):
        try:
            for rep in range(20):
                q = (dev(j["qx"]), dev(j["qy"])) if rep % 2 else (j["qx"], j["qy"])
                j["got"].append([to_np(g) for g in it.jet(*q, j["order"])])
        except BaseException as e:  # noqa: BLE001
            j["err"].append(e)

    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for j in jobs:
        assert not j["err"], j["err"]
        assert len(j["got"]) == 20
        for got in j["got"]:
            check_parts(got, j["want"], f"thread of order {j['order']}", parts_of(pkg, j["order"]))


# ---- 13: under the bounds-checked library -----------------------------------------------------------------------------------
def test_small_shapes_and_pieces_under_the_bounds_checked_library():
    """Case 1's small shapes and case 3 in a fresh child process that loads the bounds-checked build: a device-side index out
    of range (cell, strip, table) fails the call."""
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib), "build() makes the checked library"
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from conftest import load_product_package; import test_gpu_bicubic_jet as t\n"
        "pkg = load_product_package()\n"
        "for dt in (np.float32, np.float64):\n"
        "    for shape in ((5, 7, 3), (9, 6, 8)):\n"
        "        for even in (False, True):\n"
        "            t.run_hostile_queries(pkg, dt, shape, even)\n"
        "    t.run_pieces(pkg, dt)\n"
        "print('checked OK')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, NDI_LIB=lib), timeout=600)
    assert r.returncode == 0 and "checked OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
