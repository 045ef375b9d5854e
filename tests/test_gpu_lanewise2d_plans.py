"""GPU: the instances of eval_lanewise2d_kernel<T, KIND, STAGE, REC, NUX, NUY, WRAP> and the host paths of
ndi_interp2d_eval_lanewise (csrc/lanewise2d_host.hpp) that tests/test_gpu_lanewise2d.py leaves out:

  the unstaged form at f32, with the long axis on y, on a wrapping axis and with partial orders; both pyramids staged with
  two levels each; the LDS occupancy cap of the grid; all eight partial orders of a wrapping handle; a wrapped coordinate
  one ulp past the last knot (where the pre-pass and the kernel wrap separately); the partials of the local builds; the
  node-record copy under two streams and eight threads, and above its 1 GiB cap; the second chunk of host staging with the
  first-error report across the chunk boundary.

The helpers are that file's (traced, expect, run, raw_call, surface, per_lane, pool_case): every case asserts the
`[ndi plan] lanewise2d` line of the call under test, runs under NDI_LANEWISE2D_RECORDS 0 and 1 where the handle is Bicubic,
through the output-owning call (check=1) and the call into a caller's buffer (check=0), and is compared bit for bit
(hostile_inputs.check_bits) with the row-wise evaluation of the same handle."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import bicubic_periodic_ref
import hostile_inputs
import inverse_cases as ic
from conftest import ROOT
from test_gpu_bicubic_periodic_plans import past_end_axis
from test_gpu_lanewise2d import (BLOCK, DTYPES, SENTINEL, expect, grid_data, per_lane, periodic_grid, pool_case, queries, raw_call,
                                 run, surface, tdt, traced, wrap_queries)

pytestmark = pytest.mark.gpu

ORDERS = [(a, b) for a in range(3) for b in range(3) if (a, b) != (0, 0)]
WRAP = {1: "x", 2: "y", 3: "xy"}
LDS_STAGE_LIMIT = 150 * 1024          # csrc/ndinterp_api.hip
LDS_CU = 160 * 1024                   # lanewise_enqueue: per_cu = min(wgs, 160 KiB / shmem)
WGS_DEFAULT = 8                       # lanewise_knobs: NDI_LANEWISE_WGS


def pyramid(n, itemsize):
    """DevicePyramid::upload: (block, n1, levels, lds_bytes) -- block the power of two with 64 block >= n, n1 = ceil(n / block)
    top-level entries, two levels above 64 knots, both levels one allocation"""
    block = 1
    while 64 * block < n:
        block *= 2
    n1 = -(-n // block)
    return block, n1, 1 if n <= 64 else 2, (n + n1) * itemsize


def shmem(nx, ny, itemsize):
    """lanewise_enqueue: the bytes of both pyramids, rounded up to 16"""
    return (pyramid(nx, itemsize)[3] + pyramid(ny, itemsize)[3] + 15) & ~15


def partial_of(it, nu):
    return it if tuple(nu) == (0, 0) else it.partial(*nu)


# ---- unstaged forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bilinear", "pchip"])
def test_unstaged_f32(pkg, monkeypatch, capfd, kind):
    """40 001 f32 knots and their 40 top-level entries are 160 164 bytes, above the 150 KiB stage limit: the STAGE = 0
    instances at f32"""
    dt = np.float32
    nx, ny, L, Q = 40001, 3, 2, 257
    assert shmem(nx, ny, 4) > LDS_STAGE_LIMIT and pyramid(nx, 4)[:2] == (1024, 40)
    rng = np.random.default_rng(21)
    x, y = ic.knots(rng, nx, dt), ic.knots(rng, ny, dt)
    it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, dt))
    xs, ys = queries(rng, x, y, Q, L)
    run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind} 40001 x 3 x 2 f32", stage=0, wrap="none")


def run_unstaged_y(pkg, monkeypatch, capfd, kind):
    dt = np.float64
    nx, ny, L, Q = 3, 20001, 2, 257
    assert shmem(nx, ny, 8) > LDS_STAGE_LIMIT
    rng = np.random.default_rng(22)
    x, y = ic.knots(rng, nx, dt), ic.knots(rng, ny, dt)
    it = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, dt))
    xs, ys = queries(rng, x, y, Q, L)
    xs[:8], ys[:8] = x[1], rng.uniform(y[-2], y[-1], (8, L))       # the last cell of the long axis, from the last row but one
    xs[8:16] = rng.uniform(x[1], x[2], (8, L))                      # the last grid row: node (nx - 2) * ny + yi and ny more
    run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind} 3 x 20001 x 2", stage=0, wrap="none")


@pytest.mark.parametrize("kind", ["bilinear", "spline"])
def test_unstaged_with_the_long_axis_on_y(pkg, monkeypatch, capfd, kind):
    """3 x 20 001 x 2 at f64: the node stride PY.n and the record stride PY.n * L take their large values (a step from grid row
    i to i + 1 is 20 001 nodes), and the y search is the one that reads global memory through two levels"""
    run_unstaged_y(pkg, monkeypatch, capfd, kind)


def run_unstaged_wrap(pkg, monkeypatch, capfd, axes, orders):
    dt = np.float64
    n, L, Q = 20001, 2, 257
    rng = np.random.default_rng([23, axes])
    long_axis = (ic.knots(rng, n, dt) - dt(1.5)).astype(dt)
    short = ic.knots(rng, 3, dt)
    x, y = (long_axis, short) if axes == 1 else (short, long_axis)
    assert shmem(len(x), len(y), 8) > LDS_STAGE_LIMIT
    z = periodic_grid(rng, len(x), len(y), L, dt, axes)
    src = surface(pkg, "spline", x, y, z, extrapolate=True, periodic=axes)
    xs, ys = wrap_queries(rng, x, Q, L, axes & 1), wrap_queries(rng, y, Q, L, axes & 2)
    for nu in orders:
        it = partial_of(src, nu)
        run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"20001 periodic knots on {WRAP[axes]}, order {nu}",
            stage=0, wrap=WRAP[axes], nu_x=nu[0], nu_y=nu[1])


@pytest.mark.parametrize("axes", [1, 2])
def test_unstaged_on_a_wrapping_axis(pkg, monkeypatch, capfd, axes):
    """20 001 periodic f64 knots on x, then on y, of a handle built with extrapolate: STAGE = 0 x WRAP, at the orders (0, 0),
    (1, 2) and (2, 1) -- STAGE = 0 x a partial order; x0, xn of the wrap are then read from global memory"""
    run_unstaged_wrap(pkg, monkeypatch, capfd, axes, [(0, 0), (1, 2), (2, 1)])


# ---- both axes staged with upper levels -----------------------------------------------------------------------------------------------
def run_two_levels(pkg, monkeypatch, capfd, kind, dt):
    n, L, Q = 65, 2, 257
    block, n1, levels, _ = pyramid(n, np.dtype(dt).itemsize)
    assert (block, n1, levels) == (2, 33, 2) and shmem(n, n, np.dtype(dt).itemsize) <= LDS_STAGE_LIMIT
    rng = np.random.default_rng([24, np.dtype(dt).itemsize])
    x, y = ic.knots(rng, n, dt), ic.knots(rng, n, dt)
    it = surface(pkg, kind, x, y, grid_data(rng, n, n, L, dt))
    xs, ys = queries(rng, x, y, Q, L)
    T = np.dtype(dt).type
    for k, q in ((x, xs), (y, ys)):
        inner = k[1:-1]
        for l in range(L):
            for s in (k, np.nextafter(inner, T(np.inf)), np.nextafter(inner, T(-np.inf))):
                assert np.isin(s, q[:, l]).all()
    run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind} 65 x 65 x 2 {np.dtype(dt).name}", stage=1, wrap="none")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["bilinear", "pchip"])
def test_both_pyramids_staged_with_two_levels(pkg, monkeypatch, capfd, kind, dt):
    """65 knots on BOTH axes, the length at which test_pyramid_levels_on_a_wrapping_axis of the periodic plans file gets its
    second level.  How the case knows: DevicePyramid::upload (csrc/ndinterp_api.hip) sets levels = n <= 64 ? 1 : 2 and
    block = the least power of two with 64 block >= n, so n = 65 gives block = 2, levels = 2 and n1 = ceil(65 / 2) = 33
    top-level entries, the last block holding one knot (`pyramid` above restates the rule and the case asserts it); the two
    pyramids are 2 x 98 elements, far below the stage limit, and the plan line says stage=1.  The LDS layout is then
    [x lv0 (65) | x lv1 (33) | y lv0 (65) | y lv1 (33)] with PY.lv0 = PX.lv0 + 98: a y level based at PX.lv0 + 65 would search
    x's top level.  Every lane meets every knot of both axes and the floats either side (asserted)."""
    run_two_levels(pkg, monkeypatch, capfd, kind, dt)


# ---- the LDS occupancy cap ------------------------------------------------------------------------------------------------------------
def probe(pkg, monkeypatch, capfd, wgs):
    """probe_grid of tests/test_gpu_lanewise2d.py with NDI_LANEWISE_WGS = wgs (None: unset, the knob's default): the grid of a
    batch that fills it, on a 3 x 3 grid whose pyramids (48 bytes) the cap does not touch"""
    import torch
    if wgs is None:
        monkeypatch.delenv("NDI_LANEWISE_WGS", raising=False)
    else:
        monkeypatch.setenv("NDI_LANEWISE_WGS", str(wgs))
    x = np.arange(3.0)
    it = surface(pkg, "bilinear", x, x.copy(), np.zeros((3, 3, 256)))
    q = torch.full((4097, 256), 0.5, dtype=torch.float64, device="cuda:0")
    with traced(capfd) as t:
        it.interp_lanewise(q, q)
    expect(t.plans, "probe", n=1)
    return t.plans[0]["grid"]


@pytest.mark.parametrize("n,per_cu", [(12001, 1), (6001, 3)])
@pytest.mark.parametrize("kind", ["bilinear", "pchip"])
def test_the_lds_cap_sets_the_grid(pkg, monkeypatch, capfd, kind, n, per_cu):
    """12 001 f64 knots with their 47 top-level entries and the 3-knot y axis are 96 432 bytes of LDS: one workgroup fits a CU
    (160 KiB / 96 432 = 1); 6 001 knots are 48 432 bytes: three fit.  The knob asks for 8.  The grid of a batch large enough
    for 8 per CU is per_cu x the grid of a NDI_LANEWISE_WGS=1 probe, not the grid of a probe at the knob's default."""
    g1 = probe(pkg, monkeypatch, capfd, 1)
    g8 = probe(pkg, monkeypatch, capfd, None)
    assert g8 == WGS_DEFAULT * g1 and 4097 * 256 >= BLOCK * g8, (g1, g8)
    sh = shmem(n, 3, 8)
    assert sh <= LDS_STAGE_LIMIT and min(WGS_DEFAULT, LDS_CU // sh) == per_cu, sh
    assert n != 12001 or 80 * 1024 < sh < 150 * 1024
    L = 2
    Q = BLOCK * g8 // L + 1                                # more elements than 8 workgroups per CU take in one trip
    rng = np.random.default_rng([25, n])
    x, y = ic.knots(rng, n, np.float64), ic.knots(rng, 3, np.float64)
    it = surface(pkg, kind, x, y, grid_data(rng, n, 3, L, np.float64))
    xs, ys = queries(rng, x, y, Q, L)
    p = run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind} {n} x 3 x 2, the LDS cap", stage=1, grid=per_cu * g1)
    assert p["grid"] < g8 and Q * L > BLOCK * g8


# ---- all eight non-zero orders of a wrapping handle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("axes", [1, 2, 3])
def test_every_partial_order_of_a_wrapping_handle(pkg, monkeypatch, capfd, dt, axes):
    """9 x 7 x 5, Q = 67, periodic on x, y and both with extrapolate: the WRAP instances of the eight orders, host arrays and
    device tensors.  (1, 2) and (2, 1) are where a dispatch that transposes the orders shows."""
    rng = np.random.default_rng([26, axes])
    nx, ny, L, Q = 9, 7, 5, 67
    x = (ic.knots(rng, nx, dt) - dt(1.5)).astype(dt)
    y = (ic.knots(rng, ny, dt) - dt(0.75)).astype(dt)
    src = surface(pkg, "spline", x, y, periodic_grid(rng, nx, ny, L, dt, axes), extrapolate=True, periodic=axes)
    xs, ys = wrap_queries(rng, x, Q, L, axes & 1), wrap_queries(rng, y, Q, L, axes & 2)
    for nu in ORDERS:
        it = src.partial(*nu)
        run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"wrap {WRAP[axes]}, partial {nu} {np.dtype(dt).name}",
            stage=1, wrap=WRAP[axes], nu_x=nu[0], nu_y=nu[1])


# ---- a wrapped coordinate one ulp past the last knot -----------------------------------------------------------------------------------
def run_past_end(pkg, monkeypatch, capfd, dt, axes, even):
    """past_end_axis of the periodic plans file on every wrapping axis: nextafter(k0, -inf) wraps to one ulp ABOVE kn.  The
    query sits in several lanes of rows among ordinary ones and in the last element of the batch; 67 rows of 5 lanes are
    335 elements, 5 full waves and a tail of 15 whose 49 inactive lanes go through the wrap with the first knots."""
    import torch
    cap = pkg._capi
    T = np.dtype(dt).type
    nx, ny, L, Q = 9, 7, 5, 67
    assert (Q * L) % 64 != 0
    rng = np.random.default_rng([27, axes, even, np.dtype(dt).itemsize])
    x = past_end_axis(rng, nx, dt, even) if axes & 1 else (ic.knots(rng, nx, dt) - dt(1.5)).astype(dt)
    y = past_end_axis(rng, ny, dt, even) if axes & 2 else (ic.knots(rng, ny, dt) - dt(0.75)).astype(dt)
    src = surface(pkg, "spline", x, y, periodic_grid(rng, nx, ny, L, dt, axes), extrapolate=True, periodic=axes)
    xs, ys = wrap_queries(rng, x, Q, L, axes & 1), wrap_queries(rng, y, Q, L, axes & 2)
    # (both axes wrapping: three elements with both coordinates past the end, two with x alone, two with y alone)
    spots = {1: [(3, 0), (20, 2), (41, 4), (64, 1), (Q - 1, L - 1)], 2: [(5, 0), (20, 2), (41, 4), (60, 3), (Q - 1, L - 1)]}
    for k, q, bit in ((x, xs, 1), (y, ys, 2)):
        if not axes & bit:
            continue
        below = np.nextafter(k[0], T(-np.inf))
        assert bicubic_periodic_ref.wrap(k, np.array([below], dt))[0] == np.nextafter(k[-1], T(np.inf))
        for j, l in spots[bit]:
            q[j, l] = below
    for nu in ((0, 0), (2, 2)):
        it = partial_of(src, nu)
        ref = per_lane(it, xs, ys)                          # the row-wise handle accepts the query: it raises otherwise
        assert np.isfinite(ref).all()
        run(pkg, monkeypatch, capfd, it, xs, ys, ref, f"past the end, wrap {WRAP[axes]}, order {nu} {np.dtype(dt).name} even={even}",
            stage=1, wrap=WRAP[axes], nu_x=nu[0], nu_y=nu[1])
    # +inf wraps to NaN and is refused: the pre-pass (check=0) and the kernel (check=1) wrap separately and must agree
    bx, by = xs.copy(), ys.copy()
    (by if axes == 2 else bx)[41, 4] = np.inf
    axis = 1 if axes == 2 else 0
    ref = per_lane(src, xs, ys)
    dx, dy = torch.as_tensor(bx, device="cuda:0"), torch.as_tensor(by, device="cuda:0")
    for flags in (0, cap.EVAL_FRESH_OUTPUT):
        out = torch.full((Q, L), SENTINEL, dtype=tdt(dt), device="cuda:0")
        with traced(capfd) as t:
            st, info = raw_call(pkg, src, dx, dy, Q, L, out, L, q_dev=True, out_dev=True, flags=flags)
        expect(t.plans, "inf on a wrapping axis", n=1, wrap=WRAP[axes], check=int(flags != 0))
        assert (st, info.index, info.axis, info.value) == (cap.NAN_QUERY, 41 * L + 4, axis, float("inf")), \
            (flags, st, info.index, info.axis, info.value)
        hostile_inputs.check_bits(out[:41].cpu().numpy(), ref[:41], f"inf on a wrapping axis, flags = {flags}: rows before it")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("axes", [1, 2, 3])
def test_wrapped_coordinate_past_the_last_knot(pkg, monkeypatch, capfd, dt, axes):
    """the lane-wise twin of the periodic plans file's test of that name: the search clamps to the last cell and t is just over
    1; accepted, and the same bits as the row-wise handle, whether lanewise2d_check_kernel (check=0) or the evaluation kernel
    (check=1) tests it; with the O(1) guess (even knots) and through the search"""
    for even in (True, False):
        run_past_end(pkg, monkeypatch, capfd, dt, axes, even)


# ---- partials of the local builds ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["pchip", "akima", "hermite"])
def test_every_partial_order_of_the_local_builds(pkg, monkeypatch, capfd, dt, kind):
    """test_every_partial_order on Pchip, Akima and caller-given node derivatives, whose second partials jump at grid lines:
    the queries hold every knot of either axis"""
    rng = np.random.default_rng(28)
    nx, ny, L, Q = 9, 7, 5, 67
    x, y = ic.knots(rng, nx, dt), ic.knots(rng, ny, dt)
    src = surface(pkg, kind, x, y, grid_data(rng, nx, ny, L, dt))
    xs, ys = queries(rng, x, y, Q, L)
    assert np.isin(x[1:-1], xs).all() and np.isin(y[1:-1], ys).all()
    for nu in ORDERS:
        it = src.partial(*nu)
        run(pkg, monkeypatch, capfd, it, xs, ys, per_lane(it, xs, ys), f"{kind}, partial {nu} {np.dtype(dt).name}",
            nu_x=nu[0], nu_y=nu[1], stage=1, wrap="none")


# ---- the record copy under concurrency -----------------------------------------------------------------------------------------------
def records_case(pkg):
    rng = np.random.default_rng(29)
    nx, ny, L, Q = 9, 7, 5, 67
    x, y = ic.knots(rng, nx, np.float64), ic.knots(rng, ny, np.float64)
    z = grid_data(rng, nx, ny, L, np.float64)
    xs, ys = queries(rng, x, y, Q, L)
    ref = per_lane(surface(pkg, "pchip", x, y, z), xs, ys)
    return (lambda: surface(pkg, "pchip", x, y, z)), xs, ys, ref


def test_first_calls_on_two_streams(pkg, monkeypatch, capfd):
    """a first call on one stream and at once, with no synchronisation between, a second on another stream: one build, both
    results the reference's.  (Which state the second call meets -- ready, or built on another stream and waited for through
    the event -- depends on the first call's read-back and is not asserted.)"""
    import torch
    make, xs, ys, ref = records_case(pkg)
    monkeypatch.setenv("NDI_LANEWISE2D_RECORDS", "1")
    it = make()
    dx, dy = torch.as_tensor(xs, device="cuda:0"), torch.as_tensor(ys, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with traced(capfd) as t:
        with torch.cuda.stream(s1):
            a = it.interp_lanewise(dx, dy)
        with torch.cuda.stream(s2):
            b = it.interp_lanewise(dx, dy)
    torch.cuda.synchronize()
    expect(t.plans, "two streams", n=2, kind="bicubic", records=1, check=1)
    assert t.built == 1, t.built
    hostile_inputs.check_bits(a.cpu().numpy(), ref, "the first stream")
    hostile_inputs.check_bits(b.cpu().numpy(), ref, "the second stream")


def test_first_calls_from_eight_threads(pkg, monkeypatch, capfd):
    """eight host threads make the first call on one fresh handle, released together: the `build` mutex lets one of them
    build; eight correct results"""
    make, xs, ys, ref = records_case(pkg)
    monkeypatch.setenv("NDI_LANEWISE2D_RECORDS", "1")
    it = make()
    N = 8
    got, errors = [None] * N, []
    gate = threading.Barrier(N)

    def work(i):
        try:
            gate.wait(timeout=60)
            got[i] = it.interp_lanewise(xs, ys)
        except Exception as e:       # noqa: BLE001
            errors.append((i, repr(e)))
    with traced(capfd) as t:
        threads = [threading.Thread(target=work, args=(i,)) for i in range(N)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=120)
    assert not errors and not any(th.is_alive() for th in threads), errors
    expect(t.plans, "eight threads", n=N, kind="bicubic", records=1, check=1)
    assert t.built == 1, t.built
    for i in range(N):
        hostile_inputs.check_bits(got[i], ref, f"thread {i}")


# ---- the record cap ----------------------------------------------------------------------------------------------------------------------
def test_the_record_cap(pkg, monkeypatch, capfd):
    """Pchip f64, 2 x 2 x 8 388 609: the record copy would be 4 nodes x 8 388 609 lanes x 32 bytes = 2^30 + 128, one lane's four
    records over LanewiseRecords::LIMIT = 1 GiB.  So NDI_LANEWISE2D_RECORDS=1 still reads the plain table (records=0), and no
    later call retries.  Data drawn on the device; the yardstick is pool_case with a pool of 4 points (the corners)."""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    assert free > 6 * 2**30, "the test needs 6 GB of free device memory"
    monkeypatch.setenv("NDI_LANEWISE2D_RECORDS", "1")
    nx, ny, L, Q = 2, 2, 8_388_609, 2
    assert nx * ny * L * 4 * 8 == (1 << 30) + 128
    g = torch.Generator(device="cuda:0").manual_seed(30)
    z = torch.randn((nx, ny, L), generator=g, device="cuda:0", dtype=torch.float64)
    x, y = np.array([0.0, 1.5]), np.array([-1.0, 0.25])
    it = pkg.Interp2D.builder(z).x(torch.as_tensor(x, device="cuda:0")).y(torch.as_tensor(y, device="cuda:0")) \
        .strategy(pkg.Bicubic.pchip()).build()
    try:
        xs, ys, ref = pool_case(it, x, y, Q, L, 31, K=4)
        dx, dy = torch.as_tensor(xs, device="cuda:0"), torch.as_tensor(ys, device="cuda:0")
        for what in ("above the record cap", "above the record cap, second call"):      # ... and no later call retries
            with traced(capfd) as t:
                got = it.interp_lanewise(dx, dy)
            expect(t.plans, what, n=1, kind="bicubic", records=0, check=1)
            assert t.built == 0
            hostile_inputs.check_bits(got.cpu().numpy(), ref, what)
            del got
        buf = torch.full((Q, L), SENTINEL, dtype=torch.float64, device="cuda:0")
        with traced(capfd) as t:
            it.interp_lanewise_into(dx, dy, buf)
        expect(t.plans, "above the record cap, a caller's buffer", n=1, records=0, check=0)
        hostile_inputs.check_bits(buf.cpu().numpy(), ref, "above the record cap, a caller's buffer")
    finally:                                       # a failure must not hold 1.5 GiB for the tests that follow
        got = buf = dx = dy = z = None
        it.strategy.release()
        torch.cuda.empty_cache()


# ---- host staging in two chunks --------------------------------------------------------------------------------------------------------------
def test_host_staging_in_two_chunks(pkg, capfd):
    """Bilinear f32 on scalar data, 5 x 5, Q = 2^26 + 1000 host queries: a chunk of lanewise2d_run is 256 MiB per array =
    2^26 rows of 4 bytes, so the loop runs a second time with off = 2^26 (two plan lines).  Then failures planted in chunk 1:
    the report's index is row0 * lanes + f, its value is read from q + j * q_stride + l of the failing AXIS' array."""
    cap = pkg._capi
    dt = np.float32
    rng = np.random.default_rng(32)
    n, C0 = 5, 1 << 26
    Q = C0 + 1000
    x, y = ic.knots(rng, n, dt), ic.knots(rng, n, dt)
    it = surface(pkg, "bilinear", x, y, rng.normal(size=(n, n)).astype(dt))

    def draw(k):
        q = rng.random(Q, dtype=np.float32) * (k[-1] - k[0]) + k[0]
        return np.clip(q, k[0], k[-1], out=q)
    qx, qy = draw(x), draw(y)
    qx[:3], qy[:3] = [x[0], x[-1], x[2]], [y[-1], y[0], y[2]]
    qx[C0 - 1:C0 + 2] = [x[1], x[-1], x[0]]                # the last row of chunk 0, the first rows of chunk 1
    qy[C0 - 1:C0 + 2] = [y[-1], y[0], y[3]]
    ref = it.interp_array(qx, qy)
    assert ref.shape == (Q,)
    with traced(capfd) as t:
        got = it.interp_lanewise(qx, qy)
    expect(t.plans, "two chunks", n=2, kind="bilinear", stage=1, check=1)
    hostile_inputs.check_bits(got, ref, "two chunks")
    del got
    bad = C0 + 7
    y_hi, x_hi, x_lo = np.nextafter(y[-1], dt(np.inf)), np.nextafter(x[-1], dt(np.inf)), np.nextafter(x[0], dt(-np.inf))
    assert x_lo != y_hi
    qy[bad] = y_hi                                          # the lowest failing element fails on y ...
    qx[bad + 50] = x_hi                                     # ... a later one on x
    qy[bad + 100] = np.nan
    buf = np.full(Q, SENTINEL, dt)
    for what, axis, value in (("y in chunk 1", 1, y_hi), ("x and y in the same element: x is reported", 0, x_lo)):
        if axis == 0:
            qx[bad] = x_lo
        buf[:] = SENTINEL
        st, info = raw_call(pkg, it, qx, qy, Q, 1, buf, 1, q_dev=False, out_dev=False)
        assert (st, info.index, info.axis, info.status) == (cap.OUT_OF_BOUNDS, bad, axis, cap.OUT_OF_BOUNDS), \
            (what, st, info.index, info.axis, cap.last_error())
        assert info.value == float(value), (what, info.value, float(value))
        assert cap.last_error().startswith("xy"[axis] + " = "), (what, cap.last_error())
        hostile_inputs.check_bits(buf[:bad], ref[:bad], what + ": the rows before the failing query, across the chunk boundary")
        assert np.all(buf[bad:] == SENTINEL), what


# ---- the bounds-checked library ------------------------------------------------------------------------------------------------------------------
def test_checked_cases(pkg, monkeypatch, capfd):
    """what runs again under the bounds-checked library (below): the unstaged form with the long axis on y (Bilinear and the
    spline, both record settings), unstaged x wrap x records at the order (1, 2), two levels on both staged axes, and the
    wrapped coordinate one ulp past the last knot on both axes"""
    for kind in ("bilinear", "spline"):
        run_unstaged_y(pkg, monkeypatch, capfd, kind)
    run_unstaged_wrap(pkg, monkeypatch, capfd, 2, [(1, 2)])
    run_two_levels(pkg, monkeypatch, capfd, "pchip", np.float64)
    run_past_end(pkg, monkeypatch, capfd, np.float32, 3, False)


def test_the_bounds_checked_library_runs_clean():
    """NDI_CHK on p.j / p.l, on both cell indices and on the record copy's node index: a cell past the grid or a node index
    formed with the wrong stride fails the call"""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lanewise2d_plans.py"), "-m", "gpu", "-x",
                        "-q", "-k", "test_checked_cases"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
