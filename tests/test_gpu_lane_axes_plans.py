"""GPU: the forms of the lane-axes kernels (csrc/lane_axes_kernels.hpp) and the paths of the host engine through this family
(csrc/lane_axes_host.hpp, FloatEngine::eval_body, lanewise_run) that tests/test_gpu_lane_axes.py leaves out:

  columns of 4097 knots against the shared-axis search through its pyramid (the single-column handles) and through its
  bucket index (the column in three identical lanes), and against the oracle; the oracle per column for every end kind, in range and with extrapolation; the second grid-stride trip of
  lane_axes_records_kernel (n * lanes > 2^24); a cubic handle above the 1 GiB cap of the record copy, whose launch must pick
  the REC = false instance; host arrays that need a second 256 MiB chunk, with the first-error report and the output
  pointer behind the chunk boundary; a padded out_row_stride on the row-wise call, strides below `lanes`, empty batches,
  async_launch with finish, and eight threads on one handle.

The helpers are that file's (build, ref_rows, ref_lanewise, assert_bits, own_queries, common_queries).  Every comparison is
bit for bit on the integer views, zero signs included: the contract of include/ndinterp.h, so there is no tolerance."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle
from test_gpu_lane_axes import (STRATEGIES, assert_bits, build, columns, common_queries, mixed_boundary, own_queries, ref_lanewise, ref_rows,
                                table)
from test_gpu_lazy_tables import has, traced

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
SENTINEL = -77.0
MIXED = ((oracle.BC_FIRST_DERIV, 0.5), (oracle.BC_SECOND_DERIV, -1.0))      # mixed_boundary of tests/test_gpu_lane_axes.py
ORACLE_ENDS = {"CubicSpline": ((oracle.BC_NOT_A_KNOT, 0.0), (oracle.BC_NOT_A_KNOT, 0.0)),
               "CubicSpline-natural": ((oracle.BC_NATURAL, 0.0), (oracle.BC_NATURAL, 0.0)),
               "CubicSpline-clamped": ((oracle.BC_CLAMPED, 0.0), (oracle.BC_CLAMPED, 0.0)),
               "CubicSpline-mixed": MIXED}


def tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def tables_of(refs):
    return (np.concatenate([r.strategy.coefficients()[k] for r in refs], axis=1) for k in (0, 1))


# ---- 1: long columns ------------------------------------------------------------------------------------------------------------
def knot_queries(x, seed=0):
    """A query per lane, (4n - 1, lanes): every knot of the lane, the float either side of it clipped into the lane's range,
    every midpoint; the rows shuffled per lane so that the lanes of a row sit in different intervals."""
    T = x.dtype.type
    rng = np.random.default_rng([x.shape[0], seed])
    cols = []
    for l in range(x.shape[1]):
        c = x[:, l]
        q = np.concatenate([c, np.nextafter(c, T(np.inf)), np.nextafter(c, T(-np.inf)),
                            (0.5 * (c[1:].astype(np.float64) + c[:-1])).astype(x.dtype)])
        cols.append(np.clip(q, c[0], c[-1])[rng.permutation(q.size)])
    return np.ascontiguousarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["Linear", "Pchip", "CubicSpline", "CubicSpline-mixed"])
def test_long_columns_against_the_accelerated_search(pkg, monkeypatch, capfd, dt, name):
    """4097 knots in 3 lanes -- a linear, a geometric and a jittered column -- and 16 387 queries per lane: the per-lane binary
    search against the shared-axis search in both of its states, and lane_axes_spline_kernel over 4095 interior rows of the
    Thomas recurrence.  A handle of one lane never builds the bucket index below two million queries (interp1d_host.hpp,
    plan_small1: one or two lanes take eval_small_kernel, which searches the pyramid staged in LDS and prints no plan line),
    so the yardstick is twofold: the single-column handles (the pyramid), and the column in three identical lanes with the
    short-row knobs of tests/test_gpu_lazy_tables.py, whose `fused tables=memory` line must show lut=1 (plan_fused1: the
    bucket index from 4096 queries on); element 0 of its rows is the single-column value.  CubicSpline tables and rows also
    against the oracle per column."""
    import torch
    for k, v in (("NDI_SHORT_MODE", 2), ("NDI_FUSED_LDS", 0), ("NDI_FUSED_PACK", 0)):
        monkeypatch.setenv(k, str(v))
    n, L = 4097, 3
    x = np.ascontiguousarray(columns(n, 4, dt)[:, [0, 2, 3]])
    rng = np.random.default_rng(41)
    y = (np.sin(3.0 * x) + rng.uniform(-0.2, 0.2, x.shape)).astype(dt)
    it, refs = build(pkg, name, x, y, y)
    what = f"{name} 4097 x 3 {np.dtype(dt).name}"
    if name != "Linear":
        a, b = it.strategy.coefficients()
        ra, rb = tables_of(refs)
        assert_bits(a, ra, what + " a")
        assert_bits(b, rb, what + " b")
    q2 = knot_queries(x)
    assert q2.shape[0] > 4096
    lo, hi = x[0].max(), x[-1].min()
    q = np.unique(q2[(q2 >= lo) & (q2 <= hi)])
    assert q.size > 4096 and q[0] == lo and q[-1] == hi
    ref2, ref = ref_lanewise(refs, q2), ref_rows(refs, q)
    # the same columns behind the bucket index
    qd, q2d = torch.as_tensor(q, device="cuda:0"), torch.as_tensor(q2, device="cuda:0")
    wide = []
    for l in range(L):
        col = np.ascontiguousarray(np.repeat(y[:, l:l + 1], 3, axis=1))
        wide.append(pkg.Interp1D.builder(col).x(np.ascontiguousarray(x[:, l])).strategy(STRATEGIES[name][1](pkg, col, col.shape)).build())
    with traced(capfd) as t:
        idx2 = np.stack([r.interp_array(q2d[:, l].contiguous()).cpu().numpy()[:, 0] for l, r in enumerate(wide)], axis=1)
        idx = np.stack([r.interp_array(qd).cpu().numpy()[:, 0] for r in wide], axis=1)
    fused = [ln for ln in t.plans if ln.startswith("[ndi plan] fused tables=memory")]
    # (DevicePyramid::build_bucket_index makes no index for an axis whose O(1) guess is exact, which an evenly spaced column
    #  may be: the geometric and the jittered column are the ones that must show it)
    assert len(fused) == 2 * L and all("lut=1" in fused[i] for i in (1, 2, 4, 5)), t.plans
    assert_bits(idx2, ref2, what + ": the bucket index and the pyramid find the same cells, a query per lane")
    assert_bits(idx, ref, what + ": the bucket index and the pyramid find the same cells")
    assert_bits(it.interp_lanewise(q2), ref2, what + " interp_lanewise")
    assert_bits(it.interp_array(q), ref, what + " interp_array")
    assert_bits(it.interp_lanewise(q2d).cpu().numpy(), idx2, what + " interp_lanewise, device queries")
    assert_bits(it.interp_array(qd).cpu().numpy(), idx, what + " interp_array, device queries")
    if name == "Pchip":
        return
    for l in range(L):
        xc, yc = np.ascontiguousarray(x[:, l]), np.ascontiguousarray(y[:, l])
        if name == "Linear":
            st, _, want = oracle.interp1d_linear(xc, yc, q)
            st2, _, want2 = oracle.interp1d_linear(xc, yc, q2[:, l])
        else:
            left, right = ORACLE_ENDS[name]
            st, oa, ob = oracle.cubic_build(xc, yc, left=left, right=right)
            assert st == oracle.OK
            assert_bits(a[:, l], oa[:, 0], f"{what} oracle a lane {l}")
            assert_bits(b[:, l], ob[:, 0], f"{what} oracle b lane {l}")
            st, _, want = oracle.interp1d_cubic(xc, yc, oa, ob, q)
            st2, _, want2 = oracle.interp1d_cubic(xc, yc, oa, ob, q2[:, l])
        assert st == oracle.OK and st2 == oracle.OK
        assert_bits(ref[:, l], want[:, 0], f"{what} oracle rows lane {l}")
        assert_bits(ref2[:, l], want2[:, 0], f"{what} oracle lane-wise rows lane {l}")


# ---- 2: the oracle per column for every end kind ------------------------------------------------------------------------------------
def oracle_ends_case(pkg, dt, name, n, extrapolate):
    L = 3
    x, y, _ = table(n, L, dt)
    make = {"CubicSpline": lambda: pkg.CubicSpline.new(),
            "CubicSpline-natural": lambda: pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Natural),
            "CubicSpline-clamped": lambda: pkg.CubicSpline.new().boundary(pkg.BoundaryCondition.Clamped),
            "CubicSpline-mixed": lambda: pkg.CubicSpline.new().boundary(mixed_boundary(pkg, y.shape))}[name]
    it = pkg.Interp1D.builder(y).lane_axes(x).strategy(make().extrapolate(extrapolate)).build()
    a, b = it.strategy.coefficients()
    q, lo, hi = common_queries(x, 65)
    q2 = own_queries(x)
    if extrapolate:     # below and above every lane's own range, and just outside the common one
        T = np.dtype(dt).type
        q = np.concatenate([q, [x.min() - 1.0, x.max() + 1.0, np.nextafter(lo, T(-np.inf)), np.nextafter(hi, T(np.inf))],
                            x[0] - 0.125, x[-1] + 0.125]).astype(dt)
        q2 = np.concatenate([q2, [x[0] - 0.25, x[-1] + 0.25, np.nextafter(x[0], T(-np.inf)), np.nextafter(x[-1], T(np.inf))]]).astype(dt)
    got, got2 = it.interp_array(q), it.interp_lanewise(q2)
    mode = oracle.EXTRAPOLATE_YES if extrapolate else oracle.EXTRAPOLATE_NO
    left, right = ORACLE_ENDS[name]
    what = f"{name} n={n} {np.dtype(dt).name} extrapolate={extrapolate}"
    for l in range(L):
        xc, yc = np.ascontiguousarray(x[:, l]), np.ascontiguousarray(y[:, l])
        st, oa, ob = oracle.cubic_build(xc, yc, left=left, right=right)
        assert st == oracle.OK
        assert_bits(a[:, l], oa[:, 0], f"{what}: oracle a lane {l}")
        assert_bits(b[:, l], ob[:, 0], f"{what}: oracle b lane {l}")
        st, _, want = oracle.interp1d_cubic(xc, yc, oa, ob, q, mode)
        assert st == oracle.OK
        assert_bits(got[:, l], want[:, 0], f"{what}: oracle rows lane {l}")
        st, _, want = oracle.interp1d_cubic(xc, yc, oa, ob, q2[:, l], mode)
        assert st == oracle.OK
        assert_bits(got2[:, l], want[:, 0], f"{what}: oracle lane-wise rows lane {l}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("extrapolate", [False, True])
@pytest.mark.parametrize("n", [3, 4, 5, 33])
@pytest.mark.parametrize("name", list(ORACLE_ENDS))
def test_against_the_oracle_per_column_for_every_end_kind(pkg, dt, name, n, extrapolate):
    """test_against_the_oracle_per_column of tests/test_gpu_lane_axes.py has NotAKnot at n = 33.  Here natural, clamped and the
    mixed FirstDeriv / SecondDeriv ends beside it, n = 3 (NotAKnot: the parabola rows), 4, 5 and 33, 3 lanes, in range and
    with extrapolation (queries outside every lane's own range included): tables and both calls against
    oracle.cubic_build / oracle.interp1d_cubic of the column alone."""
    oracle_ends_case(pkg, dt, name, n, extrapolate)


# ---- 3, 4: the record copy beyond one trip, and the handle without a copy --------------------------------------------------------
def device_table(n, dt, seed):
    """(x, y) of shape (n, 4) made on the device.  Every spacing is 0.25 or 0.5, drawn per lane; column l rises from 0.25 l over
    the first half of the rows and falls from E + 0.25 l over the second, E = n / 2 + 8, so the first knots and the last knots
    of the four lanes lie within 0.75 of each other and the common range [Lo, Hi] reaches into the first and the last
    intervals of every lane.  Every knot is a multiple of 0.25 below 2^22 (f32, n = 2^22 + 3) or 2^23 (f64): exact in the
    element type, so the cumulative sums are exact whatever their order."""
    import torch
    dev, L = "cuda:0", 4
    g = torch.Generator(device=dev).manual_seed(seed)
    half = n // 2
    inc = torch.randint(1, 3, (n, L), generator=g, device=dev).to(tdt(dt)) * 0.25
    off = torch.arange(L, device=dev, dtype=tdt(dt)) * 0.25
    x = torch.empty((n, L), dtype=tdt(dt), device=dev)
    head = inc[:half]
    x[:half] = torch.cumsum(head, 0) - head + off
    tail = torch.flip(inc[half:], (0,))
    x[half:] = torch.flip((n / 2 + 8.0) + off - (torch.cumsum(tail, 0) - tail), (0,))
    del inc, head, tail
    assert bool((x[1:] > x[:-1]).all())
    y = torch.randn((n, L), generator=g, device=dev, dtype=tdt(dt))
    return x, y


def end_queries(tx, n, draws=0, seed=0):
    """(q, q2): the row-wise queries -- knots of any lane and their midpoints that lie in the first 64 intervals of EVERY lane
    or in the last 64 of every lane, Lo and Hi among them -- and a query per lane: knots 0 .. 64 and n - 65 .. n - 1 of the
    lane with their midpoints.  `draws` seeded draws over [Lo, Hi] / over each lane's own range are appended."""
    dt = {8: np.float64, 4: np.float32}[tx.element_size()]
    head, tail = tx[:66].cpu().numpy(), tx[n - 66:].cpu().numpy()
    lo, hi = head[0].max(), tail[-1].min()
    assert head[0].min() < lo and tail[-1].max() > hi             # the lanes' ranges differ at both ends
    mid = lambda c: (0.5 * (c[1:].astype(np.float64) + c[:-1])).astype(dt)      # noqa: E731
    pool = np.concatenate([head[:65].ravel(), mid(head[:65]).ravel(), tail[1:].ravel(), mid(tail[1:]).ravel(), [lo, hi]]).astype(dt)
    first = pool[(pool >= lo) & (pool <= head[64].min())]          # inside the first 64 intervals of every lane
    last = pool[(pool >= tail[1].max()) & (pool <= hi)]            # tail[1] is knot n - 65: inside the last 64 of every lane
    assert first.size > 100 and last.size > 100 and lo in first and hi in last
    q = np.unique(np.concatenate([first, last]))
    own = np.concatenate([head[:65], mid(head[:65]), tail[1:], mid(tail[1:])], axis=0)
    rng = np.random.default_rng(seed)
    if draws:
        q = np.concatenate([q, rng.uniform(lo, hi, draws).astype(dt).clip(lo, hi)])
        u = rng.uniform(0.0, 1.0, (draws, tx.shape[1]))
        own = np.concatenate([own, (head[0] + u * (tail[-1] - head[0])).astype(dt).clip(head[0], tail[-1])], axis=0)
    for l in range(own.shape[1]):
        own[:, l] = own[rng.permutation(own.shape[0]), l]
    return q, np.ascontiguousarray(own)


def column_handles(pkg, tx, ty):
    return [pkg.Interp1D.builder(ty[:, l].contiguous()).x(tx[:, l].contiguous()).strategy(pkg.Pchip.new()).build()
            for l in range(tx.shape[1])]


def run_large(pkg, capfd, it, refs, q, q2, records, what):
    import torch
    ref, ref2 = ref_rows(refs, q), ref_lanewise(refs, q2)
    for dev in (False, True):
        with traced(capfd) as t:
            got = it.interp_array(torch.as_tensor(q, device="cuda:0") if dev else q)
            got2 = it.interp_lanewise(torch.as_tensor(q2, device="cuda:0") if dev else q2)
        assert len(t.plans) == 2 and has(t.plans, "lane-axes eval cubic=1 laneq=0", f"records={records}") and \
            has(t.plans, "lane-axes eval cubic=1 laneq=1", f"records={records}"), t.plans
        assert_bits(got.cpu().numpy() if dev else got, ref, f"{what}: interp_array, device queries={dev}")
        assert_bits(got2.cpu().numpy() if dev else got2, ref2, f"{what}: interp_lanewise, device queries={dev}")


def test_the_records_kernel_goes_round_twice(pkg, monkeypatch, capfd):
    """f32 Pchip, 4 lanes, n = 2^22 + 3, tables made on the device: n * lanes = 2^24 + 12 elements, 12 more than the 65 536
    blocks of lane_axes_records_kernel cover in one trip, and a record copy of 256 MiB.  The records of the last rows are
    written on the second trip: the queries of both calls sit in the last 64 intervals of every lane (and in the first 64).
    Yardstick: the four single-column Pchip handles built from the device columns."""
    import torch
    monkeypatch.delenv("NDI_LANE_AXES_RECORDS", raising=False)
    n = (1 << 22) + 3
    assert n * 4 > (1 << 24) and n * 4 - (n - 65) * 4 <= 65 * 4 and n * 4 * 16 < (1 << 30)
    tx, ty = device_table(n, np.float32, 31)
    try:
        it = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(pkg.Pchip.new()).build()
        refs = column_handles(pkg, tx, ty)
        q, q2 = end_queries(tx, n)
        run_large(pkg, capfd, it, refs, q, q2, 1, "the second trip of the records kernel")
    finally:
        it = refs = tx = ty = None
        torch.cuda.empty_cache()


def test_above_the_record_cap(pkg, monkeypatch, capfd):
    """f64 Pchip, 4 lanes, n = 2^23 + 1: the record copy would be n * lanes * 32 bytes = 2^30 + 128, over REC_LIMIT, so the
    handle has none, and with NDI_LANE_AXES_RECORDS unset (the knob's 1) `launch` must still pick the REC = false instance:
    records=0 in the plan line of both calls, of the handle and of a replicate([0]) clone, and the single-column handles'
    bits on the first 64 and last 64 intervals and at 200 seeded draws."""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    assert free > 8 * 2**30, "the test needs 8 GB of free device memory"
    monkeypatch.delenv("NDI_LANE_AXES_RECORDS", raising=False)
    n = (1 << 23) + 1
    assert n * 4 * 4 * 8 == (1 << 30) + 128
    tx, ty = device_table(n, np.float64, 32)
    try:
        it = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(pkg.Pchip.new()).build()
        refs = column_handles(pkg, tx, ty)
        q, q2 = end_queries(tx, n, draws=200, seed=33)
        run_large(pkg, capfd, it, refs, q, q2, 0, "above the record cap")
        clone = it.replicate([0])[0]
        run_large(pkg, capfd, clone, refs, q, q2, 0, "above the record cap, a clone")
    finally:                                           # a failure must not hold 3 GiB for the tests that follow
        it = clone = refs = tx = ty = None
        torch.cuda.empty_cache()


# ---- 5: host arrays in two chunks --------------------------------------------------------------------------------------------------
def linear_restatement(x, y, q):
    """The header's Linear operation order on a two-knot table in the table's element type, one numpy operation per IEEE
    operation (numpy fuses nothing): ((y2 - y1) / (x2 - x1)) * (q - x1) + y1.  q: (rows,) for all lanes or (rows, lanes)."""
    assert x.shape[0] == 2 and x.dtype == y.dtype == q.dtype
    slope = (y[1] - y[0]) / (x[1] - x[0])
    d = (q[:, None] if q.ndim == 1 else q) - x[0][None, :]
    d *= slope[None, :]
    d += y[0][None, :]
    return d


def two_knot_table(L, seed):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(0.0, 0.25, L), rng.uniform(0.75, 1.0, L)]).astype(np.float32)
    y = rng.normal(size=(2, L)).astype(np.float32)
    return x, y


def test_host_arrays_in_two_chunks(pkg):
    """f32 Linear, 2 knots, 2^20 lanes, 65 query rows: 260 MiB of output.  FloatEngine::eval_body and lanewise_run cut host
    arrays into chunks of 256 MiB = 64 rows, so the second chunk holds row 64 alone, and `off` -- added to the reported index,
    to the query pointer and to the output pointer -- is 64.  Yardstick: linear_restatement, which is first shown to equal
    the single-column handles at 5 lanes."""
    import torch
    dt = np.float32
    # the restatement is not the only witness: at a small shape it equals the single-column handles
    xs, ys = two_knot_table(5, 50)
    small, refs = build(pkg, "Linear", xs, ys, ys)
    qs = np.linspace(xs[0].max(), xs[1].min(), 33).astype(dt)
    qs2 = (xs[0] + np.linspace(0.0, 1.0, 33)[:, None] * (xs[1] - xs[0])).astype(dt).clip(xs[0], xs[1])
    assert_bits(linear_restatement(xs, ys, qs), ref_rows(refs, qs), "the restatement, row-wise")
    assert_bits(linear_restatement(xs, ys, qs2), ref_lanewise(refs, qs2), "the restatement, lane-wise")
    assert_bits(small.interp_array(qs), ref_rows(refs, qs), "the small handle")
    L, rows = 1 << 20, 65
    assert (256 << 20) // (L * 4) == 64
    x, y = two_knot_table(L, 51)
    it = pkg.Interp1D.builder(y).lane_axes(x).build()
    lo, hi = x[0].max(), x[1].min()
    q = np.linspace(lo, hi, rows).astype(dt).clip(lo, hi)
    q2 = (x[0] + np.linspace(0.0, 1.0, rows)[:, None] * (x[1] - x[0])).astype(dt).clip(x[0], x[1])
    ref, ref2 = linear_restatement(x, y, q), linear_restatement(x, y, q2)
    buf = np.empty((rows, L), dt)
    bad_q = q.copy()
    bad_q[64] = np.nextafter(hi, dt(np.inf))
    bad_q2 = q2.copy()
    bad_q2[64, L - 3] = np.nextafter(x[1, L - 3], dt(np.inf))
    for where, dev in (("host", lambda v: v), ("device", lambda v: torch.as_tensor(v, device="cuda:0"))):
        # the row-wise call: right as a whole, then a failing query in the second chunk
        buf[:] = SENTINEL
        it.interp_array_into(dev(q), buf)
        assert_bits(buf, ref, f"{where} queries to host output, two chunks")
        buf[:] = SENTINEL
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array_into(dev(bad_q), buf)
        assert e.value.index == 64 and e.value.value == float(bad_q[64]), (where, e.value.index, e.value.value)
        assert_bits(buf[:64], ref[:64], f"{where} queries: the rows of chunk 0 before the failing query")
        assert np.all(buf[64] == dt(SENTINEL)), f"{where} queries: row 64 keeps the sentinel"
        # the lane-wise call
        buf[:] = SENTINEL
        it.interp_lanewise_into(dev(q2), buf)
        assert_bits(buf, ref2, f"{where} lane-wise queries to host output, two chunks")
        buf[:] = SENTINEL
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_lanewise_into(dev(bad_q2), buf)
        assert e.value.index == 64 * L + L - 3 and e.value.value == float(bad_q2[64, L - 3]), (where, e.value.index, e.value.value)
        assert_bits(buf[:64], ref2[:64], f"{where} lane-wise queries: the rows of chunk 0")
        assert np.all(buf[64] == dt(SENTINEL)), f"{where} lane-wise queries: row 64 is untouched"
    torch.cuda.empty_cache()


# ---- 6: row strides, empty batches, async, threads ------------------------------------------------------------------------------------
def ptr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def raw(pkg, it, lanewise, q, nq, q_stride, out, out_stride):
    """ndi_interp1d_eval / ndi_interp1d_eval_lanewise on host arrays or device tensors: (status, info); *info starts from a
    stale record, so a call that returns NDI_OK must have reset it"""
    c = pkg._capi
    opts, info = c.EvalOpts(), c.OobInfo()
    opts.q_memspace = c.MEM_DEVICE if hasattr(q, "data_ptr") else c.MEM_HOST
    opts.out_memspace = c.MEM_DEVICE if hasattr(out, "data_ptr") else c.MEM_HOST
    info.index, info.value, info.axis, info.status = 99, 9.0, 1, c.OUT_OF_BOUNDS
    h = it.strategy._h
    if lanewise:
        st = c.lib().ndi_interp1d_eval_lanewise(h, ptr(q), nq, q_stride, ptr(out), out_stride, C.byref(opts), C.byref(info))
    else:
        st = c.lib().ndi_interp1d_eval(h, ptr(q), nq, ptr(out), out_stride, C.byref(opts), C.byref(info))
    return st, info


def small_case(pkg, dt, name="CubicSpline"):
    n, L = 5, 3
    x, y, k = table(n, L, dt)
    it, refs = build(pkg, name, x, y, k)
    q, lo, hi = common_queries(x, 40)
    return x, it, refs, q, hi, ref_rows(refs, q)


def padded_stride_case(pkg, dt):
    import torch
    c = pkg._capi
    L = 3
    x, it, refs, q, hi, good = small_case(pkg, dt)
    stride = L + 5
    bad = q.copy()
    bad[23] = np.nextafter(hi, dt(np.inf))
    bad[31] = dt(np.nan)
    for where, mk, host in (("host", lambda: np.full((40, stride), SENTINEL, dt), lambda a: a),
                            ("device", lambda: torch.full((40, stride), SENTINEL, dtype=tdt(dt), device="cuda:0"), lambda a: a.cpu().numpy())):
        out = mk()
        qq = q if where == "host" else torch.as_tensor(q, device="cuda:0")
        st, info = raw(pkg, it, False, qq, 40, 0, out, stride)
        assert st == c.OK and (info.index, info.status) == (0, c.OK), (where, st, c.last_error())
        got = host(out)
        assert_bits(got[:, :L], good, f"padded out_row_stride, {where} output")
        assert np.all(got[:, L:] == dt(SENTINEL)), f"{where}: the padding keeps its sentinel"
        out = mk()
        qq = bad if where == "host" else torch.as_tensor(bad, device="cuda:0")
        st, info = raw(pkg, it, False, qq, 40, 0, out, stride)
        assert (st, info.index, info.status) == (c.OUT_OF_BOUNDS, 23, c.OUT_OF_BOUNDS) and info.value == float(bad[23]), (where, st, info.index)
        got = host(out)
        assert_bits(got[:23, :L], good[:23], f"{where}: the rows before the failing query")
        assert np.all(got[23:] == dt(SENTINEL)) and np.all(got[:, L:] == dt(SENTINEL)), f"{where}: rows at / after it, and the padding"


@pytest.mark.parametrize("dt", DTYPES)
def test_padded_out_row_stride_on_the_row_wise_call(pkg, dt):
    """ndi_interp1d_eval with out_row_stride = lanes + 5: into device memory it is the kernel's out_stride, into host memory
    the pitch of hipMemcpy2D.  The padding keeps its sentinel; a failing query leaves the rows at and after it untouched."""
    padded_stride_case(pkg, dt)


def refused_strides_and_empty_batches(pkg, dt):
    import torch
    c = pkg._capi
    L = 3
    x, it, refs, q, hi, good = small_case(pkg, dt)
    q2 = own_queries(x)
    for dev in (False, True):
        mk = (lambda a: torch.as_tensor(a, device="cuda:0")) if dev else (lambda a: a.copy())
        host = (lambda a: a.cpu().numpy()) if dev else (lambda a: a)
        out = mk(np.full((q2.shape[0], L), SENTINEL, dt))
        for lanewise, qq, nq, qs, os_, text in ((False, q, q.size, 0, L - 1, "out_row_stride"), (True, q2, q2.shape[0], L, L - 1, "out_row_stride"),
                                                (True, q2, q2.shape[0], L - 1, L, "q_row_stride")):
            st, info = raw(pkg, it, lanewise, mk(qq), nq, qs, out, os_)
            assert st == c.BAD_ARG and text in c.last_error() and "< lanes" in c.last_error(), (dev, lanewise, st, c.last_error())
            assert np.all(host(out) == dt(SENTINEL))
        for lanewise, qq in ((False, q), (True, q2)):        # nq == 0: NDI_OK, nothing touched, *info reset
            st, info = raw(pkg, it, lanewise, mk(qq), 0, L, out, L)
            assert st == c.OK and (info.index, info.value, info.axis, info.status) == (0, 0.0, 0, c.OK), (dev, lanewise, st, info.index)
            assert np.all(host(out) == dt(SENTINEL))
        st, info = raw(pkg, it, False, mk(q), 0, 0, out, L - 1)   # (the stride is refused before the batch is found empty)
        assert st == c.BAD_ARG
    assert_bits(it.interp_array(q), good, "after the refusals")


@pytest.mark.parametrize("dt", DTYPES)
def test_strides_below_lanes_and_empty_batches(pkg, dt):
    refused_strides_and_empty_batches(pkg, dt)


def async_case(pkg, dt):
    import torch
    L = 3
    x, it, refs, q, hi, good = small_case(pkg, dt)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        qd = torch.as_tensor(q, device="cuda:0")
        out = torch.full((40, L), SENTINEL, dtype=tdt(dt), device="cuda:0")
        it.interp_array_into(qd, out, async_launch=True)
        it.strategy.finish()
        assert_bits(out.cpu().numpy(), good, "async_launch, then finish")
        bad = q.copy()
        bad[29] = dt(np.nan)
        bad[17] = np.nextafter(hi, dt(np.inf))
        bd = torch.as_tensor(bad, device="cuda:0")
        out = torch.full((40, L), SENTINEL, dtype=tdt(dt), device="cuda:0")
        it.interp_array_into(bd, out, async_launch=True)          # the launch itself reports nothing
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.strategy.finish()
        assert e.value.index == 17 and e.value.value == float(bad[17])
        got = out.cpu().numpy()
        assert_bits(got[:17], good[:17], "async: the rows before the lowest failing query")
        assert np.all(got[17:] == dt(SENTINEL)), "async: the rows at and after it are untouched"
        it.strategy.finish()                                        # nothing pending any more
        assert_bits(it.interp_array(qd).cpu().numpy(), good, "after the failed async batch")
    torch.cuda.synchronize()
    assert_bits(it.interp_array(q), good, "after the failed async batch, host arrays")


@pytest.mark.parametrize("dt", DTYPES)
def test_async_launch_and_finish_on_the_row_wise_call(pkg, dt):
    """async_launch is allowed on ndi_interp1d_eval of a lane-axes handle (device output): on a non-default stream, once clean
    and once with two bad queries -- ndi_interp1d_finish reports the lowest index, the rows before it are right, the rows at
    and after it untouched -- and the handle evaluates correctly afterwards."""
    async_case(pkg, dt)


def threads_case(pkg, dt, calls=50):
    import torch
    x, it, refs, q, hi, good = small_case(pkg, dt)
    sets = pkg._capi.lib().ndi_interp1d_scratch_sets
    fresh = build(pkg, "CubicSpline", *table(5, 3, dt))[0]      # a handle that has never evaluated (kept alive for the call)
    idle = sets(fresh.strategy._h)
    q2 = np.tile(own_queries(x), (5, 1))
    qd, q2d = torch.as_tensor(q, device="cuda:0"), torch.as_tensor(q2, device="cuda:0")
    one, one2 = it.interp_array(qd).cpu().numpy(), it.interp_lanewise(q2d).cpu().numpy()
    assert_bits(one, good, "single-threaded rows")
    assert_bits(one2, ref_lanewise(refs, q2), "single-threaded lane-wise rows")
    N = 8
    errors, wrong = [], []
    gate = threading.Barrier(N)

    def work(i):
        try:
            gate.wait(timeout=60)
            for k in range(calls):
                a, b = it.interp_array(qd), it.interp_lanewise(q2d)
                if not (np.array_equal(a.cpu().numpy().view(np.uint8), one.view(np.uint8)) and
                        np.array_equal(b.cpu().numpy().view(np.uint8), one2.view(np.uint8))):
                    wrong.append((i, k))
        except Exception as e:       # noqa: BLE001
            errors.append((i, repr(e)))
    threads = [threading.Thread(target=work, args=(i,)) for i in range(N)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not errors and not wrong and not any(th.is_alive() for th in threads), (errors, wrong[:5])
    it.strategy.trim()
    assert sets(it.strategy._h) == idle
    assert_bits(it.interp_array(qd).cpu().numpy(), one, "after trim")


@pytest.mark.parametrize("dt", DTYPES)
def test_eight_threads_on_one_handle(pkg, dt):
    """Eight threads, released together, call interp_array and interp_lanewise on one CubicSpline handle with device arrays,
    50 calls each: every result has the single-threaded bits; after trim() the handle holds the scratch sets of an idle one."""
    threads_case(pkg, dt)
