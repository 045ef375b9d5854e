"""GPU: the seven lazily built accelerating tables when their build fails (NDI_TEST_FAIL_LAZY_ALLOC=1 throws the
out-of-memory failure of a hipMalloc on the host, before the allocation; no device fault is involved):

  DevicePyramid::ensure_bucket_index      the u16 bucket index staged in LDS behind the knot pyramid
  DevicePyramid::ensure_bucket_index32    the u32 bucket index of an axis that stays in global memory
  DevicePyramid::ensure_dense_lut         the dense index of the query-per-lane kernels (1-D and 2-D)
  Interp1DImpl::ensure_packed             the interval-packed copy of the tables of the query-order kernel
  Interp2DImpl::ensure_slopes             the slope-record copy of a 2-D grid
  Interp1DImpl::lanewise_records          the element-record copy of the lane-wise kernel
  Interp2DImpl::lanewise_records          the node-record copy of the 2-D lane-wise kernel (a Bicubic handle and its partials)

Every scenario has a CONTROL handle (same arrays, no injection) whose plan line (NDI_TRACE_PLAN) must show the table in
use -- a control that does not use it FAILS the scenario -- and then, on a fresh handle,
  (a) the first evaluation under the injection returns OK, its plan line shows the fallback, its rows are the control's
      rows and the yardstick's, bit for bit;
  (b) with the variable unset the same handle still takes the fallback (nothing retries) and gives the same bits;
  (c) after trim() the bits are the same again; a rebuild is asserted only for the two lane-wise record copies, whose
      LanewiseRecords::drop returns them to "not tried" (tests/test_gpu_lanewise.py:
      test_trim_rebuilds_the_record_copy_and_a_clone_builds_its_own; the 2-D handle's trim drops the same structure); the
      other five were observed to stay unavailable
      (DESIGN.md 4.19a), which no comment promises, so either plan is accepted for them;
  (d) a clone(0) of the failed handle, made with the variable unset, builds its own table.
The yardstick of every scenario is the one of the test file that owns the kernel: per_lane of tests/test_gpu_lanewise.py
(and of tests/test_gpu_lanewise2d.py) for the lane-wise calls, the CPU oracle (as tests/test_gpu_short_rows.py, test_gpu_lanes.py, test_gpu_slopes2d.py take
it) for the row-wise ones.  Every comparison is hostile_inputs.check_bits."""
import os

import numpy as np
import pytest

import hostile_inputs
import inverse_cases as ic
import oracle
from test_gpu_lanewise import data_for, forward, lane_queries, per_lane, set_variant
from test_gpu_parity import knots

pytestmark = pytest.mark.gpu

INJECT = "NDI_TEST_FAIL_LAZY_ALLOC"
DTYPES = [np.float64, np.float32]


class traced:
    """the plan lines of the calls inside the block; inject: NDI_TEST_FAIL_LAZY_ALLOC=1 for those calls only"""

    def __init__(self, capfd, inject=False):
        self.capfd, self.inject = capfd, inject

    def __enter__(self):
        assert INJECT not in os.environ
        os.environ["NDI_TRACE_PLAN"] = "1"
        if self.inject:
            os.environ[INJECT] = "1"
        self.capfd.readouterr()
        return self

    def __exit__(self, *a):
        os.environ.pop("NDI_TRACE_PLAN", None)
        os.environ.pop(INJECT, None)
        self.plans = [ln for ln in self.capfd.readouterr().err.splitlines() if ln.startswith("[ndi plan]")]


def scenario(capfd, what, make, evaluate, ref, uses, fallback, rebuilt_by_trim=False):
    """make(): a fresh handle; evaluate(handle): its rows as a numpy array; uses(plans) / fallback(plans): the plan lines
    of one evaluation show the table in use / the fallback"""
    control = make()
    with traced(capfd) as t:
        rows = evaluate(control)
    assert uses(t.plans), f"{what}: the control does not use the table: {t.plans}"
    hostile_inputs.check_bits(rows, ref, what + ": control against the yardstick")
    it = make()
    with traced(capfd, inject=True) as t:                          # (a)
        got = evaluate(it)
    assert fallback(t.plans) and not uses(t.plans), f"{what}: injected: {t.plans}"
    hostile_inputs.check_bits(got, ref, what + ": injected against the yardstick")
    hostile_inputs.check_bits(got, rows, what + ": injected against the control")
    with traced(capfd) as t:                                       # (b)
        got = evaluate(it)
    assert fallback(t.plans) and not uses(t.plans), f"{what}: second call, nothing retries: {t.plans}"
    hostile_inputs.check_bits(got, rows, what + ": second call")
    it.strategy.trim()                                             # (c)
    with traced(capfd) as t:
        got = evaluate(it)
    hostile_inputs.check_bits(got, rows, what + ": after trim")
    assert uses(t.plans) or fallback(t.plans), f"{what}: after trim: {t.plans}"
    if rebuilt_by_trim:
        assert uses(t.plans), f"{what}: trim returns the table to 'not tried': {t.plans}"
    rep = it.replicate([0])[0]                                     # (d)
    with traced(capfd) as t:
        got = evaluate(rep)
    assert uses(t.plans), f"{what}: the clone builds its own table: {t.plans}"
    hostile_inputs.check_bits(got, rows, what + ": clone")
    with traced(capfd) as t:                                       # ... and the source stays as it was
        got = evaluate(it)
    hostile_inputs.check_bits(got, rows, what + ": the source after its clone")


def has(plans, *frags):
    return any(all(f in ln for f in frags) for ln in plans)


def _tdt(dt):
    import torch
    return torch.float64 if dt == np.float64 else torch.float32


def lanewise_rows(xs):
    import torch
    qd = torch.as_tensor(xs, device="cuda:0")
    return lambda it: it.interp_lanewise(qd).cpu().numpy()


def rowwise_rows(pkg, q, L, dt, path=None):
    """interp_array_into on device buffers, as tests/test_gpu_short_rows.py's _device_eval"""
    import torch
    qd = torch.as_tensor(q, device="cuda:0")

    def run(it):
        if path is not None:
            it.strategy.path = path
        out = torch.full((q.size, L), -9.0, dtype=_tdt(dt), device="cuda:0")
        it.interp_array_into(qd, out)
        return out.cpu().numpy()
    return run


def oracle_rows(it, source, x, y, q):
    """the CPU oracle on the handle's own tables (tests/test_gpu_hermite.py takes a Pchip's rows the same way)"""
    if source == "linear":
        return oracle.interp1d_linear(x, y, q)[2].reshape(q.size, y.shape[1])
    a, b = it.strategy.coefficients()
    return oracle.interp1d_cubic(x, y, a, b, q)[2].reshape(q.size, y.shape[1])


# ---- Interp1DImpl::lanewise_records ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["pchip", "linear"])
def test_lanewise_records(pkg, monkeypatch, capfd, source):
    """65 x 9 f64, Q = 257, the fused kernel from the record copy (NDI_LANEWISE_RECORDS=1, NDI_LANEWISE_MODE=2): no batch
    threshold guards the copy (lanewise_host.hpp, want_records).  Injected: records=0 and no `lanewise records built`"""
    rng = np.random.default_rng(9)
    n, L, Q = 65, 9, 257
    x = ic.knots(rng, n, np.float64)
    y = data_for(source, rng, n, L, np.float64)
    xs = lane_queries(rng, x, Q, L)
    ref = per_lane(forward(pkg, source, x, y), xs)
    set_variant(monkeypatch, 1, 2)
    scenario(capfd, f"lane-wise records, {source}", lambda: forward(pkg, source, x, y), lanewise_rows(xs), ref,
             uses=lambda p: has(p, "lanewise form=fused", "records=1") and has(p, "lanewise records built"),
             fallback=lambda p: has(p, "lanewise form=fused", "records=0") and not has(p, "lanewise records built"),
             rebuilt_by_trim=True)


# ---- Interp2DImpl::lanewise_records ---------------------------------------------------------------------------------------
def test_lanewise2d_records(pkg, monkeypatch, capfd):
    """9 x 7 x 5 Pchip f64, Q = 67, NDI_LANEWISE2D_RECORDS=1.  Injected: records=0 and no `lanewise2d records built`.  The copy
    is LanewiseRecords, the structure of the 1-D copy, and Interp2DImpl::trim drops it: trim returns it to "not tried".  A
    partial handle made from the failed source shares lw_records, so it takes the fallback too and nothing retries."""
    import torch
    import test_gpu_lanewise2d as l2
    rng = np.random.default_rng(15)
    nx, ny, L, Q = 9, 7, 5, 67
    x, y = ic.knots(rng, nx, np.float64), ic.knots(rng, ny, np.float64)
    z = l2.grid_data(rng, nx, ny, L, np.float64)
    xs, ys = l2.queries(rng, x, y, Q, L)
    make = lambda: l2.surface(pkg, "pchip", x, y, z)      # noqa: E731
    ref = l2.per_lane(make(), xs, ys)
    dx, dy = torch.as_tensor(xs, device="cuda:0"), torch.as_tensor(ys, device="cuda:0")
    evaluate = lambda it: it.interp_lanewise(dx, dy).cpu().numpy()      # noqa: E731
    uses = lambda p: has(p, "lanewise2d kind=bicubic", "records=1") and has(p, "lanewise2d records built")      # noqa: E731
    fallback = lambda p: has(p, "lanewise2d kind=bicubic", "records=0") and not has(p, "lanewise2d records built")      # noqa: E731
    monkeypatch.setenv("NDI_LANEWISE2D_RECORDS", "1")
    scenario(capfd, "2-D lane-wise records", make, evaluate, ref, uses=uses, fallback=fallback, rebuilt_by_trim=True)
    # a partial handle of the failed source
    it = make()
    with traced(capfd, inject=True) as t:
        got = evaluate(it)
    assert fallback(t.plans) and not uses(t.plans), t.plans
    hostile_inputs.check_bits(got, ref, "the source of the partial, injected")
    d = it.partial(1, 0)
    ref_d = l2.per_lane(d, xs, ys)
    for h, want, what in ((d, ref_d, "a partial of the failed source"), (it, ref, "the failed source after its partial"),
                          (d, ref_d, "the partial, second call")):
        with traced(capfd) as t:
            got = evaluate(h)
        assert fallback(t.plans) and not uses(t.plans), f"{what}: nothing retries: {t.plans}"
        hostile_inputs.check_bits(got, want, what)


# ---- Interp1DImpl::ensure_packed ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["linear", "pchip"])
def test_packed_intervals(pkg, monkeypatch, capfd, source):
    """the fused_pack variant of tests/test_gpu_short_rows.py on f32 rows of 3 lanes.  Q = 1025: four workgroups of the
    query-order kernel and below the 4096 queries at which plan_fused asks for the bucket index as well
    (interp1d_host.hpp, plan_fused1: `if (P.nq >= 4096) h.pyr.ensure_bucket_index()`), so the injection meets
    ensure_packed alone"""
    for k, v in (("NDI_SHORT_MODE", 2), ("NDI_FUSED_LDS", 0), ("NDI_FUSED_PACK", 1)):
        monkeypatch.setenv(k, str(v))
    rng = np.random.default_rng(10)
    n, L, Q = 300, 3, 1025
    x = knots("rand", n, rng, np.float32)
    y = rng.uniform(-1.0, 1.0, (n, L)).astype(np.float32)
    q = rng.uniform(x[0], x[-1], Q).astype(np.float32)
    q[:4] = [x[0], x[-1], x[n // 2], np.nextafter(x[-1], x[0])]
    make = lambda: forward(pkg, source, x, y)      # noqa: E731
    scenario(capfd, f"packed intervals, {source}", make, rowwise_rows(pkg, q, L, np.float32, pkg.PATH_GATHER),
             oracle_rows(make(), source, x, y, q),
             uses=lambda p: has(p, "[ndi plan] fused tables=memory", "pack=1"),
             fallback=lambda p: has(p, "[ndi plan] fused tables=memory", "pack=0"))


# ---- DevicePyramid::ensure_bucket_index -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("source", ["linear", "pchip"])
def test_staged_bucket_index_row_wise(pkg, monkeypatch, capfd, dt, source):
    """257 clustered knots, 3 lanes, Q = 4097: the first odd batch at / above the 4096 queries from which plan_fused builds
    the index (interp1d_host.hpp, plan_fused1: `P.nq >= 4096`); the tables stay in memory and unpacked (NDI_FUSED_LDS=0,
    NDI_FUSED_PACK=0), so the index is the only lazy table in the plan.  The `lut=` field of the `fused` line"""
    for k, v in (("NDI_SHORT_MODE", 2), ("NDI_FUSED_LDS", 0), ("NDI_FUSED_PACK", 0)):
        monkeypatch.setenv(k, str(v))
    rng = np.random.default_rng(11)
    n, L, Q = 257, 3, 4097
    x = ic.knots(rng, n, dt)
    y = rng.uniform(-1.0, 1.0, (n, L)).astype(dt)
    q = rng.uniform(x[0], x[-1], Q).astype(dt)
    q[:4] = [x[0], x[-1], x[n // 2], np.nextafter(x[-1], x[0])]
    q[4:4 + n] = x
    make = lambda: forward(pkg, source, x, y)      # noqa: E731
    scenario(capfd, f"staged bucket index, row-wise, {source} {np.dtype(dt).name}", make,
             rowwise_rows(pkg, q, L, dt, pkg.PATH_GATHER), oracle_rows(make(), source, x, y, q),
             uses=lambda p: has(p, "[ndi plan] fused tables=memory", "lut=1"),
             fallback=lambda p: has(p, "[ndi plan] fused tables=memory", "lut=0"))


def test_staged_bucket_index_lane_wise(pkg, monkeypatch, capfd):
    """the shape of test_gpu_lanewise.py's test_the_staged_bucket_index: 257 clustered f32 knots x 64 lanes, Q = 4097, so
    4097 x 64 elements are above the 4096 ELEMENTS of lanewise_host.hpp (lanewise_enqueue: `if (total >= 4096)`)"""
    n, L, Q = 257, 64, 4097
    rng = np.random.default_rng([n, L, Q])
    x = ic.knots(rng, n, np.float32)
    y = data_for("pchip", rng, n, L, np.float32)
    xs = lane_queries(rng, x, Q, L)
    ref = per_lane(forward(pkg, "pchip", x, y), xs)
    set_variant(monkeypatch, 0, 2)
    scenario(capfd, "staged bucket index, lane-wise", lambda: forward(pkg, "pchip", x, y), lanewise_rows(xs), ref,
             uses=lambda p: has(p, "lanewise form=fused", "stage=1", "lut=1"),
             fallback=lambda p: has(p, "lanewise form=fused", "stage=1", "lut=0"))


# ---- DevicePyramid::ensure_bucket_index32 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["linear", "pchip"])
def test_global_bucket_index_lane_wise(pkg, monkeypatch, capfd, source):
    """40001 clustered f64 knots (320 KB: not staged), 3 lanes, Q = 1400: 4200 elements, above the 4096 of lanewise_enqueue.
    Injected, the fused kernel searches the pyramid from global memory (stage=0 lut=0)"""
    rng = np.random.default_rng(12)
    n, L, Q = 40001, 3, 1400
    x = ic.knots(rng, n, np.float64)
    y = data_for(source, rng, n, L, np.float64)
    xs = lane_queries(rng, x, Q, L)
    ref = per_lane(forward(pkg, source, x, y), xs)
    set_variant(monkeypatch, 0, 2)
    scenario(capfd, f"global bucket index, lane-wise, {source}", lambda: forward(pkg, source, x, y), lanewise_rows(xs), ref,
             uses=lambda p: has(p, "lanewise form=fused", "stage=0", "lut=2"),
             fallback=lambda p: has(p, "lanewise form=fused", "stage=0", "lut=0"))


@pytest.mark.parametrize("source", ["linear", "pchip"])
def test_global_bucket_index_row_wise(pkg, monkeypatch, capfd, source):
    """the same axis under the query-order kernel with the knots in global memory (TLDS == 3), which a batch takes from 4096
    queries on (plan_fused: `P.nq < 4096` keeps the two-kernel form): 5000 queries.  Its plan line does not show the
    index, so `uses` and `fallback` are the same line here; what the scenario checks is the bits of the kernel's pyramid
    search from global memory.  NDI_FUSED_PACK=0: the packed copy is another test's"""
    monkeypatch.setenv("NDI_FUSED_PACK", "0")
    rng = np.random.default_rng(13)
    n, L, Q = 40001, 3, 5000
    x = ic.knots(rng, n, np.float64)
    y = rng.uniform(-1.0, 1.0, (n, L))
    q = rng.uniform(x[0], x[-1], Q)
    q[:4] = [x[0], x[-1], x[n // 2], np.nextafter(x[-1], x[0])]
    q[4:2004] = x[::20][:2000]
    make = lambda: forward(pkg, source, x, y)      # noqa: E731
    line = lambda p: has(p, "[ndi plan] fused tables=memory,knots=global")      # noqa: E731
    control = make()
    run = rowwise_rows(pkg, q, L, np.float64)
    ref = oracle_rows(control, source, x, y, q)
    with traced(capfd) as t:
        rows = run(control)
    assert line(t.plans), t.plans
    hostile_inputs.check_bits(rows, ref, "control")
    it = make()
    for step, inject in (("injected", True), ("second call", False)):
        with traced(capfd, inject=inject) as t:
            got = run(it)
        assert line(t.plans), (step, t.plans)
        hostile_inputs.check_bits(got, ref, f"global bucket index, row-wise, {source}: {step}")
    it.strategy.trim()
    hostile_inputs.check_bits(run(it), ref, "after trim")
    hostile_inputs.check_bits(run(it.replicate([0])[0]), ref, "clone")
    # the lane-wise plan line of the same handles does show the index: the failed handle has none, its control has one
    set_variant(monkeypatch, 0, 2)
    xs = lane_queries(rng, x, 1400, L)
    with traced(capfd) as t:
        a = lanewise_rows(xs)(it)
    assert has(t.plans, "stage=0", "lut=0"), t.plans
    with traced(capfd) as t:
        b = lanewise_rows(xs)(control)
    assert has(t.plans, "stage=0", "lut=2"), t.plans
    hostile_inputs.check_bits(a, b, "the failed handle against its control, lane-wise")


# ---- DevicePyramid::ensure_dense_lut --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("source", ["linear", "spline"])
def test_dense_index_1d(pkg, monkeypatch, capfd, dt, L, source):
    """NDI_LANES_KERNEL=1 on the ("rand", 100, 1) and ("rand", 100, 5) shapes of tests/test_gpu_lanes.py, Q = 70 003 (forced,
    plan_lanes has no batch threshold).  Injected, plan_lanes returns false (`if (!pyr.dense_ok) return false`): no `lanes`
    line, another kernel serves the batch"""
    monkeypatch.setenv("NDI_LANES_KERNEL", "1")
    rng = np.random.default_rng(100 * 31 + L)
    n, Q = 100, 70_003
    x = knots("rand", n, rng, dt)
    y = rng.uniform(-1.0, 1.0, (n, L)).astype(dt)
    q = rng.uniform(x[0], x[-1], Q).astype(dt)
    q[:4] = [x[0], x[-1], x[n // 2], np.nextafter(x[-1], x[0])]
    q[4:4 + n] = x
    if source == "linear":
        make = lambda: pkg.Interp1D.builder(y).x(x).build()      # noqa: E731
        ref = oracle.interp1d_linear(x, y, q)[2].reshape(Q, L)
    else:
        make = lambda: pkg.Interp1D.builder(y).x(x).strategy(pkg.CubicSpline.new()).build()      # noqa: E731
        st, a, b = oracle.cubic_build(x, y)
        assert st == oracle.OK
        ref = oracle.interp1d_cubic(x, y, a, b, q)[2].reshape(Q, L)
    scenario(capfd, f"dense index, {source} x {L} {np.dtype(dt).name}", make, rowwise_rows(pkg, q, L, dt), ref,
             uses=lambda p: has(p, "[ndi plan] lanes L=", "index=dense"),
             fallback=lambda p: not has(p, "[ndi plan] lanes L="))


def grid_case(kx, ky, nx, ny, C, dt):
    rng = np.random.default_rng(nx * 13 + ny * 7 + C)
    Q = 70_003
    x, y = knots(kx, nx, rng, dt), knots(ky, ny, rng, dt)
    g = rng.uniform(-1, 1, (nx, ny, C)).astype(dt)
    qx = rng.uniform(x[0], x[-1], Q).astype(dt)
    qy = rng.uniform(y[0], y[-1], Q).astype(dt)
    k = min(nx, ny)
    qx[:k] = x[:k]; qy[:k] = y[:k]
    qx[k:k + 3] = [x[-1], x[0], x[-1]]; qy[k:k + 3] = [y[-1], y[-1], y[0]]
    return x, y, g, qx, qy, oracle.interp2d_bilinear(x, y, g, qx, qy)[3].reshape(Q, C)


def grid_rows(qx, qy, C, dt):
    import torch
    qxd, qyd = torch.as_tensor(qx, device="cuda:0"), torch.as_tensor(qy, device="cuda:0")

    def run(it):
        out = torch.full((qx.size, C), -9.0, dtype=_tdt(dt), device="cuda:0")
        it.interp_array_into(qxd, qyd, out)
        return out.cpu().numpy()
    return run


@pytest.mark.parametrize("dt", DTYPES)
def test_dense_index_2d(pkg, monkeypatch, capfd, dt):
    """NDI_LANES2D_KERNEL=1 on the ("rand", "rand", 40, 57, 5) shape of tests/test_gpu_lanes.py: both axes' dense indices
    fail, no `lanes2d` line"""
    monkeypatch.setenv("NDI_LANES2D_KERNEL", "1")
    x, y, g, qx, qy, ref = grid_case("rand", "rand", 40, 57, 5, dt)
    make = lambda: pkg.Interp2D.builder(g).x(x).y(y).build()      # noqa: E731
    scenario(capfd, f"dense index, 2-D {np.dtype(dt).name}", make, grid_rows(qx, qy, 5, dt), ref,
             uses=lambda p: has(p, "[ndi plan] lanes2d L=") and not has(p, "[ndi plan] lanes2d L=", "maxk=0,0"),
             fallback=lambda p: not has(p, "[ndi plan] lanes2d L="))


# ---- Interp2DImpl::ensure_slopes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kx,ky,nx,ny,C", [("lin", "lin", 64, 64, 8), ("rand", "rand", 100, 100, 5)])
def test_slope_records(pkg, monkeypatch, capfd, dt, kx, ky, nx, ny, C):
    """NDI_SLOPES2D_KERNEL=1 (NDI_LANES2D_KERNEL=0) on two shapes of tests/test_gpu_slopes2d.py.  On the evenly spaced axes
    the dense index is the exact O(1) guess and allocates nothing, so the injection meets ensure_slopes alone (its state
    becomes 2, which trim leaves); on the uneven axes the dense indices fail first and ensure_slopes is never reached.
    Either way: no `slopes2d` line, the same rows"""
    monkeypatch.setenv("NDI_SLOPES2D_KERNEL", "1")
    monkeypatch.setenv("NDI_LANES2D_KERNEL", "0")
    if dt == np.float32 and C == 8:
        C = 12
    x, y, g, qx, qy, ref = grid_case(kx, ky, nx, ny, C, dt)
    make = lambda: pkg.Interp2D.builder(g).x(x).y(y).build()      # noqa: E731
    scenario(capfd, f"slope records, {nx} x {ny} x {C} {np.dtype(dt).name}", make, grid_rows(qx, qy, C, dt), ref,
             uses=lambda p: has(p, "[ndi plan] slopes2d L="),
             fallback=lambda p: not has(p, "[ndi plan] slopes2d L="))
