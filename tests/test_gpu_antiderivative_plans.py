"""GPU: every launch plan of the antiderivative build (csrc/antiderivative_host.hpp, AntiderivImpl::launch_build) and of its
evaluation (enqueue, run) that tests/test_gpu_antiderivative.py does not reach, each at the smallest shape that reaches it,
BIT FOR BIT (zero signs included) against the numpy restatement (tests/antiderivative_ref.py) applied to the source handle's
own tables, AND against the plan line the library prints under NDI_TRACE_PLAN, so a case that drifts to another branch
fails instead of passing vacuously.  Knots are uneven (cumsum of uniform(0.5, 2.0)), data normal; sources Linear and Pchip
(the kernels' two template variants), f32 and f64, unless a case says otherwise.  No tolerance appears anywhere.

Build (nblk = ceil(n / 256) blocks; every case: the whole table through data_table(), and about 200 rows at knots, their
neighbours and random points, the last two blocks included):

  two chains, odd tile count   4095*256 x 1.  kb starts at 32 / lanes and is halved while ceil(nblk / kb) < 2048, so kb = 2
                               needs nblk >= 4095: 2048 tiles, the last of ONE block (k < nblk guard), and since n is a
                               multiple of 256 the last block has 255 intervals (p[nint * L] = S inside a sub-tile).
  last block of one knot       4096*256 + 1 x 1: nblk = 4097, 2049 tiles, the last block has no interval at all.
  two chains of 16 lanes       4095*256 + 7 x 16: kb = 32 / 16 = 2 survives at 4096 blocks; 32 of 256 threads run chains,
                               kk = tid / 16.
  five chains of 3 lanes       10236*256 + 100 x 3: kb = 10 -> 5 stays where ceil(nblk / 5) >= 2048, nblk >= 10236; a kb that
                               is no power of two, kk = tid / 3.
  32 chains                    65505*256 + 2 x 1: ceil(nblk / 32) >= 2048 needs nblk >= 65505.  Linear, f64 only: 2^24 knots
                               whose steps differ by a bounded ratio span 2^24 steps, where f32 (2^23 values per binade) no
                               longer tells neighbouring knots apart -- no uneven f32 axis of this length exists.
  offsets, a thread per lane   4353 x 33 and x 36: lanes > 32 leave the staged kernel, 18 blocks > AD_FUSE_BLOCKS = 17 leave the
                               fused add: antideriv_offsets_kernel<T, false>, antideriv_add_kernel<T, 1 | VN, false>.
  fuse boundary                4352 x 36: 17 blocks, the last shape whose add kernel sums the totals itself.
  staged boundary              4353 x 32: the widest staged row (kb = 1) with the WAVE offsets kernel over 18 totals.
  block edges                  256, 512, 513 x 5 and x 40: one full block (255 intervals, the nint < cnt store under
                               `single`), two blocks, a third block of one knot; staged and lanes kernels.
  vector chains                n = 256 * ceil(CU * 512 / (4096 / VN)) + 3, x 4096: antideriv_local_lanes_kernel with VN > 1
                               needs nblk * lanes / VN >= CU * 512 chains; the + 3 gives a last block of 2 intervals.  The
                               one heavy case (two tables of 512 MiB); Linear in both dtypes, Pchip in f64.

Evaluation (n x lanes, queries; LV = lanes / VN in the vector form):

  rows, ragged tail and query stride   5 x VN*257, 65 600 queries: segs = 2, the second holds ONE vector (v >= LV for the
                                       rest); gridDim.x = 65 536 so 64 blocks take a second query (qi += gridDim.x).  The
                                       first error at 65 570 is found by block 34 on that second pass.
  rows, segment stride                 3 x VN*16385, 9 queries: 65 segments on gridDim.y = 64 (seg += gridDim.y).
  flat, tile stride, scalar            7 x 513, 16 500 queries: tile_q = 1024 / 513 = 1, 16 500 tiles on 16 384 workgroups.
  flat, tile stride, vectors           7 x VN*255, 4 * 16 384 + 3 queries: tile_q = 4, 16 385 tiles, the last of 3 queries.
  flat, tile_q clamp                   4 x 1025, 50 queries: 1024 / LV = 0 is clamped to 1; also into a row stride lanes + 1.
  host output in two chunks            f64, 6 x 4096, 8192 + 100 host rows of 32 KiB: the 256 MiB staging buffer holds 8192.
  async_launch, finish()               a failing query reported by finish() through ws.last_q / last_q2.

Left out on purpose: the 64-bit index branch of antideriv_add_kernel (n * LV > 2^32 - 1) and the grid caps 1 << 16 (staged
tiles) and 1 << 20 (lanes / add workgroups) need tables of several GiB."""
import os
import re

import numpy as np
import pytest

import antiderivative_ref as ar
from hostile_inputs import check_bits
from test_gpu_antiderivative import build, queries, reference, tables_of
from test_gpu_parity import check_equal

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
SOURCES = ["linear", "pchip"]
B = ar.B
SENTINEL = -7.0
BUILD = re.compile(r"\[ndi plan\] antiderivative build linear=(\d+) staged=(\d+) kb=(\d+) vec=(\d+) vec_local=(\d+) nblk=(\d+) "
                   r"single=(\d+) fuse=(\d+) grid=(\d+)\n")
BUILD_FIELDS = ("linear", "staged", "kb", "vec", "vec_local", "nblk", "single", "fuse", "grid")
EVAL = re.compile(r"\[ndi plan\] antiderivative eval form=(rows|flat) linear=(\d+) pair=(\d+) vec=(\d+) lv=(\d+) tile_q=(\d+) "
                  r"grid=(\d+) x (\d+)\n")
EVAL_FIELDS = ("form", "linear", "pair", "vec", "lv", "tile_q", "gx", "gy")


def vn(dt):
    return 16 // np.dtype(dt).itemsize          # elements of a 16-byte vector


def traced(capfd, call, raises=None):
    """(result, build plans, evaluation plans): the call under NDI_TRACE_PLAN and the fields of every antiderivative plan
    line it printed.  `raises`: the exception class the call has to raise; the exception is the result then."""
    capfd.readouterr()
    before = os.environ.get("NDI_TRACE_PLAN")
    os.environ["NDI_TRACE_PLAN"] = "1"
    try:
        if raises is None:
            r = call()
        else:
            with pytest.raises(raises) as caught:
                call()
            r = caught.value
    finally:
        if before is None:
            del os.environ["NDI_TRACE_PLAN"]
        else:
            os.environ["NDI_TRACE_PLAN"] = before
    err = capfd.readouterr().err
    builds = [dict(zip(BUILD_FIELDS, (int(v) for v in m.groups()))) for m in BUILD.finditer(err)]
    evals = [dict(zip(EVAL_FIELDS, (m.group(1),) + tuple(int(v) for v in m.groups()[1:]))) for m in EVAL.finditer(err)]
    return r, builds, evals


def expect_plan(plans, count, what, **fields):
    assert len(plans) == count, f"{what}: {len(plans)} plan lines where {count} were expected: {plans}"
    for p in plans:
        got = {k: p[k] for k in fields}
        assert got == fields, f"{what}: plan {p} where {fields} was expected"


def dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


def to_np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def sentinel_buffer(shape, dt, on_device):
    import torch
    if on_device:
        return torch.full(shape, SENTINEL, dtype=torch.float32 if np.dtype(dt) == np.float32 else torch.float64, device="cuda:0")
    return np.full(shape, SENTINEL, dt)


def table(rng, n, L, dt):
    x = np.cumsum(rng.uniform(0.5, 2.0, n)).astype(dt)
    assert np.all(x[1:] > x[:-1])
    return x, rng.standard_normal((n, L), dtype=dt)


def message_of(pkg, src, value):
    """the source handle's own error for the one query `value`"""
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        src.interp_array(np.array([value], dtype=src.x.dtype))
    return str(e.value)


# ---- build ------------------------------------------------------------------------------------------------------------------
def build_queries(rng, x):
    """test_gpu_antiderivative's query set on 40 knots, and the same kinds of points inside the last two blocks: their first
    and last knots, the knots around the edge between them, the neighbouring floats, random points"""
    dt = x.dtype
    tail = x[max(0, ((len(x) - 1) // B - 1) * B):]
    at = [0, 1, len(tail) - 2, len(tail) - 1] + [k for k in (B - 1, B, B + 1) if k < len(tail)] + list(rng.integers(0, len(tail), 12))
    kn = tail[np.unique(np.clip(at, 0, len(tail) - 1))]
    more = np.concatenate([kn, np.nextafter(kn[1:], dt.type(-np.inf)), np.nextafter(kn[:-1], dt.type(np.inf)),
                           rng.uniform(tail[0], tail[-1], 20).astype(dt)])
    more = more[(more >= x[0]) & (more <= x[-1])]
    return np.ascontiguousarray(np.concatenate([queries(rng, x, 40, False), more]).astype(dt))


def check_build(pkg, capfd, rng, dt, source, n, L, **fields):
    what = f"{source} {n} x {L} {np.dtype(dt).name}"
    x, y = table(rng, n, L, dt)
    src = build(pkg, source, x, y)
    t = tables_of(src)
    P = ar.prefix(x, *t)
    F, builds, _ = traced(capfd, src.antiderivative)
    expect_plan(builds, 1, what, linear=int(source == "linear"), nblk=-(-n // B), **fields)
    got = F.strategy.data_table()
    check_equal(got, P, what + ": prefix table")
    check_bits(got, P, what + ": prefix table, signs of zero")
    q = build_queries(rng, x)
    ref = reference(x, t, P, q)
    check_bits(F.interp_array(q).reshape(ref.shape), ref, what + ": host rows")
    check_bits(to_np(F.interp_array(dev(q))).reshape(ref.shape), ref, what + ": device rows")


# n, lanes, sources, dtypes, the plan.  grid: the local kernel's (staged: the tiles).
STAGED_CHAINS = {
    "two-chains-odd-tile-count": (4095 * B, 1, SOURCES, DTYPES, dict(staged=1, kb=2, grid=2048, single=0, fuse=0)),
    "two-chains-last-block-of-one-knot": (4096 * B + 1, 1, SOURCES, DTYPES, dict(staged=1, kb=2, grid=2049, single=0, fuse=0)),
    "two-chains-of-16-lanes": (4095 * B + 7, 16, SOURCES, DTYPES, dict(staged=1, kb=2, grid=2048, vec=1, fuse=0)),
    "five-chains-of-3-lanes": (10236 * B + 100, 3, SOURCES, DTYPES, dict(staged=1, kb=5, grid=2048, vec=0, fuse=0)),
    "32-chains": (65505 * B + 2, 1, ["linear"], [np.float64], dict(staged=1, kb=32, grid=2048, fuse=0)),
}


@pytest.mark.parametrize("case,dt", [(c, dt) for c, v in STAGED_CHAINS.items() for dt in v[3]],
                         ids=[f"{c}-{np.dtype(dt).name}" for c, v in STAGED_CHAINS.items() for dt in v[3]])
def test_several_chains_per_workgroup(pkg, capfd, case, dt):
    n, L, sources, _, plan = STAGED_CHAINS[case]
    rng = np.random.default_rng([n, L])
    for source in sources:
        check_build(pkg, capfd, rng, dt, source, n, L, vec_local=0, **plan)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,L,plan", [
    (4353, 33, dict(staged=0, kb=0, fuse=0, vec=0, vec_local=0, single=0)),     # offsets: one thread per lane, scalar add
    (4353, 36, dict(staged=0, kb=0, fuse=0, vec=1, vec_local=0, single=0)),     # ... 16-byte add
    (4352, 36, dict(staged=0, kb=0, fuse=1, vec=1, vec_local=0, single=0)),     # 17 blocks: the fused add
    (4353, 32, dict(staged=1, kb=1, fuse=0, vec=1, vec_local=0, single=0)),     # the widest staged row, WAVE offsets, 18 totals
], ids=["offsets-33", "offsets-36", "fuse-17-blocks", "staged-32-lanes"])
def test_offsets_fuse_and_staged_boundaries(pkg, capfd, dt, n, L, plan):
    rng = np.random.default_rng([n, L, 1])
    for source in SOURCES:
        check_build(pkg, capfd, rng, dt, source, n, L, **plan)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("L", [5, 40])
@pytest.mark.parametrize("n", [256, 512, 513])
def test_block_edges(pkg, capfd, dt, n, L):
    rng = np.random.default_rng([n, L, 2])
    for source in SOURCES:
        check_build(pkg, capfd, rng, dt, source, n, L, staged=int(L <= 32), single=int(n == 256), fuse=int(n > 256),
                    kb=int(L <= 32), vec=int(L % vn(dt) == 0), vec_local=0)


@pytest.mark.parametrize("dt,source", [(np.float64, "linear"), (np.float32, "linear"), (np.float64, "pchip")],
                         ids=["f64-linear", "f32-linear", "f64-pchip"])
def test_vector_chains(pkg, capfd, dt, source):
    """The one heavy case: the product n * lanes is fixed by the threshold (67 M elements, 512 MiB a table).  The restatement
    runs over slices of lanes (lanes are independent), which keeps its temporaries small."""
    import torch
    L, V = 4096, vn(dt)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = B * -(-cu * 512 // (L // V)) + 3
    nblk = -(-n // B)
    assert nblk * (L // V) >= cu * 512 > 17 * (L // V)
    what = f"vector chains {source} {n} x {L} {np.dtype(dt).name}"
    rng = np.random.default_rng([n, L, 3])
    x, y = table(rng, n, L, dt)
    src = build(pkg, source, x, y)
    del y
    t = tables_of(src)
    strat, builds, _ = traced(capfd, src.strategy.antiderivative)
    expect_plan(builds, 1, what, linear=int(source == "linear"), staged=0, kb=0, vec=1, vec_local=1, nblk=nblk, single=0, fuse=0)
    got = strat.data_table()
    P = np.empty_like(got)
    for l0 in range(0, L, 512):
        P[:, l0:l0 + 512] = ar.prefix(x, *(None if v is None else np.ascontiguousarray(v[:, l0:l0 + 512]) for v in t))
    check_bits(got, P, what + ": prefix table")
    F = pkg.Interp1D(src.x, got, strat)
    q = build_queries(rng, x)
    ref = reference(x, t, P, q)
    check_bits(to_np(F.interp_array(dev(q))).reshape(ref.shape), ref, what + ": device rows")


# ---- evaluation -------------------------------------------------------------------------------------------------------------
class Handle:
    """A small table, its antiderivative handle held to the restatement, and a pool of query points (every knot, the floats
    next to the knots, 200 random points) with the restatement's rows: a batch of any length draws its queries from the
    pool, so its expected rows are a gather and cost no second restatement."""

    def __init__(self, pkg, rng, dt, source, n, L):
        self.pkg, self.rng, self.dt, self.source, self.L = pkg, rng, np.dtype(dt), source, L
        self.x, y = table(rng, n, L, dt)
        x = self.x
        self.src = build(pkg, source, x, y)
        t = tables_of(self.src)
        P = ar.prefix(x, *t)
        self.F = self.src.antiderivative()
        check_bits(self.F.strategy.data_table(), P, f"{source} {n} x {L}: prefix table")
        T = self.dt.type
        self.pool = np.concatenate([x, np.nextafter(x[1:], T(-np.inf)), np.nextafter(x[:-1], T(np.inf)),
                                    rng.uniform(x[0], x[-1], 200).astype(dt)])
        self.rows = reference(x, t, P, self.pool)
        self.above, self.below = x[-1] + T(1.0), x[0] - T(3.0)

    def batch(self, nq):
        """(queries, expected rows)"""
        pick = self.rng.integers(0, len(self.pool), nq)
        return np.ascontiguousarray(self.pool[pick]), self.rows[pick]

    def pairs(self, nq):
        """(lo, hi, expected F(hi) - F(lo)): one subtraction, as ar.integrate"""
        lo, hi = self.rng.integers(0, len(self.pool), nq), self.rng.integers(0, len(self.pool), nq)
        return np.ascontiguousarray(self.pool[lo]), np.ascontiguousarray(self.pool[hi]), self.rows[hi] - self.rows[lo]

    def plan(self, **fields):
        return dict(linear=int(self.source == "linear"), **fields)


def check_first_error(h, capfd, q, want, pos, what, **plan):
    """eval into a sentinel-filled device buffer: a first error at `pos`, a later one that must not be the one reported"""
    pkg = h.pkg
    bad = q.copy()
    bad[pos] = h.above
    bad[pos + 9] = h.below
    buf = sentinel_buffer(want.shape, h.dt, True)
    e, _, evals = traced(capfd, lambda: h.F.interp_array_into(dev(bad), buf), pkg.InterpolateError.OutOfBounds)
    expect_plan(evals, 1, what, **h.plan(pair=0, **plan))
    assert (e.index, e.value) == (pos, float(h.above)) and str(e) == message_of(pkg, h.src, h.above), f"{what}: {e!r} {e.index}"
    rows = to_np(buf)
    check_bits(rows[:pos], want[:pos], what + ": rows before the failure")
    assert np.all(rows[pos:] == SENTINEL), what + ": rows from the failure on keep the sentinel"


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_rows_ragged_tail_and_query_stride(pkg, capfd, dt, source):
    nq, pos = 65_600, 65_570
    h = Handle(pkg, np.random.default_rng(257), dt, source, 5, vn(dt) * 257)
    plan = dict(form="rows", vec=1, lv=257, tile_q=0, gx=65_536, gy=2)
    what = f"ragged rows {source} {h.dt.name}"
    q, want = h.batch(nq)
    rows, _, evals = traced(capfd, lambda: h.F.interp_array(dev(q)))
    expect_plan(evals, 1, what, **h.plan(pair=0, **plan))
    check_bits(to_np(rows), want, what)
    del rows
    check_first_error(h, capfd, q, want, pos, what + ", first error", **plan)
    del want
    lo, hi, want = h.pairs(nq)
    rows, _, evals = traced(capfd, lambda: h.F.integrate(dev(lo), dev(hi)))
    expect_plan(evals, 1, what + ", integrate", **h.plan(pair=1, **plan))
    check_bits(to_np(rows), want, what + ", integrate")
    del rows
    hi[pos] = h.below                  # a failing hi: axis 1; the later failing lo is not the one reported
    lo[pos + 9] = h.above
    buf = sentinel_buffer(want.shape, dt, True)
    e, _, evals = traced(capfd, lambda: h.F.strategy.integrate_into(dev(lo), dev(hi), buf), pkg.InterpolateError.OutOfBounds)
    expect_plan(evals, 1, what + ", integrate, first error", **h.plan(pair=1, **plan))
    assert (e.index, e.axis, e.value) == (pos, 1, float(h.below))
    rows = to_np(buf)
    check_bits(rows[:pos], want[:pos], what + ", integrate: rows before the failure")
    assert np.all(rows[pos:] == SENTINEL), what + ", integrate: rows from the failure on keep the sentinel"


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_rows_segment_stride(pkg, capfd, dt, source):
    h = Handle(pkg, np.random.default_rng(16_385), dt, source, 3, vn(dt) * 16_385)
    plan = dict(form="rows", vec=1, lv=16_385, tile_q=0, gx=9, gy=64)
    what = f"segment stride {source} {h.dt.name}"
    q, want = h.batch(9)
    rows, _, evals = traced(capfd, lambda: h.F.interp_array(dev(q)))
    expect_plan(evals, 1, what, **h.plan(pair=0, **plan))
    check_bits(to_np(rows), want, what)
    buf = sentinel_buffer(want.shape, dt, True)
    _, _, evals = traced(capfd, lambda: h.F.interp_array_into(dev(q), buf))
    expect_plan(evals, 1, what + " into", **h.plan(pair=0, **plan))
    check_bits(to_np(buf), want, what + " into")
    lo, hi, want = h.pairs(9)
    rows, _, evals = traced(capfd, lambda: h.F.integrate(dev(lo), dev(hi)))
    expect_plan(evals, 1, what + ", integrate", **h.plan(pair=1, **plan))
    check_bits(to_np(rows), want, what + ", integrate")


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_flat_tile_stride_scalar(pkg, capfd, dt, source):
    nq, pos = 16_500, 16_450
    h = Handle(pkg, np.random.default_rng(513), dt, source, 7, 513)
    plan = dict(form="flat", vec=0, lv=513, tile_q=1, gx=16_384, gy=1)
    what = f"flat scalar {source} {h.dt.name}"
    q, want = h.batch(nq)
    rows, _, evals = traced(capfd, lambda: h.F.interp_array(dev(q)))
    expect_plan(evals, 1, what, **h.plan(pair=0, **plan))
    check_bits(to_np(rows), want, what)
    check_first_error(h, capfd, q, want, pos, what + ", first error", **plan)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_flat_tile_stride_vectors(pkg, capfd, dt, source):
    nq = 4 * 16_384 + 3
    h = Handle(pkg, np.random.default_rng(255), dt, source, 7, vn(dt) * 255)
    plan = dict(form="flat", vec=1, lv=255, tile_q=4, gx=16_384, gy=1)
    what = f"flat vectors {source} {h.dt.name}"
    q, want = h.batch(nq)
    rows, _, evals = traced(capfd, lambda: h.F.interp_array(dev(q)))
    expect_plan(evals, 1, what, **h.plan(pair=0, **plan))
    check_bits(to_np(rows), want, what)
    del rows
    buf = sentinel_buffer(want.shape, dt, True)
    _, _, evals = traced(capfd, lambda: h.F.interp_array_into(dev(q), buf))
    expect_plan(evals, 1, what + " into", **h.plan(pair=0, **plan))
    check_bits(to_np(buf), want, what + " into")


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_flat_tile_q_clamp(pkg, capfd, dt, source):
    nq, L = 50, 1025
    h = Handle(pkg, np.random.default_rng(1025), dt, source, 4, L)
    plan = dict(form="flat", vec=0, lv=L, tile_q=1, gx=nq, gy=1)
    what = f"tile_q clamp {source} {h.dt.name}"
    q, want = h.batch(nq)
    rows, _, evals = traced(capfd, lambda: h.F.interp_array(dev(q)))
    expect_plan(evals, 1, what, **h.plan(pair=0, **plan))
    check_bits(to_np(rows), want, what)
    wide = sentinel_buffer((nq, L + 1), dt, True)          # a view with the row stride lanes + 1
    _, _, evals = traced(capfd, lambda: h.F.strategy.interp_array_into(h.F, dev(q), wide[:, :L]))
    expect_plan(evals, 1, what + " strided", **h.plan(pair=0, **plan))
    w = to_np(wide)
    check_bits(w[:, :L], want, what + " strided")
    assert np.all(w[:, L] == SENTINEL), what + ": the pad column was written"
    lo, hi, want = h.pairs(nq)
    wide = sentinel_buffer((nq, L + 1), dt, True)
    _, _, evals = traced(capfd, lambda: h.F.strategy.integrate_into(dev(lo), dev(hi), wide[:, :L]))
    expect_plan(evals, 1, what + " strided, integrate", **h.plan(pair=1, **plan))
    w = to_np(wide)
    check_bits(w[:, :L], want, what + " strided, integrate")
    assert np.all(w[:, L] == SENTINEL), what + ", integrate: the pad column was written"


@pytest.mark.parametrize("source", SOURCES)
def test_host_output_in_two_chunks(pkg, capfd, source):
    """Rows of 4096 f64 are 32 KiB: the 256 MiB staging buffer holds 8192 of them, so 8292 host rows take two chunks (the
    `off` arithmetic), and a failure at 8192 + 50 is found in the second (index_offset; hipMemcpy2D of 50 rows)."""
    dt, L, nq, pos = np.float64, 4096, 8192 + 100, 8192 + 50
    h = Handle(pkg, np.random.default_rng(4096), dt, source, 6, L)
    plan = dict(form="rows", vec=1, lv=L // 2, tile_q=0, gy=8)
    what = f"two chunks {source}"
    q, want = h.batch(nq)
    out = sentinel_buffer((nq, L), dt, False)
    _, _, evals = traced(capfd, lambda: h.F.interp_array_into(q, out))
    expect_plan(evals, 2, what, **h.plan(pair=0, **plan))
    assert [p["gx"] for p in evals] == [8192, 100], evals
    check_bits(out, want, what)
    bad = q.copy()
    bad[pos] = h.above
    bad[pos + 9] = h.below
    for on_device in (False, True):
        w = f"{what}, first error, device queries={on_device}"
        out[...] = SENTINEL
        e, _, evals = traced(capfd, lambda: h.F.interp_array_into(dev(bad) if on_device else bad, out),
                             pkg.InterpolateError.OutOfBounds)
        expect_plan(evals, 2, w, **h.plan(pair=0, **plan))
        assert (e.index, e.value) == (pos, float(h.above)) and str(e) == message_of(pkg, h.src, h.above), f"{w}: {e!r} {e.index}"
        check_bits(out[:pos], want[:pos], w + ": rows before the failure")
        assert np.all(out[pos:] == SENTINEL), w + ": rows from the failure on keep the sentinel"
    del want
    lo, hi, want = h.pairs(nq)
    out[...] = SENTINEL
    _, _, evals = traced(capfd, lambda: h.F.strategy.integrate_into(lo, hi, out))
    expect_plan(evals, 2, what + ", integrate", **h.plan(pair=1, **plan))
    check_bits(out, want, what + ", integrate")
    hi[pos] = h.below
    lo[pos + 9] = h.above
    out[...] = SENTINEL
    e, _, evals = traced(capfd, lambda: h.F.strategy.integrate_into(lo, hi, out), pkg.InterpolateError.OutOfBounds)
    expect_plan(evals, 2, what + ", integrate, first error", **h.plan(pair=1, **plan))
    assert (e.index, e.axis, e.value) == (pos, 1, float(h.below))
    check_bits(out[:pos], want[:pos], what + ", integrate: rows before the failure")
    assert np.all(out[pos:] == SENTINEL), what + ", integrate: rows from the failure on keep the sentinel"


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n,L", [(300, 7), (40, 1024)], ids=["flat", "rows"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_async_launch_then_finish_with_a_failing_query(pkg, dt, n, L, source):
    """async_launch returns before the batch is checked; finish() reports what the synchronous call reports (collect() and
    report() through the workspace's last_q), and the rows before the failure are written."""
    nq, pos = 700, 431
    h = Handle(pkg, np.random.default_rng([n, L]), dt, source, n, L)
    q, want = h.batch(nq)
    q[pos] = h.above
    q[pos + 9] = h.below
    qd = dev(q)
    s = h.F.strategy
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        s.interp_array_into(h.F, qd, sentinel_buffer((nq, L), dt, True))
    sync = (type(e.value), str(e.value), e.value.index, e.value.value)
    assert sync[1:] == (message_of(pkg, h.src, h.above), pos, float(h.above))
    buf = sentinel_buffer((nq, L), dt, True)
    s.interp_array_into(h.F, qd, buf, async_launch=True)            # no error yet
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        s.finish()
    assert (type(e.value), str(e.value), e.value.index, e.value.value) == sync
    rows = to_np(buf)
    check_bits(rows[:pos], want[:pos], "rows before the failure")
    assert np.all(rows[pos:] == SENTINEL), "rows from the failure on keep the sentinel"
    s.finish()                                                      # nothing pending: no second report
    good, want = h.batch(nq)
    check_bits(to_np(h.F.interp_array(dev(good))), want, "the handle still evaluates")


# ---- the bounds-checked build -----------------------------------------------------------------------------------------------
# test_gpu_antiderivative.py's test_checked_build_runs_the_new_kernels_clean carries the shapes of this file that the checked
# library has to see: kb > 1, the per-lane offsets kernel, the ragged rows tail.
