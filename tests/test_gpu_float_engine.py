"""The host engine behind the f32 / f64 handles (csrc/float_host.hpp), entry point by entry point and family by family:
1-D Linear, 1-D CubicSpline, 2-D Bilinear, 2-D Bicubic, an antiderivative handle's eval and its integrate.  Small
shapes on purpose (12 knots, a 12 x 12 grid): the code under test is the host's call sequence -- staging, the first-error
bookkeeping with one query array or two, the copy back to a strided host buffer, chunk boundaries, slot reuse, shard
ownership -- not the kernels.  Expected rows are the same handle's device-output evaluation of the valid queries,
compared bit for bit; error reports are compared with the texts the host strategies (generic_host) and the oracle give:
"x = 100 is not in range" / "y = 100 is not in range".  An antiderivative's second array is `hi`, which is an x too:
its failures say "x = ..." with axis 1.

What the suite asserted before this file, as found by reading the tests named on the right (`rows`: a valid batch's
rows; `fail`: a failure's index / value / axis / text and the rows it leaves alone; `.`: nothing found, so this file adds
it; `-`: the family has no such path):

  path                                Linear  Cubic      Bilinear   Bicubic  anti eval  anti integrate
  zero-copy (host in, host out)       rows,   .          .          -        -          -          test_gpu_parity
                                      index                                                         (test_baseline_c1_exact_workload)
  zero-copy, wide stride, 2nd array   .       .          .          -        -          -
  small rows, device queries          .       .          .          -        -          -
  small rows beyond the 8 MiB bounce  .       .          .          -        -          -
  small rows, failure in chunk 2      .       .          .          -        -          -
  256 MiB chunks, failure in chunk 2  .       rows fail  rows       .        .          .          test_gpu_parity
                                                                                                    (test_host_output_is_streamed_in_chunks)
  async_launch + finish               .       fail       .          rows     rows       .          test_gpu_ring_and_devices, test_gpu_bicubic,
                                                                                                    test_gpu_antiderivative
  finish with nothing pending         .       .          .          .        .          .
  ring, failure at a chunk boundary   .       rows fail  rows fail  rows     -          -          test_gpu_ring_and_devices, test_gpu_bicubic
  sharded, error across shards        .       rows fail  rows fail  rows     -          -          test_gpu_sharded, test_gpu_bicubic
  sharded 2-D, y earlier than x       -       -          fail       .        -          -          test_gpu_sharded (test_sharded_2d_bilinear)
  sharded per-shard pointers, ring    .       rows       rows       .        -          -          test_gpu_sharded
  refusal texts                       .       .          .          .        BUCKETED   .          test_gpu_antiderivative
  nq == 0 and *info                   .       .          .          .        .          .

The existing tests use large shapes and one family each; the cells above are small and the same for every family.
Families without a path (n/a) are not skipped where the same call is still valid for them: a Bicubic or antiderivative
handle given a zero-copy-sized batch takes its general path and owes the caller the same rows and the same report."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
FAMILIES = ["linear", "cubic", "bilinear", "bicubic", "anti_eval", "anti_integrate"]
RING_FAMILIES = FAMILIES[:4]          # the antiderivative handle has no ring and no sharded call
BAD_VALUE, SENTINEL = 100.0, -7.0
_CASES, _WANT = {}, {}


class Case:
    """One handle of a family: its queries are one array (x) or two (x, y / lo, hi), all valid for every nq asked for."""

    def __init__(self, pkg, fam, dt, lanes):
        self.pkg, self.fam, self.dt, self.lanes = pkg, fam, np.dtype(dt), lanes
        self.narr = 2 if fam in ("bilinear", "bicubic", "anti_integrate") else 1
        self.kind = "2d" if fam in ("bilinear", "bicubic") else ("integrate" if fam == "anti_integrate" else "1d")
        rng = np.random.default_rng(len(fam) * 100 + lanes)
        self.x = np.cumsum(rng.uniform(0.25, 0.75, 12)).astype(dt)
        self.y = (np.cumsum(rng.uniform(0.25, 0.75, 12)) - 3.0).astype(dt)
        if self.kind == "2d":
            data = rng.uniform(-1, 1, (12, 12, lanes)).astype(dt)
            b = pkg.Interp2DBuilder.new(data).x(self.x).y(self.y)
            self.owner = (b.strategy(pkg.Bicubic.new()) if fam == "bicubic" else b).build()
            self.strategy = self.owner.strategy
        else:
            data = rng.uniform(-1, 1, (12, lanes)).astype(dt)
            b = pkg.Interp1DBuilder.new(data).x(self.x)
            self.owner = (b.strategy(pkg.CubicSpline.new()) if fam != "linear" else b).build()
            self.strategy = self.owner.strategy.antiderivative() if fam.startswith("anti") else self.owner.strategy
        self.h = self.strategy._h
        self.rng = rng

    def queries(self, nq):
        """nq valid queries per array (the same ones for the same nq)."""
        rng = np.random.default_rng(nq)
        second = self.y if self.kind == "2d" else self.x
        q = [rng.uniform(self.x[0], self.x[-1], nq).astype(self.dt)]
        if self.narr == 2:
            q.append(rng.uniform(second[0], second[-1], nq).astype(self.dt))
        return q

    def spoiled(self, q, axis, index):
        bad = [a.copy() for a in q]
        bad[axis][index] = BAD_VALUE
        return bad

    def text(self, axis):
        return f"{'y' if (axis == 1 and self.kind == '2d') else 'x'} = 100 is not in range"

    def want(self, nq):
        """The handle's device-output evaluation of queries(nq): (nq, lanes), read-only, computed once."""
        key = (self.fam, self.dt.str, self.lanes, nq)
        if key not in _WANT:
            import torch
            out = torch.full((nq, self.lanes), SENTINEL, dtype=tdtype(self.dt), device="cuda:0")
            st, info, msg = raw_eval(self, self.h, [dev(a) for a in self.queries(nq)], out, self.lanes, nq)
            assert st == self.pkg._capi.OK, msg
            torch.cuda.synchronize()
            _WANT[key] = out.cpu().numpy()
            _WANT[key].setflags(write=False)
        return _WANT[key]


def case(pkg, fam, dt, lanes):
    key = (fam, np.dtype(dt).str, lanes)
    if key not in _CASES:
        _CASES[key] = Case(pkg, fam, dt, lanes)
    return _CASES[key]


def tdtype(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _opts(pkg, q0, out_device, path=0, async_launch=0):
    import torch
    o = pkg._capi.EvalOpts()
    o.q_memspace = pkg._capi.MEM_HOST if (q0 is None or isinstance(q0, np.ndarray)) else pkg._capi.MEM_DEVICE
    o.out_memspace = pkg._capi.MEM_DEVICE if out_device else pkg._capi.MEM_HOST
    o.stream = torch.cuda.current_stream(0).cuda_stream
    o.path, o.async_launch = path, async_launch
    return o


def raw_eval(c, h, q, out, stride, nq, info=None, **kw):
    """ndi_interp1d_eval / ndi_interp2d_eval / ndi_interp1d_integrate: (status, info, message)."""
    cap = c.pkg._capi
    opts = _opts(c.pkg, q[0], out is not None and not isinstance(out, np.ndarray), **kw)
    info = info if info is not None else cap.OobInfo()
    if c.kind == "1d":
        st = cap.lib().ndi_interp1d_eval(h, _ptr(q[0]), nq, _ptr(out), stride, C.byref(opts), C.byref(info))
    elif c.kind == "2d":
        st = cap.lib().ndi_interp2d_eval(h, _ptr(q[0]), _ptr(q[1]), nq, _ptr(out), stride, C.byref(opts), C.byref(info))
    else:
        st = cap.lib().ndi_interp1d_integrate(h, _ptr(q[0]), _ptr(q[1]), nq, _ptr(out), stride, C.byref(opts),
                                              C.byref(info))
    return st, info, cap.last_error()


def raw_finish(c, h, info=None):
    import torch
    cap = c.pkg._capi
    info = info if info is not None else cap.OobInfo()
    fn = cap.lib().ndi_interp2d_finish if c.kind == "2d" else cap.lib().ndi_interp1d_finish
    st = fn(h, torch.cuda.current_stream(0).cuda_stream, C.byref(info))
    return st, info, cap.last_error()


def raw_ring(c, h, q, nq, ring, consumer, **kw):
    cap = c.pkg._capi
    opts = _opts(c.pkg, q[0], True, **kw)
    info = cap.OobInfo()
    cb = cap.RING_CONSUMER(consumer) if consumer else C.cast(None, cap.RING_CONSUMER)
    if c.kind == "2d":
        st = cap.lib().ndi_interp2d_eval_ring(h, _ptr(q[0]), _ptr(q[1]), nq, C.byref(ring), cb, None, C.byref(opts),
                                              C.byref(info))
    else:
        st = cap.lib().ndi_interp1d_eval_ring(h, _ptr(q[0]), nq, C.byref(ring), cb, None, C.byref(opts), C.byref(info))
    return st, info, cap.last_error()


def is_oob(c, res, index, axis):
    st, info, msg = res
    cap = c.pkg._capi
    assert st == cap.OUT_OF_BOUNDS, (st, msg)
    assert (info.index, info.axis, info.status, info.value) == (index, axis, cap.OUT_OF_BOUNDS, BAD_VALUE), \
        (info.index, info.axis, info.status, info.value)
    assert msg == c.text(axis), msg


def axes(c):
    """The arrays a failure is put on: the first, then the second alone."""
    return range(c.narr)


def check_host_rows(c, q, nq, bad, stride, device_q):
    """Host output `stride` apart: every row on a valid batch; with query `bad` spoiled, the rows below it, the report,
    and nothing else touched."""
    cap = c.pkg._capi
    want = c.want(nq)
    place = (lambda arrs: [dev(a) for a in arrs]) if device_q else (lambda arrs: arrs)
    out = np.full((nq, stride), SENTINEL, c.dt)
    st, info, msg = raw_eval(c, c.h, place(q), out, stride, nq)
    assert st == cap.OK, msg
    assert np.array_equal(out[:, :c.lanes], want) and (out[:, c.lanes:] == SENTINEL).all()
    for axis in axes(c):
        out = np.full((nq, stride), SENTINEL, c.dt)
        is_oob(c, raw_eval(c, c.h, place(c.spoiled(q, axis, bad)), out, stride, nq), bad, axis)
        assert np.array_equal(out[:bad, :c.lanes], want[:bad]), "rows below the failure"
        assert (out[:bad, c.lanes:] == SENTINEL).all() and (out[bad:] == SENTINEL).all(), "a byte outside them was written"


# ---- 1: host in, host out, a batch small enough for the zero-copy path ----------------------------------------------
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_small_host_batch_rows_report_and_untouched_rows(pkg, fam, dt, lanes):
    c = case(pkg, fam, dt, lanes)
    check_host_rows(c, c.queries(7), 7, 4, lanes + 2, device_q=False)


# ---- 2: the small-row host path with device queries (no zero copy) --------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_device_queries_host_output(pkg, fam, dt, lanes):
    c = case(pkg, fam, dt, lanes)
    check_host_rows(c, c.queries(7), 7, 4, lanes + 2, device_q=True)


@pytest.mark.parametrize("fam", FAMILIES)
def test_host_rows_beyond_the_pinned_bounce(pkg, fam):
    """70 000 rows of 128 bytes are 8.96 MB, more than the 8 MiB bounce: the strided copy straight from the device."""
    c = case(pkg, fam, "f8", 16)
    check_host_rows(c, c.queries(70_000), 70_000, 65_001, 18, device_q=True)


# ---- 3: a failure in the second 64 MiB chunk of the small-row path --------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_failure_in_the_second_small_row_chunk_has_the_global_index(pkg, fam):
    c = case(pkg, fam, "f8", 16)
    nq = 524_288 + 3           # 64 MiB / 128 B rows, and three more
    check_host_rows(c, c.queries(nq), nq, 524_288 + 1, 16, device_q=True)


# ---- 4: the general host-output loop: 256 MiB chunks ------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
def test_failure_in_the_second_256_mib_chunk_has_the_global_index(pkg, fam):
    """Rows of 32 KiB: 8192 of them fill the staging buffer, the batch has three more, the failure is the second of those
    (on the last array the family has)."""
    c = case(pkg, fam, "f8", 4096)
    nq, bad, axis = 8192 + 3, 8192 + 1, c.narr - 1
    want = c.want(nq)
    out = np.full((nq, 4096), SENTINEL)
    is_oob(c, raw_eval(c, c.h, c.spoiled(c.queries(nq), axis, bad), out, 4096, nq), bad, axis)
    assert np.array_equal(out[:bad], want[:bad]) and (out[bad:] == SENTINEL).all()


# ---- 5: async_launch, then finish -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_async_launch_then_finish(pkg, fam, dt):
    import torch
    cap = pkg._capi
    c = case(pkg, fam, dt, 3)
    nq, bad = 23, 17
    want = c.want(nq)
    runs = [(c.queries(nq), None)] + [(c.spoiled(c.queries(nq), axis, bad), axis) for axis in axes(c)]
    for q, axis in runs:
        qd = [dev(a) for a in q]
        out = torch.full((nq, 3), SENTINEL, dtype=tdtype(dt), device="cuda:0")
        st, info, msg = raw_eval(c, c.h, qd, out, 3, nq, async_launch=1)
        assert st == cap.OK and info.status == cap.OK, msg      # nothing is known yet
        res = raw_finish(c, c.h)                                # the report reads the first call's query arrays
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        if axis is None:
            assert res[0] == cap.OK, res[2]
            assert np.array_equal(got, want)
        else:
            is_oob(c, res, bad, axis)
            assert np.array_equal(got[:bad], want[:bad]) and (got[bad:] == SENTINEL).all()
        again = cap.OobInfo()
        again.index = 99
        st, again, msg = raw_finish(c, c.h, again)              # nothing pending: OK, *info left alone
        assert st == cap.OK and again.index == 99


# ---- 6: ring ----------------------------------------------------------------------------------------------------------
def chunk_rows(c, ch):
    """The rows of a ring chunk, copied out on the chunk's stream (ordered before the slot's reuse)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                     C.c_void_p]
    host = np.empty((ch.q_count, c.lanes), c.dt)
    isz = host.itemsize
    assert hip.hipMemcpy2DAsync(host.ctypes.data, c.lanes * isz, ch.out, ch.row_stride * isz, c.lanes * isz, ch.q_count,
                                2, ch.stream) == 0
    assert hip.hipStreamSynchronize(C.c_void_p(ch.stream)) == 0
    return host


def ring_desc(c, chunk, n_slots, slots=None):
    ring = c.pkg._capi.RingDesc()
    ring.n_slots, ring.chunk_queries, ring.row_stride = n_slots, chunk, c.lanes
    if slots is not None:
        ring.keep = (C.c_void_p * n_slots)(*[t.data_ptr() for t in slots])
        ring.slots = C.cast(ring.keep, C.POINTER(C.c_void_p))
    return ring


@pytest.mark.parametrize("own", [True, False])
@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", RING_FAMILIES)
def test_ring_delivers_the_chunks_below_the_failure(pkg, fam, dt, own):
    """23 queries in chunks of 5 through two slots, query 17 out of range: chunks 0..3, the last one of 2 rows."""
    import torch
    cap = pkg._capi
    c = case(pkg, fam, dt, 3)
    nq, bad = 23, 17
    want = c.want(nq)
    for q, axis in [(c.queries(nq), None)] + [(c.spoiled(c.queries(nq), axis, bad), axis) for axis in axes(c)]:
        slots = None if own else [torch.full((5, 3), SENTINEL, dtype=tdtype(dt), device="cuda:0") for _ in range(2)]
        got = np.full((nq, 3), SENTINEL, c.dt)
        seen = []

        def consumer(_user, cptr):      # (an exception would not cross the C frames: everything is recorded and asserted below)
            ch = cptr.contents
            got[ch.q_begin:ch.q_begin + ch.q_count] = chunk_rows(c, ch)
            in_slot = own or ch.out == slots[ch.slot].data_ptr()
            seen.append((ch.index, ch.q_begin, ch.q_count, ch.slot, ch.row_stride, ch.shard, in_slot))
            return None

        for place in ((lambda a: a), dev):          # host queries are staged once, device queries pass through
            got[:] = SENTINEL
            del seen[:]
            res = raw_ring(c, c.h, [place(a) for a in q], nq, ring_desc(c, 5, 2, slots), consumer)
            rows = nq if axis is None else bad
            if axis is None:
                assert res[0] == cap.OK, res[2]
            else:
                is_oob(c, res, bad, axis)
            assert seen == [(k, 5 * k, min(5, rows - 5 * k), k % 2, 6 if own else 3, 0, True)
                            for k in range((rows + 4) // 5)], seen
            assert np.array_equal(got[:rows], want[:rows]) and (got[rows:] == SENTINEL).all()


# ---- 7: sharded, replicas made by clone on one device ------------------------------------------------------------------
def replicas(c, n):
    reps = [c.strategy] + [c.strategy.clone(0) for _ in range(n - 1)]
    return reps, (C.c_void_p * n)(*[r._h for r in reps])


def shard_io(c, n, nq, out, stride, blocks=None):
    import torch
    io = (c.pkg._capi.ShardIO * n)()
    for i in range(n):
        lo, hi = c.pkg.sharding.shard_bounds(nq, i, n)
        if out is not None:
            io[i].out = _ptr(out) + lo * stride * c.dt.itemsize
        io[i].stream = torch.cuda.current_stream(0).cuda_stream
        if blocks is not None:
            io[i].q = blocks[i][0].data_ptr()
            io[i].qy = blocks[i][1].data_ptr() if c.narr == 2 else None
    return io


def raw_sharded(c, handles, n, q, nq, io, stride, out_device, ring=None, consumer=None, **kw):
    cap = c.pkg._capi
    opts = _opts(c.pkg, q[0] if q else None, out_device, **kw)
    if q is None:
        opts.q_memspace = cap.MEM_DEVICE
    info = cap.OobInfo()
    qs = [_ptr(a) for a in q] if q else [None] * c.narr
    two = [qs[1]] if c.kind == "2d" else []
    name = "ndi_interp2d_eval" if c.kind == "2d" else "ndi_interp1d_eval"
    if ring is None:
        st = getattr(cap.lib(), name + "_sharded")(handles, n, qs[0], *two, nq, io, stride, C.byref(opts), C.byref(info))
    else:
        cb = cap.RING_CONSUMER(consumer)
        st = getattr(cap.lib(), name + "_ring_sharded")(handles, n, qs[0], *two, nq, io, ring, cb, None, C.byref(opts),
                                                        C.byref(info))
    return st, info, cap.last_error()


@pytest.mark.parametrize("n_rep", [2, 3])
@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", RING_FAMILIES)
def test_sharded_first_error_across_a_shard_boundary(pkg, fam, dt, n_rep):
    """23 queries, blocks [0, 12), [12, 23) or [0, 8), [8, 16), [16, 23): query 13 fails in the second shard -- the first
    writes all its rows, a third none.  Then per-shard query pointers instead of the whole batch."""
    import torch
    cap = pkg._capi
    c = case(pkg, fam, dt, 3)
    nq, bad = 23, 13
    want = c.want(nq)
    reps, handles = replicas(c, n_rep)
    assert pkg.sharding.shard_bounds(nq, 0, n_rep)[1] <= bad
    for q, axis in [(c.queries(nq), None)] + [(c.spoiled(c.queries(nq), axis, bad), axis) for axis in axes(c)]:
        rows = nq if axis is None else bad
        for per_shard in (False, True):
            for device in (False, True):
                if per_shard and not device:
                    continue
                out = torch.full((nq, 3), SENTINEL, dtype=tdtype(dt), device="cuda:0") if device else \
                    np.full((nq, 3), SENTINEL, c.dt)
                blocks = None
                if per_shard:
                    bounds = [pkg.sharding.shard_bounds(nq, i, n_rep) for i in range(n_rep)]
                    blocks = [[dev(a[lo:hi]) for a in q] for lo, hi in bounds]
                res = raw_sharded(c, handles, n_rep, None if per_shard else q, nq, shard_io(c, n_rep, nq, out, 3, blocks),
                                  3, device)
                torch.cuda.synchronize()
                if axis is None:
                    assert res[0] == cap.OK, res[2]
                else:
                    is_oob(c, res, bad, axis)
                got = out.cpu().numpy() if device else out
                assert np.array_equal(got[:rows], want[:rows]) and (got[rows:] == SENTINEL).all(), (axis, per_shard, device)


@pytest.mark.parametrize("n_rep", [2, 3])
@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", ["bilinear", "bicubic"])
def test_sharded_2d_an_earlier_y_failure_beats_a_later_x_failure(pkg, fam, dt, n_rep):
    """x fails at 17 (the last shard), y at 5 (shard 0): the batch's first error is y's, axis 1, reported by shard 0,
    whose x word knows no failure at all."""
    c = case(pkg, fam, dt, 3)
    nq = 23
    want = c.want(nq)
    reps, handles = replicas(c, n_rep)
    q = c.spoiled(c.spoiled(c.queries(nq), 0, 17), 1, 5)
    out = np.full((nq, 3), SENTINEL, c.dt)
    is_oob(c, raw_sharded(c, handles, n_rep, q, nq, shard_io(c, n_rep, nq, out, 3), 3, False), 5, 1)
    assert np.array_equal(out[:5], want[:5]) and (out[5:] == SENTINEL).all()


@pytest.mark.parametrize("n_rep", [2, 3])
@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", RING_FAMILIES)
def test_sharded_ring_chunks_carry_global_indices(pkg, fam, dt, n_rep):
    """Library-owned rings, chunks of 5: within a shard the chunks come in order, q_begin is the batch's index."""
    cap = pkg._capi
    c = case(pkg, fam, dt, 3)
    nq, bad = 23, 13
    want = c.want(nq)
    reps, handles = replicas(c, n_rep)
    rings = (cap.RingDesc * n_rep)()
    for r in rings:
        r.n_slots, r.chunk_queries, r.row_stride = 2, 5, 3
    for q, axis in [(c.queries(nq), None)] + [(c.spoiled(c.queries(nq), axis, bad), axis) for axis in axes(c)]:
        got = np.full((nq, 3), SENTINEL, c.dt)
        seen = [[] for _ in range(n_rep)]

        def consumer(_user, cptr):      # (shards call it from their own host threads: one list per shard)
            ch = cptr.contents
            got[ch.q_begin:ch.q_begin + ch.q_count] = chunk_rows(c, ch)
            seen[ch.shard].append((ch.index, ch.q_begin, ch.q_count, ch.slot, ch.row_stride))
            return None

        res = raw_sharded(c, handles, n_rep, q, nq, shard_io(c, n_rep, nq, None, 3), 0, True, ring=rings,
                          consumer=consumer)
        rows = nq if axis is None else bad
        if axis is None:
            assert res[0] == cap.OK, res[2]
        else:
            is_oob(c, res, bad, axis)
        for i in range(n_rep):
            lo, hi = pkg.sharding.shard_bounds(nq, i, n_rep)
            cnt = max(0, min(hi, rows) - lo)
            assert seen[i] == [(k, lo + 5 * k, min(5, cnt - 5 * k), k % 2, 6) for k in range((cnt + 4) // 5)], (i, seen[i])
        assert np.array_equal(got[:rows], want[:rows]) and (got[rows:] == SENTINEL).all()


# ---- 8: refusals ------------------------------------------------------------------------------------------------------
BUCKETED = ("NDI_PATH_BUCKETED: an antiderivative handle evaluates in the two-kernel gather form only (its quartic needs "
            "the prefix table; the grouped forms do not read it)")


@pytest.mark.parametrize("dt", ["f4", "f8"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_refusals_keep_their_texts(pkg, fam, dt):
    cap = pkg._capi
    c = case(pkg, fam, dt, 3)
    anti = fam.startswith("anti")
    nq = 7
    q = c.queries(nq)
    out = np.full((nq, 3), SENTINEL, c.dt)
    st, info, msg = raw_eval(c, c.h, q, out, 2, nq)
    assert (st, msg) == (cap.BAD_ARG, "out_row_stride (2) < lanes (3)")
    for holes in ([0], [c.narr - 1], ["out"]):
        qq = [None if i in holes else a for i, a in enumerate(q)]
        st, info, msg = raw_eval(c, c.h, qq, None if "out" in holes else out, 3, nq)
        assert (st, msg) == (cap.BAD_ARG, "null query / output pointer"), holes
    # an empty batch is no error and needs no pointers; *info is the caller's for 1-D and 2-D, reset by an antiderivative
    mine = cap.OobInfo()
    mine.index, mine.axis = 99, 1
    st, mine, msg = raw_eval(c, c.h, [None] * c.narr, None, 3, 0, info=mine)
    assert st == cap.OK and (mine.index, mine.axis) == ((0, 0) if anti else (99, 1))
    ring = ring_desc(c, 5, 2)
    if anti:
        st, info, msg = raw_eval(c, c.h, q, out, 3, nq, path=cap.PATH_BUCKETED)
        assert (st, msg) == (cap.UNSUPPORTED, BUCKETED)
        if c.kind == "1d":
            st, info, msg = raw_ring(c, c.h, q, nq, ring, None)
            assert (st, msg) == (cap.UNSUPPORTED, "eval_ring: an antiderivative handle (of CubicSpline) has no ring "
                                 "evaluation; ndi_interp1d_eval chunk by chunk serves it")
            reps, handles = replicas(c, 2)
            st, info, msg = raw_sharded(c, handles, 2, q, nq, shard_io(c, 2, nq, out, 3), 3, False)
            assert (st, msg) == (cap.UNSUPPORTED, "the sharded calls do not take antiderivative handles "
                                 "(ndi_interp1d_eval per device serves them)")
    else:
        for holes in ([0], [c.narr - 1]):
            qq = [None if i in holes else a for i, a in enumerate(q)]
            st, info, msg = raw_ring(c, c.h, qq, nq, ring, None)
            assert (st, msg) == (cap.BAD_ARG, "null query pointer"), holes
        mine.index, mine.axis = 99, 1
        opts = _opts(pkg, None, True)
        none = C.cast(None, cap.RING_CONSUMER)
        if c.kind == "2d":
            st = cap.lib().ndi_interp2d_eval_ring(c.h, None, None, 0, C.byref(ring), none, None, C.byref(opts), C.byref(mine))
        else:
            st = cap.lib().ndi_interp1d_eval_ring(c.h, None, 0, C.byref(ring), none, None, C.byref(opts), C.byref(mine))
        assert st == cap.OK and (mine.index, mine.axis) == (99, 1)
    assert (out == SENTINEL).all()


def test_this_file_under_the_checked_library():
    """Every case again with the device-side index checks of the checked build recording any violation."""
    if os.environ.get("NDI_LIB"):
        pytest.skip("already running under another library")
    subprocess.run(["make", "-C", os.path.join(ROOT, "ndarray-interp_amd", "csrc"), "debug"], check=True,
                   capture_output=True)
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-k", "not checked_library", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
