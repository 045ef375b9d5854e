"""The host engine behind the i32 / i64 and the f16 / bf16 handles, entry point by entry point: library-owned and
caller-supplied rings, host output with a row stride wider than the row, the sharded calls, async_launch + finish, trim
and the refusals.  Small shapes on purpose (9 knots, a 5 x 6 grid, 70 queries in chunks of 16 or 8): the code under test
is the host's call sequence -- slot reuse, the short last chunk, the copy back, the first-error bookkeeping -- not the
kernels.  Expected rows come from the package's host path (integers: the generic strategy; halves: the numpy
restatement of the `half` crate) and are compared exactly, integers by value and halves by bit pattern."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_half import bil_ref, build1d, build2d, lin_ref, r, tbits
from test_gpu_integer import _bil, _lin

pytestmark = pytest.mark.gpu
DTS = ["i32", "i64", "f16", "bf16"]
NQ, BAD, BAD_VALUE = 70, 37, 100
REFUSED = {True: "NDI_PATH_BUCKETED is not available for f16 / bf16 (AUTO / GATHER)",
           False: "NDI_PATH_BUCKETED is not available for integer element types (AUTO / GATHER)"}
_CASES = {}


class Case:
    """One interpolator shape: knots, data, 70 valid queries and their expected rows (storage type: the integer type,
    or uint16 bit patterns), plus the same queries with number 37 out of range (1-D: x, 2-D: y, so axis 1)."""

    def __init__(self, pkg, dt, lanes, dim):
        self.pkg, self.dt, self.lanes, self.dim = pkg, dt, lanes, dim
        self.half = dt in ("f16", "bf16")
        self.axis = dim - 1
        self.text = f"{'xy'[self.axis]} = {BAD_VALUE} is not in range"
        rng = np.random.default_rng(lanes * 10 + dim)
        if self.half:
            self.store = np.dtype(np.uint16)
            self.x = r(np.arange(9 if dim == 1 else 5, dtype=np.float32) * 0.5 - 2.0, dt)
            self.y = r(np.arange(6, dtype=np.float32) * 0.25 - 1.0, dt)
            shape = (9, lanes) if dim == 1 else (5, 6, lanes)
            self.data = r(rng.uniform(-1, 1, shape).astype(np.float32), dt)
            qx = r(rng.uniform(self.x[0], self.x[-1], NQ).astype(np.float32), dt)
            qy = r(rng.uniform(self.y[0], self.y[-1], NQ).astype(np.float32), dt)
            if dim == 1:
                self.want = lin_ref(self.x, self.data, qx, dt).reshape(NQ, lanes)
            else:
                self.want = bil_ref(self.x, self.y, self.data, qx, qy, dt).reshape(NQ, lanes)
            self.values = [qx] if dim == 1 else [qx, qy]            # f32 images
            self.q = [tbits(v, dt) for v in self.values]            # storage
        else:
            self.store = np.dtype(np.int32 if dt == "i32" else np.int64)
            self.x = np.cumsum(rng.integers(1, 9, 9 if dim == 1 else 5)).astype(self.store)
            self.y = (np.cumsum(rng.integers(1, 9, 6)) - 10).astype(self.store)
            shape = (9, lanes) if dim == 1 else (5, 6, lanes)
            self.data = rng.integers(-500, 500, shape).astype(self.store)
            qx = rng.integers(int(self.x[0]), int(self.x[-1]) + 1, NQ).astype(self.store)
            qy = rng.integers(int(self.y[0]), int(self.y[-1]) + 1, NQ).astype(self.store)
            if dim == 1:
                self.want = _lin(pkg, self.x, self.data, device=False).interp_array(qx)
            else:
                self.want = _bil(pkg, self.x, self.y, self.data, device=False).interp_array(qx, qy)
            self.want = np.ascontiguousarray(self.want, self.store).reshape(NQ, lanes)
            self.values = self.q = [qx] if dim == 1 else [qx, qy]
        self.want.setflags(write=False)
        bad = self.values[self.axis].copy()
        bad[BAD] = BAD_VALUE
        self.q_bad = list(self.q)
        self.q_bad[self.axis] = tbits(bad, dt) if self.half else bad
        self.sentinel = 0x7777 if self.half else 77
        self.interp = self.build()

    def build(self):
        if self.half:
            return build1d(self.pkg, self.x, self.data, self.dt) if self.dim == 1 else \
                build2d(self.pkg, self.x, self.y, self.data, self.dt)
        return _lin(self.pkg, self.x, self.data) if self.dim == 1 else _bil(self.pkg, self.x, self.y, self.data)

    def queries(self, bad):
        return self.q_bad if bad else self.q

    def dev(self, a):
        """A storage array as a device tensor (halves: int16, the same bits)."""
        import torch
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if self.half else np.ascontiguousarray(a)).to("cuda:0")

    def typed(self, t):
        """... seen as the element type the Python layer expects."""
        import torch
        return t.view(torch.float16 if self.dt == "f16" else torch.bfloat16) if self.half else t

    def host_typed(self, a):
        """A storage array as the host array the Python layer takes for this element type (bf16: its f32 values)."""
        if self.dt == "f16":
            return a.view(np.float16)
        if self.dt == "bf16":
            return (a.astype(np.uint32) << 16).view(np.float32)
        return a

    def filled(self, rows, cols, device=False):
        a = np.full((rows, cols), self.sentinel, self.store)
        return self.dev(a) if device else a

    def bits(self, t):
        """A device tensor (storage or typed) or host array as a storage array."""
        import torch
        if isinstance(t, torch.Tensor):
            t = t.detach().cpu()
            t = t.view(torch.int16).numpy().view(np.uint16) if self.half else t.numpy()
        return np.asarray(t).view(self.store)

    def handles(self, reps):
        return (C.c_void_p * len(reps))(*[i.strategy._h for i in reps])


def case(pkg, dt, lanes, dim):
    key = (dt, lanes, dim)
    if key not in _CASES:
        _CASES[key] = Case(pkg, dt, lanes, dim)
    return _CASES[key]


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _opts(pkg, q, out_device, path=0, async_launch=0, flags=0, stream=None):
    import torch
    o = pkg._capi.EvalOpts()
    o.q_memspace = pkg._capi.MEM_HOST if isinstance(q, np.ndarray) else pkg._capi.MEM_DEVICE
    o.out_memspace = pkg._capi.MEM_DEVICE if out_device else pkg._capi.MEM_HOST
    o.stream = torch.cuda.current_stream(0).cuda_stream if stream is None else stream
    o.path, o.async_launch, o.flags = path, async_launch, flags
    return o


def raw_eval(c, h, q, out, stride, nq=NQ, **kw):
    """ndi_interp{1,2}d_eval on storage buffers: (status, info, message)."""
    cap = c.pkg._capi
    opts = _opts(c.pkg, q[0], not isinstance(out, np.ndarray), **kw)
    info = cap.OobInfo()
    if c.dim == 1:
        st = cap.lib().ndi_interp1d_eval(h, _ptr(q[0]), nq, _ptr(out), stride, C.byref(opts), C.byref(info))
    else:
        st = cap.lib().ndi_interp2d_eval(h, _ptr(q[0]), _ptr(q[1]), nq, _ptr(out), stride, C.byref(opts), C.byref(info))
    return st, info, cap.last_error()


def raw_finish(c, h, info=None):
    import torch
    cap = c.pkg._capi
    info = info if info is not None else cap.OobInfo()
    fn = cap.lib().ndi_interp1d_finish if c.dim == 1 else cap.lib().ndi_interp2d_finish
    st = fn(h, torch.cuda.current_stream(0).cuda_stream, C.byref(info))
    return st, info, cap.last_error()


def raw_sharded(c, reps, q, io, stride, out_device, path=0):
    """ndi_interp{1,2}d_eval_sharded; q: the whole batch (host storage arrays) or None when io carries the blocks."""
    cap = c.pkg._capi
    opts = _opts(c.pkg, q[0] if q else None, out_device, path=path)
    if q is None:
        opts.q_memspace = cap.MEM_DEVICE
    info = cap.OobInfo()
    qx, qy = (_ptr(q[0]), _ptr(q[1]) if c.dim == 2 else None) if q else (None, None)
    if c.dim == 1:
        st = cap.lib().ndi_interp1d_eval_sharded(c.handles(reps), len(reps), qx, NQ, io, stride, C.byref(opts),
                                                 C.byref(info))
    else:
        st = cap.lib().ndi_interp2d_eval_sharded(c.handles(reps), len(reps), qx, qy, NQ, io, stride, C.byref(opts),
                                                 C.byref(info))
    return st, info, cap.last_error()


def is_oob(c, st, info, msg):
    cap = c.pkg._capi
    assert st == cap.OUT_OF_BOUNDS, (st, msg)
    assert (info.index, info.axis, info.status, info.value) == (BAD, c.axis, cap.OUT_OF_BOUNDS, float(BAD_VALUE))
    assert msg == c.text, msg


def raises_oob(c, call):
    with pytest.raises(c.pkg.InterpolateError.OutOfBounds) as e:
        call()
    assert e.value.index == BAD and e.value.axis == c.axis, (e.value.index, e.value.axis)
    assert c.pkg._capi.last_error() == c.text, c.pkg._capi.last_error()


def chunk_rows(c, ch):
    """The rows of a chunk in a library-owned ring, copied out on the chunk's stream (ordered before the slot's reuse)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                     C.c_void_p]
    host = np.empty((ch.q_count, c.lanes), c.store)
    isz = host.itemsize
    assert hip.hipMemcpy2DAsync(host.ctypes.data, c.lanes * isz, ch.out, ch.row_stride * isz, c.lanes * isz, ch.q_count,
                                2, ch.stream) == 0
    assert hip.hipStreamSynchronize(C.c_void_p(ch.stream)) == 0
    return host


# ---- 1, 2: rings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,own", [(1, True), (2, True), (2, False)])
@pytest.mark.parametrize("lanes", [3, 40])
@pytest.mark.parametrize("dt", DTS)
def test_ring_delivers_every_row_once_and_stops_at_the_failure(pkg, dt, lanes, dim, own):
    """70 queries in chunks of 16 through two slots: five chunks, the last one short, both slots reused."""
    import torch
    c = case(pkg, dt, lanes, dim)
    for bad in (False, True):
        qd = [c.typed(c.dev(a)) for a in c.queries(bad)]
        got = c.filled(NQ, lanes)
        seen = []
        slots = None if own else [c.typed(c.filled(16, lanes, device=True)) for _ in range(2)]

        def consumer(ch, rows):
            if own:
                assert rows is None and ch.row_stride == 2 * lanes
                host = chunk_rows(c, ch)
            else:
                assert rows.data_ptr() == ch.out == slots[ch.slot].data_ptr() and ch.row_stride == lanes
                host = c.bits(rows)
            assert (got[ch.q_begin:ch.q_begin + ch.q_count] == c.sentinel).all(), "a row delivered twice"
            got[ch.q_begin:ch.q_begin + ch.q_count] = host
            seen.append((ch.index, ch.q_begin, ch.q_count, ch.slot, ch.shard))

        def call():
            c.interp.interp_array_ring(*qd, 16, consumer, slots=slots, n_slots=2)
        rows = BAD if bad else NQ
        if bad:
            raises_oob(c, call)
        else:
            call()
        torch.cuda.synchronize()
        assert seen == [(k, 16 * k, min(16, rows - 16 * k), k % 2, 0) for k in range((rows + 15) // 16)], seen
        assert np.array_equal(got[:rows], c.want[:rows]), "delivered rows"
        assert (got[rows:] == c.sentinel).all(), "a row at or after the failure was delivered"


# ---- 3: host output, rows further apart than they are long ----------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("dt,lanes", [(dt, lanes) for dt in DTS for lanes in (3, 40)] + [("f16", 36), ("bf16", 36)])
def test_host_output_with_a_wide_row_stride(pkg, dt, lanes, dim):
    cap = pkg._capi
    c = case(pkg, dt, lanes, dim)
    h = c.interp.strategy._h
    for flags in (cap.EVAL_DEFAULT, cap.EVAL_FRESH_OUTPUT, cap.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED):
        out = c.filled(NQ, lanes + 2)
        st, info, msg = raw_eval(c, h, c.q, out, lanes + 2, flags=flags)
        assert st == cap.OK, msg
        assert np.array_equal(out[:, :lanes], c.want) and (out[:, lanes:] == c.sentinel).all(), flags
        out = c.filled(NQ, lanes + 2)
        is_oob(c, *raw_eval(c, h, c.q_bad, out, lanes + 2, flags=flags))
        assert np.array_equal(out[:BAD, :lanes], c.want[:BAD]) and (out[:BAD, lanes:] == c.sentinel).all(), flags
        if flags == cap.EVAL_DEFAULT:
            assert (out[BAD:] == c.sentinel).all(), "a caller-owned row at or after the failure was written"


# ---- 4: sharded -------------------------------------------------------------------------------------------------------
def _io(c, n, out, stride, streams=False):
    import torch
    io = (c.pkg._capi.ShardIO * n)()
    for i in range(n):
        lo, hi = c.pkg.sharding.shard_bounds(NQ, i, n)
        io[i].out = _ptr(out) + lo * stride * c.store.itemsize
        if streams:
            io[i].stream = torch.cuda.current_stream(0).cuda_stream
    return io


@pytest.mark.parametrize("n_rep", [2, 3])
@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("lanes", [3, 40])
@pytest.mark.parametrize("dt", DTS)
def test_sharded_rows_and_first_error_across_a_shard_boundary(pkg, dt, lanes, dim, n_rep):
    """Replicas on one device.  With three shards the blocks are [0, 24), [24, 47), [47, 70): query 37 fails in the
    middle one, the first shard writes all its rows and the last one none."""
    import torch
    cap = pkg._capi
    c = case(pkg, dt, lanes, dim)
    reps = [c.build() for _ in range(n_rep)]
    for device in (False, True):
        for bad in (False, True):
            out = c.filled(NQ, lanes, device=device)
            st, info, msg = raw_sharded(c, reps, c.queries(bad), _io(c, n_rep, out, lanes, streams=device), lanes, device)
            torch.cuda.synchronize()
            rows = BAD if bad else NQ
            if bad:
                is_oob(c, st, info, msg)
            else:
                assert st == cap.OK, msg
            got = c.bits(out)
            assert np.array_equal(got[:rows], c.want[:rows]), (device, bad)
            assert (got[rows:] == c.sentinel).all(), "a row at or after the failure was written"


@pytest.mark.parametrize("n_rep", [2, 3])
@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("lanes", [3, 40])
@pytest.mark.parametrize("dt", DTS)
def test_sharded_ring_chunks_are_globally_placed(pkg, dt, lanes, dim, n_rep):
    """Library-owned rings, chunks of 8: within a shard the chunks come in order, q_begin is the global index."""
    c = case(pkg, dt, lanes, dim)
    reps = [c.build() for _ in range(n_rep)]
    for bad in (False, True):
        got = c.filled(NQ, lanes)
        seen = [[] for _ in range(n_rep)]

        def consumer(ch, rows):
            assert rows is None and ch.row_stride == 2 * lanes
            host = chunk_rows(c, ch)
            assert (got[ch.q_begin:ch.q_begin + ch.q_count] == c.sentinel).all(), "a row delivered twice"
            got[ch.q_begin:ch.q_begin + ch.q_count] = host
            seen[ch.shard].append((ch.index, ch.q_begin, ch.q_count, ch.slot))

        def call():
            pkg.sharding.interp_array_ring_sharded(reps, *[c.host_typed(a) for a in c.queries(bad)], chunk_queries=8,
                                                   consumer=consumer, n_slots=2)
        rows = BAD if bad else NQ
        if bad:
            raises_oob(c, call)
        else:
            call()
        for i in range(n_rep):
            lo, hi = pkg.sharding.shard_bounds(NQ, i, n_rep)
            cnt = max(0, min(hi, rows) - lo)
            assert seen[i] == [(k, lo + 8 * k, min(8, cnt - 8 * k), k % 2) for k in range((cnt + 7) // 8)], (i, seen[i])
        assert np.array_equal(got[:rows], c.want[:rows]), "delivered rows"
        assert (got[rows:] == c.sentinel).all(), "a row at or after the failure was delivered"


@pytest.mark.parametrize("dt", DTS)
def test_sharded_per_shard_query_pointers(pkg, dt):
    """ndi_shard_io.q / .qy: every shard's block resident on its device, no whole-batch pointer."""
    import torch
    cap = pkg._capi
    c = case(pkg, dt, 3, 2)
    reps = [c.build() for _ in range(3)]
    for bad in (False, True):
        out = c.filled(NQ, 3, device=True)
        io = _io(c, 3, out, 3, streams=True)
        blocks = []
        for i in range(3):
            lo, hi = pkg.sharding.shard_bounds(NQ, i, 3)
            blocks.append([c.dev(a[lo:hi]) for a in c.queries(bad)])
            io[i].q, io[i].qy = blocks[i][0].data_ptr(), blocks[i][1].data_ptr()
        st, info, msg = raw_sharded(c, reps, None, io, 3, True)
        torch.cuda.synchronize()
        rows = BAD if bad else NQ
        if bad:
            is_oob(c, st, info, msg)
        else:
            assert st == cap.OK, msg
        got = c.bits(out)
        assert np.array_equal(got[:rows], c.want[:rows]) and (got[rows:] == c.sentinel).all(), bad


# ---- 5: async_launch, then finish -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [3, 40])
@pytest.mark.parametrize("dt", DTS)
def test_async_launch_then_finish_2d(pkg, dt, lanes):
    import torch
    cap = pkg._capi
    c = case(pkg, dt, lanes, 2)
    interp = c.build()   # a handle of its own: the test changes its state
    h = interp.strategy._h
    for bad in (False, True):
        qd = [c.dev(a) for a in c.queries(bad)]
        out = c.filled(NQ, lanes, device=True)
        st, info, msg = raw_eval(c, h, qd, out, lanes, async_launch=1)
        assert st == cap.OK, msg
        st, info, msg = raw_finish(c, h)
        torch.cuda.synchronize()
        rows = BAD if bad else NQ
        if bad:
            is_oob(c, st, info, msg)
        else:
            assert st == cap.OK and info.status == cap.OK, msg
        got = c.bits(out)
        assert np.array_equal(got[:rows], c.want[:rows]) and (got[rows:] == c.sentinel).all(), bad
        # nothing pending any more: OK; the integer handles leave *info alone, the half handles reset it
        again = cap.OobInfo()
        again.index = 99
        st, again, msg = raw_finish(c, h, again)
        assert st == cap.OK and again.index == (0 if c.half else 99)


# ---- 6: trim ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_trim_releases_scratch_and_the_handle_still_evaluates(pkg, dt):
    import torch
    cap = pkg._capi
    sets = cap.lib().ndi_interp1d_scratch_sets
    c = case(pkg, dt, 3, 1)
    interp = c.build()   # a handle of its own: the test changes its state
    h = interp.strategy._h
    assert sets(h) == 0
    if c.half:   # one scratch set per stream
        streams = [torch.cuda.Stream(0) for _ in range(2)]
        for s in streams:
            out = c.filled(NQ, 3)
            assert raw_eval(c, h, c.q, out, 3, stream=s.cuda_stream)[0] == cap.OK and np.array_equal(out, c.want)
        assert sets(h) == 2
    else:        # one per handle
        out = c.filled(NQ, 3)
        assert raw_eval(c, h, c.q, out, 3)[0] == cap.OK and np.array_equal(out, c.want)
        assert sets(h) == 1
    assert cap.lib().ndi_interp1d_trim(h) == cap.OK and sets(h) == 0
    out = c.filled(NQ, 3)
    assert raw_eval(c, h, c.q, out, 3)[0] == cap.OK and np.array_equal(out, c.want)
    is_oob(c, *raw_eval(c, h, c.q_bad, c.filled(NQ, 3), 3))
    if c.half:   # a pending async batch reads its stream's word at finish: trim keeps the scratch until then
        assert cap.lib().ndi_interp1d_trim(h) == cap.OK and sets(h) == 0
        qd = [c.dev(a) for a in c.q_bad]
        dout = c.filled(NQ, 3, device=True)
        assert raw_eval(c, h, qd, dout, 3, async_launch=1)[0] == cap.OK
        assert sets(h) == 1
        assert cap.lib().ndi_interp1d_trim(h) == cap.OK and sets(h) == 1
        is_oob(c, *raw_finish(c, h))
        got = c.bits(dout)
        assert np.array_equal(got[:BAD], c.want[:BAD]) and (got[BAD:] == c.sentinel).all()
        assert cap.lib().ndi_interp1d_trim(h) == cap.OK and sets(h) == 0


# ---- 7: refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("dt", DTS)
def test_refusals_keep_their_texts(pkg, dt, dim):
    cap = pkg._capi
    c = case(pkg, dt, 3, dim)
    h = c.interp.strategy._h
    out = c.filled(NQ, 3)
    # NDI_PATH_BUCKETED: eval, eval_ring, the sharded entry
    st, info, msg = raw_eval(c, h, c.q, out, 3, path=cap.PATH_BUCKETED)
    assert (st, msg) == (cap.UNSUPPORTED, REFUSED[c.half])
    ring = cap.RingDesc()
    ring.n_slots, ring.chunk_queries, ring.row_stride = 2, 16, 3
    opts = _opts(pkg, c.q[0], True, path=cap.PATH_BUCKETED)
    none = C.cast(None, cap.RING_CONSUMER)
    info = cap.OobInfo()
    if dim == 1:
        st = cap.lib().ndi_interp1d_eval_ring(h, _ptr(c.q[0]), NQ, C.byref(ring), none, None, C.byref(opts), C.byref(info))
    else:
        st = cap.lib().ndi_interp2d_eval_ring(h, _ptr(c.q[0]), _ptr(c.q[1]), NQ, C.byref(ring), none, None,
                                              C.byref(opts), C.byref(info))
    assert (st, cap.last_error()) == (cap.UNSUPPORTED, REFUSED[c.half])
    reps = [c.interp, c.build()]
    st, info, msg = raw_sharded(c, reps, c.q, _io(c, 2, out, 3), 3, False, path=cap.PATH_BUCKETED)
    assert (st, msg) == (cap.UNSUPPORTED, REFUSED[c.half])
    assert (out == c.sentinel).all()
    # rows that would overlap
    st, info, msg = raw_eval(c, h, c.q, out, 2)
    assert (st, msg) == (cap.BAD_ARG, "out_row_stride (2) < lanes (3)")
    if dim == 2:
        st, info, msg = raw_eval(c, h, [c.q[0], None], out, 3)
        assert (st, msg) == (cap.BAD_ARG, "null query pointer")
    assert (out == c.sentinel).all()


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
