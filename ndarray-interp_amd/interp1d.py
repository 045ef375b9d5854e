"""Host-side mirror of the reference's 1-D surface (src/interp1d/mod.rs + strategies/):
`Interp1DBuilder`, `Interp1D`, the strategy trait pair and the built-in `Linear` and `CubicSpline` -- plus
`Pchip`, `Akima` and `CubicHermite`, which the reference leaves to user strategies and this build runs on the device,
and `Interp1D.derivative(nu)` (scipy's name and meaning) for the four cubics, `Interp1D.antiderivative()` and
`Interp1D.integrate(lo, hi)` for every f32 / f64 strategy.

Names, argument meaning and error behaviour follow the reference so that the parity tests read like
its own tests.  The built-in strategies override the *batched* hook (`interp_array_into`) and call the
C ABI (include/ndinterp.h); the per-query hook `interp_into` -- the only thing the reference's trait has
(strategies/mod.rs:59-64) -- stays the extension point for user strategies, whose default batched hook
is the reference's own per-query loop (interp1d/mod.rs:326-343).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._arrays import (DEVICE_HALF_DTYPES, DEVICE_INT_DTYPES, OUTPUT_OWNED_MIN_BYTES, Buf, current_stream_ptr, dtype_id,
                      int_query, is_bf16, is_torch, np_dtype_of, output_empty, torch_dtype)
from .errors import BuilderError, InterpolateError, Panic, raise_builder, raise_eval
from .vector_extensions import Monotonic, get_lower_index, monotonic_prop


# ------------------------------------------------------------------------------------------------
# strategy traits (src/interp1d/strategies/mod.rs:12-65)
# ------------------------------------------------------------------------------------------------
class Interp1DStrategyBuilder:
    """Trait `Interp1DStrategyBuilder`: `MINIMUM_DATA_LENGHT` (sic) and `build(x, data)`."""

    MINIMUM_DATA_LENGHT = 2

    def build(self, x, data) -> "Interp1DStrategy":
        raise NotImplementedError


class Interp1DStrategy:
    """Trait `Interp1DStrategy`: per-query `interp_into(interpolator, target, x)`.

    `interp_array_into` is the defaulted batched hook added by this build: the default body is the
    reference's serial query loop, so strategies that only implement `interp_into`
    (examples/custom_strategy.rs) keep working unchanged on the host."""

    def interp_into(self, interpolator: "Interp1D", target: np.ndarray, x) -> None:
        raise NotImplementedError

    def interp_array_into(self, interpolator: "Interp1D", xs_flat, out2d) -> None:
        for i in range(len(xs_flat)):  # Zip(xs, rows).fold_while, stops at the first Err
            self.interp_into(interpolator, out2d[i].reshape(interpolator.data.shape[1:]), xs_flat[i])

    def release(self) -> None:
        pass


class _DeviceStrategy1D(Interp1DStrategy):
    """Shared body of the built-in strategies: owns an `ndi_interp1d*`."""

    _kind = _capi.LINEAR
    path = _capi.PATH_AUTO  # evaluation formulation, see include/ndinterp.h ndi_path

    def __init__(self):
        self._h = None
        self._device = 0
        self._np_dtype = None
        self._lanes = 1
        self._inflight = []

    # -- build ------------------------------------------------------------------------------
    def _create(self, x, data, *, extrapolate, periodic=False, left=(0, 0.0), right=(0, 0.0),
                per_lane=None, device=None, build_flags=0, dydx=None, lane_axes=False):
        xb_dt = np_dtype_of(data)
        tid = dtype_id(xb_dt)
        db = Buf(data)
        xb = None
        if x is not None:   # the axis travels in the same memory space as the data
            xb = Buf(_host(x), xb_dt) if db.memspace == _capi.MEM_HOST else Buf(_to_device(x, db.keep.device), xb_dt)
        if device is None:
            device = db.device if db.memspace == _capi.MEM_DEVICE else _default_device()
        n = db.shape[0]
        lanes = int(np.prod(db.shape[1:], dtype=np.int64)) if len(db.shape) > 1 else 1
        d = _capi.Interp1DDesc()
        d.dtype, d.strategy, d.extrapolate, d.device = tid, self._kind, int(bool(extrapolate)), device
        d.n, d.lanes = n, lanes
        d.x_len = xb.size if xb is not None and not lane_axes else n
        d.x = xb.ptr if xb is not None and not lane_axes else None   # (lane axes: the knot table is an argument of its own)
        d.data = db.ptr
        d.memspace = db.memspace
        d.validate = 0  # Interp1DBuilder.build() has validated already, as in the reference (:449-473)
        d.periodic = int(bool(periodic))
        d.build_flags = int(build_flags)
        d.left = _capi.Boundary(int(left[0]), float(left[1]))
        d.right = _capi.Boundary(int(right[0]), float(right[1]))
        keep = []
        if per_lane is not None:
            lk, lv, rk, rv = per_lane
            lk = np.ascontiguousarray(lk, np.int32); rk = np.ascontiguousarray(rk, np.int32)
            lv = np.ascontiguousarray(lv, np.float64); rv = np.ascontiguousarray(rv, np.float64)
            keep = [lk, lv, rk, rv]
            d.lane_left_kind, d.lane_left_value = lk.ctypes.data, lv.ctypes.data
            d.lane_right_kind, d.lane_right_value = rk.ctypes.data, rv.ctypes.data
        h = C.c_void_p()
        kb = None
        if dydx is not None:   # CubicHermite: the derivatives travel in the same memory space as the data
            kb = Buf(_host(dydx), xb_dt) if db.memspace == _capi.MEM_HOST else Buf(_to_device(dydx, db.keep.device), xb_dt)
            keep.append(kb)
        if lane_axes:   # x is the knot table (n, lanes...), a column per lane (ndi_interp1d_create_lane_axes)
            st = _capi.lib().ndi_interp1d_create_lane_axes(C.byref(d), xb.ptr, kb.ptr if kb is not None else None,
                                                           C.byref(h))
            if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):   # the library's refusals, with its reason
                raise ValueError(_capi.last_error())
        elif kb is not None:
            st = _capi.lib().ndi_interp1d_create_hermite(C.byref(d), kb.ptr, C.byref(h))
        else:
            st = _capi.lib().ndi_interp1d_create(C.byref(d), C.byref(h))
        del keep
        if st != _capi.OK:
            raise_builder(st)
        self._h, self._device, self._np_dtype, self._lanes, self._n = h, device, xb_dt, lanes, n
        return self

    def release(self):
        if self._h is not None:
            _capi.lib().ndi_interp1d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def clone(self, device: int):
        """A replica of this finished strategy on `device` (ndi_interp1d_clone): tables copied device to device."""
        import copy
        h = C.c_void_p()
        st = _capi.lib().ndi_interp1d_clone(self._h, int(device), C.byref(h))
        if st != _capi.OK:
            raise_builder(st)
        other = copy.copy(self)
        other._h, other._device, other._inflight = h, int(device), []
        return other

    def data_table(self, device: bool = False):
        """The handle's resident data table `(n, lanes)` (ndi_interp1d_data): a numpy array, or with `device=True` a
        tensor on the handle's device.  For a derivative handle this is the derivative at the knots."""
        shape = (self._n, self._lanes)
        if device or is_bf16(self._np_dtype):
            import torch
            out = torch.empty(shape, dtype=torch_dtype(self._np_dtype), device=f"cuda:{self._device}")
            st = _capi.lib().ndi_interp1d_data(self._h, out.data_ptr(), _capi.MEM_DEVICE)
        else:
            out = np.empty(shape, dtype=self._np_dtype)
            st = _capi.lib().ndi_interp1d_data(self._h, out.ctypes.data, _capi.MEM_HOST)
        if st != _capi.OK:
            raise_builder(st)
        return out

    def derivative(self, nu: int = 1) -> "DerivativeStrategy":
        """The `nu`-th derivative as a finished strategy of its own (ndi_interp1d_derivative): a new handle on this
        handle's device whose tables are derived from this handle's on the device.  This strategy stays usable.
        Orders the library refuses (include/ndinterp.h lists them) raise `ValueError` with its message."""
        import operator
        nu = operator.index(nu)
        h = C.c_void_p()
        st = _capi.lib().ndi_interp1d_derivative(self._h, nu, C.byref(h))
        if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):
            raise ValueError(_capi.last_error())
        if st != _capi.OK:
            raise_builder(st)
        d = DerivativeStrategy()
        d._h, d._device, d._np_dtype, d._lanes, d._n = h, self._device, self._np_dtype, self._lanes, self._n
        d.order = getattr(self, "order", 0) + nu
        d.origin = getattr(self, "origin", type(self))
        return d

    def antiderivative(self) -> "AntiderivativeStrategy":
        """The antiderivative `F` (`F(x[0]) = 0`) as a finished strategy of its own (ndi_interp1d_antiderivative): a new
        handle on this handle's device with a prefix table built there.  This strategy stays usable.  Sources the library
        refuses (include/ndinterp.h lists them) raise `ValueError` with its message."""
        h = C.c_void_p()
        st = _capi.lib().ndi_interp1d_antiderivative(self._h, C.byref(h))
        if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):
            raise ValueError(_capi.last_error())
        if st != _capi.OK:
            raise_builder(st)
        d = AntiderivativeStrategy()
        d._h, d._device, d._np_dtype, d._lanes, d._n = h, self._device, self._np_dtype, self._lanes, self._n
        d.origin = getattr(self, "origin", type(self))
        return d

    def inverse(self) -> "InverseStrategy":
        """The inverse `f^-1` as a finished strategy of its own (ndi_interp1d_inverse): a new handle on this handle's
        device whose queries are values `v` and whose rows are the abscissae `x` with `f_l(x) = v`.  This strategy stays
        usable.  Sources the library refuses (include/ndinterp.h lists them) raise `ValueError` with its message; a lane
        that is not monotone raises `BuilderError.Monotonic`."""
        h = C.c_void_p()
        st = _capi.lib().ndi_interp1d_inverse(self._h, C.byref(h))
        if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):
            raise ValueError(_capi.last_error())
        if st != _capi.OK:
            raise_builder(st)
        d = InverseStrategy()
        d._h, d._device, d._np_dtype, d._lanes, d._n = h, self._device, self._np_dtype, self._lanes, self._n
        d.origin = getattr(self, "origin", type(self))
        d.source = type(self)
        return d

    # -- evaluate -----------------------------------------------------------------------------
    _takes_fresh = True   # interp_array() may tell this strategy that the output buffer is its own (ndi_eval_flags)

    def interp_array_into(self, interpolator, xs_flat, out2d, *, async_launch=False, fresh=False,
                          rows_after_error_unspecified=False):
        """Replaces the reference's query loop (interp1d/mod.rs:326-343) by one C-ABI call.  `fresh`: the buffer was
        allocated for this call and is dropped on Err (Interp1D::interp_array, :197-211) -- NDI_EVAL_FRESH_OUTPUT."""
        qb = Buf(xs_flat, self._np_dtype)
        _check_out_dtype(out2d, self._np_dtype)
        opts = _capi.EvalOpts()
        opts.q_memspace = qb.memspace
        opts.path = self.path
        opts.async_launch = int(bool(async_launch))
        # rows_after_error_unspecified: a caller-owned buffer whose rows at / after a failing query the caller gives up
        # (NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED; the reference leaves them untouched, interp1d/mod.rs:334-342)
        opts.flags = (_capi.EVAL_FRESH_OUTPUT if fresh else _capi.EVAL_DEFAULT) | \
            (_capi.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED if rows_after_error_unspecified else 0)
        # an async batch reads the query array until finish(): keep every (possibly converted) copy alive
        if async_launch:
            self._inflight.append(qb)
        optr, stride = self._output(out2d, qb.memspace, opts)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp1d_eval(self._h, qb.ptr, qb.size, optr, stride, C.byref(opts), C.byref(info))
        if st != _capi.OK:
            raise_eval(st, info, int_query(self._np_dtype, [qb], info))

    def interp_lanewise_into(self, interpolator, xs2d, out2d, *, fresh=False, rows_after_error_unspecified=False):
        """`out2d[j, l] = f_l(xs2d[j, l])` (ndi_interp1d_eval_lanewise): a query per lane, `(Q, lanes)` in and out, host
        or device.  Errors name the flat element index `j * lanes + l`.  Element types the library refuses (integers,
        f16 / bf16) raise `ValueError` with its message."""
        qb = Buf(xs2d, self._np_dtype)
        _check_out_dtype(out2d, self._np_dtype)
        opts = _capi.EvalOpts()
        opts.q_memspace = qb.memspace
        opts.path = _capi.PATH_AUTO if self.path == _capi.PATH_BUCKETED else self.path
        opts.flags = (_capi.EVAL_FRESH_OUTPUT if fresh else _capi.EVAL_DEFAULT) | \
            (_capi.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED if rows_after_error_unspecified else 0)
        optr, stride = self._output(out2d, qb.memspace, opts)
        info = _capi.OobInfo()
        nq = qb.size // self._lanes
        st = _capi.lib().ndi_interp1d_eval_lanewise(self._h, qb.ptr, nq, self._lanes, optr, stride, C.byref(opts),
                                                    C.byref(info))
        if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):
            raise ValueError(_capi.last_error())
        if st != _capi.OK:
            raise_eval(st, info)

    def _output(self, out2d, q_memspace, opts):
        """(pointer, row stride in elements) of a 2-D output buffer; sets `opts.out_memspace` and, where device memory is
        involved, `opts.stream` to the current stream."""
        if is_torch(out2d):
            if not out2d.is_cuda:
                raise TypeError("torch output buffers must live on the device; use numpy for host buffers")
            opts.out_memspace = _capi.MEM_DEVICE
            optr = out2d.data_ptr()
            stride = out2d.stride(0) if out2d.dim() > 1 and out2d.shape[0] > 1 else self._lanes
            opts.stream = current_stream_ptr(self._device)
        else:
            opts.out_memspace = _capi.MEM_HOST
            optr = out2d.ctypes.data
            stride = out2d.strides[0] // out2d.itemsize if out2d.ndim > 1 and out2d.shape[0] > 1 else self._lanes
            if q_memspace == _capi.MEM_DEVICE:
                opts.stream = current_stream_ptr(self._device)
        return optr, max(stride, self._lanes)

    def finish(self):
        """Completes `async_launch` evaluations on the current stream and raises their error, if any."""
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp1d_finish(self._h, current_stream_ptr(self._device), C.byref(info))
        self._inflight.clear()
        if st != _capi.OK:
            raise_eval(st, info, int_query(self._np_dtype, None, info))

    def trim(self):
        """Frees the handle's idle scratch sets and a library-owned ring (ndi_interp1d_trim)."""
        _capi.lib().ndi_interp1d_trim(self._h)

    def interp_array_ring(self, xs_flat, chunk_queries, consumer=None, *, slots=None, n_slots=2):
        """Chunked evaluation through a device-output ring (ndi_interp1d_eval_ring): `interp_array` for batches
        whose whole output does not fit (or need not stay) in device memory.  `slots`: list of contiguous device
        tensors of shape (chunk_queries, lanes) -- the ring; None lets the library own `n_slots` buffers.
        `consumer(chunk, view)` is called once per chunk, in order, after the chunk's kernels are enqueued on the
        current stream; `view` is the slot tensor cut to the chunk's rows (None with a library-owned ring) and
        `chunk` the ndi_ring_chunk fields (index, q_begin, q_count, out, row_stride, slot, stream).  Work the
        consumer enqueues on the current stream is ordered before the slot's reuse; if it uses another stream it
        returns a `torch.cuda.Event` recorded there."""
        qb = Buf(xs_flat, self._np_dtype)
        ring = _capi.RingDesc()
        ring.chunk_queries = int(chunk_queries)
        keep_events = []
        if slots is not None:
            for t in slots:
                _check_out_dtype(t, self._np_dtype)
                if not (is_torch(t) and t.is_cuda and t.dim() == 2 and t.shape[1] == self._lanes
                        and t.shape[0] >= chunk_queries and (t.stride(1) == 1 or self._lanes == 1)
                        and t.stride(0) == slots[0].stride(0)):
                    raise TypeError("ring slots must be device tensors of shape (>= chunk_queries, lanes) with "
                                    "contiguous rows and one common row pitch (see striped_ring)")
            arr = (C.c_void_p * len(slots))(*[t.data_ptr() for t in slots])
            ring.slots = C.cast(arr, C.POINTER(C.c_void_p))
            ring.n_slots = len(slots)
            ring.row_stride = max(slots[0].stride(0), self._lanes)
        else:
            ring.n_slots = int(n_slots)
            ring.row_stride = self._lanes

        failed = []

        def _cb(_user, cptr):
            # an exception must not unwind through the C frames: remember the first one, stop consuming, re-raise
            # after the library call has returned
            if failed:
                return None
            try:
                c = cptr.contents
                view = slots[c.slot][:c.q_count] if slots is not None else None
                ev = consumer(c, view)
            except BaseException as e:  # noqa: BLE001
                failed.append(e)
                return None
            if ev is None:
                return None
            keep_events.append(ev)
            return ev.cuda_event
        cb = _capi.RING_CONSUMER(_cb) if consumer is not None else C.cast(None, _capi.RING_CONSUMER)
        opts = _capi.EvalOpts()
        opts.q_memspace = qb.memspace
        opts.out_memspace = _capi.MEM_DEVICE
        opts.path = self.path
        opts.stream = current_stream_ptr(self._device)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp1d_eval_ring(self._h, qb.ptr, qb.size, C.byref(ring), cb, None,
                                                C.byref(opts), C.byref(info))
        del keep_events
        if failed:
            raise failed[0]
        if st != _capi.OK:
            raise_eval(st, info, int_query(self._np_dtype, [qb], info))

    def interp_into(self, interpolator, target, x):
        # single query through the same device path (Q = 1)
        if is_bf16(self._np_dtype):   # bf16: torch tensors throughout (numpy has no bfloat16)
            import torch
            out = torch.empty((1, self._lanes), dtype=torch.bfloat16, device=f"cuda:{self._device}")
            self.interp_array_into(interpolator, _one_query(x), out)
            target[...] = out.reshape(target.shape)
            return
        out = np.empty((1, self._lanes), dtype=self._np_dtype)
        self.interp_array_into(interpolator, np.array([x], dtype=self._np_dtype), out)
        target[...] = out.reshape(target.shape)


def _check_out_dtype(out, dt):
    """The kernels write sizeof(data element) per output element: the buffer must have the data's element type
    (the reference enforces this at compile time)."""
    got = np_dtype_of(out)
    if got != np.dtype(dt):
        raise TypeError(f"output buffer has element type {got}, the interpolator's data is {np.dtype(dt)}")


def _default_device() -> int:
    import os
    return int(os.environ.get("LOCAL_RANK", "0")) if _capi.lib().ndi_device_count() > 1 else 0


def _to_device(a, device):
    import torch
    return a.to(device) if is_torch(a) else torch.as_tensor(np.asarray(a), device=device)


class Linear(Interp1DStrategyBuilder, _DeviceStrategy1D):
    """Linear Interpolation Strategy (src/interp1d/strategies/linear.rs)."""

    MINIMUM_DATA_LENGHT = 2  # linear.rs:52
    _kind = _capi.LINEAR

    def __init__(self):
        _DeviceStrategy1D.__init__(self)
        self._extrapolate = False
        self._device_req = None

    @staticmethod
    def new() -> "Linear":
        return Linear()

    def device(self, ordinal: int) -> "Linear":
        """Build-side option of this mirror (device selection): the HIP device that holds the tables.
        Default: the device of the data tensor, else LOCAL_RANK / device 0."""
        self._device_req = int(ordinal)
        return self

    def extrapolate(self, extrapolate: bool) -> "Linear":
        """does the strategy extrapolate? Default is `false` (linear.rs:23-26)"""
        self._extrapolate = bool(extrapolate)
        return self

    def build(self, x, data):
        dt = np_dtype_of(data)
        on_device = self._device_req is not None or (is_torch(data) and data.is_cuda)
        if (dt in DEVICE_INT_DTYPES or dt in DEVICE_HALF_DTYPES) and (on_device or is_bf16(dt)):
            # i32 / i64 / f16 on the device when asked for (.device(d) or a GPU tensor); plain host arrays keep the
            # generic path.  bf16 (torch.bfloat16 on either device) has no host path: it always takes the device
            return self._create(x, data, extrapolate=self._extrapolate, device=self._device_req)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            # integer (and other non-f32/f64) element types: the reference's generic per-query path
            from .generic_host import HostLinear
            return HostLinear(_host(x), _host(data), self._extrapolate)
        return self._create(x, data, extrapolate=self._extrapolate, device=self._device_req)

    def build_lane_axes(self, x, data):
        """`Interp1DBuilder.lane_axes`: `x` is the knot table of the data's shape.  Element types the library refuses
        (integers, f16 / bf16) raise `ValueError` with its message."""
        return self._create(x, data, extrapolate=self._extrapolate, device=self._device_req, lane_axes=True)


# ---- boundary conditions (cubic_spline.rs:153-217) ---------------------------------------------
class SingleBoundary:
    """Boundary condition for a single boundary (one side of one data row)."""

    def __init__(self, kind, value=0.0):
        self.kind, self.value = kind, float(value)

    def __eq__(self, o):
        return isinstance(o, SingleBoundary) and (self.kind, self.value) == (o.kind, o.value)

    @staticmethod
    def FirstDeriv(v):
        return SingleBoundary(_capi.BC_FIRST_DERIV, v)

    @staticmethod
    def SecondDeriv(v):
        return SingleBoundary(_capi.BC_SECOND_DERIV, v)


SingleBoundary.NotAKnot = SingleBoundary(_capi.BC_NOT_A_KNOT)
SingleBoundary.Natural = SingleBoundary(_capi.BC_NATURAL)
SingleBoundary.Clamped = SingleBoundary(_capi.BC_CLAMPED)


class RowBoundary:
    """Boundary condition for a single data row."""

    def __init__(self, left: SingleBoundary, right: SingleBoundary):
        self.left, self.right = left, right

    def __eq__(self, o):
        return isinstance(o, RowBoundary) and self.left == o.left and self.right == o.right

    @staticmethod
    def Mixed(left: SingleBoundary, right: SingleBoundary):
        return RowBoundary(left, right)


RowBoundary.NotAKnot = RowBoundary(SingleBoundary.NotAKnot, SingleBoundary.NotAKnot)
RowBoundary.Natural = RowBoundary(SingleBoundary.Natural, SingleBoundary.Natural)
RowBoundary.Clamped = RowBoundary(SingleBoundary.Clamped, SingleBoundary.Clamped)


class BoundaryCondition:
    """Boundary conditions for the whole dataset."""

    def __init__(self, tag, rows=None):
        self.tag, self.rows = tag, rows

    @staticmethod
    def Individual(rows):
        """Set individual boundary conditions for each row in the data: an array of `RowBoundary` of
        shape `[1, data.shape[1:]...]` (cubic_spline.rs:165-167, 332-340)."""
        return BoundaryCondition("Individual", np.asarray(rows, dtype=object))


BoundaryCondition.NotAKnot = BoundaryCondition("NotAKnot")
BoundaryCondition.Natural = BoundaryCondition("Natural")
BoundaryCondition.Clamped = BoundaryCondition("Clamped")
BoundaryCondition.Periodic = BoundaryCondition("Periodic")


class CubicSpline(Interp1DStrategyBuilder):
    """The CubicSpline 1d interpolation Strategy (Builder) -- cubic_spline.rs:85-88, 723-771."""

    MINIMUM_DATA_LENGHT = 3  # cubic_spline.rs:751

    def __init__(self):
        self._extrapolate = False
        self._boundary = BoundaryCondition.NotAKnot  # default, cubic_spline.rs:724-729
        self._device_req = None
        self._reference_order = False

    @staticmethod
    def new() -> "CubicSpline":
        return CubicSpline()

    def device(self, ordinal: int) -> "CubicSpline":
        """Build-side option of this mirror: the HIP device that holds the tables (see Linear.device)."""
        self._device_req = int(ordinal)
        return self

    def extrapolate(self, extrapolate: bool) -> "CubicSpline":
        self._extrapolate = bool(extrapolate)
        return self

    def reference_order(self, yes: bool = True) -> "CubicSpline":
        """Build-side option of this mirror (ndi_build_flags, NDI_BUILD_REFERENCE_ORDER): never re-associate the Thomas
        sweeps, so the a / b tables are bit-identical to CubicSpline::build's (cubic_spline.rs:678-721) for every shape.
        Default: narrow trailing axes on many knots (n >= 2048, lanes <= 256) take blocked sweeps that agree with the
        reference to a few ulp of the neighbouring entries (include/ndinterp.h states the bound)."""
        self._reference_order = bool(yes)
        return self

    def boundary(self, boundary: BoundaryCondition) -> "CubicSpline":
        self._boundary = boundary
        return self

    def build_lane_axes(self, x, data) -> "CubicSplineStrategy":
        """`Interp1DBuilder.lane_axes`: `x` is the knot table of the data's shape; the global non-periodic boundaries.
        Periodic and `Individual` raise `ValueError` with the library's message."""
        return self.build(x, data, lane_axes=True)

    def build(self, x, data, *, lane_axes=False) -> "CubicSplineStrategy":
        if np_dtype_of(data) not in (np.dtype(np.float32), np.dtype(np.float64)):
            # the reference's trait bounds (Pow / Euclid on T) keep the spline to float element types
            got = "bfloat16" if is_bf16(np_dtype_of(data)) else np_dtype_of(data)
            raise TypeError(f"CubicSpline covers float32/float64 only, got {got}")
        bc = self._boundary
        strat = CubicSplineStrategy()
        kw = dict(extrapolate=self._extrapolate, device=self._device_req,
                  build_flags=_capi.BUILD_REFERENCE_ORDER if self._reference_order else 0)
        if lane_axes:
            kw["lane_axes"] = True
        if bc.tag == "Periodic":
            kw["periodic"] = True
        elif bc.tag == "Individual":
            shape = tuple(data.shape)
            expect = (1,) + shape[1:]
            if tuple(bc.rows.shape) != expect:  # cubic_spline.rs:333-340
                raise BuilderError.ShapeError(
                    f"Boundary conditions array has wrong shape. Expected: {list(expect)}, got: {list(bc.rows.shape)}")
            rows = bc.rows.reshape(-1)
            kw["per_lane"] = ([r.left.kind for r in rows], [r.left.value for r in rows],
                              [r.right.kind for r in rows], [r.right.value for r in rows])
            if all(r == rows[0] for r in rows):  # identical rows are one global boundary
                kw.pop("per_lane")
                kw["left"] = (rows[0].left.kind, rows[0].left.value)
                kw["right"] = (rows[0].right.kind, rows[0].right.value)
        else:
            k = {"NotAKnot": _capi.BC_NOT_A_KNOT, "Natural": _capi.BC_NATURAL, "Clamped": _capi.BC_CLAMPED}[bc.tag]
            kw["left"] = kw["right"] = (k, 0.0)
        try:
            return strat._create(x, data, **kw)
        except BuilderError.ValueError as e:
            raise BuilderError.ValueError(_periodic_mismatch_message(data)) from e


def _rust_debug_row(row: np.ndarray) -> str:
    """`{:?}` of an ndarray row view, as ndarray 0.17 prints a small 1-D array."""
    from .errors import _rust_float
    body = ", ".join(_rust_float(float(v)) for v in row.reshape(-1))
    if row.ndim == 1:
        return f"[{body}], shape=[{row.shape[0]}], strides=[1], layout=CFcf (0xf), const ndim=1"
    return f"[{body}], shape={list(row.shape)}"


def _periodic_mismatch_message(data) -> str:
    """cubic_spline.rs:483-488 / 501-506: the two message forms of the periodic ValueError."""
    from .errors import _rust_float
    d = _host(data)
    head = "for periodic boundary condition the first and last value must be equal. "
    if d.ndim == 1:
        return head + f"First: {_rust_float(float(d[0]))}, last: {_rust_float(float(d[-1]))}"
    return head + f"First: {_rust_debug_row(d[0])}, last: {_rust_debug_row(d[-1])}"


class CubicSplineStrategy(_DeviceStrategy1D):
    """The CubicSpline 1d interpolation Strategy (Implementation) -- `a`, `b` live on the device
    (cubic_spline.rs:94-102)."""

    _kind = _capi.CUBIC_SPLINE

    def coefficients(self):
        """Copies the tables `a`, `b` (each `(n-1, lanes)`) to the host."""
        n = self._n
        a = np.empty((n - 1, self._lanes), dtype=self._np_dtype)
        b = np.empty_like(a)
        st = _capi.lib().ndi_interp1d_coefficients(self._h, a.ctypes.data, b.ctypes.data, _capi.MEM_HOST)
        if st != _capi.OK:
            raise_builder(st)
        return a, b

    def _create(self, x, data, **kw):
        self._n = data.shape[0]
        return super()._create(x, data, **kw)


# ---- local C1 cubics: Pchip, Akima, CubicHermite (include/ndinterp.h, ndi_strategy1d) -------------------------
class PchipStrategy(CubicSplineStrategy):
    """Finished `Pchip`: a / b tables on the device, evaluated by the spline's kernels."""

    _kind = _capi.PCHIP


class AkimaStrategy(CubicSplineStrategy):
    """Finished `Akima`."""

    _kind = _capi.AKIMA


class CubicHermiteStrategy(CubicSplineStrategy):
    """Finished `CubicHermite`."""

    _kind = _capi.CUBIC_HERMITE


class DerivativeStrategy(CubicSplineStrategy):
    """A derivative of a CubicSpline / Pchip / Akima / CubicHermite strategy (`strategy.derivative(nu)`,
    `Interp1D.derivative(nu)`): a handle of the cubic evaluation class whose tables were derived on the device.
    `order`: the derivative order counted from the interpolant (1 or 2); `origin`: the class of the strategy it started
    from; `coefficients()`: its a / b tables (equal to each other; zero for order 2)."""

    order = 0
    origin = None


class AntiderivativeStrategy(_DeviceStrategy1D):
    """The antiderivative of a Linear / CubicSpline / Pchip / Akima / CubicHermite strategy or of a derivative of one
    (`strategy.antiderivative()`, `Interp1D.antiderivative()`): a handle with a prefix table `P` (`data_table()`) and
    evaluation kernels of its own.  `interp_array_into`, `finish`, `clone`, `data_table`, `trim` and `release` are the
    shared ones; `integrate_into` is the definite integral.  `origin`: the class of the strategy it started from.  The
    ring, the sharded calls, `coefficients`, `derivative` and a second `antiderivative` are refused by the library;
    `inverse()` (a CDF's quantile function) is the shared one."""

    origin = None
    path = _capi.PATH_GATHER   # the one form these handles take (NDI_PATH_BUCKETED is refused, AUTO means this)

    def _refused(self, st):
        if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):
            raise ValueError(_capi.last_error())
        raise_builder(st)

    def derivative(self, nu: int = 1):
        h = C.c_void_p()
        self._refused(_capi.lib().ndi_interp1d_derivative(self._h, int(nu), C.byref(h)))

    def antiderivative(self):
        h = C.c_void_p()
        self._refused(_capi.lib().ndi_interp1d_antiderivative(self._h, C.byref(h)))

    def coefficients(self, device: bool = False):
        self._refused(_capi.lib().ndi_interp1d_coefficients(self._h, None, None, _capi.MEM_HOST))

    def integrate_into(self, lo_flat, hi_flat, out2d):
        """`out2d[j] = F(hi_flat[j]) - F(lo_flat[j])` (ndi_interp1d_integrate: both searches, both evaluations and the
        subtraction in one evaluation launch).  Both query arrays live in the same memory space; errors name the lowest
        failing flat index, `lo` before `hi`."""
        lb, hb = Buf(lo_flat, self._np_dtype), Buf(hi_flat, self._np_dtype)
        if lb.memspace != hb.memspace or lb.size != hb.size:
            raise TypeError("integrate_into: lo and hi must have the same length and live in the same memory space")
        _check_out_dtype(out2d, self._np_dtype)
        opts = _capi.EvalOpts()
        opts.q_memspace = lb.memspace
        opts.path = self.path
        optr, stride = self._output(out2d, lb.memspace, opts)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp1d_integrate(self._h, lb.ptr, hb.ptr, lb.size, optr, stride, C.byref(opts), C.byref(info))
        if st == _capi.OUT_OF_BOUNDS:   # both arrays are x coordinates: `axis` says which one (0: lo, 1: hi)
            from .errors import _rust_float
            raise InterpolateError.OutOfBounds(f"x = {_rust_float(info.value)} is not in range", index=int(info.index),
                                               value=float(info.value), axis=int(info.axis))
        if st != _capi.OK:
            raise_eval(st, info)


class InverseStrategy(_DeviceStrategy1D):
    """The inverse of a Linear / CubicSpline / Pchip / Akima / CubicHermite strategy, of a derivative of one, or of an
    antiderivative (`strategy.inverse()`, `Interp1D.inverse()`): queries are values `v`, rows are the abscissae `x` with
    `f_l(x) = v`, defined for `v` in the value range common to all lanes.  `interp_array_into`, `finish`, `clone`,
    `data_table` (the node table `N`), `trim` and `release` are the shared ones.  `origin`: the class of the strategy the
    chain started from; `source`: the class of the strategy that was inverted.  The ring, the sharded calls,
    `coefficients`, `derivative`, `antiderivative` and a second `inverse` are refused by the library."""

    origin = None
    source = None
    path = _capi.PATH_GATHER   # the one form these handles take (NDI_PATH_BUCKETED is refused, AUTO means this)

    def _refused(self, st):
        if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):
            raise ValueError(_capi.last_error())
        raise_builder(st)

    def derivative(self, nu: int = 1):
        h = C.c_void_p()
        self._refused(_capi.lib().ndi_interp1d_derivative(self._h, int(nu), C.byref(h)))

    def antiderivative(self):
        h = C.c_void_p()
        self._refused(_capi.lib().ndi_interp1d_antiderivative(self._h, C.byref(h)))

    def inverse(self):
        h = C.c_void_p()
        self._refused(_capi.lib().ndi_interp1d_inverse(self._h, C.byref(h)))

    def coefficients(self, device: bool = False):
        self._refused(_capi.lib().ndi_interp1d_coefficients(self._h, None, None, _capi.MEM_HOST))

    @staticmethod
    def _as_value_error(e):
        """the query of an inverse handle is a value `v`, not an `x`"""
        from .errors import _rust_float
        return InterpolateError.OutOfBounds(f"v = {_rust_float(e.value)} is not in range", index=e.index, value=e.value,
                                            axis=0)

    def interp_array_into(self, *args, **kw):
        try:
            super().interp_array_into(*args, **kw)
        except InterpolateError.OutOfBounds as e:
            raise self._as_value_error(e) from None

    def finish(self):
        try:
            super().finish()
        except InterpolateError.OutOfBounds as e:
            raise self._as_value_error(e) from None

    def interp_lanewise_into(self, *args, **kw):
        try:
            super().interp_lanewise_into(*args, **kw)
        except InterpolateError.OutOfBounds as e:
            raise self._as_value_error(e) from None


class _LocalCubic(Interp1DStrategyBuilder):
    """Shared builder body of Pchip / Akima / CubicHermite: `.extrapolate(b)` and `.device(d)` as `CubicSpline` has
    them (`extrapolate(True)` continues the first / last interval's polynomial); f32 / f64 only."""

    _finished = None

    def __init__(self):
        self._extrapolate = False
        self._device_req = None

    def device(self, ordinal: int):
        """Build-side option of this mirror: the HIP device that holds the tables (see Linear.device)."""
        self._device_req = int(ordinal)
        return self

    def extrapolate(self, extrapolate: bool):
        self._extrapolate = bool(extrapolate)
        return self

    def _check_dtype(self, data):
        if np_dtype_of(data) not in (np.dtype(np.float32), np.dtype(np.float64)):
            got = "bfloat16" if is_bf16(np_dtype_of(data)) else np_dtype_of(data)
            raise TypeError(f"{type(self).__name__} covers float32/float64 only, got {got}")

    def build(self, x, data):
        self._check_dtype(data)
        return self._finished()._create(x, data, extrapolate=self._extrapolate, device=self._device_req)

    def build_lane_axes(self, x, data):
        """`Interp1DBuilder.lane_axes`: `x` is the knot table of the data's shape."""
        self._check_dtype(data)
        return self._finished()._create(x, data, extrapolate=self._extrapolate, device=self._device_req, lane_axes=True)


class Pchip(_LocalCubic):
    """Piecewise cubic Hermite interpolating polynomial: Fritsch-Butland derivatives with the three-point
    shape-preserving end formula (what scipy's `PchipInterpolator` computes).  Monotone data gives a monotone
    interpolant: no overshoot on steps and plateaus.  Built on the device in one pass."""

    MINIMUM_DATA_LENGHT = 2
    _finished = PchipStrategy

    @staticmethod
    def new() -> "Pchip":
        return Pchip()


class Akima(_LocalCubic):
    """Akima's 1970 interpolant (scipy's `Akima1DInterpolator`, `method="akima"`): no ringing next to outliers.
    Where both weights vanish (`s == 0` exactly) the two neighbouring slopes are averaged; scipy switches to the
    average below a threshold relative to the largest `s` of the whole array."""

    MINIMUM_DATA_LENGHT = 3
    _finished = AkimaStrategy

    @staticmethod
    def new() -> "Akima":
        return Akima()


class CubicHermite(_LocalCubic):
    """Cubic Hermite interpolation with the caller's knot derivatives: `CubicHermite.new(dydx)`, `dydx` of the
    data's shape (a numpy array or a tensor)."""

    MINIMUM_DATA_LENGHT = 2
    _finished = CubicHermiteStrategy

    def __init__(self, dydx):
        super().__init__()
        self._dydx = dydx

    @staticmethod
    def new(dydx) -> "CubicHermite":
        return CubicHermite(dydx)

    def build(self, x, data, *, lane_axes=False):
        self._check_dtype(data)
        if tuple(self._dydx.shape) != tuple(data.shape):
            raise BuilderError.ShapeError(
                f"dydx has wrong shape. Expected: {list(data.shape)}, got: {list(self._dydx.shape)}")
        return self._finished()._create(x, data, extrapolate=self._extrapolate, device=self._device_req,
                                        dydx=self._dydx, **({"lane_axes": True} if lane_axes else {}))

    def build_lane_axes(self, x, data):
        return self.build(x, data, lane_axes=True)


# ------------------------------------------------------------------------------------------------
# Interp1D / Interp1DBuilder (src/interp1d/mod.rs)
# ------------------------------------------------------------------------------------------------
def _host(a) -> np.ndarray:
    if is_torch(a) and is_bf16(np_dtype_of(a)):   # numpy has no bfloat16: a host tensor instead
        return a.detach().cpu()
    return a.detach().cpu().numpy() if is_torch(a) else np.asarray(a)


def _zeros(shape, dt, device=None):
    """Array::zeros of the data's element type: numpy, or a torch.bfloat16 tensor for bf16 (on `device`, else the
    host)."""
    if is_bf16(dt):
        import torch
        return torch.zeros(shape, dtype=torch.bfloat16, device=device if device is not None else "cpu")
    return np.zeros(shape, dtype=dt)


def _one_query(v):
    """A single query for a bf16 strategy as a 1-element tensor; Python numbers stay exact (f64) until the one
    rounding to bf16 (_arrays.as_bf16_source)."""
    import torch
    return v.reshape(1) if is_torch(v) else torch.tensor([float(v)], dtype=torch.float64)


def _default_axis(n, dt):
    """0..n cast to T (interp1d/mod.rs:402-406)."""
    if is_bf16(dt):
        import torch
        return torch.arange(n).to(torch.bfloat16)
    return np.arange(n).astype(dt)


class Interp1D:
    """One dimensional interpolator (interp1d/mod.rs:39-51)."""

    def __init__(self, x, data, strategy, *, lane_axes=False):
        self.x, self.data, self.strategy = x, data, strategy
        self._x_host = _host(x)
        # an x axis per lane (Interp1DBuilder.lane_axes): `x` is the knot table of the data's shape, column l the knots of
        # lane l
        self._lane_axes = bool(lane_axes)

    # construction ---------------------------------------------------------------------------
    @staticmethod
    def builder(data) -> "Interp1DBuilder":
        return Interp1DBuilder.new(data)

    @staticmethod
    def new_unchecked(x, data, strategy) -> "Interp1D":
        """Create a interpolator without any data validation (interp1d/mod.rs:363-365)."""
        return Interp1D(x, data, strategy)

    # helpers the strategies use ------------------------------------------------------------------
    def index_point(self, index: int):
        if self._lane_axes:
            raise ValueError("index_point: this interpolator has lane axes (an x axis per lane): there is no one x per index")
        return self._x_host[index], self.data[index]

    def get_index_left_of(self, x) -> int:
        if self._lane_axes:
            raise ValueError("get_index_left_of: this interpolator has lane axes (an x axis per lane): every lane has its "
                             "own interval for x")
        k = self._x_host
        if k.dtype in (np.float32, np.float64):
            r = int(get_lower_index(np.ascontiguousarray(k), np.array([x], dtype=k.dtype))[0])
            if r < 0:
                raise Panic("not implemented: failed to convert NaN to usize")
            return r
        return int(np.clip(np.searchsorted(k, x, side="right") - 1, 0, k.size - 2))

    def is_in_range(self, x) -> bool:
        if self._lane_axes:   # the range common to all lanes: what interp / interp_array test
            return bool(self._x_host[0].max() <= x <= self._x_host[-1].min())
        return bool(self._x_host[0] <= x <= self._x_host[-1])

    # queries ----------------------------------------------------------------------------------
    def _lanes_shape(self):
        return tuple(self.data.shape[1:])

    def interp_scalar(self, x):
        """interp1d/mod.rs:108-114 (data must be 1-D)."""
        if len(self.data.shape) != 1:
            raise TypeError("interp_scalar needs 1-D data; use interp()")
        buf = _zeros((), np_dtype_of(self.data))
        self.strategy.interp_into(self, buf, x)
        return buf[()]

    def interp(self, x):
        """interp1d/mod.rs:150-156."""
        target = _zeros(self._lanes_shape(), np_dtype_of(self.data))
        self.strategy.interp_into(self, target, x)
        return target

    def interp_into(self, x, buffer):
        """interp1d/mod.rs:169-175; panics on a wrong buffer shape."""
        if tuple(buffer.shape) != self._lanes_shape():
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: "
                        f"{list(self._lanes_shape())}, got: {list(buffer.shape)}")
        self.strategy.interp_into(self, buffer, x)

    def get_buffer_shape(self, q_shape):
        """interp1d/mod.rs:346-354: query dims chained with data.shape[1..]."""
        return tuple(q_shape) + self._lanes_shape()

    def interp_array(self, xs):
        """interp1d/mod.rs:197-211.  numpy in -> numpy out; torch device tensor in -> device tensor out."""
        shape = self.get_buffer_shape(tuple(xs.shape))
        if is_torch(xs) and xs.is_cuda:
            import torch
            # element type of the *data* (the kernels write that; queries are converted to it)
            tdt = torch_dtype(np_dtype_of(self.data))
            if tdt is None:
                raise TypeError("device query tensors need f32 / f64 data; other element types use host arrays")
            nbytes = int(np.prod(shape, dtype=np.int64)) * np_dtype_of(self.data).itemsize
            if nbytes >= OUTPUT_OWNED_MIN_BYTES and not is_bf16(np_dtype_of(self.data)):
                # Array::zeros through the library's placement-checked allocator
                ys = output_empty(shape, np_dtype_of(self.data), xs.device.index or 0)
            else:
                ys = torch.empty(shape, dtype=tdt, device=xs.device)
            # the reference hands back zeros for rows it never reached only on Err, where the buffer
            # is dropped anyway (:210); no memset of the output is needed
        elif is_bf16(np_dtype_of(self.data)):
            # bf16 results are torch tensors: on the interpolator's device
            ys = _zeros(shape, np_dtype_of(self.data), f"cuda:{self.strategy._device}")
        else:
            ys = np.zeros(shape, dtype=np_dtype_of(self.data))
        # the buffer is this call's own and is dropped on Err (:210): strategies that can use the knowledge are told
        self.interp_array_into(xs, ys, **({"fresh": True} if getattr(self.strategy, "_takes_fresh", False) else {}))
        return ys

    def interp_array_into(self, xs, buffer, **kw):
        """interp1d/mod.rs:272-324.  Any query rank: a flatten of the query array and a 2-D view of
        the buffer (rows = queries, columns = lanes); panics when the buffer shape is wrong."""
        expect = self.get_buffer_shape(tuple(xs.shape))
        if tuple(buffer.shape) != expect:
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: {list(expect)}, "
                        f"got: {list(buffer.shape)}")
        if np_dtype_of(buffer) != np_dtype_of(self.data):
            raise TypeError(f"buffer has element type {np_dtype_of(buffer)}, the data is {np_dtype_of(self.data)}")
        nq = int(np.prod(xs.shape, dtype=np.int64))
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        xs_flat = xs.reshape(-1)
        if is_torch(buffer):
            if not buffer.is_contiguous():
                raise TypeError("device output buffers must be contiguous")
            out2d = buffer.view(nq, lanes)
            self.strategy.interp_array_into(self, xs_flat, out2d, **kw)
            return
        if buffer.flags.c_contiguous:
            self.strategy.interp_array_into(self, _host(xs_flat) if not is_torch(xs) else xs_flat,
                                            buffer.reshape(nq, lanes), **kw)
            return
        # strided ArrayViewMut: bounce through a contiguous temporary
        tmp = np.zeros((nq, lanes), dtype=np_dtype_of(self.data))
        done = nq
        try:
            self.strategy.interp_array_into(self, _host(xs_flat), tmp, **kw)
        except (InterpolateError.OutOfBounds, Panic) as e:
            done = e.index if getattr(e, "index", None) is not None else 0   # rows before the failing query are
            raise                                          # written, later rows stay untouched (interp1d/mod.rs:334-342)
        except BaseException:
            done = 0                                       # device failure: nothing in tmp can be trusted
            raise
        finally:
            if done and len(xs.shape) == 0:
                buffer[...] = tmp[0].reshape(buffer.shape)
            elif done:
                where = np.unravel_index(np.arange(done), tuple(xs.shape))     # works for any strides
                buffer[where] = tmp[:done].reshape((done,) + self._lanes_shape())

    def interp_lanewise(self, xs):
        """A query per lane: `xs.shape` ends with `data.shape[1:]` and `result[..., l] = f_l(xs[..., l])`, where
        `interp_array` evaluates every lane at one abscissa.  The result has `xs.shape` and the data's element type; numpy
        in -> numpy out, a device tensor in -> a tensor on its device.  On an inverse interpolator `xs` holds values, each
        tested against its own lane's range.  `InterpolateError.OutOfBounds.index` is the flat element index."""
        self._lanewise_check(xs)
        dt = np_dtype_of(self.data)
        if is_torch(xs) and xs.is_cuda:
            import torch
            ys = torch.empty(tuple(xs.shape), dtype=torch_dtype(dt), device=xs.device)
        else:
            ys = np.zeros(tuple(xs.shape), dtype=dt)
        self.interp_lanewise_into(xs, ys, fresh=True)
        return ys

    def interp_lanewise_into(self, xs, buffer, *, fresh=False, rows_after_error_unspecified=False):
        """`interp_lanewise` into a caller's buffer of `xs.shape`: rows (one per leading index) before the row of the
        first failing element are written, that row and all later ones stay untouched -- unless `fresh` or
        `rows_after_error_unspecified` give them up, which saves a pass over the queries."""
        self._lanewise_check(xs)
        if tuple(buffer.shape) != tuple(xs.shape):
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: {list(xs.shape)}, "
                        f"got: {list(buffer.shape)}")
        if np_dtype_of(buffer) != np_dtype_of(self.data):
            raise TypeError(f"buffer has element type {np_dtype_of(buffer)}, the data is {np_dtype_of(self.data)}")
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        nq = int(np.prod(xs.shape, dtype=np.int64)) // max(lanes, 1)
        kw = dict(fresh=fresh, rows_after_error_unspecified=rows_after_error_unspecified)
        if is_torch(buffer):
            if not buffer.is_contiguous():
                raise TypeError("device output buffers must be contiguous")
            self.strategy.interp_lanewise_into(self, xs.reshape(nq, lanes), buffer.view(nq, lanes), **kw)
            return
        if not buffer.flags.c_contiguous:
            raise TypeError("interp_lanewise_into needs a C-contiguous host buffer")
        self.strategy.interp_lanewise_into(self, xs.reshape(nq, lanes) if is_torch(xs) else _host(xs).reshape(nq, lanes),
                                           buffer.reshape(nq, lanes), **kw)

    def _lanewise_check(self, xs):
        if not isinstance(self.strategy, _DeviceStrategy1D):
            raise TypeError("interp_lanewise needs a built-in device strategy (Linear, CubicSpline, Pchip, Akima or "
                            "CubicHermite on f32 / f64 data, a derivative, an antiderivative or an inverse), got "
                            f"{type(self.strategy).__name__}")
        lanes_shape = self._lanes_shape()
        k = len(lanes_shape)
        if len(xs.shape) < k or tuple(xs.shape)[len(xs.shape) - k:] != lanes_shape:
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: [.., "
                        f"{', '.join(str(d) for d in lanes_shape)}], got: {list(xs.shape)}")

    def replicate(self, devices):
        """Replicas of this interpolator on the given devices (tables copied device to device, nothing rebuilt):
        what `sharding.interp_array_sharded` takes.  `interp.replicate(range(pkg.device_count()))`."""
        if not hasattr(self.strategy, "clone"):
            raise TypeError("replicate needs a built-in device strategy (f32 / f64 data)")
        return [Interp1D(self.x, self.data, self.strategy.clone(d), lane_axes=self._lane_axes) for d in devices]

    def derivative(self, nu: int = 1) -> "Interp1D":
        """The `nu`-th derivative of this interpolator as an interpolator of its own (scipy's
        `CubicSpline.derivative(nu)`): same `x`, `data` = the derivative at the knots in this data's shape (a host array
        for host-built interpolators, a tensor on the strategy's device for device-built ones), strategy a
        `DerivativeStrategy`.  CubicSpline: `nu` 1 or 2; Pchip / Akima / CubicHermite: 1; orders add up over repeated
        calls.  Everything else is a `ValueError` with the library's reason; strategies that are not the built-in device
        ones (user strategies, the generic host path) raise `TypeError`."""
        if not isinstance(self.strategy, _DeviceStrategy1D):
            raise TypeError("derivative needs a built-in device strategy (CubicSpline, Pchip, Akima or CubicHermite on "
                            f"f32 / f64 data), got {type(self.strategy).__name__}")
        strat = self.strategy.derivative(nu)
        on_device = is_torch(self.data) and self.data.is_cuda
        return Interp1D(self.x, strat.data_table(device=on_device).reshape(tuple(self.data.shape)), strat)

    def antiderivative(self) -> "Interp1D":
        """The antiderivative of this interpolator as an interpolator of its own (scipy's `.antiderivative()`, with
        `F(x[0]) = 0`): same `x`, `data` = the prefix table `P` in this data's shape (a host array for host-built
        interpolators, a tensor on the strategy's device for device-built ones), strategy an `AntiderivativeStrategy`;
        `interp`, `interp_array` and `interp_array_into` work on it unchanged.  Sources the library refuses (integer and
        half element types, the periodic mode, an antiderivative) are a `ValueError` with its reason; strategies that are
        not the built-in device ones raise `TypeError`."""
        if not isinstance(self.strategy, _DeviceStrategy1D):
            raise TypeError("antiderivative needs a built-in device strategy (Linear, CubicSpline, Pchip, Akima or "
                            f"CubicHermite on f32 / f64 data), got {type(self.strategy).__name__}")
        strat = self.strategy.antiderivative()
        on_device = is_torch(self.data) and self.data.is_cuda
        return Interp1D(self.x, strat.data_table(device=on_device).reshape(tuple(self.data.shape)), strat)

    def inverse(self) -> "Interp1D":
        """The inverse of this interpolator as an interpolator of its own (scipy's `PPoly.solve`, one root per lane and
        batched): `inv.interp_array(vs)[j, l]` is the `x` with `f_l(x) = vs[j]`, of shape `vs.shape ++ data.shape[1:]`.
        Same `x`, `data` = the node table (this data; the prefix table for an antiderivative), strategy an
        `InverseStrategy`.  Every lane must be monotone (ties allowed), else `BuilderError.Monotonic`; a value outside
        the range common to all lanes is `InterpolateError.OutOfBounds`, whatever `extrapolate` was.  Sources the library
        refuses (integer and half element types, the periodic mode, an inverse) are a `ValueError` with its reason;
        strategies that are not the built-in device ones raise `TypeError`."""
        if not isinstance(self.strategy, _DeviceStrategy1D):
            raise TypeError("inverse needs a built-in device strategy (Linear, CubicSpline, Pchip, Akima or CubicHermite "
                            f"on f32 / f64 data, a derivative or an antiderivative), got {type(self.strategy).__name__}")
        strat = self.strategy.inverse()
        on_device = is_torch(self.data) and self.data.is_cuda
        return Interp1D(self.x, strat.data_table(device=on_device).reshape(tuple(self.data.shape)), strat)

    def integrate(self, lo, hi):
        """Definite integrals (scipy's `.integrate(a, b)`, batched): `lo`, `hi` arrays of equal shape, host or device;
        the result has the shape `lo.shape ++ data.shape[1:]` and lives where the queries live.  `lo > hi` gives the
        negated integral.  On an interpolator that is no antiderivative, its antiderivative is built once, kept on the
        instance and used."""
        lo, hi = (v if is_torch(v) else np.asarray(v) for v in (lo, hi))      # (lists and scalars too)
        if tuple(lo.shape) != tuple(hi.shape):
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes lo: {list(lo.shape)}, hi: {list(hi.shape)}")
        if not isinstance(self.strategy, AntiderivativeStrategy):
            if getattr(self, "_antiderivative", None) is None:
                self._antiderivative = self.antiderivative()
            return self._antiderivative.integrate(lo, hi)
        shape = self.get_buffer_shape(tuple(lo.shape))
        dt = np_dtype_of(self.data)
        nq = int(np.prod(lo.shape, dtype=np.int64))
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        if is_torch(lo) != is_torch(hi) or (is_torch(lo) and lo.is_cuda != hi.is_cuda):
            raise TypeError("integrate: lo and hi must live in the same memory space")
        if is_torch(lo) and lo.is_cuda:
            import torch
            out = torch.empty(shape, dtype=torch_dtype(dt), device=lo.device)
            self.strategy.integrate_into(lo.reshape(-1), hi.reshape(-1), out.view(nq, lanes))
            return out
        out = np.zeros(shape, dtype=dt)
        self.strategy.integrate_into(_host(lo).reshape(-1), _host(hi).reshape(-1), out.reshape(nq, lanes))
        return out

    def interp_array_ring(self, xs, chunk_queries, consumer=None, *, slots=None, n_slots=2):
        """`interp_array` (interp1d/mod.rs:197-211) for outputs larger than device memory: the flattened
        queries are evaluated `chunk_queries` rows at a time into a ring of device buffers and handed to
        `consumer(chunk, rows)`; see `_DeviceStrategy1D.interp_array_ring` / ndi_interp1d_eval_ring."""
        if not hasattr(self.strategy, "interp_array_ring"):
            raise TypeError("the ring evaluation needs a built-in device strategy (f32 / f64 data)")
        self.strategy.interp_array_ring(xs.reshape(-1), chunk_queries, consumer, slots=slots, n_slots=n_slots)


class Interp1DBuilder:
    """Create and configure a `Interp1D` interpolator (interp1d/mod.rs:60-70, 389-477)."""

    def __init__(self, data, x=None, strategy=None, lane_x=None):
        self._data = data
        self._x = x
        self._lane_x = lane_x
        self._strategy = strategy if strategy is not None else Linear.new()  # :408

    @staticmethod
    def new(data) -> "Interp1DBuilder":
        return Interp1DBuilder(data)

    def x(self, x) -> "Interp1DBuilder":
        return Interp1DBuilder(self._data, x, self._strategy, self._lane_x)

    def lane_axes(self, x) -> "Interp1DBuilder":
        """An x axis PER LANE (this mirror's own; ndi_interp1d_create_lane_axes): `x` has the data's shape, element type
        and residence (host array or device tensor), and `x[:, l...]` holds the knots of lane `l...`, each column strictly
        rising.  Lane `l` of the interpolator is the interpolant of `(x[:, l], data[:, l])` alone: `np.interp` per row
        with `xp`, `fp` and the queries all batched.  Works with Linear, CubicSpline (the global non-periodic
        boundaries), Pchip, Akima and CubicHermite on f32 / f64 data; `.x(...)` cannot be given as well."""
        return Interp1DBuilder(self._data, self._x, self._strategy, x)

    def strategy(self, strategy) -> "Interp1DBuilder":
        return Interp1DBuilder(self._data, self._x, strategy, self._lane_x)

    def _build_lane_axes(self) -> Interp1D:
        """`build()` with `lane_axes(x)`: the reference's check order (interp1d/mod.rs:449-471) with a column per lane."""
        data, strategy, x = self._data, self._strategy, self._lane_x
        if self._x is not None:
            raise BuilderError.ValueError("both x and lane_axes were given: an interpolator has one shared x axis or an x "
                                          "axis per lane")
        n = tuple(data.shape)[0]
        need = type(strategy).MINIMUM_DATA_LENGHT
        if n < need:
            raise BuilderError.NotEnoughData(
                f"The chosen Interpolation strategy needs at least {need} data points")
        on_device = is_torch(x) and x.is_cuda
        if not on_device and len(tuple(x.shape)) >= 1:   # (device tensors: the library's kernel pass checks the columns)
            cols = _host(x)
            if is_torch(cols):   # (a host bf16 tensor: its f32 image orders the same way)
                cols = cols.float().numpy()
            cols = cols.reshape(tuple(x.shape)[0], -1)
            rising = (cols[1:] > cols[:-1]).all(axis=0) if cols.shape[0] > 1 else np.zeros(cols.shape[1], bool)
            if not rising.all():
                raise BuilderError.Monotonic("Values in the x axis need to be strictly monotonic rising "
                                             f"(lane {int(np.argmin(rising))})")
        if tuple(x.shape) != tuple(data.shape):
            raise BuilderError.ShapeError(
                f"Shapes of the lane axes and the data need to match. Got x: {list(x.shape)}, data: {list(data.shape)}")
        if np_dtype_of(x) != np_dtype_of(data):
            raise TypeError(f"lane_axes has element type {np_dtype_of(x)}, the data is {np_dtype_of(data)}")
        if on_device != (is_torch(data) and data.is_cuda):
            raise TypeError("lane_axes and data must live in the same memory space (both host arrays or both device tensors)")
        if not hasattr(strategy, "build_lane_axes"):
            raise TypeError("lane_axes needs a built-in strategy (Linear, CubicSpline, Pchip, Akima or CubicHermite), got "
                            f"{type(strategy).__name__}")
        return Interp1D(x, data, strategy.build_lane_axes(x, data), lane_axes=True)

    def build(self) -> Interp1D:
        """Validate input data and create the configured `Interp1D` (interp1d/mod.rs:443-476)."""
        data, strategy = self._data, self._strategy
        shape = tuple(data.shape)
        if len(shape) < 1:
            raise BuilderError.ShapeError("data dimension is 0, needs to be at least 1")
        if self._lane_x is not None:
            return self._build_lane_axes()
        n = shape[0]
        dt = np_dtype_of(data)
        if self._x is None:  # default axis 0..len cast to T (:402-406)
            x = _default_axis(n, dt)
        else:
            x = self._x
        need = type(strategy).MINIMUM_DATA_LENGHT
        if n < need:
            raise BuilderError.NotEnoughData(
                f"The chosen Interpolation strategy needs at least {need} data points")
        if monotonic_prop(x) != Monotonic.Rising(True):
            raise BuilderError.Monotonic("Values in the x axis need to be strictly monotonic rising")
        x_len = int(np.prod(x.shape, dtype=np.int64))
        if x_len != n:
            raise BuilderError.ShapeError(
                f"Lengths of x and data axis need to match. Got x: {x_len}, data: {n}")
        finished = strategy.build(x, data)
        return Interp1D(x, data, finished)
