"""Host-side mirror of the reference's 2-D surface (src/interp2d/mod.rs + strategies/):
`Interp2DBuilder`, `Interp2D`, the strategy trait pair and the built-in `Bilinear`; plus `Bicubic`, which the
reference does not have."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._arrays import (DEVICE_HALF_DTYPES, DEVICE_INT_DTYPES, OUTPUT_OWNED_MIN_BYTES, Buf, current_stream_ptr, dtype_id,
                      int_query, is_bf16, is_torch, np_dtype_of, output_empty, torch_dtype)
from .errors import BuilderError, InterpolateError, Panic, raise_builder, raise_eval
from .interp1d import (BoundaryCondition, RowBoundary, _check_out_dtype, _default_axis, _default_device, _host, _one_query,
                       _to_device, _zeros)
from .vector_extensions import Monotonic, get_lower_index, monotonic_prop

# The parts of a jet (ndi_interp2d_eval_jet) in their fixed order, as (nu_x, nu_y): order 1 is the value and the gradient,
# order 2 adds the three second derivatives.
JET_PARTS = {1: ((0, 0), (1, 0), (0, 1)),
             2: ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))}


class Interp2DStrategyBuilder:
    """Trait `Interp2DStrategyBuilder` (src/interp2d/strategies/mod.rs:14-44)."""

    MINIMUM_DATA_LENGHT = 2

    def build(self, x, y, data) -> "Interp2DStrategy":
        raise NotImplementedError


class Interp2DStrategy:
    """Trait `Interp2DStrategy` (src/interp2d/strategies/mod.rs:46-73): per-query
    `interp_into(interpolator, target, x, y)`; `interp_array_into` is the defaulted batched hook whose
    default body is the reference's serial loop (interp2d/mod.rs:287-307)."""

    def interp_into(self, interpolator, target, x, y) -> None:
        raise NotImplementedError

    def interp_array_into(self, interpolator, xs_flat, ys_flat, out2d) -> None:
        shape = tuple(interpolator.data.shape[2:])
        for i in range(len(xs_flat)):
            self.interp_into(interpolator, out2d[i].reshape(shape), xs_flat[i], ys_flat[i])

    def release(self) -> None:
        pass


class _DeviceStrategy2D(Interp2DStrategy):
    """What the built-in device strategies share: one `ndi_interp2d` handle and every evaluation entry point on it
    (Bilinear and Bicubic differ in how the handle is created)."""

    path = _capi.PATH_AUTO   # evaluation formulation (ndi_path)

    def __init__(self):
        self._extrapolate = False
        self._h = None
        self._device = 0
        self._device_req = None
        self._np_dtype = None
        self._lanes = 1
        self._inflight = []

    def device(self, ordinal: int):
        """Build-side option of this mirror: the HIP device that holds the grid (default: the data tensor's
        device, else LOCAL_RANK / device 0)."""
        self._device_req = int(ordinal)
        return self

    def extrapolate(self, yes: bool):
        self._extrapolate = bool(yes)
        return self

    def _create(self, x, y, data, device, create):
        """Fill an ndi_interp2d_desc from the arrays and call `create(desc, out_handle)` -> ndi_status."""
        dt = np_dtype_of(data)
        tid = dtype_id(dt)
        db = Buf(data)

        def axis(a):
            if a is None:
                return None
            if db.memspace == _capi.MEM_HOST:
                return Buf(_host(a), dt)
            return Buf(_to_device(a, db.keep.device), dt)

        xb, yb = axis(x), axis(y)
        if device is None:
            device = self._device_req
        if device is None:
            device = db.device if db.memspace == _capi.MEM_DEVICE else _default_device()
        nx, ny = db.shape[0], db.shape[1]
        lanes = int(np.prod(db.shape[2:], dtype=np.int64)) if len(db.shape) > 2 else 1
        d = _capi.Interp2DDesc()
        d.dtype, d.extrapolate, d.device, d.memspace = tid, int(self._extrapolate), device, db.memspace
        d.nx, d.ny, d.lanes = nx, ny, lanes
        d.x_len = xb.size if xb is not None else nx
        d.y_len = yb.size if yb is not None else ny
        d.x = xb.ptr if xb is not None else None
        d.y = yb.ptr if yb is not None else None
        d.data = db.ptr
        d.validate = 0  # Interp2DBuilder.build() validated already (interp2d/mod.rs:477-511)
        h = C.c_void_p()
        st = create(d, h)
        if st != _capi.OK:
            raise_builder(st)
        self._h, self._device, self._np_dtype, self._lanes = h, device, dt, lanes
        self._shape = (nx, ny) + tuple(db.shape[2:])
        return self

    def release(self):
        if self._h is not None:
            _capi.lib().ndi_interp2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def clone(self, device: int):
        """A replica of this built strategy on `device` (ndi_interp2d_clone): the grid is copied device to device."""
        import copy
        h = C.c_void_p()
        st = _capi.lib().ndi_interp2d_clone(self._h, int(device), C.byref(h))
        if st != _capi.OK:
            raise_builder(st)
        other = copy.copy(self)
        other._h, other._device, other._inflight = h, int(device), []
        return other

    _takes_fresh = True   # see _DeviceStrategy1D

    def interp_array_into(self, interpolator, xs_flat, ys_flat, out2d, *, async_launch=False, fresh=False,
                          rows_after_error_unspecified=False):
        """Replaces the reference's query loop (interp2d/mod.rs:287-307) by one C-ABI call.  `fresh`: the buffer was
        allocated for this call and is dropped on Err (Interp2D::interp_array, :175-196) -- NDI_EVAL_FRESH_OUTPUT."""
        qx = Buf(xs_flat, self._np_dtype)
        qy = Buf(ys_flat, self._np_dtype)
        if qx.memspace != qy.memspace:
            raise TypeError("xs and ys must live in the same memory space")
        _check_out_dtype(out2d, self._np_dtype)
        if async_launch:                      # every async batch reads its query arrays until finish():
            self._inflight.append((qx, qy))   # keep all (possibly converted) copies alive, not only the last
        opts = _capi.EvalOpts()
        opts.q_memspace = qx.memspace
        opts.path = self.path
        opts.async_launch = int(bool(async_launch))
        # rows_after_error_unspecified: a caller-owned buffer whose rows at / after a failing query the caller gives up
        # (NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED; the reference leaves them untouched, interp1d/mod.rs:334-342)
        opts.flags = (_capi.EVAL_FRESH_OUTPUT if fresh else _capi.EVAL_DEFAULT) | \
            (_capi.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED if rows_after_error_unspecified else 0)
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
            if qx.memspace == _capi.MEM_DEVICE:
                opts.stream = current_stream_ptr(self._device)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp2d_eval(self._h, qx.ptr, qy.ptr, qx.size, optr, max(stride, self._lanes),
                                           C.byref(opts), C.byref(info))
        if st != _capi.OK:
            raise_eval(st, info, int_query(self._np_dtype, [qx, qy], info))

    def interp_lanewise_into(self, interpolator, xs2d, ys2d, out2d, *, fresh=False, rows_after_error_unspecified=False):
        """`out2d[j, l] = f_l(xs2d[j, l], ys2d[j, l])` (ndi_interp2d_eval_lanewise): an (x, y) per lane, `(Q, lanes)` in and
        out, host or device.  Errors name the flat element index `j * lanes + l` and the axis.  Handles the library refuses
        (integral handles, integers, f16 / bf16) raise `ValueError` with its message."""
        qx = Buf(xs2d, self._np_dtype)
        qy = Buf(ys2d, self._np_dtype)
        if qx.memspace != qy.memspace:
            raise TypeError("xs and ys must live in the same memory space")
        _check_out_dtype(out2d, self._np_dtype)
        opts = _capi.EvalOpts()
        opts.q_memspace = qx.memspace
        opts.path = _capi.PATH_AUTO if self.path == _capi.PATH_BUCKETED else self.path
        opts.flags = (_capi.EVAL_FRESH_OUTPUT if fresh else _capi.EVAL_DEFAULT) | \
            (_capi.EVAL_ROWS_AFTER_ERROR_UNSPECIFIED if rows_after_error_unspecified else 0)
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
            if qx.memspace == _capi.MEM_DEVICE:
                opts.stream = current_stream_ptr(self._device)
        info = _capi.OobInfo()
        nq = qx.size // self._lanes
        st = _capi.lib().ndi_interp2d_eval_lanewise(self._h, qx.ptr, qy.ptr, nq, self._lanes, optr, max(stride, self._lanes),
                                                    C.byref(opts), C.byref(info))
        if st in (_capi.BAD_ARG, _capi.UNSUPPORTED):
            raise ValueError(_capi.last_error())
        if st != _capi.OK:
            raise_eval(st, info)

    def finish(self):
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp2d_finish(self._h, current_stream_ptr(self._device), C.byref(info))
        self._inflight.clear()
        if st != _capi.OK:
            raise_eval(st, info, int_query(self._np_dtype, None, info))

    def trim(self):
        _capi.lib().ndi_interp2d_trim(self._h)

    def interp_array_ring(self, xs_flat, ys_flat, chunk_queries, consumer=None, *, slots=None, n_slots=2):
        """ndi_interp2d_eval_ring; see `_DeviceStrategy1D.interp_array_ring`."""
        qx, qy = Buf(xs_flat, self._np_dtype), Buf(ys_flat, self._np_dtype)
        if qx.memspace != qy.memspace:
            raise TypeError("xs and ys must live in the same memory space")
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
        opts.q_memspace = qx.memspace
        opts.out_memspace = _capi.MEM_DEVICE
        opts.path = self.path
        opts.stream = current_stream_ptr(self._device)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp2d_eval_ring(self._h, qx.ptr, qy.ptr, qx.size, C.byref(ring), cb, None,
                                                C.byref(opts), C.byref(info))
        del keep_events
        if failed:
            raise failed[0]
        if st != _capi.OK:
            raise_eval(st, info, int_query(self._np_dtype, [qx, qy], info))

    def interp_into(self, interpolator, target, x, y):
        if is_bf16(self._np_dtype):   # bf16: torch tensors throughout (numpy has no bfloat16)
            import torch
            out = torch.empty((1, self._lanes), dtype=torch.bfloat16, device=f"cuda:{self._device}")
            self.interp_array_into(interpolator, _one_query(x), _one_query(y), out)
            target[...] = out.reshape(target.shape)
            return
        out = np.empty((1, self._lanes), dtype=self._np_dtype)
        self.interp_array_into(interpolator, np.array([x], dtype=self._np_dtype),
                               np.array([y], dtype=self._np_dtype), out)
        target[...] = out.reshape(target.shape)


class Bilinear(Interp2DStrategyBuilder, _DeviceStrategy2D):
    """Bilinear strategy (src/interp2d/strategies/bilinear.rs); builder and finished strategy in one,
    as in the reference (`type FinishedStrat = Self`, :43).  `path`: BUCKETED = tile-grouped query order."""

    MINIMUM_DATA_LENGHT = 2  # bilinear.rs:41

    @staticmethod
    def new() -> "Bilinear":
        return Bilinear()

    def build(self, x, y, data, device=None):
        dt = np_dtype_of(data)
        on_device = device is not None or self._device_req is not None or (is_torch(data) and data.is_cuda)
        device_t = (dt in DEVICE_INT_DTYPES or dt in DEVICE_HALF_DTYPES) and (on_device or is_bf16(dt))
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)) and not device_t:
            # i32 / i64 / f16 take the device when asked for (.device(d) or a GPU tensor); plain host arrays stay here
            # (bf16 always takes the device: it has no host path)
            # integer (and other non-f32/f64) element types: the reference's generic per-query path
            from .generic_host import HostBilinear
            return HostBilinear(_host(x), _host(y), _host(data), self._extrapolate)
        return self._create(x, y, data, device,
                            lambda d, h: _capi.lib().ndi_interp2d_create(C.byref(d), C.byref(h)))

    def partial(self, nu_x=0, nu_y=0):
        raise TypeError("Bilinear has no partial derivatives: its slope jumps at every grid line and it keeps no node "
                        "derivatives (Bicubic.partial gives them)")

    def antiderivative(self):
        raise TypeError("Bilinear has no antiderivative handle: 2-D integrals are Bicubic's (Bicubic.antiderivative)")

    def integral(self, *a, **kw):
        raise TypeError("Bilinear has no rectangle integral: 2-D integrals are Bicubic's (Bicubic.antiderivative, then "
                        "integral)")

    def jet_into(self, *a, **kw):
        raise TypeError("Bilinear has no value-and-gradient (jet) evaluation: its slope jumps at every grid line and it "
                        "keeps no node derivatives (Bicubic.jet_into gives the value and the partials in one call)")

    def probe_ceiling(self, out2d, reps=5) -> float:
        """ms of the evaluation kernel's memory access mix alone on this handle's grid (ndi_interp2d_probe_ceiling);
        `out2d`: a device tensor (nq, lanes) that is overwritten."""
        ms = C.c_double()
        st = _capi.lib().ndi_interp2d_probe_ceiling(self._h, out2d.shape[0], out2d.data_ptr(), out2d.stride(0),
                                                    current_stream_ptr(self._device), int(reps), C.byref(ms))
        if st != _capi.OK:
            from .errors import DeviceError
            raise DeviceError(_capi.last_error())
        return ms.value


class Bicubic(Interp2DStrategyBuilder, _DeviceStrategy2D):
    """Bicubic strategy: the tensor-product cubic spline on the grid (scipy: RectBivariateSpline(kx=3, ky=3, s=0) for the
    default ends, on evenly and unevenly spaced axes alike: its not-a-knot right end is the true not-a-knot row, where a
    1-D CubicSpline keeps the reference's), built and evaluated on the device (ndi_interp2d_create_bicubic;
    include/ndinterp.h states the numerical contract).  The reference has no such strategy.  Builder and finished strategy in one, like `Bilinear`.
    `Bicubic.pchip()`, `Bicubic.akima()` and `Bicubic.hermite(zx, zy, zxy)` build the same strategy with the node derivatives of a
    local rule or of the caller instead of the spline's: `partial`, `antiderivative`, `integral`, `jet_into` and the rest
    are shared."""

    MINIMUM_DATA_LENGHT = 3

    # where the node derivatives come from: None -- the spline (`new()`); "pchip" / "akima" -- the 1-D rule of that name along
    # each axis (`pchip()`, `akima()`: ndi_interp2d_create_bicubic_local); "hermite" -- the caller (`hermite(zx, zy, zxy)`:
    # ndi_interp2d_create_bicubic_hermite).  Everything after the build is the same strategy.
    rule = None

    def __init__(self):
        super().__init__()
        self._bc_x = self._bc_y = RowBoundary.NotAKnot
        self._given = None
        self._periodic = 0      # bit 0: x, bit 1: y (ndi_interp2d_create_bicubic_periodic)

    @staticmethod
    def new() -> "Bicubic":
        return Bicubic()

    @staticmethod
    def _local(rule, minimum) -> "Bicubic":
        b = Bicubic()
        b.rule, b.MINIMUM_DATA_LENGHT = rule, minimum
        return b

    @staticmethod
    def pchip() -> "Bicubic":
        """Node derivatives by the 1-D Pchip rule along each axis (scipy / MATLAB: `pchip`; at least 2 points per axis).  On
        every grid line the surface is the 1-D Pchip interpolant of that line, so it does not overshoot ALONG grid lines;
        inside a cell monotonicity is not promised.  C1: second partials jump at the grid lines."""
        return Bicubic._local("pchip", 2)

    @staticmethod
    def akima() -> "Bicubic":
        """Node derivatives by the 1-D Akima rule along each axis (at least 3 points per axis): local, an outlier moves the
        derivatives of its neighbours only.  C1: second partials jump at the grid lines."""
        return Bicubic._local("akima", 3)

    @staticmethod
    def hermite(zx, zy, zxy) -> "Bicubic":
        """The caller's node derivatives d/dx, d/dy and d2/dxdy, each of the data's shape and dtype (numpy arrays or
        tensors; `tables()` of another Bicubic strategy gives such arrays).  No rule is applied; at least 2 points per
        axis."""
        b = Bicubic._local("hermite", 2)
        b._given = (zx, zy, zxy)
        return b

    def _no_ends(self):
        if self.rule is not None:
            raise TypeError(f"Bicubic.{self.rule}() takes no boundary conditions: ends are a spline notion "
                            "(the rule needs none; Bicubic.new() builds the spline)")

    @staticmethod
    def _ends(bc) -> RowBoundary:
        """One axis' (left, right) pair from a BoundaryCondition (NotAKnot / Natural / Clamped) or a RowBoundary."""
        if isinstance(bc, RowBoundary):
            return bc
        if isinstance(bc, BoundaryCondition) and bc.tag in ("NotAKnot", "Natural", "Clamped"):
            return getattr(RowBoundary, bc.tag)
        if isinstance(bc, BoundaryCondition) and bc.tag == "Periodic":
            raise TypeError("Bicubic has no periodic ends: its boundaries are one non-periodic kind per end; a periodic "
                            "axis is Bicubic.new().periodic_x() / .periodic_y() (both: .periodic())")
        if isinstance(bc, BoundaryCondition) and bc.tag == "Individual":
            raise TypeError("Bicubic takes no per-lane (Individual) boundaries: one kind and scalar value per end "
                            "(RowBoundary.Mixed(left, right) gives an axis two different ends)")
        raise TypeError(f"Bicubic boundaries are BoundaryCondition or RowBoundary objects, got {type(bc).__name__}")

    def boundary(self, bc) -> "Bicubic":
        """The same ends on both axes."""
        self._no_ends()
        self._bc_x = self._bc_y = self._ends(bc)
        return self

    def boundary_x(self, bc) -> "Bicubic":
        self._no_ends()
        self._bc_x = self._ends(bc)
        return self

    def boundary_y(self, bc) -> "Bicubic":
        self._no_ends()
        self._bc_y = self._ends(bc)
        return self

    def periodic_x(self) -> "Bicubic":
        """The x axis is periodic with period x[-1] - x[0]: the build closes the spline along x on itself (the first and
        the last data row must be equal, exactly), and with `extrapolate(True)` an x outside the range is wrapped into it
        instead of continuing the end patch.  The axis takes no boundary condition."""
        self._no_ends()
        self._periodic |= 1
        return self

    def periodic_y(self) -> "Bicubic":
        """`periodic_x` for the y axis."""
        self._no_ends()
        self._periodic |= 2
        return self

    def periodic(self) -> "Bicubic":
        """Both axes periodic: a torus."""
        return self.periodic_x().periodic_y()

    @property
    def wraps(self) -> int:
        """The axes on which this strategy wraps out-of-range queries (bit 0: x, bit 1: y): the periodic axes of a strategy
        that extrapolates."""
        return self._periodic if self._extrapolate else 0

    @staticmethod
    def _is_default(ends) -> bool:
        return all(int(e.kind) == _capi.BC_NOT_A_KNOT and float(e.value) == 0.0 for e in (ends.left, ends.right))

    def build(self, x, y, data, device=None):
        dt = np_dtype_of(data)
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            got = "bfloat16" if is_bf16(dt) else dt
            raise TypeError(f"Bicubic covers float32/float64 only, got {got}: a spline divides (integer data takes "
                            "Bilinear) and the spline build has no half-precision form")
        for bit, name, ends in ((1, "x", self._bc_x), (2, "y", self._bc_y)):
            if self._periodic & bit and not self._is_default(ends):
                raise TypeError(f"Bicubic: the {name} axis is periodic and takes no boundary condition: a periodic end has "
                                f"no kind (boundary_{name} / boundary gave it one)")
        if self.rule in ("pchip", "akima"):
            code = _capi.PCHIP if self.rule == "pchip" else _capi.AKIMA
            return self._create(x, y, data, device,
                                lambda d, h: _capi.lib().ndi_interp2d_create_bicubic_local(C.byref(d), code, C.byref(h)))
        if self.rule == "hermite":
            return self._create_hermite(x, y, data, device)
        ends = (self._bc_x.left, self._bc_x.right, self._bc_y.left, self._bc_y.right)
        bc = (_capi.Boundary * 4)(*[_capi.Boundary(int(e.kind), float(e.value)) for e in ends])
        if self._periodic:
            per = self._periodic
            return self._create(x, y, data, device,
                                lambda d, h: _capi.lib().ndi_interp2d_create_bicubic_periodic(C.byref(d), bc, per, C.byref(h)))
        return self._create(x, y, data, device,
                            lambda d, h: _capi.lib().ndi_interp2d_create_bicubic(C.byref(d), bc, C.byref(h)))

    def _create_hermite(self, x, y, data, device):
        dt = np_dtype_of(data)
        for name, t in zip(("zx", "zy", "zxy"), self._given):
            if not hasattr(t, "shape") or not hasattr(t, "dtype"):
                raise TypeError(f"Bicubic.hermite: {name} is a numpy array or a tensor, got {type(t).__name__}")
            if tuple(t.shape) != tuple(data.shape):
                raise BuilderError.ShapeError(
                    f"{name} has wrong shape. Expected: {list(data.shape)}, got: {list(t.shape)}")
            if np_dtype_of(t) != dt:
                raise TypeError(f"Bicubic.hermite: {name} has element type {np_dtype_of(t)}, the data is {dt}")
        on_dev = is_torch(data) and data.is_cuda
        # the tables travel in the same memory space as the data
        bufs = [Buf(_to_device(t, data.device), dt) if on_dev else Buf(_host(t), dt) for t in self._given]
        return self._create(x, y, data, device,
                            lambda d, h: _capi.lib().ndi_interp2d_create_bicubic_hermite(
                                C.byref(d), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, C.byref(h)))

    orders = (0, 0)    # (nu_x, nu_y) of the partial derivative this strategy evaluates; (0, 0): the surface
    origin = None      # a partial's source strategy (kept for documentation's sake: the library owns the shared table)

    def partial(self, nu_x=0, nu_y=0) -> "Bicubic":
        """The partial derivative d^(nu_x + nu_y) / dx^nu_x dy^nu_y of this built strategy's surface as a built strategy of
        its own (ndi_interp2d_partial; scipy: `RectBivariateSpline.ev(x, y, dx=nu_x, dy=nu_y)`).  Orders are 0, 1 or 2 per
        variable, not both 0, and add up over repeated calls.  The new handle shares this one's node table on the device --
        no copy -- and either may be released first.  This strategy stays usable."""
        import operator
        try:
            nu_x, nu_y = operator.index(nu_x), operator.index(nu_y)
        except TypeError:
            raise TypeError(f"Bicubic.partial: the orders are integers, got ({type(nu_x).__name__}, "
                            f"{type(nu_y).__name__})") from None
        if nu_x < 0 or nu_y < 0:
            raise ValueError(f"Bicubic.partial: an order below 0 (asked for ({nu_x}, {nu_y})); orders are 0, 1 or 2 per "
                             "variable")
        if nu_x == 0 and nu_y == 0:
            raise ValueError("Bicubic.partial: orders (0, 0) are the strategy itself; ask for an order of 1 or 2 in at least "
                             "one variable")
        if self.is_integral:
            raise ValueError("Bicubic.partial: an integral strategy has no partial derivatives: its x-derivative is a "
                             "y-integral of the surface, which is not provided")
        tx, ty = self.orders[0] + nu_x, self.orders[1] + nu_y
        if tx > 2 or ty > 2:
            raise ValueError(f"Bicubic.partial: the third derivative of a cubic spline jumps at the grid lines; orders are 0 "
                             f"to 2 per variable (asked for ({nu_x}, {nu_y}) of a strategy of orders {self.orders}: "
                             f"({tx}, {ty}))")
        if self._h is None:
            from .errors import DeviceError
            raise DeviceError("Bicubic.partial needs a built strategy: the node table lives on the device and partial "
                              "derivatives are evaluated there; there is no CPU fallback")
        import copy
        h = C.c_void_p()
        st = _capi.lib().ndi_interp2d_partial(self._h, nu_x, nu_y, C.byref(h))
        if st == _capi.BAD_ARG:
            raise ValueError(_capi.last_error())
        if st != _capi.OK:
            raise_builder(st)
        other = copy.copy(self)
        other._h, other._inflight = h, []
        other.orders, other.origin = (tx, ty), self
        return other

    is_integral = False   # True on the strategy `antiderivative()` returns

    def antiderivative(self) -> "Bicubic":
        """F(x, y), the integral of this built strategy's surface over [x[0], x] x [y[0], y], as a built strategy of its own
        (ndi_interp2d_antiderivative).  It evaluates like any Bicubic strategy and adds `integral(xa, xb, ya, yb)` (scipy:
        `RectBivariateSpline.integral`).  The new handle shares this one's node table on the device and owns its five
        prefix tables; either may be released first.  This strategy stays usable."""
        if self.is_integral:
            raise ValueError("Bicubic.antiderivative: this strategy is already an integral; a second antiderivative is not "
                             "provided")
        if self.orders != (0, 0):
            raise ValueError(f"Bicubic.antiderivative: a partial-derivative strategy (orders {self.orders}) has no "
                             "antiderivative; ask the surface's strategy")
        if self.wraps:
            axes = " and ".join(n for b, n in ((1, "x"), (2, "y")) if self.wraps & b)
            raise TypeError(f"Bicubic.antiderivative: this strategy wraps queries on {axes} (a periodic axis with "
                            "extrapolate): the integral of a periodic surface is not periodic, and the antiderivative of a "
                            "wrapping strategy is not provided (build without extrapolate)")
        if self._h is None:
            from .errors import DeviceError
            raise DeviceError("Bicubic.antiderivative needs a built strategy: the node table lives on the device and the "
                              "prefix tables are built there; there is no CPU fallback")
        import copy
        h = C.c_void_p()
        st = _capi.lib().ndi_interp2d_antiderivative(self._h, C.byref(h))
        if st == _capi.BAD_ARG:
            raise ValueError(_capi.last_error())
        if st != _capi.OK:
            raise_builder(st)
        other = copy.copy(self)
        other._h, other._inflight = h, []
        other.is_integral, other.origin = True, self
        return other

    def integral(self, xa_flat, xb_flat, ya_flat, yb_flat, out2d, *, fresh=False):
        """Rectangle integrals (ndi_interp2d_integral): row q of `out2d` (nq, lanes) is the integral over
        [xa[q], xb[q]] x [ya[q], yb[q]].  Reversed bounds negate; equal bounds give exactly 0."""
        if not self.is_integral:
            raise TypeError("Bicubic.integral needs the integral strategy: call antiderivative() first "
                            f"(this is a Bicubic strategy of orders {self.orders})")
        q = [Buf(a, self._np_dtype) for a in (xa_flat, xb_flat, ya_flat, yb_flat)]
        if len({b.memspace for b in q}) != 1:
            raise TypeError("Bicubic.integral: the four bounds must live in the same memory space")
        if len({b.size for b in q}) != 1:
            raise ValueError(f"Bicubic.integral: the four bounds differ in length: {[b.size for b in q]}")
        _check_out_dtype(out2d, self._np_dtype)
        opts = _capi.EvalOpts()
        opts.q_memspace = q[0].memspace
        opts.path = self.path
        opts.flags = _capi.EVAL_FRESH_OUTPUT if fresh else _capi.EVAL_DEFAULT
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
            if q[0].memspace == _capi.MEM_DEVICE:
                opts.stream = current_stream_ptr(self._device)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp2d_integral(self._h, q[0].ptr, q[1].ptr, q[2].ptr, q[3].ptr, q[0].size, optr,
                                               max(stride, self._lanes), C.byref(opts), C.byref(info))
        if st != _capi.OK:
            raise_eval(st, info, None)

    def _jet_parts(self, order, n_buffers=None) -> int:
        """The refusals of a jet call that come before the library is reached; returns K, the number of parts."""
        import operator
        if self.is_integral:
            raise ValueError("Bicubic.jet_into: an integral strategy has no value-and-gradient (jet) evaluation: its "
                             "x-derivative is a y-integral of the surface, which is not provided; ask the surface's strategy")
        if self.orders != (0, 0):
            raise ValueError(f"Bicubic.jet_into: a partial-derivative strategy (orders {self.orders}) has no jet: a jet of a "
                             "partial would need third orders, which jump at the grid lines; ask the surface's strategy")
        if order is None and n_buffers is not None:
            order = {len(p): o for o, p in JET_PARTS.items()}.get(n_buffers)
            if order is None:
                raise ValueError(f"Bicubic.jet_into: {n_buffers} output buffers select no order: order 1 writes "
                                 f"{len(JET_PARTS[1])} parts, order 2 writes {len(JET_PARTS[2])}")
        try:
            order = operator.index(order)
        except TypeError:
            raise TypeError(f"Bicubic.jet_into: the order is an integer, got {type(order).__name__}") from None
        if order not in JET_PARTS:
            raise ValueError(f"Bicubic.jet_into: order {order}; a jet has order 1 (value and gradient) or 2 (with the three "
                             "second derivatives): the third derivative of a cubic spline jumps at the grid lines")
        if n_buffers is not None and n_buffers != len(JET_PARTS[order]):
            raise ValueError(f"Bicubic.jet_into: order {order} writes {len(JET_PARTS[order])} parts, got {n_buffers} output "
                             "buffers (parts cannot be skipped)")
        if self._h is None:
            from .errors import DeviceError
            raise DeviceError("Bicubic.jet_into needs a built strategy: the node table lives on the device and the jet is "
                              "evaluated there; there is no CPU fallback")
        return order

    def jet_into(self, xs_flat, ys_flat, outs, *, order=None, fresh=False):
        """The surface and its partial derivatives up to `order` at the same queries in ONE evaluation
        (ndi_interp2d_eval_jet): `outs` is a sequence of K = 3 (order 1) or 6 (order 2) buffers (nq, lanes), part k being
        the partial of orders JET_PARTS[order][k] -- bit for bit the rows `partial(nu_x, nu_y)` evaluates.  `order` is
        inferred from len(outs) when not given.  The buffers are numpy arrays (host) or torch tensors on the device, all
        in one memory space and of the data's dtype; their rows need not be contiguous with each other, but all K buffers
        share ONE row stride (planar and interleaved layouts both do)."""
        outs = list(outs)
        order = self._jet_parts(order, len(outs))
        qx = Buf(xs_flat, self._np_dtype)
        qy = Buf(ys_flat, self._np_dtype)
        if qx.memspace != qy.memspace:
            raise TypeError("xs and ys must live in the same memory space")
        if len({is_torch(o) for o in outs}) != 1:
            raise TypeError("Bicubic.jet_into: the output buffers must live in one memory space (all numpy host arrays or "
                            "all torch device tensors)")
        on_dev = is_torch(outs[0])
        strides, ptrs = [], []
        for k, o in enumerate(outs):
            _check_out_dtype(o, self._np_dtype)
            if on_dev and not o.is_cuda:
                raise TypeError("torch output buffers must live on the device; use numpy for host buffers")
            if len(o.shape) != 2 or tuple(o.shape) != (qx.size, self._lanes):
                raise ValueError(f"Bicubic.jet_into: buffer {k} has shape {tuple(o.shape)}, expected "
                                 f"{(qx.size, self._lanes)} (queries, lanes)")
            st = o.stride() if on_dev else tuple(b // o.itemsize for b in o.strides)
            if self._lanes > 1 and qx.size > 0 and st[1] != 1:
                raise ValueError(f"Bicubic.jet_into: buffer {k} has element strides {tuple(st)}: the lanes of a row must be "
                                 "contiguous")
            strides.append(st[0] if qx.size > 1 else self._lanes)
            ptrs.append(o.data_ptr() if on_dev else o.ctypes.data)
        if len(set(strides)) != 1 or strides[0] < self._lanes:
            raise ValueError(f"Bicubic.jet_into: the buffers must share one row stride >= lanes ({self._lanes}), got row "
                             f"strides {strides}")
        opts = _capi.EvalOpts()
        opts.q_memspace = qx.memspace
        opts.path = self.path
        opts.flags = _capi.EVAL_FRESH_OUTPUT if fresh else _capi.EVAL_DEFAULT
        opts.out_memspace = _capi.MEM_DEVICE if on_dev else _capi.MEM_HOST
        if on_dev or qx.memspace == _capi.MEM_DEVICE:
            opts.stream = current_stream_ptr(self._device)
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp2d_eval_jet(self._h, order, qx.ptr, qy.ptr, qx.size, arr, strides[0], C.byref(opts),
                                               C.byref(info))
        if st != _capi.OK:
            raise_eval(st, info, None)

    def integral_tables(self, on_device=False):
        """(PP, Qz, Qzy, Pz, Pzx): the five prefix tables of an integral strategy, each of the data's shape
        (ndi_interp2d_integral_tables), as host arrays -- or, with `on_device`, as tensors on the handle's device."""
        if on_device:
            import torch
            out = [torch.empty(self._shape, dtype=torch_dtype(self._np_dtype), device=f"cuda:{self._device}") for _ in range(5)]
            ptrs, space = [t.data_ptr() for t in out], _capi.MEM_DEVICE
        else:
            out = [np.empty(self._shape, dtype=self._np_dtype) for _ in range(5)]
            ptrs, space = [a.ctypes.data for a in out], _capi.MEM_HOST
        st = _capi.lib().ndi_interp2d_integral_tables(self._h, *ptrs, space)
        if st != _capi.OK:
            from .errors import DeviceError
            raise DeviceError(_capi.last_error())
        return tuple(out)

    def tables(self, on_device=False):
        """(zx, zy, zxy): the node derivatives, each of the data's shape (ndi_interp2d_tables), as host arrays -- or, with
        `on_device`, as tensors on the handle's device."""
        if on_device:
            import torch
            out = [torch.empty(self._shape, dtype=torch_dtype(self._np_dtype), device=f"cuda:{self._device}") for _ in range(3)]
            ptrs, space = [t.data_ptr() for t in out], _capi.MEM_DEVICE
        else:
            out = [np.empty(self._shape, dtype=self._np_dtype) for _ in range(3)]
            ptrs, space = [a.ctypes.data for a in out], _capi.MEM_HOST
        st = _capi.lib().ndi_interp2d_tables(self._h, ptrs[0], ptrs[1], ptrs[2], space)
        if st != _capi.OK:
            from .errors import DeviceError
            raise DeviceError(_capi.last_error())
        return tuple(out)


class Interp2D:
    """Two dimensional interpolator (interp2d/mod.rs:36-48)."""

    def __init__(self, x, y, data, strategy):
        self.x, self.y, self.data, self.strategy = x, y, data, strategy
        self._x_host, self._y_host = _host(x), _host(y)

    @staticmethod
    def builder(data) -> "Interp2DBuilder":
        return Interp2DBuilder.new(data)

    @staticmethod
    def new_unchecked(x, y, data, strategy) -> "Interp2D":
        return Interp2D(x, y, data, strategy)

    def index_point(self, x_idx: int, y_idx: int):
        return self._x_host[x_idx], self._y_host[y_idx], self.data[x_idx, y_idx]

    def get_index_left_of(self, x, y):
        def one(k, v):
            if k.dtype in (np.float32, np.float64):
                r = int(get_lower_index(np.ascontiguousarray(k), np.array([v], dtype=k.dtype))[0])
                if r < 0:
                    raise Panic("not implemented: failed to convert NaN to usize")
                return r
            return int(np.clip(np.searchsorted(k, v, side="right") - 1, 0, k.size - 2))
        return one(self._x_host, x), one(self._y_host, y)

    def is_in_x_range(self, x) -> bool:
        return bool(self._x_host[0] <= x <= self._x_host[-1])

    def is_in_y_range(self, y) -> bool:
        return bool(self._y_host[0] <= y <= self._y_host[-1])

    def _lanes_shape(self):
        return tuple(self.data.shape[2:])

    def interp_scalar(self, x, y):
        """interp2d/mod.rs:107-113 (data must be 2-D)."""
        if len(self.data.shape) != 2:
            raise TypeError("interp_scalar needs 2-D data; use interp()")
        buf = _zeros((), np_dtype_of(self.data))
        self.strategy.interp_into(self, buf, x, y)
        return buf[()]

    def interp(self, x, y):
        target = _zeros(self._lanes_shape(), np_dtype_of(self.data))
        self.strategy.interp_into(self, target, x, y)
        return target

    def interp_into(self, x, y, buffer):
        if tuple(buffer.shape) != self._lanes_shape():
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: "
                        f"{list(self._lanes_shape())}, got: {list(buffer.shape)}")
        self.strategy.interp_into(self, buffer, x, y)

    def get_buffer_shape(self, q_shape):
        """interp2d/mod.rs:310-321."""
        return tuple(q_shape) + self._lanes_shape()

    def interp_array(self, xs, ys):
        """interp2d/mod.rs:175-196; panics when `xs.shape != ys.shape`."""
        if tuple(xs.shape) != tuple(ys.shape):
            raise Panic("`xs.shape()` and `ys.shape()` do not match")
        shape = self.get_buffer_shape(tuple(xs.shape))
        if is_torch(xs) and xs.is_cuda:
            import torch
            tdt = torch_dtype(np_dtype_of(self.data))
            if tdt is None:
                raise TypeError("device query tensors need f32 / f64 data; other element types use host arrays")
            nbytes = int(np.prod(shape, dtype=np.int64)) * np_dtype_of(self.data).itemsize
            if nbytes >= OUTPUT_OWNED_MIN_BYTES and not is_bf16(np_dtype_of(self.data)):
                # Array::zeros through the library's placement-checked allocator
                zs = output_empty(shape, np_dtype_of(self.data), xs.device.index or 0)
            else:
                zs = torch.empty(shape, dtype=tdt, device=xs.device)
        elif is_bf16(np_dtype_of(self.data)):
            # bf16 results are torch tensors: on the interpolator's device
            zs = _zeros(shape, np_dtype_of(self.data), f"cuda:{self.strategy._device}")
        else:
            zs = np.zeros(shape, dtype=np_dtype_of(self.data))
        # the buffer is this call's own and is dropped on Err (:193-195): strategies that can use the knowledge are told
        self.interp_array_into(xs, ys, zs, **({"fresh": True} if getattr(self.strategy, "_takes_fresh", False) else {}))
        return zs

    def interp_array_into(self, xs, ys, buffer, **kw):
        """interp2d/mod.rs:215-285."""
        if tuple(xs.shape) != tuple(ys.shape):
            raise Panic("`xs.shape()` and `ys.shape()` do not match")
        expect = self.get_buffer_shape(tuple(xs.shape))
        if tuple(buffer.shape) != expect:
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: {list(expect)}, "
                        f"got: {list(buffer.shape)}")
        if np_dtype_of(buffer) != np_dtype_of(self.data):
            raise TypeError(f"buffer has element type {np_dtype_of(buffer)}, the data is {np_dtype_of(self.data)}")
        nq = int(np.prod(xs.shape, dtype=np.int64))
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        xf, yf = xs.reshape(-1), ys.reshape(-1)
        if is_torch(buffer):
            if not buffer.is_contiguous():
                raise TypeError("device output buffers must be contiguous")
            self.strategy.interp_array_into(self, xf, yf, buffer.view(nq, lanes), **kw)
            return
        if not is_torch(xs):
            xf, yf = _host(xf), _host(yf)
        if buffer.flags.c_contiguous:
            self.strategy.interp_array_into(self, xf, yf, buffer.reshape(nq, lanes), **kw)
            return
        tmp = np.zeros((nq, lanes), dtype=np_dtype_of(self.data))
        done = nq
        try:
            self.strategy.interp_array_into(self, xf, yf, tmp, **kw)
        except (InterpolateError.OutOfBounds, Panic) as e:
            done = e.index if getattr(e, "index", None) is not None else 0   # rows before the failing query are
            raise                                          # written, later rows stay untouched (interp2d/mod.rs:297-306)
        except BaseException:
            done = 0                                       # device failure: nothing in tmp can be trusted
            raise
        finally:
            if done and len(xs.shape) == 0:
                buffer[...] = tmp[0].reshape(buffer.shape)
            elif done:
                where = np.unravel_index(np.arange(done), tuple(xs.shape))
                buffer[where] = tmp[:done].reshape((done,) + self._lanes_shape())

    def interp_lanewise(self, xs, ys):
        """An (x, y) per channel: `xs.shape == ys.shape` ends with `data.shape[2:]` and
        `result[..., l] = f_l(xs[..., l], ys[..., l])`, where `interp_array` evaluates every channel at one point.  The
        result has `xs.shape` and the data's element type; numpy in -> numpy out, a device tensor in -> a tensor on its
        device.  Works on `partial(nu_x, nu_y)` of a Bicubic too.  `InterpolateError.OutOfBounds.index` is the flat element
        index."""
        self._lanewise_check(xs, ys)
        dt = np_dtype_of(self.data)
        if is_torch(xs) and xs.is_cuda:
            import torch
            zs = torch.empty(tuple(xs.shape), dtype=torch_dtype(dt), device=xs.device)
        else:
            zs = np.zeros(tuple(xs.shape), dtype=dt)
        self.interp_lanewise_into(xs, ys, zs, fresh=True)
        return zs

    def interp_lanewise_into(self, xs, ys, buffer, *, fresh=False, rows_after_error_unspecified=False):
        """`interp_lanewise` into a caller's buffer of `xs.shape`: rows (one per leading index) before the row of the
        first failing element are written, that row and all later ones stay untouched -- unless `fresh` or
        `rows_after_error_unspecified` give them up, which saves a pass over the queries."""
        self._lanewise_check(xs, ys)
        if tuple(buffer.shape) != tuple(xs.shape):
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: {list(xs.shape)}, "
                        f"got: {list(buffer.shape)}")
        if np_dtype_of(buffer) != np_dtype_of(self.data):
            raise TypeError(f"buffer has element type {np_dtype_of(buffer)}, the data is {np_dtype_of(self.data)}")
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        nq = int(np.prod(xs.shape, dtype=np.int64)) // max(lanes, 1)
        kw = dict(fresh=fresh, rows_after_error_unspecified=rows_after_error_unspecified)

        def rows(a):
            return a.reshape(nq, lanes) if is_torch(a) else _host(a).reshape(nq, lanes)
        if is_torch(buffer):
            if not buffer.is_contiguous():
                raise TypeError("device output buffers must be contiguous")
            self.strategy.interp_lanewise_into(self, xs.reshape(nq, lanes), ys.reshape(nq, lanes), buffer.view(nq, lanes), **kw)
            return
        if not buffer.flags.c_contiguous:
            raise TypeError("interp_lanewise_into needs a C-contiguous host buffer")
        self.strategy.interp_lanewise_into(self, rows(xs), rows(ys), buffer.reshape(nq, lanes), **kw)

    def _lanewise_check(self, xs, ys):
        if not isinstance(self.strategy, _DeviceStrategy2D):
            raise TypeError("interp_lanewise needs a built-in device strategy (Bilinear or Bicubic on f32 / f64 data, or a "
                            f"partial derivative of a Bicubic), got {type(self.strategy).__name__}")
        if tuple(xs.shape) != tuple(ys.shape):
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: {list(xs.shape)}, "
                        f"got: {list(ys.shape)}")
        lanes_shape = self._lanes_shape()
        k = len(lanes_shape)
        if len(xs.shape) < k or tuple(xs.shape)[len(xs.shape) - k:] != lanes_shape:
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: [.., "
                        f"{', '.join(str(d) for d in lanes_shape)}], got: {list(xs.shape)}")

    def partial(self, nu_x=0, nu_y=0) -> "Interp2D":
        """The partial derivative d^(nu_x + nu_y) / dx^nu_x dy^nu_y of this interpolator's surface as an interpolator over
        the same axes (`Bicubic.partial`): orders 0, 1 or 2 per variable, not both 0; they add up over repeated calls.
        `data` stays the surface's node values (the derivative shares the source's node table on the device)."""
        if not hasattr(self.strategy, "partial"):
            raise TypeError("partial needs a built Bicubic strategy (f32 / f64 data), got "
                            f"{type(self.strategy).__name__}")
        return Interp2D(self.x, self.y, self.data, self.strategy.partial(nu_x, nu_y))

    def antiderivative(self) -> "Interp2D":
        """F(x, y), the integral of this interpolator's surface over [x[0], x] x [y[0], y], as an interpolator over the same
        axes (`Bicubic.antiderivative`).  `data` stays the surface's node values.  The result also has `integral`."""
        if not hasattr(self.strategy, "antiderivative"):
            raise TypeError("antiderivative needs a built Bicubic strategy (f32 / f64 data), got "
                            f"{type(self.strategy).__name__}")
        return Interp2D(self.x, self.y, self.data, self.strategy.antiderivative())

    def integral(self, xa, xb, ya, yb):
        """Integrals of the surface over the rectangles [xa, xb] x [ya, yb] (scipy: `RectBivariateSpline.integral`), on the
        interpolator `antiderivative()` returns.  The four bounds broadcast to one common shape; the result has that shape
        followed by the trailing data shape.  Reversed bounds negate; equal bounds give exactly 0."""
        strat = self.strategy
        if not getattr(strat, "is_integral", False):
            if isinstance(strat, Bicubic):
                raise TypeError("Interp2D.integral: this is a Bicubic interpolator of the surface (or a partial); call "
                                "antiderivative() first and integrate through the interpolator it returns")
            raise TypeError(f"Interp2D.integral needs the antiderivative of a Bicubic interpolator, got "
                            f"{type(strat).__name__}: {type(strat).__name__} has no 2-D integrals")
        bounds = (xa, xb, ya, yb)
        dt = np_dtype_of(self.data)
        on_dev = [is_torch(b) and b.is_cuda for b in bounds]
        if any(on_dev) and not all(on_dev):
            raise TypeError("Bicubic integral: the four bounds must live in the same memory space")
        try:
            if all(on_dev):
                import torch
                flat = [b.to(torch_dtype(dt)) for b in bounds]
                flat = [b.contiguous() for b in torch.broadcast_tensors(*flat)]
            else:
                flat = [np.ascontiguousarray(b) for b in np.broadcast_arrays(*[np.asarray(_host(b), dtype=dt) for b in bounds])]
        except (ValueError, RuntimeError):
            raise ValueError("Bicubic integral: the bound shapes do not broadcast to one shape: "
                             f"{[tuple(np.shape(b)) for b in bounds]}") from None
        qshape = tuple(flat[0].shape)
        shape = self.get_buffer_shape(qshape)
        nq = int(np.prod(qshape, dtype=np.int64))
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        if all(on_dev):
            import torch
            zs = torch.empty(shape, dtype=torch_dtype(dt), device=flat[0].device)
            strat.integral(*[b.reshape(-1) for b in flat], zs.view(nq, lanes), fresh=True)
        else:
            zs = np.zeros(shape, dtype=dt)
            strat.integral(*[b.reshape(-1) for b in flat], zs.reshape(nq, lanes), fresh=True)
        return zs

    def _jet_strategy(self, what):
        if not hasattr(self.strategy, "jet_into"):
            raise TypeError(f"Interp2D.{what} needs a built Bicubic strategy (f32 / f64 data), got "
                            f"{type(self.strategy).__name__}")
        if not isinstance(self.strategy, Bicubic):
            self.strategy.jet_into()      # Bilinear: the TypeError naming the strategy
        return self.strategy

    def jet(self, xs, ys, order=1):
        """The surface and its partial derivatives up to `order` (1 or 2) at the queries, in ONE evaluation
        (`Bicubic.jet_into`): a tuple of K = 3 or 6 arrays in the order of JET_PARTS[order], each of shape
        `xs.shape ++ trailing data shape` and equal, bit for bit, to `partial(nu_x, nu_y).interp_array(xs, ys)` (part 0 to
        `interp_array(xs, ys)`).  They are views of one allocation of shape (K, ...): a torch tensor on the queries' device
        for device queries, a numpy array otherwise.  Panics when `xs.shape != ys.shape`."""
        strat = self._jet_strategy("jet")
        order = strat._jet_parts(order)
        if tuple(xs.shape) != tuple(ys.shape):
            raise Panic("`xs.shape()` and `ys.shape()` do not match")
        K = len(JET_PARTS[order])
        shape = self.get_buffer_shape(tuple(xs.shape))
        dt = np_dtype_of(self.data)
        nq = int(np.prod(xs.shape, dtype=np.int64))
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        if is_torch(xs) and xs.is_cuda:
            import torch
            zs = torch.empty((K,) + shape, dtype=torch_dtype(dt), device=xs.device)
            xf, yf, flat = xs.reshape(-1), ys.reshape(-1), zs.view(K, nq, lanes)
        else:
            zs = np.zeros((K,) + shape, dtype=dt)
            xf, yf, flat = _host(xs).reshape(-1), _host(ys).reshape(-1), zs.reshape(K, nq, lanes)
        strat.jet_into(xf, yf, [flat[k] for k in range(K)], order=order, fresh=True)
        return tuple(zs[k] for k in range(K))

    def value_and_gradient(self, xs, ys):
        """(z, dz/dx, dz/dy) at the queries in one evaluation: `jet(xs, ys, 1)`."""
        return self.jet(xs, ys, 1)

    def jet_into(self, xs, ys, buffers):
        """`jet` into K = 3 (order 1) or 6 (order 2) caller-owned buffers, each of the shape and dtype `interp_array_into`
        takes, with its semantics: if a query fails, the rows before it are written in every buffer and the rows from it
        on are left untouched in every buffer."""
        strat = self._jet_strategy("jet_into")
        buffers = list(buffers)
        order = strat._jet_parts(None, len(buffers))
        if tuple(xs.shape) != tuple(ys.shape):
            raise Panic("`xs.shape()` and `ys.shape()` do not match")
        expect = self.get_buffer_shape(tuple(xs.shape))
        dt = np_dtype_of(self.data)
        for b in buffers:
            if tuple(b.shape) != expect:
                raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: {list(expect)}, "
                            f"got: {list(b.shape)}")
            if np_dtype_of(b) != dt:
                raise TypeError(f"buffer has element type {np_dtype_of(b)}, the data is {dt}")
        if len({is_torch(b) for b in buffers}) != 1:
            raise TypeError("Interp2D.jet_into: the buffers must live in one memory space (all numpy host arrays or all "
                            "torch device tensors)")
        nq = int(np.prod(xs.shape, dtype=np.int64))
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        xf, yf = xs.reshape(-1), ys.reshape(-1)
        if is_torch(buffers[0]):
            if not all(b.is_contiguous() for b in buffers):
                raise TypeError("device output buffers must be contiguous")
            strat.jet_into(xf, yf, [b.view(nq, lanes) for b in buffers], order=order)
            return
        if not is_torch(xs):
            xf, yf = _host(xf), _host(yf)
        if all(b.flags.c_contiguous for b in buffers):
            strat.jet_into(xf, yf, [b.reshape(nq, lanes) for b in buffers], order=order)
            return
        tmp = np.zeros((len(buffers), nq, lanes), dtype=dt)
        done = nq
        try:
            strat.jet_into(xf, yf, list(tmp), order=order)
        except (InterpolateError.OutOfBounds, Panic) as e:
            done = e.index if getattr(e, "index", None) is not None else 0   # as interp_array_into: rows before the failure
            raise
        except BaseException:
            done = 0
            raise
        finally:
            for b, t in zip(buffers, tmp):
                if done and len(xs.shape) == 0:
                    b[...] = t[0].reshape(b.shape)
                elif done:
                    where = np.unravel_index(np.arange(done), tuple(xs.shape))
                    b[where] = t[:done].reshape((done,) + self._lanes_shape())

    def replicate(self, devices):
        """Replicas of this interpolator on the given devices (see Interp1D.replicate)."""
        if not hasattr(self.strategy, "clone"):
            raise TypeError("replicate needs a built-in device strategy (f32 / f64 data)")
        return [Interp2D(self.x, self.y, self.data, self.strategy.clone(d)) for d in devices]

    def interp_array_ring(self, xs, ys, chunk_queries, consumer=None, *, slots=None, n_slots=2):
        """`interp_array` (interp2d/mod.rs:175-196) through a device-output ring (ndi_interp2d_eval_ring)."""
        if tuple(xs.shape) != tuple(ys.shape):
            raise Panic("`xs.shape()` and `ys.shape()` do not match")
        if not hasattr(self.strategy, "interp_array_ring"):
            raise TypeError("the ring evaluation needs the built-in device strategy (f32 / f64 data)")
        self.strategy.interp_array_ring(xs.reshape(-1), ys.reshape(-1), chunk_queries, consumer, slots=slots,
                                        n_slots=n_slots)


class Interp2DBuilder:
    """Create and configure a `Interp2D` interpolator (interp2d/mod.rs:52-64, 382-519)."""

    def __init__(self, data, x=None, y=None, strategy=None):
        self._data, self._x, self._y = data, x, y
        self._strategy = strategy if strategy is not None else Bilinear.new()  # :403

    @staticmethod
    def new(data) -> "Interp2DBuilder":
        return Interp2DBuilder(data)

    def strategy(self, strategy) -> "Interp2DBuilder":
        return Interp2DBuilder(self._data, self._x, self._y, strategy)

    def x(self, x) -> "Interp2DBuilder":
        return Interp2DBuilder(self._data, x, self._y, self._strategy)

    def y(self, y) -> "Interp2DBuilder":
        return Interp2DBuilder(self._data, self._x, y, self._strategy)

    def build(self) -> Interp2D:
        """Validate the input and create the configured `Interp2D` (interp2d/mod.rs:468-518)."""
        data, strategy = self._data, self._strategy
        shape = tuple(data.shape)
        if len(shape) < 2:
            raise BuilderError.ShapeError("data dimension needs to be at least 2")
        need = strategy.MINIMUM_DATA_LENGHT    # (a Bicubic strategy of a local rule carries its own)
        if shape[0] < need:
            raise BuilderError.NotEnoughData(
                "The 0-dimension has not enough data for the chosen interpolation strategy. "
                f"Provided: {shape[0]}, Reqired: {need}")
        if shape[1] < need:
            raise BuilderError.NotEnoughData(
                "The 1-dimension has not enough data for the chosen interpolation strategy. "
                f"Provided: {shape[1]}, Reqired: {need}")
        dt = np_dtype_of(data)
        x = _default_axis(shape[0], dt) if self._x is None else self._x
        y = _default_axis(shape[1], dt) if self._y is None else self._y
        x_len = int(np.prod(x.shape, dtype=np.int64))
        y_len = int(np.prod(y.shape, dtype=np.int64))
        if x_len != shape[0]:
            raise BuilderError.ShapeError(
                f"Lenghts of x-axis and data-0-axis need to match. Got x: {x_len}, data-0: {shape[0]}")
        if y_len != shape[1]:
            raise BuilderError.ShapeError(
                f"Lenghts of y-axis and data-1-axis need to match. Got y: {y_len}, data-1: {shape[1]}")
        if monotonic_prop(x) != Monotonic.Rising(True):
            raise BuilderError.Monotonic("The x-axis needs to be strictly monotonic rising")
        if monotonic_prop(y) != Monotonic.Rising(True):
            raise BuilderError.Monotonic("The y-axis needs to be strictly monotonic rising")
        finished = strategy.build(x, y, data)
        return Interp2D(x, y, data, finished)
