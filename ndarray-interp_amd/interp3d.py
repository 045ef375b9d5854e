"""Interp3D: interpolation along the first three axes of n-dimensional data, with the `Trilinear` (include/ndinterp3d.h)
and `Tricubic` (include/ndinterp3d_cubic.h) strategies evaluated on the device.  The reference stops at two axes; these are
its Bilinear taken one axis further and the Bicubic of this project taken one axis further, written like `interp2d.py`: `Interp3D.builder(data).x(x).y(y).z(z).strategy(Trilinear.new()).build()`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._arrays import Buf, current_stream_ptr, is_torch, np_dtype_of, torch_dtype
from .errors import BuilderError, InterpolateError, Panic, raise_builder, raise_eval
from .interp1d import BoundaryCondition, RowBoundary, _check_out_dtype, _default_axis, _default_device, _host, _to_device
from .vector_extensions import Monotonic, get_lower_index, monotonic_prop

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


class Interp3DStrategyBuilder:
    """What a 3-D strategy builder provides (the shape of Interp2DStrategyBuilder, one axis further)."""

    MINIMUM_DATA_LENGHT = 2

    def build(self, x, y, z, data) -> "Interp3DStrategy":
        raise NotImplementedError


class Interp3DStrategy:
    """A finished 3-D strategy: per-query `interp_into(interpolator, target, x, y, z)`; `interp_array_into` is the batched
    hook whose default body is the serial loop."""

    def interp_into(self, interpolator, target, x, y, z) -> None:
        raise NotImplementedError

    def interp_array_into(self, interpolator, xs_flat, ys_flat, zs_flat, out2d, **kw) -> None:
        shape = tuple(interpolator.data.shape[3:])
        for i in range(len(xs_flat)):
            self.interp_into(interpolator, out2d[i].reshape(shape), xs_flat[i], ys_flat[i], zs_flat[i])

    def release(self) -> None:
        pass


class _DeviceStrategy3D(Interp3DStrategyBuilder, Interp3DStrategy):
    """What the built-in 3-D strategies share: builder and finished strategy in one, like `Bilinear`; the handle, its
    release and clone, and the one C-ABI call per batch.  A strategy states its name in the errors by being the class it
    is, and its create call in `_create_call`."""

    _takes_fresh = True

    def __init__(self):
        self._extrapolate = False
        self._h = None
        self._device = 0
        self._device_req = None
        self._np_dtype = None
        self._lanes = 1
        self._shape = None

    def device(self, ordinal: int):
        """The HIP device that holds the grid (default: the data tensor's device, else LOCAL_RANK / device 0)."""
        self._device_req = int(ordinal)
        return self

    def extrapolate(self, yes: bool):
        self._extrapolate = bool(yes)
        return self

    def _create_call(self, desc, handle) -> int:
        raise NotImplementedError

    def build(self, x, y, z, data, device=None):
        dt = np_dtype_of(data)
        if dt not in _FLOATS:
            raise TypeError(f"{type(self).__name__} takes float32 / float64 data, got {dt}: integer and f16 / bf16 element "
                            "types are not provided in three dimensions")
        db = Buf(data)

        def axis(a):
            if db.memspace == _capi.MEM_HOST:
                return Buf(_host(a), dt)
            return Buf(_to_device(a, db.keep.device), dt)

        xb, yb, zb = axis(x), axis(y), axis(z)
        if device is None:
            device = self._device_req
        if device is None:
            device = db.device if db.memspace == _capi.MEM_DEVICE else _default_device()
        d = _capi.Interp3DDesc()
        d.dtype, d.extrapolate, d.device, d.memspace = _capi.F32 if dt == _FLOATS[0] else _capi.F64, int(self._extrapolate), \
            device, db.memspace
        d.nx, d.ny, d.nz = db.shape[0], db.shape[1], db.shape[2]
        lanes = int(np.prod(db.shape[3:], dtype=np.int64))
        d.lanes = lanes
        d.x_len, d.y_len, d.z_len = xb.size, yb.size, zb.size
        d.x, d.y, d.z, d.data = xb.ptr, yb.ptr, zb.ptr, db.ptr
        d.validate = 0   # Interp3DBuilder.build() validated already
        h = C.c_void_p()
        st = self._create_call(d, h)
        if st != _capi.OK:
            raise_builder(st)
        self._h, self._device, self._np_dtype, self._lanes, self._shape = h, device, dt, lanes, tuple(db.shape)
        return self

    def release(self) -> None:
        if self._h is not None:
            _capi.lib().ndi_interp3d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def clone(self, device: int):
        """A replica of this built strategy on `device` (ndi_interp3d_clone): axes and grid are copied device to device."""
        import copy
        h = C.c_void_p()
        st = _capi.lib().ndi_interp3d_clone(self._h, int(device), C.byref(h))
        if st != _capi.OK:
            raise_builder(st)
        other = copy.copy(self)
        other._h, other._device = h, int(device)
        return other

    def interp_array_into(self, interpolator, xs_flat, ys_flat, zs_flat, out2d, *, fresh=False,
                          rows_after_error_unspecified=False):
        """One C-ABI call for the whole batch.  `fresh`: the buffer was allocated for this call and is dropped on Err
        (NDI_EVAL_FRESH_OUTPUT)."""
        q = [Buf(a, self._np_dtype) for a in (xs_flat, ys_flat, zs_flat)]
        if len({b.memspace for b in q}) != 1:
            raise TypeError("xs, ys and zs must live in the same memory space")
        _check_out_dtype(out2d, self._np_dtype)
        opts = _capi.EvalOpts()
        opts.q_memspace = q[0].memspace
        opts.path = _capi.PATH_AUTO
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
            if q[0].memspace == _capi.MEM_DEVICE:
                opts.stream = current_stream_ptr(self._device)
        info = _capi.OobInfo()
        st = _capi.lib().ndi_interp3d_eval(self._h, q[0].ptr, q[1].ptr, q[2].ptr, q[0].size, optr, max(stride, self._lanes),
                                           C.byref(opts), C.byref(info))
        if st != _capi.OK:
            raise_eval(st, info)

    def interp_into(self, interpolator, target, x, y, z):
        out = np.empty((1, self._lanes), dtype=self._np_dtype)
        one = lambda v: np.array([v], dtype=self._np_dtype)   # noqa: E731
        self.interp_array_into(interpolator, one(x), one(y), one(z), out)
        target[...] = out.reshape(target.shape)


class Trilinear(_DeviceStrategy3D):
    """Trilinear strategy on a rectilinear grid (scipy: RegularGridInterpolator(method="linear"); MATLAB: interp3): seven
    `calc_frac` per element in the reference's Bilinear order continued along z, on the device (ndi_interp3d_create /
    ndi_interp3d_eval; include/ndinterp3d.h states the value rule).  Builder and finished strategy in one, like
    `Bilinear`.  f32 / f64 data only."""

    MINIMUM_DATA_LENGHT = 2

    @staticmethod
    def new() -> "Trilinear":
        return Trilinear()

    def _create_call(self, desc, handle) -> int:
        return _capi.lib().ndi_interp3d_create(C.byref(desc), C.byref(handle))


class Tricubic(_DeviceStrategy3D):
    """Tricubic strategy: the tensor-product cubic spline on a rectilinear grid, C2 in each variable (scipy:
    RegularGridInterpolator(method="cubic") with a direct solver, for the default ends), built and evaluated on the device
    (ndi_interp3d_create_tricubic; include/ndinterp3d_cubic.h states the numerical contract).  Seven node-derivative tables
    from seven Bicubic passes, 21 Hermite forms per element.  Three or more knots per axis, f32 / f64 data only; the ends
    are `BoundaryCondition` / `RowBoundary` objects used as `Bicubic` uses them."""

    MINIMUM_DATA_LENGHT = 3

    def __init__(self):
        super().__init__()
        self._bc = [RowBoundary.NotAKnot] * 3   # x, y, z

    @staticmethod
    def new() -> "Tricubic":
        return Tricubic()

    @staticmethod
    def _ends(bc) -> RowBoundary:
        """One axis' (left, right) pair from a BoundaryCondition (NotAKnot / Natural / Clamped) or a RowBoundary."""
        if isinstance(bc, RowBoundary):
            return bc
        if isinstance(bc, BoundaryCondition) and bc.tag in ("NotAKnot", "Natural", "Clamped"):
            return getattr(RowBoundary, bc.tag)
        if isinstance(bc, BoundaryCondition) and bc.tag == "Periodic":
            raise TypeError("Tricubic has no periodic ends: its boundaries are one non-periodic kind per end, and periodic "
                            "axes are not provided in three dimensions")
        if isinstance(bc, BoundaryCondition) and bc.tag == "Individual":
            raise TypeError("Tricubic takes no per-lane (Individual) boundaries: one kind and scalar value per end "
                            "(RowBoundary.Mixed(left, right) gives an axis two different ends)")
        raise TypeError(f"Tricubic boundaries are BoundaryCondition or RowBoundary objects, got {type(bc).__name__}")

    def boundary(self, bc) -> "Tricubic":
        """The same ends on all three axes."""
        self._bc = [self._ends(bc)] * 3
        return self

    def boundary_x(self, bc) -> "Tricubic":
        self._bc[0] = self._ends(bc)
        return self

    def boundary_y(self, bc) -> "Tricubic":
        self._bc[1] = self._ends(bc)
        return self

    def boundary_z(self, bc) -> "Tricubic":
        self._bc[2] = self._ends(bc)
        return self

    def _create_call(self, desc, handle) -> int:
        ends = [e for axis in self._bc for e in (axis.left, axis.right)]
        bc = (_capi.Boundary * 6)(*[_capi.Boundary(int(e.kind), float(e.value)) for e in ends])
        return _capi.lib().ndi_interp3d_create_tricubic(C.byref(desc), bc, C.byref(handle))

    def tables(self, on_device=False):
        """(fx, fy, fz, fxy, fxz, fyz, fxyz): the node derivatives, each of the data's shape (ndi_interp3d_tables), as host
        arrays -- or, with `on_device`, as tensors on the handle's device."""
        if on_device:
            import torch
            out = [torch.empty(self._shape, dtype=torch_dtype(self._np_dtype), device=f"cuda:{self._device}") for _ in range(7)]
            ptrs, space = [t.data_ptr() for t in out], _capi.MEM_DEVICE
        else:
            out = [np.empty(self._shape, dtype=self._np_dtype) for _ in range(7)]
            ptrs, space = [a.ctypes.data for a in out], _capi.MEM_HOST
        st = _capi.lib().ndi_interp3d_tables(self._h, (C.c_void_p * 7)(*ptrs), space)
        if st != _capi.OK:
            from .errors import DeviceError
            raise DeviceError(_capi.last_error())
        return tuple(out)


class Interp3D:
    """Three dimensional interpolator: `data` is interpolated along its first three axes."""

    def __init__(self, x, y, z, data, strategy):
        self.x, self.y, self.z, self.data, self.strategy = x, y, z, data, strategy
        self._x_host, self._y_host, self._z_host = _host(x), _host(y), _host(z)

    @staticmethod
    def builder(data) -> "Interp3DBuilder":
        return Interp3DBuilder.new(data)

    @staticmethod
    def new_unchecked(x, y, z, data, strategy) -> "Interp3D":
        return Interp3D(x, y, z, data, strategy)

    def index_point(self, x_idx: int, y_idx: int, z_idx: int):
        return self._x_host[x_idx], self._y_host[y_idx], self._z_host[z_idx], self.data[x_idx, y_idx, z_idx]

    def get_index_left_of(self, x, y, z):
        def one(k, v):
            r = int(get_lower_index(np.ascontiguousarray(k), np.array([v], dtype=k.dtype))[0])
            if r < 0:
                raise Panic("not implemented: failed to convert NaN to usize")
            return r
        return one(self._x_host, x), one(self._y_host, y), one(self._z_host, z)

    def is_in_x_range(self, x) -> bool:
        return bool(self._x_host[0] <= x <= self._x_host[-1])

    def is_in_y_range(self, y) -> bool:
        return bool(self._y_host[0] <= y <= self._y_host[-1])

    def is_in_z_range(self, z) -> bool:
        return bool(self._z_host[0] <= z <= self._z_host[-1])

    def _lanes_shape(self):
        return tuple(self.data.shape[3:])

    def interp_scalar(self, x, y, z):
        """One point of 3-D data, through the batch call with one query."""
        if len(self.data.shape) != 3:
            raise TypeError("interp_scalar needs 3-D data; use interp()")
        buf = np.zeros((), dtype=np_dtype_of(self.data))
        self.strategy.interp_into(self, buf, x, y, z)
        return buf[()]

    def interp(self, x, y, z):
        target = np.zeros(self._lanes_shape(), dtype=np_dtype_of(self.data))
        self.strategy.interp_into(self, target, x, y, z)
        return target

    def get_buffer_shape(self, q_shape):
        return tuple(q_shape) + self._lanes_shape()

    @staticmethod
    def _check_shapes(xs, ys, zs):
        if not (tuple(xs.shape) == tuple(ys.shape) == tuple(zs.shape)):
            raise ValueError(f"xs, ys and zs need equal shapes, got {tuple(xs.shape)}, {tuple(ys.shape)}, {tuple(zs.shape)}")

    def interp_array(self, xs, ys, zs):
        """`out[q] = f(xs[q], ys[q], zs[q])` for queries of any rank; the result has the shape `xs.shape + data.shape[3:]`.
        Host arrays give a numpy array, device tensors a tensor."""
        self._check_shapes(xs, ys, zs)
        shape = self.get_buffer_shape(tuple(xs.shape))
        dt = np_dtype_of(self.data)
        if is_torch(xs) and xs.is_cuda:
            import torch
            out = torch.empty(shape, dtype=torch_dtype(dt), device=xs.device)
        else:
            out = np.zeros(shape, dtype=dt)
        # the buffer is this call's own and is dropped on Err: strategies that can use the knowledge are told
        self.interp_array_into(xs, ys, zs, out, **({"fresh": True} if getattr(self.strategy, "_takes_fresh", False) else {}))
        return out

    def interp_array_into(self, xs, ys, zs, buffer, **kw):
        """Rows before the first failing query are written; the failing row and all later rows stay untouched (unless
        `fresh` / `rows_after_error_unspecified` give them up)."""
        self._check_shapes(xs, ys, zs)
        expect = self.get_buffer_shape(tuple(xs.shape))
        if tuple(buffer.shape) != expect:
            raise Panic(f"ShapeError/IncompatibleShape: incompatible shapes expected: {list(expect)}, "
                        f"got: {list(buffer.shape)}")
        if np_dtype_of(buffer) != np_dtype_of(self.data):
            raise TypeError(f"buffer has element type {np_dtype_of(buffer)}, the data is {np_dtype_of(self.data)}")
        nq = int(np.prod(xs.shape, dtype=np.int64))
        lanes = int(np.prod(self._lanes_shape(), dtype=np.int64))
        qf = [q.reshape(-1) for q in (xs, ys, zs)]
        if is_torch(buffer):
            if not buffer.is_contiguous():
                raise TypeError("device output buffers must be contiguous")
            self.strategy.interp_array_into(self, *qf, buffer.view(nq, lanes), **kw)
            return
        if not is_torch(xs):
            qf = [_host(q) for q in qf]
        if buffer.flags.c_contiguous:
            self.strategy.interp_array_into(self, *qf, buffer.reshape(nq, lanes), **kw)
            return
        tmp = np.zeros((nq, lanes), dtype=np_dtype_of(self.data))
        done = nq
        try:
            self.strategy.interp_array_into(self, *qf, tmp, **kw)
        except (InterpolateError.OutOfBounds, Panic) as e:
            done = e.index if getattr(e, "index", None) is not None else 0
            raise
        except BaseException:
            done = 0
            raise
        finally:
            if done and len(xs.shape) == 0:
                buffer[...] = tmp[0].reshape(buffer.shape)
            elif done:
                where = np.unravel_index(np.arange(done), tuple(xs.shape))
                buffer[where] = tmp[:done].reshape((done,) + self._lanes_shape())

    def replicate(self, devices):
        """Replicas of this interpolator on the given devices (ndi_interp3d_clone)."""
        if not hasattr(self.strategy, "clone"):
            raise TypeError("replicate needs the built-in device strategy")
        return [Interp3D(self.x, self.y, self.z, self.data, self.strategy.clone(d)) for d in devices]


class Interp3DBuilder:
    """Create and configure an `Interp3D` interpolator; the checks and their order are Interp2DBuilder's with a third
    axis."""

    def __init__(self, data, x=None, y=None, z=None, strategy=None):
        self._data, self._x, self._y, self._z = data, x, y, z
        self._strategy = strategy if strategy is not None else Trilinear.new()

    @staticmethod
    def new(data) -> "Interp3DBuilder":
        return Interp3DBuilder(data)

    def strategy(self, strategy) -> "Interp3DBuilder":
        return Interp3DBuilder(self._data, self._x, self._y, self._z, strategy)

    def x(self, x) -> "Interp3DBuilder":
        return Interp3DBuilder(self._data, x, self._y, self._z, self._strategy)

    def y(self, y) -> "Interp3DBuilder":
        return Interp3DBuilder(self._data, self._x, y, self._z, self._strategy)

    def z(self, z) -> "Interp3DBuilder":
        return Interp3DBuilder(self._data, self._x, self._y, z, self._strategy)

    def build(self) -> Interp3D:
        data, strategy = self._data, self._strategy
        shape = tuple(data.shape)
        if len(shape) < 3:
            raise BuilderError.ShapeError("data dimension needs to be at least 3")
        need = strategy.MINIMUM_DATA_LENGHT
        for a in range(3):
            if shape[a] < need:
                raise BuilderError.NotEnoughData(
                    f"The {a}-dimension has not enough data for the chosen interpolation strategy. "
                    f"Provided: {shape[a]}, Reqired: {need}")
        dt = np_dtype_of(data)
        axes = [_default_axis(shape[a], dt) if k is None else k for a, k in enumerate((self._x, self._y, self._z))]
        for a, (name, k) in enumerate(zip("xyz", axes)):
            k_len = int(np.prod(k.shape, dtype=np.int64))
            if k_len != shape[a]:
                raise BuilderError.ShapeError(
                    f"Lenghts of {name}-axis and data-{a}-axis need to match. Got {name}: {k_len}, data-{a}: {shape[a]}")
        for name, k in zip("xyz", axes):
            if monotonic_prop(k) != Monotonic.Rising(True):
                raise BuilderError.Monotonic(f"The {name}-axis needs to be strictly monotonic rising")
        finished = strategy.build(axes[0], axes[1], axes[2], data)
        return Interp3D(axes[0], axes[1], axes[2], data, finished)
