"""Array plumbing between numpy / torch and the C ABI (pointers + memory space)."""
from __future__ import annotations

import numpy as np

from . import _capi

try:  # torch is plumbing for device memory and streams only
    import torch
except Exception:  # pragma: no cover
    torch = None


def is_torch(a) -> bool:
    return torch is not None and isinstance(a, torch.Tensor)


# numpy has no bfloat16: the mirror names it by a 2-byte structured dtype of its own (never used to hold values; bf16
# data and results travel as torch.bfloat16 tensors)
BF16 = np.dtype([("bfloat16", "<u2")])
_NP2ID = {np.dtype(np.float32): _capi.F32, np.dtype(np.float64): _capi.F64,
          np.dtype(np.int32): _capi.I32, np.dtype(np.int64): _capi.I64,
          np.dtype(np.float16): _capi.F16, BF16: _capi.BF16}
DEVICE_INT_DTYPES = (np.dtype(np.int32), np.dtype(np.int64))   # Linear / Bilinear only
DEVICE_HALF_DTYPES = (np.dtype(np.float16), BF16)               # Linear / Bilinear only


def torch_dtype(dt):
    """The torch dtype of a device element type (None for the others)."""
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
            np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
            np.dtype(np.float16): torch.float16, BF16: torch.bfloat16}.get(np.dtype(dt))


def np_dtype_of(a):
    if is_torch(a):
        return {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64),
                torch.bfloat16: BF16}.get(a.dtype) or np.dtype(str(a.dtype).replace("torch.", ""))
    return np.asarray(a).dtype


def is_bf16(dt) -> bool:
    return dt is not None and np.dtype(dt) == BF16


def as_bf16_source(a):
    """Values headed for a bf16 buffer, as a torch.bfloat16 tensor on the source's device: every value rounded to bf16
    ONCE, to nearest with ties to even (what numpy does for f16).  bf16, f16 and f32 sources are rounded by torch's
    f32 -> bf16 conversion; everything else goes through f64 (exact for integers up to 2^53) and is rounded to odd in
    f32 first -- torch's f64 -> bf16 conversion would round to nearest twice -- which makes the second rounding the
    single correct one (f32 keeps 24 >= 8 + 2 significand bits, down to bf16's subnormals)."""
    t = a if is_torch(a) else torch.as_tensor(np.ascontiguousarray(a))
    if t.dtype in (torch.bfloat16, torch.float16, torch.float32):
        return t.to(torch.bfloat16)
    t = t.to(torch.float64)
    f = t.to(torch.float32)                       # to nearest (inf beyond the f32 range)
    back = f.to(torch.float64)
    inexact = back != t                           # NaN counts as inexact; it stays NaN below
    f = torch.where(inexact & (back.abs() > t.abs()), torch.nextafter(f, torch.zeros_like(f)), f)   # toward zero
    bits = f.view(torch.int32)
    bits = torch.where(inexact, bits | 1, bits)   # round to odd: the sticky bit
    return bits.view(torch.float32).to(torch.bfloat16)


def dtype_id(dt) -> int:
    dt = np.dtype(dt)
    if dt not in _NP2ID:
        raise TypeError(f"the MI355X path covers float32/float64 (and int32/int64 for Linear / Bilinear), got {dt} "
                        "(other element types stay on the host's generic per-query path)")
    return _NP2ID[dt]


class Buf:
    """A contiguous buffer handed to the C ABI: pointer, memory space and a keep-alive."""

    def __init__(self, arr, dt=None):
        if is_bf16(dt):
            arr = as_bf16_source(arr)
        if is_torch(arr):
            if dt is not None and np.dtype(dt) in DEVICE_INT_DTYPES and arr.dtype != torch_dtype(dt):
                _check_int_values(arr, dt)
            t = arr if dt is None else arr.to(torch_dtype(dt))
            t = t.contiguous()
            self.keep = t
            self.shape = tuple(t.shape)
            self.size = t.numel()
            if t.is_cuda:
                self.memspace = _capi.MEM_DEVICE
                self.device = t.device.index if t.device.index is not None else torch.cuda.current_device()
                self.ptr = t.data_ptr()
            else:
                self.memspace = _capi.MEM_HOST
                self.device = None
                self.ptr = t.data_ptr()
            self.np_dtype = np_dtype_of(t)
        else:
            if dt is not None and np.dtype(dt) in DEVICE_INT_DTYPES and np.asarray(arr).dtype != np.dtype(dt):
                _check_int_values(np.asarray(arr), dt)
            a = np.ascontiguousarray(arr, dtype=dt)
            self.keep = a
            self.shape = a.shape
            self.size = a.size
            self.memspace = _capi.MEM_HOST
            self.device = None
            self.ptr = a.ctypes.data
            self.np_dtype = a.dtype


def _check_int_values(a, dt):
    """Values converted to an integer element type must be values of it (the reference's query type IS the element
    type): the same TypeError as generic_host._scalar -- "not a value of" for NaN / infinite / fractional values, "out
    of range for" for values outside T -- instead of a silent truncation or wrap.  Vectorised; numpy arrays and torch
    tensors (on either device).  Sources whose every value fits T (narrower integers, bool) pass unchecked."""
    from .generic_host import _scalar
    info = np.iinfo(dt)
    lo, hi_excl = float(info.min), -float(info.min)          # -2^(w-1) and 2^(w-1): exact in float64
    if is_torch(a):
        if a.dtype == torch.bool:
            return
        if a.is_floating_point():
            bad = ~torch.isfinite(a) | (a != torch.trunc(a)) | (a < lo) | (a >= hi_excl)
        elif not a.is_complex():
            si = torch.iinfo(a.dtype)
            if si.min >= info.min and si.max <= info.max:
                return
            bad = (a < int(info.min)) | (a > int(info.max))
        else:
            raise TypeError(f"queries of element type {a.dtype} are not values of {np.dtype(dt)}")
        flat = bad.reshape(-1)
        if not bool(flat.any()):
            return
        v = a.reshape(-1)[int(torch.nonzero(flat)[0])].cpu().numpy()[()]    # a numpy scalar, as the host loop sees
    else:
        a = np.asarray(a)
        if a.dtype.kind == "b":
            return
        if a.dtype.kind in "iu":
            si = np.iinfo(a.dtype)
            if si.min >= info.min and si.max <= info.max:
                return
            bad = (a < int(info.min)) | (a > int(info.max))
        elif a.dtype.kind == "f":
            with np.errstate(invalid="ignore"):
                bad = ~np.isfinite(a) | (a != np.trunc(a)) | (a < lo) | (a >= hi_excl)
        else:
            for v in a.reshape(-1):                              # object arrays: element by element
                _scalar(v, dt)
            return
        flat = bad.reshape(-1)
        if not flat.any():
            return
        v = a.reshape(-1)[int(np.argmax(flat))]
    _scalar(v, dt)
    raise TypeError(f"query {v!r} is not a value of the element type {np.dtype(dt)}")


def int_query(dt, bufs, info):
    """For an integer element type: a callable axis -> the failing query's coordinate as a Python int (read from the
    query buffer itself: ndi_oob_info.value is a double, lossy for i64 beyond 2^53); None for float types."""
    if np.dtype(dt) not in DEVICE_INT_DTYPES:
        return None

    def q(axis):
        if not bufs:
            return int(info.value)
        b = bufs[min(axis, len(bufs) - 1)].keep
        return int(b.reshape(-1)[int(info.index)].item() if is_torch(b) else b.reshape(-1)[int(info.index)])
    return q


def current_stream_ptr(device: int):
    if torch is None or not torch.cuda.is_available():
        return None
    return torch.cuda.current_stream(device).cuda_stream



def striped_ring(chunk_queries: int, lanes: int, n_slots: int, dtype=np.float64, device: int = 0):
    """The recommended ring layout on MI355X (include/ndinterp.h): ONE device allocation with the
    slots interleaved row by row.  Returns `n_slots` views of shape (chunk_queries, lanes) whose rows are
    contiguous and `n_slots * lanes` elements apart -- every chunk's output stream then covers the whole ring's
    physical extent instead of one 1/n_slots part of it."""
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)]
    base = torch.empty((chunk_queries, n_slots, lanes), dtype=tdt, device=f"cuda:{device}")
    return [base[:, s, :] for s in range(n_slots)]


class _OwnedOutput:
    """A buffer from ndi_output_alloc exposed through __cuda_array_interface__: torch.as_tensor() wraps it without a copy
    and keeps this object alive; the buffer goes back with ndi_output_free when the last tensor over it is gone."""

    def __init__(self, shape, dtype, device, max_tries=0, zeroed=True):
        import ctypes
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.device = int(device)
        nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        ptr = ctypes.c_void_p()
        self.info = _capi.OutputInfo()
        st = _capi.lib().ndi_output_alloc(self.device, nbytes, int(max_tries),
                                          _capi.OUTPUT_ZEROED if zeroed else _capi.OUTPUT_UNINITIALIZED,
                                          ctypes.byref(ptr), ctypes.byref(self.info))
        if st != _capi.OK:
            from .errors import DeviceError
            raise DeviceError(_capi.last_error())
        self.ptr = ptr.value
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False),
                                         "version": 2, "strides": None}

    def __del__(self):
        p, self.ptr = getattr(self, "ptr", None), None
        if p:
            try:
                _capi.lib().ndi_output_free(p)
            except Exception:   # interpreter shutdown
                pass


OUTPUT_OWNED_MIN_BYTES = 1 << 30


def output_trim() -> None:
    """Release the output buffers ndi_output_free keeps for reuse (ndi_output_trim)."""
    _capi.lib().ndi_output_trim()


def output_empty(shape, dtype=np.float64, device: int = 0, max_tries: int = 0, zeroed: bool = False):
    """A library-owned device output buffer (ndi_output_alloc: the allocation of interp_array, interp1d/mod.rs:209, with the
    placement check of include/ndinterp.h) as a torch tensor of `shape`.  `tensor.ndi_output_info` tells how many candidates
    were tried and the fill rate of the one kept.  Contents unspecified (NDI_OUTPUT_UNINITIALIZED: a buffer kept by
    ndi_output_free comes back without a refill -- interp_array overwrites every row or drops the buffer); `output_zeros`
    is the reference's Array::zeros."""
    own = _OwnedOutput(shape, dtype, device, max_tries, zeroed)
    with torch.cuda.device(device):
        t = torch.as_tensor(own, device=f"cuda:{device}")
    t.ndi_output_info = {"tries": own.info.tries, "fill_TBps": round(own.info.fill_tbps, 3),
                         "worst_fill_TBps": round(own.info.worst_fill_tbps, 3), "alloc_ms": round(own.info.alloc_ms, 2)}
    return t


def output_zeros(shape, dtype=np.float64, device: int = 0, max_tries: int = 0):
    """`output_empty` filled with zeros: Array::zeros (interp1d/mod.rs:209)."""
    return output_empty(shape, dtype, device, max_tries, zeroed=True)
