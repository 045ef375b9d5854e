"""i32 / i64 element types at the C ABI, without a device: dtype enumerators, the builder checks that run before any
device work, the refusal of integer splines, ndi_monotonic_prop, and the magic-number division the integer Bilinear
kernels use (csrc/int_divide.hpp, compiled for the host from the same source the kernels include)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT


def _desc(pkg, dtype, x, y, strategy=None):
    d = pkg._capi.Interp1DDesc()
    d.dtype = dtype
    d.strategy = pkg._capi.LINEAR if strategy is None else strategy
    d.n, d.lanes, d.x_len = len(y), 1, len(x)
    d.x, d.data, d.memspace, d.validate = x.ctypes.data, y.ctypes.data, pkg._capi.MEM_HOST, 1
    return d


def test_header_declares_integer_enumerators():
    h = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    for name, val in (("NDI_I32", 2), ("NDI_I64", 3), ("NDI_INT_OVERFLOW", 10), ("NDI_OP_SUBTRACT", 0),
                      ("NDI_OP_MULTIPLY", 1), ("NDI_OP_ADD", 2), ("NDI_OP_DIVIDE", 3)):
        assert re.search(rf"\b{name}\s*=\s*{val}\b", h), name


def test_integer_builder_checks_need_no_device(pkg):
    lib = pkg._capi.lib()
    h = ctypes.c_void_p()
    for dtype, npt in ((pkg._capi.I32, np.int32), (pkg._capi.I64, np.int64)):
        x = np.array([1, 2, 2], dtype=npt); y = np.array([1, 2, 3], dtype=npt)
        d = _desc(pkg, dtype, x, y)
        assert lib.ndi_interp1d_create(ctypes.byref(d), ctypes.byref(h)) == pkg._capi.MONOTONIC
        assert "strictly monotonic rising" in pkg._capi.last_error()
        assert lib.ndi_validate1d(dtype, x.ctypes.data, 3, 3, pkg._capi.LINEAR) == pkg._capi.MONOTONIC
        x2 = np.array([1, 2, 3], dtype=npt)
        assert lib.ndi_validate1d(dtype, x2.ctypes.data, 3, 2, pkg._capi.LINEAR) == pkg._capi.SHAPE
        g = np.array([0, 1], dtype=npt)
        assert lib.ndi_validate2d(dtype, g.ctypes.data, 2, x.ctypes.data, 3, 2, 3) == pkg._capi.MONOTONIC
    d = pkg._capi.Interp1DDesc()
    d.dtype = 7
    assert lib.ndi_interp1d_create(ctypes.byref(d), ctypes.byref(h)) == pkg._capi.BAD_ARG


def test_integer_spline_is_refused_with_a_message(pkg):
    lib = pkg._capi.lib()
    h = ctypes.c_void_p()
    x = np.array([0, 1, 2, 3], dtype=np.int32); y = np.array([0, 1, 4, 9], dtype=np.int32)
    d = _desc(pkg, pkg._capi.I32, x, y, pkg._capi.CUBIC_SPLINE)
    assert lib.ndi_interp1d_create(ctypes.byref(d), ctypes.byref(h)) == pkg._capi.BAD_ARG
    assert "CubicSpline" in pkg._capi.last_error() and "integer" in pkg._capi.last_error()


def test_monotonic_prop_on_integers(pkg):
    lib = pkg._capi.lib()
    cases = [([1, 2, 3], 1), ([1, 2, 2], 2), ([3, 2, 1], 3), ([3, 3, 1], 4), ([1, 3, 2], 0), ([5, 5], 0),
             ([-2**62, 0, 2**62], 1), ([2**63 - 1, -2**63], 3)]
    for v, want in cases:
        a = np.array(v, dtype=np.int64)
        assert lib.ndi_monotonic_prop(pkg._capi.I64, a.ctypes.data, len(a)) == want, v
        if all(-2**31 <= e < 2**31 for e in v):
            b = np.array(v, dtype=np.int32)
            assert lib.ndi_monotonic_prop(pkg._capi.I32, b.ctypes.data, len(b)) == want, v


def test_magic_division_equals_truncating_division(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_int_divide.cpp")
    inc = os.path.join(ROOT, "ndarray-interp_amd", "csrc")
    exe = str(tmp_path / "test_int_divide")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", inc, "-o", exe, src], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_values_converted_to_an_integer_element_type_are_checked(pkg):
    """Queries reaching an i32 / i64 device interpolator are converted to T: a value of a wider or unsigned integer
    type outside T, or a NaN / infinite / fractional float, is refused with generic_host's TypeError instead of
    wrapping or truncating (numpy arrays and CPU torch tensors; no device needed)."""
    import pytest
    import torch
    Buf = pkg._arrays.Buf
    cases = [(np.array([1, 2**32 + 1], np.int64), np.int32, "out of range"),
             (np.array([2**63 + 5], np.uint64), np.int64, "out of range"),
             (np.array([-1, 2**31], np.int64), np.int32, "out of range"),
             (np.array([1.0, 2.5]), np.int64, "not a value"),
             (np.array([np.inf]), np.int32, "not a value"),
             (np.array([3e10]), np.int32, "out of range"),
             (np.array([2.0**63]), np.int64, "out of range")]
    for a, dt, what in cases:
        with pytest.raises(TypeError, match=what):
            Buf(a, dt)
        if a.dtype != np.uint64:
            with pytest.raises(TypeError, match=what):
                Buf(torch.as_tensor(a), dt)
    for a, dt in ((np.array([-2**31, 2**31 - 1], np.int64), np.int32), (np.array([1.0, -7.0]), np.int32),
                  (np.array([5], np.int16), np.int64), (np.array([True]), np.int32)):
        assert Buf(a, dt).keep.tolist() == a.astype(dt).tolist()
        assert Buf(torch.as_tensor(a), dt).keep.tolist() == a.astype(dt).tolist()
