"""f16 / bf16 element types at the C ABI, without a device: the dtype enumerators (header and Rust shim), the builder
checks that run before any device work, the refusal of half-precision splines, and the numpy restatement of the
`half` crate's arithmetic that tests/test_gpu_half.py compares the device against (checked here against torch)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def bf16_round(a):
    """f32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN (quiet)."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return np.where(nan, (b >> 16) | 0x40, r).astype(np.uint16)


def bf16_value(bits):
    """bf16 bit patterns -> their f32 values (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def test_header_and_rust_shim_declare_half_enumerators():
    h = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    for name, val in (("NDI_F16", 4), ("NDI_BF16", 5)):
        assert re.search(rf"\b{name}\s*=\s*{val}\b", h), name
        assert re.search(rf"pub const {name}: i32 = {val};", rs), name


def _half_bits(v, bf16):
    a = np.asarray(v, dtype=np.float32)
    return bf16_round(a) if bf16 else a.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("bf16", [False, True])
def test_validate_on_half_knots(pkg, bf16):
    lib = pkg._capi.lib()
    dt = pkg._capi.BF16 if bf16 else pkg._capi.F16
    rising = _half_bits([0.0, 0.5, 1.0, 3.0], bf16)
    equal = _half_bits([0.0, 0.5, 0.5, 3.0], bf16)
    nan = _half_bits([0.0, np.nan, 1.0, 3.0], bf16)
    lin = pkg._capi.LINEAR
    assert lib.ndi_validate1d(dt, rising.ctypes.data, 4, 4, lin) == pkg._capi.OK
    assert lib.ndi_validate1d(dt, equal.ctypes.data, 4, 4, lin) == pkg._capi.MONOTONIC
    assert lib.ndi_validate1d(dt, nan.ctypes.data, 4, 4, lin) == pkg._capi.MONOTONIC
    assert lib.ndi_validate1d(dt, rising.ctypes.data, 4, 3, lin) == pkg._capi.SHAPE
    assert lib.ndi_validate2d(dt, rising.ctypes.data, 4, rising.ctypes.data, 4, 4, 4) == pkg._capi.OK
    assert lib.ndi_validate2d(dt, rising.ctypes.data, 4, equal.ctypes.data, 4, 4, 4) == pkg._capi.MONOTONIC
    assert lib.ndi_validate2d(dt, nan.ctypes.data, 4, rising.ctypes.data, 4, 4, 4) == pkg._capi.MONOTONIC
    # values that are distinct in f32 but equal in T are equal neighbours on T
    close = _half_bits([0.0, 1.0, 1.0 + 2.0 ** -12, 2.0], bf16)
    assert lib.ndi_validate1d(dt, close.ctypes.data, 4, 4, lin) == pkg._capi.MONOTONIC


@pytest.mark.parametrize("bf16", [False, True])
def test_half_spline_is_refused_before_any_device_work(pkg, bf16):
    lib = pkg._capi.lib()
    x = _half_bits([0.0, 1.0, 2.0, 3.0], bf16)
    y = _half_bits([0.0, 1.0, 4.0, 9.0], bf16)
    d = pkg._capi.Interp1DDesc()
    d.dtype = pkg._capi.BF16 if bf16 else pkg._capi.F16
    d.strategy = pkg._capi.CUBIC_SPLINE
    d.n, d.lanes, d.x_len = 4, 1, 4
    d.x, d.data, d.memspace, d.validate = x.ctypes.data, y.ctypes.data, pkg._capi.MEM_HOST, 1
    h = ctypes.c_void_p()
    assert lib.ndi_interp1d_create(ctypes.byref(d), ctypes.byref(h)) == pkg._capi.BAD_ARG
    assert "CubicSpline" in pkg._capi.last_error()
    d.dtype = 6   # values from 6 up stay invalid
    d.strategy = pkg._capi.LINEAR
    assert lib.ndi_interp1d_create(ctypes.byref(d), ctypes.byref(h)) == pkg._capi.BAD_ARG


def test_mirror_refuses_half_splines(pkg):
    import torch
    with pytest.raises(TypeError):
        pkg.CubicSpline.new().build(np.arange(4.0).astype(np.float16), np.arange(4.0).astype(np.float16))
    with pytest.raises(TypeError, match="^CubicSpline covers float32/float64 only, got bfloat16$"):
        pkg.CubicSpline.new().build(torch.arange(4.0).to(torch.bfloat16), torch.arange(4.0).to(torch.bfloat16))


def test_bf16_dtype_plumbing_without_a_device(pkg):
    import torch
    a = pkg._arrays
    t = torch.tensor([1.0, 2.5], dtype=torch.bfloat16)
    assert a.np_dtype_of(t) == a.BF16 and a.dtype_id(a.BF16) == pkg._capi.BF16
    assert a.torch_dtype(a.BF16) == torch.bfloat16 and a.dtype_id(np.float16) == pkg._capi.F16
    b = a.Buf(np.array([1.0, 1.0 + 2.0 ** -9, 3.0]), a.BF16)   # numpy in: torch rounds to bf16
    assert b.memspace == pkg._capi.MEM_HOST and b.keep.dtype == torch.bfloat16
    assert b.keep.view(torch.int16).numpy().view(np.uint16).tolist() == bf16_round([1.0, 1.0, 3.0]).tolist()
    assert pkg.monotonic_prop(torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -9], dtype=torch.bfloat16)) != \
        pkg.Monotonic.Rising(True)


def test_bf16_rounding_helper_matches_torch():
    import torch
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                         1.0 + 2.0 ** -8 + 2.0 ** -20, 3.3895313892515355e38, 3.3961e38, 3.4e38,
                         np.finfo(np.float32).max, 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -126, 9.18e-41],
                        dtype=np.float32)
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, 1 << 24, dtype=np.uint64).astype(np.uint32)
    for a in (specials, bits.view(np.float32)):
        ours = bf16_round(a)
        ref = torch.from_numpy(a.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        nan = np.isnan(a)
        assert np.array_equal(ours[~nan], ref[~nan])
        assert np.all(np.isnan(bf16_value(ours[nan]))) and np.all(np.isnan(bf16_value(ref[nan])))


@pytest.mark.parametrize("bf16", [False, True])
def test_monotonic_prop_on_half_values(pkg, bf16):
    lib = pkg._capi.lib()
    dt = pkg._capi.BF16 if bf16 else pkg._capi.F16
    for v, want in (([1.0, 2.0, 3.0], 1), ([1.0, 2.0, 2.0], 2), ([3.0, 2.0, 1.0], 3), ([3.0, 3.0, 1.0], 4),
                    ([1.0, 3.0, 2.0], 0), ([5.0, 5.0], 0), ([0.0, np.nan, 1.0], 0), ([-np.inf, 0.0, np.inf], 1)):
        a = _half_bits(v, bf16)
        assert lib.ndi_monotonic_prop(dt, a.ctypes.data, len(a)) == want, v


def test_bf16_queries_are_rounded_once(pkg):
    """Python numbers and f64 arrays reach bf16 with ONE round-to-nearest-even (as numpy rounds f64 to f16); going
    through f32 first would round twice."""
    import torch
    a = pkg._arrays
    v = np.array([1 + 2.0 ** -8 + 2.0 ** -30, -(1 + 2.0 ** -8 + 2.0 ** -30), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,
                  3.4e38, 1e300, -np.inf, -0.0, 1e-40, 2.0 ** -134 + 2.0 ** -160, 2.0 ** 40 + 1, 5e-324])
    want = [0x3F81, 0xBF81, 0x3F80, 0x3F82, 0x7F80, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x0001, 0x5380, 0x0000]
    for src in (v, torch.as_tensor(v), list(v)):
        got = a.Buf(src, a.BF16).keep.view(torch.int16).numpy().view(np.uint16)
        assert got.tolist() == want
    got = a.Buf(np.array([2 ** 40 + 2 ** 32 + 1], np.int64), a.BF16).keep.view(torch.int16).numpy().view(np.uint16)
    assert got.tolist() == [0x5381]   # integers: one rounding too
    assert np.isnan(a.Buf(np.array([np.nan]), a.BF16).keep.float().numpy()).all()


def test_f16_kernel_divides_in_f32(tmp_path):
    """Linear::calc_frac's division must be the correctly rounded f32 one followed by the RNE conversion.  For f16 the
    compiler would otherwise narrow fptrunc(fdiv(fpext a, fpext b)) to its f16 division lowering (an approximate
    reciprocal with a fix-up): the gfx950 code of the f16 kernel must hold the f32 division sequence and no f16 one."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "probe.hip"
    src.write_text("""#include <hip/hip_runtime.h>
#include <stdint.h>
namespace ndi {
constexpr int BLOCK = 256;
enum ExtrapMode : int { EX_NO = 0, EX_YES = 1 };
enum BoundsCode : int { BC_INTERVAL = 1, BC_CELL_X = 5, BC_CELL_Y = 6 };
}
#define NDI_CHK(idx, lim, code) (idx)
#include "half_kernels.hpp"
template __global__ void ndi::half_eval1d_kernel<ndi::HF_F16, false, false, false>(const uint16_t*, uint64_t,
    const float*, uint32_t, int, ndi::HalfBounds, bool, const uint16_t*, uint64_t, uint16_t*, uint64_t, uint32_t,
    const unsigned long long*, unsigned long long*);
""")
    asm = tmp_path / "probe.s"
    flags = ["-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]   # csrc/Makefile
    subprocess.run([hipcc, "--offload-arch=gfx950", *flags, "--cuda-device-only", "-S", "-I",
                    os.path.join(ROOT, "ndarray-interp_amd", "csrc"), str(src), "-o", str(asm)],
                   check=True, capture_output=True, timeout=600)
    isa = asm.read_text()
    for op in ("v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32"):
        assert op in isa, op
    assert "v_div_fixup_f16" not in isa and "v_rcp_f16" not in isa
