"""CPU: inverse handles at the boundary -- the new entry point in the header, the ctypes binding, the built library (and
its bounds-checked build's sources) and the Rust declaration; the refusals that need no handle and no device; the Python
mirror's refusals, decided before the library is reached; and the header's statement of the numerical contract against
the operations of tests/inverse_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import inverse_ref
from conftest import ROOT

RULE_LINES = (
    "search   lo = 0, hi = n-1;  while hi - lo > 1:  mid = (lo + hi) >> 1",
    "if (rising ? c[mid] <= v : c[mid] >= v) lo = mid else hi = mid",
    "i = lo;  nl = c[i], nr = c[i+1];  xl = x[i], xr = x[i+1];  dx = xr - xl",
    "start    if v == nl:  t = 0",
    "t = (v - nl) / (nr - nl)",
    "solve    tl = 0, th = 1, dprev = 1;   repeat at most K times:",
    "f = p(t) - v;            if f == 0: stop",
    "if (rising ? f < 0 : f > 0) tl = t else th = t",
    "d = p'(t);  s = f / d;  tn = t - s",
    "if !(tn > tl && tn < th) or !(|s + s| <= |dprev|):  tn = tl + 0.5 * (th - tl)",
    "step = tn - t;  dprev = step;  t = tn",
    "if |step| <= eps_T: stop",
    "eps_T = 2^-52 (f64) / 2^-23 (f32)",
    "finish   w = xl + t * dx;  x = (t == 1) ? xr : min(w, xr)",
    "p(t)  = ((1-t) yl + t yr) + (t (1-t)) (a (1-t) + b t)",
    "p'(t) = (dy + a) + t (((b - (a+a)) + (b - (a+a))) - (3 (b - a)) t)",
    "p(t)  = P[i] + dx * (t (yl + t (c1 + t (c2 - t c3))))",
    "p'(t) = dx * (yl + t ((c1 + c1) + t (3 c2 - (4 c3) t)))",
    "p(t)  = P[i] + dx * (t (yl + t c1))",
    "p'(t) = dx * (yl + t (c1 + c1))",
    "K = 128 (f64) / 64 (f32)",
    "rising = N[n-1][l] >= N[0][l]",
    "Lo = max_l min(N[0][l], N[n-1][l]) and Hi = min_l max(N[0][l], N[n-1][l])",
    "`extrapolate` of the source is IGNORED",
    "the returned x is in [xl, xr]",
    "falls into the bisection branch",
    "the run's right end is returned",
)


def test_header_capi_library_and_rust_carry_the_symbol(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    assert re.search(r"ndi_status ndi_interp1d_inverse\(const ndi_interp1d\* h, ndi_interp1d\*\* out\);", header)
    for text in RULE_LINES:
        assert text in header, text
    lib = C.CDLL(cap.LIB_PATH)
    assert "ndi_interp1d_inverse" in cap.SYMBOLS and hasattr(lib, "ndi_interp1d_inverse")
    # the ctypes prototype is the header's: a handle pointer in, a handle pointer out, ndi_status back
    res, args = cap.SYMBOLS["ndi_interp1d_inverse"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_void_p)]
    assert cap.SYMBOLS["ndi_interp1d_inverse"] == cap.SYMBOLS["ndi_interp1d_antiderivative"]
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    assert "pub fn ndi_interp1d_inverse(h: *const ndi_interp1d, out: *mut *mut ndi_interp1d) -> i32;" in rust
    assert cap.lib().ndi_version() == (0 << 16) | 5     # one new symbol, no new enumerator: no version change
    assert issubclass(pkg.InverseStrategy, pkg.Interp1DStrategy)
    for name in ("interp_array_into", "finish", "clone", "data_table", "trim", "release", "inverse"):
        assert callable(getattr(pkg.InverseStrategy, name)), name
    assert callable(pkg.Interp1D.inverse) and callable(pkg.AntiderivativeStrategy.inverse)
    assert pkg.AntiderivativeStrategy.inverse is pkg.Linear.inverse           # allowed: the shared one, not a refusal
    assert inverse_ref.K == {np.dtype(np.float64): 128, np.dtype(np.float32): 64}
    assert inverse_ref.EPS[np.dtype(np.float64)] == 2.0 ** -52 and inverse_ref.EPS[np.dtype(np.float32)] == 2.0 ** -23


def test_argument_validation_needs_no_device(pkg):
    """the refusals that need no handle come back with their status and message whether or not a device is present"""
    cap, lib = pkg._capi, pkg._capi.lib()
    h = C.c_void_p(1234)
    assert lib.ndi_interp1d_inverse(None, C.byref(h)) == cap.BAD_ARG
    assert cap.last_error() == "null handle" and h.value is None       # *out is cleared first
    assert lib.ndi_interp1d_inverse(None, None) == cap.BAD_ARG and cap.last_error() == "null out pointer"


def test_every_handle_kind_refuses_with_a_message_that_names_it():
    """the refusals that need a handle are decided by the handle's own inverse(), before any device work: every kind of
    1-D handle has one, and its message names the strategy and the reason (the GPU tests see them come back)"""
    csrc = os.path.join(ROOT, "ndarray-interp_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("int_host.hpp", "half_host.hpp", "inverse_host.hpp")}
    assert "inverse: an integer handle is a Linear interpolator of a narrow element type" in text["int_host.hpp"]
    assert "inverse: an f16 / bf16 handle is a Linear interpolator of a narrow element type" in text["half_host.hpp"]
    assert "inverse of %s: the Periodic extrapolation mode has no inverse handle" in text["inverse_host.hpp"]
    assert "inverse: this handle is already the inverse of %s" in text["inverse_host.hpp"]
    # each refusal returns before the first device call of its function
    body = text["inverse_host.hpp"]
    fn = body[body.index("ndi_status Interp1DImpl<T>::inverse("):]
    assert fn.index("EX_PERIODIC") < fn.index("inverse_create<T>(")


def test_mirror_refuses_strategies_without_a_handle(pkg):
    class Mine(pkg.Interp1DStrategy):
        def interp_into(self, interpolator, target, x):
            target[...] = 0

    x = np.array([0.0, 1.0, 2.0])
    with pytest.raises(TypeError, match="inverse needs a built-in device strategy"):
        pkg.Interp1D.new_unchecked(x, x.copy(), Mine()).inverse()
    xi = np.array([0, 1, 2], dtype=np.int16)        # the generic host path (no device handle)
    with pytest.raises(TypeError, match="inverse needs a built-in device strategy"):
        pkg.Interp1D.builder(xi.copy()).x(xi).build().inverse()
