"""CPU: the lane-wise evaluation at the boundary -- the new entry point in the header, the ctypes binding, the built library
and the Rust declaration, all with one argument list; the refusal that needs no handle and no
device; the Python mirror's refusals, decided before the library is reached; the header's statement of the value rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAME = "ndi_interp1d_eval_lanewise"
# (C type, name) of every argument, in order: the issue's contract
ARGS = (("const ndi_interp1d*", "h"), ("const void*", "q"), ("uint64_t", "nq"), ("uint64_t", "q_row_stride"), ("void*", "out"),
        ("uint64_t", "out_row_stride"), ("const ndi_eval_opts*", "opts"), ("ndi_oob_info*", "info"))
RUST = {"const ndi_interp1d*": "*const ndi_interp1d", "const void*": "*const c_void", "uint64_t": "u64", "void*": "*mut c_void",
        "const ndi_eval_opts*": "*const ndi_eval_opts", "ndi_oob_info*": "*mut ndi_oob_info"}


def _norm(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_capi_library_and_rust_carry_the_symbol_with_one_argument_list(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    m = re.search(r"ndi_status %s\(([^)]*)\);" % NAME, header)
    assert m, "the header does not declare " + NAME
    assert [_norm(a) for a in m.group(1).split(",")] == [f"{t} {n}" for t, n in ARGS]
    # the value rule, in one sentence
    assert ("out[j][l] is, bit for bit and zero signs included, element l of the row ndi_interp1d_eval(h) writes for the "
            "single query q[j][l].") in header
    assert "lane l's OWN" in _norm(header) and "j * lanes + l" in header
    res, args = cap.SYMBOLS[NAME]
    P, U = C.c_void_p, C.c_uint64
    assert res is C.c_int and args == [P, P, U, U, P, U, C.POINTER(cap.EvalOpts), C.POINTER(cap.OobInfo)]
    # ndi_interp1d_eval's list with the query stride put in
    ev = cap.SYMBOLS["ndi_interp1d_eval"][1]
    assert args == ev[:3] + [U] + ev[3:]
    assert hasattr(C.CDLL(cap.LIB_PATH), NAME)       # (the bounds-checked build: test_checked_library_exports_the_same_abi)
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    m = re.search(r"pub fn %s\(([^)]*)\) -> i32;" % NAME, rust)
    assert m, "hip_ffi.rs does not declare " + NAME
    got = [_norm(a) for a in m.group(1).split(",") if a.strip()]
    assert got == [f"{n}: {RUST[t]}" for t, n in ARGS]
    assert cap.lib().ndi_version() == (0 << 16) | 5     # one new symbol, no new enumerator: no version change
    for cls in (pkg.Linear, pkg.CubicSplineStrategy, pkg.DerivativeStrategy, pkg.AntiderivativeStrategy, pkg.InverseStrategy):
        assert callable(getattr(cls, "interp_lanewise_into")), cls
    assert callable(pkg.Interp1D.interp_lanewise) and callable(pkg.Interp1D.interp_lanewise_into)


def test_null_handle_needs_no_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    buf = np.zeros(4)
    info = cap.OobInfo()
    assert lib.ndi_interp1d_eval_lanewise(None, buf.ctypes.data, 4, 1, buf.ctypes.data, 1, None, C.byref(info)) == cap.BAD_ARG
    assert cap.last_error() == "null handle"
    assert np.all(buf == 0.0)


def test_mirror_refuses_strategies_without_a_handle(pkg):
    class Mine(pkg.Interp1DStrategy):
        def interp_into(self, interpolator, target, x):
            target[...] = 0

    x = np.array([0.0, 1.0, 2.0])
    with pytest.raises(TypeError, match="interp_lanewise needs a built-in device strategy"):
        pkg.Interp1D.new_unchecked(x, x.copy(), Mine()).interp_lanewise(x)
    xi = np.array([0, 1, 2], dtype=np.int32)        # i32 host data: the generic host path (no device handle)
    it = pkg.Interp1D.builder(xi.copy()).x(xi).build()
    with pytest.raises(TypeError, match="interp_lanewise needs a built-in device strategy"):
        it.interp_lanewise(xi)
    # ... and that is decided before the shape check
    with pytest.raises(TypeError, match="interp_lanewise needs a built-in device strategy"):
        it.interp_lanewise_into(np.zeros((2, 7), np.int32), np.zeros(3, np.int32))
