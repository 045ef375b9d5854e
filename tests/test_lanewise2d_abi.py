"""CPU: the 2-D lane-wise evaluation at the boundary -- the entry point in the header, the ctypes binding, the built library
and the Rust declaration, all with one argument list (ndi_interp2d_eval's with q_row_stride put in after nq); the refusal that
needs no handle and no device; the Python mirror's refusals, decided before the library is reached; the header's statement of
the value rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAME = "ndi_interp2d_eval_lanewise"
# (C type, name) of every argument, in order: the issue's contract
ARGS = (("const ndi_interp2d*", "h"), ("const void*", "qx"), ("const void*", "qy"), ("uint64_t", "nq"), ("uint64_t", "q_row_stride"),
        ("void*", "out"), ("uint64_t", "out_row_stride"), ("const ndi_eval_opts*", "opts"), ("ndi_oob_info*", "info"))
RUST = {"const ndi_interp2d*": "*const ndi_interp2d", "const void*": "*const c_void", "uint64_t": "u64", "void*": "*mut c_void",
        "const ndi_eval_opts*": "*const ndi_eval_opts", "ndi_oob_info*": "*mut ndi_oob_info"}


def _norm(text):
    return re.sub(r"\s+", " ", text).strip()


def test_header_capi_library_and_rust_carry_the_symbol_with_one_argument_list(pkg):
    cap = pkg._capi
    header = open(os.path.join(ROOT, "include", "ndinterp.h")).read()
    m = re.search(r"ndi_status %s\(([^)]*)\);" % NAME, header)
    assert m, "the header does not declare " + NAME
    assert [_norm(a) for a in m.group(1).split(",")] == [f"{t} {n}" for t, n in ARGS]
    # ... which is ndi_interp2d_eval's list with the query stride put in after nq
    ev = re.search(r"ndi_status ndi_interp2d_eval\(([^)]*)\);", header)
    ev = [_norm(a) for a in ev.group(1).split(",")]
    assert [f"{t} {n}" for t, n in ARGS] == ev[:4] + ["uint64_t q_row_stride"] + ev[4:]
    # the value rule, in one sentence
    assert ("out[j][l] is, bit for bit and zero signs included, element l of the row ndi_interp2d_eval(h) writes for the "
            "single query (qx[j][l], qy[j][l]).") in header
    assert header.count("j * lanes + l") >= 2            # (the 1-D comment and this one)
    assert "Not provided: lane-wise 2-D evaluation" not in header
    res, args = cap.SYMBOLS[NAME]
    P, U = C.c_void_p, C.c_uint64
    assert res is C.c_int and args == [P, P, P, U, U, P, U, C.POINTER(cap.EvalOpts), C.POINTER(cap.OobInfo)]
    ev = cap.SYMBOLS["ndi_interp2d_eval"][1]
    assert args == ev[:4] + [U] + ev[4:]
    assert hasattr(C.CDLL(cap.LIB_PATH), NAME)
    rust = open(os.path.join(ROOT, "rust", "ndarray-interp-hip", "src", "hip_ffi.rs")).read()
    m = re.search(r"pub fn %s\(([^)]*)\) -> i32;" % NAME, rust)
    assert m, "hip_ffi.rs does not declare " + NAME
    got = [_norm(a) for a in m.group(1).split(",") if a.strip()]
    assert got == [f"{n}: {RUST[t]}" for t, n in ARGS]
    assert cap.lib().ndi_version() == (0 << 16) | 5     # one new symbol, no new enumerator: no version change
    for cls in (pkg.Bilinear, pkg.Bicubic):
        assert callable(getattr(cls, "interp_lanewise_into")), cls
    assert callable(pkg.Interp2D.interp_lanewise) and callable(pkg.Interp2D.interp_lanewise_into)


def test_null_handle_needs_no_device(pkg):
    cap, lib = pkg._capi, pkg._capi.lib()
    qx, qy, out = np.zeros(4), np.ones(4), np.full(4, 7.0)
    info = cap.OobInfo()
    st = lib.ndi_interp2d_eval_lanewise(None, qx.ctypes.data, qy.ctypes.data, 4, 1, out.ctypes.data, 1, None, C.byref(info))
    assert st == cap.BAD_ARG
    assert cap.last_error() == "null handle"
    assert np.all(qx == 0.0) and np.all(qy == 1.0) and np.all(out == 7.0)


def test_mirror_refuses_strategies_without_a_handle(pkg):
    class Mine(pkg.Interp2DStrategy):
        def interp_into(self, interpolator, target, x, y):
            target[...] = 0

    x = np.array([0.0, 1.0, 2.0])
    z = np.zeros((3, 3))
    with pytest.raises(TypeError, match="interp_lanewise needs a built-in device strategy"):
        pkg.Interp2D.new_unchecked(x, x.copy(), z, Mine()).interp_lanewise(x, x)
    xi = np.array([0, 1, 2], dtype=np.int32)        # i32 host data: the generic host path (no device handle)
    it = pkg.Interp2D.builder(np.zeros((3, 3), np.int32)).x(xi).y(xi.copy()).build()
    with pytest.raises(TypeError, match="interp_lanewise needs a built-in device strategy"):
        it.interp_lanewise(xi, xi)
    # ... and that is decided before the shape check
    with pytest.raises(TypeError, match="interp_lanewise needs a built-in device strategy"):
        it.interp_lanewise_into(np.zeros((2, 7), np.int32), np.zeros(5, np.int32), np.zeros(3, np.int32))
