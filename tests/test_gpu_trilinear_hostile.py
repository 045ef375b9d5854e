"""GPU: Interp3D / Trilinear on the edges of the division window and on hostile axes, bit for bit against
tests/trilinear_ref.py (generators in tests/hostile_inputs.py, their self-checks in tests/test_hostile_inputs.py).

frac_shared (csrc/kernels.hpp) takes the reciprocal path only inside an exponent window -- the divisor in [D_LO, D_HI], the
smallest numerator magnitude of a vector >= N_LO, the sum of the vector's magnitudes <= N_HI -- and the IEEE division
outside it.  The window cases put numerators and divisors on those edges and one float either side of them, at each of the
three division levels (d100 - d000, c10 - c00, c1 - c0).  The test is vector-wide, so the scalar and the 16-byte form take
different paths for the same lane; they must agree with the reference and with each other."""
import ctypes as C

import numpy as np
import pytest

import hostile_inputs as hostile
import trilinear_ref as tr
from test_gpu_trilinear import SENTINEL, WIDE, dev, expect, make, same_bits, traced
from test_trilinear_abi import host_desc

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def every_form(pkg, monkeypatch, capfd, dt, case, ref, extrapolate=False, lanes=8):
    """host arrays, device tensors and a caller's device buffer, in the wide and the scalar form, staged and unstaged; returns
    the rows of the device-tensor call per (vec, stage)"""
    axes, data, q = case["axes"], case["data"], case["q"]
    qd = [dev(a) for a in q]
    it = make(pkg, *axes, data, extrapolate)
    on_dev = make(pkg, *[dev(k) for k in axes], dev(data), extrapolate)
    rows = {}
    for vec in (WIDE[dt], 1):
        for stage in (1, 0):
            monkeypatch.setenv("NDI_TRILINEAR_VEC", "1" if vec == 1 else "-1")
            monkeypatch.setenv("NDI_TRILINEAR_STAGE", "-1" if stage else "0")
            what = f"{case['tag']} vec={vec} stage={stage}"
            with traced(capfd) as t:
                got = it.interp_array(*q)
            expect(t.plans, what + ": host arrays", vec=vec, stage=stage, check=1)
            same_bits(got, ref, what + ": host arrays")
            for h, name in ((it, "device tensors"), (on_dev, "device tensors, a handle built on tensors")):
                with traced(capfd) as t:
                    got = h.interp_array(*qd)
                expect(t.plans, what + ": " + name, vec=vec, stage=stage, check=1)
                same_bits(got.cpu().numpy(), ref, what + ": " + name)
            rows[vec, stage] = got.cpu().numpy()
            buf = dev(np.full((q[0].size, lanes), SENTINEL, dt))
            with traced(capfd) as t:
                it.interp_array_into(*qd, buf)
            expect(t.plans, what + ": a caller's device buffer", vec=vec, stage=stage, check=0)
            same_bits(buf.cpu().numpy(), ref, what + ": a caller's device buffer")
    monkeypatch.delenv("NDI_TRILINEAR_VEC")
    monkeypatch.delenv("NDI_TRILINEAR_STAGE")
    return rows


# ---- the edges of the division window ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("vary", [0, 1, 2])
def test_window_edges_on_every_division_level(pkg, monkeypatch, capfd, dt, vary):
    """the nine cases of one division level: three lane tables x three kinds of the varying axis, 125 queries each"""
    cases = [c for c in hostile.trilinear_window_cases(dt) if c["vary"] == vary]
    assert len(cases) == 9
    for c in cases:
        fail, _, ref = tr.trilinear_ref(*c["axes"], c["data"], *c["q"])
        assert fail is None and np.isfinite(ref).all(), c["tag"]
        rows = every_form(pkg, monkeypatch, capfd, dt, c, ref)
        for stage in (1, 0):
            same_bits(rows[WIDE[dt], stage], rows[1, stage], f"{c['tag']} stage={stage}: the wide form against the scalar form")


@pytest.mark.parametrize("dt", DTYPES)
def test_an_overflowing_difference_in_an_in_window_vector(pkg, monkeypatch, capfd, dt):
    """+-inf numerators (finite nodes whose difference overflows) beside in-window lanes: only the sum test of the window
    keeps them off the reciprocal path, on which inf - inf would turn the quotient into NaN"""
    for c in hostile.trilinear_nonfinite_lane_cases(dt):
        fail, _, ref = tr.trilinear_ref(*c["axes"], c["data"], *c["q"])
        assert fail is None and np.isinf(ref).any() == (c["vary"] == 2), c["tag"]
        rows = every_form(pkg, monkeypatch, capfd, dt, c, ref)
        same_bits(rows[WIDE[dt], 1], rows[1, 1], c["tag"] + ": the wide form against the scalar form")


# ---- hostile axes --------------------------------------------------------------------------------------------------------------
def raw_create(pkg, x, y, z, data, on_device):
    """ndi_interp3d_create with validate = 1 on host or on device arrays: (status, handle)"""
    cap = pkg._capi
    keep = [x, y, z, data]
    d = host_desc(pkg, x, y, z, data)
    if on_device:
        keep = [dev(a) for a in keep]
        d.memspace = cap.MEM_DEVICE
        d.x, d.y, d.z, d.data = (t.data_ptr() for t in keep)
    h = C.c_void_p()
    st = cap.lib().ndi_interp3d_create(C.byref(d), C.byref(h))
    return st, h


@pytest.mark.parametrize("dt", DTYPES)
def test_infinite_end_knots_are_accepted_from_host_and_device_axes(pkg, dt):
    """the builder's scan takes -inf < ... < +inf for strictly rising: the same verdict from host and from device axes, on
    each of the three axes"""
    cap = pkg._capi
    for c in hostile.trilinear_axis_cases(dt):
        if c["kind"] != "infinite ends":
            continue
        for on_device in (False, True):
            st, h = raw_create(pkg, *c["axes"], c["data"], on_device)
            assert st == cap.OK and h.value, (c["tag"], on_device, cap.last_error())
            cap.lib().ndi_interp3d_destroy(h)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("hostile_axis", [0, 1, 2])
def test_hostile_axes(pkg, dt, hostile_axis):
    """neighbouring floats, mixed and huge spacings, a -0.0 knot, infinite end knots and a subnormal spacing on one axis, the
    two others uneven: host arrays and device tensors, in range and extrapolating"""
    cases = [c for c in hostile.trilinear_axis_cases(dt) if c["hostile"] == hostile_axis]
    assert [c["kind"] for c in cases] == list(hostile.TRILINEAR_AXIS_KINDS)
    for c in cases:
        axes, data = c["axes"], c["data"]
        for extrapolate in (False, True):
            q = c["q"][extrapolate]
            what = f"{c['tag']} extrapolate={extrapolate}"
            fail, _, ref = hostile.trilinear_axis_reference(c, extrapolate)
            assert fail is None, what
            it = make(pkg, *axes, data, extrapolate)
            same_bits(it.interp_array(*q), ref, what + ": host arrays")
            on_dev = make(pkg, *[dev(k) for k in axes], dev(data), extrapolate)
            for h in (it, on_dev):
                same_bits(h.interp_array(*[dev(a) for a in q]).cpu().numpy(), ref, what + ": device tensors")
        # get_index_left_of against the reference's cell at the float either side of every interior knot
        import oracle
        k = axes[hostile_axis]
        if c["kind"] == "infinite ends":
            continue            # (the reference's search does not place a query between infinite ends)
        it = make(pkg, *axes, data)
        for v in np.concatenate([np.nextafter(k[1:-1], dt(-np.inf)), np.nextafter(k[1:-1], dt(np.inf)), k[1:-1]]):
            p = [a[1] for a in axes]
            p[hostile_axis] = v
            want = tuple(int(oracle.get_lower_index(a, np.array([e], dt))[0]) for a, e in zip(axes, p))
            assert it.get_index_left_of(*p) == want, (c["tag"], v)
