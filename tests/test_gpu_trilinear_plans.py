"""GPU: the plans of Interp3D / Trilinear that tests/test_gpu_trilinear.py does not reach, bit for bit against
tests/trilinear_ref.py: later trips of the grid-stride loop with a live (row, vector) carry, a failure in a later trip, the
second trip of the range pre-pass, padded output strides, device queries with a host output in several chunks, a chunk
budget below one row, validation of device axes through the C call, eight threads on one handle with failing calls among
them, the mirror's copy-back into a non-contiguous buffer after a failure, CPU torch tensors as queries; and the later-trip
cases again under the bounds-checked library."""
import ctypes as C
import functools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import trilinear_ref as tr
from conftest import ROOT
from test_gpu_trilinear import (BLOCK, SENTINEL, WIDE, dev, error_fixture, expect, inside, make, nonuniform, plant, raw_call,
                                same_bits, traced)
from test_trilinear_abi import host_desc

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
NQ = 70_001
VPRS = (3, 5, 7)


def torch_full(shape, dt):
    import torch
    return torch.full(shape, SENTINEL, dtype=dev(np.zeros(1, dt)).dtype, device="cuda:0")


# ---- later trips of the grid-stride loop ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def later_trip_fixture(dt, staged):
    """(axes, data, queries, reference) with the most lanes any case needs; a case of fewer lanes takes the leading lanes of data
    and reference (the lanes of a row are independent).  staged: the x axis fills more than half a CU's LDS, so the resident
    grid is one workgroup per CU; else a small grid, evaluated with NDI_TRILINEAR_STAGE=0 at eight workgroups per CU."""
    rng = np.random.default_rng(21 + staged)
    shape = (100_000 // np.dtype(dt).itemsize, 2, 2) if staged else (5, 4, 3)
    lanes = (7 if staged else 9) * WIDE[dt]
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + (lanes,)).astype(dt)
    q = [inside(rng, k, NQ, dt) for k in ax]
    fail, _, ref = tr.trilinear_ref(*ax, data, *q)
    assert fail is None
    for a in (data, ref):            # shared between the cases: left unchanged
        a.setflags(write=False)
    return ax, data, q, ref


def later_trip_case(pkg, monkeypatch, capfd, dt, staged, lanes, wide, check):
    """one call of 70 001 queries; returns the plan's grid"""
    ax, data, q, ref = later_trip_fixture(dt, staged)
    it = make(pkg, *ax, np.ascontiguousarray(data[..., :lanes]))
    vec = WIDE[dt] if wide else 1
    assert lanes % vec == 0
    vpr = lanes // vec
    monkeypatch.setenv("NDI_TRILINEAR_VEC", "-1" if wide else "1")
    monkeypatch.setenv("NDI_TRILINEAR_STAGE", "-1" if staged else "0")
    what = f"{np.dtype(dt)} staged={staged} lanes={lanes} vec={vec} check={check}"
    qd = [dev(a) for a in q]
    with traced(capfd) as t:
        if check:
            got = it.interp_array(*qd)
        else:
            got = torch_full((NQ, lanes), dt)
            it.interp_array_into(*qd, got)
    monkeypatch.delenv("NDI_TRILINEAR_VEC")
    monkeypatch.delenv("NDI_TRILINEAR_STAGE")
    expect(t.plans, what, vec=vec, stage=int(staged), check=check)
    grid = t.plans[0]["grid"]
    assert grid * BLOCK < NQ * vpr, f"{what}: one trip only, grid {grid}"
    same_bits(got.cpu().numpy(), np.ascontiguousarray(ref[:, :lanes]), what)
    return grid


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wide", [True, False])
def test_later_trips_with_a_live_carry_staged_axes(pkg, monkeypatch, capfd, dt, wide):
    """3, 5 and 7 vectors per row over a grid of one workgroup per CU: every thread walks the batch several times and, where
    the grid's stride is no multiple of the vectors per row, moves on by a (rows, vectors) step with a carry.  That at least one
    of the three strides is such is a condition of the test."""
    grids = {}
    for vpr in VPRS:
        lanes = vpr * (WIDE[dt] if wide else 1)
        for check in (1, 0):
            grids[vpr, check] = later_trip_case(pkg, monkeypatch, capfd, dt, True, lanes, wide, check)
    live = [vpr for (vpr, _), g in grids.items() if (g * BLOCK) % vpr != 0]
    assert live, f"no case with a nonzero vector step: grids {grids}"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wide", [True, False])
def test_later_trips_with_axes_in_global_memory(pkg, monkeypatch, capfd, dt, wide):
    """f32 with 36 lanes and f64 with 18 (nine 16-byte vectors per row; 36 / 18 single elements in the scalar form) at eight
    workgroups per CU"""
    lanes = 9 * WIDE[dt]
    for check in (1, 0):
        later_trip_case(pkg, monkeypatch, capfd, dt, False, lanes, wide, check)


def later_trip_failure(pkg, monkeypatch, capfd, dt, wide):
    from ndarray_interp_amd.errors import _rust_float
    ax, data, q, ref = later_trip_fixture(dt, True)
    lanes = 3 * (WIDE[dt] if wide else 1)
    it = make(pkg, *ax, np.ascontiguousarray(data[..., :lanes]))
    monkeypatch.setenv("NDI_TRILINEAR_VEC", "-1" if wide else "1")
    what = f"{np.dtype(dt)} wide={wide}"
    with traced(capfd) as t:
        it.interp_array(*[dev(a) for a in q])                                        # a clean call: the grid of this shape
    expect(t.plans, what, vec=WIDE[dt] if wide else 1, stage=1, check=1)
    step = t.plans[0]["grid"] * BLOCK
    row = 2 * step // 3 + 1                                                          # its first item is just beyond two strides
    assert 2 * step < row * 3 <= 2 * step + 3 and row + 1000 < NQ, (what, step, row)
    bad = np.nextafter(ax[1][-1], dt(np.inf))
    qq = plant(q, [(1, row, bad), (0, row + 1000, np.nan)])
    assert tr.first_failure(*ax, *qq, False) == (row, 1)
    for mode in ({}, {"fresh": True}):
        buf = torch_full((NQ, lanes), dt)
        with traced(capfd) as t:
            with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
                it.interp_array_into(*[dev(a) for a in qq], buf, **mode)
        expect(t.plans, f"{what} {mode}", check=1 if mode else 0, grid=step // BLOCK)
        err = e.value
        assert (err.index, err.axis, err.value) == (row, 1, float(bad)), (what, mode, err.index, err.axis, err.value)
        assert str(err) == f"y = {_rust_float(float(bad))} is not in range"
        got = buf.cpu().numpy()
        same_bits(got[:row], np.ascontiguousarray(ref[:row, :lanes]), f"{what} {mode}: the rows before the failing query")
        if not mode:
            assert np.all(got[row:] == SENTINEL), f"{what}: the failing row and all later rows are untouched"
    monkeypatch.delenv("NDI_TRILINEAR_VEC")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wide", [True, False])
def test_a_failure_in_a_later_trip(pkg, monkeypatch, capfd, dt, wide):
    """an out-of-range y in the row whose first item lies just beyond two strides of the grid, a NaN x 1000 rows later: with the
    pre-pass the evaluation stops at rows * vpr items; without it the report comes from the carried row"""
    later_trip_failure(pkg, monkeypatch, capfd, dt, wide)


# ---- the pre-pass past its grid cap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_the_pre_pass_goes_round_twice(pkg, capfd, dt):
    """4096 * 256 + 300 queries: range_check3_kernel's grid is capped at 4096 workgroups, so queries from 1 048 576 on are
    tested on its second trip; one failure, on z, at 1 048 676"""
    rng = np.random.default_rng(22)
    shape, Q, at = (3, 3, 3), 4096 * BLOCK + 300, 4096 * BLOCK + 100
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape).astype(dt)
    q = [inside(rng, k, Q, dt) for k in ax]
    fail, _, ref = tr.trilinear_direct(*ax, data, *q)
    assert fail is None
    it = make(pkg, *ax, data)
    bad = np.nextafter(ax[2][-1], dt(np.inf))
    qq = plant(q, [(2, at, bad)])
    assert tr.first_failure(*ax, *qq, False) == (at, 2)
    buf = torch_full((Q,), dt)
    with traced(capfd) as t:
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array_into(*[dev(a) for a in qq], buf)
    expect(t.plans, "a failure on the second trip", vec=1, stage=1, check=0)
    assert (e.value.index, e.value.axis, e.value.value) == (at, 2, float(bad))
    got = buf.cpu().numpy()
    same_bits(got[:at], ref[:at, 0], "the rows before the failing query")
    assert got[at:].size == 200 and np.all(got[at:] == SENTINEL)
    buf = torch_full((Q,), dt)
    with traced(capfd) as t:
        it.interp_array_into(*[dev(a) for a in q], buf)
    expect(t.plans, "a clean batch of the same size", vec=1, stage=1, check=0)
    same_bits(buf.cpu().numpy(), ref[:, 0], "a clean batch of the same size")


# ---- strides, chunks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("q_dev", [False, True])
def test_a_host_output_with_a_padded_stride(pkg, dt, q_dev):
    """out_row_stride = lanes + 4 into host memory: the pitch of the copy out of the staging buffer"""
    cap = pkg._capi
    ax, data, q, it = error_fixture(pkg, dt, False)
    Q, lanes = 300, 4
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    out = np.full((Q, lanes + 4), SENTINEL, dt)
    st, _ = raw_call(pkg, it, *([dev(a) for a in q] if q_dev else q), Q, out, lanes + 4, q_dev=q_dev)
    assert st == cap.OK, cap.last_error()
    same_bits(np.ascontiguousarray(out[:, :lanes]), ref, "a padded host output")
    assert np.all(out[:, lanes:] == SENTINEL), "the padding of a row is not written"
    bad = np.nextafter(ax[0][0], dt(-np.inf))
    qq = plant(q, [(0, 200, bad)])
    out = np.full((Q, lanes + 4), SENTINEL, dt)
    st, info = raw_call(pkg, it, *([dev(a) for a in qq] if q_dev else qq), Q, out, lanes + 4, q_dev=q_dev)
    assert st == cap.OUT_OF_BOUNDS and (info.index, info.axis, info.value) == (200, 0, float(bad))
    same_bits(np.ascontiguousarray(out[:200, :lanes]), ref[:200], "a padded host output: the rows before the failing query")
    assert np.all(out[:200, lanes:] == SENTINEL) and np.all(out[200:] == SENTINEL)


@pytest.mark.parametrize("dt", DTYPES)
def test_the_wide_form_with_a_padded_stride(pkg, capfd, dt):
    """out_row_stride = lanes + WIDE into an aligned device buffer keeps the 16-byte form"""
    import torch
    cap = pkg._capi
    ax, data, q, it = error_fixture(pkg, dt, False)
    Q, lanes, W = 300, 4, WIDE[dt]
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    out = torch_full((Q, lanes + W), dt)
    assert out.data_ptr() % 16 == 0
    with traced(capfd) as t:
        st, _ = raw_call(pkg, it, *[dev(a) for a in q], Q, out, lanes + W, q_dev=True, out_dev=True)
        torch.cuda.synchronize()
    assert st == cap.OK, cap.last_error()
    expect(t.plans, "the wide form, padded", vec=W, stage=1, check=0)
    got = out.cpu().numpy()
    same_bits(np.ascontiguousarray(got[:, :lanes]), ref, "the wide form, padded")
    assert np.all(got[:, lanes:] == SENTINEL), "the padding of a row is not written"


@pytest.mark.parametrize("dt", DTYPES)
def test_device_queries_and_a_host_output_in_two_chunks(pkg, monkeypatch, capfd, dt):
    """160 rows per chunk, 300 queries in device memory: the failing value of the second chunk is read back from the caller's
    device array at the batch's index"""
    cap = pkg._capi
    ax, data, q, it = error_fixture(pkg, dt, False)
    Q, lanes = 300, 4
    monkeypatch.setenv("NDI_TRILINEAR_CHUNK", str(160 * lanes * np.dtype(dt).itemsize))
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    out = np.full((Q, lanes), SENTINEL, dt)
    with traced(capfd) as t:
        st, _ = raw_call(pkg, it, *[dev(a) for a in q], Q, out, lanes, q_dev=True)
    assert st == cap.OK, cap.last_error()
    expect(t.plans, "two chunks", n=2, check=1)
    same_bits(out, ref, "two chunks")
    bad = np.nextafter(ax[2][-1], dt(np.inf))
    qq = plant(q, [(2, 200, bad), (2, 40, ax[2][0]), (0, 250, np.nan)])       # (row 40 = 200 - 160 holds a value in range)
    out = np.full((Q, lanes), SENTINEL, dt)
    with traced(capfd) as t:
        st, info = raw_call(pkg, it, *[dev(a) for a in qq], Q, out, lanes, q_dev=True)
    expect(t.plans, "a failure in the second chunk", n=2, check=1)
    assert st == cap.OUT_OF_BOUNDS and (info.index, info.axis, info.value) == (200, 2, float(bad)), (info.index, info.axis, info.value)
    ref2 = tr.trilinear_ref(*ax, data, *qq)[2]
    same_bits(out[:200], ref2[:200], "the rows before the failure, across the chunk boundary")
    assert np.all(out[200:] == SENTINEL)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_chunk_budget_below_one_row(pkg, monkeypatch, capfd, dt):
    """NDI_TRILINEAR_CHUNK=1: one row per chunk, never none"""
    ax, data, q, it = error_fixture(pkg, dt, False)
    q = [a[:5].copy() for a in q]
    monkeypatch.setenv("NDI_TRILINEAR_CHUNK", "1")
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    with traced(capfd) as t:
        got = it.interp_array(*q)
    expect(t.plans, "five chunks", n=5, check=1)
    same_bits(got, ref, "five chunks")
    qq = plant(q, [(1, 3, np.nan)])
    buf = np.full((5, 4), SENTINEL, dt)
    with traced(capfd) as t:
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_array_into(*qq, buf)
    expect(t.plans, "a failure in the fourth chunk", n=4, check=1)
    assert (e.value.index, e.value.axis) == (3, 1) and np.isnan(e.value.value)
    same_bits(buf[:3], ref[:3], "the rows before the failing chunk")
    assert np.all(buf[3:] == SENTINEL)


# ---- validate = 1 on device axes ------------------------------------------------------------------------------------------------------
def test_validation_of_device_axes_through_the_c_call(pkg):
    """ndi_interp3d_create with validate != 0 and device pointers: the axes are fetched and pass check_axes_3d, in its order"""
    cap, lib = pkg._capi, pkg._capi.lib()
    rng = np.random.default_rng(23)
    shape, lanes = (5, 4, 3), 4
    ax = [nonuniform(rng, n, np.float64) for n in shape]
    data = rng.uniform(-1, 1, shape + (lanes,))
    q = [inside(rng, k, 300, np.float64) for k in ax]

    def create(x, y, z):
        keep = [dev(a) for a in (x, y, z, data)]
        d = host_desc(pkg, x, y, z, data, validate=1)
        d.memspace = cap.MEM_DEVICE
        d.x, d.y, d.z, d.data = (t.data_ptr() for t in keep)
        h = C.c_void_p(0xdead)
        st = lib.ndi_interp3d_create(C.byref(d), C.byref(h))
        return st, cap.last_error() if st != cap.OK else "", h

    st, _, h = create(*ax)
    assert st == cap.OK and h.value
    opts = cap.EvalOpts()
    out = np.full((300, lanes), SENTINEL)
    assert lib.ndi_interp3d_eval(h, *[a.ctypes.data for a in q], 300, out.ctypes.data, lanes, C.byref(opts), None) == cap.OK
    same_bits(out, tr.trilinear_ref(*ax, data, *q)[2], "a handle validated on device axes")
    lib.ndi_interp3d_destroy(h)
    tie = ax[0].copy(); tie[2] = tie[1]
    falling = ax[1][::-1].copy()
    nan = ax[2].copy(); nan[1] = np.nan
    short = ax[2][:2].copy()
    rising = "The %s-axis needs to be strictly monotonic rising"
    for axes, status, text in (((tie, falling, nan), cap.MONOTONIC, rising % "x"),        # every flaw at once: x is named
                               ((ax[0], falling, nan), cap.MONOTONIC, rising % "y"),
                               ((ax[0], ax[1], nan), cap.MONOTONIC, rising % "z"),
                               ((tie, falling, short), cap.SHAPE, "Lenghts of z-axis and data-2-axis need to match. Got z: 2, data-2: 3"),
                               ((tie, ax[1], ax[2]), cap.MONOTONIC, rising % "x")):
        st, msg, h = create(*axes)
        assert (st, msg) == (status, text), (st, msg)
        assert h.value is None, "no handle is returned"


# ---- threads ---------------------------------------------------------------------------------------------------------------------------
def test_eight_threads_on_one_handle_half_of_them_failing(pkg):
    """thread t runs five calls; even threads pass rolled clean batches, odd threads plant a failure at row 17 t on axis t % 3:
    every failing call reports its own index, axis and value and leaves its own rows before it, every clean call is whole"""
    dt = np.float32
    ax, data, q, it = error_fixture(pkg, dt, False)
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    results, errors = {}, []

    def work(tid):
        try:
            for r in range(5):
                qq = [np.roll(a, tid + r) for a in q]
                want = np.roll(ref, tid + r, axis=0)
                if tid % 2 == 0:
                    results[tid, r] = (None, it.interp_array(*qq), want)
                    continue
                axis, index = tid % 3, 17 * tid
                bad = np.nextafter(ax[axis][-1], dt(np.inf)) + dt(tid + r)
                qq = plant(qq, [(axis, index, bad)])
                buf = np.full((300, 4), SENTINEL, dt)
                try:
                    it.interp_array_into(*qq, buf)
                    results[tid, r] = ("no error", buf, want)
                except pkg.InterpolateError.OutOfBounds as e:
                    results[tid, r] = ((e.index, e.axis, e.value, index, axis, float(bad)), buf, want)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 40
    for (tid, r), (err, got, want) in results.items():
        if tid % 2 == 0:
            same_bits(got, want, f"thread {tid} call {r}")
        else:
            assert err != "no error" and err[:3] == err[3:], (tid, r, err)
            same_bits(got[:err[3]], want[:err[3]], f"thread {tid} call {r}: the rows before the failing query")
            assert np.all(got[err[3]:] == SENTINEL), (tid, r)


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------
def test_a_failure_into_a_non_contiguous_host_buffer(pkg):
    """interp_array_into a strided numpy view with a failing query at flat row 7 of rank-3 queries: rows 0 .. 6 are copied back
    into the view, everything else keeps the sentinel"""
    rng = np.random.default_rng(24)
    dt, shape, trailing = np.float64, (5, 4, 3), (2, 3)
    ax = [nonuniform(rng, n, dt) for n in shape]
    data = rng.uniform(-1, 1, shape + trailing)
    it = make(pkg, *ax, data)
    q = [inside(rng, k, 24, dt) for k in ax]
    q[2][7] = ax[2][-1] + 1.0
    fail, axis, ref = tr.trilinear_ref(*ax, data, *q)
    assert (fail, axis) == (7, 2)
    wide = np.full((2, 3, 4, 2, 6), SENTINEL)
    view = wide[..., ::2]
    assert not view.flags.c_contiguous
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        it.interp_array_into(*[a.reshape(2, 3, 4) for a in q], view)
    assert (e.value.index, e.value.axis, e.value.value) == (7, 2, float(q[2][7]))
    flat = np.ascontiguousarray(view).reshape(24, 6)
    same_bits(flat[:7], ref[:7], "the rows before the failing query, in the view")
    assert np.all(flat[7:] == SENTINEL) and np.all(wide[..., 1::2] == SENTINEL)


@pytest.mark.parametrize("dt", DTYPES)
def test_cpu_torch_tensors_as_queries(pkg, dt):
    """CPU tensors are host arrays to the mirror, as in the 1-D and 2-D mirrors (Buf takes their pointer as host memory): a numpy
    result, bit-equal to the numpy call"""
    import torch
    ax, data, q, it = error_fixture(pkg, dt, False)
    ref = tr.trilinear_ref(*ax, data, *q)[2]
    want = it.interp_array(*q)
    got = it.interp_array(*[torch.from_numpy(a) for a in q])
    assert isinstance(got, np.ndarray) and got.shape == want.shape
    same_bits(got, want, "CPU tensors against numpy arrays")
    same_bits(got, ref, "CPU tensors against the reference")
    got = it.interp_array(*[torch.from_numpy(a.astype(np.float64)).reshape(3, 100) for a in q])     # another dtype, another rank
    same_bits(got.reshape(300, 4), ref, "CPU tensors of rank 2")
    buf = np.full((300, 4), SENTINEL, dt)
    qq = plant(q, [(0, 11, np.nan)])
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        it.interp_array_into(*[torch.from_numpy(a) for a in qq], buf)
    assert (e.value.index, e.value.axis) == (11, 0)
    same_bits(buf[:11], ref[:11], "CPU tensors: the rows before the failing query")
    assert np.all(buf[11:] == SENTINEL)


# ---- the bounds-checked library ------------------------------------------------------------------------------------------------------
def test_checked_cases(pkg, monkeypatch, capfd):
    """what runs again under the bounds-checked library (below): the later trips -- both stagings, both forms, both check values
    -- and the failure in a later trip.  NDI_CHK on the carried row and vector is what a drifting carry trips there."""
    for dt in DTYPES:
        for wide in (True, False):
            for check in (1, 0):
                for vpr in VPRS:
                    later_trip_case(pkg, monkeypatch, capfd, dt, True, vpr * (WIDE[dt] if wide else 1), wide, check)
                later_trip_case(pkg, monkeypatch, capfd, dt, False, 9 * WIDE[dt], wide, check)
            later_trip_failure(pkg, monkeypatch, capfd, dt, wide)


def test_the_bounds_checked_library_runs_clean():
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_trilinear_plans.py"), "-m", "gpu", "-x",
                        "-q", "-k", "test_checked_cases"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
