"""An x axis per lane on hostile inputs: knot spacings at the denormal edge and of order 1e300 (f32: 1e30), data with
signed zeros, infinities and NaN in single entries -- parity with the single-column handle must still hold bit for bit,
NaN payloads aside (there NaN-ness is compared); device-resident axes whose only flaw is in the last lane, found by the
kernel pass; and one case per kernel under the bounds-checked library with no recorded violation."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_lane_axes import STRATEGIES, assert_bits, build, own_queries, ref_lanewise, ref_rows, table

pytestmark = pytest.mark.gpu


def assert_bits_or_nan(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN-ness differs"
    z = got.dtype.type(0)
    assert_bits(np.where(np.isnan(got), z, got), np.where(np.isnan(ref), z, ref), what)


def check_all(pkg, name, x, y, k, what):
    """tables, the row-wise call on [Lo, Hi] and the lane-wise call on every knot and midpoint, against the columns"""
    it, refs = build(pkg, name, x, y, k)
    if name != "Linear":
        a, b = it.strategy.coefficients()
        assert_bits_or_nan(a, np.concatenate([r.strategy.coefficients()[0] for r in refs], axis=1), what + " a")
        assert_bits_or_nan(b, np.concatenate([r.strategy.coefficients()[1] for r in refs], axis=1), what + " b")
    lo, hi = x[0].max(), x[-1].min()
    if lo <= hi:
        inside = np.unique(x[(x >= lo) & (x <= hi)])
        q = np.unique(np.concatenate([inside, inside[:-1] + 0.5 * (inside[1:] - inside[:-1]), [lo, hi]]).astype(x.dtype))
        q = q[(q >= lo) & (q <= hi)]
        assert_bits_or_nan(it.interp_array(q), ref_rows(refs, q), what + " rows")
    q2 = own_queries(x)
    assert_bits_or_nan(it.interp_lanewise(q2), ref_lanewise(refs, q2), what + " lane-wise")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(STRATEGIES))
def test_extreme_spacings(pkg, dt, name):
    n = 6
    fi = np.finfo(dt)
    sub = fi.smallest_subnormal
    big = dt(1e300) if dt == np.float64 else dt(1e30)
    steps = np.array([0, 1, 3, 4, 9, 10], dtype=dt)
    x = np.stack([steps * sub * dt(4),                      # subnormal knots, spacings of a few ulp of zero
                  steps * sub * dt(4) + fi.tiny,            # spacings below the smallest normal, on normal knots
                  steps * big,                              # dx * dx overflows
                  -big + steps * (big / dt(8)),             # large knots, both signs
                  steps * dt(1e-3) + dt(1.0)], axis=1).astype(dt)
    assert np.all(x[1:] > x[:-1])
    rng = np.random.default_rng(5)
    y = rng.uniform(-1.0, 1.0, x.shape).astype(dt)
    k = rng.uniform(-1.0, 1.0, x.shape).astype(dt)
    check_all(pkg, name, x, y, k, f"{name} {np.dtype(dt).name} extreme spacings")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(STRATEGIES))
def test_hostile_data_entries(pkg, dt, name):
    n, L = 7, 6
    x, y, k = table(n, L, dt)
    y[2, 0] = dt(0.0)
    y[3, 0] = dt(-0.0)
    y[:, 1] = dt(-0.0)                 # a column of negative zeros: the zero signs of the results
    y[3, 2] = dt(np.inf)
    y[0, 3] = dt(-np.inf)
    y[6, 4] = dt(np.nan)
    y[1, 5] = np.finfo(dt).max
    y[2, 5] = -np.finfo(dt).max
    k[4, 0] = dt(np.nan)
    k[2, 2] = dt(np.inf)
    check_all(pkg, name, x, y, k, f"{name} {np.dtype(dt).name} hostile data")


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n,rows", [(33, (31, 32)), (130, (63, 64)), (130, (64, 65)), (2, (0, 1))])
@pytest.mark.parametrize("how", ["tie", "nan"])
def test_device_axes_are_checked_by_the_kernel_pass(pkg, dt, n, rows, how):
    """A flaw in the LAST lane only, between two given rows (130 knots: across the edge of a thread's run of 64)."""
    import torch
    L = 65
    x, y, _ = table(n, L, dt)
    if how == "tie":
        x[rows[1], L - 1] = x[rows[0], L - 1]
    else:
        x[rows[1], L - 1] = np.nan
    tx, ty = torch.as_tensor(x, device="cuda:0"), torch.as_tensor(y, device="cuda:0")
    with pytest.raises(pkg.BuilderError.Monotonic) as e:
        pkg.Interp1D.builder(ty).lane_axes(tx).build()
    assert str(e.value).endswith(f"Values in the x axis need to be strictly monotonic rising (lane {L - 1})"), str(e.value)
    x[0, 7] = x[1, 7] if n > 2 else np.nan        # and a lower lane as well: the lowest one is named
    with pytest.raises(pkg.BuilderError.Monotonic, match=r"\(lane 7\)"):
        pkg.Interp1D.builder(ty).lane_axes(torch.as_tensor(x, device="cuda:0")).build()


def test_one_case_per_kernel(pkg, monkeypatch):
    """Every new kernel instance once: the check pass, the spline build (general and parabola rows), the local cubics with
    the per-lane knot accessor, and the evaluation kernel for Linear and the cubic class, row-wise and lane-wise, from the
    plain tables and from the record copy; more elements than one grid-stride trip of a small grid covers."""
    import torch
    for dt in (np.float64, np.float32):
        for name, n in (("Linear", 2), ("CubicSpline", 3), ("CubicSpline-natural", 33), ("Pchip", 33), ("Akima", 5), ("CubicHermite", 4)):
            x, y, k = table(n, 65, dt)
            tx, ty, tk = (torch.as_tensor(a, device="cuda:0") for a in (x, y, k))
            it, refs = build(pkg, name, x, y, k)
            dev = pkg.Interp1D.builder(ty).lane_axes(tx).strategy(STRATEGIES[name][1](pkg, tk, y.shape)).build()
            lo, hi = x[0].max(), x[-1].min()
            q = np.random.default_rng(n).uniform(lo, hi, 1500).astype(dt).clip(lo, hi)
            q2 = np.tile(own_queries(x), (20, 1))
            ref, ref2 = ref_rows(refs, q), ref_lanewise(refs, q2)
            for records in ("0", "1"):
                monkeypatch.setenv("NDI_LANE_AXES_RECORDS", records)
                monkeypatch.setenv("NDI_LANEWISE_WGS", "1")
                for h in (it, dev):
                    assert_bits(h.interp_array(q), ref, f"{name} rows records={records}")
                    assert_bits(h.interp_array(torch.as_tensor(q, device="cuda:0")).cpu().numpy(), ref, f"{name} device rows")
                    assert_bits(h.interp_lanewise(q2), ref2, f"{name} lane-wise records={records}")
                    buf = torch.empty(q2.shape, dtype=tx.dtype, device="cuda:0")
                    h.interp_lanewise_into(torch.as_tensor(q2, device="cuda:0"), buf)     # (with the pre-pass)
                    assert_bits(buf.cpu().numpy(), ref2, f"{name} device lane-wise")


def test_the_bounds_checked_library_runs_clean():
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lane_axes_hostile.py"), "-m", "gpu", "-x",
                        "-q", "-k", "test_one_case_per_kernel or test_device_axes_are_checked"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
