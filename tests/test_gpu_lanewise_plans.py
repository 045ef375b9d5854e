"""GPU: the lane-wise plans and geometries that tests/test_gpu_lanewise.py and tests/test_gpu_inverse.py leave out: rows
wider than a grid step (LanewisePos::advance with step_rows == 0, step_lanes == 0 and a carry in every trip), the pre-pass
beyond one trip of its 4096 blocks, what AUTO takes with both knobs unset, the unstaged axis at f32, the record cap, the
host staging loop of lanewise_run in two chunks, and inverse_eval_kernel past its grid of 2^20 blocks (its stride loop and
its 64-bit division branch).  Every case asserts, from the plan line (NDI_TRACE_PLAN) of the call under test, the plan it
claims to run.  Every comparison is bit for bit: hostile_inputs.check_bits, or torch.equal on integer views for the large
device-resident arrays.

The yardstick for wide rows: per_lane of tests/test_gpu_lanewise.py makes L row-wise calls, impossible at 1e5 lanes and
more.  Instead a pool of K = 16 abscissae (both end knots, an interior knot, its two neighbouring floats, uniform values)
is evaluated by ONE row-wise call, rows = interp_array(pool) of shape (K, L); the queries are xs[j, l] = pool[k[j, l]] with k
random, and the reference is rows[k[j, l], l].  For inverse handles the pool lies inside the range common to all lanes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_inputs
import inverse_cases as ic
from conftest import ROOT
from test_gpu_lanewise import VARIANTS, all_variants, data_for, forward, lane_queries, per_lane, set_variant

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
K = 16
BLOCK = 256          # threads of a workgroup of every lane-wise kernel (csrc/kernels.hpp)


def _tdt(dt):
    import torch
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def _idt(t):
    import torch
    return torch.int64 if t.dtype == torch.float64 else torch.int32


def same_bits(got, ref, what):
    """device tensors: check_bits on the host up to 2^22 elements, beyond that torch.equal on the integer views"""
    import torch
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.numel() <= 1 << 22:
        hostile_inputs.check_bits(got.cpu().numpy(), ref.cpu().numpy(), what)
    else:
        assert not bool(torch.isnan(ref).any()), what
        assert torch.equal(got.contiguous().view(_idt(got)), ref.contiguous().view(_idt(ref))), what + ": the bits differ"


class traced:
    def __init__(self, capfd):
        self.capfd = capfd

    def __enter__(self):
        os.environ["NDI_TRACE_PLAN"] = "1"
        self.capfd.readouterr()
        return self

    def __exit__(self, *a):
        os.environ.pop("NDI_TRACE_PLAN", None)
        self.plans = [ln for ln in self.capfd.readouterr().err.splitlines() if ln.startswith("[ndi plan] lanewise form=")
                      or ln.startswith("[ndi plan] inverse eval")]


def grid_of(line):
    return int(line.rsplit("grid=", 1)[1].split()[0])


# ---- tables of L lanes and their pools --------------------------------------------------------------------------------------
def wide_handle(pkg, source, dt, n, L, seed):
    """(the handle, the pool's limits lo / hi) on device-resident tables drawn on the device: 'linear', 'pchip', 'anti_pchip',
    'anti_linear', 'inv_linear', 'inv_pchip'.  Inverse sources: every lane rises from -1 - pad0[l] to 1 + pad1[l], so the
    lanes have their own limits and the common range holds [-1, 1] up to rounding; lo / hi are read from the node table"""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    step = torch.rand(n, dtype=torch.float64, device="cuda:0", generator=g) * 1.5 + 0.5
    step[1::3] *= 0.05                                         # uneven steps, as inverse_cases.knots
    x = (torch.cumsum(step, 0) - step[0]).to(_tdt(dt))
    if source.startswith("inv_"):
        inc = torch.rand((n - 1, L), dtype=torch.float64, device="cuda:0", generator=g) + 0.01
        c = torch.cat([torch.zeros((1, L), dtype=torch.float64, device="cuda:0"), torch.cumsum(inc, 0)])
        pad = torch.rand((2, L), dtype=torch.float64, device="cuda:0", generator=g) * 0.25
        y = ((-1.0 - pad[0]) + c / c[-1] * (2.0 + pad[0] + pad[1])).to(_tdt(dt))
    else:
        y = torch.randn((n, L), dtype=_tdt(dt), device="cuda:0", generator=g)
        if source.startswith("anti_"):
            y = y.abs()
    B = pkg.Interp1D.builder
    base = source.split("_")[-1]
    it = B(y).x(x).strategy(pkg.Pchip.new() if base == "pchip" else pkg.Linear.new()).build()
    if source.startswith("anti_"):
        it = it.antiderivative()
    if source.startswith("inv_"):
        it = it.inverse()
        N = it.strategy.data_table(device=True)
        assert bool((N[0] <= N[-1]).all())
        return it, float(N[0].max()), float(N[-1].min()), N
    return it, float(x[0]), float(x[-1]), x


def pool_of(dt, lo, hi, inner, seed):
    """K abscissae in [lo, hi]: both ends, `inner`, its two neighbouring floats, uniform values"""
    T = np.dtype(dt).type
    rng = np.random.default_rng(seed)
    lo, hi, inner = T(lo), T(hi), T(inner)
    assert lo < inner < hi
    p = np.concatenate([[lo, hi, inner, np.nextafter(inner, T(np.inf)), np.nextafter(inner, T(-np.inf))],
                        rng.uniform(lo, hi, K - 5)]).astype(dt)
    return np.clip(p, lo, hi)


def wide_case(pkg, source, dt, n, L, Q, seed):
    """(handle, xs (Q, L), ref (Q, L)) on the device: ONE row-wise call of the pool is the reference"""
    import torch
    it, lo, hi, aux = wide_handle(pkg, source, dt, n, L, seed)
    inner = float(aux[n // 2]) if not source.startswith("inv_") else 0.5 * (lo + hi)
    pool = torch.as_tensor(pool_of(dt, lo, hi, inner, seed), device="cuda:0")
    rows = it.interp_array(pool)
    assert tuple(rows.shape) == (K, L)
    g = torch.Generator(device="cuda:0").manual_seed(seed + 1)
    k = torch.randint(0, K, (Q, L), device="cuda:0", generator=g)
    if L >= K:
        k[0, :K] = torch.arange(K, device="cuda:0")                    # every pool value at least once
    xs = pool[k]
    ref = torch.gather(rows, 0, k)
    del rows, k
    return it, xs, ref


def lanewise_calls(capfd, it, xs, ref, what, expect):
    """the device call that owns its output (the kernel tests the queries: check=1) and the call into a caller's buffer (the
    pre-pass: check=0); `expect`: fragments of the plan line.  Returns the plan lines"""
    import torch
    lines = []
    with traced(capfd) as t:
        got = it.interp_lanewise(xs)
    same_bits(got, ref, what + ": own output")
    assert len(t.plans) == 1 and all(f in t.plans[0] for f in expect), (what, expect, t.plans)
    lines += t.plans
    del got
    buf = torch.full(tuple(xs.shape), 7.0, dtype=xs.dtype, device="cuda:0")
    with traced(capfd) as t:
        it.interp_lanewise_into(xs, buf)
    same_bits(buf, ref, what + ": a caller's buffer")
    assert len(t.plans) == 1 and all(f in t.plans[0] for f in expect), (what, expect, t.plans)
    return lines + t.plans


# ---- 1. rows against the grid step ------------------------------------------------------------------------------------------
FORWARD_EXPECT = {(0, 2): ("form=fused", "records=0"), (1, 2): ("form=fused", "records=1"),
                  (0, 1): ("form=two-kernel",), (1, 1): ("form=two-kernel",)}


def probe_grid(pkg, monkeypatch, capfd):
    """NDI_LANEWISE_WGS=1: the grid of 256 lanes x 4097 rows, one workgroup per CU"""
    monkeypatch.setenv("NDI_LANEWISE_WGS", "1")
    set_variant(monkeypatch, 0, 2)
    it, xs, ref = wide_case(pkg, "linear", np.float64, 5, 256, 4097, 1)
    g = grid_of(lanewise_calls(capfd, it, xs, ref, "probe", ("form=fused",))[0])
    assert g >= 1 and 2 * BLOCK * g <= 4097 * 256, g
    return g


def grid_step_shapes(g):
    """(L, Q, the relation of the step 256 g to L)"""
    s = BLOCK * g
    return ((s - 1, 5, lambda step, L: step == L + 1),      # step_rows = 1, step_lanes = 1
            (s, 4, lambda step, L: step == L),              # step_rows = 1, step_lanes = 0
            (s + 1, 3, lambda step, L: step == L - 1),      # step_rows = 0: a row longer than the launched grid, a carry in (almost) every trip
            (256, 2 * g + 1, lambda step, L: step == g * L))      # step_rows = g, step_lanes = 0


def run_grid_step_shape(pkg, monkeypatch, capfd, dt, L, Q, relation, sources=("linear", "pchip", "anti_pchip", "inv_pchip")):
    n = 5
    for source in sources:
        it, xs, ref = wide_case(pkg, source, dt, n, L, Q, L + Q)
        if source in ("linear", "pchip"):
            todo = [((r, m), FORWARD_EXPECT[(r, m)]) for r, m in VARIANTS]
        else:
            todo = [((0, 1), ("form=two-kernel",) if source.startswith("anti_") else ("form=inverse",))]
        for (records, mode), expect in todo:
            set_variant(monkeypatch, records, mode)
            what = f"{source} {np.dtype(dt).name} {n} x {L}, Q = {Q}, records = {records}, mode = {mode}"
            for ln in lanewise_calls(capfd, it, xs, ref, what, expect):
                grid = grid_of(ln)
                assert 2 * BLOCK * grid <= Q * L, (what, ln)          # every thread takes at least two trips
                assert relation(BLOCK * grid, L), (what, L, ln)
        del it, xs, ref


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", range(4))
def test_rows_against_the_grid_step(pkg, monkeypatch, capfd, dt, shape):
    g = probe_grid(pkg, monkeypatch, capfd)
    L, Q, relation = grid_step_shapes(g)[shape]
    run_grid_step_shape(pkg, monkeypatch, capfd, dt, L, Q, relation)


# ---- 2. the pre-pass beyond one trip ----------------------------------------------------------------------------------------
def run_prepass_case(pkg, capfd, source, dt, L):
    """Q = 3 rows of L lanes: lanewise_check_kernel's 4096 blocks cover 1 048 576 elements a trip, so row 2 is met in the
    third trip"""
    import torch
    n, Q = 3, 3
    assert Q * L > 2 * 4096 * BLOCK
    it, xs, ref = wide_case(pkg, source, dt, n, L, Q, L)
    form = "form=inverse" if source.startswith("inv_") else "form=fused"
    what = f"{source} {np.dtype(dt).name} {n} x {L}"
    buf = torch.full((Q, L), 7.0, dtype=_tdt(dt), device="cuda:0")
    with traced(capfd) as t:
        it.interp_lanewise_into(xs, buf)                                # without `fresh`: the pre-pass runs
    assert len(t.plans) == 1 and form in t.plans[0] and "check=0" in t.plans[0], t.plans
    same_bits(buf, ref, what + ": the good batch")
    # the only bad elements: (2, 5) and (2, 900000)
    T = np.dtype(dt).type
    if source.startswith("inv_"):
        N = it.strategy.data_table(device=True)
        bad = float(np.nextafter(T(float(N[-1, 5])), T(np.inf)))        # one float above lane 5's OWN upper limit
    else:
        bad = float(np.nextafter(T(float(xs.max())), T(np.inf)))        # the pool holds the last knot
    qq = xs.clone()
    qq[2, 5] = bad
    qq[2, 900000] = float("-inf")
    buf.fill_(7.0)
    with traced(capfd) as t:
        with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
            it.interp_lanewise_into(qq, buf)
    assert len(t.plans) == 1 and "check=0" in t.plans[0], t.plans
    assert e.value.index == 2 * L + 5 and e.value.value == bad, (what, e.value.index, e.value.value, bad)
    same_bits(buf[:2], ref[:2], what + ": the rows before the failing row")
    assert bool((buf[2] == 7.0).all()), what + ": the failing row keeps the sentinel"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("L", [1_048_575, 1_048_576, 1_048_577])
def test_the_prepass_beyond_one_trip(pkg, monkeypatch, capfd, dt, L):
    monkeypatch.delenv("NDI_LANEWISE_RECORDS", raising=False)
    monkeypatch.delenv("NDI_LANEWISE_MODE", raising=False)
    for source in ("linear", "pchip", "inv_linear"):
        run_prepass_case(pkg, capfd, source, dt, L)


# ---- 3. AUTO ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,n,L,expect", [
    ("linear", 40001, 1, ("form=two-kernel", "kind=0")),                # scalar Linear on an axis beyond LDS
    ("linear", 40001, 3, ("form=fused", "stage=0", "records=0")),
    ("linear", 180001, 3, ("form=fused", "records=1")),                 # a 4.3 MB data table: above the 4 MiB of L2
    ("pchip", 33, 63, ("form=fused", "records=1")),                     # rows shorter than a wavefront
    ("pchip", 33, 64, ("form=fused", "records=0")),
    ("linear", 257, 4, ("form=fused", "stage=1", "records=0")),
])
def test_auto_takes_the_measured_decisions(pkg, monkeypatch, capfd, source, n, L, expect):
    """DESIGN.md 4.19 with both knobs unset: records only below 64 lanes, Linear records only above a 4 MiB table, the
    two-kernel form only for scalar Linear on an axis beyond LDS -- and every one of them bit-exact against per_lane"""
    import torch
    monkeypatch.delenv("NDI_LANEWISE_RECORDS", raising=False)
    monkeypatch.delenv("NDI_LANEWISE_MODE", raising=False)
    rng = np.random.default_rng([n, L])
    x = ic.knots(rng, n, np.float64)
    it = forward(pkg, source, x, data_for(source, rng, n, L, np.float64))
    Q = 257
    xs = lane_queries(rng, x, Q, L)
    ref = per_lane(it, xs)
    what = f"AUTO {source} {n} x {L}"
    with traced(capfd) as t:
        hostile_inputs.check_bits(it.interp_lanewise(xs), ref, what + ": host")
        hostile_inputs.check_bits(it.interp_lanewise(torch.as_tensor(xs, device="cuda:0")).cpu().numpy(), ref, what + ": device")
    assert len(t.plans) == 2 and all(all(f in ln for f in expect) for ln in t.plans), (what, expect, t.plans)


# ---- 4. the unstaged axis at f32 ----------------------------------------------------------------------------------------------
def test_an_axis_beyond_the_lds_budget_f32(pkg, monkeypatch, capfd):
    """test_gpu_lanewise.py's test_an_axis_beyond_the_lds_budget at f32: 40001 f32 knots and their 40 top-level entries are
    160 164 bytes, above the 150 KiB stage limit"""
    rng = np.random.default_rng(2)
    n, L = 40001, 3
    x = ic.knots(rng, n, np.float32)
    for source in ("linear", "pchip"):
        it = forward(pkg, source, x, data_for(source, rng, n, L, np.float32))
        for Q, lut in ((257, "lut=0"), (1400, "lut=2")):
            xs = lane_queries(rng, x, Q, L)
            ref = per_lane(it, xs)
            monkeypatch.setenv("NDI_TRACE_PLAN", "1")
            capfd.readouterr()
            all_variants(pkg, monkeypatch, it, xs, ref, f"{source} 40001 x 3 f32, Q = {Q}")
            plans = [ln for ln in capfd.readouterr().err.splitlines() if "lanewise form=fused" in ln]
            monkeypatch.delenv("NDI_TRACE_PLAN")
            assert plans and all("stage=0" in ln and lut in ln for ln in plans), plans
            assert any("records=1" in ln for ln in plans) and any("records=0" in ln for ln in plans), plans


# ---- 5. the record cap --------------------------------------------------------------------------------------------------------
def test_the_record_cap(pkg, monkeypatch, capfd):
    """Pchip f64, 3 x 16 777 217: the record copy would be 2 x 16 777 217 x 32 bytes, one record over
    LanewiseRecords::LIMIT = 1 GiB, so NDI_LANEWISE_RECORDS=1 still reads the plain tables (records=0)"""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    assert free > 12 * 2**30, "the test needs 12 GB of free device memory"
    monkeypatch.setenv("NDI_LANEWISE_RECORDS", "1")
    monkeypatch.delenv("NDI_LANEWISE_MODE", raising=False)
    n, L, Q = 3, 16_777_217, 2
    assert (n - 1) * L * 4 * 8 == (1 << 30) + 64
    it, xs, ref = wide_case(pkg, "pchip", np.float64, n, L, Q, 5)
    with traced(capfd) as t:
        got = it.interp_lanewise(xs)
    assert len(t.plans) == 1 and "form=fused" in t.plans[0] and "records=0" in t.plans[0], t.plans
    same_bits(got, ref, "above the record cap")
    with traced(capfd) as t:                     # and no later call retries
        got = it.interp_lanewise(xs)
    assert len(t.plans) == 1 and "records=0" in t.plans[0], t.plans
    same_bits(got, ref, "above the record cap, second call")
    del got, xs, ref
    it.strategy.release()
    torch.cuda.empty_cache()


# ---- 6. host staging in two chunks ----------------------------------------------------------------------------------------------
def test_host_staging_in_two_chunks(pkg, monkeypatch, capfd):
    """Linear f32 on scalar data, Q = 2^26 + 1000 host queries: a chunk of lanewise_run is 256 MiB = 2^26 rows of 4 bytes,
    so the loop runs with off = 2^26 (two plan lines)"""
    monkeypatch.delenv("NDI_LANEWISE_RECORDS", raising=False)
    monkeypatch.delenv("NDI_LANEWISE_MODE", raising=False)
    rng = np.random.default_rng(6)
    n, Q = 5, (1 << 26) + 1000
    x = ic.knots(rng, n, np.float32)
    y = rng.normal(size=n).astype(np.float32)
    it = pkg.Interp1D.builder(y).x(x).strategy(pkg.Linear.new()).build()
    q = rng.random(Q, dtype=np.float32) * (x[-1] - x[0]) + x[0]
    np.clip(q, x[0], x[-1], out=q)
    q[:3] = [x[0], x[-1], x[2]]
    q[(1 << 26) - 1:(1 << 26) + 2] = [x[1], x[-1], x[0]]
    ref = it.interp_array(q)
    assert ref.shape == (Q,)
    with traced(capfd) as t:
        got = it.interp_lanewise(q)
    assert len(t.plans) == 2 and all("form=fused" in ln for ln in t.plans), t.plans
    hostile_inputs.check_bits(got, ref, "two chunks")
    del got
    bad = (1 << 26) + 7
    q[bad] = np.nextafter(x[-1], np.float32(np.inf))
    q[bad + 100] = np.nan
    buf = np.full(Q, 7.0, np.float32)
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        it.interp_lanewise_into(q, buf)
    assert e.value.index == bad and e.value.value == float(q[bad]), (e.value.index, e.value.value)
    hostile_inputs.check_bits(buf[:bad], ref[:bad], "the rows before the failing query, across the chunk boundary")
    assert np.all(buf[bad:] == 7.0)


# ---- 7. inverse_eval_kernel past its grid ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("source,L,free_gb", [("inv_pchip", 64, 6), ("inv_linear", 1024, 40)])
def test_inverse_rows_past_the_grid(pkg, capfd, source, L, free_gb):
    """inverse_eval_kernel caps its grid at 2^20 blocks of 256 threads.  64 lanes x 4 194 305 queries are 2^28 + 64 elements:
    the stride loop takes a second trip.  1024 lanes x 4 194 305 are 2^32 + 1024: the 64-bit division branch.  Reference:
    the same handle in slices of 65 536 queries, each a single trip"""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    assert free > free_gb * 2**30, f"the test needs {free_gb} GB of free device memory"
    dt, n, Q, S = np.float32, 5, 4_194_305, 65_536
    assert Q * L > (1 << 20) * BLOCK and (L < 1024 or Q * L > 1 << 32)
    it, lo, hi, _ = wide_handle(pkg, source, dt, n, L, 7)
    g = torch.Generator(device="cuda:0").manual_seed(8)
    q = (torch.rand(Q, dtype=torch.float32, device="cuda:0", generator=g) * (hi - lo) + lo).clamp(lo, hi)
    q[0], q[1], q[Q - 1] = lo, hi, hi
    out = torch.full((Q, L), 7.0, dtype=torch.float32, device="cuda:0")
    with traced(capfd) as t:
        it.interp_array_into(q, out)
    assert len(t.plans) == 1 and grid_of(t.plans[0]) == 1 << 20, t.plans
    buf = torch.empty((S, L), dtype=torch.float32, device="cuda:0")
    for a in range(0, Q, S):
        b = min(a + S, Q)
        with traced(capfd) as t:
            it.interp_array_into(q[a:b], buf[:b - a])
        assert len(t.plans) == 1 and grid_of(t.plans[0]) * BLOCK >= (b - a) * L, t.plans      # a single trip
        assert torch.equal(out[a:b].view(torch.int32), buf[:b - a].view(torch.int32)), f"{source} x {L}: slice at {a}"
    # a value outside the range in the last slice
    q[Q - 1] = float(np.nextafter(np.float32(hi), np.float32(np.inf)))
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        it.interp_array_into(q, out)
    assert e.value.index == Q - 1 and e.value.value == float(q[Q - 1]), (e.value.index, e.value.value)
    del out, buf, q
    it.strategy.release()
    torch.cuda.empty_cache()


# ---- 8. the bounds-checked library ----------------------------------------------------------------------------------------------
def test_wide_rows_one_case_per_kernel_class(pkg, monkeypatch, capfd):
    """what runs again under the bounds-checked library (below): a row longer than the launched grid (f64) and one lane
    shorter than it (f32) through every kernel class -- the fused kernel with records and plain tables, the two-kernel form
    of Linear, the cubic class and both antiderivative classes, the inverse kernels -- and the 1 048 577-lane pre-pass"""
    g = probe_grid(pkg, monkeypatch, capfd)
    shapes = grid_step_shapes(g)
    sources = ("linear", "pchip", "anti_pchip", "anti_linear", "inv_pchip", "inv_linear")
    run_grid_step_shape(pkg, monkeypatch, capfd, np.float64, *shapes[2], sources=sources)
    run_grid_step_shape(pkg, monkeypatch, capfd, np.float32, *shapes[0], sources=sources)
    monkeypatch.delenv("NDI_LANEWISE_RECORDS", raising=False)
    monkeypatch.delenv("NDI_LANEWISE_MODE", raising=False)
    monkeypatch.delenv("NDI_LANEWISE_WGS", raising=False)
    for source in ("linear", "pchip", "inv_linear"):
        run_prepass_case(pkg, capfd, source, np.float64, 1_048_577)


def test_the_bounds_checked_library_runs_clean():
    """the NDI_CHK on p.j / p.l of every lane-wise kernel is what would catch a bad carry of LanewisePos::advance"""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_lanewise_plans.py"), "-m", "gpu", "-x", "-q",
                        "-k", "test_wide_rows_one_case_per_kernel_class"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
