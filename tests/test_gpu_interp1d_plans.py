"""GPU: every form the 1-D planner (csrc/interp1d_host.hpp: plan_lanes1, plan_small1, plan_fused1 and its legs, the grouping
decision, the two-kernel forms) can choose, each at the smallest shape of the launch A/B matrix (tools/launch_trace_ab.py,
cases_1d) that reaches it, for Linear and CubicSpline in f32 and f64, against the CPU oracle bit for bit AND -- where the
library prints one -- against the `[ndi plan]` line, so a case cannot silently stop reaching the kernel it exists for.  SMALL,
ROWS, FLAT and both BUCKETED forms print no line: they are pinned by their bits, by the absence of every other form's line and
by the library's own counters (profile_read: evaluation, search and grouping launches, the path taken).

Device queries, once through interp_array (a fresh output: no range pre-pass where the kernel tests the range itself) and once
through interp_array_into (a caller-owned buffer).  One first-error case per form: a query out of range in the middle of the
batch without extrapolation -- the error names it, the rows before it are written and the caller's sentinel stays in every
row from it on."""
import os
import re

import numpy as np
import pytest

import oracle
from test_gpu_bilinear_plans import SENTINEL, dev, expect_plan, tdt, torch_mask, vn
from test_gpu_parity import blocked_build, check_equal, knots

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
KINDS = ["linear", "cubic"]
LANES = {"NDI_LANES_KERNEL": "1"}
FUSED = {"NDI_SHORT_MODE": "2"}
FLAT = {"NDI_SHORT_MODE": "1"}
SORTED = {"NDI_SHORT_MODE": "2", "NDI_FUSED_SORTED": "1", "NDI_FUSED_LDS": "0"}
PLAN = re.compile(r"^\[ndi plan\] (lanes|fused sorted|fused|ring bucketed) (.*)$", re.M)
# what profile_read counts for the forms that print no line: evaluation, search and grouping launches, the path.  (The range
# pre-pass counts as a search: SMALL always has one.)
QUERY_ORDER = {"eval_launches": 1, "locate_launches": 1, "group_launches": 0, "last_path": "gather"}
GROUPED = {"eval_launches": 1, "locate_launches": 1, "group_launches": 1, "last_path": "bucketed"}


def traced(pkg, capfd, env, call):
    """(result or the exception, plans, counters): the call under NDI_TRACE_PLAN and the live variables `env`, all restored
    afterwards; plans = [(form, {field: text})] of every 1-D plan line it printed, in order; counters = profile_read over it"""
    import torch
    capfd.readouterr()
    env = dict(env, NDI_TRACE_PLAN="1")
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    pkg.profile_enable(True)
    pkg.profile_read(True)
    try:
        try:
            r = call()
        except Exception as e:      # (handed back: the first-error cases look at it)
            r = e
        torch.cuda.synchronize()
        prof = pkg.profile_read(True)
    finally:
        pkg.profile_enable(False)
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    err = capfd.readouterr().err
    other = [ln for ln in err.splitlines() if ln.startswith("[ndi plan]") and not PLAN.match(ln)]
    assert not other, f"a plan line of another family: {other}"
    plans = [(m.group(1), dict(f.split("=", 1) for f in m.group(2).split())) for m in PLAN.finditer(err)]
    return r, plans, {k: prof[k] for k in QUERY_ORDER}


class Case:
    """One table, its queries and the oracle's rows, computed once."""

    def __init__(self, pkg, dt, kind, n, lanes, nq, path="AUTO"):
        self.pkg, self.dt, self.lanes, self.nq = pkg, dt, lanes, nq
        rng = np.random.default_rng(n * 13 + lanes * 7 + (kind == "cubic"))
        self.x = x = knots("lin", n, rng, dt)      # (the matrix's axis: uniform -- the exact O(1) guess where it is exact)
        y = rng.uniform(-1, 1, (n, lanes)).astype(dt)
        q = rng.uniform(x[0], x[-1], nq).astype(dt).clip(x[0], x[-1])
        k = min(n, nq - 2)
        q[:k] = x[:k]                       # knot hits
        q[k:k + 2] = [x[-1], x[0]]          # the last interval's right end, the first one's left end
        self.q = q
        if kind == "cubic":
            _, a, b = oracle.cubic_build(x, y)
            self.ref = oracle.interp1d_cubic(x, y, a, b, q)[2].reshape(nq, lanes)
            # (many knots on a narrow trailing axis: the blocked build is the one form that is not the oracle's bits)
            strat = pkg.CubicSpline.new().reference_order() if blocked_build(n, lanes) else pkg.CubicSpline.new()
        else:
            self.ref = oracle.interp1d_linear(x, y, q)[2].reshape(nq, lanes)
            strat = pkg.Linear.new()
        self.it = pkg.Interp1DBuilder.new(dev(y)).x(dev(x)).strategy(strat).build()
        self.it.strategy.path = getattr(pkg, "PATH_" + path)

    def buffer(self, kind="aligned"):
        import torch
        nq, C = self.nq, self.lanes
        if kind == "aligned":
            flat = torch.full((nq * C,), SENTINEL, dtype=tdt(self.dt), device="cuda:0")
            return flat, flat.view(nq, C)
        flat = torch.full((nq * C + 2,), SENTINEL, dtype=tdt(self.dt), device="cuda:0")   # contiguous rows, the base one
        return flat, flat[1:1 + nq * C].view(nq, C)                                       # element past a 16-byte boundary

    def check(self, capfd, env, what, forms, out="aligned", counters=None, **fields):
        """fresh output and caller-owned buffer: bits, the plan lines (or the counters), nothing written around the rows"""
        pkg, it, q = self.pkg, self.it, dev(self.q)
        if out == "aligned":
            rows, plans, prof = traced(pkg, capfd, env, lambda: it.interp_array(q))
            assert not isinstance(rows, Exception), f"{what} fresh: {rows!r}"
            expect_plan(plans, f"{what} fresh", forms, **dict(fields, **({"prepass": 0} if "prepass" in fields else {})))
            check_equal(rows.cpu().numpy().reshape(self.nq, self.lanes), self.ref, f"{what} fresh")
            assert counters is None or prof == counters, f"{what} fresh: counters {prof} where {counters} was expected"
        flat, view = self.buffer(out)
        r, plans, prof = traced(pkg, capfd, env, lambda: it.strategy.interp_array_into(it, q, view))
        assert not isinstance(r, Exception), f"{what} into: {r!r}"
        expect_plan(plans, f"{what} into", forms, **fields)
        check_equal(view.cpu().numpy(), self.ref, f"{what} into")
        assert counters is None or prof == counters, f"{what} into: counters {prof} where {counters} was expected"
        written = torch_mask(flat, view)
        assert bool((flat[~written] == SENTINEL).all()), f"{what}: elements around the caller's rows were written"

    def check_first_error(self, capfd, env, what, forms):
        """out of range at nq // 2 (a later NaN must not be the one reported): the same error from both entry points, the
        rows before it written, the sentinel in every row from it on"""
        pkg, it, pos = self.pkg, self.it, self.nq // 2
        q = self.q.copy()
        q[pos] = self.x[-1] + self.dt(1)
        q[pos + 7] = np.nan
        dq = dev(q)

        def named(e):
            return isinstance(e, pkg.InterpolateError.OutOfBounds) and e.index == pos and \
                re.fullmatch(r"x = \S+ is not in range", str(e)) and "NaN" not in str(e)
        e, plans, _ = traced(pkg, capfd, env, lambda: it.interp_array(dq))
        assert named(e), f"{what} fresh: {e!r}"
        expect_plan(plans, f"{what} fresh, first error", forms)
        flat, view = self.buffer()
        e, plans, _ = traced(pkg, capfd, env, lambda: it.strategy.interp_array_into(it, dq, view))
        assert named(e), f"{what} into: {e!r}"
        expect_plan(plans, f"{what} into, first error", forms)
        got = view.cpu().numpy()
        check_equal(got[:pos], self.ref[:pos], f"{what}: rows before the failure")
        assert np.all(got[pos:] == SENTINEL), f"{what}: rows from the failure on keep the sentinel"


both = pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
kinds = pytest.mark.parametrize("kind", KINDS)


# ---- SMALL: search and evaluation in one launch, a query per thread (no plan line) -------------------------------------------
@kinds
@both
def test_small(pkg, capfd, dt, kind):
    c = Case(pkg, dt, kind, 33, 1, 1000)
    c.check(capfd, {}, "SMALL", [], counters=QUERY_ORDER)
    c.check_first_error(capfd, {}, "SMALL", [])


# ---- LANES: the tables in LDS, a query per lane ------------------------------------------------------------------------------
@kinds
@both
def test_lanes_scalar_data(pkg, capfd, dt, kind):
    """L = 1: a 16-byte vector of queries per lane where the buffers allow it, else one"""
    c = Case(pkg, dt, kind, 33, 1, 4000)
    c.check(capfd, LANES, "LANES L=1 vector", ["lanes"], L=1, qpl=vn(dt), index="guess", tb=256, prepass=1)
    c.check(capfd, LANES, "LANES L=1 scalar", ["lanes"], out="unaligned", L=1, qpl=1, index="guess", tb=256, prepass=1)
    c.check_first_error(capfd, LANES, "LANES L=1", ["lanes"])


@pytest.mark.parametrize("lanes", [2, 4, 5, 8])
@kinds
@both
def test_lanes(pkg, capfd, dt, kind, lanes):
    c = Case(pkg, dt, kind, 33, lanes, 4000)
    c.check(capfd, LANES, f"LANES L={lanes}", ["lanes"], L=lanes, qpl=1, index="guess", tb=256, prepass=1)
    if lanes in (2, 5):
        c.check_first_error(capfd, LANES, f"LANES L={lanes}", ["lanes"])


@pytest.mark.parametrize("lanes", [1, 2])
@kinds
@both
def test_lanes_1024_threads(pkg, capfd, dt, kind, lanes):
    """tables of more than 40 KiB: four workgroups of 256 no longer fit a CU -- one of 1024"""
    big = 1024 if (dt == np.float64 and kind == "cubic") else 2048
    n = big if lanes == 1 or (kind == "linear" and dt == np.float32) else big // 2
    c = Case(pkg, dt, kind, n, lanes, 5000)
    c.check(capfd, LANES, f"LANES tables > 40 KiB L={lanes}", ["lanes"], L=lanes, qpl=vn(dt) if lanes == 1 else 1, tb=1024, prepass=1)


# ---- FUSED: query order with the search fused in -----------------------------------------------------------------------------
@kinds
@both
def test_fused_tables(pkg, capfd, dt, kind):
    """rows of 8 vectors on 33 knots: the tables from memory (a batch this small does not pay for staging them), {y, a, b} in
    LDS when pinned, {y, k} in LDS for the spline, whose build kept k; unaligned rows take the scalar instance"""
    c = Case(pkg, dt, kind, 33, 8 * vn(dt), 4000)
    c.check(capfd, FUSED, "FUSED tables=memory", ["fused"], tables="memory", lut=0, pack=0, unr=2, tb=256, prepass=1)
    c.check(capfd, dict(FUSED, NDI_FUSED_LDS="1"), "FUSED lds{y,a,b}", ["fused"], tables="lds{y,a,b}", tb=1024, prepass=1)
    c.check(capfd, dict(FUSED, NDI_FUSED_LDS="2"), "FUSED lds{y,k}", ["fused"],
            tables="lds{y,k}" if kind == "cubic" else "lds{y,a,b}", tb=1024, prepass=1)
    c.check(capfd, FUSED, "FUSED unaligned", ["fused"], out="unaligned", tables="memory", pack=0, tb=256, prepass=1)
    c.check_first_error(capfd, FUSED, "FUSED tables=memory", ["fused"])
    c.check_first_error(capfd, dict(FUSED, NDI_FUSED_LDS="1"), "FUSED lds{y,a,b}", ["fused"])


@pytest.mark.parametrize("pack", [0, 1])
@kinds
@both
def test_fused_packed_rows(pkg, capfd, dt, kind, pack):
    """rows shorter than a cache line: one interval-packed record per item, or the three row pieces"""
    c = Case(pkg, dt, kind, 33, 2 * vn(dt), 4000)
    env = dict(FUSED, NDI_FUSED_LDS="0", NDI_FUSED_PACK=str(pack))
    c.check(capfd, env, f"FUSED pack={pack}", ["fused"], tables="memory", pack=pack, prepass=1)
    c.check_first_error(capfd, env, f"FUSED pack={pack}", ["fused"])


@kinds
@both
def test_fused_knots_global(pkg, capfd, dt, kind):
    """the pyramid exceeds what the kernel stages: the knots stay in global memory behind the u32 bucket index"""
    c = Case(pkg, dt, kind, 40000 if dt == np.float32 else 20000, 2 * vn(dt), 4096)
    c.check(capfd, FUSED, "FUSED knots=global", ["fused"], tables="memory,knots=global", lut=0, pack=1, unr=2, tb=256, prepass=1)
    c.check(capfd, FUSED, "FUSED knots=global scalar", ["fused"], out="unaligned", tables="memory,knots=global", tb=256, prepass=1)
    c.check_first_error(capfd, FUSED, "FUSED knots=global", ["fused"])


@kinds
@both
def test_fused_sorted(pkg, capfd, dt, kind):
    """rows of 64 bytes on 257 knots: a workgroup round ordered by interval in LDS"""
    c = Case(pkg, dt, kind, 257, 64 // np.dtype(dt).itemsize, 8192)
    c.check(capfd, SORTED, "FUSED sorted", ["fused sorted"], lut=0, tb=512, prepass=1)
    c.check(capfd, SORTED, "FUSED sorted scalar", ["fused sorted"], out="unaligned", lut=0, tb=512, prepass=1)
    c.check_first_error(capfd, SORTED, "FUSED sorted", ["fused sorted"])


# ---- the two-kernel forms (no plan line) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cq", [16, 64])
@kinds
@both
def test_bucketed_short(pkg, capfd, dt, kind, cq):
    c = Case(pkg, dt, kind, 17, 16 * vn(dt), 3000, "BUCKETED")
    env = {"NDI_SHORT_CQ": str(cq)}
    c.check(capfd, env, f"BUCKETED_SHORT cq={cq}", [], counters=GROUPED)
    c.check_first_error(capfd, env, f"BUCKETED_SHORT cq={cq}", [])


@kinds
@both
def test_bucketed(pkg, capfd, dt, kind):
    c = Case(pkg, dt, kind, 9, 256 * vn(dt), 300, "BUCKETED")
    c.check(capfd, {}, "BUCKETED", [], counters=GROUPED)
    c.check_first_error(capfd, {}, "BUCKETED", [])


@kinds
@both
def test_rows(pkg, capfd, dt, kind):
    c = Case(pkg, dt, kind, 9, 256 * vn(dt), 300, "GATHER")
    c.check(capfd, {}, "ROWS", [], counters=QUERY_ORDER)
    c.check_first_error(capfd, {}, "ROWS", [])


@pytest.mark.parametrize("lanes", [3, 8])
@kinds
@both
def test_flat(pkg, capfd, dt, kind, lanes):
    c = Case(pkg, dt, kind, 33, lanes, 3000, "GATHER")
    c.check(capfd, FLAT, f"FLAT L={lanes}", [], counters=QUERY_ORDER)
    c.check_first_error(capfd, FLAT, f"FLAT L={lanes}", [])
