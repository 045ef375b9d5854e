"""GPU: every form the 2-D Bilinear planner (csrc/bilinear_host.hpp: plan_lanes2, plan_slopes2, plan_small2, plan_fused2, the
tile decision, the gather order) can choose, each at the smallest shape of the launch A/B matrix (tools/launch_trace_ab.py)
that reaches it, against the CPU oracle bit for bit AND -- where the library prints one -- against the `[ndi plan]` line, so a
case cannot silently stop reaching the kernel it exists for.  SMALL and the gather order print no line: they are pinned by
their bits and by the absence of every other form's line.

Both element types, device queries, once through interp_array (a fresh output: no range pre-pass where the kernel tests the
range itself) and once through interp_array_into (a caller-owned buffer).  One first-error case per form: a query out of
range in the middle of the batch without extrapolation -- the error names it, the rows before it are written and the
caller's sentinel stays in every row from it on."""
import os
import re

import numpy as np
import pytest

import oracle
from test_gpu_parity import check_equal, knots

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
SENTINEL = -7.0
OFF2 = {"NDI_LANES2D_KERNEL": "0", "NDI_SLOPES2D_KERNEL": "0"}
LANES2 = {"NDI_LANES2D_KERNEL": "1"}
SLOPES2 = {"NDI_SLOPES2D_KERNEL": "1", "NDI_LANES2D_KERNEL": "0"}
TWO_LEVEL = dict(OFF2, NDI_GROUP_TWO_LEVEL="1")
PLAN = re.compile(r"^\[ndi plan\] (lanes2d|slopes2d|fused2d|tiles|two-level grouping) (.*)$", re.M)


def vn(dt):
    return 16 // np.dtype(dt).itemsize          # elements of a 16-byte vector


def tdt(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.float32 else torch.float64


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def traced(capfd, env, call):
    """(result or the exception, plans): the call under NDI_TRACE_PLAN and the live variables `env`, all restored afterwards;
    plans = [(form, {field: text})] of every Bilinear plan line it printed, in order"""
    capfd.readouterr()
    env = dict(env, NDI_TRACE_PLAN="1")
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        try:
            r = call()
        except Exception as e:      # (handed back: the first-error cases look at it)
            r = e
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    err = capfd.readouterr().err
    other = [ln for ln in err.splitlines() if ln.startswith("[ndi plan]") and not PLAN.match(ln)]
    assert not other, f"a plan line of another family: {other}"
    return r, [(m.group(1), dict(f.split("=") for f in m.group(2).split())) for m in PLAN.finditer(err)]


def expect_plan(plans, what, forms, **fields):
    """exactly the lines `forms`, in order, and `fields` in the last of them (the evaluation's)"""
    assert [p[0] for p in plans] == list(forms), f"{what}: plan lines {plans} where {forms} was expected"
    if forms:
        got = {k: plans[-1][1].get(k) for k in fields}
        assert got == {k: str(v) for k, v in fields.items()}, f"{what}: plan {plans[-1]} where {fields} was expected"


class Case:
    """One grid, its queries and the oracle's rows, computed once."""

    def __init__(self, pkg, dt, nx, ny, lanes, nq, path="AUTO"):
        self.pkg, self.dt, self.lanes, self.nq = pkg, dt, lanes, nq
        rng = np.random.default_rng(nx * 13 + ny * 7 + lanes)
        self.x, self.y = knots("jit", nx, rng, dt), knots("jit", ny, rng, dt)
        self.g = rng.uniform(-1, 1, (nx, ny, lanes)).astype(dt)
        qx = rng.uniform(self.x[0], self.x[-1], nq).astype(dt).clip(self.x[0], self.x[-1])
        qy = rng.uniform(self.y[0], self.y[-1], nq).astype(dt).clip(self.y[0], self.y[-1])
        k = min(nx, ny, nq - 3)
        qx[:k] = self.x[:k]; qy[:k] = self.y[:k]                                          # grid-point hits
        qx[k:k + 3] = [self.x[-1], self.x[0], self.x[-1]]; qy[k:k + 3] = [self.y[-1], self.y[-1], self.y[0]]   # the last cells
        self.qx, self.qy = qx, qy
        self.ref = oracle.interp2d_bilinear(self.x, self.y, self.g, qx, qy)[3].reshape(nq, lanes)
        self.it = pkg.Interp2DBuilder.new(dev(self.g)).x(dev(self.x)).y(dev(self.y)).build()
        self.it.strategy.path = getattr(pkg, "PATH_" + path)

    def buffer(self, kind="aligned"):
        import torch
        nq, C = self.nq, self.lanes
        if kind == "aligned":
            flat = torch.full((nq * C,), SENTINEL, dtype=tdt(self.dt), device="cuda:0")
            return flat, flat.view(nq, C)
        if kind == "unaligned":        # contiguous rows, the base one element past a 16-byte boundary
            flat = torch.full((nq * C + 2,), SENTINEL, dtype=tdt(self.dt), device="cuda:0")
            return flat, flat[1:1 + nq * C].view(nq, C)
        flat = torch.full((nq * (C + 3),), SENTINEL, dtype=tdt(self.dt), device="cuda:0")      # strided: a row pitch wider than the row
        return flat, flat.view(nq, C + 3)[:, :C]

    def check(self, capfd, env, what, forms, out="aligned", **fields):
        """fresh output and caller-owned buffer: bits, the plan lines, and nothing written around the caller's rows"""
        it, qx, qy = self.it, dev(self.qx), dev(self.qy)
        if out == "aligned":
            rows, plans = traced(capfd, env, lambda: it.interp_array(qx, qy))
            assert not isinstance(rows, Exception), f"{what} fresh: {rows!r}"
            expect_plan(plans, f"{what} fresh", forms, **dict(fields, **({"prepass": 0} if "prepass" in fields else {})))
            check_equal(rows.cpu().numpy().reshape(self.nq, self.lanes), self.ref, f"{what} fresh")
        flat, view = self.buffer(out)
        r, plans = traced(capfd, env, lambda: it.strategy.interp_array_into(it, qx, qy, view))
        assert not isinstance(r, Exception), f"{what} into: {r!r}"
        expect_plan(plans, f"{what} into", forms, **fields)
        check_equal(view.cpu().numpy(), self.ref, f"{what} into")
        written = torch_mask(flat, view)
        assert bool((flat[~written] == SENTINEL).all()), f"{what}: elements around the caller's rows were written"

    def check_first_error(self, capfd, env, what, forms):
        """x out of range at nq // 2 (a later NaN in y must not be the one reported): the same error from both entry points,
        the rows before it written, the sentinel in every row from it on"""
        pkg, it, pos = self.pkg, self.it, self.nq // 2
        qx, qy = self.qx.copy(), self.qy.copy()
        qx[pos] = self.x[-1] + self.dt(1)
        qy[pos + 7] = np.nan
        dqx, dqy = dev(qx), dev(qy)
        e, plans = traced(capfd, env, lambda: it.interp_array(dqx, dqy))
        assert isinstance(e, pkg.InterpolateError.OutOfBounds) and (e.index, e.axis) == (pos, 0), f"{what} fresh: {e!r}"
        expect_plan(plans, f"{what} fresh, first error", forms)
        flat, view = self.buffer()
        e, plans = traced(capfd, env, lambda: it.strategy.interp_array_into(it, dqx, dqy, view))
        assert isinstance(e, pkg.InterpolateError.OutOfBounds) and (e.index, e.axis) == (pos, 0), f"{what} into: {e!r}"
        got = view.cpu().numpy()
        check_equal(got[:pos], self.ref[:pos], f"{what}: rows before the failure")
        assert np.all(got[pos:] == SENTINEL), f"{what}: rows from the failure on keep the sentinel"


def torch_mask(flat, view):
    """the elements of `flat` that `view` covers"""
    import torch
    mark = torch.zeros_like(flat, dtype=torch.bool)
    mark.as_strided(view.size(), view.stride(), view.storage_offset() - flat.storage_offset())[...] = True
    return mark


# ---- LANES2: the grid in LDS, a query per lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_lanes2(pkg, capfd, dt, lanes):
    c = Case(pkg, dt, 33, 17, lanes, 4000)
    c.check(capfd, LANES2, f"LANES2 L={lanes}", ["lanes2d"], L=lanes, qpl=vn(dt) if lanes == 1 else 1, tb=256, prepass=1)
    c.check_first_error(capfd, LANES2, f"LANES2 L={lanes}", ["lanes2d"])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_lanes2_1024_threads(pkg, capfd, dt):
    """120 x 120: four workgroups of 256 no longer fit a CU beside the grid -- one of 1024"""
    c = Case(pkg, dt, 120, 120, 1, 4000)
    c.check(capfd, LANES2, "LANES2 tb=1024", ["lanes2d"], L=1, qpl=vn(dt), tb=1024, prepass=1)


# ---- SLOPES2: slope records -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 4, 5])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_slopes2(pkg, capfd, dt, lanes):
    c = Case(pkg, dt, 40, 30, lanes, 3000)
    c.check(capfd, SLOPES2, f"SLOPES2 L={lanes}", ["slopes2d"], L=lanes, tb=256, prepass=1)
    for out in ("unaligned", "strided"):          # one value per lane with a row pitch / contiguous rows without 16-byte stores
        c.check(capfd, SLOPES2, f"SLOPES2 L={lanes} {out}", ["slopes2d"], out=out, L=lanes, tb=256, prepass=1)
    c.check_first_error(capfd, SLOPES2, f"SLOPES2 L={lanes}", ["slopes2d"])


# ---- SMALL: both searches and the evaluation in one launch, a query per thread (no plan line) --------------------------------
@pytest.mark.parametrize("nq", [1000, 5000], ids=["pyramids", "bucket-indices"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_small(pkg, capfd, dt, lanes, nq):
    """from 4096 queries the launch asks for the bucket indices and stages them when the axes have any"""
    c = Case(pkg, dt, 33, 17, lanes, nq)
    c.check(capfd, {}, f"SMALL L={lanes} nq={nq}", [])
    c.check_first_error(capfd, {}, f"SMALL L={lanes} nq={nq}", [])


# ---- FUSED2: query order with both searches fused in ------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [1, 0], ids=["vector", "scalar"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_fused2(pkg, capfd, dt, vec):
    lanes = 2 * vn(dt) if vec else 5
    c = Case(pkg, dt, 100, 100, lanes, 65536)
    c.check(capfd, OFF2, f"FUSED2 L={lanes}", ["fused2d"], vec=vec, lv=2 if vec else 5, prepass=1)
    c.check_first_error(capfd, OFF2, f"FUSED2 L={lanes}", ["fused2d"])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_fused2_long_axis(pkg, capfd, dt):
    """3000 knots: the staged axes leave no room for several workgroups of 256 -- a larger workgroup keeps more waves"""
    c = Case(pkg, dt, 3000, 40, 2 * vn(dt), 65536)
    c.check(capfd, OFF2, "FUSED2 long axis", ["fused2d"], vec=1, lv=2, lut=1, prepass=1)
    c.check_first_error(capfd, OFF2, "FUSED2 long axis", ["fused2d"])


# ---- TILED: the tile order (BUCKETED) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("vecs", [1, 8], ids=["whole-rows", "half-rows"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_tiled_one_pass(pkg, capfd, dt, vecs):
    """one-pass grouping; rows of one vector keep one workgroup per CU, rows of eight are split between two"""
    c = Case(pkg, dt, 65, 70, vecs * vn(dt), 5000, "BUCKETED")
    fields = dict(ts=6, split=1) if vecs == 1 else dict(ts=4, split=2)
    c.check(capfd, OFF2, f"TILED {vecs} vectors", ["tiles"], compact=int(dt == np.float32), **fields)
    c.check_first_error(capfd, OFF2, f"TILED {vecs} vectors", ["tiles"])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_tiled_two_levels(pkg, capfd, dt):
    c = Case(pkg, dt, 300, 280, 8 * vn(dt), 20000, "BUCKETED")
    forms = ["two-level grouping", "tiles"]
    c.check(capfd, TWO_LEVEL, "TILED two levels", forms, ts=4, split=2, compact=int(dt == np.float32))
    _, plans = traced(capfd, TWO_LEVEL, lambda: c.it.interp_array(dev(c.qx), dev(c.qy)))
    assert (plans[0][1]["ntx"], plans[0][1]["nty"]) == ("19", "18"), plans
    c.check_first_error(capfd, TWO_LEVEL, "TILED two levels", forms)


# ---- GATHER: the search, then the query-order kernel (no plan line) ---------------------------------------------------------
@pytest.mark.parametrize("vec", [1, 0], ids=["vector", "scalar"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_gather(pkg, capfd, dt, vec):
    lanes = 2 * vn(dt) if vec else 5
    c = Case(pkg, dt, 33, 17, lanes, 3000, "GATHER")
    c.check(capfd, OFF2, f"GATHER L={lanes}", [])
    c.check_first_error(capfd, OFF2, f"GATHER L={lanes}", [])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_gather_axes_outside_lds(pkg, capfd, dt):
    """the two pyramids do not fit LDS together (160 000 B of x knots alone): one search launch per axis, each with its own
    first-error slot -- x is reported before y for the same query"""
    c = Case(pkg, dt, 40000 if dt == np.float32 else 20000, 4, vn(dt), 3000, "GATHER")
    c.check(capfd, OFF2, "GATHER axes outside LDS", [])
    c.check_first_error(capfd, OFF2, "GATHER axes outside LDS", [])
    qx, qy, pos = c.qx.copy(), c.qy.copy(), 1500
    qy[pos] = c.y[0] - dt(1)
    qx[pos + 3] = c.x[-1] + dt(1)
    e, _ = traced(capfd, OFF2, lambda: c.it.interp_array(dev(qx), dev(qy)))
    assert isinstance(e, pkg.InterpolateError.OutOfBounds) and (e.index, e.axis) == (pos, 1), repr(e)
