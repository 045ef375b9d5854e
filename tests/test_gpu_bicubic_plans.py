"""GPU: every form the Bicubic launch planner (csrc/bicubic_host.hpp, bicubic_launch_eval) can choose, each against the
numpy restatement (tests/bicubic_ref.py) bit for bit AND against the plan line the library prints under NDI_TRACE_PLAN, so a
case cannot silently stop reaching the kernel form it exists for:

  knots in global memory (klds=0), the O(1) index guess accepted and rejected, one- and two-level pyramids with ragged last
  blocks, every short-row width through the magic division, long rows cut along blockIdx.y with ragged last pieces and the
  first-error semantics across pieces, a wave's second batch, strided and misaligned caller buffers, the empty batch.

Lanes are independent (one IEEE operation per element and line), so one restatement of a wide grid serves every narrower
handle built on a slice of its lanes.  Host and device queries, fresh output (interp_array) and caller-owned buffers
(interp_array_into)."""
import os
import re

import numpy as np
import pytest

import bicubic_ref
from hostile_inputs import check_bits
from test_gpu_bicubic import build, failure

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
PLAN = re.compile(r"\[ndi plan\] bicubic vec=(\d+) lv=(\d+) klds=(\d+) grid=(\d+) x (\d+) lds=(\d+) prepass=(\d+) "
                  r"guess=(\d+),(\d+) levels=(\d+),(\d+)")
FIELDS = ("vec", "lv", "klds", "gx", "gy", "lds", "prepass", "guess_x", "guess_y", "levels_x", "levels_y")
SENTINEL = -7.0


def vn(dt):
    return 16 // np.dtype(dt).itemsize          # elements of a 16-byte vector


def traced(capfd, call):
    """(result, plans): the call under NDI_TRACE_PLAN and the fields of every Bicubic plan line it printed"""
    capfd.readouterr()
    before = os.environ.get("NDI_TRACE_PLAN")
    os.environ["NDI_TRACE_PLAN"] = "1"
    try:
        r = call()
    finally:
        if before is None:
            del os.environ["NDI_TRACE_PLAN"]
        else:
            os.environ["NDI_TRACE_PLAN"] = before
    err = capfd.readouterr().err
    plans = [dict(zip(FIELDS, (int(v) for v in m.groups()))) for m in PLAN.finditer(err)]
    assert plans, f"no Bicubic plan line in: {err[-500:]}"
    return r, plans


def expect_plan(plans, what, **fields):
    for p in plans:
        got = {k: p[k] for k in fields}
        assert got == fields, f"{what}: plan {p} where {fields} was expected"


def dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


def to_np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def sentinel_buffer(shape, dt, on_device):
    import torch
    if on_device:
        return torch.full(shape, SENTINEL, dtype=torch.float32 if np.dtype(dt) == np.float32 else torch.float64, device="cuda:0")
    return np.full(shape, SENTINEL, dt)


def run_all(it, qx, qy, want, capfd, what, fresh_device=None, **fields):
    """host and device queries x fresh output and caller-owned buffer: bits, and `fields` in every launch's plan.
    `fresh_device`: further fields of the fresh device output's plan, for the cases that are about that launch."""
    C = want.shape[1]
    for on_device in (False, True):
        q = (dev(qx), dev(qy)) if on_device else (qx, qy)
        rows, plans = traced(capfd, lambda: it.interp_array(*q))
        more = fresh_device if on_device and fresh_device else {}
        expect_plan(plans, f"{what} fresh device={on_device}", **fields, **more)
        check_bits(to_np(rows), want, f"{what} fresh device={on_device}")
        buf = sentinel_buffer((len(qx), C), want.dtype, on_device)
        _, plans = traced(capfd, lambda: it.interp_array_into(*q, buf))
        expect_plan(plans, f"{what} into device={on_device}", **fields)
        check_bits(to_np(buf), want, f"{what} into device={on_device}")
    return plans[-1]


def run_unaligned(it, qx, qy, want, capfd, what, **fields):
    """a caller-owned device buffer whose base is one element past a 16-byte boundary: the scalar form at any width"""
    nq, C = want.shape
    flat = sentinel_buffer((nq * C + 2,), want.dtype, True)
    view = flat[1:1 + nq * C].view(nq, C)
    _, plans = traced(capfd, lambda: it.strategy.interp_array_into(it, dev(qx), dev(qy), view))
    expect_plan(plans, what, vec=0, lv=C, **fields)
    h = to_np(flat)
    check_bits(h[1:1 + nq * C].reshape(nq, C), want, what)
    assert h[0] == SENTINEL and h[-1] == SENTINEL, f"{what}: the elements around the buffer were written"


def guess_of(k):
    """DevicePyramid::upload's predicate: every knot within 0.45 of a step of the evenly spaced axis through the ends"""
    step = (float(k[-1]) - float(k[0])) / (len(k) - 1)
    return int(bool(np.all(np.abs(k.astype(np.float64) - (float(k[0]) + step * np.arange(len(k)))) < 0.45 * step)))


def uneven(rng, n, dt):
    """the axis of the other Bicubic tests, drawn again until the host does not take it for evenly spaced"""
    while True:
        k = np.cumsum(rng.uniform(0.5, 1.5, n)).astype(dt)
        if not guess_of(k):
            return k


def near(k):
    """every knot, the float just below and just above each (clipped into range)"""
    T = k.dtype.type
    return np.clip(np.concatenate([k, np.nextafter(k, T(-np.inf)), np.nextafter(k, T(np.inf))]), k[0], k[-1]).astype(k.dtype)


def sweep(rng, x, y, n_random):
    """each axis' knots and their neighbours (the other coordinate walks through its own set), then random points"""
    sx, sy = near(x), near(y)
    qx = np.concatenate([sx, np.resize(sx, len(sy)), rng.uniform(x[0], x[-1], n_random)]).astype(x.dtype)
    qy = np.concatenate([np.resize(sy, len(sx)), sy, rng.uniform(y[0], y[-1], n_random)]).astype(y.dtype)
    return np.clip(qx, x[0], x[-1]), np.clip(qy, y[0], y[-1])


class Wide:
    """One wide grid and the restatement's tables; `handle(lo, hi)` builds on the lanes lo..hi and holds the device's
    tables to the restatement's, `rows` evaluates once for all lanes."""

    def __init__(self, pkg, rng, x, y, C):
        self.pkg, self.x, self.y = pkg, x, y
        self.z = rng.normal(size=(len(x), len(y), C)).astype(x.dtype)
        with np.errstate(all="ignore"):
            self.tabs = bicubic_ref.tables(x, y, self.z)

    def handle(self, lo, hi, what, **kw):
        it = build(self.pkg, self.x, self.y, np.ascontiguousarray(self.z[:, :, lo:hi]), **kw)
        for name, g, r in zip(("zx", "zy", "zxy"), it.strategy.tables(), self.tabs):
            check_bits(g, r[:, :, lo:hi], f"{what} lanes {lo}:{hi} {name}")
        return it

    def rows(self, qx, qy):
        with np.errstate(all="ignore"):
            return bicubic_ref.evaluate(self.x, self.y, self.z, *self.tabs, qx, qy)


# ---- knots in global memory -------------------------------------------------------------------------------------------------
GLOBAL_SHAPES = [(np.float64, 20_000, 3), (np.float64, 3, 20_000), (np.float32, 40_000, 5), (np.float32, 5, 40_000)]
SLICES_145 = ((0, 1), (1, 5), (5, 10))          # lanes 1, 4, 5 out of one grid of 10


@pytest.mark.parametrize("even", [False, True], ids=["uneven", "even"])
@pytest.mark.parametrize("dt,nx,ny", GLOBAL_SHAPES, ids=[f"{np.dtype(s[0]).name}-{s[1]}x{s[2]}" for s in GLOBAL_SHAPES])
def test_knots_in_global_memory(pkg, capfd, dt, nx, ny, even):
    """The two pyramids and the strips pass 153 600 B of LDS: KLDS=false, the search reads `const T*`, with the guess (exactly
    even knots) and without."""
    rng = np.random.default_rng(nx * 7 + ny)
    mk = (lambda n: np.arange(n).astype(dt)) if even else (lambda n: uneven(rng, n, dt))
    w = Wide(pkg, rng, mk(nx), mk(ny), 10)
    qx, qy = sweep(rng, w.x, w.y, 10_000)
    want = w.rows(qx, qy)
    for lo, hi in SLICES_145:
        C = hi - lo
        vec = int(C % vn(dt) == 0)
        it = w.handle(lo, hi, "global knots")
        run_all(it, qx, qy, want[:, lo:hi], capfd, f"global knots {nx}x{ny} C={C} even={even}", klds=0, vec=vec,
                lv=C // vn(dt) if vec else C, guess_x=int(even), guess_y=int(even), levels_x=1 + (nx > 64), levels_y=1 + (ny > 64))


# f64: the strips take 10 240 B, so the knots may take 143 360 B = 17 920 entries of both pyramids.  ny = 3 is 3 + 3
# entries; nx = 17 879 has a top level of ceil(17 879 / 512) = 35 entries: 17 879 + 35 + 6 = 17 920, the last shape that
# fits (lds = 153 600 exactly).  One knot more, and 64 more, do not.
@pytest.mark.parametrize("nx,klds", [(17_879, 1), (17_880, 0), (17_943, 0)])
def test_either_side_of_the_lds_limit(pkg, capfd, nx, klds):
    rng = np.random.default_rng(nx)
    w = Wide(pkg, rng, uneven(rng, nx, np.float64), uneven(rng, 3, np.float64), 5)
    qx, qy = sweep(rng, w.x, w.y, 10_000)
    want = w.rows(qx, qy)
    for lo, hi in ((0, 1), (1, 5)):
        it = w.handle(lo, hi, "lds limit")
        p = run_all(it, qx, qy, want[:, lo:hi], capfd, f"lds limit nx={nx} C={hi - lo}", klds=klds, vec=int(hi - lo == 4))
        assert p["lds"] == (153_600 if klds else 10_240), p


# ---- the index guess --------------------------------------------------------------------------------------------------------
def guess_axes(n, dt):
    """exactly even; even with one interior knot a few ulps up (the host still sets `guess`: queries just below that knot
    are guessed into its cell and rejected, the other lanes of the wave accepted); a step of 0.1, where
    (n-1)/(kn-k0)*(x-k0) rounds across an integer at knots"""
    T = np.dtype(dt).type
    even = np.arange(n).astype(dt)
    nudged = even.copy()
    for _ in range(3):
        nudged[n // 2] = np.nextafter(nudged[n // 2], T(np.inf))
    return (("even", even), ("nudged", nudged), ("tenths", (np.arange(n) * 0.1).astype(dt)))


@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("n", [3, 64, 65, 1000])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_index_guess(pkg, capfd, dt, n, axis):
    rng = np.random.default_rng(n + axis)
    other = uneven(rng, 4, dt)
    for name, k in guess_axes(n, dt):
        assert np.all(k[1:] > k[:-1])
        x, y = (k, other) if axis == 0 else (other, k)
        w = Wide(pkg, rng, x, y, 5)
        qx, qy = sweep(rng, x, y, 10_000)
        want = w.rows(qx, qy)
        for lo, hi in ((0, 1), (1, 5)):
            it = w.handle(lo, hi, f"guess {name}")
            run_all(it, qx, qy, want[:, lo:hi], capfd, f"guess {name} n={n} axis={axis} C={hi - lo}", klds=1,
                    guess_x=int(axis == 0), guess_y=int(axis == 1), vec=int(hi - lo == 4))


# ---- pyramid levels and ragged blocks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
@pytest.mark.parametrize("n", [64, 65, 66, 127, 128, 129, 4096, 4097])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_pyramid_levels_and_ragged_blocks(pkg, capfd, dt, n, axis):
    """DevicePyramid::upload doubles the block while 64 * block < n.  n = 64: the knots themselves are the top level; 65 .. 128:
    a second level over blocks of 2 knots, the last block full (66, 128) or of one knot (65, 127); 129: blocks of 4, the last of
    one knot; 4096: blocks of 64, all full; 4097: blocks of 128, the last of one knot."""
    rng = np.random.default_rng(n * 2 + axis)
    k, other = uneven(rng, n, dt), uneven(rng, 3, dt)
    x, y = (k, other) if axis == 0 else (other, k)
    w = Wide(pkg, rng, x, y, 5)
    qx, qy = sweep(rng, x, y, 0)
    want = w.rows(qx, qy)
    lv = {"levels_x" if axis == 0 else "levels_y": 1 if n <= 64 else 2, "levels_y" if axis == 0 else "levels_x": 1}
    for lo, hi in ((0, 1), (1, 5)):
        it = w.handle(lo, hi, "levels")
        run_all(it, qx, qy, want[:, lo:hi], capfd, f"levels n={n} axis={axis} C={hi - lo}", klds=1, guess_x=0, guess_y=0,
                vec=int(hi - lo == 4), **lv)


# ---- short rows: every lv ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_short_rows_every_lv(pkg, capfd, dt):
    """4 x 5 grid, lanes 1 .. 130, 130 queries (two waves, the second partial: nq_here * lv is no multiple of 64).  Aligned
    buffers give the vector form wherever the lanes divide; a misaligned caller buffer runs those widths through the scalar
    form as well, so every lv in 1 .. 63 divides by its magic multiplier in the scalar form, every lv the lanes allow in the
    vector form, and the first lv >= 64 take the long-row branch."""
    rng = np.random.default_rng(130)
    w = Wide(pkg, rng, uneven(rng, 4, dt), uneven(rng, 5, dt), 130)
    qx, qy = sweep(rng, w.x, w.y, 130 - 3 * 4 - 3 * 5)
    assert len(qx) == 130
    want = w.rows(qx, qy)
    seen = {0: set(), 1: set()}
    for C in range(1, 131):
        vec = int(C % vn(dt) == 0)
        lv = C // vn(dt) if vec else C
        it = w.handle(0, C, "short rows")
        run_all(it, qx, qy, want[:, :C], capfd, f"short rows C={C}", vec=vec, lv=lv, gx=1, gy=1, klds=1)
        seen[vec].add(lv)
        if vec:
            run_unaligned(it, qx, qy, want[:, :C], capfd, f"short rows C={C} unaligned", gx=1, gy=1)
            seen[0].add(C)
    assert seen[0] >= set(range(1, 131)), sorted(set(range(1, 131)) - seen[0])
    assert seen[1] == set(range(1, 130 // vn(dt) + 1)), sorted(seen[1])


# ---- long rows and pieces along y -------------------------------------------------------------------------------------------
LONG_LV = [64, 65, 127, 129, 511, 512, 513, 1024, 1025, 1537]


@pytest.fixture(scope="module", params=DTYPES, ids=DT_IDS)
def long_rows(pkg, request):
    """4 x 5 x (VN * 1537) and 200 queries: the restatement once per dtype"""
    dt = request.param
    rng = np.random.default_rng(1537)
    w = Wide(pkg, rng, uneven(rng, 4, dt), uneven(rng, 5, dt), vn(dt) * 1537)
    qx, qy = sweep(rng, w.x, w.y, 200 - 3 * 4 - 3 * 5)
    return dict(dt=dt, w=w, qx=qx, qy=qy, want=w.rows(qx, qy))


@pytest.mark.parametrize("lv", LONG_LV)
def test_long_rows_and_pieces_along_y(pkg, capfd, long_rows, lv):
    """lv >= 64: one query at a time, 64 vectors per trip with a tail (v < W); rows of more than 512 vectors are cut along
    blockIdx.y with a last piece of 1 (513, 1025, 1537) or 512 vectors.  The vector form at lanes = VN * lv; the scalar form
    at lanes = lv (odd lv: the lanes do not divide; even lv: a misaligned caller buffer)."""
    dt, w = long_rows["dt"], long_rows["w"]
    gy = -(-lv // 512)
    assert gy == {64: 1, 65: 1, 127: 1, 129: 1, 511: 1, 512: 1, 513: 2, 1024: 2, 1025: 3, 1537: 4}[lv]
    for C, vec in ((vn(dt) * lv, 1), (lv, 0)):
        it = w.handle(0, C, f"long rows lv={lv}")
        for nq in (1, 65, 200):
            qx, qy, want = long_rows["qx"][:nq], long_rows["qy"][:nq], long_rows["want"][:nq, :C]
            what = f"long rows lv={lv} vec={vec} nq={nq}"
            if vec or lv % 2:
                # a fresh device output is checked in the kernel, by the piece blockIdx.y == 0 alone: no pre-pass
                run_all(it, qx, qy, want, capfd, what, fresh_device=dict(prepass=0) if gy > 1 else None,
                        vec=vec, lv=lv, gx=1, gy=gy, klds=1)
            else:
                run_unaligned(it, qx, qy, want, capfd, what, gx=1, gy=gy, klds=1)


@pytest.mark.parametrize("lv", [513, 1025])
def test_first_error_across_pieces(pkg, long_rows, lv):
    """test_out_of_range_is_bilinears with gridDim.y > 1: only blockIdx.y == 0 range-checks a fresh output, and every piece
    of a caller-owned buffer stops at the first failing query.  The error is Bilinear's on the same queries."""
    import torch
    dt, w = long_rows["dt"], long_rows["w"]
    x, y, nq = w.x, w.y, 200
    tdt = torch.float32 if dt == np.float32 else torch.float64
    for C in (vn(dt) * lv, lv):
        z = np.ascontiguousarray(w.z[:, :, :C])
        bic = build(pkg, x, y, z)
        bil = pkg.Interp2DBuilder.new(z).x(x).y(y).build()
        want = long_rows["want"][:, :C]
        for kind in ("x_high", "y_low"):
            for pos in (0, nq // 2, nq - 1):
                qx, qy = long_rows["qx"].copy(), long_rows["qy"].copy()
                if kind == "x_high":
                    qx[pos] = x[-1] + dt(0.25)
                else:
                    qy[pos] = y[0] - dt(0.25)
                if pos + 7 < nq:
                    qy[pos + 7] = np.nan                   # a later failure must not be the one reported
                what = f"lv={lv} C={C} {kind} at {pos}"
                exp = failure(bil, qx, qy)
                assert exp[2] == pos and exp[4] == (1 if kind == "y_low" else 0), what
                assert failure(bic, qx, qy) == exp, what
                dqx, dqy = dev(qx), dev(qy)
                assert failure(bic, dqx, dqy) == exp, what
                for mk in (lambda: np.full((nq, C), SENTINEL, dt), lambda: torch.full((nq, C), SENTINEL, dtype=tdt, device="cuda:0")):
                    buf = mk()
                    q = (qx, qy) if isinstance(buf, np.ndarray) else (dqx, dqy)
                    assert failure(bic, *q, into=buf) == exp, what
                    rows = to_np(buf)
                    check_bits(rows[:pos], want[:pos], f"{what}: rows before the failure")
                    assert np.all(rows[pos:] == SENTINEL), f"{what}: rows from the failure on keep the sentinel in every piece"


# ---- a wave's second batch --------------------------------------------------------------------------------------------------
# f64 takes its second batch in the scalar form only: at 4 lanes (the vector form, VN = 2) 3 * 2^20 + 71 rows of f64 are
# 100 MB of output and twice the restatement's time, past what one test here may take; the f64 vector form's other paths
# are in every test above.
NQ_SECOND = 3 * 2**20 + 71
SECOND = [(np.float32, 9, 7, 1), (np.float32, 9, 7, 4), (np.float64, 9, 7, 1), (np.float32, 40_000, 5, 1), (np.float32, 40_000, 5, 4)]


@pytest.mark.parametrize("dt,nx,ny,C", SECOND, ids=[f"{np.dtype(s[0]).name}-{s[1]}x{s[2]}-C{s[3]}" for s in SECOND])
def test_second_batch_of_a_wave(pkg, capfd, dt, nx, ny, C):
    """More queries than gridDim.x * 256: waves come round (base += wave_step) and rewrite their strip after the closing
    wave barrier.  gridDim.x is at most cu_count * 8 * 4 = 8192 on a 256-CU device, below 3 * 2^20 + 71 queries / 256."""
    import torch
    rng = np.random.default_rng(nx + C)
    w = Wide(pkg, rng, uneven(rng, nx, dt), uneven(rng, ny, dt), C)
    it = w.handle(0, C, "second batch")
    bil = pkg.Interp2DBuilder.new(w.z).x(w.x).y(w.y).build()
    qx, qy = sweep(rng, w.x, w.y, NQ_SECOND - 3 * nx - 3 * ny)
    assert len(qx) == NQ_SECOND
    want = w.rows(qx, qy)
    p = run_all(it, qx, qy, want, capfd, f"second batch {nx}x{ny} C={C}", klds=int(nx < 40_000), gy=1, vec=int(C == 4))
    assert NQ_SECOND > p["gx"] * 256, p
    pos = p["gx"] * 256 + 1000                             # the first error, found by a wave in its second batch
    assert pos + 7 < NQ_SECOND
    qx[pos] = w.x[-1] + dt(0.25)
    qy[pos + 7] = np.nan
    exp = failure(bil, qx, qy)
    assert exp[2] == pos and exp[4] == 0
    dqx, dqy = dev(qx), dev(qy)
    assert failure(it, dqx, dqy) == exp
    buf = torch.full((NQ_SECOND, C), SENTINEL, dtype=torch.float32 if dt == np.float32 else torch.float64, device="cuda:0")
    assert failure(it, dqx, dqy, into=buf) == exp
    rows = to_np(buf)
    check_bits(rows[:pos], want[:pos], "rows before the failure")
    assert np.all(rows[pos:] == SENTINEL), "rows from the failure on keep the sentinel"


# ---- strided and misaligned caller buffers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 5, 64])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_strided_and_misaligned_buffers(pkg, capfd, dt, C):
    """64 x 48, 1000 queries into a view of a larger sentinel-filled buffer: a row stride of lanes + VN (the vector form when
    the lanes divide), of lanes + 1, and of lanes from a base one element in (both scalar).  Every gap element keeps the
    sentinel.  Device views with device queries, and the same strides as host views with host queries."""
    rng = np.random.default_rng(C)
    w = Wide(pkg, rng, uneven(rng, 64, dt), uneven(rng, 48, dt), C)
    it = w.handle(0, C, "strided")
    qx, qy = sweep(rng, w.x, w.y, 1000 - 3 * 64 - 3 * 48)
    nq = len(qx)
    assert nq == 1000
    want = w.rows(qx, qy)
    V = vn(dt)
    for name, stride, base, vec in (("lanes + VN", C + V, 0, int(C % V == 0)), ("lanes + 1", C + 1, 0, 0), ("base + 1", C, 1, 0)):
        for on_device in (True, False):
            flat = sentinel_buffer((nq * stride + base + 1,), dt, on_device)
            body = flat[base:base + nq * stride]
            view = (body.view(nq, stride) if on_device else body.reshape(nq, stride))[:, :C]
            q = (dev(qx), dev(qy)) if on_device else (qx, qy)
            _, plans = traced(capfd, lambda: it.strategy.interp_array_into(it, *q, view))
            what = f"{name} C={C} device={on_device}"
            if on_device:
                expect_plan(plans, what, vec=vec, lv=C // V if vec else C)
            h = to_np(flat)
            check_bits(h[base:base + nq * stride].reshape(nq, stride)[:, :C], want, what)
            gaps = np.ones(h.shape, bool)
            gaps[base:base + nq * stride].reshape(nq, stride)[:, :C] = False
            assert np.all(h[gaps] == SENTINEL), f"{what}: {int((h[gaps] != SENTINEL).sum())} gap elements were written"


# ---- the empty batch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_empty_batch(pkg, dt):
    import torch
    rng = np.random.default_rng(0)
    for C in (1, 4, 5):
        w = Wide(pkg, rng, uneven(rng, 4, dt), uneven(rng, 5, dt), C)
        it = w.handle(0, C, "empty")
        e = np.empty(0, dt)
        rows = it.interp_array(e, e)
        assert rows.shape == (0, C) and rows.dtype == np.dtype(dt)
        rows = it.interp_array(dev(e), dev(e))
        assert tuple(rows.shape) == (0, C)
        it.interp_array_into(e, e, np.empty((0, C), dt))
        it.interp_array_into(dev(e), dev(e), torch.empty((0, C), dtype=rows.dtype, device="cuda:0"))
        q = np.array([w.x[1]], dt), np.array([w.y[2]], dt)          # and the handle still evaluates
        check_bits(it.interp_array(*q), w.rows(*q), "after the empty batches")
