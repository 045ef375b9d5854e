"""GPU tests of the ring producer's group launches: the chunks of a 1-D ring evaluation whose slots are free
are evaluated by ONE launch of the long-row bucketed kernel (eval_bucketed_group_kernel) instead of one launch each.

Shapes: the smallest that still take the long-row bucketed plan (256 16-byte vectors per row and more) -- one FULL segment
with U = 1 (512 f64 / 1024 f32 lanes), U = 8 (4096 f64 lanes) and widths that are no whole segment (520 f64, 1032 f32
lanes), on 16 and on 300 knots; 5 chunks of 300 queries (no multiple of the kernel's 128-query pieces) with a ragged last
one of 137; 1, 2 and 3 slots as a striped ring and as separate buffers whose row pitch exceeds the row.  The plan and the
width of every launch are read from the `[ndi plan] ring bucketed` trace line, the launch counts from profile_read; every
row is compared bit for bit with interp_array_into of the same queries into one buffer (computed once per shape)."""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import knots

pytestmark = pytest.mark.gpu

CHUNK, Q = 300, 4 * 300 + 137
NCHUNKS = 5
#          dtype      lanes knots path
SHAPES = [(np.float64, 512, 16, "auto"),        # one FULL segment, U = 1; AUTO picks the bucketed plan (chunk >= 5 * 15)
          (np.float64, 4096, 300, "bucketed"),  # U = 8, FULL
          (np.float64, 520, 300, "bucketed"),   # 260 vectors: no whole segment
          (np.float32, 1024, 16, "auto"),       # f32: one FULL segment
          (np.float32, 1032, 300, "bucketed")]  # f32, 258 vectors
IDS = [f"{np.dtype(dt).name}-{L}-{n}" for dt, L, n, _ in SHAPES]
LINE = re.compile(r"^\[ndi plan\] ring bucketed L=(\d+) lv=(\d+) width=(\d+) nq=(\d+)$")

# what the producer must launch for 5 chunks (NDI_RING_GROUP: 0 one launch per chunk, 1 full-width groups from the start,
# 2 a narrow first launch), by number of slots
WIDTHS = {("0", 1): [1] * 5, ("0", 2): [1] * 5, ("0", 3): [1] * 5,
          ("1", 1): [1] * 5, ("1", 2): [2, 2, 1], ("1", 3): [3, 2],
          ("2", 1): [1] * 5, ("2", 2): [1, 2, 2], ("2", 3): [1, 3, 1]}

_cache = {}


def _case(pkg, dt, L, n, path):
    """The interpolator of a shape, its queries on the device and the reference rows (one interp_array_into), built once."""
    import torch
    key = (np.dtype(dt).name, L, n)
    if key not in _cache:
        rng = np.random.default_rng(4000 + L + n)
        x = knots("rand", n, rng, dt)
        y = rng.uniform(0.0, 1.0, (n, L)).astype(dt)
        interp = pkg.Interp1DBuilder.new(torch.as_tensor(y, device="cuda:0")).x(torch.as_tensor(x, device="cuda:0")) \
            .strategy(pkg.CubicSpline.new()).build()
        q = rng.uniform(x[0], x[-1], Q).astype(dt)
        qd = torch.as_tensor(q, device="cuda:0")
        ref = torch.empty((Q, L), dtype=qd.dtype, device="cuda:0")
        interp.interp_array_into(qd, ref)
        _cache[key] = (interp, x, y, q, qd, ref.cpu().numpy())
    interp = _cache[key][0]
    interp.strategy.path = pkg.PATH_BUCKETED if path == "bucketed" else pkg.PATH_AUTO
    return _cache[key]


def _ring(pkg, dt, L, n_slots, layout):
    import torch
    if layout == "striped":
        return pkg.striped_ring(CHUNK, L, n_slots, dt, 0)
    tdt = torch.float64 if np.dtype(dt) == np.float64 else torch.float32
    pitch = L + 16                         # separate buffers, row pitch > lanes (whole 16-byte vectors)
    return [torch.full((CHUNK, pitch), -7.0, dtype=tdt, device="cuda:0")[:, :L] for _ in range(n_slots)]


def _widths(capfd, L):
    """The widths of the ring's evaluation launches, from the trace; every launch took the long-row bucketed plan."""
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[ndi plan]")]
    assert lines and all(LINE.match(ln) for ln in lines), lines
    assert all(int(LINE.match(ln).group(1)) == L for ln in lines), lines
    return [int(LINE.match(ln).group(3)) for ln in lines]


def _gather(interp, qd, ring, shape, dt):
    """Runs the ring; the consumer copies every chunk out of its slot (stream-ordered: returns None)."""
    got = np.full(shape, np.nan, dtype=dt)
    seen = []

    def consumer(c, rows):
        assert tuple(rows.shape) == (c.q_count, shape[1]) and rows.data_ptr() == c.out
        got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
        seen.append((c.index, c.q_begin, c.q_count, c.slot))
    interp.interp_array_ring(qd, CHUNK, consumer, slots=ring)
    return got, seen


@pytest.mark.parametrize("dt,L,n,path", SHAPES, ids=IDS)
def test_groups_equal_one_batch(pkg, capfd, monkeypatch, dt, L, n, path):
    """Rows gathered from the slots are bit-equal to one interp_array_into, with groups in either producer order, with
    the knob forcing one launch per chunk and with the default; the trace shows the widths the slots allow."""
    interp, x, y, q, qd, ref = _case(pkg, dt, L, n, path)
    monkeypatch.setenv("NDI_TRACE_PLAN", "1")
    pkg.profile_enable(True)
    try:
        for n_slots in (1, 2, 3):
            for layout in ("striped", "separate"):
                ring = _ring(pkg, dt, L, n_slots, layout)
                for mode in ("1", "2", "0", None):
                    if mode is None:
                        monkeypatch.delenv("NDI_RING_GROUP", raising=False)
                    else:
                        monkeypatch.setenv("NDI_RING_GROUP", mode)
                    capfd.readouterr()
                    pkg.profile_read(reset=True)
                    got, seen = _gather(interp, qd, ring, ref.shape, dt)
                    what = (n_slots, layout, mode)
                    widths = _widths(capfd, L)
                    assert [s[0] for s in seen] == list(range(NCHUNKS)), what
                    assert [s[1] for s in seen] == [k * CHUNK for k in range(NCHUNKS)] and seen[-1][2] == 137, what
                    assert [s[3] for s in seen] == [k % n_slots for k in range(NCHUNKS)], what
                    assert np.array_equal(got, ref), what
                    if mode is None:      # whichever order is the default: every chunk once, groups where slots allow
                        assert sum(widths) == NCHUNKS and (max(widths) > 1) == (n_slots > 1), (what, widths)
                    else:
                        assert widths == WIDTHS[(mode, n_slots)], (what, widths)
                    assert pkg.profile_read(reset=True)["eval_launches"] == len(widths), what
    finally:
        pkg.profile_enable(False)


def test_consumer_on_its_own_stream_gets_one_chunk_per_launch(pkg, capfd, monkeypatch):
    """A consumer that returns an event from its second call on keeps the overlap of the next chunk's evaluation with its
    own work: from that return on every launch is one chunk wide (launch counts from profile_read), rows still equal."""
    import torch
    dt, L, n, path = SHAPES[0]
    interp, x, y, q, qd, ref = _case(pkg, dt, L, n, path)
    monkeypatch.setenv("NDI_TRACE_PLAN", "1")
    side = torch.cuda.Stream()
    pkg.profile_enable(True)
    try:
        for n_slots, mode, expect in ((2, "1", [2, 1, 1, 1]), (3, "1", [3, 1, 1]), (3, "2", [1, 3, 1]), (2, "0", [1] * 5)):
            monkeypatch.setenv("NDI_RING_GROUP", mode)
            ring = _ring(pkg, dt, L, n_slots, "striped")
            total = torch.full((Q, L), -1.0, dtype=torch.float64, device="cuda:0")
            capfd.readouterr()
            pkg.profile_read(reset=True)

            def consumer(c, rows):
                if c.index == 0:                                   # stream-ordered: nothing to return
                    total[c.q_begin:c.q_begin + c.q_count].copy_(rows, non_blocking=True)
                    return None
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    side.wait_event(ready)
                    for _ in range(8):                             # a drain slower than the producer
                        total[c.q_begin:c.q_begin + c.q_count].copy_(rows, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(side)
                return done
            interp.interp_array_ring(qd, CHUNK, consumer, slots=ring)
            torch.cuda.synchronize()
            widths = _widths(capfd, L)
            assert widths == expect, (n_slots, mode, widths)
            assert pkg.profile_read(reset=True)["eval_launches"] == len(expect), (n_slots, mode)
            assert np.array_equal(total.cpu().numpy(), ref), (n_slots, mode)
    finally:
        pkg.profile_enable(False)


@pytest.mark.parametrize("mode", ["1", "2", "0"])
def test_first_error_inside_a_group(pkg, monkeypatch, mode):
    """A failing query in the second chunk of a group, in the first chunk of a group and in a group's only chunk: exactly
    the rows [0, F) are produced (the slot's rows at and after F keep their fill), the error names F and its value."""
    import torch
    dt, L, n, path = SHAPES[2]
    interp, x, y, q, qd, ref = _case(pkg, dt, L, n, path)
    monkeypatch.setenv("NDI_RING_GROUP", mode)
    for F in (450, 100, 700, 300):
        bad = q.copy()
        bad[F] = x[-1] + 2.5
        bad[min(F + 40, Q - 1)] = x[0] - 1.0          # later failures do not matter
        bad[Q - 1] = np.nan
        ring = _ring(pkg, dt, L, 2, "separate")
        produced = []

        def consumer(c, rows):
            produced.append((c.index, c.q_begin, c.q_count, rows.cpu().numpy()))
        with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^x = .* is not in range") as ei:
            interp.interp_array_ring(torch.as_tensor(bad, device="cuda:0"), CHUNK, consumer, slots=ring)
        assert ei.value.index == F, (F, ei.value.index)
        full, part = divmod(F, CHUNK)
        want = [(k, k * CHUNK, CHUNK) for k in range(full)] + ([(full, full * CHUNK, part)] if part else [])
        assert [p[:3] for p in produced] == want, F
        assert np.array_equal(np.concatenate([p[3] for p in produced]), ref[:F]), F
        if part and full < 2:      # the cut chunk's slot, first use: rows before F written, the others never touched
            slot = ring[full % 2].cpu().numpy()
            assert np.array_equal(slot[:part], ref[full * CHUNK:F]) and np.all(slot[part:] == -7.0), F


def test_sharded_ring_groups_two_shards_on_one_device(pkg, capfd, monkeypatch):
    """The sharded ring goes through the same producer: two shards on one device, each streaming 5 chunks."""
    dt, L, n, path = SHAPES[0]
    interp, x, y, q, qd, ref = _case(pkg, dt, L, n, path)
    reps = [pkg.Interp1DBuilder.new(y).x(x).strategy(pkg.CubicSpline.new().device(0)).build() for _ in range(2)]
    rng = np.random.default_rng(9)
    q2 = np.concatenate([q, rng.uniform(x[0], x[-1], Q).astype(dt)])
    ref2 = np.empty((2 * Q, L), dtype=dt)
    interp.interp_array_into(q2, ref2)
    assert np.array_equal(ref2[:Q], ref)
    monkeypatch.setenv("NDI_TRACE_PLAN", "1")
    lock = threading.Lock()
    for mode in ("1", "0"):
        monkeypatch.setenv("NDI_RING_GROUP", mode)
        slots = [pkg.striped_ring(CHUNK, L, 2, dt, 0) for _ in range(2)]
        got = np.full_like(ref2, np.nan)
        capfd.readouterr()

        def consumer(c, rows):
            with lock:
                got[c.q_begin:c.q_begin + c.q_count] = rows.cpu().numpy()
        pkg.sharding.interp_array_ring_sharded(reps, q2, chunk_queries=CHUNK, consumer=consumer, slots=slots)
        assert np.array_equal(got, ref2), mode
        widths = _widths(capfd, L)
        assert sorted(widths) == (sorted([2, 2, 1] * 2) if mode == "1" else [1] * 10), (mode, widths)


def test_a_grouped_case_runs_clean_under_the_checked_library():
    """The bounds-checked build (every record position, query index and interval of the group kernel goes through
    NDI_CHK) runs the U = 8 shape through every slot count, layout and producer order: no violation, equal rows."""
    from test_gpu_checked_build import _ensure_debug_library
    _ensure_debug_library()
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_ring_groups.py"), "-m", "gpu",
                        "-x", "-q", "-k", "test_groups_equal_one_batch and float64-4096-300"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "failed" not in r.stdout.splitlines()[-1]
