"""Launch-for-launch A/B of two builds of the library: the same kernels, grids, workgroups and LDS, the same bytes.

A refactor of the host code that picks and launches the kernels must change nothing a profiler or a caller can see.
This tool runs a fixed matrix of shapes -- the values of the dispatch dimensions of the launch ladders, each at the
smallest shape that reaches it, and every build form of the 1-D cubic tables (`cases_build`: a, b and one evaluation per
build); `launch_trace_ab_cases.txt` shows what every case reached and the notes in the report name the legs that none
does -- once per library (`NDI_LIB` selects the file, a name beside the package's own
library), each process under `rocprofv3 --kernel-trace` with the program after `--`, and compares

  * the ordered list of (kernel name with template arguments, grid, workgroup, LDS bytes) of every process -- the
    library's kernels and torch's; the HIP runtime's own `__amd_rocclr_*` copy kernels are counted but not compared,
  * the `[ndi plan]` lines the library printed (NDI_TRACE_PLAN) and its launch counters (ndi_profile_read) per case,
  * the sha256 of every output the driver saved.

Variables that are read once per process (NDI_TILE_SLOPES, NDI_TILE_WG, NDI_TILE_TS, NDI_GROUP_*_SORT) get a process of their own.
One process at a time, each under its own timeout; nothing more is started after a failing one.  No counters are
collected.  With `--bench-rounds N` plain `bench.py` runs follow, the two libraries alternating, and the flagship
`ms_per_step`, the host-path leg and the bilinear leg's `step_minus_kernels_ms` are compared against the parent's own
run-to-run spread.  Everything is written to `<out>/launch_trace_ab.md` with the raw rows in `launch_trace_ab.jsonl`; a section
"## Notes (added by hand)" at the end of an existing report is kept.

    make -C ndarray-interp_amd/csrc LIB=../libndinterp_hip_parent.so      # in a checkout of the parent; copy the file here
    python tools/launch_trace_ab.py --out profiles [--parent-lib libndinterp_hip_parent.so] [--bench-rounds 5]
    python tools/launch_trace_ab.py --no-trace ...                           # rocprofv3 unusable: plan lines + counters + bytes
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {   # process -> the read-once variables it runs under
    "main": {},
    "tile_slopes0": {"NDI_TILE_SLOPES": "0"},
    "tile_wg512": {"NDI_TILE_WG": "512"},
    "group_nosort": {"NDI_GROUP_COARSE_SORT": "0", "NDI_GROUP_FINE_SORT": "0"},
    "tile_slopes256": {"NDI_TILE_SLOPES": "256"},      # the slope form with 256 records per hand-over
    "tile_ts5": {"NDI_TILE_TS": "5"},                  # a tile of 33 x 33 points: f64 slopes beside 1024 records (2 lanes)
    **{f"group_fine_sort{v}": {"NDI_GROUP_FINE_SORT": str(v)} for v in (2, 3, 4, 5)},
}
LIVE = ("NDI_SHORT_MODE", "NDI_FUSED_UNR", "NDI_FUSED_TB", "NDI_FUSED_LDS", "NDI_FUSED_PACK", "NDI_FUSED_SORTED",
        "NDI_SHORT_CQ", "NDI_LANES_KERNEL", "NDI_LANES2D_KERNEL", "NDI_SLOPES2D_KERNEL", "NDI_GROUP_TWO_LEVEL",
        "NDI_LANEWISE_MODE", "NDI_LANEWISE_RECORDS", "NDI_RING_GROUP", "NDI_SPLINE_BLOCKED", "NDI_SPLINE_WIDE",
        "NDI_SPLINE_KEEP_K")


# ---------------------------------------------------------------------------------------------------------------------
# the driver: one process, one library, one group of cases
# ---------------------------------------------------------------------------------------------------------------------
def driver(group, save_dir):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    dev = "cuda:0"
    rng = np.random.default_rng(1234)
    F32, F64 = np.float32, np.float64
    results = []
    pkg.profile_enable(True)      # the library's own launch counters, read per case

    def t(a):
        return torch.as_tensor(np.ascontiguousarray(a), device=dev)

    def axis(n, dt, clustered=False):
        """n uniform knots on [0, 1] -- or, clustered, n - 5 of them and 5 more within 5 * 2^-20 above the middle one: six
        knots that share a bucket of the dense index at every size it tries, so it stops at its 64 KiB cap with maxk = 6."""
        if not clustered:
            return np.linspace(0.0, 1.0, n).astype(dt)
        assert (n - 5) % 2 == 1, "the middle knot must be 0.5, a bucket boundary at every power of two"
        u = np.linspace(0.0, 1.0, n - 5)
        return np.sort(np.concatenate([u, 0.5 + np.arange(1, 6) * 2.0 ** -20])).astype(dt)

    def queries(lo, hi, nq, dt):
        return rng.uniform(float(lo), float(hi), nq).astype(dt).clip(lo, hi)

    def out_buffer(nq, lanes, dt, kind):
        td = torch.float32 if dt == F32 else torch.float64
        if kind == "aligned":
            return torch.zeros((nq, lanes), dtype=td, device=dev)
        if kind == "unaligned":        # contiguous rows, the base one element past a 16-byte boundary
            return torch.zeros(nq * lanes + 1, dtype=td, device=dev)[1:].view(nq, lanes)
        if kind == "strided":          # a row pitch wider than the row
            return torch.zeros((nq, lanes + 3), dtype=td, device=dev)[:, :lanes]
        raise ValueError(kind)

    def case(name, env, fn):
        """Runs fn() under the live variables `env`; its tensors are hashed (and the small ones saved)."""
        for k in LIVE:
            os.environ.pop(k, None)
        os.environ.update(env)
        sys.stderr.flush()
        print(f"[case] {name}", file=sys.stderr, flush=True)
        pkg.profile_read(True)
        outs = fn()           # (any exception ends the process: a case that did not run must not compare equal)
        torch.cuda.synchronize()
        prof = pkg.profile_read(True)
        outs = outs if isinstance(outs, (list, tuple)) else [outs]
        h = hashlib.sha256()
        nbytes = 0
        for i, o in enumerate(outs):
            a = o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o)
            a = np.ascontiguousarray(a)
            h.update(a.tobytes())
            nbytes += a.nbytes
            if a.nbytes <= (1 << 20):
                np.save(os.path.join(save_dir, f"{len(results):04d}_{i}.npy"), a)
        results.append({"case": name, "sha256": h.hexdigest(), "bytes": nbytes,
                        "counters": {k: prof[k] for k in ("eval_launches", "locate_launches", "group_launches", "last_path")}})

    # ---- 1-D ----------------------------------------------------------------------------------------------------------
    def strat1(kind):
        return pkg.CubicSpline.new() if kind == "cubic" else pkg.Linear.new()

    def h1(kind, n, lanes, dt):
        x = axis(n, dt)
        y = rng.uniform(0.0, 1.0, (n, lanes)).astype(dt)
        return pkg.Interp1DBuilder.new(t(y)).x(t(x)).strategy(strat1(kind)).build(), x

    def eval1(kind, n, lanes, nq, dt, path, out="aligned", fresh=False):
        def fn():
            it, x = h1(kind, n, lanes, dt)
            it.strategy.path = path
            q = t(queries(x[0], x[-1], nq, dt))
            o = out_buffer(nq, lanes, dt, out)
            it.strategy.interp_array_into(it, q, o, fresh=fresh)
            return o
        return fn

    AUTO, GATHER, BUCKETED = pkg.PATH_AUTO, pkg.PATH_GATHER, pkg.PATH_BUCKETED

    def cases_1d():
        for dt in (F32, F64):
            d = "f32" if dt == F32 else "f64"
            vn = 4 if dt == F32 else 2
            for kind in ("linear", "cubic"):
                k = f"1d {d} {kind}"
                case(f"{k} SMALL", {}, eval1(kind, 33, 1, 1000, dt, AUTO))
                on = {"NDI_LANES_KERNEL": "1"}
                case(f"{k} LANES L=1 vector", on, eval1(kind, 33, 1, 4000, dt, AUTO))
                case(f"{k} LANES L=1 scalar", on, eval1(kind, 33, 1, 4000, dt, AUTO, "unaligned"))
                case(f"{k} LANES L=1 fresh", on, eval1(kind, 33, 1, 4000, dt, AUTO, fresh=True))
                for lanes in (2, 4, 5, 8):
                    case(f"{k} LANES L={lanes}", on, eval1(kind, 33, lanes, 4000, dt, AUTO))
                # tables of more than 40 KiB (four workgroups no longer fit a CU): 1024 threads
                big = 1024 if (dt == F64 and kind == "cubic") else 2048
                case(f"{k} LANES tables > 40 KiB", on, eval1(kind, big, 1, 5000, dt, AUTO))
                case(f"{k} LANES tables > 40 KiB L=2", on, eval1(kind, big if kind == "linear" and dt == F32 else big // 2, 2, 5000, dt, AUTO))
                fu = {"NDI_SHORT_MODE": "2"}
                rows = 8 * vn            # 8 vectors per row
                case(f"{k} FUSED default", fu, eval1(kind, 33, rows, 4000, dt, AUTO))
                case(f"{k} FUSED fresh", fu, eval1(kind, 33, rows, 4000, dt, AUTO, fresh=True))
                for unr in ("1", "4"):
                    case(f"{k} FUSED unr={unr}", dict(fu, NDI_FUSED_UNR=unr), eval1(kind, 33, rows, 4000, dt, AUTO))
                for tb in ("256", "512", "1024"):
                    case(f"{k} FUSED tb={tb}", dict(fu, NDI_FUSED_TB=tb), eval1(kind, 33, rows, 4000, dt, AUTO))
                for lds in ("0", "1", "2"):
                    case(f"{k} FUSED lds={lds}", dict(fu, NDI_FUSED_LDS=lds), eval1(kind, 33, rows, 4000, dt, AUTO))
                case(f"{k} FUSED unaligned", fu, eval1(kind, 33, rows, 4000, dt, AUTO, "unaligned"))
                case(f"{k} FUSED unaligned lds=0", dict(fu, NDI_FUSED_LDS="0"), eval1(kind, 33, rows, 4000, dt, AUTO, "unaligned"))
                for pack in ("0", "1"):
                    case(f"{k} FUSED pack={pack}", dict(fu, NDI_FUSED_LDS="0", NDI_FUSED_PACK=pack),
                         eval1(kind, 33, 2 * vn, 4000, dt, AUTO))
                n_long = 40000 if dt == F32 else 20000      # the pyramid exceeds LDS_STAGE_LIMIT - 8 KiB
                case(f"{k} FUSED knots=global", fu, eval1(kind, n_long, 2 * vn, 4096, dt, AUTO))
                case(f"{k} FUSED knots=global scalar", fu, eval1(kind, n_long, 2 * vn, 4096, dt, AUTO, "unaligned"))
                so = {"NDI_SHORT_MODE": "2", "NDI_FUSED_SORTED": "1", "NDI_FUSED_LDS": "0"}
                case(f"{k} FUSED sorted", so, eval1(kind, 257, 64 // dt().itemsize, 8192, dt, AUTO))
                case(f"{k} FUSED sorted scalar", so, eval1(kind, 257, 64 // dt().itemsize, 8192, dt, AUTO, "unaligned"))
                for v in (4, 16, 32, 64, 128, 200):
                    case(f"{k} BUCKETED_SHORT v={v}", {}, eval1(kind, 17, v * vn, 3000, dt, BUCKETED))
                case(f"{k} BUCKETED_SHORT cq=16", {"NDI_SHORT_CQ": "16"}, eval1(kind, 17, 16 * vn, 3000, dt, BUCKETED))
                case(f"{k} BUCKETED_SHORT cq=64", {"NDI_SHORT_CQ": "64"}, eval1(kind, 17, 16 * vn, 3000, dt, BUCKETED))
                for v in (256, 300, 512, 600, 1024, 2048):
                    case(f"{k} BUCKETED v={v}", {}, eval1(kind, 9, v * vn, 300, dt, BUCKETED))
                case(f"{k} ROWS", {}, eval1(kind, 9, 256 * vn, 300, dt, GATHER))
                for lanes in (3, 8):
                    case(f"{k} FLAT L={lanes}", {"NDI_SHORT_MODE": "1"}, eval1(kind, 33, lanes, 3000, dt, GATHER))
                for n_slots in (2, 4):
                    def ring(n_slots=n_slots, kind=kind, dt=dt, vn=vn):
                        chunk, lanes, nchunks = 256, 256 * vn, 7
                        it, x = h1(kind, 9, lanes, dt)
                        it.strategy.path = BUCKETED
                        q = t(queries(x[0], x[-1], chunk * nchunks - 50, dt))
                        slots = pkg.striped_ring(chunk, lanes, n_slots, dt, 0)
                        got = torch.zeros((chunk * nchunks, lanes), dtype=slots[0].dtype, device=dev)

                        def consumer(c, rows):
                            got[c.q_begin:c.q_begin + c.q_count].copy_(rows)
                        it.interp_array_ring(q, chunk, consumer, slots=slots)
                        return got
                    case(f"{k} RING slots={n_slots}", {}, ring)

    # ---- the searches' own ladders, and the kernels only long rows or long batches reach ------------------------------
    def cases_search():
        flat = {"NDI_SHORT_MODE": "1"}
        for dt in (F32, F64):
            d = "f32" if dt == F32 else "f64"
            vn = 4 if dt == F32 else 2
            n_long = 40000 if dt == F32 else 20000        # the pyramid does not fit LDS: locate_kernel<T, false, .>
            case(f"search {d} knots outside LDS", flat, eval1("linear", n_long, 3, 3000, dt, GATHER))
            for kind in ("linear", "cubic"):          # rows of 256 vectors: antideriv_eval_rows_kernel
                def rows(kind=kind, dt=dt, vn=vn, pair=False):
                    it, x = h1(kind, 9, 256 * vn, dt)
                    q = t(queries(x[0], x[-1], 300, dt))
                    if pair:
                        return it.integrate(q, t(queries(x[0], x[-1], 300, dt)))
                    return it.antiderivative().interp_array(q)
                case(f"antiderivative {d} {kind} long rows eval", {}, rows)
                case(f"antiderivative {d} {kind} long rows integrate", {}, lambda f=rows: f(pair=True))
        # 16 and more batches of 64 queries per wave: the searches that request four batches together (QB = LOCATE_QB)
        case("search f32 deep, knots in LDS (grouped short rows)", {}, eval1("linear", 17, 16, 4_500_000, F32, BUCKETED))
        case("search f32 deep, knots outside LDS", flat, eval1("linear", 40000, 1, 34_000_000, F32, GATHER))
        case("search f32 deep, two axes (tiles)", OFF2, eval2(65, 70, 4, 4_500_000, F32, BUCKETED))

    # ---- 1-D families -------------------------------------------------------------------------------------------------
    def cases_families():
        for dt in (F32, F64):
            d = "f32" if dt == F32 else "f64"
            for kind in ("linear", "cubic"):
                for staged in (True, False):
                    for rec in ("0", "1"):
                        def lw(kind=kind, staged=staged, dt=dt):
                            n = 65 if staged else (40000 if dt == F32 else 20000)
                            it, x = h1(kind, n, 4, dt)
                            q = t(rng.uniform(float(x[0]), float(x[-1]), (3000, 4)).astype(dt).clip(x[0], x[-1]))
                            o = out_buffer(3000, 4, dt, "aligned")
                            it.interp_lanewise_into(q, o)
                            return o
                        case(f"lanewise {d} {kind} staged={int(staged)} records={rec}",
                             {"NDI_LANEWISE_MODE": "2", "NDI_LANEWISE_RECORDS": rec}, lw)
                for lanes in (4, 3):          # vector rows, scalar rows
                    def anti(kind=kind, lanes=lanes, dt=dt, pair=False):
                        it, x = h1(kind, 33, lanes, dt)
                        Fh = it.antiderivative()
                        q = t(queries(x[0], x[-1], 3000, dt))
                        if pair:
                            return it.integrate(q, t(queries(x[0], x[-1], 3000, dt)))
                        return Fh.interp_array(q)
                    case(f"antiderivative {d} {kind} L={lanes} eval", {}, anti)
                    case(f"antiderivative {d} {kind} L={lanes} integrate", {}, lambda a=anti: a(pair=True))
                def inv(kind=kind, dt=dt):
                    x = axis(33, dt)
                    y = (np.cumsum(rng.uniform(0.5, 1.5, (33, 3)), axis=0)).astype(dt)
                    strat = pkg.Pchip.new() if kind == "cubic" else pkg.Linear.new()
                    it = pkg.Interp1DBuilder.new(t(y)).x(t(x)).strategy(strat).build()
                    lo, hi = float(y[0].max()), float(y[-1].min())
                    return it.inverse().interp_array(t(queries(lo, hi, 2000, dt)))
                case(f"inverse {d} {kind}", {}, inv)

    # ---- the builds of the 1-D cubic tables (csrc/spline_build_host.hpp) -----------------------------------------------
    def cases_build():
        """Every build form at the smallest shape that reaches it.  Hashed: a, b, and one evaluation of 256 queries with the
        tables in LDS wherever they fit -- {y, k} where the build kept k, so the k table is compared too."""
        KEPT = {"NDI_SHORT_MODE": "2", "NDI_FUSED_LDS": "2"}
        BC = pkg.BoundaryCondition

        def built(n, lanes, dt, make_strategy, periodic=False, host=False):
            def fn():
                x = axis(n, dt)
                y = rng.uniform(0.0, 1.0, (n, lanes)).astype(dt)
                if periodic:
                    y[-1] = y[0]
                strat = make_strategy(x, y)
                it = pkg.Interp1DBuilder.new(y if host else t(y)).x(x if host else t(x)).strategy(strat).build()
                a, b = it.strategy.coefficients()
                o = out_buffer(256, lanes, dt, "aligned")
                it.strategy.interp_array_into(it, t(queries(x[0], x[-1], 256, dt)), o)
                return [a, b, o]
            return fn

        def spline(bc=None, reference_order=False):
            def make(x, y):
                s = pkg.CubicSpline.new().reference_order(reference_order)
                return s if bc is None else s.boundary(bc)
            return make

        def individual(x, y):
            SB, lanes = pkg.SingleBoundary, y.shape[1]
            ends = [SB.NotAKnot, SB.Natural, SB.Clamped, SB.FirstDeriv(0.5), SB.SecondDeriv(-0.25)]
            rows = [pkg.RowBoundary.Mixed(ends[l % 5], ends[(l // 2 + 1) % 5]) for l in range(lanes)]
            rows[-1] = pkg.RowBoundary.NotAKnot          # (with n == 3: the parabola rows)
            r = np.empty((1, lanes), dtype=object)
            r[0, :] = rows
            return pkg.CubicSpline.new().boundary(BC.Individual(r))

        for dt in (F32, F64):
            d = "f32" if dt == F32 else "f64"
            vn = 4 if dt == F32 else 2
            k = f"build {d}"
            case(f"{k} one workgroup in LDS (100, 5)", KEPT, built(100, 5, dt, spline()))
            case(f"{k} one workgroup in LDS, k dropped", dict(KEPT, NDI_SPLINE_KEEP_K="0"), built(100, 5, dt, spline()))
            case(f"{k} one workgroup in LDS, natural ends", KEPT, built(100, 5, dt, spline(BC.Natural)))
            case(f"{k} one launch, over 96 KiB", KEPT, built(2000, 8, dt, spline()))
            case(f"{k} one launch, over 256 lanes", KEPT, built(100, 300, dt, spline()))
            case(f"{k} serial, three kernels", KEPT, built(600, 300, dt, spline()))
            case(f"{k} serial, wide", KEPT, built(33, 5000, dt, spline()))
            case(f"{k} serial, wide 1400 lanes", KEPT, built(97, 1400, dt, spline()))
            case(f"{k} serial, wide forced", dict(KEPT, NDI_SPLINE_WIDE="1"), built(600, 300, dt, spline()))
            case(f"{k} serial, wide off", dict(KEPT, NDI_SPLINE_WIDE="0"), built(33, 5000, dt, spline()))
            case(f"{k} n = 3 parabola", KEPT, built(3, 5, dt, spline()))
            case(f"{k} n = 3 periodic", KEPT, built(3, 5, dt, spline(BC.Periodic), periodic=True))
            case(f"{k} serial periodic", KEPT, built(100, 5, dt, spline(BC.Periodic), periodic=True))
            case(f"{k} blocked sweeps", KEPT, built(2048, 8, dt, spline()))
            case(f"{k} blocked sweeps, periodic", KEPT, built(2048, 8, dt, spline(BC.Periodic), periodic=True))
            case(f"{k} blocked sweeps, device-side elimination", KEPT, built(32768, 2, dt, spline()))
            case(f"{k} NDI_SPLINE_BLOCKED=0", dict(KEPT, NDI_SPLINE_BLOCKED="0"), built(2048, 8, dt, spline()))
            case(f"{k} NDI_SPLINE_BLOCKED=1", dict(KEPT, NDI_SPLINE_BLOCKED="1"), built(100, 5, dt, spline()))
            case(f"{k} NDI_SPLINE_BLOCKED=1 periodic", dict(KEPT, NDI_SPLINE_BLOCKED="1"),
                 built(100, 5, dt, spline(BC.Periodic), periodic=True))
            case(f"{k} NDI_BUILD_REFERENCE_ORDER", KEPT, built(2048, 8, dt, spline(reference_order=True)))
            case(f"{k} Individual n = 3", KEPT, built(3, 6, dt, individual))
            case(f"{k} Individual", KEPT, built(10, 6, dt, individual))
            case(f"{k} Individual, k dropped", dict(KEPT, NDI_SPLINE_KEEP_K="0"), built(10, 6, dt, individual))
            for lanes, rows in ((2 * vn, "vector"), (3, "scalar")):
                case(f"{k} Pchip {rows}", KEPT, built(33, lanes, dt, lambda x, y: pkg.Pchip.new()))
                case(f"{k} Akima {rows}", KEPT, built(33, lanes, dt, lambda x, y: pkg.Akima.new()))
                case(f"{k} CubicHermite {rows}, device derivatives", KEPT,
                     built(33, lanes, dt, lambda x, y: pkg.CubicHermite.new(t(2.0 * y))))
                case(f"{k} CubicHermite {rows}, host derivatives", KEPT,
                     built(33, lanes, dt, lambda x, y: pkg.CubicHermite.new(2.0 * y), host=True))
            # (host derivatives without a kept k table: the upload goes to a temporary)
            case(f"{k} CubicHermite host derivatives, k dropped", dict(KEPT, NDI_SPLINE_KEEP_K="0"),
                 built(33, 3, dt, lambda x, y: pkg.CubicHermite.new(2.0 * y), host=True))

    # ---- 2-D Bilinear -------------------------------------------------------------------------------------------------
    def h2(nx, ny, lanes, dt, clustered=False, strategy=None):
        gx, gy = axis(nx, dt, clustered), axis(ny, dt)      # (one clustered axis: its index alone takes 64 KiB of LDS)
        g = rng.uniform(0.0, 1.0, (nx, ny, lanes)).astype(dt)
        b = pkg.Interp2DBuilder.new(t(g)).x(t(gx)).y(t(gy))
        if strategy is not None:
            b = b.strategy(strategy)
        return b.build(), gx, gy

    def eval2(nx, ny, lanes, nq, dt, path, out="aligned", clustered=False, fresh=False):
        def fn():
            it, gx, gy = h2(nx, ny, lanes, dt, clustered)
            it.strategy.path = path
            qx, qy = t(queries(gx[0], gx[-1], nq, dt)), t(queries(gy[0], gy[-1], nq, dt))
            o = out_buffer(nq, lanes, dt, out)
            it.strategy.interp_array_into(it, qx, qy, o, fresh=fresh)
            return o
        return fn

    OFF2 = {"NDI_LANES2D_KERNEL": "0", "NDI_SLOPES2D_KERNEL": "0"}

    def cases_2d():
        for dt in (F32, F64):
            d = "f32" if dt == F32 else "f64"
            vn = 4 if dt == F32 else 2
            k = f"2d {d}"
            on = {"NDI_LANES2D_KERNEL": "1"}
            case(f"{k} LANES2 L=1 vector", on, eval2(33, 17, 1, 4000, dt, AUTO))
            case(f"{k} LANES2 L=1 strided", on, eval2(33, 17, 1, 4000, dt, AUTO, "strided"))
            case(f"{k} LANES2 L=3", on, eval2(33, 17, 3, 4000, dt, AUTO))
            case(f"{k} LANES2 L=3 fresh", on, eval2(33, 17, 3, 4000, dt, AUTO, fresh=True))
            case(f"{k} LANES2 tb=1024", on, eval2(120, 120, 1, 4000, dt, AUTO))
            case(f"{k} LANES2 tb=1024 L=2", on, eval2(80, 80, 2, 4000, dt, AUTO))
            on = {"NDI_SLOPES2D_KERNEL": "1", "NDI_LANES2D_KERNEL": "0"}
            for lanes in range(1, 13 if dt == F32 else 9):
                case(f"{k} SLOPES2 L={lanes}", on, eval2(40, 30, lanes, 3000, dt, AUTO))
            case(f"{k} SLOPES2 clustered", on, eval2(40, 30, 3, 3000, dt, AUTO, clustered=True))
            case(f"{k} SLOPES2 unaligned", on, eval2(40, 30, 4, 3000, dt, AUTO, "unaligned"))
            case(f"{k} SLOPES2 strided", on, eval2(40, 30, 4, 3000, dt, AUTO, "strided"))
            case(f"{k} SLOPES2 clustered strided", on, eval2(40, 30, 5, 3000, dt, AUTO, "strided", clustered=True))
            case(f"{k} SMALL L=1", {}, eval2(33, 17, 1, 1000, dt, AUTO))
            case(f"{k} SMALL L=2", {}, eval2(33, 17, 2, 1000, dt, AUTO))
            case(f"{k} SMALL L=2 lut", {}, eval2(33, 17, 2, 5000, dt, AUTO))
            case(f"{k} FUSED2 vector", OFF2, eval2(100, 100, 2 * vn, 65536, dt, AUTO))
            case(f"{k} FUSED2 scalar", OFF2, eval2(100, 100, 5, 65536, dt, AUTO))
            case(f"{k} FUSED2 fresh", OFF2, eval2(100, 100, 5, 65536, dt, AUTO, fresh=True))
            case(f"{k} FUSED2 long axes", OFF2, eval2(3000, 40, 2 * vn, 65536, dt, AUTO))
            case(f"{k} TILED split", OFF2, eval2(65, 70, 8 * vn, 5000, dt, BUCKETED))
            case(f"{k} TILED no split", OFF2, eval2(65, 70, vn, 5000, dt, BUCKETED))
            case(f"{k} TILED wide rows", OFF2, eval2(65, 70, 64 * vn, 5000, dt, BUCKETED))
            case(f"{k} TILED two-level", dict(OFF2, NDI_GROUP_TWO_LEVEL="1"), eval2(300, 280, 8 * vn, 20000, dt, BUCKETED))
            case(f"{k} GATHER vector", OFF2, eval2(33, 17, 2 * vn, 3000, dt, GATHER))
            case(f"{k} GATHER scalar", OFF2, eval2(33, 17, 5, 3000, dt, GATHER))
            case(f"{k} GATHER 2^20 knots in LDS, pair-packed", OFF2, eval2(200, 200, vn, 1 << 20, dt, BUCKETED))
            case(f"{k} GATHER 2^20 knots in LDS", OFF2, eval2(30, 30, 3 * vn, 1 << 20, dt, BUCKETED))
            n_long = 40000 if dt == F32 else 20000      # the two pyramids do not fit LDS together: one search launch per axis
            case(f"{k} GATHER axes outside LDS", OFF2, eval2(n_long, 4, vn, 3000, dt, GATHER))

    def cases_tiles_only():
        for dt in (F32, F64):
            d = "f32" if dt == F32 else "f64"
            vn = 4 if dt == F32 else 2
            case(f"2d {d} TILED split", OFF2, eval2(65, 70, 8 * vn, 5000, dt, BUCKETED))
            case(f"2d {d} TILED no split", OFF2, eval2(65, 70, vn, 5000, dt, BUCKETED))
            case(f"2d {d} TILED two-level", dict(OFF2, NDI_GROUP_TWO_LEVEL="1"), eval2(300, 280, 8 * vn, 20000, dt, BUCKETED))

    # ---- Bicubic ------------------------------------------------------------------------------------------------------
    def cases_bicubic():
        for dt in (F32, F64):
            d = "f32" if dt == F32 else "f64"
            vn = 4 if dt == F32 else 2
            shapes = {"vector": (20, 15, vn), "scalar": (20, 15, 3), "knots outside LDS": (40000 if dt == F32 else 20000, 4, vn)}
            for label, (nx, ny, lanes) in shapes.items():
                def mk(nx=nx, ny=ny, lanes=lanes, dt=dt):
                    it, gx, gy = h2(nx, ny, lanes, dt, strategy=pkg.Bicubic.new())
                    nq = 3000
                    return it, [t(queries(a[0], a[-1], nq, dt)) for a in (gx, gx, gy, gy)]
                orders = [(a, b) for a in range(3) for b in range(3)] if label == "vector" else [(0, 0), (1, 2)]
                for nu in orders:
                    def part(mk=mk, nu=nu):
                        it, (xa, xb, ya, yb) = mk()
                        h = it if nu == (0, 0) else it.partial(*nu)
                        return h.interp_array(xa, ya)
                    case(f"bicubic {d} {label} nu={nu[0]},{nu[1]}", {}, part)

                def into(mk=mk, lanes=lanes, dt=dt):
                    it, (xa, xb, ya, yb) = mk()
                    o = out_buffer(3000, lanes, dt, "aligned")
                    it.strategy.interp_array_into(it, xa, ya, o)
                    return o
                case(f"bicubic {d} {label} into (pre-pass)", {}, into)

                def integral(mk=mk, rect=False):
                    it, (xa, xb, ya, yb) = mk()
                    A = it.antiderivative()
                    return A.integral(xa, xb, ya, yb) if rect else A.interp_array(xa, ya)
                case(f"bicubic {d} {label} integral points", {}, integral)
                case(f"bicubic {d} {label} integral rectangles", {}, lambda f=integral: f(rect=True))
                for order in (1, 2):
                    def jet(mk=mk, order=order):
                        it, (xa, xb, ya, yb) = mk()
                        return list(it.jet(xa, ya, order=order))
                    case(f"bicubic {d} {label} jet order={order}", {}, jet)

    if group == "main":
        cases_1d()
        cases_families()
        cases_build()
        cases_2d()
        cases_bicubic()
        cases_search()
    else:
        cases_tiles_only()
    json.dump({"cases": results}, open(os.path.join(save_dir, "outputs.json"), "w"), indent=0)
    print(f"driver {group}: {len(results)} cases", flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def read_trace(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            def dims(prefix):
                return tuple(int(r[k]) for k in sorted(r) if k.startswith(prefix))
            lds = [int(r[k]) for k in r if k.startswith("LDS")]
            rows.append((int(r.get("Dispatch_Id") or r.get("Start_Timestamp") or len(rows)), r["Kernel_Name"],
                         dims("Grid_Size"), dims("Workgroup_Size"), lds[0] if lds else -1))
    rows.sort(key=lambda x: x[0])
    return [x[1:] for x in rows]


def own_launches(trace):
    """Without the HIP runtime's own copy / fill kernels (`__amd_rocclr_*`): whether a hipMemcpy runs as one of them or on a
    DMA engine is the runtime's choice at that moment, not the program's, and differs between two runs of one library."""
    return [x for x in trace if not x[0].startswith("__amd_rocclr_")]


def plan_lines(stderr_text):
    """[(case, [plan lines])] from the driver's stderr."""
    out, cur = [], None
    for ln in stderr_text.splitlines():
        if ln.startswith("[case] "):
            cur = (ln[7:], [])
            out.append(cur)
        elif ln.startswith("[ndi plan]") and cur is not None:
            cur[1].append(ln)
    return out


def run_matrix(args, libs, log):
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    got = {}
    for lib_name, lib_env in libs.items():
        for group, genv in GROUPS.items():
            save = tempfile.mkdtemp(prefix=f"ndi_trace_{lib_name}_{group}_")
            tdir = os.path.join(save, "trace")
            cmd = [sys.executable, os.path.abspath(__file__), "--driver", group, "--save", save]
            if not args.no_trace:
                cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tdir, "--"] + cmd
            env = dict(os.environ, NDI_TUNE_LIVE="1", NDI_TRACE_PLAN="1", **genv, **lib_env)
            t0 = time.time()
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=args.process_timeout)
            if r.returncode != 0:      # nothing more is started on the device after a failing run
                open(os.path.join(args.out, "launch_trace_ab_failed_stderr.txt"), "w").write(r.stderr[-20000:])
                sys.exit(f"{lib_name}/{group}: exit status {r.returncode}\n{r.stderr[-3000:]}")
            res = json.load(open(os.path.join(save, "outputs.json")))
            got[(lib_name, group)] = {"trace": [] if args.no_trace else read_trace(tdir), "plans": plan_lines(r.stderr),
                                      "cases": res["cases"]}
            log({"kind": "matrix", "lib": lib_name, "group": group, "cases": len(res["cases"]),
                 "launches": len(got[(lib_name, group)]["trace"]),
                 "eval_launches": sum(c["counters"]["eval_launches"] for c in res["cases"]),
                 "locate_launches": sum(c["counters"]["locate_launches"] for c in res["cases"]), "wall_s": round(time.time() - t0, 1)})
            if args.keep:
                print("kept", save)
            else:
                shutil.rmtree(save, ignore_errors=True)
    return got


def compare(got, no_trace):
    """-> (lines for the report, ok)"""
    lines, ok = [], True
    ncases, kernels, launches = 0, set(), 0
    for group in GROUPS:
        a, b = got[("parent", group)], got[("new", group)]
        rt = [len(g["trace"]) - len(own_launches(g["trace"])) for g in (a, b)]
        a, b = dict(a, trace=own_launches(a["trace"])), dict(b, trace=own_launches(b["trace"]))
        ncases += len(a["cases"])
        kernels.update(x[0] for x in a["trace"])
        launches += len(a["trace"])
        first = None
        if not no_trace:
            if len(a["trace"]) != len(b["trace"]):
                first = f"{len(a['trace'])} launches under the parent, {len(b['trace'])} under the change"
            for i, (x, y) in enumerate(zip(a["trace"], b["trace"])):
                if x != y:
                    first = f"launch {i}: parent {x} / change {y}"
                    break
        if first is None and a["plans"] != b["plans"]:
            for x, y in zip(a["plans"], b["plans"]):
                if x != y:
                    first = f"plan lines of case {x[0]!r}: parent {x[1]} / change {y[1]}"
                    break
            first = first or "a different number of cases printed plan lines"
        if first is None:
            for x, y in zip(a["cases"], b["cases"]):
                if x != y:
                    first = (f"case {x['case']!r}: parent {x['sha256'][:16]} ({x['bytes']} B) {x['counters']} / "
                             f"change {y['case']!r} {y['sha256'][:16]} ({y['bytes']} B) {y['counters']}")
                    break
            if first is None and len(a["cases"]) != len(b["cases"]):
                first = "a different number of cases ran"
        ok = ok and first is None
        lines.append(f"* process `{group}` ({len(a['cases'])} cases, {len(a['trace'])} kernel launches, "
                     f"{sum(len(p[1]) for p in a['plans'])} plan lines; left out: {rt[0]} / {rt[1]} launches of the HIP runtime's "
                     f"own `__amd_rocclr_*` copy kernels under the parent / the change): "
                     + ("**identical**" if first is None else f"**first difference** {first}"))
    head = [f"* cases: {ncases} in {len(GROUPS)} processes per library; kernel launches traced: {launches}; "
            f"distinct kernels (name with template arguments) seen: {len(kernels)}"]
    if no_trace:
        head.append("* `rocprofv3 --kernel-trace` was not used in this run: the comparison below rests on the `[ndi plan]` lines, "
                    "the library's launch counters and the output bytes only -- **the stronger check (kernel, grid, workgroup, "
                    "LDS per launch) is missing**")
    return head + lines, ok


# the legs behind the timed region that carry the host path and the bilinear leg, nothing else
LEGS = ["--full", "--no-pmc", "--no-cpu-baseline", "--no-check", "--no-gather-leg", "--placement-probe", "0"]


def run_bench(args, libs, log):
    """Plain runs (the flagship ms_per_step), then runs with the secondary legs; the libraries alternate in both."""
    rows = []
    t_start = time.time()
    for flags, rounds in (([], args.bench_rounds), (LEGS, args.legs_rounds)):
        for i in range(rounds):
            if time.time() - t_start > args.budget_s:      # no further round is started
                break
            for lib_name, lib_env in libs.items():
                t0 = time.time()
                r = subprocess.run([sys.executable, "bench.py"] + flags, cwd=ROOT, env=dict(os.environ, **lib_env),
                                   capture_output=True, text=True, timeout=args.process_timeout)
                if r.returncode != 0:
                    sys.exit(f"{lib_name}: bench.py exited with {r.returncode}\n{r.stderr[-3000:]}")
                line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                sec = line.get("secondary", {})
                row = {"kind": "bench", "flags": " ".join(flags) or "(plain)", "round": i, "lib": lib_name,
                       "ms_per_step": None if flags else line.get("ms_per_step"),
                       "ms_per_step_with_legs": line.get("ms_per_step") if flags else None,
                       "host_path_ms_per_call": sec.get("host_path", {}).get("ms_per_call"),
                       "bilinear_c5_step_minus_kernels_ms": sec.get("c5_share", {}).get("step_minus_kernels_ms"),
                       "bilinear_c3_step_minus_kernels_ms": sec.get("c3", {}).get("step_minus_kernels_ms"),
                       "wall_s": round(time.time() - t0, 1)}
                rows.append(row)
                log(row)
    return rows


def bench_report(rows):
    lines, ok = [], True
    lines.append("| figure | parent: median (min .. max) | change: median (min .. max) | change - parent | parent's spread | within |")
    lines.append("|---|---|---|---|---|---|")
    for key in ("ms_per_step", "host_path_ms_per_call", "bilinear_c5_step_minus_kernels_ms", "bilinear_c3_step_minus_kernels_ms"):
        v = {lib: sorted(r[key] for r in rows if r["lib"] == lib and r.get(key) is not None) for lib in ("parent", "new")}
        if not v["parent"] or not v["new"]:
            lines.append(f"| `{key}` | not measured in this run | | | | |")
            continue
        med = {lib: x[len(x) // 2] if len(x) % 2 else 0.5 * (x[len(x) // 2 - 1] + x[len(x) // 2]) for lib, x in v.items()}
        spread = v["parent"][-1] - v["parent"][0]
        within = med["new"] - med["parent"] <= spread
        ok = ok and within
        lines.append(f"| `{key}` | {med['parent']:.4f} ({v['parent'][0]:.4f} .. {v['parent'][-1]:.4f}) | "
                     f"{med['new']:.4f} ({v['new'][0]:.4f} .. {v['new'][-1]:.4f}) | {med['new'] - med['parent']:+.4f} | "
                     f"{spread:.4f} | {'yes' if within else '**no**'} |")
    return lines, ok


NOTES = "## Notes (added by hand)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", help=argparse.SUPPRESS)
    ap.add_argument("--save", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--parent-lib", default="libndinterp_hip_parent.so",
                    help="the parent commit's library, a file name beside the package's own library (NDI_LIB)")
    ap.add_argument("--no-trace", action="store_true", help="without rocprofv3: plan lines, launch counters and bytes only")
    ap.add_argument("--no-matrix", action="store_true")
    ap.add_argument("--bench-rounds", type=int, default=0, help="alternating rounds of plain bench.py (the flagship ms_per_step)")
    ap.add_argument("--legs-rounds", type=int, default=0,
                    help="alternating rounds of bench.py with its secondary legs (the host-path leg, the bilinear legs)")
    ap.add_argument("--budget-s", type=float, default=900.0, help="no further bench round is started after this")
    ap.add_argument("--process-timeout", type=float, default=400.0)
    ap.add_argument("--keep", action="store_true", help="keep every process's directory (outputs, trace)")
    args = ap.parse_args()
    if args.driver:
        driver(args.driver, args.save)
        return
    os.makedirs(args.out, exist_ok=True)
    libs = {"parent": {"NDI_LIB": args.parent_lib}, "new": {}}
    fresh = not args.no_matrix          # a run with the matrix starts both files over; --no-matrix adds to them
    raw = open(os.path.join(args.out, "launch_trace_ab.jsonl"), "w" if fresh else "a")

    def log(rec):
        raw.write(json.dumps(rec) + "\n")
        raw.flush()
        print(json.dumps(rec), flush=True)

    md = ["# Launch-for-launch A/B: the parent's library against this tree's", "",
          "Written by `tools/launch_trace_ab.py`; raw rows in `launch_trace_ab.jsonl`.", ""]
    ok = True
    if not args.no_matrix:
        got = run_matrix(args, libs, log)
        lines, ok = compare(got, args.no_trace)
        with open(os.path.join(args.out, "launch_trace_ab_cases.txt"), "w") as f:   # what the matrix reached (this tree's library)
            for group in GROUPS:
                g = got[("new", group)]
                plans = dict(g["plans"])
                f.write(f"== process {group}\n")
                for c in g["cases"]:
                    f.write(f"{c['case']}: {c['counters']} {c['bytes']} B {c['sha256'][:16]}\n")
                    for ln in plans.get(c["case"], []):
                        f.write(f"    {ln}\n")
            f.write("== distinct kernels\n")
            for k in sorted({x[0] for g in got.values() for x in g["trace"]}):
                f.write(k + "\n")
        md += ["## Kernel launches, plan lines, outputs", ""] + lines + ["", f"Outcome: **{'identical' if ok else 'DIFFERENT'}**", ""]
    if args.bench_rounds or args.legs_rounds:
        rows = run_bench(args, libs, log)
        lines, bok = bench_report(rows)
        md += [f"## Speed: `bench.py`, the two libraries alternating -- {sum(1 for r in rows if r['flags'] == '(plain)') // 2} plain rounds "
               f"(`ms_per_step`), {sum(1 for r in rows if r['flags'] != '(plain)') // 2} rounds with `{' '.join(LEGS)}` (the legs)", "",
               "The yardstick is the parent's own run-to-run spread (max - min) in this session: the change passes a figure "
               "when its median is no more than that spread above the parent's median (ms; lower is better).", ""] + lines + [""]
        ok = ok and bok
    md_path = os.path.join(args.out, "launch_trace_ab.md")
    old = open(md_path).read() if os.path.exists(md_path) else ""
    tail = old[old.index(NOTES):] if NOTES in old else ""       # the hand-written part survives a rerun
    body = "\n".join(md) + "\n"
    open(md_path, "w").write((body if fresh else old[:len(old) - len(tail)] + body) + tail)
    print("\n".join(md))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
