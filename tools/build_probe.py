"""CubicSpline::build (cubic_spline.rs:754-771) through the library -- ndi_interp1d_create: validation, uploads, the
x-only plan on the host, the Thomas kernels -- next to the single-thread CPU port (oracle.cubic_build), for the shapes
VERDICT r3 names: many knots with scalar / narrow data, the reference's (100, 5), and C2.

    python tools/build_probe.py > profiles/r05_build_probe.jsonl
    NDI_LIB=libndinterp_hip_parent.so python tools/build_probe.py 100x5 1024x8 4096x8     # an A/B of two libraries: alternate
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
import oracle

pkg = g.load_package()
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)


def med(f, reps=5):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        del r
    return float(np.median(ts))


SHAPES = ((100, 5), (4096, 8), (100_000, 1), (1_000_000, 1), (1_000_000, 8), (4096, 256), (4096, 4096))
if len(sys.argv) > 1:      # only these: `100x5 1024x8 4096x8`, the small builds whose milliseconds are host-side
    SHAPES = tuple(tuple(int(v) for v in a.split("x")) for a in sys.argv[1:])

for n, L in SHAPES:
    x = np.sort(rng.uniform(0, 1, n)) if n < 1_000_000 else np.cumsum(rng.uniform(0.5, 1.5, n))
    x = np.unique(x)
    n = x.size
    y = rng.uniform(0, 1, (n, L))
    yp = y.copy(); yp[-1] = yp[0]
    xd, yd = torch.as_tensor(x, device=dev), torch.as_tensor(y, device=dev)
    ypd = torch.as_tensor(yp, device=dev)
    rec = {"n": n, "lanes": L}
    for name, bc, data, ddata in (("not_a_knot", pkg.BoundaryCondition.NotAKnot, y, yd),
                                  ("natural", pkg.BoundaryCondition.Natural, y, yd),
                                  ("periodic", pkg.BoundaryCondition.Periodic, yp, ypd)):
        def build_host():
            it = pkg.Interp1DBuilder.new(data).x(x).strategy(pkg.CubicSpline.new().boundary(bc)).build()
            it.strategy.release()

        def build_dev():
            it = pkg.Interp1DBuilder.new(ddata).x(xd).strategy(pkg.CubicSpline.new().boundary(bc)).build()
            it.strategy.release()
        build_host()
        rec[name + "_create_host_arrays_ms"] = round(med(build_host) * 1e3, 3)
        rec[name + "_create_device_arrays_ms"] = round(med(build_dev) * 1e3, 3)
        # the time INSIDE ndi_interp1d_create alone (device-resident arrays; the mirror's validation and object
        # plumbing around it is what the two numbers above add): median of 9 bare C calls
        import ctypes as C
        cap = pkg._capi
        d = cap.Interp1DDesc()
        d.dtype, d.strategy, d.extrapolate, d.device = cap.F64, cap.CUBIC_SPLINE, 0, 0
        d.n, d.lanes, d.x_len = n, L, n
        d.x, d.data, d.memspace, d.validate = xd.data_ptr(), ddata.data_ptr(), cap.MEM_DEVICE, 0
        d.periodic = int(name == "periodic")
        kind = {"not_a_knot": cap.BC_NOT_A_KNOT, "natural": cap.BC_NATURAL, "periodic": cap.BC_NOT_A_KNOT}[name]
        d.left = cap.Boundary(kind, 0.0); d.right = cap.Boundary(kind, 0.0)
        ts = []
        for _ in range(9):
            h = C.c_void_p()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = cap.lib().ndi_interp1d_create(C.byref(d), C.byref(h))
            ts.append(time.perf_counter() - t0)
            assert st == 0, cap.last_error()
            cap.lib().ndi_interp1d_destroy(h)
        rec[name + "_c_call_ms"] = round(float(np.median(ts)) * 1e3, 3)
        if name == "not_a_knot":
            cpu = med(lambda: oracle.cubic_build(x, y), reps=3)
            rec["cpu_port_1_thread_ms"] = round(cpu * 1e3, 3)
            # parity of what was built (tolerances: bit-exact on the per-lane serial kernels, 1e-10 relative to the
            # table's largest magnitude on the blocked narrow-lane variant)
            it = pkg.Interp1DBuilder.new(ddata).x(xd).strategy(pkg.CubicSpline.new().boundary(bc)).build()
            ca, cb = it.strategy.coefficients()
            st, a, b = oracle.cubic_build(x, y)
            ca = np.asarray(ca).reshape(a.shape); cb = np.asarray(cb).reshape(b.shape)
            rec["bit_exact"] = bool(np.array_equal(ca, a) and np.array_equal(cb, b))
            scale = max(np.max(np.abs(a)), np.max(np.abs(b)))
            rec["max_abs_err_over_max_abs"] = float(max(np.max(np.abs(ca - a)), np.max(np.abs(cb - b))) / scale)
            it.strategy.release()
    rec["create_vs_cpu"] = round(rec["not_a_knot_create_device_arrays_ms"] / rec["cpu_port_1_thread_ms"], 2)
    print(json.dumps(rec), flush=True)
