"""f16 / bf16 Linear and Bilinear on the device, compared bit for bit with a numpy restatement of the `half` crate's
arithmetic (every operation: operands to f32 exactly, one f32 operation, round to T with ties to even).  NaN results
compare as "both NaN"; everything else compares as bits, so -0.0 and +0.0 differ."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_half_abi import bf16_round, bf16_value

pytestmark = pytest.mark.gpu
DTS = ["f16", "bf16"]


def tbits(v, dt):
    """f32 values -> T bit patterns (uint16)."""
    v = np.asarray(v, dtype=np.float32)
    return v.astype(np.float16).view(np.uint16) if dt == "f16" else bf16_round(v)


def tval(bits, dt):
    """T bit patterns -> f32 values (exact)."""
    bits = np.asarray(bits, dtype=np.uint16)
    return bits.view(np.float16).astype(np.float32) if dt == "f16" else bf16_value(bits)


def r(v, dt):
    """One T operation's rounding of an f32 result."""
    return tval(tbits(v, dt), dt)


def to_t(v, dt, device=None):
    """f32 values -> T: numpy float16 for f16 (a torch tensor if `device`), torch.bfloat16 for bf16."""
    import torch
    bits = tbits(v, dt)
    if dt == "f16" and device is None:
        return bits.view(np.float16)
    t = torch.from_numpy(bits.view(np.int16).copy()).view(torch.float16 if dt == "f16" else torch.bfloat16)
    return t.to(device) if device is not None else t


def out_bits(res):
    import torch
    if isinstance(res, torch.Tensor):
        return res.detach().cpu().view(torch.int16).numpy().view(np.uint16)
    return np.asarray(res).view(np.uint16)


def frac(y1, y2, dx, d, dt):
    """Linear::calc_frac in T with dx = r(x2 - x1), d = r(x - x1) given."""
    dy = r(y2 - y1, dt)
    m = r(dy / dx, dt)
    p = r(m * d, dt)
    return r(p + y1, dt)


def lin_ref(xk, data, q, dt):
    """Expected bits of Linear on T (inputs as f32 images of T values)."""
    with np.errstate(all="ignore"):
        n = len(xk)
        d2 = data.reshape(n, -1)
        i = np.clip(np.searchsorted(xk, q, side="right") - 1, 0, n - 2)
        dx = r(xk[i + 1] - xk[i], dt)[:, None]
        d = r(q - xk[i], dt)[:, None]
        return tbits(frac(d2[i], d2[i + 1], dx, d, dt), dt)


def bil_ref(xk, yk, g, qx, qy, dt):
    with np.errstate(all="ignore"):
        g3 = g.reshape(len(xk), len(yk), -1)
        xi = np.clip(np.searchsorted(xk, qx, side="right") - 1, 0, len(xk) - 2)
        yi = np.clip(np.searchsorted(yk, qy, side="right") - 1, 0, len(yk) - 2)
        dx = r(xk[xi + 1] - xk[xi], dt)[:, None]; ddx = r(qx - xk[xi], dt)[:, None]
        dy = r(yk[yi + 1] - yk[yi], dt)[:, None]; ddy = r(qy - yk[yi], dt)[:, None]
        z1 = frac(g3[xi, yi], g3[xi + 1, yi], dx, ddx, dt)
        z2 = frac(g3[xi, yi + 1], g3[xi + 1, yi + 1], dx, ddx, dt)
        return tbits(frac(z1, z2, dy, ddy, dt), dt)


def same(got_bits, want_bits, what=""):
    got_bits = np.asarray(got_bits).reshape(-1); want_bits = np.asarray(want_bits).reshape(-1)
    assert got_bits.shape == want_bits.shape, what
    bad = got_bits != want_bits
    if bad.any():
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {int(np.argmax(bad))}: "
                             f"got {got_bits[bad][0]:#06x} want {want_bits[bad][0]:#06x}")


def same_t(got_bits, want_bits, dt, what=""):
    got_bits = np.asarray(got_bits, np.uint16).reshape(-1); want_bits = np.asarray(want_bits, np.uint16).reshape(-1)
    gn, wn = np.isnan(tval(got_bits, dt)), np.isnan(tval(want_bits, dt))
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    same(got_bits[~gn], want_bits[~wn], what)


def build1d(pkg, x, data, dt, extrapolate=False, device=True):
    """x, data: f32 values (already values of T); data on the device for bf16 or when `device`."""
    s = pkg.Linear.new().extrapolate(extrapolate)
    dev = "cuda:0" if (device or dt == "bf16") else None
    b = pkg.Interp1DBuilder.new(to_t(data, dt, dev)).x(to_t(x, dt))
    interp = b.strategy(s).build()
    assert interp.strategy._h is not None
    return interp


def build2d(pkg, x, y, g, dt, extrapolate=False):
    s = pkg.Bilinear.new().extrapolate(extrapolate)
    interp = pkg.Interp2DBuilder.new(to_t(g, dt, "cuda:0")).x(to_t(x, dt)).y(to_t(y, dt)).strategy(s).build()
    assert interp.strategy._h is not None
    return interp


def _axis(rng, n, dt, even):
    if even:
        x = np.arange(n, dtype=np.float32) * 0.25 - 8.0
    else:
        x = np.sort(rng.uniform(-30.0, 30.0, n)).astype(np.float32)
    x = np.unique(r(x, dt))
    return x if len(x) >= 2 else r(np.array([-1.0, 2.0], np.float32), dt)


def _floats(v):
    if isinstance(v, list):
        return [_floats(e) for e in v]
    return float(v) if isinstance(v, str) else v


@pytest.mark.parametrize("dt", DTS)
def test_reference_vectors_cast_to_t(pkg, refvec, dt):
    import torch
    done = 0
    for case in refvec["linear"]:
        x = r(np.array(_floats(case["x"]), np.float64), dt)
        if not np.all(np.diff(x) > 0):
            continue   # the axis is not strictly rising in T
        data = r(np.array(_floats(case["data"]), np.float64), dt)
        q = r(np.array(_floats(case["q"]), np.float64), dt)
        if not case.get("extrapolate") and not np.all((x[0] <= q) & (q <= x[-1])):
            continue
        interp = build1d(pkg, x, data, dt, extrapolate=case.get("extrapolate", False))
        got = interp.interp_array(to_t(q, dt, "cuda:0"))
        want = lin_ref(x, data, q, dt)
        same_t(out_bits(got), want, dt, case["name"])
        if dt == "f16":   # today's public path on the same input
            host = pkg.Interp1DBuilder.new(data.astype(np.float16)).x(x.astype(np.float16)).strategy(
                pkg.Linear.new().extrapolate(case.get("extrapolate", False))).build()
            assert host.strategy.__class__.__name__ == "HostLinear"
            same_t(out_bits(host.interp_array(q.astype(np.float16))), want, dt, case["name"] + " generic_host")
            dev = interp.interp_array(q.astype(np.float16))   # host queries, host output
            same_t(out_bits(dev), want, dt, case["name"] + " host buffers")
        done += 1
    for case in refvec["bilinear"]:
        x = r(np.array(_floats(case["x"]), np.float64), dt); y = r(np.array(_floats(case["y"]), np.float64), dt)
        if not (np.all(np.diff(x) > 0) and np.all(np.diff(y) > 0)):
            continue
        g = r(np.array(_floats(case["data"]), np.float64), dt)
        qx = r(np.array(_floats(case["qx"]), np.float64), dt); qy = r(np.array(_floats(case["qy"]), np.float64), dt)
        if not case.get("extrapolate") and not np.all((x[0] <= qx) & (qx <= x[-1]) & (y[0] <= qy) & (qy <= y[-1])):
            continue
        interp = build2d(pkg, x, y, g, dt, extrapolate=case.get("extrapolate", False))
        got = interp.interp_array(to_t(qx, dt, "cuda:0"), to_t(qy, dt, "cuda:0"))
        assert got.dtype == (torch.float16 if dt == "f16" else torch.bfloat16)
        want = bil_ref(x, y, g, qx.reshape(-1), qy.reshape(-1), dt)
        same_t(out_bits(got), want, dt, case["name"])
        if dt == "f16":
            host = pkg.Interp2DBuilder.new(g.astype(np.float16)).x(x.astype(np.float16)).y(y.astype(np.float16)) \
                .strategy(pkg.Bilinear.new().extrapolate(case.get("extrapolate", False))).build()
            assert host.strategy.__class__.__name__ == "HostBilinear"
            same_t(out_bits(host.interp_array(qx.astype(np.float16), qy.astype(np.float16))), want, dt,
                   case["name"] + " generic_host")
        done += 1
    assert done >= 4


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [2, 17, 300, 5000])
def test_linear_random_shapes(pkg, dt, n):
    import torch
    rng = np.random.default_rng(n * 3 + (dt == "bf16"))
    for lanes in (1, 2, 5, 8, 16, 64, 128, 1000, 4096):
        if n * lanes > 4_000_000:
            continue
        for even in (True, False):
            x = _axis(rng, n, dt, even)
            data = r(rng.uniform(-100, 100, (len(x), lanes)).astype(np.float32), dt)
            nq = 3000 if lanes <= 128 else 300
            q = r(rng.uniform(x[0], x[-1], nq).astype(np.float32), dt)
            q[:3] = [x[0], x[-1], x[len(x) // 2]]
            interp = build1d(pkg, x, data.reshape((len(x),) + ((lanes,) if lanes > 1 else ())), dt)
            want = lin_ref(x, data, q, dt)
            got = interp.interp_array(to_t(q, dt, "cuda:0"))
            same_t(out_bits(got), want, dt, f"n={n} lanes={lanes} even={even}")
            # a caller-owned row whose byte offset is not 16-byte aligned
            # a caller-owned output one element past a 16-byte boundary: the element-wise fallback of the vector path
            flat = torch.full((nq * lanes + 1,), 7.0, dtype=got.dtype, device="cuda:0")
            view = flat[1:].view(nq, lanes)
            assert view.data_ptr() % 16 == 2
            interp.strategy.interp_array_into(interp, to_t(q, dt, "cuda:0"), view)
            same_t(out_bits(view), want, dt, f"unaligned n={n} lanes={lanes}")
            assert float(flat[0]) == 7.0


@pytest.mark.parametrize("dt", DTS)
def test_bilinear_random_grids(pkg, dt):
    import torch
    rng = np.random.default_rng(11 + (dt == "bf16"))
    for nx, ny, lanes, nq in ((2, 3, 1, 5000), (17, 40, 3, 5000), (100, 100, 5, 100_000), (300, 257, 64, 20000),
                              (2000, 2500, 8, 20000), (2048, 2048, 64, 20000), (5, 7, 200, 2000),
                              (30, 41, 37, 5000)):
        x = _axis(rng, nx, dt, nx % 2 == 0); y = _axis(rng, ny, dt, False)
        g = r(rng.uniform(-50, 50, (len(x), len(y), lanes)).astype(np.float32), dt)
        qx = r(rng.uniform(x[0], x[-1], nq).astype(np.float32), dt)
        qy = r(rng.uniform(y[0], y[-1], nq).astype(np.float32), dt)
        qx[:2] = [x[-1], x[0]]; qy[:2] = [y[-1], y[0]]
        interp = build2d(pkg, x, y, g, dt)
        got = interp.interp_array(to_t(qx, dt, "cuda:0"), to_t(qy, dt, "cuda:0"))
        want = bil_ref(x, y, g, qx, qy, dt)
        same_t(out_bits(got), want, dt, f"{nx}x{ny}x{lanes}")
        if lanes > 32:   # the group mapping into an output one element past a 16-byte boundary
            flat = torch.full((nq * lanes + 1,), 7.0, dtype=got.dtype, device="cuda:0")
            view = flat[1:].view(nq, lanes)
            interp.strategy.interp_array_into(interp, to_t(qx, dt, "cuda:0"), to_t(qy, dt, "cuda:0"), view)
            same_t(out_bits(view), want, dt, f"unaligned {nx}x{ny}x{lanes}")
            assert float(flat[0]) == 7.0
            del flat, view
        del interp, got
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dt", DTS)
def test_edge_values(pkg, dt):
    big = 60000.0 if dt == "f16" else 3.0e38
    tiny = 2.0 ** -24 if dt == "f16" else 2.0 ** -133
    x = r(np.array([-2.0, -1.0, 0.0, 0.5, 3.0]), dt)
    data = r(np.array([[big, -0.0, tiny, 1.0], [-big, 0.0, 3 * tiny, -1.0], [big, -0.0, -tiny, 0.0],
                       [-big, 0.0, tiny, 2.0], [big, 1.0, 0.0, 0.0]], np.float32), dt)
    q = r(np.array([3.0, -2.0, -5.0, 7.0, 0.25, -0.0, 0.0, -1.5, 2.0, 1e-3, -1e-3]), dt)
    interp = build1d(pkg, x, data, dt, extrapolate=True)
    want = lin_ref(x, data, q, dt)
    got = out_bits(interp.interp_array(to_t(q, dt, "cuda:0")))
    same_t(got, want, dt, "edges")
    assert np.isinf(tval(want, dt)).any() and (want == 0x8000).any()   # the restatement does reach inf and -0.0


@pytest.mark.parametrize("dt", DTS)
def test_first_error_keeps_caller_rows(pkg, dt):
    import torch
    rng = np.random.default_rng(5)
    for lanes in (1, 8, 300):
        x = r(np.arange(50, dtype=np.float32), dt)
        data = r(rng.uniform(-1, 1, (50, lanes)).astype(np.float32), dt)
        interp = build1d(pkg, x, data, dt)
        q = r(rng.uniform(0, 49, 4000).astype(np.float32), dt)
        q[2500] = 60.0; q[3000] = -3.0
        want = lin_ref(x, data, q, dt)
        out = torch.full((4000, lanes), 9.0, dtype=torch.float16 if dt == "f16" else torch.bfloat16, device="cuda:0")
        with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^x = 60\.0 is not in range$") as e:
            interp.strategy.interp_array_into(interp, to_t(q, dt, "cuda:0"), out)
        assert e.value.index == 2500
        same_t(out_bits(out[:2500]), want[:2500], dt, "rows before the failure")
        assert bool((out[2500:] == 9.0).all())
        if dt == "f16":   # host buffers, and the generic path's message
            hout = np.full((4000, lanes), 9.0, np.float16)
            with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^x = 60\.0 is not in range$"):
                interp.strategy.interp_array_into(interp, q.astype(np.float16), hout)
            same_t(hout[:2500].view(np.uint16), want[:2500], dt, "host rows")
            assert np.all(hout[2500:] == 9.0)
        # NaN while extrapolating: the reference's panic
        ie = build1d(pkg, x, data, dt, extrapolate=True)
        q2 = q.copy(); q2[100] = np.nan
        with pytest.raises(pkg.Panic, match="NaN") as e:
            ie.interp_array(to_t(q2, dt, "cuda:0"))
        assert e.value.index == 100
    # 2-D: x before y
    g = r(rng.uniform(-1, 1, (10, 12, 3)).astype(np.float32), dt)
    b = build2d(pkg, r(np.arange(10.0), dt), r(np.arange(12.0), dt), g, dt)
    qx = r(np.array([1.0, 2.0, 3.0, 20.0]), dt); qy = r(np.array([1.0, 30.0, 2.0, 40.0]), dt)
    with pytest.raises(pkg.InterpolateError.OutOfBounds, match=r"^y = 30\.0 is not in range$") as e:
        b.interp_array(to_t(qx, dt, "cuda:0"), to_t(qy, dt, "cuda:0"))
    assert e.value.index == 1 and e.value.axis == 1


@pytest.mark.parametrize("dt", DTS)
def test_ring_and_sharded_first_error(pkg, dt):
    import torch
    rng = np.random.default_rng(7)
    x = r(np.arange(64, dtype=np.float32), dt)
    data = r(rng.uniform(-1, 1, (64, 16)).astype(np.float32), dt)
    interp = build1d(pkg, x, data, dt)
    q = r(rng.uniform(0, 63, 10000).astype(np.float32), dt)
    want = lin_ref(x, data, q, dt).reshape(10000, 16)
    q_bad = q.copy(); q_bad[5555] = 100.0
    for qq, fail in ((q, None), (q_bad, 5555)):
        seen = np.full((10000, 16), 0xFFFF, np.uint16)

        def consumer(c, rows):
            seen[c.q_begin:c.q_begin + c.q_count] = out_bits(rows)
        slots = [torch.empty((1000, 16), dtype=torch.float16 if dt == "f16" else torch.bfloat16, device="cuda:0")
                 for _ in range(2)]
        if fail is None:
            interp.interp_array_ring(to_t(qq, dt, "cuda:0"), 1000, consumer, slots=slots)
            same_t(seen, want, dt, "ring")
        else:
            with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
                interp.interp_array_ring(to_t(qq, dt, "cuda:0"), 1000, consumer, slots=slots)
            assert e.value.index == fail
            same_t(seen[:fail], want[:fail], dt, "ring rows before the failure")
            assert np.all(seen[fail:] == 0xFFFF)
    for n_rep in (2, 3, 4):
        reps = [build1d(pkg, x, data, dt) for _ in range(n_rep)]
        if dt == "f16":
            out = np.full((10000, 16), 5.0, np.float16)
            with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
                pkg.sharding.interp_array_sharded(reps, q_bad.astype(np.float16), out=out)
            assert e.value.index == 5555
            same_t(out[:5555].view(np.uint16), want[:5555], dt, "sharded rows")
            assert np.all(out[5555:] == 5.0)
        outs = pkg.sharding.interp_array_sharded(reps, q.astype(np.float32) if dt == "bf16" else q.astype(np.float16))
        same_t(np.concatenate([out_bits(o) for o in outs]), want, dt, f"sharded x{n_rep}")


@pytest.mark.parametrize("dt", DTS)
def test_async_locator_paths_and_handles(pkg, dt):
    import torch
    rng = np.random.default_rng(3)
    x = r(np.sort(rng.uniform(-10, 10, 200)).astype(np.float32), dt); x = np.unique(x)
    data = r(rng.uniform(-1, 1, (len(x), 64)).astype(np.float32), dt)
    interp = build1d(pkg, x, data, dt)
    q = r(rng.uniform(x[0], x[-1], 50000).astype(np.float32), dt)
    want = lin_ref(x, data, q, dt)
    out = torch.empty((50000, 64), dtype=torch.float16 if dt == "f16" else torch.bfloat16, device="cuda:0")
    interp.strategy.interp_array_into(interp, to_t(q, dt, "cuda:0"), out, async_launch=True)
    interp.strategy.finish()
    same_t(out_bits(out), want, dt, "async")
    q_bad = q.copy(); q_bad[40000] = 50.0
    interp.strategy.interp_array_into(interp, to_t(q_bad, dt, "cuda:0"), out, async_launch=True)
    with pytest.raises(pkg.InterpolateError.OutOfBounds) as e:
        interp.strategy.finish()
    assert e.value.index == 40000
    # BUCKETED is refused, GATHER evaluates
    interp.strategy.path = pkg.PATH_BUCKETED
    with pytest.raises(pkg.DeviceError, match="UNSUPPORTED"):
        interp.interp_array(to_t(q, dt, "cuda:0"))
    interp.strategy.path = pkg.PATH_GATHER
    same_t(out_bits(interp.interp_array(to_t(q, dt, "cuda:0"))), want, dt, "gather")
    # the locator and get_lower_index on T
    kt = to_t(x, dt, "cuda:0"); qt = to_t(q, dt, "cuda:0")
    ref_idx = np.clip(np.searchsorted(x, q, side="right") - 1, 0, len(x) - 2)
    assert np.array_equal(pkg.get_lower_index(kt, qt).cpu().numpy(), ref_idx)
    assert np.array_equal(pkg.Locator(kt).get_lower_index(qt).cpu().numpy(), ref_idx)
    if dt == "f16":
        assert np.array_equal(pkg.get_lower_index(x.astype(np.float16), q.astype(np.float16)), ref_idx)
    # the strategy on the device: .device(0) with host data (f16), a GPU tensor, and bf16 on either device
    lin = pkg.Linear.new().device(0).build(to_t(x, dt), to_t(data, dt))
    assert lin._h is not None
    lin2 = pkg.Linear.new().build(to_t(x, dt, "cuda:0"), to_t(data, dt, "cuda:0"))
    assert lin2._h is not None
    if dt == "bf16":   # host bf16 tensors run on the device, results are bf16 tensors
        it = pkg.Interp1DBuilder.new(to_t(data, dt)).x(to_t(x, dt)).build()
        res = it.interp_array(to_t(q[:100], dt))
        assert isinstance(res, torch.Tensor) and res.dtype == torch.bfloat16
        same_t(out_bits(res), want[:100], dt, "bf16 host tensors")
        one = it.interp(float(tval(tbits([q[5]], dt), dt)[0]))
        same_t(out_bits(one), want[5], dt, "interp()")


def test_checked_build_has_no_bounds_violation(tmp_path):
    lib = os.path.join(ROOT, "ndarray-interp_amd", "libndinterp_hip_dbg.so")
    assert os.path.exists(lib)
    script = tmp_path / "child.py"
    script.write_text(f"""
import sys
sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})
import numpy as np, torch
from conftest import load_product_package
from test_gpu_half import build1d, build2d, lin_ref, bil_ref, out_bits, same_t, r, to_t
pkg = load_product_package()
rng = np.random.default_rng(1)
for dt in ("f16", "bf16"):
    for n, lanes in ((5000, 3), (300, 64), (17, 1)):
        x = r(np.arange(n, dtype=np.float32) * 0.5, dt); x = np.unique(x)
        data = r(rng.uniform(-1, 1, (len(x), lanes)).astype(np.float32), dt)
        q = r(rng.uniform(x[0], x[-1], 2000).astype(np.float32), dt)
        it = build1d(pkg, x, data, dt)
        same_t(out_bits(it.interp_array(to_t(q, dt, "cuda:0"))), lin_ref(x, data, q, dt), dt, "dbg 1d")
    x = r(np.arange(3000, dtype=np.float32), dt); x = np.unique(x); y = r(np.arange(40, dtype=np.float32), dt)
    g = r(rng.uniform(-1, 1, (len(x), len(y), 8)).astype(np.float32), dt)
    qx = r(rng.uniform(x[0], x[-1], 3000).astype(np.float32), dt); qy = r(rng.uniform(0, 39, 3000).astype(np.float32), dt)
    b = build2d(pkg, x, y, g, dt)
    same_t(out_bits(b.interp_array(to_t(qx, dt, "cuda:0"), to_t(qy, dt, "cuda:0"))), bil_ref(x, y, g, qx, qy, dt), dt, "dbg 2d")
print("ok")
""")
    env = dict(os.environ, NDI_LIB="libndinterp_hip_dbg.so")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout + p.stderr


@pytest.mark.parametrize("dt", DTS)
def test_division_over_many_operand_pairs(pkg, dt):
    """calc_frac's m = r(r(y2 - y1) / r(x2 - x1)) over ~10^6 distinct (dy, dx) pairs: every interval of a random axis
    has its own dx, and the data covers T's whole range (subnormals, huge values, signed zeros) so that dy does too."""
    rng = np.random.default_rng(17 + (dt == "bf16"))
    bits = rng.integers(0, 1 << 16, 40000, dtype=np.uint32).astype(np.uint16)
    vals = tval(bits, dt)
    vals = vals[np.isfinite(vals)]
    x = np.unique(vals)[:: max(1, len(np.unique(vals)) // 2000)]
    lanes = 512
    data = tval(rng.integers(0, 1 << 16, (len(x), lanes), dtype=np.uint32).astype(np.uint16), dt)
    data[~np.isfinite(data)] = 0.0
    interp = build1d(pkg, x, data, dt, extrapolate=True)
    with np.errstate(all="ignore"):
        q = r(x[:-1] + (x[1:] - x[:-1]) * rng.uniform(0, 1, len(x) - 1).astype(np.float32), dt)
    q = np.where(np.isfinite(q), q, x[:-1])   # inside its interval, never NaN
    got = interp.interp_array(to_t(q, dt, "cuda:0"))
    same_t(out_bits(got), lin_ref(x, data, q, dt), dt, "division sweep")
