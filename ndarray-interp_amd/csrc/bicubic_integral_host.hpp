// csrc/bicubic_integral_host.hpp -- host side of the 2-D antiderivative handles of Bicubic (ndi_interp2d_antiderivative,
// ndi_interp2d_integral, ndi_interp2d_integral_tables); included by ndinterp_api.hip after bicubic_host.hpp and
// antiderivative_host.hpp.
//
// An integral handle IS an Interp2DImpl (bicubic == true, integral == true): it shares the source's node table and owns
// the record table {PP, Qz, Qzy, Pz, Pzx} (`itable`) and its two knot pyramids.  Everything that takes two query arrays --
// eval, async_launch / finish, the ring, the sharded calls, trim, clone -- is the Bilinear / Bicubic code; only the plan
// (Plan2::BICUBIC_INT: the range pre-pass unless the output is fresh, then eval_bicubic_integral_kernel) is its own.
// The rectangle call carries four query arrays, which the float host engine (two arrays, two status words) does not:
// it has a host body of its own here (bicubic_integral_rect): staging, the host-output chunk loop, the first-error report.
// It has no async_launch form.
//
// Build (NULL stream, complete on return, temporaries freed before that): the node table is unpacked into four plain
// grids; every prefix is hermite_ab_kernel (the a / b rows of the Hermite data) followed by the 1-D build
// (antideriv_prefix_build) on an (nx, ny L) view for the x passes and on transposed copies viewed as (ny, nx L) for
// the y passes; one pack writes the records.
#pragma once

template <class T>
static void integral_hermite_prefix(int device, const T* knots, uint64_t n, uint64_t L, const T* p, const T* k, T* a, T* b,
                                    T* P) {
  const unsigned g = bicubic_copy_grid((n - 1) * L);
  hipLaunchKernelGGL(hermite_ab_kernel<T>, dim3(g), dim3(BLOCK), 0, (hipStream_t) nullptr, p, k, knots, a, b, n, L);
  NDI_HIP(hipGetLastError());
  antideriv_prefix_build<T, false>(device, n, L, p, (const T*)a, (const T*)b, knots, P);
}

template <class T>
static void bicubic_integral_build(const Interp2DImpl<T>& src, Interp2DImpl<T>& h) {
  Range rg("ndi:bicubic_integral_build");
  const uint64_t nx = src.nx, ny = src.ny, L = src.lanes, total = nx * ny * L;
  const size_t bytes = (size_t)total * sizeof(T);
  const int dev = src.device;
  const unsigned g = bicubic_copy_grid(total);
  hipStream_t s0 = nullptr;
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] bicubic integral build nx=%llu ny=%llu lanes=%llu xview=%llu yview=%llu passes=5\n",
                 (unsigned long long)nx, (unsigned long long)ny, (unsigned long long)L, (unsigned long long)(ny * L),
                 (unsigned long long)(nx * L));
  DevBuf z, zx, zy, zxy, a, b, trA, trB, qz, qzy, pzT, pzxT, pz, pzx, pp;
  for (DevBuf* d : {&z, &zx, &zy, &zxy, &a, &b, &trA, &trB, &qz, &qzy, &pzT, &pzxT, &pz, &pzx, &pp}) d->reserve(bytes);
  hipLaunchKernelGGL(integral_unpack_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, (const T*)src.table->template as<T>(), z.as<T>(),
                     zx.as<T>(), zy.as<T>(), zxy.as<T>(), nx * ny, L);
  NDI_HIP(hipGetLastError());
  const T* kx = h.px.view.lv0;
  const T* ky = h.py.view.lv0;
  // along x on (nx, ny L) views
  integral_hermite_prefix<T>(dev, kx, nx, ny * L, z.as<T>(), zx.as<T>(), a.as<T>(), b.as<T>(), qz.as<T>());
  integral_hermite_prefix<T>(dev, kx, nx, ny * L, zy.as<T>(), zxy.as<T>(), a.as<T>(), b.as<T>(), qzy.as<T>());
  // along y on transposed copies viewed as (ny, nx L)
  auto transpose = [&](const DevBuf& in, DevBuf& out, uint64_t n0, uint64_t n1) {
    hipLaunchKernelGGL(transpose_nodes_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, (const T*)in.as<T>(), out.as<T>(), n0, n1, L);
    NDI_HIP(hipGetLastError());
  };
  transpose(z, trA, nx, ny);
  transpose(zy, trB, nx, ny);
  integral_hermite_prefix<T>(dev, ky, ny, nx * L, trA.as<T>(), trB.as<T>(), a.as<T>(), b.as<T>(), pzT.as<T>());
  transpose(zx, trA, nx, ny);
  transpose(zxy, trB, nx, ny);
  integral_hermite_prefix<T>(dev, ky, ny, nx * L, trA.as<T>(), trB.as<T>(), a.as<T>(), b.as<T>(), pzxT.as<T>());
  // PP: along x of (Pz, Pzx), in grid order
  transpose(pzT, pz, ny, nx);
  transpose(pzxT, pzx, ny, nx);
  integral_hermite_prefix<T>(dev, kx, nx, ny * L, pz.as<T>(), pzx.as<T>(), a.as<T>(), b.as<T>(), pp.as<T>());
  h.itable.reserve(5 * bytes);
  hipLaunchKernelGGL(integral_pack_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, (const T*)pp.as<T>(), (const T*)qz.as<T>(),
                     (const T*)qzy.as<T>(), (const T*)pzT.as<T>(), (const T*)pzxT.as<T>(), h.itable.template as<T>(), nx, ny, L);
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipStreamSynchronize(s0));         // the records are complete on return: any stream may read them
}

// Plan2::BICUBIC_INT and the rectangle call: the launch (the range pre-pass, when there is one, was enqueued before).
// qx_lo == nullptr: F(qx, qy); else the rectangle [qx_lo, qx] x [qy_lo, qy].
template <class T>
static void bicubic_integral_launch_eval(const Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const T* qx, const T* qy,
                                         const T* qx_lo, const T* qy_lo, uint64_t nq, T* out, uint64_t out_stride,
                                         bool check) {
  constexpr int VN = Wide<T>::N;
  constexpr unsigned TB = 256;
  const bool rect = qx_lo != nullptr;
  const bool vec = (h.lanes % VN == 0) && (out_stride % VN == 0) && aligned16(out);
  BicubicIntegralArgs<T> A{};
  A.px = h.px.view; A.py = h.py.view;
  A.table = h.table->template as<T>();
  A.itable = h.itable.template as<T>();
  A.qx = qx; A.qy = qy; A.qx_lo = qx_lo; A.qy_lo = qy_lo;
  A.out = out;
  A.nq = nq;
  A.out_stride = out_stride;
  A.lv = vec ? h.lanes / VN : h.lanes;
  A.lv_magic = (A.lv >= 2 && A.lv < 64) ? (uint32_t)(((1ull << 32) + A.lv - 1) / A.lv) : 0u;
  uint64_t vchunk = 512;                     // as Bicubic: pieces of 512 vectors, more when that would pass the grid limit
  while ((A.lv + vchunk - 1) / vchunk > 32768) vchunk *= 2;
  A.vchunk = (uint32_t)vchunk;
  const unsigned gy = (unsigned)((A.lv + vchunk - 1) / vchunk);
  A.mode = h.mode;
  A.first_fail = &st->first_fail[0];
  A.check = check ? 1 : 0;
  const size_t nb = rect ? 2 : 1;
  const size_t strips = (size_t)(TB / 64) * 64 * nb * (2 * sizeof(uint32_t) + 4 * sizeof(T));
  const size_t knots = (h.px.lds_bytes + h.py.lds_bytes + 15) & ~(size_t)15;
  const bool klds = knots + strips <= LDS_STAGE_LIMIT;
  const size_t lds = (klds ? knots : 0) + strips;
  const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + TB - 1) / TB,
                                                                        std::max<uint64_t>(1, (uint64_t)cu_count() * wgs_per_cu(lds, TB) * 4 / gy)));
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] bicubic integral rect=%d vec=%d lv=%llu klds=%d grid=%u x %u lds=%zu prepass=%d\n",
                 (int)rect, (int)vec, (unsigned long long)A.lv, (int)klds, gx, gy, lds, check ? 0 : 1);
  pick_bool(rect, [&](auto rect_) {
    constexpr bool RC = rect_;
    bicubic_pick_form<T>(vec, klds, [&](auto vec_, auto kl_) {
      launch_lds<T>(eval_bicubic_integral_kernel<T, vec_, kl_, TB, RC>, LDS_STAGE_LIMIT, s, PC_EVAL, dim3(gx, gy), dim3(TB), lds, A);
    });
  });
}

// ndi_interp2d_integral_tables: the five prefix tables as plain [nx][ny][lanes] arrays (any of them may be NULL)
template <class T>
static ndi_status bicubic_integral_tables(const Interp2DImpl<T>& h, void* const dst[5], int memspace) {
  DeviceGuard dg(h.device);
  const uint64_t nodes = h.nx * h.ny, total = nodes * h.lanes;
  const size_t bytes = (size_t)total * sizeof(T);
  DevBuf tmp[5];
  T* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < 5; ++k) {
    if (!dst[k]) continue;
    if (memspace == NDI_MEM_DEVICE) {
      dev[k] = static_cast<T*>(dst[k]);
    } else {
      tmp[k].reserve(bytes);
      dev[k] = tmp[k].template as<T>();
    }
  }
  hipLaunchKernelGGL(integral_unpack_tables_kernel<T>, dim3(bicubic_copy_grid(total)), dim3(BLOCK), 0, (hipStream_t) nullptr,
                     (const T*)h.itable.template as<T>(), dev[0], dev[1], dev[2], dev[3], dev[4], nodes, h.lanes);
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipStreamSynchronize(nullptr));
  if (memspace != NDI_MEM_DEVICE)
    for (int k = 0; k < 5; ++k)
      if (dst[k]) NDI_HIP(hipMemcpy(dst[k], dev[k], bytes, hipMemcpyDeviceToHost));
  return NDI_OK;
}

// ndi_interp2d_integral: out = (F(xb, yb) - F(xa, yb)) - (F(xb, ya) - F(xa, ya)), one evaluation launch per batch.
// Status word 0 is the lowest failing index over the two x bounds, word 1 over the two y bounds; the lower bound is tested
// before the upper one at that index, here on the host from the two values.
template <class T>
static ndi_status bicubic_integral_rect(Interp2DImpl<T>& h, const void* xa_, const void* xb_, const void* ya_, const void* yb_,
                                        uint64_t nq, void* out_, uint64_t out_stride, const ndi_eval_opts* opts,
                                        ndi_oob_info* info) {
  ndi_eval_opts o{};
  if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
  if (o.path == NDI_PATH_BUCKETED)
    return fail(NDI_BAD_ARG, "Bicubic has no tile-grouped evaluation form: NDI_PATH_BUCKETED is Bilinear's (AUTO and GATHER "
                "evaluate)");
  if (o.async_launch)
    return fail(NDI_UNSUPPORTED, "ndi_interp2d_integral has no async_launch form: its four bounds do not fit the two-array "
                "record ndi_interp2d_finish reports from (ndi_interp2d_eval of the integral handle has one)");
  if (out_stride < h.lanes)
    return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)out_stride, (unsigned long long)h.lanes);
  if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
  if (nq == 0) return NDI_OK;
  if (!xa_ || !xb_ || !ya_ || !yb_ || !out_) return fail(NDI_BAD_ARG, "null bound / output pointer");
  DeviceGuard dg(h.device);
  Range rg("ndi_interp2d_integral");
  hipStream_t s = (hipStream_t)o.stream;
  SpaceLease lease(h.spaces, s);
  Workspace& ws = lease.ws;
  const T* orig[4] = {(const T*)xa_, (const T*)xb_, (const T*)ya_, (const T*)yb_};
  const T* q[4] = {orig[0], orig[1], orig[2], orig[3]};
  if (o.q_memspace == NDI_MEM_HOST) {        // one allocation, four slices
    ws.qdev.reserve(4 * nq * sizeof(T));
    for (int k = 0; k < 4; ++k) {
      T* d = ws.qdev.template as<T>() + (uint64_t)k * nq;
      NDI_HIP(hipMemcpyAsync(d, orig[k], nq * sizeof(T), hipMemcpyHostToDevice, s));
      q[k] = d;
    }
  }
  ws.ensure_status();
  g_last_path.store(NDI_PATH_GATHER);
  const T x0 = h.px.host_knots.front(), xn = h.px.host_knots.back(), y0 = h.py.host_knots.front(), yn = h.py.host_knots.back();
  // one batch on device pointers; the status is on the host and the stream idle when it returns
  auto batch = [&](uint64_t off, uint64_t cq, T* out, uint64_t stride, bool fresh) -> FirstFail {
    StatusBlock* st = ws.sc[0].status.template as<StatusBlock>();
    reset_status(st, s);
    if (!fresh) {
      const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((cq + BLOCK - 1) / BLOCK, 4096));
      ProfScope ps(s, PC_LOCATE);
      for (int k = 0; k < 2; ++k) {          // (xa, ya), then (xb, yb): both land in the same two words
        hipLaunchKernelGGL(range_check_kernel<T>, dim3(g), dim3(BLOCK), 0, s, q[k] + off, q[2 + k] + off, cq, x0, xn, y0, yn,
                           h.mode, &st->first_fail[0]);
        NDI_HIP(hipGetLastError());
      }
      ps.done();
    }
    bicubic_integral_launch_eval<T>(h, s, st, q[1] + off, q[3] + off, q[0] + off, q[2] + off, cq, out, stride, fresh);
    NDI_HIP(hipMemcpyAsync(ws.host_status, st, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    ws.pending = false;
    return FirstFail{ws.host_status->first_fail[0], ws.host_status->first_fail[1]};
  };
  auto report = [&](FirstFail f, uint64_t off) -> ndi_status {
    const int axis = f.f0 <= f.f1 ? 0 : 1;
    const unsigned long long ff = axis ? f.f1 : f.f0;
    const T* lo = orig[2 * axis] + off;
    const T* hi = orig[2 * axis + 1] + off;
    T v;
    if (o.q_memspace == NDI_MEM_DEVICE) NDI_HIP(hipMemcpy(&v, lo + ff, sizeof(T), hipMemcpyDeviceToHost));
    else v = lo[ff];
    const T k0 = axis ? y0 : x0, kn = axis ? yn : xn;
    const bool lo_bad = (h.mode == EX_NO) ? !((k0 <= v) && (v <= kn)) : !(v == v);
    const T* pick = lo_bad ? lo : hi;
    const Queries<T> qr = axis ? Queries<T>{lo, pick} : Queries<T>{pick, lo};
    return h.report(qr, o.q_memspace, f, off, info);
  };
  if (o.out_memspace == NDI_MEM_DEVICE) {
    const FirstFail f = batch(0, nq, (T*)out_, out_stride, (o.flags & NDI_EVAL_FRESH_OUTPUT) != 0);
    return f.first() == NO_FAIL ? NDI_OK : report(f, 0);
  }
  // host output: a device staging buffer in query chunks of 256 MiB; only the rows before the first failure are copied out
  const uint64_t lanes = h.lanes, row_bytes = lanes * sizeof(T);
  const uint64_t chunk_q = std::max<uint64_t>(1, std::min<uint64_t>(nq, (256ull << 20) / row_bytes));
  ws.stage.reserve(chunk_q * row_bytes);
  for (uint64_t off = 0; off < nq; off += chunk_q) {
    const uint64_t cq = std::min<uint64_t>(chunk_q, nq - off);
    const FirstFail f = batch(off, cq, ws.stage.template as<T>(), lanes, false);
    const uint64_t good = (f.first() == NO_FAIL) ? cq : (uint64_t)f.first();
    if (good)
      NDI_HIP(hipMemcpy2D((T*)out_ + off * out_stride, out_stride * sizeof(T), ws.stage.p, row_bytes, row_bytes, good,
                          hipMemcpyDeviceToHost));
    if (f.first() != NO_FAIL) return report(f, off);
  }
  return NDI_OK;
}
