// csrc/bicubic_jet_host.hpp -- host side of the fused value-and-derivatives call of Bicubic (ndi_interp2d_eval_jet);
// included by ndinterp_api.hip after bicubic_host.hpp.
//
// The call writes K = 3 (order 1) or 6 (order 2) output arrays from one evaluation launch (eval_bicubic_jet_kernel), which
// the float host engine (one output, Plan2) does not carry: like the rectangle integral (bicubic_integral_rect) it has a
// synchronous host body of its own here -- staging of host queries, the range pre-pass unless the output is fresh, the
// launch with bicubic_launch_eval's geometry, the host-output chunk loop over one staging allocation cut into K slices, the
// first-error report of the engine.  It has no async_launch, ring or sharded form.
#pragma once

// The launch (the range pre-pass, when there is one, was enqueued before): gx, gy, vchunk, lds and the klds decision are
// bicubic_launch_eval's rules; the vector form needs every part's base 16-byte aligned, else all parts are scalar.
template <class T>
static void bicubic_jet_launch(const Interp2DImpl<T>& h, int order, hipStream_t s, StatusBlock* st, const T* qx, const T* qy,
                               uint64_t nq, T* const* outs, uint64_t out_stride, bool check) {
  constexpr int VN = Wide<T>::N;
  constexpr unsigned TB = 256;
  const int K = order == 1 ? 3 : 6;
  bool vec = (h.lanes % VN == 0) && (out_stride % VN == 0);
  BicubicJetArgs<T> A{};
  for (int k = 0; k < K; ++k) {
    A.out[k] = outs[k];
    vec = vec && aligned16(outs[k]);
  }
  A.px = h.px.view; A.py = h.py.view;
  A.table = h.table->template as<T>();
  A.qx = qx; A.qy = qy;
  A.nq = nq;
  A.out_stride = out_stride;
  A.lv = vec ? h.lanes / VN : h.lanes;
  A.lv_magic = (A.lv >= 2 && A.lv < 64) ? (uint32_t)(((1ull << 32) + A.lv - 1) / A.lv) : 0u;
  uint64_t vchunk = 512;                     // as Bicubic: pieces of 512 vectors, more when that would pass the grid limit
  while ((A.lv + vchunk - 1) / vchunk > 32768) vchunk *= 2;
  A.vchunk = (uint32_t)vchunk;
  const unsigned gy = (unsigned)((A.lv + vchunk - 1) / vchunk);
  A.mode = h.mode;
  A.wrap = h.wrap_axes();
  A.first_fail = &st->first_fail[0];
  A.check = check ? 1 : 0;
  const size_t strips = (size_t)(TB / 64) * 64 * (sizeof(unsigned long long) + 4 * sizeof(T));
  const size_t knots = (h.px.lds_bytes + h.py.lds_bytes + 15) & ~(size_t)15;
  const bool klds = knots + strips <= LDS_STAGE_LIMIT;
  const size_t lds = (klds ? knots : 0) + strips;
  const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + TB - 1) / TB,
                                                                        std::max<uint64_t>(1, (uint64_t)cu_count() * wgs_per_cu(lds, TB) * 4 / gy)));
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] bicubic_jet order=%d vec=%d lv=%llu klds=%d grid=%u x %u lds=%zu prepass=%d%s\n", order,
                 (int)vec, (unsigned long long)A.lv, (int)klds, gx, gy, lds, check ? 0 : 1,
                 A.wrap == 0 ? "" : A.wrap == 1 ? " wrap=x" : A.wrap == 2 ? " wrap=y" : " wrap=xy");   // (as bicubic_launch_eval's)
  pick_or<2, 1>(order, [&](auto ord_) {
    constexpr int ORD = ord_;
    bicubic_pick_form<T>(vec, klds, [&](auto vec_, auto kl_) {
      // (a handle that wraps: the wrap kernel, as bicubic_launch_eval's WRAP variant)
      if (A.wrap != 0)
        launch_lds<T>(eval_bicubic_jet_wrap_kernel<T, vec_, kl_, TB, ORD>, LDS_STAGE_LIMIT, s, PC_EVAL, dim3(gx, gy), dim3(TB), lds, A);
      else
        launch_lds<T>(eval_bicubic_jet_kernel<T, vec_, kl_, TB, ORD>, LDS_STAGE_LIMIT, s, PC_EVAL, dim3(gx, gy), dim3(TB), lds, A);
    });
  });
}

// ndi_interp2d_eval_jet of a Bicubic surface handle (Interp2DImpl::eval_jet has refused every other handle).  Every
// refusal is decided before any device work.
template <class T>
static ndi_status bicubic_jet_eval(Interp2DImpl<T>& h, int order, const void* qx_, const void* qy_, uint64_t nq,
                                   void* const* outs_, uint64_t out_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
  if (order != 1 && order != 2)
    return fail(NDI_BAD_ARG, "Bicubic: ndi_interp2d_eval_jet takes order 1 (value and gradient) or 2 (with the three second "
                "derivatives), got %d: the third derivative of a cubic spline jumps at the grid lines", order);
  const int K = order == 1 ? 3 : 6;
  ndi_eval_opts o{};
  if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
  if (o.path == NDI_PATH_BUCKETED)
    return fail(NDI_BAD_ARG, "Bicubic has no tile-grouped evaluation form: NDI_PATH_BUCKETED is Bilinear's (AUTO and GATHER "
                "evaluate)");
  if (o.async_launch)
    return fail(NDI_UNSUPPORTED, "Bicubic: ndi_interp2d_eval_jet has no async_launch form: it completes before it returns "
                "(ndi_interp2d_eval of the handle and of its ndi_interp2d_partial handles has one)");
  if (out_stride < h.lanes)
    return fail(NDI_BAD_ARG, "Bicubic: ndi_interp2d_eval_jet: out_row_stride (%llu) < lanes (%llu)",
                (unsigned long long)out_stride, (unsigned long long)h.lanes);
  if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
  if (nq == 0) return NDI_OK;
  if (!qx_ || !qy_) return fail(NDI_BAD_ARG, "Bicubic: ndi_interp2d_eval_jet: null query pointer");
  for (int k = 0; k < K; ++k) {
    if (!outs_[k])
      return fail(NDI_BAD_ARG, "Bicubic: ndi_interp2d_eval_jet: outs[%d] is null (order %d writes %d parts; parts cannot be "
                  "skipped)", k, order, K);
    for (int j = 0; j < k; ++j)
      if (outs_[j] == outs_[k])
        return fail(NDI_BAD_ARG, "Bicubic: ndi_interp2d_eval_jet: outs[%d] and outs[%d] are the same pointer (parts must not "
                    "overlap)", j, k);
  }
  DeviceGuard dg(h.device);
  Range rg("ndi_interp2d_eval_jet");
  hipStream_t s = (hipStream_t)o.stream;
  SpaceLease lease(h.spaces, s);
  Workspace& ws = lease.ws;
  const Queries<T> orig{(const T*)qx_, (const T*)qy_};
  const Queries<T> q = h.stage_queries(s, ws, orig, nq, o.q_memspace);
  ws.ensure_status();
  // one batch on device pointers; the status is on the host and the stream idle when it returns
  auto batch = [&](uint64_t off, uint64_t cq, T* const* outs, uint64_t stride, bool fresh) -> FirstFail {
    StatusBlock* st = ws.sc[0].status.template as<StatusBlock>();
    reset_status(st, s);
    h.range_prepass(s, ws.sc[0], q + off, cq, fresh);
    bicubic_jet_launch<T>(h, order, s, st, q.a + off, q.b + off, cq, outs, stride, fresh);
    NDI_HIP(hipMemcpyAsync(ws.host_status, st, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    ws.pending = false;
    return FirstFail{ws.host_status->first_fail[0], ws.host_status->first_fail[1]};
  };
  T* parts[JET_MAX_PARTS] = {};
  if (o.out_memspace == NDI_MEM_DEVICE) {
    for (int k = 0; k < K; ++k) parts[k] = (T*)outs_[k];
    const FirstFail f = batch(0, nq, parts, out_stride, (o.flags & NDI_EVAL_FRESH_OUTPUT) != 0);
    return f.first() == NO_FAIL ? NDI_OK : h.report(orig, o.q_memspace, f, 0, info);
  }
  // host output: ONE device staging buffer cut into K slices (each a multiple of 16 bytes, so the slices keep the vector
  // form), in query chunks so that the slices together stay within 256 MiB; per part only the rows before the first
  // failure are copied out
  const uint64_t lanes = h.lanes, row_bytes = lanes * sizeof(T);
  const uint64_t slice_limit = ((256ull << 20) / (uint64_t)K) & ~15ull;
  const uint64_t chunk_q = std::max<uint64_t>(1, std::min<uint64_t>(nq, slice_limit / row_bytes));
  const uint64_t slice_bytes = (chunk_q * row_bytes + 15) & ~15ull;
  ws.stage.reserve((size_t)K * slice_bytes);
  for (int k = 0; k < K; ++k) parts[k] = reinterpret_cast<T*>(static_cast<char*>(ws.stage.p) + (size_t)k * slice_bytes);
  for (uint64_t off = 0; off < nq; off += chunk_q) {
    const uint64_t cq = std::min<uint64_t>(chunk_q, nq - off);
    const FirstFail f = batch(off, cq, parts, lanes, false);
    const uint64_t good = (f.first() == NO_FAIL) ? cq : (uint64_t)f.first();
    if (good)
      for (int k = 0; k < K; ++k)
        NDI_HIP(hipMemcpy2D((T*)outs_[k] + off * out_stride, out_stride * sizeof(T), parts[k], row_bytes, row_bytes, good,
                            hipMemcpyDeviceToHost));
    if (f.first() != NO_FAIL) return h.report(orig + off, o.q_memspace, f, off, info);
  }
  return NDI_OK;
}
