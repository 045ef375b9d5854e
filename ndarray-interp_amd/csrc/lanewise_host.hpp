// csrc/lanewise_host.hpp -- the host side of ndi_interp1d_eval_lanewise (a query per lane: out[j][l] = f_l(q[j][l]));
// included by ndinterp_api.hip inside namespace ndi, behind Interp1DImpl, AntiderivImpl and InverseImpl.
//
// One driver (lanewise_run) serves the three f32 / f64 families: the refusals, staging of host queries and outputs in row
// chunks, the status read-back and the first-error report on the flat ELEMENT index j * lanes + l.  A family supplies
// lanewise_enqueue(s, ws, q, q_stride, rows, out, out_stride, check): one chunk on device pointers through scratch set 0,
// which leaves the chunk's lowest failing element in that set's first_fail[0].  `check`: the kernel tests the queries itself
// (NDI_EVAL_FRESH_OUTPUT, and every chunk that goes to the library's own staging buffer); otherwise a pre-pass
// (lanewise_check_kernel) runs first and the rows at / after the failing row stay untouched.
//   Interp1DImpl   the fused kernel (eval_lanewise_kernel), from the element-record copy or the plain tables; or the
//                  two-kernel form (locate_kernel over the flat queries, then lanewise_point_kernel)
//   AntiderivImpl  the two-kernel form only, as its row-wise evaluation
//   InverseImpl    inverse_lanewise_kernel, with lane l's OWN value range as the limits
// There is no zero-copy path, no ring, no sharded form and no async_launch (the finish record carries a query index, not an
// element index).

// Tuning knobs (through NDI_TUNE_LIVE like the short-row ones):
//   NDI_LANEWISE_MODE      0 = auto (the fused kernel, except Linear on scalar data whose axis does not fit LDS), 1 = the
//                          two-kernel form, 2 = the fused kernel (Linear / cubic handles)
//   NDI_LANEWISE_RECORDS   unset / -1 = auto (rows shorter than a wavefront; Linear only with a data table above 4 MiB),
//                          0 = the plain tables, 1 = the element-record copy (where it fits its cap)
//   NDI_LANEWISE_WGS       workgroups per CU of the element kernels' grids
struct LanewiseKnobs {
  int mode, records, wgs;
};
static LanewiseKnobs lanewise_knobs() {
  static const Knob mode{"NDI_LANEWISE_MODE", 0, Knob::live}, records{"NDI_LANEWISE_RECORDS", -1, Knob::live},
      wgs{"NDI_LANEWISE_WGS", 8, Knob::live};
  const int w = wgs.get();
  return {mode.get(), records.get(), w < 1 || w > 64 ? 8 : w};
}

// Grid of an element kernel over `total` elements and the geometry its threads advance by.
static unsigned lanewise_grid(uint64_t total, uint64_t max_blocks) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, std::max<uint64_t>(max_blocks, 1)));
}
static LanewiseGeom lanewise_geom(uint64_t rows, uint64_t lanes, uint64_t q_stride, uint64_t out_stride, unsigned grid) {
  const uint64_t step = (uint64_t)grid * BLOCK;
  return LanewiseGeom{lanes, rows, q_stride, out_stride, step / lanes, step % lanes};
}

template <class T>
static void lanewise_prepass(hipStream_t s, const T* q, const LanewiseGeom& G0, T x0, T xn, int mode, const T* lo, const T* hi,
                             unsigned long long* first_fail) {
  const unsigned grid = lanewise_grid(G0.rows * G0.lanes, 4096);
  const LanewiseGeom G = lanewise_geom(G0.rows, G0.lanes, G0.q_stride, G0.out_stride, grid);
  ProfScope ps(s, PC_LOCATE);
  hipLaunchKernelGGL(lanewise_check_kernel<T>, dim3(grid), dim3(BLOCK), 0, s, q, G, x0, xn, mode, lo, hi, first_fail);
  NDI_HIP(hipGetLastError());
  ps.done();
}

// The two-kernel form: locate_kernel over the flat rows * lanes queries (rows with a pitch above lanes are packed first),
// then ONE element launch that reads idx[] / t[].  locate_kernel publishes the lowest failing element itself, so the form
// needs no pre-pass: rows at / after the failing row are never written.
template <class T>
static void lanewise_two_kernel(hipStream_t s, Workspace& ws, const DevicePyramid<T>& pyr, int mode, int kind, uint64_t n,
                                const T* y, const T* a, const T* b, const T* P, const T* q, uint64_t q_stride, uint64_t rows,
                                uint64_t lanes, T* out, uint64_t out_stride, int wgs) {
  Scratch& sc = ws.sc[0];
  StatusBlock* st = sc.status.as<StatusBlock>();
  const uint64_t total = rows * lanes;
  if (q_stride != lanes) {
    sc.recq.reserve(total * sizeof(T));
    NDI_HIP(hipMemcpy2DAsync(sc.recq.p, lanes * sizeof(T), q, q_stride * sizeof(T), lanes * sizeof(T), rows,
                             hipMemcpyDeviceToDevice, s));
    q = sc.recq.as<T>();
  }
  const bool with_t = kind != LW_LINEAR;
  sc.idx.reserve(total * sizeof(uint32_t));
  if (with_t) sc.t.reserve(total * sizeof(T));
  run_locate<T>(s, pyr, q, total, sc.idx.as<uint32_t>(), nullptr, with_t ? sc.t.as<T>() : nullptr, &st->first_fail[0], mode);
  const unsigned grid = lanewise_grid(total, (uint64_t)cu_count() * wgs);
  LanewisePointArgs<T> A{};
  A.knots = pyr.view.lv0;
  A.y = y; A.a = a; A.b = b; A.P = P;
  A.q = q;
  A.idx = sc.idx.as<uint32_t>();
  A.t = sc.t.as<T>();
  A.out = out;
  A.G = lanewise_geom(rows, lanes, lanes, out_stride, grid);
  A.first_fail = &st->first_fail[0];
  A.n_int = (uint32_t)(n - 1);
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] lanewise form=two-kernel kind=%d packed_q=%d grid=%u\n", kind, (int)(q_stride != lanes), grid);
  switch (kind) {
    case LW_LINEAR: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, lanewise_point_kernel<T, LW_LINEAR>, A); break;
    case LW_CUBIC: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, lanewise_point_kernel<T, LW_CUBIC>, A); break;
    case LW_ANTI_LINEAR: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, lanewise_point_kernel<T, LW_ANTI_LINEAR>, A); break;
    default: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, lanewise_point_kernel<T, LW_ANTI_CUBIC>, A); break;
  }
}

// ---- the driver ---------------------------------------------------------------------------------------------------------
template <class T, class Impl>
static ndi_status lanewise_report(Impl& h, const T* q, uint64_t q_stride, int q_space, uint64_t row0, unsigned long long f,
                                  ndi_oob_info* info) {
  const uint64_t j = row0 + f / h.lanes, l = f % h.lanes;
  const unsigned long long index = (unsigned long long)row0 * h.lanes + f;
  const T* src = q + j * q_stride + l;
  T v;
  if (q_space == NDI_MEM_DEVICE) NDI_HIP(hipMemcpy(&v, src, sizeof(T), hipMemcpyDeviceToHost));
  else v = *src;
  const ndi_status st = h.failure_status(v);
  if (info) {
    info->index = index;
    info->value = (double)v;
    info->axis = 0;
    info->status = st;
  }
  if (st == NDI_NAN_QUERY) return fail(st, "failed to convert NaN to usize (query %llu)", index);
  return fail(st, "%s = %.17g is not in range", h.axis_name(0), (double)v);
}

template <class T, class Impl>
static ndi_status lanewise_run(Impl& h, const char* what, const void* q_, uint64_t nq, uint64_t q_stride, void* out_,
                               uint64_t out_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
  ndi_eval_opts o{};
  if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
  const uint64_t lanes = h.lanes;
  if (o.path == NDI_PATH_BUCKETED)
    return fail(NDI_BAD_ARG, "eval_lanewise of %s: NDI_PATH_BUCKETED groups the queries of a batch by interval, and with a "
                "query per lane a row has no one interval", what);
  if (o.async_launch)
    return fail(NDI_UNSUPPORTED, "eval_lanewise of %s: async_launch is not provided (the finish record carries a query "
                "index, not an element index)", what);
  if (q_stride < lanes)
    return fail(NDI_BAD_ARG, "q_row_stride (%llu) < lanes (%llu)", (unsigned long long)q_stride, (unsigned long long)lanes);
  if (out_stride < lanes)
    return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)out_stride, (unsigned long long)lanes);
  if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
  if (nq == 0) return NDI_OK;
  if (!q_ || !out_) return fail(NDI_BAD_ARG, "null query / output pointer");
  DeviceGuard dg(h.device);
  Range rg("ndi_interp1d_eval_lanewise");
  hipStream_t s = (hipStream_t)o.stream;
  SpaceLease lease(h.spaces, s);
  Workspace& ws = lease.ws;
  ws.ensure_status();
  const T* q = (const T*)q_;
  T* out = (T*)out_;
  const bool q_host = o.q_memspace == NDI_MEM_HOST, out_host = o.out_memspace == NDI_MEM_HOST;
  const uint64_t row_bytes = lanes * sizeof(T);
  // host arrays travel through device staging in row chunks of 256 MiB; a batch on device pointers is one chunk
  const uint64_t chunk = (q_host || out_host) ? std::max<uint64_t>(1, std::min<uint64_t>(nq, (256ull << 20) / row_bytes)) : nq;
  if (q_host) ws.qdev.reserve(chunk * row_bytes);
  if (out_host) ws.stage.reserve(chunk * row_bytes);
  for (uint64_t off = 0; off < nq; off += chunk) {
    const uint64_t rows = std::min<uint64_t>(chunk, nq - off);
    const T* qd = q + off * q_stride;
    uint64_t qs = q_stride;
    if (q_host) {
      NDI_HIP(hipMemcpy2DAsync(ws.qdev.p, row_bytes, qd, q_stride * sizeof(T), row_bytes, rows, hipMemcpyHostToDevice, s));
      qd = ws.qdev.as<T>();
      qs = lanes;
    }
    T* od = out_host ? ws.stage.as<T>() : out + off * out_stride;
    const uint64_t os = out_host ? lanes : out_stride;
    const bool check = out_host || (o.flags & NDI_EVAL_FRESH_OUTPUT) != 0;
    h.lanewise_enqueue(s, ws, qd, qs, rows, od, os, check);
    NDI_HIP(hipMemcpyAsync(ws.host_status, ws.sc[0].status.p, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    const unsigned long long f = ws.host_status->first_fail[0];
    const uint64_t good = f == NO_FAIL ? rows : std::min<uint64_t>(rows, f / lanes);
    if (out_host && good)   // only the rows before the failing row reach the caller
      NDI_HIP(hipMemcpy2D(out + off * out_stride, out_stride * sizeof(T), ws.stage.p, row_bytes, row_bytes, good,
                          hipMemcpyDeviceToHost));
    if (f != NO_FAIL) return lanewise_report<T>(h, q, q_stride, o.q_memspace, off, f, info);
  }
  return NDI_OK;
}

// ---- Linear and the cubic class -------------------------------------------------------------------------------------------
// The element-record copy (lanewise_records_kernel), built on the first lane-wise call that wants it, by a kernel on the
// caller's stream; calls on other streams are ordered behind it with an event until it is known complete.  Never while
// the stream is being captured and never fatal: a failed allocation leaves the handle on the plain tables.
template <class T>
const void* Interp1DImpl<T>::lanewise_records(hipStream_t s) {
  LanewiseRecords& R = records;
  int st = R.state.load(std::memory_order_acquire);
  if (st == 1) return R.buf.p;
  if (st == 2) return nullptr;
  std::lock_guard<std::mutex> g(R.build);
  st = R.state.load(std::memory_order_acquire);
  if (st == 1) return R.buf.p;
  if (st == 2) return nullptr;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
  if (cs != hipStreamCaptureStatusNone) return nullptr;   // this batch reads the plain tables
  if (st == 0) {
    const bool cubic = strategy == NDI_CUBIC_SPLINE;
    const size_t bytes = (size_t)(n - 1) * lanes * (cubic ? 4 : 2) * sizeof(T);
    if (bytes == 0 || bytes > LanewiseRecords::LIMIT) {
      R.state.store(2, std::memory_order_release);
      return nullptr;
    }
    try {
      maybe_fail_lazy_alloc(__LINE__);
      R.buf.reserve(bytes);
      if (!R.ev) NDI_HIP(hipEventCreateWithFlags(&R.ev, hipEventDisableTiming));
      const uint64_t total = (n - 1) * lanes;
      const unsigned gr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 65536));
      if (cubic)
        hipLaunchKernelGGL((lanewise_records_kernel<T, 4>), dim3(gr), dim3(BLOCK), 0, s, (const T*)data.as<T>(),
                           (const T*)ca.as<T>(), (const T*)cb.as<T>(), static_cast<LanewiseRecord<T, 4>*>(R.buf.p), n, lanes);
      else
        hipLaunchKernelGGL((lanewise_records_kernel<T, 2>), dim3(gr), dim3(BLOCK), 0, s, (const T*)data.as<T>(),
                           (const T*)nullptr, (const T*)nullptr, static_cast<LanewiseRecord<T, 2>*>(R.buf.p), n, lanes);
      NDI_HIP(hipGetLastError());
      NDI_HIP(hipEventRecord(R.ev, s));
    } catch (const HipFailure&) {
      (void)hipGetLastError();
      R.buf.release();
      R.state.store(2, std::memory_order_release);
      return nullptr;
    }
    if (trace_plan()) std::fprintf(stderr, "[ndi plan] lanewise records built bytes=%zu\n", bytes);
    R.stream = s;
    R.state.store(3, std::memory_order_release);
    return R.buf.p;
  }
  // st == 3
  if (hipEventQuery(R.ev) == hipSuccess) {
    R.state.store(1, std::memory_order_release);
    return R.buf.p;
  }
  (void)hipGetLastError();
  if (s != R.stream) NDI_HIP(hipStreamWaitEvent(s, R.ev, 0));
  return R.buf.p;
}

template <class T>
void Interp1DImpl<T>::lanewise_enqueue(hipStream_t s, Workspace& ws, const T* q, uint64_t q_stride, uint64_t rows, T* out,
                                       uint64_t out_stride, bool check) {
  g_last_path.store(NDI_PATH_GATHER);
  const LanewiseKnobs K = lanewise_knobs();
  const bool cubic = strategy == NDI_CUBIC_SPLINE;
  ws.sc[0].status.reserve(sizeof(StatusBlock));
  reset_status(ws.sc[0].status.p, s);
  StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
  const bool stage = pyr.lds_bytes <= LDS_STAGE_LIMIT;
  // AUTO (measured): the fused kernel, except Linear on scalar data whose axis does not fit LDS
  if (K.mode == 1 || (K.mode == 0 && !cubic && lanes == 1 && !stage)) {
    lanewise_two_kernel<T>(s, ws, pyr, mode, cubic ? LW_CUBIC : LW_LINEAR, n, data.as<T>(), ca.as<T>(), cb.as<T>(),
                           (const T*)nullptr, q, q_stride, rows, lanes, out, out_stride, K.wgs);
    return;
  }
  const uint64_t total = rows * lanes;
  size_t shmem = stage ? ((pyr.lds_bytes + 15) & ~(size_t)15) : 0;
  // the axis' bucket index, where run_locate would use it: staged behind the pyramid, or read from global memory
  BucketIndex<T> bx{nullptr, 0, T(0)};
  BucketIndex32<T> bx32{nullptr, 0, T(0)};
  if (total >= 4096) {
    if (stage) {
      pyr.ensure_bucket_index();
      if (pyr.lut_bytes && shmem + pyr.lut_bytes <= LDS_STAGE_LIMIT) {
        bx = pyr.bidx;
        shmem += pyr.lut_bytes;
      }
    } else {
      pyr.ensure_bucket_index32();
      bx32 = pyr.bidx32;
    }
  }
  uint64_t per_cu = (uint64_t)K.wgs;
  if (stage) per_cu = std::min<uint64_t>(per_cu, std::max<size_t>(1, (160 * 1024) / std::max<size_t>(shmem, 1)));
  const unsigned grid = lanewise_grid(total, (uint64_t)cu_count() * per_cu);
  LanewiseArgs<T> A{};
  A.pyr = pyr.view;
  A.bx = bx;
  A.bx32 = bx32;
  A.data = data.as<T>();
  A.ca = ca.as<T>();
  A.cb = cb.as<T>();
  A.q = q;
  A.out = out;
  A.G = lanewise_geom(rows, lanes, q_stride, out_stride, grid);
  A.mode = mode;
  A.check = check ? 1 : 0;
  A.first_fail = &st->first_fail[0];
  if (!check)
    lanewise_prepass<T>(s, q, A.G, pyr.host_knots.front(), pyr.host_knots.back(), mode, (const T*)nullptr, (const T*)nullptr,
                        A.first_fail);
  // the records are read under the shared side of records.use: trim releases them under the exclusive one
  std::shared_lock<std::shared_mutex> use(records.use);
  // AUTO (measured): rows shorter than a wavefront -- and Linear, whose record saves one read of two,
  // only where the data table is larger than the 4 MiB L2
  const bool want_records = K.records >= 0 ? K.records != 0
                                           : lanes < 64 && (cubic || (size_t)n * lanes * sizeof(T) > ((size_t)4 << 20));
  A.rec = want_records ? lanewise_records(s) : nullptr;
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] lanewise form=fused cubic=%d stage=%d lut=%d records=%d check=%d grid=%u\n", (int)cubic,
                 (int)stage, bx.lut ? 1 : (bx32.lut ? 2 : 0), (int)(A.rec != nullptr), A.check, grid);
  pick<ST_CUBIC, ST_LINEAR>(strat(), [&](auto st_) {
    constexpr int ST = st_;
    pick_bool(stage, [&](auto stage_) {
      constexpr bool STAGE = stage_;
      pick_bool(A.rec != nullptr, [&](auto rec_) {
        auto kern = eval_lanewise_kernel<T, ST, STAGE, rec_>;
        if (STAGE) allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)LDS_STAGE_LIMIT);
        launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), shmem, kern, A);
      });
    });
  });
}

template <class T>
ndi_status Interp1DImpl<T>::eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                                          const ndi_eval_opts* opts, ndi_oob_info* info) {
  const char* name = strategy == NDI_CUBIC_SPLINE ? hermite_rule_name(rule) : "Linear";
  return lanewise_run<T>(*this, name, q, nq, q_stride, out, out_stride, opts, info);
}

// ---- antiderivative handles: the two-kernel form only ---------------------------------------------------------------------
template <class T>
void AntiderivImpl<T>::lanewise_enqueue(hipStream_t s, Workspace& ws, const T* q, uint64_t q_stride, uint64_t rows, T* out,
                                        uint64_t out_stride, bool) {
  g_last_path.store(NDI_PATH_GATHER);
  ws.sc[0].status.reserve(sizeof(StatusBlock));
  reset_status(ws.sc[0].status.p, s);
  lanewise_two_kernel<T>(s, ws, pyr, mode, linear ? LW_ANTI_LINEAR : LW_ANTI_CUBIC, n, y.as<T>(), a.as<T>(), b.as<T>(), P.as<T>(),
                         q, q_stride, rows, lanes, out, out_stride, lanewise_knobs().wgs);
}

template <class T>
ndi_status AntiderivImpl<T>::eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                                           const ndi_eval_opts* opts, ndi_oob_info* info) {
  const std::string what = std::string("the antiderivative of ") + source_name();
  return lanewise_run<T>(*this, what.c_str(), q, nq, q_stride, out, out_stride, opts, info);
}

// ---- inverse handles: lane l's own value range ------------------------------------------------------------------------------
template <class T>
void InverseImpl<T>::lanewise_enqueue(hipStream_t s, Workspace& ws, const T* q, uint64_t q_stride, uint64_t rows, T* out,
                                      uint64_t out_stride, bool check) {
  g_last_path.store(NDI_PATH_GATHER);
  ws.sc[0].status.reserve(sizeof(StatusBlock));
  reset_status(ws.sc[0].status.p, s);
  StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
  const uint64_t total = rows * lanes;
  const unsigned grid = lanewise_grid(total, (uint64_t)cu_count() * lanewise_knobs().wgs);
  LanewiseInverseArgs<T> W{};
  W.A.knots = pyr.view.lv0;
  W.A.N = node_table();
  W.A.y = y.as<T>(); W.A.a = a.as<T>(); W.A.b = b.as<T>();
  W.A.n = n; W.A.lanes = lanes;
  W.q = q;
  W.out = out;
  W.lo = lane_dev.as<T>();
  W.hi = lane_dev.as<T>() + lanes;
  W.G = lanewise_geom(rows, lanes, q_stride, out_stride, grid);
  W.check = check ? 1 : 0;
  W.first_fail = &st->first_fail[0];
  if (!check) lanewise_prepass<T>(s, q, W.G, T(0), T(0), (int)EX_NO, W.lo, W.hi, W.first_fail);
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] lanewise form=inverse class=%d check=%d grid=%u\n", cls, W.check, grid);
  switch (cls) {
    case IC_LINEAR: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_lanewise_kernel<T, IC_LINEAR>, W); break;
    case IC_CUBIC: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_lanewise_kernel<T, IC_CUBIC>, W); break;
    case IC_ANTI_CUBIC: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_lanewise_kernel<T, IC_ANTI_CUBIC>, W); break;
    default: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_lanewise_kernel<T, IC_ANTI_LINEAR>, W); break;
  }
}

template <class T>
ndi_status InverseImpl<T>::eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                                         const ndi_eval_opts* opts, ndi_oob_info* info) {
  const std::string what = std::string("the inverse of ") + source_name();
  return lanewise_run<T>(*this, what.c_str(), q, nq, q_stride, out, out_stride, opts, info);
}
