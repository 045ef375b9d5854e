// csrc/lanewise2d_host.hpp -- the host side of ndi_interp2d_eval_lanewise (an (x, y) per lane:
// out[j][l] = f_l(qx[j][l], qy[j][l])); included by ndinterp_api.hip inside namespace ndi, behind Interp2DImpl and the
// Bicubic launchers.
//
// lanewise2d_run is lanewise_run (lanewise_host.hpp) for two query arrays of one pitch, built from its parts: the same
// refusals, staging of host arrays in row chunks of 256 MiB per array, the status read-back and the first-error report on
// the flat ELEMENT index j * lanes + l -- here per axis, x before y for the same element, as FloatEngine::report has it.
// Interp2DImpl::lanewise_enqueue runs one chunk on device pointers through scratch set 0: the pre-pass
// (lanewise2d_check_kernel) unless the kernel tests the queries itself (`check`: NDI_EVAL_FRESH_OUTPUT, and every chunk that
// goes to the library's own staging buffer), then ONE launch of eval_lanewise2d_kernel.  The search is the pyramid search on
// both axes and there is no two-kernel form.  There is no ring, no sharded form and no async_launch (the
// finish record carries a query index, not an element index).

// Tuning knobs (through NDI_TUNE_LIVE like the 1-D ones):
//   NDI_LANEWISE2D_RECORDS   unset / -1 = auto (the node-record copy for a Bicubic handle, but the plain node table for an
//                            f32 handle whose table is above 256 MiB: DESIGN.md 4.21), 0 = the plain node table, 1 = the
//                            copy (either way only where it fits its cap)
//   NDI_LANEWISE_WGS         workgroups per CU of the grid, shared with the 1-D kernels
constexpr size_t LANEWISE2D_F32_AUTO_LIMIT = (size_t)256 << 20;
static int lanewise2d_records_knob() {
  static const Knob records{"NDI_LANEWISE2D_RECORDS", -1, Knob::live};
  return records.get();
}

// The node-record copy (lanewise2d_records_kernel), built on the first lane-wise call that wants it, by a kernel on the
// caller's stream, under the state machine of Interp1DImpl::lanewise_records / ensure_slopes: calls on other streams are
// ordered behind it with an event until it is known complete; never while the stream is being captured and never fatal -- a
// failed allocation leaves the handle on the plain table.  The copy is shared with the partial handles (lw_records).
template <class T>
const void* Interp2DImpl<T>::lanewise_records(hipStream_t s) {
  LanewiseRecords& R = *lw_records;
  int st = R.state.load(std::memory_order_acquire);
  if (st == 1) return R.buf.p;
  if (st == 2) return nullptr;
  std::lock_guard<std::mutex> g(R.build);
  st = R.state.load(std::memory_order_acquire);
  if (st == 1) return R.buf.p;
  if (st == 2) return nullptr;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
  if (cs != hipStreamCaptureStatusNone) return nullptr;   // this batch reads the plain table
  if (st == 0) {
    const size_t bytes = (size_t)nx * ny * lanes * 4 * sizeof(T);   // the size of the node table
    if (bytes == 0 || bytes > LanewiseRecords::LIMIT) {
      R.state.store(2, std::memory_order_release);
      return nullptr;
    }
    try {
      maybe_fail_lazy_alloc(__LINE__);
      R.buf.reserve(bytes);
      if (!R.ev) NDI_HIP(hipEventCreateWithFlags(&R.ev, hipEventDisableTiming));
      const uint64_t total = nx * ny * lanes;
      const unsigned gr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 65536));
      hipLaunchKernelGGL(lanewise2d_records_kernel<T>, dim3(gr), dim3(BLOCK), 0, s, (const T*)table->template as<T>(),
                         static_cast<LanewiseRecord<T, 4>*>(R.buf.p), nx * ny, lanes);
      NDI_HIP(hipGetLastError());
      NDI_HIP(hipEventRecord(R.ev, s));
    } catch (const HipFailure&) {
      (void)hipGetLastError();
      R.buf.release();
      R.state.store(2, std::memory_order_release);
      return nullptr;
    }
    if (trace_plan()) std::fprintf(stderr, "[ndi plan] lanewise2d records built bytes=%zu\n", bytes);
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
void Interp2DImpl<T>::lanewise_enqueue(hipStream_t s, Workspace& ws, const T* qx, const T* qy, uint64_t q_stride, uint64_t rows,
                                       T* out, uint64_t out_stride, bool check) {
  g_last_path.store(NDI_PATH_GATHER);
  ws.sc[0].status.reserve(sizeof(StatusBlock));
  reset_status(ws.sc[0].status.p, s);
  StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
  const uint64_t total = rows * lanes;
  const size_t knots = (px.lds_bytes + py.lds_bytes + 15) & ~(size_t)15;
  const bool stage = knots <= LDS_STAGE_LIMIT;
  const size_t shmem = stage ? knots : 0;
  uint64_t per_cu = (uint64_t)lanewise_knobs().wgs;
  if (stage) per_cu = std::min<uint64_t>(per_cu, std::max<size_t>(1, (160 * 1024) / std::max<size_t>(shmem, 1)));
  const unsigned grid = lanewise_grid(total, (uint64_t)cu_count() * per_cu);
  Lanewise2DArgs<T> A{};
  A.px = px.view; A.py = py.view;
  A.data = bicubic ? (const T*)table->template as<T>() : (const T*)data.as<T>();
  A.qx = qx; A.qy = qy;
  A.out = out;
  A.G = lanewise_geom(rows, lanes, q_stride, out_stride, grid);
  A.row_elems = layout().row_cells * layout().cell_elems;
  A.cell_elems = layout().cell_elems;
  A.mode = mode;
  A.wrap = wrap_axes();
  A.check = check ? 1 : 0;
  A.first_fail = &st->first_fail[0];
  if (!check) {   // the pre-pass leaves the lowest failing element of either axis in the status block first
    const unsigned cg = lanewise_grid(total, 4096);
    const LanewiseGeom CG = lanewise_geom(rows, lanes, q_stride, out_stride, cg);
    ProfScope ps(s, PC_LOCATE);
    hipLaunchKernelGGL(lanewise2d_check_kernel<T>, dim3(cg), dim3(BLOCK), 0, s, qx, qy, CG, px.host_knots.front(),
                       px.host_knots.back(), py.host_knots.front(), py.host_knots.back(), mode, A.wrap, A.first_fail);
    NDI_HIP(hipGetLastError());
    ps.done();
  }
  // the records are read under the shared side of lw_records->use: trim releases them under the exclusive one
  std::shared_lock<std::shared_mutex> use(lw_records->use);
  // AUTO (measured): a Bicubic handle takes the copy -- it wins on per-lane queries in all sixteen cells --
  // except an f32 handle whose node table is larger than 256 MiB, the one cell where it loses on broadcast queries by more
  // than the spread (Bilinear reads four elements and has no copy)
  const int knob = lanewise2d_records_knob();
  const size_t node_bytes = (size_t)nx * ny * lanes * 4 * sizeof(T);
  const bool want_records = knob >= 0 ? knob != 0 : (sizeof(T) == 8 || node_bytes <= LANEWISE2D_F32_AUTO_LIMIT);
  A.rec = (bicubic && want_records) ? lanewise_records(s) : nullptr;
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] lanewise2d kind=%s stage=%d records=%d nu=%d,%d wrap=%s check=%d grid=%u layout=%s\n",
                 bicubic ? "bicubic" : "bilinear", (int)stage, (int)(A.rec != nullptr), nu_x, nu_y,
                 A.wrap == 0 ? "none" : A.wrap == 1 ? "x" : A.wrap == 2 ? "y" : "xy", A.check, grid,
                 bicubic ? "nodes" : pair_packed ? "packed" : "plain");
  auto go = [&](auto kern) {
    if (stage) allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)LDS_STAGE_LIMIT);
    launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), shmem, kern, A);
  };
  if (!bicubic) {
    pick_bool(stage, [&](auto stage_) { go(eval_lanewise2d_kernel<T, LW2_BILINEAR, stage_, false, 0, 0, false>); });
    return;
  }
  // the orders were checked when the handle was made (Interp2DImpl::partial): 0 .. 2 each
  const bool known = pick<0, 1, 2, 3, 4, 5, 6, 7, 8>(nu_x * 3 + nu_y, [&](auto nu_) {
    constexpr int NX = nu_ / 3, NY = nu_ % 3;
    pick_bool(A.wrap != 0, [&](auto wrap_) {
      pick_bool(stage, [&](auto stage_) {
        pick_bool(A.rec != nullptr, [&](auto rec_) { go(eval_lanewise2d_kernel<T, LW2_BICUBIC, stage_, rec_, NX, NY, wrap_>); });
      });
    });
  });
  if (!known) throw HipFailure{hipErrorInvalidValue, "lanewise_enqueue: partial orders outside 0 .. 2", __LINE__};
}

// The reference's error for the chunk whose lowest failing elements are f0 (x) and f1 (y), relative to row `row0`.
template <class T>
static ndi_status lanewise2d_report(Interp2DImpl<T>& h, const T* qx, const T* qy, uint64_t q_stride, int q_space, uint64_t row0,
                                    unsigned long long f0, unsigned long long f1, ndi_oob_info* info) {
  const int axis = f0 <= f1 ? 0 : 1;   // x before y for the same element (bilinear.rs:71-80)
  const unsigned long long f = axis ? f1 : f0;
  const uint64_t j = row0 + f / h.lanes, l = f % h.lanes;
  const unsigned long long index = (unsigned long long)row0 * h.lanes + f;
  const T* src = (axis ? qy : qx) + j * q_stride + l;
  T v;
  if (q_space == NDI_MEM_DEVICE) NDI_HIP(hipMemcpy(&v, src, sizeof(T), hipMemcpyDeviceToHost));
  else v = *src;
  const ndi_status st = h.failure_status(v);
  if (info) {
    info->index = index;
    info->value = (double)v;
    info->axis = axis;
    info->status = st;
  }
  if (st == NDI_NAN_QUERY) return fail(st, "failed to convert NaN to usize (query %llu)", index);
  return fail(st, "%s = %.17g is not in range", h.axis_name(axis), (double)v);
}

template <class T>
static ndi_status lanewise2d_run(Interp2DImpl<T>& h, const char* what, const void* qx_, const void* qy_, uint64_t nq,
                                 uint64_t q_stride, void* out_, uint64_t out_stride, const ndi_eval_opts* opts,
                                 ndi_oob_info* info) {
  ndi_eval_opts o{};
  if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
  const uint64_t lanes = h.lanes;
  if (o.path == NDI_PATH_BUCKETED)
    return fail(NDI_BAD_ARG, "eval_lanewise of %s: NDI_PATH_BUCKETED groups the queries of a batch by tile, and with a "
                "query per lane a row has no one cell", what);
  if (o.async_launch)
    return fail(NDI_UNSUPPORTED, "eval_lanewise of %s: async_launch is not provided (the finish record carries a query "
                "index, not an element index)", what);
  if (q_stride < lanes)
    return fail(NDI_BAD_ARG, "q_row_stride (%llu) < lanes (%llu)", (unsigned long long)q_stride, (unsigned long long)lanes);
  if (out_stride < lanes)
    return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)out_stride, (unsigned long long)lanes);
  if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
  if (nq == 0) return NDI_OK;
  if (!qx_ || !qy_ || !out_) return fail(NDI_BAD_ARG, "null query / output pointer");
  DeviceGuard dg(h.device);
  Range rg("ndi_interp2d_eval_lanewise");
  hipStream_t s = (hipStream_t)o.stream;
  SpaceLease lease(h.spaces, s);
  Workspace& ws = lease.ws;
  ws.ensure_status();
  const T* qx = (const T*)qx_;
  const T* qy = (const T*)qy_;
  T* out = (T*)out_;
  const bool q_host = o.q_memspace == NDI_MEM_HOST, out_host = o.out_memspace == NDI_MEM_HOST;
  const uint64_t row_bytes = lanes * sizeof(T);
  // host arrays travel through device staging in row chunks of 256 MiB per array; a batch on device pointers is one chunk
  const uint64_t chunk = (q_host || out_host) ? std::max<uint64_t>(1, std::min<uint64_t>(nq, (256ull << 20) / row_bytes)) : nq;
  if (q_host) {
    ws.qdev.reserve(chunk * row_bytes);
    ws.qdev2.reserve(chunk * row_bytes);
  }
  if (out_host) ws.stage.reserve(chunk * row_bytes);
  for (uint64_t off = 0; off < nq; off += chunk) {
    const uint64_t rows = std::min<uint64_t>(chunk, nq - off);
    const T* xd = qx + off * q_stride;
    const T* yd = qy + off * q_stride;
    uint64_t qs = q_stride;
    if (q_host) {   // padded rows are packed on the way up
      NDI_HIP(hipMemcpy2DAsync(ws.qdev.p, row_bytes, xd, q_stride * sizeof(T), row_bytes, rows, hipMemcpyHostToDevice, s));
      NDI_HIP(hipMemcpy2DAsync(ws.qdev2.p, row_bytes, yd, q_stride * sizeof(T), row_bytes, rows, hipMemcpyHostToDevice, s));
      xd = ws.qdev.as<T>();
      yd = ws.qdev2.as<T>();
      qs = lanes;
    }
    T* od = out_host ? ws.stage.as<T>() : out + off * out_stride;
    const uint64_t os = out_host ? lanes : out_stride;
    const bool check = out_host || (o.flags & NDI_EVAL_FRESH_OUTPUT) != 0;
    h.lanewise_enqueue(s, ws, xd, yd, qs, rows, od, os, check);
    NDI_HIP(hipMemcpyAsync(ws.host_status, ws.sc[0].status.p, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    const unsigned long long f0 = ws.host_status->first_fail[0], f1 = ws.host_status->first_fail[1];
    const unsigned long long f = std::min(f0, f1);
    const uint64_t good = f == NO_FAIL ? rows : std::min<uint64_t>(rows, f / lanes);
    if (out_host && good)   // only the rows before the failing row reach the caller
      NDI_HIP(hipMemcpy2D(out + off * out_stride, out_stride * sizeof(T), ws.stage.p, row_bytes, row_bytes, good,
                          hipMemcpyDeviceToHost));
    if (f != NO_FAIL) return lanewise2d_report<T>(h, qx, qy, q_stride, o.q_memspace, off, f0, f1, info);
  }
  return NDI_OK;
}

template <class T>
ndi_status Interp2DImpl<T>::eval_lanewise(const void* qx, const void* qy, uint64_t nq, uint64_t q_stride, void* out,
                                          uint64_t out_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
  if (integral) return Interp2DBase::eval_lanewise(qx, qy, nq, q_stride, out, out_stride, opts, info);
  const char* name = !bicubic ? "Bilinear" : (nu_x || nu_y) ? "a Bicubic partial-derivative handle" : "Bicubic";
  return lanewise2d_run<T>(*this, name, qx, qy, nq, q_stride, out, out_stride, opts, info);
}
