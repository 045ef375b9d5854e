// csrc/lane_axes_host.hpp -- the host side of handles with an x axis per lane (ndi_interp1d_create_lane_axes); included by
// ndinterp_api.hip inside namespace ndi, behind lanewise_host.hpp.
//
// A lane-axes handle is an Interp1DBase of its own on FloatEngine, like an inverse handle, and follows its shape: it owns
// copies of the knot table x[n][lanes], the data and (cubic class) the a / b tables.  Creation checks every column (host
// arrays: on the host, before any device work -- host_logic.hpp; device arrays: ONE pass of lane_axes_check_kernel), keeps
// the range common to all lanes [Lo, Hi] on the host and the per-lane ranges on the device, and builds the tables on the
// NULL stream, complete on return; the cubic class also keeps the record copy R[i][l] = {x, y, a, b} its evaluation reads
// (DESIGN.md 4.23).  Evaluation is ONE launch of lane_axes_eval_kernel for either entry point: the row-wise
// call behind the range pre-pass on [Lo, Hi] (eval_body), the lane-wise call through lanewise_run with each lane's own
// range.  Staging, the first-error report, the host-output chunk loop, finish and trim are the engine's.

// NDI_LANE_AXES_RECORDS (through NDI_TUNE_LIVE like the other knobs): the cubic class evaluates from the
// record copy R[i][l] = {x, y, a, b} wherever the handle has one -- measured faster than the plain tables at every shape,
// element type and query kind tried, by 15 to 35 % (tools/lane_axes_bench.py).  0 = the plain tables: the
// other side of that measurement.
static bool lane_axes_use_records() {
  static const Knob records{"NDI_LANE_AXES_RECORDS", 1, Knob::live};
  return records.get() != 0;
}

template <class T>
struct LaneAxesImpl final : Interp1DBase, FloatEngine<T, LaneAxesImpl<T>> {
  int strategy = NDI_LINEAR;   // the evaluation class, as Interp1DImpl: NDI_CUBIC_SPLINE = "has a / b tables"
  int rule = HR_SPLINE;
  int mode = EX_NO;            // EX_NO / EX_YES: each lane continues its own end interval
  uint64_t n = 0;
  DevBuf x, y, a, b;           // x, y: [n][lanes]; a, b: [n-1][lanes] (cubic class)
  T Lo = T(0), Hi = T(0);      // the range common to all lanes: max_l x[0][l], min_l x[n-1][l] (Lo > Hi: no query passes)
  std::vector<T> lane_limits;  // [2][lanes]: x[0][l] and x[n-1][l], lane l's own range (the lane-wise evaluation)
  DevBuf lane_dev;             // ... and its device copy
  // the record copy of the cubic class (lane_axes_records_kernel), made at creation / clone like the tables; none above
  // its memory cap or where its allocation fails: the plain tables then serve
  DevBuf rec;
  static constexpr size_t REC_LIMIT = 1ull << 30;
  SpaceSet spaces;

  bool cubic() const { return strategy == NDI_CUBIC_SPLINE; }
  const char* name() const { return cubic() ? hermite_rule_name(rule) : "Linear"; }

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, lane_limits.data(), lane_limits.size() * sizeof(T));
    const uint64_t f[3] = {n, (uint64_t)strategy | ((uint64_t)rule << 8) | (1ull << 26) /* lane axes */, (uint64_t)mode};
    return fnv1a(h, f, sizeof(f));
  }

  void reserve_tables() {
    const size_t data_b = (size_t)n * lanes * sizeof(T);
    x.reserve(data_b);
    y.reserve(data_b);
    if (cubic()) {
      a.reserve((size_t)(n - 1) * lanes * sizeof(T));
      b.reserve((size_t)(n - 1) * lanes * sizeof(T));
    }
  }
  void upload_lane_limits() {
    lane_dev.reserve((size_t)2 * lanes * sizeof(T));
    NDI_HIP(hipMemcpy(lane_dev.p, lane_limits.data(), (size_t)2 * lanes * sizeof(T), hipMemcpyHostToDevice));
  }

  // ---- creation (NULL stream, complete on return) ------------------------------------------------------------------------
  // Device-resident axes: the monotonicity pass over the handle's copy of x.
  ndi_status check_columns() {
    Range rg("ndi:lane_axes_check");
    const hipStream_t s0 = nullptr;
    DevBuf flags;
    flags.reserve((size_t)lanes * sizeof(unsigned int));
    NDI_HIP(hipMemsetAsync(flags.p, 0, (size_t)lanes * sizeof(unsigned int), s0));
    const uint64_t total = ((n + INV_CHECK_RUN - 1) / INV_CHECK_RUN) * lanes;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
    hipLaunchKernelGGL(lane_axes_check_kernel<T>, dim3(grid), dim3(BLOCK), 0, s0, (const T*)x.as<T>(), n, lanes,
                       flags.as<unsigned int>());
    NDI_HIP(hipGetLastError());
    std::vector<unsigned int> hf(lanes);
    NDI_HIP(hipMemcpy(hf.data(), flags.p, (size_t)lanes * sizeof(unsigned int), hipMemcpyDeviceToHost));
    for (uint64_t l = 0; l < lanes; ++l)
      if (hf[l]) return lane_axes_monotonic_error(l);
    return NDI_OK;
  }

  // The first and last row of x: every lane's own range and the range common to all of them.
  void take_ranges() {
    lane_limits.resize((size_t)2 * lanes);
    NDI_HIP(hipMemcpy(lane_limits.data(), x.p, (size_t)lanes * sizeof(T), hipMemcpyDeviceToHost));
    NDI_HIP(hipMemcpy(lane_limits.data() + lanes, x.as<T>() + (size_t)(n - 1) * lanes, (size_t)lanes * sizeof(T),
                      hipMemcpyDeviceToHost));
    Lo = lane_limits[0];
    Hi = lane_limits[lanes];
    for (uint64_t l = 1; l < lanes; ++l) {
      Lo = std::max(Lo, lane_limits[l]);
      Hi = std::min(Hi, lane_limits[lanes + l]);
    }
    upload_lane_limits();
  }

  // CubicSpline: one thread per lane, the whole plan per lane (lane_axes_spline_kernel); the scratch is freed on return.
  void build_spline(const ndi_interp1d_desc& d) {
    Range rg("ndi:lane_axes_spline_build");
    int lk, rk;
    double lv, rv;
    specialize_end(d.left.kind, d.left.value, lk, lv);
    specialize_end(d.right.kind, d.right.value, rk, rv);
    DevBuf scratch;
    scratch.reserve((size_t)2 * n * lanes * sizeof(T));
    LaneAxesSplineArgs<T> A{};
    A.x = x.as<T>(); A.y = y.as<T>(); A.ca = a.as<T>(); A.cb = b.as<T>();
    A.mp = scratch.as<T>();
    A.rr = scratch.as<T>() + (size_t)n * lanes;
    A.n = n; A.lanes = lanes;
    A.left_kind = lk; A.right_kind = rk;
    A.left_val = T(lv); A.right_val = T(rv);
    A.parabola = (n == 3 && lk == END_NOT_A_KNOT && rk == END_NOT_A_KNOT) ? 1 : 0;
    hipLaunchKernelGGL(lane_axes_spline_kernel<T>, dim3(build_lane_grid(lanes)), dim3(64), 0, (hipStream_t) nullptr, A);
    NDI_HIP(hipGetLastError());
    NDI_HIP(hipStreamSynchronize(nullptr));
  }

  // Pchip, Akima, CubicHermite: hermite_build_kernel on one lane per thread, the knots read per lane.
  void build_hermite(const void* dydx, int memspace) {
    Range rg("ndi:lane_axes_hermite_build");
    HermiteArgs<T> A{};
    A.data = y.as<T>();
    A.x = x.as<T>();
    A.ca = a.as<T>();
    A.cb = b.as<T>();
    A.n = n;
    A.lanes = lanes;
    A.kout = nullptr;
    DevBuf tmp;
    if (rule == HR_GIVEN) {
      if (memspace == NDI_MEM_DEVICE) {
        A.dydx = static_cast<const T*>(dydx);
      } else {
        tmp.reserve((size_t)n * lanes * sizeof(T));
        NDI_HIP(hipMemcpy(tmp.p, dydx, (size_t)n * lanes * sizeof(T), hipMemcpyHostToDevice));
        A.dydx = tmp.as<T>();
      }
    }
    const uint64_t total = (n - 1) * lanes;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
    pick<HR_PCHIP, HR_AKIMA, HR_GIVEN>(rule, [&](auto rule_) {
      hipLaunchKernelGGL((hermite_build_kernel<T, rule_, 1, true>), dim3(grid), dim3(BLOCK), 0, (hipStream_t) nullptr, A);
    });
    NDI_HIP(hipGetLastError());
    NDI_HIP(hipStreamSynchronize(nullptr));
  }

  // The record copy, on the NULL stream like the builds before it; complete on return.  Never fatal.
  void build_records() {
    const size_t bytes = (size_t)n * lanes * 4 * sizeof(T);
    if (!cubic() || bytes > REC_LIMIT) return;
    try {
      rec.reserve(bytes);
      const uint64_t total = n * lanes;
      const unsigned gr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 65536));
      hipLaunchKernelGGL(lane_axes_records_kernel<T>, dim3(gr), dim3(BLOCK), 0, (hipStream_t) nullptr, (const T*)x.as<T>(),
                         (const T*)y.as<T>(), (const T*)a.as<T>(), (const T*)b.as<T>(), static_cast<LanewiseRecord<T, 4>*>(rec.p),
                         n, lanes);
      NDI_HIP(hipGetLastError());
      NDI_HIP(hipStreamSynchronize(nullptr));
    } catch (const HipFailure&) {
      (void)hipGetLastError();
      rec.release();
    }
  }

  // ---- evaluation --------------------------------------------------------------------------------------------------------
  // One launch of the evaluation kernel.  laneq: a query per lane (q is [rows][q_stride], first_fail a flat element
  // index); otherwise q is [rows] and first_fail a query index.
  void launch(hipStream_t s, StatusBlock* st, bool laneq, const T* q, uint64_t q_stride, uint64_t rows, T* out,
              uint64_t out_stride, bool check) {
    const uint64_t total = rows * lanes;
    const unsigned grid = lanewise_grid(total, (uint64_t)cu_count() * lanewise_knobs().wgs);
    LaneAxesArgs<T> A{};
    A.x = x.as<T>(); A.y = y.as<T>(); A.a = a.as<T>(); A.b = b.as<T>();
    A.rec = lane_axes_use_records() ? rec.p : nullptr;
    A.q = q;
    A.out = out;
    A.lo = lane_dev.as<T>();
    A.hi = lane_dev.as<T>() + lanes;
    A.Lo = Lo; A.Hi = Hi;
    A.G = lanewise_geom(rows, lanes, q_stride, out_stride, grid);
    A.n = n;
    A.mode = mode;
    A.check = check ? 1 : 0;
    A.first_fail = &st->first_fail[0];
    if (trace_plan())
      std::fprintf(stderr, "[ndi plan] lane-axes eval cubic=%d laneq=%d records=%d check=%d grid=%u\n", (int)cubic(), (int)laneq,
                   (int)(A.rec != nullptr), A.check, grid);
    pick_bool(laneq, [&](auto laneq_) {
      if (!cubic()) {
        launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, lane_axes_eval_kernel<T, ST_LINEAR, laneq_, false>, A);
      } else {
        pick_bool(A.rec != nullptr, [&](auto rec_) {
          launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, lane_axes_eval_kernel<T, ST_CUBIC, laneq_, rec_>, A);
        });
      }
    });
  }

  // One batch of ndi_interp1d_eval on device pointers: status reset, the range pre-pass on [Lo, Hi] (or the kernel's own
  // test: NDI_EVAL_FRESH_OUTPUT), ONE evaluation launch.
  void enqueue(hipStream_t s, Workspace& ws, Queries<T> qs, uint64_t nq, T* out, uint64_t out_stride, int, int flags) {
    ws.sc[0].status.reserve(sizeof(StatusBlock));
    reset_status(ws.sc[0].status.p, s);
    const bool check = this->range_prepass(s, ws.sc[0], {qs.a, nullptr}, nq, (flags & NDI_EVAL_FRESH_OUTPUT) != 0);
    launch(s, ws.sc[0].status.as<StatusBlock>(), false, qs.a, 0, nq, out, out_stride, check);
  }

  // ---- what the host engine (float_host.hpp) takes from this family: no small-row paths, no ring -----------------------
  static constexpr int query_arrays = 1;
  static constexpr bool small_rows = false, ring = false;
  static const char* axis_name(int) { return "x"; }
  void range_limits(T lim[4]) const { lim[0] = lim[2] = Lo; lim[1] = lim[3] = Hi; }

  ndi_status eval(const void* q_, uint64_t nq, void* out_, uint64_t out_stride, const ndi_eval_opts* opts,
                  ndi_oob_info* info) override {
    ndi_eval_opts o{};
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED: a lane-axes handle (%s) evaluates in one form only (a search over "
                  "its own knots per lane: there is no common interval to group queries by)", name());
    if (out_stride < lanes)
      return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)out_stride, (unsigned long long)lanes);
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    if (nq == 0) return NDI_OK;
    if (!q_ || !out_) return fail(NDI_BAD_ARG, "null query / output pointer");
    DeviceGuard dg(device);
    Range rg("ndi_interp1d_eval");
    hipStream_t s = (hipStream_t)o.stream;
    SpaceLease lease(spaces, s);
    Workspace& ws = lease.ws;
    const Queries<T> orig{(const T*)q_, nullptr};
    return this->eval_body(s, ws, this->stage_queries(s, ws, orig, nq, o.q_memspace), orig, o.q_memspace, nq, out_,
                           out_stride, o, info);
  }

  ndi_status finish(void* stream, ndi_oob_info* info) override { return this->run_finish(stream, info); }

  // the lane-wise call: each element against its own lane's range (or, extrapolating, against NaN alone)
  void lanewise_enqueue(hipStream_t s, Workspace& ws, const T* q, uint64_t q_stride, uint64_t rows, T* out,
                        uint64_t out_stride, bool check) {
    g_last_path.store(NDI_PATH_GATHER);
    ws.sc[0].status.reserve(sizeof(StatusBlock));
    reset_status(ws.sc[0].status.p, s);
    StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
    if (!check) {
      const LanewiseGeom G = lanewise_geom(rows, lanes, q_stride, out_stride, 1);
      if (mode == EX_NO) lanewise_prepass<T>(s, q, G, T(0), T(0), (int)EX_NO, lane_dev.as<T>(), lane_dev.as<T>() + lanes, &st->first_fail[0]);
      else lanewise_prepass<T>(s, q, G, T(0), T(0), (int)EX_YES, (const T*)nullptr, (const T*)nullptr, &st->first_fail[0]);
    }
    launch(s, st, true, q, q_stride, rows, out, out_stride, check);
  }
  ndi_status eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                           const ndi_eval_opts* opts, ndi_oob_info* info) override {
    if (opts && opts->path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "eval_lanewise: NDI_PATH_BUCKETED: a lane-axes handle (%s) evaluates in one form only "
                  "(there is no common interval to group queries by)", name());
    const std::string what = std::string(name()) + " with an x axis per lane";
    return lanewise_run<T>(*this, what.c_str(), q, nq, q_stride, out, out_stride, opts, info);
  }

  ndi_status eval_ring(const void*, uint64_t, const ndi_ring_desc*, ndi_ring_consumer, void*, const ndi_eval_opts*,
                       ndi_oob_info*) override {
    return fail(NDI_UNSUPPORTED, "eval_ring: a lane-axes handle (%s) has no ring evaluation; ndi_interp1d_eval chunk by "
                "chunk serves it", name());
  }

  ndi_status trim() override {
    DeviceGuard dg(device);
    this->trim_front();
    return NDI_OK;
  }
  uint64_t scratch_sets() override { return spaces.size(); }

  ndi_status coefficients(void* a_out, void* b_out, int memspace) override {
    DeviceGuard dg(device);
    if (!cubic()) return fail(NDI_BAD_ARG, "Linear has no coefficient tables");
    const size_t tab = (size_t)(n - 1) * lanes * sizeof(T);
    const hipMemcpyKind k = memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (a_out) NDI_HIP(hipMemcpy(a_out, a.p, tab, k));
    if (b_out) NDI_HIP(hipMemcpy(b_out, b.p, tab, k));
    return NDI_OK;
  }
  ndi_status derivative(int, Interp1DBase**) override {
    return fail(NDI_UNSUPPORTED, "derivative: a lane-axes handle (%s) has no derivative handle: the derivative rule reads one "
                "knot spacing per interval, and here every lane has its own", name());
  }
  ndi_status antiderivative(Interp1DBase**) override {
    return fail(NDI_UNSUPPORTED, "antiderivative: a lane-axes handle (%s) has no antiderivative handle: the prefix build reads "
                "one knot spacing per interval, and here every lane has its own", name());
  }
  ndi_status inverse(Interp1DBase**) override {
    return fail(NDI_UNSUPPORTED, "inverse: a lane-axes handle (%s) has no inverse handle: an inverse maps values back to one "
                "shared axis, and here every lane has its own", name());
  }

  ndi_status data_table(void* data_out, int memspace) override {
    DeviceGuard dg(device);
    NDI_HIP(hipMemcpy(data_out, y.p, (size_t)n * lanes * sizeof(T),
                      memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return NDI_OK;
  }

  ndi_status clone_to(int dev, Interp1DBase** out) override {
    std::unique_ptr<LaneAxesImpl<T>> h(new LaneAxesImpl<T>());
    h->dtype = dtype; h->device = dev; h->lanes = lanes; h->lane_axes_handle = true;
    h->strategy = strategy; h->rule = rule; h->mode = mode; h->n = n;
    h->Lo = Lo; h->Hi = Hi;
    h->lane_limits = lane_limits;
    {
      DeviceGuard dg(device);
      NDI_HIP(hipDeviceSynchronize());     // the source tables are complete
    }
    DeviceGuard dg(dev);
    h->reserve_tables();
    h->upload_lane_limits();
    const size_t data_b = (size_t)n * lanes * sizeof(T), tab_b = (size_t)(n - 1) * lanes * sizeof(T);
    copy_across_devices(h->x.p, dev, x.p, device, data_b);
    copy_across_devices(h->y.p, dev, y.p, device, data_b);
    if (cubic()) {
      copy_across_devices(h->a.p, dev, a.p, device, tab_b);
      copy_across_devices(h->b.p, dev, b.p, device, tab_b);
    }
    h->build_records();
    *out = h.release();
    return NDI_OK;
  }
};

// ndi_interp1d_create_lane_axes behind its argument checks (and, for host arrays, behind the column validation).
template <class T>
static ndi_status create_lane_axes(const ndi_interp1d_desc& d, const void* x_lanes, const void* dydx, Interp1DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp1d_create_lane_axes");
  std::unique_ptr<LaneAxesImpl<T>> h(new LaneAxesImpl<T>());
  h->dtype = d.dtype; h->device = d.device; h->lanes = d.lanes; h->lane_axes_handle = true;
  const bool cubic = d.strategy != NDI_LINEAR;
  h->strategy = cubic ? NDI_CUBIC_SPLINE : NDI_LINEAR;
  h->rule = d.strategy == NDI_PCHIP ? HR_PCHIP : d.strategy == NDI_AKIMA ? HR_AKIMA : d.strategy == NDI_CUBIC_HERMITE ? HR_GIVEN : HR_SPLINE;
  h->mode = d.extrapolate ? EX_YES : EX_NO;
  h->n = d.n;
  h->reserve_tables();
  const size_t bytes = (size_t)d.n * d.lanes * sizeof(T);
  const hipMemcpyKind kind = d.memspace == NDI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  NDI_HIP(hipMemcpy(h->x.p, x_lanes, bytes, kind));
  NDI_HIP(hipMemcpy(h->y.p, d.data, bytes, kind));
  if (d.memspace == NDI_MEM_DEVICE)
    if (const ndi_status st = h->check_columns(); st != NDI_OK) return st;
  h->take_ranges();
  if (d.strategy == NDI_CUBIC_SPLINE) h->build_spline(d);
  else if (cubic) h->build_hermite(dydx, d.memspace);
  h->build_records();
  *out = h.release();
  return NDI_OK;
}
