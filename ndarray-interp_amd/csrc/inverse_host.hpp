// csrc/inverse_host.hpp -- the host side of inverse handles (ndi_interp1d_inverse); included by ndinterp_api.hip inside
// namespace ndi, behind Interp1DImpl and AntiderivImpl.
//
// An inverse handle is an Interp1DBase of its own, like an antiderivative handle, and follows its convention: it owns
// copies of everything it reads (the knots, the node table N, and the tables the interval polynomial needs), so the
// source is only read and either handle may be destroyed first.  Creation runs ONE device pass over N
// (inverse_check_kernel: is every lane monotone?) and brings back the per-lane flag words and the first and last rows
// of N, from which the host keeps the value range common to all lanes, [Lo, Hi].  Evaluation is the range pre-pass of
// the other handles with Lo / Hi in place of the end knots, then ONE launch of inverse_eval_kernel
// (inverse_kernels.hpp).  Staging, the first-error report, the host-output chunk loop and finish are the float host
// engine's (float_host.hpp).

template <class T>
struct InverseImpl final : Interp1DBase, FloatEngine<T, InverseImpl<T>> {
  int cls = IC_LINEAR;     // InverseClass
  int rule = HR_SPLINE;    // the source's rule and derivative order (names in messages, the replica signature)
  int deriv = 0;
  int mode = EX_NO;        // the inverse is defined on the node range only, whatever the source extrapolates
  uint64_t n = 0;
  DevicePyramid<T> pyr;    // (the knots; their host copy)
  DevBuf y, a, b, P;       // y: the source's data; a, b: the cubic class; P: antiderivative sources.  N is P or y.
  T Lo = T(0), Hi = T(0);  // the value range common to all lanes
  std::vector<T> lane_limits;   // [2][lanes]: lane l's own range, min and max of N[0][l] and N[n-1][l] (the lane-wise evaluation)
  DevBuf lane_dev;              // ... and its device copy, uploaded with the other tables at creation / clone
  void upload_lane_limits() {
    lane_dev.reserve((size_t)2 * lanes * sizeof(T));
    NDI_HIP(hipMemcpy(lane_dev.p, lane_limits.data(), (size_t)2 * lanes * sizeof(T), hipMemcpyHostToDevice));
  }
  SpaceSet spaces;

  bool anti() const { return cls == IC_ANTI_CUBIC || cls == IC_ANTI_LINEAR; }
  bool cubic() const { return cls == IC_CUBIC || cls == IC_ANTI_CUBIC; }
  const T* node_table() const { return anti() ? P.as<T>() : y.as<T>(); }
  std::string source_name() const {
    const char* base = cubic() ? hermite_rule_name(rule) : "Linear";
    return anti() ? std::string("the antiderivative of ") + base : std::string(base);
  }

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, pyr.host_knots.data(), pyr.host_knots.size() * sizeof(T));
    const uint64_t f[3] = {n, (uint64_t)cls | ((uint64_t)rule << 8) | ((uint64_t)deriv << 16) | (1ull << 25) /* Inverse */,
                           (uint64_t)mode};
    return fnv1a(h, f, sizeof(f));
  }

  void reserve_tables(const T* knots) {
    pyr.upload(knots, n);
    y.reserve((size_t)n * lanes * sizeof(T));
    if (anti()) P.reserve((size_t)n * lanes * sizeof(T));
    if (cubic()) {
      a.reserve((size_t)(n - 1) * lanes * sizeof(T));
      b.reserve((size_t)(n - 1) * lanes * sizeof(T));
    }
  }

  // ---- creation: the monotonicity pass and the common range (NULL stream, complete on return) ---------------------------
  ndi_status check_and_range() {
    Range rg("ndi:inverse_check");
    const hipStream_t s0 = nullptr;
    DevBuf flags;
    flags.reserve((size_t)lanes * sizeof(unsigned int));
    NDI_HIP(hipMemsetAsync(flags.p, 0, (size_t)lanes * sizeof(unsigned int), s0));
    const uint64_t total = ((n + INV_CHECK_RUN - 1) / INV_CHECK_RUN) * lanes;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
    hipLaunchKernelGGL(inverse_check_kernel<T>, dim3(grid), dim3(BLOCK), 0, s0, node_table(), n, lanes, flags.as<unsigned int>());
    NDI_HIP(hipGetLastError());
    std::vector<unsigned int> hf(lanes);
    std::vector<T> ends((size_t)2 * lanes);
    NDI_HIP(hipMemcpy(hf.data(), flags.p, (size_t)lanes * sizeof(unsigned int), hipMemcpyDeviceToHost));
    NDI_HIP(hipMemcpy(ends.data(), node_table(), (size_t)lanes * sizeof(T), hipMemcpyDeviceToHost));
    NDI_HIP(hipMemcpy(ends.data() + lanes, node_table() + (size_t)(n - 1) * lanes, (size_t)lanes * sizeof(T), hipMemcpyDeviceToHost));
    for (uint64_t l = 0; l < lanes; ++l) {
      const bool nan = (hf[l] & 4u) != 0, both = (hf[l] & 3u) == 3u;
      if (nan || both)
        return fail(NDI_MONOTONIC, "inverse of %s: lane %llu of the node table %s; every lane must be monotone "
                    "(ties allowed) to be inverted", source_name().c_str(), (unsigned long long)l,
                    nan ? "holds a NaN" : "both rises and falls");
    }
    lane_limits.resize((size_t)2 * lanes);
    for (uint64_t l = 0; l < lanes; ++l) {
      lane_limits[l] = std::min(ends[l], ends[lanes + l]);
      lane_limits[lanes + l] = std::max(ends[l], ends[lanes + l]);
    }
    upload_lane_limits();
    Lo = std::min(ends[0], ends[lanes]);
    Hi = std::max(ends[0], ends[lanes]);
    for (uint64_t l = 1; l < lanes; ++l) {
      Lo = std::max(Lo, std::min(ends[l], ends[lanes + l]));
      Hi = std::min(Hi, std::max(ends[l], ends[lanes + l]));
    }
    return NDI_OK;
  }

  // ---- evaluation ------------------------------------------------------------------------------------------------------
  // One batch on device pointers: status reset, the range pre-pass on [Lo, Hi], ONE evaluation launch.
  // (path and flags: the engine's; this family has one form and always its range test)
  void enqueue(hipStream_t s, Workspace& ws, Queries<T> qs, uint64_t nq, T* out, uint64_t out_stride, int, int) {
    ws.sc[0].status.reserve(sizeof(StatusBlock));
    reset_status(ws.sc[0].status.p, s);
    StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
    this->range_prepass(s, ws.sc[0], {qs.a, nullptr}, nq, false);   // (mode is EX_NO: the node range only)
    InverseEvalArgs<T> A{};
    A.knots = pyr.view.lv0;
    A.N = node_table();
    A.y = y.as<T>(); A.a = a.as<T>(); A.b = b.as<T>();
    A.q = qs.a;
    A.out = out;
    A.n = n; A.lanes = lanes; A.out_stride = out_stride; A.nq = nq;
    A.status = st;
    const uint64_t total = nq * lanes;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
    if (trace_plan()) std::fprintf(stderr, "[ndi plan] inverse eval class=%d grid=%u\n", cls, grid);
    switch (cls) {
      case IC_LINEAR: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_eval_kernel<T, IC_LINEAR>, A); break;
      case IC_CUBIC: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_eval_kernel<T, IC_CUBIC>, A); break;
      case IC_ANTI_CUBIC: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_eval_kernel<T, IC_ANTI_CUBIC>, A); break;
      default: launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), 0, inverse_eval_kernel<T, IC_ANTI_LINEAR>, A); break;
    }
  }

  // ---- what the host engine (float_host.hpp) takes from this family: no small-row paths, no ring -----------------------
  static constexpr bool small_rows = false, ring = false;
  static const char* axis_name(int) { return "v"; }
  void range_limits(T lim[4]) const { lim[0] = lim[2] = Lo; lim[1] = lim[3] = Hi; }
  // a value outside [Lo, Hi] is a range failure, a NaN its own status -- whatever the source's extrapolation mode was
  ndi_status failure_status(T v) { return v == v ? NDI_OUT_OF_BOUNDS : NDI_NAN_QUERY; }

  ndi_status eval(const void* q_, uint64_t nq, void* out_, uint64_t out_stride, const ndi_eval_opts* opts,
                  ndi_oob_info* info) override {
    ndi_eval_opts o{};
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED: an inverse handle (of %s) evaluates in one form only (a search over "
                  "node values per lane: there is no interval to group queries by)", source_name().c_str());
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

  // lane-wise evaluation (defined in lanewise_host.hpp): values per lane, tested against the lane's own range
  void lanewise_enqueue(hipStream_t s, Workspace& ws, const T* q, uint64_t q_stride, uint64_t rows, T* out,
                        uint64_t out_stride, bool check);
  ndi_status eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                           const ndi_eval_opts* opts, ndi_oob_info* info) override;

  ndi_status eval_ring(const void*, uint64_t, const ndi_ring_desc*, ndi_ring_consumer, void*, const ndi_eval_opts*,
                       ndi_oob_info*) override {
    return fail(NDI_UNSUPPORTED, "eval_ring: an inverse handle (of %s) has no ring evaluation; ndi_interp1d_eval chunk by "
                "chunk serves it", source_name().c_str());
  }

  ndi_status trim() override {
    DeviceGuard dg(device);
    this->trim_front();
    return NDI_OK;
  }
  uint64_t scratch_sets() override { return spaces.size(); }

  ndi_status coefficients(void*, void*, int) override {
    return fail(NDI_BAD_ARG, "coefficients: the inverse of %s is no piecewise polynomial: it has no a / b tables "
                "(ndi_interp1d_data hands back its node table)", source_name().c_str());
  }
  ndi_status derivative(int, Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "derivative: the inverse of %s is no piecewise polynomial, which the derivative rule for "
                "{y, a, b} tables does not take (1 / f' at the returned x is its derivative)", source_name().c_str());
  }
  ndi_status antiderivative(Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "antiderivative: the inverse of %s is no piecewise polynomial: it has no prefix table",
                source_name().c_str());
  }
  ndi_status integrate(const void*, const void*, uint64_t, void*, uint64_t, const ndi_eval_opts*, ndi_oob_info*) override {
    return fail(NDI_BAD_ARG, "integrate: the inverse of %s is no antiderivative handle (integrate takes "
                "ndi_interp1d_antiderivative of a handle)", source_name().c_str());
  }
  ndi_status inverse(Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "inverse: this handle is already the inverse of %s; its inverse is the handle it was made from",
                source_name().c_str());
  }

  ndi_status data_table(void* data_out, int memspace) override {
    DeviceGuard dg(device);
    NDI_HIP(hipMemcpy(data_out, node_table(), (size_t)n * lanes * sizeof(T),
                      memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return NDI_OK;
  }

  std::unique_ptr<InverseImpl<T>> shell(int dev) const {
    std::unique_ptr<InverseImpl<T>> h(new InverseImpl<T>());
    h->dtype = dtype; h->device = dev; h->lanes = lanes; h->inverse_handle = true;
    h->cls = cls; h->rule = rule; h->deriv = deriv; h->n = n;
    h->Lo = Lo; h->Hi = Hi;
    h->lane_limits = lane_limits;
    return h;
  }

  ndi_status clone_to(int dev, Interp1DBase** out) override {
    std::unique_ptr<InverseImpl<T>> h = shell(dev);
    {
      DeviceGuard dg(device);
      NDI_HIP(hipDeviceSynchronize());     // the source tables are complete
    }
    DeviceGuard dg(dev);
    h->reserve_tables(pyr.host_knots.data());
    h->upload_lane_limits();
    const size_t data_b = (size_t)n * lanes * sizeof(T), tab_b = (size_t)(n - 1) * lanes * sizeof(T);
    copy_across_devices(h->y.p, dev, y.p, device, data_b);
    if (anti()) copy_across_devices(h->P.p, dev, P.p, device, data_b);
    if (cubic()) {
      copy_across_devices(h->a.p, dev, a.p, device, tab_b);
      copy_across_devices(h->b.p, dev, b.p, device, tab_b);
    }
    *out = h.release();
    return NDI_OK;
  }
};

// ndi_interp1d_inverse of an f32 / f64 handle, behind the source's own refusals: a new handle on the source's device with
// its own copies of the tables (device pointers y, a, b, P of the source; a, b null for Linear, P null unless the source is
// an antiderivative handle), checked and ranged there.
template <class T>
static ndi_status inverse_create(const Interp1DBase& src, int cls, int rule, int deriv, uint64_t n, const T* knots,
                                 const void* y, const void* a, const void* b, const void* P, Interp1DBase** out) {
  DeviceGuard dg(src.device);
  std::unique_ptr<InverseImpl<T>> h(new InverseImpl<T>());
  h->dtype = src.dtype; h->device = src.device; h->lanes = src.lanes; h->inverse_handle = true;
  h->cls = cls; h->rule = rule; h->deriv = deriv; h->n = n;
  h->reserve_tables(knots);
  const size_t data_b = (size_t)n * src.lanes * sizeof(T), tab_b = (size_t)(n - 1) * src.lanes * sizeof(T);
  NDI_HIP(hipMemcpyAsync(h->y.p, y, data_b, hipMemcpyDeviceToDevice, nullptr));
  if (h->anti()) NDI_HIP(hipMemcpyAsync(h->P.p, P, data_b, hipMemcpyDeviceToDevice, nullptr));
  if (h->cubic()) {
    NDI_HIP(hipMemcpyAsync(h->a.p, a, tab_b, hipMemcpyDeviceToDevice, nullptr));
    NDI_HIP(hipMemcpyAsync(h->b.p, b, tab_b, hipMemcpyDeviceToDevice, nullptr));
  }
  if (const ndi_status st = h->check_and_range(); st != NDI_OK) return st;
  *out = h.release();
  return NDI_OK;
}

template <class T>
ndi_status Interp1DImpl<T>::inverse(Interp1DBase** out) {
  const bool lin = strategy != NDI_CUBIC_SPLINE;
  const char* name = lin ? "Linear" : hermite_rule_name(rule);
  if (mode == EX_PERIODIC)
    return fail(NDI_BAD_ARG, "inverse of %s: the Periodic extrapolation mode has no inverse handle (a periodic function "
                "takes every value in infinitely many places)", name);
  return inverse_create<T>(*this, lin ? IC_LINEAR : IC_CUBIC, rule, deriv, n, pyr.host_knots.data(), data.p, ca.p, cb.p,
                           nullptr, out);
}

template <class T>
ndi_status AntiderivImpl<T>::inverse(Interp1DBase** out) {
  if (mode == EX_PERIODIC)
    return fail(NDI_BAD_ARG, "inverse of the antiderivative of %s: the Periodic extrapolation mode has no inverse handle",
                source_name());
  return inverse_create<T>(*this, linear ? IC_ANTI_LINEAR : IC_ANTI_CUBIC, rule, deriv, n, pyr.host_knots.data(), y.p, a.p,
                           b.p, P.p, out);
}
