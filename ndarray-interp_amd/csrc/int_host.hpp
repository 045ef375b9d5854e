// csrc/int_host.hpp -- host side of the i32 / i64 Linear and Bilinear handles (included by ndinterp_api.hip inside
// namespace ndi, after the float handles; kernels in int_kernels.hpp).
//
// IntEngine is the NarrowEngine (narrow_host.hpp: staging, first_fail, eval_rows, the ring, trim, the sharded call) of
// the integer handles.  Its own part:
//   run          ndi_interp{1,2}d_eval: caller-owned buffers take first_fail + eval_rows over [0, F); fresh /
//                unspecified-rows outputs take the fused pass
//   diagnose     the failing query alone, on the host, in the reference's order (generic_host.calc_frac): which
//                range test or which operation of which lane failed first
// The staging buffers are the handle's (one scratch set, calls serialised by the engine's mutex).  async_launch is
// accepted and completes inside the call; ndi_interp{1,2}d_finish then reports that batch's status.

// Linear::calc_frac (linear.rs:29-36) in T, in the reference's order: the ndi_int_op of the first overflowing operation,
// or -1 (result in res).
template <class T>
static int int_calc_frac_host(T x1, T y1, T x2, T y2, T x, T& res) {
  T dy, dx, d, p;
  if (__builtin_sub_overflow(y2, y1, &dy)) return NDI_OP_SUBTRACT;
  if (__builtin_sub_overflow(x2, x1, &dx)) return NDI_OP_SUBTRACT;
  if (dx == 0 || (dx == (T)-1 && dy == std::numeric_limits<T>::min())) return NDI_OP_DIVIDE;
  const T m = dy / dx;
  if (__builtin_sub_overflow(x, x1, &d)) return NDI_OP_SUBTRACT;
  if (__builtin_mul_overflow(m, d, &p)) return NDI_OP_MULTIPLY;
  if (__builtin_add_overflow(p, y1, &res)) return NDI_OP_ADD;
  return -1;
}

template <class T>
static uint64_t int_lower_index_host(const std::vector<T>& k, T x) {
  const uint64_t n = k.size();
  if (x <= k[0]) return 0;
  if (x >= k[n - 1]) return n - 2;
  uint64_t lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (k[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

static unsigned int_grid(uint64_t items) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + BLOCK - 1) / BLOCK, (uint64_t)cu_count() * 16));
}

// AUTO rule of the integer kernels: one output element per thread for rows of up to 32 elements (scalar
// data: a query per lane), one query per wavefront beyond (the search is done once per query and the row is streamed
// by the wave).  NDI_INT_MAP = 1 / 2 forces the element / wave mapping (tests).
static bool int_wave_mapping(uint64_t lanes) {
  static const Knob map{"NDI_INT_MAP", 0};
  if (map.get() == 1) return false;
  if (map.get() == 2) return true;
  return lanes > 32;
}

static const char* const INT_OP_NAMES[4] = {"subtract", "multiply", "add", "divide"};   // indexed by ndi_int_op

template <class T>
struct IntEngine : NarrowEngine<T> {
  NarrowScratch scratch;   // one set per handle
  std::map<void*, std::pair<ndi_status, ndi_oob_info>> pending;   // async_launch batches awaiting finish, per stream
  std::string pending_err;

  virtual void launch_eval(const T* qx, const T* qy, uint64_t nq, T* out, uint64_t stride, hipStream_t s,
                           bool check, unsigned long long* w) = 0;
  virtual ndi_status diagnose_at(T x, T y, ndi_oob_info* info) = 0;

  NarrowScratch& ws(hipStream_t) override { return scratch; }
  void release_scratch() override { scratch.release(); }
  const char* bucketed_refusal() const override {
    return "NDI_PATH_BUCKETED is not available for integer element types (AUTO / GATHER)";
  }
  void launch_rows(const T* dx, const T* dy, uint64_t cnt, T* out, uint64_t stride, hipStream_t s) override {
    launch_eval(dx, dy, cnt, out, stride, s, false, nullptr);
  }
  // serial, on the calling thread, in shard order; a HIP failure unwinds to the entry point
  ndi_status each_shard(uint32_t ns, const std::function<void(uint32_t)>& fn) override {
    for (uint32_t i = 0; i < ns; ++i) fn(i);
    return NDI_OK;
  }

  // The failing query j alone: its x (and y) fetched, the reference's checks replayed in order.
  ndi_status diagnose(const void* qx, const void* qy, uint64_t j, int qmem, uint64_t index,
                      ndi_oob_info* info) override {
    T x = 0, y = 0;
    this->fetch_query(qx, qy, j, qmem, &x, &y);
    ndi_oob_info tmp{};
    if (!info) info = &tmp;
    ndi_status st = diagnose_at(x, y, info);
    info->index = index;
    return st;
  }
  ndi_status overflow(int op, ndi_oob_info* info) {
    info->axis = op;
    info->status = NDI_INT_OVERFLOW;
    return fail(NDI_INT_OVERFLOW, "attempt to %s with overflow", INT_OP_NAMES[op]);
  }

  ndi_status run(const void* qx, const void* qy, uint64_t nq, void* out, uint64_t stride, const ndi_eval_opts* opts,
                 ndi_oob_info* info) {
    ndi_eval_opts o{};
    if (const ndi_status hs = this->run_head(opts, o, qx, out, nq, stride, info); hs != NDI_OK) return hs;
    DeviceGuard dg(this->dev);
    std::lock_guard<std::mutex> lk(this->mu);
    hipStream_t s = (hipStream_t)o.stream;
    ndi_status st = NDI_OK;
    if (nq) {
      NarrowScratch& W = scratch;
      const uint64_t elanes = this->elanes;
      const T* dx = this->stage(qx, nq, o.q_memspace, W.qx, s);
      const T* dy = this->stage(qy, nq, o.q_memspace, W.qy, s);
      uint64_t F;
      if (o.flags & NDI_EVAL_FRESH_OUTPUT) {   // fused: rows at / after the failure may be written
        const bool dev_out = o.out_memspace == NDI_MEM_DEVICE;
        if (!dev_out) W.out.reserve(nq * elanes * sizeof(T));
        unsigned long long* w = this->reset_word(W, s);
        launch_eval(dx, dy, nq, dev_out ? static_cast<T*>(out) : W.out.as<T>(), dev_out ? stride : elanes, s,
                    true, w);
        NDI_HIP(hipGetLastError());
        F = this->read_word(W, s);
        if (!dev_out) this->rows_to_host(out, stride, W.out, std::min<uint64_t>(F, nq), s);
      } else {   // caller-owned rows: the check pass, the host reads F, then rows [0, F)
        F = this->first_fail(dx, dy, nq, W, s);
        this->eval_rows(dx, dy, std::min<uint64_t>(F, nq), out, stride, o.out_memspace, W, s);
      }
      NDI_HIP(hipStreamSynchronize(s));
      if (F < nq) st = diagnose(qx, qy, F, o.q_memspace, F, info);
    }
    if (o.async_launch) {
      ndi_oob_info rec = info ? *info : ndi_oob_info{0, 0.0, 0, st};
      pending[o.stream] = {st, rec};
      pending_err = st == NDI_OK ? std::string() : tls_error();
      return NDI_OK;
    }
    return st;
  }

  ndi_status finish_impl(void* stream, ndi_oob_info* info) {
    std::lock_guard<std::mutex> lk(this->mu);
    auto it = pending.find(stream);
    if (it == pending.end()) return NDI_OK;
    const ndi_status st = it->second.first;
    if (info) *info = it->second.second;
    pending.erase(it);
    if (st != NDI_OK) tls_error() = pending_err;
    return st;
  }
};

// ---- 1-D --------------------------------------------------------------------------------------------------------
template <class T>
struct Interp1DIntImpl final : Interp1DBase, IntEngine<T> {
  uint64_t n = 0;
  std::vector<T> hx;
  DevBuf knots, rec, iv;

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, &dtype, sizeof(dtype));
    h = fnv1a(h, &this->emode, sizeof(int));
    h = fnv1a(h, &n, sizeof(n));
    h = fnv1a(h, &lanes, sizeof(lanes));
    return fnv1a(h, hx.data(), hx.size() * sizeof(T));
  }
  void launch_check(const T* qx, const T*, uint64_t nq, hipStream_t s, unsigned long long* w) override {
    hipLaunchKernelGGL(int_check1d_kernel<T>, dim3(int_grid(nq)), dim3(BLOCK), 0, s, qx, nq, knots.as<T>(),
                       (uint32_t)n, this->emode, iv.as<IntIv>(), w);
  }
  void launch_eval(const T* qx, const T*, uint64_t nq, T* out, uint64_t stride, hipStream_t s, bool check,
                   unsigned long long* w) override {
    const IntRec<T>* r = rec.as<IntRec<T>>();
    if (int_wave_mapping(lanes)) {
      const unsigned g = int_grid(nq * 64);
      if (check)
        hipLaunchKernelGGL((int_eval1d_kernel<T, true, true>), dim3(g), dim3(BLOCK), 0, s, qx, nq, knots.as<T>(),
                           (uint32_t)n, this->emode, iv.as<IntIv>(), r, lanes, out, stride, w);
      else
        hipLaunchKernelGGL((int_eval1d_kernel<T, true, false>), dim3(g), dim3(BLOCK), 0, s, qx, nq, knots.as<T>(),
                           (uint32_t)n, this->emode, iv.as<IntIv>(), r, lanes, out, stride, w);
    } else {
      const unsigned g = int_grid(nq * lanes);
      if (check)
        hipLaunchKernelGGL((int_eval1d_kernel<T, false, true>), dim3(g), dim3(BLOCK), 0, s, qx, nq, knots.as<T>(),
                           (uint32_t)n, this->emode, iv.as<IntIv>(), r, lanes, out, stride, w);
      else
        hipLaunchKernelGGL((int_eval1d_kernel<T, false, false>), dim3(g), dim3(BLOCK), 0, s, qx, nq, knots.as<T>(),
                           (uint32_t)n, this->emode, iv.as<IntIv>(), r, lanes, out, stride, w);
    }
  }
  ndi_status diagnose_at(T x, T, ndi_oob_info* info) override {
    info->value = (double)x;
    if (this->emode == EX_NO && !(hx[0] <= x && x <= hx[n - 1])) {
      info->axis = 0;
      info->status = NDI_OUT_OF_BOUNDS;
      return fail(NDI_OUT_OF_BOUNDS, "x = %lld is not in range", (long long)x);
    }
    const uint64_t i = int_lower_index_host(hx, x);
    std::vector<IntRec<T>> r(2 * lanes);
    NDI_HIP(hipMemcpy(r.data(), rec.as<IntRec<T>>() + i * lanes, 2 * lanes * sizeof(IntRec<T>), hipMemcpyDeviceToHost));
    for (uint64_t l = 0; l < lanes; ++l) {
      T res;
      const int op = int_calc_frac_host<T>(hx[i], r[l].v, hx[i + 1], r[lanes + l].v, x, res);
      if (op >= 0) return this->overflow(op, info);
    }
    return fail(NDI_HIP_ERROR, "integer evaluation reported query %lld as failing, but it evaluates", (long long)x);
  }

  ndi_status eval(const void* q, uint64_t nq, void* out, uint64_t out_stride, const ndi_eval_opts* opts,
                  ndi_oob_info* info) override {
    return this->run(q, nullptr, nq, out, out_stride, opts, info);
  }
  ndi_status finish(void* stream, ndi_oob_info* info) override { return this->finish_impl(stream, info); }
  ndi_status coefficients(void*, void*, int) override {
    return fail(NDI_BAD_ARG, "coefficients: an integer handle is a Linear interpolator (no spline tables)");
  }
  ndi_status derivative(int, Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "derivative: an integer handle is a Linear interpolator: its slope jumps at the knots "
                "(derivative takes f32 / f64 CubicSpline, Pchip, Akima and CubicHermite handles)");
  }
  ndi_status antiderivative(Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "antiderivative: an integer handle is a Linear interpolator of a narrow element type: the prefix table would "
                "round at every knot (antiderivative takes f32 / f64 Linear, CubicSpline, Pchip, Akima and CubicHermite handles)");
  }
  ndi_status inverse(Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "inverse: an integer handle is a Linear interpolator of a narrow element type: the returned abscissae "
                "would round to it (inverse takes f32 / f64 Linear, CubicSpline, Pchip, Akima, CubicHermite, derivative and "
                "antiderivative handles)");
  }
  ndi_status data_table(void* data_out, int memspace) override {   // the values of the slope records {v, m}
    DeviceGuard dg(device);
    NDI_HIP(hipMemcpy2D(data_out, sizeof(T), rec.p, sizeof(IntRec<T>), sizeof(T), n * lanes,
                        memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return NDI_OK;
  }
  ndi_status eval_ring(const void* q, uint64_t nq, const ndi_ring_desc* ring, ndi_ring_consumer consume, void* user,
                       const ndi_eval_opts* opts, ndi_oob_info* info) override {
    return this->run_ring(q, nullptr, nq, ring, consume, user, opts, info);
  }
  ndi_status trim() override { return this->trim_impl(); }
  uint64_t scratch_sets() override { return this->scratch.out.p || this->scratch.qx.p ? 1 : 0; }

  // build from host knots and device-resident data
  void build(const T* data_dev) {
    const uint64_t nl = n * lanes;
    knots.reserve(n * sizeof(T));
    NDI_HIP(hipMemcpy(knots.p, hx.data(), n * sizeof(T), hipMemcpyHostToDevice));
    rec.reserve(nl * sizeof(IntRec<T>));
    std::vector<IntIv> init(n - 1, IntIv{(long long)std::numeric_limits<T>::min(),
                                         (long long)std::numeric_limits<T>::max()});
    iv.reserve((n - 1) * sizeof(IntIv));
    NDI_HIP(hipMemcpy(iv.p, init.data(), (n - 1) * sizeof(IntIv), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(int_slopes1d_kernel<T>, dim3(int_grid(nl)), dim3(BLOCK), 0, (hipStream_t) nullptr,
                       knots.as<T>(), data_dev, n, lanes, rec.as<IntRec<T>>(), iv.as<IntIv>());
    NDI_HIP(hipGetLastError());
    NDI_HIP(hipDeviceSynchronize());
  }

  ndi_status clone_to(int d, Interp1DBase** out) override {
    std::unique_ptr<Interp1DIntImpl<T>> c(new Interp1DIntImpl<T>());
    {
      DeviceGuard dg(d);
      set_scalars(*c, dtype, d, this->emode, lanes);
      c->n = n; c->hx = hx;
      c->knots.reserve(knots.bytes); c->rec.reserve(rec.bytes); c->iv.reserve(iv.bytes);
    }
    copy_across_devices(c->knots.p, d, knots.p, device, knots.bytes);
    copy_across_devices(c->rec.p, d, rec.p, device, rec.bytes);
    copy_across_devices(c->iv.p, d, iv.p, device, iv.bytes);
    *out = c.release();
    return NDI_OK;
  }
};

template <class T>
static ndi_status create1d_int(const ndi_interp1d_desc& d, Interp1DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp1d_create");
  std::unique_ptr<Interp1DIntImpl<T>> h(new Interp1DIntImpl<T>());
  set_scalars(*h, d.dtype, d.device, d.extrapolate ? EX_YES : EX_NO, d.lanes);
  h->n = d.n;
  h->hx = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.n);
  if (const ndi_status st = check_desc_1d(d, h->hx.data()); st != NDI_OK) return st;
  const size_t bytes = (size_t)d.n * d.lanes * sizeof(T);
  DevBuf tmp;
  const T* src = static_cast<const T*>(d.data);
  if (d.memspace != NDI_MEM_DEVICE) {
    tmp.reserve(bytes);
    NDI_HIP(hipMemcpy(tmp.p, d.data, bytes, hipMemcpyHostToDevice));
    src = tmp.as<T>();
  }
  h->build(src);
  *out = h.release();
  return NDI_OK;
}

// ---- 2-D --------------------------------------------------------------------------------------------------------
template <class T>
struct Interp2DIntImpl final : Interp2DBase, IntEngine<T> {
  uint64_t nx = 0, ny = 0;
  std::vector<T> hx, hy;
  DevBuf kx, ky, rec, pbad, yiv;

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, &dtype, sizeof(dtype));
    h = fnv1a(h, &this->emode, sizeof(int));
    h = fnv1a(h, &lanes, sizeof(lanes));
    h = fnv1a(h, hx.data(), hx.size() * sizeof(T));
    return fnv1a(h, hy.data(), hy.size() * sizeof(T));
  }
  template <bool WAVE, bool CHECK, bool WRITE>
  void go(unsigned g, const T* qx, const T* qy, uint64_t nq, T* out, uint64_t stride, hipStream_t s,
          unsigned long long* w) {
    hipLaunchKernelGGL((int_eval2d_kernel<T, WAVE, CHECK, WRITE>), dim3(g), dim3(BLOCK), 0, s, qx, qy, nq,
                       kx.as<T>(), (uint32_t)nx, ky.as<T>(), (uint32_t)ny, this->emode, pbad.as<uint8_t>(),
                       yiv.as<IntYIv<T>>(), rec.as<IntRec<T>>(), lanes, out, stride, w);
  }
  void launch_check(const T* qx, const T* qy, uint64_t nq, hipStream_t s, unsigned long long* w) override {
    if (int_wave_mapping(lanes)) go<true, true, false>(int_grid(nq * 64), qx, qy, nq, nullptr, 0, s, w);
    else go<false, true, false>(int_grid(nq * lanes), qx, qy, nq, nullptr, 0, s, w);
  }
  void launch_eval(const T* qx, const T* qy, uint64_t nq, T* out, uint64_t stride, hipStream_t s, bool check,
                   unsigned long long* w) override {
    const bool wave = int_wave_mapping(lanes);
    const unsigned g = int_grid(wave ? nq * 64 : nq * lanes);
    if (wave) {
      if (check) go<true, true, true>(g, qx, qy, nq, out, stride, s, w);
      else go<true, false, true>(g, qx, qy, nq, out, stride, s, w);
    } else {
      if (check) go<false, true, true>(g, qx, qy, nq, out, stride, s, w);
      else go<false, false, true>(g, qx, qy, nq, out, stride, s, w);
    }
  }
  ndi_status diagnose_at(T x, T y, ndi_oob_info* info) override {
    info->value = (double)x;
    if (this->emode == EX_NO && !(hx[0] <= x && x <= hx[nx - 1])) {   // x before y (bilinear.rs:71-80)
      info->axis = 0;
      info->status = NDI_OUT_OF_BOUNDS;
      return fail(NDI_OUT_OF_BOUNDS, "x = %lld is not in range", (long long)x);
    }
    if (this->emode == EX_NO && !(hy[0] <= y && y <= hy[ny - 1])) {
      info->value = (double)y;
      info->axis = 1;
      info->status = NDI_OUT_OF_BOUNDS;
      return fail(NDI_OUT_OF_BOUNDS, "y = %lld is not in range", (long long)y);
    }
    const uint64_t xi = int_lower_index_host(hx, x), yi = int_lower_index_host(hy, y);
    std::vector<IntRec<T>> a(2 * lanes), b(2 * lanes);   // (xi, yi..yi+1), (xi+1, yi..yi+1)
    const IntRec<T>* r = rec.as<IntRec<T>>();
    NDI_HIP(hipMemcpy(a.data(), r + (xi * ny + yi) * lanes, 2 * lanes * sizeof(IntRec<T>), hipMemcpyDeviceToHost));
    NDI_HIP(hipMemcpy(b.data(), r + ((xi + 1) * ny + yi) * lanes, 2 * lanes * sizeof(IntRec<T>),
                      hipMemcpyDeviceToHost));
    const T x1 = hx[xi], x2 = hx[xi + 1], y1 = hy[yi], y2 = hy[yi + 1];
    for (uint64_t l = 0; l < lanes; ++l) {   // bilinear.rs:88-97
      T z1, z2, res;
      int op = int_calc_frac_host<T>(x1, a[l].v, x2, b[l].v, x, z1);
      if (op < 0) op = int_calc_frac_host<T>(x1, a[lanes + l].v, x2, b[lanes + l].v, x, z2);
      if (op < 0) op = int_calc_frac_host<T>(y1, z1, y2, z2, y, res);
      if (op >= 0) return this->overflow(op, info);
    }
    return fail(NDI_HIP_ERROR, "integer evaluation reported a query as failing, but it evaluates");
  }

  ndi_status eval(const void* qx, const void* qy, uint64_t nq, void* out, uint64_t out_stride,
                  const ndi_eval_opts* opts, ndi_oob_info* info) override {
    if (nq && !qy) return fail(NDI_BAD_ARG, "null query pointer");
    return this->run(qx, qy, nq, out, out_stride, opts, info);
  }
  ndi_status finish(void* stream, ndi_oob_info* info) override { return this->finish_impl(stream, info); }
  ndi_status eval_ring(const void* qx, const void* qy, uint64_t nq, const ndi_ring_desc* ring,
                       ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts, ndi_oob_info* info) override {
    if (nq && !qy) return fail(NDI_BAD_ARG, "null query pointer");
    return this->run_ring(qx, qy, nq, ring, consume, user, opts, info);
  }
  ndi_status trim() override { return this->trim_impl(); }
  ndi_status probe_ceiling(uint64_t, void*, uint64_t, void*, int, double*) override {
    return fail(NDI_UNSUPPORTED, "probe_ceiling measures the float gather; not available for integer handles");
  }

  ndi_status build(const T* data_dev) {
    kx.reserve(nx * sizeof(T));
    ky.reserve(ny * sizeof(T));
    NDI_HIP(hipMemcpy(kx.p, hx.data(), nx * sizeof(T), hipMemcpyHostToDevice));
    NDI_HIP(hipMemcpy(ky.p, hy.data(), ny * sizeof(T), hipMemcpyHostToDevice));
    std::vector<IntYIv<T>> yv(ny - 1);
    for (uint64_t j = 0; j + 1 < ny; ++j) {
      T dy;
      yv[j] = IntYIv<T>{IntMagic<T>{0, 0, 1}, (T)0, 0};
      if (__builtin_sub_overflow(hy[j + 1], hy[j], &dy) || dy <= 0) {
        yv[j].bad = 1;   // dy overflows T (a strictly rising axis has dy >= 1)
      } else {
        yv[j].mg = int_magic<T>(dy);
        yv[j].dy = dy;
      }
    }
    yiv.reserve(yv.size() * sizeof(IntYIv<T>));
    NDI_HIP(hipMemcpy(yiv.p, yv.data(), yv.size() * sizeof(IntYIv<T>), hipMemcpyHostToDevice));
    const uint64_t total = nx * ny * lanes;
    rec.reserve(total * sizeof(IntRec<T>));
    pbad.reserve(nx * ny);
    NDI_HIP(hipMemset(pbad.p, 0, nx * ny));
    hipLaunchKernelGGL(int_slopes2d_kernel<T>, dim3(int_grid(total)), dim3(BLOCK), 0, (hipStream_t) nullptr,
                       kx.as<T>(), data_dev, nx, ny, lanes, rec.as<IntRec<T>>(), pbad.as<uint8_t>());
    NDI_HIP(hipGetLastError());
    NDI_HIP(hipDeviceSynchronize());
    return NDI_OK;
  }

  ndi_status clone_to(int d, Interp2DBase** out) override {
    std::unique_ptr<Interp2DIntImpl<T>> c(new Interp2DIntImpl<T>());
    {
      DeviceGuard dg(d);
      set_scalars(*c, dtype, d, this->emode, lanes);
      c->nx = nx; c->ny = ny; c->hx = hx; c->hy = hy;
      c->kx.reserve(kx.bytes); c->ky.reserve(ky.bytes); c->rec.reserve(rec.bytes);
      c->pbad.reserve(pbad.bytes); c->yiv.reserve(yiv.bytes);
    }
    copy_across_devices(c->kx.p, d, kx.p, device, kx.bytes);
    copy_across_devices(c->ky.p, d, ky.p, device, ky.bytes);
    copy_across_devices(c->rec.p, d, rec.p, device, rec.bytes);
    copy_across_devices(c->pbad.p, d, pbad.p, device, pbad.bytes);
    copy_across_devices(c->yiv.p, d, yiv.p, device, yiv.bytes);
    *out = c.release();
    return NDI_OK;
  }
};

template <class T>
static ndi_status create2d_int(const ndi_interp2d_desc& d, Interp2DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp2d_create");
  std::unique_ptr<Interp2DIntImpl<T>> h(new Interp2DIntImpl<T>());
  set_scalars(*h, d.dtype, d.device, d.extrapolate ? EX_YES : EX_NO, d.lanes);
  h->nx = d.nx;
  h->ny = d.ny;
  h->hx = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.nx);
  h->hy = d.y ? fetch_axis<T>(d.y, d.y_len, d.memspace) : default_axis<T>(d.ny);
  if (const ndi_status st = check_desc_2d(d, h->hx.data(), h->hy.data()); st != NDI_OK) return st;
  const size_t bytes = (size_t)d.nx * d.ny * d.lanes * sizeof(T);
  DevBuf tmp;
  const T* src = static_cast<const T*>(d.data);
  if (d.memspace != NDI_MEM_DEVICE) {
    tmp.reserve(bytes);
    NDI_HIP(hipMemcpy(tmp.p, d.data, bytes, hipMemcpyHostToDevice));
    src = tmp.as<T>();
  }
  ndi_status st = h->build(src);
  if (st != NDI_OK) return st;
  *out = h.release();
  return NDI_OK;
}

// ---- locator ----------------------------------------------------------------------------------------------------
template <class T>
struct IntLocatorImpl final : LocatorBase {
  DevBuf knots, qbuf, obuf;
  uint64_t n = 0;
  std::mutex mu;
  ndi_status eval(const void* q, uint64_t nq, int64_t* out_idx, int memspace, void* stream) override {
    DeviceGuard dg(device);
    if (nq == 0) return NDI_OK;
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t s = (hipStream_t)stream;
    const T* qd = static_cast<const T*>(q);
    int64_t* od = out_idx;
    if (memspace == NDI_MEM_HOST) {
      qbuf.reserve(nq * sizeof(T));
      obuf.reserve(nq * sizeof(int64_t));
      NDI_HIP(hipMemcpyAsync(qbuf.p, q, nq * sizeof(T), hipMemcpyHostToDevice, s));
      qd = qbuf.as<T>();
      od = obuf.as<int64_t>();
    }
    hipLaunchKernelGGL(int_locate_kernel<T>, dim3(int_grid(nq)), dim3(BLOCK), 0, s, qd, nq, knots.as<T>(),
                       (uint32_t)n, od);
    NDI_HIP(hipGetLastError());
    if (memspace == NDI_MEM_HOST)
      NDI_HIP(hipMemcpyAsync(out_idx, od, nq * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    return NDI_OK;
  }
};

template <class T>
static ndi_status create_int_locator(int device, const void* knots, uint64_t n, int memspace, LocatorBase** out) {
  DeviceGuard dg(device);
  if (n < 2) return fail(NDI_BAD_ARG, "get_lower_index needs at least 2 knots");
  if (n > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "too many knots");
  std::unique_ptr<IntLocatorImpl<T>> h(new IntLocatorImpl<T>());
  h->dtype = DType<T>::id;
  h->device = device;
  h->n = n;
  std::vector<T> x = fetch_axis<T>(knots, n, memspace);
  h->knots.reserve(n * sizeof(T));
  NDI_HIP(hipMemcpy(h->knots.p, x.data(), n * sizeof(T), hipMemcpyHostToDevice));
  *out = h.release();
  return NDI_OK;
}
