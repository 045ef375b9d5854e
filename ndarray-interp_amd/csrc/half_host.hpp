// csrc/half_host.hpp -- host side of the f16 / bf16 Linear and Bilinear handles (included by ndinterp_api.hip inside
// namespace ndi, after the integer handles; kernels in half_kernels.hpp).
//
// T values travel as their 16-bit patterns (uint16_t); the host keeps f32 images of the knots (exact) for the range
// bounds, the diagnosis of a failing query and the replica signature.  HalfEngine is the NarrowEngine (narrow_host.hpp:
// staging, first_fail, eval_rows, the ring, trim, the sharded call) of these handles.  Its own part:
//   run          ndi_interp{1,2}d_eval.  Caller-owned buffers: the write-free range pre-pass records the first failing
//                query in a device word and the evaluation kernel, on the same stream, skips the rows at / after it --
//                no host round trip in between, so async_launch (device output) really returns after the enqueue and
//                ndi_interp{1,2}d_finish reads the word.  FRESH_OUTPUT / ROWS_AFTER_ERROR_UNSPECIFIED: one fused pass
//   diagnose     the failing query alone, on the host: range test (x before y) or NaN while extrapolating
// Scratch (staged queries, host-output bounce buffer, the first-failure word) is kept per stream.  Calls on one handle
// are serialised by the engine's mutex.

template <int F>
static float half_to_float_host(uint16_t u) {
  uint32_t b;
  if (F == HF_BF16) {
    b = (uint32_t)u << 16;
  } else {
    const uint32_t s = (uint32_t)(u & 0x8000u) << 16, e = (u >> 10) & 0x1fu, m = u & 0x3ffu;
    if (e == 0x1f) b = s | 0x7f800000u | (m << 13);
    else if (e != 0) b = s | ((e + 112u) << 23) | (m << 13);
    else return (s ? -1.0f : 1.0f) * std::ldexp((float)m, -24);   // zero / subnormal (exact)
  }
  float f;
  std::memcpy(&f, &b, sizeof(f));
  return f;
}

template <int F>
static std::vector<float> half_images(const std::vector<uint16_t>& v) {
  std::vector<float> f(v.size());
  for (size_t i = 0; i < v.size(); ++i) f[i] = half_to_float_host<F>(v[i]);
  return f;
}

template <int F>
static std::vector<float> half_images(const void* host_v, uint64_t n) {
  const uint16_t* p = static_cast<const uint16_t*>(host_v);
  return half_images<F>(std::vector<uint16_t>(p, p + n));
}

// The default axis 0..n cast to T (interp1d/mod.rs:402-406), as f32 images: integers rounded to T's significand
// (11 bits for f16, 8 for bf16) with ties to even, inf beyond T's range.
template <int F>
static std::vector<float> half_default_axis(uint64_t n) {
  const int bits = F == HF_F16 ? 11 : 8;
  const double maxv = F == HF_F16 ? 65504.0 : 3.3895313892515355e38;
  std::vector<float> v(n);
  for (uint64_t i = 0; i < n; ++i) {
    double x = (double)i;
    const int e = x > 0 ? std::ilogb(x) : 0;
    if (e >= bits) {
      const double q = std::ldexp(1.0, e - bits + 1);
      x = std::nearbyint(x / q) * q;   // default rounding mode: to nearest, ties to even
    }
    v[i] = x > maxv ? INFINITY : (float)x;
  }
  return v;
}

static unsigned half_grid(uint64_t units, unsigned cap_per_cu) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(units, (uint64_t)cu_count() * cap_per_cu));
}

// Mapping of a row of `lanes` elements: one element per thread up to 32 elements (scalar data: a query per
// thread), beyond that one query per group of lanes, the group as wide as the row's 16-byte vectors (8 .. 64 lanes).
// NDI_HALF_MAP = 1 / 2 forces the element / group mapping (tests).
static bool half_group_mapping(uint64_t lanes) {
  static const Knob map{"NDI_HALF_MAP", 0};
  if (map.get() == 1) return false;
  if (map.get() == 2) return true;
  return lanes > 32;
}
static uint32_t half_glog(uint64_t lanes, bool vec) {
  const uint64_t units = vec ? lanes / 8 : lanes;
  uint32_t g = 0;
  while (g < 6 && (1ull << g) < units) ++g;
  return g;
}

template <int F>
struct HalfEngine : NarrowEngine<uint16_t> {
  HalfBounds bnd{};
  std::map<void*, std::unique_ptr<NarrowScratch>> scratch;   // per stream
  struct Pending {
    bool launched;                  // device output, enqueued: the status is read from the stream's word at finish
    const void *qx, *qy;
    uint64_t nq;
    int qmem;
    ndi_status st;
    ndi_oob_info info;
    std::string err;
  };
  std::map<void*, Pending> pending;   // async_launch batches awaiting finish, per stream

  virtual void launch_eval(const uint16_t* qx, const uint16_t* qy, uint64_t nq, uint16_t* out, uint64_t stride,
                           hipStream_t s, bool check, const unsigned long long* limit, unsigned long long* w) = 0;
  virtual ndi_status diagnose_at(float x, float y, ndi_oob_info* info) = 0;

  NarrowScratch& ws(hipStream_t s) override {
    std::unique_ptr<NarrowScratch>& p = scratch[(void*)s];
    if (!p) p.reset(new NarrowScratch());
    return *p;
  }
  void release_scratch() override {
    if (pending.empty()) scratch.clear();   // an async batch still reads its stream's word
  }
  const char* bucketed_refusal() const override {
    return "NDI_PATH_BUCKETED is not available for f16 / bf16 (AUTO / GATHER)";
  }
  void launch_check(const uint16_t* qx, const uint16_t* qy, uint64_t nq, hipStream_t s,
                    unsigned long long* w) override {
    hipLaunchKernelGGL(half_check_kernel<F>, dim3(half_grid((nq + BLOCK - 1) / BLOCK, 16)), dim3(BLOCK), 0, s, qx, qy,
                       nq, emode, bnd, w);
  }
  void launch_rows(const uint16_t* dx, const uint16_t* dy, uint64_t cnt, uint16_t* out, uint64_t stride,
                   hipStream_t s) override {
    launch_eval(dx, dy, cnt, out, stride, s, false, nullptr, nullptr);
  }
  // one host thread per shard; what a thread throws becomes the call's status (lowest shard first)
  ndi_status each_shard(uint32_t ns, const std::function<void(uint32_t)>& fn) override {
    std::vector<ndi_status> sst(ns, NDI_OK);
    std::vector<std::string> serr(ns);
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < ns; ++i)
      th.emplace_back([&, i] {
        try {
          fn(i);
        } catch (const HipFailure& f) {
          sst[i] = from_hip(f);
          serr[i] = tls_error();
        } catch (...) {
          sst[i] = NDI_HIP_ERROR;
          serr[i] = "unexpected C++ exception in a shard thread";
        }
      });
    for (std::thread& t : th) t.join();
    for (uint32_t i = 0; i < ns; ++i)
      if (sst[i] != NDI_OK) {
        tls_error() = serr[i];
        return sst[i];
      }
    return NDI_OK;
  }

  // Pre-pass + limited evaluation (caller-owned rows) or the fused pass, all enqueued on s; the word holds the first
  // failing query afterwards.
  void enqueue(const uint16_t* dx, const uint16_t* dy, uint64_t nq, uint16_t* out, uint64_t stride, bool fused,
               NarrowScratch& W, hipStream_t s) {
    unsigned long long* w = reset_word(W, s);
    if (fused) {
      launch_eval(dx, dy, nq, out, stride, s, true, nullptr, w);
    } else {
      launch_check(dx, dy, nq, s, w);
      NDI_HIP(hipGetLastError());
      launch_eval(dx, dy, nq, out, stride, s, false, w, nullptr);
    }
    NDI_HIP(hipGetLastError());
  }

  // The failing query j alone: its x (and y) fetched, the reference's checks replayed in order.
  ndi_status diagnose(const void* qx, const void* qy, uint64_t j, int qmem, uint64_t index,
                      ndi_oob_info* info) override {
    uint16_t x = 0, y = 0;
    fetch_query(qx, qy, j, qmem, &x, &y);
    ndi_oob_info tmp{};
    if (!info) info = &tmp;
    ndi_status st = diagnose_at(half_to_float_host<F>(x), half_to_float_host<F>(y), info);
    info->index = index;
    if (st == NDI_NAN_QUERY) return fail(st, "failed to convert NaN to usize (query %llu)", (unsigned long long)index);
    if (st != NDI_OUT_OF_BOUNDS) return st;   // diagnose_at has set the message
    return fail(st, "%s = %.9g is not in range", info->axis == 0 ? "x" : "y", info->value);
  }
  ndi_status out_of_bounds(int axis, float v, ndi_oob_info* info) {
    info->axis = axis;
    info->value = (double)v;
    info->status = NDI_OUT_OF_BOUNDS;
    return NDI_OUT_OF_BOUNDS;
  }
  ndi_status nan_query(float v, ndi_oob_info* info) {
    info->axis = 0;
    info->value = (double)v;
    info->status = NDI_NAN_QUERY;
    return NDI_NAN_QUERY;
  }

  ndi_status run(const void* qx, const void* qy, uint64_t nq, void* out, uint64_t stride, const ndi_eval_opts* opts,
                 ndi_oob_info* info) {
    ndi_eval_opts o{};
    if (const ndi_status hs = run_head(opts, o, qx, out, nq, stride, info); hs != NDI_OK) return hs;
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t s = (hipStream_t)o.stream;
    ndi_status st = NDI_OK;
    if (nq) {
      NarrowScratch& W = ws(s);
      const uint16_t* dx = stage(qx, nq, o.q_memspace, W.qx, s);
      const uint16_t* dy = stage(qy, nq, o.q_memspace, W.qy, s);
      const bool fused = (o.flags & (NDI_EVAL_FRESH_OUTPUT | NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED)) != 0;
      const bool dev_out = o.out_memspace == NDI_MEM_DEVICE;
      if (dev_out) {
        enqueue(dx, dy, nq, static_cast<uint16_t*>(out), stride, fused, W, s);
        if (o.async_launch) {
          pending[o.stream] = Pending{true, qx, qy, nq, o.q_memspace, NDI_OK, ndi_oob_info{0, 0.0, 0, NDI_OK}, {}};
          return NDI_OK;
        }
      } else {
        W.out.reserve(nq * elanes * sizeof(uint16_t));
        enqueue(dx, dy, nq, W.out.as<uint16_t>(), elanes, fused, W, s);
      }
      const uint64_t F_ = read_word(W, s);
      const uint64_t rows = std::min<uint64_t>(F_, nq);
      if (!dev_out && rows) {
        rows_to_host(out, stride, W.out, rows, s);
        NDI_HIP(hipStreamSynchronize(s));
      }
      if (F_ < nq) st = diagnose(qx, qy, F_, o.q_memspace, F_, info);
    }
    if (o.async_launch) {   // completed inside the call (host output or an empty batch): finish reports it
      pending[o.stream] = Pending{false, nullptr, nullptr, 0, 0, st, info ? *info : ndi_oob_info{0, 0.0, 0, st},
                                  st == NDI_OK ? std::string() : tls_error()};
      return NDI_OK;
    }
    return st;
  }

  ndi_status finish_impl(void* stream, ndi_oob_info* info) {
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    auto it = pending.find(stream);
    if (it == pending.end()) return NDI_OK;
    const Pending p = it->second;
    pending.erase(it);
    if (p.launched) {
      const uint64_t F_ = read_word(ws((hipStream_t)stream), (hipStream_t)stream);
      return F_ < p.nq ? diagnose(p.qx, p.qy, F_, p.qmem, F_, info) : NDI_OK;
    }
    if (info) *info = p.info;
    if (p.st != NDI_OK) tls_error() = p.err;
    return p.st;
  }
};

// ---- 1-D --------------------------------------------------------------------------------------------------------
template <int F>
struct Interp1DHalfImpl final : Interp1DBase, HalfEngine<F> {
  uint64_t n = 0;
  std::vector<float> hx;   // f32 images of the knots
  DevBuf kf, data;         // f32 knot images, the data as given (T)

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, &dtype, sizeof(dtype));
    h = fnv1a(h, &this->emode, sizeof(int));
    h = fnv1a(h, &n, sizeof(n));
    h = fnv1a(h, &lanes, sizeof(lanes));
    return fnv1a(h, hx.data(), hx.size() * sizeof(float));
  }
  template <bool WAVE, bool CHECK, bool VEC>
  void go(unsigned g, uint32_t glog, const uint16_t* q, uint64_t nq, uint16_t* out, uint64_t stride, hipStream_t s,
          const unsigned long long* limit, unsigned long long* w) {
    const bool lds = n <= HALF_LDS_KNOTS;
    hipLaunchKernelGGL((half_eval1d_kernel<F, WAVE, CHECK, VEC>), dim3(g), dim3(BLOCK), lds ? n * sizeof(float) : 0, s,
                       q, nq, kf.as<float>(), (uint32_t)n, this->emode, this->bnd, lds, data.as<uint16_t>(), lanes,
                       out, stride, glog, limit, w);
  }
  void launch_eval(const uint16_t* q, const uint16_t*, uint64_t nq, uint16_t* out, uint64_t stride, hipStream_t s,
                   bool check, const unsigned long long* limit, unsigned long long* w) override {
    if (half_group_mapping(lanes)) {
      const bool vec = lanes % 8 == 0 && stride % 8 == 0 && ((uintptr_t)out & 15) == 0;
      const uint32_t glog = half_glog(lanes, vec);
      const unsigned g = half_grid((nq + (BLOCK >> glog) - 1) / (BLOCK >> glog), 8);
      if (vec) {
        if (check) go<true, true, true>(g, glog, q, nq, out, stride, s, limit, w);
        else go<true, false, true>(g, glog, q, nq, out, stride, s, limit, w);
      } else {
        if (check) go<true, true, false>(g, glog, q, nq, out, stride, s, limit, w);
        else go<true, false, false>(g, glog, q, nq, out, stride, s, limit, w);
      }
    } else {
      const unsigned g = half_grid((nq * lanes + BLOCK - 1) / BLOCK, 8);
      if (check) go<false, true, false>(g, 0, q, nq, out, stride, s, limit, w);
      else go<false, false, false>(g, 0, q, nq, out, stride, s, limit, w);
    }
  }
  ndi_status diagnose_at(float x, float, ndi_oob_info* info) override {
    if (this->emode == EX_NO && !(hx[0] <= x && x <= hx[n - 1])) return this->out_of_bounds(0, x, info);
    if (x != x) return this->nan_query(x, info);
    return fail(NDI_HIP_ERROR, "f16 / bf16 evaluation reported query %g as failing, but it evaluates", (double)x);
  }

  ndi_status eval(const void* q, uint64_t nq, void* out, uint64_t out_stride, const ndi_eval_opts* opts,
                  ndi_oob_info* info) override {
    return this->run(q, nullptr, nq, out, out_stride, opts, info);
  }
  ndi_status finish(void* stream, ndi_oob_info* info) override { return this->finish_impl(stream, info); }
  ndi_status coefficients(void*, void*, int) override {
    return fail(NDI_BAD_ARG, "coefficients: an f16 / bf16 handle is a Linear interpolator (no spline tables)");
  }
  ndi_status derivative(int, Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "derivative: an f16 / bf16 handle is a Linear interpolator: its slope jumps at the knots "
                "(derivative takes f32 / f64 CubicSpline, Pchip, Akima and CubicHermite handles)");
  }
  ndi_status antiderivative(Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "antiderivative: an f16 / bf16 handle is a Linear interpolator of a narrow element type: the prefix table would "
                "round at every knot (antiderivative takes f32 / f64 Linear, CubicSpline, Pchip, Akima and CubicHermite handles)");
  }
  ndi_status inverse(Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "inverse: an f16 / bf16 handle is a Linear interpolator of a narrow element type: the returned abscissae "
                "would round to it (inverse takes f32 / f64 Linear, CubicSpline, Pchip, Akima, CubicHermite, derivative and "
                "antiderivative handles)");
  }
  ndi_status data_table(void* data_out, int memspace) override {
    DeviceGuard dg(device);
    NDI_HIP(hipMemcpy(data_out, data.p, n * lanes * sizeof(uint16_t),
                      memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return NDI_OK;
  }
  ndi_status eval_ring(const void* q, uint64_t nq, const ndi_ring_desc* ring, ndi_ring_consumer consume, void* user,
                       const ndi_eval_opts* opts, ndi_oob_info* info) override {
    return this->run_ring(q, nullptr, nq, ring, consume, user, opts, info);
  }
  ndi_status trim() override { return this->trim_impl(); }
  uint64_t scratch_sets() override { return this->scratch.size(); }

  ndi_status clone_to(int d, Interp1DBase** out) override {
    std::unique_ptr<Interp1DHalfImpl<F>> c(new Interp1DHalfImpl<F>());
    {
      DeviceGuard dg(d);
      set_scalars(*c, dtype, d, this->emode, lanes);
      c->n = n; c->hx = hx; c->bnd = this->bnd;
      c->kf.reserve(kf.bytes); c->data.reserve(data.bytes);
    }
    copy_across_devices(c->kf.p, d, kf.p, device, kf.bytes);
    copy_across_devices(c->data.p, d, data.p, device, data.bytes);
    *out = c.release();
    return NDI_OK;
  }
};

template <int F>
static ndi_status create1d_half(const ndi_interp1d_desc& d, Interp1DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp1d_create");
  std::unique_ptr<Interp1DHalfImpl<F>> h(new Interp1DHalfImpl<F>());
  set_scalars(*h, d.dtype, d.device, d.extrapolate ? EX_YES : EX_NO, d.lanes);
  h->n = d.n;
  h->hx = d.x ? half_images<F>(fetch_axis<uint16_t>(d.x, d.x_len, d.memspace)) : half_default_axis<F>(d.n);
  if (const ndi_status st = check_desc_1d(d, h->hx.data()); st != NDI_OK) return st;
  h->bnd = HalfBounds{h->hx[0], h->hx[d.n - 1], 0.0f, 0.0f};
  h->kf.reserve(d.n * sizeof(float));
  NDI_HIP(hipMemcpy(h->kf.p, h->hx.data(), d.n * sizeof(float), hipMemcpyHostToDevice));
  const size_t bytes = (size_t)d.n * d.lanes * sizeof(uint16_t);
  h->data.reserve(bytes);
  NDI_HIP(hipMemcpy(h->data.p, d.data, bytes, d.memspace == NDI_MEM_DEVICE ? hipMemcpyDeviceToDevice
                                                                         : hipMemcpyHostToDevice));
  *out = h.release();
  return NDI_OK;
}

// ---- 2-D --------------------------------------------------------------------------------------------------------
template <int F>
struct Interp2DHalfImpl final : Interp2DBase, HalfEngine<F> {
  uint64_t nx = 0, ny = 0;
  std::vector<float> hx, hy;
  DevBuf kxf, kyf, grid;

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, &dtype, sizeof(dtype));
    h = fnv1a(h, &this->emode, sizeof(int));
    h = fnv1a(h, &lanes, sizeof(lanes));
    h = fnv1a(h, hx.data(), hx.size() * sizeof(float));
    return fnv1a(h, hy.data(), hy.size() * sizeof(float));
  }
  template <bool WAVE, bool CHECK, bool VEC>
  void go(unsigned g, uint32_t glog, const uint16_t* qx, const uint16_t* qy, uint64_t nq, uint16_t* out,
          uint64_t stride, hipStream_t s, const unsigned long long* limit, unsigned long long* w) {
    const bool lds = nx + ny <= HALF_LDS_KNOTS;
    hipLaunchKernelGGL((half_eval2d_kernel<F, WAVE, CHECK, VEC>), dim3(g), dim3(BLOCK),
                       lds ? (nx + ny) * sizeof(float) : 0, s, qx, qy, nq, kxf.as<float>(), (uint32_t)nx,
                       kyf.as<float>(), (uint32_t)ny, this->emode, this->bnd, lds, grid.as<uint16_t>(), lanes, out,
                       stride, glog, limit, w);
  }
  void launch_eval(const uint16_t* qx, const uint16_t* qy, uint64_t nq, uint16_t* out, uint64_t stride, hipStream_t s,
                   bool check, const unsigned long long* limit, unsigned long long* w) override {
    if (half_group_mapping(lanes)) {
      const bool vec = lanes % 8 == 0 && stride % 8 == 0 && ((uintptr_t)out & 15) == 0;
      const uint32_t glog = half_glog(lanes, vec);
      const unsigned g = half_grid((nq + (BLOCK >> glog) - 1) / (BLOCK >> glog), 8);
      if (vec) {
        if (check) go<true, true, true>(g, glog, qx, qy, nq, out, stride, s, limit, w);
        else go<true, false, true>(g, glog, qx, qy, nq, out, stride, s, limit, w);
      } else {
        if (check) go<true, true, false>(g, glog, qx, qy, nq, out, stride, s, limit, w);
        else go<true, false, false>(g, glog, qx, qy, nq, out, stride, s, limit, w);
      }
    } else {
      const unsigned g = half_grid((nq * lanes + BLOCK - 1) / BLOCK, 8);
      if (check) go<false, true, false>(g, 0, qx, qy, nq, out, stride, s, limit, w);
      else go<false, false, false>(g, 0, qx, qy, nq, out, stride, s, limit, w);
    }
  }
  ndi_status diagnose_at(float x, float y, ndi_oob_info* info) override {
    if (this->emode == EX_NO && !(hx[0] <= x && x <= hx[nx - 1])) return this->out_of_bounds(0, x, info);
    if (this->emode == EX_NO && !(hy[0] <= y && y <= hy[ny - 1])) return this->out_of_bounds(1, y, info);
    if (x != x) return this->nan_query(x, info);   // get_lower_index on x first (bilinear.rs:81-82)
    if (y != y) return this->nan_query(y, info);
    return fail(NDI_HIP_ERROR, "f16 / bf16 evaluation reported a query as failing, but it evaluates");
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
    return fail(NDI_UNSUPPORTED, "probe_ceiling measures the float gather; not available for f16 / bf16 handles");
  }

  ndi_status clone_to(int d, Interp2DBase** out) override {
    std::unique_ptr<Interp2DHalfImpl<F>> c(new Interp2DHalfImpl<F>());
    {
      DeviceGuard dg(d);
      set_scalars(*c, dtype, d, this->emode, lanes);
      c->nx = nx; c->ny = ny; c->hx = hx; c->hy = hy; c->bnd = this->bnd;
      c->kxf.reserve(kxf.bytes); c->kyf.reserve(kyf.bytes); c->grid.reserve(grid.bytes);
    }
    copy_across_devices(c->kxf.p, d, kxf.p, device, kxf.bytes);
    copy_across_devices(c->kyf.p, d, kyf.p, device, kyf.bytes);
    copy_across_devices(c->grid.p, d, grid.p, device, grid.bytes);
    *out = c.release();
    return NDI_OK;
  }
};

template <int F>
static ndi_status create2d_half(const ndi_interp2d_desc& d, Interp2DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp2d_create");
  std::unique_ptr<Interp2DHalfImpl<F>> h(new Interp2DHalfImpl<F>());
  set_scalars(*h, d.dtype, d.device, d.extrapolate ? EX_YES : EX_NO, d.lanes);
  h->nx = d.nx;
  h->ny = d.ny;
  h->hx = d.x ? half_images<F>(fetch_axis<uint16_t>(d.x, d.x_len, d.memspace)) : half_default_axis<F>(d.nx);
  h->hy = d.y ? half_images<F>(fetch_axis<uint16_t>(d.y, d.y_len, d.memspace)) : half_default_axis<F>(d.ny);
  if (const ndi_status st = check_desc_2d(d, h->hx.data(), h->hy.data()); st != NDI_OK) return st;
  h->bnd = HalfBounds{h->hx[0], h->hx[d.nx - 1], h->hy[0], h->hy[d.ny - 1]};
  h->kxf.reserve(d.nx * sizeof(float));
  h->kyf.reserve(d.ny * sizeof(float));
  NDI_HIP(hipMemcpy(h->kxf.p, h->hx.data(), d.nx * sizeof(float), hipMemcpyHostToDevice));
  NDI_HIP(hipMemcpy(h->kyf.p, h->hy.data(), d.ny * sizeof(float), hipMemcpyHostToDevice));
  const size_t bytes = (size_t)d.nx * d.ny * d.lanes * sizeof(uint16_t);
  h->grid.reserve(bytes);
  NDI_HIP(hipMemcpy(h->grid.p, d.data, bytes, d.memspace == NDI_MEM_DEVICE ? hipMemcpyDeviceToDevice
                                                                          : hipMemcpyHostToDevice));
  *out = h.release();
  return NDI_OK;
}

// ---- locator ----------------------------------------------------------------------------------------------------
// The float locator over the knots' f32 images; queries are converted to f32 first (exact, order-preserving).
template <int F>
struct HalfLocatorImpl final : LocatorBase {
  std::unique_ptr<LocatorBase> f32;
  DevBuf qbuf;
  std::mutex mu;
  ndi_status eval(const void* q, uint64_t nq, int64_t* out_idx, int memspace, void* stream) override {
    DeviceGuard dg(device);
    if (nq == 0) return NDI_OK;
    f32->one_shot = one_shot;
    if (memspace == NDI_MEM_HOST) {
      const std::vector<float> qf = half_images<F>(q, nq);
      return f32->eval(qf.data(), nq, out_idx, NDI_MEM_HOST, stream);
    }
    std::lock_guard<std::mutex> lk(mu);
    qbuf.reserve(nq * sizeof(float));
    hipLaunchKernelGGL(half_to_f32_kernel<F>, dim3(half_grid((nq + BLOCK - 1) / BLOCK, 16)), dim3(BLOCK), 0,
                       (hipStream_t)stream, static_cast<const uint16_t*>(q), nq, qbuf.as<float>());
    NDI_HIP(hipGetLastError());
    return f32->eval(qbuf.p, nq, out_idx, NDI_MEM_DEVICE, stream);
  }
};

template <int F>
static ndi_status create_half_locator(int device, const void* knots, uint64_t n, int memspace, LocatorBase** out) {
  DeviceGuard dg(device);
  if (n < 2) return fail(NDI_BAD_ARG, "get_lower_index needs at least 2 knots");
  std::unique_ptr<HalfLocatorImpl<F>> h(new HalfLocatorImpl<F>());
  h->dtype = F == HF_F16 ? NDI_F16 : NDI_BF16;
  h->device = device;
  const std::vector<float> x = half_images<F>(fetch_axis<uint16_t>(knots, n, memspace));
  LocatorBase* inner = nullptr;
  ndi_status st = create_locator<float>(device, x.data(), n, NDI_MEM_HOST, &inner);
  if (st != NDI_OK) return st;
  h->f32.reset(inner);
  *out = h.release();
  return NDI_OK;
}
