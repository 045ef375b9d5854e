// csrc/half_host.hpp -- host side of the f16 / bf16 Linear and Bilinear handles (included by ndinterp_api.hip inside
// namespace ndi, after the integer handles; kernels in half_kernels.hpp).
//
// T values travel as their 16-bit patterns (uint16_t); the host keeps f32 images of the knots (exact) for the range
// bounds, the diagnosis of a failing query and the replica signature.  One engine serves every entry point:
//   run          ndi_interp{1,2}d_eval.  Caller-owned buffers: the write-free range pre-pass records the first failing
//                query in a device word and the evaluation kernel, on the same stream, skips the rows at / after it --
//                no host round trip in between, so async_launch (device output) really returns after the enqueue and
//                ndi_interp{1,2}d_finish reads the word.  FRESH_OUTPUT / ROWS_AFTER_ERROR_UNSPECIFIED: one fused pass
//   run_ring     the pre-pass, then the rows below the first failure chunk by chunk
//   diagnose     the failing query alone, on the host: range test (x before y) or NaN while extrapolating
// Scratch (staged queries, host-output bounce buffer, the first-failure word) is kept per stream.  Calls on one handle
// are serialised by its mutex.

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
  static const int env = [] { const char* e = std::getenv("NDI_HALF_MAP"); return e ? std::atoi(e) : 0; }();
  if (env == 1) return false;
  if (env == 2) return true;
  return lanes > 32;
}
static uint32_t half_glog(uint64_t lanes, bool vec) {
  const uint64_t units = vec ? lanes / 8 : lanes;
  uint32_t g = 0;
  while (g < 6 && (1ull << g) < units) ++g;
  return g;
}

struct HalfScratch {
  DevBuf qx, qy, out, word;
};

template <int F>
struct HalfEngine {
  int dev = 0, emode = EX_NO;
  uint64_t elanes = 0;
  HalfBounds bnd{};
  std::mutex mu;
  std::map<void*, std::unique_ptr<HalfScratch>> scratch;   // per stream
  OwnedRing ring_own;
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

  virtual ~HalfEngine() = default;
  virtual void launch_eval(const uint16_t* qx, const uint16_t* qy, uint64_t nq, uint16_t* out, uint64_t stride,
                           hipStream_t s, bool check, const unsigned long long* limit, unsigned long long* w) = 0;
  virtual ndi_status diagnose_at(float x, float y, ndi_oob_info* info) = 0;

  HalfScratch& ws(hipStream_t s) {
    std::unique_ptr<HalfScratch>& p = scratch[(void*)s];
    if (!p) p.reset(new HalfScratch());
    return *p;
  }
  void release_scratch() { scratch.clear(); }

  const uint16_t* stage(const void* q, uint64_t nq, int memspace, DevBuf& buf, hipStream_t s) {
    if (!q || memspace == NDI_MEM_DEVICE) return static_cast<const uint16_t*>(q);
    buf.reserve(nq * sizeof(uint16_t));
    NDI_HIP(hipMemcpyAsync(buf.p, q, nq * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    return buf.as<uint16_t>();
  }
  unsigned long long* reset_word(HalfScratch& W, hipStream_t s) {
    W.word.reserve(sizeof(unsigned long long));
    NDI_HIP(hipMemsetAsync(W.word.p, 0xff, sizeof(unsigned long long), s));
    return W.word.as<unsigned long long>();
  }
  uint64_t read_word(HalfScratch& W, hipStream_t s) {
    unsigned long long f = NO_FAIL;
    NDI_HIP(hipMemcpyAsync(&f, W.word.p, sizeof(f), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    return f;
  }
  void launch_check(const uint16_t* qx, const uint16_t* qy, uint64_t nq, hipStream_t s, unsigned long long* w) {
    hipLaunchKernelGGL(half_check_kernel<F>, dim3(half_grid((nq + BLOCK - 1) / BLOCK, 16)), dim3(BLOCK), 0, s, qx, qy,
                       nq, emode, bnd, w);
    NDI_HIP(hipGetLastError());
  }
  // Pre-pass + limited evaluation (caller-owned rows) or the fused pass, all enqueued on s; the word holds the first
  // failing query afterwards.
  void enqueue(const uint16_t* dx, const uint16_t* dy, uint64_t nq, uint16_t* out, uint64_t stride, bool fused,
               HalfScratch& W, hipStream_t s) {
    unsigned long long* w = reset_word(W, s);
    if (fused) {
      launch_eval(dx, dy, nq, out, stride, s, true, nullptr, w);
    } else {
      launch_check(dx, dy, nq, s, w);
      launch_eval(dx, dy, nq, out, stride, s, false, w, nullptr);
    }
    NDI_HIP(hipGetLastError());
  }

  // The failing query j alone: its x (and y) fetched, the reference's checks replayed in order.
  ndi_status diagnose(const void* qx, const void* qy, uint64_t j, int qmem, uint64_t index, ndi_oob_info* info) {
    uint16_t x = 0, y = 0;
    if (qmem == NDI_MEM_DEVICE) {
      NDI_HIP(hipMemcpy(&x, static_cast<const uint16_t*>(qx) + j, sizeof(x), hipMemcpyDeviceToHost));
      if (qy) NDI_HIP(hipMemcpy(&y, static_cast<const uint16_t*>(qy) + j, sizeof(y), hipMemcpyDeviceToHost));
    } else {
      x = static_cast<const uint16_t*>(qx)[j];
      if (qy) y = static_cast<const uint16_t*>(qy)[j];
    }
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
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED is not available for f16 / bf16 (AUTO / GATHER)");
    if (stride < elanes)
      return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)stride,
                  (unsigned long long)elanes);
    if (nq && (!qx || !out)) return fail(NDI_BAD_ARG, "null query or output pointer");
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t s = (hipStream_t)o.stream;
    ndi_status st = NDI_OK;
    if (nq) {
      HalfScratch& W = ws(s);
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
        NDI_HIP(hipMemcpy2DAsync(out, stride * sizeof(uint16_t), W.out.p, elanes * sizeof(uint16_t),
                                 elanes * sizeof(uint16_t), rows, hipMemcpyDeviceToHost, s));
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

  // Rows [0, rows) through a device-output ring (rows already cut at the first failure).  q_begin: flat index of qx[0]
  // in the caller's batch; shard: reported in every chunk.
  void ring_rows(const uint16_t* dx, const uint16_t* dy, uint64_t rows, const ndi_ring_desc* ring, uint64_t stride,
                 ndi_ring_consumer consume, void* user, hipStream_t s, uint64_t q_begin, uint32_t shard) {
    const uint32_t ns = ring->n_slots;
    std::vector<uint16_t*> slots(ns);
    uint64_t rstride = stride;
    std::unique_lock<std::mutex> rl(ring_own.mu, std::defer_lock);
    if (ring->slots) {
      for (uint32_t i = 0; i < ns; ++i) slots[i] = static_cast<uint16_t*>(ring->slots[i]);
    } else {   // library-owned: one allocation, slots interleaved row by row (ndinterp.h)
      rl.lock();
      rstride = (uint64_t)ns * stride;
      ring_own.ensure(1, ring->chunk_queries, rstride * sizeof(uint16_t));
      for (uint32_t i = 0; i < ns; ++i) slots[i] = ring_own.buf.as<uint16_t>() + (uint64_t)i * stride;
    }
    std::vector<hipEvent_t> waits(ns, nullptr);
    uint64_t k = 0;
    for (uint64_t b = 0; b < rows; b += ring->chunk_queries, ++k) {
      const uint64_t cnt = std::min<uint64_t>(ring->chunk_queries, rows - b);
      const uint32_t slot = (uint32_t)(k % ns);
      if (waits[slot]) NDI_HIP(hipStreamWaitEvent(s, waits[slot], 0));
      waits[slot] = nullptr;
      launch_eval(dx + b, dy ? dy + b : nullptr, cnt, slots[slot], rstride, s, false, nullptr, nullptr);
      NDI_HIP(hipGetLastError());
      ndi_ring_chunk c{k, q_begin + b, cnt, slots[slot], rstride, slot, shard, (void*)s};
      waits[slot] = consume ? (hipEvent_t)consume(user, &c) : nullptr;
    }
    NDI_HIP(hipStreamSynchronize(s));
  }

  // Lowest failing query of [0, nq) (NO_FAIL if none), queries staged into the stream's scratch.
  uint64_t first_fail(const void* qx, const void* qy, uint64_t nq, int qmem, hipStream_t s, const uint16_t** dx,
                      const uint16_t** dy) {
    HalfScratch& W = ws(s);
    *dx = stage(qx, nq, qmem, W.qx, s);
    *dy = stage(qy, nq, qmem, W.qy, s);
    unsigned long long* w = reset_word(W, s);
    launch_check(*dx, *dy, nq, s, w);
    return read_word(W, s);
  }

  ndi_status run_ring(const void* qx, const void* qy, uint64_t nq, const ndi_ring_desc* ring,
                      ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts, ndi_oob_info* info) {
    ndi_eval_opts o{};
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED is not available for f16 / bf16 (AUTO / GATHER)");
    uint64_t stride = 0;
    if (const ndi_status rs = check_ring_desc(ring, elanes, &stride); rs != NDI_OK) return rs;
    if (nq && !qx) return fail(NDI_BAD_ARG, "null query pointer");
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    if (nq == 0) return NDI_OK;
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t s = (hipStream_t)o.stream;
    const uint16_t *dx, *dy;
    const uint64_t F_ = first_fail(qx, qy, nq, o.q_memspace, s, &dx, &dy);
    ring_rows(dx, dy, std::min<uint64_t>(F_, nq), ring, stride, consume, user, s, 0, 0);
    return F_ < nq ? diagnose(qx, qy, F_, o.q_memspace, F_, info) : NDI_OK;
  }

  ndi_status trim_impl() {
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    std::lock_guard<std::mutex> rl(ring_own.mu);
    if (pending.empty()) release_scratch();   // an async batch still reads its stream's word
    ring_own.clear();
    return NDI_OK;
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
      c->dtype = dtype; c->device = d; c->lanes = lanes; c->n = n; c->hx = hx;
      c->dev = d; c->elanes = lanes; c->emode = this->emode; c->bnd = this->bnd;
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
  h->dtype = d.dtype;
  h->device = h->dev = d.device;
  h->emode = d.extrapolate ? EX_YES : EX_NO;
  h->n = d.n;
  h->lanes = h->elanes = d.lanes;
  h->hx = d.x ? half_images<F>(fetch_axis<uint16_t>(d.x, d.x_len, d.memspace)) : half_default_axis<F>(d.n);
  const uint64_t x_len = d.x ? d.x_len : d.n;
  if (d.validate) {
    ndi_status st = check_axis_1d<float>(h->hx.data(), x_len, d.n, d.strategy);
    if (st != NDI_OK) return st;
  } else if (x_len != d.n || d.n < 2) {
    return fail(NDI_BAD_ARG, "unvalidated create with inconsistent sizes (x_len %llu, n %llu)",
                (unsigned long long)x_len, (unsigned long long)d.n);
  }
  if (d.lanes == 0) return fail(NDI_BAD_ARG, "lanes must be >= 1");
  if (d.n > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "more than %llu knots", (unsigned long long)MAX_KNOTS);
  if (!d.data) return fail(NDI_BAD_ARG, "null data pointer");
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
      c->dtype = dtype; c->device = d; c->lanes = lanes; c->nx = nx; c->ny = ny; c->hx = hx; c->hy = hy;
      c->dev = d; c->elanes = lanes; c->emode = this->emode; c->bnd = this->bnd;
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
  h->dtype = d.dtype;
  h->device = h->dev = d.device;
  h->emode = d.extrapolate ? EX_YES : EX_NO;
  h->nx = d.nx;
  h->ny = d.ny;
  h->lanes = h->elanes = d.lanes;
  h->hx = d.x ? half_images<F>(fetch_axis<uint16_t>(d.x, d.x_len, d.memspace)) : half_default_axis<F>(d.nx);
  h->hy = d.y ? half_images<F>(fetch_axis<uint16_t>(d.y, d.y_len, d.memspace)) : half_default_axis<F>(d.ny);
  const uint64_t x_len = d.x ? d.x_len : d.nx, y_len = d.y ? d.y_len : d.ny;
  if (d.validate) {
    ndi_status st = check_axes_2d<float>(h->hx.data(), x_len, h->hy.data(), y_len, d.nx, d.ny);
    if (st != NDI_OK) return st;
  } else if (x_len != d.nx || y_len != d.ny || d.nx < 2 || d.ny < 2) {
    return fail(NDI_BAD_ARG, "unvalidated create with inconsistent sizes");
  }
  if (d.lanes == 0) return fail(NDI_BAD_ARG, "lanes must be >= 1");
  if (d.nx > MAX_KNOTS || d.ny > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "too many knots");
  if (!d.data) return fail(NDI_BAD_ARG, "null data pointer");
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

// ---- sharded ----------------------------------------------------------------------------------------------------
// One host thread per shard, twice: every shard finds its first failure (pre-pass on its handle's device and stream),
// the minimum F is the serial loop's first failure, then every shard produces its rows below F -- into its output or
// through its ring.
template <int F, class Impl>
static ndi_status sharded_half(const std::vector<Impl*>& H, const void* qx, const void* qy, uint64_t nq,
                               const ndi_shard_io* io, uint64_t stride, const ndi_ring_desc* rings,
                               ndi_ring_consumer consume, void* user, const ndi_eval_opts& o, ndi_oob_info* info) {
  if (o.path == NDI_PATH_BUCKETED)
    return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED is not available for f16 / bf16 (AUTO / GATHER)");
  if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
  const uint32_t ns = (uint32_t)H.size();
  std::vector<uint64_t> lo(ns), hi(ns), fi(ns, NO_FAIL);
  std::vector<const void*> px(ns), py(ns);
  std::vector<const uint16_t*> dx(ns), dy(ns);
  for (uint32_t i = 0; i < ns; ++i) {
    shard_range(nq, i, ns, &lo[i], &hi[i]);
    const bool own = io && io[i].q;
    px[i] = own ? io[i].q : static_cast<const uint16_t*>(qx) + lo[i];
    py[i] = own ? io[i].qy : (qy ? static_cast<const uint16_t*>(qy) + lo[i] : nullptr);
  }
  std::vector<ndi_status> sst(ns, NDI_OK);
  std::vector<std::string> serr(ns);
  auto each = [&](const std::function<void(uint32_t)>& fn) {
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
  };
  ndi_status st = each([&](uint32_t i) {
    if (hi[i] == lo[i]) return;
    DeviceGuard dg(H[i]->dev);
    std::lock_guard<std::mutex> lk(H[i]->mu);
    fi[i] = H[i]->first_fail(px[i], py[i], hi[i] - lo[i], o.q_memspace, (hipStream_t)(io ? io[i].stream : nullptr),
                             &dx[i], &dy[i]);
  });
  if (st != NDI_OK) return st;
  uint64_t F_ = NO_FAIL;
  for (uint32_t i = 0; i < ns; ++i)
    if (fi[i] != NO_FAIL) F_ = std::min<uint64_t>(F_, lo[i] + fi[i]);
  if (rings)
    for (uint32_t i = 0; i < ns; ++i) {
      uint64_t rs = 0;
      if (const ndi_status rst = check_ring_desc(&rings[i], H[i]->elanes, &rs); rst != NDI_OK) return rst;
    }
  st = each([&](uint32_t i) {
    const uint64_t end = std::min<uint64_t>(hi[i], F_);
    if (end <= lo[i]) return;
    DeviceGuard dg(H[i]->dev);
    std::lock_guard<std::mutex> lk(H[i]->mu);
    hipStream_t s = (hipStream_t)(io ? io[i].stream : nullptr);
    const uint64_t rows = end - lo[i];
    if (rings) {
      uint64_t rs = 0;
      check_ring_desc(&rings[i], H[i]->elanes, &rs);
      H[i]->ring_rows(dx[i], dy[i], rows, &rings[i], rs, consume, user, s, lo[i], i);
    } else if (o.out_memspace == NDI_MEM_DEVICE) {
      H[i]->launch_eval(dx[i], dy[i], rows, static_cast<uint16_t*>(io[i].out), stride, s, false, nullptr, nullptr);
      NDI_HIP(hipStreamSynchronize(s));
    } else {
      HalfScratch& W = H[i]->ws(s);
      W.out.reserve(rows * H[i]->elanes * sizeof(uint16_t));
      H[i]->launch_eval(dx[i], dy[i], rows, W.out.as<uint16_t>(), H[i]->elanes, s, false, nullptr, nullptr);
      NDI_HIP(hipMemcpy2DAsync(io[i].out, stride * sizeof(uint16_t), W.out.p, H[i]->elanes * sizeof(uint16_t),
                               H[i]->elanes * sizeof(uint16_t), rows, hipMemcpyDeviceToHost, s));
      NDI_HIP(hipStreamSynchronize(s));
    }
  });
  if (st != NDI_OK) return st;
  if (F_ >= nq) return NDI_OK;
  uint32_t owner = 0;
  while (owner + 1 < ns && F_ >= hi[owner]) ++owner;
  DeviceGuard dg(H[owner]->dev);
  return H[owner]->diagnose(px[owner], py[owner], F_ - lo[owner], o.q_memspace, F_, info);
}
