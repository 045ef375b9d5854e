// csrc/int_host.hpp -- host side of the i32 / i64 Linear and Bilinear handles (included by ndinterp_api.hip inside
// namespace ndi, after the float handles; kernels in int_kernels.hpp).
//
// One engine serves every entry point of an integer handle:
//   first_fail   lowest failing query of a block (1-D: the query-only pre-pass; 2-D: the write-free check pass)
//   eval_rows    rows that are known to be valid (no checks)
//   run          ndi_interp{1,2}d_eval: caller-owned buffers take first_fail + eval_rows over [0, F); fresh /
//                unspecified-rows outputs take the fused pass
//   diagnose     the failing query alone, on the host, in the reference's order (generic_host.calc_frac): which
//                range test or which operation of which lane failed first
// Calls on one handle are serialised by its mutex (the staging buffers are the handle's).  async_launch is accepted and
// completes inside the call; ndi_interp{1,2}d_finish then reports that batch's status.

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
  static const int env = [] { const char* e = std::getenv("NDI_INT_MAP"); return e ? std::atoi(e) : 0; }();
  if (env == 1) return false;
  if (env == 2) return true;
  return lanes > 32;
}

template <class T>
struct IntEngine {
  int dev = 0, emode = EX_NO;
  uint64_t elanes = 0;
  std::mutex mu;
  DevBuf qx_buf, qy_buf, out_buf, word;
  OwnedRing ring_own;
  std::map<void*, std::pair<ndi_status, ndi_oob_info>> pending;   // async_launch batches awaiting finish, per stream
  std::string pending_err;

  virtual ~IntEngine() = default;
  virtual void launch_check(const T* qx, const T* qy, uint64_t nq, hipStream_t s, unsigned long long* w) = 0;
  virtual void launch_eval(const T* qx, const T* qy, uint64_t nq, T* out, uint64_t stride, hipStream_t s,
                           bool check, unsigned long long* w) = 0;
  virtual ndi_status diagnose_at(T x, T y, ndi_oob_info* info) = 0;

  const T* stage(const void* q, uint64_t nq, int memspace, DevBuf& buf, hipStream_t s) {
    if (!q || memspace == NDI_MEM_DEVICE) return static_cast<const T*>(q);
    buf.reserve(nq * sizeof(T));
    NDI_HIP(hipMemcpyAsync(buf.p, q, nq * sizeof(T), hipMemcpyHostToDevice, s));
    return buf.as<T>();
  }
  unsigned long long* reset_word(hipStream_t s) {
    word.reserve(sizeof(unsigned long long));
    NDI_HIP(hipMemsetAsync(word.p, 0xff, sizeof(unsigned long long), s));
    return word.as<unsigned long long>();
  }
  uint64_t read_word(hipStream_t s) {
    unsigned long long f = NO_FAIL;
    NDI_HIP(hipMemcpyAsync(&f, word.p, sizeof(f), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    return f;
  }

  // Lowest failing query of [0, nq) (NO_FAIL if none); queries already on the device.
  uint64_t first_fail_dev(const T* qx, const T* qy, uint64_t nq, hipStream_t s) {
    unsigned long long* w = reset_word(s);
    launch_check(qx, qy, nq, s, w);
    NDI_HIP(hipGetLastError());
    return read_word(s);
  }
  uint64_t first_fail(const void* qx, const void* qy, uint64_t nq, int qmem, hipStream_t s) {
    const T* dx = stage(qx, nq, qmem, qx_buf, s);
    const T* dy = stage(qy, nq, qmem, qy_buf, s);
    return first_fail_dev(dx, dy, nq, s);
  }

  // Rows [0, rows) of out, every query valid; host outputs are staged and copied back row by row (stride kept).
  void eval_rows(const void* qx, const void* qy, uint64_t rows, void* out, uint64_t stride, int qmem, int omem,
                 hipStream_t s) {
    if (rows == 0) return;
    const T* dx = stage(qx, rows, qmem, qx_buf, s);
    const T* dy = stage(qy, rows, qmem, qy_buf, s);
    if (omem == NDI_MEM_DEVICE) {
      launch_eval(dx, dy, rows, static_cast<T*>(out), stride, s, false, nullptr);
      NDI_HIP(hipGetLastError());
      return;
    }
    out_buf.reserve(rows * elanes * sizeof(T));
    launch_eval(dx, dy, rows, out_buf.as<T>(), elanes, s, false, nullptr);
    NDI_HIP(hipGetLastError());
    NDI_HIP(hipMemcpy2DAsync(out, stride * sizeof(T), out_buf.p, elanes * sizeof(T), elanes * sizeof(T), rows,
                             hipMemcpyDeviceToHost, s));
  }

  // The failing query j alone: its x (and y) fetched, the reference's checks replayed in order.
  ndi_status diagnose(const void* qx, const void* qy, uint64_t j, int qmem, uint64_t index, ndi_oob_info* info) {
    T x = 0, y = 0;
    if (qmem == NDI_MEM_DEVICE) {
      NDI_HIP(hipMemcpy(&x, static_cast<const T*>(qx) + j, sizeof(T), hipMemcpyDeviceToHost));
      if (qy) NDI_HIP(hipMemcpy(&y, static_cast<const T*>(qy) + j, sizeof(T), hipMemcpyDeviceToHost));
    } else {
      x = static_cast<const T*>(qx)[j];
      if (qy) y = static_cast<const T*>(qy)[j];
    }
    ndi_oob_info tmp{};
    if (!info) info = &tmp;
    ndi_status st = diagnose_at(x, y, info);
    info->index = index;
    return st;
  }

  ndi_status run(const void* qx, const void* qy, uint64_t nq, void* out, uint64_t stride, const ndi_eval_opts* opts,
                 ndi_oob_info* info) {
    ndi_eval_opts o{};
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED is not available for integer element types (AUTO / GATHER)");
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
      const T* dx = stage(qx, nq, o.q_memspace, qx_buf, s);
      const T* dy = stage(qy, nq, o.q_memspace, qy_buf, s);
      uint64_t F;
      if (o.flags & NDI_EVAL_FRESH_OUTPUT) {   // fused: rows at / after the failure may be written
        T* od = static_cast<T*>(out);
        uint64_t ost = stride;
        if (o.out_memspace != NDI_MEM_DEVICE) {
          out_buf.reserve(nq * elanes * sizeof(T));
          od = out_buf.as<T>();
          ost = elanes;
        }
        unsigned long long* w = reset_word(s);
        launch_eval(dx, dy, nq, od, ost, s, true, w);
        NDI_HIP(hipGetLastError());
        F = read_word(s);
        const uint64_t rows = std::min<uint64_t>(F, nq);
        if (o.out_memspace != NDI_MEM_DEVICE && rows)
          NDI_HIP(hipMemcpy2DAsync(out, stride * sizeof(T), out_buf.p, elanes * sizeof(T), elanes * sizeof(T), rows,
                                   hipMemcpyDeviceToHost, s));
      } else {
        F = first_fail_dev(dx, dy, nq, s);
        const uint64_t rows = std::min<uint64_t>(F, nq);
        if (rows) {
          if (o.out_memspace == NDI_MEM_DEVICE) {
            launch_eval(dx, dy, rows, static_cast<T*>(out), stride, s, false, nullptr);
            NDI_HIP(hipGetLastError());
          } else {
            out_buf.reserve(rows * elanes * sizeof(T));
            launch_eval(dx, dy, rows, out_buf.as<T>(), elanes, s, false, nullptr);
            NDI_HIP(hipGetLastError());
            NDI_HIP(hipMemcpy2DAsync(out, stride * sizeof(T), out_buf.p, elanes * sizeof(T), elanes * sizeof(T), rows,
                                     hipMemcpyDeviceToHost, s));
          }
        }
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
    std::lock_guard<std::mutex> lk(mu);
    auto it = pending.find(stream);
    if (it == pending.end()) return NDI_OK;
    const ndi_status st = it->second.first;
    if (info) *info = it->second.second;
    pending.erase(it);
    if (st != NDI_OK) tls_error() = pending_err;
    return st;
  }

  // Rows [0, rows) through a device-output ring (rows already cut at the first failure).  q_begin: flat index of qx[0]
  // in the caller's batch; shard: reported in every chunk.
  void ring_rows(const T* dx, const T* dy, uint64_t rows, const ndi_ring_desc* ring, uint64_t stride,
                 ndi_ring_consumer consume, void* user, hipStream_t s, uint64_t q_begin, uint32_t shard) {
    const uint32_t ns = ring->n_slots;
    std::vector<T*> slots(ns);
    uint64_t rstride = stride;
    std::unique_lock<std::mutex> rl(ring_own.mu, std::defer_lock);
    if (ring->slots) {
      for (uint32_t i = 0; i < ns; ++i) slots[i] = static_cast<T*>(ring->slots[i]);
    } else {   // library-owned: one allocation, slots interleaved row by row (ndinterp.h)
      rl.lock();
      rstride = (uint64_t)ns * stride;
      ring_own.ensure(1, ring->chunk_queries, rstride * sizeof(T));
      for (uint32_t i = 0; i < ns; ++i) slots[i] = ring_own.buf.as<T>() + (uint64_t)i * stride;
    }
    std::vector<hipEvent_t> waits(ns, nullptr);
    uint64_t k = 0;
    for (uint64_t b = 0; b < rows; b += ring->chunk_queries, ++k) {
      const uint64_t cnt = std::min<uint64_t>(ring->chunk_queries, rows - b);
      const uint32_t slot = (uint32_t)(k % ns);
      if (waits[slot]) NDI_HIP(hipStreamWaitEvent(s, waits[slot], 0));
      waits[slot] = nullptr;
      launch_eval(dx + b, dy ? dy + b : nullptr, cnt, slots[slot], rstride, s, false, nullptr);
      NDI_HIP(hipGetLastError());
      ndi_ring_chunk c{k, q_begin + b, cnt, slots[slot], rstride, slot, shard, (void*)s};
      waits[slot] = consume ? (hipEvent_t)consume(user, &c) : nullptr;
    }
    NDI_HIP(hipStreamSynchronize(s));
  }

  ndi_status run_ring(const void* qx, const void* qy, uint64_t nq, const ndi_ring_desc* ring,
                      ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts, ndi_oob_info* info) {
    ndi_eval_opts o{};
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED is not available for integer element types (AUTO / GATHER)");
    uint64_t stride = 0;
    if (const ndi_status rs = check_ring_desc(ring, elanes, &stride); rs != NDI_OK) return rs;
    if (nq && !qx) return fail(NDI_BAD_ARG, "null query pointer");
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    if (nq == 0) return NDI_OK;
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t s = (hipStream_t)o.stream;
    const T* dx = stage(qx, nq, o.q_memspace, qx_buf, s);
    const T* dy = stage(qy, nq, o.q_memspace, qy_buf, s);
    const uint64_t F = first_fail_dev(dx, dy, nq, s);
    ring_rows(dx, dy, std::min<uint64_t>(F, nq), ring, stride, consume, user, s, 0, 0);
    return F < nq ? diagnose(qx, qy, F, o.q_memspace, F, info) : NDI_OK;
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
      if (op >= 0) {
        static const char* const names[4] = {"subtract", "multiply", "add", "divide"};
        info->axis = op;
        info->status = NDI_INT_OVERFLOW;
        return fail(NDI_INT_OVERFLOW, "attempt to %s with overflow", names[op]);
      }
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
  ndi_status trim() override {
    DeviceGuard dg(device);
    std::lock_guard<std::mutex> lk(this->mu);
    std::lock_guard<std::mutex> rl(this->ring_own.mu);
    this->qx_buf.release();
    this->qy_buf.release();
    this->out_buf.release();
    this->ring_own.clear();
    return NDI_OK;
  }
  uint64_t scratch_sets() override { return this->out_buf.p || this->qx_buf.p ? 1 : 0; }

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
      c->dtype = dtype; c->device = d; c->lanes = lanes; c->n = n; c->hx = hx;
      c->dev = d; c->elanes = lanes; c->emode = this->emode;
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
  h->dtype = d.dtype;
  h->device = h->dev = d.device;
  h->emode = d.extrapolate ? EX_YES : EX_NO;
  h->n = d.n;
  h->lanes = h->elanes = d.lanes;
  h->hx = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.n);
  const uint64_t x_len = d.x ? d.x_len : d.n;
  if (d.validate) {
    ndi_status st = check_axis_1d<T>(h->hx.data(), x_len, d.n, d.strategy);
    if (st != NDI_OK) return st;
  } else if (x_len != d.n || d.n < 2) {
    return fail(NDI_BAD_ARG, "unvalidated create with inconsistent sizes (x_len %llu, n %llu)",
                (unsigned long long)x_len, (unsigned long long)d.n);
  }
  if (d.lanes == 0) return fail(NDI_BAD_ARG, "lanes must be >= 1");
  if (d.n > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "more than %llu knots", (unsigned long long)MAX_KNOTS);
  if (!d.data) return fail(NDI_BAD_ARG, "null data pointer");
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
      if (op >= 0) {
        static const char* const names[4] = {"subtract", "multiply", "add", "divide"};
        info->axis = op;
        info->status = NDI_INT_OVERFLOW;
        return fail(NDI_INT_OVERFLOW, "attempt to %s with overflow", names[op]);
      }
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
  ndi_status trim() override {
    DeviceGuard dg(device);
    std::lock_guard<std::mutex> lk(this->mu);
    std::lock_guard<std::mutex> rl(this->ring_own.mu);
    this->qx_buf.release();
    this->qy_buf.release();
    this->out_buf.release();
    this->ring_own.clear();
    return NDI_OK;
  }
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
      c->dtype = dtype; c->device = d; c->lanes = lanes; c->nx = nx; c->ny = ny; c->hx = hx; c->hy = hy;
      c->dev = d; c->elanes = lanes; c->emode = this->emode;
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
  h->dtype = d.dtype;
  h->device = h->dev = d.device;
  h->emode = d.extrapolate ? EX_YES : EX_NO;
  h->nx = d.nx;
  h->ny = d.ny;
  h->lanes = h->elanes = d.lanes;
  h->hx = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.nx);
  h->hy = d.y ? fetch_axis<T>(d.y, d.y_len, d.memspace) : default_axis<T>(d.ny);
  const uint64_t x_len = d.x ? d.x_len : d.nx, y_len = d.y ? d.y_len : d.ny;
  if (d.validate) {
    ndi_status st = check_axes_2d<T>(h->hx.data(), x_len, h->hy.data(), y_len, d.nx, d.ny);
    if (st != NDI_OK) return st;
  } else if (x_len != d.nx || y_len != d.ny || d.nx < 2 || d.ny < 2) {
    return fail(NDI_BAD_ARG, "unvalidated create with inconsistent sizes");
  }
  if (d.lanes == 0) return fail(NDI_BAD_ARG, "lanes must be >= 1");
  if (d.nx > MAX_KNOTS || d.ny > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "too many knots");
  if (!d.data) return fail(NDI_BAD_ARG, "null data pointer");
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

// ---- sharded ----------------------------------------------------------------------------------------------------
// The shards' first failures are found block by block (each on its handle's device and stream), the minimum F is the
// serial loop's first failure, then every shard produces its rows below F -- into its output or through its ring.
template <class T, class Impl>
static ndi_status sharded_int(const std::vector<Impl*>& H, const void* qx, const void* qy, uint64_t nq,
                              const ndi_shard_io* io, uint64_t stride, const ndi_ring_desc* rings,
                              ndi_ring_consumer consume, void* user, const ndi_eval_opts& o, ndi_oob_info* info) {
  if (o.path == NDI_PATH_BUCKETED)
    return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED is not available for integer element types (AUTO / GATHER)");
  if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
  const uint32_t ns = (uint32_t)H.size();
  std::vector<uint64_t> lo(ns), hi(ns);
  std::vector<const T*> px(ns), py(ns);
  uint64_t F = NO_FAIL;
  for (uint32_t i = 0; i < ns; ++i) {
    shard_range(nq, i, ns, &lo[i], &hi[i]);
    const bool own = io && io[i].q;
    px[i] = own ? static_cast<const T*>(io[i].q) : static_cast<const T*>(qx) + lo[i];
    py[i] = own ? static_cast<const T*>(io[i].qy) : (qy ? static_cast<const T*>(qy) + lo[i] : nullptr);
  }
  for (uint32_t i = 0; i < ns; ++i) {
    if (hi[i] == lo[i]) continue;
    DeviceGuard dg(H[i]->dev);
    std::lock_guard<std::mutex> lk(H[i]->mu);
    const uint64_t f = H[i]->first_fail(px[i], py[i], hi[i] - lo[i], o.q_memspace, (hipStream_t)(io ? io[i].stream : nullptr));
    if (f != NO_FAIL) F = std::min<uint64_t>(F, lo[i] + f);
  }
  for (uint32_t i = 0; i < ns; ++i) {
    const uint64_t end = std::min<uint64_t>(hi[i], F);
    if (end <= lo[i]) continue;
    DeviceGuard dg(H[i]->dev);
    std::lock_guard<std::mutex> lk(H[i]->mu);
    hipStream_t s = (hipStream_t)(io ? io[i].stream : nullptr);
    if (rings) {
      uint64_t rs = 0;
      if (const ndi_status st = check_ring_desc(&rings[i], H[i]->elanes, &rs); st != NDI_OK) return st;
      const T* dx = H[i]->stage(px[i], end - lo[i], o.q_memspace, H[i]->qx_buf, s);
      const T* dy = H[i]->stage(py[i], end - lo[i], o.q_memspace, H[i]->qy_buf, s);
      H[i]->ring_rows(dx, dy, end - lo[i], &rings[i], rs, consume, user, s, lo[i], i);
    } else {
      H[i]->eval_rows(px[i], py[i], end - lo[i], io[i].out, stride, o.q_memspace, o.out_memspace, s);
      NDI_HIP(hipStreamSynchronize(s));
    }
  }
  if (F >= nq) return NDI_OK;
  uint32_t owner = 0;
  while (owner + 1 < ns && F >= hi[owner]) ++owner;
  DeviceGuard dg(H[owner]->dev);
  return H[owner]->diagnose(px[owner], py[owner], F - lo[owner], o.q_memspace, F, info);
}
