// csrc/narrow_host.hpp -- the host engine shared by the i32 / i64 handles (int_host.hpp) and the f16 / bf16 handles
// (half_host.hpp); included by ndinterp_api.hip inside namespace ndi, before those two.
//
// E is the element's storage type (int32_t, int64_t; uint16_t for the halves' bit patterns).  The engine owns what the
// two families do alike: the handle state, staging of host queries, the first-failure word, the copy of staged rows
// back to a strided host buffer, the ring loop, the common checks of an evaluation, trim, and the sharded call.  A
// family supplies its kernels (launch_check, launch_rows), where its scratch lives (ws), how it names a failing query
// (diagnose) and how the shards of a sharded call run (each_shard).  What the families do differently is listed in
// DESIGN.md 4.9a.

struct NarrowScratch {
  DevBuf qx, qy, out, word;   // staged queries, the host-output bounce buffer, the first-failure word
  void release() {
    qx.release();
    qy.release();
    out.release();
    word.release();
  }
};

template <class E>
struct NarrowEngine {
  using Elem = E;
  int dev = 0, emode = EX_NO;
  uint64_t elanes = 0;
  std::mutex mu;   // serialises the calls on one handle
  OwnedRing ring_own;

  virtual ~NarrowEngine() = default;
  virtual NarrowScratch& ws(hipStream_t s) = 0;
  virtual void release_scratch() = 0;
  virtual const char* bucketed_refusal() const = 0;
  // the write-free check pass: the lowest failing query of the block goes to *w
  virtual void launch_check(const E* dx, const E* dy, uint64_t nq, hipStream_t s, unsigned long long* w) = 0;
  // evaluate these rows, unchecked
  virtual void launch_rows(const E* dx, const E* dy, uint64_t cnt, E* out, uint64_t stride, hipStream_t s) = 0;
  // the failing query j of a block alone, on the host; index: its flat index in the caller's batch
  virtual ndi_status diagnose(const void* qx, const void* qy, uint64_t j, int qmem, uint64_t index,
                              ndi_oob_info* info) = 0;
  // fn(i) for every shard of a sharded call whose first handle this is
  virtual ndi_status each_shard(uint32_t ns, const std::function<void(uint32_t)>& fn) = 0;

  const E* stage(const void* q, uint64_t nq, int memspace, DevBuf& buf, hipStream_t s) {
    if (!q || memspace == NDI_MEM_DEVICE) return static_cast<const E*>(q);
    buf.reserve(nq * sizeof(E));
    NDI_HIP(hipMemcpyAsync(buf.p, q, nq * sizeof(E), hipMemcpyHostToDevice, s));
    return buf.as<E>();
  }
  unsigned long long* reset_word(NarrowScratch& W, hipStream_t s) {
    W.word.reserve(sizeof(unsigned long long));
    NDI_HIP(hipMemsetAsync(W.word.p, 0xff, sizeof(unsigned long long), s));
    return W.word.as<unsigned long long>();
  }
  uint64_t read_word(NarrowScratch& W, hipStream_t s) {
    unsigned long long f = NO_FAIL;
    NDI_HIP(hipMemcpyAsync(&f, W.word.p, sizeof(f), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    return f;
  }
  // Query j (x, and y if there is one) from host or device memory.
  void fetch_query(const void* qx, const void* qy, uint64_t j, int qmem, E* x, E* y) {
    if (qmem == NDI_MEM_DEVICE) {
      NDI_HIP(hipMemcpy(x, static_cast<const E*>(qx) + j, sizeof(E), hipMemcpyDeviceToHost));
      if (qy) NDI_HIP(hipMemcpy(y, static_cast<const E*>(qy) + j, sizeof(E), hipMemcpyDeviceToHost));
    } else {
      *x = static_cast<const E*>(qx)[j];
      if (qy) *y = static_cast<const E*>(qy)[j];
    }
  }
  // Staged rows (elanes apart) back to the caller's host buffer (stride apart).
  void rows_to_host(void* out, uint64_t stride, const DevBuf& staged, uint64_t rows, hipStream_t s) {
    if (rows == 0) return;
    NDI_HIP(hipMemcpy2DAsync(out, stride * sizeof(E), staged.p, elanes * sizeof(E), elanes * sizeof(E), rows,
                             hipMemcpyDeviceToHost, s));
  }

  // Lowest failing query of [0, nq) (NO_FAIL if none); queries already on the device.
  uint64_t first_fail(const E* dx, const E* dy, uint64_t nq, NarrowScratch& W, hipStream_t s) {
    unsigned long long* w = reset_word(W, s);
    launch_check(dx, dy, nq, s, w);
    NDI_HIP(hipGetLastError());
    return read_word(W, s);
  }
  // Rows [0, rows) of out, every query valid; host outputs are staged and copied back row by row (stride kept).
  void eval_rows(const E* dx, const E* dy, uint64_t rows, void* out, uint64_t stride, int omem, NarrowScratch& W,
                 hipStream_t s) {
    if (rows == 0) return;
    if (omem == NDI_MEM_DEVICE) {
      launch_rows(dx, dy, rows, static_cast<E*>(out), stride, s);
      NDI_HIP(hipGetLastError());
      return;
    }
    W.out.reserve(rows * elanes * sizeof(E));
    launch_rows(dx, dy, rows, W.out.as<E>(), elanes, s);
    NDI_HIP(hipGetLastError());
    rows_to_host(out, stride, W.out, rows, s);
  }

  // What every ndi_interp{1,2}d_eval checks before it touches the device.
  ndi_status run_head(const ndi_eval_opts* opts, ndi_eval_opts& o, const void* qx, const void* out, uint64_t nq,
                      uint64_t stride, ndi_oob_info* info) {
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED) return fail(NDI_UNSUPPORTED, "%s", bucketed_refusal());
    if (stride < elanes)
      return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)stride,
                  (unsigned long long)elanes);
    if (nq && (!qx || !out)) return fail(NDI_BAD_ARG, "null query or output pointer");
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    return NDI_OK;
  }

  // Rows [0, rows) through a device-output ring (rows already cut at the first failure).  q_begin: flat index of dx[0]
  // in the caller's batch; shard: reported in every chunk.
  void ring_rows(const E* dx, const E* dy, uint64_t rows, const ndi_ring_desc* ring, uint64_t stride,
                 ndi_ring_consumer consume, void* user, hipStream_t s, uint64_t q_begin, uint32_t shard) {
    const uint32_t ns = ring->n_slots;
    std::vector<E*> slots(ns);
    uint64_t rstride = stride;
    std::unique_lock<std::mutex> rl(ring_own.mu, std::defer_lock);
    if (ring->slots) {
      for (uint32_t i = 0; i < ns; ++i) slots[i] = static_cast<E*>(ring->slots[i]);
    } else {   // library-owned: one allocation, slots interleaved row by row (ndinterp.h)
      rl.lock();
      rstride = (uint64_t)ns * stride;
      ring_own.ensure(1, ring->chunk_queries, rstride * sizeof(E));
      for (uint32_t i = 0; i < ns; ++i) slots[i] = ring_own.buf.as<E>() + (uint64_t)i * stride;
    }
    std::vector<hipEvent_t> waits(ns, nullptr);
    uint64_t k = 0;
    for (uint64_t b = 0; b < rows; b += ring->chunk_queries, ++k) {
      const uint64_t cnt = std::min<uint64_t>(ring->chunk_queries, rows - b);
      const uint32_t slot = (uint32_t)(k % ns);
      if (waits[slot]) NDI_HIP(hipStreamWaitEvent(s, waits[slot], 0));
      waits[slot] = nullptr;
      launch_rows(dx + b, dy ? dy + b : nullptr, cnt, slots[slot], rstride, s);
      NDI_HIP(hipGetLastError());
      ndi_ring_chunk c{k, q_begin + b, cnt, slots[slot], rstride, slot, shard, (void*)s};
      waits[slot] = consume ? (hipEvent_t)consume(user, &c) : nullptr;
    }
    NDI_HIP(hipStreamSynchronize(s));
  }

  // ndi_interp{1,2}d_eval_ring: the check pass, then the rows below the first failure chunk by chunk.
  ndi_status run_ring(const void* qx, const void* qy, uint64_t nq, const ndi_ring_desc* ring,
                      ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts, ndi_oob_info* info) {
    ndi_eval_opts o{};
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED) return fail(NDI_UNSUPPORTED, "%s", bucketed_refusal());
    uint64_t stride = 0;
    if (const ndi_status rs = check_ring_desc(ring, elanes, &stride); rs != NDI_OK) return rs;
    if (nq && !qx) return fail(NDI_BAD_ARG, "null query pointer");
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    if (nq == 0) return NDI_OK;
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    hipStream_t s = (hipStream_t)o.stream;
    NarrowScratch& W = ws(s);
    const E* dx = stage(qx, nq, o.q_memspace, W.qx, s);
    const E* dy = stage(qy, nq, o.q_memspace, W.qy, s);
    const uint64_t F = first_fail(dx, dy, nq, W, s);
    ring_rows(dx, dy, std::min<uint64_t>(F, nq), ring, stride, consume, user, s, 0, 0);
    return F < nq ? diagnose(qx, qy, F, o.q_memspace, F, info) : NDI_OK;
  }

  ndi_status trim_impl() {
    DeviceGuard dg(dev);
    std::lock_guard<std::mutex> lk(mu);
    std::lock_guard<std::mutex> rl(ring_own.mu);
    release_scratch();
    ring_own.clear();
    return NDI_OK;
  }
};

// The fields a create and a clone set alike on a handle (Impl: an Interp{1,2}DBase that is a NarrowEngine).
template <class Impl>
static void set_scalars(Impl& h, int dtype, int device, int mode, uint64_t lanes) {
  h.dtype = dtype;
  h.device = h.dev = device;
  h.lanes = h.elanes = lanes;
  h.emode = mode;
}

// ---- sharded --------------------------------------------------------------------------------------------------------
// Every shard finds the first failure of its block (check pass on its handle's device and stream), the minimum F is the
// serial loop's first failure, then every shard produces its rows below F -- into its output or through its ring --
// from the queries it staged for the check.  (The rings have been validated by the entry point, and no two shards
// share a handle, so a shard's staged queries are still there.)  How the shards run -- one after the other on the
// calling thread, or a host thread each -- is the family's each_shard.
template <class E>
static ndi_status sharded_narrow(const std::vector<NarrowEngine<E>*>& H, const ShardCall& c, ndi_oob_info* info) {
  if (c.o.path == NDI_PATH_BUCKETED) return fail(NDI_UNSUPPORTED, "%s", H[0]->bucketed_refusal());
  if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
  const uint32_t ns = (uint32_t)H.size();
  std::vector<uint64_t> lo(ns), hi(ns), fi(ns, NO_FAIL);
  std::vector<const void*> px(ns), py(ns);
  std::vector<const E*> dx(ns), dy(ns);
  for (uint32_t i = 0; i < ns; ++i) {
    shard_range(c.nq, i, ns, &lo[i], &hi[i]);
    const bool own = c.io && c.io[i].q;
    px[i] = own ? c.io[i].q : static_cast<const E*>(c.qx) + lo[i];
    py[i] = own ? c.io[i].qy : (c.qy ? static_cast<const E*>(c.qy) + lo[i] : nullptr);
  }
  auto stream = [&](uint32_t i) { return (hipStream_t)(c.io ? c.io[i].stream : nullptr); };
  ndi_status st = H[0]->each_shard(ns, [&](uint32_t i) {
    if (hi[i] == lo[i]) return;
    DeviceGuard dg(H[i]->dev);
    std::lock_guard<std::mutex> lk(H[i]->mu);
    hipStream_t s = stream(i);
    NarrowScratch& W = H[i]->ws(s);
    dx[i] = H[i]->stage(px[i], hi[i] - lo[i], c.o.q_memspace, W.qx, s);
    dy[i] = H[i]->stage(py[i], hi[i] - lo[i], c.o.q_memspace, W.qy, s);
    fi[i] = H[i]->first_fail(dx[i], dy[i], hi[i] - lo[i], W, s);
  });
  if (st != NDI_OK) return st;
  uint64_t F = NO_FAIL;
  for (uint32_t i = 0; i < ns; ++i)
    if (fi[i] != NO_FAIL) F = std::min<uint64_t>(F, lo[i] + fi[i]);
  st = H[0]->each_shard(ns, [&](uint32_t i) {
    const uint64_t end = std::min<uint64_t>(hi[i], F);
    if (end <= lo[i]) return;
    DeviceGuard dg(H[i]->dev);
    std::lock_guard<std::mutex> lk(H[i]->mu);
    hipStream_t s = stream(i);
    if (c.rings) {
      uint64_t rs = 0;
      (void)check_ring_desc(&c.rings[i], H[i]->elanes, &rs);   // validated by the entry point: the stride is wanted
      H[i]->ring_rows(dx[i], dy[i], end - lo[i], &c.rings[i], rs, c.consume, c.user, s, lo[i], i);
    } else {
      H[i]->eval_rows(dx[i], dy[i], end - lo[i], c.io[i].out, c.out_stride, c.o.out_memspace, H[i]->ws(s), s);
      NDI_HIP(hipStreamSynchronize(s));
    }
  });
  if (st != NDI_OK) return st;
  if (F >= c.nq) return NDI_OK;
  uint32_t owner = 0;
  while (owner + 1 < ns && F >= hi[owner]) ++owner;
  DeviceGuard dg(H[owner]->dev);
  return H[owner]->diagnose(px[owner], py[owner], F - lo[owner], c.o.q_memspace, F, info);
}
