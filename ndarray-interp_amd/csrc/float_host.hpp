// csrc/float_host.hpp -- the host engine shared by the f32 / f64 handles: Interp1DImpl and Interp2DImpl
// (ndinterp_api.hip) and AntiderivImpl (antiderivative_host.hpp); included by ndinterp_api.hip inside namespace ndi,
// behind Workspace / SpaceSet / OwnedRing and before those three.
//
// The engine owns what the three families do alike whether a batch carries one query array or two: the first-error
// report, the status read-back, staging of host queries, the range pre-pass, the host-output chunk loop, the shells of
// the two small-row paths, the entry sequences of eval / finish / eval_ring, the two-stream ring pipeline and the front
// of trim.  A family (Impl, the CRTP parameter) supplies
//   device, lanes, mode, spaces        its state (and ring_own where it has a ring)
//   query_arrays                       1 or 2: how many query arrays eval / eval_ring take
//   small_rows, ring                   whether it has the small-row paths / the ring evaluation
//   axis_name(axis)                    the letter a failure on that array is reported with
//   enqueue(s, ws, q, nq, out, stride, path, flags)   one batch on device pointers through scratch set 0
// and, where it has them,
//   range_limits(lim)                  {lo, hi} of either axis for the range pre-pass
//   small_rows_fit() / zero_copy_fits(nq, q_space, out_space) / small_begin() / launch_small(s, st, q, out, nq)
//   Plan, prep(s, sc, q, ...), launch_eval(s, sc, P)   the two stages of a ring chunk
//   ring_groups = true, groupable(P), launch_eval_group(s, sets, plans, w)   one evaluation launch for w ring chunks
// The sharded call of these handles (Job / Shard / sharded_float) is written once too, beside run_shards in
// ndinterp_api.hip, whose worker pool it needs.  What the families do differently is listed in DESIGN.md 4.9b.  This is not NarrowEngine (narrow_host.hpp): that one
// serialises a handle's calls on a mutex and owns one scratch set; this one takes a per-stream workspace lease with a
// side stream and an asynchronous status.

// The query arrays of one batch: `a` alone (1-D; an antiderivative's eval) or `a` and `b` (2-D: x, y; integrate: lo, hi).
template <class T>
struct Queries {
  const T* a = nullptr;
  const T* b = nullptr;
  int count() const { return b ? 2 : 1; }
  Queries operator+(uint64_t off) const { return {a + off, b ? b + off : nullptr}; }
};

// The lowest failing query index per array of the batch whose status block has just been read back.
struct FirstFail {
  unsigned long long f0 = NO_FAIL, f1 = NO_FAIL;
  unsigned long long first() const { return std::min(f0, f1); }
  template <class T>
  static FirstFail of(const Workspace& ws, Queries<T> q) {
    return {ws.host_status->first_fail[0], q.b ? ws.host_status->first_fail[1] : NO_FAIL};
  }
};

constexpr size_t ZERO_COPY_LIMIT = 1u << 20;   // the zero-copy path: queries + rows of a batch, in bytes

// The state of a ring evaluation between ring_begin and ring_produce.
template <class Plan>
struct RingRun {
  std::unique_lock<std::mutex> own;
  std::vector<void*> slots;
  uint64_t pitch = 0, chunk = 0;
  uint32_t n_slots = 0;
  uint32_t wmax = 1;         // chunks per evaluation launch, at most (1: the family or NDI_RING_GROUP has no groups)
  bool narrow_first = false; // chunk 0 is launched alone (NDI_RING_GROUP=2)
  uint32_t n_sets = 2;       // scratch sets in use: chunk k lives in set k % n_sets
  uint64_t prepped = 0;      // chunks [0, prepped) were located + grouped by ring_begin
  std::vector<Plan> plans;   // the plan of the chunk in every set
  hipStream_t side = nullptr;
};

template <class T, class Impl>
struct FloatEngine {
  Impl& self() { return static_cast<Impl&>(*this); }

  // The reference's error for the batch whose lowest failing queries are q.a[f.f0] / q.b[f.f1] (reported as index_offset +
  // index); the first array is tested before the second for the same query (bilinear.rs:71-80).
  ndi_status report(Queries<T> q, int q_space, FirstFail f, uint64_t index_offset, ndi_oob_info* info) {
    const int axis = f.f0 <= f.f1 ? 0 : 1;
    const unsigned long long ff = axis ? f.f1 : f.f0;
    const T* src = axis ? q.b : q.a;
    T v;
    if (q_space == NDI_MEM_DEVICE) NDI_HIP(hipMemcpy(&v, src + ff, sizeof(T), hipMemcpyDeviceToHost));
    else v = src[ff];
    const ndi_status st = self().failure_status(v);
    if (info) {
      info->index = index_offset + ff;
      info->value = (double)v;
      info->axis = axis;
      info->status = st;
    }
    if (st == NDI_NAN_QUERY) return fail(st, "failed to convert NaN to usize (query %llu)", index_offset + ff);
    return fail(st, "%s = %.17g is not in range", self().axis_name(axis), (double)v);
  }

  // The status of a failing query v.  Without extrapolation every failure is a range failure (NaN included: "x = NaN is
  // not in range"); with it the only failure is the search meeting a NaN -- the query itself or an infinite query that
  // the periodic wrap turned into NaN (the reference panics: vector_extensions.rs:83-84).  (An inverse handle has its own.)
  ndi_status failure_status(T) { return (self().mode != EX_NO) ? NDI_NAN_QUERY : NDI_OUT_OF_BOUNDS; }

  // Reads the status block of the batch enqueued with scratch set 0 (the stream is idle afterwards) and converts it to
  // the reference's error, with the query pointers the batch was issued with.
  ndi_status collect(hipStream_t s, Workspace& ws, uint64_t index_offset, ndi_oob_info* info) {
    ws.ensure_status();
    NDI_HIP(hipMemcpyAsync(ws.host_status, ws.sc[0].status.p, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    ws.pending = false;
    const Queries<T> q{(const T*)ws.last_q, (const T*)ws.last_q2};
    const FirstFail f = FirstFail::of(ws, q);
    if (f.first() == NO_FAIL) return NDI_OK;
    return report(q, ws.last_q_space, f, index_offset, info);
  }

  ndi_status run_finish(void* stream, ndi_oob_info* info) {
    DeviceGuard dg(self().device);
    hipStream_t s = (hipStream_t)stream;
    SpaceLease lease(self().spaces, s);
    Workspace& ws = lease.ws;
    if (!ws.pending) {
      NDI_HIP(hipStreamSynchronize(s));
      return NDI_OK;
    }
    return collect(s, ws, 0, info);
  }

  // Host queries are uploaded once per call into the workspace, every array that is there; device pointers pass through.
  Queries<T> stage_queries(hipStream_t s, Workspace& ws, Queries<T> q, uint64_t nq, int q_space) {
    if (q_space != NDI_MEM_HOST) return q;
    auto upload = [&](DevBuf& buf, const T* src) -> const T* {
      if (!src) return nullptr;
      buf.reserve(nq * sizeof(T));
      NDI_HIP(hipMemcpyAsync(buf.p, src, nq * sizeof(T), hipMemcpyHostToDevice, s));
      return buf.as<T>();
    };
    const T* a = upload(ws.qdev, q.a);
    return {a, upload(ws.qdev2, q.b)};
  }

  // range_check_kernel over the one or two query arrays of a batch against the family's range_limits: the lowest failing
  // index per array into st->first_fail.
  void launch_range_check(hipStream_t s, StatusBlock* st, Queries<T> q, uint64_t nq) {
    T lim[4];
    self().range_limits(lim);
    const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + BLOCK - 1) / BLOCK, 4096));
    ProfScope ps(s, PC_LOCATE);
    hipLaunchKernelGGL(range_check_kernel<T>, dim3(g), dim3(BLOCK), 0, s, q.a, q.b, nq, lim[0], lim[1], lim[2], lim[3],
                       self().mode, &st->first_fail[0]);
    NDI_HIP(hipGetLastError());
    ps.done();
  }

  // The tail of every query-order plan: the path is recorded, and the range pre-pass the evaluation kernel relies on is
  // enqueued -- unless `in_kernel`: a fresh output (NDI_EVAL_FRESH_OUTPUT: the buffer is dropped on Err) needs no
  // pre-pass, the kernel's own range test reports the failure.  Returns in_kernel, the plan's l_check.  (The SMALL
  // plans always pre-check and pass false.)
  bool range_prepass(hipStream_t s, Scratch& sc, Queries<T> q, uint64_t nq, bool in_kernel) {
    g_last_path.store(NDI_PATH_GATHER);
    if (!in_kernel) self().launch_range_check(s, sc.status.as<StatusBlock>(), q, nq);   // (a family may have its own test)
    return in_kernel;
  }

  // Range pre-pass over a whole batch (8 B per query and array): the lowest failing index per array lands in
  // ws.host_status once the stream has been synchronised.  The ring and the sharded evaluations need it before any row
  // is produced.
  void enqueue_prepass(hipStream_t s, Workspace& ws, Queries<T> q, uint64_t nq) {
    ws.ensure_status();
    reset_status(ws.status.p, s);
    self().launch_range_check(s, ws.status.as<StatusBlock>(), q, nq);
    NDI_HIP(hipMemcpyAsync(ws.host_status, ws.status.p, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
  }

  // `good` rows of lanes elements, packed in host memory at src, into the caller's rows out_stride apart.
  void rows_out(T* dst, uint64_t out_stride, const void* src, uint64_t good) {
    const uint64_t lanes = self().lanes, row_bytes = lanes * sizeof(T);
    if (out_stride == lanes) std::memcpy(dst, src, good * row_bytes);
    else
      for (uint64_t r = 0; r < good; ++r) std::memcpy(dst + r * out_stride, (const char*)src + r * row_bytes, row_bytes);
  }

  // Host output with short trailing axes (the reference's own bench shapes: scalar data, a few lanes): one fused
  // search + evaluate launch per 64 MiB chunk into a staging buffer the library owns, results and status brought back
  // with one synchronisation (chunks of up to 8 MiB bounce through pinned memory), and only the rows before the first
  // failing query are copied into the caller's buffer.
  ndi_status eval_small_host(hipStream_t s, Workspace& ws, Queries<T> q_dev, Queries<T> q_orig, int q_space, uint64_t nq,
                             T* out, uint64_t out_stride, ndi_oob_info* info) {
    const uint64_t row_bytes = self().lanes * sizeof(T);
    const uint64_t chunk_q = std::max<uint64_t>(1, std::min<uint64_t>(nq, (64ull << 20) / row_bytes));
    constexpr size_t BOUNCE = 8ull << 20;
    ws.stage.reserve(chunk_q * row_bytes);
    ws.ensure_status();
    self().small_begin();
    StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
    for (uint64_t off = 0; off < nq; off += chunk_q) {
      const uint64_t cq = std::min<uint64_t>(chunk_q, nq - off);
      const size_t bytes = cq * row_bytes;
      NDI_HIP(hipMemsetAsync(st, 0xFF, 2 * sizeof(unsigned long long), s));
      self().launch_small(s, st, q_dev + off, ws.stage.as<T>(), cq);
      const bool bounce = bytes <= BOUNCE;
      if (bounce) {
        ws.ensure_pin(BOUNCE);
        NDI_HIP(hipMemcpyAsync(ws.pin, ws.stage.p, bytes, hipMemcpyDeviceToHost, s));
      }
      NDI_HIP(hipMemcpyAsync(ws.host_status, st, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
      NDI_HIP(hipStreamSynchronize(s));
      const FirstFail f = FirstFail::of(ws, q_dev);
      const uint64_t good = (f.first() == NO_FAIL) ? cq : (uint64_t)f.first();
      T* dst = out + off * out_stride;
      if (good) {
        if (bounce) rows_out(dst, out_stride, ws.pin, good);
        else
          NDI_HIP(hipMemcpy2D(dst, out_stride * sizeof(T), ws.stage.p, row_bytes, row_bytes, good,
                              hipMemcpyDeviceToHost));
      }
      if (f.first() != NO_FAIL) return report(q_orig + off, q_space, f, off, info);
    }
    return NDI_OK;
  }

  // Host arrays in and out, short trailing axes, small batch (the reference's own bench shapes: 1e4 queries on scalar
  // data): ZERO-COPY.  The queries are copied into the workspace's pinned buffer with a plain memcpy -- [a | b? | rows],
  // the query blocks 256-byte aligned -- the fused search + evaluation kernel reads them and writes the rows straight
  // through the host mapping of that buffer (a hipHostMalloc allocation is device-accessible), and one synchronisation
  // later the rows are memcpy'd to the caller: no H2D / D2H copy commands at all, only the 32-byte status read-back.
  // Saves two DMA round trips per call.  Rows at / after the first failing query are not copied out.
  ndi_status eval_small_zero_copy(hipStream_t s, Workspace& ws, Queries<T> q_host, uint64_t nq, T* out,
                                  uint64_t out_stride, ndi_oob_info* info) {
    const size_t q_bytes = ((nq * sizeof(T)) + 255) & ~(size_t)255, row_bytes = self().lanes * sizeof(T);
    const size_t rows_at = q_host.count() * q_bytes;
    ws.ensure_pin(std::max<size_t>(rows_at + nq * row_bytes, 8ull << 20));
    ws.ensure_status();
    T* pa = reinterpret_cast<T*>(ws.pin);
    T* pb = q_host.b ? reinterpret_cast<T*>((char*)ws.pin + q_bytes) : nullptr;
    T* po = reinterpret_cast<T*>((char*)ws.pin + rows_at);
    std::memcpy(pa, q_host.a, nq * sizeof(T));
    if (pb) std::memcpy(pb, q_host.b, nq * sizeof(T));
    self().small_begin();
    StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
    NDI_HIP(hipMemsetAsync(st, 0xFF, 2 * sizeof(unsigned long long), s));
    const Queries<T> q_pin{ws.pin_device<const T>(pa), pb ? ws.pin_device<const T>(pb) : nullptr};
    self().launch_small(s, st, q_pin, ws.pin_device<T>(po), nq);
    NDI_HIP(hipMemcpyAsync(ws.host_status, st, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
    NDI_HIP(hipStreamSynchronize(s));
    const FirstFail f = FirstFail::of(ws, q_host);
    const uint64_t good = (f.first() == NO_FAIL) ? nq : (uint64_t)f.first();
    if (good) rows_out(out, out_stride, po, good);
    if (f.first() != NO_FAIL) return report(q_host, NDI_MEM_HOST, f, 0, info);
    return NDI_OK;
  }

  // interp_array_into on staged (device) queries q; q_orig / q_space name the caller's arrays for error reports.
  ndi_status eval_body(hipStream_t s, Workspace& ws, Queries<T> q, Queries<T> q_orig, int q_space, uint64_t nq,
                       void* out_, uint64_t out_stride, const ndi_eval_opts& o, ndi_oob_info* info) {
    ws.last_q = q_orig.a;
    ws.last_q2 = q_orig.b;
    ws.last_q_space = q_space;
    ws.last_nq = nq;
    if (o.out_memspace == NDI_MEM_DEVICE) {
      self().enqueue(s, ws, q, nq, (T*)out_, out_stride, o.path, o.flags);
      ws.pending = true;
      if (o.async_launch) return NDI_OK;
      return collect(s, ws, 0, info);
    }
    // host output: the batch goes through a device staging buffer in query chunks of 256 MiB; only the rows before the
    // first failure are copied into the caller's buffer
    const uint64_t lanes = self().lanes, row_bytes = lanes * sizeof(T);
    if constexpr (Impl::small_rows)
      if (self().small_rows_fit()) return eval_small_host(s, ws, q, q_orig, q_space, nq, (T*)out_, out_stride, info);
    const uint64_t chunk_q = std::max<uint64_t>(1, std::min<uint64_t>(nq, (256ull << 20) / row_bytes));
    ws.stage.reserve(chunk_q * row_bytes);
    ws.ensure_status();
    for (uint64_t off = 0; off < nq; off += chunk_q) {
      const uint64_t cq = std::min<uint64_t>(chunk_q, nq - off);
      self().enqueue(s, ws, q + off, cq, ws.stage.as<T>(), lanes, o.path, 0);
      NDI_HIP(hipMemcpyAsync(ws.host_status, ws.sc[0].status.p, sizeof(StatusBlock), hipMemcpyDeviceToHost, s));
      NDI_HIP(hipStreamSynchronize(s));
      const FirstFail f = FirstFail::of(ws, q);
      const uint64_t good = (f.first() == NO_FAIL) ? cq : (uint64_t)f.first();
      if (good)
        NDI_HIP(hipMemcpy2D((T*)out_ + off * out_stride, out_stride * sizeof(T), ws.stage.p, row_bytes, row_bytes, good,
                            hipMemcpyDeviceToHost));
      if (f.first() != NO_FAIL) return report(q_orig + off, q_space, f, off, info);
    }
    return NDI_OK;
  }

  // ndi_interp{1,2}d_eval of a family with the small-row paths.
  ndi_status run_eval(const char* range, Queries<T> q_, uint64_t nq, void* out_, uint64_t out_stride,
                      const ndi_eval_opts* opts, ndi_oob_info* info) {
    DeviceGuard dg(self().device);
    Range rg(range);
    ndi_eval_opts o{};
    if (const ndi_status vs__ = take_opts(opts, o); vs__ != NDI_OK) return vs__;
    hipStream_t s = (hipStream_t)o.stream;  // NULL = the HIP default stream
    if (out_stride < self().lanes) return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)",
                                               (unsigned long long)out_stride, (unsigned long long)self().lanes);
    if (nq == 0) return NDI_OK;
    if (!q_.a || q_.count() != Impl::query_arrays || !out_) return fail(NDI_BAD_ARG, "null query / output pointer");
    SpaceLease lease(self().spaces, s);
    Workspace& ws = lease.ws;
    if (self().zero_copy_fits(nq, o.q_memspace, o.out_memspace))
      return eval_small_zero_copy(s, ws, q_, nq, (T*)out_, out_stride, info);
    const Queries<T> q = stage_queries(s, ws, q_, nq, o.q_memspace);
    return eval_body(s, ws, q, q_, o.q_memspace, nq, out_, out_stride, o, info);
  }

  // ---- ring evaluation ----------------------------------------------------------------------
  // interp_array for outputs that do not fit / need not stay in device memory: chunks through a ring.  The producer is a
  // two-stream pipeline: locate + group of the next chunks run on the workspace's side stream into scratch sets of their
  // own while the previous ones are evaluated on the caller's stream; events order the two.
  //
  // Groups (a family with ring_groups: the 1-D long-row bucketed plan).  Up to wmax = min(n_slots, RING_GROUP_MAX)
  // consecutive chunks, each prepared on its own, are evaluated by ONE launch (launch_eval_group): the launch's fixed cost
  // -- the table set read once beside the write stream, ramp and drain -- is paid once per group instead of once per
  // chunk.  A chunk joins a group only while every consumer so far has released its slot stream-ordered (returned NULL):
  // the slots a group writes are then free as soon as the caller's stream gets there.  A consumer that returns an event
  // works on another stream and lives on the overlap of chunk k+1's evaluation with its own work on chunk k: from its
  // first event on, the call runs one chunk per launch, as it always has.  consume() is still called once per chunk, in
  // order, after the chunk's kernels (its group's launch) are enqueued.  Chunk k uses scratch set k mod 2 * wmax: a
  // group being evaluated and the group being prepared never share a set.
  static constexpr bool ring_groups = false;   // (shadowed by a family that has launch_eval_group / groupable)

  template <class Plan>
  void ring_prep(hipStream_t s, Workspace& ws, Queries<T> q, uint64_t k, uint64_t cq, RingRun<Plan>& R, int path,
                 bool beside_eval) {
    Scratch& sc = ws.sc[k % R.n_sets];
    if (k >= R.n_sets) NDI_HIP(hipStreamWaitEvent(R.side, sc.eval_done, 0));   // chunk k - n_sets has released the set
    R.plans[k % R.n_sets] = self().prep(R.side, sc, q + k * R.chunk, cq, (T*)R.slots[k % R.n_slots], R.pitch, path,
                                        beside_eval);
    NDI_HIP(hipEventRecord(sc.prep_done, R.side));
  }

  // ring_begin resolves the ring and starts locate + group of chunk 0 on the side stream -- before the first failing
  // index of the batch is known on the host (it does not depend on it: the evaluation kernels skip rows at / after the
  // chunk's own first failure), so the range pre-pass and its synchronisation are hidden behind it.  With full-width
  // groups from the start, so are the other chunks of the first group.
  template <class Plan>
  void ring_begin(hipStream_t s, Workspace& ws, Queries<T> q, uint64_t nq, const ndi_ring_desc* ring, uint64_t stride,
                  const ndi_eval_opts& o, RingRun<Plan>& R) {
    R.n_slots = ring->n_slots;
    R.chunk = ring->chunk_queries;
    R.slots.resize(ring->n_slots);
    R.pitch = stride;          // row pitch of a chunk, in elements
    if (ring->slots) {
      for (uint32_t i = 0; i < ring->n_slots; ++i) R.slots[i] = ring->slots[i];
    } else {
      OwnedRing& ring_own = self().ring_own;
      R.own = std::unique_lock<std::mutex>(ring_own.mu);   // library-owned ring: one allocation, slots
      ring_own.ensure(ring->n_slots, ring->chunk_queries, stride * sizeof(T));   // interleaved row by row (OwnedRing)
      for (uint32_t i = 0; i < ring->n_slots; ++i) R.slots[i] = (char*)ring_own.buf.p + (size_t)i * stride * sizeof(T);
      R.pitch = (uint64_t)ring->n_slots * stride;
    }
    R.side = ring_overlap() ? ws.side_stream() : s;
    const int mode = Impl::ring_groups ? ring_group_mode() : 0;
    R.wmax = mode ? std::min<uint32_t>({R.n_slots, (uint32_t)RING_GROUP_MAX, Workspace::MAX_SETS / 2}) : 1u;
    R.narrow_first = mode == 2;
    R.n_sets = 2 * R.wmax;
    R.plans.assign(R.n_sets, Plan{});
    for (uint32_t i = 0; i < R.n_sets; ++i) ws.sc[i].ensure_events();
    // the side stream starts after everything already enqueued on s (the query upload)
    NDI_HIP(hipEventRecord(ws.order_event(), s));
    NDI_HIP(hipStreamWaitEvent(R.side, ws.order_event(), 0));
    uint64_t first = 1;   // chunks of the first launch
    if constexpr (Impl::ring_groups)
      if (!R.narrow_first) first = std::min<uint64_t>(R.wmax, (nq + R.chunk - 1) / R.chunk);
    for (R.prepped = 0; R.prepped < first;) {
      const uint64_t k = R.prepped++;
      ring_prep(s, ws, q, k, std::min<uint64_t>(R.chunk, nq - k * R.chunk), R, o.path, false);
      if constexpr (Impl::ring_groups)
        if (!self().groupable(R.plans[k])) break;   // no group starts here: nothing to prepare ahead
    }
  }

  // Produces the rows [0, limit) of the batch chunk by chunk.  q_offset / shard: position of this batch in a
  // sharded evaluation (the consumer sees global query indices).
  template <class Plan>
  void ring_produce(hipStream_t s, Workspace& ws, Queries<T> q, uint64_t limit, RingRun<Plan>& R,
                    ndi_ring_consumer consume, void* user, const ndi_eval_opts& o, uint64_t q_offset, uint32_t shard) {
    std::vector<hipEvent_t> busy(R.n_slots, nullptr);
    const uint64_t nchunks = (limit + R.chunk - 1) / R.chunk;
    auto count = [&](uint64_t k) { return std::min<uint64_t>(R.chunk, limit - k * R.chunk); };
    bool solo = R.wmax == 1;      // one chunk per launch: no groups, or a consumer has returned an event
    uint64_t prepped = R.prepped; // chunks [k, prepped) are located + grouped
    for (uint64_t k = 0; k < nchunks;) {
      uint32_t want = solo || (R.narrow_first && k == 0) ? 1u : (uint32_t)std::min<uint64_t>(R.wmax, nchunks - k);
      uint32_t w = 0;
      while (w < want) {
        if (k + w >= prepped) {
          ring_prep(s, ws, q, k + w, count(k + w), R, o.path, R.side != s);
          prepped = k + w + 1;
        }
        bool joins = w == 0;     // the first chunk is evaluated whatever its plan; the others only by a group launch
        if constexpr (Impl::ring_groups) joins = joins || (self().groupable(R.plans[k % R.n_sets]) &&
                                                          self().groupable(R.plans[(k + w) % R.n_sets]));
        if (!joins) break;       // (it stays prepared and opens the next launch)
        ++w;
      }
      Scratch* sets[RING_GROUP_MAX];
      Plan plans[RING_GROUP_MAX];
      for (uint32_t i = 0; i < w; ++i) {
        sets[i] = &ws.sc[(k + i) % R.n_sets];
        plans[i] = R.plans[(k + i) % R.n_sets];
        NDI_HIP(hipStreamWaitEvent(s, sets[i]->prep_done, 0));
        const uint32_t slot = (uint32_t)((k + i) % R.n_slots);
        if (busy[slot]) {   // the consumer reads this slot on another stream: wait for it there
          NDI_HIP(hipStreamWaitEvent(s, busy[slot], 0));
          busy[slot] = nullptr;
        }
      }
      bool grouped = false;
      if constexpr (Impl::ring_groups)
        if (self().groupable(plans[0])) {
          self().launch_eval_group(s, sets, plans, w);
          grouped = true;
        }
      if (!grouped) self().launch_eval(s, *sets[0], plans[0]);   // (w == 1)
      for (uint32_t i = 0; i < w; ++i) NDI_HIP(hipEventRecord(sets[i]->eval_done, s));
      for (uint32_t i = 0; i < w && consume; ++i) {
        const uint32_t slot = (uint32_t)((k + i) % R.n_slots);
        ndi_ring_chunk c{};
        c.index = k + i; c.q_begin = q_offset + (k + i) * R.chunk; c.q_count = count(k + i); c.out = R.slots[slot];
        c.row_stride = R.pitch; c.slot = slot; c.shard = shard; c.stream = (void*)s;
        busy[slot] = (hipEvent_t)consume(user, &c);
        if (busy[slot]) solo = true;   // a consumer on another stream: it keeps its overlap, one chunk per launch from here
      }
      k += w;
    }
    NDI_HIP(hipStreamSynchronize(s));
    NDI_HIP(hipStreamSynchronize(R.side));   // (speculative chunks that were never evaluated)
    for (hipEvent_t e : busy)
      if (e) NDI_HIP(hipEventSynchronize(e));
    ws.pending = false;
  }

  // ndi_interp{1,2}d_eval_ring.
  ndi_status run_ring(const char* range, Queries<T> q_, uint64_t nq, const ndi_ring_desc* ring, ndi_ring_consumer consume,
                      void* user, const ndi_eval_opts* opts, ndi_oob_info* info) {
    DeviceGuard dg(self().device);
    ndi_eval_opts o{};
    if (const ndi_status vs__ = take_opts(opts, o); vs__ != NDI_OK) return vs__;
    hipStream_t s = (hipStream_t)o.stream;
    uint64_t stride = 0;
    ndi_status rs = check_ring_desc(ring, self().lanes, &stride);
    if (rs != NDI_OK) return rs;
    if (nq == 0) return NDI_OK;
    if (!q_.a || q_.count() != Impl::query_arrays) return fail(NDI_BAD_ARG, "null query pointer");
    Range rg(range);
    SpaceLease lease(self().spaces, s);
    Workspace& ws = lease.ws;
    const Queries<T> q = stage_queries(s, ws, q_, nq, o.q_memspace);
    // range pre-pass over the whole batch: the first failing index is known before any chunk is handed out
    enqueue_prepass(s, ws, q, nq);
    RingRun<typename Impl::Plan> R;
    ring_begin(s, ws, q, nq, ring, stride, o, R);
    NDI_HIP(hipStreamSynchronize(s));
    const FirstFail f = FirstFail::of(ws, q);
    const uint64_t limit = f.first() == NO_FAIL ? nq : std::min<uint64_t>(nq, f.first());
    ring_produce(s, ws, q, limit, R, consume, user, o, 0, 0);
    if (f.first() == NO_FAIL) return NDI_OK;
    return report(q_, o.q_memspace, f, 0, info);
  }

  // The front of every trim (under the family's DeviceGuard): the idle scratch sets and the library-owned ring.
  void trim_front() {
    self().spaces.trim();
    if constexpr (Impl::ring) {
      std::lock_guard<std::mutex> g(self().ring_own.mu);
      self().ring_own.clear();
    }
  }
};
