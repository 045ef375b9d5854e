// csrc/antiderivative_host.hpp -- the host side of antiderivative handles (ndi_interp1d_antiderivative,
// ndi_interp1d_integrate); included by ndinterp_api.hip inside namespace ndi, behind Interp1DImpl.
//
// An antiderivative handle is an Interp1DBase of its own, so that every existing handle takes exactly the code paths it
// took before.  It owns copies of the source's y (cubic class: a, b too), the knot pyramid and the prefix table P, and
// evaluates in the two-kernel form only: locate_kernel writes idx[] / t[] and the first failing index, then ONE
// evaluation launch reads them (antiderivative_kernels.hpp).  integrate() runs the search twice (lo into scratch set 0
// and first_fail[0], hi into set 1 and first_fail[1]) and the same single evaluation launch with the pair flag.
// Staging, the first-error report, the host-output chunk loop and finish are the float host engine's (float_host.hpp).

// ---- the prefix table P[n][lanes] of the tables y (a, b) on the device-resident knots x (NULL stream, complete on return).
// The 2-D integral build (bicubic_integral_host.hpp) runs it on views of its grids.
template <class T, bool LINEAR>
static void antideriv_prefix_build(int device, uint64_t n, uint64_t lanes, const T* y, const T* a, const T* b, const T* x, T* P) {
  AntiBuildArgs<T> A{};
  A.y = y; A.a = a; A.b = b; A.x = x; A.P = P;
  A.n = n; A.lanes = lanes;
  A.nblk = (n + AD_B - 1) / AD_B;
  A.single = A.nblk == 1 ? 1u : 0u;
  DevBuf tmp;
  if (!A.single) {   // the block totals: kept per host thread like the spline build's temporaries
    const size_t tb = (size_t)A.nblk * lanes * sizeof(T);
    if (tb <= ((size_t)64 << 20)) A.tot = static_cast<T*>(build_scratch().device_buf(device, tb));
    else {
      tmp.reserve(tb);
      A.tot = tmp.as<T>();
    }
  }
  constexpr int VN = Wide<T>::N;
  const hipStream_t s0 = nullptr;
  const bool vec = lanes % VN == 0 && aligned16(A.y) && aligned16(A.a) && aligned16(A.b) && aligned16(A.P) && aligned16(A.tot);
  const bool staged = lanes <= AD_STAGED_LANES;
  const bool fuse = A.nblk <= AD_FUSE_BLOCKS;
  bool vec_local = false;
  unsigned local_grid = 0;
  if (staged) {
    // chains per workgroup: as many blocks as AD_STAGED_CHAINS allows, halved while the grid would leave the chip's
    // 2048 resident workgroups unused (phase 2 takes the same time for one chain as for 32)
    uint32_t kb = std::max<uint32_t>(1, AD_STAGED_CHAINS / (uint32_t)lanes);
    while (kb > 1 && (A.nblk + kb - 1) / kb < 2048) kb /= 2;
    A.kb = kb;
    const size_t lds = (size_t)kb * (AD_B * lanes + lanes) * sizeof(T);
    const unsigned grid = local_grid = (unsigned)std::min<uint64_t>((A.nblk + kb - 1) / kb, 1u << 16);
    allow_dynamic_lds(reinterpret_cast<const void*>(&antideriv_local_staged_kernel<T, LINEAR>), 96 * 1024);
    hipLaunchKernelGGL((antideriv_local_staged_kernel<T, LINEAR>), dim3(grid), dim3(BLOCK), lds, s0, A);
  } else {
    // every thread is a 256-step chain, so the threads are what hides the latency: 16-byte vectors only where they
    // still leave the chip a full set of waves (4096 x 4096 has 65536 chains: one lane each, 4-8 byte coalesced loads)
    vec_local = vec && A.nblk * (lanes / VN) >= (uint64_t)cu_count() * 8 * 64;
    const uint64_t total = A.nblk * (vec_local ? lanes / VN : lanes);
    const unsigned grid = local_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
    if (vec_local) hipLaunchKernelGGL((antideriv_local_lanes_kernel<T, VN, LINEAR>), dim3(grid), dim3(BLOCK), 0, s0, A);
    else hipLaunchKernelGGL((antideriv_local_lanes_kernel<T, 1, LINEAR>), dim3(grid), dim3(BLOCK), 0, s0, A);
  }
  NDI_HIP(hipGetLastError());
  if (trace_plan())   // grid: the local kernel's; kb / vec_local: 0 on the local kernel that has no such field
    std::fprintf(stderr, "[ndi plan] antiderivative build linear=%d staged=%d kb=%u vec=%d vec_local=%d nblk=%llu single=%d fuse=%d "
                 "grid=%u\n", (int)LINEAR, (int)staged, A.kb, (int)vec, (int)vec_local, (unsigned long long)A.nblk, (int)A.single,
                 (int)(!A.single && fuse), local_grid);
  if (!A.single) {
    if (!fuse) {
      if (staged) {
        const unsigned grid = (unsigned)((lanes * 64 + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL((antideriv_offsets_kernel<T, true>), dim3(grid), dim3(BLOCK), 0, s0, A.tot, A.nblk, (n - 1) / AD_B, lanes);
      } else {
        const unsigned grid = (unsigned)((lanes + BLOCK - 1) / BLOCK);
        hipLaunchKernelGGL((antideriv_offsets_kernel<T, false>), dim3(grid), dim3(BLOCK), 0, s0, A.tot, A.nblk, (n - 1) / AD_B, lanes);
      }
      NDI_HIP(hipGetLastError());
    }
    const uint64_t total = n * (vec ? lanes / VN : lanes);
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
    if (vec && fuse) hipLaunchKernelGGL((antideriv_add_kernel<T, VN, true>), dim3(grid), dim3(BLOCK), 0, s0, A);
    else if (vec) hipLaunchKernelGGL((antideriv_add_kernel<T, VN, false>), dim3(grid), dim3(BLOCK), 0, s0, A);
    else if (fuse) hipLaunchKernelGGL((antideriv_add_kernel<T, 1, true>), dim3(grid), dim3(BLOCK), 0, s0, A);
    else hipLaunchKernelGGL((antideriv_add_kernel<T, 1, false>), dim3(grid), dim3(BLOCK), 0, s0, A);
    NDI_HIP(hipGetLastError());
  }
  NDI_HIP(hipStreamSynchronize(s0));   // the table is complete on return: any stream may read it (and tmp may go)
}

template <class T>
struct AntiderivImpl final : Interp1DBase, FloatEngine<T, AntiderivImpl<T>> {
  bool linear = false;     // the source's evaluation class
  int rule = HR_SPLINE;    // the source's rule and derivative order (names in messages, the replica signature)
  int deriv = 0;
  int mode = EX_NO;
  uint64_t n = 0;
  DevBuf arena;            // small handles: ONE allocation behind pyr.buf / y / a / b / P; declared first: freed last
  DevicePyramid<T> pyr;
  DevBuf y, a, b, P;
  SpaceSet spaces;

  const char* source_name() const { return linear ? "Linear" : hermite_rule_name(rule); }
  bool is_antiderivative() const override { return true; }

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, pyr.host_knots.data(), pyr.host_knots.size() * sizeof(T));
    const uint64_t f[3] = {n, (uint64_t)(linear ? NDI_LINEAR : NDI_CUBIC_SPLINE) | ((uint64_t)rule << 8) |
                                  ((uint64_t)deriv << 16) | (1ull << 24) /* Antiderivative */, (uint64_t)mode};
    return fnv1a(h, f, sizeof(f));
  }

  // The arena of Interp1DImpl, extended by one table.
  void adopt_arena() {
    auto al = [](size_t bts) { return (bts + 255) & ~(size_t)255; };
    uint64_t block = 1;
    while ((uint64_t)64 * block < n) block *= 2;
    const size_t pyr_b = al((n + (n + block - 1) / block) * sizeof(T));
    const size_t data_b = al((size_t)n * lanes * sizeof(T));
    const size_t tab_b = linear ? 0 : al((size_t)(n - 1) * lanes * sizeof(T));
    const size_t total = pyr_b + 2 * data_b + 2 * tab_b;
    if (total > ((size_t)1 << 20)) return;
    arena.reserve(total);
    char* p0 = static_cast<char*>(arena.p);
    pyr.buf.adopt(p0, pyr_b);
    y.adopt(p0 + pyr_b, data_b);
    P.adopt(p0 + pyr_b + data_b, data_b);
    if (tab_b) {
      a.adopt(p0 + pyr_b + 2 * data_b, tab_b);
      b.adopt(p0 + pyr_b + 2 * data_b + tab_b, tab_b);
    }
  }

  void reserve_tables(const T* knots) {
    adopt_arena();
    pyr.upload(knots, n);
    y.reserve((size_t)n * lanes * sizeof(T));
    P.reserve((size_t)n * lanes * sizeof(T));
    if (!linear) {
      a.reserve((size_t)(n - 1) * lanes * sizeof(T));
      b.reserve((size_t)(n - 1) * lanes * sizeof(T));
    }
  }

  // ---- build: the prefix table from this handle's own copies (NULL stream, complete on return) ----------------------
  template <bool LINEAR>
  void launch_build() {
    antideriv_prefix_build<T, LINEAR>(device, n, lanes, y.as<T>(), a.as<T>(), b.as<T>(), pyr.view.lv0, P.as<T>());
  }

  void build() {
    Range rg("ndi:antiderivative_build");
    if (linear) launch_build<true>();
    else launch_build<false>();
  }

  // ---- evaluation ------------------------------------------------------------------------------------------------------
  // Search of one query array into scratch set `sc` and first_fail[axis] of scratch set 0's status block.
  void locate(hipStream_t s, Workspace& ws, int axis, const T* q, uint64_t nq) {
    Scratch& sc = ws.sc[axis];
    sc.idx.reserve(nq * sizeof(uint32_t));
    sc.t.reserve(nq * sizeof(T));
    StatusBlock* st = ws.sc[0].status.as<StatusBlock>();
    run_locate<T>(s, pyr, q, nq, sc.idx.as<uint32_t>(), nullptr, sc.t.as<T>(), &st->first_fail[axis], mode);
  }

  // One batch on device pointers: status reset, the search(es), ONE evaluation launch.  hi == nullptr: F(q); else F(hi) - F(q).
  // (path and flags: the engine's; this family has one form and always its range test)
  void enqueue(hipStream_t s, Workspace& ws, Queries<T> qs, uint64_t nq, T* out, uint64_t out_stride, int, int) {
    const T* q = qs.a;
    const T* hi = qs.b;
    g_last_path.store(NDI_PATH_GATHER);
    ws.sc[0].status.reserve(sizeof(StatusBlock));
    reset_status(ws.sc[0].status.p, s);
    locate(s, ws, 0, q, nq);
    if (hi) locate(s, ws, 1, hi, nq);
    AntiEvalArgs<T> A{};
    A.knots = pyr.view.lv0;
    A.y = y.as<T>(); A.a = a.as<T>(); A.b = b.as<T>(); A.P = P.as<T>();
    A.idx = ws.sc[0].idx.as<uint32_t>();
    A.t = ws.sc[0].t.as<T>();
    A.idx2 = hi ? ws.sc[1].idx.as<uint32_t>() : nullptr;
    A.t2 = hi ? ws.sc[1].t.as<T>() : nullptr;
    A.out = out;
    A.lanes = lanes; A.out_stride = out_stride; A.nq = nq;
    A.status = ws.sc[0].status.as<StatusBlock>();
    A.n_int = (uint32_t)(n - 1);
    constexpr int VN = Wide<T>::N;
    const bool vec_ok = (lanes % VN == 0) && (out_stride % VN == 0) && aligned16(out) && aligned16(A.y) && aligned16(A.a) &&
                        aligned16(A.b) && aligned16(A.P);
    const uint64_t LV = vec_ok ? lanes / VN : lanes;
    const bool pair = hi != nullptr;
    if (vec_ok && LV >= (uint64_t)BLOCK) {   // long rows
      const uint64_t segs = (LV + BLOCK - 1) / BLOCK;
      const dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nq, 65536)), (unsigned)std::min<uint64_t>(segs, 64));
      if (trace_plan())
        std::fprintf(stderr, "[ndi plan] antiderivative eval form=rows linear=%d pair=%d vec=1 lv=%llu tile_q=0 grid=%u x %u\n",
                     (int)linear, (int)pair, (unsigned long long)LV, grid.x, grid.y);
      pick_bool(linear, [&](auto lin_) {
        constexpr bool LIN = lin_;
        pick_bool(pair, [&](auto pair_) { launch1<T>(s, PC_EVAL, grid, dim3(BLOCK), 0, antideriv_eval_rows_kernel<T, LIN, pair_>, A); });
      });
      return;
    }
    const uint32_t tile_q = (uint32_t)std::max<uint64_t>(1, 1024 / std::max<uint64_t>(LV, 1));
    const uint64_t ntiles = (nq + tile_q - 1) / tile_q;
    const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, 16384));
    if (trace_plan())
      std::fprintf(stderr, "[ndi plan] antiderivative eval form=flat linear=%d pair=%d vec=%d lv=%llu tile_q=%u grid=%u x 1\n",
                   (int)linear, (int)pair, (int)vec_ok, (unsigned long long)LV, tile_q, gx);
    ProfScope ps(s, PC_EVAL);
    pick_bool(linear, [&](auto lin_) {
      constexpr bool LIN = lin_;
      pick_bool(pair, [&](auto pair_) {
        constexpr bool PAIR = pair_;
        pick_or<1, VN>(vec_ok ? VN : 1, [&](auto vec_) {
          hipLaunchKernelGGL((antideriv_eval_flat_kernel<T, LIN, PAIR, vec_>), dim3(gx), dim3(BLOCK), 0, s, A, tile_q);
        });
      });
    });
    NDI_HIP(hipGetLastError());
    ps.done();
  }

  // ---- what the host engine (float_host.hpp) takes from this family: no small-row paths, no ring -----------------------
  static constexpr bool small_rows = false, ring = false;
  // lo is tested before hi at the same index, and both are the source's "x"
  static const char* axis_name(int) { return "x"; }

  // eval (hi_ == nullptr) and integrate share one body.
  ndi_status run(const void* q_, const void* hi_, bool pair, uint64_t nq, void* out_, uint64_t out_stride,
                 const ndi_eval_opts* opts, ndi_oob_info* info) {
    ndi_eval_opts o{};
    if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
    if (o.path == NDI_PATH_BUCKETED)
      return fail(NDI_UNSUPPORTED, "NDI_PATH_BUCKETED: an antiderivative handle evaluates in the two-kernel gather form only "
                  "(its quartic needs the prefix table; the grouped forms do not read it)");
    if (out_stride < lanes)
      return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)out_stride, (unsigned long long)lanes);
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    if (nq == 0) return NDI_OK;
    if (!q_ || !out_ || (pair && !hi_)) return fail(NDI_BAD_ARG, "null query / output pointer");
    DeviceGuard dg(device);
    Range rg(pair ? "ndi_interp1d_integrate" : "ndi_interp1d_eval");
    hipStream_t s = (hipStream_t)o.stream;
    SpaceLease lease(spaces, s);
    Workspace& ws = lease.ws;
    const Queries<T> orig{(const T*)q_, pair ? (const T*)hi_ : nullptr};
    return this->eval_body(s, ws, this->stage_queries(s, ws, orig, nq, o.q_memspace), orig, o.q_memspace, nq, out_,
                           out_stride, o, info);
  }

  ndi_status eval(const void* q_, uint64_t nq, void* out_, uint64_t out_stride, const ndi_eval_opts* opts,
                  ndi_oob_info* info) override {
    return run(q_, nullptr, false, nq, out_, out_stride, opts, info);
  }

  ndi_status integrate(const void* lo, const void* hi, uint64_t nq, void* out_, uint64_t out_stride,
                       const ndi_eval_opts* opts, ndi_oob_info* info) override {
    return run(lo, hi, true, nq, out_, out_stride, opts, info);
  }

  ndi_status finish(void* stream, ndi_oob_info* info) override { return this->run_finish(stream, info); }

  // lane-wise evaluation (defined in lanewise_host.hpp)
  void lanewise_enqueue(hipStream_t s, Workspace& ws, const T* q, uint64_t q_stride, uint64_t rows, T* out,
                        uint64_t out_stride, bool check);
  ndi_status eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                           const ndi_eval_opts* opts, ndi_oob_info* info) override;

  ndi_status eval_ring(const void*, uint64_t, const ndi_ring_desc*, ndi_ring_consumer, void*, const ndi_eval_opts*,
                       ndi_oob_info*) override {
    return fail(NDI_UNSUPPORTED, "eval_ring: an antiderivative handle (of %s) has no ring evaluation; ndi_interp1d_eval "
                "chunk by chunk serves it", source_name());
  }

  ndi_status trim() override {
    DeviceGuard dg(device);
    this->trim_front();
    return NDI_OK;
  }
  uint64_t scratch_sets() override { return spaces.size(); }

  ndi_status coefficients(void*, void*, int) override {
    return fail(NDI_BAD_ARG, "coefficients: the antiderivative of %s is a piecewise quartic: it has no a / b tables "
                "(ndi_interp1d_data hands back its prefix table)", source_name());
  }
  ndi_status derivative(int, Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "derivative: the antiderivative of %s is a piecewise quartic, which the derivative rule for "
                "{y, a, b} tables does not take; its derivative is the handle it was made from", source_name());
  }
  ndi_status antiderivative(Interp1DBase**) override {
    return fail(NDI_BAD_ARG, "antiderivative: this handle is already the antiderivative of %s; a second antiderivative "
                "(a piecewise quintic) is not provided", source_name());
  }
  ndi_status inverse(Interp1DBase** out) override;   // (defined behind InverseImpl)

  ndi_status data_table(void* data_out, int memspace) override {
    DeviceGuard dg(device);
    NDI_HIP(hipMemcpy(data_out, P.p, (size_t)n * lanes * sizeof(T),
                      memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return NDI_OK;
  }

  std::unique_ptr<AntiderivImpl<T>> shell(int dev) const {
    std::unique_ptr<AntiderivImpl<T>> h(new AntiderivImpl<T>());
    h->dtype = dtype; h->device = dev; h->lanes = lanes;
    h->linear = linear; h->rule = rule; h->deriv = deriv; h->mode = mode; h->n = n;
    return h;
  }

  ndi_status clone_to(int dev, Interp1DBase** out) override {
    std::unique_ptr<AntiderivImpl<T>> h = shell(dev);
    {
      DeviceGuard dg(device);
      NDI_HIP(hipDeviceSynchronize());     // the source tables are complete
    }
    DeviceGuard dg(dev);
    h->reserve_tables(pyr.host_knots.data());
    const size_t data_b = (size_t)n * lanes * sizeof(T), tab_b = (size_t)(n - 1) * lanes * sizeof(T);
    copy_across_devices(h->y.p, dev, y.p, device, data_b);
    copy_across_devices(h->P.p, dev, P.p, device, data_b);
    if (!linear) {
      copy_across_devices(h->a.p, dev, a.p, device, tab_b);
      copy_across_devices(h->b.p, dev, b.p, device, tab_b);
    }
    *out = h.release();
    return NDI_OK;
  }
};

// ndi_interp1d_antiderivative of an f32 / f64 handle: the refusals first, then a new handle on this handle's device with
// its own copies of the tables (this handle is only read and is destroyed independently) and the prefix table built there.
template <class T>
ndi_status Interp1DImpl<T>::antiderivative(Interp1DBase** out) {
  const bool lin = strategy != NDI_CUBIC_SPLINE;
  const char* name = lin ? "Linear" : hermite_rule_name(rule);
  if (mode == EX_PERIODIC)
    return fail(NDI_BAD_ARG, "%s: the Periodic extrapolation mode has no antiderivative handle (F outside the knots needs "
                "m * P[n-1] + F(wrapped x), which is not provided)", name);
  DeviceGuard dg(device);
  std::unique_ptr<AntiderivImpl<T>> h(new AntiderivImpl<T>());
  h->dtype = dtype; h->device = device; h->lanes = lanes;
  h->linear = lin; h->rule = rule; h->deriv = deriv; h->mode = mode; h->n = n;
  h->reserve_tables(pyr.host_knots.data());
  const size_t data_b = (size_t)n * lanes * sizeof(T), tab_b = (size_t)(n - 1) * lanes * sizeof(T);
  NDI_HIP(hipMemcpyAsync(h->y.p, data.p, data_b, hipMemcpyDeviceToDevice, nullptr));
  if (!lin) {
    NDI_HIP(hipMemcpyAsync(h->a.p, ca.p, tab_b, hipMemcpyDeviceToDevice, nullptr));
    NDI_HIP(hipMemcpyAsync(h->b.p, cb.p, tab_b, hipMemcpyDeviceToDevice, nullptr));
  }
  h->build();
  *out = h.release();
  return NDI_OK;
}
