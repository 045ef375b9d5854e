// csrc/trilinear_host.hpp -- the host side of the 3-D handles (ndi_interp3d_*, include/ndinterp3d.h): Interp3DImpl<T> with the
// Trilinear strategy; included by ndinterp_api.hip inside namespace ndi, behind float_host.hpp's helpers.
//
// Interp3DDriver<T> is what every 3-D strategy shares (the axes, eval's chunking / staging / report, the head of a chunk, the
// launch geometry); Interp3DImpl<T> (Trilinear, here) and Tricubic3DImpl<T> (tricubic_host.hpp) add their table and enqueue.
// The 3-D handles keep a small driver of their own, as AntiderivImpl does: three query arrays do not fit Queries<T> /
// FirstFail, which every other family instantiates, and the 3-D handle has no ring, no sharded form, no async_launch and no
// small-row paths to share.  It is built from the common parts -- take_opts, the workspace lease, device staging of host
// arrays in row chunks, the status read-back, ProfScope through launch1 -- in the order: options, refusals, lease, stage,
// pre-pass or not, launch, status, copy-out, report.
//
// Plan: ONE launch of eval_trilinear_kernel<T, VEC, STAGE, CHECK> per chunk.
//   VEC    16-byte vectors (4 x f32 / 2 x f64) when lanes and the output stride are multiples of it and the grid and the output
//          are 16-byte aligned, else single elements
//   STAGE  the three axes in LDS when (nx + ny + nz) * sizeof(T) fits LDS_STAGE_LIMIT, else bisected in global memory
//   CHECK  the kernel's own range / NaN test: NDI_EVAL_FRESH_OUTPUT / NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED, and every chunk
//          that goes to the library's own staging buffer; otherwise range_check3_kernel runs first
// Tuning knobs (through NDI_TUNE_LIVE like the others):
//   NDI_TRILINEAR_STAGE   unset / -1 = auto, 0 = never, 1 = where it fits (the same as auto; kept for A/B)
//   NDI_TRILINEAR_VEC     unset / -1 = auto, 1 = single elements
//   NDI_TRILINEAR_CHUNK   bytes of rows per staging chunk of a call on host arrays (unset / <= 0: 256 MiB)
constexpr uint64_t TRILINEAR_CHUNK_BYTES = 256ull << 20;
struct TrilinearKnobs {
  int stage, vec;
  uint64_t chunk_bytes;
};
static TrilinearKnobs trilinear_knobs() {
  static const Knob stage{"NDI_TRILINEAR_STAGE", -1, Knob::live}, vec{"NDI_TRILINEAR_VEC", -1, Knob::live},
      chunk{"NDI_TRILINEAR_CHUNK", 0, Knob::live};
  const int c = chunk.get();
  return {stage.get(), vec.get(), c > 0 ? (uint64_t)c : TRILINEAR_CHUNK_BYTES};
}

// The builder's checks on host axes, Interp2DBuilder::build's order (interp2d/mod.rs:480-509) with a third axis.  A null axis
// is 0..n: its length is the data's and it rises.
template <class T>
ndi_status check_axes_3d(const T* x, uint64_t x_len, const T* y, uint64_t y_len, const T* z, uint64_t z_len, uint64_t nx,
                         uint64_t ny, uint64_t nz, unsigned long long need = 2) {
  const uint64_t n[3] = {nx, ny, nz}, len[3] = {x ? x_len : nx, y ? y_len : ny, z ? z_len : nz};
  const T* k[3] = {x, y, z};
  static const char* const name[3] = {"x", "y", "z"};
  for (int a = 0; a < 3; ++a)
    if (n[a] < need)
      return fail(NDI_NOT_ENOUGH_DATA,
                  "The %d-dimension has not enough data for the chosen interpolation strategy. "
                  "Provided: %llu, Reqired: %llu", a, (unsigned long long)n[a], need);
  for (int a = 0; a < 3; ++a)
    if (len[a] != n[a])
      return fail(NDI_SHAPE, "Lenghts of %s-axis and data-%d-axis need to match. Got %s: %llu, data-%d: %llu", name[a], a,
                  name[a], (unsigned long long)len[a], a, (unsigned long long)n[a]);
  for (int a = 0; a < 3; ++a)
    if (k[a] && monotonic_scan(k[a], len[a]) != NDI_MONO_RISING_STRICT)
      return fail(NDI_MONOTONIC, "The %s-axis needs to be strictly monotonic rising", name[a]);
  return NDI_OK;
}

struct Interp3DBase {
  virtual ~Interp3DBase() = default;
  int dtype = 0, device = 0;
  uint64_t lanes = 0;
  virtual ndi_status eval(const void* qx, const void* qy, const void* qz, uint64_t nq, void* out, uint64_t out_stride,
                          const ndi_eval_opts& o, ndi_oob_info* info) = 0;
  virtual ndi_status clone_to(int dev, Interp3DBase** out) = 0;
  // ndi_interp3d_tables (include/ndinterp3d_cubic.h): Tricubic handles only
  virtual ndi_status tables(void* const t[7], int memspace) {
    return fail(NDI_BAD_ARG, "ndi_interp3d_tables takes a Tricubic handle: Trilinear keeps no node derivatives");
  }
};

// The options of ndi_interp3d_eval and the refusals that need no handle (so they come first, and answer without a device).
static ndi_status trilinear_take_opts(const ndi_eval_opts* opts, ndi_eval_opts& o) {
  if (const ndi_status vs = take_opts(opts, o); vs != NDI_OK) return vs;
  if (o.path == NDI_PATH_BUCKETED)
    return fail(NDI_BAD_ARG, "Trilinear has no tile-grouped evaluation form: NDI_PATH_BUCKETED is Bilinear's (AUTO and "
                "GATHER evaluate)");
  if (o.async_launch) return fail(NDI_UNSUPPORTED, "ndi_interp3d_eval: async_launch is not provided");
  return NDI_OK;
}

// What the 3-D strategies share: the axes, the chunking / staging / report driver (eval) and the head of a chunk (the status
// words and the range pre-pass).  A strategy adds its table and the ONE strategy-specific step, enqueue.
template <class T>
struct Interp3DDriver : Interp3DBase {
  int mode = EX_NO;
  uint64_t nx = 0, ny = 0, nz = 0;
  std::vector<T> hx, hy, hz;   // the axes on the host: range limits, clones
  DevBuf axes;                 // [x | y | z], one allocation
  SpaceSet spaces;

  const T* dev_axis(int a) const { return axes.as<T>() + (a == 0 ? 0 : a == 1 ? nx : nx + ny); }

  void upload_axes() {
    axes.reserve((nx + ny + nz) * sizeof(T));
    NDI_HIP(hipMemcpy((T*)dev_axis(0), hx.data(), nx * sizeof(T), hipMemcpyHostToDevice));
    NDI_HIP(hipMemcpy((T*)dev_axis(1), hy.data(), ny * sizeof(T), hipMemcpyHostToDevice));
    NDI_HIP(hipMemcpy((T*)dev_axis(2), hz.data(), nz * sizeof(T), hipMemcpyHostToDevice));
  }

  // One chunk on device pointers through scratch set 0: the pre-pass unless `check`, then ONE evaluation launch.
  virtual void enqueue(hipStream_t s, Workspace& ws, const T* qx, const T* qy, const T* qz, uint64_t nq, T* out,
                       uint64_t out_stride, bool check) = 0;

  // The head of a chunk: the status words cleared, and the range pre-pass unless the kernel tests the queries itself.
  TrilinearStatus* begin_chunk(hipStream_t s, Workspace& ws, const T* qx, const T* qy, const T* qz, uint64_t nq, bool check) {
    g_last_path.store(NDI_PATH_GATHER);
    TrilinearStatus* st = ws.sc[0].status.as<TrilinearStatus>();
    NDI_HIP(hipMemsetAsync(st, 0xFF, sizeof(TrilinearStatus), s));   // NO_FAIL on every axis
    if (!check) {
      const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + BLOCK - 1) / BLOCK, 4096));
      ProfScope ps(s, PC_LOCATE);
      hipLaunchKernelGGL(range_check3_kernel<T>, dim3(g), dim3(BLOCK), 0, s, qx, qy, qz, nq, hx.front(), hx.back(), hy.front(),
                         hy.back(), hz.front(), hz.back(), mode, &st->first_fail[0]);
      NDI_HIP(hipGetLastError());
      ps.done();
    }
    return st;
  }

  // the axes and the scalars of a replica on `dev` (the strategy copies its table)
  void clone_driver_to(int dev, Interp3DDriver<T>& h) const {
    h.dtype = dtype; h.device = dev; h.lanes = lanes;
    h.mode = mode;
    h.nx = nx; h.ny = ny; h.nz = nz;
    h.hx = hx; h.hy = hy; h.hz = hz;
    {
      DeviceGuard dg(dev);
      h.axes.reserve((nx + ny + nz) * sizeof(T));
    }
    copy_across_devices(h.axes.p, dev, axes.p, device, (nx + ny + nz) * sizeof(T));
  }

  // The fields of a descriptor and its axes, checked as the builder checks them with `need` knots per axis.
  ndi_status take_desc(const ndi_interp3d_desc& d, unsigned long long need) {
    dtype = d.dtype;
    device = d.device;
    mode = d.extrapolate ? EX_YES : EX_NO;
    nx = d.nx; ny = d.ny; nz = d.nz;
    lanes = d.lanes;
    hx = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.nx);
    hy = d.y ? fetch_axis<T>(d.y, d.y_len, d.memspace) : default_axis<T>(d.ny);
    hz = d.z ? fetch_axis<T>(d.z, d.z_len, d.memspace) : default_axis<T>(d.nz);
    if (d.validate) {
      const ndi_status st = check_axes_3d<T>(hx.data(), hx.size(), hy.data(), hy.size(), hz.data(), hz.size(), d.nx, d.ny, d.nz,
                                             need);
      if (st != NDI_OK) return st;
    } else if (hx.size() != d.nx || hy.size() != d.ny || hz.size() != d.nz || d.nx < need || d.ny < need || d.nz < need) {
      return fail(NDI_BAD_ARG, "unvalidated create with inconsistent sizes");
    }
    if (d.lanes == 0) return fail(NDI_BAD_ARG, "lanes must be >= 1");
    if (d.nx > MAX_KNOTS || d.ny > MAX_KNOTS || d.nz > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "too many knots");
    if (!d.data) return fail(NDI_BAD_ARG, "null data pointer");
    return NDI_OK;
  }

  // The launch geometry both strategies take: 16-byte vectors where lanes, stride and alignment allow, the axes in LDS where
  // they fit, a resident grid over the items and its stride as a (rows, vectors) carry.  `stage_knob` / `vec_knob`: the
  // strategy's NDI_*_STAGE / NDI_*_VEC.
  struct Geometry {
    bool wide, stage;
    int vec;
    size_t shmem;
    uint64_t vpr, step_rows, step_vecs;
    unsigned grid;
  };
  Geometry geometry(int stage_knob, int vec_knob, const void* table, const T* out, uint64_t out_stride, uint64_t nq) const {
    constexpr int W = Wide<T>::N;
    Geometry g{};
    g.wide = vec_knob != 1 && lanes % W == 0 && out_stride % W == 0 && aligned16(table) && aligned16(out);
    g.vec = g.wide ? W : 1;
    const size_t knots = ((nx + ny + nz) * sizeof(T) + 15) & ~(size_t)15;
    g.stage = stage_knob != 0 && knots <= LDS_STAGE_LIMIT;
    g.shmem = g.stage ? knots : 0;
    g.vpr = lanes / (uint64_t)g.vec;
    g.grid = resident_grid(nq * g.vpr, BLOCK, g.shmem, BLOCK);
    const uint64_t step = (uint64_t)g.grid * BLOCK;
    g.step_rows = step / g.vpr;
    g.step_vecs = step % g.vpr;
    return g;
  }

  // The reference's error for the chunk whose lowest failing queries per axis are f[0..2], relative to query `off`: the
  // lowest index wins, x before y before z for the same query (bilinear.rs:71-80, one axis further).
  ndi_status report(const T* const q[3], int q_space, uint64_t off, const unsigned long long f[3], ndi_oob_info* info) {
    int axis = 0;
    for (int a = 1; a < 3; ++a)
      if (f[a] < f[axis]) axis = a;
    const unsigned long long index = off + f[axis];
    T v;
    if (q_space == NDI_MEM_DEVICE) NDI_HIP(hipMemcpy(&v, q[axis] + index, sizeof(T), hipMemcpyDeviceToHost));
    else v = q[axis][index];
    const ndi_status st = (mode != EX_NO) ? NDI_NAN_QUERY : NDI_OUT_OF_BOUNDS;
    if (info) {
      info->index = index;
      info->value = (double)v;
      info->axis = axis;
      info->status = st;
    }
    if (st == NDI_NAN_QUERY) return fail(st, "failed to convert NaN to usize (query %llu)", index);
    static const char* const name[3] = {"x", "y", "z"};
    return fail(st, "%s = %.17g is not in range", name[axis], (double)v);
  }

  ndi_status eval(const void* qx_, const void* qy_, const void* qz_, uint64_t nq, void* out_, uint64_t out_stride,
                  const ndi_eval_opts& o, ndi_oob_info* info) override {
    if (out_stride < lanes)
      return fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)out_stride, (unsigned long long)lanes);
    if (nq == 0) return NDI_OK;
    if (!qx_ || !qy_ || !qz_ || !out_) return fail(NDI_BAD_ARG, "null query / output pointer");
    if (info) *info = ndi_oob_info{0, 0.0, 0, NDI_OK};
    DeviceGuard dg(device);
    Range rg("ndi_interp3d_eval");
    hipStream_t s = (hipStream_t)o.stream;   // NULL = the HIP default stream
    SpaceLease lease(spaces, s);
    Workspace& ws = lease.ws;
    ws.ensure_status();
    const T* const q[3] = {(const T*)qx_, (const T*)qy_, (const T*)qz_};
    T* out = (T*)out_;
    const bool q_host = o.q_memspace == NDI_MEM_HOST, out_host = o.out_memspace == NDI_MEM_HOST;
    const uint64_t row_bytes = lanes * sizeof(T);
    // host arrays travel through device staging in row chunks; a batch on device pointers is one chunk
    const uint64_t chunk =
        (q_host || out_host) ? std::max<uint64_t>(1, std::min<uint64_t>(nq, trilinear_knobs().chunk_bytes / row_bytes)) : nq;
    const uint64_t q_pitch = (chunk * sizeof(T) + 255) & ~(uint64_t)255;   // [qx | qy | qz] in one staging buffer
    if (q_host) ws.qdev.reserve(3 * q_pitch);
    if (out_host) ws.stage.reserve(chunk * row_bytes);
    for (uint64_t off = 0; off < nq; off += chunk) {
      const uint64_t rows = std::min<uint64_t>(chunk, nq - off);
      const T* qd[3] = {q[0] + off, q[1] + off, q[2] + off};
      if (q_host)
        for (int a = 0; a < 3; ++a) {
          T* dst = reinterpret_cast<T*>((char*)ws.qdev.p + a * q_pitch);
          NDI_HIP(hipMemcpyAsync(dst, qd[a], rows * sizeof(T), hipMemcpyHostToDevice, s));
          qd[a] = dst;
        }
      T* od = out_host ? ws.stage.as<T>() : out + off * out_stride;
      const uint64_t os = out_host ? lanes : out_stride;
      const bool check = out_host || (o.flags & NDI_EVAL_FRESH_OUTPUT) != 0;
      enqueue(s, ws, qd[0], qd[1], qd[2], rows, od, os, check);
      TrilinearStatus* hs = reinterpret_cast<TrilinearStatus*>(ws.host_status);
      NDI_HIP(hipMemcpyAsync(hs, ws.sc[0].status.p, sizeof(TrilinearStatus), hipMemcpyDeviceToHost, s));
      NDI_HIP(hipStreamSynchronize(s));
      const unsigned long long f[3] = {hs->first_fail[0], hs->first_fail[1], hs->first_fail[2]};
      const unsigned long long first = std::min({f[0], f[1], f[2]});
      const uint64_t good = first == NO_FAIL ? rows : std::min<uint64_t>(rows, first);
      if (out_host && good)   // only the rows before the failing query reach the caller
        NDI_HIP(hipMemcpy2D(out + off * out_stride, out_stride * sizeof(T), ws.stage.p, row_bytes, row_bytes, good,
                            hipMemcpyDeviceToHost));
      if (first != NO_FAIL) return report(q, o.q_memspace, off, f, info);
    }
    return NDI_OK;
  }
};

template <class T>
struct Interp3DImpl final : Interp3DDriver<T> {
  using D = Interp3DDriver<T>;
  DevBuf data;                 // T[nx][ny][nz][lanes]

  void enqueue(hipStream_t s, Workspace& ws, const T* qx, const T* qy, const T* qz, uint64_t nq, T* out, uint64_t out_stride,
               bool check) override {
    TrilinearStatus* st = D::begin_chunk(s, ws, qx, qy, qz, nq, check);
    const TrilinearKnobs K = trilinear_knobs();
    constexpr int W = Wide<T>::N;
    const typename D::Geometry G = D::geometry(K.stage, K.vec, data.p, out, out_stride, nq);
    TrilinearArgs<T> A{};
    A.x = D::dev_axis(0); A.y = D::dev_axis(1); A.z = D::dev_axis(2);
    A.data = data.as<T>();
    A.qx = qx; A.qy = qy; A.qz = qz;
    A.out = out;
    A.nq = nq; A.lanes = D::lanes; A.out_stride = out_stride;
    A.vpr = G.vpr;
    A.step_rows = G.step_rows;
    A.step_vecs = G.step_vecs;
    A.nx = (uint32_t)D::nx; A.ny = (uint32_t)D::ny; A.nz = (uint32_t)D::nz;
    A.mode = D::mode;
    A.first_fail = &st->first_fail[0];
    if (trace_plan())
      std::fprintf(stderr, "[ndi plan] trilinear vec=%d stage=%d check=%d grid=%u\n", G.vec, (int)G.stage, (int)check, G.grid);
    pick_bool(G.wide, [&](auto wide_) {
      constexpr int VEC = wide_ ? W : 1;
      pick_bool(G.stage, [&](auto stage_) {
        constexpr bool STAGE = stage_;
        pick_bool(check, [&](auto check_) {
          constexpr bool CHECK = check_;
          auto kern = eval_trilinear_kernel<T, VEC, STAGE, CHECK>;
          if constexpr (STAGE) allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)LDS_STAGE_LIMIT);
          launch1<T>(s, PC_EVAL, dim3(G.grid), dim3(BLOCK), G.shmem, kern, A);
        });
      });
    });
  }

  ndi_status clone_to(int dev, Interp3DBase** out) override {
    std::unique_ptr<Interp3DImpl<T>> h(new Interp3DImpl<T>());
    D::clone_driver_to(dev, *h);
    {
      DeviceGuard dg(dev);
      h->data.reserve(data.bytes);
    }
    copy_across_devices(h->data.p, dev, data.p, D::device, data.bytes);
    *out = h.release();
    return NDI_OK;
  }
};

template <class T>
static ndi_status create3d(const ndi_interp3d_desc& d, Interp3DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp3d_create");
  std::unique_ptr<Interp3DImpl<T>> h(new Interp3DImpl<T>());
  if (const ndi_status st = h->take_desc(d, 2); st != NDI_OK) return st;
  h->upload_axes();
  const size_t bytes = (size_t)d.nx * d.ny * d.nz * d.lanes * sizeof(T);
  h->data.reserve(bytes);
  NDI_HIP(hipMemcpy(h->data.p, d.data, bytes, d.memspace == NDI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  *out = h.release();
  return NDI_OK;
}
