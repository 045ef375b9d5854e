// csrc/bicubic_host.hpp -- host side of the 2-D Bicubic strategy (included by ndinterp_api.hip after Interp2DImpl).
//
// A Bicubic handle IS an Interp2DImpl (bicubic == true, `table` instead of `data`): eval, async_launch / finish, the ring,
// the sharded calls, trim and clone are the Bilinear code; only the plan (Plan2::BICUBIC: range pre-pass unless the output
// is fresh, then eval_bicubic_kernel) and the build below are its own.  A partial-derivative handle
// (ndi_interp2d_partial, Interp2DImpl::partial) is the same again with the orders nu_x, nu_y set and the node table shared
// with its source: bicubic_launch_eval picks the kernel instance of the orders, nothing else knows about them.
//
// Build: three 1-D CubicSpline builds in the reference operation order (NDI_BUILD_REFERENCE_ORDER: the serial kernels,
// bit-identical to the reference for every shape) followed by the derivative rule (derivative_build_kernel):
//   x-pass  knots x on z viewed as (nx, ny L)                        -> zx
//   y-pass  knots y on the transposed copy zT viewed as (ny, nx L)   -> zyT
//   cross   knots y on the transposed copy of zx, end values 0       -> zxyT
// then one pack into the node table.  Everything is launched on the NULL stream and complete when create returns; the
// temporaries are freed before that.
// A pass along a periodic axis (ndi_interp2d_create_bicubic_periodic) is the same temporary 1-D handle built with
// periodic = 1 -- the reference's cyclic system, or its closed form on 3 knots -- and the cross pass along a periodic y is
// that pass on zx: no solver of its own.  Its last row is then a copy of its first (the same knot derivative, rounded
// twice by the rule); the lanes of a pass run identical operations, so with equal first and last data rows every table
// has the same bits at index 0 and at index n-1 of a periodic axis.
#pragma once

// knot derivatives of the spline through `src` (n, lanes) on the device-resident knots: out (n, lanes)
template <class T>
static ndi_status bicubic_axis_pass(int dtype, int device, const T* knots_dev, uint64_t n, uint64_t lanes, const T* src,
                                    const ndi_boundary& left, const ndi_boundary& right, T* out, bool periodic = false) {
  ndi_interp1d_desc d{};
  d.dtype = dtype;
  d.strategy = NDI_CUBIC_SPLINE;
  d.device = device;
  d.n = n;
  d.lanes = lanes;
  d.x_len = n;
  d.x = knots_dev;
  d.data = src;
  d.memspace = NDI_MEM_DEVICE;
  d.build_flags = NDI_BUILD_REFERENCE_ORDER | BUILD_TRUE_NOT_A_KNOT;
  d.left = left;
  d.right = right;
  d.periodic = periodic ? 1 : 0;   // (the ends are not read then); a mismatch of the end rows comes back as NDI_VALUE
  Interp1DBase* base = nullptr;
  const ndi_status st = create1d<T>(d, &base);
  if (st != NDI_OK) return st;
  std::unique_ptr<Interp1DImpl<T>> h(static_cast<Interp1DImpl<T>*>(base));
  DerivArgs<T> D{};
  D.y = h->data.template as<T>(); D.a = h->ca.template as<T>(); D.b = h->cb.template as<T>();
  D.x = h->pyr.view.lv0;
  D.Y = out;
  // the rule's A / B are not wanted: they overwrite a / b in place (an entry is read and written by the same thread only)
  D.A = h->ca.template as<T>(); D.B = h->cb.template as<T>();
  D.n = n; D.lanes = lanes;
  constexpr int VN = Wide<T>::N;
  const bool vec = lanes % VN == 0 && aligned16(D.y) && aligned16(D.a) && aligned16(D.b) && aligned16(D.Y);
  const uint64_t total = (n - 1) * (vec ? lanes / VN : lanes);
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
  if (vec) hipLaunchKernelGGL((derivative_build_kernel<T, VN>), dim3(grid), dim3(BLOCK), 0, (hipStream_t) nullptr, D);
  else hipLaunchKernelGGL((derivative_build_kernel<T, 1>), dim3(grid), dim3(BLOCK), 0, (hipStream_t) nullptr, D);
  NDI_HIP(hipGetLastError());
  // A periodic pass: the rule's first and last row are two roundings of the same knot derivative (the cyclic system has
  // k[n-1] = k[0]); the last row takes the first row's bits, a copy, so the table is periodic bit for bit.
  if (periodic)
    NDI_HIP(hipMemcpyAsync(out + (n - 1) * lanes, out, (size_t)lanes * sizeof(T), hipMemcpyDeviceToDevice, (hipStream_t) nullptr));
  NDI_HIP(hipStreamSynchronize(nullptr));   // the temporary handle's tables are read until here
  return NDI_OK;
}

static unsigned bicubic_copy_grid(uint64_t total) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
}

// NDI_VALUE of a periodic pass, restated for the 2-D caller: which axis, and what must be equal
static ndi_status bicubic_periodic_mismatch(ndi_status st, const char* axis, const char* what) {
  if (st != NDI_VALUE) return st;
  return fail(NDI_VALUE, "Bicubic: the %s axis is periodic, so the first and the last %s must be equal, element for element "
              "(exact equality, NaN included)", axis, what);
}

template <class T>
static ndi_status create2d_bicubic(const ndi_interp2d_desc& d, const ndi_boundary bc[4], Interp2DBase** out,
                                   int periodic_axes = 0) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp2d_create_bicubic");
  const bool per_x = (periodic_axes & 1) != 0, per_y = (periodic_axes & 2) != 0;
  std::unique_ptr<Interp2DImpl<T>> h(new Interp2DImpl<T>());
  h->dtype = d.dtype;
  h->device = d.device;
  h->mode = d.extrapolate ? EX_YES : EX_NO;
  h->nx = d.nx;
  h->ny = d.ny;
  h->lanes = d.lanes;
  h->bicubic = true;
  h->periodic_axes = periodic_axes;
  std::vector<T> x = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.nx);
  std::vector<T> y = d.y ? fetch_axis<T>(d.y, d.y_len, d.memspace) : default_axis<T>(d.ny);
  if (const ndi_status st = check_desc_2d(d, x.data(), y.data()); st != NDI_OK) return st;
  h->px.upload(x.data(), d.nx);
  h->py.upload(y.data(), d.ny);
  const uint64_t nx = d.nx, ny = d.ny, L = d.lanes, total = nx * ny * L;
  const size_t bytes = (size_t)total * sizeof(T);
  DevBuf zup;
  const T* z = static_cast<const T*>(d.data);
  if (d.memspace != NDI_MEM_DEVICE) {
    zup.reserve(bytes);
    NDI_HIP(hipMemcpy(zup.p, d.data, bytes, hipMemcpyHostToDevice));
    z = zup.as<T>();
  }
  const unsigned g = bicubic_copy_grid(total);
  hipStream_t s0 = nullptr;
  DevBuf zx, zyT, zxyT;
  zx.reserve(bytes);
  ndi_status st = bicubic_axis_pass<T>(d.dtype, d.device, h->px.view.lv0, nx, ny * L, z, bc[0], bc[1], zx.as<T>(), per_x);
  if (st != NDI_OK) return bicubic_periodic_mismatch(st, "x", "data row (z[0][j][c] and z[nx-1][j][c])");
  {
    DevBuf tr;                               // the transposed copy the y-passes read: z, then zx
    tr.reserve(bytes);
    zyT.reserve(bytes);
    hipLaunchKernelGGL(transpose_nodes_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, z, tr.as<T>(), nx, ny, L);
    NDI_HIP(hipGetLastError());
    st = bicubic_axis_pass<T>(d.dtype, d.device, h->py.view.lv0, ny, nx * L, tr.as<T>(), bc[2], bc[3], zyT.as<T>(), per_y);
    if (st != NDI_OK) return bicubic_periodic_mismatch(st, "y", "data column (z[i][0][c] and z[i][ny-1][c])");
    zxyT.reserve(bytes);
    hipLaunchKernelGGL(transpose_nodes_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, (const T*)zx.as<T>(), tr.as<T>(), nx, ny, L);
    NDI_HIP(hipGetLastError());
    // zx's own end condition along y: the x-derivative of a constant end value is 0, so the same kinds with value 0
    ndi_boundary cl = bc[2], cr = bc[3];
    cl.value = 0.0;
    cr.value = 0.0;
    st = bicubic_axis_pass<T>(d.dtype, d.device, h->py.view.lv0, ny, nx * L, tr.as<T>(), cl, cr, zxyT.as<T>(), per_y);
    if (st != NDI_OK) return bicubic_periodic_mismatch(st, "y", "column of zx (a NaN among the x-derivatives)");
  }
  h->table = std::make_shared<DevBuf>();
  h->table->reserve(4 * bytes);
  hipLaunchKernelGGL(pack_nodes_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, z, (const T*)zx.as<T>(), (const T*)zyT.as<T>(),
                     (const T*)zxyT.as<T>(), h->table->template as<T>(), nx, ny, L);
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipStreamSynchronize(s0));         // the table is complete when create returns: any stream may read it
  *out = h.release();
  return NDI_OK;
}

// The vector-width x knots-in-LDS ladder of the three Bicubic launchers (surface, integral, jet): f(Int<VEC>, KLDS).
template <class T, class F>
static void bicubic_pick_form(bool vec, bool klds, F&& f) {
  pick_or<1, Wide<T>::N>(vec ? Wide<T>::N : 1, [&](auto vec_) { pick_bool(klds, [&](auto kl_) { f(vec_, kl_); }); });
}

// Plan2::BICUBIC: the launch (the range pre-pass, when there is one, was enqueued by prep)
template <class T>
static void bicubic_launch_eval(const Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const T* qx, const T* qy,
                                uint64_t nq, T* out, uint64_t out_stride, bool check) {
  constexpr int VN = Wide<T>::N;
  constexpr unsigned TB = 256;
  const bool vec = (h.lanes % VN == 0) && (out_stride % VN == 0) && aligned16(out);
  BicubicArgs<T> A{};
  A.px = h.px.view; A.py = h.py.view;
  A.table = h.table->template as<T>();
  A.qx = qx; A.qy = qy;
  A.out = out;
  A.nq = nq;
  A.out_stride = out_stride;
  A.lv = vec ? h.lanes / VN : h.lanes;
  A.lv_magic = (A.lv >= 2 && A.lv < 64) ? (uint32_t)(((1ull << 32) + A.lv - 1) / A.lv) : 0u;
  // rows of 64 vectors and more are cut along blockIdx.y: 512 vectors per piece, more when that would pass the grid limit
  uint64_t vchunk = 512;
  while ((A.lv + vchunk - 1) / vchunk > 32768) vchunk *= 2;
  A.vchunk = (uint32_t)vchunk;
  const unsigned gy = (unsigned)((A.lv + vchunk - 1) / vchunk);
  A.mode = h.mode;
  A.wrap = h.wrap_axes();
  A.first_fail = &st->first_fail[0];
  A.check = check ? 1 : 0;
  const size_t strips = (size_t)(TB / 64) * 64 * (sizeof(unsigned long long) + 4 * sizeof(T));
  const size_t knots = (h.px.lds_bytes + h.py.lds_bytes + 15) & ~(size_t)15;
  const bool klds = knots + strips <= LDS_STAGE_LIMIT;
  const size_t lds = (klds ? knots : 0) + strips;
  // staging the axes is the fixed cost of a workgroup: no more workgroups than a few per resident slot
  const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + TB - 1) / TB,
                                                                        std::max<uint64_t>(1, (uint64_t)cu_count() * wgs_per_cu(lds, TB) * 4 / gy)));
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] bicubic vec=%d lv=%llu klds=%d grid=%u x %u lds=%zu prepass=%d guess=%d,%d levels=%d,%d "
                 "nu=%d,%d%s\n",
                 (int)vec, (unsigned long long)A.lv, (int)klds, gx, gy, lds, check ? 0 : 1, A.px.guess, A.py.guess,
                 A.px.levels, A.py.levels, h.nu_x, h.nu_y,
                 A.wrap == 0 ? "" : A.wrap == 1 ? " wrap=x" : A.wrap == 2 ? " wrap=y" : " wrap=xy");   // (the line as it was, else)
  // the orders were checked when the handle was made (Interp2DImpl::partial): 0 .. 2 each
  const bool known = pick<0, 1, 2, 3, 4, 5, 6, 7, 8>(h.nu_x * 3 + h.nu_y, [&](auto nu_) {
    constexpr int NX = nu_ / 3, NY = nu_ % 3;
    // a handle that wraps takes the WRAP variant; every other handle the instance it always took
    pick_bool(A.wrap != 0, [&](auto wrap_) {
      bicubic_pick_form<T>(vec, klds, [&](auto vec_, auto kl_) {
        launch_lds<T>(eval_bicubic_kernel<T, vec_, kl_, TB, NX, NY, wrap_>, LDS_STAGE_LIMIT, s, PC_EVAL, dim3(gx, gy), dim3(TB),
                      lds, A);
      });
    });
  });
  if (!known) throw HipFailure{hipErrorInvalidValue, "bicubic_launch_eval: partial orders outside 0 .. 2", __LINE__};
}

// ndi_interp2d_tables: zx, zy, zxy as plain [nx][ny][lanes] arrays (any of them may be NULL)
template <class T>
static ndi_status bicubic_tables(const Interp2DImpl<T>& h, void* zx, void* zy, void* zxy, int memspace) {
  DeviceGuard dg(h.device);
  const uint64_t nodes = h.nx * h.ny, total = nodes * h.lanes;
  const size_t bytes = (size_t)total * sizeof(T);
  void* dst[3] = {zx, zy, zxy};
  DevBuf tmp[3];
  T* dev[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3; ++k) {
    if (!dst[k]) continue;
    if (memspace == NDI_MEM_DEVICE) {
      dev[k] = static_cast<T*>(dst[k]);
    } else {
      tmp[k].reserve(bytes);
      dev[k] = tmp[k].template as<T>();
    }
  }
  hipLaunchKernelGGL(unpack_nodes_kernel<T>, dim3(bicubic_copy_grid(total)), dim3(BLOCK), 0, (hipStream_t) nullptr,
                     (const T*)h.table->template as<T>(), dev[0], dev[1], dev[2], nodes, h.lanes);
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipStreamSynchronize(nullptr));
  if (memspace != NDI_MEM_DEVICE)
    for (int k = 0; k < 3; ++k)
      if (dst[k]) NDI_HIP(hipMemcpy(dst[k], dev[k], bytes, hipMemcpyDeviceToHost));
  return NDI_OK;
}

