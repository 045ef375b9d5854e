// csrc/bicubic_local_host.hpp -- host side of the Bicubic handles whose node derivatives come from a local rule or from
// the caller (ndi_interp2d_create_bicubic_local, ndi_interp2d_create_bicubic_hermite); included by ndinterp_api.hip after
// bicubic_host.hpp.
//
// The handle is the Bicubic Interp2DImpl of create2d_bicubic (bicubic == true, orders (0, 0)): only the build differs.
//   HR_PCHIP / HR_AKIMA  two launches of bicubic_local_kernel on the NULL stream: PASS 0 writes z, zx, zy into the node
//                        table, PASS 1 forms zxy from the zx slots PASS 0 wrote.  The only temporary is the uploaded z when
//                        the data comes from the host.
//   HR_GIVEN             pack_nodes_grid_kernel on the caller's four arrays, uploaded first when they are on the host.
// Everything is complete when create returns.
#pragma once

template <class T, int RULE>
static void bicubic_local_launch(const BicubicLocalArgs<T>& A) {
  constexpr int VN = Wide<T>::N;
  const bool vec = A.lanes % VN == 0 && aligned16(A.z) && aligned16(A.table);
  const uint64_t total = A.nx * A.ny * (vec ? A.lanes / VN : A.lanes);
  const dim3 g(bicubic_copy_grid(total)), b(BLOCK);
  hipStream_t s0 = nullptr;
  if (vec) {
    hipLaunchKernelGGL((bicubic_local_kernel<T, RULE, VN, 0>), g, b, 0, s0, A);
    hipLaunchKernelGGL((bicubic_local_kernel<T, RULE, VN, 1>), g, b, 0, s0, A);
  } else {
    hipLaunchKernelGGL((bicubic_local_kernel<T, RULE, 1, 0>), g, b, 0, s0, A);
    hipLaunchKernelGGL((bicubic_local_kernel<T, RULE, 1, 1>), g, b, 0, s0, A);
  }
}

// rule: HR_PCHIP, HR_AKIMA (zx, zy, zxy unused) or HR_GIVEN (the caller's tables, in d.memspace)
template <class T>
static ndi_status create2d_bicubic_local(const ndi_interp2d_desc& d, int rule, const void* zx, const void* zy, const void* zxy,
                                         Interp2DBase** out) {
  DeviceGuard dg(d.device);
  Range rg(rule == HR_GIVEN ? "ndi_interp2d_create_bicubic_hermite" : "ndi_interp2d_create_bicubic_local");
  std::unique_ptr<Interp2DImpl<T>> h(new Interp2DImpl<T>());
  h->dtype = d.dtype;
  h->device = d.device;
  h->mode = d.extrapolate ? EX_YES : EX_NO;
  h->nx = d.nx;
  h->ny = d.ny;
  h->lanes = d.lanes;
  h->bicubic = true;
  std::vector<T> x = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.nx);
  std::vector<T> y = d.y ? fetch_axis<T>(d.y, d.y_len, d.memspace) : default_axis<T>(d.ny);
  if (const ndi_status st = check_desc_2d(d, x.data(), y.data()); st != NDI_OK) return st;
  h->px.upload(x.data(), d.nx);
  h->py.upload(y.data(), d.ny);
  const uint64_t nodes = d.nx * d.ny, total = nodes * d.lanes;
  const size_t bytes = (size_t)total * sizeof(T);
  const int n_src = rule == HR_GIVEN ? 4 : 1;
  const void* given[4] = {d.data, zx, zy, zxy};
  const T* src[4] = {nullptr, nullptr, nullptr, nullptr};
  DevBuf up[4];
  for (int k = 0; k < n_src; ++k) {
    src[k] = static_cast<const T*>(given[k]);
    if (d.memspace != NDI_MEM_DEVICE) {
      up[k].reserve(bytes);
      NDI_HIP(hipMemcpy(up[k].p, given[k], bytes, hipMemcpyHostToDevice));
      src[k] = up[k].template as<T>();
    }
  }
  h->table = std::make_shared<DevBuf>();
  h->table->reserve(4 * bytes);
  hipStream_t s0 = nullptr;
  if (rule == HR_GIVEN) {
    hipLaunchKernelGGL(pack_nodes_grid_kernel<T>, dim3(bicubic_copy_grid(total)), dim3(BLOCK), 0, s0, src[0], src[1], src[2],
                       src[3], h->table->template as<T>(), nodes, (uint64_t)d.lanes);
  } else {
    BicubicLocalArgs<T> A{};
    A.z = src[0];
    A.x = h->px.view.lv0;
    A.y = h->py.view.lv0;
    A.table = h->table->template as<T>();
    A.nx = d.nx; A.ny = d.ny; A.lanes = d.lanes;
    if (rule == HR_PCHIP) bicubic_local_launch<T, HR_PCHIP>(A);
    else bicubic_local_launch<T, HR_AKIMA>(A);
  }
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipStreamSynchronize(s0));         // the table is complete when create returns: any stream may read it
  *out = h.release();
  return NDI_OK;
}
