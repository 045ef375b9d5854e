// csrc/tricubic_host.hpp -- the host side of the Tricubic strategy of the 3-D handles (ndi_interp3d_create_tricubic,
// ndi_interp3d_tables; include/ndinterp3d_cubic.h); included by ndinterp_api.hip inside namespace ndi, after bicubic_host.hpp
// (bicubic_axis_pass) and trilinear_host.hpp (Interp3DDriver).
//
// A Tricubic handle is an Interp3DDriver<T> with the node table T[nx][ny][nz][8][lanes] instead of the grid: eval, the
// staging chunks, the status read-back and the report are the driver's; the plan line, the knobs and the launch are its own.
//
// Build: seven bicubic_axis_pass calls -- the reference-order CubicSpline build with the true not-a-knot
// right row, then the derivative rule's Y -- on views of the grid.  Lanes are independent and run identical operations, so a
// transposed layout gives the same bits:
//   x-pass    on (nx, ny nz L), as the grid lies
//   y-passes  on transpose_nodes_kernel copies (nx, ny, nz L) -> (ny, nx, nz L)
//   z-passes  on transpose_nodes_kernel copies of the view (nx ny, nz, L) -> (nz, nx ny, L)
// in the order fx, fy, fz (from f), fxy, fxz (from fx), fyz (from fy), fxyz (from fxy); a pass on a derivative table takes the
// axis' end kinds with value 0.  Every result is packed into its part of the node table as soon as it exists
// (pack_nodes3_kernel reads the layout the pass left it in) and a later pass reads its source back out of the table
// (unpack_nodes3_kernel), so three work grids serve the whole build:
//   A  the source in grid order (host data are uploaded into it; device data are read where they lie until fz is done)
//   B  its transposed copy                C  the pass' result
// Device memory at the peak: the table (8 grids), A, B, C and the temporary 1-D handle of the running pass (its copy of the
// source and its two coefficient tables, about 3 grids): about 14 grids.  Everything is launched on the NULL stream and
// complete when create returns; the temporaries are freed before that.
//
// Plan: ONE launch of eval_tricubic_kernel<T, VEC, STAGE, CHECK> per chunk, VEC / STAGE / CHECK chosen by Trilinear's rules
// (trilinear_host.hpp).  Knobs (through NDI_TUNE_LIVE like the others):
//   NDI_TRICUBIC_STAGE    unset / -1 = auto, 0 = never, 1 = where it fits (the same as auto; kept for A/B)
//   NDI_TRICUBIC_VEC      unset / -1 = auto, 1 = single elements
// The staging chunk of a call on host arrays is NDI_TRILINEAR_CHUNK, shared with Trilinear.
#pragma once

struct TricubicKnobs {
  int stage, vec;
};
static TricubicKnobs tricubic_knobs() {
  static const Knob stage{"NDI_TRICUBIC_STAGE", -1, Knob::live}, vec{"NDI_TRICUBIC_VEC", -1, Knob::live};
  return {stage.get(), vec.get()};
}

// ndi_interp3d_tables' order fx, fy, fz, fxy, fxz, fyz, fxyz as parts of the node table (p = 4 [dx] + 2 [dy] + [dz])
constexpr int TRICUBIC_TABLE_PART[7] = {4, 2, 1, 6, 5, 3, 7};

template <class T>
struct Tricubic3DImpl final : Interp3DDriver<T> {
  using D = Interp3DDriver<T>;
  DevBuf table;                // T[nx][ny][nz][8][lanes]

  uint64_t nodes() const { return D::nx * D::ny * D::nz; }

  void enqueue(hipStream_t s, Workspace& ws, const T* qx, const T* qy, const T* qz, uint64_t nq, T* out, uint64_t out_stride,
               bool check) override {
    TrilinearStatus* st = D::begin_chunk(s, ws, qx, qy, qz, nq, check);
    const TricubicKnobs K = tricubic_knobs();
    constexpr int W = Wide<T>::N;
    const typename D::Geometry G = D::geometry(K.stage, K.vec, table.p, out, out_stride, nq);
    TricubicArgs<T> A{};
    A.x = D::dev_axis(0); A.y = D::dev_axis(1); A.z = D::dev_axis(2);
    A.table = table.as<T>();
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
      std::fprintf(stderr, "[ndi plan] tricubic vec=%d stage=%d check=%d grid=%u\n", G.vec, (int)G.stage, (int)check, G.grid);
    pick_bool(G.wide, [&](auto wide_) {
      constexpr int VEC = wide_ ? W : 1;
      pick_bool(G.stage, [&](auto stage_) {
        constexpr bool STAGE = stage_;
        pick_bool(check, [&](auto check_) {
          constexpr bool CHECK = check_;
          auto kern = eval_tricubic_kernel<T, VEC, STAGE, CHECK>;
          if constexpr (STAGE) allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)LDS_STAGE_LIMIT);
          launch1<T>(s, PC_EVAL, dim3(G.grid), dim3(BLOCK), G.shmem, kern, A);
        });
      });
    });
  }

  ndi_status clone_to(int dev, Interp3DBase** out) override {
    std::unique_ptr<Tricubic3DImpl<T>> h(new Tricubic3DImpl<T>());
    D::clone_driver_to(dev, *h);
    {
      DeviceGuard dg(dev);
      h->table.reserve(table.bytes);
    }
    copy_across_devices(h->table.p, dev, table.p, D::device, table.bytes);
    *out = h.release();
    return NDI_OK;
  }

  // ndi_interp3d_tables: fx, fy, fz, fxy, fxz, fyz, fxyz as plain [nx][ny][nz][lanes] arrays (any of them may be NULL);
  // host arrays go through ONE staging grid, a table at a time
  ndi_status tables(void* const t[7], int memspace) override {
    DeviceGuard dg(D::device);
    const uint64_t total = nodes() * D::lanes;
    const size_t bytes = (size_t)total * sizeof(T);
    DevBuf tmp;
    for (int k = 0; k < 7; ++k) {
      if (!t[k]) continue;
      T* dev = static_cast<T*>(t[k]);
      if (memspace != NDI_MEM_DEVICE) {
        tmp.reserve(bytes);
        dev = tmp.as<T>();
      }
      hipLaunchKernelGGL(unpack_nodes3_kernel<T>, dim3(bicubic_copy_grid(total)), dim3(BLOCK), 0, (hipStream_t) nullptr,
                         (const T*)table.as<T>(), TRICUBIC_TABLE_PART[k], dev, nodes(), D::lanes);
      NDI_HIP(hipGetLastError());
      NDI_HIP(hipStreamSynchronize(nullptr));
      if (memspace != NDI_MEM_DEVICE) NDI_HIP(hipMemcpy(t[k], dev, bytes, hipMemcpyDeviceToHost));
    }
    return NDI_OK;
  }
};

template <class T>
static ndi_status create3d_tricubic(const ndi_interp3d_desc& d, const ndi_boundary bc[6], Interp3DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp3d_create_tricubic");
  std::unique_ptr<Tricubic3DImpl<T>> h(new Tricubic3DImpl<T>());
  if (const ndi_status st = h->take_desc(d, 3); st != NDI_OK) return st;
  h->upload_axes();
  const uint64_t nx = d.nx, ny = d.ny, nz = d.nz, L = d.lanes, nodes = nx * ny * nz, total = nodes * L;
  const size_t bytes = (size_t)total * sizeof(T);
  const unsigned g = bicubic_copy_grid(total);
  hipStream_t s0 = nullptr;
  h->table.reserve(8 * bytes);
  T* const table = h->table.template as<T>();
  DevBuf A, B, C;
  B.reserve(bytes);
  C.reserve(bytes);
  const T* f = static_cast<const T*>(d.data);
  if (d.memspace != NDI_MEM_DEVICE) {
    A.reserve(bytes);
    NDI_HIP(hipMemcpy(A.p, d.data, bytes, hipMemcpyHostToDevice));
    f = A.as<T>();
  }
  auto pack = [&](const T* src, int layout, int part) {
    hipLaunchKernelGGL(pack_nodes3_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, src, layout, part, table, nx, ny, nz, L);
    NDI_HIP(hipGetLastError());
  };
  // the table's part `part` back in grid order, in A: the source of a pass on a derivative table
  auto source = [&](int part) -> const T* {
    A.reserve(bytes);
    hipLaunchKernelGGL(unpack_nodes3_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, (const T*)table, part, A.as<T>(), nodes, L);
    NDI_HIP(hipGetLastError());
    return A.as<T>();
  };
  // D_axis of `src` (grid order) into part `part`; `cross`: a pass on a derivative table, the end kinds with value 0
  auto pass = [&](const T* src, int axis, bool cross, int part) -> ndi_status {
    ndi_boundary l = bc[2 * axis], r = bc[2 * axis + 1];
    if (cross) {
      l.value = 0.0;
      r.value = 0.0;
    }
    const uint64_t n = axis == 0 ? nx : axis == 1 ? ny : nz;
    const T* in = src;
    if (axis != 0) {
      if (axis == 1) hipLaunchKernelGGL(transpose_nodes_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, src, B.as<T>(), nx, ny, nz * L);
      else hipLaunchKernelGGL(transpose_nodes_kernel<T>, dim3(g), dim3(BLOCK), 0, s0, src, B.as<T>(), nx * ny, nz, L);
      NDI_HIP(hipGetLastError());
      in = B.as<T>();
    }
    const ndi_status st = bicubic_axis_pass<T>(d.dtype, d.device, h->dev_axis(axis), n, total / n, in, l, r, C.as<T>());
    if (st != NDI_OK) return st;
    pack(C.as<T>(), axis == 0 ? TL_GRID : axis == 1 ? TL_Y : TL_Z, part);
    return NDI_OK;
  };
  pack(f, TL_GRID, 0);
  ndi_status st = pass(f, 0, false, 4);                      // fx  = D_x f
  if (st == NDI_OK) st = pass(f, 1, false, 2);               // fy  = D_y f
  if (st == NDI_OK) st = pass(f, 2, false, 1);               // fz  = D_z f
  if (st == NDI_OK) {
    const T* fx = source(4);
    st = pass(fx, 1, true, 6);                               // fxy = D_y fx
    if (st == NDI_OK) st = pass(fx, 2, true, 5);             // fxz = D_z fx
  }
  if (st == NDI_OK) st = pass(source(2), 2, true, 3);        // fyz = D_z fy
  if (st == NDI_OK) st = pass(source(6), 2, true, 7);        // fxyz = D_z fxy
  NDI_HIP(hipStreamSynchronize(s0));           // the table is complete when create returns: any stream may read it
  if (st != NDI_OK) return st;
  *out = h.release();
  return NDI_OK;
}
