// csrc/bicubic_local_kernels.hpp -- node derivatives of the 2-D Bicubic strategy from a LOCAL rule (Pchip, Akima) or from
// the caller (ndi_interp2d_create_bicubic_local, ndi_interp2d_create_bicubic_hermite), f32 / f64.
//
// Everything downstream of the node table {z, zx, zy, zxy} (eval_bicubic_kernel and its partial forms, the jet, the prefix
// tables) does not care where the derivatives came from.  The spline chooses them by three Thomas solves; a local rule
// needs at most five neighbours along one axis per node derivative, so its build is a stencil that writes the packed
// table T[nx][ny][4][C] directly: no recurrence, no transposed copies, no grid-sized temporaries.
//
//   bicubic_local_kernel<T, RULE, VN, PASS>   one thread per node and lane (or 16-byte vector of lanes); consecutive
//                                             threads on consecutive lanes, then consecutive j, so the x-neighbour loads
//                                             (stride ny C) and the y-neighbour loads (stride C) are each coalesced
//                                             across the wavefront.
//                                             PASS 0: z, zx = RULE(x) down the column, zy = RULE(y) along the row
//                                             PASS 1: zxy = RULE(y) on the zx slots of the row's records (stride 4 C),
//                                                     which PASS 0 -- an earlier launch on the same stream -- wrote
//   pack_nodes_grid_kernel<T>                 the caller's z, zx, zy, zxy, all in grid order -> the node table
//                                             (pack_nodes_kernel takes zy, zxy transposed, as the spline build has them)
//
// Numerical contract (include/ndinterp.h, ndi_interp2d_create_bicubic_local): k = RULE(knots, column) is ndi_strategy1d's
// rule, every line one IEEE operation in T in its order, nothing fused.  The arithmetic is hermite_kernels.hpp's
// (pchip_interior, pchip_edge, akima_knot, akima_extend); this file only picks the window of a knot.
#pragma once

namespace ndi {

template <class T>
struct BicubicLocalArgs {
  const T* z;       // [nx][ny][C] (PASS 0)
  const T* x;       // [nx] knots (the pyramids' level 0)
  const T* y;       // [ny]
  T* table;         // [nx][ny][4][C]
  uint64_t nx, ny, lanes;
};

// The rule's derivative at knot `kn` of the column col[r * stride], r = 0 .. n-1 (VN lanes of it), on `knots`.
// The window is the one hermite_entry forms for an interval: interval i = kn, or n-2 for the last knot, whose derivative is
// that interval's right one.  Rows that do not exist are not read, and neither are rows the knot's own formula leaves out.
template <class T, int RULE, int VN>
__device__ __forceinline__ typename VecT<T, VN>::type local_knot(const T* col, uint64_t stride, const T* knots, uint64_t n,
                                                                 uint64_t kn) {
  using V = typename VecT<T, VN>::type;
  static_assert(RULE == HR_PCHIP || RULE == HR_AKIMA, "a local rule");
  constexpr int HALO = RULE == HR_AKIMA ? 2 : 1;
  constexpr int ROWS = 2 + 2 * HALO;
  const bool last = kn + 1 == n;
  const uint64_t i = last ? n - 2 : kn;
  V y[ROWS];
  T xs[ROWS];
#pragma unroll
  for (int w = 0; w < ROWS; ++w) {
    bool ok = i + w >= (uint64_t)HALO && i + w - HALO < n;
    if constexpr (RULE == HR_AKIMA) ok = ok && (last ? w != 0 : w != ROWS - 1);   // m_{i-2} / m_{i+2}: the other knot's
    else ok = ok && (w != ROWS - 1 || kn == 0);                                   // delta_{i+1}: the left end's formula only
    y[w] = V(0);
    xs[w] = T(0);
    if (ok) {
      const uint64_t r = NDI_CHK(i + w - HALO, n, BC_INTERVAL);
      y[w] = *reinterpret_cast<const V*>(col + r * stride);
      xs[w] = const_load(knots, r);
    }
  }
  constexpr int ND = ROWS - 1;           // slopes delta_{i-HALO} .. delta_{i+HALO}; [HALO] is interval i's
  T h[ND];
  V dl[ND];
#pragma unroll
  for (int w = 0; w < ND; ++w) {
    h[w] = xs[w + 1] - xs[w];
    dl[w] = (y[w + 1] - y[w]) / h[w];    // (rows that were not read give 0 / 0 here; never used below)
  }
  V k;
#pragma unroll
  for (int c = 0; c < VN; ++c) {
    T r;
    if constexpr (RULE == HR_PCHIP) {
      const T d0 = hermite_get<T, VN>(dl[0], c), d1 = hermite_get<T, VN>(dl[1], c), d2 = hermite_get<T, VN>(dl[2], c);
      if (n == 2) r = d1;
      else if (last) r = pchip_edge(h[1], h[0], d1, d0);
      else if (kn == 0) r = pchip_edge(h[1], h[2], d1, d2);
      else r = pchip_interior(h[0], h[1], d0, d1);
    } else {
      T m[5];
#pragma unroll
      for (int w = 0; w < 5; ++w) m[w] = hermite_get<T, VN>(dl[w], c);
      akima_extend(m, i, n);
      r = last ? akima_knot(m[1], m[2], m[3], m[4]) : akima_knot(m[0], m[1], m[2], m[3]);
    }
    hermite_set<T, VN>(k, c, r);
  }
  return k;
}

template <class T, int RULE, int VN, int PASS>
__global__ __launch_bounds__(BLOCK) void bicubic_local_kernel(BicubicLocalArgs<T> A) {
  using V = typename VecT<T, VN>::type;
  const uint64_t C = A.lanes, LV = C / VN, nodes = A.nx * A.ny, total = nodes * LV;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    uint64_t node, lv, i, j;
    if (total <= 0xffffffffull) {          // (32-bit divisions where they serve: uniform branch)
      const uint32_t nd = LV == 1 ? (uint32_t)e : (uint32_t)e / (uint32_t)LV;
      const uint32_t q = nd / (uint32_t)A.ny;
      node = nd;
      lv = (uint32_t)e - nd * (uint32_t)LV;
      i = q;
      j = nd - q * (uint32_t)A.ny;
    } else {
      node = e / LV;
      lv = e - node * LV;
      i = node / A.ny;
      j = node - i * A.ny;
    }
    node = NDI_CHK(node, nodes, BC_INTERVAL);
    i = NDI_CHK(i, A.nx, BC_CELL_X);       // (node indices here: the limits are nx, ny)
    j = NDI_CHK(j, A.ny, BC_CELL_Y);
    const uint64_t col = lv * VN;
    T* rec = A.table + node * 4 * C + col;
    if constexpr (PASS == 0) {
      *reinterpret_cast<V*>(rec) = *reinterpret_cast<const V*>(A.z + node * C + col);
      *reinterpret_cast<V*>(rec + C) = local_knot<T, RULE, VN>(A.z + j * C + col, A.ny * C, A.x, A.nx, i);
      *reinterpret_cast<V*>(rec + 2 * C) = local_knot<T, RULE, VN>(A.z + i * A.ny * C + col, C, A.y, A.ny, j);
    } else {
      *reinterpret_cast<V*>(rec + 3 * C) = local_knot<T, RULE, VN>(A.table + i * A.ny * 4 * C + C + col, 4 * C, A.y, A.ny, j);
    }
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void pack_nodes_grid_kernel(const T* z, const T* zx, const T* zy, const T* zxy, T* table,
                                                                uint64_t nodes, uint64_t L) {
  const uint64_t total = nodes * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {   // e: element of z
    const uint64_t node = NDI_CHK(e / L, nodes, BC_INTERVAL), c = e - node * L;
    T* rec = table + node * 4 * L + c;
    rec[0] = z[e];
    rec[L] = zx[e];
    rec[2 * L] = zy[e];
    rec[3 * L] = zxy[e];
  }
}

}  // namespace ndi
