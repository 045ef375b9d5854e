// csrc/lanewise2d_kernels.hpp -- lane-wise evaluation of the 2-D handles (ndi_interp2d_eval_lanewise): an (x, y) per lane,
//     out[j][l] = f_l(qx[j][l], qy[j][l]).
//
// Value rule (include/ndinterp.h): out[j][l] is, bit for bit, element l of the row ndi_interp2d_eval writes for the single
// query (qx[j][l], qy[j][l]).  The kernels get it by construction: both searches are locate_index (the unique clamped
// cell), the wrap is bicubic_wrap_query once per coordinate before the search, the Bicubic point is hermite_nu<NUY> four
// times and hermite_nu<NUX> once on the t, u, hx, hy of eval_bicubic_kernel, the Bilinear point is bilinear.rs:88-97 with
// plain IEEE divisions (frac_v: the bits div_shared reproduces); nothing re-associated.
//
// Mapping: lanewise_kernels.hpp's -- one thread per output ELEMENT e = j * lanes + l, lanes fastest, so a wavefront's two
// query loads and its store coalesce; LanewiseGeom / LanewisePos unchanged (one 64-bit division per thread before the loop,
// a carry per trip); wave-uniform trip count, because both searches are wave-cooperative (inactive lanes take part with
// the first knots).  Each thread keeps its own t, u, hx, hy: there is no per-wave LDS strip.
//
//   eval_lanewise2d_kernel<T, KIND, STAGE, REC, NUX, NUY, WRAP>
//                               KIND: Bilinear (four element reads through the handle's layout, plain or pair-packed) or
//                               Bicubic (sixteen element reads of the node table T[nx][ny][4][lanes], whose four parts of
//                               a node lie `lanes` elements apart -- or, REC, four aligned node-record loads).  STAGE:
//                               both knot pyramids in LDS (else read from global memory).  NUX, NUY: the partial orders
//                               of a Bicubic handle.  WRAP: the variant of a handle that wraps on a periodic axis; every
//                               other instance compiles none of it.
//   lanewise2d_check_kernel     the pre-pass, lanewise_check_kernel's geometry: the lowest failing flat element index per
//                               axis (first_fail[0]: x, [1]: y) by lane_check2's test, on the wrapped coordinate where the
//                               axis wraps (bicubic_wrap_check_kernel's rule: finite after the wrap)
//   lanewise2d_records_kernel   the node-record copy R[i][j][l] = {z, zx, zy, zxy}: values copied, never recomputed
#pragma once

namespace ndi {

enum Lanewise2DKind : int { LW2_BILINEAR = 0, LW2_BICUBIC = 1 };

// Rows that may be written: all of them when the kernel tests the queries itself, else the rows before the row of the
// lowest failing element of either axis (the pre-pass's).
__device__ __forceinline__ uint64_t lanewise2d_rows(const LanewiseGeom& G, const unsigned long long* first_fail, int check) {
  if (check) return G.rows;
  const unsigned long long f = first_fail[0] < first_fail[1] ? first_fail[0] : first_fail[1];
  if (f == NO_FAIL) return G.rows;
  const uint64_t r = f / G.lanes;
  return r < G.rows ? r : G.rows;
}

template <class T>
__global__ __launch_bounds__(BLOCK) void lanewise2d_records_kernel(const T* table, LanewiseRecord<T, 4>* out, uint64_t nodes,
                                                                   uint64_t lanes) {
  const uint64_t total = nodes * lanes;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
    const uint64_t node = NDI_CHK(e / lanes, nodes, BC_INTERVAL), c = e - node * lanes;
    const T* rec = table + node * 4 * lanes + c;
    LanewiseRecord<T, 4> r;
    r.v[0] = rec[0];
    r.v[1] = rec[lanes];
    r.v[2] = rec[2 * lanes];
    r.v[3] = rec[3 * lanes];
    out[e] = r;
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void lanewise2d_check_kernel(const T* qx, const T* qy, LanewiseGeom G, T x0, T xn, T y0,
                                                                 T yn, int mode, int wrap, unsigned long long* first_fail) {
  const uint64_t total = G.rows * G.lanes;
  uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= total) return;
  LanewisePos p;
  p.start(G, e);
  for (; e < total; e += (uint64_t)gridDim.x * BLOCK, p.advance(G)) {
    const uint64_t j = NDI_CHK(p.j, G.rows, BC_QUERY), l = NDI_CHK(p.l, G.lanes, BC_LANE);
    const uint64_t at = j * G.q_stride + l;
    // (a handle that wraps extrapolates: lane_check2 then tests "not NaN", on the wrapped coordinate of a wrapping axis)
    const T xs = bicubic_wrap_query<T>(qx[at], x0, xn, (wrap & 1) != 0);
    const T ys = bicubic_wrap_query<T>(qy[at], y0, yn, (wrap & 2) != 0);
    lane_check2<T>(first_fail, e, xs, ys, x0, xn, y0, yn, mode);
  }
}

template <class T>
struct Lanewise2DArgs {
  Pyramid<T> px, py;
  const T* data;         // Bilinear: the grid in the handle's layout; Bicubic: the node table T[nx][ny][4][lanes]
  const void* rec;       // Bicubic node records [nx][ny][lanes] (REC), else unused
  const T* qx;           // [rows][q_stride]
  const T* qy;
  T* out;                // [rows][out_stride]
  LanewiseGeom G;
  uint64_t row_elems;    // Bilinear: elements between grid rows xi and xi + 1 (row_cells * cell_elems of the layout)
  uint64_t cell_elems;   // Bilinear: elements between cells (xi, yi) and (xi, yi + 1): lanes (plain) or 2 lanes (pair-packed)
  int mode;              // ExtrapMode
  int wrap;              // WRAP variants: the axes that wrap (bit 0: x, bit 1: y)
  int check;             // 1: the kernel tests the queries itself and publishes the lowest failing element per axis
  unsigned long long* first_fail;   // [2]: x, y
};

template <class T, int KIND, bool STAGE, bool REC, int NUX, int NUY, bool WRAP>
__global__ __launch_bounds__(BLOCK) void eval_lanewise2d_kernel(Lanewise2DArgs<T> A) {
  static_assert(KIND == LW2_BICUBIC || (!REC && !WRAP && NUX == 0 && NUY == 0), "Bilinear has one form per STAGE");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  using PTR = typename std::conditional<STAGE, lds_ptr<T>, const T*>::type;
  const uint32_t tid = threadIdx.x;
  const uint32_t nxa = A.px.n + A.px.n1, nya = A.py.n + A.py.n1;   // the levels of a pyramid are one allocation
  PyramidT<T, PTR> PX, PY;
  if constexpr (STAGE) {   // LDS: [x pyramid | y pyramid]
    T* sx = reinterpret_cast<T*>(smem_raw);
    T* sy = sx + nxa;
    for (uint32_t i = tid; i < nxa; i += BLOCK) sx[i] = A.px.lv0[i];
    for (uint32_t i = tid; i < nya; i += BLOCK) sy[i] = A.py.lv0[i];
    __syncthreads();
    PX.lv0 = (lds_ptr<T>)(smem_raw);
    PX.lv1 = PX.lv0 + A.px.n;
    PY.lv0 = PX.lv0 + nxa;
    PY.lv1 = PY.lv0 + A.py.n;
  } else {
    PX.lv0 = A.px.lv0; PX.lv1 = A.px.lv1;
    PY.lv0 = A.py.lv0; PY.lv1 = A.py.lv1;
  }
  PX.n = A.px.n; PX.n1 = A.px.n1; PX.levels = A.px.levels; PX.guess = A.px.guess; PX.block = A.px.block;
  PY.n = A.py.n; PY.n1 = A.py.n1; PY.levels = A.py.levels; PY.guess = A.py.guess; PY.block = A.py.block;
  const T x0 = PX.lv0[0], xn = PX.lv0[PX.n - 1], y0 = PY.lv0[0], yn = PY.lv0[PY.n - 1];
  const uint32_t lane = tid & 63u;
  const LanewiseGeom G = A.G;
  const uint64_t L = G.lanes;
  const uint64_t total = lanewise2d_rows(G, A.first_fail, A.check) * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  uint64_t base = (uint64_t)blockIdx.x * BLOCK + (tid & ~63u);   // wave-uniform: all 64 lanes run the same trips
  if (base >= total) return;                                      // (no barrier follows)
  LanewisePos p;
  p.start(G, base + lane);
  for (; base < total; base += step, p.advance(G)) {
    const uint64_t e = base + lane;
    const bool active = e < total;
    const uint64_t j = active ? NDI_CHK(p.j, G.rows, BC_QUERY) : 0, l = active ? NDI_CHK(p.l, L, BC_LANE) : 0;
    T x = active ? A.qx[j * G.q_stride + l] : x0;   // inactive lanes take part with the first knots
    T y = active ? A.qy[j * G.q_stride + l] : y0;
    if constexpr (WRAP) {                            // once per coordinate, before the search
      x = bicubic_wrap_query<T>(x, x0, xn, (A.wrap & 1) != 0);
      y = bicubic_wrap_query<T>(y, y0, yn, (A.wrap & 2) != 0);
    }
    uint32_t xi = locate_index<T, PTR>(PX, x0, xn, x, lane);   // all 64 lanes take part
    uint32_t yi = locate_index<T, PTR>(PY, y0, yn, y, lane);
    if (!active) continue;
    // lane_check2's test per axis (a handle that wraps extrapolates: "not NaN", on the wrapped coordinate)
    const bool badx = (A.mode == EX_NO) ? !((x0 <= x) && (x <= xn)) : !(x == x);
    const bool bady = (A.mode == EX_NO) ? !((y0 <= y) && (y <= yn)) : !(y == y);
    if (badx || bady) {
      if (A.check) {
        if (badx) atomicMin(&A.first_fail[0], (unsigned long long)e);
        if (bady) atomicMin(&A.first_fail[1], (unsigned long long)e);
      }
      continue;
    }
    xi = NDI_CHK(xi, PX.n - 1u, BC_CELL_X);
    yi = NDI_CHK(yi, PY.n - 1u, BC_CELL_Y);
    const T x1 = PX.lv0[xi], x2 = PX.lv0[xi + 1], y1 = PY.lv0[yi], y2 = PY.lv0[yi + 1];
    T r;
    if constexpr (KIND == LW2_BILINEAR) {
      const T* g = A.data + ((uint64_t)xi * A.row_elems + (uint64_t)yi * A.cell_elems + l);
      const T a11 = g[0], a12 = g[L], a21 = g[A.row_elems], a22 = g[A.row_elems + L];
      const T z1 = frac_v<T, T>(x1, a11, x2, a21, x);   // bilinear.rs:88-97
      const T z2 = frac_v<T, T>(x1, a12, x2, a22, x);
      r = frac_v<T, T>(y1, z1, y2, z2, y);
    } else {
      const T hx = x2 - x1, hy = y2 - y1;
      const T t = (x - x1) / hx, u = (y - y1) / hy;     // cubic_spline.rs:820's t, on each axis
      const uint64_t node = (uint64_t)xi * PY.n + yi;   // node (i, j); (i, j + 1) follows, (i + 1, j) is ny nodes on
      T z00, zx00, zy00, zxy00, z01, zx01, zy01, zxy01, z10, zx10, zy10, zxy10, z11, zx11, zy11, zxy11;
      if constexpr (REC) {
        const LanewiseRecord<T, 4>* R = static_cast<const LanewiseRecord<T, 4>*>(A.rec) + (node * L + l);
        const LanewiseRecord<T, 4> r00 = R[0], r01 = R[L], r10 = R[(uint64_t)PY.n * L], r11 = R[(uint64_t)PY.n * L + L];
        z00 = r00.v[0]; zx00 = r00.v[1]; zy00 = r00.v[2]; zxy00 = r00.v[3];
        z01 = r01.v[0]; zx01 = r01.v[1]; zy01 = r01.v[2]; zxy01 = r01.v[3];
        z10 = r10.v[0]; zx10 = r10.v[1]; zy10 = r10.v[2]; zxy10 = r10.v[3];
        z11 = r11.v[0]; zx11 = r11.v[1]; zy11 = r11.v[2]; zxy11 = r11.v[3];
      } else {
        const T* g0 = A.data + (node * 4u * L + l);
        const T* g1 = g0 + (uint64_t)PY.n * 4u * L;
        z00 = g0[0]; zx00 = g0[L]; zy00 = g0[2 * L]; zxy00 = g0[3 * L];
        z01 = g0[4 * L]; zx01 = g0[5 * L]; zy01 = g0[6 * L]; zxy01 = g0[7 * L];
        z10 = g1[0]; zx10 = g1[L]; zy10 = g1[2 * L]; zxy10 = g1[3 * L];
        z11 = g1[4 * L]; zx11 = g1[5 * L]; zy11 = g1[6 * L]; zxy11 = g1[7 * L];
      }
      const T one = T(1);
      const T cu = one - u, cu2 = u * cu, ct = one - t, ct2 = t * ct;
      const T p0 = hermite_nu<NUY, T, T>(z00, z01, zy00, zy01, hy, u, cu, cu2);
      const T p1 = hermite_nu<NUY, T, T>(z10, z11, zy10, zy11, hy, u, cu, cu2);
      const T d0 = hermite_nu<NUY, T, T>(zx00, zx01, zxy00, zxy01, hy, u, cu, cu2);
      const T d1 = hermite_nu<NUY, T, T>(zx10, zx11, zxy10, zxy11, hy, u, cu, cu2);
      r = hermite_nu<NUX, T, T>(p0, p1, d0, d1, hx, t, ct, ct2);
    }
    A.out[j * G.out_stride + l] = r;
  }
}

}  // namespace ndi
