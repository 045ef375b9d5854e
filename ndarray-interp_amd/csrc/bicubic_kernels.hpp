// csrc/bicubic_kernels.hpp -- the 2-D Bicubic strategy: tensor-product cubic spline (bicubic Hermite patch per cell).
//
// The node table holds one record per grid node, {z, zx, zy, zxy} with the lanes of each part contiguous:
// T[nx][ny][4][lanes].  A query reads two contiguous runs of 8 * lanes elements, at (i, j .. j+1) and (i+1, j .. j+1) --
// the access shape of Bilinear's two corner segments, four times as long.
//
//   transpose_nodes_kernel<T>   [n0][n1][L] -> [n1][n0][L]: the y-passes of the build solve along the second axis, the
//                               spline build along the first (lanes are independent: the bits do not change)
//   pack_nodes_kernel<T>        z, zx (grid order) and zy, zxy (transposed order) -> the node table
//   unpack_nodes_kernel<T>      the node table -> three plain [nx][ny][L] arrays (ndi_interp2d_tables)
//   eval_bicubic_kernel<T, VEC, KLDS, TB, NUX, NUY>
//                               QUERY ORDER with both searches fused in, as eval_fused2d_kernel: a wave takes 64
//                               consecutive queries, one per lane (search on each axis, the cell's record offset, t, u and
//                               the two knot spacings parked in a wave-private LDS strip), then walks the batch's output
//                               vectors in row-major order, 64 per trip: 16 operand loads, five Hermite forms, one
//                               streaming store.  Rows shorter than 64 vectors share a trip among several queries; longer
//                               rows are cut into chunks of `vchunk` vectors along blockIdx.y, so a batch of few queries
//                               on a very wide trailing axis still fills the chip.  KLDS: knot pyramids staged in LDS
//                               (else read from global memory: axes that do not fit).  NUX, NUY: the orders of the
//                               partial derivative the kernel evaluates (ndi_interp2d_partial): the four forms along y
//                               are H_NUY, the one along x is H_NUX (hermite_nu); (0, 0) is the surface itself and
//                               compiles to the code it was before the orders existed.  Nothing else differs.
//                               WRAP (a further parameter, false by default): the variant a handle launches that wraps
//                               on a periodic axis (ndi_interp2d_create_bicubic_periodic with extrapolate): the per-axis
//                               range test and the wrap of bicubic_wrap_query, once per query, before the search.  With
//                               WRAP == false none of it is compiled and the instances are the code they were.
//
// Numerical contract (include/ndinterp.h, ndi_interp2d_create_bicubic): every line one IEEE operation in T, in the stated
// order, nothing fused (-ffp-contract=off), so rows are bit-identical to the numpy restatement (tests/bicubic_ref.py).
#pragma once

#include <type_traits>

namespace ndi {

template <class T>
__global__ __launch_bounds__(BLOCK) void transpose_nodes_kernel(const T* in, T* out, uint64_t n0, uint64_t n1, uint64_t L) {
  const uint64_t total = n0 * n1 * L, row = n0 * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {   // e: element of `out`
    const uint64_t j = e / row, r = e - j * row;
    const uint64_t i = r / L, c = r - i * L;
    out[e] = in[NDI_CHK((i * n1 + j) * L + c, total, BC_INTERVAL)];
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void pack_nodes_kernel(const T* z, const T* zx, const T* zyT, const T* zxyT, T* table,
                                                           uint64_t nx, uint64_t ny, uint64_t L) {
  const uint64_t total = nx * ny * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {   // e: element of z
    const uint64_t node = e / L, c = e - node * L;
    const uint64_t i = node / ny, j = node - i * ny;
    const uint64_t et = NDI_CHK((j * nx + i) * L + c, total, BC_INTERVAL);
    T* rec = table + node * 4 * L + c;
    rec[0] = z[e];
    rec[L] = zx[e];
    rec[2 * L] = zyT[et];
    rec[3 * L] = zxyT[et];
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void unpack_nodes_kernel(const T* table, T* zx, T* zy, T* zxy, uint64_t nodes, uint64_t L) {
  const uint64_t total = nodes * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t node = NDI_CHK(e / L, nodes, BC_INTERVAL), c = e - node * L;
    const T* rec = table + node * 4 * L + c;
    if (zx) zx[e] = rec[L];
    if (zy) zy[e] = rec[2 * L];
    if (zxy) zxy[e] = rec[3 * L];
  }
}

template <class T>
struct BicubicArgs {
  Pyramid<T> px, py;
  const T* table;          // T[nx][ny][4][lanes]
  const T* qx;
  const T* qy;
  T* out;
  uint64_t nq, out_stride;
  uint64_t lv;             // vectors per part row (lanes / VEC)
  uint32_t lv_magic;       // ceil(2^32 / lv) for 2 <= lv < 64
  uint32_t vchunk;         // vectors of a row per blockIdx.y (a multiple of 64; >= lv when gridDim.y == 1)
  int mode;
  int wrap;                // WRAP variants: the axes that wrap (bit 0: x, bit 1: y); sits in the padding after `mode`
  unsigned long long* first_fail;   // [2]: x, y (range_check_kernel, or this kernel when `check`)
  int check;                        // fresh output: the kernel's own range test, no pre-pass
};

// A coordinate of a wrapping handle (a periodic axis of a handle built with extrapolate; the other axis of such a handle
// passes `wraps == false`).  Out of range on a wrapping axis: cubic_spline.rs:805-809, one IEEE operation in T per line --
//   d = q - k0;  p = kn - k0;  r = fmod(d, p);  if (r < 0) r = r + |p|;  qs = r + k0
// (rem_euclid_t), in range: the coordinate itself.  +-inf wraps to NaN.  Returns the coordinate the search and t are formed
// from; a NaN result is the only failure of such a handle (lane_query_fails' test of EX_PERIODIC / EX_YES).
template <class T>
__device__ __forceinline__ T bicubic_wrap_query(T q, T k0, T kn, bool wraps) {
  const bool inr = (k0 <= q) && (q <= kn);
  return (wraps && !inr) ? rem_euclid_t(q - k0, kn - k0) + k0 : q;
}

// The range pre-pass of a wrapping handle into a caller-owned buffer: range_check_kernel's geometry and first-error
// semantics, each axis by its own rule -- finite after the wrap on a wrapping axis, not NaN on the other.
template <class T>
__global__ __launch_bounds__(BLOCK) void bicubic_wrap_check_kernel(const T* qx, const T* qy, uint64_t nq, T x0, T xn, T y0, T yn,
                                                                   int wrap, unsigned long long* first_fail) {
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t qi = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; qi < nq; qi += step) {
    const T xs = bicubic_wrap_query<T>(qx[qi], x0, xn, (wrap & 1) != 0);
    const T ys = bicubic_wrap_query<T>(qy[qi], y0, yn, (wrap & 2) != 0);
    if (!(xs == xs)) atomicMin(&first_fail[0], (unsigned long long)qi);
    if (!(ys == ys)) atomicMin(&first_fail[1], (unsigned long long)qi);
  }
}

// The cubic Hermite form of cubic_spline.rs:824-828 on end values pl, pr and end derivatives kl, kr over a spacing h:
//   d = pr - pl;  a = kl h - d;  b = d - kr h;  (1-s) pl + s pr + s (1-s) (a (1-s) + b s)
template <class T, class V>
__device__ __forceinline__ V hermite_form(V pl, V pr, V kl, V kr, T h, T s, T c0, T c2) {
  const V d = pr - pl;
  const V a = kl * h - d;
  const V b = d - kr * h;
  return c0 * pl + s * pr + c2 * (a * c0 + b * s);
}

// H_NU of the header (ndi_interp2d_partial): the NU-th derivative of that form with respect to the coordinate s lives on.
//   c1 = d + a;  c2 = b - (a + a);  c3 = b - a
//   H1 = (c1 + s ((c2 + c2) - (3 c3) s)) / h          H2 = ((c2 + c2) - (6 c3) s) / (h h)
template <int NU, class T, class V>
__device__ __forceinline__ V hermite_nu(V pl, V pr, V kl, V kr, T h, T s, T c0, T c2) {
  static_assert(NU >= 0 && NU <= 2, "orders 0, 1 and 2");
  if constexpr (NU == 0) {
    return hermite_form<T, V>(pl, pr, kl, kr, h, s, c0, c2);
  } else {
    const V d = pr - pl;
    const V a = kl * h - d;
    const V b = d - kr * h;
    const V q2 = b - (a + a);
    const V q3 = b - a;
    if constexpr (NU == 1) {
      const V q1 = d + a;
      return (q1 + s * ((q2 + q2) - (T(3) * q3) * s)) / h;
    } else {
      return ((q2 + q2) - (T(6) * q3) * s) / (h * h);
    }
  }
}

template <class T, int VEC, bool KLDS, int TB, int NUX = 0, int NUY = 0, bool WRAP = false>
__global__ __launch_bounds__(TB) void eval_bicubic_kernel(BicubicArgs<T> A) {
  using V = typename VecT<T, VEC>::type;
  using PTR = typename std::conditional<KLDS, lds_ptr<T>, const T*>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr uint32_t WAVES = TB / 64;
  if (A.nq == 0) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nxa = A.px.n + A.px.n1, nya = A.py.n + A.py.n1;
  // LDS: [x pyramid | y pyramid | per-wave strips: record offset (u64), t, u, hx, hy]
  size_t off = 0;
  if (KLDS) {
    T* sx = reinterpret_cast<T*>(smem_raw);
    T* sy = sx + nxa;
    for (uint32_t i = tid; i < nxa; i += TB) sx[i] = A.px.lv0[i];
    for (uint32_t i = tid; i < nya; i += TB) sy[i] = A.py.lv0[i];
    off = ((size_t)(nxa + nya) * sizeof(T) + 15u) & ~(size_t)15u;
  }
  unsigned long long* w_o = reinterpret_cast<unsigned long long*>(smem_raw + off) + wave * 64u;
  off += (size_t)WAVES * 64u * sizeof(unsigned long long);
  T* w_s = reinterpret_cast<T*>(smem_raw + off) + wave * 64u * 4u;   // [4][64] per wave: t, u, hx, hy
  if (KLDS) __syncthreads();
  PyramidT<T, PTR> PX, PY;
  if constexpr (KLDS) {
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
  unsigned long long limit = A.check ? NO_FAIL : (A.first_fail[0] < A.first_fail[1] ? A.first_fail[0] : A.first_fail[1]);
  if (limit > A.nq) limit = A.nq;
  const V* const G = reinterpret_cast<const V*>(A.table);
  const uint64_t LV = A.lv;
  const uint64_t RS = (uint64_t)A.py.n * 4u * LV;            // vectors between grid rows i and i + 1
  const uint64_t v_lo = (uint64_t)blockIdx.y * A.vchunk;     // this workgroup's piece of every row
  const uint32_t W = (uint32_t)((LV - v_lo < (uint64_t)A.vchunk) ? LV - v_lo : (uint64_t)A.vchunk);
  const T one = T(1);
  const uint64_t wave_step = (uint64_t)gridDim.x * TB;
  for (uint64_t base = ((uint64_t)blockIdx.x * WAVES + wave) * 64u; base < limit; base += wave_step) {
    {
      const uint64_t p = base + lane;
      const bool in = p < limit;
      T x = in ? A.qx[p] : x0, y = in ? A.qy[p] : y0;
      if constexpr (WRAP) {                   // once per query, before the search; the test is on the wrapped coordinate
        x = bicubic_wrap_query<T>(x, x0, xn, (A.wrap & 1) != 0);
        y = bicubic_wrap_query<T>(y, y0, yn, (A.wrap & 2) != 0);
        if (A.check && in && blockIdx.y == 0) lane_check2<T>(A.first_fail, p, x, y, x0, xn, y0, yn, (int)EX_YES);
      } else {
        if (A.check && in && blockIdx.y == 0) lane_check2<T>(A.first_fail, p, x, y, x0, xn, y0, yn, A.mode);   // fresh output
      }
      const uint32_t xi = locate_index<T, PTR>(PX, x0, xn, x, lane);   // all 64 lanes take part
      const uint32_t yi = locate_index<T, PTR>(PY, y0, yn, y, lane);
      const T x1 = PX.lv0[xi], hx = PX.lv0[xi + 1] - x1, y1 = PY.lv0[yi], hy = PY.lv0[yi + 1] - y1;
      w_o[lane] = ((uint64_t)NDI_CHK(xi, PX.n - 1u, BC_CELL_X) * PY.n + NDI_CHK(yi, PY.n - 1u, BC_CELL_Y)) * 4u * LV;
      w_s[0 * 64 + lane] = (x - x1) / hx;       // cubic_spline.rs:820's t, on each axis
      w_s[1 * 64 + lane] = (y - y1) / hy;
      w_s[2 * 64 + lane] = hx;
      w_s[3 * 64 + lane] = hy;
    }
    __builtin_amdgcn_wave_barrier();        // LDS operations of one wave execute in order: no s_barrier needed
    const uint32_t nq_here = (limit - base < 64u) ? (uint32_t)(limit - base) : 64u;
    auto item = [&](uint32_t ql, uint64_t v) {
      ql = NDI_CHK(ql, 64u, BC_STRIP);
      const T t = w_s[0 * 64 + ql], u = w_s[1 * 64 + ql], hx = w_s[2 * 64 + ql], hy = w_s[3 * 64 + ql];
      const V* g0 = G + (w_o[ql] + v);        // node (i, j): z, zx, zy, zxy; node (i, j + 1) follows
      const V* g1 = g0 + RS;                  // nodes (i + 1, j), (i + 1, j + 1)
      const V z00 = g0[0], zx00 = g0[LV], zy00 = g0[2 * LV], zxy00 = g0[3 * LV];
      const V z01 = g0[4 * LV], zx01 = g0[5 * LV], zy01 = g0[6 * LV], zxy01 = g0[7 * LV];
      const V z10 = g1[0], zx10 = g1[LV], zy10 = g1[2 * LV], zxy10 = g1[3 * LV];
      const V z11 = g1[4 * LV], zx11 = g1[5 * LV], zy11 = g1[6 * LV], zxy11 = g1[7 * LV];
      const T cu = one - u, cu2 = u * cu, ct = one - t, ct2 = t * ct;
      const V p0 = hermite_nu<NUY, T, V>(z00, z01, zy00, zy01, hy, u, cu, cu2);
      const V p1 = hermite_nu<NUY, T, V>(z10, z11, zy10, zy11, hy, u, cu, cu2);
      const V d0 = hermite_nu<NUY, T, V>(zx00, zx01, zxy00, zxy01, hy, u, cu, cu2);
      const V d1 = hermite_nu<NUY, T, V>(zx10, zx11, zxy10, zxy11, hy, u, cu, cu2);
      const V r = hermite_nu<NUX, T, V>(p0, p1, d0, d1, hx, t, ct, ct2);
      store_stream<true>(reinterpret_cast<V*>(A.out + (base + ql) * A.out_stride) + v, r);
    };
    if (LV < 64u) {                         // several queries per trip (one chunk: W == LV)
      const uint32_t lv = (uint32_t)LV, items = nq_here * lv;
      for (uint32_t it = lane; it < items; it += 64u) {
        const uint32_t ql = (lv == 1u) ? it : __umulhi(it, A.lv_magic);
        item(ql, it - ql * lv);
      }
    } else {
      for (uint32_t ql = 0; ql < nq_here; ++ql)
        for (uint32_t v = lane; v < W; v += 64u) item(ql, v_lo + v);
    }
    __builtin_amdgcn_wave_barrier();        // the strip is rewritten by the next batch
  }
}

}  // namespace ndi
