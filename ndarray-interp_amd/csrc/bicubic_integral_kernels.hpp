// csrc/bicubic_integral_kernels.hpp -- 2-D antiderivative handles of the Bicubic strategy (ndi_interp2d_antiderivative,
// ndi_interp2d_integral): F(qx, qy) = the integral of the surface over [x[0], qx] x [y[0], qy], and rectangle integrals.
//
// The antiderivative of a tensor-product Hermite cubic is the tensor product of the 1-D rule (antiderivative_kernels.hpp)
// with itself.  Beside the source's node table {z, zx, zy, zxy} the handle keeps one record per node,
// {PP, Qz, Qzy, Pz, Pzx} with the lanes of each part contiguous: T[nx][ny][5][lanes].
//   Qz, Qzy   prefix along x of the Hermite data (z, zx), (zy, zxy)
//   Pz, Pzx   prefix along y of the Hermite data (z, zy), (zx, zxy)
//   PP        prefix along x of (Pz, Pzx)
// Every prefix is the 1-D build's fixed blocked sum (AD_B = 256), run by the 1-D build's own kernels on (nx, ny lanes) views
// (x passes) and on transposed copies (y passes); the kernels here only move data and form the Hermite a / b rows.
//
//   integral_unpack_kernel<T>     the node table -> z, zx, zy, zxy as plain [nx][ny][L] arrays
//   hermite_ab_kernel<T>          (p, k) [n][L] on knots x -> a, b [n-1][L]: H's three lines (d, a, b)
//   integral_pack_kernel<T>       PP, Qz, Qzy (grid order), PzT, PzxT (transposed order) -> the record table
//   integral_unpack_tables_kernel<T>   the record table -> five plain arrays (ndi_interp2d_integral_tables)
//   eval_bicubic_integral_kernel<T, VEC, KLDS, TB, RECT>
//                                 eval_bicubic_kernel's mapping (a wave takes 64 queries, parks their cells in a wave-private
//                                 strip, then walks the output vectors 64 per trip); 25 operand loads per F.  RECT: four
//                                 query arrays; the strip holds two x cells {i, t, hx} and two y cells {j, u, hy} per query,
//                                 the four F come from one device function and meet in three subtractions.
//
// Numerical contract (include/ndinterp.h, ndi_interp2d_antiderivative): every line one IEEE operation in T, in the stated
// order, nothing fused (-ffp-contract=off), so tables and rows are bit-identical to tests/bicubic_integral_ref.py.
#pragma once

#include <type_traits>

namespace ndi {

template <class T>
__global__ __launch_bounds__(BLOCK) void integral_unpack_kernel(const T* table, T* z, T* zx, T* zy, T* zxy, uint64_t nodes,
                                                                uint64_t L) {
  const uint64_t total = nodes * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t node = NDI_CHK(e / L, nodes, BC_INTERVAL), c = e - node * L;
    const T* rec = table + node * 4 * L + c;
    z[e] = rec[0];
    zx[e] = rec[L];
    zy[e] = rec[2 * L];
    zxy[e] = rec[3 * L];
  }
}

// d = p[i+1] - p[i];  a[i] = k[i] h - d;  b[i] = d - k[i+1] h   (h = x[i+1] - x[i])
template <class T>
__global__ __launch_bounds__(BLOCK) void hermite_ab_kernel(const T* p, const T* k, const T* x, T* a, T* b, uint64_t n,
                                                           uint64_t L) {
  const uint64_t total = (n - 1) * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t i = NDI_CHK(e / L, n - 1, BC_INTERVAL);
    const T h = x[i + 1] - x[i];
    const T d = p[e + L] - p[e];
    a[e] = k[e] * h - d;
    b[e] = d - k[e + L] * h;
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void integral_pack_kernel(const T* pp, const T* qz, const T* qzy, const T* pzT,
                                                              const T* pzxT, T* table, uint64_t nx, uint64_t ny, uint64_t L) {
  const uint64_t total = nx * ny * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {   // e: element of a grid-order array
    const uint64_t node = e / L, c = e - node * L;
    const uint64_t i = node / ny, j = node - i * ny;
    const uint64_t et = NDI_CHK((j * nx + i) * L + c, total, BC_INTERVAL);
    T* rec = table + node * 5 * L + c;
    rec[0] = pp[e];
    rec[L] = qz[e];
    rec[2 * L] = qzy[e];
    rec[3 * L] = pzT[et];
    rec[4 * L] = pzxT[et];
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void integral_unpack_tables_kernel(const T* table, T* pp, T* qz, T* qzy, T* pz, T* pzx,
                                                                       uint64_t nodes, uint64_t L) {
  const uint64_t total = nodes * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t node = NDI_CHK(e / L, nodes, BC_INTERVAL), c = e - node * L;
    const T* rec = table + node * 5 * L + c;
    if (pp) pp[e] = rec[0];
    if (qz) qz[e] = rec[L];
    if (qzy) qzy[e] = rec[2 * L];
    if (pz) pz[e] = rec[3 * L];
    if (pzx) pzx[e] = rec[4 * L];
  }
}

template <class T>
struct BicubicIntegralArgs {
  Pyramid<T> px, py;
  const T* table;          // the source's nodes: T[nx][ny][4][lanes]
  const T* itable;         // the prefix records: T[nx][ny][5][lanes]
  const T* qx;             // F: the queries; RECT: xb, yb (the upper bounds)
  const T* qy;
  const T* qx_lo;          // RECT: xa, ya
  const T* qy_lo;
  T* out;
  uint64_t nq, out_stride;
  uint64_t lv;             // vectors per part row (lanes / VEC)
  uint32_t lv_magic;       // ceil(2^32 / lv) for 2 <= lv < 64
  uint32_t vchunk;         // vectors of a row per blockIdx.y (a multiple of 64; >= lv when gridDim.y == 1)
  int mode;
  unsigned long long* first_fail;   // [2]: the x bounds, the y bounds (range_check_kernel, or this kernel when `check`)
  int check;                        // fresh output: the kernel's own range test, no pre-pass
};

// h G(s) of the header: the antiderivative of the Hermite form on end values pl, pr and end derivatives kl, kr from the
// interval's left end to s (in units of the spacing h).
template <class T, class V>
__device__ __forceinline__ V hermite_antideriv(V pl, V pr, V kl, V kr, T h, T s) {
  const V d = pr - pl;
  const V a = kl * h - d;
  const V b = d - kr * h;
  const V c1 = (d + a) * T(0.5);
  const V c2 = (b - (a + a)) / T(3);
  const V c3 = (b - a) * T(0.25);
  return h * (s * (pl + s * (c1 + s * (c2 - s * c3))));
}

// F at (cell i, j; t, u) for output vector v.  n0 / r0: vector offsets of node (i, j) in the node / the record table;
// RS4 / RS5: vectors between grid rows.  The four y-direction forms of the node records reduce 20 operands to 4 before
// the Q operands are read.
template <class T, class V>
__device__ __forceinline__ V integral_point(const V* __restrict__ N, const V* __restrict__ R, uint64_t n0, uint64_t r0,
                                            uint64_t RS4, uint64_t RS5, uint64_t LV, T t, T u, T hx, T hy) {
  const V* g0 = N + n0;               // node (i, j): z, zx, zy, zxy; node (i, j + 1) follows
  const V* g1 = g0 + RS4;             // nodes (i + 1, j), (i + 1, j + 1)
  const V* r0p = R + r0;              // record (i, j): PP, Qz, Qzy, Pz, Pzx; record (i, j + 1) follows
  const V* r1p = r0p + RS5;           // record (i + 1, j)
  V w0, w1, v0, v1;
  {
    const V z00 = g0[0], zy00 = g0[2 * LV], z01 = g0[4 * LV], zy01 = g0[6 * LV];
    w0 = r0p[3 * LV] + hermite_antideriv<T, V>(z00, z01, zy00, zy01, hy, u);
  }
  {
    const V z10 = g1[0], zy10 = g1[2 * LV], z11 = g1[4 * LV], zy11 = g1[6 * LV];
    w1 = r1p[3 * LV] + hermite_antideriv<T, V>(z10, z11, zy10, zy11, hy, u);
  }
  {
    const V zx00 = g0[LV], zxy00 = g0[3 * LV], zx01 = g0[5 * LV], zxy01 = g0[7 * LV];
    v0 = r0p[4 * LV] + hermite_antideriv<T, V>(zx00, zx01, zxy00, zxy01, hy, u);
  }
  {
    const V zx10 = g1[LV], zxy10 = g1[3 * LV], zx11 = g1[5 * LV], zxy11 = g1[7 * LV];
    v1 = r1p[4 * LV] + hermite_antideriv<T, V>(zx10, zx11, zxy10, zxy11, hy, u);
  }
  const V inner = hermite_antideriv<T, V>(w0, w1, v0, v1, hx, t);
  const V pp = r0p[0], qz0 = r0p[LV], qzy0 = r0p[2 * LV], qz1 = r0p[6 * LV], qzy1 = r0p[7 * LV];
  const V e = pp + hermite_antideriv<T, V>(qz0, qz1, qzy0, qzy1, hy, u);
  return e + inner;
}

template <class T, int VEC, bool KLDS, int TB, bool RECT>
__global__ __launch_bounds__(TB) void eval_bicubic_integral_kernel(BicubicIntegralArgs<T> A) {
  using V = typename VecT<T, VEC>::type;
  using PTR = typename std::conditional<KLDS, lds_ptr<T>, const T*>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr uint32_t WAVES = TB / 64;
  constexpr uint32_t NB = RECT ? 2u : 1u;   // cells per axis and query: (upper, lower)
  if (A.nq == 0) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t nxa = A.px.n + A.px.n1, nya = A.py.n + A.py.n1;
  // LDS: [x pyramid | y pyramid | per-wave strips: i, j (u32) and t, hx, u, hy, NB of each]
  size_t off = 0;
  if (KLDS) {
    T* sx = reinterpret_cast<T*>(smem_raw);
    T* sy = sx + nxa;
    for (uint32_t i = tid; i < nxa; i += TB) sx[i] = A.px.lv0[i];
    for (uint32_t i = tid; i < nya; i += TB) sy[i] = A.py.lv0[i];
    off = ((size_t)(nxa + nya) * sizeof(T) + 15u) & ~(size_t)15u;
  }
  T* w_s = reinterpret_cast<T*>(smem_raw + off) + wave * 64u * 4u * NB;   // [4 NB][64] per wave: t, hx, u, hy
  off += (size_t)WAVES * 64u * 4u * NB * sizeof(T);
  uint32_t* w_c = reinterpret_cast<uint32_t*>(smem_raw + off) + wave * 64u * 2u * NB;   // [2 NB][64] per wave: i, j
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
  const V* const N = reinterpret_cast<const V*>(A.table);
  const V* const R = reinterpret_cast<const V*>(A.itable);
  const uint64_t LV = A.lv;
  const uint64_t RS4 = (uint64_t)A.py.n * 4u * LV, RS5 = (uint64_t)A.py.n * 5u * LV;
  const uint64_t v_lo = (uint64_t)blockIdx.y * A.vchunk;     // this workgroup's piece of every row
  const uint32_t W = (uint32_t)((LV - v_lo < (uint64_t)A.vchunk) ? LV - v_lo : (uint64_t)A.vchunk);
  const uint64_t wave_step = (uint64_t)gridDim.x * TB;
  for (uint64_t base = ((uint64_t)blockIdx.x * WAVES + wave) * 64u; base < limit; base += wave_step) {
    {
      const uint64_t p = base + lane;
      const bool in = p < limit;
#pragma unroll
      for (uint32_t k = 0; k < NB; ++k) {
        const T* ax = k ? A.qx_lo : A.qx;
        const T* ay = k ? A.qy_lo : A.qy;
        const T x = in ? ax[p] : x0, y = in ? ay[p] : y0;
        if (A.check && in && blockIdx.y == 0) lane_check2<T>(A.first_fail, p, x, y, x0, xn, y0, yn, A.mode);   // fresh output
        const uint32_t xi = locate_index<T, PTR>(PX, x0, xn, x, lane);   // all 64 lanes take part
        const uint32_t yi = locate_index<T, PTR>(PY, y0, yn, y, lane);
        const T x1 = PX.lv0[xi], hx = PX.lv0[xi + 1] - x1, y1 = PY.lv0[yi], hy = PY.lv0[yi + 1] - y1;
        w_c[(2 * k + 0) * 64 + lane] = NDI_CHK(xi, PX.n - 1u, BC_CELL_X);
        w_c[(2 * k + 1) * 64 + lane] = NDI_CHK(yi, PY.n - 1u, BC_CELL_Y);
        w_s[(4 * k + 0) * 64 + lane] = (x - x1) / hx;       // Bicubic's t and u
        w_s[(4 * k + 1) * 64 + lane] = hx;
        w_s[(4 * k + 2) * 64 + lane] = (y - y1) / hy;
        w_s[(4 * k + 3) * 64 + lane] = hy;
      }
    }
    __builtin_amdgcn_wave_barrier();        // LDS operations of one wave execute in order: no s_barrier needed
    const uint32_t nq_here = (limit - base < 64u) ? (uint32_t)(limit - base) : 64u;
    // F at the query's x cell kx and y cell ky (0: the upper bound / the query, 1: the lower bound)
    auto F = [&](uint32_t ql, uint32_t kx, uint32_t ky, uint64_t v) -> V {
      const uint64_t i = w_c[(2 * kx) * 64 + ql], j = w_c[(2 * ky + 1) * 64 + ql];
      const T t = w_s[(4 * kx) * 64 + ql], hx = w_s[(4 * kx + 1) * 64 + ql];
      const T u = w_s[(4 * ky + 2) * 64 + ql], hy = w_s[(4 * ky + 3) * 64 + ql];
      const uint64_t node = i * PY.n + j;
      return integral_point<T, V>(N, R, node * 4u * LV + v, node * 5u * LV + v, RS4, RS5, LV, t, u, hx, hy);
    };
    auto item = [&](uint32_t ql, uint64_t v) {
      ql = NDI_CHK(ql, 64u, BC_STRIP);
      V r;
      if constexpr (RECT) {
        const V fbb = F(ql, 0, 0, v);
        const V fab = F(ql, 1, 0, v);
        const V top = fbb - fab;
        const V fba = F(ql, 0, 1, v);
        const V faa = F(ql, 1, 1, v);
        r = top - (fba - faa);
      } else {
        r = F(ql, 0, 0, v);
      }
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
