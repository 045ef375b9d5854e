// csrc/tricubic_kernels.hpp -- the Tricubic strategy of the 3-D handles (ndi_interp3d_create_tricubic,
// include/ndinterp3d_cubic.h): the tensor-product cubic spline on a rectilinear grid, a tricubic Hermite patch per cell.
//
// The node table holds one record per grid node: eight parts, the lanes of each part contiguous,
//     T[nx][ny][nz][8][lanes],   part p = 4 [d/dx] + 2 [d/dy] + [d/dz]:   f, fz, fy, fyz, fx, fxz, fxy, fxyz.
// The z-pair k, k+1 of one (i', j') corner is one contiguous run of 16 * lanes elements, so a query reads four such runs.
// Every offset into the table is 64-bit.
//
//   pack_nodes3_kernel<T>     one plain table of the grid's shape, in the layout its pass left it in, -> one part of the
//                             node table.  Layouts: TL_GRID [nx][ny][nz][L]; TL_Y [ny][nx][nz][L] (what a y-pass works on:
//                             transpose_nodes_kernel of the view (nx, ny, nz L)); TL_Z [nz][nx][ny][L] (a z-pass:
//                             transpose_nodes_kernel of the view (nx ny, nz, L)).
//   unpack_nodes3_kernel<T>   one part of the node table -> a plain [nx][ny][nz][L] array (ndi_interp3d_tables, and the
//                             build's own re-reads of fx, fy, fxy)
//   eval_tricubic_kernel<T, VEC, STAGE, CHECK>
//                             eval_trilinear_kernel's mapping and selection rules (trilinear_kernels.hpp), unchanged: one item
//                             is one output vector of VEC elements, the vector index runs fastest, a grid-stride loop over a
//                             resident grid with the (row, vector) carry, per-thread bisection through
//                             trilinear_lower_index (in LDS with STAGE), CHECK reports by atomicMin from vector 0 and a
//                             failing item stores nothing.  An item works a corner at a time: sixteen operand loads of one
//                             (i', j'), four H along z, and once both corners of an i' are done two H along y; one H along x
//                             ends it -- 21 H, and the 64 operands are never live together.
//
// Numerical contract (include/ndinterp3d_cubic.h): every line one IEEE operation in T, in the stated order, nothing fused
// (-ffp-contract=off); t, u, w are three IEEE divisions per item.  Rows are bit-identical to tests/tricubic_ref.py.
#pragma once

namespace ndi {

enum TableLayout : int { TL_GRID = 0, TL_Y = 1, TL_Z = 2 };

// the element of a plain table in `layout` that belongs to grid element (i, j, k, c)
__device__ __forceinline__ uint64_t tricubic_plain_index(int layout, uint64_t i, uint64_t j, uint64_t k, uint64_t c, uint64_t nx,
                                                         uint64_t ny, uint64_t nz, uint64_t L) {
  return layout == TL_GRID ? ((i * ny + j) * nz + k) * L + c
         : layout == TL_Y  ? ((j * nx + i) * nz + k) * L + c
                           : ((k * nx + i) * ny + j) * L + c;
}

template <class T>
__global__ __launch_bounds__(BLOCK) void pack_nodes3_kernel(const T* src, int layout, int part, T* table, uint64_t nx, uint64_t ny,
                                                            uint64_t nz, uint64_t L) {
  const uint64_t total = nx * ny * nz * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {   // e: element of the grid
    const uint64_t node = e / L, c = e - node * L;
    const uint64_t ij = node / nz, k = node - ij * nz;
    const uint64_t i = ij / ny, j = ij - i * ny;
    const uint64_t es = NDI_CHK(tricubic_plain_index(layout, i, j, k, c, nx, ny, nz, L), total, BC_INTERVAL);
    table[(node * 8u + (uint64_t)part) * L + c] = src[es];
  }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void unpack_nodes3_kernel(const T* table, int part, T* dst, uint64_t nodes, uint64_t L) {
  const uint64_t total = nodes * L;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t node = NDI_CHK(e / L, nodes, BC_INTERVAL), c = e - node * L;
    dst[e] = table[(node * 8u + (uint64_t)part) * L + c];
  }
}

template <class T>
struct TricubicArgs {
  const T* x;            // [nx]
  const T* y;            // [ny]
  const T* z;            // [nz]
  const T* table;        // [nx][ny][nz][8][lanes]
  const T* qx;           // [nq]
  const T* qy;
  const T* qz;
  T* out;                // [nq][out_stride]
  uint64_t nq, lanes, out_stride;
  uint64_t vpr;          // vectors per row: lanes / VEC
  uint64_t step_rows;    // the grid's stride gridDim.x * BLOCK as (rows, vectors): step = step_rows * vpr + step_vecs
  uint64_t step_vecs;
  uint32_t nx, ny, nz;
  int mode;              // ExtrapMode
  unsigned long long* first_fail;   // [3]: x, y, z
};

// One (i', j') corner: the run at g holds the eight parts at k, then the eight parts at k + 1, `L` elements each.  Four H
// along z, each a part P in {f, fy, fx, fxy} with its z-derivative P + 1:  r[0] = f, r[1] = fy, r[2] = fx, r[3] = fxy.
template <class T, class V>
__device__ __forceinline__ void tricubic_corner(const T* g, uint64_t L, T hz, T w, T cw, T cw2, V r[4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const T* p = g + (uint64_t)(2 * m) * L;
    const V pl = *reinterpret_cast<const V*>(p), kl = *reinterpret_cast<const V*>(p + L);
    const V pr = *reinterpret_cast<const V*>(p + 8u * L), kr = *reinterpret_cast<const V*>(p + 9u * L);
    r[m] = hermite_form<T, V>(pl, pr, kl, kr, hz, w, cw, cw2);
  }
}

template <class T, int VEC, bool STAGE, bool CHECK>
__global__ __launch_bounds__(BLOCK) void eval_tricubic_kernel(TricubicArgs<T> A) {
  using V = typename VecT<T, VEC>::type;
  using PTR = typename std::conditional<STAGE, lds_ptr<T>, const T*>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const uint32_t tid = threadIdx.x;
  const uint32_t nx = A.nx, ny = A.ny, nz = A.nz;
  PTR kx, ky, kz;
  if constexpr (STAGE) {   // LDS: [x | y | z]
    T* s = reinterpret_cast<T*>(smem_raw);
    for (uint32_t i = tid; i < nx; i += BLOCK) s[i] = A.x[i];
    for (uint32_t i = tid; i < ny; i += BLOCK) s[nx + i] = A.y[i];
    for (uint32_t i = tid; i < nz; i += BLOCK) s[nx + ny + i] = A.z[i];
    __syncthreads();
    kx = (lds_ptr<T>)(smem_raw);
    ky = kx + nx;
    kz = ky + ny;
  } else {
    kx = A.x;
    ky = A.y;
    kz = A.z;
  }
  const T x0 = kx[0], xn = kx[nx - 1u], y0 = ky[0], yn = ky[ny - 1u], z0 = kz[0], zn = kz[nz - 1u];
  uint64_t rows = A.nq;
  if constexpr (!CHECK) {   // the pre-pass has left the lowest failing query per axis: rows at / after it stay untouched
    unsigned long long f = A.first_fail[0] < A.first_fail[1] ? A.first_fail[0] : A.first_fail[1];
    f = f < A.first_fail[2] ? f : A.first_fail[2];
    if (f < rows) rows = f;
  }
  const uint64_t vpr = A.vpr;
  const uint64_t total = rows * vpr;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  uint64_t item = (uint64_t)blockIdx.x * BLOCK + tid;
  if (item >= total) return;   // (no barrier follows)
  uint64_t row = item / vpr, vec = item - row * vpr;
  const uint64_t L = A.lanes;
  const uint64_t sz = 8u * L, sy = (uint64_t)nz * sz, sx = (uint64_t)ny * sy;   // element strides of the node table
  const T one = T(1);
  for (; item < total; item += step) {
    const uint64_t r = NDI_CHK(row, A.nq, BC_QUERY), v = NDI_CHK(vec, vpr, BC_ITEM);
    row += A.step_rows;   // the next trip's (row, vector): a carry instead of a division
    vec += A.step_vecs;
    if (vec >= vpr) {
      vec -= vpr;
      ++row;
    }
    const T x = A.qx[r], y = A.qy[r], z = A.qz[r];
    const bool badx = trilinear_bad<T>(x, x0, xn, A.mode), bady = trilinear_bad<T>(y, y0, yn, A.mode),
               badz = trilinear_bad<T>(z, z0, zn, A.mode);
    if (badx || bady || badz) {
      if constexpr (CHECK) {
        if (v == 0) {   // one report per row
          if (badx) atomicMin(&A.first_fail[0], (unsigned long long)r);
          if (bady) atomicMin(&A.first_fail[1], (unsigned long long)r);
          if (badz) atomicMin(&A.first_fail[2], (unsigned long long)r);
        }
      }
      continue;
    }
    const uint32_t xi = NDI_CHK((trilinear_lower_index<T, PTR>(kx, nx, x)), nx - 1u, BC_CELL_X);
    const uint32_t yi = NDI_CHK((trilinear_lower_index<T, PTR>(ky, ny, y)), ny - 1u, BC_CELL_Y);
    const uint32_t zi = NDI_CHK((trilinear_lower_index<T, PTR>(kz, nz, z)), nz - 1u, BC_CELL_Z);
    const T x1 = kx[xi], hx = kx[xi + 1u] - x1, y1 = ky[yi], hy = ky[yi + 1u] - y1, z1 = kz[zi], hz = kz[zi + 1u] - z1;
    const T t = (x - x1) / hx, u = (y - y1) / hy, w = (z - z1) / hz;
    const T ct = one - t, ct2 = t * ct, cu = one - u, cu2 = u * cu, cw = one - w, cw2 = w * cw;
    const T* g = A.table + ((uint64_t)xi * sx + (uint64_t)yi * sy + (uint64_t)zi * sz + v * (uint64_t)VEC);
    V val[2], der[2];
#pragma unroll
    for (int di = 0; di < 2; ++di) {
      V lo[4], hi[4];   // the z-results of the corners (i', j) and (i', j + 1)
      tricubic_corner<T, V>(g + (uint64_t)di * sx, L, hz, w, cw, cw2, lo);
      tricubic_corner<T, V>(g + (uint64_t)di * sx + sy, L, hz, w, cw, cw2, hi);
      val[di] = hermite_form<T, V>(lo[0], hi[0], lo[1], hi[1], hy, u, cu, cu2);   // (f, fy)
      der[di] = hermite_form<T, V>(lo[2], hi[2], lo[3], hi[3], hy, u, cu, cu2);   // (fx, fxy)
    }
    const V res = hermite_form<T, V>(val[0], val[1], der[0], der[1], hx, t, ct, ct2);
    __builtin_nontemporal_store(res, reinterpret_cast<V*>(A.out + r * A.out_stride + v * (uint64_t)VEC));
  }
}

}  // namespace ndi
