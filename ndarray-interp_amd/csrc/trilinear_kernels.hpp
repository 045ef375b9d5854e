// csrc/trilinear_kernels.hpp -- Trilinear evaluation of the 3-D handles (ndi_interp3d_eval):
//     out[j][l] = f_l(qx[j], qy[j], qz[j]),   the grid T[nx][ny][nz][lanes], lanes fastest.
//
// Value rule (include/ndinterp3d.h): the intervals i, j, k are the largest index with knot <= q, clamped to [0, n - 2];
// the point is seven Linear::calc_frac (linear.rs:29-36) in the reference's Bilinear order (bilinear.rs:94-96) continued by
// one axis -- four along x, two along y, one along z -- every step one IEEE operation in T.  The seven divisions go through
// frac_shared (kernels.hpp): one correctly rounded reciprocal per axis and item, the IEEE quotient's bits, the IEEE division
// itself outside its exponent window.  Nothing else differs from the written order.
//
// Mapping: one work item is one output vector of VEC elements (16 bytes: 4 x f32 / 2 x f64, or one element), the flat item
// index runs with the vector index fastest (row = item / (lanes / VEC)), so a wavefront's stores coalesce and the three
// coordinates of a row are broadcast loads; a grid-stride loop over a resident grid, the (row, vector) pair carried from
// trip to trip without a division.  A cell's eight corners are eight VEC-wide loads: d[.][.][k] and d[.][.][k+1] lie `lanes`
// elements apart, so for short rows a cell's z-pair is one contiguous piece.
//
//   eval_trilinear_kernel<T, VEC, STAGE, CHECK>
//                             STAGE: the three axes are copied into LDS once per workgroup and bisected there (else they are
//                             bisected in global memory).  CHECK: the kernel tests the queries itself and publishes the lowest
//                             failing query per axis (a failing item stores nothing); without it the pre-pass has run and only
//                             rows below the first failure are evaluated.
//   range_check3_kernel       the pre-pass: range_check_kernel's test on three arrays (first_fail[0]: x, [1]: y, [2]: z)
#pragma once

namespace ndi {

constexpr int BC_CELL_Z = 10;   // (BoundsCode) 3-D cell index along z, limit nz - 1
constexpr int BC_ITEM = 11;     // (BoundsCode) vector of a row, limit lanes / VEC

// The status words of one 3-D batch: the lowest failing query per axis.  It lives in a scratch set's status buffer.
struct TrilinearStatus {
  unsigned long long first_fail[3];   // x, y, z
};
static_assert(sizeof(TrilinearStatus) <= sizeof(StatusBlock), "the 3-D status lives in a StatusBlock's buffer");

// The failure test of one coordinate: outside [k0, kn] (a NaN fails it too) without extrapolation, NaN with it.
template <class T>
__device__ __forceinline__ bool trilinear_bad(T q, T k0, T kn, int mode) {
  return (mode == EX_NO) ? !((k0 <= q) && (q <= kn)) : !(q == q);
}

template <class T>
__global__ __launch_bounds__(BLOCK) void range_check3_kernel(const T* qx, const T* qy, const T* qz, uint64_t nq, T x0, T xn,
                                                             T y0, T yn, T z0, T zn, int mode,
                                                             unsigned long long* first_fail) {
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t qi = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; qi < nq; qi += step) {
    const T x = qx[qi], y = qy[qi], z = qz[qi];
    if (trilinear_bad<T>(x, x0, xn, mode)) atomicMin(&first_fail[0], (unsigned long long)qi);
    if (trilinear_bad<T>(y, y0, yn, mode)) atomicMin(&first_fail[1], (unsigned long long)qi);
    if (trilinear_bad<T>(z, z0, zn, mode)) atomicMin(&first_fail[2], (unsigned long long)qi);
  }
}

// The largest index i with k[i] <= q, clamped to [0, n - 2] (n >= 2): a plain bisection whose probes stay in [1, n - 2].
// A NaN compares false everywhere and gives 0 (such an item is never evaluated).
template <class T, class PTR>
__device__ __forceinline__ uint32_t trilinear_lower_index(PTR k, uint32_t n, T q) {
  uint32_t lo = 0, hi = n - 1u;   // invariant: the answer is in [lo, hi - 1]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k[mid] <= q) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <class T>
struct TrilinearArgs {
  const T* x;            // [nx]
  const T* y;            // [ny]
  const T* z;            // [nz]
  const T* data;         // [nx][ny][nz][lanes]
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

template <class T, int VEC, bool STAGE, bool CHECK>
__global__ __launch_bounds__(BLOCK) void eval_trilinear_kernel(TrilinearArgs<T> A) {
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
  const uint64_t sz = A.lanes, sy = (uint64_t)nz * sz, sx = (uint64_t)ny * sy;   // element strides of the grid
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
    const T x1 = kx[xi], x2 = kx[xi + 1u], y1 = ky[yi], y2 = ky[yi + 1u], z1 = kz[zi], z2 = kz[zi + 1u];
    const T* g = A.data + ((uint64_t)xi * sx + (uint64_t)yi * sy + (uint64_t)zi * sz + v * (uint64_t)VEC);
    const V d000 = *reinterpret_cast<const V*>(g), d001 = *reinterpret_cast<const V*>(g + sz);
    const V d010 = *reinterpret_cast<const V*>(g + sy), d011 = *reinterpret_cast<const V*>(g + sy + sz);
    const V d100 = *reinterpret_cast<const V*>(g + sx), d101 = *reinterpret_cast<const V*>(g + sx + sz);
    const V d110 = *reinterpret_cast<const V*>(g + sx + sy), d111 = *reinterpret_cast<const V*>(g + sx + sy + sz);
    const SharedDivisor<T> dx = shared_divisor<T>(x2 - x1), dy = shared_divisor<T>(y2 - y1), dz = shared_divisor<T>(z2 - z1);
    const V c00 = frac_shared<T, V>(x1, d000, dx, d100, x);   // bilinear.rs:94-96 on the slab k ...
    const V c10 = frac_shared<T, V>(x1, d010, dx, d110, x);
    const V c01 = frac_shared<T, V>(x1, d001, dx, d101, x);   // ... and on the slab k + 1
    const V c11 = frac_shared<T, V>(x1, d011, dx, d111, x);
    const V c0 = frac_shared<T, V>(y1, c00, dy, c10, y);
    const V c1 = frac_shared<T, V>(y1, c01, dy, c11, y);
    const V res = frac_shared<T, V>(z1, c0, dz, c1, z);
    __builtin_nontemporal_store(res, reinterpret_cast<V*>(A.out + r * A.out_stride + v * (uint64_t)VEC));
  }
}

}  // namespace ndi
