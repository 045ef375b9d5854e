// csrc/antiderivative_kernels.hpp -- antiderivative handles of the cubic evaluation class and of Linear.
//
// The antiderivative of a piecewise cubic is a piecewise quartic: it does not fit the evaluation form the other kernels
// share, so it has a prefix table P[n][lanes] (the integral from x[0] to every knot), a build of its own (a scan along
// the knot axis) and evaluation kernels of its own.  The search is the existing one (locate_kernel: idx[], t[]).
//
// Numerical contract (include/ndinterp.h, ndi_interp1d_antiderivative): every line one IEEE operation in T, in the stated
// order, nothing fused (-ffp-contract=off, correctly rounded division); tests/antiderivative_ref.py restates it in numpy.
//   cubic class:  dy = yr - yl;  c1 = (dy + a) * 0.5;  c2 = (b - (a + a)) / 3;  c3 = (b - a) * 0.25
//                 G(t) = t * (yl + t * (c1 + t * (c2 - t * c3)));  I[i] = dx * (yl + (c1 + (c2 - c3)))
//   Linear:       c1 = (yr - yl) * 0.5;  G(t) = t * (yl + t * c1);  I[i] = dx * (yl + c1)
//   F(xq) = P[i] + dx * G(t)
// The prefix table is a FIXED blocked sum, AD_B = 256 knots per block, whatever the launch geometry:
//   S[i] = +0 where i % B == 0, else S[i-1] + I[i-1];  T[k] = S[kB + B - 1] + I[kB + B - 1];  O[0] = +0, O[k+1] = O[k] + T[k]
//   P[i] = O[i / B] + S[i]
//
// Build, at most three launches (I is formed on the fly and never reaches memory):
//   antideriv_local_lanes_kernel    S -> P and T, one thread per (block, lane or 16-byte vector of lanes), consecutive
//                                   threads on consecutive lanes: coalesced rows, nblk * lanes / VN chains of 256 steps
//   antideriv_local_staged_kernel   the same for rows of up to AD_STAGED_LANES lanes (scalar data: 1e6 x 1 has 3907 blocks
//                                   and one lane): a workgroup reads the intervals of KB consecutive blocks coalesced, parks
//                                   I in LDS, KB * lanes threads run the 256-step chains out of LDS, all threads write S back
//   antideriv_offsets_kernel        T -> O in place, serially per lane: a thread per lane for long rows, a WAVE per lane for
//                                   short ones (64 totals per coalesced load, the chain runs over v_readlane)
//   antideriv_add_kernel            P[i] = O[i / B] + S[i], elementwise
// One block (n <= 256): the local kernel writes +0 + S itself, one launch.  Up to AD_FUSE_BLOCKS blocks: the add kernel
// sums O[k] from T serially per thread (the same chain, the same bits), two launches.
#pragma once

namespace ndi {

constexpr uint32_t AD_B = 256;            // knots per block of the prefix sum: part of the numerical contract
constexpr uint32_t AD_STAGED_LANES = 32;  // rows of up to this many lanes take the LDS-staged local kernel
constexpr uint32_t AD_STAGED_CHAINS = 32; // ... with at most this many chains (blocks x lanes) per workgroup
constexpr uint32_t AD_FUSE_BLOCKS = 17;   // up to this many blocks the add kernel forms O itself

// I of one interval from its operands (cubic class / Linear).
template <bool LINEAR, class T, class V>
__device__ __forceinline__ V antideriv_interval(V yl, V yr, V a, V b, T dx) {
  if constexpr (LINEAR) {
    const V c1 = (yr - yl) * T(0.5);
    return dx * (yl + c1);
  } else {
    const V dy = yr - yl;
    const V c1 = (dy + a) * T(0.5);
    const V c2 = (b - (a + a)) / T(3);
    const V c3 = (b - a) * T(0.25);
    return dx * (yl + (c1 + (c2 - c3)));
  }
}

// dx * G(t) of one interval.
template <bool LINEAR, class T, class V>
__device__ __forceinline__ V antideriv_point(V yl, V yr, V a, V b, T dx, T t) {
  if constexpr (LINEAR) {
    const V c1 = (yr - yl) * T(0.5);
    return dx * (t * (yl + t * c1));
  } else {
    const V dy = yr - yl;
    const V c1 = (dy + a) * T(0.5);
    const V c2 = (b - (a + a)) / T(3);
    const V c3 = (b - a) * T(0.25);
    return dx * (t * (yl + t * (c1 + t * (c2 - t * c3))));
  }
}

template <class T>
struct AntiBuildArgs {
  const T* y;   // source tables: [n][lanes], [n-1][lanes], [n-1][lanes] (Linear: a == b == nullptr)
  const T* a;
  const T* b;
  const T* x;   // [n] knots
  T* P;         // [n][lanes]: S after the local kernel, the prefix table after the add
  T* tot;       // [nblk][lanes]: T after the local kernel, O after the offsets kernel
  uint64_t n, lanes, nblk;
  uint32_t kb;      // staged kernel: blocks per workgroup
  uint32_t single;  // one block: the local kernel writes +0 + S
};

// ---- local sums, lanes across threads ---------------------------------------------------------------------------------
template <class T, int VN, bool LINEAR>
__global__ __launch_bounds__(BLOCK) void antideriv_local_lanes_kernel(AntiBuildArgs<T> A) {
  using V = typename VecT<T, VN>::type;
  constexpr int U = 4;   // intervals whose operand rows are requested together: the loads do not depend on the chain
  const uint64_t L = A.lanes, LV = L / VN, total = A.nblk * LV;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    const uint64_t k = e / LV, lv = e - k * LV;
    const uint64_t i0 = k * AD_B;                                          // first knot of the block
    const uint64_t cnt = (A.n - i0 < AD_B) ? A.n - i0 : (uint64_t)AD_B;      // its knots
    const uint64_t nint = (A.n - 1 - i0 < AD_B) ? A.n - 1 - i0 : (uint64_t)AD_B;   // its intervals (the last block: cnt - 1)
    const uint64_t col = lv * VN;
    V S = V(T(0));
    V yl = *reinterpret_cast<const V*>(A.y + NDI_CHK(i0, A.n, BC_INTERVAL) * L + col);
    uint64_t j = 0;
    for (; j + U <= nint; j += U) {
      V ry[U], ra[U], rb[U];
      T rdx[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t i = NDI_CHK(i0 + j + u, A.n - 1, BC_INTERVAL);
        ry[u] = *reinterpret_cast<const V*>(A.y + (i + 1) * L + col);
        if constexpr (!LINEAR) {
          ra[u] = *reinterpret_cast<const V*>(A.a + i * L + col);
          rb[u] = *reinterpret_cast<const V*>(A.b + i * L + col);
        } else {
          ra[u] = V(T(0));
          rb[u] = V(T(0));
        }
        rdx[u] = const_load(A.x, i + 1) - const_load(A.x, i);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t i = i0 + j + u;
        *reinterpret_cast<V*>(A.P + i * L + col) = A.single ? V(T(0)) + S : S;
        S = S + antideriv_interval<LINEAR, T, V>(yl, ry[u], ra[u], rb[u], rdx[u]);
        yl = ry[u];
      }
    }
    for (; j < nint; ++j) {
      const uint64_t i = NDI_CHK(i0 + j, A.n - 1, BC_INTERVAL);
      const V yr = *reinterpret_cast<const V*>(A.y + (i + 1) * L + col);
      V a = V(T(0)), b = V(T(0));
      if constexpr (!LINEAR) {
        a = *reinterpret_cast<const V*>(A.a + i * L + col);
        b = *reinterpret_cast<const V*>(A.b + i * L + col);
      }
      const T dx = const_load(A.x, i + 1) - const_load(A.x, i);
      *reinterpret_cast<V*>(A.P + i * L + col) = A.single ? V(T(0)) + S : S;
      S = S + antideriv_interval<LINEAR, T, V>(yl, yr, a, b, dx);
      yl = yr;
    }
    // nint == AD_B: S is T[k], the running sum taken over the block's end; else S is S of the block's (the table's) last knot
    if (nint == AD_B) *reinterpret_cast<V*>(A.tot + k * L + col) = S;
    else if (nint < cnt) *reinterpret_cast<V*>(A.P + NDI_CHK(i0 + nint, A.n, BC_INTERVAL) * L + col) = A.single ? V(T(0)) + S : S;
  }
}

// ---- local sums, short rows: staged through LDS --------------------------------------------------------------------------
// Workgroup w takes the blocks [w * kb, w * kb + kb).  LDS: kb sub-tiles of AD_B * lanes + lanes elements (the pad moves the
// chains of neighbouring blocks to other banks).  Phase 1: every thread forms I for its share of the tile's (interval, lane)
// pairs, in memory order (coalesced).  Phase 2: thread c < kb * lanes runs chain (block c / lanes, lane c % lanes) over the
// tile, leaving S where I was.  Phase 3: every thread writes its share of S back, in memory order.
template <class T, bool LINEAR>
__global__ __launch_bounds__(BLOCK) void antideriv_local_staged_kernel(AntiBuildArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ad_smem[];
  T* tile = reinterpret_cast<T*>(ad_smem);
  const uint32_t L = (uint32_t)A.lanes, kb = A.kb;
  const uint32_t sub = AD_B * L + L;   // elements per sub-tile
  for (uint64_t k0 = (uint64_t)blockIdx.x * kb; k0 < A.nblk; k0 += (uint64_t)gridDim.x * kb) {
    const uint64_t i0 = k0 * AD_B;
    const uint64_t knots = (A.n - i0 < (uint64_t)kb * AD_B) ? A.n - i0 : (uint64_t)kb * AD_B;          // knots of the tile
    const uint64_t ints = (A.n - 1 - i0 < (uint64_t)kb * AD_B) ? A.n - 1 - i0 : (uint64_t)kb * AD_B;   // its intervals
    const uint32_t items = (uint32_t)ints * L;
    for (uint32_t e = threadIdx.x; e < items; e += BLOCK) {
      const uint32_t j = e / L, l = e - j * L;
      const uint64_t i = NDI_CHK(i0 + j, A.n - 1, BC_INTERVAL);
      const T yl = A.y[i * L + l], yr = A.y[(i + 1) * L + l];
      const T a = LINEAR ? T(0) : A.a[i * L + l];
      const T b = LINEAR ? T(0) : A.b[i * L + l];
      const T dx = const_load(A.x, i + 1) - const_load(A.x, i);
      tile[(j / AD_B) * sub + (j % AD_B) * L + l] = antideriv_interval<LINEAR, T, T>(yl, yr, a, b, dx);
    }
    __syncthreads();
    if (threadIdx.x < kb * L) {
      const uint32_t kk = threadIdx.x / L, l = threadIdx.x - kk * L;
      const uint64_t k = k0 + kk;
      if (k < A.nblk) {
        const uint64_t b0 = k * AD_B;
        const uint32_t nint = (uint32_t)((A.n - 1 - b0 < AD_B) ? A.n - 1 - b0 : (uint64_t)AD_B);
        T* p = tile + kk * sub + l;
        T S = T(0);
        for (uint32_t j = 0; j < nint; ++j) {
          const T v = p[j * L];
          p[j * L] = S;
          S = S + v;
        }
        if (nint == AD_B) A.tot[k * L + l] = S;
        else p[nint * L] = S;   // S of the table's last knot, which lies in this block (nint <= AD_B - 1: inside the sub-tile)
      }
    }
    __syncthreads();
    const uint32_t kitems = (uint32_t)knots * L;
    for (uint32_t e = threadIdx.x; e < kitems; e += BLOCK) {
      const uint32_t j = e / L, l = e - j * L;
      const T S = tile[(j / AD_B) * sub + (j % AD_B) * L + l];
      A.P[NDI_CHK(i0 + j, A.n, BC_INTERVAL) * L + l] = A.single ? T(0) + S : S;
    }
    __syncthreads();
  }
}

// ---- block offsets: T -> O in place, serially per lane -------------------------------------------------------------------
// nfull: the blocks whose total was written (a last block that is not full has none; its O is still stored).
// WAVE == false: one thread per lane, consecutive threads on consecutive lanes (long rows, few blocks).
// WAVE == true:  one wave per lane (short rows, many blocks): the wave reads 64 consecutive totals of its lane with one
//                load, the chain runs over them with v_readlane in block order, every lane keeps the offset of its block.
//                Only the adds are on the dependent path; whole groups of 64 run without a branch.
template <class T>
__device__ __forceinline__ void antideriv_offsets_step(T& O, T& mine, T v, uint32_t lane, int j) {
  mine = lane == (uint32_t)j ? O : mine;
  O = O + readlane_t(v, j);
}

template <class T, bool WAVE>
__global__ __launch_bounds__(BLOCK) void antideriv_offsets_kernel(T* tot, uint64_t nblk, uint64_t nfull, uint64_t lanes) {
  if constexpr (!WAVE) {
    const uint64_t l = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (l >= lanes) return;
    T O = T(0);
    for (uint64_t k = 0; k < nblk; ++k) {
      const T v = k < nfull ? tot[k * lanes + l] : T(0);
      tot[k * lanes + l] = O;
      O = O + v;
    }
  } else {
    const uint64_t l = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) / 64u;   // wave-uniform
    const uint32_t lane = threadIdx.x & 63u;
    if (l >= lanes) return;
    T O = T(0);
    T next = lane < nfull ? tot[(uint64_t)lane * lanes + l] : T(0);            // one group ahead of the chain
    for (uint64_t k0 = 0; k0 < nblk; k0 += 64u) {
      const uint64_t k = k0 + lane;
      const T v = next;
      next = k + 64u < nfull ? tot[(k + 64u) * lanes + l] : T(0);
      T mine = T(0);
      if (nblk - k0 >= 64u) {
#pragma unroll
        for (int j = 0; j < 64; ++j) antideriv_offsets_step(O, mine, v, lane, j);
      } else {
        const uint32_t cnt = (uint32_t)(nblk - k0);   // wave-uniform
#pragma unroll
        for (int j = 0; j < 64; ++j)
          if ((uint32_t)j < cnt) antideriv_offsets_step(O, mine, v, lane, j);
      }
      if (k < nblk) tot[k * lanes + l] = mine;
    }
  }
}

// ---- P[i] = O[i / B] + S[i] ------------------------------------------------------------------------------------------------
// FUSE: tot still holds T; every thread forms O[k] by the serial chain itself (few blocks).
template <class T, int VN, bool FUSE>
__global__ __launch_bounds__(BLOCK) void antideriv_add_kernel(AntiBuildArgs<T> A) {
  using V = typename VecT<T, VN>::type;
  const uint64_t L = A.lanes, LV = L / VN, total = A.n * LV;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += step) {
    uint64_t i, lv;
    if (LV == 1) {
      i = e;
      lv = 0;
    } else if (total <= 0xffffffffull) {
      const uint32_t q = (uint32_t)e / (uint32_t)LV;
      i = q;
      lv = (uint32_t)e - q * (uint32_t)LV;
    } else {
      i = e / LV;
      lv = e - i * LV;
    }
    i = NDI_CHK(i, A.n, BC_INTERVAL);
    const uint64_t k = i / AD_B, col = lv * VN;
    V O = V(T(0));
    if constexpr (FUSE) {
      for (uint64_t kk = 0; kk < k; ++kk) O = O + *reinterpret_cast<const V*>(A.tot + kk * L + col);
    } else {
      O = *reinterpret_cast<const V*>(A.tot + k * L + col);
    }
    V* p = reinterpret_cast<V*>(A.P + i * L + col);
    *p = O + *p;
  }
}

// ---- evaluation ------------------------------------------------------------------------------------------------------------
template <class T>
struct AntiEvalArgs {
  const T* knots;
  const T* y;      // [n][lanes]
  const T* a;      // [n-1][lanes] (cubic class)
  const T* b;
  const T* P;      // [n][lanes]
  const uint32_t* idx;    // interval and t per query (locate_kernel)
  const T* t;
  const uint32_t* idx2;   // PAIR (ndi_interp1d_integrate): idx / t are lo's, idx2 / t2 hi's
  const T* t2;
  T* out;
  uint64_t lanes, out_stride, nq;
  const StatusBlock* status;   // first_fail[0]: eval's queries / lo; first_fail[1]: hi
  uint32_t n_int;              // n - 1: limit of every interval index (checked build)
};

template <class T>
__device__ __forceinline__ unsigned long long antideriv_limit(const AntiEvalArgs<T>& A) {
  unsigned long long limit = A.status->first_fail[0];
  if (A.status->first_fail[1] < limit) limit = A.status->first_fail[1];
  return limit > A.nq ? A.nq : limit;
}

// F at (interval i, t) for the lanes [v * VN, v * VN + VN).
template <class T, class V, bool LINEAR>
__device__ __forceinline__ V antideriv_row(const AntiEvalArgs<T>& A, uint32_t i, T t, T dx, uint64_t v) {
  const uint64_t row = (uint64_t)i * A.lanes;
  const V yl = reinterpret_cast<const V*>(A.y + row)[v];
  const V yr = reinterpret_cast<const V*>(A.y + row + A.lanes)[v];
  V a = V(T(0)), b = V(T(0));
  if constexpr (!LINEAR) {
    a = reinterpret_cast<const V*>(A.a + row)[v];
    b = reinterpret_cast<const V*>(A.b + row)[v];
  }
  const V p = reinterpret_cast<const V*>(A.P + row)[v];
  return p + antideriv_point<LINEAR, T, V>(yl, yr, a, b, dx, t);
}

// Long rows (as eval_rows_kernel): grid.x strides over queries, grid.y over 256-vector segments of a row; 16-byte loads,
// non-temporal 16-byte stores.
template <class T, bool LINEAR, bool PAIR>
__global__ __launch_bounds__(BLOCK) void antideriv_eval_rows_kernel(AntiEvalArgs<T> A) {
  constexpr int VN = Wide<T>::N;
  using V = typename VecT<T, VN>::type;
  const uint64_t LV = A.lanes / VN;
  const uint32_t segs = (uint32_t)((LV + BLOCK - 1) / BLOCK);
  const unsigned long long limit = antideriv_limit(A);
  for (uint64_t qi = blockIdx.x; qi < limit; qi += gridDim.x) {
    const uint32_t i = NDI_CHK(A.idx[qi], A.n_int, BC_INTERVAL);
    const T t = A.t[qi];
    const T dx = A.knots[i + 1] - A.knots[i];
    uint32_t i2 = 0;
    T t2 = T(0), dx2 = T(0);
    if constexpr (PAIR) {
      i2 = NDI_CHK(A.idx2[qi], A.n_int, BC_INTERVAL);
      t2 = A.t2[qi];
      dx2 = A.knots[i2 + 1] - A.knots[i2];
    }
    V* o = reinterpret_cast<V*>(A.out + qi * A.out_stride);
    for (uint32_t seg = blockIdx.y; seg < segs; seg += gridDim.y) {
      const uint64_t v = (uint64_t)seg * BLOCK + threadIdx.x;
      if (v >= LV) continue;
      const V f = antideriv_row<T, V, LINEAR>(A, i, t, dx, v);
      if constexpr (PAIR) store_stream<true>(o + v, antideriv_row<T, V, LINEAR>(A, i2, t2, dx2, v) - f);
      else store_stream<true>(o + v, f);
    }
  }
}

// Short / unaligned rows (as eval_flat_kernel): one VEC-wide output vector per thread, tile_q queries per workgroup tile.
template <class T, bool LINEAR, bool PAIR, int VEC>
__global__ __launch_bounds__(BLOCK) void antideriv_eval_flat_kernel(AntiEvalArgs<T> A, uint32_t tile_q) {
  using V = typename VecT<T, VEC>::type;
  const uint32_t LV = (uint32_t)(A.lanes / VEC);
  const unsigned long long limit = antideriv_limit(A);
  const uint64_t ntiles = (limit + tile_q - 1) / tile_q;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t q0 = tile * tile_q;
    const uint32_t nq_here = (limit - q0 < tile_q) ? (uint32_t)(limit - q0) : tile_q;
    const uint32_t items = nq_here * LV;
    for (uint32_t it = threadIdx.x; it < items; it += BLOCK) {
      const uint32_t ql = it / LV;
      const uint32_t v = it - ql * LV;
      const uint64_t qi = q0 + ql;
      const uint32_t i = NDI_CHK(A.idx[qi], A.n_int, BC_INTERVAL);
      const V f = antideriv_row<T, V, LINEAR>(A, i, A.t[qi], A.knots[i + 1] - A.knots[i], v);
      V* o = reinterpret_cast<V*>(A.out + qi * A.out_stride);
      if constexpr (PAIR) {
        const uint32_t i2 = NDI_CHK(A.idx2[qi], A.n_int, BC_INTERVAL);
        o[v] = antideriv_row<T, V, LINEAR>(A, i2, A.t2[qi], A.knots[i2 + 1] - A.knots[i2], v) - f;
      } else {
        o[v] = f;
      }
    }
  }
}

}  // namespace ndi
