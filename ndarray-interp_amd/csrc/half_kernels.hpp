// csrc/half_kernels.hpp -- the f16 / bf16 Linear and Bilinear kernels (included by kernels.hpp).
//
// The reference's Linear and Bilinear are generic over `T: Num + PartialOrd + ...` (linear.rs:13-36,
// bilinear.rs:20-27, 64-99); for T = half::f16 / half::bf16 every operation converts both operands to f32 exactly,
// does one IEEE f32 operation and rounds the result to T (round to nearest even, overflow to inf).  These kernels do
// the same: the library is built with -ffp-contract=off and correctly rounded f32 division, and f32 subnormals are
// kept (float_denorm_mode_32 = 3), so every operation below is bit-exact to `half`'s.  For f16 the compiler turns the
// add / subtract / multiply steps into native f16 instructions, which give the same bits; the division is kept in f32
// (opaque_f32).
//   half_eval1d_kernel     Linear::calc_frac per output element: dy = r(y2 - y1), m = r(dy / dx), p = r(m * d),
//                          r(p + y1), with dx = r(x2 - x1) and d = r(x - x1) per query.  WAVE: one query per group of
//                          2^glog lanes (up to a wavefront), the row streamed with 16-byte loads and stores (8 elements,
//                          VEC) when rows are aligned;
//                          FLAT: one output element per thread (short rows, scalar data)
//   half_eval2d_kernel     Bilinear (bilinear.rs:83-97): z1, z2 along x, then along y, each a calc_frac in T; the same
//                          two mappings
//   half_check_kernel      write-free range pre-pass for caller-owned buffers (first-error semantics): reads queries only
//   half_to_f32_kernel     f32 images of T values (the locator searches on them)
// Every f16 / bf16 value converts to f32 exactly and the conversion keeps order, so the interval search runs on f32
// images of the knots (staged in LDS when they fit) and of the queries, and finds what get_lower_index finds on T.
// `limit` (optional): rows at / after *limit are skipped -- the first failure found by a pre-pass on the same stream, so
// caller-owned buffers keep the reference's state without a host round trip.
#pragma once

namespace ndi {

enum HalfFmt : int { HF_F16 = 0, HF_BF16 = 1 };
constexpr uint32_t HALF_LDS_KNOTS = 4096;   // f32 knot images staged in LDS (16 KiB) up to this many (both axes for 2-D)

template <int F>
__device__ __forceinline__ float h2f(uint16_t u) {
  if (F == HF_F16) return (float)__builtin_bit_cast(_Float16, u);
  return __uint_as_float((uint32_t)u << 16);
}
template <int F>
__device__ __forceinline__ uint16_t f2h(float f) {
  if (F == HF_F16) return __builtin_bit_cast(uint16_t, (_Float16)f);   // v_cvt_f16_f32: RNE, subnormals kept
  const uint32_t b = __float_as_uint(f);
  if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((b >> 16) | 0x40u);   // NaN stays NaN (quiet)
  return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);                  // RNE; carries into inf on overflow
}
template <int F>
__device__ __forceinline__ float hr(float v) {   // one T operation's rounding
  return h2f<F>(f2h<F>(v));
}

// VectorExtensions::get_lower_index on f32 images: the unique i with k[i] <= x < k[i+1], clamped to [0, n-2].
__device__ __forceinline__ uint32_t half_lower_index(const float* k, uint32_t n, float x) {
  if (x <= k[0]) return 0;
  if (x >= k[n - 1]) return n - 2;
  uint32_t lo = 0, hi = n - 1;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (k[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// An f32 value the optimiser cannot see through.  For f16, LLVM folds fptrunc(op(fpext a, fpext b)) into the native
// half operation: harmless for add / subtract / multiply (rounding twice through f32 is exact for f16, 24 >= 2 * 11 + 2)
// but not for the division, whose f16 lowering is an approximate reciprocal with a fix-up.  Hiding the divisor and the
// dividend keeps the correctly rounded f32 division (v_div_scale / v_div_fmas / v_div_fixup_f32) before the RNE
// conversion.
__device__ __forceinline__ float opaque_f32(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Linear::calc_frac (linear.rs:29-36) for one lane; dx = r(x2 - x1) and d = r(x - x1) are the query's.
template <int F>
__device__ __forceinline__ float half_frac(float y1, float y2, float dx, float d) {
  const float dy = hr<F>(y2 - y1);
  const float m = hr<F>(opaque_f32(dy) / opaque_f32(dx));   // the f32 division, never the f16 one
  const float p = hr<F>(m * d);
  return hr<F>(p + y1);
}

struct HalfBounds {   // the knots' ends (range test, linear.rs:81-83 / bilinear.rs:71-80)
  float x0, xn, y0, yn;
};

__device__ __forceinline__ bool half_bad1(int mode, const HalfBounds& b, float x) {
  return mode == EX_NO ? !((b.x0 <= x) && (x <= b.xn)) : !(x == x);
}
__device__ __forceinline__ bool half_bad2(int mode, const HalfBounds& b, float x, float y) {
  return mode == EX_NO ? !((b.x0 <= x) && (x <= b.xn) && (b.y0 <= y) && (y <= b.yn)) : !(x == x && y == y);
}

// Stages `n` f32 knot images in LDS when `lds`; returns the pointer the search reads.
__device__ __forceinline__ const float* half_stage(const float* __restrict__ k, uint32_t n, bool lds, float* sk) {
  if (!lds) return k;
  for (uint32_t i = threadIdx.x; i < n; i += BLOCK) sk[i] = k[i];
  __syncthreads();
  return sk;
}

template <int F>
__global__ __launch_bounds__(BLOCK) void half_check_kernel(const uint16_t* __restrict__ qx,
                                                           const uint16_t* __restrict__ qy, uint64_t nq, int mode,
                                                           HalfBounds b, unsigned long long* __restrict__ first_fail) {
  for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * BLOCK) {
    const float x = h2f<F>(qx[j]);
    const bool bad = qy ? half_bad2(mode, b, x, h2f<F>(qy[j])) : half_bad1(mode, b, x);
    if (bad) atomicMin(first_fail, (unsigned long long)j);
  }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// element e of 8 packed in a 16-byte vector
template <int F>
__device__ __forceinline__ float h8(const u32x4& v, int e) {
  return h2f<F>((uint16_t)(v[e >> 1] >> ((e & 1) * 16)));
}

// 1-D.  CHECK: failing queries are reported (atomicMin) and their rows skipped (the fused form for fresh outputs);
// without it every query below the limit is valid.
template <int F, bool WAVE, bool CHECK, bool VEC>
__global__ __launch_bounds__(BLOCK) void half_eval1d_kernel(const uint16_t* __restrict__ q, uint64_t nq,
                                                            const float* __restrict__ kf, uint32_t n, int mode,
                                                            HalfBounds b, bool lds, const uint16_t* __restrict__ data,
                                                            uint64_t lanes, uint16_t* __restrict__ out, uint64_t stride,
                                                            uint32_t glog, const unsigned long long* __restrict__ limit,
                                                            unsigned long long* __restrict__ first_fail) {
  extern __shared__ float half_sk[];
  const float* k = half_stage(kf, n, lds, half_sk);
  const uint64_t lim = limit ? min(nq, (uint64_t)*limit) : nq;
  if (WAVE) {
    const uint64_t G = 1ull << glog;   // lanes of a query group (a power of two, at most a wavefront)
    const uint64_t lane = threadIdx.x & (G - 1);
    const uint64_t groups = (uint64_t)gridDim.x * (BLOCK >> glog);
    for (uint64_t j = (uint64_t)blockIdx.x * (BLOCK >> glog) + (threadIdx.x >> glog); j < lim; j += groups) {
      const float x = h2f<F>(q[j]);
      if (CHECK && half_bad1(mode, b, x)) {
        if (lane == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const uint32_t i = NDI_CHK(half_lower_index(k, n, x), n - 1, BC_INTERVAL);
      const float x1 = k[i];
      const float dx = hr<F>(k[i + 1] - x1), d = hr<F>(x - x1);
      const uint16_t* r1 = data + (uint64_t)i * lanes;
      const uint16_t* r2 = r1 + lanes;
      uint16_t* o = out + j * stride;
      if (VEC) {   // lanes % 8 == 0, rows and output 16-byte aligned (host)
        for (uint64_t c = lane; c < lanes / 8; c += G) {
          const u32x4 a = *reinterpret_cast<const u32x4*>(r1 + c * 8);
          const u32x4 e = *reinterpret_cast<const u32x4*>(r2 + c * 8);
          u32x4 res;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const uint32_t lo = f2h<F>(half_frac<F>(h8<F>(a, 2 * w), h8<F>(e, 2 * w), dx, d));
            const uint32_t hi = f2h<F>(half_frac<F>(h8<F>(a, 2 * w + 1), h8<F>(e, 2 * w + 1), dx, d));
            res[w] = lo | (hi << 16);
          }
          __builtin_nontemporal_store(res, reinterpret_cast<u32x4*>(o + c * 8));
        }
      } else {
        for (uint64_t l = lane; l < lanes; l += G)
          o[l] = f2h<F>(half_frac<F>(h2f<F>(r1[l]), h2f<F>(r2[l]), dx, d));
      }
    }
  } else {
    const uint64_t total = lim * lanes;
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
      const uint64_t j = lanes == 1 ? e : e / lanes;
      const uint64_t l = e - j * lanes;
      const float x = h2f<F>(q[j]);
      if (CHECK && half_bad1(mode, b, x)) {
        if (l == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const uint32_t i = NDI_CHK(half_lower_index(k, n, x), n - 1, BC_INTERVAL);
      const float x1 = k[i];
      const float dx = hr<F>(k[i + 1] - x1), d = hr<F>(x - x1);
      const uint16_t* r1 = data + (uint64_t)i * lanes + l;
      out[j * stride + l] = f2h<F>(half_frac<F>(h2f<F>(r1[0]), h2f<F>(r1[lanes]), dx, d));
    }
  }
}

// One query of Bilinear::interp_into: the cell and the query's per-axis differences.
struct HalfCell {
  uint64_t p00, p10;        // element offsets of grid points (xi, yi) and (xi + 1, yi); (., yi + 1) follow at + lanes
  float dx, ddx, dy, ddy;   // r(x2 - x1), r(x - x1), r(y2 - y1), r(y - y1)
};
template <int F>
__device__ __forceinline__ HalfCell half_cell(const float* kx, uint32_t nx, const float* ky, uint32_t ny, float x,
                                              float y, uint64_t lanes) {
  const uint32_t xi = NDI_CHK(half_lower_index(kx, nx, x), nx - 1, BC_CELL_X);
  const uint32_t yi = NDI_CHK(half_lower_index(ky, ny, y), ny - 1, BC_CELL_Y);
  HalfCell c;
  c.p00 = ((uint64_t)xi * ny + yi) * lanes;
  c.p10 = c.p00 + (uint64_t)ny * lanes;
  c.dx = hr<F>(kx[xi + 1] - kx[xi]);
  c.ddx = hr<F>(x - kx[xi]);
  c.dy = hr<F>(ky[yi + 1] - ky[yi]);
  c.ddy = hr<F>(y - ky[yi]);
  return c;
}
template <int F>
__device__ __forceinline__ float half_bilinear(float z11, float z12, float z21, float z22, const HalfCell& c) {
  const float z1 = half_frac<F>(z11, z21, c.dx, c.ddx);   // bilinear.rs:88-97
  const float z2 = half_frac<F>(z12, z22, c.dx, c.ddx);
  return half_frac<F>(z1, z2, c.dy, c.ddy);
}

template <int F, bool WAVE, bool CHECK, bool VEC>
__global__ __launch_bounds__(BLOCK) void half_eval2d_kernel(const uint16_t* __restrict__ qx,
                                                            const uint16_t* __restrict__ qy, uint64_t nq,
                                                            const float* __restrict__ kxf, uint32_t nx,
                                                            const float* __restrict__ kyf, uint32_t ny, int mode,
                                                            HalfBounds b, bool lds, const uint16_t* __restrict__ g,
                                                            uint64_t lanes, uint16_t* __restrict__ out, uint64_t stride,
                                                            uint32_t glog, const unsigned long long* __restrict__ limit,
                                                            unsigned long long* __restrict__ first_fail) {
  extern __shared__ float half_sk[];
  const float* kx = half_stage(kxf, nx, lds, half_sk);
  const float* ky = lds ? half_stage(kyf, ny, true, half_sk + nx) : kyf;
  const uint64_t lim = limit ? min(nq, (uint64_t)*limit) : nq;
  if (WAVE) {
    const uint64_t G = 1ull << glog;   // lanes of a query group (a power of two, at most a wavefront)
    const uint64_t lane = threadIdx.x & (G - 1);
    const uint64_t groups = (uint64_t)gridDim.x * (BLOCK >> glog);
    for (uint64_t j = (uint64_t)blockIdx.x * (BLOCK >> glog) + (threadIdx.x >> glog); j < lim; j += groups) {
      const float x = h2f<F>(qx[j]), y = h2f<F>(qy[j]);
      if (CHECK && half_bad2(mode, b, x, y)) {
        if (lane == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const HalfCell c = half_cell<F>(kx, nx, ky, ny, x, y, lanes);
      const uint16_t* a0 = g + c.p00;   // (xi, yi), then (xi, yi + 1) at + lanes: one contiguous run
      const uint16_t* a1 = g + c.p10;
      uint16_t* o = out + j * stride;
      if (VEC) {
        for (uint64_t v = lane; v < lanes / 8; v += G) {
          const u32x4 z11 = *reinterpret_cast<const u32x4*>(a0 + v * 8);
          const u32x4 z12 = *reinterpret_cast<const u32x4*>(a0 + lanes + v * 8);
          const u32x4 z21 = *reinterpret_cast<const u32x4*>(a1 + v * 8);
          const u32x4 z22 = *reinterpret_cast<const u32x4*>(a1 + lanes + v * 8);
          u32x4 res;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const uint32_t lo = f2h<F>(half_bilinear<F>(h8<F>(z11, 2 * w), h8<F>(z12, 2 * w), h8<F>(z21, 2 * w),
                                                        h8<F>(z22, 2 * w), c));
            const uint32_t hi = f2h<F>(half_bilinear<F>(h8<F>(z11, 2 * w + 1), h8<F>(z12, 2 * w + 1),
                                                        h8<F>(z21, 2 * w + 1), h8<F>(z22, 2 * w + 1), c));
            res[w] = lo | (hi << 16);
          }
          __builtin_nontemporal_store(res, reinterpret_cast<u32x4*>(o + v * 8));
        }
      } else {
        for (uint64_t l = lane; l < lanes; l += G)
          o[l] = f2h<F>(half_bilinear<F>(h2f<F>(a0[l]), h2f<F>(a0[lanes + l]), h2f<F>(a1[l]), h2f<F>(a1[lanes + l]),
                                         c));
      }
    }
  } else {
    const uint64_t total = lim * lanes;
    for (uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BLOCK) {
      const uint64_t j = lanes == 1 ? e : e / lanes;
      const uint64_t l = e - j * lanes;
      const float x = h2f<F>(qx[j]), y = h2f<F>(qy[j]);
      if (CHECK && half_bad2(mode, b, x, y)) {
        if (l == 0) atomicMin(first_fail, (unsigned long long)j);
        continue;
      }
      const HalfCell c = half_cell<F>(kx, nx, ky, ny, x, y, lanes);
      const uint16_t* a0 = g + c.p00 + l;
      const uint16_t* a1 = g + c.p10 + l;
      out[j * stride + l] = f2h<F>(half_bilinear<F>(h2f<F>(a0[0]), h2f<F>(a0[lanes]), h2f<F>(a1[0]),
                                                    h2f<F>(a1[lanes]), c));
    }
  }
}

template <int F>
__global__ __launch_bounds__(BLOCK) void half_to_f32_kernel(const uint16_t* __restrict__ q, uint64_t nq,
                                                            float* __restrict__ out) {
  for (uint64_t j = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; j < nq; j += (uint64_t)gridDim.x * BLOCK)
    out[j] = h2f<F>(q[j]);
}

}  // namespace ndi
