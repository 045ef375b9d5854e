// csrc/bicubic_jet_kernels.hpp -- the fused value-and-derivatives (jet) evaluation of the 2-D Bicubic strategy
// (ndi_interp2d_eval_jet): the surface and its partial derivatives up to ORDER at the same queries, from ONE read of the
// sixteen operand vectors of the node table {z, zx, zy, zxy}.
//
//   eval_bicubic_jet_kernel<T, VEC, KLDS, TB, ORDER>, eval_bicubic_jet_wrap_kernel<T, VEC, KLDS, TB, ORDER>
//                               eval_bicubic_kernel's geometry (bicubic_kernels.hpp): query order with both searches fused
//                               in, the wave-private strip {record offset, t, u, hx, hy}, short rows sharing a trip through
//                               lv_magic, long rows cut into `vchunk` pieces along blockIdx.y, knots in LDS (KLDS) or in
//                               global memory, the fresh-output range test on blockIdx.y == 0 only.  Per item: the same
//                               sixteen loads; per grid row the y-forms H_0 .. H_ORDER of (z, zy) and of (zx, zxy); then
//                               the x-forms, K = 3 (ORDER 1) or 6 (ORDER 2) of them, each with a streaming store of its own:
//                                   part 0 (0,0) = H0x(P0)    part 1 (1,0) = H1x(P0)    part 2 (0,1) = H0x(P1)
//                                   part 3 (2,0) = H2x(P0)    part 4 (1,1) = H1x(P1)    part 5 (0,2) = H0x(P2)
//                               where Pm = the four y-forms of order m.  The prologue is eval_bicubic_kernel's, restated
//                               here so that kernel's instances compile to the code they were.  The _wrap_ kernel is the
//                               variant of a handle that wraps on a periodic axis (bicubic_wrap_query before the search,
//                               as eval_bicubic_kernel's WRAP): both kernels are one body, bicubic_jet_body.inc.
//
// Numerical contract: no formula of its own.  Every form is a call of hermite_nu<NU> (bicubic_kernels.hpp), so part k is,
// bit for bit, the row eval_bicubic_kernel<.., nu_x, nu_y> writes: the shared lines d, a, b of two forms on the same
// operands are the same IEEE operations (-ffp-contract=off), whether the compiler merges them or not.
#pragma once

#include <type_traits>

namespace ndi {

constexpr int JET_MAX_PARTS = 6;

template <class T>
struct BicubicJetArgs {
  Pyramid<T> px, py;
  const T* table;          // T[nx][ny][4][lanes]
  const T* qx;
  const T* qy;
  T* out[JET_MAX_PARTS];   // part k of query i: out[k] + i * out_stride; the first K are set
  uint64_t nq, out_stride;
  uint64_t lv;             // vectors per part row (lanes / VEC)
  uint32_t lv_magic;       // ceil(2^32 / lv) for 2 <= lv < 64
  uint32_t vchunk;         // vectors of a row per blockIdx.y (a multiple of 64; >= lv when gridDim.y == 1)
  int mode;
  int wrap;                // WRAP variants: the axes that wrap (bit 0: x, bit 1: y); sits in the padding after `mode`
  unsigned long long* first_fail;   // [2]: x, y (range_check_kernel, or this kernel when `check`)
  int check;                        // fresh output: the kernel's own range test, no pre-pass
};

// One body (bicubic_jet_body.inc), two kernels: the jet of a handle that does not wrap -- its sixteen instances keep their
// names and their code -- and the variant of a handle that wraps.
template <class T, int VEC, bool KLDS, int TB, int ORDER>
__global__ __launch_bounds__(TB) void eval_bicubic_jet_kernel(BicubicJetArgs<T> A) {
  constexpr bool WRAP = false;
#include "bicubic_jet_body.inc"
}

template <class T, int VEC, bool KLDS, int TB, int ORDER>
__global__ __launch_bounds__(TB) void eval_bicubic_jet_wrap_kernel(BicubicJetArgs<T> A) {
  constexpr bool WRAP = true;
#include "bicubic_jet_body.inc"
}

}  // namespace ndi
