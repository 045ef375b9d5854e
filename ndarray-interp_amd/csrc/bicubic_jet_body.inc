// csrc/bicubic_jet_body.inc -- the body of eval_bicubic_jet_kernel and eval_bicubic_jet_wrap_kernel (bicubic_jet_kernels.hpp),
// included inside each of them after `constexpr bool WRAP = ...;`.  Shared as text, not as an inlined function: the sixteen
// instances of the kernel that does not wrap then compile to the code they were, instruction for instruction (an inlined
// body taking the arguments by reference scheduled their argument loads differently).  In scope: T, VEC, KLDS, TB, ORDER,
// WRAP and the kernel's argument A.
  static_assert(ORDER == 1 || ORDER == 2, "orders 1 and 2");
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
      const uint64_t row = (base + ql) * A.out_stride;
      auto put = [&](int k, V r) { store_stream<true>(reinterpret_cast<V*>(A.out[k] + row) + v, r); };
      // P0: the y-forms of order 0 -- the value and the pure x-partials
      const V p0 = hermite_nu<0, T, V>(z00, z01, zy00, zy01, hy, u, cu, cu2);
      const V p1 = hermite_nu<0, T, V>(z10, z11, zy10, zy11, hy, u, cu, cu2);
      const V d0 = hermite_nu<0, T, V>(zx00, zx01, zxy00, zxy01, hy, u, cu, cu2);
      const V d1 = hermite_nu<0, T, V>(zx10, zx11, zxy10, zxy11, hy, u, cu, cu2);
      put(0, hermite_nu<0, T, V>(p0, p1, d0, d1, hx, t, ct, ct2));
      put(1, hermite_nu<1, T, V>(p0, p1, d0, d1, hx, t, ct, ct2));
      if constexpr (ORDER == 2) put(3, hermite_nu<2, T, V>(p0, p1, d0, d1, hx, t, ct, ct2));
      // P1: the y-forms of order 1
      const V p0y = hermite_nu<1, T, V>(z00, z01, zy00, zy01, hy, u, cu, cu2);
      const V p1y = hermite_nu<1, T, V>(z10, z11, zy10, zy11, hy, u, cu, cu2);
      const V d0y = hermite_nu<1, T, V>(zx00, zx01, zxy00, zxy01, hy, u, cu, cu2);
      const V d1y = hermite_nu<1, T, V>(zx10, zx11, zxy10, zxy11, hy, u, cu, cu2);
      put(2, hermite_nu<0, T, V>(p0y, p1y, d0y, d1y, hx, t, ct, ct2));
      if constexpr (ORDER == 2) {
        put(4, hermite_nu<1, T, V>(p0y, p1y, d0y, d1y, hx, t, ct, ct2));
        // P2: the y-forms of order 2
        const V p0yy = hermite_nu<2, T, V>(z00, z01, zy00, zy01, hy, u, cu, cu2);
        const V p1yy = hermite_nu<2, T, V>(z10, z11, zy10, zy11, hy, u, cu, cu2);
        const V d0yy = hermite_nu<2, T, V>(zx00, zx01, zxy00, zxy01, hy, u, cu, cu2);
        const V d1yy = hermite_nu<2, T, V>(zx10, zx11, zxy10, zxy11, hy, u, cu, cu2);
        put(5, hermite_nu<0, T, V>(p0yy, p1yy, d0yy, d1yy, hx, t, ct, ct2));
      }
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
