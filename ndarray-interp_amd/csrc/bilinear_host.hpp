// csrc/bilinear_host.hpp -- the evaluation host of 2-D Bilinear (included by ndinterp_api.hip after Interp2DImpl): one planner
// and one launcher per plan, free templates over the handle.  Interp2DImpl::prep is the cascade over plan_lanes2, plan_slopes2,
// plan_small2 and plan_fused2, then plan_tiles, the search (locate2) and group_tiles; launch_eval the switch over the
// launchers.  A planner that accepts enqueues the range pre-pass as its last step, and asks for a lazy device table
// (ensure_dense_lut, ensure_bucket_index, ensure_slopes) only after its cheap conditions have passed: when a table is built, and
// on which stream, is something a caller can observe (tests/test_gpu_lazy_tables.py).
#pragma once

// The bucket indices staged behind the two pyramids: their LDS bytes when the axes have any and pyramids + indices stay within
// `limit`, else 0.  Asks for the lazy build: only for a batch that may use them (>= 4096 queries).
template <class T>
static size_t staged_index_bytes(const Interp2DImpl<T>& h, size_t limit) {
  h.px.ensure_bucket_index();
  h.py.ensure_bucket_index();
  const size_t lut = h.px.lut_bytes + h.py.lut_bytes;
  return lut != 0 && h.small_shmem() + lut <= limit ? lut : 0;
}

// What both query-per-lane kernels stage first: the two axes with their LANE_SENTINELS, each rounded to 16 bytes, and the
// two dense indices (after ensure_dense_lut).
template <class T>
static size_t dense_axes_lds_bytes(const Interp2DImpl<T>& h) {
  return (((size_t)(h.nx + LANE_SENTINELS) * sizeof(T) + 15) & ~(size_t)15) +
         (((size_t)(h.ny + LANE_SENTINELS) * sizeof(T) + 15) & ~(size_t)15) + h.px.dlut_bytes + h.py.dlut_bytes;
}

// LDS of a staged tile of (2^ts + 1)^2 grid points beside its five axis strips: the values alone, values + x slopes, or
// values + x slopes of one half of the trailing axis.  The planner (tile_shape) and the launcher (tile_form) both ask here:
// a tile the planner accepts is one the launcher can stage.
enum TileLds { TILE_VALUES, TILE_SLOPES, TILE_HALF_SLOPES };
template <class T>
static size_t tile_lds_bytes(uint32_t ts, uint64_t lanes, TileLds what) {
  const size_t s1 = ((size_t)1 << ts) + 1;
  const size_t elems = what == TILE_VALUES ? s1 * s1 * lanes : (s1 * s1 + (s1 - 1) * s1) * (what == TILE_HALF_SLOPES ? lanes / 2 : lanes);
  return elems * sizeof(T) + 5 * s1 * sizeof(T) + 16;
}
// ... and the kernel's static LDS beside it: `records` grouped records per hand-over (256 or 1024)
template <class T>
static size_t tile_record_strip_bytes(int records, bool compact) {
  return (size_t)records * 16 + (compact ? 2 : 2 * records) * sizeof(T) + 320;
}

// What the Args of the query-order kernels have alike: the batch, the row pitch, the mode, the status slot, the range test.
template <class A, class T>
static void batch_args(A& F, const Interp2DImpl<T>& h, StatusBlock* st, const Plan2<T>& P) {
  F.qx = P.qx; F.qy = P.qy; F.out = P.out;
  F.nq = P.nq; F.out_stride = P.out_stride;
  F.lanes = (uint32_t)h.lanes; F.mode = h.mode;
  F.first_fail = &st->first_fail[0];
  F.check = P.l_check ? 1 : 0;
}

// Grids that fit LDS beside their axes (the reference's 100 x 100 scalar grid: 80 KB in f64), rows of up to 64 bytes,
// large batches: query per lane with every corner read served by LDS (eval_scalar2d_kernel / eval_lanes2d_kernel).
// NDI_LANES2D_KERNEL=0: A/B.
template <class T>
static bool plan_lanes2(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, Plan2<T>& P, int path, bool fresh) {
  static const Knob on_knob{"NDI_LANES2D_KERNEL", -1, Knob::live};
  const int on = on_knob.get();
  const uint64_t nx = h.nx, ny = h.ny, lanes = h.lanes, nq = P.nq;
  const size_t grid_b = (size_t)nx * ny * lanes * sizeof(T);
  if (!(on != 0 && path != NDI_PATH_BUCKETED && !h.pair_packed && nx <= 16384 && ny <= 16384 && lanes * sizeof(T) <= (on > 0 ? 64 : 56) &&
        grid_b + (nx + ny) * 5 * sizeof(T) <= FUSED_LDS_LIMIT && (uint64_t)nx * ny * lanes < (1ull << 31) &&
        (on > 0 || (nq >= 65536 && (double)nq * (double)lanes * sizeof(T) >= 4.0 * (double)cu_count() * (double)grid_b))))
    return false;
  h.px.ensure_dense_lut();
  h.py.ensure_dense_lut();
  const size_t fixed = dense_axes_lds_bytes(h) + (size_t)(nx - 1 + ny - 1) * 4 * sizeof(T) + ((grid_b + 15) & ~(size_t)15);
  auto need_of = [&](unsigned tb) { return fixed + (lanes > 1 ? (size_t)(tb / 64) * 64 * lanes * sizeof(T) : 0); };
  unsigned tb = need_of(256) * 4 <= 160 * 1024 ? 256u : 1024u;
  if (need_of(tb) > FUSED_LDS_LIMIT) tb = 256u;   // (the strips of 16 waves do not fit: 4 waves)
  if (!(h.px.dense_ok && h.py.dense_ok && need_of(tb) <= FUSED_LDS_LIMIT)) return false;
  P.kind = Plan2<T>::LANES2;
  P.f_tb = tb;
  P.f_lds = need_of(tb);
  P.l_qpl = (lanes == 1 && P.out_stride == 1 && aligned16(P.qx) && aligned16(P.qy) && aligned16(P.out)) ? Wide<T>::N : 1;
  P.f_grid = resident_grid(nq, (uint64_t)P.f_tb * (lanes == 1 ? (uint64_t)P.l_qpl : 1), P.f_lds, P.f_tb);
  P.l_check = h.range_prepass(s, sc, {P.qx, P.qy}, nq, fresh);
  return true;
}

template <class T>
static void launch_lanes2(Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const Plan2<T>& P) {
  const uint64_t lanes = h.lanes;
  EvalLanes2Args<T> F{};
  F.xk = h.px.view.lv0; F.yk = h.py.view.lv0;
  F.nx = (uint32_t)h.nx; F.ny = (uint32_t)h.ny;
  F.dx = h.px.dlut; F.dy = h.py.dlut;
  F.data = h.data.template as<T>();
  batch_args(F, h, st, P);
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] lanes2d L=%llu qpl=%d maxk=%u,%u tb=%u grid=%u lds=%zu prepass=%d\n", (unsigned long long)lanes,
                 P.l_qpl, h.px.dlut.maxk, h.py.dlut.maxk, P.f_tb, P.f_grid, P.f_lds, P.l_check ? 0 : 1);
  constexpr int VNl = Wide<T>::N;
  pick_or<256, 1024>((int)P.f_tb, [&](auto tb_) {
    constexpr int TB = tb_;
    if (lanes == 1)
      pick_or<1, VNl>(P.l_qpl, [&](auto qpl_) {
        launch_lds<T>(eval_scalar2d_kernel<T, qpl_, TB>, FUSED_LDS_LIMIT, s, PC_EVAL, dim3(P.f_grid), dim3(P.f_tb), P.f_lds, F);
      });
    else launch_lds<T>(eval_lanes2d_kernel<T, TB>, FUSED_LDS_LIMIT, s, PC_EVAL, dim3(P.f_grid), dim3(P.f_tb), P.f_lds, F);
  });
}

// Short rows (up to 64 bytes) on a grid that does not fit LDS, large batches: slope records {z, m} -- one contiguous
// run of 4 L values per query, one division per value instead of three, an item per lane (eval_slopes2d_kernel; the
// copy, 2 x the grid, is built on first use -- ensure_slopes, the last condition).  NDI_SLOPES2D_KERNEL=0 / 1: A/B.
template <class T>
static bool plan_slopes2(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, Plan2<T>& P, int path, bool fresh) {
  static const Knob on_knob{"NDI_SLOPES2D_KERNEL", -1, Knob::live};
  const int on = on_knob.get();
  const uint64_t nx = h.nx, ny = h.ny, lanes = h.lanes, nq = P.nq;
  const size_t cell_b = (size_t)lanes * sizeof(T);
  // (f32 rows beyond 48 bytes: 13 .. 16 trips -- the compiler stops unrolling and the per-trip arrays go to scratch; the
  //  query-order kernel was level there anyway)
  if (!(on != 0 && path != NDI_PATH_BUCKETED && lanes >= 1 && cell_b <= (sizeof(T) == 4 ? 48 : 64) && nx <= 16384 && ny <= 16384 &&
        (uint64_t)h.slopes_bytes() < (1ull << 32) && h.slopes_bytes() <= h.SLOPES_LIMIT &&
        // AUTO: measured ahead of (f64 x 8, f32 x 16: level with) the query-order kernel on every row of up to 64 bytes
        // (profiles/r06_slopes2d_rates.txt); batches large enough to pay for building the copy; 1-2 values per point:
        // the one-thread-per-query kernel keeps the smaller batches, as before
        (on > 0 || (nq >= (lanes <= 2 ? 524288u : 65536u) && (double)nq * (double)cell_b >= 2.0 * (double)h.slopes_bytes()))))
    return false;
  h.px.ensure_dense_lut();
  h.py.ensure_dense_lut();
  const unsigned tb = 256u;
  size_t need = dense_axes_lds_bytes(h) + (size_t)(ny - 1) * 4 * sizeof(T) + (size_t)(tb / 64) * 2 * 64 * (4 + 4 * sizeof(T));
  const size_t res_strip = (size_t)(tb / 64) * 64 * lanes * sizeof(T);      // the rows of a batch, for 16-byte stores
  const bool wide_fits = need + res_strip <= FUSED_LDS_LIMIT;
  if (wide_fits) need += res_strip;
  if (!(h.px.dense_ok && h.py.dense_ok && need <= FUSED_LDS_LIMIT && h.ensure_slopes(s))) return false;
  P.kind = Plan2<T>::SLOPES2;
  P.f_tb = tb;
  P.f_lds = need;
  P.f_lds_wide = wide_fits;
  P.f_grid = resident_grid(nq, P.f_tb, P.f_lds, P.f_tb);
  P.l_check = h.range_prepass(s, sc, {P.qx, P.qy}, nq, fresh);
  return true;
}

template <class T>
static void launch_slopes2(Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const Plan2<T>& P) {
  const uint64_t lanes = h.lanes;
  EvalSlopes2Args<T> F{};
  F.xk = h.px.view.lv0; F.yk = h.py.view.lv0;
  F.nx = (uint32_t)h.nx; F.ny = (uint32_t)h.ny;
  F.dx = h.px.dlut; F.dy = h.py.dlut;
  F.recs = h.slopes.template as<T>();
#ifdef NDI_TUNING
  F.debug = env_int("NDI_SLOPES2D_DEBUG", 0);
#endif
  const size_t col_bytes = h.slopes_cells() ? h.slopes_cell_stride_bytes() : 2 * lanes * sizeof(T);   // cell or point records
  F.col_bytes = (uint32_t)col_bytes;
  F.row_bytes = (uint32_t)((h.slopes_cells() ? h.ny - 1 : h.ny) * col_bytes);
  batch_args(F, h, st, P);
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] slopes2d L=%llu recs=%s tb=%u grid=%u lds=%zu prepass=%d\n", (unsigned long long)lanes,
                 h.slopes_cells() ? "cell" : "point", P.f_tb, P.f_grid, P.f_lds, P.l_check ? 0 : 1);
  // rows leave as 16-byte vectors through a wave-private strip when the buffer allows it (+2-6 % over one value per lane)
  const int contig = P.out_stride != lanes ? 0 : (aligned16(P.out) && P.f_lds_wide) ? 2 : 1;
  const int mk = (int)std::max(h.px.dlut.lut ? h.px.dlut.maxk : 0u, h.py.dlut.lut ? h.py.dlut.maxk : 0u) <= 4 ? 4 : 8;
  auto launch = [&](auto lc_) {
    constexpr int LCS = lc_;
    pick_or<8, 4>(mk, [&](auto mk_) {
      constexpr int MKS = mk_;
      pick_or<1, 2, 0>(contig, [&](auto ct_) {
        launch_lds<T>(eval_slopes2d_kernel<T, LCS, MKS, ct_, 256>, FUSED_LDS_LIMIT, s, PC_EVAL, dim3(P.f_grid), dim3(256), P.f_lds, F);
      });
    });
  };
  // (plan_slopes2 plans rows of up to 64 bytes, f32 of up to 48: lanes 9 .. 12 exist for 4-byte elements only)
  bool known = pick<1, 2, 3, 4, 5, 6, 7, 8>((int)lanes, launch);
  if constexpr (sizeof(T) == 4) known = known || pick<9, 10, 11, 12>((int)lanes, launch);
  if (!known) throw HipFailure{hipErrorInvalidValue, "launch_slopes2: no slope-record kernel for this lane count", __LINE__};
}

// 1-2 values per grid point: one query per thread -- both searches and the evaluation in one launch, no (xi, yi)
// round trip, two reciprocals per query instead of three divisions per value.  (Extended to unaligned rows of more
// values in A/B runs, since removed: measured SLOWER from 3 values -- 100 x 100 x 5 f64: 11 vs
// 21 Gqueries/s -- a thread per query turns every operand load into 64 scattered sectors, where the item-per-lane
// gather kernel reads each query's 40-byte segments whole.)
template <class T>
static bool plan_small2(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, Plan2<T>& P, int path) {
  const bool small2d = h.lanes <= 2;
  const bool small2d_yields = h.lanes >= 1 && P.nq >= 8 * 65536;   // (to the query-order kernel, at 8 x its own floor)
  if (!(small2d && !small2d_yields && h.small_shmem() <= LDS_STAGE_LIMIT && path != NDI_PATH_BUCKETED)) return false;
  // short trailing axes: range pre-check, then both searches + evaluation fused in one launch
  P.kind = Plan2<T>::SMALL;
  h.range_prepass(s, sc, {P.qx, P.qy}, P.nq, false);
  return true;
}

// The arguments of eval_small2d_kernel but the staged bucket indices and the shared-divisor switch: for the SMALL plan
// (pre-checked, the caller's row pitch) and for the small-row paths of the engine (Interp2DImpl::launch_small: packed rows,
// the kernel's own range test).
template <class T>
static EvalSmall2Args<T> small2_args(const Interp2DImpl<T>& h, StatusBlock* st, const T* qx, const T* qy, T* out, uint64_t nq,
                                     uint64_t out_stride, int prechecked) {
  EvalSmall2Args<T> S{};
  S.px = h.px.view; S.py = h.py.view;
  S.data = h.data.template as<T>();
  S.qx = qx; S.qy = qy; S.out = out;
  S.nq = nq; S.out_stride = out_stride;
  S.row_cells = h.layout().row_cells; S.cell_elems = h.layout().cell_elems;
  S.lanes = (uint32_t)h.lanes; S.mode = h.mode;
  S.first_fail = &st->first_fail[0];
  S.prechecked = prechecked;
  return S;
}

template <class T>
static void launch_small2(Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const Plan2<T>& P) {
  const uint64_t nq = P.nq;
  const size_t both = h.small_shmem();
  const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + BLOCK - 1) / BLOCK, 4096));
  allow_dynamic_lds(reinterpret_cast<const void*>(&eval_small2d_kernel<T>), (int)LDS_STAGE_LIMIT);
  EvalSmall2Args<T> S = small2_args(h, st, P.qx, P.qy, P.out, nq, P.out_stride, 1);
  // large batches: bucket indices behind the pyramids (as the two-axis search stages them), and from two values per
  // query the shared-divisor division (two reciprocals per query instead of three divisions per value: same bits)
  const size_t lut = nq >= 4096 ? staged_index_bytes(h, LDS_STAGE_LIMIT / 2) : 0;   // (the bucket index: A/B settled in round 3)
  if (lut) { S.bx = h.px.bidx; S.by = h.py.bidx; }
  const size_t shm = both + lut;
  S.sdiv = h.lanes >= 2 ? 1 : 0;
  unsigned gs = g;
  if (shm > both)   // staging is the fixed cost of a workgroup: no more workgroups than the chip holds at once
    gs = (unsigned)std::min<uint64_t>(g, (uint64_t)cu_count() * std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / shm)));
  launch1<T>(s, PC_EVAL, dim3(gs), dim3(BLOCK), shm, eval_small2d_kernel<T>, S);
}

// Rows of fewer than 256 vectors on axes that fit LDS twice over (the reference's 100 x 100 x 5; few-channel grids),
// batches from 65 536 queries: query order with both searches fused in (eval_fused2d_kernel) -- no (xi, yi)
// round trip, one reciprocal per direction and query.  Grids the tile order takes are left to it.
template <class T>
static bool plan_fused2(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, Plan2<T>& P, int path, bool fresh) {
  constexpr int VNf = Wide<T>::N;
  const uint64_t lanes = h.lanes, nq = P.nq;
  const size_t both = h.small_shmem();
  const bool vec = (lanes % VNf == 0) && (P.out_stride % VNf == 0) && aligned16(P.out);
  const uint64_t LVf = vec ? lanes / VNf : lanes;
  const uint64_t grid_vecs = h.nx * h.layout().row_cells * h.layout().cell_elems / (vec ? VNf : 1);
  // workgroup size and search: the combination that keeps most waves on a CU beside the staged axes (the gathers
  // are latency-bound: waves first); the bucket indices when they cost no waves, or at most half of them
  const size_t lut_b = nq >= 4096 && both <= LDS_STAGE_LIMIT ? staged_index_bytes(h, LDS_STAGE_LIMIT) : 0;
  auto plan = [&](bool with_lut, unsigned& tb_out, size_t& lds_out) -> size_t {
    size_t best = 0;
    for (unsigned tb : {256u, 512u, 1024u}) {
      const size_t need = both + (with_lut ? lut_b : 0) + (size_t)(tb / 64) * 64 * (sizeof(uint32_t) + 6 * sizeof(T));
      if (need > LDS_STAGE_LIMIT) continue;
      const size_t waves = wgs_per_cu(need, tb) * (tb / 64);
      if (waves > best) { best = waves; tb_out = tb; lds_out = need; }
    }
    return best;
  };
  unsigned tb0 = 256, tb1 = 256;
  size_t lds0 = 0, lds1 = 0;
  const size_t w0 = plan(false, tb0, lds0);
  const size_t w1 = lut_b ? plan(true, tb1, lds1) : 0;
  const bool lut = w1 != 0 && 2 * w1 >= w0;
  const unsigned TBf = lut ? tb1 : tb0;
  const size_t lds = lut ? lds1 : lds0;
  const bool tile_candidate = path == NDI_PATH_BUCKETED || (path == NDI_PATH_AUTO && h.auto_tiles(nq) && lanes * sizeof(T) >= 64);
  if (!(nq >= 65536 && lanes >= 1 && LVf < 256 && 64 * LVf * LVf < (1ull << 32) && grid_vecs < (1ull << 32) && (lut ? w1 : w0) != 0 &&
        !tile_candidate))
    return false;
  P.kind = Plan2<T>::FUSED2;
  P.f_vec = vec; P.f_lv = LVf; P.f_lut = lut; P.f_lds = lds; P.f_tb = TBf;
  P.f_grid = resident_grid(nq, TBf, lds, TBf, 4);
  P.l_check = h.range_prepass(s, sc, {P.qx, P.qy}, nq, fresh);
  return true;
}

template <class T>
static void launch_fused2(Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const Plan2<T>& P) {
  EvalFused2Args<T> F{};
  F.px = h.px.view; F.py = h.py.view;
  F.bx = P.f_lut ? h.px.bidx : BucketIndex<T>{nullptr, 0, T(0)};
  F.by = P.f_lut ? h.py.bidx : BucketIndex<T>{nullptr, 0, T(0)};
  F.data = h.data.template as<T>();
  batch_args(F, h, st, P);
  F.lv = (uint32_t)P.f_lv;
  F.lv_magic = F.lv >= 2 ? (uint32_t)(((1ull << 32) + F.lv - 1) / F.lv) : 0u;
  const uint64_t vec = P.f_vec ? Wide<T>::N : 1;
  F.cell_vecs = (uint32_t)(h.layout().cell_elems / vec);
  F.row_vecs = (uint32_t)(h.layout().row_cells * h.layout().cell_elems / vec);
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] fused2d vec=%d lv=%u lut=%d tb=%u grid=%u lds=%zu prepass=%d\n", (int)P.f_vec, F.lv, (int)P.f_lut,
                 P.f_tb, P.f_grid, P.f_lds, P.l_check ? 0 : 1);
  constexpr int VNf = Wide<T>::N;
  pick_or<1, VNf>(P.f_vec ? VNf : 1, [&](auto vec_) {
    constexpr int VEC = vec_;
    pick_or<256, 1024, 512>((int)P.f_tb, [&](auto tb_) {
      launch_lds<T>(eval_fused2d_kernel<T, VEC, 2, tb_>, LDS_STAGE_LIMIT, s, PC_EVAL, dim3(P.f_grid), dim3(tb_), P.f_lds, F);
    });
  });
}

// BUCKETED for 2-D = tile grouping: the queries are ordered by the tile of 2^ts x 2^ts cells they fall in and
// eval_bilinear_tiles_kernel evaluates tile by tile out of LDS, so every grid value is read from memory once
// per tile instead of four times per query.  It pays when a tile sees several queries per cell (C3: 2.4) and
// cannot when the batch touches less data than the tiles hold (C5's share: 0.19 queries per cell): AUTO
// decides by queries per cell (Interp2DImpl::auto_tiles).  Needs vector rows whose length divides the workgroup, the plain
// grid layout, a tile that fits LDS and a tile histogram that fits next to the pyramids in locate2_kernel.
struct TilePlan {
  bool tiled = false;
  uint32_t ts = 0, nty = 0, nb = 0, ntx = 0;   // tile shift, tiles per grid row, tiles, tile rows
  bool compact = false;      // self-contained 16-byte records (f32)
  bool cell_words = false;   // the search writes one cell word per query: all the scatter needs
  bool two_level = false;    // grouping by tile row, then by tile
};

// The largest tile that leaves room for two workgroups per CU, else the largest that fits at all; false: no tile order.
// `axes_lds`: the pyramids and the staged bucket indices of locate2_kernel, which keeps the tile histogram behind them.
template <class T>
static bool tile_shape(const Interp2DImpl<T>& h, const Plan2<T>& P, size_t axes_lds, TilePlan& TP) {
  constexpr int VNp = Wide<T>::N;
  const uint64_t nx = h.nx, ny = h.ny, lanes = h.lanes;
  const bool vec_ok_p = (lanes % VNp == 0) && (P.out_stride % VNp == 0) && aligned16(P.out);
  const uint64_t LVp = vec_ok_p ? lanes / VNp : 0;
  if (!(vec_ok_p && !h.pair_packed && LVp >= 1 && LVp <= 1024 && 1024 % LVp == 0 && h.small_shmem() <= LDS_STAGE_LIMIT &&
        nx < (1ull << 31) && ny < (1ull << 31) && ny * lanes < (1ull << 32) && P.out_stride < (1ull << 32)))
    return false;
  auto ntiles_of = [&](uint64_t pts, uint32_t sh) { return (uint32_t)(((pts - 1) + ((uint64_t)1 << sh) - 1) >> sh); };
  static const Knob ts_knob{"NDI_TILE_TS", -1};
  const int ts_env = ts_knob.get();
  // the tile must fit the kernel's register double-buffer (6 x 1024 16-byte vectors = 96 KiB) next to 24-32 KiB of
  // static LDS; the smaller budget is tried first (shorter staging per tile)
  for (size_t budget : {(size_t)76 * 1024, (size_t)96 * 1024})
    for (int sh = 6; sh >= 1; --sh) {
      if (ts_env >= 0 && sh != ts_env) continue;
      const uint64_t bins = (uint64_t)ntiles_of(nx, sh) * ntiles_of(ny, sh);
      if (tile_lds_bytes<T>(sh, lanes, TILE_VALUES) <= budget && bins <= GROUP_MAX_BINS &&
          ((axes_lds + 15) & ~(size_t)15) + (size_t)bins * 4 <= LDS_STAGE_LIMIT) {
        TP.ts = (uint32_t)sh;
        TP.nty = ntiles_of(ny, sh);
        TP.nb = (uint32_t)bins;
        return true;
      }
    }
  return false;
}

// Tile order or query order for this batch, and how the tile order groups.
//
// `compact` is fixed by the element type: a tile order needs both pyramids in LDS_STAGE_LIMIT (150 KiB: fewer than 38 400
// f32 knots on both axes together), far inside the 65 536 knots per axis a compact record can address -- every tiled f32 batch
// has compact records, no f64 batch has.  The non-compact f32 instances of the scatter and tile kernels are therefore never
// launched (they stay compiled: dropping them changes the kernel set); a plan that asked for one is refused here.
template <class T>
static TilePlan plan_tiles(const Interp2DImpl<T>& h, const Plan2<T>& P, int path, size_t axes_lds) {
  TilePlan TP;
  const uint64_t nq = P.nq;
  const size_t both = h.small_shmem();
  const bool can_tile = tile_shape(h, P, axes_lds, TP) && nq >= 2 && nq < 0xffffffffull;
  if (path == NDI_PATH_BUCKETED) TP.tiled = can_tile;
  else if (path == NDI_PATH_AUTO) TP.tiled = can_tile && h.auto_tiles(nq);
  TP.compact = std::is_same<T, float>::value && h.nx <= 65536 && h.ny <= 65536;
  if (TP.tiled && std::is_same<T, float>::value && !TP.compact)
    throw HipFailure{hipErrorInvalidValue, "plan_tiles: an f32 tile order without compact records", __LINE__};
  static const Knob cw_knob{"NDI_TILE_CELLWORDS", 1};   // A/B
  TP.cell_words = TP.tiled && TP.compact && both <= LDS_STAGE_LIMIT && cw_knob.get();
  // Two-level grouping (tile row, then tile: coarse_scatter2d_kernel / fine_scatter2d_kernel) when the one-pass scatter
  // would leave fewer than a line's worth of records per (slice, tile) and the batch is large enough to pay for the
  // second pass.  NDI_GROUP_TWO_LEVEL=0 / 1: A/B.
  static const Knob tl_knob{"NDI_GROUP_TWO_LEVEL", -1, Knob::live};
  const int tl_env = tl_knob.get();
  TP.ntx = TP.tiled ? TP.nb / TP.nty : 0;
  TP.two_level = TP.tiled && both <= LDS_STAGE_LIMIT && TP.ntx >= 2 && TP.ntx <= 4096 && TP.nty <= 4096 &&
                 (tl_env == 1 || (tl_env < 0 && nq >= (1u << 20) && (double)nq / group_blocks() / TP.nb < 8.0));
  return TP;
}

struct Slices { uint64_t slice = 0, blocks = 0; };   // queries per slice of the batch, slices (= workgroups of the search)

// Both axes in one launch (locate2_kernel: the pyramids, the bucket indices when `axes_lds` has room for them, and for the
// tile order the tile histograms of every slice).
template <class T>
static Slices locate2(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan2<T>& P, const TilePlan& TP, size_t axes_lds,
                      bool beside_eval) {
  const uint64_t nq = P.nq;
  StatusBlock* st = sc.status.as<StatusBlock>();
  Locate2Args<T> LA{};
  LA.px = h.px.view; LA.py = h.py.view;
  LA.qx = P.qx; LA.qy = P.qy; LA.nq = nq;
  LA.xi = sc.idx.as<uint32_t>(); LA.yi = sc.idx2.as<uint32_t>();
  if (TP.cell_words) LA.yi = nullptr;   // one cell word per query: all the scatter needs
  LA.first_fail = &st->first_fail[0];
  LA.mode = h.mode;
  LA.bx = BucketIndex<T>{nullptr, 0, T(0)};
  LA.by = LA.bx;
  if (axes_lds != h.small_shmem()) {
    LA.bx = h.px.bidx;      // [x pyramid | y pyramid | x lut | y lut]; an axis whose formula guess is exact has none
    LA.by = h.py.bidx;
  }
  size_t shmem = axes_lds;
  if (TP.tiled) {
    sc.hist.reserve((size_t)std::max<uint32_t>(group_blocks(), GROUP_MAX_BLOCKS) * TP.nb * sizeof(uint32_t));
    LA.hist = sc.hist.as<uint32_t>();
    LA.nb = TP.nb; LA.sx = TP.ts; LA.sy = TP.ts; LA.nty = TP.nty;
    shmem = ((axes_lds + 15) & ~(size_t)15) + (size_t)TP.nb * 4;
    if (TP.two_level) {
      sc.chist.reserve((size_t)std::max<uint32_t>(group_blocks(), GROUP_MAX_BLOCKS) * TP.ntx * sizeof(uint32_t));
      LA.chist = sc.chist.as<uint32_t>();
      LA.ntx = TP.ntx;
    }
  }
  const unsigned threads = beside_eval ? 256u : threads_for_lds(shmem);
  Slices sl;
  sl.blocks = std::max<uint64_t>(1, std::min<uint64_t>((nq + 1023) / 1024, TP.tiled ? group_blocks() : 2048));
  if ((LA.bx.lut || LA.by.lut || TP.tiled) && !(TP.tiled && group_blocks() > GROUP_MAX_BLOCKS))   // staging is the fixed cost of a
    // workgroup: no more workgroups than the chip holds at once (NDI_GROUP_BLOCKS > 256 lifts the cap: A/B)
    sl.blocks = std::min<uint64_t>(sl.blocks, (uint64_t)cu_count() * std::max<size_t>(1, (160 * 1024) / shmem));
  sl.slice = (nq + sl.blocks - 1) / sl.blocks;
  sl.slice = (sl.slice + threads - 1) / threads * threads;
  sl.blocks = (nq + sl.slice - 1) / sl.slice;
  LA.slice = sl.slice;
  if (TP.two_level) {   // column-block-major tile histograms: (blocks * hist_w) words per block, ceil(nb / hist_w) <= blocks blocks
    LA.hist_w = (uint32_t)((TP.nb + sl.blocks - 1) / sl.blocks);
    sc.hist.reserve((size_t)sl.blocks * LA.hist_w * sl.blocks * sizeof(uint32_t));
    LA.hist = sc.hist.as<uint32_t>();
  }
  pick_or<1, LOCATE_QB>(sl.slice / threads >= 16 ? LOCATE_QB : 1, [&](auto qb_) {
    launch_lds<T>(locate2_kernel<T, qb_>, LDS_STAGE_LIMIT, s, PC_LOCATE, dim3((unsigned)sl.blocks), dim3(threads), shmem, LA);
  });
  return sl;
}

// One pass: slice offsets, the scan of the tile totals and the tile each evaluation chunk starts in (one launch), then the
// scatter into tile order.
template <class T>
static void group_one_pass(hipStream_t s, Scratch& sc, const Plan2<T>& P, const TilePlan& TP, Slices sl, unsigned gthreads,
                           uint32_t chunk) {
  StatusBlock* st = sc.status.as<StatusBlock>();
  hipLaunchKernelGGL(group_offsets_scan_kernel, dim3((TP.nb + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s,
                     sc.hist.as<uint32_t>(), (uint32_t)sl.blocks, TP.nb, sc.counts.as<uint32_t>(),
                     sc.cursor.as<uint32_t>(), st, P.nq, chunk, sc.chunkbin.as<uint32_t>());
  const uint32_t* yi_in = TP.cell_words ? (const uint32_t*)nullptr : (const uint32_t*)sc.idx2.as<uint32_t>();
  pick_bool(P.compact, [&](auto cp_) {
    constexpr bool CP = cp_;
    hipLaunchKernelGGL((group_scatter2d_kernel<T, CP>), dim3((unsigned)sl.blocks), dim3(gthreads), (size_t)TP.nb * 4, s,
                       (const uint32_t*)sc.idx.as<uint32_t>(), yi_in, P.qx, P.qy, P.nq,
                       sl.slice, (const uint32_t*)sc.hist.as<uint32_t>(), (const uint32_t*)sc.cursor.as<uint32_t>(),
                       TP.nb, TP.ts, TP.ts, TP.nty, sc.perm.as<uint4>(), CP ? (T*)nullptr : sc.recq.as<T>());
  });
}

// Two levels: the coarse scatter by tile row (the trips sorted in LDS, or direct), the scan of the tile totals, the fine
// scatter by tile within each row (the round's records sorted in LDS, or direct).
template <class T>
static void group_two_levels(hipStream_t s, Scratch& sc, const Plan2<T>& P, const TilePlan& TP, Slices sl, unsigned gthreads,
                             uint32_t chunk) {
  StatusBlock* st = sc.status.as<StatusBlock>();
  const uint64_t nq = P.nq, blocks = sl.blocks;
  const uint32_t ntx = TP.ntx, nty = TP.nty, nb = TP.nb;
  sc.perm2.reserve(nq * sizeof(uint4));
  if (!P.compact) sc.recq2.reserve(nq * 2 * sizeof(T));
  sc.cursor2.reserve(((size_t)nb + 4) * sizeof(uint32_t));
  const size_t shm_c = ((size_t)3 * ntx + (size_t)2 * gthreads) * 4;
  static const Knob ft_knob{"NDI_GROUP_FINE_THREADS", 0};
  const int ft_env = ft_knob.get();
  constexpr int FR = 4;   // records per thread and round of the fine pass (2 / 8 measured level: r05_c3_fine_round_variants.txt)
  const unsigned fthreads = (ft_env == 256 || ft_env == 512 || ft_env == 1024) ? (unsigned)ft_env : 1024u;
  // parts per tile row: one round per workgroup on evenly spread queries (measured at C3, profiles/r05_tuning.md:
  // 2560 one-round workgroups 78 us; 512 workgroups walking five rounds each with the next round's records in
  // flight 115 us -- the pass wants its parallelism across workgroups)
  const uint64_t per_row = (nq + ntx - 1) / ntx;
  const uint64_t rounds_row = (per_row + (uint64_t)FR * fthreads - 1) / ((uint64_t)FR * fthreads);
  const uint32_t G = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(rounds_row, 4096));
  const unsigned fgrid = (unsigned)(((ntx + 7u) / 8u) * 8u * G);
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] two-level grouping ntx=%u nty=%u slices=%llu G=%u\n", ntx, nty,
                 (unsigned long long)blocks, G);
  const uint32_t* yi_c = TP.cell_words ? (const uint32_t*)nullptr : (const uint32_t*)sc.idx2.as<uint32_t>();
  T* rq2 = P.compact ? (T*)nullptr : sc.recq2.as<T>();
  T* rq1 = P.compact ? (T*)nullptr : sc.recq.as<T>();
  auto coarse = [&](auto kern, size_t limit, size_t shm) {
    allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)limit);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(gthreads), shm, s,
                       (const uint32_t*)sc.idx.as<uint32_t>(), yi_c, P.qx, P.qy, nq, sl.slice,
                       (const uint32_t*)sc.chist.as<uint32_t>(), (const uint32_t*)sc.hist.as<uint32_t>(), nb, ntx,
                       TP.ts, sc.perm2.as<uint4>(), rq2, sc.counts.as<uint32_t>());
  };
  static const Knob csort_knob{"NDI_GROUP_COARSE_SORT", 1};
  const size_t shm_cs = ((((size_t)6 * ntx + 2 * gthreads) * 4 + 15) & ~(size_t)15) + (size_t)4 * gthreads * 20;
  // trips sorted in LDS (NDI_GROUP_COARSE_SORT=0: direct, A/B)
  if (P.compact && std::is_same<T, float>::value && csort_knob.get() && shm_cs <= 150 * 1024) coarse(coarse_scatter2d_kernel<T, true, true>, 150 * 1024, shm_cs);
  else if (P.compact) coarse(coarse_scatter2d_kernel<T, true>, 64 * 1024, shm_c);
  else coarse(coarse_scatter2d_kernel<T, false>, 64 * 1024, shm_c);
  hipLaunchKernelGGL(scan_bin_totals_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)sc.counts.as<uint32_t>(), nb,
                     sc.cursor.as<uint32_t>(), sc.cursor2.as<uint32_t>(), st, chunk, sc.chunkbin.as<uint32_t>());
  static const Knob fsort_knob{"NDI_GROUP_FINE_SORT", 1};
  const int fsort_env = fsort_knob.get();
  if (P.compact && std::is_same<T, float>::value && fsort_env) {   // the round's records sorted in LDS, coalesced copy-out (NDI_GROUP_FINE_SORT=0: the direct form, A/B)
    // records per thread and round x workgroup size: 1 = 4 x 512; 2 .. 5 = 8 x 512, 4 x 1024, 2 x 512, 4 x 256 (A/B)
    pick_or<1, 2, 3, 4, 5>(fsort_env, [&](auto v_) {
      constexpr int V = v_, SR = V == 2 ? 8 : (V == 4 ? 2 : 4), STB = V == 3 ? 1024 : (V == 5 ? 256 : 512);
      const uint64_t rr = (per_row + (uint64_t)SR * STB - 1) / ((uint64_t)SR * STB);
      const uint32_t Gs = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(rr, 4096));
      const unsigned sgrid = (unsigned)(((ntx + 7u) / 8u) * 8u * Gs);
      const size_t shm_s = ((((size_t)3 * nty + 16) * 4 + 15) & ~(size_t)15) + (size_t)SR * STB * 20;
      auto kern = fine_scatter2d_sorted_kernel<SR, STB>;
      allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)(128 * 1024));
      hipLaunchKernelGGL(kern, dim3(sgrid), dim3(STB), shm_s, s, (const uint4*)sc.perm2.as<uint4>(), sc.perm.as<uint4>(),
                         (const uint32_t*)sc.cursor.as<uint32_t>(), sc.cursor2.as<uint32_t>(), nq, ntx, nty, TP.ts, Gs);
    });
  } else
    pick_bool(P.compact, [&](auto cp_) {
      hipLaunchKernelGGL((fine_scatter2d_kernel<T, cp_, FR>), dim3(fgrid), dim3(fthreads), (size_t)nty * 8, s,
                         (const uint4*)sc.perm2.as<uint4>(), (const T*)rq2, sc.perm.as<uint4>(), rq1,
                         (const uint32_t*)sc.cursor.as<uint32_t>(), sc.cursor2.as<uint32_t>(), nq, ntx, nty, TP.ts, G);
    });
}

// The tile order's plan and its grouping launches (PC_GROUP), after the search has left the histograms of `sl.blocks` slices.
template <class T>
static void group_tiles(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, Plan2<T>& P, const TilePlan& TP, Slices sl, bool beside_eval) {
  const uint64_t nq = P.nq;
  P.kind = Plan2<T>::TILED;
  P.ts = TP.ts; P.nty = TP.nty; P.nb = TP.nb;
  P.compact = TP.compact;
  // the scatter is a latency-bound chain (load -> LDS atomic -> scattered store): many waves per CU
  const unsigned gthreads = beside_eval ? 256u : (sl.slice >= 4096 ? 1024u : (unsigned)BLOCK);
  sc.perm.reserve(nq * sizeof(uint4));            // grouped records
  if (!P.compact) sc.recq.reserve(nq * 2 * sizeof(T));
  sc.counts.reserve(((size_t)TP.nb + 4) * sizeof(uint32_t));   // (+4: the fused scan reads / writes 16-byte pieces)
  sc.cursor.reserve(((size_t)TP.nb + 4) * sizeof(uint32_t));
  allow_dynamic_lds(reinterpret_cast<const void*>(&group_scatter2d_kernel<T, true>), (int)(GROUP_MAX_BINS * 4));
  allow_dynamic_lds(reinterpret_cast<const void*>(&group_scatter2d_kernel<T, false>), (int)(GROUP_MAX_BINS * 4));
  ProfScope ps(s, PC_GROUP);
  const uint32_t chunk = h.tile_chunk();
  sc.chunkbin.reserve(((nq + chunk - 1) / chunk) * sizeof(uint32_t));
  if (TP.two_level) group_two_levels(s, sc, P, TP, sl, gthreads, chunk);
  else group_one_pass(s, sc, P, TP, sl, gthreads, chunk);
  NDI_HIP(hipGetLastError());
  ps.done();
}

template <class T>
static Eval2Args<T> eval2_args(const Interp2DImpl<T>& h, Scratch& sc, const Plan2<T>& P) {
  Eval2Args<T> A{};
  A.xk = h.px.view.lv0; A.yk = h.py.view.lv0;
  A.data = h.data.template as<T>();
  A.qx = P.qx; A.qy = P.qy; A.out = P.out;
  A.xi = sc.idx.as<uint32_t>(); A.yi = sc.idx2.as<uint32_t>();
  A.nx = h.nx; A.ny = h.ny; A.lanes = h.lanes;
  A.nq = P.nq; A.out_stride = P.out_stride;
  A.row_cells = h.layout().row_cells; A.cell_elems = h.layout().cell_elems;
  A.status = sc.status.as<StatusBlock>();
  return A;   // (rec_i, rec_q: null -- the gather order has no grouped records)
}

// The forms of eval_bilinear_tiles_kernel: workgroup size, records per hand-over, vectors per thread of the staging double
// buffer, x slopes staged, and the LDS a workgroup may take (a half-tile workgroup shares its CU with a second one).
struct TileForm { int tb, rb, maxi; bool slope; int lds_kib; };
static constexpr TileForm TILE_FORMS[5] = {{512, 256, 5, true, 80}, {1024, 1024, 6, true, 160}, {1024, 256, 6, true, 160},
                                           {512, 256, 10, false, 160}, {1024, 1024, 6, false, 160}};
struct TileFormChoice { int form; size_t lds; unsigned ch_split; };

// The form a tiled plan runs in (an index into TILE_FORMS) and the tile's LDS bytes in that form.
template <class T>
static TileFormChoice tile_form(const Interp2DImpl<T>& h, const Plan2<T>& P) {
  constexpr int VNt = Wide<T>::N;
  const uint64_t lanes = h.lanes;
  const size_t s1 = ((size_t)1 << P.ts) + 1;
  // Channel split: two 512-thread workgroups per CU, each staging one half of the trailing axis of its tile (values +
  // x slopes), when two such half-tiles fit the CU's LDS beside 256 records each and a half-row still fills whole
  // 16-byte vectors.  NDI_TILE_SPLIT=0 keeps one 1024-thread workgroup per CU (A/B).
  static const Knob split_knob{"NDI_TILE_SPLIT", -1}, slope_knob{"NDI_TILE_SLOPES", 1}, wg_knob{"NDI_TILE_WG", 0};
  const int slope_env = slope_knob.get();
  const uint64_t lv_full = lanes / VNt;
  const size_t shm = tile_lds_bytes<T>(P.ts, lanes, TILE_VALUES), shm_slope = tile_lds_bytes<T>(P.ts, lanes, TILE_SLOPES),
               shm_half = tile_lds_bytes<T>(P.ts, lanes, TILE_HALF_SLOPES);
  const size_t static512 = tile_record_strip_bytes<T>(256, P.compact);   // 256 records beside a tile
  const bool split2 = split_knob.get() != 0 && slope_env != 0 && lv_full >= 2 && lv_full % 2 == 0 &&
                      s1 * s1 * (lv_full / 2) <= 5 * 512 && 512 % (lv_full / 2) == 0 &&
                      2 * (shm_half + static512) <= 160 * 1024;
  // (Four quarter-row workgroups per CU were measured slower -- 1.05-1.08 vs 0.77-0.85 ms at C3: 64-byte half-line stores,
  //  four decodes per record -- and are gone: profiles/r05_tuning.md 2.)
  // One 1024-thread workgroup per CU.  NDI_TILE_WG=512 (A/B only): two 512-thread workgroups per CU when two tiles
  // (+ 256 records each) fit the 160 KiB and the tile fits the 10 x 512-vector register double buffer -- measured
  // slower at C3 (1.54 vs 1.17 ms: twice the tile staging per CU, half the rows per trip).
  const size_t tile_vecs = s1 * s1 * lv_full;
  const bool two_wg = wg_knob.get() == 512 && tile_vecs <= 10 * 512 && 2 * (shm + static512) <= 160 * 1024 &&
                      lv_full <= 512 && 512 % lv_full == 0;
  // x slopes of the tile staged next to its values (one division per channel and query instead of three): needs a
  // second tile-sized array in LDS, so the records are handed over 256 at a time.  NDI_TILE_SLOPES=0: A/B.
  const bool slopes = slope_env != 0 && !two_wg && shm_slope + static512 <= 160 * 1024;
  // ... 1024 at a time when that still fits (compact f32 records at C3: 143.9 KiB + 16 KiB)
  const bool slopes_rb1024 = slopes && shm_slope + tile_record_strip_bytes<T>(1024, P.compact) <= 160 * 1024 && slope_env != 256;
  return {split2 ? 0 : (slopes_rb1024 ? 1 : (slopes ? 2 : (two_wg ? 3 : 4))), split2 ? shm_half : (slopes ? shm_slope : shm),
          split2 ? 2u : 1u};
}

template <class T>
static void launch_tiles(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan2<T>& P) {
  constexpr int VNt = Wide<T>::N;
  const uint64_t nq = P.nq;
  Eval2Args<T> A = eval2_args(h, sc, P);
  A.rec_i = sc.perm.as<uint4>();
  A.rec_q = P.compact ? nullptr : sc.recq.as<T>();
  A.bin_start = sc.cursor.as<uint32_t>();
  A.nb = P.nb; A.ts = P.ts; A.nty = P.nty;
  A.chunk = h.tile_chunk();
  A.chunk_bin = sc.chunkbin.as<uint32_t>();
  const TileFormChoice F = tile_form(h, P);
  A.ch_split = F.ch_split;
  {   // item -> (grid row, vector) of the tile staging: ceil(2^32 / vectors per tile row), full and last-column tiles
    const uint64_t lvv = h.lanes / VNt / A.ch_split;
    const uint64_t full = (((uint64_t)1 << P.ts) + 1) * lvv;
    const uint64_t edge = (h.ny - ((uint64_t)(P.nty - 1) << P.ts)) * lvv;
    A.rvm_full = (uint32_t)((((uint64_t)1 << 32) + full - 1) / full);
    A.rvm_edge = (uint32_t)((((uint64_t)1 << 32) + edge - 1) / edge);
  }
  A.debug = 0;
#ifdef NDI_TUNING
  A.debug = env_int("NDI_FUSED_DEBUG", 0);
#endif
  const uint64_t nchunks = (nq + A.chunk - 1) / A.chunk;
  const uint64_t resident = (uint64_t)cu_count() * std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (tile_lds_bytes<T>(P.ts, h.lanes, TILE_VALUES) + 64)));
  const unsigned gmul = 8u * A.ch_split;   // XCD-aware chunk order; the halves of a chunk are neighbours on one XCD
  const unsigned gx = (unsigned)((std::max<uint64_t>(1, std::min<uint64_t>(nchunks * A.ch_split, resident * 4 * A.ch_split)) + gmul - 1) / gmul * gmul);
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] tiles ts=%u split=%u compact=%d grid=%u\n", P.ts, A.ch_split, (int)P.compact, gx);
  pick<0, 1, 2, 3, 4>(F.form, [&](auto f_) {
    constexpr TileForm V = TILE_FORMS[f_];
    auto launch = [&](auto cp_) {
      launch_lds<T>(eval_bilinear_tiles_kernel<T, VNt, V.tb, V.rb, V.maxi, cp_, V.slope>,
                    V.lds_kib * 1024 - V.rb * (16 + 2 * sizeof(T)) - 512, s, PC_EVAL, dim3(gx), dim3(V.tb), F.lds, A);
    };
    if constexpr (std::is_same<T, float>::value) {   // compact records exist for f32 only
      if (P.compact) return launch(std::true_type{});
    }
    launch(std::false_type{});
  });
}

// The gather order: the query-order kernel on the indices the search left.
template <class T>
static void launch_gather2(Interp2DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan2<T>& P) {
  constexpr int VN = Wide<T>::N;
  const uint64_t nq = P.nq, lanes = h.lanes;
  const Eval2Args<T> A = eval2_args(h, sc, P);
  const bool vec_ok = (lanes % VN == 0) && (P.out_stride % VN == 0) && aligned16(P.out);
  const uint64_t LV = vec_ok ? lanes / VN : lanes;
  // knots in LDS: both axes must fit next to each other with two 1024-thread workgroups per CU, and the batch
  // must be large enough to amortise the staging
  const size_t knot_bytes = (size_t)(h.nx + h.ny) * sizeof(T);
  const bool klds = vec_ok && knot_bytes <= 72 * 1024 && nq >= (1u << 20);
  ProfScope ps(s, PC_EVAL);
  const uint32_t tile_q = (uint32_t)std::max<uint64_t>(1, (klds ? 2048u : 1024u) / std::max<uint64_t>(LV, 1));
  const uint64_t ntiles = (nq + tile_q - 1) / tile_q;
  const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, klds ? 512 : 32768));
  if (klds) {
    constexpr int TB = 1024;
    // Short rows (the pair-packed layout, <= 64 bytes per grid point: C5) divide with the shared-divisor division
    // of kernels.hpp -- two IEEE reciprocals per item instead of twelve divisions: 1.5-6 % faster at C5's share
    // (A/B on two boxes: 0.773 -> 0.726 and 0.749 -> 0.736 ms; the measured ceiling of the access mix is
    // 0.72-0.74), neutral with index axes; long rows (C3, HBM-bound at 7.1 TB/s) get 3 % slower with it and keep
    // the IEEE divisions.  Same bits either way.
    pick_bool(h.pair_packed, [&](auto sdiv_) {
      auto kern = eval_bilinear_kernel<T, VN, false, 2, TB, true, sdiv_>;
      allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)LDS_STAGE_LIMIT);
      hipLaunchKernelGGL(kern, dim3(gx), dim3(TB), (knot_bytes + 15) & ~(size_t)15, s, A, tile_q);
    });
  } else {
    pick_or<1, VN>(vec_ok ? VN : 1, [&](auto vec_) {
      hipLaunchKernelGGL((eval_bilinear_kernel<T, vec_>), dim3(gx), dim3(BLOCK), 0, s, A, tile_q);
    });
  }
  NDI_HIP(hipGetLastError());
  ps.done();
}

template <class T>
Plan2<T> Interp2DImpl<T>::prep(hipStream_t s, Scratch& sc, Queries<T> q, uint64_t nq, T* out, uint64_t out_stride, int path,
                               bool beside_eval, int flags) {
  Plan P;
  P.qx = q.a; P.qy = q.b; P.nq = nq; P.out = out; P.out_stride = out_stride;
  sc.status.reserve(sizeof(StatusBlock));
  reset_status(sc.status.p, s);
  const bool fresh = (flags & NDI_EVAL_FRESH_OUTPUT) != 0;
  if (bicubic) {   // one kernel for AUTO and GATHER (eval_bicubic_kernel); BUCKETED was refused at the entry point
    P.kind = integral ? Plan::BICUBIC_INT : Plan::BICUBIC;   // (an integral handle: eval_bicubic_integral_kernel)
    P.l_check = this->range_prepass(s, sc, q, nq, fresh);
    return P;
  }
  sc.idx.reserve(nq * sizeof(uint32_t));
  sc.idx2.reserve(nq * sizeof(uint32_t));
  if (plan_lanes2(*this, s, sc, P, path, fresh)) return P;
  if (plan_slopes2(*this, s, sc, P, path, fresh)) return P;
  if (plan_small2(*this, s, sc, P, path)) return P;
  if (plan_fused2(*this, s, sc, P, path, fresh)) return P;
  // the search writes (xi, yi) for the gather order or, for the tile order, the histograms the grouping scatters by;
  // its LDS: both pyramids and, from 4096 queries, the bucket indices behind them (A/B settled in round 3)
  const size_t both = small_shmem();
  const size_t axes_lds = both + (nq >= 4096 && both <= LDS_STAGE_LIMIT ? staged_index_bytes(*this, LDS_STAGE_LIMIT) : 0);
  const TilePlan TP = plan_tiles(*this, P, path, axes_lds);
  g_last_path.store(TP.tiled ? NDI_PATH_BUCKETED : NDI_PATH_GATHER);
  if (both <= LDS_STAGE_LIMIT) {   // both axes in one launch
    const Slices sl = locate2(*this, s, sc, P, TP, axes_lds, beside_eval);
    if (TP.tiled) group_tiles(*this, s, sc, P, TP, sl, beside_eval);
  } else {   // (never tiled: a tile order needs both axes in LDS)
    StatusBlock* st = sc.status.as<StatusBlock>();
    run_locate<T>(s, px, q.a, nq, sc.idx.as<uint32_t>(), nullptr, nullptr, &st->first_fail[0], mode);
    run_locate<T>(s, py, q.b, nq, sc.idx2.as<uint32_t>(), nullptr, nullptr, &st->first_fail[1], mode);
  }
  return P;
}

template <class T>
void Interp2DImpl<T>::launch_eval(hipStream_t s, Scratch& sc, const Plan& P) {
  StatusBlock* st = sc.status.as<StatusBlock>();
  switch (P.kind) {
    case Plan::BICUBIC: return bicubic_launch_eval<T>(*this, s, st, P.qx, P.qy, P.nq, P.out, P.out_stride, P.l_check);
    case Plan::BICUBIC_INT:
      return bicubic_integral_launch_eval<T>(*this, s, st, P.qx, P.qy, (const T*)nullptr, (const T*)nullptr, P.nq, P.out,
                                             P.out_stride, P.l_check);
    case Plan::SMALL: return launch_small2(*this, s, st, P);
    case Plan::SLOPES2: return launch_slopes2(*this, s, st, P);
    case Plan::LANES2: return launch_lanes2(*this, s, st, P);
    case Plan::FUSED2: return launch_fused2(*this, s, st, P);
    case Plan::TILED: return launch_tiles(*this, s, sc, P);
    case Plan::GATHER: return launch_gather2(*this, s, sc, P);
  }
}
