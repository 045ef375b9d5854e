// csrc/interp1d_host.hpp -- the evaluation host of the 1-D float handles (included by ndinterp_api.hip after Interp1DImpl): one
// planner and one launcher per plan, free templates over the handle.  Interp1DImpl::prep is the cascade over plan_lanes1,
// plan_small1 and plan_fused1, then the grouping decision (grouping1), the search (run_locate) and the grouping
// (group_one_pass1 / group_atomics1); launch_eval the switch over the launchers.  A planner that accepts enqueues the range
// pre-pass as its last step, and asks for a lazy device table (ensure_dense_lut, ensure_bucket_index, ensure_bucket_index32,
// ensure_packed) only after its cheap conditions have passed: when a table is built, and on which stream, is something a
// caller can observe (tests/test_gpu_lazy_tables.py).
#pragma once

// The table pointers every Args struct of the 1-D kernels takes: the knots -- level 0 of the pyramid, or the whole pyramid
// for the kernels that stage it -- the data and the a / b tables.
template <class A, class = void>
struct takes_knots : std::false_type {};
template <class A>
struct takes_knots<A, std::void_t<decltype(std::declval<A&>().knots)>> : std::true_type {};
template <class A, class T>
static void table_args(A& F, const Interp1DImpl<T>& h) {
  if constexpr (takes_knots<A>::value) F.knots = h.pyr.view.lv0;
  else F.pyr = h.pyr.view;
  F.data = h.data.template as<T>();
  F.ca = h.ca.template as<T>();
  F.cb = h.cb.template as<T>();
}

// What the Args of the query-order kernels have alike: the batch, the row pitch, the mode, the status slot.
template <class A, class T>
static void batch_args(A& F, const Interp1DImpl<T>& h, StatusBlock* st, const T* q, T* out, uint64_t nq, uint64_t out_stride) {
  F.q = q;
  F.out = out;
  F.nq = nq;
  F.out_stride = out_stride;
  F.lanes = (uint32_t)h.lanes;
  F.mode = h.mode;
  F.first_fail = &st->first_fail[0];
}

// ---- LANES ---------------------------------------------------------------------------------------------------------------
// Query per lane with the whole table set in LDS (eval_scalar_kernel / eval_lanes_kernel): rows of up to 56 bytes
// whose records fit LDS beside the knots, an axis the branch-free search covers (dense bucket index
// or exact O(1) guess), batches that give every workgroup several times its staging bytes to write.
// NDI_LANES_KERNEL=0 leaves these shapes to the query-order kernel (A/B); =1 takes it whenever it fits.
template <class T>
static bool plan_lanes1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, Plan1<T>& P, int path, bool fresh) {
  const uint64_t n = h.n, lanes = h.lanes;
  // rows of up to 56 bytes: at 64 bytes the query-order kernel is level (f64 x 8: 65 vs 61-65 Gqueries/s) or ahead
  // (f32 x 16: 74 vs 57), profiles/r05_small_shapes_rates.txt
  static const Knob on_knob{"NDI_LANES_KERNEL", -1, Knob::live};
  const int on = on_knob.get();
  constexpr int maxb = 56;
  if (on == 0 || path == NDI_PATH_BUCKETED || n < 3 || n > 16384) return false;
  if (on < 0 && short_knobs().mode != 0) return false;   // a pinned short-row variant (NDI_SHORT_MODE) is what runs
  if (lanes * sizeof(T) > (size_t)(on > 0 ? std::max(maxb, 64) : maxb)) return false;   // (forced: up to 64 bytes, for the tests)
  const size_t tab = ((size_t)n * sizeof(T)) + (size_t)(n - 1) * (4 + lanes * 4) * sizeof(T);   // (before the index is known)
  if (tab > FUSED_LDS_LIMIT) return false;
  if (on < 0 && (P.nq < 65536 || (double)P.nq * (double)lanes * sizeof(T) < 4.0 * (double)cu_count() * (double)tab)) return false;
  h.pyr.ensure_dense_lut();
  if (!h.pyr.dense_ok) return false;
  // workgroup: 256 threads when four or more fit a CU beside each other (small tables: the staging pass is cheap and
  // short workgroups retire independently), else 1024
  P.f_tb = h.lanes_lds_bytes(256) * 4 <= 160 * 1024 ? 256u : 1024u;
  if (h.lanes_lds_bytes(P.f_tb) > FUSED_LDS_LIMIT) P.f_tb = 256u;   // (the strips of 16 waves do not fit: 4 waves)
  P.f_lds = h.lanes_lds_bytes(P.f_tb);
  if (P.f_lds > FUSED_LDS_LIMIT) return false;
  constexpr int VN = Wide<T>::N;
  P.l_qpl = (lanes == 1 && P.out_stride == 1 && aligned16(P.q) && aligned16(P.out)) ? VN : 1;
  const uint64_t per_wg = (uint64_t)P.f_tb * (lanes == 1 ? (uint64_t)P.l_qpl : 1);
  P.f_grid = resident_grid(P.nq, per_wg, P.f_lds, P.f_tb);
  P.kind = Plan1<T>::LANES;
  P.l_check = h.range_prepass(s, sc, {P.q, nullptr}, P.nq, fresh);
  return true;
}

template <class T>
static void launch_lanes1(Interp1DImpl<T>& h, hipStream_t s, StatusBlock* st, const Plan1<T>& P) {
  const uint64_t lanes = h.lanes;
  EvalLanesArgs<T> F{};
  table_args(F, h);
  F.n = (uint32_t)h.n;
  F.dl = h.pyr.dlut;
  batch_args(F, h, st, P.q, P.out, P.nq, P.out_stride);
  F.check = P.l_check ? 1 : 0;
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] lanes L=%llu qpl=%d index=%s m=%u maxk=%u tb=%u grid=%u lds=%zu prepass=%d\n", (unsigned long long)lanes,
                 P.l_qpl, h.pyr.dlut.lut ? "dense" : "guess", h.pyr.dlut.m, h.pyr.dlut.maxk, P.f_tb, P.f_grid, P.f_lds, P.l_check ? 0 : 1);
  constexpr int VN = Wide<T>::N;
  const dim3 grid(P.f_grid), block(P.f_tb);
  pick<ST_CUBIC, ST_LINEAR>(h.strat(), [&](auto st_) {
    constexpr int ST = st_;
    pick_or<256, 1024>((int)P.f_tb, [&](auto tb_) {
      constexpr int TB = tb_;
      if (lanes == 1)
        pick_or<1, VN>(P.l_qpl, [&](auto qpl_) {
          launch_lds<T>(eval_scalar_kernel<T, ST, qpl_, TB>, FUSED_LDS_LIMIT, s, PC_EVAL, grid, block, P.f_lds, F);
        });
      else
        pick_or<0, 2, 5, 8>((int)lanes, [&](auto lc_) {
          launch_lds<T>(eval_lanes_kernel<T, ST, lc_, TB>, FUSED_LDS_LIMIT, s, PC_EVAL, grid, block, P.f_lds, F);
        });
    });
  });
}

// ---- FUSED ---------------------------------------------------------------------------------------------------------------
// What the fused legs share.  The acceptance tail: the plan's kind and the range pre-pass the kernel relies on.
template <class T>
static bool accept_fused1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, Plan1<T>& P, bool fresh) {
  P.kind = Plan1<T>::FUSED;
  P.l_check = h.range_prepass(s, sc, {P.q, nullptr}, P.nq, fresh);
  return true;
}
// The workgroup size where no table form picks one: NDI_FUSED_TB when it pins 512 or 1024, else the planner's own.
static unsigned fused_tb_or(const ShortKnobs& K, unsigned tb_auto) { return (K.tb == 512 || K.tb == 1024) ? (unsigned)K.tb : tb_auto; }
// rows shorter than a cache line read from L2: one contiguous record per interval instead of three row pieces
// (NDI_FUSED_PACK pins it; the copy itself is ensure_packed's, asked for last)
template <class T>
static bool packed_rows_wanted(const Interp1DImpl<T>& h, const ShortKnobs& K) {
  return K.pack > 0 || (K.pack < 0 && h.lanes * sizeof(T) < 128);
}

// Axes too long for LDS: the same kernel with the knots left in global memory and searched through the u32 bucket
// index (TLDS == 3) -- one launch, no idx[] / t[] round trip.  Batches below 4096 queries keep the two-kernel form.
// Its LDS: the per-wave strips of one launch shape (UNR 2, TB 256) alone.
template <class T>
static size_t fused_global_lds_bytes(const Interp1DImpl<T>& h) {
  return h.fused_strip_bytes(256, h.strategy != NDI_CUBIC_SPLINE);
}
template <class T>
static bool plan_fused_global1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, Plan1<T>& P, const ShortKnobs& K, bool fresh) {
  if (P.nq < 4096) return false;
  h.pyr.ensure_bucket_index32();
  P.f_lut = false;
  P.f_unr = 2;
  P.f_tlds = 3;
  P.f_tb = 256;
  P.f_lds = fused_global_lds_bytes(h);
  P.f_pack = packed_rows_wanted(h, K) && h.ensure_packed(s);
  P.f_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((P.nq + 255) / 256, (uint64_t)cu_count() * 8 * 4));
  return accept_fused1(h, s, sc, P, fresh);
}

// The bucket index beside the knots when it costs no more than half the waves a CU could hold without it, and the
// workgroup size that keeps most waves on a CU (tables from memory: fused_lds_bytes(.., 0)).  False: no size fits.
template <class T>
static bool fused_index_and_tb1(const Interp1DImpl<T>& h, Plan1<T>& P, unsigned& tb_auto) {
  auto waves_at = [&](bool with_lut, unsigned tb) -> size_t {
    const size_t need = h.fused_lds_bytes(with_lut, tb, 0);
    return need > LDS_STAGE_LIMIT ? 0 : wgs_per_cu(need, tb) * (tb / 64);
  };
  auto best_tb = [&](bool with_lut, unsigned& tb_out) -> size_t {
    size_t best = 0;
    for (unsigned tb : {256u, 512u, 1024u}) {
      const size_t w = waves_at(with_lut, tb);
      if (w > best) { best = w; tb_out = tb; }
    }
    return best;
  };
  unsigned tb_plain = 256, tb_lut = 256;
  const size_t w_plain = best_tb(false, tb_plain);
  const size_t w_lut = (P.nq >= 4096 && h.pyr.lut_bytes != 0) ? best_tb(true, tb_lut) : 0;
  if (w_plain == 0 && w_lut == 0) return false;
  P.f_lut = w_lut != 0 && 2 * w_lut >= w_plain;
  tb_auto = P.f_lut ? tb_lut : tb_plain;
  return true;
}

// Tables in LDS when they fit beside everything else, and when the batch gives every workgroup several times the
// table size to write (the staging pass is per workgroup).  Workgroup size: the one that keeps most waves on a
// CU beside the tables; among equals the largest (fewest staging passes).
// {y, k} (the spline's derivatives, kept by small builds) is two thirds of {y, a, b}: it fits where the latter
// does not, and leaves room for more waves where both do.  NDI_FUSED_LDS = 1 / 2 pins the form.
// Sets P.f_tlds and P.f_tb (fused_lds_bytes(.., form) is the need of a form).
template <class T>
static void fused_table_form1(const Interp1DImpl<T>& h, Plan1<T>& P, const ShortKnobs& K, unsigned tb_auto) {
  const uint64_t lanes = h.lanes;
  P.f_tlds = 0;
  P.f_tb = fused_tb_or(K, tb_auto);
  if (K.lds == 0) return;
  size_t best_waves = 0;
  const bool yk_ok = h.strategy == NDI_CUBIC_SPLINE && h.ck.p;
  const int pinned = (K.lds == 2 && !yk_ok) ? 1 : K.lds;
  for (int form : {1, 2}) {   // equal wave counts: {y, a, b} (no per-item re-forming; 2-3 % faster where both fit)
    if (form == 2 && !yk_ok) continue;
    if (pinned > 0 && pinned <= 2 && pinned != form) continue;
    for (unsigned tb : {1024u, 512u, 256u}) {
      if (K.tb && (unsigned)K.tb != tb) continue;
      const size_t need = h.fused_lds_bytes(P.f_lut, tb, form);
      if (need > FUSED_LDS_LIMIT) continue;
      const size_t waves = wgs_per_cu(need, tb) * (tb / 64);
      if (waves > best_waves) {
        best_waves = waves;
        P.f_tlds = form;
        P.f_tb = tb;
      }
    }
  }
  const size_t tab = h.fused_lds_bytes(false, 64, P.f_tlds) - h.fused_lds_bytes(false, 64, 0);
  // not for small batches (the staging pass is per workgroup), and not for Linear rows of 128 B (f32: 64 B) or more:
  // two operand reads per item from L2 beat the workgroups that fit around a 64-128 KiB table (f32 x 32: 5.6 vs 4.9
  // TB/s, f32 x 16: 5.25 vs 4.76; f64 x 8 and f32 x 8 stay in LDS: 3.75 vs 2.8, 4.0 vs 2.8)
  if (P.f_tlds && K.lds < 0 && (P.nq * lanes * sizeof(T) < 8 * (size_t)cu_count() * tab ||
                                (h.strategy != NDI_CUBIC_SPLINE && lanes * sizeof(T) >= (sizeof(T) == 4 ? 64 : 128)))) {
    P.f_tlds = 0;
    P.f_tb = fused_tb_or(K, tb_auto);
  }
}

// Tables from L2, rows of 64 bytes and more, a large batch on an axis of up to 4096 intervals: the workgroup-local
// interval order (eval_fused_sorted_kernel: the operand rows of neighbouring items coincide and come from L1 -- the
// query-order form is bound by the L2 request rate on these).  NDI_FUSED_SORTED=0 / 1: A/B.
// Its LDS: [pyramid | lut | interval histogram | one round of queries: 4096 items (Linear 2048) of {index, 1 or 2 T}]
template <class T>
static size_t fused_sorted_lds_bytes(const Interp1DImpl<T>& h, bool with_lut) {
  const bool cubic = h.strategy == NDI_CUBIC_SPLINE;
  return ((h.pyr.lds_bytes + 15) & ~(size_t)15) + (with_lut ? h.pyr.lut_bytes : 0) + (((size_t)(h.n - 1) * 4 + 15) & ~(size_t)15) +
         (size_t)4096 / (cubic ? 1 : 2) * (4 + (cubic ? 1 : 2) * sizeof(T));
}
template <class T>
static bool plan_fused_sorted1(const Interp1DImpl<T>& h, Plan1<T>& P) {
  static const Knob fs_knob{"NDI_FUSED_SORTED", -1, Knob::live};
  const int fs = fs_knob.get();
  const uint64_t n = h.n, lanes = h.lanes;
  const bool cubic = h.strategy == NDI_CUBIC_SPLINE;
  const size_t lds_s = fused_sorted_lds_bytes(h, P.f_lut);
  // AUTO: where it was measured ahead (profiles/r05_tuning.md 10): CubicSpline (four operand rows per output row), rows of
  // 128 bytes and more, at least two queries per interval and round (4096 queries: axes of up to 2049 knots)
  P.f_sorted = fs != 0 && !P.f_tlds && n >= 3 && n - 1 <= 4096 && P.LV >= 2 && lanes * sizeof(T) >= 64 && lds_s <= FUSED_LDS_LIMIT - 256 &&
               (fs > 0 || (cubic && lanes * sizeof(T) >= 128 && n - 1 <= 2048 && P.nq >= (1u << 18)));
  if (!P.f_sorted) return false;
  P.f_pack = false;
  P.f_tb = 512;
  P.f_lds = lds_s;
  const size_t per_cu = std::max<size_t>(1, std::min<size_t>((160 * 1024) / lds_s, 4));
  const uint64_t nqw = cubic ? 4096 : 2048;
  P.f_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((P.nq + nqw - 1) / nqw, (uint64_t)cu_count() * per_cu * 4));
  return true;
}

// Query-order fused search + evaluation (short rows): decides the variant and its launch shape, and enqueues the
// range pre-pass the kernel relies on.  Returns false when the shape is not eligible.
template <class T>
static bool plan_fused1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, Plan1<T>& P, const ShortKnobs& K, bool fresh) {
  const uint64_t LV = P.LV;
  if (LV == 0 || 64ull * LV * LV >= (1ull << 32) || (uint64_t)h.n * LV >= (1ull << 32) * 1ull) return false;   // 32-bit item / vector indices
  // (axes beyond half the LDS: one large workgroup per CU; the bucket index: A/B settled in round 3)
  if (h.pyr.lds_bytes > LDS_STAGE_LIMIT - 8 * 1024) return plan_fused_global1(h, s, sc, P, K, fresh);
  if (P.nq >= 4096) h.pyr.ensure_bucket_index();
  unsigned tb_auto = 256;
  if (!fused_index_and_tb1(h, P, tb_auto)) return false;
  P.f_unr = (K.unr == 1 || K.unr == 4) ? K.unr : 2;
  fused_table_form1(h, P, K, tb_auto);
  P.f_lds = h.fused_lds_bytes(P.f_lut, P.f_tb, P.f_tlds);
  P.f_pack = !P.f_tlds && packed_rows_wanted(h, K) && h.ensure_packed(s);
  if (plan_fused_sorted1(h, P)) return accept_fused1(h, s, sc, P, fresh);
  const uint64_t want = (uint64_t)cu_count() * (K.wgs > 0 ? (size_t)K.wgs : wgs_per_cu(P.f_lds, P.f_tb) * (P.f_tlds ? 1 : 4));
  P.f_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((P.nq + P.f_tb - 1) / P.f_tb, want));
  return accept_fused1(h, s, sc, P, fresh);
}

template <class T>
static void launch_fused1(Interp1DImpl<T>& h, hipStream_t s, StatusBlock* st, const Plan1<T>& P) {
  const uint64_t lanes = h.lanes;
  EvalFusedArgs<T> F{};
  table_args(F, h);
  F.bx = P.f_lut ? h.pyr.bidx : BucketIndex<T>{nullptr, 0, T(0)};
  F.ck = h.ck.template as<T>();
  F.bx32 = P.f_tlds == 3 ? h.pyr.bidx32 : BucketIndex32<T>{nullptr, 0, T(0)};
  F.rec_stride = (uint32_t)P.LV;
  if (P.f_pack) {   // {y[i], y[i+1], a[i], b[i]} per interval
    F.data = h.packed.template as<T>();
    F.ca = h.packed.template as<T>() + 2 * lanes;
    F.cb = h.packed.template as<T>() + 3 * lanes;
    F.rec_stride = (uint32_t)P.LV * (h.strategy == NDI_CUBIC_SPLINE ? 4u : 2u);
  }
  batch_args(F, h, st, P.q, P.out, P.nq, P.out_stride);
  F.lv = (uint32_t)P.LV;
  F.lv_magic = F.lv >= 2 ? (uint32_t)(((1ull << 32) + F.lv - 1) / F.lv) : 0u;
  F.check = P.l_check ? 1 : 0;
  F.debug = 0;
#ifdef NDI_TUNING
  F.debug = env_int("NDI_FUSED_DEBUG", 0);
#endif
  constexpr int VN = Wide<T>::N;
  const dim3 grid(P.f_grid), block(P.f_tb);
  if (P.f_sorted) {
    if (trace_plan())
      std::fprintf(stderr, "[ndi plan] fused sorted lut=%d tb=%u grid=%u lds=%zu prepass=%d\n", (int)P.f_lut, P.f_tb, P.f_grid,
                   P.f_lds, P.l_check ? 0 : 1);
    pick<ST_CUBIC, ST_LINEAR>(h.strat(), [&](auto st_) {
      constexpr int ST = st_, QPT = ST == ST_CUBIC ? 8 : 4;   // 4096 queries per workgroup round, Linear 2048 (plan_fused_sorted1)
      pick_or<1, VN>(P.vec_ok ? VN : 1, [&](auto vec_) {
        launch_lds<T>(eval_fused_sorted_kernel<T, ST, vec_, 512, QPT>, FUSED_LDS_LIMIT - 256, s, PC_EVAL, grid, dim3(512), P.f_lds, F);
      });
    });
    return;
  }
  if (trace_plan())   // which variant a batch took (tests assert on it; read per call)
    std::fprintf(stderr, "[ndi plan] fused tables=%s lut=%d pack=%d unr=%d tb=%u grid=%u lds=%zu prepass=%d\n",
                 P.f_tlds == 2 ? "lds{y,k}" : (P.f_tlds == 1 ? "lds{y,a,b}" : (P.f_tlds == 3 ? "memory,knots=global" : "memory")),
                 (int)P.f_lut, (int)P.f_pack,
                 P.f_unr, P.f_tb, P.f_grid, P.f_lds, P.l_check ? 0 : 1);
  // TLDS: 0 = tables from memory, 1 = {y, a, b} in LDS, 2 = {y, k} in LDS (the spline only), 3 = knots in global memory
  // (one launch shape: UNR 2, TB 256)
  pick<ST_CUBIC, ST_LINEAR>(P.f_tlds == 2 ? (int)ST_CUBIC : h.strat(), [&](auto st_) {
    constexpr int ST = st_;
    pick_or<1, VN>(P.vec_ok ? VN : 1, [&](auto vec_) {
      constexpr int VEC = vec_;
      pick_or<1, 0, 2, 3>(P.f_tlds, [&](auto tl_) {
        constexpr int TL = tl_;
        if constexpr (TL == 3) {
          launch_lds<T>(eval_fused_kernel<T, ST, VEC, 2, 256, 3>, FUSED_LDS_LIMIT, s, PC_EVAL, grid, block, P.f_lds, F);
        } else if constexpr (TL != 2 || ST == ST_CUBIC) {
          pick_or<2, 4, 1>(P.f_unr, [&](auto unr_) {
            constexpr int UNR = unr_;
            pick_or<256, 1024, 512>((int)P.f_tb, [&](auto tb_) {
              launch_lds<T>(eval_fused_kernel<T, ST, VEC, UNR, tb_, TL>, FUSED_LDS_LIMIT, s, PC_EVAL, grid, block, P.f_lds, F);
            });
          });
        }
      });
    });
  });
}

// ---- SMALL ---------------------------------------------------------------------------------------------------------------
// 1-2 lanes: one thread per query (search + evaluation in one launch, tables gathered from L2) is the latency path
// and the faster one up to a few million queries; beyond, the query-order kernel with the tables in LDS takes over
// (scalar data at 1e8 queries: 98 -> 157 Gqueries/s f64, 2 lanes 45 -> 141).  Measured crossover
// (profiles/r04_scalar_crossover.jsonl): ~8e6 output elements on <= 1024 knots, proportionally earlier on longer
// axes (8192 knots: ~1e6), whose table gathers miss L1.
template <class T>
static bool plan_small1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, Plan1<T>& P, bool fresh) {
  constexpr long small_maxq = 8000000;
  if (!(h.lanes <= 2 && h.pyr.lds_bytes <= LDS_STAGE_LIMIT)) return false;
  const double small_work = (double)P.nq * (double)h.lanes * (double)std::max<uint64_t>(h.n, 1024) / 1024.0;
  if (small_work >= (double)small_maxq) {
    const ShortKnobs K0 = short_knobs();
    if (K0.mode != 1 && K0.mode != 3 && plan_fused1(h, s, sc, P, K0, fresh)) return true;
  }
  // short trailing axes: range pre-check (so rows after the first failing query stay untouched in the
  // caller's buffer), then search + evaluation fused in one launch -- no index / t round trip through HBM
  P.kind = Plan1<T>::SMALL;
  h.range_prepass(s, sc, {P.q, nullptr}, P.nq, false);
  return true;
}

// The arguments and the launch shape of eval_small_kernel: for the SMALL plan (pre-checked, the caller's row pitch) and for
// the small-row paths of the engine (Interp1DImpl::launch_small: packed rows, the kernel's own range test).
template <class T>
static EvalSmallArgs<T> small1_args(const Interp1DImpl<T>& h, StatusBlock* st, const T* q, T* out, uint64_t nq, uint64_t out_stride,
                                    int prechecked) {
  EvalSmallArgs<T> S{};
  table_args(S, h);
  batch_args(S, h, st, q, out, nq, out_stride);
  S.prechecked = prechecked;
  return S;
}
static unsigned small1_grid(uint64_t nq) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + BLOCK - 1) / BLOCK, 4096)); }
template <class T>
static size_t small1_lds_bytes(const Interp1DImpl<T>& h) { return (h.pyr.lds_bytes + 15) & ~(size_t)15; }

template <class T>
static void launch_small1(Interp1DImpl<T>& h, hipStream_t s, StatusBlock* st, const Plan1<T>& P) {
  const EvalSmallArgs<T> S = small1_args(h, st, P.q, P.out, P.nq, P.out_stride, 1);
  pick<ST_CUBIC, ST_LINEAR>(h.strat(), [&](auto st_) {
    launch_lds<T>(eval_small_kernel<T, st_>, LDS_STAGE_LIMIT, s, PC_EVAL, dim3(small1_grid(P.nq)), dim3(BLOCK), small1_lds_bytes(h), S);
  });
}

// The fused search + evaluation launch of the small-row paths: nq packed rows into out, the kernel's own range test.
template <class T>
void Interp1DImpl<T>::launch_small(hipStream_t s, StatusBlock* st, Queries<T> q, T* out, uint64_t nq) {
  const EvalSmallArgs<T> A = small1_args(*this, st, q.a, out, nq, lanes, 0);
  const dim3 grid(small1_grid(nq));
  if (strategy == NDI_CUBIC_SPLINE) launch1<T>(s, PC_EVAL, grid, dim3(BLOCK), small1_lds_bytes(*this), eval_small_kernel<T, ST_CUBIC>, A);
  else launch1<T>(s, PC_EVAL, grid, dim3(BLOCK), small1_lds_bytes(*this), eval_small_kernel<T, ST_LINEAR>, A);
}

// ---- the two-kernel forms: grouped (BUCKETED, BUCKETED_SHORT) or in query order (ROWS, FLAT) --------------------------------
// Which batches are grouped by interval: long rows (`bucketed`, eval_bucketed_kernel) and short ones (`grouped_short`,
// eval_bucketed_short_kernel).  rows_ok: whole workgroup passes of aligned vectors; short_rows: shorter than one (or
// unaligned) -- grouped from a few hundred bytes per row upwards when the batch has enough queries per interval, else query
// order with the search fused in.
struct Grouping1 {
  bool bucketed = false, grouped_short = false;
};
template <class T>
static Grouping1 grouping1(const Interp1DImpl<T>& h, const Plan1<T>& P, const ShortKnobs& K, int path, bool rows_ok, bool short_rows) {
  const uint64_t n = h.n, lanes = h.lanes, nq = P.nq;
  // (axes whose interval histogram does not fit LDS are grouped with global atomics, as long rows are)
  const bool group_ok = nq < 0xffffffffull && P.vec_ok && P.LV < (uint64_t)BLOCK;
  Grouping1 g;
  if (path == NDI_PATH_BUCKETED) {
    g.bucketed = rows_ok && nq < 0xffffffffull;
    g.grouped_short = short_rows && group_ok && K.mode != 1 && K.mode != 2;
  } else if (path == NDI_PATH_AUTO) {
    g.bucketed = rows_ok && nq < 0xffffffffull && nq >= 5 * (n - 1);  // measured crossover (tools/auto_threshold.py)
    // (Linear reads two operand rows per item instead of four: its query-order form already runs at 5-6 TB/s on rows
    //  of 128 B - 2 KiB and beats the grouped form everywhere: profiles/r04_short_rows_linear_sweep.txt)
    g.grouped_short = short_rows && group_ok && nq >= 5 * (n - 1) &&
                      (K.mode == 3 ||
                       // Linear: only when its one table outgrows L2 and the rows are 1 KiB or more (16 384 knots x 512 f32
                       // lanes, 33.6 MB: 3.54 vs 2.55 TB/s)
                       (K.mode == 0 && h.strategy != NDI_CUBIC_SPLINE && lanes * sizeof(T) >= 1024 &&
                        (size_t)n * lanes * sizeof(T) >= ((size_t)8 << 20)) ||
                       (K.mode == 0 && h.strategy == NDI_CUBIC_SPLINE &&
                                       (lanes * sizeof(T) >= (uint64_t)K.rowb ||
                                        // tables that outgrow L2 (its 4 MiB per XCD): the query-order form re-reads them
                                        // from memory per query, the grouped form once per interval -- from 512-byte rows
                                        // (8192 knots x 128 f32 lanes, 12.6 MB: 3.94 vs 2.21 TB/s; tools/group_vs_fused_probe.py)
                                        (lanes * sizeof(T) >= 512 && (size_t)(3 * n - 2) * lanes * sizeof(T) >= ((size_t)8 << 20)))));
  }
  return g;
}

// The search, then block-local counting sort: histogram per query slice in LDS, no global atomics.  `t_out`: where the
// search leaves t (cubic; Linear: nullptr); `sval`: what a grouped record carries -- t (cubic) / raw x (linear).
template <class T>
static void group_one_pass1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan1<T>& P, T* t_out, const T* sval, bool beside_eval) {
  StatusBlock* st = sc.status.as<StatusBlock>();
  const uint32_t nb = (uint32_t)(h.n - 1);
  sc.hist.reserve((size_t)GROUP_MAX_BLOCKS * nb * sizeof(uint32_t));
  uint64_t slice = 0;
  uint32_t blocks = 0;
  run_locate<T>(s, h.pyr, P.q, P.nq, sc.idx.as<uint32_t>(), nullptr, t_out,
                &st->first_fail[0], h.mode, sc.hist.as<uint32_t>(), nb, &slice, &blocks, beside_eval);
  ProfScope ps(s, PC_GROUP);
  hipLaunchKernelGGL(group_offsets_scan_kernel, dim3((nb + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s,
                     sc.hist.as<uint32_t>(), blocks, nb, sc.counts.as<uint32_t>(), sc.cursor.as<uint32_t>(), st,
                     P.nq, 0u, (uint32_t*)nullptr);
  allow_dynamic_lds(reinterpret_cast<const void*>(&group_scatter_kernel<T>), (int)(GROUP_MAX_BINS * 4));
  hipLaunchKernelGGL(group_scatter_kernel<T>, dim3(blocks), dim3(BLOCK), (size_t)nb * 4, s,
                     (const uint32_t*)sc.idx.as<uint32_t>(), sval, P.nq, slice,
                     (const uint32_t*)sc.hist.as<uint32_t>(), (const uint32_t*)sc.cursor.as<uint32_t>(),
                     nb, sc.perm.as<uint4>());
  NDI_HIP(hipGetLastError());
  ps.done();
}

// ... many intervals: histogram and placement with global atomics
template <class T>
static void group_atomics1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan1<T>& P, T* t_out, const T* sval) {
  StatusBlock* st = sc.status.as<StatusBlock>();
  const uint32_t nb = (uint32_t)(h.n - 1);
  const uint64_t nq = P.nq;
  run_locate<T>(s, h.pyr, P.q, nq, sc.idx.as<uint32_t>(), nullptr, t_out, &st->first_fail[0], h.mode);
  ProfScope ps(s, PC_GROUP);
  NDI_HIP(hipMemsetAsync(sc.counts.p, 0, (size_t)nb * sizeof(uint32_t), s));
  const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + BLOCK - 1) / BLOCK, 2048));
  hipLaunchKernelGGL(bucket_count_kernel, dim3(g), dim3(BLOCK), 0, s, (const uint32_t*)sc.idx.as<uint32_t>(), nq,
                     (const StatusBlock*)st, sc.counts.as<uint32_t>());
  hipLaunchKernelGGL(bucket_scan_kernel<256>, dim3(1), dim3(256), 0, s, sc.counts.as<uint32_t>(), nb,
                     sc.cursor.as<uint32_t>(), st);
  hipLaunchKernelGGL(bucket_scatter_kernel<T>, dim3(g), dim3(BLOCK), 0, s, (const uint32_t*)sc.idx.as<uint32_t>(),
                     sval, nq, (const StatusBlock*)st, sc.cursor.as<uint32_t>(), sc.perm.as<uint4>());
  NDI_HIP(hipGetLastError());
  ps.done();
}

// What the evaluation kernels of the two-kernel forms take: the tables, the batch, the search's idx / t (grouped: `rec`).
template <class T>
static Eval1Args<T> eval1_args(const Interp1DImpl<T>& h, Scratch& sc, const Plan1<T>& P) {
  Eval1Args<T> A{};
  table_args(A, h);
  A.q = P.q;
  A.idx = sc.idx.as<uint32_t>();
  A.t = sc.t.as<T>();
  A.out = P.out;
  A.lanes = h.lanes;
  A.out_stride = P.out_stride;
  A.nq = P.nq;
  A.status = sc.status.as<StatusBlock>();
  A.n_int = (uint32_t)(h.n - 1);
#ifdef NDI_BOUNDS
  if (env_int("NDI_BOUNDS_SELFTEST", 0)) A.n_int = 1;   // checked build: provoke the checker (rows are then wrong)
#endif
  return A;
}

// The long-row grouped evaluation: eval_bucketed_kernel for one chunk, eval_bucketed_group_kernel (GROUP) for the chunks
// of a ring group.  U vectors per thread by row length, gx workgroups per segment row; rows of whole segments only
// take the straight-line kernel variant.
template <bool GROUP, class T, class Args>
static void launch_bucketed(Interp1DImpl<T>& h, hipStream_t s, uint64_t LV, unsigned gx, const Args& A) {
  constexpr int CQ = Interp1DImpl<T>::BUCKETED_CQ;
  const int U = LV >= 2048 ? 8 : (LV >= 1024 ? 4 : (LV >= 512 ? 2 : 1));
  const uint64_t segs = (LV + (uint64_t)BLOCK * U - 1) / ((uint64_t)BLOCK * U);
  const dim3 grid(gx, (unsigned)std::min<uint64_t>(segs, 64));
  const bool full = LV % ((uint64_t)BLOCK * U) == 0;
  pick<ST_CUBIC, ST_LINEAR>(h.strat(), [&](auto st_) {
    constexpr int ST = st_;
    pick_or<1, 8, 4, 2>(U, [&](auto u_) {
      constexpr int UU = u_;
      pick_bool(full, [&](auto full_) {
        if constexpr (GROUP) launch1<T>(s, PC_EVAL, grid, dim3(BLOCK), 0, eval_bucketed_group_kernel<T, ST, UU, CQ, true, full_>, A);
        else launch1<T>(s, PC_EVAL, grid, dim3(BLOCK), 0, eval_bucketed_kernel<T, ST, UU, CQ, true, full_>, A);
      });
    });
  });
}

template <class T>
static void launch_bucketed1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan1<T>& P) {
  Eval1Args<T> A = eval1_args(h, sc, P);
  A.rec = sc.perm.as<uint4>();
  constexpr int CQ = Interp1DImpl<T>::BUCKETED_CQ;
  // a multiple of 8 so that a workgroup keeps its XCD residue when it strides (XCD-aware chunk order);
  // every workgroup takes a run of consecutive chunks (operand rows stay in registers across them)
  const uint64_t per_xcd = ((P.nq + CQ - 1) / CQ + 7) / 8;
  A.run = BUCKETED_RUN;
  const uint64_t runs_per_xcd = (per_xcd + A.run - 1) / A.run;
  launch_bucketed<false>(h, s, P.LV, (unsigned)std::max<uint64_t>(8, std::min<uint64_t>(runs_per_xcd * 8, 65528)), A);
}

template <class T>
static void launch_bucketed_short1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan1<T>& P) {
  Eval1Args<T> A = eval1_args(h, sc, P);
  A.rec = sc.perm.as<uint4>();
  uint32_t G = 8;
  while (G < P.LV) G *= 2;   // threads per row: power of two >= vectors per row (LV < 256)
  const int CQ = P.s_cq == 16 ? 16 : 64;
  const uint64_t wq = (uint64_t)(BLOCK / G) * CQ;
  const uint64_t per_xcd = ((P.nq + wq - 1) / wq + 7) / 8;
  const unsigned gx = (unsigned)std::max<uint64_t>(8, std::min<uint64_t>(per_xcd * 8, 65528));
  pick<ST_CUBIC, ST_LINEAR>(h.strat(), [&](auto st_) {
    constexpr int ST = st_;
    pick_or<256, 8, 16, 32, 64, 128>((int)G, [&](auto g_) {
      constexpr int GG = g_;
      pick_or<64, 16>(CQ, [&](auto cq_) {
        launch1<T>(s, PC_EVAL, dim3(gx), dim3(BLOCK), 0, eval_bucketed_short_kernel<T, ST, GG, cq_>, A);
      });
    });
  });
}

template <class T>
static void launch_rows1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan1<T>& P) {
  const Eval1Args<T> A = eval1_args(h, sc, P);
  // one 256-vector segment per workgroup pass and many workgroups: measured best on MI355X
  const uint64_t segs = (P.LV + BLOCK - 1) / BLOCK;
  const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(P.nq, 65536));
  dim3 grid(gx, (unsigned)std::min<uint64_t>(segs, 64));
  pick<ST_CUBIC, ST_LINEAR>(h.strat(), [&](auto st_) { launch1<T>(s, PC_EVAL, grid, dim3(BLOCK), 0, eval_rows_kernel<T, st_, 1>, A); });
}

template <class T>
static void launch_flat1(Interp1DImpl<T>& h, hipStream_t s, Scratch& sc, const Plan1<T>& P) {
  const Eval1Args<T> A = eval1_args(h, sc, P);
  constexpr int VN = Wide<T>::N;
  const uint32_t tile_q = (uint32_t)std::max<uint64_t>(1, 1024 / std::max<uint64_t>(P.LV, 1));
  const uint64_t ntiles = (P.nq + tile_q - 1) / tile_q;
  const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, 16384));
  ProfScope ps(s, PC_EVAL);
  pick<ST_CUBIC, ST_LINEAR>(h.strat(), [&](auto st_) {
    constexpr int ST = st_;
    pick_or<1, VN>(P.vec_ok ? VN : 1, [&](auto vec_) {
      hipLaunchKernelGGL((eval_flat_kernel<T, ST, vec_>), dim3(gx), dim3(BLOCK), 0, s, A, tile_q);
    });
  });
  NDI_HIP(hipGetLastError());
  ps.done();
}

// ---- the two stages ----------------------------------------------------------------------------------------------------------
template <class T>
Plan1<T> Interp1DImpl<T>::prep(hipStream_t s, Scratch& sc, const T* q, uint64_t nq, T* out, uint64_t out_stride, int path,
                               bool beside_eval, int flags) {
  Plan P;
  P.q = q; P.nq = nq; P.out = out; P.out_stride = out_stride;
  constexpr int VN = Wide<T>::N;
  P.vec_ok = (lanes % VN == 0) && (out_stride % VN == 0) && aligned16(out);
  P.LV = P.vec_ok ? lanes / VN : lanes;
  sc.status.reserve(sizeof(StatusBlock));
  reset_status(sc.status.p, s);
  StatusBlock* st = sc.status.as<StatusBlock>();
  const bool fresh = (flags & NDI_EVAL_FRESH_OUTPUT) != 0;
  if (plan_lanes1(*this, s, sc, P, path, fresh)) return P;
  if (plan_small1(*this, s, sc, P, fresh)) return P;
  const bool rows_ok = P.vec_ok && P.LV >= (uint64_t)BLOCK;
  const ShortKnobs K = short_knobs();
  const bool short_rows = !rows_ok || (P.vec_ok && P.LV < (uint64_t)K.maxlv);
  const Grouping1 g = grouping1(*this, P, K, path, rows_ok, short_rows);
  if (short_rows && !g.grouped_short && !g.bucketed && K.mode != 1 && K.mode != 3 && plan_fused1(*this, s, sc, P, K, fresh)) return P;
  g_last_path.store(g.bucketed || g.grouped_short ? NDI_PATH_BUCKETED : NDI_PATH_GATHER);
  sc.idx.reserve(nq * sizeof(uint32_t));   // the two-kernel forms: interval index (and t) per query
  if (strategy == NDI_CUBIC_SPLINE) sc.t.reserve(nq * sizeof(T));
  T* t_out = strategy == NDI_CUBIC_SPLINE ? sc.t.as<T>() : nullptr;
  if (g.bucketed || g.grouped_short) {
    P.kind = g.bucketed ? Plan::BUCKETED : Plan::BUCKETED_SHORT;
    P.s_cq = K.cq;
    const uint32_t nb = (uint32_t)(n - 1);
    sc.counts.reserve(((size_t)nb + 4) * sizeof(uint32_t));   // (+4: the fused scan reads / writes 16-byte pieces)
    sc.cursor.reserve(((size_t)nb + 4) * sizeof(uint32_t));
    sc.perm.reserve(nq * sizeof(uint4));
    const T* sval = strategy == NDI_CUBIC_SPLINE ? (const T*)t_out : q;   // t (cubic) / raw x (linear)
    if (lds_sort_fits(pyr, nb)) group_one_pass1(*this, s, sc, P, t_out, sval, beside_eval);
    else group_atomics1(*this, s, sc, P, t_out, sval);
    return P;
  }
  run_locate<T>(s, pyr, q, nq, sc.idx.as<uint32_t>(), nullptr, t_out, &st->first_fail[0], mode);
  P.kind = rows_ok ? Plan::ROWS : Plan::FLAT;
  return P;
}

template <class T>
void Interp1DImpl<T>::launch_eval(hipStream_t s, Scratch& sc, const Plan& P) {
  StatusBlock* st = sc.status.as<StatusBlock>();
  switch (P.kind) {
    case Plan::SMALL: return launch_small1(*this, s, st, P);
    case Plan::LANES: return launch_lanes1(*this, s, st, P);
    case Plan::FUSED: return launch_fused1(*this, s, st, P);
    case Plan::BUCKETED: return launch_bucketed1(*this, s, sc, P);
    case Plan::BUCKETED_SHORT: return launch_bucketed_short1(*this, s, sc, P);
    case Plan::ROWS: return launch_rows1(*this, s, sc, P);
    case Plan::FLAT: return launch_flat1(*this, s, sc, P);
  }
}

// ---- ring groups: one evaluation launch for several chunks of a ring (float_host.hpp ring_produce) ----------------
// Evaluates the w >= 1 chunks prepared into sc[0 .. w) with the plans P[0 .. w) -- all groupable, one row pitch -- in
// ONE launch (w = 1: the single-chunk kernel, launch_eval).
template <class T>
void Interp1DImpl<T>::launch_eval_group(hipStream_t s, Scratch* const* sc, const Plan* P, uint32_t w) {
  if (trace_plan())
    std::fprintf(stderr, "[ndi plan] ring bucketed L=%llu lv=%llu width=%u nq=%llu\n", (unsigned long long)lanes,
                 (unsigned long long)P[0].LV, w, (unsigned long long)P[0].nq);
  if (w == 1) {
    launch_eval(s, *sc[0], P[0]);
    return;
  }
  if (w > (uint32_t)RING_GROUP_MAX) throw HipFailure{hipErrorInvalidValue, "launch_eval_group: group too wide", __LINE__};
  EvalGroupArgs<T> G{};
  table_args(G.A, *this);
  G.A.lanes = lanes;
  G.A.out_stride = P[0].out_stride;
  G.A.n_int = (uint32_t)(n - 1);
  G.width = w;
  constexpr int CQ = BUCKETED_CQ;
  uint64_t nmax = 0;
  for (uint32_t i = 0; i < w; ++i) {
    if (!groupable(P[i]) || P[i].out_stride != P[0].out_stride || P[i].LV != P[0].LV)
      throw HipFailure{hipErrorInvalidValue, "launch_eval_group: plans of one group differ", __LINE__};
    G.rec[i] = sc[i]->perm.as<uint4>();
    G.nq[i] = P[i].nq;
    G.out[i] = P[i].out;
    G.status[i] = sc[i]->status.as<StatusBlock>();
    nmax = std::max<uint64_t>(nmax, (P[i].nq + CQ - 1) / CQ);
  }
  const uint64_t per_xcd = (nmax * w + 7) / 8;
  launch_bucketed<true>(*this, s, P[0].LV, (unsigned)std::max<uint64_t>(8, std::min<uint64_t>(per_xcd * 8, 65528)), G);
}
