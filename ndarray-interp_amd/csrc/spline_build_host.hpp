// csrc/spline_build_host.hpp -- the build host of the 1-D cubic tables (included by ndinterp_api.hip after Interp1DImpl): the
// CubicSpline build (Interp1DImpl::build_spline, a dispatcher over build_form, build_small_fused, build_blocked and
// build_serial), BoundaryCondition::Individual (build_spline_individual) and the local cubics (Interp1DImpl::build_hermite).
// Every build runs on the NULL stream and its tables are complete when create() returns.  What the forms have alike is stated
// once: the reserve of a / b (reserve_tables), the BuildArgs fill from a SplinePlan (build_args), the two grids
// (build_rows_grid, build_lane_grid), spline_build_general_kernel with or without the kept k table (launch_build_general) and
// the periodic verdict (periodic_verdict).
#pragma once

template <class T>
static void reserve_tables(Interp1DImpl<T>& h) {
  const size_t tab = (size_t)(h.n - 1) * h.lanes * sizeof(T);
  h.ca.reserve(tab);
  h.cb.reserve(tab);
}

// One thread per (row, lane) -- the right-hand sides and the blocked fix / finish passes -- and one lane per thread in waves
// of 64: the serial sweeps.
static unsigned build_rows_grid(uint64_t n, uint64_t lanes) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n * lanes + BLOCK - 1) / BLOCK, 65536));
}
static unsigned build_lane_grid(uint64_t lanes) { return (unsigned)((lanes + 63) / 64); }

// What every spline build hands its kernels: the tables and the x-only scalars of the plan (the end kinds and values, the
// not-a-knot rows, the squared end spacings, the periodic denominator).  The Individual build's kernels take the end kinds
// and values per lane instead.
template <class T>
static BuildArgs<T> build_args(Interp1DImpl<T>& h, const SplinePlan<T>& P) {
  BuildArgs<T> A{};
  A.data = h.data.template as<T>();
  A.ca = h.ca.template as<T>();
  A.cb = h.cb.template as<T>();
  A.n = h.n;
  A.lanes = h.lanes;
  A.left_kind = P.left_kind;
  A.right_kind = P.right_kind;
  A.left_val = P.left_val;
  A.right_val = P.right_val;
  A.nkL_tmp1 = P.nkL_tmp1; A.nkL_d = P.nkL_d;
  A.nkR_tmp1 = P.nkR_tmp1; A.nkR_d = P.nkR_d;
  A.dx0_sq = P.dx0_sq; A.dxl_sq = P.dxl_sq;
  A.per_den = P.per_den;
  return A;
}

// spline_build_general_kernel on one lane per thread, with the k table where reserve_k kept one.  Named with the three
// (PER_LANE, FUSED) pairs that are launched -- <false, true> the one-launch build, <false, false> the serial build,
// <true, false> Individual -- and with no other: every instance named here is emitted.
template <class T, bool PER_LANE, bool FUSED>
static void launch_build_general(const BuildArgs<T>& A) {
  pick_bool(A.kout != nullptr, [&](auto kout_) {
    hipLaunchKernelGGL((spline_build_general_kernel<T, PER_LANE, kout_, FUSED>), dim3(build_lane_grid(A.lanes)), dim3(64), 0,
                       (hipStream_t) nullptr, A);
  });
}

// What the build reports through its status block: first and last value of a periodic lane must be equal.  A periodic build
// that passes turns an extrapolating handle periodic -- Extrapolate::{No,Yes,Periodic}, cubic_spline.rs:763-769.
template <class T>
static ndi_status periodic_verdict(Interp1DImpl<T>& h, const StatusBlock& hs, bool periodic) {
  if (hs.periodic_mismatch != 0)
    return fail(NDI_VALUE,
                "for periodic boundary condition the first and last value must be equal "
                "(%llu lane(s) differ)", hs.periodic_mismatch);
  if (h.mode != EX_NO && periodic) h.mode = EX_PERIODIC;
  return NDI_OK;
}

// Blocked sweeps or serial kernels, and where the x-only elimination runs.
struct BuildForm {
  bool blocked, dev_elim;
};
template <class T>
static BuildForm build_form(const Interp1DImpl<T>& h, const ndi_interp1d_desc& d) {
  const uint64_t n = h.n;
  // Blocked sweeps or serial kernels?  Narrow trailing axes with many knots: the per-lane serial kernel would be one
  // or two waves doing 2n dependent steps.  The blocked sweeps (kernels.hpp, spline_blocked_*) take over -- the one
  // path whose tables are not bit-identical to the reference order (a few ulp; NDI_SPLINE_BLOCKED=0 keeps the serial
  // kernels, =1 forces the blocked ones wherever they apply).
  static const Knob blocked_knob{"NDI_SPLINE_BLOCKED", -1, Knob::live};
  const int blocked_env = blocked_knob.get();
  // ... and only on axes whose neighbouring knot spacings differ by less than 1e3 (f32) / 1e9 (f64): the re-associated
  // sweeps are accurate relative to the NEIGHBOURING table magnitudes, and where the spacing jumps by 1e6 from one
  // interval to the next those magnitudes jump likewise -- in f32 evaluated rows then miss the 1e-5 bar (4 of 5000 rows
  // at 4e-5 on gaps drawn log-uniformly over six decades, tests/test_gpu_spline_blocked.py).  Such axes keep the serial
  // kernels: bit-identical.
  bool tame = true;
  if (blocked_env != 0 && n >= 16) {      // (also when the blocked build is forced: the device-side elimination needs it)
    const double lim = sizeof(T) == 4 ? 1e3 : 1e9;
    const T* xs = h.pyr.host_knots.data();
    for (uint64_t i = 2; tame && i < n; ++i) {
      const double a = (double)xs[i] - (double)xs[i - 1], b = (double)xs[i - 1] - (double)xs[i - 2];
      tame = a <= lim * b && b <= lim * a;
    }
  }
  // (n >= 16: the system is the GENERAL or the PERIODIC one -- the closed forms are n == 3)
  const bool blocked = n >= 16 && !(d.build_flags & NDI_BUILD_REFERENCE_ORDER) &&
                       (blocked_env > 0 || (blocked_env < 0 && n >= 2048 && h.lanes <= 256 && tame));
  // Long axes: the x-only elimination factors on the device as well (spline_eliminate_kernel); the host then forms only
  // the boundary rows' scalars.
  return {blocked, blocked && tame && !d.periodic && n >= 32768};
}

// Small systems (the reference's (100, 5); 1024 x 8; ...): ONE launch -- right-hand sides, elimination, back
// substitution and the a / b epilogue in spline_build_general_kernel<FUSED>, dx / up formed from the resident knots;
// the x-only factors w, mid' travel through a kept pinned buffer into a kept device buffer: no allocation, no free,
// no status read-back (only the periodic build has one).  Same operations as the three-kernel form: bit-identical.
template <class T>
static ndi_status build_small_fused(Interp1DImpl<T>& h, const SplinePlan<T>& P, BuildClock& clk) {
  const uint64_t n = h.n, lanes = h.lanes;
  BuildScratch& bs = build_scratch();
  const size_t plan_b = 2 * (size_t)n * sizeof(T);
  T* hp = static_cast<T*>(bs.pinned(plan_b));
  T* dp = static_cast<T*>(bs.device_buf(h.device, plan_b));
  std::memcpy(hp, P.w.data(), (size_t)n * sizeof(T));
  std::memcpy(hp + n, P.midp.data(), (size_t)n * sizeof(T));
  NDI_HIP(hipMemcpyAsync(dp, hp, plan_b, hipMemcpyHostToDevice, nullptr));
  clk.mark("    plan staged + copy enqueued");
  BuildArgs<T> A = build_args(h, P);
  A.x = h.pyr.view.lv0;
  A.w = dp;
  A.midp = dp + n;
  A.up_len = P.up.size();
  A.left_up0 = P.up.front();
  A.up_last = P.up.back();
  A.kout = h.reserve_k();
  // the smallest systems -- data and right-hand sides fit LDS twice over, one workgroup covers the trailing axis --
  // form their right-hand sides with the whole workgroup and sweep out of LDS (spline_build_lds_kernel)
  const size_t lds_need = 2 * (size_t)n * lanes * sizeof(T);
  if (lanes <= (uint64_t)BLOCK && lds_need <= 96 * 1024 && n >= 4) {
    allow_dynamic_lds(reinterpret_cast<const void*>(&spline_build_lds_kernel<T, true>), 96 * 1024);
    allow_dynamic_lds(reinterpret_cast<const void*>(&spline_build_lds_kernel<T, false>), 96 * 1024);
    pick_bool(A.kout != nullptr, [&](auto kout_) {
      hipLaunchKernelGGL((spline_build_lds_kernel<T, kout_>), dim3(1), dim3(BLOCK), lds_need, (hipStream_t) nullptr, A);
    });
  } else {
    launch_build_general<T, false, true>(A);
  }
  NDI_HIP(hipGetLastError());
  clk.mark("    kernel enqueued");
  NDI_HIP(hipStreamSynchronize(nullptr));   // the tables are complete when create() returns: any stream may read them
  clk.mark("  fused small build");
  return NDI_OK;
}

// ONE temporary allocation of the larger builds (one hipMalloc, one hipFree -- each costs as much as the kernels of a small
// build):
//   [status | dx (n) | up (n) | w (n) | mid' (n) | k2 (n) | blocked: fP | dco | bP | rfull | ends | carry]
// dx and up are formed on the device from the knots already there (the same subtractions in T as the host plan's);
// w, mid' and k2 -- the results of the host's division chain -- are uploaded straight from their vectors.
template <class T>
struct BuildTemp {
  uint64_t rows;       // order of the system the two sweeps run over
  uint64_t S = 64;     // ~sqrt(n) rows per block: local sweeps and carry chain balance
  uint64_t nblk;
  DevBuf own;          // (a temporary too large to keep)
  void* p = nullptr;
  T *dx, *up, *w, *mid, *k2, *sweeps;

  BuildTemp(const Interp1DImpl<T>& h, bool per, bool blocked) {
    const uint64_t n = h.n, lanes = h.lanes;
    rows = per ? n - 2 : n;
    while (S * S < rows && S < 2048) S *= 2;
    nblk = (rows + S - 1) / S;
    const size_t plan_elems = 5 * (size_t)n;
    const size_t blk_elems = blocked ? 3 * (size_t)n + (size_t)n * lanes + 2 * (size_t)nblk * lanes : 0;
    // temporaries: kept per host thread up to 64 MiB (hipMalloc + hipFree of a 48 MB buffer cost 4 ms of a 1e6-knot build,
    // and more than the kernels of a 4096 x 8 one); larger ones are allocated and freed here
    const size_t bytes = 256 + (plan_elems + blk_elems) * sizeof(T);
    if (bytes <= ((size_t)64 << 20)) {
      p = build_scratch().device_buf(h.device, bytes);
    } else {
      own.reserve(bytes);
      p = own.p;
    }
    T* const plan = reinterpret_cast<T*>((char*)p + 256);
    dx = plan;
    up = plan + n;
    w = plan + 2 * (size_t)n;
    mid = plan + 3 * (size_t)n;
    k2 = plan + 4 * (size_t)n;
    sweeps = plan + plan_elems;
  }
  StatusBlock* status() const { return static_cast<StatusBlock*>(p); }

  // the plan's part of the arguments
  void plan_into(BuildArgs<T>& A) const {
    A.dx = dx;
    A.up = up;
    A.w = w;
    A.midp = mid;
    A.k2 = k2;
    A.status = status();
  }
  // [fP | dco | bP | rfull | ends | carry]; the coefficient products are formed on the device
  void sweeps_into(BuildArgs<T>& A) const {
    const uint64_t n = A.n, lanes = A.lanes;
    A.fP = sweeps;
    A.dco = sweeps + n;
    A.bP = sweeps + 2 * n;
    A.rfull = sweeps + 3 * n;
    A.ends = A.rfull + n * lanes;
    A.carry = A.ends + nblk * lanes;
    A.S = S;
    A.nblocks = nblk;
    A.rows = rows;
  }
};

// The status block cleared, the host's factors uploaded (w, mid', k2), dx and up formed on the device -- and, with the
// device-side elimination, w and mid' as well.
template <class T>
static void upload_plan(const Interp1DImpl<T>& h, const SplinePlan<T>& P, const SplineEnds<T>& ends, bool dev_elim,
                        const BuildTemp<T>& tmp) {
  const uint64_t n = h.n;
  NDI_HIP(hipMemsetAsync(tmp.p, 0, sizeof(StatusBlock), nullptr));
  if (!P.w.empty()) NDI_HIP(hipMemcpyAsync(tmp.w, P.w.data(), P.w.size() * sizeof(T), hipMemcpyHostToDevice, nullptr));
  if (!P.midp.empty()) NDI_HIP(hipMemcpyAsync(tmp.mid, P.midp.data(), P.midp.size() * sizeof(T), hipMemcpyHostToDevice, nullptr));
  if (!P.k2.empty()) NDI_HIP(hipMemcpyAsync(tmp.k2, P.k2.data(), P.k2.size() * sizeof(T), hipMemcpyHostToDevice, nullptr));
  const uint64_t up_len = dev_elim ? n : P.up.size();
  const T up_first = dev_elim ? ends.up_first : (up_len ? P.up[0] : T(0));
  const T up_last = dev_elim ? T(0) : (up_len ? P.up[up_len - 1] : T(0));
  const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + BLOCK - 1) / BLOCK, 4096));
  hipLaunchKernelGGL(spline_dx_up_kernel<T>, dim3(g), dim3(BLOCK), 0, (hipStream_t) nullptr, (const T*)h.pyr.view.lv0, tmp.dx, tmp.up,
                     n, up_len, up_first, up_last);
  if (dev_elim) {   // w, mid' where the host plan would have been uploaded
    const uint64_t SE = 256;
    const uint64_t tasks = (n + SE - 1) / SE;
    hipLaunchKernelGGL(spline_eliminate_kernel<T>, dim3((unsigned)((tasks + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t) nullptr,
                       (const T*)h.pyr.view.lv0, n, ends.up_first, ends.mid_first, ends.low_last, ends.mid_last, tmp.w, tmp.mid, SE);
  }
  NDI_HIP(hipGetLastError());
}

// The blocked sweeps, general and periodic: nine launches.  The periodic build reads its status back into `hs`, the general
// one waits for the stream.
template <class T>
static void build_blocked(BuildArgs<T>& A, const BuildTemp<T>& tmp, bool per, StatusBlock& hs) {
  tmp.sweeps_into(A);
  hipStream_t s = nullptr;
  const uint64_t nblk = tmp.nblk;
  const unsigned grid = build_lane_grid(A.lanes), gr = build_rows_grid(A.n, A.lanes);
  const unsigned gl = (unsigned)((nblk * A.lanes + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(spline_blocked_coef_kernel<T>, dim3((unsigned)((nblk + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s,
                     A.w, A.up, A.midp, tmp.sweeps, tmp.sweeps + A.n, tmp.sweeps + 2 * A.n, tmp.rows, tmp.S, nblk);
  if (per) hipLaunchKernelGGL(spline_periodic_rhs_kernel<T>, dim3(gr), dim3(BLOCK), 0, s, A);
  else hipLaunchKernelGGL((spline_rhs_kernel<T, false>), dim3(gr), dim3(BLOCK), 0, s, A);
  hipLaunchKernelGGL(spline_blocked_local_kernel<T>, dim3(gl), dim3(BLOCK), 0, s, A, 0);
  hipLaunchKernelGGL(spline_blocked_carry_kernel<T>, dim3(grid), dim3(64), 0, s, A, 0);
  hipLaunchKernelGGL(spline_blocked_fix_forward_kernel<T>, dim3(gr), dim3(BLOCK), 0, s, A);
  hipLaunchKernelGGL(spline_blocked_local_kernel<T>, dim3(gl), dim3(BLOCK), 0, s, A, 1);
  hipLaunchKernelGGL(spline_blocked_carry_kernel<T>, dim3(grid), dim3(64), 0, s, A, 1);
  if (per) {
    hipLaunchKernelGGL(spline_periodic_km1_kernel<T>, dim3(grid), dim3(64), 0, s, A);
    hipLaunchKernelGGL(spline_periodic_finish_kernel<T>, dim3(gr), dim3(BLOCK), 0, s, A);
  } else {
    hipLaunchKernelGGL(spline_blocked_finish_kernel<T>, dim3(gr), dim3(BLOCK), 0, s, A);
  }
  NDI_HIP(hipGetLastError());
  if (per) NDI_HIP(hipMemcpy(&hs, tmp.p, sizeof(hs), hipMemcpyDeviceToHost));   // (only the periodic build reports through it)
  else NDI_HIP(hipStreamSynchronize(s));                                         // the tables are complete on return
}

// The serial kernels, one lane per thread, by the system's mode; the status read-back synchronises.
template <class T>
static void build_serial(int spline_mode, const BuildArgs<T>& A, const BuildTemp<T>& tmp, StatusBlock& hs) {
  const uint64_t n = A.n, lanes = A.lanes;
  const unsigned grid = build_lane_grid(lanes);
  hipStream_t s = nullptr;
  switch (spline_mode) {
    case SPLINE_GENERAL: {
      // Wide trailing axes: four waves per 64 lanes, the right-hand sides never leave the chip (spline_build_wide_kernel).
      // NDI_SPLINE_WIDE=0 / 1: A/B (1 takes it for every width).
      static const Knob wide_knob{"NDI_SPLINE_WIDE", -1, Knob::live};
      const int wide_env = wide_knob.get();
      if (!A.kout && n >= 4 && (wide_env > 0 || (wide_env < 0 && lanes >= 1024))) {
        constexpr int RW = 16, RBW = 3 * RW;       // rows per producer wave / per block
        const size_t shm = (size_t)(4 * RBW * 64 + 2 * 4 * RBW) * sizeof(T);
        auto kern = spline_build_wide_kernel<T, RW>;
        allow_dynamic_lds(reinterpret_cast<const void*>(kern), (int)shm);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), shm, s, A);
        break;
      }
      hipLaunchKernelGGL((spline_rhs_kernel<T, false>), dim3(build_rows_grid(n, lanes)), dim3(BLOCK), 0, s, A);
      launch_build_general<T, false, false>(A);
      break;
    }
    case SPLINE_PARABOLA3:
      hipLaunchKernelGGL(spline_build_n3_kernel<T>, dim3(grid), dim3(64), 0, s, A, 0);
      break;
    case SPLINE_PERIODIC3:
      hipLaunchKernelGGL(spline_build_n3_kernel<T>, dim3(grid), dim3(64), 0, s, A, 1);
      break;
    case SPLINE_PERIODIC:
      hipLaunchKernelGGL(spline_build_periodic_kernel<T>, dim3(grid), dim3(64), 0, s, A);
      break;
  }
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipMemcpy(&hs, tmp.p, sizeof(hs), hipMemcpyDeviceToHost));  // synchronises
}

// BoundaryCondition::Individual (cubic_spline.rs:332-347 + solve_for_k_individual :370-403): one scalar
// solve per trailing element in the reference; here every lane picks its end kinds / values and one of
// the precomputed elimination plans (4 left kinds x 4 right kinds, kind 3 = the n == 3 parabola rows).
template <class T>
static ndi_status build_spline_individual(Interp1DImpl<T>& h, const ndi_interp1d_desc& d) {
  const uint64_t n = h.n, lanes = h.lanes;
  const T* x = h.pyr.host_knots.data();
  std::vector<uint8_t> cls(lanes);
  std::vector<T> lval(lanes), rval(lanes);
  for (uint64_t l = 0; l < lanes; ++l) {
    int lk, rk;
    double lv, rv;
    specialize_end(d.lane_left_kind[l], d.lane_left_value[l], lk, lv);
    specialize_end(d.lane_right_kind[l], d.lane_right_value[l], rk, rv);
    if (n == 3 && lk == END_NOT_A_KNOT && rk == END_NOT_A_KNOT) lk = rk = 3;  // :569-596
    cls[l] = (uint8_t)(lk | (rk << 2));
    lval[l] = T(lv);
    rval[l] = T(rv);
  }
  static const int to_ndi[3] = {NDI_BC_NOT_A_KNOT, NDI_BC_FIRST_DERIV, NDI_BC_SECOND_DERIV};
  std::vector<T> w4(4 * n, T(0)), midp4(4 * n, T(1)), up0_4(4, T(0)), wl(16, T(0)), midl(16, T(1));
  SplinePlan<T> ref;
  for (int lk = 0; lk < 3; ++lk)
    for (int rk = 0; rk < 3; ++rk) {
      SplinePlan<T> P = make_spline_plan<T>(x, n, false, to_ndi[lk], 0.0, to_ndi[rk], 0.0);
      int a = lk, b = rk;
      if (P.mode == SPLINE_PARABOLA3) a = b = 3;
      for (uint64_t i = 0; i + 1 < n; ++i) {
        w4[a * n + i] = P.w[i];
        midp4[a * n + i] = P.midp[i];
      }
      up0_4[a] = P.up[0];
      wl[a * 4 + b] = P.w[n - 1];
      midl[a * 4 + b] = P.midp[n - 1];
      if (lk == 2 && rk == 2) ref = P;  // a general-mode plan: shared dx / interior up / not-a-knot scalars
      if (P.mode != SPLINE_PARABOLA3 && lk == 0) { ref.nkL_tmp1 = P.nkL_tmp1; ref.nkL_d = P.nkL_d; }
      if (P.mode != SPLINE_PARABOLA3 && rk == 0) { ref.nkR_tmp1 = P.nkR_tmp1; ref.nkR_d = P.nkR_d; }
    }
  {  // not-a-knot row scalars depend on x only; take them from plans that have them (n == 3 included)
    SplinePlan<T> PL = make_spline_plan<T>(x, n, false, NDI_BC_NOT_A_KNOT, 0.0, NDI_BC_FIRST_DERIV, 0.0);
    SplinePlan<T> PR = make_spline_plan<T>(x, n, false, NDI_BC_FIRST_DERIV, 0.0, NDI_BC_NOT_A_KNOT, 0.0);
    ref.nkL_tmp1 = PL.nkL_tmp1; ref.nkL_d = PL.nkL_d;
    ref.nkR_tmp1 = PR.nkR_tmp1; ref.nkR_d = PR.nkR_d;
  }
  reserve_tables(h);
  std::vector<T> pack;
  auto put = [&pack](const std::vector<T>& v) { size_t o = pack.size(); pack.insert(pack.end(), v.begin(), v.end()); return o; };
  const size_t o_dx = put(ref.dx), o_up = put(ref.up), o_w4 = put(w4), o_m4 = put(midp4), o_u0 = put(up0_4),
               o_wl = put(wl), o_ml = put(midl), o_lv = put(lval), o_rv = put(rval);
  DevBuf plan, dcls;
  plan.reserve(pack.size() * sizeof(T));
  NDI_HIP(hipMemcpy(plan.p, pack.data(), pack.size() * sizeof(T), hipMemcpyHostToDevice));
  dcls.reserve(lanes);
  NDI_HIP(hipMemcpy(dcls.p, cls.data(), lanes, hipMemcpyHostToDevice));
  BuildArgs<T> A = build_args(h, ref);   // (the end kinds and values of `ref` are not read: the lanes bring their own)
  const T* base = plan.as<T>();
  A.dx = base + o_dx; A.up = base + o_up; A.w = base + o_w4; A.midp = base + o_m4;
  A.w4 = base + o_w4; A.midp4 = base + o_m4; A.up0_4 = base + o_u0; A.wl = base + o_wl; A.midl = base + o_ml;
  A.lane_lval = base + o_lv; A.lane_rval = base + o_rv;
  A.lane_cls = dcls.as<uint8_t>();
  hipLaunchKernelGGL((spline_rhs_kernel<T, true>), dim3(build_rows_grid(n, lanes)), dim3(BLOCK), 0, (hipStream_t) nullptr, A);
  A.kout = h.reserve_k();
  launch_build_general<T, true, false>(A);
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipDeviceSynchronize());
  return NDI_OK;
}

// ---- build (CubicSpline::build, cubic_spline.rs:754-771) --------------------------------
template <class T>
ndi_status Interp1DImpl<T>::build_spline(const ndi_interp1d_desc& d) {
  Range rg("ndi:spline_build");
  const bool per_lane = d.lane_left_kind || d.lane_left_value || d.lane_right_kind || d.lane_right_value;
  if (per_lane) {
    if (!(d.lane_left_kind && d.lane_left_value && d.lane_right_kind && d.lane_right_value))
      return fail(NDI_BAD_ARG, "BoundaryCondition::Individual needs all four lane_* arrays");
    if (d.periodic) return fail(NDI_BAD_ARG, "Periodic cannot be combined with per-lane boundaries");
    return build_spline_individual(*this, d);
  }
  const bool periodic = d.periodic != 0;
  BuildClock clk;
  reserve_tables(*this);
  const BuildForm form = build_form(*this, d);
  SplineEnds<T> ends;
  SplinePlan<T> P = form.dev_elim ? make_spline_plan_scalars<T>(pyr.host_knots.data(), n, d.left.kind, d.left.value, d.right.kind,
                                                                d.right.value, ends)
                                  : make_spline_plan<T>(pyr.host_knots.data(), n, periodic, d.left.kind, d.left.value,
                                                        d.right.kind, d.right.value, (d.build_flags & BUILD_TRUE_NOT_A_KNOT) != 0);
  clk.mark("  host plan");
  if (P.mode == SPLINE_GENERAL && !form.blocked && (uint64_t)n * lanes <= (1u << 17)) return build_small_fused(*this, P, clk);
  const BuildTemp<T> tmp(*this, P.mode == SPLINE_PERIODIC, form.blocked);
  upload_plan(*this, P, ends, form.dev_elim, tmp);
  clk.mark("  tables alloc + plan upload");
  BuildArgs<T> A = build_args(*this, P);
  tmp.plan_into(A);
  A.kout = reserve_k();
  StatusBlock hs{};
  if (form.blocked) {
    build_blocked(A, tmp, P.mode == SPLINE_PERIODIC, hs);
    clk.mark("  blocked sweeps");
  } else {
    build_serial(P.mode, A, tmp, hs);
  }
  return periodic_verdict(*this, hs, periodic);
}

// ---- build of the local cubics: Pchip, Akima, CubicHermite (hermite_kernels.hpp) -----------------------
// One launch, no host plan, no temporaries: the knots are the pyramid's level 0, already resident.  `dydx` (HR_GIVEN):
// the caller's derivatives in `memspace`.  Like the spline build it runs on the NULL stream and the tables are complete
// when create returns.
template <int RULE, class T>
static void launch_hermite(const HermiteArgs<T>& A, bool vec) {
  constexpr int VN = Wide<T>::N;
  const uint64_t total = (A.n - 1) * (vec ? A.lanes / VN : A.lanes);
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
  pick_or<1, VN>(vec ? VN : 1, [&](auto vn_) {
    hipLaunchKernelGGL((hermite_build_kernel<T, RULE, vn_>), dim3(grid), dim3(BLOCK), 0, (hipStream_t) nullptr, A);
  });
}

template <class T>
ndi_status Interp1DImpl<T>::build_hermite(const void* dydx, int memspace) {
  Range rg("ndi:hermite_build");
  reserve_tables(*this);
  HermiteArgs<T> A{};
  A.data = data.as<T>();
  A.x = pyr.view.lv0;
  A.ca = ca.as<T>();
  A.cb = cb.as<T>();
  A.n = n;
  A.lanes = lanes;
  A.kout = reserve_k();
  DevBuf tmp;
  if (rule == HR_GIVEN) {
    if (memspace == NDI_MEM_DEVICE) {
      A.dydx = static_cast<const T*>(dydx);
    } else {   // host derivatives: uploaded into the kept k table where there is one, else into a temporary
      T* dst = A.kout;
      if (!dst) {
        tmp.reserve((size_t)n * lanes * sizeof(T));
        dst = tmp.as<T>();
      }
      NDI_HIP(hipMemcpy(dst, dydx, (size_t)n * lanes * sizeof(T), hipMemcpyHostToDevice));
      A.dydx = dst;
      A.kout = nullptr;
    }
  }
  const bool vec = lanes % Wide<T>::N == 0 && aligned16(A.data) && aligned16(A.ca) && aligned16(A.cb) && aligned16(A.kout) &&
                   aligned16(A.dydx);
  if (rule == HR_PCHIP) launch_hermite<HR_PCHIP>(A, vec);
  else if (rule == HR_AKIMA) launch_hermite<HR_AKIMA>(A, vec);
  else launch_hermite<HR_GIVEN>(A, vec);
  NDI_HIP(hipGetLastError());
  NDI_HIP(hipStreamSynchronize(nullptr));   // the tables are complete when create() returns: any stream may read them
  return NDI_OK;
}
