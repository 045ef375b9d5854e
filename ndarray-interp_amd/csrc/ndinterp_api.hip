// csrc/ndinterp_api.hip -- the extern "C" surface of libndinterp_hip.so (include/ndinterp.h).
//
// Host side of the drop-in boundary: owns the device copies of knots / data / spline tables,
// validates like the reference's builders, sequences the kernels of kernels.hpp on a HIP stream
// and translates the device status word into the reference's error values.
// There is deliberately NO CPU evaluation path in this library.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <shared_mutex>
#include <stdexcept>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "common.hpp"
#include "../../include/ndinterp3d_cubic.h"
#include "host_logic.hpp"
#include "kernels.hpp"
#include "hermite_kernels.hpp"
#include "derivative_kernels.hpp"
#include "antiderivative_kernels.hpp"
#include "inverse_kernels.hpp"
#include "lanewise_kernels.hpp"
#include "lane_axes_kernels.hpp"
#include "bicubic_kernels.hpp"
#include "bicubic_local_kernels.hpp"
#include "bicubic_integral_kernels.hpp"
#include "bicubic_jet_kernels.hpp"
#include "lanewise2d_kernels.hpp"
#include "trilinear_kernels.hpp"
#include "tricubic_kernels.hpp"

#define NDI_API extern "C" __attribute__((visibility("default")))

namespace ndi {

// ---------------------------------------------------------------------------------------------
// small RAII helpers
// ---------------------------------------------------------------------------------------------
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    NDI_HIP(hipGetDevice(&prev));
    if (prev != dev) NDI_HIP(hipSetDevice(dev));
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool owned = true;   // false: a view into another allocation (adopt): released by forgetting it
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p && owned) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    owned = true;
  }
  // A slice of a larger allocation that outlives this buffer (small handles keep all their tables in ONE allocation:
  // every hipMalloc costs as much as the kernels of a small build).  reserve() beyond the slice falls back to an
  // allocation of its own.
  void adopt(void* ptr, size_t nbytes) {
    release();
    p = ptr;
    bytes = nbytes;
    owned = false;
  }
  void reserve(size_t need) {
    if (need <= bytes) return;
    release();
    NDI_HIP(hipMalloc(&p, need));
    bytes = need;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// Device-to-device copy of a replica's tables (ndi_interp{1,2}d_clone).  Between two GPUs that can address each
// other (xGMI peers) it is one hipMemcpyPeer; when hipDeviceCanAccessPeer says no -- or NDI_CLONE_STAGED=1 forces it,
// which is how the 1-GPU test box exercises the path -- the bytes are staged through a pinned host buffer in
// 64 MiB pieces (device -> host on the source device, host -> device on the destination).
static void copy_across_devices(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes) {
  if (bytes == 0) return;
  const char* force = std::getenv("NDI_CLONE_STAGED");   // read per call: a test switches it
  int can = 1;
  if (dst_dev != src_dev) NDI_HIP(hipDeviceCanAccessPeer(&can, dst_dev, src_dev));
  if (can && !(force && force[0] == '1')) {
    NDI_HIP(hipMemcpyPeer(dst, dst_dev, src, src_dev, bytes));
    return;
  }
  constexpr size_t PIECE = 64ull << 20;
  void* pin = nullptr;
  NDI_HIP(hipHostMalloc(&pin, std::min(bytes, PIECE), hipHostMallocPortable));
  struct Free { void* p; ~Free() { (void)hipHostFree(p); } } guard{pin};
  for (size_t off = 0; off < bytes; off += PIECE) {
    const size_t nb = std::min(PIECE, bytes - off);
    {
      DeviceGuard g(src_dev);
      NDI_HIP(hipMemcpy(pin, (const char*)src + off, nb, hipMemcpyDeviceToHost));
    }
    {
      DeviceGuard g(dst_dev);
      NDI_HIP(hipMemcpy((char*)dst + off, pin, nb, hipMemcpyHostToDevice));
    }
  }
}

// Test hook (tests/test_gpu_lazy_tables.py): NDI_TEST_FAIL_LAZY_ALLOC=1 makes the lazily built optional copies (bucket
// indices, interval-packed tables, slope and element records) fail as an out-of-memory hipMalloc would -- the fallbacks
// must serve the batch.
static void maybe_fail_lazy_alloc(int line) {
  const char* e = std::getenv("NDI_TEST_FAIL_LAZY_ALLOC");
  if (e && e[0] == '1') throw HipFailure{hipErrorOutOfMemory, "injected lazy-allocation failure", line};
}

// Workspaces are keyed by (stream, calling thread): work enqueued on one stream is ordered, so a
// thread may reuse its scratch across stream-ordered evaluations, and two host threads that share a
// stream (e.g. the default stream) still get private scratch -- `eval` on one handle is re-entrant.
struct SpaceKey {
  hipStream_t stream;
  std::thread::id tid;
  bool operator<(const SpaceKey& o) const {
    return stream != o.stream ? std::less<hipStream_t>()(stream, o.stream) : tid < o.tid;
  }
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the function on the *current device*: one flag per
// (function, device), and the return code is checked (a process may drive several devices, one handle each).
static void allow_dynamic_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  int dev = 0;
  NDI_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  if (done.count({fn, dev})) return;
  NDI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.insert({fn, dev});
}

// roctx ranges around build / locate / group / evaluate (rocprofv3 --marker-trace).  The marker library is
// resolved at run time and only when NDI_ROCTX=1, so the product has no link-time dependency on a profiler.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char* on = std::getenv("NDI_ROCTX");
    if (!on || on[0] == '0') return;
    void* h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so.4", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
static const Roctx& roctx() {
  static Roctx r;
  return r;
}
struct Range {
  bool on;
  explicit Range(const char* name) : on(roctx().push != nullptr) {
    if (on) roctx().push(name);
  }
  ~Range() {
    if (on) roctx().pop();
  }
};

// ---------------------------------------------------------------------------------------------
// per-kernel event profiling (ndi_profile_*)
// ---------------------------------------------------------------------------------------------
enum ProfCat : int { PC_EVAL = 0, PC_LOCATE = 1, PC_GROUP = 2 };
struct ProfRec { hipEvent_t a, b; int cat; int dev; };
static std::atomic<int> g_prof_on{0};
static std::mutex g_prof_mu;
static std::vector<ProfRec> g_prof_recs;
static ndi_profile g_prof_acc{};
static std::atomic<int> g_last_path{0};

static const char* const PROF_NAMES[3] = {"ndi:evaluate", "ndi:locate", "ndi:group"};
// Timing events are recycled (creating two events per launch costs the host ~0.1 ms per ring step, and the host
// path of chunk 0 is exposed): finished records hand their events back to this pool (g_prof_mu held).  Events
// belong to a device: the pool is keyed by it.
static std::map<int, std::vector<hipEvent_t>> g_prof_pool;
static hipEvent_t prof_event_locked(int dev) {
  auto& pool = g_prof_pool[dev];
  if (!pool.empty()) {
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  NDI_HIP(hipEventCreate(&e));
  return e;
}
struct ProfScope {
  hipStream_t s;
  ProfRec r{};
  int dev = 0;
  bool on;
  Range range;   // host-side enqueue range of the stage (the kernels inside carry their own names)
  ProfScope(hipStream_t stream, int cat) : s(stream), on(g_prof_on.load() != 0), range(PROF_NAMES[cat]) {
    if (!on) return;
    r.cat = cat;
    NDI_HIP(hipGetDevice(&dev));
    {
      std::lock_guard<std::mutex> g(g_prof_mu);
      r.a = prof_event_locked(dev);
      r.b = prof_event_locked(dev);
    }
    r.dev = dev;
    NDI_HIP(hipEventRecord(r.a, s));
  }
  void done() {
    if (!on) return;
    NDI_HIP(hipEventRecord(r.b, s));
    std::lock_guard<std::mutex> g(g_prof_mu);
    g_prof_recs.push_back(r);
    if (g_prof_recs.size() >= 4096) fold_finished_locked();   // profiling left on and never read: stay bounded
  }
  static void account_locked(const ProfRec& r, float ms) {
    if (r.cat == PC_EVAL) { g_prof_acc.eval_launches++; g_prof_acc.eval_ms += ms; }
    else if (r.cat == PC_LOCATE) { g_prof_acc.locate_launches++; g_prof_acc.locate_ms += ms; }
    else { g_prof_acc.group_launches++; g_prof_acc.group_ms += ms; }
  }
  // Adds the records whose kernels have finished to the running totals and recycles their events (g_prof_mu held).
  static void fold_finished_locked() {
    size_t keep = 0;
    for (size_t i = 0; i < g_prof_recs.size(); ++i) {
      ProfRec& r = g_prof_recs[i];
      if (hipEventQuery(r.b) != hipSuccess) {
        (void)hipGetLastError();
        g_prof_recs[keep++] = r;
        continue;
      }
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) account_locked(r, ms);
      g_prof_pool[r.dev].push_back(r.a);
      g_prof_pool[r.dev].push_back(r.b);
    }
    g_prof_recs.resize(keep);
  }
};

// ---------------------------------------------------------------------------------------------
// knot pyramid on the device
// ---------------------------------------------------------------------------------------------
template <class T>
struct DevicePyramid {
  DevBuf buf;
  Pyramid<T> view{};
  std::vector<T> host_knots;
  size_t lds_bytes = 0;

  void upload(const T* knots, uint64_t n) {
    host_knots.assign(knots, knots + n);
    uint32_t block = 1;
    while ((uint64_t)64 * block < n) block *= 2;          // top level <= 64 entries: one per lane
    const uint32_t n1 = (uint32_t)((n + block - 1) / block);
    std::vector<T> all(n + n1);
    std::copy(knots, knots + n, all.begin());
    for (uint32_t j = 0; j < n1; ++j) all[n + j] = knots[(uint64_t)j * block];
    buf.reserve(all.size() * sizeof(T));
    NDI_HIP(hipMemcpy(buf.p, all.data(), all.size() * sizeof(T), hipMemcpyHostToDevice));
    view.lv0 = buf.as<T>();
    view.lv1 = view.lv0 + n;
    view.n = (uint32_t)n;
    view.n1 = n1;
    view.block = block;
    view.levels = (n <= 64) ? 1 : 2;
    // evenly spaced within less than half a step everywhere -> the reference's O(1) guess will mostly be right
    bool even = n >= 2;
    const double step = ((double)knots[n - 1] - (double)knots[0]) / (double)(n - 1);
    for (uint64_t i = 0; even && i < n; ++i)
      even = std::fabs((double)knots[i] - ((double)knots[0] + step * (double)i)) < 0.45 * step;
    view.guess = even ? 1 : 0;
    lds_bytes = all.size() * sizeof(T);
    // Is the formula guess right for EVERY x (then no bucket index is needed)?  The guess is monotone in x, so it is
    // enough that it maps every knot k[i] and the last value before k[i+1] to i (same T arithmetic as locate_index).
    bool exact = even;
    if (exact) {
      const T k0 = knots[0], kn = knots[n - 1];
      auto guess = [&](T x) -> uint64_t {
        const T m = (T(n - 1u) - T(0)) / (kn - k0) * (x - k0) + T(0);
        return (m >= T(0)) ? (uint64_t)(m < T(n - 2u) ? m : T(n - 2u)) : 0u;
      };
      for (uint64_t i = 0; exact && i + 1 < n; ++i)
        exact = guess(knots[i]) == std::min<uint64_t>(i, n - 2) &&
                guess(std::nextafter(knots[i + 1], knots[i])) == std::min<uint64_t>(i, n - 2);
    }
    guess_is_exact = exact;
  }

  // The bucket index is built on first use by a batch large enough to use it (>= 4096 queries): one-shot searches
  // and latency-bound small batches never pay for it.
  bool guess_is_exact = false;
  mutable std::once_flag lut_once;
  // A build that fails (out of device memory, a copy refused during stream capture) leaves the axis without the
  // index: the pyramid search serves every batch as before -- nothing is thrown out of call_once, no later call
  // retries, no evaluation fails because an optional accelerator could not be built.
  void ensure_bucket_index() const {   // lazily built cache: logically const
    std::call_once(lut_once, [this] {
      DevicePyramid* self = const_cast<DevicePyramid*>(this);
      try {
        maybe_fail_lazy_alloc(__LINE__);
        self->build_bucket_index(host_knots.data(), host_knots.size(), guess_is_exact);
      } catch (const HipFailure&) {
        (void)hipGetLastError();
        self->bidx = BucketIndex<T>{nullptr, 0, T(0)};
        self->lut_bytes = 0;
        self->lut_buf.release();
      }
    });
  }

  // The global-memory form for axes that are not staged in LDS (kernels.hpp, BucketIndex32): u32 entries, 2n <= m < 4n
  // buckets, at most 256 MiB.  Built on first use by a batch of >= 4096 queries.
  DevBuf lut32_buf;
  BucketIndex32<T> bidx32{nullptr, 0, T(0)};
  mutable std::once_flag lut32_once;
  void ensure_bucket_index32() const {
    std::call_once(lut32_once, [this] {
      DevicePyramid* self = const_cast<DevicePyramid*>(this);
      const T* knots = host_knots.data();
      const uint64_t n = host_knots.size();
      if (guess_is_exact || n <= 64 || n > (1ull << 25)) return;
      uint32_t m = 1;
      while (m < 2 * n) m *= 2;
      const T k0 = knots[0], kn = knots[n - 1];
      const T scale = T(m) / (kn - k0);
      if (!(scale > T(0)) || !std::isfinite((double)scale)) return;
      std::vector<uint32_t> lut((size_t)m + 2, 0);
      for (uint64_t i = 0; i < n; ++i) lut[bucket_of<T>(knots[i], k0, scale, m) + 1]++;   // counts, shifted by one
      for (uint32_t b = 0; b < m; ++b) lut[b + 1] += lut[b];                              // lut[b] = knots in buckets < b
      lut[m + 1] = (uint32_t)n;
      try {   // (failure: no index, the pyramid search from memory serves the axis -- see ensure_bucket_index)
        maybe_fail_lazy_alloc(__LINE__);
        self->lut32_buf.reserve(lut.size() * sizeof(uint32_t));
        NDI_HIP(hipMemcpy(self->lut32_buf.p, lut.data(), lut.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        self->bidx32 = BucketIndex32<T>{self->lut32_buf.template as<uint32_t>(), m, scale};
      } catch (const HipFailure&) {
        (void)hipGetLastError();
        self->bidx32 = BucketIndex32<T>{nullptr, 0, T(0)};
        self->lut32_buf.release();
      }
    });
  }

  // Dense bucket index of the query-per-lane kernels (kernels.hpp, DenseLut): so many uniform buckets that none holds
  // more than `maxk` knots -- the device then counts lut[bucket] + (the next maxk knots <= x) without a loop whose trip
  // count depends on the data.  4n buckets to start with, doubled until maxk <= 3 or the index would outgrow 64 KiB of
  // LDS; accepted up to maxk = 8 (clustered axes beyond that keep the other kernels).  Axes whose formula guess is exact
  // need no index.  Built on first use with the device's arithmetic; a failed build leaves dense_ok = false.
  DevBuf dlut_buf;
  DenseLut<T> dlut{nullptr, 0, 0, T(0)};
  size_t dlut_bytes = 0;   // LDS bytes of the staged index (16-byte multiple); 0 = none
  bool dense_ok = false;
  mutable std::once_flag dlut_once;
  void ensure_dense_lut() const {
    std::call_once(dlut_once, [this] {
      DevicePyramid* self = const_cast<DevicePyramid*>(this);
      const T* knots = host_knots.data();
      const uint64_t n = host_knots.size();
      if (n < 2) return;
      if (guess_is_exact) { self->dense_ok = true; return; }
      if (n > 16384) return;
      const T k0 = knots[0], kn = knots[n - 1];
      uint32_t m = 64;
      while (m < 4 * n) m *= 2;
      std::vector<uint32_t> cnt;
      // candidates m = 4n .. 32768 (64 KiB of LDS): the smallest index with one knot per bucket if that costs at most
      // 16 KiB, else the smallest with <= 3, else the densest (accepted up to 8)
      uint32_t best_m = 0, best_k = 0;
      T best_scale = T(0);
      uint32_t m1 = 0, m3 = 0, ml = 0, kl = 0;
      T s1 = T(0), s3 = T(0), sl = T(0);
      for (; m <= 32768; m *= 2) {
        const T scale = T(m) / (kn - k0);
        if (!(scale > T(0)) || !std::isfinite((double)scale)) break;
        cnt.assign(m, 0);
        uint32_t mk = 0;
        for (uint64_t i = 0; i < n; ++i) {
          T f = (knots[i] - k0) * scale;
          f = std::fmax(f, T(0));
          f = std::fmin(f, T(m - 1u));
          mk = std::max(mk, ++cnt[(uint32_t)f]);
        }
        ml = m; kl = mk; sl = scale;
        if (!m3 && mk <= 3) { m3 = m; s3 = scale; }
        if (!m1 && mk <= 1 && m <= 8192) { m1 = m; s1 = scale; }
        if (m1 || (m3 && m >= 8192)) break;
      }
      if (m1) { best_m = m1; best_k = 1; best_scale = s1; }
      else if (m3) { best_m = m3; best_k = 3; best_scale = s3; }
      else { best_m = ml; best_k = kl; best_scale = sl; }
      if (!best_m || best_k > 8) return;
      const T scale = best_scale;
      m = best_m;
      cnt.assign(m, 0);
      best_k = 0;
      for (uint64_t i = 0; i < n; ++i) {
        T f = (knots[i] - k0) * scale;
        f = std::fmax(f, T(0));
        f = std::fmin(f, T(m - 1u));
        best_k = std::max(best_k, ++cnt[(uint32_t)f]);
      }
      std::vector<uint16_t> lut((size_t)m + 2 + 6, (uint16_t)n);
      uint32_t run = 0;
      for (uint32_t b = 0; b < m; ++b) {
        lut[b] = (uint16_t)run;
        run += cnt[b];
      }
      const size_t bytes = (((size_t)(m + 2) / 2) * 4 + 15) & ~(size_t)15;
      try {
        maybe_fail_lazy_alloc(__LINE__);
        self->dlut_buf.reserve(std::max(bytes, lut.size() * sizeof(uint16_t)));
        NDI_HIP(hipMemcpy(self->dlut_buf.p, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      } catch (const HipFailure&) {
        (void)hipGetLastError();
        self->dlut_buf.release();
        return;
      }
      self->dlut = DenseLut<T>{self->dlut_buf.template as<uint16_t>(), m, best_k, scale};
      self->dlut_bytes = bytes;
      self->dense_ok = true;
    });
  }

  // Bucket index (kernels.hpp, BucketIndex): only for axes the O(1) formula guess does not resolve for every x, with
  // u16 entries (n <= 65535) and more than one top-level block.  Built with bucket_of(), the function the device uses.
  DevBuf lut_buf;
  BucketIndex<T> bidx{nullptr, 0, T(0)};
  size_t lut_bytes = 0;   // LDS bytes of the staged lut (16-byte multiple); 0 = none
  void build_bucket_index(const T* knots, uint64_t n, bool guess_is_exact) {
    bidx = BucketIndex<T>{nullptr, 0, T(0)};
    lut_bytes = 0;
    if (guess_is_exact || n <= 64 || n > 65535) return;
    uint32_t m = 1;
    while (m < 2 * n) m *= 2;                       // 2n <= m < 4n buckets
    const T k0 = knots[0], kn = knots[n - 1];
    const T scale = T(m) / (kn - k0);
    if (!(scale > T(0)) || !std::isfinite((double)scale)) return;   // degenerate span: keep the pyramid search
    std::vector<uint16_t> lut(m + 2 + 6, 0);        // m + 1 entries, padded to a whole number of 16-byte units
    std::vector<uint32_t> cnt(m, 0);
    for (uint64_t i = 0; i < n; ++i) cnt[bucket_of<T>(knots[i], k0, scale, m)]++;
    uint32_t run = 0;
    for (uint32_t b = 0; b < m; ++b) {
      lut[b] = (uint16_t)run;
      run += cnt[b];
    }
    for (size_t b = m; b < lut.size(); ++b) lut[b] = (uint16_t)n;   // lut[m] = n; padding likewise
    const size_t bytes = (((size_t)(m + 2) / 2) * 4 + 15) & ~(size_t)15;
    lut_buf.reserve(std::max(bytes, lut.size() * sizeof(uint16_t)));
    NDI_HIP(hipMemcpy(lut_buf.p, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    bidx = BucketIndex<T>{lut_buf.as<uint16_t>(), m, scale};
    lut_bytes = bytes;
  }
};

constexpr uint64_t MAX_KNOTS = (1ull << 31) - 1;          // interval indices are 32-bit
constexpr size_t LDS_STAGE_LIMIT = 150 * 1024;          // of the CU's 160 KiB
constexpr size_t FUSED_LDS_LIMIT = 160 * 1024;          // eval_fused_kernel with the tables in LDS: all of it

// ---------------------------------------------------------------------------------------------
// workspace: per (handle, stream) scratch, reused across stream-ordered evaluations
// ---------------------------------------------------------------------------------------------
// One set of per-chunk scratch: what the locate / group kernels of a chunk write and its evaluation reads.  A
// workspace carries MAX_SETS of them (buffers are allocated on first use; every path but the ring uses set 0 -- the
// antiderivative pair also set 1): the ring evaluation locates + groups the next chunks on a side stream while the
// previous ones are being evaluated, chunk k in set k mod 2W for a group width of W (a set is handed back by its
// eval_done event).
struct Scratch {
  DevBuf idx, idx2, t, perm, counts, cursor, hist, status, recq, chunkbin;
  DevBuf perm2, recq2, chist, cursor2;   // two-level 2-D grouping: coarse-ordered records, row histograms, consumable cursors
  hipEvent_t prep_done = nullptr, eval_done = nullptr;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    if (prep_done) (void)hipEventDestroy(prep_done);
    if (eval_done) (void)hipEventDestroy(eval_done);
  }
  void ensure_events() {
    if (!prep_done) NDI_HIP(hipEventCreateWithFlags(&prep_done, hipEventDisableTiming));
    if (!eval_done) NDI_HIP(hipEventCreateWithFlags(&eval_done, hipEventDisableTiming));
  }
};

struct Workspace {
  static constexpr uint32_t MAX_SETS = 8;
  Scratch sc[MAX_SETS];
  DevBuf status, qdev, qdev2, stage;   // status: the range pre-pass of the ring / sharded evaluations
  StatusBlock* host_status = nullptr;  // pinned
  void* pin = nullptr;                 // pinned bounce buffer of the small-batch host path
  void* pin_dev = nullptr;             // its device-side address (hipHostGetDevicePointer)
  size_t pin_bytes = 0;
  hipStream_t side = nullptr;          // ring evaluation: locate + group of the next chunk run here
  hipEvent_t ev = nullptr;             // general-purpose ordering event (timing disabled)
  // record of the last batch (for finish())
  uint64_t last_nq = 0;
  const void* last_q = nullptr;
  const void* last_q2 = nullptr;
  int last_q_space = NDI_MEM_DEVICE;
  bool pending = false;
  // SpaceSet bookkeeping (guarded by the set's mutex)
  int users = 0;
  uint64_t last_use = 0;
  ~Workspace() {
    if (side) (void)hipStreamDestroy(side);   // waits for the stream's work
    if (ev) (void)hipEventDestroy(ev);
    if (host_status) (void)hipHostFree(host_status);
    if (pin) (void)hipHostFree(pin);
  }
  void ensure_pin(size_t need) {
    if (need <= pin_bytes) return;
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    pin_dev = nullptr;
    pin_bytes = 0;
    NDI_HIP(hipHostMalloc(&pin, need, hipHostMallocMapped | hipHostMallocPortable));
    NDI_HIP(hipHostGetDevicePointer(&pin_dev, pin, 0));   // the address kernels use for the zero-copy path
    pin_bytes = need;
  }
  template <class U>
  U* pin_device(const void* host_ptr) const {   // device view of an address inside the pinned buffer
    return reinterpret_cast<U*>((char*)pin_dev + ((const char*)host_ptr - (const char*)pin));
  }
  void ensure_status() {
    status.reserve(sizeof(StatusBlock));
    for (int i = 0; i < 2; ++i) sc[i].status.reserve(sizeof(StatusBlock));   // (prep() reserves the status of the set it fills)
    if (!host_status) NDI_HIP(hipHostMalloc((void**)&host_status, sizeof(StatusBlock), hipHostMallocDefault));
  }
  hipStream_t side_stream() {
    if (!side) {   // highest priority: its small kernels are dispatched ahead of the evaluation's next workgroups
      int lo = 0, hi = 0;
      NDI_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
      NDI_HIP(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, hi));
    }
    return side;
  }
  hipEvent_t order_event() {
    if (!ev) NDI_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return ev;
  }
};

// The scratch sets of one handle.  A set is *idle* when no call is inside it and its last batch has been
// collected (its stream was synchronised after the last kernel that touched the scratch).  At most MAX_IDLE idle
// sets are kept -- thread pools and short-lived streams would otherwise grow the map without bound; the least
// recently used idle set is freed first (hipFree / hipHostFree synchronise, so freeing is safe in any case).
struct SpaceSet {
  static constexpr size_t MAX_IDLE = 16;
  std::mutex mu;
  std::map<SpaceKey, std::unique_ptr<Workspace>> map;
  uint64_t tick = 0;

  Workspace& acquire(hipStream_t s) {
    std::lock_guard<std::mutex> g(mu);
    auto& slot = map[SpaceKey{s, std::this_thread::get_id()}];
    if (!slot) slot.reset(new Workspace());
    slot->users++;
    slot->last_use = ++tick;
    evict_locked(MAX_IDLE);
    return *slot;
  }
  void release(Workspace& w) {
    std::lock_guard<std::mutex> g(mu);
    w.users--;
  }
  void evict_locked(size_t keep) {
    for (;;) {
      size_t idle = 0;
      auto victim = map.end();
      for (auto it = map.begin(); it != map.end(); ++it) {
        if (it->second->users != 0 || it->second->pending) continue;
        ++idle;
        if (victim == map.end() || it->second->last_use < victim->second->last_use) victim = it;
      }
      if (idle <= keep || victim == map.end()) return;
      map.erase(victim);
    }
  }
  void trim() {
    std::lock_guard<std::mutex> g(mu);
    evict_locked(0);
  }
  size_t size() {
    std::lock_guard<std::mutex> g(mu);
    return map.size();
  }
};

struct SpaceLease {
  SpaceSet& set;
  Workspace& ws;
  SpaceLease(SpaceSet& st, hipStream_t s) : set(st), ws(st.acquire(s)) {}
  ~SpaceLease() { set.release(ws); }
  SpaceLease(const SpaceLease&) = delete;
  SpaceLease& operator=(const SpaceLease&) = delete;
};

// A ring of device buffers owned by a handle (ndi_ring_desc::slots == NULL): ONE allocation in which the slots
// are interleaved row by row -- row r of slot s lives at (r * n_slots + s) * row_stride, i.e. the chunk's rows have
// the pitch n_slots * row_stride.  Measured on MI355X (profiles/r02_placement_*.jsonl): the rate at
// which a kernel streams into a 32.8 GB extent depends on where the extent lies in physical memory (slots laid
// out one after the other in one allocation ran 6.1 / 5.9 / 5.6 / 4.7 ms for the same chunk, stable, and the same
// for sequential fills); with the rows of every slot striped over the whole ring each chunk's stream covers the
// ring's full extent and runs at the fast end (4.57-4.77 ms in 8 of 9 processes, < 1 % apart within a ring).
struct OwnedRing {
  std::mutex mu;   // one ring evaluation at a time uses the library-owned ring
  DevBuf buf;
  void ensure(uint32_t n, size_t chunk_rows, size_t stride_bytes) { buf.reserve((size_t)n * chunk_rows * stride_bytes); }
  void clear() { buf.release(); }
};

template <class T, class K, class A>
static void launch1(hipStream_t s, int cat, dim3 grid, dim3 block, size_t shmem, K kernel, const A& args) {
  ProfScope ps(s, cat);
  hipLaunchKernelGGL(kernel, grid, block, shmem, s, args);
  NDI_HIP(hipGetLastError());
  ps.done();
}

// launch1 of a kernel whose dynamic LDS may exceed the 64 KiB default: `limit` is what it is allowed (allow_dynamic_lds).
template <class T, class K, class A>
static void launch_lds(K kernel, size_t limit, hipStream_t s, int cat, dim3 grid, dim3 block, size_t shmem, const A& args) {
  allow_dynamic_lds(reinterpret_cast<const void*>(kernel), (int)limit);
  launch1<T>(s, cat, grid, block, shmem, kernel, args);
}

static void reset_status(void* status, hipStream_t s) {
  // first_fail[0..1] = NO_FAIL (all ones), the rest zero -- ONE launch (two hipMemsetAsync calls cost the host twice
  // the enqueue time of a kernel, and the host path of a 0.8 ms step matters: DESIGN.md 4.4)
  hipLaunchKernelGGL(reset_status_kernel, dim3(1), dim3(1), 0, s, reinterpret_cast<StatusBlock*>(status));
  NDI_HIP(hipGetLastError());
}

constexpr uint32_t BUCKETED_RUN = 1;         // consecutive 128-query chunks per workgroup of eval_bucketed_kernel
                                             // (1 / 4 / 8 / 16 / 32 measured equal within 1 %: tools/sweep_target.py)
constexpr uint32_t GROUP_MAX_BLOCKS = 256;   // query slices of the block-local counting sort (1-D; 2-D default)
constexpr uint32_t GROUP_MAX_BLOCKS_2D = 1024;   // upper limit of NDI_GROUP_BLOCKS for the 2-D tile grouping
// NDI_GROUP_BLOCKS (A/B, read once): fewer, longer slices -- longer runs per (slice, bin) in the record scatter
static uint32_t group_blocks() {
  static const Knob knob{"NDI_GROUP_BLOCKS", 0};
  const int k = knob.get();
  return (uint32_t)(k >= 8 && k <= (int)GROUP_MAX_BLOCKS_2D ? k : (int)GROUP_MAX_BLOCKS);
}
constexpr uint32_t GROUP_MAX_BINS = 16384;   // histogram must fit LDS next to the pyramid

template <class T>
static bool lds_sort_fits(const DevicePyramid<T>& pyr, uint64_t nb) {
  const size_t stage = pyr.lds_bytes <= LDS_STAGE_LIMIT ? ((pyr.lds_bytes + 15) & ~(size_t)15) : 0;
  return nb <= GROUP_MAX_BINS && stage + nb * 4 <= LDS_STAGE_LIMIT;   // (the bucket index is dropped first)
}

// Compute units of the current device (cached per device).
static unsigned cu_count() {
  static std::mutex mu;
  static std::map<int, unsigned> cache;
  int dev = 0;
  NDI_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  int n = 0;
  NDI_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  return cache[dev] = (unsigned)std::max(n, 1);
}

// Workgroups of `tb` threads and `lds` bytes each that a CU holds at once (160 KiB LDS, 32 waves), at least one.
static size_t wgs_per_cu(size_t lds, unsigned tb) {
  return std::max<size_t>(1, std::min<size_t>((160 * 1024) / std::max<size_t>(lds, 1), 32 / (tb / 64)));
}

// Workgroup size for a kernel that needs `lds` bytes per workgroup: as few threads as keep 32 waves on a CU
// (160 KiB LDS, at most 1024 threads per workgroup).
// The grid of a query-order kernel whose workgroups walk the batch: one workgroup per `per_wg` queries, at most `rounds`
// times what the chip holds at once beside `lds` bytes of LDS each.
static unsigned resident_grid(uint64_t nq, uint64_t per_wg, size_t lds, unsigned tb, unsigned rounds = 1) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + per_wg - 1) / per_wg, (uint64_t)cu_count() * wgs_per_cu(lds, tb) * rounds));
}

static unsigned threads_for_lds(size_t lds) {
  unsigned best = 256;
  size_t best_waves = 0;
  for (unsigned threads : {256u, 512u, 1024u}) {
    const size_t waves = wgs_per_cu(lds, threads) * (threads / 64);
    if (waves > best_waves) {
      best_waves = waves;
      best = threads;
    }
  }
  return best;
}

// Launches locate_kernel.  With `hist` the grid is one workgroup per contiguous query slice and each
// leaves its interval histogram in hist[b][nb]; *slice_out / *blocks_out describe the slicing.
template <class T>
static void run_locate(hipStream_t s, const DevicePyramid<T>& pyr, const T* q, uint64_t nq,
                       uint32_t* idx, int64_t* idx64, T* t, unsigned long long* first_fail, int mode,
                       uint32_t* hist = nullptr, uint32_t nb = 0, uint64_t* slice_out = nullptr,
                       uint32_t* blocks_out = nullptr, bool beside_eval = false) {
  LocateArgs<T> A{};
  A.pyr = pyr.view;
  A.q = q;
  A.nq = nq;
  A.idx = idx;
  A.idx64 = idx64;
  A.t = t;
  A.first_fail = first_fail;
  A.mode = mode;
  A.stage_lds = pyr.lds_bytes <= LDS_STAGE_LIMIT ? 1 : 0;
  size_t shmem = A.stage_lds ? ((pyr.lds_bytes + 15) & ~(size_t)15) : 0;
  uint64_t blocks = hist ? std::min<uint64_t>((nq + 2047) / 2048, GROUP_MAX_BLOCKS)
                         : std::min<uint64_t>((nq + 1023) / 1024, 2048);
  blocks = std::max<uint64_t>(blocks, 1);
  A.bx = BucketIndex<T>{nullptr, 0, T(0)};
  // (the bucket index: A/B settled in round 3)
  if (A.stage_lds && nq >= 4096) pyr.ensure_bucket_index();
  if (A.stage_lds && pyr.lut_bytes && nq >= 4096 &&
      shmem + pyr.lut_bytes + (hist ? (size_t)nb * 4 : 0) <= LDS_STAGE_LIMIT) {
    A.bx = pyr.bidx;          // bucket index staged behind the pyramid: [pyramid | lut | histogram]
    shmem += pyr.lut_bytes;
    // staging is the fixed cost of a workgroup now: no more workgroups than the chip holds at once
    const size_t total = shmem + (hist ? (size_t)nb * 4 : 0);
    blocks = std::min<uint64_t>(blocks, (uint64_t)cu_count() * std::max<size_t>(1, (160 * 1024) / total));
  }
  A.bx32 = BucketIndex32<T>{nullptr, 0, T(0)};
  if (!A.stage_lds && nq >= 4096) {
    pyr.ensure_bucket_index32();
    A.bx32 = pyr.bidx32;
  }
  if (hist) shmem += (size_t)nb * 4;
  // beside a running evaluation kernel (ring pipeline) a 4-wave workgroup finds room wherever one evaluation
  // workgroup has retired; the 16-wave one that is best on an idle chip would wait for a quarter of a CU to drain
  const unsigned threads = beside_eval ? 256u : threads_for_lds(shmem);
  uint64_t slice = (nq + blocks - 1) / blocks;
  slice = (slice + threads - 1) / threads * threads;   // whole 64-query batches per wave
  blocks = (nq + slice - 1) / slice;
  A.slice = slice;
  A.hist = hist;
  A.nb = nb;
  if (slice_out) *slice_out = slice;
  if (blocks_out) *blocks_out = (uint32_t)blocks;
  const bool deep = slice / threads >= 16;   // batches per wave: queries of 4 batches requested together only then
  pick_bool(A.stage_lds != 0, [&](auto stage) {
    pick_or<1, LOCATE_QB>(deep ? LOCATE_QB : 1, [&](auto qb) {
      launch_lds<T>(&locate_kernel<T, stage.value, qb.value>, LDS_STAGE_LIMIT, s, PC_LOCATE, dim3((unsigned)blocks), dim3(threads), shmem, A);
    });
  });
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Tuning knobs of the short-row 1-D kernels (tools/short_rows_sweep.py).  Read once -- unless NDI_TUNE_LIVE is set
// when the library is loaded, in which case every evaluation re-reads them (one process then sweeps the variants).
//   NDI_SHORT_MODE   0 = auto, 1 = the two-kernel flat form (locate, then eval_flat_kernel), 2 = fused query order,
//                    3 = grouped (eval_bucketed_short_kernel)
//   NDI_FUSED_UNR    trips issued together by eval_fused_kernel (1 / 2 / 4)
//   NDI_FUSED_TB     its workgroup size (256 / 512 / 1024; 0 = chosen from the LDS footprint)
//   NDI_FUSED_LDS    tables in LDS: -1 = when they fit, 0 = never, 1 = whenever they fit (same as -1; kept for A/B)
//   NDI_FUSED_WGS    workgroups per CU of its grid (0 = default)
//   NDI_SHORT_CQ     grouped records per thread group and pass (16 / 64)
//   NDI_SHORT_ROWB   auto: the grouped form is taken from rows of this many bytes upwards
//   NDI_FUSED_PACK   interval-packed table copy for the fused kernel: -1 = rows shorter than a cache line,
//                    0 = never, 1 = always
// ndi_eval_opts as the entry points take it: defaults for NULL, unknown flag bits and a non-zero `reserved` refused (a
// caller compiled against an older header -- a shorter struct, uninitialised padding -- is told so instead of silently
// selecting an option), and NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED folded into the internal "no range pre-pass" bit.
static ndi_status take_opts(const ndi_eval_opts* opts, ndi_eval_opts& o) {
  o = ndi_eval_opts{};
  if (!opts) return NDI_OK;
  o = *opts;
  constexpr int32_t KNOWN = NDI_EVAL_FRESH_OUTPUT | NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED;
  if (o.flags & ~KNOWN) return fail(NDI_BAD_ARG, "ndi_eval_opts.flags has unknown bits (0x%x): built against another header version?", (unsigned)o.flags);
  if (o.reserved != 0) return fail(NDI_BAD_ARG, "ndi_eval_opts.reserved must be 0 (got %d): built against another header version?", (int)o.reserved);
  if (o.flags & NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED) o.flags |= NDI_EVAL_FRESH_OUTPUT;
  return NDI_OK;
}

struct ShortKnobs {
  int mode, unr, tb, lds, wgs, cq, rowb, pack, maxlv = 256;
};
static ShortKnobs short_knobs() {
  static const Knob mode{"NDI_SHORT_MODE", 0, Knob::live}, unr{"NDI_FUSED_UNR", 2, Knob::live}, tb{"NDI_FUSED_TB", 0, Knob::live},
      lds{"NDI_FUSED_LDS", -1, Knob::live}, wgs{"NDI_FUSED_WGS", 0, Knob::live}, cq{"NDI_SHORT_CQ", 64, Knob::live},
      rowb{"NDI_SHORT_ROWB", 1024, Knob::live}, pack{"NDI_FUSED_PACK", -1, Knob::live};
  return {mode.get(), unr.get(), tb.get(), lds.get(), wgs.get(), cq.get(), rowb.get(), pack.get()};
}

// The ring's locate + group of chunk k + 1 run on a side stream beside chunk k's evaluation (measured against running
// them on the evaluation stream: profiles/r03_ring_overlap.md).
static constexpr bool ring_overlap() { return true; }

// NDI_RING_GROUP: how the ring producer groups the chunks whose slots are free into one evaluation launch (1-D long-row
// bucketed plan; float_host.hpp ring_produce).  0 = one launch per chunk; 1 = full-width groups from the first chunk on;
// 2 = a narrow first launch (chunk 0 alone: only its own search + grouping are exposed), full-width groups after it.
// Read once, or per call under NDI_TUNE_LIVE.
constexpr int RING_GROUP_DEFAULT = 1;
static int ring_group_mode() {
  static const Knob knob{"NDI_RING_GROUP", RING_GROUP_DEFAULT, Knob::live};
  const int m = knob.get();
  return m >= 0 && m <= 2 ? m : RING_GROUP_DEFAULT;
}

static ndi_status check_ring_desc(const ndi_ring_desc* ring, uint64_t lanes, uint64_t* stride) {
  if (!ring || ring->n_slots == 0 || ring->chunk_queries == 0)
    return fail(NDI_BAD_ARG, "ring needs n_slots >= 1 and chunk_queries >= 1");
  *stride = ring->row_stride ? ring->row_stride : lanes;
  if (*stride < lanes) return fail(NDI_BAD_ARG, "ring row_stride (%llu) < lanes (%llu)",
                                   (unsigned long long)*stride, (unsigned long long)lanes);
  if (ring->slots)
    for (uint32_t i = 0; i < ring->n_slots; ++i)
      if (!ring->slots[i]) return fail(NDI_BAD_ARG, "ring slot %u is null", i);
  return NDI_OK;
}

// ---------------------------------------------------------------------------------------------
// the host engine the f32 / f64 handles share (Interp1DImpl, AntiderivImpl, Interp2DImpl below)
// ---------------------------------------------------------------------------------------------
#include "float_host.hpp"

// ---------------------------------------------------------------------------------------------
// Interp1D
// ---------------------------------------------------------------------------------------------
// NDI_BUILD_TIMING=1: wall-clock milestones of create() on stderr (where a build's milliseconds go: tools/build_probe.py)
struct BuildClock {
  bool on;
  std::chrono::steady_clock::time_point t0, last;
  BuildClock() : on(std::getenv("NDI_BUILD_TIMING") != nullptr), t0(std::chrono::steady_clock::now()), last(t0) {}
  void mark(const char* what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[ndi build] %-28s +%8.3f ms  (%8.3f)\n", what,
                 std::chrono::duration<double, std::milli>(now - last).count(),
                 std::chrono::duration<double, std::milli>(now - t0).count());
    last = now;
  }
};

// Temporaries of small builds: one device buffer and one pinned staging buffer per host thread and device, grown on
// demand and kept (a build of (100, 5) spends more time in hipMalloc / hipFree / pageable copies than in its kernel).
// Deliberately never freed: thread-exit and process-exit order against the HIP runtime is not ours to rely on.
struct BuildScratch {
  std::map<int, std::pair<void*, size_t>> dev;   // device ordinal -> (buffer, bytes)
  void* pin = nullptr;
  size_t pin_bytes = 0;
  void* device_buf(int device, size_t need) {
    auto& e = dev[device];
    if (need > e.second) {
      if (e.first) (void)hipFree(e.first);
      e = {nullptr, 0};
      const size_t cap = std::max<size_t>(need, 64 * 1024);
      NDI_HIP(hipMalloc(&e.first, cap));
      e.second = cap;
    }
    return e.first;
  }
  void* pinned(size_t need) {
    if (need > pin_bytes) {
      if (pin) (void)hipHostFree(pin);
      pin = nullptr;
      pin_bytes = 0;
      const size_t cap = std::max<size_t>(need, 64 * 1024);
      NDI_HIP(hipHostMalloc(&pin, cap, hipHostMallocPortable));
      pin_bytes = cap;
    }
    return pin;
  }
};
static BuildScratch& build_scratch() {
  static thread_local BuildScratch* p = nullptr;
  if (!p) p = new BuildScratch();
  return *p;
}

// What makes two handles replicas of ONE interpolator beyond element type and lanes: knot count and values,
// strategy, extrapolation mode.  (Data and coefficient tables live on the devices and are not compared.)
static uint64_t fnv1a(uint64_t h, const void* p, size_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}
constexpr uint64_t FNV_SEED = 0xcbf29ce484222325ull;

struct Interp1DBase {
  virtual ~Interp1DBase() = default;
  virtual uint64_t signature() const = 0;
  int dtype = 0, device = 0;
  uint64_t lanes = 0;
  virtual ndi_status eval(const void* q, uint64_t nq, void* out, uint64_t out_stride,
                          const ndi_eval_opts* opts, ndi_oob_info* info) = 0;
  virtual ndi_status finish(void* stream, ndi_oob_info* info) = 0;
  virtual ndi_status coefficients(void* a_out, void* b_out, int memspace) = 0;
  virtual ndi_status eval_ring(const void* q, uint64_t nq, const ndi_ring_desc* ring, ndi_ring_consumer consume,
                               void* user, const ndi_eval_opts* opts, ndi_oob_info* info) = 0;
  virtual ndi_status trim() = 0;
  virtual uint64_t scratch_sets() = 0;
  virtual ndi_status clone_to(int dev, Interp1DBase** out) = 0;
  // ndi_interp1d_derivative: the refusals come before any device work
  virtual ndi_status derivative(int nu, Interp1DBase** out) = 0;
  // ndi_interp1d_data: the resident data table T[n * lanes]
  virtual ndi_status data_table(void* data_out, int memspace) = 0;
  // ndi_interp1d_antiderivative: the refusals come before any device work
  virtual ndi_status antiderivative(Interp1DBase** out) = 0;
  virtual bool is_antiderivative() const { return false; }
  // ndi_interp1d_integrate: antiderivative handles only
  virtual ndi_status integrate(const void* lo, const void* hi, uint64_t nq, void* out, uint64_t out_stride,
                               const ndi_eval_opts* opts, ndi_oob_info* info) {
    return fail(NDI_BAD_ARG, "integrate takes an antiderivative handle (ndi_interp1d_antiderivative of this handle)");
  }
  // ndi_interp1d_inverse: the refusals come before any device work
  virtual ndi_status inverse(Interp1DBase** out) = 0;
  bool inverse_handle = false;   // an inverse handle (inverse_host.hpp): its queries are values, its rows abscissae
  bool lane_axes_handle = false; // a handle with an x axis per lane (lane_axes_host.hpp)
  // ndi_interp1d_eval_lanewise (lanewise_host.hpp): f32 / f64 handles only
  virtual ndi_status eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                                   const ndi_eval_opts* opts, ndi_oob_info* info) {
    return fail(NDI_BAD_ARG, "eval_lanewise: %s handle is a Linear interpolator of a narrow element type; the lane-wise "
                "evaluation takes f32 / f64 handles", (dtype == NDI_I32 || dtype == NDI_I64) ? "an integer" : "an f16 / bf16");
  }
};

// The element-record copy of a Linear / cubic handle's tables for the lane-wise evaluation (lanewise_kernels.hpp), built on
// first use; a replica builds its own, trim releases it.
struct LanewiseRecords {
  static constexpr size_t LIMIT = 1ull << 30;   // the copy's memory cap: above it the plain tables serve
  DevBuf buf;
  // 0 = not tried, 1 = ready and known complete, 2 = unavailable (above the cap / allocation failed), 3 = built by a kernel
  // enqueued on `stream`, completion signalled by `ev`
  std::atomic<int> state{0};
  std::mutex build;            // the state machine
  std::shared_mutex use;       // shared: a call between taking the pointer and its launch; exclusive: drop
  hipEvent_t ev = nullptr;
  hipStream_t stream = nullptr;
  ~LanewiseRecords() {
    if (ev) (void)hipEventDestroy(ev);
  }
  void drop() {   // (hipFree waits for the kernels that read the copy)
    std::unique_lock<std::shared_mutex> u(use);
    std::lock_guard<std::mutex> g(build);
    buf.release();
    state.store(0, std::memory_order_release);
  }
};

static const char* hermite_rule_name(int rule) {
  switch (rule) {
    case HR_SPLINE: return "CubicSpline";
    case HR_PCHIP: return "Pchip";
    case HR_AKIMA: return "Akima";
    case HR_GIVEN: return "CubicHermite";
  }
  return "?";
}

// What Interp1DImpl::prep decides for a batch and launch_eval runs (both in interp1d_host.hpp): the kind and its launch geometry.
template <class T>
struct Plan1 {
  enum Kind { SMALL, BUCKETED, ROWS, FLAT, FUSED, BUCKETED_SHORT, LANES } kind = ROWS;
  const T* q = nullptr;
  uint64_t nq = 0;
  T* out = nullptr;
  uint64_t out_stride = 0;
  bool vec_ok = false;
  uint64_t LV = 0;
  // FUSED (eval_fused_kernel)
  bool f_lut = false, f_pack = false;
  bool f_sorted = false;   // FUSED: the queries of a workgroup round ordered by interval in LDS (eval_fused_sorted_kernel)
  int f_tlds = 0;   // 0: tables from memory, 1: {y, a, b} in LDS, 2: {y, k} in LDS
  unsigned f_tb = 256, f_grid = 1;
  int f_unr = 2;
  size_t f_lds = 0;
  int s_cq = 64;   // BUCKETED_SHORT
  int l_qpl = 1;   // LANES, scalar data: queries per lane (1, or one 16-byte vector)
  bool l_check = false;   // LANES: no range pre-pass, the kernel checks the queries itself (NDI_EVAL_FRESH_OUTPUT)
};

template <class T>
struct Interp1DImpl final : Interp1DBase, FloatEngine<T, Interp1DImpl<T>> {
  int strategy = NDI_LINEAR;   // the evaluation class: NDI_CUBIC_SPLINE = "has a / b tables" (Pchip, Akima, CubicHermite too)
  int strat() const { return strategy == NDI_CUBIC_SPLINE ? ST_CUBIC : ST_LINEAR; }   // ... as the kernels' STRAT
  int rule = HR_SPLINE;        // ... and which rule chose the knot derivatives behind those tables (HermiteRule)
  int deriv = 0;               // derivative order: 0 = the interpolant; 1, 2 = ndi_interp1d_derivative of a handle of `rule`
  int mode = EX_NO;
  uint64_t n = 0;
  DevBuf arena;  // small handles: ONE allocation behind pyr.buf / data / ca / cb / ck (create1d); declared first: freed last
  DevicePyramid<T> pyr;
  DevBuf data, ca, cb;
  DevBuf ck;   // the spline's derivatives k [n][lanes]: kept by builds whose {y, k} fit LDS (eval_fused_kernel, TLDS == 2)
  SpaceSet spaces;
  OwnedRing ring_own;
  // interval-packed copy of the tables for rows shorter than a cache line (pack_intervals_kernel), built on first
  // use by a batch that takes the query-order kernel; a replica builds its own
  DevBuf packed;
  static constexpr size_t PACKED_LIMIT = 1ull << 30;
  // 0 = not tried, 1 = ready and known complete, 2 = unavailable (too large / allocation failed: the unpacked tables serve
  // every batch), 3 = built by a kernel enqueued on packed_stream, completion signalled by packed_ev
  std::atomic<int> packed_state{0};
  std::mutex packed_mu;
  hipEvent_t packed_ev = nullptr;
  hipStream_t packed_stream = nullptr;
  ~Interp1DImpl() override {
    if (packed_ev) (void)hipEventDestroy(packed_ev);
  }
  // lane-wise evaluation (defined in lanewise_host.hpp)
  LanewiseRecords records;
  const void* lanewise_records(hipStream_t s);
  void lanewise_enqueue(hipStream_t s, Workspace& ws, const T* q, uint64_t q_stride, uint64_t rows, T* out,
                        uint64_t out_stride, bool check);
  ndi_status eval_lanewise(const void* q, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                           const ndi_eval_opts* opts, ndi_oob_info* info) override;
  // The copy is made by a kernel on the CALLER's stream (no NULL-stream launch, no device-wide synchronisation on the
  // evaluation path: the ring's side stream keeps running); calls on other streams are ordered behind it with an event
  // until it is known complete.  Never while the stream is being captured, and never fatal: a failed allocation leaves
  // the handle on the unpacked tables.
  bool ensure_packed(hipStream_t s) {
    int st = packed_state.load(std::memory_order_acquire);
    if (st == 1) return true;
    if (st == 2) return false;
    std::lock_guard<std::mutex> g(packed_mu);
    st = packed_state.load(std::memory_order_acquire);
    if (st == 1) return true;
    if (st == 2) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
    if (cs != hipStreamCaptureStatusNone) return false;   // this batch reads the unpacked tables
    if (st == 0) {
      const int parts = strategy == NDI_CUBIC_SPLINE ? 4 : 2;
      const size_t bytes = (size_t)(n - 1) * parts * lanes * sizeof(T);
      if (bytes == 0 || bytes > PACKED_LIMIT) {
        packed_state.store(2, std::memory_order_release);
        return false;
      }
      try {
        maybe_fail_lazy_alloc(__LINE__);
        packed.reserve(bytes);
        if (!packed_ev) NDI_HIP(hipEventCreateWithFlags(&packed_ev, hipEventDisableTiming));
        const uint64_t total = (n - 1) * (uint64_t)parts * lanes;
        const unsigned gr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 65536));
        hipLaunchKernelGGL(pack_intervals_kernel<T>, dim3(gr), dim3(BLOCK), 0, s, (const T*)data.as<T>(),
                           (const T*)ca.as<T>(), (const T*)cb.as<T>(), packed.as<T>(), n, lanes, parts);
        NDI_HIP(hipGetLastError());
        NDI_HIP(hipEventRecord(packed_ev, s));
      } catch (const HipFailure&) {
        (void)hipGetLastError();
        packed.release();
        packed_state.store(2, std::memory_order_release);
        return false;
      }
      packed_stream = s;
      packed_state.store(3, std::memory_order_release);
      return true;
    }
    // st == 3
    if (hipEventQuery(packed_ev) == hipSuccess) {
      packed_state.store(1, std::memory_order_release);
      return true;
    }
    (void)hipGetLastError();
    if (s != packed_stream) NDI_HIP(hipStreamWaitEvent(s, packed_ev, 0));
    return true;
  }

  // Small handles: ONE allocation for the knot pyramid, the data and the cubic tables (a / b / k); called before anything
  // is reserved.  `with_k`: set a slice aside for the k table where {y, k} can fit LDS (reserve_k decides whether it is used).
  void adopt_arena(bool cubic, bool with_k) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    uint64_t block = 1;
    while ((uint64_t)64 * block < n) block *= 2;
    const size_t pyr_b = al((n + (n + block - 1) / block) * sizeof(T));
    const size_t data_b = al((size_t)n * lanes * sizeof(T));
    const size_t tab_b = cubic ? al((size_t)(n - 1) * lanes * sizeof(T)) : 0;
    const size_t k_b = (cubic && with_k && 2 * data_b <= FUSED_LDS_LIMIT) ? data_b : 0;
    const size_t total = pyr_b + data_b + 2 * tab_b + k_b;
    if (total > ((size_t)1 << 20)) return;
    arena.reserve(total);
    char* p0 = static_cast<char*>(arena.p);
    pyr.buf.adopt(p0, pyr_b);
    data.adopt(p0 + pyr_b, data_b);
    if (tab_b) {
      ca.adopt(p0 + pyr_b + data_b, tab_b);
      cb.adopt(p0 + pyr_b + data_b + tab_b, tab_b);
    }
    if (k_b) ck.adopt(p0 + pyr_b + data_b + 2 * tab_b, k_b);
  }

  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, pyr.host_knots.data(), pyr.host_knots.size() * sizeof(T));
    const uint64_t f[3] = {n, (uint64_t)strategy | ((uint64_t)rule << 8) | ((uint64_t)deriv << 16), (uint64_t)mode};
    return fnv1a(h, f, sizeof(f));
  }

  // The derivatives k are kept next to a / b when {y, k} (2 n lanes elements) can sit in LDS beside the knots and the
  // smallest strip set: the query-order kernel then re-forms a / b per item instead of gathering them (TLDS == 2).
  // NDI_SPLINE_KEEP_K=0 drops them.
  T* reserve_k() {
    static const Knob keep{"NDI_SPLINE_KEEP_K", 1, Knob::live};
    if (!keep.get() || lanes > 2048 || fused_lds_bytes(false, 256, 2) > FUSED_LDS_LIMIT) {
      ck.release();   // (a slice of the handle's arena may have been set aside: ck.p != nullptr means "k was kept")
      return nullptr;
    }
    ck.reserve((size_t)n * lanes * sizeof(T));
    return ck.as<T>();
  }

  // ---- build: the CubicSpline tables (CubicSpline::build, cubic_spline.rs:754-771) and the local cubics -- Pchip, Akima,
  // CubicHermite (hermite_kernels.hpp).  Both, with the forms they dispatch over: spline_build_host.hpp.
  ndi_status build_spline(const ndi_interp1d_desc& d);
  ndi_status build_hermite(const void* dydx, int memspace);

  // ---- evaluation core on device pointers --------------------------------------------------
  // A batch is evaluated in two stages that may run on different streams: prep() = search (+ grouping) into a
  // scratch set, launch_eval() = the evaluation kernel reading that set.  Plan1 carries what prep() decided.
  // Both, with the planners and launchers they call: interp1d_host.hpp.
  using Plan = Plan1<T>;      // (the engine in float_host.hpp reads Impl::Plan)
  Plan prep(hipStream_t s, Scratch& sc, const T* q, uint64_t nq, T* out, uint64_t out_stride, int path,
            bool beside_eval = false, int flags = 0);
  void launch_eval(hipStream_t s, Scratch& sc, const Plan& P);

  // LDS footprint of eval_scalar_kernel / eval_lanes_kernel: [knots | dense index | interval records | table records | strips]
  size_t lanes_lds_bytes(unsigned tb) const {
    const size_t tr = strategy == NDI_CUBIC_SPLINE ? 4 : std::max<size_t>(2, 16 / sizeof(T));   // (whole 16-byte units)
    size_t b = ((size_t)(n + LANE_SENTINELS) * sizeof(T) + 15) & ~(size_t)15;
    b += pyr.dlut_bytes;
    if (strategy == NDI_CUBIC_SPLINE) b += (size_t)(n - 1) * 4 * sizeof(T);
    b += ((size_t)(n - 1) * lanes * tr * sizeof(T) + 15) & ~(size_t)15;
    if (lanes > 1) b += (size_t)(tb / 64) * 64 * lanes * sizeof(T);
    return b;
  }

  // The per-wave strips of eval_fused_kernel: an interval index and one operand (two: Linear, or the {y, k} form) per lane
  static size_t fused_strip_bytes(unsigned tb, bool strip2) {
    return (size_t)(tb / 64) * 64 * (sizeof(uint32_t) + (strip2 ? 2 : 1) * sizeof(T));
  }
  // LDS footprint of eval_fused_kernel: [pyramid | lut | per-wave strips | tables]
  size_t fused_lds_bytes(bool with_lut, unsigned tb, int tables) const {
    size_t b = (pyr.lds_bytes + 15) & ~(size_t)15;
    if (with_lut) b += pyr.lut_bytes;
    b += fused_strip_bytes(tb, strategy != NDI_CUBIC_SPLINE || tables == 2);
    if (tables) {
      const size_t rows = tables == 2 ? 2 * n : (strategy == NDI_CUBIC_SPLINE ? 3 * n - 2 : n);
      b += rows * lanes * sizeof(T);
    }
    return b;
  }

  // The long-row grouped evaluation (launch_bucketed, interp1d_host.hpp): eval_bucketed_kernel for one chunk,
  // eval_bucketed_group_kernel for the chunks of a ring group.
  static constexpr int BUCKETED_CQ = 128;   // queries per chunk of the two kernels: their CQ, and the unit of both grids

  // ---- ring groups: one evaluation launch for several chunks of a ring (float_host.hpp ring_produce) ----------------
  // Only the long-row bucketed plan has a group form; every other plan keeps one launch per chunk.
  static constexpr bool ring_groups = true;
  static bool groupable(const Plan& P) { return P.kind == Plan::BUCKETED; }
  void launch_eval_group(hipStream_t s, Scratch* const* sc, const Plan* P, uint32_t w);   // (interp1d_host.hpp)

  // ---- what the host engine (float_host.hpp) takes from this family ------------------------------------------------
  using Elem = T;
  static constexpr int query_arrays = 1;
  static constexpr bool small_rows = true, ring = true;
  static const char* axis_name(int) { return "x"; }
  void range_limits(T lim[4]) const {
    lim[0] = lim[2] = pyr.host_knots.front();
    lim[1] = lim[3] = pyr.host_knots.back();
  }
  Plan prep(hipStream_t s, Scratch& sc, Queries<T> q, uint64_t nq, T* out, uint64_t out_stride, int path,
            bool beside_eval = false, int flags = 0) {
    return prep(s, sc, q.a, nq, out, out_stride, path, beside_eval, flags);
  }
  void enqueue(hipStream_t s, Workspace& ws, Queries<T> q, uint64_t nq, T* out, uint64_t out_stride, int path, int flags) {
    launch_eval(s, ws.sc[0], prep(s, ws.sc[0], q.a, nq, out, out_stride, path, false, flags));
  }
  // the small-row paths: the knot pyramid in LDS
  bool small_rows_fit() const { return lanes <= (uint64_t)SMALL_LANES && pyr.lds_bytes <= LDS_STAGE_LIMIT; }
  bool zero_copy_fits(uint64_t nq, int q_space, int out_space) const {
    return q_space == NDI_MEM_HOST && out_space == NDI_MEM_HOST && small_rows_fit() &&
           nq * (lanes + 1) * sizeof(T) <= ZERO_COPY_LIMIT;
  }
  void small_begin() {
    g_last_path.store(NDI_PATH_GATHER);
    allow_dynamic_lds(reinterpret_cast<const void*>(&eval_small_kernel<T, ST_CUBIC>), (int)LDS_STAGE_LIMIT);
    allow_dynamic_lds(reinterpret_cast<const void*>(&eval_small_kernel<T, ST_LINEAR>), (int)LDS_STAGE_LIMIT);
  }
  // The fused search + evaluation launch of the small-row paths: nq packed rows into out, the kernel's own range test
  // (interp1d_host.hpp).
  void launch_small(hipStream_t s, StatusBlock* st, Queries<T> q, T* out, uint64_t nq);

  ndi_status eval(const void* q_, uint64_t nq, void* out_, uint64_t out_stride,
                  const ndi_eval_opts* opts, ndi_oob_info* info) override {
    return this->run_eval("ndi_interp1d_eval", {(const T*)q_, nullptr}, nq, out_, out_stride, opts, info);
  }
  ndi_status finish(void* stream, ndi_oob_info* info) override { return this->run_finish(stream, info); }
  // Interp1D::interp_array through a device-output ring.
  ndi_status eval_ring(const void* q_, uint64_t nq, const ndi_ring_desc* ring, ndi_ring_consumer consume,
                       void* user, const ndi_eval_opts* opts, ndi_oob_info* info) override {
    return this->run_ring("ndi_interp1d_eval_ring", {(const T*)q_, nullptr}, nq, ring, consume, user, opts, info);
  }

  ndi_status trim() override {
    DeviceGuard dg(device);
    this->trim_front();
    records.drop();
    return NDI_OK;
  }

  uint64_t scratch_sets() override { return spaces.size(); }

  // A replica on another (or the same) device: the knot pyramid is rebuilt from the host copy, data and the spline
  // tables are copied device to device (over xGMI between two GPUs) -- no second upload of the caller's arrays, no
  // second Thomas solve.
  ndi_status clone_to(int dev, Interp1DBase** out) override {
    std::unique_ptr<Interp1DImpl<T>> h(new Interp1DImpl<T>());
    h->dtype = dtype; h->device = dev; h->lanes = lanes;
    h->strategy = strategy; h->rule = rule; h->deriv = deriv; h->mode = mode; h->n = n;
    {
      DeviceGuard dg(device);
      NDI_HIP(hipDeviceSynchronize());     // the source tables are complete
    }
    DeviceGuard dg(dev);
    h->pyr.upload(pyr.host_knots.data(), n);
    auto copy = [&](DevBuf& dst, const DevBuf& src) {
      if (!src.p) return;
      dst.reserve(src.bytes);
      copy_across_devices(dst.p, dev, src.p, device, src.bytes);
    };
    copy(h->data, data);
    copy(h->ca, ca);
    copy(h->cb, cb);
    copy(h->ck, ck);
    *out = h.release();
    return NDI_OK;
  }

  ndi_status coefficients(void* a_out, void* b_out, int memspace) override {
    DeviceGuard dg(device);
    if (strategy != NDI_CUBIC_SPLINE) return fail(NDI_BAD_ARG, "Linear has no coefficient tables");
    const size_t tab = (size_t)(n - 1) * lanes * sizeof(T);
    const hipMemcpyKind k = memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (a_out) NDI_HIP(hipMemcpy(a_out, ca.p, tab, k));
    if (b_out) NDI_HIP(hipMemcpy(b_out, cb.p, tab, k));
    return NDI_OK;
  }

  ndi_status data_table(void* data_out, int memspace) override {
    DeviceGuard dg(device);
    NDI_HIP(hipMemcpy(data_out, data.p, (size_t)n * lanes * sizeof(T),
                      memspace == NDI_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return NDI_OK;
  }

  // ---- derivative handles (derivative_kernels.hpp) -----------------------------------------------------------
  // One application of the rule: a new handle on this handle's device whose {data, a, b} are derived from this handle's
  // {data, a, b} by one launch (no host plan, no temporaries; NULL stream like the other builds, complete on return).
  // This handle is only read.  The new handle keeps no k table: the {y, k} LDS form re-forms a / b from k and must
  // reproduce the table bits, which A == B == c cannot promise.
  std::unique_ptr<Interp1DImpl<T>> derive_once() const {
    std::unique_ptr<Interp1DImpl<T>> h(new Interp1DImpl<T>());
    h->dtype = dtype; h->device = device; h->lanes = lanes;
    h->strategy = strategy; h->rule = rule; h->deriv = deriv + 1; h->mode = mode; h->n = n;
    h->adopt_arena(true, false);
    h->pyr.upload(pyr.host_knots.data(), n);
    const size_t tab = (size_t)(n - 1) * lanes * sizeof(T);
    h->data.reserve((size_t)n * lanes * sizeof(T));
    h->ca.reserve(tab);
    h->cb.reserve(tab);
    DerivArgs<T> D{};
    D.y = data.as<T>(); D.a = ca.as<T>(); D.b = cb.as<T>();
    D.x = pyr.view.lv0;
    D.Y = h->data.template as<T>(); D.A = h->ca.template as<T>(); D.B = h->cb.template as<T>();
    D.n = n; D.lanes = lanes;
    constexpr int VN = Wide<T>::N;
    auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = lanes % VN == 0 && aligned(D.y) && aligned(D.a) && aligned(D.b) && aligned(D.Y) && aligned(D.A) &&
                     aligned(D.B);
    const uint64_t total = (n - 1) * (vec ? lanes / VN : lanes);
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 1u << 20));
    if (vec) hipLaunchKernelGGL((derivative_build_kernel<T, VN>), dim3(grid), dim3(BLOCK), 0, (hipStream_t) nullptr, D);
    else hipLaunchKernelGGL((derivative_build_kernel<T, 1>), dim3(grid), dim3(BLOCK), 0, (hipStream_t) nullptr, D);
    NDI_HIP(hipGetLastError());
    NDI_HIP(hipStreamSynchronize(nullptr));   // the tables are complete on return: any stream may read them
    return h;
  }

  ndi_status derivative(int nu, Interp1DBase** out) override {
    if (strategy != NDI_CUBIC_SPLINE)
      return fail(NDI_BAD_ARG, "Linear has no derivative handle: its slope jumps at the knots, and a handle's tables hold one "
                  "value per knot (derivative takes CubicSpline, Pchip, Akima and CubicHermite handles)");
    const int total = deriv + nu;
    const char* name = hermite_rule_name(rule);
    if (rule != HR_SPLINE && total >= 2)
      return fail(NDI_BAD_ARG, "%s: the second derivative of a C1 interpolant jumps at the knots, and a handle's tables hold "
                  "one value per knot (order 1 only; asked for order %d of %s)", name, nu,
                  deriv ? "its first derivative" : "the interpolant");
    if (total >= 3)
      return fail(NDI_BAD_ARG, "%s: the third derivative of a cubic spline jumps at the knots, and a handle's tables hold one "
                  "value per knot (orders 1 and 2 only; asked for order %d of %s)", name, nu,
                  deriv == 2 ? "its second derivative" : "its first derivative");
    DeviceGuard dg(device);
    Range rg("ndi:derivative_build");
    std::unique_ptr<Interp1DImpl<T>> h = derive_once();
    if (nu == 2) h = h->derive_once();   // the rule applied twice; the intermediate tables are freed here
    *out = h.release();
    return NDI_OK;
  }

  ndi_status antiderivative(Interp1DBase** out) override;   // (defined behind AntiderivImpl)
  ndi_status inverse(Interp1DBase** out) override;          // (defined behind InverseImpl)
};

#include "spline_build_host.hpp"
#include "interp1d_host.hpp"
#include "antiderivative_host.hpp"
#include "inverse_host.hpp"
#include "lanewise_host.hpp"
#include "lane_axes_host.hpp"

template <class T>
static std::vector<T> default_axis(uint64_t n) {
  std::vector<T> v(n);
  for (uint64_t i = 0; i < n; ++i) v[i] = (T)i;  // interp1d/mod.rs:402-406
  return v;
}

template <class T>
static std::vector<T> fetch_axis(const void* p, uint64_t len, int memspace) {
  std::vector<T> v(len);
  if (len == 0) return v;
  if (memspace == NDI_MEM_DEVICE)
    NDI_HIP(hipMemcpy(v.data(), p, len * sizeof(T), hipMemcpyDeviceToHost));
  else
    std::memcpy(v.data(), p, len * sizeof(T));
  return v;
}

// The descriptor checks every create makes once the axes are on the host, in the order of the reference's builders
// (interp1d/mod.rs:449-471, interp2d/mod.rs): the float, the integer and the half handles alike.  A: the axis as the
// family keeps it on the host (T, or the f32 images of f16 / bf16 knots).
template <class A>
static ndi_status check_desc_1d(const ndi_interp1d_desc& d, const A* x) {
  const uint64_t x_len = d.x ? d.x_len : d.n;
  if (d.validate) {
    ndi_status st = check_axis_1d<A>(x, x_len, d.n, d.strategy);
    if (st != NDI_OK) return st;
  } else if (x_len != d.n || d.n < min_len_1d(d.strategy)) {
    return fail(NDI_BAD_ARG, "unvalidated create with inconsistent sizes (x_len %llu, n %llu)",
                (unsigned long long)x_len, (unsigned long long)d.n);
  }
  if (d.lanes == 0) return fail(NDI_BAD_ARG, "lanes must be >= 1");
  if (d.n > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "more than %llu knots", (unsigned long long)MAX_KNOTS);
  if (!d.data) return fail(NDI_BAD_ARG, "null data pointer");
  return NDI_OK;
}

template <class A>
static ndi_status check_desc_2d(const ndi_interp2d_desc& d, const A* x, const A* y) {
  const uint64_t x_len = d.x ? d.x_len : d.nx, y_len = d.y ? d.y_len : d.ny;
  if (d.validate) {
    ndi_status st = check_axes_2d<A>(x, x_len, y, y_len, d.nx, d.ny);
    if (st != NDI_OK) return st;
  } else if (x_len != d.nx || y_len != d.ny || d.nx < 2 || d.ny < 2) {
    return fail(NDI_BAD_ARG, "unvalidated create with inconsistent sizes");
  }
  if (d.lanes == 0) return fail(NDI_BAD_ARG, "lanes must be >= 1");
  if (d.nx > MAX_KNOTS || d.ny > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "too many knots");
  if (!d.data) return fail(NDI_BAD_ARG, "null data pointer");
  return NDI_OK;
}

template <class T>
static ndi_status create1d(const ndi_interp1d_desc& d, Interp1DBase** out, const void* dydx = nullptr) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp1d_create");
  std::unique_ptr<Interp1DImpl<T>> h(new Interp1DImpl<T>());
  h->dtype = d.dtype;
  h->device = d.device;
  // Pchip / Akima / CubicHermite handles are of the cubic evaluation class: a / b tables, every evaluation form of the spline
  const bool cubic = d.strategy != NDI_LINEAR;
  h->strategy = cubic ? NDI_CUBIC_SPLINE : NDI_LINEAR;
  h->rule = d.strategy == NDI_PCHIP ? HR_PCHIP : d.strategy == NDI_AKIMA ? HR_AKIMA : d.strategy == NDI_CUBIC_HERMITE ? HR_GIVEN : HR_SPLINE;
  h->mode = d.extrapolate ? EX_YES : EX_NO;
  h->n = d.n;
  h->lanes = d.lanes;
  BuildClock clk;
  std::vector<T> x = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.n);
  clk.mark("fetch axis");
  if (const ndi_status st = check_desc_1d(d, x.data()); st != NDI_OK) return st;
  clk.mark("validate");
  h->adopt_arena(cubic, cubic);
  h->pyr.upload(x.data(), d.n);
  clk.mark("knot pyramid");
  const size_t bytes = (size_t)d.n * d.lanes * sizeof(T);
  h->data.reserve(bytes);
  NDI_HIP(hipMemcpy(h->data.p, d.data, bytes,
                    d.memspace == NDI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  clk.mark("data copy");
  if (d.strategy == NDI_CUBIC_SPLINE) {
    ndi_status st = h->build_spline(d);
    if (st != NDI_OK) return st;
    clk.mark("build_spline");
  } else if (cubic) {
    ndi_status st = h->build_hermite(dydx, d.memspace);
    if (st != NDI_OK) return st;
    clk.mark("build_hermite");
  }
  *out = h.release();
  return NDI_OK;
}

// ---------------------------------------------------------------------------------------------
// Interp2D (Bilinear; Bicubic: bicubic_host.hpp)
// ---------------------------------------------------------------------------------------------
struct Interp2DBase {
  virtual ~Interp2DBase() = default;
  virtual uint64_t signature() const = 0;
  int dtype = 0, device = 0;
  uint64_t lanes = 0;
  bool bicubic = false;   // the strategy: Bilinear (every element type) or Bicubic (f32 / f64, ndi_interp2d_create_bicubic)
  bool integral = false;  // Bicubic: a 2-D antiderivative handle (ndi_interp2d_antiderivative)
  // ndi_interp2d_tables: Bicubic handles only
  virtual ndi_status tables(void* zx, void* zy, void* zxy, int memspace) {
    return fail(NDI_BAD_ARG, "ndi_interp2d_tables takes a Bicubic handle: Bilinear keeps no node derivatives");
  }
  virtual ndi_status eval(const void* qx, const void* qy, uint64_t nq, void* out, uint64_t out_stride,
                          const ndi_eval_opts* opts, ndi_oob_info* info) = 0;
  virtual ndi_status finish(void* stream, ndi_oob_info* info) = 0;
  virtual ndi_status eval_ring(const void* qx, const void* qy, uint64_t nq, const ndi_ring_desc* ring,
                               ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts,
                               ndi_oob_info* info) = 0;
  virtual ndi_status trim() = 0;
  virtual ndi_status probe_ceiling(uint64_t nq, void* out, uint64_t out_stride, void* stream, int reps, double* ms) = 0;
  virtual ndi_status clone_to(int dev, Interp2DBase** out) = 0;
  // ndi_interp2d_partial: Bicubic handles and their partials only (Interp2DImpl::partial); every other handle is Bilinear
  virtual ndi_status partial(int nu_x, int nu_y, Interp2DBase** out) {
    return fail(NDI_BAD_ARG, "Bilinear has no partial-derivative handle: its slope jumps at every grid line and it keeps no "
                "node derivatives (ndi_interp2d_partial takes a Bicubic handle or a partial handle of one)");
  }
  // ndi_interp2d_antiderivative / _integral / _integral_tables: Bicubic surface handles and their integral handles only
  virtual ndi_status antiderivative(Interp2DBase** out) {
    return fail(NDI_BAD_ARG, "Bilinear has no antiderivative handle: ndi_interp2d_antiderivative takes a Bicubic surface handle "
                "(the integral of a Bilinear surface is not provided)");
  }
  virtual ndi_status integral_rect(const void* xa, const void* xb, const void* ya, const void* yb, uint64_t nq, void* out,
                                   uint64_t out_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
    return fail(NDI_BAD_ARG, "ndi_interp2d_integral takes an integral handle (ndi_interp2d_antiderivative of a Bicubic handle): "
                "this is a Bilinear handle");
  }
  virtual ndi_status integral_tables(void* const dst[5], int memspace) {
    return fail(NDI_BAD_ARG, "ndi_interp2d_integral_tables takes an integral handle (ndi_interp2d_antiderivative of a Bicubic "
                "handle): this is a Bilinear handle");
  }
  // ndi_interp2d_eval_jet: Bicubic surface handles only
  virtual ndi_status eval_jet(int order, const void* qx, const void* qy, uint64_t nq, void* const* outs, uint64_t out_stride,
                              const ndi_eval_opts* opts, ndi_oob_info* info) {
    return fail(NDI_BAD_ARG, "Bilinear has no value-and-gradient (jet) evaluation: its slope jumps at every grid line and it "
                "keeps no node derivatives (ndi_interp2d_eval_jet takes a Bicubic surface handle)");
  }
  // ndi_interp2d_eval_lanewise (lanewise2d_host.hpp): f32 / f64 Bilinear and Bicubic surface / partial handles only
  virtual ndi_status eval_lanewise(const void* qx, const void* qy, uint64_t nq, uint64_t q_stride, void* out,
                                   uint64_t out_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
    if (integral)
      return fail(NDI_BAD_ARG, "eval_lanewise: this is an integral handle (ndi_interp2d_antiderivative); the integral of a "
                  "surface per lane is not provided: the lane-wise evaluation takes Bilinear handles, Bicubic surface "
                  "handles and their partial-derivative handles");
    return fail(NDI_BAD_ARG, "eval_lanewise: %s handle is a Bilinear interpolator of a narrow element type; the lane-wise "
                "evaluation takes f32 / f64 handles", (dtype == NDI_I32 || dtype == NDI_I64) ? "an integer" : "an f16 / bf16");
  }
};

template <class T>
struct Interp2DImpl;
template <class T>
static void bicubic_launch_eval(const Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const T* qx, const T* qy,
                                uint64_t nq, T* out, uint64_t out_stride, bool check);
template <class T>
static ndi_status bicubic_tables(const Interp2DImpl<T>& h, void* zx, void* zy, void* zxy, int memspace);
template <class T>
static void bicubic_integral_build(const Interp2DImpl<T>& src, Interp2DImpl<T>& h);
template <class T>
static void bicubic_integral_launch_eval(const Interp2DImpl<T>& h, hipStream_t s, StatusBlock* st, const T* qx, const T* qy,
                                         const T* qx_lo, const T* qy_lo, uint64_t nq, T* out, uint64_t out_stride, bool check);
template <class T>
static ndi_status bicubic_integral_tables(const Interp2DImpl<T>& h, void* const dst[5], int memspace);
template <class T>
static ndi_status bicubic_integral_rect(Interp2DImpl<T>& h, const void* xa, const void* xb, const void* ya, const void* yb,
                                        uint64_t nq, void* out, uint64_t out_stride, const ndi_eval_opts* opts,
                                        ndi_oob_info* info);
template <class T>
static ndi_status bicubic_jet_eval(Interp2DImpl<T>& h, int order, const void* qx, const void* qy, uint64_t nq,
                                   void* const* outs, uint64_t out_stride, const ndi_eval_opts* opts, ndi_oob_info* info);

// What Interp2DImpl::prep decides for a batch and launch_eval runs (both in bilinear_host.hpp): the kind and its launch geometry.
template <class T>
struct Plan2 {
  enum Kind { SMALL, GATHER, TILED, FUSED2, LANES2, SLOPES2, BICUBIC, BICUBIC_INT } kind = GATHER;
  int l_qpl = 1;          // LANES2, scalar grids: queries per lane (1, or one 16-byte vector)
  bool l_check = false;   // LANES2: no range pre-pass (NDI_EVAL_FRESH_OUTPUT)
  bool f_lds_wide = false;   // SLOPES2: f_lds includes the result strip of the 16-byte store path
  // FUSED2 (eval_fused2d_kernel)
  bool f_vec = false, f_lut = false;
  uint64_t f_lv = 0;
  unsigned f_grid = 1, f_tb = 256;
  size_t f_lds = 0;
  bool compact = false;   // TILED: self-contained 16-byte records (group_scatter2d_kernel<T, true>)
  uint32_t ts = 0, nty = 0, nb = 0;   // TILED: tile shift, tiles per grid row, number of tiles
  const T* qx = nullptr;
  const T* qy = nullptr;
  uint64_t nq = 0;
  T* out = nullptr;
  uint64_t out_stride = 0;
};
template <class T>
static EvalSmall2Args<T> small2_args(const Interp2DImpl<T>& h, StatusBlock* st, const T* qx, const T* qy, T* out, uint64_t nq,
                                     uint64_t out_stride, int prechecked);

template <class T>
struct Interp2DImpl final : Interp2DBase, FloatEngine<T, Interp2DImpl<T>> {
  using Plan = Plan2<T>;      // (the engine in float_host.hpp reads Impl::Plan)
  int mode = EX_NO;
  uint64_t nx = 0, ny = 0;
  DevicePyramid<T> px, py;
  DevBuf data;
  // Bicubic: the node table T[nx][ny][4][lanes] ({z, zx, zy, zxy}); `data` is not kept.  Shared between a handle and its
  // partial-derivative handles (ndi_interp2d_partial), which only read it: freed with the last of them, in any order.
  std::shared_ptr<DevBuf> table;
  int nu_x = 0, nu_y = 0;     // Bicubic: the orders of the partial derivative this handle evaluates ((0, 0): the surface)
  // Bicubic: the periodic axes of the build (ndi_interp2d_create_bicubic_periodic; bit 0: x, bit 1: y).  The handle WRAPS
  // on such an axis when it extrapolates: an out-of-range coordinate is taken modulo the period before the search.
  int periodic_axes = 0;
  int wrap_axes() const { return mode != EX_NO ? periodic_axes : 0; }
  DevBuf itable;              // integral handles: the prefix records T[nx][ny][5][lanes] ({PP, Qz, Qzy, Pz, Pzx}), owned
  bool pair_packed = false;   // data holds the pair-packed layout (pack_pairs_kernel)
  // Bicubic: the node-record copy of the lane-wise evaluation (lanewise2d_host.hpp), shared with the partial handles exactly
  // as `table` is; a replica has its own
  std::shared_ptr<LanewiseRecords> lw_records = std::make_shared<LanewiseRecords>();
  // The stored grid as the kernels address it: cells per grid row and elements per cell of `data` (a pair-packed cell holds
  // the values of two neighbouring grid points of a row, and a row has one cell fewer).
  struct Layout { uint64_t row_cells, cell_elems; };
  Layout layout() const { return pair_packed ? Layout{ny - 1, 2 * lanes} : Layout{ny, lanes}; }
  SpaceSet spaces;
  OwnedRing ring_own;
  // lazy copies of the grid are built on first use by a kernel on the caller's stream, as Interp1DImpl::ensure_packed builds
  // its copy -- state 0 = not built, 1 = built and complete, 2 = not available, 3 = enqueued on *_stream, completion
  // signalled by *_ev
  ~Interp2DImpl() {
    if (slopes_ev) (void)hipEventDestroy(slopes_ev);
  }
  // the slope-record copy (slope_pack_kernel, eval_slopes2d_kernel): {z, m} per grid point of rows 0 .. nx - 2, 2 x the
  // grid, built on first use
  DevBuf slopes;
  std::atomic<int> slopes_state{0};
  std::mutex slopes_mu;
  hipEvent_t slopes_ev = nullptr;
  hipStream_t slopes_stream = nullptr;
  static constexpr size_t SLOPES_LIMIT = (size_t)256 << 20;
  // Layout of the copy: POINT records (2 x the grid; a query reads 4 L sizeof(T) contiguous bytes at the alignment of one
  // record) or CELL records (every cell owns its 4 L values at a stride padded to a power of two / a multiple of 128 bytes: a
  // query then touches ceil(bytes / 128) lines exactly).  The kernel is bound by L1 misses in flight (counters:
  // profiles/r06_slopes2d_*), so the layout with fewer lines per query wins; a tie goes to the smaller table.
  size_t slopes_cell_stride_bytes() const {
    const size_t need = 4 * lanes * sizeof(T);
    size_t sb = 32;
    while (sb < need && sb < 128) sb *= 2;
    if (sb < need) sb = (need + 127) / 128 * 128;
    return sb;
  }
  bool slopes_cells() const {
    const double need = (double)(4 * lanes * sizeof(T));
    const double lines_point = 1.0 + (need - 2.0 * sizeof(T)) / 128.0;
    const double lines_cell = (double)((slopes_cell_stride_bytes() + 127) / 128);
    return lines_cell <= 0.85 * lines_point;
  }
  size_t slopes_bytes() const {
    return slopes_cells() ? (size_t)(nx - 1) * (ny - 1) * slopes_cell_stride_bytes() : (size_t)(nx - 1) * ny * 2 * lanes * sizeof(T);
  }
  bool ensure_slopes(hipStream_t s) {
    int st = slopes_state.load(std::memory_order_acquire);
    if (st == 1) return true;
    if (st == 2) return false;
    std::lock_guard<std::mutex> g(slopes_mu);
    st = slopes_state.load(std::memory_order_acquire);
    if (st == 1) return true;
    if (st == 2) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) (void)hipGetLastError();
    if (cs != hipStreamCaptureStatusNone) return false;   // this batch takes another kernel
    if (st == 0) {
      const size_t bytes = slopes_bytes();
      if (bytes == 0 || bytes > SLOPES_LIMIT) {
        slopes_state.store(2, std::memory_order_release);
        return false;
      }
      try {
        maybe_fail_lazy_alloc(__LINE__);
        slopes.reserve(bytes);
        if (!slopes_ev) NDI_HIP(hipEventCreateWithFlags(&slopes_ev, hipEventDisableTiming));
        const uint64_t total = (uint64_t)(nx - 1) * ny * 2 * lanes;
        const unsigned gr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((total + BLOCK - 1) / BLOCK, 65536));
        if (slopes_cells()) NDI_HIP(hipMemsetAsync(slopes.p, 0, bytes, s));     // (the padding is never read; kept defined)
        hipLaunchKernelGGL(slope_pack_kernel<T>, dim3(gr), dim3(BLOCK), 0, s, (const T*)data.as<T>(), (const T*)px.view.lv0,
                           slopes.as<T>(), nx, ny, lanes, layout().row_cells, layout().cell_elems,
                           (uint64_t)(slopes_cells() ? slopes_cell_stride_bytes() / sizeof(T) : 0));
        NDI_HIP(hipGetLastError());
        NDI_HIP(hipEventRecord(slopes_ev, s));
      } catch (const HipFailure&) {
        (void)hipGetLastError();
        slopes.release();
        slopes_state.store(2, std::memory_order_release);
        return false;
      }
      slopes_stream = s;
      slopes_state.store(3, std::memory_order_release);
      return true;
    }
    if (hipEventQuery(slopes_ev) == hipSuccess) {   // st == 3
      slopes_state.store(1, std::memory_order_release);
      return true;
    }
    (void)hipGetLastError();
    if (s != slopes_stream) NDI_HIP(hipStreamWaitEvent(s, slopes_ev, 0));
    return true;
  }
  uint64_t signature() const override {
    uint64_t h = fnv1a(FNV_SEED, px.host_knots.data(), px.host_knots.size() * sizeof(T));
    h = fnv1a(h, py.host_knots.data(), py.host_knots.size() * sizeof(T));
    // (the strategy, the partial orders and the integral bit: no Bilinear / Bicubic mix, no surface beside its partial or
    // its integral, no two partials)
    const uint64_t f[3] = {nx, ny, (uint64_t)mode | ((uint64_t)bicubic << 8) | ((uint64_t)nu_x << 16) | ((uint64_t)nu_y << 24) |
                                       ((uint64_t)integral << 32) | ((uint64_t)periodic_axes << 40)};
    return fnv1a(h, f, sizeof(f));
  }
  ndi_status tables(void* zx, void* zy, void* zxy, int memspace) override {
    if (!bicubic) return Interp2DBase::tables(zx, zy, zxy, memspace);
    return bicubic_tables<T>(*this, zx, zy, zxy, memspace);
  }


  // Two stages as in Interp1DImpl: prep() = the plan -- a query-order kernel that searches for itself, or both searches
  // (+ the tile grouping) into a scratch set -- and launch_eval() = the kernel of that plan.  Both, with the planners and
  // launchers they call: bilinear_host.hpp.
  Plan prep(hipStream_t s, Scratch& sc, Queries<T> q, uint64_t nq, T* out, uint64_t out_stride, int path,
            bool beside_eval = false, int flags = 0);
  void launch_eval(hipStream_t s, Scratch& sc, const Plan& P);

  // grouped positions per unit of work of eval_bilinear_tiles_kernel (sweep: profiles/r03_c3_grouped.md)
  static uint32_t tile_chunk() {
    static const Knob chunk_knob{"NDI_TILE_CHUNK", 0};
    return chunk_knob.get() > 0 ? (uint32_t)chunk_knob.get() : 8192u;
  }

  // AUTO for 2-D: tile-grouped order when the batch has enough queries per grid cell to pay for staging every
  // tile once (C3 grid, profiles/r04_c3_qpc_sweep.jsonl: 0.95 queries per cell +5 % time, 1.2: -12 %, 1.4: -23 %,
  // 1.9: -34 %, 2.4 (C3): -37 %; below 1 the gather order wins) and the grid is far larger than what the caches hold.
  bool auto_tiles(uint64_t nq) const {
    constexpr double thr = 1.1;
    const double cells = (double)(nx - 1) * (double)(ny - 1);
    const size_t grid_bytes = (size_t)nx * ny * lanes * sizeof(T);
    if ((double)nq >= thr * cells && grid_bytes >= ((size_t)256 << 20) && lanes * sizeof(T) >= 64) return true;
    // Smaller grids (they sit in L2 / the Infinity Cache, the gather order is not HBM-bound) with rows of 256 bytes and
    // more: the tile order still wins -- up to 2 x -- once the batch is large enough to cover its fixed cost of staging
    // every tile (~0.13 ms) and has two queries per cell (profiles/r06_tiles_small_grids.jsonl: 64 MB grid, 1e6 queries
    // 0.206 -> 0.161 ms; 125 MB, 2e6: 0.38 -> 0.22; at 1 query per cell or 10 MB grids the gather order stays ahead).
    // Found by tests/test_gpu_auto_guard.py.
    return (double)nq >= 2.0 * cells && nq >= 800000 && lanes * sizeof(T) >= 256 && (lanes * sizeof(T)) % 16 == 0 && !pair_packed &&
           grid_bytes >= ((size_t)20 << 20);
  }

  // ---- what the host engine (float_host.hpp) takes from this family: x is array a, y is array b ---------------------
  using Elem = T;
  static constexpr int query_arrays = 2;
  static constexpr bool small_rows = true, ring = true;
  static const char* axis_name(int axis) { return axis == 0 ? "x" : "y"; }
  void range_limits(T lim[4]) const {
    lim[0] = px.host_knots.front(); lim[1] = px.host_knots.back();
    lim[2] = py.host_knots.front(); lim[3] = py.host_knots.back();
  }
  // The range pre-pass: the engine's (one mode for both axes), but for a Bicubic handle that wraps -- each axis by its own
  // rule (bicubic_wrap_check_kernel).
  void launch_range_check(hipStream_t s, StatusBlock* st, Queries<T> q, uint64_t nq) {
    if (wrap_axes() == 0) return FloatEngine<T, Interp2DImpl<T>>::launch_range_check(s, st, q, nq);
    T lim[4];
    range_limits(lim);
    const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + BLOCK - 1) / BLOCK, 4096));
    ProfScope ps(s, PC_LOCATE);
    hipLaunchKernelGGL(bicubic_wrap_check_kernel<T>, dim3(g), dim3(BLOCK), 0, s, q.a, q.b, nq, lim[0], lim[1], lim[2], lim[3],
                       wrap_axes(), &st->first_fail[0]);
    NDI_HIP(hipGetLastError());
    ps.done();
  }
  void enqueue(hipStream_t s, Workspace& ws, Queries<T> q, uint64_t nq, T* out, uint64_t out_stride, int path, int flags) {
    launch_eval(s, ws.sc[0], prep(s, ws.sc[0], q, nq, out, out_stride, path, false, flags));
  }
  // the small-row paths (Bilinear only): both pyramids in LDS
  size_t small_shmem() const { return (px.lds_bytes + py.lds_bytes + 15) & ~(size_t)15; }
  bool small_rows_fit() const { return !bicubic && lanes <= (uint64_t)SMALL_LANES && small_shmem() <= LDS_STAGE_LIMIT; }
  bool zero_copy_fits(uint64_t nq, int q_space, int out_space) const {
    return q_space == NDI_MEM_HOST && out_space == NDI_MEM_HOST && small_rows_fit() &&
           nq * (lanes + 2) * sizeof(T) <= ZERO_COPY_LIMIT;
  }
  void small_begin() {
    g_last_path.store(NDI_PATH_GATHER);
    allow_dynamic_lds(reinterpret_cast<const void*>(&eval_small2d_kernel<T>), (int)LDS_STAGE_LIMIT);
  }
  // The fused search + evaluation launch of the small-row paths: nq packed rows into out, the kernel's own range test.
  void launch_small(hipStream_t s, StatusBlock* st, Queries<T> q, T* out, uint64_t nq) {
    const EvalSmall2Args<T> A = small2_args<T>(*this, st, q.a, q.b, out, nq, lanes, 0);
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + BLOCK - 1) / BLOCK, 4096));
    launch1<T>(s, PC_EVAL, dim3(grid), dim3(BLOCK), small_shmem(), eval_small2d_kernel<T>, A);
  }

  ndi_status eval(const void* qx_, const void* qy_, uint64_t nq, void* out_, uint64_t out_stride,
                  const ndi_eval_opts* opts, ndi_oob_info* info) override {
    return this->run_eval("ndi_interp2d_eval", {(const T*)qx_, (const T*)qy_}, nq, out_, out_stride, opts, info);
  }
  ndi_status finish(void* stream, ndi_oob_info* info) override { return this->run_finish(stream, info); }
  // lane-wise evaluation (defined in lanewise2d_host.hpp)
  const void* lanewise_records(hipStream_t s);
  void lanewise_enqueue(hipStream_t s, Workspace& ws, const T* qx, const T* qy, uint64_t q_stride, uint64_t rows, T* out,
                        uint64_t out_stride, bool check);
  ndi_status eval_lanewise(const void* qx, const void* qy, uint64_t nq, uint64_t q_stride, void* out, uint64_t out_stride,
                           const ndi_eval_opts* opts, ndi_oob_info* info) override;
  // Interp2D::interp_array through a device-output ring.
  ndi_status eval_ring(const void* qx_, const void* qy_, uint64_t nq, const ndi_ring_desc* ring,
                       ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts,
                       ndi_oob_info* info) override {
    return this->run_ring("ndi_interp2d_eval_ring", {(const T*)qx_, (const T*)qy_}, nq, ring, consume, user, opts, info);
  }

  // A replica on another (or the same) device (see Interp1DImpl::clone_to): the grid is copied device to device in
  // the layout it is kept in (plain or pair-packed).
  ndi_status clone_to(int dev, Interp2DBase** out) override {
    std::unique_ptr<Interp2DImpl<T>> h(new Interp2DImpl<T>());
    h->dtype = dtype; h->device = dev; h->lanes = lanes;
    h->mode = mode; h->nx = nx; h->ny = ny; h->pair_packed = pair_packed;
    h->bicubic = bicubic;
    {
      DeviceGuard dg(device);
      NDI_HIP(hipDeviceSynchronize());
    }
    DeviceGuard dg(dev);
    h->px.upload(px.host_knots.data(), nx);
    h->py.upload(py.host_knots.data(), ny);
    if (bicubic) {   // the node table as it is: no rebuild; a replica owns its copy and keeps the partial orders
      h->nu_x = nu_x; h->nu_y = nu_y;
      h->periodic_axes = periodic_axes;
      h->table = std::make_shared<DevBuf>();
      h->table->reserve(table->bytes);
      copy_across_devices(h->table->p, dev, table->p, device, table->bytes);
      if (integral) {   // ... and the integral flag with a copy of the prefix records
        h->integral = true;
        h->itable.reserve(itable.bytes);
        copy_across_devices(h->itable.p, dev, itable.p, device, itable.bytes);
      }
    } else {
      h->data.reserve(data.bytes);
      copy_across_devices(h->data.p, dev, data.p, device, data.bytes);
    }
    *out = h.release();
    return NDI_OK;
  }

  // ndi_interp2d_partial: a handle on this handle's device that evaluates the partial derivative of the summed orders on
  // the SAME node table (shared ownership, no copy, no device work but the upload of the two knot axes).  Every refusal is
  // decided before that.
  ndi_status partial(int nux, int nuy, Interp2DBase** out) override {
    if (!bicubic) return Interp2DBase::partial(nux, nuy, out);
    if (integral)
      return fail(NDI_BAD_ARG, "Bicubic: an integral handle has no partial-derivative handle: its x-derivative is a y-integral "
                  "of the surface, which is not provided (the mixed (1, 1) partial is the handle it was made from)");
    if (nux < 0 || nuy < 0)
      return fail(NDI_BAD_ARG, "Bicubic: a partial-derivative order below 0 (asked for (%d, %d)); orders are 0, 1 or 2 per "
                  "variable", nux, nuy);
    if (nux == 0 && nuy == 0)
      return fail(NDI_BAD_ARG, "Bicubic: the partial derivative of orders (0, 0) is the handle itself; ask for an order of 1 "
                  "or 2 in at least one variable (ndi_interp2d_clone makes a copy)");
    const long long tx = (long long)nu_x + nux, ty = (long long)nu_y + nuy;
    if (tx > 2 || ty > 2)
      return fail(NDI_BAD_ARG, "Bicubic: the third derivative of a cubic spline jumps at the grid lines, and the node table "
                  "determines orders 0 to 2 per variable (asked for (%d, %d) of a handle of orders (%d, %d): (%lld, %lld))",
                  nux, nuy, nu_x, nu_y, tx, ty);
    DeviceGuard dg(device);
    std::unique_ptr<Interp2DImpl<T>> h(new Interp2DImpl<T>());
    h->dtype = dtype; h->device = device; h->lanes = lanes;
    h->mode = mode; h->nx = nx; h->ny = ny;
    h->bicubic = true;
    h->nu_x = (int)tx; h->nu_y = (int)ty;
    h->periodic_axes = periodic_axes;   // the table is shared: so are its periodic axes, and the wrap with them
    h->px.upload(px.host_knots.data(), nx);
    h->py.upload(py.host_knots.data(), ny);
    h->table = table;
    h->lw_records = lw_records;
    *out = h.release();
    return NDI_OK;
  }

  // ndi_interp2d_antiderivative: a handle on this handle's device that evaluates F(qx, qy), the integral of the surface over
  // [x[0], qx] x [y[0], qy].  It shares the node table (no copy) and owns the five prefix tables, built here on the NULL
  // stream.  Every refusal is decided before any device work.
  ndi_status antiderivative(Interp2DBase** out) override {
    if (!bicubic) return Interp2DBase::antiderivative(out);
    if (integral)
      return fail(NDI_BAD_ARG, "Bicubic: this handle is already an integral handle; a second antiderivative is not provided");
    if (nu_x != 0 || nu_y != 0)
      return fail(NDI_BAD_ARG, "Bicubic: a partial-derivative handle (orders (%d, %d)) has no antiderivative handle: the "
                  "integral of a partial is not provided (ndi_interp2d_antiderivative takes the surface handle)", nu_x, nu_y);
    if (wrap_axes() != 0)
      return fail(NDI_BAD_ARG, "Bicubic: this handle wraps queries on %s (a periodic axis with extrapolate): the integral of a "
                  "periodic surface is not periodic, and the antiderivative of a wrapping handle is not provided (build "
                  "with extrapolate = 0)", wrap_axes() == 3 ? "x and y" : wrap_axes() == 1 ? "x" : "y");
    DeviceGuard dg(device);
    std::unique_ptr<Interp2DImpl<T>> h(new Interp2DImpl<T>());
    h->dtype = dtype; h->device = device; h->lanes = lanes;
    h->mode = mode; h->nx = nx; h->ny = ny;
    h->bicubic = true;
    h->integral = true;
    h->periodic_axes = periodic_axes;   // (it never wraps -- refused above; kept for the replica signature)
    h->px.upload(px.host_knots.data(), nx);
    h->py.upload(py.host_knots.data(), ny);
    h->table = table;
    bicubic_integral_build<T>(*this, *h);
    *out = h.release();
    return NDI_OK;
  }
  ndi_status integral_rect(const void* xa, const void* xb, const void* ya, const void* yb, uint64_t nq, void* out_,
                           uint64_t out_stride, const ndi_eval_opts* opts, ndi_oob_info* info) override {
    if (!integral)
      return fail(NDI_BAD_ARG, "ndi_interp2d_integral takes an integral handle (ndi_interp2d_antiderivative of a Bicubic "
                  "handle): this is a %s handle", !bicubic ? "Bilinear" : (nu_x || nu_y) ? "Bicubic partial-derivative"
                                                                                         : "Bicubic surface");
    return bicubic_integral_rect<T>(*this, xa, xb, ya, yb, nq, out_, out_stride, opts, info);
  }
  ndi_status integral_tables(void* const dst[5], int memspace) override {
    if (!integral)
      return fail(NDI_BAD_ARG, "ndi_interp2d_integral_tables takes an integral handle (ndi_interp2d_antiderivative of a Bicubic "
                  "handle): this is a %s handle", !bicubic ? "Bilinear" : (nu_x || nu_y) ? "Bicubic partial-derivative"
                                                                                         : "Bicubic surface");
    return bicubic_integral_tables<T>(*this, dst, memspace);
  }
  ndi_status eval_jet(int order, const void* qx, const void* qy, uint64_t nq, void* const* outs, uint64_t out_stride,
                      const ndi_eval_opts* opts, ndi_oob_info* info) override {
    if (!bicubic) return Interp2DBase::eval_jet(order, qx, qy, nq, outs, out_stride, opts, info);
    if (integral)
      return fail(NDI_BAD_ARG, "Bicubic: an integral handle has no value-and-gradient (jet) evaluation: its x-derivative is a "
                  "y-integral of the surface, which is not provided (ndi_interp2d_eval_jet takes the surface handle)");
    if (nu_x != 0 || nu_y != 0)
      return fail(NDI_BAD_ARG, "Bicubic: a partial-derivative handle (orders (%d, %d)) has no value-and-gradient (jet) "
                  "evaluation: a jet of a partial would need third orders, which jump at the grid lines "
                  "(ndi_interp2d_eval_jet takes the surface handle)", nu_x, nu_y);
    return bicubic_jet_eval<T>(*this, order, qx, qy, nq, outs, out_stride, opts, info);
  }

  // Median time of `reps` launches of probe_gather_kernel over nq queries (see kernels.hpp).
  ndi_status probe_ceiling(uint64_t nq, void* out, uint64_t out_stride, void* stream, int reps, double* ms) override {
    if (bicubic) return fail(NDI_BAD_ARG, "Bicubic: the probe runs Bilinear's access mix (four corner vectors of the plain grid)");
    DeviceGuard dg(device);
    constexpr int VN = Wide<T>::N;
    if (!out || !ms || nq == 0 || reps < 1) return fail(NDI_BAD_ARG, "probe needs an output buffer, nq >= 1, reps >= 1");
    if (out_stride < lanes) return fail(NDI_BAD_ARG, "out_row_stride < lanes");
    if (lanes % VN || out_stride % VN || !aligned16(out))
      return fail(NDI_UNSUPPORTED, "the probe covers the vectorised layout only (lanes a multiple of %d)", VN);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t items = nq * (lanes / VN);
    const unsigned g = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + BLOCK - 1) / BLOCK, 32768));
    hipEvent_t a, b;
    NDI_HIP(hipEventCreate(&a));
    NDI_HIP(hipEventCreate(&b));
    std::vector<float> ts;
    for (int r = 0; r <= reps; ++r) {   // the first launch is a warm-up
      NDI_HIP(hipEventRecord(a, s));
      hipLaunchKernelGGL((probe_gather_kernel<T, VN>), dim3(g), dim3(BLOCK), 0, s, (const T*)data.as<T>(), nx, ny,
                         layout().row_cells, layout().cell_elems, lanes, nq,
                         (uint64_t)(12345 + r), (T*)out, out_stride);
      NDI_HIP(hipGetLastError());
      NDI_HIP(hipEventRecord(b, s));
      NDI_HIP(hipEventSynchronize(b));
      float t = 0.f;
      NDI_HIP(hipEventElapsedTime(&t, a, b));
      if (r) ts.push_back(t);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    std::sort(ts.begin(), ts.end());
    *ms = ts[ts.size() / 2];
    return NDI_OK;
  }

  ndi_status trim() override {
    DeviceGuard dg(device);
    this->trim_front();
    {   // the slope-record copy (up to 256 MiB) goes too when it is complete and idle; the next batch that wants it rebuilds it
      std::lock_guard<std::mutex> g(slopes_mu);
      int st = slopes_state.load(std::memory_order_acquire);
      if (st == 3 && hipEventQuery(slopes_ev) == hipSuccess) st = 1;
      if (st == 1) {
        slopes.release();
        slopes_state.store(0, std::memory_order_release);
      } else {
        (void)hipGetLastError();
      }
    }
    if (bicubic && !integral) lw_records->drop();   // the lane-wise node-record copy: the next call that wants it rebuilds it
    return NDI_OK;
  }
};

template <class T>
static ndi_status create2d(const ndi_interp2d_desc& d, Interp2DBase** out) {
  DeviceGuard dg(d.device);
  Range rg("ndi_interp2d_create");
  std::unique_ptr<Interp2DImpl<T>> h(new Interp2DImpl<T>());
  h->dtype = d.dtype;
  h->device = d.device;
  h->mode = d.extrapolate ? EX_YES : EX_NO;
  h->nx = d.nx;
  h->ny = d.ny;
  h->lanes = d.lanes;
  std::vector<T> x = d.x ? fetch_axis<T>(d.x, d.x_len, d.memspace) : default_axis<T>(d.nx);
  std::vector<T> y = d.y ? fetch_axis<T>(d.y, d.y_len, d.memspace) : default_axis<T>(d.ny);
  if (const ndi_status st = check_desc_2d(d, x.data(), y.data()); st != NDI_OK) return st;
  h->px.upload(x.data(), d.nx);
  h->py.upload(y.data(), d.ny);
  const size_t bytes = (size_t)d.nx * d.ny * d.lanes * sizeof(T);
  const hipMemcpyKind kind = d.memspace == NDI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // Short trailing axes (<= 64 B per grid point): keep the pair-packed layout instead of the plain one -- unless the
  // whole grid fits a CU's LDS (the reference's 100 x 100 bench grids): those stay plain, the layout eval_lanes2d_kernel
  // stages, and never leave L2 for the other kernels.  NDI_PAIR_PACK=1 packs every eligible grid (tests), 0 none.
  static const Knob pack_knob{"NDI_PAIR_PACK", -1};
  const int pack_env = pack_knob.get();
  h->pair_packed = d.lanes * sizeof(T) <= 64 && d.ny >= 2 && (pack_env > 0 || (pack_env < 0 && bytes > FUSED_LDS_LIMIT));
  if (h->pair_packed) {
    const size_t packed = (size_t)d.nx * (d.ny - 1) * 2 * d.lanes * sizeof(T);
    h->data.reserve(packed);
    const void* src = d.data;
    DevBuf tmp;
    if (d.memspace != NDI_MEM_DEVICE) {
      tmp.reserve(bytes);
      NDI_HIP(hipMemcpy(tmp.p, d.data, bytes, kind));
      src = tmp.p;
    }
    // copy in 16-byte vectors when a grid point is a whole number of them (and both buffers are aligned)
    const size_t cell_bytes = (size_t)d.lanes * sizeof(T);
    const bool vec = cell_bytes % 16 == 0 && aligned16(src) && aligned16(h->data.p);
    const uint32_t units = vec ? (uint32_t)(cell_bytes / 16) : (uint32_t)d.lanes;
    int shift = -1;
    for (int b = 0; b < 31; ++b)
      if ((1u << b) == units) shift = b;
    const uint64_t row_out = (uint64_t)(d.ny - 1) * 2 * units;
    dim3 grid((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((row_out + BLOCK - 1) / BLOCK, 1024)),
              (unsigned)std::min<uint64_t>(d.nx, 16384));
    if (vec)
      hipLaunchKernelGGL(pack_pairs_kernel<uint4>, grid, dim3(BLOCK), 0, (hipStream_t) nullptr, (const uint4*)src,
                         (uint4*)h->data.p, (uint64_t)d.nx, (uint64_t)d.ny, units, shift);
    else
      hipLaunchKernelGGL(pack_pairs_kernel<T>, grid, dim3(BLOCK), 0, (hipStream_t) nullptr, (const T*)src,
                         h->data.template as<T>(), (uint64_t)d.nx, (uint64_t)d.ny, units, shift);
    NDI_HIP(hipGetLastError());
    NDI_HIP(hipDeviceSynchronize());
  } else {
    h->data.reserve(bytes);
    NDI_HIP(hipMemcpy(h->data.p, d.data, bytes, kind));
  }
  *out = h.release();
  return NDI_OK;
}

// ---------------------------------------------------------------------------------------------
// Interp2D Bicubic: build, launch and table read-back
// ---------------------------------------------------------------------------------------------
#include "bilinear_host.hpp"
#include "bicubic_host.hpp"
#include "bicubic_local_host.hpp"
#include "bicubic_integral_host.hpp"
#include "bicubic_jet_host.hpp"
#include "lanewise2d_host.hpp"

// ---------------------------------------------------------------------------------------------
// Interp3D (Trilinear)
// ---------------------------------------------------------------------------------------------
#include "trilinear_host.hpp"
#include "tricubic_host.hpp"

// ---------------------------------------------------------------------------------------------
// Locator: VectorExtensions::get_lower_index with the knot pyramid resident on the device
// ---------------------------------------------------------------------------------------------
struct LocatorBase {
  virtual ~LocatorBase() = default;
  int dtype = 0, device = 0;
  virtual ndi_status eval(const void* q, uint64_t nq, int64_t* out_idx, int memspace, void* stream) = 0;
  bool one_shot = false;   // built for a single search (ndi_get_lower_index_batch): no pinned buffer is set up
};

template <class T>
struct LocatorImpl final : LocatorBase {
  DevicePyramid<T> pyr;
  SpaceSet spaces;

  ndi_status eval(const void* q, uint64_t nq, int64_t* out_idx, int memspace, void* stream) override {
    DeviceGuard dg(device);
    if (nq == 0) return NDI_OK;
    Range rg("ndi_locator_eval");
    hipStream_t s = (hipStream_t)stream;
    const T* qdev = (const T*)q;
    int64_t* odev = out_idx;
    if (memspace == NDI_MEM_HOST && !one_shot && nq * (sizeof(T) + sizeof(int64_t)) <= ((size_t)1 << 20)) {
      // small host batch: zero-copy through the pinned buffer's host mapping (see eval_small_zero_copy)
      SpaceLease lease(spaces, s);
      Workspace& ws = lease.ws;
      const size_t q_bytes = ((nq * sizeof(T)) + 255) & ~(size_t)255;
      ws.ensure_pin(std::max<size_t>(q_bytes + nq * sizeof(int64_t), 8ull << 20));
      T* pq = reinterpret_cast<T*>(ws.pin);
      int64_t* po = reinterpret_cast<int64_t*>((char*)ws.pin + q_bytes);
      std::memcpy(pq, q, nq * sizeof(T));
      run_locate<T>(s, pyr, ws.pin_device<const T>(pq), nq, nullptr, ws.pin_device<int64_t>(po), nullptr, nullptr, EX_YES);
      NDI_HIP(hipStreamSynchronize(s));
      std::memcpy(out_idx, po, nq * sizeof(int64_t));
      return NDI_OK;
    }
    if (memspace == NDI_MEM_HOST) {
      SpaceLease lease(spaces, s);
      Workspace& ws = lease.ws;
      ws.qdev.reserve(nq * sizeof(T));
      ws.stage.reserve(nq * sizeof(int64_t));
      NDI_HIP(hipMemcpyAsync(ws.qdev.p, q, nq * sizeof(T), hipMemcpyHostToDevice, s));
      qdev = ws.qdev.as<T>();
      odev = ws.stage.as<int64_t>();
      run_locate<T>(s, pyr, qdev, nq, nullptr, odev, nullptr, nullptr, EX_YES);
      NDI_HIP(hipMemcpyAsync(out_idx, odev, nq * sizeof(int64_t), hipMemcpyDeviceToHost, s));
      NDI_HIP(hipStreamSynchronize(s));
      return NDI_OK;
    }
    run_locate<T>(s, pyr, qdev, nq, nullptr, odev, nullptr, nullptr, EX_YES);
    NDI_HIP(hipStreamSynchronize(s));
    return NDI_OK;
  }
};

template <class T>
static ndi_status create_locator(int device, const void* knots, uint64_t n, int memspace, LocatorBase** out) {
  DeviceGuard dg(device);
  if (n < 2) return fail(NDI_BAD_ARG, "get_lower_index needs at least 2 knots");
  if (n > MAX_KNOTS) return fail(NDI_UNSUPPORTED, "too many knots");
  std::unique_ptr<LocatorImpl<T>> h(new LocatorImpl<T>());
  h->dtype = DType<T>::id;
  h->device = device;
  std::vector<T> x = fetch_axis<T>(knots, n, memspace);
  h->pyr.upload(x.data(), n);
  *out = h.release();
  return NDI_OK;
}

// ---------------------------------------------------------------------------------------------
// sharded evaluation: one call, N handles (normally one per device), one host thread per shard
// ---------------------------------------------------------------------------------------------
// The reference's multi-worker shape is one interpolator driven from many threads over contiguous blocks of the
// query array (benches/bench_interp1d.rs:49-79).  Here shard i of n evaluates the block shard_range(nq, i, n) on
// handles[i]'s device (shard 0 on the calling thread, the others on the caller's persistent workers).  The
// reference's first-error result (interp1d/mod.rs:326-343) is reproduced across shards:
// every shard range-checks its block first, the minimum global failing index F is agreed on at a host barrier, and
// only the rows [0, F) are produced -- later rows are never written.  No device-to-device traffic.
static void shard_range(uint64_t nq, uint32_t i, uint32_t n, uint64_t* lo, uint64_t* hi) {
  const uint64_t base = nq / n, rem = nq % n;
  *lo = (uint64_t)i * base + std::min<uint64_t>(i, rem);
  *hi = *lo + base + (i < rem ? 1 : 0);
}
static uint64_t shard_lo(uint64_t nq, uint32_t i, uint32_t n) {
  uint64_t lo, hi;
  shard_range(nq, i, n, &lo, &hi);
  return lo;
}

struct ShardBarrier {
  std::mutex m;
  std::condition_variable cv;
  unsigned n, count = 0, gen = 0;
  explicit ShardBarrier(unsigned n_) : n(n_) {}
  void wait() {
    std::unique_lock<std::mutex> l(m);
    const unsigned g = gen;
    if (++count == n) {
      count = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(l, [&] { return g != gen; });
    }
  }
  // k shards will never arrive (their worker could not be started): the others must not wait for them
  void drop(unsigned k) {
    std::unique_lock<std::mutex> l(m);
    n -= k;
    if (n > 0 && count == n) {
      count = 0;
      ++gen;
      cv.notify_all();
    }
  }
};

struct ShardOutcome {
  ndi_status st = NDI_OK;
  std::string msg;
};

// The worker threads of sharded calls are persistent and belong to the CALLING thread (thread_local): shard i of
// every sharded call a host thread makes runs on the same worker, so the per-(stream, thread) scratch of a handle is
// found again on the next call instead of being allocated and later evicted (hipMalloc / hipFree per call), and two
// host threads issuing sharded calls at the same time never wait for each other's workers (the shards of one call
// meet at a barrier: they must all be running).  Workers are joined when their owner thread exits.
class ShardWorkers {
  struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, stop = false;
  };
  std::vector<std::unique_ptr<Worker>> w_;
  static void loop(Worker* w) {
    std::unique_lock<std::mutex> l(w->m);
    for (;;) {
      w->cv.wait(l, [w] { return w->has_job || w->stop; });
      if (w->stop) return;
      std::function<void()> job = std::move(w->job);
      l.unlock();
      job();          // the shard bodies catch everything
      l.lock();
      w->has_job = false;
      w->cv.notify_all();
    }
  }

 public:
  ShardWorkers() = default;
  ShardWorkers(const ShardWorkers&) = delete;
  ShardWorkers& operator=(const ShardWorkers&) = delete;
  ~ShardWorkers() {
    for (auto& w : w_) {
      {
        std::lock_guard<std::mutex> g(w->m);
        w->stop = true;
      }
      w->cv.notify_all();
      if (w->th.joinable()) w->th.join();
    }
  }
  // A worker enters the pool only once its thread runs: if std::thread throws (the case run_shards drops shards for),
  // the thread-less Worker is taken out again, so a later call never start()s a job nobody will run.
  // NDI_TEST_FAIL_WORKER_START=k (tests only, read per call): the k-th and later workers of a pool fail to start.
  void ensure(size_t n) {
    while (w_.size() < n) {
      w_.emplace_back(new Worker());
      Worker* w = w_.back().get();
      try {
        if (const char* e = std::getenv("NDI_TEST_FAIL_WORKER_START"))
          if (*e && w_.size() >= (size_t)std::max(1, std::atoi(e))) throw std::runtime_error("injected: worker thread start");
        w->th = std::thread(loop, w);
      } catch (...) {
        w_.pop_back();
        throw;
      }
    }
  }
  size_t size() const { return w_.size(); }
  void start(size_t i, std::function<void()> f) {
    Worker* w = w_[i].get();
    {
      std::lock_guard<std::mutex> g(w->m);
      w->job = std::move(f);
      w->has_job = true;
    }
    w->cv.notify_all();
  }
  void wait(size_t n) {
    for (size_t i = 0; i < n; ++i) {
      Worker* w = w_[i].get();
      std::unique_lock<std::mutex> l(w->m);
      w->cv.wait(l, [w] { return !w->has_job; });
    }
  }
};
static ShardWorkers& shard_workers() {
  static thread_local ShardWorkers p;
  return p;
}

// Shard: constructed on the worker thread (the scratch lease is keyed by the thread), pre() = upload + range
// pre-pass (+ the ring's speculative first chunk), run(limit) = produce the shard's first `limit` rows.
template <class Shard, class Job>
static void run_shards(const Job& job, uint32_t n, std::vector<ShardOutcome>& out, unsigned long long F[2]) {
  ShardBarrier bar(n);
  std::atomic<unsigned long long> fx{NO_FAIL}, fy{NO_FAIL};
  std::atomic<int> broken{0};
  auto amin = [](std::atomic<unsigned long long>& a, unsigned long long v) {
    unsigned long long c = a.load();
    while (v < c && !a.compare_exchange_weak(c, v)) {
    }
  };
  auto work = [&](uint32_t i) {
    bool arrived = false;
    try {
      Shard c(job, i, n);
      unsigned long long lx = NO_FAIL, ly = NO_FAIL;
      c.pre(&lx, &ly);
      if (lx != NO_FAIL) amin(fx, c.lo + lx);
      if (ly != NO_FAIL) amin(fy, c.lo + ly);
      arrived = true;
      bar.wait();
      const unsigned long long f = std::min(fx.load(), fy.load());
      const uint64_t limit = broken.load() ? 0 : (f <= c.lo ? 0 : std::min<uint64_t>(c.cnt, f - c.lo));
      const ndi_status st = c.run(limit);
      if (st != NDI_OK) {
        out[i].st = st;
        out[i].msg = tls_error();
      }
    } catch (const HipFailure& f) {
      out[i].st = from_hip(f);
      out[i].msg = tls_error();
      broken.store(1);
    } catch (const std::bad_alloc&) {
      out[i].st = NDI_HIP_ERROR;
      out[i].msg = "host out of memory";
      broken.store(1);
    } catch (...) {
      out[i].st = NDI_HIP_ERROR;
      out[i].msg = "unexpected C++ exception";
      broken.store(1);
    }
    if (!arrived) bar.wait();
  };
  // The workers run `work` by reference to this frame: whatever happens while they are being started, this frame
  // must not unwind before every started worker is idle again, and the shards that did start must not wait at the
  // barrier for shards that never will.  The pool belongs to the calling thread and is busy for the whole call: a
  // nested sharded call from the same host thread (a ring consumer issuing one) is refused by the callers.
  ShardWorkers& pool = shard_workers();
  uint32_t started = 0;
  try {
    pool.ensure(n - 1);
    for (uint32_t i = 1; i < n; ++i) {
      pool.start(i - 1, [&work, i] { work(i); });
      ++started;
    }
  } catch (...) {
    broken.store(1);
    for (uint32_t i = started + 1; i < n; ++i) {
      out[i].st = NDI_HIP_ERROR;
      out[i].msg = "could not start the shard's host thread";
    }
    bar.drop(n - 1 - started);
  }
  work(0);   // shard 0 runs on the calling thread (never throws: the body catches everything)
  pool.wait(started);
  F[0] = fx.load();
  F[1] = fy.load();
}

// One sharded call at a time per calling host thread (its persistent workers are busy until the call returns).
struct ShardedCallScope {
  static bool& flag() {
    static thread_local bool in_call = false;
    return in_call;
  }
  bool nested;
  ShardedCallScope() : nested(flag()) { flag() = true; }
  ~ShardedCallScope() {
    if (!nested) flag() = false;
  }
};

// The arguments of a sharded entry point (qy: 2-D only; out_stride or rings / consume / user).
struct ShardCall {
  const void* qx;
  const void* qy;
  uint64_t nq;
  const ndi_shard_io* io;
  uint64_t out_stride;
  const ndi_ring_desc* rings;
  ndi_ring_consumer consume;
  void* user;
  ndi_eval_opts o;
};

// The f32 / f64 handles (Impl: a FloatEngine, float_host.hpp): a shard's query arrays are the caller's per-shard
// pointers, or its block of the whole batch.
template <class Impl>
struct Job : ShardCall {
  using T = typename Impl::Elem;
  std::vector<Impl*> H;
  explicit Job(const ShardCall& c) : ShardCall(c) {}
  Queries<T> q_src(uint32_t i, uint32_t n) const {
    constexpr bool two = Impl::query_arrays == 2;
    if (io && io[i].q) return {(const T*)io[i].q, two ? (const T*)io[i].qy : nullptr};
    return Queries<T>{(const T*)qx, two ? (const T*)qy : nullptr} + shard_lo(nq, i, n);
  }
};

template <class Impl>
struct Shard {
  using T = typename Impl::Elem;
  const Job<Impl>& J;
  uint32_t i;
  Impl* h;
  uint64_t lo, cnt;
  DeviceGuard dg;
  hipStream_t s;
  SpaceLease lease;
  Workspace& ws;
  Queries<T> q_src, q;
  uint64_t stride = 0;
  RingRun<typename Impl::Plan> R;
  Shard(const Job<Impl>& j, uint32_t i_, uint32_t n)
      : J(j), i(i_), h(j.H[i_]), lo(shard_lo(j.nq, i_, n)), cnt(shard_lo(j.nq, i_ + 1, n) - shard_lo(j.nq, i_, n)),
        dg(h->device), s((hipStream_t)(j.io ? j.io[i_].stream : nullptr)), lease(h->spaces, s), ws(lease.ws),
        q_src(j.q_src(i_, n)) {}
  void pre(unsigned long long* fx, unsigned long long* fy) {
    if (!cnt) return;
    q = h->stage_queries(s, ws, q_src, cnt, J.o.q_memspace);
    h->enqueue_prepass(s, ws, q, cnt);
    if (J.rings) {
      (void)check_ring_desc(&J.rings[i], h->lanes, &stride);   // validated before the threads started
      h->ring_begin(s, ws, q, cnt, &J.rings[i], stride, J.o, R);
    }
    NDI_HIP(hipStreamSynchronize(s));
    const FirstFail f = FirstFail::of(ws, q);
    *fx = f.f0;
    *fy = f.f1;
  }
  ndi_status run(uint64_t limit) {
    if (!cnt) return NDI_OK;
    if (J.rings) {
      h->ring_produce(s, ws, q, limit, R, J.consume, J.user, J.o, lo, i);
      return NDI_OK;
    }
    if (!limit) return NDI_OK;
    ndi_eval_opts o = J.o;
    o.async_launch = 0;
    ndi_oob_info none{};
    return h->eval_body(s, ws, q, q_src, J.o.q_memspace, limit, J.io[i].out, J.out_stride, o, &none);
  }
};

// Outcome of a sharded call on the calling thread: a device failure of any shard wins (lowest shard first);
// otherwise the reference's first-error result for the global index F, reported by the shard that owns it.
static ndi_status shards_failed(const std::vector<ShardOutcome>& out) {
  for (size_t i = 0; i < out.size(); ++i)
    if (out[i].st != NDI_OK) return fail(out[i].st, "shard %zu: %s", i, out[i].msg.c_str());
  return NDI_OK;
}
static uint32_t shard_owner(uint64_t nq, uint32_t n, uint64_t index) {
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t lo, hi;
    shard_range(nq, i, n, &lo, &hi);
    if (index >= lo && index < hi) return i;
  }
  return n - 1;
}

template <class Impl>
static ndi_status sharded_float(Job<Impl>& J, ndi_oob_info* info) {
  ShardedCallScope scope;
  if (scope.nested)
    return fail(NDI_BAD_ARG, "nested sharded call: this host thread is inside a sharded evaluation (e.g. its ring "
                "consumer); issue the inner call from another thread");
  const uint32_t n = (uint32_t)J.H.size();
  std::vector<ShardOutcome> out(n);
  unsigned long long F[2];
  run_shards<Shard<Impl>>(J, n, out, F);
  ndi_status st = shards_failed(out);
  const unsigned long long f = std::min(F[0], F[1]);
  if (st != NDI_OK || f == NO_FAIL) return st;
  const uint32_t w = shard_owner(J.nq, n, f);
  const uint64_t lo = shard_lo(J.nq, w, n);
  DeviceGuard dg(J.H[w]->device);
  // indices relative to the owner's block; an axis whose first failure lies in a later shard stays larger
  const FirstFail rel{F[0] == NO_FAIL ? NO_FAIL : F[0] - lo, F[1] == NO_FAIL ? NO_FAIL : F[1] - lo};
  return J.H[w]->report(J.q_src(w, n), J.o.q_memspace, rel, lo, info);
}

// ---------------------------------------------------------------------------------------------
// the host engine the narrow element types share (integer and half handles below)
// ---------------------------------------------------------------------------------------------
#include "narrow_host.hpp"

// ---------------------------------------------------------------------------------------------
// integer element types (i32 / i64): Linear and Bilinear
// ---------------------------------------------------------------------------------------------
#include "int_host.hpp"

// ---------------------------------------------------------------------------------------------
// half-precision element types (f16 / bf16): Linear and Bilinear
// ---------------------------------------------------------------------------------------------
#include "half_host.hpp"

}  // namespace ndi

// =============================================================================================
// extern "C"
// =============================================================================================
namespace ndi {
// Checked build (-DNDI_BOUNDS): what the device-side index checks recorded since the last look (kernels.hpp,
// NDI_CHK).  Called where an entry point returns; reading the device word synchronises the device, which is fine
// for a debugging build.  A recorded violation turns any status into NDI_HIP_ERROR with the first violation's
// code, source line, index and limit.
static ndi_status bounds_verdict(ndi_status st, int device) {
#ifdef NDI_BOUNDS
  try {
    DeviceGuard dg(device);
    unsigned long long w[4] = {0, 0, 0, 0};
    NDI_HIP(hipMemcpyFromSymbol(w, HIP_SYMBOL(g_ndi_bounds), sizeof(w)));
    if (w[0] != 0) {
      const unsigned long long z[4] = {0, 0, 0, 0};
      NDI_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_ndi_bounds), z, sizeof(z)));
      return fail(NDI_HIP_ERROR, "device bounds check failed: %llu violation(s); first: code %u at kernels.hpp:%u, "
                  "index %llu, limit %llu", w[0], (unsigned)(w[1] >> 32), (unsigned)(w[1] & 0xffffffffu), w[2], w[3]);
    }
  } catch (const HipFailure& f) {
    return from_hip(f);
  }
#else
  (void)device;
#endif
  return st;
}
}  // namespace ndi

struct ndi_interp1d { ndi::Interp1DBase* impl; };
struct ndi_interp2d { ndi::Interp2DBase* impl; };
struct ndi_locator { ndi::LocatorBase* impl; };
struct ndi_interp3d { ndi::Interp3DBase* impl; };

#define NDI_TRY try {
#define NDI_CATCH                                                                  \
  }                                                                                \
  catch (const ndi::HipFailure& f) { return ndi::from_hip(f); }                    \
  catch (const std::bad_alloc&) { return ndi::fail(NDI_HIP_ERROR, "host out of memory"); } \
  catch (...) { return ndi::fail(NDI_HIP_ERROR, "unexpected C++ exception"); }

static ndi_status need_device(int device) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0)
    return ndi::fail(NDI_HIP_ERROR, "no HIP device available (%s); this library has no CPU fallback",
                     e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  if (device < 0 || device >= cnt)
    return ndi::fail(NDI_BAD_ARG, "device ordinal %d out of range [0, %d)", device, cnt);
  return NDI_OK;
}

static const char* strategy1d_name(int strategy) {
  switch (strategy) {
    case NDI_LINEAR: return "Linear";
    case NDI_CUBIC_SPLINE: return "CubicSpline";
    case NDI_PCHIP: return "Pchip";
    case NDI_AKIMA: return "Akima";
    case NDI_CUBIC_HERMITE: return "CubicHermite";
  }
  return "?";
}

// ndi_interp1d_create (dydx == nullptr) and ndi_interp1d_create_hermite.  Every check that needs no device comes first,
// so it behaves the same everywhere.
static ndi_status create1d_checked(const ndi_interp1d_desc* desc, const void* dydx, bool hermite_entry, ndi_interp1d** out) {
  if (!desc || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  if (desc->dtype < NDI_F32 || desc->dtype > NDI_BF16) return ndi::fail(NDI_BAD_ARG, "unknown dtype");
  if (desc->strategy < NDI_LINEAR || desc->strategy > NDI_CUBIC_HERMITE)
    return ndi::fail(NDI_BAD_ARG, "unknown strategy");
  if (hermite_entry && desc->strategy != NDI_CUBIC_HERMITE)
    return ndi::fail(NDI_BAD_ARG, "ndi_interp1d_create_hermite builds NDI_CUBIC_HERMITE only (strategy %d: %s takes "
                     "ndi_interp1d_create)", (int)desc->strategy, strategy1d_name(desc->strategy));
  if (!hermite_entry && desc->strategy == NDI_CUBIC_HERMITE)
    return ndi::fail(NDI_BAD_ARG, "CubicHermite needs the knot derivatives: build it with ndi_interp1d_create_hermite");
  const bool local_cubic = desc->strategy >= NDI_PCHIP;
  const char* name = strategy1d_name(desc->strategy);
  const bool int_t = desc->dtype == NDI_I32 || desc->dtype == NDI_I64;
  if (int_t && desc->strategy == NDI_CUBIC_SPLINE)
    return ndi::fail(NDI_BAD_ARG, "CubicSpline needs a float element type (f32 / f64): the reference's trait bounds "
                     "rule out integer splines; integer data takes Linear");
  if (int_t && local_cubic)
    return ndi::fail(NDI_BAD_ARG, "%s needs a float element type (f32 / f64); integer data takes Linear", name);
  const bool half_t = desc->dtype == NDI_F16 || desc->dtype == NDI_BF16;
  if (half_t && desc->strategy == NDI_CUBIC_SPLINE)
    return ndi::fail(NDI_BAD_ARG, "CubicSpline needs f32 / f64: the reference's SplineNum bounds (Pow, ScalarOperand, "
                     "Euclid) rule out f16 / bf16 splines; half-precision data takes Linear");
  if (half_t && local_cubic)
    return ndi::fail(NDI_BAD_ARG, "%s needs f32 / f64; half-precision data takes Linear", name);
  if (local_cubic) {   // the spline's notions do not apply
    if (desc->periodic) return ndi::fail(NDI_BAD_ARG, "%s has no periodic mode (periodic must be 0)", name);
    if (desc->build_flags) return ndi::fail(NDI_BAD_ARG, "%s takes no build_flags (NDI_BUILD_REFERENCE_ORDER is the spline's)", name);
    if (desc->left.kind || desc->left.value != 0.0 || desc->right.kind || desc->right.value != 0.0)
      return ndi::fail(NDI_BAD_ARG, "%s takes no boundary condition (left / right must be zero)", name);
    if (desc->lane_left_kind || desc->lane_left_value || desc->lane_right_kind || desc->lane_right_value)
      return ndi::fail(NDI_BAD_ARG, "%s takes no per-lane boundary conditions (lane_* must be NULL)", name);
  }
  if (hermite_entry && !dydx) return ndi::fail(NDI_BAD_ARG, "null dydx pointer");
  // Builder checks that need no device come first, so they behave the same everywhere.
  if (desc->validate && desc->memspace == NDI_MEM_HOST && desc->x) {
    ndi_status st = ndi_validate1d(desc->dtype, desc->x, desc->x_len, desc->n, desc->strategy);
    if (st != NDI_OK) return st;
  } else if (desc->validate && !desc->x && desc->n < ndi::min_len_1d(desc->strategy)) {
    return ndi::fail(NDI_NOT_ENOUGH_DATA, "The chosen Interpolation strategy needs at least %llu data points",
                     (unsigned long long)ndi::min_len_1d(desc->strategy));
  }
  ndi_status ds = need_device(desc->device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::Interp1DBase* impl = nullptr;
  ndi_interp1d_desc dd = *desc;
  dd.build_flags &= ~ndi::BUILD_TRUE_NOT_A_KNOT;   // internal to the Bicubic axis passes: as before, unknown bits do nothing
  ndi_status st = desc->dtype == NDI_F32   ? ndi::create1d<float>(dd, &impl, dydx)
                  : desc->dtype == NDI_F64 ? ndi::create1d<double>(dd, &impl, dydx)
                  : desc->dtype == NDI_I32 ? ndi::create1d_int<int32_t>(dd, &impl)
                  : desc->dtype == NDI_I64 ? ndi::create1d_int<int64_t>(dd, &impl)
                  : desc->dtype == NDI_F16 ? ndi::create1d_half<ndi::HF_F16>(dd, &impl)
                                           : ndi::create1d_half<ndi::HF_BF16>(dd, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp1d{impl};
  return NDI_OK;
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_create(const ndi_interp1d_desc* desc, ndi_interp1d** out) {
  return create1d_checked(desc, nullptr, false, out);
}

NDI_API ndi_status ndi_interp1d_create_hermite(const ndi_interp1d_desc* desc, const void* dydx, ndi_interp1d** out) {
  return create1d_checked(desc, dydx, true, out);
}

// ndi_interp1d_create_lane_axes: every check that needs no device comes first -- for host arrays the column validation too.
NDI_API ndi_status ndi_interp1d_create_lane_axes(const ndi_interp1d_desc* desc, const void* x_lanes, const void* dydx,
                                                 ndi_interp1d** out) {
  if (!desc || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  if (desc->dtype < NDI_F32 || desc->dtype > NDI_BF16) return ndi::fail(NDI_BAD_ARG, "unknown dtype");
  if (desc->dtype != NDI_F32 && desc->dtype != NDI_F64)
    return ndi::fail(NDI_UNSUPPORTED, "an x axis per lane needs f32 / f64 data: %s handles search one shared axis of widened "
                     "knots, which a knot column per lane does not have",
                     (desc->dtype == NDI_I32 || desc->dtype == NDI_I64) ? "integer" : "f16 / bf16");
  if (desc->strategy < NDI_LINEAR || desc->strategy > NDI_CUBIC_HERMITE) return ndi::fail(NDI_BAD_ARG, "unknown strategy");
  const char* name = strategy1d_name(desc->strategy);
  if (desc->x) return ndi::fail(NDI_BAD_ARG, "ndi_interp1d_create_lane_axes takes the knots as x_lanes: desc->x must be NULL");
  if (desc->x_len != desc->n)
    return ndi::fail(NDI_BAD_ARG, "desc->x_len (%llu) must equal desc->n (%llu): x_lanes has the data's shape",
                     (unsigned long long)desc->x_len, (unsigned long long)desc->n);
  if (desc->memspace != NDI_MEM_HOST && desc->memspace != NDI_MEM_DEVICE) return ndi::fail(NDI_BAD_ARG, "unknown memspace");
  if (!x_lanes) return ndi::fail(NDI_BAD_ARG, "null x_lanes pointer");
  if (!desc->data) return ndi::fail(NDI_BAD_ARG, "null data pointer");
  if (desc->lanes == 0) return ndi::fail(NDI_BAD_ARG, "lanes must be >= 1");
  if (desc->strategy == NDI_CUBIC_HERMITE && !dydx) return ndi::fail(NDI_BAD_ARG, "null dydx pointer (CubicHermite needs the knot derivatives)");
  if (desc->strategy != NDI_CUBIC_HERMITE && dydx) return ndi::fail(NDI_BAD_ARG, "%s takes no dydx (it must be NULL)", name);
  if (desc->periodic)
    return ndi::fail(NDI_UNSUPPORTED, "%s with an x axis per lane has no periodic mode: the periodic system and the wrapped "
                     "query need one period, and here every lane has its own end knots", name);
  if (desc->lane_left_kind || desc->lane_left_value || desc->lane_right_kind || desc->lane_right_value)
    return ndi::fail(NDI_UNSUPPORTED, "%s with an x axis per lane takes the global boundaries left / right only: "
                     "BoundaryCondition::Individual (the lane_* arrays) selects among elimination plans of ONE shared axis", name);
  if (desc->strategy == NDI_CUBIC_SPLINE) {
    for (const ndi_boundary* bd : {&desc->left, &desc->right})
      if (bd->kind < NDI_BC_NOT_A_KNOT || bd->kind > NDI_BC_SECOND_DERIV) return ndi::fail(NDI_BAD_ARG, "unknown boundary kind %d", (int)bd->kind);
  } else if (desc->strategy != NDI_LINEAR) {
    if (desc->left.kind || desc->left.value != 0.0 || desc->right.kind || desc->right.value != 0.0)
      return ndi::fail(NDI_BAD_ARG, "%s takes no boundary condition (left / right must be zero)", name);
  }
  if (desc->n < ndi::min_len_1d(desc->strategy))
    return ndi::fail(NDI_NOT_ENOUGH_DATA, "The chosen Interpolation strategy needs at least %llu data points",
                     (unsigned long long)ndi::min_len_1d(desc->strategy));
  if (desc->n > ndi::MAX_KNOTS) return ndi::fail(NDI_UNSUPPORTED, "more than %llu knots", (unsigned long long)ndi::MAX_KNOTS);
  if (desc->memspace == NDI_MEM_HOST) {
    const ndi_status vs = desc->dtype == NDI_F32
                              ? ndi::check_lane_axes(static_cast<const float*>(x_lanes), desc->n, desc->lanes, desc->strategy)
                              : ndi::check_lane_axes(static_cast<const double*>(x_lanes), desc->n, desc->lanes, desc->strategy);
    if (vs != NDI_OK) return vs;
  }
  ndi_status ds = need_device(desc->device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::Interp1DBase* impl = nullptr;
  ndi_status st = desc->dtype == NDI_F32 ? ndi::create_lane_axes<float>(*desc, x_lanes, dydx, &impl)
                                         : ndi::create_lane_axes<double>(*desc, x_lanes, dydx, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp1d{impl};
  return ndi::bounds_verdict(NDI_OK, impl->device);
  NDI_CATCH
}

NDI_API void ndi_interp1d_destroy(ndi_interp1d* h) {
  if (!h) return;
  try {
    ndi::DeviceGuard dg(h->impl->device);
    delete h->impl;
  } catch (...) {
  }
  delete h;
}

NDI_API ndi_status ndi_interp2d_create(const ndi_interp2d_desc* desc, ndi_interp2d** out) {
  if (!desc || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  if (desc->dtype < NDI_F32 || desc->dtype > NDI_BF16) return ndi::fail(NDI_BAD_ARG, "unknown dtype");
  if (desc->validate && desc->memspace == NDI_MEM_HOST && desc->x && desc->y) {
    ndi_status st = ndi_validate2d(desc->dtype, desc->x, desc->x_len, desc->y, desc->y_len, desc->nx, desc->ny);
    if (st != NDI_OK) return st;
  }
  ndi_status ds = need_device(desc->device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::Interp2DBase* impl = nullptr;
  ndi_status st = desc->dtype == NDI_F32   ? ndi::create2d<float>(*desc, &impl)
                  : desc->dtype == NDI_F64 ? ndi::create2d<double>(*desc, &impl)
                  : desc->dtype == NDI_I32 ? ndi::create2d_int<int32_t>(*desc, &impl)
                  : desc->dtype == NDI_I64 ? ndi::create2d_int<int64_t>(*desc, &impl)
                  : desc->dtype == NDI_F16 ? ndi::create2d_half<ndi::HF_F16>(*desc, &impl)
                                           : ndi::create2d_half<ndi::HF_BF16>(*desc, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp2d{impl};
  return NDI_OK;
  NDI_CATCH
}

// Every refusal is decided before any device work, so it behaves the same everywhere.  `periodic_axes` < 0: the plain
// entry point (no periodic argument to check).
static ndi_status create_bicubic_spline(const ndi_interp2d_desc* desc, const ndi_boundary* bc, int periodic_axes,
                                        ndi_interp2d** out) {
  if (!desc || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  if (desc->dtype < NDI_F32 || desc->dtype > NDI_BF16) return ndi::fail(NDI_BAD_ARG, "unknown dtype");
  if (desc->dtype == NDI_I32 || desc->dtype == NDI_I64)
    return ndi::fail(NDI_BAD_ARG, "Bicubic needs a float element type (f32 / f64): a spline divides; integer data takes Bilinear");
  if (desc->dtype == NDI_F16 || desc->dtype == NDI_BF16)
    return ndi::fail(NDI_BAD_ARG, "Bicubic needs f32 / f64: the spline build has no half-precision form; f16 / bf16 data takes "
                     "Bilinear");
  ndi_boundary b4[4] = {{NDI_BC_NOT_A_KNOT, 0.0}, {NDI_BC_NOT_A_KNOT, 0.0}, {NDI_BC_NOT_A_KNOT, 0.0}, {NDI_BC_NOT_A_KNOT, 0.0}};
  static const char* const END[4] = {"x-left", "x-right", "y-left", "y-right"};
  for (int k = 0; bc && k < 4; ++k) {
    b4[k] = bc[k];
    if (periodic_axes > 0 && ((periodic_axes >> (k / 2)) & 1)) {
      if (bc[k].kind != NDI_BC_NOT_A_KNOT || bc[k].value != 0.0)
        return ndi::fail(NDI_BAD_ARG, "Bicubic: the %s axis is periodic and takes no boundary condition: a periodic end has no "
                         "kind, its bc entries must be {NDI_BC_NOT_A_KNOT, 0} (%s end: kind %d, value %g)", k < 2 ? "x" : "y",
                         END[k], (int)bc[k].kind, bc[k].value);
      continue;
    }
    if (bc[k].kind < NDI_BC_NOT_A_KNOT || bc[k].kind > NDI_BC_SECOND_DERIV)
      return ndi::fail(NDI_BAD_ARG, "Bicubic takes one non-periodic boundary kind with a scalar value per end (ndi_bc_kind); "
                       "periodic and per-lane boundaries are not provided (%s end: kind %d)", END[k], (int)bc[k].kind);
  }
  if (desc->validate && desc->memspace == NDI_MEM_HOST && desc->x && desc->y) {
    ndi_status st = ndi_validate2d(desc->dtype, desc->x, desc->x_len, desc->y, desc->y_len, desc->nx, desc->ny);
    if (st != NDI_OK) return st;
  }
  if (desc->nx < 3 || desc->ny < 3)
    return ndi::fail(NDI_NOT_ENOUGH_DATA, "Bicubic needs at least 3 data points on each axis (got %llu x %llu)",
                     (unsigned long long)desc->nx, (unsigned long long)desc->ny);
  ndi_status ds = need_device(desc->device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  const int per = periodic_axes > 0 ? periodic_axes : 0;
  ndi::Interp2DBase* impl = nullptr;
  ndi_status st = desc->dtype == NDI_F32 ? ndi::create2d_bicubic<float>(*desc, b4, &impl, per)
                                         : ndi::create2d_bicubic<double>(*desc, b4, &impl, per);
  if (st != NDI_OK) return st;
  *out = new ndi_interp2d{impl};
  return ndi::bounds_verdict(NDI_OK, impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_create_bicubic(const ndi_interp2d_desc* desc, const ndi_boundary* bc, ndi_interp2d** out) {
  return create_bicubic_spline(desc, bc, -1, out);
}

// Bicubic with periodic axes (bit 0 of periodic_axes: x, bit 1: y); with no bit set it is the call above.
NDI_API ndi_status ndi_interp2d_create_bicubic_periodic(const ndi_interp2d_desc* desc, const ndi_boundary* bc,
                                                        int32_t periodic_axes, ndi_interp2d** out) {
  if (out) *out = nullptr;
  if (periodic_axes < 0 || periodic_axes > 3)
    return ndi::fail(NDI_BAD_ARG, "Bicubic: periodic_axes is a bit set of 1 (x) and 2 (y): 0 .. 3, got %d", (int)periodic_axes);
  return create_bicubic_spline(desc, bc, periodic_axes, out);
}

// The Bicubic handles of a local rule (Pchip, Akima) and of caller-given node derivatives: bicubic_local_host.hpp.
// Every refusal is decided before any device work.  `rule`: HR_PCHIP, HR_AKIMA or HR_GIVEN.
static ndi_status create_bicubic_local(const char* name, const ndi_interp2d_desc* desc, int rule, const void* zx, const void* zy,
                                       const void* zxy, ndi_interp2d** out) {
  if (desc->dtype < NDI_F32 || desc->dtype > NDI_BF16) return ndi::fail(NDI_BAD_ARG, "unknown dtype");
  if (desc->dtype == NDI_I32 || desc->dtype == NDI_I64)
    return ndi::fail(NDI_BAD_ARG, "Bicubic (%s) needs a float element type (f32 / f64): the rule divides; integer data takes "
                     "Bilinear", name);
  if (desc->dtype == NDI_F16 || desc->dtype == NDI_BF16)
    return ndi::fail(NDI_BAD_ARG, "Bicubic (%s) needs f32 / f64: the node build has no half-precision form; f16 / bf16 data "
                     "takes Bilinear", name);
  if (rule == ndi::HR_GIVEN && (!zx || !zy || !zxy))
    return ndi::fail(NDI_BAD_ARG, "Bicubic (%s) needs all three node derivative tables: %s is null", name,
                     !zx ? "zx" : !zy ? "zy" : "zxy");
  if (desc->validate && desc->memspace == NDI_MEM_HOST && desc->x && desc->y) {
    ndi_status st = ndi_validate2d(desc->dtype, desc->x, desc->x_len, desc->y, desc->y_len, desc->nx, desc->ny);
    if (st != NDI_OK) return st;
  }
  const unsigned long long need = rule == ndi::HR_AKIMA ? 3 : 2;
  if (desc->nx < need || desc->ny < need)
    return ndi::fail(NDI_NOT_ENOUGH_DATA, "Bicubic (%s) needs at least %llu data points on each axis (got %llu x %llu)", name,
                     need, (unsigned long long)desc->nx, (unsigned long long)desc->ny);
  ndi_status ds = need_device(desc->device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::Interp2DBase* impl = nullptr;
  ndi_status st = desc->dtype == NDI_F32 ? ndi::create2d_bicubic_local<float>(*desc, rule, zx, zy, zxy, &impl)
                                         : ndi::create2d_bicubic_local<double>(*desc, rule, zx, zy, zxy, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp2d{impl};
  return ndi::bounds_verdict(NDI_OK, impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_create_bicubic_local(const ndi_interp2d_desc* desc, int32_t rule, ndi_interp2d** out) {
  if (!desc || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  if (rule != NDI_PCHIP && rule != NDI_AKIMA)
    return ndi::fail(NDI_BAD_ARG, "Bicubic (local rule) takes NDI_PCHIP or NDI_AKIMA as its rule (ndi_strategy1d), got %d: the "
                     "spline is ndi_interp2d_create_bicubic, caller-given derivatives ndi_interp2d_create_bicubic_hermite",
                     (int)rule);
  return rule == NDI_PCHIP ? create_bicubic_local("Pchip", desc, ndi::HR_PCHIP, nullptr, nullptr, nullptr, out)
                           : create_bicubic_local("Akima", desc, ndi::HR_AKIMA, nullptr, nullptr, nullptr, out);
}

NDI_API ndi_status ndi_interp2d_create_bicubic_hermite(const ndi_interp2d_desc* desc, const void* zx, const void* zy,
                                                       const void* zxy, ndi_interp2d** out) {
  if (!desc || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  return create_bicubic_local("Hermite", desc, ndi::HR_GIVEN, zx, zy, zxy, out);
}

NDI_API ndi_status ndi_interp2d_tables(const ndi_interp2d* h, void* zx, void* zy, void* zxy, int32_t memspace) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if (memspace != NDI_MEM_HOST && memspace != NDI_MEM_DEVICE) return ndi::fail(NDI_BAD_ARG, "unknown memspace");
  NDI_TRY
  if (!h->impl->bicubic) return h->impl->tables(zx, zy, zxy, memspace);
  return ndi::bounds_verdict(h->impl->tables(zx, zy, zxy, memspace), h->impl->device);
  NDI_CATCH
}

// Every refusal is decided before any device work: the null checks here, the handle's own in Interp2DImpl::partial.
NDI_API ndi_status ndi_interp2d_partial(const ndi_interp2d* h, int32_t nu_x, int32_t nu_y, ndi_interp2d** out) {
  if (!out) return ndi::fail(NDI_BAD_ARG, "null out pointer");
  *out = nullptr;
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  ndi::Range rg("ndi_interp2d_partial");
  ndi::Interp2DBase* impl = nullptr;
  ndi_status st = h->impl->partial(nu_x, nu_y, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp2d{impl};
  return NDI_OK;
  NDI_CATCH
}

// Every refusal is decided before any device work: the null checks here, the handle's own in Interp2DImpl::antiderivative.
NDI_API ndi_status ndi_interp2d_antiderivative(const ndi_interp2d* h, ndi_interp2d** out) {
  if (!out) return ndi::fail(NDI_BAD_ARG, "null out pointer");
  *out = nullptr;
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  ndi::Range rg("ndi_interp2d_antiderivative");
  ndi::Interp2DBase* impl = nullptr;
  ndi_status st = h->impl->antiderivative(&impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp2d{impl};
  return ndi::bounds_verdict(NDI_OK, impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_integral(const ndi_interp2d* h, const void* xa, const void* xb, const void* ya, const void* yb,
                                         uint64_t nq, void* out, uint64_t out_row_stride, const ndi_eval_opts* opts,
                                         ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  if (!h->impl->integral) return h->impl->integral_rect(xa, xb, ya, yb, nq, out, out_row_stride, opts, info);
  return ndi::bounds_verdict(h->impl->integral_rect(xa, xb, ya, yb, nq, out, out_row_stride, opts, info), h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_integral_tables(const ndi_interp2d* h, void* pp, void* qz, void* qzy, void* pz, void* pzx,
                                                int32_t memspace) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if (memspace != NDI_MEM_HOST && memspace != NDI_MEM_DEVICE) return ndi::fail(NDI_BAD_ARG, "unknown memspace");
  NDI_TRY
  void* const dst[5] = {pp, qz, qzy, pz, pzx};
  if (!h->impl->integral) return h->impl->integral_tables(dst, memspace);
  return ndi::bounds_verdict(h->impl->integral_tables(dst, memspace), h->impl->device);
  NDI_CATCH
}

// Every refusal is decided before any device work: the null checks here, the handle's kind in Interp2DImpl::eval_jet, the
// rest at the top of bicubic_jet_eval.
NDI_API ndi_status ndi_interp2d_eval_jet(const ndi_interp2d* h, int32_t order, const void* qx, const void* qy, uint64_t nq,
                                         void* const* outs, uint64_t out_row_stride, const ndi_eval_opts* opts,
                                         ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if (!outs) return ndi::fail(NDI_BAD_ARG, "null outs pointer (ndi_interp2d_eval_jet takes a host array of part pointers)");
  NDI_TRY
  if (!h->impl->bicubic) return h->impl->eval_jet(order, qx, qy, nq, outs, out_row_stride, opts, info);
  return ndi::bounds_verdict(h->impl->eval_jet(order, qx, qy, nq, outs, out_row_stride, opts, info), h->impl->device);
  NDI_CATCH
}

// Bicubic has one evaluation form: NDI_PATH_BUCKETED (the tile-grouped order) is Bilinear's.
static ndi_status bicubic_path_check(const ndi_interp2d* h, const ndi_eval_opts* opts) {
  if (h->impl->bicubic && opts && opts->path == NDI_PATH_BUCKETED)
    return ndi::fail(NDI_BAD_ARG, "Bicubic has no tile-grouped evaluation form: NDI_PATH_BUCKETED is Bilinear's (AUTO and "
                     "GATHER evaluate)");
  return NDI_OK;
}

NDI_API void ndi_interp2d_destroy(ndi_interp2d* h) {
  if (!h) return;
  try {
    ndi::DeviceGuard dg(h->impl->device);
    delete h->impl;
  } catch (...) {
  }
  delete h;
}

NDI_API ndi_status ndi_interp1d_clone(const ndi_interp1d* h, int32_t device, ndi_interp1d** out) {
  if (!h || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  ndi_status ds = need_device(device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::Range rg("ndi_interp1d_clone");
  ndi::Interp1DBase* impl = nullptr;
  ndi_status st = h->impl->clone_to(device, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp1d{impl};
  return NDI_OK;
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_clone(const ndi_interp2d* h, int32_t device, ndi_interp2d** out) {
  if (!h || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  ndi_status ds = need_device(device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::Range rg("ndi_interp2d_clone");
  ndi::Interp2DBase* impl = nullptr;
  ndi_status st = h->impl->clone_to(device, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp2d{impl};
  return NDI_OK;
  NDI_CATCH
}

// Every refusal is decided before any device work: the argument checks here, the handle's own in Interp1D*Impl::derivative.
NDI_API ndi_status ndi_interp1d_derivative(const ndi_interp1d* h, int32_t nu, ndi_interp1d** out) {
  if (!out) return ndi::fail(NDI_BAD_ARG, "null out pointer");
  *out = nullptr;
  if (nu < 1) return ndi::fail(NDI_BAD_ARG, "nu = %d: the derivative order must be 1 or 2", (int)nu);
  if (nu > 2)
    return ndi::fail(NDI_BAD_ARG, "nu = %d: the third and higher derivatives of a piecewise cubic jump at the knots, and a "
                     "handle's tables hold one value per knot (orders 1 and 2 only)", (int)nu);
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  ndi::Interp1DBase* impl = nullptr;
  ndi_status st = h->impl->derivative(nu, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp1d{impl};
  return NDI_OK;
  NDI_CATCH
}

// Every refusal is decided before any device work: the argument checks here, the handle's own in its antiderivative().
NDI_API ndi_status ndi_interp1d_antiderivative(const ndi_interp1d* h, ndi_interp1d** out) {
  if (!out) return ndi::fail(NDI_BAD_ARG, "null out pointer");
  *out = nullptr;
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  ndi::Interp1DBase* impl = nullptr;
  ndi_status st = h->impl->antiderivative(&impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp1d{impl};
  return ndi::bounds_verdict(NDI_OK, impl->device);
  NDI_CATCH
}

// Every refusal is decided before any device work: the argument checks here, the handle's own in its inverse().
NDI_API ndi_status ndi_interp1d_inverse(const ndi_interp1d* h, ndi_interp1d** out) {
  if (!out) return ndi::fail(NDI_BAD_ARG, "null out pointer");
  *out = nullptr;
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  ndi::Range rg("ndi_interp1d_inverse");
  ndi::Interp1DBase* impl = nullptr;
  ndi_status st = h->impl->inverse(&impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp1d{impl};
  return ndi::bounds_verdict(NDI_OK, impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_integrate(const ndi_interp1d* h, const void* lo, const void* hi, uint64_t nq, void* out,
                                          uint64_t out_row_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  if (!h->impl->is_antiderivative()) return h->impl->integrate(lo, hi, nq, out, out_row_stride, opts, info);
  return ndi::bounds_verdict(h->impl->integrate(lo, hi, nq, out, out_row_stride, opts, info), h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_data(const ndi_interp1d* h, void* data_out, int32_t memspace) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if (!data_out) return ndi::fail(NDI_BAD_ARG, "null data_out pointer");
  if (memspace != NDI_MEM_HOST && memspace != NDI_MEM_DEVICE) return ndi::fail(NDI_BAD_ARG, "unknown memspace");
  NDI_TRY
  return h->impl->data_table(data_out, memspace);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_coefficients(const ndi_interp1d* h, void* a_out, void* b_out, int32_t memspace) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return h->impl->coefficients(a_out, b_out, memspace);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_eval(const ndi_interp1d* h, const void* q, uint64_t nq, void* out,
                                     uint64_t out_row_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return ndi::bounds_verdict(h->impl->eval(q, nq, out, out_row_stride, opts, info), h->impl->device);
  NDI_CATCH
}

// Every refusal is decided before any device work: the null handle here, the rest in the handle's eval_lanewise().
NDI_API ndi_status ndi_interp1d_eval_lanewise(const ndi_interp1d* h, const void* q, uint64_t nq, uint64_t q_row_stride,
                                              void* out, uint64_t out_row_stride, const ndi_eval_opts* opts,
                                              ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  const ndi_status st = h->impl->eval_lanewise(q, nq, q_row_stride, out, out_row_stride, opts, info);
  if (st == NDI_BAD_ARG || st == NDI_UNSUPPORTED) return st;   // a refusal: no device was touched
  return ndi::bounds_verdict(st, h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_eval(const ndi_interp2d* h, const void* qx, const void* qy, uint64_t nq,
                                     void* out, uint64_t out_row_stride, const ndi_eval_opts* opts,
                                     ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if (const ndi_status ps = bicubic_path_check(h, opts); ps != NDI_OK) return ps;
  NDI_TRY
  return ndi::bounds_verdict(h->impl->eval(qx, qy, nq, out, out_row_stride, opts, info), h->impl->device);
  NDI_CATCH
}

// Every refusal is decided before any device work: the null handle here, the rest in the handle's eval_lanewise().
NDI_API ndi_status ndi_interp2d_eval_lanewise(const ndi_interp2d* h, const void* qx, const void* qy, uint64_t nq,
                                              uint64_t q_row_stride, void* out, uint64_t out_row_stride,
                                              const ndi_eval_opts* opts, ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  const ndi_status st = h->impl->eval_lanewise(qx, qy, nq, q_row_stride, out, out_row_stride, opts, info);
  if (st == NDI_BAD_ARG || st == NDI_UNSUPPORTED) return st;   // a refusal: no device was touched
  return ndi::bounds_verdict(st, h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_finish(const ndi_interp1d* h, void* stream, ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return ndi::bounds_verdict(h->impl->finish(stream, info), h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_finish(const ndi_interp2d* h, void* stream, ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return ndi::bounds_verdict(h->impl->finish(stream, info), h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_eval_ring(const ndi_interp1d* h, const void* q, uint64_t nq,
                                          const ndi_ring_desc* ring, ndi_ring_consumer consume, void* user,
                                          const ndi_eval_opts* opts, ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return ndi::bounds_verdict(h->impl->eval_ring(q, nq, ring, consume, user, opts, info), h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_eval_ring(const ndi_interp2d* h, const void* qx, const void* qy, uint64_t nq,
                                          const ndi_ring_desc* ring, ndi_ring_consumer consume, void* user,
                                          const ndi_eval_opts* opts, ndi_oob_info* info) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if (const ndi_status ps = bicubic_path_check(h, opts); ps != NDI_OK) return ps;
  NDI_TRY
  return ndi::bounds_verdict(h->impl->eval_ring(qx, qy, nq, ring, consume, user, opts, info), h->impl->device);
  NDI_CATCH
}

// ---- sharded evaluation ------------------------------------------------------------------------
NDI_API void ndi_shard_bounds(uint64_t nq, uint32_t shard, uint32_t n_shards, uint64_t* lo, uint64_t* hi) {
  uint64_t l = 0, h = 0;
  if (n_shards && shard < n_shards) ndi::shard_range(nq, shard, n_shards, &l, &h);
  if (lo) *lo = l;
  if (hi) *hi = h;
}

template <class Impl, class Handle>
static ndi_status gather_handles(const Handle* const* handles, uint32_t n, int dtype, std::vector<Impl*>& out) {
  out.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (handles[i]->impl->dtype != dtype || handles[i]->impl->lanes != handles[0]->impl->lanes)
      return ndi::fail(NDI_BAD_ARG, "shard %u: the handles of a sharded call must be replicas (same element type "
                       "and trailing lanes)", i);
    // ... and the same knots, strategy and extrapolation mode: every shard range-checks and evaluates with its own
    // handle, so a mismatched set would mix interpolators and report a first-error index no serial loop produces
    if (i > 0 && handles[i]->impl->signature() != handles[0]->impl->signature())
      return ndi::fail(NDI_BAD_ARG, "shard %u: the handles of a sharded call must be replicas of one interpolator "
                       "(same knots, strategy and extrapolation mode as shard 0)", i);
    out[i] = static_cast<Impl*>(handles[i]->impl);
  }
  return NDI_OK;
}

template <class Handle>
static ndi_status check_sharded_args(const Handle* const* handles, uint32_t n, const void* q, const void* qy,
                                     bool two_d, uint64_t nq, const ndi_shard_io* io, bool need_out,
                                     const ndi_ring_desc* rings, bool need_rings, uint64_t out_stride) {
  if (!handles || n == 0) return ndi::fail(NDI_BAD_ARG, "a sharded call needs at least one handle");
  for (uint32_t i = 0; i < n; ++i)
    if (!handles[i]) return ndi::fail(NDI_BAD_ARG, "shard %u: null handle", i);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < i; ++j)
      if (handles[i] == handles[j]) return ndi::fail(NDI_BAD_ARG, "shards %u and %u share one handle", j, i);
  const uint64_t lanes = handles[0]->impl->lanes;
  if (need_out && !io) return ndi::fail(NDI_BAD_ARG, "null shard io array");
  if (need_out && out_stride < lanes)
    return ndi::fail(NDI_BAD_ARG, "out_row_stride (%llu) < lanes (%llu)", (unsigned long long)out_stride,
                     (unsigned long long)lanes);
  if (need_rings && !rings) return ndi::fail(NDI_BAD_ARG, "null ring array");
  for (uint32_t i = 0; i < n && nq; ++i) {
    uint64_t lo, hi;
    ndi::shard_range(nq, i, n, &lo, &hi);
    const bool own_q = io && io[i].q;
    if (two_d && io && ((io[i].q != nullptr) != (io[i].qy != nullptr)))
      return ndi::fail(NDI_BAD_ARG, "shard %u: q and qy must be given together", i);
    if (!own_q && (!q || (two_d && !qy))) return ndi::fail(NDI_BAD_ARG, "null query pointer");
    if (need_out && hi > lo && !io[i].out) return ndi::fail(NDI_BAD_ARG, "shard %u: null output pointer", i);
    if (need_rings) {
      uint64_t stride = 0;
      ndi_status st = ndi::check_ring_desc(&rings[i], lanes, &stride);
      if (st != NDI_OK) return st;
    }
  }
  return NDI_OK;
}

// One sharded call of handles whose implementation is Impl, a NarrowEngine (integer and half handles).
template <class Impl, class Handle>
static ndi_status sharded_narrow_call(const Handle* const* handles, uint32_t n, const ndi::ShardCall& c,
                                      ndi_oob_info* info) {
  std::vector<Impl*> H;
  const ndi_status st = gather_handles(handles, n, handles[0]->impl->dtype, H);
  if (st != NDI_OK) return st;
  return ndi::sharded_narrow(std::vector<ndi::NarrowEngine<typename Impl::Elem>*>(H.begin(), H.end()), c, info);
}

// One sharded call of f32 / f64 handles whose implementation is Impl, a FloatEngine.
template <class Impl, class Handle>
static ndi_status sharded_float_call(const Handle* const* handles, uint32_t n, const ndi::ShardCall& c, ndi_oob_info* info) {
  ndi::Job<Impl> J(c);
  const ndi_status st = gather_handles(handles, n, handles[0]->impl->dtype, J.H);
  return st != NDI_OK ? st : ndi::sharded_float(J, info);
}

// The element type of a sharded call is the first handle's (gather_handles holds the others to it).
static ndi_status sharded_call(const ndi_interp1d* const* handles, uint32_t n, const ndi::ShardCall& c,
                               ndi_oob_info* info) {
  const int dtype = handles[0]->impl->dtype;
  // antiderivative handles take no sharded call; a set that mixes a function with its antiderivative is no set of
  // replicas at all (the signatures differ), which is the first thing to say about it
  bool anti = false, inv = false, lax = false;
  for (uint32_t i = 0; i < n; ++i) {
    anti = anti || handles[i]->impl->is_antiderivative();
    inv = inv || handles[i]->impl->inverse_handle;
    lax = lax || handles[i]->impl->lane_axes_handle;
  }
  if (anti || inv || lax) {
    std::vector<ndi::Interp1DBase*> H;
    const ndi_status st = gather_handles(handles, n, dtype, H);
    if (st != NDI_OK) return st;
    return ndi::fail(NDI_UNSUPPORTED, "the sharded calls do not take %s handles (ndi_interp1d_eval per device serves them)",
                     lax ? "lane-axes" : inv ? "inverse" : "antiderivative");
  }
  switch (dtype) {
    case NDI_I32: return sharded_narrow_call<ndi::Interp1DIntImpl<int32_t>>(handles, n, c, info);
    case NDI_I64: return sharded_narrow_call<ndi::Interp1DIntImpl<int64_t>>(handles, n, c, info);
    case NDI_F16: return sharded_narrow_call<ndi::Interp1DHalfImpl<ndi::HF_F16>>(handles, n, c, info);
    case NDI_BF16: return sharded_narrow_call<ndi::Interp1DHalfImpl<ndi::HF_BF16>>(handles, n, c, info);
    case NDI_F32: return sharded_float_call<ndi::Interp1DImpl<float>>(handles, n, c, info);
  }
  return sharded_float_call<ndi::Interp1DImpl<double>>(handles, n, c, info);
}

static ndi_status sharded_call(const ndi_interp2d* const* handles, uint32_t n, const ndi::ShardCall& c,
                               ndi_oob_info* info) {
  const int dtype = handles[0]->impl->dtype;
  for (uint32_t i = 0; i < n; ++i)
    if (const ndi_status ps = bicubic_path_check(handles[i], &c.o); ps != NDI_OK) return ps;
  switch (dtype) {
    case NDI_I32: return sharded_narrow_call<ndi::Interp2DIntImpl<int32_t>>(handles, n, c, info);
    case NDI_I64: return sharded_narrow_call<ndi::Interp2DIntImpl<int64_t>>(handles, n, c, info);
    case NDI_F16: return sharded_narrow_call<ndi::Interp2DHalfImpl<ndi::HF_F16>>(handles, n, c, info);
    case NDI_BF16: return sharded_narrow_call<ndi::Interp2DHalfImpl<ndi::HF_BF16>>(handles, n, c, info);
    case NDI_F32: return sharded_float_call<ndi::Interp2DImpl<float>>(handles, n, c, info);
  }
  return sharded_float_call<ndi::Interp2DImpl<double>>(handles, n, c, info);
}

NDI_API ndi_status ndi_interp1d_eval_sharded(const ndi_interp1d* const* handles, uint32_t n_shards, const void* q,
                                             uint64_t nq, const ndi_shard_io* io, uint64_t out_row_stride,
                                             const ndi_eval_opts* opts, ndi_oob_info* info) {
  ndi_status st = check_sharded_args(handles, n_shards, q, nullptr, false, nq, io, true, nullptr, false, out_row_stride);
  if (st != NDI_OK || nq == 0) return st;
  NDI_TRY
  ndi::Range rg("ndi_interp1d_eval_sharded");
  ndi::ShardCall c{q, nullptr, nq, io, out_row_stride, nullptr, nullptr, nullptr, {}};
  if (const ndi_status vs__ = ndi::take_opts(opts, c.o); vs__ != NDI_OK) return vs__;
  return sharded_call(handles, n_shards, c, info);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_eval_ring_sharded(const ndi_interp1d* const* handles, uint32_t n_shards,
                                                  const void* q, uint64_t nq, const ndi_shard_io* io,
                                                  const ndi_ring_desc* rings, ndi_ring_consumer consume, void* user,
                                                  const ndi_eval_opts* opts, ndi_oob_info* info) {
  ndi_status st = check_sharded_args(handles, n_shards, q, nullptr, false, nq, io, false, rings, true, 0);
  if (st != NDI_OK || nq == 0) return st;
  NDI_TRY
  ndi::Range rg("ndi_interp1d_eval_ring_sharded");
  ndi::ShardCall c{q, nullptr, nq, io, 0, rings, consume, user, {}};
  if (const ndi_status vs__ = ndi::take_opts(opts, c.o); vs__ != NDI_OK) return vs__;
  return sharded_call(handles, n_shards, c, info);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_eval_sharded(const ndi_interp2d* const* handles, uint32_t n_shards, const void* qx,
                                             const void* qy, uint64_t nq, const ndi_shard_io* io,
                                             uint64_t out_row_stride, const ndi_eval_opts* opts,
                                             ndi_oob_info* info) {
  ndi_status st = check_sharded_args(handles, n_shards, qx, qy, true, nq, io, true, nullptr, false, out_row_stride);
  if (st != NDI_OK || nq == 0) return st;
  NDI_TRY
  ndi::Range rg("ndi_interp2d_eval_sharded");
  ndi::ShardCall c{qx, qy, nq, io, out_row_stride, nullptr, nullptr, nullptr, {}};
  if (const ndi_status vs__ = ndi::take_opts(opts, c.o); vs__ != NDI_OK) return vs__;
  return sharded_call(handles, n_shards, c, info);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_eval_ring_sharded(const ndi_interp2d* const* handles, uint32_t n_shards,
                                                  const void* qx, const void* qy, uint64_t nq,
                                                  const ndi_shard_io* io, const ndi_ring_desc* rings,
                                                  ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts,
                                                  ndi_oob_info* info) {
  ndi_status st = check_sharded_args(handles, n_shards, qx, qy, true, nq, io, false, rings, true, 0);
  if (st != NDI_OK || nq == 0) return st;
  NDI_TRY
  ndi::Range rg("ndi_interp2d_eval_ring_sharded");
  ndi::ShardCall c{qx, qy, nq, io, 0, rings, consume, user, {}};
  if (const ndi_status vs__ = ndi::take_opts(opts, c.o); vs__ != NDI_OK) return vs__;
  return sharded_call(handles, n_shards, c, info);
  NDI_CATCH
}

// ---- Interp3D (include/ndinterp3d.h) ----------------------------------------------------------
// Every refusal is decided before any device work, and the builder's checks on host axes run on the host, so both behave
// the same on a machine without a device.
// The refusals of a 3-D create that need no device, for the strategy `name` with `need` knots per axis; `bc`: the six ends
// of a Tricubic create (NULL: none to check).
static ndi_status interp3d_create_refusals(const char* name, unsigned long long need, const ndi_interp3d_desc* desc,
                                           const ndi_boundary* bc, ndi_interp3d** out) {
  if (out) *out = nullptr;
  if (!desc || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  if (desc->dtype != NDI_F32 && desc->dtype != NDI_F64)
    return ndi::fail(NDI_BAD_ARG, "%s takes f32 / f64 data (dtype %d): integer and f16 / bf16 element types are not "
                     "provided in three dimensions", name, (int)desc->dtype);
  if (desc->reserved != 0)
    return ndi::fail(NDI_BAD_ARG, "ndi_interp3d_desc.reserved must be 0 (got %d): built against another header version?",
                     (int)desc->reserved);
  static const char* const END[6] = {"x-left", "x-right", "y-left", "y-right", "z-left", "z-right"};
  for (int k = 0; bc && k < 6; ++k)
    if (bc[k].kind < NDI_BC_NOT_A_KNOT || bc[k].kind > NDI_BC_SECOND_DERIV)
      return ndi::fail(NDI_BAD_ARG, "%s takes one non-periodic boundary kind with a scalar value per end (ndi_bc_kind); "
                       "periodic and per-lane boundaries are not provided (%s end: kind %d)", name, END[k], (int)bc[k].kind);
  if (desc->validate && desc->memspace == NDI_MEM_HOST) {
    const ndi_status st =
        desc->dtype == NDI_F32
            ? ndi::check_axes_3d<float>((const float*)desc->x, desc->x_len, (const float*)desc->y, desc->y_len,
                                        (const float*)desc->z, desc->z_len, desc->nx, desc->ny, desc->nz, need)
            : ndi::check_axes_3d<double>((const double*)desc->x, desc->x_len, (const double*)desc->y, desc->y_len,
                                         (const double*)desc->z, desc->z_len, desc->nx, desc->ny, desc->nz, need);
    if (st != NDI_OK) return st;
  }
  return need_device(desc->device);
}

NDI_API ndi_status ndi_interp3d_create(const ndi_interp3d_desc* desc, ndi_interp3d** out) {
  if (const ndi_status rs = interp3d_create_refusals("Trilinear", 2, desc, nullptr, out); rs != NDI_OK) return rs;
  NDI_TRY
  ndi::Interp3DBase* impl = nullptr;
  const ndi_status st = desc->dtype == NDI_F32 ? ndi::create3d<float>(*desc, &impl) : ndi::create3d<double>(*desc, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp3d{impl};
  return NDI_OK;
  NDI_CATCH
}

NDI_API ndi_status ndi_interp3d_eval(const ndi_interp3d* h, const void* qx, const void* qy, const void* qz, uint64_t nq,
                                     void* out, uint64_t out_row_stride, const ndi_eval_opts* opts, ndi_oob_info* info) {
  ndi_eval_opts o;
  if (const ndi_status os = ndi::trilinear_take_opts(opts, o); os != NDI_OK) return os;
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return ndi::bounds_verdict(h->impl->eval(qx, qy, qz, nq, out, out_row_stride, o, info), h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp3d_clone(const ndi_interp3d* h, int32_t device, ndi_interp3d** out) {
  if (out) *out = nullptr;
  if (!h || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  ndi_status ds = need_device(device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::Range rg("ndi_interp3d_clone");
  ndi::Interp3DBase* impl = nullptr;
  ndi_status st = h->impl->clone_to(device, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp3d{impl};
  return NDI_OK;
  NDI_CATCH
}

NDI_API void ndi_interp3d_destroy(ndi_interp3d* h) {
  if (!h) return;
  try {
    ndi::DeviceGuard dg(h->impl->device);
    delete h->impl;
  } catch (...) {
  }
  delete h;
}

// ---- Interp3D, Tricubic (include/ndinterp3d_cubic.h) -------------------------------------------
// ndi_interp3d_create's refusals with 3 knots per axis and the six ends, all before any device work.
NDI_API ndi_status ndi_interp3d_create_tricubic(const ndi_interp3d_desc* desc, const ndi_boundary* bc, ndi_interp3d** out) {
  if (const ndi_status rs = interp3d_create_refusals("Tricubic", 3, desc, bc, out); rs != NDI_OK) return rs;
  NDI_TRY
  ndi_boundary b6[6];
  for (int k = 0; k < 6; ++k) b6[k] = bc ? bc[k] : ndi_boundary{NDI_BC_NOT_A_KNOT, 0.0};
  ndi::Interp3DBase* impl = nullptr;
  const ndi_status st = desc->dtype == NDI_F32 ? ndi::create3d_tricubic<float>(*desc, b6, &impl)
                                               : ndi::create3d_tricubic<double>(*desc, b6, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_interp3d{impl};
  return ndi::bounds_verdict(NDI_OK, impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp3d_tables(const ndi_interp3d* h, void* const tables[7], int32_t memspace) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if (!tables) return ndi::fail(NDI_BAD_ARG, "null tables array");
  if (memspace != NDI_MEM_HOST && memspace != NDI_MEM_DEVICE) return ndi::fail(NDI_BAD_ARG, "unknown memspace");
  NDI_TRY
  const ndi_status st = h->impl->tables(tables, memspace);
  return st == NDI_BAD_ARG ? st : ndi::bounds_verdict(st, h->impl->device);
  NDI_CATCH
}

NDI_API ndi_status ndi_interp1d_trim(const ndi_interp1d* h) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return h->impl->trim();
  NDI_CATCH
}

NDI_API uint64_t ndi_interp1d_scratch_sets(const ndi_interp1d* h) { return h ? h->impl->scratch_sets() : 0; }

NDI_API ndi_status ndi_interp2d_trim(const ndi_interp2d* h) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return h->impl->trim();
  NDI_CATCH
}

NDI_API ndi_status ndi_interp2d_probe_ceiling(const ndi_interp2d* h, uint64_t nq, void* out, uint64_t out_row_stride,
                                              void* stream, int32_t reps, double* ms) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  NDI_TRY
  return h->impl->probe_ceiling(nq, out, out_row_stride, stream, reps, ms);
  NDI_CATCH
}

NDI_API ndi_status ndi_locator_create(int32_t dtype, int32_t device, const void* knots, uint64_t n,
                                      int32_t memspace, ndi_locator** out) {
  if (!knots || !out) return ndi::fail(NDI_BAD_ARG, "null argument");
  *out = nullptr;
  if (dtype < NDI_F32 || dtype > NDI_BF16) return ndi::fail(NDI_BAD_ARG, "unknown dtype");
  ndi_status ds = need_device(device);
  if (ds != NDI_OK) return ds;
  NDI_TRY
  ndi::LocatorBase* impl = nullptr;
  ndi_status st = dtype == NDI_F32   ? ndi::create_locator<float>(device, knots, n, memspace, &impl)
                  : dtype == NDI_F64 ? ndi::create_locator<double>(device, knots, n, memspace, &impl)
                  : dtype == NDI_I32 ? ndi::create_int_locator<int32_t>(device, knots, n, memspace, &impl)
                  : dtype == NDI_I64 ? ndi::create_int_locator<int64_t>(device, knots, n, memspace, &impl)
                  : dtype == NDI_F16 ? ndi::create_half_locator<ndi::HF_F16>(device, knots, n, memspace, &impl)
                                     : ndi::create_half_locator<ndi::HF_BF16>(device, knots, n, memspace, &impl);
  if (st != NDI_OK) return st;
  *out = new ndi_locator{impl};
  return NDI_OK;
  NDI_CATCH
}

NDI_API ndi_status ndi_locator_eval(const ndi_locator* h, const void* q, uint64_t nq, int64_t* out_idx,
                                    int32_t memspace, void* stream) {
  if (!h) return ndi::fail(NDI_BAD_ARG, "null handle");
  if ((!q || !out_idx) && nq) return ndi::fail(NDI_BAD_ARG, "null argument");
  NDI_TRY
  return h->impl->eval(q, nq, out_idx, memspace, stream);
  NDI_CATCH
}

NDI_API void ndi_locator_destroy(ndi_locator* h) {
  if (!h) return;
  try {
    ndi::DeviceGuard dg(h->impl->device);
    delete h->impl;
  } catch (...) {
  }
  delete h;
}

// One-shot form: builds a locator, searches, drops it (allocation + knot upload per call).
NDI_API ndi_status ndi_get_lower_index_batch(int32_t dtype, int32_t device, const void* knots, uint64_t n,
                                             const void* q, uint64_t nq, int64_t* out_idx, int32_t memspace) {
  if (!knots || (!q && nq) || (!out_idx && nq)) return ndi::fail(NDI_BAD_ARG, "null argument");
  ndi_locator* loc = nullptr;
  ndi_status st = ndi_locator_create(dtype, device, knots, n, memspace, &loc);
  if (st != NDI_OK) return st;
  loc->impl->one_shot = true;   // pinning a buffer costs more than the two small copies it would save
  st = ndi_locator_eval(loc, q, nq, out_idx, memspace, nullptr);
  ndi_locator_destroy(loc);
  return st;
}

NDI_API int32_t ndi_monotonic_prop(int32_t dtype, const void* host_v, uint64_t n) {
  if (dtype == NDI_F32) return ndi::monotonic_scan<float>((const float*)host_v, n);
  if (dtype == NDI_I32) return ndi::monotonic_scan<int32_t>((const int32_t*)host_v, n);
  if (dtype == NDI_I64) return ndi::monotonic_scan<int64_t>((const int64_t*)host_v, n);
  if (dtype == NDI_F16) return ndi::monotonic_scan<float>(ndi::half_images<ndi::HF_F16>(host_v, n).data(), n);
  if (dtype == NDI_BF16) return ndi::monotonic_scan<float>(ndi::half_images<ndi::HF_BF16>(host_v, n).data(), n);
  return ndi::monotonic_scan<double>((const double*)host_v, n);
}

NDI_API ndi_status ndi_validate1d(int32_t dtype, const void* host_x, uint64_t x_len, uint64_t n, int32_t strategy) {
  if (dtype == NDI_F32) return ndi::check_axis_1d<float>((const float*)host_x, x_len, n, strategy);
  if (dtype == NDI_F64) return ndi::check_axis_1d<double>((const double*)host_x, x_len, n, strategy);
  if (dtype == NDI_I32) return ndi::check_axis_1d<int32_t>((const int32_t*)host_x, x_len, n, strategy);
  if (dtype == NDI_I64) return ndi::check_axis_1d<int64_t>((const int64_t*)host_x, x_len, n, strategy);
  if (dtype == NDI_F16 || dtype == NDI_BF16) {   // monotonicity on T = on its exact, order-preserving f32 images
    const std::vector<float> x = dtype == NDI_F16 ? ndi::half_images<ndi::HF_F16>(host_x, x_len)
                                                  : ndi::half_images<ndi::HF_BF16>(host_x, x_len);
    return ndi::check_axis_1d<float>(x.data(), x_len, n, strategy);
  }
  return ndi::fail(NDI_BAD_ARG, "unknown dtype");
}

NDI_API ndi_status ndi_validate2d(int32_t dtype, const void* host_x, uint64_t x_len, const void* host_y,
                                  uint64_t y_len, uint64_t nx, uint64_t ny) {
  if (dtype == NDI_F32)
    return ndi::check_axes_2d<float>((const float*)host_x, x_len, (const float*)host_y, y_len, nx, ny);
  if (dtype == NDI_F64)
    return ndi::check_axes_2d<double>((const double*)host_x, x_len, (const double*)host_y, y_len, nx, ny);
  if (dtype == NDI_I32)
    return ndi::check_axes_2d<int32_t>((const int32_t*)host_x, x_len, (const int32_t*)host_y, y_len, nx, ny);
  if (dtype == NDI_I64)
    return ndi::check_axes_2d<int64_t>((const int64_t*)host_x, x_len, (const int64_t*)host_y, y_len, nx, ny);
  if (dtype == NDI_F16 || dtype == NDI_BF16) {
    const bool f16 = dtype == NDI_F16;
    const std::vector<float> x = f16 ? ndi::half_images<ndi::HF_F16>(host_x, x_len)
                                     : ndi::half_images<ndi::HF_BF16>(host_x, x_len);
    const std::vector<float> y = f16 ? ndi::half_images<ndi::HF_F16>(host_y, y_len)
                                     : ndi::half_images<ndi::HF_BF16>(host_y, y_len);
    return ndi::check_axes_2d<float>(x.data(), x_len, y.data(), y_len, nx, ny);
  }
  return ndi::fail(NDI_BAD_ARG, "unknown dtype");
}

// ---- library-owned output buffers -------------------------------------------------------------------------------
// The rate at which a kernel streams rows into a multi-gigabyte buffer depends on which physical pages back it: the same
// evaluation runs 4.6 .. 6.1 ms per 1e6 queries (C2) into buffers the allocator hands out one after the other, stable per
// buffer whatever the order or the warm-up (profiles/r06_placement_vs_ramp.jsonl), and neither hipMemCreate chunks nor
// chunks spread over the physical range change the odds (profiles/r06_output_alloc_probe*.jsonl).  What user space CAN do
// is look: the zero fill Array::zeros performs anyway is timed, and a buffer that fills slowly is set aside and another
// one is asked for while it is still held (so the allocator cannot hand the same pages back), up to `max_tries`; the
// fastest-filling candidate is kept, the others are freed.  A sequential fill and the scattered row stream of the
// evaluation run at the same rate into a given buffer (profiles/r03_tuning.md, "Output placement").
namespace ndi {
struct OutputRegistry {
  std::mutex mu;
  std::unordered_map<void*, std::pair<int, size_t>> live;   // ptr -> (device, bytes)
  // Freed buffers kept for the next request of the same size on the same device (a caller that evaluates batch after
  // batch through interp_array would otherwise pay the allocator -- seconds for tens of gigabytes -- on every call, where a
  // caching allocator pays it once): at most two, and together at most a third of the device's memory; ndi_output_trim
  // releases them.  Their fill rate is known, so a cached buffer is taken without another search.
  struct Spare { void* p; int dev; size_t bytes; double rate; };
  std::vector<Spare> spare;
  std::unordered_map<void*, double> rate;                    // fill rate of the live buffers (TB/s)
  void rates_set(void* p, double r) {
    std::lock_guard<std::mutex> g(mu);
    rate[p] = r;
  }
};
static OutputRegistry& output_registry() {
  static OutputRegistry r;
  return r;
}
static double timed_zero_fill(void* p, size_t bytes, hipEvent_t a, hipEvent_t b) {
  const uint64_t nvec = bytes / 16;
  const uint64_t nrows = (nvec + 2047) / 2048;
  uint64_t mult = 2654435761ull % (nrows ? nrows : 1);         // a multiplier coprime to nrows: the walk is a permutation of the rows
  if (mult < 2) mult = 1;
  auto gcd = [](uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; };
  while (mult > 1 && gcd(mult, nrows) != 1) --mult;
  const unsigned gr = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nrows, (uint64_t)cu_count() * 32));
  NDI_HIP(hipEventRecord(a, nullptr));
  hipLaunchKernelGGL(zero_fill_kernel, dim3(gr), dim3(BLOCK), 0, (hipStream_t) nullptr, (dbl2*)p, nvec, nrows, mult);
  NDI_HIP(hipGetLastError());
  if (bytes % 16) NDI_HIP(hipMemsetAsync((char*)p + nvec * 16, 0, bytes % 16, nullptr));
  NDI_HIP(hipEventRecord(b, nullptr));
  NDI_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  NDI_HIP(hipEventElapsedTime(&ms, a, b));
  return (double)ms;
}
}  // namespace ndi

NDI_API ndi_status ndi_output_alloc(int32_t device, uint64_t bytes, uint32_t max_tries, uint32_t flags, void** out,
                                    ndi_output_info* info) {
  if (!out) return ndi::fail(NDI_BAD_ARG, "null argument");
  if (flags & ~(uint32_t)NDI_OUTPUT_UNINITIALIZED) return ndi::fail(NDI_BAD_ARG, "unknown ndi_output_flags bit");
  *out = nullptr;
  if (info) *info = ndi_output_info{};
  if (bytes == 0) return ndi::fail(NDI_BAD_ARG, "zero-sized output");
  NDI_TRY
  ndi::DeviceGuard dg(device);
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  static const double accept_tbs = [] { const char* e = std::getenv("NDI_OUTPUT_ACCEPT_TBPS"); return e && *e ? std::atof(e) : 6.6; }();   // (a rate, not an integer Knob; read once)
  static const ndi::Knob tries_knob{"NDI_OUTPUT_TRIES", 0};
  const int tries_env = tries_knob.get();
  uint32_t tries = max_tries;
  if (tries == 0) {       // as many candidates as fit into about half of what is free, 2 .. 8
    size_t fr = 0, tot = 0;
    NDI_HIP(hipMemGetInfo(&fr, &tot));
    tries = (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(2, (uint64_t)(0.55 * (double)fr / (double)bytes)));
  }
  if (tries_env > 0) tries = (uint32_t)tries_env;
  // small buffers: a fill this short says nothing about placement, and placement matters little to them
  if (bytes < ((uint64_t)1 << 30)) tries = 1;
  hipEvent_t ea = nullptr, eb = nullptr;
  NDI_HIP(hipEventCreate(&ea));
  NDI_HIP(hipEventCreate(&eb));
  struct Ev { hipEvent_t a, b; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } evg{ea, eb};
  {   // a kept buffer of this size on this device: zero it again and hand it out
    auto& R = ndi::output_registry();
    void* hit = nullptr;
    double rate = 0.0;
    {
      std::lock_guard<std::mutex> g(R.mu);
      for (size_t i = 0; i < R.spare.size(); ++i)
        if (R.spare[i].dev == device && R.spare[i].bytes == (size_t)bytes) {
          hit = R.spare[i].p;
          rate = R.spare[i].rate;
          R.spare.erase(R.spare.begin() + (long)i);
          break;
        }
    }
    if (hit) {
      // NDI_OUTPUT_UNINITIALIZED: the caller overwrites every row it reads (interp_array: the buffer is dropped on Err), so a
      // kept buffer -- whose placement is known -- goes out as it is; the zero fill of 32.8 GB costs what evaluating into it costs
      const double ms = (flags & NDI_OUTPUT_UNINITIALIZED) ? 0.0 : ndi::timed_zero_fill(hit, bytes, ea, eb);
      {
        std::lock_guard<std::mutex> g(R.mu);
        R.live[hit] = {device, (size_t)bytes};
      }
      R.rates_set(hit, rate);
      if (info) {
        info->tries = 0;                                         // 0: a kept buffer, no candidate was allocated
        info->fill_tbps = ms > 0.0 ? (double)bytes / (ms * 1e-3) / 1e12 : rate;   // (not refilled: the rate it was kept with)
        info->worst_fill_tbps = info->fill_tbps;
        info->alloc_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
      }
      *out = hit;
      return NDI_OK;
    }
  }
  std::vector<std::pair<void*, double>> cand;   // (pointer, TB/s of its zero fill)
  auto free_all_but = [&](void* keep) {
    for (auto& c : cand)
      if (c.first != keep) (void)hipFree(c.first);
  };
  void* best = nullptr;
  double best_rate = 0.0;
  try {
    for (uint32_t t = 0; t < tries; ++t) {
      if (t > 0) {     // a further candidate only while the device has room for it beside what is held
        size_t fr = 0, tot = 0;
        NDI_HIP(hipMemGetInfo(&fr, &tot));
        if (fr < bytes + ((size_t)2 << 30)) break;
      }
      void* p = nullptr;
      const hipError_t me = hipMalloc(&p, bytes);
      if (me != hipSuccess) {
        (void)hipGetLastError();
        if (cand.empty()) throw ndi::HipFailure{me, "hipMalloc(output buffer)", __LINE__};
        break;
      }
      double ms = ndi::timed_zero_fill(p, bytes, ea, eb);
      if (tries > 1 && t == 0) ms = ndi::timed_zero_fill(p, bytes, ea, eb);   // (the first fill of a process also pays clock ramp-up)
      const double rate = (double)bytes / (ms * 1e-3) / 1e12;
      cand.emplace_back(p, rate);
      if (rate > best_rate) { best_rate = rate; best = p; }
      if (rate >= accept_tbs) break;
    }
  } catch (...) {
    free_all_but(nullptr);
    throw;
  }
  free_all_but(best);
  {
    auto& R = ndi::output_registry();
    std::lock_guard<std::mutex> g(R.mu);
    R.live[best] = {device, (size_t)bytes};
    R.rate[best] = best_rate;
  }
  if (info) {
    info->tries = (uint32_t)cand.size();
    info->fill_tbps = best_rate;
    info->alloc_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
    info->worst_fill_tbps = best_rate;
    for (auto& c : cand) info->worst_fill_tbps = std::min(info->worst_fill_tbps, c.second);
  }
  *out = best;
  return NDI_OK;
  NDI_CATCH
}

NDI_API ndi_status ndi_output_free(void* p) {
  if (!p) return NDI_OK;
  NDI_TRY
  int dev = -1;
  size_t bytes = 0;
  double rate = 0.0;
  void* evict = nullptr;
  int evict_dev = -1;
  {
    auto& R = ndi::output_registry();
    std::lock_guard<std::mutex> g(R.mu);
    auto it = R.live.find(p);
    if (it == R.live.end()) return ndi::fail(NDI_BAD_ARG, "pointer was not returned by ndi_output_alloc");
    dev = it->second.first;
    bytes = it->second.second;
    R.live.erase(it);
    auto ir = R.rate.find(p);
    if (ir != R.rate.end()) { rate = ir->second; R.rate.erase(ir); }
  }
  ndi::DeviceGuard dg(dev);
  // keep it for the next request of this size?  (buffers of >= 1 GiB only; two at most, a third of the device's memory)
  static const ndi::Knob keep_knob{"NDI_OUTPUT_KEEP", 2};
  const int keep_env = keep_knob.get();
  bool kept = false;
  if (keep_env > 0 && bytes >= ((size_t)1 << 30)) {
    size_t fr = 0, tot = 0;
    NDI_HIP(hipMemGetInfo(&fr, &tot));
    auto& R = ndi::output_registry();
    std::lock_guard<std::mutex> g(R.mu);
    size_t held = bytes;
    for (auto& sp : R.spare)
      if (sp.dev == dev) held += sp.bytes;
    if (held <= tot / 3) {
      if (R.spare.size() >= (size_t)keep_env) {     // the oldest goes
        evict = R.spare.front().p;
        evict_dev = R.spare.front().dev;
        R.spare.erase(R.spare.begin());
      }
      R.spare.push_back({p, dev, bytes, rate});
      kept = true;
    }
  }
  // hipFree waits for the device; a kept buffer gives the same guarantee -- whoever gets it next (possibly without a refill,
  // NDI_OUTPUT_UNINITIALIZED) must not meet the previous owner's kernels still writing into it from a non-blocking stream
  if (kept) NDI_HIP(hipDeviceSynchronize());
  if (evict) {
    ndi::DeviceGuard de(evict_dev);
    NDI_HIP(hipFree(evict));
  }
  if (!kept) NDI_HIP(hipFree(p));
  return NDI_OK;
  NDI_CATCH
}

NDI_API ndi_status ndi_output_trim(void) {
  NDI_TRY
  std::vector<ndi::OutputRegistry::Spare> gone;
  {
    auto& R = ndi::output_registry();
    std::lock_guard<std::mutex> g(R.mu);
    gone.swap(R.spare);
  }
  for (auto& sp : gone) {
    ndi::DeviceGuard dg(sp.dev);
    NDI_HIP(hipFree(sp.p));
  }
  return NDI_OK;
  NDI_CATCH
}

NDI_API int32_t ndi_device_count(void) {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
  return cnt;
}

NDI_API const char* ndi_last_error_string(void) { return ndi::tls_error().c_str(); }

NDI_API uint32_t ndi_version(void) { return (NDI_VERSION_MAJOR << 16) | NDI_VERSION_MINOR; }

NDI_API void ndi_profile_enable(int32_t on) { ndi::g_prof_on.store(on ? 1 : 0); }

NDI_API ndi_status ndi_profile_read(ndi_profile* out, int32_t reset) {
  if (!out) return ndi::fail(NDI_BAD_ARG, "null argument");
  NDI_TRY
  std::lock_guard<std::mutex> g(ndi::g_prof_mu);
  for (auto& r : ndi::g_prof_recs) {
    NDI_HIP(hipEventSynchronize(r.b));
    float ms = 0.f;
    NDI_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    ndi::ProfScope::account_locked(r, ms);
    ndi::g_prof_pool[r.dev].push_back(r.a);
    ndi::g_prof_pool[r.dev].push_back(r.b);
  }
  ndi::g_prof_recs.clear();
  ndi::g_prof_acc.last_path = ndi::g_last_path.load();
  *out = ndi::g_prof_acc;
  if (reset) ndi::g_prof_acc = ndi_profile{};
  return NDI_OK;
  NDI_CATCH
}
