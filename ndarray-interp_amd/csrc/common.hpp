// csrc/common.hpp -- shared host-side plumbing of libndinterp_hip.so (error text, HIP checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "../../include/ndinterp.h"

namespace ndi {

inline std::string& tls_error() {
  static thread_local std::string s;
  return s;
}

inline ndi_status fail(ndi_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  tls_error() = buf;
  return st;
}

struct HipFailure {
  hipError_t err;
  const char* what;
  int line;
};

#define NDI_HIP(expr)                                                     \
  do {                                                                    \
    hipError_t e__ = (expr);                                              \
    if (e__ != hipSuccess) throw ::ndi::HipFailure{e__, #expr, __LINE__}; \
  } while (0)

inline ndi_status from_hip(const HipFailure& f) {
  return fail(NDI_HIP_ERROR, "HIP error %d (%s) at %s [csrc line %d]", (int)f.err,
              hipGetErrorString(f.err), f.what, f.line);
}

// Run-time value -> compile-time value: pick<8, 4, 2>(u, f) calls f(Int<V>{}) for the listed V that equals u and returns
// whether one did; pick_or<1, 8, 4, 2>(u, f) calls f(Int<1>{}) for every other u; pick_bool(b, f) calls f(std::true_type{})
// or f(std::false_type{}).  f is a generic lambda that names its kernel with the constant
// (`[&](auto u_) { constexpr int U = u_; ... kernel<T, U> ... }`: the parameter is taken by value, so it converts inside a
// constant expression; an inner lambda uses the constexpr copy, not the captured parameter).  Nest the calls for several
// dimensions, and keep combinations that must not be instantiated out with `if constexpr` or separate lists: every kernel
// named in a lambda body that is not discarded is emitted, reached or not.
template <int V>
using Int = std::integral_constant<int, V>;
template <int... Vs, class F>
inline bool pick(int v, F&& f) {
  return ((v == Vs && (f(Int<Vs>{}), true)) || ...);
}
template <int Default, int... Vs, class F>
inline void pick_or(int v, F&& f) {
  if (!pick<Vs...>(v, f)) f(Int<Default>{});
}
template <class F>
inline void pick_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}

// NDI_TRACE_PLAN: every plan prints its `[ndi plan]` line to stderr.  A getenv per call: the tests switch the variable inside
// a running process.
inline bool trace_plan() { return std::getenv("NDI_TRACE_PLAN") != nullptr; }

// An integer tuning variable of the environment (the table of all of them: DESIGN.md 8a).  Unset or empty: the default.
// `once` is read when the Knob is constructed (a function-local static: the first call) and never again; `live` is too,
// unless NDI_TUNE_LIVE was set at that moment -- then every get() re-reads it, so one process can sweep the variants.
// Without NDI_TUNE_LIVE get() is a load: no getenv on the per-call path.
inline int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e && *e ? std::atoi(e) : dflt;
}
struct Knob {
  enum Kind { once, live };
  Knob(const char* name_, int dflt_, Kind kind = once)
      : name(name_), dflt(dflt_), first(env_int(name_, dflt_)), reread(kind == live && std::getenv("NDI_TUNE_LIVE") != nullptr) {}
  int get() const { return reread ? env_int(name, dflt) : first; }

 private:
  const char* name;
  int dflt, first;
  bool reread;
};

template <class T>
struct DType;
template <>
struct DType<float> {
  static constexpr int id = NDI_F32;
};
template <>
struct DType<double> {
  static constexpr int id = NDI_F64;
};
template <>
struct DType<int32_t> {
  static constexpr int id = NDI_I32;
};
template <>
struct DType<int64_t> {
  static constexpr int id = NDI_I64;
};

}  // namespace ndi
