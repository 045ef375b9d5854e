/* include/ndinterp.h -- C ABI of libndinterp_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the batched `interp_array` hot path of the Rust crate
 * ndarray-interp v0.6.0 (1D Linear, 1D CubicSpline, 2D Bilinear), plus a 2D Bicubic strategy
 * (ndi_interp2d_create_bicubic; with Pchip, Akima or caller-given node derivatives: ndi_interp2d_create_bicubic_local,
 * ndi_interp2d_create_bicubic_hermite) and three 1D strategies the
 * reference leaves to user code: Pchip, Akima and CubicHermite (ndi_strategy1d), and first / second
 * derivatives of the four cubics as handles of their own (ndi_interp1d_derivative), and antiderivatives / definite
 * integrals of every f32 / f64 1D interpolant (ndi_interp1d_antiderivative, ndi_interp1d_integrate).  The reference
 * has no FFI of its own: its boundary is the strategy trait pair plus the inherent
 * methods of Interp1D / Interp2D.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference tree).  A Rust
 * `extern "C"` block binding exactly these symbols, and the strategy overrides that
 * call them, are shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; no exceptions, no panics cross the ABI; every call
 *    returns an ndi_status (ndi_last_error_string() has the text for the calling
 *    thread).
 *  - element type T is selected per handle by ndi_dtype: f32 / f64 (every strategy), and -- added in v0.5,
 *    backward-compatible: new enumerators only -- i32 / i64 for Linear and Bilinear.  Integer T follows the
 *    reference's `T` arithmetic exactly: division truncates toward zero and an intermediate that does not fit T is
 *    reported as NDI_INT_OVERFLOW (a Rust debug build panics there).  Integer handles keep slope records {y, m}
 *    instead of the data on the device, about twice the data's memory.  Other integer widths (unsigned, 8/16-bit)
 *    stay on the host's generic per-query path, see INTEGRATION.md.
 *    Also v0.5, backward-compatible: f16 / bf16 (IEEE binary16 and bfloat16, passed as their 16-bit patterns) for
 *    Linear and Bilinear.  They follow the `half` crate's arithmetic: every operation converts its operands to f32
 *    exactly, does one IEEE f32 operation and rounds to T with ties to even (overflow gives inf), so results are
 *    bit-exact.  Only the float errors exist (NDI_OUT_OF_BOUNDS, NDI_NAN_QUERY).  Half handles keep the data as
 *    given plus f32 images of the knots; async_launch and the sharded calls behave as for f32 / f64.
 *  - arrays are C-order and contiguous: data[n][lanes], data2d[nx][ny][lanes];
 *    "lanes" = product of the trailing (non-interpolated) axes.
 *  - every pointer argument carries a memory space (host or device).  Device
 *    pointers must belong to the handle's device.
 *  - the product has NO CPU fallback: without a usable HIP device every compute
 *    entry point fails with NDI_HIP_ERROR.
 */
#ifndef NDINTERP_H
#define NDINTERP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NDI_VERSION_MAJOR 0
#define NDI_VERSION_MINOR 5

/* BuilderError / InterpolateError (src/lib.rs:127-146) + ABI-only codes. */
typedef enum ndi_status {
  NDI_OK = 0,
  NDI_NOT_ENOUGH_DATA = 1, /* BuilderError::NotEnoughData                                  */
  NDI_MONOTONIC = 2,       /* BuilderError::Monotonic                                      */
  NDI_SHAPE = 3,           /* BuilderError::ShapeError                                     */
  NDI_VALUE = 4,           /* BuilderError::ValueError (periodic y[0] != y[n-1])           */
  NDI_OUT_OF_BOUNDS = 5,   /* InterpolateError::OutOfBounds                                */
  NDI_NAN_QUERY = 6,       /* reference panics: vector_extensions.rs:83-84                 */
  NDI_HIP_ERROR = 7,       /* no device / HIP runtime failure                              */
  NDI_BAD_ARG = 8,
  NDI_UNSUPPORTED = 9,
  NDI_INT_OVERFLOW = 10    /* integer T: "attempt to {subtract,multiply,add,divide} with overflow" (a Rust debug
                              build's panic inside Linear::calc_frac, linear.rs:29-36); added in v0.5 */
} ndi_status;

/* NDI_I32 / NDI_I64 (v0.5, backward-compatible): NDI_LINEAR and Bilinear only; NDI_CUBIC_SPLINE is refused with
 * NDI_BAD_ARG (the reference's trait bounds forbid it), ndi_interp1d_coefficients on such a handle is NDI_BAD_ARG and
 * NDI_PATH_BUCKETED is NDI_UNSUPPORTED (AUTO and GATHER evaluate).  NDI_F16 / NDI_BF16 (v0.5, backward-compatible):
 * the same restrictions. */
typedef enum ndi_dtype { NDI_F32 = 0, NDI_F64 = 1, NDI_I32 = 2, NDI_I64 = 3, NDI_F16 = 4, NDI_BF16 = 5 } ndi_dtype;

/* The operation of Linear::calc_frac (linear.rs:29-36) that overflowed: ndi_oob_info.axis for NDI_INT_OVERFLOW. */
typedef enum ndi_int_op {
  NDI_OP_SUBTRACT = 0,
  NDI_OP_MULTIPLY = 1,
  NDI_OP_ADD = 2,
  NDI_OP_DIVIDE = 3
} ndi_int_op;
typedef enum ndi_memspace { NDI_MEM_HOST = 0, NDI_MEM_DEVICE = 1 } ndi_memspace;

/* 1D strategies: Linear (src/interp1d/strategies/linear.rs),
 * CubicSpline (src/interp1d/strategies/cubic_spline.rs).
 *
 * NDI_PCHIP, NDI_AKIMA, NDI_CUBIC_HERMITE (backward-compatible: new enumerators only; f32 / f64) are local C1 cubics.  The
 * reference leaves them to user strategies; here they are built on the device.  CubicSplineStrategy::interp_into
 * (cubic_spline.rs:811-828) evaluates the cubic Hermite form for any knot derivatives k once the tables
 *   a_i = k_i h_i - dy,  b_i = dy - k_{i+1} h_i        (dy = y[i+1] - y[i], h_i = x[i+1] - x[i]; cubic_spline.rs:362-363)
 * exist, so these strategies only choose k differently; their handles take every evaluation entry point, path and AUTO
 * rule of a CubicSpline handle of the same shape.  `extrapolate` != 0 continues the first / last interval's polynomial.
 * Numerical contract -- this project's own, there is no Rust to follow: per lane, every line one IEEE operation in T in
 * this order, nothing fused; delta_i = dy / h_i; sgn(v) = (v > 0) - (v < 0) is -1, 0 or 1, so sgn(NaN) = 0; +0 is
 * positive zero.  Non-finite data is not refused: it goes through these lines as IEEE values, and a comparison with a NaN
 * is false.  For Pchip's ends that means: a NaN slope (m0, m1 or d NaN) makes that end's k NaN, unless sgn(d) != sgn(m0)
 * has already decided for +0 (d NaN beside a non-zero m0).  tests/test_hostile_inputs.py has the table.
 *  NDI_PCHIP (>= 2 knots; what scipy's PchipInterpolator computes).  n == 2: k_0 = k_1 = delta_0.  Interior knots:
 *      if delta_{i-1} == 0 or delta_i == 0 or (delta_{i-1} > 0) != (delta_i > 0):  k_i = +0
 *      else  w1 = (h_i + h_i) + h_{i-1};  w2 = h_i + (h_{i-1} + h_{i-1});  k_i = (w1 + w2) / (w1 / delta_{i-1} + w2 / delta_i)
 *    ends: k_0 = edge(h_0, h_1, delta_0, delta_1),  k_{n-1} = edge(h_{n-2}, h_{n-3}, delta_{n-2}, delta_{n-3}) with
 *      edge(h0, h1, m0, m1):  d = (((h0 + h0) + h1) m0 - h0 m1) / (h0 + h1)
 *                             sgn(d) != sgn(m0): +0;  else sgn(m0) != sgn(m1) and |d| > 3 |m0|: 3 m0;  else d
 *  NDI_AKIMA (>= 3 knots; Akima 1970, scipy's Akima1DInterpolator with method="akima").  m_j = delta_j (0 <= j <= n-2),
 *    m_{-1} = (m_0 + m_0) - m_1,  m_{-2} = (m_{-1} + m_{-1}) - m_0,  m_{n-1} = (m_{n-2} + m_{n-2}) - m_{n-3},
 *    m_n = (m_{n-1} + m_{n-1}) - m_{n-2};  for every knot:
 *      w1 = |m_{i+1} - m_i|;  w2 = |m_{i-1} - m_{i-2}|;  s = w1 + w2
 *      k_i = s == 0 ? 0.5 (m_{i-1} + m_i) : (w1 m_{i-1} + w2 m_i) / s
 *    Deviation from scipy: scipy takes the average below a threshold relative to the largest s of the whole array (a global
 *    reduction for a rounding-level effect); here the test is the exact s == 0.
 *  NDI_CUBIC_HERMITE (>= 2 knots): k is given by the caller, see ndi_interp1d_create_hermite.
 * For these three a non-zero `periodic`, `build_flags`, boundary field or lane_* pointer of the descriptor is NDI_BAD_ARG
 * (they are spline notions), and so is an integer or half-precision dtype. */
typedef enum ndi_strategy1d {
  NDI_LINEAR = 0,
  NDI_CUBIC_SPLINE = 1,
  NDI_PCHIP = 2,
  NDI_AKIMA = 3,
  NDI_CUBIC_HERMITE = 4
} ndi_strategy1d;

/* SingleBoundary (cubic_spline.rs:204-217).  Natural == SecondDeriv(0),
 * Clamped == FirstDeriv(0) (:287-296). */
typedef enum ndi_bc_kind {
  NDI_BC_NOT_A_KNOT = 0,
  NDI_BC_NATURAL = 1,
  NDI_BC_CLAMPED = 2,
  NDI_BC_FIRST_DERIV = 3,
  NDI_BC_SECOND_DERIV = 4
} ndi_bc_kind;

typedef struct ndi_boundary {
  int32_t kind; /* ndi_bc_kind */
  double value; /* derivative value for FIRST_DERIV / SECOND_DERIV */
} ndi_boundary;

/* Monotonic (src/vector_extensions.rs:25-29). */
typedef enum ndi_monotonic {
  NDI_MONO_NOT = 0,
  NDI_MONO_RISING_STRICT = 1,
  NDI_MONO_RISING = 2,
  NDI_MONO_FALLING_STRICT = 3,
  NDI_MONO_FALLING = 4
} ndi_monotonic;

/* Evaluation formulation (results are identical):
 *  GATHER   one coalesced row gather per query (4 operand rows in, 1 row out);
 *  BUCKETED queries are grouped by interval on the device so each table row is
 *           read once per group and the kernel becomes a pure output stream;
 *  AUTO     BUCKETED when the batch has enough queries per interval (>= 5) to pay for
 *           the grouping pass, else GATHER. */
typedef enum ndi_path { NDI_PATH_AUTO = 0, NDI_PATH_GATHER = 1, NDI_PATH_BUCKETED = 2 } ndi_path;

/* CubicSpline::build (cubic_spline.rs:310-368, 409-721) -- numerical contract of the coefficient tables.
 * The serial per-lane kernels evaluate thomas (:678-721) in the reference's operation order without contraction: the
 * a / b tables are BIT-IDENTICAL to the reference's.  For narrow trailing axes on many knots (n >= 2048 and
 * lanes <= 256: scalar data on 1e5-1e6 knots, 8 lanes on 4096) that would be one or two wavefronts doing 2n dependent
 * steps, so by default such builds -- on axes whose neighbouring knot spacings differ by less than 1e3 (f32) / 1e9
 * (f64); wilder axes keep the serial kernels -- take blocked sweeps: both first-order recurrences are cut into blocks and
 * re-associated (back substitution as r'/mid' + (-up/mid') k).  Every coefficient then agrees with the reference's to
 * within 1e-12 (f64) / 1e-5 (f32) of the larger of: the magnitudes of the table entries within 32 rows of it, and the
 * interval's |dy| -- errors do not travel (the recurrences' multipliers are <= 1/2 in magnitude) -- and evaluated
 * rows meet the crate's own assertion form at 1e-10 / 1e-5 (tests/test_gpu_spline_blocked.py, incl. geometric and
 * clustered knots).  NDI_BUILD_REFERENCE_ORDER keeps the serial kernels for the handle: bit-identical tables at the
 * serial kernels' speed. */
typedef enum ndi_build_flags {
  NDI_BUILD_DEFAULT = 0,
  NDI_BUILD_REFERENCE_ORDER = 1 /* never re-associate the Thomas sweeps: tables bit-identical to the reference's */
} ndi_build_flags;

/* Replaces Interp1DBuilder::{new,x,strategy,build} (src/interp1d/mod.rs:399-476)
 * + Interp1DStrategyBuilder::build (src/interp1d/strategies/mod.rs:12-40):
 * Linear::build (linear.rs:54-63) / CubicSpline::build (cubic_spline.rs:754-771). */
typedef struct ndi_interp1d_desc {
  int32_t dtype;       /* ndi_dtype */
  int32_t strategy;    /* ndi_strategy1d */
  int32_t extrapolate; /* Linear::extrapolate / CubicSpline::extrapolate (bool) */
  int32_t device;      /* HIP device ordinal */
  uint64_t n;          /* data.shape()[0] */
  uint64_t lanes;      /* product of data.shape()[1..] (1 for 1-D data) */
  uint64_t x_len;      /* x.len(); checked against n exactly as build() does (:465-471) */
  const void* x;       /* T[x_len] knots, or NULL for the default axis 0..n (:402-406) */
  const void* data;    /* T[n * lanes] */
  int32_t memspace;    /* ndi_memspace of x and data */
  int32_t validate;    /* != 0: run Interp1DBuilder::build's checks (:449-471) here */
  /* CubicSpline boundary (BoundaryCondition, cubic_spline.rs:153-168) */
  int32_t periodic;    /* BoundaryCondition::Periodic */
  int32_t build_flags; /* ndi_build_flags (0 = default); occupies what was alignment padding in v0.3: same layout */
  ndi_boundary left;   /* applied to every lane unless lane_* are given */
  ndi_boundary right;
  /* BoundaryCondition::Individual (per trailing element, cubic_spline.rs:332-347):
   * arrays of `lanes` entries, host memory; all four NULL for a global boundary. */
  const int32_t* lane_left_kind;
  const double* lane_left_value;
  const int32_t* lane_right_kind;
  const double* lane_right_value;
} ndi_interp1d_desc;

/* Replaces Interp2DBuilder::{new,x,y,strategy,build} (src/interp2d/mod.rs:382-519)
 * + Bilinear::build (src/interp2d/strategies/bilinear.rs:45-52).
 * Device memory: one copy of the grid; for short trailing axes (lanes * sizeof(T) <= 64 bytes) the copy
 * is kept pair-packed instead ({z[xi][yi], z[xi][yi+1]} per cell), which takes twice the grid size. */
typedef struct ndi_interp2d_desc {
  int32_t dtype;
  int32_t extrapolate; /* Bilinear::extrapolate */
  int32_t device;
  int32_t memspace;    /* of x, y, data */
  uint64_t nx, ny;     /* data.shape()[0], data.shape()[1] */
  uint64_t lanes;      /* product of data.shape()[2..] */
  uint64_t x_len, y_len;
  const void* x;       /* T[x_len] or NULL for 0..nx (:389-393) */
  const void* y;       /* T[y_len] or NULL for 0..ny (:394-398) */
  const void* data;    /* T[nx * ny * lanes] */
  int32_t validate;    /* != 0: run Interp2DBuilder::build's checks (:477-509) here */
  int32_t reserved;
} ndi_interp2d_desc;

/* Bicubic (ndi_interp2d_create_bicubic; f32 / f64): the tensor-product cubic spline on the grid, what scipy computes with
 * RectBivariateSpline(x, y, z, kx=3, ky=3, s=0) for the default ends on any strictly rising axes -- C2 across every grid line where Bilinear is C0.  It
 * is a bicubic Hermite patch per cell whose node derivatives zx, zy, zxy come from 1-D spline solves along each axis.
 * The handle is an ndi_interp2d like any other: ndi_interp2d_eval (sync, async_launch + ndi_interp2d_finish), _trim,
 * _clone (the node table is copied device to device, no rebuild), _eval_ring, _eval_sharded / _eval_ring_sharded (the
 * replica signature includes the strategy: a set that mixes Bilinear and Bicubic handles is refused), _destroy.
 * Numerical contract -- this project's own.  T in {f32, f64}, data z[nx][ny][C], axes x[nx], y[ny], one ndi_boundary of any
 * ndi_bc_kind per end (x-left, x-right, y-left, y-right; default NotAKnot on all four).  Every line is one IEEE operation in
 * T, in this order, nothing fused.
 *  Node derivatives, three tables of z's shape:
 *     x-pass  the CubicSpline coefficient build with knots x on z viewed as (nx, ny C), in the REFERENCE operation order (what
 *             NDI_BUILD_REFERENCE_ORDER means; n == 3 with both ends NotAKnot takes the build's parabola branch), giving
 *             a, b.  ONE entry differs from CubicSpline::build: for a NotAKnot right end the last row of the system has
 *             x[n-2] - x[n-3] on the diagonal, which is what the not-a-knot condition gives, where the reference has
 *             x[n-1] - x[n-2] (cubic_spline.rs:635).  So a pass is bit-identical to CubicSpline::build on those columns
 *             whenever the right end is not NotAKnot or the last two intervals are equal, and differs in that entry alone
 *             otherwise -- which is what makes the default ends scipy's spline on unevenly spaced axes as well
 *             (ndi_interp1d handles keep the reference's row).  Then ndi_interp1d_derivative's rule per column, with
 *             dz = z[i+1] - z[i], dx = x[i+1] - x[i]:
 *                 zx[i]    = (dz + a[i]) / dx        i < nx-1
 *                 zx[nx-1] = (dz - b[nx-2]) / dx     with i = nx-2
 *     y-pass  the same with knots y on each z[i] viewed as (ny, C), giving zy
 *     cross   the y-pass applied to zx with the y ends' kinds and end value 0 (the x-derivative of a constant end value),
 *             giving zxy
 *  Evaluation: i, j from get_lower_index on each axis; hx = x[i+1] - x[i], t = (qx - x[i]) / hx, likewise hy, u; with
 *     H(pl, pr, kl, kr, h, s):  d = pr - pl;  a = kl h - d;  b = d - kr h;
 *                               (1-s) pl + s pr + s (1-s) (a (1-s) + b s)        (the order of cubic_spline.rs:824-828)
 *  per lane:
 *     p0 = H(z[i][j],    z[i][j+1],    zy[i][j],    zy[i][j+1],    hy, u)
 *     p1 = H(z[i+1][j],  z[i+1][j+1],  zy[i+1][j],  zy[i+1][j+1],  hy, u)
 *     d0 = H(zx[i][j],   zx[i][j+1],   zxy[i][j],   zxy[i][j+1],   hy, u)
 *     d1 = H(zx[i+1][j], zx[i+1][j+1], zxy[i+1][j], zxy[i+1][j+1], hy, u)
 *     result = H(p0, p1, d0, d1, hx, t)
 *  Range, errors, extrapolation are Bilinear's: inclusive range test, x before y for the same query, the lowest failing flat
 *  index, NDI_NAN_QUERY by the same rule; after an error rows before the failing query are written and later rows untouched;
 *  NDI_EVAL_FRESH_OUTPUT and NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED are honoured.  `extrapolate` != 0 uses the end cell's
 *  patch with t / u outside [0, 1], as the 1-D spline does.
 *  Refused before any device work, each with a message naming Bicubic and the reason: fewer than 3 points on an axis
 *  (NDI_NOT_ENOUGH_DATA); with NDI_BAD_ARG integer and f16 / bf16 element types and any boundary kind outside ndi_bc_kind
 *  (a periodic END has no encoding here -- a periodic AXIS is ndi_interp2d_create_bicubic_periodic, below -- and per-lane
 *  boundaries are not provided).  NDI_PATH_AUTO and NDI_PATH_GATHER
 *  take the one evaluation kernel; NDI_PATH_BUCKETED is NDI_BAD_ARG naming the strategy, and so is
 *  ndi_interp2d_probe_ceiling.
 *  Device memory: the node table {z, zx, zy, zxy} per grid node, T[nx][ny][4][C] = four times the grid, plus the two knot
 *  axes; the plain grid is not kept.  The build's temporaries (about seven grids at the peak) are freed before create returns.
 * Partial derivatives (ndi_interp2d_partial): a handle that evaluates d^(nu_x + nu_y) / dx^nu_x dy^nu_y of the surface,
 * nu_x, nu_y in {0, 1, 2}, not both 0 -- the orders scipy's RectBivariateSpline.ev(x, y, dx, dy) offers.  The node table
 * {z, zx, zy, zxy} determines all of them; the handle SHARES its source's table (no copy: three gradient handles cost three
 * pairs of knot axes, not three tables), and the table is freed with the last handle that holds it, whatever the order of
 * the ndi_interp2d_destroy calls.  Every line is one IEEE operation in T, in this order, nothing fused; d, a, b as in H:
 *     c1 = d + a          c2 = b - (a + a)          c3 = b - a
 *     H0(pl, pr, kl, kr, h, s) = H(pl, pr, kl, kr, h, s)
 *     H1(pl, pr, kl, kr, h, s) = (c1 + s * ((c2 + c2) - (3 * c3) * s)) / h
 *     H2(pl, pr, kl, kr, h, s) = ((c2 + c2) - (6 * c3) * s) / (h * h)
 *  (the form is q(s) = pl + (d + a) s + (b - 2a) s^2 - (b - a) s^3, the expansion of the 1-D antiderivative contract), and
 *  the evaluation is the one above with the forms swapped: p0, p1, d0, d1 = H_{nu_y}(..., hy, u) on the same sixteen
 *  operands, result = H_{nu_x}(p0, p1, d0, d1, hx, t); cell, t, u, hx, hy exactly as above, and with `extrapolate` the end
 *  cell's patch continued with t / u outside [0, 1].  The spline is C2 in each variable, so all eight orders are continuous
 *  across grid lines up to rounding; a query on an interior grid line evaluates the cell to its right / above
 *  (get_lower_index), the 1-D handles' convention.  Range, NaN, first-error and rows-before-the-error semantics, the eval
 *  flags, the ring and sharded calls, _trim, _clone (the table is copied, the orders kept), _tables (the origin's zx, zy,
 *  zxy) and the refusal of NDI_PATH_BUCKETED / _probe_ceiling are the Bicubic handle's, unchanged.  The orders are part of
 *  the replica signature: a sharded set that mixes a surface with its partial, or two different partials, is refused.
 * Integrals (ndi_interp2d_antiderivative, ndi_interp2d_integral): a handle that evaluates
 *     F(qx, qy) = the integral of the surface over [x[0], qx] x [y[0], qy]
 * and rectangle integrals through it -- scipy's RectBivariateSpline.integral(xa, xb, ya, yb).  The antiderivative of a
 * tensor-product Hermite cubic is the tensor product of ndi_interp1d_antiderivative's rule with itself.  Every line is one
 * IEEE operation in T, in this order, nothing fused.  G is that rule's cubic-class G in Hermite form; d, a, b are H's lines:
 *     G(pl, pr, kl, kr, h, s):  d = pr - pl;  a = kl h - d;  b = d - kr h;
 *                               c1 = (d + a) * 0.5;  c2 = (b - (a + a)) / 3;  c3 = (b - a) * 0.25
 *                               s * (pl + s * (c1 + s * (c2 - s * c3)))
 *     the integral over the whole interval:  I = h * (pl + (c1 + (c2 - c3)))
 *  prefix_axis(knots, p, k): ndi_interp1d_antiderivative's FIXED blocked sum with B = 256 along one axis over the I of the
 *  Hermite data (values p, slopes k) -- the same S / T / O / P recurrences, bits that do not depend on launch geometry.
 *  Five prefix tables of the grid's shape, from the node table {z, zx, zy, zxy}:
 *     Qz  = prefix along x of (values z,  slopes zx)        Pz  = prefix along y of (values z,  slopes zy)
 *     Qzy = prefix along x of (values zy, slopes zxy)       Pzx = prefix along y of (values zx, slopes zxy)
 *     PP  = prefix along x of (values Pz, slopes Pzx)
 *  (PP along y of (Qz, Qzy) is the same number and other bits: the contract is x of (Pz, Pzx).)
 *  Evaluation: cell i, j and t, u, hx, hy exactly Bicubic's; per lane
 *     w0 = Pz [i]  [j] + hy * G(z [i]  [j], z [i]  [j+1], zy [i]  [j], zy [i]  [j+1], hy, u)
 *     w1 = Pz [i+1][j] + hy * G(z [i+1][j], z [i+1][j+1], zy [i+1][j], zy [i+1][j+1], hy, u)
 *     v0 = Pzx[i]  [j] + hy * G(zx[i]  [j], zx[i]  [j+1], zxy[i]  [j], zxy[i]  [j+1], hy, u)
 *     v1 = Pzx[i+1][j] + hy * G(zx[i+1][j], zx[i+1][j+1], zxy[i+1][j], zxy[i+1][j+1], hy, u)
 *     e  = PP [i]  [j] + hy * G(Qz[i][j], Qz[i][j+1], Qzy[i][j], Qzy[i][j+1], hy, u)
 *     F  = e + hx * G(w0, w1, v0, v1, hx, t)
 *  25 operands per output element.  `extrapolate` continues the end cell's form with t / u outside [0, 1]; a query on an
 *  interior grid line takes the cell to its right / above.  The rectangle integral is, in ONE evaluation launch,
 *     out = (F(xb, yb) - F(xa, yb)) - (F(xb, ya) - F(xa, ya))
 *  in this association: xa == xb or ya == yb gives exactly 0; xa > xb or ya > yb negates, as scipy does.
 *  The integral handle SHARES its source's node table (no copy; freed with the last handle that holds it, in any order of
 *  the destroy calls) and owns the five prefix tables (five times the grid) and its two knot axes.  Through
 *  ndi_interp2d_eval it is a Bicubic handle: range, NaN, first-error and rows-before-the-error semantics, the eval flags,
 *  async_launch / _finish, the ring and sharded calls, _trim, _clone (the tables are copied, the flag kept), _tables (the
 *  origin's zx, zy, zxy) and the refusal of NDI_PATH_BUCKETED / _probe_ceiling are unchanged.  The integral bit is part
 *  of the replica signature: a sharded set that mixes a surface with its integral is refused.
 * Value and derivatives in one call (ndi_interp2d_eval_jet): the surface and its partials up to `order` (1: value and
 * gradient, 2: with the three second derivatives) at the same queries, from ONE read of the sixteen operands -- per point
 * 16 + K element reads and writes where K separate handle calls move 17 K.  There are no new formulas: part k is, bit for
 * bit, what ndi_interp2d_eval of ndi_interp2d_partial(h, nu_x, nu_y) writes for the same queries (part 0: what
 * ndi_interp2d_eval(h) writes), in the fixed order of (nu_x, nu_y)
 *     order 1:  (0,0) (1,0) (0,1)                    order 2:  (0,0) (1,0) (0,1) (2,0) (1,1) (0,2)
 *  with Pm = the four y-forms H_m(..., hy, u) of the sixteen operands:  (0,0) = H0(P0, hx, t)   (1,0) = H1(P0, hx, t)
 *  (0,1) = H0(P1, hx, t)   (2,0) = H2(P0, hx, t)   (1,1) = H1(P1, hx, t)   (0,2) = H0(P2, hx, t).  Cell, t, u, hx, hy, the
 *  range test, the NaN rule and `extrapolate` are the Bicubic handle's.
 * Local rules and caller-given node derivatives (ndi_interp2d_create_bicubic_local, ndi_interp2d_create_bicubic_hermite):
 * the same Bicubic handle with the node derivatives chosen differently, as NDI_PCHIP / NDI_AKIMA / NDI_CUBIC_HERMITE choose
 * k differently in 1-D.  Numerical contract -- this project's own.  Let k = RULE(knots, columns) be the knot-derivative
 * rule exactly as ndi_strategy1d states it for NDI_PCHIP / NDI_AKIMA: every line one IEEE operation in T, in that order,
 * nothing fused, n == 2, the sgn rule, the +0 rule and the exact s == 0 included.  One rule serves both axes of a handle:
 *     zx  = RULE(x, .) on z viewed as (nx, ny C)
 *     zy  = RULE(y, .) on each z[i] viewed as (ny, C)
 *     zxy = RULE(y, .) on each zx[i] viewed as (ny, C)        (the "cross" composition of the spline Bicubic)
 *  For the hermite call zx, zy, zxy are the caller's arrays and no rule is applied; ndi_interp2d_tables hands them back bit
 *  for bit.  Evaluation, partials, jet, F and rectangle integrals are the formulas above on that table, character for
 *  character: there are no new evaluation formulas and no new evaluation kernels.
 *  Grid-line property: on a grid line x = x[i] the surface is, bit for bit for finite tables, the 1-D strategy's interpolant
 *  of the column z[i][:] (t == 0; t == 1 on the last line), and likewise along y.  Pchip therefore does not overshoot
 *  ALONG GRID LINES.  Monotonicity INSIDE a cell is NOT promised: the tensor composition of a monotone rule is not monotone
 *  in 2-D, and a cell's interior may leave the range of its four corners.
 *  Smoothness and partials: these surfaces are C1, not C2.  Partial handles of order 2 in a variable are piecewise and JUMP at
 *  the grid lines of that variable; a query on an interior line takes the cell to its right / above, as always.  The 1-D
 *  derivative handles offer "Pchip, Akima, CubicHermite (C1)  nu = 1" only, for the reason ndi_interp1d_derivative states:
 *  "a table holds one value per knot, so only a derivative that is continuous at the knots".  That reason does not bind here:
 *  a 2-D partial handle keeps no derivative table, it evaluates H_nu on the shared node table per cell, so
 *  ndi_interp2d_partial (every order of the spline handle), ndi_interp2d_eval_jet order 2 and the integral handles stay
 *  allowed, and the jump is the documented behaviour.
 *  Minimum points per axis: Pchip 2, Akima 3, caller-given 2.  Non-finite data is not refused; it flows through as IEEE
 *  values, as in 1-D.  The handle is a Bicubic handle in every other respect: every entry point, the AUTO / GATHER rule and
 *  the BUCKETED refusal, and the replica signature (the rule is not part of it, just as the boundary kinds are not).
 *  Device memory: the node table and the two knot axes; the build is a stencil that writes the table directly and keeps no
 *  grid-sized temporary beyond the uploaded z (host data), or the four uploaded arrays of the hermite call.
 * Periodic axes (ndi_interp2d_create_bicubic_periodic): the same Bicubic handle built so that the surface closes on itself
 * along x, along y or along both (longitude x latitude, angle x radius, a torus), and which wraps out-of-range queries on
 * those axes when it extrapolates.  `periodic_axes` is a bit set: bit 0 is x, bit 1 is y; 0 builds, bit for bit, the handle
 * ndi_interp2d_create_bicubic builds.  Numerical contract -- this project's own; every line one IEEE operation in T, in
 * this order, nothing fused.
 *  Build: a pass along a periodic axis is the CubicSpline coefficient build with periodic = 1 in the REFERENCE operation
 *  order (cubic_spline.rs:480-496 on 3 knots, :498-565 otherwise), followed by the same rule
 *                 zx[i]    = (dz + a[i]) / dx        i < nx-1
 *                 zx[nx-1] = zx[0]                   a copy
 *  (the cyclic system has k[nx-1] = k[0]: the rule's first row and its last row (dz - b[nx-2]) / dx are two roundings of
 *  that one knot derivative, an ulp apart; the copy makes them one); the cross pass along a periodic y is the periodic pass on zx.  A pass along a non-periodic axis is exactly the
 *  one above, the true not-a-knot row included, with that axis' two ends of any ndi_bc_kind.  The two `bc` entries of a
 *  periodic axis must be {NDI_BC_NOT_A_KNOT, 0} (or bc == NULL): a periodic end has no kind.
 *  The data must be periodic: z[0][j][c] != z[nx-1][j][c] for any j, c (along y: z[i][0][c] != z[i][ny-1][c]) is
 *  NDI_VALUE with a message naming Bicubic and the axis -- exact equality, as in the reference (cubic_spline.rs:501-507),
 *  so a NaN in the seam row fails it.
 *  The seam: along the pass the last row is the first row's copy, and across it the lanes of one pass run identical
 *  operations, so equal first and last data rows give a table that is periodic
 *  BIT FOR BIT: zx, zy, zxy at index 0 and at index n-1 of a periodic axis are the same bits.  Partials, the jet and the
 *  integrals read that table and nothing else, so they are seamless with it.
 *  Evaluation, per axis (cubic_spline.rs:763-769, 805-809).  extrapolate == 0: both axes take the inclusive range test; a
 *  periodic axis changes only the build.  extrapolate != 0: the handle WRAPS on its periodic axes -- a coordinate q outside
 *  [k0, kn] (the axis' first and last knot) is replaced before the search, and only when it is outside, by
 *     d = q - k0
 *     p = kn - k0
 *     r = fmod(d, p)
 *     if (r < 0) r = r + |p|
 *     qs = r + k0
 *  and cell, t, u, hx, hy come from qs.  fl(r + k0) may land an ulp past kn: the search then clamps to the last cell with t
 *  just over 1, as the 1-D handle does.  +-inf wraps to NaN and then fails exactly as a NaN query does (NDI_NAN_QUERY).  A
 *  non-periodic axis of such a handle continues its end cell's patch, as above.  x is tested before y for the same query,
 *  the lowest failing flat index wins, rows before it are written and later rows untouched; NDI_EVAL_FRESH_OUTPUT and
 *  NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED are unchanged.
 *  The periodic bits live on the handle: _clone copies them, ndi_interp2d_partial inherits them with the shared table, and
 *  ndi_interp2d_eval, async_launch / _finish, the ring, the sharded calls and ndi_interp2d_eval_jet honour them; part k of a
 *  jet stays, bit for bit, the separate partial handle's rows, wrapped queries included.  They are part of the replica
 *  signature: a sharded set that mixes handles with different periodic bits is refused.  ndi_interp2d_tables is unchanged.
 *  ndi_interp2d_antiderivative of a handle that wraps is NDI_BAD_ARG, naming the reason (the integral of a periodic surface
 *  is not periodic; the 1-D antiderivative refuses the Periodic extrapolation mode likewise); with extrapolate == 0 the
 *  integral handle of a periodic build is the one above.
 *  Handles that do not wrap launch the kernel instances they always did; the wrap is a compile-time variant of the
 *  evaluation kernels, taken once per query before the search.
 * Not provided: periodic local rules (ndi_interp2d_create_bicubic_local / _hermite), per-lane boundaries, integrals of
 * wrapping handles, a blocked-sweep periodic build for narrow grids, a different rule per axis, integrals of Bilinear or of partial
 * handles, partials of an integral handle, a second antiderivative, a ring / sharded / async_launch form of the four-array
 * rectangle call and of the jet call, a jet of a partial or of an integral handle, null entries in the jet's `outs` to skip
 * parts, jet orders above 2, third derivatives, a tile-grouped evaluation form, a blocked-sweep build for narrow grids,
 * half and integer element types. */
typedef struct ndi_interp1d ndi_interp1d; /* owns device copies of x, data (and a, b) */
typedef struct ndi_interp2d ndi_interp2d;

/* First failing query of a batch: the reference's query loop stops at the first Err
 * (src/interp1d/mod.rs:334-342, src/interp2d/mod.rs:297-306).  `index` is the lowest
 * flat query index that failed, `value` the offending coordinate and `axis` 0 for x,
 * 1 for y (x is tested before y for the same query: bilinear.rs:71-80), so the host
 * can format the reference's message ("x = {x:#?} is not in range").
 * Integer handles: the lowest failing query wins whether it is out of bounds or overflows; within a query the range
 * tests come first (x before y).  For NDI_INT_OVERFLOW `axis` is the ndi_int_op of the first overflowing operation in
 * the reference's order (lane by lane; z1, z2, then the y step for Bilinear) and `value` the query's x converted to
 * double -- lossy for i64 beyond 2^53: bindings format messages from the query element itself. */
typedef struct ndi_oob_info {
  uint64_t index;
  double value;
  int32_t axis;
  int32_t status; /* NDI_OUT_OF_BOUNDS, NDI_NAN_QUERY or NDI_INT_OVERFLOW */
} ndi_oob_info;

typedef struct ndi_eval_opts {
  int32_t q_memspace;   /* ndi_memspace of the query array(s) */
  int32_t out_memspace; /* ndi_memspace of the output buffer */
  void* stream;         /* hipStream_t the kernels are enqueued on; NULL = the HIP default stream
                           (hipStreamPerThread is accepted like any other handle) */
  int32_t path;         /* ndi_path */
  int32_t async_launch; /* != 0 (device out only): enqueue and return; fetch the batch
                           status later with ndi_interp{1,2}d_finish on the same stream (from the
                           same host thread); the query array(s) must stay valid until then.
                           Integer (i32 / i64) handles accept the flag but complete the batch inside
                           the call (no overlap with the caller); finish then reports its status */
  int32_t flags;        /* ndi_eval_flags */
  int32_t reserved;     /* 0 */
} ndi_eval_opts;

/* NDI_EVAL_FRESH_OUTPUT: the output buffer was allocated for this call and is dropped if the call fails -- what
 * Interp1D::interp_array / Interp2D::interp_array do (src/interp1d/mod.rs:197-211: `zeros(..)`, `?` on Err).  The
 * library may then write rows at / after the first failing query; status, index and value of the failure are reported as
 * always.  Without the flag (interp_array_into semantics: a caller-owned buffer) rows at / after the first failing query
 * are left untouched, as the reference's serial loop leaves them (:334-342) -- which costs the short-row kernels a
 * pre-pass over the queries (8-16 bytes per query, a quarter of the time of a scalar batch). */
/* NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED (v0.5): an interp_array_into caller's opt-in to the same kernels on a buffer it
 * OWNS -- if the call fails, rows at / after the first failing query hold unspecified values (rows before it are the
 * reference's, the failure report is unchanged).  The reference leaves those rows untouched (:334-342); a caller that
 * discards or overwrites the buffer on Err anyway gets the pre-pass back: scalar f64 data 200 -> 280 Gqueries/s.
 * Unknown flag bits and a non-zero `reserved` are refused with NDI_BAD_ARG (v0.5): a binary built against an older,
 * shorter ndi_eval_opts cannot silently select an option. */
typedef enum ndi_eval_flags {
  NDI_EVAL_DEFAULT = 0,
  NDI_EVAL_FRESH_OUTPUT = 1,
  NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED = 2
} ndi_eval_flags;

/* ---- build ------------------------------------------------------------------ */
ndi_status ndi_interp1d_create(const ndi_interp1d_desc* desc, ndi_interp1d** out);
/* NDI_CUBIC_HERMITE: the cubic Hermite interpolant of `desc->data` with the caller's knot derivatives k = dydx,
 * T[n * lanes] in desc->memspace, laid out like the data (ndi_strategy1d states the tables; no rule is applied to k, so
 * there is nothing of scipy's to deviate from).  desc->strategy must be NDI_CUBIC_HERMITE; ndi_interp1d_create refuses that
 * strategy with NDI_BAD_ARG.  The handle is an ndi_interp1d like any other. */
ndi_status ndi_interp1d_create_hermite(const ndi_interp1d_desc* desc, const void* dydx, ndi_interp1d** out);
/* An x axis PER LANE (this project's own; np.interp per row with xp, fp and the queries all batched): `x_lanes` is
 * T[n][lanes] in desc->memspace, C order like `data`; column l holds the knots of lane l, and lane l of the handle is the
 * interpolant of (x_lanes[:, l], data[:, l]) alone -- a calibration curve per channel, each measured at its own abscissae.
 * desc->x must be NULL and desc->x_len == n.  `dydx` is T[n][lanes] for NDI_CUBIC_HERMITE and NULL otherwise.  f32 / f64 only:
 * the integer and half-precision types are NDI_UNSUPPORTED.  `*out` is cleared first.  The handle is an ndi_interp1d.
 * Strategies: NDI_LINEAR, NDI_PCHIP, NDI_AKIMA, NDI_CUBIC_HERMITE, and NDI_CUBIC_SPLINE with the global ends desc->left /
 * desc->right (NotAKnot, Natural, Clamped, FirstDeriv, SecondDeriv; the n == 3 NotAKnot x NotAKnot parabola rows included).
 * desc->periodic and the four lane_* arrays (BoundaryCondition::Individual) are NDI_UNSUPPORTED with a message that names
 * the reason.  The minimum lengths are the strategies' own (NDI_NOT_ENOUGH_DATA below them).  desc->validate and
 * desc->build_flags are not read: the columns are always checked, and the build is always in the reference's order.
 * Validation: every column must be strictly rising with no NaN, else NDI_MONOTONIC with the text
 * "Values in the x axis need to be strictly monotonic rising (lane L)", L the lowest offending lane.  Host arrays are
 * checked on the host before any device work (the error comes back on a machine with no GPU); device arrays by one
 * kernel pass.  The build runs on the NULL stream and is complete on return.
 * Build value rule: ndi_interp1d_coefficients(h, a, b, ...) returns tables whose column l is, bit for bit, what it returns for
 * the shared-axis handle built from (x_lanes[:, l], data[:, l]) alone with the same strategy and ends and build_flags =
 * NDI_BUILD_REFERENCE_ORDER.  Every line of the build is one IEEE operation in T, nothing fused, divisions correctly
 * rounded: the local cubics are the stencil stated at ndi_strategy1d with h_i = x[i+1][l] - x[i][l]; the spline forms
 * low / mid / up, w = low[i] / mid'[i-1], mid'[i] = mid[i] - w * up[i-1] and the boundary rows per lane in the reference's
 * operation order (cubic_spline.rs:409-721; a, b :350-365).
 * Evaluation: the handle takes both entry points,
 *     ndi_interp1d_eval(h, q[nq], ...)                         out[j][l] = f_l(q[j])
 *     ndi_interp1d_eval_lanewise(h, q[nq][q_row_stride], ...)  out[j][l] = f_l(q[j][l]).
 * The search is part of the contract:  lo = 0, hi = n-1;  while (hi - lo > 1) { mid = (lo + hi) >> 1;
 * if (x[mid][l] <= q) lo = mid; else hi = mid; }  -- the unique cell with x[i] <= q < x[i+1], clamped to [0, n-2], so
 * q == x[n-1][l] lands in n-2 with t = 1.  Linear evaluates ((y2-y1)/(x2-x1)) * (q-x1) + y1; the cubic class t = (q - xl) /
 * (xr - xl) and cubic_spline.rs:824-828.
 * Evaluation value rule: out[j][l] is, bit for bit and zero signs included, element 0 of the row ndi_interp1d_eval writes for
 * that query on the single-column handle of lane l -- with `extrapolate` too, where each lane continues its own end
 * interval.
 * Range and errors: ndi_interp1d_eval tests the range common to all lanes, Lo = max_l x[0][l], Hi = min_l x[n-1][l] (a
 * query outside it is outside some lane's range; Lo > Hi is allowed, then every query fails).  Without `extrapolate` the
 * lowest failing query index wins: info->index = j, info->value = q[j], axis 0, "x = ... is not in range"; rows before it
 * are written and later rows are untouched (NDI_EVAL_FRESH_OUTPUT: the kernel tests the queries itself, later rows are
 * unspecified).  With `extrapolate` a NaN gives NDI_NAN_QUERY.  ndi_interp1d_eval_lanewise tests each element against its
 * own lane's [x[0][l], x[n-1][l]] and reports the first failing flat element j * lanes + l, as on every other handle.
 * Not provided, each NDI_UNSUPPORTED with a message: NDI_PATH_BUCKETED (there is no common interval to group queries by),
 * async_launch on the lane-wise call, ndi_interp1d_eval_ring, the sharded calls, ndi_interp1d_derivative, _antiderivative
 * and _inverse.  ndi_interp1d_clone copies the tables; ndi_interp1d_data, _coefficients (cubic class), _destroy and _trim
 * work as on any handle. */
ndi_status ndi_interp1d_create_lane_axes(const ndi_interp1d_desc* desc, const void* x_lanes, const void* dydx,
                                         ndi_interp1d** out);
void ndi_interp1d_destroy(ndi_interp1d* h);
ndi_status ndi_interp2d_create(const ndi_interp2d_desc* desc, ndi_interp2d** out);
/* The Bicubic strategy (contract above ndi_interp1d).  `bc`: four boundaries in the order x-left, x-right, y-left, y-right,
 * or NULL for NotAKnot on all four.  A new symbol; ndi_interp2d_desc keeps its layout. */
ndi_status ndi_interp2d_create_bicubic(const ndi_interp2d_desc* desc, const ndi_boundary* bc, ndi_interp2d** out);
/* Bicubic with periodic axes (contract above ndi_interp1d).  periodic_axes: bit 0 is x, bit 1 is y; 0 is
 * ndi_interp2d_create_bicubic.  NDI_BAD_ARG, *out cleared first: bits outside 0 .. 3; a `bc` entry of a periodic axis other
 * than {NDI_BC_NOT_A_KNOT, 0} (the message names Bicubic, the axis and the reason); and every refusal of
 * ndi_interp2d_create_bicubic (element types, null arguments; NDI_NOT_ENOUGH_DATA below 3 points on an axis).  NDI_VALUE:
 * the first and last data rows along a periodic axis differ.  A new symbol: no new enumerator, no struct change, no
 * version change. */
ndi_status ndi_interp2d_create_bicubic_periodic(const ndi_interp2d_desc* desc, const ndi_boundary* bc,
                                                int32_t periodic_axes, ndi_interp2d** out);
/* Bicubic with the node derivatives of a local rule (contract above ndi_interp1d).  rule: NDI_PCHIP or NDI_AKIMA
 * (ndi_strategy1d), the same on both axes.  Refused before any device work, *out cleared first, the message naming the
 * strategy and the reason: NDI_BAD_ARG for a null `desc` or `out`, any other rule, integer and f16 / bf16 dtypes;
 * NDI_NOT_ENOUGH_DATA for fewer than 2 (Pchip) / 3 (Akima) points on an axis; `validate` as in
 * ndi_interp2d_create_bicubic.  Built on the NULL stream, complete on return.  A new symbol: no new enumerator, no struct
 * change. */
ndi_status ndi_interp2d_create_bicubic_local(const ndi_interp2d_desc* desc, int32_t rule, ndi_interp2d** out);
/* Bicubic with the caller's node derivatives: zx, zy, zxy are T[nx][ny][lanes] in desc->memspace, laid out like the data; no
 * rule is applied (the 2-D counterpart of ndi_interp1d_create_hermite; ndi_interp2d_tables of another handle gives such
 * arrays).  At least 2 points per axis.  Refusals as above, and NDI_BAD_ARG for a null table. */
ndi_status ndi_interp2d_create_bicubic_hermite(const ndi_interp2d_desc* desc, const void* zx, const void* zy,
                                               const void* zxy, ndi_interp2d** out);
/* The node derivatives of a Bicubic handle as plain T[nx][ny][lanes] arrays, whatever the internal layout (any of the three
 * may be NULL): the 2-D counterpart of ndi_interp1d_coefficients.  NDI_BAD_ARG for a Bilinear handle. */
ndi_status ndi_interp2d_tables(const ndi_interp2d* h, void* zx, void* zy, void* zxy, int32_t memspace);
/* A new handle that evaluates the partial derivative of orders (nu_x, nu_y) of `h`'s surface (contract above ndi_interp1d):
 * the 2-D counterpart of ndi_interp1d_derivative.  `h`: a Bicubic handle or a partial handle of one; orders add (a partial of
 * a partial acts as if asked of the origin with the orders summed); after summing nu_x, nu_y in {0, 1, 2}.  NDI_BAD_ARG, with
 * *out cleared first and a message naming the strategy and the reason, decided before any device work: a Bilinear handle,
 * an order below 0 or summing above 2, (0, 0), a null `h` or `out`.  The new handle shares `h`'s node table and has its
 * knots, `extrapolate` and device; either may be destroyed first.  A new symbol: no new enumerator, no struct change. */
ndi_status ndi_interp2d_partial(const ndi_interp2d* h, int32_t nu_x, int32_t nu_y, ndi_interp2d** out);
/* A new handle that evaluates F, the integral of `h`'s surface from (x[0], y[0]) (contract above ndi_interp1d): the 2-D
 * counterpart of ndi_interp1d_antiderivative.  `h`: a Bicubic surface handle.  NDI_BAD_ARG, with *out cleared first and a
 * message naming the strategy and the reason, decided before any device work: a Bilinear handle, a partial handle, an
 * integral handle, a null `h` or `out`.  The new handle shares `h`'s node table, owns its five prefix tables (built on the
 * NULL stream, complete on return) and has `h`'s knots, `extrapolate` and device; either may be destroyed first.
 * ndi_interp2d_partial of an integral handle is NDI_BAD_ARG (its x-derivative is a y-integral, which is not provided).
 * New symbols: no new enumerator, no struct change. */
ndi_status ndi_interp2d_antiderivative(const ndi_interp2d* h, ndi_interp2d** out);
/* Rectangle integrals through an integral handle (scipy: .integral(xa, xb, ya, yb)): out[q][l] = the integral of lane l
 * over [xa[q], xb[q]] x [ya[q], yb[q]], four searches, four F and three subtractions in ONE evaluation launch.  `h` must be
 * an integral handle (anything else: NDI_BAD_ARG).  Host or device bounds and outputs (ndi_eval_opts), strided rows.
 * Errors: the lowest failing flat index wins; within a query the order is xa, xb, ya, yb; info->axis is 0 for an x bound
 * and 1 for a y bound, info->value the offending bound; rows before the failing index are written, later rows untouched
 * (NDI_EVAL_FRESH_OUTPUT and NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED are honoured); NDI_NAN_QUERY by Bilinear's rule.
 * NDI_PATH_BUCKETED is NDI_BAD_ARG.  async_launch != 0 is NDI_UNSUPPORTED: the call completes before it returns (the four
 * bounds do not fit the two-array record ndi_interp2d_finish reports from). */
ndi_status ndi_interp2d_integral(const ndi_interp2d* h, const void* xa, const void* xb, const void* ya, const void* yb,
                                 uint64_t nq, void* out, uint64_t out_row_stride, const ndi_eval_opts* opts,
                                 ndi_oob_info* info);
/* The five prefix tables of an integral handle as plain T[nx][ny][lanes] arrays, whatever the internal layout (any of them
 * may be NULL): the counterpart of ndi_interp2d_tables.  NDI_BAD_ARG for any handle that is not an integral handle. */
ndi_status ndi_interp2d_integral_tables(const ndi_interp2d* h, void* pp, void* qz, void* qzy, void* pz, void* pzx,
                                        int32_t memspace);
/* The surface and its partial derivatives up to `order` at the same queries, in ONE evaluation launch (contract above
 * ndi_interp1d).  `order` is 1 or 2 and selects K = 3 or 6 parts in the fixed order of (nu_x, nu_y)
 *     order 1: (0,0), (1,0), (0,1)        order 2: (0,0), (1,0), (0,1), (2,0), (1,1), (0,2)
 * Part k is, bit for bit, what ndi_interp2d_eval of ndi_interp2d_partial(h, nu_x, nu_y) writes for the same queries; part 0
 * is what ndi_interp2d_eval(h) writes.  `outs` is a HOST array of K pointers (whatever out_memspace says about what they
 * point to); part k of query i, lane l goes to outs[k][i * out_row_stride + l]: ONE row stride in elements, >= lanes,
 * common to all parts.  Both natural layouts are expressible: planar (K, nq, lanes) is stride = lanes with the bases
 * nq * lanes apart, interleaved (nq, K, lanes) is stride = K * lanes with the bases lanes apart.  Parts must not overlap:
 * two equal pointers in `outs` are refused, any other overlap is the caller's responsibility.  The 16-byte vector form is
 * taken when lanes and the stride are multiples of a vector and ALL K bases are 16-byte aligned, else every part takes
 * the scalar form (the same bits).
 * `h` must be a Bicubic surface handle: a Bilinear handle, a partial handle (a jet of a partial would need third orders)
 * and an integral handle are NDI_BAD_ARG with a message naming the strategy and the reason.  Also NDI_BAD_ARG, all decided
 * before any device work: `order` outside {1, 2}; a null `h` or `outs`; with nq > 0 a null query pointer or a null
 * outs[k]; two equal pointers in `outs`; out_row_stride < lanes; NDI_PATH_BUCKETED.  async_launch != 0 is NDI_UNSUPPORTED:
 * the call completes before it returns (the partial handles have an async_launch form).  nq == 0 is NDI_OK and touches
 * nothing.
 * Errors are ndi_interp2d_eval's: the lowest failing flat index wins, x before y, `info` filled the same way; without
 * NDI_EVAL_FRESH_OUTPUT rows before the failing index are written in EVERY part and rows from it on are untouched in EVERY
 * part (a range pre-pass over the queries); with it there is no pre-pass and the kernel applies its own range test;
 * NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED is honoured as elsewhere.  Thread-safety is ndi_interp2d_eval's.
 * Not provided: ring, sharded and async_launch forms; a jet of a partial or of an integral handle; null entries in `outs`
 * to skip parts; orders above 2.  A new symbol: no new enumerator, no struct change. */
ndi_status ndi_interp2d_eval_jet(const ndi_interp2d* h, int32_t order, const void* qx, const void* qy, uint64_t nq,
                                 void* const* outs, uint64_t out_row_stride, const ndi_eval_opts* opts, ndi_oob_info* info);
void ndi_interp2d_destroy(ndi_interp2d* h);

/* A replica of a built interpolator on `device` (any device, the handle's own included): the device-resident knots /
 * data / spline tables are copied device to device (between two GPUs: over xGMI) -- the caller's arrays are not
 * uploaded again and CubicSpline::build's Thomas solve (cubic_spline.rs:754-771) is not repeated.  What the sharded
 * calls below take as `handles`: knots / coefficients replicated per device.  The replica is independent of the
 * original (destroy each with ndi_interp{1,2}d_destroy). */
ndi_status ndi_interp1d_clone(const ndi_interp1d* h, int32_t device, ndi_interp1d** out);
ndi_status ndi_interp2d_clone(const ndi_interp2d* h, int32_t device, ndi_interp2d** out);

/* CubicSplineStrategy{a, b} (cubic_spline.rs:94-102): copies the coefficient tables,
 * each T[(n-1) * lanes], to `a_out` / `b_out` (either may be NULL). */
ndi_status ndi_interp1d_coefficients(const ndi_interp1d* h, void* a_out, void* b_out,
                                     int32_t memspace);

/* Copies the handle's resident data table, T[n * lanes], to `data_out` (any 1-D handle; an integer handle hands back the
 * values of its slope records).  For a handle made by ndi_interp1d_create it is the caller's data; for a derivative
 * handle it is Y below. */
ndi_status ndi_interp1d_data(const ndi_interp1d* h, void* data_out, int32_t memspace);

/* The nu-th derivative of a piecewise cubic interpolant as a NEW HANDLE (scipy: CubicSpline.derivative(nu), cs(x, nu)).
 * The evaluation computes (1-t) y_l + t y_r + t (1-t) (a (1-t) + b t) for any tables {y, a, b}; the derivative of a
 * piecewise cubic is a piecewise quadratic, and a quadratic is exactly of that form with a == b.  So the new handle's
 * three tables are computed from `h`'s three tables by one device pass, and it takes every evaluation entry point, path,
 * AUTO rule, the ring, ndi_interp1d_clone, the sharded calls, ndi_interp1d_coefficients and ndi_interp1d_data like any
 * handle.  It is built on h's device (other devices: ndi_interp1d_clone), `h` is only read and stays usable -- also
 * concurrently -- and is destroyed independently.  Knots, `extrapolate` and the periodic mode are h's.
 * Numerical contract -- this project's own.  Source tables y[n][L], a[n-1][L], b[n-1][L], knots x[n]; per interval i and
 * lane, dx = x[i+1] - x[i], dy = y[i+1] - y[i]; each line one IEEE operation in T, in this order, nothing fused:
 *     Y[i]   = (dy + a[i]) / dx                 i = 0 .. n-2     the derivative at the left end of interval i
 *     Y[n-1] = (dy - b[n-2]) / dx               with i = n-2     the derivative at the last knot
 *     A[i]   = B[i] = (3 * (b[i] - a[i])) / dx
 * {Y, A, B} are the new handle's data and coefficient tables.  (With q(t) = y_l + t dy + t (1-t) (a + (b-a) t): dq/dt is
 * dy + a at 0 and dy - b at 1, its second t-derivative is -6 (b-a); a quadratic p is (1-t) p0 + t p1 + t (1-t) c with
 * c = -p''/2.)  nu = 2 is the rule applied twice: there 3 * (B - A) is exactly 0, so the result is the piecewise-linear
 * interpolant of Y'[i] = ((Y[i+1] - Y[i]) + A[i]) / dx with zero coefficient tables.
 * Which orders exist -- a table holds one value per knot, so only a derivative that is continuous at the knots:
 *     CubicSpline (C2; every boundary kind, periodic, per-lane boundaries)   nu = 1, nu = 2
 *     Pchip, Akima, CubicHermite (C1)                                        nu = 1
 *     a derivative handle                          as if asked of its origin with the orders added
 *     Linear, integer, f16 / bf16 handles          none
 * Everything else (nu < 1, nu > 2, a null pointer included) is NDI_BAD_ARG with a message that names the source's strategy
 * and the reason, decided before any device work.
 * Where continuity holds only to rounding, an interior knot carries the value of the interval to its RIGHT: a query at
 * that knot returns Y[i] exactly, a query just left of it evaluates the left interval's polynomial, whose end value
 * (dy - b[i-1]) / dx of interval i-1 differs from Y[i] by rounding for a first derivative, and for a spline's second
 * derivative by the residual of the Thomas solve at that knot.  An antiderivative handle (ndi_interp1d_antiderivative)
 * follows the same convention: a query at an interior knot x[i] returns P[i] exactly (interval i at t = 0); a query at the
 * LAST knot evaluates interval n-2 at t = 1, and that result may differ from P[n-1] by rounding.
 * Y is always re-derived from y, a, b; a k table the source may have kept is never read, so the bits do not depend on
 * whether it kept one.  For NDI_CUBIC_HERMITE, Y[i] is therefore the caller's dydx[i] up to the rounding of
 * ((k dx - dy) + dy) / dx, not its bits.  A derivative handle keeps no k table of its own: the evaluation form that holds
 * {y, k} in LDS re-forms a / b from k and could not reproduce A == B bit for bit, so AUTO gives such handles the forms
 * that read a / b (scalar and short-row data: a measured cost).
 * Not provided: second derivatives of the C1 strategies, third derivatives. */
ndi_status ndi_interp1d_derivative(const ndi_interp1d* h, int32_t nu, ndi_interp1d** out);

/* The antiderivative F of an interpolant as a NEW HANDLE (scipy: CubicSpline.antiderivative(), PchipInterpolator
 * .antiderivative()), F(x[0]) = +0 for every lane.  It is built on h's device, `h` is only read and stays usable, the new
 * handle keeps its own copies of what it reads and is destroyed independently; knots and `extrapolate` are h's.
 * Sources: f32 / f64 handles of the cubic evaluation class (CubicSpline with every boundary kind and per-lane boundaries,
 * Pchip, Akima, CubicHermite, and their derivative handles) and f32 / f64 Linear handles.  Refused with NDI_BAD_ARG, before
 * any device work, with a message that names the strategy and the reason: integer handles, f16 / bf16 handles, an
 * antiderivative handle, a handle whose extrapolation mode is Periodic, a null `h` or `out` (`*out` is cleared first).
 * Numerical contract -- this project's own.  Every line is one IEEE operation in T, in this order, nothing fused.  Per
 * interval i and lane, with yl = y[i], yr = y[i+1], a = a[i], b = b[i] and dx = x[i+1] - x[i]:
 *     cubic class:   dy = yr - yl
 *                    c1 = (dy + a) * 0.5
 *                    c2 = (b - (a + a)) / 3
 *                    c3 = (b - a) * 0.25
 *                    G(t) = t * (yl + t * (c1 + t * (c2 - t * c3)))
 *                    I[i] = dx * (yl + (c1 + (c2 - c3)))              (= dx * G(1))
 *     Linear:        c1 = (yr - yl) * 0.5
 *                    G(t) = t * (yl + t * c1)
 *                    I[i] = dx * (yl + c1)
 *     evaluation:    t = (xq - x[i]) / dx          (the cubic evaluation's t, interval by get_lower_index)
 *                    F(xq) = P[i] + dx * G(t)
 * (q(t) = yl + (dy + a) t + (b - 2a) t^2 - (b - a) t^3, and its integral over [0, 1] is (yl + yr) / 2 + (a + b) / 12.)
 * `extrapolate` continues the end interval's quartic: t falls outside [0, 1].
 * The prefix table P[n][lanes] is a FIXED blocked sum with B = 256 knots per block; its bits do not depend on the launch
 * geometry:
 *     local sums:    S[i] = +0 where i % B == 0, otherwise S[i] = S[i-1] + I[i-1]
 *     block totals:  T[k] = S[kB + B - 1] + I[kB + B - 1]      the local running sum taken over the block's end
 *     block offsets: O[0] = +0, O[k+1] = O[k] + T[k]           summed serially
 *     table:         P[i] = O[i / B] + S[i]                    i = 0 .. n-1
 * What an antiderivative handle takes: ndi_interp1d_eval in every form (sync, async_launch + ndi_interp1d_finish, host or
 * device queries and outputs, strided rows; with a HOST output buffer async_launch is accepted and the call completes
 * before it returns, as for every 1-D handle: the rows are copied out of a staging buffer) with the source's range, NaN and first-error semantics and messages (the
 * lowest failing flat index is reported, rows before it are written, later rows are untouched; NDI_EVAL_FRESH_OUTPUT and
 * NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED are accepted and ignored); ndi_interp1d_data (hands back P); ndi_interp1d_clone,
 * ndi_interp1d_trim, ndi_interp1d_destroy.  ndi_interp1d_coefficients, ndi_interp1d_derivative and
 * ndi_interp1d_antiderivative of it are NDI_BAD_ARG with a reason; ndi_interp1d_eval_ring, the sharded calls and
 * NDI_PATH_BUCKETED are NDI_UNSUPPORTED with a message.  A function and its antiderivative are not replicas of each other
 * (a sharded call that mixes them is refused as any non-replica set is).
 * Not provided: the Periodic extrapolation mode, second antiderivatives, 2-D, integer and f16 / bf16 element types. */
ndi_status ndi_interp1d_antiderivative(const ndi_interp1d* h, ndi_interp1d** out);

/* Definite integrals through an antiderivative handle (scipy: .integrate(a, b)): out[j][l] = F(hi[j])[l] - F(lo[j])[l],
 * one subtraction in T, for nq pairs; `lo`, `hi` are T[nq] in opts->q_memspace, `out` as for ndi_interp1d_eval.  `h` must
 * be an antiderivative handle (anything else: NDI_BAD_ARG).  lo > hi is allowed and gives the negated integral; lo == hi
 * gives F - F.  Both searches, both evaluations and the subtraction are ONE evaluation launch.  Errors: the lowest failing
 * flat index is reported, lo[j] is tested before hi[j]; info->axis is 0 for lo and 1 for hi; rows before the failing index
 * are written, later rows are untouched, as for ndi_interp1d_eval. */
ndi_status ndi_interp1d_integrate(const ndi_interp1d* h, const void* lo, const void* hi, uint64_t nq,
                                  void* out, uint64_t out_row_stride,
                                  const ndi_eval_opts* opts, ndi_oob_info* info);

/* The inverse of an interpolant as a NEW HANDLE (scipy: PPoly.solve / CubicSpline.solve, one root per lane): the new
 * handle's queries are VALUES v and its rows are abscissae,
 *     out[j * out_row_stride + l] = x   with   f_l(x) = v[j].
 * It is built on h's device, `h` is only read and stays usable, the new handle keeps its own copies of what it reads (as an
 * antiderivative handle does) and either handle may be destroyed first.
 * Sources (f32 and f64 only): Linear; the cubic evaluation class (CubicSpline with every boundary kind, Pchip, Akima,
 * CubicHermite, and derivative handles); antiderivative handles of either (a CDF: F^-1(u) is inverse-transform sampling).
 * Refused with NDI_BAD_ARG, before any device work, with a message that names the strategy and the reason: integer and
 * f16 / bf16 handles, a handle whose extrapolation mode is Periodic, an inverse handle, a null `h` or `out` (`*out` is
 * cleared first).
 * The node table N[n][lanes] is the data table y (Linear and cubic sources) or the prefix table P (antiderivative sources).
 * Every lane of N must be monotone; ties are allowed (a density that is zero over an interval gives a flat run in P).  One
 * device pass at creation checks it: a lane that both rises and falls, or holds a NaN, gives NDI_MONOTONIC, and the
 * message names the lowest such lane.  Per lane, rising = N[n-1][l] >= N[0][l].  The handle keeps the value range common
 * to all lanes, Lo = max_l min(N[0][l], N[n-1][l]) and Hi = min_l max(N[0][l], N[n-1][l]).
 * Evaluation: ndi_interp1d_eval in every form (sync, async_launch + ndi_interp1d_finish, host or device queries and
 * outputs, strided rows).  A row is defined only where v lies in every lane's range: v outside [Lo, Hi] (inclusive test)
 * is NDI_OUT_OF_BOUNDS, a NaN is NDI_NAN_QUERY; the lowest failing flat index is reported with value = v and axis = 0, rows
 * before it are written, later rows are untouched (NDI_EVAL_FRESH_OUTPUT and NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED are
 * accepted and ignored).  `extrapolate` of the source is IGNORED: the inverse is defined on the node range only.
 * Numerical contract -- this project's own.  Every line is one IEEE operation in T, in this order, nothing fused.  Per
 * output element (query v, lane l, column c = N[:, l]):
 *     search   lo = 0, hi = n-1;  while hi - lo > 1:  mid = (lo + hi) >> 1
 *                  if (rising ? c[mid] <= v : c[mid] >= v) lo = mid else hi = mid
 *              i = lo;  nl = c[i], nr = c[i+1];  xl = x[i], xr = x[i+1];  dx = xr - xl
 *     start    if v == nl:  t = 0                         -> finish
 *              t = (v - nl) / (nr - nl)                   Linear sources: -> finish (closed form)
 *     solve    tl = 0, th = 1, dprev = 1;   repeat at most K times:
 *                  f = p(t) - v;            if f == 0: stop
 *                  if (rising ? f < 0 : f > 0) tl = t else th = t
 *                  d = p'(t);  s = f / d;  tn = t - s
 *                  if !(tn > tl && tn < th) or !(|s + s| <= |dprev|):  tn = tl + 0.5 * (th - tl)
 *                  step = tn - t;  dprev = step;  t = tn
 *                  if |step| <= eps_T: stop                eps_T = 2^-52 (f64) / 2^-23 (f32)
 *     finish   w = xl + t * dx;  x = (t == 1) ? xr : min(w, xr)          min(w, xr) = (w < xr) ? w : xr
 * p(t) is exactly the forward evaluation's expression of the class, with yl = y[i], yr = y[i+1], a = a[i], b = b[i]:
 *     cubic class:                p(t)  = ((1-t) yl + t yr) + (t (1-t)) (a (1-t) + b t)
 *                                 p'(t) = (dy + a) + t (((b - (a+a)) + (b - (a+a))) - (3 (b - a)) t)        dy = yr - yl
 *     antiderivative, cubic:      p(t)  = P[i] + dx * (t (yl + t (c1 + t (c2 - t c3))))
 *                                 p'(t) = dx * (yl + t ((c1 + c1) + t (3 c2 - (4 c3) t)))
 *     antiderivative of Linear:   p(t)  = P[i] + dx * (t (yl + t c1))
 *                                 p'(t) = dx * (yl + t (c1 + c1))
 * with c1, c2, c3 as stated for ndi_interp1d_antiderivative.  K = 128 (f64) / 64 (f32) is a safety net, not part of the
 * accuracy argument: the |step| <= eps_T stop ends the iteration long before it.
 * Properties: (1) the returned x is in [xl, xr], so a forward evaluation of it is never out of bounds; (2) a comparison
 * with NaN or an infinite Newton step falls into the bisection branch, so the loop terminates for any table contents;
 * (3) t always lies in a bracket across which the COMPUTED residual changes sign: where the interpolant is monotone on
 * the interval (Linear, Pchip, and CDFs always) that is THE root, for an overshooting spline it is A root of that
 * interval; (4) for a value taken on a whole flat run the run's right end is returned (the search takes the last i with
 * c[i] == v; a flat run that reaches the last node returns x[n-2], the left end of the last interval).
 * Other entry points on an inverse handle: ndi_interp1d_data hands back N; ndi_interp1d_clone, ndi_interp1d_trim and
 * ndi_interp1d_destroy work.  ndi_interp1d_coefficients, ndi_interp1d_derivative, ndi_interp1d_antiderivative,
 * ndi_interp1d_integrate and ndi_interp1d_inverse of it are NDI_BAD_ARG with a reason; ndi_interp1d_eval_ring, the
 * sharded calls and NDI_PATH_BUCKETED are NDI_UNSUPPORTED with a message.
 * A value per lane (independent quantiles: inverse-transform sampling from `lanes` densities) is ndi_interp1d_eval_lanewise.
 * Not provided: all roots of a non-monotone interpolant, extrapolated inverses, 2-D, the ring, the sharded calls, integer
 * and f16 / bf16 element types. */
ndi_status ndi_interp1d_inverse(const ndi_interp1d* h, ndi_interp1d** out);

/* ---- evaluate ----------------------------------------------------------------
 * Replaces Interp1D::interp_array_into for a flattened query array
 * (src/interp1d/mod.rs:272-343) with Linear::interp_into (linear.rs:73-98) or
 * CubicSplineStrategy::interp_into (cubic_spline.rs:791-830) as the per-query body:
 *   out[i * out_row_stride + l] = strategy(q[i])[l],  i < nq, l < lanes.
 * out_row_stride is in elements (>= lanes).  On NDI_OUT_OF_BOUNDS / NDI_NAN_QUERY
 * rows before info->index are written and later rows are untouched, as in the
 * reference.  General-rank queries are a flatten on the caller's side. */
ndi_status ndi_interp1d_eval(const ndi_interp1d* h, const void* q, uint64_t nq, void* out,
                             uint64_t out_row_stride, const ndi_eval_opts* opts,
                             ndi_oob_info* info);

/* Lane-wise evaluation, a query per lane (this project's own; the reference evaluates all lanes at one abscissa):
 *     out[j * out_row_stride + l] = f_l(q[j * q_row_stride + l]),   j < nq, l < lanes.
 * `q` is T[nq][q_row_stride] in opts->q_memspace, `out` is T[nq][out_row_stride] in opts->out_memspace; both strides are
 * in elements and at least lanes.
 * Value rule: out[j][l] is, bit for bit and zero signs included, element l of the row ndi_interp1d_eval(h) writes for the single query q[j][l].
 * It holds for every handle kind the call accepts, every extrapolation mode (none, end-interval, periodic wrap) and
 * whatever path, table layout or kernel form is taken.
 * Handles accepted (f32 and f64 only): Linear; the cubic evaluation class (CubicSpline with every boundary kind, Pchip,
 * Akima, CubicHermite, and derivative handles); antiderivative handles; inverse handles, where `q` holds values and `out`
 * abscissae.  Integer and f16 / bf16 handles are NDI_BAD_ARG with a message that names the strategy.
 * Failures: the lowest failing flat ELEMENT index j * lanes + l wins (computed with lanes, not with the strides);
 * info->index is that index, info->value is q[j][l], info->axis is 0; status and message are those of ndi_interp1d_eval on
 * the handle ("x = ... is not in range", NDI_NAN_QUERY for a NaN the search meets).  Forward and antiderivative handles
 * test against the knot range with the extrapolation mode's rule; an inverse handle tests q[j][l] against lane l's OWN
 * value range [min(N[0][l], N[n-1][l]), max(N[0][l], N[n-1][l])], not the range common to all lanes (a NaN is
 * NDI_NAN_QUERY).  Rows j < index / lanes are written whole; the failing row and all later rows are untouched.
 * NDI_EVAL_FRESH_OUTPUT and NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED drop the pre-pass over the queries that this needs: the
 * report is the same, the rows at and after the failing row are then unspecified.
 * Refused before any device work: a null `h`, with nq > 0 a null `q` or `out`, a stride below lanes, NDI_PATH_BUCKETED,
 * unknown flag bits or a non-zero `reserved` (all NDI_BAD_ARG); async_launch != 0 is NDI_UNSUPPORTED (the finish record
 * carries no element index).  nq == 0 is NDI_OK and touches nothing.
 * Host arrays go through device staging in row chunks; only rows before the failing row are copied back.  Linear / cubic
 * handles may keep an element-record copy of their tables for this call (built on the first lane-wise call, at most 1 GiB,
 * released by ndi_interp1d_trim; a clone builds its own).
 * Not provided: the ring, the sharded calls, async_launch, integer and f16 / bf16 element types.  (The 2-D form is
 * ndi_interp2d_eval_lanewise, below.) */
ndi_status ndi_interp1d_eval_lanewise(const ndi_interp1d* h, const void* q, uint64_t nq, uint64_t q_row_stride,
                                      void* out, uint64_t out_row_stride, const ndi_eval_opts* opts, ndi_oob_info* info);

/* Replaces Interp2D::interp_array_into (src/interp2d/mod.rs:215-307) with
 * Bilinear::interp_into (bilinear.rs:64-99) as the per-query body. */
ndi_status ndi_interp2d_eval(const ndi_interp2d* h, const void* qx, const void* qy, uint64_t nq,
                             void* out, uint64_t out_row_stride, const ndi_eval_opts* opts,
                             ndi_oob_info* info);

/* Lane-wise 2-D evaluation, an (x, y) per lane (this project's own; the reference evaluates all lanes at one point):
 *     out[j * out_row_stride + l] = f_l(qx[j * q_row_stride + l], qy[j * q_row_stride + l]),   j < nq, l < lanes.
 * `qx` and `qy` are T[nq][q_row_stride] in opts->q_memspace and share one pitch, `out` is T[nq][out_row_stride] in
 * opts->out_memspace; both strides are in elements and at least lanes.
 * Value rule: out[j][l] is, bit for bit and zero signs included, element l of the row ndi_interp2d_eval(h) writes for the single query (qx[j][l], qy[j][l]).
 * It holds for every handle the call accepts, every extrapolation mode, every table layout and every kernel form.
 * Handles accepted (f32 and f64 only): Bilinear, in whichever layout the handle keeps its grid; Bicubic from every build
 * (the spline with any boundary kinds, pchip, akima, hermite, periodic axes -- a handle that wraps takes the wrap once per
 * coordinate, before the search) and every partial-derivative handle of one (orders 0 .. 2 per variable).  An integral
 * handle (ndi_interp2d_antiderivative: the integral of a surface per lane is not provided), integer and f16 / bf16
 * handles are NDI_BAD_ARG with a message that names the reason.
 * Failures: the lowest failing flat ELEMENT index j * lanes + l wins (computed with lanes, not with the strides).  The two
 * axes are recorded separately and x is reported before y for the same element: info->index is that index, info->value
 * is qx[j][l] or qy[j][l], info->axis is 0 or 1; status and message are those of ndi_interp2d_eval on the handle
 * ("x = ... is not in range" / "y = ...", NDI_NAN_QUERY where the handle extrapolates; on a wrapping axis the test is
 * "finite after the wrap", so +-inf is NDI_NAN_QUERY).  Rows j < index / lanes are written whole; the failing row and all
 * later rows are untouched.  NDI_EVAL_FRESH_OUTPUT and NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED drop the pre-pass over the
 * queries that this needs: the report is the same, the rows at and after the failing row are then unspecified.
 * Refused before any device work: a null `h`, with nq > 0 a null `qx`, `qy` or `out`, a stride below lanes,
 * NDI_PATH_BUCKETED, unknown flag bits or a non-zero `reserved` (all NDI_BAD_ARG); async_launch != 0 is NDI_UNSUPPORTED
 * (the finish record carries no element index).  nq == 0 is NDI_OK and touches nothing.
 * Host arrays go through device staging in row chunks of 256 MiB per array; only rows before the failing row are copied
 * back.  A Bicubic handle may keep a node-record copy of its node table for this call ({z, zx, zy, zxy} of a node and lane
 * side by side: built on the first lane-wise call that wants it, the size of the node table and at most 1 GiB, shared
 * with the partial handles as the node table is, released by ndi_interp2d_trim; a clone builds its own).
 * Not provided: integral handles, the ring, the sharded calls, async_launch, integer and f16 / bf16 element types. */
ndi_status ndi_interp2d_eval_lanewise(const ndi_interp2d* h, const void* qx, const void* qy, uint64_t nq,
                                      uint64_t q_row_stride, void* out, uint64_t out_row_stride,
                                      const ndi_eval_opts* opts, ndi_oob_info* info);

/* Completes async_launch evaluations on `stream`: synchronises it and reports the
 * status of the last batch enqueued there. */
ndi_status ndi_interp1d_finish(const ndi_interp1d* h, void* stream, ndi_oob_info* info);
ndi_status ndi_interp2d_finish(const ndi_interp2d* h, void* stream, ndi_oob_info* info);

/* ---- chunked evaluation through a device-output ring ---------------------------------
 * Replaces Interp1D::interp_array (src/interp1d/mod.rs:197-211: allocate zeros(xs.shape ++ lanes), then the
 * query loop :326-343) for batches whose whole output does not fit, or need not stay, in device memory
 * (4096 lanes x 1e7 queries of f64 = 327.7 GB > 288 GB HBM).  The flattened queries are evaluated in chunks of
 * `chunk_queries` rows into a ring of `n_slots` device buffers; after a chunk's kernels are enqueued the
 * `consume` callback is called on the calling host thread with the chunk's location, and the slot is reused
 * n_slots chunks later.  Nothing is copied to the host.
 *
 * Slot hand-off is stream-ordered: a consumer that enqueues its work on chunk->stream needs nothing else and
 * returns NULL; a consumer that works on another stream records a hipEvent_t there when it is done with the slot
 * and returns it -- the library makes its stream wait for that event before the slot is overwritten.
 *
 * First-error semantics are the reference's: a range pre-pass over all queries finds the lowest failing flat
 * index F before any chunk is produced; exactly the rows [0, F) are produced (the last chunk is cut short),
 * then NDI_OUT_OF_BOUNDS / NDI_NAN_QUERY is returned with info filled in.  The call returns after the last
 * chunk's kernels (and the consumer's stream-ordered work) have completed.
 *
 * Internally the producer is a two-stream pipeline: the search + grouping of the next chunks run on a side stream the
 * handle owns while the previous ones are evaluated on opts->stream (event-ordered; a scratch set per chunk in
 * flight).  Everything the consumer can observe -- the chunk's rows and chunk->stream -- is on opts->stream.
 *
 * Group launches (1-D, rows of 256 16-byte vectors and more on the bucketed path).  While every consumer call so far
 * has returned NULL -- the slots are handed back stream-ordered, so all n_slots of them are free as far as
 * opts->stream is concerned -- up to min(n_slots, 4) consecutive chunks are evaluated by ONE kernel launch.  `consume`
 * is still called once per chunk, in order, after that chunk's kernels are enqueued (for a group: after the group's
 * launch), and chunk->stream is still opts->stream; what changes is only that the rows of chunk k may be written
 * together with those of the chunks that share its launch.  A consumer that works on another stream keeps its
 * overlap (chunk k+1 evaluated while it drains chunk k): it signals itself by returning an event, and from the first
 * non-NULL return on the rest of the call runs one chunk per launch, waiting for each slot's event as before.  A NULL
 * `consume` pointer counts as stream-ordered.  NDI_RING_GROUP=0 in the environment forces one chunk per launch. */
typedef struct ndi_ring_chunk {
  uint64_t index;      /* chunk number, 0, 1, ... */
  uint64_t q_begin;    /* flat index of the chunk's first query */
  uint64_t q_count;    /* rows produced in this chunk */
  void* out;           /* device pointer, T[q_count][row_stride] */
  uint64_t row_stride; /* elements */
  uint32_t slot;       /* ring slot the chunk lives in */
  uint32_t shard;      /* sharded evaluation: index of the handle (device) that produced the chunk; else 0 */
  void* stream;        /* hipStream_t the chunk's kernels were enqueued on */
} ndi_ring_chunk;

typedef void* (*ndi_ring_consumer)(void* user, const ndi_ring_chunk* chunk);

/* Ring layout.  slots[i] points at row 0 of slot i; row r of a chunk is at slots[i] + r * row_stride elements.
 * Slots may be separate buffers (row_stride >= lanes), but on MI355X the recommended layout is ONE allocation with
 * the slots interleaved row by row: slots[i] = base + i * lanes, row_stride = n_slots * lanes.  The rate at which
 * a kernel streams into a 32.8 GB extent depends on where that extent lies in physical memory (up to 27 %
 * between the slots of one allocation); striping every chunk over the whole ring removes the dependence
 * (DESIGN.md 4.3).  With slots == NULL the library owns the ring (allocated once per handle, kept until trim /
 * destroy) and uses exactly that layout: chunk->row_stride is then n_slots * max(row_stride, lanes). */
typedef struct ndi_ring_desc {
  void* const* slots;     /* n_slots device pointers, or NULL for a library-owned ring */
  uint32_t n_slots;       /* >= 1 */
  uint32_t reserved;
  uint64_t chunk_queries; /* rows per chunk */
  uint64_t row_stride;    /* elements between consecutive rows of a slot (>= lanes; 0 = lanes) */
} ndi_ring_desc;

ndi_status ndi_interp1d_eval_ring(const ndi_interp1d* h, const void* q, uint64_t nq,
                                  const ndi_ring_desc* ring, ndi_ring_consumer consume, void* user,
                                  const ndi_eval_opts* opts, ndi_oob_info* info);
/* Same for Interp2D::interp_array (src/interp2d/mod.rs:175-196, 287-307). */
ndi_status ndi_interp2d_eval_ring(const ndi_interp2d* h, const void* qx, const void* qy, uint64_t nq,
                                  const ndi_ring_desc* ring, ndi_ring_consumer consume, void* user,
                                  const ndi_eval_opts* opts, ndi_oob_info* info);

/* ---- sharded evaluation: one call, several devices -------------------------------------------------
 * The reference is single-threaded; its multi-worker shape is one interpolator driven from many threads over
 * contiguous blocks of the query array (benches/bench_interp1d.rs:49-79; rayon support "planned", README.md:16-18).
 * These calls are that shape below the host language: `handles` are n_shards replicas of one interpolator (same
 * knots / data / strategy; normally one per device, built with ndi_interp{1,2}d_create and desc.device = d), the
 * flattened query array is split into contiguous blocks -- shard i owns [lo_i, hi_i) = ndi_shard_bounds(nq, i,
 * n_shards), block sizes differ by at most one -- and every shard is evaluated by its own host thread on its
 * handle's device: shard 0 on the calling thread, shard i > 0 on the i-th persistent worker thread the library keeps
 * for that calling thread (so a handle's per-thread scratch is reused from call to call, and concurrent sharded calls
 * from different host threads do not share workers).  No device-to-device traffic, no collective.
 *
 * First-error semantics are the reference's serial loop (src/interp1d/mod.rs:326-343, src/interp2d/mod.rs:287-307)
 * over the WHOLE batch: every shard range-checks its block first, the shards agree on the minimum failing flat
 * index F at a host barrier, and exactly the rows [0, F) are produced -- rows at or after F are never written, in
 * any shard.  info->index is the global flat index.
 *
 * ndi_shard_io (one per shard):
 *   q / qy  NULL: the shard reads its block of the flattened q (qx, qy) -- these are then host arrays or memory
 *           every device can read; non-NULL: the shard's own block (hi_i - lo_i queries), e.g. already resident on
 *           the shard's device.  Memory space of either form: opts->q_memspace.
 *   out     the shard's rows, T[hi_i - lo_i][out_row_stride], memory space opts->out_memspace (device pointers
 *           belong to the shard's device).  For one host output array: out = base + lo_i * out_row_stride.
 *   stream  hipStream_t on the shard's device (NULL = its default stream); opts->stream is ignored.
 * The handles must be distinct.  opts->async_launch is ignored (the call returns when every shard has finished).
 * Integer (i32 / i64) handles: the shards are visited one after another from the calling thread (no worker threads),
 * so a multi-device integer batch does not overlap across devices; results and first-error semantics are the same. */
typedef struct ndi_shard_io {
  const void* q;
  const void* qy;
  void* out;
  void* stream;
} ndi_shard_io;

void ndi_shard_bounds(uint64_t nq, uint32_t shard, uint32_t n_shards, uint64_t* lo, uint64_t* hi);

ndi_status ndi_interp1d_eval_sharded(const ndi_interp1d* const* handles, uint32_t n_shards, const void* q,
                                     uint64_t nq, const ndi_shard_io* io, uint64_t out_row_stride,
                                     const ndi_eval_opts* opts, ndi_oob_info* info);
ndi_status ndi_interp2d_eval_sharded(const ndi_interp2d* const* handles, uint32_t n_shards, const void* qx,
                                     const void* qy, uint64_t nq, const ndi_shard_io* io, uint64_t out_row_stride,
                                     const ndi_eval_opts* opts, ndi_oob_info* info);

/* The same through one device-output ring per shard (rings[i] on handles[i]'s device; slots == NULL: the handle
 * owns it): what ndi_interp{1,2}d_eval_ring is to one device.  `io` may be NULL (out is unused).  `consume` is
 * called from the shards' host threads CONCURRENTLY (once per chunk, in order within a shard); chunk->shard names
 * the shard, chunk->q_begin is the global flat index of the chunk's first query, chunk->index counts within the
 * shard.  Exactly the rows [0, F) are handed out. */
ndi_status ndi_interp1d_eval_ring_sharded(const ndi_interp1d* const* handles, uint32_t n_shards, const void* q,
                                          uint64_t nq, const ndi_shard_io* io, const ndi_ring_desc* rings,
                                          ndi_ring_consumer consume, void* user, const ndi_eval_opts* opts,
                                          ndi_oob_info* info);
ndi_status ndi_interp2d_eval_ring_sharded(const ndi_interp2d* const* handles, uint32_t n_shards, const void* qx,
                                          const void* qy, uint64_t nq, const ndi_shard_io* io,
                                          const ndi_ring_desc* rings, ndi_ring_consumer consume, void* user,
                                          const ndi_eval_opts* opts, ndi_oob_info* info);

/* Per-(stream, host thread) scratch is cached on the handle (at most 16 idle sets are kept; the least recently
 * used idle set is freed beyond that).  trim frees every idle set and a library-owned ring now. */
ndi_status ndi_interp1d_trim(const ndi_interp1d* h);
ndi_status ndi_interp2d_trim(const ndi_interp2d* h);
/* Diagnostic: number of scratch sets currently cached on the handle. */
uint64_t ndi_interp1d_scratch_sets(const ndi_interp1d* h);

/* ---- helpers on the path ------------------------------------------------------ */
/* VectorExtensions::get_lower_index (src/vector_extensions.rs:55-111), batched:
 * out_idx[i] = the unique j with knots[j] <= q[i] < knots[j+1], clamped to [0, n-2];
 * -1 for a NaN query.  Device search (wavefront-cooperative, knots in LDS). */
ndi_status ndi_get_lower_index_batch(int32_t dtype, int32_t device, const void* knots, uint64_t n,
                                     const void* q, uint64_t nq, int64_t* out_idx,
                                     int32_t memspace);

/* The same search with the knot pyramid resident on the device (no per-call allocation or knot upload):
 * what Interp1D::get_index_left_of (src/interp1d/mod.rs:380-382) is to a built interpolator.
 * `stream` as in ndi_eval_opts; the call returns when out_idx is complete. */
typedef struct ndi_locator ndi_locator;
ndi_status ndi_locator_create(int32_t dtype, int32_t device, const void* knots, uint64_t n,
                              int32_t memspace, ndi_locator** out);
ndi_status ndi_locator_eval(const ndi_locator* h, const void* q, uint64_t nq, int64_t* out_idx,
                            int32_t memspace, void* stream);
void ndi_locator_destroy(ndi_locator* h);

/* VectorExtensions::monotonic_prop (src/vector_extensions.rs:40-53, 116-198).
 * Host-side O(n) validation; returns an ndi_monotonic. */
int32_t ndi_monotonic_prop(int32_t dtype, const void* host_v, uint64_t n);

/* Interp1DBuilder::build / Interp2DBuilder::build checks alone (host). */
ndi_status ndi_validate1d(int32_t dtype, const void* host_x, uint64_t x_len, uint64_t n,
                          int32_t strategy);
ndi_status ndi_validate2d(int32_t dtype, const void* host_x, uint64_t x_len, const void* host_y,
                          uint64_t y_len, uint64_t nx, uint64_t ny);

/* ---- library-owned output buffers ---------------------------------------------------------------------------
 * Replaces the `Array::zeros(..)` of Interp1D::interp_array / Interp2D::interp_array (src/interp1d/mod.rs:204-209,
 * src/interp2d/mod.rs:183-188): a device buffer of `bytes` zero bytes for a batch's output rows.  On MI355X the rate at
 * which rows stream into a multi-gigabyte buffer depends on the physical pages behind it (4.6 .. 6.1 ms per 1e6 queries of
 * BASELINE configs[1] into buffers allocated one after the other; a property of the buffer, not of order or warm-up), so
 * the zero fill -- done the way the evaluation writes, whole 32 KiB rows at scattered positions: a sequential fill is blind
 * to the difference -- is timed and a slowly filling buffer is set aside for another candidate, up to `max_tries` (0 = as many as
 * fit into half of the free memory, 2 .. 8; buffers under 1 GiB: 1), while the device has room; the best candidate is returned, the others are freed.  `info` (may be NULL)
 * reports what happened.  Free with ndi_output_free (NDI_BAD_ARG for any other pointer).  The mirrors' interp_array uses
 * it for device outputs of >= 1 GiB; interp_array_into never allocates.
 * ndi_output_free keeps up to two freed buffers of >= 1 GiB (together at most a third of the device's memory) for the next
 * request of the same size on the same device -- a fresh 32.8 GB allocation costs the allocator 0.7-1.4 s, a caller that
 * evaluates batch after batch would pay it on every call -- and ndi_output_alloc hands such a buffer out again, zeroed
 * (info->tries == 0).  ndi_output_trim releases the kept buffers.
 * `flags` = NDI_OUTPUT_UNINITIALIZED: the contents are unspecified -- for a caller that overwrites every row it will read, as
 * interp_array does (the buffer is dropped on Err, src/interp1d/mod.rs:210): a kept buffer then goes out without the refill
 * (zeroing 32.8 GB costs what evaluating into it costs); new candidates are still filled, the fill being the measurement.
 * ndi_output_free waits for the device before it keeps a buffer, as hipFree does before it releases one. */
typedef enum ndi_output_flags {
  NDI_OUTPUT_ZEROED = 0,
  NDI_OUTPUT_UNINITIALIZED = 1
} ndi_output_flags;
typedef struct ndi_output_info {
  uint32_t tries;          /* candidates allocated and filled (0: a buffer kept by ndi_output_free was reused) */
  uint32_t reserved;
  double fill_tbps;        /* zero-fill rate of the buffer returned, TB/s */
  double worst_fill_tbps;  /* ... of the slowest candidate seen */
  double alloc_ms;         /* wall time of the whole call */
} ndi_output_info;
ndi_status ndi_output_alloc(int32_t device, uint64_t bytes, uint32_t max_tries, uint32_t flags, void** out,
                            ndi_output_info* info);
ndi_status ndi_output_free(void* p);
ndi_status ndi_output_trim(void);

/* ---- runtime ------------------------------------------------------------------ */
int32_t ndi_device_count(void);
const char* ndi_last_error_string(void);
uint32_t ndi_version(void); /* (major << 16) | minor */

/* Per-kernel HIP-event timing of the evaluation stages, recorded on the stream the
 * kernels run on.  Enable, run evaluations, then read (read synchronises the events). */
typedef struct ndi_profile {
  uint64_t eval_launches;   /* dominant kernel: gather / bucketed evaluation */
  double eval_ms;           /* summed duration of those launches */
  uint64_t locate_launches; /* per-query search kernel */
  double locate_ms;
  uint64_t group_launches;  /* bucketed path only: count + scan + scatter kernels */
  double group_ms;
  int32_t last_path;        /* ndi_path actually taken by the last evaluation */
  int32_t reserved;
} ndi_profile;
void ndi_profile_enable(int32_t on);
ndi_status ndi_profile_read(ndi_profile* out, int32_t reset);

/* Measurement aid for the 2-D gather (Bilinear::interp_into, bilinear.rs:83-97): runs the evaluation kernel's memory
 * access mix alone -- per query one uniformly random cell of the handle's own grid, the four corner vectors with
 * the kernel's lane mapping, the output row stored; no searches, knots or query values -- `reps` times and returns
 * the median launch duration in *ms.  `out`: device buffer T[nq][out_row_stride] (overwritten with meaningless
 * values).  The ceiling the memory system sets for this gather on this box: bench.py reports the evaluation
 * kernel against it next to the fraction of the HBM spec peak. */
ndi_status ndi_interp2d_probe_ceiling(const ndi_interp2d* h, uint64_t nq, void* out, uint64_t out_row_stride,
                                      void* stream, int32_t reps, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* NDINTERP_H */
