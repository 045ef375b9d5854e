/* include/ndinterp3d_cubic.h -- the Tricubic strategy of the 3-D handles of libndinterp_hip.so (MI355X / gfx950): the
 * tensor-product cubic spline on a rectilinear grid, C2 in each variable (scipy: RegularGridInterpolator(method="cubic")
 * with a direct solver, for the default ends; the reference interpolates along one or two axes).
 *
 * include/ndinterp.h and include/ndinterp3d.h are frozen lists, so the cubic part of the 3-D interface has a header of its
 * own.  It adds to ndinterp3d.h and changes nothing in it: ndi_interp3d, ndi_interp3d_desc, ndi_interp3d_eval, _clone and
 * _destroy are those of ndinterp3d.h and take a Tricubic handle as they are; ndi_boundary and ndi_bc_kind are those of
 * ndinterp.h.  The functions live in the same shared object and ndi_version() is unchanged.  The conventions hold here too:
 * plain C, every call returns an ndi_status with the text in ndi_last_error_string(), arrays are C-order and contiguous,
 * every pointer carries a memory space, and there is NO CPU fallback.
 */
#ifndef NDINTERP3D_CUBIC_H
#define NDINTERP3D_CUBIC_H

#include "ndinterp3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Builds a Tricubic handle from the descriptor of ndi_interp3d_create (dtype NDI_F32 / NDI_F64, any lanes) and six end
 * conditions `bc`, one ndi_boundary of any ndi_bc_kind per end in the order x-left, x-right, y-left, y-right, z-left,
 * z-right; a NULL `bc` is NotAKnot on all six.  Per-lane and periodic ends have no encoding.
 *
 * Numerical contract -- this project's own.  T in {f32, f64}, data f[nx][ny][nz][C], axes x[nx], y[ny], z[nz], at least 3
 * knots each.  Every line is one IEEE operation in T, in this order, nothing fused, nothing re-associated.
 *  Node derivatives.  D_a g is the knot derivative of the 1-D spline through g along axis a, exactly a pass of the Bicubic
 *  contract (ndinterp.h, ndi_interp2d_create_bicubic): the CubicSpline coefficient build with the axis' knots on g viewed as
 *  (n_a, everything else), in the REFERENCE operation order (NDI_BUILD_REFERENCE_ORDER) with the TRUE not-a-knot right row
 *  (x[n-2] - x[n-3] on the last diagonal entry, where cubic_spline.rs:635 has x[n-1] - x[n-2]); n == 3 with both ends
 *  NotAKnot takes the build's parabola branch; giving a, b; then ndi_interp1d_derivative's rule per column, with
 *  dg = g[i+1] - g[i], dx = x[i+1] - x[i]:
 *         Y[i]   = (dg + a[i]) / dx        i < n-1
 *         Y[n-1] = (dg - b[n-2]) / dx      with i = n-2
 *  Seven tables of the data's shape, in this order of derivation:
 *         fx   = D_x f          fy   = D_y f          fz   = D_z f
 *         fxy  = D_y fx         fxz  = D_z fx         fyz  = D_z fy
 *         fxyz = D_z fxy
 *  A pass on f takes the axis' two ends as given; a pass on a derivative table takes the same end KINDS with value 0 (the
 *  derivative, along another axis, of a constant end value) -- Bicubic's cross-pass rule.  Lanes, and the columns of a pass,
 *  are independent and run identical operations: the bits do not depend on how the build lays its columns out.
 *  Evaluation.  The cells i, j, k are those of ndi_interp3d_eval: the largest index with knot <= q, clamped to [0, n - 2], so
 *  the end patch continues under `extrapolate`.
 *         hx = x[i+1] - x[i];  t = (qx - x[i]) / hx        hy, u from (y, j, qy) and hz, w from (z, k, qz) likewise
 *         H(pl, pr, kl, kr, h, s):  d = pr - pl;  a = kl h - d;  b = d - kr h;
 *                                   (1-s) pl + s pr + s (1-s) (a (1-s) + b s)        (the Bicubic contract's H)
 *  Twenty-one H per lane, z first, then y, then x.  With i' in {i, i+1}, j' in {j, j+1}:
 *         Zf  [i'][j'] = H(f  [i'][j'][k], f  [i'][j'][k+1], fz  [i'][j'][k], fz  [i'][j'][k+1], hz, w)
 *         Zfx [i'][j'] = H(fx [i'][j'][k], fx [i'][j'][k+1], fxz [i'][j'][k], fxz [i'][j'][k+1], hz, w)
 *         Zfy [i'][j'] = H(fy [i'][j'][k], fy [i'][j'][k+1], fyz [i'][j'][k], fyz [i'][j'][k+1], hz, w)
 *         Zfxy[i'][j'] = H(fxy[i'][j'][k], fxy[i'][j'][k+1], fxyz[i'][j'][k], fxyz[i'][j'][k+1], hz, w)        (16 forms)
 *         P[i'] = H(Zf [i'][j], Zf [i'][j+1], Zfy [i'][j], Zfy [i'][j+1], hy, u)
 *         Q[i'] = H(Zfx[i'][j], Zfx[i'][j+1], Zfxy[i'][j], Zfxy[i'][j+1], hy, u)                                  (4 forms)
 *         out   = H(P[i], P[i+1], Q[i], Q[i+1], hx, t)
 *  Whatever kernel form, vector width or search is taken, these are the bits (tests/tricubic_ref.py restates them).
 *  On the default ends this is scipy's RegularGridInterpolator(method="cubic") solved directly, and its "cubic_legacy", up to
 *  rounding (DESIGN.md 4.27 has the figures); scipy's default iterative solver is itself only good to about 1e-5.
 *
 * Range, NaN, errors, buffer state and refusals of an evaluation are ndi_interp3d_eval's, unchanged.
 *
 * Refused before any device work, with *out cleared where there is one: what ndi_interp3d_create refuses (NDI_BAD_ARG: a
 * null `desc` or `out`, a dtype other than NDI_F32 / NDI_F64, a non-zero `reserved`), and with NDI_BAD_ARG any boundary
 * kind outside ndi_bc_kind.  validate != 0 with host axes runs the builder's checks of ndi_interp3d_create on the host, in
 * its order, with 3 knots required per axis (NDI_NOT_ENOUGH_DATA "... Provided: 2, Reqired: 3"), so they answer on a machine
 * without a device; with device axes they run after the axes have been fetched; validate == 0 trusts the caller, and
 * inconsistent sizes are still NDI_BAD_ARG.  Without a usable device the call then fails with NDI_HIP_ERROR
 * ("... no CPU fallback").
 *
 * Device memory kept: the three axes and the node table T[nx][ny][nz][8][C] -- f and the seven derivative tables, eight
 * times the grid; the plain grid is not kept.  During create the peak is about 14 grids: the table, three work grids (the
 * source of a pass, its transposed copy, its result) and the temporary 1-D spline of the running pass (about three).  All
 * temporaries are freed before create returns, and the table is complete on return: any stream may evaluate at once.
 *
 * Not provided: partial-derivative handles and a jet; periodic axes; Pchip, Akima and caller-given node derivatives; the
 * ring, the sharded calls, async_launch; integer and f16 / bf16 element types; lane-wise evaluation; a tile-grouped order. */
ndi_status ndi_interp3d_create_tricubic(const ndi_interp3d_desc* desc, const ndi_boundary* bc, ndi_interp3d** out);

/* The seven derivative tables of a Tricubic handle as plain T[nx][ny][nz][lanes] arrays in `memspace`, in the order
 * fx, fy, fz, fxy, fxz, fyz, fxyz.  Any entry of `tables` may be NULL and is skipped.  NDI_BAD_ARG: a null `h` or `tables`,
 * an unknown memspace, and a Trilinear handle (it keeps no node derivatives).  This mirrors ndi_interp2d_tables. */
ndi_status ndi_interp3d_tables(const ndi_interp3d* h, void* const tables[7], int32_t memspace);

#ifdef __cplusplus
}
#endif

#endif /* NDINTERP3D_CUBIC_H */
