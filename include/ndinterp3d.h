/* include/ndinterp3d.h -- the 3-D part of the C ABI of libndinterp_hip.so (MI355X / gfx950): Interp3D with the
 * Trilinear strategy, this project's own (the reference interpolates along one or two axes; scipy:
 * RegularGridInterpolator(method="linear"), MATLAB: interp3).
 *
 * The 3-D interface has a header of its own because include/ndinterp.h is a frozen list: the Rust shim and the
 * Python symbol table bind exactly the functions and handle types it declares.  This header adds to it and changes
 * nothing in it: ndi_status, ndi_dtype, ndi_memspace, ndi_eval_opts, ndi_eval_flags and ndi_oob_info are those of
 * ndinterp.h, the library is the same shared object, and ndi_version() is unchanged.  Its conventions hold here too:
 * plain C, every call returns an ndi_status with the text in ndi_last_error_string(), arrays are C-order and
 * contiguous, every pointer carries a memory space, and there is NO CPU fallback.
 */
#ifndef NDINTERP3D_H
#define NDINTERP3D_H

#include "ndinterp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ndi_interp3d ndi_interp3d; /* owns device copies of x, y, z and the grid */

/* Interp3DBuilder::{new,x,y,z,strategy,build} of the Python mirror; the 2-D descriptor taken one axis further.
 * Device memory: the three axes and one copy of the grid. */
typedef struct ndi_interp3d_desc {
  int32_t dtype;        /* NDI_F32 / NDI_F64 only */
  int32_t extrapolate;  /* Trilinear::extrapolate: the end cell of every axis continues */
  int32_t device;
  int32_t memspace;     /* of x, y, z, data */
  uint64_t nx, ny, nz;  /* data.shape()[0..3] */
  uint64_t lanes;       /* product of data.shape()[3..] */
  uint64_t x_len, y_len, z_len;
  const void* x;        /* T[x_len], or NULL for 0..nx (as ndi_interp2d_desc) */
  const void* y;        /* T[y_len], or NULL for 0..ny */
  const void* z;        /* T[z_len], or NULL for 0..nz */
  const void* data;     /* T[nx][ny][nz][lanes], lanes fastest */
  int32_t validate;     /* != 0: run the builder's checks here (below) */
  int32_t reserved;     /* 0 */
} ndi_interp3d_desc;

/* Builds a Trilinear handle.
 * Refused before any device work, with *out cleared where there is one (NDI_BAD_ARG): a null `desc` or `out`, a dtype
 * other than NDI_F32 / NDI_F64, a non-zero `reserved`.
 * validate != 0 with host axes runs the builder's checks on the host, so they answer on a machine without a device, in
 * the order of Interp2DBuilder::build (src/interp2d/mod.rs:480-509) with a third axis: nx, ny, nz below 2 is
 * NDI_NOT_ENOUGH_DATA ("The 2-dimension has not enough data ..."), then x_len != nx, y_len != ny, z_len != nz is
 * NDI_SHAPE ("Lenghts of z-axis and data-2-axis need to match ..."), then x, y, z not strictly rising is
 * NDI_MONOTONIC ("The z-axis needs to be strictly monotonic rising").  A NULL axis is 0..n and passes.  With device
 * axes the same checks run after the axes have been fetched.  validate == 0 trusts the caller; inconsistent sizes are
 * still NDI_BAD_ARG.  Without a usable device the call then fails with NDI_HIP_ERROR ("... no CPU fallback"). */
ndi_status ndi_interp3d_create(const ndi_interp3d_desc* desc, ndi_interp3d** out);

/* out[j][l] = f_l(qx[j], qy[j], qz[j]) for j < nq, l < lanes: every lane of the grid at one point per query.
 * `qx`, `qy`, `qz` are T[nq] in opts->q_memspace, `out` is T[nq][out_row_stride] in opts->out_memspace; the stride is in
 * elements and at least lanes.  opts->stream is honoured; NULL opts are the defaults (host arrays, default stream).
 *
 * Value rule.  Let i, j, k be the intervals the library's search finds on the three axes: the largest index with
 * knot <= q, clamped to [0, n - 2] (get_lower_index, vector_extensions.rs:55-111, with this project's stated fix for
 * nextbefore(k[n-1])).  With
 *     calc_frac((x1, y1), (x2, y2), x) = ((y2 - y1) / (x2 - x1)) * (x - x1) + y1        (linear.rs:29-36)
 * every line below is one IEEE operation per step in T, nothing fused and nothing re-associated -- the reference's
 * Bilinear order (bilinear.rs:94-96) continued by one axis:
 *     c00 = calc_frac((x1, d[i][j  ][k  ]), (x2, d[i+1][j  ][k  ]), x)     c01 = ... [j  ][k+1]
 *     c10 = calc_frac((x1, d[i][j+1][k  ]), (x2, d[i+1][j+1][k  ]), x)     c11 = ... [j+1][k+1]
 *     c0  = calc_frac((y1, c00), (y2, c10), y)                              c1  = calc_frac((y1, c01), (y2, c11), y)
 *     out = calc_frac((z1, c0), (z2, c1), z)
 * Equivalently: c0 and c1 are, bit for bit, what ndi_interp2d_eval writes for (x, y) on the Bilinear handles of the
 * slabs data[:, :, k] and data[:, :, k+1] (same x, y axes and extrapolation), and out is one calc_frac along z between
 * them.  Whatever kernel form, vector width or search is taken, these are the bits.
 *
 * Range and errors: those of ndi_interp2d_eval, extended by one axis.  Without `extrapolate` a coordinate outside
 * [k[0], k[n-1]] of its axis is NDI_OUT_OF_BOUNDS, and a NaN fails that test too; with `extrapolate` the end cell
 * continues and a NaN is NDI_NAN_QUERY.  The lowest failing query index wins; within one query x is reported before y
 * before z.  info->index is the query, info->axis 0, 1 or 2, info->value the offending coordinate; the text is
 * "x = ... is not in range" / "y = ..." / "z = ...".
 *
 * Buffer state.  By default (interp_array_into semantics: a caller-owned buffer) rows before the first failing query
 * are written and the failing row and all later rows are untouched.  NDI_EVAL_FRESH_OUTPUT and
 * NDI_EVAL_ROWS_AFTER_ERROR_UNSPECIFIED drop the pre-pass over the queries that this needs: the report is the same, the
 * rows at and after the failure are then unspecified.
 *
 * Refused before any device work (NDI_BAD_ARG): a null `h`; with nq > 0 a null query or output pointer;
 * out_row_stride < lanes; unknown flag bits or a non-zero `reserved`; NDI_PATH_BUCKETED (there is no tile-grouped
 * order).  async_launch != 0 is NDI_UNSUPPORTED.  nq == 0 is NDI_OK and touches nothing.
 *
 * Host arrays go through device staging in row chunks; only rows before the failing query are copied back.
 * Not provided: the ring, the sharded calls, async_launch, integer and f16 / bf16 element types, lane-wise
 * evaluation, a tile-grouped order, tricubic. */
ndi_status ndi_interp3d_eval(const ndi_interp3d* h, const void* qx, const void* qy, const void* qz, uint64_t nq,
                             void* out, uint64_t out_row_stride, const ndi_eval_opts* opts, ndi_oob_info* info);

/* A replica of the handle on `device`: axes and grid are copied device to device (what a replicate() needs).  A null
 * `h` or `out` is NDI_BAD_ARG (*out cleared where there is one). */
ndi_status ndi_interp3d_clone(const ndi_interp3d* h, int32_t device, ndi_interp3d** out);

/* Frees the handle and its device memory; ndi_interp3d_destroy(NULL) is a no-op. */
void ndi_interp3d_destroy(ndi_interp3d* h);

#ifdef __cplusplus
}
#endif

#endif /* NDINTERP3D_H */
