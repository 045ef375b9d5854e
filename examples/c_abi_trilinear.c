/* examples/c_abi_trilinear.c -- the 3-D part of the C ABI (include/ndinterp3d.h) from plain C99.
 * Builds a Trilinear interpolator on a 3 x 3 x 3 grid of f(x, y, z) = 1 + 2x - 3y + 0.5z from host arrays, evaluates five
 * points into a host buffer and prints them (a trilinear interpolant reproduces an affine function), then shows the
 * first-error report; exits non-zero on any error.  Link: -lndinterp_hip (needs an MI355X at run time).
 *
 *   gcc -std=c99 -Wall -pedantic examples/c_abi_trilinear.c -Iinclude -Lndarray-interp_amd -lndinterp_hip
 */
#include <stdio.h>
#include <string.h>

#include "ndinterp3d.h"

int main(void) {
  const double x[3] = {0.0, 1.0, 3.0};
  const double y[3] = {-1.0, 0.0, 0.5};
  const double z[3] = {0.0, 2.0, 4.0};
  double grid[27];
  double qx[5] = {0.0, 0.5, 2.0, 3.0, 1.25};
  double qy[5] = {-1.0, -0.5, 0.25, 0.5, 0.0};
  double qz[5] = {0.0, 1.0, 3.0, 4.0, 2.5};
  double out[5];
  int i, j, k;
  ndi_interp3d_desc d;
  ndi_interp3d* h = NULL;
  ndi_eval_opts opts;
  ndi_oob_info info;
  ndi_status st;

  for (i = 0; i < 3; ++i)
    for (j = 0; j < 3; ++j)
      for (k = 0; k < 3; ++k) grid[(i * 3 + j) * 3 + k] = 1.0 + 2.0 * x[i] - 3.0 * y[j] + 0.5 * z[k];
  memset(&d, 0, sizeof d);
  d.dtype = NDI_F64;
  d.nx = 3; d.ny = 3; d.nz = 3; d.lanes = 1;
  d.x_len = 3; d.y_len = 3; d.z_len = 3;
  d.x = x; d.y = y; d.z = z; d.data = grid;
  d.memspace = NDI_MEM_HOST;
  d.validate = 1;
  st = ndi_interp3d_create(&d, &h);
  if (st != NDI_OK) { fprintf(stderr, "create: %d %s\n", (int)st, ndi_last_error_string()); return 1; }
  memset(&opts, 0, sizeof opts);   /* host queries, host output, default stream */
  memset(&info, 0, sizeof info);
  st = ndi_interp3d_eval(h, qx, qy, qz, 5, out, 1, &opts, &info);
  if (st != NDI_OK) { fprintf(stderr, "eval: %d %s\n", (int)st, ndi_last_error_string()); return 2; }
  for (i = 0; i < 5; ++i) printf("%.17g\n", out[i]);
  /* the lowest failing query wins, x before y before z within it: query 3 leaves the z axis */
  qz[3] = 4.5;
  st = ndi_interp3d_eval(h, qx, qy, qz, 5, out, 1, &opts, &info);
  if (st != NDI_OUT_OF_BOUNDS || info.index != 3 || info.axis != 2) {
    fprintf(stderr, "first error: %d %s\n", (int)st, ndi_last_error_string());
    return 3;
  }
  ndi_interp3d_destroy(h);
  return 0;
}
