/* examples/c_abi_tricubic.c -- the Tricubic strategy of the C ABI (include/ndinterp3d_cubic.h) from plain C99.
 * Builds a Tricubic interpolator on a 4 x 5 x 4 grid of the cubic polynomial
 *     f(x, y, z) = (1 + x^3) (2 - y + y^2) (1 + z - z^3)
 * from host arrays with the default (not-a-knot) ends -- a not-a-knot spline reproduces a cubic, so the tensor-product
 * spline is the polynomial -- evaluates five points into a host buffer, checks them against the polynomial and prints them,
 * reads the fxyz table back and checks one node of it, then shows the first-error report; exits non-zero on any error.
 * Link: -lndinterp_hip (needs an MI355X at run time).
 *
 *   gcc -std=c99 -Wall -pedantic examples/c_abi_tricubic.c -Iinclude -Lndarray-interp_amd -lndinterp_hip
 */
#include <stdio.h>
#include <string.h>

#include "ndinterp3d_cubic.h"

static double fx_(double x) { return 1.0 + x * x * x; }
static double fy_(double y) { return 2.0 - y + y * y; }
static double fz_(double z) { return 1.0 + z - z * z * z; }
static double absd(double v) { return v < 0.0 ? -v : v; }

int main(void) {
  const double x[4] = {0.0, 0.5, 1.5, 2.0};
  const double y[5] = {-1.0, -0.25, 0.0, 0.5, 1.0};
  const double z[4] = {0.0, 1.0, 1.25, 2.0};
  double grid[4 * 5 * 4];
  double fxyz[4 * 5 * 4];
  void* tables[7] = {NULL, NULL, NULL, NULL, NULL, NULL, NULL};
  double qx[5] = {0.0, 0.25, 1.0, 2.0, 1.75};
  double qy[5] = {-1.0, -0.5, 0.25, 1.0, 0.0};
  double qz[5] = {0.0, 0.5, 1.125, 2.0, 1.5};
  double out[5];
  int i, j, k;
  ndi_interp3d_desc d;
  ndi_interp3d* h = NULL;
  ndi_eval_opts opts;
  ndi_oob_info info;
  ndi_status st;

  for (i = 0; i < 4; ++i)
    for (j = 0; j < 5; ++j)
      for (k = 0; k < 4; ++k) grid[(i * 5 + j) * 4 + k] = fx_(x[i]) * fy_(y[j]) * fz_(z[k]);
  memset(&d, 0, sizeof d);
  d.dtype = NDI_F64;
  d.nx = 4; d.ny = 5; d.nz = 4; d.lanes = 1;
  d.x_len = 4; d.y_len = 5; d.z_len = 4;
  d.x = x; d.y = y; d.z = z; d.data = grid;
  d.memspace = NDI_MEM_HOST;
  d.validate = 1;
  st = ndi_interp3d_create_tricubic(&d, NULL, &h);   /* NULL: NotAKnot on all six ends */
  if (st != NDI_OK) { fprintf(stderr, "create: %d %s\n", (int)st, ndi_last_error_string()); return 1; }
  memset(&opts, 0, sizeof opts);   /* host queries, host output, default stream */
  memset(&info, 0, sizeof info);
  st = ndi_interp3d_eval(h, qx, qy, qz, 5, out, 1, &opts, &info);
  if (st != NDI_OK) { fprintf(stderr, "eval: %d %s\n", (int)st, ndi_last_error_string()); return 2; }
  for (i = 0; i < 5; ++i) {
    const double want = fx_(qx[i]) * fy_(qy[i]) * fz_(qz[i]);
    if (absd(out[i] - want) > 1e-12 * (1.0 + absd(want))) {
      fprintf(stderr, "point %d: %.17g, the polynomial is %.17g\n", i, out[i], want);
      return 3;
    }
    printf("%.17g\n", out[i]);
  }
  /* the seventh table, d3 f / dx dy dz at the nodes: 3 x^2 (2 y - 1) (1 - 3 z^2) */
  tables[6] = fxyz;
  st = ndi_interp3d_tables(h, tables, NDI_MEM_HOST);
  if (st != NDI_OK) { fprintf(stderr, "tables: %d %s\n", (int)st, ndi_last_error_string()); return 4; }
  {
    const double want = 3.0 * x[2] * x[2] * (2.0 * y[4] - 1.0) * (1.0 - 3.0 * z[1] * z[1]);
    const double got = fxyz[(2 * 5 + 4) * 4 + 1];
    if (absd(got - want) > 1e-11 * (1.0 + absd(want))) {
      fprintf(stderr, "fxyz[2][4][1]: %.17g, the polynomial's is %.17g\n", got, want);
      return 5;
    }
  }
  /* the lowest failing query wins, x before y before z within it: query 3 leaves the z axis */
  qz[3] = 2.5;
  st = ndi_interp3d_eval(h, qx, qy, qz, 5, out, 1, &opts, &info);
  if (st != NDI_OUT_OF_BOUNDS || info.index != 3 || info.axis != 2) {
    fprintf(stderr, "first error: %d %s\n", (int)st, ndi_last_error_string());
    return 6;
  }
  ndi_interp3d_destroy(h);
  return 0;
}
