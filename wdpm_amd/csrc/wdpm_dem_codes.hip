/*
 * wdpm_dem_codes.hip — the DEM just uploaded as verified codes (wdpm_kernels.h::DemCode): the search for a grid on the host, every
 * check on the device.  One unit of the context layer (wdpm_ctx.h); wdpm_capi.hip's uploads call encode_dem.
 */
#include <cmath>

#include "wdpm_ctx.h"

/* One attempt at the grid D: codes q with dem == (q + k0) / D, checked by the device on every cell with the decoder the
 * iteration kernels use.  *ok says whether every cell came back bit for bit; the codes are then in charge. */
static int try_dem_grid(wdpm_ctx *x, double k0, double D, double rD, double rDlo, int force, bool *ok) {
  HIP_TRY(wdpm_launch_dem_encode(x->d_dem, x->cells, k0, D, rD, rDlo, x->d_dem32, x->d_bits, x->stream));
  unsigned long long bad;
  if (read_back(x, x->d_bits, &bad, sizeof bad)) return 1;
  *ok = !bad;
  if (!bad) {
    x->dem32_encodable = true;
    x->code = DemCode{x->d_dem32, k0, D, rD, rDlo, force, nullptr, nullptr, 0};
  }
  return 0;
}

/* Try to express the DEM just uploaded as 32-bit codes k with dem == (k + k0) / D bit for bit.  First D = 10^e (e = 0..6, the
 * smallest that works: DEMs read from decimal text), then once D = 2^s with 2^-s the weight of the lowest bit set in any
 * elevation (DEMs that were binary all along: a Float32 raster around 500 m lies on 2^-15 m).  The device checks every cell
 * with the decoder the iteration kernel uses; any miss leaves the fp64 DEM in charge. */
int encode_dem(wdpm_ctx *x) {
  drop_graphs(x);
  /* every level starts from "not encodable": a DEM uploaded over an earlier one inherits nothing (a smooth DEM, then a
   * rough one that passes only the 32-bit check, left dem16_encodable set and d_dem16 holding truncated offsets) */
  x->dem32_encodable = false; x->dem16_encodable = false; x->dem_bounded = false; x->dem16_wanted = true;
  x->dem_grid = x->dem_grid_exp = 0;
  x->code = kNoCodes;
  HIP_TRY(wdpm_launch_dem_min(x->d_dem, x->cells, x->d_bits, x->stream));
  unsigned long long v[3];
  if (read_back(x, x->d_bits, v, sizeof v)) return 1;
  const unsigned long long key = v[0], amax = v[1], low = v[2];
  x->dem_bounded = amax < 0x41d0000000000000ull;               /* |dem| < 2^30 on every valid cell (none at all: 0) */
  const char *env = getenv("WDPM_DEM32");
  if (env && atoi(env) == 0) return 0;
  if (key == ~0ull) return 0;                                  /* no valid cell at all */
  const double vmin = wdpm_dem_key_to_double(key);
  const int force = (env && atoi(env) == 2) ? 1 : 0;           /* WDPM_DEM32=2: on launches of any size */
  static const double p10[7] = {1.0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6};
  for (int e = 0; e <= 6; e++) {
    const double D = p10[e], rD = 1.0 / D, k0 = rint(vmin * D);
    /* the reciprocal's second word: 1 - rD * D is exact in one FMA (|.| < 2^-52 on the grid of the product's last bit), so the one
     * rounding of the division makes this RN(1 / D - rD) */
    const double rDlo = fma(-rD, D, 1.0) / D;
    if (!(fabs(k0) < 4.0e15)) break;                           /* k = q + k0 must stay an exact integer */
    bool ok;
    if (try_dem_grid(x, k0, D, rD, rDlo, force, &ok)) return 1;
    if (ok) {
      x->dem_grid = 10;
      x->dem_grid_exp = e;
      break;
    }
  }
  /* no decimal grid: one attempt at the binary grid the elevations themselves name.  2^-s is the coarsest power of two all of
   * them are multiples of (zeros lie on every grid), so vmin * 2^s is an exact integer and rD = 2^-s needs no second word.
   * s <= 52: a finer grid cannot hold real terrain in 31 bits of relief, and D stays finite whatever vmin is; s >= 1: an
   * integer grid was e = 0's to take.  WDPM_DEM_BINARY=0: never (the decimal grids alone, for A/B runs) */
  const char *envb = getenv("WDPM_DEM_BINARY");
  if (!x->dem32_encodable && low != ~0ull && !(envb && atoi(envb) == 0)) {
    const long long s = 1075 - (long long)low;
    if (s >= 1 && s <= 52) {
      const double D = ldexp(1.0, (int)s), rD = ldexp(1.0, -(int)s), k0 = rint(vmin * D);
      if (fabs(k0) < 4.0e15) {
        bool ok;
        if (try_dem_grid(x, k0, D, rD, 0.0, force, &ok)) return 1;
        if (ok) {
          x->dem_grid = 2;
          x->dem_grid_exp = (int)s;
        }
      }
    }
  }
  /* second level: the codes as 16-bit offsets from one base per 48 columns of a row - where the terrain allows it (WDPM_DEM16=0: never) */
  const char *env16 = getenv("WDPM_DEM16");
  if (x->dem32_encodable && !(env16 && atoi(env16) == 0)) {
    const int ngroups = dem_groups(x->g.ncp);
    HIP_TRY(wdpm_launch_dem16_encode(x->code, x->g.rows, x->g.ncp, ngroups, x->d_dem16, x->d_gbase, x->d_bits, x->stream));
    unsigned long long bad;
    if (read_back(x, x->d_bits, &bad, sizeof bad)) return 1;
    if (!bad) {
      x->dem16_encodable = true;
      x->code.h = x->d_dem16;
      x->code.gb = x->d_gbase;
      x->code.ngroups = ngroups;
    }
  }
  return 0;
}
