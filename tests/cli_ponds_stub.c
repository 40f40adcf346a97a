/* cli_ponds_stub.c - a canned pond back-end for the command line's pond files (tests/test_cli_pond_files.py): the pond symbols
 * wdpm_amd/csrc/wdpmcl_ponds.c refers to, answering with fixed tables, linked with the command line and the CPU restatement into
 * one program.  Nothing here looks at the raster: what is tested is the command line's side - which calls it makes, in which
 * order, and what it writes from what they return.
 *   STUB_N=<n>          ponds (default 3).  Pond 2 has no rim cell, no outlet and no curve; pond 1 has no land that drains to it
 *                       and volume_q / fill_q above 2^53
 *   STUB_TRACE=1        one "stub: <symbol>" line per call on stderr, with the min_depth of a label call
 *   STUB_FAIL=<symbol>  that call sets "<symbol> failed" as the last error and returns 1
 *   STUB_GUARD_BAD=<n>  what the guard calls report
 *   -DSTUB_UNITS=k      1..5 (default 5): the symbols of the units above k - rims, catchments, outlets, curves - stay undefined */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/wdpm.h"
#include "../include/wdpm_group_ponds.h"
#include "../include/wdpm_pond_catchments.h"
#include "../include/wdpm_pond_curves.h"
#include "../include/wdpm_pond_outlets.h"
#include "../include/wdpm_pond_rims.h"

#ifndef STUB_UNITS
#define STUB_UNITS 5
#endif

static int64_t env_int(const char *name, int64_t dflt) { return getenv(name) ? atoll(getenv(name)) : dflt; }
static int64_t stub_n(void) { return env_int("STUB_N", 3); }

/* trace the call; non-zero when it is the one to fail */
static int enter(const char *sym, const double *min_depth) {
  if (env_int("STUB_TRACE", 0)) {
    if (min_depth) fprintf(stderr, "stub: %s min_depth=%.17g\n", sym, *min_depth);
    else fprintf(stderr, "stub: %s\n", sym);
  }
  const char *fail = getenv("STUB_FAIL");
  if (!fail || strcmp(fail, sym) != 0) return 0;
  char msg[96];
  snprintf(msg, sizeof msg, "%s failed", sym);
  wdpm_set_last_error(msg);
  return 1;
}
#define ENTER(sym) do { if (enter(#sym, NULL)) return 1; } while (0)
#define LABEL(sym) do { if (enter(#sym, &min_depth)) return 1; *nponds = stub_n(); return 0; } while (0)
#define ROWS(sym) do { ENTER(sym); if (capacity < stub_n()) { wdpm_set_last_error(#sym ": capacity"); return 1; } } while (0)

/* distinct per pond k and column j, none of them short in binary */
static double val(int64_t k, int j) { return 500.0 + (double)(k + 1) * 0.37 + (double)j / 7.0; }
static uint64_t quanta(int64_t k, int j) { return k == 0 ? (1ull << 60) + 12345u + (unsigned)j : 123456789ull + 1000003ull * (uint64_t)k + (unsigned)j; }

static int handle, group_handle;
static wdpm_group *the_group;

int wdpm_ponds_create(wdpm_ponds **out, wdpm_ctx *ctx) { (void)ctx; ENTER(wdpm_ponds_create); *out = (wdpm_ponds *)&handle; return 0; }
void wdpm_ponds_destroy(wdpm_ponds *h) { (void)h; enter("wdpm_ponds_destroy", NULL); }
int wdpm_ponds_label(wdpm_ponds *h, double min_depth, int64_t *nponds) { (void)h; LABEL(wdpm_ponds_label); }
int wdpm_ponds_guard_bad(wdpm_ponds *h, int64_t *bytes) { (void)h; ENTER(wdpm_ponds_guard_bad); *bytes = env_int("STUB_GUARD_BAD", 0); return 0; }
static void fill_ponds(wdpm_pond *out) {
  for (int64_t k = 0; k < stub_n(); k++) {
    const int32_t r = (int32_t)(2 + 3 * k), c = (int32_t)(3 + 5 * k);
    out[k] = (wdpm_pond){r, c + 1, 11 + 7 * k, quanta(k, 0), val(k, 0) / 1000.0, r, r + 4, c, c + 6};
  }
}
int wdpm_ponds_table(wdpm_ponds *h, wdpm_pond *out, int64_t capacity) { (void)h; ROWS(wdpm_ponds_table); fill_ponds(out); return 0; }

int wdpm_group_ponds_create(wdpm_group_ponds **out, wdpm_group *grp) {
  ENTER(wdpm_group_ponds_create);
  the_group = grp;
  *out = (wdpm_group_ponds *)&group_handle;
  return 0;
}
void wdpm_group_ponds_destroy(wdpm_group_ponds *h) { (void)h; enter("wdpm_group_ponds_destroy", NULL); }
int wdpm_group_ponds_label(wdpm_group_ponds *h, double min_depth, int64_t *nponds) { (void)h; LABEL(wdpm_group_ponds_label); }
int wdpm_group_ponds_table(wdpm_group_ponds *h, wdpm_pond *out, int64_t capacity) { (void)h; ROWS(wdpm_group_ponds_table); fill_ponds(out); return 0; }
int wdpm_group_ponds_guard_bad(wdpm_group_ponds *h, int64_t *bytes) { (void)h; ENTER(wdpm_group_ponds_guard_bad); *bytes = env_int("STUB_GUARD_BAD", 0); return 0; }
int wdpm_group_ponds_stats(wdpm_group_ponds *h, wdpm_group_pond_stats *out) {
  (void)h;
  ENTER(wdpm_group_ponds_stats);
  *out = (wdpm_group_pond_stats){wdpm_group_size(the_group), stub_n(), stub_n() + 7, 9, 7, 0.25};
  return 0;
}

#if STUB_UNITS >= 2
int wdpm_rims_label(wdpm_ponds *h, double min_depth, int64_t *nponds) { (void)h; LABEL(wdpm_rims_label); }
int wdpm_rims_table(wdpm_ponds *h, wdpm_pond_rim *out, int64_t capacity) {
  (void)h;
  ROWS(wdpm_rims_table);
  for (int64_t k = 0; k < stub_n(); k++) {
    out[k] = (wdpm_pond_rim){val(k, 1), val(k, 2), val(k, 3), (int32_t)(4 + 3 * k), (int32_t)(9 + 5 * k), 21 + k, 5 + 2 * k};
    if (k == 1) { out[k].rim_level = INFINITY; out[k].rim_row = out[k].rim_col = -1; }
  }
  return 0;
}
#endif

#if STUB_UNITS >= 3
int wdpm_catch_label(wdpm_ponds *h, double min_depth, int64_t *nponds) { (void)h; LABEL(wdpm_catch_label); }
int wdpm_catch_table(wdpm_ponds *h, wdpm_pond_catchment *out, int64_t capacity) {
  (void)h;
  ROWS(wdpm_catch_table);
  for (int64_t k = 0; k < stub_n(); k++) {
    const int32_t r = (int32_t)(1 + 3 * k), c = (int32_t)(2 + 5 * k);
    out[k] = (wdpm_pond_catchment){k == 0 ? 0 : 101 + 13 * k, 3 * k, k == 0 ? -INFINITY : val(k, 4), r, r + 8, c, c + 9};
  }
  return 0;
}
int wdpm_catch_stats(wdpm_ponds *h, wdpm_pond_catchment_stats *out) {
  (void)h;
  ENTER(wdpm_catch_stats);
  *out = (wdpm_pond_catchment_stats){1111, 22, 333, 4, stub_n()};
  return 0;
}
#endif

#if STUB_UNITS >= 4
int wdpm_outlets_label(wdpm_ponds *h, double min_depth, int64_t *nponds) { (void)h; LABEL(wdpm_outlets_label); }
int wdpm_outlets_table(wdpm_ponds *h, wdpm_pond_outlet *out, int64_t capacity) {
  (void)h;
  ROWS(wdpm_outlets_table);
  for (int64_t k = 0; k < stub_n(); k++) {
    const int32_t r = (int32_t)(5 + 3 * k), c = (int32_t)(7 + 5 * k);
    out[k] = (wdpm_pond_outlet){val(k, 5), r, c, r + 1, c - 1, (int32_t)k / 2, 0, 31 + k, 41 + 9 * k, quanta(k, 1)};
    if (k == 1) out[k] = (wdpm_pond_outlet){INFINITY, -1, -1, -1, -1, -1, 0, 0, 0, 0};
  }
  return 0;
}
int wdpm_outlets_stats(wdpm_ponds *h, wdpm_pond_outlet_stats *out) {
  (void)h;
  ENTER(wdpm_outlets_stats);
  *out = (wdpm_pond_outlet_stats){stub_n(), 5, 6, 77};
  return 0;
}
#endif

#if STUB_UNITS >= 5
int wdpm_curves_label(wdpm_ponds *h, double min_depth, int64_t *nponds) { (void)h; LABEL(wdpm_curves_label); }
int wdpm_curves_table(wdpm_ponds *h, wdpm_pond_curve *out, int64_t capacity) {
  (void)h;
  ROWS(wdpm_curves_table);
  for (int64_t k = 0; k < stub_n(); k++) {
    out[k].bed_level = val(k, 6);
    out[k].top_level = k == 1 ? INFINITY : val(k, 6) + val(k, 7) / 300.0;
    for (int s = 0; s < WDPM_CURVE_STAGES; s++) {
      out[k].cells[s] = k == 1 ? 0 : (s + 1) * (3 + k);
      out[k].q[s] = k == 1 ? 0 : quanta(k, 2) / (uint64_t)(WDPM_CURVE_STAGES - s);
    }
  }
  return 0;
}
int wdpm_curves_stats(wdpm_ponds *h, wdpm_pond_curve_stats *out) {
  (void)h;
  ENTER(wdpm_curves_stats);
  *out = (wdpm_pond_curve_stats){stub_n(), 8, 9, 1010};
  return 0;
}
/* the library's rule (include/wdpm_pond_curves.h): bed for s == 0, top for s == 16, between them one subtraction, one
 * multiplication by the exact s / 16 and one addition, each rounded (built with -ffp-contract=off); NaN for any other s */
double wdpm_curves_stage_level(double bed, double top, int s) {
  if (s == 0) return bed;
  if (s == WDPM_CURVE_STAGES) return top;
  if (s < 0 || s > WDPM_CURVE_STAGES) return NAN;
  const double span = top - bed, part = span * ((double)s / WDPM_CURVE_STAGES);
  return bed + part;
}
#endif
