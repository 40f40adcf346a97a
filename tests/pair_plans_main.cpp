/* Prints, one JSON object per line, what plan_iter2() (wdpm_amd/csrc/wdpm_dispatch.h) decides for a request that meets every
 * condition of a two-iteration launch and for requests that miss exactly one of them: tests/test_pair_iterations.py.  Host compiler only.
 *
 * With arguments: one line per argument `name:R:C:codes16:balance:ring:clamp_ok` - the forced two-iteration launch (WDPM_RELAY=0
 * WDPM_TRI=0 WDPM_ITER2=2, codes forced) of an R x C raster as tests/test_iter2_corners.py plays it: 16-bit offsets or 32-bit codes,
 * WDPM_BALANCE, WDPM_ITER2_RING, and whether the clamped neighbour step is allowed (WDPM_CLAMP and the DEM's bound). */
#include <cstdio>
#include <cstring>

#include "../wdpm_amd/csrc/wdpm_dispatch.h"

static DeviceFacts mi355x() {
  DeviceFacts f{256, 163840, 256 * 2 * 4, {}};
  for (int m = 0; m < 2; m++)
    for (int k = 0; k < 3; k++) f.resident_waves[m][k] = 256 * (m == 1 && k == 2 ? 1 : 2) * 4;
  return f;
}

static LaunchRequest request(const int rows, const int ncp) {
  LaunchRequest q{};
  q.module = WDPM_ADD;
  q.g = SlabGeom{rows, ncp, 0, rows - 2, ncp - 2, rows / 2, ncp / 2, -1.0};
  q.A0 = 0; q.out_last = rows - 1;
  q.flags = WDPM_LAUNCH_PLAIN | WDPM_LAUNCH_CLAMP_OK;
  q.codes32 = q.codes16 = true;
  q.balance_mode = 1; q.balance_capacity = 1 << 16;
  return q;
}

static bool same_plan(const LaunchPlan &a, const LaunchPlan &b) {
  bool s = a.error == b.error && a.family == b.family && a.grid == b.grid && a.block == b.block && a.lds == b.lds && a.nstrips == b.nstrips &&
           a.nchunks == b.nchunks && a.nitems == b.nitems && a.H == b.H && a.wpb == b.wpb && a.prio == b.prio && a.no_clamp == b.no_clamp &&
           a.fold_md == b.fold_md && a.tiles_fit == b.tiles_fit && a.keep_tiles == b.keep_tiles && a.balance == b.balance && a.table == b.table &&
           a.steady == b.steady && a.measure_equal == b.measure_equal && a.pair == b.pair && a.ipx == b.ipx && a.rot == b.rot &&
           a.ledger_sw == b.ledger_sw && a.relay_flags == b.relay_flags;
  for (int k = 0; k < 6; k++) s = s && a.targs[k] == b.targs[k];
  return s;
}

static void say(const char *name, const LaunchRequest &q, const Switches &sw, const int left) {
  const DeviceFacts f = mi355x();
  const LaunchPlan p = plan_iter2(q, f, sw, left), one = plan_iteration(q, f, sw);
  printf("{\"case\": \"%s\", \"iter2\": %d, \"single_untouched\": %s, \"grid\": %u, \"block\": %u, \"lds\": %u, \"groups\": %d, \"nchunks\": %d, "
         "\"H\": %d, \"ring_rows\": %d, \"ledger_sw\": %d, \"table\": %s, \"ipx\": %d, \"codes\": %d, \"single_codes\": %d, "
         "\"single_ledger_sw\": %d, \"single_marching\": %s}\n",
         name, p.iter2, (p.iter2 || same_plan(p, one)) ? "true" : "false", p.grid, p.block, p.lds, p.nstrips, p.nchunks, p.H, p.ring_rows,
         p.ledger_sw, p.table ? "true" : "false", p.ipx, p.targs[2], one.targs[2], one.ledger_sw,
         one.family == WDPM_FAMILY_MARCHING && one.targs[5] == 1 ? "true" : "false");
}

/* the launches tests/test_iter2_corners.py forces onto small rasters */
static int corners(const int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    char name[128];
    int R, C, codes16, balance, ring, clamp_ok;
    if (sscanf(argv[i], "%127[^:]:%d:%d:%d:%d:%d:%d", name, &R, &C, &codes16, &balance, &ring, &clamp_ok) != 7) return 1;
    Switches sw; sw.iter2 = 2; sw.relay = 0; sw.tri = 0; sw.iter2_ring = ring;
    LaunchRequest q = request(R + 2, C + 2);
    q.force_codes = 1;
    q.codes16 = codes16 != 0;
    q.flags = WDPM_LAUNCH_PLAIN | (clamp_ok ? WDPM_LAUNCH_CLAMP_OK : 0);
    q.balance_mode = balance; q.balance_capacity = 16384;
    say(name, q, sw, 2);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1) return corners(argc, argv);
  const Switches dflt;
  const LaunchRequest big = request(16386, 16386);
  say("offered", big, dflt, 2);
  say("offered-many-left", big, dflt, 998);
  { LaunchRequest q = big; q.module = WDPM_SUBTRACT; say("offered-subtract", q, dflt, 2); }
  { LaunchRequest q = big; q.codes16 = false; say("offered-codes32", q, dflt, 2); }
  { LaunchRequest q = big; q.module = WDPM_DRAIN; say("refused-drain", q, dflt, 2); }
  { LaunchRequest q = big; q.A0 = 300; say("refused-window-top", q, dflt, 2); }
  { LaunchRequest q = big; q.out_last = 9000; say("refused-window-bottom", q, dflt, 2); }
  { LaunchRequest q = big; q.flush = true; say("refused-flush", q, dflt, 2); }
  { LaunchRequest q = big; q.max_diff = true; say("refused-max-diff", q, dflt, 2); }
  { LaunchRequest q = big; q.flags = WDPM_LAUNCH_CLAMP_OK; say("refused-gated-water", q, dflt, 2); }
  { LaunchRequest q = big; q.signed_zero_safe = true; say("refused-negative-zero", q, dflt, 2); }
  { LaunchRequest q = big; q.codes32 = q.codes16 = false; say("refused-fp64-dem", q, dflt, 2); }
  { LaunchRequest q = big; q.tiles_offered = true; q.tile_capacity = 1 << 20; say("refused-dry-tile-flags", q, dflt, 2); }
  { LaunchRequest q = big; q.chunk_rows = 24; say("refused-caller-chunk-height", q, dflt, 2); }
  { LaunchRequest q = big; q.leave_cus = 8; say("refused-room-for-transfers", q, dflt, 2); }
  say("refused-one-iteration-left", big, dflt, 1);
  { Switches sw; sw.iter2 = 0; say("refused-switched-off", big, sw, 2); }
  { Switches sw; sw.chunk_rows = 24; say("refused-env-chunk-height", big, sw, 2); }
  { Switches sw; sw.plain = 0; LaunchRequest q = big; q.flags = wdpm_launch_flags(sw, true, true); say("refused-plain-off", q, sw, 2); }
  // the size threshold: automatic from the 2049 x 16384 add slab up, forced wherever the marching kernel runs with codes
  say("offered-8192", request(8194, 8194), dflt, 2);
  say("offered-slab", request(2051, 16386), dflt, 2);
  say("refused-4096", request(4098, 4098), dflt, 2);
  { Switches sw; sw.iter2 = 2; say("forced-4096", request(4098, 4098), sw, 2); }
  { Switches sw; sw.iter2 = 2; sw.relay = 0; sw.tri = 0; LaunchRequest q = request(304, 1702); q.force_codes = 1; say("forced-small", q, sw, 2); }
  { Switches sw; sw.iter2 = 2; sw.relay = 0; sw.tri = 0; LaunchRequest q = request(304, 1702); q.force_codes = 1; q.module = WDPM_DRAIN; say("forced-small-refused-drain", q, sw, 2); }
  { Switches sw; sw.iter2 = 2; LaunchRequest q = request(304, 1702); q.force_codes = 1; say("forced-small-refused-relay", q, sw, 2); }
  { Switches sw; sw.iter2_ring = 12; say("ring-12", big, sw, 2); }
  return 0;
}
