/* Prints what plan_iteration() (wdpm_amd/csrc/wdpm_dispatch.h) decides for every request of the sweep in dispatch_sweep.h, one
 * line per request, under every switch profile: tests/test_dispatch_plans.py compares it with tests/golden/dispatch_plans.json.gz.
 * Host compiler only (wdpm_amd/csrc/Makefile: dispatch_plans); exits 1 when a plan names an instantiation that is in no variant list. */
#include "../wdpm_amd/csrc/wdpm_dispatch.h"
#include "dispatch_sweep.h"

static DeviceFacts facts_of(const SweepDevice &d) {
  DeviceFacts f{d.cus, d.lds_per_cu, d.cus * d.tri_blocks * 4, {}};
  const int built_for[2][3] = {{2, 2, 2}, {2, 2, 1}};     /* fused_built_for of the six occupancy classes (wdpm_march.hip) */
  for (int m = 0; m < 2; m++)
    for (int k = 0; k < 3; k++) f.resident_waves[m][k] = d.cus * (d.blocks[m][k] < built_for[m][k] ? d.blocks[m][k] : built_for[m][k]) * 4;
  return f;
}

int main(int argc, char **argv) {
  int unlisted = 0;
  for (int pi = 0; pi < kSweepProfileCount; pi++) {
    const SweepProfile &prof = kSweepProfiles[pi];
    if (argc > 1 && strcmp(argv[1], prof.name)) continue;
    const Switches sw = wdpm_read_switches([&](const char *name) { return sweep_profile_get(prof, name); });
    const DeviceFacts facts = facts_of(kSweepDevices[prof.device]);
    printf("# profile %s\n", prof.name);
    for (const SweepCase &c : sweep_cases(pi == 0)) {
      LaunchRequest q{};
      q.module = c.module;
      q.g = SlabGeom{c.rows, c.ncp, 0, c.rows - 2, c.ncp - 2, c.rows / 2, c.ncp / 2, -1.0};
      q.A0 = c.A0; q.out_last = c.out_last; q.chunk_rows = c.chunk_rows;
      q.signed_zero_safe = c.szs; q.flush = c.flush; q.max_diff = c.md;
      q.flags = wdpm_launch_flags(sw, c.water_plain, c.dem_bounded);
      q.leave_cus = c.leave_cus;
      q.codes32 = c.dem >= 1; q.codes16 = c.dem >= 2; q.force_codes = c.force;
      q.tiles_offered = c.tiles != 0; q.tile_capacity = c.tile_cap; q.wide_tri_ok = c.tiles == 2;
      q.balance_mode = c.bal_mode; q.balance_capacity = c.bal_cap;
      const LaunchPlan p = plan_iteration(q, facts, sw);
      SweepRow r{};
      r.error = p.error;
      if (!p.error) {
        r.family = p.family;
        for (int k = 0; k < 6; k++) r.targs[k] = p.targs[k];
        r.grid = p.grid; r.block = p.block; r.lds = p.lds; r.nstrips = p.nstrips; r.nitems = p.nitems;
        r.relay_flags = p.relay_flags; r.ledger_sw = p.ledger_sw;
        if (p.family == WDPM_FAMILY_MARCHING) {
          r.nchunks = p.nchunks; r.H = p.H; r.prio = p.prio; r.no_clamp = p.no_clamp;
          r.tiles_fit = p.tiles_fit; r.keep_tiles = p.keep_tiles; r.table = p.table;
          r.measured = (p.table && p.steady) || p.measure_equal;      /* on balance state as a context starts with */
          r.rot = p.table ? p.rot : p.measure_equal;
          if (p.table) { r.pair = p.pair; r.ipx = p.ipx; }            /* (xcd_rebalance_kernel's arguments: only then) */
        }
        const int at = p.family == WDPM_FAMILY_MARCHING ? wdpm_find_variant(kMarchingVariants, p.targs)
                       : p.family == WDPM_FAMILY_RELAY  ? wdpm_find_variant(kRelayVariants, p.targs)
                                                        : wdpm_find_variant(kTriangleVariants, p.targs);
        if (at < 0) { unlisted++; fprintf(stderr, "not in its family's variant list: "); sweep_print(stderr, c, r); }
      }
      sweep_print(stdout, c, r);
    }
  }
  return unlisted ? 1 : 0;
}
