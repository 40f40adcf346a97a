/* The fixed sweep of iteration-launch requests behind tests/test_dispatch_plans.py, the switch profiles it runs under and the
 * format of a row of tests/golden/dispatch_plans.json.gz.  Plain C++17, no dependency on the dispatch: the fixture was recorded
 * by running this same sweep through the host dispatch of the commit named in the fixture's header. */
#ifndef WDPM_DISPATCH_SWEEP_H
#define WDPM_DISPATCH_SWEEP_H

#include <cstdio>
#include <cstring>
#include <vector>

struct SweepDevice { int cus, lds_per_cu, tri_blocks, blocks[2][3]; };   /* blocks: occupancy of the marching kernel, [drain][fp64, codes, -0.0-safe] */
/* [0]: read on an MI355X from the build of the commit the fixture was recorded from (occupancy API, before the cap of fused_built_for);
 * [1]: an invented smaller device, for the comparisons that no size reaches on the real one (the LDS pad, the occupancy cap) */
constexpr SweepDevice kSweepDevices[2] = {{256, 163840, 3, {{2, 2, 3}, {2, 2, 2}}}, {64, 65536, 2, {{2, 1, 1}, {1, 2, 2}}}};

struct SweepCase {
  int module, rows, ncp, A0, out_last;
  int chunk_rows, szs, flush, md;
  int water_plain, dem_bounded;      /* what wdpm_launch_flags() makes LaunchRequest::flags from */
  int leave_cus, dem /* 0 fp64 only, 1 32-bit codes, 2 and 16-bit offsets */, force;
  int tiles /* 0 none, 1 offered, 2 offered and wide_tri_ok */, tile_cap, bal_mode, bal_cap;
};

struct SweepRow {          /* what was decided; fields a family does not have stay 0 */
  int error, family, targs[6];
  unsigned grid, block, lds;
  int nstrips, nchunks, nitems, H, prio, no_clamp, relay_flags, tiles_fit, keep_tiles, table, measured, rot, pair, ipx, ledger_sw;
};

struct SweepProfile { const char *name; const char *env[5][2]; int device = 0; };
/* the default switches; every environment of tests/test_forced_variants.py::VARIANTS and tests/test_kernel_coverage.py::PROFILES as
 * far as it steers the dispatch (WDPM_DEM32 / _DEM16 / _BALANCE / _GRAPH reach it through the request: see sweep_cases); one
 * profile each for the switches those leave alone, and the remaining values of the forcing switches */
constexpr SweepProfile kSweepProfiles[] = {
    {"default", {}},
    {"gated-unclamped-no-priorities", {{"WDPM_PLAIN", "0"}, {"WDPM_CLAMP", "0"}, {"WDPM_PRIO", "0"}}},
    {"marching-everywhere", {{"WDPM_RELAY", "0"}, {"WDPM_TRI", "0"}}},
    {"marching-everywhere-paired", {{"WDPM_RELAY", "0"}, {"WDPM_TRI", "0"}, {"WDPM_PAIR", "2"}}},
    {"relay-everywhere-four-waves", {{"WDPM_RELAY", "2"}, {"WDPM_RELAY_NW", "4"}, {"WDPM_RELAY_PRIO", "2"}}},
    {"relay-everywhere-eight-waves", {{"WDPM_RELAY", "2"}, {"WDPM_RELAY_NW", "8"}, {"WDPM_RELAY_PRIO", "2"}}},
    {"triangle-everywhere-six-rows", {{"WDPM_TRI", "2"}, {"WDPM_RELAY", "0"}, {"WDPM_TRI_K", "2"}}},
    {"triangle-everywhere-three-rows", {{"WDPM_TRI", "2"}, {"WDPM_RELAY", "0"}, {"WDPM_TRI_K", "1"}}},
    {"relay-nw8", {{"WDPM_RELAY_NW", "8"}}},
    {"relay-nw4", {{"WDPM_RELAY_NW", "4"}}},
    {"triangle", {{"WDPM_RELAY", "0"}}},
    {"triangle-k2", {{"WDPM_RELAY", "0"}, {"WDPM_TRI_K", "2"}}},
    {"triangle-k1", {{"WDPM_RELAY", "0"}, {"WDPM_TRI_K", "1"}}},
    {"rot-0", {{"WDPM_ROT", "0"}}},
    {"pair-0", {{"WDPM_PAIR", "0"}}},
    {"relay-dem32-0", {{"WDPM_RELAY_DEM32", "0"}}},
    {"chunk-rows-48", {{"WDPM_CHUNK_ROWS", "48"}}},
    {"chunk-rows-2", {{"WDPM_CHUNK_ROWS", "2"}}},
    {"tri-0", {{"WDPM_TRI", "0"}}},
    {"prio-0", {{"WDPM_PRIO", "0"}}},
    {"relay-prio-0", {{"WDPM_RELAY_PRIO", "0"}}},
    {"small-device", {}, 1},
};
constexpr int kSweepProfileCount = (int)(sizeof kSweepProfiles / sizeof kSweepProfiles[0]);
inline const char *sweep_profile_get(const SweepProfile &p, const char *name) {
  for (const auto &kv : p.env)
    if (kv[0] && !strcmp(kv[0], name)) return kv[1];
  return nullptr;
}

struct SweepShape { int rows, ncp; };
/* padded squares from 3^2 to 16384^2 - either side of every comparison of the dispatch at kSweepDevice (one strip / two, one round of
 * relay workgroups, of triangle waves, 2.7 rounds, seven / ten relay rounds, every slot filled at 18 / 12 rows a chunk, 10^8 cells) -
 * and the slabs DESIGN.md and tests/test_balance_pairing.py quote */
inline std::vector<SweepShape> sweep_shapes(const bool all) {
  std::vector<SweepShape> s;
  const int every[] = {3, 4, 5, 6, 8, 11, 14, 20, 50, 100, 171, 177, 178, 179, 180, 300, 482, 500, 700, 760, 770, 800, 1000, 1200, 1400,
                       1500, 1600, 1800, 2000, 2100, 2200, 2300, 2400, 2500, 2600, 2700, 2800, 2900, 3072, 3200, 3300, 3600,
                       5000, 6000, 9998, 10000, 12000};
  const int few[] = {3, 8, 100, 179, 482, 770, 1200, 1600, 2000, 2200, 2400, 2700, 3300, 3600, 10000};
  if (all) for (const int n : every) s.push_back({n + 2, n + 2});
  else for (const int n : few) s.push_back({n + 2, n + 2});
  const SweepShape slabs[] = {{1055, 8192}, {2116, 16384}, {1053, 8190}, {482, 471}, {484, 473}, {2051, 16386}, {4098, 4098}, {8194, 8194}, {16386, 16386}, {3002, 3002},
                              {12, 180000}, {40, 30000}};      /* more strips than resident waves */
  for (const auto &b : slabs) s.push_back(b);
  return s;
}

/* The sweep: not the full product of all inputs, but every input varied against the shapes and the places in a block. */
inline std::vector<SweepCase> sweep_cases(const bool is_default_profile) {
  std::vector<SweepCase> out;
  const int places[5][2] = {{1, 0}, {0, 0}, {0, 1}, {1, 1}, {0, 0}};   /* (flush, max diff); the last: steady on water that is not plain */
  auto whole = [](const int module, const SweepShape sh) {
    return SweepCase{module, sh.rows, sh.ncp, 0, sh.rows - 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1, 16384};
  };
  auto tile_cap = [](const SweepShape sh) { return (sh.ncp / 171 + 4) * (sh.rows / 6 + 4); };
  for (const auto sh : sweep_shapes(is_default_profile))
    for (const int module : {0, 1, 2})
      for (int place = 0; place < 5; place++) {
        SweepCase c = whole(module, sh);
        c.flush = places[place][0]; c.md = places[place][1]; c.water_plain = place != 4;
        if (module == 1 && place != 1) continue;                       /* subtract is add to the dispatch: shown once per shape */
        for (const int dem : {0, 1, 2, 3}) {                           /* DEM fp64 / 32-bit codes / 16-bit offsets / forced */
          c.dem = dem == 3 ? 2 : dem; c.force = dem == 3;
          if (!is_default_profile && (dem == 1 || (place > 2 && dem != 2))) continue;
          out.push_back(c);
        }
        c.dem = 2; c.force = 0;
        if (place > 2) continue;
        SweepCase v = c; v.szs = 1; v.water_plain = 0; out.push_back(v);               /* a -0.0 somewhere */
        v = c; v.bal_mode = 2; out.push_back(v);                                       /* WDPM_BALANCE=2 */
        v = c; v.tiles = 1; v.tile_cap = tile_cap(sh); v.bal_mode = 1; out.push_back(v);    /* dry-tile flags kept */
        if (!is_default_profile) continue;
        v = c; v.dem_bounded = 0; out.push_back(v);                                    /* no clamped step */
        v = c; v.szs = 1; v.water_plain = 0; v.flush = 0; v.tiles = 1; v.tile_cap = tile_cap(sh); out.push_back(v);
        v = c; v.bal_mode = 0; out.push_back(v);                                       /* WDPM_BALANCE=0 */
        for (const int cap : {600, 2000}) {                                            /* a table too small, or too small for every slot filled */
          v = c; v.bal_cap = cap; out.push_back(v);
          v.bal_mode = 2; out.push_back(v);
        }
        for (const int t : {1, 2})
          for (const int cap : {tile_cap(sh), 40}) {
            if (place != 1 && cap == 40) continue;
            v = c; v.tiles = t; v.tile_cap = cap; v.bal_mode = t == 2 ? 0 : 1; out.push_back(v);
            v.chunk_rows = 96; out.push_back(v);                                       /* a sparse raster's chunk height */
            v.bal_mode = 2; out.push_back(v);
          }
        v = c; v.tiles = 1; v.tile_cap = 0; out.push_back(v);                          /* the graph path's question */
        for (const int h : {1, 2, 3, 4, 7, 12, 30, 100000}) {
          if (place != 1 && h != 3 && h != 30) continue;
          v = c; v.chunk_rows = h; out.push_back(v); v.bal_mode = 2; out.push_back(v); }
        if (place == 0) { v = c; v.szs = 1; out.push_back(v); }                        /* flush and -0.0: refused */
      }
  /* max diff where no folding variant exists, and windows that are refused */
  for (const auto sh : sweep_shapes(false)) {
    SweepCase c = whole(2, sh); c.md = 1; out.push_back(c);
    c = whole(0, sh); c.md = 1; c.szs = 1; out.push_back(c);
    for (const int module : {0, 2})          /* windows of one and two rows */
      for (const int last : {6, 7}) { c = whole(module, sh); c.A0 = 6; c.out_last = last; if (last < sh.rows) out.push_back(c); }
    if (!is_default_profile) continue;
    c = whole(0, sh); c.A0 = -3; out.push_back(c);
    c = whole(0, sh); c.A0 = 1; out.push_back(c);
    c = whole(0, sh); c.out_last = sh.rows; out.push_back(c);
    if (sh.rows > 6) { c = whole(0, sh); c.A0 = 6; c.out_last = 5; out.push_back(c); }
  }
  /* the three windows of an overlapped iteration (wdpm_iterate_overlapped), with 0 and 8 compute units left free */
  for (const auto sh : sweep_shapes(is_default_profile)) {
    if (sh.rows < 64) continue;
    for (const int halo : {3, 24, 96}) {
      if (!is_default_profile && halo != 24) continue;
      int t_last = halo - 1, b_first = sh.rows - halo;
      while ((t_last + 1) % 3 != 2) t_last++;
      while (b_first % 3 != 2) b_first--;
      if (b_first - (t_last + 1) < 24) continue;
      const int win[3][2] = {{0, t_last}, {b_first - 2, sh.rows - 1}, {t_last - 1, b_first - 1}};
      for (int w = 0; w < 3; w++)
        for (int place = 0; place < (is_default_profile ? 4 : 2); place++)
          for (const int leave : {0, 8, 127, 128, 200}) {
            if (leave && w != 2) continue;
            if (leave > 8 && !(is_default_profile && place == 1 && halo == 24)) continue;
            SweepCase c = whole(0, sh);
            c.A0 = win[w][0]; c.out_last = win[w][1]; c.flush = places[place][0]; c.md = places[place][1];
            c.bal_mode = 0; c.leave_cus = leave; c.dem = 2;
            out.push_back(c);
            if (is_default_profile && halo == 24 && place == 1) {
              c.chunk_rows = 30; out.push_back(c); c.chunk_rows = 0; c.szs = 1; c.water_plain = 0; out.push_back(c);
              c.szs = 0; c.water_plain = 1; c.chunk_rows = 30; c.bal_mode = 2; c.tiles = 1; c.tile_cap = tile_cap(sh); out.push_back(c); c.tiles = 0; out.push_back(c);
            }
          }
    }
  }
  return out;
}

inline void sweep_print(FILE *f, const SweepCase &c, const SweepRow &r) {
  fprintf(f, "m=%d %dx%d w=%d:%d ch=%d z=%d fl=%d md=%d wp=%d db=%d lc=%d dem=%d frc=%d t=%d tc=%d b=%d bc=%d -> ", c.module, c.rows, c.ncp,
          c.A0, c.out_last, c.chunk_rows, c.szs, c.flush, c.md, c.water_plain, c.dem_bounded, c.leave_cus, c.dem, c.force, c.tiles,
          c.tile_cap, c.bal_mode, c.bal_cap);
  if (r.error) { fprintf(f, "refused\n"); return; }
  static const char *const names[] = {"relay", "triangle", "marching"};
  fprintf(f, "%s<%d,%d,%d,%d,%d", names[r.family], r.targs[0], r.targs[1], r.targs[2], r.targs[3], r.targs[4]);
  if (r.family == 2) fprintf(f, ",%d", r.targs[5]);
  fprintf(f, "> grid=%u block=%u lds=%u nstrips=%d nitems=%d", r.grid, r.block, r.lds, r.nstrips, r.nitems);
  if (r.family == 0) fprintf(f, " flags=%d", r.relay_flags);
  if (r.family == 2)
    fprintf(f, " nchunks=%d H=%d prio=%d no_clamp=%d tiles=%d/%d table=%d measured=%d rot=%d pair=%d ipx=%d", r.nchunks, r.H, r.prio, r.no_clamp,
            r.tiles_fit, r.keep_tiles, r.table, r.measured, r.rot, r.pair, r.ipx);
  fprintf(f, " ledger=%d\n", r.ledger_sw);
}

#endif
