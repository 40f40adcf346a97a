/*
 * wdpm_dispatch.h — which kernel instantiation an iteration launch uses, with which grid, chunk height, LDS pad and switches
 * (DESIGN.md §4.4 is the specification; nearly every threshold below was bought with an A/B run under profiles/).
 * Plain C++17 and nothing else: no HIP header, no getenv, no statics, no pointer dereferenced.  plan_iteration() only decides;
 * wdpm_march.hip and wdpm_small.hip launch what it decided, wdpm_block.hip asks.  tests/test_dispatch_plans.py holds every decision against a
 * recorded table (tests/golden/dispatch_plans.json.gz) without a GPU.
 */
#ifndef WDPM_DISPATCH_H
#define WDPM_DISPATCH_H

#include <cstdlib>

#include "../../include/wdpm.h"

/* A raster slab resident in HBM: rows x ncp doubles, row-major, row 0 of the slab is padded
 * row `row0` of the whole raster (row0 % 3 == 0). */
struct SlabGeom {
  int rows;      /* padded rows held */
  int ncp;       /* padded columns (ncols + 2) */
  int row0;      /* global padded row of slab row 0 */
  int R, C;      /* file raster size (centres are global rows 1..R, cols 1..C) */
  int dr, dc;    /* drain cell, slab-local row / column (drain module; may lie outside the slab) */
  double miss;   /* NODATA value */
};

constexpr int kLanes = 64;
constexpr int kStripIn = 3 * kLanes;                     // 192 columns loaded per wave
// Per fused iteration an error at a strip's edge travels at most 8 columns inward from the left and
// 12 from the right (cell-level dependency simulation, tests/test_rowblock.py); 13 are given up on
// the right so that the strip pitch, 171, is a multiple of 3 and every strip starts on a block edge.
constexpr int kHaloL = 8, kHaloR = 13;
constexpr int kStripOut = kStripIn - kHaloL - kHaloR;    // 171 columns stored per wave
// Two iterations per launch (plan_iter2): four neighbouring strips share their exact columns through LDS, so only the two outer
// edges of the GROUP pay for the wider dependency cone: 3 x 171 + 192 columns in, 42 fewer out - 663 = 3 x 221, group origins stay
// on block edges.  Over TWO iterations an error at the group's edge travels 17 columns inward from the left (not 2 x 8: the second
// iteration's unknown columns end at column 7, which is no block edge) and 24 from the right (tests/test_pair_iterations.py runs
// the cell-level dependency simulation); 25 are given up on the right so that the group pitch is a multiple of 3.
constexpr int kGroupStrips = 4;
constexpr int kGroupIn = (kGroupStrips - 1) * kStripOut + kStripIn;     // 705
constexpr int kGroupHaloL = 17, kGroupHaloR = 25;
constexpr int kGroupOut = kGroupIn - kGroupHaloL - kGroupHaloR;         // 663
// A ring row is a group row and a few cells that take the columns a producer does not own.
constexpr int kRingPitch = kGroupIn + 7;                                 // 712 doubles

/* The switches that steer the iteration dispatch: (member, environment variable, default).  README has the table of meanings;
 * A/B runs and tests set them, nobody else. */
#define WDPM_SWITCHES(X)                                                                                              \
  X(tri, "WDPM_TRI", 1)                 /* 0 keeps the marching kernel, 2 forces the triangle kernel on any size */   \
  X(tri_k, "WDPM_TRI_K", 0)             /* 1|2 forces the triangle kernel's height (tuning, tests); 0 = automatic */  \
  X(relay, "WDPM_RELAY", 1)             /* 0 never, 2 on any size */                                                  \
  X(relay_nw, "WDPM_RELAY_NW", 0)       /* 4|8 forces the workgroup's height (tuning); 0 = automatic */               \
  X(relay_prio, "WDPM_RELAY_PRIO", 1)   /* stage priorities: 0 never, 2 always */                                     \
  X(relay_dem32, "WDPM_RELAY_DEM32", 1) /* 0: the fp64 DEM in the relay kernel (A/B) */                               \
  X(chunk_rows, "WDPM_CHUNK_ROWS", 0)   /* >= 3: the marching kernel's chunk height */                                \
  X(pair, "WDPM_PAIR", 1)               /* 0: round 4's geometry (A/B, tests); 2: see plan_iteration */               \
  X(rot, "WDPM_ROT", 1)                 /* 0: shares and measurements by blockIdx % 8, as in round 4 (A/B) */         \
  X(prio, "WDPM_PRIO", 1)               /* 0: no priorities (A/B, tests) */                                           \
  X(clamp, "WDPM_CLAMP", 1)             /* 0: the unclamped neighbour step everywhere (A/B, tests) */                 \
  X(plain, "WDPM_PLAIN", 1)             /* 0: gated variants only (A/B, tests) */                                     \
  X(iter2, "WDPM_ITER2", 1)             /* two iterations per marching launch: 0 never, 1 where it pays, 2 wherever it fits */ \
  X(iter2_ring, "WDPM_ITER2_RING", 0)   /* >= 6: group rows in its LDS ring (tuning); 0 = automatic */                \
  X(iter2_prio, "WDPM_ITER2_PRIO", 1)   /* 0: its producers keep the default issue priority (A/B) */
struct Switches {
#define WDPM_SWITCH_MEMBER(member, name, dflt) int member = dflt;
  WDPM_SWITCHES(WDPM_SWITCH_MEMBER)
#undef WDPM_SWITCH_MEMBER
};
/* `get` is getenv or a stand-in.  The library reads its environment through this once per process (wdpm_ctx.h::wdpm_switches) */
template <class Get> inline Switches wdpm_read_switches(Get get) {
  Switches sw;
#define WDPM_SWITCH_READ(member, name, dflt) if (const char *e = get(name)) sw.member = atoi(e);
  WDPM_SWITCHES(WDPM_SWITCH_READ)
#undef WDPM_SWITCH_READ
  return sw;
}

/* LaunchRequest::flags.  bit 0 (WDPM_LAUNCH_PLAIN): the caller knows (wdpm_launch_scan_water, and nothing written since that could change
 * it) that every cell of w_in that may not give water holds +0.0: launches that have such a variant then run without the centre gate.
 * bit 1 (WDPM_LAUNCH_CLAMP_OK): every valid elevation is below 2^30 m in magnitude (wdpm_launch_dem_min), so that half an ulp of an
 * elevation is nothing against a depth: the kernels may take a flow's `max(x / 8, -0.0)` as one clamped instruction wherever
 * the depths they hold are shallow enough for it to be exact (wdpm_stencil.h::eighth_clamped, `deep` in wdpm_march.hip). */
enum { WDPM_LAUNCH_PLAIN = 1, WDPM_LAUNCH_CLAMP_OK = 2 };
inline int wdpm_launch_flags(const Switches &sw, const bool water_plain, const bool dem_bounded) {
  return (sw.plain != 0 && water_plain ? WDPM_LAUNCH_PLAIN : 0) | (sw.clamp != 0 && dem_bounded ? WDPM_LAUNCH_CLAMP_OK : 0);
}

/* The 16-bit DEM offsets (wdpm_kernels.h::DemCode) only where they pay: rasters far beyond the 256 MB Infinity Cache, where the bytes are what a launch waits for (16384^2
 * +2.5 %, 8192^2 +0.3 %, 4096^2 -2.2 %: nine integer adds more per step; profiles/r04/dem16_bench*_ab.txt) - or when forced (tests) */
inline bool wdpm_dem16_pays(long long cells_of_the_launch, int force) { return cells_of_the_launch >= 100000000LL || force != 0; }

/* What the dispatch needs to know of a device.  Filled once per device ordinal by the units that own the kernels (wdpm_march.hip, wdpm_small.hip:
 * the occupancy API needs their addresses), never on the launch path. */
struct DeviceFacts {
  int cus;               /* compute units */
  int lds_per_cu;        /* bytes */
  int tri_slots;         /* waves of the triangle kernel the chip holds at once */
  /* Number of waves of the marching kernel the whole chip holds at once (CUs x blocks/CU x 4 waves), [drain module][-0.0-safe ? 2 :
   * DEM codes ? 1 : 0].  All work items of a launch are made resident together — one round, no tail — so the item count is sized
   * to this.  Never more than the kernel was built for (fused_built_for): the chunk heights and every threshold of the dispatch
   * were measured at that occupancy, and the register count an instantiation ends up with may allow more from one compiler run
   * to the next. */
  int resident_waves[2][3];
};

/* what the caller knows of one iteration launch */
struct LaunchRequest {
  int module;              /* WDPM_ADD | WDPM_SUBTRACT | WDPM_DRAIN */
  SlabGeom g;
  int A0, out_last;        /* the output rows [A0 + 2 (0 when A0 == 0), out_last]; A0 % 3 == 0 */
  int chunk_rows;          /* >= 3: the caller's chunk height */
  bool signed_zero_safe;   /* the water raster may hold a -0.0 (wdpm_stencil.h::flow_add_nz is not exact then) */
  bool flush;              /* the block's threshold flush rides on this launch */
  bool max_diff;           /* max |w - oldw| is folded into it */
  int flags;               /* WDPM_LAUNCH_* */
  int leave_cus;           /* size the launch as if the chip had that many compute units fewer - the interior launch of an overlapped
                            * iteration leaves room for the RCCL send/recv kernels queued beside it (a launch otherwise fills every
                            * slot for its whole duration, and the transfer would start only when the first waves retire) */
  bool codes32, codes16;   /* DemCode::q / ::h exist */
  int force_codes;         /* DemCode::force */
  bool tiles_offered;      /* a TilePlan comes with the launch ... */
  int tile_capacity;       /* ... with flag arrays of that many tiles (0: none) */
  bool wide_tri_ok;        /* TilePlan::wide_tri_ok */
  int balance_mode;        /* XcdBalance::mode, 0 where no balance state comes with the launch */
  int balance_capacity;    /* XcdBalance::capacity */
};

enum LaunchFamily { WDPM_FAMILY_RELAY = 0, WDPM_FAMILY_TRIANGLE = 1, WDPM_FAMILY_MARCHING = 2 };

struct LaunchPlan {
  int error;               /* nonzero: the request is invalid (hipErrorInvalidValue), nothing else below is meaningful */
  LaunchFamily family;
  int targs[6];            /* the instantiation's template arguments in its family's order (see the variant lists below) */
  unsigned grid, block, lds;   /* workgroups, threads of each, dynamic LDS in bytes */
  int nstrips, nchunks, nitems, H, wpb;   /* strips, chunks per strip, work items, chunk height in rows, waves per workgroup */
  int prio, no_clamp;      /* marching kernel arguments */
  int relay_flags;         /* relay kernel: bit 0 ordinary stores, bit 1 stage priorities, bit 2 no clamped step */
  bool fold_md;            /* the launch takes the caller's MaxDiffArgs */
  bool tiles_fit;          /* the launch's tiling is handed to the TilePlan ... */
  bool keep_tiles;         /* ... and the kernel reads / writes the flags */
  bool balance;            /* the launch may look at the balance state at all ... */
  bool table;              /* ... and takes its chunk heights from the table */
  bool steady;             /* neither a block's first launch (flush) nor its last (max diff) */
  bool measure_equal;      /* no table, but equal chunks tall enough to learn the XCDs' speeds from */
  int pair, ipx;           /* xcd_rebalance_kernel's arguments */
  bool rot;                /* with the table: shares and measurements by physical XCD (BalanceArgs::rot) */
  int ledger_sw;           /* the switches this launch hands the kernel, for the launch ledger (include/wdpm.h: WDPM_LEDGER_*) */
  int iter2;               /* plan_iter2: the launch runs two iterations (Iter2Args); nstrips then counts GROUPS of four strips and
                            * nitems workgroups, one per group and chunk */
  int ring_rows, iter2_prio;   /* Iter2Args */
};

/* One list per kernel family of the instantiations the library contains: wdpm_march.hip / wdpm_small.hip instantiate the kernels, register the
 * ledger slots and build their launch tables from these and nothing else; a plan whose targs are not in its family's list is an
 * error at the launch, not a fallback. */
/* fused_iteration_kernel<module, -0.0-safe, DEM codes (0 fp64, 1 32-bit, 2 16-bit offsets), flush on load, max diff folded in, gate-free> */
#define WDPM_VARIANTS_MARCHING(X)                                                                          \
  X(0, true, 0, false, false, false) X(2, true, 0, false, false, false)                                   \
  X(0, false, 0, false, false, false) X(0, false, 0, true, false, false) X(0, false, 0, false, false, true) \
  X(0, false, 0, false, true, false) X(0, false, 0, true, true, false)                                    \
  X(0, false, 1, false, false, false) X(0, false, 1, true, false, false) X(0, false, 1, false, false, true) \
  X(0, false, 1, false, true, false) X(0, false, 1, true, true, false)                                    \
  X(0, false, 2, false, false, false) X(0, false, 2, true, false, false) X(0, false, 2, false, false, true) \
  X(0, false, 2, false, true, false) X(0, false, 2, true, true, false)                                    \
  X(2, false, 0, false, false, false) X(2, false, 0, true, false, false) X(2, false, 0, false, false, true) \
  X(2, false, 1, false, false, false) X(2, false, 1, true, false, false) X(2, false, 1, false, false, true) \
  X(2, false, 2, false, false, false) X(2, false, 2, true, false, false) X(2, false, 2, false, false, true)
/* relay_iteration_kernel<module, flush on load, gate-free, waves per workgroup, DEM as 32-bit codes> */
#define WDPM_VARIANTS_RELAY(X)                                                                             \
  X(0, false, false, 4, false) X(0, true, false, 4, false) X(0, false, true, 4, false)                    \
  X(0, false, false, 8, false) X(0, true, false, 8, false) X(0, false, true, 8, false)                    \
  X(0, false, false, 8, true) X(0, true, false, 8, true) X(0, false, true, 8, true)                       \
  X(2, false, false, 4, false) X(2, true, false, 4, false) X(2, false, true, 4, false)                    \
  X(2, false, false, 8, false) X(2, true, false, 8, false) X(2, false, true, 8, false)
/* tri_iteration_kernel<module, flush on load, output row triples per wave, gate-free, max diff folded in> */
#define WDPM_VARIANTS_TRIANGLE(X)                                                                          \
  X(0, false, 1, false, false) X(0, true, 1, false, false) X(0, false, 1, true, false)                    \
  X(0, false, 1, false, true) X(0, true, 1, false, true)                                                  \
  X(0, false, 2, false, false) X(0, true, 2, false, false) X(0, false, 2, true, false)                    \
  X(2, false, 1, false, false) X(2, true, 1, false, false) X(2, false, 1, true, false)
#define WDPM_VARIANT_ROW(...) {__VA_ARGS__},
constexpr int kMarchingVariants[][6] = {WDPM_VARIANTS_MARCHING(WDPM_VARIANT_ROW)};
constexpr int kRelayVariants[][6] = {WDPM_VARIANTS_RELAY(WDPM_VARIANT_ROW)};
constexpr int kTriangleVariants[][6] = {WDPM_VARIANTS_TRIANGLE(WDPM_VARIANT_ROW)};
#undef WDPM_VARIANT_ROW
template <int N> inline int wdpm_find_variant(const int (&list)[N][6], const int (&targs)[6]) {
  for (int i = 0; i < N; i++) {
    bool same = true;
    for (int k = 0; k < 6; k++) same = same && list[i][k] == targs[k];
    if (same) return i;
  }
  return -1;
}

/* strips of kStripOut stored columns that cover ncp padded columns */
inline int wdpm_strips(const int ncp) {
  int nstrips = 1;
  if (ncp > kStripIn - kHaloR) nstrips = (ncp - (kStripIn - kHaloR) + kStripOut - 1) / kStripOut + 1;
  return nstrips;
}

/* chunk height in rows (multiple of 3): the rows are cut into as many chunks as keep
 * strips x chunks within one resident round; each chunk pays a 6-row warm-up. */
inline int wdpm_chunk_rows(const int rows, const int nstrips, const int override_rows, const int slots, const int env_h) {
  int H;
  if (override_rows >= 3) {
    H = override_rows / 3 * 3;
  } else if (env_h >= 3) {
    H = env_h / 3 * 3;
  } else {
    int nch = slots / nstrips;
    if (nch < 1) nch = 1;
    H = ((rows - 2 + nch - 1) / nch + 2) / 3 * 3;
    // small rasters cannot fill the chip: short chunks then cost redundant warm-up rows on CUs that
    // would idle anyway and cut the launch's critical path (a wave's march) to a few steps - down to
    // one 3-row step of output per wave (basin5-sized rasters: 12.3 us per iteration against 14.3 with
    // 6-row chunks; the formula only gets there when all chunks still fit in one resident round)
  }
  if (H > rows) H = (rows + 2) / 3 * 3;
  if (H < 3) H = 3;
  return H;
}

/* One iteration restricted to the request's window: relay kernel, triangle kernel or marching kernel, and how. */
inline LaunchPlan plan_iteration(const LaunchRequest &q, const DeviceFacts &dev, const Switches &sw) {
  LaunchPlan p{};
  const int module = q.module, A0 = q.A0, out_last = q.out_last, chunk_rows = q.chunk_rows;
  const bool signed_zero_safe = q.signed_zero_safe, flush = q.flush;
  /* The gate-free variants (PLAIN, see block_update) run for the launches between a block's first (flush on load) and last
   * (max diff), every module and kernel family, whenever the water kinds allow it (drain 8192^2 +4.5 %, 482^2 +3 %, add 16384^2
   * +1.3 % once the two waves of a SIMD ran in step: profiles/r03/plain_water_ab.txt, plain_add_prio_ab.txt). */
  const bool plain = (q.flags & WDPM_LAUNCH_PLAIN) && !signed_zero_safe && !flush && !q.max_diff;
  const int no_clamp = (q.flags & WDPM_LAUNCH_CLAMP_OK) ? 0 : 1;     /* see `deep` in the marching kernel */
  const bool fold_md = q.max_diff && module != 2 && !signed_zero_safe;
  p.error = 1;
  if (q.max_diff && !fold_md) return p;     /* the caller asks only where a folding variant exists */
  if (A0 < 0 || A0 % 3 != 0 || out_last > q.g.rows - 1 || out_last < A0) return p;
  if (flush && signed_zero_safe) return p;   /* the caller flushes in place for that variant */
  p.error = 0;
  p.fold_md = fold_md;
  p.no_clamp = no_clamp;
  const int nstrips = wdpm_strips(q.g.ncp);
  p.nstrips = nstrips;
  const int m2 = module == 2 ? 2 : 0;

  /* The launches of small and mid-size rasters (relay and triangle kernels). */
  {
    // Small launches: if every 3-row chunk of the window fits on the chip at once, the triangle kernel's six
    // lockstep stages beat the marching kernel's nine dependent ones (482 x 471: DESIGN.md §4.1c).
    // WDPM_TRI=0 keeps the marching kernel (A/B runs), WDPM_TRI=2 forces the triangle kernel on any size.
    int nch = (out_last - A0 - 1 + 2) / 3;
    if (nch < 1) nch = 1;
    long long items = (long long)nstrips * nch;
    // ... and somewhat beyond: up to 2.7 rounds of (three-row) triangle waves still beat the marching kernel, whose chunks are
    // only a few steps high at these sizes - with six rows per wave (K = 2) for add / subtract once there is more than one round
    // (1200^2: 24.5 -> 14.7 us per add iteration, 1600^2: 30.2 -> 24.6, 2000^2: 35.8 -> 33.7; drain 1200^2: 31.3 -> 20.8,
    // 2000^2: 48.6 -> 46.8; profiles/r02/tri_sweep.txt)
    // ... unless dry-tile flags are being kept and have not (yet, or lately) said that most of the raster works: the triangle
    // kernel keeps no flags, and a mostly dry raster of this size is better off with the marching kernel skipping its dry tiles
    const bool wide = !q.tiles_offered || q.wide_tri_ok;
    const long long slots_now = dev.tri_slots;
    const long long tri_limit = wide ? slots_now * 27 / 10 : slots_now;
    // more than one round of waves: the launch is bound by instruction issue, and six rows per wave (K = 2: 9 block stages
    // instead of 12 for them) are the cheaper way through; one round: three rows per wave is the shorter critical path
    const bool two = module != 2 && (sw.tri_k == 2 || (sw.tri_k == 0 && items > slots_now));
    // the relay kernel (four or eight waves per strip of six / eighteen rows): add 482^2 7.3 -> 5.2 us per iteration, 700^2
    // 10.0 -> 7.3, 1200^2 14.8 -> 11.8, 1600^2 24.9 -> 23.2; drain 482^2 12.1 -> 8.2, 1000^2 16.3 -> 13.1, 1600^2 34.3 -> 25.5,
    // 2400^2 51.6 -> 45.3, 3000^2 77.5 -> 67.3 (profiles/r03/relay_nw_sweep.txt)
    const long long cus = dev.cus;
    const int rows_out = out_last - A0 - 1;
    const long long nwg4 = (long long)nstrips * ((rows_out + 5) / 6 > 0 ? (rows_out + 5) / 6 : 1);        // four waves: six rows out of twelve
    const long long nwg8 = (long long)nstrips * ((rows_out + 17) / 18 > 0 ? (rows_out + 17) / 18 : 1);    // eight waves: 18 out of 24
    // rounds of workgroups at two waves per SIMD (a CU holds two workgroups of four waves or one of eight); the taller workgroup
    // where it needs fewer rounds: fewer waves and less re-reading per row, but twice as many rows behind one barrier
    const long long r4 = (nwg4 + 2 * cus - 1) / (2 * cus), r8 = (nwg8 + cus - 1) / cus;
    const bool tall = sw.relay_nw == 8 || (sw.relay_nw == 0 && r8 < r4);
    const long long nwg = tall ? nwg8 : nwg4;
    // With every wave on a SIMD of its own: always.  Beyond that, while the sweeps (profiles/r03/relay_nw_sweep.txt) have it ahead
    // of the triangle / marching kernels - add / subtract up to eight rounds (1600^2 20.2 against 24.8 us, 2000^2 28.6 against 33.9,
    // 2400^2 39.0 against 42.4, 3000^2 a tie), drain up to fourteen (3000^2 67 against 78 us, 3600^2 behind) - and where the triangle kernel would run in one
    // round anyway or the raster is known to be mostly wet: like the triangle kernel this one keeps no dry-tile flags (`wide`)
    // Round 4, after the marching kernel's gains (profiles/r04/relay_breakeven.txt, relay against marching, us per iteration): add
    // 2000^2 27.5 / 37.8, 2200^2 (7 rounds) 32.6 / 33.3, 2400^2 (8) 38.4 / 37.4, 2700^2 47.8 / 47.1; drain 2400^2 (8) 51.6 / 57.4,
    // 2700^2 (10) 62.7 / 66.3, 3000^2 (12) 75.9 / 73.6, the 1053 x 8190 slab (12) 74.4 / 72.2: seven and ten rounds.
    const bool relay_ok = sw.tri && !signed_zero_safe && chunk_rows < 3 &&
                          (nwg4 * 4 <= 4 * cus || ((wide || items <= slots_now) && (tall ? r8 : r4) <= (module == 2 ? 10 : 7)) ||
                           sw.relay == 2);
    if (sw.relay && !fold_md && relay_ok) {
      p.family = WDPM_FAMILY_RELAY;
      p.grid = ((unsigned)nwg + 7) / 8 * 8;
      p.block = tall ? 512 : 256;
      p.wpb = tall ? 8 : 4;
      p.nitems = (int)nwg;
      int relay_plain = (module != 2 && tall && r8 >= 6) ? 1 : 0;   // 2000^2 25.8 -> 25.1 us, 3000^2 50.1 -> 46.1
      // bit 1: stage priorities, where workgroups share SIMDs and the launch is a few rounds long (see the kernel; WDPM_RELAY_PRIO=0/2: never / always)
      if (sw.relay_prio == 2 || (sw.relay_prio == 1 && nwg > cus && (tall ? r8 : r4) <= 4)) relay_plain |= 2;
      if (no_clamp) relay_plain |= 4;        // bit 2: the clamped neighbour step is not exact on this DEM (see the kernel)
      p.relay_flags = p.ledger_sw = relay_plain;
      // the DEM as 32-bit codes from two rounds of workgroups on (700^2, one round: 7.05 against 7.5 us with the decode on the latency
      // path; 1200^2 11.7 -> 10.95, 1600^2 22.0 -> 20.2, 2400^2 42.9 -> 39.0; profiles/r03/relay_dem32_ab.txt)
      const bool dem32 = tall && module != 2 && q.codes32 && sw.relay_dem32 && (r8 >= 2 || q.force_codes);
      const int targs[6] = {m2, flush, plain, tall ? 8 : 4, dem32, 0};
      for (int k = 0; k < 6; k++) p.targs[k] = targs[k];
      return p;
    }
    // the block's last launch (max diff folded in) stays here where three rows per wave do (round 3); six-row waves have no
    // registers left for the snapshot's rows: those launches go to the marching kernel as before
    if (sw.tri && !signed_zero_safe && !(fold_md && two) && chunk_rows < 3 && (items <= tri_limit || sw.tri == 2)) {
      if (two) {
        nch = (out_last - A0 - 1 + 5) / 6;
        if (nch < 1) nch = 1;
        items = (long long)nstrips * nch;
      }
      p.family = WDPM_FAMILY_TRIANGLE;
      p.grid = ((unsigned)((items + 3) / 4) + 7) / 8 * 8;
      p.block = 256;
      p.wpb = 4;
      p.nitems = (int)items;
      const int targs[6] = {m2, flush, two ? 2 : 1, plain, fold_md, 0};
      for (int k = 0; k < 6; k++) p.targs[k] = targs[k];
      return p;
    }
  }

  p.family = WDPM_FAMILY_MARCHING;
  const bool fast = !signed_zero_safe;
  const int (&waves)[3] = dev.resident_waves[module == 2 ? 1 : 0];
  // add / subtract with an encodable DEM: 20 B per cell-update instead of 24 (drain: see big_drain below)
  // ... and only pays on launches big enough for two waves per SIMD (see below): at one wave per SIMD
  // the wave's own latency chain is the limit and the nine decodes per step cost 3-5 % (size sweep in
  // profiles/r01: 512^2 - 3072^2 slower with codes, 4096^2 and up 5-12 % faster).
  // Chunk height at two waves per SIMD from which a launch fills every slot: 18 rows (add / subtract), 12 (drain).  Rounds 1 - 3 had
  // 36 / 18; with the two waves of a SIMD keeping each other in step and chunk heights following the XCDs, the second wave pays on
  // shorter chunks: add 2700^2 +3.4 %, 3000^2 +6.7 %, 3300^2 +9.7 %, 3600^2 +2.6 %; drain 2400^2 +2.0 %, 3000^2 +1.1 %
  // (profiles/r04/tall_rows_sweep.txt).
  constexpr long long tall_add = 18, tall_drain = 12;
  const bool big = (long long)(out_last - A0 + 1) * nstrips >= tall_add * dev.resident_waves[0][0];
  // Drain with the codes (round 4, late): "latency-bound, the decode would only add instructions" was round 1's reading of a kernel
  // at one wave per SIMD; at two, and with the card at its power cap whatever the kernel does, four bytes per
  // cell-update less are worth more than the nine decodes of a step - on launches that fill every slot at two waves per SIMD.
  const bool big_drain = module == 2 && fast && (long long)(out_last - A0 + 1) * nstrips >= tall_drain * dev.resident_waves[1][1];
  const bool dem32 = fast && q.codes32 && ((module == 2 ? big_drain : big) || q.force_codes);
  bool two_per_simd = false;      /* every slot filled: two waves per SIMD, workgroups of eight waves (one per CU) */
  int slots = !fast ? waves[2] : dem32 ? waves[1] : waves[0];
  {
    // (Round 1, fp64 DEM:) the kernel is bound by the memory system with ONE wave per SIMD already; a second wave per SIMD only adds
    // concurrent DRAM row streams and, on rasters too small to fill the chip, makes the dispatcher
    // double up waves on some SIMDs while others idle.  Filling half of the resident slots measured
    // +4 % at 16384^2, +13 % at 6000^2, x1.9 at 1500^2, x2.3 at 1024^2 (-4 % at 4096^2).
    // The drain variant is different: 16 instructions per neighbour step on one dependent chain per
    // lane leave it latency-bound (59 % VALU issue at one wave per SIMD), and a second wave per SIMD
    // fills the bubbles: +21 % at 8192^2, +30 % at 16384^2 - as long as the chunks stay tall enough
    // for the 6-row warm-up of each not to eat the gain.
    // With the DEM as 32-bit codes the add kernel is in the same position: fewer bytes, nine decodes
    // more per step - one wave per SIMD 1.34 ms per 16384^2 launch (no gain), two waves 1.23 ms.
    // Thresholds from tools/threshold_sweep.sh and tools/slab_sweep.sh (profiles/r01): chunk height at
    // two waves per SIMD >= 36 rows for the DEM-code add kernel (3072^2 still loses, 3600^2 gains 12 %),
    // >= 18 rows for drain (+11 % on a 1055 x 8190 slab, +15 % at 3072^2, a wash at 2048^2).
    if (dem32 && big) two_per_simd = true;
    if (module == 2 && fast && (long long)(out_last - A0 + 1) * nstrips >= tall_drain * slots) two_per_simd = true;
    if (!two_per_simd && !(module == 2 && !fast)) slots = slots / 2;      /* (the -0.0-safe drain variant is built for one wave per SIMD) */
    if (q.leave_cus > 0) {                             // room for somebody else's kernels (see LaunchRequest)
      const int cus = dev.cus;
      if (q.leave_cus < cus / 2) slots = (int)((long long)slots * (cus - q.leave_cus) / cus);
    }
  }
  const int wrows = out_last - A0 + 1;                       // rows of this launch's window
  const int H = wdpm_chunk_rows(wrows, nstrips, chunk_rows, slots, sw.chunk_rows);
  // chunk i stores rows [A0+H*i+2 (0 for A0+H*i = 0), A0+H*(i+1)+1]; the last must reach out_last
  int nchunks = (out_last - A0 - 1 + H - 1) / H;
  if (nchunks < 1) nchunks = 1;
  int nitems = nstrips * nchunks;
  const int wpb = two_per_simd ? 8 : 4;                            // waves per workgroup (see the kernel: `prio`)
  unsigned grid = ((nitems + wpb - 1) / wpb + 7) / 8 * 8;         // multiple of 8: see the XCD remap
  // dry-tile flags (wdpm_kernels.h::TileFlags): whole-slab launches of chunks of two row triples at least, where no -0.0 exists
  p.tiles_fit = q.tiles_offered && q.tile_capacity > 0 && fast && H >= 6 && A0 == 0 && out_last == q.g.rows - 1 &&
                (nstrips + 2) * (nchunks + 2) <= q.tile_capacity;
  p.keep_tiles = p.tiles_fit && !fold_md;   /* max diff: every wave must look at its block: no skipping in this launch */
  // Chunk heights by what each XCD delivers (wdpm_kernels.h::XcdBalance): whole-slab launches of two waves per SIMD that keep no
  // dry-tile flags.  Every launch may be measured (the block's first and last are other instantiations: not those); the table
  // needs chunks of a dozen rows at least, so that whole row triples can follow weights a few per cent apart.
  const bool bal_forced = q.balance_mode == 2;          /* tests: the table on launches of any size, from skewed weights */
  p.steady = !flush && !fold_md;
  if (q.balance_mode && (two_per_simd || bal_forced) && A0 == 0 && out_last == q.g.rows - 1 && (chunk_rows < 3 || bal_forced) && nchunks >= 2) {
    p.balance = true;
    const bool can_table = !p.keep_tiles && H >= (bal_forced ? 6 : 12) && (nchunks + 1) * nstrips <= q.balance_capacity;
    // Round 5: with the table in charge a strip's chunks need not be equally tall, so a strip is cut into as many chunks as the
    // resident round has slots for - equal heights in whole triples left slots empty (the 8-GPU drain slab, 1055 x 8190: 27-row
    // chunks, 39 x 48 = 1872 waves on 2048 slots) - and the table pairs tall chunks with short ones on every SIMD (`pair` in
    // xcd_rebalance_kernel).  WDPM_PAIR=0: round 4's geometry (A/B, tests).
    // (WDPM_PAIR=2, tests: also on forced tables and launches of one wave per SIMD, down to the table's minimum of two triples a chunk)
    const int pair = ((wpb == 8 && !bal_forced && sw.pair != 0) || sw.pair == 2) ? 1 : 0;
    if (can_table && pair) {
      const int T = (out_last - 1 - A0 + 2) / 3, nc = slots / nstrips;
      if (nc > nchunks && T / nc >= (sw.pair == 2 ? 2 : 4) && (nc + 1) * nstrips <= q.balance_capacity) {
        nchunks = nc;
        nitems = nstrips * nchunks;
        grid = ((nitems + wpb - 1) / wpb + 7) / 8 * 8;
      }
    }
    p.pair = pair;
    p.ipx = wpb * (int)(grid / 8);
    p.table = can_table;
    p.rot = sw.rot != 0;
    // equal heights (a block that keeps dry-tile flags): what the XCDs deliver can be learnt there already
    p.measure_equal = !can_table && p.steady && H >= 12;
  }
  p.grid = grid;
  p.block = 64 * wpb;
  p.nchunks = nchunks;
  p.nitems = nitems;
  p.H = H;
  p.wpb = wpb;
  // Workgroups per CU, whatever the register allocator ends up with (an instantiation at 166 VGPRs would let the dispatcher stack
  // three four-wave workgroups on some CUs and one on others): unused dynamic LDS beside the 36 KiB of staging - four-wave
  // workgroups 36 KiB (two fit a CU's 160 KiB, three do not), eight-wave workgroups 48 KiB (one fits).
  // The pad follows the CU's LDS (not a constant tied to one architecture): an eight-wave workgroup takes just over half
  // of it, a four-wave one just over a third; 160 KiB on gfx950: 45 KiB and 18 KiB beside the 36 KiB of staging.
  const int staging = 8 * 3 * kStripIn * (int)sizeof(double) + 64;
  const int share = dev.lds_per_cu / (wpb == 8 ? 2 : 3) + 1024;
  p.lds = share > staging ? (unsigned)(share - staging) : 0u;
  // the two waves of a SIMD keep each other in step (see the marching loop); WDPM_PRIO=0: no priorities (A/B, tests)
  p.prio = (wpb == 8 && sw.prio != 0) ? 1 : 0;
  p.ledger_sw = (no_clamp ? WDPM_LEDGER_NO_CLAMP : 0) | (p.prio ? WDPM_LEDGER_PRIO : 0) | (p.keep_tiles ? WDPM_LEDGER_TILE_FLAGS : 0) |
                (p.table ? WDPM_LEDGER_BALANCE : 0);
  // <module, -0.0-safe, DEM codes, flush on load, max diff folded in, gate-free>: which instantiation runs is decided here and
  // nowhere else (DESIGN.md §4 has the table)
  // the codes as 16-bit offsets (18.1 B of HBM traffic per cell-update) on launches of 10^8 cells and more: wdpm_dem16_pays
  const bool dem16 = dem32 && q.codes16 && wdpm_dem16_pays((long long)wrows * q.g.ncp, q.force_codes);
  const int targs[6] = {m2, !fast, dem16 ? 2 : dem32 ? 1 : 0, flush, fold_md, plain};
  for (int k = 0; k < 6; k++) p.targs[k] = targs[k];
  return p;
}

/* groups of kGroupOut stored columns that cover ncp padded columns */
inline int wdpm_groups(const int ncp) {
  const int first = kGroupIn - kGroupHaloR;                // columns the first group covers (it stores from column 0)
  return ncp <= first ? 1 : (ncp - first + kGroupOut - 1) / kGroupOut + 1;
}

/* Launches from which two iterations per launch pay (WDPM_ITER2=1), in cells.  The sweep over the shapes that matter, forced against
 * the parent's single launches (profiles/r06/ab_shapes.txt, A/A spread 0.1 - 0.4 %): 4096^2 -1.0 %, the 2049 x 16384 add slab +9.2 %,
 * 8192^2 +3.7 %, 16384^2 +3.9 %.  The threshold sits just under the smallest shape measured ahead. */
constexpr long long kIter2MinCells = 30000000LL;

/* Two iterations in ONE marching launch (wdpm_march.hip::iter2_march), offered (LaunchPlan::iter2 == 1) or not (== 0: the caller
 * launches plan_iteration()'s plan).  `iterations_left`: launches like this one the caller still has to queue, this one included -
 * neither the block's first (flush) nor its last where that folds the max diff.  Offered only to the gate-free add / subtract
 * instantiations that stream the DEM as codes, on whole-slab steady launches of two waves per SIMD that keep no dry-tile flags and
 * have no chunk height of the caller's. */
inline LaunchPlan plan_iter2(const LaunchRequest &q, const DeviceFacts &dev, const Switches &sw, const int iterations_left) {
  LaunchPlan p = plan_iteration(q, dev, sw);
  p.iter2 = 0;
  if (p.error || sw.iter2 == 0 || iterations_left < 2) return p;
  if (p.family != WDPM_FAMILY_MARCHING || q.module == 2 || !p.steady || (p.wpb != 8 && sw.iter2 != 2)) return p;
  if (p.targs[0] != 0 || p.targs[1] != 0 || p.targs[2] == 0 || p.targs[3] != 0 || p.targs[4] != 0 || p.targs[5] != 1) return p;
  if (q.A0 != 0 || q.out_last != q.g.rows - 1 || q.chunk_rows >= 3 || sw.chunk_rows >= 3 || p.tiles_fit || q.leave_cus > 0) return p;
  if (sw.iter2 != 2 && (long long)q.g.rows * q.g.ncp < kIter2MinCells) return p;
  // LDS: the eight staging slices and the words of the single loop (static), the ring and its dump row (dynamic).  As deep a ring
  // as fits up to six row triples; one workgroup per CU needs more than half of the CU's LDS taken
  const int fixed = 8 * 3 * kStripIn * (int)sizeof(double) + 256;
  const int row_bytes = kRingPitch * (int)sizeof(double);
  int ring = ((dev.lds_per_cu - fixed) / row_bytes - 1) / 3 * 3;
  if (ring > 18) ring = 18;
  if (sw.iter2_ring >= 6 && sw.iter2_ring / 3 * 3 < ring) ring = sw.iter2_ring / 3 * 3;
  if (ring < 6) return p;
  int lds = (ring + 1) * row_bytes;
  const int half = dev.lds_per_cu / 2 + 1024 - fixed;
  if (lds < half) lds = half;
  const int rows = q.g.rows, ngroups = wdpm_groups(q.g.ncp);
  // one workgroup per CU, all resident together: chunks twice as tall as the single launch's
  int H = wdpm_chunk_rows(rows, ngroups, 0, dev.cus, 0);
  if (H < 6) H = 6;                                        // (forced on a small raster: fewer workgroups than CUs)
  int nchunks = (q.out_last - 1 + H - 1) / H;
  if (nchunks < 1) nchunks = 1;
  p.iter2 = 1;
  p.ring_rows = ring;
  p.iter2_prio = sw.iter2_prio != 0 ? 1 : 0;
  p.lds = (unsigned)lds;
  p.nstrips = ngroups;
  p.prio = 0;
  p.keep_tiles = false;
  // chunk heights by what each XCD delivers, as in the single launch: a table row per group
  const bool bal_forced = q.balance_mode == 2;
  p.balance = p.table = p.measure_equal = false;
  p.pair = 0;
  if (q.balance_mode && nchunks >= 2) {
    p.balance = true;
    const int T = (q.out_last - 1 + 2) / 3, nc = dev.cus / ngroups;
    bool can_table = H >= (bal_forced ? 6 : 12) && (nchunks + 1) * ngroups <= q.balance_capacity;
    if (can_table && !bal_forced && nc > nchunks && T / nc >= 4 && (nc + 1) * ngroups <= q.balance_capacity) nchunks = nc;
    p.table = can_table;
    p.rot = sw.rot != 0;
    p.measure_equal = !can_table && H >= 12;
  }
  p.nchunks = nchunks;
  p.nitems = ngroups * nchunks;
  p.grid = ((unsigned)p.nitems + 7) / 8 * 8;
  p.ipx = (int)(p.grid / 8);
  p.block = 512;
  p.H = H;
  p.ledger_sw = (p.no_clamp ? WDPM_LEDGER_NO_CLAMP : 0) | (p.iter2_prio ? WDPM_LEDGER_PRIO : 0) | (p.table ? WDPM_LEDGER_BALANCE : 0) | WDPM_LEDGER_ITER2;
  return p;
}

#endif /* WDPM_DISPATCH_H */
