/*
 * wdpm_route_plan.h — which launches sweep the levels of the pond routing (include/wdpm_pond_routing.h), decided on the host from
 * the offsets of the ponds sorted by level.  Plain C++, no HIP, in the manner of wdpm_dispatch.h: wdpm_pond_routing.hip launches
 * what this returns, tests/route_plans_main.cpp prints it for level sizes made up directly.
 *
 * Level l holds the ponds order[offsets[l] .. offsets[l + 1]), l = hops.  A pond of level l spills into one of level l - 1, so the
 * sweep runs from the deepest level down to level 0, and a level starts only when the one above it has ended:
 *   wide    a level of more ponds than `narrow` (at most kRouteBlock, one workgroup): one grid launch of its own
 *   run     consecutive levels of at most `narrow` ponds each: ONE launch of a single workgroup, which walks them with a block
 *           barrier in between; at most `run_levels` levels to a run, so that no kernel runs long
 * The trip count of a run is decided here; nothing on the device waits for a condition or for another workgroup.
 */
#ifndef WDPM_ROUTE_PLAN_H
#define WDPM_ROUTE_PLAN_H

#include <cstdlib>
#include <vector>

constexpr int kRouteBlock = 256;           /* threads of a workgroup of the sweep: kBlock of wdpm_ponds_priv.h */
constexpr int kRouteRunLevels = 65536;     /* levels one run walks at most */

/* levels top, top - 1, ..., top - levels + 1, in that order; a wide launch holds one level */
struct RouteLaunch {
  int top, levels;
  bool wide;
  int first, count;                        /* wide: the level's ponds are order[first .. first + count) */
};

struct RoutePlan {
  std::vector<RouteLaunch> launches;
  long long wide_levels = 0;
};

/* a bound from the environment (WDPM_ROUTE_NARROW, WDPM_ROUTE_RUN_LEVELS): what the text says where it lies in [lo, hi], else dflt */
inline int route_bound(const char *text, int lo, int hi, int dflt) {
  if (!text || !*text) return dflt;
  const long v = atol(text);
  return v >= lo && v <= hi ? (int)v : dflt;
}

/* offsets: levels + 1 values, offsets[0] == 0, never falling */
inline RoutePlan route_plan(const int *offsets, int levels, int narrow, int run_levels) {
  RoutePlan p;
  if (narrow < 1 || narrow > kRouteBlock) narrow = kRouteBlock;
  if (run_levels < 1) run_levels = kRouteRunLevels;
  for (int l = levels - 1; l >= 0; l--) {
    const int first = offsets[l], count = offsets[l + 1] - offsets[l];
    if (count > narrow) {
      p.launches.push_back(RouteLaunch{l, 1, true, first, count});
      p.wide_levels++;
    } else if (!p.launches.empty() && !p.launches.back().wide && p.launches.back().levels < run_levels) {
      p.launches.back().levels++;
    } else {
      p.launches.push_back(RouteLaunch{l, 1, false, 0, 0});
    }
  }
  return p;
}

#endif
