/*
 * wdpm_curves_merge.h — the host half of the pond stage curves over row blocks (include/wdpm_group_pond_curves.h): what makes the
 * curve table of the whole raster out of the ranks' own.  Plain C++17 and nothing else, like wdpm_ponds_stitch.h, wdpm_rims_merge.h,
 * wdpm_catch_stitch.h and wdpm_outlets_merge.h beside it: no HIP header, no getenv, no statics.  wdpm_pond_curves.hip calls `bed`
 * between the ranks' bed pass and their stage pass and `merge` after it; tests/group_curves_emu_main.cpp holds both against a plain
 * loop over all cells and stages of the whole raster without a GPU.
 *
 * A rank holds one table row per SLOT: its local and foreign ponds as the rim rows name them, then its remote ponds
 * (wdpm_catch_stitch.h); every basin > 0 of its owned rows has one.  The bed of a basin is the lowest ground over ALL ranks and every
 * stage height depends on it: `bed` takes the minimum of the ranks' keys (the order-preserving image of a double, ~0 where a rank
 * holds no cell of the basin) and hands every rank its slots' final keys.  The key is turned into a double here, once per pond, and
 * nowhere before.  After the stage pass the ranks' sixteen counts and sixteen sums of a pond add up: every cell was counted once, by
 * its owner, against the same sixteen heights.
 */
#ifndef WDPM_CURVES_MERGE_H
#define WDPM_CURVES_MERGE_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/wdpm_pond_curves.h"

namespace wdpm_curves_merge {

constexpr unsigned long long kNoBed = ~0ull;       /* no cell of the basin seen */

/* a slot's row as a rank's stage pass leaves it: the layout the device accumulates in */
struct SlotRow {
  unsigned long long bed_key;        /* the merged key, as it went up */
  double top_level;                  /* the merged pour level of the slot's pond, +inf without an outlet */
  unsigned long long cells[WDPM_CURVE_STAGES], q[WDPM_CURVE_STAGES];
};
static_assert(sizeof(SlotRow) == sizeof(wdpm_pond_curve), "a slot's row lies as a table row does");

inline double level_from_key(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &b, 8);
  return v;
}

/* one rank as both functions see it */
struct Rank {
  const int *label;                  /* the pond's number in the whole raster, 1..ponds, of slots 0 .. slots - nremote - 1 */
  long long slots;
  const int *remote;                 /* ... and of the last nremote slots */
  long long nremote;
  const unsigned long long *key;     /* per slot, after the bed pass: the rank's own lowest ground of the basin, kNoBed without a cell */
  const SlotRow *rows;               /* per slot, after the stage pass (merge only) */
};

inline long long label_of(const Rank &rk, long long s) {
  const long long held = rk.slots - rk.nremote;
  return s < held ? rk.label[s] : rk.remote[s - held];
}

/* Between the bed pass and the stage pass.  bed_key takes `ponds` entries: the lowest key over the ranks.  up[rank] takes the final
 * key of each of the rank's slots.  split_basins: the ponds for which more than one rank offered a key.  0, or 1 with a message. */
inline int bed(const std::vector<Rank> &ranks, long long ponds, unsigned long long *bed_key, std::vector<unsigned long long *> &up,
               long long &split_basins, std::string &err) {
  std::vector<int> offers((size_t)ponds, 0);
  for (long long k = 0; k < ponds; k++) bed_key[k] = kNoBed;
  for (const Rank &rk : ranks)
    for (long long s = 0; s < rk.slots; s++) {
      const long long L = label_of(rk, s);
      if (L < 1 || L > ponds) { err = "a rank's curve row names a pond outside the whole raster's table"; return 1; }
      if (rk.key[s] == kNoBed) continue;
      offers[(size_t)(L - 1)]++;
      if (rk.key[s] < bed_key[L - 1]) bed_key[L - 1] = rk.key[s];
    }
  split_basins = 0;
  for (long long k = 0; k < ponds; k++) {
    if (bed_key[k] == kNoBed) { err = "a pond has no bed: no rank holds a cell of its basin"; return 1; }
    split_basins += offers[(size_t)k] > 1;
  }
  for (size_t r = 0; r < ranks.size(); r++)
    for (long long s = 0; s < ranks[r].slots; s++) up[r][s] = bed_key[label_of(ranks[r], s) - 1];
  return 0;
}

/* what the merge counts: the four of wdpm_pond_curve_stats, then the group's own */
struct Totals {
  long long ponds = 0, no_curve = 0, flat = 0, stage_cells = 0;
  long long remote_beds = 0;         /* ponds that have stage cells on a rank other than the lowest rank holding the bed */
};

/* After the stage pass.  `whole` takes `ponds` rows, whatever they held; bed_key is what `bed` gave; ranks in row order, their `key`
 * still what came down after the bed pass.  0, or 1 with a message: a sum that leaves 64 bits, two ranks that disagree about a pond's top level. */
inline int merge(const std::vector<Rank> &ranks, long long ponds, const unsigned long long *bed_key, wdpm_pond_curve *whole, Totals &tot,
                 std::string &err) {
  tot = Totals();
  tot.ponds = ponds;
  std::vector<unsigned char> seen((size_t)ponds, 0), bed_found((size_t)ponds, 0), away((size_t)ponds, 0);
  for (const Rank &rk : ranks) {
    for (long long s = 0; s < rk.slots; s++) {
      const long long L = label_of(rk, s);
      if (L < 1 || L > ponds) { err = "a rank's curve row names a pond outside the whole raster's table"; return 1; }
      const SlotRow &p = rk.rows[s];
      wdpm_pond_curve &t = whole[L - 1];
      const bool first = !seen[(size_t)(L - 1)];
      if (first) {                                        /* a pond's row is written once and then added to: no pass over the table before */
        seen[(size_t)(L - 1)] = 1;
        t.bed_level = level_from_key(bed_key[L - 1]);
        t.top_level = p.top_level;
      } else if (memcmp(&t.top_level, &p.top_level, 8) != 0) {
        err = "two ranks hold different top levels for one pond";
        return 1;
      }
      /* the lowest rank that holds the bed: ranks come in row order, and the first whose own key is the merged one is it */
      const bool holds_bed = rk.key[s] == bed_key[L - 1];
      const bool first_holder = holds_bed && !bed_found[(size_t)(L - 1)];
      if (first_holder) bed_found[(size_t)(L - 1)] = 1;
      const bool curve = t.top_level < INFINITY;          /* no outlet: the bed, and zeros */
      if (curve && p.cells[WDPM_CURVE_STAGES - 1] != 0ull && !first_holder) away[(size_t)(L - 1)] = 1;
      for (int st = 0; st < WDPM_CURVE_STAGES; st++) {
        const unsigned long long c = curve ? p.cells[st] : 0ull, q = curve ? p.q[st] : 0ull;
        if (first) {
          if (c > (unsigned long long)INT64_MAX) { err = "cells of a pond's stage summed over the row blocks overflows int64"; return 1; }
          t.cells[st] = (long long)c;
          t.q[st] = q;
          continue;
        }
        if (c > (unsigned long long)(INT64_MAX - t.cells[st])) { err = "cells of a pond's stage summed over the row blocks overflows int64"; return 1; }
        if (q > UINT64_MAX - t.q[st]) { err = "q of a pond's stage summed over the row blocks overflows 64 bits"; return 1; }
        t.cells[st] += (long long)c;
        t.q[st] += q;
      }
    }
  }
  for (long long k = 0; k < ponds; k++) {
    const wdpm_pond_curve &t = whole[k];
    if (!seen[(size_t)k]) { err = "a pond has no curve row on any rank"; return 1; }
    if (!(t.top_level < INFINITY)) {
      tot.no_curve++;
      continue;
    }
    tot.flat += t.top_level == t.bed_level;
    if (t.cells[WDPM_CURVE_STAGES - 1] > INT64_MAX - tot.stage_cells) { err = "the stage cells summed over the ponds overflow int64"; return 1; }
    tot.stage_cells += t.cells[WDPM_CURVE_STAGES - 1];
    tot.remote_beds += away[(size_t)k];
  }
  return 0;
}

}  // namespace wdpm_curves_merge
#endif
