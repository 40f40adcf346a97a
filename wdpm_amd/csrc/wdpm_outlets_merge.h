/*
 * wdpm_outlets_merge.h — the host half of the pond outlets over row blocks (include/wdpm_group_pond_outlets.h): what makes the
 * outlet table of the whole raster out of the ranks' own.  Plain C++17 and nothing else, like wdpm_ponds_stitch.h,
 * wdpm_rims_merge.h and wdpm_catch_stitch.h beside it: no HIP header, no getenv, no statics.  wdpm_pond_outlets.hip calls `pour`
 * between the ranks' passes and their locate pass and `merge` after it; tests/group_outlets_emu_main.cpp holds both against a
 * plain loop over all pairs of the whole raster without a GPU.
 *
 * A rank owns every pass (a, b) whose a lies in its owned rows and holds one table row per SLOT: its local and foreign ponds as the
 * rim rows name them, then its remote ponds (wdpm_catch_stitch.h).  The pour level of a pond is the lowest of the ranks' lowest
 * passes and must be known before a cell is filled or a pair offered: `pour` takes the minimum of the ranks' keys (the
 * order-preserving image of a double, ~0 where a rank saw no pass) and hands every rank its slots' final keys.  After the locate
 * pass every rank whose own minimum equals that key has offered its first pair as view_index * 8 + direction; the lowest rank
 * that offered wins, which is the smallest whole-raster index since ranks own ascending rows.
 */
#ifndef WDPM_OUTLETS_MERGE_H
#define WDPM_OUTLETS_MERGE_H

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/wdpm_pond_outlets.h"

namespace wdpm_outlets_merge {

constexpr unsigned long long kNone = ~0ull;        /* no pour key, no pair */

/* a slot's row as a rank's locate pass and its finish leave it: the layout the device accumulates in */
struct SlotRow {
  unsigned long long pour_key, pair, spare;
  int to_basin, reserved;
  unsigned long long divide_cells, fill_cells, fill_q;
};
static_assert(sizeof(SlotRow) == sizeof(wdpm_pond_outlet), "a slot's row lies as a table row does");

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
  const unsigned long long *key;     /* per slot, after the passes: the rank's lowest pass, kNone without one */
  const unsigned long long *divide;  /* per slot: the rank's owned cells that stand in a pass */
  const SlotRow *rows;               /* per slot, after locate and finish (merge only) */
  int row_shift;                     /* the whole-raster row of the view's row 0 */
  int own_lo, own_rows;              /* the rank's owned rows, whole-raster */
};

inline long long label_of(const Rank &rk, long long s) {
  const long long held = rk.slots - rk.nremote;
  return s < held ? rk.label[s] : rk.remote[s - held];
}

/* Between the passes and the locate pass.  pour_key and divide take `ponds` entries: the lowest key over the ranks, the divide
 * cells added up (each cell a was counted once, by its owner).  up[rank] takes the final key of each of the rank's slots.  0, or 1
 * with a message. */
inline int pour(const std::vector<Rank> &ranks, long long ponds, unsigned long long *pour_key, long long *divide,
                std::vector<unsigned long long *> &up, std::string &err) {
  for (long long k = 0; k < ponds; k++) {
    pour_key[k] = kNone;
    divide[k] = 0;
  }
  for (const Rank &rk : ranks)
    for (long long s = 0; s < rk.slots; s++) {
      const long long L = label_of(rk, s);
      if (L < 1 || L > ponds) { err = "a rank's outlet row names a pond outside the whole raster's table"; return 1; }
      if (rk.key[s] < pour_key[L - 1]) pour_key[L - 1] = rk.key[s];
      if (rk.divide[s] > (unsigned long long)(INT64_MAX - divide[L - 1])) { err = "divide_cells of a pond summed over the row blocks overflows int64"; return 1; }
      divide[L - 1] += (long long)rk.divide[s];
    }
  for (size_t r = 0; r < ranks.size(); r++)
    for (long long s = 0; s < ranks[r].slots; s++) up[r][s] = pour_key[label_of(ranks[r], s) - 1];
  return 0;
}

/* what the merge counts: the four of wdpm_pond_outlet_stats, then the group's own */
struct Totals {
  long long ponds = 0, no_outlet = 0, to_land = 0, divide_cells = 0;
  long long seam_outlets = 0;        /* ponds whose outlet pair (a, b) lies in two ranks' rows */
  long long split_ponds = 0;         /* ponds for which more than one rank held divide or fill cells */
};

/* After the locate pass.  `whole` takes `ponds` rows; pour_key and divide are what `pour` gave; ranks in row order.  0, or 1 with a
 * message: a sum that leaves 64 bits, a pour level no rank found the pass of. */
inline int merge(const std::vector<Rank> &ranks, long long ponds, int ncp, const unsigned long long *pour_key, const long long *divide,
                 wdpm_pond_outlet *whole, Totals &tot, std::string &err) {
  tot = Totals();
  tot.ponds = ponds;
  std::vector<int> holders((size_t)ponds, 0);
  std::vector<unsigned char> won((size_t)ponds, 0);
  for (long long k = 0; k < ponds; k++) {
    wdpm_pond_outlet &t = whole[k];
    t.pour_level = INFINITY;
    t.from_row = t.from_col = t.to_row = t.to_col = -1;
    t.to_basin = -1;
    t.reserved = 0;
    t.divide_cells = t.fill_cells = 0;
    t.fill_q = 0;
  }
  for (const Rank &rk : ranks)
    for (long long s = 0; s < rk.slots; s++) {
      const long long L = label_of(rk, s);
      if (L < 1 || L > ponds) { err = "a rank's outlet row names a pond outside the whole raster's table"; return 1; }
      const SlotRow &p = rk.rows[s];
      wdpm_pond_outlet &t = whole[L - 1];
      if (pour_key[L - 1] == kNone) continue;             /* no pass anywhere: nothing was filled, nothing offered */
      if (rk.divide[s] != 0ull || p.fill_cells != 0ull) holders[(size_t)(L - 1)]++;
      if (p.fill_cells > (unsigned long long)(INT64_MAX - t.fill_cells)) { err = "fill_cells of a pond summed over the row blocks overflows int64"; return 1; }
      if (p.fill_q > UINT64_MAX - t.fill_q) { err = "fill_q of a pond summed over the row blocks overflows 64 bits"; return 1; }
      t.fill_cells += (long long)p.fill_cells;
      t.fill_q += p.fill_q;
      if (p.pair == kNone || won[(size_t)(L - 1)]) continue;
      won[(size_t)(L - 1)] = 1;                           /* the lowest rank that offered: the smallest whole-raster index */
      const long long from = (long long)(p.pair >> 3);
      const int i8 = (int)(p.pair & 7ull);
      const int dr = (i8 < 3 ? -1 : i8 < 5 ? 0 : 1), dc = (i8 < 3 ? i8 - 1 : i8 == 3 ? -1 : i8 == 4 ? 1 : i8 - 6);
      const int row = (int)(from / ncp), col = (int)(from - (long long)row * ncp);
      t.from_row = row + rk.row_shift;
      t.from_col = col;
      t.to_row = t.from_row + dr;
      t.to_col = col + dc;
      t.to_basin = p.to_basin;
      if (t.to_row < rk.own_lo || t.to_row >= rk.own_lo + rk.own_rows) tot.seam_outlets++;
    }
  for (long long k = 0; k < ponds; k++) {
    wdpm_pond_outlet &t = whole[k];
    if (pour_key[k] == kNone) {
      tot.no_outlet++;
      continue;
    }
    if (!won[(size_t)k]) { err = "a pond has a pour level and no rank found the pass that gives it"; return 1; }
    t.pour_level = level_from_key(pour_key[k]);
    t.divide_cells = divide[k];
    if (t.divide_cells > INT64_MAX - tot.divide_cells) { err = "divide_cells summed over the ponds overflows int64"; return 1; }
    tot.divide_cells += t.divide_cells;
    tot.to_land += t.to_basin == 0;
    tot.split_ponds += holders[(size_t)k] > 1;
  }
  return 0;
}

}  // namespace wdpm_outlets_merge
#endif
