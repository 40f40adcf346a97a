/*
 * wdpm_rims_merge.h — the host half of the pond rims over row blocks (include/wdpm_group_pond_rims.h): what makes the rim table
 * of the whole raster out of the ranks' own.  Plain C++17 and nothing else, like wdpm_ponds_stitch.h beside it: no HIP header,
 * no getenv, no statics.  wdpm_pond_rims.hip calls it after the ranks' rim rows have come down; tests/group_rims_emu_main.cpp
 * holds it against a plain loop over the whole raster without a GPU.
 *
 * Every rank has taken the rim of its owned rows: one finished wdpm_pond_rim per SLOT, a slot being a pond of the whole raster
 * the rank touches - with its cells, or only with dry cells next to a pond that lives in the rows of a neighbour (a foreign
 * pond: no surface, so surface_min / surface_max are still what no cell ever lowered or raised).  A slot nothing was sent to
 * changes nothing here.  Every cell was counted by exactly one rank, so counts add and extremes are extremes of extremes,
 * compared through the order-preserving image of a double the device uses (-0.0 below +0.0).  A rank's rim cell is the one
 * with the smallest index among those at ITS lowest level; ranks are in row order, so the first rank whose lowest level is the
 * lowest of all holds the cell with the smallest index of the whole raster.
 */
#ifndef WDPM_RIMS_MERGE_H
#define WDPM_RIMS_MERGE_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/wdpm_pond_rims.h"

namespace wdpm_rims_merge {

/* one rank as the merge sees it */
struct RankRims {
  const wdpm_pond_rim *rows;   /* `slots` finished rows; rim_row and rim_col are local to the rank's view, -1 without a rim cell */
  const int *label;            /* label[slot]: the pond's number in the whole raster, 1..ponds */
  long long slots;
  int row_shift;               /* the whole-raster row of the view's row 0 */
};

inline unsigned long long key_of(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double from_key(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  memcpy(&v, &b, 8);
  return v;
}

/* `whole` takes `ponds` rows; ranks in row order.  0, or 1 with a message: a label outside 1..ponds, a negative count, or a
 * count that leaves int64. */
inline int merge(const std::vector<RankRims> &ranks, long long ponds, wdpm_pond_rim *whole, std::string &err) {
  for (long long k = 0; k < ponds; k++) {
    wdpm_pond_rim &t = whole[k];
    t.surface_min = from_key(~0ull);          /* what the device's table starts from */
    t.surface_max = from_key(0ull);
    t.rim_level = INFINITY;
    t.rim_row = t.rim_col = -1;
    t.rim_cells = t.wall_cells = 0;
  }
  for (const RankRims &rk : ranks)
    for (long long s = 0; s < rk.slots; s++) {
      const wdpm_pond_rim &p = rk.rows[s];
      const long long L = rk.label[s];
      if (L < 1 || L > ponds) { err = "a rank's rim row names a pond outside the whole raster's table"; return 1; }
      wdpm_pond_rim &t = whole[L - 1];
      if (key_of(p.surface_min) < key_of(t.surface_min)) t.surface_min = p.surface_min;
      if (key_of(p.surface_max) > key_of(t.surface_max)) t.surface_max = p.surface_max;
      /* a later rank takes the rim cell only with a strictly lower level: of equals the upper rank's cell has the smaller index */
      if (p.rim_row >= 0 && (t.rim_row < 0 || key_of(p.rim_level) < key_of(t.rim_level))) {
        t.rim_level = p.rim_level;
        t.rim_row = p.rim_row + rk.row_shift;
        t.rim_col = p.rim_col;
      }
      if (p.rim_cells < 0 || p.wall_cells < 0) { err = "a rank's rim row holds a negative count"; return 1; }
      if (p.rim_cells > INT64_MAX - t.rim_cells) { err = "rim_cells of a pond joined across row blocks overflows int64"; return 1; }
      if (p.wall_cells > INT64_MAX - t.wall_cells) { err = "wall_cells of a pond joined across row blocks overflows int64"; return 1; }
      t.rim_cells += p.rim_cells;
      t.wall_cells += p.wall_cells;
    }
  return 0;
}

/* The whole-raster labels in the rows beside a rank's own that none of the rank's cells carries: `beside` holds those two rows'
 * labels one after the other (2 * ncp, or ncp at either end of the raster), `own_seams` the rank's own first and last owned row
 * likewise.  A pond with cells on both sides of a boundary has cells in both rows next to it, so a label of `beside` is foreign
 * exactly when `own_seams` lacks it.  Sorted, each once. */
inline void foreign_labels(const int *beside, size_t nbeside, const int *own_seams, size_t nown, std::vector<int> &out) {
  std::vector<int> own;
  for (size_t i = 0; i < nown; i++)
    if (own_seams[i] && (own.empty() || own.back() != own_seams[i])) own.push_back(own_seams[i]);
  std::sort(own.begin(), own.end());
  out.clear();
  for (size_t i = 0; i < nbeside; i++)
    if (beside[i] && (out.empty() || out.back() != beside[i]) && !std::binary_search(own.begin(), own.end(), beside[i]))
      out.push_back(beside[i]);
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
}

}  // namespace wdpm_rims_merge
#endif
