/*
 * wdpm_catch_stitch.h — the host half of the pond catchments over row blocks (include/wdpm_group_pond_catchments.h): what ends
 * the descents that leave a rank's rows, and what makes the catchment table of the whole raster out of the ranks' own.  Plain
 * C++17 and nothing else, like wdpm_ponds_stitch.h and wdpm_rims_merge.h beside it: no HIP header, no getenv, no statics.
 * wdpm_pond_catchments.hip calls it between the ranks' jump rounds and their tally; tests/group_catch_emu_main.cpp holds it
 * against a plain loop over the whole raster without a GPU.
 *
 * Links.  After its jump rounds every owned cell of a rank holds a TERMINAL, an int32 below zero: pond k as -1 - k (k a label of
 * the whole raster), a pit as -1, a cell without a level as INT_MIN - and, where the descent left the rank's rows through a slope
 * cell of a neighbour's row, an EXIT that names (side, column): kExitBase + side * ncp + column, side 0 the row above the rank's
 * first owned row, side 1 the row below its last.  Exits lie in [INT_MIN + 1, INT_MIN + 2 * ncp] and pond codes reach down to
 * -1 - N, so the two never meet while N + 2 * ncp + 2 <= 2^31 (codes_fit; the caller refuses anything else before a link is
 * written).
 *
 * resolve.  An exit (side, column) of rank r is the cell `column` of the facing seam row of rank r -+ 1: the last owned row of the
 * rank above, the first owned row of the rank below.  That cell holds a pond, a pit or another exit - through its rank's far
 * boundary or back across the same one.  The seam cells are the nodes of a graph in which every node has at most one way out;
 * levels fall strictly along a descent, so it has no cycle.  Every chain is followed once, iteratively and with memoisation (a
 * chain can be as long as the seam cells are many), and a cycle ends as an error, never as a loop.
 */
#ifndef WDPM_CATCH_STITCH_H
#define WDPM_CATCH_STITCH_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/wdpm_pond_catchments.h"
#include "../../include/wdpm_ponds.h"

namespace wdpm_catch_stitch {

constexpr int kPit = -1;               /* pond k is -1 - k */
constexpr int kNone = INT_MIN;
constexpr int kExitBase = INT_MIN + 1;

/* pond codes and exit codes of a raster of ncp padded columns with `ponds` ponds lie apart */
inline bool codes_fit(long long ponds, long long ncp) { return ponds + 2 * ncp + 2 <= (1ll << 31); }
inline bool is_exit(int v, int ncp) { return v != kNone && v <= kExitBase + (2 * ncp - 1); }
inline int exit_code(int side, int col, int ncp) { return kExitBase + side * ncp + col; }

/* one rank as resolve sees it: the links of its first and of its last owned row after its jump rounds, ncp each.  A rank of one
 * owned row gives the same pointer twice. */
struct RankLinks {
  const int *top, *bottom;
};

struct Resolved {
  std::vector<std::vector<int>> exit_basin;   /* [rank][side * ncp + column]: where that exit ends - a pond, a pit; kNone where
                                                 the facing cell has no level or there is no rank on that side */
  long long crossings = 0;                    /* seam cells that held an exit: the nodes that were followed */
};

/* 0, or 1 with a message: a seam cell whose link is no terminal, an exit that leaves the raster, a cycle */
inline int resolve(const std::vector<RankLinks> &ranks, int ncp, Resolved &out, std::string &err) {
  const size_t nr = ranks.size(), row = (size_t)ncp;
  out = Resolved();
  out.exit_basin.assign(nr, std::vector<int>(2 * row, kNone));
  if (nr == 0 || ncp <= 0) return 0;
  /* node (rank, side, column); a rank whose two seam rows are one row (the same pointer, or one owned row) is read twice */
  auto link_of = [&](size_t node) {
    const size_t r = node / (2 * row), rest = node - r * 2 * row, side = rest / row, c = rest - side * row;
    return (side ? ranks[r].bottom : ranks[r].top)[c];
  };
  std::vector<unsigned char> state(nr * 2 * row, 0);      /* 0 new, 1 on the chain under way, 2 done */
  std::vector<int> fin(nr * 2 * row, kNone);
  std::vector<size_t> chain;
  /* the first rank's first owned row and the last rank's last one lie on no boundary: no exit leads there, and they are no nodes */
  auto on_boundary = [&](size_t node) {
    const size_t r = node / (2 * row), side = (node - r * 2 * row) / row;
    return side ? r + 1 < nr : r > 0;
  };
  for (size_t start = 0; start < state.size(); start++) {
    if (state[start] || !on_boundary(start)) continue;
    chain.clear();
    size_t cur = start;
    int end = kNone;
    for (;;) {
      if (state[cur] == 2) { end = fin[cur]; break; }
      if (state[cur] == 1) { err = "the descents across the row blocks form a cycle: levels must fall strictly"; return 1; }
      const int v = link_of(cur);
      if (v >= 0) { err = "a cell of a rank's first or last owned row is still on its way after the jump rounds"; return 1; }
      if (!is_exit(v, ncp)) { state[cur] = 2; fin[cur] = end = v; break; }
      const size_t r = cur / (2 * row);
      const int e = v - kExitBase, side = e / ncp, col = e - side * ncp;
      if (side ? r + 1 == nr : r == 0) { err = "a descent leaves the raster through its first or last row"; return 1; }
      state[cur] = 1;
      chain.push_back(cur);
      out.crossings++;
      cur = ((side ? r + 1 : r - 1) * 2 + (side ? 0 : 1)) * row + (size_t)col;      /* the facing row of the rank next door */
    }
    for (size_t node : chain) { fin[node] = end; state[node] = 2; }
  }
  for (size_t r = 0; r < nr; r++)
    for (size_t side = 0; side < 2; side++) {
      if (side ? r + 1 == nr : r == 0) continue;
      const size_t facing = ((side ? r + 1 : r - 1) * 2 + (side ? 0 : 1)) * row;
      for (size_t c = 0; c < row; c++) out.exit_basin[r][side * row + c] = fin[facing + c];
    }
  /* a rank whose first owned row is its last one shows each of its cells in two nodes: count them once */
  for (size_t r = 1; r + 1 < nr; r++)
    if (ranks[r].top == ranks[r].bottom)
      for (size_t c = 0; c < row; c++) out.crossings -= is_exit(ranks[r].top[c], ncp);
  return 0;
}

/* The ponds a rank's exits end in that it holds no table row for yet.  A rank holds a row for its local and its foreign ponds:
 * those with a cell in the rows of its view, [view_lo, view_hi] of the whole raster (its owned rows and the one beside either
 * end).  A pond is 8-connected, so it has a cell in every row from row_min to row_max of its row in the merged pond table, and is
 * held exactly when that range meets the view's: the work is in the few ponds the exits end in, not in the many the rank holds.
 * Sorted, each once; 2 * ncp at most. */
inline void remote_labels(const std::vector<int> &exit_basin, int ncp, const wdpm_pond *pond_table, int view_lo, int view_hi,
                          std::vector<int> &out) {
  out.clear();
  for (int v : exit_basin) {
    if (v >= kPit || v == kNone || is_exit(v, ncp)) continue;
    const wdpm_pond &p = pond_table[-2 - v];                /* pond k = -1 - v is row k - 1 */
    if (p.row_max < view_lo || p.row_min > view_hi) out.push_back(-1 - v);
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
}

/* one rank as the merge sees it */
struct RankCatch {
  const wdpm_pond_catchment *rows;   /* `slots` finished rows; row_min and row_max are local to the rank's view, the box of a slot */
                                     /* without catch_cells is empty (row_max < row_min) */
  const int *label;                  /* the pond's number in the whole raster, 1..ponds, of slots 0 .. slots - nremote - 1: the */
                                     /* rank's local and foreign ponds, as its rim rows name them (not copied for this) */
  long long slots;
  const int *remote;                 /* ... and of the last nremote slots: its remote ponds */
  long long nremote;
  int row_shift;                     /* the whole-raster row of the view's row 0 */
  long long slope, pit, unponded, exits, rounds;
};

struct Totals {
  long long slope = 0, pit = 0, unponded = 0, exits = 0, rounds = 0;
};

inline unsigned long long key_of(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

/* `whole` takes `ponds` rows, `pond_table` holds the merged pond table (each pond's own box); ranks in row order.  Every slope
 * cell was counted by the rank that owns it, so counts add; the head is the highest of the ranks' heads through the
 * order-preserving image; the box is the pond's own united with the ranks' boxes.  0, or 1 with a message: a label outside
 * 1..ponds, a negative count, a count that leaves int64. */
inline int merge(const std::vector<RankCatch> &ranks, long long ponds, const wdpm_pond *pond_table, wdpm_pond_catchment *whole,
                 Totals &tot, std::string &err) {
  tot = Totals();
  for (long long k = 0; k < ponds; k++) {
    wdpm_pond_catchment &t = whole[k];
    t.catch_cells = t.inflow_cells = 0;
    t.head_level = -INFINITY;
    t.row_min = pond_table[k].row_min;
    t.row_max = pond_table[k].row_max;
    t.col_min = pond_table[k].col_min;
    t.col_max = pond_table[k].col_max;
  }
  auto add = [&](long long &sum, long long v, const char *what) {
    if (v < 0) { err = std::string("a rank reports a negative count of ") + what; return 1; }
    if (v > INT64_MAX - sum) { err = std::string(what) + " summed over the row blocks overflows int64"; return 1; }
    sum += v;
    return 0;
  };
  for (const RankCatch &rk : ranks) {
    if (add(tot.slope, rk.slope, "slope_cells") || add(tot.pit, rk.pit, "pit_cells") || add(tot.unponded, rk.unponded, "unponded_cells") ||
        add(tot.exits, rk.exits, "exits"))
      return 1;
    tot.rounds = std::max(tot.rounds, rk.rounds);
    for (long long s = 0; s < rk.slots; s++) {
      const wdpm_pond_catchment &p = rk.rows[s];
      const long long held = rk.slots - rk.nremote, L = s < held ? rk.label[s] : rk.remote[s - held];
      if (L < 1 || L > ponds) { err = "a rank's catchment row names a pond outside the whole raster's table"; return 1; }
      wdpm_pond_catchment &t = whole[L - 1];
      if (p.catch_cells < 0 || p.inflow_cells < 0) { err = "a rank's catchment row holds a negative count"; return 1; }
      if (p.catch_cells > INT64_MAX - t.catch_cells) { err = "catch_cells of a pond summed over the row blocks overflows int64"; return 1; }
      if (p.inflow_cells > INT64_MAX - t.inflow_cells) { err = "inflow_cells of a pond summed over the row blocks overflows int64"; return 1; }
      t.inflow_cells += p.inflow_cells;
      if (p.catch_cells == 0) continue;                 /* nothing of the slot's head or box was ever sent */
      if (t.catch_cells == 0 || key_of(p.head_level) > key_of(t.head_level)) t.head_level = p.head_level;
      t.catch_cells += p.catch_cells;
      t.row_min = std::min(t.row_min, p.row_min + rk.row_shift);
      t.row_max = std::max(t.row_max, p.row_max + rk.row_shift);
      t.col_min = std::min(t.col_min, p.col_min);
      t.col_max = std::max(t.col_max, p.col_max);
    }
  }
  return 0;
}

}  // namespace wdpm_catch_stitch
#endif
