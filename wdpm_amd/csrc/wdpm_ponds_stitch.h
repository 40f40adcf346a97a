/*
 * wdpm_ponds_stitch.h — the host half of the pond inventory over row blocks (include/wdpm_group_ponds.h): what joins the ranks'
 * own inventories into the inventory of the whole raster.  Plain C++17 and nothing else: no HIP header, no getenv, no statics.
 * wdpm_ponds.hip calls it between the ranks' scan and their table kernels; tests/group_ponds_emu_main.cpp holds it against a
 * flood fill of the whole raster without a GPU.
 *
 * Every rank has labelled its owned rows by itself: local labels 1..n in first-cell order, and the labels of its first and of
 * its last owned row (ncp int32 each, 0 = no pond).  Ranks are in row order, so the whole raster's numbering by first cell is
 * the concatenation of the ranks' numberings with every pond struck out that is joined, across some boundary, to a pond that
 * begins earlier; a struck-out pond takes the number of the first member of its set.  Only labels that occur in a seam row can
 * be joined, so the union-find runs over those and every other label is numbered by counting.
 */
#ifndef WDPM_PONDS_STITCH_H
#define WDPM_PONDS_STITCH_H

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/wdpm_ponds.h"

namespace wdpm_stitch {

/* one rank as the stitch sees it; `top` is unused for the first rank and `bottom` for the last one (may be null there) */
struct RankSeams {
  long long n;          /* local ponds */
  const int *top;       /* local labels of the first owned row */
  const int *bottom;    /* local labels of the last owned row */
};

struct Result {
  std::vector<std::vector<int>> map;   /* map[rank][local label - 1] = label in the whole raster */
  long long ponds = 0;                 /* N of the whole raster */
  long long local_ponds = 0;           /* sum of the ranks' own counts */
  long long unions = 0;                /* pairs of touching runs across a row-block boundary (8-connectivity), each joined */
  long long merged = 0;                /* local ponds that gave up their number: ponds == local_ponds - merged */
};

namespace detail {

struct Run { int s, e, label; };   /* columns [s, e) */

inline void runs_of(const int *row, int ncp, std::vector<Run> &out) {
  out.clear();
  for (int c = 0; c < ncp;) {
    if (!row[c]) { c++; continue; }
    int e = c + 1;
    while (e < ncp && row[e]) e++;
    out.push_back({c, e, row[c]});
    c = e;
  }
}

inline long long find(std::vector<long long> &parent, long long x) {
  while (parent[x] != x) {
    parent[x] = parent[parent[x]];
    x = parent[x];
  }
  return x;
}

}  // namespace detail

/* 0, or 1 with a message: a label outside 1..n in a seam row, or 2^31 ponds and more in the whole raster */
inline int stitch(const std::vector<RankSeams> &ranks, int ncp, Result &out, std::string &err) {
  using namespace detail;
  const size_t nr = ranks.size();
  out = Result();
  out.map.resize(nr);
  /* the nodes: (rank, label) for the labels of the seam rows, in that order - which is first-cell order */
  std::vector<std::vector<int>> seam(nr);
  std::vector<long long> first(nr + 1, 0);
  for (size_t r = 0; r < nr; r++) {
    if (ranks[r].n < 0) { err = "a rank reports a negative number of ponds"; return 1; }
    std::vector<int> &s = seam[r];
    for (int side = 0; side < 2; side++) {
      const int *row = side ? ranks[r].bottom : ranks[r].top;
      if ((side ? r + 1 == nr : r == 0) || !row) continue;
      for (int c = 0; c < ncp; c++)
        if (row[c]) {
          if (row[c] < 0 || row[c] > ranks[r].n) { err = "a seam row holds a label outside its rank's table"; return 1; }
          if (s.empty() || s.back() != row[c]) s.push_back(row[c]);
        }
    }
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    first[r + 1] = first[r] + (long long)s.size();
    out.local_ponds += ranks[r].n;
  }
  auto node = [&](size_t r, int label) {
    return first[r] + (std::lower_bound(seam[r].begin(), seam[r].end(), label) - seam[r].begin());
  };
  std::vector<long long> parent((size_t)first[nr]);
  for (size_t i = 0; i < parent.size(); i++) parent[i] = (long long)i;

  /* a cell of the upper row touches columns c - 1, c, c + 1 of the lower one: runs [a, b) and [c, d) touch when a <= d and c <= b */
  std::vector<Run> up, lo;
  for (size_t r = 0; r + 1 < nr; r++) {
    if (!ranks[r].bottom || !ranks[r + 1].top) { err = "a seam row is missing"; return 1; }
    runs_of(ranks[r].bottom, ncp, up);
    runs_of(ranks[r + 1].top, ncp, lo);
    size_t i = 0, j = 0;
    while (i < up.size() && j < lo.size()) {
      if (up[i].s <= lo[j].e && lo[j].s <= up[i].e) {
        out.unions++;
        const long long a = find(parent, node(r, up[i].label)), b = find(parent, node(r + 1, lo[j].label));
        if (a != b) parent[std::max(a, b)] = std::min(a, b);   /* roots are first members */
      }
      if (up[i].e < lo[j].e) i++; else j++;
    }
  }

  /* numbering: every label that is its set's first member (or in no seam row) takes the next number */
  std::vector<int> number(parent.size(), 0);
  long long next = 0;
  for (size_t r = 0; r < nr; r++) {
    std::vector<int> &m = out.map[r];
    m.resize((size_t)ranks[r].n);
    size_t k = 0;                      /* next seam label of this rank */
    for (long long l = 1; l <= ranks[r].n; l++) {
      long long g;
      if (k < seam[r].size() && seam[r][k] == l) {
        const long long me = first[r] + (long long)k, root = find(parent, me);
        k++;
        if (root == me) g = ++next;
        else { g = number[(size_t)root]; out.merged++; }
        if (g <= INT32_MAX) number[(size_t)me] = (int)g;
      } else {
        g = ++next;
      }
      if (next > INT32_MAX) { err = "2^31 ponds or more: labels are int32"; return 1; }
      m[(size_t)(l - 1)] = (int)g;
    }
  }
  out.ponds = next;
  return 0;
}

/* One rank's local table into the whole raster's: rows shifted by `row_shift` (the whole-raster row of the rank's local row
 * 0), first members copied to their row, struck-out ones folded into their target.  `whole` has Result::ponds rows, zeroed
 * (cells == 0 marks a row nobody has written yet); call in rank order.  0, or 1 with a message when cells or volume_q of a
 * joined pond leave their types. */
inline int fold_table(const wdpm_pond *local, const std::vector<int> &map, int row_shift, wdpm_pond *whole, std::string &err) {
  for (size_t i = 0; i < map.size(); i++) {
    wdpm_pond p = local[i];
    p.first_row += row_shift;
    p.row_min += row_shift;
    p.row_max += row_shift;
    wdpm_pond &t = whole[map[i] - 1];
    if (t.cells == 0) { t = p; continue; }   /* first member (ranks and labels come in first-cell order) */
    if (p.cells > INT64_MAX - t.cells) { err = "the cell count of a pond joined across row blocks overflows int64"; return 1; }
    if (p.volume_q > UINT64_MAX - t.volume_q) { err = "volume_q of a pond joined across row blocks overflows its 64 bits"; return 1; }
    t.cells += p.cells;
    t.volume_q += p.volume_q;
    if (p.max_depth > t.max_depth) t.max_depth = p.max_depth;
    t.row_min = std::min(t.row_min, p.row_min);
    t.row_max = std::max(t.row_max, p.row_max);
    t.col_min = std::min(t.col_min, p.col_min);
    t.col_max = std::max(t.col_max, p.col_max);
  }
  return 0;
}

}  // namespace wdpm_stitch
#endif
