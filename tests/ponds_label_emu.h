/* The label kernels (wdpm_amd/csrc/wdpm_ponds.hip) on the host, for tests/ponds_emu_main.cpp and tests/group_ponds_emu_main.cpp:
 * their noise raster, the flood fill that also fills the table, and the launches of wdpm_ponds_label in its order. */
#ifndef WDPM_TESTS_PONDS_LABEL_EMU_H
#define WDPM_TESTS_PONDS_LABEL_EMU_H

#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_ponds.hip"
#include "pond_emu.h"

static Raster make_raster(int R, int C, double density, int seed) {
  Raster a = blank(R, C, seed);
  srand(seed);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      const size_t i = a.at(r, c);
      a.dem[i] = rand() % 100 < 5 ? INFINITY : 100.0;                           /* 5 % NODATA, with water on it */
      const double u = unit_random();
      a.w[i] = unit_random() < density ? (u < 0.1 ? 3.0 + u * 40 : u * 0.02) : 0.0;
      if (rand() % 50 == 0) a.w[i] = (rand() % 1000 + 0.5) * ldexp(1.0, -24);   /* ties of rint */
      if (rand() % 200 == 0) a.w[i] = NAN;                                      /* never a pond cell */
    }
  return a;
}

/* the flood fill's labels and, from a walk over them in row-major order, the table as wdpm_ponds_table hands it out */
static void flood_fill(const Raster &a, std::vector<int> &labels, std::vector<PondRow> &table) {
  int n = 0;
  flood_fill(a, labels, n);
  table.assign((size_t)n, PondRow{0, 0, 0ull, 0ull, 0ull, INT_MAX, -1, INT_MAX, -1});
  std::vector<double> deepest((size_t)n, -1.0);
  for (int r = 0; r < a.g.rows; r++)
    for (int c = 0; c < a.g.ncp; c++) {
      const int L = labels[a.at(r, c)];
      if (!L) continue;
      PondRow &p = table[(size_t)L - 1];
      const double d = a.w[a.at(r, c)];
      if (!p.cells++) { p.first_row = r; p.first_col = c; }
      p.volume_q += (unsigned long long)rint(d * 16777216.0);
      deepest[(size_t)L - 1] = std::max(deepest[(size_t)L - 1], d);
      p.row_min = std::min(p.row_min, r);
      p.row_max = std::max(p.row_max, r);
      p.col_min = std::min(p.col_min, c);
      p.col_max = std::max(p.col_max, c);
    }
  for (int k = 0; k < n; k++) memcpy(&table[k].depth_key, &deepest[k], 8);      /* the finished table holds the depth itself */
}

/* the buffers of one label call, of exact size: the sanitizer sees a stray index */
struct LabelRun {
  std::vector<unsigned long long> masks, rootmask, busum;
  std::vector<int> parent, labels, cnt, bsum;
  std::vector<unsigned> ucnt;
  std::vector<PondRow> table;
  Status st;
  int rpw;
};

/* mask, merge, flatten, the three scan kernels: st.ponds and every run's base are known after this */
static void label_scan(const Raster &a, LabelRun &s) {
  const Geom g = a.g;
  const int nb = (g.nseg + kScanTile - 1) / kScanTile;
  s.masks.resize(g.nseg);
  s.rootmask.resize(g.nseg);
  s.parent.assign(a.w.size(), -7);
  s.labels.assign(a.w.size(), -1);
  s.cnt.resize(g.nseg);
  s.ucnt.resize(g.nseg);
  s.bsum.resize(nb);
  s.busum.resize(2 * nb);
  memset(&s.st, 0, sizeof s.st);
  const unsigned seg_blocks = blocks_for(g.nseg, kWaves);
  launch(seg_blocks, [&] { ponds_mask_kernel(a.w.data(), a.dem.data(), g, a.min_depth, s.masks.data(), s.parent.data(), &s.st); });
  launch(seg_blocks, [&] { ponds_merge_kernel(s.masks.data(), s.parent.data(), g, s.ucnt.data()); });
  launch(seg_blocks, [&] { ponds_flatten_kernel(s.masks.data(), s.parent.data(), g, s.cnt.data(), s.rootmask.data()); });
  launch(nb, [&] { ponds_scan_reduce_kernel(s.cnt.data(), s.ucnt.data(), g.nseg, s.bsum.data(), s.busum.data()); });
  launch(1, [&] { ponds_scan_sums_kernel(s.bsum.data(), s.busum.data(), nb, &s.st); });
  launch(nb, [&] { ponds_scan_down_kernel(s.cnt.data(), g.nseg, s.bsum.data()); });
}

/* table init, body, finish; with a map (row blocks: exactly st.ponds entries) the mapped body */
static void label_table(const Raster &a, LabelRun &s, int forced_rpw, const int *map) {
  const Geom g = a.g;
  const long long n = s.st.ponds;
  s.table.resize(n);
  const Waves wv = waves_over(g, g.rows, forced_rpw);
  s.rpw = wv.rpw;
  if (n) launch(blocks_for(n, kBlock), [&] { ponds_table_init_kernel(s.table.data(), n); });
  launch(blocks_for(wv.n, kWaves), [&] {
    if (map)
      ponds_table_mapped_kernel(a.w.data(), s.masks.data(), s.parent.data(), s.cnt.data(), s.rootmask.data(), g, wv.rpw, wv.n,
                                s.labels.data(), s.table.data(), map);
    else
      ponds_table_kernel(a.w.data(), s.masks.data(), s.parent.data(), s.cnt.data(), s.rootmask.data(), g, wv.rpw, wv.n,
                         s.labels.data(), s.table.data());
  });
  if (n) launch(blocks_for(n, kBlock), [&] { ponds_table_finish_kernel(s.table.data(), n); });
}

#endif
