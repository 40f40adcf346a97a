/* Host emulation of the pond rims over row blocks (include/wdpm_group_pond_rims.h), after tests/rims_emu_main.cpp: a raster is cut
 * into strips of rows, each strip a rank.  A rank gets the whole-raster labels and wet masks of its owned rows and of the one row
 * beyond either end - and rubbish for the DEM and the water of those two rows, which nobody may read - numbers its own ponds by a
 * flood fill of its rows alone, finds its foreign ponds with wdpm_rims_merge::foreign_labels, and runs the rim kernels' own source
 * (wdpm_amd/csrc/wdpm_pond_rims.hip, compiled with WDPM_PONDS_EMULATION) as 256 host threads per block on buffers of exact size:
 * slots, init, the rim pass and the locate pass over its owned rows, finish.  wdpm_rims_merge::merge (wdpm_amd/csrc/
 * wdpm_rims_merge.h) then makes the whole table, which is held against a plain loop over the whole raster's cells and their eight
 * neighbours.  Built with -fsanitize=address,undefined by tests/test_group_pond_rims_merge.py; nothing here is loaded into python.
 *
 *   group_rims_emu noise ROWS COLS DENSITY SEED STRIP [ROWS_PER_WAVE]    (file rows and columns; STRIP owned rows per rank)
 *   group_rims_emu cases STRIP [ROWS_PER_WAVE]     hand-made ponds on the boundaries of strips of 4: foreign, counted once, ties
 *   group_rims_emu merge                           wdpm_rims_merge::merge alone on hand-written rank tables
 */
#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_pond_rims.hip"
#include "../wdpm_amd/csrc/wdpm_rims_merge.h"
#include "pond_emu.h"

/* ---- the raster, the reference ------------------------------------------------------------------------------------------- */
static Raster make_raster(int R, int C, double density, int seed) {
  Raster a = blank(R, C, seed);
  srand(seed);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      const size_t i = a.at(r, c);
      /* 5 % NODATA with water on it, a few NaN elevations (walls too); few distinct levels, so that ties decide; both zeros */
      const int e = rand() % 100;
      a.dem[i] = e < 5 ? INFINITY : e < 6 ? NAN : e < 10 ? (e & 1 ? -0.0 : 0.0) : 100.0 + (e % 7) * 0.25;
      const double u = unit_random();
      a.w[i] = unit_random() < density ? (u < 0.1 ? 3.0 + u * 40 : u * 0.02) : 0.0;
      if (rand() % 20 == 0) a.w[i] = 0.0005;                                    /* below either threshold's reach or not: on the rim */
      if (rand() % 100 == 0) a.w[i] = -0.25;                                    /* never added to a level */
      if (rand() % 100 == 0) a.w[i] = NAN;                                      /* never a pond cell, never added */
    }
  return a;
}

/* every cell, its eight neighbours: the definitions of include/wdpm_pond_rims.h as they are written */
static std::vector<wdpm_pond_rim> reference(const Raster &a, const std::vector<int> &labels, int n) {
  std::vector<wdpm_pond_rim> t((size_t)n);
  std::vector<unsigned long long> smin((size_t)n, ~0ull), smax((size_t)n, 0ull), rmin((size_t)n, ~0ull);
  for (auto &p : t) { p.rim_cells = p.wall_cells = 0; p.rim_row = p.rim_col = -1; p.rim_level = INFINITY; }
  for (int r = 0; r < a.g.rows; r++)
    for (int c = 0; c < a.g.ncp; c++) {
      const size_t i = a.at(r, c);
      const int L = labels[i];
      if (L) {
        const unsigned long long k = key_of(a.dem[i] + a.w[i]);
        smin[L - 1] = std::min(smin[L - 1], k);
        smax[L - 1] = std::max(smax[L - 1], k);
        continue;
      }
      int seen[8], nseen = 0;
      for (int di = -1; di <= 1; di++)
        for (int dj = -1; dj <= 1; dj++) {
          if ((!di && !dj) || !a.inside(r + di, c + dj)) continue;
          const int K = labels[a.at(r + di, c + dj)];
          if (!K || std::find(seen, seen + nseen, K) != seen + nseen) continue;
          seen[nseen++] = K;
          wdpm_pond_rim &p = t[K - 1];
          if (!(a.dem[i] < INFINITY)) { p.wall_cells++; continue; }
          p.rim_cells++;
          const double lvl = a.w[i] > 0 ? a.dem[i] + a.w[i] : a.dem[i];
          if (key_of(lvl) < rmin[K - 1]) {       /* row-major order: the first of equals stays */
            rmin[K - 1] = key_of(lvl);
            p.rim_level = lvl;
            p.rim_row = r;
            p.rim_col = c;
          }
        }
    }
  for (int k = 0; k < n; k++)
    for (int i = 0; i < 2; i++) {
      const unsigned long long key = i ? smax[k] : smin[k];
      const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
      memcpy(i ? &t[k].surface_max : &t[k].surface_min, &b, 8);
    }
  return t;
}


/* ---- the hand-made raster: 14 x 130, padded 16 x 132; with strips of 4 the boundaries lie under rows 3, 7 and 11 ------------- */
static Raster make_cases() {
  Raster a = blank(14, 130, 1);      /* labels at 0.001 m */
  for (int r = 1; r <= a.R; r++)
    for (int c = 1; c <= a.C; c++) a.dem[a.at(r, c)] = 200.0 + r * 0.5 + c * 0.01;      /* a ramp: no two dry levels alike */
  auto wet = [&](int r, int c, double d) { a.w[a.at(r, c)] = d; a.dem[a.at(r, c)] = 100.0; };
  /* foreign pond: wholly above the boundary under row 3, its lowest rim cell in row 4 - and mirrored upward at the one under 7 */
  for (int c = 5; c <= 8; c++) { wet(2, c, 1.0); wet(3, c, 1.5); }
  a.dem[a.at(4, 6)] = 50.0;
  for (int c = 60; c <= 66; c++) { wet(8, c, 1.0); wet(9, c, 0.5); }      /* column 63 / 64: lane 63 and lane 0 */
  a.dem[a.at(7, 64)] = 40.0;
  a.w[a.at(7, 64)] = 0.0005;                                             /* a film below the threshold: counts into the level */
  /* counted once: (4, 20) touches the same pond in row 3 and in row 5 */
  for (int c = 19; c <= 21; c++) { wet(3, c, 1.0); wet(5, c, 1.0); }
  wet(4, 22, 1.0);
  /* a tie across the boundary under row 7: (6, 31) and (9, 31) at one level, the upper one holds the rim; and both zeros */
  for (int c = 30; c <= 33; c++) { wet(7, c, 1.0); wet(8, c, 1.0); }
  a.dem[a.at(6, 31)] = a.dem[a.at(9, 31)] = 150.0;
  for (int c = 40; c <= 43; c++) { wet(7, c, 1.0); wet(8, c, 1.0); }
  a.dem[a.at(6, 41)] = 0.0;
  a.dem[a.at(9, 41)] = -0.0;
  for (int c = 50; c <= 53; c++) { wet(7, c, 1.0); wet(8, c, 1.0); }
  a.dem[a.at(6, 51)] = -0.0;
  a.dem[a.at(9, 51)] = 0.0;
  /* walls only: one cell in a ring of NODATA across the boundary under row 11 */
  wet(11, 100, 2.0);
  for (int r = 10; r <= 12; r++)
    for (int c = 99; c <= 101; c++)
      if (r != 11 || c != 100) a.dem[a.at(r, c)] = INFINITY;
  /* two arms of one rank joined only through the next one: one pond, two local ponds above the boundary under row 11 */
  for (int r = 9; r <= 12; r++) { wet(r, 110, 1.0); wet(r, 114, 1.25); }
  for (int c = 110; c <= 114; c++) wet(12, c, 1.0);
  /* ponds leaning on the raster's first and last row and on its last column */
  for (int c = 120; c <= 130; c++) { wet(1, c, 1.0); wet(14, c, 1.0); }
  return a;
}

/* ---- one rank ---------------------------------------------------------------------------------------------------------------- */
struct Strip { int lo, hi; };     /* owned rows of the padded raster */

static std::vector<Strip> cut(int P, int strip) {
  std::vector<Strip> out;
  for (int lo = 0; lo < P; lo += strip) out.push_back({lo, std::min(lo + strip, P) - 1});
  if (out.size() > 1 && out.back().hi - out.back().lo + 1 < 2) {      /* a view holds three rows at least */
    out[out.size() - 2].hi = out.back().hi;
    out.pop_back();
  }
  return out;
}

struct RankOut {
  std::vector<wdpm_pond_rim> rows;
  std::vector<int> label;
  int view0;
  long long foreign;
};

static RankOut run_rank(const Raster &a, const std::vector<int> &whole, int nwhole, Strip st, int forced_rpw) {
  const int P = a.g.rows, ncp = a.g.ncp;
  const int v0 = st.lo > 0 ? st.lo - 1 : 0, v1 = st.hi < P - 1 ? st.hi + 1 : P - 1;
  Geom g;
  g.rows = v1 - v0 + 1;
  g.ncp = ncp;
  g.nsc = a.g.nsc;
  g.nseg = g.rows * g.nsc;
  const int ra = st.lo - v0, rb = ra + (st.hi - st.lo + 1);
  std::vector<double> w((size_t)g.rows * ncp), dem(w.size());
  std::vector<int> labels(w.size());
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < ncp; c++) {
      const size_t i = (size_t)r * ncp + c, j = a.at(v0 + r, c);
      const bool own = r >= ra && r < rb;
      w[i] = own ? a.w[j] : 1e300;            /* a halo row's water and DEM are not current between exchanges: never read */
      dem[i] = own ? a.dem[j] : -1e300;
      labels[i] = whole[j];
    }
  const std::vector<unsigned long long> masks = wet_masks(g, labels);
  /* the rank's own numbering: a flood fill of its owned rows alone, first-cell order; map[local - 1] = the whole raster's number */
  std::vector<int> local(w.size(), 0), map;
  for (int r = ra; r < rb; r++)
    for (int c = 0; c < ncp; c++) {
      if (!labels[(size_t)r * ncp + c] || local[(size_t)r * ncp + c]) continue;
      map.push_back(labels[(size_t)r * ncp + c]);
      const int l = (int)map.size();
      std::queue<std::pair<int, int>> todo;
      todo.push({r, c});
      local[(size_t)r * ncp + c] = l;
      while (!todo.empty()) {
        const auto [i, j] = todo.front();
        todo.pop();
        for (int di = -1; di <= 1; di++)
          for (int dj = -1; dj <= 1; dj++) {
            const int y = i + di, x = j + dj;
            if (y < ra || y >= rb || x < 0 || x >= ncp) continue;
            if (labels[(size_t)y * ncp + x] && !local[(size_t)y * ncp + x]) {
              local[(size_t)y * ncp + x] = l;
              todo.push({y, x});
            }
          }
      }
    }
  std::vector<int> beside, own;
  if (st.lo > 0) {
    beside.insert(beside.end(), labels.begin(), labels.begin() + ncp);
    own.insert(own.end(), labels.begin() + (size_t)ra * ncp, labels.begin() + (size_t)(ra + 1) * ncp);
  }
  if (st.hi < P - 1) {
    beside.insert(beside.end(), labels.end() - ncp, labels.end());
    own.insert(own.end(), labels.begin() + (size_t)(rb - 1) * ncp, labels.begin() + (size_t)rb * ncp);
  }
  std::vector<int> foreign;
  wdpm_rims_merge::foreign_labels(beside.data(), beside.size(), own.data(), own.size(), foreign);

  RankOut out;
  out.view0 = v0;
  out.foreign = (long long)foreign.size();
  out.label = map;
  out.label.insert(out.label.end(), foreign.begin(), foreign.end());
  const long long slots = (long long)out.label.size();
  out.rows.resize((size_t)slots);
  if (!slots) return out;
  const int nlocal = (int)map.size(), nforeign = (int)foreign.size();
  std::vector<int> slot_of((size_t)nwhole + 1, 0x7f7f7f7f);
  std::vector<RimRow> table((size_t)slots);
  const Waves wv = waves_over(g, rb - ra, forced_rpw);
  const int rpw = wv.rpw, nwaves = wv.n;
  launch(blocks_for(slots, kBlock), [&] { rims_slots_kernel(map.data(), nlocal, foreign.data(), nforeign, slot_of.data()); });
  launch(blocks_for(slots, kBlock), [&] { rims_init_kernel(table.data(), slots); });
  launch(blocks_for(nwaves, kWaves), [&] {
    rims_pass_rows_kernel(w.data(), dem.data(), masks.data(), labels.data(), g, rpw, nwaves, table.data(), ra, rb, slot_of.data());
  });
  launch(blocks_for(nwaves, kWaves), [&] {
    rims_locate_rows_kernel(w.data(), dem.data(), masks.data(), labels.data(), g, rpw, nwaves, table.data(), ra, rb, slot_of.data());
  });
  launch(blocks_for(slots, kBlock), [&] { rims_finish_kernel(table.data(), slots, ncp); });
  memcpy(out.rows.data(), table.data(), (size_t)slots * sizeof(wdpm_pond_rim));
  return out;
}

static int run_raster(const Raster &a, int strip, int forced_rpw, const char *what) {
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  const std::vector<Strip> strips = cut(a.g.rows, strip);
  std::vector<RankOut> outs;
  for (const Strip &st : strips) outs.push_back(run_rank(a, labels, n, st, forced_rpw));
  std::vector<wdpm_rims_merge::RankRims> ranks;
  long long foreign = 0, slots = 0;
  for (const RankOut &o : outs) {
    ranks.push_back({o.rows.data(), o.label.data(), (long long)o.label.size(), o.view0});
    foreign += o.foreign;
    slots += (long long)o.label.size();
  }
  std::vector<wdpm_pond_rim> table((size_t)n);
  std::string err;
  if (wdpm_rims_merge::merge(ranks, n, table.data(), err)) {
    printf("merge failed: %s\n", err.c_str());
    return 1;
  }
  const std::vector<wdpm_pond_rim> ref = reference(a, labels, n);
  long long bad = 0, no_rim = 0;
  for (int k = 0; k < n; k++) {
    bad += memcmp(&ref[k], &table[k], sizeof(wdpm_pond_rim)) != 0;
    no_rim += ref[k].rim_cells == 0;
  }
  printf("%s %dx%d strips of %d rows (%zu ranks): N %d slots %lld foreign %lld ponds without a rim %lld  rim mismatches %lld\n", what,
         a.R, a.C, strip, strips.size(), n, slots, foreign, no_rim, bad);
  return bad != 0;
}

/* ---- the merge alone ----------------------------------------------------------------------------------------------------------- */
static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }
#define CHECK(cond) do { if (!(cond)) { printf("merge check failed: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static int run_merge_checks() {
  using namespace wdpm_rims_merge;
  const double unset_min = from_key(~0ull), unset_max = from_key(0ull);
  std::string err;
  /* pond 1: a tie of the rim level in two ranks - the upper rank's cell; pond 2: -0.0 in the lower rank beats +0.0 in the upper one;
   * pond 3: +0.0 below, -0.0 above: the upper one stays; pond 4: no rim anywhere; pond 5: rank 1 holds it as a foreign pond */
  const wdpm_pond_rim r0[] = {{10.0, 11.0, 5.0, 3, 7, 4, 1},        {1.0, 2.0, 0.0, 2, 2, 1, 0},  {1.0, 2.0, -0.0, 2, 9, 1, 0},
                              {7.0, 7.5, INFINITY, -1, -1, 0, 8},   {3.0, 3.5, 9.0, 1, 1, 2, 0}};
  const int l0[] = {1, 2, 3, 4, 5};
  const wdpm_pond_rim r1[] = {{9.5, 10.5, 5.0, 1, 2, 6, 2},         {-0.0, 0.0, -0.0, 2, 3, 2, 1}, {0.5, 3.0, 0.0, 1, 4, 2, 0},
                              {7.25, 8.0, INFINITY, -1, -1, 0, 3},  {unset_min, unset_max, 8.0, 1, 5, 1, 1}};
  const int l1[] = {1, 2, 3, 4, 5};
  std::vector<RankRims> ranks = {{r0, l0, 5, 0}, {r1, l1, 5, 4}};
  wdpm_pond_rim t[5];
  CHECK(merge(ranks, 5, t, err) == 0);
  CHECK(t[0].surface_min == 9.5 && t[0].surface_max == 11.0 && t[0].rim_level == 5.0 && t[0].rim_row == 3 && t[0].rim_col == 7);
  CHECK(t[0].rim_cells == 10 && t[0].wall_cells == 3);
  CHECK(same_bits(t[1].rim_level, -0.0) && t[1].rim_row == 6 && t[1].rim_col == 3 && same_bits(t[1].surface_min, -0.0));
  CHECK(same_bits(t[2].rim_level, -0.0) && t[2].rim_row == 2 && t[2].rim_col == 9 && t[2].surface_max == 3.0);
  CHECK(std::isinf(t[3].rim_level) && t[3].rim_level > 0 && t[3].rim_row == -1 && t[3].rim_col == -1 && t[3].rim_cells == 0 && t[3].wall_cells == 11);
  CHECK(t[4].surface_min == 3.0 && t[4].surface_max == 3.5 && t[4].rim_level == 8.0 && t[4].rim_row == 5 && t[4].rim_col == 5 && t[4].rim_cells == 3);
  /* a slot nothing was sent to (two local ponds that are one) changes nothing, wherever it stands */
  const wdpm_pond_rim r2[] = {{unset_min, unset_max, INFINITY, -1, -1, 0, 0}, {2.0, 2.5, 1.0, 0, 1, 1, 0}};
  const int l2[] = {1, 1};
  ranks = {{r2, l2, 2, 10}};
  CHECK(merge(ranks, 1, t, err) == 0);
  CHECK(t[0].surface_min == 2.0 && t[0].surface_max == 2.5 && t[0].rim_level == 1.0 && t[0].rim_row == 10 && t[0].rim_cells == 1);
  /* counts that leave int64, a label outside the table: a message, not a wrong number */
  const wdpm_pond_rim big[] = {{1.0, 1.0, 0.5, 1, 1, INT64_MAX - 1, 0}}, two[] = {{1.0, 1.0, 0.5, 1, 1, 2, 0}};
  const wdpm_pond_rim wbig[] = {{1.0, 1.0, 0.5, 1, 1, 1, INT64_MAX}}, wone[] = {{1.0, 1.0, 0.5, 1, 1, 1, 1}};
  const int one[] = {1}, nine[] = {9};
  ranks = {{big, one, 1, 0}, {two, one, 1, 4}};
  err.clear();
  CHECK(merge(ranks, 1, t, err) == 1 && err.find("rim_cells") != std::string::npos && err.find("overflows") != std::string::npos);
  ranks = {{wbig, one, 1, 0}, {wone, one, 1, 4}};
  err.clear();
  CHECK(merge(ranks, 1, t, err) == 1 && err.find("wall_cells") != std::string::npos);
  ranks = {{two, nine, 1, 0}};
  err.clear();
  CHECK(merge(ranks, 1, t, err) == 1 && !err.empty());
  ranks.clear();
  CHECK(merge(ranks, 0, nullptr, err) == 0);
  printf("merge checks ok\n");
  return 0;
}

int main(int argc, char **argv) {
  emu_init();
  if (argc == 2 && !strcmp(argv[1], "merge")) return run_merge_checks();
  if (argc >= 3 && !strcmp(argv[1], "cases")) return run_raster(make_cases(), atoi(argv[2]), argc > 3 ? atoi(argv[3]) : 0, "cases");
  if (argc >= 7 && !strcmp(argv[1], "noise"))
    return run_raster(make_raster(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atoi(argv[5])), atoi(argv[6]), argc > 7 ? atoi(argv[7]) : 0,
                      "noise");
  fprintf(stderr, "usage: %s noise ROWS COLS DENSITY SEED STRIP [ROWS_PER_WAVE] | cases STRIP [ROWS_PER_WAVE] | merge\n", argv[0]);
  return 2;
}
