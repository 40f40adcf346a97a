/* Host emulation of the outlet kernels (wdpm_amd/csrc/wdpm_pond_outlets.hip, compiled with WDPM_PONDS_EMULATION), after the pattern
 * of tests/catch_emu_main.cpp: the kernels' own source runs as 256 threads per block, in lockstep wherever lanes talk to each other,
 * blocks one after another, atomics as host atomics.  Built with -fsanitize=address,undefined by
 * tests/test_pond_outlets_emulation.py: a window lane that reads outside a raster is found here, on a CPU.  Labels come from a
 * row-major flood fill, the basin raster from a walk down every cell's descent one step at a time, every buffer has its exact
 * size, and the table and the counts are held against a plain double loop over all pairs of neighbouring cells.
 *
 *   outlets_emu ROWS COLS DENSITY SEED [ROWS_PER_WAVE]   (file rows and columns; odd seeds label at 0.001 m, even ones at 0;
 *                                                         seed 0: one ramp into one pond, a single basin - DENSITY unused)
 */
#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_pond_outlets.hip"
#include "pond_emu.h"

/* ---- the raster, the reference ------------------------------------------------------------------------------------------- */
static Raster make_raster(int R, int C, double density, int seed) {
  Raster a = blank(R, C, seed);
  srand(seed);
  const int period = 5 + seed % 4;
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      const size_t i = a.at(r, c);
      /* 5 % NODATA with water on it, a few NaN elevations; quarter-metre steps down slanted valleys that repeat, so that basins
       * are several cells wide, cross every seam and meet ties on their divides; both zeros */
      const int e = rand() % 100;
      const int ramp = abs((r * 2 + c) % (2 * period) - period);
      a.dem[i] = e < 5 ? INFINITY : e < 6 ? NAN : e < 9 ? (e & 1 ? -0.0 : 0.0) : 100.0 + (ramp + e % 2) * 0.25;
      const double u = unit_random();
      a.w[i] = unit_random() < density ? (u < 0.1 ? 3.0 + u * 40 : u * 0.02) : 0.0;
      if (rand() % 20 == 0) a.w[i] = 0.0005;                                    /* a film: below either threshold's reach or not */
      if (rand() % 50 == 0) a.w[i] = (rand() % 1000 + 0.5) * ldexp(1.0, -24);   /* ties of rint */
      if (rand() % 100 == 0) a.w[i] = -0.25;                                    /* never added to a level */
      if (rand() % 100 == 0) a.w[i] = NAN;                                      /* never a pond cell, never added */
    }
  return a;
}

/* a plane that falls towards the last column, whose last two columns are one pond: one basin over everything, no pass anywhere */
static Raster make_ramp(int R, int C) {
  Raster a = blank(R, C, 0);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      a.dem[a.at(r, c)] = 1000.0 - 0.5 * c;
      a.w[a.at(r, c)] = c >= C - 1 ? 0.25 : 0.0;       /* the surface stays below the land */
    }
  return a;
}

static double level_of(const Raster &a, size_t i) { return a.w[i] > 0 ? a.dem[i] + a.w[i] : a.dem[i]; }

/* basin(c) of include/wdpm_pond_catchments.h as it is written: follow receivers one step at a time */
static std::vector<int> basins_of(const Raster &a, const std::vector<int> &labels) {
  const Geom g = a.g;
  auto has_level = [&](int r, int c) { return a.inside(r, c) && a.dem[a.at(r, c)] < INFINITY; };
  std::vector<int> basin(a.w.size(), -1);
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      if (!has_level(r, c)) continue;
      int pr = r, pc = c, end = 0;
      for (;;) {
        if (labels[a.at(pr, pc)]) { end = labels[a.at(pr, pc)]; break; }
        bool found = false;
        unsigned long long best = 0;
        int nr = 0, nc = 0;
        for (int di = -1; di <= 1; di++)
          for (int dj = -1; dj <= 1; dj++) {
            if ((!di && !dj) || !has_level(pr + di, pc + dj)) continue;
            const unsigned long long k = key_of(level_of(a, a.at(pr + di, pc + dj)));
            if (!found || k < best) { found = true; best = k; nr = pr + di; nc = pc + dj; }
          }
        if (!found || !(best < key_of(level_of(a, a.at(pr, pc))))) break;
        pr = nr; pc = nc;
      }
      basin[a.at(r, c)] = end;
    }
  return basin;
}

struct Reference {
  std::vector<wdpm_pond_outlet> table;
  long long no_outlet, to_land, divide;
  bool deep;
};

/* the definitions of include/wdpm_pond_outlets.h as they are written: every cell, every neighbour */
static Reference reference(const Raster &a, const std::vector<int> &basin, int n) {
  const Geom g = a.g;
  Reference ref;
  ref.table.assign((size_t)n, wdpm_pond_outlet());
  ref.no_outlet = ref.to_land = ref.divide = 0;
  ref.deep = false;
  std::vector<unsigned long long> pour((size_t)n, 0ull);
  std::vector<char> found((size_t)n, 0);
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      const int k = basin[a.at(r, c)];
      if (k <= 0) continue;
      bool on_divide = false;
      for (int di = -1; di <= 1; di++)
        for (int dj = -1; dj <= 1; dj++) {
          if ((!di && !dj) || !a.inside(r + di, c + dj)) continue;
          const int j = basin[a.at(r + di, c + dj)];
          if (j < 0 || j == k) continue;
          on_divide = true;
          const unsigned long long h = std::max(key_of(level_of(a, a.at(r, c))), key_of(level_of(a, a.at(r + di, c + dj))));
          wdpm_pond_outlet &t = ref.table[(size_t)k - 1];
          if (found[(size_t)k - 1] && !(h < pour[(size_t)k - 1])) continue;     /* row-major a, neighbour order b: the first stays */
          found[(size_t)k - 1] = 1;
          pour[(size_t)k - 1] = h;
          t.from_row = r; t.from_col = c; t.to_row = r + di; t.to_col = c + dj; t.to_basin = j;
        }
      ref.table[(size_t)k - 1].divide_cells += on_divide;
    }
  for (int k = 0; k < n; k++) {
    wdpm_pond_outlet &t = ref.table[(size_t)k];
    if (!found[(size_t)k]) {
      t.pour_level = INFINITY;
      t.from_row = t.from_col = t.to_row = t.to_col = t.to_basin = -1;
      ref.no_outlet++;
      continue;
    }
    const unsigned long long key = pour[(size_t)k], b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    memcpy(&t.pour_level, &b, 8);
    ref.to_land += t.to_basin == 0;
    ref.divide += t.divide_cells;
  }
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      const int k = basin[a.at(r, c)];
      if (k <= 0 || !found[(size_t)k - 1]) continue;
      const double lvl = level_of(a, a.at(r, c));
      if (!(key_of(lvl) < pour[(size_t)k - 1])) continue;
      const double depth = ref.table[(size_t)k - 1].pour_level - lvl;
      if (!(depth < 512.0)) { ref.deep = true; continue; }
      ref.table[(size_t)k - 1].fill_cells++;
      ref.table[(size_t)k - 1].fill_q += (unsigned long long)rint(depth * 16777216.0);
    }
  return ref;
}

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s ROWS COLS DENSITY SEED [ROWS_PER_WAVE]\n", argv[0]);
    return 2;
  }
  const int seed = atoi(argv[4]);
  const Raster a = seed ? make_raster(atoi(argv[1]), atoi(argv[2]), atof(argv[3]), seed) : make_ramp(atoi(argv[1]), atoi(argv[2]));
  const int forced_rpw = argc > 5 ? atoi(argv[5]) : 0;
  emu_init();

  const Geom g = a.g;
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  const std::vector<int> basin = basins_of(a, labels);                 /* exact sizes: the sanitizer sees a stray index */

  std::vector<OutletRow> table((size_t)n);
  OutletStatus st;
  memset(&st, 0, sizeof st);
  const Waves wv = waves_over(g, g.rows, forced_rpw);
  const int rpw = wv.rpw, nwaves = wv.n;
  if (n) {                                                             /* the launches of wdpm_outlets_label */
    launch(blocks_for(n, kBlock), [&] { outlet_init_kernel(table.data(), n); });
    launch(blocks_for(nwaves, kWaves), [&] { outlet_passes_kernel(a.w.data(), a.dem.data(), basin.data(), g, rpw, nwaves, table.data()); });
    launch(blocks_for(nwaves, kWaves), [&] {
      outlet_locate_kernel(a.w.data(), a.dem.data(), basin.data(), g, rpw, nwaves, table.data(), &st);
    });
    launch(blocks_for(n, kBlock), [&] { outlet_finish_kernel(table.data(), n, basin.data(), g.ncp, &st); });
  }

  const Reference ref = reference(a, basin, n);
  long long bad_rows = 0, filled = 0;
  for (int k = 0; k < n; k++) {
    bad_rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_outlet)) != 0;
    filled += ref.table[k].fill_cells;
  }
  const bool counts = (long long)st.no_outlet == ref.no_outlet && (long long)st.to_land == ref.to_land && (long long)st.divide == ref.divide &&
                      (st.deep != 0) == ref.deep;
  printf("%dx%d density %.2f min_depth %.3f: N %d without outlet %lld to land %lld divide %lld filled %lld rows per wave %d  "
         "table mismatches %lld counts %s\n",
         a.R, a.C, atof(argv[3]), a.min_depth, n, ref.no_outlet, ref.to_land, ref.divide, filled, rpw, bad_rows,
         counts ? "agree" : "DIFFER");
  return bad_rows != 0 || !counts || ref.deep;
}
