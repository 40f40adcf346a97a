/* Host emulation of the curve kernels (wdpm_amd/csrc/wdpm_pond_curves.hip, compiled with WDPM_PONDS_EMULATION), after the pattern
 * of tests/outlets_emu_main.cpp: the kernels' own source runs as 256 threads per block, in lockstep wherever lanes talk to each other,
 * blocks one after another, atomics as host atomics.  Built with -fsanitize=address,undefined by
 * tests/test_pond_curves_emulation.py: a lane that reads outside a raster or a table is found here, on a CPU.  Labels come from a
 * row-major flood fill, the basin raster from a walk down every cell's descent one step at a time, the pour levels from a plain
 * double loop over all pairs of neighbouring cells, every buffer has its exact size, and the table and the counts are held against a
 * plain double loop over all cells and stages.
 *
 *   curves_emu ROWS COLS DENSITY SEED [ROWS_PER_WAVE]    (file rows and columns; odd seeds label at 0.001 m, even ones at 0;
 *                                                         seed 0: one ramp into one pond, a single basin - DENSITY unused)
 */
#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_pond_curves.hip"
#include "pond_emu.h"

/* ---- the raster, the reference ------------------------------------------------------------------------------------------- */
static Raster make_raster(int R, int C, double density, int seed) {
  Raster a = blank(R, C, seed);
  srand(seed);
  const int period = 5 + seed % 4;
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      const size_t i = a.at(r, c);
      /* 5 % NODATA with water on it, a few NaN elevations; valleys that repeat, with ground in steps of 2^-5 m so that heights fall
       * on stages and between them; both zeros */
      const int e = rand() % 100;
      const int ramp = abs((r * 2 + c) % (2 * period) - period);
      a.dem[i] = e < 5 ? INFINITY : e < 6 ? NAN : e < 9 ? (e & 1 ? -0.0 : 0.0) : 100.0 + ramp * 0.25 + (e % 8) * 0.03125;
      const double u = unit_random();
      a.w[i] = unit_random() < density ? (u < 0.1 ? 3.0 + u * 40 : u * 0.02) : 0.0;
      if (rand() % 20 == 0) a.w[i] = 0.0005;
      if (rand() % 50 == 0) a.w[i] = (rand() % 1000 + 0.5) * ldexp(1.0, -24);   /* ties of rint */
      if (rand() % 100 == 0) a.w[i] = -0.25;
      if (rand() % 100 == 0) a.w[i] = NAN;
    }
  return a;
}

/* a plane that falls towards the last column, whose last two columns are one pond: one basin over everything, no outlet, no curve */
static Raster make_ramp(int R, int C) {
  Raster a = blank(R, C, 0);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      a.dem[a.at(r, c)] = 1000.0 - 0.5 * c;
      a.w[a.at(r, c)] = c >= C - 1 ? 0.25 : 0.0;
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

/* pour_level of include/wdpm_pond_outlets.h as it is written; the other columns of the outlet rows stay zero: the curve pass reads
 * the pour level alone */
static std::vector<wdpm_pond_outlet> pour_levels(const Raster &a, const std::vector<int> &basin, int n) {
  const Geom g = a.g;
  std::vector<wdpm_pond_outlet> out((size_t)n, wdpm_pond_outlet());
  std::vector<unsigned long long> pour((size_t)n, 0ull);
  std::vector<char> found((size_t)n, 0);
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      const int k = basin[a.at(r, c)];
      if (k <= 0) continue;
      for (int di = -1; di <= 1; di++)
        for (int dj = -1; dj <= 1; dj++) {
          if ((!di && !dj) || !a.inside(r + di, c + dj)) continue;
          const int j = basin[a.at(r + di, c + dj)];
          if (j < 0 || j == k) continue;
          const unsigned long long h = std::max(key_of(level_of(a, a.at(r, c))), key_of(level_of(a, a.at(r + di, c + dj))));
          if (found[(size_t)k - 1] && !(h < pour[(size_t)k - 1])) continue;
          found[(size_t)k - 1] = 1;
          pour[(size_t)k - 1] = h;
        }
    }
  for (int k = 0; k < n; k++) {
    const unsigned long long key = pour[(size_t)k], b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    if (found[(size_t)k]) memcpy(&out[(size_t)k].pour_level, &b, 8);
    else out[(size_t)k].pour_level = INFINITY;
  }
  return out;
}

struct Reference {
  std::vector<wdpm_pond_curve> table;
  long long no_curve, flat, stage_cells;
  bool deep;
};

/* the definitions of include/wdpm_pond_curves.h as they are written: every cell, every stage.  volatile keeps each of the three
 * operations of a stage height a rounded double of its own whatever the compiler would like to do with them. */
static Reference reference(const Raster &a, const std::vector<int> &basin, const std::vector<wdpm_pond_outlet> &outlets, int n) {
  const Geom g = a.g;
  Reference ref;
  ref.table.assign((size_t)n, wdpm_pond_curve());
  ref.no_curve = ref.flat = ref.stage_cells = 0;
  ref.deep = false;
  std::vector<char> seen((size_t)n, 0);
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      const int k = basin[a.at(r, c)];
      if (k <= 0) continue;
      wdpm_pond_curve &t = ref.table[(size_t)k - 1];
      const double e = a.dem[a.at(r, c)];
      if (!seen[(size_t)k - 1] || key_of(e) < key_of(t.bed_level)) t.bed_level = e;
      seen[(size_t)k - 1] = 1;
    }
  for (int k = 0; k < n; k++) {
    wdpm_pond_curve &t = ref.table[(size_t)k];
    t.top_level = outlets[(size_t)k].pour_level;
    ref.no_curve += !(t.top_level < INFINITY);
    ref.flat += t.top_level == t.bed_level;
  }
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      const int k = basin[a.at(r, c)];
      if (k <= 0) continue;
      wdpm_pond_curve &t = ref.table[(size_t)k - 1];
      if (!(t.top_level < INFINITY)) continue;
      const double e = a.dem[a.at(r, c)];
      for (int s = 1; s <= WDPM_CURVE_STAGES; s++) {
        volatile double span = t.top_level - t.bed_level;
        volatile double part = span * (s / 16.0);
        volatile double sum = t.bed_level + part;
        const double h = s == WDPM_CURVE_STAGES ? t.top_level : sum;
        if (!(key_of(e) < key_of(h))) continue;
        const double depth = h - e;
        if (!(depth < 512.0)) { ref.deep = true; continue; }
        t.cells[s - 1]++;
        t.q[s - 1] += (unsigned long long)rint(depth * 16777216.0);
      }
    }
  for (int k = 0; k < n; k++) ref.stage_cells += ref.table[(size_t)k].cells[WDPM_CURVE_STAGES - 1];
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
  const std::vector<wdpm_pond_outlet> outlets = pour_levels(a, basin, n);

  std::vector<CurveRow> table((size_t)n);
  CurveStatus st;
  memset(&st, 0, sizeof st);
  const Waves wv = waves_over(g, g.rows, forced_rpw);
  const int rpw = wv.rpw, nwaves = wv.n;
  if (n) {                                                             /* the launches of wdpm_curves_label */
    launch(blocks_for((long long)n * kCurveWords, kBlock), [&] { curves_init_kernel(table.data(), n, outlets.data()); });
    launch(blocks_for(nwaves, kWaves), [&] { curves_bed_kernel(a.dem.data(), basin.data(), g, rpw, nwaves, table.data()); });
    launch(blocks_for(nwaves, kWaves), [&] { curves_stages_kernel(a.dem.data(), basin.data(), g, rpw, nwaves, table.data(), &st); });
    launch(blocks_for(n, kBlock), [&] { curves_finish_kernel(table.data(), n, &st); });
  }

  const Reference ref = reference(a, basin, outlets, n);
  long long bad_rows = 0, distinct = 0;
  for (int k = 0; k < n; k++) {
    bad_rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_curve)) != 0;
    int d = 0;
    for (int s = 0; s < WDPM_CURVE_STAGES; s++) d += ref.table[k].cells[s] != (s ? ref.table[k].cells[s - 1] : 0);
    distinct = std::max<long long>(distinct, d);
  }
  const bool counts = (long long)st.no_curve == ref.no_curve && (long long)st.flat == ref.flat && (long long)st.stage_cells == ref.stage_cells &&
                      (st.deep != 0) == ref.deep;
  printf("%dx%d density %.2f min_depth %.3f: N %d without curve %lld flat %lld stage cells %lld most steps %lld rows per wave %d  "
         "table mismatches %lld counts %s\n",
         a.R, a.C, atof(argv[3]), a.min_depth, n, ref.no_curve, ref.flat, ref.stage_cells, distinct, rpw, bad_rows,
         counts ? "agree" : "DIFFER");
  return bad_rows != 0 || !counts || ref.deep;
}
