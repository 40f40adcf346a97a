/* Host emulation of the rim kernels (wdpm_amd/csrc/wdpm_pond_rims.hip, compiled with WDPM_PONDS_EMULATION), after the pattern of
 * tests/ponds_emu_main.cpp: the kernels' own source runs as 256 threads per block, in lockstep wherever lanes talk to each other,
 * blocks one after another, atomics as host atomics.  Built with -fsanitize=address,undefined by
 * tests/test_pond_rims_emulation.py: a halo lane that reads outside a raster (column 0 / ncp - 1, row 0 / rows - 1, the cells
 * beside a segment) is found here, on a CPU.  Labels and wet masks come from a row-major flood fill, every buffer has its exact
 * size, and the rim table is held against a plain loop over the cells and their eight neighbours.
 *
 *   rims_emu ROWS COLS DENSITY SEED [ROWS_PER_WAVE]      (file rows and columns; odd seeds label at 0.001 m, even ones at 0)
 */
#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_pond_rims.hip"
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

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s ROWS COLS DENSITY SEED [ROWS_PER_WAVE]\n", argv[0]);
    return 2;
  }
  const Raster a = make_raster(atoi(argv[1]), atoi(argv[2]), atof(argv[3]), atoi(argv[4]));
  const int forced_rpw = argc > 5 ? atoi(argv[5]) : 0;
  emu_init();

  const Geom g = a.g;
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  const std::vector<unsigned long long> masks = wet_masks(g, labels);
  std::vector<RimRow> table((size_t)n);                                /* exact sizes: the sanitizer sees a stray index */
  const Waves wv = waves_over(g, g.rows, forced_rpw);
  const int rpw = wv.rpw, nwaves = wv.n;
  if (n) {
    launch(blocks_for(n, kBlock), [&] { rims_init_kernel(table.data(), n); });
    launch(blocks_for(nwaves, kWaves), [&] {
      rims_pass_kernel(a.w.data(), a.dem.data(), masks.data(), labels.data(), g, rpw, nwaves, table.data());
    });
    launch(blocks_for(nwaves, kWaves), [&] {
      rims_locate_kernel(a.w.data(), a.dem.data(), masks.data(), labels.data(), g, rpw, nwaves, table.data());
    });
    launch(blocks_for(n, kBlock), [&] { rims_finish_kernel(table.data(), n, g.ncp); });
  }

  const std::vector<wdpm_pond_rim> ref = reference(a, labels, n);
  long long bad = 0, rim_total = 0, wall_total = 0, no_rim = 0;
  for (int k = 0; k < n; k++) {
    bad += memcmp(&ref[k], &table[k], sizeof(wdpm_pond_rim)) != 0;
    rim_total += ref[k].rim_cells;
    wall_total += ref[k].wall_cells;
    no_rim += ref[k].rim_cells == 0;
  }
  printf("%dx%d density %.2f min_depth %.3f: N %d rim memberships %lld wall memberships %lld ponds without a rim %lld "
         "rows per wave %d  rim mismatches %lld\n",
         a.R, a.C, atof(argv[3]), a.min_depth, n, rim_total, wall_total, no_rim, rpw, bad);
  return bad != 0;
}
