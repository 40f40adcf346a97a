/* Host emulation of the catchment kernels (wdpm_amd/csrc/wdpm_pond_catchments.hip, compiled with WDPM_PONDS_EMULATION), after the
 * pattern of tests/rims_emu_main.cpp: the kernels' own source runs as 256 threads per block, in lockstep wherever lanes talk to each
 * other, blocks one after another, atomics as host atomics - so the relaxed loads and stores of the jump rounds really race.  Built
 * with -fsanitize=address,undefined by tests/test_pond_catchments_emulation.py: a window lane that reads outside a raster is found
 * here, on a CPU.  Labels and wet masks come from a row-major flood fill, every buffer has its exact size, and basin raster, table
 * and counts are held against a plain loop that walks every cell's descent one step at a time.
 *
 *   catch_emu ROWS COLS DENSITY SEED [ROWS_PER_WAVE]     (file rows and columns; odd seeds label at 0.001 m, even ones at 0;
 *                                                         seed 0: a serpentine channel into one pond cell, DENSITY unused)
 */
#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_pond_catchments.hip"
#include "pond_emu.h"

/* ---- the raster, the reference ------------------------------------------------------------------------------------------- */
static Raster make_raster(int R, int C, double density, int seed) {
  Raster a = blank(R, C, seed);
  srand(seed);
  const int period = 5 + seed % 4;
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      const size_t i = a.at(r, c);
      /* 5 % NODATA with water on it, a few NaN elevations; quarter-metre steps down slanted valleys that repeat, so that descents
       * are several cells long, cross every seam and meet ties on the way; both zeros */
      const int e = rand() % 100;
      const int ramp = abs((r * 2 + c) % (2 * period) - period);
      a.dem[i] = e < 5 ? INFINITY : e < 6 ? NAN : e < 9 ? (e & 1 ? -0.0 : 0.0) : 100.0 + (ramp + e % 2) * 0.25;
      const double u = unit_random();
      a.w[i] = unit_random() < density ? (u < 0.1 ? 3.0 + u * 40 : u * 0.02) : 0.0;
      if (rand() % 20 == 0) a.w[i] = 0.0005;                                    /* a film: below either threshold's reach or not */
      if (rand() % 100 == 0) a.w[i] = -0.25;                                    /* never added to a level */
      if (rand() % 100 == 0) a.w[i] = NAN;                                      /* never a pond cell, never added */
    }
  return a;
}

/* a channel that snakes through every other row between high walls and ends in one pond cell: thousands of hops */
static Raster make_serpentine(int R, int C) {
  Raster a = blank(R, C, 0);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) a.dem[a.at(r, c)] = 5000.0 + r;
  int k = 0, r = 1, c = 1, dir = 1;
  for (;;) {
    a.dem[a.at(r, c)] = 1000.0 - 0.125 * k++;
    const int cn = c + dir;
    if (cn >= 1 && cn <= C) { c = cn; continue; }
    if (r + 2 > R) break;
    a.dem[a.at(r + 1, c)] = 1000.0 - 0.125 * k++;
    r += 2;
    dir = -dir;
  }
  a.dem[a.at(r, c)] -= 1.0;                         /* the pond's surface stays below the channel's last cell */
  a.w[a.at(r, c)] = 0.5;
  return a;
}

struct Reference {
  std::vector<int> basin;
  std::vector<wdpm_pond_catchment> table;
  long long slope, pit, unponded, longest;
};

/* the definitions of include/wdpm_pond_catchments.h as they are written */
static Reference reference(const Raster &a, const std::vector<int> &labels, int n) {
  const Geom g = a.g;
  auto has_level = [&](int r, int c) { return a.inside(r, c) && a.dem[a.at(r, c)] < INFINITY; };
  auto level = [&](int r, int c) {
    const size_t i = a.at(r, c);
    return key_of(labels[i] ? a.dem[i] + a.w[i] : a.w[i] > 0 ? a.dem[i] + a.w[i] : a.dem[i]);
  };
  auto receiver = [&](int r, int c, int &rr, int &rc) {
    bool found = false;
    unsigned long long best = 0;
    for (int di = -1; di <= 1; di++)
      for (int dj = -1; dj <= 1; dj++) {
        if ((!di && !dj) || !has_level(r + di, c + dj)) continue;
        const unsigned long long k = level(r + di, c + dj);
        if (!found || k < best) { found = true; best = k; rr = r + di; rc = c + dj; }
      }
    return found && best < level(r, c);
  };
  Reference ref;
  ref.basin.assign(a.w.size(), -1);
  ref.table.assign((size_t)n, wdpm_pond_catchment());
  ref.slope = ref.pit = ref.unponded = ref.longest = 0;
  std::vector<unsigned long long> head((size_t)n, 0ull);
  for (auto &t : ref.table) { t.catch_cells = t.inflow_cells = 0; t.row_min = t.col_min = INT_MAX; t.row_max = t.col_max = -1; }
  auto box = [&](int k, int r, int c) {
    wdpm_pond_catchment &t = ref.table[(size_t)k - 1];
    t.row_min = std::min(t.row_min, r); t.row_max = std::max(t.row_max, r);
    t.col_min = std::min(t.col_min, c); t.col_max = std::max(t.col_max, c);
  };
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      const size_t i = a.at(r, c);
      if (!has_level(r, c)) continue;
      if (labels[i]) { ref.basin[i] = labels[i]; box(labels[i], r, c); continue; }
      ref.slope++;
      int pr = r, pc = c, nr = 0, nc = 0, end = 0;
      long long hops = 0;
      for (;;) {                                         /* one step at a time */
        if (labels[a.at(pr, pc)]) { end = labels[a.at(pr, pc)]; break; }
        if (!receiver(pr, pc, nr, nc)) { ref.pit += hops == 0; break; }
        if (hops == 0 && labels[a.at(nr, nc)]) ref.table[(size_t)labels[a.at(nr, nc)] - 1].inflow_cells++;
        pr = nr; pc = nc; hops++;
      }
      ref.longest = std::max(ref.longest, hops);
      ref.basin[i] = end;
      if (!end) { ref.unponded++; continue; }
      ref.table[(size_t)end - 1].catch_cells++;
      head[(size_t)end - 1] = std::max(head[(size_t)end - 1], level(r, c));
      box(end, r, c);
    }
  for (int k = 0; k < n; k++) {
    double d = -INFINITY;
    if (ref.table[k].catch_cells) {
      const unsigned long long key = head[k], b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
      memcpy(&d, &b, 8);
    }
    ref.table[k].head_level = d;
  }
  return ref;
}

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s ROWS COLS DENSITY SEED [ROWS_PER_WAVE]\n", argv[0]);
    return 2;
  }
  const int seed = atoi(argv[4]);
  const Raster a = seed ? make_raster(atoi(argv[1]), atoi(argv[2]), atof(argv[3]), seed) : make_serpentine(atoi(argv[1]), atoi(argv[2]));
  const int forced_rpw = argc > 5 ? atoi(argv[5]) : 0;
  emu_init();

  const Geom g = a.g;
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  const std::vector<unsigned long long> masks = wet_masks(g, labels);  /* exact sizes: the sanitizer sees a stray index */
  std::vector<PondRow> ponds((size_t)n);
  for (auto &p : ponds) { p.row_min = p.col_min = INT_MAX; p.row_max = p.col_max = -1; }
  long long pond_cells = 0, levelled = 0;
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      levelled += a.dem[a.at(r, c)] < INFINITY;
      const int L = labels[a.at(r, c)];
      if (!L) continue;
      pond_cells++;
      PondRow &p = ponds[(size_t)L - 1];
      p.row_min = std::min(p.row_min, r); p.row_max = std::max(p.row_max, r);
      p.col_min = std::min(p.col_min, c); p.col_max = std::max(p.col_max, c);
    }

  const int cells = g.rows * g.ncp;
  std::vector<int> link((size_t)cells, 12345678);
  std::vector<CatchRow> table((size_t)n);
  CatchStatus st;
  memset(&st, 0, sizeof st);
  const Waves wv = waves_over(g, g.rows, forced_rpw);
  const int rpw = wv.rpw, nwaves = wv.n;
  if (n) launch(blocks_for(n, kBlock), [&] { catch_init_kernel(table.data(), ponds.data(), n); });
  launch(blocks_for(nwaves, kWaves), [&] {
    catch_receivers_kernel(a.w.data(), a.dem.data(), masks.data(), labels.data(), g, rpw, nwaves, link.data(), table.data(), &st);
  });
  int rounds = 0;
  for (;;) {                                                           /* the host's loop of wdpm_catch_label */
    for (int b = 0; b < kCatchBatch; b++, rounds++)
      launch(blocks_for(cells, kBlock), [&] { catch_jump_kernel(link.data(), cells, rounds, &st); });
    if (st.unres[rounds - 1] == 0u) break;
    if (rounds >= kCatchRoundCap) { printf("still unresolved after %d rounds\n", rounds); return 1; }
  }
  launch(blocks_for(nwaves, kWaves), [&] {
    catch_tally_kernel(a.w.data(), a.dem.data(), masks.data(), g, rpw, nwaves, link.data(), table.data(), &st);
  });
  if (n) launch(blocks_for(n, kBlock), [&] { catch_finish_kernel(table.data(), n); });

  const Reference ref = reference(a, labels, n);
  long long bad_basin = 0, bad_rows = 0, caught = 0;
  for (int i = 0; i < cells; i++) bad_basin += link[(size_t)i] != ref.basin[(size_t)i];
  for (int k = 0; k < n; k++) {
    bad_rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_catchment)) != 0;
    caught += ref.table[k].catch_cells;
  }
  const bool counts = (long long)st.slope == ref.slope && (long long)st.pit == ref.pit && (long long)st.unponded == ref.unponded;
  const bool identity = pond_cells + caught + ref.unponded == levelled;
  printf("%dx%d density %.2f min_depth %.3f: N %d slope %lld pits %lld unponded %lld caught %lld longest descent %lld rounds %d "
         "rows per wave %d  basin mismatches %lld table mismatches %lld counts %s identity %s\n",
         a.R, a.C, atof(argv[3]), a.min_depth, n, ref.slope, ref.pit, ref.unponded, caught, ref.longest, rounds, rpw, bad_basin,
         bad_rows, counts ? "agree" : "DIFFER", identity ? "holds" : "BROKEN");
  return bad_basin != 0 || bad_rows != 0 || !counts || !identity;
}
