/* Host emulation of the pond outlets over row blocks (include/wdpm_group_pond_outlets.h), after tests/group_catch_emu_main.cpp: a
 * raster is cut into strips of rows, each strip a rank.  A rank gets the whole-raster basins of its owned rows and of the one row
 * beyond either end, the level keys of those two rows as their owners write them - and rubbish for their DEM and water, which nobody
 * may read - and runs the outlet kernels' own source (wdpm_amd/csrc/wdpm_pond_outlets.hip, compiled with WDPM_PONDS_EMULATION) as 256
 * host threads per block on buffers of exact size, in the order of wdpm_group_outlets_label: init, passes and the keys' way down on
 * every rank; the real wdpm_outlets_merge::pour; the keys' way up, locate and finish on every rank; the real
 * wdpm_outlets_merge::merge.  Table and counts are held against the plain double loop of tests/outlets_emu_main.cpp over all pairs of
 * the WHOLE raster, the group's own counts against loops over that table.  Built with -fsanitize=address,undefined by
 * tests/test_group_outlets_merge.py; nothing here is loaded into python.
 *
 *   group_outlets_emu noise ROWS COLS DENSITY SEED STRIP [ROWS_PER_WAVE]   (file rows and columns; STRIP owned rows per rank)
 *   group_outlets_emu merge                                  pour and merge alone on hand-written slot tables
 */
#define main outlets_emu_whole_raster_main      /* the whole-raster program's rasters and its reference, without its main */
#include "outlets_emu_main.cpp"
#undef main
#include "../wdpm_amd/csrc/wdpm_outlets_merge.h"

#include <set>

namespace om = wdpm_outlets_merge;

/* ---- one rank ---------------------------------------------------------------------------------------------------------------- */
struct Strip { int lo, hi; };     /* owned rows of the padded raster */

static std::vector<Strip> cut(int P, int strip) {
  std::vector<Strip> out;
  for (int lo = 0; lo < P; lo += strip) out.push_back({lo, std::min(lo + strip, P) - 1});
  if (out.size() > 1 && out.back().hi - out.back().lo + 1 < 2) {      /* a view holds three rows at least */
    out[out.size() - 2].hi = out.back().hi;
    out.pop_back();
  }
  if (out.size() > 1 && out.front().hi == 0) {                        /* the first rank owns more than the border row */
    out[1].lo = 0;
    out.erase(out.begin());
  }
  return out;
}

struct Rank {
  Geom g;
  int v0;
  OutRows rw;
  std::vector<double> w, dem;
  std::vector<int> basins, slot_of, label, remote;
  std::vector<unsigned long long> nkeys, okeys, up;
  std::vector<OutletRow> table;
  OutletStatus st;
  int rpw, nwaves;
  long long slots;
};

static void make_rank(Rank &k, const Raster &a, const std::vector<int> &whole, int nwhole, Strip st, bool first, bool last, int forced_rpw) {
  const int P = a.g.rows, ncp = a.g.ncp;
  const int v0 = st.lo > 0 ? st.lo - 1 : 0, v1 = st.hi < P - 1 ? st.hi + 1 : P - 1;
  k.v0 = v0;
  k.g.rows = v1 - v0 + 1;
  k.g.ncp = ncp;
  k.g.nsc = a.g.nsc;
  k.g.nseg = k.g.rows * k.g.nsc;
  const int ra = st.lo - v0, rb = ra + (st.hi - st.lo + 1);
  k.w.resize((size_t)k.g.rows * ncp);
  k.dem.resize(k.w.size());
  k.basins.resize(k.w.size());
  for (int r = 0; r < k.g.rows; r++)
    for (int c = 0; c < ncp; c++) {
      const size_t i = (size_t)r * ncp + c, j = a.at(v0 + r, c);
      const bool own = r >= ra && r < rb;
      k.w[i] = own ? a.w[j] : 1e300;          /* a halo row's water and DEM are not current between exchanges: never read */
      k.dem[i] = own ? a.dem[j] : -1e300;
      k.basins[i] = whole[j];                 /* the halo rows' basins are their owners', as the group sends them up */
    }
  /* the level keys of the rows beside the rank's own, as the catchment pass leaves them: no level's key where there is none */
  k.nkeys.assign((size_t)2 * ncp, 0x1234ull);
  for (int side = 0; side < 2; side++) {
    if (side ? last : first) continue;
    const int r = side ? v1 : v0;
    for (int c = 0; c < ncp; c++) {
      const size_t j = a.at(r, c);
      k.nkeys[(size_t)side * ncp + c] = a.dem[j] < INFINITY ? key_of(level_of(a, j)) : ~0ull;
    }
  }
  /* the slots the catchment pass leaves: one for every basin > 0 of the view, in the order the cells meet them from the last row
   * up (no order is promised); the last third of them plays the remote ponds, whose labels lie in a list of their own */
  std::vector<int> all;
  for (int r = k.g.rows - 1; r >= 0; r--)
    for (int c = 0; c < ncp; c++) {
      const int L = k.basins[(size_t)r * ncp + c];
      if (L > 0 && std::find(all.begin(), all.end(), L) == all.end()) all.push_back(L);
    }
  const size_t nremote = all.size() / 3;
  k.label.assign(all.begin(), all.end() - nremote);
  k.remote.assign(all.end() - nremote, all.end());
  k.slots = (long long)all.size();
  k.slot_of.assign((size_t)nwhole + 1, 0x7f7f7f7f);
  for (size_t s = 0; s < all.size(); s++) k.slot_of[(size_t)all[s]] = (int)s;
  k.table.resize((size_t)k.slots);
  k.okeys.assign((size_t)2 * k.slots, 0x5555ull);
  k.up.assign((size_t)k.slots, 0x5555ull);
  memset(&k.st, 0, sizeof k.st);
  const Waves wv = waves_over(k.g, rb - ra, forced_rpw);
  k.rpw = wv.rpw;
  k.nwaves = wv.n;
  k.rw.ra = ra;
  k.rw.rb = rb;
  k.rw.halo = (first ? 0 : 1) | (last ? 0 : 2);
  k.rw.nkeys = k.nkeys.data();
  k.rw.slot_of = k.slot_of.data();
}

static int run_raster(const Raster &a, int strip, int forced_rpw, const char *what) {
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  const Geom g = a.g;
  const int ncp = g.ncp;
  const std::vector<int> basin = basins_of(a, labels);
  const std::vector<Strip> strips = cut(g.rows, strip);
  const size_t nr = strips.size();
  std::vector<Rank> ranks(nr);
  for (size_t i = 0; i < nr; i++) make_rank(ranks[i], a, basin, n, strips[i], i == 0, i + 1 == nr, forced_rpw);

  /* (A) init, passes, keys and divide counts */
  for (Rank &k : ranks) {
    if (!k.slots) continue;
    launch(blocks_for(k.slots, kBlock), [&] { outlet_init_kernel(k.table.data(), k.slots); });
    launch(blocks_for(k.nwaves, kWaves), [&] {
      outlet_passes_rows_kernel(k.w.data(), k.dem.data(), k.basins.data(), k.g, k.rpw, k.nwaves, k.table.data(), k.rw);
    });
    launch(blocks_for(k.slots, kBlock), [&] { outlet_pour_down_kernel(k.table.data(), k.slots, k.okeys.data()); });
  }
  std::vector<om::Rank> mr(nr);
  std::vector<unsigned long long *> up(nr);
  for (size_t i = 0; i < nr; i++) {
    Rank &k = ranks[i];
    mr[i].label = k.label.data();
    mr[i].slots = k.slots;
    mr[i].remote = k.remote.data();
    mr[i].nremote = (long long)k.remote.size();
    mr[i].key = k.okeys.data();
    mr[i].divide = k.okeys.data() + k.slots;
    mr[i].rows = reinterpret_cast<const om::SlotRow *>(k.table.data());
    mr[i].row_shift = k.v0;
    mr[i].own_lo = strips[i].lo;
    mr[i].own_rows = strips[i].hi - strips[i].lo + 1;
    up[i] = k.up.data();
  }
  std::vector<unsigned long long> pour_key((size_t)n);
  std::vector<long long> divide((size_t)n);
  std::string err;
  if (om::pour(mr, n, pour_key.data(), divide.data(), up, err)) { printf("pour failed: %s\n", err.c_str()); return 1; }

  /* (B) the merged keys, locate, finish */
  bool deep = false;
  for (Rank &k : ranks) {
    if (!k.slots) continue;
    launch(blocks_for(k.slots, kBlock), [&] { outlet_pour_up_kernel(k.table.data(), k.slots, k.up.data()); });
    launch(blocks_for(k.nwaves, kWaves), [&] {
      outlet_locate_rows_kernel(k.w.data(), k.dem.data(), k.basins.data(), k.g, k.rpw, k.nwaves, k.table.data(), &k.st, k.rw);
    });
    launch(blocks_for(k.slots, kBlock), [&] { outlet_finish_rows_kernel(k.table.data(), k.slots, k.basins.data(), ncp); });
    deep = deep || k.st.deep != 0;
  }
  std::vector<wdpm_pond_outlet> table((size_t)n);
  om::Totals tot;
  if (om::merge(mr, n, ncp, pour_key.data(), divide.data(), table.data(), tot, err)) { printf("merge failed: %s\n", err.c_str()); return 1; }

  const Reference ref = reference(a, basin, n);
  /* the group's own counts from the whole raster: the strip of a row; the strips that hold a divide cell or a fill cell of a pond */
  std::vector<int> strip_of((size_t)g.rows, 0);
  for (size_t i = 0; i < nr; i++)
    for (int r = strips[i].lo; r <= strips[i].hi; r++) strip_of[(size_t)r] = (int)i;
  std::vector<std::set<int>> holders((size_t)n);
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < ncp; c++) {
      const int k = basin[a.at(r, c)];
      if (k <= 0 || ref.table[(size_t)k - 1].to_basin < 0) continue;
      bool hold = key_of(level_of(a, a.at(r, c))) < key_of(ref.table[(size_t)k - 1].pour_level);
      for (int di = -1; di <= 1 && !hold; di++)
        for (int dj = -1; dj <= 1; dj++)
          if ((di || dj) && a.inside(r + di, c + dj) && basin[a.at(r + di, c + dj)] >= 0 && basin[a.at(r + di, c + dj)] != k) hold = true;
      if (hold) holders[(size_t)k - 1].insert(strip_of[(size_t)r]);
    }
  long long bad_rows = 0, filled = 0, seam = 0, split = 0;
  for (int k = 0; k < n; k++) {
    bad_rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_outlet)) != 0;
    filled += ref.table[k].fill_cells;
    if (ref.table[k].to_basin >= 0) seam += strip_of[(size_t)ref.table[k].from_row] != strip_of[(size_t)ref.table[k].to_row];
    split += holders[(size_t)k].size() > 1;
  }
  const bool counts = tot.ponds == n && tot.no_outlet == ref.no_outlet && tot.to_land == ref.to_land && tot.divide_cells == ref.divide &&
                      deep == ref.deep && tot.seam_outlets == seam && tot.split_ponds == split;
  printf("%s %dx%d strips of %d rows (%zu ranks): N %d without outlet %lld to land %lld divide %lld filled %lld rows per wave %d "
         "seam outlets %lld split ponds %lld  table mismatches %lld counts %s\n",
         what, a.R, a.C, strip, nr, n, ref.no_outlet, ref.to_land, ref.divide, filled, ranks[0].rpw, tot.seam_outlets, tot.split_ponds,
         bad_rows, counts ? "agree" : "DIFFER");
  return bad_rows != 0 || !counts || ref.deep;
}

/* ---- pour and merge alone ---------------------------------------------------------------------------------------------------- */
#define CHECK(cond) do { if (!(cond)) { printf("merge check failed: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static om::SlotRow slot_row(unsigned long long pair, int to_basin, unsigned long long fill_cells, unsigned long long fill_q) {
  om::SlotRow r;
  r.pour_key = r.spare = 0ull;
  r.pair = pair;
  r.to_basin = to_basin;
  r.reserved = 0;
  r.divide_cells = 0ull;
  r.fill_cells = fill_cells;
  r.fill_q = fill_q;
  return r;
}

static int run_merge_checks() {
  const int ncp = 10;
  std::string err;
  om::Totals tot;
  const unsigned long long k5 = key_of(5.0), k7 = key_of(7.0), kz = key_of(-0.0);
  CHECK(om::level_from_key(k5) == 5.0 && std::signbit(om::level_from_key(kz)) && om::level_from_key(key_of(INFINITY)) == INFINITY);
  /* two ranks of ten rows: rank 0 owns rows 0 .. 9 (its view starts at row 0), rank 1 rows 10 .. 19 (its view at row 9).
   * pond 1: a tie - both ranks hold a pass at 5.0; pond 2: only rank 1 holds a pass, rank 0 holds fill cells alone;
   * pond 3: no pass anywhere; pond 4: rank 0's pass leads downwards into rank 1's first row and into basin 0 */
  const int l0[] = {1, 2, 3, 4}, l1[] = {2}, m1[] = {1, 3};
  const unsigned long long key0[] = {k5, om::kNone, om::kNone, kz}, div0[] = {3, 0, 0, 1};
  const unsigned long long key1[] = {k7, k5, om::kNone}, div1[] = {2, 4, 0};
  unsigned long long up0[4], up1[3];
  std::vector<om::Rank> ranks(2);
  ranks[0] = {l0, 4, nullptr, 0, key0, div0, nullptr, 0, 0, 10};
  ranks[1] = {l1, 3, m1, 2, key1, div1, nullptr, 9, 10, 10};
  std::vector<unsigned long long *> up = {up0, up1};
  unsigned long long pk[4];
  long long dv[4];
  CHECK(om::pour(ranks, 4, pk, dv, up, err) == 0);
  CHECK(pk[0] == k5 && pk[1] == k7 && pk[2] == om::kNone && pk[3] == kz);
  CHECK(dv[0] == 7 && dv[1] == 2 && dv[2] == 0 && dv[3] == 1);
  CHECK(up0[0] == k5 && up0[1] == k7 && up0[2] == om::kNone && up0[3] == kz && up1[0] == k7 && up1[1] == k5 && up1[2] == om::kNone);
  /* locate: rank 0 offers for pond 1 at view cell (4, 3) towards the right, for pond 4 at (9, 2) down-left; rank 1 offers for pond 1
   * at its view cell (2, 1) upwards and for pond 2 at (5, 5) up-right */
  const om::SlotRow r0[] = {slot_row((4 * ncp + 3) * 8 + 4, 2, 5, 500), slot_row(om::kNone, -1, 6, 600), slot_row(om::kNone, -1, 0, 0),
                            slot_row((9 * ncp + 2) * 8 + 5, 0, 0, 0)};
  const om::SlotRow r1[] = {slot_row((5 * ncp + 5) * 8 + 2, 1, 1, 100), slot_row((2 * ncp + 1) * 8 + 1, 2, 2, 250), slot_row(om::kNone, -1, 0, 0)};
  ranks[0].rows = r0;
  ranks[1].rows = r1;
  wdpm_pond_outlet t[4];
  CHECK(om::merge(ranks, 4, ncp, pk, dv, t, tot, err) == 0);
  CHECK(t[0].pour_level == 5.0 && t[0].from_row == 4 && t[0].from_col == 3 && t[0].to_row == 4 && t[0].to_col == 4 && t[0].to_basin == 2);
  CHECK(t[0].divide_cells == 7 && t[0].fill_cells == 7 && t[0].fill_q == 750 && t[0].reserved == 0);        /* the lower rank's pair won */
  CHECK(t[1].pour_level == 7.0 && t[1].from_row == 14 && t[1].from_col == 5 && t[1].to_row == 13 && t[1].to_col == 6 && t[1].to_basin == 1);
  CHECK(t[1].divide_cells == 2 && t[1].fill_cells == 7 && t[1].fill_q == 700);                              /* rank 0 filled, rank 1 found */
  CHECK(std::isinf(t[2].pour_level) && t[2].pour_level > 0 && t[2].from_row == -1 && t[2].from_col == -1 && t[2].to_row == -1 && t[2].to_col == -1 &&
        t[2].to_basin == -1 && t[2].divide_cells == 0 && t[2].fill_cells == 0 && t[2].fill_q == 0);
  CHECK(std::signbit(t[3].pour_level) && t[3].pour_level == 0.0 && t[3].from_row == 9 && t[3].from_col == 2 && t[3].to_row == 10 && t[3].to_col == 1 &&
        t[3].to_basin == 0);
  CHECK(tot.ponds == 4 && tot.no_outlet == 1 && tot.to_land == 1 && tot.divide_cells == 10 && tot.seam_outlets == 1 && tot.split_ponds == 2);
  /* sums that leave 64 bits, a key nobody found the pass of, a label outside the table: a message, not a wrong number */
  const int one[] = {1}, nine[] = {9};
  const unsigned long long ka[] = {k5}, da[] = {1}, dbig[] = {(unsigned long long)INT64_MAX};
  const om::SlotRow qa[] = {slot_row(8, 0, 1, UINT64_MAX - 5)}, qb[] = {slot_row(om::kNone, -1, 1, 6)}, qc[] = {slot_row(om::kNone, -1, (unsigned long long)INT64_MAX, 1)};
  unsigned long long upa[1], upb[1];
  up = {upa, upb};
  ranks[0] = {one, 1, nullptr, 0, ka, da, qa, 0, 0, 10};
  ranks[1] = {one, 1, nullptr, 0, ka, da, qb, 9, 10, 10};
  CHECK(om::pour(ranks, 1, pk, dv, up, err) == 0 && dv[0] == 2);
  err.clear();
  CHECK(om::merge(ranks, 1, ncp, pk, dv, t, tot, err) == 1 && err.find("fill_q") != std::string::npos && err.find("overflows") != std::string::npos);
  ranks[1].rows = qc;
  err.clear();
  CHECK(om::merge(ranks, 1, ncp, pk, dv, t, tot, err) == 1 && err.find("fill_cells") != std::string::npos);
  ranks[0].rows = qb;
  ranks[1].rows = qb;
  err.clear();
  CHECK(om::merge(ranks, 1, ncp, pk, dv, t, tot, err) == 1 && err.find("no rank found") != std::string::npos);
  ranks[0].divide = dbig;
  err.clear();
  CHECK(om::pour(ranks, 1, pk, dv, up, err) == 1 && err.find("divide_cells") != std::string::npos);
  ranks[0] = {nine, 1, nullptr, 0, ka, da, qa, 0, 0, 10};
  err.clear();
  CHECK(om::pour(ranks, 1, pk, dv, up, err) == 1 && !err.empty());
  /* no rank, no pond */
  CHECK(om::pour(std::vector<om::Rank>(), 0, nullptr, nullptr, up, err) == 0);
  CHECK(om::merge(std::vector<om::Rank>(), 0, ncp, nullptr, nullptr, nullptr, tot, err) == 0 && tot.ponds == 0 && tot.no_outlet == 0);
  printf("merge checks ok\n");
  return 0;
}

int main(int argc, char **argv) {
  emu_init();
  if (argc == 2 && !strcmp(argv[1], "merge")) return run_merge_checks();
  if (argc >= 7 && !strcmp(argv[1], "noise"))
    return run_raster(make_raster(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atoi(argv[5])), atoi(argv[6]), argc > 7 ? atoi(argv[7]) : 0,
                      "noise");
  fprintf(stderr, "usage: %s noise ROWS COLS DENSITY SEED STRIP [ROWS_PER_WAVE] | merge\n", argv[0]);
  return 2;
}
