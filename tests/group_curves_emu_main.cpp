/* Host emulation of the pond stage curves over row blocks (include/wdpm_group_pond_curves.h), after tests/group_outlets_emu_main.cpp: a
 * raster is cut into strips of rows, each strip a rank.  A rank gets the DEM and the whole-raster basins of its owned rows - and
 * rubbish for the DEM and the basins of the one row beyond either end, which nobody may read (the curve kernels take no water at all) -
 * one slot per basin > 0 of its view, the merged pour key in every slot's outlet row, and runs the curve kernels' own source
 * (wdpm_amd/csrc/wdpm_pond_curves.hip, compiled with WDPM_PONDS_EMULATION) as 256 host threads per block on buffers of exact size, in
 * the order of wdpm_group_curves_label: init, bed and the keys' way down on every rank; the real wdpm_curves_merge::bed; the keys' way
 * up and the stage pass on every rank; the real wdpm_curves_merge::merge.  Table and counts are held against the plain double loop of
 * tests/curves_emu_main.cpp over all cells and stages of the WHOLE raster, the group's own counts against loops over that table.
 * Built with -fsanitize=address,undefined by tests/test_group_curves_merge.py; nothing here is loaded into python.
 *
 *   group_curves_emu noise ROWS COLS DENSITY SEED STRIP [ROWS_PER_WAVE]   (file rows and columns; STRIP owned rows per rank)
 *   group_curves_emu merge                                  bed and merge alone on hand-written slot tables
 */
#define main curves_emu_whole_raster_main       /* the whole-raster program's rasters and its reference, without its main */
#include "curves_emu_main.cpp"
#undef main
#include "../wdpm_amd/csrc/wdpm_curves_merge.h"

#include <set>

namespace cm = wdpm_curves_merge;

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
  CurveRows rw;
  std::vector<double> dem;
  std::vector<int> basins, slot_of, label, remote;
  std::vector<OutletRow> outlets;               /* per slot: the pour key as the group's outlet pass leaves it */
  std::vector<unsigned long long> down, up;
  std::vector<CurveRow> table;
  CurveStatus st;
  int rpw, nwaves;
  long long slots;
};

static void make_rank(Rank &k, const Raster &a, const std::vector<int> &whole, const std::vector<wdpm_pond_outlet> &pour, int nwhole, Strip st,
                      int forced_rpw) {
  const int P = a.g.rows, ncp = a.g.ncp;
  const int v0 = st.lo > 0 ? st.lo - 1 : 0, v1 = st.hi < P - 1 ? st.hi + 1 : P - 1;
  k.g.rows = v1 - v0 + 1;
  k.g.ncp = ncp;
  k.g.nsc = a.g.nsc;
  k.g.nseg = k.g.rows * k.g.nsc;
  const int ra = st.lo - v0, rb = ra + (st.hi - st.lo + 1);
  /* the slots the catchment pass leaves: one for every basin > 0 of the view, halo rows included, in the order the cells meet them
   * from the last row up (no order is promised); the last third of them plays the remote ponds, whose labels lie in a list of
   * their own */
  std::vector<int> all;
  for (int r = k.g.rows - 1; r >= 0; r--)
    for (int c = 0; c < ncp; c++) {
      const int L = whole[a.at(v0 + r, c)];
      if (L > 0 && std::find(all.begin(), all.end(), L) == all.end()) all.push_back(L);
    }
  k.dem.resize((size_t)k.g.rows * ncp);
  k.basins.resize(k.dem.size());
  for (int r = 0; r < k.g.rows; r++)
    for (int c = 0; c < ncp; c++) {
      const size_t i = (size_t)r * ncp + c, j = a.at(v0 + r, c);
      const bool own = r >= ra && r < rb;
      /* a halo row is never read: ground far below every bed, and basins that are some slot of the rank, so that a stray read
       * changes a curve rather than the program's exit status alone */
      k.dem[i] = own ? a.dem[j] : -1e300;
      k.basins[i] = own ? whole[j] : all.empty() ? 0x7f7f7f7f : all[(size_t)c % all.size()];
    }
  const size_t nremote = all.size() / 3;
  k.label.assign(all.begin(), all.end() - nremote);
  k.remote.assign(all.end() - nremote, all.end());
  k.slots = (long long)all.size();
  k.slot_of.assign((size_t)nwhole + 1, 0x7f7f7f7f);
  k.outlets.assign((size_t)k.slots, OutletRow());
  for (size_t s = 0; s < all.size(); s++) {
    k.slot_of[(size_t)all[s]] = (int)s;
    const double level = pour[(size_t)all[s] - 1].pour_level;
    memset(&k.outlets[s], 0x5a, sizeof(OutletRow));
    k.outlets[s].pour_key = level < INFINITY ? key_of(level) : ~0ull;
  }
  k.table.resize((size_t)k.slots);
  k.down.assign((size_t)k.slots, 0x5555ull);
  k.up.assign((size_t)k.slots, 0x5555ull);
  memset(&k.st, 0, sizeof k.st);
  const Waves wv = waves_over(k.g, rb - ra, forced_rpw);
  k.rpw = wv.rpw;
  k.nwaves = wv.n;
  k.rw.ra = ra;
  k.rw.rb = rb;
  k.rw.slot_of = k.slot_of.data();
}

static int run_raster(const Raster &a, int strip, int forced_rpw, const char *what) {
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  const Geom g = a.g;
  const int ncp = g.ncp;
  const std::vector<int> basin = basins_of(a, labels);
  const std::vector<wdpm_pond_outlet> outlets = pour_levels(a, basin, n);
  const std::vector<Strip> strips = cut(g.rows, strip);
  const size_t nr = strips.size();
  std::vector<Rank> ranks(nr);
  for (size_t i = 0; i < nr; i++) make_rank(ranks[i], a, basin, outlets, n, strips[i], forced_rpw);

  /* (A) init, bed, the keys side by side */
  for (Rank &k : ranks) {
    if (!k.slots) continue;
    launch(blocks_for(k.slots * kCurveWords, kBlock), [&] { curves_init_rows_kernel(k.table.data(), k.slots, k.outlets.data()); });
    launch(blocks_for(k.nwaves, kWaves), [&] { curves_bed_rows_kernel(k.dem.data(), k.basins.data(), k.g, k.rpw, k.nwaves, k.table.data(), k.rw); });
    launch(blocks_for(k.slots, kBlock), [&] { curves_bed_down_kernel(k.table.data(), k.slots, k.down.data()); });
  }
  std::vector<cm::Rank> mr(nr);
  std::vector<unsigned long long *> up(nr);
  for (size_t i = 0; i < nr; i++) {
    Rank &k = ranks[i];
    mr[i].label = k.label.data();
    mr[i].slots = k.slots;
    mr[i].remote = k.remote.data();
    mr[i].nremote = (long long)k.remote.size();
    mr[i].key = k.down.data();
    mr[i].rows = reinterpret_cast<const cm::SlotRow *>(k.table.data());
    up[i] = k.up.data();
  }
  std::vector<unsigned long long> bed_key((size_t)n);
  std::string err;
  long long split_basins = 0;
  if (cm::bed(mr, n, bed_key.data(), up, split_basins, err)) { printf("bed failed: %s\n", err.c_str()); return 1; }

  /* (B) the merged keys, the stage pass */
  bool deep = false;
  for (Rank &k : ranks) {
    if (!k.slots) continue;
    launch(blocks_for(k.slots, kBlock), [&] { curves_bed_up_kernel(k.table.data(), k.slots, k.up.data()); });
    launch(blocks_for(k.nwaves, kWaves), [&] {
      curves_stages_rows_kernel(k.dem.data(), k.basins.data(), k.g, k.rpw, k.nwaves, k.table.data(), &k.st, k.rw);
    });
    deep = deep || k.st.deep != 0;
  }
  std::vector<wdpm_pond_curve> table((size_t)n);
  cm::Totals tot;
  if (cm::merge(mr, n, bed_key.data(), table.data(), tot, err)) { printf("merge failed: %s\n", err.c_str()); return 1; }

  const Reference ref = reference(a, basin, outlets, n);
  /* the group's own counts from the whole raster: the strips that hold a cell of a pond's basin; the lowest strip that holds a cell at
   * the bed; the strips that hold a cell below the top of a pond that has one */
  std::vector<int> strip_of((size_t)g.rows, 0);
  for (size_t i = 0; i < nr; i++)
    for (int r = strips[i].lo; r <= strips[i].hi; r++) strip_of[(size_t)r] = (int)i;
  std::vector<std::set<int>> holders((size_t)n), stagers((size_t)n);
  std::vector<int> bed_strip((size_t)n, -1);
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < ncp; c++) {
      const int k = basin[a.at(r, c)];
      if (k <= 0) continue;
      const wdpm_pond_curve &t = ref.table[(size_t)k - 1];
      const double e = a.dem[a.at(r, c)];
      holders[(size_t)k - 1].insert(strip_of[(size_t)r]);
      if (key_of(e) == key_of(t.bed_level) && bed_strip[(size_t)k - 1] < 0) bed_strip[(size_t)k - 1] = strip_of[(size_t)r];
      if (t.top_level < INFINITY && key_of(e) < key_of(t.top_level)) stagers[(size_t)k - 1].insert(strip_of[(size_t)r]);
    }
  long long bad_rows = 0, split = 0, remote = 0;
  for (int k = 0; k < n; k++) {
    bad_rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_curve)) != 0;
    split += holders[(size_t)k].size() > 1;
    std::set<int> away = stagers[(size_t)k];
    away.erase(bed_strip[(size_t)k]);
    remote += !away.empty();
  }
  const bool counts = tot.ponds == n && tot.no_curve == ref.no_curve && tot.flat == ref.flat && tot.stage_cells == ref.stage_cells &&
                      deep == ref.deep && split_basins == split && tot.remote_beds == remote;
  printf("%s %dx%d strips of %d rows (%zu ranks): N %d without curve %lld flat %lld stage cells %lld rows per wave %d "
         "split basins %lld remote beds %lld  table mismatches %lld counts %s\n",
         what, a.R, a.C, strip, nr, n, ref.no_curve, ref.flat, ref.stage_cells, ranks[0].rpw, split_basins, tot.remote_beds, bad_rows,
         counts ? "agree" : "DIFFER");
  return bad_rows != 0 || !counts || ref.deep;
}

/* ---- bed and merge alone ----------------------------------------------------------------------------------------------------- */
#define CHECK(cond) do { if (!(cond)) { printf("merge check failed: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static cm::SlotRow slot_row(unsigned long long bed_key, double top, unsigned long long cells_from, unsigned long long q_each) {
  cm::SlotRow r;
  r.bed_key = bed_key;
  r.top_level = top;
  for (int s = 0; s < WDPM_CURVE_STAGES; s++) {      /* cumulative, as the device leaves them */
    r.cells[s] = cells_from ? cells_from + (unsigned long long)s : 0ull;
    r.q[s] = r.cells[s] * q_each;
  }
  return r;
}

static int run_merge_checks() {
  std::string err;
  cm::Totals tot;
  long long split = -1;
  const unsigned long long k1 = key_of(1.0), k2 = key_of(2.0), kz = key_of(-0.0), kp = key_of(0.0);
  CHECK(kz < kp && cm::level_from_key(k2) == 2.0 && std::signbit(cm::level_from_key(kz)) && !std::signbit(cm::level_from_key(kp)));
  /* three ranks.  pond 1: rank 0 and rank 2 hold cells, the bed (1.0) in rank 2, stage cells in both - a remote bed; rank 1 holds a
   * slot of it and no cell.  pond 2: ranks 0 and 1 tie at -0.0: rank 0 is the lowest holder, rank 1 has stage cells
   * - remote.  pond 3: no outlet, rank 1 alone.  pond 4: flat (top == bed), rank 2 alone, through a remote slot.
   * pond 5: bed and all stage cells in rank 1, rank 0 holds cells at or above the top only - split, not remote. */
  const int l0[] = {1, 2, 5}, l1[] = {5, 1, 3, 2}, l2[] = {1}, m2[] = {4};
  const unsigned long long key0[] = {k2, kz, k2}, key1[] = {k1, cm::kNoBed, k2, kz}, key2[] = {k1, k2};
  unsigned long long up0[3], up1[4], up2[2];
  std::vector<cm::Rank> ranks(3);
  ranks[0] = {l0, 3, nullptr, 0, key0, nullptr};
  ranks[1] = {l1, 4, nullptr, 0, key1, nullptr};
  ranks[2] = {l2, 2, m2, 1, key2, nullptr};
  std::vector<unsigned long long *> up = {up0, up1, up2};
  unsigned long long bk[5];
  CHECK(cm::bed(ranks, 5, bk, up, split, err) == 0);
  CHECK(bk[0] == k1 && bk[1] == kz && bk[2] == k2 && bk[3] == k2 && bk[4] == k1 && split == 3);
  CHECK(up0[0] == k1 && up0[1] == kz && up0[2] == k1 && up1[0] == k1 && up1[1] == k1 && up1[2] == k2 && up1[3] == kz && up2[0] == k1 && up2[1] == k2);
  const cm::SlotRow r0[] = {slot_row(k1, 9.0, 3, 10), slot_row(kz, 4.0, 1, 7), slot_row(k1, 3.0, 0, 0)};
  const cm::SlotRow r1[] = {slot_row(k1, 3.0, 2, 5), slot_row(k1, 9.0, 0, 0), slot_row(k2, INFINITY, 0, 0), slot_row(kz, 4.0, 2, 7)};
  const cm::SlotRow r2[] = {slot_row(k1, 9.0, 5, 10), slot_row(k2, 2.0, 0, 0)};
  ranks[0].rows = r0;
  ranks[1].rows = r1;
  ranks[2].rows = r2;
  wdpm_pond_curve t[5];
  CHECK(cm::merge(ranks, 5, bk, t, tot, err) == 0);
  CHECK(t[0].bed_level == 1.0 && t[0].top_level == 9.0 && t[0].cells[0] == 8 && t[0].cells[15] == 38 && t[0].q[15] == 380);
  CHECK(t[1].bed_level == 0.0 && std::signbit(t[1].bed_level) && t[1].top_level == 4.0 && t[1].cells[0] == 3 && t[1].q[0] == 21);
  CHECK(t[2].bed_level == 2.0 && std::isinf(t[2].top_level) && t[2].top_level > 0 && t[2].cells[15] == 0 && t[2].q[15] == 0);
  CHECK(t[3].bed_level == 2.0 && t[3].top_level == 2.0 && t[3].cells[15] == 0);
  CHECK(t[4].bed_level == 1.0 && t[4].top_level == 3.0 && t[4].cells[0] == 2 && t[4].cells[15] == 17 && t[4].q[15] == 85);
  CHECK(tot.ponds == 5 && tot.no_curve == 1 && tot.flat == 1 && tot.stage_cells == 38 + 33 + 17 && tot.remote_beds == 2);
  /* a pond without an outlet keeps its bed and gets zeros, whatever a slot's arrays hold */
  const cm::SlotRow junk[] = {slot_row(k1, INFINITY, 4, 4)};
  const int one[] = {1}, nine[] = {9};
  const unsigned long long ka[] = {k1};
  unsigned long long upa[1], upb[1];
  up = {upa, upb};
  ranks.resize(2);
  ranks[0] = {one, 1, nullptr, 0, ka, junk};
  ranks[1] = {one, 1, nullptr, 0, ka, junk};
  CHECK(cm::bed(ranks, 1, bk, up, split, err) == 0 && split == 1 && upa[0] == k1 && upb[0] == k1);
  CHECK(cm::merge(ranks, 1, bk, t, tot, err) == 0 && t[0].bed_level == 1.0 && t[0].cells[15] == 0 && t[0].q[15] == 0 && tot.no_curve == 1 &&
        tot.remote_beds == 0);
  /* sums that leave 64 bits, tops that differ, a pond nobody holds, a label outside the table: a message, not a wrong number */
  cm::SlotRow qa = slot_row(k1, 5.0, 1, 1), qb = slot_row(k1, 5.0, 1, 1), qc = slot_row(k1, 6.0, 1, 1);
  qa.q[7] = UINT64_MAX - 5;
  qb.q[7] = 6;
  ranks[0].rows = &qa;
  ranks[1].rows = &qb;
  err.clear();
  CHECK(cm::merge(ranks, 1, bk, t, tot, err) == 1 && err.find("q of") != std::string::npos && err.find("overflows") != std::string::npos);
  qa.q[7] = 8;
  qa.cells[15] = (unsigned long long)INT64_MAX;
  err.clear();
  CHECK(cm::merge(ranks, 1, bk, t, tot, err) == 1 && err.find("cells of") != std::string::npos && err.find("overflows") != std::string::npos);
  qa.cells[15] = 16;
  err.clear();
  CHECK(cm::merge(ranks, 1, bk, t, tot, err) == 0 && t[0].q[7] == 14 && t[0].cells[15] == 32);
  ranks[1].rows = &qc;
  err.clear();
  CHECK(cm::merge(ranks, 1, bk, t, tot, err) == 1 && err.find("top level") != std::string::npos);
  const unsigned long long none[] = {cm::kNoBed};
  ranks[0].key = none;
  ranks[1].key = none;
  err.clear();
  CHECK(cm::bed(ranks, 1, bk, up, split, err) == 1 && err.find("no bed") != std::string::npos);
  ranks[0] = {nine, 1, nullptr, 0, ka, &qa};
  err.clear();
  CHECK(cm::bed(ranks, 1, bk, up, split, err) == 1 && !err.empty());
  err.clear();
  CHECK(cm::merge(ranks, 1, bk, t, tot, err) == 1 && !err.empty());
  /* no rank, no pond */
  CHECK(cm::bed(std::vector<cm::Rank>(), 0, nullptr, up, split, err) == 0 && split == 0);
  CHECK(cm::merge(std::vector<cm::Rank>(), 0, nullptr, nullptr, tot, err) == 0 && tot.ponds == 0 && tot.no_curve == 0);
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
