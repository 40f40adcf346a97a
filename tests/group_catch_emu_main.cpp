/* Host emulation of the pond catchments over row blocks (include/wdpm_group_pond_catchments.h), after tests/group_rims_emu_main.cpp:
 * a raster is cut into strips of rows, each strip a rank.  A rank gets the whole-raster labels and wet masks of its owned rows and of
 * the one row beyond either end - and rubbish for the DEM and the water of those two rows, which nobody may read - and runs the
 * catchment kernels' own source (wdpm_amd/csrc/wdpm_pond_catchments.hip, compiled with WDPM_PONDS_EMULATION) as 256 host threads per
 * block on buffers of exact size, in the order of wdpm_group_catch_label: every rank's seam keys; the neighbours' keys, receivers and
 * jump rounds over its owned rows (relaxed atomics that really race, links that start as rubbish); the exits followed by the real
 * wdpm_catch_stitch::resolve; remote slots, tally and finish; wdpm_catch_stitch::merge.  Basin raster, table and counts are held
 * against the plain loop of tests/catch_emu_main.cpp, which walks every descent of the WHOLE raster one step at a time.  Built with
 * -fsanitize=address,undefined by tests/test_group_catch_stitch.py; nothing here is loaded into python.
 *
 *   group_catch_emu noise ROWS COLS DENSITY SEED STRIP [ROWS_PER_WAVE]   (file rows and columns; STRIP owned rows per rank)
 *   group_catch_emu snake ROWS COLS STRIP [ROWS_PER_WAVE]    a channel down and up the columns: every boundary, both directions
 *   group_catch_emu stitch                                   resolve, remote_labels and merge alone on hand-written seam tables
 */
#define main catch_emu_whole_raster_main      /* the whole-raster program's rasters and its reference, without its main */
#include "catch_emu_main.cpp"
#undef main
#include "../wdpm_amd/csrc/wdpm_catch_stitch.h"
#include "../wdpm_amd/csrc/wdpm_rims_merge.h"

namespace cs = wdpm_catch_stitch;

/* a channel that runs down column 1, up column 3, down column 5 ... between high walls and ends in one pond cell: it crosses
 * every boundary between strips once per column it runs along, downwards and upwards in turn */
static Raster make_snake(int R, int C) {
  Raster a = blank(R, C, 0);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) a.dem[a.at(r, c)] = 9000.0 + r + c;
  int k = 0, r = 1, c = 1, dir = 1;
  for (;;) {
    a.dem[a.at(r, c)] = 4000.0 - 0.125 * k++;
    const int rn = r + dir;
    if (rn >= 1 && rn <= R) { r = rn; continue; }
    if (c + 2 > C) break;
    a.dem[a.at(r, c + 1)] = 4000.0 - 0.125 * k++;
    c += 2;
    dir = -dir;
  }
  a.dem[a.at(r, c)] -= 1.0;                         /* the pond's surface stays below the channel's last cell */
  a.w[a.at(r, c)] = 0.5;
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
  if (out.size() > 1 && out.front().hi == 0) {                        /* the first rank owns more than the border row */
    out[1].lo = 0;
    out.erase(out.begin());
  }
  return out;
}

struct Rank {
  Geom g;
  int v0;
  CatchRows rw;
  std::vector<double> w, dem;
  std::vector<int> labels, link, slot_of, label, exit_basin, remote;
  std::vector<unsigned long long> masks, keys, nkeys;
  std::vector<CatchRow> table;
  CatchStatus st;
  int rounds, rpw, nwaves;
  long long held;
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
  k.labels.resize(k.w.size());
  for (int r = 0; r < k.g.rows; r++)
    for (int c = 0; c < ncp; c++) {
      const size_t i = (size_t)r * ncp + c, j = a.at(v0 + r, c);
      const bool own = r >= ra && r < rb;
      k.w[i] = own ? a.w[j] : 1e300;          /* a halo row's water and DEM are not current between exchanges: never read */
      k.dem[i] = own ? a.dem[j] : -1e300;
      k.labels[i] = whole[j];
    }
  k.masks = wet_masks(k.g, k.labels);
  /* the slots the rim pass leaves: the whole-raster labels of the owned rows in first-cell order (one slot per label here: what
   * the device calls local ponds that are one pond share a slot as well), then the foreign ones */
  std::vector<int> beside, own;
  for (int r = ra; r < rb; r++)
    for (int c = 0; c < ncp; c++) {
      const int L = k.labels[(size_t)r * ncp + c];
      if (L && std::find(k.label.begin(), k.label.end(), L) == k.label.end()) k.label.push_back(L);
    }
  if (!first) {
    beside.insert(beside.end(), k.labels.begin(), k.labels.begin() + ncp);
    own.insert(own.end(), k.labels.begin() + (size_t)ra * ncp, k.labels.begin() + (size_t)(ra + 1) * ncp);
  }
  if (!last) {
    beside.insert(beside.end(), k.labels.end() - ncp, k.labels.end());
    own.insert(own.end(), k.labels.begin() + (size_t)(rb - 1) * ncp, k.labels.begin() + (size_t)rb * ncp);
  }
  std::vector<int> foreign;
  wdpm_rims_merge::foreign_labels(beside.data(), beside.size(), own.data(), own.size(), foreign);
  k.label.insert(k.label.end(), foreign.begin(), foreign.end());
  k.held = (long long)k.label.size();
  k.slot_of.assign((size_t)nwhole + 1, 0x7f7f7f7f);
  for (size_t s = 0; s < k.label.size(); s++) k.slot_of[(size_t)k.label[s]] = (int)s;
  k.table.resize((size_t)k.held + 2 * (size_t)ncp);
  k.link.assign(k.w.size(), 12345678);       /* rubbish: a jump round that followed it would leave the raster */
  k.keys.assign((size_t)2 * ncp, 0x1234ull);
  k.nkeys.assign((size_t)2 * ncp, 0x1234ull);
  k.exit_basin.assign((size_t)2 * ncp, 7);
  memset(&k.st, 0, sizeof k.st);
  k.rounds = 0;
  const Waves wv = waves_over(k.g, rb - ra, forced_rpw);
  k.rpw = wv.rpw;
  k.nwaves = wv.n;
  k.rw.ra = ra;
  k.rw.rb = rb;
  k.rw.halo = (first ? 0 : 1) | (last ? 0 : 2);
}

static int run_raster(const Raster &a, int strip, int forced_rpw, const char *what) {
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  const Geom g = a.g;
  const int ncp = g.ncp;
  const std::vector<Strip> strips = cut(g.rows, strip);
  const size_t nr = strips.size();
  std::vector<Rank> ranks(nr);
  for (size_t i = 0; i < nr; i++) make_rank(ranks[i], a, labels, n, strips[i], i == 0, i + 1 == nr, forced_rpw);

  /* every rank's seam keys (and a terminal into the links of its neighbours' rows) */
  for (Rank &k : ranks)
    launch(blocks_for(2 * ncp, kBlock), [&] { catch_seam_keys_kernel(k.w.data(), k.dem.data(), k.g, k.rw.halo, k.keys.data(), k.link.data()); });
  /* the neighbours' keys, receivers, jump rounds */
  for (size_t i = 0; i < nr; i++) {
    Rank &k = ranks[i];
    if (i > 0) std::copy(ranks[i - 1].keys.begin() + ncp, ranks[i - 1].keys.end(), k.nkeys.begin());
    if (i + 1 < nr) std::copy(ranks[i + 1].keys.begin(), ranks[i + 1].keys.begin() + ncp, k.nkeys.begin() + ncp);
    k.rw.nkeys = k.nkeys.data();
    k.rw.slot_of = k.slot_of.data();
    k.rw.exit_basin = k.exit_basin.data();
    const long long cap = (long long)k.table.size();
    const int cells = k.g.rows * ncp;
    launch(blocks_for(cap, kBlock), [&] { catch_init_rows_kernel(k.table.data(), cap); });
    launch(blocks_for(k.nwaves, kWaves), [&] {
      catch_receivers_rows_kernel(k.w.data(), k.dem.data(), k.masks.data(), k.labels.data(), k.g, k.rpw, k.nwaves, k.link.data(),
                                  k.table.data(), &k.st, k.rw);
    });
    for (;;) {
      for (int b = 0; b < kCatchBatch; b++, k.rounds++)
        launch(blocks_for(cells, kBlock), [&] { catch_jump_kernel(k.link.data(), cells, k.rounds, &k.st); });
      if (k.st.unres[k.rounds - 1] == 0u) break;
      if (k.rounds >= kCatchRoundCap) { printf("still unresolved after %d rounds\n", k.rounds); return 1; }
    }
  }
  /* the exits */
  std::vector<cs::RankLinks> links(nr);
  for (size_t i = 0; i < nr; i++) {
    const Rank &k = ranks[i];
    links[i].top = k.link.data() + ncp;
    links[i].bottom = k.link.data() + (size_t)(k.g.rows - 2) * ncp;
  }
  cs::Resolved res;
  std::string err;
  if (cs::resolve(links, ncp, res, err)) { printf("resolve failed: %s\n", err.c_str()); return 1; }
  /* the pond table as the label call has merged it by now: every pond's own box */
  std::vector<wdpm_pond> ponds((size_t)n);
  for (auto &p : ponds) { p.cells = 0; p.row_min = p.col_min = INT_MAX; p.row_max = p.col_max = -1; }
  long long pond_cells = 0, levelled = 0;
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < ncp; c++) {
      levelled += a.dem[a.at(r, c)] < INFINITY;
      const int L = labels[a.at(r, c)];
      if (!L) continue;
      pond_cells++;
      wdpm_pond &p = ponds[(size_t)L - 1];
      p.cells++;
      p.row_min = std::min(p.row_min, r); p.row_max = std::max(p.row_max, r);
      p.col_min = std::min(p.col_min, c); p.col_max = std::max(p.col_max, c);
    }
  /* remote slots, tally, finish */
  long long remote = 0;
  for (size_t i = 0; i < nr; i++) {
    Rank &k = ranks[i];
    k.exit_basin = res.exit_basin[i];
    k.rw.exit_basin = k.exit_basin.data();
    cs::remote_labels(k.exit_basin, ncp, ponds.data(), k.v0, k.v0 + k.g.rows - 1, k.remote);
    for (int L : k.remote)                                 /* what the row ranges say, the rank's own slots must say too */
      if (std::find(k.label.begin(), k.label.end(), L) != k.label.end()) { printf("pond %d is held and remote\n", L); return 1; }
    for (int v : k.exit_basin)
      if (v < cs::kPit && v != cs::kNone && k.slot_of[(size_t)(-1 - v)] == 0x7f7f7f7f &&
          std::find(k.remote.begin(), k.remote.end(), -1 - v) == k.remote.end()) { printf("pond %d has no slot\n", -1 - v); return 1; }
    if (k.remote.size() > (size_t)2 * ncp) { printf("%zu remote ponds on %d columns\n", k.remote.size(), ncp); return 1; }
    const int nremote = (int)k.remote.size(), base = (int)k.held;
    if (nremote) launch(blocks_for(nremote, kBlock), [&] { catch_remote_slots_kernel(k.remote.data(), nremote, base, k.slot_of.data()); });
    launch(blocks_for(k.nwaves, kWaves), [&] {
      catch_tally_rows_kernel(k.w.data(), k.dem.data(), k.masks.data(), k.g, k.rpw, k.nwaves, k.link.data(), k.table.data(), &k.st, k.rw);
    });
    const long long slots = k.held + nremote;              /* the rims' slots, then the remote ones */
    if (slots) launch(blocks_for(slots, kBlock), [&] { catch_finish_kernel(k.table.data(), slots); });
    for (long long s = k.held; s < slots; s++) remote += k.table[(size_t)s].catch_cells > 0;      /* the remote slots that took a cell */
  }
  /* the merge */
  std::vector<cs::RankCatch> rc(nr);
  for (size_t i = 0; i < nr; i++) {
    const Rank &k = ranks[i];
    rc[i] = {reinterpret_cast<const wdpm_pond_catchment *>(k.table.data()), k.label.data(), k.held + (long long)k.remote.size(), k.remote.data(),
             (long long)k.remote.size(), k.v0,
             (long long)k.st.slope, (long long)k.st.pit, (long long)k.st.unponded, (long long)k.st.exits, k.rounds};
  }
  std::vector<wdpm_pond_catchment> table((size_t)n);
  cs::Totals tot;
  if (cs::merge(rc, n, ponds.data(), table.data(), tot, err)) { printf("merge failed: %s\n", err.c_str()); return 1; }

  const Reference ref = reference(a, labels, n);
  long long bad_basin = 0, bad_rows = 0, caught = 0;
  for (size_t i = 0; i < nr; i++)
    for (int r = strips[i].lo; r <= strips[i].hi; r++)
      for (int c = 0; c < ncp; c++)
        bad_basin += ranks[i].link[(size_t)(r - ranks[i].v0) * ncp + c] != ref.basin[a.at(r, c)];
  for (int k = 0; k < n; k++) {
    bad_rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_catchment)) != 0;
    caught += table[(size_t)k].catch_cells;
  }
  const bool counts = tot.slope == ref.slope && tot.pit == ref.pit && tot.unponded == ref.unponded;
  const bool identity = pond_cells + caught + tot.unponded == levelled;
  printf("%s %dx%d strips of %d rows (%zu ranks): N %d slope %lld pits %lld unponded %lld caught %lld longest descent %lld rounds %lld "
         "rows per wave %d exits %lld crossings %lld remote %lld  basin mismatches %lld table mismatches %lld counts %s identity %s\n",
         what, a.R, a.C, strip, nr, n, ref.slope, ref.pit, ref.unponded, caught, ref.longest, tot.rounds, ranks[0].rpw, tot.exits,
         res.crossings, remote, bad_basin, bad_rows, counts ? "agree" : "DIFFER", identity ? "holds" : "BROKEN");
  return bad_basin != 0 || bad_rows != 0 || !counts || !identity;
}

/* ---- resolve, remote_labels and merge alone ---------------------------------------------------------------------------------- */
#define CHECK(cond) do { if (!(cond)) { printf("stitch check failed: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

struct Seams {
  int ncp;
  std::vector<std::vector<int>> top, bottom;
  Seams(size_t nr, int ncp_) : ncp(ncp_), top(nr, std::vector<int>((size_t)ncp_, cs::kNone)), bottom(top) {}
  std::vector<cs::RankLinks> links() const {
    std::vector<cs::RankLinks> l(top.size());
    for (size_t i = 0; i < top.size(); i++) l[i] = {top[i].data(), bottom[i].data()};
    return l;
  }
  int down(int col) const { return cs::exit_code(1, col, ncp); }
  int up(int col) const { return cs::exit_code(0, col, ncp); }
};

static int run_stitch_checks() {
  cs::Resolved res;
  std::string err;
  const int ncp = 8;
  CHECK(cs::codes_fit(100, ncp) && cs::codes_fit((1ll << 31) - 2 * ncp - 2, ncp) && !cs::codes_fit((1ll << 31) - 2 * ncp - 1, ncp));
  CHECK(cs::is_exit(cs::exit_code(1, ncp - 1, ncp), ncp) && !cs::is_exit(cs::exit_code(1, ncp - 1, ncp) + 1, ncp) && !cs::is_exit(cs::kNone, ncp) &&
        !cs::is_exit(cs::kPit, ncp));
  { /* back and forth across one boundary three times, into pond 7 */
    Seams s(2, ncp);
    s.bottom[0][1] = s.down(2); s.top[1][2] = s.up(3); s.bottom[0][3] = s.down(4); s.top[1][4] = s.up(5); s.bottom[0][5] = s.down(6);
    s.top[1][6] = -1 - 7;
    CHECK(cs::resolve(s.links(), ncp, res, err) == 0 && res.crossings == 5);
    for (int c : {2, 4, 6}) CHECK(res.exit_basin[0][(size_t)ncp + c] == -8);       /* rank 0's exits downwards */
    for (int c : {1, 3, 5}) CHECK(res.exit_basin[1][(size_t)c] == -8);             /* rank 1's exits upwards */
    CHECK(res.exit_basin[0][0] == cs::kNone && res.exit_basin[1][(size_t)ncp + 6] == cs::kNone && res.exit_basin[0][(size_t)ncp + 7] == cs::kNone);
  }
  { /* down through eight ranks and back up, into pond 3 of rank 0 */
    Seams s(8, ncp);
    s.bottom[0][1] = s.down(1);
    for (int r = 1; r < 7; r++) s.top[r][1] = s.down(1);
    s.top[7][1] = s.up(2);
    for (int r = 6; r >= 1; r--) s.bottom[r][2] = s.up(2);
    s.bottom[0][2] = -1 - 3;
    CHECK(cs::resolve(s.links(), ncp, res, err) == 0 && res.crossings == 14);
    for (int r = 0; r < 7; r++) CHECK(res.exit_basin[(size_t)r][(size_t)ncp + 1] == -4);
    for (int r = 1; r < 8; r++) CHECK(res.exit_basin[(size_t)r][2] == -4);
  }
  { /* onto a pit, onto a pond the rank holds, onto one it has no slot for yet; a rank of one row */
    Seams s(3, ncp);
    s.top[1][1] = cs::kPit; s.top[1][2] = -1 - 5; s.top[1][3] = s.down(3); s.top[2][3] = -1 - 9;
    s.bottom[1] = s.top[1];
    std::vector<cs::RankLinks> l = s.links();
    l[1].bottom = l[1].top;                                 /* one owned row: the same cells */
    CHECK(cs::resolve(l, ncp, res, err) == 0 && res.crossings == 1);
    CHECK(res.exit_basin[0][(size_t)ncp + 1] == cs::kPit && res.exit_basin[0][(size_t)ncp + 2] == -6 && res.exit_basin[0][(size_t)ncp + 3] == -10);
    std::vector<int> remote;
    wdpm_pond boxes[9];                                     /* pond k in rows 2 k - 2 .. 2 k - 1: pond 5 in 8 .. 9, pond 9 in 16 .. 17 */
    for (int k = 1; k <= 9; k++) { boxes[k - 1] = wdpm_pond(); boxes[k - 1].row_min = 2 * k - 2; boxes[k - 1].row_max = 2 * k - 1; }
    cs::remote_labels(res.exit_basin[0], ncp, boxes, 0, 8, remote);         /* a view that ends in pond 5's first row */
    CHECK(remote == std::vector<int>({9}));
    cs::remote_labels(res.exit_basin[0], ncp, boxes, 0, 7, remote);
    CHECK(remote == std::vector<int>({5, 9}));
    cs::remote_labels(res.exit_basin[0], ncp, boxes, 9, 16, remote);        /* ... and one that begins in its last and ends in pond 9's first */
    CHECK(remote.empty());
    cs::remote_labels(res.exit_basin[0], ncp, boxes, 18, 30, remote);
    CHECK(remote == std::vector<int>({5, 9}));
  }
  { /* a cycle, an exit out of the raster, a link that is no terminal: messages, not loops */
    Seams s(2, ncp);
    s.bottom[0][1] = s.down(1); s.top[1][1] = s.up(1);
    err.clear();
    CHECK(cs::resolve(s.links(), ncp, res, err) == 1 && err.find("cycle") != std::string::npos);
    Seams t(2, ncp);
    t.bottom[0][1] = t.up(1);
    err.clear();
    CHECK(cs::resolve(t.links(), ncp, res, err) == 1 && err.find("leaves the raster") != std::string::npos);
    Seams u(2, ncp);
    u.top[1][1] = u.down(1);
    err.clear();
    CHECK(cs::resolve(u.links(), ncp, res, err) == 1 && err.find("leaves the raster") != std::string::npos);
    Seams v(2, ncp);
    v.top[1][4] = 17;
    err.clear();
    CHECK(cs::resolve(v.links(), ncp, res, err) == 1 && err.find("still on its way") != std::string::npos);
  }
  { /* an empty raster: no rank, and ranks without a level anywhere */
    CHECK(cs::resolve(std::vector<cs::RankLinks>(), ncp, res, err) == 0 && res.crossings == 0 && res.exit_basin.empty());
    Seams s(3, ncp);
    CHECK(cs::resolve(s.links(), ncp, res, err) == 0 && res.crossings == 0);
    for (const auto &eb : res.exit_basin)
      for (int v : eb) CHECK(v == cs::kNone);
    cs::Totals tot;
    CHECK(cs::merge(std::vector<cs::RankCatch>(), 0, nullptr, nullptr, tot, err) == 0 && tot.slope == 0 && tot.rounds == 0);
  }
  { /* the merge: counts add, the head through the order-preserving image, boxes with the pond's own, an empty slot changes nothing */
    const wdpm_pond ponds[2] = {{5, 5, 3, 0, 1.0, 5, 6, 5, 6}, {20, 2, 1, 0, 0.5, 20, 20, 2, 2}};
    const wdpm_pond_catchment r0[] = {{4, 2, -0.0, 2, 3, 4, 9}, {0, 0, -INFINITY, INT_MAX, -1, INT_MAX, -1}};
    const wdpm_pond_catchment r1[] = {{0, 1, -INFINITY, INT_MAX, -1, INT_MAX, -1}, {6, 0, 0.0, 1, 4, 1, 3}, {2, 1, 7.5, 1, 1, 7, 8}};
    const int l0[] = {1, 2}, l1[] = {2, 1}, m1[] = {1};      /* rank 1 holds pond 1 twice: in a slot of the rims' and in a remote one */
    std::vector<cs::RankCatch> ranks = {{r0, l0, 2, nullptr, 0, 0, 10, 1, 2, 3, 4}, {r1, l1, 3, m1, 1, 10, 20, 2, 3, 4, 8}};
    wdpm_pond_catchment t[2];
    cs::Totals tot;
    CHECK(cs::merge(ranks, 2, ponds, t, tot, err) == 0);
    CHECK(tot.slope == 30 && tot.pit == 3 && tot.unponded == 5 && tot.exits == 7 && tot.rounds == 8);
    CHECK(t[0].catch_cells == 12 && t[0].inflow_cells == 3 && t[0].head_level == 7.5);
    CHECK(t[0].row_min == 2 && t[0].row_max == 14 && t[0].col_min == 1 && t[0].col_max == 9);
    CHECK(t[1].catch_cells == 0 && t[1].inflow_cells == 1 && std::isinf(t[1].head_level) && t[1].head_level < 0);
    CHECK(t[1].row_min == 20 && t[1].row_max == 20 && t[1].col_min == 2 && t[1].col_max == 2);
    /* +0.0 in the lower rank beats -0.0 in the upper one, bit for bit */
    const wdpm_pond_catchment z0[] = {{1, 0, -0.0, 5, 5, 5, 5}}, z1[] = {{1, 0, 0.0, 0, 0, 6, 6}};
    const int one[] = {1};
    ranks = {{z0, one, 1, nullptr, 0, 0, 0, 0, 0, 0, 0}, {z1, one, 1, nullptr, 0, 6, 0, 0, 0, 0, 0}};
    CHECK(cs::merge(ranks, 1, ponds, t, tot, err) == 0 && t[0].head_level == 0.0 && !std::signbit(t[0].head_level) && t[0].catch_cells == 2);
    /* counts that leave int64, a label outside the table: a message, not a wrong number */
    const wdpm_pond_catchment big[] = {{INT64_MAX - 1, 0, 1.0, 5, 5, 5, 5}}, two[] = {{2, 0, 1.0, 5, 5, 5, 5}};
    const wdpm_pond_catchment ibig[] = {{0, INT64_MAX, -INFINITY, INT_MAX, -1, INT_MAX, -1}}, ione[] = {{0, 1, -INFINITY, INT_MAX, -1, INT_MAX, -1}};
    const int nine[] = {9};
    ranks = {{big, one, 1, nullptr, 0, 0, 0, 0, 0, 0, 0}, {two, one, 1, nullptr, 0, 6, 0, 0, 0, 0, 0}};
    err.clear();
    CHECK(cs::merge(ranks, 1, ponds, t, tot, err) == 1 && err.find("catch_cells") != std::string::npos && err.find("overflows") != std::string::npos);
    ranks = {{ibig, one, 1, nullptr, 0, 0, 0, 0, 0, 0, 0}, {ione, one, 1, nullptr, 0, 6, 0, 0, 0, 0, 0}};
    err.clear();
    CHECK(cs::merge(ranks, 1, ponds, t, tot, err) == 1 && err.find("inflow_cells") != std::string::npos);
    ranks = {{two, one, 1, nullptr, 0, 0, INT64_MAX, 0, 0, 0, 0}, {two, one, 1, nullptr, 0, 6, 1, 0, 0, 0, 0}};
    err.clear();
    CHECK(cs::merge(ranks, 1, ponds, t, tot, err) == 1 && err.find("slope_cells") != std::string::npos);
    ranks = {{two, one, 1, nine, 1, 0, 0, 0, 0, 0, 0}};
    err.clear();
    CHECK(cs::merge(ranks, 1, ponds, t, tot, err) == 1 && !err.empty());
  }
  printf("stitch checks ok\n");
  return 0;
}

int main(int argc, char **argv) {
  emu_init();
  if (argc == 2 && !strcmp(argv[1], "stitch")) return run_stitch_checks();
  if (argc >= 5 && !strcmp(argv[1], "snake"))
    return run_raster(make_snake(atoi(argv[2]), atoi(argv[3])), atoi(argv[4]), argc > 5 ? atoi(argv[5]) : 0, "snake");
  if (argc >= 7 && !strcmp(argv[1], "noise"))
    return run_raster(make_raster(atoi(argv[2]), atoi(argv[3]), atof(argv[4]), atoi(argv[5])), atoi(argv[6]), argc > 7 ? atoi(argv[7]) : 0,
                      "noise");
  fprintf(stderr, "usage: %s noise ROWS COLS DENSITY SEED STRIP [ROWS_PER_WAVE] | snake ROWS COLS STRIP [ROWS_PER_WAVE] | stitch\n", argv[0]);
  return 2;
}
