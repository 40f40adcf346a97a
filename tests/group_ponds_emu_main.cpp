/* The pond inventory over row blocks on the host (include/wdpm_group_ponds.h), under the sanitizers of
 * tests/test_group_ponds_stitch.py, over what tests/ponds_emu_main.cpp runs on: the stand-ins for the HIP device language, the
 * raster, the flood fill and the launches of a label call (tests/ponds_label_emu.h).
 *
 *   group_ponds_emu stitch                                   the product's stitch (wdpm_amd/csrc/wdpm_ponds_stitch.h) alone: strips of
 *                                                            a raster are labelled by the flood fill, joined by the stitch and held
 *                                                            against the flood fill of the whole raster
 *   group_ponds_emu kernels ROWS COLS STRIPS DENSITY SEED [ROWS_PER_WAVE]
 *                                                            the kernels' own source per strip: the seven existing kernels, the seam
 *                                                            kernel, the stitch, the mapping table kernel
 */
#include <functional>

#include "ponds_label_emu.h"
#include "../wdpm_amd/csrc/wdpm_ponds_stitch.h"

static_assert(sizeof(PondRow) == sizeof(wdpm_pond), "the finished device table is a wdpm_pond table");

/* rows [v0, v1] of `a` as a raster of its own: its first and last row are the dry border to whoever labels it */
struct Strip {
  int own_lo, own_hi, v0;
  Raster a;
};

static std::vector<Strip> cut(const Raster &whole, int n) {
  const int P = whole.g.rows;
  std::vector<Strip> out;
  for (int k = 0; k < n; k++) {
    Strip s;
    s.own_lo = (int)((long long)P * k / n);
    s.own_hi = (int)((long long)P * (k + 1) / n) - 1;
    s.v0 = s.own_lo > 0 ? s.own_lo - 1 : 0;
    const int v1 = s.own_hi < P - 1 ? s.own_hi + 1 : P - 1;
    s.a.g = whole.g;
    s.a.g.rows = v1 - s.v0 + 1;
    s.a.g.nseg = s.a.g.rows * s.a.g.nsc;
    s.a.R = s.a.g.rows - 2;
    s.a.C = whole.C;
    s.a.min_depth = whole.min_depth;
    s.a.w.assign(whole.w.begin() + (size_t)s.v0 * whole.g.ncp, whole.w.begin() + (size_t)(v1 + 1) * whole.g.ncp);
    s.a.dem.assign(whole.dem.begin() + (size_t)s.v0 * whole.g.ncp, whole.dem.begin() + (size_t)(v1 + 1) * whole.g.ncp);
    out.push_back(s);
  }
  return out;
}

static Raster raster_from(int R, int C, const std::function<double(int, int)> &depth) {
  Raster a = blank(R, C, 0);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      a.dem[a.at(r, c)] = 100.0;
      a.w[a.at(r, c)] = depth(r - 1, c - 1);
    }
  return a;
}

/* strips' labels (already whole-raster numbers, or local ones to be sent through the maps) and tables against the whole flood fill */
static long long compare(const Raster &whole, const std::vector<Strip> &strips, const std::vector<std::vector<int>> &labels,
                         const std::vector<std::vector<PondRow>> &tables, const wdpm_stitch::Result &res, bool labels_are_local,
                         const char *what) {
  std::vector<int> ref_labels;
  std::vector<PondRow> ref_table;
  flood_fill(whole, ref_labels, ref_table);
  const int ncp = whole.g.ncp;
  long long label_bad = 0, table_bad = (long long)ref_table.size() != res.ponds;
  for (size_t k = 0; k < strips.size(); k++)
    for (int r = strips[k].own_lo; r <= strips[k].own_hi; r++)
      for (int c = 0; c < ncp; c++) {
        int l = labels[k][(size_t)(r - strips[k].v0) * ncp + c];
        if (labels_are_local && l) l = res.map[k][(size_t)l - 1];
        label_bad += l != ref_labels[(size_t)r * ncp + c];
      }
  std::vector<wdpm_pond> merged((size_t)res.ponds);
  memset(merged.data(), 0, merged.size() * sizeof(wdpm_pond));
  std::string err;
  for (size_t k = 0; k < strips.size(); k++) {
    std::vector<wdpm_pond> local(tables[k].size());
    memcpy(local.data(), tables[k].data(), local.size() * sizeof(wdpm_pond));
    if (wdpm_stitch::fold_table(local.data(), res.map[k], strips[k].v0, merged.data(), err)) { printf("%s: %s\n", what, err.c_str()); return 1; }
  }
  for (size_t i = 0; i < ref_table.size() && i < merged.size(); i++) table_bad += memcmp(&ref_table[i], &merged[i], sizeof(PondRow)) != 0;
  long long local_sum = 0;
  for (const auto &t : tables) local_sum += (long long)t.size();
  const bool counts_bad = res.local_ponds != local_sum || res.ponds != res.local_ponds - res.merged;
  printf("%s: %dx%d in %zu strips: N %lld (reference %zu) local %lld merged %lld stitch unions %lld  label mismatches %lld  "
         "table mismatches %lld%s\n", what, whole.R, whole.C, strips.size(), res.ponds, ref_table.size(), res.local_ponds, res.merged,
         res.unions, label_bad, table_bad, counts_bad ? "  COUNTS DISAGREE" : "");
  return label_bad + table_bad + counts_bad;
}

/* ---- the stitch alone ---------------------------------------------------------------------------------------------------- */
static long long stitch_case(const Raster &whole, int n, const char *what) {
  const std::vector<Strip> strips = cut(whole, n);
  std::vector<std::vector<int>> labels(n);
  std::vector<std::vector<PondRow>> tables(n);
  std::vector<wdpm_stitch::RankSeams> seams(n);
  const int ncp = whole.g.ncp;
  for (int k = 0; k < n; k++) {
    flood_fill(strips[k].a, labels[k], tables[k]);
    seams[k].n = (long long)tables[k].size();
    seams[k].top = labels[k].data() + ncp;
    seams[k].bottom = labels[k].data() + (size_t)(strips[k].a.g.rows - 2) * ncp;
  }
  wdpm_stitch::Result res;
  std::string err;
  if (wdpm_stitch::stitch(seams, ncp, res, err)) { printf("%s: %s\n", what, err.c_str()); return 1; }
  return compare(whole, strips, labels, tables, res, true, what);
}

static int stitch_main() {
  long long bad = 0;
  const int R = 300, C = 500;
  int seed = 11;
  for (double density : {0.30, 0.41, 0.60})
    for (int n : {2, 3, 8}) bad += stitch_case(make_raster(R, C, density, seed++), n, "noise");
  for (int n : {2, 3, 8}) {
    /* two arms joined by a bar in the last strip, isolated cells beside them in every strip */
    bad += stitch_case(raster_from(R, C, [&](int r, int c) {
      if (c == 10 || c == 200) return 0.5 + r * 1e-3;
      if (r == R - 2 && c >= 10 && c <= 200) return 0.25;
      return (c > 250 && c % 2 == 0 && r % 2 == 0) ? 0.125 + c * 1e-4 : 0.0;
    }), n, "arms");
    /* a comb with teeth in every other column of the left half, joined only in the last strip; isolated cells after the teeth */
    bad += stitch_case(raster_from(R, C, [&](int r, int c) {
      if (c < 250) return (c % 2 == 0 || r == R - 1) ? 0.002 + (r * C + c) * 1e-6 : 0.0;
      return (c > 251 && c % 2 == 0 && r % 2 == 0) ? 0.5 : 0.0;
    }), n, "comb");
    /* the mirror image: the bar in the first strip */
    bad += stitch_case(raster_from(R, C, [&](int r, int c) {
      if (c < 250) return (c % 2 == 0 || r == 0) ? 0.002 + (r * C + c) * 1e-6 : 0.0;
      return (c > 251 && c % 2 == 0 && r % 2 == 0) ? 0.5 : 0.0;
    }), n, "comb mirrored");
    /* the serpentine, transposed: one pond that crosses every boundary many times */
    bad += stitch_case(raster_from(R, C, [&](int r, int c) {
      const bool wet = c % 2 == 0 || (c % 4 == 1 && r == R - 1) || (c % 4 == 3 && r == 0);
      return wet ? 0.002 + (r * C + c) * 1e-5 : 0.0;
    }), n, "serpentine transposed");
  }
  printf("stitch: total mismatches %lld\n", bad);
  return bad != 0;
}

/* ---- the kernels per strip ----------------------------------------------------------------------------------------------- */
static int kernels_main(int argc, char **argv) {
  if (argc < 7) return 2;
  const Raster whole = make_raster(atoi(argv[2]), atoi(argv[3]), atof(argv[5]), atoi(argv[6]));
  const int n = atoi(argv[4]), forced_rpw = argc > 7 ? atoi(argv[7]) : 0;
  emu_init();
  const std::vector<Strip> strips = cut(whole, n);
  const int ncp = whole.g.ncp;
  std::vector<LabelRun> run(n);
  std::vector<std::vector<int>> seam(n);
  std::vector<wdpm_stitch::RankSeams> seams(n);

  /* every strip up to its scan and its seam rows: what wdpm_group_ponds_label queues first */
  for (int k = 0; k < n; k++) {
    const Geom g = strips[k].a.g;
    LabelRun &s = run[k];
    label_scan(strips[k].a, s);
    seam[k].assign((size_t)2 * ncp, -1);
    launch(blocks_for(2 * g.nsc, kWaves), [&] {
      ponds_seam_kernel(s.masks.data(), s.parent.data(), s.cnt.data(), s.rootmask.data(), g, seam[k].data());
    });
    seams[k].n = s.st.ponds;
    seams[k].top = seam[k].data();
    seams[k].bottom = seam[k].data() + ncp;
  }
  wdpm_stitch::Result res;
  std::string err;
  if (wdpm_stitch::stitch(seams, ncp, res, err)) { printf("kernels: %s\n", err.c_str()); return 1; }

  /* every strip's table kernel with its map: whole-raster numbers into the label raster, local rows in the table */
  std::vector<std::vector<int>> labels(n);
  std::vector<std::vector<PondRow>> tables(n);
  for (int k = 0; k < n; k++) {
    const std::vector<int> map = res.map[k];      /* a copy: exactly st.ponds entries */
    label_table(strips[k].a, run[k], forced_rpw, map.data());
    labels[k] = run[k].labels;
    tables[k] = run[k].table;
  }
  return compare(whole, strips, labels, tables, res, false, "kernels") != 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "stitch")) return stitch_main();
  if (argc >= 7 && !strcmp(argv[1], "kernels")) return kernels_main(argc, argv);
  fprintf(stderr, "usage: %s stitch | kernels ROWS COLS STRIPS DENSITY SEED [ROWS_PER_WAVE]\n", argv[0]);
  return 2;
}
