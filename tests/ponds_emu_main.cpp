/* Host emulation of the pond kernels (wdpm_amd/csrc/wdpm_ponds.hip) over tests/hip_emu.h, under the sanitizers of
 * tests/test_ponds_emulation.py: the launches of wdpm_ponds_label (tests/ponds_label_emu.h) on buffers of exact size, labels and
 * table held against a row-major flood fill.
 *
 *   ponds_emu ROWS COLS DENSITY SEED [ROWS_PER_WAVE]      (file rows and columns; odd seeds label at 0.001 m, even ones at 0)
 */
#include "ponds_label_emu.h"

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s ROWS COLS DENSITY SEED [ROWS_PER_WAVE]\n", argv[0]);
    return 2;
  }
  const Raster a = make_raster(atoi(argv[1]), atoi(argv[2]), atof(argv[3]), atoi(argv[4]));
  emu_init();
  LabelRun s;
  label_scan(a, s);
  label_table(a, s, argc > 5 ? atoi(argv[5]) : 0, nullptr);

  const long long n = s.st.ponds;
  std::vector<int> ref_labels;
  std::vector<PondRow> ref_table;
  flood_fill(a, ref_labels, ref_table);
  long long label_bad = 0, table_bad = (long long)ref_table.size() != n;
  for (size_t i = 0; i < s.labels.size(); i++) label_bad += s.labels[i] != ref_labels[i];
  for (size_t k = 0; k < ref_table.size() && k < (size_t)n; k++) table_bad += memcmp(&ref_table[k], &s.table[k], sizeof(PondRow)) != 0;
  printf("%dx%d density %.2f min_depth %.3f: N %lld (reference %zu) unions %llu seam %llu rows per wave %d  "
         "label mismatches %lld  table mismatches %lld deep %u\n",
         a.R, a.C, atof(argv[3]), a.min_depth, n, ref_table.size(), s.st.unions, s.st.seam_unions, s.rpw, label_bad, table_bad, s.st.deep);
  return label_bad || table_bad;
}
