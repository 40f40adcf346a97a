/* Host emulation of the three scan kernels of wdpm_amd/csrc/wdpm_ponds.hip alone, over tests/hip_emu.h, under the sanitizers of
 * tests/test_pond_scan_emulation.py.  A whole label call reaches the second trip of ponds_scan_sums_kernel (more than 256 scan
 * blocks = more than 262 144 segments) only with a raster of that many segments; the scan itself needs nothing but the counts, so
 * this program makes them up: root counts 0..32 in cnt, packed union counts (low 16 bits <= 129, high bits <= 3) in ucnt, on
 * buffers of exact size.  cnt is held against a sequential exclusive prefix sum, the status words against plain sums.
 *
 *   scan_emu NSEG SEED [zero]      ("zero": every count is 0)
 */
#include "ponds_label_emu.h"

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s NSEG SEED [zero]\n", argv[0]);
    return 2;
  }
  const int nseg = atoi(argv[1]);
  const bool zero = argc > 3 && !strcmp(argv[3], "zero");
  if (nseg < 1) {
    fprintf(stderr, "NSEG must be at least 1\n");
    return 2;
  }
  const int nb = (nseg + kScanTile - 1) / kScanTile;
  srand(atoi(argv[2]));
  std::vector<int> cnt((size_t)nseg), bsum((size_t)nb, -7);
  std::vector<unsigned> ucnt((size_t)nseg);
  std::vector<unsigned long long> busum((size_t)2 * nb, ~0ull);
  std::vector<long long> want((size_t)nseg);
  long long ponds = 0;
  unsigned long long unions = 0ull, seam = 0ull;
  for (int i = 0; i < nseg; i++) {
    cnt[i] = zero ? 0 : rand() % 33;
    const unsigned all = zero ? 0u : rand() % 130, sm = zero ? 0u : rand() % 4;
    ucnt[i] = all | (sm << 16);
    want[i] = ponds;
    ponds += cnt[i];
    unions += all;
    seam += sm;
  }
  Status st;
  memset(&st, 0, sizeof st);

  emu_init();
  launch(nb, [&] { ponds_scan_reduce_kernel(cnt.data(), ucnt.data(), nseg, bsum.data(), busum.data()); });
  launch(1, [&] { ponds_scan_sums_kernel(bsum.data(), busum.data(), nb, &st); });
  launch(nb, [&] { ponds_scan_down_kernel(cnt.data(), nseg, bsum.data()); });

  long long scan_bad = 0, first_bad = -1;
  for (int i = 0; i < nseg; i++)
    if (cnt[i] != want[i]) {
      if (!scan_bad++) first_bad = i;
    }
  const int status_bad = (st.ponds != ponds) + (st.unions != unions) + (st.seam_unions != seam);
  printf("%d segments, %d scan blocks, %d trips: ponds %lld (reference %lld) unions %llu (%llu) seam %llu (%llu)  "
         "scan mismatches %lld (first at %lld)  status mismatches %d\n",
         nseg, nb, (nb + kBlock - 1) / kBlock, st.ponds, ponds, st.unions, unions, st.seam_unions, seam, scan_bad, first_bad,
         status_bad);
  return scan_bad || status_bad;
}
