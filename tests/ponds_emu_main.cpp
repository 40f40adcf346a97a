/* Host emulation of the pond kernels (wdpm_amd/csrc/wdpm_ponds.hip, compiled with WDPM_PONDS_EMULATION): the kernels' own source
 * runs as 256 threads per block, in lockstep wherever lanes talk to each other (__ballot, __shfl*: a barrier over the wave's 64
 * threads either side of an exchange array; __syncthreads: a barrier over the block), blocks one after another, atomics as host
 * atomics - so the unions really race.  Built with -fsanitize=address,undefined by tests/test_ponds_emulation.py: an index outside a
 * buffer is found here, on a CPU, and not on a GPU.  Checks labels and table against a row-major flood fill.
 *
 *   ponds_emu ROWS COLS DENSITY SEED [ROWS_PER_WAVE]      (file rows and columns; odd seeds label at 0.001 m, even ones at 0)
 */
#include <pthread.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <thread>
#include <vector>

/* ---- stand-ins for the HIP device language ------------------------------------------------------------------------------- */
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static          /* blocks run one after another, so one copy serves */
#define __HIP_MEMORY_SCOPE_AGENT 0

struct Dim { unsigned x; };
static thread_local Dim threadIdx, blockIdx;
static pthread_barrier_t wave_bar[4], block_bar;
static unsigned long long slots[4][64];          /* what the lanes of a wave show each other */

static inline int wave_of_thread() { return threadIdx.x >> 6; }
static inline int lane_of_thread() { return threadIdx.x & 63; }
static void wave_sync() { pthread_barrier_wait(&wave_bar[wave_of_thread()]); }
static void __syncthreads() { pthread_barrier_wait(&block_bar); }

static unsigned long long __ballot(bool pred) {
  unsigned long long *slot = slots[wave_of_thread()];
  slot[lane_of_thread()] = pred;
  wave_sync();
  unsigned long long mask = 0;
  for (int i = 0; i < 64; i++) mask |= (slot[i] & 1ull) << i;
  wave_sync();
  return mask;
}

/* every lane shows its value, then takes lane src's (its own when src is no lane) */
template <class T>
static T exchange(T v, int src) {
  unsigned long long *slot = slots[wave_of_thread()];
  unsigned long long raw = 0;
  memcpy(&raw, &v, sizeof(T));
  slot[lane_of_thread()] = raw;
  wave_sync();
  T out = v;
  if (src >= 0 && src < 64) memcpy(&out, &slot[src], sizeof(T));
  wave_sync();
  return out;
}
template <class T> static T __shfl(T v, int src) { return exchange(v, src & 63); }
template <class T> static T __shfl_up(T v, int d) { return exchange(v, lane_of_thread() - d); }
template <class T> static T __shfl_xor(T v, int d) { return exchange(v, lane_of_thread() ^ d); }

static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }
static inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, 8); return r; }
static inline double __longlong_as_double(long long d) { double r; memcpy(&r, &d, 8); return r; }

template <class T> static T __hip_atomic_load(const T *p, int, int) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
template <class T> static void __hip_atomic_store(T *p, T v, int, int) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
template <class T> static T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <class T>
static T atomicMin(T *p, T v) {
  T old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
template <class T>
static T atomicMax(T *p, T v) {
  T old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old;
}
using std::max;
using std::min;

#define WDPM_PONDS_EMULATION
#include "../wdpm_amd/csrc/wdpm_ponds.hip"

/* one launch: 256 threads walk the blocks together */
template <class F>
static void launch(unsigned blocks, F kernel) {
  std::vector<std::thread> threads;
  for (unsigned t = 0; t < 256; t++)
    threads.emplace_back([=] {
      threadIdx.x = t;
      for (unsigned b = 0; b < blocks; b++) {
        blockIdx.x = b;
        kernel();
        pthread_barrier_wait(&block_bar);
      }
    });
  for (auto &t : threads) t.join();
}
static unsigned blocks_for(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

/* ---- the raster, the reference ------------------------------------------------------------------------------------------- */
struct Raster {
  int R, C;                        /* file rows and columns */
  Geom g;
  std::vector<double> w, dem;      /* padded; NODATA and the border are +inf in dem */
  double min_depth;
  size_t at(int r, int c) const { return (size_t)r * g.ncp + c; }
  bool pond_cell(int r, int c) const {
    return r >= 1 && r <= R && c >= 1 && c <= C && dem[at(r, c)] < INFINITY && w[at(r, c)] > min_depth;
  }
};

static double unit_random() { return rand() / (double)RAND_MAX; }

static Raster make_raster(int R, int C, double density, int seed) {
  Raster a;
  a.R = R;
  a.C = C;
  a.g.rows = R + 2;
  a.g.ncp = C + 2;
  a.g.nsc = (a.g.ncp + 63) / 64;
  a.g.nseg = a.g.rows * a.g.nsc;
  a.min_depth = 0.001 * (seed % 2);
  a.w.assign((size_t)a.g.rows * a.g.ncp, 0.0);
  a.dem.assign(a.w.size(), INFINITY);
  srand(seed);
  for (int r = 1; r <= R; r++)
    for (int c = 1; c <= C; c++) {
      const size_t i = a.at(r, c);
      a.dem[i] = rand() % 100 < 5 ? INFINITY : 100.0;                           /* 5 % NODATA, with water on it */
      const double u = unit_random();
      a.w[i] = unit_random() < density ? (u < 0.1 ? 3.0 + u * 40 : u * 0.02) : 0.0;
      if (rand() % 50 == 0) a.w[i] = (rand() % 1000 + 0.5) * ldexp(1.0, -24);   /* ties of rint */
      if (rand() % 200 == 0) a.w[i] = NAN;                                      /* never a pond cell */
    }
  return a;
}

/* flood fill from every unlabelled pond cell in row-major order: numbering by first cell comes by itself */
static void flood_fill(const Raster &a, std::vector<int> &labels, std::vector<PondRow> &table) {
  labels.assign(a.w.size(), 0);
  table.clear();
  for (int r = 0; r < a.g.rows; r++)
    for (int c = 0; c < a.g.ncp; c++) {
      if (!a.pond_cell(r, c) || labels[a.at(r, c)]) continue;
      PondRow p;
      p.first_row = r;
      p.first_col = c;
      p.cells = p.volume_q = 0;
      p.row_min = p.col_min = INT_MAX;
      p.row_max = p.col_max = -1;
      double deepest = -1;
      const int label = (int)table.size() + 1;
      std::queue<std::pair<int, int>> todo;
      todo.push({r, c});
      labels[a.at(r, c)] = label;
      while (!todo.empty()) {
        const auto [i, j] = todo.front();
        todo.pop();
        const double d = a.w[a.at(i, j)];
        p.cells++;
        p.volume_q += (unsigned long long)rint(d * 16777216.0);
        deepest = std::max(deepest, d);
        p.row_min = std::min(p.row_min, i);
        p.row_max = std::max(p.row_max, i);
        p.col_min = std::min(p.col_min, j);
        p.col_max = std::max(p.col_max, j);
        for (int di = -1; di <= 1; di++)
          for (int dj = -1; dj <= 1; dj++)
            if (a.pond_cell(i + di, j + dj) && !labels[a.at(i + di, j + dj)]) {
              labels[a.at(i + di, j + dj)] = label;
              todo.push({i + di, j + dj});
            }
      }
      memcpy(&p.depth_key, &deepest, 8);          /* the finished table holds the depth itself */
      table.push_back(p);
    }
}

/* ---- the launches of wdpm_ponds_label, in its order ---------------------------------------------------------------------- */
int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s ROWS COLS DENSITY SEED [ROWS_PER_WAVE]\n", argv[0]);
    return 2;
  }
  const Raster a = make_raster(atoi(argv[1]), atoi(argv[2]), atof(argv[3]), atoi(argv[4]));
  const int forced_rpw = argc > 5 ? atoi(argv[5]) : 0;
  for (int i = 0; i < 4; i++) pthread_barrier_init(&wave_bar[i], nullptr, 64);
  pthread_barrier_init(&block_bar, nullptr, 256);

  const Geom g = a.g;
  std::vector<unsigned long long> masks(g.nseg), rootmask(g.nseg);
  std::vector<int> parent(a.w.size(), -7), labels(a.w.size(), -1), cnt(g.nseg);     /* exact sizes: the sanitizer sees a stray index */
  std::vector<unsigned> ucnt(g.nseg);
  const int nb = (g.nseg + kScanTile - 1) / kScanTile;
  std::vector<int> bsum(nb);
  std::vector<unsigned long long> busum(2 * nb);
  Status st;
  memset(&st, 0, sizeof st);

  const unsigned seg_blocks = blocks_for(g.nseg, kWaves);
  launch(seg_blocks, [&] { ponds_mask_kernel(a.w.data(), a.dem.data(), g, a.min_depth, masks.data(), parent.data(), &st); });
  launch(seg_blocks, [&] { ponds_merge_kernel(masks.data(), parent.data(), g, ucnt.data()); });
  launch(seg_blocks, [&] { ponds_flatten_kernel(masks.data(), parent.data(), g, cnt.data(), rootmask.data()); });
  launch(nb, [&] { ponds_scan_reduce_kernel(cnt.data(), ucnt.data(), g.nseg, bsum.data(), busum.data()); });
  launch(1, [&] { ponds_scan_sums_kernel(bsum.data(), busum.data(), nb, &st); });
  launch(nb, [&] { ponds_scan_down_kernel(cnt.data(), g.nseg, bsum.data()); });

  const long long n = st.ponds;
  std::vector<PondRow> table(n);
  const int rpw = ponds_rows_per_wave(g.nseg, g.rows, forced_rpw);
  const int nwaves = ((g.rows + rpw - 1) / rpw) * g.nsc;
  if (n) launch(blocks_for(n, kBlock), [&] { ponds_table_init_kernel(table.data(), n); });
  launch(blocks_for(nwaves, kWaves), [&] {
    ponds_table_kernel(a.w.data(), masks.data(), parent.data(), cnt.data(), rootmask.data(), g, rpw, nwaves, labels.data(),
                       table.data());
  });
  if (n) launch(blocks_for(n, kBlock), [&] { ponds_table_finish_kernel(table.data(), n); });

  std::vector<int> ref_labels;
  std::vector<PondRow> ref_table;
  flood_fill(a, ref_labels, ref_table);
  long long label_bad = 0, table_bad = (long long)ref_table.size() != n;
  for (size_t i = 0; i < labels.size(); i++) label_bad += labels[i] != ref_labels[i];
  for (size_t k = 0; k < ref_table.size() && k < (size_t)n; k++) table_bad += memcmp(&ref_table[k], &table[k], sizeof(PondRow)) != 0;
  printf("%dx%d density %.2f min_depth %.3f: N %lld (reference %zu) unions %llu seam %llu rows per wave %d  "
         "label mismatches %lld  table mismatches %lld deep %u\n",
         a.R, a.C, atof(argv[3]), a.min_depth, n, ref_table.size(), st.unions, st.seam_unions, rpw, label_bad, table_bad, st.deep);
  return label_bad || table_bad;
}
