/* Host emulation of the rim kernels (wdpm_amd/csrc/wdpm_pond_rims.hip, compiled with WDPM_PONDS_EMULATION), after the pattern of
 * tests/ponds_emu_main.cpp: the kernels' own source runs as 256 threads per block, in lockstep wherever lanes talk to each other,
 * blocks one after another, atomics as host atomics.  Built with -fsanitize=address,undefined by
 * tests/test_pond_rims_emulation.py: a halo lane that reads outside a raster (column 0 / ncp - 1, row 0 / rows - 1, the cells
 * beside a segment) is found here, on a CPU.  Labels and wet masks come from a row-major flood fill, every buffer has its exact
 * size, and the rim table is held against a plain loop over the cells and their eight neighbours.
 *
 *   rims_emu ROWS COLS DENSITY SEED [ROWS_PER_WAVE]      (file rows and columns; odd seeds label at 0.001 m, even ones at 0)
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

/* ---- stand-ins for the HIP device language (those of tests/ponds_emu_main.cpp, and __shfl_down) -------------------------- */
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
#define __HIP_MEMORY_SCOPE_AGENT 0

struct Dim { unsigned x; };
static thread_local Dim threadIdx, blockIdx;
static pthread_barrier_t wave_bar[4], block_bar;
static unsigned long long slots[4][64];          /* what the lanes of a wave show each other */

static inline int wave_of_thread() { return threadIdx.x >> 6; }
static inline int lane_of_thread() { return threadIdx.x & 63; }
static void wave_sync() { pthread_barrier_wait(&wave_bar[wave_of_thread()]); }

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
template <class T> static T __shfl_down(T v, int d) { return exchange(v, lane_of_thread() + d); }
template <class T> static T __shfl_xor(T v, int d) { return exchange(v, lane_of_thread() ^ d); }

static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline long long __double_as_longlong(double d) { long long r; memcpy(&r, &d, 8); return r; }
static inline double __longlong_as_double(long long d) { double r; memcpy(&r, &d, 8); return r; }

template <class T> static T __hip_atomic_load(const T *p, int, int) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
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
#include "../wdpm_amd/csrc/wdpm_pond_rims.hip"

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
  bool inside(int r, int c) const { return r >= 0 && r < g.rows && c >= 0 && c < g.ncp; }
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

static void flood_fill(const Raster &a, std::vector<int> &labels, int &n) {
  labels.assign(a.w.size(), 0);
  n = 0;
  for (int r = 0; r < a.g.rows; r++)
    for (int c = 0; c < a.g.ncp; c++) {
      if (!a.pond_cell(r, c) || labels[a.at(r, c)]) continue;
      const int label = ++n;
      std::queue<std::pair<int, int>> todo;
      todo.push({r, c});
      labels[a.at(r, c)] = label;
      while (!todo.empty()) {
        const auto [i, j] = todo.front();
        todo.pop();
        for (int di = -1; di <= 1; di++)
          for (int dj = -1; dj <= 1; dj++)
            if (a.pond_cell(i + di, j + dj) && !labels[a.at(i + di, j + dj)]) {
              labels[a.at(i + di, j + dj)] = label;
              todo.push({i + di, j + dj});
            }
      }
    }
}

static unsigned long long key_of(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
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
  for (int i = 0; i < 4; i++) pthread_barrier_init(&wave_bar[i], nullptr, 64);
  pthread_barrier_init(&block_bar, nullptr, 256);

  const Geom g = a.g;
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  std::vector<unsigned long long> masks((size_t)g.nseg, 0ull);         /* exact sizes: the sanitizer sees a stray index */
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++)
      if (labels[a.at(r, c)]) masks[(size_t)r * g.nsc + c / 64] |= 1ull << (c % 64);

  std::vector<RimRow> table((size_t)n);
  const int rpw = ponds_rows_per_wave(g.nseg, g.rows, forced_rpw);
  const int nwaves = ((g.rows + rpw - 1) / rpw) * g.nsc;
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
