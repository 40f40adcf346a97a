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

/* ---- stand-ins for the HIP device language (those of tests/rims_emu_main.cpp, and the relaxed store of a link) ----------- */
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

static inline int __clzll(long long v) { return __builtin_clzll((unsigned long long)v); }
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
#include "../wdpm_amd/csrc/wdpm_pond_catchments.hip"

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

static Raster blank(int R, int C, int seed) {
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
  return a;
}

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
  for (int i = 0; i < 4; i++) pthread_barrier_init(&wave_bar[i], nullptr, 64);
  pthread_barrier_init(&block_bar, nullptr, 256);

  const Geom g = a.g;
  std::vector<int> labels;
  int n = 0;
  flood_fill(a, labels, n);
  std::vector<unsigned long long> masks((size_t)g.nseg, 0ull);         /* exact sizes: the sanitizer sees a stray index */
  std::vector<PondRow> ponds((size_t)n);
  for (auto &p : ponds) { p.row_min = p.col_min = INT_MAX; p.row_max = p.col_max = -1; }
  long long pond_cells = 0, levelled = 0;
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++) {
      levelled += a.dem[a.at(r, c)] < INFINITY;
      const int L = labels[a.at(r, c)];
      if (!L) continue;
      pond_cells++;
      masks[(size_t)r * g.nsc + c / 64] |= 1ull << (c % 64);
      PondRow &p = ponds[(size_t)L - 1];
      p.row_min = std::min(p.row_min, r); p.row_max = std::max(p.row_max, r);
      p.col_min = std::min(p.col_min, c); p.col_max = std::max(p.col_max, c);
    }

  const int cells = g.rows * g.ncp;
  std::vector<int> link((size_t)cells, 12345678);
  std::vector<CatchRow> table((size_t)n);
  CatchStatus st;
  memset(&st, 0, sizeof st);
  const int rpw = ponds_rows_per_wave(g.nseg, g.rows, forced_rpw);
  const int nwaves = ((g.rows + rpw - 1) / rpw) * g.nsc;
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
