/* Stand-ins for the HIP device language, for the host emulations of the pond units (tests/*_emu_main.cpp): a unit of
 * wdpm_amd/csrc compiled with WDPM_PONDS_EMULATION after this header runs its kernels' own source as 256 host threads per block, in
 * lockstep wherever lanes talk to each other (__ballot, __shfl*: a barrier over the wave's 64 threads either side of an exchange
 * array; __syncthreads: a barrier over the block), blocks one after another, atomics as relaxed host atomics - so what races on the
 * device races here.  The programs are built with -fsanitize=address,undefined (tests/emu_build.py): an index outside a buffer is
 * found on a CPU and not on a GPU.  Include this, then the unit; call emu_init() before the first launch(). */
#ifndef WDPM_TESTS_HIP_EMU_H
#define WDPM_TESTS_HIP_EMU_H

#include <pthread.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#define WDPM_PONDS_EMULATION
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

static void emu_init() {
  for (int i = 0; i < 4; i++) pthread_barrier_init(&wave_bar[i], nullptr, 64);
  pthread_barrier_init(&block_bar, nullptr, 256);
}

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
template <class T> static T __shfl_down(T v, int d) { return exchange(v, lane_of_thread() + d); }
template <class T> static T __shfl_xor(T v, int d) { return exchange(v, lane_of_thread() ^ d); }

static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline int __clzll(long long v) { return v ? __builtin_clzll((unsigned long long)v) : 64; }   /* 64 for 0, as on the device */
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

#endif
