/*
 * wdpm_small.hip — the launches of small and mid-size rasters: the triangle kernel (tri_iteration_kernel), the relay kernel
 * (relay_iteration_kernel) and wdpm_launch_small, which wdpm_launch_iteration (wdpm_march.hip) hands their plans to.  The
 * trapezoid, the lane layout and the per-block arithmetic they share with the marching kernel: wdpm_iteration.h.
 *
 * A translation unit of its own, because the two want different
 * instruction schedulers: the marching kernel is 2 % faster under the compiler's max-ILP strategy (-mllvm -amdgpu-sched-strategy=max-ilp:
 * add 16384^2 1.1425 -> 1.1189 ms), the eight-wave relay instantiations 2.4 % slower (profiles/r03/sched_strategy_ab.txt).
 * This unit is built under the default one.
 */
#include "wdpm_iteration.h"

namespace {

#ifdef WDPM_WAVE_TIMES   /* timing builds only (tools/relay_times.py) */
static __device__ unsigned long long g_wave_times[4 * 8192];   /* this unit's own (wdpm_march.hip has one for the marching kernel): each has its accessor */
/* relay kernel: eight stamps per wave (tools/relay_times.py); the wait in front of each makes the stamp mean "everything before is done" */
#define WDPM_RSTAMP(k) do { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0); rst[k] = wall_clock64(); __builtin_amdgcn_s_waitcnt(0); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define WDPM_RSTAMP(k) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// Small rasters: the "triangle" kernel.
//
// A raster of a few hundred rows cannot fill the chip, and the marching kernel (wdpm_march.hip) then runs at its
// latency floor: every wave needs H/3 + 2 window steps of nine DEPENDENT 3x3 blocks each (one lane works
// on one block at a time), about 10 us per launch on a 482 x 471 raster however many SIMDs idle.  Here a
// wave takes NINE rows at once and produces the three middle ones in one go:
//       oi = 1 on rows 0-2, 3-5, 6-8      three independent row blocks ...
//       oi = 2 on rows 1-3, 4-6           ... two ...
//       oi = 3 on rows 2-4                ... one: rows 2-4 have then seen all nine passes
// Six stages instead of the marching kernel's nine for a 3-row chunk, and the row blocks of a stage are
// advanced in LOCKSTEP - neighbour step k of block a, of block b, of block c, then step k+1 ... - so the
// fp64 pipeline sees up to three independent dependency chains instead of one.
// Same trapezoid, same pass order per cell, same arithmetic (stage_impl's blocks): bit-identical.
// ---------------------------------------------------------------------------------------------
/* NB independent 3x3 blocks of one colour pass, advanced in lockstep (non-outlet form; block b is
 * w[b][row][col] with the centre at [1][1], neighbours in row-major order) */
template <int MODULE, int NB, int FLAGS = 0>   /* FLAGS as block_update's: bit 0 PLAIN, bit 1 CLAMP */
__device__ __forceinline__ void blocks_lockstep(double (&w)[NB][3][3], const double (&d)[NB][3][3]) {
  constexpr bool PLAIN = (FLAGS & 1) != 0, CL = (FLAGS & 2) != 0;
  double wc[NB], dce[NB];
  bool gate[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    wc[b] = w[b][1][1];
    gate[b] = PLAIN || ((wc[b] > 0.0) & (d[b][1][1] < WDPM_INF));  // WDPMCL.c:1099 (PLAIN: see block_update)
    dce[b] = gate[b] ? d[b][1][1] : -WDPM_INF;                      // see flow_add_nz / flow_drain_nz
    if (MODULE == 2) wc[b] = gate[b] ? wc[b] : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int r = 1 + nb_dr(k), c = 1 + nb_dc(k);
#pragma unroll
    for (int b = 0; b < NB; b++) {
      if (MODULE == 2) flow_drain_nz<CL>(dce[b], wc[b], d[b][r][c], w[b][r][c]);
      else flow_add_nz<CL>(dce[b], wc[b], d[b][r][c], w[b][r][c]);
    }
  }
#pragma unroll
  for (int b = 0; b < NB; b++) w[b][1][1] = MODULE == 2 ? (gate[b] ? wc[b] : w[b][1][1]) : wc[b];
}

/* one row alignment (three column alignments oj = 1,2,3) on the NB row blocks at window slots
 * S0 + 3b .. S0 + 3b + 2 of a window of NR rows; the lockstep twin of stage_impl */
template <int MODULE, int NB, int S0, int NR, int FLAGS = 0>
__device__ __forceinline__ void stage_lockstep(double (&W)[NR][3], const double (&D)[NR][3]) {
  double w[NB][3][3], d[NB][3][3];
  double n0[NB][3], n1[NB][3], e0[NB][3], e1[NB][3];      // columns 0 and 1 of the next lane: water, elevation
  // oj = 1: own columns 0,1,2
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) { w[b][r][c] = W[S0 + 3 * b + r][c]; d[b][r][c] = D[S0 + 3 * b + r][c]; }
  blocks_lockstep<MODULE, NB, FLAGS>(w, d);
  // oj = 2: own columns 1,2 + column 0 of the next lane
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      n0[b][r] = lane_next(w[b][r][0]);
      e0[b][r] = lane_next(d[b][r][0]);
      W[S0 + 3 * b + r][0] = w[b][r][0];                  // column 0 is done for this row alignment (until handed back)
      w[b][r][0] = w[b][r][1]; w[b][r][1] = w[b][r][2]; w[b][r][2] = n0[b][r];
      d[b][r][0] = d[b][r][1]; d[b][r][1] = d[b][r][2]; d[b][r][2] = e0[b][r];
    }
  blocks_lockstep<MODULE, NB, FLAGS>(w, d);
  // oj = 3: own column 2 + columns 0,1 of the next lane
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      n1[b][r] = lane_next(W[S0 + 3 * b + r][1] = w[b][r][0]);   // own column 1 as updated by oj = 1,2 ...
      e1[b][r] = lane_next(D[S0 + 3 * b + r][1]);                // ... the next lane's is the one we borrow
      w[b][r][0] = w[b][r][1]; w[b][r][1] = w[b][r][2]; w[b][r][2] = n1[b][r];
      d[b][r][0] = d[b][r][1]; d[b][r][1] = d[b][r][2]; d[b][r][2] = e1[b][r];
    }
  blocks_lockstep<MODULE, NB, FLAGS>(w, d);
  // own column 2 back into the window; the borrowed columns back to lane+1 (lane 0 keeps its own)
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      W[S0 + 3 * b + r][2] = w[b][r][0];
      W[S0 + 3 * b + r][0] = lane_prev(w[b][r][1], W[S0 + 3 * b + r][0]);
      W[S0 + 3 * b + r][1] = lane_prev(w[b][r][2], W[S0 + 3 * b + r][1]);
    }
}

template <int MODULE, bool FLUSH, int K = 1, bool PLAIN = false, bool MD = false>
__global__ void __launch_bounds__(256, 2)
tri_iteration_kernel(const double *__restrict__ win, double *__restrict__ wout, const double *__restrict__ dem,
                     const SlabGeom g, const int nstrips, const int nitems, const int A0, const int out_last,
                     double *__restrict__ totaldrain, const double thres, const int drain_owed, const MaxDiffArgs md) {
  static_assert(!MD || (K == 1 && MODULE != 2), "the max-diff variant exists for three rows per wave, add / subtract");
  // K row blocks out per wave: 3K + 6 rows in, oi = 1 on K + 2 row blocks, oi = 2 on K + 1, oi = 3 on K.  K = 1 is the kernel
  // described above; K = 2 (add / subtract only) does 9 block stages for six rows instead of 12 - for rasters whose waves no
  // longer fit on the chip in one round, where the launch is bound by instruction issue, not by a single wave's latency.
  static_assert(K == 1 || MODULE != 2, "the outlet's permutation below is written for K = 1");
  constexpr int NR = 3 * K + 6;
  const int lane = threadIdx.x & 63;
  const int vb = (blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;       // XCD-contiguous items
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int item = vb * 4 + wave;
  if (item >= nitems) return;                                               // wave-uniform
  const int strip = item % nstrips, chunk = item / nstrips;
  const int c0 = kStripOut * strip;
  const int oc_lo = strip == 0 ? 0 : c0 + kHaloL;
  int oc_hi = c0 + kStripIn - 1 - kHaloR;
  if (oc_hi > g.ncp - 1) oc_hi = g.ncp - 1;
  const int A = A0 + 3 * K * chunk;               // window rows A .. A+NR-1; exact output rows A+2 .. A+3K+1
  const int or_lo = A == 0 ? 0 : A + 2;
  int or_hi = A + 3 * K + 1;
  if (or_hi > out_last) or_hi = out_last;
  const int colb = c0 + 3 * lane;
  const size_t pitch = (size_t)g.ncp;

  DrainState ds;
  ds.td = MODULE == 2 ? *totaldrain : 0.0;
  ds.hit = false;
  bool owner = false;
  const bool outlet_inside = g.dr >= 1 && g.dr <= g.rows - 2 && g.dc >= 1 && g.dc <= g.ncp - 2;
  if (MODULE == 2) {
    owner = g.dr >= or_lo && g.dr <= or_hi && g.dc >= oc_lo && g.dc <= oc_hi;
    if (drain_owed && owner && outlet_inside) ds.td = ds.td + owed_drain_sum(win, dem, g);   // the previous iteration's drain(), see above
  }

  // nine rows x three columns per lane; cells outside the slab: dem = +inf, water = 0.  Row bases are
  // wave-uniform (scalar registers), the lane contributes a 32-bit byte offset: saddr-form loads, no 64-bit
  // address arithmetic on the vector unit.  Only waves at the slab's right / lower edge mask anything.
  const bool edge = (c0 + kStripIn > g.ncp) || (A + NR > g.rows);                  // wave-uniform
  unsigned voff[3];
#pragma unroll
  for (int j = 0; j < 3; j++) voff[j] = 8u * (unsigned)(colb + j < g.ncp ? colb + j : g.ncp - 1);
  double W[NR][3], D[NR][3];
#pragma unroll
  for (int i = 0; i < NR; i++) {
    const int rc = A + i < g.rows ? A + i : g.rows - 1;
    const char *bw = reinterpret_cast<const char *>(win + (size_t)rc * pitch);
    const char *bd = reinterpret_cast<const char *>(dem + (size_t)rc * pitch);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      W[i][j] = *reinterpret_cast<const double *>(bw + voff[j]);
      D[i][j] = *reinterpret_cast<const double *>(bd + voff[j]);
    }
  }
  // MD (round 3): the block's last launch of a small raster stays with this kernel - the snapshot's rows behind the rows this
  // wave will store, requested with the window (the snapshot may still be owed the block's flush: applied as it is compared)
  double O[3 * K + 2][3];
  if (MD) {
#pragma unroll
    for (int i = 0; i < 3 * K + 2; i++) {
      const int rc = A + i < g.rows ? A + i : g.rows - 1;
      const char *bo = reinterpret_cast<const char *>(md.old + (size_t)rc * pitch);
#pragma unroll
      for (int j = 0; j < 3; j++) O[i][j] = *reinterpret_cast<const double *>(bo + voff[j]);
    }
  }
  if (FLUSH) {
#pragma unroll
    for (int i = 0; i < NR; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) W[i][j] = W[i][j] < thres ? 0.0 : W[i][j];       // WDPMCL.c:1059-1062
  }
  if (MODULE == 2 && drain_owed && outlet_inside && A + NR - 1 >= g.dr - 1 && A <= g.dr + 1) {   // wave-uniform, rare
#pragma unroll
    for (int i = 0; i < NR; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int r = A + i, c = colb + j;
        W[i][j] = (r >= g.dr - 1 && r <= g.dr + 1 && c >= g.dc - 1 && c <= g.dc + 1) ? 0.0 : W[i][j];   // :1885-1889
      }
  }
  if (edge) {
#pragma unroll
    for (int i = 0; i < NR; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const bool ok = (A + i < g.rows) & (colb + j < g.ncp);
        W[i][j] = ok ? W[i][j] : 0.0;
        D[i][j] = ok ? D[i][j] : WDPM_INF;
      }
  }

  bool outlet_here = false;
  if constexpr (MODULE == 2) outlet_here = g.dr >= A && g.dr <= A + 8;
  if constexpr (MODULE == 2) if (outlet_here) {
    // The outlet's row is in this window (a handful of waves).  In every row alignment at most ONE row block
    // holds that row (row blocks of an alignment are disjoint, so totaldrain still accumulates in pass order):
    // it runs the marching kernel's stage with runoffd()'s sink, the other blocks of the alignment stay in
    // lockstep.  Which block it is is wave-uniform but only known at run time: the window is permuted with
    // selects so that one copy of the code serves every position.
    bool cdr[5];
#pragma unroll
    for (int j = 0; j < 5; j++) cdr[j] = colb + j == g.dc;
    const int off = g.dr - A;                                   // 0 .. 8
    auto sel = [](const bool c, const double a, const double b) { return c ? a : b; };
    double P[9][3], Q[9][3];
    {  // oi = 1: row blocks at slots 0, 3, 6; the outlet's is block ob = off / 3
      const int ob = off / 3;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          P[r][j] = sel(ob == 0, W[r][j], sel(ob == 1, W[3 + r][j], W[6 + r][j]));
          Q[r][j] = sel(ob == 0, D[r][j], sel(ob == 1, D[3 + r][j], D[6 + r][j]));
          P[3 + r][j] = sel(ob == 0, W[3 + r][j], W[r][j]);         Q[3 + r][j] = sel(ob == 0, D[3 + r][j], D[r][j]);
          P[6 + r][j] = sel(ob == 2, W[3 + r][j], W[6 + r][j]);     Q[6 + r][j] = sel(ob == 2, D[3 + r][j], D[6 + r][j]);
        }
      double Wm[7][3], Dm[7][3];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int j = 0; j < 3; j++) { Wm[r][j] = P[r][j]; Dm[r][j] = Q[r][j]; }
      stage_impl<2, false, 0, true>(Wm, Dm, A + 3 * ob, g.dr, cdr, ds);
      stage_lockstep<2, 2, 3, 9>(P, Q);
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const double o = Wm[r][j], x = P[3 + r][j], y = P[6 + r][j];   // outlet block, first other, second other
          W[r][j] = sel(ob == 0, o, x);
          W[3 + r][j] = sel(ob == 1, o, sel(ob == 0, x, y));
          W[6 + r][j] = sel(ob == 2, o, y);
        }
    }
    {  // oi = 2: row blocks at slots 1 and 4 (rows 1-3, 4-6); the outlet's row is in one of them for off = 1 .. 6
      const int ob = off >= 1 && off <= 6 ? (off - 1) / 3 : -1;
      if (ob < 0) {
        stage_lockstep<2, 2, 1, 9>(W, D);
      } else {
        double Wm[7][3], Dm[7][3], Wo[3][3], Do[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int j = 0; j < 3; j++) {
            Wm[r][j] = sel(ob == 0, W[1 + r][j], W[4 + r][j]);   Dm[r][j] = sel(ob == 0, D[1 + r][j], D[4 + r][j]);
            Wo[r][j] = sel(ob == 0, W[4 + r][j], W[1 + r][j]);   Do[r][j] = sel(ob == 0, D[4 + r][j], D[1 + r][j]);
          }
        stage_impl<2, false, 0, true>(Wm, Dm, A + 1 + 3 * ob, g.dr, cdr, ds);
        stage_lockstep<2, 1, 0, 3>(Wo, Do);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int j = 0; j < 3; j++) {
            W[1 + r][j] = sel(ob == 0, Wm[r][j], Wo[r][j]);
            W[4 + r][j] = sel(ob == 0, Wo[r][j], Wm[r][j]);
          }
      }
    }
    // oi = 3: the one row block at slot 2 (rows 2-4)
    if (off >= 2 && off <= 4) {
      double Wm[7][3], Dm[7][3];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int j = 0; j < 3; j++) { Wm[r][j] = W[2 + r][j]; Dm[r][j] = D[2 + r][j]; }
      stage_impl<2, false, 0, true>(Wm, Dm, A + 2, g.dr, cdr, ds);
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int j = 0; j < 3; j++) W[2 + r][j] = Wm[r][j];
    } else {
      stage_lockstep<2, 1, 2, 9>(W, D);
    }
  }
  if (!outlet_here) {
    // (no clamped neighbour step here - see `deep` in the marching kernel: this kernel sits at 256 VGPRs, and a second copy of
    // the stages behind a test of the window's depths made five of its instantiations spill, 8 - 164 bytes, round 4)
    constexpr int F = PLAIN ? 1 : 0;
    stage_lockstep<MODULE, K + 2, 0, NR, F>(W, D);   // oi = 1 on rows 0-2, 3-5, 6-8 (, 9-11)
    stage_lockstep<MODULE, K + 1, 1, NR, F>(W, D);   // oi = 2 on rows 1-3, 4-6 (, 7-9)
    stage_lockstep<MODULE, K, 2, NR, F>(W, D);       // oi = 3 on rows 2-4 (, 5-7)
  }

  // rows or_lo .. or_hi, columns oc_lo .. oc_hi (slots 0 and 1 only for the raster's first rows)
#pragma unroll
  for (int i = 0; i < 3 * K + 2; i++) {
    const int r = A + i;
    if (r < or_lo || r > or_hi) continue;                                    // wave-uniform
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int c = colb + j;
      if (c >= oc_lo && c <= oc_hi) __builtin_nontemporal_store(W[i][j], wout + (size_t)r * pitch + c);
    }
  }
  if (MODULE == 2 && owner && lane == 0) *totaldrain = ds.td;
  if (MD) {
    // max |w - oldw| over the cells this wave stored, of the rows asked for, with bigdem > missingvalue - plus the reference's
    // seed cell [0][0] (WDPMCL.c:1239-1254); `if (d > m)` per lane, wave maximum, one atomicMax
    double md_max = 0.0;
#pragma unroll
    for (int i = 0; i < 3 * K + 2; i++) {
      const int r = A + i;
      const bool row_in = r >= or_lo && r <= or_hi && r >= md.row_lo && r < md.row_hi;           // wave-uniform
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int c = colb + j;
        double o = O[i][j];
        o = o < md.thres ? 0.0 : o;                                                               // :1059-1062
        const double dd = __builtin_fabs(W[i][j] - o);                                            // :1241
        const bool cell = row_in & (c >= oc_lo) & (c <= oc_hi) & ((D[i][j] < WDPM_INF) | ((r == 0) & (c == 0)));
        md_max = (cell & (dd > md_max)) ? dd : md_max;
      }
    }
    fold_max_diff(md_max, md, lane);
  }
}

// ---------------------------------------------------------------------------------------------
// Smallest rasters: the "relay" kernel (round 3).  A workgroup of four waves takes twelve rows of one strip and
// produces the middle six; each wave carries ONE row block through a row alignment - a single dependent chain per lane, which
// runs at its latency, where the triangle kernel's wave issues three, two, one blocks in lockstep and is bound by instruction
// issue - and the rows two alignments share pass from wave to wave through LDS:
//       oi = 1   wave w on rows 3w .. 3w+2                      (w = 0..3)
//       row 3w+3 (wave w+1's first row) -> wave w               LDS + s_barrier
//       oi = 2   wave w on rows 3w+1 .. 3w+3                    (w = 0..2)
//       row 3w+4 (wave w+1's second row) -> wave w              LDS + s_barrier
//       oi = 3   wave w on rows 3w+2 .. 3w+4, stored            (w = 0, 1)
// Nine block stages for six rows, as in the six-row triangle wave, but three in a row per wave instead of nine.  Same trapezoid,
// same pass order per cell, same arithmetic (stage_lockstep with one block): bit-identical.
// ---------------------------------------------------------------------------------------------
template <int MODULE, bool FLUSH, bool PLAIN, int NW = 4, bool DEM32 = false>
__global__ void __launch_bounds__(64 * NW, 2)
relay_iteration_kernel(const double *__restrict__ win, double *__restrict__ wout, const double *__restrict__ dem,
                       const SlabGeom g, const int nstrips, const int nwg, const int A0, const int out_last, const double thres,
                       double *__restrict__ totaldrain, const int drain_owed, const DemCode code, const int store_plain) {
  static_assert(!DEM32 || (MODULE != 2 && NW == 8), "the DEM as 32-bit codes: add / subtract launches of several rounds");
  const int lane = threadIdx.x & 63;
  const int vb = (blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;       // XCD-contiguous workgroups
  if (vb >= nwg) return;                                                    // workgroup-uniform: nobody is left at a barrier
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int strip = vb % nstrips, chunk = vb / nstrips;
  const int c0 = kStripOut * strip;
  const int oc_lo = strip == 0 ? 0 : c0 + kHaloL;
  int oc_hi = c0 + kStripIn - 1 - kHaloR;
  if (oc_hi > g.ncp - 1) oc_hi = g.ncp - 1;
  // NW waves: rows A .. A + 3 NW - 1 in, the middle 3 (NW - 2) out (NW = 4: twelve in, six out; NW = 8: 24 in, 18 out - fewer
  // waves and less re-reading per row where the waves no longer fit on the chip at once)
  constexpr int kOut = 3 * (NW - 2);
  const int A = A0 + kOut * chunk;                // exact output rows A+2 .. A+kOut+1
  const int or_lo = A == 0 ? 0 : A + 2;
  int or_hi = A + kOut + 1;
  if (or_hi > out_last) or_hi = out_last;
  const int R0 = A + 3 * wave;                    // this wave's rows R0 .. R0+2, later up to R0+4
  const int colb = c0 + 3 * lane;
  const size_t pitch = (size_t)g.ncp;
#ifdef WDPM_WAVE_TIMES
  unsigned long long rst[8];
  rst[0] = wall_clock64();
#endif
  const bool rprio = (store_plain & 2) != 0;      // wave-uniform: see the stages
  if (rprio) __builtin_amdgcn_s_setprio(3);       // the loads of a new workgroup go out ahead of an older one's arithmetic
  unsigned voff[3];
#pragma unroll
  for (int j = 0; j < 3; j++) voff[j] = 8u * (unsigned)(colb + j < g.ncp ? colb + j : g.ncp - 1);
  double W[7][3], D[7][3];                        // slots 0 .. 4 are used (seven: stage_impl's window type)
  // Every wave fetches its own three rows of water and of elevations.  The elevations of the two rows it takes over later are
  // static data the wave below holds anyway: they come with the water through LDS (LDSDEM) where the launch is more than a
  // round of waves - five rows of DEM fetched per wave made those memory-bound (add 2000^2 32.9 -> 30.0 us, 3000^2 66.7 -> 63.0,
  // drain 1200^2 15.0 -> 14.3) - and for drain; add / subtract workgroups of four waves, the one-round sizes, fetch all five
  // themselves: there the extra LDS traffic sits on the latency path (482^2 5.23 against 5.38 us; profiles/r03/relay_ldsdem_ab.txt)
  constexpr bool LDSDEM = NW == 8 || MODULE == 2;
#pragma unroll
  for (int i = 0; i < (LDSDEM ? 3 : 5); i++) {
    const int rc = R0 + i < g.rows ? R0 + i : g.rows - 1;
    const char *bw = reinterpret_cast<const char *>(win + (size_t)rc * pitch);
    const char *bd = reinterpret_cast<const char *>(dem + (size_t)rc * pitch);
    const char *bq = reinterpret_cast<const char *>(code.q + (size_t)rc * pitch);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      // DEM32: the elevations as verified-lossless 32-bit codes (wdpm_kernels.h::DemCode): launches of several rounds are bound
      // by the memory system, and four bytes per cell less are worth nine decodes per wave there
      if (DEM32) D[i][j] = dem32_decode_nan(*reinterpret_cast<const int *>(bq + voff[j] / 2), code.k0, code.D, code.rD, code.rDlo);
      else D[i][j] = *reinterpret_cast<const double *>(bd + voff[j]);
      W[i][j] = i < 3 ? *reinterpret_cast<const double *>(bw + voff[j]) : 0.0;
    }
  }
#pragma unroll
  for (int i = (LDSDEM ? 3 : 5); i < 7; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { W[i][j] = 0.0; D[i][j] = WDPM_INF; }

  // Drain: totaldrain is carried from row alignment to row alignment by whichever wave holds the outlet's block (at most one
  // per alignment and workgroup: wave-uniform arithmetic every wave can do), through LDS; the workgroup whose stored block
  // holds the outlet has seen every pass that touches it, in the reference's order, and writes it back.
  DrainState ds;
  ds.td = 0.0;
  ds.hit = false;
  bool owner = false;
  int wo[3] = {-1, -1, -1};                       // wave that holds the outlet's row in its block of alignment oi = 1, 2, 3
  bool cdr[5];
#pragma unroll
  for (int j = 0; j < 5; j++) cdr[j] = MODULE == 2 && colb + j == g.dc;
  if (MODULE == 2) {
    const bool outlet_inside = g.dr >= 1 && g.dr <= g.rows - 2 && g.dc >= 1 && g.dc <= g.ncp - 2;
    const bool col_here = g.dc >= c0 && g.dc <= c0 + kStripIn + 1;      // the strip and the two columns lane 63 borrows
#pragma unroll
    for (int st = 0; st < 3; st++) {
      const int rel = g.dr - A - st;              // alignment st + 1: wave w on rows A + 3w + st .. + 2
      if (col_here && rel >= 0 && rel / 3 <= NW - 1 - st) wo[st] = rel / 3;
    }
    owner = g.dr >= or_lo && g.dr <= or_hi && g.dc >= oc_lo && g.dc <= oc_hi;
    ds.td = *totaldrain;
    if (drain_owed && outlet_inside) {
      // the previous iteration's drain() (see fused_iteration_kernel): every wave of the owning workgroup adds it up for itself
      if (owner) ds.td = ds.td + owed_drain_sum(win, dem, g);
      if (R0 + 2 >= g.dr - 1 && R0 <= g.dr + 1) {                                   // wave-uniform, rare
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) {
            const int r = R0 + i, c = colb + j;
            W[i][j] = (r >= g.dr - 1 && r <= g.dr + 1 && c >= g.dc - 1 && c <= g.dc + 1) ? 0.0 : W[i][j];   // :1885-1889
          }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < (LDSDEM ? 3 : 5); i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      if (FLUSH && i < 3) W[i][j] = W[i][j] < thres ? 0.0 : W[i][j];               // WDPMCL.c:1059-1062
      const bool ok = (R0 + i < g.rows) & (colb + j < g.ncp);                      // outside the slab: dem = +inf, water = 0
      W[i][j] = ok ? W[i][j] : 0.0;
      D[i][j] = ok ? D[i][j] : WDPM_INF;
    }
  __shared__ double xch[2][NW][3 * kLanes];
  __shared__ double xdem[2][LDSDEM ? NW : 1][LDSDEM ? 3 * kLanes : 1];   // elevations of a wave's first two rows, for the wave above
  __shared__ double td_sh[3];
  __shared__ int deep_sh[NW];
  // The clamped neighbour step where the depths are shallow enough for it to be exact (see `deep` in the marching kernel: the same
  // bound).  A wave tests the three rows it loaded: enough for the first alignment, which stays inside them; the rows it takes
  // over afterwards have been through other waves' blocks, so from the first barrier on the workgroup's OR decides.  Wave-uniform.
  bool deep = (store_plain & 4) != 0;              // the host's part: elevations too large (WDPM_LAUNCH_CLAMP_OK not given)
  deep = deep || any_above_3m(&W[0]);
  if (lane == 0) deep_sh[wave] = deep ? 1 : 0;
  // one row alignment on this wave's block at slots S0 .. S0+2 (st = S0): the outlet's block takes block_update's outlet form
#define WDPM_RELAY_STAGE(S0)                                                                               \
  do {                                                                                                     \
    if (MODULE == 2 && wo[S0] == wave) {                                                                   \
      stage_impl<2, false, S0, true>(W, D, R0 + S0, g.dr, cdr, ds);                                        \
      if (lane == 0) td_sh[S0] = ds.td;                                                                    \
    } else if (MODULE == 2 || deep) {      /* drain: never clamped here - the second copy of the stages took the  */ \
      /* drain instantiations from 112 to 150 VGPRs, one eight-wave workgroup per CU instead of two: -17 % (round 4) */   \
      stage_lockstep<MODULE, 1, S0, 7, PLAIN ? 1 : 0>(W, D);                                               \
    } else {                                                                                               \
      stage_lockstep<MODULE, 1, S0, 7, (PLAIN ? 1 : 0) | 2>(W, D);                                         \
    }                                                                                                      \
  } while (0)
  // rprio (launches of a few rounds of workgroups: the host decides): a workgroup's issue priority falls from stage to stage, so that
  // of the workgroups sharing a CU's SIMDs the one behind is served first (the arbiter's own rule is oldest first: see the marching
  // loop).  profiles/r03/relay_prio_ab.txt: 1000^2 add 9.72 -> 9.11 us, drain 13.5 -> 12.0; 1200^2 and 1400^2 add +4.5 %; from five
  // rounds of workgroups on nothing or a loss (1800^2 drain -4 %, add -10 %; 2400^2 add -10 %: there the old workgroups' early exit is
  // what feeds the next round), so only launches of up to four rounds carry the flag
  if (rprio) __builtin_amdgcn_s_setprio(2);
  WDPM_RSTAMP(1);                                                             // rows loaded
  WDPM_RELAY_STAGE(0);                                                        // oi = 1
  WDPM_RSTAMP(2);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    xch[0][wave][j * kLanes + lane] = W[0][j];
    if (LDSDEM) {
      xdem[0][wave][j * kLanes + lane] = D[0][j];
      xdem[1][wave][j * kLanes + lane] = D[1][j];
    }
  }
  __syncthreads();
  WDPM_RSTAMP(3);
#pragma unroll
  for (int w = 0; w < NW; w++) deep = deep || deep_sh[w] != 0;
  if (MODULE == 2 && wo[0] >= 0) ds.td = td_sh[0];
  if (wave < NW - 1) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      W[3][j] = xch[0][wave + 1][j * kLanes + lane];
      if (LDSDEM) {
        D[3][j] = xdem[0][wave + 1][j * kLanes + lane];
        D[4][j] = xdem[1][wave + 1][j * kLanes + lane];
      }
    }
    if (rprio) __builtin_amdgcn_s_setprio(1);
    WDPM_RELAY_STAGE(1);                                                      // oi = 2
  }
  WDPM_RSTAMP(4);
#pragma unroll
  for (int j = 0; j < 3; j++) xch[1][wave][j * kLanes + lane] = W[1][j];
  __syncthreads();
  WDPM_RSTAMP(5);
#ifdef WDPM_WAVE_TIMES
  if (wave >= NW - 2 && lane == 0) {
    const int wid = ((int)blockIdx.x * NW + wave);
    if (wid < 4096) { for (int k = 0; k < 6; k++) g_wave_times[8 * wid + k] = rst[k]; g_wave_times[8 * wid + 6] = rst[5]; g_wave_times[8 * wid + 7] = rst[5]; }
  }
#endif
  if (wave >= NW - 2) return;
  if (MODULE == 2 && wo[1] >= 0) ds.td = td_sh[1];
#pragma unroll
  for (int j = 0; j < 3; j++) W[4][j] = xch[1][wave + 1][j * kLanes + lane];
  if (rprio) __builtin_amdgcn_s_setprio(0);
  WDPM_RELAY_STAGE(2);                                                        // oi = 3
  WDPM_RSTAMP(6);
#undef WDPM_RELAY_STAGE
  // wave w stores rows A+3w+2 .. A+3w+4 (wave 0 also rows 0, 1 of the raster's first chunk)
  if (LDSDEM) {
    // Through the wave's LDS slices (free since the second barrier), so that one store instruction writes 512 contiguous
    // bytes - as the marching kernel does.  Lane by lane a wave's three stores per row interleave at 24-byte strides, and as
    // non-temporal stores they reach the memory as partial lines: 52 MB written per 2000^2 launch for 32 MB of raster
    // (profiles/r03/add2000_pmc_summary.json; add 2000^2 28.9 -> 26.1 us, 3000^2 58.2 -> 50.8, relay_stores_ab.txt).  Lanes past
    // the exact output range are clamped onto its last column.  store_plain bit 0: ordinary instead of non-temporal stores (the
    // host sets it for launches of six rounds and more: relay_stores_ab.txt).
    double *const t[3] = {&xdem[0][wave][0], &xdem[1][wave][0], &xch[0][wave][0]};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) t[i][3 * lane + j] = W[2 + i][j];
    __builtin_amdgcn_wave_barrier();
    const int lo = oc_lo - c0, hi = oc_hi - c0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const int r = R0 + 2 + i;
      if (r < or_lo || r > or_hi) continue;                                         // wave-uniform
#pragma unroll
      for (int kk = 0; kk < 3; kk++) {
        const int c = lo + 64 * kk + lane < hi ? lo + 64 * kk + lane : hi;
        double *const q = wout + (size_t)r * pitch + c0 + c;
        if (store_plain & 1) *q = t[i][c];
        else __builtin_nontemporal_store(t[i][c], q);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < (LDSDEM ? 2 : 5); i++) {
    const int r = R0 + i;
    if (r < or_lo || r > or_hi || (i < 2 && !(wave == 0 && A == 0))) continue;    // wave-uniform
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int c = colb + j;
      if (c >= oc_lo && c <= oc_hi) __builtin_nontemporal_store(W[i][j], wout + (size_t)r * pitch + c);
    }
  }
  // the wave that ran the last alignment's outlet block holds the final value; if that alignment had none here, wave 0 does
  if (MODULE == 2 && owner && lane == 0 && wave == (wo[2] >= 0 ? wo[2] : 0)) *totaldrain = ds.td;
#ifdef WDPM_WAVE_TIMES
  WDPM_RSTAMP(7);
  if (lane == 0) {
    const int wid = ((int)blockIdx.x * NW + wave);
    if (wid < 4096) for (int k = 0; k < 8; k++) g_wave_times[8 * wid + k] = rst[k];
  }
#endif
}

}  // namespace

using RelayFn = decltype(&relay_iteration_kernel<0, false, false, 4, false>);
using TriangleFn = decltype(&tri_iteration_kernel<0, false, 1, false, false>);
#define WDPM_ROW_RELAY(...) WDPM_VARIANT_ROW(relay_iteration_kernel, __VA_ARGS__)
#define WDPM_ROW_TRIANGLE(...) WDPM_VARIANT_ROW(tri_iteration_kernel, __VA_ARGS__)
static const VariantRow<RelayFn> kRelayTable[] = {WDPM_VARIANTS_RELAY(WDPM_ROW_RELAY)};
static const VariantRow<TriangleFn> kTriangleTable[] = {WDPM_VARIANTS_TRIANGLE(WDPM_ROW_TRIANGLE)};

/* this unit's part of DeviceFacts (cus is filled already) */
void wdpm_small_device_facts(DeviceFacts *f) {
  int blocks = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, tri_iteration_kernel<0, false, 1, false, false>, 256, 0) != hipSuccess || blocks < 1) blocks = 1;
  f->tri_slots = f->cus * blocks * 4;
}

hipError_t wdpm_launch_small(const LaunchRequest &q, const LaunchPlan &p, const IterationBuffers &b) {
  const int drain_owed = q.module == 2 ? b.drain_owed : 0;
  if (p.family == WDPM_FAMILY_RELAY) {
    const int at = wdpm_find_variant(kRelayVariants, p.targs);
    if (at < 0) return hipErrorInvalidValue;
    wdpm_ledger_count(*kRelayTable[at].slot, p.ledger_sw);
    hipLaunchKernelGGL(kRelayTable[at].fn, dim3(p.grid), dim3(p.block), 0, b.stream, b.w_in, b.w_out, b.dem, q.g, p.nstrips, p.nitems, q.A0,
                       q.out_last, b.thres, b.totaldrain, drain_owed, *b.code, p.relay_flags);
  } else {
    const int at = wdpm_find_variant(kTriangleVariants, p.targs);
    if (at < 0) return hipErrorInvalidValue;
    const MaxDiffArgs tmd = p.fold_md ? *b.md : MaxDiffArgs{nullptr, 0.0, 0, 0, nullptr};
    wdpm_ledger_count(*kTriangleTable[at].slot, p.ledger_sw);
    hipLaunchKernelGGL(kTriangleTable[at].fn, dim3(p.grid), dim3(p.block), 0, b.stream, b.w_in, b.w_out, b.dem, q.g, p.nstrips, p.nitems, q.A0,
                       q.out_last, b.totaldrain, b.thres, drain_owed, tmd);
  }
  return hipGetLastError();
}

#ifdef WDPM_WAVE_TIMES
extern "C" int wdpm_debug_relay_times(unsigned long long *out, int nwaves) {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), (size_t)nwaves * 32) != hipSuccess;
}
#endif
