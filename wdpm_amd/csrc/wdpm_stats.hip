/*
 * wdpm_stats.hip — what a driver reads off a context between blocks: cell counts, the outlet, single cells, totaldrain, the
 * drain module's closing figures and the reference's sequential volume sum, exactly.  One unit of the context layer (wdpm_ctx.h).
 */
#include <cmath>
#include <vector>

#include "wdpm_ctx.h"

extern "C" {

int wdpm_count_stats(wdpm_ctx *x, int32_t row_lo, int32_t row_hi, int64_t *valid, int64_t *wet, double *maxv) {
  if (!rows_inside(x, row_lo, row_hi)) return wdpm_fail("wdpm_count_stats: bad row range");
  if (bind(x) || wdpm_apply_owed_flush(x)) return 1;
  if (!x->d_stat) HIP_TRY(hipMalloc(&x->d_stat, 4 * sizeof(unsigned long long)));
  HIP_TRY(wdpm_launch_count_stats(x->d_w[x->cur], x->d_dem, (size_t)row_lo * x->g.ncp, (size_t)row_hi * x->g.ncp, x->g.miss,
                                  x->d_stat, x->stream));
  unsigned long long v[3];
  if (read_back(x, x->d_stat, v, sizeof v)) return 1;
  if (valid) *valid = (int64_t)v[0];
  if (wet) *wet = (int64_t)v[1];
  if (maxv) *maxv = v[2] ? wdpm_dem_key_to_double(v[2]) : -__builtin_inf();
  return 0;
}

int wdpm_find_drain(wdpm_ctx *x, int32_t row_lo, int32_t row_hi, double *mindem, int32_t *row, int32_t *col) {
  if (!rows_inside(x, row_lo, row_hi) || !mindem || !row || !col) return wdpm_fail("wdpm_find_drain: bad argument");
  if (bind(x)) return 1;
  if (!x->d_stat) HIP_TRY(hipMalloc(&x->d_stat, 4 * sizeof(unsigned long long)));
  HIP_TRY(wdpm_launch_find_drain(x->d_dem, (size_t)row_lo * x->g.ncp, (size_t)row_hi * x->g.ncp, x->d_stat, x->stream));
  unsigned long long v[2];
  if (read_back(x, x->d_stat, v, sizeof v)) return 1;
  if (v[0] == ~0ull || v[1] == ~0ull) { *row = -1; *col = -1; *mindem = __builtin_inf(); return 0; }
  *mindem = wdpm_dem_key_to_double(v[0]);
  *row = (int32_t)(v[1] / x->g.ncp);
  *col = (int32_t)(v[1] % x->g.ncp);
  return 0;
}

int wdpm_get_cell(wdpm_ctx *x, int32_t row, int32_t col, double *water, double *dem) {
  if (row < 0 || row >= x->g.rows || col < 0 || col >= x->g.ncp) return wdpm_fail("wdpm_get_cell: cell outside the slab");
  if (bind(x) || wdpm_apply_owed_flush(x)) return 1;
  const size_t k = (size_t)row * x->g.ncp + col;
  HIP_TRY(hipMemcpyAsync(x->h_pin, x->d_w[x->cur] + k, sizeof(double), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipMemcpyAsync(x->h_pin + 1, x->d_dem + k, sizeof(double), hipMemcpyDeviceToHost, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  if (water) *water = x->h_pin[0];
  if (dem) *dem = x->h_pin[1] < __builtin_inf() ? x->h_pin[1] : x->g.miss;     /* the device marks NODATA as +inf */
  return 0;
}

int wdpm_set_totaldrain(wdpm_ctx *x, double v) {
  if (bind(x) || wdpm_apply_owed_drain(x)) return 1;
  x->h_pin[0] = v;
  HIP_TRY(hipMemcpyAsync(x->d_scal, x->h_pin, sizeof(double), hipMemcpyHostToDevice, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  return 0;
}

int wdpm_get_totaldrain(wdpm_ctx *x, double *v) {
  if (bind(x) || wdpm_apply_owed_drain(x)) return 1;
  return read_back(x, x->d_scal, v, sizeof *v);
}

/* WDPMCL.c:1257-1268.  final_sum is the reference's sequential row-major sum (an ordinary parallel
 * sum would round differently): wdpm_volume_partial evaluates exactly that sum on the device. */
int wdpm_drain_stats(wdpm_ctx *x, double *diffdrain, double *final_sum) {
  if (bind(x) || wdpm_apply_owed_drain(x)) return 1;
  if (diffdrain) {
    double drain[2];   /* totaldrain, olddrain */
    if (read_back(x, x->d_scal, drain, sizeof drain)) return 1;
    *diffdrain = fabs(drain[0] - drain[1]);
  }
  if (final_sum) return wdpm_volume_partial(x, 0, x->g.rows, 0.0, final_sum);
  return 0;
}

/* The reference's sequential row-major sum over the valid cells of rows [row_lo, row_hi), continued
 * from `start` - evaluated in parallel on the device, bit for bit the left-to-right fp64 sum
 * (tests/seqsum_model.py explains why that is possible and models every step below).  Only chunks
 * whose running sum comes too close to a power of two, or that hold an exact rounding tie or a
 * negative / non-finite depth, are fetched and summed term by term. */
int wdpm_volume_partial(wdpm_ctx *x, int32_t row_lo, int32_t row_hi, double start, double *sum) {
  if (!rows_inside(x, row_lo, row_hi) || !sum) return wdpm_fail("wdpm_volume_partial: bad row range");
  if (bind(x)) return 1;
  if (wdpm_apply_owed_flush(x)) return 1;
  const size_t first = (size_t)row_lo * x->g.ncp, n = (size_t)(row_hi - row_lo) * x->g.ncp;
  const size_t nchunks = (n + kSeqSumChunk - 1) / kSeqSumChunk;
  if (nchunks == 0) { *sum = start; return 0; }
  const size_t cap = x->cells / kSeqSumChunk + 2;
  if (!x->d_sum_approx) {
    HIP_TRY(hipMalloc(&x->d_sum_approx, cap * sizeof(double)));
    HIP_TRY(hipMalloc(&x->d_sum_i, cap * sizeof(long long)));
    HIP_TRY(hipMalloc(&x->d_sum_k, cap * sizeof(int)));
    HIP_TRY(hipMalloc(&x->d_sum_flag, cap * sizeof(unsigned)));
  }
  const double *w = x->d_w[x->cur] + first, *dem = x->d_dem + first;
  std::vector<double> approx(nchunks), tw, td;
  std::vector<unsigned> flag(nchunks);
  std::vector<int> kexp(nchunks);
  std::vector<long long> isum(nchunks);

  /* pass A: ordinary per-chunk sums -> which binade each chunk's running sum will live in */
  HIP_TRY(wdpm_launch_seqsum_a(w, dem, n, x->d_sum_approx, x->d_sum_flag, x->stream));
  HIP_TRY(hipMemcpyAsync(approx.data(), x->d_sum_approx, nchunks * sizeof(double), hipMemcpyDeviceToHost, x->stream));
  HIP_TRY(hipMemcpyAsync(flag.data(), x->d_sum_flag, nchunks * sizeof(unsigned), hipMemcpyDeviceToHost, x->stream));
  if (wdpm_stream_sync(x, x->stream)) return 1;
  const bool start_ok = start >= 0.0 && start < __builtin_inf();
  double prefix = start_ok ? start : 0.0;
  size_t eligible = 0;
  for (size_t c = 0; c < nchunks; c++) {
    const double lo = prefix, hi = prefix + approx[c];
    prefix = hi;
    kexp[c] = (int)0x80000000;
    if (start_ok && !flag[c] && lo > 1e-290 && hi < 1e300) {
      int e_lo, e_hi;
      (void)frexp(lo * (1.0 - 1e-6), &e_lo);
      (void)frexp(hi * (1.0 + 1e-6), &e_hi);
      if (e_lo == e_hi) { kexp[c] = e_lo - 1; eligible++; }          /* 2^k <= running sum < 2^(k+1) all through the chunk */
    }
  }
  /* pass B: exact integer sums in units of 2^(k-52) */
  if (eligible) {
    HIP_TRY(hipMemcpyAsync(x->d_sum_k, kexp.data(), nchunks * sizeof(int), hipMemcpyHostToDevice, x->stream));
    HIP_TRY(wdpm_launch_seqsum_b(w, dem, n, x->d_sum_k, x->d_sum_i, x->d_sum_flag, x->stream));
    HIP_TRY(hipMemcpyAsync(isum.data(), x->d_sum_i, nchunks * sizeof(long long), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(hipMemcpyAsync(flag.data(), x->d_sum_flag, nchunks * sizeof(unsigned), hipMemcpyDeviceToHost, x->stream));
    if (wdpm_stream_sync(x, x->stream)) return 1;
  }
  /* chain: a chunk's integer sum is used only if its assumption holds for the ACTUAL running sum */
  double s = start;
  for (size_t c = 0; c < nchunks; c++) {
    const int k = kexp[c];
    if (k != (int)0x80000000 && !flag[c] && s >= ldexp(1.0, k)) {
      const double s_new = s + ldexp((double)isum[c], k - 52);        /* exact: both are multiples of 2^(k-52) */
      if (s_new < ldexp(1.0, k + 1)) { s = s_new; continue; }
    }
    const size_t off = c * kSeqSumChunk, len = n - off < (size_t)kSeqSumChunk ? n - off : (size_t)kSeqSumChunk;
    tw.resize(len); td.resize(len);
    HIP_TRY(hipMemcpyAsync(tw.data(), w + off, len * sizeof(double), hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(hipMemcpyAsync(td.data(), dem + off, len * sizeof(double), hipMemcpyDeviceToHost, x->stream));
    if (wdpm_stream_sync(x, x->stream)) return 1;
    for (size_t i = 0; i < len; i++)
      if (td[i] < __builtin_inf()) s += tw[i];                        /* the device DEM holds +inf for NODATA */
  }
  *sum = s;
  return 0;
}

} /* extern "C" */
