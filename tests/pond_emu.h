/* What the host emulations of the pond units share once tests/hip_emu.h and a unit of wdpm_amd/csrc are included: the padded
 * raster, the labels of a row-major flood fill and their wet masks, the order-preserving image of a level, the waves of a launch.
 * The cell recipes (make_raster) and the references stay with each program: they differ on purpose. */
#ifndef WDPM_TESTS_POND_EMU_H
#define WDPM_TESTS_POND_EMU_H

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

/* dry, all border and NODATA; odd seeds label at 0.001 m, even ones at 0 */
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

static double unit_random() { return rand() / (double)RAND_MAX; }

/* flood fill from every unlabelled pond cell in row-major order: numbering by first cell comes by itself */
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

/* one bit per labelled cell of a g.rows x g.ncp label raster, of exact size: the sanitizer sees a stray index */
static std::vector<unsigned long long> wet_masks(const Geom &g, const std::vector<int> &labels) {
  std::vector<unsigned long long> masks((size_t)g.nseg, 0ull);
  for (int r = 0; r < g.rows; r++)
    for (int c = 0; c < g.ncp; c++)
      if (labels[(size_t)r * g.ncp + c]) masks[(size_t)r * g.nsc + c / 64] |= 1ull << (c % 64);
  return masks;
}

static unsigned long long key_of(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

/* rows per wave as the library chooses them for g (or as forced), and the waves that then cover `rows` rows */
struct Waves { int rpw, n; };
static Waves waves_over(const Geom &g, int rows, int forced_rpw) {
  const int rpw = ponds_rows_per_wave(g.nseg, g.rows, forced_rpw);
  return {rpw, ((rows + rpw - 1) / rpw) * g.nsc};
}

#endif
