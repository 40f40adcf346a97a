/* Host emulation of the spill kernels (wdpm_amd/csrc/wdpm_pond_spills.hip, compiled with WDPM_PONDS_EMULATION), after the pattern of
 * tests/curves_emu_main.cpp: the kernels' own source runs as 256 threads per block, in lockstep wherever lanes talk to each other,
 * blocks one after another, atomics as host atomics.  Built with -fsanitize=address,undefined by tests/test_pond_spills_emulation.py:
 * a lane that reads outside a table or an array is found here, on a CPU.  The unit reads no raster, so the four tables are made up
 * directly - a graph in to_basin, random cells, catchments and fill_q, pour levels and surfaces that give the flags asked for - every
 * array of N words is a vector of its own with exactly N entries, and the whole table and the counts are held against sequential
 * walks: a ring is where a walk meets its own path, a chain is filled in from its end backwards, the sums go down pond by pond.
 *
 *   spills_emu KIND N SEED FLAGS
 *     KIND   random: every pond spills into a random other pond, onto land or nowhere
 *            ring:   one ring of N ponds with N / 2 + 37 ponds in trees hanging on it, a mutual pair beside it, labels shuffled
 *            chain:  one chain of N ponds, N -> N - 1 -> ... -> 1 -> land (the ring pass lowers its minimum in every round)
 *            hub:    ponds 2..N + 1 all spill into pond 1
 *            votes:  a wave of hubs and, N times over, five waves made lane by lane for push_group's votes (make_votes), then one
 *                    pond in a wave of its own
 *     FLAGS  0: spilling at random, 1: every pond with an outlet spills, 2: none does, 3: every second one
 */
#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_pond_spills.hip"

#include <numeric>
#include <random>

/* One launch of a kernel that never meets at a block barrier: the 256 threads walk the blocks as in launch() of tests/hip_emu.h, but a
 * wave waits for nobody except its own 64 lanes (at a vote), so the four waves run different blocks at the same time, as waves of a
 * device do - and a round that returns at once costs nothing. */
template <class F>
static void launch_waves(unsigned blocks, F kernel) {
  std::vector<std::thread> threads;
  for (unsigned t = 0; t < 256; t++)
    threads.emplace_back([=] {
      threadIdx.x = t;
      for (unsigned b = 0; b < blocks; b++) {
        blockIdx.x = b;
        kernel();
      }
    });
  for (auto &t : threads) t.join();
}

struct Tables {
  std::vector<wdpm_pond> ponds;
  std::vector<wdpm_pond_rim> rims;
  std::vector<wdpm_pond_catchment> cat;
  std::vector<wdpm_pond_outlet> out;
};

/* The table for push_group, lane by lane.  Wave 0 holds the hubs: ponds 8 -> 7 -> ... -> 1 (so the lanes that share a hub share
 * the next one a round later), 9 onto land, 10 without an outlet, 11 -> 9, 12 -> 10, and 52 ponds that spill into the twelve in turn.
 * Then `times` times five waves:
 *   A  groups of 8, 7, 9 and 40 on hubs 1, 2, 3 and 9, scattered over the wave (lane l takes entry 37 l mod 64); lane 0 is one of
 *      the 8, lane 1 one of the 40, lane 2 one of the 7: two votes succeed, the third fails, the 9 are never asked
 *   B  four groups of 16 on hubs 4, 5, 11 and 12, lane l on group l mod 4: more hubs than tries
 *   C  lanes 0..13 on hubs 6 and 7 in turn, lanes 14..33 on hub 8, the last 30 on land or without an outlet: no vote succeeds
 *   D  the mirror: 20 lanes on hub 9 first, the 30 without a target, then hubs 2 and 11 in turn
 *   E  lane 0 without an outlet, lanes 1..7 on hub 4, lanes 8..16 on hub 6, the others on hub 12: a failed vote, then two that
 *      succeed
 * and at the end one pond on hub 1 in a wave of its own.  Pond 1 spills into the first of wave A's eight that spill into it: a ring
 * of two whose marked pond - lane 0 of wave A, whose target is the first put to the vote - goes through the butterfly with seven
 * other lanes. */
static std::vector<int> make_votes(int times) {
  std::vector<int> to;
  for (int k = 1; k <= 64; k++) to.push_back(k == 1 ? 0 : k <= 8 ? k - 1 : k == 9 ? 0 : k == 10 ? -1 : k == 11 ? 9 : k == 12 ? 10 : 1 + k % 12);
  for (int rep = 0; rep < times; rep++) {
    std::vector<int> sorted;
    for (int l = 0; l < 64; l++) sorted.push_back(l < 8 ? 1 : l < 15 ? 2 : l < 24 ? 3 : 9);
    for (int l = 0; l < 64; l++) to.push_back(sorted[(size_t)(37 * l % 64)]);                       /* A */
    const int four[4] = {4, 5, 11, 12};
    for (int l = 0; l < 64; l++) to.push_back(four[l % 4]);                                          /* B */
    for (int l = 0; l < 64; l++) to.push_back(l < 14 ? 6 + l % 2 : l < 34 ? 8 : -(l % 2));           /* C */
    for (int l = 0; l < 64; l++) to.push_back(l < 20 ? 9 : l < 50 ? -(l % 2) : l % 2 ? 11 : 2);      /* D */
    for (int l = 0; l < 64; l++) to.push_back(l == 0 ? -1 : l < 8 ? 4 : l < 17 ? 6 : 12);            /* E */
  }
  to.push_back(1);
  for (size_t k = 64; k < to.size(); k++)
    if (to[k] == 1) {
      to[0] = (int)k + 1;
      break;
    }
  return to;
}

static std::vector<int> make_graph(const std::string &kind, int size, std::mt19937_64 &rng) {
  std::vector<int> to;
  if (kind == "votes") return make_votes(size);
  auto below = [&](int n) { return (int)(rng() % (unsigned long long)n); };
  if (kind == "random") {
    for (int k = 1; k <= size; k++) {
      const int u = below(100);
      int j = u < 4 ? 0 : u < 8 ? -1 : 1 + below(size);
      if (j == k) j = size > 1 ? (k % size) + 1 : 0;             /* no pond spills into itself */
      to.push_back(j);
    }
  } else if (kind == "chain") {
    for (int k = 1; k <= size; k++) to.push_back(k - 1);
  } else if (kind == "hub") {
    to.push_back(0);
    for (int k = 2; k <= size + 1; k++) to.push_back(1);
  } else {                                                       /* ring */
    const int trees = size / 2 + 37, n = size + trees + 2;
    std::vector<int> plain;
    for (int k = 1; k <= size; k++) plain.push_back(k % size + 1);
    for (int k = size + 1; k <= size + trees; k++) plain.push_back(1 + below(k - 1));       /* onto the ring or onto an older tree */
    plain.push_back(n);
    plain.push_back(n - 1);                                      /* the pair */
    std::vector<int> name(n);
    std::iota(name.begin(), name.end(), 1);
    std::shuffle(name.begin(), name.end(), rng);
    to.assign(n, 0);
    for (int k = 1; k <= n; k++) to[name[k - 1] - 1] = name[plain[k - 1] - 1];
  }
  return to;
}

static Tables make_tables(const std::vector<int> &to, int flags, std::mt19937_64 &rng) {
  const size_t n = to.size();
  Tables t;
  t.ponds.assign(n, wdpm_pond());
  t.rims.assign(n, wdpm_pond_rim());
  t.cat.assign(n, wdpm_pond_catchment());
  t.out.assign(n, wdpm_pond_outlet());
  for (size_t k = 0; k < n; k++) {
    t.ponds[k].cells = 1 + (long long)(rng() % 5000);
    t.cat[k].catch_cells = (long long)(rng() % 100000);
    t.out[k].to_basin = to[k];
    t.out[k].fill_q = to[k] >= 0 ? rng() % (1ull << 40) : 0ull;
    t.out[k].pour_level = to[k] >= 0 ? 500.0 + (double)(rng() % 1000) / 8.0 : INFINITY;
    const bool want = flags == 1 || (flags == 0 && rng() % 2) || (flags == 3 && k % 2);
    /* within the tolerance of 2^-10 m: at the level, above it, or half the tolerance below; beyond it: the next double, or 1 m */
    const double pour = to[k] >= 0 ? t.out[k].pour_level : 400.0;
    const double tol = 1.0 / 1024;
    const int how = (int)(rng() % 3);
    t.rims[k].surface_max = want ? (how == 0 ? pour : how == 1 ? pour + 0.25 : pour - tol / 2) : (how == 0 ? nextafter(pour - tol, 0.0) : pour - 1.0);
  }
  return t;
}

struct Reference {
  std::vector<wdpm_pond_spill> table;
  wdpm_pond_spill_stats stats;
};

static Reference reference(const Tables &t, double tol) {
  const int n = (int)t.out.size();
  Reference ref;
  ref.table.assign((size_t)n, wdpm_pond_spill());
  memset(&ref.stats, 0, sizeof ref.stats);
  std::vector<int> next((size_t)n), stamp((size_t)n, 0), place((size_t)n, 0);
  std::vector<char> spill((size_t)n), on_ring((size_t)n, 0);
  for (int k = 0; k < n; k++) {
    next[k] = t.out[k].to_basin;
    volatile double headroom = t.out[k].pour_level - t.rims[k].surface_max;
    spill[k] = next[k] >= 0 && headroom <= tol;
  }
  /* rings: walk from every pond not yet walked over; meeting this walk's own path closes a ring */
  std::vector<int> to = next;
  for (int start = 1; start <= n; start++) {
    std::vector<int> path;
    int k = start;
    while (k > 0 && stamp[k - 1] == 0) {
      stamp[k - 1] = start;
      place[k - 1] = (int)path.size();
      path.push_back(k);
      k = to[k - 1];
    }
    if (k > 0 && stamp[k - 1] == start) {
      int head = k;
      for (size_t i = (size_t)place[k - 1]; i < path.size(); i++) {
        on_ring[path[i] - 1] = 1;
        head = std::min(head, path[i]);
        ref.stats.ring_ponds++;
      }
      next[head - 1] = -2;
      ref.stats.rings++;
    }
  }
  /* chains: from the end backwards */
  std::vector<char> known((size_t)n, 0);
  for (int start = 1; start <= n; start++) {
    std::vector<int> path;
    int k = start;
    while (!known[k - 1] && next[k - 1] > 0) {
      path.push_back(k);
      k = next[k - 1];
      if ((int)path.size() > n) abort();                         /* the heads are cut: no walk comes back */
    }
    if (!known[k - 1]) {
      wdpm_pond_spill &r = ref.table[k - 1];
      r.sink = r.rest = k;
      r.path_fill_q = t.out[k - 1].fill_q;
      known[k - 1] = 1;
    }
    for (size_t i = path.size(); i-- > 0;) {
      const int p = path[i], j = next[p - 1];
      wdpm_pond_spill &r = ref.table[p - 1];
      const wdpm_pond_spill &d = ref.table[j - 1];
      r.sink = d.sink;
      r.hops = d.hops + 1;
      r.path_fill_q = t.out[p - 1].fill_q + d.path_fill_q;
      r.rest = spill[p - 1] ? d.rest : p;
      r.rest_hops = spill[p - 1] ? d.rest_hops + 1 : 0;
      known[p - 1] = 1;
    }
  }
  std::vector<int> order((size_t)n);
  std::iota(order.begin(), order.end(), 1);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return ref.table[x - 1].hops > ref.table[y - 1].hops; });
  for (int k = 0; k < n; k++) {
    wdpm_pond_spill &r = ref.table[k];
    r.next = next[k];
    r.end = next[r.sink - 1];
    r.spilling = spill[k];
    r.up_ponds = r.live_ponds = 1;
    r.up_cells = r.live_cells = t.ponds[k].cells + t.cat[k].catch_cells;
    r.up_fill_q = t.out[k].fill_q;
  }
  for (int k : order) {                                          /* the ponds furthest from their sinks first */
    const int j = next[k - 1];
    if (j <= 0) continue;
    const wdpm_pond_spill &r = ref.table[k - 1];
    wdpm_pond_spill &d = ref.table[j - 1];
    d.up_ponds += r.up_ponds;
    d.up_cells += r.up_cells;
    d.up_fill_q += r.up_fill_q;
    if (spill[k - 1]) {
      d.live_ponds += r.live_ponds;
      d.live_cells += r.live_cells;
    }
  }
  for (int k = 0; k < n; k++) {
    ref.stats.spilling += spill[k];
    ref.stats.ends_land += next[k] == 0;
    ref.stats.ends_none += next[k] == -1;
    ref.stats.ends_ring += next[k] == -2;
    ref.stats.max_hops = std::max<int64_t>(ref.stats.max_hops, ref.table[k].hops);
  }
  ref.stats.ponds = n;
  return ref;
}

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s random|ring|chain|hub|votes N SEED FLAGS\n", argv[0]);
    return 2;
  }
  std::mt19937_64 rng((unsigned long long)atoll(argv[3]) * 7919u + 13u);
  const std::vector<int> to = make_graph(argv[1], atoi(argv[2]), rng);
  const Tables t = make_tables(to, atoi(argv[4]), rng);
  const long long n = (long long)to.size();
  const double tol = 1.0 / 1024;
  emu_init();

  /* every array a vector of its own, of exact size: the sanitizer sees a stray index */
  std::vector<std::vector<int>> words(kSpillWords, std::vector<int>((size_t)n, -77));
  std::vector<std::vector<unsigned long long>> longs(4, std::vector<unsigned long long>((size_t)n, 77ull));
  std::vector<unsigned long long> acc0((size_t)(kAccs * n), 77ull), acc1((size_t)(kAccs * n), 77ull);
  SpillArrays a;
  int **w[kSpillWords] = {&a.next, &a.flag, &a.mark, &a.ptr[0], &a.ptr[1], &a.low[0], &a.low[1], &a.link[0], &a.link[1], &a.hops[0], &a.hops[1],
                          &a.llink[0], &a.llink[1], &a.lhops[0], &a.lhops[1]};
  for (int j = 0; j < kSpillWords; j++) *w[j] = words[j].data();
  a.cells = longs[0].data();
  a.fq = longs[1].data();
  a.path[0] = longs[2].data();
  a.path[1] = longs[3].data();
  a.acc[0] = acc0.data();
  a.acc[1] = acc1.data();
  std::vector<wdpm_pond_spill> table((size_t)n);
  SpillStatus st;
  memset(&st, 0, sizeof st);
  const int rounds = spill_rounds(n);
  const unsigned blocks = blocks_for(n, kBlock);
  /* the launches of wdpm_spill_label */
  launch_waves(blocks, [&] { spill_init_kernel(n, t.ponds.data(), t.rims.data(), t.cat.data(), t.out.data(), tol, a, &st); });
  for (int r = 0; r < rounds; r++) launch_waves(blocks, [&] { spill_ring_kernel(n, r, a, &st); });
  launch_waves(blocks, [&] { spill_cut_kernel(n, rounds, a, &st); });
  launch_waves(blocks, [&] { spill_chain_init_kernel(n, a, &st); });
  for (int r = 0; r < rounds; r++) launch_waves(blocks, [&] { spill_chain_kernel(n, r, a, &st); });
  launch_waves(blocks, [&] { spill_sums_init_kernel(n, a, &st); });
  for (int r = 0; r < rounds; r++) launch_waves(blocks, [&] { spill_sums_kernel(n, r, a, &st); });
  launch_waves(blocks, [&] { spill_finish_kernel(n, rounds, a, table.data(), &st); });

  const Reference ref = reference(t, tol);
  long long bad_rows = 0;
  for (long long k = 0; k < n; k++) bad_rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_spill)) != 0;
  const wdpm_pond_spill_stats &s = ref.stats;
  const bool counts = (long long)st.rings == s.rings && (long long)st.ring_ponds == s.ring_ponds && (long long)st.spilling == s.spilling &&
                      (long long)st.ends_land == s.ends_land && (long long)st.ends_none == s.ends_none && (long long)st.ends_ring == s.ends_ring &&
                      (long long)st.max_hops == s.max_hops;
  int ran[kSpillPasses];
  for (int p = 0; p < kSpillPasses; p++) {
    ran[p] = 0;
    while (ran[p] < rounds && st.work[p][ran[p]]) ran[p]++;
  }
  printf("%s %s: N %lld rings %lld ring ponds %lld spilling %lld ends land %lld none %lld ring %lld max hops %lld rounds %d ran %d %d %d  "
         "table mismatches %lld counts %s\n",
         argv[1], argv[2], n, (long long)s.rings, (long long)s.ring_ponds, (long long)s.spilling, (long long)s.ends_land, (long long)s.ends_none,
         (long long)s.ends_ring, (long long)s.max_hops, rounds, ran[0], ran[1], ran[2], bad_rows, counts ? "agree" : "DIFFER");
  return bad_rows != 0 || !counts;
}
