/* Host emulation of the routing kernels (wdpm_amd/csrc/wdpm_pond_routing.hip, compiled with WDPM_PONDS_EMULATION), after the pattern
 * of tests/spills_emu_main.cpp: the kernels' own source runs as 256 threads per block - a real block barrier between the levels of a
 * run - atomics as host atomics.  Built with -fsanitize=address,undefined by tests/test_pond_routing_emulation.py: a lane that reads
 * outside a table or an array is found here, on a CPU.  The unit reads no raster, so the tables are made up directly - a forest in
 * next, its hops, random cells, catchments and fill_q - every array is a vector of exactly its length, and the whole table and the
 * totals are held against a sequential walk, the ponds with the most hops first.
 *
 *   routing_emu KIND N SEED NARROW RUN_LEVELS RUNOFF_Q [RUNOFF_Q ...]
 *     KIND    random: every pond spills into a random pond with a smaller label, onto land, nowhere, or is a ring's head
 *             chain:  N -> N - 1 -> ... -> 1 -> land
 *             hub:    ponds 2 .. N + 1 all spill into pond 1
 *             ladder: three levels of exactly N ponds, pond j of a level into pond 7 j mod N of the level below
 *             exact:  1 -> 2 -> 3 -> land where 5 quanta fill pond 2 exactly (N = 0) or leave one quantum over (N = 1)
 *     NARROW, RUN_LEVELS   the planner's two bounds (wdpm_route_plan.h)
 *     RUNOFF_Q             the first is the label call's; every further one is a rerun on the same state
 */
#include "hip_emu.h"
#include "../wdpm_amd/csrc/wdpm_pond_routing.hip"

#include <random>

/* one launch of a kernel that never meets at a block barrier: a wave waits for nobody except its own 64 lanes (tests/spills_emu_main.cpp) */
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
  std::vector<wdpm_pond_catchment> cat;
  std::vector<wdpm_pond_outlet> out;
  std::vector<wdpm_pond_spill> spill;
};

static Tables make_tables(const std::string &kind, int size, std::mt19937_64 &rng) {
  std::vector<int> next;
  auto below = [&](int n) { return (int)(rng() % (unsigned long long)n); };
  if (kind == "random") {
    for (int k = 1; k <= size; k++) {
      const int u = below(100);
      next.push_back(k == 1 || u < 4 ? 0 : u < 8 ? -1 : u < 10 ? -2 : 1 + below(k - 1));
    }
  } else if (kind == "chain") {
    for (int k = 1; k <= size; k++) next.push_back(k - 1);
  } else if (kind == "hub") {
    next.push_back(0);
    for (int k = 2; k <= size + 1; k++) next.push_back(1);
  } else if (kind == "ladder") {
    for (int l = 0; l < 3; l++)
      for (int j = 0; j < size; j++) next.push_back(l == 0 ? (j % 3 == 0 ? -2 : 0) : (l - 1) * size + (7 * j) % size + 1);
  } else {
    next = {2, 3, 0};
  }
  const size_t n = next.size();
  Tables t;
  t.ponds.assign(n, wdpm_pond());
  t.cat.assign(n, wdpm_pond_catchment());
  t.out.assign(n, wdpm_pond_outlet());
  t.spill.assign(n, wdpm_pond_spill());
  for (size_t k = 0; k < n; k++) {
    t.ponds[k].cells = 1 + (long long)(rng() % 5000);
    t.cat[k].catch_cells = (long long)(rng() % 100000);
    const unsigned long long area = (unsigned long long)(t.ponds[k].cells + t.cat[k].catch_cells);
    const int depth = 8 + 11 * (int)(rng() % 3);               /* shallow, middling and deep storage */
    t.out[k].to_basin = next[k] == -2 ? 1 : next[k];
    t.out[k].fill_q = next[k] == -1 ? 0ull : rng() % (area << depth);
    t.spill[k].next = next[k];
    t.spill[k].hops = next[k] > 0 ? t.spill[(size_t)next[k] - 1].hops + 1 : 0;      /* every pond spills into a smaller label */
  }
  if (kind == "exact") {                                        /* the one graph whose labels rise downstream */
    const long long cells[3] = {10, 20, 30};
    const unsigned long long fill[3] = {20ull, size ? 129ull : 130ull, 1000ull};
    for (int k = 0; k < 3; k++) {
      t.ponds[k].cells = cells[k];
      t.cat[k].catch_cells = 0;
      t.out[k].fill_q = fill[k];
      t.spill[k].hops = 2 - k;
    }
  }
  return t;
}

struct Reference {
  std::vector<wdpm_pond_route> table;
  RouteStatus status;
};

static Reference reference(const Tables &t, unsigned long long q) {
  const int n = (int)t.spill.size();
  Reference ref;
  ref.table.assign((size_t)n, wdpm_pond_route());
  memset(&ref.status, 0, sizeof ref.status);
  std::vector<int> order((size_t)n);
  for (int k = 0; k < n; k++) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return t.spill[x].hops > t.spill[y].hops; });
  for (int k = 0; k < n; k++) {
    wdpm_pond_route &r = ref.table[k];
    r.reach_ponds = 1;
    r.reach_cells = t.ponds[k].cells + t.cat[k].catch_cells;
    r.own_q = q * (unsigned long long)r.reach_cells;
    r.level = t.spill[k].hops;
  }
  for (int k : order) {                                          /* the ponds furthest from their sinks first */
    wdpm_pond_route &r = ref.table[k];
    const int next = t.spill[k].next;
    const unsigned long long all = r.own_q + r.in_q, fill = t.out[k].fill_q;
    r.out_q = next != -1 && all > fill ? all - fill : 0ull;
    r.kept_q = all - r.out_q;
    r.overflows = r.out_q != 0ull;
    r.full = next != -1 && all >= fill;
    if (next > 0 && r.overflows) {
      wdpm_pond_route &d = ref.table[(size_t)next - 1];
      d.in_q += r.out_q;
      d.reach_ponds += r.reach_ponds;
      d.reach_cells += r.reach_cells;
    }
    ref.status.overflowing += (unsigned long long)r.overflows;
    ref.status.full += (unsigned long long)r.full;
    ref.status.own_q += r.own_q;
    ref.status.kept_q += r.kept_q;
    if (next == 0) ref.status.out_land_q += r.out_q;
    if (next == -2) ref.status.out_ring_q += r.out_q;
  }
  return ref;
}

int main(int argc, char **argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: %s random|chain|hub|ladder|exact N SEED NARROW RUN_LEVELS RUNOFF_Q [RUNOFF_Q ...]\n", argv[0]);
    return 2;
  }
  std::mt19937_64 rng((unsigned long long)atoll(argv[3]) * 7919u + 13u);
  const Tables t = make_tables(argv[1], atoi(argv[2]), rng);
  const long long n = (long long)t.spill.size();
  const int narrow = atoi(argv[4]), run_levels = atoi(argv[5]);
  int levels = 0;
  for (const wdpm_pond_spill &s : t.spill) levels = std::max(levels, s.hops + 1);
  emu_init();

  /* every array a vector of its own, of exact size: the sanitizer sees a stray index */
  std::vector<int> next((size_t)n, -77), level((size_t)n, -77), order((size_t)n, -77), offsets((size_t)levels + 1, 0), cursor((size_t)levels, -77);
  std::vector<unsigned long long> area((size_t)n, 77ull), fq((size_t)n, 77ull), acc((size_t)(kRouteAccs * n), 77ull);
  std::vector<wdpm_pond_route> table((size_t)n);
  RouteArrays a;
  a.next = next.data();
  a.level = level.data();
  a.order = order.data();
  a.offsets = offsets.data();
  a.cursor = cursor.data();
  a.area = area.data();
  a.fq = fq.data();
  a.acc = acc.data();
  const unsigned blocks = blocks_for(n, kBlock);
  /* the launches of wdpm_route_label: order ... */
  launch_waves(blocks, [&] { route_init_kernel(n, t.ponds.data(), t.cat.data(), t.out.data(), t.spill.data(), a); });
  launch(1, [&] { route_scan_kernel(levels, a); });
  launch_waves(blocks, [&] { route_scatter_kernel(n, a); });
  bool sorted = offsets[0] == 0 && offsets[(size_t)levels] == n;
  std::vector<char> seen((size_t)n, 0);
  for (int l = 0; l < levels; l++) {
    sorted = sorted && cursor[l] == offsets[(size_t)l + 1];
    for (int i = offsets[l]; i < offsets[(size_t)l + 1]; i++) {
      const int pond = order[i];
      sorted = sorted && pond >= 1 && pond <= n && !seen[(size_t)pond - 1] && t.spill[(size_t)pond - 1].hops == l;
      if (pond >= 1 && pond <= n) seen[(size_t)pond - 1] = 1;
    }
  }
  const RoutePlan plan = route_plan(offsets.data(), levels, narrow, run_levels);
  /* ... then sweep and finish, once per runoff */
  long long bad_rows = 0, bad_totals = 0;
  for (int r = 6; r < argc; r++) {
    const unsigned long long q = strtoull(argv[r], nullptr, 10);
    RouteStatus st;
    memset(&st, 0, sizeof st);
    std::fill(acc.begin(), acc.end(), 0ull);
    for (const RouteLaunch &l : plan.launches) {
      if (l.wide)
        launch_waves(blocks_for(l.count, kBlock), [&] { route_level_kernel(l.first, l.count, l.top == 0, n, q, a, &st); });
      else
        launch(1, [&] { route_run_kernel(l.top, l.levels, n, q, a, &st); });
    }
    launch_waves(blocks, [&] { route_finish_kernel(n, q, a, table.data(), &st); });
    const Reference ref = reference(t, q);
    long long rows = 0;
    for (long long k = 0; k < n; k++) rows += memcmp(&ref.table[k], &table[k], sizeof(wdpm_pond_route)) != 0;
    const bool totals = memcmp(&ref.status, &st, sizeof st) == 0;
    printf("%s %s runoff_q %llu: N %lld levels %d launches %zu wide %lld overflowing %llu full %llu land %llu ring %llu  table mismatches %lld totals %s\n",
           argv[1], argv[2], q, n, levels, plan.launches.size(), plan.wide_levels, ref.status.overflowing, ref.status.full, ref.status.out_land_q,
           ref.status.out_ring_q, rows, totals ? "agree" : "DIFFER");
    if (!strcmp(argv[1], "exact") && n == 3)
      printf("exact: in %llu %llu %llu out %llu %llu %llu full %d %d %d reach %lld %lld %lld\n", (unsigned long long)table[0].in_q,
             (unsigned long long)table[1].in_q, (unsigned long long)table[2].in_q, (unsigned long long)table[0].out_q, (unsigned long long)table[1].out_q,
             (unsigned long long)table[2].out_q, table[0].full, table[1].full, table[2].full, (long long)table[0].reach_ponds, (long long)table[1].reach_ponds,
             (long long)table[2].reach_ponds);
    bad_rows += rows;
    bad_totals += !totals;
  }
  printf("order %s\n", sorted ? "sorted" : "WRONG");
  return bad_rows != 0 || bad_totals != 0 || !sorted;
}
