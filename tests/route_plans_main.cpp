/* Prints, as one JSON object, what route_plan() (wdpm_amd/csrc/wdpm_route_plan.h) decides for level sizes made up directly:
 * tests/test_pond_routing_plans.py.  Host compiler only, in the manner of tests/pair_plans_main.cpp.
 *
 *   route_plans NARROW RUN_LEVELS SIZE[xCOUNT] ...     the sizes of levels 0, 1, ...; SIZExCOUNT stands for COUNT levels of SIZE ponds
 *   route_plans bound TEXT LO HI DEFAULT               route_bound() of an environment text ("-" for an unset variable)
 */
#include <cstdio>
#include <cstring>

#include "../wdpm_amd/csrc/wdpm_route_plan.h"

int main(int argc, char **argv) {
  if (argc == 6 && !strcmp(argv[1], "bound")) {
    printf("%d\n", route_bound(strcmp(argv[2], "-") ? argv[2] : nullptr, atoi(argv[3]), atoi(argv[4]), atoi(argv[5])));
    return 0;
  }
  if (argc < 3) return 2;
  std::vector<int> offsets(1, 0);
  for (int i = 3; i < argc; i++) {
    int size = 0, count = 1;
    if (sscanf(argv[i], "%dx%d", &size, &count) < 1) return 2;
    for (int c = 0; c < count; c++) offsets.push_back(offsets.back() + size);
  }
  const int levels = (int)offsets.size() - 1;
  const RoutePlan p = route_plan(offsets.data(), levels, atoi(argv[1]), atoi(argv[2]));
  printf("{\"levels\": %d, \"wide_levels\": %lld, \"launches\": [", levels, p.wide_levels);
  for (size_t i = 0; i < p.launches.size(); i++) {
    const RouteLaunch &l = p.launches[i];
    printf("%s[%d, %d, %d, %d, %d]", i ? ", " : "", l.top, l.levels, l.wide ? 1 : 0, l.first, l.count);
  }
  printf("]}\n");
  return 0;
}
