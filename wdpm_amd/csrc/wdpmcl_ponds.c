/*
 * wdpmcl_ponds.c - the pond files of the WDPMCL command line: one CSV per pond unit of the final water, each asked for by a
 * variable of its own.  Nothing of it goes to stdout, and the run's raster never depends on it.
 *
 *   WDPM_PONDS=<path>             the 8-connected water bodies, numbered by first cell (include/wdpm_ponds.h).  A pond cell holds more
 *                                 than WDPM_PONDS_MIN_DEPTH_MM of water (default 1.0: the reference's own wet threshold, water > 0.001,
 *                                 WDPMCL.c:1397-1404, so the cells column sums to the wet count of the final statistics)
 *   WDPM_POND_RIMS=<path>         spill level, freeboard and shoreline of the same ponds (include/wdpm_pond_rims.h)
 *   WDPM_POND_CATCHMENTS=<path>   the dry land that drains to each of them (include/wdpm_pond_catchments.h)
 *   WDPM_POND_OUTLETS=<path>      where each basin spills and what it holds until then (include/wdpm_pond_outlets.h)
 *   WDPM_POND_CURVES=<path>       flooded area and storage by level (include/wdpm_pond_curves.h)
 *   WDPM_POND_SPILLS=<path>       where each pond's overflow ends up, what drains through it and what is connected to it now
 *                                 (include/wdpm_pond_spills.h).  A pond counts as spilling when its surface stands within
 *                                 WDPM_POND_HEADROOM_MM (default 0) of its pour level
 *   WDPM_POND_ROUTING=<path>      WDPM_POND_RUNOFF_MM (default 0) of runoff on every basin, sent down the spill graph: what each pond
 *                                 takes, keeps and passes on, and the land connected to it afterwards (include/wdpm_pond_routing.h)
 *
 * The units are the rows of one table, `units`, in that order; everything else here is written once and driven by it.  One label
 * call - that of the highest unit asked for - serves every file of the run; the tables then fetched are those the rows' `needs`
 * name.  A further unit is one more row with its typed thunks, its row printer and, if it has statistics, their tail of the stderr
 * line; a unit that can be taken over several row blocks fills the row's group_* column.
 *
 * The pond units are the HIP library's alone: weak references, so that the command line also links against a back-end that exports
 * include/wdpm.h and nothing else (a variable then says so, writes no file, and the run ends with status 4).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wdpmcl_ponds.h"
#include "../../include/wdpm_group_ponds.h"
#include "../../include/wdpm_pond_rims.h"
#include "../../include/wdpm_pond_catchments.h"
#include "../../include/wdpm_pond_outlets.h"
#include "../../include/wdpm_pond_curves.h"
#include "../../include/wdpm_pond_spills.h"
#include "../../include/wdpm_pond_routing.h"
#pragma weak wdpm_ponds_create
#pragma weak wdpm_ponds_destroy
#pragma weak wdpm_ponds_label
#pragma weak wdpm_ponds_table
#pragma weak wdpm_ponds_guard_bad
#pragma weak wdpm_group_ponds_create
#pragma weak wdpm_group_ponds_destroy
#pragma weak wdpm_group_ponds_label
#pragma weak wdpm_group_ponds_table
#pragma weak wdpm_group_ponds_guard_bad
#pragma weak wdpm_group_ponds_stats
#pragma weak wdpm_rims_label
#pragma weak wdpm_rims_table
#pragma weak wdpm_catch_label
#pragma weak wdpm_catch_table
#pragma weak wdpm_catch_stats
#pragma weak wdpm_outlets_label
#pragma weak wdpm_outlets_table
#pragma weak wdpm_outlets_stats
#pragma weak wdpm_curves_label
#pragma weak wdpm_curves_table
#pragma weak wdpm_curves_stats
#pragma weak wdpm_curves_stage_level
#pragma weak wdpm_spill_label
#pragma weak wdpm_spill_table
#pragma weak wdpm_spill_stats
#pragma weak wdpm_route_label
#pragma weak wdpm_route_table
#pragma weak wdpm_route_stats

enum { PONDS, RIMS, CATCH, OUTLETS, CURVES, SPILLS, ROUTING, UNITS };
#define BIT(u) (1u << (u))

typedef struct {
  void *table[UNITS];          /* N rows of the unit's struct each, or NULL */
  int64_t n, guard_bad, blocks, joined;
  wdpm_pond_catchment_stats catch_stats;
  wdpm_pond_outlet_stats outlet_stats;
  wdpm_pond_curve_stats curve_stats;
  wdpm_pond_spill_stats spill_stats;
  wdpm_pond_route_stats route_stats;
  double cellarea;
} pond_inventory;

typedef struct {
  const char *var, *name, *noun;                        /* "<noun> taken on a whole raster only" */
  size_t row;
  unsigned needs;                                       /* the tables a run that writes this file fetches */
  int (*there)(void);                                   /* does the back-end have the unit? */
  int (*label)(wdpm_ponds *, double, int64_t *);
  int (*table)(wdpm_ponds *, pond_inventory *);
  int (*stats)(wdpm_ponds *, pond_inventory *);         /* or NULL */
  int (*group_label)(wdpm_group_ponds *, double, int64_t *);   /* over several row blocks; NULL: whole rasters only */
  int (*group_table)(wdpm_group_ponds *, pond_inventory *);
  const char *header;
  void (*print)(FILE *, const pond_inventory *, int64_t k);    /* the lines of pond k + 1 */
  void (*tail)(const pond_inventory *, char *buf, size_t len); /* the end of the "written to" line, or NULL */
} pond_unit;

/* ---- the calls of each unit, typed ---- */
static int ponds_there(void) { return wdpm_ponds_create && wdpm_ponds_destroy && wdpm_ponds_label && wdpm_ponds_table && wdpm_ponds_guard_bad; }
static int group_there(void) {
  return wdpm_group_ponds_create && wdpm_group_ponds_destroy && wdpm_group_ponds_label && wdpm_group_ponds_table &&
         wdpm_group_ponds_guard_bad && wdpm_group_ponds_stats;
}
static int rims_there(void) { return wdpm_rims_label && wdpm_rims_table; }
static int catch_there(void) { return wdpm_catch_label && wdpm_catch_table && wdpm_catch_stats; }
static int outlets_there(void) { return wdpm_outlets_label && wdpm_outlets_table && wdpm_outlets_stats; }
static int curves_there(void) { return wdpm_curves_label && wdpm_curves_table && wdpm_curves_stats && wdpm_curves_stage_level; }
static int spills_there(void) { return wdpm_spill_label && wdpm_spill_table && wdpm_spill_stats; }
static int routing_there(void) { return wdpm_route_label && wdpm_route_table && wdpm_route_stats; }

static int ponds_table(wdpm_ponds *h, pond_inventory *v) { return wdpm_ponds_table(h, (wdpm_pond *)v->table[PONDS], v->n); }
static int group_ponds_table(wdpm_group_ponds *g, pond_inventory *v) { return wdpm_group_ponds_table(g, (wdpm_pond *)v->table[PONDS], v->n); }
static int rims_table(wdpm_ponds *h, pond_inventory *v) { return wdpm_rims_table(h, (wdpm_pond_rim *)v->table[RIMS], v->n); }
static int catch_table(wdpm_ponds *h, pond_inventory *v) { return wdpm_catch_table(h, (wdpm_pond_catchment *)v->table[CATCH], v->n); }
static int catch_stats(wdpm_ponds *h, pond_inventory *v) { return wdpm_catch_stats(h, &v->catch_stats); }
static int outlets_table(wdpm_ponds *h, pond_inventory *v) { return wdpm_outlets_table(h, (wdpm_pond_outlet *)v->table[OUTLETS], v->n); }
static int outlets_stats(wdpm_ponds *h, pond_inventory *v) { return wdpm_outlets_stats(h, &v->outlet_stats); }
static int curves_table(wdpm_ponds *h, pond_inventory *v) { return wdpm_curves_table(h, (wdpm_pond_curve *)v->table[CURVES], v->n); }
static int curves_stats(wdpm_ponds *h, pond_inventory *v) { return wdpm_curves_stats(h, &v->curve_stats); }
/* the spill pass takes a second parameter, read once (wdpmcl_pond_files) before the row's label call */
static double headroom_tol;
static int spills_label(wdpm_ponds *h, double min_depth, int64_t *n) { return wdpm_spill_label(h, min_depth, headroom_tol, n); }
static int spills_table(wdpm_ponds *h, pond_inventory *v) { return wdpm_spill_table(h, (wdpm_pond_spill *)v->table[SPILLS], v->n); }
static int spills_stats(wdpm_ponds *h, pond_inventory *v) { return wdpm_spill_stats(h, &v->spill_stats); }
/* and the routing pass a third, read beside it */
static double runoff_m;
static int routing_label(wdpm_ponds *h, double min_depth, int64_t *n) { return wdpm_route_label(h, min_depth, headroom_tol, runoff_m, n); }
static int routing_table(wdpm_ponds *h, pond_inventory *v) { return wdpm_route_table(h, (wdpm_pond_route *)v->table[ROUTING], v->n); }
static int routing_stats(wdpm_ponds *h, pond_inventory *v) { return wdpm_route_stats(h, &v->route_stats); }

/* ---- the row printers: coordinates leave as file coordinates, 0-based (padded - 1), -1 where there is none; doubles as %.17g
 * so that they read back exactly; volumes in quanta of 2^-24 m and in cubic metres ---- */
static void print_pond(FILE *f, const pond_inventory *v, int64_t k) {
  const wdpm_pond *q = (const wdpm_pond *)v->table[PONDS] + k;
  fprintf(f, "%lld,%d,%d,%lld,%.17g,%llu,%.17g,%.17g,%d,%d,%d,%d\n", (long long)(k + 1), q->first_row - 1, q->first_col - 1,
          (long long)q->cells, (double)q->cells * v->cellarea, (unsigned long long)q->volume_q,
          ldexp((double)q->volume_q, -24) * v->cellarea, q->max_depth, q->row_min - 1, q->row_max - 1, q->col_min - 1, q->col_max - 1);
}

/* freeboard = rim level - highest surface */
static void print_rim(FILE *f, const pond_inventory *v, int64_t k) {
  const wdpm_pond_rim *q = (const wdpm_pond_rim *)v->table[RIMS] + k;
  const int none = q->rim_row < 0;
  fprintf(f, "%lld,%.17g,%.17g,%.17g,%.17g,%d,%d,%lld,%lld\n", (long long)(k + 1), q->surface_min, q->surface_max, q->rim_level,
          q->rim_level - q->surface_max, none ? -1 : q->rim_row - 1, none ? -1 : q->rim_col - 1, (long long)q->rim_cells,
          (long long)q->wall_cells);
}

/* head level -inf: no cell drains to the pond; the box is that of pond and catchment together */
static void print_catchment(FILE *f, const pond_inventory *v, int64_t k) {
  const wdpm_pond_catchment *q = (const wdpm_pond_catchment *)v->table[CATCH] + k;
  fprintf(f, "%lld,%lld,%.17g,%lld,%.17g,%d,%d,%d,%d\n", (long long)(k + 1), (long long)q->catch_cells,
          (double)q->catch_cells * v->cellarea, (long long)q->inflow_cells, q->head_level, q->row_min - 1, q->row_max - 1,
          q->col_min - 1, q->col_max - 1);
}

/* headroom = pour level - highest surface, which the rim table holds; to_label 0: land that ends in a pit, -1: none */
static void print_outlet(FILE *f, const pond_inventory *v, int64_t k) {
  const wdpm_pond_outlet *q = (const wdpm_pond_outlet *)v->table[OUTLETS] + k;
  const int none = q->from_row < 0;
  fprintf(f, "%lld,%.17g,%.17g,%d,%d,%d,%d,%d,%lld,%lld,%.17g,%llu,%.17g\n", (long long)(k + 1), q->pour_level,
          q->pour_level - ((const wdpm_pond_rim *)v->table[RIMS])[k].surface_max, none ? -1 : q->from_row - 1,
          none ? -1 : q->from_col - 1, none ? -1 : q->to_row - 1, none ? -1 : q->to_col - 1, q->to_basin, (long long)q->divide_cells,
          (long long)q->fill_cells, (double)q->fill_cells * v->cellarea, (unsigned long long)q->fill_q,
          ldexp((double)q->fill_q, -24) * v->cellarea);
}

/* one line `stage 0` with the lowest ground of the pond's basin and zeros, and - where the pond has an outlet - one line per stage
 * 1..16 with its level (wdpm_curves_stage_level; stage 16 is the pour level), the cells of the basin below it and the storage */
static void print_curve(FILE *f, const pond_inventory *v, int64_t k) {
  const wdpm_pond_curve *q = (const wdpm_pond_curve *)v->table[CURVES] + k;
  fprintf(f, "%lld,0,%.17g,0,%.17g,0,%.17g\n", (long long)(k + 1), q->bed_level, 0.0, 0.0);
  if (!(q->top_level < INFINITY)) return;
  for (int s = 1; s <= WDPM_CURVE_STAGES; s++)
    fprintf(f, "%lld,%d,%.17g,%lld,%.17g,%llu,%.17g\n", (long long)(k + 1), s, wdpm_curves_stage_level(q->bed_level, q->top_level, s),
            (long long)q->cells[s - 1], (double)q->cells[s - 1] * v->cellarea, (unsigned long long)q->q[s - 1],
            ldexp((double)q->q[s - 1], -24) * v->cellarea);
}

/* next_label / end: 0 land that ends in a pit, -1 no outlet, -2 a ring of ponds closed at this pond; up_* once everything above is
 * full, live_* through the ponds that spill now */
static void print_spill(FILE *f, const pond_inventory *v, int64_t k) {
  const wdpm_pond_spill *q = (const wdpm_pond_spill *)v->table[SPILLS] + k;
  fprintf(f, "%lld,%d,%d,%d,%d,%d,%llu,%.17g,%lld,%lld,%.17g,%llu,%.17g,%d,%d,%lld,%lld,%.17g\n", (long long)(k + 1), q->next, q->spilling,
          q->sink, q->end, q->hops, (unsigned long long)q->path_fill_q, ldexp((double)q->path_fill_q, -24) * v->cellarea,
          (long long)q->up_ponds, (long long)q->up_cells, (double)q->up_cells * v->cellarea, (unsigned long long)q->up_fill_q,
          ldexp((double)q->up_fill_q, -24) * v->cellarea, q->rest, q->rest_hops, (long long)q->live_ponds, (long long)q->live_cells,
          (double)q->live_cells * v->cellarea);
}

/* what the pond takes, keeps and passes on in quanta of 2^-24 m times cells, the overflow also in cubic metres; reach_*: the pond
 * itself and what is connected to it through ponds that overflow */
static void print_route(FILE *f, const pond_inventory *v, int64_t k) {
  const wdpm_pond_route *q = (const wdpm_pond_route *)v->table[ROUTING] + k;
  fprintf(f, "%lld,%d,%llu,%llu,%llu,%llu,%.17g,%d,%d,%lld,%lld,%.17g\n", (long long)(k + 1), q->level, (unsigned long long)q->own_q,
          (unsigned long long)q->in_q, (unsigned long long)q->kept_q, (unsigned long long)q->out_q, ldexp((double)q->out_q, -24) * v->cellarea,
          q->full, q->overflows, (long long)q->reach_ponds, (long long)q->reach_cells, (double)q->reach_cells * v->cellarea);
}

static void tail_ponds(const pond_inventory *v, char *buf, size_t len) {
  if (v->blocks > 1) snprintf(buf, len, " (%lld row blocks, %lld joined across them)", (long long)v->blocks, (long long)v->joined);
}
static void tail_catchments(const pond_inventory *v, char *buf, size_t len) {
  const wdpm_pond_catchment_stats *s = &v->catch_stats;
  snprintf(buf, len, " (%lld slope cells, %lld pits, %lld cells drain to no pond, %lld rounds)", (long long)s->slope_cells,
           (long long)s->pit_cells, (long long)s->unponded_cells, (long long)s->rounds);
}
static void tail_outlets(const pond_inventory *v, char *buf, size_t len) {
  const wdpm_pond_outlet_stats *s = &v->outlet_stats;
  snprintf(buf, len, " (%lld without an outlet, %lld spill onto land that ends in a pit, %lld cells on the divides)",
           (long long)s->no_outlet, (long long)s->to_land, (long long)s->divide_cells);
}
static void tail_curves(const pond_inventory *v, char *buf, size_t len) {
  const wdpm_pond_curve_stats *s = &v->curve_stats;
  snprintf(buf, len, " (%lld without a curve, %lld flat, %lld cells below the last stage)", (long long)s->no_curve, (long long)s->flat,
           (long long)s->stage_cells);
}
static void tail_spills(const pond_inventory *v, char *buf, size_t len) {
  const wdpm_pond_spill_stats *s = &v->spill_stats;
  snprintf(buf, len, " (%lld rings of %lld ponds, %lld spilling, chains end: %lld on land, %lld without an outlet, %lld at a ring; longest chain %lld)",
           (long long)s->rings, (long long)s->ring_ponds, (long long)s->spilling, (long long)s->ends_land, (long long)s->ends_none,
           (long long)s->ends_ring, (long long)s->max_hops);
}

static void tail_routing(const pond_inventory *v, char *buf, size_t len) {
  const wdpm_pond_route_stats *s = &v->route_stats;
  snprintf(buf, len, " (%.17g mm of runoff: %lld full, %lld overflowing, %.17g m3 kept, %.17g m3 left over land, %.17g m3 at rings; %lld levels)",
           ldexp((double)s->runoff_q, -24) * 1000.0, (long long)s->full, (long long)s->overflowing, ldexp((double)s->kept_q, -24) * v->cellarea,
           ldexp((double)s->out_land_q, -24) * v->cellarea, ldexp((double)s->out_ring_q, -24) * v->cellarea, (long long)s->levels);
}

/* ---- the table.  needs: an outlets file reads the rim table for its headroom and fetches the catchment table with it; a curves
 * file, a spills file and a routing file each read their own table alone ---- */
static const pond_unit units[UNITS] = {
    {"WDPM_PONDS", "pond inventory", NULL, sizeof(wdpm_pond), BIT(PONDS), ponds_there, wdpm_ponds_label, ponds_table, NULL,
     wdpm_group_ponds_label, group_ponds_table,
     "label,row,col,cells,area_m2,volume_q,volume_m3,max_depth_m,row_min,row_max,col_min,col_max", print_pond, tail_ponds},
    {"WDPM_POND_RIMS", "pond rims", "rims are", sizeof(wdpm_pond_rim), BIT(PONDS) | BIT(RIMS), rims_there, wdpm_rims_label, rims_table,
     NULL, NULL, NULL, "label,surface_min_m,surface_max_m,rim_level_m,freeboard_m,rim_row,rim_col,rim_cells,wall_cells", print_rim, NULL},
    {"WDPM_POND_CATCHMENTS", "pond catchments", "catchments are", sizeof(wdpm_pond_catchment), BIT(PONDS) | BIT(RIMS) | BIT(CATCH),
     catch_there, wdpm_catch_label, catch_table, catch_stats, NULL, NULL,
     "label,catch_cells,catch_area_m2,inflow_cells,head_level_m,row_min,row_max,col_min,col_max", print_catchment, tail_catchments},
    {"WDPM_POND_OUTLETS", "pond outlets", "outlets are", sizeof(wdpm_pond_outlet), BIT(PONDS) | BIT(RIMS) | BIT(CATCH) | BIT(OUTLETS),
     outlets_there, wdpm_outlets_label, outlets_table, outlets_stats, NULL, NULL,
     "label,pour_level_m,headroom_m,from_row,from_col,to_row,to_col,to_label,divide_cells,fill_cells,fill_area_m2,fill_q,fill_m3",
     print_outlet, tail_outlets},
    {"WDPM_POND_CURVES", "pond curves", "stage curves are", sizeof(wdpm_pond_curve), BIT(PONDS) | BIT(CURVES), curves_there,
     wdpm_curves_label, curves_table, curves_stats, NULL, NULL, "label,stage,level_m,cells,area_m2,q,volume_m3", print_curve, tail_curves},
    {"WDPM_POND_SPILLS", "pond spills", "spills are", sizeof(wdpm_pond_spill), BIT(PONDS) | BIT(SPILLS), spills_there, spills_label,
     spills_table, spills_stats, NULL, NULL,
     "label,next_label,spilling,sink_label,end,hops,path_fill_q,path_fill_m3,up_ponds,up_cells,up_area_m2,up_fill_q,up_fill_m3,rest_label,"
     "rest_hops,live_ponds,live_cells,live_area_m2",
     print_spill, tail_spills},
    {"WDPM_POND_ROUTING", "pond routing", "routing is", sizeof(wdpm_pond_route), BIT(PONDS) | BIT(ROUTING), routing_there, routing_label,
     routing_table, routing_stats, NULL, NULL,
     "label,level,own_q,in_q,kept_q,out_q,out_m3,full,overflows,reach_ponds,reach_cells,reach_area_m2", print_route, tail_routing},
};

static void free_tables(pond_inventory *v) {
  for (int u = 0; u < UNITS; u++) {
    free(v->table[u]);
    v->table[u] = NULL;
  }
}

/* label once for the highest unit of `asked`, then fetch what its units need: on the group's one context, or - ndev > 1 - over
 * its row blocks with every block labelled where it lies (include/wdpm_group_ponds.h).  Non-zero: said why, nothing is held. */
static int take_inventory(wdpm_group *grp, int ndev, unsigned asked, double min_depth, pond_inventory *v) {
  const int group = ndev > 1;
  wdpm_ponds *h = NULL;
  wdpm_group_ponds *g = NULL;
  int top = PONDS;
  unsigned fetch = 0;
  for (int u = 0; u < UNITS; u++)
    if (asked & BIT(u)) {
      top = u;
      fetch |= units[u].needs;
    }
  if (!(group ? group_there() : ponds_there())) {
    fprintf(stderr, "WDPMCL: pond inventory: back-end %s has none, no file written\n", wdpm_backend_name());
    return 1;
  }
  int rc = group ? wdpm_group_ponds_create(&g, grp) : wdpm_ponds_create(&h, wdpm_rank_ctx(wdpm_group_rank(grp, 0)));
  if (!rc) rc = group ? units[top].group_label(g, min_depth, &v->n) : units[top].label(h, min_depth, &v->n);
  if (!rc && group) {
    wdpm_group_pond_stats gs;
    rc = wdpm_group_ponds_stats(g, &gs);
    if (!rc) {
      v->blocks = gs.ranks;
      v->joined = gs.merged;
    }
  }
  for (int u = 0; !rc && u < UNITS; u++)
    if (fetch & BIT(u)) {
      v->table[u] = malloc((size_t)(v->n > 0 ? v->n : 1) * units[u].row);
      if (!v->table[u]) {
        wdpm_set_last_error("out of host memory for the pond table");
        rc = 1;
      }
    }
  for (int u = 0; !rc && u < UNITS; u++)
    if (fetch & BIT(u)) {
      rc = group ? units[u].group_table(g, v) : units[u].table(h, v);
      if (!rc && !group && units[u].stats) rc = units[u].stats(h, v);
    }
  if (!rc && getenv("WDPM_GUARD_KB")) rc = group ? wdpm_group_ponds_guard_bad(g, &v->guard_bad) : wdpm_ponds_guard_bad(h, &v->guard_bad);
  if (rc) {
    fprintf(stderr, "WDPMCL: pond inventory failed, no file written: %s\n", wdpm_last_error());
    free_tables(v);
  }
  if (!group) wdpm_ponds_destroy(h);   /* takes NULL */
  else if (g) wdpm_group_ponds_destroy(g);
  return rc;
}

static int write_unit(const pond_unit *u, const char *path, const pond_inventory *v) {
  char tail[384] = "";
  FILE *f = fopen(path, "w");
  if (!f) {
    fprintf(stderr, "WDPMCL: cannot write %s %s\n", u->name, path);
    return 1;
  }
  fprintf(f, "%s\n", u->header);
  for (int64_t k = 0; k < v->n; k++) u->print(f, v, k);
  const int bad = ferror(f);
  if (fclose(f) != 0 || bad) {
    fprintf(stderr, "WDPMCL: error writing %s %s\n", u->name, path);
    return 1;
  }
  if (u->tail) u->tail(v, tail, sizeof tail);
  fprintf(stderr, "WDPMCL: %s: %lld pond%s written to %s%s\n", u->name, (long long)v->n, v->n == 1 ? "" : "s", path, tail);
  return 0;
}

int wdpmcl_pond_files(wdpm_group *grp, int ndev, double cellarea, int64_t *guard_bad, void (*phase)(const char *name)) {
  const char *path[UNITS];
  unsigned asked = 0;
  int failed = 0, there = 1;
  *guard_bad = 0;
  for (int u = 0; u < UNITS; u++) {
    path[u] = getenv(units[u].var);
    if (path[u] && !*path[u]) path[u] = NULL;
    if (path[u] && ndev > 1 && !units[u].group_label) {
      fprintf(stderr, "WDPMCL: %s: the raster lies in %d row blocks and %s taken on a whole raster only, no file written to %s\n",
              units[u].name, ndev, units[u].noun, path[u]);
      failed = 1;
      path[u] = NULL;
    }
    /* a unit stands on those below it; whether the inventory itself is there is the handle's to say (take_inventory) */
    if (u > PONDS) there = there && units[u].there();
    if (path[u] && !there) {
      fprintf(stderr, "WDPMCL: %s: back-end %s has none, no file written\n", units[u].name, wdpm_backend_name());
      failed = 1;
      path[u] = NULL;
    }
    if (path[u]) asked |= BIT(u);
  }
  if (!asked) return failed;
  const double min_depth = (getenv("WDPM_PONDS_MIN_DEPTH_MM") ? atof(getenv("WDPM_PONDS_MIN_DEPTH_MM")) : 1.0) / 1000.0;
  headroom_tol = (getenv("WDPM_POND_HEADROOM_MM") ? atof(getenv("WDPM_POND_HEADROOM_MM")) : 0.0) / 1000.0;
  runoff_m = (getenv("WDPM_POND_RUNOFF_MM") ? atof(getenv("WDPM_POND_RUNOFF_MM")) : 0.0) / 1000.0;
  pond_inventory v;
  memset(&v, 0, sizeof v);
  v.blocks = 1;
  v.cellarea = cellarea;
  phase("statistics + download");
  if (take_inventory(grp, ndev, asked, min_depth, &v)) failed = 1;
  else
    for (int u = 0; u < UNITS; u++)
      if (path[u] && write_unit(&units[u], path[u], &v)) failed = 1;
  free_tables(&v);
  *guard_bad = v.guard_bad;
  phase("pond inventory");
  return failed;
}
