/* tbnav_nav.h — C-ABI of the GOAL FIELD: the exact shortest-path cost-to-go to a goal cell over a cost grid, solved on the MI355X
 * and handed to the MPPI handle device to device (an OPTION; nothing changes for a handle that does not use it).
 *
 * The reference has a package for this job — planner/: a grid map with inflation (planner/src/planner/grid_map.cpp) and D* Lite
 * over the 8-connected grid (planner/src/planner/dstar_light.cpp:367-461: the eight actions at :370-373, a move priced by the cell
 * it enters, 1 or sqrt(2) cells or an occupied-cell cost, at :444-461) — but its controller never sees it: MPPI's pull towards the
 * waypoint is the quadratic distance (controller/include/controller/mppi.hpp:87-105), which points straight through whatever
 * stands in the way.  A cost field (tbnav_mppi.h, COST FIELD) that holds METRES TO GO ROUND THE WALLS instead pulls the rollouts
 * out of a pocket.  Not built: D* Lite's incremental repair (every solve starts afresh), several goals, heading-dependent costs.
 *
 * This section is the whole specification; tests/nav_restatement.py restates G1-G6 in Python integers, tests/nav_from_map_restatement.py G7-G8.
 *
 * G1. Grid.  nx, ny in 2 .. TBNAV_NAV_MAX_SIDE; (xmin, ymin), finite, are the world coordinates of the OUTER corner of cell (0, 0);
 *     resolution finite and > 0.  Cell (ix, iy) is at index ix*ny + iy (x is the slow index): the cost field's layout and, for the
 *     square grids the filter supports, tbnav_rbpf_get_occ_dist's — nothing needs transposing.  The cell of a world position:
 *       ix = (int)floor((x - xmin) * inv),  iy = (int)floor((y - ymin) * inv),  inv = 1.0 / resolution formed on the host, fp64.
 *     A position outside the grid, or not finite, is TBNAV_ERR_OUT_OF_WORLD.
 * G2. Cost grid.  uint8_t cost[nx*ny]: 0 = blocked; 1 .. TBNAV_NAV_MAX_COST is the multiplier a move pays for ENTERING the cell.
 *     A value above TBNAV_NAV_MAX_COST is TBNAV_ERR_INVALID_ARG and nothing changes.
 * G3. Moves.  From cell a to one of its 8 neighbours b, in the order of dstar_light.cpp:370-373 read as (dix, diy):
 *       (0,-1) (0,1) (-1,0) (1,0) (-1,-1) (-1,1) (1,-1) (1,1).
 *     A move is allowed when b is inside the grid and cost[a] != 0 and cost[b] != 0 and, for a diagonal move, BOTH cells
 *     orthogonally between them, (a.ix, b.iy) and (b.ix, a.iy), are non-blocked as well (the mapper draws walls with Bresenham;
 *     such a wall is only 8-connected, and without this rule every diagonal wall leaks).  Price: w * cost[b], w = 10 for a straight
 *     and 14 for a diagonal move (dstar_light.cpp:444-461 prices a move by the cell entered).  Integers on purpose: the cost-to-go
 *     is then ONE number whatever order a parallel relaxation works in, and the tests' bar is ==, not a tolerance.
 * G4. Cost-to-go.  uint32_t d[nx*ny]: d[goal] = 0; d[a] = min over allowed moves a -> b of d[b] + w*cost[b];
 *     TBNAV_NAV_UNREACHED (0xFFFFFFFF) for blocked cells and cells with no way to the goal.  It cannot overflow: a simple path
 *     enters fewer than 2048^2 cells, and 2048^2 * 14 * 64 = 3 758 096 384 < 2^32.  A goal that is blocked or outside the grid
 *     is TBNAV_ERR_INVALID_ARG, and the last solution stays.
 * G5. Field for the controller.  cap finite and > 0; with the handle's resolution, all in fp64 without contraction,
 *       t = ((double)d * resolution) / 10.0;  v = (float)(t < cap ? t : cap);  v = (float)cap where d == TBNAV_NAV_UNREACHED.
 *     Metres to go, capped; every value is finite by construction.
 * G6. Path from a start cell.  A start outside the grid is TBNAV_ERR_INVALID_ARG; a blocked or unreached start is
 *     TBNAV_ERR_UNSUPPORTED.  Otherwise step to the allowed neighbour b with the least d[b] + w*cost[b], ties to the first in G3's
 *     order, and stop at the goal.  By G4 that minimum equals d[a], so d falls strictly and the walk ends.  Output
 *     int32_t cells[n][2] = (ix, iy), start and goal included.  A buffer too small is TBNAV_ERR_INVALID_ARG with *n set to the
 *     length needed.  A host loop over the downloaded d; not a kernel.  (The host copy of the solved grid it walks over is, after a
 *     grid set on the device, fetched at the first path and not at the set.)
 *
 * The solver (csrc/nav.hip).  A workgroup takes one 32 x 32 tile with a one-cell halo into LDS (one halo cell is enough for G3:
 * both orthogonal cells of any diagonal move out of the interior lie inside it), relaxes there until nothing in the tile changes
 * (every thread owns its cells and only ever lowers them: min is monotone and the fixed point unique, so stale reads of a
 * neighbour are harmless and d needs no atomics), writes the interior back and, if a value on its rim changed, marks the up to
 * eight neighbouring tiles active for the next round.  A round is one launch over the active tiles; no workgroup waits for another
 * inside a launch, every loop in the kernel is bounded by the tile size, and a tile that runs into its sweep bound stays active.
 * The host enqueues rounds in batches, reads one small record per batch of how much each round changed, and stops at the first
 * round that changed nothing — the proof of the fixed point.  Every solve starts from d = UNREACHED but for the goal, with the tiles
 * active that see the goal in their interior or halo.
 *
 * G7. Inflation tables (tbnav_nav_inflation_tables; pure host arithmetic, fp64 without contraction).  d(c) = sqrt((double)c) * resolution
 *     is the distance of a cell whose nearest occupied cell lies at squared cell distance c — the expression tbnav_rbpf_get_occ_dist uses.
 *       cost[c]  = 0 where d <= r_robot, else 1 + rint(k*t*t), t = (r_inflate - d) / (r_inflate - r_robot) clamped to 0 .. 1
 *                  (planner::navCostFromDistance / rtn_amd.nav.nav_cost_from_distance);
 *       field[c] = 1 where d <= r_robot, 0 where d >= r_inflate, else (float)(t*t)
 *                  (controller::costFieldFromDistance / rtn_amd.mppi.cost_field_from_distance).
 *     Reach R = (int)ceil(r_inflate / resolution) + 1; the tables hold the entries c = 0 .. R*R and, behind them at index R*R + 1, the
 *     OPEN VALUE: that of d = 10.0, the filter's max_occ_dist, which a cell with nothing occupied within R takes — cost 1, field 0.
 *     Past R the formulas have reached those values already (d > r_inflate), and the filter's own radius, ceil(10 / resolution), is
 *     never the smaller one: for r_inflate <= 10.0 the table form equals, with ==, the host route over the filter's distance field.
 *     0 <= r_robot < r_inflate <= 10.0, 0 <= k <= 63 and resolution > 0, all finite, else TBNAV_ERR_INVALID_ARG;
 *     R > TBNAV_NAV_MAX_REACH (one tile of halo) is TBNAV_ERR_UNSUPPORTED.
 * G8. Cost grid from a particle (tbnav_nav_set_cost_from_rbpf).  A cell is OCCUPIED when its bit in the particle's tiles is set
 *     (probability >= 0.90; tbnav_rbpf.h), whatever distance-field mode the filter runs in: the bits are the source, not a stored field.
 *     c(cell) = the exact minimum of di^2 + dj^2 over occupied cells with |di|, |dj| <= R; the cell's value is table[c] where
 *     c <= R*R, the open value otherwise.  Unknown cells are free, as on the host route.  The nav handle's grid must be the
 *     filter's: nx == ny == the filter's side, and xmin, ymin, resolution equal as doubles — else TBNAV_ERR_INVALID_ARG, as is a
 *     particle that is neither a slot of the filter nor TBNAV_NAV_BEST_PARTICLE.  Handles on different devices:
 *     TBNAV_ERR_UNSUPPORTED.  Anything rejected changes nothing.  The filter's stored distance field is neither read nor allocated.
 * G9. Ordering.  The kernel is enqueued on the filter handle's stream, behind whatever that handle has in flight, and the call returns
 *     when the grid is in place.  Solves are synchronous, as before.
 *
 * The kernel (csrc/nav_from_map.hip, nav_cost_from_occ<OUT>, OUT = uint8_t for the cost grid and float for an MPPI cost field).  One
 * workgroup per 32 x 32 output tile stages the occupancy rows of its 3 x 3 tile neighbourhood, read through the particle's tile table,
 * as 96 rows x 3 u32 in LDS (tile id 0 and tiles outside the map are empty; a ragged last tile is cut at the map's side).  A
 * neighbourhood without a bit writes the open value and leaves.  Otherwise a thread takes, for its cell, the rows at distance
 * 0, 1, .. R either side, finds the nearest set bit left and right of its column with clz / ffs, keeps min(dr^2 + dc^2) and stops at
 * the first dr with dr^2 >= that minimum; then one look into the table, held in LDS.  Integers only, no atomics, no waiting.
 *
 * Not thread-safe; one handle per planner object; the handle owns all device memory.  Bad arguments return before any device call.
 */
#ifndef TBNAV_NAV_H
#define TBNAV_NAV_H

#include <stdint.h>
#include "tbnav_mppi.h"
#include "tbnav_rbpf.h"
#include "tbnav_status.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBNAV_NAV_MAX_SIDE 2048 /* BASELINE configs[4] is 2000 x 2000 */
#define TBNAV_NAV_MAX_COST 64
#define TBNAV_NAV_UNREACHED 0xFFFFFFFFu
#define TBNAV_NAV_MAX_REACH 32 /* G7's R: one tile of halo round a workgroup's tile */
#define TBNAV_NAV_BEST_PARTICLE (-1)

typedef struct tbnav_nav_params {
  int32_t nx, ny;     /* cells along x (slow index) and y, each 2 .. TBNAV_NAV_MAX_SIDE */
  double xmin, ymin;  /* world coordinates of the outer corner of cell (0, 0) */
  double resolution;  /* cell side, > 0 */
  int32_t device;     /* HIP device ordinal, -1 = current device */
  int32_t reserved;
} tbnav_nav_params;

typedef struct tbnav_nav tbnav_nav; /* opaque */

/* What the last successful solve took (tbnav_nav_last_solve). */
typedef struct tbnav_nav_solve_info {
  int32_t solved;       /* 1 once a solve has succeeded on this handle                                             */
  int32_t goal[2];      /* its goal cell                                                                            */
  int32_t rounds;       /* rounds up to and including the first that changed nothing                                */
  int32_t launches;     /* launches of the relaxation kernel (rounds are enqueued in batches: >= rounds)            */
  int32_t tiles[2];     /* tiles along x and y                                                                      */
  int64_t tile_visits;  /* workgroups that found their tile active and relaxed it, over all rounds                  */
} tbnav_nav_solve_info;

/* G1.  Without a GPU: TBNAV_ERR_NO_DEVICE, as everywhere else.  No cost grid is set yet: tbnav_nav_solve is
 * TBNAV_ERR_INVALID_ARG until tbnav_nav_set_cost has succeeded once. */
int tbnav_nav_create(const tbnav_nav_params* params, tbnav_nav** out);
void tbnav_nav_destroy(tbnav_nav* h);

/* G2.  The grid is copied; it is what the NEXT solve uses.  The last solution (cost-to-go, field, path) stays as it is. */
int tbnav_nav_set_cost(tbnav_nav* h, const uint8_t* cost_host);
/* The grid the next solve uses, however it was set (nx*ny values); TBNAV_ERR_INVALID_ARG while none is set. */
int tbnav_nav_get_cost(tbnav_nav* h, uint8_t* cost_host);

/* G7, no device needed.  *n = R*R + 1, the number of table entries, and *reach = R (either may be null).  cost and field (either may
 * be null) receive *n entries FOLLOWED BY the open value, so each needs room for *n + 1 values; cap, the room each has, too small:
 * TBNAV_ERR_INVALID_ARG with *n set. */
int tbnav_nav_inflation_tables(double resolution, double r_robot, double r_inflate, double k, uint8_t* cost, float* field, int32_t cap,
                               int32_t* n, int32_t* reach);
/* G8-G9.  particle: a slot of the filter handle, or TBNAV_NAV_BEST_PARTICLE — the arg-max of the weights found on the device (strict >,
 * the first wins: tbnav_rbpf_best_state's rule), with no host round trip for the index.  Replaces the grid like tbnav_nav_set_cost; the
 * last solution stays as it is. */
int tbnav_nav_set_cost_from_rbpf(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, double r_robot, double r_inflate, double k);
/* Measurement hook (tools/nav_from_map_time.py): tbnav_nav_set_cost_from_rbpf with the kernel launched `launches` >= 1 times in a row
 * between two events on the filter's stream (where the best particle is asked for, its arg-max with each); *kernel_ms = the
 * events' interval / launches.  The grid is the same as after one launch. */
int tbnav_nav_profile_cost_from_rbpf(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, double r_robot, double r_inflate, double k, int32_t launches,
                                     float* kernel_ms);
/* The same search with the float table, installed as the MPPI handle's cost field — geometry the filter's, weight the call's — through
 * the setters tbnav_nav_apply_to_mppi uses: bit for bit tbnav_mppi_set_cost_field of the host route's array
 * (cost_field_from_distance of tbnav_rbpf_get_occ_dist).  Rejections as in G7 (k does not enter) and G8; a field set earlier stays. */
int tbnav_mppi_set_cost_field_from_rbpf(tbnav_mppi* mppi, tbnav_rbpf* pf, int32_t particle, double r_robot, double r_inflate, double weight);
/* The kernel tbnav_nav_set_cost_from_rbpf launched, spelled as a profiler prints it; "" until that route has run on this handle. */
int tbnav_nav_last_cost_kernel(const tbnav_nav* h, char* kernel, int32_t kernel_cap);

/* G3-G4, synchronous.  Solving again on the same handle resets what the last solve left (another goal, a changed cost grid). */
int tbnav_nav_solve(tbnav_nav* h, int32_t goal_ix, int32_t goal_iy);
/* G1's cell of a world position. */
int tbnav_nav_cell_of(const tbnav_nav* h, double x, double y, int32_t* ix, int32_t* iy);

/* The results below are TBNAV_ERR_INVALID_ARG before the first successful solve. */
int tbnav_nav_get_cost_to_go(tbnav_nav* h, uint32_t* d_host);   /* G4, nx*ny values */
int tbnav_nav_get_field(tbnav_nav* h, double cap, float* out);  /* G5, formed on the device, nx*ny values */
/* G6.  cells: room for cells_cap pairs (may be null when cells_cap is 0: *n is then the length needed). */
int tbnav_nav_path(tbnav_nav* h, int32_t start_ix, int32_t start_iy, int32_t* cells, int32_t cells_cap, int32_t* n);

/* info, and the relaxation kernel's name spelled as a profiler prints it ("nav_relax_tiles"; empty before the first solve), as
 * tbnav_mppi_last_kernel_names does.  Either output may be null. */
int tbnav_nav_last_solve(const tbnav_nav* h, tbnav_nav_solve_info* info, char* kernel, int32_t kernel_cap);

/* Hand-over without a host round trip: forms G5 on the nav handle's device and installs it as the MPPI handle's cost field —
 * geometry the nav handle's, weight the call's — by a device-to-device copy when both handles are on one device (a peer copy
 * otherwise).  The result equals, bit for bit, tbnav_mppi_set_cost_field called with the array tbnav_nav_get_field returns.  As
 * tbnav_mppi.h F5 demands, it waits for the MPPI handle's device first, and no graph of ticks captured earlier is replayed.  F1's
 * finiteness holds by construction (G5).  Anything rejected changes nothing: a field set earlier stays in force. */
int tbnav_nav_apply_to_mppi(tbnav_nav* h, tbnav_mppi* mppi, double cap, double weight);
/* Every member of the group receives the field, or none does. */
int tbnav_nav_apply_to_mppi_group(tbnav_nav* h, tbnav_mppi_group* group, double cap, double weight);

#ifdef __cplusplus
}
#endif
#endif /* TBNAV_NAV_H */
