/* tbnav_nav.h — C-ABI of the GOAL FIELD: the exact shortest-path cost-to-go to a goal cell over a cost grid, solved on the MI355X
 * and handed to the MPPI handle device to device (an OPTION; nothing changes for a handle that does not use it).
 *
 * The reference has a package for this job — planner/: a grid map with inflation (planner/src/planner/grid_map.cpp) and D* Lite
 * over the 8-connected grid (planner/src/planner/dstar_light.cpp:367-461: the eight actions at :370-373, a move priced by the cell
 * it enters, 1 or sqrt(2) cells or an occupied-cell cost, at :444-461) — but its controller never sees it: MPPI's pull towards the
 * waypoint is the quadratic distance (controller/include/controller/mppi.hpp:87-105), which points straight through whatever
 * stands in the way.  A cost field (tbnav_mppi.h, COST FIELD) that holds METRES TO GO ROUND THE WALLS instead pulls the rollouts
 * out of a pocket.  Not built: D* Lite's incremental repair (every solve starts afresh), heading-dependent costs.
 *
 * This section is the whole specification; tests/nav_restatement.py restates G1-G6 in Python integers, tests/nav_from_map_restatement.py G7-G8,
 * tests/nav_frontier_restatement.py G10-G16, tests/nav_gain_restatement.py G17-G20.
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
 * EXPLORATION FRONTIERS AS GOALS (csrc/nav_frontier.hip; an option like everything here).  A robot that is building its map has a source
 * of goals of its own: the border between what it has seen to be free and what it has not seen at all.  Everything below is integer or
 * order-free, so the tests' bar stays ==.
 *
 * G10. Classes.  A cell of a particle's map is UNKNOWN or FREE exactly where GridMapper::gridMap (tbnav_rbpf_particle_map) exports -1 or
 *     0, by the cuts the filter handle holds for that export: UNKNOWN where half_lo <= l <= half_hi (probability exactly 0.5), FREE where
 *     l <= free_cut (probability <= 0.35).  A tile nobody has written (table id 0) is unknown throughout; a cell outside the map is
 *     neither.  The nav grid's cell (ix, iy) is the filter's cell (ci, cj) = (ix, iy), as in G8; the exported int8 map is that grid
 *     TRANSPOSED.
 * G11. Frontier cell: FREE, and passable (cost != 0 in the grid the next solve would use, however that grid was set), and not visited
 *     (G14), and at least one of its FOUR edge neighbours inside the grid is UNKNOWN.  Four and not eight: the mapper's walls are only
 *     8-connected, and a diagonal look leaks through them.
 * G12. Clusters.  A cluster is an 8-connected component of frontier cells (no corner rule: this is connectivity of a set, not a move).
 *     A cell's label is the least index ix*ny + iy in its component; a cell that is no frontier cell has the label TBNAV_NAV_UNREACHED.
 *     A cluster's size is its number of cells.
 * G13. Seeds.  A seed is any cell of a cluster of size >= min_cells; min_cells >= 1, anything else is TBNAV_ERR_INVALID_ARG.
 *     tbnav_nav_find_frontiers runs G10-G13 for a slot of the filter or TBNAV_NAV_BEST_PARTICLE.  Grid and device must match as in G8,
 *     with G8's rejections, and TBNAV_ERR_INVALID_ARG while no cost grid is set.  It is enqueued on the filter's stream (G9) and returns
 *     when done.  Anything rejected changes nothing.
 * G14. Visited mask.  One bit per cell, owned by the handle, empty at create.  tbnav_nav_mark_visited adds the disc
 *     dix^2 + diy^2 <= radius^2 round (ix, iy), cut at the grid; 0 <= radius <= TBNAV_NAV_MAX_VISIT_RADIUS and a centre inside the grid,
 *     else TBNAV_ERR_INVALID_ARG.  tbnav_nav_clear_visited empties it; there is no other way to take a mark back.  The host holds the
 *     mask and uploads it when it changed: marking is not a kernel.  Why it is part of this and not left to the caller: the reference's
 *     mapper drops a beam without a return (sensor_model.cpp:43-112), so standing on a frontier does not clear it when the wall behind
 *     it is out of range, and a robot without the mask sits on such a seed for ever.
 * G15. Several goals.  tbnav_nav_solve_goals: d = 0 at every listed cell, G3-G4 otherwise, so d is the cost-to-go to the NEAREST goal.
 *     n >= 1; a cell listed twice is harmless; one blocked or outside cell is TBNAV_ERR_INVALID_ARG and the last solution stays.  With
 *     n = 1 it equals tbnav_nav_solve bit for bit, tbnav_nav_last_solve's info included.  tbnav_nav_solve_frontiers: the same with the
 *     seeds of the last find as goals, taken from the device with no list crossing the host; TBNAV_ERR_UNSUPPORTED when that find left no
 *     seed — nothing left to explore — and the last solution stays; TBNAV_ERR_INVALID_ARG before any find, or when the cost grid or the
 *     visited mask was set again since (every successful set, mark or clear counts, whatever it changed).  Everything that reads a
 *     solution works unchanged (G5, G6, the hand-over); G6's walk stops at the first d == 0, which is the seed reached.
 *     tbnav_nav_solve_info.goal is the first listed goal for solve_goals and (-1, -1) for solve_frontiers.
 * G16. Results for people.  tbnav_nav_get_frontier_labels returns G12; tbnav_nav_frontier_list one record per cluster in ascending label
 *     order — a host loop over the downloaded labels, like G6, not a kernel; a buffer too small is TBNAV_ERR_INVALID_ARG with *n set.
 *     Both are TBNAV_ERR_INVALID_ARG before the first find and keep the last find's results whatever is set afterwards.
 *
 * The kernels.  nav_frontier_mark: one workgroup of 256 per 32 x 32 tile (nav_cost_from_occ's tiling) reads the tile's 1024 log-odds
 * through the particle's tile table (8 KB, rows contiguous) and the facing row or column of its four edge neighbours, classifies them
 * against the cuts passed by value, packs UNKNOWN / FREE / passable into row words with wave ballots (a wave64 is two rows of 32), forms
 * each row's frontier word with shifts and ORs of the unknown words above, below and either side, ANDs in the visited word, writes
 * frontier[nx][TW] (the pool's bm layout), the initial labels (own index or UNREACHED) and zeros for the sizes, and sets the tile's active
 * flag when any bit is set; a tile nobody has written holds no FREE cell, writes zeros and UNREACHED and leaves early; one count per
 * workgroup is its only atomic.  nav_frontier_label: minimum-label propagation over the 8 neighbours in the shape of nav_relax_tiles (an
 * active tile with a one-cell halo in LDS, sweeps to the tile's own fixed point under the same bound, the interior written back, a changed
 * rim wakes the neighbours, a round is a launch, the host stops at the first round that changed nothing).  nav_frontier_sizes: one integer
 * atomicAdd per frontier cell into size[label] — order-free, hence exact.  nav_frontier_seeds: the seed words by ballot, and the counts.
 * nav_reset_goals: a solve's start from the seed words or from an uploaded list, active the tiles that see a goal (nav_reset's rule).  No
 * kernel waits for another workgroup; every loop is bounded by the tile.
 *
 * FRONTIERS RANKED BY WHAT A SCAN FROM THEM WOULD REVEAL (csrc/nav_gain.hip; an option like everything here).  The nearest seed is the
 * crudest choice there is: a gap into a closed pocket of 50 unknown cells beats a doorway into the unexplored half of the building whenever
 * it is a step closer.  Below, every seed cell is a viewpoint, its gain the number of unknown cells a scanner of R cells' range would look
 * at from there, and the solve starts every seed at a handicap that falls with its gain.  Integer rays and a count of distinct cells: the
 * gain is one number whatever order the work is done in, and the bar stays ==.  tests/nav_gain_restatement.py restates G17-G20.
 *
 * G17. Rays (host arithmetic, integers only, no trigonometry).  The range R is in cells, 1 <= R <= TBNAV_NAV_MAX_GAIN_RANGE.  The end
 *     points are the ring E(R) = {(ex, ey) : R*R - R < ex*ex + ey*ey <= R*R + R}, in ascending (ex, ey); no component exceeds R, so a
 *     viewpoint's rays stay inside the (2R+1)^2 window round it.  The ray to (ex, ey) has n = max(|ex|, |ey|) steps; step s = 1 .. n is the
 *     offset (sgn(ex) * ((2*s*|ex| + n) / (2*n)), sgn(ey) * ((2*s*|ey| + n) / (2*n))), integer division: closed form per step, no error
 *     term carried from step to step.  tbnav_nav_gain_rays returns the ring.  (The rays enter about 95 % of the disc's cells; that is
 *     the rule, not a defect to repair.)
 * G18. What a ray sees.  UNKNOWN is G10's class, a tile with id 0 unknown throughout; OCCUPIED is G8's bit.  From the viewpoint v a ray
 *     walks its steps in order and ENDS, without counting the cell, at the first step that leaves the grid, or enters an OCCUPIED cell,
 *     or changes both coordinates while BOTH cells orthogonally between the previous cell and this one are OCCUPIED (G3's reason: the
 *     mapper's walls are only 8-connected; with one of the two occupied the ray goes on — grazing a corner does not block it).  Every
 *     other cell entered is passed through, and is SEEN if it is UNKNOWN.  gain(v) = the number of DISTINCT seen cells over all rays of
 *     E(R).  FREE cells, known cells that are neither, and v itself never count.
 * G19. Find with gain.  tbnav_nav_find_frontiers_gain runs G10-G13 exactly as tbnav_nav_find_frontiers does — results, info, kernels and
 *     rejections the same — and then, in the same call on the filter's stream with nothing of the filter's between the two, gain(v) for
 *     every seed cell of that find from the same particle's map.  A cell that is no seed has gain 0 and is no viewpoint.
 *     tbnav_nav_gain_info.best is the least cell index among those with gain_max, (-1, -1) with no viewpoint; a find that leaves no seed
 *     sets computed = 1 and viewpoints = 0 (gain_min = gain_max = 0), and launches none of the gain's kernels.  The gain belongs to the
 *     find that made it: a later plain tbnav_nav_find_frontiers leaves the handle with NO gain.  range_cells outside
 *     1 .. TBNAV_NAV_MAX_GAIN_RANGE is TBNAV_ERR_INVALID_ARG and changes nothing.  tbnav_nav_get_frontier_gain: uint32 [nx*ny];
 *     tbnav_nav_frontier_gain_list: one record per cluster in ascending label order — root, the cluster's gain_max and the least cell index
 *     with it; a cluster that is no seed gets 0 and (-1, -1) — a host loop over the downloaded arrays, like G16.  Both are
 *     TBNAV_ERR_INVALID_ARG while the handle has no gain.
 * G20. Ranked solve.  tbnav_nav_solve_frontiers_ranked, 0 <= gain_weight <= TBNAV_NAV_MAX_GAIN_WEIGHT: the start is
 *     start[seed] = gain_weight * (gain_max - gain(seed)) at every seed and UNREACHED elsewhere, and the fixed point
 *     d[a] = min(start[a], min over allowed moves a -> b of d[b] + w*cost[b]).  The relaxation only ever lowers values, so it is
 *     nav_relax_tiles unchanged and the fixed point stays unique.  It cannot overflow: a window holds (2*128+1)^2 - 1 = 66048 cells
 *     beside the viewpoint, so a start is at most 4096 * 66048 = 270 532 608, and with G4's bound 3 758 096 384 the sum is
 *     4 028 628 992 < 2^32.  gain_weight = 0, or every gain equal, gives tbnav_nav_solve_frontiers bit for bit.  gain_max reaches the
 *     start kernel on the device; the seed list never crosses the host.  TBNAV_ERR_INVALID_ARG when the handle has no gain, or the cost
 *     grid or the visited mask was set again since the find (G15's rule), or the weight is out of range; TBNAV_ERR_UNSUPPORTED when the
 *     find left no seed; in both cases the last solution stays.  G6 generalised: the walk of a ranked solution stops at the first cell
 *     that is a seed whose d equals its own start value (with all starts 0 that is d == 0; every solve that is not ranked keeps the
 *     d == 0 rule).  tbnav_nav_solve_info.goal is (-1, -1).  G5 and the hand-over are untouched.
 *
 * The kernels (csrc/nav_gain.hip).  nav_gain_classes: one workgroup per tile, nav_frontier_mark's ballots, writes the dense row-word
 * bitmaps unk[nx][TW] and occ[nx][TW] (the columns of a ragged last word past the map's side are set in occ: leaving the grid ends a
 * ray as an occupied cell does, and no cell orthogonally beside a step inside the grid lies outside it).  nav_gain_list: the seed words'
 * bits as a list of cell indices, a slot counter its one atomic; the order is free, the result is indexed by cell.
 * nav_frontier_gain<RMAX>, RMAX = 32 for R <= 32 and 128 above: one workgroup per viewpoint stages the window's rows of both bitmaps,
 * shifted so that bit 0 is the window's first column, into LDS beside a zeroed seen bitmap; lanes take rays, walk them (the quotients of
 * G17 by carrying the remainder — the same integers) and OR bits into the seen bitmap; a popcount gives gain[cell], and one 64-bit
 * atomicMax of (gain << 32 | ~cell) gives gain_max and best at once, another of ~gain gain_min.  nav_reset_ranked: G20's start.  Integers
 * only; no workgroup waits for another; every loop is bounded by R or the tile.
 *
 * G21. Not built here: sharded filters and handles on different devices; gain per heading or field of view; the reference mapper's habit
 * of dropping beams without a return (sensor_model.cpp:43-112), which makes the gain an UPPER bound on what a scan clears; gain at cells
 * that are not seeds; any utility other than the linear one; clearing along beams without a return (the mapper's behaviour stays the
 * reference's); incremental updates between scans; a time-out for marks.
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
#define TBNAV_NAV_MAX_VISIT_RADIUS 64 /* G14, cells */
#define TBNAV_NAV_MAX_GAIN_RANGE 128  /* G17, cells */
#define TBNAV_NAV_MAX_GAIN_WEIGHT 4096 /* G20 */

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

/* What the last find left (G13). */
typedef struct tbnav_nav_frontier_info {
  int32_t found;          /* 1 once a find has succeeded on this handle                                    */
  int32_t min_cells;      /* its threshold                                                                   */
  int32_t cells;          /* frontier cells (G11)                                                            */
  int32_t clusters;       /* clusters (G12)                                                                  */
  int32_t seed_clusters;  /* clusters of size >= min_cells                                                   */
  int32_t seed_cells;     /* their cells: the goals of tbnav_nav_solve_frontiers                             */
  int32_t rounds;         /* the labelling's rounds up to and including the first that changed nothing       */
  int32_t launches;       /* launches of nav_frontier_label (>= rounds)                                      */
  int64_t tile_visits;    /* workgroups that found their tile active, over all rounds                        */
} tbnav_nav_frontier_info;

/* One cluster (G16). */
typedef struct tbnav_nav_frontier {
  int32_t root[2];        /* the cell whose index is the label                                               */
  int32_t size;           /* cells                                                                           */
  int32_t seeds;          /* 1 where size >= the find's min_cells                                            */
  int32_t box[4];         /* ix_min, iy_min, ix_max, iy_max                                                  */
  int64_t sum_ix, sum_iy; /* over the cells: the centroid is (sum_ix / size, sum_iy / size)                  */
} tbnav_nav_frontier;

/* G10-G13.  info may be null. */
int tbnav_nav_find_frontiers(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info);
/* Measurement hook (tools/nav_frontier_time.py): the same find with events on the filter's stream between its stages; stage_ms[4] = mark,
 * the label rounds with the host's reads of their records, sizes, seeds. */
int tbnav_nav_profile_find_frontiers(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info, float* stage_ms);
/* The last find's info (found = 0 before the first). */
int tbnav_nav_last_frontiers(const tbnav_nav* h, tbnav_nav_frontier_info* info);
/* The kernels of a find, spelled as a profiler prints them and separated by ';'; "" before the first find. */
int tbnav_nav_last_frontier_kernels(const tbnav_nav* h, char* kernels, int32_t kernels_cap);
/* G14.  tbnav_nav_get_visited: nx*ny bytes, 1 = visited. */
int tbnav_nav_mark_visited(tbnav_nav* h, int32_t ix, int32_t iy, int32_t radius_cells);
int tbnav_nav_clear_visited(tbnav_nav* h);
int tbnav_nav_get_visited(tbnav_nav* h, uint8_t* visited_host);
/* G15, synchronous like tbnav_nav_solve.  cells: n pairs (ix, iy). */
int tbnav_nav_solve_goals(tbnav_nav* h, const int32_t* cells, int32_t n);
int tbnav_nav_solve_frontiers(tbnav_nav* h);
/* G16.  labels_host: nx*ny values.  out: room for cap records (may be null when cap is 0: *n is then the number needed). */
int tbnav_nav_get_frontier_labels(tbnav_nav* h, uint32_t* labels_host);
int tbnav_nav_frontier_list(tbnav_nav* h, tbnav_nav_frontier* out, int32_t cap, int32_t* n);

/* What the last find with gain left (G19). */
typedef struct tbnav_nav_gain_info {
  int32_t computed;       /* 1 while the handle holds the gain of its last find                              */
  int32_t range_cells;    /* R                                                                               */
  int32_t rays;           /* |E(R)|                                                                          */
  int32_t viewpoints;     /* the find's seed cells                                                           */
  int32_t gain_min;       /* over the viewpoints; 0 with none                                                */
  int32_t gain_max;
  int32_t best[2];        /* the least cell index with gain_max; (-1, -1) with no viewpoint                  */
} tbnav_nav_gain_info;

/* One cluster's gain (G19). */
typedef struct tbnav_nav_frontier_gain {
  int32_t root[2];        /* as in tbnav_nav_frontier                                                        */
  int32_t gain_max;       /* the most over the cluster's cells; 0 where the cluster is no seed               */
  int32_t best[2];        /* the least cell index of the cluster with it; (-1, -1) where it is no seed       */
} tbnav_nav_frontier_gain;

/* G17, no device needed.  *n = |E(R)| (may be null).  ends (may be null) receives *n pairs (ex, ey); cap, the room it has in pairs, too
 * small: TBNAV_ERR_INVALID_ARG with *n set. */
int tbnav_nav_gain_rays(int32_t range_cells, int32_t* ends, int32_t cap, int32_t* n);
/* G19.  info and ginfo may be null. */
int tbnav_nav_find_frontiers_gain(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, int32_t range_cells,
                                  tbnav_nav_frontier_info* info, tbnav_nav_gain_info* ginfo);
/* Measurement hook (tools/nav_gain_time.py): tbnav_nav_profile_find_frontiers with, in stage_ms[4], the gain's kernels together. */
int tbnav_nav_profile_find_frontiers_gain(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, int32_t range_cells,
                                          tbnav_nav_frontier_info* info, tbnav_nav_gain_info* ginfo, float* stage_ms);
/* The handle's gain info (computed = 0 where it has none). */
int tbnav_nav_last_gain(const tbnav_nav* h, tbnav_nav_gain_info* ginfo);
/* The gain's kernels of the last find with gain, spelled as a profiler prints them and separated by ';'; "" where none ran. */
int tbnav_nav_last_gain_kernels(const tbnav_nav* h, char* kernels, int32_t kernels_cap);
/* gain_host: nx*ny values.  out: room for cap records (may be null when cap is 0: *n is then the number needed). */
int tbnav_nav_get_frontier_gain(tbnav_nav* h, uint32_t* gain_host);
int tbnav_nav_frontier_gain_list(tbnav_nav* h, tbnav_nav_frontier_gain* out, int32_t cap, int32_t* n);
/* G20, synchronous like tbnav_nav_solve. */
int tbnav_nav_solve_frontiers_ranked(tbnav_nav* h, int32_t gain_weight);

#ifdef __cplusplus
}
#endif
#endif /* TBNAV_NAV_H */
