// nav_tiles.hpp — what the planner's kernels share: the 32 x 32 tile and its constants, the particle of a filter whose map a kernel
// reads (ParticleRef), and the one body of a tiled fixed-point iteration (tile_fixed_point), which nav_relax_tiles (nav.hip: min-plus
// over G3's moves) and nav_frontier_label (nav_frontier.hip: min over the 3 x 3 cells) each call with a rule of their own.  The host
// side of the rounds is nav_host.hpp's run_rounds.
#ifndef TBNAV_NAV_TILES_HPP
#define TBNAV_NAV_TILES_HPP
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rbpf_device.hpp"
#include "tbnav_nav.h"

namespace tbnav_nk {

constexpr int kTile = 32;                 // cells per tile side
constexpr int kHalo = kTile + 2;          // ... with the one-cell halo (G3: both orthogonal cells of a diagonal move out of the interior lie inside it)
constexpr int kThreads = 256;             // four waves; a wave's 64 lanes are two rows of 32 consecutive iy: no LDS bank is hit twice by a half, and one ballot is two row words
constexpr int kOwn = kTile * kTile / kThreads;   // cells a thread owns: rows (tid >> 5) + 8 j
constexpr int kRowStep = kThreads / kTile;
// Sweeps per visit.  A front crosses an open tile in at most kTile sweeps along an axis and kTile along the diagonal, so 4 * kTile
// leaves a tile of open space or plain walls converged in one visit; a labyrinth inside one tile (a path of up to kTile^2 cells)
// runs into the bound, writes back what it has and stays active for the next round.
constexpr int kMaxSweeps = 4 * kTile;
constexpr unsigned kInf = TBNAV_NAV_UNREACHED;   // no cost-to-go, no label: the largest value there is
// bits of a tile's wake word: 0..8 the tile at (dx + 1) * 3 + (dy + 1) — 4 is the tile itself —, 9: something in the tile changed
constexpr int kSelfBit = 4, kChangedBit = 9;
static_assert(kTile == tbnav_rk::kTS, "a workgroup's tile is a tile of the filter's pool");

// The particle of a filter whose map a kernel reads (nav_cost_from_occ, nav_frontier_mark); the host fills it: nav_host.hpp, particle_ref
struct ParticleRef {
  const unsigned int* table;   // [N][TT] the particles' tile tables
  const int* best;             // where the particle's index is on the device (rbpf_argmax), or null: `particle`
  int particle;
  int TW, TT;                  // tiles per side, per map
  int side;                    // cells per side of the map and of the nav grid (G8)
};
// the particle's tile ids (by value: behind a reference or as a member nav_frontier_mark compiles to other code than it did spelled out)
__device__ __forceinline__ const unsigned int* particle_row(ParticleRef r) { return r.table + (size_t)(r.best ? *r.best : r.particle) * r.TT; }

struct TileArgs {
  unsigned* v;           // [nx][ny] the values: cost-to-go, or labels
  unsigned* cur;         // [tiles_x][tiles_y] 1 = active this round (cleared by the workgroup that takes the tile)
  unsigned* nxt;         // ... next round (all zero when this round starts)
  unsigned* rec;         // this round's record: [0] tiles visited, [1] tiles in which something changed
  int nx, ny, tiles_y;
};

// One visit of one workgroup (kThreads threads, blockIdx = (tile_y, tile_x)) to its tile, if the tile is active: the values of the
// tile and its halo into s_v[kHalo * kHalo], every owned cell lowered to the least candidate of its rule until a sweep lowers nothing
// or kMaxSweeps are done, the cells that changed back to a.v, and the tiles that have to look again flagged in a.nxt.  The rule:
//   stage(i, in, g)        what else is staged for LDS cell i (grid cell g, or outside the grid: !in), before the barrier
//   Cell, prepare(c, o)    what a thread keeps for the owned cell at LDS cell c, formed after the barrier
//   idle(mine)             a cell holding `mine` takes no part
//   lower(o, c, best, s_v) the least of `best` and the candidates of that cell
// (The rule and the arguments come by value and the cells are an array of their own: held in one object with a price array that is
// indexed in a loop, the rule's pointers stay in memory until the loops are unrolled, and nav_relax_tiles gets 130 more instructions.)
template <class Rule>
__device__ __forceinline__ void tile_fixed_point(TileArgs a, unsigned* s_v, unsigned* s_wake, Rule rule) {
  const int tile_x = blockIdx.y, tile_y = blockIdx.x, tile = tile_x * a.tiles_y + tile_y;
  if (a.cur[tile] == 0) return;   // (the whole workgroup alike)
  const int tid = threadIdx.x;
  const int x0 = tile_x * kTile - 1, y0 = tile_y * kTile - 1;   // the grid cell of LDS cell (0, 0)
  for (int i = tid; i < kHalo * kHalo; i += kThreads) {
    const int lx = i / kHalo, ly = i - lx * kHalo, gx = x0 + lx, gy = y0 + ly;
    const bool in = gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny;   // outside the grid: blocked (G3), no label
    const int g = gx * a.ny + gy;
    rule.stage(i, in, g);
    s_v[i] = in ? a.v[g] : kInf;
  }
  if (tid == 0) *s_wake = 0;
  __syncthreads();

  const int c0 = (1 + (tid >> 5)) * kHalo + 1 + (tid & 31);
  typename Rule::Cell own[kOwn];
  unsigned mine[kOwn], first[kOwn];
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int c = c0 + j * kRowStep * kHalo;
    rule.prepare(c, own[j]);
    first[j] = mine[j] = s_v[c];
  }

  // Sweep until nothing is lowered.  A thread writes its own cells only and only lowers them, so whether a neighbour's value is read
  // before or after its owner's write of this sweep does not matter: min is monotone and the fixed point is unique (the cost-to-go of
  // G4; every cell of a component holding the component's least index, G12), and no atomics are needed on the values.
  int more = 1;
  for (int s = 0; s < kMaxSweeps && more; ++s) {
    int changed = 0;
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      if (rule.idle(mine[j])) continue;
      const int c = c0 + j * kRowStep * kHalo;
      const unsigned best = rule.lower(own[j], c, mine[j], s_v);
      if (best < mine[j]) { mine[j] = best; s_v[c] = best; changed = 1; }
    }
    more = __syncthreads_or(changed);
  }

  // the interior back (a cell outside the grid never changes), and who has to look again
  unsigned wake = more ? 1u << kSelfBit : 0u;   // the sweep bound was hit: this tile stays active
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    if (mine[j] != first[j]) {
      const int ix = (tid >> 5) + j * kRowStep, iy = tid & 31;   // 0 .. kTile-1
      a.v[(x0 + 1 + ix) * a.ny + (y0 + 1 + iy)] = mine[j];
      const int ex = ix == 0 ? -1 : (ix == kTile - 1 ? 1 : 0), ey = iy == 0 ? -1 : (iy == kTile - 1 ? 1 : 0);
      wake |= 1u << kChangedBit;
      if (ex != 0) wake |= 1u << ((ex + 1) * 3 + 1);
      if (ey != 0) wake |= 1u << (3 + ey + 1);
      if (ex != 0 && ey != 0) wake |= 1u << ((ex + 1) * 3 + ey + 1);
    }
  }
  if (wake) atomicOr(s_wake, wake);
  __syncthreads();
  const unsigned w = *s_wake;
  if (tid < 9 && ((w >> tid) & 1u)) {
    const int tx = tile_x + tid / 3 - 1, ty = tile_y + tid % 3 - 1;
    if (tx >= 0 && tx < (int)gridDim.y && ty >= 0 && ty < a.tiles_y) a.nxt[tx * a.tiles_y + ty] = 1u;
  }
  if (tid == 0) {
    a.cur[tile] = 0;   // (every wave has read it: two barriers ago)
    atomicAdd(&a.rec[0], 1u);
    if (w >> kSelfBit & 1u || w >> kChangedBit & 1u) atomicAdd(&a.rec[1], 1u);
  }
}

}  // namespace tbnav_nk

#endif
