// What the step driver DECIDES about a neighbour build before it launches anything: the cell grid of a bounding box, the sorting grid
// and tiles of a step, and whether the cell sort may run as a merge.  Pure host arithmetic, no HIP: tests/host/build_plan_check.cpp
// compiles this header with plain g++ and tests/test_build_plan_host.py compares it with tests/neighbour_scenes.py.
// All arithmetic is f32 / int / long long in exactly this order: the grids are part of the bit-exact contract (cell_index).
#pragma once

#include <math.h>
#include <stdint.h>

struct GridP {
    float cs;            // cell size = support radius of the largest particle
    int minx, miny;      // cells_min  (neighborhood_search.rs:273)
    int sx, sy;          // grid size  (cells_max - cells_min)
    uint32_t ncells;
};

struct GridBox {
    float min_x, min_y, max_x, max_y;
};

// CellGrid (neighborhood_search.rs:261-275) of cell size `cs` around `box`: one empty cell on every side of the occupied ones, and
// `margin` more (the grid of a build queued ahead is a prediction).  false: a dimension does not fit 16 bits (cx | cy << 16) or the
// table has 2^27 cells or more -- `out` then holds the cell size only.
inline bool plan_grid(const GridBox& box, float cs, int margin, GridP& out)
{
    out = GridP{};
    out.cs = cs;
    const float lo_x = floorf(box.min_x / cs), lo_y = floorf(box.min_y / cs), hi_x = floorf(box.max_x / cs), hi_y = floorf(box.max_y / cs);
    if (!(fabsf(lo_x) < 2e9f && fabsf(lo_y) < 2e9f && fabsf(hi_x) < 2e9f && fabsf(hi_y) < 2e9f)) return false;   // (the casts below must be defined)
    const int minx = (int)lo_x - 1 - margin, miny = (int)lo_y - 1 - margin;
    const long long sx = (long long)((int)hi_x + 2 + margin) - minx, sy = (long long)((int)hi_y + 2 + margin) - miny;
    if (sx <= 0 || sy <= 0 || sx >= 65536 || sy >= 65536 || sx * sy >= (1ll << 27)) return false;
    out.minx = minx;
    out.miny = miny;
    out.sx = (int)sx;
    out.sy = (int)sy;
    out.ncells = (uint32_t)sx * (uint32_t)sy;
    return true;
}

inline int tiles_across(int cells, int ts) { return (cells + ts - 1) / ts; }   // tiles of ts x ts cells that cover a grid dimension

// The grids of one step.  `coarse` (cell = support radius of the largest particle) is the grid the reference's convention defines;
// uniform scenes sort by it.  Multi-resolution scenes sort by a finer grid (cell = support of the smallest particle, doubled until the
// table fits) and give every particle its own stencil width (TileP, sph_device.h), so a fine particle far from any coarse one still
// looks at 3 x 3 small cells instead of 3 x 3 large ones.  tile_ts = 0: `sort` is `coarse`, every stencil is 3 x 3 cells.
struct SortGridPlan {
    GridP coarse, sort;
    int tile_ts, tile_tsx, tile_tsy;
};
// `empty`: nothing to sort (a slab rank without particles) -- grids of one cell.  false: the coarse grid is too large.
inline bool plan_sorting_grid(const GridBox& box, bool empty, float h_min, float h_max, bool uniform, SortGridPlan& out)
{
    auto grid = [&](float cs, GridP& g) {
        if (!empty) return plan_grid(box, cs, 0, g);
        g = GridP{cs, 0, 0, 1, 1, 1u};
        return true;
    };
    out = SortGridPlan{};
    if (!grid(h_max * 2.f, out.coarse)) return false;
    out.sort = out.coarse;
    // (a narrow h distribution -- FromDistribution* support lengths wander by a few percent -- keeps the one-cell stencil of the coarse
    //  grid: the fine grid only pays once 3 x 3 coarse cells hold several times the needed candidates)
    if (uniform || !(h_max >= 1.75f * h_min)) return true;
    float cs = h_min * 2.f;
    bool ok = false;
    for (int k = 0; k < 24 && cs < out.coarse.cs; k++, cs *= 2.f)
        if ((ok = grid(cs, out.sort))) break;
    if (ok) {
        int ts = (int)ceilf(out.coarse.cs / out.sort.cs);
        while ((float)ts * out.sort.cs < out.coarse.cs) ts++;
        out.tile_ts = ts;
    } else {
        out.sort = out.coarse;   // the finest grid that fits is the coarse one: a one-cell tile, 3 x 3 stencils
        out.tile_ts = 1;
    }
    out.tile_tsx = tiles_across(out.sort.sx, out.tile_ts);
    out.tile_tsy = tiles_across(out.sort.sy, out.tile_ts);
    return true;
}

// ---- may the cell sort run as a merge (sph_sort.hip: incremental_cell_sort_*)? ---------------------------------------------------------
// Its scan adds up the preceding block sums per block (k_inc_scan): quadratic in ncells / 1024 -- a grid much sparser than one cell per
// particle takes the radix sort.
inline bool inc_sort_fits(uint32_t ncells, uint32_t n) { return ncells <= n + 4096u; }
// Its cost grows with the particles that change cell: above this many the radix sort is the cheaper one (Options::inc_sort > 1: the divisor)
inline uint32_t inc_sort_mover_limit(uint32_t n, int inc_sort) { return n / (inc_sort > 1 ? (uint32_t)inc_sort : 3u); }
// ... judged by the last count the device reported (a build or two old; `count_valid`: one was reported since the state was replaced).
// While it is above the limit the builds take the radix sort and `streak` counts them; every eighth one probes the merge again.  A small
// count leaves the streak alone.
inline bool inc_sort_worthwhile(bool count_valid, uint32_t movers, uint32_t limit, int& streak)
{
    if (!count_valid || movers <= limit) return true;
    if (++streak < 8) return false;
    streak = 0;
    return true;
}
