// What the step driver DECIDES on the host between its launches: the widths of a slab's ghost layer, how many tiles a search reaches, the
// first batch of the level propagation, the pacing of a solve, and whether the build queued ahead is adopted, planned, fused, or a slab's
// sort runs as a merge.  Pure host arithmetic over values and small PODs, no HIP and no sph_ctx: tests/host/step_plan_check.cpp compiles
// this header with plain g++ and tests/test_step_plan_host.py holds the expected answers.  (The grids themselves: sph_grid_plan.hpp.)
// All arithmetic is f32 / int in exactly this order.  `range_k` is level_estimation_range / ETA (simulation.rs:2036) throughout.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sph_grid_plan.hpp"

// ---- ghost layer of a slab, in smoothing lengths of the largest particle ---------------------------------------------------------------
// Level estimation AFTER advection looks for neighbours at the advected positions among the ghosts selected BEFORE the step: the layer
// is widened by twice the largest displacement the step may produce -- 4 x the previous step's (all-reduced) largest displacement, at
// least 2 h_max -- and the step checks afterwards that it sufficed.
inline float slab_slack_k(bool level_on, bool after, bool multi, float last_dmax, float h_max_step)
{
    return (level_on && after && multi) ? fmaxf(2.f, h_max_step > 0.f ? 4.f * last_dmax / h_max_step : 0.f) : 0.f;
}
// two rings of one support radius (2 h_max each), or the extended range of the level estimation
inline float halo_base_k(bool level_on, float range_k) { return fmaxf(4.f, level_on ? range_k : 0.f); }

// ---- tiles a search reaches (multi-resolution scenes; tile side >= 2 h_max) ------------------------------------------------------------
// the extended-range lists reach range_k * h_max with range_k > 2: a larger particle may sit ceil(range_k / 2) tiles away
inline int ext_tile_reach(bool want_ext, float range_k) { return want_ext ? (int)ceilf(fmaxf(range_k, 2.f) * 0.5f) : 1; }
// lists of the advected positions from the cells of the pre-step ones: a neighbour may now sit ceil((k h_max + slack) / tile side) tiles away
inline int slack_tile_reach(float k, float h_max, float slack, int tile_ts, float cs)
{
    const float tile_side = (float)tile_ts * cs;
    const int d = (int)ceilf((k * h_max + slack) / tile_side);
    return d < 1 ? 1 : d;
}

// ---- level propagation, one context: the first batch is as long as the previous step's propagation + 1 -- the fluid's depth hardly
// changes from step to step -- so a step usually waits once instead of once per 8 sweeps (`batch8`: measurement aid, always 8)
inline int level_first_batch(uint32_t last_level_sweeps, bool batch8)
{
    if (batch8) return 8;
    const uint32_t b = last_level_sweeps + 1u;
    return (int)(b < 8u ? 8u : b > 1000u ? 1000u : b);
}

// ---- pacing of a solve (sph_step.hip: solve_paced) -------------------------------------------------------------------------------------
// Small scenes: an iteration of n particles takes ~46 us x n / 2^20 on the device, the host's answer to a decision ~10-20 us: the
// lead grows as the sweeps shrink (1 from ~0.45M particles up), and the unpaced head is the smaller of the last two counts; large
// scenes queue nothing unpaced (measured on configs[1]'s driver window: 1.148 ms/step, against 1.164 with the head and 1.201-1.207
// with the predicted queue; profiles/r3_variants.md section 5).  SPH_PACE_LEAD / SPH_PACE_PRED override both.
inline uint32_t pace_lead(uint32_t n, int opt_lead)
{
    if (opt_lead > 0) return (uint32_t)opt_lead;
    const uint32_t per = (450000u + n - 1u) / (n > 1u ? n : 1u);
    return per < 1u ? 1u : per > 8u ? 8u : per;
}
inline uint32_t pace_prediction(uint32_t n, int opt_pred, uint32_t last, uint32_t prev)
{
    // 0: nothing unpaced; 1: min of the last two counts; 2: the last count; 0xffff: by particle count
    const int md = opt_pred == 0xffff ? (n >= 450000u ? 0 : 1) : opt_pred;
    if (md == 0) return 2u;
    if (md == 2 || prev == 0u) return last;
    return last < prev ? last : prev;
}
// the predicted queue fell short at iteration k: a quarter more iterations per wait, at least one -- a skipped iteration costs two
// empty launches (~9 us), a wait the round trip to the host
// (measured on the driver window, 5 runs each: k/4 1.279-1.295 ms per step, k/2 1.284-1.292, k 1.300-1.311)
inline uint32_t solve_extend_upto(uint32_t k) { return k + (k / 4u > 1u ? k / 4u : 1u); }
// HybridDFSPH's two solves are chained only while the divergence solve's iteration count repeats from step to step
// (SPH_CHAIN=1: always, =0: never, negative: by the counts)
inline bool chain_wanted(int opt_chain, uint32_t last_div, uint32_t prev_div) { return opt_chain >= 0 ? opt_chain == 1 : last_div == prev_div; }

// ---- the build queued ahead ------------------------------------------------------------------------------------------------------------
struct AheadBuild {   // the build queued while sph_ctx::ahead_valid
    GridP g{};
    float h_max = 0.f, h_min = 0.f, rest_density = 0.f;
    int tile_ts = 0, tile_tsx = 0, tile_tsy = 0;   // multi-resolution scenes: the tiles of the predicted grid
    uint64_t n = 0;
    bool xv_rec = false;   // its place launch left {x, y, v} in xvn (the step that adopts it may run OpFuseU; gone with ahead_valid)
};
// what the step that may adopt it knows once its own grids are planned
struct StepBuild {
    bool ahead_usable;   // one context, and the header the previous step left behind was still the one in force
    bool ahead_valid, dist_on, exact, uniform_h;
    uint64_t ctx_n;      // particles of the context
    uint32_t n;          // particles in the step's arrays
    float h_max, h_min, rest_density;
    int tile_ts;
    GridP g;             // the grid the step sorts by
};
// Adopted if nothing touched the state since, the scene is what it predicted and the real bounding box fits its grid.
// (A multi-resolution scene: the same smoothing lengths, hence the same cell size and tile side; its tiles then lie on the predicted
//  grid -- another tiling bounds the neighbours' h as well, and the visiting order of a list does not depend on the stencil width it was
//  gathered with.)
inline bool adopt_ahead_build(const AheadBuild& a, const StepBuild& s)
{
    const GridP &ag = a.g, &g = s.g;
    return s.ahead_usable && s.ahead_valid && !s.dist_on && a.n == s.ctx_n && s.n == (uint32_t)s.ctx_n && a.h_max == s.h_max && a.h_min == s.h_min &&
           a.rest_density == s.rest_density && (s.uniform_h ? s.tile_ts == 0 : s.tile_ts > 0) && a.tile_ts == s.tile_ts && !s.exact && ag.cs == g.cs &&
           g.minx >= ag.minx && g.miny >= ag.miny && g.minx + g.sx <= ag.minx + ag.sx && g.miny + g.sy <= ag.miny + ag.sy;
}
// May this step queue the next one's build?  One context, paced solves (the tail is queued once the stop decision was seen),
// mass-derived smoothing lengths; uniform scenes, and multi-resolution scenes sorted by their fine grid (tile_ts > 0) -- a narrow h
// distribution on the coarse grid (FromDistribution*) is excluded with h_from_mass.
struct AheadWish {
    bool multi, paced, opt_ahead_build, h_from_mass, constrain_neighborhood_count, uniform_h, exact;
    int tile_ts;
    uint32_t n;
};
inline bool ahead_build_eligible(const AheadWish& w)
{
    return !(w.multi || !w.paced || !w.opt_ahead_build || !w.h_from_mass || w.constrain_neighborhood_count || (!w.uniform_h && w.tile_ts <= 0) ||
             (w.uniform_h && w.tile_ts != 0) || w.exact || w.n == 0);
}
// Fused (the default): the merge right behind the tail that classifies for it -- every step without the level estimation, whose build
// waits for the smoothing -- takes the tail's header reduction into its count launch
inline bool ahead_build_fused(bool opt_boundary_fused, bool level_on, bool hdr_partials) { return opt_boundary_fused && !level_on && hdr_partials; }

// ---- a slab rank's sort behind its fused refresh as a merge ----------------------------------------------------------------------------
// Slots [0, n_prev) are last step's sorted array (some of them left the rank), the arrivals follow unsorted: the stable sort is the merge
// of sph_sort.hip (incremental_cell_sort_perm) with the arrivals as movers, if they and the particles that changed cell last time are few.
struct SlabSort {
    bool pre;   // the rank's arrays are the ones its fused refresh left
    int inc_sort;
    bool prev_valid;   // the grid of the last build, if nothing touched the state since
    float prev_cs;
    uint32_t prev_ncells;
    float cs;   // this step's sorting grid
    uint32_t ncells, n_prev, n_sort;
    bool exact, count_valid;
    uint32_t movers;   // the last count the device reported
};
inline bool slab_merge_admitted(const SlabSort& s, int& streak)
{
    const bool merge = s.pre && s.inc_sort && s.prev_valid && s.prev_cs == s.cs && s.prev_ncells > 0 && s.n_prev > 0 && s.n_prev <= s.n_sort && !s.exact &&
                       inc_sort_fits(s.ncells, s.n_sort);
    if (!merge) return false;
    // (the arrivals are movers of THIS build, whatever the last count was: too many of them do not touch the streak)
    const uint32_t limit = inc_sort_mover_limit(s.n_sort, s.inc_sort);
    return s.n_sort - s.n_prev <= limit && inc_sort_worthwhile(s.count_valid, s.movers, limit, streak);
}
