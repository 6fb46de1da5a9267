// The index arithmetic of the fused step boundary (sph_sort.hip: k_inc_count<true>, k_inc_place_reorder<false, true>; sph_api.hip:
// k_header_ahead): which partial a lane of the header reduction loads in which trip, how two headers merge, and the two-level form of
// the cell-range table.  Plain C++ behind a host/device macro: tests/host/boundary_fused_check.cpp compiles this header with g++ and
// tests/test_boundary_fused_host.py runs it.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SPH_HD __host__ __device__ __forceinline__
#else
#define SPH_HD inline
#endif

// ---- step header: per-step scalars reduced on the device, read once by the host ---------------
struct HeaderOut {
    float min_x, min_y, max_x, max_y, h_max, h_min, min_cfl;
    uint32_t pad;
};

// The reduction over the integrating tail's partials runs in ONE workgroup of HDR_AHEAD_THREADS lanes: lane t visits, in trip k0 = t,
// t + 4 * HDR_AHEAD_THREADS, ..., the four partials header_ahead_slot(k0, 0 .. 3, nparts), requested together.  A slot beyond the end
// repeats the last partial (a repeated partial changes no minimum or maximum).
#define HDR_AHEAD_THREADS 1024u
SPH_HD uint32_t header_ahead_slot(uint32_t k0, uint32_t u, uint32_t nparts)
{
    const uint32_t k = k0 + HDR_AHEAD_THREADS * u;
    return k < nparts - 1u ? k : nparts - 1u;
}
SPH_HD HeaderOut header_neutral()
{
    const float inf = INFINITY;
    return HeaderOut{inf, inf, -inf, -inf, 0.f, inf, inf, 0u};
}
SPH_HD void header_merge(HeaderOut& o, const HeaderOut& q)
{
    o.min_x = fminf(o.min_x, q.min_x); o.min_y = fminf(o.min_y, q.min_y);
    o.max_x = fmaxf(o.max_x, q.max_x); o.max_y = fmaxf(o.max_y, q.max_y);
    o.h_max = fmaxf(o.h_max, q.h_max); o.h_min = fminf(o.h_min, q.h_min);
    o.min_cfl = fminf(o.min_cfl, q.min_cfl);
}

// ---- the incremental sort's cell-range table in two levels --------------------------------------
// k_inc_count takes INC_CELLS cells per workgroup.  Fused, it leaves local[c] = the populations of the cells of c's workgroup in front
// of c and, as ever, the workgroups' sums; bpre[b] = the sums of all workgroups in front of b (bpre[number of workgroups] = the total)
// is taken behind the launch boundary by whoever needs it (k_inc_place_reorder: every wave in registers, the finishing workgroups for
// their own block): first slot of cell c = local[c] + bpre[c / INC_CELLS].
#define INC_CELLS_LOG2 10
#define INC_CELLS (1 << INC_CELLS_LOG2)
SPH_HD uint32_t inc_cell_first(const uint32_t* local, const uint32_t* bpre, uint32_t c) { return local[c] + bpre[c >> INC_CELLS_LOG2]; }
SPH_HD uint32_t inc_count_blocks(uint32_t ncells) { return (ncells + (uint32_t)INC_CELLS - 1u) >> INC_CELLS_LOG2; }

// ---- a particle's rank among the stayers of its new cell (k_inc_place_reorder) ------------------
// The slot of particle i = first slot of its new cell + the stayers (flag byte 0) of that cell in front of it + the listed movers in
// front of it.  The stayers in front of it are flag bytes [b, e) of the CURRENT order:
//   a stayer: those of its own cell in front of it -- b = the cell's start, e = i;
//   a mover:  all stayers of the cell it enters, old range [b, eb), if it comes from behind that range, none if from in front of it.
SPH_HD uint32_t inc_mover_range_end(uint32_t i, uint32_t b, uint32_t eb) { return i >= eb ? eb : b; }
// A stayer's range ends at itself and the particles of a cell are consecutive, so the part of [b, i) that lies inside the particle's
// wave -- lane l holds particle w0 + l, the particle is lane i - w0 -- is read off the wave's ballot of "is a stayer": the lanes
// [max(b, w0) - w0, i - w0) count.  Only a cell that starts in front of the wave leaves a part outside, the bytes [b, w0), for a loop.
SPH_HD uint64_t inc_rank_ballot_lanes(uint32_t w0, uint32_t b, uint32_t i)
{
    const uint32_t lo = b > w0 ? b - w0 : 0u, hi = i - w0;   // (w0 <= i < w0 + 64, b <= i)
    return ((1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
}
SPH_HD uint32_t inc_rank_outside_end(uint32_t w0, uint32_t b) { return b < w0 ? w0 : b; }   // the loop's range is [b, this): empty unless b < w0
