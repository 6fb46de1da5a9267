// Internal host-side interface between the translation units of libsph_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "sph_device.h"
#include "sph_ffi.h"

// ---- HIP-event profiler (measurement hook; sph_profile_* in the C ABI) ------------------------
struct Profiler {
    int mode = 0;  // 0 off, 1 every kernel, 2 only names starting with "density" (sampled: every 8th step),
                   // 3 (diagnostic) the SWEEPS only, stamped on the device's own clock: the first blocks stamp the constant 100 MHz
                   //   counter at their start, every block at its end, into the launch's slot of a ring (atomic min / max).  The stamps'
                   //   same-address atomics make a sweep ~30 us longer, so this mode does not TIME a sweep; it places the dispatch: first
                   //   wave 3 us behind rocprofv3's start, last wave 0.8 us before its end (profiles/r4_event_calibration.md)
                   // 4 every kernel like mode 1, but a scope that holds ONE sweep launch is timed by that dispatch's own start / end
                   //   timestamps (hipExtLaunchKernelGGL's start / stop events: the completion signal's, what rocprofv3 --kernel-trace
                   //   reports) instead of a marker bracket around it -- no marker excess to calibrate away (bench.py's roofline figures)
    uint64_t step_index = 0;
    struct Rec {
        std::string name;
        uint64_t launches = 0;
        double total_ms = 0;
        std::vector<float> samples;   // per-launch ms
    };
    struct Pending {
        int rec;
        hipEvent_t a, b;
        int slot;   // >= 0: device timestamps in ts_dev[slot] / ts_dev[TS_RING + slot] instead of events
    };
    std::vector<Rec> recs;
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;

    int find(const char* name);
    bool wants(const char* name) const;
    hipEvent_t get_event();
    void begin(const char* name, hipStream_t s, bool single_launch = false);
    void end(hipStream_t s);
    // mode 3, inside a single-launch scope: the launch's slot for its device timestamps (nullptr: not wanted)
    unsigned long long* take_slot();
    // mode 4, inside a single-launch scope: the event pair the launch itself carries (false: not wanted, launch plainly)
    bool take_events(hipEvent_t* a, hipEvent_t* b);
    enum { TS_RING = 1 << 16 };
    unsigned long long* ts_dev = nullptr;   // [0, TS_RING): first start (min), [TS_RING, 2 TS_RING): last end (max)
    uint32_t ts_next = 0;
    void collect();  // after a stream sync: fold pending event pairs into recs
    void reset();
    ~Profiler();
    int cur = -1;
    int depth = 0;   // open scopes (only the outermost is timed)
    hipEvent_t cur_a = nullptr, cur_b = nullptr;
    bool ext_open = false;
    int ext_slot = -1;
    bool kev_open = false, kev_taken = false;
};

struct ProfScope {
    Profiler* p;
    hipStream_t s;
    bool on;
    // (mode 3 times the stamped sweeps ONLY: one timing-enabled event anywhere in the process switches the queue to per-dispatch
    //  profiling, and the sweeps themselves then run ~2 us longer -- bench.py takes the other kernels from a mode-1 pass)
    ProfScope(Profiler* p_, const char* name, hipStream_t s_, bool single_launch = false)
        : p(p_), s(s_), on(p_ && p_->mode && p_->wants(name) && (p_->mode != 3 || single_launch))
    {
        if (on) p->begin(name, s, single_launch);
    }
    ~ProfScope()
    {
        if (on) p->end(s);
    }
};

#include "sph_boundary_fused.hpp"   // HeaderOut (the step header), the header reduction's visiting order, the two-level cell-range table
#include "sph_solve_rule.hpp"       // the pressure solve: stop rule, progress word, deciders / sweep parts / tails / source kinds

// ---- Jacobi control block (device resident; copied to the host at sync points) ----------------
struct SolverCtrl {
    uint32_t done;    // stop decision taken (iisph_pressure_iterations break)
    uint32_t iters;   // num_pressure_iters at the break
    uint32_t cur;     // index of the pressure buffer holding the current iterate
    uint32_t peer_error;   // slab decomposition: a device-side guard fired on some rank (the solve was ended on every rank)
    uint32_t normal, singular, negative;
    float sum_err, max_err;
    uint32_t slot_done[2];   // stop decision as seen by the launches of one iteration (written by sweep A(k) into slot k & 1, sph_sweeps.hip)
    uint32_t seq;            // host copy only: sequence number of the k_publish that wrote it (wait_publish)
};

// error word layout: first failing guard wins (atomicCAS from 0)
struct DeviceStatus {
    uint32_t error;  // SPH_ERR_* or 0
    uint32_t info;   // particle index (host order) or auxiliary value
};

// what the reduction behind an integrating tail works on (sph_api.hip: k_header_ahead; sph_sort.hip: the header workgroup of the fused
// k_inc_count): the tail's partials, the solve's control block (nothing is reduced before the stop decision), the header's place in
// mapped host memory and -- h_ctrl != nullptr -- k_publish's job: control block and guard word to the host, `seq` last
struct HeaderAheadP {
    const HeaderOut* partials;
    uint32_t nparts;
    const SolverCtrl* ctrl;
    HeaderOut* out;
    const DeviceStatus* status;
    SolverCtrl* h_ctrl;
    DeviceStatus* h_status;
    uint32_t seq;
};
// ... by ONE workgroup of HDR_AHEAD_THREADS lanes in a fixed order (sph_boundary_fused.hpp: header_ahead_slot; lanes, then waves in
// index order).  Four partials per lane requested together: the launch sits on the step's critical path -- the host waits for its last
// store -- and 16 dependent load round trips per lane were most of its 8 us.  Every lane of the workgroup calls it; a __syncthreads()
// sits inside.
__device__ __forceinline__ void header_ahead_block(const HeaderAheadP& a)
{
    if (a.ctrl->done == 0u) {
        if (a.h_ctrl && threadIdx.x == 0) {
            SolverCtrl v = *a.ctrl;
            v.seq = a.seq - 1u;
            *a.h_ctrl = v;
            *a.h_status = *a.status;
            __threadfence_system();
            ((volatile SolverCtrl*)a.h_ctrl)->seq = a.seq;
        }
        return;
    }
    HeaderOut o = header_neutral();
    for (uint32_t k0 = threadIdx.x; k0 < a.nparts; k0 += 4u * HDR_AHEAD_THREADS) {
        HeaderOut q[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) q[u] = a.partials[header_ahead_slot(k0, u, a.nparts)];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) header_merge(o, q[u]);
    }
    o.min_x = wave_min(o.min_x); o.min_y = wave_min(o.min_y); o.max_x = wave_max(o.max_x); o.max_y = wave_max(o.max_y);
    o.h_max = wave_max(o.h_max); o.h_min = wave_min(o.h_min); o.min_cfl = wave_min(o.min_cfl);
    __shared__ HeaderOut s_hdr[HDR_AHEAD_THREADS / 64u];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane == 0) s_hdr[w] = o;
    __syncthreads();
    if (threadIdx.x == 0) {
        HeaderOut r = s_hdr[0];
        for (uint32_t k = 1; k < HDR_AHEAD_THREADS / 64u; k++) header_merge(r, s_hdr[k]);
        *a.out = r;
        if (a.h_ctrl) {
            SolverCtrl v = *a.ctrl;
            v.seq = a.seq - 1u;
            *a.h_ctrl = v;
            *a.h_status = *a.status;
            __threadfence_system();
            ((volatile SolverCtrl*)a.h_ctrl)->seq = a.seq;
        }
    }
}

// ---- sph_sort.hip ------------------------------------------------------------------------------
// Stable LSD radix sort of (key,val) pairs on `bits` key bits.  Returns 0 if the result is in
// (keyA,valA), 1 if in (keyB,valB).
// the cell sort's key source: cell index of a record; slots [0, n_gone) whose class byte is >= gone_from get the key ncells
struct CellKeyGen {
    const float4* pm;
    GridP g;
    const uint8_t* gone;
    uint32_t n_gone, gone_from;
    // 1: a record outside the grid gets the key of the nearest cell instead of an index beyond the cell table -- the grid of a build
    // queued AHEAD is a prediction (sph_step.hip: plan_ahead_build -- plan_grid with a margin, sph_grid_plan.hpp); such a build is never
    // adopted (the real bounding box does not fit its grid), but its kernels have run by then
    int clamp = 0;
};
// keygen != nullptr: the first pass computes the keys (keyA) and the identity values (valA) itself
int radix_sort_pairs(hipStream_t s, Profiler* prof, uint32_t* keyA, uint32_t* valA, uint32_t* keyB, uint32_t* valB,
                     uint32_t n, int bits, uint32_t* hist_scratch /* >= 256 * nblocks + 256 */, const CellKeyGen* keygen = nullptr);
size_t radix_sort_scratch_elems(uint32_t n);
// The same stable sort as a MERGE, for an array that is sorted by the cells q.cxy_cur (grid q.cur, ranges cell_start_cur) and whose
// particles mostly stay in their cells -- with the reorder of the per-particle arrays in the same pass: sorted keys of the positions
// pm_new in grid q.nxt (same cell size, clamped keys), the arrays of `io` in the new order and the new cell-range table
// [q.nxt.ncells + 1], bit for bit what radix_sort_pairs + launch_reorder + launch_cell_start produce (the permutation itself is never
// stored).  `classified`: the kernel that computed pm_new has run inc_classify_particle (sph_device.h) for every particle already.
// Scratch: q.nk[n], q.mv[n] bytes, q.next[n], q.head[q.nxt.ncells] (zeroed once when allocated, never cleared: q.epoch must differ
// from call to call and from 0), bsum[incremental_sort_block_sums(ncells)], movers (one zeroed word; the call leaves the number of
// movers in *movers_host).
struct ReorderIO {   // the per-particle arrays a reorder moves (h2n, lam, szc: optional, nullptr = not moved); sph_step.hip: reorder_io
    const float4* pm_in;
    const float2* vel_in;
    const uint32_t* orig_in;
    const float *lvl_in, *lvlold_in;
    float4* pm_out;
    float2* vel_out;
    uint32_t* orig_out;
    float *lvl_out, *lvlold_out;
    uint32_t* cxy_out;
    const float* h2n_in;
    float* h2n_out;
    const float* lam_in;
    float* lam_prev_out;
    const uint8_t* szc_in;
    uint8_t* szc_out;
    // lvl_in == nullptr (launch-uniform): the level fields hold the upload's constants in every slot of both halves and are not moved
    // (sph_ctx::lvl_pristine).  xv_out != nullptr: the merge's place launch also leaves {x, y, vx, vy} of every particle in its new
    // slot, the record the next step's fused a_ii / force sweep gathers (OpFuseU)
    float4* xv_out = nullptr;
};
size_t incremental_sort_block_sums(uint32_t ncells);
// `fused` (the build a plain context queues ahead behind its integrating tail, classified by that tail): count and place in TWO
// launches, and the count launch carries the reduction of the tail's header partials in a workgroup of its own -- no k_header_ahead
// in front, no k_inc_scan between.  Scratch on top of the above: local[ncells + 1], the cell-range table in its two-level form
// (sph_boundary_fused.hpp).
struct IncFusedP {
    uint32_t* local;
    HeaderAheadP hdr;
};
void incremental_cell_sort_reorder(hipStream_t s, Profiler* prof, uint32_t n, const float4* pm_new, const IncClassifyP& q, bool classified,
                                   const uint32_t* cell_start_cur, uint32_t* key_out, uint32_t* cell_start_out, const ReorderIO& io, uint32_t* bsum, uint32_t* movers,
                                   uint32_t* movers_host, const IncFusedP* fused = nullptr,
                                   bool serial_flags = false /* laboratory: the flag bytes of a cell one per round trip (Options::boundary_chains = 0) */);

// ... for a slab rank behind its fused refresh: slots [0, n_prev) are last step's sorted array (those of class >= kg.gone_from in
// kg.gone[0 .. kg.n_gone) left the rank and are not placed), [n_prev, n) this step's arrivals; sorted keys and the permutation
// (slot -> current index) of the live slots, and the cell-range table -- what radix_sort_pairs (with the key `ncells` for the slots
// that left) + launch_cell_start produce for them
void incremental_cell_sort_perm(hipStream_t s, Profiler* prof, uint32_t n, uint32_t n_prev, const CellKeyGen& kg, const IncClassifyP& q, const uint32_t* cell_start_cur,
                                uint32_t* key_out, uint32_t* perm_out, uint32_t* cell_start_out, uint32_t* bsum, uint32_t* movers, uint32_t* movers_host, bool serial_flags = false);

// out[i] = in[perm[i]] for every array of `io`, cxy_out[i] = the cell of sorted_key[i] in grid g; cell_start_scratch != nullptr: also
// clears the work-list counter of the launch_cell_start that follows
void launch_reorder(hipStream_t s, Profiler* prof, uint32_t n, GridP g, const uint32_t* sorted_key, const uint32_t* perm, const ReorderIO& io,
                    void* cell_start_scratch);
size_t cell_start_scratch_bytes();
void launch_cell_start(hipStream_t s, Profiler* prof, const uint32_t* sorted_key, uint32_t n, uint32_t ncells,
                       uint32_t* cell_start /* [ncells+1] */, void* scratch /* cell_start_scratch_bytes() */,
                       bool count_zeroed = false /* launch_reorder(.., scratch) already cleared the work-list counter */);
void launch_tile_hmax(hipStream_t s, Profiler* prof, uint32_t n, const float4* pm, GridP g, int ts, int tsx, int tsy, uint32_t* raw,
                      uint32_t* out /* dilated by one tile */, uint32_t* out_ext = nullptr /* dilated by d_ext tiles */, int d_ext = 2);

// ---- sph_sweeps.hip ----------------------------------------------------------------------------
struct SweepArgs {
    GridP g;
    StepP sp;
    uint32_t n;
    int exact;       // EXACT math mode
    int uniform_h;   // all h bit-identical
    float h_uniform;
    // grid structure
    const uint32_t* cell_start;
    const uint32_t* orig;
    // particle state (sorted order)
    const float4* pm;
    float2* vel;
    float2* vel_tmp;
    float* rho;
    float* lam_sum;
    float2* lam_grad;
    float2* wall_pl = nullptr;    // EXACT policy: the boundary handler's per-SDF gradient entries and their count (MathExact, sph_device.h)
    uint8_t* wall_cnt = nullptr;
    float* constf;
    float* aii;
    float* src;
    float* p0;
    float* p1;
    float4* pacc;       // {x, y, a^p} per particle (OpPressureAccel writes it, OpJacobiU gathers it whole)
    float* dens_err;
    float* stat;
    uint32_t* ncount;
    uint4* nl;          // neighbour list words (sph_sweeps.hip)
    uint4* nlx;         // explicit index lists (multi-resolution scenes)
    HeaderOut* hdr_partials;   // per-block partials of the NEXT step's header, written by the integrating final sweep (or nullptr)
    IncClassifyP inc;          // the integrating tail also classifies its particles for the incremental cell sort queued behind it (head == nullptr: no)
    int h_mode;         // support_length_estimation (SPH_H_*)
    int sp_check_aii;   // SimulationParams::check_aii
    float* h2_next;     // FromDistribution*: the estimate for the next step is written here by the density sweep
    float* omega;       // IISPH2
    const uint8_t* size_class;
    const float* lam_prev;
    const uint2* nloff = nullptr;   // relative-offset lists of this step (sph_sweeps.hip: k_sweep_off) and their header bytes; nullptr: the
    const uint8_t* nlh = nullptr;   //   gradient sweeps of a uniform scene replay the mask words
    uint2* nloff_out = nullptr;     // the density BUILD sweep writes them (set for that launch only)
    uint8_t* nlh_out = nullptr;
    uint4* nl_ext;      // list words / index lists of the extended-range lists (level estimation)
    uint4* nlx_ext;
    TileP t;            // stencil bound per tile (multi-resolution scenes; ts = 0: uniform)
    TileP t_ext;        // the same bound over a wider tile neighbourhood, for the extended-range lists
    float* partials;    // per-block solver statistics
    const uint8_t* owned;  // slab decomposition: 1 owned, 0 ghost (nullptr: everything is owned)
    const uint8_t* ring1;  // slab decomposition: 1 = ghost within one support radius of the cut (runs the RING1 ops)
    // slab decomposition, split sweep (SweepCommon): 1 = halo member or ghost; the halo members' slots, the ghosts' slots
    const uint8_t* edge = nullptr;
    const uint32_t* elist_a = nullptr;
    const uint32_t* elist_b = nullptr;
    uint32_t n_ea = 0, n_eb = 0;
    SweepPart part = PART_WHOLE;
    double* solver_tot; // multi-rank: all-reduced solver totals (RCCL: this rank's own row; the others' rows in tot_table)
    const double* tot_table = nullptr;   // RCCL transport: every rank's totals side by side, summed by the readers (SolveP, sph_sweeps.hip)
    int tot_nr = 0, tot_self = 0;
    float* mrho;        // m / rho
    float* pt0;         // p / rho^2 for pressure buffer 0 / 1
    float* pt1;
    float4* rec0 = nullptr;   // {x, y, p / rho^2, p} for pressure buffer 0 / 1: written INSTEAD of pt0 / pt1 by the solves of uniform-h scenes
    float4* rec1 = nullptr;   // on one context (OpPressureAccelU gathers one record per neighbour); nullptr: slabs, IISPH2
    float4* xv = nullptr;     // {x, y, vx, vy}: what the source-term sweep of such a scene gathers per neighbour (OpSourceU) -- written by whoever
    bool xv_ok = false;       // writes the velocities behind the step's sort (the non-pressure forces, the divergence solve's tail); xv_ok: it
                              // holds the current positions and velocities (set by the step driver behind those launches); nullptr: slabs, IISPH2
    // the fused a_ii / force sweep of such a scene on records (OpFuseU): xv_in = {x, y, vx, vy} in this step's order, left by the place
    // launch of the build this step adopted (nullptr: it left none -- another build, or something dropped it)
    const float4* xv_in = nullptr;
    // boundary
    const BoundaryP* planes;
    const float* lam_lut;
    const float* dlam_lut;
    // control
    SolverCtrl* ctrl;
    const uint32_t* gate = nullptr;   // chained solves: the launches of the second solve leave at once while this word is 0 (k_solver_handoff)
    DeviceStatus* status;
    // paced solves: the stop decision of every iteration is also stored in mapped host memory (sph_solve_rule.hpp: prog_word), so that
    // the host queues iterations against the device's progress (sph_step.hip: solve_paced)
    uint32_t* prog_host = nullptr;
    uint32_t prog_epoch = 0;
    int opt_tile = 0, opt_jacobi_generic = 0;   // Options::tile / ::jacobi_generic of the context (sph_context.hpp)
    int opt_boundary_chains = 1;                // Options::boundary_chains (the tail's form: launch_solver_tail, solver_tail_partials)
    Profiler* prof = nullptr;                   // host side only: the context's profiler (launch_sweep asks it for a timestamp slot)
};

// the solves of this step keep p / rho^2 inside the 16-byte records {x, y, p / rho^2, p} (rec0 / rec1) that sweep A gathers whole, not
// in pt0 / pt1: what a slab decomposition exchanges for its ghosts per iteration is then word 2 of those records
bool sweep_a_on_records(const SweepArgs& a);
bool source_term_on_records(const SweepArgs& a);   // the step driver sets SweepArgs::xv_ok behind the launches that write the record
bool fused_sweep_on_records(const SweepArgs& a);   // launch_aii_const_non_pressure runs OpFuseU (xv_in set by the step driver)
size_t sweep_list_bytes(uint32_t n);
size_t sweep_index_list_bytes(uint32_t n);   // explicit index lists (multi-resolution scenes)
size_t sweep_offset_list_bytes(uint32_t n);  // relative-offset lists (uniform scenes whose solves run on records)
bool sweeps_want_offset_lists(const SweepArgs& a);
bool sweep_forces_index_lists();             // build variant SPH_FORCE_IDX
uint32_t solver_reduce_blocks(uint32_t n);
void launch_density(hipStream_t s, Profiler* prof, const SweepArgs& a);
void launch_density_replay(hipStream_t s, Profiler* prof, const SweepArgs& a);
void launch_constrain_init(hipStream_t s, Profiler* prof, const SweepArgs& a, uint32_t target, float* thr, uint32_t* consumed, float* h_new, uint8_t* flag);
void launch_constrain_pass(hipStream_t s, Profiler* prof, const SweepArgs& a, uint32_t target, float* thr, uint32_t* consumed, float* h_new, uint32_t* pending);
void launch_constrain_apply(hipStream_t s, Profiler* prof, const SweepArgs& a, float4* pm, const float* h_new, float* h2_next);
void launch_aii_const(hipStream_t s, Profiler* prof, const SweepArgs& a);
void launch_aii_const_non_pressure(hipStream_t s, Profiler* prof, const SweepArgs& a);   // + the non-pressure acceleration, one sweep
void launch_non_pressure(hipStream_t s, Profiler* prof, const SweepArgs& a);                // vel -> vel_tmp
void launch_source_term(hipStream_t s, Profiler* prof, const SweepArgs& a, SourceKind kind, int residual_density);  // includes Jacobi iteration 0
// sweep A of iteration iter >= 1 and, by its block 0, the stop decision of iteration iter - 1 (`decider`; the two launches of a split
// sweep, `part` != PART_WHOLE, take DECIDE_NOT_HERE); iter < 0: a^p from the solve's final pressures, nothing is decided or read of `rule`
void launch_pressure_accel(hipStream_t s, Profiler* prof, const SweepArgs& a, int iter, const SolveRule& rule, SolveDecider decider, SweepPart part = PART_WHOLE);
// slab decomposition: this rank's totals of iteration `iter`, as block 0 of the launch that packs the halo members' values for the
// iteration's ghost exchange (sph_slabs.hip: refresh_ghosts)
void launch_pack_and_totals(hipStream_t s, Profiler* prof, const SweepArgs& a, int iter, const uint32_t* src_idx, uint32_t cnt0, uint32_t cnt1, int words, int stride,
                            int off, const float* field, float* out0, float* out1);
void launch_ctrl_reset(hipStream_t s, SolverCtrl* ctrl, const uint32_t* gate);
// slab decomposition: the decision on iteration `iter` from the all-reduced totals (DECIDE_FROM_TOTALS) by a launch of its own
void launch_solver_progress(hipStream_t s, Profiler* prof, const SweepArgs& a, int iter, const SolveRule& rule);
void launch_solver_handoff(hipStream_t s, Profiler* prof, SolverCtrl* ctrl, SolverCtrl* saved_host, uint32_t* gate);
// the integrate map of the solver mode, once the solve is done; gate_out: the tail also does k_solver_handoff's job
void launch_solver_tail(hipStream_t s, Profiler* prof, const SweepArgs& a, SolveTail tail, float4* pm_out, SolverCtrl* handoff_host = nullptr,
                        uint32_t* gate_out = nullptr);
// A workgroup of the tail owns a tile of U x 256 consecutive particles (k_solver_tail): U of the integrating tails and of TAIL_VEL, as
// measured (profiles/step_boundary_chains.md; a variant build sets another one, scripts/variants).  `chains` =
// Options::boundary_chains: 0 (laboratory build) the one-particle form the tiled one replaced.
#ifndef SOLVER_TAIL_U
#define SOLVER_TAIL_U 2       // (1: 16.5, 2: 16.0, 4: 16.6 us for the integrating tail at 2^20 particles, the one-particle form 17.1)
#endif
#ifndef SOLVER_TAIL_VEL_U
#define SOLVER_TAIL_VEL_U 2   // (1: 10.5, 2: 9.1, 4: 9.9 us, the one-particle form 11.4 in the same traces)
#endif
inline uint32_t solver_tail_tile(SolveTail tail, int chains)
{
    if (chains == 0) return 1u;
    return tail == TAIL_VEL ? (uint32_t)SOLVER_TAIL_VEL_U : (uint32_t)SOLVER_TAIL_U;
}
// the header partials an integrating tail leaves for n particles: one per workgroup -- what every reader of SweepArgs::hdr_partials is told
inline uint32_t solver_tail_partials(uint32_t n, int chains)
{
    const uint32_t tile = 256u * solver_tail_tile(TAIL_VX, chains);
    return (n + tile - 1u) / tile;
}
void launch_jacobi_update(hipStream_t s, Profiler* prof, const SweepArgs& a, int iter, const SolveRule& rule);   // sweep B
// level estimation (sorted order)
struct LevelArgs {
    float k;                       // level_estimation_range / ETA
    float threshold;               // cos(50 degrees)
    float max_surface_distance;
    int boundary_is_fluid_surface;
    float2* nrm;
    uint8_t* state;
    uint8_t* flag_surface;
    uint8_t* flag_insufficient;
    float maximum_range;   // is_neighbor_in_level_estimation_range (FromDistribution / FromDistribution2), < 0: rule off
    uint8_t* size_class;
    float* level;                  // the level field (detection output, propagated in place)
    uint32_t* when;                // propagation sweep that assigned the value (sph_sweeps.hip)
    uint32_t* mark;                // 2 n words: frontier marks, double-buffered by sweep parity 
    uint8_t* fmap = nullptr;       // one context: the propagation on a compacted frontier (sph_sweeps.hip: k_level_frontier) -- two candidate
    uint32_t fmap_lg_s = 0;        //   maps of 64 S bytes, S = 1 << fmap_lg_s >= n / 64 (transposed: particle j at byte (j mod S) 64 + j / S); nullptr: the sweep forms
    float* level_old;
    float* stash_first;            // stash filled right after the detection (SurfaceDistanceFirst) or nullptr
    int center_diff;               // surface_detection_by_center_diff instead of the empty-angle detector
    int plain_propagate;           // slab decomposition: 1 = propagation without frontier marks, 2 = frontier form with probing halo members (OpLevelPropagate)
    const uint8_t* edge;           // mode 2: the slab's halo-member / ghost flags (sph_slabs.hip)
    int replay_step_lists;         // after advection without the extended range: the step's k = 2 lists at the advected positions
    const float4* pm_cell;         // level estimation after advection: the pre-step positions (cells); a.pm = advected. Else nullptr
};
void launch_max_disp(hipStream_t s, Profiler* prof, uint32_t n, const float4* pm_old, const float4* pm_new, uint32_t* out);
void launch_tile_redilate(hipStream_t s, Profiler* prof, int tsx, int tsy, int d, const uint32_t* raw, uint32_t* out);
void launch_level_detect(hipStream_t s, Profiler* prof, const SweepArgs& a, const LevelArgs& l);
void launch_level_propagate(hipStream_t s, Profiler* prof, const SweepArgs& a, const LevelArgs& l, uint32_t t, uint32_t* changed);
void launch_fill_stash(hipStream_t s, Profiler* prof, const SweepArgs& a, const LevelArgs& l, float* stash);
void launch_level_smooth(hipStream_t s, Profiler* prof, const SweepArgs& a, const LevelArgs& l, const float4* pm_new, const float* in, float* out);
void launch_classify(hipStream_t s, Profiler* prof, uint32_t n, const float4* pm, const float* level, uint8_t* size_class, const uint8_t* owned,
                     const uint32_t* orig, DeviceStatus* status, const sph_params* p);
// reduce the per-block header partials of the integrating final sweep into `out_dev` (skipped while the solve is not done)
void launch_header_ahead(sph_ctx* c, uint32_t nblocks, HeaderOut* out_dev, bool publish = false);   // publish: also k_publish's job (the next launch_publish is a no-op)
// ... or its arguments, for the launch that carries the reduction instead (the fused k_inc_count: IncFusedP::hdr); the same bookkeeping
HeaderAheadP header_ahead_args(sph_ctx* c, uint32_t nblocks, HeaderOut* out_dev, bool publish);
// IISPH2: p /= sqrt(omega) on the current pressure buffer (+ p / rho^2), simulation.rs:2358-2360
void launch_iisph2_scale(hipStream_t s, Profiler* prof, const SweepArgs& a);
void launch_check_aii(hipStream_t s, Profiler* prof, const SweepArgs& a);   // after launch_aii_const when check_aii is set

// ---- regather of the persistent state into a new HOST-index order (sparse edits, merging, splitting; sph_api.hip) ----
struct EditSrc {
    uint32_t obj;      // object: < n_old = the particle with that OLD host index, else a default particle of an EXTEND
    uint32_t set_idx;  // index into the override records, or 0xffffffff
};
struct EditSet {
    uint32_t fields;   // SPH_EDIT_F_* of the values to take from this record
    float mass, px, py, vx, vy, h2, h2_next, lvl, lvlold;
};
struct sph_ctx;
// final index f holds object d_src[f].obj (+ the overrides of d_sets[d_src[f].set_idx]); both arrays live on the DEVICE.
// Slot f = host index f afterwards, like a fresh upload; per-step outputs, lists and the header are invalidated.
int regather_host_order(sph_ctx* c, uint32_t n_new, const EditSrc* d_src, const EditSet* d_sets);
// out[i] = sum of in[0 .. i) ; *total (device word) = sum of all.  scratch: >= (n / 2048 + 2) words
void device_exclusive_scan_u32(hipStream_t s, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* scratch, uint32_t* total);
// sph_adapt.hip: share (merging = 0) / merge (1) applied from partner / counter arrays that are on the device (sph_partner_problem.hip)
int transfer_on_device(struct sph_ctx* c, const struct sph_params* p, const struct sph_adapt_params* ap, const uint32_t* d_partner, const uint16_t* d_counter,
                       int merging);
