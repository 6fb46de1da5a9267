// The pressure solve's protocol, stated once for the device (sph_sweeps.hip) and the host (sph_step.hip): the stop rule and its three
// parameters, the progress word a paced solve publishes, and the roles a launch of the solve can take (who decides, which part of a
// split sweep, which tail, which source term).  Plain C++ behind a host/device macro: tests/host/solve_rule_check.cpp compiles this
// header with g++ and tests/test_solve_rule_host.py runs it.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef SPH_HD
#if defined(__HIPCC__)
#define SPH_HD __host__ __device__ __forceinline__
#else
#define SPH_HD inline
#endif
#endif

// ---- the stop rule (iisph_pressure_iterations, simulation.rs:1453-1479) ------------------------------------------------------------
struct SolveRule {
    int residual_density;   // 1: the residual is a density error (relative to rest_density); 0: a divergence error (times dt)
    float max_avg_error;
    uint32_t max_iters;
};
// ... for iteration `iter`, from the number of "normal" particles and the sum of their residuals
SPH_HD bool solver_stop_rule(uint32_t normal, float sum_err, int iter, const SolveRule& q, float rest_density, float dt)
{
    const float avg = normal > 0 ? sum_err / (float)normal : NAN;
    bool stop;
    if (q.residual_density) stop = normal == 0 || (fabsf(avg / rest_density) < q.max_avg_error && iter > 1);
    else stop = normal == 0 || (fabsf(avg) < q.max_avg_error / dt && iter > 1);
    if (!stop && (uint32_t)iter == q.max_iters) stop = true;
    return stop;
}

// ---- the progress word of a paced solve ---------------------------------------------------------------------------------------------
// Whoever takes the stop decision of an iteration also stores it in one word of mapped host memory, (epoch << 16) | (stop << 15) |
// iteration, and the host queues iterations against it (sph_step.hip: solve_paced).  Every paced solve of a context carries the next
// epoch; epoch 0 is never handed out, so a zeroed word -- and any word an earlier solve left -- is not "seen" by the solve that reads it.
// The iteration has 15 bits: a solve that may run longer than PROG_MAX_ITERS iterations is not paced.
#define PROG_MAX_ITERS 0x7fffu
SPH_HD uint32_t prog_word(uint32_t epoch, bool stop, uint32_t iter) { return (epoch << 16) | (stop ? 0x8000u : 0u) | (iter & PROG_MAX_ITERS); }
SPH_HD bool prog_seen(uint32_t word, uint32_t epoch) { return (word >> 16) == epoch; }   // written by a launch of THIS solve
SPH_HD bool prog_stopped(uint32_t word) { return (word & 0x8000u) != 0u; }
SPH_HD uint32_t prog_decided(uint32_t word) { return word & PROG_MAX_ITERS; }             // iterations 0 .. this one are decided
SPH_HD uint32_t prog_next_epoch(uint32_t epoch) { return epoch >= 0xffffu ? 1u : epoch + 1u; }

// ---- roles ------------------------------------------------------------------------------------------------------------------------
// Who takes the stop decision of iteration k - 1 in the launch of sweep A(k):
enum SolveDecider : int {
    DECIDE_FROM_PARTIALS = 0,   // one context: block 0 reduces the partials sweep B left behind and decides
    DECIDE_FROM_TOTALS = 1,     // slab decomposition: the launch runs BEHIND the all-reduce of the totals that travelled with the ghost
                                // exchange, its block 0 decides from them (solver_decide_multi) -- the place and the protocol of the
                                // one-context form, so sweep B and the tail read one flag whatever the transport
    DECIDE_NOT_HERE = 2,        // nobody in this launch (the two launches of a split sweep A: k_solver_progress decides between them)
};
// A sweep of a slab decomposition in two launches (the ghost exchange runs under the first):
enum SweepPart : int {
    PART_WHOLE = 0,      // one launch
    PART_INTERIOR = 1,   // every lane whose `edge` byte is 0 (owned, no ghost within reach)
    PART_EDGE = 2,       // the listed slots (the halo members, then the ghosts)
};
// What follows the LAST pressure-acceleration sweep of a solve (k_solver_tail, a per-particle map):
enum SolveTail : int {
    TAIL_NONE = 0,     // nothing
    TAIL_VEL = 1,      // HybridDFSPH after the divergence solve: v += dt a^p                    (simulation.rs:2547-2560)
    TAIL_VX = 2,       // IISPH / OnlyDivergence: v += dt a^p ; x += dt v                         (simulation.rs:2433-2445, 2486-2499)
    TAIL_HYBRID = 3,   // HybridDFSPH: x += dt v + dt^2 a^p ; v += dt a^p * min(dt*factor, 1)   (simulation.rs:2644-2646)
};
// The source term of the pressure equation (OpSource):
enum SourceKind : int {
    SRC_DIVERGENCE = 0,     // prepare_ppe_divergence
    SRC_FULL = 1,           // prepare_full_ppe
    SRC_ONLY_DENSITY = 2,   // prepare_only_density_part_ppe
    SRC_FULL_OMEGA = 3,     // IISPH2: the full source term with the per-particle omega
};
