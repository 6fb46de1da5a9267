/*
 * sph_partner_search.h -- the partner searches on the device: the decisions never cross the bus.
 *
 * sph_partner_problem.h numbers the participants of a search 0..K-1 on the device and lets the host run the sequential loop
 * (find_share_partner_sequential, adaptivity/particle_sharing.rs:14-117; find_merge_partner_sequential, particle_merging.rs:16-125) on
 * that problem.  Here the loop itself runs on the device, in its exact parallel schedule:
 *
 *   touch(i) = row(i) + {i} for a donor i with a non-empty candidate row: everything the loop reads or writes of merge_partner while it
 *   visits i.  writers(x): the donors whose touch set holds x, ascending.  A donor is FINISHED once it ran its row and RETIRED once it
 *   was claimed before it ran (the loop lets such a donor accept nobody).  head(x): the first writer of x that is neither.  Donor i is
 *   READY iff every x of touch(i) is claimed already (final: i skips it) or has head(x) == i.  A round runs the rows of all ready donors
 *   as the loop does -- entries in their order, new_mass_j = mass[j] + dropped_i / (float)(counter_i + 1) in f32, the same comparisons.
 *   Two ready donors never share an unclaimed particle, the smallest undecided donor is always ready, and by induction over the donor
 *   index every row sees what it sees in the sequential loop: merge_partner / merge_counter are those of the loop, entry for entry.
 *
 * The decisions stay on the device as THE OPEN SOLUTION of the context, next to the open problem they belong to;
 * sph_share_particles_device / sph_merge_particles_device expand and apply them there.  Only the info struct crosses the bus.
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only.  Status codes are those of sph_ffi.h.
 * Every launch runs on the context's stream.
 */
#ifndef SPH_PARTNER_SEARCH_H
#define SPH_PARTNER_SEARCH_H

#include <stdint.h>

#include "sph_ffi.h"
#include "sph_partner_problem.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t participants; /* K of sph_download_partner_problem for the same state and kind */
    uint64_t candidates;   /* the entries of its rows */
    uint64_t donors;       /* participants with merge_counter > 0 */
    uint64_t transfers;    /* the sum of merge_counter */
    uint32_t rounds;       /* rounds of the schedule */
    uint32_t max_frontier; /* the most donors ready in one round */
    uint32_t wide_rounds;  /* rounds that ran as grid launches (frontier >= the wide threshold) */
    uint32_t reserved;
} sph_partner_search_info;

/* kind: 0 share, 1 merge.  Builds the compact problem of sph_download_partner_problem(ctx, kind, params, ap, ..) on the device -- the same
 * lists, tests and field values -- and solves it there.  On success the problem is THE OPEN PROBLEM of the context (it replaces an
 * earlier one, sph_share_particles_compact / sph_merge_particles_compact would accept it) and its decisions are THE OPEN SOLUTION;
 * everything that closes an open problem (the list in sph_partner_problem.h) closes the solution with it, and so does the next
 * sph_download_partner_problem.  The call changes nothing of the simulation state.
 * wide_threshold: a round whose frontier holds at least that many donors runs as grid launches, a smaller one inside the resident
 * one-workgroup kernel; 0 = the library's default, 1 = every round wide, 0xFFFFFFFF = every round resident.  The decisions do not
 * depend on it.
 * K == 0 (no donor has a candidate): success, *info all zero, an open solution without decisions.
 * The decisions are validated on the device (validate_share_partners, particle_sharing.rs:119-150 / validate_merge_partners,
 * particle_merging.rs:226-268); a violation, a merge counter of 1000, or a round without a ready donor while donors remain
 * -> SPH_ERR_DEVICE, no open solution.
 * Refusals are those of sph_download_partner_problem: a slab context -> SPH_ERR_UNSUPPORTED; no lists and nothing to build them from,
 * kind outside {0, 1}, params, ap or info NULL -> SPH_ERR_INVALID_ARGUMENT; a poisoned context -> SPH_ERR_POISONED. */
int sph_find_partners_device(sph_ctx* ctx, int kind, const sph_params* params, const sph_adapt_params* ap, uint32_t wide_threshold,
                             sph_partner_search_info* info);

/* Inspection only; leaves the solution open.  ids[k] as in sph_download_partner_problem; partner_c[k] holds SPH_MERGE_PARTNER_AVAILABLE,
 * SPH_MERGE_PARTNER_DELETE or a compact id < k, counter_c[k] the merge counters.  Every pointer may be NULL.
 * No open solution, or k != K -> SPH_ERR_INVALID_ARGUMENT. */
int sph_download_partner_decisions(sph_ctx* ctx, uint64_t k, uint32_t* ids, uint32_t* partner_c, uint16_t* counter_c);

/* sph_share_particles / sph_merge_particles from the open solution: the decisions are expanded on the device into merge_partner /
 * merge_counter of the whole vector (AVAILABLE / 0 for everything that is no participant, compact ids mapped through ids) and applied as
 * sph_share_particles / sph_merge_particles apply those arrays: the resulting state is the same bit for bit.  With K == 0 that is the
 * apply of all-AVAILABLE arrays.  The solution and its problem are consumed.
 * SPH_ERR_INVALID_ARGUMENT, before anything on the device is modified: no open solution (none was made, or a step, an upload, an edit,
 * a merge, a split, a policy change or a later sph_download_partner_problem closed it) or one of the other kind (share: 0, merge: 1).
 * A slab context -> SPH_ERR_UNSUPPORTED; a poisoned one -> SPH_ERR_POISONED. */
int sph_share_particles_device(sph_ctx* ctx, const sph_params* params, const sph_adapt_params* ap);
int sph_merge_particles_device(sph_ctx* ctx, const sph_params* params, const sph_adapt_params* ap);

#ifdef __cplusplus
}
#endif

#endif /* SPH_PARTNER_SEARCH_H */
