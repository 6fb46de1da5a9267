/*
 * sph_slab_partner_problem.h -- the compact partner problem on SLAB contexts: only the participants cross the bus.
 *
 * sph_partner_problem.h refuses a slab context (SPH_ERR_UNSUPPORTED): its compact ids number the host indices of ONE vector.
 * sph_slab_candidates.h filters the rows on every rank, but the host still gathers the five decision fields of every particle and every
 * rank still takes merge_partner / merge_counter of the whole vector.  These entry points are the slab form of sph_partner_problem.h:
 * every rank packs ITS LOCAL PROBLEM -- the participants its own rows touch -- on the device, the host merges the ranks' problems by
 * global id into one problem of size K (distributed.merge_slab_partner_problems), runs the same sequential search on it with n = K
 * (find_share_partner_sequential, adaptivity/particle_sharing.rs:14-117; find_merge_partner_sequential, particle_merging.rs:16-125),
 * and every rank applies the K decisions to its own slab.
 *
 * THE LOCAL PROBLEM of a rank, for the candidate rows sph_slab_candidates_prepare(ctx, kind, params, ap, ..) prepares (the same lists,
 * tests and field values; sph_slab_candidates.h states them):
 *   - OWNED participants: every owned particle whose candidate row is not empty, and every owned particle that occurs in a row of this
 *     rank.  They come first, in row order: the order of sph_download(SPH_F_PARTICLE_ID), not sorted by id.
 *   - FOREIGN participants: every particle of another rank that occurs in a row of this rank (it sits in this rank's ghost layer).  They
 *     follow the owned ones in the order of their slots in the rank's arrays at the prepare: the same state gives the same order, two
 *     ranks or two steps need not agree on it, and it is not sorted by id -- the host merge orders everything by id.
 *   - per participant: its global id, its size class, mass, level_estimation, position and h2 -- the values sph_download returns for
 *     that particle ON ITS OWNER at the moment of the prepare, bit for bit.  A foreign participant's come from its ghost record and
 *     level, which the prepare refreshes from the owner first (stale behind a share otherwise), and its class is what
 *     sph_classify(params) gives the owner.  h2 is the record's own h2 word, as sph_download(SPH_F_H2) reads it.
 *   - offsets[n_owned_participants + 1]: the candidate rows of the OWNED participants, in their order; a participant that is no donor
 *     has an empty row, a foreign participant has no row on this rank (its owner reports it).
 *   - indices[n_indices]: the entries in GLOBAL ids -- the very array sph_slab_candidates_download returns, not a second copy.  Every
 *     entry names a participant of this rank.
 * A particle that takes part on two ranks (owned on one, foreign on the other, or foreign on two) is reported by both with equal field
 * values.  Nothing an owned particle holds is written by the prepare.
 *
 * VALIDITY.  The packed problem is a snapshot: sph_slab_partner_problem_download returns what was packed at the prepare, also behind a
 * share that has changed the masses since.  It is valid exactly as long as the prepared rows are (sph_slab_candidates.h: dropped by
 * sph_step / sph_group_step, sph_upload, sph_upload_field of position, mass or particle ids, sph_apply_edits, sph_set_math_policy, a
 * merge or split that renumbered the vector) and it is dropped by a later sph_slab_candidates_prepare, which replaces the rows.
 *
 * THE APPLY carries its ids: there is no open problem on a slab context.  It fills merge_partner / merge_counter of the whole vector with
 * AVAILABLE / 0 on the device, uploads the K ids and decisions (10 B per participant and rank) and scatters them -- a compact partner id
 * mapped through ids, the sentinels left alone; everything behind that point is sph_share_particles / sph_merge_particles on a slab
 * context with those arrays, so the resulting state is the same bit for bit.
 *
 * A separate header from sph_ffi.h.  Status codes are those of sph_ffi.h: a plain context -> SPH_ERR_UNSUPPORTED (it takes
 * sph_partner_problem.h), a poisoned one -> SPH_ERR_POISONED; SPH_ERR_INVALID_ARGUMENT for everything sph_slab_candidates_prepare
 * refuses (kind outside {0, 1}, NULL params or ap, no step before the call, no lists and nothing to build them from), a download
 * without a prepared problem or after it was dropped, a capacity that is too small, and the apply's argument checks below.
 */
#ifndef SPH_SLAB_PARTNER_PROBLEM_H
#define SPH_SLAB_PARTNER_PROBLEM_H

#include <stdint.h>

#include "sph_ffi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* COLLECTIVE through the context's own transport, like sph_slab_candidates_prepare, which it runs first (the prepared rows are then
 * those sph_slab_candidates_download returns): every rank calls it, in the same order, behind the same step and its own sph_classify.
 * Then mark, scan and pack on the rank's stream; only the three counts cross the bus.  *n_participants = the local problem's size,
 * *n_owned_participants = how many of them this rank owns (they come first), *n_indices = the entries of its rows.  A failure on one
 * rank ends the call on every rank; no problem is prepared then. */
int sph_slab_partner_problem_prepare(sph_ctx* ctx, int kind, const sph_params* params, const sph_adapt_params* ap, uint64_t* n_participants,
                                     uint64_t* n_owned_participants, uint64_t* n_indices);
/* The same for the n contexts of ONE process that sph_group_step steps as ranks 0 .. n-1; the three outputs are arrays of n. */
int sph_group_slab_partner_problem_prepare(sph_ctx** ctxs, int n, int kind, const sph_params* params, const sph_adapt_params* ap,
                                           uint64_t* n_participants, uint64_t* n_owned_participants, uint64_t* n_indices);

/* Local, no collective: the problem packed by the last prepare.  Every array pointer may be NULL (the two-call convention of
 * sph_download_partner_problem: a call with all of them NULL sizes the problem through the three count pointers, each of which may be
 * NULL as well and is set whenever a problem is prepared, also when a capacity is then refused):
 *   ids[K], size_class[K], mass[K], level_estimation[K], position[2 K], h2[K]      K = *n_participants, owned participants first
 *   offsets[Ko + 1]                                                               Ko = *n_owned_participants
 *   indices[*n_indices]                                                           global ids
 * participants_capacity counts the entries of the per-participant arrays (offsets: participants_capacity + 1), indices_capacity those
 * of indices.  A per-participant array or offsets given with participants_capacity < K, or indices given with indices_capacity <
 * *n_indices -> SPH_ERR_INVALID_ARGUMENT with the counts set; the problem stays prepared.  No prepared problem: the counts are 0. */
int sph_slab_partner_problem_download(sph_ctx* ctx, uint32_t* ids, uint8_t* size_class, float* mass, float* level_estimation, float* position,
                                      float* h2, uint32_t* offsets, uint64_t participants_capacity, uint32_t* indices, uint64_t indices_capacity,
                                      uint64_t* n_participants, uint64_t* n_owned_participants, uint64_t* n_indices);

/* sph_share_particles / sph_merge_particles on a slab context from K decisions.  COLLECTIVE like them; every rank passes the SAME arrays:
 *   ids[k]        global particle ids, strictly ascending (the merged problem's ids)
 *   partner_c[k]  SPH_MERGE_PARTNER_AVAILABLE, SPH_MERGE_PARTNER_DELETE or a compact id < k
 *   counter_c[k]  the merge counters
 * Everything that is not named by ids keeps AVAILABLE / 0.  k = 0 is valid (nothing is transferred).
 * SPH_ERR_INVALID_ARGUMENT, on the host, before anything on the device is written and on every rank alike: an array NULL with k > 0,
 * ids not strictly ascending, a partner that is neither a sentinel nor < k (all three before any collective), an id >= n_global (as
 * soon as the ranks' counts are added up -- the apply's first collective, which also sph_share_particles starts with; the transport
 * stays usable).  The other refusals are those of sph_share_particles on a slab context (no step before the call, a donor that is no
 * neighbour of its receiver, ...). */
int sph_slab_share_particles_compact(sph_ctx* ctx, const sph_params* params, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids,
                                     const uint32_t* partner_c, const uint16_t* counter_c);
int sph_slab_merge_particles_compact(sph_ctx* ctx, const sph_params* params, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids,
                                     const uint32_t* partner_c, const uint16_t* counter_c);
/* The same for the n contexts of ONE process (sph_group_adapt's form); op: 0 share, 1 merge.  A split takes no decisions: sph_group_adapt. */
int sph_group_adapt_compact(sph_ctx** ctxs, int n, int op, const sph_params* params, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids,
                            const uint32_t* partner_c, const uint16_t* counter_c);

#ifdef __cplusplus
}
#endif

#endif /* SPH_SLAB_PARTNER_PROBLEM_H */
