/*
 * sph_partner_problem.h -- the partner searches as a compact problem: only the donors and their candidates cross the bus.
 *
 * sph_candidates.h hands the host the candidate rows of find_share_partner_sequential (adaptivity/particle_sharing.rs:14-117) /
 * find_merge_partner_sequential (particle_merging.rs:16-125) as a CSR over ALL particles, and the host still downloads the five
 * decision fields of every particle and uploads merge_partner / merge_counter of every particle.  The search reads and writes only
 * two sets of particles: the donors that have at least one candidate, and the particles that occur as candidates -- the
 * PARTICIPANTS.  sph_download_partner_problem numbers them 0..K-1 on the device and hands the host a self-contained problem of
 * size K; sph_share_particles_compact / sph_merge_particles_compact take the decisions back in that numbering.
 *
 * Why the host's loop, run UNCHANGED with n = K on the compact arrays, takes the decisions it takes on the full vector:
 *   - it visits the donors in ascending index, and the renumbering is monotone (compact id c = rank of host index ids[c]), so
 *     the donors are visited in the same order; rows and their entries keep their order, so every donor tries the same j in the
 *     same order;
 *   - a donor whose candidate row is empty writes nothing in the full loop (it is left out here), and every state the loop reads
 *     or writes belongs to a participant: mass[i], mass[j], target_mass(level[i]), target_mass(level[j]), merge_partner[j],
 *     merge_partner[i], merge_counter[i] for a donor i with a non-empty row and an entry j of that row;
 *   - class, position and h2 are read by the two tests the rows have passed already (idempotent, sph_candidates.h).
 * Everything that is no participant keeps merge_partner = AVAILABLE, merge_counter = 0.  validate_share_partners /
 * validate_merge_partners hold on the compact arrays as they hold on the candidate rows.
 *
 * A separate header from sph_ffi.h and sph_candidates.h: these entry points exist in the product library only.
 * Status codes are those of sph_ffi.h.  Every launch runs on the context's stream.
 */
#ifndef SPH_PARTNER_PROBLEM_H
#define SPH_PARTNER_PROBLEM_H

#include <stdint.h>

#include "sph_ffi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind: 0 share, 1 merge.  The candidate rows are exactly those of sph_download_partner_candidates(ctx, kind, params, ap, ..): the
 * same lists (kept on the device from the first export of a step), the same two tests, the same field values -- those sph_download
 * would return at the moment of the call.  Participants: every donor whose candidate row is not empty, and every j that occurs in a
 * candidate row; numbered in ascending host index.
 *
 * Outputs (K = *n_participants, always set; *n_indices = the candidates' total, always set).  Every array pointer may be NULL (the
 * two-call convention of sph_download_neighbors: a call with all of them NULL sizes the problem):
 *   ids[K]                       host index of compact id c, strictly ascending
 *   size_class[K], mass[K], level_estimation[K], position[2 K], h2[K]      the fields of particle ids[c]
 *   offsets[K + 1], indices[*n_indices]      the candidate rows of the participants in COMPACT ids, rows and entries in their
 *                                            original order; a participant that is no donor has an empty row
 * participants_capacity counts the entries of the per-participant arrays (offsets: participants_capacity + 1), indices_capacity those
 * of indices.  A per-participant array given with participants_capacity < K, or indices given with indices_capacity < *n_indices ->
 * SPH_ERR_INVALID_ARGUMENT with both counts set and no problem open.
 * Refusals are those of sph_download_partner_candidates: a slab context -> SPH_ERR_UNSUPPORTED; no lists and nothing to build them
 * from, kind outside {0, 1}, params or ap NULL -> SPH_ERR_INVALID_ARGUMENT; a poisoned context -> SPH_ERR_POISONED.
 * The call changes nothing of the simulation state.
 *
 * On success the library keeps ids and kind on the device as THE OPEN PROBLEM of the context.  It is closed by everything that drops
 * the lists (sph_step, sph_upload, sph_upload_field of position or mass, sph_apply_edits, sph_merge_particles, sph_split_particles,
 * sph_set_math_policy), by the next sph_download_partner_problem (which replaces it, or closes it when it fails) and by the apply
 * call that consumes it. */
int sph_download_partner_problem(sph_ctx* ctx, int kind, const sph_params* params, const sph_adapt_params* ap, uint32_t* ids, uint8_t* size_class,
                                 float* mass, float* level_estimation, float* position, float* h2, uint32_t* offsets, uint64_t participants_capacity,
                                 uint32_t* indices, uint64_t indices_capacity, uint64_t* n_participants, uint64_t* n_indices);

/* sph_share_particles / sph_merge_particles from the decisions on the open problem: partner_c[k] holds SPH_MERGE_PARTNER_AVAILABLE,
 * SPH_MERGE_PARTNER_DELETE or a compact id < k, counter_c[k] the merge counters.  The two arrays (6 bytes per participant) are
 * uploaded and expanded on the device into merge_partner / merge_counter of the whole vector -- AVAILABLE / 0 for everything that is
 * no participant, compact ids mapped through ids -- and the apply that follows is that of sph_share_particles / sph_merge_particles
 * on those arrays: the resulting state is the same bit for bit.
 * SPH_ERR_INVALID_ARGUMENT, before anything on the device is modified and with the problem left open: no open problem of that kind
 * (share: kind 0, merge: kind 1), k != K, partner_c or counter_c NULL with k > 0, an id that is neither a sentinel nor < k.
 * A slab context -> SPH_ERR_UNSUPPORTED; a poisoned one -> SPH_ERR_POISONED.  The problem is consumed by a call that passes those checks. */
int sph_share_particles_compact(sph_ctx* ctx, const sph_params* params, const sph_adapt_params* ap, uint64_t k, const uint32_t* partner_c,
                                const uint16_t* counter_c);
int sph_merge_particles_compact(sph_ctx* ctx, const sph_params* params, const sph_adapt_params* ap, uint64_t k, const uint32_t* partner_c,
                                const uint16_t* counter_c);

#ifdef __cplusplus
}
#endif

#endif /* SPH_PARTNER_PROBLEM_H */
