/*
 * sph_candidates.h -- the partner searches' candidates, filtered on the device.
 *
 * find_share_partner_sequential (adaptivity/particle_sharing.rs:14-117) and find_merge_partner_sequential
 * (particle_merging.rs:16-125) stay host code: a sequential greedy loop whose result depends on its order.  But of the
 * neighbour lists it iterates it reads only the rows of the donors (Large particles when sharing, TooSmall ones when merging),
 * and the first two tests on a neighbour j -- its size class (particle_sharing.rs:50-58, particle_merging.rs:57-69) and its
 * distance (particle_sharing.rs:61-65, particle_merging.rs:72-76) -- read nothing the loop writes: class, mass, position and
 * h2 are constant while it runs.  sph_download_partner_candidates evaluates both where the lists and the fields already are
 * and hands the host only the j that pass, in list order.  The host's loop runs UNCHANGED on that CSR (the two tests are
 * idempotent: a j that passed here passes again there; the rows keep their order) and takes the same decisions;
 * validate_share_partners / validate_merge_partners count merge_partner[row] == i and hold on the filtered rows as well.
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only.
 * Status codes are those of sph_ffi.h.  Neither call changes the simulation state; every launch runs on the context's stream.
 */
#ifndef SPH_CANDIDATES_H
#define SPH_CANDIDATES_H

#include <stdint.h>

#include "sph_ffi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind: 0 share, 1 merge (as sph_host_find_partners).
 * CSR over ALL particles in host order: offsets[n + 1], indices[*n_indices].
 * Row i is empty unless particle_size_class[i] is the donor class of `kind` (share: Large, merge: TooSmall).
 * A donor row holds, in the order of row i of sph_download_neighbors, every j != i that passes
 *   - the class test of `kind` with the allow_* flags of `ap` (merge: including
 *     allow_merge_on_size_difference && mass[j] > 5 * mass[i], which overrides a failed class test), and
 *   - the distance test  dx*dx + dy*dy > max_dist*max_dist  -> rejected,
 *     max_dist = ((h2[i] + h2[j]) * 0.5f) * max_{share,merge}_distance.
 * Every operation is one IEEE f32 operation in that order, without contraction, under both math policies.
 *
 * The LISTS are those of the last step -- the rows sph_download_neighbors returns, the extended lists of the advected positions
 * with level_estimation_after_advection -- and stay usable across sph_share_particles, which renumbers nothing (the merge search
 * of single_step_adaptivity runs after share_particles on the step's lists, simulation.rs:2732-2796): the library keeps their
 * CSR on the device from the first export of a step (this call or sph_download_neighbors) until sph_step, sph_upload,
 * sph_upload_field of position or mass, sph_apply_edits, sph_merge_particles, sph_split_particles or sph_set_math_policy.
 * The FIELD VALUES are those sph_download would return at the moment of the call: the class of the last sph_classify, the
 * current mass, position and h2.
 *
 * Same two-call convention as sph_download_neighbors: offsets and / or indices may be NULL; *n_indices is always set;
 * indices_capacity too small -> SPH_ERR_INVALID_ARGUMENT with *n_indices set.  No lists and nothing to build them from
 * (before the first step, after one of the calls above) -> SPH_ERR_INVALID_ARGUMENT.  A slab context -> SPH_ERR_UNSUPPORTED. */
int sph_download_partner_candidates(sph_ctx* ctx, int kind, const sph_params* params, const sph_adapt_params* ap,
                                    uint32_t* offsets, uint32_t* indices, uint64_t indices_capacity, uint64_t* n_indices);

/* Sum of the particle masses in f64, reduced on the device in a fixed order (two calls on the same state: same bits).
 * A slab context -> SPH_ERR_UNSUPPORTED. */
int sph_sum_mass(sph_ctx* ctx, double* total);

#ifdef __cplusplus
}
#endif

#endif /* SPH_CANDIDATES_H */
