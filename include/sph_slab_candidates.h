/*
 * sph_slab_candidates.h -- the partner searches' candidates on a SLAB context, filtered on the device, in global particle ids.
 *
 * sph_candidates.h and sph_partner_problem.h refuse a slab context (SPH_ERR_UNSUPPORTED): their rows are host indices of ONE
 * vector.  These entry points are the slab form of the first: every rank filters the rows of the particles it owns and hands the
 * host a few candidates per donor instead of every neighbour list; the host assembles the ranks' rows by id and runs the same
 * sequential search on them (find_share_partner_sequential, adaptivity/particle_sharing.rs:14-117; find_merge_partner_sequential,
 * particle_merging.rs:16-125).
 *
 * THE ROWS mirror the slab contract of sph_download_neighbors: one row per OWNED particle in the order of
 * sph_download(SPH_F_PARTICLE_ID); the entries are global particle ids.  A row is empty unless its particle's size class is the
 * donor class of `kind` (0 share: Large, 1 merge: TooSmall).  A donor row holds, in order, every entry j != i of the row
 * sph_download_neighbors returns for that particle on that rank that passes
 *   - the class test of `kind` with the allow_* flags of `ap` (merge: including allow_merge_on_size_difference &&
 *     mass[j] > 5 * mass[i], which overrides a failed class test), and
 *   - the distance test  dx*dx + dy*dy > max_dist*max_dist  -> rejected,
 *     max_dist = ((h2[i] + h2[j]) * 0.5f) * max_{share,merge}_distance.
 * Every operation is one IEEE f32 operation in that order, without contraction, under both math policies.  With
 * level_estimation_after_advection the lists are the extended lists of the advected positions, as sph_download_neighbors has them.
 *
 * THE LISTS are those of the last step.  The first prepare behind a step builds their CSR on the device (slot indices, no host
 * loop); it cannot be built later, because the share's apply on a slab overwrites the pre-step snapshot the lists are rebuilt from.
 * The CSR stays valid across sph_share_particles on the slab (the merge search of single_step_adaptivity runs behind the share on the
 * step's lists, simulation.rs:2732-2796) and is dropped by sph_step / sph_group_step, sph_upload, sph_upload_field of position, mass
 * or particle ids, sph_apply_edits, sph_set_math_policy, and a merge or split apply that renumbered the vector.
 * THE FIELD VALUES are those of the moment of the call.  An owned particle's class is that of the last sph_classify (the caller
 * classifies first, as on a plain context).  A ghost's record and level are refreshed from their owner inside prepare, and its
 * class is computed from them: what sph_classify(params) gives its owner at the call.  Nothing an owned particle holds is written.
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only.  Status codes are those of sph_ffi.h:
 * a plain context -> SPH_ERR_UNSUPPORTED, a poisoned one -> SPH_ERR_POISONED; SPH_ERR_INVALID_ARGUMENT for a kind outside {0, 1},
 * NULL params, no step before the call (or a merge / split apply since), no CSR and nothing to build it from, a download without
 * prepared rows or after they were dropped, a capacity that is too small.
 */
#ifndef SPH_SLAB_CANDIDATES_H
#define SPH_SLAB_CANDIDATES_H

#include <stdint.h>

#include "sph_ffi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* COLLECTIVE through the context's own transport, like sph_share_particles on a slab context: every rank calls it, in the same
 * order, behind the same step.  *n_rows = the rank's owned particles, *n_indices = the entries of its rows.  A failure on one rank
 * ends the call on every rank. */
int sph_slab_candidates_prepare(sph_ctx* ctx, int kind, const sph_params* params, const sph_adapt_params* ap, uint64_t* n_rows,
                                uint64_t* n_indices);
/* The same for the n contexts of ONE process that sph_group_step steps as ranks 0 .. n-1; n_rows[n], n_indices[n]. */
int sph_group_slab_candidates_prepare(sph_ctx** ctxs, int n, int kind, const sph_params* params, const sph_adapt_params* ap,
                                      uint64_t* n_rows, uint64_t* n_indices);
/* Local, no collective: the rows prepared last.  offsets[n_rows + 1] and / or indices may be NULL. */
int sph_slab_candidates_download(sph_ctx* ctx, uint32_t* offsets, uint32_t* indices, uint64_t indices_capacity);
/* Local: the f64 sum of the OWNED particles' masses, reduced on the device in a fixed order (two calls on the same state: same
 * bits).  The host adds the ranks' sums. */
int sph_slab_sum_mass(sph_ctx* ctx, double* total);

#ifdef __cplusplus
}
#endif

#endif /* SPH_SLAB_CANDIDATES_H */
