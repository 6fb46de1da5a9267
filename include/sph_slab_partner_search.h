/*
 * sph_slab_partner_search.h -- the partner searches of a SLAB GROUP on the device: merge, solve, hand over, apply.
 *
 * sph_slab_partner_problem.h packs every rank's LOCAL problem on its device; the host then brings the problems down, merges them by
 * global id (distributed.merge_slab_partner_problems), runs the sequential search and sends 10 B x K back up to every rank.
 * sph_partner_search.h solves a compact problem on the device in its exact parallel schedule, but refuses a slab context.  These entry
 * points join the two for the n contexts of ONE process that sph_group_step steps as ranks 0 .. n-1 (the loopback transport, on one
 * device or on n): the local problems are merged on the device of one member -- the ROOT --, solved and validated there with the
 * solver of sph_partner_search.h, and the K decisions go to every member device to device.  Only the info struct crosses the host bus.
 *
 * THE MERGED PROBLEM, as it sits on the root (sph_group_download_merged_partner_problem returns it), is the problem
 * distributed.merge_slab_partner_problems makes of the same local problems, array for array and bit for bit:
 *   ids[K]                the union of the ranks' participants, global ids ascending; the position in it is the COMPACT id
 *   size_class .. h2      the five decision fields, from whichever rank reports the participant
 *   offsets[K + 1]        the candidate row of every participant: its owner's row, empty for one that is nobody's donor
 *   indices               the entries in compact ids, in the order of the owner's row
 * How it is made (one thread per element, on the root's stream):
 *   staging   every member's packed arrays are copied to the root's device (a peer copy between two devices, a device-to-device copy
 *             on one); the streams are ordered with events; no kernel reads another device's memory
 *   mark      a flag word per global id, zeroed; every reported id stores 1
 *   scan      rank[g] = the compact id of g, K = the total, ids[rank[g]] = g
 *   fields    one launch per member, in rank order: a participant seen for the first time writes its five fields, one seen before
 *             compares them bit for bit; an owned one writes its row's length
 *   rows      scan of the lengths -> offsets; every owner copies its row, the entries relabelled through rank[]
 * A particle that two ranks report with different bits (a stale ghost), one that two ranks own, an id >= the group's particle count,
 * an entry that names no participant, offsets that do not describe the reported entries: the merge's error word is set, nothing is
 * picked, the call fails with SPH_ERR_DEVICE.  Every index a kernel forms is checked against the counts the host read.
 *
 * THE OPEN SOLUTION of the group: ids[K], partner_c[K] (SPH_MERGE_PARTNER_AVAILABLE, SPH_MERGE_PARTNER_DELETE or a compact id < K)
 * and counter_c[K] on EVERY member's device.  It is open on a member exactly while the problem that member prepared for it is (the
 * VALIDITY paragraph of sph_slab_partner_problem.h: closed by sph_step / sph_group_step, sph_upload, sph_upload_field of position,
 * mass or particle ids, sph_apply_edits, sph_set_math_policy, a merge or split that renumbered the vector, a later
 * sph_slab_candidates_prepare or sph_slab_partner_problem_prepare); sph_group_adapt_device consumes it -- a share leaves the prepared
 * rows open, the solution not.  The entry points below need it open on every member.
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only.  Status codes are those of sph_ffi.h.
 * Refusals, before anything is launched: a plain context among ctxs -> SPH_ERR_UNSUPPORTED; a poisoned member -> SPH_ERR_POISONED;
 * SPH_ERR_INVALID_ARGUMENT for ctxs NULL, n < 1, a NULL entry, contexts that are not configured as ranks 0 .. n-1 of n, and what each
 * entry point names below.
 */
#ifndef SPH_SLAB_PARTNER_SEARCH_H
#define SPH_SLAB_PARTNER_SEARCH_H

#include <stdint.h>

#include "sph_ffi.h"
#include "sph_partner_search.h"
#include "sph_slab_partner_problem.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kind: 0 share, 1 merge.  Runs sph_group_slab_partner_problem_prepare(ctxs, n, kind, params, ap, ..) unchanged -- the same rows, the
 * same local problems, the same three count arrays (n entries each, each may be NULL) --, merges the local problems on the device of
 * member `root`, solves there (wide_threshold: as in sph_find_partners_device; the decisions do not depend on it) and validates there
 * (validate_share_partners / validate_merge_partners), and copies ids, partner_c and counter_c to every member's device.  Afterwards
 * every member holds THE OPEN SOLUTION of the group.  *info describes the merged problem and its search, as sph_find_partners_device
 * describes a plain context's.  Nothing of the simulation state is written (the prepare refreshes ghost records, as it always does).
 * K == 0 (no rank has a donor with a candidate): success, *info all zero, an open solution without decisions.
 * SPH_ERR_INVALID_ARGUMENT: root outside 0 .. n-1; params, ap or info NULL; kind outside {0, 1}; what the prepare refuses (no step
 * before the call, no lists and nothing to build them from); the ranks' candidate counts add up to 2^32 or more.
 * SPH_ERR_DEVICE: the merge's error word (above), or the solver's (sph_partner_search.h).  No solution is open then; the prepared local
 * problems stay, the group can step. */
int sph_group_find_partners_device(sph_ctx** ctxs, int n, int kind, const sph_params* params, const sph_adapt_params* ap, uint32_t wide_threshold,
                                   int root, sph_partner_search_info* info, uint64_t* n_participants, uint64_t* n_owned_participants,
                                   uint64_t* n_indices);

/* Inspection only; leaves the solution open.  The merged problem as it sits on the root, in the layout and the two-call size convention
 * of sph_download_partner_problem: ids[K], size_class[K], mass[K], level_estimation[K], position[2 K], h2[K], offsets[K + 1],
 * indices[*n_indices] in compact ids; every pointer may be NULL; the two counts are set whenever a solution is open, also when a
 * capacity is then refused (a per-participant array or offsets with participants_capacity < K, indices with indices_capacity <
 * *n_indices -> SPH_ERR_INVALID_ARGUMENT).  No open solution -> SPH_ERR_INVALID_ARGUMENT, the counts are 0. */
int sph_group_download_merged_partner_problem(sph_ctx** ctxs, int n, uint32_t* ids, uint8_t* size_class, float* mass, float* level_estimation,
                                              float* position, float* h2, uint32_t* offsets, uint64_t participants_capacity, uint32_t* indices,
                                              uint64_t indices_capacity, uint64_t* n_participants, uint64_t* n_indices);

/* Inspection only; leaves the solution open.  The copy of the decisions that member `from_member` holds (a hand-over that went wrong
 * shows up here, not in the root's arrays).  Every array pointer may be NULL.
 * SPH_ERR_INVALID_ARGUMENT: from_member outside 0 .. n-1, no open solution, k != K. */
int sph_group_download_partner_decisions(sph_ctx** ctxs, int n, int from_member, uint64_t k, uint32_t* ids, uint32_t* partner_c,
                                         uint16_t* counter_c);

/* op: 0 share, 1 merge.  Applies the open solution exactly as sph_group_adapt_compact(ctxs, n, op, params, ap, K, ids, partner_c,
 * counter_c) applies the same K decisions -- every member expands its own copy on its own device, nothing is uploaded -- and consumes
 * it on every member, whatever the apply returns.  With K == 0 that is the apply of all-AVAILABLE arrays.
 * SPH_ERR_INVALID_ARGUMENT, before anything on the device is modified: params or ap NULL, op outside {0, 1}, no open solution on some
 * member, a solution of the other kind.  The other refusals are those of sph_group_adapt. */
int sph_group_adapt_device(sph_ctx** ctxs, int n, int op, const sph_params* params, const sph_adapt_params* ap);

#ifdef __cplusplus
}
#endif

#endif /* SPH_SLAB_PARTNER_SEARCH_H */
