/*
 * sph_rank_partner_search.h -- the partner searches on the device with ONE PROCESS (or thread) PER RANK: relay, merge, solve, relay, apply.
 *
 * sph_slab_partner_search.h merges, solves and applies for the n contexts of ONE process (the loopback transport).  These entry points do
 * the same for a slab context that calls sph_step for itself over its own transport -- RCCL, the thread group, the shared-memory segment,
 * the peer-mapped push transport --, every rank making the same call, as it makes every other collective call of a slab context:
 *
 *   prepare    sph_slab_partner_problem_prepare, unchanged: the rank's LOCAL problem in its packed arrays, the entries in global ids
 *   table      every rank learns every rank's (participants, owned participants, entries, particles, message limit): one all-reduce of
 *              host words, each rank filling only its own five words of a zeroed row.  All that follows is derived from this table,
 *              alike on every rank
 *   blob       ONE launch packs the local problem into one message, every piece at a multiple of 16 bytes: ids[K], size_class[K], mass[K],
 *              level_estimation[K], position[2 K], h2[K], offsets[Ko + 1], the T entries.  A rank without a participant has no blob
 *   gather     THE RELAY (below) towards the root: afterwards the root holds all blobs in rank order in one device buffer; it does not
 *              unpack them -- the merge reads the pieces where they lie
 *   merge      the merge of sph_slab_partner_search.h (one definition serves both headers; only the staging in front of it differs): the
 *              same merged problem, the same error word and texts.  The mark kernel is launched once per blob
 *   solve      the solver of sph_partner_search.h on the root, validated there
 *   broadcast  the relay run outwards, twice: a 256-byte header -- the info struct, K, the entries' total, the root's status and its error
 *              text --, then ids[K], partner_c[K], counter_c[K], which every rank copies into its open solution
 *
 * THE RELAY.  The ranks are a row; sph_step's exchange moves device buffers between x-neighbours on every transport, and nothing else is
 * used.  Round t = 1 .. max(root, n - 1 - root): a blob that started d hops from the root has moved min(t, d) hops; a rank left of the
 * root sends to its right neighbour what it received in the round before (in round 1: its own blob), the mirror image holds on the right,
 * the root receives blob root - t and blob root + t.  A round is cut into sub-rounds of at most chunk_bytes = min(the transports' message
 * limit -- the smallest in the table; 2^30 where there is none --, relay_bytes) rounded down to a multiple of 16; their number follows
 * from the table -- the largest blob under way in that round --, so every rank runs the same sub-rounds and both ends of a pair name the same byte count in each, zero for an idle side.  The
 * broadcast is the same schedule in the other direction.  sph_relay_plan returns the schedule; the relay itself is driven by it.
 *
 * THE OPEN SOLUTION is the one of sph_slab_partner_search.h, on this rank: K decisions in the rank's own device buffers, open exactly while
 * the problem the rank prepared for it is (closed by sph_step, sph_upload, sph_upload_field of position, mass or particle ids,
 * sph_apply_edits, sph_set_math_policy, a merge or split that renumbered the vector, a later prepare); sph_slab_adapt_device consumes it.
 *
 * COLLECTIVE: every rank of the decomposition calls sph_slab_find_partners_device / sph_slab_adapt_device with the same arguments behind
 * the same step.  A refusal named below is taken by every rank alike, before anything is queued, and leaves the transport usable.  A
 * failure on the root inside merge or solve travels in the broadcast header: every rank returns the root's SPH_ERR_DEVICE with the root's
 * text, no solution is open anywhere, the transport stays usable.  Any other failure of one rank abandons the transport, so that the
 * others' next collective reports it instead of waiting (thread and shared-memory transports; THE COLLECTIVE RULE).
 *
 * WHAT HAS RUN WHERE: the relay with peers has run over the thread transport, the shared-memory transport and the peer-mapped push
 * transport, all ranks on ONE device.  Over RCCL it has run with one rank only (an empty relay); hipIpc inboxes between two devices have
 * never carried it.
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only.  Status codes are those of sph_ffi.h.
 */
#ifndef SPH_RANK_PARTNER_SEARCH_H
#define SPH_RANK_PARTNER_SEARCH_H

#include <stdint.h>

#include "sph_ffi.h"
#include "sph_partner_search.h"
#include "sph_slab_partner_problem.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one direction of one side of a sub-round: `bytes` bytes of rank `origin`'s blob from byte `offset` of it on; bytes == 0: nothing */
typedef struct sph_relay_leg {
    uint64_t origin, offset, bytes;
} sph_relay_leg;
/* what one rank does in one sub-round; [0]: its left neighbour, [1]: its right neighbour */
typedef struct sph_relay_step {
    uint32_t round, sub_round;
    sph_relay_leg send[2], recv[2];
} sph_relay_step;

/* The relay's schedule for `rank` of `n_ranks`; needs no device and no context.  outwards == 0: the gather of the blobs of
 * bytes_of_rank[0 .. n_ranks) bytes to `root`; outwards != 0: the broadcast of the root's blob (bytes_of_rank[root]; the other entries
 * are not read).  Every sub-round of every round is listed, in order, also those in which this rank is idle (all legs zero): every rank
 * gets the same *n_steps.  Two-call size convention: steps == NULL sets *n_steps only; otherwise steps_capacity < *n_steps ->
 * SPH_ERR_INVALID_ARGUMENT with *n_steps set.  SPH_ERR_INVALID_ARGUMENT also for n_ranks < 1, root or rank outside 0 .. n_ranks-1,
 * bytes_of_rank or n_steps NULL, chunk_bytes == 0. */
int sph_relay_plan(int n_ranks, int root, int rank, int outwards, const uint64_t* bytes_of_rank, uint64_t chunk_bytes, sph_relay_step* steps,
                   uint64_t steps_capacity, uint64_t* n_steps);

/* kind: 0 share, 1 merge.  Runs sph_slab_partner_problem_prepare(ctx, kind, params, ap, ..) unchanged -- the three counts are this rank's,
 * each pointer may be NULL --, then table, blob, gather, merge and solve on `root`, broadcast (above).  Afterwards this rank holds THE OPEN
 * SOLUTION; *info is the root's on every rank.  wide_threshold: as in sph_find_partners_device.  relay_bytes: the most bytes of one relay
 * message; 0: the transport's limit (one message per blob where there is none).
 * K == 0 (the table says no rank has a participant): no relay, success, *info all zero, an open solution without decisions.
 * Before anything is queued: a plain context -> SPH_ERR_UNSUPPORTED (it takes sph_find_partners_device); a poisoned one ->
 * SPH_ERR_POISONED; SPH_ERR_INVALID_ARGUMENT for a member of a loopback group (it takes sph_group_find_partners_device), root outside
 * 0 .. nranks-1, params, ap or info NULL, kind outside {0, 1}, 0 < relay_bytes < 4096, more than 819 ranks (the table's 4096 words), and
 * what the prepare refuses (no step before the call, no lists and nothing to build them from: agreed between the ranks).
 * SPH_ERR_INVALID_ARGUMENT on every rank alike when the table adds up to 2^32 entries or more.
 * SPH_ERR_DEVICE: the merge's error word or the solver's on the root, on every rank, with the root's text. */
int sph_slab_find_partners_device(sph_ctx* ctx, int kind, const sph_params* params, const sph_adapt_params* ap, uint32_t wide_threshold, int root,
                                  uint64_t relay_bytes, sph_partner_search_info* info, uint64_t* n_participants, uint64_t* n_owned_participants,
                                  uint64_t* n_indices);

/* op: 0 share, 1 merge.  Applies this rank's open solution exactly as sph_slab_share_particles_compact / sph_slab_merge_particles_compact
 * apply the same K decisions -- nothing is uploaded -- and consumes it, whatever the apply returns.  Collective like those.  The ranks
 * first agree (one all-reduce of a host word) that every one of them holds an open solution of kind `op`: a solution that was closed on
 * one rank only -- an upload there -- makes every rank refuse, and nobody waits in the apply for a rank that left.
 * SPH_ERR_INVALID_ARGUMENT, before anything on the device is modified and leaving an open solution open: params or ap NULL, op outside
 * {0, 1}, no open solution on some rank, a solution of the other kind, a member of a loopback group (sph_group_adapt_device).  Plain
 * and poisoned contexts: as above. */
int sph_slab_adapt_device(sph_ctx* ctx, int op, const sph_params* params, const sph_adapt_params* ap);

/* Inspection only, local; leaves the solution open.  This rank's copy of the decisions.  Every array pointer may be NULL.
 * SPH_ERR_INVALID_ARGUMENT: no open solution, k != K. */
int sph_slab_download_partner_decisions(sph_ctx* ctx, uint64_t k, uint32_t* ids, uint32_t* partner_c, uint16_t* counter_c);

/* Inspection only, local; leaves the solution open.  The merged problem as it sits on the root, in the layout and the two-call size
 * convention of sph_group_download_merged_partner_problem.  SPH_ERR_INVALID_ARGUMENT on a rank that is not the solution's root, without
 * an open solution (the counts are 0 then), and for a capacity that is too small (the counts are set). */
int sph_slab_download_merged_partner_problem(sph_ctx* ctx, uint32_t* ids, uint8_t* size_class, float* mass, float* level_estimation, float* position,
                                             float* h2, uint32_t* offsets, uint64_t participants_capacity, uint32_t* indices,
                                             uint64_t indices_capacity, uint64_t* n_participants, uint64_t* n_indices);

/* Inspection only, local; leaves the solution open.  What the relays of the open solution's search moved: bytes_of_rank[*n_ranks] the
 * blobs of the gather (two-call size convention: NULL sets *n_ranks only), *chunk_bytes the sub-round size, *header_bytes and
 * *decisions_bytes the two broadcasts (0 and 0 with K == 0: nothing was relayed), *bytes_sent / *bytes_received what this rank passed to
 * and took from its neighbours in them -- the sums sph_relay_plan gives for the same sizes.  Every pointer may be NULL.
 * SPH_ERR_INVALID_ARGUMENT: no open solution, capacity < *n_ranks. */
int sph_slab_relay_sizes(sph_ctx* ctx, uint64_t* bytes_of_rank, uint64_t capacity, uint64_t* n_ranks, uint64_t* chunk_bytes, uint64_t* header_bytes,
                         uint64_t* decisions_bytes, uint64_t* bytes_sent, uint64_t* bytes_received);

#ifdef __cplusplus
}
#endif

#endif /* SPH_RANK_PARTNER_SEARCH_H */
