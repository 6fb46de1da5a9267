/*
 * sph_slab_probe.h -- the probe sets of sph_probe.h on SLAB contexts: gauges and tracers from every rank.  Every rank scatters the
 * particles it owns onto its replica of the point set, packs the points it touched into a COMPACT layer of int64 sums, and the layers
 * are ADDED per point.  sph_probe_sample and sph_probe_advect themselves keep refusing a slab context (one rank holds a slab of the
 * particles).
 *
 * Why it decomposes.  sph_probe.h's raw words are sums of 64-bit integers, one term per (particle, point) pair; integer addition is
 * associative and commutative, and every particle is owned by exactly one rank.  So the per-point sum of the ranks' words is BIT FOR
 * BIT what one context holding the same particles gives: it depends neither on the cuts nor on the rank count nor on the order of the
 * layers.  What is a property of the WHOLE vector, and therefore needs an agreement, are the automatic exponents and the data
 * preconditions -- the agreement sph_slab_sample.h settles for lattices, reused here: the same 32-byte verdict, the same fold.
 *
 * A REPLICA.  sph_probe_set_create, _upload, _download, _size, _bins and _destroy work on a slab context as they are.  Every rank holds
 * a set with THE SAME POINTS IN THE SAME ORDER; a layer speaks of points by their index in that order.  That the replicas' coordinates
 * agree is the caller's contract: the library compares their sizes only.
 *
 * A separate header from sph_ffi.h, like sph_probe.h: product library only.  sph_probe_params, sph_probe_advect_params, sph_probe_info,
 * sph_slab_sample_words and every formula of sph_sample.h and sph_probe.h are reused unchanged; status codes are those of sph_ffi.h.
 * tests/slab_probe_reference.py restates the layer and the compose in numpy, tests/probe_reference.py the sums.
 *
 * RANGE (sph_slab_probe_range; local to the rank, no communication)
 *   reads       the rank's owned slots (ghosts are skipped), the channels and the volume of `pp`; no probe set
 *   one pass    sph_slab_sample_range's: the preconditions of sph_sample.h and max |a_j| per channel, into the same
 *               sph_slab_sample_words (first_bad: the smallest offending GLOBAL id << 8 | reason, all ones: none)
 *   The call returns SPH_OK whatever the data says: the verdict belongs to the fold.
 *
 * FOLD (sph_probe_fold_words; plain host arithmetic, no context, no device)
 *   reads       the n ranks' words and the exponents in pp_io
 *   The rule of sph_sample_fold_words (one implementation serves both): the unsigned minimum of first_bad, the unsigned maxima of
 *   max_bits; an offender gives SPH_ERR_INVALID_ARGUMENT and in `msg` the sentence sph_probe_sample leaves for the same offender
 *   ("... (particle i=<global id>)"), truncated to msg_bytes - 1 characters and always terminated (msg may be NULL); otherwise every
 *   SPH_SAMPLE_AUTO_EXPONENT in pp_io is replaced by the exponent of the whole vector ("needs the exponent" above
 *   SPH_SAMPLE_MAX_EXPONENT); explicit exponents are left alone.  For a tracer step the caller folds a sph_probe_params that holds the
 *   two velocity channels {SPH_F_VELOCITY, 0, exponent_x}, {SPH_F_VELOCITY, 1, exponent_y} and the advect's volume -- what
 *   sph_probe_advect builds internally -- and copies the two exponents into its sph_probe_advect_params.
 *
 * LAYER (sph_slab_probe_layer; local to the rank, no communication; explicit exponents only: the fold comes first)
 *   reads       the rank's owned slots and the set's points; a ghost slot adds nothing.  No data precondition is checked here
 *   scatter     sph_probe.h's, onto the set's binned points: the predicate q < 1 alone decides which pairs add
 *   pack        on the device: the ENTRIES are the points touched by at least one owned particle (q < 1), also where all of their words
 *               are 0.  n_entries uint32 indices, strictly ascending, in the caller's point order; then (C+1) x n_entries int64 words,
 *               plane-major, plane 0 = the weight: word (plane, e) is the sum of the rank's owned particles' terms at point indices[e]
 *   storage     the layer stays with the SET until the next layer call on that set or its destroy.  It is a read-out, not simulation
 *               state: a step does not drop it, and the call changes nothing a step reads
 *   info        sph_slab_probe_layer_info: n_entries, the exponents used, the RANK's n_touching and n_pairs -- over the ranks these add
 *               up to the whole vector's.  May be NULL.
 *   sph_slab_probe_layer_download copies the kept layer to the host: capacity_entries >= n_entries; with n_entries == 0 it succeeds and
 *   writes nothing (the buffers may be NULL).
 *
 * COMPOSE (sph_probe_compose; the context that owns `set`, plain or slab -- it reads no particle, only `pp`, the set's size and the
 * host layers)
 *   clears (C+1) x n_points planes, adds every layer's entries on the device (indices within one layer are distinct: one launch per
 *   layer, in stream order, no atomics), then sph_probe_sample's resolved output: normalise, min_weight and fill as there, with pp's
 *   exponents, which must be explicit.  indices[k] / words[k] are HOST pointers to layer k as the download gives it; they may be NULL
 *   iff n_entries[k] is 0; n_layers may be 0 (all-zero planes).  Every layer is validated on the host before anything is added.
 *   info->n_touched_points: the points present in at least one layer; n_touching and n_pairs are left 0 (the caller adds the ranks').
 *
 * COMPOSE AND MOVE (sph_probe_compose_advect; the tracer step of a replica)
 *   stages and sums the same way with 3 planes -- weight, x, y -- and ap's two explicit exponents, then moves the set's own points:
 *   the arithmetic of sph_probe_advect, line for line (one kernel serves both).  The set re-bins itself at its next use.  Every rank
 *   calls this with the same layers, in any order: the move is a deterministic per-point function of integer sums, so EVERY REPLICA
 *   ENDS WITH THE SAME POINTS BIT FOR BIT.  n_moved and n_stalled as sph_probe_advect fills them.
 *
 * GROUP CALLS (sph_group_probe_sample, sph_group_probe_advect; the n slab contexts of one process that sph_group_step steps; sets[i] is
 * a live set of ctxs[i]; all sets hold the same number of points; automatic exponents are allowed)
 *   When all members sit on ONE device nothing but the words and the result crosses the bus: every member's range pass reduces into
 *   member 0's words, one synchronisation, the host takes the exponents or refuses; every member scatters its owned slots with 64-bit
 *   atomics straight into member 0's planes; member 0 resolves and copies out, or every member moves its own set from those planes.
 *   When the members do not share a device the call runs the per-rank calls above through the host: ranges, fold, layers, downloads,
 *   compose on member 0 (compose-and-move on every member).
 *   (Only the one-device branch has run anywhere: the project's machines have one GPU.)
 *   info: the exponents used, the summed n_touching and n_pairs, n_touched_points, member 0's n_moved / n_stalled and bin geometry.
 *   After sph_group_probe_advect every member's set holds the same points.  Whichever member refuses, the sentence is left in member
 *   0's sph_last_error.
 *
 * REFUSALS (taken before anything is launched, except the data preconditions)
 *   SPH_ERR_UNSUPPORTED        sph_slab_probe_range / _layer / _layer_download on a plain context, a plain context as a group member
 *                              (sph_probe_sample samples a plain context)
 *   SPH_ERR_POISONED           a poisoned context (range, layer, group calls)
 *   SPH_ERR_INVALID_ARGUMENT   every channel, volume, exponent and buffer refusal of sph_probe_sample, unchanged: an unknown field, a
 *                              component the field does not have, more than SPH_SAMPLE_MAX_CHANNELS channels, an unknown volume mode,
 *                              an exponent outside the range, (C+1) * n_points * 8 above SPH_SAMPLE_MAX_RAW_BYTES, a short output buffer;
 *                              every dt and min_weight refusal of sph_probe_advect, with its text (compose-and-move, group advect);
 *                              SPH_SAMPLE_AUTO_EXPONENT given to the layer call, to compose or to compose-and-move ("the fold comes first");
 *                              a data precondition (fold, group calls), naming the smallest offending global id;
 *                              a handle that is not a live set of the context it is used with;
 *                              a layer, named by its number, whose indices are not strictly ascending, or hold an index >= n_points,
 *                              or whose pointers are NULL while n_entries[k] > 0; n_layers < 0, or layers without their arrays;
 *                              a download without a layer or with capacity_entries below n_entries;
 *                              sets of different sizes in a group call; null parameters or outputs;
 *                              n < 1, null words or null pp_io in the fold; n < 1 in a group call
 *   SPH_ERR_DEVICE
 * A short `msg` buffer truncates and does not fail.  After a refusal the output buffers are unspecified; no refused call poisons a
 * context, moves a point, or changes anything a step reads.  Every launch runs on the stream of the context it works for.
 */
#ifndef SPH_SLAB_PROBE_H
#define SPH_SLAB_PROBE_H

#include <stdint.h>

#include "sph_probe.h"
#include "sph_slab_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sph_slab_probe_layer_info {
    int32_t  exponents[SPH_SAMPLE_MAX_CHANNELS];   /* e_c as used (0 beyond the call's channels) */
    uint64_t n_entries;                            /* points touched by at least one owned particle */
    uint64_t n_touching;                           /* owned particles that touch at least one point */
    uint64_t n_pairs;                              /* (owned particle, point) pairs with q < 1 */
} sph_slab_probe_layer_info;

SPH_PROBE_STATIC_ASSERT(sizeof(sph_slab_probe_layer_info) == 48, "sph_slab_probe_layer_info");
SPH_PROBE_STATIC_ASSERT(sizeof(sph_slab_sample_words) == 32, "sph_slab_sample_words");

/* local to the rank */
int sph_slab_probe_range(sph_ctx* ctx, const sph_params* params, const sph_probe_params* pp, sph_slab_sample_words* words_out);
int sph_slab_probe_layer(sph_ctx* ctx, const sph_params* params, sph_probe_set* set, const sph_probe_params* pp, sph_slab_probe_layer_info* layer_info_out);
/* indices_out: n_entries uint32; words_out: (C+1) x n_entries int64, plane-major */
int sph_slab_probe_layer_download(sph_ctx* ctx, sph_probe_set* set, uint32_t* indices_out, int64_t* words_out, uint64_t capacity_entries);

/* no context: the ranks' words -> the exponents of the whole vector in pp_io, or the refusal's sentence in msg */
int sph_probe_fold_words(int n, const sph_slab_sample_words* words, sph_probe_params* pp_io, char* msg, uint64_t msg_bytes);

/* the context that owns `set` (plain or slab); indices[k] / words[k] are HOST pointers, NULL iff n_entries[k] is 0; n_layers may be 0 */
int sph_probe_compose(sph_ctx* ctx, sph_probe_set* set, const sph_probe_params* pp, int n_layers, const uint64_t* n_entries, const uint32_t* const* indices,
                      const int64_t* const* words, float* values_out, uint64_t values_bytes, int64_t* raw_out, uint64_t raw_bytes, sph_probe_info* info);
int sph_probe_compose_advect(sph_ctx* ctx, sph_probe_set* set, const sph_probe_advect_params* ap, int n_layers, const uint64_t* n_entries,
                             const uint32_t* const* indices, const int64_t* const* words, sph_probe_info* info);

/* the n slab contexts of one process that sph_group_step steps; sets[i] belongs to ctxs[i] */
int sph_group_probe_sample(sph_ctx** ctxs, int n, const sph_params* params, sph_probe_set* const* sets, const sph_probe_params* pp, float* values_out,
                           uint64_t values_bytes, int64_t* raw_out, uint64_t raw_bytes, sph_probe_info* info);
int sph_group_probe_advect(sph_ctx** ctxs, int n, const sph_params* params, sph_probe_set* const* sets, const sph_probe_advect_params* ap, sph_probe_info* info);

#ifdef __cplusplus
}
#endif

#endif /* SPH_SLAB_PROBE_H */
