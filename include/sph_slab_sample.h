/*
 * sph_slab_sample.h -- the planes of sph_sample.h sampled from SLAB contexts: every rank scatters the particles it owns into a layer
 * of int64 sums, the layers are ADDED per sample.  sph_sample_grid and sph_sample_field_range themselves keep refusing a slab context
 * (one rank holds a slab of the particles).
 *
 * Why it decomposes.  sph_sample.h's planes are sums of 64-bit integers, one term per (particle, sample) pair; integer addition is
 * associative and commutative, and every particle is owned by exactly one rank.  So the sum of the ranks' raw planes is BIT FOR BIT
 * the raw plane of one vector that holds the same particles: it depends neither on the cuts nor on the rank count nor on the order
 * of the layers.  What is a property of the WHOLE vector, and therefore needs an agreement, are the automatic exponents and the data
 * preconditions: every rank must scatter with the same exponents, and every rank must refuse with the same message, naming the
 * smallest offending GLOBAL particle id.  Only the verdict words, the bands, the layers and the planes cross the bus: a rank's
 * particles sit in an x-slab, its layer is a band of sample columns, the bands together are about one grid of words, independent
 * of the particle count.
 *
 * A separate header from sph_ffi.h, like sph_sample.h: product library only.  sph_sample_params, sph_sample_channel, sph_sample_info
 * and every formula of sph_sample.h are reused unchanged; status codes are those of sph_ffi.h.  Every operation below is one IEEE f32
 * operation, no contraction; tests/slab_sample_reference.py restates the box, the band and the fold in numpy, tests/sample_reference.py
 * the planes.
 *
 * RANGE (sph_slab_sample_range; local to the rank, no communication)
 *   particles   the rank's owned slots only (before the first step, and behind an upload, every slot is owned; ghosts are skipped)
 *   one pass    sph_sample.h's preconditions -- h finite and > 0; V finite and >= 0; V * norm < 2^20; every a_j of a channel finite and
 *               |a_j| < 2^e_c where `sp` gives the exponent e_c, |a_j| < +inf where it gives SPH_SAMPLE_AUTO_EXPONENT -- and
 *               max |a_j| per channel.  A particle reports its FIRST failing check in that order
 *   verdict     sph_slab_sample_words, 32 bytes:
 *                 first_bad   all ones: no owned particle offends; else (global id << 8) | reason of the SMALLEST offending global id
 *                             (SPH_F_PARTICLE_ID), reason = 1 h, 2 V, 3 V * norm, 4 + c channel c
 *                 max_bits    max |a_j| per channel as float bits (the bit order of non-negative floats is their value order); 0
 *                             beyond n_channels and for a rank without owned particles
 *   The call returns SPH_OK whatever the data says: the verdict belongs to the fold.
 *
 * FOLD (sph_sample_fold_words; plain host arithmetic, no context, no device)
 *   first_bad = the unsigned minimum over the n ranks' words, max_bits[c] = the unsigned maximum.  If a particle offends:
 *   SPH_ERR_INVALID_ARGUMENT, and `msg` receives the sentence sph_sample_grid leaves in sph_last_error for the same offender
 *   ("... (particle i=<global id>)"), truncated to msg_bytes - 1 characters and always terminated (msg may be NULL).  Otherwise every
 *   SPH_SAMPLE_AUTO_EXPONENT in sp_io is replaced by the exponent sph_sample_grid uses for the whole vector: the smallest e with
 *   max < 2^e (0 for a maximum of 0), raised to SPH_SAMPLE_MIN_EXPONENT, refused (SPH_ERR_INVALID_ARGUMENT, "needs the exponent")
 *   above SPH_SAMPLE_MAX_EXPONENT.  Explicit exponents are left alone.  Every rank that folds the same words gets the same sp_io and
 *   the same refusal.
 *
 * LAYER (sph_slab_sample_layer; local to the rank, no communication; explicit exponents only)
 *   particles   the rank's owned slots; a ghost slot has an empty box and adds nothing.  The layer call checks no data precondition:
 *               the range pass and the fold come first
 *   box         of a particle (x, y, h) on the grid (nx, ny, origin, spacing), sph_sample.hip's sample_box as it stands:
 *                   gx = (x - origin_x) / spacing - 0.5f          gy likewise
 *                   rs = (2.f * h) / spacing
 *                   live only if |gx| < 1e30f, |gy| < 1e30f, rs >= 0   (a position or an h that is not finite: no box)
 *                   px = rs + (((|origin_x| + |x|) + (float)nx * spacing) * 4.8e-7f) / spacing + rs * 1e-5f       py likewise with ny
 *                   x0 = max(floor(gx - px) - 1.f, 0.f)           x1 = min(ceil(gx + px) + 1.f, (float)(nx - 1))
 *                   y0, y1 likewise against ny;  live only if x0 <= x1 and y0 <= y1 (the box meets the grid in x AND y)
 *               a superset of the samples the particle touches (the predicate q < 1 of sph_sample.h alone decides membership)
 *   band        sph_sample_band, 16 bytes: [sx0, sx1) = the union of [x0, x1 + 1) over the owned particles whose box is live, n_boxes
 *               their count; nothing to add: sx0 == sx1 == 0, n_boxes == 0
 *   storage     the layer stays in the context: (C+1) planes of ny x (sx1 - sx0) int64 words, plane-major, then row-major, row 0 =
 *               the LOWEST y, word (plane, sy, sx - sx0), until the next layer call on that context or sph_destroy.  Every word holds
 *               exactly the sum of sph_sample.h's terms of the rank's owned particles at that sample.  It is a read-out, not simulation
 *               state: a step does not drop it, and the call changes nothing a step reads.
 *   info        the exponents used and the RANK's counts: n_touching and n_pairs of the ranks add up to the whole vector's,
 *               max_footprint is their maximum.  May be NULL.
 *   sph_slab_sample_layer_download copies the layer to the host.
 *
 * COMPOSE (sph_sample_compose; any context, plain or slab -- it reads no particle, only `sp` and the host layers)
 *   per sample and plane the sum over the layers whose band holds its column, then sph_sample.h's resolved output (normalise,
 *   min_weight and fill as there) with sp's exponents, which must be explicit.  layers[k] is a HOST pointer to (C+1) * ny * (sx1 - sx0)
 *   words of bands[k]; it may be NULL iff bands[k] is empty; n_layers may be 0 (all-zero planes).  values_out / raw_out as
 *   sph_sample_grid.
 *
 * GROUP CALL (sph_group_sample_grid; the n slab contexts of one process that sph_group_step steps; `sp` may hold automatic exponents)
 *   the same planes without host transit when all members sit on ONE device: every member's range pass reduces into member 0's
 *   words (a 64-bit atomic minimum and 32-bit atomic maxima fold by themselves), one synchronisation, the host takes the exponents
 *   or refuses; every member computes its band and scatters its layer on its own stream; member 0 adds the layers straight from the
 *   members' buffers (one launch per layer, ordered by events), resolves and copies out.  Only the words, the bands and the resolved
 *   planes cross the bus.  When the members do not all sit on one device it runs the per-rank calls above: ranges, fold, layers,
 *   downloads, compose on member 0.
 *   (Only the one-device branch and the host path have run anywhere: the project's machines have one GPU.)
 *   info: the exponents used, the summed counts, the maximum footprint.  Every member's layer is left as sph_slab_sample_layer leaves it.
 *   Whichever member refuses, the sentence is left in member 0's sph_last_error.
 *
 * REFUSALS (taken before anything is launched, except the data preconditions)
 *   SPH_ERR_UNSUPPORTED        sph_slab_sample_range / _layer / _layer_download on a plain context, a plain context as a group member
 *                              (sph_sample_grid samples it)
 *   SPH_ERR_POISONED           a poisoned context (range, layer, group call)
 *   SPH_ERR_INVALID_ARGUMENT   every geometry, channel and buffer refusal of sph_sample_grid, unchanged: nx or ny outside
 *                              1..SPH_SAMPLE_MAX_SIDE, (C+1)*nx*ny*8 above 2 GiB, spacing not finite or <= 0, origin not finite, an
 *                              unknown field, a component the field does not have, more than SPH_SAMPLE_MAX_CHANNELS channels, an unknown
 *                              volume mode, an exponent outside the range, a short output buffer;
 *                              SPH_SAMPLE_AUTO_EXPONENT given to the layer call or to compose (sph_sample_fold_words comes first);
 *                              a data precondition (fold, group call), naming the smallest offending global id;
 *                              a band with sx0 > sx1 or outside [0, nx]; a NULL layer for a non-empty band; n_layers < 0;
 *                              a download without a layer or with capacity_words below (C+1) * ny * (sx1 - sx0);
 *                              n < 1, null words or null sp_io in the fold; n < 1 in the group call
 *   SPH_ERR_DEVICE
 * A short `msg` buffer truncates and does not fail.  After a refusal the output buffers are unspecified; no context is poisoned and
 * nothing of it changed.  Nothing here changes the simulation state; every launch runs on the stream of the context it works for.
 */
#ifndef SPH_SLAB_SAMPLE_H
#define SPH_SLAB_SAMPLE_H

#include <stdint.h>

#include "sph_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sph_slab_sample_words {
    uint64_t first_bad;                           /* all ones: none; else (global id << 8) | reason */
    uint32_t max_bits[SPH_SAMPLE_MAX_CHANNELS];   /* max |a_j| per channel as float bits */
} sph_slab_sample_words;   /* 32 bytes */

typedef struct sph_sample_band {
    int32_t  sx0, sx1;   /* sample columns [sx0, sx1) of the nx columns that hold this rank's layer; sx0 == sx1: empty */
    uint32_t n_boxes;    /* owned particles whose box is live */
    uint32_t reserved;
} sph_sample_band;         /* 16 bytes */

/* local to the rank */
int sph_slab_sample_range(sph_ctx* ctx, const sph_params* params, const sph_sample_params* sp, sph_slab_sample_words* out);
int sph_slab_sample_layer(sph_ctx* ctx, const sph_params* params, const sph_sample_params* sp, sph_sample_band* band, sph_sample_info* info);
int sph_slab_sample_layer_download(sph_ctx* ctx, int64_t* words, uint64_t capacity_words);

/* no context: the ranks' words -> the exponents of the whole vector in sp_io, or the refusal's sentence in msg */
int sph_sample_fold_words(int n, const sph_slab_sample_words* words, sph_sample_params* sp_io, char* msg, uint64_t msg_bytes);

/* any context (plain or slab); layers are HOST pointers, layers[k] may be NULL iff bands[k] is empty; n_layers may be 0 */
int sph_sample_compose(sph_ctx* ctx, const sph_sample_params* sp, int n_layers, const sph_sample_band* bands, const int64_t* const* layers,
                       float* values_out, uint64_t values_bytes, int64_t* raw_out, uint64_t raw_bytes);

/* the n slab contexts of one process that sph_group_step steps */
int sph_group_sample_grid(sph_ctx** ctxs, int n, const sph_params* params, const sph_sample_params* sp, float* values_out, uint64_t values_bytes,
                          int64_t* raw_out, uint64_t raw_bytes, sph_sample_info* info);

#ifdef __cplusplus
}
#endif

#endif /* SPH_SLAB_SAMPLE_H */
