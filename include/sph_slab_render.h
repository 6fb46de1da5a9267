/*
 * sph_slab_render.h -- the frame of sph_render.h drawn from SLAB contexts: every rank draws the particles it owns into a layer, the
 * layers are composed per sample.  sph_render itself keeps refusing a slab context (one rank holds a slab of the frame's particles).
 *
 * Why it decomposes.  sph_render.h's painter gives a sample to the covering particle with the LARGEST REFERENCE INDEX.  On slabs the
 * reference index is the global particle id (SPH_F_PARTICLE_ID) and every particle is owned by exactly one rank, so a rank resolves
 * its own particles into one 64-bit word per sample,
 *     word = 0                                     no owned particle covers the sample
 *     word = ((uint64)(id + 1) << 32) | rgb24      id = the largest covering global id among the owned particles;
 *                                                  rgb24 = r | g << 8 | b << 16 of its fill colour if d2 < ri*ri, else 0 (stroke band)
 * and the frame's sample is the UNSIGNED MAXIMUM of the ranks' words: the high half orders by id, ids are unique, so the maximum is
 * the winner's word.  The maximum is commutative and associative -- the frame does not depend on the order of the layers -- and the
 * result is byte for byte the frame sph_render draws for one context that holds the same particles.  Only the layers cross the
 * bus: a rank's particles sit in an x-slab, its layer is a band of sample columns, the bands together are about one frame of words,
 * independent of the particle count.
 *
 * A separate header from sph_ffi.h, like sph_render.h: product library only.  sph_render_params is reused unchanged; of its flags
 * SPH_RENDER_INTERPOLATE is refused (below).  Status codes are those of sph_ffi.h.  Every operation below is one IEEE f32 operation,
 * no contraction, in sph_render.h's order; tests/render_reference.py restates it in numpy.
 *
 * PRESSURE MAXIMUM (read only for SPH_VIS_PRESSURE)
 *   sph_slab_render_pressure_max: fold(0, max) over the OWNED particles' current pressure; a NaN or a value <= 0 leaves the
 *   accumulator (sph_render.h's reduction).  The host takes the maximum of the ranks' values -- an f32 maximum does not depend on
 *   the order -- and passes it to every rank's layer call as `pressure_max`; the stops are (0, white), (0.9 * pressure_max, red).
 *
 * LAYER (sph_slab_render_layer; local to the rank, no communication)
 *   particles   the rank's owned slots only (before the first step, and behind an upload, every slot is owned; ghosts draw nothing)
 *   colour      sph_render.h's, of the fields this rank holds; RANDOM_COLOR hashes the global id; position and radius as there
 *   MIN_DISTANCE  the walk runs over owned + ghost slots with the candidates and the predicate sph_download_neighbors uses on a
 *               slab context; the distance to a ghost is taken to the advected record the step's level estimation refreshed from its
 *               owner (a ghost lane does not integrate), so it needs a step WITH level estimation behind it (refusals)
 *   band        [sx0, sx1): the union of the sample-column ranges of the drawable owned discs' boxes
 *                   x in [max(floor(px - ro) - 1, 0), min(ceil(px + ro) + 1, WS - 1)],  y likewise against HS
 *               (a disc is drawable if ro > 0 and px, py, ro are finite and below 1e30; its box must meet the frame in x AND y).
 *               Every covered sample lies in the band; n_drawn counts those discs; nothing to draw: sx0 == sx1 == 0, n_drawn == 0
 *   storage     the layer stays in the context: HS * (sx1 - sx0) words, row-major, row 0 at the top, word (sy, sx - sx0), until the
 *               next layer call on that context or sph_destroy.  It is a picture, not simulation state: a step does not drop it.
 *   sph_slab_render_layer_download copies it to the host.
 *
 * COMPOSE (sph_render_compose; any context, plain or slab -- it reads no particle, only `rp`'s frame geometry and boundary)
 *   per sample the unsigned maximum over the layers whose band holds its column; a word != 0 gives its low 24 bits as rgb; a word 0
 *   gives black on a boundary stroke, else white (sph_render.h: "boundary"); a pixel is (sum of its S*S samples + S*S/2) / (S*S).
 *   layers[k] is a HOST pointer to HS * (sx1 - sx0) words of bands[k]; it may be NULL iff bands[k] is empty; n_layers may be 0 (the
 *   frame of an empty context: background and boundary).  rgb_out / out_bytes as sph_render.
 *
 * GROUP RENDER (sph_group_render; the n slab contexts of one process that sph_group_step steps)
 *   the same frame without host transit when all members sit on ONE device: the pressure maximum is reduced into one device word
 *   by all members, every member draws its layer, member 0 merges the layers straight from the members' buffers (one launch per
 *   layer, ordered by events) and resolves the frame; only the three band words per member and the frame cross the bus.  When the
 *   members do not all sit on one device it runs the per-rank calls above: pressure maxima, layers, downloads, compose on member 0.
 *   (Only the one-device branch and the host path have run anywhere: the project's machines have one GPU.)
 *   Every member's layer is left as sph_slab_render_layer leaves it.
 *
 * REFUSALS
 *   SPH_ERR_UNSUPPORTED        sph_slab_render_pressure_max / _layer / _layer_download on a plain context (sph_render draws it);
 *                              SPH_RENDER_INTERPOLATE on a slab (a particle may have changed rank since the snapshot)
 *   SPH_ERR_POISONED           a poisoned context (pressure maximum, layer, group render)
 *   SPH_ERR_INVALID_ARGUMENT   SPH_VIS_MIN_DISTANCE_TO_NEIGHBOR where sph_download_neighbors on that slab context refuses (no step
 *                              yet, or the lists are gone), or behind a step without level estimation (see LAYER);
 *                              S outside 1..4, W or H < 1, more than 16384 samples per side, zoom_out <= 0, more than 32 segments,
 *                              no stops or more than 16 for a mapped attribute, a short output buffer -- as sph_render;
 *                              a download without a layer or with capacity_words below HS * (sx1 - sx0);
 *                              a band with sx0 > sx1 or outside [0, WS]; a NULL layer for a non-empty band; n_layers < 0;
 *                              n < 1 or a member that is no slab context in the group call
 *   SPH_ERR_DEVICE
 * Nothing here changes the simulation state; every launch runs on the stream of the context it works for.
 */
#ifndef SPH_SLAB_RENDER_H
#define SPH_SLAB_RENDER_H

#include <stdint.h>

#include "sph_render.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t  sx0, sx1;   /* sample columns [sx0, sx1) of the WS x HS sample grid that hold this rank's layer; sx0 == sx1: empty */
    uint32_t n_drawn;    /* owned particles with a drawable disc whose box meets the frame */
    uint32_t reserved;
} sph_render_band;      /* 16 bytes */

/* local to the rank */
int sph_slab_render_pressure_max(sph_ctx* ctx, float* out);
int sph_slab_render_layer(sph_ctx* ctx, const sph_params* params, const sph_render_params* rp, float pressure_max, sph_render_band* band);
int sph_slab_render_layer_download(sph_ctx* ctx, uint64_t* words, uint64_t capacity_words);

/* any context (plain or slab); layers are HOST pointers, layers[k] may be NULL iff bands[k] is empty; n_layers may be 0 */
int sph_render_compose(sph_ctx* ctx, const sph_render_params* rp, int n_layers, const sph_render_band* bands,
                       const uint64_t* const* layers, uint8_t* rgb_out, uint64_t out_bytes);

/* the n slab contexts of one process that sph_group_step steps */
int sph_group_render(sph_ctx** ctxs, int n, const sph_params* params, const sph_render_params* rp, uint8_t* rgb_out, uint64_t out_bytes);

#ifdef __cplusplus
}
#endif

#endif /* SPH_SLAB_RENDER_H */
