/*
 * sph_probe.h -- SPH fields at arbitrary points, and tracers, on the device, reproducibly.
 *
 * sph_sample.h answers "what is the field here?" on a lattice.  This header answers it at a SET OF POINTS the caller chooses -- the
 * gauges of a validation run (a pressure sensor on the wall, a vertical line of points for the water height, a cross-section) -- and
 * moves such points with the fluid's interpolated velocity (tracers: dye points, independent of the particles that share, merge and
 * split under them).  Only the points' values cross PCIe; an advect moves the points where they live.
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only.
 *
 * THE TERMS are those of sph_sample.h, "THE PLANES" and "THE RESOLVED OUTPUT", word for word, with (X, Y) the probe's own two floats
 * in place of a sample's centre: the same f32 operations in the same order (one device function evaluates a pair for both forms), the
 * same 64-bit fixed-point sums, the same channels, volumes, exponent rules and SPH_SAMPLE_AUTO_EXPONENT.  A probe that sits on a
 * lattice sample's centre therefore gets that sample's raw words bit for bit, and the raw sums of disjoint particle sets add exactly.
 *
 * A PROBE SET (sph_probe_set) is a device-resident array of points that belongs to the context it was created with: the points in the
 * caller's order, and a table that bins them into square cells over their bounding box (the particles are scattered ONTO the binned
 * points: a particle reads the cells its support overlaps).  Every coordinate must be finite: a point that is not is refused at
 * create / upload (SPH_ERR_INVALID_ARGUMENT, "probe k=...", the smallest index).  0 <= n_points <= SPH_PROBE_MAX_POINTS, and for a call
 * with C channels (C+1) * n_points * 8 <= SPH_SAMPLE_MAX_RAW_BYTES.
 *   cell_hint   0: the library chooses the cell size from the points' bounding box and count.  A positive finite value asks for that
 *               size; the library RAISES it as far as needed to keep the table within SPH_PROBE_MAX_CELLS cells (2^22), so the memory
 *               of a set is O(n_points + SPH_PROBE_MAX_CELLS) whatever the coordinates are.  The geometry actually used comes back in
 *               sph_probe_info.  NO OUTPUT DEPENDS ON THE CELL SIZE: the predicate q < 1 alone decides which pairs add, and integer
 *               addition is associative.
 * A set is freed by sph_probe_set_destroy or, at the latest, by sph_destroy of its context.  A handle that is not a live set of the
 * context it is used with -- a set of another context, a destroyed set -- is refused with SPH_ERR_INVALID_ARGUMENT: the context keeps
 * the list of its sets and looks the handle up without reading through it.
 *
 * sph_probe_sample.  Output (C+1) x n_points, plane-major, plane 0 = the weight, in the caller's point order: values_out f32 as
 * sph_sample.h resolves them (SPH_SAMPLE_NORMALIZE, min_weight, fill), raw_out -- may be NULL -- the same planes as int64.  With
 * n_points == 0 the call succeeds and writes nothing (the buffers may be NULL).  The preconditions on the particles, the range pass
 * that checks them, the exponent handling and the refusal texts are sph_sample_grid's; the smallest offending reference index is named.
 *
 * sph_probe_advect, the tracer step: explicit Euler with the interpolated velocity, no sub-stepping.  The weight and the two velocity
 * channels are accumulated as above (exponent_x, exponent_y: a value or SPH_SAMPLE_AUTO_EXPONENT), then per point, every line one f32
 * operation, no contraction:
 *     weight = (float)((double)Q0 * 2^-32)
 *     u_c    = (float)((double)Qc * 2^(e_c - 32)) / weight        c = x, y
 *     X' = X + dt * u_x ;  Y' = Y + dt * u_y
 * where weight >= min_weight and both results are finite (n_moved counts these points, also where the velocity is 0); elsewhere the
 * point stays where it is and counts in n_stalled.  dt must be finite (any sign), min_weight finite and > 0.  The points are updated
 * in place on the device and the set bins itself again before its next use; nothing crosses the bus but the info struct.
 *
 * WHICH STATE (sph_sample.h has the paragraph).  h, density and pressure are outputs of a step: sample density or pressure -- and
 * anything under SPH_SAMPLE_VOLUME_DENSITY -- directly behind sph_step, before the step's adaptivity.  Velocity (and level_estimation)
 * under SPH_SAMPLE_VOLUME_REST is valid at any time: that is what tracers behind an adaptive step use.
 *
 * Status codes are those of sph_sample.h: SPH_ERR_INVALID_ARGUMENT (arguments, points, a handle that is not a live set of the context,
 * a short buffer, a precondition), SPH_ERR_POISONED, SPH_ERR_UNSUPPORTED (slab contexts: one rank holds a slab of the particles; the
 * raw sums of disjoint particle sets add exactly, so sph_slab_probe.h composes the ranks' raw words: sph_group_probe_sample / _advect
 * for the group of one process, the range, layer and compose calls for one process per rank), SPH_ERR_DEVICE.  The calls read
 * the simulation state and change none of it (no row of the carry table is involved); every launch runs on the context's stream.
 */
#ifndef SPH_PROBE_H
#define SPH_PROBE_H

#include <stdint.h>

#include "sph_sample.h"

#ifdef __cplusplus
extern "C" {
#define SPH_PROBE_STATIC_ASSERT(cond, text) static_assert(cond, text)
#else
#define SPH_PROBE_STATIC_ASSERT(cond, text) _Static_assert(cond, text)
#endif

#define SPH_PROBE_MAX_POINTS (1ull << 24)
#define SPH_PROBE_MAX_CELLS (1u << 22)   /* the bin table of a set: cells_x * cells_y never exceeds it */

typedef struct sph_probe_set sph_probe_set;   /* opaque */

typedef struct sph_probe_params {
    int32_t  volume;               /* SPH_SAMPLE_VOLUME_* */
    uint32_t flags;                /* SPH_SAMPLE_NORMALIZE */
    float    min_weight, fill;     /* (with SPH_SAMPLE_NORMALIZE) */
    int32_t  n_channels;           /* C: 0 .. SPH_SAMPLE_MAX_CHANNELS */
    sph_sample_channel channels[SPH_SAMPLE_MAX_CHANNELS];
} sph_probe_params;

typedef struct sph_probe_advect_params {
    float   dt;                    /* finite, any sign */
    int32_t volume;                /* SPH_SAMPLE_VOLUME_* */
    float   min_weight;            /* finite and > 0 */
    int32_t exponent_x, exponent_y;   /* of the two velocity channels: a value or SPH_SAMPLE_AUTO_EXPONENT */
} sph_probe_advect_params;

typedef struct sph_probe_info {
    int32_t  exponents[SPH_SAMPLE_MAX_CHANNELS];   /* e_c as used (0 beyond the call's channels; an advect: x, y) */
    uint64_t n_touching;                           /* particles that touch at least one point */
    uint64_t n_pairs;                              /* (particle, point) pairs with q < 1 */
    uint64_t n_touched_points;                     /* points with at least one touching particle */
    uint64_t n_moved, n_stalled;                   /* sph_probe_advect only (0 from sph_probe_sample) */
    float    cell_size;                            /* the bin geometry the call used (0 x 0 cells for an empty set) */
    int32_t  cells_x, cells_y;
    int32_t  reserved;
} sph_probe_info;

SPH_PROBE_STATIC_ASSERT(sizeof(sph_probe_params) == 92, "sph_probe_params");
SPH_PROBE_STATIC_ASSERT(sizeof(sph_probe_advect_params) == 20, "sph_probe_advect_params");
SPH_PROBE_STATIC_ASSERT(sizeof(sph_probe_info) == 80, "sph_probe_info");

/* xy: n_points pairs (x, y); may be NULL when n_points is 0.  cell_hint: see above. */
int sph_probe_set_create(sph_ctx* ctx, const float* xy, uint64_t n_points, float cell_hint, sph_probe_set** out);
/* replaces the points (n_points may change); the cell hint stays */
int sph_probe_set_upload(sph_ctx* ctx, sph_probe_set* set, const float* xy, uint64_t n_points);
/* the points as they are now, in the caller's order: bytes >= n_points * 8 */
int sph_probe_set_download(sph_ctx* ctx, sph_probe_set* set, float* xy_out, uint64_t bytes);
int sph_probe_set_size(sph_ctx* ctx, sph_probe_set* set, uint64_t* n_points);
/* the bin geometry the set's next use works with (behind an advect: chosen from the moved points); any output may be NULL */
int sph_probe_set_bins(sph_ctx* ctx, sph_probe_set* set, float* cell_size, int32_t* cells_x, int32_t* cells_y);
int sph_probe_set_destroy(sph_ctx* ctx, sph_probe_set* set);
/* values_out: (C+1) x n_points f32 (>= that many * 4 bytes); raw_out -- may be NULL -- the same as int64; info may be NULL */
int sph_probe_sample(sph_ctx* ctx, const sph_params* params, sph_probe_set* set, const sph_probe_params* pp, float* values_out, uint64_t values_bytes,
                     int64_t* raw_out, uint64_t raw_bytes, sph_probe_info* info);
int sph_probe_advect(sph_ctx* ctx, const sph_params* params, sph_probe_set* set, const sph_probe_advect_params* ap, sph_probe_info* info);

#ifdef __cplusplus
}
#endif

#endif /* SPH_PROBE_H */
