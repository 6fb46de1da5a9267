/*
 * sph_sample.h -- SPH fields sampled on a regular grid on the device, reproducibly.
 *
 * What every SPH host asks of a particle state -- "what is the field at this point?" -- answered where the state lives: the SPH
 * interpolant  A(X) = sum_j V_j a_j W(|X - x_j|, h_j)  of density, pressure, velocity, the constant field or the surface distance on
 * nx x ny points, and the weight  sum_j V_j W  (the partition of unity) beside it.  Only the planes cross PCIe.
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only (the CPU oracle samples nothing).
 *
 * The sums are 64-BIT FIXED-POINT INTEGERS.  Integer addition is associative: the planes do not depend on the device's cell-sorted
 * order, on the launch shape or on the order the atomics arrive in; a restatement in numpy reproduces every sum bit for bit
 * (tests/sample_reference.py), and the raw planes of disjoint particle sets add exactly.
 *
 * THE PLANES, exactly (every operation below is one IEEE f32 operation, no contraction, correctly rounded `/` and sqrtf):
 *   grid        nx columns, ny rows, sample (sx, sy), row 0 = LOWEST y
 *               X = origin_x + ((float)sx + 0.5f) * spacing
 *               Y = origin_y + ((float)sy + 0.5f) * spacing
 *   particle j  (x, y, m, h) as sph_download returns position, mass, h2 at the time of the call (h2 IS the smoothing length)
 *               rho_j = SPH_F_DENSITY
 *               dx = X - x;  dy = Y - y;  r = sqrtf(dx*dx + dy*dy);  q = r / (2.f * h)
 *               touches the sample iff q < 1
 *               k = cubic_unnorm(q):  q < 0.5f: 6.f * (q*q*q - q*q) + 1.f;  else v = 1.f - q, 2.f * (v*v*v)    (sph_kernels.rs:23-32)
 *               norm = 10.f / ((7.f * PI_F) * (h * h))                                                        (sph_kernels.rs:50)
 *               W = norm * k
 *               V = m / rho_j           (SPH_SAMPLE_VOLUME_DENSITY, the default)
 *               V = m / rest_density    (SPH_SAMPLE_VOLUME_REST)
 *               w = V * W
 *   plane 0     Q0[sy][sx] = sum_j (int64) trunc(w * 4294967296.f)
 *   channel c   value a_j, exponent e_c
 *               t = w * a_j
 *               Qc[sy][sx] = sum_j (int64) trunc(t * 2^(32 - e_c))
 * A channel is a (field, component) pair: SPH_F_DENSITY, SPH_F_PRESSURE, SPH_F_VELOCITY (component 0 or 1), SPH_F_CONSTANT_FIELD,
 * SPH_F_LEVEL_ESTIMATION (a NaN -- FluidInterior -- counts as -maximum_surface_distance, the renderer's DISTANCE rule); component 0
 * for the scalars.  At most SPH_SAMPLE_MAX_CHANNELS per call.
 *
 * EXPONENTS.  e_c is the smallest integer with max_j |a_j| < 2^e_c, or 0 when the maximum is 0.  The caller gives it, or gives
 * SPH_SAMPLE_AUTO_EXPONENT: the library then takes it from an exact reduction on the device (the maximum of the bit patterns of
 * |a_j|, which order like the values) -- sph_sample_field_range exposes the same reduction on a plain context; the ranks of a slab
 * decomposition agree on an exponent through sph_slab_sample.h.  Allowed: SPH_SAMPLE_MIN_EXPONENT .. SPH_SAMPLE_MAX_EXPONENT; an automatic exponent below the range is raised to its lower
 * end, one above it is refused.  The exponents used come back in sph_sample_info.
 *
 * THE RESOLVED OUTPUT (f32 planes, (C+1) x ny x nx, plane 0 = the weight):
 *   weight  = (float)((double)Q0 * 2^-32)
 *   value_c = (float)((double)Qc * 2^(e_c - 32))
 * and with SPH_SAMPLE_NORMALIZE
 *   value_c = value_c / weight   where weight >= min_weight
 *   value_c = fill               elsewhere (fill is the caller's value, NaN allowed)
 * raw_out is optional: the same planes as int64.
 *
 * PRECONDITIONS, all data-driven: one pass over all particles checks them before anything is accumulated, and a failure
 * (SPH_ERR_INVALID_ARGUMENT) names the SMALLEST offending reference index in sph_last_error:
 *   h finite and > 0 (after sph_upload and before the first step h is 0: the call is refused);  V finite and >= 0;
 *   V * norm < 2^20;  every a_j of a requested channel finite (after the level rule) and |a_j| < 2^e_c.
 * They bound every term below 2^52 in magnitude.  After such a refusal the output buffers are unspecified; the context is not
 * poisoned and nothing of it changed.
 *
 * WHICH STATE.  h, density and pressure are OUTPUTS OF A STEP (sph_ffi.h, "per-step outputs"): they line up with the particles from the
 * end of sph_step until the next call that edits the vector -- sph_apply_edits, sph_share_particles / sph_merge_particles /
 * sph_split_particles and their compact and device forms, sph_upload_field of mass or position.  Behind such a call the density and
 * pressure arrays are the old vector's: the density and pressure channels and the volume m / rho_j (so the weight and EVERY plane under
 * SPH_SAMPLE_VOLUME_DENSITY) then mix particles, and a particle a split appended has no density at all, which the V precondition
 * refuses.  The library does not track this (it reads no flag of the step's state): call sph_sample_grid directly behind sph_step,
 * before the step's adaptivity, or sample carried fields only (velocity, level_estimation) with SPH_SAMPLE_VOLUME_REST.
 *
 * Status codes are those of sph_ffi.h: SPH_ERR_INVALID_ARGUMENT (nx or ny outside 1..SPH_SAMPLE_MAX_SIDE, (C+1)*nx*ny*8 above 2 GiB,
 * spacing not finite or <= 0, origin not finite, an unknown field, a component the field does not have, more than
 * SPH_SAMPLE_MAX_CHANNELS channels, an unknown volume mode, an exponent outside the range, a short output buffer, a precondition),
 * SPH_ERR_POISONED, SPH_ERR_UNSUPPORTED (slab contexts: one rank holds a slab of the particles -- sph_slab_sample.h samples them: the
 * composition of the ranks' RAW planes is exact addition), SPH_ERR_DEVICE.  Nothing here reads a flag of the simulation state or changes it; every launch runs on
 * the context's stream; the buffers are allocated on first use, reused, and freed by sph_destroy.
 */
#ifndef SPH_SAMPLE_H
#define SPH_SAMPLE_H

#include <stdint.h>

#include "sph_ffi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_SAMPLE_MAX_CHANNELS 6
#define SPH_SAMPLE_MAX_SIDE 16384
#define SPH_SAMPLE_MAX_RAW_BYTES (1ull << 31)   /* (C+1) * nx * ny * 8 */
#define SPH_SAMPLE_MIN_EXPONENT (-64)
#define SPH_SAMPLE_MAX_EXPONENT 64
#define SPH_SAMPLE_AUTO_EXPONENT 0x7fffffff

enum { SPH_SAMPLE_VOLUME_DENSITY = 0, SPH_SAMPLE_VOLUME_REST = 1 };
enum { SPH_SAMPLE_NORMALIZE = 1 };

typedef struct sph_sample_channel {
    int32_t field;       /* SPH_F_DENSITY | SPH_F_PRESSURE | SPH_F_VELOCITY | SPH_F_CONSTANT_FIELD | SPH_F_LEVEL_ESTIMATION */
    int32_t component;   /* 0, or 1 for the y component of SPH_F_VELOCITY */
    int32_t exponent;    /* e_c, or SPH_SAMPLE_AUTO_EXPONENT */
} sph_sample_channel;

typedef struct sph_sample_params {
    int32_t  nx, ny;
    float    origin_x, origin_y;   /* the lower left corner of sample (0, 0)'s cell: its centre lies half a spacing inside */
    float    spacing;
    int32_t  volume;               /* SPH_SAMPLE_VOLUME_* */
    uint32_t flags;                /* SPH_SAMPLE_NORMALIZE */
    float    min_weight, fill;     /* (with SPH_SAMPLE_NORMALIZE) */
    int32_t  n_channels;           /* C: 0 .. SPH_SAMPLE_MAX_CHANNELS */
    sph_sample_channel channels[SPH_SAMPLE_MAX_CHANNELS];
} sph_sample_params;

typedef struct sph_sample_info {
    int32_t  exponents[SPH_SAMPLE_MAX_CHANNELS];   /* e_c as used (0 beyond n_channels) */
    uint64_t n_touching;                           /* particles that touch at least one sample */
    uint64_t max_footprint;                        /* the most samples one particle touches */
    uint64_t n_pairs;                              /* (particle, sample) pairs with q < 1: every one adds to C+1 planes (zero terms are skipped) */
} sph_sample_info;

/* The planes: values_out receives (C+1) x ny x nx f32 (>= that many * 4 bytes), raw_out -- may be NULL -- the same planes as int64
 * (>= that many * 8 bytes); info may be NULL. */
int sph_sample_grid(sph_ctx* ctx, const sph_params* params, const sph_sample_params* sp, float* values_out, uint64_t values_bytes,
                    int64_t* raw_out, uint64_t raw_bytes, sph_sample_info* info);
/* max_j |a_j| of one channel and the exponent that goes with it (not clamped to the allowed range).  Refused with
 * SPH_ERR_INVALID_ARGUMENT, naming the particle, when a value is not finite.  Either output may be NULL. */
int sph_sample_field_range(sph_ctx* ctx, const sph_params* params, int field, int component, float* max_abs, int32_t* exponent);

#ifdef __cplusplus
}
#endif

#endif /* SPH_SAMPLE_H */
