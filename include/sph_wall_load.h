/*
 * sph_wall_load.h -- the load the fluid puts on its boundary: force, torque, normal force and the peak pressure PER BOUNDARY ELEMENT,
 * with an optional pressure profile along a plane, reduced where the state lives.  What a dam break or a sloshing tank is run for.
 *
 * A separate header from sph_ffi.h, like sph_ledger.h: this entry point exists in the product library only.
 *
 * THE FORCE IS THE ONE THE SOLVER EXCHANGES WITH THE WALL, not an interpolant read next to it.  The semi-analytic boundary gives every
 * particle near SDF number k an entry (lambda_k, grad lambda_k) (boundary_winchenbach2020.rs:58-152); the pressure solve pushes the
 * particle with a_i = sum_k -rho_b (p_i / rho_i^2 + p_ib / rho_b^2) grad lambda_k (:164-194; Winchenbach 2020, Eq. 47).  By Newton's
 * third law the wall receives +m_i times each term.  The step keeps only the per-particle sum over k; here the entries stay apart.
 *
 * ELEMENTS.  E = the number of SDFs of the context's boundary: n_planes plane elements in the order given to sph_create, or ONE element
 * when sph_set_boundary_polygon replaced them.  E <= SPH_MAX_PLANES (8).  A context without a boundary has E = 0: the call succeeds, reads
 * nothing, and the result is all zero bytes.
 *
 * WHICH STATE.  The "WHICH STATE" paragraph of sph_sample.h applies word for word.  The entries are evaluated at the CURRENT positions
 * and h (what SPH_LEDGER_STEP_OUTPUTS reads as h); pressure and density are the arrays sph_ledger.h reads for SPH_LEDGER_STEP_OUTPUTS.
 * Plainly: PRESSURE AND DENSITY BELONG TO THE STEP, THE POSITIONS TO ITS END -- the step solved its pressure with the entries of the
 * positions it started from and then moved the particles; the load pairs that pressure with the entries of where the particles are now.
 * Valid from the end of sph_step until the next call that edits the particle vector.
 *
 * THE ENTRY of particle i at element k.  f32, one IEEE operation per operator, no contraction, in the order of the step's density sweep:
 *   1. sr = 2 h
 *   2. d = probe_k(x, y) / sr;  no entry unless d < 1
 *   3. the central-difference gradient of probe_k with eps = params->sdf_gradient_eps:
 *        gx = (probe_k(x + eps, y) - probe_k(x - eps, y)) * (1 / (2 eps)),  gy likewise;  gn = sqrt(gx gx + gy gy);
 *      no entry unless gn >= 1e-5;  (nx, ny) = (gx / gn, gy / gn)
 *   4. penalty, dpenalty from params->boundary_penalty_term:
 *        None        1, 0
 *        Linear      1 - d, -1
 *        Quadratic1  d > 0: 1, 0;   d > -1:   0.5 d d + 1, d;   else 0.5 - d, -1
 *        Quadratic2  d > 0: 1, 0;   d > -0.5: d d + 1, 2 d;     else 0.75 - d, -1
 *   5. lambda, dlambda: d <= -1: 1, 0;  else the two lookup-table lerps of the step (LookupTable1D::get over (-1, 1, 10000))
 *   6. s = dpenalty * lambda + penalty * dlambda;   g = (nx / sr * s, ny / sr * s)
 *   probe_k: (dir_x * x + dir_y * y) + delta of plane k, or the polygon's signed distance as the step probes it.
 *
 * THE COEFFICIENT (f32, the order of boundary_winchenbach2020.rs:191): rho_b = params->rest_density; p_ib = p_i under
 * ConsistentSymmetricGradient, else 0;  c = rho_b * (p_i / (rho_i * rho_i) + p_ib / (rho_b * rho_b)).
 *
 * THE TERMS of an entry.  D(a) is the exact conversion of an f32 to f64; every operator ONE IEEE f64 operation:
 *   fx = (D(m) * D(c)) * D(g.x)        fy = (D(m) * D(c)) * D(g.y)
 *   tq = D(x) * fy - D(y) * fx         (about the origin)
 *   fn = -(fx * D(nx) + fy * D(ny))    (positive where the fluid presses against the wall)
 *
 * THE SUMS, four per element (SPH_WALL_LOAD_N_SUMS): FORCE_X, FORCE_Y, TORQUE, NORMAL.  Each is a 128-bit fixed-point integer under the
 * rules of sph_ledger.h: Q = sum over the entries of (int64) trunc(t * 2^(60 - e)), e per (element, sum) given in spec.exponent[k][s] or
 * SPH_LEDGER_AUTO_EXPONENT (then the smallest e with max |t| < 2^e, 0 without entries, raised to SPH_LEDGER_MIN_EXPONENT, refused above
 * SPH_LEDGER_MAX_EXPONENT); resolved as the nearest f64 of Q times 2^(e - 60).  Integer addition: the result depends neither on the
 * device's order nor on the launch shape, and tests/wall_load_reference.py reproduces every byte.  No floating-point atomic anywhere.
 *
 * PER ELEMENT besides: n_entries; n_wet, the entries with p_i > 0; max_pressure, a maximum key in the ledger's key format (ord(p) << 32 |
 * 0xffffffff - id, unsigned maximum) over the particles with an entry: the value and the id, ties to the smallest id, {0, SPH_LEDGER_NO_ID}
 * without entries.  id = the reference index of the slot (SPH_F_PARTICLE_ID).
 *
 * THE PROFILE along a plane (optional; plane elements only).  spec.bins = 0, or 1 .. SPH_WALL_LOAD_MAX_BINS: the row length of `profile`
 * (E rows of spec.bins int64 words).  Element k has B = spec.n_bins[k] in 0 .. spec.bins bins over [s_lo[k], s_hi[k]); B = 0: no profile
 * (its row stays 0).  inv_ds = (float)B / (s_hi - s_lo), computed once on the host in f32 and returned.  Of an entry:
 *   s = (-dir_y * x) + (dir_x * y)            f32, the tangential coordinate
 *   fb = floorf((s - s_lo) * inv_ds)          f32;  binned when 0 <= fb < B, then b = (int)fb
 *   profile[k][b] += (int64) trunc(fn * 2^(40 - e_NORMAL[k]))     a 64-bit integer atomic
 * Every other entry of an element with B > 0 counts in n_unbinned[k].  Each term is below 2^40 in magnitude; an element with bins and
 * 2^23 or more entries is refused (a condition, not a measurement: 2^23 terms below 2^40 cannot leave 63 bits).  The resolved value of
 * a bin is (double)word * 2^(e_NORMAL - 40): a force; divided by the bin width (s_hi - s_lo) / B a line pressure.
 *
 * PRECONDITIONS, data-driven like the ledger's: the range pass checks them before anything is accumulated, and a failure
 * (SPH_ERR_INVALID_ARGUMENT) names the SMALLEST offending id and the reason in sph_last_error.  EVERY particle is checked, with or
 * without an entry; a particle reports its FIRST failing check (the reason codes of sph_wall_load_words.first_bad in brackets):
 *   1. not finite: m [1], x [2], y [3], h [4], rho [5], p [6]
 *   2. rho > 0 does not hold [7].  Before the first step rho is 0: the call is refused, and the sentence says so
 *   3. h > 0 does not hold [8]
 *   4. a term is not finite, or not below 2^e in magnitude for an explicit exponent [16 + 4 k + s]
 * After a refusal the outputs are unspecified; the context is not poisoned and nothing of it changed.
 *
 * ONE CONTEXT: two streaming passes on the context's stream -- the range pass (checks, counts, keys, max |t| as f64 bits: the 66 words of
 * sph_wall_load_words) and the sum pass (the 32 sums and the profile) -- and two waits.  sph_wall_load_words, the 128-bit sums and the
 * int64 profile words are what a follow-up needs to add range -> fold -> sums -> compose over slab ranks exactly as sph_ledger.h does:
 * every word folds by minimum, sum or maximum, the integers add.  SLAB CONTEXTS ARE NOT SUPPORTED HERE.
 *
 * REFUSALS (taken before anything is launched, except the data preconditions and the 2^23 condition)
 *   SPH_ERR_UNSUPPORTED        a slab context
 *   SPH_ERR_POISONED           a poisoned context
 *   SPH_ERR_INVALID_ARGUMENT   null pointers (profile may be NULL when bins = 0); flags != 0; bins outside 0 .. 4096; an explicit exponent
 *                              outside the range; n_bins[k] outside 0 .. bins; with n_bins[k] > 0: s_lo / s_hi not finite, s_hi <= s_lo,
 *                              inv_ds not finite; bins > 0 on a polygon context; a data precondition
 *   SPH_ERR_DEVICE
 * Nothing here reads a flag of the simulation state or writes anything a step reads; every launch runs on the context's stream; the
 * small buffers are allocated on first use, reused, and freed by sph_destroy.
 */
#ifndef SPH_WALL_LOAD_H
#define SPH_WALL_LOAD_H

#include <stdint.h>

#include "sph_ffi.h"
#include "sph_ledger.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_WALL_LOAD_MAX_ELEMENTS 8   /* SPH_MAX_PLANES */
#define SPH_WALL_LOAD_N_SUMS 4
#define SPH_WALL_LOAD_MAX_BINS 4096
#define SPH_WALL_LOAD_MAX_BINNED_ENTRIES 8388608   /* 2^23 */
#define SPH_WALL_LOAD_BIN_SHIFT 40

enum { SPH_WALL_LOAD_FORCE_X = 0, SPH_WALL_LOAD_FORCE_Y, SPH_WALL_LOAD_TORQUE, SPH_WALL_LOAD_NORMAL };

typedef struct sph_wall_load_spec {
    uint32_t flags;                                                             /* 0 */
    int32_t  bins;                                                              /* 0, or the row length of `profile` */
    int32_t  exponent[SPH_WALL_LOAD_MAX_ELEMENTS][SPH_WALL_LOAD_N_SUMS];        /* e, or SPH_LEDGER_AUTO_EXPONENT */
    int32_t  n_bins[SPH_WALL_LOAD_MAX_ELEMENTS];                                /* B of element k, 0 .. bins */
    float    s_lo[SPH_WALL_LOAD_MAX_ELEMENTS];
    float    s_hi[SPH_WALL_LOAD_MAX_ELEMENTS];
} sph_wall_load_spec;      /* 232 bytes */

typedef struct sph_wall_load_element_words {
    uint64_t n_entries, n_wet, n_unbinned;
    uint64_t max_bits[SPH_WALL_LOAD_N_SUMS];                                    /* max |t| per sum as f64 bits */
    uint64_t max_pressure;                                                      /* the key */
} sph_wall_load_element_words;   /* 64 bytes */

typedef struct sph_wall_load_words {
    uint64_t first_bad;                                                         /* all ones: none; else (id << 8) | reason */
    uint64_t n;                                                                 /* the particles looked at */
    sph_wall_load_element_words element[SPH_WALL_LOAD_MAX_ELEMENTS];
} sph_wall_load_words;     /* 528 bytes */

typedef struct sph_wall_load_element {
    int32_t  exponent[SPH_WALL_LOAD_N_SUMS];                                    /* e as used */
    sph_ledger_sum raw[SPH_WALL_LOAD_N_SUMS];                                   /* Q */
    double   sum[SPH_WALL_LOAD_N_SUMS];                                         /* resolved */
    uint64_t n_entries, n_wet, n_unbinned;
    sph_ledger_extreme max_pressure;
    float    inv_ds;                                                            /* as used; 0 without bins */
    int32_t  n_bins;
} sph_wall_load_element;   /* 152 bytes, no padding */

typedef struct sph_wall_load_result {
    uint32_t n_elements;                                                        /* E */
    int32_t  bins;
    uint64_t n;
    sph_wall_load_element element[SPH_WALL_LOAD_MAX_ELEMENTS];                  /* zero from E on */
} sph_wall_load_result;    /* 1232 bytes, no padding */

/* a plain context; profile: E x spec->bins int64 words, may be NULL when bins = 0 */
int sph_wall_load_compute(sph_ctx* ctx, const sph_params* params, const sph_wall_load_spec* spec, sph_wall_load_result* out, int64_t* profile);

#ifdef __cplusplus
}
#endif

#endif /* SPH_WALL_LOAD_H */
