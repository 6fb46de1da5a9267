/*
 * sph_ledger.h -- the state ledger: what a host asks of a running simulation to watch it -- is it blowing up, which particle is
 * fastest, how many are below the floor, did the merge conserve mass and momentum -- reduced where the state lives.  Conserved
 * quantities as EXACT INTEGERS, extremes with the id of the particle that attains them, counts, and the refusal "particle i=... is not
 * finite".  A few hundred bytes cross the bus instead of whole fields.
 *
 * A separate header from sph_ffi.h, like sph_sample.h: these entry points exist in the product library only.
 *
 * The sums are 128-BIT FIXED-POINT INTEGERS.  Integer addition is associative and commutative: a sum depends neither on the device's
 * cell-sorted order nor on the launch shape nor on how the particles are cut across ranks; a restatement in numpy and Python ints
 * reproduces it bit for bit (tests/ledger_reference.py), and the sums of disjoint particle sets add exactly.  No floating-point
 * addition of two particles' terms and no floating-point atomic appears anywhere in the reduction.
 *
 * PARTICLES.  Every particle of a plain context.  On a slab context the slots the rank OWNS (before the first step, and behind an
 * upload, every slot is owned; ghosts are skipped), as sph_slab_sample.h takes them.  id = the reference index of the slot
 * (SPH_F_PARTICLE_ID): on a slab context the global particle id.
 *
 * WHAT IS ASKED FOR: spec.what, a bit set; no bit, or a bit not listed here, is refused.
 *   SPH_LEDGER_CARRIED        reads m, x, y, vx, vy.  Valid at any time: right after sph_upload, behind a step, behind share / merge /
 *                             split.  Sums 0..6, extremes 0..6
 *   SPH_LEDGER_STEP_OUTPUTS   reads m, density, the current pressure array and h (h2: the smoothing length).  OUTPUTS OF A STEP: valid
 *                             from the end of sph_step until the next call that edits the vector -- the "WHICH STATE" paragraph of
 *                             sph_sample.h applies word for word.  Sums 7..8, extremes 7..12
 *   SPH_LEDGER_OUTSIDE        reads x, y and the context's boundary.  Valid at any time.  The count n_outside
 *
 * THE SUMS (SPH_LEDGER_N_SUMS = 9).  D(a) is the exact conversion of an f32 to f64; every operation below is ONE IEEE f64 operation,
 * no contraction; rest = params->rest_density.
 *   s  name         group    term t_j
 *   0  MASS         carried  D(m)
 *   1  MOMENTUM_X   carried  D(m) * D(vx)
 *   2  MOMENTUM_Y   carried  D(m) * D(vy)
 *   3  MOMENT_X     carried  D(m) * D(x)
 *   4  MOMENT_Y     carried  D(m) * D(y)
 *   5  KINETIC      carried  0.5 * (D(m) * (D(vx) * D(vx) + D(vy) * D(vy)))
 *   6  ANGULAR      carried  D(m) * (D(x) * D(vy) - D(y) * D(vx))
 *   7  VOLUME       step     D(m) / D(rho)
 *   8  COMPRESSION  step     d = D(rho) - D(rest);  d > 0 ? d : 0
 *   Q_s = sum_j (int64) trunc(t_j * 2^(60 - e_s)), accumulated as a 128-bit two's-complement integer: sph_ledger_sum {lo, hi}, the
 *   value hi * 2^64 + lo.  The precondition |t_j| < 2^(e_s) keeps every term below 2^60 in magnitude: 2^31 particles cannot overflow.
 *   A sum whose group is not asked for is 0 with exponent 0; its spec.exponent is not looked at.
 *
 * EXPONENTS.  e_s is the smallest integer with max_j |t_j| < 2^(e_s), or 0 when the maximum is 0 (or no particle takes part).  The
 * maximum is exact: the maximum of the f64 BIT PATTERNS of |t_j|, which order like the values.  The caller gives spec.exponent[s], or
 * SPH_LEDGER_AUTO_EXPONENT.  Allowed: SPH_LEDGER_MIN_EXPONENT .. SPH_LEDGER_MAX_EXPONENT; an automatic exponent below the range is
 * raised to its lower end, one above it is refused.  The exponents used come back in the result.
 *
 * THE RESOLVED VALUE.  sum[s] = the 128-bit integer converted to the NEAREST f64, ties to even, times 2^(e_s - 60) (exact: a power of
 * two, no underflow in the allowed range).  In Python: math.ldexp(float(Q), e - 60).
 *
 * THE EXTREMES (SPH_LEDGER_N_EXTREMES = 13): a value and the id that attains it; among equal values the SMALLEST id.
 *   k   name           group    value (f32)
 *   0   MAX_SPEED2     carried  speed2 = vx * vx + vy * vy    (two products and one sum, each rounded to f32)
 *   1   MIN_X          carried  x          2  MAX_X
 *   3   MIN_Y          carried  y          4  MAX_Y
 *   5   MIN_MASS       carried  m          6  MAX_MASS
 *   7   MIN_DENSITY    step     rho        8  MAX_DENSITY
 *   9   MIN_PRESSURE   step     p          10 MAX_PRESSURE
 *   11  MIN_H          step     h          12 MAX_H
 *   Each is a 64-bit key reduction.  ord(a) = the f32 bit pattern of a, XOR 0x80000000 where the sign bit is clear, complemented
 *   where it is set: ord orders finite values like the values, -0 below +0.
 *     a maximum (k = 0 and every even k)   key = ord(a) << 32 | (0xffffffff - id), folded by UNSIGNED MAXIMUM; the empty key is 0
 *     a minimum (every odd k)              key = ord(a) << 32 | id,                folded by UNSIGNED MINIMUM; the empty key is all ones
 *   The result holds the value and the id; value 0 and id 0xffffffff where the key is empty (no particle, or the group not asked for).
 *
 * THE COUNTS.  n: the particles that took part.  n_outside (SPH_LEDGER_OUTSIDE): the particles with min_k probe_k(x, y) < 0 over the
 * context's planes -- probe = (dir_x * x + dir_y * y) + delta in f32 -- or its one polygon (sph_set_boundary_polygon: the signed
 * distance the step itself probes).  A probe of exactly 0 is not outside; a context without a boundary counts 0.
 *
 * PRECONDITIONS, all data-driven: the first pass checks them before anything is accumulated, and a failure
 * (SPH_ERR_INVALID_ARGUMENT) names the SMALLEST offending id and the reason in sph_last_error.  A particle reports its FIRST failing
 * check, in this order (the reason codes of sph_ledger_words.first_bad in brackets):
 *   1. an input that is read is not finite: m [1] (carried, step), x [2], y [3] (carried, outside), vx [4], vy [5] (carried),
 *      rho [6], p [7], h [8] (step)
 *   2. speed2 is not finite [9] (carried)
 *   3. rho > 0 does not hold [10] (step).  Before the first step rho is 0: the call is refused, and the sentence says so
 *   4. a term of a sum that is asked for is not finite, or is not below 2^(e_s) in magnitude for an explicit exponent [16 + s]
 * An offending particle counts in n and adds to nothing else.  After a refusal the outputs are unspecified; the context is not
 * poisoned and nothing of it changed.
 *
 * ONE CONTEXT (sph_ledger_compute; a plain context): two streaming passes on the context's stream -- the range pass (checks, keys,
 * counts, max |t| as f64 bits) and the sum pass -- and two waits.
 *
 * SLAB CONTEXTS, one call per stage, the first and the third local to the rank (no communication):
 *   RANGE    sph_slab_ledger_range -> sph_ledger_words, 200 bytes: first_bad (all ones: no owned particle offends; else
 *            (global id << 8) | reason of the smallest offending global id), n, n_outside, max_bits[s] (0 for a sum not asked for or a
 *            rank without particles), extreme[k] (keys; empty where nothing is asked).  SPH_OK whatever the data says: the verdict
 *            belongs to the fold.  Explicit exponents in `spec` are checked against (check 4); automatic ones check finiteness only
 *   FOLD     sph_ledger_fold_words (no context, host arithmetic): first_bad = the minimum, n and n_outside = the sums, max_bits = the
 *            maxima, keys = the minimum or maximum, into `folded` (may be NULL).  If a particle offends: SPH_ERR_INVALID_ARGUMENT and
 *            `msg` receives the sentence sph_ledger_compute leaves for the same offender, truncated to msg_bytes - 1 characters and
 *            always terminated (msg may be NULL).  Otherwise every SPH_LEDGER_AUTO_EXPONENT of a sum that is asked for is replaced in
 *            spec_io by the exponent of the WHOLE vector (refused above the range, "needs the exponent"); the exponent of a sum that
 *            is not asked for becomes 0.  Every rank that folds the same words gets the same spec_io and the same refusal
 *   SUMS     sph_slab_ledger_sums -> the rank's nine 128-bit sums under spec's EXPLICIT exponents.  It checks no data: range and fold
 *            come first
 *   COMPOSE  sph_ledger_compose (no context): adds the ranks' 128-bit sums, folds keys and counts, resolves.  sums: n x 9, rank-major.
 *            Refused when a rank's words name an offender
 *   sph_group_ledger: the slab contexts of one process -- range, fold, sums, compose over its members (a few hundred bytes per rank:
 *            nothing is gained by merging on the device).  Whichever member refuses, the sentence is left in member 0's sph_last_error.
 * sph_ledger_compute on a plain context and range -> fold -> sums -> compose over ANY partition of the same particles, in any order
 * of the ranks, give the same sph_ledger_result, byte for byte.
 *
 * REFUSALS (taken before anything is launched, except the data preconditions)
 *   SPH_ERR_UNSUPPORTED        sph_ledger_compute on a slab context; sph_slab_ledger_range / _sums on a plain context, a plain context
 *                              as a group member
 *   SPH_ERR_POISONED           a poisoned context
 *   SPH_ERR_INVALID_ARGUMENT   null pointers; n < 1; no `what` bit or an unknown one; an explicit exponent outside the range;
 *                              SPH_LEDGER_AUTO_EXPONENT given to sph_slab_ledger_sums or to sph_ledger_compose; a data precondition
 *   SPH_ERR_DEVICE
 * Nothing here reads a flag of the simulation state or writes anything a step reads; every launch runs on the context's stream; the
 * small buffers are allocated on first use, reused, and freed by sph_destroy.
 */
#ifndef SPH_LEDGER_H
#define SPH_LEDGER_H

#include <stdint.h>

#include "sph_ffi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPH_LEDGER_N_SUMS 9
#define SPH_LEDGER_N_EXTREMES 13
#define SPH_LEDGER_MIN_EXPONENT (-200)
#define SPH_LEDGER_MAX_EXPONENT 200
#define SPH_LEDGER_AUTO_EXPONENT 0x7fffffff
#define SPH_LEDGER_NO_OFFENDER 0xffffffffffffffffull
#define SPH_LEDGER_NO_ID 0xffffffffu

enum { SPH_LEDGER_CARRIED = 1, SPH_LEDGER_STEP_OUTPUTS = 2, SPH_LEDGER_OUTSIDE = 4 };
enum {
    SPH_LEDGER_MASS = 0, SPH_LEDGER_MOMENTUM_X, SPH_LEDGER_MOMENTUM_Y, SPH_LEDGER_MOMENT_X, SPH_LEDGER_MOMENT_Y, SPH_LEDGER_KINETIC,
    SPH_LEDGER_ANGULAR, SPH_LEDGER_VOLUME, SPH_LEDGER_COMPRESSION
};
enum {
    SPH_LEDGER_MAX_SPEED2 = 0, SPH_LEDGER_MIN_X, SPH_LEDGER_MAX_X, SPH_LEDGER_MIN_Y, SPH_LEDGER_MAX_Y, SPH_LEDGER_MIN_MASS,
    SPH_LEDGER_MAX_MASS, SPH_LEDGER_MIN_DENSITY, SPH_LEDGER_MAX_DENSITY, SPH_LEDGER_MIN_PRESSURE, SPH_LEDGER_MAX_PRESSURE,
    SPH_LEDGER_MIN_H, SPH_LEDGER_MAX_H
};

typedef struct sph_ledger_spec {
    uint32_t what;                          /* SPH_LEDGER_CARRIED | SPH_LEDGER_STEP_OUTPUTS | SPH_LEDGER_OUTSIDE */
    int32_t  exponent[SPH_LEDGER_N_SUMS];   /* e_s, or SPH_LEDGER_AUTO_EXPONENT */
} sph_ledger_spec;     /* 40 bytes */

typedef struct sph_ledger_sum {
    uint64_t lo;
    int64_t  hi;
} sph_ledger_sum;      /* 16 bytes: the integer hi * 2^64 + lo */

typedef struct sph_ledger_extreme {
    float    value;
    uint32_t id;                            /* SPH_LEDGER_NO_ID: empty */
} sph_ledger_extreme;  /* 8 bytes */

typedef struct sph_ledger_words {
    uint64_t first_bad;                         /* all ones: none; else (id << 8) | reason */
    uint64_t n, n_outside;
    uint64_t max_bits[SPH_LEDGER_N_SUMS];       /* max |t_j| per sum as f64 bits */
    uint64_t extreme[SPH_LEDGER_N_EXTREMES];    /* the keys */
} sph_ledger_words;    /* 200 bytes */

typedef struct sph_ledger_result {
    uint32_t what;
    int32_t  exponent[SPH_LEDGER_N_SUMS];       /* e_s as used */
    uint64_t n, n_outside;
    sph_ledger_sum raw[SPH_LEDGER_N_SUMS];      /* Q_s */
    double   sum[SPH_LEDGER_N_SUMS];            /* resolved */
    sph_ledger_extreme extreme[SPH_LEDGER_N_EXTREMES];
} sph_ledger_result;   /* 376 bytes, no padding */

/* a plain context */
int sph_ledger_compute(sph_ctx* ctx, const sph_params* params, const sph_ledger_spec* spec, sph_ledger_result* out);
/* local to the rank (slab contexts) */
int sph_slab_ledger_range(sph_ctx* ctx, const sph_params* params, const sph_ledger_spec* spec, sph_ledger_words* out);
int sph_slab_ledger_sums(sph_ctx* ctx, const sph_params* params, const sph_ledger_spec* spec, sph_ledger_sum* out);
/* no context: the ranks' words -> explicit exponents in spec_io, or the refusal's sentence in msg; folded may be NULL */
int sph_ledger_fold_words(int n, const sph_ledger_words* words, sph_ledger_spec* spec_io, sph_ledger_words* folded, char* msg, uint64_t msg_bytes);
/* no context: sums holds n x SPH_LEDGER_N_SUMS entries, rank-major; spec holds explicit exponents */
int sph_ledger_compose(int n, const sph_ledger_words* words, const sph_ledger_sum* sums, const sph_ledger_spec* spec, sph_ledger_result* out);
/* the n slab contexts of one process that sph_group_step steps */
int sph_group_ledger(sph_ctx** ctxs, int n, const sph_params* params, const sph_ledger_spec* spec, sph_ledger_result* out);

#ifdef __cplusplus
}
#endif

#endif /* SPH_LEDGER_H */
