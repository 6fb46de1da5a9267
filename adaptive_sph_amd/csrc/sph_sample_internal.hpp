// What the field sampling of one context (sph_sample.hip), of slab contexts (sph_slab_sample.hip) and at the points of a probe set
// (sph_probe.hip) share: the words of the range pass, the terms of include/sph_sample.h (point_pair: one pair once the point is known),
// the box of a particle, the range and scatter kernels, the resolve kernel and its launcher, the parameter checks and the exponent rule.  Every operation is one IEEE f32 operation in the header's order (the library is
// compiled with -ffp-contract=off, `/` and sqrtf are correctly rounded).
//
// The range and the scatter kernel come in two compile-time variants, in the style of k_render_color<SLAB>:
//   <false>  one context: every slot is a particle, a plane row holds g.nx words -- the code sph_sample_grid launches
//   <true>   a slab context: a slot takes part only where `owned` says so (nullptr: every slot), and the planes are a BAND of `bw`
//            sample columns starting at column sx0 -- word (sy, sx - sx0) of a row of bw words
//
// Everything sits in an unnamed namespace: each of the translation units compiles its own copy of the kernels it launches.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "sph_context.hpp"
#include "sph_sample.h"
#include "sph_slab_sample.h"   // sph_slab_sample_words: the verdict the fold takes

namespace {

constexpr int kMaxCh = SPH_SAMPLE_MAX_CHANNELS;

// what the range pass and the scatter write besides the planes.  The scatter's counts are spread over kStatSlots cache lines, a wave
// adding to slot (wave index % kStatSlots): 16 384 waves adding to ONE word took 0.6 ms of a 0.65 ms launch, whatever they scattered
// (one word takes about 88 atomics per microsecond); the host adds the slots up.
constexpr int kStatSlots = 128;
struct SampleStat {
    unsigned long long n_touching, n_pairs;
    uint32_t max_footprint;
    uint32_t pad[11];               // one slot per 64-byte line
};
struct SampleRed {
    unsigned long long first_bad;   // (reference index << 8 | reason) of the smallest offending reference index; all ones: none
    uint32_t max_bits[kMaxCh];      // max |a_j| per channel as float bits
    uint32_t pad[8];
    SampleStat stat[kStatSlots];
};
static_assert(sizeof(SampleStat) == 64 && sizeof(SampleRed) == 64 + 64 * kStatSlots, "one line per slot");
enum { BAD_H = 1, BAD_V = 2, BAD_VNORM = 3, BAD_CHANNEL = 4 /* + c */ };

// the state a call reads (device order)
struct SampleIn {
    const float4* pm;      // {x, y, mass, h}
    const float2* vel;
    const uint32_t* orig;  // device slot -> reference index (a slab context: the global particle id)
    const float *rho, *pres, *constf, *lvl;
    float rest_density, max_surface_distance;
    int volume, nch;
    int values_only;       // sph_sample_field_range: check the channels' values, not h and the volume
    int field[kMaxCh], comp[kMaxCh];
    float limit[kMaxCh];   // 2^e_c, or +inf while the exponent is still to be taken from the range pass
};

struct SampleGrid {
    int nx, ny;
    float ox, oy, spacing;
    float scale[kMaxCh];   // 2^(32 - e_c)
};

__device__ __forceinline__ float channel_value(const SampleIn& a, int c, uint32_t i)
{
    switch (a.field[c]) {
    case SPH_F_DENSITY: return a.rho[i];
    case SPH_F_PRESSURE: return a.pres[i];
    case SPH_F_VELOCITY: {
        const float2 v = a.vel[i];
        return a.comp[c] ? v.y : v.x;
    }
    case SPH_F_CONSTANT_FIELD: return a.constf[i];
    default: {   // SPH_F_LEVEL_ESTIMATION
        const float d = a.lvl[i];
        return d != d ? -a.max_surface_distance : d;   // LevelEstimationState::FluidInterior
    }
    }
}

__device__ __forceinline__ float particle_volume(const SampleIn& a, float m, uint32_t i)
{
    return a.volume == SPH_SAMPLE_VOLUME_REST ? m / a.rest_density : m / a.rho[i];
}
__device__ __forceinline__ float kernel_norm(float h) { return 10.f / (SPH_SEVEN_PI * (h * h)); }

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// n: the slots; SLAB: a slot whose `owned` byte is 0 (a ghost lane) checks nothing and reduces nothing
template <bool SLAB>
__global__ __launch_bounds__(256) void k_sample_range(uint32_t n, SampleIn a, SampleRed* __restrict__ red, const uint8_t* __restrict__ owned)
{
    __shared__ uint32_t part[4][kMaxCh];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t bits[kMaxCh];
    for (int c = 0; c < kMaxCh; c++) bits[c] = 0u;
    if (i < n && (!SLAB || !owned || owned[i])) {
        const float4 A = a.pm[i];
        const float h = A.w;
        uint32_t bad = 0;
        if (a.values_only) bad = 0;
        else if (!(h > 0.f) || !(h < INFINITY)) bad = BAD_H;
        else {
            const float V = particle_volume(a, A.z, i);
            if (!(V >= 0.f) || !(V < INFINITY)) bad = BAD_V;
            else if (!(V * kernel_norm(h) < 1048576.f)) bad = BAD_VNORM;
        }
        for (int c = 0; c < a.nch; c++) {
            const float m = fabsf(channel_value(a, c, i));
            bits[c] = __float_as_uint(m);
            if (!bad && !(m < a.limit[c])) bad = BAD_CHANNEL + c;   // (inf and NaN fail against +inf too)
        }
        if (bad) atomicMin(&red->first_bad, ((unsigned long long)a.orig[i] << 8) | bad);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < a.nch; c++) {
        const uint32_t m = wave_max_u32(bits[c]);
        if (lane == 0) part[wave][c] = m;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.nch) {
        const int c = threadIdx.x;
        const uint32_t m = max(max(part[0][c], part[1][c]), max(part[2][c], part[3][c]));
        // (the word only grows: a block whose maximum is not above what it reads there has nothing to add -- one atomic per block and
        //  channel on one word was most of this launch)
        if (m > __hip_atomic_load(&red->max_bits[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&red->max_bits[c], m);
    }
}

__device__ __forceinline__ void add_i64(long long* p, long long v)
{
    if (v) (void)atomicAdd((unsigned long long*)p, (unsigned long long)v);   // (result unused: the non-returning form)
}

// The samples a particle may touch: a superset computed in float (the predicate q < 1 alone decides membership), clamped to the
// grid BEFORE the conversion to int.  False: nothing to do (a position that is not finite touches no sample).
// The predicate sees X = ox + (sx + 0.5) * spacing ROUNDED to f32: where the spacing is below the ulp of the coordinates several
// columns share one X, and a sample some columns outside the exact support passes q < 1.  So the box is padded, besides its one
// sample, by the rounding of X, of x - ox and of q measured in samples: 2^-21 (|ox| + |x| + nx spacing) / spacing + 1e-5 rs, more
// than the three roundings can add up to (nothing for an ordinary grid, hundreds of columns for origin 1e5 at spacing 1e-4).
__device__ __forceinline__ bool sample_box(const SampleGrid& g, float x, float y, float h, int& x0, int& x1, int& y0, int& y1)
{
    const float gx = (x - g.ox) / g.spacing - 0.5f, gy = (y - g.oy) / g.spacing - 0.5f;
    const float rs = (2.f * h) / g.spacing;
    if (!(fabsf(gx) < 1e30f) || !(fabsf(gy) < 1e30f) || !(rs >= 0.f)) return false;
    const float px = rs + (((fabsf(g.ox) + fabsf(x)) + (float)g.nx * g.spacing) * 4.8e-7f) / g.spacing + rs * 1e-5f;
    const float py = rs + (((fabsf(g.oy) + fabsf(y)) + (float)g.ny * g.spacing) * 4.8e-7f) / g.spacing + rs * 1e-5f;
    const float fx0 = fmaxf(floorf(gx - px) - 1.f, 0.f), fx1 = fminf(ceilf(gx + px) + 1.f, (float)(g.nx - 1));
    const float fy0 = fmaxf(floorf(gy - py) - 1.f, 0.f), fy1 = fminf(ceilf(gy + py) + 1.f, (float)(g.ny - 1));
    if (!(fx0 <= fx1) || !(fy0 <= fy1)) return false;
    x0 = (int)fx0;
    x1 = (int)fx1;
    y0 = (int)fy0;
    y1 = (int)fy1;
    return true;
}

// One (particle, point) pair once the point (X, Y) is known -- a sample's centre (sample_pair) or a probe's own two floats
// (sph_probe.hip: k_probe_scatter): the predicate, w once, the adds to every plane.  `q0`: the point's word of plane 0 (read only behind
// the predicate), plane c + 1's word lies (c + 1) * plane_stride words behind it; scale[c] = 2^(32 - e_c).  True: the particle touches
// the point.  THE terms of include/sph_sample.h: both forms call this, so they cannot drift.
template <int NCH>
__device__ __forceinline__ bool point_pair(float X, float Y, long long* __restrict__ q0, size_t plane_stride, const float* scale, float x, float y,
                                           float h, float norm, float V, const float* av)
{
    const float dx = X - x, dy = Y - y;
    const float r = sqrtf(dx * dx + dy * dy);
    const float q = r / (2.f * h);
    if (!(q < 1.f)) return false;
    const float W = norm * cubic_unnorm(q);
    const float w = V * W;
    add_i64(q0, (long long)(w * 4294967296.f));
    for (int c = 0; c < NCH; c++) {
        const float t = w * av[c];
        add_i64(q0 + (size_t)(c + 1) * plane_stride, (long long)(t * scale[c]));
    }
    return true;
}

// One (particle, sample) pair: the sample's centre, then point_pair.  True: the particle touches the sample.
// (0 <= sx < nx, 0 <= sy < ny: the caller's box is clamped to the grid; SLAB: sx0 <= sx < sx0 + bw, clamped to the band)
template <int NCH, bool SLAB>
__device__ __forceinline__ bool sample_pair(const SampleGrid& g, long long* __restrict__ planes, size_t plane_stride, int sx0, int bw, int sx, int sy,
                                            float x, float y, float h, float norm, float V, const float* av)
{
    const float X = g.ox + ((float)sx + 0.5f) * g.spacing;
    const float Y = g.oy + ((float)sy + 0.5f) * g.spacing;
    long long* q0 = SLAB ? planes + (size_t)sy * (size_t)bw + (size_t)(sx - sx0) : planes + (size_t)sy * (size_t)g.nx + (size_t)sx;
    return point_pair<NCH>(X, Y, q0, plane_stride, g.scale, x, y, h, norm, V, av);
}

// boxes above this many samples take the row passes (64 of the others: below 2^21 slots).  -DSPH_SAMPLE_FLAT_MAX_AREA=0 builds the
// comparison form of profiles/r15_sample_grid.md, every box in row passes (scripts/gpu_sample_time.py with SPH_HIP_LIBRARY)
#ifndef SPH_SAMPLE_FLAT_MAX_AREA
#define SPH_SAMPLE_FLAT_MAX_AREA (1u << 15)
#endif
constexpr uint32_t kFlatMaxArea = SPH_SAMPLE_FLAT_MAX_AREA;
static_assert(kFlatMaxArea <= (1u << 20), "64 boxes of the flat form must stay below 2^32 slots");
constexpr int kRecF = 5;                      // x, y, h, norm, V; then the channels' values

// One wave per batch of 64 particles; lane l loads particle l once and computes its box.  Two forms of "lanes across the columns":
//   flat   the boxes of the batch (each at most kFlatMaxArea samples) laid end to end, row-major: slot t belongs to the particle p with
//          prefix[p] <= t < prefix[p + 1] (a 6-step search over the wave's prefix sums in LDS), to row (t - prefix[p]) / width and
//          column (t - prefix[p]) % width of its box.  Consecutive lanes take consecutive columns of a row, of the next row, of the
//          next particle's box: every lane works whatever the footprints are -- a fine particle's box of 3 x 3 samples does not hold
//          a wave for a pass of its own (measured: profiles/r15_sample_grid.md)
//   rows   a box above kFlatMaxArea: the wave takes the particle alone, 64 columns of one row per pass
// SLAB: n counts slots; a ghost lane (owned[i] == 0) has an empty box and writes nothing; `planes` are ny rows of the bw columns from
// sx0 on, per plane.  The box of an owned particle lies inside the band by construction (k_layer_band reduced the same boxes); the
// clamp to it keeps every address inside the buffer whatever the band says.
template <int NCH, bool SLAB>
__global__ __launch_bounds__(256) void k_sample_scatter(uint32_t n, SampleIn a, SampleGrid g, long long* __restrict__ planes,
                                                        SampleRed* __restrict__ red, const uint8_t* __restrict__ owned, int sx0, int bw)
{
    __shared__ float s_rec[4][64][kRecF + (NCH > 0 ? NCH : 1)];
    __shared__ int s_box[4][64][3];        // x0, y0, width
    __shared__ uint32_t s_pref[4][64];     // exclusive prefix of the flat areas
    __shared__ uint32_t s_foot[4][64];     // samples touched per particle (flat form)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * 4u + (uint32_t)wv;
    const uint32_t i = wave * 64u + (uint32_t)lane;
    const size_t plane_stride = SLAB ? (size_t)bw * (size_t)g.ny : (size_t)g.nx * (size_t)g.ny;
    // lane l: particle l of the batch
    float mx = 0.f, my = 0.f, mh = 1.f, mnorm = 0.f, mV = 0.f;
    float ma[NCH > 0 ? NCH : 1];
    for (int c = 0; c < NCH; c++) ma[c] = 0.f;
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
    bool live = false;
    if (i < n && (!SLAB || !owned || owned[i])) {
        const float4 A = a.pm[i];
        mx = A.x;
        my = A.y;
        mh = A.w;
        mnorm = kernel_norm(mh);
        mV = particle_volume(a, A.z, i);
        for (int c = 0; c < NCH; c++) ma[c] = channel_value(a, c, i);
        live = sample_box(g, mx, my, mh, bx0, bx1, by0, by1);
        if (SLAB && live) {
            bx0 = max(bx0, sx0);
            bx1 = min(bx1, sx0 + bw - 1);
            live = bx0 <= bx1;
        }
    }
    const uint32_t bw_ = live ? (uint32_t)(bx1 - bx0 + 1) : 0u, bh = live ? (uint32_t)(by1 - by0 + 1) : 0u;   // each <= 16384
    const uint32_t box_area = bw_ * bh;                                                                      // <= 2^28
    const bool rows_form = box_area > kFlatMaxArea;
    const uint32_t area = rows_form ? 0u : box_area;
    uint32_t incl = area;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);   // <= 64 * kFlatMaxArea
    s_rec[wv][lane][0] = mx;
    s_rec[wv][lane][1] = my;
    s_rec[wv][lane][2] = mh;
    s_rec[wv][lane][3] = mnorm;
    s_rec[wv][lane][4] = mV;
    for (int c = 0; c < NCH; c++) s_rec[wv][lane][kRecF + c] = ma[c];
    s_box[wv][lane][0] = bx0;
    s_box[wv][lane][1] = by0;
    s_box[wv][lane][2] = (int)(bw_ ? bw_ : 1u);
    s_pref[wv][lane] = incl - area;
    s_foot[wv][lane] = 0u;
    __syncthreads();
    // ---- flat form
    for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
        const uint32_t t = t0 + (uint32_t)lane;
        if (t < total) {
            int p = 0;   // the last particle whose prefix is <= t: the one slot t belongs to (empty boxes share their successor's prefix)
            for (int step = 32; step > 0; step >>= 1)
                if (s_pref[wv][p + step] <= t) p += step;
            const uint32_t local = t - s_pref[wv][p];
            const uint32_t width = (uint32_t)s_box[wv][p][2];
            const uint32_t row = local / width, col = local - row * width;
            float av[NCH > 0 ? NCH : 1];
            for (int c = 0; c < NCH; c++) av[c] = s_rec[wv][p][kRecF + c];
            if (sample_pair<NCH, SLAB>(g, planes, plane_stride, sx0, bw, s_box[wv][p][0] + (int)col, s_box[wv][p][1] + (int)row, s_rec[wv][p][0],
                                       s_rec[wv][p][1], s_rec[wv][p][2], s_rec[wv][p][3], s_rec[wv][p][4], av))
                atomicAdd(&s_foot[wv][p], 1u);
        }
    }
    __syncthreads();
    uint32_t my_foot = s_foot[wv][lane];
    // ---- rows form
    unsigned long long todo = __ballot(rows_form);
    while (todo) {
        const int p = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float x = __shfl(mx, p, 64), y = __shfl(my, p, 64), h = __shfl(mh, p, 64);
        const float norm = __shfl(mnorm, p, 64), V = __shfl(mV, p, 64);
        float av[NCH > 0 ? NCH : 1];
        for (int c = 0; c < NCH; c++) av[c] = __shfl(ma[c], p, 64);
        const int x0 = __shfl(bx0, p, 64), x1 = __shfl(bx1, p, 64), y0 = __shfl(by0, p, 64), y1 = __shfl(by1, p, 64);
        uint32_t foot = 0;   // wave-uniform
        for (int sy = y0; sy <= y1; sy++)
            for (int xb = x0; xb <= x1; xb += 64) {
                const int sx = xb + lane;
                const bool touch = sx <= x1 && sample_pair<NCH, SLAB>(g, planes, plane_stride, sx0, bw, sx, sy, x, y, h, norm, V, av);
                foot += (uint32_t)__popcll(__ballot(touch));
            }
        if (lane == p) my_foot = foot;
    }
    // ---- the counts: one add per wave
    const uint32_t touching = (uint32_t)__popcll(__ballot(my_foot != 0u));
    const uint32_t maxfoot = wave_max_u32(my_foot);
    unsigned long long pairs = my_foot;
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)pairs, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(pairs >> 32), o, 64);
        pairs += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0 && touching) {
        SampleStat* st = &red->stat[wave % (uint32_t)kStatSlots];
        atomicAdd(&st->n_touching, (unsigned long long)touching);
        atomicAdd(&st->n_pairs, pairs);
        atomicMax(&st->max_footprint, maxfoot);
    }
}

struct ResolveP {
    uint32_t n_samples;
    int nch, normalize;
    float min_weight, fill;
    double scale[kMaxCh];   // 2^(e_c - 32)
};

__global__ __launch_bounds__(256) void k_sample_resolve(ResolveP r, const long long* __restrict__ planes, float* __restrict__ out)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= r.n_samples) return;
    const float weight = (float)((double)planes[s] * 2.3283064365386963e-10 /* 2^-32 */);
    out[s] = weight;
    const bool keep = weight >= r.min_weight;
    for (int c = 0; c < r.nch; c++) {
        const size_t k = (size_t)(c + 1) * r.n_samples + s;
        float v = (float)((double)planes[k] * r.scale[c]);
        if (r.normalize) v = keep ? v / weight : r.fill;
        out[k] = v;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
inline const char* field_name(int field)
{
    switch (field) {
    case SPH_F_DENSITY: return "density";
    case SPH_F_PRESSURE: return "pressure";
    case SPH_F_VELOCITY: return "velocity";
    case SPH_F_CONSTANT_FIELD: return "constant_field";
    case SPH_F_LEVEL_ESTIMATION: return "level_estimation";
    default: return nullptr;
    }
}

inline int check_channel(sph_ctx* c, int field, int component)
{
    if (!field_name(field))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: field %d cannot be sampled (density, pressure, velocity, constant_field, level_estimation)", field);
    if (component < 0 || component > (field == SPH_F_VELOCITY ? 1 : 0))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: %s has no component %d", field_name(field), component);
    return SPH_OK;
}

inline uint64_t sample_count(const sph_sample_params* sp) { return (uint64_t)sp->nx * (uint64_t)sp->ny; }
inline uint64_t value_count(const sph_sample_params* sp) { return sample_count(sp) * (uint64_t)(sp->n_channels + 1); }

// the geometry and the channels of a call, in sph_sample_grid's order
inline int check_sample_params(sph_ctx* c, const sph_sample_params* sp)
{
    if (!sp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: null sample parameters");
    if (sp->nx < 1 || sp->ny < 1 || sp->nx > SPH_SAMPLE_MAX_SIDE || sp->ny > SPH_SAMPLE_MAX_SIDE)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: %d x %d samples (1..%d per side)", sp->nx, sp->ny, SPH_SAMPLE_MAX_SIDE);
    if (sp->n_channels < 0 || sp->n_channels > kMaxCh)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: %d channels (0..%d)", sp->n_channels, kMaxCh);
    const int C = sp->n_channels;
    const uint64_t n_values = value_count(sp);
    if (n_values * 8 > SPH_SAMPLE_MAX_RAW_BYTES)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: %d planes of %d x %d samples take %llu bytes as int64 (at most %llu)", C + 1, sp->nx, sp->ny,
                       (unsigned long long)(n_values * 8), (unsigned long long)SPH_SAMPLE_MAX_RAW_BYTES);
    if (!(sp->spacing > 0.f) || !(sp->spacing < INFINITY)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: the spacing must be finite and positive");
    if (!(std::fabs(sp->origin_x) < INFINITY) || !(std::fabs(sp->origin_y) < INFINITY))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: the origin must be finite");
    if (sp->volume != SPH_SAMPLE_VOLUME_DENSITY && sp->volume != SPH_SAMPLE_VOLUME_REST)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: unknown volume mode %d", sp->volume);
    for (int k = 0; k < C; k++) {
        if (int rc = check_channel(c, sp->channels[k].field, sp->channels[k].component)) return rc;
        const int e = sp->channels[k].exponent;
        if (e != SPH_SAMPLE_AUTO_EXPONENT && (e < SPH_SAMPLE_MIN_EXPONENT || e > SPH_SAMPLE_MAX_EXPONENT))
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: channel %d: exponent %d (%d..%d, or SPH_SAMPLE_AUTO_EXPONENT)", k, e, SPH_SAMPLE_MIN_EXPONENT,
                           SPH_SAMPLE_MAX_EXPONENT);
    }
    return SPH_OK;
}

inline int check_sample_buffers(sph_ctx* c, const sph_sample_params* sp, const float* values_out, uint64_t values_bytes, const int64_t* raw_out,
                                uint64_t raw_bytes)
{
    const uint64_t n_values = value_count(sp);
    if (!values_out || values_bytes < n_values * 4)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: output buffer of %llu bytes, %llu needed", (unsigned long long)values_bytes,
                       (unsigned long long)(n_values * 4));
    if (raw_out && raw_bytes < n_values * 8)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: raw output buffer of %llu bytes, %llu needed", (unsigned long long)raw_bytes,
                       (unsigned long long)(n_values * 8));
    return SPH_OK;
}

// the arrays of the current state and the channels of `sp`: limit[k] = 2^e_k, +inf for an automatic exponent
inline SampleIn make_sample_in(sph_ctx* c, const sph_params* p, int volume)
{
    const int k = c->cur;
    SampleIn a{};
    a.pm = c->pm[c->pcur].as<float4>();
    a.vel = c->vel[k].as<float2>();
    a.orig = c->orig[k].as<uint32_t>();
    a.rho = c->rho.as<float>();
    a.pres = (c->pressure_cur ? c->p1 : c->p0).as<float>();
    a.constf = c->constf.as<float>();
    a.lvl = c->lvl[k].as<float>();
    a.rest_density = p->rest_density;
    a.max_surface_distance = p->maximum_surface_distance;
    a.volume = volume;
    return a;
}

inline SampleIn make_sample_in(sph_ctx* c, const sph_params* p, const sph_sample_params* sp)
{
    SampleIn a = make_sample_in(c, p, sp->volume);
    a.nch = sp->n_channels;
    for (int k = 0; k < sp->n_channels; k++) {
        a.field[k] = sp->channels[k].field;
        a.comp[k] = sp->channels[k].component;
        const int e = sp->channels[k].exponent;
        a.limit[k] = e == SPH_SAMPLE_AUTO_EXPONENT ? INFINITY : std::ldexp(1.f, e);
    }
    return a;
}

// the grid of `sp` with the scatter's scales of the exponents `expo`
inline SampleGrid make_sample_grid(const sph_sample_params* sp, const int* expo)
{
    SampleGrid g{};
    g.nx = sp->nx;
    g.ny = sp->ny;
    g.ox = sp->origin_x;
    g.oy = sp->origin_y;
    g.spacing = sp->spacing;
    for (int k = 0; k < sp->n_channels; k++) g.scale[k] = std::ldexp(1.f, 32 - expo[k]);
    return g;
}

// e with m < 2^e <= 2 m for m > 0 (frexp: m = f 2^e, 0.5 <= f < 1), 0 for m = 0
inline int exponent_of(float max_abs)
{
    if (!(max_abs > 0.f)) return 0;
    int e = 0;
    (void)std::frexp(max_abs, &e);
    return e;
}

// the sentence of a refused particle: `first_bad` as the range pass left it (not all ones), `limit` the channel's 2^e or +inf
inline int format_offender(char* buf, size_t bytes, unsigned long long first_bad, const int* fields, const float* limit)
{
    const unsigned long long ref = first_bad >> 8;
    const int why = (int)(first_bad & 0xffu);
    if (why == BAD_H)
        return snprintf(buf, bytes, "sample: the smoothing length is not finite and positive (particle i=%llu; before the first step h is 0)", ref);
    if (why == BAD_V) return snprintf(buf, bytes, "sample: the volume m / rho is not finite and >= 0 (particle i=%llu)", ref);
    if (why == BAD_VNORM) return snprintf(buf, bytes, "sample: volume x kernel normalisation reaches 2^20 (particle i=%llu)", ref);
    const int ch = std::min(std::max(why - BAD_CHANNEL, 0), kMaxCh - 1);
    const char* name = field_name(fields[ch]) ? field_name(fields[ch]) : "?";
    if (limit[ch] < INFINITY)
        return snprintf(buf, bytes, "sample: channel %d (%s) is not finite or not below 2^exponent = %g (particle i=%llu)", ch, name, (double)limit[ch], ref);
    return snprintf(buf, bytes, "sample: channel %d (%s) is not finite (particle i=%llu)", ch, name, ref);
}

// the exponent an automatic channel takes from the maximum the range pass found; false: above the range (`e` holds what it needs)
inline bool auto_exponent(uint32_t max_bits, int& e)
{
    e = exponent_of(__builtin_bit_cast(float, max_bits));
    if (e < SPH_SAMPLE_MIN_EXPONENT) e = SPH_SAMPLE_MIN_EXPONENT;
    return e <= SPH_SAMPLE_MAX_EXPONENT;
}

// int64 planes of `sp`'s grid -> c->smp_out (queued on c's stream)
inline int launch_resolve(sph_ctx* c, const sph_sample_params* sp, const int* expo, const long long* planes)
{
    ResolveP r{};
    r.n_samples = (uint32_t)sample_count(sp);
    r.nch = sp->n_channels;
    r.normalize = (sp->flags & SPH_SAMPLE_NORMALIZE) ? 1 : 0;
    r.min_weight = sp->min_weight;
    r.fill = sp->fill;
    for (int k = 0; k < sp->n_channels; k++) r.scale[k] = std::ldexp(1.0, expo[k] - 32);
    ProfScope ps(&c->prof, "sample_resolve", c->stream);
    hipLaunchKernelGGL(k_sample_resolve, dim3((r.n_samples + 255) / 256), dim3(256), 0, c->stream, r, planes, c->smp_out.as<float>());
    return SPH_OK;
}

// the range pass of one context (sph_sample.hip, sph_probe.hip): clears the words, checks the preconditions, reduces max |a| per channel; `out`: the words as the pass left them
inline int range_pass(sph_ctx* c, const SampleIn& a, SampleRed* out)
{
    hipStream_t s = c->stream;
    const uint32_t n = (uint32_t)c->n;
    HIPCHK(c, c->smp_red.ensure(sizeof(SampleRed)));
    HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0, sizeof(SampleRed), s));
    HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0xff, sizeof(unsigned long long), s));
    if (n) {
        ProfScope ps(&c->prof, "sample_range", s);
        hipLaunchKernelGGL(k_sample_range<false>, dim3((n + 255) / 256), dim3(256), 0, s, n, a, c->smp_red.as<SampleRed>(), (const uint8_t*)nullptr);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (out->first_bad != ~0ull) {
        char msg[400];
        format_offender(msg, sizeof msg, out->first_bad, a.field, a.limit);
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s", msg);
    }
    return SPH_OK;
}

// ---- slab contexts (sph_slab_sample.hip, sph_slab_probe.hip): the words, the range pass over the owned slots, the fold ----
// what a call on a slab context refuses of the context itself.  plain_hint: what serves a plain context instead
inline int slab_refuse(sph_ctx* c, const char* what, const char* plain_hint)
{
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s: not a slab context (%s)", what, plain_hint);
    if (c->poisoned) return c->refuse_poisoned();
    return SPH_OK;
}

// a layer or compose call takes explicit exponents only.  fold_first: the calls that give them ("... come first")
inline int refuse_auto(sph_ctx* c, const char* what, const sph_sample_params* sp, const char* fold_first)
{
    for (int k = 0; k < sp->n_channels; k++)
        if (sp->channels[k].exponent == SPH_SAMPLE_AUTO_EXPONENT)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: channel %d has an automatic exponent (%s: every rank must scatter with the exponents of the whole "
                                                     "vector)", what, k, fold_first);
    return SPH_OK;
}

inline void exponents_of(const sph_sample_params* sp, int* expo)
{
    for (int k = 0; k < kMaxCh; k++) expo[k] = k < sp->n_channels ? sp->channels[k].exponent : 0;
}

// clear c's words on its stream (the group call orders that before the range launches of the other members)
inline int clear_words(sph_ctx* c)
{
    HIPCHK(c, c->smp_red.ensure(sizeof(SampleRed)));
    HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0, sizeof(SampleRed), c->stream));
    HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0xff, sizeof(unsigned long long), c->stream));
    return SPH_OK;
}

// a slab context's range pass over its nt slots (owned: sph_slab_layers.hpp's owned_flags), on c's stream, into `red` (its own words, or
// member 0's)
inline int launch_range(sph_ctx* c, const SampleIn& a, SampleRed* red, uint32_t nt, const uint8_t* owned)
{
    if (nt) {
        ProfScope ps(&c->prof, "slab_sample_range", c->stream);
        hipLaunchKernelGGL(k_sample_range<true>, dim3((nt + 255) / 256), dim3(256), 0, c->stream, nt, a, red, owned);
    }
    HIPCHK(c, hipGetLastError());
    return SPH_OK;
}

// the verdict of the folded words: the offender's sentence, or the exponents of the whole vector in sp_io
inline int fold_words(int n, const sph_slab_sample_words* words, sph_sample_params* sp_io, char* msg, size_t msg_bytes)
{
    sph_slab_sample_words w;
    w.first_bad = ~0ull;
    for (int k = 0; k < kMaxCh; k++) w.max_bits[k] = 0u;
    for (int r = 0; r < n; r++) {
        w.first_bad = std::min<uint64_t>(w.first_bad, words[r].first_bad);
        for (int k = 0; k < kMaxCh; k++) w.max_bits[k] = std::max(w.max_bits[k], words[r].max_bits[k]);
    }
    const int C = std::min(std::max(sp_io->n_channels, 0), kMaxCh);
    int fields[kMaxCh] = {0, 0, 0, 0, 0, 0};
    float limit[kMaxCh];
    for (int k = 0; k < kMaxCh; k++) {
        const int e = k < C ? sp_io->channels[k].exponent : SPH_SAMPLE_AUTO_EXPONENT;
        if (k < C) fields[k] = sp_io->channels[k].field;
        limit[k] = e == SPH_SAMPLE_AUTO_EXPONENT ? INFINITY : std::ldexp(1.f, std::min(std::max(e, -200), 200));
    }
    if (w.first_bad != ~0ull) {
        if (msg && msg_bytes) format_offender(msg, msg_bytes, w.first_bad, fields, limit);
        return SPH_ERR_INVALID_ARGUMENT;
    }
    for (int k = 0; k < C; k++) {
        if (sp_io->channels[k].exponent != SPH_SAMPLE_AUTO_EXPONENT) continue;
        int e = 0;
        if (!auto_exponent(w.max_bits[k], e)) {
            if (msg && msg_bytes)
                snprintf(msg, msg_bytes, "sample: channel %d (%s) needs the exponent %d (at most %d)", k, field_name(fields[k]) ? field_name(fields[k]) : "?", e,
                         SPH_SAMPLE_MAX_EXPONENT);
            return SPH_ERR_INVALID_ARGUMENT;
        }
        sp_io->channels[k].exponent = e;
    }
    if (msg && msg_bytes) msg[0] = 0;
    return SPH_OK;
}

// the counts the scatter left in `red`'s slots
inline void fold_stats(const SampleRed& red, sph_sample_info* info)
{
    info->n_touching = info->max_footprint = info->n_pairs = 0;
    for (const SampleStat& st : red.stat) {
        info->n_touching += st.n_touching;
        info->n_pairs += st.n_pairs;
        info->max_footprint = std::max<uint64_t>(info->max_footprint, st.max_footprint);
    }
}

}  // namespace
