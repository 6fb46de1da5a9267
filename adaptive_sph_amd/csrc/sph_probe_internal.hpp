// What the probe sets of one context (sph_probe.hip) and of slab contexts (sph_slab_probe.hip) share: the set itself, its bins, the
// scatter, touched-count and move kernels, the accumulation, the channel checks and the info struct.  The pair arithmetic is point_pair
// of sph_sample_internal.hpp.
//
// k_probe_scatter comes in two compile-time variants, in the style of k_sample_scatter<C, SLAB>:
//   <false>  one context: every slot is a particle -- the code sph_probe_sample and sph_probe_advect launch
//   <true>   a slab context: a slot takes part only where `owned` says so (nullptr: every slot); a ghost lane reaches no cell
//
// Everything but the set sits in an unnamed namespace: each translation unit compiles its own copy of the kernels it launches.
#pragma once

#include "sph_probe.h"
#include "sph_sample_internal.hpp"

struct sph_probe_set {
    sph_ctx* owner = nullptr;
    uint64_t n = 0;
    float hint = 0.f;
    float bb[4] = {0.f, 0.f, 0.f, 0.f};   // min x, min y, max x, max y of the points (n > 0)
    bool binned = false;                  // cell_start / sxy / sidx describe xy
    float cell = 0.f;                     // the geometry of the bins
    int cx = 0, cy = 0;
    DevBuf xy;                            // float2 per point, the caller's order
    DevBuf sxy, sidx;                     // the points and their caller indices in cell order
    DevBuf cellid, loc, cnt, cell_start, scan, touched;
    // sph_slab_probe.hip: the compact layer a slab rank packed last (indices ascending, then planes x n_entries words), kept until the
    // set's next layer call or its destroy; the scan of the touched flags; the staging of the layers a compose receives
    bool lay_have = false;
    uint64_t lay_entries = 0;
    int lay_planes = 0;
    DevBuf lay_idx, lay_words, lay_pos, lay_total, stage_idx, stage_words;
    void release()
    {
        for (DevBuf* b : {&xy, &sxy, &sidx, &cellid, &loc, &cnt, &cell_start, &scan, &touched, &lay_idx, &lay_words, &lay_pos, &lay_total, &stage_idx,
                          &stage_words})
            b->release();
    }
};

namespace {

struct ProbeBins {
    float x0, y0, x1, y1;   // the points' bounding box
    float s;                // cell size
    int cx, cy;
};
struct ProbeScale {
    float scale[kMaxCh];    // 2^(32 - e_c)
};
struct ProbeSlot {
    unsigned long long touched, moved, stalled, pad[5];   // one 64-byte line per slot
};
struct ProbeStat {
    uint32_t bb[4];         // ordered words of min x, min y, max x, max y behind an advect
    uint32_t pad[12];
    ProbeSlot slot[kStatSlots];
};
static_assert(sizeof(ProbeSlot) == 64 && sizeof(ProbeStat) == 64 + 64 * kStatSlots, "one line per slot");

// floats as words that order like the values
__host__ __device__ inline uint32_t ordered_of(float f)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float float_of(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __builtin_bit_cast(float, u);
}

// The cell coordinate of X along one axis: monotone in X (an f32 subtraction, a division by a positive number, floor and the clamp all
// are), so the cells of [lo, hi] contain the cell of every X in between -- the particle's range needs no rounding analysis of its own.
__device__ __forceinline__ float cell_coord(float X, float b0, float s, int nc) { return fminf(fmaxf(floorf((X - b0) / s), 0.f), (float)(nc - 1)); }

__global__ __launch_bounds__(256) void k_probe_bin_count(uint32_t n, const float2* __restrict__ xy, ProbeBins b, uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ cellid, uint32_t* __restrict__ loc)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float2 P = xy[k];
    const uint32_t c = (uint32_t)cell_coord(P.y, b.y0, b.s, b.cy) * (uint32_t)b.cx + (uint32_t)cell_coord(P.x, b.x0, b.s, b.cx);
    cellid[k] = c;
    loc[k] = atomicAdd(&cnt[c], 1u);   // (the order inside a cell is free)
}

__global__ __launch_bounds__(256) void k_probe_bin_place(uint32_t n, const float2* __restrict__ xy, const uint32_t* __restrict__ cellid,
                                                         const uint32_t* __restrict__ loc, const uint32_t* __restrict__ cell_start,
                                                         float2* __restrict__ sxy, uint32_t* __restrict__ sidx)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t at = cell_start[cellid[k]] + loc[k];   // < n: the counts add up to n
    sxy[at] = xy[k];
    sidx[at] = k;
}

// The cells a particle may reach.  |X - x| <= 2h (1 + 4 * 2^-24) for every X that passes q < 1 (the roundings of dx, of the sum of
// squares, of sqrtf and of the quotient); the reach below adds 1e-4 of the radius and 4.8e-7 of (|x| + 2h) for the rounding of
// x -+ reach itself.  False: the reach misses the points' bounding box (or the position is not finite): nothing to do.
__device__ __forceinline__ bool probe_range(const ProbeBins& b, float x, float y, float h, int& cx0, int& cx1, int& cy0, int& cy1)
{
    if (!(fabsf(x) < INFINITY) || !(fabsf(y) < INFINITY)) return false;
    const float d = 2.f * h;
    const float rx = d * 1.0001f + (fabsf(x) + d) * 4.8e-7f, ry = d * 1.0001f + (fabsf(y) + d) * 4.8e-7f;
    const float xl = x - rx, xh = x + rx, yl = y - ry, yh = y + ry;
    if (!(xl <= b.x1) || !(xh >= b.x0) || !(yl <= b.y1) || !(yh >= b.y0)) return false;
    cx0 = (int)cell_coord(xl, b.x0, b.s, b.cx);
    cx1 = (int)cell_coord(xh, b.x0, b.s, b.cx);
    cy0 = (int)cell_coord(yl, b.y0, b.s, b.cy);
    cy1 = (int)cell_coord(yh, b.y0, b.s, b.cy);
    return true;
}

// the last of 64 ascending prefixes that is <= t (empty entries share their successor's prefix)
__device__ __forceinline__ int last_at_or_below(const uint32_t* pref, uint32_t t)
{
    int p = 0;
    for (int step = 32; step > 0; step >>= 1)
        if (pref[p + step] <= t) p += step;
    return p;
}

constexpr int kProbeRecF = 5;   // x, y, h, norm, V; then the channels' values

// One block of ONE wave per 64 particles: every __syncthreads below is a barrier of that wave alone, inside loops whose trip counts are
// uniform across it.  planes: (NCH + 1) x n_points words in the caller's point order; touched: one word per point.
// SLAB: n counts slots; a ghost lane (owned[i] == 0) has no rows, like a particle that misses the points' box.
template <int NCH, bool SLAB>
__global__ __launch_bounds__(64) void k_probe_scatter(uint32_t n, SampleIn a, ProbeBins b, ProbeScale sc, const uint32_t* __restrict__ cell_start,
                                                      const float2* __restrict__ sxy, const uint32_t* __restrict__ sidx, size_t n_points,
                                                      long long* __restrict__ planes, uint32_t* __restrict__ touched, SampleRed* __restrict__ red,
                                                      const uint8_t* __restrict__ owned)
{
    __shared__ float s_rec[64][kProbeRecF + (NCH > 0 ? NCH : 1)];
    __shared__ int s_rng[64][3];         // cx0, cx1, cy0
    __shared__ uint32_t s_rpref[64];     // exclusive prefix of the particles' row counts
    __shared__ uint32_t s_hit[64];       // the particle has a non-empty segment
    __shared__ uint32_t s_foot[64];      // points touched per particle
    __shared__ uint32_t s_spref[64];     // a pass of 64 segments: exclusive prefix of their lengths,
    __shared__ uint32_t s_sstart[64];    //   their first point in cell order
    __shared__ int s_spart[64];          //   and their particle
    const int lane = threadIdx.x;
    const uint32_t wave = blockIdx.x;
    const uint32_t i = wave * 64u + (uint32_t)lane;
    float mx = 0.f, my = 0.f, mh = 1.f, mm = 0.f;
    int cx0 = 0, cx1 = 0, cy0 = 0, cy1 = -1;
    if (i < n && (!SLAB || !owned || owned[i])) {
        const float4 A = a.pm[i];
        mx = A.x;
        my = A.y;
        mm = A.z;
        mh = A.w;
        if (!probe_range(b, mx, my, mh, cx0, cx1, cy0, cy1)) cy1 = cy0 - 1;
    }
    const uint32_t rows = (uint32_t)(cy1 - cy0 + 1);   // <= cy
    uint32_t incl = rows;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= o) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);   // <= 64 * 2^22
    if (total == 0u) return;   // (the whole wave: no particle of it reaches the points' box)
    s_rng[lane][0] = cx0;
    s_rng[lane][1] = cx1;
    s_rng[lane][2] = cy0;
    s_rpref[lane] = incl - rows;
    s_hit[lane] = 0u;
    s_foot[lane] = 0u;
    __syncthreads();
    // ---- which particles reach a non-empty cell
    for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
        const uint32_t t = t0 + (uint32_t)lane;
        if (t < total) {
            const int p = last_at_or_below(s_rpref, t);
            const uint32_t base = (uint32_t)(s_rng[p][2] + (int)(t - s_rpref[p])) * (uint32_t)b.cx;
            if (cell_start[base + (uint32_t)s_rng[p][1] + 1u] != cell_start[base + (uint32_t)s_rng[p][0]]) s_hit[p] = 1u;
        }
    }
    __syncthreads();
    const bool hit = s_hit[lane] != 0u;
    if (!__ballot(hit)) return;
    s_rec[lane][0] = mx;
    s_rec[lane][1] = my;
    s_rec[lane][2] = mh;
    if (hit) {   // (only these read rho and the channels)
        s_rec[lane][3] = kernel_norm(mh);
        s_rec[lane][4] = particle_volume(a, mm, i);
        for (int c = 0; c < NCH; c++) s_rec[lane][kProbeRecF + c] = channel_value(a, c, i);
    }
    // ---- the segments, 64 at a time, and their points end to end across the lanes
    for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
        const uint32_t t = t0 + (uint32_t)lane;
        uint32_t start = 0u, len = 0u;
        int part = 0;
        if (t < total) {
            part = last_at_or_below(s_rpref, t);
            const uint32_t base = (uint32_t)(s_rng[part][2] + (int)(t - s_rpref[part])) * (uint32_t)b.cx;
            start = cell_start[base + (uint32_t)s_rng[part][0]];
            len = cell_start[base + (uint32_t)s_rng[part][1] + 1u] - start;   // <= n_points <= 2^24
        }
        uint32_t sin = len;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)sin, o, 64);
            if (lane >= o) sin += v;
        }
        const uint32_t stot = (uint32_t)__shfl((int)sin, 63, 64);   // <= 2^30
        __syncthreads();   // (the previous pass has read its segments; the first pass: s_rec is written)
        s_spref[lane] = sin - len;
        s_sstart[lane] = start;
        s_spart[lane] = part;
        __syncthreads();
        for (uint32_t u0 = 0; u0 < stot; u0 += 64u) {
            const uint32_t u = u0 + (uint32_t)lane;
            if (u < stot) {
                const int g = last_at_or_below(s_spref, u);
                const uint32_t k = s_sstart[g] + (u - s_spref[g]);   // < n_points: inside the segment's run
                const int p = s_spart[g];
                const float2 P = sxy[k];
                const uint32_t idx = sidx[k];
                float av[NCH > 0 ? NCH : 1];
                for (int c = 0; c < NCH; c++) av[c] = s_rec[p][kProbeRecF + c];
                if (point_pair<NCH>(P.x, P.y, planes + idx, n_points, sc.scale, s_rec[p][0], s_rec[p][1], s_rec[p][2], s_rec[p][3], s_rec[p][4], av)) {
                    atomicAdd(&s_foot[p], 1u);
                    touched[idx] = 1u;
                }
            }
        }
    }
    __syncthreads();
    // ---- the counts: one add per wave
    const uint32_t my_foot = s_foot[lane];
    const uint32_t touching = (uint32_t)__popcll(__ballot(my_foot != 0u));
    unsigned long long pairs = my_foot;
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)pairs, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(pairs >> 32), o, 64);
        pairs += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0 && touching) {
        SampleStat* st = &red->stat[wave % (uint32_t)kStatSlots];
        atomicAdd(&st->n_touching, (unsigned long long)touching);
        atomicAdd(&st->n_pairs, pairs);
    }
}

__global__ __launch_bounds__(256) void k_probe_touched(uint32_t n, const uint32_t* __restrict__ touched, ProbeStat* __restrict__ stat)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(k < n && touched[k] != 0u));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&stat->slot[(k >> 6) % (uint32_t)kStatSlots].touched, (unsigned long long)cnt);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// The tracer step of include/sph_probe.h: planes = weight, x, y sums in the caller's order; sx, sy = 2^(e - 32).  A grid-stride loop of
// at most kMoveBlocks blocks; a thread keeps its counts and its corner of the box in registers, the wave folds them with shuffles, the
// block through LDS, and ONE thread per block adds to the counts and the box: tracers seeded in particle order extend the box wave
// after wave, and one atomic per wave on its four words was most of this launch.
constexpr uint32_t kMoveBlocks = 1024;
__global__ __launch_bounds__(256) void k_probe_move(uint32_t n, const long long* __restrict__ planes, float2* __restrict__ xy, float dt, float min_weight,
                                                    double sx, double sy, ProbeStat* __restrict__ stat)
{
    __shared__ uint32_t s_part[4][6];
    uint32_t n_moved = 0u, n_in = 0u, lo_x = 0xffffffffu, lo_y = 0xffffffffu, hi_x = 0u, hi_y = 0u;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        float2 P = xy[k];
        const float weight = (float)((double)planes[k] * 2.3283064365386963e-10 /* 2^-32 */);
        if (weight >= min_weight) {
            const float ux = (float)((double)planes[(size_t)n + k] * sx) / weight;
            const float uy = (float)((double)planes[2 * (size_t)n + k] * sy) / weight;
            const float X = P.x + dt * ux;
            const float Y = P.y + dt * uy;
            if (fabsf(X) < INFINITY && fabsf(Y) < INFINITY) {
                n_moved++;
                P = make_float2(X, Y);
                xy[k] = P;
            }
        }
        n_in++;
        const uint32_t ox = ordered_of(P.x), oy = ordered_of(P.y);
        lo_x = min(lo_x, ox);
        lo_y = min(lo_y, oy);
        hi_x = max(hi_x, ox);
        hi_y = max(hi_y, oy);
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_moved += (uint32_t)__shfl_xor((int)n_moved, o, 64);
        n_in += (uint32_t)__shfl_xor((int)n_in, o, 64);
    }
    lo_x = wave_min_u32(lo_x);
    lo_y = wave_min_u32(lo_y);
    hi_x = wave_max_u32(hi_x);
    hi_y = wave_max_u32(hi_y);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_part[wave][0] = n_moved;
        s_part[wave][1] = n_in;
        s_part[wave][2] = lo_x;
        s_part[wave][3] = lo_y;
        s_part[wave][4] = hi_x;
        s_part[wave][5] = hi_y;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; w++) {
        n_moved += s_part[w][0];
        n_in += s_part[w][1];
        lo_x = min(lo_x, s_part[w][2]);
        lo_y = min(lo_y, s_part[w][3]);
        hi_x = max(hi_x, s_part[w][4]);
        hi_y = max(hi_y, s_part[w][5]);
    }
    if (!n_in) return;
    ProbeSlot* sl = &stat->slot[blockIdx.x % (uint32_t)kStatSlots];
    if (n_moved) atomicAdd(&sl->moved, (unsigned long long)n_moved);
    if (n_in - n_moved) atomicAdd(&sl->stalled, (unsigned long long)(n_in - n_moved));
    // (the words only shrink / grow: a block that cannot extend what it reads there has nothing to add)
    if (lo_x < __hip_atomic_load(&stat->bb[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&stat->bb[0], lo_x);
    if (lo_y < __hip_atomic_load(&stat->bb[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&stat->bb[1], lo_y);
    if (hi_x > __hip_atomic_load(&stat->bb[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&stat->bb[2], hi_x);
    if (hi_y > __hip_atomic_load(&stat->bb[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&stat->bb[3], hi_y);
}

using ProbeScatterFn = void (*)(uint32_t, SampleIn, ProbeBins, ProbeScale, const uint32_t*, const float2*, const uint32_t*, size_t, long long*, uint32_t*,
                                SampleRed*, const uint8_t*);
template <bool SLAB>
inline ProbeScatterFn probe_scatter_fn(int C)
{
    static const ProbeScatterFn table[kMaxCh + 1] = {k_probe_scatter<0, SLAB>, k_probe_scatter<1, SLAB>, k_probe_scatter<2, SLAB>, k_probe_scatter<3, SLAB>,
                                                     k_probe_scatter<4, SLAB>, k_probe_scatter<5, SLAB>, k_probe_scatter<6, SLAB>};
    return table[C];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// the handle is looked up in the context's list, never read through before that
inline int check_set(sph_ctx* c, sph_probe_set* set)
{
    if (!set || std::find(c->probe_sets.begin(), c->probe_sets.end(), set) == c->probe_sets.end())
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: not a live probe set of this context (a set belongs to the context it was created with, until "
                                                 "sph_probe_set_destroy)");
    return SPH_OK;
}

inline int check_probe_context(sph_ctx* c, const sph_params* p, sph_probe_set* set)
{
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null parameters");
    if (c->poisoned) return c->refuse_poisoned();
    if (c->dist.on)
        return c->fail(SPH_ERR_UNSUPPORTED, "probe: slab contexts are not supported (one rank holds a slab of the particles; the raw sums of disjoint particle "
                                            "sets add exactly, so the ranks' raw words compose by addition: a later form)");
    return check_set(c, set);
}

// the smallest index of a point that is not finite, and the bounding box of the points
inline int check_points(sph_ctx* c, const float* xy, uint64_t n, float* bb)
{
    if (n > SPH_PROBE_MAX_POINTS)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: %llu points (at most %llu)", (unsigned long long)n, (unsigned long long)SPH_PROBE_MAX_POINTS);
    if (n && !xy) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null points");
    bb[0] = bb[1] = INFINITY;
    bb[2] = bb[3] = -INFINITY;
    for (uint64_t k = 0; k < n; k++) {
        const float x = xy[2 * k], y = xy[2 * k + 1];
        if (!(std::fabs(x) < INFINITY) || !(std::fabs(y) < INFINITY))
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: the coordinates of a point must be finite (probe k=%llu)", (unsigned long long)k);
        bb[0] = std::min(bb[0], x);
        bb[1] = std::min(bb[1], y);
        bb[2] = std::max(bb[2], x);
        bb[3] = std::max(bb[3], y);
    }
    return SPH_OK;
}

// The geometry of the bins from the bounding box, the count and the hint.  Without a hint: about four points per cell over the box,
// and no more cells along its longer side than there are points (a line of gauges has no area: about one point per cell).  The cap: a
// size that gives more than SPH_PROBE_MAX_CELLS cells is raised until it does not.
inline void choose_bins(sph_probe_set* ps)
{
    if (!ps->n) {
        ps->cell = 0.f;
        ps->cx = ps->cy = 0;
        return;
    }
    const double ex = (double)ps->bb[2] - (double)ps->bb[0], ey = (double)ps->bb[3] - (double)ps->bb[1];
    const double e = std::max(ex, ey), cap = (double)SPH_PROBE_MAX_CELLS;
    double s = ps->hint > 0.f ? (double)ps->hint : (e > 0.0 ? std::max(2.0 * std::sqrt(ex * ey / (double)ps->n), e / (double)ps->n) : 1.0);
    s = std::max(s, std::max(std::sqrt(ex * ey / cap), e / cap));
    s = std::min(std::max(s, 1e-37), 3e38);
    float sf = (float)s;
    for (;;) {
        if ((double)sf < s) sf = std::nextafter(sf, INFINITY);
        const double nx = std::floor(ex / (double)sf) + 1.0, ny = std::floor(ey / (double)sf) + 1.0;
        if (nx * ny <= cap) {
            ps->cell = sf;
            ps->cx = (int)nx;
            ps->cy = (int)ny;
            return;
        }
        s = (double)sf * 1.02;
        sf = (float)s;
    }
}

inline ProbeBins bins_of(const sph_probe_set* ps) { return ProbeBins{ps->bb[0], ps->bb[1], ps->bb[2], ps->bb[3], ps->cell, ps->cx, ps->cy}; }

// cell_start, sxy, sidx of the set's points as they are (queued on the stream)
inline int ensure_binned(sph_ctx* c, sph_probe_set* ps)
{
    if (ps->binned) return SPH_OK;
    choose_bins(ps);
    if (!ps->n) {
        ps->binned = true;
        return SPH_OK;
    }
    hipStream_t s = c->stream;
    const uint32_t n = (uint32_t)ps->n;
    const uint32_t cells = (uint32_t)ps->cx * (uint32_t)ps->cy;
    HIPCHK(c, ps->sxy.ensure((size_t)n * 8));
    HIPCHK(c, ps->sidx.ensure((size_t)n * 4));
    HIPCHK(c, ps->cellid.ensure((size_t)n * 4));
    HIPCHK(c, ps->loc.ensure((size_t)n * 4));
    HIPCHK(c, ps->cnt.ensure(((size_t)cells + 1) * 4));
    HIPCHK(c, ps->cell_start.ensure(((size_t)cells + 1) * 4));
    HIPCHK(c, ps->scan.ensure(((size_t)cells / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
    HIPCHK(c, hipMemsetAsync(ps->cnt.p, 0, ((size_t)cells + 1) * 4, s));
    {
        ProfScope prof(&c->prof, "probe_bin", s);
        hipLaunchKernelGGL(k_probe_bin_count, dim3((n + 255) / 256), dim3(256), 0, s, n, ps->xy.as<float2>(), bins_of(ps), ps->cnt.as<uint32_t>(),
                           ps->cellid.as<uint32_t>(), ps->loc.as<uint32_t>());
        device_exclusive_scan_u32(s, ps->cnt.as<uint32_t>(), ps->cell_start.as<uint32_t>(), cells, ps->scan.as<uint32_t>(), ps->cell_start.as<uint32_t>() + cells);
        hipLaunchKernelGGL(k_probe_bin_place, dim3((n + 255) / 256), dim3(256), 0, s, n, ps->xy.as<float2>(), ps->cellid.as<uint32_t>(), ps->loc.as<uint32_t>(),
                           ps->cell_start.as<uint32_t>(), ps->sxy.as<float2>(), ps->sidx.as<uint32_t>());
    }
    HIPCHK(c, hipGetLastError());
    ps->binned = true;
    return SPH_OK;
}

inline int set_points(sph_ctx* c, sph_probe_set* ps, const float* xy, uint64_t n, const float* bb)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (n) {
        HIPCHK(c, ps->xy.ensure((size_t)n * 8));
        HIPCHK(c, hipMemcpyAsync(ps->xy.p, xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (the caller's array is free again)
    }
    ps->n = n;
    for (int k = 0; k < 4; k++) ps->bb[k] = bb[k];
    ps->binned = false;
    return ensure_binned(c, ps);
}

inline void free_set(sph_probe_set* ps)
{
    ps->release();
    delete ps;
}

// the counts of a call, cleared on c's stream (the two minima of the box start at the largest word)
inline int clear_probe_stat(sph_ctx* c)
{
    HIPCHK(c, c->prb_stat.ensure(sizeof(ProbeStat)));
    HIPCHK(c, hipMemsetAsync(c->prb_stat.p, 0, sizeof(ProbeStat), c->stream));
    HIPCHK(c, hipMemsetAsync(c->prb_stat.p, 0xff, 2 * sizeof(uint32_t), c->stream));
    return SPH_OK;
}

// `planes` planes of the set's n > 0 points in c->smp_planes and the set's touched flags, cleared on c's stream; room for the resolve
inline int clear_probe_planes(sph_ctx* c, sph_probe_set* ps, int planes)
{
    const size_t np = (size_t)ps->n, n_values = (size_t)planes * np;
    HIPCHK(c, c->smp_planes.ensure(n_values * 8));
    HIPCHK(c, c->smp_out.ensure(n_values * 4));
    HIPCHK(c, ps->touched.ensure(np * 4));
    HIPCHK(c, hipMemsetAsync(c->smp_planes.p, 0, n_values * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(ps->touched.p, 0, np * 4, c->stream));
    return SPH_OK;
}

// The accumulation both calls share: the range pass, the exponents, the bins, the planes in smp_planes ((C+1) x n words, caller order),
// the counts in smp_red / prb_stat.  sp: a grid of n x 1 samples whose channels are the call's; expo: the exponents used.  Queued, not
// waited for (the range pass itself waits).
inline int accumulate(sph_ctx* c, const sph_params* p, sph_probe_set* ps, const sph_sample_params* sp, int* expo)
{
    hipStream_t s = c->stream;
    const int C = sp->n_channels;
    const uint32_t n = (uint32_t)c->n, np = (uint32_t)ps->n;
    const SampleIn a = make_sample_in(c, p, sp);
    SampleRed red;
    if (int rc = range_pass(c, a, &red)) return rc;
    for (int k = 0; k < C; k++) {
        expo[k] = sp->channels[k].exponent;
        if (expo[k] == SPH_SAMPLE_AUTO_EXPONENT && !auto_exponent(red.max_bits[k], expo[k]))
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: channel %d (%s) needs the exponent %d (at most %d)", k, field_name(a.field[k]), expo[k],
                           SPH_SAMPLE_MAX_EXPONENT);
    }
    if (int rc = clear_probe_stat(c)) return rc;
    if (!np) return SPH_OK;
    if (int rc = ensure_binned(c, ps)) return rc;
    if (int rc = clear_probe_planes(c, ps, C + 1)) return rc;
    ProbeScale sc{};
    for (int k = 0; k < C; k++) sc.scale[k] = std::ldexp(1.f, 32 - expo[k]);
    if (n) {
        ProfScope prof(&c->prof, "probe_scatter", s);
        hipLaunchKernelGGL(probe_scatter_fn<false>(C), dim3((n + 63) / 64), dim3(64), 0, s, n, a, bins_of(ps), sc, ps->cell_start.as<uint32_t>(),
                           ps->sxy.as<float2>(), ps->sidx.as<uint32_t>(), (size_t)np, c->smp_planes.as<long long>(), ps->touched.as<uint32_t>(),
                           c->smp_red.as<SampleRed>(), (const uint8_t*)nullptr);
    }
    hipLaunchKernelGGL(k_probe_touched, dim3((np + 255) / 256), dim3(256), 0, s, np, ps->touched.as<uint32_t>(), c->prb_stat.as<ProbeStat>());
    HIPCHK(c, hipGetLastError());
    return SPH_OK;
}

inline void fill_info(sph_probe_info* info, const sph_probe_set* ps, const int* expo, const SampleRed& red, const ProbeStat& st)
{
    *info = sph_probe_info{};
    for (int k = 0; k < kMaxCh; k++) info->exponents[k] = expo[k];
    for (const SampleStat& s : red.stat) {
        info->n_touching += s.n_touching;
        info->n_pairs += s.n_pairs;
    }
    for (const ProbeSlot& s : st.slot) {
        info->n_touched_points += s.touched;
        info->n_moved += s.moved;
        info->n_stalled += s.stalled;
    }
    info->cell_size = ps->cell;
    info->cells_x = ps->cx;
    info->cells_y = ps->cy;
}

// the n x 1 grid whose channels, volume and resolve terms are the call's (spacing and origin play no part: the points are the set's)
inline sph_sample_params as_sample_params(const sph_probe_set* ps, int volume, uint32_t flags, float min_weight, float fill, int C, const sph_sample_channel* ch)
{
    sph_sample_params sp{};
    sp.nx = (int32_t)ps->n;
    sp.ny = 1;
    sp.spacing = 1.f;
    sp.volume = volume;
    sp.flags = flags;
    sp.min_weight = min_weight;
    sp.fill = fill;
    sp.n_channels = C;
    for (int k = 0; k < C && k < kMaxCh; k++) sp.channels[k] = ch[k];
    return sp;
}

// volume, channels and exponents, in check_sample_params' words
inline int check_channels(sph_ctx* c, const sph_sample_params* sp)
{
    if (sp->n_channels < 0 || sp->n_channels > kMaxCh) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: %d channels (0..%d)", sp->n_channels, kMaxCh);
    const uint64_t raw_bytes = (uint64_t)(sp->n_channels + 1) * (uint64_t)(uint32_t)sp->nx * 8;
    if (raw_bytes > SPH_SAMPLE_MAX_RAW_BYTES)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: %d planes of %u points take %llu bytes as int64 (at most %llu)", sp->n_channels + 1, (uint32_t)sp->nx,
                       (unsigned long long)raw_bytes, (unsigned long long)SPH_SAMPLE_MAX_RAW_BYTES);
    if (sp->volume != SPH_SAMPLE_VOLUME_DENSITY && sp->volume != SPH_SAMPLE_VOLUME_REST)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: unknown volume mode %d", sp->volume);
    for (int k = 0; k < sp->n_channels; k++) {
        if (int rc = check_channel(c, sp->channels[k].field, sp->channels[k].component)) return rc;
        const int e = sp->channels[k].exponent;
        if (e != SPH_SAMPLE_AUTO_EXPONENT && (e < SPH_SAMPLE_MIN_EXPONENT || e > SPH_SAMPLE_MAX_EXPONENT))
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: channel %d: exponent %d (%d..%d, or SPH_SAMPLE_AUTO_EXPONENT)", k, e, SPH_SAMPLE_MIN_EXPONENT,
                           SPH_SAMPLE_MAX_EXPONENT);
    }
    return SPH_OK;
}

}  // namespace
