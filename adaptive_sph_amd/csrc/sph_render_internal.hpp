// What the renderer of one context (sph_render.hip) and the renderer of slab contexts (sph_slab_render.hip) share: the colour pass,
// the disc / sample / boundary predicates of include/sph_render.h, the frame set-up and the argument checks.  Every operation is one
// IEEE f32 operation in the header's order (the library is compiled with -ffp-contract=off, `/` and sqrtf are correctly rounded).
//
// Everything sits in an unnamed namespace: each of the two translation units compiles its own copy of the kernels it launches.
#pragma once

#include <algorithm>

#include "sph_context.hpp"
#include "sph_render.h"

namespace {

constexpr int kMaxSegments = 32;

struct ColorMapP {
    int n;
    float v[SPH_RENDER_MAX_STOPS];
    float c[SPH_RENDER_MAX_STOPS][3];
};

// what the colour pass reads (device order; nullptr = the field still holds ParticleVec's default 0 / false)
struct RenderIn {
    const float4* pm;          // {x, y, mass, h} of the current state
    const float2* vel;
    const uint32_t* orig;      // device slot -> reference index (a slab context: the global particle id)
    const float *rho, *aii, *constf, *src, *pres, *lvl, *stash;
    const uint32_t* ncount;
    const uint8_t *szc, *f_surface, *f_insufficient, *f_reduced;
    const float2* prev;        // snapshot by reference index (SPH_RENDER_INTERPOLATE)
    float alpha;
    int attr;
    uint32_t flags;
    float rest_density, max_surface_distance;
    const uint32_t* pmax_bits; // Pressure: the maximum as float bits on the device (a slab layer without one: pmax below)
    float pmax;
    // MinDistanceToNeighbor: the lists sph_download_neighbors exports (k_fill_neighbors' candidates and predicate)
    GridP g;
    TileP t;
    const uint32_t *cell_start, *cxy;
    const float4* pm_lists;    // the geometry the lists were built from
    float krange;
};

struct FrameP {
    int w, h, s, ws, hs;
    float scale, cx, cy;
    float line_hw;
    int n_seg;
    float seg[kMaxSegments][4];   // sample-space endpoints
};

__device__ __forceinline__ uint32_t pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

__device__ __forceinline__ uint32_t to_u8(float c)
{
    float t = floorf(c * 255.f + 0.5f);
    t = fminf(fmaxf(t, 0.f), 255.f);
    return (uint32_t)t;
}

__device__ __forceinline__ uint32_t rgb_f(float r, float g, float b) { return pack_rgb(to_u8(r), to_u8(g), to_u8(b)); }

// ColorMap::get (color_map.rs:14-30)
__device__ uint32_t cmap_get(const ColorMapP& m, float x)
{
    const int last = m.n - 1;
    if (!(x == x) || x <= m.v[0]) return rgb_f(m.c[0][0], m.c[0][1], m.c[0][2]);
    if (x >= m.v[last]) return rgb_f(m.c[last][0], m.c[last][1], m.c[last][2]);
    for (int k = 0; k < last; k++) {
        if (x >= m.v[k] && x <= m.v[k + 1]) {
            const float t = (x - m.v[k]) / (m.v[k + 1] - m.v[k]);
            float o[3];
            for (int ch = 0; ch < 3; ch++) o[ch] = m.c[k][ch] + t * (m.c[k + 1][ch] - m.c[k][ch]);
            return rgb_f(o[0], o[1], o[2]);
        }
    }
    return rgb_f(m.c[0][0], m.c[0][1], m.c[0][2]);   // (unreachable for ascending stops)
}

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

// SipHash-1-3, keys (0, 0), of one 8-byte little-endian message: Rust's DefaultHasher after `usize::hash`
__device__ uint64_t siphash13_u64(uint64_t m)
{
    uint64_t v0 = 0x736f6d6570736575ull, v1 = 0x646f72616e646f6dull, v2 = 0x6c7967656e657261ull, v3 = 0x7465646279746573ull;
    auto round = [&]() {
        v0 += v1; v1 = rotl64(v1, 13); v1 ^= v0; v0 = rotl64(v0, 32);
        v2 += v3; v3 = rotl64(v3, 16); v3 ^= v2;
        v0 += v3; v3 = rotl64(v3, 21); v3 ^= v0;
        v2 += v1; v1 = rotl64(v1, 17); v1 ^= v2; v2 = rotl64(v2, 32);
    };
    v3 ^= m;
    round();
    v0 ^= m;
    const uint64_t b = 8ull << 56;
    v3 ^= b;
    round();
    v0 ^= b;
    v2 ^= 0xffull;
    round();
    round();
    round();
    return v0 ^ v1 ^ v2 ^ v3;
}

// max(0, max_i p_i) as float bits: block reduction + one u32 atomicMax per block (p >= 0: the bit order is the value order; the
// result does not depend on the order of the blocks).  `owned` (a slab context behind a step): ghost slots are left out.
__global__ __launch_bounds__(256) void k_render_pmax(uint32_t n, const float* __restrict__ p, const uint8_t* __restrict__ owned,
                                                      uint32_t* __restrict__ out)
{
    __shared__ uint32_t red[256];
    uint32_t best = 0;   // fold(0., FT::max): a NaN or a value <= 0 leaves the accumulator
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (owned && !owned[i]) continue;
        const float v = p[i];
        if (v > 0.f) best = max(best, __float_as_uint(v));
    }
    red[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicMax(out, red[0]);
}

// MinDistanceToNeighbor: min over j in list(i), j != i, of |x_i - x_j| / h_i, chained with 2 (colors.rs:460-472)
__device__ float min_distance_to_neighbor(const RenderIn& a, uint32_t i, float4 Ai)
{
    const float4 Li = a.pm_lists[i];
    const uint32_t c = a.cxy[i];
    const int cx = c & 0xffffu, cy = c >> 16;
    const int R = stencil_radius(a.g, a.t, Li.w, cx, cy, a.krange);
    float best = 2.f;
    for (int dy = -R; dy <= R; dy++) {
        const int yy = cy + dy;
        if (yy < 0 || yy >= a.g.sy) continue;
        const uint32_t b = a.cell_start[(uint32_t)yy * a.g.sx + max(cx - R, 0)];
        const uint32_t e = a.cell_start[(uint32_t)yy * a.g.sx + min(cx + R + 1, a.g.sx)];
        for (uint32_t j = b; j < e; j++) {
            const float4 Lj = a.pm_lists[j];
            const float dx = Li.x - Lj.x, dyy = Li.y - Lj.y;
            const float r2 = dx * dx + dyy * dyy;
            const float s = ((Li.w + Lj.w) * 0.5f) * a.krange;
            if (!(r2 < s * s) || j == i) continue;
            const float4 Aj = a.pm[j];
            const float ex = Ai.x - Aj.x, ey = Ai.y - Aj.y;
            const float d = sqrtf(ex * ex + ey * ey) / Ai.w;
            best = fminf(best, d);
        }
    }
    return best;
}

// One thread per slot: the colour, the render position, the radius.
//   SLAB = false  one context: the record goes to rec[reference index]
//   SLAB = true   a slab context: the arrays hold owned + ghost slots and the reference index is a GLOBAL id, which indexes no local
//                 array -- the record goes to rec[slot], ghost slots (owned[slot] == 0) write none; thread 0 also resets the three
//                 words of the band reduction that follows (band_init: min column, max column + 1, count)
template <bool SLAB>
__global__ __launch_bounds__(256) void k_render_color(uint32_t n, RenderIn a, ColorMapP m, uint4* __restrict__ rec, const uint8_t* __restrict__ owned,
                                                       uint32_t* __restrict__ band_init)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (SLAB && i == 0 && band_init) {
        band_init[0] = 0xffffffffu;
        band_init[1] = 0u;
        band_init[2] = 0u;
    }
    if (i >= n) return;
    if (SLAB && owned && !owned[i]) return;
    const uint32_t ref = a.orig[i];
    const float4 A = a.pm[i];
    float x = A.x, y = A.y;
    if (!SLAB && (a.flags & SPH_RENDER_INTERPOLATE)) {   // alpha * p_after + (1 - alpha) * p_before (animation/mod.rs:208-211)
        const float2 b = a.prev[ref];
        const float om = 1.f - a.alpha;
        x = a.alpha * x + om * b.x;
        y = a.alpha * y + om * b.y;
    }
    const float r = sqrtf((A.z / a.rest_density) * SPH_FRAC_1_PI_F);   // sphere_volume_to_radius (sph_kernels.rs:203-206)
    const bool show_surface = (a.flags & SPH_RENDER_SHOW_SURFACE) != 0;
    uint32_t rgb;
    if ((a.flags & SPH_RENDER_SHOW_NEIGHBORHOOD_REDUCED) && a.f_reduced && a.f_reduced[i]) rgb = pack_rgb(0, 255, 0);
    else if (show_surface && a.f_surface && a.f_surface[i]) rgb = pack_rgb(255, 0, 0);
    else if (show_surface && a.f_insufficient && a.f_insufficient[i]) rgb = pack_rgb(0, 255, 0);
    else {
        switch (a.attr) {
        case SPH_VIS_AII: rgb = cmap_get(m, a.aii[i]); break;
        case SPH_VIS_DISTANCE: {
            float d;
            if (a.flags & SPH_RENDER_FROM_STASH) d = a.stash ? a.stash[i] : 0.f;
            else {
                d = a.lvl[i];
                if (d != d) d = -a.max_surface_distance;   // LevelEstimationState::FluidInterior
            }
            rgb = cmap_get(m, d);
        } break;
        case SPH_VIS_PRESSURE: {
            ColorMapP pm;
            pm.n = 2;
            pm.v[0] = 0.f;
            pm.v[1] = (a.pmax_bits ? __uint_as_float(*a.pmax_bits) : a.pmax) * 0.9f;
            for (int ch = 0; ch < 3; ch++) pm.c[0][ch] = 1.f;
            pm.c[1][0] = 1.f;
            pm.c[1][1] = 0.f;
            pm.c[1][2] = 0.f;
            rgb = cmap_get(pm, a.pres[i]);
        } break;
        case SPH_VIS_VELOCITY: {
            const float2 v = a.vel[i];
            rgb = cmap_get(m, sqrtf(v.x * v.x + v.y * v.y));
        } break;
        case SPH_VIS_DENSITY: rgb = cmap_get(m, a.rho[i] / a.rest_density); break;
        case SPH_VIS_NEIGHBOR_COUNT: rgb = cmap_get(m, (float)a.ncount[i] - (SPH_ETA * 2.f) * (SPH_ETA * 2.f)); break;
        case SPH_VIS_RANDOM_COLOR: {
            const uint64_t v = siphash13_u64((uint64_t)ref);
            rgb = (uint32_t)(v & 0xffffffull);
        } break;
        case SPH_VIS_CONSTANT_FIELD: rgb = cmap_get(m, a.constf[i]); break;
        case SPH_VIS_MIN_DISTANCE_TO_NEIGHBOR: rgb = cmap_get(m, min_distance_to_neighbor(a, i, A)); break;
        case SPH_VIS_PARTICLE_SIZE_CLASS: {
            // adaptivity/mod.rs:12-23 order: TooSmall, Small, Optimal, Large, TooLarge (colors.rs:475-486)
            const uint8_t k = a.szc[i];
            rgb = k == 0 ? pack_rgb(0, 0, 255) : k == 1 ? pack_rgb(128, 128, 255) : k == 2 ? pack_rgb(255, 255, 255)
                : k == 3 ? pack_rgb(255, 128, 128) : pack_rgb(255, 0, 0);
        } break;
        case SPH_VIS_SINGLE_COLOR: rgb = pack_rgb(80, 140, 255); break;
        case SPH_VIS_SOURCE_TERM: rgb = cmap_get(m, a.src[i]); break;
        default: rgb = 0; break;
        }
    }
    rec[SLAB ? i : ref] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(r), rgb);
}

// a particle's disc in sample space (sph_render.h: "particle i")
struct Disc {
    float px, py, ro, ri;
};
__device__ __forceinline__ Disc disc_of(const FrameP& f, uint4 q)
{
    Disc d;
    d.px = f.cx + __uint_as_float(q.x) * f.scale;
    d.py = f.cy - __uint_as_float(q.y) * f.scale;
    const float r = __uint_as_float(q.z);
    d.ro = (r * 1.05f) * f.scale;
    d.ri = (r * 0.95f) * f.scale;
    return d;
}
__device__ __forceinline__ float sample_d2(const Disc& d, int sx, int sy)
{
    const float du = ((float)sx + 0.5f) - d.px, dv = ((float)sy + 0.5f) - d.py;
    return du * du + dv * dv;
}

// The samples a disc may cover: a superset (the predicate decides), clamped to the frame before the conversion to int.  False: the
// disc is not drawable (no radius, not finite) or its box misses the frame.
struct SampleBox {
    int x0, x1, y0, y1;   // inclusive
};
__device__ __forceinline__ bool disc_box(const FrameP& f, const Disc& d, SampleBox& b)
{
    if (!(d.ro > 0.f) || !(fabsf(d.px) < 1e30f) || !(fabsf(d.py) < 1e30f) || !(d.ro < 1e30f)) return false;
    const float x0 = fmaxf(floorf(d.px - d.ro) - 1.f, 0.f), x1 = fminf(ceilf(d.px + d.ro) + 1.f, (float)(f.ws - 1));
    const float y0 = fmaxf(floorf(d.py - d.ro) - 1.f, 0.f), y1 = fminf(ceilf(d.py + d.ro) + 1.f, (float)(f.hs - 1));
    if (x0 > x1 || y0 > y1) return false;
    b.x0 = (int)x0;
    b.x1 = (int)x1;
    b.y0 = (int)y0;
    b.y1 = (int)y1;
    return true;
}

// boundary strokes: butt-capped segments of half width hw (sph_render.h: "boundary")
__device__ bool on_boundary(const FrameP& f, int sx, int sy)
{
    const float u = (float)sx + 0.5f, v = (float)sy + 0.5f;
    const float hw2 = f.line_hw * f.line_hw;
    for (int k = 0; k < f.n_seg; k++) {
        const float ax = f.seg[k][0], ay = f.seg[k][1];
        const float ex = f.seg[k][2] - ax, ey = f.seg[k][3] - ay;
        const float wx = u - ax, wy = v - ay;
        const float t = wx * ex + wy * ey;
        const float L2 = ex * ex + ey * ey;
        const float c = wx * ey - wy * ex;
        if (t >= 0.f && t <= L2 && c * c < hw2 * L2) return true;
    }
    return false;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
inline bool attribute_uses_map(int attr)
{
    return !(attr == SPH_VIS_PRESSURE || attr == SPH_VIS_RANDOM_COLOR || attr == SPH_VIS_SINGLE_COLOR || attr == SPH_VIS_PARTICLE_SIZE_CLASS);
}

// the attribute and its colour map
inline int check_attribute(sph_ctx* c, const sph_render_params* rp)
{
    if (rp->attribute < 0 || rp->attribute >= SPH_VIS_COUNT_) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: unknown attribute %d", rp->attribute);
    if (attribute_uses_map(rp->attribute) && (rp->n_stops < 1 || rp->n_stops > SPH_RENDER_MAX_STOPS))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: %d colour-map stops (1..%d)", rp->n_stops, SPH_RENDER_MAX_STOPS);
    return SPH_OK;
}

// the frame geometry: S, W x H, zoom_out, the boundary segments
inline int check_frame_geometry(sph_ctx* c, const sph_render_params* rp)
{
    const int S = rp->supersample;
    if (S < 1 || S > 4) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: supersample %d (1..4)", S);
    if (rp->width < 1 || rp->height < 1 || (int64_t)rp->width * S > SPH_RENDER_MAX_SAMPLES_PER_SIDE ||
        (int64_t)rp->height * S > SPH_RENDER_MAX_SAMPLES_PER_SIDE)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: %d x %d pixels at %d x %d samples (at most %d samples per side)", rp->width, rp->height,
                       S, S, SPH_RENDER_MAX_SAMPLES_PER_SIDE);
    return SPH_OK;
}
inline int check_frame_output(sph_ctx* c, const sph_render_params* rp, const uint8_t* rgb_out, uint64_t out_bytes)
{
    const uint64_t need = (uint64_t)rp->width * (uint64_t)rp->height * 3;
    if (!rgb_out || out_bytes < need)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: output buffer of %llu bytes, %llu needed", (unsigned long long)out_bytes, (unsigned long long)need);
    return SPH_OK;
}
inline int check_frame_view(sph_ctx* c, const sph_render_params* rp)
{
    if (!(rp->zoom_out > 0.f)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: zoom_out must be positive");
    if (rp->n_segments < 0 || rp->n_segments > kMaxSegments || (rp->n_segments > 0 && !rp->segments))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: %d boundary segments (0..%d)", rp->n_segments, kMaxSegments);
    return SPH_OK;
}

inline FrameP make_frame(const sph_render_params* rp)
{
    FrameP f{};
    const int S = rp->supersample;
    f.w = rp->width;
    f.h = rp->height;
    f.s = S;
    f.ws = rp->width * S;
    f.hs = rp->height * S;
    f.scale = (float)(std::min(rp->width, rp->height) * S) / (2.f * rp->zoom_out);
    f.cx = (float)f.ws * 0.5f;
    f.cy = (float)f.hs * 0.5f;
    f.line_hw = (rp->line_width * 0.5f) * f.scale;
    f.n_seg = rp->n_segments;
    for (int k = 0; k < f.n_seg; k++) {
        const float* q = rp->segments + 4 * k;
        f.seg[k][0] = f.cx + q[0] * f.scale;
        f.seg[k][1] = f.cy - q[1] * f.scale;
        f.seg[k][2] = f.cx + q[2] * f.scale;
        f.seg[k][3] = f.cy - q[3] * f.scale;
    }
    return f;
}

// the colour pass's view of the context's state (slot order: the same arrays on one context and on a slab)
inline RenderIn make_render_in(sph_ctx* c, const sph_params* p, const sph_render_params* rp)
{
    const int k = c->cur;
    RenderIn a{};
    a.pm = c->pm[c->pcur].as<float4>();
    a.vel = c->vel[k].as<float2>();
    a.orig = c->orig[k].as<uint32_t>();
    a.rho = c->rho.as<float>();
    a.aii = c->aii.as<float>();
    a.constf = c->constf.as<float>();
    a.src = c->src.as<float>();
    a.pres = (c->pressure_cur ? c->p1 : c->p0).as<float>();
    a.lvl = c->lvl[k].as<float>();
    a.stash = c->have_level ? c->stash.as<float>() : nullptr;
    a.ncount = c->ncount.as<uint32_t>();
    a.szc = c->szc[k].as<uint8_t>();
    a.f_surface = c->have_level ? c->flag_surface.as<uint8_t>() : nullptr;
    a.f_insufficient = c->have_level ? c->flag_insufficient.as<uint8_t>() : nullptr;
    a.f_reduced = c->have_reduced ? c->flag_reduced.as<uint8_t>() : nullptr;
    a.flags = rp->flags & ~(uint32_t)SPH_RENDER_INTERPOLATE;
    a.attr = rp->attribute;
    a.rest_density = p->rest_density;
    a.max_surface_distance = p->maximum_surface_distance;
    if (rp->attribute == SPH_VIS_MIN_DISTANCE_TO_NEIGHBOR) {   // the candidates and predicate of sph_download_neighbors (sph_api.hip)
        a.g = c->fgrid;
        a.cell_start = c->cell_start.as<uint32_t>();
        a.cxy = c->cxy.as<uint32_t>();
        if (!c->lists_after) {
            a.t = TileP{c->tile_ts, c->tile_tsx, c->tile_tsy, c->tile_h.as<uint32_t>(), 0.f};
            a.pm_lists = c->pm[c->pcur ^ 1].as<float4>();
            a.krange = 2.f;
        } else {
            a.t = TileP{c->tile_ts, c->tile_tsx, c->tile_tsy, c->tile_h_ext.as<uint32_t>(), c->lists_after_slack};
            a.pm_lists = c->pm[c->pcur].as<float4>();
            a.krange = c->lists_after_k;
        }
    }
    return a;
}

inline ColorMapP make_color_map(const sph_render_params* rp)
{
    ColorMapP m{};
    m.n = attribute_uses_map(rp->attribute) ? rp->n_stops : 1;
    for (int q = 0; q < m.n && q < SPH_RENDER_MAX_STOPS; q++) {
        m.v[q] = rp->stops[q][0];
        for (int ch = 0; ch < 3; ch++) m.c[q][ch] = rp->stops[q][1 + ch];
    }
    return m;
}

}  // namespace
