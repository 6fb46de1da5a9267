// Frames of the particle state on the device (include/sph_render.h): the colour pass of get_color_for_particle (colors.rs:386-492) and
// a rasteriser that replaces cairo's render2d (cairo_renderer.rs:19-110).  The predicates are stated in sph_render.h; every operation
// here is one IEEE f32 operation in that order (the library is compiled with -ffp-contract=off, `/` and sqrtf are correctly rounded),
// so tests/render_reference.py reproduces colours and frames byte for byte.
//
// Kernels (all on the context's stream, reading the state, writing only the render buffers):
//   k_render_pmax     Pressure only: max(0, max_i p_i) as float bits, block reduction + one u32 atomicMax per block (p >= 0: the
//                     bit order is the value order; the result does not depend on the order of the blocks)
//   k_render_color    one thread per particle in device order: the colour, the render position, the radius -> rec[ref index]
//   k_render_scatter  one thread per particle in reference order: atomicMax(key, ref + 1) over the samples its outer disc covers
//   k_render_resolve  one thread per pixel: the S x S samples' winners (or the boundary test), averaged in integers
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
    const uint32_t* orig;      // device slot -> reference index
    const float *rho, *aii, *constf, *src, *pres, *lvl, *stash;
    const uint32_t* ncount;
    const uint8_t *szc, *f_surface, *f_insufficient, *f_reduced;
    const float2* prev;        // snapshot by reference index (SPH_RENDER_INTERPOLATE)
    float alpha;
    int attr;
    uint32_t flags;
    float rest_density, max_surface_distance;
    const uint32_t* pmax_bits;
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

__global__ __launch_bounds__(256) void k_render_pmax(uint32_t n, const float* __restrict__ p, uint32_t* __restrict__ out)
{
    __shared__ uint32_t red[256];
    uint32_t best = 0;   // fold(0., FT::max): a NaN or a value <= 0 leaves the accumulator
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
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

__global__ __launch_bounds__(256) void k_render_color(uint32_t n, RenderIn a, ColorMapP m, uint4* __restrict__ rec)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t ref = a.orig[i];
    const float4 A = a.pm[i];
    float x = A.x, y = A.y;
    if (a.flags & SPH_RENDER_INTERPOLATE) {   // alpha * p_after + (1 - alpha) * p_before (animation/mod.rs:208-211)
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
            pm.v[1] = __uint_as_float(*a.pmax_bits) * 0.9f;
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
    rec[ref] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(r), rgb);
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

__global__ __launch_bounds__(256) void k_render_scatter(uint32_t n, const uint4* __restrict__ rec, FrameP f, uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Disc d = disc_of(f, rec[i]);
    if (!(d.ro > 0.f) || !(fabsf(d.px) < 1e30f) || !(fabsf(d.py) < 1e30f) || !(d.ro < 1e30f)) return;
    // a superset of the covered samples (the predicate decides), clamped to the frame before the conversion to int
    const float x0 = fmaxf(floorf(d.px - d.ro) - 1.f, 0.f), x1 = fminf(ceilf(d.px + d.ro) + 1.f, (float)(f.ws - 1));
    const float y0 = fmaxf(floorf(d.py - d.ro) - 1.f, 0.f), y1 = fminf(ceilf(d.py + d.ro) + 1.f, (float)(f.hs - 1));
    if (x0 > x1 || y0 > y1) return;
    const float ro2 = d.ro * d.ro;
    const int ix0 = (int)x0, ix1 = (int)x1, iy0 = (int)y0, iy1 = (int)y1;
    for (int sy = iy0; sy <= iy1; sy++)
        for (int sx = ix0; sx <= ix1; sx++)
            if (sample_d2(d, sx, sy) < ro2) atomicMax(&keys[(uint32_t)sy * (uint32_t)f.ws + (uint32_t)sx], i + 1u);
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

__global__ __launch_bounds__(256) void k_render_resolve(const uint4* __restrict__ rec, const uint32_t* __restrict__ keys, FrameP f,
                                                        uint8_t* __restrict__ out)
{
    const uint32_t pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= (uint32_t)f.w * (uint32_t)f.h) return;
    const int px = (int)(pix % (uint32_t)f.w), py = (int)(pix / (uint32_t)f.w);
    uint32_t acc[3] = {0, 0, 0};
    for (int j = 0; j < f.s; j++)
        for (int i = 0; i < f.s; i++) {
            const int sx = px * f.s + i, sy = py * f.s + j;
            const uint32_t key = keys[(uint32_t)sy * (uint32_t)f.ws + (uint32_t)sx];
            uint32_t rgb;
            if (key) {
                const uint4 q = rec[key - 1u];
                const Disc d = disc_of(f, q);
                rgb = sample_d2(d, sx, sy) < d.ri * d.ri ? q.w : 0u;   // the stroke band [0.95 r, 1.05 r) is black
            } else {
                rgb = on_boundary(f, sx, sy) ? 0u : 0xffffffu;
            }
            acc[0] += rgb & 0xffu;
            acc[1] += (rgb >> 8) & 0xffu;
            acc[2] += (rgb >> 16) & 0xffu;
        }
    const uint32_t ss = (uint32_t)(f.s * f.s);
    for (int ch = 0; ch < 3; ch++) out[(size_t)pix * 3 + ch] = (uint8_t)((acc[ch] + ss / 2) / ss);
}

__global__ __launch_bounds__(256) void k_render_unpack(uint32_t n, const uint4* __restrict__ rec, uint8_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t rgb = rec[i].w;
    out[(size_t)i * 3 + 0] = (uint8_t)(rgb & 0xffu);
    out[(size_t)i * 3 + 1] = (uint8_t)((rgb >> 8) & 0xffu);
    out[(size_t)i * 3 + 2] = (uint8_t)((rgb >> 16) & 0xffu);
}

__global__ __launch_bounds__(256) void k_render_snapshot(uint32_t n, const float4* __restrict__ pm, const uint32_t* __restrict__ orig,
                                                         float2* __restrict__ prev)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 A = pm[i];
    prev[orig[i]] = make_float2(A.x, A.y);
}

bool attribute_uses_map(int attr)
{
    return !(attr == SPH_VIS_PRESSURE || attr == SPH_VIS_RANDOM_COLOR || attr == SPH_VIS_SINGLE_COLOR || attr == SPH_VIS_PARTICLE_SIZE_CLASS);
}

int check_common(sph_ctx* c, const sph_params* p, const sph_render_params* rp)
{
    if (!p || !rp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: null parameters");
    if (c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "render: slab contexts are not supported (each rank holds only its slab of the particles)");
    if (rp->attribute < 0 || rp->attribute >= SPH_VIS_COUNT_) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: unknown attribute %d", rp->attribute);
    if (attribute_uses_map(rp->attribute) && (rp->n_stops < 1 || rp->n_stops > SPH_RENDER_MAX_STOPS))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: %d colour-map stops (1..%d)", rp->n_stops, SPH_RENDER_MAX_STOPS);
    if (rp->attribute == SPH_VIS_MIN_DISTANCE_TO_NEIGHBOR && !c->grid_valid)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: MinDistanceToNeighbor needs the neighbour lists of a step (none since the last change of the particle set)");
    return SPH_OK;
}

// the colour pass into c->rnd_rec (reference order)
int color_pass(sph_ctx* c, const sph_params* p, const sph_render_params* rp)
{
    const uint32_t n = (uint32_t)c->n;
    hipStream_t s = c->stream;
    HIPCHK(c, c->rnd_rec.ensure((size_t)(n ? n : 1) * sizeof(uint4)));
    HIPCHK(c, c->rnd_max.ensure(sizeof(uint32_t)));
    if (n == 0) return SPH_OK;
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
    a.pmax_bits = c->rnd_max.as<uint32_t>();
    if (rp->flags & SPH_RENDER_INTERPOLATE) {
        a.flags |= SPH_RENDER_INTERPOLATE;
        a.prev = c->rnd_prev.as<float2>();
        a.alpha = rp->alpha;
    }
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
    ColorMapP m{};
    m.n = attribute_uses_map(rp->attribute) ? rp->n_stops : 1;
    for (int q = 0; q < m.n && q < SPH_RENDER_MAX_STOPS; q++) {
        m.v[q] = rp->stops[q][0];
        for (int ch = 0; ch < 3; ch++) m.c[q][ch] = rp->stops[q][1 + ch];
    }
    const uint32_t blocks = (n + 255) / 256;
    if (rp->attribute == SPH_VIS_PRESSURE) {
        ProfScope ps(&c->prof, "render_pmax", s);
        HIPCHK(c, hipMemsetAsync(c->rnd_max.p, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_render_pmax, dim3(std::min(blocks, 1024u)), dim3(256), 0, s, n, a.pres, c->rnd_max.as<uint32_t>());
    }
    {
        ProfScope ps(&c->prof, "render_color", s);
        hipLaunchKernelGGL(k_render_color, dim3(blocks), dim3(256), 0, s, n, a, m, c->rnd_rec.as<uint4>());
    }
    HIPCHK(c, hipGetLastError());
    return SPH_OK;
}

}  // namespace

extern "C" int sph_render_snapshot(sph_ctx* c)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "render: slab contexts are not supported");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t n = (uint32_t)c->n;
    HIPCHK(c, c->rnd_prev.ensure((size_t)(n ? n : 1) * sizeof(float2)));
    if (n)
        hipLaunchKernelGGL(k_render_snapshot, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->pm[c->pcur].as<float4>(),
                           c->orig[c->cur].as<uint32_t>(), c->rnd_prev.as<float2>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rnd_prev_n = n;
    c->rnd_have_prev = true;
    return SPH_OK;
}

extern "C" int sph_render_colors(sph_ctx* c, const sph_params* p, const sph_render_params* rp, uint8_t* rgb_out, uint64_t out_bytes)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    int rc = check_common(c, p, rp);
    if (rc) return rc;
    const uint32_t n = (uint32_t)c->n;
    if (!rgb_out || out_bytes < (uint64_t)n * 3) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: output buffer of %llu bytes, %llu needed",
                                                              (unsigned long long)out_bytes, (unsigned long long)n * 3);
    HIPCHK(c, hipSetDevice(c->device));
    sph_render_params cp = *rp;
    cp.flags &= ~(uint32_t)SPH_RENDER_INTERPOLATE;   // colours do not depend on the drawn positions
    rc = color_pass(c, p, &cp);
    if (rc) return rc;
    if (n == 0) return SPH_OK;
    HIPCHK(c, c->rnd_out.ensure((size_t)n * 3));
    hipLaunchKernelGGL(k_render_unpack, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->rnd_rec.as<uint4>(), c->rnd_out.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rgb_out, c->rnd_out.p, (size_t)n * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

extern "C" int sph_render(sph_ctx* c, const sph_params* p, const sph_render_params* rp, uint8_t* rgb_out, uint64_t out_bytes)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    int rc = check_common(c, p, rp);
    if (rc) return rc;
    const int S = rp->supersample;
    if (S < 1 || S > 4) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: supersample %d (1..4)", S);
    if (rp->width < 1 || rp->height < 1 || (int64_t)rp->width * S > SPH_RENDER_MAX_SAMPLES_PER_SIDE ||
        (int64_t)rp->height * S > SPH_RENDER_MAX_SAMPLES_PER_SIDE)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: %d x %d pixels at %d x %d samples (at most %d samples per side)", rp->width, rp->height,
                       S, S, SPH_RENDER_MAX_SAMPLES_PER_SIDE);
    const uint64_t need = (uint64_t)rp->width * (uint64_t)rp->height * 3;
    if (!rgb_out || out_bytes < need)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: output buffer of %llu bytes, %llu needed", (unsigned long long)out_bytes, (unsigned long long)need);
    if (!(rp->zoom_out > 0.f)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: zoom_out must be positive");
    if (rp->n_segments < 0 || rp->n_segments > kMaxSegments || (rp->n_segments > 0 && !rp->segments))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: %d boundary segments (0..%d)", rp->n_segments, kMaxSegments);
    if (rp->flags & SPH_RENDER_INTERPOLATE) {
        if (!c->rnd_have_prev) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: interpolation without a snapshot (sph_render_snapshot)");
        if (c->rnd_prev_n != c->n)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: the snapshot holds %llu particles, the state %llu", (unsigned long long)c->rnd_prev_n,
                           (unsigned long long)c->n);
    }
    HIPCHK(c, hipSetDevice(c->device));
    rc = color_pass(c, p, rp);
    if (rc) return rc;

    FrameP f{};
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
    hipStream_t s = c->stream;
    const uint32_t n = (uint32_t)c->n;
    const size_t n_samples = (size_t)f.ws * (size_t)f.hs;
    HIPCHK(c, c->rnd_keys.ensure(n_samples * sizeof(uint32_t)));
    HIPCHK(c, c->rnd_out.ensure((size_t)need));
    HIPCHK(c, hipMemsetAsync(c->rnd_keys.p, 0, n_samples * sizeof(uint32_t), s));
    if (n) {
        ProfScope ps(&c->prof, "render_scatter", s);
        hipLaunchKernelGGL(k_render_scatter, dim3((n + 255) / 256), dim3(256), 0, s, n, c->rnd_rec.as<uint4>(), f, c->rnd_keys.as<uint32_t>());
    }
    {
        const uint32_t pixels = (uint32_t)rp->width * (uint32_t)rp->height;
        ProfScope ps(&c->prof, "render_resolve", s);
        hipLaunchKernelGGL(k_render_resolve, dim3((pixels + 255) / 256), dim3(256), 0, s, c->rnd_rec.as<uint4>(), c->rnd_keys.as<uint32_t>(), f,
                           c->rnd_out.as<uint8_t>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rgb_out, c->rnd_out.p, (size_t)need, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}
