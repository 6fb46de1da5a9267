// Frames of the particle state on the device (include/sph_render.h): the colour pass of get_color_for_particle (colors.rs:386-492) and
// a rasteriser that replaces cairo's render2d (cairo_renderer.rs:19-110).  The predicates are stated in sph_render.h; every operation
// here is one IEEE f32 operation in that order (the library is compiled with -ffp-contract=off, `/` and sqrtf are correctly rounded),
// so tests/render_reference.py reproduces colours and frames byte for byte.
//
// The colour pass, the predicates and the frame set-up are shared with the renderer of slab contexts (sph_render_internal.hpp,
// sph_slab_render.hip): k_render_pmax and k_render_color live there.
//
// Kernels (all on the context's stream, reading the state, writing only the render buffers):
//   k_render_pmax     Pressure only: max(0, max_i p_i) as float bits, block reduction + one u32 atomicMax per block (p >= 0: the
//                     bit order is the value order; the result does not depend on the order of the blocks)
//   k_render_color    one thread per particle in device order: the colour, the render position, the radius -> rec[ref index]
//   k_render_scatter  one thread per particle in reference order: atomicMax(key, ref + 1) over the samples its outer disc covers
//   k_render_resolve  one thread per pixel: the S x S samples' winners (or the boundary test), averaged in integers
#include "sph_render_internal.hpp"

namespace {

__global__ __launch_bounds__(256) void k_render_scatter(uint32_t n, const uint4* __restrict__ rec, FrameP f, uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Disc d = disc_of(f, rec[i]);
    SampleBox b;
    if (!disc_box(f, d, b)) return;
    const float ro2 = d.ro * d.ro;
    for (int sy = b.y0; sy <= b.y1; sy++)
        for (int sx = b.x0; sx <= b.x1; sx++)
            if (sample_d2(d, sx, sy) < ro2) atomicMax(&keys[(uint32_t)sy * (uint32_t)f.ws + (uint32_t)sx], i + 1u);
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

int check_common(sph_ctx* c, const sph_params* p, const sph_render_params* rp)
{
    if (!p || !rp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: null parameters");
    if (c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "render: slab contexts are not supported (each rank holds only its slab of the particles)");
    if (int rc = check_attribute(c, rp)) return rc;
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
    RenderIn a = make_render_in(c, p, rp);
    a.pmax_bits = c->rnd_max.as<uint32_t>();
    if (rp->flags & SPH_RENDER_INTERPOLATE) {
        a.flags |= SPH_RENDER_INTERPOLATE;
        a.prev = c->rnd_prev.as<float2>();
        a.alpha = rp->alpha;
    }
    const ColorMapP m = make_color_map(rp);
    const uint32_t blocks = (n + 255) / 256;
    if (rp->attribute == SPH_VIS_PRESSURE) {
        ProfScope ps(&c->prof, "render_pmax", s);
        HIPCHK(c, hipMemsetAsync(c->rnd_max.p, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_render_pmax, dim3(std::min(blocks, 1024u)), dim3(256), 0, s, n, a.pres, (const uint8_t*)nullptr, c->rnd_max.as<uint32_t>());
    }
    {
        ProfScope ps(&c->prof, "render_color", s);
        hipLaunchKernelGGL(k_render_color<false>, dim3(blocks), dim3(256), 0, s, n, a, m, c->rnd_rec.as<uint4>(), (const uint8_t*)nullptr, (uint32_t*)nullptr);
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
    if ((rc = check_frame_geometry(c, rp))) return rc;
    if ((rc = check_frame_output(c, rp, rgb_out, out_bytes))) return rc;
    if ((rc = check_frame_view(c, rp))) return rc;
    const uint64_t need = (uint64_t)rp->width * (uint64_t)rp->height * 3;
    if (rp->flags & SPH_RENDER_INTERPOLATE) {
        if (!c->rnd_have_prev) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: interpolation without a snapshot (sph_render_snapshot)");
        if (c->rnd_prev_n != c->n)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: the snapshot holds %llu particles, the state %llu", (unsigned long long)c->rnd_prev_n,
                           (unsigned long long)c->n);
    }
    HIPCHK(c, hipSetDevice(c->device));
    rc = color_pass(c, p, rp);
    if (rc) return rc;

    const FrameP f = make_frame(rp);
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
