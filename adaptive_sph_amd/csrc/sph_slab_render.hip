// include/sph_slab_render.h: the frame of sph_render.h drawn from slab contexts.  Every rank resolves the particles it OWNS into a
// layer of 64-bit words over a band of sample columns, word = (global id + 1) << 32 | rgb24; the frame's sample is the unsigned maximum
// of the ranks' words (the painter's "largest reference index wins", ids being unique), then sph_render.h's background, boundary and
// down-sampling rule.  The colour pass, the disc / sample / boundary predicates and the frame set-up are sph_render.hip's
// (sph_render_internal.hpp): one definition of the arithmetic for both renderers.
//
// Kernels (each on the stream of the context it works for; they read the state and write only the render buffers):
//   k_render_pmax          Pressure only: max(0, max p) over the owned slots as float bits (one u32 atomicMax per block)
//   k_render_color<true>   one thread per slot: colour, render position, radius -> rec[slot]; ghost slots write nothing; thread 0
//                          resets the band words (no memset launch)
//   k_layer_band<DiscColumns>  (sph_slab_layers.hpp) the clamped boxes of the owned discs -> [min column, max column + 1) and their
//                          count: block reduction in LDS, three atomics per block that drew something
//   k_slab_scatter         one thread per owned slot: 64-bit atomicMax((id + 1) << 32 | slot) over the band samples its outer disc covers
//   k_slab_layer_resolve   one thread per band sample, in place: key -> (id + 1) << 32 | (fill ? rgb : 0)
//   k_slab_merge           one launch per layer, in stream order: plain loads and stores of max(dst, src) over the layer's columns of the
//                          WS x HS word buffer; the FIRST launch covers the whole buffer and writes src or 0 (it stands in for the memset)
//   k_slab_frame_resolve   one thread per pixel: word / boundary / white of its S x S samples, averaged in integers -> RGB8
// The band must reach the host before the layer can be allocated for it: one 12-byte copy and one wait per layer call.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "sph_slab_render.h"
#include "sph_render_internal.hpp"
#include "sph_slab_layers.hpp"

namespace {

typedef unsigned long long u64;

// k_layer_band's box of a slot: the sample columns of its colour record's outer disc
struct DiscColumns {
    const uint4* rec;
    FrameP f;
    __device__ bool operator()(uint32_t slot, int& x0, int& x1) const
    {
        SampleBox b;
        if (!disc_box(f, disc_of(f, rec[slot]), b)) return false;
        x0 = b.x0;
        x1 = b.x1;
        return true;
    }
};

// keys: hs rows of the band's columns [sx0, sx1).  The box of an owned disc lies inside the band by construction (k_layer_band reduced
// the same boxes); the clamp to it keeps every address inside the buffer whatever the band says.
__global__ __launch_bounds__(256) void k_slab_scatter(uint32_t nt, const uint4* __restrict__ rec, const uint8_t* __restrict__ owned,
                                                       const uint32_t* __restrict__ orig, FrameP f, int sx0, int sx1, u64* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt || (owned && !owned[i])) return;
    const Disc d = disc_of(f, rec[i]);
    SampleBox b;
    if (!disc_box(f, d, b)) return;
    const int x0 = max(b.x0, sx0), x1 = min(b.x1, sx1 - 1);
    const float ro2 = d.ro * d.ro;
    const size_t bw = (size_t)(sx1 - sx0);
    const u64 key = (((u64)orig[i] + 1ull) << 32) | (u64)i;
    for (int sy = b.y0; sy <= b.y1; sy++)
        for (int sx = x0; sx <= x1; sx++)
            if (sample_d2(d, sx, sy) < ro2) atomicMax(&keys[(size_t)sy * bw + (size_t)(sx - sx0)], key);
}

__global__ __launch_bounds__(256) void k_slab_layer_resolve(uint32_t n_words, u64* __restrict__ buf, const uint4* __restrict__ rec, FrameP f, int sx0,
                                                             int bw)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_words) return;
    const u64 key = buf[t];
    if (!key) return;
    const uint4 q = rec[(uint32_t)key];
    const Disc d = disc_of(f, q);
    const int sx = sx0 + (int)(t % (uint32_t)bw), sy = (int)(t / (uint32_t)bw);
    const uint32_t rgb = sample_d2(d, sx, sy) < d.ri * d.ri ? q.w : 0u;   // the stroke band [0.95 r, 1.05 r) is black
    buf[t] = (key & 0xffffffff00000000ull) | (u64)rgb;
}

// init != 0: one thread per frame sample, dst = the layer's word inside its band, 0 outside (src == nullptr: 0 everywhere);
// init == 0: one thread per band sample, dst = max(dst, src)
__global__ __launch_bounds__(256) void k_slab_merge(u64* __restrict__ dst, int ws, int hs, const u64* __restrict__ src, int sx0, int sx1, int init)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t bw = (uint32_t)(sx1 - sx0);
    if (init) {
        if (t >= (uint32_t)ws * (uint32_t)hs) return;
        const int sx = (int)(t % (uint32_t)ws);
        const uint32_t sy = t / (uint32_t)ws;
        dst[t] = (src && sx >= sx0 && sx < sx1) ? src[(size_t)sy * bw + (uint32_t)(sx - sx0)] : 0ull;
    } else {
        if (t >= bw * (uint32_t)hs) return;
        const uint32_t bx = t % bw, sy = t / bw;
        const size_t at = (size_t)sy * (uint32_t)ws + (uint32_t)sx0 + bx;
        const u64 a = dst[at], b = src[t];
        if (b > a) dst[at] = b;
    }
}

// words == nullptr: no layer drew anything (every sample is background or boundary)
__global__ __launch_bounds__(256) void k_slab_frame_resolve(const u64* __restrict__ words, FrameP f, uint8_t* __restrict__ out)
{
    const uint32_t pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= (uint32_t)f.w * (uint32_t)f.h) return;
    const int px = (int)(pix % (uint32_t)f.w), py = (int)(pix / (uint32_t)f.w);
    uint32_t acc[3] = {0, 0, 0};
    for (int j = 0; j < f.s; j++)
        for (int i = 0; i < f.s; i++) {
            const int sx = px * f.s + i, sy = py * f.s + j;
            const u64 w = words ? words[(size_t)sy * (uint32_t)f.ws + (uint32_t)sx] : 0ull;
            const uint32_t rgb = w ? ((uint32_t)w & 0xffffffu) : (on_boundary(f, sx, sy) ? 0u : 0xffffffu);
            acc[0] += rgb & 0xffu;
            acc[1] += (rgb >> 8) & 0xffu;
            acc[2] += (rgb >> 16) & 0xffu;
        }
    const uint32_t ss = (uint32_t)(f.s * f.s);
    for (int ch = 0; ch < 3; ch++) out[(size_t)pix * 3 + ch] = (uint8_t)((acc[ch] + ss / 2) / ss);
}

int slab_refuse(sph_ctx* c, const char* what)
{
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s: not a slab context (sph_render draws a plain context)", what);
    if (c->poisoned) return c->refuse_poisoned();
    return SPH_OK;
}

// everything a layer call refuses, in sph_render's order where it refuses the same
int check_layer(sph_ctx* c, const char* what, const sph_params* p, const sph_render_params* rp)
{
    if (!p || !rp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: null parameters");
    if (int rc = slab_refuse(c, what)) return rc;
    if (rp->flags & SPH_RENDER_INTERPOLATE)
        return c->fail(SPH_ERR_UNSUPPORTED, "render: interpolated frames are not drawn from slab contexts (a particle may have changed rank since the snapshot)");
    if (int rc = check_attribute(c, rp)) return rc;
    if (rp->attribute == SPH_VIS_MIN_DISTANCE_TO_NEIGHBOR) {
        // (the guards of sph_download_neighbors on a slab context)
        if (!c->grid_valid || !c->have_flags)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: MinDistanceToNeighbor needs the neighbour lists of a step (none since the last change of the particle set)");
        // the ghost lanes do not integrate: their advected records are their owners' only where the step's level estimation refreshed them
        if (!c->have_level)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: MinDistanceToNeighbor on a slab needs a step with level estimation (it brings the ghosts' advected positions from their owners)");
    }
    if (int rc = check_frame_geometry(c, rp)) return rc;
    return check_frame_view(c, rp);
}

// ---- a layer in two halves: up to the copy of the band words (queued), and from the band on (after the wait) ----
int layer_front(sph_ctx* c, const sph_params* p, const sph_render_params* rp, const FrameP& f, float pmax, const uint32_t* pmax_dev, uint32_t* hb)
{
    const uint32_t nt = owned_slots(c);
    hipStream_t s = c->stream;
    c->rnd_layer.have = false;
    hb[0] = hb[1] = hb[2] = 0u;
    HIPCHK(c, c->rnd_rec.ensure((size_t)(nt ? nt : 1) * sizeof(uint4)));
    HIPCHK(c, c->rnd_layer.band.ensure(4 * sizeof(uint32_t)));
    if (nt == 0) return SPH_OK;
    RenderIn a = make_render_in(c, p, rp);
    a.pmax_bits = pmax_dev;
    a.pmax = pmax;
    const ColorMapP m = make_color_map(rp);
    const dim3 grid((nt + 255) / 256), blk(256);
    {
        ProfScope ps(&c->prof, "slab_render_color", s);
        hipLaunchKernelGGL(k_render_color<true>, grid, blk, 0, s, nt, a, m, c->rnd_rec.as<uint4>(), owned_flags(c), c->rnd_layer.band.as<uint32_t>());
    }
    {
        ProfScope ps(&c->prof, "slab_render_band", s);
        hipLaunchKernelGGL(k_layer_band<DiscColumns>, grid, blk, 0, s, nt, owned_flags(c), DiscColumns{c->rnd_rec.as<uint4>(), f}, c->rnd_layer.band.as<uint32_t>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hb, c->rnd_layer.band.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return SPH_OK;
}

int layer_back(sph_ctx* c, const FrameP& f, const uint32_t* hb, sph_render_band* band)
{
    hipStream_t s = c->stream;
    band_of(hb, f.ws, band->sx0, band->sx1);
    band->n_drawn = hb[2];
    band->reserved = 0;
    const int bw = band->sx1 - band->sx0;
    if (bw > 0) {
        const uint32_t nt = owned_slots(c);
        const size_t n_words = (size_t)bw * (size_t)f.hs;
        HIPCHK(c, c->rnd_layer.words.ensure(n_words * sizeof(u64)));
        HIPCHK(c, hipMemsetAsync(c->rnd_layer.words.p, 0, n_words * sizeof(u64), s));
        {
            ProfScope ps(&c->prof, "slab_render_scatter", s);
            hipLaunchKernelGGL(k_slab_scatter, dim3((nt + 255) / 256), dim3(256), 0, s, nt, c->rnd_rec.as<uint4>(), owned_flags(c),
                               c->orig[c->cur].as<uint32_t>(), f, band->sx0, band->sx1, c->rnd_layer.words.as<u64>());
        }
        {
            ProfScope ps(&c->prof, "slab_render_layer", s);
            hipLaunchKernelGGL(k_slab_layer_resolve, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, s, (uint32_t)n_words, c->rnd_layer.words.as<u64>(),
                               c->rnd_rec.as<uint4>(), f, band->sx0, bw);
        }
        HIPCHK(c, hipGetLastError());
    }
    c->rnd_layer.keep(band->sx0, band->sx1, f.hs, 1);
    return SPH_OK;
}

// ---- compose: layers that are on c's device and ordered before this point of c's stream -> the frame in rgb_out ----
int merge_and_resolve(sph_ctx* c, const sph_render_params* rp, const FrameP& f, const std::vector<LayerRef>& L, uint8_t* rgb_out)
{
    hipStream_t s = c->stream;
    const size_t n_samples = (size_t)f.ws * (size_t)f.hs;
    const size_t need = (size_t)rp->width * (size_t)rp->height * 3;
    HIPCHK(c, c->rnd_out.ensure(need));
    bool any = false;
    for (const LayerRef& l : L) {
        if (l.sx1 <= l.sx0) continue;
        ProfScope ps(&c->prof, "slab_render_merge", s);
        if (!any) {
            HIPCHK(c, c->rnd_words.ensure(n_samples * sizeof(u64)));
            hipLaunchKernelGGL(k_slab_merge, dim3((uint32_t)((n_samples + 255) / 256)), dim3(256), 0, s, c->rnd_words.as<u64>(), f.ws, f.hs, l.as<u64>(), l.sx0, l.sx1, 1);
            any = true;
        } else {
            const size_t n_band = (size_t)(l.sx1 - l.sx0) * (size_t)f.hs;
            hipLaunchKernelGGL(k_slab_merge, dim3((uint32_t)((n_band + 255) / 256)), dim3(256), 0, s, c->rnd_words.as<u64>(), f.ws, f.hs, l.as<u64>(), l.sx0, l.sx1, 0);
        }
    }
    {
        const uint32_t pixels = (uint32_t)rp->width * (uint32_t)rp->height;
        ProfScope ps(&c->prof, "slab_render_resolve", s);
        hipLaunchKernelGGL(k_slab_frame_resolve, dim3((pixels + 255) / 256), dim3(256), 0, s, any ? c->rnd_words.as<u64>() : (const u64*)nullptr, f,
                           c->rnd_out.as<uint8_t>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(rgb_out, c->rnd_out.p, need, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

// c's pressure maximum over its owned slots, on c's stream, into `max_bits` (its own word, or member 0's)
int launch_pmax(sph_ctx* c, uint32_t* max_bits)
{
    const uint32_t nt = owned_slots(c);
    if (nt) {
        ProfScope ps(&c->prof, "slab_render_pmax", c->stream);
        hipLaunchKernelGGL(k_render_pmax, dim3(std::min((nt + 255) / 256, 1024u)), dim3(256), 0, c->stream, nt, (c->pressure_cur ? c->p1 : c->p0).as<float>(),
                           owned_flags(c), max_bits);
    }
    HIPCHK(c, hipGetLastError());
    return SPH_OK;
}

}  // namespace

extern "C" int sph_slab_render_pressure_max(sph_ctx* c, float* out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_render_pressure_max: null output");
    *out = 0.f;
    if (int rc = slab_refuse(c, "sph_slab_render_pressure_max")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIPCHK(c, c->rnd_max.ensure(sizeof(uint32_t)));
    HIPCHK(c, hipMemsetAsync(c->rnd_max.p, 0, sizeof(uint32_t), s));
    if (int rc = launch_pmax(c, c->rnd_max.as<uint32_t>())) return rc;
    uint32_t bits = 0;
    HIPCHK(c, hipMemcpyAsync(&bits, c->rnd_max.p, sizeof bits, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    memcpy(out, &bits, sizeof bits);
    return SPH_OK;
}

extern "C" int sph_slab_render_layer(sph_ctx* c, const sph_params* p, const sph_render_params* rp, float pressure_max, sph_render_band* band)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!band) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_render_layer: null band");
    *band = sph_render_band{0, 0, 0, 0};
    if (int rc = check_layer(c, "sph_slab_render_layer", p, rp)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const FrameP f = make_frame(rp);
    uint32_t hb[3];
    if (int rc = layer_front(c, p, rp, f, pressure_max, nullptr, hb)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = layer_back(c, f, hb, band)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

extern "C" int sph_slab_render_layer_download(sph_ctx* c, uint64_t* words, uint64_t capacity_words)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    return layer_download(c, c->rnd_layer, "sph_slab_render_layer", "sph_render draws a plain context", words, capacity_words);
}

extern "C" int sph_render_compose(sph_ctx* c, const sph_render_params* rp, int n_layers, const sph_render_band* bands, const uint64_t* const* layers,
                                  uint8_t* rgb_out, uint64_t out_bytes)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!rp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: null parameters");
    int rc;
    if ((rc = check_frame_geometry(c, rp))) return rc;
    if ((rc = check_frame_output(c, rp, rgb_out, out_bytes))) return rc;
    if ((rc = check_frame_view(c, rp))) return rc;
    if (n_layers < 0 || (n_layers > 0 && !bands)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "render: %d layers without their bands", n_layers);
    const FrameP f = make_frame(rp);
    std::vector<LayerRef> L;
    if ((rc = stage_layers(c, c->rnd_layer, n_layers, bands, f.ws, (size_t)f.hs, layers, "render", L))) return rc;
    return merge_and_resolve(c, rp, f, L, rgb_out);
}

extern "C" int sph_group_render(sph_ctx** ctxs, int n, const sph_params* p, const sph_render_params* rp, uint8_t* rgb_out, uint64_t out_bytes)
{
    // Unlike sph_group_sample_grid and sph_group_ledger this is no group_call, and a plain member is an invalid argument, not unsupported:
    // the errors are neither cleared nor forwarded to member 0 (ffi.group_render joins every member's sentence and would print a
    // forwarded one twice).  Left as it is: aligning the three changes what callers see.
    if (!ctxs || n < 1) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]) return SPH_ERR_INVALID_ARGUMENT;
    sph_ctx* c0 = ctxs[0];
    int rc;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on) return ctxs[i]->fail(SPH_ERR_INVALID_ARGUMENT, "sph_group_render: context %d is no slab context (sph_render draws a plain context)", i);
    for (int i = 0; i < n; i++)
        if ((rc = check_layer(ctxs[i], "sph_group_render", p, rp))) return rc;
    if ((rc = check_frame_output(c0, rp, rgb_out, out_bytes))) return rc;
    const FrameP f = make_frame(rp);
    const bool pressure = rp->attribute == SPH_VIS_PRESSURE;

    if (!same_device(ctxs, n)) {   // the per-rank calls: the layers pass through the host
        float pmax = 0.f;
        if (pressure)
            for (int i = 0; i < n; i++) {
                float v = 0.f;
                if ((rc = sph_slab_render_pressure_max(ctxs[i], &v))) return rc;
                pmax = std::max(pmax, v);
            }
        std::vector<sph_render_band> bands((size_t)n);
        std::vector<std::vector<uint64_t>> words((size_t)n);
        std::vector<const uint64_t*> ptrs((size_t)n, nullptr);
        for (int i = 0; i < n; i++) {
            if ((rc = sph_slab_render_layer(ctxs[i], p, rp, pmax, &bands[(size_t)i]))) return rc;
            words[(size_t)i].resize((size_t)(bands[(size_t)i].sx1 - bands[(size_t)i].sx0) * (size_t)f.hs);
            if (words[(size_t)i].empty()) continue;
            if ((rc = sph_slab_render_layer_download(ctxs[i], words[(size_t)i].data(), words[(size_t)i].size()))) return rc;
            ptrs[(size_t)i] = words[(size_t)i].data();
        }
        rc = sph_render_compose(c0, rp, n, bands.data(), ptrs.data(), rgb_out, out_bytes);
        return rc;
    }

    // ---- one device: nothing but the band words and the frame crosses the bus
    HIPCHK(c0, hipSetDevice(c0->device));
    Events ev;
    HIPCHK(c0, ev.create((size_t)n + 1));
    const uint32_t* pmax_dev = nullptr;
    if (pressure) {   // every member's maximum into ONE word (member 0's); every colour pass behind all of them
        HIPCHK(c0, c0->rnd_max.ensure(sizeof(uint32_t)));
        HIPCHK(c0, hipMemsetAsync(c0->rnd_max.p, 0, sizeof(uint32_t), c0->stream));
        if ((rc = fan_in_to_first(ev, ctxs, n, [&](int i) { return launch_pmax(ctxs[i], c0->rnd_max.as<uint32_t>()); }))) return rc;
        for (int i = 1; i < n; i++)   // (member 0 has waited for every other; so does every other before it reads the word)
            for (int j = 0; j < n; j++)
                if (j != i) HIPCHK(ctxs[i], hipStreamWaitEvent(ctxs[i]->stream, ev.e[(size_t)j], 0));
        pmax_dev = c0->rnd_max.as<uint32_t>();
    }
    std::vector<uint32_t> hb((size_t)n * 3, 0u);
    std::vector<LayerRef> L;
    rc = group_layers(
        ev, ctxs, n, [&](int i) { return layer_front(ctxs[i], p, rp, f, 0.f, pmax_dev, &hb[(size_t)i * 3]); },
        [&](int i) {
            sph_render_band band;
            if (int rb = layer_back(ctxs[i], f, &hb[(size_t)i * 3], &band)) return rb;
            L.push_back(LayerRef{ctxs[i]->rnd_layer.words.p, band.sx0, band.sx1});
            return (int)SPH_OK;
        });
    if (rc) return rc;
    return merge_and_resolve(c0, rp, f, L, rgb_out);   // (ends with a wait for member 0's stream, which waited for every member's layer)
}
