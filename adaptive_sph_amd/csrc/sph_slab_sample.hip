// include/sph_slab_sample.h: the planes of sph_sample.h sampled from slab contexts.  Every rank scatters the particles it OWNS into a
// layer of int64 sums over a band of sample columns; the planes are the sums of the ranks' layers, bit for bit the planes of one
// vector holding the same particles (integer addition is associative, every particle has one owner); then sph_sample.h's resolved
// output.  The terms, the box, the range and the scatter kernels, the resolve kernel and the parameter checks are sph_sample.hip's
// (sph_sample_internal.hpp): one definition of the arithmetic for both.
//
// Kernels (each on the stream of the context it works for; they read the state and write only the sample buffers):
//   k_sample_range<true>      one thread per slot, ghost slots skipped: the preconditions (64-bit atomicMin of global id << 8 | reason)
//                             and max |a| per channel as float bits (one u32 atomicMax per block and channel that has something to add)
//   k_layer_band<BoxColumns>  (sph_slab_layers.hpp) the boxes of the owned particles -> [min column, max column + 1) and their count:
//                             block reduction in LDS, three atomics per block that holds a live box
//   k_sample_scatter<C, true> sph_sample.hip's scatter, both forms (flat, and row passes above SPH_SAMPLE_FLAT_MAX_AREA), into the
//                             band's planes; a ghost lane has an empty box
//   k_sample_merge            one launch per layer, in stream order: plain 64-bit loads and stores of dst + src over the layer's columns
//                             of the (C+1) x ny x nx planes, no atomics (the planes were cleared by a memset before the first)
//   k_sample_resolve          the shared resolve
// The band must reach the host before the layer can be allocated for it: one 12-byte copy and one wait per layer call.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sph_slab_sample.h"
#include "sph_sample_internal.hpp"
#include "sph_slab_layers.hpp"

static_assert(sizeof(sph_slab_sample_words) == 32 && sizeof(sph_sample_band) == 16, "the sizes sph_slab_sample.h states");
static_assert(offsetof(SampleRed, max_bits) == offsetof(sph_slab_sample_words, max_bits), "the verdict is the head of the range pass's words");

namespace {

using ScatterFn = void (*)(uint32_t, SampleIn, SampleGrid, long long*, SampleRed*, const uint8_t*, int, int);
const ScatterFn kScatterSlab[kMaxCh + 1] = {k_sample_scatter<0, true>, k_sample_scatter<1, true>, k_sample_scatter<2, true>, k_sample_scatter<3, true>,
                                            k_sample_scatter<4, true>, k_sample_scatter<5, true>, k_sample_scatter<6, true>};

// k_layer_band's box of a slot: the sample columns of the particle's box
struct BoxColumns {
    const float4* pm;
    SampleGrid g;
    __device__ bool operator()(uint32_t slot, int& x0, int& x1) const
    {
        const float4 A = pm[slot];
        int y0, y1;
        return sample_box(g, A.x, A.y, A.w, x0, x1, y0, y1);
    }
};

// one thread per word of the layer (planes x ny x bw): dst word (plane, sy, sx0 + bx) of the planes x ny x nx planes += src
__global__ __launch_bounds__(256) void k_sample_merge(long long* __restrict__ dst, int nx, int ny, int planes, const long long* __restrict__ src, int sx0, int bw)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t per_plane = (uint32_t)ny * (uint32_t)bw;
    if (t >= per_plane * (uint32_t)planes) return;
    const uint32_t pl = t / per_plane, rem = t - pl * per_plane;
    const uint32_t sy = rem / (uint32_t)bw, bx = rem - sy * (uint32_t)bw;
    const size_t at = ((size_t)pl * (uint32_t)ny + sy) * (uint32_t)nx + (uint32_t)sx0 + bx;
    dst[at] = dst[at] + src[t];
}

// what serves a plain context instead, and what gives a layer call its exponents
const char* const kPlainHint = "sph_sample_grid samples a plain context";
const char* const kFoldFirst = "sph_slab_sample_range and sph_sample_fold_words come first";

// everything a per-rank call refuses before it launches, in sph_sample_grid's order where it refuses the same
int check_rank_call(sph_ctx* c, const char* what, const sph_params* p, const sph_sample_params* sp)
{
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: null parameters");
    if (int rc = slab_refuse(c, what, kPlainHint)) return rc;
    return check_sample_params(c, sp);
}

// ---- a layer in two halves: up to the copy of the band words (queued), and from the band on (after the wait) ----
int layer_front(sph_ctx* c, const SampleGrid& g, uint32_t* hb)
{
    const uint32_t nt = owned_slots(c);
    hipStream_t s = c->stream;
    c->smp_layer.have = false;
    hb[0] = hb[1] = hb[2] = 0u;
    HIPCHK(c, c->smp_layer.band.ensure(4 * sizeof(uint32_t)));
    if (nt == 0) return SPH_OK;
    HIPCHK(c, hipMemsetAsync(c->smp_layer.band.p, 0, 4 * sizeof(uint32_t), s));
    HIPCHK(c, hipMemsetAsync(c->smp_layer.band.p, 0xff, sizeof(uint32_t), s));
    {
        ProfScope ps(&c->prof, "slab_sample_band", s);
        hipLaunchKernelGGL(k_layer_band<BoxColumns>, dim3((nt + 255) / 256), dim3(256), 0, s, nt, owned_flags(c), BoxColumns{c->pm[c->pcur].as<float4>(), g},
                           c->smp_layer.band.as<uint32_t>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hb, c->smp_layer.band.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return SPH_OK;
}

// the scatter into the band (queued); its counts stay in c's words until read_stats
int layer_back(sph_ctx* c, const SampleIn& a, const SampleGrid& g, const uint32_t* hb, sph_sample_band* band)
{
    hipStream_t s = c->stream;
    band_of(hb, g.nx, band->sx0, band->sx1);
    band->n_boxes = hb[2];
    band->reserved = 0;
    const int bw = band->sx1 - band->sx0;
    if (bw > 0) {
        const uint32_t nt = owned_slots(c);
        const size_t n_words = (size_t)(a.nch + 1) * (size_t)g.ny * (size_t)bw;
        HIPCHK(c, c->smp_layer.words.ensure(n_words * sizeof(long long)));
        HIPCHK(c, c->smp_red.ensure(sizeof(SampleRed)));
        HIPCHK(c, hipMemsetAsync(c->smp_layer.words.p, 0, n_words * sizeof(long long), s));
        HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0, sizeof(SampleRed), s));
        {
            ProfScope ps(&c->prof, "slab_sample_scatter", s);
            const uint32_t waves = (nt + 63) / 64;
            hipLaunchKernelGGL(kScatterSlab[a.nch], dim3((waves + 3) / 4), dim3(256), 0, s, nt, a, g, c->smp_layer.words.as<long long>(), c->smp_red.as<SampleRed>(),
                               owned_flags(c), band->sx0, bw);
        }
        HIPCHK(c, hipGetLastError());
    }
    c->smp_layer.keep(band->sx0, band->sx1, g.ny, a.nch + 1);
    return SPH_OK;
}

// the counts of the layer c scattered last (waits for c's stream); an empty band scattered nothing
int read_stats(sph_ctx* c, sph_sample_info* one)
{
    one->n_touching = one->max_footprint = one->n_pairs = 0;
    if (c->smp_layer.sx1 <= c->smp_layer.sx0) return SPH_OK;
    std::vector<SampleRed> red(1);
    HIPCHK(c, hipMemcpyAsync(&red[0], c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fold_stats(red[0], one);
    return SPH_OK;
}

// ---- compose: layers that are on c's device and ordered before this point of c's stream -> the planes in values_out / raw_out ----
int merge_and_resolve(sph_ctx* c, const sph_sample_params* sp, const std::vector<LayerRef>& L, float* values_out, int64_t* raw_out)
{
    hipStream_t s = c->stream;
    const size_t n_values = (size_t)value_count(sp);
    int expo[kMaxCh];
    exponents_of(sp, expo);
    HIPCHK(c, c->smp_planes.ensure(n_values * 8));
    HIPCHK(c, c->smp_out.ensure(n_values * 4));
    HIPCHK(c, hipMemsetAsync(c->smp_planes.p, 0, n_values * 8, s));
    for (const LayerRef& l : L) {
        if (l.sx1 <= l.sx0) continue;
        const size_t n_words = (size_t)(sp->n_channels + 1) * (size_t)sp->ny * (size_t)(l.sx1 - l.sx0);
        ProfScope ps(&c->prof, "slab_sample_merge", s);
        hipLaunchKernelGGL(k_sample_merge, dim3((uint32_t)((n_words + 255) / 256)), dim3(256), 0, s, c->smp_planes.as<long long>(), sp->nx, sp->ny,
                           sp->n_channels + 1, l.as<long long>(), l.sx0, l.sx1 - l.sx0);
    }
    launch_resolve(c, sp, expo, c->smp_planes.as<long long>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(values_out, c->smp_out.p, n_values * 4, hipMemcpyDeviceToHost, s));
    if (raw_out) HIPCHK(c, hipMemcpyAsync(raw_out, c->smp_planes.p, n_values * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

void add_info(sph_sample_info* sum, const sph_sample_info& one)
{
    sum->n_touching += one.n_touching;
    sum->n_pairs += one.n_pairs;
    sum->max_footprint = std::max(sum->max_footprint, one.max_footprint);
}

}  // namespace

extern "C" int sph_slab_sample_range(sph_ctx* c, const sph_params* p, const sph_sample_params* sp, sph_slab_sample_words* out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_sample_range: null output");
    out->first_bad = ~0ull;
    for (int k = 0; k < kMaxCh; k++) out->max_bits[k] = 0u;
    if (int rc = check_rank_call(c, "sph_slab_sample_range", p, sp)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const SampleIn a = make_sample_in(c, p, sp);
    if (int rc = clear_words(c)) return rc;
    if (int rc = launch_range(c, a, c->smp_red.as<SampleRed>(), owned_slots(c), owned_flags(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->smp_red.p, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

extern "C" int sph_sample_fold_words(int n, const sph_slab_sample_words* words, sph_sample_params* sp_io, char* msg, uint64_t msg_bytes)
{
    if (msg && msg_bytes) msg[0] = 0;
    if (n < 1 || !words || !sp_io) {
        if (msg && msg_bytes) snprintf(msg, (size_t)msg_bytes, "sph_sample_fold_words: n < 1, null words or null sample parameters");
        return SPH_ERR_INVALID_ARGUMENT;
    }
    return fold_words(n, words, sp_io, msg, (size_t)msg_bytes);
}

extern "C" int sph_slab_sample_layer(sph_ctx* c, const sph_params* p, const sph_sample_params* sp, sph_sample_band* band, sph_sample_info* info)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!band) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_sample_layer: null band");
    *band = sph_sample_band{0, 0, 0, 0};
    if (int rc = check_rank_call(c, "sph_slab_sample_layer", p, sp)) return rc;
    if (int rc = refuse_auto(c, "sph_slab_sample_layer", sp, kFoldFirst)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    int expo[kMaxCh];
    exponents_of(sp, expo);
    const SampleIn a = make_sample_in(c, p, sp);
    const SampleGrid g = make_sample_grid(sp, expo);
    uint32_t hb[3];
    if (int rc = layer_front(c, g, hb)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = layer_back(c, a, g, hb, band)) return rc;
    sph_sample_info one{};
    if (int rc = read_stats(c, &one)) return rc;   // (ends with the wait for the scatter)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (info) {
        *info = one;
        for (int k = 0; k < kMaxCh; k++) info->exponents[k] = expo[k];
    }
    return SPH_OK;
}

extern "C" int sph_slab_sample_layer_download(sph_ctx* c, int64_t* words, uint64_t capacity_words)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    return layer_download(c, c->smp_layer, "sph_slab_sample_layer", "sph_sample_grid samples a plain context", words, capacity_words);
}

extern "C" int sph_sample_compose(sph_ctx* c, const sph_sample_params* sp, int n_layers, const sph_sample_band* bands, const int64_t* const* layers,
                                  float* values_out, uint64_t values_bytes, int64_t* raw_out, uint64_t raw_bytes)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_sample_params(c, sp))) return rc;
    if ((rc = refuse_auto(c, "sph_sample_compose", sp, kFoldFirst))) return rc;
    if ((rc = check_sample_buffers(c, sp, values_out, values_bytes, raw_out, raw_bytes))) return rc;
    if (n_layers < 0 || (n_layers > 0 && !bands)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: %d layers without their bands", n_layers);
    std::vector<LayerRef> L;
    if ((rc = stage_layers(c, c->smp_layer, n_layers, bands, sp->nx, (size_t)(sp->n_channels + 1) * (size_t)sp->ny, layers, "sample", L))) return rc;
    return merge_and_resolve(c, sp, L, values_out, raw_out);
}

namespace {

int group_sample_grid(sph_ctx** ctxs, int n, const sph_params* p, const sph_sample_params* sp, float* values_out, uint64_t values_bytes, int64_t* raw_out,
                      uint64_t raw_bytes, sph_sample_info* info)
{
    sph_ctx* c0 = ctxs[0];
    int rc;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on)
            return ctxs[i]->fail(SPH_ERR_UNSUPPORTED, "sph_group_sample_grid: context %d is no slab context (sph_sample_grid samples a plain context)", i);
    for (int i = 0; i < n; i++)
        if ((rc = check_rank_call(ctxs[i], "sph_group_sample_grid", p, sp))) return rc;
    if ((rc = check_sample_buffers(c0, sp, values_out, values_bytes, raw_out, raw_bytes))) return rc;
    sph_sample_params sq = *sp;   // the exponents of the whole vector take the place of the automatic ones
    char msg[400];
    sph_sample_info sum{};

    if (!same_device(ctxs, n)) {   // the per-rank calls: the words and the layers pass through the host
        std::vector<sph_slab_sample_words> words((size_t)n);
        for (int i = 0; i < n; i++)
            if ((rc = sph_slab_sample_range(ctxs[i], p, sp, &words[(size_t)i]))) return rc;
        if ((rc = fold_words(n, words.data(), &sq, msg, sizeof msg))) return c0->fail(rc, "%s", msg);
        std::vector<sph_sample_band> bands((size_t)n);
        std::vector<std::vector<int64_t>> lay((size_t)n);
        std::vector<const int64_t*> ptrs((size_t)n, nullptr);
        for (int i = 0; i < n; i++) {
            sph_sample_info one{};
            if ((rc = sph_slab_sample_layer(ctxs[i], p, &sq, &bands[(size_t)i], &one))) return rc;
            add_info(&sum, one);
            lay[(size_t)i].resize((size_t)(sq.n_channels + 1) * (size_t)sq.ny * (size_t)(bands[(size_t)i].sx1 - bands[(size_t)i].sx0));
            if (lay[(size_t)i].empty()) continue;
            if ((rc = sph_slab_sample_layer_download(ctxs[i], lay[(size_t)i].data(), lay[(size_t)i].size()))) return rc;
            ptrs[(size_t)i] = lay[(size_t)i].data();
        }
        if ((rc = sph_sample_compose(c0, &sq, n, bands.data(), ptrs.data(), values_out, values_bytes, raw_out, raw_bytes))) return rc;
    } else {
        // ---- one device: nothing but the words, the bands and the planes crosses the bus
        HIPCHK(c0, hipSetDevice(c0->device));
        Events ev;
        HIPCHK(c0, ev.create((size_t)n + 1));
        // every member's range pass into ONE set of words (member 0's): the atomic minimum and maxima fold by themselves
        if ((rc = clear_words(c0))) return rc;
        rc = fan_in_to_first(ev, ctxs, n, [&](int i) { return launch_range(ctxs[i], make_sample_in(ctxs[i], p, sp), c0->smp_red.as<SampleRed>(), owned_slots(ctxs[i]), owned_flags(ctxs[i])); });
        if (rc) return rc;
        sph_slab_sample_words words;
        HIPCHK(c0, hipMemcpyAsync(&words, c0->smp_red.p, sizeof words, hipMemcpyDeviceToHost, c0->stream));
        HIPCHK(c0, hipStreamSynchronize(c0->stream));   // the one synchronisation before the scatter: the exponents, or the refusal
        if ((rc = fold_words(1, &words, &sq, msg, sizeof msg))) return c0->fail(rc, "%s", msg);
        int expo[kMaxCh];
        exponents_of(&sq, expo);
        const SampleGrid g = make_sample_grid(&sq, expo);
        std::vector<uint32_t> hb((size_t)n * 3, 0u);
        std::vector<LayerRef> L;
        rc = group_layers(
            ev, ctxs, n, [&](int i) { return layer_front(ctxs[i], g, &hb[(size_t)i * 3]); },
            [&](int i) {
                sph_sample_band band;
                if (int rb = layer_back(ctxs[i], make_sample_in(ctxs[i], p, &sq), g, &hb[(size_t)i * 3], &band)) return rb;
                L.push_back(LayerRef{ctxs[i]->smp_layer.words.p, band.sx0, band.sx1});
                return (int)SPH_OK;
            });
        if (rc) return rc;
        // (ends with a wait for member 0's stream, which waited for every member's layer)
        if ((rc = merge_and_resolve(c0, &sq, L, values_out, raw_out))) return rc;
        for (int i = 0; i < n; i++) {
            sph_sample_info one{};
            if ((rc = read_stats(ctxs[i], &one))) return rc;
            add_info(&sum, one);
        }
    }
    if (info) {
        exponents_of(&sq, info->exponents);
        info->n_touching = sum.n_touching;
        info->n_pairs = sum.n_pairs;
        info->max_footprint = sum.max_footprint;
    }
    return SPH_OK;
}

}  // namespace

extern "C" int sph_group_sample_grid(sph_ctx** ctxs, int n, const sph_params* p, const sph_sample_params* sp, float* values_out, uint64_t values_bytes,
                                     int64_t* raw_out, uint64_t raw_bytes, sph_sample_info* info)
{
    return group_call(ctxs, n, [&] { return group_sample_grid(ctxs, n, p, sp, values_out, values_bytes, raw_out, raw_bytes, info); });
}
