// include/sph_slab_sample.h: the planes of sph_sample.h sampled from slab contexts.  Every rank scatters the particles it OWNS into a
// layer of int64 sums over a band of sample columns; the planes are the sums of the ranks' layers, bit for bit the planes of one
// vector holding the same particles (integer addition is associative, every particle has one owner); then sph_sample.h's resolved
// output.  The terms, the box, the range and the scatter kernels, the resolve kernel and the parameter checks are sph_sample.hip's
// (sph_sample_internal.hpp): one definition of the arithmetic for both.
//
// Kernels (each on the stream of the context it works for; they read the state and write only the sample buffers):
//   k_sample_range<true>      one thread per slot, ghost slots skipped: the preconditions (64-bit atomicMin of global id << 8 | reason)
//                             and max |a| per channel as float bits (one u32 atomicMax per block and channel that has something to add)
//   k_sample_band             the boxes of the owned particles -> [min column, max column + 1) and their count: block reduction in
//                             LDS, three atomics per block that holds a live box
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

static_assert(sizeof(sph_slab_sample_words) == 32 && sizeof(sph_sample_band) == 16, "the sizes sph_slab_sample.h states");
static_assert(offsetof(SampleRed, max_bits) == offsetof(sph_slab_sample_words, max_bits), "the verdict is the head of the range pass's words");

namespace {

using ScatterFn = void (*)(uint32_t, SampleIn, SampleGrid, long long*, SampleRed*, const uint8_t*, int, int);
const ScatterFn kScatterSlab[kMaxCh + 1] = {k_sample_scatter<0, true>, k_sample_scatter<1, true>, k_sample_scatter<2, true>, k_sample_scatter<3, true>,
                                            k_sample_scatter<4, true>, k_sample_scatter<5, true>, k_sample_scatter<6, true>};

// out: {min x0, max x1 + 1, live boxes} (set to {all ones, 0, 0} before the launch)
__global__ __launch_bounds__(256) void k_sample_band(uint32_t nt, const float4* __restrict__ pm, const uint8_t* __restrict__ owned, SampleGrid g,
                                                      uint32_t* __restrict__ out)
{
    __shared__ uint32_t lo[256], hi[256], cnt[256];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t l = 0xffffffffu, h = 0u, c = 0u;
    if (i < nt && (!owned || owned[i])) {
        const float4 A = pm[i];
        int x0, x1, y0, y1;
        if (sample_box(g, A.x, A.y, A.w, x0, x1, y0, y1)) {
            l = (uint32_t)x0;
            h = (uint32_t)x1 + 1u;
            c = 1u;
        }
    }
    lo[threadIdx.x] = l;
    hi[threadIdx.x] = h;
    cnt[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            lo[threadIdx.x] = min(lo[threadIdx.x], lo[threadIdx.x + s]);
            hi[threadIdx.x] = max(hi[threadIdx.x], hi[threadIdx.x + s]);
            cnt[threadIdx.x] += cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && cnt[0]) {
        atomicMin(&out[0], lo[0]);
        atomicMax(&out[1], hi[0]);
        atomicAdd(&out[2], cnt[0]);
    }
}

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

int slab_refuse(sph_ctx* c, const char* what)
{
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s: not a slab context (sph_sample_grid samples a plain context)", what);
    if (c->poisoned) return c->refuse_poisoned();
    return SPH_OK;
}

// slots in the arrays and their ownership flags: behind a step owned + ghosts, else the owned particles alone
uint32_t slab_slots(const sph_ctx* c) { return c->have_flags ? c->dist.n_tot : (uint32_t)c->n; }
const uint8_t* slab_owned(const sph_ctx* c) { return c->have_flags ? c->dist.owned.as<uint8_t>() : nullptr; }

// everything a per-rank call refuses before it launches, in sph_sample_grid's order where it refuses the same
int check_rank_call(sph_ctx* c, const char* what, const sph_params* p, const sph_sample_params* sp)
{
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: null parameters");
    if (int rc = slab_refuse(c, what)) return rc;
    return check_sample_params(c, sp);
}

int refuse_auto(sph_ctx* c, const char* what, const sph_sample_params* sp)
{
    for (int k = 0; k < sp->n_channels; k++)
        if (sp->channels[k].exponent == SPH_SAMPLE_AUTO_EXPONENT)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: channel %d has an automatic exponent (sph_slab_sample_range and sph_sample_fold_words come first: "
                                                     "every rank must scatter with the exponents of the whole vector)", what, k);
    return SPH_OK;
}

// clear c's words on its stream (the group call orders that before the range launches of the other members)
int clear_words(sph_ctx* c)
{
    HIPCHK(c, c->smp_red.ensure(sizeof(SampleRed)));
    HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0, sizeof(SampleRed), c->stream));
    HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0xff, sizeof(unsigned long long), c->stream));
    return SPH_OK;
}

// c's range pass over its owned slots, on c's stream, into `red` (its own words, or member 0's)
int launch_range(sph_ctx* c, const SampleIn& a, SampleRed* red)
{
    const uint32_t nt = slab_slots(c);
    if (nt) {
        ProfScope ps(&c->prof, "slab_sample_range", c->stream);
        hipLaunchKernelGGL(k_sample_range<true>, dim3((nt + 255) / 256), dim3(256), 0, c->stream, nt, a, red, slab_owned(c));
    }
    HIPCHK(c, hipGetLastError());
    return SPH_OK;
}

// the verdict of the folded words: the offender's sentence, or the exponents of the whole vector in sp_io
int fold_words(int n, const sph_slab_sample_words* words, sph_sample_params* sp_io, char* msg, size_t msg_bytes)
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

void exponents_of(const sph_sample_params* sp, int* expo)
{
    for (int k = 0; k < kMaxCh; k++) expo[k] = k < sp->n_channels ? sp->channels[k].exponent : 0;
}

// ---- a layer in two halves: up to the copy of the band words (queued), and from the band on (after the wait) ----
int layer_front(sph_ctx* c, const SampleGrid& g, uint32_t* hb)
{
    const uint32_t nt = slab_slots(c);
    hipStream_t s = c->stream;
    c->smp_have_layer = false;
    hb[0] = hb[1] = hb[2] = 0u;
    HIPCHK(c, c->smp_band.ensure(4 * sizeof(uint32_t)));
    if (nt == 0) return SPH_OK;
    HIPCHK(c, hipMemsetAsync(c->smp_band.p, 0, 4 * sizeof(uint32_t), s));
    HIPCHK(c, hipMemsetAsync(c->smp_band.p, 0xff, sizeof(uint32_t), s));
    {
        ProfScope ps(&c->prof, "slab_sample_band", s);
        hipLaunchKernelGGL(k_sample_band, dim3((nt + 255) / 256), dim3(256), 0, s, nt, c->pm[c->pcur].as<float4>(), slab_owned(c), g, c->smp_band.as<uint32_t>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hb, c->smp_band.p, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return SPH_OK;
}

// the scatter into the band (queued); its counts stay in c's words until read_stats
int layer_back(sph_ctx* c, const SampleIn& a, const SampleGrid& g, const uint32_t* hb, sph_sample_band* band)
{
    hipStream_t s = c->stream;
    band->sx0 = band->sx1 = 0;
    band->n_boxes = hb[2];
    band->reserved = 0;
    if (hb[2]) {
        // (what the device reduced are columns of boxes clamped to the grid; the clamp here guards the allocation all the same)
        band->sx0 = (int32_t)std::min(hb[0], (uint32_t)g.nx);
        band->sx1 = (int32_t)std::min(hb[1], (uint32_t)g.nx);
        if (band->sx0 >= band->sx1) band->sx0 = band->sx1 = 0;
    }
    const int bw = band->sx1 - band->sx0;
    if (bw > 0) {
        const uint32_t nt = slab_slots(c);
        const size_t n_words = (size_t)(a.nch + 1) * (size_t)g.ny * (size_t)bw;
        HIPCHK(c, c->smp_layer.ensure(n_words * sizeof(long long)));
        HIPCHK(c, c->smp_red.ensure(sizeof(SampleRed)));
        HIPCHK(c, hipMemsetAsync(c->smp_layer.p, 0, n_words * sizeof(long long), s));
        HIPCHK(c, hipMemsetAsync(c->smp_red.p, 0, sizeof(SampleRed), s));
        {
            ProfScope ps(&c->prof, "slab_sample_scatter", s);
            const uint32_t waves = (nt + 63) / 64;
            hipLaunchKernelGGL(kScatterSlab[a.nch], dim3((waves + 3) / 4), dim3(256), 0, s, nt, a, g, c->smp_layer.as<long long>(), c->smp_red.as<SampleRed>(),
                               slab_owned(c), band->sx0, bw);
        }
        HIPCHK(c, hipGetLastError());
    }
    c->smp_layer_sx0 = band->sx0;
    c->smp_layer_sx1 = band->sx1;
    c->smp_layer_ny = g.ny;
    c->smp_layer_planes = a.nch + 1;
    c->smp_have_layer = true;
    return SPH_OK;
}

// the counts of the layer c scattered last (waits for c's stream); an empty band scattered nothing
int read_stats(sph_ctx* c, sph_sample_info* one)
{
    one->n_touching = one->max_footprint = one->n_pairs = 0;
    if (c->smp_layer_sx1 <= c->smp_layer_sx0) return SPH_OK;
    std::vector<SampleRed> red(1);
    HIPCHK(c, hipMemcpyAsync(&red[0], c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fold_stats(red[0], one);
    return SPH_OK;
}

// ---- compose: layers that are on c's device and ordered before this point of c's stream -> the planes in values_out / raw_out ----
struct LayerRef {
    const long long* words;
    int sx0, sx1;
};

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
                           sp->n_channels + 1, l.words, l.sx0, l.sx1 - l.sx0);
    }
    launch_resolve(c, sp, expo, c->smp_planes.as<long long>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(values_out, c->smp_out.p, n_values * 4, hipMemcpyDeviceToHost, s));
    if (raw_out) HIPCHK(c, hipMemcpyAsync(raw_out, c->smp_planes.p, n_values * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

int check_band(sph_ctx* c, const sph_sample_params* sp, int k, const sph_sample_band& b)
{
    if (b.sx0 > b.sx1 || b.sx0 < 0 || b.sx1 > sp->nx)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: band %d = [%d, %d) is no column range of the %d sample columns", k, b.sx0, b.sx1, sp->nx);
    return SPH_OK;
}

// events of one group call, destroyed on every path out
struct Events {
    std::vector<hipEvent_t> e;
    hipError_t create(size_t n)
    {
        for (size_t i = 0; i < n; i++) {
            hipEvent_t v = nullptr;
            const hipError_t rc = hipEventCreateWithFlags(&v, hipEventDisableTiming);
            if (rc != hipSuccess) return rc;
            e.push_back(v);
        }
        return hipSuccess;
    }
    ~Events()
    {
        for (hipEvent_t v : e) (void)hipEventDestroy(v);
    }
};

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
    if (int rc = launch_range(c, a, c->smp_red.as<SampleRed>())) return rc;
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
    if (int rc = refuse_auto(c, "sph_slab_sample_layer", sp)) return rc;
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
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "sph_slab_sample_layer_download: not a slab context (sph_sample_grid samples a plain context)");
    if (!c->smp_have_layer) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_sample_layer_download: no layer (sph_slab_sample_layer comes first)");
    const uint64_t n_words = (uint64_t)c->smp_layer_planes * (uint64_t)c->smp_layer_ny * (uint64_t)(c->smp_layer_sx1 - c->smp_layer_sx0);
    if (n_words == 0) return SPH_OK;
    if (!words || capacity_words < n_words)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_sample_layer_download: capacity of %llu words, the layer holds %llu", (unsigned long long)capacity_words,
                       (unsigned long long)n_words);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(words, c->smp_layer.p, (size_t)n_words * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

extern "C" int sph_sample_compose(sph_ctx* c, const sph_sample_params* sp, int n_layers, const sph_sample_band* bands, const int64_t* const* layers,
                                  float* values_out, uint64_t values_bytes, int64_t* raw_out, uint64_t raw_bytes)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = check_sample_params(c, sp))) return rc;
    if ((rc = refuse_auto(c, "sph_sample_compose", sp))) return rc;
    if ((rc = check_sample_buffers(c, sp, values_out, values_bytes, raw_out, raw_bytes))) return rc;
    if (n_layers < 0 || (n_layers > 0 && !bands)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: %d layers without their bands", n_layers);
    const size_t per_column = (size_t)(sp->n_channels + 1) * (size_t)sp->ny;
    size_t total = 0;
    for (int k = 0; k < n_layers; k++) {
        if ((rc = check_band(c, sp, k, bands[k]))) return rc;
        const size_t n_words = per_column * (size_t)(bands[k].sx1 - bands[k].sx0);
        if (n_words && (!layers || !layers[k]))
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: layer %d is NULL, its band [%d, %d) is not empty", k, bands[k].sx0, bands[k].sx1);
        total += n_words;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // the layers side by side in one staging buffer: every copy has a place of its own, nothing waits for a merge
    HIPCHK(c, c->smp_stage.ensure((total ? total : 1) * sizeof(long long)));
    std::vector<LayerRef> L;
    size_t at = 0;
    for (int k = 0; k < n_layers; k++) {
        const size_t n_words = per_column * (size_t)(bands[k].sx1 - bands[k].sx0);
        if (!n_words) continue;
        long long* dst = c->smp_stage.as<long long>() + at;
        HIPCHK(c, hipMemcpyAsync(dst, layers[k], n_words * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        L.push_back(LayerRef{dst, bands[k].sx0, bands[k].sx1});
        at += n_words;
    }
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
    bool one_device = true;
    for (int i = 1; i < n; i++) one_device = one_device && ctxs[i]->device == c0->device;
    sph_sample_params sq = *sp;   // the exponents of the whole vector take the place of the automatic ones
    char msg[400];
    sph_sample_info sum{};

    if (!one_device) {   // the per-rank calls: the words and the layers pass through the host
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
        HIPCHK(c0, hipEventRecord(ev.e[(size_t)n], c0->stream));
        for (int i = 0; i < n; i++) {
            sph_ctx* c = ctxs[i];
            if (i) HIPCHK(c, hipStreamWaitEvent(c->stream, ev.e[(size_t)n], 0));
            if ((rc = launch_range(c, make_sample_in(c, p, sp), c0->smp_red.as<SampleRed>()))) return rc;
            if (i) HIPCHK(c, hipEventRecord(ev.e[(size_t)i], c->stream));
        }
        for (int i = 1; i < n; i++) HIPCHK(c0, hipStreamWaitEvent(c0->stream, ev.e[(size_t)i], 0));
        sph_slab_sample_words words;
        HIPCHK(c0, hipMemcpyAsync(&words, c0->smp_red.p, sizeof words, hipMemcpyDeviceToHost, c0->stream));
        HIPCHK(c0, hipStreamSynchronize(c0->stream));   // the one synchronisation before the scatter: the exponents, or the refusal
        if ((rc = fold_words(1, &words, &sq, msg, sizeof msg))) return c0->fail(rc, "%s", msg);
        int expo[kMaxCh];
        exponents_of(&sq, expo);
        const SampleGrid g = make_sample_grid(&sq, expo);
        std::vector<uint32_t> hb((size_t)n * 3, 0u);
        for (int i = 0; i < n; i++)
            if ((rc = layer_front(ctxs[i], g, &hb[(size_t)i * 3]))) return rc;
        std::vector<LayerRef> L;
        for (int i = 0; i < n; i++) {
            sph_ctx* c = ctxs[i];
            sph_sample_band band;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if ((rc = layer_back(c, make_sample_in(c, p, &sq), g, &hb[(size_t)i * 3], &band))) return rc;
            HIPCHK(c, hipEventRecord(ev.e[(size_t)i], c->stream));
            L.push_back(LayerRef{c->smp_layer.as<long long>(), band.sx0, band.sx1});
        }
        for (int i = 1; i < n; i++) HIPCHK(c0, hipStreamWaitEvent(c0->stream, ev.e[(size_t)i], 0));
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
    if (!ctxs || n < 1) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]) return SPH_ERR_INVALID_ARGUMENT;
    // whichever member refuses, the sentence is found in member 0's sph_last_error
    for (int i = 0; i < n; i++) ctxs[i]->err.clear();
    const int rc = group_sample_grid(ctxs, n, p, sp, values_out, values_bytes, raw_out, raw_bytes, info);
    for (int i = 1; rc != SPH_OK && ctxs[0]->err.empty() && i < n; i++) ctxs[0]->err = ctxs[i]->err;
    return rc;
}
