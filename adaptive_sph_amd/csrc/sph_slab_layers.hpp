// What the outputs drawn from slab contexts share -- frames (sph_slab_render.hip), fields on a grid (sph_slab_sample.hip) and the state
// ledger's group call (sph_ledger.hip).  A rank reduces the slots it owns to a band of sample columns, draws or scatters a layer over
// that band and keeps it (SlabLayer, sph_context.hpp); the layer is downloaded, or stays where a group shares one device; the ranks'
// layers are staged side by side on one context, merged and resolved.  Here: the owned slots, the band reduction, the band clamp, the
// kept layer's download, the staging of a compose, and the stream plumbing of a group on one device.  The scatter, merge and resolve
// kernels, the range passes and the argument checks differ per feature and stay in its file.
//
// Everything sits in an unnamed namespace: each translation unit compiles its own copy of the kernel it launches.
#pragma once

#include <algorithm>
#include <vector>

#include "sph_context.hpp"

namespace {

// slots in the arrays and their ownership flags: a plain context holds particles only; a slab context behind a step owned + ghosts,
// else the owned particles alone
inline uint32_t owned_slots(const sph_ctx* c) { return c->dist.on && c->have_flags ? c->dist.n_tot : (uint32_t)c->n; }
inline const uint8_t* owned_flags(const sph_ctx* c) { return c->dist.on && c->have_flags ? c->dist.owned.as<uint8_t>() : nullptr; }

// The sample columns the owned slots touch.  Box: trivially copyable, bool operator()(uint32_t slot, int& x0, int& x1) const -- false:
// the slot has no box on the grid, else its inclusive column range.  out: {min x0, max x1 + 1, live boxes}, set to {all ones, 0, 0}
// before the launch by the caller.  Block reduction in LDS, three atomics per block that holds a live box.
template <class Box>
__global__ __launch_bounds__(256) void k_layer_band(uint32_t nt, const uint8_t* __restrict__ owned, Box box, uint32_t* __restrict__ out)
{
    __shared__ uint32_t lo[256], hi[256], cnt[256];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t l = 0xffffffffu, h = 0u, c = 0u;
    if (i < nt && (!owned || owned[i])) {
        int x0, x1;
        if (box(i, x0, x1)) {
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

// the band words on the host -> [sx0, sx1) of `width` columns; an empty band is 0, 0.  (What the device reduced are columns of boxes
// clamped to the grid; the clamp here guards the allocation all the same.)
inline void band_of(const uint32_t* hb, int width, int32_t& sx0, int32_t& sx1)
{
    sx0 = sx1 = 0;
    if (!hb[2]) return;
    sx0 = (int32_t)std::min(hb[0], (uint32_t)width);
    sx1 = (int32_t)std::min(hb[1], (uint32_t)width);
    if (sx0 >= sx1) sx0 = sx1 = 0;
}

// <layer_call>_download: the layer kept by the last layer call -> dst.  plain_hint: what serves a plain context instead.
inline int layer_download(sph_ctx* c, const SlabLayer& l, const char* layer_call, const char* plain_hint, void* dst, uint64_t capacity_words)
{
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s_download: not a slab context (%s)", layer_call, plain_hint);
    if (!l.have) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s_download: no layer (%s comes first)", layer_call, layer_call);
    const uint64_t n_words = (uint64_t)l.planes * (uint64_t)l.rows * (uint64_t)(l.sx1 - l.sx0);
    if (n_words == 0) return SPH_OK;
    if (!dst || capacity_words < n_words)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s_download: capacity of %llu words, the layer holds %llu", layer_call, (unsigned long long)capacity_words,
                       (unsigned long long)n_words);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, l.words.p, (size_t)n_words * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

// a layer on the composing context's device, ordered before the merge on its stream
struct LayerRef {
    const void* words;
    int sx0, sx1;
    template <class T>
    const T* as() const { return (const T*)words; }
};

// The layers of a compose call side by side in c's staging buffer -> L (the empty ones left out): every copy has a place of its own,
// nothing waits for a merge.  Band: sph_render_band or sph_sample_band; width: the grid's columns; prefix: "render" or "sample".
template <class W, class Band>
int stage_layers(sph_ctx* c, SlabLayer& l, int n_layers, const Band* bands, int width, size_t words_per_column, const W* const* layers, const char* prefix,
                 std::vector<LayerRef>& L)
{
    static_assert(sizeof(W) == 8, "a layer word is 64 bits");
    size_t total = 0;
    for (int k = 0; k < n_layers; k++) {
        const Band& b = bands[k];
        if (b.sx0 > b.sx1 || b.sx0 < 0 || b.sx1 > width)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: band %d = [%d, %d) is no column range of the %d sample columns", prefix, k, b.sx0, b.sx1, width);
        const size_t n_words = words_per_column * (size_t)(b.sx1 - b.sx0);
        if (n_words && (!layers || !layers[k])) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: layer %d is NULL, its band [%d, %d) is not empty", prefix, k, b.sx0, b.sx1);
        total += n_words;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, l.stage.ensure((total ? total : 1) * sizeof(W)));
    size_t at = 0;
    for (int k = 0; k < n_layers; k++) {
        const size_t n_words = words_per_column * (size_t)(bands[k].sx1 - bands[k].sx0);
        if (!n_words) continue;
        W* dst = l.stage.as<W>() + at;
        HIPCHK(c, hipMemcpyAsync(dst, layers[k], n_words * sizeof(W), hipMemcpyHostToDevice, c->stream));
        L.push_back(LayerRef{dst, bands[k].sx0, bands[k].sx1});
        at += n_words;
    }
    return SPH_OK;
}

// ---- a group on one device: the members' streams fan out and back in to member 0 through events ----
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

inline bool same_device(sph_ctx* const* ctxs, int n)
{
    for (int i = 1; i < n; i++)
        if (ctxs[i]->device != ctxs[0]->device) return false;
    return true;
}

// Every member adds to words of member 0's that member 0's stream has just cleared: the members wait for that point (ev.e[n]), run
// body(i) on their streams and record ev.e[i]; member 0 waits for all of them.  ev holds n + 1 events.
template <class Body>
int fan_in_to_first(Events& ev, sph_ctx* const* ctxs, int n, Body body)
{
    sph_ctx* c0 = ctxs[0];
    HIPCHK(c0, hipEventRecord(ev.e[(size_t)n], c0->stream));
    for (int i = 0; i < n; i++) {
        sph_ctx* c = ctxs[i];
        if (i) HIPCHK(c, hipStreamWaitEvent(c->stream, ev.e[(size_t)n], 0));
        if (int rc = body(i)) return rc;
        HIPCHK(c, hipEventRecord(ev.e[(size_t)i], c->stream));
    }
    for (int i = 1; i < n; i++) HIPCHK(c0, hipStreamWaitEvent(c0->stream, ev.e[(size_t)i], 0));
    return SPH_OK;
}

// The members' layers: front(i) queues member i's work up to the copy of its band words, for every member before any is waited for;
// then per member the wait, back(i) (from the band on) and ev.e[i]; member 0's stream waits for every member's layer.
template <class Front, class Back>
int group_layers(Events& ev, sph_ctx* const* ctxs, int n, Front front, Back back)
{
    for (int i = 0; i < n; i++)
        if (int rc = front(i)) return rc;
    for (int i = 0; i < n; i++) {
        sph_ctx* c = ctxs[i];
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (int rc = back(i)) return rc;
        HIPCHK(c, hipEventRecord(ev.e[(size_t)i], c->stream));
    }
    for (int i = 1; i < n; i++) HIPCHK(ctxs[0], hipStreamWaitEvent(ctxs[0]->stream, ev.e[(size_t)i], 0));
    return SPH_OK;
}

// a group entry point: whichever member refuses in body(), the sentence is found in member 0's sph_last_error
template <class Body>
int group_call(sph_ctx** ctxs, int n, Body body)
{
    if (!ctxs || n < 1) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++) ctxs[i]->err.clear();
    const int rc = body();
    for (int i = 1; rc != SPH_OK && ctxs[0]->err.empty() && i < n; i++) ctxs[0]->err = ctxs[i]->err;
    return rc;
}

}  // namespace
