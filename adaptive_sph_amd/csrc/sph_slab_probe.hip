// include/sph_slab_probe.h: the probe sets of sph_probe.h on slab contexts.  Every rank scatters the particles it OWNS onto its replica
// of the point set and packs the touched points into a compact layer (ascending point indices, then int64 words); the planes are the
// per-point sums of the ranks' layers, bit for bit the planes of one vector holding the same particles (integer addition is
// associative, every particle has one owner); then sph_probe_sample's resolve, or sph_probe_advect's move on every replica.  The set,
// the scatter, the move and the checks are sph_probe.hip's (sph_probe_internal.hpp), the range pass, the fold and the resolve are the
// lattice form's (sph_sample_internal.hpp): one definition of the arithmetic for all of them.
//
// Kernels (each on the stream of the context it works for; they read the state and write only probe buffers):
//   k_sample_range<true>        the owned slots' preconditions and max |a| per channel (sph_slab_sample.hip launches the same)
//   k_probe_scatter<C, true>    sph_probe.hip's scatter; a ghost lane has no rows.  Into the rank's own planes (layer call) or, in a group
//                               on one device, with the same 64-bit atomics straight into member 0's planes
//   k_probe_pack                behind device_exclusive_scan_u32 over the touched flags (0 / 1 words): point k with touched[k] writes
//                               entry pos[k] -- its index and its C + 1 words.  The planes are in the caller's point order already (the
//                               scatter writes through sidx), so the layer is in the caller's numbering
//   k_probe_compose             one launch per layer, in stream order: one thread per (plane, entry), plain 64-bit load, add, store at
//                               planes[plane * n_points + index[e]] -- the indices of one layer are distinct (validated on the host
//                               before the first launch), the planes were cleared by a memset; plane 0's thread flags the point
//   k_probe_touched, k_sample_resolve, k_probe_move   as sph_probe.hip launches them
// The entry count must reach the host before the layer can be allocated for it: one wait per layer call, for the 4-byte count and the
// scatter's counts together; the pack is queued behind it on the same stream, which every reader of the layer uses.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sph_slab_probe.h"
#include "sph_probe_internal.hpp"
#include "sph_slab_layers.hpp"

static_assert(offsetof(SampleRed, max_bits) == offsetof(sph_slab_sample_words, max_bits), "the verdict is the head of the range pass's words");

namespace {

// point k < n with touched[k] -> entry pos[k] < n_entries: its index, its `planes` words
__global__ __launch_bounds__(256) void k_probe_pack(uint32_t n, int planes, const uint32_t* __restrict__ touched, const uint32_t* __restrict__ pos,
                                                    const long long* __restrict__ src, uint32_t n_entries, uint32_t* __restrict__ idx,
                                                    long long* __restrict__ words)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n || !touched[k]) return;
    const uint32_t e = pos[k];
    if (e >= n_entries) return;   // (the scan's total is n_entries: never taken)
    idx[e] = k;
    for (int pl = 0; pl < planes; pl++) words[(size_t)pl * n_entries + e] = src[(size_t)pl * n + k];
}

// one thread per word of the layer (planes x n_entries)
__global__ __launch_bounds__(256) void k_probe_compose(long long* __restrict__ dst, uint32_t n_points, int planes, const uint32_t* __restrict__ idx,
                                                       const long long* __restrict__ words, uint32_t n_entries, uint32_t* __restrict__ touched)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)planes * n_entries) return;
    const uint32_t pl = (uint32_t)(t / n_entries), e = (uint32_t)(t - (size_t)pl * n_entries);
    const uint32_t k = idx[e];
    if (k >= n_points) return;    // (validated on the host: never taken)
    const size_t at = (size_t)pl * n_points + k;
    dst[at] = dst[at] + words[t];
    if (pl == 0) touched[k] = 1u;
}

// what serves a plain context instead, and what gives a layer call its exponents
const char* const kPlainHint = "sph_probe_sample samples a plain context";
const char* const kFoldFirst = "the fold comes first: sph_slab_probe_range and sph_probe_fold_words";

// the n x 1 grid of a sph_probe_params (n: the set's points, 0 where no set takes part)
sph_sample_params sample_params_of(const sph_probe_set* set, const sph_probe_params* pp)
{
    sph_probe_set none;
    return as_sample_params(set ? set : &none, pp->volume, pp->flags, pp->min_weight, pp->fill, pp->n_channels, pp->channels);
}

// the n x 1 grid of a tracer step: the two velocity channels, as sph_probe_advect builds them
sph_sample_params sample_params_of(const sph_probe_set* set, const sph_probe_advect_params* ap)
{
    const sph_sample_channel ch[2] = {{SPH_F_VELOCITY, 0, ap->exponent_x}, {SPH_F_VELOCITY, 1, ap->exponent_y}};
    return as_sample_params(set, ap->volume, 0u, ap->min_weight, 0.f, 2, ch);
}

// sph_probe_advect's refusals of its own arguments, with its texts
int check_advect_params(sph_ctx* c, const sph_probe_advect_params* ap)
{
    if (!ap) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null advect parameters");
    if (!(std::fabs(ap->dt) < INFINITY)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: advect: dt must be finite");
    if (!(ap->min_weight > 0.f) || !(ap->min_weight < INFINITY))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: advect: min_weight must be finite and > 0 (a point divides by its weight)");
    return SPH_OK;
}

// sph_probe_sample's refusals of its output buffers, with its texts
int check_probe_buffers(sph_ctx* c, uint64_t n_values, const float* values_out, uint64_t values_bytes, const int64_t* raw_out, uint64_t raw_bytes)
{
    if (n_values && (!values_out || values_bytes < n_values * 4))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: output buffer of %llu bytes, %llu needed", (unsigned long long)values_bytes,
                       (unsigned long long)(n_values * 4));
    if (n_values && raw_out && raw_bytes < n_values * 8)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: raw output buffer of %llu bytes, %llu needed", (unsigned long long)raw_bytes,
                       (unsigned long long)(n_values * 8));
    return SPH_OK;
}

// c's owned slots scattered onto ps's binned points (ps: a set of c, binned) into `planes` / `touched` / `red` -- c's own, or member
// 0's on the same device -- on c's stream
int launch_slab_scatter(sph_ctx* c, const sph_params* p, sph_probe_set* ps, const sph_sample_params* sp, const int* expo, long long* planes, uint32_t* touched,
                        SampleRed* red)
{
    const uint32_t nt = owned_slots(c);
    if (!nt || !ps->n) return SPH_OK;
    const int C = sp->n_channels;
    ProbeScale sc{};
    for (int k = 0; k < C; k++) sc.scale[k] = std::ldexp(1.f, 32 - expo[k]);
    {
        ProfScope prof(&c->prof, "slab_probe_scatter", c->stream);
        hipLaunchKernelGGL(probe_scatter_fn<true>(C), dim3((nt + 63) / 64), dim3(64), 0, c->stream, nt, make_sample_in(c, p, sp), bins_of(ps), sc,
                           ps->cell_start.as<uint32_t>(), ps->sxy.as<float2>(), ps->sidx.as<uint32_t>(), (size_t)ps->n, planes, touched, red, owned_flags(c));
    }
    HIPCHK(c, hipGetLastError());
    return SPH_OK;
}

void launch_touched(sph_ctx* c, sph_probe_set* ps)
{
    const uint32_t np = (uint32_t)ps->n;
    if (np) hipLaunchKernelGGL(k_probe_touched, dim3((np + 255) / 256), dim3(256), 0, c->stream, np, ps->touched.as<uint32_t>(), c->prb_stat.as<ProbeStat>());
}

// the tracer step of ps's points from `planes` (weight, x, y sums of ps->n points each) on c's stream, its counts and box into c's words
void launch_move(sph_ctx* c, sph_probe_set* ps, const sph_probe_advect_params* ap, const int* expo, const long long* planes)
{
    const uint32_t np = (uint32_t)ps->n;
    if (!np) return;
    ProfScope prof(&c->prof, "probe_move", c->stream);
    hipLaunchKernelGGL(k_probe_move, dim3(std::min((np + 255) / 256, kMoveBlocks)), dim3(256), 0, c->stream, np, planes, ps->xy.as<float2>(), ap->dt,
                       ap->min_weight, std::ldexp(1.0, expo[0] - 32), std::ldexp(1.0, expo[1] - 32), c->prb_stat.as<ProbeStat>());
}

// the counts of c's last call (waits for c's stream)
int read_words(sph_ctx* c, SampleRed* red, ProbeStat* st)
{
    HIPCHK(c, hipMemcpyAsync(red, c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, c->prb_stat.p, sizeof(ProbeStat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

// behind a move: the box of the points as they are now came with the counts; the bins follow at the next use
void moved(sph_probe_set* ps, const ProbeStat& st)
{
    if (!ps->n) return;
    for (int k = 0; k < 4; k++) ps->bb[k] = float_of(st.bb[k]);
    ps->binned = false;
}

// ---- compose: the layers validated on the host, staged side by side in the set's buffers, added into c->smp_planes (queued) ----
int stage_and_sum(sph_ctx* c, sph_probe_set* ps, int planes, int n_layers, const uint64_t* n_entries, const uint32_t* const* indices,
                  const int64_t* const* words)
{
    const uint64_t np = ps->n;
    if (n_layers < 0 || (n_layers > 0 && !n_entries)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: %d layers without their entry counts", n_layers);
    size_t total = 0;
    for (int k = 0; k < n_layers; k++) {
        const uint64_t ne = n_entries[k];
        if (!ne) continue;
        if (!indices || !indices[k] || !words || !words[k])
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: layer %d is NULL, it has %llu entries", k, (unsigned long long)ne);
        const uint32_t* ix = indices[k];
        for (uint64_t e = 0; e < ne; e++) {
            if (ix[e] >= np)
                return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: layer %d: entry %llu is point %u, the set holds %llu points", k, (unsigned long long)e, ix[e],
                               (unsigned long long)np);
            if (e && ix[e] <= ix[e - 1])
                return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: layer %d: the indices are not strictly ascending (entry %llu is point %u behind point %u)", k,
                               (unsigned long long)e, ix[e], ix[e - 1]);
        }
        total += (size_t)ne;   // (ne <= np <= 2^24 per layer)
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = clear_probe_stat(c)) return rc;
    if (!np) return SPH_OK;
    hipStream_t s = c->stream;
    if (int rc = clear_probe_planes(c, ps, planes)) return rc;
    HIPCHK(c, ps->stage_idx.ensure((total ? total : 1) * 4));
    HIPCHK(c, ps->stage_words.ensure((total ? total : 1) * (size_t)planes * 8));
    size_t at = 0;
    for (int k = 0; k < n_layers; k++) {
        const size_t ne = (size_t)n_entries[k];
        if (!ne) continue;
        uint32_t* d_idx = ps->stage_idx.as<uint32_t>() + at;
        long long* d_words = ps->stage_words.as<long long>() + at * (size_t)planes;
        HIPCHK(c, hipMemcpyAsync(d_idx, indices[k], ne * 4, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_words, words[k], ne * (size_t)planes * 8, hipMemcpyHostToDevice, s));
        {
            ProfScope prof(&c->prof, "slab_probe_compose", s);
            hipLaunchKernelGGL(k_probe_compose, dim3((uint32_t)((ne * (size_t)planes + 255) / 256)), dim3(256), 0, s, c->smp_planes.as<long long>(), (uint32_t)np,
                               planes, d_idx, d_words, (uint32_t)ne, ps->touched.as<uint32_t>());
        }
        at += ne;
    }
    launch_touched(c, ps);
    HIPCHK(c, hipGetLastError());
    return SPH_OK;
}

// member 0's planes resolved and copied out (queued on c0's stream)
int resolve_out(sph_ctx* c, const sph_sample_params* sp, const int* expo, uint64_t n_values, float* values_out, int64_t* raw_out)
{
    if (!n_values) return SPH_OK;
    launch_resolve(c, sp, expo, c->smp_planes.as<long long>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(values_out, c->smp_out.p, (size_t)n_values * 4, hipMemcpyDeviceToHost, c->stream));
    if (raw_out) HIPCHK(c, hipMemcpyAsync(raw_out, c->smp_planes.p, (size_t)n_values * 8, hipMemcpyDeviceToHost, c->stream));
    return SPH_OK;
}

// ---- a layer: scatter, scan, the entry count to the host, pack ----
int make_layer(sph_ctx* c, const sph_params* p, sph_probe_set* ps, const sph_sample_params* sp, const int* expo, sph_slab_probe_layer_info* out)
{
    hipStream_t s = c->stream;
    const int planes = sp->n_channels + 1;
    const uint32_t np = (uint32_t)ps->n;
    ps->lay_have = false;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = clear_words(c)) return rc;
    uint32_t ne = 0;
    uint32_t* d_total = nullptr;
    if (np) {
        if (int rc = ensure_binned(c, ps)) return rc;
        if (int rc = clear_probe_planes(c, ps, planes)) return rc;
        if (int rc = launch_slab_scatter(c, p, ps, sp, expo, c->smp_planes.as<long long>(), ps->touched.as<uint32_t>(), c->smp_red.as<SampleRed>())) return rc;
        HIPCHK(c, ps->lay_pos.ensure((size_t)np * 4));
        HIPCHK(c, ps->lay_total.ensure(((size_t)np / 2048 + 4) * 4 + 4));   // the scan's word per tile of 2048, then its total
        d_total = ps->lay_total.as<uint32_t>() + ((size_t)np / 2048 + 4);
        {
            ProfScope prof(&c->prof, "slab_probe_pack", s);
            device_exclusive_scan_u32(s, ps->touched.as<uint32_t>(), ps->lay_pos.as<uint32_t>(), np, ps->lay_total.as<uint32_t>(), d_total);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&ne, d_total, 4, hipMemcpyDeviceToHost, s));
    }
    // the one wait of a layer call: the entry count, and with it the scatter's counts.  The pack is queued behind it; the download,
    // the next call and the set's destroy all run on this stream
    SampleRed red;
    HIPCHK(c, hipMemcpyAsync(&red, c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (ne > np) return c->fail(SPH_ERR_DEVICE, "sph_slab_probe_layer: %u entries of %u points", ne, np);
    if (ne) {
        HIPCHK(c, ps->lay_idx.ensure((size_t)ne * 4));
        HIPCHK(c, ps->lay_words.ensure((size_t)ne * (size_t)planes * 8));
        ProfScope prof(&c->prof, "slab_probe_pack", s);
        hipLaunchKernelGGL(k_probe_pack, dim3((np + 255) / 256), dim3(256), 0, s, np, planes, ps->touched.as<uint32_t>(), ps->lay_pos.as<uint32_t>(),
                           c->smp_planes.as<long long>(), ne, ps->lay_idx.as<uint32_t>(), ps->lay_words.as<long long>());
        HIPCHK(c, hipGetLastError());
    }
    ps->lay_entries = ne;
    ps->lay_planes = planes;
    ps->lay_have = true;
    if (out) {
        *out = sph_slab_probe_layer_info{};
        for (int k = 0; k < kMaxCh; k++) out->exponents[k] = expo[k];
        out->n_entries = ne;
        for (const SampleStat& st : red.stat) {
            out->n_touching += st.n_touching;
            out->n_pairs += st.n_pairs;
        }
    }
    return SPH_OK;
}

int layer_to_host(sph_ctx* c, sph_probe_set* ps, uint32_t* indices_out, int64_t* words_out, uint64_t capacity_entries)
{
    if (!ps->lay_have) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_probe_layer_download: no layer (sph_slab_probe_layer comes first)");
    const uint64_t ne = ps->lay_entries;
    if (!ne) return SPH_OK;
    if (!indices_out || !words_out || capacity_entries < ne)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_probe_layer_download: capacity of %llu entries, the layer holds %llu", (unsigned long long)capacity_entries,
                       (unsigned long long)ne);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(indices_out, ps->lay_idx.p, (size_t)ne * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(words_out, ps->lay_words.p, (size_t)ne * (size_t)ps->lay_planes * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

}  // namespace

extern "C" int sph_slab_probe_range(sph_ctx* c, const sph_params* p, const sph_probe_params* pp, sph_slab_sample_words* out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_probe_range: null output");
    out->first_bad = ~0ull;
    for (int k = 0; k < kMaxCh; k++) out->max_bits[k] = 0u;
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null parameters");
    if (int rc = slab_refuse(c, "sph_slab_probe_range", kPlainHint)) return rc;
    if (!pp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null probe parameters");
    const sph_sample_params sp = sample_params_of(nullptr, pp);
    if (int rc = check_channels(c, &sp)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = clear_words(c)) return rc;
    if (int rc = launch_range(c, make_sample_in(c, p, &sp), c->smp_red.as<SampleRed>(), owned_slots(c), owned_flags(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->smp_red.p, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

extern "C" int sph_probe_fold_words(int n, const sph_slab_sample_words* words, sph_probe_params* pp_io, char* msg, uint64_t msg_bytes)
{
    if (msg && msg_bytes) msg[0] = 0;
    if (n < 1 || !words || !pp_io) {
        if (msg && msg_bytes) snprintf(msg, (size_t)msg_bytes, "sph_probe_fold_words: n < 1, null words or null probe parameters");
        return SPH_ERR_INVALID_ARGUMENT;
    }
    sph_sample_params sp = sample_params_of(nullptr, pp_io);
    const int rc = fold_words(n, words, &sp, msg, (size_t)msg_bytes);
    if (rc == SPH_OK)
        for (int k = 0; k < sp.n_channels && k < kMaxCh; k++) pp_io->channels[k].exponent = sp.channels[k].exponent;
    return rc;
}

extern "C" int sph_slab_probe_layer(sph_ctx* c, const sph_params* p, sph_probe_set* set, const sph_probe_params* pp, sph_slab_probe_layer_info* out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (out) *out = sph_slab_probe_layer_info{};
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null parameters");
    if (int rc = slab_refuse(c, "sph_slab_probe_layer", kPlainHint)) return rc;
    if (int rc = check_set(c, set)) return rc;
    if (!pp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null probe parameters");
    const sph_sample_params sp = sample_params_of(set, pp);
    if (int rc = check_channels(c, &sp)) return rc;
    if (int rc = refuse_auto(c, "sph_slab_probe_layer", &sp, kFoldFirst)) return rc;
    int expo[kMaxCh];
    exponents_of(&sp, expo);
    return make_layer(c, p, set, &sp, expo, out);
}

extern "C" int sph_slab_probe_layer_download(sph_ctx* c, sph_probe_set* set, uint32_t* indices_out, int64_t* words_out, uint64_t capacity_entries)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "sph_slab_probe_layer_download: not a slab context (sph_probe_sample samples a plain context)");
    if (int rc = check_set(c, set)) return rc;
    return layer_to_host(c, set, indices_out, words_out, capacity_entries);
}

extern "C" int sph_probe_compose(sph_ctx* c, sph_probe_set* set, const sph_probe_params* pp, int n_layers, const uint64_t* n_entries,
                                 const uint32_t* const* indices, const int64_t* const* words, float* values_out, uint64_t values_bytes, int64_t* raw_out,
                                 uint64_t raw_bytes, sph_probe_info* info)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_set(c, set)) return rc;
    if (!pp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null probe parameters");
    const sph_sample_params sp = sample_params_of(set, pp);
    if (int rc = check_channels(c, &sp)) return rc;
    if (int rc = refuse_auto(c, "sph_probe_compose", &sp, kFoldFirst)) return rc;
    const uint64_t n_values = (uint64_t)(sp.n_channels + 1) * set->n;
    if (int rc = check_probe_buffers(c, n_values, values_out, values_bytes, raw_out, raw_bytes)) return rc;
    int expo[kMaxCh];
    exponents_of(&sp, expo);
    if (int rc = stage_and_sum(c, set, sp.n_channels + 1, n_layers, n_entries, indices, words)) return rc;
    if (int rc = resolve_out(c, &sp, expo, n_values, values_out, raw_out)) return rc;
    ProbeStat st;
    HIPCHK(c, hipMemcpyAsync(&st, c->prb_stat.p, sizeof(ProbeStat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (info) fill_info(info, set, expo, SampleRed{}, st);   // (no particle was read: n_touching and n_pairs stay 0)
    return SPH_OK;
}

extern "C" int sph_probe_compose_advect(sph_ctx* c, sph_probe_set* set, const sph_probe_advect_params* ap, int n_layers, const uint64_t* n_entries,
                                        const uint32_t* const* indices, const int64_t* const* words, sph_probe_info* info)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_set(c, set)) return rc;
    if (int rc = check_advect_params(c, ap)) return rc;
    const sph_sample_params sp = sample_params_of(set, ap);
    if (int rc = check_channels(c, &sp)) return rc;
    if (int rc = refuse_auto(c, "sph_probe_compose_advect", &sp, kFoldFirst)) return rc;
    int expo[kMaxCh];
    exponents_of(&sp, expo);
    if (int rc = stage_and_sum(c, set, 3, n_layers, n_entries, indices, words)) return rc;
    launch_move(c, set, ap, expo, c->smp_planes.as<long long>());
    HIPCHK(c, hipGetLastError());
    ProbeStat st;
    HIPCHK(c, hipMemcpyAsync(&st, c->prb_stat.p, sizeof(ProbeStat), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (info) fill_info(info, set, expo, SampleRed{}, st);
    moved(set, st);
    return SPH_OK;
}

namespace {

// what both group calls refuse of their members and sets before anything is launched
int check_group(sph_ctx** ctxs, int n, const char* what, const sph_params* p, sph_probe_set* const* sets)
{
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on) return ctxs[i]->fail(SPH_ERR_UNSUPPORTED, "%s: context %d is no slab context (sph_probe_sample samples a plain context)", what, i);
    if (!p) return ctxs[0]->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null parameters");
    if (!sets) return ctxs[0]->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null probe sets");
    for (int i = 0; i < n; i++) {
        if (int rc = slab_refuse(ctxs[i], what, kPlainHint)) return rc;
        if (int rc = check_set(ctxs[i], sets[i])) return rc;
        if (sets[i]->n != sets[0]->n)
            return ctxs[i]->fail(SPH_ERR_INVALID_ARGUMENT, "%s: the sets of a group hold the same points: set %d holds %llu points, set 0 holds %llu", what, i,
                                 (unsigned long long)sets[i]->n, (unsigned long long)sets[0]->n);
    }
    return SPH_OK;
}

// The accumulation of a group.  One device: the members' range passes into member 0's words, the exponents or the refusal, every
// member's scatter into member 0's planes, touched flags and counts; member 0's stream has waited for all of them, nothing is waited
// for on the host.  Else the per-rank calls: ranges, fold, layers, downloads -> lay (the caller composes).  sq: the exponents used.
struct HostLayers {
    std::vector<uint64_t> ne;
    std::vector<std::vector<uint32_t>> idx;
    std::vector<std::vector<int64_t>> words;
    std::vector<const uint32_t*> pi;
    std::vector<const int64_t*> pw;
    uint64_t n_touching = 0, n_pairs = 0;
};

int group_accumulate(Events& ev, sph_ctx** ctxs, int n, const sph_params* p, sph_probe_set* const* sets, sph_sample_params* sq, bool one_device, HostLayers* lay)
{
    sph_ctx* c0 = ctxs[0];
    char msg[400];
    int rc;
    int expo[kMaxCh];
    const int C = sq->n_channels;
    if (!one_device) {
        std::vector<sph_slab_sample_words> words((size_t)n);
        sph_probe_params pp{};
        pp.volume = sq->volume;
        pp.n_channels = C;
        for (int k = 0; k < C; k++) pp.channels[k] = sq->channels[k];
        for (int i = 0; i < n; i++)
            if ((rc = sph_slab_probe_range(ctxs[i], p, &pp, &words[(size_t)i]))) return rc;
        if ((rc = fold_words(n, words.data(), sq, msg, sizeof msg))) return c0->fail(rc, "%s", msg);
        exponents_of(sq, expo);
        lay->ne.assign((size_t)n, 0);
        lay->idx.resize((size_t)n);
        lay->words.resize((size_t)n);
        lay->pi.assign((size_t)n, nullptr);
        lay->pw.assign((size_t)n, nullptr);
        for (int i = 0; i < n; i++) {
            sph_slab_probe_layer_info one{};
            if ((rc = make_layer(ctxs[i], p, sets[i], sq, expo, &one))) return rc;
            lay->n_touching += one.n_touching;
            lay->n_pairs += one.n_pairs;
            lay->ne[(size_t)i] = one.n_entries;
            if (!one.n_entries) continue;
            lay->idx[(size_t)i].resize((size_t)one.n_entries);
            lay->words[(size_t)i].resize((size_t)one.n_entries * (size_t)(C + 1));
            if ((rc = layer_to_host(ctxs[i], sets[i], lay->idx[(size_t)i].data(), lay->words[(size_t)i].data(), one.n_entries))) return rc;
            lay->pi[(size_t)i] = lay->idx[(size_t)i].data();
            lay->pw[(size_t)i] = lay->words[(size_t)i].data();
        }
        return SPH_OK;
    }
    HIPCHK(c0, hipSetDevice(c0->device));
    if ((rc = clear_words(c0))) return rc;
    rc = fan_in_to_first(ev, ctxs, n, [&](int i) {
        return launch_range(ctxs[i], make_sample_in(ctxs[i], p, sq), c0->smp_red.as<SampleRed>(), owned_slots(ctxs[i]), owned_flags(ctxs[i]));
    });
    if (rc) return rc;
    sph_slab_sample_words words;
    HIPCHK(c0, hipMemcpyAsync(&words, c0->smp_red.p, sizeof words, hipMemcpyDeviceToHost, c0->stream));
    HIPCHK(c0, hipStreamSynchronize(c0->stream));   // the one synchronisation before the scatter: the exponents, or the refusal
    if ((rc = fold_words(1, &words, sq, msg, sizeof msg))) return c0->fail(rc, "%s", msg);
    exponents_of(sq, expo);
    if ((rc = clear_probe_stat(c0))) return rc;
    if (!sets[0]->n) return SPH_OK;
    if ((rc = clear_probe_planes(c0, sets[0], C + 1))) return rc;
    rc = fan_in_to_first(ev, ctxs, n, [&](int i) {
        if (int rb = ensure_binned(ctxs[i], sets[i])) return rb;
        return launch_slab_scatter(ctxs[i], p, sets[i], sq, expo, c0->smp_planes.as<long long>(), sets[0]->touched.as<uint32_t>(), c0->smp_red.as<SampleRed>());
    });
    if (rc) return rc;
    launch_touched(c0, sets[0]);
    HIPCHK(c0, hipGetLastError());
    return SPH_OK;
}

int group_probe_sample(sph_ctx** ctxs, int n, const sph_params* p, sph_probe_set* const* sets, const sph_probe_params* pp, float* values_out, uint64_t values_bytes,
                       int64_t* raw_out, uint64_t raw_bytes, sph_probe_info* info)
{
    sph_ctx* c0 = ctxs[0];
    int rc;
    if ((rc = check_group(ctxs, n, "sph_group_probe_sample", p, sets))) return rc;
    if (!pp) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null probe parameters");
    sph_sample_params sq = sample_params_of(sets[0], pp);   // the exponents of the whole vector take the place of the automatic ones
    if ((rc = check_channels(c0, &sq))) return rc;
    const uint64_t n_values = (uint64_t)(sq.n_channels + 1) * sets[0]->n;
    if ((rc = check_probe_buffers(c0, n_values, values_out, values_bytes, raw_out, raw_bytes))) return rc;
    const bool one_device = same_device(ctxs, n);
    Events ev;
    HIPCHK(c0, hipSetDevice(c0->device));
    HIPCHK(c0, ev.create((size_t)n + 1));
    HostLayers lay;
    if ((rc = group_accumulate(ev, ctxs, n, p, sets, &sq, one_device, &lay))) return rc;
    int expo[kMaxCh];
    exponents_of(&sq, expo);
    if (!one_device) {
        sph_probe_params pq = *pp;
        for (int k = 0; k < sq.n_channels; k++) pq.channels[k].exponent = expo[k];
        if ((rc = sph_probe_compose(c0, sets[0], &pq, n, lay.ne.data(), lay.pi.data(), lay.pw.data(), values_out, values_bytes, raw_out, raw_bytes, info))) return rc;
        if (info) {
            info->n_touching = lay.n_touching;
            info->n_pairs = lay.n_pairs;
        }
        return SPH_OK;
    }
    if ((rc = resolve_out(c0, &sq, expo, n_values, values_out, raw_out))) return rc;
    SampleRed red;
    ProbeStat st;
    if ((rc = read_words(c0, &red, &st))) return rc;
    if (info) fill_info(info, sets[0], expo, red, st);
    return SPH_OK;
}

int group_probe_advect(sph_ctx** ctxs, int n, const sph_params* p, sph_probe_set* const* sets, const sph_probe_advect_params* ap, sph_probe_info* info)
{
    sph_ctx* c0 = ctxs[0];
    int rc;
    if ((rc = check_group(ctxs, n, "sph_group_probe_advect", p, sets))) return rc;
    if ((rc = check_advect_params(c0, ap))) return rc;
    sph_sample_params sq = sample_params_of(sets[0], ap);
    if ((rc = check_channels(c0, &sq))) return rc;
    const bool one_device = same_device(ctxs, n);
    Events ev;
    HIPCHK(c0, hipSetDevice(c0->device));
    HIPCHK(c0, ev.create((size_t)n + 2));
    HostLayers lay;
    if ((rc = group_accumulate(ev, ctxs, n, p, sets, &sq, one_device, &lay))) return rc;
    int expo[kMaxCh];
    exponents_of(&sq, expo);
    if (!one_device) {
        sph_probe_advect_params aq = *ap;
        aq.exponent_x = expo[0];
        aq.exponent_y = expo[1];
        for (int i = n - 1; i >= 0; i--)   // (member 0 last: its info is the call's)
            if ((rc = sph_probe_compose_advect(ctxs[i], sets[i], &aq, n, lay.ne.data(), lay.pi.data(), lay.pw.data(), info))) return rc;
        if (info) {
            info->n_touching = lay.n_touching;
            info->n_pairs = lay.n_pairs;
        }
        return SPH_OK;
    }
    // every member moves its own replica from member 0's planes: member 0's stream has waited for every scatter, the others wait for it
    const long long* planes = c0->smp_planes.as<long long>();
    HIPCHK(c0, hipEventRecord(ev.e[(size_t)n + 1], c0->stream));
    for (int i = 1; i < n; i++) {
        sph_ctx* c = ctxs[i];
        HIPCHK(c, hipStreamWaitEvent(c->stream, ev.e[(size_t)n + 1], 0));
        if ((rc = clear_probe_stat(c))) return rc;
    }
    for (int i = 0; i < n; i++) {
        launch_move(ctxs[i], sets[i], ap, expo, planes);
        HIPCHK(ctxs[i], hipGetLastError());
    }
    SampleRed red;
    ProbeStat st;
    if ((rc = read_words(c0, &red, &st))) return rc;
    if (info) fill_info(info, sets[0], expo, red, st);
    moved(sets[0], st);
    for (int i = 1; i < n; i++) {
        ProbeStat sti;
        HIPCHK(ctxs[i], hipMemcpyAsync(&sti, ctxs[i]->prb_stat.p, sizeof(ProbeStat), hipMemcpyDeviceToHost, ctxs[i]->stream));
        HIPCHK(ctxs[i], hipStreamSynchronize(ctxs[i]->stream));   // (member 0's planes are free again only behind every member's move)
        moved(sets[i], sti);
    }
    return SPH_OK;
}

}  // namespace

extern "C" int sph_group_probe_sample(sph_ctx** ctxs, int n, const sph_params* p, sph_probe_set* const* sets, const sph_probe_params* pp, float* values_out,
                                      uint64_t values_bytes, int64_t* raw_out, uint64_t raw_bytes, sph_probe_info* info)
{
    return group_call(ctxs, n, [&] { return group_probe_sample(ctxs, n, p, sets, pp, values_out, values_bytes, raw_out, raw_bytes, info); });
}

extern "C" int sph_group_probe_advect(sph_ctx** ctxs, int n, const sph_params* p, sph_probe_set* const* sets, const sph_probe_advect_params* ap, sph_probe_info* info)
{
    return group_call(ctxs, n, [&] { return group_probe_advect(ctxs, n, p, sets, ap, info); });
}
