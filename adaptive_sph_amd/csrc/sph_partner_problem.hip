// include/sph_partner_problem.h: the partner searches as a compact problem.  The candidate rows of sph_candidates.hip stay what they
// are (cand_count_rows / cand_fill_rows: the same kernels, the same buffers); what is added here is the renumbering of the particles
// those rows touch, so that the host receives K records instead of n and sends K decisions back.
//
//   mark     one thread per host row (the walk of k_cand_rows over the FILLED rows): flag[i] = 1 if row i is not empty, flag[j] = 1
//            for every entry j.  Many lanes store the same 1 to the same word: plain stores, nobody reads a flag in this launch
//   rank     device_exclusive_scan_u32 over the flags: rank[i] = compact id of participant i, K in the last word.  Only K and the
//            candidates' total cross the bus before the bulk copies
//   pack     one thread per host index, a non-participant leaves after one load: ids, the five fields and offsets at rank[i].  The
//            candidate offsets restricted to the participants ARE the compact CSR's offsets (every row in between is empty)
//   relabel  one thread per candidate entry: indices_c[e] = rank[cand_idx[e]]
//   expand   (apply side) merge_partner / merge_counter of the whole vector from the K decisions: AVAILABLE / 0 everywhere, then one
//            thread per compact id scatters its pair, a partner id mapped through ids
//
// The packed arrays (ProbBufs / ProbOut), their download, the host check of compact decisions and expand + apply are the slab problem's
// too (sph_slab_partner_problem.hip, slab_adapt in sph_adapt.hip): prob_out, prob_download, prob_check_decisions, prob_expand below.
//
// All of them are bandwidth-trivial next to the row walk (a few words per particle, coalesced except for the scatter through ids and
// the gather through rank); thread per element, 256-thread blocks like their neighbours in sph_candidates.hip.
#include <hip/hip_runtime.h>

#include "sph_candidates.hpp"
#include "sph_partner_problem.h"

__global__ __launch_bounds__(256) void k_prob_mark(uint32_t n, const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx, uint32_t tot,
                                                    uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = off[i], e = min(off[i + 1], tot);
    if (b >= e) return;
    flag[i] = 1u;
    for (uint32_t p = b; p < e; p++) {
        const uint32_t j = idx[p];
        if (j < n) flag[j] = 1u;
    }
}

// level_estimation in host order beside cand_rec / cand_cls (k_cand_gather's outputs stay what they are)
__global__ __launch_bounds__(256) void k_prob_level(uint32_t n, const uint32_t* __restrict__ orig, const float* __restrict__ lvl, float* __restrict__ lvl_host)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = orig[s];
    if (i < n) lvl_host[i] = lvl[s];
}

__global__ __launch_bounds__(256) void k_prob_pack(uint32_t n, uint32_t K, uint32_t tot, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                    const float4* __restrict__ rec, const uint8_t* __restrict__ cls, const float* __restrict__ lvl_host,
                                                    const uint32_t* __restrict__ cand_off, ProbOut o)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0) o.off[K] = tot;
    if (!flag[i]) return;
    const uint32_t c = rank[i];
    if (c >= K) return;
    const float4 A = rec[i];
    o.ids[c] = i;
    o.cls[c] = cls[i];
    o.mass[c] = A.z;
    o.level[c] = lvl_host[i];
    o.pos[c] = make_float2(A.x, A.y);
    o.h2[c] = A.w;
    o.off[c] = cand_off[i];
}

__global__ __launch_bounds__(256) void k_prob_relabel(uint32_t tot, uint32_t n, const uint32_t* __restrict__ cand_idx, const uint32_t* __restrict__ rank,
                                                       uint32_t* __restrict__ idx_c)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const uint32_t j = cand_idx[e];
    idx_c[e] = j < n ? rank[j] : 0u;
}

// (n: the particles of the whole vector -- of all ranks on a slab context, where the ids are the caller's: neither an id nor a mapped
//  partner outside it is written.  The problem's own ids of a plain context are inside it by construction)
__global__ __launch_bounds__(256) void k_prob_expand(uint32_t K, uint32_t n, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ partner_c,
                                                      const uint16_t* __restrict__ counter_c, uint32_t* __restrict__ partner, uint16_t* __restrict__ counter)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    const uint32_t i = ids[c];
    if (i >= n) return;   // (the host check refused it)
    uint32_t pc = partner_c[c];
    if (pc != SPH_MERGE_PARTNER_AVAILABLE && pc != SPH_MERGE_PARTNER_DELETE) {
        pc = pc < K ? ids[pc] : SPH_MERGE_PARTNER_AVAILABLE;   // (the host check refused pc >= K)
        if (pc >= n) pc = SPH_MERGE_PARTNER_AVAILABLE;
    }
    partner[i] = pc;
    counter[i] = counter_c[c];
}

int prob_out(sph_ctx* c, ProbBufs& b, size_t K, size_t n_off, ProbOut* o)
{
    HIPCHK(c, b.ids.ensure(K * 4));
    HIPCHK(c, b.cls.ensure(K));
    HIPCHK(c, b.mass.ensure(K * 4));
    HIPCHK(c, b.level.ensure(K * 4));
    HIPCHK(c, b.pos.ensure(K * 8));
    HIPCHK(c, b.h2.ensure(K * 4));
    HIPCHK(c, b.off.ensure((n_off + 1) * 4));
    *o = ProbOut{b.ids.as<uint32_t>(), b.cls.as<uint8_t>(), b.mass.as<float>(), b.level.as<float>(), b.pos.as<float2>(), b.h2.as<float>(), b.off.as<uint32_t>()};
    return SPH_OK;
}

int prob_download(sph_ctx* c, const ProbBufs& b, size_t K, size_t n_off, uint64_t tot, const void* d_indices, uint32_t* ids, uint8_t* size_class, float* mass,
                  float* level, float* position, float* h2, uint32_t* offsets, uint32_t* indices)
{
    if (!K) {
        if (offsets) offsets[0] = 0;
        return SPH_OK;
    }
    hipStream_t s = c->stream;
    if (ids) HIPCHK(c, hipMemcpyAsync(ids, b.ids.p, K * 4, hipMemcpyDeviceToHost, s));
    if (size_class) HIPCHK(c, hipMemcpyAsync(size_class, b.cls.p, K, hipMemcpyDeviceToHost, s));
    if (mass) HIPCHK(c, hipMemcpyAsync(mass, b.mass.p, K * 4, hipMemcpyDeviceToHost, s));
    if (level) HIPCHK(c, hipMemcpyAsync(level, b.level.p, K * 4, hipMemcpyDeviceToHost, s));
    if (position) HIPCHK(c, hipMemcpyAsync(position, b.pos.p, K * 8, hipMemcpyDeviceToHost, s));
    if (h2) HIPCHK(c, hipMemcpyAsync(h2, b.h2.p, K * 4, hipMemcpyDeviceToHost, s));
    if (offsets) HIPCHK(c, hipMemcpyAsync(offsets, b.off.p, (n_off + 1) * 4, hipMemcpyDeviceToHost, s));
    if (indices && tot) HIPCHK(c, hipMemcpyAsync(indices, d_indices, (size_t)tot * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

int prob_check_decisions(sph_ctx* c, const char* what, uint64_t K, const uint32_t* ids, const uint32_t* partner_c)
{
    for (uint64_t i = 0; i < K; i++) {
        if (ids && i && ids[i] <= ids[i - 1]) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: ids is not strictly ascending (entry %llu: %u after %u)", what, (unsigned long long)i, ids[i], ids[i - 1]);
        if (partner_c[i] >= K && partner_c[i] != SPH_MERGE_PARTNER_AVAILABLE && partner_c[i] != SPH_MERGE_PARTNER_DELETE)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: partner_c holds an id outside the problem (compact id %llu: %u)", what, (unsigned long long)i, partner_c[i]);
    }
    return SPH_OK;
}

// (ExpandStage) the host's array *p of K words goes up into `stage` and *p becomes the copy's address
template <class T>
static int expand_staged(sph_ctx* c, DevBuf* stage, const T** p, uint32_t K)
{
    if (!stage) return SPH_OK;
    HIPCHK(c, stage->ensure((size_t)K * sizeof(T) + 4));
    HIPCHK(c, hipMemcpyAsync(stage->p, *p, (size_t)K * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *p = (const T*)stage->p;
    return SPH_OK;
}

int prob_expand(sph_ctx* c, const char* scope, uint32_t n, uint32_t K, const uint32_t* ids, const uint32_t* partner_c, const uint16_t* counter_c, uint32_t* d_partner,
                uint16_t* d_counter, ExpandStage stage)
{
    hipStream_t s = c->stream;
    ProfScope ps(&c->prof, scope, s);
    HIPCHK(c, hipMemsetAsync(d_partner, 0xff, (size_t)n * 4, s));   // SPH_MERGE_PARTNER_AVAILABLE
    HIPCHK(c, hipMemsetAsync(d_counter, 0, (size_t)n * 2, s));
    if (!K) return SPH_OK;
    if (int rc = expand_staged(c, stage.ids, &ids, K)) return rc;
    if (int rc = expand_staged(c, stage.partner_c, &partner_c, K)) return rc;
    if (int rc = expand_staged(c, stage.counter_c, &counter_c, K)) return rc;
    hipLaunchKernelGGL(k_prob_expand, dim3((K + 255) / 256), dim3(256), 0, s, K, n, ids, partner_c, counter_c, d_partner, d_counter);
    return SPH_OK;
}

// mark / rank / pack / relabel on the device, no bulk copy: the compact problem of `kind` in prob_ids .. prob_idx (see the head of this
// file).  n > 0 or not; *K / *tot are set once they are known (one 4-byte copy each), also when `caps` then refuses the sizes.
int prob_build_on_device(sph_ctx* c, int kind, const sph_adapt_params* ap, const char* what, const ProbCaps* caps, uint32_t* K_out, uint32_t* tot_out)
{
    const uint32_t n = (uint32_t)c->n;
    hipStream_t s = c->stream;
    const dim3 grid((n + 255) / 256), blk(256);
    uint32_t tot = 0, K = 0;
    if (n) {
        const CandP q = cand_params(kind, ap);
        if (int rc = cand_count_rows(c, q, nullptr, &tot)) return rc;
        if (tot) {
            if (int rc = cand_fill_rows(c, q, tot)) return rc;
            HIPCHK(c, c->prob_flag.ensure((size_t)n * 4));
            HIPCHK(c, c->prob_rank.ensure(((size_t)n + 1) * 4));
            HIPCHK(c, c->cand_scan.ensure(((size_t)n / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
            {
                ProfScope ps(&c->prof, "problem_mark", s);
                HIPCHK(c, hipMemsetAsync(c->prob_flag.p, 0, (size_t)n * 4, s));
                hipLaunchKernelGGL(k_prob_mark, grid, blk, 0, s, n, (const uint32_t*)c->cand_off.as<uint32_t>(), (const uint32_t*)c->cand_idx.as<uint32_t>(), tot,
                                   c->prob_flag.as<uint32_t>());
                device_exclusive_scan_u32(s, c->prob_flag.as<uint32_t>(), c->prob_rank.as<uint32_t>(), n, c->cand_scan.as<uint32_t>(), c->prob_rank.as<uint32_t>() + n);
            }
            HIPCHK(c, hipMemcpyAsync(&K, c->prob_rank.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (K == 0 || K > n) return c->fail(SPH_ERR_DEVICE, "%s: %u candidates but %u participants of %u particles", what, tot, K, n);
        }
    }
    *K_out = K;
    *tot_out = tot;
    if (caps && caps->participants_given && caps->participants < K) return c->fail(SPH_ERR_INVALID_ARGUMENT, "participant buffers too small");
    if (caps && caps->indices_given && caps->indices < tot) return c->fail(SPH_ERR_INVALID_ARGUMENT, "indices buffer too small");
    if (K) {
        ProbOut out;
        HIPCHK(c, c->prob_lvl.ensure((size_t)n * 4));
        if (int rc = prob_out(c, c->prob, K, K, &out)) return rc;
        HIPCHK(c, c->prob_idx.ensure((size_t)tot * 4));
        ProfScope ps(&c->prof, "problem_pack", s);
        hipLaunchKernelGGL(k_prob_level, grid, blk, 0, s, n, (const uint32_t*)c->orig[c->cur].as<uint32_t>(), (const float*)c->lvl[c->cur].as<float>(),
                           c->prob_lvl.as<float>());
        hipLaunchKernelGGL(k_prob_pack, grid, blk, 0, s, n, K, tot, (const uint32_t*)c->prob_flag.as<uint32_t>(), (const uint32_t*)c->prob_rank.as<uint32_t>(),
                           (const float4*)c->cand_rec.as<float4>(), (const uint8_t*)c->cand_cls.as<uint8_t>(), (const float*)c->prob_lvl.as<float>(),
                           (const uint32_t*)c->cand_off.as<uint32_t>(), out);
        hipLaunchKernelGGL(k_prob_relabel, dim3((tot + 255) / 256), blk, 0, s, tot, n, (const uint32_t*)c->cand_idx.as<uint32_t>(),
                           (const uint32_t*)c->prob_rank.as<uint32_t>(), c->prob_idx.as<uint32_t>());
    }
    return SPH_OK;
}

void prob_open_problem(sph_ctx* c, int kind, uint32_t K)
{
    c->prob_open = true;
    c->prob_kind = kind;
    c->prob_k = K;
    c->prob_serial++;   // (a solution of an earlier problem is not one of this problem: sph_partner_search.hip)
}

int prob_apply(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, int merging, const uint32_t* partner_c, const uint16_t* counter_c, bool on_host)
{
    c->prob_open = false;   // consumed, and a solution with it
    const uint32_t n = (uint32_t)c->n;
    if (merging) c->drop(DROPS_EXPORT_EARLY);   // (as sph_merge_particles: the lists index the vector before the deletions)
    if (n == 0) return SPH_OK;
    TmpBuf d_partner, d_counter, up_partner, up_counter;
    if (d_partner.ensure((size_t)n * 4) != hipSuccess || d_counter.ensure((size_t)n * 2) != hipSuccess) return c->fail(SPH_ERR_DEVICE, "out of device memory");
    if (int rc = prob_expand(c, "problem_expand", n, c->prob_k, c->prob.ids.as<uint32_t>(), partner_c, counter_c, d_partner.as<uint32_t>(), d_counter.as<uint16_t>(),
                             ExpandStage{nullptr, on_host ? &up_partner : nullptr, on_host ? &up_counter : nullptr}))
        return rc;
    return transfer_on_device(c, p, ap, d_partner.as<uint32_t>(), d_counter.as<uint16_t>(), merging);
}

extern "C" int sph_download_partner_problem(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t* ids, uint8_t* size_class, float* mass,
                                            float* level, float* position, float* h2, uint32_t* offsets, uint64_t pcap, uint32_t* indices, uint64_t icap,
                                            uint64_t* n_participants, uint64_t* n_indices)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (n_participants) *n_participants = 0;
    if (n_indices) *n_indices = 0;
    c->prob_open = false;   // (this call replaces the open problem, or closes it)
    if (int rc = cand_check_args(c, "sph_download_partner_problem", kind, p, ap)) return rc;
    if (int rc = cand_refuse_common(c, "sph_download_partner_problem")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = cand_need_lists(c)) return rc;
    uint32_t tot = 0, K = 0;
    const ProbCaps caps{ids || size_class || mass || level || position || h2 || offsets, pcap, indices != nullptr, icap};
    const int rc = prob_build_on_device(c, kind, ap, "sph_download_partner_problem", &caps, &K, &tot);
    if (n_participants) *n_participants = K;
    if (n_indices) *n_indices = tot;
    if (rc) return rc;
    if (int rc2 = prob_download(c, c->prob, K, K, tot, c->prob_idx.p, ids, size_class, mass, level, position, h2, offsets, indices)) return rc2;
    prob_open_problem(c, kind, K);
    return SPH_OK;
}

static int apply_compact(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* partner_c, const uint16_t* counter_c, int merging)
{
    const char* what = merging ? "sph_merge_particles_compact" : "sph_share_particles_compact";
    if (!c || !p || !ap) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = cand_refuse_common(c, what)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->prob_open) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open problem (sph_download_partner_problem comes first; a step, an upload, an edit, a merge or a split closes it)", what);
    if (c->prob_kind != merging) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: the open problem is of kind %d", what, c->prob_kind);
    if (k != c->prob_k) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: k=%llu, the open problem has %u participants", what, (unsigned long long)k, c->prob_k);
    if (k && (!partner_c || !counter_c)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: partner_c and counter_c must be given", what);
    if (int rc = prob_check_decisions(c, what, k, nullptr, partner_c)) return rc;
    return prob_apply(c, p, ap, merging, partner_c, counter_c, true);
}

extern "C" int sph_share_particles_compact(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* partner_c, const uint16_t* counter_c)
{
    return apply_compact(c, p, ap, k, partner_c, counter_c, 0);
}

extern "C" int sph_merge_particles_compact(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* partner_c, const uint16_t* counter_c)
{
    return apply_compact(c, p, ap, k, partner_c, counter_c, 1);
}
