// include/sph_slab_partner_problem.h: the rank's LOCAL partner problem of a slab context -- sph_partner_problem.hip's renumbering on the
// rows of sph_slab_candidates.hip.  The prepare of sph_slab_candidates.h runs first, unchanged (lists, ghost refresh, classes, count, scan,
// fill: cand_cls, cand_off, cand_idx); what is added here, per member and on its stream:
//
//   mark    2 n_tot flag words, zeroed: [0, n_tot) the owned slots, [n_tot, 2 n_tot) the ghost slots.  The row walk once more
//           (k_slab_cand_rows<ROWS_MARK>: the fill writes global ids, the survivors' SLOTS are known only inside the walk): a donor with a
//           survivor flags itself and every survivor.  Plain stores, nobody reads a flag in that launch
//   scan    device_exclusive_scan_u32 over the 2 n_tot words: rank[t] is the local id.  Owned participants come first in slot order -- the
//           rows are the owned slots in slot order (slab_lists_on_device), so that is row order -- and the ghosts behind them in slot
//           order.  rank[n_tot] = the owned participants, the last word = all of them: the two words that cross the bus
//   pack    one thread per flag word, a non-participant leaves after one load: global id (orig), class (the per-slot scratch of the
//           prepare: szc for an owned slot, k_classify on the refreshed record for a ghost), mass / position / h2 from the slot's record
//           -- the words sph_download reads --, level from lvl.  An owned participant also writes offsets[c] = cand_off[row]: every row
//           between two owned participants is empty, so the prepared offsets restricted to them are the local CSR's (as k_prob_pack)
//
// The entries stay in cand_idx (global ids).  A few words per slot, coalesced except for the scatter through rank: thread per element,
// 256-thread blocks, like sph_partner_problem.hip, whose packed arrays and download these are (ProbBufs, prob_out, prob_download).
// Collective rule: each_member / rank_entry / group_entry (sph_dist.hpp).
#include <hip/hip_runtime.h>

#include <vector>

#include "sph_slab_partner_problem.h"
#include "sph_candidates.hpp"
#include "sph_dist.hpp"

__global__ __launch_bounds__(256) void k_slab_prob_pack(uint32_t nt, uint32_t K, uint32_t Ko, uint32_t n_rows, uint32_t tot, const uint32_t* __restrict__ flag,
                                                         const uint32_t* __restrict__ rank, const uint32_t* __restrict__ orig, const uint8_t* __restrict__ cls,
                                                         const float4* __restrict__ pm, const float* __restrict__ lvl, const uint32_t* __restrict__ slot_row,
                                                         const uint32_t* __restrict__ cand_off, ProbOut o)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2u * nt) return;
    if (t == 0) o.off[Ko] = tot;
    if (!flag[t]) return;
    const uint32_t c = rank[t];
    if (c >= K) return;
    const bool own = t < nt;
    const uint32_t s = own ? t : t - nt;
    const float4 A = pm[s];
    o.ids[c] = orig[s];
    o.cls[c] = cls[s];
    o.mass[c] = A.z;
    o.level[c] = lvl[s];
    o.pos[c] = make_float2(A.x, A.y);
    o.h2[c] = A.w;
    if (own && c < Ko) {
        const uint32_t r = slot_row[s];
        o.off[c] = r < n_rows ? cand_off[r] : tot;
    }
}

int slab_prob_prepare(Group& G, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_part, uint64_t* n_owned, uint64_t* n_indices, bool* together)
{
    const size_t nm = G.m.size();
    std::vector<uint64_t> rows(nm, 0), tots(nm, 0);
    int rc = slab_cand_prepare(G, kind, p, ap, rows.data(), tots.data(), together);   // (it closes the members' problems first)
    if (rc) return rc;
    const CandP q = cand_params(kind, ap);
    rc = each_member(G, [&](size_t i, sph_ctx* c) -> int {
        hipStream_t s = c->stream;
        const uint32_t nt = c->dist.n_tot, n = c->slab_rows_n, tot = (uint32_t)c->slab_rows_tot;
        uint32_t K = 0, Ko = 0;
        if (n && nt && tot) {
            const size_t words = 2 * (size_t)nt;
            HIPCHK(c, c->slab_prob_flag.ensure(words * 4));
            HIPCHK(c, c->slab_prob_rank.ensure((words + 1) * 4));
            HIPCHK(c, c->cand_scan.ensure((words / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
            uint32_t* rank = c->slab_prob_rank.as<uint32_t>();
            {
                ProfScope ps(&c->prof, "slab_problem_mark", s);
                HIPCHK(c, hipMemsetAsync(c->slab_prob_flag.p, 0, words * 4, s));
                slab_cand_mark_launch(c, q, c->slab_prob_flag.as<uint32_t>());
                device_exclusive_scan_u32(s, c->slab_prob_flag.as<uint32_t>(), rank, (uint32_t)words, c->cand_scan.as<uint32_t>(), rank + words);
            }
            HIPCHK(c, hipMemcpyAsync(&Ko, rank + nt, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(&K, rank + words, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (K == 0 || Ko == 0 || Ko > K || Ko > n || K > words)
                return c->fail(SPH_ERR_DEVICE, "sph_slab_partner_problem_prepare: %u candidates but %u participants (%u owned) of %u slots", tot, K, Ko, nt);
            ProbOut out;
            if (int rc2 = prob_out(c, c->slab_prob, K, Ko, &out)) return rc2;
            ProfScope ps(&c->prof, "slab_problem_pack", s);
            hipLaunchKernelGGL(k_slab_prob_pack, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, s, nt, K, Ko, n, tot, (const uint32_t*)c->slab_prob_flag.as<uint32_t>(),
                               (const uint32_t*)rank, (const uint32_t*)c->orig[c->cur].as<uint32_t>(), (const uint8_t*)c->cand_cls.as<uint8_t>(),
                               (const float4*)c->pm[c->pcur].as<float4>(), (const float*)c->lvl[c->cur].as<float>(), (const uint32_t*)c->slab_slot_row.as<uint32_t>(),
                               (const uint32_t*)c->cand_off.as<uint32_t>(), out);
            HIPCHK(c, hipStreamSynchronize(s));   // (the snapshot is complete before anybody changes the records it was packed from)
        }
        c->slab_prob_open = true;
        c->slab_prob_serial++;   // (a solution of an earlier problem is not one of this problem: sph_slab_partner_search.hip)
        c->slab_prob_k = K;
        c->slab_prob_ko = Ko;
        n_part[i] = K;
        n_owned[i] = Ko;
        n_indices[i] = tot;
        return SPH_OK;
    });
    if (rc)
        for (auto c : G.m) c->slab_prob_open = false;   // (the rows of sph_slab_candidates_prepare stay: they are complete)
    return rc;
}

extern "C" int sph_slab_partner_problem_prepare(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_participants,
                                                uint64_t* n_owned_participants, uint64_t* n_indices)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    uint64_t K = 0, Ko = 0, tot = 0;
    if (n_participants) *n_participants = 0;
    if (n_owned_participants) *n_owned_participants = 0;
    if (n_indices) *n_indices = 0;
    // (argument refusals are every rank's alike -- the ranks make the same call -- and come before any collective)
    if (int rc = cand_check_args(c, "sph_slab_partner_problem_prepare", kind, p, ap)) return rc;
    if (int rc = slab_cand_refuse(c, "sph_slab_partner_problem_prepare")) return rc;
    const int rc = rank_entry(c, "sph_group_slab_partner_problem_prepare",
                              [&](Group& G, bool* together) -> int { return slab_prob_prepare(G, kind, p, ap, &K, &Ko, &tot, together); });
    if (rc) return rc;
    if (n_participants) *n_participants = K;
    if (n_owned_participants) *n_owned_participants = Ko;
    if (n_indices) *n_indices = tot;
    return SPH_OK;
}

extern "C" int sph_group_slab_partner_problem_prepare(sph_ctx** ctxs, int n, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_participants,
                                                      uint64_t* n_owned_participants, uint64_t* n_indices)
{
    if (!ctxs || n <= 0) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++) {
        if (n_participants) n_participants[i] = 0;
        if (n_owned_participants) n_owned_participants[i] = 0;
        if (n_indices) n_indices[i] = 0;
    }
    if (int rc = cand_check_args(ctxs[0], "sph_group_slab_partner_problem_prepare", kind, p, ap)) return rc;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on) return slab_cand_refuse(ctxs[i], "sph_group_slab_partner_problem_prepare");
    Group G;
    if (int rc = group_entry(G, ctxs, n)) return rc;
    std::vector<uint64_t> K((size_t)n, 0), Ko((size_t)n, 0), tot((size_t)n, 0);
    bool together = false;
    const int rc = slab_prob_prepare(G, kind, p, ap, K.data(), Ko.data(), tot.data(), &together);
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        if (n_participants) n_participants[i] = K[(size_t)i];
        if (n_owned_participants) n_owned_participants[i] = Ko[(size_t)i];
        if (n_indices) n_indices[i] = tot[(size_t)i];
    }
    return SPH_OK;
}

extern "C" int sph_slab_partner_problem_download(sph_ctx* c, uint32_t* ids, uint8_t* size_class, float* mass, float* level, float* position, float* h2,
                                                 uint32_t* offsets, uint64_t pcap, uint32_t* indices, uint64_t icap, uint64_t* n_participants,
                                                 uint64_t* n_owned_participants, uint64_t* n_indices)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (n_participants) *n_participants = 0;
    if (n_owned_participants) *n_owned_participants = 0;
    if (n_indices) *n_indices = 0;
    if (int rc = slab_cand_refuse(c, "sph_slab_partner_problem_download")) return rc;
    if (!c->slab_prob_open || !c->slab_rows_open || !c->slab_lists_valid || c->slab_rows_n != (uint32_t)c->n)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_partner_problem_download: no prepared problem (sph_slab_partner_problem_prepare comes first; a step, an upload, an edit, a merge, a split or sph_slab_candidates_prepare drops it)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t K = c->slab_prob_k, Ko = c->slab_prob_ko;
    const uint64_t tot = c->slab_rows_tot;
    if (n_participants) *n_participants = K;
    if (n_owned_participants) *n_owned_participants = Ko;
    if (n_indices) *n_indices = tot;
    if ((ids || size_class || mass || level || position || h2 || offsets) && pcap < K)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "participant buffers too small (%llu participants prepared)", (unsigned long long)K);
    if (indices && icap < tot) return c->fail(SPH_ERR_INVALID_ARGUMENT, "indices buffer too small (%llu entries prepared)", (unsigned long long)tot);
    return prob_download(c, c->slab_prob, K, Ko, tot, c->cand_idx.p, ids, size_class, mass, level, position, h2, offsets, indices);
}
