// include/sph_slab_candidates.h: the share / merge partner candidates of a SLAB context, filtered on the device, in global ids.
//
// sph_candidates.hip refuses a slab context: its rows are host indices of one vector.  Here every rank filters the rows of the
// particles it owns; what the host assembles by id (distributed.assemble_lists) is the filtered CSR of the whole vector.
//
//   lists    the CSR of the step's lists over the owned rows, entries = SLOT indices (slab_lists_on_device, sph_api.hip), built by the
//            first prepare behind a step and kept across the slab share: that apply overwrites pm[pcur ^ 1], the snapshot
//            k_fill_neighbors reads, and clears grid_valid, so the lists cannot be rebuilt behind it
//   ghosts   refresh_ghosts for the records and the level: a ghost holds what its owner holds NOW (stale behind a share)
//   classes  one byte per slot in a scratch array: an owned slot's from szc (the caller's sph_classify), a ghost's computed by
//            k_classify from its refreshed mass and level -- szc itself is not written
//   count    one thread per owned row; a row that is no donor leaves after one byte load
//   scan     device_exclusive_scan_u32 (sph_adapt.hip): offsets[n + 1], the total in the last word
//   fill     the same walk, writing orig[slot_j] -- the global id -- of every survivor at the row's offset
//
// The records are read in slot space (pm[pcur]): no gather into another order.  Only the two totals cross the bus before
// sph_slab_candidates_download.  Arithmetic: cand_pass (sph_candidates.hpp), the one definition of the two tests.
//
// Collective pattern of slab_adapt (sph_adapt.hip): a failure inside a per-member loop becomes this rank's local_rc and reaches the
// agree() that follows, so no rank waits in a collective for one that left.
#include <hip/hip_runtime.h>

#include <vector>

#include "sph_slab_candidates.h"
#include "sph_candidates.hpp"
#include "sph_dist.hpp"

// ghost[s] = 1 for a ghost slot (the mask k_classify then classifies), cls[s] = the owned slot's class (0xff for a ghost until
// k_classify has run: neither a donor nor a class any test accepts), row_cls[row] = the same byte by row
__global__ __launch_bounds__(256) void k_slab_cand_classes(uint32_t nt, const uint8_t* __restrict__ owned, const uint8_t* __restrict__ szc,
                                                            const uint32_t* __restrict__ slot_row, uint32_t n_rows, uint8_t* __restrict__ ghost,
                                                            uint8_t* __restrict__ cls, uint8_t* __restrict__ row_cls)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nt) return;
    const bool own = owned[s] != 0;
    ghost[s] = own ? 0 : 1;
    const uint8_t c = own ? szc[s] : (uint8_t)0xff;
    cls[s] = c;
    if (own) {
        const uint32_t r = slot_row[s];
        if (r < n_rows) row_cls[r] = c;
    }
}

// ROWS_COUNT: cnt[r] = candidates of row r.  ROWS_FILL: their global ids at out_off[r] (out_off: the scanned counts).  ROWS_MARK
// (sph_slab_partner_problem.hip): the same walk over the same rows; flag[] holds a word per owned slot and, behind those nt words, a word
// per ghost slot -- the donor of a row that is not empty sets its own and every survivor sets its slot's (slot_row: 0xffffffff for a
// ghost).  Many lanes store the same 1 to the same word: plain stores, nobody reads a flag in that launch (as k_prob_mark).
enum { ROWS_COUNT = 0, ROWS_FILL = 1, ROWS_MARK = 2 };
template <int MODE>
__global__ __launch_bounds__(256) void k_slab_cand_rows(uint32_t n_rows, uint32_t nt, CandP q, const uint8_t* __restrict__ row_cls,
                                                         const uint32_t* __restrict__ row_slot, const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx,
                                                         uint64_t tot, const float4* __restrict__ pm, const uint8_t* __restrict__ cls,
                                                         const uint32_t* __restrict__ orig, uint32_t* __restrict__ cnt, const uint32_t* __restrict__ out_off,
                                                         uint32_t* __restrict__ out_idx, const uint32_t* __restrict__ slot_row, uint32_t* __restrict__ flag)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    uint32_t c = 0;
    if (row_cls[r] == q.donor_class) {
        const uint32_t s = row_slot[r];
        if (s < nt) {
            const float4 Ai = pm[s];
            const uint32_t b = off[r];
            const uint64_t e = min((uint64_t)off[r + 1], tot);
            uint32_t w = 0, w_end = 0;
            if (MODE == ROWS_FILL) {
                w = out_off[r];
                w_end = out_off[r + 1];
            }
            for (uint64_t p = b; p < e; p++) {
                const uint32_t j = idx[p];
                if (j == s || j >= nt) continue;
                if (!cand_pass(q, Ai, j, pm, cls)) continue;
                if (MODE == ROWS_FILL) {
                    if (w < w_end) out_idx[w] = orig[j];
                    w++;
                } else if (MODE == ROWS_MARK) {
                    flag[slot_row[j] == 0xffffffffu ? nt + j : j] = 1u;
                    c++;
                } else c++;
            }
            if (MODE == ROWS_MARK && c) flag[s] = 1u;
        }
    }
    if (MODE == ROWS_COUNT) cnt[r] = c;
}

int slab_cand_refuse(sph_ctx* c, const char* what)
{
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s: not a slab context (a plain context takes sph_download_partner_candidates / sph_sum_mass)", what);
    if (c->poisoned) return c->refuse_poisoned();
    return SPH_OK;
}

static float* sel_cand_pm(Member& m) { return m.lv_pmnew; }
static float* sel_cand_lvl(Member& m) { return m.lv_level; }

#define HIPLOC(ctx, call)                                                                                            \
    {                                                                                                                \
        hipError_t e_ = (call);                                                                                      \
        if (e_ != hipSuccess) {                                                                                      \
            local_rc = (ctx)->fail(SPH_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_));                   \
            break;                                                                                                   \
        }                                                                                                            \
    }

// *together: the status came out of an agree() -- every rank leaves with a failure, the transport stays usable
int slab_cand_prepare(Group& G, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_rows, uint64_t* n_indices, bool* together)
{
    const size_t nm = G.m.size();
    int rc = SPH_OK, local_rc = SPH_OK;
    // (as slab_adapt: a poisoned member ends the call before any collective -- the step that poisoned it failed on every rank, and on a
    //  per-rank transport it abandoned the group, whose collectives report that instead of waiting)
    for (auto c : G.m)
        if (c->poisoned) {
            *together = true;
            return slab_cand_refuse(c, "sph_slab_candidates_prepare");
        }
    // ---- lists: the CSR of the step's lists, built once per step
    for (size_t i = 0; i < nm && !local_rc; i++) {
        sph_ctx* c = G.m[i];
        c->slab_rows_open = c->slab_prob_open = false;   // (a slab context, not poisoned: both entry points and the loop above have seen to it)
        if (!c->have_flags) {
            local_rc = c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_candidates_prepare follows a step (it filters that step's lists and reads the neighbours across a cut from its ghost layer)");
            break;
        }
        HIPLOC(c, hipSetDevice(c->device));
        if (c->slab_lists_valid && c->slab_lists_rows == (uint32_t)c->n) continue;
        if (!c->grid_valid) {
            local_rc = c->fail(SPH_ERR_INVALID_ARGUMENT, "no neighbour lists of the step on the device and nothing to build them from: the first sph_slab_candidates_prepare of a step comes before its share");
            break;
        }
        local_rc = slab_lists_on_device(c);
    }
    *together = true;
    if ((rc = agree(G, local_rc))) return rc;
    *together = false;
    // ---- the ghosts' records and levels as their owners hold them now
    std::vector<Member> M(nm);
    for (size_t i = 0; i < nm; i++) {
        sph_ctx* c = G.m[i];
        M[i].c = c;
        M[i].n = c->dist.n_tot;
        M[i].lv_pmnew = (float*)c->pm[c->pcur].as<float4>();
        M[i].lv_level = c->lvl[c->cur].as<float>();
    }
    if ((rc = refresh_ghosts(G, M, sel_cand_pm, 4, "pm"))) return rc;
    if ((rc = refresh_ghosts(G, M, sel_cand_lvl, 1, "level"))) return rc;
    // ---- classes, count, scan, fill
    const CandP q = cand_params(kind, ap);
    const dim3 blk(256);
    for (size_t i = 0; i < nm && !local_rc; i++) {
        sph_ctx* c = G.m[i];
        HIPLOC(c, hipSetDevice(c->device));
        hipStream_t s = c->stream;
        const uint32_t nt = c->dist.n_tot, n = (uint32_t)c->n;
        const int k = c->cur;
        TmpBuf d_ghost;
        HIPLOC(c, d_ghost.ensure((size_t)nt + 4));
        HIPLOC(c, c->cand_cls.ensure((size_t)nt + n + 4));
        HIPLOC(c, c->cand_cnt.ensure((size_t)n * 4 + 4));
        HIPLOC(c, c->cand_off.ensure(((size_t)n + 1) * 4));
        HIPLOC(c, c->cand_scan.ensure(((size_t)n / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
        uint8_t* cls = c->cand_cls.as<uint8_t>();
        uint8_t* row_cls = cls + nt;
        uint32_t* out_off = c->cand_off.as<uint32_t>();
        const dim3 grid_t((nt + 255) / 256), grid_r((n + 255) / 256);
        if (nt) {
            hipLaunchKernelGGL(k_slab_cand_classes, grid_t, blk, 0, s, nt, c->dist.owned.as<uint8_t>(), c->szc[k].as<uint8_t>(), c->slab_slot_row.as<uint32_t>(), n,
                               d_ghost.as<uint8_t>(), cls, row_cls);
            launch_classify(s, &c->prof, nt, c->pm[c->pcur].as<float4>(), c->lvl[k].as<float>(), cls, d_ghost.as<uint8_t>(), c->orig[k].as<uint32_t>(),
                            c->status.as<DeviceStatus>(), p);
        }
        {
            ProfScope ps(&c->prof, "slab_candidates_count", s);
            if (n)
                hipLaunchKernelGGL(k_slab_cand_rows<ROWS_COUNT>, grid_r, blk, 0, s, n, nt, q, row_cls, c->slab_row_slot.as<uint32_t>(), c->slab_off.as<uint32_t>(),
                                   c->slab_idx.as<uint32_t>(), c->slab_lists_tot, c->pm[c->pcur].as<float4>(), cls, c->orig[k].as<uint32_t>(),
                                   c->cand_cnt.as<uint32_t>(), (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr);
            device_exclusive_scan_u32(s, c->cand_cnt.as<uint32_t>(), out_off, n, c->cand_scan.as<uint32_t>(), out_off + n);
        }
        uint32_t tot = 0;
        DeviceStatus st{};
        HIPLOC(c, hipMemcpyAsync(&tot, out_off + n, 4, hipMemcpyDeviceToHost, s));
        HIPLOC(c, hipMemcpyAsync(&st, c->status.p, sizeof st, hipMemcpyDeviceToHost, s));
        HIPLOC(c, hipStreamSynchronize(s));   // (d_ghost goes with this scope)
        if (st.error) {   // a ghost without a level value: LevelEstimationState::level of FluidInterior, as sph_classify reports it for an owned one
            (void)hipMemsetAsync(c->status.p, 0, sizeof(DeviceStatus), s);
            local_rc = c->fail((int)st.error, "sph_slab_candidates_prepare: a ghost particle has no level value (particle i=%u)", st.info);
            break;
        }
        HIPLOC(c, c->cand_idx.ensure((size_t)tot * 4 + 4));
        if (n && tot) {
            ProfScope ps(&c->prof, "slab_candidates_fill", s);
            hipLaunchKernelGGL(k_slab_cand_rows<ROWS_FILL>, grid_r, blk, 0, s, n, nt, q, row_cls, c->slab_row_slot.as<uint32_t>(), c->slab_off.as<uint32_t>(),
                               c->slab_idx.as<uint32_t>(), c->slab_lists_tot, c->pm[c->pcur].as<float4>(), cls, c->orig[k].as<uint32_t>(), (uint32_t*)nullptr,
                               (const uint32_t*)out_off, c->cand_idx.as<uint32_t>(), (const uint32_t*)nullptr, (uint32_t*)nullptr);
        }
        c->slab_rows_open = true;
        c->slab_rows_n = n;
        c->slab_rows_tot = tot;
        n_rows[i] = n;
        n_indices[i] = tot;
    }
    *together = true;
    rc = agree(G, local_rc);
    if (rc)
        for (auto c : G.m) c->slab_rows_open = false;
    return rc;
}

// the walk of the rows prepared last, in ROWS_MARK mode (sph_slab_partner_problem.hip; q: the CandP they were prepared with): queued on the
// context's stream.  flag[2 nt], zeroed by the caller
void slab_cand_mark_launch(sph_ctx* c, const CandP& q, uint32_t* flag)
{
    const uint32_t nt = c->dist.n_tot, n = c->slab_rows_n;
    if (!n || !nt) return;
    const uint8_t* cls = c->cand_cls.as<uint8_t>();
    hipLaunchKernelGGL(k_slab_cand_rows<ROWS_MARK>, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, nt, q, cls + nt, c->slab_row_slot.as<uint32_t>(),
                       c->slab_off.as<uint32_t>(), c->slab_idx.as<uint32_t>(), c->slab_lists_tot, c->pm[c->pcur].as<float4>(), cls, c->orig[c->cur].as<uint32_t>(),
                       (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, c->slab_slot_row.as<uint32_t>(), flag);
}

extern "C" int sph_slab_candidates_prepare(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_rows, uint64_t* n_indices)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    uint64_t rows = 0, tot = 0;
    if (n_rows) *n_rows = 0;
    if (n_indices) *n_indices = 0;
    // (argument refusals are every rank's alike -- the ranks make the same call -- and come before any collective)
    if (!p || !ap) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_candidates_prepare: params and ap must be given");
    if (kind != 0 && kind != 1) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_candidates_prepare: kind %d is neither 0 (share) nor 1 (merge)", kind);
    if (int rc = slab_cand_refuse(c, "sph_slab_candidates_prepare")) return rc;   // (a plain context; a poisoned one, whatever its transport)
    HIPCHK(c, hipSetDevice(c->device));
    Group G;
    G.m.push_back(c);
    int rc = comm_for_rank(c, &G.comm);
    if (rc) return rc;
    if (!G.comm) return c->fail(SPH_ERR_INVALID_ARGUMENT, "a slab context of a loopback group takes sph_group_slab_candidates_prepare");
    bool together = false;
    rc = slab_cand_prepare(G, kind, p, ap, &rows, &tot, &together);
    if (rc && !together) comm_abandon(c);   // (thread / shared-memory transports: the other ranks' next collective reports it instead of waiting)
    if (rc) return rc;
    if (n_rows) *n_rows = rows;
    if (n_indices) *n_indices = tot;
    return SPH_OK;
}

extern "C" int sph_group_slab_candidates_prepare(sph_ctx** ctxs, int n, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_rows,
                                                 uint64_t* n_indices)
{
    if (!ctxs || n <= 0) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]) return SPH_ERR_INVALID_ARGUMENT;
    if (!p || !ap) return ctxs[0]->fail(SPH_ERR_INVALID_ARGUMENT, "sph_group_slab_candidates_prepare: params and ap must be given");
    if (kind != 0 && kind != 1) return ctxs[0]->fail(SPH_ERR_INVALID_ARGUMENT, "sph_group_slab_candidates_prepare: kind %d is neither 0 (share) nor 1 (merge)", kind);
    Group G;
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]->dist.on) return slab_cand_refuse(ctxs[i], "sph_group_slab_candidates_prepare");
        if (ctxs[i]->dist.rank != i || ctxs[i]->dist.nranks != n)
            return ctxs[i]->fail(SPH_ERR_INVALID_ARGUMENT, "context %d is not configured as rank %d of %d (sph_dist_configure)", i, i, n);
        G.m.push_back(ctxs[i]);
    }
    G.comm = comm_loopback();
    std::vector<uint64_t> rows((size_t)n, 0), tot((size_t)n, 0);
    bool together = false;
    const int rc = slab_cand_prepare(G, kind, p, ap, rows.data(), tot.data(), &together);
    for (int i = 0; i < n; i++) {
        if (n_rows) n_rows[i] = rc ? 0 : rows[(size_t)i];
        if (n_indices) n_indices[i] = rc ? 0 : tot[(size_t)i];
    }
    return rc;
}

extern "C" int sph_slab_candidates_download(sph_ctx* c, uint32_t* offsets, uint32_t* indices, uint64_t cap)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = slab_cand_refuse(c, "sph_slab_candidates_download")) return rc;
    if (!c->slab_rows_open || !c->slab_lists_valid || c->slab_rows_n != (uint32_t)c->n)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_candidates_download: no prepared rows (sph_slab_candidates_prepare comes first; a step, an upload, an edit, a merge or a split drops them)");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t n = c->slab_rows_n;
    const uint64_t tot = c->slab_rows_tot;
    if (indices && cap < tot) return c->fail(SPH_ERR_INVALID_ARGUMENT, "indices buffer too small (%llu entries prepared)", (unsigned long long)tot);
    hipStream_t s = c->stream;
    if (offsets) HIPCHK(c, hipMemcpyAsync(offsets, c->cand_off.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s));
    if (indices && tot) HIPCHK(c, hipMemcpyAsync(indices, c->cand_idx.p, (size_t)tot * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

extern "C" int sph_slab_sum_mass(sph_ctx* c, double* total)
{
    if (!c || !total) return SPH_ERR_INVALID_ARGUMENT;
    *total = 0.0;
    if (int rc = slab_cand_refuse(c, "sph_slab_sum_mass")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // (behind a step the arrays also hold the ghosts: k_sum_mass's tree over all slots, a ghost adding 0.0)
    const bool flags = c->have_flags;
    return cand_sum_mass(c, flags ? c->dist.n_tot : (uint32_t)c->n, flags ? c->dist.owned.as<uint8_t>() : nullptr, total);
}
