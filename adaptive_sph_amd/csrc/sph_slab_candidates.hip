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
// The work on the members is the body of each_member, the entry points go through rank_entry / group_entry: the collective rule is
// stated there (sph_dist.hpp).
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
            uint32_t w = 0, w_end = 0;
            if (MODE == ROWS_FILL) {
                w = out_off[r];
                w_end = out_off[r + 1];
            }
            cand_walk_row(q, r, s, nt, pm[s], off, idx, tot, pm, cls, [&](uint32_t j) {
                if (MODE == ROWS_FILL) {
                    if (w < w_end) out_idx[w] = orig[j];
                    w++;
                } else if (MODE == ROWS_MARK) {
                    flag[slot_row[j] == 0xffffffffu ? nt + j : j] = 1u;
                    c++;
                } else c++;
            });
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

// *together: as rank_entry reads it (sph_dist.hpp)
int slab_cand_prepare(Group& G, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_rows, uint64_t* n_indices, bool* together)
{
    int rc = SPH_OK;
    // (as slab_adapt: a poisoned member ends the call before any collective -- the step that poisoned it failed on every rank, and on a
    //  per-rank transport it abandoned the group, whose collectives report that instead of waiting)
    for (auto c : G.m)
        if (c->poisoned) {
            *together = true;
            return slab_cand_refuse(c, "sph_slab_candidates_prepare");
        }
    // ---- lists: the CSR of the step's lists, built once per step
    *together = true;
    rc = each_member(G, [&](size_t, sph_ctx* c) -> int {
        c->slab_rows_open = c->slab_prob_open = false;   // (a slab context, not poisoned: both entry points and the loop above have seen to it)
        if (!c->have_flags)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_candidates_prepare follows a step (it filters that step's lists and reads the neighbours across a cut from its ghost layer)");
        if (c->slab_lists_valid && c->slab_lists_rows == (uint32_t)c->n) return SPH_OK;
        if (!c->grid_valid)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "no neighbour lists of the step on the device and nothing to build them from: the first sph_slab_candidates_prepare of a step comes before its share");
        return slab_lists_on_device(c);
    });
    if (rc) return rc;
    *together = false;
    // ---- the ghosts' records and levels as their owners hold them now
    if ((rc = refresh_ghost_state(G, false))) return rc;
    // ---- classes, count, scan, fill
    const CandP q = cand_params(kind, ap);
    const dim3 blk(256);
    *together = true;
    rc = each_member(G, [&](size_t i, sph_ctx* c) -> int {
        hipStream_t s = c->stream;
        const uint32_t nt = c->dist.n_tot, n = (uint32_t)c->n;
        const int k = c->cur;
        TmpBuf d_ghost;
        HIPCHK(c, d_ghost.ensure((size_t)nt + 4));
        HIPCHK(c, c->cand_cls.ensure((size_t)nt + n + 4));
        HIPCHK(c, c->cand_cnt.ensure((size_t)n * 4 + 4));
        HIPCHK(c, c->cand_off.ensure(((size_t)n + 1) * 4));
        HIPCHK(c, c->cand_scan.ensure(((size_t)n / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
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
        HIPCHK(c, hipMemcpyAsync(&tot, out_off + n, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(&st, c->status.p, sizeof st, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));   // (d_ghost goes with this scope)
        if (st.error) {   // a ghost without a level value: LevelEstimationState::level of FluidInterior, as sph_classify reports it for an owned one
            (void)hipMemsetAsync(c->status.p, 0, sizeof(DeviceStatus), s);
            return c->fail((int)st.error, "sph_slab_candidates_prepare: a ghost particle has no level value (particle i=%u)", st.info);
        }
        HIPCHK(c, c->cand_idx.ensure((size_t)tot * 4 + 4));
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
        return SPH_OK;
    });
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
    if (int rc = cand_check_args(c, "sph_slab_candidates_prepare", kind, p, ap)) return rc;
    if (int rc = slab_cand_refuse(c, "sph_slab_candidates_prepare")) return rc;   // (a plain context; a poisoned one, whatever its transport)
    const int rc = rank_entry(c, "sph_group_slab_candidates_prepare",
                              [&](Group& G, bool* together) -> int { return slab_cand_prepare(G, kind, p, ap, &rows, &tot, together); });
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
    if (int rc = cand_check_args(ctxs[0], "sph_group_slab_candidates_prepare", kind, p, ap)) return rc;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on) return slab_cand_refuse(ctxs[i], "sph_group_slab_candidates_prepare");
    Group G;
    if (int rc = group_entry(G, ctxs, n)) return rc;
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
