// include/sph_slab_partner_search.h: the partner searches of a slab GROUP on the device.  The prepare of sph_slab_partner_problem.hip runs
// first, unchanged (every member's local problem in its slab_prob arrays, the entries in cand_idx, global ids); what is added here:
//
//   staging  every member's packed arrays to the ROOT's device (ss_stage: the members' ids side by side, then per member its five
//            fields, offsets and entries): hipMemcpyPeerAsync between two devices, a device-to-device copy on one, queued on the root's
//            stream behind an event of the member's stream.  No kernel reads another device's memory.  (slab_merge_on_root.  Everything below
//            is slab_merge_staged, which the per-process form -- sph_rank_partner_search.hip: staging by a relay -- calls as well)
//   mark     flag[n_global], zeroed; one thread per reported id stores 1 (plain stores of equal values, nobody reads a flag in that
//            launch); an id >= n_global sets the error word and is skipped
//   scan     device_exclusive_scan_u32 over the flags: rank[g] = compact id, K in the last word; ids_c[rank[g]] = g (one thread per
//            global id): ascending, as distributed.merge_slab_partner_problems orders them
//   fields   ONE LAUNCH PER MEMBER, in rank order, one thread per local participant.  Seen for the first time (a byte per compact id):
//            its five fields are written.  Seen before: they are compared bit for bit, a difference sets the error word -- picking one
//            value would hide a stale ghost (the rule merge_slab_partner_problems states).  An owned participant writes rowlen[c] from
//            its offsets; a second owner sets the error word.  Ids are unique within a member's problem: a launch has no race
//   rows     rowlen[c] is 0 for everyone nobody owns a row of; scan -> off_c[K + 1]; one thread per owned participant copies its row to
//            off_c[c], every entry relabelled through rank[] (an entry that names no participant sets the error word)
//   solve    ps_solve (sph_partner_search.hip) on the root: writers CSR, first, resident / wide rounds, validate
//   hand-over  ids_c, partner_c, counter_c to every member's slab_sol_* buffers, on the root's stream; every member's stream waits for
//            the event behind them
//
// The merged problem lands in the root's prob / prob_idx buffers, which a slab context has no other use for.  Every index a kernel forms
// is checked against the counts the host read (K_i, Ko_i, T_i of the prepare, n_global, K, the rows' total): bad input ends in the error
// word, never in an access outside an array.  A few words per participant: thread per element, 256-thread blocks, like
// sph_partner_problem.hip.
#include <hip/hip_runtime.h>

#include <vector>

#include "sph_slab_partner_search.h"
#include "sph_candidates.hpp"
#include "sph_dist.hpp"

enum : uint32_t { SM_ERR_ID = 1, SM_ERR_BITS = 2, SM_ERR_OWNERS = 3, SM_ERR_ENTRY = 4, SM_ERR_ROWS = 5 };

__global__ __launch_bounds__(256) void k_slab_merge_mark(uint32_t n_ids, const uint32_t* __restrict__ ids, uint32_t n_global, uint32_t* __restrict__ flag,
                                                          uint32_t* __restrict__ err)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_ids) return;
    const uint32_t g = ids[t];
    if (g >= n_global) {
        *err = SM_ERR_ID;
        return;
    }
    flag[g] = 1u;
}

__global__ __launch_bounds__(256) void k_slab_merge_ids(uint32_t n_global, uint32_t K, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                         uint32_t* __restrict__ ids_c)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_global || !flag[g]) return;
    const uint32_t c = rank[g];
    if (c < K) ids_c[c] = g;
}

__global__ __launch_bounds__(256) void k_slab_merge_fields(SmPart q, uint32_t n_global, uint32_t K, const uint32_t* __restrict__ flag,
                                                            const uint32_t* __restrict__ rank, ProbOut o, uint8_t* __restrict__ seen, uint32_t* __restrict__ rowlen,
                                                            uint32_t* __restrict__ err)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= q.K) return;
    const uint32_t g = q.ids[t];
    if (g >= n_global || !flag[g]) {   // (the mark launch reported it)
        *err = SM_ERR_ID;
        return;
    }
    const uint32_t c = rank[g];
    if (c >= K) {
        *err = SM_ERR_ID;
        return;
    }
    const uint8_t cls = q.cls[t];
    const float m = q.mass[t], l = q.level[t], h = q.h2[t];
    const float2 x = q.pos[t];
    uint8_t sn = seen[c];
    if (!(sn & 1u)) {
        o.cls[c] = cls;
        o.mass[c] = m;
        o.level[c] = l;
        o.pos[c] = x;
        o.h2[c] = h;
        sn = 1u;
    } else {
        const float2 y = o.pos[c];
        if (o.cls[c] != cls || __float_as_uint(o.mass[c]) != __float_as_uint(m) || __float_as_uint(o.level[c]) != __float_as_uint(l) ||
            __float_as_uint(y.x) != __float_as_uint(x.x) || __float_as_uint(y.y) != __float_as_uint(x.y) || __float_as_uint(o.h2[c]) != __float_as_uint(h))
            *err = SM_ERR_BITS;
    }
    if (t < q.Ko) {
        if (sn & 2u) *err = SM_ERR_OWNERS;
        else {
            const uint32_t b = q.off[t], e = q.off[t + 1];
            if (e < b || e > q.T) *err = SM_ERR_ROWS;
            else rowlen[c] = e - b;
            sn |= 2u;
        }
    }
    seen[c] = sn;
}

__global__ __launch_bounds__(256) void k_slab_merge_rows(SmPart q, uint32_t n_global, uint32_t K, uint32_t tot_c, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ rank, const uint32_t* __restrict__ off_c, uint32_t* __restrict__ idx_c,
                                                          uint32_t* __restrict__ err)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= q.Ko || t >= q.K) return;
    const uint32_t g = q.ids[t];
    if (g >= n_global || !flag[g]) return;
    const uint32_t c = rank[g];
    if (c >= K) return;
    const uint32_t b = q.off[t], e = min(q.off[t + 1], q.T);
    if (b >= e) return;
    const uint32_t dst = off_c[c];
    if (off_c[c + 1] - dst != e - b || off_c[c + 1] > tot_c) {   // (the row this owner announced in the fields launch)
        *err = SM_ERR_ROWS;
        return;
    }
    for (uint32_t p = b; p < e; p++) {
        const uint32_t j = q.idx[p];
        uint32_t cj = 0u;
        if (j < n_global && flag[j] && rank[j] < K) cj = rank[j];
        else *err = SM_ERR_ENTRY;
        idx_c[dst + (p - b)] = cj;
    }
}

static const char* sm_error_text(uint32_t e)
{
    switch (e) {
    case SM_ERR_ID: return "a rank reports a participant id outside the group's particle vector";
    case SM_ERR_BITS: return "a particle comes with different field bits from two ranks (a stale ghost)";
    case SM_ERR_OWNERS: return "a particle is owned by two ranks";
    case SM_ERR_ENTRY: return "a candidate entry names no participant";
    case SM_ERR_ROWS: return "a rank's offsets do not describe its entries";
    }
    return "unknown error";
}

// an event of one call, made on the device that is current, destroyed on every path out
struct SmEvent {
    hipEvent_t e = nullptr;
    hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    ~SmEvent()
    {
        if (e) (void)hipEventDestroy(e);
    }
};

// `bytes` from src on device src_dev to dst on device dst_dev, queued on s
static hipError_t sm_copy(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t s)
{
    if (!bytes) return hipSuccess;
    if (dst_dev != src_dev) return hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, s);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
}

// what every entry point of this header refuses first; fills G
static int slab_search_entry(Group& G, sph_ctx** ctxs, int n, const char* what)
{
    if (!ctxs || n <= 0) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on) return ctxs[i]->fail(SPH_ERR_UNSUPPORTED, "%s: context %d is not a slab context (a plain context takes sph_find_partners_device)", what, i);
    for (int i = 0; i < n; i++)
        if (ctxs[i]->poisoned) return ctxs[i]->refuse_poisoned();
    return group_entry(G, ctxs, n);
}

// STAGING, the group form: the members' packed arrays copied to the root's device (peer copies between two devices), the members' ids
// side by side in front; then THE MERGE (slab_merge_staged, below) on what was staged.  The per-process form stages by a relay over the
// ranks' transport instead (sph_rank_partner_search.hip) and calls the same merge.
static int slab_merge_on_root(Group& G, size_t root, const char* what, const uint64_t* Ki, const uint64_t* Koi, const uint64_t* Ti, uint32_t n_global, uint32_t* K_out,
                              uint32_t* tot_out)
{
    const size_t nm = G.m.size();
    sph_ctx* r = G.m[root];
    *K_out = *tot_out = 0;
    uint64_t sum_k = 0;
    for (size_t i = 0; i < nm; i++) sum_k += Ki[i];
    if (sum_k == 0) return SPH_OK;
    // ---- where each member's arrays sit in the staging buffer (16-byte aligned)
    struct Place {
        size_t ids, cls, mass, level, pos, h2, off, idx;
    };
    std::vector<Place> at(nm);
    size_t bytes = 0;
    auto take = [&](size_t b) {
        const size_t a = bytes;
        bytes += (b + 15) & ~(size_t)15;
        return a;
    };
    for (size_t i = 0; i < nm; i++) {   // (the members' ids side by side: ONE mark launch reads them all)
        at[i].ids = bytes;
        bytes += (size_t)Ki[i] * 4;
    }
    bytes = (bytes + 15) & ~(size_t)15;
    for (size_t i = 0; i < nm; i++) {
        const size_t k = (size_t)Ki[i];
        at[i].cls = take(k);
        at[i].mass = take(k * 4);
        at[i].level = take(k * 4);
        at[i].pos = take(k * 8);
        at[i].h2 = take(k * 4);
        at[i].off = take(((size_t)Koi[i] + 1) * 4);
        at[i].idx = take((size_t)Ti[i] * 4);
    }
    // ---- every member's stream has packed (the prepare waited for it; the event keeps the order where it does not)
    std::vector<SmEvent> packed(nm);
    for (size_t i = 0; i < nm; i++) {
        sph_ctx* c = G.m[i];
        if (i == root || !Ki[i]) continue;
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, packed[i].create());
        HIPCHK(c, hipEventRecord(packed[i].e, c->stream));
    }
    HIPCHK(r, hipSetDevice(r->device));
    hipStream_t s = r->stream;
    HIPCHK(r, r->ss_stage.ensure(bytes + 16));
    uint8_t* stage = r->ss_stage.as<uint8_t>();
    std::vector<SmPart> part(nm);
    {
        ProfScope ps(&r->prof, "slab_search_stage", s);
        for (size_t i = 0; i < nm; i++) {
            sph_ctx* c = G.m[i];
            const size_t k = (size_t)Ki[i], ko = (size_t)Koi[i], t = (size_t)Ti[i];
            part[i] = SmPart{(const uint32_t*)(stage + at[i].ids), stage + at[i].cls, (const float*)(stage + at[i].mass), (const float*)(stage + at[i].level),
                             (const float2*)(stage + at[i].pos), (const float*)(stage + at[i].h2), (const uint32_t*)(stage + at[i].off), (const uint32_t*)(stage + at[i].idx),
                             (uint32_t)k, (uint32_t)ko, (uint32_t)t};
            if (!k) continue;
            if (packed[i].e) HIPCHK(r, hipStreamWaitEvent(s, packed[i].e, 0));
            const ProbBufs& b = c->slab_prob;
            HIPCHK(r, sm_copy(stage + at[i].ids, r->device, b.ids.p, c->device, k * 4, s));
            HIPCHK(r, sm_copy(stage + at[i].cls, r->device, b.cls.p, c->device, k, s));
            HIPCHK(r, sm_copy(stage + at[i].mass, r->device, b.mass.p, c->device, k * 4, s));
            HIPCHK(r, sm_copy(stage + at[i].level, r->device, b.level.p, c->device, k * 4, s));
            HIPCHK(r, sm_copy(stage + at[i].pos, r->device, b.pos.p, c->device, k * 8, s));
            HIPCHK(r, sm_copy(stage + at[i].h2, r->device, b.h2.p, c->device, k * 4, s));
            HIPCHK(r, sm_copy(stage + at[i].off, r->device, b.off.p, c->device, (ko + 1) * 4, s));
            HIPCHK(r, sm_copy(stage + at[i].idx, r->device, c->cand_idx.p, c->device, t * 4, s));
        }
    }
    return slab_merge_staged(r, (int)root, what, part, (const uint32_t*)stage, n_global, K_out, tot_out);
}

// THE MERGE, once for both forms: the local problems `part` (every pointer in the root's memory, queued behind whatever staged them on
// r's stream) -> the merged problem in r's prob / prob_idx; *K_out / *tot_out: its participants and entries.  ids_side_by_side: the
// members' ids in one array in member order (the group form's staging: ONE mark launch reads them all), or nullptr: the ids sit inside
// each member's blob and the mark kernel is launched once per blob (the relay's staging) -- equal stores to the same flags either way.
int slab_merge_staged(sph_ctx* r, int root, const char* what, const std::vector<SmPart>& part, const uint32_t* ids_side_by_side, uint32_t n_global, uint32_t* K_out,
                      uint32_t* tot_out)
{
    const size_t nm = part.size();
    hipStream_t s = r->stream;
    *K_out = *tot_out = 0;
    uint64_t sum_k = 0, sum_t = 0;
    for (size_t i = 0; i < nm; i++) {
        sum_k += part[i].K;
        sum_t += part[i].T;
    }
    if (sum_k == 0) return SPH_OK;
    HIPCHK(r, r->ss_flag.ensure((size_t)n_global * 4 + 4));
    HIPCHK(r, r->ss_rank.ensure(((size_t)n_global + 1) * 4));
    HIPCHK(r, r->ss_err.ensure(16));
    HIPCHK(r, r->cand_scan.ensure(((size_t)std::max<uint64_t>(n_global, sum_k) / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
    uint32_t* flag = r->ss_flag.as<uint32_t>();
    uint32_t* rank = r->ss_rank.as<uint32_t>();
    uint32_t* err = r->ss_err.as<uint32_t>();
    const dim3 blk(256);
    uint32_t K = 0, e = 0;
    {
        ProfScope ps(&r->prof, "slab_search_mark", s);
        HIPCHK(r, hipMemsetAsync(flag, 0, (size_t)n_global * 4, s));
        HIPCHK(r, hipMemsetAsync(err, 0, 16, s));
        if (ids_side_by_side)
            hipLaunchKernelGGL(k_slab_merge_mark, dim3((uint32_t)((sum_k + 255) / 256)), blk, 0, s, (uint32_t)sum_k, ids_side_by_side, n_global, flag, err);
        else
            for (size_t i = 0; i < nm; i++)
                if (part[i].K) hipLaunchKernelGGL(k_slab_merge_mark, dim3((part[i].K + 255) / 256), blk, 0, s, part[i].K, part[i].ids, n_global, flag, err);
        device_exclusive_scan_u32(s, flag, rank, n_global, r->cand_scan.as<uint32_t>(), rank + n_global);
    }
    HIPCHK(r, hipMemcpyAsync(&K, rank + n_global, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(r, hipMemcpyAsync(&e, err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(r, hipStreamSynchronize(s));
    if (!e && (K == 0 || K > n_global || K > sum_k)) e = SM_ERR_ID;
    if (e) return r->fail(SPH_ERR_DEVICE, "%s: %s (merge on rank %d, %llu local participants)", what, sm_error_text(e), root, (unsigned long long)sum_k);
    ProbOut out;
    if (int rc = prob_out(r, r->prob, K, K, &out)) return rc;
    HIPCHK(r, r->ss_seen.ensure((size_t)K + 4));
    HIPCHK(r, r->ss_rowlen.ensure((size_t)K * 4 + 4));
    uint8_t* seen = r->ss_seen.as<uint8_t>();
    uint32_t* rowlen = r->ss_rowlen.as<uint32_t>();
    uint32_t tot_c = 0;
    {
        ProfScope ps(&r->prof, "slab_search_fields", s);
        HIPCHK(r, hipMemsetAsync(seen, 0, K, s));
        HIPCHK(r, hipMemsetAsync(rowlen, 0, (size_t)K * 4, s));
        hipLaunchKernelGGL(k_slab_merge_ids, dim3((n_global + 255) / 256), blk, 0, s, n_global, K, (const uint32_t*)flag, (const uint32_t*)rank, out.ids);
        for (size_t i = 0; i < nm; i++)
            if (part[i].K)
                hipLaunchKernelGGL(k_slab_merge_fields, dim3((part[i].K + 255) / 256), blk, 0, s, part[i], n_global, K, (const uint32_t*)flag, (const uint32_t*)rank, out, seen,
                                   rowlen, err);
        device_exclusive_scan_u32(s, rowlen, out.off, K, r->cand_scan.as<uint32_t>(), out.off + K);
    }
    HIPCHK(r, hipMemcpyAsync(&tot_c, out.off + K, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(r, hipMemcpyAsync(&e, err, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(r, hipStreamSynchronize(s));
    if (!e && tot_c != sum_t) e = SM_ERR_ROWS;
    if (e) return r->fail(SPH_ERR_DEVICE, "%s: %s (merge on rank %d, K=%u)", what, sm_error_text(e), root, K);
    HIPCHK(r, r->prob_idx.ensure((size_t)tot_c * 4 + 4));
    if (tot_c) {
        ProfScope ps(&r->prof, "slab_search_rows", s);
        for (size_t i = 0; i < nm; i++)
            if (part[i].Ko && part[i].T)
                hipLaunchKernelGGL(k_slab_merge_rows, dim3((part[i].Ko + 255) / 256), blk, 0, s, part[i], n_global, K, tot_c, (const uint32_t*)flag, (const uint32_t*)rank,
                                   (const uint32_t*)out.off, r->prob_idx.as<uint32_t>(), err);
        HIPCHK(r, hipMemcpyAsync(&e, err, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(r, hipStreamSynchronize(s));
        if (e) return r->fail(SPH_ERR_DEVICE, "%s: %s (merge on rank %d, K=%u)", what, sm_error_text(e), root, K);
    }
    *K_out = K;
    *tot_out = tot_c;
    return SPH_OK;
}

extern "C" int sph_group_find_partners_device(sph_ctx** ctxs, int n, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t wide_threshold, int root,
                                              sph_partner_search_info* info, uint64_t* n_participants, uint64_t* n_owned_participants, uint64_t* n_indices)
{
    const char* what = "sph_group_find_partners_device";
    if (info) *info = sph_partner_search_info{};
    for (int i = 0; ctxs && i < n; i++) {
        if (n_participants) n_participants[i] = 0;
        if (n_owned_participants) n_owned_participants[i] = 0;
        if (n_indices) n_indices[i] = 0;
    }
    Group G;
    if (int rc = slab_search_entry(G, ctxs, n, what)) return rc;
    for (auto c : G.m) c->slab_sol_serial = 0;   // (this call replaces the open solution, or closes it)
    sph_ctx* c0 = ctxs[0];
    if (!p || !ap || !info) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: params, ap and info must be given", what);
    if (int rc = cand_check_args(c0, what, kind, p, ap)) return rc;
    if (root < 0 || root >= n) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: root %d is no member of the %d contexts", what, root, n);
    const size_t nm = (size_t)n;
    std::vector<uint64_t> K(nm, 0), Ko(nm, 0), T(nm, 0);
    bool together = false;
    if (int rc = slab_prob_prepare(G, kind, p, ap, K.data(), Ko.data(), T.data(), &together)) return rc;
    uint64_t sum_t = 0, n_global = 0;
    for (size_t i = 0; i < nm; i++) {
        if (n_participants) n_participants[i] = K[i];
        if (n_owned_participants) n_owned_participants[i] = Ko[i];
        if (n_indices) n_indices[i] = T[i];
        sum_t += T[i];
        n_global += G.m[i]->n;
    }
    if (sum_t >= (1ull << 32)) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: %llu candidates do not fit the 32-bit offsets of the search", what, (unsigned long long)sum_t);
    if (n_global >= 0xfffffff0ull) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: %llu particles", what, (unsigned long long)n_global);
    sph_ctx* r = G.m[(size_t)root];
    uint32_t Km = 0, tot = 0;
    if (int rc = slab_merge_on_root(G, (size_t)root, what, K.data(), Ko.data(), T.data(), (uint32_t)n_global, &Km, &tot)) return rc;
    HIPCHK(r, hipSetDevice(r->device));
    if (Km) {
        PsOutcome o;
        if (int rc = ps_solve(r, kind, p, ap, wide_threshold, Km, tot, info, &o)) return rc;
        if (o.error) return r->fail(SPH_ERR_DEVICE, "%s: %s (K=%u, %u donors undecided after %u rounds)", what, ps_error_text(o.error), Km, o.undecided, o.rounds);
        // ---- hand-over: the K decisions and ids to every member's device, on the root's stream; the members' streams wait for them
        for (auto c : G.m) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, c->slab_sol_ids.ensure((size_t)Km * 4));
            HIPCHK(c, c->slab_sol_partner.ensure((size_t)Km * 4));
            HIPCHK(c, c->slab_sol_counter.ensure((size_t)Km * 2));
        }
        HIPCHK(r, hipSetDevice(r->device));
        SmEvent handed;
        HIPCHK(r, handed.create());
        {
            ProfScope ps(&r->prof, "slab_search_handover", r->stream);
            for (auto c : G.m) {
                HIPCHK(r, sm_copy(c->slab_sol_ids.p, c->device, r->prob.ids.p, r->device, (size_t)Km * 4, r->stream));
                HIPCHK(r, sm_copy(c->slab_sol_partner.p, c->device, r->sol_partner.p, r->device, (size_t)Km * 4, r->stream));
                HIPCHK(r, sm_copy(c->slab_sol_counter.p, c->device, r->sol_counter.p, r->device, (size_t)Km * 2, r->stream));
            }
        }
        HIPCHK(r, hipEventRecord(handed.e, r->stream));
        for (auto c : G.m)
            if (c != r) HIPCHK(c, hipStreamWaitEvent(c->stream, handed.e, 0));
    }
    for (auto c : G.m) {
        c->slab_sol_k = Km;
        c->slab_sol_tot = tot;
        c->slab_sol_kind = kind;
        c->slab_sol_root = root;
        c->slab_sol_serial = c->slab_prob_serial;
    }
    return SPH_OK;
}

// the solution is open on every member, and it is one solution
static int slab_need_solution(Group& G, const char* what)
{
    sph_ctx* c0 = G.m[0];
    for (auto c : G.m)
        if (!slab_solution_open(c) || c->slab_sol_k != c0->slab_sol_k || c->slab_sol_kind != c0->slab_sol_kind || c->slab_sol_root != c0->slab_sol_root)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution on rank %d (sph_group_find_partners_device comes first; a step, an upload, an edit, a merge, a split, a later prepare or sph_group_adapt_device closes it)", what, c->dist.rank);
    if (c0->slab_sol_root < 0 || (size_t)c0->slab_sol_root >= G.m.size()) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution", what);
    return SPH_OK;
}

extern "C" int sph_group_download_merged_partner_problem(sph_ctx** ctxs, int n, uint32_t* ids, uint8_t* size_class, float* mass, float* level, float* position, float* h2,
                                                         uint32_t* offsets, uint64_t pcap, uint32_t* indices, uint64_t icap, uint64_t* n_participants, uint64_t* n_indices)
{
    const char* what = "sph_group_download_merged_partner_problem";
    if (n_participants) *n_participants = 0;
    if (n_indices) *n_indices = 0;
    Group G;
    if (int rc = slab_search_entry(G, ctxs, n, what)) return rc;
    if (int rc = slab_need_solution(G, what)) return rc;
    sph_ctx* r = G.m[(size_t)G.m[0]->slab_sol_root];
    const size_t K = r->slab_sol_k;
    const uint64_t tot = r->slab_sol_tot;
    if (n_participants) *n_participants = K;
    if (n_indices) *n_indices = tot;
    if ((ids || size_class || mass || level || position || h2 || offsets) && pcap < K)
        return r->fail(SPH_ERR_INVALID_ARGUMENT, "%s: participant buffers too small (%llu participants)", what, (unsigned long long)K);
    if (indices && icap < tot) return r->fail(SPH_ERR_INVALID_ARGUMENT, "%s: indices buffer too small (%llu entries)", what, (unsigned long long)tot);
    HIPCHK(r, hipSetDevice(r->device));
    return prob_download(r, r->prob, K, K, tot, r->prob_idx.p, ids, size_class, mass, level, position, h2, offsets, indices);
}

extern "C" int sph_group_download_partner_decisions(sph_ctx** ctxs, int n, int from_member, uint64_t k, uint32_t* ids, uint32_t* partner_c, uint16_t* counter_c)
{
    const char* what = "sph_group_download_partner_decisions";
    Group G;
    if (int rc = slab_search_entry(G, ctxs, n, what)) return rc;
    if (from_member < 0 || from_member >= n) return ctxs[0]->fail(SPH_ERR_INVALID_ARGUMENT, "%s: member %d of %d contexts", what, from_member, n);
    if (int rc = slab_need_solution(G, what)) return rc;
    sph_ctx* c = G.m[(size_t)from_member];
    if (k != c->slab_sol_k) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: k=%llu, the open solution has %u participants", what, (unsigned long long)k, c->slab_sol_k);
    if (k == 0) return SPH_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (ids) HIPCHK(c, hipMemcpyAsync(ids, c->slab_sol_ids.p, (size_t)k * 4, hipMemcpyDeviceToHost, s));
    if (partner_c) HIPCHK(c, hipMemcpyAsync(partner_c, c->slab_sol_partner.p, (size_t)k * 4, hipMemcpyDeviceToHost, s));
    if (counter_c) HIPCHK(c, hipMemcpyAsync(counter_c, c->slab_sol_counter.p, (size_t)k * 2, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

extern "C" int sph_group_adapt_device(sph_ctx** ctxs, int n, int op, const sph_params* p, const sph_adapt_params* ap)
{
    const char* what = "sph_group_adapt_device";
    Group G;
    if (int rc = slab_search_entry(G, ctxs, n, what)) return rc;
    sph_ctx* c0 = ctxs[0];
    if (!p || !ap) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: params and ap must be given", what);
    if (op != 0 && op != 1) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: op %d is neither 0 (share) nor 1 (merge)", what, op);
    if (int rc = slab_need_solution(G, what)) return rc;
    if (c0->slab_sol_kind != op) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "%s: the open solution is of kind %d", what, c0->slab_sol_kind);
    const uint64_t k = c0->slab_sol_k;
    for (auto c : G.m) c->slab_sol_serial = 0;   // consumed (a share leaves the prepared rows open, the solution not)
    return slab_adapt_device(G, op, p, ap, k);
}
