// include/sph_rank_partner_search.h: the partner searches on the device with ONE PROCESS PER RANK.  Everything that decides is reused
// unchanged -- the prepare of sph_slab_partner_problem.hip, the merge of sph_slab_partner_search.hip (slab_merge_staged: the one merge of
// both forms), ps_solve of sph_partner_search.hip, slab_adapt_device of sph_adapt.hip, the open solution's fields and lifetime.  What is
// added here is the STAGING in front of the merge and the hand-over behind the solve, for ranks that reach each other only through their
// transport's exchange:
//
//   table      allreduce_sum_u32 of a zeroed row, five words per rank (K, Ko, T, particles, message limit / 16), each rank filling its own
//   blob       k_rank_prob_blob: ONE launch copies the eight packed arrays into one message, every piece at a multiple of 16 bytes, in
//              the order of slab_merge_on_root's Place for one member -- ids, the five fields, offsets, entries -- straight into the
//              rank's place of the gather buffer (ss_stage).  16-byte loads and stores where the source is aligned, byte stores otherwise
//              and for a piece's tail; the padding is zeroed.  It replaces eight copies per hop
//   gather     relay_gather (sph_relay.hip).  The root does not unpack: the SmPart pointers of the merge point into the blobs.  The ids
//              are the first piece of every blob, not side by side: k_slab_merge_mark is launched ONCE PER BLOB (slab_merge_staged)
//   header     256 bytes from the root to every rank: the info struct, K, the entries' total, the root's status and the text of its
//              error.  A merge or solver failure on the root thereby ends the call on every rank with the root's status and text
//   decisions  the same kernel packs ids[K], partner_c[K], counter_c[K] behind the header; relay_bcast; three aligned copies on every rank
//              into slab_sol_ids / slab_sol_partner / slab_sol_counter
//
// Every index the blob kernel forms lies inside a piece whose size the host computed from the counts the prepare returned; the merge
// checks what the blobs CONTAIN, as it does in the group form.  Collective rule: rank_entry (sph_dist.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sph_rank_partner_search.h"
#include "sph_candidates.hpp"
#include "sph_dist.hpp"

enum { RS_TABLE_WORDS = 5, RS_MAX_RANKS = SHM_MAX_U32 / RS_TABLE_WORDS, RS_PIECES = 8 };
static const uint64_t RS_UNLIMITED_CHUNK = 1ull << 30;   // the message size where the transport sets none

// `bytes` bytes from src to blob + dst, the rest of the last 16 bytes zeroed
struct RsPiece {
    const uint8_t* src;
    uint64_t dst, bytes;
};
struct RsJob {
    RsPiece p[RS_PIECES];
};

__global__ __launch_bounds__(256) void k_rank_prob_blob(RsJob j, uint8_t* __restrict__ blob)
{
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, nth = (uint64_t)gridDim.x * 256;
    for (int q = 0; q < RS_PIECES; q++) {
        const RsPiece P = j.p[q];
        if (!P.bytes) continue;
        const uint64_t padded = (P.bytes + 15) & ~(uint64_t)15;
        uint8_t* d = blob + P.dst;   // (a multiple of 16 in a 16-byte aligned buffer)
        uint64_t done = 0;
        if (((uintptr_t)P.src & 15u) == 0) {
            const uint64_t full = P.bytes / 16;
            for (uint64_t g = tid; g < full; g += nth) ((uint4*)d)[g] = ((const uint4*)P.src)[g];
            done = full * 16;
        }
        for (uint64_t b = done + tid; b < padded; b += nth) d[b] = b < P.bytes ? P.src[b] : (uint8_t)0;
    }
}

// where the pieces of one rank's blob sit (slab_merge_on_root's Place for one member, the ids in front)
struct RsPlace {
    uint64_t ids, cls, mass, level, pos, h2, off, idx, bytes;
};
static RsPlace rs_place(uint64_t K, uint64_t Ko, uint64_t T)
{
    RsPlace a{};
    if (!K) return a;
    uint64_t b = 0;
    auto take = [&](uint64_t n) {
        const uint64_t at = b;
        b += (n + 15) & ~(uint64_t)15;
        return at;
    };
    a.ids = take(K * 4);
    a.cls = take(K);
    a.mass = take(K * 4);
    a.level = take(K * 4);
    a.pos = take(K * 8);
    a.h2 = take(K * 4);
    a.off = take((Ko + 1) * 4);
    a.idx = take(T * 4);
    a.bytes = b;
    return a;
}
static uint64_t rs_decisions_bytes(uint64_t K) { return 2 * ((K * 4 + 15) & ~(uint64_t)15) + ((K * 2 + 15) & ~(uint64_t)15); }

static void rs_launch_blob(sph_ctx* c, const char* scope, const RsJob& j, uint8_t* blob)
{
    uint64_t most = 0;
    for (const RsPiece& p : j.p) most = std::max(most, p.bytes);
    ProfScope ps(&c->prof, scope, c->stream);
    hipLaunchKernelGGL(k_rank_prob_blob, dim3((uint32_t)std::min<uint64_t>(1024, std::max<uint64_t>(1, (most / 16 + 255) / 256))), dim3(256), 0, c->stream, j, blob);
}

struct RsHeader {
    sph_partner_search_info info;
    uint32_t K, tot;
    int32_t status;
    uint32_t reserved;
    char text[192];
};
static_assert(sizeof(RsHeader) == 256, "the broadcast header is 256 bytes");

// a slab context that has no transport of its own is a member of a loopback group
static bool rs_loopback_member(const sph_ctx* c) { return !c->dist.tgroup && !c->dist.shm && !c->dist.ipc && !c->dist.nccl; }

// what every entry point of this header refuses first
static int rs_entry(sph_ctx* c, const char* what, const char* plain_takes, const char* group_takes)
{
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s: not a slab context (a plain context takes %s)", what, plain_takes);
    if (c->poisoned) return c->refuse_poisoned();
    if (rs_loopback_member(c)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: a slab context of a loopback group takes %s", what, group_takes);
    return SPH_OK;
}

static int rs_find(Group& G, bool* together, const char* what, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t wide_threshold, int root,
                   uint64_t relay_bytes, sph_partner_search_info* info, uint64_t* Kl, uint64_t* Kol, uint64_t* Tl)
{
    sph_ctx* c = G.m[0];
    const int n = c->dist.nranks, rank = c->dist.rank;
    if (int rc = slab_prob_prepare(G, kind, p, ap, Kl, Kol, Tl, together)) return rc;
    // ---- the table: every rank's counts and message limit, the same on every rank
    const uint64_t limit = std::min<uint64_t>(G.comm->max_message_bytes(G), RS_UNLIMITED_CHUNK);
    uint64_t chunk = (relay_bytes ? std::min<uint64_t>(relay_bytes, limit) : limit) & ~(uint64_t)15;
    std::vector<std::vector<uint32_t>> rows(1, std::vector<uint32_t>((size_t)n * RS_TABLE_WORDS, 0u));
    {
        uint32_t* mine = &rows[0][(size_t)rank * RS_TABLE_WORDS];
        mine[0] = (uint32_t)*Kl;
        mine[1] = (uint32_t)*Kol;
        mine[2] = (uint32_t)*Tl;
        mine[3] = (uint32_t)c->n;
        mine[4] = (uint32_t)(chunk / 16);
    }
    if (int rc = G.comm->allreduce_sum_u32(G, rows)) return rc;
    const uint32_t* tab = rows[0].data();
    uint64_t sum_k = 0, sum_t = 0, n_global = 0;
    std::vector<uint64_t> bytes((size_t)n, 0), base((size_t)n + 1, 0);
    for (int o = 0; o < n; o++) {
        const uint32_t* w = tab + (size_t)o * RS_TABLE_WORDS;
        sum_k += w[0];
        sum_t += w[2];
        n_global += w[3];
        chunk = std::min<uint64_t>(chunk, (uint64_t)w[4] * 16);   // (a launch gives every rank the same limit; the smallest one holds if not)
        bytes[(size_t)o] = rs_place(w[0], w[1], w[2]).bytes;
        base[(size_t)o + 1] = base[(size_t)o] + bytes[(size_t)o];
    }
    // (refusals out of the table: every rank takes them alike)
    *together = true;
    if (sum_t >= (1ull << 32)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: %llu candidates do not fit the 32-bit offsets of the search", what, (unsigned long long)sum_t);
    if (n_global >= 0xfffffff0ull) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: %llu particles", what, (unsigned long long)n_global);
    if (chunk < 16) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: a rank's transport takes no message", what);
    *together = false;
    c->rs_blob_bytes = bytes;
    c->rs_chunk = chunk;
    c->rs_header_bytes = c->rs_dec_bytes = c->rs_sent = c->rs_received = 0;
    uint32_t Km = 0, tot = 0;
    if (sum_k) {
        hipStream_t s = c->stream;
        // ---- blob: this rank's local problem at its place among the ranks' blobs
        HIPCHK(c, c->ss_stage.ensure((size_t)base[(size_t)n] + 16));
        HIPCHK(c, c->rs_bcast.ensure(sizeof(RsHeader) + (size_t)rs_decisions_bytes(sum_k) + 16));
        uint8_t* stage = c->ss_stage.as<uint8_t>();
        if (*Kl) {
            const RsPlace at = rs_place(*Kl, *Kol, *Tl);
            const ProbBufs& b = c->slab_prob;
            const uint64_t k = *Kl;
            const RsJob j{{{(const uint8_t*)b.ids.p, at.ids, k * 4},
                           {(const uint8_t*)b.cls.p, at.cls, k},
                           {(const uint8_t*)b.mass.p, at.mass, k * 4},
                           {(const uint8_t*)b.level.p, at.level, k * 4},
                           {(const uint8_t*)b.pos.p, at.pos, k * 8},
                           {(const uint8_t*)b.h2.p, at.h2, k * 4},
                           {(const uint8_t*)b.off.p, at.off, (*Kol + 1) * 4},
                           {(const uint8_t*)c->cand_idx.p, at.idx, *Tl * 4}}};
            rs_launch_blob(c, "rank_search_blob", j, stage + base[(size_t)rank]);
        }
        // ---- gather
        if (int rc = relay_gather(G, root, bytes, chunk, stage, &c->rs_sent, &c->rs_received)) return rc;
        // ---- merge and solve on the root; whatever they answer travels in the header
        RsHeader h{};
        uint8_t* bc = c->rs_bcast.as<uint8_t>();
        if (rank == root) {
            std::vector<SmPart> part((size_t)n);
            for (int o = 0; o < n; o++) {
                const uint32_t* w = tab + (size_t)o * RS_TABLE_WORDS;
                const RsPlace at = rs_place(w[0], w[1], w[2]);
                const uint8_t* q = stage + base[(size_t)o];
                part[(size_t)o] = SmPart{(const uint32_t*)(q + at.ids), q + at.cls, (const float*)(q + at.mass), (const float*)(q + at.level), (const float2*)(q + at.pos),
                                         (const float*)(q + at.h2), (const uint32_t*)(q + at.off), (const uint32_t*)(q + at.idx), w[0], w[1], w[2]};
            }
            int rrc = slab_merge_staged(c, root, what, part, nullptr, (uint32_t)n_global, &Km, &tot);
            if (!rrc) {
                PsOutcome o{};
                rrc = ps_solve(c, kind, p, ap, wide_threshold, Km, tot, &h.info, &o);
                if (!rrc && o.error)
                    rrc = c->fail(SPH_ERR_DEVICE, "%s: %s (K=%u, %u donors undecided after %u rounds)", what, ps_error_text(o.error), Km, o.undecided, o.rounds);
            }
            h.K = Km;
            h.tot = tot;
            h.status = rrc;
            if (rrc) {
                h.info = sph_partner_search_info{};
                strncpy(h.text, c->err.c_str(), sizeof h.text - 1);
            }
            HIPCHK(c, hipMemcpyAsync(bc, &h, sizeof h, hipMemcpyHostToDevice, s));
            HIPCHK(c, hipStreamSynchronize(s));   // (h is this frame's)
        }
        if (int rc = relay_bcast(G, root, sizeof(RsHeader), chunk, bc, &c->rs_sent, &c->rs_received)) return rc;
        if (rank != root) {
            HIPCHK(c, hipMemcpyAsync(&h, bc, sizeof h, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            h.text[sizeof h.text - 1] = 0;
        }
        c->rs_header_bytes = sizeof(RsHeader);
        if (h.status) {   // (the root's failure, on every rank: out of a collective)
            *together = true;
            return c->fail(h.status, "%s", h.text);
        }
        Km = h.K;
        tot = h.tot;
        if (Km == 0 || Km > sum_k) return c->fail(SPH_ERR_DEVICE, "%s: the root announces %u participants of %llu reported", what, Km, (unsigned long long)sum_k);
        // ---- the decisions: packed behind the header on the root, relayed, copied into the open solution's arrays
        const uint64_t w4 = ((uint64_t)Km * 4 + 15) & ~(uint64_t)15, dec = rs_decisions_bytes(Km);
        uint8_t* pay = bc + sizeof(RsHeader);
        if (rank == root) {
            RsJob j{};
            j.p[0] = RsPiece{(const uint8_t*)c->prob.ids.p, 0, (uint64_t)Km * 4};
            j.p[1] = RsPiece{(const uint8_t*)c->sol_partner.p, w4, (uint64_t)Km * 4};
            j.p[2] = RsPiece{(const uint8_t*)c->sol_counter.p, 2 * w4, (uint64_t)Km * 2};
            rs_launch_blob(c, "rank_search_decisions", j, pay);
        }
        if (int rc = relay_bcast(G, root, dec, chunk, pay, &c->rs_sent, &c->rs_received)) return rc;
        c->rs_dec_bytes = dec;
        HIPCHK(c, c->slab_sol_ids.ensure((size_t)Km * 4));
        HIPCHK(c, c->slab_sol_partner.ensure((size_t)Km * 4));
        HIPCHK(c, c->slab_sol_counter.ensure((size_t)Km * 2));
        {
            ProfScope ps(&c->prof, "rank_search_handover", s);
            HIPCHK(c, hipMemcpyAsync(c->slab_sol_ids.p, pay, (size_t)Km * 4, hipMemcpyDeviceToDevice, s));
            HIPCHK(c, hipMemcpyAsync(c->slab_sol_partner.p, pay + w4, (size_t)Km * 4, hipMemcpyDeviceToDevice, s));
            HIPCHK(c, hipMemcpyAsync(c->slab_sol_counter.p, pay + 2 * w4, (size_t)Km * 2, hipMemcpyDeviceToDevice, s));
        }
        *info = h.info;
    }
    c->slab_sol_k = Km;
    c->slab_sol_tot = tot;
    c->slab_sol_kind = kind;
    c->slab_sol_root = root;
    c->slab_sol_serial = c->slab_prob_serial;
    return SPH_OK;
}

extern "C" int sph_slab_find_partners_device(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t wide_threshold, int root, uint64_t relay_bytes,
                                             sph_partner_search_info* info, uint64_t* n_participants, uint64_t* n_owned_participants, uint64_t* n_indices)
{
    const char* what = "sph_slab_find_partners_device";
    if (info) *info = sph_partner_search_info{};
    if (n_participants) *n_participants = 0;
    if (n_owned_participants) *n_owned_participants = 0;
    if (n_indices) *n_indices = 0;
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = rs_entry(c, what, "sph_find_partners_device", "sph_group_find_partners_device")) return rc;
    c->slab_sol_serial = 0;   // (this call replaces the open solution, or closes it)
    // (argument refusals are every rank's alike -- the ranks make the same call -- and come before any collective)
    if (!p || !ap || !info) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: params, ap and info must be given", what);
    if (int rc = cand_check_args(c, what, kind, p, ap)) return rc;
    if (root < 0 || root >= c->dist.nranks) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: root %d is no rank of the %d", what, root, c->dist.nranks);
    if (relay_bytes && relay_bytes < 4096) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: relay_bytes %llu (0: the transport's limit; otherwise 4096 or more)", what, (unsigned long long)relay_bytes);
    if (c->dist.nranks > RS_MAX_RANKS) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: %d ranks (the size table takes %d)", what, c->dist.nranks, (int)RS_MAX_RANKS);
    uint64_t K = 0, Ko = 0, T = 0;
    const int rc = rank_entry(c, "sph_group_find_partners_device", [&](Group& G, bool* together) -> int {
        return rs_find(G, together, what, kind, p, ap, wide_threshold, root, relay_bytes, info, &K, &Ko, &T);
    });
    if (n_participants) *n_participants = K;
    if (n_owned_participants) *n_owned_participants = Ko;
    if (n_indices) *n_indices = T;
    if (rc) *info = sph_partner_search_info{};
    return rc;
}

extern "C" int sph_slab_adapt_device(sph_ctx* c, int op, const sph_params* p, const sph_adapt_params* ap)
{
    const char* what = "sph_slab_adapt_device";
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = rs_entry(c, what, "sph_share_particles_device / sph_merge_particles_device", "sph_group_adapt_device")) return rc;
    if (!p || !ap) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: params and ap must be given", what);
    if (op != 0 && op != 1) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: op %d is neither 0 (share) nor 1 (merge)", what, op);
    return rank_entry(c, "sph_group_adapt_device", [&](Group& G, bool* together) -> int {
        // one rank's solution may have been closed behind the others' backs (an upload on that rank): the ranks agree before any of them
        // enters the apply, so that all of them refuse
        std::vector<int> missing(1, !slab_solution_open(c) || c->slab_sol_kind != op ? 1 : 0);
        if (int rc = G.comm->allreduce_max_i32(G, missing)) return rc;
        if (missing[0]) {   // (a refusal leaves what is open open, as the group form's does)
            *together = true;
            if (slab_solution_open(c) && c->slab_sol_kind != op) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: the open solution is of kind %d", what, c->slab_sol_kind);
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution on every rank (sph_slab_find_partners_device comes first; a step, an upload, an edit, a merge, a split, a later prepare or sph_slab_adapt_device closes it)", what);
        }
        const uint64_t k = c->slab_sol_k;
        c->slab_sol_serial = 0;   // consumed, whatever the apply returns (a share leaves the prepared rows open, the solution not)
        return slab_adapt_device(G, op, p, ap, k);
    });
}

extern "C" int sph_slab_download_partner_decisions(sph_ctx* c, uint64_t k, uint32_t* ids, uint32_t* partner_c, uint16_t* counter_c)
{
    const char* what = "sph_slab_download_partner_decisions";
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = rs_entry(c, what, "sph_download_partner_decisions", "sph_group_download_partner_decisions")) return rc;
    if (!slab_solution_open(c)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution", what);
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

extern "C" int sph_slab_download_merged_partner_problem(sph_ctx* c, uint32_t* ids, uint8_t* size_class, float* mass, float* level, float* position, float* h2,
                                                        uint32_t* offsets, uint64_t pcap, uint32_t* indices, uint64_t icap, uint64_t* n_participants, uint64_t* n_indices)
{
    const char* what = "sph_slab_download_merged_partner_problem";
    if (n_participants) *n_participants = 0;
    if (n_indices) *n_indices = 0;
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = rs_entry(c, what, "sph_download_partner_problem", "sph_group_download_merged_partner_problem")) return rc;
    if (!slab_solution_open(c)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution", what);
    if (c->slab_sol_root != c->dist.rank) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: the merged problem sits on rank %d, this is rank %d", what, c->slab_sol_root, c->dist.rank);
    const size_t K = c->slab_sol_k;
    const uint64_t tot = c->slab_sol_tot;
    if (n_participants) *n_participants = K;
    if (n_indices) *n_indices = tot;
    if ((ids || size_class || mass || level || position || h2 || offsets) && pcap < K)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: participant buffers too small (%llu participants)", what, (unsigned long long)K);
    if (indices && icap < tot) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: indices buffer too small (%llu entries)", what, (unsigned long long)tot);
    HIPCHK(c, hipSetDevice(c->device));
    return prob_download(c, c->prob, K, K, tot, c->prob_idx.p, ids, size_class, mass, level, position, h2, offsets, indices);
}

extern "C" int sph_slab_relay_sizes(sph_ctx* c, uint64_t* bytes_of_rank, uint64_t capacity, uint64_t* n_ranks, uint64_t* chunk_bytes, uint64_t* header_bytes,
                                    uint64_t* decisions_bytes, uint64_t* bytes_sent, uint64_t* bytes_received)
{
    const char* what = "sph_slab_relay_sizes";
    if (n_ranks) *n_ranks = 0;
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = rs_entry(c, what, "sph_find_partners_device, which relays nothing", "sph_group_find_partners_device, which stages by copies")) return rc;
    if (!slab_solution_open(c)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution", what);
    const size_t n = c->rs_blob_bytes.size();
    if (n_ranks) *n_ranks = n;
    if (chunk_bytes) *chunk_bytes = c->rs_chunk;
    if (header_bytes) *header_bytes = c->rs_header_bytes;
    if (decisions_bytes) *decisions_bytes = c->rs_dec_bytes;
    if (bytes_sent) *bytes_sent = c->rs_sent;
    if (bytes_received) *bytes_received = c->rs_received;
    if (bytes_of_rank) {
        if (capacity < n) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: room for %llu of %zu ranks", what, (unsigned long long)capacity, n);
        std::copy(c->rs_blob_bytes.begin(), c->rs_blob_bytes.end(), bytes_of_rank);
    }
    return SPH_OK;
}
