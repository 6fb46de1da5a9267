// The candidate rows on the device and the plumbing of the partner problems made from them, shared by sph_candidates.hip (which hands
// the rows to the host as they are), sph_partner_problem.hip (which renumbers their participants), sph_partner_search.hip and the slab
// forms of the first two: one definition of the tests, of the row walk, of the packed arrays and of the way decisions come back.
#pragma once

#include <vector>

#include "sph_context.hpp"
#include "sph_partner_search.h"   // sph_partner_search_info

struct CandP {
    int share;             // kind == 0
    uint32_t donor_class;  // Large (3) when sharing, TooSmall (0) when merging
    float max_dist_factor;
    int allow_optimal;     // allow_{share,merge}_with_optimal_particle
    int allow_too_small;   // allow_share_with_too_small_particle
    int allow_size_diff;   // allow_merge_on_size_difference
};
CandP cand_params(int kind, const sph_adapt_params* ap);
// what every entry point that takes a search's `kind` and parameters refuses first: SPH_ERR_INVALID_ARGUMENT
int cand_check_args(sph_ctx* c, const char* what, int kind, const sph_params* p, const sph_adapt_params* ap);

// particle_sharing.rs:50-67 / particle_merging.rs:57-78 for the pair (i, j): true = j stays in row i.  rec / cls: the {x, y, mass, h2}
// records and class bytes in the index space of j (host order in sph_candidates.hip, slots in sph_slab_candidates.hip).
__device__ __forceinline__ bool cand_pass(const CandP& q, const float4 Ai, uint32_t j, const float4* __restrict__ rec, const uint8_t* __restrict__ cls)
{
    const uint32_t cj = cls[j];
    bool can;
    if (q.share) can = cj == 1u || (cj == 0u && q.allow_too_small) || (cj == 2u && q.allow_optimal);
    else can = cj == 1u || cj == 0u || (cj == 2u && q.allow_optimal);
    if (!can && !(!q.share && q.allow_size_diff)) return false;   // (the record is read only where a test needs it)
    const float4 Aj = rec[j];
    if (!can && !(Aj.z > __fmul_rn(5.f, Ai.z))) return false;
    const float dx = __fsub_rn(Ai.x, Aj.x), dy = __fsub_rn(Ai.y, Aj.y);
    const float max_dist = __fmul_rn(__fmul_rn(__fadd_rn(Ai.w, Aj.w), 0.5f), q.max_dist_factor);
    return !(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) > __fmul_rn(max_dist, max_dist));
}

// The walk of ONE donor's row r of the step's lists (off / idx, `tot` entries in all; the entries live in [0, n): host indices or
// slots): the row ends at min(off[r + 1], tot), the donor itself (`self`) and an entry outside the index space are skipped, and
// survivor(j) is called, in list order, for every j that passes cand_pass against the donor's record Ai.  Counting, filling and
// marking differ only in what they do with a survivor.
template <class F>
__device__ __forceinline__ void cand_walk_row(const CandP& q, uint32_t r, uint32_t self, uint32_t n, const float4 Ai, const uint32_t* __restrict__ off,
                                              const uint32_t* __restrict__ idx, uint64_t tot, const float4* __restrict__ rec, const uint8_t* __restrict__ cls,
                                              F&& survivor)
{
    const uint64_t e = min((uint64_t)off[r + 1], tot);
    for (uint64_t p = off[r]; p < e; p++) {
        const uint32_t j = idx[p];
        if (j == self || j >= n) continue;
        if (cand_pass(q, Ai, j, rec, cls)) survivor(j);
    }
}

// poisoned -> SPH_ERR_POISONED, a slab context -> SPH_ERR_UNSUPPORTED
int cand_refuse_common(sph_ctx* c, const char* what);
// the CSR of the last step's lists on the device (export_valid), built here if neither export has built it yet
int cand_need_lists(sph_ctx* c);
// n > 0, lists present.  gather + count + scan: cand_rec / cand_cls in host order, cand_off[n + 1]; *tot = the candidates' total
// (one 4-byte copy; the offsets travel with it when offsets_host is given).  Synchronises the stream.
int cand_count_rows(sph_ctx* c, const CandP& q, uint32_t* offsets_host, uint32_t* tot);
// tot > 0, after cand_count_rows with the same q: the rows' entries into cand_idx[tot].  Queues the launch, does not wait.
int cand_fill_rows(sph_ctx* c, const CandP& q, uint32_t tot);
// the f64 sum of pm[pcur][0 .. n).z over the slots whose `owned` byte is set (nullptr: all of them), k_sum_mass's fixed-order tree.
// Synchronises the stream.
int cand_sum_mass(sph_ctx* c, uint32_t n, const uint8_t* owned, double* total);

// ---- sph_partner_problem.hip: the compact problem's plumbing, for the plain and the slab problem alike --------------------------------
// what a pack kernel writes through: the arrays of a ProbBufs (sph_context.hpp)
struct ProbOut {
    uint32_t* ids;
    uint8_t* cls;
    float* mass;
    float* level;
    float2* pos;
    float* h2;
    uint32_t* off;
};
// room for K participants and n_off + 1 offsets in b; *o: its arrays
int prob_out(sph_ctx* c, ProbBufs& b, size_t K, size_t n_off, ProbOut* o);
// the download of a packed problem: whatever host pointer was given is filled -- K entries each, n_off + 1 offsets, the `tot` entries of
// d_indices -- and the stream is synchronised; K == 0: offsets[0] = 0 and no copy
int prob_download(sph_ctx* c, const ProbBufs& b, size_t K, size_t n_off, uint64_t tot, const void* d_indices, uint32_t* ids, uint8_t* size_class, float* mass,
                  float* level, float* position, float* h2, uint32_t* offsets, uint32_t* indices);
// the host check of K compact decisions, before anything is launched (a bad id must not leave some receivers and donors already modified):
// a partner is a compact id < K or one of the two sentinels; ids (may be null: the problem's own, on the device) strictly ascending
int prob_check_decisions(sph_ctx* c, const char* what, uint64_t K, const uint32_t* ids, const uint32_t* partner_c);
// K decisions in compact ids -> merge_partner / merge_counter of the WHOLE vector (n entries) in d_partner / d_counter: AVAILABLE / 0
// everywhere, then one thread per compact id scatters its pair, the partner mapped through ids (k_prob_expand).  ids / partner_c /
// counter_c are device arrays, except where ExpandStage names a buffer: then that one is the host's and is staged there first.  `scope`:
// the ProfScope all of it runs in.  Queued on the context's stream.
struct ExpandStage {
    DevBuf *ids, *partner_c, *counter_c;
};
int prob_expand(sph_ctx* c, const char* scope, uint32_t n, uint32_t K, const uint32_t* ids, const uint32_t* partner_c, const uint16_t* counter_c, uint32_t* d_partner,
                uint16_t* d_counter, ExpandStage stage = {nullptr, nullptr, nullptr});
// prob_build_on_device: the compact problem of `kind` into prob .. prob_idx without a bulk copy (lists present: cand_need_lists came
// first); `caps` (may be null): the host buffers a download was given.
struct ProbCaps {
    bool participants_given;
    uint64_t participants;
    bool indices_given;
    uint64_t indices;
};
int prob_build_on_device(sph_ctx* c, int kind, const sph_adapt_params* ap, const char* what, const ProbCaps* caps, uint32_t* K, uint32_t* tot);
// the problem just built becomes THE OPEN PROBLEM of the context
void prob_open_problem(sph_ctx* c, int kind, uint32_t K);
// the open problem is consumed: its prob_k decisions -- the host's (on_host: staged here) or the open solution's on the device -- are
// expanded over the vector and applied (transfer_on_device).  What sph_*_particles_compact and sph_*_particles_device share.
int prob_apply(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, int merging, const uint32_t* partner_c, const uint16_t* counter_c, bool on_host);

// sph_slab_candidates.hip, shared with sph_slab_partner_problem.hip.  slab_cand_refuse: a plain context -> SPH_ERR_UNSUPPORTED, a poisoned
// one -> SPH_ERR_POISONED.  slab_cand_prepare: the collective prepare of sph_slab_candidates.h for the members of G; *together: as
// rank_entry (sph_dist.hpp) reads it.  slab_cand_mark_launch: the walk of the rows prepared last once more, setting flag[slot] (owned
// slots) / flag[n_tot + slot] (ghost slots) of every donor with a candidate and every candidate.
struct Group;
int slab_cand_refuse(sph_ctx* c, const char* what);
int slab_cand_prepare(Group& G, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_rows, uint64_t* n_indices, bool* together);
void slab_cand_mark_launch(sph_ctx* c, const CandP& q, uint32_t* flag);

// sph_partner_search.hip, shared with sph_slab_partner_search.hip: the exact-schedule search on the compact problem that sits in c's
// prob.off[K + 1] / prob_idx[tot] / prob.mass / prob.level / prob.cls (K > 0), on c's stream and work arrays -- the writers CSR, first,
// the resident and wide rounds, validate.  The decisions land in c->sol_partner / c->sol_counter.  A HIP failure is the return value;
// what the search itself found wrong (ps_error_text) is out->error, with SPH_OK returned.  *info is filled when neither happened.
struct PsOutcome {
    uint32_t error, undecided, rounds;
};
int ps_solve(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t wide_threshold, uint32_t K, uint32_t tot, sph_partner_search_info* info,
             PsOutcome* out);
const char* ps_error_text(uint32_t e);
// sph_slab_partner_problem.hip: the collective prepare of sph_slab_partner_problem.h for the members of G (the three arrays: one entry per member)
int slab_prob_prepare(Group& G, int kind, const sph_params* p, const sph_adapt_params* ap, uint64_t* n_part, uint64_t* n_owned, uint64_t* n_indices, bool* together);
// sph_adapt.hip: slab_adapt (op 0 share, 1 merge) from the k decisions every member holds on its own device (slab_sol_ids /
// slab_sol_partner / slab_sol_counter): the device form of SlabCompact
int slab_adapt_device(Group& G, int op, const sph_params* p, const sph_adapt_params* ap, uint64_t k);

// sph_slab_partner_search.hip, shared with sph_rank_partner_search.hip: one member's local problem as it is STAGED in the root's memory,
// and the merge of the staged problems -- the one merge of both forms; what differs is how the arrays got there (peer copies in the
// group form, a relay over the ranks' transport in the per-process form).  slab_merge_staged: see its definition.
struct SmPart {
    const uint32_t* ids;   // [K] owned participants first
    const uint8_t* cls;
    const float* mass;
    const float* level;
    const float2* pos;
    const float* h2;
    const uint32_t* off;   // [Ko + 1]
    const uint32_t* idx;   // [T] global ids
    uint32_t K, Ko, T;
};
int slab_merge_staged(sph_ctx* r, int root, const char* what, const std::vector<SmPart>& part, const uint32_t* ids_side_by_side, uint32_t n_global, uint32_t* K_out,
                      uint32_t* tot_out);
// THE OPEN SOLUTION is open on c (the lifetime rule of sph_slab_partner_search.h)
inline bool slab_solution_open(const sph_ctx* c)
{
    return c->slab_prob_open && c->slab_rows_open && c->slab_lists_valid && c->slab_sol_serial != 0 && c->slab_sol_serial == c->slab_prob_serial;
}
