// include/sph_partner_search.h: the partner searches' sequential loop on the device, in its exact parallel schedule (DESIGN.md 10.3;
// numpy twin: adaptivity.find_partners_frontier).  Everything below works on the COMPACT problem of sph_partner_problem.hip: K
// participants, rows off[K + 1] / idx[tot] in compact ids, the fields mass / level / cls per participant.
//
//   writers CSR  writers(x) = the donors d with x in touch(d) = row(d) + {d}, ascending.  count (non-returning atomics, thread per donor
//                row) -> device_exclusive_scan_u32 -> fill (one returning atomic per entry) -> sort (thread per x, insertion sort: rows are
//                a few tens of entries; the sort removes the fill's nondeterminism).  tot + donors entries.
//   first        thread per donor: the donors that are ready before anything is decided (the only pass over all donors)
//   a round      four phases over index lists, each a __device__ function per item:
//       decide   a ready donor runs its row as the loop does; what it claims goes to the CLAIMED list
//       collect  a claimed particle puts its undecided writers on the RECHECK list; a claimed donor retires and puts the unclaimed
//                particles of its touch set on the DIRTY list; a finished donor does the same with what it left unclaimed
//       walk     one thread per dirty x moves head(x) past finished / retired writers; the new head goes on the RECHECK list
//       check    a recheck donor that is undecided and ready goes on the next FRONTIER
//     Both dedupe lists (dirty, recheck) through a stamp word per particle: atomicExch(stamp, round) != round appends.
//
// Two drivers call the same four functions.  RESIDENT (k_ps_resident): ONE workgroup loops over the rounds inside one launch, phases
// separated by a workgroup-scope fence and a workgroup barrier; the lists' first entries live in LDS, the rest spills to the global
// arrays the wide driver uses.  Frontiers are a handful of donors for tens to thousands of rounds (profiles/r11_device_search.md), so a
// round costs its dependent loads and four barriers, not six launches.  There is no barrier, flag or wait between workgroups anywhere.
// WIDE (k_ps_w_*): the same phases as grid launches for a round whose frontier has reached the wide threshold; appends are
// wave-aggregated (one returning atomic per wave), rounds are queued in batches, a batch's kernels leave at once when the frontier is
// empty or small again, and the host reads the 16-byte progress record once per batch.
//
// Every loop is bounded: a round decides at least one donor, the resident loop runs at most `donors` rounds, and a round that finds
// nobody ready while donors remain sets the error word and leaves -- nothing waits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sph_candidates.hpp"
#include "sph_partner_search.h"
#include "sph_target_mass.hpp"

#define PS_AVAILABLE SPH_MERGE_PARTNER_AVAILABLE
#define PS_DELETE SPH_MERGE_PARTNER_DELETE
enum : uint8_t { PS_UNDECIDED = 0, PS_FINISHED = 1, PS_RETIRED = 2 };
enum : uint32_t { PS_ERR_STUCK = 1, PS_ERR_COUNTER = 2, PS_ERR_OVERFLOW = 3, PS_ERR_VALIDATE = 4 };

static const uint32_t PS_DEFAULT_WIDE_THRESHOLD = 256;    // profiles/r11_device_search.md: beyond it six launches cost less than one workgroup's walk
static const int PS_WIDE_BATCH = 8;                       // wide rounds queued between two reads of the progress record
// LDS heads of the resident driver's lists (entries beyond them live in the global arrays)
#define PS_LDS_FRONTIER 512
#define PS_LDS_CLAIMED 1024
#define PS_LDS_DIRTY 2048
#define PS_LDS_RECHECK 2048

// the progress record (first 16 bytes: what the host reads per batch) and the counters of the wide driver
struct PsRec {
    uint32_t remaining;   // undecided donors
    uint32_t n_frontier;  // donors of the current frontier
    uint32_t rounds;
    uint32_t error;
    uint32_t max_frontier, wide_rounds, parity, stop;
    uint32_t n_claimed, n_dirty, n_recheck, n_next, n_retired, donors_with_row, pad0, pad1;
    unsigned long long donors, transfers;
};

struct PsP {
    uint32_t K;
    const uint32_t* off;    // [K + 1]
    const uint32_t* idx;    // [tot]
    uint32_t tot;
    const uint32_t* woff;   // [K + 1] writers CSR
    const uint32_t* w;      // [wtot]
    uint32_t* hp;           // [K] position of head(x) in w
    uint8_t* state;         // [K]
    uint32_t* partner;      // [K]
    uint16_t* counter;      // [K]
    const float* mass;
    const float* level;
    uint32_t* stamp_x;      // [K] dirty dedupe
    uint32_t* stamp_d;      // [K] recheck dedupe
    int share;
    float max_transfer, dt, mass_base;
    TargetP tp;
};

// An index list: entry k in LDS while k < cap, else in the global array (at k: the wide driver, cap == 0, sees a plain array).
struct PsList {
    uint32_t* lds;
    uint32_t cap;
    uint32_t* glob;
    uint32_t limit;   // entries the global array holds (K)
    uint32_t* count;
    __device__ __forceinline__ uint32_t get(uint32_t k) const { return k < cap ? lds[k] : glob[k]; }
};

// Append from divergent code: the lanes that are active here take consecutive places behind ONE returning atomic of their leader.
__device__ __forceinline__ void ps_push(const PsList& l, uint32_t v, uint32_t* err)
{
    const unsigned long long m = __ballot(1);
    const uint32_t lane = threadIdx.x & 63u;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(l.count, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    const uint32_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (k < l.cap) l.lds[k] = v;
    else if (k < l.limit) l.glob[k] = v;
    else *err = PS_ERR_OVERFLOW;
}

__device__ __forceinline__ bool ps_has_row(const PsP& P, uint32_t i) { return P.off[i + 1] > P.off[i]; }

// READY: every x of touch(i) is claimed, or i is the head of its writers
__device__ bool ps_ready(const PsP& P, uint32_t i)
{
    if (P.partner[i] != PS_AVAILABLE) return false;   // (claimed: it retires, it never runs)
    const uint32_t b = P.off[i], e = min(P.off[i + 1], P.tot);
    for (uint32_t q = b; q <= e; q++) {               // q == e: i itself
        const uint32_t x = q < e ? P.idx[q] : i;
        if (x >= P.K || P.partner[x] != PS_AVAILABLE) continue;
        const uint32_t h = P.hp[x];
        if (h >= P.woff[x + 1] || P.w[h] != i) return false;
    }
    return true;
}

// find_share_partner_sequential / find_merge_partner_sequential for donor i (sph_host_find_partners, sph_adapt.hip: the same f32
// expressions in the same order; the class and distance tests were passed when the row was built)
__device__ void ps_decide(const PsP& P, uint32_t i, const PsList& claimed, uint32_t* err)
{
    const float mi = P.mass[i];
    float dropped;
    if (P.share) {
        const float target = target_mass(P.level[i], P.tp);
        dropped = fminf(mi - target, target * P.max_transfer * P.dt);
    } else dropped = mi;
    uint32_t cnt = 0;
    const uint32_t b = P.off[i], e = min(P.off[i + 1], P.tot);
    for (uint32_t q = b; q < e; q++) {
        const uint32_t j = P.idx[q];
        if (j == i || j >= P.K) continue;
        if (P.partner[j] != PS_AVAILABLE) continue;   // the neighbour is somebody's partner already
        const float new_mass_j = P.mass[j] + dropped / (float)(cnt + 1u);
        const float target_j = target_mass(P.level[j], P.tp);
        if (new_mass_j >= target_j * 1.1f /* PARTICLE_SIZE_FACTOR_LARGE */) continue;
        if (new_mass_j > P.mass_base) continue;
        if (cnt == 0) P.partner[i] = PS_DELETE;       // (available: a ready donor is unclaimed)
        P.partner[j] = i;
        cnt++;
        ps_push(claimed, j, err);
        if (!(cnt < 1000u)) {                         // assert!(merge_counter[i] < 1000)
            *err = PS_ERR_COUNTER;
            break;
        }
    }
    P.counter[i] = (uint16_t)cnt;
    P.state[i] = PS_FINISHED;
}

__device__ __forceinline__ void ps_mark_dirty(const PsP& P, uint32_t x, uint32_t round, const PsList& dirty, uint32_t* err)
{
    if (x >= P.K || P.partner[x] != PS_AVAILABLE) return;   // (a claimed particle blocks nobody: its head is of no interest)
    if (atomicExch(&P.stamp_x[x], round) != round) ps_push(dirty, x, err);
}

// every unclaimed x of touch(d) gets a new head
__device__ void ps_dirty_touch(const PsP& P, uint32_t d, uint32_t round, const PsList& dirty, uint32_t* err)
{
    const uint32_t b = P.off[d], e = min(P.off[d + 1], P.tot);
    for (uint32_t q = b; q <= e; q++) ps_mark_dirty(P, q < e ? P.idx[q] : d, round, dirty, err);
}

// particle j was claimed in this round: its writers are checked again; if it is an undecided donor, it retires
__device__ void ps_collect_claimed(const PsP& P, uint32_t j, uint32_t round, const PsList& dirty, const PsList& recheck, uint32_t* n_retired, uint32_t* err)
{
    for (uint32_t q = P.woff[j], e = P.woff[j + 1]; q < e; q++) {
        const uint32_t d = P.w[q];
        if (d >= P.K || d == j || P.state[d] != PS_UNDECIDED) continue;
        if (atomicExch(&P.stamp_d[d], round) != round) ps_push(recheck, d, err);
    }
    if (ps_has_row(P, j) && P.state[j] == PS_UNDECIDED) {
        P.state[j] = PS_RETIRED;
        atomicAdd(n_retired, 1u);
        ps_dirty_touch(P, j, round, dirty, err);
    }
}

// head(x) moves past finished and retired writers; the new head is checked again
__device__ void ps_walk(const PsP& P, uint32_t x, uint32_t round, const PsList& recheck, uint32_t* err)
{
    if (P.partner[x] != PS_AVAILABLE) return;
    uint32_t h = P.hp[x];
    const uint32_t e = P.woff[x + 1];
    while (h < e && P.state[P.w[h]] != PS_UNDECIDED) h++;
    P.hp[x] = h;
    if (h < e) {
        const uint32_t d = P.w[h];
        if (atomicExch(&P.stamp_d[d], round) != round) ps_push(recheck, d, err);
    }
}

__device__ __forceinline__ void ps_check(const PsP& P, uint32_t d, const PsList& next, uint32_t* err)
{
    if (P.state[d] == PS_UNDECIDED && ps_ready(P, d)) ps_push(next, d, err);
}

// ---- writers CSR ---------------------------------------------------------------------------------------------------------------
// FILL = false: cnt[x] += 1 for every x of touch(d).  FILL = true: d into x's row at a place taken from cur[x].
template <bool FILL>
__global__ __launch_bounds__(256) void k_ps_writers(uint32_t K, const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx, uint32_t tot,
                                                     uint32_t* __restrict__ cnt, const uint32_t* __restrict__ woff, uint32_t* __restrict__ w)
{
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d >= K) return;
    const uint32_t b = off[d], e = min(off[d + 1], tot);
    if (b >= e) return;
    for (uint32_t q = b; q <= e; q++) {
        const uint32_t x = q < e ? idx[q] : d;
        if (x >= K || (q < e && x == d)) continue;   // (d itself is entered once, by q == e)
        if (FILL) {
            const uint32_t at = woff[x] + atomicAdd(&cnt[x], 1u);
            if (at < woff[x + 1]) w[at] = d;
        } else atomicAdd(&cnt[x], 1u);
    }
}

__global__ __launch_bounds__(256) void k_ps_sort(uint32_t K, const uint32_t* __restrict__ woff, uint32_t* __restrict__ w, uint32_t* __restrict__ hp)
{
    const uint32_t x = blockIdx.x * 256 + threadIdx.x;
    if (x >= K) return;
    const uint32_t b = woff[x], e = woff[x + 1];
    hp[x] = b;
    for (uint32_t q = b + 1; q < e; q++) {
        const uint32_t v = w[q];
        uint32_t r = q;
        while (r > b && w[r - 1] > v) {
            w[r] = w[r - 1];
            r--;
        }
        w[r] = v;
    }
}

// the donors that are ready before anything is decided -> frontier 0; the number of donors that have a row -> remaining
__global__ __launch_bounds__(256) void k_ps_first(PsP P, PsList fr, PsRec* __restrict__ rec)
{
    const uint32_t d = blockIdx.x * 256 + threadIdx.x;
    if (d >= P.K || !ps_has_row(P, d)) return;
    const unsigned long long m = __ballot(1);
    if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) {
        atomicAdd(&rec->remaining, (uint32_t)__popcll(m));
        atomicAdd(&rec->donors_with_row, (uint32_t)__popcll(m));
    }
    if (ps_ready(P, d)) ps_push(fr, d, &rec->error);
}

// ---- the resident driver: one workgroup, every round inside this launch ------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_ps_resident(PsP P, uint32_t* __restrict__ lists, PsRec* __restrict__ rec, uint32_t wide_threshold)
{
    __shared__ uint32_t s_fr[2][PS_LDS_FRONTIER], s_claimed[PS_LDS_CLAIMED], s_dirty[PS_LDS_DIRTY], s_recheck[PS_LDS_RECHECK];
    __shared__ uint32_t s_n[8];   // 0/1: frontier counts by parity, 2 claimed, 3 dirty, 4 recheck, 5 retired, 6 error
    const uint32_t tid = threadIdx.x, nt = blockDim.x, K = P.K;
    uint32_t par = rec->parity, remaining = rec->remaining, rounds = rec->rounds, max_frontier = rec->max_frontier;
    const uint32_t bound = remaining;   // a round decides at least one donor
    if (tid < 8) s_n[tid] = 0;
    __syncthreads();
    const uint32_t nf0 = min(rec->n_frontier, K);
    if (tid == 0) s_n[par] = nf0;
    for (uint32_t k = tid; k < min(nf0, (uint32_t)PS_LDS_FRONTIER); k += nt) s_fr[par][k] = lists[(size_t)par * K + k];
    __syncthreads();
    PsList fr[2] = {{s_fr[0], PS_LDS_FRONTIER, lists, K, &s_n[0]}, {s_fr[1], PS_LDS_FRONTIER, lists + K, K, &s_n[1]}};
    const PsList claimed{s_claimed, PS_LDS_CLAIMED, lists + 2 * (size_t)K, K, &s_n[2]};
    const PsList dirty{s_dirty, PS_LDS_DIRTY, lists + 3 * (size_t)K, K, &s_n[3]};
    const PsList recheck{s_recheck, PS_LDS_RECHECK, lists + 4 * (size_t)K, K, &s_n[4]};
    uint32_t* const err = &s_n[6];
    uint32_t nf = s_n[par];
    for (uint32_t it = 0; it < bound && nf != 0 && nf < wide_threshold && *err == 0; it++) {
        rounds++;
        max_frontier = max(max_frontier, nf);
        // decide
        for (uint32_t k = tid; k < nf; k += nt) ps_decide(P, fr[par].get(k), claimed, err);
        __threadfence_block();
        __syncthreads();
        // collect: the claimed particles, then the finished donors
        const uint32_t nc = min(s_n[2], K);
        for (uint32_t k = tid; k < nc + nf; k += nt) {
            if (k < nc) ps_collect_claimed(P, claimed.get(k), rounds, dirty, recheck, &s_n[5], err);
            else ps_dirty_touch(P, fr[par].get(k - nc), rounds, dirty, err);
        }
        __threadfence_block();
        __syncthreads();
        // walk
        const uint32_t nd = min(s_n[3], K);
        for (uint32_t k = tid; k < nd; k += nt) ps_walk(P, dirty.get(k), rounds, recheck, err);
        __threadfence_block();
        __syncthreads();
        // check
        const uint32_t nr = min(s_n[4], K);
        for (uint32_t k = tid; k < nr; k += nt) ps_check(P, recheck.get(k), fr[par ^ 1], err);
        __threadfence_block();
        __syncthreads();
        const uint32_t gone = nf + s_n[5];
        remaining = remaining > gone ? remaining - gone : 0u;
        nf = min(s_n[par ^ 1], K);
        __syncthreads();   // (everybody has read the counts)
        if (tid == 0) s_n[par] = s_n[2] = s_n[3] = s_n[4] = s_n[5] = 0;
        par ^= 1;
        __syncthreads();
    }
    // hand over: the frontier's LDS head to the global array, the record
    for (uint32_t k = tid; k < min(nf, (uint32_t)PS_LDS_FRONTIER); k += nt) lists[(size_t)par * K + k] = s_fr[par][k];
    if (tid == 0) {
        uint32_t e = *err;
        if (!e && nf == 0 && remaining != 0) e = PS_ERR_STUCK;   // nobody is ready and donors remain: an error, not a wait
        rec->remaining = remaining;
        rec->n_frontier = nf;
        rec->rounds = rounds;
        rec->max_frontier = max_frontier;
        rec->parity = par;
        rec->stop = 0;
        if (e) rec->error = e;
    }
}

// ---- the wide driver: one round = begin, decide, collect, walk, check, end ---------------------------------------------------------
// (the current frontier's count is n_frontier and the next one's n_next, whichever parity holds their entries: k_ps_w_end moves n_next over)
struct PsWide {
    uint32_t* lists;   // [5 K]: frontier 0, frontier 1, claimed, dirty, recheck
    PsRec* rec;
    uint32_t K;
};
__device__ __forceinline__ PsList ps_wlist(const PsWide& W, uint32_t which, uint32_t* count) { return PsList{nullptr, 0, W.lists + (size_t)which * W.K, W.K, count}; }

__global__ void k_ps_w_begin(PsRec* __restrict__ rec, uint32_t wide_threshold)
{
    if (rec->stop) return;
    const uint32_t nf = rec->n_frontier;
    if (rec->error || nf == 0 || nf < wide_threshold) {
        rec->stop = 1;
        return;
    }
    rec->rounds++;
    rec->wide_rounds++;
    rec->max_frontier = max(rec->max_frontier, nf);
    rec->n_claimed = rec->n_dirty = rec->n_recheck = rec->n_next = rec->n_retired = 0;
}
__global__ __launch_bounds__(256) void k_ps_w_decide(PsP P, PsWide W)
{
    PsRec* rec = W.rec;
    if (rec->stop) return;
    const uint32_t nf = min(rec->n_frontier, P.K), par = rec->parity;
    const PsList fr = ps_wlist(W, par, &rec->n_frontier), claimed = ps_wlist(W, 2, &rec->n_claimed);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < nf; k += gridDim.x * 256) ps_decide(P, fr.get(k), claimed, &rec->error);
}
__global__ __launch_bounds__(256) void k_ps_w_collect(PsP P, PsWide W)
{
    PsRec* rec = W.rec;
    if (rec->stop) return;
    const uint32_t nf = min(rec->n_frontier, P.K), nc = min(rec->n_claimed, P.K), par = rec->parity, round = rec->rounds;
    const PsList fr = ps_wlist(W, par, &rec->n_frontier), claimed = ps_wlist(W, 2, &rec->n_claimed), dirty = ps_wlist(W, 3, &rec->n_dirty),
                 recheck = ps_wlist(W, 4, &rec->n_recheck);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < nc + nf; k += gridDim.x * 256) {
        if (k < nc) ps_collect_claimed(P, claimed.get(k), round, dirty, recheck, &rec->n_retired, &rec->error);
        else ps_dirty_touch(P, fr.get(k - nc), round, dirty, &rec->error);
    }
}
__global__ __launch_bounds__(256) void k_ps_w_walk(PsP P, PsWide W)
{
    PsRec* rec = W.rec;
    if (rec->stop) return;
    const uint32_t nd = min(rec->n_dirty, P.K), round = rec->rounds;
    const PsList dirty = ps_wlist(W, 3, &rec->n_dirty), recheck = ps_wlist(W, 4, &rec->n_recheck);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < nd; k += gridDim.x * 256) ps_walk(P, dirty.get(k), round, recheck, &rec->error);
}
__global__ __launch_bounds__(256) void k_ps_w_check(PsP P, PsWide W)
{
    PsRec* rec = W.rec;
    if (rec->stop) return;
    const uint32_t nr = min(rec->n_recheck, P.K), par = rec->parity;
    const PsList recheck = ps_wlist(W, 4, &rec->n_recheck), next = ps_wlist(W, par ^ 1u, &rec->n_next);
    for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < nr; k += gridDim.x * 256) ps_check(P, recheck.get(k), next, &rec->error);
}
__global__ void k_ps_w_end(PsRec* __restrict__ rec, uint32_t K)
{
    if (rec->stop) return;
    const uint32_t gone = rec->n_frontier + rec->n_retired;
    rec->remaining = rec->remaining > gone ? rec->remaining - gone : 0u;
    rec->n_frontier = min(rec->n_next, K);
    rec->parity ^= 1u;
    if (rec->n_frontier == 0 && rec->remaining != 0 && !rec->error) rec->error = PS_ERR_STUCK;
}

// ---- validate_share_partners / validate_merge_partners on the compact arrays, and the two sums ------------------------------------------
__global__ __launch_bounds__(256) void k_ps_validate(PsP P, const uint8_t* __restrict__ cls, uint32_t donor_class, PsRec* __restrict__ rec)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    uint32_t cnt = 0;
    bool bad = false;
    if (c < P.K) {
        cnt = P.counter[c];
        const uint32_t pc = P.partner[c];
        if (cnt > 0) {
            bad = cls[c] != donor_class || pc != PS_DELETE;
            uint32_t c2 = 0;
            for (uint32_t q = P.off[c], e = min(P.off[c + 1], P.tot); q < e; q++) {
                const uint32_t j = P.idx[q];
                c2 += (j < P.K && P.partner[j] == c) ? 1u : 0u;
            }
            bad = bad || c2 != cnt;
        } else {
            bad = pc == PS_DELETE;
            if (pc != PS_AVAILABLE && pc != PS_DELETE) bad = pc >= P.K || P.partner[pc] != PS_DELETE;
        }
        if (ps_has_row(P, c) && P.state[c] == PS_UNDECIDED) bad = true;   // every donor finished or retired
    }
    if (bad) rec->error = PS_ERR_VALIDATE;
    uint32_t t = cnt, d = cnt > 0 ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) {
        t += __shfl_down(t, o);
        d += __shfl_down(d, o);
    }
    if ((threadIdx.x & 63u) == 0 && t) {
        atomicAdd(&rec->transfers, (unsigned long long)t);
        atomicAdd(&rec->donors, (unsigned long long)d);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static bool solution_open(sph_ctx* c)
{
    return c->prob_open && c->sol_serial == c->prob_serial;
}

const char* ps_error_text(uint32_t e)
{
    switch (e) {
    case PS_ERR_STUCK: return "no donor is ready while donors remain";
    case PS_ERR_COUNTER: return "a merge counter reached 1000";
    case PS_ERR_OVERFLOW: return "a round list overflowed";
    case PS_ERR_VALIDATE: return "the decisions fail validate_share_partners / validate_merge_partners";
    }
    return "unknown error";
}

// The search on the compact problem in c's prob / prob_idx buffers (sph_candidates.hpp: ps_solve), for sph_find_partners_device on its own
// context and for sph_group_find_partners_device on the root of a slab group.
int ps_solve(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t wide_threshold, uint32_t K, uint32_t tot, sph_partner_search_info* info,
             PsOutcome* out)
{
    *out = PsOutcome{0, 0, 0};
    hipStream_t s = c->stream;
    if (wide_threshold == 0) wide_threshold = PS_DEFAULT_WIDE_THRESHOLD;
    const size_t k = K, wtot = (size_t)tot + k;   // a writers entry per candidate entry and one per donor
    // words: woff[K + 1], cnt[K], hp[K], stamp_x[K], stamp_d[K], lists[5 K]
    HIPCHK(c, c->sol_partner.ensure(k * 4));
    HIPCHK(c, c->sol_counter.ensure(k * 2));
    HIPCHK(c, c->ps_w.ensure(wtot * 4));
    HIPCHK(c, c->ps_words.ensure((10 * k + 4) * 4));
    HIPCHK(c, c->ps_state.ensure(k));
    HIPCHK(c, c->ps_rec.ensure(sizeof(PsRec)));
    HIPCHK(c, c->cand_scan.ensure((k / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
    uint32_t* words = c->ps_words.as<uint32_t>();
    uint32_t *woff = words, *cnt = woff + k + 1, *hp = cnt + k, *stamp_x = hp + k, *stamp_d = stamp_x + k, *lists = stamp_d + k;
    PsRec* rec = c->ps_rec.as<PsRec>();
    PsP P{};
    P.K = K;
    P.off = c->prob.off.as<uint32_t>();
    P.idx = c->prob_idx.as<uint32_t>();
    P.tot = tot;
    P.woff = woff;
    P.w = c->ps_w.as<uint32_t>();
    P.hp = hp;
    P.state = c->ps_state.as<uint8_t>();
    P.partner = c->sol_partner.as<uint32_t>();
    P.counter = c->sol_counter.as<uint16_t>();
    P.mass = c->prob.mass.as<float>();
    P.level = c->prob.level.as<float>();
    P.stamp_x = stamp_x;
    P.stamp_d = stamp_d;
    P.share = kind == 0;
    P.max_transfer = ap->max_mass_transfer_sharing;
    P.dt = ap->dt;
    P.mass_base = (SPH_PI_F * p->particle_radius_base * p->particle_radius_base) * p->rest_density;   // SimulationParams::mass_base
    P.tp = target_params(p);
    const dim3 gk((K + 255) / 256), blk(256);
    {
        ProfScope ps(&c->prof, "search_writers", s);
        HIPCHK(c, hipMemsetAsync(P.partner, 0xff, k * 4, s));   // SPH_MERGE_PARTNER_AVAILABLE
        HIPCHK(c, hipMemsetAsync(P.counter, 0, k * 2, s));
        HIPCHK(c, hipMemsetAsync(P.state, 0, k, s));
        HIPCHK(c, hipMemsetAsync(cnt, 0, 4 * k * 4, s));        // cnt, hp, stamp_x, stamp_d
        HIPCHK(c, hipMemsetAsync(rec, 0, sizeof(PsRec), s));
        hipLaunchKernelGGL(k_ps_writers<false>, gk, blk, 0, s, K, P.off, P.idx, tot, cnt, (const uint32_t*)nullptr, (uint32_t*)nullptr);
        device_exclusive_scan_u32(s, cnt, woff, K, c->cand_scan.as<uint32_t>(), woff + K);
        HIPCHK(c, hipMemsetAsync(cnt, 0, k * 4, s));
        hipLaunchKernelGGL(k_ps_writers<true>, gk, blk, 0, s, K, P.off, P.idx, tot, cnt, (const uint32_t*)woff, c->ps_w.as<uint32_t>());
        hipLaunchKernelGGL(k_ps_sort, gk, blk, 0, s, K, (const uint32_t*)woff, c->ps_w.as<uint32_t>(), hp);
        hipLaunchKernelGGL(k_ps_first, gk, blk, 0, s, P, PsList{nullptr, 0, lists, K, &rec->n_frontier}, rec);
    }
    const PsWide W{lists, rec, K};
    const dim3 gw(std::min((K + 255) / 256, 1024u));
    uint32_t prog[4] = {0, 0, 0, 0};   // remaining, n_frontier, rounds, error
    {
        ProfScope ps(&c->prof, "search_rounds", s);
        // Every launch of the resident kernel and every wide batch decides at least one donor or ends the search (an empty frontier, an
        // error): at most K + 2 of them.  The host reads the 16-byte record once per resident launch and once per wide batch.
        bool wide = false;
        for (uint64_t turn = 0; turn < (uint64_t)K + 2; turn++) {
            if (!wide) hipLaunchKernelGGL(k_ps_resident, dim3(1), dim3(c->opt.search_block), 0, s, P, lists, rec, wide_threshold);
            else
                for (int b = 0; b < PS_WIDE_BATCH; b++) {
                    hipLaunchKernelGGL(k_ps_w_begin, dim3(1), dim3(1), 0, s, rec, wide_threshold);
                    hipLaunchKernelGGL(k_ps_w_decide, gw, blk, 0, s, P, W);
                    hipLaunchKernelGGL(k_ps_w_collect, gw, blk, 0, s, P, W);
                    hipLaunchKernelGGL(k_ps_w_walk, gw, blk, 0, s, P, W);
                    hipLaunchKernelGGL(k_ps_w_check, gw, blk, 0, s, P, W);
                    hipLaunchKernelGGL(k_ps_w_end, dim3(1), dim3(1), 0, s, rec, K);
                }
            HIPCHK(c, hipMemcpyAsync(prog, rec, sizeof prog, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (prog[3] || prog[1] == 0) break;
            wide = prog[1] >= wide_threshold;
        }
    }
    if (!prog[3] && (prog[1] != 0 || prog[0] != 0)) prog[3] = PS_ERR_STUCK;
    PsRec r{};
    if (!prog[3]) {
        ProfScope ps(&c->prof, "search_validate", s);
        hipLaunchKernelGGL(k_ps_validate, gk, blk, 0, s, P, (const uint8_t*)c->prob.cls.as<uint8_t>(), kind == 0 ? 3u : 0u, rec);
        HIPCHK(c, hipMemcpyAsync(&r, rec, sizeof r, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        prog[3] = r.error;
    }
    *out = PsOutcome{prog[3], prog[0], prog[2]};
    if (prog[3]) return SPH_OK;
    info->participants = K;
    info->candidates = tot;
    info->donors = r.donors;
    info->transfers = r.transfers;
    info->rounds = r.rounds;
    info->max_frontier = r.max_frontier;
    info->wide_rounds = r.wide_rounds;
    return SPH_OK;
}

extern "C" int sph_find_partners_device(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t wide_threshold, sph_partner_search_info* info)
{
    const char* what = "sph_find_partners_device";
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (info) *info = sph_partner_search_info{};
    c->prob_open = false;   // (this call replaces the open problem, or closes it)
    if (!p || !ap || !info) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: params, ap and info must be given", what);
    if (int rc = cand_check_args(c, what, kind, p, ap)) return rc;
    if (int rc = cand_refuse_common(c, what)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = cand_need_lists(c)) return rc;
    uint32_t K = 0, tot = 0;
    if (int rc = prob_build_on_device(c, kind, ap, what, nullptr, &K, &tot)) return rc;
    if (K == 0) {
        prob_open_problem(c, kind, 0);
        c->sol_serial = c->prob_serial;
        return SPH_OK;
    }
    PsOutcome o;
    if (int rc = ps_solve(c, kind, p, ap, wide_threshold, K, tot, info, &o)) return rc;
    prob_open_problem(c, kind, K);   // (the problem itself is sound: the host may still solve it)
    if (o.error) return c->fail(SPH_ERR_DEVICE, "%s: %s (K=%u, %u donors undecided after %u rounds)", what, ps_error_text(o.error), K, o.undecided, o.rounds);
    c->sol_serial = c->prob_serial;
    return SPH_OK;
}

extern "C" int sph_download_partner_decisions(sph_ctx* c, uint64_t k, uint32_t* ids, uint32_t* partner_c, uint16_t* counter_c)
{
    const char* what = "sph_download_partner_decisions";
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = cand_refuse_common(c, what)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!solution_open(c)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution (sph_find_partners_device comes first)", what);
    if (k != c->prob_k) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: k=%llu, the open solution has %u participants", what, (unsigned long long)k, c->prob_k);
    if (k == 0) return SPH_OK;
    hipStream_t s = c->stream;
    if (partner_c) HIPCHK(c, hipMemcpyAsync(partner_c, c->sol_partner.p, (size_t)k * 4, hipMemcpyDeviceToHost, s));
    if (counter_c) HIPCHK(c, hipMemcpyAsync(counter_c, c->sol_counter.p, (size_t)k * 2, hipMemcpyDeviceToHost, s));
    return prob_download(c, c->prob, (size_t)k, 0, 0, nullptr, ids, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);   // (ids; it waits for all three)
}

static int apply_device(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, int merging)
{
    const char* what = merging ? "sph_merge_particles_device" : "sph_share_particles_device";
    if (!c || !p || !ap) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = cand_refuse_common(c, what)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!solution_open(c))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: no open solution (sph_find_partners_device comes first; a step, an upload, an edit, a merge, a split or a later problem closes it)", what);
    if (c->prob_kind != merging) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: the open solution is of kind %d", what, c->prob_kind);
    return prob_apply(c, p, ap, merging, c->sol_partner.as<uint32_t>(), c->sol_counter.as<uint16_t>(), false);
}

extern "C" int sph_share_particles_device(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap) { return apply_device(c, p, ap, 0); }
extern "C" int sph_merge_particles_device(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap) { return apply_device(c, p, ap, 1); }
