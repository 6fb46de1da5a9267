// Adaptivity data path on the device: the apply half of single_step_adaptivity
// (/root/reference/src/simulation/simulation.rs:2732-2796).  The partner DECISIONS are the host's -- the reference takes them
// in a sequential loop over the particles (adaptivity/particle_sharing.rs:14-117, particle_merging.rs:16-125) -- and arrive as
// the merge_partner / merge_counter arrays of ParticleVec; what those arrays imply for the particle data is computed here, on
// the device-resident state, in the reference's index space:
//
//   share_particles   particle_sharing.rs:152-240   gather form: a receiver reads its donor, a donor only itself
//   merge_particles   particle_merging.rs:270-370   the same transfer + the swap-with-the-last deletion loop, restated as
//                                                    "the k-th hole from the front receives the k-th survivor from the back"
//                                                    (prefix sums over the delete flags in host order)
//   split_particles   splitting.rs:19-82            children appended in the order of the parents' indices (prefix sums over
//                                                    the child counts), positions from the SplitPatterns table
//
// Particles live in cell-sorted order on the device; orig[] maps a slot to the host index, slot_of[] back.  Merging and
// splitting end in a regather into host order (regather_host_order, sph_api.hip), like a sparse edit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "sph_candidates.hpp"
#include "sph_dist.hpp"
#include "sph_slab_partner_problem.h"
#include "sph_target_mass.hpp"

// (a slab context takes the slab form below: slab_adapt)
struct SlabCompact;
static int slab_adapt_rank(sph_ctx* c, int op, const sph_params* p, const sph_adapt_params* ap, const uint32_t* partner, const uint16_t* counter,
                           const SlabCompact* cd = nullptr);
#define ADAPT_CHECK(c, OP, PARTNER, COUNTER)                                                                                    \
    if (!(c) || !p || !ap) return SPH_ERR_INVALID_ARGUMENT;                                                                     \
    if ((c)->poisoned) return (c)->refuse_poisoned();                                                                           \
    (c)->lvl_pristine = false; /* every adaptivity entry point: the reorders move the level fields again */                    \
    if ((c)->dist.on) return slab_adapt_rank((c), (OP), p, ap, (PARTNER), (COUNTER))

// ---- exclusive prefix sum (u32), three launches: block sums, scan of the block sums, local scans ------------------------
#define SCAN_BLOCK 256
#define SCAN_ITEMS 8
#define SCAN_TILE (SCAN_BLOCK * SCAN_ITEMS)

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total)
{
    __shared__ uint32_t s_w[SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int k = 0; k < SCAN_BLOCK / 64; k++) {
        if (k < w) base += s_w[k];
        tot += s_w[k];
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_block_sums(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ sums)
{
    const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t v = 0;
    for (int k = 0; k < SCAN_ITEMS; k++)
        if (base + k < n) v += in[base + k];
    uint32_t tot;
    block_exclusive_scan(v, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_sums(uint32_t* __restrict__ sums, uint32_t nb, uint32_t* __restrict__ total)
{
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += SCAN_BLOCK) {   // one block walks the block sums in chunks (nb <= n / 2048)
        const uint32_t k = b0 + threadIdx.x;
        const uint32_t v = k < nb ? sums[k] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan(v, &tot);
        if (k < nb) sums[k] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_apply(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, const uint32_t* __restrict__ sums)
{
    const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    uint32_t loc[SCAN_ITEMS], v = 0;
    for (int k = 0; k < SCAN_ITEMS; k++) {
        loc[k] = base + k < n ? in[base + k] : 0u;
        v += loc[k];
    }
    uint32_t tot;
    uint32_t run = sums[blockIdx.x] + block_exclusive_scan(v, &tot);
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (base + k < n) out[base + k] = run;
        run += loc[k];
    }
}
void device_exclusive_scan_u32(hipStream_t s, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* scratch, uint32_t* total)
{
    const uint32_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    if (nb) hipLaunchKernelGGL(k_scan_block_sums, dim3(nb), dim3(SCAN_BLOCK), 0, s, in, n, scratch);
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_BLOCK), 0, s, scratch, nb, total);
    if (nb) hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(SCAN_BLOCK), 0, s, in, out, n, scratch);
}

// LevelEstimationState::target_mass (TargetP, target_mass, target_params): sph_target_mass.hpp, shared with sph_partner_search.hip

__global__ __launch_bounds__(256) void k_slot_of(uint32_t n, const uint32_t* __restrict__ orig, uint32_t* __restrict__ slot_of)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) slot_of[orig[i]] = i;
}

// ---- pass 1 of share_particles / merge_particles: the receivers (particle_sharing.rs:165-215, particle_merging.rs:277-325).
// A receiver writes only itself and reads only its donor, which no thread writes in this launch (merge_partner[donor] is
// DELETE, so the donor is nobody's receiver).  merging: the donor drops its whole mass (dropped_mass_merging, :372-385).
__global__ __launch_bounds__(256) void k_transfer_receive(uint32_t n, int merging, const uint32_t* __restrict__ orig, const uint32_t* __restrict__ slot_of,
                                                           const uint32_t* __restrict__ partner, const uint16_t* __restrict__ counter, uint32_t min_partners,
                                                           float dt, float max_transfer, TargetP tp, float4* __restrict__ pm, float2* __restrict__ vel,
                                                           const float* __restrict__ lvl, float* __restrict__ h2n, DeviceStatus* status)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = orig[s];
    const uint32_t j = partner[i];
    if (j == SPH_MERGE_PARTNER_AVAILABLE || j == SPH_MERGE_PARTNER_DELETE) return;
    if (j >= n) {
        if (atomicCAS(&status->error, 0u, (uint32_t)SPH_ERR_INVALID_ARGUMENT) == 0u) status->info = i;
        return;
    }
    const uint32_t cj = counter[j];
    if (cj < min_partners) return;
    const uint32_t sj = slot_of[j];
    float4 Pi = pm[s];
    const float4 Pj = pm[sj];
    float2 vi = vel[s];
    const float2 vj = vel[sj];
    float dropped;
    if (merging) dropped = Pj.z;
    else {
        const float target = target_mass(lvl[sj], tp);
        dropped = fminf(Pj.z - target, target * max_transfer * dt);
    }
    const float mass_i = Pi.z;
    const float mass_n = dropped / (float)cj;
    const float mass = mass_i + mass_n;
    vi.x = (mass_i * vi.x + mass_n * vj.x) / mass;
    vi.y = (mass_i * vi.y + mass_n * vj.y) / mass;
    Pi.x = (mass_i * Pi.x + mass_n * Pj.x) / mass;
    Pi.y = (mass_i * Pi.y + mass_n * Pj.y) / mass;
    Pi.z = mass;
    pm[s] = Pi;
    vel[s] = vi;
    h2n[s] = h_from_mass(mass, tp.rest_density);
}

// ---- pass 2: the donors.  sharing (particle_sharing.rs:217-239): mass -= dropped, h2_next from it.  merging
// (particle_merging.rs:339-355): mass -= dropped (h2_next untouched) and the particle is deleted if what is left is < 1e-6.
__global__ __launch_bounds__(256) void k_transfer_donate(uint32_t n, int merging, const uint32_t* __restrict__ orig, const uint32_t* __restrict__ partner,
                                                          const uint16_t* __restrict__ counter, uint32_t min_partners, float dt, float max_transfer,
                                                          TargetP tp, float4* __restrict__ pm, const float* __restrict__ lvl, float* __restrict__ h2n,
                                                          uint32_t* __restrict__ del_host)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = orig[s];
    uint32_t del = 0;
    if (partner[i] == SPH_MERGE_PARTNER_DELETE && counter[i] >= min_partners) {
        float4 P = pm[s];
        if (merging) {
            P.z -= P.z;   // dropped_mass_merging returns the whole mass
            del = P.z < 0.000001f ? 1u : 0u;
        } else {
            const float target = target_mass(lvl[s], tp);
            const float dropped = fminf(P.z - target, target * max_transfer * dt);
            P.z -= dropped;
            h2n[s] = h_from_mass(P.z, tp.rest_density);
        }
        pm[s] = P;
    }
    if (del_host) del_host[i] = del;
}

// ---- deletion order of merge_particles' swap loop (particle_merging.rs:337-365) in closed form.  n' = n - #deleted.
// Holes = deleted indices < n' (ascending); tail survivors = kept indices >= n' (descending); hole k <- tail survivor k.
__global__ __launch_bounds__(256) void k_merge_holes(uint32_t n, uint32_t n_new, const uint32_t* __restrict__ del, const uint32_t* __restrict__ del_before,
                                                      uint32_t* __restrict__ hole_by_rank, EditSrc* __restrict__ src)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_new) return;
    src[f] = EditSrc{f, 0xffffffffu};           // kept particles below n' stay where they are
    if (del[f]) hole_by_rank[del_before[f]] = f;
}
__global__ __launch_bounds__(256) void k_merge_fill(uint32_t n, uint32_t n_new, uint32_t n_del, const uint32_t* __restrict__ del, const uint32_t* __restrict__ del_before,
                                                     const uint32_t* __restrict__ hole_by_rank, EditSrc* __restrict__ src)
{
    const uint32_t t = n_new + blockIdx.x * 256 + threadIdx.x;
    if (t >= n || del[t]) return;
    // survivors with a larger index: (n - 1 - t) positions behind t, minus the deleted ones among them
    const uint32_t del_after = n_del - del_before[t] - del[t];
    const uint32_t rank = (n - 1u - t) - del_after;
    src[hole_by_rank[rank]] = EditSrc{t, 0xffffffffu};
}

// ---- split_particles (splitting.rs:19-82) ---------------------------------------------------------------------------
// child count of every host index (0 for a particle that does not split): num_children - 1 goes into the prefix sum
__global__ __launch_bounds__(256) void k_split_count(uint32_t n, const uint32_t* __restrict__ orig, const float4* __restrict__ pm, const float* __restrict__ lvl,
                                                      const uint8_t* __restrict__ szc, TargetP tp, uint32_t max_children, int fail_on_missing,
                                                      uint32_t* __restrict__ extra_host, DeviceStatus* status)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = orig[s];
    uint32_t extra = 0;
    if (szc[s] == 4 /* ParticleSizeClass::TooLarge */) {
        const float lv = lvl[s];
        const float target = target_mass(lv, tp);
        const float r = roundf(pm[s].z / target);            // FT::round: half away from zero
        // `as usize`: saturating, NaN -> 0
        uint32_t nc = !(r > 0.f) ? 0u : (r >= 4294967040.f ? 0xffffffffu : (uint32_t)r);
        bool bad = isnan(lv);                                  // LevelEstimationState::level() of FluidInterior: unreachable!()
        if (nc > max_children) {
            if (fail_on_missing) bad = true;                   // panic!("no split pattern for a 1-to-{} split")
            nc = max_children;
        }
        if (!(nc > 1u)) bad = true;                            // assert!(num_children > 1)
        if (bad) {
            if (atomicCAS(&status->error, 0u, (uint32_t)SPH_ERR_NO_SPLIT_PATTERN) == 0u) status->info = i;
        } else extra = nc - 1u;
    }
    extra_host[i] = extra;
}

// final index f -> what it holds: an old particle (the parent slot takes child 0's values) or an appended child
__global__ __launch_bounds__(256) void k_split_plan(uint32_t n, uint32_t n_new, const uint32_t* __restrict__ slot_of, const float4* __restrict__ pm,
                                                     const float2* __restrict__ vel, const float* __restrict__ lvl, const uint32_t* __restrict__ extra,
                                                     const uint32_t* __restrict__ base, const float2* __restrict__ patterns, float rest_density,
                                                     EditSrc* __restrict__ src, EditSet* __restrict__ sets)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_new) return;
    uint32_t parent, child_id;
    if (f < n) {
        parent = f;
        child_id = 0;
        if (extra[f] == 0u) {
            src[f] = EditSrc{f, 0xffffffffu};
            return;
        }
    } else {
        // the parent p with base[p] <= c < base[p] + extra[p]: the last index whose exclusive prefix sum is <= c
        const uint32_t c = f - n;
        uint32_t lo = 0, hi = n - 1u;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (base[mid] <= c) lo = mid;
            else hi = mid - 1u;
        }
        parent = lo;
        child_id = c - base[parent] + 1u;
    }
    const uint32_t sp = slot_of[parent];
    const float4 P = pm[sp];
    const uint32_t nc = extra[parent] + 1u;
    const float2 off = patterns[(nc - 1u) * nc / 2u - 1u + child_id];         // patterns of 2, 3, ... children, concatenated
    const float scale = sqrtf((P.z / 1.f /* INIT_REST_DENSITY */) * SPH_FRAC_1_PI_F);   // DU::sphere_volume_to_radius (sph_kernels.rs:203-206)
    const float child_mass = P.z / (float)nc;
    EditSet q{};
    q.mass = child_mass;
    q.px = P.x + off.x * scale;
    q.py = P.y + off.y * scale;
    q.h2 = q.h2_next = h_from_mass(child_mass, rest_density);
    if (child_id == 0u) {
        // the parent slot: mass, position, h2, h2_next (velocity, level_estimation, level_old are rewritten with their own values)
        q.fields = SPH_EDIT_F_MASS | SPH_EDIT_F_POSITION | SPH_EDIT_F_H2 | SPH_EDIT_F_H2_NEXT;
        src[f] = EditSrc{parent, f};
    } else {
        // an appended child: ParticleVec defaults + mass, velocity, position, h2_next, level_estimation.  h2 and level_old are
        // written to the PARENT's slot by the reference (splitting.rs:73, 76) and stay 0 here.
        const float2 v = vel[sp];
        q.vx = v.x;
        q.vy = v.y;
        q.lvl = lvl[sp];
        q.fields = SPH_EDIT_F_MASS | SPH_EDIT_F_POSITION | SPH_EDIT_F_VELOCITY | SPH_EDIT_F_H2_NEXT | SPH_EDIT_F_LEVEL_ESTIMATION;
        src[f] = EditSrc{0xfffffffeu /* a default particle */, f};
    }
    sets[f] = q;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static int check_status(sph_ctx* c, const char* what)
{
    DeviceStatus st;
    HIPCHK(c, hipMemcpyAsync(&st, c->status.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (st.error) {
        (void)hipMemsetAsync(c->status.p, 0, sizeof(DeviceStatus), c->stream);
        return c->fail((int)st.error, "%s (particle i=%u)", what, st.info);
    }
    return SPH_OK;
}

static int transfer(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, const uint32_t* partner, const uint16_t* counter, int merging)
{
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t n = (uint32_t)c->n;
    if (n == 0) return SPH_OK;
    if (!partner || !counter) return SPH_ERR_INVALID_ARGUMENT;
    // (before anything is launched: a bad index must not leave some receivers and donors already modified)
    for (uint32_t i = 0; i < n; i++)
        if (partner[i] >= n && partner[i] != SPH_MERGE_PARTNER_AVAILABLE && partner[i] != SPH_MERGE_PARTNER_DELETE)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "merge_partner holds an index outside the particle vector (particle i=%u: %u)", i, partner[i]);
    hipStream_t s = c->stream;
    TmpBuf d_partner, d_counter;
    if (d_partner.ensure((size_t)n * 4) != hipSuccess || d_counter.ensure((size_t)n * 2) != hipSuccess) return c->fail(SPH_ERR_DEVICE, "out of device memory");
    HIPCHK(c, hipMemcpyAsync(d_partner.p, partner, (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_counter.p, counter, (size_t)n * 2, hipMemcpyHostToDevice, s));
    return transfer_on_device(c, p, ap, d_partner.as<uint32_t>(), d_counter.as<uint16_t>(), merging);
}

// The receive / donate / delete path on merge_partner / merge_counter arrays that are on the device already (n > 0 entries each, queued
// on the context's stream): what transfer() runs behind its two uploads, and what the compact apply of sph_partner_problem.hip runs
// behind its expansion.  Returns after the stream has drained (check_status), so the caller may free the two arrays.
int transfer_on_device(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, const uint32_t* d_partner_p, const uint16_t* d_counter_p, int merging)
{
    const uint32_t n = (uint32_t)c->n;
    hipStream_t s = c->stream;
    const int k = c->cur;
    TmpBuf d_slot, d_del, d_before, d_scratch, d_holes, d_src, d_sets;
    auto release = [&] {
        for (TmpBuf* b : {&d_slot, &d_del, &d_before, &d_scratch, &d_holes, &d_src, &d_sets}) b->release();
    };
    auto guard = [&](hipError_t e) { return e == hipSuccess; };
    if (!guard(d_slot.ensure((size_t)n * 4))) {
        release();
        return c->fail(SPH_ERR_DEVICE, "out of device memory");
    }
    const dim3 grid((n + 255) / 256), blk(256);
    const TargetP tp = target_params(p);
    const uint32_t min_partners = merging ? ap->minimum_merge_partners : ap->minimum_share_partners;
    if (merging) {
        if (!guard(d_del.ensure((size_t)n * 4)) || !guard(d_before.ensure((size_t)n * 4 + 4)) || !guard(d_scratch.ensure(((size_t)n / SCAN_TILE + 4) * 4)) ||
            !guard(d_holes.ensure((size_t)n * 4))) {
            release();
            return c->fail(SPH_ERR_DEVICE, "out of device memory");
        }
    }
    hipLaunchKernelGGL(k_slot_of, grid, blk, 0, s, n, c->orig[k].as<uint32_t>(), d_slot.as<uint32_t>());
    hipLaunchKernelGGL(k_transfer_receive, grid, blk, 0, s, n, merging, c->orig[k].as<uint32_t>(), d_slot.as<uint32_t>(), d_partner_p,
                       d_counter_p, min_partners, ap->dt, ap->max_mass_transfer_sharing, tp, c->pm[c->pcur].as<float4>(), c->vel[k].as<float2>(),
                       c->lvl[k].as<float>(), c->h2n[k].as<float>(), c->status.as<DeviceStatus>());
    hipLaunchKernelGGL(k_transfer_donate, grid, blk, 0, s, n, merging, c->orig[k].as<uint32_t>(), d_partner_p, d_counter_p, min_partners,
                       ap->dt, ap->max_mass_transfer_sharing, tp, c->pm[c->pcur].as<float4>(), c->lvl[k].as<float>(), c->h2n[k].as<float>(),
                       merging ? d_del.as<uint32_t>() : nullptr);
    int rc = check_status(c, "merge_partner holds an index outside the particle vector");
    // positions and masses changed: what the last step left behind no longer describes the state
    c->drop(DROPS_TRANSFER);
    c->lvl_pristine = false;   // (an adaptivity entry point: the level fields may take other values)
    // (sharing neither reorders nor resizes the vector: stash and the step's flags keep describing the particles in their slots,
    //  as the reference's ParticleVec keeps them through share_particles -- snapshots taken after single_step show them)
    if (rc || !merging) {
        release();
        return rc;
    }
    // ---- delete (particle_merging.rs:337-369)
    uint32_t* d_total = d_before.as<uint32_t>() + n;
    device_exclusive_scan_u32(s, d_del.as<uint32_t>(), d_before.as<uint32_t>(), n, d_scratch.as<uint32_t>(), d_total);
    uint32_t n_del = 0;
    HIPCHK(c, hipMemcpyAsync(&n_del, d_total, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (n_del == 0) {
        release();
        return SPH_OK;
    }
    c->lvl_pristine = false;
    c->drop(DROPS_DELETION);   // the deletion reorders the vector: per-step outputs that do not travel (stash, flags) are gone
    // (the reference's loop never removes the particle it ends on when everything is deleted: last_particle_id is a usize that
    //  would underflow -- it panics there; an empty vector is what truncate(0) would leave)
    const uint32_t n_new = n - n_del;
    if (!guard(d_src.ensure(((size_t)n_new + 1) * sizeof(EditSrc))) || !guard(d_sets.ensure(sizeof(EditSet)))) {
        release();
        return c->fail(SPH_ERR_DEVICE, "out of device memory");
    }
    if (n_new) {
        hipLaunchKernelGGL(k_merge_holes, dim3((n_new + 255) / 256), blk, 0, s, n, n_new, d_del.as<uint32_t>(), d_before.as<uint32_t>(), d_holes.as<uint32_t>(),
                           d_src.as<EditSrc>());
        hipLaunchKernelGGL(k_merge_fill, dim3((n_del + 255) / 256), blk, 0, s, n, n_new, n_del, d_del.as<uint32_t>(), d_before.as<uint32_t>(),
                           d_holes.as<uint32_t>(), d_src.as<EditSrc>());
    }
    rc = regather_host_order(c, n_new, d_src.as<EditSrc>(), d_sets.as<EditSet>());
    release();
    return rc;
}

extern "C" int sph_share_particles(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, const uint32_t* partner, const uint16_t* counter)
{
    ADAPT_CHECK(c, 0, partner, counter);
    return transfer(c, p, ap, partner, counter, 0);
}

extern "C" int sph_merge_particles(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, const uint32_t* partner, const uint16_t* counter)
{
    ADAPT_CHECK(c, 1, partner, counter);
    c->drop(DROPS_EXPORT_EARLY);   // (the candidate export's lists index the vector before the deletions: sph_candidates.hip)
    return transfer(c, p, ap, partner, counter, 1);
}

extern "C" int sph_set_split_patterns(sph_ctx* c, uint32_t n_patterns, const float* pos_s_xy)
{
    if (!c || (n_patterns && !pos_s_xy)) return SPH_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->device));
    // SplitPatterns::new (splitting.rs:99-105): pattern k has k + 2 children
    size_t n_pos = 0;
    for (uint32_t k = 0; k < n_patterns; k++) n_pos += (size_t)k + 2;
    HIPCHK(c, c->split_patterns.ensure((n_pos ? n_pos : 1) * sizeof(float2)));
    if (n_pos) HIPCHK(c, hipMemcpy(c->split_patterns.p, pos_s_xy, n_pos * sizeof(float2), hipMemcpyHostToDevice));
    c->n_split_patterns = n_patterns;
    return SPH_OK;
}

extern "C" int sph_split_particles(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap)
{
    ADAPT_CHECK(c, 2, nullptr, nullptr);
    c->drop(DROPS_EXPORT_EARLY);
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t n = (uint32_t)c->n;
    if (n == 0) return SPH_OK;
    hipStream_t s = c->stream;
    const int k = c->cur;
    const uint32_t max_children = c->n_split_patterns + 1u;   // SplitPatterns::get_max_num_children (splitting.rs:115-117)
    TmpBuf d_extra, d_base, d_scratch, d_slot, d_src, d_sets;
    auto release = [&] {
        for (TmpBuf* b : {&d_extra, &d_base, &d_scratch, &d_slot, &d_src, &d_sets}) b->release();
    };
    if (d_extra.ensure((size_t)n * 4) != hipSuccess || d_base.ensure((size_t)n * 4 + 4) != hipSuccess ||
        d_scratch.ensure(((size_t)n / SCAN_TILE + 4) * 4) != hipSuccess || d_slot.ensure((size_t)n * 4) != hipSuccess) {
        release();
        return c->fail(SPH_ERR_DEVICE, "out of device memory");
    }
    const dim3 grid((n + 255) / 256), blk(256);
    const TargetP tp = target_params(p);
    hipLaunchKernelGGL(k_slot_of, grid, blk, 0, s, n, c->orig[k].as<uint32_t>(), d_slot.as<uint32_t>());
    hipLaunchKernelGGL(k_split_count, grid, blk, 0, s, n, c->orig[k].as<uint32_t>(), c->pm[c->pcur].as<float4>(), c->lvl[k].as<float>(), c->szc[k].as<uint8_t>(), tp,
                       max_children, ap->fail_on_missing_split_pattern, d_extra.as<uint32_t>(), c->status.as<DeviceStatus>());
    uint32_t* d_total = d_base.as<uint32_t>() + n;
    device_exclusive_scan_u32(s, d_extra.as<uint32_t>(), d_base.as<uint32_t>(), n, d_scratch.as<uint32_t>(), d_total);
    uint32_t n_extra = 0;
    HIPCHK(c, hipMemcpyAsync(&n_extra, d_total, 4, hipMemcpyDeviceToHost, s));
    int rc = check_status(c, max_children < 2 ? "no split pattern for a 1-to-2 split (sph_set_split_patterns was not called)"
                                              : "no split pattern for this split, or num_children <= 1");
    if (rc || n_extra == 0) {
        release();
        return rc;
    }
    if ((uint64_t)n + n_extra > c->cap) {
        release();
        return c->fail(SPH_ERR_CAPACITY, "splitting needs %llu particles, capacity %llu", (unsigned long long)n + n_extra, (unsigned long long)c->cap);
    }
    const uint32_t n_new = n + n_extra;
    if (d_src.ensure((size_t)n_new * sizeof(EditSrc)) != hipSuccess || d_sets.ensure((size_t)n_new * sizeof(EditSet)) != hipSuccess) {
        release();
        return c->fail(SPH_ERR_DEVICE, "out of device memory");
    }
    hipLaunchKernelGGL(k_split_plan, dim3((n_new + 255) / 256), blk, 0, s, n, n_new, d_slot.as<uint32_t>(), c->pm[c->pcur].as<float4>(), c->vel[k].as<float2>(),
                       c->lvl[k].as<float>(), d_extra.as<uint32_t>(), d_base.as<uint32_t>(), c->split_patterns.as<float2>(), p->rest_density,
                       d_src.as<EditSrc>(), d_sets.as<EditSet>());
    rc = regather_host_order(c, n_new, d_src.as<EditSrc>(), d_sets.as<EditSet>());
    release();
    return rc;
}


// =================================================================================================================================
// The same apply on a SLAB DECOMPOSITION (VERDICT r3 missing 1): the particles stay on their ranks.
//   * The reference's indices ARE the particles' global ids (SPH_F_PARTICLE_ID): merge_partner / merge_counter arrive as the arrays of
//     the WHOLE vector, indexed by id, the same on every rank (the decisions are taken in one place, sequentially, as the reference
//     takes them); n_global is the all-reduced sum of the owned counts.
//   * A receiver's donor is one of its neighbours (the partner searches walk the neighbour lists), so it sits in the rank's arrays as
//     an owned particle or as a ghost of the last step; the ghosts' records (position, mass, velocity, level) are refreshed from
//     their owners first -- the same bits on both sides of a cut -- and the gather-form transfer reads them like an owned donor's.
//     A donor only touches itself.  What a transfer moves across a cut is therefore carried by the ghost refresh; a receiver whose
//     new position lies beyond its slab is handed over by the next step's migration, like any particle that crossed.
//   * merge_particles' swap-with-the-last deletion renumbers the vector.  The delete flags follow from the two global arrays alone
//     (dropped_mass_merging returns the whole mass: a donor with enough receivers ends at mass 0 < 1e-6), so every rank derives the
//     SAME new index of every surviving id by itself (prefix sums over the n_global flags; "hole k <- tail survivor k"), deletes its
//     own donors, and renames its survivors: no collective at all.
//   * split_particles appends the children in the order of the parents' indices: the child counts are computed where the parents
//     live, scattered into an n_global array by id and ALL-REDUCED (the one collective of the apply), prefix-summed on every rank;
//     a child is created on its parent's rank with the id  n_global + prefix(parent) + child - 1.
// Afterwards every rank holds owned particles only (ids = the reference's new indices); the next step selects new ghosts.
// =================================================================================================================================
__global__ __launch_bounds__(256) void k_slab_slot_of(uint32_t n_tot, const uint32_t* __restrict__ orig, uint32_t n_global, uint32_t* __restrict__ slot_of,
                                                       DeviceStatus* status)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_tot) return;
    const uint32_t i = orig[s];
    if (i >= n_global) {
        if (atomicCAS(&status->error, 0u, (uint32_t)SPH_ERR_INVALID_ARGUMENT) == 0u) status->info = i;
        return;
    }
    slot_of[i] = s;
}
__global__ __launch_bounds__(256) void k_slab_receive(uint32_t n_tot, int merging, const uint8_t* __restrict__ owned, const uint32_t* __restrict__ orig,
                                                       const uint32_t* __restrict__ slot_of, uint32_t n_global, const uint32_t* __restrict__ partner,
                                                       const uint16_t* __restrict__ counter, uint32_t min_partners, float dt, float max_transfer, TargetP tp,
                                                       const float4* __restrict__ pm_in, const float2* __restrict__ vel_in, float4* __restrict__ pm_out,
                                                       float2* __restrict__ vel_out, const float* __restrict__ lvl, float* __restrict__ h2n, DeviceStatus* status)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_tot || !owned[s]) return;
    const uint32_t i = orig[s];
    const uint32_t j = partner[i];
    if (j == SPH_MERGE_PARTNER_AVAILABLE || j == SPH_MERGE_PARTNER_DELETE) return;
    const uint32_t sj = j < n_global ? slot_of[j] : 0xffffffffu;
    if (sj == 0xffffffffu) {   // an index outside the vector, or a donor that is no neighbour of its receiver (not among this rank's ghosts)
        if (atomicCAS(&status->error, 0u, (uint32_t)SPH_ERR_INVALID_ARGUMENT) == 0u) status->info = i;
        return;
    }
    const uint32_t cj = counter[j];
    if (cj < min_partners) return;
    float4 Pi = pm_in[s];
    const float4 Pj = pm_in[sj];
    float2 vi = vel_in[s];
    const float2 vj = vel_in[sj];
    float dropped;
    if (merging) dropped = Pj.z;
    else {
        const float target = target_mass(lvl[sj], tp);
        dropped = fminf(Pj.z - target, target * max_transfer * dt);
    }
    const float mass_i = Pi.z;
    const float mass_n = dropped / (float)cj;
    const float mass = mass_i + mass_n;
    vi.x = (mass_i * vi.x + mass_n * vj.x) / mass;
    vi.y = (mass_i * vi.y + mass_n * vj.y) / mass;
    Pi.x = (mass_i * Pi.x + mass_n * Pj.x) / mass;
    Pi.y = (mass_i * Pi.y + mass_n * Pj.y) / mass;
    Pi.z = mass;
    // (written to the OTHER record buffer: an owned donor next door must still be read as it was -- on one context nobody's donor is
    //  a receiver, here a receiver's record may be another lane's ghost-free donor only by the same rule, but the copy costs nothing)
    pm_out[s] = Pi;
    vel_out[s] = vi;
    h2n[s] = h_from_mass(mass, tp.rest_density);
}
__global__ __launch_bounds__(256) void k_slab_donate(uint32_t n_tot, int merging, const uint8_t* __restrict__ owned, const uint32_t* __restrict__ orig,
                                                      const uint32_t* __restrict__ partner, const uint16_t* __restrict__ counter, uint32_t min_partners, float dt,
                                                      float max_transfer, TargetP tp, float4* __restrict__ pm, const float* __restrict__ lvl, float* __restrict__ h2n)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_tot || !owned[s]) return;
    const uint32_t i = orig[s];
    if (partner[i] == SPH_MERGE_PARTNER_DELETE && counter[i] >= min_partners) {
        float4 P = pm[s];
        if (merging) P.z -= P.z;
        else {
            const float target = target_mass(lvl[s], tp);
            const float dropped = fminf(P.z - target, target * max_transfer * dt);
            P.z -= dropped;
            h2n[s] = h_from_mass(P.z, tp.rest_density);
        }
        pm[s] = P;
    }
}
// delete flags of the WHOLE vector from the decision arrays (merging: a donor with enough receivers drops its whole mass)
__global__ __launch_bounds__(256) void k_slab_del_flags(uint32_t n_global, const uint32_t* __restrict__ partner, const uint16_t* __restrict__ counter, uint32_t min_partners,
                                                         uint32_t* __restrict__ del)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_global) del[i] = (partner[i] == SPH_MERGE_PARTNER_DELETE && counter[i] >= min_partners) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_slab_newid(uint32_t n_new, const EditSrc* __restrict__ src, uint32_t* __restrict__ newid)
{
    const uint32_t f = blockIdx.x * 256 + threadIdx.x;
    if (f < n_new) newid[src[f].obj] = f;
}
// keep flag of every slot (owned survivors), then -- behind the scan -- the gather into the other buffer set
__global__ __launch_bounds__(256) void k_slab_keep(uint32_t n_tot, const uint8_t* __restrict__ owned, const uint32_t* __restrict__ orig, const uint32_t* __restrict__ del,
                                                    uint32_t* __restrict__ keep)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < n_tot) keep[s] = (owned[s] && !(del && del[orig[s]])) ? 1u : 0u;
}
struct SlabGather {
    const float4* pm_in; const float2* vel_in; const uint32_t* orig_in; const float* lvl_in; const float* lvlold_in; const float* h2n_in; const float* lam_in; const uint8_t* szc_in;
    float4* pm_out; float2* vel_out; uint32_t* orig_out; float* lvl_out; float* lvlold_out; float* h2n_out; float* lam_out; uint8_t* szc_out;
};
__global__ __launch_bounds__(256) void k_slab_compact(uint32_t n_tot, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ newid,
                                                       SlabGather g)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_tot || !keep[s]) return;
    const uint32_t f = pos[s];
    g.pm_out[f] = g.pm_in[s];
    g.vel_out[f] = g.vel_in[s];
    const uint32_t id = g.orig_in[s];
    g.orig_out[f] = newid ? newid[id] : id;
    g.lvl_out[f] = g.lvl_in[s];
    g.lvlold_out[f] = g.lvlold_in[s];
    g.h2n_out[f] = g.h2n_in[s];
    g.lam_out[f] = g.lam_in[s];
    g.szc_out[f] = g.szc_in[s];
}
// split: child count - 1 of every owned slot (k_split_count's rules), also scattered into the global array by id
__global__ __launch_bounds__(256) void k_slab_split_count(uint32_t n_tot, const uint8_t* __restrict__ owned, const uint32_t* __restrict__ orig, const float4* __restrict__ pm,
                                                           const float* __restrict__ lvl, const uint8_t* __restrict__ szc, TargetP tp, uint32_t max_children,
                                                           int fail_on_missing, uint32_t* __restrict__ extra_slot, uint32_t* __restrict__ extra_global, DeviceStatus* status)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_tot) return;
    uint32_t extra = 0;
    if (owned[s] && szc[s] == 4 /* ParticleSizeClass::TooLarge */) {
        const uint32_t i = orig[s];
        const float lv = lvl[s];
        const float target = target_mass(lv, tp);
        const float r = roundf(pm[s].z / target);
        uint32_t nc = !(r > 0.f) ? 0u : (r >= 4294967040.f ? 0xffffffffu : (uint32_t)r);
        bool bad = isnan(lv);
        if (nc > max_children) {
            if (fail_on_missing) bad = true;
            nc = max_children;
        }
        if (!(nc > 1u)) bad = true;
        if (bad) {
            if (atomicCAS(&status->error, 0u, (uint32_t)SPH_ERR_NO_SPLIT_PATTERN) == 0u) status->info = i;
        } else {
            extra = nc - 1u;
            extra_global[i] = extra;
        }
    }
    extra_slot[s] = extra;
}
// the owned particles (parents take child 0's values) to the front, the children behind them in slot order
__global__ __launch_bounds__(256) void k_slab_split_apply(uint32_t n_tot, uint32_t n_own, uint32_t n_global, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                                                           const uint32_t* __restrict__ extra_slot, const uint32_t* __restrict__ child_base, const uint32_t* __restrict__ base_global,
                                                           const float2* __restrict__ patterns, float rest_density, SlabGather g)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_tot || !keep[s]) return;
    const uint32_t f = pos[s];
    const float4 P = g.pm_in[s];
    const float2 v = g.vel_in[s];
    const uint32_t id = g.orig_in[s];
    const uint32_t extra = extra_slot[s];
    float4 Pf = P;
    float hn = g.h2n_in[s];
    if (extra) {
        const uint32_t nc = extra + 1u;
        const float scale = sqrtf((P.z / 1.f /* INIT_REST_DENSITY */) * SPH_FRAC_1_PI_F);
        const float child_mass = P.z / (float)nc;
        const float hc = h_from_mass(child_mass, rest_density);
        const float2* pat = patterns + ((nc - 1u) * nc / 2u - 1u);
        Pf = make_float4(P.x + pat[0].x * scale, P.y + pat[0].y * scale, child_mass, hc);   // child 0 in the parent's place: mass, position, h2, h2_next
        hn = hc;
        for (uint32_t k = 1; k < nc; k++) {
            const uint32_t fc = n_own + child_base[s] + (k - 1u);
            g.pm_out[fc] = make_float4(P.x + pat[k].x * scale, P.y + pat[k].y * scale, child_mass, 0.f);   // (h2 is written to the PARENT's slot by the reference: splitting.rs:73)
            g.vel_out[fc] = v;
            g.orig_out[fc] = n_global + base_global[id] + (k - 1u);
            g.lvl_out[fc] = g.lvl_in[s];
            g.lvlold_out[fc] = 0.f;
            g.h2n_out[fc] = hc;
            g.lam_out[fc] = 0.f;
            g.szc_out[fc] = 2;   // ParticleSizeClass::Optimal (ParticleVec default)
        }
    }
    g.pm_out[f] = Pf;
    g.vel_out[f] = v;
    g.orig_out[f] = id;
    g.lvl_out[f] = g.lvl_in[s];
    g.lvlold_out[f] = g.lvlold_in[s];
    g.h2n_out[f] = hn;
    g.lam_out[f] = g.lam_in[s];
    g.szc_out[f] = g.szc_in[s];
}

int refresh_ghost_state(Group& G, bool with_velocity)
{
    std::vector<Member> M(G.m.size());
    for (size_t i = 0; i < M.size(); i++) {
        sph_ctx* c = G.m[i];
        M[i].c = c;
        M[i].n = c->dist.n_tot;
        M[i].lv_pmnew = (float*)c->pm[c->pcur].as<float4>();
        M[i].lv_level = c->lvl[c->cur].as<float>();
        M[i].a.vel = c->vel[c->cur].as<float2>();
    }
    if (int rc = refresh_ghosts(G, M, [](Member& m) { return m.lv_pmnew; }, 4, "pm")) return rc;
    if (with_velocity)
        if (int rc = refresh_ghosts(G, M, [](Member& m) { return (float*)m.a.vel; }, 2, "vel")) return rc;
    return refresh_ghosts(G, M, [](Member& m) { return m.lv_level; }, 1, "level");
}

static SlabGather slab_gather_of(sph_ctx* c)
{
    const int k = c->cur;
    return SlabGather{c->pm[c->pcur].as<float4>(), c->vel[k].as<float2>(), c->orig[k].as<uint32_t>(), c->lvl[k].as<float>(), c->lvlold[k].as<float>(),
                      c->h2n[k].as<float>(), c->lam_sum.as<float>(), c->szc[k].as<uint8_t>(),
                      c->pm[c->pcur ^ 1].as<float4>(), c->vel[k ^ 1].as<float2>(), c->orig[k ^ 1].as<uint32_t>(), c->lvl[k ^ 1].as<float>(), c->lvlold[k ^ 1].as<float>(),
                      c->h2n[k ^ 1].as<float>(), c->lam_prev.as<float>(), c->szc[k ^ 1].as<uint8_t>()};
}
// the arrays now hold n_new owned particles in the other buffer set (lam_prev holds their lambda sums)
static void slab_after_regather(sph_ctx* c, uint32_t n_new)
{
    std::swap(c->lam_sum, c->lam_prev);
    c->cur ^= 1;
    c->pcur ^= 1;
    c->n = n_new;
    c->dist.n_tot = n_new;
    c->dist.n_ghost[0] = c->dist.n_ghost[1] = c->dist.n_halo[0] = c->dist.n_halo[1] = 0;
    c->drop(DROPS_REGATHER);
    c->lvl_pristine = false;   // (the regather writes one half of the level fields only)
}

// The decisions of a COMPACT problem (include/sph_slab_partner_problem.h): k participants by ascending global id, a partner named by its
// compact id.  The three arrays are the host's, the same on every rank; or (on_device, sph_slab_partner_search.hip) every member holds them
// on its own device -- slab_sol_ids / slab_sol_partner / slab_sol_counter, checked where they were made -- and the pointers here are null.
struct SlabCompact {
    uint64_t k;
    const uint32_t* ids;
    const uint32_t* partner_c;
    const uint16_t* counter_c;
    bool on_device = false;
};
// merge_partner / merge_counter of the whole vector on a member's device: copied from the host's arrays, or (cd) expanded from the k
// decisions (prob_expand, sph_partner_problem.hip) -- 10 B per participant go up instead of 6 B per particle.  Everything behind this
// point reads the two arrays and does not know which form they came in.  up_*: staging that lives as long as the arrays
static int slab_decisions_to_device(sph_ctx* c, hipStream_t s, uint32_t n_global, const uint32_t* partner, const uint16_t* counter, const SlabCompact* cd,
                                    uint32_t* d_partner, uint16_t* d_counter, TmpBuf& up_ids, TmpBuf& up_partner, TmpBuf& up_counter)
{
    if (cd && cd->on_device)   // (device arrays: nothing is staged)
        return prob_expand(c, "slab_problem_expand", n_global, (uint32_t)cd->k, c->slab_sol_ids.as<uint32_t>(), c->slab_sol_partner.as<uint32_t>(),
                           c->slab_sol_counter.as<uint16_t>(), d_partner, d_counter);
    if (cd) return prob_expand(c, "slab_problem_expand", n_global, (uint32_t)cd->k, cd->ids, cd->partner_c, cd->counter_c, d_partner, d_counter, ExpandStage{&up_ids, &up_partner, &up_counter});
    HIPCHK(c, hipMemcpyAsync(d_partner, partner, (size_t)n_global * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_counter, counter, (size_t)n_global * 2, hipMemcpyHostToDevice, s));
    return SPH_OK;
}

// op: 0 share, 1 merge, 2 split -- for every member of the group (collective over ALL ranks of the decomposition; the work on the
// members is the body of each_member: the collective rule, sph_dist.hpp)
// cd: the decisions come as a compact problem (partner / counter unused).  *together (optional): as rank_entry reads it -- here the one
// refusal every rank takes alike between two collectives
static int slab_adapt(Group& G, int op, const sph_params* p, const sph_adapt_params* ap, const uint32_t* partner, const uint16_t* counter, const SlabCompact* cd = nullptr,
                      bool* together = nullptr)
{
    const size_t nm = G.m.size();
    int rc = SPH_OK;
    for (auto c : G.m) {
        if (c->poisoned) return c->refuse_poisoned();
        if (!c->have_flags)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "the adaptivity apply on a slab context follows a step (it reads the donors across a cut from that step's ghost layer)");
        if (op == 2 && c->n_split_patterns + 1u < 2u) return c->fail(SPH_ERR_NO_SPLIT_PATTERN, "no split pattern for a 1-to-2 split (sph_set_split_patterns was not called)");
    }
    if (op != 2 && !cd && (!partner || !counter)) return SPH_ERR_INVALID_ARGUMENT;
    // ---- n_global: the vector the indices refer to
    uint32_t n_global = 0;
    {
        std::vector<std::vector<uint32_t>> rows(nm, std::vector<uint32_t>(1));
        for (size_t i = 0; i < nm; i++) rows[i][0] = (uint32_t)G.m[i]->n;
        if ((rc = G.comm->allreduce_sum_u32(G, rows))) return rc;
        n_global = rows[0][0];
    }
    if (cd && !cd->on_device && cd->k && cd->ids[cd->k - 1] >= n_global) {   // (ascending: the last id is the largest.  Every rank holds the same ids and the same sum)
        if (together) *together = true;
        return G.m[0]->fail(SPH_ERR_INVALID_ARGUMENT, "ids holds %u, the vector has %u particles", cd->ids[cd->k - 1], n_global);
    }
    if (n_global == 0) return SPH_OK;
    // ---- the ghosts' records as their owners hold them now
    if ((rc = refresh_ghost_state(G, true))) return rc;
    const TargetP tp = target_params(p);
    const dim3 blk(256);
    std::vector<TmpBuf> B(nm * 15);
    auto buf = [&](size_t i, int k) -> TmpBuf& { return B[i * 15 + (size_t)k]; };
    enum { B_PARTNER, B_COUNTER, B_SLOT, B_DEL, B_BEFORE, B_SCRATCH, B_HOLES, B_SRC, B_NEWID, B_KEEP, B_POS, B_EXTRA, B_UP_IDS, B_UP_PARTNER, B_UP_COUNTER };
    auto need = [&](sph_ctx* c, TmpBuf& b, size_t bytes) { return b.ensure(bytes ? bytes : 4) == hipSuccess ? SPH_OK : c->fail(SPH_ERR_DEVICE, "out of device memory"); };
    if (op != 2) {
        const int merging = op == 1;
        const uint32_t min_partners = merging ? ap->minimum_merge_partners : ap->minimum_share_partners;
        uint32_t n_del = 0, n_new_global = n_global;
        rc = each_member(G, [&](size_t i, sph_ctx* c) -> int {
            hipStream_t s = c->stream;
            const uint32_t nt = c->dist.n_tot;
            const int k = c->cur;
            int r;
            if ((r = need(c, buf(i, B_PARTNER), (size_t)n_global * 4)) || (r = need(c, buf(i, B_COUNTER), (size_t)n_global * 2)) || (r = need(c, buf(i, B_SLOT), (size_t)n_global * 4)))
                return r;
            if ((r = slab_decisions_to_device(c, s, n_global, partner, counter, cd, buf(i, B_PARTNER).as<uint32_t>(), buf(i, B_COUNTER).as<uint16_t>(), buf(i, B_UP_IDS),
                                              buf(i, B_UP_PARTNER), buf(i, B_UP_COUNTER))))
                return r;
            HIPCHK(c, hipMemsetAsync(buf(i, B_SLOT).p, 0xff, (size_t)n_global * 4, s));
            if (!nt) return SPH_OK;
            const dim3 grid((nt + 255) / 256);
            hipLaunchKernelGGL(k_slab_slot_of, grid, blk, 0, s, nt, c->orig[k].as<uint32_t>(), n_global, buf(i, B_SLOT).as<uint32_t>(), c->status.as<DeviceStatus>());
            // receivers write the other record / velocity buffers, which first take a copy of the current ones (donors, bystanders)
            HIPCHK(c, hipMemcpyAsync(c->pm[c->pcur ^ 1].p, c->pm[c->pcur].p, (size_t)nt * sizeof(float4), hipMemcpyDeviceToDevice, s));
            HIPCHK(c, hipMemcpyAsync(c->vel[k ^ 1].p, c->vel[k].p, (size_t)nt * sizeof(float2), hipMemcpyDeviceToDevice, s));
            hipLaunchKernelGGL(k_slab_receive, grid, blk, 0, s, nt, merging, c->dist.owned.as<uint8_t>(), c->orig[k].as<uint32_t>(), buf(i, B_SLOT).as<uint32_t>(), n_global,
                               buf(i, B_PARTNER).as<uint32_t>(), buf(i, B_COUNTER).as<uint16_t>(), min_partners, ap->dt, ap->max_mass_transfer_sharing, tp,
                               c->pm[c->pcur].as<float4>(), c->vel[k].as<float2>(), c->pm[c->pcur ^ 1].as<float4>(), c->vel[k ^ 1].as<float2>(), c->lvl[k].as<float>(),
                               c->h2n[k].as<float>(), c->status.as<DeviceStatus>());
            hipLaunchKernelGGL(k_slab_donate, grid, blk, 0, s, nt, merging, c->dist.owned.as<uint8_t>(), c->orig[k].as<uint32_t>(), buf(i, B_PARTNER).as<uint32_t>(),
                               buf(i, B_COUNTER).as<uint16_t>(), min_partners, ap->dt, ap->max_mass_transfer_sharing, tp, c->pm[c->pcur ^ 1].as<float4>(), c->lvl[k].as<float>(),
                               c->h2n[k].as<float>());
            // the updated records become the current ones (velocities likewise); the slots stay where they are
            HIPCHK(c, hipMemcpyAsync(c->pm[c->pcur].p, c->pm[c->pcur ^ 1].p, (size_t)nt * sizeof(float4), hipMemcpyDeviceToDevice, s));
            HIPCHK(c, hipMemcpyAsync(c->vel[k].p, c->vel[k ^ 1].p, (size_t)nt * sizeof(float2), hipMemcpyDeviceToDevice, s));
            r = check_status(c, "merge_partner holds an index outside the particle vector, or a donor that is not a neighbour of its receiver");
            c->lvl_pristine = false;
            c->drop(DROPS_TRANSFER);   // (also behind a failed check: the records were written)
            return r;
        });
        if (rc) return rc;
        if (!merging) return SPH_OK;
        // ---- delete: every rank derives the new index of every id from the two global arrays
        rc = each_member(G, [&](size_t i, sph_ctx* c) -> int {
            hipStream_t s = c->stream;
            int r;
            if ((r = need(c, buf(i, B_DEL), (size_t)n_global * 4)) || (r = need(c, buf(i, B_BEFORE), (size_t)n_global * 4 + 4)) ||
                (r = need(c, buf(i, B_SCRATCH), ((size_t)n_global / SCAN_TILE + 4) * 4)) || (r = need(c, buf(i, B_HOLES), (size_t)n_global * 4)))
                return r;
            hipLaunchKernelGGL(k_slab_del_flags, dim3((n_global + 255) / 256), blk, 0, s, n_global, buf(i, B_PARTNER).as<uint32_t>(), buf(i, B_COUNTER).as<uint16_t>(),
                               min_partners, buf(i, B_DEL).as<uint32_t>());
            uint32_t* d_total = buf(i, B_BEFORE).as<uint32_t>() + n_global;
            device_exclusive_scan_u32(s, buf(i, B_DEL).as<uint32_t>(), buf(i, B_BEFORE).as<uint32_t>(), n_global, buf(i, B_SCRATCH).as<uint32_t>(), d_total);
            uint32_t nd = 0;
            HIPCHK(c, hipMemcpyAsync(&nd, d_total, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            n_del = nd;   // (the same on every member: the same arrays)
            return SPH_OK;
        });
        if (rc) return rc;
        if (n_del == 0) return SPH_OK;
        n_new_global = n_global - n_del;
        return each_member(G, [&](size_t i, sph_ctx* c) -> int {
            hipStream_t s = c->stream;
            const uint32_t nt = c->dist.n_tot;
            int r;
            if ((r = need(c, buf(i, B_SRC), ((size_t)n_new_global + 1) * sizeof(EditSrc))) || (r = need(c, buf(i, B_NEWID), (size_t)n_global * 4)) ||
                (r = need(c, buf(i, B_KEEP), (size_t)nt * 4 + 4)) || (r = need(c, buf(i, B_POS), (size_t)nt * 4 + 8)))
                return r;
            if (n_new_global) {
                hipLaunchKernelGGL(k_merge_holes, dim3((n_new_global + 255) / 256), blk, 0, s, n_global, n_new_global, buf(i, B_DEL).as<uint32_t>(), buf(i, B_BEFORE).as<uint32_t>(),
                                   buf(i, B_HOLES).as<uint32_t>(), buf(i, B_SRC).as<EditSrc>());
                hipLaunchKernelGGL(k_merge_fill, dim3((n_del + 255) / 256), blk, 0, s, n_global, n_new_global, n_del, buf(i, B_DEL).as<uint32_t>(), buf(i, B_BEFORE).as<uint32_t>(),
                                   buf(i, B_HOLES).as<uint32_t>(), buf(i, B_SRC).as<EditSrc>());
                hipLaunchKernelGGL(k_slab_newid, dim3((n_new_global + 255) / 256), blk, 0, s, n_new_global, buf(i, B_SRC).as<EditSrc>(), buf(i, B_NEWID).as<uint32_t>());
            }
            uint32_t n_keep = 0;
            if (nt) {
                const dim3 grid((nt + 255) / 256);
                hipLaunchKernelGGL(k_slab_keep, grid, blk, 0, s, nt, c->dist.owned.as<uint8_t>(), c->orig[c->cur].as<uint32_t>(), buf(i, B_DEL).as<uint32_t>(), buf(i, B_KEEP).as<uint32_t>());
                uint32_t* d_tot = buf(i, B_POS).as<uint32_t>() + nt;
                device_exclusive_scan_u32(s, buf(i, B_KEEP).as<uint32_t>(), buf(i, B_POS).as<uint32_t>(), nt, buf(i, B_SCRATCH).as<uint32_t>(), d_tot);
                hipLaunchKernelGGL(k_slab_compact, grid, blk, 0, s, nt, buf(i, B_KEEP).as<uint32_t>(), buf(i, B_POS).as<uint32_t>(), buf(i, B_NEWID).as<uint32_t>(), slab_gather_of(c));
                HIPCHK(c, hipMemcpyAsync(&n_keep, d_tot, 4, hipMemcpyDeviceToHost, s));
            }
            HIPCHK(c, hipStreamSynchronize(s));
            slab_after_regather(c, n_keep);
            return SPH_OK;
        });
    }
    // ---- split
    uint32_t n_extra_global = 0;
    rc = each_member(G, [&](size_t i, sph_ctx* c) -> int {
        hipStream_t s = c->stream;
        const uint32_t nt = c->dist.n_tot;
        int r;
        if ((r = need(c, buf(i, B_EXTRA), (size_t)nt * 4 + 4)) || (r = need(c, buf(i, B_DEL), (size_t)n_global * 4)) || (r = need(c, buf(i, B_BEFORE), (size_t)n_global * 4 + 4)) ||
            (r = need(c, buf(i, B_SCRATCH), ((size_t)std::max(n_global, nt) / SCAN_TILE + 4) * 4)))
            return r;
        HIPCHK(c, hipMemsetAsync(buf(i, B_DEL).p, 0, (size_t)n_global * 4, s));   // (B_DEL: the child counts - 1 of the whole vector, by id)
        if (nt)
            hipLaunchKernelGGL(k_slab_split_count, dim3((nt + 255) / 256), blk, 0, s, nt, c->dist.owned.as<uint8_t>(), c->orig[c->cur].as<uint32_t>(), c->pm[c->pcur].as<float4>(),
                               c->lvl[c->cur].as<float>(), c->szc[c->cur].as<uint8_t>(), tp, c->n_split_patterns + 1u, ap->fail_on_missing_split_pattern,
                               buf(i, B_EXTRA).as<uint32_t>(), buf(i, B_DEL).as<uint32_t>(), c->status.as<DeviceStatus>());
        return check_status(c, "no split pattern for this split, or num_children <= 1");
    });
    if (rc) return rc;
    {
        std::vector<uint32_t*> bufs(nm);
        for (size_t i = 0; i < nm; i++) bufs[i] = buf(i, B_DEL).as<uint32_t>();
        if ((rc = G.comm->allreduce_sum_u32_dev(G, bufs, n_global))) return rc;
    }
    rc = each_member(G, [&](size_t i, sph_ctx* c) -> int {
        hipStream_t s = c->stream;
        uint32_t* d_total = buf(i, B_BEFORE).as<uint32_t>() + n_global;
        device_exclusive_scan_u32(s, buf(i, B_DEL).as<uint32_t>(), buf(i, B_BEFORE).as<uint32_t>(), n_global, buf(i, B_SCRATCH).as<uint32_t>(), d_total);
        uint32_t ne = 0;
        HIPCHK(c, hipMemcpyAsync(&ne, d_total, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        n_extra_global = ne;
        return SPH_OK;
    });
    if (rc) return rc;
    if (n_extra_global == 0) return SPH_OK;
    if ((uint64_t)n_global + n_extra_global >= 0xfffffff0ull) return G.m[0]->fail(SPH_ERR_CAPACITY, "splitting needs %llu particle ids", (unsigned long long)n_global + n_extra_global);
    return each_member(G, [&](size_t i, sph_ctx* c) -> int {
        hipStream_t s = c->stream;
        const uint32_t nt = c->dist.n_tot, n_own = (uint32_t)c->n;
        int r;
        if ((r = need(c, buf(i, B_KEEP), (size_t)nt * 4 + 4)) || (r = need(c, buf(i, B_POS), (size_t)nt * 4 + 8)) || (r = need(c, buf(i, B_HOLES), (size_t)nt * 4 + 8))) return r;
        uint32_t n_children = 0, n_keep = 0;
        if (nt) {
            const dim3 grid((nt + 255) / 256);
            hipLaunchKernelGGL(k_slab_keep, grid, blk, 0, s, nt, c->dist.owned.as<uint8_t>(), c->orig[c->cur].as<uint32_t>(), (const uint32_t*)nullptr, buf(i, B_KEEP).as<uint32_t>());
            uint32_t* d_tot = buf(i, B_POS).as<uint32_t>() + nt;
            device_exclusive_scan_u32(s, buf(i, B_KEEP).as<uint32_t>(), buf(i, B_POS).as<uint32_t>(), nt, buf(i, B_SCRATCH).as<uint32_t>(), d_tot);
            uint32_t* d_tot2 = buf(i, B_HOLES).as<uint32_t>() + nt;   // (B_HOLES: exclusive prefix of the children over the slots)
            device_exclusive_scan_u32(s, buf(i, B_EXTRA).as<uint32_t>(), buf(i, B_HOLES).as<uint32_t>(), nt, buf(i, B_SCRATCH).as<uint32_t>(), d_tot2);
            HIPCHK(c, hipMemcpyAsync(&n_keep, d_tot, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipMemcpyAsync(&n_children, d_tot2, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            if (n_keep != n_own) r = c->fail(SPH_ERR_DEVICE, "owned-particle count mismatch");
            else if ((uint64_t)n_own + n_children > c->cap)
                r = c->fail(SPH_ERR_CAPACITY, "splitting needs %llu particles on rank %d, capacity %llu", (unsigned long long)n_own + n_children, c->dist.rank, (unsigned long long)c->cap);
            else
                hipLaunchKernelGGL(k_slab_split_apply, grid, blk, 0, s, nt, n_own, n_global, buf(i, B_KEEP).as<uint32_t>(), buf(i, B_POS).as<uint32_t>(), buf(i, B_EXTRA).as<uint32_t>(),
                                   buf(i, B_HOLES).as<uint32_t>(), buf(i, B_BEFORE).as<uint32_t>(), c->split_patterns.as<float2>(), p->rest_density, slab_gather_of(c));
        }
        HIPCHK(c, hipStreamSynchronize(s));
        if (!r) slab_after_regather(c, n_own + n_children);
        return r;
    });
}

static int slab_adapt_rank(sph_ctx* c, int op, const sph_params* p, const sph_adapt_params* ap, const uint32_t* partner, const uint16_t* counter, const SlabCompact* cd)
{
    return rank_entry(c, "sph_group_adapt", [&](Group& G, bool* together) -> int { return slab_adapt(G, op, p, ap, partner, counter, cd, together); });
}

// share (op 0) / merge (1) / split (2) for the k contexts of ONE process that sph_group_step steps as ranks 0 .. k-1
extern "C" int sph_group_adapt(sph_ctx** ctxs, int n, int op, const sph_params* p, const sph_adapt_params* ap, const uint32_t* merge_partner,
                               const uint16_t* merge_counter)
{
    if (!p || !ap || op < 0 || op > 2) return SPH_ERR_INVALID_ARGUMENT;
    Group G;
    if (int rc = group_entry(G, ctxs, n)) return rc;
    return slab_adapt(G, op, p, ap, merge_partner, merge_counter);
}

// ---- include/sph_slab_partner_problem.h: the same apply from the K decisions of a compact problem ----------------------------
// on the host, before any collective and before anything on the device is written (the id >= n_global check follows in slab_adapt)
static int slab_compact_check(sph_ctx* c, const char* what, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids, const uint32_t* partner_c,
                              const uint16_t* counter_c)
{
    if (!p || !ap) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: params and ap must be given", what);
    if (k >= 0xfffffff0ull) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: k=%llu", what, (unsigned long long)k);
    if (k && (!ids || !partner_c || !counter_c)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: ids, partner_c and counter_c must be given", what);
    return prob_check_decisions(c, what, k, ids, partner_c);
}

static int slab_apply_compact_rank(sph_ctx* c, int op, const char* what, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids,
                                   const uint32_t* partner_c, const uint16_t* counter_c)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s: not a slab context (a plain context takes sph_download_partner_problem and sph_share_particles_compact / sph_merge_particles_compact)", what);
    if (c->poisoned) return c->refuse_poisoned();
    if (int rc = slab_compact_check(c, what, p, ap, k, ids, partner_c, counter_c)) return rc;
    const SlabCompact cd{k, ids, partner_c, counter_c, false};
    return slab_adapt_rank(c, op, p, ap, nullptr, nullptr, &cd);
}

extern "C" int sph_slab_share_particles_compact(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids, const uint32_t* partner_c,
                                                const uint16_t* counter_c)
{
    return slab_apply_compact_rank(c, 0, "sph_slab_share_particles_compact", p, ap, k, ids, partner_c, counter_c);
}

extern "C" int sph_slab_merge_particles_compact(sph_ctx* c, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids, const uint32_t* partner_c,
                                                const uint16_t* counter_c)
{
    return slab_apply_compact_rank(c, 1, "sph_slab_merge_particles_compact", p, ap, k, ids, partner_c, counter_c);
}

extern "C" int sph_group_adapt_compact(sph_ctx** ctxs, int n, int op, const sph_params* p, const sph_adapt_params* ap, uint64_t k, const uint32_t* ids,
                                       const uint32_t* partner_c, const uint16_t* counter_c)
{
    if (!ctxs || n <= 0) return SPH_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n; i++)
        if (!ctxs[i]) return SPH_ERR_INVALID_ARGUMENT;
    if (op != 0 && op != 1) return ctxs[0]->fail(SPH_ERR_INVALID_ARGUMENT, "sph_group_adapt_compact: op %d is neither 0 (share) nor 1 (merge)", op);
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on) return ctxs[i]->fail(SPH_ERR_UNSUPPORTED, "sph_group_adapt_compact: context %d is not a slab context", i);
    Group G;
    if (int rc = group_entry(G, ctxs, n)) return rc;
    for (auto c : G.m)
        if (c->poisoned) return c->refuse_poisoned();
    if (int rc = slab_compact_check(ctxs[0], "sph_group_adapt_compact", p, ap, k, ids, partner_c, counter_c)) return rc;
    const SlabCompact cd{k, ids, partner_c, counter_c, false};
    return slab_adapt(G, op, p, ap, nullptr, nullptr, &cd);
}

int slab_adapt_device(Group& G, int op, const sph_params* p, const sph_adapt_params* ap, uint64_t k)
{
    const SlabCompact cd{k, nullptr, nullptr, nullptr, true};
    return slab_adapt(G, op, p, ap, nullptr, nullptr, &cd);
}

// ---- the partner searches as host code (sph_ffi.h: sph_host_find_partners) ------------------------------------------------
static float host_target_mass(float lv, const sph_params* p)
{
    const float lvl = fmaxf(lv, -p->maximum_surface_distance);
    const float interp = lvl / -p->maximum_surface_distance;
    const float mass_fine = (SPH_PI_F * p->particle_radius_fine * p->particle_radius_fine) * p->rest_density;
    const float mass_base = (SPH_PI_F * p->particle_radius_base * p->particle_radius_base) * p->rest_density;
    if (p->sizing_function == SPH_SIZING_MASS) return mass_fine * (1.f - interp) + mass_base * interp;
    if (p->sizing_function == SPH_SIZING_RADIUS) {
        const float r = p->particle_radius_fine * (1.f - interp) + p->particle_radius_base * interp;
        return (SPH_PI_F * r * r) * p->rest_density;
    }
    const float e = 1.f / 2.f;
    const float r = p->particle_radius_fine * (1.f - powf(interp, e)) + p->particle_radius_base * powf(interp, e);
    return (SPH_PI_F * r * r) * p->rest_density;
}

extern "C" int sph_host_find_partners(int kind, uint64_t n, const uint8_t* cls, const float* mass, const float* level, const float* pos, const float* h2,
                                      const uint32_t* off, const uint32_t* idx, const sph_params* p, const sph_adapt_params* ap, uint32_t* partner,
                                      uint16_t* counter, uint64_t* n_transfers)
{
    if ((kind != 0 && kind != 1) || !p || !ap || !n_transfers || (n && (!cls || !mass || !level || !pos || !h2 || !off || !idx || !partner || !counter)))
        return SPH_ERR_INVALID_ARGUMENT;
    const bool share = kind == 0;
    const uint8_t donor_class = share ? 3 /* Large */ : 0 /* TooSmall */;
    const float mass_base = (SPH_PI_F * p->particle_radius_base * p->particle_radius_base) * p->rest_density;   // SimulationParams::mass_base
    const float max_dist_factor = share ? ap->max_share_distance : ap->max_merge_distance;
    for (uint64_t i = 0; i < n; i++) partner[i] = SPH_MERGE_PARTNER_AVAILABLE;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        counter[i] = 0;
        if (cls[i] != donor_class) continue;
        float dropped;
        if (share) {
            const float target = host_target_mass(level[i], p);     // dropped_mass_sharing (particle_sharing.rs:242-253)
            dropped = fminf(mass[i] - target, target * ap->max_mass_transfer_sharing * ap->dt);
        } else dropped = mass[i];                                   // dropped_mass_merging (particle_merging.rs:372-385)
        // Two reorderings of the reference's filters that cannot change a decision (every filter is a pure test; nothing is written
        // before all of them passed): (i) a donor that is already somebody's partner accepts nobody -- with counter[i] == 0 every
        // candidate ends at the "this particle is itself somebody's partner" test below -- so its row is only bounds-checked; (ii) "the
        // neighbour is somebody's partner already" is tested first: it reads one word where the others read five arrays at a random j.
        // In configs[4]'s merging pass (3 M donors of 4 M particles) most rows and most candidates leave there.
        if (partner[i] != SPH_MERGE_PARTNER_AVAILABLE) {
            for (uint32_t q = off[i]; q < off[i + 1]; q++)
                if (idx[q] >= n) return SPH_ERR_INVALID_ARGUMENT;
            continue;
        }
        for (uint32_t q = off[i]; q < off[i + 1]; q++) {
            const uint64_t j = idx[q];
            if (j == i) continue;
            if (j >= n) return SPH_ERR_INVALID_ARGUMENT;
            if (partner[j] != SPH_MERGE_PARTNER_AVAILABLE) continue;   // the neighbour is somebody's partner already
            bool can;
            if (share) can = cls[j] == 1 || (cls[j] == 0 && ap->allow_share_with_too_small_particle) || (cls[j] == 2 && ap->allow_share_with_optimal_particle);
            else {
                can = cls[j] == 1 || cls[j] == 0 || (cls[j] == 2 && ap->allow_merge_with_optimal_particle);
                if (ap->allow_merge_on_size_difference && mass[j] > 5.f * mass[i]) can = true;
            }
            if (!can) continue;
            // the partner must lie within max_{share,merge}_distance mean smoothing lengths (particle_sharing.rs:60-67, particle_merging.rs:71-78)
            const float dx = pos[2 * i] - pos[2 * j], dy = pos[2 * i + 1] - pos[2 * j + 1];
            const float max_dist = ((h2[i] + h2[j]) * 0.5f) * max_dist_factor;
            if (dx * dx + dy * dy > max_dist * max_dist) continue;
            const float new_mass_j = mass[j] + dropped / (float)(counter[i] + 1);
            const float target_j = host_target_mass(level[j], p);
            if (new_mass_j >= target_j * 1.1f /* PARTICLE_SIZE_FACTOR_LARGE */) continue;
            if (new_mass_j > mass_base) continue;
            if (counter[i] == 0) partner[i] = SPH_MERGE_PARTNER_DELETE;   // (available: tested at the head of the row)
            partner[j] = (uint32_t)i;
            counter[i] += 1;
            total += 1;
            if (!(counter[i] < 1000)) return SPH_ERR_INVALID_ARGUMENT;   // assert!(merge_counter[i] < 1000)
        }
    }
    // validate_share_partners / validate_merge_partners (particle_sharing.rs:119-150, particle_merging.rs:226-268)
    for (uint64_t i = 0; i < n; i++) {
        if (counter[i] > 0) {
            if (cls[i] != donor_class || partner[i] != SPH_MERGE_PARTNER_DELETE) return SPH_ERR_INVALID_ARGUMENT;
            uint32_t c2 = 0;
            for (uint32_t q = off[i]; q < off[i + 1]; q++) c2 += partner[idx[q]] == (uint32_t)i ? 1u : 0u;
            if (c2 != counter[i]) return SPH_ERR_INVALID_ARGUMENT;
        } else {
            if (partner[i] == SPH_MERGE_PARTNER_DELETE) return SPH_ERR_INVALID_ARGUMENT;
            if (partner[i] != SPH_MERGE_PARTNER_AVAILABLE && partner[partner[i]] != SPH_MERGE_PARTNER_DELETE) return SPH_ERR_INVALID_ARGUMENT;
        }
    }
    *n_transfers = total;
    return SPH_OK;
}
