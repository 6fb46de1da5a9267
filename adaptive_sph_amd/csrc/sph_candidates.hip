// include/sph_candidates.h: the share / merge partner candidates filtered on the device, and the mass sum of the adaptive step's
// conservation check.
//
// The partner searches (find_share_partner_sequential, particle_sharing.rs:14-117; find_merge_partner_sequential,
// particle_merging.rs:16-125) stay on the host.  What moves here are their two state-independent tests -- the neighbour's size
// class and its distance -- so that the host receives a few candidates per donor instead of every neighbour list.
//
//   gather   slot s -> host index i = orig[s]: the {x, y, mass, h2} record and the class byte in HOST order (the CSR's rows
//            and its entries are host indices; one gather per list entry then reads one record instead of slot_of + record)
//   count    one thread per host row; a row that is no donor writes 0 without reading its list
//   scan     device_exclusive_scan_u32 (sph_adapt.hip): offsets[n + 1], the total in the last word; only that word and the
//            finished offsets cross the bus
//   fill     the same walk, writing the passing j at the row's offset
//
// Mapping: thread per row over ALL rows, idle lanes for the non-donors (no compaction of the donor ids).  A lane whose row is no
// donor costs one byte load; a compacted donor list would save the divergence inside mixed waves and cost a second scan
// (scripts/gpu_candidates_time.py reports the two kernels' times: scopes candidates_count / candidates_fill).
//
// Arithmetic: the reference's f32 operations in its order, written with the explicit round-to-nearest intrinsics -- nothing here
// may contract into an fma under either math policy, since the result is an index set compared entry by entry with the host's.
#include <hip/hip_runtime.h>

#include "sph_candidates.h"
#include "sph_candidates.hpp"

__global__ __launch_bounds__(256) void k_cand_gather(uint32_t n, const uint32_t* __restrict__ orig, const float4* __restrict__ pm,
                                                      const uint8_t* __restrict__ szc, float4* __restrict__ rec, uint8_t* __restrict__ cls)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = orig[s];
    if (i >= n) return;
    rec[i] = pm[s];
    cls[i] = szc[s];
}

// FILL = false: cnt[i] = candidates of row i.  FILL = true: the candidates at out_off[i] (out_off: the scanned counts).
template <bool FILL>
__global__ __launch_bounds__(256) void k_cand_rows(uint32_t n, CandP q, const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx, uint64_t tot,
                                                    const float4* __restrict__ rec, const uint8_t* __restrict__ cls, uint32_t* __restrict__ cnt,
                                                    const uint32_t* __restrict__ out_off, uint32_t* __restrict__ out_idx)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t c = 0;
    if (cls[i] == q.donor_class) {
        uint32_t w = 0, w_end = 0;
        if (FILL) {
            w = out_off[i];
            w_end = out_off[i + 1];
        }
        cand_walk_row(q, i, i, n, rec[i], off, idx, tot, rec, cls, [&](uint32_t j) {
            if (FILL) {
                if (w < w_end) out_idx[w] = j;
                w++;
            } else c++;
        });
    }
    if (!FILL) cnt[i] = c;
}

int cand_refuse_common(sph_ctx* c, const char* what)
{
    if (c->poisoned) return c->refuse_poisoned();
    if (c->dist.on)
        return c->fail(SPH_ERR_UNSUPPORTED, "%s: a slab context holds a slab of the particles (assemble the full lists: sph_download_neighbors per rank)", what);
    return SPH_OK;
}

int cand_check_args(sph_ctx* c, const char* what, int kind, const sph_params* p, const sph_adapt_params* ap)
{
    if (!p || !ap) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: params and ap must be given", what);
    if (kind != 0 && kind != 1) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: kind %d is neither 0 (share) nor 1 (merge)", what, kind);
    return SPH_OK;
}

CandP cand_params(int kind, const sph_adapt_params* ap)
{
    return CandP{kind == 0,
                 kind == 0 ? 3u : 0u,
                 kind == 0 ? ap->max_share_distance : ap->max_merge_distance,
                 kind == 0 ? ap->allow_share_with_optimal_particle : ap->allow_merge_with_optimal_particle,
                 ap->allow_share_with_too_small_particle,
                 ap->allow_merge_on_size_difference};
}

int cand_need_lists(sph_ctx* c)
{
    if (c->export_valid) return SPH_OK;
    if (!c->grid_valid) return c->fail(SPH_ERR_INVALID_ARGUMENT, "no neighbour lists of a step on the device: run a step first");
    return export_lists_on_device(c);
}

int cand_count_rows(sph_ctx* c, const CandP& q, uint32_t* offsets_host, uint32_t* tot)
{
    const uint32_t n = (uint32_t)c->n;
    hipStream_t s = c->stream;
    HIPCHK(c, c->cand_rec.ensure((size_t)n * sizeof(float4)));
    HIPCHK(c, c->cand_cls.ensure((size_t)n));
    HIPCHK(c, c->cand_cnt.ensure((size_t)n * 4));
    HIPCHK(c, c->cand_off.ensure(((size_t)n + 1) * 4));
    HIPCHK(c, c->cand_scan.ensure(((size_t)n / 2048 + 4) * 4));   // device_exclusive_scan_u32: one word per tile of 2048
    const dim3 grid((n + 255) / 256), blk(256);
    uint32_t* out_off = c->cand_off.as<uint32_t>();
    {
        ProfScope ps(&c->prof, "candidates_count", s);
        hipLaunchKernelGGL(k_cand_gather, grid, blk, 0, s, n, c->orig[c->cur].as<uint32_t>(), c->pm[c->pcur].as<float4>(), c->szc[c->cur].as<uint8_t>(),
                           c->cand_rec.as<float4>(), c->cand_cls.as<uint8_t>());
        hipLaunchKernelGGL(k_cand_rows<false>, grid, blk, 0, s, n, q, c->export_d_off.as<uint32_t>(), c->export_d_idx.as<uint32_t>(), c->export_tot,
                           c->cand_rec.as<float4>(), c->cand_cls.as<uint8_t>(), c->cand_cnt.as<uint32_t>(), (const uint32_t*)nullptr, (uint32_t*)nullptr);
        device_exclusive_scan_u32(s, c->cand_cnt.as<uint32_t>(), out_off, n, c->cand_scan.as<uint32_t>(), out_off + n);
    }
    *tot = 0;
    HIPCHK(c, hipMemcpyAsync(tot, out_off + n, 4, hipMemcpyDeviceToHost, s));
    if (offsets_host) HIPCHK(c, hipMemcpyAsync(offsets_host, out_off, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

int cand_fill_rows(sph_ctx* c, const CandP& q, uint32_t tot)
{
    const uint32_t n = (uint32_t)c->n;
    hipStream_t s = c->stream;
    HIPCHK(c, c->cand_idx.ensure((size_t)tot * 4));
    ProfScope ps(&c->prof, "candidates_fill", s);
    hipLaunchKernelGGL(k_cand_rows<true>, dim3((n + 255) / 256), dim3(256), 0, s, n, q, c->export_d_off.as<uint32_t>(), c->export_d_idx.as<uint32_t>(), c->export_tot,
                       c->cand_rec.as<float4>(), c->cand_cls.as<uint8_t>(), (uint32_t*)nullptr, (const uint32_t*)c->cand_off.as<uint32_t>(),
                       c->cand_idx.as<uint32_t>());
    return SPH_OK;
}

extern "C" int sph_download_partner_candidates(sph_ctx* c, int kind, const sph_params* p, const sph_adapt_params* ap, uint32_t* offsets, uint32_t* indices,
                                               uint64_t cap, uint64_t* n_indices)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (n_indices) *n_indices = 0;
    if (int rc = cand_check_args(c, "sph_download_partner_candidates", kind, p, ap)) return rc;
    if (int rc = cand_refuse_common(c, "sph_download_partner_candidates")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = cand_need_lists(c)) return rc;
    if (c->n == 0) {
        if (offsets) offsets[0] = 0;
        return SPH_OK;
    }
    const CandP q = cand_params(kind, ap);
    uint32_t tot = 0;
    if (int rc = cand_count_rows(c, q, offsets, &tot)) return rc;
    if (n_indices) *n_indices = tot;
    if (!indices) return SPH_OK;
    if (cap < tot) return c->fail(SPH_ERR_INVALID_ARGUMENT, "indices buffer too small");
    if (tot == 0) return SPH_OK;
    if (int rc = cand_fill_rows(c, q, tot)) return rc;
    HIPCHK(c, hipMemcpyAsync(indices, c->cand_idx.p, (size_t)tot * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

// ---- sum of the masses in f64, fixed order: SUM_BLOCKS x 256 strided partial sums, a tree in LDS per block, one block over the partials
#define SUM_BLOCKS 1024

__device__ __forceinline__ double block_sum_f64(double v)
{
    __shared__ double s_v[256];
    s_v[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_v[threadIdx.x] += s_v[threadIdx.x + o];
        __syncthreads();
    }
    return s_v[0];
}

// (owned: a slab context's ownership bytes -- a ghost slot adds 0.0, the tree stays the same; nullptr on a plain context)
__global__ __launch_bounds__(256) void k_sum_mass(uint32_t n, const float4* __restrict__ pm, const uint8_t* __restrict__ owned, double* __restrict__ partials)
{
    double v = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)SUM_BLOCKS * 256)
        if (!owned || owned[i]) v += (double)pm[i].z;
    const double t = block_sum_f64(v);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_sum_mass_final(const double* __restrict__ partials, double* __restrict__ out)
{
    double v = 0.0;
    for (int k = threadIdx.x; k < SUM_BLOCKS; k += 256) v += partials[k];
    const double t = block_sum_f64(v);
    if (threadIdx.x == 0) *out = t;
}

int cand_sum_mass(sph_ctx* c, uint32_t n, const uint8_t* owned, double* total)
{
    *total = 0.0;
    if (n == 0) return SPH_OK;
    hipStream_t s = c->stream;
    HIPCHK(c, c->cand_red.ensure((SUM_BLOCKS + 1) * sizeof(double)));
    double* d = c->cand_red.as<double>();
    {
        ProfScope ps(&c->prof, "sum_mass", s);
        hipLaunchKernelGGL(k_sum_mass, dim3(SUM_BLOCKS), dim3(256), 0, s, n, c->pm[c->pcur].as<float4>(), owned, d);
        hipLaunchKernelGGL(k_sum_mass_final, dim3(1), dim3(256), 0, s, (const double*)d, d + SUM_BLOCKS);
    }
    HIPCHK(c, hipMemcpyAsync(total, d + SUM_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

extern "C" int sph_sum_mass(sph_ctx* c, double* total)
{
    if (!c || !total) return SPH_ERR_INVALID_ARGUMENT;
    *total = 0.0;
    if (int rc = cand_refuse_common(c, "sph_sum_mass")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return cand_sum_mass(c, (uint32_t)c->n, nullptr, total);
}
