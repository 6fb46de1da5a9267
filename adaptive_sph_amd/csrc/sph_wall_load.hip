// Wall loads (include/sph_wall_load.h): per boundary element the force, the torque, the normal force and the peak pressure the fluid
// puts on it, as 128-bit fixed-point integers and a 64-bit key, with an optional binned profile of the normal force along a plane.  The
// shape is the ledger's (sph_ledger.hip): a range pass, a verdict on the host, a sum pass; every term is stated in sph_wall_load.h and
// evaluated in that order (-ffp-contract=off), and integer addition, minimum and maximum are associative and commutative, so
// tests/wall_load_reference.py reproduces every word bit for bit whatever the device order or the launch shape.
//
// Kernels (on the context's stream; they read the state and write only the wall load's three buffers):
//   k_wall_range         grid-stride over the slots, at most kMaxBlocks blocks.  A lane checks its particle, then tests d < 1 against all E
//                        elements; a WAVE WITHOUT ANY ENTRY GOES ON TO ITS NEXT PARTICLES before any f64 work (most particles are nowhere
//                        near a wall).  The 66 words of sph_wall_load_words live in registers, fold by shuffles in the wave and through
//                        LDS in the block; ONE PARTIAL per block and word, stored plainly at part[word][block]
//   k_wall_fold_words    one wave per word: the partials of all blocks -> the word
//   k_wall_sums          the same shape over the E x 4 sums: (int64) trunc(t * 2^(60 - e)) added with carry per thread, per wave, per
//                        block; the profile's terms go to global memory with a 64-bit integer atomic each (few particles have one)
//   k_wall_fold_sums     one wave per sum: 128-bit addition of the partials
// No floating-point atomic anywhere.  Each pass reads 28 bytes per particle (pm 16, id 4, density 4, pressure 4).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "sph_context.hpp"
#include "sph_fixed_sums.hpp"
#include "sph_wall_load.h"
#include "sph_wall_load_internal.hpp"

static_assert(sizeof(sph_wall_load_spec) == 232 && sizeof(sph_wall_load_element_words) == 64 && sizeof(sph_wall_load_words) == 528, "the sizes sph_wall_load.h states");
static_assert(sizeof(sph_wall_load_element) == 152 && sizeof(sph_wall_load_result) == 1232, "the sizes sph_wall_load.h states");
static_assert(SPH_WALL_LOAD_MAX_ELEMENTS == SPH_MAX_PLANES, "one element per SDF");

namespace {

constexpr int kEl = SPH_WALL_LOAD_MAX_ELEMENTS, kS = SPH_WALL_LOAD_N_SUMS;
constexpr int kElWords = 8, kWords = 2 + kEl * kElWords;   // sph_wall_load_words as 66 u64, in its order
constexpr int kSums = kEl * kS;
constexpr uint32_t kMaxBlocks = 1024;   // blocks of a streaming pass at most (the rest of the slots by grid stride)
constexpr int kFoldWidth = 64;          // lanes of a fold launch: more than kFoldWidth blocks give a lane more than one partial
constexpr size_t kOutSums = 1024;       // wl_out: the 66 words, then (at this byte) the 32 sums
static_assert(sizeof(sph_wall_load_words) == kWords * 8 && kWords * 8 <= (int)kOutSums, "the words are 66 u64");
static_assert(sizeof(U128) == sizeof(sph_ledger_sum) && offsetof(U128, hi) == offsetof(sph_ledger_sum, hi), "a partial is a sph_ledger_sum");

enum { BAD_M = 1, BAD_X, BAD_Y, BAD_H, BAD_RHO, BAD_P, BAD_RHO_SIGN, BAD_H_SIGN, BAD_TERM = 16 /* + 4 k + s */ };
enum { OP_MIN, OP_ADD, OP_MAX };
enum { W_ENTRIES = 0, W_WET, W_UNBINNED, W_BITS /* .. + 3 */, W_KEY = 7 };

// how word q of sph_wall_load_words folds: the first offender by minimum, the counts by addition, max |t| and the key by maximum
__host__ __device__ inline int word_op(int q)
{
    if (q == 0) return OP_MIN;
    if (q == 1) return OP_ADD;
    return ((q - 2) & (kElWords - 1)) < W_BITS ? OP_ADD : OP_MAX;
}
__host__ __device__ inline unsigned long long word_empty(int q) { return word_op(q) == OP_MIN ? ~0ull : 0ull; }
__host__ __device__ inline unsigned long long word_fold(int q, unsigned long long a, unsigned long long b)
{
    const int op = word_op(q);
    return op == OP_ADD ? a + b : op == OP_MIN ? (a < b ? a : b) : (a > b ? a : b);
}

// the state and the constants a pass reads (device order)
struct WallIn {
    const float4* pm;      // {x, y, mass, h}
    const uint32_t* orig;  // device slot -> reference index
    const float *rho, *pres;
    const BoundaryP* bnd;
    const float *lam_lut, *dlam_lut;
    int n_el, penalty, symmetric;
    float rest_density, sdf_eps;
    int n_bins[kEl];       // B per element (0: no profile)
    float s_lo[kEl], inv_ds[kEl];
    double limit[kSums];   // range pass: 2^e, or +inf while the exponent is still to be taken from this pass
    double scale[kSums];   // sum pass: 2^(60 - e)
    double bin_scale[kEl]; // sum pass: 2^(40 - e_NORMAL)
};

// the elements particle (x, y, h) has d < 1 at, as a bit set; d[k] for those
__device__ __forceinline__ uint32_t near_elements(const WallIn& a, float x, float y, float sr, float* d)
{
    uint32_t near = 0;
#pragma unroll
    for (int k = 0; k < kEl; k++) {
        d[k] = 0.f;
        if (k < a.n_el) {
            d[k] = sdf_probe(a.bnd, k, x, y) / sr;
            if (d[k] < 1.f) near |= 1u << k;
        }
    }
    return near;
}

// the profile's bin of an entry of element k at (x, y): -1 where it is not binned
__device__ __forceinline__ int wall_bin(const WallIn& a, int k, float x, float y)
{
    const PlaneP pl = a.bnd->planes[k];
    const float s = (-pl.dy * x) + (pl.dx * y);
    const float fb = floorf((s - a.s_lo[k]) * a.inv_ds[k]);
    return (fb >= 0.f && fb < (float)a.n_bins[k]) ? (int)fb : -1;
}

// n: the slots; part: kWords rows of gridDim.x partials
__global__ __launch_bounds__(256) void k_wall_range(uint32_t n, WallIn a, unsigned long long* __restrict__ part)
{
    __shared__ unsigned long long s_w[4][kWords];
    unsigned long long w[kWords];
#pragma unroll
    for (int q = 0; q < kWords; q++) w[q] = word_empty(q);
    // every lane of a wave runs the same number of rounds (__any below)
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256; base < (size_t)n; base += stride) {
        const size_t i = base + threadIdx.x;
        const bool live = i < (size_t)n;
        float x = 0.f, y = 0.f, m = 0.f, h = 1.f, rho = 1.f, p = 0.f;
        uint32_t id = 0, bad = 0, near = 0;
        float d[kEl];
        if (live) {
            const float4 A = a.pm[i];
            id = a.orig[i];
            x = A.x, y = A.y, m = A.z, h = A.w;
            rho = a.rho[i];
            p = a.pres[i];
            w[1] += 1ull;
            if (!finite_f32(m)) bad = BAD_M;
            else if (!finite_f32(x)) bad = BAD_X;
            else if (!finite_f32(y)) bad = BAD_Y;
            else if (!finite_f32(h)) bad = BAD_H;
            else if (!finite_f32(rho)) bad = BAD_RHO;
            else if (!finite_f32(p)) bad = BAD_P;
            else if (!(rho > 0.f)) bad = BAD_RHO_SIGN;
            else if (!(h > 0.f)) bad = BAD_H_SIGN;
        }
        const float sr = h * 2.f;
        if (live && !bad) near = near_elements(a, x, y, sr, d);
        if (live && bad) {
            const unsigned long long key = ((unsigned long long)id << 8) | bad;
            w[0] = key < w[0] ? key : w[0];
        }
        if (!__any(near != 0)) continue;   // wave-uniform: nobody here is near a wall
        if (!near) continue;
        const float c = wall_coefficient(p, rho, a.rest_density, a.symmetric != 0);
        // first the verdict on every term of the particle (an offender adds to nothing), then its words
        double t[kEl][kS];
        uint32_t has = 0;
#pragma unroll
        for (int k = 0; k < kEl; k++) {
            if (!((near >> k) & 1u)) continue;
            WallEntry e;
            if (!wall_entry(a.bnd, k, x, y, sr, d[k], a.sdf_eps, a.penalty, a.lam_lut, a.dlam_lut, e)) continue;
            has |= 1u << k;
            wall_terms(m, c, x, y, e, t[k]);
        }
#pragma unroll
        for (int k = kEl - 1; k >= 0; k--) {   // (downwards: the smallest failing (k, s) is assigned last)
            if (!((has >> k) & 1u)) continue;
#pragma unroll
            for (int s = kS - 1; s >= 0; s--)
                if (!(fabs(t[k][s]) < a.limit[k * kS + s])) bad = BAD_TERM + (uint32_t)(k * kS + s);   // (inf and NaN fail against +inf too)
        }
        if (bad) {
            const unsigned long long key = ((unsigned long long)id << 8) | bad;
            w[0] = key < w[0] ? key : w[0];
            continue;
        }
#pragma unroll
        for (int k = 0; k < kEl; k++) {
            if (!((has >> k) & 1u)) continue;
            unsigned long long* e = &w[2 + k * kElWords];
            e[W_ENTRIES] += 1ull;
            if (p > 0.f) e[W_WET] += 1ull;
            if (a.n_bins[k] > 0 && wall_bin(a, k, x, y) < 0) e[W_UNBINNED] += 1ull;
#pragma unroll
            for (int s = 0; s < kS; s++) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(t[k][s]));
                e[W_BITS + s] = b > e[W_BITS + s] ? b : e[W_BITS + s];
            }
            key_max(e[W_KEY], p, id);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kWords; q++) {
        unsigned long long v = w[q];
        for (int o = 32; o > 0; o >>= 1) v = word_fold(q, v, shfl_xor_u64(v, o));
        if (lane == 0) s_w[wave][q] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < kWords) {
        const int q = threadIdx.x;
        const unsigned long long v = word_fold(q, word_fold(q, s_w[0][q], s_w[1][q]), word_fold(q, s_w[2][q], s_w[3][q]));
        part[(size_t)q * gridDim.x + blockIdx.x] = v;
    }
}

// one wave per word (blockIdx.x): the nb partials of its row -> out[word]
__global__ __launch_bounds__(kFoldWidth) void k_wall_fold_words(uint32_t nb, const unsigned long long* __restrict__ part, unsigned long long* __restrict__ out)
{
    const int q = blockIdx.x;
    unsigned long long v = word_empty(q);
    for (uint32_t b = threadIdx.x; b < nb; b += kFoldWidth) v = word_fold(q, v, part[(size_t)q * nb + b]);
    for (int o = 32; o > 0; o >>= 1) v = word_fold(q, v, shfl_xor_u64(v, o));
    if (threadIdx.x == 0) out[q] = v;
}

// n: the slots; part: kSums rows of gridDim.x partials; profile: n_el rows of `bins` words (nullptr: no bins), cleared before the launch.
// Checks nothing: the range pass and its verdict come first
__global__ __launch_bounds__(256) void k_wall_sums(uint32_t n, WallIn a, U128* __restrict__ part, unsigned long long* __restrict__ profile, int bins)
{
    __shared__ U128 s_q[4][kSums];
    U128 acc[kSums];
#pragma unroll
    for (int s = 0; s < kSums; s++) acc[s] = U128{0ull, 0ll};
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256; base < (size_t)n; base += stride) {
        const size_t i = base + threadIdx.x;
        float x = 0.f, y = 0.f, m = 0.f, sr = 1.f;
        uint32_t near = 0;
        float d[kEl];
        if (i < (size_t)n) {
            const float4 A = a.pm[i];
            x = A.x, y = A.y, m = A.z;
            sr = A.w * 2.f;
            near = near_elements(a, x, y, sr, d);
        }
        if (!__any(near != 0)) continue;   // wave-uniform
        if (!near) continue;
        const float c = wall_coefficient(a.pres[i], a.rho[i], a.rest_density, a.symmetric != 0);
#pragma unroll
        for (int k = 0; k < kEl; k++) {
            if (!((near >> k) & 1u)) continue;
            WallEntry e;
            if (!wall_entry(a.bnd, k, x, y, sr, d[k], a.sdf_eps, a.penalty, a.lam_lut, a.dlam_lut, e)) continue;
            double t[kS];
            wall_terms(m, c, x, y, e, t);
#pragma unroll
            for (int s = 0; s < kS; s++) {
                const long long q = (long long)(t[s] * a.scale[k * kS + s]);   // trunc; |t * scale| < 2^60 by the range pass's verdict
                add128(acc[k * kS + s], (unsigned long long)q, q >> 63);
            }
            if (profile && a.n_bins[k] > 0) {
                const int b = wall_bin(a, k, x, y);   // 0 <= b < n_bins[k] <= bins, or -1
                if (b >= 0) {
                    const long long q = (long long)(t[SPH_WALL_LOAD_NORMAL] * a.bin_scale[k]);   // below 2^40 in magnitude
                    atomicAdd(&profile[(size_t)k * (size_t)bins + (size_t)b], (unsigned long long)q);   // (two's complement: the signed sum)
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < kSums; s++) {
        const U128 v = wave_add128(acc[s]);
        if (lane == 0) s_q[wave][s] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < kSums) {
        const int s = threadIdx.x;
        U128 v = s_q[0][s];
        for (int k = 1; k < 4; k++) add128(v, s_q[k][s].lo, s_q[k][s].hi);
        part[(size_t)s * gridDim.x + blockIdx.x] = v;
    }
}

// one wave per sum (blockIdx.x): the nb partials of its row -> out[sum]
__global__ __launch_bounds__(kFoldWidth) void k_wall_fold_sums(uint32_t nb, const U128* __restrict__ part, U128* __restrict__ out)
{
    const int s = blockIdx.x;
    U128 v{0ull, 0ll};
    for (uint32_t b = threadIdx.x; b < nb; b += kFoldWidth) {
        const U128 p = part[(size_t)s * nb + b];
        add128(v, p.lo, p.hi);
    }
    v = wave_add128(v);
    if (threadIdx.x == 0) out[s] = v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
const char* const kSumName[kS] = {"force_x", "force_y", "torque", "normal"};
const char* const kInputName[6] = {"mass", "x", "y", "smoothing length", "density", "pressure"};
const char* const kWho = "sph_wall_load_compute";

// the sentence of a refused particle: `first_bad` as the range pass left it (not all ones)
void format_offender(char* buf, size_t bytes, unsigned long long first_bad, const sph_wall_load_spec* spec)
{
    const unsigned long long id = first_bad >> 8;
    const int why = (int)(first_bad & 0xffu);
    if (why >= BAD_M && why <= BAD_P) snprintf(buf, bytes, "wall load: the %s is not finite (particle i=%llu)", kInputName[why - BAD_M], id);
    else if (why == BAD_RHO_SIGN)
        snprintf(buf, bytes, "wall load: the density is not positive (particle i=%llu; before the first step the density is 0: the load exists behind sph_step)", id);
    else if (why == BAD_H_SIGN) snprintf(buf, bytes, "wall load: the smoothing length is not positive (particle i=%llu)", id);
    else {
        const int q = std::min(std::max(why - BAD_TERM, 0), kSums - 1), k = q / kS, s = q % kS;
        const int e = spec->exponent[k][s];
        if (e == SPH_LEDGER_AUTO_EXPONENT) snprintf(buf, bytes, "wall load: the term of sum %d (%s) at element %d is not finite (particle i=%llu)", s, kSumName[s], k, id);
        else
            snprintf(buf, bytes, "wall load: the term of sum %d (%s) at element %d is not finite or not below 2^exponent = 2^%d (particle i=%llu)", s, kSumName[s], k, e,
                     id);
    }
}

int ensure_buffers(sph_ctx* c, size_t profile_bytes)
{
    HIPCHK(c, c->wl_part.ensure((size_t)kMaxBlocks * std::max((size_t)kWords * 8, (size_t)kSums * sizeof(U128))));
    HIPCHK(c, c->wl_out.ensure(kOutSums + (size_t)kSums * sizeof(U128)));
    if (profile_bytes) HIPCHK(c, c->wl_profile.ensure(profile_bytes));
    return SPH_OK;
}

}  // namespace

extern "C" int sph_wall_load_compute(sph_ctx* c, const sph_params* p, const sph_wall_load_spec* spec, sph_wall_load_result* out, int64_t* profile)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: null output", kWho);
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: null parameters", kWho);
    if (!spec) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: null wall-load spec", kWho);
    if (c->dist.on)
        return c->fail(SPH_ERR_UNSUPPORTED, "%s: slab contexts are not supported (one rank holds a slab of the particles; the words fold and the integers add, but "
                                            "no range / fold / sums / compose is stated for wall loads yet)", kWho);
    if (c->poisoned) return c->refuse_poisoned();
    if (spec->flags != 0) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: flags = 0x%x has unknown bits (0)", kWho, spec->flags);
    const int bins = spec->bins, E = c->n_planes;
    if (bins < 0 || bins > SPH_WALL_LOAD_MAX_BINS) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: bins = %d (0, or 1..%d)", kWho, bins, SPH_WALL_LOAD_MAX_BINS);
    if (bins > 0 && !profile) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: null profile with bins = %d", kWho, bins);
    if (bins > 0 && c->bnd_h.poly_n > 0)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: bins on a polygon boundary (a profile runs along a plane; the polygon is one element without a direction)", kWho);
    float inv_ds[kEl] = {};
    for (int k = 0; k < E; k++) {
        for (int s = 0; s < kS; s++) {
            const int e = spec->exponent[k][s];
            if (e != SPH_LEDGER_AUTO_EXPONENT && (e < SPH_LEDGER_MIN_EXPONENT || e > SPH_LEDGER_MAX_EXPONENT))
                return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: sum %d (%s) at element %d: exponent %d (%d..%d, or SPH_LEDGER_AUTO_EXPONENT)", kWho, s, kSumName[s], k, e,
                               SPH_LEDGER_MIN_EXPONENT, SPH_LEDGER_MAX_EXPONENT);
        }
        if (bins == 0) continue;
        const int B = spec->n_bins[k];
        if (B < 0 || B > bins) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: element %d: n_bins = %d (0..bins = %d)", kWho, k, B, bins);
        if (B == 0) continue;
        const float lo = spec->s_lo[k], hi = spec->s_hi[k];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo))
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: element %d: the profile's range [%g, %g) is empty or not finite (s_hi > s_lo)", kWho, k, (double)lo, (double)hi);
        inv_ds[k] = (float)B / (hi - lo);
        if (!std::isfinite(inv_ds[k])) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: element %d: bins per length (float)n_bins / (s_hi - s_lo) is not finite", kWho, k);
    }
    memset(out, 0, sizeof *out);
    if (profile && bins > 0 && E > 0) memset(profile, 0, (size_t)E * (size_t)bins * sizeof(int64_t));
    if (E == 0) return SPH_OK;   // no boundary: nothing is read

    HIPCHK(c, hipSetDevice(c->device));
    const size_t profile_bytes = (size_t)E * (size_t)bins * sizeof(int64_t);
    if (int rc = ensure_buffers(c, profile_bytes)) return rc;
    hipStream_t st = c->stream;
    const uint32_t n = (uint32_t)c->n, nb = std::min(std::max((n + 255u) / 256u, 1u), kMaxBlocks);
    WallIn a{};
    a.pm = c->pm[c->pcur].as<float4>();
    a.orig = c->orig[c->cur].as<uint32_t>();
    a.rho = c->rho.as<float>();
    a.pres = (c->pressure_cur ? c->p1 : c->p0).as<float>();
    a.bnd = c->planes_d.as<BoundaryP>();
    a.lam_lut = c->lam_lut.as<float>();
    a.dlam_lut = c->dlam_lut.as<float>();
    a.n_el = E;
    a.penalty = p->boundary_penalty_term;
    a.symmetric = p->operator_discretization == SPH_OP_SYMMETRIC_GRADIENT;
    a.rest_density = p->rest_density;
    a.sdf_eps = p->sdf_gradient_eps;
    for (int k = 0; k < kEl; k++) {
        a.n_bins[k] = (k < E && bins > 0) ? spec->n_bins[k] : 0;
        a.s_lo[k] = a.n_bins[k] > 0 ? spec->s_lo[k] : 0.f;
        a.inv_ds[k] = inv_ds[k];
        a.bin_scale[k] = 1.0;
        for (int s = 0; s < kS; s++) {
            const int e = spec->exponent[k][s];
            a.limit[k * kS + s] = (k < E && e != SPH_LEDGER_AUTO_EXPONENT) ? std::ldexp(1.0, e) : (double)INFINITY;
            a.scale[k * kS + s] = 1.0;
        }
    }
    // ---- the range pass
    sph_wall_load_words words;
    {
        ProfScope ps(&c->prof, "wall_load_range", st);
        hipLaunchKernelGGL(k_wall_range, dim3(nb), dim3(256), 0, st, n, a, c->wl_part.as<unsigned long long>());
        hipLaunchKernelGGL(k_wall_fold_words, dim3(kWords), dim3(kFoldWidth), 0, st, nb, c->wl_part.as<unsigned long long>(), c->wl_out.as<unsigned long long>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&words, c->wl_out.p, sizeof words, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // ---- the verdict
    char msg[400];
    if (words.first_bad != SPH_LEDGER_NO_OFFENDER) {
        format_offender(msg, sizeof msg, words.first_bad, spec);
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s", msg);
    }
    int used[kEl][kS] = {};
    for (int k = 0; k < E; k++) {
        const sph_wall_load_element_words& w = words.element[k];
        for (int s = 0; s < kS; s++) {
            int e = spec->exponent[k][s];
            if (e == SPH_LEDGER_AUTO_EXPONENT) {
                e = std::max(exponent_of_bits(w.max_bits[s]), SPH_LEDGER_MIN_EXPONENT);
                if (e > SPH_LEDGER_MAX_EXPONENT)
                    return c->fail(SPH_ERR_INVALID_ARGUMENT, "wall load: sum %d (%s) at element %d needs the exponent %d (at most %d)", s, kSumName[s], k, e,
                                   SPH_LEDGER_MAX_EXPONENT);
            }
            used[k][s] = e;
            a.scale[k * kS + s] = std::ldexp(1.0, 60 - e);
        }
        a.bin_scale[k] = std::ldexp(1.0, SPH_WALL_LOAD_BIN_SHIFT - used[k][SPH_WALL_LOAD_NORMAL]);
        if (a.n_bins[k] > 0 && w.n_entries >= (uint64_t)SPH_WALL_LOAD_MAX_BINNED_ENTRIES)
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "wall load: element %d has %llu entries: with bins fewer than 2^23 = %d (the profile's 64-bit words hold that many "
                                                     "terms below 2^40)", k, (unsigned long long)w.n_entries, SPH_WALL_LOAD_MAX_BINNED_ENTRIES);
    }
    // ---- the sum pass
    sph_ledger_sum sums[kSums];
    U128* dst = (U128*)((char*)c->wl_out.p + kOutSums);
    unsigned long long* prof_d = bins > 0 ? c->wl_profile.as<unsigned long long>() : nullptr;
    if (prof_d) HIPCHK(c, hipMemsetAsync(prof_d, 0, profile_bytes, st));
    {
        ProfScope ps(&c->prof, "wall_load_sums", st);
        hipLaunchKernelGGL(k_wall_sums, dim3(nb), dim3(256), 0, st, n, a, c->wl_part.as<U128>(), prof_d, bins);
        hipLaunchKernelGGL(k_wall_fold_sums, dim3(kSums), dim3(kFoldWidth), 0, st, nb, c->wl_part.as<U128>(), dst);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sums, dst, sizeof sums, hipMemcpyDeviceToHost, st));
    if (prof_d) HIPCHK(c, hipMemcpyAsync(profile, prof_d, profile_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // ---- the result
    out->n_elements = (uint32_t)E;
    out->bins = bins;
    out->n = words.n;
    for (int k = 0; k < E; k++) {
        sph_wall_load_element& el = out->element[k];
        const sph_wall_load_element_words& w = words.element[k];
        for (int s = 0; s < kS; s++) {
            el.exponent[s] = used[k][s];
            el.raw[s] = sums[k * kS + s];
            el.sum[s] = resolve128(el.raw[s], used[k][s] - 60);
        }
        el.n_entries = w.n_entries;
        el.n_wet = w.n_wet;
        el.n_unbinned = w.n_unbinned;
        el.max_pressure = unpack_max_key(w.max_pressure);
        el.inv_ds = inv_ds[k];
        el.n_bins = a.n_bins[k];
    }
    return SPH_OK;
}
