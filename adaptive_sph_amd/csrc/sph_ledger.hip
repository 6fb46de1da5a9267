// The state ledger (include/sph_ledger.h): conserved quantities as 128-bit fixed-point integers, extremes as 64-bit keys that carry the
// particle's id, counts, and the refusal that names the smallest offending id -- of one context, of a slab rank, and composed over
// ranks on the host.  The terms are stated in sph_ledger.h; every operation here is one IEEE operation in that order (the library is
// compiled with -ffp-contract=off, `/` is correctly rounded), and integer addition, minimum and maximum are associative and
// commutative, so tests/ledger_reference.py reproduces every word bit for bit whatever the device order, the launch shape or the cuts.
//
// Kernels (on the context's stream; they read the state and write only the ledger's two buffers):
//   k_ledger_range<SLAB>    grid-stride over the slots, at most kMaxBlocks blocks: each thread keeps the 25 words of sph_ledger_words in
//                           registers (first offender, counts, max |t| as f64 bits, the 13 keys), folds them over its particles, the
//                           wave folds them with shuffles (64-bit words as two 32-bit halves), the block through LDS; ONE PARTIAL per
//                           block and word, stored plainly at part[word][block] -- no atomic, nothing to clear before the launch
//   k_ledger_fold_words     one wave per word: the partials of all blocks -> the word
//   k_ledger_sums<SLAB>     the same shape over the nine 128-bit sums: (int64) trunc(t * 2^(60 - e)) added with carry per thread, per
//                           wave, per block; one 16-byte partial per block and sum
//   k_ledger_fold_sums      one wave per sum: 128-bit addition of the partials
// <SLAB>: a slot takes part only where `owned` says so (nullptr: every slot), as in k_sample_range.
// No word is contended: a launch of 1024 blocks adding to ONE word would queue 1024 atomics behind each other (one word takes about 88
// atomics per microsecond, sph_sample_internal.hpp) -- 12 us, half of what the range pass over a million particles takes (profiles/r17_ledger.md).
// Each pass reads at most 36 bytes per particle (pm 16, velocity 8, id 4, density 4, pressure 4) and one ownership byte on slabs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sph_fixed_sums.hpp"
#include "sph_ledger.h"
#include "sph_slab_layers.hpp"

static_assert(sizeof(sph_ledger_spec) == 40 && sizeof(sph_ledger_sum) == 16 && sizeof(sph_ledger_extreme) == 8, "the sizes sph_ledger.h states");
static_assert(sizeof(sph_ledger_words) == 200 && sizeof(sph_ledger_result) == 376, "the sizes sph_ledger.h states");

namespace {

constexpr int kSums = SPH_LEDGER_N_SUMS, kExt = SPH_LEDGER_N_EXTREMES;
constexpr int kWords = 3 + kSums + kExt;   // sph_ledger_words as 25 u64, in its order
constexpr int kFirstBits = 3, kFirstKey = 3 + kSums;
// blocks of a streaming pass at most (the rest of the slots by grid stride).  -DSPH_LEDGER_MAX_BLOCKS=<k> builds the comparison forms of
// profiles/r17_ledger.md (scripts/gpu_ledger_time.py with SPH_HIP_LIBRARY)
#ifndef SPH_LEDGER_MAX_BLOCKS
#define SPH_LEDGER_MAX_BLOCKS 1024
#endif
constexpr uint32_t kMaxBlocks = SPH_LEDGER_MAX_BLOCKS;
constexpr uint32_t kAllBits = SPH_LEDGER_CARRIED | SPH_LEDGER_STEP_OUTPUTS | SPH_LEDGER_OUTSIDE;
constexpr size_t kOutSums = 256;           // led_out: the 25 words, then (at this byte) the nine sums
static_assert(sizeof(sph_ledger_words) == kWords * 8 && kWords * 8 <= (int)kOutSums, "the words are 25 u64");

enum { BAD_M = 1, BAD_X, BAD_Y, BAD_VX, BAD_VY, BAD_RHO, BAD_P, BAD_H, BAD_SPEED2, BAD_RHO_SIGN, BAD_TERM = 16 /* + s */ };
enum { OP_MIN, OP_ADD, OP_MAX };

__host__ __device__ inline uint32_t sum_mask(uint32_t what) { return ((what & SPH_LEDGER_CARRIED) ? 0x7fu : 0u) | ((what & SPH_LEDGER_STEP_OUTPUTS) ? 0x180u : 0u); }
__host__ __device__ inline uint32_t extreme_mask(uint32_t what) { return ((what & SPH_LEDGER_CARRIED) ? 0x7fu : 0u) | ((what & SPH_LEDGER_STEP_OUTPUTS) ? 0x1f80u : 0u); }
// how word q of sph_ledger_words folds: the first offender by minimum, the counts by addition, max |t| by maximum, key k by maximum
// (k = 0 and every even k) or minimum (every odd k)
__host__ __device__ inline int word_op(int q)
{
    if (q == 0) return OP_MIN;
    if (q < kFirstBits) return OP_ADD;
    if (q < kFirstKey) return OP_MAX;
    return ((q - kFirstKey) & 1) ? OP_MIN : OP_MAX;
}
__host__ __device__ inline unsigned long long word_empty(int q) { return word_op(q) == OP_MIN ? ~0ull : 0ull; }
__host__ __device__ inline unsigned long long word_fold(int q, unsigned long long a, unsigned long long b)
{
    const int op = word_op(q);
    return op == OP_ADD ? a + b : op == OP_MIN ? (a < b ? a : b) : (a > b ? a : b);
}

// the state a pass reads (device order)
struct LedgerIn {
    const float4* pm;      // {x, y, mass, h}
    const float2* vel;
    const uint32_t* orig;  // device slot -> reference index (a slab context: the global particle id)
    const float *rho, *pres;
    const BoundaryP* bnd;
    int n_planes;
    uint32_t what;
    float rest_density;
    double limit[kSums];   // range pass: 2^e_s, or +inf while the exponent is still to be taken from this pass
    double scale[kSums];   // sum pass: 2^(60 - e_s); 1 for a sum that is not asked for (its term is 0)
};

// sph_ledger.h's terms; 0 for a sum whose group is not asked for
__device__ __forceinline__ void ledger_terms(uint32_t what, float x, float y, float m, float vx, float vy, float rho, float rest, double* t)
{
    const double M = (double)m;
    if (what & SPH_LEDGER_CARRIED) {
        const double X = (double)x, Y = (double)y, VX = (double)vx, VY = (double)vy;
        t[0] = M;
        t[1] = M * VX;
        t[2] = M * VY;
        t[3] = M * X;
        t[4] = M * Y;
        t[5] = 0.5 * (M * (VX * VX + VY * VY));
        t[6] = M * (X * VY - Y * VX);
    } else {
        for (int s = 0; s < 7; s++) t[s] = 0.0;
    }
    if (what & SPH_LEDGER_STEP_OUTPUTS) {
        t[7] = M / (double)rho;
        const double d = (double)rho - (double)rest;
        t[8] = d > 0.0 ? d : 0.0;
    } else {
        t[7] = t[8] = 0.0;
    }
}

// n: the slots; part: kWords rows of gridDim.x partials
template <bool SLAB>
__global__ __launch_bounds__(256) void k_ledger_range(uint32_t n, LedgerIn a, const uint8_t* __restrict__ owned, unsigned long long* __restrict__ part)
{
    __shared__ unsigned long long s_w[4][kWords];
    unsigned long long w[kWords];
#pragma unroll
    for (int q = 0; q < kWords; q++) w[q] = word_empty(q);
    const bool carried = a.what & SPH_LEDGER_CARRIED, step = a.what & SPH_LEDGER_STEP_OUTPUTS, outside = a.what & SPH_LEDGER_OUTSIDE;
    const uint32_t asked = sum_mask(a.what);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
        if (SLAB && owned && !owned[i]) continue;
        const float4 A = a.pm[i];
        const uint32_t id = a.orig[i];
        const float x = A.x, y = A.y, m = A.z, h = A.w;
        float vx = 0.f, vy = 0.f, rho = 0.f, p = 0.f;
        if (carried) {
            const float2 v = a.vel[i];
            vx = v.x;
            vy = v.y;
        }
        if (step) {
            rho = a.rho[i];
            p = a.pres[i];
        }
        w[1] += 1ull;
        const float speed2 = vx * vx + vy * vy;
        uint32_t bad = 0;
        if ((carried || step) && !finite_f32(m)) bad = BAD_M;
        else if ((carried || outside) && !finite_f32(x)) bad = BAD_X;
        else if ((carried || outside) && !finite_f32(y)) bad = BAD_Y;
        else if (carried && !finite_f32(vx)) bad = BAD_VX;
        else if (carried && !finite_f32(vy)) bad = BAD_VY;
        else if (step && !finite_f32(rho)) bad = BAD_RHO;
        else if (step && !finite_f32(p)) bad = BAD_P;
        else if (step && !finite_f32(h)) bad = BAD_H;
        else if (carried && !finite_f32(speed2)) bad = BAD_SPEED2;
        else if (step && !(rho > 0.f)) bad = BAD_RHO_SIGN;
        double t[kSums];
        ledger_terms(bad ? 0u : a.what, x, y, m, vx, vy, rho, a.rest_density, t);
        if (!bad) {
#pragma unroll
            for (int s = kSums - 1; s >= 0; s--)   // (downwards: the smallest failing s is assigned last)
                if (((asked >> s) & 1u) && !(fabs(t[s]) < a.limit[s])) bad = BAD_TERM + (uint32_t)s;   // (inf and NaN fail against +inf too)
        }
        if (bad) {
            const unsigned long long k = ((unsigned long long)id << 8) | bad;
            w[0] = k < w[0] ? k : w[0];
            continue;
        }
#pragma unroll
        for (int s = 0; s < kSums; s++) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(t[s]));
            w[kFirstBits + s] = b > w[kFirstBits + s] ? b : w[kFirstBits + s];
        }
        if (carried) {
            key_max(w[kFirstKey + SPH_LEDGER_MAX_SPEED2], speed2, id);
            key_min(w[kFirstKey + SPH_LEDGER_MIN_X], x, id);
            key_max(w[kFirstKey + SPH_LEDGER_MAX_X], x, id);
            key_min(w[kFirstKey + SPH_LEDGER_MIN_Y], y, id);
            key_max(w[kFirstKey + SPH_LEDGER_MAX_Y], y, id);
            key_min(w[kFirstKey + SPH_LEDGER_MIN_MASS], m, id);
            key_max(w[kFirstKey + SPH_LEDGER_MAX_MASS], m, id);
        }
        if (step) {
            key_min(w[kFirstKey + SPH_LEDGER_MIN_DENSITY], rho, id);
            key_max(w[kFirstKey + SPH_LEDGER_MAX_DENSITY], rho, id);
            key_min(w[kFirstKey + SPH_LEDGER_MIN_PRESSURE], p, id);
            key_max(w[kFirstKey + SPH_LEDGER_MAX_PRESSURE], p, id);
            key_min(w[kFirstKey + SPH_LEDGER_MIN_H], h, id);
            key_max(w[kFirstKey + SPH_LEDGER_MAX_H], h, id);
        }
        if (outside && a.n_planes > 0) {
            float dist = INFINITY;
            for (int k = 0; k < a.n_planes; k++) dist = fminf(dist, sdf_probe(a.bnd, k, x, y));
            if (dist < 0.f) w[2] += 1ull;
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
__global__ __launch_bounds__(64) void k_ledger_fold_words(uint32_t nb, const unsigned long long* __restrict__ part, unsigned long long* __restrict__ out)
{
    const int q = blockIdx.x;
    unsigned long long v = word_empty(q);
    for (uint32_t b = threadIdx.x; b < nb; b += 64) v = word_fold(q, v, part[(size_t)q * nb + b]);
    for (int o = 32; o > 0; o >>= 1) v = word_fold(q, v, shfl_xor_u64(v, o));
    if (threadIdx.x == 0) out[q] = v;
}

// n: the slots; part: kSums rows of gridDim.x partials.  Checks nothing: the range pass and its verdict come first
template <bool SLAB>
__global__ __launch_bounds__(256) void k_ledger_sums(uint32_t n, LedgerIn a, const uint8_t* __restrict__ owned, U128* __restrict__ part)
{
    __shared__ U128 s_q[4][kSums];
    U128 acc[kSums];
#pragma unroll
    for (int s = 0; s < kSums; s++) acc[s] = U128{0ull, 0ll};
    const bool carried = a.what & SPH_LEDGER_CARRIED, step = a.what & SPH_LEDGER_STEP_OUTPUTS;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
        if (SLAB && owned && !owned[i]) continue;
        const float4 A = a.pm[i];
        float vx = 0.f, vy = 0.f, rho = 0.f;
        if (carried) {
            const float2 v = a.vel[i];
            vx = v.x;
            vy = v.y;
        }
        if (step) rho = a.rho[i];
        double t[kSums];
        ledger_terms(a.what, A.x, A.y, A.z, vx, vy, rho, a.rest_density, t);
#pragma unroll
        for (int s = 0; s < kSums; s++) {
            const long long q = (long long)(t[s] * a.scale[s]);   // trunc; |t * scale| < 2^60 by the range pass's verdict
            add128(acc[s], (unsigned long long)q, q >> 63);
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
__global__ __launch_bounds__(64) void k_ledger_fold_sums(uint32_t nb, const U128* __restrict__ part, U128* __restrict__ out)
{
    const int s = blockIdx.x;
    U128 v{0ull, 0ll};
    for (uint32_t b = threadIdx.x; b < nb; b += 64) {
        const U128 p = part[(size_t)s * nb + b];
        add128(v, p.lo, p.hi);
    }
    v = wave_add128(v);
    if (threadIdx.x == 0) out[s] = v;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
const char* const kSumName[kSums] = {"mass", "momentum_x", "momentum_y", "moment_x", "moment_y", "kinetic", "angular", "volume", "compression"};
const char* const kInputName[8] = {"mass", "x", "y", "vx", "vy", "density", "pressure", "smoothing length"};

// what is wrong with a spec before any data is looked at (nullptr: nothing); the sentence goes to buf
const char* spec_fault(const sph_ledger_spec* spec, bool allow_auto, const char* who, char* buf, size_t bytes)
{
    if (!spec) {
        snprintf(buf, bytes, "%s: null ledger spec", who);
        return buf;
    }
    if (spec->what == 0 || (spec->what & ~kAllBits)) {
        snprintf(buf, bytes, "%s: what = 0x%x asks for nothing or for an unknown group (SPH_LEDGER_CARRIED | SPH_LEDGER_STEP_OUTPUTS | SPH_LEDGER_OUTSIDE)", who, spec->what);
        return buf;
    }
    const uint32_t asked = sum_mask(spec->what);
    for (int s = 0; s < kSums; s++) {
        if (!((asked >> s) & 1u)) continue;
        const int e = spec->exponent[s];
        if (e == SPH_LEDGER_AUTO_EXPONENT) {
            if (allow_auto) continue;
            snprintf(buf, bytes, "%s: sum %d (%s) has an automatic exponent (the range pass and sph_ledger_fold_words come first: every rank must sum with the "
                                 "exponents of the whole vector)", who, s, kSumName[s]);
            return buf;
        }
        if (e < SPH_LEDGER_MIN_EXPONENT || e > SPH_LEDGER_MAX_EXPONENT) {
            snprintf(buf, bytes, "%s: sum %d (%s): exponent %d (%d..%d, or SPH_LEDGER_AUTO_EXPONENT)", who, s, kSumName[s], e, SPH_LEDGER_MIN_EXPONENT,
                     SPH_LEDGER_MAX_EXPONENT);
            return buf;
        }
    }
    return nullptr;
}

// the sentence of a refused particle: `first_bad` as the range pass left it (not all ones)
void format_offender(char* buf, size_t bytes, unsigned long long first_bad, const sph_ledger_spec* spec)
{
    const unsigned long long id = first_bad >> 8;
    const int why = (int)(first_bad & 0xffu);
    if (why >= BAD_M && why <= BAD_H) snprintf(buf, bytes, "ledger: the %s is not finite (particle i=%llu)", kInputName[why - BAD_M], id);
    else if (why == BAD_SPEED2) snprintf(buf, bytes, "ledger: the squared speed vx * vx + vy * vy is not finite in f32 (particle i=%llu)", id);
    else if (why == BAD_RHO_SIGN)
        snprintf(buf, bytes, "ledger: the density is not positive (particle i=%llu; before the first step the density is 0: step outputs exist behind sph_step)", id);
    else {
        const int s = std::min(std::max(why - BAD_TERM, 0), kSums - 1);
        const int e = spec->exponent[s];
        if (e == SPH_LEDGER_AUTO_EXPONENT) snprintf(buf, bytes, "ledger: the term of sum %d (%s) is not finite (particle i=%llu)", s, kSumName[s], id);
        else snprintf(buf, bytes, "ledger: the term of sum %d (%s) is not finite or not below 2^exponent = 2^%d (particle i=%llu)", s, kSumName[s], e, id);
    }
}

void fold_only(int n, const sph_ledger_words* words, sph_ledger_words* w)
{
    uint64_t* f = (uint64_t*)w;
    for (int q = 0; q < kWords; q++) f[q] = word_empty(q);
    for (int r = 0; r < n; r++) {
        const uint64_t* v = (const uint64_t*)&words[r];
        for (int q = 0; q < kWords; q++) f[q] = word_fold(q, f[q], v[q]);
    }
}

// the verdict of the folded words: the offender's sentence, or the exponents of the whole vector in spec_io
int fold_words(int n, const sph_ledger_words* words, sph_ledger_spec* spec_io, sph_ledger_words* folded, char* msg, size_t msg_bytes)
{
    sph_ledger_words w;
    fold_only(n, words, &w);
    if (folded) *folded = w;
    if (w.first_bad != SPH_LEDGER_NO_OFFENDER) {
        if (msg && msg_bytes) format_offender(msg, msg_bytes, w.first_bad, spec_io);
        return SPH_ERR_INVALID_ARGUMENT;
    }
    const uint32_t asked = sum_mask(spec_io->what);
    for (int s = 0; s < kSums; s++) {
        if (!((asked >> s) & 1u)) {
            spec_io->exponent[s] = 0;
            continue;
        }
        if (spec_io->exponent[s] != SPH_LEDGER_AUTO_EXPONENT) continue;
        int e = exponent_of_bits(w.max_bits[s]);
        if (e < SPH_LEDGER_MIN_EXPONENT) e = SPH_LEDGER_MIN_EXPONENT;
        if (e > SPH_LEDGER_MAX_EXPONENT) {
            if (msg && msg_bytes) snprintf(msg, msg_bytes, "ledger: sum %d (%s) needs the exponent %d (at most %d)", s, kSumName[s], e, SPH_LEDGER_MAX_EXPONENT);
            return SPH_ERR_INVALID_ARGUMENT;
        }
        spec_io->exponent[s] = e;
    }
    if (msg && msg_bytes) msg[0] = 0;
    return SPH_OK;
}

// the ranks' words and sums -> the result; spec holds explicit exponents
int compose(int n, const sph_ledger_words* words, const sph_ledger_sum* sums, const sph_ledger_spec* spec, sph_ledger_result* out)
{
    sph_ledger_words w;
    fold_only(n, words, &w);
    if (w.first_bad != SPH_LEDGER_NO_OFFENDER) return SPH_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof *out);
    out->what = spec->what;
    out->n = w.n;
    out->n_outside = (spec->what & SPH_LEDGER_OUTSIDE) ? w.n_outside : 0;
    const uint32_t asked = sum_mask(spec->what), keys = extreme_mask(spec->what);
    for (int s = 0; s < kSums; s++) {
        if (!((asked >> s) & 1u)) continue;
        U128 t{0ull, 0ll};
        for (int r = 0; r < n; r++) add128(t, sums[(size_t)r * kSums + s].lo, sums[(size_t)r * kSums + s].hi);
        out->exponent[s] = spec->exponent[s];
        out->raw[s].lo = t.lo;
        out->raw[s].hi = t.hi;
        out->sum[s] = resolve128(out->raw[s], spec->exponent[s] - 60);
    }
    for (int k = 0; k < kExt; k++) {
        const bool is_max = !(k & 1);
        const uint64_t key = w.extreme[k];
        out->extreme[k].value = 0.f;
        out->extreme[k].id = SPH_LEDGER_NO_ID;
        if (!((keys >> k) & 1u) || key == (is_max ? 0ull : ~0ull)) continue;
        const uint32_t o = (uint32_t)(key >> 32), low = (uint32_t)key;
        out->extreme[k].value = __builtin_bit_cast(float, (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
        out->extreme[k].id = is_max ? 0xffffffffu - low : low;
    }
    return SPH_OK;
}

uint32_t ledger_blocks(uint32_t n) { return std::min(std::max((n + 255u) / 256u, 1u), kMaxBlocks); }

LedgerIn make_ledger_in(sph_ctx* c, const sph_params* p, const sph_ledger_spec* spec)
{
    const int k = c->cur;
    LedgerIn a{};
    a.pm = c->pm[c->pcur].as<float4>();
    a.vel = c->vel[k].as<float2>();
    a.orig = c->orig[k].as<uint32_t>();
    a.rho = c->rho.as<float>();
    a.pres = (c->pressure_cur ? c->p1 : c->p0).as<float>();
    a.bnd = c->planes_d.as<BoundaryP>();
    a.n_planes = c->n_planes;
    a.what = spec->what;
    a.rest_density = p->rest_density;
    const uint32_t asked = sum_mask(spec->what);
    for (int s = 0; s < kSums; s++) {
        const int e = spec->exponent[s];
        const bool fixed = ((asked >> s) & 1u) && e != SPH_LEDGER_AUTO_EXPONENT;
        a.limit[s] = fixed ? std::ldexp(1.0, e) : (double)INFINITY;
        a.scale[s] = fixed ? std::ldexp(1.0, 60 - e) : 1.0;
    }
    return a;
}

int ensure_buffers(sph_ctx* c)
{
    HIPCHK(c, c->led_part.ensure((size_t)kMaxBlocks * std::max((size_t)kWords * 8, (size_t)kSums * sizeof(U128))));
    HIPCHK(c, c->led_out.ensure(kOutSums + (size_t)kSums * sizeof(U128)));
    return SPH_OK;
}

// the range pass over c's particles (a slab context: its owned slots) -> the words on the host (waits for c's stream)
int range_pass(sph_ctx* c, const sph_params* p, const sph_ledger_spec* spec, sph_ledger_words* out)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_buffers(c)) return rc;
    hipStream_t s = c->stream;
    const uint32_t n = owned_slots(c), nb = ledger_blocks(n);
    const LedgerIn a = make_ledger_in(c, p, spec);
    {
        ProfScope ps(&c->prof, "ledger_range", s);
        if (c->dist.on) hipLaunchKernelGGL(k_ledger_range<true>, dim3(nb), dim3(256), 0, s, n, a, owned_flags(c), c->led_part.as<unsigned long long>());
        else hipLaunchKernelGGL(k_ledger_range<false>, dim3(nb), dim3(256), 0, s, n, a, (const uint8_t*)nullptr, c->led_part.as<unsigned long long>());
        hipLaunchKernelGGL(k_ledger_fold_words, dim3(kWords), dim3(64), 0, s, nb, c->led_part.as<unsigned long long>(), c->led_out.as<unsigned long long>());
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->led_out.p, sizeof *out, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

// the sum pass under spec's explicit exponents -> the nine sums on the host (waits for c's stream)
int sum_pass(sph_ctx* c, const sph_params* p, const sph_ledger_spec* spec, sph_ledger_sum* out)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_buffers(c)) return rc;
    hipStream_t s = c->stream;
    const uint32_t n = owned_slots(c), nb = ledger_blocks(n);
    const LedgerIn a = make_ledger_in(c, p, spec);
    U128* dst = (U128*)((char*)c->led_out.p + kOutSums);
    {
        ProfScope ps(&c->prof, "ledger_sums", s);
        if (c->dist.on) hipLaunchKernelGGL(k_ledger_sums<true>, dim3(nb), dim3(256), 0, s, n, a, owned_flags(c), c->led_part.as<U128>());
        else hipLaunchKernelGGL(k_ledger_sums<false>, dim3(nb), dim3(256), 0, s, n, a, (const uint8_t*)nullptr, c->led_part.as<U128>());
        hipLaunchKernelGGL(k_ledger_fold_sums, dim3(kSums), dim3(64), 0, s, nb, c->led_part.as<U128>(), dst);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, dst, (size_t)kSums * sizeof(sph_ledger_sum), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return SPH_OK;
}

// everything a call on a context refuses before it launches
int check_call(sph_ctx* c, const char* who, bool slab, const sph_params* p, const sph_ledger_spec* spec, bool allow_auto)
{
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s: null parameters", who);
    if (slab && !c->dist.on) return c->fail(SPH_ERR_UNSUPPORTED, "%s: not a slab context (sph_ledger_compute takes a plain context)", who);
    if (!slab && c->dist.on)
        return c->fail(SPH_ERR_UNSUPPORTED, "%s: slab contexts are not supported here (one rank holds a slab of the particles; the ranks' words fold and their sums "
                                            "add exactly: sph_slab_ledger_range / sph_ledger_fold_words / sph_slab_ledger_sums / sph_ledger_compose / sph_group_ledger)", who);
    if (c->poisoned) return c->refuse_poisoned();
    char msg[400];
    if (spec_fault(spec, allow_auto, who, msg, sizeof msg)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "%s", msg);
    return SPH_OK;
}

static_assert(sizeof(U128) == sizeof(sph_ledger_sum) && offsetof(U128, hi) == offsetof(sph_ledger_sum, hi), "a partial is a sph_ledger_sum");

int group_ledger(sph_ctx** ctxs, int n, const sph_params* p, const sph_ledger_spec* spec, sph_ledger_result* out)
{
    sph_ctx* c0 = ctxs[0];
    if (!out) return c0->fail(SPH_ERR_INVALID_ARGUMENT, "sph_group_ledger: null output");
    for (int i = 0; i < n; i++)
        if (!ctxs[i]->dist.on) return ctxs[i]->fail(SPH_ERR_UNSUPPORTED, "sph_group_ledger: context %d is no slab context (sph_ledger_compute takes a plain context)", i);
    std::vector<sph_ledger_words> words((size_t)n);
    std::vector<sph_ledger_sum> sums((size_t)n * kSums);
    int rc;
    for (int i = 0; i < n; i++)
        if ((rc = sph_slab_ledger_range(ctxs[i], p, spec, &words[(size_t)i]))) return rc;
    sph_ledger_spec sq = *spec;
    char msg[400];
    if ((rc = fold_words(n, words.data(), &sq, nullptr, msg, sizeof msg))) return c0->fail(rc, "%s", msg);
    for (int i = 0; i < n; i++)
        if ((rc = sph_slab_ledger_sums(ctxs[i], p, &sq, &sums[(size_t)i * kSums]))) return rc;
    return compose(n, words.data(), sums.data(), &sq, out);
}

}  // namespace

extern "C" int sph_ledger_compute(sph_ctx* c, const sph_params* p, const sph_ledger_spec* spec, sph_ledger_result* out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_ledger_compute: null output");
    if (int rc = check_call(c, "sph_ledger_compute", false, p, spec, true)) return rc;
    sph_ledger_words words;
    if (int rc = range_pass(c, p, spec, &words)) return rc;
    sph_ledger_spec sq = *spec;
    char msg[400];
    if (int rc = fold_words(1, &words, &sq, nullptr, msg, sizeof msg)) return c->fail(rc, "%s", msg);
    sph_ledger_sum sums[kSums];
    if (int rc = sum_pass(c, p, &sq, sums)) return rc;
    return compose(1, &words, sums, &sq, out);
}

extern "C" int sph_slab_ledger_range(sph_ctx* c, const sph_params* p, const sph_ledger_spec* spec, sph_ledger_words* out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_ledger_range: null output");
    fold_only(0, nullptr, out);
    if (int rc = check_call(c, "sph_slab_ledger_range", true, p, spec, true)) return rc;
    return range_pass(c, p, spec, out);
}

extern "C" int sph_slab_ledger_sums(sph_ctx* c, const sph_params* p, const sph_ledger_spec* spec, sph_ledger_sum* out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sph_slab_ledger_sums: null output");
    memset(out, 0, (size_t)kSums * sizeof *out);
    if (int rc = check_call(c, "sph_slab_ledger_sums", true, p, spec, false)) return rc;
    return sum_pass(c, p, spec, out);
}

extern "C" int sph_ledger_fold_words(int n, const sph_ledger_words* words, sph_ledger_spec* spec_io, sph_ledger_words* folded, char* msg, uint64_t msg_bytes)
{
    if (msg && msg_bytes) msg[0] = 0;
    if (n < 1 || !words || !spec_io) {
        if (msg && msg_bytes) snprintf(msg, (size_t)msg_bytes, "sph_ledger_fold_words: n < 1, null words or null ledger spec");
        return SPH_ERR_INVALID_ARGUMENT;
    }
    char why[400];
    if (spec_fault(spec_io, true, "sph_ledger_fold_words", why, sizeof why)) {
        if (msg && msg_bytes) snprintf(msg, (size_t)msg_bytes, "%s", why);
        return SPH_ERR_INVALID_ARGUMENT;
    }
    return fold_words(n, words, spec_io, folded, msg, (size_t)msg_bytes);
}

extern "C" int sph_ledger_compose(int n, const sph_ledger_words* words, const sph_ledger_sum* sums, const sph_ledger_spec* spec, sph_ledger_result* out)
{
    char why[400];
    if (n < 1 || !words || !sums || !out || spec_fault(spec, false, "sph_ledger_compose", why, sizeof why)) return SPH_ERR_INVALID_ARGUMENT;
    return compose(n, words, sums, spec, out);
}

extern "C" int sph_group_ledger(sph_ctx** ctxs, int n, const sph_params* p, const sph_ledger_spec* spec, sph_ledger_result* out)
{
    return group_call(ctxs, n, [&] { return group_ledger(ctxs, n, p, spec, out); });
}
