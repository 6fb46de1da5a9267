// SPH fields on a regular grid (include/sph_sample.h): the interpolant of up to six (field, component) channels and the weight plane,
// accumulated as 64-bit fixed-point integers.  The terms are stated in sph_sample.h; every operation here is one IEEE f32 operation in
// that order (the library is compiled with -ffp-contract=off, `/` and sqrtf are correctly rounded), and integer addition is
// associative, so tests/sample_reference.py reproduces every plane bit for bit whatever the device order, the launch shape or the
// arrival order of the atomics.
//
// A scatter, not a gather: a gather over a cell grid walks cells of the LARGEST support, thousands of fine particles per sample under
// 50:1 radii; a scatter costs each particle its own footprint.
//
// Kernels (all on the context's stream, reading the state, writing only the sample buffers):
//   k_sample_range    one thread per particle in device order: the preconditions (the smallest offending reference index wins: one
//                     64-bit atomicMin) and max |a| per channel as float bits (wave reduction, LDS across the waves, one u32 atomicMax
//                     per block and channel: the bit order of non-negative floats is their value order)
//   k_sample_scatter  one wave per batch of 64 particles: lane l loads particle l once; the wave then walks the batch's boxes with its
//                     lanes ACROSS THE COLUMNS -- the boxes laid end to end, row-major, so that consecutive lanes add to contiguous
//                     samples of a row and no lane idles behind a small footprint; a box of more than 2^15 samples is taken alone,
//                     64 columns of a row per pass; w once per (particle, sample), reused by every channel; non-returning 64-bit
//                     atomicAdd per plane
//   k_sample_resolve  one thread per sample: int64 -> f64 -> f32, normalise and fill
// The step's guard word (DeviceStatus) is the step's: a refusal here must leave the context as it was, so the range pass reports into
// a word of its own.
// The kernels, the terms and the parameter checks live in sph_sample_internal.hpp, shared with the sampling of slab contexts
// (sph_slab_sample.hip); this file launches their <false> variants: every slot a particle, full plane rows.
#include "sph_sample_internal.hpp"

namespace {

using ScatterFn = void (*)(uint32_t, SampleIn, SampleGrid, long long*, SampleRed*, const uint8_t*, int, int);
const ScatterFn kScatter[kMaxCh + 1] = {k_sample_scatter<0, false>, k_sample_scatter<1, false>, k_sample_scatter<2, false>, k_sample_scatter<3, false>,
                                        k_sample_scatter<4, false>, k_sample_scatter<5, false>, k_sample_scatter<6, false>};

int check_context(sph_ctx* c, const sph_params* p)
{
    if (!p) return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: null parameters");
    if (c->poisoned) return c->refuse_poisoned();
    if (c->dist.on)
        return c->fail(SPH_ERR_UNSUPPORTED, "sample: slab contexts are not supported here (one rank holds a slab of the particles; the ranks' raw planes add exactly: "
                                            "sph_slab_sample_layer / sph_sample_compose / sph_group_sample_grid of sph_slab_sample.h)");
    return SPH_OK;
}

}  // namespace

extern "C" int sph_sample_field_range(sph_ctx* c, const sph_params* p, int field, int component, float* max_abs, int32_t* exponent)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_context(c, p)) return rc;
    if (int rc = check_channel(c, field, component)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    SampleIn a = make_sample_in(c, p, SPH_SAMPLE_VOLUME_REST);
    a.nch = 1;
    a.field[0] = field;
    a.comp[0] = component;
    a.limit[0] = INFINITY;
    a.values_only = 1;   // (the channel's values alone: h and the volume are sph_sample_grid's business)
    SampleRed red;
    if (int rc = range_pass(c, a, &red)) return rc;
    const float m = __builtin_bit_cast(float, red.max_bits[0]);
    if (max_abs) *max_abs = m;
    if (exponent) *exponent = exponent_of(m);
    return SPH_OK;
}

extern "C" int sph_sample_grid(sph_ctx* c, const sph_params* p, const sph_sample_params* sp, float* values_out, uint64_t values_bytes,
                               int64_t* raw_out, uint64_t raw_bytes, sph_sample_info* info)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_context(c, p)) return rc;
    if (int rc = check_sample_params(c, sp)) return rc;
    if (int rc = check_sample_buffers(c, sp, values_out, values_bytes, raw_out, raw_bytes)) return rc;
    const int C = sp->n_channels;
    const uint64_t n_values = value_count(sp);

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint32_t n = (uint32_t)c->n;
    const SampleIn a = make_sample_in(c, p, sp);
    SampleRed red;
    if (int rc = range_pass(c, a, &red)) return rc;

    int expo[kMaxCh] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < C; k++) {
        expo[k] = sp->channels[k].exponent;
        if (expo[k] == SPH_SAMPLE_AUTO_EXPONENT && !auto_exponent(red.max_bits[k], expo[k]))
            return c->fail(SPH_ERR_INVALID_ARGUMENT, "sample: channel %d (%s) needs the exponent %d (at most %d)", k, field_name(a.field[k]), expo[k],
                           SPH_SAMPLE_MAX_EXPONENT);
    }
    const SampleGrid g = make_sample_grid(sp, expo);

    HIPCHK(c, c->smp_planes.ensure((size_t)n_values * 8));
    HIPCHK(c, c->smp_out.ensure((size_t)n_values * 4));
    HIPCHK(c, hipMemsetAsync(c->smp_planes.p, 0, (size_t)n_values * 8, s));
    if (n) {
        ProfScope ps(&c->prof, "sample_scatter", s);
        const uint32_t waves = (n + 63) / 64;
        hipLaunchKernelGGL(kScatter[C], dim3((waves + 3) / 4), dim3(256), 0, s, n, a, g, c->smp_planes.as<long long>(), c->smp_red.as<SampleRed>(),
                           (const uint8_t*)nullptr, 0, 0);
    }
    launch_resolve(c, sp, expo, c->smp_planes.as<long long>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(values_out, c->smp_out.p, (size_t)n_values * 4, hipMemcpyDeviceToHost, s));
    if (raw_out) HIPCHK(c, hipMemcpyAsync(raw_out, c->smp_planes.p, (size_t)n_values * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&red, c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (info) {
        for (int k = 0; k < kMaxCh; k++) info->exponents[k] = expo[k];
        fold_stats(red, info);
    }
    return SPH_OK;
}
