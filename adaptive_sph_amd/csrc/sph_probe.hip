// SPH fields at arbitrary points and tracers (include/sph_probe.h): the terms of sph_sample.h with (X, Y) a probe's own two floats.
// The pair arithmetic is point_pair of sph_sample_internal.hpp, the function sample_pair calls for a lattice sample, so a probe on a
// sample's centre gets that sample's words; the sums are 64-bit integers, so no word depends on the bins, the launch shape or the
// order the atomics arrive in (tests/probe_reference.py restates them in numpy).
//
// A scatter, for the reason sph_sample.hip states: a gather walks cells of the LARGEST support.  Here the POINTS are binned, not the
// particles: square cells over the points' bounding box, cell_start[] and the points in cell order (row-major, so the cells
// [cx0, cx1] of one row hold one contiguous run of points).  A particle reads the rows its support overlaps.
//
// The set, the kernels and the accumulation sit in sph_probe_internal.hpp, shared with the slab form (sph_slab_probe.hip); this file
// holds the entry points of sph_probe.h.
//
// Kernels (all on the context's stream; they read the state and write only the probe buffers):
//   k_probe_bin_count / k_probe_bin_place   the cell of every point and its place inside the cell (one returning atomic per point),
//                     device_exclusive_scan_u32 between them: cell_start[], then coordinates and caller indices in cell order.  Run at
//                     create / upload and behind an advect (lazily: before the set's next use)
//   k_probe_scatter   one wave (one block of 64) per 64 particles: lane l loads pm[l] only and derives the rows and columns of cells its
//                     support may reach -- a superset: the predicate q < 1 alone decides membership.  A wave none of whose particles
//                     reaches the points' bounding box ends there: a sparse set costs the streaming read of 16 B per particle.  The
//                     (particle, row) SEGMENTS of the wave are laid end to end across the lanes (two loads of cell_start each); rho,
//                     the channel values and the norm are loaded only by particles with a non-empty segment; then the points of 64
//                     segments at a time are laid end to end across the lanes, so no lane idles behind a particle with few points.
//                     w once per pair, non-returning 64-bit atomicAdd per plane (point_pair), planes in the CALLER's point order
//   k_probe_touched   counts the points a pair touched
//   k_sample_resolve  the lattice form's, with nx = n_points, ny = 1
//   k_probe_move      the advect's per-point update, its counts and the new bounding box
#include "sph_probe_internal.hpp"

void probe_sets_release(sph_ctx* c)
{
    for (sph_probe_set* ps : c->probe_sets) free_set(ps);
    c->probe_sets.clear();
}

extern "C" int sph_probe_set_create(sph_ctx* c, const float* xy, uint64_t n_points, float cell_hint, sph_probe_set** out)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (!out) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null output handle");
    *out = nullptr;
    if (!(cell_hint >= 0.f) || !(cell_hint < INFINITY)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: the cell hint must be 0 or finite and positive");
    float bb[4];
    if (int rc = check_points(c, xy, n_points, bb)) return rc;
    sph_probe_set* ps = new sph_probe_set;
    ps->owner = c;
    ps->hint = cell_hint;
    if (int rc = set_points(c, ps, xy, n_points, bb)) {
        free_set(ps);
        return rc;
    }
    c->probe_sets.push_back(ps);
    *out = ps;
    return SPH_OK;
}

extern "C" int sph_probe_set_upload(sph_ctx* c, sph_probe_set* set, const float* xy, uint64_t n_points)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_set(c, set)) return rc;
    float bb[4];
    if (int rc = check_points(c, xy, n_points, bb)) return rc;   // (a refused upload leaves the set as it was)
    return set_points(c, set, xy, n_points, bb);
}

extern "C" int sph_probe_set_download(sph_ctx* c, sph_probe_set* set, float* xy_out, uint64_t bytes)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_set(c, set)) return rc;
    if (bytes < set->n * 8 || (set->n && !xy_out))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: output buffer of %llu bytes, %llu needed", (unsigned long long)bytes, (unsigned long long)(set->n * 8));
    if (!set->n) return SPH_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(xy_out, set->xy.p, (size_t)set->n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SPH_OK;
}

extern "C" int sph_probe_set_size(sph_ctx* c, sph_probe_set* set, uint64_t* n_points)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_set(c, set)) return rc;
    if (!n_points) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null output");
    *n_points = set->n;
    return SPH_OK;
}

extern "C" int sph_probe_set_bins(sph_ctx* c, sph_probe_set* set, float* cell_size, int32_t* cells_x, int32_t* cells_y)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_set(c, set)) return rc;
    if (!set->binned) choose_bins(set);   // (behind an advect: what the next use will bin with)
    if (cell_size) *cell_size = set->cell;
    if (cells_x) *cells_x = set->cx;
    if (cells_y) *cells_y = set->cy;
    return SPH_OK;
}

extern "C" int sph_probe_set_destroy(sph_ctx* c, sph_probe_set* set)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_set(c, set)) return rc;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->probe_sets.erase(std::find(c->probe_sets.begin(), c->probe_sets.end(), set));
    free_set(set);
    return SPH_OK;
}

extern "C" int sph_probe_sample(sph_ctx* c, const sph_params* p, sph_probe_set* set, const sph_probe_params* pp, float* values_out, uint64_t values_bytes,
                                int64_t* raw_out, uint64_t raw_bytes, sph_probe_info* info)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_probe_context(c, p, set)) return rc;
    if (!pp) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null probe parameters");
    const sph_sample_params sp = as_sample_params(set, pp->volume, pp->flags, pp->min_weight, pp->fill, pp->n_channels, pp->channels);
    if (int rc = check_channels(c, &sp)) return rc;
    const int C = sp.n_channels;
    const uint64_t n_values = (uint64_t)(C + 1) * set->n;
    if (n_values && (!values_out || values_bytes < n_values * 4))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: output buffer of %llu bytes, %llu needed", (unsigned long long)values_bytes,
                       (unsigned long long)(n_values * 4));
    if (n_values && raw_out && raw_bytes < n_values * 8)
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: raw output buffer of %llu bytes, %llu needed", (unsigned long long)raw_bytes,
                       (unsigned long long)(n_values * 8));

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int expo[kMaxCh] = {0, 0, 0, 0, 0, 0};
    if (int rc = accumulate(c, p, set, &sp, expo)) return rc;
    if (n_values) {
        launch_resolve(c, &sp, expo, c->smp_planes.as<long long>());
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(values_out, c->smp_out.p, (size_t)n_values * 4, hipMemcpyDeviceToHost, s));
        if (raw_out) HIPCHK(c, hipMemcpyAsync(raw_out, c->smp_planes.p, (size_t)n_values * 8, hipMemcpyDeviceToHost, s));
    }
    SampleRed red;
    ProbeStat st;
    HIPCHK(c, hipMemcpyAsync(&red, c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&st, c->prb_stat.p, sizeof(ProbeStat), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (info) fill_info(info, set, expo, red, st);
    return SPH_OK;
}

extern "C" int sph_probe_advect(sph_ctx* c, const sph_params* p, sph_probe_set* set, const sph_probe_advect_params* ap, sph_probe_info* info)
{
    if (!c) return SPH_ERR_INVALID_ARGUMENT;
    if (int rc = check_probe_context(c, p, set)) return rc;
    if (!ap) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: null advect parameters");
    if (!(std::fabs(ap->dt) < INFINITY)) return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: advect: dt must be finite");
    if (!(ap->min_weight > 0.f) || !(ap->min_weight < INFINITY))
        return c->fail(SPH_ERR_INVALID_ARGUMENT, "probe: advect: min_weight must be finite and > 0 (a point divides by its weight)");
    const sph_sample_channel ch[2] = {{SPH_F_VELOCITY, 0, ap->exponent_x}, {SPH_F_VELOCITY, 1, ap->exponent_y}};
    const sph_sample_params sp = as_sample_params(set, ap->volume, 0u, ap->min_weight, 0.f, 2, ch);
    if (int rc = check_channels(c, &sp)) return rc;

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int expo[kMaxCh] = {0, 0, 0, 0, 0, 0};
    if (int rc = accumulate(c, p, set, &sp, expo)) return rc;
    const uint32_t np = (uint32_t)set->n;
    if (np) {
        ProfScope prof(&c->prof, "probe_move", s);
        hipLaunchKernelGGL(k_probe_move, dim3(std::min((np + 255) / 256, kMoveBlocks)), dim3(256), 0, s, np, c->smp_planes.as<long long>(), set->xy.as<float2>(), ap->dt, ap->min_weight,
                           std::ldexp(1.0, expo[0] - 32), std::ldexp(1.0, expo[1] - 32), c->prb_stat.as<ProbeStat>());
        HIPCHK(c, hipGetLastError());
    }
    SampleRed red;
    ProbeStat st;
    HIPCHK(c, hipMemcpyAsync(&red, c->smp_red.p, sizeof(SampleRed), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&st, c->prb_stat.p, sizeof(ProbeStat), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (info) fill_info(info, set, expo, red, st);   // (the geometry the call used)
    if (np) {   // the box of the points as they are now comes with the counts; the bins follow at the next use
        for (int k = 0; k < 4; k++) set->bb[k] = float_of(st.bb[k]);
        set->binned = false;
    }
    return SPH_OK;
}
