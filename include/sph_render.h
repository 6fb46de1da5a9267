/*
 * sph_render.h -- frames of the particle state drawn on the device (the reference's `image` harness without cairo).
 *
 * Replaces, for a Rust or Python host, the per-frame work of platform/desktop/animation/mod.rs:138-272:
 *   get_color_for_particle      colors.rs:386-492      -> the colour pass (one RGB8 per particle)
 *   render2d                    cairo_renderer.rs:19-110 -> the rasteriser (a W x H RGB8 frame)
 * Only the frame crosses PCIe; positions, masses and the visualised field stay where the step left them.
 * The legend bar and the text (legend numbers, title) are drawn by the host (adaptive_sph_amd/render.py).
 *
 * A separate header from sph_ffi.h: these entry points exist in the product library only (the CPU oracle draws nothing).
 *
 * THE FRAME, exactly (every operation below is one IEEE f32 operation, no contraction; a restatement in numpy reproduces the
 * bytes -- tests/render_reference.py):
 *   sample grid   WS = W*S columns, HS = H*S rows, sample (sx, sy), row 0 at the top; its centre (u, v) = (sx + 0.5, sy + 0.5)
 *   mapping       scale = (float)(min(W, H) * S) / (2 * zoom_out);  cx = (float)WS * 0.5;  cy = (float)HS * 0.5
 *                 scene (x, y) -> sample space (cx + x*scale, cy - y*scale)            (origin at the centre, y up)
 *   particle i    position p (interpolated: alpha*p_after + (1 - alpha)*p_before), radius r = sqrt((m / rho0) * FRAC_1_PI)
 *                 px = cx + p.x*scale, py = cy - p.y*scale, ro = (r*1.05)*scale, ri = (r*0.95)*scale
 *                 du = u - px, dv = v - py, d2 = du*du + dv*dv
 *                 covers the sample if d2 < ro*ro; fills it with its colour if also d2 < ri*ri, else paints it black (stroke band)
 *   painter       a sample takes the particle with the LARGEST REFERENCE INDEX that covers it (cairo paints in index order)
 *   boundary      a sample no particle covers is black if it lies on a boundary segment (a, b) (sample-space endpoints
 *                 a = (cx + a.x*scale, cy - a.y*scale), ...): with e = b - a, w = (u, v) - a, t = w.e, c = w.x*e.y - w.y*e.x,
 *                 L2 = e.e, hw = (line_width*0.5)*scale:  0 <= t <= L2 and c*c < (hw*hw)*L2   (a butt-capped stroke); else white
 *   colour -> u8  floor(c*255 + 0.5), clamped to 0..255, per sample; a pixel is (sum of its S*S samples + S*S/2) / (S*S)
 *
 * THE COLOUR of particle i (colors.rs:386-492, in the reference's order):
 *   flag_neighborhood_reduced && SPH_RENDER_SHOW_NEIGHBORHOOD_REDUCED -> green; flag_is_fluid_surface && SPH_RENDER_SHOW_SURFACE ->
 *   red; flag_insufficient_neighs && SPH_RENDER_SHOW_SURFACE -> green (the reference gates this one by the surface switch too);
 *   else the attribute: ColorMap::get (color_map.rs:14-30) over the host's stops of the value
 *     AII aii | DISTANCE level_estimation (FluidInterior -> -maximum_surface_distance), stash with SPH_RENDER_FROM_STASH |
 *     DENSITY density / rest_density | VELOCITY |v| = sqrt(vx*vx + vy*vy) | NEIGHBOR_COUNT (float)count - 3.8*3.8 |
 *     CONSTANT_FIELD | SOURCE_TERM ppe_source_term | MIN_DISTANCE min over the exported neighbour list without i of
 *     sqrt(dx*dx + dy*dy) / h_i, and 2 | PRESSURE: the stops (0, white), (0.9 * max(0, max_j p_j), red), the max a device reduction;
 *   SIZE_CLASS five fixed colours; SINGLE_COLOR (80, 140, 255); RANDOM_COLOR bytes 0..2 of SipHash-1-3 (keys 0) of the reference
 *   index as 8 little-endian bytes (Rust's DefaultHasher of a usize).
 *   ColorMap::get: x <= v_0 -> c_0; x >= v_last -> c_last; else the first k with v_k <= x <= v_(k+1):
 *   t = (x - v_k) / (v_(k+1) - v_k), c = c_k + t*(c_(k+1) - c_k) per channel.  A NaN value takes c_0 (the reference panics).
 *
 * Status codes are those of sph_ffi.h: SPH_ERR_INVALID_ARGUMENT (S outside 1..4, W or H < 1, more than 16384 x 16384 samples,
 * a short output buffer, more than 16 stops or none for a mapped attribute, interpolation without a snapshot or with one of
 * another particle count, MIN_DISTANCE before the first step), SPH_ERR_UNSUPPORTED (slab contexts: one rank holds a slab of
 * the frame's particles), SPH_ERR_DEVICE.  Nothing here changes the simulation state; every launch runs on the context's stream.
 */
#ifndef SPH_RENDER_H
#define SPH_RENDER_H

#include <stdint.h>

#include "sph_ffi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* VisualizedAttribute, simulation.rs:2804-2817 (same order) */
enum {
    SPH_VIS_DISTANCE = 0, SPH_VIS_SINGLE_COLOR = 1, SPH_VIS_PARTICLE_SIZE_CLASS = 2, SPH_VIS_PRESSURE = 3, SPH_VIS_DENSITY = 4,
    SPH_VIS_VELOCITY = 5, SPH_VIS_RANDOM_COLOR = 6, SPH_VIS_AII = 7, SPH_VIS_NEIGHBOR_COUNT = 8, SPH_VIS_MIN_DISTANCE_TO_NEIGHBOR = 9,
    SPH_VIS_CONSTANT_FIELD = 10, SPH_VIS_SOURCE_TERM = 11, SPH_VIS_COUNT_ = 12
};

/* VisualizationParams switches (simulation.rs:2875-2888) + the video interpolation */
enum {
    SPH_RENDER_SHOW_SURFACE = 1,                 /* show_flag_is_fluid_surface */
    SPH_RENDER_SHOW_NEIGHBORHOOD_REDUCED = 2,    /* show_flag_neighborhood_reduced */
    SPH_RENDER_FROM_STASH = 4,                   /* take_data_from_stash */
    SPH_RENDER_INTERPOLATE = 8                   /* positions alpha*now + (1 - alpha)*snapshot (animation/mod.rs:195-213) */
};

#define SPH_RENDER_MAX_STOPS 16
#define SPH_RENDER_MAX_SAMPLES_PER_SIDE 16384

typedef struct sph_render_params {
    int32_t  width, height;          /* output pixels */
    int32_t  supersample;            /* S: S x S samples per pixel, 1..4 */
    float    zoom_out;               /* 1.04 in the reference's default */
    int32_t  attribute;              /* SPH_VIS_* */
    uint32_t flags;                  /* SPH_RENDER_* */
    float    alpha;                  /* interpolation weight of the current positions (with SPH_RENDER_INTERPOLATE) */
    int32_t  n_stops;                /* colour map: stops[k] = (value, r, g, b), values ascending (ColorMap::new sorts them) */
    float    stops[SPH_RENDER_MAX_STOPS][4];
    int32_t  n_segments;             /* boundary lines: segments[4k .. 4k+3] = (a.x, a.y, b.x, b.y), scene units */
    const float* segments;
    float    line_width;             /* scene units (cairo_renderer.rs:73, 80: 5 / 1000) */
} sph_render_params;

/* The frame: height rows of width RGB8 pixels, top row first (rgb_out: >= width*height*3 bytes). */
int sph_render(sph_ctx* ctx, const sph_params* params, const sph_render_params* rp, uint8_t* rgb_out, uint64_t out_bytes);
/* The colour pass alone: one RGB8 per particle in reference (host) order (rgb_out: >= n*3 bytes). */
int sph_render_colors(sph_ctx* ctx, const sph_params* params, const sph_render_params* rp, uint8_t* rgb_out, uint64_t out_bytes);
/* Keep the current positions (by reference index) for the next interpolated frame: call it right before the step. */
int sph_render_snapshot(sph_ctx* ctx);

#ifdef __cplusplus
}
#endif

#endif /* SPH_RENDER_H */
