// The boundary entry of one particle at one SDF (include/sph_wall_load.h: THE ENTRY), stated once for the wall-load kernels.  The same
// arithmetic as the step's density sweep (sph_sweeps.hip: OpDensity::begin) -- every IEEE operation in its order; the library is compiled
// with -ffp-contract=off -- but a statement of its own: the step's kernels are not touched, and tests/test_wall_load_host.py and
// tests/test_gpu_wall_load.py tie the two together bit for bit.
#pragma once

#include "sph_device.h"

struct WallEntry {
    float nx, ny;   // the normalised gradient of the SDF
    float gx, gy;   // grad lambda
};

// d = sdf_probe(k, x, y) / sr of the caller (who has tested d < 1).  false: no entry (the gradient's norm is below 1e-5 or no number)
__device__ __forceinline__ bool wall_entry(const BoundaryP* __restrict__ b, int k, float x, float y, float sr, float d, float eps, int penalty_term,
                                           const float* __restrict__ lam_lut, const float* __restrict__ dlam_lut, WallEntry& e)
{
    const float inv_2eps = 1.f / (2.f * eps);
    float gx = (sdf_probe(b, k, x + eps, y) - sdf_probe(b, k, x - eps, y)) * inv_2eps;
    float gy = (sdf_probe(b, k, x, y + eps) - sdf_probe(b, k, x, y - eps)) * inv_2eps;
    const float gn = sqrtf(gx * gx + gy * gy);
    if (!(gn >= 0.00001f)) return false;
    gx /= gn;
    gy /= gn;
    float penalty, dpenalty;
    if (penalty_term == SPH_PENALTY_NONE) {
        penalty = 1.f;
        dpenalty = 0.f;
    } else if (penalty_term == SPH_PENALTY_LINEAR) {
        penalty = 1.f - d;
        dpenalty = -1.f;
    } else if (penalty_term == SPH_PENALTY_QUADRATIC1) {
        if (d > 0.f) { penalty = 1.f; dpenalty = 0.f; }
        else if (d > -1.f) { penalty = 0.5f * d * d + 1.f; dpenalty = d; }
        else { penalty = 0.5f - d; dpenalty = -1.f; }
    } else {
        if (d > 0.f) { penalty = 1.f; dpenalty = 0.f; }
        else if (d > -0.5f) { penalty = d * d + 1.f; dpenalty = 2.f * d; }
        else { penalty = 0.75f - d; dpenalty = -1.f; }
    }
    float lambda, dlambda;
    if (d <= -1.f) { lambda = 1.f; dlambda = 0.f; }
    else { lambda = lut_get(lam_lut, d); dlambda = lut_get(dlam_lut, d); }   // (-1 < d < 1: the table's range)
    const float s = dpenalty * lambda + penalty * dlambda;
    e.nx = gx;
    e.ny = gy;
    e.gx = gx / sr * s;
    e.gy = gy / sr * s;
    return true;
}

// include/sph_wall_load.h: THE COEFFICIENT
__device__ __forceinline__ float wall_coefficient(float p, float rho, float rho_b, bool symmetric)
{
    const float p_ib = symmetric ? p : 0.f;
    return rho_b * (p / (rho * rho) + p_ib / (rho_b * rho_b));
}

// include/sph_wall_load.h: THE TERMS -- t[0..3] = fx, fy, tq, fn
__device__ __forceinline__ void wall_terms(float m, float c, float x, float y, const WallEntry& e, double* t)
{
    const double mc = (double)m * (double)c;
    const double fx = mc * (double)e.gx, fy = mc * (double)e.gy;
    t[0] = fx;
    t[1] = fy;
    t[2] = (double)x * fy - (double)y * fx;
    t[3] = -(fx * (double)e.nx + fy * (double)e.ny);
}
