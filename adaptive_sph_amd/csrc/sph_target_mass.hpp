// LevelEstimationState::target_mass on the device, shared by the apply kernels of sph_adapt.hip and the partner search of
// sph_partner_search.hip: one definition, so a donor's dropped mass and a receiver's target are the same f32 values in both.
#pragma once

#include "sph_internal.hpp"

// ---- LevelEstimationState::target_mass (simulation.rs:213-237) -- the same IEEE operations as k_classify -----------------
struct TargetP {
    float max_surface_distance, rest_density, radius_fine, radius_base;
    int sizing_function;
};
__device__ __forceinline__ float target_mass(float lv, const TargetP& t)
{
    const float lvl = fmaxf(lv, -t.max_surface_distance);
    const float interp = lvl / -t.max_surface_distance;
    const float mass_fine = (SPH_PI_F * t.radius_fine * t.radius_fine) * t.rest_density;
    const float mass_base = (SPH_PI_F * t.radius_base * t.radius_base) * t.rest_density;
    if (t.sizing_function == SPH_SIZING_MASS) return mass_fine * (1.f - interp) + mass_base * interp;
    if (t.sizing_function == SPH_SIZING_RADIUS) {
        const float r = t.radius_fine * (1.f - interp) + t.radius_base * interp;
        return (SPH_PI_F * r * r) * t.rest_density;
    }
    const float e = 1.f / 2.f;
    const float r = t.radius_fine * (1.f - powf(interp, e)) + t.radius_base * powf(interp, e);
    return (SPH_PI_F * r * r) * t.rest_density;
}
static inline TargetP target_params(const sph_params* p)
{
    return TargetP{p->maximum_surface_distance, p->rest_density, p->particle_radius_fine, p->particle_radius_base, p->sizing_function};
}
