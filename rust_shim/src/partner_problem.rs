//! Rust side of `include/sph_partner_problem.h` (product library only; a block of its own, like the header).
//!
//! `sph_download_partner_problem` hands back the partner search of `kind` restricted to its K participants -- the donors that
//! have a candidate and the candidates -- numbered in ascending host index: their five decision fields and their candidate rows
//! in compact ids.  Fill a `ParticleVec` of K particles and a `NeighborhoodCache` of K rows from it and run
//! `find_share_partner_sequential` (kind 0) / `find_merge_partner_sequential` (kind 1) and `validate_*_partners` UNCHANGED: the
//! renumbering is monotone and the loop touches participants only, so the K decisions are those of the full vector.  Hand
//! `merge_partner` / `merge_counter` of those K particles to `sph_share_particles_compact` / `sph_merge_particles_compact`.
use std::os::raw::{c_int, c_void};

use crate::ffi::{SphAdaptParams, SphParams};

extern "C" {
    pub fn sph_download_partner_problem(ctx: *mut c_void, kind: c_int, params: *const SphParams, ap: *const SphAdaptParams,
                                        ids: *mut u32, size_class: *mut u8, mass: *mut f32, level_estimation: *mut f32,
                                        position: *mut f32, h2: *mut f32, offsets: *mut u32, participants_capacity: u64,
                                        indices: *mut u32, indices_capacity: u64, n_participants: *mut u64, n_indices: *mut u64) -> c_int;
    pub fn sph_share_particles_compact(ctx: *mut c_void, params: *const SphParams, ap: *const SphAdaptParams, k: u64,
                                       partner_c: *const u32, counter_c: *const u16) -> c_int;
    pub fn sph_merge_particles_compact(ctx: *mut c_void, params: *const SphParams, ap: *const SphAdaptParams, k: u64,
                                       partner_c: *const u32, counter_c: *const u16) -> c_int;
}
