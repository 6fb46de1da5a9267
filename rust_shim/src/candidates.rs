//! Rust side of `include/sph_candidates.h` (product library only; a block of its own, like the header).
//!
//! `sph_download_partner_candidates` hands back the CSR a `NeighborhoodCache` is filled from -- over all particles, host
//! order -- in which only the donors' rows are populated, with the neighbours that pass the class and the distance test of
//! `find_share_partner_sequential` (kind 0) / `find_merge_partner_sequential` (kind 1).  Both searches run UNCHANGED on a cache
//! built from it: the two tests are idempotent and the rows keep their order, so `merge_partner` / `merge_counter` come out as
//! on the full lists, and `validate_*_partners` (which count `merge_partner[j] == i` over row i) hold as well.
use std::os::raw::{c_int, c_void};

use crate::ffi::{SphAdaptParams, SphParams};

extern "C" {
    pub fn sph_download_partner_candidates(ctx: *mut c_void, kind: c_int, params: *const SphParams, ap: *const SphAdaptParams,
                                           offsets: *mut u32, indices: *mut u32, indices_capacity: u64, n_indices: *mut u64) -> c_int;
    pub fn sph_sum_mass(ctx: *mut c_void, total: *mut f64) -> c_int;
}
