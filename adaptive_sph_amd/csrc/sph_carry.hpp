// What a step leaves behind for the next step and for the host, and what each entry point called between two steps drops of it: the
// table of DESIGN.md ("What a call between two steps invalidates"), one named mask per row.  sph_ctx derives from Carry; drop() is the
// only writer of `false` to these flags outside the code that produces the state (the step driver, the export and partner entry points).
// Pure host code, no HIP: tests/host/carry_check.cpp compiles this header with plain g++ and tests/test_carry_host.py compares every
// cell with its own restatement of the table.
#pragma once

#include <cstdint>

// one bit per thing that can go stale; two things share a bit only if no entry point drops one without the other
enum : unsigned {
    CARRY_HEADER = 1u << 0,        // hdr_ahead: hdr_host already holds the header of the state on the device (no k_header needed)
    CARRY_BUILD = 1u << 1,         // ahead_valid: the neighbour build queued on the predicted grid
    CARRY_LISTS = 1u << 2,         // grid_valid: the lists and cell indices of the last step
    CARRY_EXPORT = 1u << 3,        // export_valid: the CSR of those lists; prob_open: the partner problem made from it, and its solution
    CARRY_SLAB_LISTS = 1u << 4,    // slab_lists_valid, slab_rows_open, slab_prob_open: the same CSR, the prepared rows and the problem packed from them on a slab context
    CARRY_LEVEL = 1u << 5,         // have_level, have_reduced: level outputs that do not travel with a particle (stash, flags)
    CARRY_LISTS_AFTER = 1u << 6,   // lists_after: the cache holds the extended lists of the advected positions
    CARRY_MOVERS = 1u << 7,        // inc_count_valid: the mapped mover-count word was written by a merge queued SINCE the state was last replaced
    CARRY_GHOSTS = 1u << 8,        // have_flags: dist.owned describes the current arrays of a slab context
    CARRY_SNAPSHOT = 1u << 9,      // rnd_have_prev: the positions kept for an interpolated frame
};

// ---- the rows.  The step adopts the queued build only while the header the same step left is in force, so whatever writes particle
// state drops both; sph_classify writes the classes alone: the header does not read them, the build carries a copy from before the call
constexpr unsigned DROPS_CLASSIFY = CARRY_BUILD;
// sph_upload_field: the list exports index positions and masses; the entries of a slab context's lists become ids as well
constexpr int CARRY_F_MASS = 0, CARRY_F_POSITION = 1, CARRY_F_PARTICLE_ID = 22;   // (SPH_F_*: sph_api.hip asserts the values)
constexpr unsigned drops_upload_field(int field)
{
    return CARRY_HEADER | CARRY_BUILD | (field == CARRY_F_POSITION || field == CARRY_F_MASS ? CARRY_EXPORT | CARRY_SLAB_LISTS : 0u) |
           (field == CARRY_F_PARTICLE_ID ? CARRY_SLAB_LISTS : 0u);
}
// a transfer between partners (share; merge before it deletes): positions and masses change, the vector keeps its order -- stash and
// flags keep describing the particles in their slots, the exports stay for the merge search that follows a share
constexpr unsigned DROPS_TRANSFER = CARRY_HEADER | CARRY_BUILD | CARRY_LISTS | CARRY_MOVERS | CARRY_LISTS_AFTER;
constexpr unsigned DROPS_DELETION = CARRY_LEVEL;   // merge with a deletion, on top of DROPS_TRANSFER: the vector is about to be reordered
// the regather into host order (merge with a deletion, split with a split, edits, the slab merge / split): another vector.  (a slab
// context never holds a valid CSR export, so its regather shares the row)
constexpr unsigned DROPS_REGATHER = DROPS_TRANSFER | DROPS_DELETION | CARRY_EXPORT | CARRY_SLAB_LISTS | CARRY_GHOSTS;
// merge and split drop the export right behind their argument checks (a split with nobody TooLarge drops nothing else), edits the slab lists too
constexpr unsigned DROPS_EXPORT_EARLY = CARRY_EXPORT, DROPS_EDITS_EARLY = CARRY_EXPORT | CARRY_SLAB_LISTS;
constexpr unsigned DROPS_UPLOAD = DROPS_REGATHER | CARRY_SNAPSHOT;
constexpr unsigned DROPS_POLICY = DROPS_TRANSFER | CARRY_EXPORT | CARRY_SLAB_LISTS;   // to the other policy: the particle state is policy-free
constexpr unsigned DROPS_DIST_CONFIGURE = CARRY_HEADER | CARRY_BUILD | CARRY_GHOSTS;
constexpr unsigned DROPS_STEP_START = CARRY_EXPORT | CARRY_SLAB_LISTS;   // an accepted step replaces the lists the exports were made from
constexpr unsigned DROPS_STEP_FAILED = CARRY_HEADER;   // ... and one that failed after it started poisons the context

struct Carry {
    bool hdr_ahead = false, ahead_valid = false, grid_valid = false, export_valid = false, prob_open = false, slab_lists_valid = false, slab_rows_open = false;
    bool slab_prob_open = false;   // (sph_slab_partner_problem.hip: valid exactly as long as the prepared rows are)
    bool have_level = false, have_reduced = false, lists_after = false, inc_count_valid = false, have_flags = false, rnd_have_prev = false;
    volatile uint32_t* movers_host = nullptr;   // the mapped mover-count word (sph_create; null until the mapped block exists)

    void drop(unsigned what)
    {
        if (what & CARRY_HEADER) hdr_ahead = false;
        if (what & CARRY_BUILD) ahead_valid = false;
        if (what & CARRY_LISTS) grid_valid = false;
        if (what & CARRY_EXPORT) export_valid = prob_open = false;
        if (what & CARRY_SLAB_LISTS) slab_lists_valid = slab_rows_open = slab_prob_open = false;
        if (what & CARRY_LEVEL) have_level = have_reduced = false;
        if (what & CARRY_LISTS_AFTER) lists_after = false;
        if (what & CARRY_MOVERS) inc_count_valid = false;   // (a build still in flight may write its stale count after the reset below)
        if ((what & CARRY_MOVERS) && movers_host) *movers_host = 0u;
        if (what & CARRY_GHOSTS) have_flags = false;
        if (what & CARRY_SNAPSHOT) rnd_have_prev = false;
    }
    // an export built the CSR: a rebuild closes the problem made from the CSR before it, a re-export of the valid CSR keeps it open
    void export_built() { if (!export_valid) drop(CARRY_EXPORT); export_valid = true; }
};
