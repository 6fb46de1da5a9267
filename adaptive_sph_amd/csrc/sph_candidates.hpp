// The candidate rows on the device, shared by sph_candidates.hip (which hands them to the host as they are) and
// sph_partner_problem.hip (which renumbers their participants): one definition of the rows, two exports.
#pragma once

#include "sph_context.hpp"

struct CandP {
    int share;             // kind == 0
    uint32_t donor_class;  // Large (3) when sharing, TooSmall (0) when merging
    float max_dist_factor;
    int allow_optimal;     // allow_{share,merge}_with_optimal_particle
    int allow_too_small;   // allow_share_with_too_small_particle
    int allow_size_diff;   // allow_merge_on_size_difference
};
CandP cand_params(int kind, const sph_adapt_params* ap);

// poisoned -> SPH_ERR_POISONED, a slab context -> SPH_ERR_UNSUPPORTED
int cand_refuse_common(sph_ctx* c, const char* what);
// the CSR of the last step's lists on the device (export_valid), built here if neither export has built it yet
int cand_need_lists(sph_ctx* c);
// n > 0, lists present.  gather + count + scan: cand_rec / cand_cls in host order, cand_off[n + 1]; *tot = the candidates' total
// (one 4-byte copy; the offsets travel with it when offsets_host is given).  Synchronises the stream.
int cand_count_rows(sph_ctx* c, const CandP& q, uint32_t* offsets_host, uint32_t* tot);
// tot > 0, after cand_count_rows with the same q: the rows' entries into cand_idx[tot].  Queues the launch, does not wait.
int cand_fill_rows(sph_ctx* c, const CandP& q, uint32_t tot);
