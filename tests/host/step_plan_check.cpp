// TEST-ONLY driver of csrc/sph_step_plan.hpp (the step driver's host decisions: ghost widths, tile reach, first propagation batch, pacing,
// adoption / eligibility of the build queued ahead, admission of the slab merge) on the CPU: reads cases from stdin, one per line, and
// prints what the header decides; tests/test_step_plan_host.py compares.  Floats travel as the hex of their f32 bits.  Built with plain
// g++ under AddressSanitizer + UBSan; no HIP.
//
//   widths <level_on> <after> <multi> <last_dmax> <h_max_step> <range_k>     -> widths <slab_slack_k> <halo_base_k>
//   ext <want_ext> <range_k>                                                 -> ext <tiles>
//   reach <k> <h_max> <slack> <tile_ts> <cs>                                 -> reach <tiles>
//   batch <last_level_sweeps> <batch8>                                       -> batch <sweeps>
//   lead <n> <opt_lead>                                                      -> lead <iterations>
//   pred <n> <opt_pred> <last> <prev>                                        -> pred <iterations>
//   extend <k>                                                               -> extend <upto>
//   chain <opt_chain> <last_div> <prev_div>                                  -> chain 0|1
//   adopt <ahead: cs minx miny sx sy h_max h_min rest_density tile_ts n>
//         <step: usable valid dist_on exact uniform_h ctx_n n h_max h_min rest_density tile_ts cs minx miny sx sy>   -> adopt 0|1
//   eligible <multi> <paced> <opt> <h_from_mass> <constrain> <uniform_h> <exact> <tile_ts> <n>                       -> eligible 0|1
//   fused <opt_boundary_fused> <level_on> <hdr_partials>                     -> fused 0|1
//   merge <pre> <inc_sort> <prev_valid> <prev_cs> <prev_ncells> <cs> <ncells> <n_prev> <n_sort> <exact> <count_valid> <movers> <streak>
//                                                                            -> merge 0|1 / <streak afterwards>
#include <cstdio>
#include <cstring>

#include "sph_step_plan.hpp"

static float f32(unsigned bits)
{
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

int main()
{
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "widths")) {
            int level_on, after, multi;
            unsigned b[3];
            if (scanf("%d %d %d %x %x %x", &level_on, &after, &multi, &b[0], &b[1], &b[2]) != 6) return 2;
            printf("widths %.9g %.9g\n", (double)slab_slack_k(level_on != 0, after != 0, multi != 0, f32(b[0]), f32(b[1])), (double)halo_base_k(level_on != 0, f32(b[2])));
        } else if (!strcmp(cmd, "ext")) {
            int want;
            unsigned b;
            if (scanf("%d %x", &want, &b) != 2) return 2;
            printf("ext %d\n", ext_tile_reach(want != 0, f32(b)));
        } else if (!strcmp(cmd, "reach")) {
            unsigned b[3], cs;
            int ts;
            if (scanf("%x %x %x %d %x", &b[0], &b[1], &b[2], &ts, &cs) != 5) return 2;
            printf("reach %d\n", slack_tile_reach(f32(b[0]), f32(b[1]), f32(b[2]), ts, f32(cs)));
        } else if (!strcmp(cmd, "batch")) {
            unsigned last;
            int batch8;
            if (scanf("%u %d", &last, &batch8) != 2) return 2;
            printf("batch %d\n", level_first_batch(last, batch8 != 0));
        } else if (!strcmp(cmd, "lead")) {
            unsigned n;
            int opt;
            if (scanf("%u %d", &n, &opt) != 2) return 2;
            printf("lead %u\n", pace_lead(n, opt));
        } else if (!strcmp(cmd, "pred")) {
            unsigned n, last, prev;
            int opt;
            if (scanf("%u %d %u %u", &n, &opt, &last, &prev) != 4) return 2;
            printf("pred %u\n", pace_prediction(n, opt, last, prev));
        } else if (!strcmp(cmd, "extend")) {
            unsigned k;
            if (scanf("%u", &k) != 1) return 2;
            printf("extend %u\n", solve_extend_upto(k));
        } else if (!strcmp(cmd, "chain")) {
            int opt;
            unsigned last, prev;
            if (scanf("%d %u %u", &opt, &last, &prev) != 3) return 2;
            printf("chain %d\n", chain_wanted(opt, last, prev) ? 1 : 0);
        } else if (!strcmp(cmd, "adopt")) {
            AheadBuild a;
            StepBuild s{};
            unsigned acs, ah[3], scs, sh[3];
            unsigned long long an, ctx_n;
            int f[5];
            if (scanf("%x %d %d %d %d %x %x %x %d %llu", &acs, &a.g.minx, &a.g.miny, &a.g.sx, &a.g.sy, &ah[0], &ah[1], &ah[2], &a.tile_ts, &an) != 10) return 2;
            if (scanf("%d %d %d %d %d %llu %u %x %x %x %d %x %d %d %d %d", &f[0], &f[1], &f[2], &f[3], &f[4], &ctx_n, &s.n, &sh[0], &sh[1], &sh[2], &s.tile_ts, &scs,
                      &s.g.minx, &s.g.miny, &s.g.sx, &s.g.sy) != 16)
                return 2;
            a.g.cs = f32(acs);
            a.h_max = f32(ah[0]);
            a.h_min = f32(ah[1]);
            a.rest_density = f32(ah[2]);
            a.n = an;
            s.ahead_usable = f[0] != 0;
            s.ahead_valid = f[1] != 0;
            s.dist_on = f[2] != 0;
            s.exact = f[3] != 0;
            s.uniform_h = f[4] != 0;
            s.ctx_n = ctx_n;
            s.h_max = f32(sh[0]);
            s.h_min = f32(sh[1]);
            s.rest_density = f32(sh[2]);
            s.g.cs = f32(scs);
            printf("adopt %d\n", adopt_ahead_build(a, s) ? 1 : 0);
        } else if (!strcmp(cmd, "eligible")) {
            int f[7];
            AheadWish w{};
            if (scanf("%d %d %d %d %d %d %d %d %u", &f[0], &f[1], &f[2], &f[3], &f[4], &f[5], &f[6], &w.tile_ts, &w.n) != 9) return 2;
            w.multi = f[0] != 0;
            w.paced = f[1] != 0;
            w.opt_ahead_build = f[2] != 0;
            w.h_from_mass = f[3] != 0;
            w.constrain_neighborhood_count = f[4] != 0;
            w.uniform_h = f[5] != 0;
            w.exact = f[6] != 0;
            printf("eligible %d\n", ahead_build_eligible(w) ? 1 : 0);
        } else if (!strcmp(cmd, "fused")) {
            int f[3];
            if (scanf("%d %d %d", &f[0], &f[1], &f[2]) != 3) return 2;
            printf("fused %d\n", ahead_build_fused(f[0] != 0, f[1] != 0, f[2] != 0) ? 1 : 0);
        } else if (!strcmp(cmd, "merge")) {
            SlabSort s{};
            int pre, prev_valid, exact, count_valid, streak;
            unsigned prev_cs, cs;
            if (scanf("%d %d %d %x %u %x %u %u %u %d %d %u %d", &pre, &s.inc_sort, &prev_valid, &prev_cs, &s.prev_ncells, &cs, &s.ncells, &s.n_prev, &s.n_sort, &exact,
                      &count_valid, &s.movers, &streak) != 13)
                return 2;
            s.pre = pre != 0;
            s.prev_valid = prev_valid != 0;
            s.prev_cs = f32(prev_cs);
            s.cs = f32(cs);
            s.exact = exact != 0;
            s.count_valid = count_valid != 0;
            const bool merge = slab_merge_admitted(s, streak);
            printf("merge %d / %d\n", merge ? 1 : 0, streak);
        } else {
            fprintf(stderr, "unknown case '%s'\n", cmd);
            return 2;
        }
    }
    return 0;
}
