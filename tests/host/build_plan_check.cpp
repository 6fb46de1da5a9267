// TEST-ONLY driver of csrc/sph_grid_plan.hpp (the grids of a neighbour build and the admission of the incremental sort) on the CPU:
// reads cases from stdin, one per line, and prints what the header decides; tests/test_build_plan_host.py compares.  Floats travel as
// the hex of their f32 bits.  Built with plain g++ under AddressSanitizer + UBSan; no HIP.
//
//   sorting <min_x> <min_y> <max_x> <max_y> <h_min> <h_max> <uniform> <empty>
//       -> sorting <coarse sx sy> <sort minx miny sx sy> <doublings, -1: fallback> <tile_ts tsx tsy>   |   sorting refused
//   grid <min_x> <min_y> <max_x> <max_y> <cs> <margin>      -> grid <minx miny sx sy ncells>            |   grid refused
//   fits <ncells> <n>                                       -> fits 0|1
//   limit <n> <inc_sort>                                    -> limit <movers>
//   streak <count_valid> <movers> <limit> <streak> <calls>  -> streak <result of every call> / <streak afterwards>
#include <cstdio>
#include <cstring>

#include "sph_grid_plan.hpp"

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
        if (!strcmp(cmd, "sorting")) {
            unsigned b[6];
            int uniform, empty;
            if (scanf("%x %x %x %x %x %x %d %d", &b[0], &b[1], &b[2], &b[3], &b[4], &b[5], &uniform, &empty) != 8) return 2;
            const float h_min = f32(b[4]), h_max = f32(b[5]);
            SortGridPlan sg;
            if (!plan_sorting_grid(GridBox{f32(b[0]), f32(b[1]), f32(b[2]), f32(b[3])}, empty != 0, h_min, h_max, uniform != 0, sg)) {
                printf("sorting refused\n");
                continue;
            }
            int doublings = sg.tile_ts == 1 ? -1 : 0;
            if (sg.tile_ts > 1)
                for (float cs = h_min * 2.f; cs != sg.sort.cs && doublings < 64; cs *= 2.f) doublings++;
            printf("sorting %d %d %d %d %d %d %d %d %d %d\n", sg.coarse.sx, sg.coarse.sy, sg.sort.minx, sg.sort.miny, sg.sort.sx, sg.sort.sy, doublings, sg.tile_ts,
                   sg.tile_tsx, sg.tile_tsy);
        } else if (!strcmp(cmd, "grid")) {
            unsigned b[5];
            int margin;
            if (scanf("%x %x %x %x %x %d", &b[0], &b[1], &b[2], &b[3], &b[4], &margin) != 6) return 2;
            GridP g;
            if (plan_grid(GridBox{f32(b[0]), f32(b[1]), f32(b[2]), f32(b[3])}, f32(b[4]), margin, g))
                printf("grid %d %d %d %d %u\n", g.minx, g.miny, g.sx, g.sy, g.ncells);
            else
                printf("grid refused\n");
        } else if (!strcmp(cmd, "fits")) {
            unsigned ncells, n;
            if (scanf("%u %u", &ncells, &n) != 2) return 2;
            printf("fits %d\n", inc_sort_fits(ncells, n) ? 1 : 0);
        } else if (!strcmp(cmd, "limit")) {
            unsigned n;
            int inc_sort;
            if (scanf("%u %d", &n, &inc_sort) != 2) return 2;
            printf("limit %u\n", inc_sort_mover_limit(n, inc_sort));
        } else if (!strcmp(cmd, "streak")) {
            unsigned movers, limit;
            int valid, streak, calls;
            if (scanf("%d %u %u %d %d", &valid, &movers, &limit, &streak, &calls) != 5) return 2;
            printf("streak");
            for (int k = 0; k < calls; k++) printf(" %d", inc_sort_worthwhile(valid != 0, movers, limit, streak) ? 1 : 0);
            printf(" / %d\n", streak);
        } else {
            fprintf(stderr, "unknown case '%s'\n", cmd);
            return 2;
        }
    }
    return 0;
}
