// TEST-ONLY driver of the rank arithmetic in csrc/sph_boundary_fused.hpp (k_inc_place_reorder: a stayer's rank among the stayers of
// its cell from the wave's ballot plus a loop over the bytes in front of the wave; a mover's range in the cell it enters) on the CPU:
// reads cases from stdin, one per line; tests/test_boundary_chains_host.py compares.  Built with plain g++ under AddressSanitizer +
// UBSan; no HIP.
//
//   rank <ncells> <seed> <maxpop> <long_every> <mover_permille>
//        cells with populations lcg >> 24 mod (maxpop + 1), every long_every-th cell (0: none) 70 particles longer; flag bytes: a mover
//        with the given probability, which enters a cell drawn by the generator.  The array is cut into workgroups of 256 and waves of
//        64 as the place launch does; for every particle the rank from the ballot word + the outside loop (stayers), or the count over
//        the range inc_mover_range_end selects (movers), against a plain count of the stayers of the new cell in front of it.
//        -> rank ok <n> <stayers whose cell starts in front of their wave> <cells spanning two workgroups> <cells longer than 64>
//                   <empty cells> <movers from in front of the entered range> <movers from behind it> <particles in the last workgroup>
//         | rank BAD <first particle that differs>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sph_boundary_fused.hpp"

static uint32_t lcg(uint32_t& x)
{
    x = x * 1664525u + 1013904223u;
    return x;
}

static uint32_t popcount64(uint64_t v)
{
    uint32_t r = 0;
    for (; v; v &= v - 1ull) r++;
    return r;
}

int main()
{
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (strcmp(cmd, "rank")) return 2;
        uint32_t ncells, seed, maxpop, long_every, permille;
        if (scanf("%u %u %u %u %u", &ncells, &seed, &maxpop, &long_every, &permille) != 5 || ncells == 0u) return 2;
        std::vector<uint32_t> start(ncells + 1u);
        uint32_t n = 0, empty = 0, longer = 0, two_groups = 0;
        for (uint32_t c = 0; c < ncells; c++) {
            uint32_t pop = (lcg(seed) >> 24) % (maxpop + 1u);
            if (long_every && c % long_every == long_every - 1u) pop += 70u;
            start[c] = n;
            n += pop;
            empty += pop == 0u;
            longer += pop > 64u;
            two_groups += pop > 0u && start[c] / 256u != (n - 1u) / 256u;
        }
        start[ncells] = n;
        std::vector<uint8_t> mv(n);
        std::vector<uint32_t> cell(n), enters(n);
        for (uint32_t c = 0; c < ncells; c++)
            for (uint32_t i = start[c]; i < start[c + 1u]; i++) {
                cell[i] = c;
                mv[i] = (lcg(seed) >> 16) % 1000u < permille ? 1 : 0;
                enters[i] = (lcg(seed) >> 8) % ncells;
                if (mv[i] && enters[i] == c) mv[i] = 0;   // (a mover changes its cell)
            }
        long bad = -1;
        uint32_t outside = 0, from_front = 0, from_behind = 0;
        for (uint32_t g0 = 0; g0 < n && bad < 0; g0 += 256u)          // one workgroup
            for (uint32_t w0 = g0; w0 < g0 + 256u && w0 < n && bad < 0; w0 += 64u) {   // one wave: lane l holds particle w0 + l
                uint64_t stay = 0;
                for (uint32_t l = 0; l < 64u; l++)
                    if (w0 + l < n && mv[w0 + l] == 0) stay |= 1ull << l;   // (a lane past the last particle is no stayer)
                for (uint32_t l = 0; l < 64u && w0 + l < n; l++) {
                    const uint32_t i = w0 + l;
                    uint32_t got = 0, plain = 0;
                    if (mv[i] == 0) {
                        const uint32_t b = start[cell[i]], e = inc_rank_outside_end(w0, b);
                        if (e > i || (b >= w0 && e != b)) { bad = (long)i; break; }
                        for (uint32_t j = b; j < e; j++) got += mv[j] ? 0u : 1u;
                        outside += e > b;
                        got += popcount64(stay & inc_rank_ballot_lanes(w0, b, i));
                        for (uint32_t j = b; j < i; j++) plain += mv[j] ? 0u : 1u;
                    } else {
                        const uint32_t b = start[enters[i]], eb = start[enters[i] + 1u], e = inc_mover_range_end(i, b, eb);
                        for (uint32_t j = b; j < e; j++) got += mv[j] ? 0u : 1u;
                        for (uint32_t j = b; j < eb; j++) plain += (mv[j] == 0 && j < i) ? 1u : 0u;
                        from_front += i < b;
                        from_behind += i >= eb;
                    }
                    if (got != plain) { bad = (long)i; break; }
                }
            }
        if (bad >= 0) printf("rank BAD %ld\n", bad);
        else printf("rank ok %u %u %u %u %u %u %u %u\n", n, outside, two_groups, longer, empty, from_front, from_behind, n ? (n - 1u) % 256u + 1u : 0u);
    }
    return 0;
}
