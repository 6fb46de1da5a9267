// TEST-ONLY driver of csrc/sph_boundary_fused.hpp (the index arithmetic of the fused step boundary: the two-level cell-range table of
// k_inc_count / k_inc_place_reorder and the visiting order of the header reduction) on the CPU: reads cases from stdin, one per line;
// tests/test_boundary_fused_host.py compares.  Built with plain g++ under AddressSanitizer + UBSan; no HIP.
//
//   prefix <ncells> <seed>   the populations count(c) = lcg >> 24 mod 7 laid out as the count launch leaves them -- local[c]: exclusive
//                            prefix within the cell's block of INC_CELLS, bpre[b]: exclusive prefix of the block sums, the total last --
//                            and inc_cell_first(local, bpre, c) against the plain exclusive scan for every cell
//                            -> prefix ok <blocks> <total>          |   prefix BAD <first cell that differs>
//   header <nparts> <seed>   partials from the same generator, reduced in the workgroup's order (lane t: trips t, t + 4 * 1024, ..., four
//                            slots header_ahead_slot each; lanes, then waves in index order) against a plain loop over the partials
//                            -> header ok <distinct partials visited> <loads>   |   header BAD
#include <cstdio>
#include <cstring>
#include <vector>

#include "sph_boundary_fused.hpp"

static uint32_t lcg(uint32_t& x)
{
    x = x * 1664525u + 1013904223u;
    return x;
}

static bool same(const HeaderOut& a, const HeaderOut& b) { return memcmp(&a, &b, sizeof(float) * 7) == 0; }

int main()
{
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "prefix")) {
            uint32_t ncells, seed;
            if (scanf("%u %u", &ncells, &seed) != 2) return 2;
            std::vector<uint32_t> count(ncells), local(ncells + 1u, 0xdeadbeefu), plain(ncells + 1u);
            for (auto& c : count) c = (lcg(seed) >> 24) % 7u;
            const uint32_t blocks = inc_count_blocks(ncells);
            std::vector<uint32_t> bsum(blocks), bpre(blocks + 1u);
            for (uint32_t b = 0; b < blocks; b++) {   // one count block
                uint32_t run = 0;
                for (uint32_t t = 0; t < (uint32_t)INC_CELLS; t++) {
                    const uint32_t c = b * (uint32_t)INC_CELLS + t;
                    if (c >= ncells) break;
                    local[c] = run;
                    run += count[c];
                }
                bsum[b] = run;
            }
            uint32_t carry = 0;   // the block that finishes last
            for (uint32_t b = 0; b < blocks; b++) {
                bpre[b] = carry;
                carry += bsum[b];
            }
            bpre[blocks] = carry;
            uint32_t run = 0;
            for (uint32_t c = 0; c < ncells; c++) {
                plain[c] = run;
                run += count[c];
            }
            plain[ncells] = run;
            long bad = -1;
            for (uint32_t c = 0; c < ncells && bad < 0; c++)
                if (inc_cell_first(local.data(), bpre.data(), c) != plain[c]) bad = (long)c;
            if (bad < 0 && bpre[inc_count_blocks(ncells)] != plain[ncells]) bad = (long)ncells;
            if (bad >= 0) printf("prefix BAD %ld\n", bad);
            else printf("prefix ok %u %u\n", blocks, plain[ncells]);
        } else if (!strcmp(cmd, "header")) {
            uint32_t nparts, seed;
            if (scanf("%u %u", &nparts, &seed) != 2 || nparts == 0u) return 2;
            std::vector<HeaderOut> part(nparts);
            auto val = [&]() { return (float)(int)(lcg(seed) >> 8) / 65536.f - 128.f; };
            for (auto& q : part) {
                q = HeaderOut{val(), val(), val(), val(), val() + 128.f, val() + 128.f, val() + 128.f, 0u};
            }
            HeaderOut plain = header_neutral();
            for (const auto& q : part) header_merge(plain, q);
            std::vector<uint32_t> visits(nparts, 0u);
            unsigned long loads = 0;
            HeaderOut total = header_neutral();
            bool first_wave = true;
            for (uint32_t w = 0; w < HDR_AHEAD_THREADS / 64u; w++) {
                HeaderOut wave = header_neutral();
                for (uint32_t lane = 0; lane < 64u; lane++) {
                    HeaderOut o = header_neutral();
                    for (uint32_t k0 = w * 64u + lane; k0 < nparts; k0 += 4u * HDR_AHEAD_THREADS)
                        for (uint32_t u = 0; u < 4u; u++) {
                            const uint32_t k = header_ahead_slot(k0, u, nparts);
                            if (k >= nparts) {
                                printf("header BAD\n");
                                return 0;
                            }
                            visits[k]++;
                            loads++;
                            header_merge(o, part[k]);
                        }
                    header_merge(wave, o);
                }
                if (first_wave) total = wave;
                else header_merge(total, wave);
                first_wave = false;
            }
            uint32_t distinct = 0;
            for (uint32_t v : visits) distinct += v ? 1u : 0u;
            if (!same(total, plain) || total.pad != 0u) printf("header BAD\n");
            else printf("header ok %u %lu\n", distinct, loads);
        } else
            return 2;
    }
    return 0;
}
