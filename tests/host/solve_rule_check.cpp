// TEST-ONLY driver of csrc/sph_solve_rule.hpp (the pressure solve's stop rule and the progress word of a paced solve) on the CPU: reads
// cases from stdin, one per line; tests/test_solve_rule_host.py compares.  Built with plain g++ under AddressSanitizer + UBSan; no HIP.
// Floats travel as the hexadecimal bit patterns of their float32 values, so that no conversion rounds.
//
//   stop <residual_density> <max_avg_error> <max_iters> <normal> <sum_err> <iter> <rest_density> <dt>
//                            -> stop <0|1>                               solver_stop_rule
//   word <epoch> <stop> <iter> <reader's epoch>
//                            -> word <hex word> <seen> <stopped> <decided>   prog_word, read back with prog_seen / _stopped / _decided
//   next <epoch>             -> next <prog_next_epoch(epoch)>
//   cycle <start>            65536 steps of prog_next_epoch from <start>; at every step the epoch e it yields is asked whether it "sees" a
//                            zeroed word and the words (both stop bits, iterations 0 and PROG_MAX_ITERS) of the epoch in front of it
//                            -> cycle <zeros yielded> <zeroed words seen> <previous epoch's words seen> <distinct epochs> <last epoch>
//   limits                   -> limits <PROG_MAX_ITERS>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sph_solve_rule.hpp"

static float as_float(uint32_t bits)
{
    float f;
    memcpy(&f, &bits, sizeof f);
    return f;
}

int main()
{
    char cmd[32];
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "stop")) {
            int residual_density, iter;
            uint32_t err, max_iters, normal, sum, rest, dt;
            if (scanf("%d %x %u %u %x %d %x %x", &residual_density, &err, &max_iters, &normal, &sum, &iter, &rest, &dt) != 8) return 2;
            const SolveRule rule{residual_density, as_float(err), max_iters};
            printf("stop %d\n", solver_stop_rule(normal, as_float(sum), iter, rule, as_float(rest), as_float(dt)) ? 1 : 0);
        } else if (!strcmp(cmd, "word")) {
            uint32_t epoch, stop, iter, reader;
            if (scanf("%u %u %u %u", &epoch, &stop, &iter, &reader) != 4) return 2;
            const uint32_t w = prog_word(epoch, stop != 0u, iter);
            printf("word %x %d %d %u\n", w, prog_seen(w, reader) ? 1 : 0, prog_stopped(w) ? 1 : 0, prog_decided(w));
        } else if (!strcmp(cmd, "next")) {
            uint32_t epoch;
            if (scanf("%u", &epoch) != 1) return 2;
            printf("next %u\n", prog_next_epoch(epoch));
        } else if (!strcmp(cmd, "cycle")) {
            uint32_t e;
            if (scanf("%u", &e) != 1) return 2;
            std::vector<uint8_t> met(0x10000u, 0);
            uint32_t zeros = 0, zeroed_seen = 0, previous_seen = 0, distinct = 0;
            for (uint32_t step = 0; step < 0x10000u; step++) {
                const uint32_t before = e;
                e = prog_next_epoch(e);
                if (e > 0xffffu) return 3;   // (an epoch must fit the word's upper half)
                zeros += e == 0u ? 1u : 0u;
                zeroed_seen += prog_seen(0u, e) ? 1u : 0u;
                for (uint32_t stop = 0; stop < 2u; stop++)
                    for (uint32_t iter : {0u, (uint32_t)PROG_MAX_ITERS}) previous_seen += prog_seen(prog_word(before, stop != 0u, iter), e) ? 1u : 0u;
                distinct += met[e] ? 0u : 1u;
                met[e] = 1;
            }
            printf("cycle %u %u %u %u %u\n", zeros, zeroed_seen, previous_seen, distinct, e);
        } else if (!strcmp(cmd, "limits")) {
            printf("limits %u\n", (uint32_t)PROG_MAX_ITERS);
        } else
            return 2;
    }
    return 0;
}
