// The relay's schedule (csrc/sph_relay_plan.hpp: relay_rounds, relay_sub_rounds, relay_step -- what sph_relay_plan lists and what
// relay_gather / relay_bcast walk) as a program of its own for the CPU, to be built with -fsanitize=address,undefined
// (tests/test_relay_plan_sanitized.py).  It executes the plans of all ranks side by side over byte vectors: a message is what the sender's
// step names, copied to where the receiver's step puts it; every leg is checked against the blob it names before it is used.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sph_relay_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            failures++;                   \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
        }                                 \
    } while (0)

static bool same_leg(const sph_relay_leg& a, const sph_relay_leg& b) { return a.origin == b.origin && a.offset == b.offset && a.bytes == b.bytes; }

static void run(int n, int root, bool outwards, const std::vector<uint64_t>& bytes, uint64_t chunk)
{
    // data[r][o]: what rank r holds of blob o; have[r][o]: which bytes of it
    std::vector<std::vector<std::vector<uint8_t>>> data((size_t)n, std::vector<std::vector<uint8_t>>((size_t)n)), have = data;
    for (int r = 0; r < n; r++)
        for (int o = 0; o < n; o++) {
            data[(size_t)r][(size_t)o].assign((size_t)bytes[(size_t)o], 0);
            have[(size_t)r][(size_t)o].assign((size_t)bytes[(size_t)o], 0);
        }
    for (int o = 0; o < n; o++) {
        if (outwards && o != root) continue;
        for (size_t b = 0; b < bytes[(size_t)o]; b++) {
            data[(size_t)o][(size_t)o][b] = (uint8_t)(131 * o + 7 * b + 1);
            have[(size_t)o][(size_t)o][b] = 1;
        }
    }
    struct Arrival {
        int dst;
        sph_relay_leg leg;
        std::vector<uint8_t> payload;
    };
    for (int t = 1; t <= relay_rounds(n, root); t++) {
        const uint64_t subs = relay_sub_rounds(n, root, outwards, bytes.data(), chunk, t);
        for (uint64_t s = 0; s < subs; s++) {
            std::vector<sph_relay_step> st;
            for (int r = 0; r < n; r++) st.push_back(relay_step(n, root, r, outwards, bytes.data(), chunk, t, s));
            CHECK(st[0].send[0].bytes == 0 && st[0].recv[0].bytes == 0 && st[(size_t)n - 1].send[1].bytes == 0 && st[(size_t)n - 1].recv[1].bytes == 0,
                  "a message across the outer edge (n=%d root=%d)", n, root);
            std::vector<Arrival> arriving;
            for (int r = 0; r + 1 < n; r++) {
                const int ends[2][4] = {{r, 1, r + 1, 0}, {r + 1, 0, r, 1}};
                for (auto& e : ends) {
                    const sph_relay_leg sent = st[(size_t)e[0]].send[e[1]], taken = st[(size_t)e[2]].recv[e[3]];
                    CHECK(sent.bytes == taken.bytes, "pair (%d, %d) disagrees: %llu sent, %llu expected (n=%d root=%d t=%d)", e[0], e[2], (unsigned long long)sent.bytes,
                          (unsigned long long)taken.bytes, n, root, t);
                    if (!sent.bytes || sent.bytes != taken.bytes) continue;
                    CHECK(same_leg(sent, taken), "pair (%d, %d) names different messages", e[0], e[2]);
                    CHECK(sent.bytes <= chunk, "a message of %llu bytes", (unsigned long long)sent.bytes);
                    if (sent.origin >= (uint64_t)n || sent.offset + sent.bytes > bytes[(size_t)sent.origin]) {
                        CHECK(false, "a leg outside its blob");
                        continue;
                    }
                    Arrival a{e[2], sent, {}};
                    for (uint64_t b = 0; b < sent.bytes; b++) {
                        CHECK(have[(size_t)e[0]][(size_t)sent.origin][(size_t)(sent.offset + b)], "rank %d forwards a byte it does not hold", e[0]);
                        a.payload.push_back(data[(size_t)e[0]][(size_t)sent.origin][(size_t)(sent.offset + b)]);
                    }
                    arriving.push_back(a);
                }
            }
            for (const Arrival& a : arriving)
                for (uint64_t b = 0; b < a.leg.bytes; b++) {
                    CHECK(!have[(size_t)a.dst][(size_t)a.leg.origin][(size_t)(a.leg.offset + b)], "a byte received twice");
                    data[(size_t)a.dst][(size_t)a.leg.origin][(size_t)(a.leg.offset + b)] = a.payload[(size_t)b];
                    have[(size_t)a.dst][(size_t)a.leg.origin][(size_t)(a.leg.offset + b)] = 1;
                }
        }
    }
    for (int r = 0; r < n; r++) {
        if (!outwards && r != root) continue;
        for (int o = 0; o < n; o++) {
            if (outwards && o != root) continue;
            for (size_t b = 0; b < bytes[(size_t)o]; b++)
                CHECK(have[(size_t)r][(size_t)o][b] && data[(size_t)r][(size_t)o][b] == (uint8_t)(131 * o + 7 * b + 1), "rank %d lacks byte %zu of blob %d (n=%d root=%d outwards=%d)",
                      r, b, o, n, root, (int)outwards);
        }
    }
}

int main()
{
    int cases = 0;
    for (uint64_t chunk : {(uint64_t)16, (uint64_t)4096}) {
        const uint64_t edge[5] = {0, 1, chunk, chunk + 1, 3 * chunk + 17};
        for (int n = 1; n <= 6; n++)
            for (int root = 0; root < n; root++)
                for (int shift = 0; shift < 5; shift++) {
                    std::vector<uint64_t> bytes((size_t)n);
                    for (int r = 0; r < n; r++) bytes[(size_t)r] = edge[(r + shift) % 5];
                    run(n, root, false, bytes, chunk);
                    run(n, root, true, bytes, chunk);
                    cases += 2;
                }
    }
    fprintf(stderr, "relay plan: %d case(s), %d failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}
