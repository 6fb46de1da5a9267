// The relay's schedule (include/sph_rank_partner_search.h, THE RELAY) as plain host arithmetic: no device, no context, no transport.
// sph_relay_plan lists it, relay_gather / relay_bcast (sph_relay.hip) walk it -- the same two functions below serve both, so what the
// host test simulates is what runs.
#pragma once

#include <algorithm>
#include <cstdint>

#include "sph_rank_partner_search.h"

// rounds of a relay to / from `root` in a row of n ranks
inline int relay_rounds(int n, int root) { return std::max(root, n - 1 - root); }

inline uint64_t relay_chunks(uint64_t bytes, uint64_t chunk) { return bytes / chunk + (bytes % chunk ? 1u : 0u); }

// sub-rounds of round t (1-based): what the largest blob under way in it takes.  Gather: the blobs that started t or more hops away.
// Broadcast: the root's blob.
inline uint64_t relay_sub_rounds(int n, int root, bool outwards, const uint64_t* bytes, uint64_t chunk, int t)
{
    if (outwards) return relay_chunks(bytes[root], chunk);
    uint64_t s = 0;
    for (int o = 0; o < n; o++)
        if (std::abs(root - o) >= t) s = std::max(s, relay_chunks(bytes[o], chunk));
    return s;
}

// chunk s of rank o's blob
inline sph_relay_leg relay_leg(int o, const uint64_t* bytes, uint64_t chunk, uint64_t s)
{
    const uint64_t off = s * chunk;
    if (off >= bytes[o]) return sph_relay_leg{0, 0, 0};
    return sph_relay_leg{(uint64_t)o, off, std::min(chunk, bytes[o] - off)};
}

// what `rank` does in sub-round s of round t
inline sph_relay_step relay_step(int n, int root, int rank, bool outwards, const uint64_t* bytes, uint64_t chunk, int t, uint64_t s)
{
    sph_relay_step st{};
    st.round = (uint32_t)t;
    st.sub_round = (uint32_t)s;
    if (outwards) {   // the root's blob: rank root -/+ (t - 1) passes it on to rank root -/+ t
        if (rank == root - (t - 1) && rank - 1 >= 0) st.send[0] = relay_leg(root, bytes, chunk, s);
        if (rank == root + (t - 1) && rank + 1 < n) st.send[1] = relay_leg(root, bytes, chunk, s);
        if (rank == root - t) st.recv[1] = relay_leg(root, bytes, chunk, s);
        if (rank == root + t) st.recv[0] = relay_leg(root, bytes, chunk, s);
        return st;
    }
    // towards the root: blob o is at rank o +/- (t - 1) when round t begins, if it has not arrived
    if (rank < root && rank - (t - 1) >= 0) st.send[1] = relay_leg(rank - (t - 1), bytes, chunk, s);
    if (rank > root && rank + (t - 1) < n) st.send[0] = relay_leg(rank + (t - 1), bytes, chunk, s);
    if (rank <= root && rank - t >= 0) st.recv[0] = relay_leg(rank - t, bytes, chunk, s);
    if (rank >= root && rank + t < n) st.recv[1] = relay_leg(rank + t, bytes, chunk, s);
    return st;
}
