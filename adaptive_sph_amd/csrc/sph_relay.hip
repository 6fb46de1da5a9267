// A gather to one rank and a broadcast from it as a RELAY ALONG THE ROW of ranks, on Comm::exchange alone (sph_dist.hpp: relay_gather,
// relay_bcast; include/sph_rank_partner_search.h: THE RELAY and sph_relay_plan).  No transport code: whatever moves a halo between
// x-neighbours moves these messages, and all ordering is exchange's -- no kernel here, no flag, no wait of its own.
//
// Why it cannot deadlock.  Both ends of a pair derive a sub-round's byte counts from the same table with the same function
// (sph_relay_plan.hpp), so they enter the pair in the same sub-rounds, and every transport takes the left side of an exchange before the
// right one.  Order the meetings by (sub-round, pair index): every rank goes through its own meetings in that order, so the earliest
// meeting still outstanding has both its ranks free to come.  A rank that fails leaves through rank_entry, which abandons the transport:
// the others' rendezvous reports it instead of waiting (THE COLLECTIVE RULE, sph_dist.hpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "sph_dist.hpp"
#include "sph_relay_plan.hpp"

extern "C" int sph_relay_plan(int n_ranks, int root, int rank, int outwards, const uint64_t* bytes_of_rank, uint64_t chunk_bytes, sph_relay_step* steps,
                              uint64_t steps_capacity, uint64_t* n_steps)
{
    if (n_steps) *n_steps = 0;
    if (n_ranks < 1 || root < 0 || root >= n_ranks || rank < 0 || rank >= n_ranks || !bytes_of_rank || !n_steps || chunk_bytes == 0) return SPH_ERR_INVALID_ARGUMENT;
    const int rounds = relay_rounds(n_ranks, root);
    uint64_t total = 0;
    for (int t = 1; t <= rounds; t++) total += relay_sub_rounds(n_ranks, root, outwards != 0, bytes_of_rank, chunk_bytes, t);
    *n_steps = total;
    if (!steps) return SPH_OK;
    if (steps_capacity < total) return SPH_ERR_INVALID_ARGUMENT;
    uint64_t k = 0;
    for (int t = 1; t <= rounds; t++) {
        const uint64_t subs = relay_sub_rounds(n_ranks, root, outwards != 0, bytes_of_rank, chunk_bytes, t);
        for (uint64_t s = 0; s < subs; s++) steps[k++] = relay_step(n_ranks, root, rank, outwards != 0, bytes_of_rank, chunk_bytes, t, s);
    }
    return SPH_OK;
}

// base[o]: where rank o's blob begins in buf
static int relay_run(Group& G, int root, bool outwards, const uint64_t* bytes, const uint64_t* base, uint64_t chunk, uint8_t* buf, uint64_t* sent, uint64_t* received)
{
    sph_ctx* c = G.m[0];
    const int n = c->dist.nranks, rank = c->dist.rank;
    if (G.m.size() != 1 || !G.comm) return c->fail(SPH_ERR_INVALID_ARGUMENT, "the relay serves a rank on its own transport");
    if (chunk < 16 || chunk % 16) return c->fail(SPH_ERR_INVALID_ARGUMENT, "relay messages of %llu bytes", (unsigned long long)chunk);
    std::vector<Xfer> x(1);
    const int rounds = relay_rounds(n, root);
    for (int t = 1; t <= rounds; t++) {
        const uint64_t subs = relay_sub_rounds(n, root, outwards, bytes, chunk, t);
        for (uint64_t s = 0; s < subs; s++) {
            const sph_relay_step st = relay_step(n, root, rank, outwards, bytes, chunk, t, s);
            Xfer& xf = x[0];
            memset(&xf, 0, sizeof xf);
            void* room[2] = {nullptr, nullptr};
            for (int side = 0; side < 2; side++) {
                if (st.send[side].bytes) {
                    xf.send[side] = buf + base[st.send[side].origin] + st.send[side].offset;
                    xf.send_bytes[side] = (size_t)st.send[side].bytes;
                }
                if (st.recv[side].bytes) {
                    room[side] = buf + base[st.recv[side].origin] + st.recv[side].offset;
                    xf.recv[side] = room[side];
                    xf.recv_bytes[side] = (size_t)st.recv[side].bytes;
                }
            }
            if (!xf.send_bytes[0] && !xf.send_bytes[1] && !xf.recv_bytes[0] && !xf.recv_bytes[1]) continue;   // (idle in this sub-round; so are both neighbours towards this rank)
            if (int rc = G.comm->exchange(G, x)) return rc;
            // Xfer::recv is an OUT parameter: a transport may hand back its own buffer (the push transport's inbox, which it writes again two
            // exchanges later): the chunk is copied to its place on the stream before the next exchange is queued
            for (int side = 0; side < 2; side++)
                if (xf.recv_bytes[side] && xf.recv[side] != room[side])
                    HIPCHK(c, hipMemcpyAsync(room[side], xf.recv[side], xf.recv_bytes[side], hipMemcpyDeviceToDevice, c->stream));
            if (sent) *sent += xf.send_bytes[0] + xf.send_bytes[1];
            if (received) *received += xf.recv_bytes[0] + xf.recv_bytes[1];
        }
    }
    return SPH_OK;
}

int relay_gather(Group& G, int root, const std::vector<uint64_t>& bytes, uint64_t chunk, uint8_t* buf, uint64_t* sent, uint64_t* received)
{
    std::vector<uint64_t> base(bytes.size() + 1, 0);
    for (size_t o = 0; o < bytes.size(); o++) base[o + 1] = base[o] + bytes[o];
    return relay_run(G, root, false, bytes.data(), base.data(), chunk, buf, sent, received);
}

int relay_bcast(Group& G, int root, uint64_t bytes, uint64_t chunk, uint8_t* buf, uint64_t* sent, uint64_t* received)
{
    std::vector<uint64_t> all((size_t)G.m[0]->dist.nranks, 0), base((size_t)G.m[0]->dist.nranks, 0);
    all[(size_t)root] = bytes;
    return relay_run(G, root, true, all.data(), base.data(), chunk, buf, sent, received);
}
