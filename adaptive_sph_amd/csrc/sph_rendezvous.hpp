// The rendezvous protocol of the thread and the shared-memory transport (sph_transport.hip), written once and free of HIP: plain host
// code that a host tool can look at (tests/host/rendezvous_check.cpp runs it under ThreadSanitizer / AddressSanitizer on the CPU).
//   two BOARDS   where the ranks meet: ThreadGroup (threads of one process: mutex and condvar) and ShmSegment (processes of one node:
//                atomics and spin in a segment all ranks map).  A board owns the per-rank slots, n, barrier(), pair_barrier(lower rank),
//                abandon() / the broken flag and its label for the messages
//   Rendezvous   the protocol over a board: meet (publish -> everybody is there -> consume -> everybody is done), the host-value
//                collectives on top of it, and the point-to-point skeleton of an exchange
// A collective that not every rank enters, or a send that no receive of the same size matches, is what would hang RCCL: here it is a
// time-out / an error.  Failures come back as the SPH_ERR_* code, the text in Rendezvous::err.
#pragma once

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <time.h>

#include "sph_ffi.h"

struct RefreshCounts {
    uint32_t mig[2], halo[2];         // this rank: migrants to / halo members (that stay) towards [left, right]
    uint32_t in_mig[2], in_halo[2];   // the neighbours': migrants for me / their halo members towards me, from [left, right]
    float hreg[2], in_hreg[2];        // largest h among this rank's particles in the region of its [left, right] cut; the neighbours' figure for the same cut
};

#define SHM_MAX_RANKS 16
#define SHM_MAX_F32 16     // capacities of a rank's slots on both boards (Comm::allreduce_sum_u32_dev chunks by SHM_MAX_U32)
#define SHM_MAX_U32 4096
// how long a rank waits for the others before the board is broken; per process, a caller may lower it (while no rank waits)
inline std::chrono::milliseconds rdv_wait_limit{60000};

// ---- threads: one HOST THREAD per rank, all ranks in this process (and on whatever devices their contexts name) -----------------
struct ThreadGroup {
    static constexpr const char* label = "thread transport";
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    std::atomic<bool> broken{false};
    // a ghost / migrant exchange is point to point, as ncclSend / ncclRecv are: rank r meets only the x-neighbours it sends to or
    // receives from (a rank with nothing for either neighbour does not enter at all).  One channel per adjacent pair (r, r + 1).
    struct PairChan {
        std::mutex mu;
        std::condition_variable cv;
        int arrived = 0;
        uint64_t gen = 0;
        uint64_t send_bytes[2][2], recv_bytes[2][2];   // [who: 0 the lower rank, 1 the upper][side]
        const void* send[2][2];                        // the sender's staging buffers: the receiver copies out of them
    };
    std::unique_ptr<PairChan[]> pair;
    std::vector<int32_t> op;          // which collective each rank is in (a mismatch is reported, not waited out)
    std::vector<std::array<double, 8>> tot;
    std::vector<std::array<float, SHM_MAX_F32>> f32rows;
    std::vector<std::array<uint32_t, SHM_MAX_U32>> u32rows;
    std::vector<uint32_t> f32len, u32len;
    std::vector<int32_t> i32vals;
    std::vector<std::array<uint32_t, 8>> words;
    explicit ThreadGroup(int k) : n(k), pair(new PairChan[(size_t)std::max(k - 1, 1)]), op(k), tot(k), f32rows(k), u32rows(k), f32len(k), u32len(k), i32vals(k), words(k) {}
    // the two ranks of a channel meet; false: the other one did not come (rdv_wait_limit) or somebody left with an error
    bool pair_barrier(int lower)
    {
        PairChan& ch = pair[(size_t)lower];
        std::unique_lock<std::mutex> lk(ch.mu);
        if (broken) return false;
        const uint64_t g = ch.gen;
        if (++ch.arrived == 2) {
            ch.arrived = 0;
            ch.gen++;
            ch.cv.notify_all();
            return true;
        }
        const auto t_end = std::chrono::steady_clock::now() + rdv_wait_limit;
        while (ch.gen == g && !broken) {
            if (ch.cv.wait_until(lk, std::min(t_end, std::chrono::steady_clock::now() + std::chrono::milliseconds(50))) == std::cv_status::timeout &&
                std::chrono::steady_clock::now() >= t_end) {
                broken = true;
                break;
            }
        }
        if (broken) ch.cv.notify_all();
        return ch.gen != g && !broken;
    }
    // all ranks meet; false: somebody did not come (rdv_wait_limit) or left with an error
    bool barrier()
    {
        std::unique_lock<std::mutex> lk(mu);
        if (broken) return false;
        const uint64_t g = gen;
        if (++arrived == n) {
            arrived = 0;
            gen++;
            cv.notify_all();
            return true;
        }
        if (!cv.wait_for(lk, rdv_wait_limit, [&] { return gen != g || broken; })) broken = true;
        if (broken) cv.notify_all();
        return !broken;
    }
    void abandon()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            broken = true;
            cv.notify_all();
        }
        for (int i = 0; i + 1 < n; i++) {   // (the pair waits poll `broken` every 50 ms as well)
            std::lock_guard<std::mutex> lk(pair[(size_t)i].mu);
            pair[(size_t)i].cv.notify_all();
        }
    }
};

// ---- processes of one node: the same slots and barriers in a POSIX shared-memory segment, ghost and migrant records staged through it --
struct ShmSegment {
    static constexpr const char* label = "shared-memory transport";
    static constexpr uint32_t MAGIC = 0x53504853u;
    uint32_t magic;   // written last by the creating rank
    uint32_t n;
    uint64_t bytes_per_side, total_bytes;
    std::atomic<uint32_t> arrived, gen, broken;
    struct Pair {
        std::atomic<uint32_t> arrived, gen;
        uint64_t send_bytes[2][2], recv_bytes[2][2];   // [who: 0 the lower rank, 1 the upper][side]
    } pair[SHM_MAX_RANKS];
    int32_t op[SHM_MAX_RANKS];
    double tot[SHM_MAX_RANKS][8];
    float f32rows[SHM_MAX_RANKS][SHM_MAX_F32];
    uint32_t f32len[SHM_MAX_RANKS];
    uint32_t u32rows[SHM_MAX_RANKS][SHM_MAX_U32];
    uint32_t u32len[SHM_MAX_RANKS];
    int32_t i32vals[SHM_MAX_RANKS];
    uint32_t words[SHM_MAX_RANKS][8];
    // followed by the outboxes: rank r, side s at payload() + (2 r + s) * bytes_per_side
    uint8_t* outbox(int r, int side) { return reinterpret_cast<uint8_t*>(this) + ((sizeof(ShmSegment) + 4095) & ~(size_t)4095) + ((size_t)2 * r + side) * bytes_per_side; }
    static size_t size_for(int n, uint64_t per_side) { return ((sizeof(ShmSegment) + 4095) & ~(size_t)4095) + (size_t)2 * n * per_side; }
    // the creating rank's part: `mem` = size_for(n, per_side) bytes that every rank maps
    static ShmSegment* create(void* mem, int n, uint64_t per_side)
    {
        memset(mem, 0, sizeof(ShmSegment));   // (the rest is zero-filled by whoever made the mapping)
        ShmSegment* g = (ShmSegment*)mem;
        g->n = (uint32_t)n;
        g->bytes_per_side = per_side;
        g->total_bytes = size_for(n, per_side);
        std::atomic_thread_fence(std::memory_order_release);
        g->magic = MAGIC;
        return g;
    }
    static bool spin_until(std::atomic<uint32_t>& word, uint32_t old, std::atomic<uint32_t>& broken)
    {
        const auto t_end = std::chrono::steady_clock::now() + rdv_wait_limit;
        for (uint32_t k = 0; word.load(std::memory_order_acquire) == old; k++) {
            if (broken.load(std::memory_order_relaxed)) return false;
            if ((k & 63u) == 63u) {
                if (std::chrono::steady_clock::now() >= t_end) {
                    broken.store(1u);
                    return false;
                }
                struct timespec ts = {0, 20000};
                nanosleep(&ts, nullptr);
            }
        }
        return !broken.load(std::memory_order_relaxed);
    }
    static bool meet_at(std::atomic<uint32_t>& arrived, std::atomic<uint32_t>& gen, uint32_t n, std::atomic<uint32_t>& broken)
    {
        if (broken.load()) return false;
        const uint32_t g = gen.load(std::memory_order_acquire);
        if (arrived.fetch_add(1u, std::memory_order_acq_rel) + 1u == n) {
            arrived.store(0u, std::memory_order_relaxed);
            gen.fetch_add(1u, std::memory_order_release);
            return true;
        }
        return spin_until(gen, g, broken);
    }
    bool barrier() { return meet_at(arrived, gen, n, broken); }
    bool pair_barrier(int lower) { return meet_at(pair[lower].arrived, pair[lower].gen, 2u, broken); }
    void abandon() { broken.store(1u); }
};

// ---- the protocol, for rank `r` of a board ------------------------------------------------------------------------------------------
template <class Board>
struct Rendezvous {
    Board& b;
    const int r;
    std::string err;   // the message of the failure a method returned
    Rendezvous(Board& board, int rank) : b(board), r(rank) {}
    int ranks() const { return (int)b.n; }
    int fail(int code, const char* fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    // publish -> everybody is there -> consume -> everybody is done (the slots may be overwritten again)
    template <class Pub, class Con>
    int meet(int opcode, Pub pub, Con con)
    {
        b.op[r] = opcode;
        pub();
        if (!b.barrier()) return fail(SPH_ERR_DEVICE, "%s: a rank did not enter collective %d (it would hang over RCCL)", Board::label, opcode);
        int rc = SPH_OK;
        for (int k = 0; k < ranks(); k++)
            if (b.op[k] != opcode) rc = fail(SPH_ERR_DEVICE, "%s: rank %d is in collective %d, rank %d in %d", Board::label, r, opcode, k, (int)b.op[k]);
        if (!rc) rc = con();
        if (!b.barrier() && !rc) rc = fail(SPH_ERR_DEVICE, "%s: a rank left collective %d early", Board::label, opcode);
        return rc;
    }
    // element-wise minimum over the ranks of `len` floats
    int min_f32(float* v, size_t len)
    {
        if (len > SHM_MAX_F32) return fail(SPH_ERR_INVALID_ARGUMENT, "%s: all-reduce of %zu floats", Board::label, len);
        b.f32len[r] = (uint32_t)len;
        return meet(1, [&] { memcpy(&b.f32rows[r][0], v, len * 4); },
                    [&] {
                        for (size_t k = 0; k < len; k++)
                            for (int q = 0; q < ranks(); q++) {
                                if (b.f32len[q] != len) return fail(SPH_ERR_DEVICE, "%s: all-reduce sizes differ", Board::label);
                                v[k] = fminf(v[k], b.f32rows[q][k]);
                            }
                        return (int)SPH_OK;
                    });
    }
    int max_i32(int* v)
    {
        return meet(2, [&] { b.i32vals[r] = *v; },
                    [&] {
                        for (int q = 0; q < ranks(); q++) *v = std::max(*v, (int)b.i32vals[q]);
                        return (int)SPH_OK;
                    });
    }
    // element-wise sum over the ranks of `len` words
    int sum_u32(uint32_t* v, size_t len)
    {
        if (len > SHM_MAX_U32) return fail(SPH_ERR_INVALID_ARGUMENT, "%s: all-reduce of %zu words", Board::label, len);
        b.u32len[r] = (uint32_t)len;
        return meet(3, [&] { memcpy(&b.u32rows[r][0], v, len * 4); },
                    [&] {
                        for (size_t k = 0; k < len; k++) {
                            v[k] = 0;
                            for (int q = 0; q < ranks(); q++) v[k] += b.u32rows[q][k];
                        }
                        return (int)SPH_OK;
                    });
    }
    // what the x-neighbours are about to send this rank; `status` (optional) becomes the maximum over all ranks
    int neighbour_counts(uint32_t to_left, uint32_t to_right, uint32_t* from_left, uint32_t* from_right, int* status)
    {
        const uint32_t w[8] = {to_left, to_right, status ? (uint32_t)*status : 0u, 0, 0, 0, 0, 0};
        return meet(4, [&] { memcpy(&b.words[r][0], w, sizeof w); },
                    [&] {
                        *from_left = r > 0 ? b.words[r - 1][1] : 0;
                        *from_right = r + 1 < ranks() ? b.words[r + 1][0] : 0;
                        if (status)
                            for (int q = 0; q < ranks(); q++) *status = std::max(*status, (int)b.words[q][2]);
                        return (int)SPH_OK;
                    });
    }
    // the fused refresh: this rank's counts and region figures (o.mig, o.halo, o.hreg) out, the neighbours' in (o.in_*); `status` and
    // `fallback` become their maxima over all ranks
    int refresh(RefreshCounts& o, int* status, int* fallback)
    {
        uint32_t w[8] = {o.mig[0], o.halo[0], o.mig[1], o.halo[1], (uint32_t)*status, (uint32_t)*fallback, 0, 0};
        memcpy(w + 6, o.hreg, 8);
        return meet(5, [&] { memcpy(&b.words[r][0], w, sizeof w); },
                    [&] {
                        o.in_mig[0] = r > 0 ? b.words[r - 1][2] : 0;
                        o.in_halo[0] = r > 0 ? b.words[r - 1][3] : 0;
                        o.in_mig[1] = r + 1 < ranks() ? b.words[r + 1][0] : 0;
                        o.in_halo[1] = r + 1 < ranks() ? b.words[r + 1][1] : 0;
                        o.in_hreg[0] = o.in_hreg[1] = 0.f;
                        if (r > 0) memcpy(&o.in_hreg[0], &b.words[r - 1][7], 4);        // the left rank's figure for ITS right cut = my left one
                        if (r + 1 < ranks()) memcpy(&o.in_hreg[1], &b.words[r + 1][6], 4);
                        for (int q = 0; q < ranks(); q++) {
                            *status = std::max(*status, (int)b.words[q][4]);
                            if (b.words[q][5]) *fallback = 1;
                        }
                        return (int)SPH_OK;
                    });
    }
    // sum over the ranks of six doubles, handed to done(const double*) while the ranks are still together
    template <class Done>
    int sum_f64x6(int opcode, const double* mine, Done done)
    {
        return meet(opcode, [&] { memcpy(&b.tot[r][0], mine, 48); },
                    [&] {
                        double t[6] = {0, 0, 0, 0, 0, 0};
                        for (int q = 0; q < ranks(); q++)
                            for (int k = 0; k < 6; k++) t[k] += b.tot[q][k];   // (rank order: the same sum on every rank)
                        return done((const double*)t);
                    });
    }
    // maximum over the ranks of the guard word, handed to done(uint32_t)
    template <class Done>
    int max_guard(uint32_t e, Done done)
    {
        return meet(9, [&] { b.i32vals[r] = (int)e; },
                    [&] {
                        uint32_t m = 0;
                        for (int q = 0; q < ranks(); q++) m = std::max(m, (uint32_t)b.i32vals[q]);
                        return done(m);
                    });
    }

    // ---- an exchange is point to point, like the grouped ncclSend / ncclRecv of the RCCL transport: one rendezvous per x-neighbour this
    // rank has something for or expects something from; RCCL pairs every send with a receive of the same size on the other side -- the
    // same rule, checked; a neighbour that does not come is what would hang RCCL.  Per side: pair_side, [the sender stages its payload],
    // pair_meet, [the receiver takes it], pair_leave.
    enum { SKIP = -1 };   // pair_side: nothing in either direction, the rank does not enter that pair
    int neighbour(int side) const { return side == 0 ? r - 1 : r + 1; }
    int lower(int side) const { return std::min(r, neighbour(side)); }   // the pair's channel
    int who(int side) const { return r < neighbour(side) ? 0 : 1; }      // this rank's half of it
    int pair_side(int side, const size_t* send_bytes, const size_t* recv_bytes)
    {
        const int nb = neighbour(side);
        if (nb < 0 || nb >= ranks()) {
            if (send_bytes[side] || recv_bytes[side]) return fail(SPH_ERR_DEVICE, "halo exchange across the outer edge of the slab row (rank %d)", r);
            return SKIP;
        }
        return send_bytes[side] || recv_bytes[side] ? (int)SPH_OK : (int)SKIP;
    }
    int pair_meet(int side, const size_t* send_bytes, const size_t* recv_bytes)
    {
        const int nb = neighbour(side), mine = who(side);
        auto& ch = b.pair[lower(side)];
        for (int sd = 0; sd < 2; sd++) {
            ch.send_bytes[mine][sd] = send_bytes[sd];
            ch.recv_bytes[mine][sd] = recv_bytes[sd];
        }
        if (!b.pair_barrier(lower(side)))
            return fail(SPH_ERR_DEVICE, "%s: rank %d did not enter the exchange rank %d has %zu bytes to send to / %zu bytes to receive from it for (it would hang over RCCL)",
                        Board::label, nb, r, send_bytes[side], recv_bytes[side]);
        const int oside = side ^ 1;   // my left neighbour's right side and vice versa
        const uint64_t o_send = ch.send_bytes[mine ^ 1][oside], o_recv = ch.recv_bytes[mine ^ 1][oside];
        if (recv_bytes[side] != o_send || send_bytes[side] != o_recv) {
            b.abandon();
            return fail(SPH_ERR_DEVICE, "halo exchange sizes of ranks %d and %d do not pair up (rank %d: send %zu recv %zu; rank %d: send %llu recv %llu)", r, nb, r,
                        send_bytes[side], recv_bytes[side], nb, (unsigned long long)o_send, (unsigned long long)o_recv);
        }
        return SPH_OK;
    }
    // (the sender may reuse its staging buffer / outbox once both are past this)
    int pair_leave(int side)
    {
        if (!b.pair_barrier(lower(side))) return fail(SPH_ERR_DEVICE, "%s: rank %d left the exchange with rank %d early", Board::label, neighbour(side), r);
        return SPH_OK;
    }
};
