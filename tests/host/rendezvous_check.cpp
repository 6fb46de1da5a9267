// The rendezvous protocol of the thread and the shared-memory transport (adaptive_sph_amd/csrc/sph_rendezvous.hpp) on the CPU: 4 ranks
// as 4 threads per board, every collective against the value computed serially, the exchange skeleton with a rank that stays out of
// a pair, and the three refusals.  Built and run by tests/test_rendezvous_host.py under ThreadSanitizer and AddressSanitizer / UBSan;
// exit status 0 = everything held.
#include "sph_rendezvous.hpp"

#include <pthread.h>
#include <sys/mman.h>

#include <thread>

#if defined(__SANITIZE_THREAD__)
// The ThreadSanitizer runtime of g++ 11 intercepts pthread_cond_wait and pthread_cond_timedwait but not pthread_cond_clockwait, which
// libstdc++ calls for waits on the steady clock: it then misses the unlock inside the wait and reports a "double lock" and a race on
// everything the mutex guards.  The same wait through the call it does intercept (this definition comes before the C library's):
extern "C" int pthread_cond_clockwait(pthread_cond_t* cv, pthread_mutex_t* mu, clockid_t clock, const struct timespec* until)
{
    struct timespec now, real;
    clock_gettime(clock, &now);
    clock_gettime(CLOCK_REALTIME, &real);
    real.tv_sec += until->tv_sec - now.tv_sec;
    real.tv_nsec += until->tv_nsec - now.tv_nsec;
    while (real.tv_nsec < 0) real.tv_nsec += 1000000000L, real.tv_sec--;
    while (real.tv_nsec >= 1000000000L) real.tv_nsec -= 1000000000L, real.tv_sec++;
    return pthread_cond_timedwait(cv, mu, &real);
}
#endif

static const int N = 4;
static std::atomic<int> g_failures{0};
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            g_failures++;                                   \
            fprintf(stderr, "%s:%d: CHECK(%s) ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
        }                                                   \
    } while (0)

// ---- a board of N ranks, fresh ----
template <class Board>
struct Fresh;
template <>
struct Fresh<ThreadGroup> {
    ThreadGroup g{N};
    ThreadGroup& board() { return g; }
};
template <>
struct Fresh<ShmSegment> {
    size_t bytes = ShmSegment::size_for(N, 4096);
    void* mem = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_ANONYMOUS | MAP_SHARED, -1, 0);
    ShmSegment* g = mem == MAP_FAILED ? nullptr : ShmSegment::create(mem, N, 4096);
    ShmSegment& board() { return *g; }
    ~Fresh() { if (g) munmap(mem, bytes); }
    Fresh() = default;
    Fresh(const Fresh&) = delete;
};

// f(R) on one thread per rank in `who`
template <class Board, class F>
static void on_ranks(Board& b, std::initializer_list<int> who, F f)
{
    std::vector<std::thread> t;
    for (int r : who)
        t.emplace_back([&b, r, f] {
            Rendezvous<Board> R(b, r);
            f(R);
        });
    for (auto& x : t) x.join();
}
static double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// ---- rank- and round-dependent inputs: every rank computes everybody's, so it knows the serial result ----
static void in_f32(int r, int it, float v[8])
{
    for (int k = 0; k < 8; k++) v[k] = (float)((r * 7 + k * 13 + it * 5) % 23) - 11.f + 0.25f * (float)r;
    v[2] = (r & 1) ? -0.0f : 1.0f;                       // a negative zero is the minimum
    v[3] = (it % 3 == 0 || r != it % N) ? INFINITY : 2.f;   // infinite on all ranks in every third round, else on all but one
}
static int in_i32(int r, int it) { return (r * 37 + it * 11) % 101 - 50; }
static uint32_t in_u32(int r, int it, size_t k) { return (uint32_t)k * 2654435761u + (uint32_t)r * 97u + (uint32_t)it; }
static uint32_t in_left(int r, int it) { return r == 0 ? 0u : (uint32_t)(r * 100 + it); }
static uint32_t in_right(int r, int it) { return r == N - 1 ? 0u : (uint32_t)(r * 1000 + it * 3); }
static int in_status(int r, int it) { return it % 5 == 0 && r == it % N ? (int)SPH_ERR_UNSUPPORTED : (it % 7 == 0 && r == 1 ? (int)SPH_ERR_CAPACITY : 0); }
static int in_fallback(int r, int it) { return it % 4 == 1 && r == (it / 4) % N; }
static RefreshCounts in_refresh(int r, int it)
{
    RefreshCounts o{};
    for (int s = 0; s < 2; s++) {
        o.mig[s] = (uint32_t)(r * 10 + s + it);
        o.halo[s] = (uint32_t)(r * 20 + s * 3 + it * 2);
        o.hreg[s] = 0.01f * (float)(r + 1) + 0.001f * (float)(s + it % 9);
    }
    return o;
}
static void in_f64(int r, int it, double v[6])
{
    const double big[N] = {1.0, 1e16, -1e16, 3.0};   // (the sum depends on the order: rank order is part of the contract)
    for (int k = 0; k < 6; k++) v[k] = big[(r + k) % N] + 0.1 * (double)(it % 10) + (double)k;
}
static uint32_t in_guard(int r, int it) { return it % 6 == 2 && r == it % N ? (uint32_t)SPH_ERR_AII_NEGATIVE : 0u; }

template <class Board>
static void one_round(Rendezvous<Board>& R, int it)
{
    const int r = R.r;
    switch (it % 7) {
    case 0: {
        float v[8], o[8], e[8];
        in_f32(r, it, v);
        memcpy(e, v, sizeof e);
        for (int k = 0; k < 8; k++)
            for (int q = 0; q < N; q++) {
                in_f32(q, it, o);
                e[k] = fminf(e[k], o[k]);
            }
        CHECK(R.min_f32(v, 8) == SPH_OK, "%s", R.err.c_str());
        CHECK(memcmp(v, e, sizeof e) == 0 && std::signbit(v[2]), "min of floats, rank %d round %d", r, it);
    } break;
    case 1: {
        int v = in_i32(r, it), e = v;
        for (int q = 0; q < N; q++) e = std::max(e, in_i32(q, it));
        CHECK(R.max_i32(&v) == SPH_OK, "%s", R.err.c_str());
        CHECK(v == e, "max of ints, rank %d round %d: %d, serially %d", r, it, v, e);
    } break;
    case 2: {
        std::vector<uint32_t> v(SHM_MAX_U32);
        for (size_t k = 0; k < v.size(); k++) v[k] = in_u32(r, it, k);
        CHECK(R.sum_u32(v.data(), v.size()) == SPH_OK, "%s", R.err.c_str());
        size_t bad = 0;
        for (size_t k = 0; k < v.size(); k++) {
            uint32_t e = 0;
            for (int q = 0; q < N; q++) e += in_u32(q, it, k);
            bad += v[k] != e;
        }
        CHECK(bad == 0, "sum of words, rank %d round %d: %zu differ", r, it, bad);
    } break;
    case 3: {
        uint32_t fl = 77, fr = 77;
        int st = in_status(r, it), e = 0;
        for (int q = 0; q < N; q++) e = std::max(e, in_status(q, it));
        const bool with_status = (it / 7) % 2 == 0;   // (the same choice on every rank)
        CHECK(R.neighbour_counts(in_left(r, it), in_right(r, it), &fl, &fr, with_status ? &st : nullptr) == SPH_OK, "%s", R.err.c_str());
        CHECK(fl == (r > 0 ? in_right(r - 1, it) : 0u) && fr == (r + 1 < N ? in_left(r + 1, it) : 0u), "neighbour counts, rank %d round %d", r, it);
        CHECK(st == (with_status ? e : in_status(r, it)), "status maximum, rank %d round %d", r, it);
    } break;
    case 4: {
        RefreshCounts o = in_refresh(r, it);
        int st = in_status(r, it), fb = in_fallback(r, it), est = 0, efb = 0;
        for (int q = 0; q < N; q++) {
            est = std::max(est, in_status(q, it));
            efb |= in_fallback(q, it);
        }
        CHECK(R.refresh(o, &st, &fb) == SPH_OK, "%s", R.err.c_str());
        RefreshCounts e = in_refresh(r, it);
        if (r > 0) {
            const RefreshCounts l = in_refresh(r - 1, it);
            e.in_mig[0] = l.mig[1], e.in_halo[0] = l.halo[1], e.in_hreg[0] = l.hreg[1];
        }
        if (r + 1 < N) {
            const RefreshCounts g = in_refresh(r + 1, it);
            e.in_mig[1] = g.mig[0], e.in_halo[1] = g.halo[0], e.in_hreg[1] = g.hreg[0];
        }
        CHECK(memcmp(&o, &e, sizeof e) == 0, "refresh words, rank %d round %d", r, it);
        CHECK(st == est && fb == efb, "refresh status / fallback, rank %d round %d", r, it);
    } break;
    case 5: {
        double v[6], o[6], e[6] = {0, 0, 0, 0, 0, 0}, got[6] = {0, 0, 0, 0, 0, 0};
        in_f64(r, it, v);
        for (int q = 0; q < N; q++) {
            in_f64(q, it, o);
            for (int k = 0; k < 6; k++) e[k] += o[k];
        }
        CHECK(R.sum_f64x6(7 + (it & 1), v, [&](const double* t) { memcpy(got, t, 48); return (int)SPH_OK; }) == SPH_OK, "%s", R.err.c_str());
        CHECK(memcmp(got, e, 48) == 0, "six doubles are not the rank-order sum bit for bit, rank %d round %d", r, it);
    } break;
    case 6: {
        uint32_t got = 99, e = 0;
        for (int q = 0; q < N; q++) e = std::max(e, in_guard(q, it));
        CHECK(R.max_guard(in_guard(r, it), [&](uint32_t m) { got = m; return (int)SPH_OK; }) == SPH_OK, "%s", R.err.c_str());
        CHECK(got == e, "guard maximum, rank %d round %d", r, it);
    } break;
    }
}

// ---- the exchange skeleton; the payload moves as in sph_transport.hip, with memcpy in the place of the device copies ----
static void stage(Rendezvous<ThreadGroup>& R, const uint8_t* const send[2], const size_t*, int side)
{
    for (int sd = 0; sd < 2; sd++) R.b.pair[(size_t)R.lower(side)].send[R.who(side)][sd] = send[sd];
}
static void take(Rendezvous<ThreadGroup>& R, uint8_t* dst, size_t bytes, int side) { memcpy(dst, R.b.pair[(size_t)R.lower(side)].send[R.who(side) ^ 1][side ^ 1], bytes); }
static void stage(Rendezvous<ShmSegment>& R, const uint8_t* const send[2], const size_t* send_bytes, int side) { memcpy(R.b.outbox(R.r, side), send[side], send_bytes[side]); }
static void take(Rendezvous<ShmSegment>& R, uint8_t* dst, size_t bytes, int side) { memcpy(dst, R.b.outbox(R.neighbour(side), side ^ 1), bytes); }

// rank 0 has nothing at all, rank 1 nothing for (or from) its left neighbour: neither enters pair (0, 1); between 1 and 2 bytes flow in
// one direction only
static const size_t X_SEND[N][2] = {{0, 0}, {0, 64}, {0, 16}, {48, 0}}, X_RECV[N][2] = {{0, 0}, {0, 0}, {64, 48}, {16, 0}};
static uint8_t payload(int from, int side, int it, size_t k) { return (uint8_t)(from * 50 + side * 7 + it + (int)k); }
template <class Board>
static void one_exchange(Rendezvous<Board>& R, int it)
{
    const int r = R.r;
    uint8_t out[2][64], in[2][64];
    for (int s = 0; s < 2; s++)
        for (size_t k = 0; k < 64; k++) out[s][k] = payload(r, s, it, k);
    memset(in, 0xee, sizeof in);
    const uint8_t* const send[2] = {out[0], out[1]};
    int entered = 0;
    for (int side = 0; side < 2; side++) {
        int rc = R.pair_side(side, X_SEND[r], X_RECV[r]);
        if (rc == Rendezvous<Board>::SKIP) continue;
        entered++;
        CHECK(rc == SPH_OK, "%s", R.err.c_str());
        stage(R, send, X_SEND[r], side);
        CHECK((rc = R.pair_meet(side, X_SEND[r], X_RECV[r])) == SPH_OK, "%s", R.err.c_str());
        if (rc) return;
        take(R, in[side], X_RECV[r][side], side);
        CHECK(R.pair_leave(side) == SPH_OK, "%s", R.err.c_str());
        size_t bad = 0;
        for (size_t k = 0; k < 64; k++) bad += in[side][k] != (k < X_RECV[r][side] ? payload(R.neighbour(side), side ^ 1, it, k) : 0xee);
        CHECK(bad == 0, "exchange payload, rank %d side %d round %d: %zu bytes differ", r, side, it, bad);
    }
    const int expect[N] = {0, 1, 2, 1};
    CHECK(entered == expect[r], "rank %d entered %d pairs", r, entered);
}

// ---- the refusals: each once, on a fresh board, with the limit at 200 ms; afterwards the board is broken ----
template <class Board>
static void expect_refusal(Rendezvous<Board>& R, int rc, const char* what, bool labelled)
{
    CHECK(rc == SPH_ERR_DEVICE, "rank %d: status %d", R.r, rc);
    CHECK(R.err.find(what) != std::string::npos, "rank %d: \"%s\" lacks \"%s\"", R.r, R.err.c_str(), what);
    if (labelled) CHECK(R.err.find(Board::label) != std::string::npos, "rank %d: \"%s\" lacks the board's label", R.r, R.err.c_str());
}
template <class Board>
static void later_meets_fail_at_once(Board& b, int rank)
{
    rdv_wait_limit = std::chrono::milliseconds(60000);   // a meet that waited would now wait a minute
    const auto t0 = std::chrono::steady_clock::now();
    Rendezvous<Board> R(b, rank);
    int v = 1;
    expect_refusal(R, R.max_i32(&v), "did not enter collective 2", true);
    CHECK(seconds_since(t0) < 2.0, "a meet on a broken board waited %.2f s", seconds_since(t0));
}
template <class Board>
static void refusals()
{
    for (int which = 0; which < 3; which++) {
        Fresh<Board> f;
        Board& b = f.board();
        rdv_wait_limit = std::chrono::milliseconds(200);
        const auto t0 = std::chrono::steady_clock::now();
        if (which == 0) {   // one rank enters collective 1 while the others enter 2
            on_ranks(b, {0, 1, 2, 3}, [](Rendezvous<Board>& R) {
                float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                int w = 3;
                expect_refusal(R, R.r == 0 ? R.min_f32(v, 8) : R.max_i32(&w), R.r == 0 ? "rank 0 is in collective 1, rank 3 in 2" : "in collective 2, rank 0 in 1", true);
                R.b.abandon();   // (what a rank does when its step failed: sph_step.hip, comm_abandon)
            });
        } else if (which == 1) {   // one rank does not come
            on_ranks(b, {1, 2, 3}, [](Rendezvous<Board>& R) {
                int w = 3;
                expect_refusal(R, R.max_i32(&w), "a rank did not enter collective 2 (it would hang over RCCL)", true);
            });
        } else {   // a pair posts sizes that do not pair up: whoever sees it says so and breaks the board; a rank still inside the pair's
                   // barrier at that moment reports the neighbour as absent
            std::atomic<int> named{0};
            on_ranks(b, {1, 2}, [&named](Rendezvous<Board>& R) {
                const size_t send[2] = {0, R.r == 1 ? 64u : 0u}, recv[2] = {R.r == 2 ? 32u : 0u, 0};
                const int side = R.r == 1 ? 1 : 0;
                CHECK(R.pair_side(side, send, recv) == SPH_OK, "%s", R.err.c_str());
                const int rc = R.pair_meet(side, send, recv);
                if (R.err.find("do not pair up") != std::string::npos) expect_refusal(R, rc, R.r == 1 ? "rank 1: send 64 recv 0; rank 2: send 0 recv 32" : "rank 2: send 0 recv 32; rank 1: send 64 recv 0", false), named++;
                else expect_refusal(R, rc, "did not enter the exchange", true);
            });
            CHECK(named.load() >= 1, "no rank named the sizes that do not pair up");
        }
        CHECK(seconds_since(t0) < 2.0, "refusal %d of the %s took %.2f s", which, Board::label, seconds_since(t0));
        later_meets_fail_at_once(b, 0);
    }
    rdv_wait_limit = std::chrono::milliseconds(60000);
}

template <class Board>
static void check_board()
{
    {
        Fresh<Board> f;
        on_ranks(f.board(), {0, 1, 2, 3}, [](Rendezvous<Board>& R) {
            for (int it = 0; it < 200; it++) one_round(R, it);
            for (int it = 0; it < 50; it++) one_exchange(R, it);
            // sizes the slots do not hold, and bytes across the outer edge, are refused before anybody waits
            std::vector<float> big(SHM_MAX_F32 + 1);
            CHECK(R.min_f32(big.data(), big.size()) == SPH_ERR_INVALID_ARGUMENT && R.err.find(Board::label) != std::string::npos, "%s", R.err.c_str());
            const size_t some[2] = {8, 8}, none[2] = {0, 0};
            if (R.r == 0) CHECK(R.pair_side(0, some, none) == SPH_ERR_DEVICE, "rank 0 sends to the left");
            if (R.r == N - 1) CHECK(R.pair_side(1, none, some) == SPH_ERR_DEVICE, "rank %d receives from the right", N - 1);
        });
    }
    refusals<Board>();
    fprintf(stderr, "%s: %d failure(s) so far\n", Board::label, g_failures.load());
}

int main()
{
    check_board<ThreadGroup>();
    check_board<ShmSegment>();
    return g_failures.load() ? 1 : 0;
}
