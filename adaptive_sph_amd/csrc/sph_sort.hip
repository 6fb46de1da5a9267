// Spatial-hash neighbour build for gfx950: cell index -> stable LSD radix sort of (cell, particle)
// pairs -> cell-range table (-> per-tile bound on the neighbours' h in multi-resolution scenes).
//
// What is computed follows the reference's own uniform-grid scheme
// (/root/reference/src/simulation/neighborhood_search.rs:243-321 and CellGrid :355-410):
//   cell      = floor(x / cell_size) per axis as i32                     (:253-255)
//   cells_min = floor(min / cell_size) - 1, cells_max = floor(max / cell_size) + 2   (:273-274)
//   linear    = (cx - minx) + (cy - miny) * size_x, x fastest            (:383-395)
// How it is computed is MI355X-native: 1024-key tiles, four waves per tile, each wave ranks its 256 keys
// with ballot-based match-any (no LDS atomics in the ranking), digit histograms are scanned row-wise, and the cell-range table is written by the
// threads that sit on a key boundary of the sorted sequence (no atomics, deterministic).
#include "sph_internal.hpp"

#define RS_ITEMS 32
#define RS_TILE (64 * RS_ITEMS)

// ------------------------------------------------------------------------------------------------
// radix sort
// ------------------------------------------------------------------------------------------------
// digit of a key and, within the wave, which lanes hold the same digit (match-any by ballots: no LDS atomics)
template <int NB>
__device__ __forceinline__ uint64_t rs_peers(uint32_t d, bool valid)
{
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// NB = digit width in bits (8, 9 or 10: the fewest passes that cover the key; 18-bit cell ids take two 9-bit passes).
// per-tile digit histogram: 256 threads, wave w owns keys [256 w, 256 w + 256) of the tile in 4 rounds of 64
// KEYGEN: the first pass of the cell sort makes its keys itself -- cell index of particle idx from its record, stored for the
// scatter together with val = idx -- instead of reading them from a launch of their own.  Slots [0, n_gone) whose class byte is
// >= gone_from left this rank's arrays (slab decomposition: last step's ghosts, particles handed to a neighbour): they get the key
// `ncells`, one past the last cell -- the sort moves them behind the live particles and nothing after it looks at them, i.e. the
// compaction of the arrays rides in the cell sort.
__device__ __forceinline__ uint32_t cell_key_of(const CellKeyGen& kg, uint32_t i)
{
    if (kg.gone && i < kg.n_gone && kg.gone[i] >= kg.gone_from) return kg.g.ncells;
    const float4 p = kg.pm[i];
    if (kg.clamp) return cell_key_clamped(kg.g, p.x, p.y);   // (launch-uniform)
    // IEEE division, like `(particle_pos / kernel_support_radius).map(|x| x.floor() as i32)`
    const int cx = (int)floorf(p.x / kg.g.cs) - kg.g.minx;
    const int cy = (int)floorf(p.y / kg.g.cs) - kg.g.miny;
    return (uint32_t)cx + (uint32_t)cy * (uint32_t)kg.g.sx;
}
template <int NB, bool KEYGEN>
__global__ __launch_bounds__(256) void k_rs_hist(uint32_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t n, int shift, uint32_t nblocks,
                                                  uint32_t* __restrict__ hist, CellKeyGen kg)
{
    constexpr int DIG = 1 << NB;
    __shared__ uint32_t h[DIG];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int d = tid; d < DIG; d += 256) h[d] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * RS_TILE + w * (RS_TILE / 4);
    const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < RS_ITEMS / 4; r++) {
        const uint32_t idx = base + r * 64 + lane;
        const bool valid = idx < n;
        uint32_t kv = 0u;
        if (valid) {
            if (KEYGEN) {
                kv = cell_key_of(kg, idx);
                key[idx] = kv;
                val[idx] = idx;
            } else kv = key[idx];
        }
        const uint32_t d = valid ? (kv >> shift) & (uint32_t)(DIG - 1) : 0u;
        const uint64_t peers = rs_peers<NB>(d, valid);
        if (valid && (peers & lt) == 0ull) atomicAdd(&h[d], (uint32_t)__popcll(peers));   // one add per distinct digit of the round
    }
    __syncthreads();
    for (int d = tid; d < DIG; d += 256) hist[(size_t)d * nblocks + blockIdx.x] = h[d];
}

// one workgroup per digit: exclusive scan of that digit's per-block counts, total -> totals[d]
// (four consecutive counts per thread: 1024 tiles -- 1M keys -- are one trip of loads and one block scan instead of four of each)
__global__ __launch_bounds__(256) void k_rs_rowscan(uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t* __restrict__ totals)
{
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t carry_s;
    uint32_t* row = hist + (size_t)blockIdx.x * nblocks;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t b = 0; b < nblocks; b += 1024) {
        const uint32_t i = b + 4u * (uint32_t)tid;
        uint32_t v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) v[u] = i + u < nblocks ? row[i + u] : 0u;
        const uint32_t own = v[0] + v[1] + v[2] + v[3];
        uint32_t x = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t woff = 0;
        for (int k = 0; k < w; k++) woff += wsum[k];
        const uint32_t carry = carry_s;
        uint32_t run = carry + woff + x - own;
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            if (i + u < nblocks) row[i + u] = run;
            run += v[u];
        }
        __syncthreads();
        if (tid == 255) carry_s = carry + woff + x;
        __syncthreads();
    }
    if (tid == 0) totals[blockIdx.x] = carry_s;
}

// stable scatter of one tile: wave w ranks its 256 keys in 4 rounds (match-any), the per-wave digit counts give each wave
// its offset behind the waves before it, the row-scanned histogram gives the tile its offset behind the tiles before it
template <int NB>
__global__ __launch_bounds__(256) void k_rs_scatter(const uint32_t* __restrict__ key_in, const uint32_t* __restrict__ val_in,
                                                     uint32_t* __restrict__ key_out, uint32_t* __restrict__ val_out, uint32_t n,
                                                     int shift, uint32_t nblocks, const uint32_t* __restrict__ hist,
                                                     const uint32_t* __restrict__ totals)
{
    constexpr int DIG = 1 << NB, PER = DIG / 256;   // digits per thread in the per-digit phases
    __shared__ uint32_t wcount[4][DIG];   // digit counts of each wave, then its running offsets
    __shared__ uint32_t gbase[DIG];       // global offset of the tile's first key of each digit
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int k = 0; k < 4; k++)
        for (int q = 0; q < PER; q++) wcount[k][tid * PER + q] = 0;
    // exclusive scan of the digit totals (PER consecutive digits per thread) + this tile's row-scanned offsets
    {
        uint32_t t[PER], sum = 0;
        for (int q = 0; q < PER; q++) {
            t[q] = totals[tid * PER + q];
            sum += t[q];
        }
        uint32_t x = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        uint32_t off = x - sum;
        for (int k = 0; k < w; k++) off += wsum[k];
        for (int q = 0; q < PER; q++) {
            gbase[tid * PER + q] = off + hist[(size_t)(tid * PER + q) * nblocks + blockIdx.x];
            off += t[q];
        }
    }
    const uint32_t base = blockIdx.x * RS_TILE + w * (RS_TILE / 4);
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t k_[RS_ITEMS / 4], v_[RS_ITEMS / 4], d_[RS_ITEMS / 4], rank_[RS_ITEMS / 4];
    bool ok_[RS_ITEMS / 4];
    __syncthreads();
    // phase 1: rank inside the wave (rounds in order => stable), count per digit
#pragma unroll
    for (int r = 0; r < RS_ITEMS / 4; r++) {
        const uint32_t idx = base + r * 64 + lane;
        ok_[r] = idx < n;
        k_[r] = ok_[r] ? key_in[idx] : 0u;
        v_[r] = ok_[r] ? val_in[idx] : 0u;
        d_[r] = (k_[r] >> shift) & (uint32_t)(DIG - 1);
        const uint64_t peers = rs_peers<NB>(d_[r], ok_[r]);
        const uint32_t before = wcount[w][d_[r]];          // keys of this digit in the wave's earlier rounds
        rank_[r] = before + (uint32_t)__popcll(peers & lt);
        // the wave's own LDS row: one writer per digit and round, ordered by the wave's program order
        __builtin_amdgcn_wave_barrier();
        if (ok_[r] && (peers & lt) == 0ull) wcount[w][d_[r]] = before + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // phase 2: offsets of the waves behind each other (each thread handles its PER digits)
    for (int q = 0; q < PER; q++) {
        const int d = tid * PER + q;
        uint32_t run = gbase[d];
        for (int k = 0; k < 4; k++) {
            const uint32_t c = wcount[k][d];
            wcount[k][d] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS / 4; r++) {
        if (ok_[r]) {
            const uint32_t dst = wcount[w][d_[r]] + rank_[r];
            key_out[dst] = k_[r];
            val_out[dst] = v_[r];
        }
    }
}

#define RS_MAX_DIGITS 1024

size_t radix_sort_scratch_elems(uint32_t n)
{
    size_t nblocks = ((size_t)n + RS_TILE - 1) / RS_TILE;
    return RS_MAX_DIGITS * (nblocks ? nblocks : 1) + RS_MAX_DIGITS;
}

template <int NB>
static void radix_pass(hipStream_t s, Profiler* prof, uint32_t* ki, uint32_t* vi, uint32_t* ko, uint32_t* vo, uint32_t n, int shift,
                       uint32_t nblocks, uint32_t* hist, uint32_t* totals, const CellKeyGen* kg)
{
    {
        ProfScope ps(prof, "sort_hist", s);
        if (kg) hipLaunchKernelGGL((k_rs_hist<NB, true>), dim3(nblocks), dim3(256), 0, s, ki, vi, n, shift, nblocks, hist, *kg);
        else hipLaunchKernelGGL((k_rs_hist<NB, false>), dim3(nblocks), dim3(256), 0, s, ki, vi, n, shift, nblocks, hist, CellKeyGen{});
    }
    {
        ProfScope ps(prof, "sort_rowscan", s);
        hipLaunchKernelGGL(k_rs_rowscan, dim3(1 << NB), dim3(256), 0, s, hist, nblocks, totals);
    }
    {
        ProfScope ps(prof, "sort_scatter", s);
        hipLaunchKernelGGL(k_rs_scatter<NB>, dim3(nblocks), dim3(256), 0, s, ki, vi, ko, vo, n, shift, nblocks, hist, totals);
    }
}

int radix_sort_pairs(hipStream_t s, Profiler* prof, uint32_t* keyA, uint32_t* valA, uint32_t* keyB, uint32_t* valB, uint32_t n,
                     int bits, uint32_t* scratch, const CellKeyGen* keygen)
{
    if (n == 0) return 0;
    uint32_t nblocks = (n + RS_TILE - 1) / RS_TILE;
    uint32_t* hist = scratch;
    uint32_t* totals = scratch + (size_t)RS_MAX_DIGITS * nblocks;
    if (bits < 1) bits = 1;
    // the fewest passes with digits of at most 10 bits, then the narrowest digit that still covers the key in that many
    const int passes = (bits + 9) / 10;
    int nb = (bits + passes - 1) / passes;
    if (nb < 8) nb = 8;
    int cur = 0;
    for (int p = 0; p < passes; p++) {
        uint32_t *ki = cur ? keyB : keyA, *vi = cur ? valB : valA, *ko = cur ? keyA : keyB, *vo = cur ? valA : valB;
        const CellKeyGen* kg = p == 0 ? keygen : nullptr;   // (keygen: keyA / valA are written by the first pass itself)
        if (nb == 8) radix_pass<8>(s, prof, ki, vi, ko, vo, n, p * nb, nblocks, hist, totals, kg);
        else if (nb == 9) radix_pass<9>(s, prof, ki, vi, ko, vo, n, p * nb, nblocks, hist, totals, kg);
        else radix_pass<10>(s, prof, ki, vi, ko, vo, n, p * nb, nblocks, hist, totals, kg);
        cur ^= 1;
    }
    return cur;
}

// ------------------------------------------------------------------------------------------------
// Incremental cell sort (round 4; VERDICT r3 "do not sort every step"): the array is ALREADY sorted by the cells its particles
// stood in at the start of the step, and a step moves few of them into another cell (configs[1]: 0.1-1 % per step,
// scripts/gpu_cell_movers.py).  The stable sort by the new cells is then a MERGE: the particles that stay (their keys are still
// ascending) with the few movers -- and every particle can compute its own slot:
//     slot(i) = first slot of its new cell                                    (scan over the cells' new populations)
//             + stayers of that cell in front of it                           (a look at the cell's old range: ~5 flags)
//             + movers INTO that cell with a smaller old index                (a per-cell list, empty for 96 % of the cells)
// which is exactly where the stable LSD sort puts it (ties by old index).  Classification (by the step's integrating tail, which holds
// the new positions, or a launch of its own), count, scan, place + reorder in one scatter pass -- three or four launches instead of the
// six of two radix passes, the gather reorder and the two of the cell-range table; same sorted keys, same order of the arrays and same
// cell_start bit for bit, whatever the number of movers -- the per-cell lists are built with atomics but only ever COUNTED, so no
// result depends on their order.  Cost grows with the movers (one 64-bit atomic exchange each, list walks in the cells they
// enter): the caller falls back to the radix sort when the previous step's count was large (sph_grid_plan.hpp: inc_sort_worthwhile).
// The grids of the two steps differ by a translation only (same cell size): lexicographic order of the cells is the same in both.
// Two callers: the build a plain context queues AHEAD behind its integrating tail (incremental_cell_sort_reorder), and a slab rank's
// sort at the start of its step, where last step's ghosts and migrants leave the array and the arrivals behind it are movers whatever
// their cell (incremental_cell_sort_perm: the rank builds the maps of its ghost layer from the permutation, so that form stores it).
// ------------------------------------------------------------------------------------------------
struct IncGrid {
    GridP cur, nxt;   // the grid the array is sorted by; the grid of the keys to sort by (same cs)
};
// range of next-grid cell c in the CURRENT order ([0, 0) if the current grid has no such cell)
__device__ __forceinline__ void inc_cur_range(const IncGrid& G, uint32_t c, const uint32_t* __restrict__ cell_start_cur, uint32_t& b, uint32_t& e)
{
    const uint32_t cy = c / (uint32_t)G.nxt.sx, cx = c - cy * (uint32_t)G.nxt.sx;
    const int ox = (int)cx + G.nxt.minx - G.cur.minx, oy = (int)cy + G.nxt.miny - G.cur.miny;
    b = e = 0u;
    if (ox >= 0 && ox < G.cur.sx && oy >= 0 && oy < G.cur.sy) {
        const uint32_t k = (uint32_t)ox + (uint32_t)oy * (uint32_t)G.cur.sx;
        b = cell_start_cur[k];
        e = cell_start_cur[k + 1];
    }
}

// stayers (flag 0) among the flag bytes mv[b, e) of a cell's old range: BATCH bytes requested together, so a cell of up to BATCH
// particles costs one load round trip where a loop over single bytes costs one per particle (the addresses are clamped into the
// range, the bytes behind its end do not count).  `serial` (launch-uniform; laboratory build only, Options::boundary_chains = 0): the
// loop over single bytes.
template <uint32_t BATCH>
__device__ __forceinline__ uint32_t inc_count_stayers(const uint8_t* __restrict__ mv, uint32_t b, uint32_t e, bool serial)
{
    uint32_t r = 0;
#ifdef SPH_LAB
    if (serial) {
        for (uint32_t j = b; j < e; j++) r += mv[j] ? 0u : 1u;
        return r;
    }
#endif
    for (uint32_t j = b; j < e; j += BATCH) {
        uint32_t f[BATCH];
#pragma unroll
        for (uint32_t u = 0; u < BATCH; u++) f[u] = mv[min(j + u, e - 1u)];
#pragma unroll
        for (uint32_t u = 0; u < BATCH; u++) r += (j + u < e && f[u] == 0u) ? 1u : 0u;
    }
    return r;
}

// 1. new key and mover flag of every particle; a mover hangs itself into the list of the cell it enters (head[c]: epoch-tagged, so
//    the table is never cleared -- an entry of another step reads as "empty").  inc_classify_particle, sph_device.h; the integrating
//    tail of the step's last solve does the same for the positions it has just computed, and this launch is then not needed.
__global__ __launch_bounds__(256) void k_inc_classify(uint32_t n, const float4* __restrict__ pm, IncClassifyP q)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pm[i];
    inc_classify_particle(q, i, p.x, p.y);
}

// ... of a slab rank (sph_slabs.hip: fused refresh): the array is last step's sorted slots [0, n_prev) -- of which the ones that left
// this rank (last step's ghosts, particles handed to a neighbour: class byte >= gone_from) take no part: flag 2 -- followed by this
// step's arrivals [n_prev, n) in the order they were unpacked: movers all, whatever their cell
__global__ __launch_bounds__(256) void k_inc_classify_slab(uint32_t n, uint32_t n_prev, CellKeyGen kg, IncClassifyP q)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (kg.gone && i < kg.n_gone && kg.gone[i] >= kg.gone_from) {
        q.mv[i] = 2;
        return;
    }
    const uint32_t k = cell_key_of(kg, i);
    inc_register(q, i, k, i >= n_prev || k != inc_key_of_cur_cell(q.cur, q.nxt, q.cxy_cur[i]));
}

// 2. new population of every cell = its stayers + the length of its list; per-block sums (INC_CELLS cells per block, one per thread:
//    the chain range -> flags -> list is three dependent round trips, so the launch wants many short threads)
//    FUSED (the build queued ahead behind the integrating tail: incremental_cell_sort_reorder with IncFusedP):
//    - `count` receives the populations' exclusive prefix WITHIN the block (the two-level form of the table: sph_boundary_fused.hpp);
//      the block sums and the mover counter are as in the other form, and nothing crosses from one workgroup to another inside the
//      launch: the prefix of the block sums is taken behind the launch boundary, by the workgroups of k_inc_place_reorder that need it;
//    - one more workgroup, the grid's last, reduces the header partials the tail in front left: k_header_ahead without its launch
//      (header_ahead_block, sph_internal.hpp: it depends on that tail alone, and publishes where the caller waits behind it).
template <bool FUSED>
__global__ __launch_bounds__(INC_CELLS) void k_inc_count(IncGrid G, const uint32_t* __restrict__ cell_start_cur, const uint8_t* __restrict__ mv,
                                                          const uint32_t* __restrict__ next, const unsigned long long* __restrict__ head, uint32_t epoch,
                                                          uint32_t* __restrict__ count /* cell_start of the next grid, used as scratch (FUSED: the local prefixes) */,
                                                          uint32_t* __restrict__ bsum, uint32_t* __restrict__ movers, HeaderAheadP hdr)
{
    __shared__ uint32_t ws[INC_CELLS / 64], wm[INC_CELLS / 64];
    if (FUSED && blockIdx.x + 1u == gridDim.x) {
        header_ahead_block(hdr);
        return;
    }
    const uint32_t c = blockIdx.x * (uint32_t)INC_CELLS + threadIdx.x;
    uint32_t cnt = 0, listed = 0;
    if (c < G.nxt.ncells) {
        uint32_t b, e;
        inc_cur_range(G, c, cell_start_cur, b, e);
        const unsigned long long h = head[c];
        for (uint32_t j = b; j < e; j++) cnt += mv[j] ? 0u : 1u;
        if ((uint32_t)(h >> 32) == epoch)
            for (uint32_t m = (uint32_t)h; m; m = next[m - 1u]) listed++;
        cnt += listed;
        if (!FUSED) count[c] = cnt;
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t x = cnt, y = listed;
    if (FUSED) {   // x: inclusive prefix within the wave, lane 63 holds the wave's sum
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(x, o, 64);
            if (lane >= (uint32_t)o) x += u;
        }
        for (int o = 32; o > 0; o >>= 1) y += (uint32_t)__shfl_xor((int)y, o, 64);
    } else {
        for (int o = 32; o > 0; o >>= 1) {
            x += (uint32_t)__shfl_xor((int)x, o, 64);
            y += (uint32_t)__shfl_xor((int)y, o, 64);
        }
    }
    if (lane == 63u) {
        ws[w] = x;
        wm[w] = y;
    }
    __syncthreads();
    if (FUSED && c < G.nxt.ncells) {
        uint32_t base = 0;
        for (uint32_t k = 0; k < w; k++) base += ws[k];
        count[c] = base + x - cnt;
    }
    if (threadIdx.x == 0) {
        uint32_t t = 0, m = 0;
        for (int k = 0; k < INC_CELLS / 64; k++) {
            t += ws[k];
            m += wm[k];
        }
        bsum[blockIdx.x] = t;
        if (m) atomicAdd(movers, m);   // (what the caller's next decision is taken on: a few hundred adds at most)
    }
}

// 3. exclusive scan of the populations: cell_start of the next grid (in place); block 0 hands the mover count to the host
__global__ __launch_bounds__(256) void k_inc_scan(uint32_t ncells, uint32_t* __restrict__ cell_start, const uint32_t* __restrict__ bsum, uint32_t* __restrict__ movers,
                                                   uint32_t* __restrict__ movers_host)
{
    __shared__ uint32_t ws[4], base_s;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t pre = 0;
    for (uint32_t k = tid; k < blockIdx.x; k += 256) pre += bsum[k];
    for (int o = 32; o > 0; o >>= 1) pre += (uint32_t)__shfl_xor((int)pre, o, 64);
    if (lane == 0) ws[w] = pre;
    __syncthreads();
    if (tid == 0) base_s = ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    const uint32_t c0 = blockIdx.x * (uint32_t)INC_CELLS + 4u * (uint32_t)tid;
    uint32_t v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; u++) v[u] = c0 + u < ncells ? cell_start[c0 + u] : 0u;
    const uint32_t own = v[0] + v[1] + v[2] + v[3];
    uint32_t x = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) ws[w] = x;
    __syncthreads();
    uint32_t run = base_s + x - own;
    for (int k = 0; k < w; k++) run += ws[k];
#pragma unroll
    for (uint32_t u = 0; u < 4u; u++) {
        if (c0 + u < ncells) cell_start[c0 + u] = run;
        run += v[u];
        if (c0 + u + 1u == ncells) cell_start[ncells] = run;
    }
    if (blockIdx.x == 0 && tid == 0) {
        *movers_host = *movers;
        *movers = 0u;
    }
}

// 4. every particle to its slot, with everything k_reorder moves (the merge knows where a particle GOES, so the reorder is a scatter of
//    coalesced reads -- a near-identity one -- and the permutation is never stored); the sorted keys as the radix sort leaves them
//    PERM (a slab rank: the maps of its ghost layer are built from the permutation): slot -> current index instead of the reorder;
//    slots that left the rank (flag 2) are not placed
//    FUSED (behind k_inc_count<true>): cell_start_nxt is the table in its two-level form, first slot = local prefix + prefix of the
//    block sums in front of the cell's count block (inc_cell_first).  Every workgroup takes that second level for itself, behind the
//    launch boundary: every wave of the particles' workgroups scans the block sums in its registers, 256 at a time (a few hundred at
//    2^20 particles: one 16-byte load per lane, no barrier), and the workgroups in front of them, one per count block, add up the sums in
//    front of theirs as k_inc_scan does and write the finished table, [ncells] = the total, to cell_start_fin for the next step's
//    BUILD (a buffer of its own: readers of the local form and finishers never touch the same words); the first of them hands the
//    mover count to the host.  A lane past the last particle goes along with its wave's scan and stores nothing.
template <bool PERM, bool FUSED>
__global__ __launch_bounds__(256) void k_inc_place_reorder(uint32_t n, IncGrid G, const uint32_t* __restrict__ cell_start_cur, const uint32_t* __restrict__ cell_start_nxt,
                                                            const uint32_t* __restrict__ nk, const uint8_t* __restrict__ mv, const uint32_t* __restrict__ next,
                                                            const unsigned long long* __restrict__ head, uint32_t epoch, const uint32_t* __restrict__ cxy_cur,
                                                            uint32_t* __restrict__ key_out, ReorderIO io, uint32_t* __restrict__ perm_out,
                                                            const uint32_t* __restrict__ bsum, uint32_t* __restrict__ cell_start_fin, uint32_t* __restrict__ movers,
                                                            uint32_t* __restrict__ movers_host, bool serial_flags)
{
    __shared__ uint32_t s_w[4];
    const uint32_t fin_blocks = FUSED ? inc_count_blocks(G.nxt.ncells) : 0u;   // (in FRONT of the particles': they run beside the first of them, not behind the last)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    if (FUSED && blockIdx.x < fin_blocks) {
        const uint32_t ncells = G.nxt.ncells, blk = blockIdx.x, c0 = blk * (uint32_t)INC_CELLS + 4u * tid;
        uint32_t pre = 0;
        for (uint32_t k = tid; k < blk; k += 256u) pre += bsum[k];
        for (int o = 32; o > 0; o >>= 1) pre += (uint32_t)__shfl_xor((int)pre, o, 64);
        if (lane == 0) s_w[w] = pre;
        __syncthreads();
        pre = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (c0 + 3u < ncells) {
            const uint4 l = *(const uint4*)(cell_start_nxt + c0);
            *(uint4*)(cell_start_fin + c0) = make_uint4(l.x + pre, l.y + pre, l.z + pre, l.w + pre);
        } else
            for (uint32_t c = c0; c < ncells; c++) cell_start_fin[c] = cell_start_nxt[c] + pre;
        if (tid == 0) {
            if (blk + 1u == fin_blocks) cell_start_fin[ncells] = pre + bsum[blk];
            if (blk == 0) {   // (as k_inc_scan's block 0)
                *movers_host = *movers;
                *movers = 0u;
            }
        }
        return;
    }
    const uint32_t i_raw = (blockIdx.x - fin_blocks) * 256 + tid;
    if (!FUSED && i_raw >= n) return;
    const bool past = FUSED && i_raw >= n;
    const uint32_t i = past ? n - 1u : i_raw;
    // (everything that does not depend on the slot is requested first, and nothing waits for the flag byte in front of it: the cell
    //  word is in bounds for every i < n -- an arrival has no current cell and does not use what it reads)
    const uint32_t flag = mv[i];
    const uint32_t c = nk[i];
    const uint32_t own = cxy_cur[i];
    float4 pm;
    float2 vel;
    uint32_t orig = 0;
    float lvl = 0.f, lvlold = 0.f, h2n = 0.f, lam = 0.f;
    uint8_t szc = 0;
    if (!PERM) {
        pm = io.pm_in[i];
        vel = io.vel_in[i];
        orig = io.orig_in[i];
        if (io.lvl_in) {   // (launch-uniform; nullptr: both level fields hold the upload's constants in every slot of both halves)
            lvl = io.lvl_in[i];
            lvlold = io.lvlold_in[i];
        }
        if (io.h2n_in) h2n = io.h2n_in[i];   // (launch-uniform, like the next two)
        if (io.lam_in) lam = io.lam_in[i];
        if (io.szc_in) szc = io.szc_in[i];
    }
    if (PERM && flag == 2u) return;
    const bool mover = flag != 0u;
    // the stayers of the wave: a stayer reads its rank among those of its cell off this word (sph_boundary_fused.hpp).  A lane that has
    // left -- past the end, a slot that left the rank -- or goes along past the last particle is no stayer.
    const uint64_t stay = __ballot(!mover && !past);
    const unsigned long long h = head[c];
    uint32_t first = cell_start_nxt[c];
    // the flag bytes in front of the particle in its new cell: [b, e) to be counted by loads, r_in already counted from the ballot
    uint32_t b = 0, e = 0, r_in = 0;
    if (!mover && !past) {   // the particle's own cell: no division
        const uint32_t k = (own & 0xffffu) + (own >> 16) * (uint32_t)G.cur.sx;
        b = cell_start_cur[k];
        const uint32_t w0 = i - lane;
        e = inc_rank_outside_end(w0, b);   // (only a cell that starts in front of the wave leaves bytes for the loop)
        r_in = (uint32_t)__popcll(stay & inc_rank_ballot_lanes(w0, b, i));
#ifdef SPH_LAB
        if (serial_flags) {
            e = i;
            r_in = 0;
        }
#endif
    } else if (mover) {   // stayers of the cell it enters: all of them if it comes from behind the cell's old range, none if from before it
        uint32_t eb;
        inc_cur_range(G, c, cell_start_cur, b, eb);
        e = inc_mover_range_end(i, b, eb);
    }
    if (FUSED) {   // + the block sums in front of the cell's count block: every WAVE for itself, no barrier -- lane l takes the sums 4l .. 4l + 3 of a chunk of 256
        const uint32_t cb = c >> INC_CELLS_LOG2;
        uint32_t carry = 0, mine = 0;
        for (uint32_t k0 = 0; k0 < fin_blocks; k0 += 256u) {   // (wave-uniform)
            const uint32_t k = k0 + 4u * lane;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (k + 3u < fin_blocks) v = *(const uint4*)(bsum + k);
            else {
                if (k < fin_blocks) v.x = bsum[k];
                if (k + 1u < fin_blocks) v.y = bsum[k + 1u];
                if (k + 2u < fin_blocks) v.z = bsum[k + 2u];
            }
            const uint32_t own4 = v.x + v.y + v.z + v.w;
            uint32_t z = own4;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = __shfl_up(z, o, 64);
                if (lane >= (uint32_t)o) z += u;
            }
            const uint32_t excl = carry + z - own4;   // the sums in front of this lane's four
            const uint32_t e = cb - k0, src = (e >> 2) & 63u, sub = e & 3u;   // the entry this lane's cell wants, if it lies in the chunk
            const uint32_t ex = __shfl(excl, (int)src, 64), x0 = __shfl(v.x, (int)src, 64), x1 = __shfl(v.y, (int)src, 64), x2 = __shfl(v.z, (int)src, 64);
            if (e < 256u) mine = ex + (sub > 0u ? x0 : 0u) + (sub > 1u ? x1 : 0u) + (sub > 2u ? x2 : 0u);
            carry += __shfl(z, 63, 64);
        }
        first += mine;
    }
    uint32_t r = r_in + inc_count_stayers<4u>(mv, b, e, serial_flags);
    if ((uint32_t)(h >> 32) == epoch)
        for (uint32_t m = (uint32_t)h; m; m = next[m - 1u]) r += (m - 1u < i) ? 1u : 0u;
    const uint32_t dst = first + r;
    if (past) return;
    key_out[dst] = c;
    if (PERM) {
        perm_out[dst] = i;
        return;
    }
    io.pm_out[dst] = pm;
    io.vel_out[dst] = vel;
    io.orig_out[dst] = orig;
    if (io.xv_out) io.xv_out[dst] = make_float4(pm.x, pm.y, vel.x, vel.y);   // (launch-uniform: the record of the next step's OpFuseU)
    if (io.lvl_in) {
        io.lvl_out[dst] = lvl;
        io.lvlold_out[dst] = lvlold;
    }
    if (io.h2n_in) io.h2n_out[dst] = h2n;
    if (io.lam_in) io.lam_prev_out[dst] = lam;
    if (io.szc_in) io.szc_out[dst] = szc;
    const uint32_t cy = c / (uint32_t)G.nxt.sx;
    io.cxy_out[dst] = (c - cy * (uint32_t)G.nxt.sx) | (cy << 16);
}

size_t incremental_sort_block_sums(uint32_t ncells) { return inc_count_blocks(ncells); }

void incremental_cell_sort_reorder(hipStream_t s, Profiler* prof, uint32_t n, const float4* pm_new, const IncClassifyP& q, bool classified,
                                   const uint32_t* cell_start_cur, uint32_t* key_out, uint32_t* cell_start_out, const ReorderIO& io, uint32_t* bsum, uint32_t* movers,
                                   uint32_t* movers_host, const IncFusedP* fused, bool serial_flags)
{
    const IncGrid G{q.cur, q.nxt};
    const uint32_t ncells = q.nxt.ncells, cblocks = (uint32_t)incremental_sort_block_sums(ncells);
    if (fused && classified) {   // two launches; the header of the tail in front rides in the first
        {
            ProfScope ps(prof, "inc_count", s);
            hipLaunchKernelGGL(k_inc_count<true>, dim3(cblocks + 1u), dim3(INC_CELLS), 0, s, G, cell_start_cur, q.mv, q.next, q.head, q.epoch, fused->local, bsum, movers,
                               fused->hdr);
        }
        {
            ProfScope ps(prof, "inc_reorder", s);
            hipLaunchKernelGGL((k_inc_place_reorder<false, true>), dim3((n + 255) / 256 + cblocks), dim3(256), 0, s, n, G, cell_start_cur, (const uint32_t*)fused->local,
                               q.nk, q.mv, q.next, q.head, q.epoch, q.cxy_cur, key_out, io, (uint32_t*)nullptr, (const uint32_t*)bsum, cell_start_out, movers, movers_host, serial_flags);
        }
        return;
    }
    if (!classified) {
        ProfScope ps(prof, "inc_classify", s);
        hipLaunchKernelGGL(k_inc_classify, dim3((n + 255) / 256), dim3(256), 0, s, n, pm_new, q);
    }
    {
        ProfScope ps(prof, "inc_count", s);
        hipLaunchKernelGGL(k_inc_count<false>, dim3(cblocks), dim3(INC_CELLS), 0, s, G, cell_start_cur, q.mv, q.next, q.head, q.epoch, cell_start_out, bsum, movers,
                           HeaderAheadP{});
    }
    {
        ProfScope ps(prof, "inc_scan", s);
        hipLaunchKernelGGL(k_inc_scan, dim3(cblocks), dim3(256), 0, s, ncells, cell_start_out, bsum, movers, movers_host);
    }
    {
        ProfScope ps(prof, "inc_reorder", s);
        hipLaunchKernelGGL((k_inc_place_reorder<false, false>), dim3((n + 255) / 256), dim3(256), 0, s, n, G, cell_start_cur, cell_start_out, q.nk, q.mv, q.next, q.head,
                           q.epoch, q.cxy_cur, key_out, io, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, serial_flags);
    }
}

void incremental_cell_sort_perm(hipStream_t s, Profiler* prof, uint32_t n, uint32_t n_prev, const CellKeyGen& kg, const IncClassifyP& q, const uint32_t* cell_start_cur,
                                uint32_t* key_out, uint32_t* perm_out, uint32_t* cell_start_out, uint32_t* bsum, uint32_t* movers, uint32_t* movers_host, bool serial_flags)
{
    const IncGrid G{q.cur, q.nxt};
    const uint32_t ncells = q.nxt.ncells, cblocks = (uint32_t)incremental_sort_block_sums(ncells);
    {
        ProfScope ps(prof, "inc_classify", s);
        hipLaunchKernelGGL(k_inc_classify_slab, dim3((n + 255) / 256), dim3(256), 0, s, n, n_prev, kg, q);
    }
    {
        ProfScope ps(prof, "inc_count", s);
        hipLaunchKernelGGL(k_inc_count<false>, dim3(cblocks), dim3(INC_CELLS), 0, s, G, cell_start_cur, q.mv, q.next, q.head, q.epoch, cell_start_out, bsum, movers,
                           HeaderAheadP{});
    }
    {
        ProfScope ps(prof, "inc_scan", s);
        hipLaunchKernelGGL(k_inc_scan, dim3(cblocks), dim3(256), 0, s, ncells, cell_start_out, bsum, movers, movers_host);
    }
    {
        ProfScope ps(prof, "inc_place", s);
        hipLaunchKernelGGL((k_inc_place_reorder<true, false>), dim3((n + 255) / 256), dim3(256), 0, s, n, G, cell_start_cur, cell_start_out, q.nk, q.mv, q.next, q.head,
                           q.epoch, q.cxy_cur, key_out, ReorderIO{}, perm_out, (const uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, serial_flags);
    }
}

// ------------------------------------------------------------------------------------------------
// cell keys / reorder / cell-range table / tiles
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_reorder(uint32_t n, GridP g, const uint32_t* __restrict__ sorted_key,
                                                  const uint32_t* __restrict__ perm, const float4* __restrict__ pm_in,
                                                  const float2* __restrict__ vel_in, const uint32_t* __restrict__ orig_in,
                                                  const float* __restrict__ lvl_in, const float* __restrict__ lvlold_in,
                                                  float4* __restrict__ pm_out, float2* __restrict__ vel_out,
                                                  uint32_t* __restrict__ orig_out, float* __restrict__ lvl_out,
                                                  float* __restrict__ lvlold_out, uint32_t* __restrict__ cxy,
                                                  const float* __restrict__ h2n_in, float* __restrict__ h2n_out,
                                                  const float* __restrict__ lam_in, float* __restrict__ lam_prev_out,
                                                  uint32_t* __restrict__ zero_word, const uint8_t* __restrict__ szc_in,
                                                  uint8_t* __restrict__ szc_out)
{
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && zero_word) *zero_word = 0u;   // work-list counter of the cell-range kernels that follow
    if (i >= n) return;
    uint32_t src = perm[i];
    if (h2n_in) h2n_out[i] = h2n_in[src];
    if (lam_in) lam_prev_out[i] = lam_in[src];
    if (szc_in) szc_out[i] = szc_in[src];
    pm_out[i] = pm_in[src];
    vel_out[i] = vel_in[src];
    orig_out[i] = orig_in[src];
    if (lvl_in) {   // (launch-uniform: see ReorderIO)
        lvl_out[i] = lvl_in[src];
        lvlold_out[i] = lvlold_in[src];
    }
    uint32_t k = sorted_key[i];
    uint32_t cy = k / (uint32_t)g.sx;
    uint32_t cx = k - cy * (uint32_t)g.sx;
    cxy[i] = cx | (cy << 16);
}

void launch_reorder(hipStream_t s, Profiler* prof, uint32_t n, GridP g, const uint32_t* sorted_key, const uint32_t* perm, const ReorderIO& io,
                    void* cell_start_scratch)
{
    ProfScope ps(prof, "reorder", s);
    hipLaunchKernelGGL(k_reorder, dim3((n + 255) / 256), dim3(256), 0, s, n, g, sorted_key, perm, io.pm_in, io.vel_in, io.orig_in, io.lvl_in,
                       io.lvlold_in, io.pm_out, io.vel_out, io.orig_out, io.lvl_out, io.lvlold_out, io.cxy_out, io.h2n_in, io.h2n_out, io.lam_in,
                       io.lam_prev_out, (uint32_t*)cell_start_scratch, io.szc_in, io.szc_out);
}

// cell_start[c] = index of the first sorted particle whose cell is >= c; cell_start[ncells] = n.
// Thread i (0..n) owns the boundary between sorted particles i-1 and i and fills the cells in
// (key[i-1], key[i]].  Short gaps (the normal case: adjacent occupied cells, row ends) are filled by the
// owning thread; long gaps (empty regions of a sparse grid, e.g. after a particle escaped the box) go to
// a work list that k_cell_fill spreads over whole workgroups -- no thread ever loops over more than
// CS_INLINE cells.
#define CS_INLINE 64u
#define CS_WORK_CAP 65536u

struct CellGap {
    uint32_t lo, hi, val;
};

__global__ __launch_bounds__(256) void k_cell_start(const uint32_t* __restrict__ key, uint32_t n, uint32_t ncells,
                                                     uint32_t* __restrict__ cell_start, CellGap* __restrict__ work,
                                                     uint32_t* __restrict__ work_count)
{
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    uint32_t lo, hi;  // fill cells lo..hi inclusive with i
    if (i == 0) {
        lo = 0;
        hi = n ? key[0] : ncells;
    } else if (i == n) {
        lo = key[n - 1] + 1;
        hi = ncells;
    } else {
        uint32_t a = key[i - 1], b = key[i];
        if (a == b) return;
        lo = a + 1;
        hi = b;
    }
    if (hi - lo >= CS_INLINE) {
        uint32_t slot = atomicAdd(work_count, 1u);
        if (slot < CS_WORK_CAP) {
            work[slot] = CellGap{lo, hi, i};
            return;
        }
    }
    for (uint32_t c = lo; c <= hi; c++) cell_start[c] = i;
}

__global__ __launch_bounds__(256) void k_cell_fill(const CellGap* __restrict__ work, const uint32_t* __restrict__ work_count,
                                                    uint32_t* __restrict__ cell_start)
{
    const uint32_t cnt = min(*work_count, CS_WORK_CAP);
    for (uint32_t e = blockIdx.x; e < cnt; e += gridDim.x) {
        const CellGap g = work[e];
        for (uint32_t c = g.lo + threadIdx.x; c <= g.hi; c += 256) cell_start[c] = g.val;
    }
}

size_t cell_start_scratch_bytes() { return (size_t)CS_WORK_CAP * sizeof(CellGap) + 16; }

void launch_cell_start(hipStream_t s, Profiler* prof, const uint32_t* sorted_key, uint32_t n, uint32_t ncells, uint32_t* cell_start,
                       void* scratch, bool count_zeroed)
{
    ProfScope ps(prof, "cell_start", s);
    uint32_t* count = (uint32_t*)scratch;
    CellGap* work = (CellGap*)((char*)scratch + 16);
    if (!count_zeroed) (void)hipMemsetAsync(count, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(k_cell_start, dim3((n + 1 + 255) / 256), dim3(256), 0, s, sorted_key, n, ncells, cell_start, work, count);
    hipLaunchKernelGGL(k_cell_fill, dim3(512), dim3(256), 0, s, work, count, cell_start);
}

// per-tile largest smoothing length (TileP, sph_device.h): atomicMax over the particles of the tile, then the
// maximum over the (2D+1) x (2D+1) tiles around each tile.  A neighbour within range (h_i + h_j)/2 * k <= h_max * k sits at
// most ceil(k * h_max / tile side) <= ceil(k / 2) tiles away (tile side >= 2 h_max): D = 1 for the SPH support (k = 2),
// D = 2 for the extended lists of the level estimation (k = 5.5 / 1.9) -- `out_ext`, nullptr when not wanted
__global__ __launch_bounds__(256) void k_tile_hmax(uint32_t n, const float4* __restrict__ pm, GridP g, int ts, int tsx, uint32_t* __restrict__ raw)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t tile = 0xffffffffu, hb = 0u;
    if (i < n) {
        const float4 p = pm[i];
        // clamped into the grid like the cell keys (cell_key_clamped): the grid of a build queued AHEAD is a prediction, and a particle an
        // exploding solve threw out of it indexed a tile beyond the table -- a memory fault BEHIND the step that had already returned its
        // error (round 5, configs[4]'s blocks too close to the floor: scripts/gpu_fault_bisect.sh); such a build is never adopted
        int cx = (int)floorf(p.x / g.cs) - g.minx, cy = (int)floorf(p.y / g.cs) - g.miny;
        cx = min(max(cx, 0), g.sx - 1);
        cy = min(max(cy, 0), g.sy - 1);
        tile = (uint32_t)(cy / ts) * (uint32_t)tsx + (uint32_t)(cx / ts);
        hb = __float_as_uint(p.w);
    }
    // the array is cell-sorted, so a wave usually sits in one or two tiles: one atomic per run of equal tiles (the
    // lane that starts the run carries the maximum of the run) instead of 64 atomics on the same address
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t ot = (uint32_t)__shfl_down((int)tile, o, 64), oh = (uint32_t)__shfl_down((int)hb, o, 64);
        if (lane + o < 64 && ot == tile) hb = max(hb, oh);   // suffix maximum within the run (runs are contiguous)
    }
    const uint32_t prev = (uint32_t)__shfl_up((int)tile, 1, 64);
    if (i < n && (lane == 0 || prev != tile)) atomicMax(&raw[tile], hb);
}
__global__ __launch_bounds__(256) void k_tile_dilate(int tsx, int tsy, int D, const uint32_t* __restrict__ raw, uint32_t* __restrict__ out)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint32_t)tsx * (uint32_t)tsy) return;
    const int tx = (int)(t % (uint32_t)tsx), ty = (int)(t / (uint32_t)tsx);
    uint32_t m = 0;
    for (int dy = -D; dy <= D; dy++)
        for (int dx = -D; dx <= D; dx++) {
            const int x = tx + dx, y = ty + dy;
            if (x >= 0 && x < tsx && y >= 0 && y < tsy) m = max(m, raw[(uint32_t)y * (uint32_t)tsx + (uint32_t)x]);
        }
    out[t] = m;
}

void launch_tile_hmax(hipStream_t s, Profiler* prof, uint32_t n, const float4* pm, GridP g, int ts, int tsx, int tsy, uint32_t* raw, uint32_t* out,
                      uint32_t* out_ext, int d_ext)
{
    ProfScope ps(prof, "tile_hmax", s);
    const uint32_t nt = (uint32_t)tsx * (uint32_t)tsy;
    (void)hipMemsetAsync(raw, 0, (size_t)nt * 4, s);
    if (n) hipLaunchKernelGGL(k_tile_hmax, dim3((n + 255) / 256), dim3(256), 0, s, n, pm, g, ts, tsx, raw);
    hipLaunchKernelGGL(k_tile_dilate, dim3((nt + 255) / 256), dim3(256), 0, s, tsx, tsy, 1, raw, out);
    if (out_ext) hipLaunchKernelGGL(k_tile_dilate, dim3((nt + 255) / 256), dim3(256), 0, s, tsx, tsy, d_ext, raw, out_ext);
}

void launch_tile_redilate(hipStream_t s, Profiler* prof, int tsx, int tsy, int d, const uint32_t* raw, uint32_t* out)
{
    ProfScope ps(prof, "tile_hmax", s);
    const uint32_t nt = (uint32_t)tsx * (uint32_t)tsy;
    hipLaunchKernelGGL(k_tile_dilate, dim3((nt + 255) / 256), dim3(256), 0, s, tsx, tsy, d, raw, out);
}
