// Ordered stream compaction and exact top-M selection of the integer image kernels (chessboard.hip, features.hip, sift.hip,
// scene.hip).  Device helpers only; LDS stays declared in the kernel that calls them.  Everything here is integer and
// independent of the order in which waves run: the results are bitwise reproducible.
//  - compaction keeps the elements that pass a predicate, in index order, across workgroups, in two launches.  The count
//    launch stores each workgroup's survivors (tile_count); the write launch turns the counts into offsets (group_offsets)
//    and walks its tile in chunks of one element a thread (ordered_write, or ordered_rank by hand).
//  - selection keeps the m largest 64-bit keys of a stream, ties to the earlier element, in stream order: select_threshold
//    finds the key of descending rank m - 1, select_rank is the step of the ordered scatter that follows.
#pragma once
#include "common.h"
#include "reduce.h"

namespace skimi {

// The number of kept elements of this chunk ahead of the calling thread (earlier waves, then earlier lanes); `chunk`: the
// chunk's total.  wtot: kWaves counters in LDS.  The contract:
//  - every thread of the workgroup calls it, kept or not: there is one barrier inside (loops around it have a uniform trip
//    count);
//  - consecutive calls alternate between two `wtot` buffers (s_wtot[buf], buf ^= 1): a call never gets the buffer of the
//    call before it.  A wave that is past the barrier of call k may write the totals of call k + 1 while another still
//    reads those of call k, but none reaches call k + 2 before all have met call k + 1's barrier, their reads of call k
//    behind them: that is why one barrier a call suffices.
template <int kWaves>
__device__ __forceinline__ unsigned ordered_rank(bool kept, unsigned* wtot, unsigned& chunk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(kept);
    if (lane == 0) wtot[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned ahead = 0;
    chunk = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const unsigned c = wtot[k];
        if (k < wave) ahead += c;
        chunk += c;
    }
    return ahead + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// The preamble of a write launch: bc holds the counts of the stream's `groups` workgroups.  Afterwards s_total (LDS) is the
// count of the whole stream and s_offset (LDS) the rows ahead of workgroup g.  Integer sums, any order.  Two barriers.
template <int kThreads>
__device__ inline void group_offsets(const unsigned* __restrict__ bc, int groups, long g, unsigned& s_total, unsigned& s_offset) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_total = 0;
        s_offset = 0;
    }
    __syncthreads();
    unsigned tot = 0, off = 0;
    for (int i = tid; i < groups; i += kThreads) {
        const unsigned v = bc[i];
        tot += v;
        if (i < g) off += v;
    }
    tot = wave_sum(tot);
    off = wave_sum(off);
    if ((tid & 63) == 0) {
        atomicAdd(&s_total, tot);
        atomicAdd(&s_offset, off);
    }
    __syncthreads();
}

// The body of a count launch: how many i of [beg, end) pass pred(i).  s_cnt: one counter in LDS.  Two barriers; the
// result is the workgroup's (thread 0 stores it).
template <int kThreads, class Pred>
__device__ inline unsigned tile_count(long beg, long end, unsigned& s_cnt, Pred&& pred) {
    const int tid = threadIdx.x;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    unsigned cnt = 0;
    for (long i = beg + tid; i < end; i += kThreads) cnt += pred(i) ? 1u : 0u;
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    return s_cnt;
}

// The chunk loop of a write launch: emit(i, row) for every i of [beg, end) that passes pred(i), where row = row0 + the
// number of such elements ahead of i.  Every thread of the workgroup calls it with the same beg, end and row0; s_wtot: the
// two buffers of ordered_rank.  Capacity is the sink's business: row is not clipped.
template <int kThreads, class Pred, class Emit>
__device__ inline void ordered_write(long beg, long end, long row0, unsigned (*s_wtot)[kThreads / 64], Pred&& pred, Emit&& emit) {
    const int tid = threadIdx.x;
    int buf = 0;
    for (long i0 = beg; i0 < end; i0 += kThreads) {   // uniform trip count: every thread reaches the barrier
        const long i = i0 + tid;
        const bool kept = i < end && pred(i);
        unsigned chunk;
        const unsigned rank = ordered_rank<kThreads / 64>(kept, s_wtot[buf], chunk);
        if (kept) emit(i, row0 + rank);
        row0 += chunk;
        buf ^= 1;   // the next chunk writes the other totals: one barrier per chunk
    }
}

// Exact selection by the whole workgroup: T, the key of descending rank m - 1 (0-based) among the keys, and `need`, how many
// of the keys equal to T belong to the m largest; the same in every thread.  for_keys(f) calls f(key) for each of the
// calling thread's keys (reduce.h's wave_select2 has the same shape); there are more than m keys.  Eight passes of an
// 8-bit histogram from the top byte down.  s_hist: kThreads = 256 bins in LDS; s_digit, s_need: LDS.
template <int kThreads, class ForKeys>
__device__ inline void select_threshold(unsigned m, ForKeys&& for_keys, unsigned* s_hist, unsigned& s_digit, unsigned& s_need,
                                        unsigned long long& T, unsigned& need) {
    static_assert(kThreads == 256, "a bin a thread");
    const int tid = threadIdx.x;
    T = 0;
    need = m;
    for (int pass = 7; pass >= 0; --pass) {
        s_hist[tid] = 0;
        __syncthreads();
        for_keys([&](unsigned long long key) {
            if (pass == 7 || (key >> (8 * (pass + 1))) == (T >> (8 * (pass + 1)))) atomicAdd(&s_hist[(unsigned)(key >> (8 * pass)) & 255u], 1u);
        });
        __syncthreads();
        if (tid == 0) {
            unsigned left = need;
            int d = 255;
            for (; d > 0; --d) {
                if (s_hist[d] >= left) break;
                left -= s_hist[d];
            }
            s_digit = (unsigned)d;
            s_need = left;
        }
        __syncthreads();
        T |= (unsigned long long)s_digit << (8 * pass);
        need = s_need;
        __syncthreads();                  // s_hist and s_need are rewritten by the next pass
    }
}

// One chunk of the ordered scatter behind select_threshold: is this thread's element among the selected, and how many
// selected elements of the chunk are ahead of it (`rank`; `chunk`: the chunk's total).  live: the thread has an element that
// may be kept.  cut: a threshold was selected (otherwise every live element is kept and T, need are not read).  Keys above
// T are kept, and the first `need` of those equal to T in stream order: eq0 carries their number over the chunks.  Two
// ordered_rank calls, on s_wtot[0] and s_wtot[1]: the caller alternates s_wtot between two such pairs, and every thread
// of the workgroup calls this.
template <int kWaves>
__device__ __forceinline__ bool select_rank(unsigned long long key, bool live, bool cut, unsigned long long T, unsigned need,
                                            unsigned& eq0, unsigned (*s_wtot)[kWaves], unsigned& rank, unsigned& chunk) {
    const bool eq = live && cut && key == T;
    unsigned eq_chunk;
    const unsigned eq_rank = eq0 + ordered_rank<kWaves>(eq, s_wtot[0], eq_chunk);
    const bool kept = live && (!cut || key > T || (eq && eq_rank < need));
    rank = ordered_rank<kWaves>(kept, s_wtot[1], chunk);
    eq0 += eq_chunk;
    return kept;
}

}  // namespace skimi
