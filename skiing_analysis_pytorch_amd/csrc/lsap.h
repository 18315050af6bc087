// The rectangular linear sum assignment problem solved by ONE WAVE: the shortest-augmenting-path method with dual
// variables in float64 (Crouse 2016, the method behind scipy.optimize.linear_sum_assignment), written once for the batch
// kernel (the costs in global memory) and the box tracker (the costs in LDS) of assign.hip: `Cost` is how an entry is read.
// The rules are in include/skimi.h ("linear assignment"); tests/assign_restated.py is the restatement, and the kernels are
// bitwise that restatement: every float64 operation below is written in the order the restatement performs it, nothing is
// fused (-ffp-contract=off) and no sum is taken across lanes.
//
// The caller passes nr <= nc (it reads the transpose otherwise).  Lane l owns the columns l, l + 64, ...: their tentative
// distance sp, dual v, predecessor row, "visited" flag are touched by that lane alone while a path grows, so a Dijkstra
// step needs no barrier: a scan of the owned columns, then the (value, index) butterfly of reduce.h.  u, row4col and
// col4row are read by every lane and written between barriers only.
#pragma once
#include <limits.h>

#include "reduce.h"

namespace skimi {

struct LsapState {
    double *sp, *v, *u;                       // [P] each: tentative distances and duals of the columns, duals of the rows
    int *pred, *row4col, *col4row, *seen;     // [P] each
};
// bytes of state for problems of at most P rows and P columns
__host__ __device__ constexpr size_t lsap_state_bytes(int P) { return (size_t)P * (3 * sizeof(double) + 4 * sizeof(int)); }
__device__ inline LsapState lsap_carve(double* base, int P) {
    LsapState s;
    s.sp = base, s.v = base + P, s.u = base + 2 * P;
    s.pred = reinterpret_cast<int*>(base + 3 * P);
    s.row4col = s.pred + P, s.col4row = s.pred + 2 * P, s.seen = s.pred + 3 * P;
    return s;
}

// Solves rows 0 .. nr - 1 against columns 0 .. nc - 1, 0 <= nr <= nc <= P, called by all 64 lanes of a one-wave workgroup.
// On return (a barrier stands behind the last write) col4row[i] is the column of row i and row4col[j] the row of column j
// or -1.  false: some step found no column at a finite distance (the arithmetic overflowed); the maps are then unspecified.
template <class Cost>
__device__ inline bool lsap_wave(int nr, int nc, const Cost& cost, const LsapState& s) {
    const int lane = threadIdx.x & 63;
    const double inf = __builtin_huge_val();
    for (int j = lane; j < nc; j += 64) s.v[j] = 0.0, s.row4col[j] = -1;
    for (int i = lane; i < nr; i += 64) s.u[i] = 0.0, s.col4row[i] = -1;
    __syncthreads();
    for (int cur = 0; cur < nr; ++cur) {      // rows are inserted in ascending order
        for (int j = lane; j < nc; j += 64) s.sp[j] = inf, s.pred[j] = -1, s.seen[j] = 0;
        double minv = 0.0;
        int i = cur, sink = -1;
        // every step visits one more column and at most cur of them are assigned: at most cur + 1 steps
        for (int step = 0; step <= cur && sink < 0; ++step) {
            const double ui = s.u[i];
            double low = inf;
            int idx = INT_MAX;
            for (int j = lane; j < nc; j += 64) {
                if (s.seen[j]) continue;
                const double r = ((minv + cost(i, j)) - ui) - s.v[j];
                double d = s.sp[j];
                if (r < d) d = r, s.sp[j] = r, s.pred[j] = i;
                if (d < low) low = d, idx = j;      // ascending j: a tie stays with the lower column
            }
            wave_argmin(low, idx);                  // the smallest distance, ties to the LOWEST column; uniform
            if (idx == INT_MAX) return false;
            minv = low;
            if ((idx & 63) == lane) s.seen[idx] = 1;
            const int r4 = s.row4col[idx];
            if (r4 < 0) sink = idx;
            else i = r4;
        }
        if (sink < 0) return false;                 // cannot happen (see the step bound); never walk a path that has no end
        // the duals: every visited column other than the sink is assigned, to a visited row
        for (int j = lane; j < nc; j += 64)
            if (s.seen[j] && j != sink) {
                const double d = minv - s.sp[j];
                const int r = s.row4col[j];
                s.u[r] = s.u[r] + d;
                s.v[j] = s.v[j] - d;
            }
        if (lane == 0) s.u[cur] = s.u[cur] + minv;
        __syncthreads();                            // row4col was read above and pred written by its owners
        if (lane == 0) {
            int j = sink;
            for (int step = 0; step <= cur; ++step) {   // flip the path back to `cur`
                const int r = s.pred[j];
                s.row4col[j] = r;
                const int next = s.col4row[r];
                s.col4row[r] = j;
                j = next;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    return true;
}

}  // namespace skimi
