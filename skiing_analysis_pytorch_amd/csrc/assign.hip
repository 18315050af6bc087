// Association and tracking (DESIGN §2 "Association and tracking"): a batch of rectangular linear assignment problems in one
// launch, and a box tracker that keeps persistent ids over a clip.  Both run lsap.h's one-wave solver; the rules are in
// include/skimi.h and tests/assign_restated.py is the restatement.  One wave a problem / a clip, no atomics and nothing
// between workgroups: the results are bitwise reproducible, bitwise the restatement's, and those of a problem alone.
#include <math.h>

#include "common.h"
#include "lsap.h"

namespace skimi {

namespace {

constexpr int kWave = 64;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) < __builtin_huge_val(); }   // false for NaN

// entry (i, j) of the problem the solver sees: the block itself, or its transpose, by the two strides
struct StridedCost {
    const double* c;
    long si, sj;
    __device__ __forceinline__ double operator()(int i, int j) const { return c[i * si + j * sj]; }
};

// ---- linear assignment: a wave a problem ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void assign_kernel(const double* __restrict__ cost, const int* __restrict__ n_rows,
                                                       const int* __restrict__ n_cols, int N, int M, int* __restrict__ row_to_col,
                                                       int* __restrict__ col_to_row, double* __restrict__ total, int* __restrict__ status) {
    extern __shared__ double s_state[];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const LsapState s = lsap_carve(s_state, max(N, M));
    const double* c = cost + b * N * M;
    const int nr = n_rows ? min(max(n_rows[b], 0), N) : N;     // a count outside 0 .. N reads nothing outside the matrix
    const int nc = n_cols ? min(max(n_cols[b], 0), M) : M;
    int* rc = row_to_col + b * N;
    int* cr = col_to_row + b * M;

    bool bad = false;
    for (int i = 0; i < nr; ++i)
        for (int j = lane; j < nc; j += kWave) bad |= !finite_d(c[(size_t)i * M + j]);
    bad = __any(bad);

    const bool tr = nr > nc;                                   // the transpose is solved: its rows are the block's columns
    const StridedCost rd{c, tr ? 1 : M, tr ? M : 1};
    const bool ok = !bad && lsap_wave(tr ? nc : nr, tr ? nr : nc, rd, s);
    const int* of_row = tr ? s.row4col : s.col4row;
    const int* of_col = tr ? s.col4row : s.row4col;
    for (int i = lane; i < N; i += kWave) {
        const int j = ok && i < nr ? of_row[i] : -1;
        rc[i] = j;
        if (i < nr) s.sp[i] = j >= 0 ? c[(size_t)i * M + j] : 0.0;     // sp is free now: the assigned costs, for the sum
    }
    for (int j = lane; j < M; j += kWave) cr[j] = ok && j < nc ? of_col[j] : -1;
    __syncthreads();
    if (lane == 0) {
        double t = 0.0;
        if (ok) {
            for (int i = 0; i < nr; ++i)
                if (of_row[i] >= 0) t = t + s.sp[i];           // in ascending row order
        } else {
            t = __builtin_nan("");
        }
        total[b] = t;
        status[b] = ok ? 0 : 1;
    }
}

// ---- box tracker: a wave a clip ------------------------------------------------------------------------------------------------
struct Box {
    double x1, y1, x2, y2;
};
// IoU = inter / union, 0 when union <= 0; the restatement's order of operations
__device__ __forceinline__ double box_iou(const Box& a, const Box& b) {
    const double iw = fmin(a.x2, b.x2) - fmax(a.x1, b.x1);
    const double ih = fmin(a.y2, b.y2) - fmax(a.y1, b.y1);
    const double inter = (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
    const double aa = (a.x2 - a.x1) * (a.y2 - a.y1);
    const double ab = (b.x2 - b.x1) * (b.y2 - b.y1);
    const double uni = (aa + ab) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

struct LdsCost {
    const double* c;   // [64][64], detections x live tracks
    bool tr;
    __device__ __forceinline__ double operator()(int i, int j) const { return tr ? c[j * kWave + i] : c[i * kWave + j]; }
};

__global__ __launch_bounds__(kWave) void link_kernel(const double* __restrict__ boxes, const double* __restrict__ scores, int T, int N, int K,
                                                     double iou_thr, int max_age, double new_score, int* __restrict__ ids,
                                                     int* __restrict__ n_tracks, int* __restrict__ table, int* __restrict__ overflow) {
    __shared__ double s_cost[kWave * kWave];
    __shared__ double s_state[lsap_state_bytes(kWave) / sizeof(double)];
    __shared__ Box s_det[kWave], s_trk[kWave];
    __shared__ int s_age[kWave], s_first[kWave], s_last[kWave], s_hits[kWave], s_det_at[kWave], s_live_at[kWave], s_hit[kWave];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const LsapState s = lsap_carve(s_state, kWave);
    const unsigned long long below = (1ull << lane) - 1ull;
    s_age[lane] = 0, s_first[lane] = -1, s_last[lane] = -1, s_hits[lane] = 0;
    int ntr = 0, over = 0;
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const size_t at = (b * T + t) * N + lane;
        Box box{0.0, 0.0, 0.0, 0.0};
        bool valid = false, may_start = false;
        if (lane < N) {
            const double* p = boxes + at * 4;
            box = Box{p[0], p[1], p[2], p[3]};
            valid = finite_d(box.x1) && finite_d(box.y1) && finite_d(box.x2) && finite_d(box.y2);
            may_start = valid && (!scores || scores[at] >= new_score);
        }
        // rule 1: the live tracks and the detections, each in ascending order
        const bool live = lane < ntr && s_age[lane] <= max_age;
        const unsigned long long bv = __ballot(valid), bl = __ballot(live);
        const int D = __popcll(bv), L = __popcll(bl), my = __popcll(bv & below);
        if (valid) s_det_at[my] = lane, s_det[lane] = box;
        if (live) s_live_at[__popcll(bl & below)] = lane;
        s_hit[lane] = 0;
        __syncthreads();
        // rule 2
        for (int e = lane; e < D * L; e += kWave) {
            const int d = e / L, k = e - d * L;
            s_cost[d * kWave + k] = 1.0 - box_iou(s_det[s_det_at[d]], s_trk[s_live_at[k]]);
        }
        __syncthreads();
        const bool tr = D > L;
        const bool ok = lsap_wave(tr ? L : D, tr ? D : L, LdsCost{s_cost, tr}, s);
        // rule 3
        int id = -1, k = -1;
        if (valid && ok) {
            const int m = tr ? s.row4col[my] : s.col4row[my];
            if (m >= 0 && box_iou(box, s_trk[s_live_at[m]]) >= iou_thr) k = s_live_at[m];
        }
        __syncthreads();                             // every old box is read before one is replaced
        if (k >= 0) {
            id = k;
            s_trk[k] = box, s_hit[k] = 1, s_last[k] = t, s_hits[k] += 1;
        }
        // rules 3 and 4: new tracks in detection order while ids are left
        const bool start = may_start && k < 0;
        const unsigned long long bs = __ballot(start);
        const int wanted = __popcll(bs), room = min(wanted, K - ntr);
        if (start) {
            const int nid = ntr + __popcll(bs & below);
            if (nid < K) {
                id = nid;
                s_trk[nid] = box, s_hit[nid] = 1, s_first[nid] = t, s_last[nid] = t, s_hits[nid] = 1;
            }
        }
        over += wanted - room;
        ntr += room;
        __syncthreads();
        // rule 5
        if (lane < ntr) s_age[lane] = s_hit[lane] ? 0 : s_age[lane] + 1;
        if (lane < N) ids[at] = id;
        __syncthreads();
    }
    if (lane < K) {
        int* row = table + (b * K + lane) * 3;
        row[0] = s_first[lane], row[1] = s_last[lane], row[2] = s_hits[lane];
    }
    if (lane == 0) n_tracks[b] = ntr, overflow[b] = over;
}

}  // namespace

}  // namespace skimi

using namespace skimi;

extern "C" {

int skimi_linear_assignment(const double* cost, const int32_t* n_rows, const int32_t* n_cols, int64_t B, int32_t N, int32_t M,
                            int32_t* row_to_col, int32_t* col_to_row, double* total, int32_t* status, void* stream) {
    SKIMI_CHECK_ARG(B >= 1 && B < (1ll << 31) && N >= 1 && M >= 1 && N <= SKIMI_ASSIGN_MAX && M <= SKIMI_ASSIGN_MAX,
                    "skimi_linear_assignment: B = %lld problems of %d x %d outside 1 <= B < 2^31, 1 <= N, M <= %d", (long long)B, N, M,
                    SKIMI_ASSIGN_MAX);
    SKIMI_CHECK_ARG(cost && row_to_col && col_to_row && total && status,
                    "skimi_linear_assignment: NULL cost, row_to_col, col_to_row, total or status");
    const size_t lds = lsap_state_bytes(N > M ? N : M);
    hipLaunchKernelGGL(assign_kernel, dim3((unsigned)B), dim3(kWave), lds, (hipStream_t)stream, cost, n_rows, n_cols, N, M, row_to_col,
                       col_to_row, total, status);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

int skimi_link_boxes(const double* boxes, const double* scores, int64_t B, int32_t T, int32_t N, int32_t K, double iou_threshold,
                     int32_t max_age, double new_score, int32_t* ids, int32_t* n_tracks, int32_t* table, int32_t* overflow, void* stream) {
    SKIMI_CHECK_ARG(B >= 1 && B < (1ll << 31) && T >= 1 && N >= 1 && N <= SKIMI_LINK_MAX && K >= 1 && K <= SKIMI_LINK_MAX &&
                        B * T * N < (1ll << 31),
                    "skimi_link_boxes: B = %lld clips of T = %d frames, N = %d boxes, K = %d tracks outside 1 <= B, T, 1 <= N, K <= %d, "
                    "B T N < 2^31", (long long)B, T, N, K, SKIMI_LINK_MAX);
    SKIMI_CHECK_ARG(max_age >= 0 && iou_threshold == iou_threshold && new_score == new_score,
                    "skimi_link_boxes: max_age = %d (>= 0), iou_threshold = %g, new_score = %g (not NaN)", max_age, iou_threshold, new_score);
    SKIMI_CHECK_ARG(boxes && ids && n_tracks && table && overflow, "skimi_link_boxes: NULL boxes, ids, n_tracks, table or overflow");
    hipLaunchKernelGGL(link_kernel, dim3((unsigned)B), dim3(kWave), 0, (hipStream_t)stream, boxes, scores, T, N, K, iou_threshold, max_age,
                       new_score, ids, n_tracks, table, overflow);
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
