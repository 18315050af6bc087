// Kinematic analysis of clips of 3D joints (angle/main.py of the reference): the 14 per-frame series, their 28 change
// series, the facing heading, the split into turns and the per-turn statistics.  tests/kinematics_restated.py is the
// restatement; rules: include/skimi.h and DESIGN §2 "Kinematics".
//
// Three launches for all clips:
//  (a) kin_series_kernel: one thread per (clip, frame) -> the base series and the heading, written series-major
//      ([clips, 42, frames]) so that the passes over time of (b) and (c) read neighbouring addresses.
//  (b) kin_turns_kernel: one workgroup per clip -> the change series and the whole heading pipeline.  The clip's arrays
//      (three of `frames` doubles) live in LDS or in a workspace; the code is the same, only the pointer differs.  The fill
//      needs the last finite index to the left and the next to the right, the greedy boundary walk the next extremum at or
//      after a frame: all three are integer max / min scans, exact in any order.  With the "next extremum" table the walk,
//      sequential by nature, is one lane making one step per boundary rather than per frame.  The unwrap's running sum is
//      the same blocked scan on doubles: chunks of ceil(T / 256) samples in time order, then the chunk totals in order, so
//      its order is a function of the clip's length alone.
//  (c) kin_stats_kernel: one wave per (clip, turn slot, series): per-lane strided sums in time order, then a fixed xor
//      butterfly; slots at and beyond the clip's turn count (read from device memory) are filled with NaN / 0.
// All arithmetic is float64 and the file is compiled without FMA contraction.  No floating-point atomics.
#include <math.h>

#include "common.h"
#include "fp64_util.h"
#include "reduce.h"

namespace skimi {
namespace {

constexpr int kThreads = 256;
constexpr int kRoles = SKIMI_KIN_ROLES;
constexpr int kBase = SKIMI_KIN_BASE_SERIES;
constexpr int kSeries = SKIMI_KIN_SERIES;
constexpr long kMaxElems = 1L << 40;
constexpr double kPi = 3.14159265358979323846;
constexpr double kDeg = 180.0 / kPi, kRad = kPi / 180.0;

struct KinArgs {
    const double* X;
    const int32_t* lengths;
    double *series, *heading, *hs, *vs, *dh, *stats, *ws;
    uint8_t* boundary;
    int32_t *n_turns, *turn_frames, *dir, *counts;
    long B, T;
    int J, m, w1, w2, max_turns, down;
    int idx[kRoles];
    double upu[3], thr;
};

__device__ inline int clip_len(const KinArgs& a, long b) {
    return a.lengths ? (int)min(max((long)a.lengths[b], 0L), a.T) : (int)a.T;
}

struct Pt {
    double v[3];
    bool ok;
};

__device__ inline Pt load_joint(const double* frame, int j) {
    Pt p;
    if (j < 0) {
        p.v[0] = p.v[1] = p.v[2] = qnan();
        p.ok = false;
        return p;
    }
    p.v[0] = frame[3 * j], p.v[1] = frame[3 * j + 1], p.v[2] = frame[3 * j + 2];
    p.ok = is_fin(p.v[0]) && is_fin(p.v[1]) && is_fin(p.v[2]);
    return p;
}

// v / |v|; false where the norm is zero or not finite
__device__ inline bool unit3(const double* v, double* u) {
    const double n = sqrt(dot3(v, v));
    if (n == 0.0 || !is_fin(n)) return false;
    u[0] = v[0] / n, u[1] = v[1] / n, u[2] = v[2] / n;
    return true;
}

__device__ inline double angle_abc(const Pt& a, const Pt& b, const Pt& c) {
    if (!(a.ok && b.ok && c.ok)) return qnan();
    const double ba[3] = {a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2]};
    const double bc[3] = {c.v[0] - b.v[0], c.v[1] - b.v[1], c.v[2] - b.v[2]};
    const double na = sqrt(dot3(ba, ba)), nc = sqrt(dot3(bc, bc));
    if (na == 0.0 || nc == 0.0) return qnan();
    double cs = dot3(ba, bc) / (na * nc);
    cs = cs < -1.0 ? -1.0 : cs > 1.0 ? 1.0 : cs;      // a NaN cosine stays NaN, as np.clip leaves it
    return acos(cs) * kDeg;
}

// the mean of the finite ones of two joints
__device__ inline Pt centre(const Pt& a, const Pt& b) {
    Pt c;
    if (a.ok && b.ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c.v[k] = (a.v[k] + b.v[k]) / 2.0;
        c.ok = is_fin(c.v[0]) && is_fin(c.v[1]) && is_fin(c.v[2]);
        return c;
    }
    if (a.ok) return a;
    if (b.ok) return b;
    c.v[0] = c.v[1] = c.v[2] = qnan();
    c.ok = false;
    return c;
}

__device__ inline double tilt(const Pt& to, const Pt& from, const double* l, const double* u, const double* f) {
    const double v[3] = {to.v[0] - from.v[0], to.v[1] - from.v[1], to.v[2] - from.v[2]};
    if (!(is_fin(v[0]) && is_fin(v[1]) && is_fin(v[2]))) return qnan();
    const double d = dot3(v, l);
    const double p[3] = {v[0] - d * l[0], v[1] - d * l[1], v[2] - d * l[2]};
    if (!(is_fin(p[0]) && is_fin(p[1]) && is_fin(p[2]))) return qnan();
    double q[3];
    if (!unit3(p, q)) return qnan();
    double cs = dot3(q, u);
    cs = cs < -1.0 ? -1.0 : cs > 1.0 ? 1.0 : cs;
    const double th = acos(cs) * kDeg;
    return dot3(q, f) >= 0.0 ? th : -th;
}

// ---- (a) base series and heading: one thread per (clip, frame) --------------------------------------------------------
__global__ __launch_bounds__(kThreads) void kin_series_kernel(KinArgs a) {
    const long g = (long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= a.B * a.T) return;
    const long b = g / a.T, t = g - b * a.T;
    double out[kBase], head = qnan();
#pragma unroll
    for (int k = 0; k < kBase; ++k) out[k] = qnan();
    if (t < clip_len(a, b)) {
        const double* frame = a.X + (b * a.T + t) * (long)a.J * 3;
        const Pt sho_l = load_joint(frame, a.idx[SKIMI_KIN_SHOULDER_L]), sho_r = load_joint(frame, a.idx[SKIMI_KIN_SHOULDER_R]);
        const Pt elb_l = load_joint(frame, a.idx[SKIMI_KIN_ELBOW_L]), elb_r = load_joint(frame, a.idx[SKIMI_KIN_ELBOW_R]);
        const Pt hip_l = load_joint(frame, a.idx[SKIMI_KIN_HIP_L]), hip_r = load_joint(frame, a.idx[SKIMI_KIN_HIP_R]);
        const Pt knee_l = load_joint(frame, a.idx[SKIMI_KIN_KNEE_L]), knee_r = load_joint(frame, a.idx[SKIMI_KIN_KNEE_R]);
        const Pt foot_l = load_joint(frame, a.idx[SKIMI_KIN_FOOT_L]), foot_r = load_joint(frame, a.idx[SKIMI_KIN_FOOT_R]);
        const Pt hand_l = load_joint(frame, a.idx[SKIMI_KIN_HAND_L]), hand_r = load_joint(frame, a.idx[SKIMI_KIN_HAND_R]);
        const Pt neck = load_joint(frame, a.idx[SKIMI_KIN_NECK]);
        out[0] = angle_abc(hip_l, knee_l, foot_l);
        out[1] = angle_abc(hip_r, knee_r, foot_r);
        out[2] = angle_abc(sho_l, elb_l, hand_l);
        out[3] = angle_abc(sho_r, elb_r, hand_r);
        out[4] = angle_abc(neck, sho_l, elb_l);
        out[5] = angle_abc(neck, sho_r, elb_r);
        out[6] = angle_abc(neck, hip_l, knee_l);
        out[7] = angle_abc(neck, hip_r, knee_r);
        const Pt pelvis = centre(hip_l, hip_r), shoulder = centre(sho_l, sho_r), knee = centre(knee_l, knee_r);
        out[8] = angle_abc(shoulder, pelvis, knee);
        if (is_fin(out[0]) && is_fin(out[1])) out[9] = out[0] - out[1];
        if (pelvis.ok) {
            if (elb_l.ok) {
                const double dx = elb_l.v[0] - pelvis.v[0], dz = elb_l.v[2] - pelvis.v[2];
                out[10] = sqrt(dx * dx + dz * dz);
            }
            if (elb_r.ok) {
                const double dx = elb_r.v[0] - pelvis.v[0], dz = elb_r.v[2] - pelvis.v[2];
                out[11] = sqrt(dx * dx + dz * dz);
            }
        }
        double lr[3];
        bool have = false;
        if (hip_l.ok && hip_r.ok) {
            have = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) lr[k] = hip_r.v[k] - hip_l.v[k];
        } else if (sho_l.ok && sho_r.ok) {
            have = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) lr[k] = sho_r.v[k] - sho_l.v[k];
        }
        double l[3], c[3], f[3];
        if (have && unit3(lr, l)) {
            if (a.down)
                cross3(a.upu, l, c);
            else
                cross3(l, a.upu, c);
            if (unit3(c, f)) {
                out[12] = tilt(shoulder, pelvis, l, a.upu, f);
                out[13] = tilt(knee, pelvis, l, a.upu, f);
                head = atan2(f[0], f[2]) * kDeg;
            }
        }
    }
    double* s = a.series + b * kSeries * a.T + t;
#pragma unroll
    for (int k = 0; k < kBase; ++k) s[k * a.T] = out[k];
    a.heading[g] = head;
}

// ---- (b) changes and turns: one workgroup per clip --------------------------------------------------------------------
struct OpMax {
    __device__ int operator()(int x, int y) const { return max(x, y); }
};
struct OpMin {
    __device__ int operator()(int x, int y) const { return min(x, y); }
};
struct OpSum {
    __device__ double operator()(double x, double y) const { return x + y; }
};

// In-place inclusive scan of a[0..n) by the workgroup (rev: from the last element down).  Thread t scans the chunk of
// c = ceil(n / 256) elements t c .. in order; wave 0 scans the 256 chunk totals (four per lane in order, then the lanes in
// a fixed shuffle tree); every element then takes op(total of the chunks before, own running value).  part: 256 values in
// LDS.  Ends with a barrier.
template <class V, class Op>
__device__ void block_scan(V* a, int n, bool rev, V ident, Op op, V* part) {
    const int tid = threadIdx.x, c = (n + kThreads - 1) / kThreads;
    const int lo = min(tid * c, n), hi = min(lo + c, n);
    V run = ident;
    for (int j = lo; j < hi; ++j) {
        V* p = a + (rev ? n - 1 - j : j);
        run = op(run, *p);
        *p = run;
    }
    part[tid] = run;
    __syncthreads();
    if (tid < 64) {
        V e[4], s = ident;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[k] = s;
            s = op(s, part[4 * tid + k]);
        }
        V inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const V u = __shfl_up(inc, o, 64);
            if (tid >= o) inc = op(u, inc);
        }
        V exc = __shfl_up(inc, 1, 64);
        if (tid == 0) exc = ident;
#pragma unroll
        for (int k = 0; k < 4; ++k) part[4 * tid + k] = op(exc, e[k]);
    }
    __syncthreads();
    const V pre = part[tid];
    for (int j = lo; j < hi; ++j) {
        V* p = a + (rev ? n - 1 - j : j);
        *p = op(pre, *p);
    }
    __syncthreads();
}

// the mean of the samples of x[i - w/2 .. i + w/2] inside 0 .. n - 1, summed in ascending order
__device__ inline double box_mean(const double* x, int i, int n, int w) {
    const int lo = max(i - w / 2, 0), hi = min(i + w / 2, n - 1);
    double s = 0.0;
    for (int j = lo; j <= hi; ++j) s += x[j];
    return s / (double)(hi - lo + 1);
}

__global__ __launch_bounds__(kThreads) void kin_turns_kernel(KinArgs a) {
    extern __shared__ double lds[];
    __shared__ double part_d[kThreads];
    __shared__ int part_i[kThreads];
    __shared__ int n_valid;
    const long b = blockIdx.x;
    const int tid = threadIdx.x, T = (int)a.T, n = clip_len(a, b);
    const long Tp = (a.T + 1) & ~1L;                   // keeps every array 16-byte aligned
    double* A = a.ws ? a.ws + b * 3 * Tp : lds;
    double *Bf = A + Tp, *Cf = Bf + Tp;
    int *L = reinterpret_cast<int*>(Bf), *R = reinterpret_cast<int*>(Cf);
    const double* h = a.heading + b * a.T;
    double *hs = a.hs + b * a.T, *vs = a.vs + b * a.T;
    uint8_t* bd = a.boundary + b * a.T;
    const double nan = qnan();

    // the change series
    double* s0 = a.series + b * kSeries * a.T;
    for (int k = 0; k < kBase; ++k) {
        const double* s = s0 + (long)k * a.T;
        double *d = s0 + (long)(kBase + 2 * k) * a.T, *ad = d + a.T;
        for (int i = tid; i < T; i += kThreads) {
            double v = nan;
            if (i >= 1 && i < n) {
                const double p = s[i - 1], c = s[i];
                if (is_fin(p) && is_fin(c)) v = c - p;
            }
            d[i] = v;
            ad[i] = fabs(v);
        }
    }
    // defaults of everything the walk may leave alone
    for (int i = tid; i < T; i += kThreads) bd[i] = 0;
    for (int k = tid; k < a.max_turns; k += kThreads) {
        const long r = b * a.max_turns + k;
        a.turn_frames[2 * r] = a.turn_frames[2 * r + 1] = 0;
        a.dh[r] = nan;
        a.dir[r] = 0;
    }
    for (int i = n + tid; i < T; i += kThreads) hs[i] = vs[i] = nan;
    if (tid == 0) n_valid = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += kThreads) {
        const bool ok = is_fin(h[i]);
        mine += ok;
        L[i] = ok ? i : -1;
        R[i] = ok ? i : n;
    }
    if (mine) atomicAdd(&n_valid, mine);              // an integer count: exact in any order
    __syncthreads();
    if (n_valid < 5) {                                 // rule 1 (uniform: every thread reads the same count)
        for (int i = tid; i < n; i += kThreads) hs[i] = vs[i] = nan;
        if (tid == 0) a.n_turns[b] = 0;
        return;
    }
    block_scan(L, n, false, -1, OpMax(), part_i);      // the last finite heading at or before i
    block_scan(R, n, true, n, OpMin(), part_i);        // the next at or after i
    // rule 2 and the radians of rule 3
    for (int i = tid; i < n; i += kThreads) {
        double v = h[i];
        if (!is_fin(v)) {
            const int l = L[i], r = R[i];
            if (l < 0)
                v = h[r];
            else if (r >= n)
                v = h[l];
            else
                v = (h[r] - h[l]) / (double)(r - l) * (double)(i - l) + h[l];
        }
        A[i] = v * kRad;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
        double c = 0.0;
        if (i >= 1) {
            const double dd = A[i] - A[i - 1];
            double md = fmod(dd + kPi, 2.0 * kPi);     // np.mod: the sign of the divisor
            if (md < 0.0) md += 2.0 * kPi;
            md -= kPi;
            if (md == -kPi && dd > 0.0) md = kPi;
            c = fabs(dd) < kPi ? 0.0 : md - dd;
        }
        Bf[i] = c;
    }
    __syncthreads();
    block_scan(Bf, n, false, 0.0, OpSum(), part_d);
    for (int i = tid; i < n; i += kThreads) Cf[i] = (i >= 1 ? A[i] + Bf[i] : A[i]) * kDeg;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) hs[i] = A[i] = box_mean(Cf, i, n, a.w1);       // rule 4
    __syncthreads();
    for (int i = tid; i < n; i += kThreads)                                                 // rule 5 (n >= 5 here)
        Bf[i] = i == 0 ? A[1] - A[0] : i == n - 1 ? A[n - 1] - A[n - 2] : (A[i + 1] - A[i - 1]) / 2.0;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) vs[i] = Cf[i] = box_mean(Bf, i, n, a.w2);
    __syncthreads();
    int* nxt = reinterpret_cast<int*>(Bf);             // the gradient is done with
    for (int i = tid; i < n; i += kThreads) nxt[i] = (i >= 1 && Cf[i - 1] * Cf[i] < 0.0) ? i : n;
    __syncthreads();
    block_scan(nxt, n, true, n, OpMin(), part_i);      // the next extremum at or after i
    if (tid == 0) {                                    // rules 6 and 7: one step per boundary
        int s = 0, nt = 0;
        for (;;) {
            const long q = (long)s + a.m;
            int e = q <= n - 1 ? nxt[q] : n;
            bool last = false;
            if (e >= n) {
                if (n - 1 - s < 1) break;              // the last boundary is T - 1 already
                e = n - 1;
                last = true;
            }
            if (!(e - s + 1 < a.m)) {
                const double dh = A[e] - A[s];
                if (!(fabs(dh) < a.thr) && nt < a.max_turns) {
                    const long r = b * a.max_turns + nt;
                    a.turn_frames[2 * r] = s;
                    a.turn_frames[2 * r + 1] = e;
                    a.dh[r] = dh;
                    a.dir[r] = dh > 0.0 ? 1 : -1;
                    bd[s] = bd[e] = 1;
                    ++nt;
                }
            }
            if (last) break;
            s = e;
        }
        a.n_turns[b] = nt;
    }
}

// ---- (c) per-turn statistics: one wave per (clip, turn slot, series) --------------------------------------------------
__global__ __launch_bounds__(kThreads) void kin_stats_kernel(KinArgs a) {
    const long w = (long)blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (w >= a.B * a.max_turns * kSeries) return;
    const long r = w / kSeries;                        // (clip, slot)
    const int k = (int)(w - r * kSeries);
    const long b = r / a.max_turns;
    const int slot = (int)(r - b * a.max_turns);
    double mean = qnan(), sd = qnan(), lo = qnan(), hi = qnan();
    int cnt = 0;
    if (slot < a.n_turns[b]) {
        const int s = a.turn_frames[2 * r], e = a.turn_frames[2 * r + 1];
        const double* x = a.series + (b * kSeries + k) * a.T;
        double sum = 0.0, mn = INFINITY, mx = -INFINITY;
        for (int i = s + lane; i <= e; i += 64) {
            const double v = x[i];
            if (is_fin(v)) {
                sum += v;
                mn = fmin(mn, v);
                mx = fmax(mx, v);
                ++cnt;
            }
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            mn = fmin(mn, __shfl_xor(mn, o, 64));
            mx = fmax(mx, __shfl_xor(mx, o, 64));
        }
        if (cnt > 0) {
            mean = sum / (double)cnt;
            double ss = 0.0;
            for (int i = s + lane; i <= e; i += 64) {
                const double v = x[i];
                if (is_fin(v)) ss += (v - mean) * (v - mean);
            }
            sd = sqrt(wave_sum(ss) / (double)cnt);
            lo = mn, hi = mx;
        }
    }
    if (lane == 0) {
        double* o = a.stats + w * 4;
        o[0] = mean, o[1] = sd, o[2] = lo, o[3] = hi;
        a.counts[w] = cnt;
    }
}

inline long kin_max_turns(long frames, int m) { return frames > 0 ? (frames - 1) / m + 1 : 0; }

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

size_t skimi_kin_workspace_bytes(int64_t clips, int64_t frames) {
    if (clips <= 0 || frames <= 0 || frames > 0x7fffffffLL || clips > kMaxElems / frames) return 0;
    return (size_t)clips * 3 * (size_t)((frames + 1) & ~1LL) * sizeof(double);
}

int skimi_kinematics(const double* X, const int32_t* lengths, int64_t clips, int64_t frames, int32_t joints,
                     const int32_t* layout, const double* up, int32_t min_turn_frames, double min_heading_change_deg,
                     int32_t heading_window, int32_t velocity_window, int32_t max_turns, void* workspace,
                     size_t workspace_bytes, double* series, double* heading, double* heading_smooth, double* velocity_smooth,
                     uint8_t* boundary, int32_t* n_turns, int32_t* turn_frames, double* turn_heading_change,
                     int32_t* turn_direction, double* turn_stats, int32_t* turn_counts, void* stream) {
    SKIMI_CHECK_ARG(clips >= 0 && frames >= 0 && frames <= 0x7fffffffLL - kThreads && joints >= 1 &&
                        (frames == 0 || clips <= kMaxElems / frames / joints / 3),
                    "skimi_kinematics: clips = %lld, frames = %lld, joints = %d outside clips >= 0, 0 <= frames < 2^31 - 256, joints >= 1, "
                    "clips * frames * joints * 3 <= 2^40", (long long)clips, (long long)frames, joints);
    SKIMI_CHECK_ARG(clips <= 0x7fffffffLL, "skimi_kinematics: clips = %lld exceeds 2^31 - 1", (long long)clips);
    SKIMI_CHECK_ARG(layout && up, "skimi_kinematics: NULL layout or up");
    for (int r = 0; r < kRoles; ++r)
        SKIMI_CHECK_ARG(layout[r] >= -1 && layout[r] < joints, "skimi_kinematics: layout[%d] = %d outside -1 .. joints - 1 = %d", r,
                        layout[r], joints - 1);
    const double un = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
    SKIMI_CHECK_ARG(isfinite(up[0]) && isfinite(up[1]) && isfinite(up[2]) && isfinite(un) && un > 0.0,
                    "skimi_kinematics: up = (%g, %g, %g) is not a finite non-zero vector", up[0], up[1], up[2]);
    SKIMI_CHECK_ARG(heading_window >= 3 && heading_window % 2 == 1 && velocity_window >= 3 && velocity_window % 2 == 1,
                    "skimi_kinematics: windows %d, %d are not odd numbers >= 3", heading_window, velocity_window);
    SKIMI_CHECK_ARG(min_turn_frames >= 1, "skimi_kinematics: min_turn_frames = %d < 1", min_turn_frames);
    SKIMI_CHECK_ARG(!isnan(min_heading_change_deg), "skimi_kinematics: min_heading_change_deg is NaN");
    const long mt = kin_max_turns(frames, min_turn_frames);
    SKIMI_CHECK_ARG(max_turns == mt, "skimi_kinematics: max_turns = %d, the outputs must be sized for (frames - 1) / min_turn_frames + 1 = %ld",
                    max_turns, mt);
    SKIMI_CHECK_ARG(mt == 0 || clips <= (1L << 32) / kSeries / mt,
                    "skimi_kinematics: clips * max_turns * 42 = %lld * %ld * 42 exceeds 2^32", (long long)clips, mt);
    if (clips == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(n_turns, "skimi_kinematics: NULL n_turns");
    if (frames > 0) {
        SKIMI_CHECK_ARG(X && series && heading && heading_smooth && velocity_smooth && boundary && turn_frames && turn_heading_change &&
                            turn_direction && turn_stats && turn_counts, "skimi_kinematics: NULL input or output");
        if (workspace)
            SKIMI_CHECK_ARG(workspace_bytes >= skimi_kin_workspace_bytes(clips, frames) && ((uintptr_t)workspace & 7) == 0,
                            "skimi_kinematics: the workspace has %zu bytes, skimi_kin_workspace_bytes asks for %zu (8-byte aligned)",
                            workspace_bytes, skimi_kin_workspace_bytes(clips, frames));
        else
            SKIMI_CHECK_ARG(frames <= SKIMI_KIN_LDS_FRAMES, "skimi_kinematics: frames = %lld > %d needs a workspace", (long long)frames,
                            SKIMI_KIN_LDS_FRAMES);
    }
    KinArgs a;
    a.X = X, a.lengths = lengths;
    a.series = series, a.heading = heading, a.hs = heading_smooth, a.vs = velocity_smooth, a.dh = turn_heading_change;
    a.stats = turn_stats, a.ws = frames > 0 ? (double*)workspace : nullptr;
    a.boundary = boundary, a.n_turns = n_turns, a.turn_frames = turn_frames, a.dir = turn_direction, a.counts = turn_counts;
    a.B = clips, a.T = frames, a.J = joints, a.m = min_turn_frames, a.w1 = heading_window, a.w2 = velocity_window;
    a.max_turns = (int)mt, a.down = up[1] < 0.0;
    for (int r = 0; r < kRoles; ++r) a.idx[r] = layout[r];
    for (int k = 0; k < 3; ++k) a.upu[k] = up[k] / un;
    a.thr = min_heading_change_deg;
    hipStream_t st = (hipStream_t)stream;
    if (frames > 0) {
        hipLaunchKernelGGL(kin_series_kernel, dim3((unsigned)cdiv(clips * frames, kThreads)), dim3(kThreads), 0, st, a);
        SKIMI_LAUNCH_CHECK();
    }
    const size_t lds = a.ws ? 0 : 3 * (size_t)((frames + 1) & ~1LL) * sizeof(double);
    hipLaunchKernelGGL(kin_turns_kernel, dim3((unsigned)clips), dim3(kThreads), lds, st, a);
    SKIMI_LAUNCH_CHECK();
    if (mt > 0) {
        hipLaunchKernelGGL(kin_stats_kernel, dim3((unsigned)cdiv(clips * mt * kSeries, kThreads / 64)), dim3(kThreads), 0, st, a);
        SKIMI_LAUNCH_CHECK();
    }
    return SKIMI_OK;
}

}  // extern "C"
