// Conversion of a clip between the COCO-17 and the H36M-17 skeleton on the device (VideoPose3D/coco_hm36.py: coco_to_h36m,
// h36m_to_coco; the host functions of skeleton.py are the restatement; rules: DESIGN §2 "Skeleton conversion").
//
// One thread per frame, C = 2 or 3 coordinates per joint, float64, compiled without FMA contraction; NaN propagates through
// the arithmetic as on the host.  h36m_to_coco with synthesized eyes and ears tests the CLIP MEAN of the shoulder width
// against 1e-8 (the reference's quirk): every workgroup sums the widths in the same fixed order (a thread's frames in
// ascending order, a shuffle tree per wave, the four waves in order), so every frame sees the same bits.  That is one
// launch at the price of frames^2 / 256 reads in all: nothing for a clip of hundreds of frames (three workgroups at T =
// 600), quadratic for long ones, so this form is limited to 2^20 frames (2^32 reads, from L2).
#include <math.h>

#include "common.h"
#include "fp64_util.h"
#include "reduce.h"

namespace skimi {
namespace {

constexpr int kJ = 17;
constexpr int kThreads = 256;
constexpr long kMaxFrames = 1L << 34, kMaxFaceFrames = 1L << 20;

// COCO-17: 0 nose, 1 l_eye, 2 r_eye, 3 l_ear, 4 r_ear, 5 l_sho, 6 r_sho, 7 l_elb, 8 r_elb, 9 l_wri, 10 r_wri, 11 l_hip,
// 12 r_hip, 13 l_knee, 14 r_knee, 15 l_ank, 16 r_ank.  H36M-17: 0 pelvis, 1-3 right leg, 4-6 left leg, 7 spine, 8 thorax,
// 9 neck, 10 head, 11-13 left arm, 14-16 right arm.  kCocoOfH36m[h]: the COCO joint copied to H36M joint h (-1: computed)
__constant__ int kCocoOfH36m[kJ] = {-1, 12, 14, 16, 11, 13, 15, -1, -1, 0, -1, 5, 7, 9, 6, 8, 10};
// kH36mOfCoco[c]: the H36M joint copied to COCO joint c (-1: eyes and ears)
__constant__ int kH36mOfCoco[kJ] = {9, -1, -1, -1, -1, 11, 14, 12, 15, 13, 16, 4, 1, 5, 2, 6, 3};

template <int C>
__device__ inline double normc(const double* v) {
    return C == 2 ? sqrt(v[0] * v[0] + v[1] * v[1]) : sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

template <int C>
__global__ __launch_bounds__(kThreads) void coco_to_h36m_kernel(const double* __restrict__ X, long T, int synth_head, double* __restrict__ Y) {
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const double* x = X + t * kJ * C;
    double* y = Y + t * kJ * C;
#pragma unroll
    for (int h = 0; h < kJ; ++h) {
        const int src = kCocoOfH36m[h];
        if (src < 0) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) y[h * C + c] = x[src * C + c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double pelvis = (x[11 * C + c] + x[12 * C + c]) * 0.5, thorax = (x[5 * C + c] + x[6 * C + c]) * 0.5;
        const double nose = x[c], eyes = (x[1 * C + c] + x[2 * C + c]) * 0.5;
        y[0 * C + c] = pelvis;
        y[8 * C + c] = thorax;
        y[7 * C + c] = (pelvis + thorax) * 0.5;
        y[10 * C + c] = synth_head ? nose + 0.5 * (nose - eyes) : nose;
    }
}

template <int C>
__global__ __launch_bounds__(kThreads) void h36m_to_coco_kernel(const double* __restrict__ X, long T, int synth_face, double* __restrict__ Y) {
    __shared__ double red[kThreads / 64][1];
    bool degenerate = false;
    if (synth_face) {                          // before any thread leaves: block_sum holds a barrier
        double part[1] = {0.0};
        for (long u = threadIdx.x; u < T; u += kThreads) {
            double d[C];
#pragma unroll
            for (int c = 0; c < C; ++c) d[c] = X[(u * kJ + 11) * C + c] - X[(u * kJ + 14) * C + c];
            part[0] += normc<C>(d);
        }
        block_sum(part, red);
        degenerate = total<kThreads / 64>(red, 0) / (double)T < 1e-8;            // a NaN mean: the normal branch
    }
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= T) return;
    const double nan = qnan();
    const double* x = X + t * kJ * C;
    double* y = Y + t * kJ * C;
#pragma unroll
    for (int k = 0; k < kJ; ++k) {
        const int src = kH36mOfCoco[k];
#pragma unroll
        for (int c = 0; c < C; ++c) y[k * C + c] = src < 0 ? nan : x[src * C + c];
    }
    if (!synth_face) return;
    double sv[C], up[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        sv[c] = degenerate ? (c == 0 ? 1.0 : 0.0) : x[11 * C + c] - x[14 * C + c];
        up[c] = x[10 * C + c] - x[9 * C + c];
    }
    const double w = normc<C>(sv), un = normc<C>(up);
    const double eye_side = 0.25 * w, eye_up = 0.15 * w, ear_side = 0.35 * w, ear_up = 0.10 * w;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double side = sv[c] / (w + 1e-9), u = up[c] / (un + 1e-9), head = x[10 * C + c];
        y[1 * C + c] = (head + eye_side * side) - eye_up * u;
        y[2 * C + c] = (head + -eye_side * side) - eye_up * u;
        y[3 * C + c] = (head + ear_side * side) - ear_up * u;
        y[4 * C + c] = (head + -ear_side * side) - ear_up * u;
    }
}

}  // namespace
}  // namespace skimi

using namespace skimi;

extern "C" {

int skimi_convert_skeleton(const double* X, int64_t frames, int32_t coords, int32_t direction, int32_t synthesize, double* Y,
                           void* stream) {
    SKIMI_CHECK_ARG(coords == 2 || coords == 3, "skimi_convert_skeleton: coords = %d is neither 2 nor 3", coords);
    SKIMI_CHECK_ARG(direction == SKIMI_SKELETON_COCO_TO_H36M || direction == SKIMI_SKELETON_H36M_TO_COCO,
                    "skimi_convert_skeleton: unknown direction %d", direction);
    // the clip mean of the synthesized face is re-summed by every workgroup: frames^2 / 256 reads, so that form stops at 2^20
    const bool clip_mean = direction == SKIMI_SKELETON_H36M_TO_COCO && synthesize != 0;
    SKIMI_CHECK_ARG(frames >= 0 && frames <= (clip_mean ? kMaxFaceFrames : kMaxFrames),
                    "skimi_convert_skeleton: frames = %lld outside 0..2^34 (0..2^20 for h36m_to_coco with synthesize)", (long long)frames);
    if (frames == 0) return SKIMI_OK;
    SKIMI_CHECK_ARG(X && Y && X != Y, "skimi_convert_skeleton: NULL input or output, or Y is X");
    const dim3 grid((unsigned)cdiv(frames, kThreads)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    const int syn = synthesize != 0;
    if (direction == SKIMI_SKELETON_COCO_TO_H36M) {
        if (coords == 2) hipLaunchKernelGGL(coco_to_h36m_kernel<2>, grid, block, 0, st, X, (long)frames, syn, Y);
        else hipLaunchKernelGGL(coco_to_h36m_kernel<3>, grid, block, 0, st, X, (long)frames, syn, Y);
    } else {
        if (coords == 2) hipLaunchKernelGGL(h36m_to_coco_kernel<2>, grid, block, 0, st, X, (long)frames, syn, Y);
        else hipLaunchKernelGGL(h36m_to_coco_kernel<3>, grid, block, 0, st, X, (long)frames, syn, Y);
    }
    SKIMI_LAUNCH_CHECK();
    return SKIMI_OK;
}

}  // extern "C"
