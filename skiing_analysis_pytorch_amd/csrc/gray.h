// The gray value of a B, G, R(, A) byte pixel (rule 1 of the chessboard block of include/skimi.h), shared by the image-feature
// kernels: features.hip and sift.hip.
#pragma once
#include "common.h"

namespace skimi {

template <int CH>
__device__ __forceinline__ int orb_gray(const unsigned char* p) {
    if (CH == 1) return p[0];
    return (3735 * (int)p[0] + 19235 * (int)p[1] + 9798 * (int)p[2] + 16384) >> 15;
}

}  // namespace skimi
