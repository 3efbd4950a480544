// Layout of the prepared MANO asset table (`poem_mano_prepare`, csrc/mano.hip's header), shared by the kernels that read it:
// mano.hip (the layer) and mano_fit.hip (the fit) -- and the two tables of the 21-joint hand order both write their joints by.
#pragma once
#include <hip/hip_runtime.h>

namespace {
constexpr int NV = 778, NJ = 16, NPOSE = 135, NBETA = 10;
constexpr int VP = 832;                    // vertices padded to 13 tiles of 64
constexpr int K4 = 37;                     // 148 / 4 coefficient groups (10 shape + 135 pose + 3 zero)
constexpr int OFF_VT = 0;                  // [3][VP]
constexpr int OFF_D = OFF_VT + 3 * VP;     // [K4][3][VP][4]
constexpr int OFF_W = OFF_D + K4 * 3 * VP * 4;   // [NJ][VP]
constexpr int OFF_JT = OFF_W + NJ * VP;    // [48]
constexpr int OFF_JSD = OFF_JT + 48;       // [48][10]
constexpr int TABLE_FLOATS = OFF_JSD + 48 * NBETA;
// finger-tip vertices (joints 16..20 of [16 kinematic joints | 5 tips]) and the source row of each joint of the 21-joint order
__constant__ int kTips[5] = {745, 317, 444, 556, 673};
__constant__ int kOrder[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
const int kOrderHost[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
}  // namespace
