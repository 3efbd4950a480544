// MANO -> OpenPose joint tables shared by the kernels that restate mano_to_openpose (lib/utils/transform.py:836-872 upstream):
// metrics.hip (mano_to_openpose_kernel) and loss.hip (the from-mesh joints of compute_loss).
#pragma once
#include <hip/hip_runtime.h>

// output joint o of the OpenPose order = row kOpenposeFromMano[o] of [16 regressed joints | 5 finger tips]
static __constant__ int kOpenposeFromMano[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
// the finger-tip vertices (CONST.MANO_KPID_2_VERTICES, lib/utils/misc.py:76-82)
static __constant__ int kTipVertex[5] = {744, 320, 443, 555, 672};
