// Arguments of the loss kernels (loss.hip); filled by poem_loss_terms (ops.cpp) from include/poem_hip.h's poem_loss_cfg_t.
#pragma once
#include <hip/hip_runtime.h>

// slots of the result array, in the key order of upstream's loss_dict (lib/models/POEM.py:380,451-465)
enum { LOSS_HEATMAP = 0, LOSS_J3D, LOSS_MESH, LOSS_V3D, LOSS_RECON, LOSS_J2D, LOSS_V2D, LOSS_POSE, LOSS_SHAPE, LOSS_TOTAL, LOSS_NTERMS };
// block partials in the workspace: view blocks write LOSS_VIEW_SLOTS doubles, sample blocks LOSS_SAMPLE_SLOTS
#define LOSS_VIEW_GROUPS 4      // blocks of 256 threads per view: 21 joints + 778 vertices = 799 points
#define LOSS_VIEW_SLOTS 3       // heat-map joints | projected joints | projected vertices
#define LOSS_SAMPLE_SLOTS 5     // joints | joints from mesh | vertices | pose | shape

struct LossArgs {
  const float* coords;          // (B, 799, 3) last decoder layer: 21 joints then 778 vertices
  const float* pred_uv;         // (BN, 21, 2)
  const float* pred_pose;       // (B, 16, 3)   parametric only
  const float* pred_shape;      // (B, 10)      parametric only
  const float* gt_joints;       // (B, 21, 3)
  const float* gt_verts;        // (B, 778, 3)
  const float* gt_uv;           // (BN, 21, 2)
  const float* intr;            // (BN, 3, 3)
  const float* extr;            // (BN, 4, 4) camera -> master
  const int* view_offsets;      // (B + 1) device prefix sums
  const float* mano_pose;       // (BN, 16, 3)  parametric only
  const float* mano_shape;      // (BN, 10)     parametric only
  const float* jreg;            // (16, 778)
  double w_joints, w_verts, w_joints_2d, w_verts_2d, w_heatmap, w_pose, w_shape;
  double img_scale;             // sqrt(W^2 + H^2)
  int joints_l2, verts_l2, parametric, center_idx;
  int B, BN;
  int view_groups;              // 1 when the vertices are not projected, else LOSS_VIEW_GROUPS
  double* part;                 // workspace: (BN * view_groups, LOSS_VIEW_SLOTS) then (B, LOSS_SAMPLE_SLOTS)
  double* out;                  // (LOSS_NTERMS)
};
