// The similarity of PAEval.align_w_scale (lib/metrics/pa_eval.py:104-124), solved by one wave: the one body behind pa_epe_kernel
// (metrics.hip), which reduces the aligned set to a mean distance, and pa_align_kernel (meshscore.hip), which writes it out.
//   centre both point sets, scale each to unit Frobenius norm (+1e-8), R, s = scipy.linalg.orthogonal_procrustes(gt_n, pred_n)
//   [R = U V^T, s = sum(w) for gt_n^T pred_n = U w V^T; no reflection handling -- exactly as upstream],
//   aligned = pred_n R^T s * s_gt + mean_gt.
// The 3x3 polar factor comes from a fp64 Jacobi eigen-decomposition of M^T M -- and, where a set is flat or a line, so that a
// singular value vanishes, from M itself, so that R is orthogonal whenever M is not 0.
#pragma once
#include "common.h"

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct PaSolve {
  double mp[3], mg[3];     // means of pred and gt
  double R[3][3], scale;   // rotation and sum of singular values
  double s1, s2;           // |gt_c| + 1e-8, |pred_c| + 1e-8
};

// Every lane of the wave calls it with the sample's p, g (P,3) and ends with the same values.
__device__ __forceinline__ void pa_solve(const float* __restrict__ p, const float* __restrict__ g, int P, int lane, PaSolve& o) {
  double sp[3] = {0, 0, 0}, sg[3] = {0, 0, 0};
  for (int i = lane; i < P; i += 64)
    for (int d = 0; d < 3; ++d) { sp[d] += p[i * 3 + d]; sg[d] += g[i * 3 + d]; }
  double mp[3], mg[3];
  for (int d = 0; d < 3; ++d) { mp[d] = wave_sum(sp[d]) / P; mg[d] = wave_sum(sg[d]) / P; }
  double np2 = 0, ng2 = 0, M[3][3] = {};            // M = gt_c^T pred_c (un-normalised; scales factor out below)
  for (int i = lane; i < P; i += 64) {
    double pc[3], gc[3];
    for (int d = 0; d < 3; ++d) { pc[d] = p[i * 3 + d] - mp[d]; gc[d] = g[i * 3 + d] - mg[d]; }
    for (int d = 0; d < 3; ++d) { np2 += pc[d] * pc[d]; ng2 += gc[d] * gc[d]; }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] += gc[r] * pc[c];
  }
  np2 = wave_sum(np2); ng2 = wave_sum(ng2);
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] = wave_sum(M[r][c]);
  const double s1 = sqrt(ng2) + 1e-8, s2 = sqrt(np2) + 1e-8;       // pa_eval.py:113-116
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] /= (s1 * s2);
  // S = M^T M = V w^2 V^T  (Jacobi, fp64)
  double S[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { S[r][c] = 0; for (int k = 0; k < 3; ++k) S[r][c] += M[k][r] * M[k][c]; }
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[1][2] * S[1][2];
    const double diag = S[0][0] * S[0][0] + S[1][1] * S[1][1] + S[2][2] * S[2][2];
    if (off <= 1e-40 * diag) break;
    for (int pp = 0; pp < 2; ++pp)
      for (int q = pp + 1; q < 3; ++q) {
        if (S[pp][q] == 0.0) continue;
        const double theta = (S[q][q] - S[pp][pp]) / (2.0 * S[pp][q]);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 3; ++k) { const double a = S[k][pp], bq = S[k][q]; S[k][pp] = c * a - s * bq; S[k][q] = s * a + c * bq; }
        for (int k = 0; k < 3; ++k) { const double a = S[pp][k], bq = S[q][k]; S[pp][k] = c * a - s * bq; S[q][k] = s * a + c * bq; }
        for (int k = 0; k < 3; ++k) { const double a = V[k][pp], bq = V[k][q]; V[k][pp] = c * a - s * bq; V[k][q] = s * a + c * bq; }
      }
  }
  double w[3], scale = 0;
  for (int k = 0; k < 3; ++k) { w[k] = sqrt(fmax(S[k][k], 0.0)); scale += w[k]; }
  // R = U V^T = M V diag(1/w) V^T   (3x3)
  double MV[3][3], R[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { MV[r][c] = 0; for (int k = 0; k < 3; ++k) MV[r][c] += M[r][k] * V[k][c]; }
  const double wmax = fmax(w[0], fmax(w[1], w[2]));
  int k3 = w[1] < w[0] ? 1 : 0;
  if (w[2] < w[k3]) k3 = 2;
  int k1 = (k3 + 1) % 3, k2 = (k3 + 2) % 3;
  if (w[k2] > w[k1]) { const int t = k1; k1 = k2; k2 = t; }          // w[k1] >= w[k2] >= w[k3]
  if (wmax > 0.0 && w[k3] < 1e-3 * wmax) {
    // A flat point set (three points, a planar ground truth) or a line: M^T M squares the conditioning, so w[k3] has lost its
    // digits -- or is 0 while the other set does extend along that direction.  R stays orthogonal, as scipy's is: the left
    // vectors come from M itself (u = M v / |M v|, the second made orthogonal to the first; for rank 1 any unit vector across
    // the first), the third pair is completed by cross products, and its sign and singular value are u3^T M v3, which keeps
    // its sign down to rounding of M.  Where that value is exactly 0 either sign is an answer of upstream's.
    double u1[3], u2[3], n1 = 0, n2 = 0, dot = 0;
    for (int r = 0; r < 3; ++r) n1 += MV[r][k1] * MV[r][k1];
    n1 = sqrt(n1);
    for (int r = 0; r < 3; ++r) { u1[r] = MV[r][k1] / n1; dot += u1[r] * MV[r][k2]; }
    for (int r = 0; r < 3; ++r) { u2[r] = MV[r][k2] - dot * u1[r]; n2 += u2[r] * u2[r]; }
    n2 = sqrt(n2);
    double un = n2;
    if (!(n2 > 1e-12 * n1)) {
      int m = fabs(u1[1]) < fabs(u1[0]) ? 1 : 0;
      if (fabs(u1[2]) < fabs(u1[m])) m = 2;
      un = 0;
      for (int r = 0; r < 3; ++r) { u2[r] = (r == m ? 1.0 : 0.0) - u1[m] * u1[r]; un += u2[r] * u2[r]; }
      un = sqrt(un);
    }
    for (int r = 0; r < 3; ++r) u2[r] /= un;
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {V[1][k1] * V[2][k2] - V[2][k1] * V[1][k2], V[2][k1] * V[0][k2] - V[0][k1] * V[2][k2],
                          V[0][k1] * V[1][k2] - V[1][k1] * V[0][k2]};
    double d3 = 0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) d3 += u3[r] * M[r][c] * v3[c];
    const double sg = d3 < 0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r][c] = u1[r] * V[c][k1] + u2[r] * V[c][k2] + sg * u3[r] * v3[c];
    scale = n1 + n2 + fabs(d3);
  } else {
    // well conditioned -- or M = 0 (a prediction that is one point), where R = 0 and scale = 0 put every point on the gt's mean
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        R[r][c] = 0;
        for (int k = 0; k < 3; ++k) if (w[k] > 1e-14 * wmax) R[r][c] += MV[r][k] / w[k] * V[c][k];
      }
  }
  for (int d = 0; d < 3; ++d) { o.mp[d] = mp[d]; o.mg[d] = mg[d]; }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) o.R[r][c] = R[r][c];
  o.scale = scale, o.s1 = s1, o.s2 = s2;
}

// aligned_i = (pred_c_i / s2) R^T * scale * s1 + mean_gt, in fp64: point i of p -> al[3]
__device__ __forceinline__ void pa_aligned_point(const PaSolve& o, const float* __restrict__ p, int i, double al[3]) {
  double pc[3];
  for (int d = 0; d < 3; ++d) pc[d] = (p[i * 3 + d] - o.mp[d]) / o.s2;
  for (int d = 0; d < 3; ++d) al[d] = (o.R[d][0] * pc[0] + o.R[d][1] * pc[1] + o.R[d][2] * pc[2]) * o.scale * o.s1 + o.mg[d];
}
