// Ragged batched DLT triangulation of the 21 hand joints (the producer of `reference_joints`).
// Replaces lib/utils/triangulation.py:5-45 (batch_triangulate_dlt_torch) and the per-sample Python loop around it
// (lib/models/POEM.py:284-299 upstream): for every (sample, joint)
//   M_n = K_n . T_n[:3, :]            (T_n = inv(cam_extr_n) = master -> camera; fp32 like the reference's matmul)
//   A   = [u_n M_n[2] - M_n[0] ; v_n M_n[2] - M_n[1]]_n          (2 N_i x 4)
//   x   = right singular vector of A for the smallest singular value;  X = x[:3] / (x[3] + 1e-7)
// The reference calls torch.linalg.svd on every (2N x 4) matrix; here the 4x4 normal matrix A^T A is accumulated in
// fp64 and its smallest eigenvector found with cyclic Jacobi rotations in fp64 (same subspace).  Accuracy, measured on the
// conditioning ladder of tests/test_dlt_forms.py against the fp64 SVD of the same fp32 rows: for sigma1/sigma3 up to 1e4 every
// joint is within one fp32 rounding of the fp64 answer and closer to it than an fp32 SVD of those rows is; at 1e5 (a 0.03 mm
// baseline at 0.6 m) that no longer holds for every joint -- forming A^T A costs cond(A)^2 2^-53.  Physical rigs sit below 1e3.
// The sign of x is fixed to x[3] >= 0 (LAPACK returns either; with the + 1e-7 the two differ by 2e-7 |X| / x[3]).  A NaN or an
// infinite uv makes its joint NaN, a NaN camera its whole sample; nothing else is touched.
// dlt_kernel: one thread per (sample, joint), the whole stage is ~700 threads.
#include "common.h"

#define DLT_MODE_THRESHOLD 1
#define DLT_MODE_WEIGHTED 2

// Joint j of a sample over its views v0..v1 -> o[0..2]; returns the number of views that took part.  CONF = false is the plain
// solve (conf, mode and thr are not read).  CONF = true, the confidence-aware form (below): a view takes part when its
// confidence is above thr (mode 1), or both its rows are scaled by its confidence (mode 2).  Everything else is one
// arithmetic -- M and the rows in fp32, normal matrix and Jacobi in fp64, the sign, the +1e-7 of :43 -- so that confidence 1
// everywhere (mode 2) or a threshold of 0 with positive confidences (mode 1) gives the plain solve's bits.
template <bool CONF>
__device__ __forceinline__ int dlt_solve(const float* __restrict__ uv, const float* __restrict__ conf,
                                         const float* __restrict__ intr, const float* __restrict__ mat, int v0, int v1, int J,
                                         int j, int invert, int mode, double thr, float* __restrict__ o) {
  int used = 0;
  double G[4][4] = {};
  for (int v = v0; v < v1; ++v) {
    double cf = 1.0;
    if constexpr (CONF) {
      cf = (double)conf[(size_t)v * J + j];
      if (mode == DLT_MODE_THRESHOLD && !(cf > thr)) continue;                   // :135
    }
    ++used;
    float T[3][4];
    if (invert) {
      double Ti[16];
      invert4x4(mat + (size_t)v * 16, Ti);                                        // (common.h)
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T[r][c] = (float)Ti[r * 4 + c];
    } else {
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T[r][c] = mat[(size_t)v * 16 + r * 4 + c];
    }
    const float* K = intr + (size_t)v * 9;
    float M[3][4];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) M[r][c] = fmaf(K[r * 3 + 2], T[2][c], fmaf(K[r * 3 + 1], T[1][c], K[r * 3] * T[0][c]));
    const float u = uv[((size_t)v * J + j) * 2], w = uv[((size_t)v * J + j) * 2 + 1];
    float a0[4], a1[4];
    for (int c = 0; c < 4; ++c) { a0[c] = u * M[2][c] - M[0][c]; a1[c] = w * M[2][c] - M[1][c]; }
    if constexpr (CONF) {
      const double sc = mode == DLT_MODE_WEIGHTED ? cf : 1.0;
      double d0[4], d1[4];
      for (int c = 0; c < 4; ++c) { d0[c] = (double)a0[c] * sc; d1[c] = (double)a1[c] * sc; }
      for (int r = 0; r < 4; ++r)
        for (int c = r; c < 4; ++c) G[r][c] += d0[r] * d0[c] + d1[r] * d1[c];
    } else {
      for (int r = 0; r < 4; ++r)
        for (int c = r; c < 4; ++c) G[r][c] += (double)a0[r] * (double)a0[c] + (double)a1[r] * (double)a1[c];
    }
  }
  for (int r = 1; r < 4; ++r) for (int c = 0; c < r; ++c) G[r][c] = G[c][r];
  // cyclic Jacobi: G <- R^T G R, V <- V R
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int r = 0; r < 4; ++r) { diag += G[r][r] * G[r][r]; for (int c = r + 1; c < 4; ++c) off += G[r][c] * G[r][c]; }
    if (off <= 1e-40 * diag && diag < HUGE_VAL) break;                             // (inf <= inf: an infinite G, from an infinite uv, is
                                                                                   //  not converged; it rotates on into NaN, as a NaN does)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (G[p][q] == 0.0) continue;
        const double theta = (G[q][q] - G[p][p]) / (2.0 * G[p][q]);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 4; ++k) { const double gkp = G[k][p], gkq = G[k][q]; G[k][p] = c * gkp - s * gkq; G[k][q] = s * gkp + c * gkq; }
        for (int k = 0; k < 4; ++k) { const double gpk = G[p][k], gqk = G[q][k]; G[p][k] = c * gpk - s * gqk; G[q][k] = s * gpk + c * gqk; }
        for (int k = 0; k < 4; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
      }
  }
  int m = 0;
  for (int k = 1; k < 4; ++k) if (G[k][k] < G[m][m]) m = k;
  double x[4] = {V[0][m], V[1][m], V[2][m], V[3][m]};
  if (x[3] < 0) { x[0] = -x[0]; x[1] = -x[1]; x[2] = -x[2]; x[3] = -x[3]; }        // the sign of a singular vector is free
  const double den = x[3] + 1e-7;                                                  // triangulation.py:43
  o[0] = (float)(x[0] / den);
  o[1] = (float)(x[1] / den);
  o[2] = (float)(x[2] / den);
  return used;
}

__global__ __launch_bounds__(64) void dlt_kernel(const float* __restrict__ uv, const float* __restrict__ intr,
                                                 const float* __restrict__ mat, const int* __restrict__ offs,
                                                 float* __restrict__ out, int B, int J, int invert) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;                      // B * J fits an int (poem_triangulate_dlt): the last
  if (t >= (unsigned)(B * J)) return;                                            // block's spare threads stay below 2^32
  const int b = (int)(t / (unsigned)J), j = (int)(t % (unsigned)J);
  dlt_solve<false>(uv, nullptr, intr, mat, offs[b], offs[b + 1], J, j, invert, 0, 0.0, out + (size_t)t * 3);
}

extern "C" hipError_t poem_launch_dlt(const float* uv, const float* intr, const float* mat, const int* offs, float* out,
                                      int B, int J, int invert, hipStream_t s) {
  const unsigned total = (unsigned)B * (unsigned)J;                              // <= INT_MAX: the entry point refuses more
  hipLaunchKernelGGL(dlt_kernel, dim3((total + 63u) / 64u), dim3(64), 0, s, uv, intr, mat, offs, out, B, J, invert);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Confidence-aware form of the same solve.  Replaces lib/utils/triangulation.py:111-148 (triangulate_dlt) and the
// per-sample loop a caller would put around it: dlt_solve<true>; dlt_kernel stays the default route.
//   mode 1 (threshold), triangulation.py:133-147 as it runs: per joint, in order, a camera is selected when
//     conf > thr; while at most one camera is selected and thr > 0, thr -= 0.05 (fp64, :139).  `confi_thres` is the
//     function's own argument, so a lowered threshold is what the FOLLOWING joints of that sample start from.  That is
//     a sequential pass over the sample's joints: lane 0 of the sample's block runs it (J x N_i compares per
//     lowering) and leaves the threshold of every joint in LDS; the block's threads then solve one joint each over
//     the selected cameras.  No workspace, no second launch, nothing read back by the host.
//   mode 2 (weighted): both rows of view n are scaled by conf[n][j] (fp64, after the fp32 row is formed); no view is
//     dropped.  (Upstream has no weighted form; this is the usual confidence-weighted least squares.)
// One block per sample, thread j -> joint j (+64, ...).
__global__ __launch_bounds__(64) void dlt_conf_kernel(const float* __restrict__ uv, const float* __restrict__ conf,
                                                      const float* __restrict__ intr, const float* __restrict__ mat,
                                                      const int* __restrict__ offs, float* __restrict__ out,
                                                      int* __restrict__ sel_count, int J, int invert, int mode,
                                                      double threshold) {
  extern __shared__ double thr_of[];                                             // [J]: the threshold joint j is solved with
  const int b = blockIdx.x;
  const int v0 = offs[b], v1 = offs[b + 1];
  if (mode == DLT_MODE_THRESHOLD) {
    if (threadIdx.x == 0) {
      double thr = threshold;
      for (int j = 0; j < J; ++j) {
        while (thr > 0) {                                                        // :136 leaves the loop at thr <= 0
          int n = 0;
          for (int v = v0; v < v1; ++v) n += (double)conf[(size_t)v * J + j] > thr;
          if (n > 1) break;
          thr -= 0.05;                                                           // :139
        }
        thr_of[j] = thr;
      }
    }
    __syncthreads();
  }
  for (int j = threadIdx.x; j < J; j += blockDim.x) {
    const size_t t = (size_t)b * J + j;
    const int used = dlt_solve<true>(uv, conf, intr, mat, v0, v1, J, j, invert, mode, mode == DLT_MODE_THRESHOLD ? thr_of[j] : 0.0,
                                     out + t * 3);
    if (sel_count) sel_count[t] = used;
  }
}

// J doubles of LDS hold the per-joint thresholds: J <= 4096 (the release has 21).
extern "C" hipError_t poem_launch_dlt_confidence(const float* uv, const float* conf, const float* intr, const float* mat,
                                                 const int* offs, float* out, int* sel_count, int B, int J, int invert,
                                                 int mode, double threshold, hipStream_t s) {
  if (J > 4096) return hipErrorInvalidValue;
  const size_t lds = mode == DLT_MODE_THRESHOLD ? (size_t)J * sizeof(double) : 0;
  hipLaunchKernelGGL(dlt_conf_kernel, dim3(B), dim3(64), lds, s, uv, conf, intr, mat, offs, out, sel_count, J, invert, mode,
                     threshold);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Heat-map read-out in front of the triangulation (tail of heatmap_stage, lib/models/POEM.py:213-222 upstream, with
// integral_heatmap2d, lib/models/integal_pose.py:194-218): per (view, joint)
//   pdf = hmap / (sum(hmap) + 1e-6);  u = sum_x (x / W_h) * sum_y pdf[y][x];  v = sum_y (y / H_h) * sum_x pdf[y][x]
//   uv_im = (u * W_img, v * H_img)
// One wave per (view, joint); fp32 like the reference, fp64 only for the three running sums.
// CONF: also the joint's confidence = the maximum of the map (the peak that the expectation throws away; what
// triangulate_dlt's `confis` holds, lib/utils/triangulation.py:115), a NaN pixel making it NaN as torch.amax does.  The
// sums are untouched by it, so uv has the bits of the CONF = false instantiation, which is the kernel as it was.
template <bool CONF>
__global__ __launch_bounds__(256) void heatmap_uv_kernel(const float* __restrict__ hmap, float* __restrict__ uv,
                                                         float* __restrict__ conf, int maps, int hh, int hw, float img_w,
                                                         float img_h) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= maps) return;
  const float* h = hmap + (size_t)m * hh * hw;
  double s = 0, su = 0, sv = 0;
  float mx = -INFINITY;
  int bad = 0;
  for (int i = lane; i < hh * hw; i += 64) {
    const float v = h[i];
    const int y = i / hw, x = i - y * hw;
    s += v;
    su += (double)v * ((float)x / (float)hw);
    sv += (double)v * ((float)y / (float)hh);
    if (CONF) { mx = fmaxf(mx, v); bad |= v != v; }                              // fmaxf drops a NaN operand: flag it
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); su += __shfl_xor(su, o, 64); sv += __shfl_xor(sv, o, 64); }
  if (CONF) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); bad |= __shfl_xor(bad, o, 64); }
  }
  if (lane == 0) {
    const double den = (double)((float)s + 1e-6f);
    uv[(size_t)m * 2 + 0] = (float)(su / den) * img_w;
    uv[(size_t)m * 2 + 1] = (float)(sv / den) * img_h;
    if (CONF) conf[m] = bad ? __builtin_nanf("") : mx;
  }
}

extern "C" hipError_t poem_launch_heatmap_uv(const float* hmap, float* uv, int maps, int hh, int hw, float img_w,
                                             float img_h, hipStream_t s) {
  hipLaunchKernelGGL(heatmap_uv_kernel<false>, dim3((maps + 3) / 4), dim3(256), 0, s, hmap, uv, (float*)nullptr, maps, hh, hw,
                     img_w, img_h);
  return hipGetLastError();
}

extern "C" hipError_t poem_launch_heatmap_uv_conf(const float* hmap, float* uv, float* conf, int maps, int hh, int hw,
                                                  float img_w, float img_h, hipStream_t s) {
  hipLaunchKernelGGL(heatmap_uv_kernel<true>, dim3((maps + 3) / 4), dim3(256), 0, s, hmap, uv, conf, maps, hh, hw, img_w,
                     img_h);
  return hipGetLastError();
}
