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
// dlt_kernel: one thread per (sample, joint), the whole stage is ~700 threads.  dlt_conf_kernel: the same solve with views chosen
// or weighted by confidence.  dlt_robust_kernel: the same solve with the views that disagree with the others' geometry left out.
#include "common.h"

#define DLT_MODE_THRESHOLD 1
#define DLT_MODE_WEIGHTED 2

// The solve in three pieces, shared by every kernel of this file so that all of them have one arithmetic (a view set solved by one
// kernel has the bits another kernel gives it): dlt_view_matrix (M = K . T in fp32), dlt_add_view (the view's two fp32 rows into the
// fp64 normal matrix) and dlt_null_vector (cyclic Jacobi, the sign, the +1e-7 of :43).
__device__ __forceinline__ void dlt_view_matrix(const float* __restrict__ intr, const float* __restrict__ mat, int v, int invert,
                                                float M[3][4]) {
  float T[3][4];
  if (invert) {
    double Ti[16];
    invert4x4(mat + (size_t)v * 16, Ti);                                          // (common.h)
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T[r][c] = (float)Ti[r * 4 + c];
  } else {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) T[r][c] = mat[(size_t)v * 16 + r * 4 + c];
  }
  const float* K = intr + (size_t)v * 9;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) M[r][c] = fmaf(K[r * 3 + 2], T[2][c], fmaf(K[r * 3 + 1], T[1][c], K[r * 3] * T[0][c]));
}

// G (upper triangle) += the two rows of a view that saw the joint at (u, w).  SCALED: both rows times sc in fp64 (weighted mode).
template <bool SCALED>
__device__ __forceinline__ void dlt_add_view(const float M[3][4], float u, float w, double sc, double G[4][4]) {
  float a0[4], a1[4];
  for (int c = 0; c < 4; ++c) { a0[c] = u * M[2][c] - M[0][c]; a1[c] = w * M[2][c] - M[1][c]; }
  if constexpr (SCALED) {
    double d0[4], d1[4];
    for (int c = 0; c < 4; ++c) { d0[c] = (double)a0[c] * sc; d1[c] = (double)a1[c] * sc; }
    for (int r = 0; r < 4; ++r)
      for (int c = r; c < 4; ++c) G[r][c] += d0[r] * d0[c] + d1[r] * d1[c];
  } else {
    for (int r = 0; r < 4; ++r)
      for (int c = r; c < 4; ++c) G[r][c] += (double)a0[r] * (double)a0[c] + (double)a1[r] * (double)a1[c];
  }
}

// Upper triangle of the normal matrix -> X = x[:3] / (x[3] + 1e-7) of its smallest eigenvector x, in fp64.
__device__ __forceinline__ void dlt_null_vector(double G[4][4], double X[3]) {
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
  double gm = G[0][0];
  for (int k = 1; k < 4; ++k) if (G[k][k] < gm) { gm = G[k][k]; m = k; }
  double x[4];                                                                     // column m of V by selects: V[k][m] with a run-time
  for (int k = 0; k < 4; ++k) x[k] = m == 0 ? V[k][0] : m == 1 ? V[k][1] : m == 2 ? V[k][2] : V[k][3];   // m would put V in scratch
  if (x[3] < 0) { x[0] = -x[0]; x[1] = -x[1]; x[2] = -x[2]; x[3] = -x[3]; }        // the sign of a singular vector is free
  const double den = x[3] + 1e-7;                                                  // triangulation.py:43
  X[0] = x[0] / den;
  X[1] = x[1] / den;
  X[2] = x[2] / den;
}

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
    float M[3][4];
    dlt_view_matrix(intr, mat, v, invert, M);
    const float u = uv[((size_t)v * J + j) * 2], w = uv[((size_t)v * J + j) * 2 + 1];
    dlt_add_view<CONF>(M, u, w, CONF && mode == DLT_MODE_WEIGHTED ? cf : 1.0, G);
  }
  double X[3];
  dlt_null_vector(G, X);
  o[0] = (float)X[0];
  o[1] = (float)X[1];
  o[2] = (float)X[2];
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
// Outlier-robust form of the same solve (upstream has no counterpart: lib/utils/triangulation.py stops at triangulate_dlt).  A view
// whose 2-D joint is confidently wrong -- a heat map that peaks on another finger, the held object, the other hand -- is found from
// geometry alone.  Deterministic and exhaustive over minimal samples, no random sampling: per (sample, joint)
//   1. every pair (a < c) of the sample's N views gives a two-view solve X (fp64);
//   2. view v is an inlier of X iff |proj_v(X) - uv_v|^2 < px^2 AND depth_v(X) > 0 (both strict: a NaN is never an inlier); the
//      pair's key is (-count, sum of the inliers' r^2 in view order, a N + c), the smallest key wins;
//   3. with >= 2 inliers the joint is solved again over the inlier set (ascending, unweighted), else over all views with an
//      empty inlier set (count 0) -- the plain solve, NaN behaviour included.  A camera that is not finite sends its whole sample
//      down that second road: a NaN camera is a broken calibration and not an outlier, and it makes its sample NaN as it always has;
//   4. `refine` Gauss-Newton steps on the inliers' (after the fallback: all views') summed r^2 in fp64, 3x3 normal equations,
//      J = (M[:2,:3] - p M[2,:3]) / h[2]; a step is kept only while the cost gets strictly smaller.
// One wave per (sample, joint), four per block; grid (B, ceil(J / 4)).  The block's first N threads form their view's M once
// (dlt_view_matrix, the fp64 inverse included) into LDS, 12 floats per view.  The lanes of a wave stride over the N (N - 1) / 2
// pairs (one pass up to N = 11), each keeps its best key and inlier mask, __shfl_xor reduces them (the key is a strict total
// order, so every lane ends with the same winner whatever the lane order); refit and refinement run redundantly on all lanes
// (no broadcast), then lane v writes view v's inlier flag and residual.  The inlier set is one 64-bit mask: N <= 64.  A sample
// with fewer than 2 or more than 64 views is not solved: NaN joints and residuals, count 0 (the Python layer refuses it).
#define DLT_ROBUST_MAX_VIEWS 64

// r^2 of X in the view whose M is m[0..11]; *depth = h[2]
__device__ __forceinline__ double dlt_reproj2(const float* __restrict__ m, const double X[3], float u, float w, double* depth) {
  const double h0 = (double)m[0] * X[0] + (double)m[1] * X[1] + (double)m[2] * X[2] + (double)m[3];
  const double h1 = (double)m[4] * X[0] + (double)m[5] * X[1] + (double)m[6] * X[2] + (double)m[7];
  const double h2 = (double)m[8] * X[0] + (double)m[9] * X[1] + (double)m[10] * X[2] + (double)m[11];
  const double du = h0 / h2 - (double)u, dv = h1 / h2 - (double)w;
  *depth = h2;
  return du * du + dv * dv;
}

// the solve over the views of `mask` (bit v = view v0 + v), ascending
__device__ __forceinline__ void dlt_solve_mask(const float* __restrict__ Ms, const float* __restrict__ uvj, int N, int J,
                                               unsigned long long mask, double X[3]) {
  double G[4][4] = {};
  for (int v = 0; v < N; ++v) {
    if (!((mask >> v) & 1ull)) continue;
    float M[3][4];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) M[r][c] = Ms[v * 12 + r * 4 + c];
    dlt_add_view<false>(M, uvj[(size_t)v * J * 2], uvj[(size_t)v * J * 2 + 1], 1.0, G);
  }
  dlt_null_vector(G, X);
}

// sum over the views of `mask` of r^2 at X
__device__ __forceinline__ double dlt_mask_cost(const float* __restrict__ Ms, const float* __restrict__ uvj, int N, int J,
                                                unsigned long long mask, const double X[3]) {
  double cost = 0.0, depth;
  for (int v = 0; v < N; ++v)
    if ((mask >> v) & 1ull) cost += dlt_reproj2(Ms + v * 12, X, uvj[(size_t)v * J * 2], uvj[(size_t)v * J * 2 + 1], &depth);
  return cost;
}

__global__ __launch_bounds__(256) void dlt_robust_kernel(const float* __restrict__ uv, const float* __restrict__ intr,
                                                         const float* __restrict__ mat, const int* __restrict__ offs,
                                                         float* __restrict__ out, unsigned char* __restrict__ inlier,
                                                         int* __restrict__ count, float* __restrict__ resid, int J, int invert,
                                                         double px2, int refine) {
  __shared__ float Ms[DLT_ROBUST_MAX_VIEWS * 12];
  const int b = blockIdx.x, lane = threadIdx.x & 63;
  const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int v0 = offs[b], N = offs[b + 1] - v0;                                   // block-uniform
  const float qnan = __builtin_nanf("");
  if (N < 2 || N > DLT_ROBUST_MAX_VIEWS) {
    if (j < J) {
      const size_t t = (size_t)b * J + j;
      if (lane < 3) out[t * 3 + lane] = qnan;
      if (lane == 0 && count) count[t] = 0;
      for (int v = lane; v < N; v += 64) {
        if (inlier) inlier[(size_t)(v0 + v) * J + j] = 0;
        if (resid) resid[(size_t)(v0 + v) * J + j] = qnan;
      }
    }
    return;
  }
  int bad = 0;
  if ((int)threadIdx.x < N) {
    float M[3][4];
    dlt_view_matrix(intr, mat, v0 + (int)threadIdx.x, invert, M);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) { Ms[threadIdx.x * 12 + r * 4 + c] = M[r][c]; bad |= !(fabsf(M[r][c]) < INFINITY); }
  }
  bad = __syncthreads_or(bad);                                                    // (also the barrier behind the LDS writes)
  if (j >= J) return;                                                             // spare waves of the last block row
  const float* uvj = uv + ((size_t)v0 * J + j) * 2;                               // view v of this joint: uvj[v * J * 2 + {0, 1}]
  const unsigned long long all = N == 64 ? ~0ull : (1ull << N) - 1ull;

  // 1 + 2: pair hypotheses, each lane its best key
  int bcnt = -1, bid = 0x7fffffff;
  double bsum = 0.0;
  unsigned long long bmask = 0;
  if (!bad) {
    const int npairs = N * (N - 1) / 2;
    for (int p = lane; p < npairs; p += 64) {
      int a = 0, rem = p;
      while (rem >= N - 1 - a) { rem -= N - 1 - a; ++a; }                         // pairs in the order of a N + c
      const int c = a + 1 + rem;
      double X[3];
      dlt_solve_mask(Ms, uvj, N, J, (1ull << a) | (1ull << c), X);
      int cnt = 0;
      double sum = 0.0;
      unsigned long long mask = 0;
      for (int v = 0; v < N; ++v) {
        double depth;
        const double r2 = dlt_reproj2(Ms + v * 12, X, uvj[(size_t)v * J * 2], uvj[(size_t)v * J * 2 + 1], &depth);
        if (r2 < px2 && depth > 0.0) { ++cnt; sum += r2; mask |= 1ull << v; }
      }
      const int id = a * N + c;
      if (cnt > bcnt || (cnt == bcnt && (sum < bsum || (sum == bsum && id < bid)))) { bcnt = cnt; bsum = sum; bid = id; bmask = mask; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int ocnt = __shfl_xor(bcnt, o, 64), oid = __shfl_xor(bid, o, 64);
      const double osum = __shfl_xor(bsum, o, 64);
      const unsigned long long omask = __shfl_xor(bmask, o, 64);
      if (ocnt > bcnt || (ocnt == bcnt && (osum < bsum || (osum == bsum && oid < bid)))) { bcnt = ocnt; bsum = osum; bid = oid; bmask = omask; }
    }
  }

  // 3: refit over the winner's inliers, or the plain solve
  const bool fit = bcnt >= 2;
  const unsigned long long over = fit ? bmask : all;
  double X[3];
  dlt_solve_mask(Ms, uvj, N, J, over, X);

  // 4: Gauss-Newton on the summed r^2 of `over`
  if (refine > 0) {
    double cost = dlt_mask_cost(Ms, uvj, N, J, over, X);
    for (int it = 0; it < refine; ++it) {
      double A00 = 0, A01 = 0, A02 = 0, A11 = 0, A12 = 0, A22 = 0, g0 = 0, g1 = 0, g2 = 0;
      for (int v = 0; v < N; ++v) {
        if (!((over >> v) & 1ull)) continue;
        const float* m = Ms + v * 12;
        const double h0 = (double)m[0] * X[0] + (double)m[1] * X[1] + (double)m[2] * X[2] + (double)m[3];
        const double h1 = (double)m[4] * X[0] + (double)m[5] * X[1] + (double)m[6] * X[2] + (double)m[7];
        const double h2 = (double)m[8] * X[0] + (double)m[9] * X[1] + (double)m[10] * X[2] + (double)m[11];
        const double pu = h0 / h2, pv = h1 / h2;
        const double eu = pu - (double)uvj[(size_t)v * J * 2], ev = pv - (double)uvj[(size_t)v * J * 2 + 1];
        const double ju0 = ((double)m[0] - pu * (double)m[8]) / h2, ju1 = ((double)m[1] - pu * (double)m[9]) / h2,
                     ju2 = ((double)m[2] - pu * (double)m[10]) / h2;
        const double jv0 = ((double)m[4] - pv * (double)m[8]) / h2, jv1 = ((double)m[5] - pv * (double)m[9]) / h2,
                     jv2 = ((double)m[6] - pv * (double)m[10]) / h2;
        A00 += ju0 * ju0 + jv0 * jv0; A01 += ju0 * ju1 + jv0 * jv1; A02 += ju0 * ju2 + jv0 * jv2;
        A11 += ju1 * ju1 + jv1 * jv1; A12 += ju1 * ju2 + jv1 * jv2; A22 += ju2 * ju2 + jv2 * jv2;
        g0 += ju0 * eu + jv0 * ev; g1 += ju1 * eu + jv1 * ev; g2 += ju2 * eu + jv2 * ev;
      }
      // (J^T J) d = -J^T e by the adjugate of the symmetric 3x3
      const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
      const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
      const double det = A00 * c00 + A01 * c01 + A02 * c02;
      const double Y[3] = {X[0] - (c00 * g0 + c01 * g1 + c02 * g2) / det, X[1] - (c01 * g0 + c11 * g1 + c12 * g2) / det,
                           X[2] - (c02 * g0 + c12 * g1 + c22 * g2) / det};
      const double trial = dlt_mask_cost(Ms, uvj, N, J, over, Y);
      if (!(trial < cost)) break;                                                 // (a NaN trial stops here too)
      X[0] = Y[0]; X[1] = Y[1]; X[2] = Y[2];
      cost = trial;
    }
  }

  // 5: outputs
  const size_t t = (size_t)b * J + j;
  if (lane < 3) out[t * 3 + lane] = (float)(lane == 0 ? X[0] : lane == 1 ? X[1] : X[2]);
  if (lane == 0 && count) count[t] = fit ? bcnt : 0;
  if (lane < N) {
    const size_t e = (size_t)(v0 + lane) * J + j;
    if (inlier) inlier[e] = fit ? (unsigned char)((bmask >> lane) & 1ull) : (unsigned char)0;
    if (resid) {
      double depth;
      const float r = (float)sqrt(dlt_reproj2(Ms + lane * 12, X, uvj[(size_t)lane * J * 2], uvj[(size_t)lane * J * 2 + 1], &depth));
      resid[e] = fabsf(r) < INFINITY ? r : qnan;
    }
  }
}

// B * J <= INT_MAX and J <= 4096: the entry point refuses more (the grid's second dimension is ceil(J / 4)).
extern "C" hipError_t poem_launch_dlt_robust(const float* uv, const float* intr, const float* mat, const int* offs, float* out,
                                             unsigned char* inlier, int* count, float* resid, int B, int J, int invert,
                                             double inlier_px, int refine, hipStream_t s) {
  if (J > 4096) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dlt_robust_kernel, dim3(B, (J + 3) / 4), dim3(256), 0, s, uv, intr, mat, offs, out, inlier, count, resid, J,
                     invert, inlier_px * inlier_px, refine);
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
