// The training losses of the reference, evaluated on the device (forward only): every term of
// PtEmbedMultiviewStereoV2.compute_loss (lib/models/POEM.py:363-466 upstream) with loss_proj_to_multicam (:336-361) for a ragged
// batch in ONE launch plus a one-block finalize.  Upstream loops over samples in Python (two batched matmuls and a torch.linalg.inv
// per sample) and LossMetric.feed calls .item() per key (lib/metrics/basic_metric.py:74-88); here nothing returns to the host.
//
// Numeric rules (DESIGN.md section 7 "L"): the inputs are fp32, EVERY arithmetic step is fp64 -- the 4x4 inverse, the projection, the
// clamp and the squares included.  The reduction has one fixed order: per-thread partial -> xor butterfly inside the wave -> waves
// 0..3 -> one block partial in the workspace -> loss_finalize_kernel adds the block partials strided by thread, then the same tree.
// No floating-point atomics, so two runs give the same bits.  A NaN propagates as in torch: torch.clamp keeps it, v_min / v_max would
// not, so the clamp and the |z| < 1e-7 rule are compare + select (common.h relu_nan has the history).
// Disabled terms (a zero 2-D weight; pose / shape without PARAMETRIC_OUTPUT) are not computed and come out as 0.
//
// Blocks [0, BN * groups): one block group per view, one thread per (view, point) over the 21 joints + 778 vertices; the view's
// inv(extr) (common.h invert4x4, kept in fp64) and K are set up once per block.  groups = 1 when the vertices are not projected.
// Blocks [BN * groups, + B): one per sample -- the 3-D terms, the 16 x 778 joint regression of mano_to_openpose on the predicted and
// the ground-truth vertices (written for this kernel in fp64; the tables are metrics.hip's: mano_tables.h) and pose / shape.
#include "common.h"
#include "launchers.h"
#include "mano_tables.h"

namespace {

constexpr int LT = 256;
constexpr int NJ = 21, NV = 778, NQ = NJ + NV;

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide sums of v[0..N); the result is valid in thread 0
template <int N>
__device__ inline void block_sum(double (&v)[N], double (*red)[N]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum64(v[k]);
  if (lane == 0)
    for (int k = 0; k < N; ++k) red[wave][k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 0; k < N; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// torch.nn.MSELoss / L1Loss element (the mean is taken at the end)
__device__ __forceinline__ double crit(double d, int l2) { return l2 ? d * d : fabs(d); }

// torch.clamp(v, lo, hi): a NaN stays a NaN (every comparison with it is false)
__device__ __forceinline__ double clamp_nan(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// largest b with offs[b] <= v: the sample that owns view v
__device__ __forceinline__ int sample_of_view(const int* __restrict__ offs, int B, int v) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offs[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// batch_cam_extr_transf then batch_cam_intr_projection (lib/utils/transform.py:898-930): R p + t, the full 3x3 K, z = eps where |z| < eps
__device__ __forceinline__ void project(const double* T, const double* K, const float* __restrict__ p, double& u, double& w) {
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  const double cx = (T[0] * x + T[1] * y + T[2] * z) + T[3];
  const double cy = (T[4] * x + T[5] * y + T[6] * z) + T[7];
  const double cz = (T[8] * x + T[9] * y + T[10] * z) + T[11];
  const double hx = K[0] * cx + K[1] * cy + K[2] * cz;
  const double hy = K[3] * cx + K[4] * cy + K[5] * cz;
  double hz = K[6] * cx + K[7] * cy + K[8] * cz;
  if (fabs(hz) < 1e-7) hz = 1e-7;                      // (false for a NaN: it stays)
  u = hx / hz, w = hy / hz;
}

// sum over the two image axes of (clamp(a - b, -s/2, s/2) / s)^2          (loss_proj_to_multicam, POEM.py:357-359)
__device__ __forceinline__ double offset_sq(double au, double aw, double bu, double bw, double scale) {
  const double du = clamp_nan(au - bu, -0.5 * scale, 0.5 * scale) / scale;
  const double dw = clamp_nan(aw - bw, -0.5 * scale, 0.5 * scale) / scale;
  return du * du + dw * dw;
}

__device__ void view_block(const LossArgs& a, int vb) {
  __shared__ double T[16], K[9];
  __shared__ double red[4][LOSS_VIEW_SLOTS];
  const int t = threadIdx.x;
  const int v = vb / a.view_groups, g = vb % a.view_groups;
  const bool joints_2d = a.w_joints_2d != 0.0, verts_2d = a.view_groups > 1;
  if (joints_2d || verts_2d) {
    if (t == 0) invert4x4(a.extr + (size_t)v * 16, T);
    if (t >= 64 && t < 73) K[t - 64] = (double)a.intr[(size_t)v * 9 + (t - 64)];
  }
  __syncthreads();
  const int b = sample_of_view(a.view_offsets, a.B, v);
  const int p = g * LT + t;
  const double scale = a.img_scale;
  double acc[LOSS_VIEW_SLOTS] = {0.0, 0.0, 0.0};
  if (p < NJ) {
    const float* pu = a.pred_uv + ((size_t)v * NJ + p) * 2;
    const float* gu = a.gt_uv + ((size_t)v * NJ + p) * 2;
    const double du = ((double)pu[0] - (double)gu[0]) / scale, dw = ((double)pu[1] - (double)gu[1]) / scale;      // POEM.py:377-378
    acc[0] = du * du + dw * dw;
    if (joints_2d) {
      double u, w;
      project(T, K, a.coords + ((size_t)b * NQ + p) * 3, u, w);
      acc[1] = offset_sq(u, w, (double)gu[0], (double)gu[1], scale);
    }
  } else if (p < NQ && verts_2d) {
    double u, w, gu, gw;
    project(T, K, a.coords + ((size_t)b * NQ + p) * 3, u, w);
    project(T, K, a.gt_verts + ((size_t)b * NV + (p - NJ)) * 3, gu, gw);      // gt_verts_2d_ncams, POEM.py:389-400
    acc[2] = offset_sq(u, w, gu, gw, scale);
  }
  block_sum(acc, red);
  if (t == 0)
    for (int k = 0; k < LOSS_VIEW_SLOTS; ++k) a.part[(size_t)vb * LOSS_VIEW_SLOTS + k] = acc[k];
}

__device__ void sample_block(const LossArgs& a, int b) {
  __shared__ double jm[2][NJ][3];                       // [predicted | ground truth] MANO-ordered joints: 16 regressed + 5 tips
  __shared__ double red[4][LOSS_SAMPLE_SLOTS];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* pj = a.coords + (size_t)b * NQ * 3;
  const float* pv = pj + NJ * 3;
  const float* gj = a.gt_joints + (size_t)b * NJ * 3;
  const float* gv = a.gt_verts + (size_t)b * NV * 3;
  // mano_to_openpose: J_regressor (16,778) . verts for both meshes -- 32 dot products of 778 x 3, eight per wave
  for (int task = wave; task < 32; task += 4) {
    const int m = task >> 1, which = task & 1;
    const float* src = which ? gv : pv;
    const float* wr = a.jreg + (size_t)m * NV;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = lane; i < NV; i += 64) {
      const double wi = (double)wr[i];
      s0 += wi * (double)src[i * 3], s1 += wi * (double)src[i * 3 + 1], s2 += wi * (double)src[i * 3 + 2];
    }
    s0 = wave_sum64(s0), s1 = wave_sum64(s1), s2 = wave_sum64(s2);
    if (lane == 0) jm[which][m][0] = s0, jm[which][m][1] = s1, jm[which][m][2] = s2;
  }
  if (t < 30) {
    const int which = t / 15, tip = (t % 15) / 3, c = t % 3;
    jm[which][16 + tip][c] = (double)(which ? gv : pv)[kTipVertex[tip] * 3 + c];
  }
  __syncthreads();
  double acc[LOSS_SAMPLE_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < NJ * 3) {
    const int o = t / 3, c = t % 3, src = kOpenposeFromMano[o];
    acc[0] = crit((double)pj[t] - (double)gj[t], a.joints_l2);                                   // POEM.py:404
    acc[1] = crit(jm[0][src][c] - jm[1][src][c], a.joints_l2);                                   // POEM.py:403
  }
  for (int i = t; i < NV * 3; i += LT) {
    double d;
    if (a.parametric) {                                 // (pred - c) - (gt - c), c = the GROUND-TRUTH centre joint (POEM.py:413-416)
      const double c = (double)gj[a.center_idx * 3 + i % 3];
      d = ((double)pv[i] - c) - ((double)gv[i] - c);
    } else {
      d = (double)pv[i] - (double)gv[i];
    }
    acc[2] += crit(d, a.verts_l2);
  }
  if (a.parametric) {                                   // the master view's row of mano_pose / mano_shape (POEM.py:439-444)
    const int master = min(max(a.view_offsets[b], 0), a.BN - 1);
    if (t < 48) {
      const double d = (double)a.pred_pose[(size_t)b * 48 + t] - (double)a.mano_pose[(size_t)master * 48 + t];
      acc[3] = d * d;
    } else if (t >= 64 && t < 74) {
      const double d = (double)a.pred_shape[(size_t)b * 10 + (t - 64)] - (double)a.mano_shape[(size_t)master * 10 + (t - 64)];
      acc[4] = d * d;
    }
  }
  block_sum(acc, red);
  if (t == 0) {
    double* sp = a.part + (size_t)a.BN * a.view_groups * LOSS_VIEW_SLOTS + (size_t)b * LOSS_SAMPLE_SLOTS;
    for (int k = 0; k < LOSS_SAMPLE_SLOTS; ++k) sp[k] = acc[k];
  }
}

}  // namespace

__global__ void __launch_bounds__(256) loss_terms_kernel(const LossArgs a) {
  const int nvb = a.BN * a.view_groups;
  if ((int)blockIdx.x < nvb) view_block(a, (int)blockIdx.x);
  else sample_block(a, (int)blockIdx.x - nvb);
}

// one block: the block partials in a fixed order, then the means and the weighted sums in upstream's order of operations
__global__ void __launch_bounds__(256) loss_finalize_kernel(const LossArgs a) {
  __shared__ double red[4][LOSS_VIEW_SLOTS + LOSS_SAMPLE_SLOTS];
  const int t = threadIdx.x;
  const size_t nvb = (size_t)a.BN * a.view_groups;
  const double* sp = a.part + nvb * LOSS_VIEW_SLOTS;
  double acc[LOSS_VIEW_SLOTS + LOSS_SAMPLE_SLOTS] = {};
  for (size_t i = t; i < nvb; i += LT)
    for (int k = 0; k < LOSS_VIEW_SLOTS; ++k) acc[k] += a.part[i * LOSS_VIEW_SLOTS + k];
  for (int i = t; i < a.B; i += LT)
    for (int k = 0; k < LOSS_SAMPLE_SLOTS; ++k) acc[LOSS_VIEW_SLOTS + k] += sp[(size_t)i * LOSS_SAMPLE_SLOTS + k];
  block_sum(acc, red);
  if (t != 0) return;
  const double B = (double)a.B, BN = (double)a.BN;
  double* o = a.out;
  o[LOSS_HEATMAP] = acc[0] / (BN * NJ);
  o[LOSS_J2D] = a.w_joints_2d != 0.0 ? acc[1] / (BN * NJ) : 0.0;
  o[LOSS_V2D] = a.view_groups > 1 ? acc[2] / (BN * NV) : 0.0;
  o[LOSS_J3D] = acc[3] / (B * NJ * 3);
  o[LOSS_MESH] = acc[4] / (B * NJ * 3);
  o[LOSS_V3D] = acc[5] / (B * NV * 3);
  o[LOSS_POSE] = a.parametric ? acc[6] / (B * 48) : 0.0;
  o[LOSS_SHAPE] = a.parametric ? acc[7] / (B * 10) : 0.0;
  double recon = a.w_joints * (o[LOSS_J3D] + o[LOSS_MESH]);                    // POEM.py:405
  recon += a.w_verts * o[LOSS_V3D];                                            // :419
  recon += a.w_joints_2d * o[LOSS_J2D];                                        // :427
  recon += a.w_verts_2d * o[LOSS_V2D];                                         // :435
  recon += a.w_pose * o[LOSS_POSE] + a.w_shape * o[LOSS_SHAPE];                // :448
  o[LOSS_RECON] = recon;
  o[LOSS_TOTAL] = a.w_heatmap * o[LOSS_HEATMAP] + recon;                       // :381,455
}

extern "C" hipError_t poem_launch_loss_terms(const LossArgs* a, hipStream_t s) {
  const unsigned blocks = (unsigned)a->BN * (unsigned)a->view_groups + (unsigned)a->B;
  hipLaunchKernelGGL(loss_terms_kernel, dim3(blocks), dim3(LT), 0, s, *a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(LT), 0, s, *a);
  return hipGetLastError();
}
