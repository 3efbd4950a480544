// Fit MANO pose, shape and translation to a mesh (include/poem_hip.h poem_mano_fit): Levenberg-Marquardt on
//   x = (pose_aa[48], betas[10], tsl[3]),  r = V(x) - target,  V = the uncentred MANO mesh of csrc/mano.hip's header + tsl,
// with the smooth exponential map for Rodrigues (no +1e-8; series below |aa| = 1e-2, so that a joint at exactly zero has the three
// generators as its derivative).  fp32 inputs, every step fp64, no floating-point atomics (loss.hip's rule).
//
// `mano_fit_init_kernel` (B blocks of one wave) flags non-finite input and forms the start: the caller's x0, or the rotation of
// procrustes.h's alignment of the template onto the target, through the quaternion with its largest component first.
// `mano_fit_eval_kernel` (grid 49 vertex tiles of 16 x B, 256 threads) evaluates [J | r] for its 16 vertices into LDS (48 rows x 62
// columns) and writes the lower triangle of [J | r]^T [J | r] -- H, g and the cost: 1891 + 61 + 1 sums, each over the 48 rows in
// order -- into its slot of the workspace.  Its prologue repeats per block what depends on the sample only: the 16 rotations and
// their 48 derivatives, J(betas), the kinematic chain, and dA_j / dx_p for the parameters that move joint j: its own three and its
// ancestors' (46 (joint, chain depth) slots of three 3x4 matrices) and the betas (which move translations only: 10 x 16 x 3).
// `mano_fit_step_kernel` (B blocks) adds the 49 slots in order, accepts or rejects the candidate, solves (H + mu D) dx = -g by
// Cholesky in LDS and writes the next candidate.  The same eval kernel in its OUT form writes the fp32 results.
// Fixed trip counts everywhere: 2 * iters + 4 launches, no host synchronisation, no block waits for another.
//
// poem_mano_fit_terms adds 3-D joint targets and 2-D keypoints in calibrated views: `mano_fit_joint_kernel` (B blocks) runs next to
// the eval kernel at every evaluation, on the same prologue (`fit_prologue`), and writes one more slot per sample; the step kernel
// adds mesh_weight x (the 49 slots) and that slot.  poem_mano_fit is the case "mesh alone, weight 1" of the same launches.  The
// trip count of the view loops comes from the device's view offsets (uniform per block): 3 * iters + 5 launches with both.
#include "../../include/poem_hip.h"   // poem_mano_fit_terms_t, POEM_FIT_ZMIN
#include "common.h"
#include "mano_layout.h"
#include "procrustes.h"

namespace {
constexpr int NX = 61, NE = 62;                  // unknowns; columns of [J | r]
constexpr int NSUM = NE * (NE + 1) / 2;          // 1953 = 1891 (H) + 61 (g) + 1 (cost)
constexpr int TV = 16, NT = (NV + TV - 1) / TV;  // 49 vertex tiles
constexpr int ROWS = 3 * TV;
constexpr int NSLOT = 46;                        // (joint, chain depth <= its own) pairs of the 16-joint tree
// per-sample state in the workspace (doubles)
constexpr int ST_X = 0, ST_XC = 64, ST_G = 128, ST_C = 192, ST_MU = 193, ST_ACC = 194, ST_STATUS = 195, ST_FIRST = 196;
constexpr int ST_H = 200, ST_DOUBLES = ST_H + NX * NX + 7;     // 3928
constexpr int HS = 62;                           // row stride of the step kernel's matrix in LDS

__device__ __forceinline__ int joint_depth(int j) { return j == 0 ? 0 : 1 + (j - 1) % 3; }
// first slot of joint j; its ancestor-or-self at chain depth d (0 = root) is slot joint_slot(j) + d
__device__ __forceinline__ int joint_slot(int j) {
  if (j == 0) return 0;
  const int l = (j - 1) % 3;
  return 1 + 9 * ((j - 1) / 3) + (l == 0 ? 0 : l == 1 ? 2 : 5);
}
// (p, q), p >= q, of entry e of a packed lower triangle
__device__ __forceinline__ void tri_decode(int e, int& p, int& q) {
  p = (int)((sqrtf(8.f * (float)e + 1.f) - 1.f) * 0.5f);
  if (p * (p + 1) / 2 > e) --p;
  if ((p + 1) * (p + 2) / 2 <= e) ++p;
  q = e - p * (p + 1) / 2;
}

// R = exp([w]x) and its three partial derivatives, row-major
__device__ void rodrigues_d(const double* w, double* R, double* dR) {
  const double s = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double a, b, da, db;      // sin t / t, (1 - cos t) / t^2, and their derivatives by w_i divided by w_i
  if (s < 1e-4) {
    a = 1.0 + s * (-1.0 / 6 + s * (1.0 / 120 - s / 5040));
    b = 0.5 + s * (-1.0 / 24 + s * (1.0 / 720 - s / 40320));
    da = -1.0 / 3 + s * (1.0 / 30 + s * (-1.0 / 840 + s / 45360));
    db = -1.0 / 12 + s * (1.0 / 180 + s * (-1.0 / 6720 + s / 453600));
  } else {
    const double t = sqrt(s), sn = sin(t), cs = cos(t), h = sin(0.5 * t);
    a = sn / t;
    b = 2.0 * h * h / s;
    da = (t * cs - sn) / (s * t);
    db = (t * sn - 4.0 * h * h) / (s * s);
  }
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double K2[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K2[r * 3 + c] = w[r] * w[c] - (r == c ? s : 0.0);
  for (int e = 0; e < 9; ++e) R[e] = (e % 4 == 0 ? 1.0 : 0.0) + a * K[e] + b * K2[e];
  for (int i = 0; i < 3; ++i) {
    double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i == 0) { E[5] = -1; E[7] = 1; } else if (i == 1) { E[2] = 1; E[6] = -1; } else { E[1] = -1; E[3] = 1; }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const double dK2 = (r == i ? w[c] : 0.0) + (c == i ? w[r] : 0.0) - (r == c ? 2.0 * w[i] : 0.0);
        dR[i * 9 + r * 3 + c] = a * E[r * 3 + c] + da * w[i] * K[r * 3 + c] + b * dK2 + db * w[i] * K2[r * 3 + c];
      }
  }
}

// G = P . [R | t]   (3x4, row-major)
__device__ __forceinline__ void chain_d(const double* P, const double* R, const double* t, double* G) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) G[r * 4 + c] = P[r * 4 + 0] * R[c] + P[r * 4 + 1] * R[3 + c] + P[r * 4 + 2] * R[6 + c];
    G[r * 4 + 3] = P[r * 4 + 0] * t[0] + P[r * 4 + 1] * t[1] + P[r * 4 + 2] * t[2] + P[r * 4 + 3];
  }
}

__device__ __forceinline__ float table_d(const float* __restrict__ table, int k, int c, int v) {      // blend-shape basis k of (c, v)
  return table[OFF_D + (((size_t)(k >> 2) * 3 + c) * VP + v) * 4 + (k & 3)];
}

// the data terms of poem_mano_fit_terms_t as the kernels take them (a null pointer: the term is absent)
struct FitTerms {
  const float *target, *joints3d, *joints3d_weight, *keypoints, *keypoint_weight, *cam_intr, *cam_extr;
  const int32_t* view_offsets;
  int total_views;
  double mesh_weight, image_scale, zmin;
};
// sample b's views [n0, n1), kept inside [0, total_views] whatever the offsets hold
__device__ __forceinline__ int view_begin(const FitTerms& tm, int b) { return min(max(tm.view_offsets[b], 0), tm.total_views); }
__device__ __forceinline__ int view_end(const FitTerms& tm, int b, int n0) { return min(max(tm.view_offsets[b + 1], n0), tm.total_views); }
}  // namespace

// ---- the start ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mano_fit_init_kernel(const float* __restrict__ table, const FitTerms tm,
                                                           const float* __restrict__ x0, double* __restrict__ ws) {
  __shared__ float tp[NV * 3];
  const int b = blockIdx.x, lane = threadIdx.x;
  double* st = ws + (size_t)b * ST_DOUBLES;
  const float* tg = tm.target ? tm.target + (size_t)b * NV * 3 : nullptr;
  const float* j3 = tm.joints3d ? tm.joints3d + (size_t)b * 63 : nullptr;
  int bad_t = 0, bad_x = 0;
  if (tg) for (int i = lane; i < NV * 3; i += 64) bad_t |= !isfinite(tg[i]);
  int j3_partial = 0;                         // a joint target that cannot enter the rigid start
  if (j3 && lane < 21) {
    const float w = tm.joints3d_weight[(size_t)b * 21 + lane];
    bad_t |= !(w >= 0.f) || isinf(w);         // (negative, NaN or infinite)
    const bool fin = isfinite(j3[lane * 3]) && isfinite(j3[lane * 3 + 1]) && isfinite(j3[lane * 3 + 2]);
    if (w > 0.f) bad_t |= !fin;
    j3_partial = !(w > 0.f) || !fin;
  }
  if (tm.keypoints) {                         // the sample's views, one after the other; a view without a positive weight is not read
    const int n0 = view_begin(tm, b), n1 = view_end(tm, b, n0);
    for (int n = n0; n < n1; ++n) {
      float w = 0.f;
      if (lane < 21) {
        w = tm.keypoint_weight[(size_t)n * 21 + lane];
        bad_t |= !(w >= 0.f) || isinf(w);
        if (w > 0.f) bad_t |= !isfinite(tm.keypoints[((size_t)n * 21 + lane) * 2]) || !isfinite(tm.keypoints[((size_t)n * 21 + lane) * 2 + 1]);
      }
      if (__any(w > 0.f)) {
        if (lane < 9) bad_t |= !isfinite(tm.cam_intr[(size_t)n * 9 + lane]);
        if (lane >= 16 && lane < 32) bad_t |= !isfinite(tm.cam_extr[(size_t)n * 16 + lane - 16]);
      }
    }
  }
  bad_t = __any(bad_t);
  j3_partial = __any(j3_partial);
  double start = 0.0;                         // lane i < 61 holds x_i
  if (x0) {
    if (lane < NX) start = (double)x0[(size_t)b * NX + lane];
    bad_x = __any(!isfinite(start));
  } else if (!tg && (!j3 || j3_partial)) {
    bad_x = 1;                                // no rigid start without a mesh or from joints that are not all there
  } else if (!bad_t) {
    // the rigid rule on the mesh, or (without one) on the 21 zero-pose joints in kOrder against joints3d
    const int np = tg ? NV : 21;
    if (tg) {
      for (int i = lane; i < NV * 3; i += 64) tp[i] = table[OFF_VT + (i % 3) * VP + i / 3];
    } else if (lane < 63) {
      const int src = kOrder[lane / 3], c = lane % 3;
      tp[lane] = src < NJ ? table[OFF_JT + src * 3 + c] : table[OFF_VT + c * VP + kTips[src - NJ]];
    }
    __syncthreads();
    PaSolve o;
    pa_solve(tp, tg ? tg : j3, np, lane, o);
    const double(*R)[3] = o.R;
    const double q2[4] = {1 + R[0][0] + R[1][1] + R[2][2], 1 + R[0][0] - R[1][1] - R[2][2], 1 - R[0][0] + R[1][1] - R[2][2],
                          1 - R[0][0] - R[1][1] + R[2][2]};
    int m = 0;
    for (int i = 1; i < 4; ++i) if (q2[i] > q2[m]) m = i;
    const double h = 0.5 * sqrt(fmax(q2[m], 0.0)), f = 0.25 / h;
    double q[4];                              // w, x, y, z
    if (m == 0) { q[0] = h; q[1] = (R[2][1] - R[1][2]) * f; q[2] = (R[0][2] - R[2][0]) * f; q[3] = (R[1][0] - R[0][1]) * f; }
    else if (m == 1) { q[1] = h; q[0] = (R[2][1] - R[1][2]) * f; q[2] = (R[0][1] + R[1][0]) * f; q[3] = (R[0][2] + R[2][0]) * f; }
    else if (m == 2) { q[2] = h; q[0] = (R[0][2] - R[2][0]) * f; q[1] = (R[0][1] + R[1][0]) * f; q[3] = (R[1][2] + R[2][1]) * f; }
    else { q[3] = h; q[0] = (R[1][0] - R[0][1]) * f; q[1] = (R[0][2] + R[2][0]) * f; q[2] = (R[1][2] + R[2][1]) * f; }
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), sg = q[0] < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 4; ++i) q[i] *= sg / qn;
    const double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double k = n > 1e-12 ? 2.0 * atan2(n, q[0]) / n : 2.0;
    // tsl: the centroid of the target minus the centroid of the rotated template (the root rotation turns about joint 0)
    double tsl[3];
    for (int d = 0; d < 3; ++d) {
      double rot = 0;
      for (int c = 0; c < 3; ++c) rot += R[d][c] * (o.mp[c] - (double)table[OFF_JT + c]);
      tsl[d] = o.mg[d] - rot - (double)table[OFF_JT + d];
    }
    if (lane < 3) start = k * q[1 + lane];
    if (lane >= 58 && lane < NX) start = tsl[lane - 58];
    bad_x = __any(!isfinite(start));
  }
  if (lane < NX) { st[ST_X + lane] = start; st[ST_XC + lane] = start; }
  if (lane == 0) {
    st[ST_C] = __longlong_as_double(0x7ff8000000000000ll);
    st[ST_MU] = 1e-3;
    st[ST_ACC] = 0.0;
    st[ST_STATUS] = (double)((bad_t ? 1 : 0) | (bad_x ? 2 : 0));
    st[ST_FIRST] = 1.0;
  }
}

// ---- what depends on the sample only, for the eval kernel and the joint-term kernel alike ---------------------------------------
// The per-sample tables, in the LDS of the kernel that calls `fit_prologue` (a block of 256 threads):
struct FitTables {
  double *xs, *R, *dR, *Jj, *G, *A, *coef;      // [64], [NJ * 9], [NJ * 27], [NJ * 3], [NJ * 12], [NJ * 12], [K4 * 4]
  double* dAb;                                   // [NBETA * NJ * 3]  d A_j^t / d beta_k (the rotation part is 0)
  double* dAp;                                   // [NSLOT * 3 * 12]  d A_j / d pose of the chain joint at depth d, axis a: [(slot(j) + d) * 3 + a][12]
};
constexpr int FIT_TABLE_DOUBLES = 64 + NJ * (9 + 27 + 3 + 12 + 12) + K4 * 4 + NBETA * NJ * 3 + NSLOT * 3 * 12;      // 3356

// x (the accepted point in the OUT form, the candidate otherwise) -> rotations, J(betas), the chain G, A; without OUT also the
// derivatives dR, dAp, dAb.  xs .. coef are complete for every thread when it returns; A, dAp and dAb after the caller's next
// __syncthreads().
template <bool OUT>
__device__ __forceinline__ void fit_prologue(const float* __restrict__ table, const double* st, int t, const FitTables& s) {
  double *const xs = s.xs, *const R = s.R, *const dR = s.dR, *const Jj = s.Jj, *const G = s.G, *const A = s.A, *const coef = s.coef;
  double *const dAb = s.dAb, *const dAp = s.dAp;
  if (t < 64) xs[t] = t < NX ? st[(OUT ? ST_X : ST_XC) + t] : 0.0;
  __syncthreads();
  if (t < NJ) rodrigues_d(xs + 3 * t, R + 9 * t, dR + 27 * t);
  if (t >= 64 && t < 64 + NJ * 3) {
    const int q = t - 64;
    double acc = (double)table[OFF_JT + q];
    for (int k = 0; k < NBETA; ++k) acc += (double)table[OFF_JSD + q * NBETA + k] * xs[48 + k];
    Jj[q] = acc;
  }
  if (t >= 128 && t < 128 + NBETA) coef[t - 128] = xs[48 + t - 128];
  if (t >= 138 && t < 141) coef[NBETA + NPOSE + t - 138] = 0.0;
  __syncthreads();
  if (t < NPOSE) coef[NBETA + t] = R[9 + t] - ((t % 9) % 4 == 0 ? 1.0 : 0.0);
  if (t >= 192 && t < 197) {                    // one thread per finger walks its three joints down from the root
    double par[12];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) par[r * 4 + c] = R[r * 3 + c];
      par[r * 4 + 3] = Jj[r];
    }
    if (t == 192) for (int e = 0; e < 12; ++e) G[e] = par[e];
    int pj = 0;
    for (int l = 0; l < 3; ++l) {
      const int j = 1 + 3 * (t - 192) + l;
      const double rel[3] = {Jj[j * 3] - Jj[pj * 3], Jj[j * 3 + 1] - Jj[pj * 3 + 1], Jj[j * 3 + 2] - Jj[pj * 3 + 2]};
      double g[12];
      chain_d(par, R + j * 9, rel, g);
      for (int e = 0; e < 12; ++e) { G[j * 12 + e] = g[e]; par[e] = g[e]; }
      pj = j;
    }
  }
  __syncthreads();
  if (t < NJ) {                                  // A_j = [G^R | G^t - G^R J_j]
    const double* g = G + t * 12;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) A[t * 12 + r * 4 + c] = g[r * 4 + c];
      A[t * 12 + r * 4 + 3] = g[r * 4 + 3] - (g[r * 4] * Jj[t * 3] + g[r * 4 + 1] * Jj[t * 3 + 1] + g[r * 4 + 2] * Jj[t * 3 + 2]);
    }
  }
  if (!OUT && t >= 64 && t < 64 + 48) {
    // pose parameter (i, a): dG_i = [G_parent(i)^R dR_i^a | 0], and down the subtree dG_j = dG_parent(j) . [R_j | t_j]
    const int p = t - 64, i = p / 3, a = p % 3, di = joint_depth(i);
    const int pi = i == 0 ? -1 : (di == 1 ? 0 : i - 1);
    double top[12];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        double acc = 0;
        for (int k = 0; k < 3; ++k) acc += (pi < 0 ? (r == k ? 1.0 : 0.0) : G[pi * 12 + r * 4 + k]) * dR[i * 27 + a * 9 + k * 3 + c];
        top[r * 4 + c] = acc;
      }
      top[r * 4 + 3] = 0.0;
    }
    const int nf = i == 0 ? 5 : 1;               // the root's subtree is all five fingers
    for (int f = 0; f <= nf; ++f) {
      // f == 0: joint i itself; f >= 1: the joints below it on finger (i == 0 ? f - 1 : its own)
      double cur[12];
      for (int e = 0; e < 12; ++e) cur[e] = top[e];
      int j = i, pj = i;
      const int steps = f == 0 ? 1 : (i == 0 ? 3 : 3 - di);
      for (int l = 0; l < steps; ++l) {
        if (f > 0) {
          j = i == 0 ? 1 + 3 * (f - 1) + l : i + 1 + l;
          const double rel[3] = {Jj[j * 3] - Jj[pj * 3], Jj[j * 3 + 1] - Jj[pj * 3 + 1], Jj[j * 3 + 2] - Jj[pj * 3 + 2]};
          double g[12];
          chain_d(cur, R + j * 9, rel, g);       // (dG_parent^t carries on as the translation of the product)
          for (int e = 0; e < 12; ++e) cur[e] = g[e];
          pj = j;
        }
        double* d = dAp + ((joint_slot(j) + di) * 3 + a) * 12;
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) d[r * 4 + c] = cur[r * 4 + c];
          d[r * 4 + 3] = cur[r * 4 + 3] - (cur[r * 4] * Jj[j * 3] + cur[r * 4 + 1] * Jj[j * 3 + 1] + cur[r * 4 + 2] * Jj[j * 3 + 2]);
        }
      }
    }
  }
  if (!OUT && t >= 128 && t < 128 + NBETA) {
    // beta k moves the joints only: dG_j^R = 0, dG_j^t = dG_parent^t + G_parent^R (dJ_j - dJ_parent), dA_j^t = dG_j^t - G_j^R dJ_j
    const int k = t - 128;
    double root[3] = {0, 0, 0}, prev[3] = {0, 0, 0};      // dG^t of joint 0 and of joint j - 1
    for (int j = 0; j < NJ; ++j) {
      const int pj = j == 0 ? -1 : (joint_depth(j) == 1 ? 0 : j - 1);
      double dJ[3], rel[3], cur[3];
      for (int c = 0; c < 3; ++c) {
        dJ[c] = (double)table[OFF_JSD + (j * 3 + c) * NBETA + k];
        rel[c] = dJ[c] - (pj < 0 ? 0.0 : (double)table[OFF_JSD + (pj * 3 + c) * NBETA + k]);
      }
      for (int r = 0; r < 3; ++r) {
        double v = pj < 0 ? rel[r] : (pj == 0 ? root[r] : prev[r]);
        if (pj >= 0) for (int c = 0; c < 3; ++c) v += G[pj * 12 + r * 4 + c] * rel[c];
        cur[r] = v;
      }
      for (int r = 0; r < 3; ++r) {
        dAb[(k * NJ + j) * 3 + r] = cur[r] - (G[j * 12 + r * 4] * dJ[0] + G[j * 12 + r * 4 + 1] * dJ[1] + G[j * 12 + r * 4 + 2] * dJ[2]);
        prev[r] = cur[r];
        if (j == 0) root[r] = cur[r];
      }
    }
  }
}

// column p of d V_v / dx (3 numbers) for vertex v: vp = its blended rest position, T = its skinning transform sum_j w_j A_j,
// w[j * wstride] = its skinning weights
__device__ __forceinline__ void vertex_column(const float* __restrict__ table, const FitTables& s, int p, int v, const double* vp,
                                              const double* T, const double* w_v, int wstride, double* col) {
  const double *const dR = s.dR, *const dAb = s.dAb, *const dAp = s.dAp;
  col[0] = col[1] = col[2] = 0.0;
  if (p < 48) {
    const int i = p / 3, a = p % 3, di = joint_depth(i);
    const int jb = i, je = i == 0 ? NJ - 1 : 3 * ((i - 1) / 3) + 3;
    for (int j = jb; j <= je; ++j) {
      const double w = w_v[j * wstride];
      const double* d = dAp + ((joint_slot(j) + di) * 3 + a) * 12;
      for (int r = 0; r < 3; ++r) col[r] += w * (d[r * 4] * vp[0] + d[r * 4 + 1] * vp[1] + d[r * 4 + 2] * vp[2] + d[r * 4 + 3]);
    }
    if (i >= 1) {                              // the pose-corrective blend shapes against d(R_i - I)
      double dv[3] = {0, 0, 0};
      for (int e = 0; e < 9; ++e) {
        const double dr = dR[i * 27 + a * 9 + e];
        for (int c = 0; c < 3; ++c) dv[c] += (double)table_d(table, NBETA + 9 * (i - 1) + e, c, v) * dr;
      }
      for (int r = 0; r < 3; ++r) col[r] += T[r * 4] * dv[0] + T[r * 4 + 1] * dv[1] + T[r * 4 + 2] * dv[2];
    }
  } else if (p < 58) {
    const int k = p - 48;
    for (int j = 0; j < NJ; ++j) {
      const double w = w_v[j * wstride];
      for (int r = 0; r < 3; ++r) col[r] += w * dAb[(k * NJ + j) * 3 + r];
    }
    double dv[3];
    for (int c = 0; c < 3; ++c) dv[c] = (double)table_d(table, k, c, v);
    for (int r = 0; r < 3; ++r) col[r] += T[r * 4] * dv[0] + T[r * 4 + 1] * dv[1] + T[r * 4 + 2] * dv[2];
  } else {
    for (int r = 0; r < 3; ++r) col[r] = r == p - 58 ? 1.0 : 0.0;
  }
}

// ---- cost, gradient and normal matrix at the candidate (OUT = false); the fp32 results at the accepted point (OUT = true) -----
// (One signature for both forms: the o_* pointers are read by the OUT form only, `target` by the other.  After a step whose
// Cholesky met a bad pivot the candidate is the accepted point itself (dx = 0) and the next launch evaluates it once more: the
// definition's "evaluate at x + dx", whose equal cost the strict comparison then rejects -- no special case, at the price of one
// repeated evaluation.)  `nslots`: NSUM slots per sample in the workspace (the 49 tiles', and one more where joint terms are fitted).
template <bool OUT>
__global__ __launch_bounds__(256) void mano_fit_eval_kernel(const float* __restrict__ table, const float* __restrict__ target,
                                                            double* __restrict__ ws, int B, int nslots, float* __restrict__ o_pose,
                                                            float* __restrict__ o_betas, float* __restrict__ o_tsl,
                                                            float* __restrict__ o_verts, float* __restrict__ o_joints,
                                                            double* __restrict__ o_cost, int32_t* __restrict__ o_acc,
                                                            int32_t* __restrict__ o_status) {
  __shared__ double xs[64], R[NJ * 9], dR[NJ * 27], Jj[NJ * 3], G[NJ * 12], A[NJ * 12], coef[K4 * 4];
  __shared__ double dAb[NBETA * NJ * 3];
  __shared__ double dAp[NSLOT * 3 * 12];
  __shared__ double part[16][3][TV], wl[NJ][TV];
  __shared__ double Jt[OUT ? 1 : ROWS * NE];
  const int b = blockIdx.y, t = threadIdx.x, lv = t & (TV - 1), pg = t >> 4;
  double* st = ws + (size_t)b * ST_DOUBLES;
  if (!OUT && st[ST_STATUS] != 0.0) return;     // a flagged sample keeps its start (the whole block leaves)
  const FitTables tabs = {xs, R, dR, Jj, G, A, coef, dAb, dAp};
  fit_prologue<OUT>(table, st, t, tabs);
  // ---- the tile's vertices: thread (vertex lv, group pg of 16); v < 49 * 16 <= VP, and the table's padded columns are zeros
  const int v = blockIdx.x * TV + lv;
  const bool live = v < NV;
  {
    const float4* D = reinterpret_cast<const float4*>(table + OFF_D);
    double acc[3] = {0, 0, 0};
    for (int k4 = pg; k4 < K4; k4 += 16)
      for (int c = 0; c < 3; ++c) {
        const float4 d = D[((size_t)k4 * 3 + c) * VP + v];
        acc[c] += (double)d.x * coef[4 * k4] + (double)d.y * coef[4 * k4 + 1] + (double)d.z * coef[4 * k4 + 2] + (double)d.w * coef[4 * k4 + 3];
      }
    for (int c = 0; c < 3; ++c) part[pg][c][lv] = acc[c];
    wl[pg][lv] = (double)table[OFF_W + pg * VP + v];
  }
  __syncthreads();                               // A, dAp, dAb, the partial blend sums and the weights are in place
  double vp[3], T[12], vo[3];
  for (int c = 0; c < 3; ++c) {
    double s = (double)table[OFF_VT + c * VP + v];
    for (int g = 0; g < 16; ++g) s += part[g][c][lv];
    vp[c] = s;
  }
  for (int e = 0; e < 12; ++e) T[e] = 0.0;
  for (int j = 0; j < NJ; ++j) {
    const double w = wl[j][lv];
    for (int e = 0; e < 12; ++e) T[e] += w * A[j * 12 + e];
  }
  for (int r = 0; r < 3; ++r) vo[r] = T[r * 4] * vp[0] + T[r * 4 + 1] * vp[1] + T[r * 4 + 2] * vp[2] + T[r * 4 + 3] + xs[58 + r];
  if (OUT) {
    if (pg < 3 && live) {
      o_verts[((size_t)b * NV + v) * 3 + pg] = (float)vo[pg];
      for (int f = 0; f < 5; ++f)
        if (v == kTips[f]) {
          int pos = 0;
          for (int q = 0; q < 21; ++q) if (kOrder[q] == NJ + f) pos = q;
          o_joints[(size_t)b * 63 + pos * 3 + pg] = (float)vo[pg];
        }
    }
    if (blockIdx.x == 0) {
      if (t < 63) {
        const int src = kOrder[t / 3], c = t % 3;
        if (src < NJ) o_joints[(size_t)b * 63 + t] = (float)(G[src * 12 + c * 4 + 3] + xs[58 + c]);
      }
      if (t < 48) o_pose[(size_t)b * 48 + t] = (float)xs[t];
      else if (t < 58) o_betas[(size_t)b * NBETA + t - 48] = (float)xs[t];
      else if (t < NX) o_tsl[(size_t)b * 3 + t - 58] = (float)xs[t];
      if (t == 64) {
        o_cost[b] = st[ST_C];
        o_acc[b] = (int32_t)st[ST_ACC];
        o_status[b] = (int32_t)st[ST_STATUS];
      }
    }
    return;
  }
  for (int p = pg; p < NX; p += 16) {
    double col[3];
    vertex_column(table, tabs, p, v, vp, T, &wl[0][lv], TV, col);
    for (int r = 0; r < 3; ++r) Jt[(lv * 3 + r) * NE + p] = live ? col[r] : 0.0;
  }
  if (pg == 15)
    for (int r = 0; r < 3; ++r)
      Jt[(lv * 3 + r) * NE + NX] = live ? vo[r] - (double)target[((size_t)b * NV + v) * 3 + r] : 0.0;
  __syncthreads();
  double* slot = ws + (size_t)B * ST_DOUBLES + ((size_t)b * nslots + blockIdx.x) * NSUM;
  for (int e = t; e < NSUM; e += 256) {
    int p, q;
    tri_decode(e, p, q);
    double acc = 0.0;
    for (int row = 0; row < ROWS; ++row) acc += Jt[row * NE + p] * Jt[row * NE + q];
    slot[e] = acc;
  }
}

// ---- terms J and K at the candidate: 3-D joint targets and 2-D keypoints in the sample's views ----------------------------------
// One block per sample.  After the prologue the block forms JP = [dP_q / dx | P_q] for the 21 points P_q of the `joints` output
// (63 rows x 62 columns in LDS): a chain joint from dG_j^t = dA_j^R J_j + dA_j^t (a beta: dAb + G_j^R dJ_j), a tip by the vertex
// code on its vertex.  No per-view Jacobian exists: thread q < 21 walks the sample's views in order and accumulates, for its joint,
//   W_q = sum_n M^T M (3x3, symmetric),  b_q = sum_n M^T r,  s_q = sum_n |r|^2,   M = sqrt(w) / scale . dpi/dp_cam . R_n  (2x3),
// term J adding w3 I, w3 (P - target) and w3 |P - target|^2 first.  Then H = sum_q JP_q^T W_q JP_q, g = sum_q JP_q^T b_q and
// c = sum_q s_q over q = 0..20 in order, each thread its strided share of the 1953 sums, into slot NT of the sample.
// A weight that is not positive skips its entry: nothing of it is read.  A positive-weight keypoint at camera depth <= zmin makes
// the cost +inf (the step kernel's rule rejects it); at the first evaluation it sets status bit 2 here instead.
// The cameras are inverted eight views at a time (threads 0..7, common.h invert4x4 in fp64).
constexpr int CAMV = 8;                          // views per chunk
constexpr int TIPF = 5;
__global__ __launch_bounds__(256) void mano_fit_joint_kernel(const float* __restrict__ table, const FitTerms tm, double* __restrict__ ws,
                                                             int B, int nslots) {
  __shared__ double tb[FIT_TABLE_DOUBLES];
  __shared__ double JP[63 * NE];
  __shared__ double tvp[TIPF][3], tw[TIPF][NJ], tT[TIPF][12];      // the five tip vertices: blended rest position, weights, transform
  __shared__ double cam[CAMV][21];               // inv(extr) rows 0..2 (12) | K (9)
  __shared__ double Wq[21][6], bq[21][3], sq[21];
  __shared__ int behind_s[21];
  const int b = blockIdx.x, t = threadIdx.x;
  double* st = ws + (size_t)b * ST_DOUBLES;
  if (st[ST_STATUS] != 0.0) return;              // a flagged sample keeps its start (the whole block leaves)
  const bool first = st[ST_FIRST] != 0.0;
  double* o = tb;
  FitTables s;
  s.xs = o; o += 64;
  s.R = o; o += NJ * 9;
  s.dR = o; o += NJ * 27;
  s.Jj = o; o += NJ * 3;
  s.G = o; o += NJ * 12;
  s.A = o; o += NJ * 12;
  s.coef = o; o += K4 * 4;
  s.dAb = o; o += NBETA * NJ * 3;
  s.dAp = o;
  fit_prologue<false>(table, st, t, s);
  if (t < TIPF * 3) {                            // the tips' blended rest positions (coef is complete)
    const int f = t / 3, c = t % 3, v = kTips[f];
    double acc = (double)table[OFF_VT + c * VP + v];
    for (int k = 0; k < K4 * 4; ++k) acc += (double)table_d(table, k, c, v) * s.coef[k];
    tvp[f][c] = acc;
  }
  if (t >= 64 && t < 64 + TIPF * NJ) tw[(t - 64) / NJ][(t - 64) % NJ] = (double)table[OFF_W + ((t - 64) % NJ) * VP + kTips[(t - 64) / NJ]];
  __syncthreads();                               // A, dAp, dAb, tvp, tw
  if (t < TIPF * 12) {
    const int f = t / 12, e = t % 12;
    double acc = 0.0;
    for (int j = 0; j < NJ; ++j) acc += tw[f][j] * s.A[j * 12 + e];
    tT[f][e] = acc;
  }
  __syncthreads();
  for (int task = t; task < 21 * NE; task += 256) {
    const int q = task / NE, p = task % NE, src = kOrder[q];
    double col[3] = {0.0, 0.0, 0.0};
    if (src < NJ) {
      const int j = src;
      if (p < 48) {
        const int i = p / 3, a = p % 3;
        if (i == 0 || (j >= 1 && (i - 1) / 3 == (j - 1) / 3 && i <= j)) {      // joint i is j or above it on the chain
          const double* d = s.dAp + ((joint_slot(j) + joint_depth(i)) * 3 + a) * 12;
          for (int r = 0; r < 3; ++r)
            col[r] = d[r * 4] * s.Jj[j * 3] + d[r * 4 + 1] * s.Jj[j * 3 + 1] + d[r * 4 + 2] * s.Jj[j * 3 + 2] + d[r * 4 + 3];
        }
      } else if (p < 58) {
        const int k = p - 48;
        double dJ[3];
        for (int c = 0; c < 3; ++c) dJ[c] = (double)table[OFF_JSD + (j * 3 + c) * NBETA + k];
        for (int r = 0; r < 3; ++r)
          col[r] = s.dAb[(k * NJ + j) * 3 + r] + (s.G[j * 12 + r * 4] * dJ[0] + s.G[j * 12 + r * 4 + 1] * dJ[1] + s.G[j * 12 + r * 4 + 2] * dJ[2]);
      } else if (p < NX) {
        col[p - 58] = 1.0;
      } else {
        for (int r = 0; r < 3; ++r) col[r] = s.G[j * 12 + r * 4 + 3] + s.xs[58 + r];
      }
    } else {
      const int f = src - NJ;
      if (p < NX) {
        vertex_column(table, s, p, kTips[f], tvp[f], tT[f], tw[f], 1, col);
      } else {
        const double *T = tT[f], *vp = tvp[f];
        for (int r = 0; r < 3; ++r) col[r] = T[r * 4] * vp[0] + T[r * 4 + 1] * vp[1] + T[r * 4 + 2] * vp[2] + T[r * 4 + 3] + s.xs[58 + r];
      }
    }
    for (int r = 0; r < 3; ++r) JP[(q * 3 + r) * NE + p] = col[r];
  }
  __syncthreads();
  // ---- per joint: W, b, s over term J and the views in order
  double W[6] = {0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0}, sacc = 0.0, P[3] = {0, 0, 0};
  int behind = 0;
  if (t < 21) {
    for (int r = 0; r < 3; ++r) P[r] = JP[(t * 3 + r) * NE + NX];
    if (tm.joints3d) {
      const float w3 = tm.joints3d_weight[(size_t)b * 21 + t];
      if (w3 > 0.f) {
        const double w = (double)w3;
        double d[3];
        for (int r = 0; r < 3; ++r) d[r] = P[r] - (double)tm.joints3d[((size_t)b * 21 + t) * 3 + r];
        W[0] += w; W[3] += w; W[5] += w;
        for (int r = 0; r < 3; ++r) bv[r] += w * d[r];
        sacc += w * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      }
    }
  }
  if (tm.keypoints) {
    const int n0 = view_begin(tm, b), n1 = view_end(tm, b, n0);      // (the same for every thread of the block)
    for (int c0 = n0; c0 < n1; c0 += CAMV) {
      __syncthreads();                           // the previous chunk's cameras have been read
      if (t < CAMV && c0 + t < n1) {
        bool used = false;                       // a view without a positive weight: its camera is not read
        for (int q = 0; q < 21; ++q) used |= tm.keypoint_weight[(size_t)(c0 + t) * 21 + q] > 0.f;
        if (used) {
          double Ti[16];
          invert4x4(tm.cam_extr + (size_t)(c0 + t) * 16, Ti);
          for (int e = 0; e < 12; ++e) cam[t][e] = Ti[e];
          for (int e = 0; e < 9; ++e) cam[t][12 + e] = (double)tm.cam_intr[(size_t)(c0 + t) * 9 + e];
        }
      }
      __syncthreads();
      if (t < 21) {
        const int ne = min(CAMV, n1 - c0);
        for (int l = 0; l < ne; ++l) {
          const size_t ent = (size_t)(c0 + l) * 21 + t;
          const float w2 = tm.keypoint_weight[ent];
          if (w2 > 0.f) {
            const double *T = cam[l], *K = cam[l] + 12;
            double pc[3], h[3];
            for (int r = 0; r < 3; ++r) pc[r] = (T[r * 4] * P[0] + T[r * 4 + 1] * P[1] + T[r * 4 + 2] * P[2]) + T[r * 4 + 3];
            for (int r = 0; r < 3; ++r) h[r] = K[r * 3] * pc[0] + K[r * 3 + 1] * pc[1] + K[r * 3 + 2] * pc[2];
            if (pc[2] <= tm.zmin) behind = 1;
            const double u = h[0] / h[2], v = h[1] / h[2], sw = sqrt((double)w2) / tm.image_scale;
            const double r0 = sw * (u - (double)tm.keypoints[ent * 2]), r1 = sw * (v - (double)tm.keypoints[ent * 2 + 1]);
            double a0[3], a1[3], M0[3], M1[3];   // d(u, v) / dp_cam, then through R_n
            for (int c = 0; c < 3; ++c) { a0[c] = (K[c] - u * K[6 + c]) / h[2]; a1[c] = (K[3 + c] - v * K[6 + c]) / h[2]; }
            for (int c = 0; c < 3; ++c) {
              M0[c] = sw * (a0[0] * T[c] + a0[1] * T[4 + c] + a0[2] * T[8 + c]);
              M1[c] = sw * (a1[0] * T[c] + a1[1] * T[4 + c] + a1[2] * T[8 + c]);
            }
            W[0] += M0[0] * M0[0] + M1[0] * M1[0]; W[1] += M0[0] * M0[1] + M1[0] * M1[1]; W[2] += M0[0] * M0[2] + M1[0] * M1[2];
            W[3] += M0[1] * M0[1] + M1[1] * M1[1]; W[4] += M0[1] * M0[2] + M1[1] * M1[2]; W[5] += M0[2] * M0[2] + M1[2] * M1[2];
            for (int c = 0; c < 3; ++c) bv[c] += M0[c] * r0 + M1[c] * r1;
            sacc += r0 * r0 + r1 * r1;
          }
        }
      }
    }
  }
  if (t < 21) {
    for (int e = 0; e < 6; ++e) Wq[t][e] = W[e];
    for (int e = 0; e < 3; ++e) bq[t][e] = bv[e];
    sq[t] = sacc;
    behind_s[t] = behind;
  }
  __syncthreads();
  int any_behind = 0;
  for (int q = 0; q < 21; ++q) any_behind |= behind_s[q];
  if (any_behind && first) {                     // the start lies behind a camera: flagged, the start stays
    if (t == 0) st[ST_STATUS] = 4.0;
    return;
  }
  double* slot = ws + (size_t)B * ST_DOUBLES + ((size_t)b * nslots + NT) * NSUM;
  for (int e = t; e < NSUM; e += 256) {
    int p, q;
    tri_decode(e, p, q);
    double acc = 0.0;
    if (p < NX) {
      for (int jq = 0; jq < 21; ++jq) {
        const double* Jr = JP + jq * 3 * NE;
        const double a0 = Jr[p], a1 = Jr[NE + p], a2 = Jr[2 * NE + p];
        const double* w = Wq[jq];
        const double t0 = a0 * w[0] + a1 * w[1] + a2 * w[2], t1 = a0 * w[1] + a1 * w[3] + a2 * w[4], t2 = a0 * w[2] + a1 * w[4] + a2 * w[5];
        acc += t0 * Jr[q] + t1 * Jr[NE + q] + t2 * Jr[2 * NE + q];
      }
    } else if (q < NX) {
      for (int jq = 0; jq < 21; ++jq) {
        const double* Jr = JP + jq * 3 * NE;
        acc += bq[jq][0] * Jr[q] + bq[jq][1] * Jr[NE + q] + bq[jq][2] * Jr[2 * NE + q];
      }
    } else {
      for (int jq = 0; jq < 21; ++jq) acc += sq[jq];
      if (any_behind) acc = __longlong_as_double(0x7ff0000000000000ll);
    }
    slot[e] = acc;
  }
}

// ---- add the slots, accept or reject, solve, next candidate --------------------------------------------------------------------
// `mesh`: the 49 tiles' slots hold term M, which enters as mesh_weight times their sum (times 1.0 is exact); `joint`: slot NT holds
// terms J and K.
__global__ __launch_bounds__(256) void mano_fit_step_kernel(double* __restrict__ ws, int B, int nslots, int mesh, double mesh_weight,
                                                            int joint, double shape_reg, double pose_reg, int last) {
  __shared__ double Hs[NX * HS], gs[64], xs[64], rhs[64], dg[64];
  __shared__ double cnew_s;
  const int b = blockIdx.x, t = threadIdx.x;
  double* st = ws + (size_t)b * ST_DOUBLES;
  const double status = st[ST_STATUS], first = st[ST_FIRST], cold = st[ST_C], mu_old = st[ST_MU], acc_old = st[ST_ACC];
  if (status != 0.0) return;
  const double* slots = ws + (size_t)B * ST_DOUBLES + (size_t)b * nslots * NSUM;
  for (int e = t; e < NSUM; e += 256) {
    double s = 0.0;
    if (mesh) {
      for (int tile = 0; tile < NT; ++tile) s += slots[(size_t)tile * NSUM + e];
      s *= mesh_weight;
    }
    if (joint) s += slots[(size_t)NT * NSUM + e];
    int p, q;
    tri_decode(e, p, q);
    if (p < NX) { Hs[p * HS + q] = s; Hs[q * HS + p] = s; }
    else if (q < NX) gs[q] = s;
    else cnew_s = s;
  }
  if (t < NX) xs[t] = st[ST_XC + t];
  __syncthreads();
  if (t < NX) {                                  // the regularisers' terms
    const double lam = t >= 58 ? 0.0 : t >= 48 ? shape_reg : t >= 3 ? pose_reg : 0.0;
    gs[t] += lam * xs[t];
    Hs[t * HS + t] += lam;
  }
  double cnew = cnew_s;
  for (int i = 3; i < 58; ++i) cnew += (i >= 48 ? shape_reg : pose_reg) * xs[i] * xs[i];
  __syncthreads();                               // (everybody has read cnew_s, xs)
  if (first != 0.0 && !isfinite(cnew)) {         // a start whose cost overflows: flagged, the start stays
    if (t == 0) st[ST_STATUS] = 2.0;
    return;
  }
  const bool accept = first != 0.0 || cnew < cold;      // (a NaN compares false)
  double mu = mu_old;
  if (first == 0.0) mu = accept ? fmax(mu_old / 10.0, 1e-9) : fmin(mu_old * 10.0, 1e8);
  if (accept) {
    if (t < NX) { st[ST_X + t] = xs[t]; st[ST_G + t] = gs[t]; }
    for (int e = t; e < NX * NX; e += 256) st[ST_H + e] = Hs[(e / NX) * HS + e % NX];
  } else {
    if (t < NX) { xs[t] = st[ST_X + t]; gs[t] = st[ST_G + t]; }
    for (int e = t; e < NX * NX; e += 256) Hs[(e / NX) * HS + e % NX] = st[ST_H + e];
  }
  if (t == 0) {
    if (accept) st[ST_C] = cnew;
    st[ST_MU] = mu;
    st[ST_ACC] = acc_old + ((accept && first == 0.0) ? 1.0 : 0.0);
    st[ST_FIRST] = 0.0;
  }
  if (last) return;
  __syncthreads();
  if (t < NX) { dg[t] = fmax(Hs[t * HS + t], 1e-12); rhs[t] = -gs[t]; }
  __syncthreads();
  if (t < NX) Hs[t * HS + t] += mu * dg[t];
  __syncthreads();
  // Cholesky, lower triangle in place.  A pivot that is not positive or not finite marks the step as rejected; the loops go on
  // with 1 in its place (fixed trip counts) and dx is dropped at the end.
  bool bad = false;
  for (int k = 0; k < NX; ++k) {
    double piv = Hs[k * HS + k];
    if (!(piv > 0.0) || !isfinite(piv)) { bad = true; piv = 1.0; }
    const double l = sqrt(piv);
    __syncthreads();
    if (t == k) Hs[k * HS + k] = l;
    if (t > k && t < NX) Hs[t * HS + k] /= l;
    __syncthreads();
    for (int i = k + 1 + (t >> 4); i < NX; i += 16)
      for (int j = k + 1 + (t & 15); j <= i; j += 16) Hs[i * HS + j] -= Hs[i * HS + k] * Hs[j * HS + k];
    __syncthreads();
  }
  for (int k = 0; k < NX; ++k) {                 // L y = -g
    if (t == k) rhs[k] /= Hs[k * HS + k];
    __syncthreads();
    if (t > k && t < NX) rhs[t] -= Hs[t * HS + k] * rhs[k];
    __syncthreads();
  }
  for (int k = NX - 1; k >= 0; --k) {            // L^T dx = y
    if (t == k) rhs[k] /= Hs[k * HS + k];
    __syncthreads();
    if (t < k) rhs[t] -= Hs[k * HS + t] * rhs[k];
    __syncthreads();
  }
  if (t < NX) st[ST_XC + t] = xs[t] + (bad ? 0.0 : rhs[t]);
}

extern "C" size_t poem_mano_fit_workspace_doubles_impl(int B) { return (size_t)B * ((size_t)ST_DOUBLES + (size_t)NT * NSUM); }
extern "C" size_t poem_mano_fit_terms_workspace_doubles_impl(int B) { return (size_t)B * ((size_t)ST_DOUBLES + (size_t)(NT + 1) * NSUM); }

// poem_mano_fit is the call with term M alone, weight 1 and `joint_slot` 0 (its documented workspace has the 49 tiles' slots only);
// poem_mano_fit_terms passes joint_slot 1.  Launches: 1 + (iters + 1) (M + JK + 1) + 1 with M, JK = 1 where the term's kernel runs.
extern "C" hipError_t poem_launch_mano_fit_terms(const float* table, const poem_mano_fit_terms_t* terms, int joint_slot, const float* x0,
                                                 int B, int iters, float shape_reg, float pose_reg, double* ws, float* pose, float* betas,
                                                 float* tsl, float* verts, float* joints, double* cost, int32_t* accepted, int32_t* status,
                                                 hipStream_t s) {
  FitTerms tm;
  tm.target = terms->target_verts;
  tm.joints3d = terms->joints3d;
  tm.joints3d_weight = terms->joints3d_weight;
  tm.keypoints = terms->keypoints;
  tm.keypoint_weight = terms->keypoint_weight;
  tm.cam_intr = terms->cam_intr;
  tm.cam_extr = terms->cam_extr;
  tm.view_offsets = terms->view_offsets;
  tm.total_views = terms->total_views;
  tm.mesh_weight = (double)terms->mesh_weight;
  tm.image_scale = (double)terms->image_scale;
  tm.zmin = POEM_FIT_ZMIN;
  const int mesh = tm.target != nullptr, joint = tm.joints3d != nullptr || tm.keypoints != nullptr;
  const int nslots = NT + (joint_slot ? 1 : 0);
  if (joint && !joint_slot) return hipErrorInvalidValue;
  const dim3 tiles(NT, B);
  hipLaunchKernelGGL(mano_fit_init_kernel, dim3(B), dim3(64), 0, s, table, tm, x0, ws);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  for (int it = 0; it <= iters; ++it) {
    if (mesh) {
      hipLaunchKernelGGL(mano_fit_eval_kernel<false>, tiles, dim3(256), 0, s, table, tm.target, ws, B, nslots, pose, betas, tsl, verts,
                         joints, cost, accepted, status);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    if (joint) {
      hipLaunchKernelGGL(mano_fit_joint_kernel, dim3(B), dim3(256), 0, s, table, tm, ws, B, nslots);
      if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mano_fit_step_kernel, dim3(B), dim3(256), 0, s, ws, B, nslots, mesh, tm.mesh_weight, joint, (double)shape_reg,
                       (double)pose_reg, it == iters ? 1 : 0);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(mano_fit_eval_kernel<true>, tiles, dim3(256), 0, s, table, tm.target, ws, B, nslots, pose, betas, tsl, verts, joints,
                     cost, accepted, status);
  return hipGetLastError();
}
