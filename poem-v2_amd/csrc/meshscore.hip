// Benchmark-protocol mesh scores on the device: the pieces behind F@5 / F@15 and the Procrustes-aligned AUC of the FreiHAND /
// HO3D protocols (their evaluation scripts loop over samples on the host through open3d; the reference tree has no code of
// these).  Two kernels: the aligned point set of PAEval.align_w_scale written out, and the brute-force nearest-neighbour
// distance between two point sets in both directions, with threshold counts and distance sums per (sample, direction).
#include "common.h"
#include "procrustes.h"

// ---- the aligned set ------------------------------------------------------------------------------------------------------------
// pa_solve is pa_epe_kernel's solve (procrustes.h); aligned = fp32 rounding of the fp64 point pa_epe_kernel measures.
// transform (B,13) fp64 = c, R (row-major), t with aligned = c R p + t:  c = scale s1 / s2,  t = mean_gt - c R mean_pred.
// One wave per sample, four samples per block.
__global__ __launch_bounds__(256) void pa_align_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       float* __restrict__ aligned, double* __restrict__ transform, int B, int P) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* p = pred + (size_t)b * P * 3;
  const float* g = gt + (size_t)b * P * 3;
  PaSolve o;
  pa_solve(p, g, P, lane, o);
  if (aligned) {
    float* a = aligned + (size_t)b * P * 3;
    for (int i = lane; i < P; i += 64) {
      double al[3];
      pa_aligned_point(o, p, i, al);
      for (int d = 0; d < 3; ++d) a[i * 3 + d] = (float)al[d];
    }
  }
  if (transform && lane < 13) {
    const double c = o.scale * o.s1 / o.s2;
    double v;
    if (lane == 0) v = c;
    else if (lane < 10) v = o.R[(lane - 1) / 3][(lane - 1) % 3];
    else {
      const int d = lane - 10;
      v = o.mg[d] - c * (o.R[d][0] * o.mp[0] + o.R[d][1] * o.mp[1] + o.R[d][2] * o.mp[2]);
    }
    transform[(size_t)b * 13 + lane] = v;
  }
}

extern "C" hipError_t poem_launch_pa_align(const float* pred, const float* gt, float* aligned, double* transform, int B, int P,
                                           hipStream_t s) {
  hipLaunchKernelGGL(pa_align_kernel, dim3((B + 3) / 4), dim3(256), 0, s, pred, gt, aligned, transform, B, P);
  return hipGetLastError();
}

// ---- nearest-neighbour distances, both directions -------------------------------------------------------------------------------
// Direction 0: every point of a against the set b (dist_ab); direction 1: every point of b against a (dist_ba).
// One block per (sample, direction, chunk of NN_QUERIES query points), one query point per thread; the target set passes
// through LDS NN_TARGETS points at a time, so any na, nb works.
//   square   fp32, numpy's order ((dx*dx + dy*dy) + dz*dz), every operation rounded on its own (contraction off, as
//            pck_accumulate_kernel pins it)
//   minimum  over the fp32 squares (exact, so the order of the targets does not matter)
//   root     once per query point, of the minimum, through fp64 -- the correctly rounded fp32 root (metrics.hip)
//   count    (double)d < thr_t, STRICT, as the FreiHAND / HO3D scripts compare (_PCKMetric's <= stays what it is)
// NaN rule: a point with a NaN coordinate is nearest to nothing and nothing is nearest to it.  Its square against every
// point is NaN, and the running minimum is fminf, which keeps the other operand: so it never lowers another point's
// minimum, its own minimum stays the NaN the minimum starts from (NaN in dist_*, counted under no threshold, carried by
// sums), and a direction whose target set is all NaN gives NaN distances and zero counts.
// Counts and sums in a fixed order: one value per lane, a wave butterfly, the block's four waves in order into the
// block's slot of the workspace; nn_finalize_kernel then adds a (sample, direction)'s slots, lane-strided and by the
// same butterfly.  No atomics; a sample's slots and their order depend on na, nb alone, never on the batch.
#define NN_QUERIES 256
#define NN_TARGETS 1024
#define NN_MAX_THR 8

struct NNThresholds { double v[NN_MAX_THR]; };

__device__ inline int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(NN_QUERIES) void nn_distance_kernel(const float* __restrict__ a, int na, const float* __restrict__ b,
                                                                 int nb, float* __restrict__ dist_ab, float* __restrict__ dist_ba,
                                                                 NNThresholds thr, int nthr, double* __restrict__ slot_sum,
                                                                 int* __restrict__ slot_cnt, int reduce) {
  __shared__ float4 tgt[NN_TARGETS];
  __shared__ double wsum[NN_QUERIES / 64];
  __shared__ int wcnt[NN_QUERIES / 64][NN_MAX_THR];
  const int ca = (na + NN_QUERIES - 1) / NN_QUERIES, cb = (nb + NN_QUERIES - 1) / NN_QUERIES;
  const int s = blockIdx.x / (ca + cb), r = blockIdx.x % (ca + cb);
  const int dir = r >= ca ? 1 : 0, chunk = dir ? r - ca : r;
  float* dist = dir ? dist_ba : dist_ab;
  if (!dist && !reduce) return;                                    // nothing of this direction is asked for
  const int nq = dir ? nb : na, nt = dir ? na : nb;
  const float* q = (dir ? b : a) + (size_t)s * nq * 3;
  const float* t = (dir ? a : b) + (size_t)s * nt * 3;
  const int i = chunk * NN_QUERIES + threadIdx.x;
  const bool live = i < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) { qx = q[(size_t)i * 3]; qy = q[(size_t)i * 3 + 1]; qz = q[(size_t)i * 3 + 2]; }
  float m = __builtin_nanf("");
  for (int t0 = 0; t0 < nt; t0 += NN_TARGETS) {
    const int n = min(NN_TARGETS, nt - t0);
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += NN_QUERIES) {
      const float* tp = t + (size_t)(t0 + j) * 3;
      tgt[j] = make_float4(tp[0], tp[1], tp[2], 0.f);
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const float4 p = tgt[j];
      float d2;
      {
#pragma clang fp contract(off)
        const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        d2 = (xx + yy) + zz;
      }
      m = fminf(m, d2);
    }
  }
  const float d = (float)sqrt((double)m);
  if (live && dist) dist[(size_t)s * nq + i] = d;
  if (!reduce) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double dsum = wave_sum(live ? (double)d : 0.0);
  if (lane == 0) wsum[wave] = dsum;
  for (int k = 0; k < nthr; ++k) {
    const int c = wave_sum_i(live && (double)d < thr.v[k] ? 1 : 0);
    if (lane == 0) wcnt[wave][k] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) slot_sum[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  if (threadIdx.x < nthr)
    slot_cnt[(size_t)blockIdx.x * nthr + threadIdx.x] = ((wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x]) + wcnt[2][threadIdx.x]) + wcnt[3][threadIdx.x];
}

// One wave per (sample, direction): the slots of its query chunks, lane-strided in order, then the butterfly.
__global__ __launch_bounds__(64) void nn_finalize_kernel(const double* __restrict__ slot_sum, const int* __restrict__ slot_cnt, int na,
                                                         int nb, int nthr, int* __restrict__ counts, double* __restrict__ sums) {
  const int ca = (na + NN_QUERIES - 1) / NN_QUERIES, cb = (nb + NN_QUERIES - 1) / NN_QUERIES;
  const int s = blockIdx.x >> 1, dir = blockIdx.x & 1, lane = threadIdx.x;
  const size_t first = (size_t)s * (ca + cb) + (dir ? ca : 0);
  const int n = dir ? cb : ca;
  if (sums) {
    double acc = 0;
    for (int c = lane; c < n; c += 64) acc += slot_sum[first + c];
    acc = wave_sum(acc);
    if (lane == 0) sums[blockIdx.x] = acc;
  }
  if (counts)
    for (int k = 0; k < nthr; ++k) {
      int acc = 0;
      for (int c = lane; c < n; c += 64) acc += slot_cnt[(first + c) * nthr + k];
      acc = wave_sum_i(acc);
      if (lane == 0) counts[(size_t)blockIdx.x * nthr + k] = acc;
    }
}

// slots: one double and nthr ints per block of nn_distance_kernel -- the doubles first
extern "C" size_t poem_nn_distance_slots(int B, int na, int nb) {
  return (size_t)B * ((size_t)((na + NN_QUERIES - 1) / NN_QUERIES) + (size_t)((nb + NN_QUERIES - 1) / NN_QUERIES));
}

extern "C" hipError_t poem_launch_nn_distance(const float* a, int na, const float* b, int nb, float* dist_ab, float* dist_ba,
                                              const double* thr, int nthr, int* counts, double* sums, void* workspace, int B,
                                              hipStream_t s) {
  NNThresholds t{};
  for (int k = 0; k < nthr && k < NN_MAX_THR; ++k) t.v[k] = thr[k];
  const size_t slots = poem_nn_distance_slots(B, na, nb);
  const int reduce = (counts || sums) ? 1 : 0;
  double* slot_sum = (double*)workspace;
  int* slot_cnt = reduce ? (int*)(slot_sum + slots) : nullptr;
  hipLaunchKernelGGL(nn_distance_kernel, dim3((unsigned)slots), dim3(NN_QUERIES), 0, s, a, na, b, nb, dist_ab, dist_ba, t,
                     counts ? nthr : 0, slot_sum, slot_cnt, reduce);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !reduce) return e;
  hipLaunchKernelGGL(nn_finalize_kernel, dim3((unsigned)B * 2), dim3(64), 0, s, slot_sum, slot_cnt, na, nb, counts ? nthr : 0, counts,
                     sums);
  return hipGetLastError();
}
