// Row H2 of the scope table: what the ResNet-18/34/50 backbones (lib/models/backbones/resnet.py upstream) and the non-HRNet
// decode branch (lib/models/POEM.py:168-181,205-206) need besides the 3x3 convolutions of decode.hip and the 1x1 of hrnet.hip --
//   conv7x7_s2_kernel  the stem: relu(conv7x7(pad 3, stride 2) * scale + shift) of a plain (views, 3, H, W) image as an implicit
//                      GEMM on the fp32 matrix cores, K = 3 * 49 = 147 zero-padded to 152 (19 chunks of 8)
//   maxpool3x3_s2_kernel  nn.MaxPool2d(3, 2, 1), map in, map out, torch's bits (NaN propagates, padding is -inf)
//   sconv1x1_kernel    a 1x1 convolution whose operand is gathered from a map twice the output's size: POOL = 0 reads
//                      in(2y, 2x) (the stride-2 shortcut of a stage's first block), POOL = 1 reads max_pool2d(2, 2)
//                      (feat_in / uv_out of the non-HRNet decode branch; optional sigmoid)
// (poem_launch_upcat_pad_staged, the branch's [bilinear x2 of a | b] with a zero border, is upcat_pad_kernel<true> of decode.hip.)
// Both matrix kernels split the launch into wave items and walk their tiles' channels as conv.h has it: lane = pixel (32
// raster-consecutive output pixels of one view), the packed weights are the A operand in fragment order (common.h), a wave owns CT
// channel tiles of one pixel tile, waves are independent (no LDS, no barriers), and the k order is fixed -- chunk after chunk, k-step t of chunk cc multiplies
// k = 8cc + t (lower half-wave) and 8cc + 4 + t (upper) -- so a result is bit-reproducible and does not depend on the other
// views of the launch.
#include "conv.h"

#define STEM_K 147     // 3 * 7 * 7, k = (ci * 7 + ky) * 7 + kx
#define STEM_KC 19     // chunks of 8: 152 = STEM_K zero-padded

__global__ void pack_conv7x7_kernel(const float* __restrict__ w, int Cout, float4* __restrict__ out, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int lane = i & 63, f = i >> 6;
  const int cc = f % STEM_KC, cot = f / STEM_KC;
  const int co = cot * 32 + (lane & 31), k0 = 8 * cc + 4 * (lane >> 5);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (co < Cout && k0 + e < STEM_K) ? w[(size_t)co * STEM_K + k0 + e] : 0.f;
  out[i] = make_float4(v[0], v[1], v[2], v[3]);
}

extern "C" size_t poem_conv7x7_packed_floats(int Cout) { return (size_t)((Cout + 31) / 32) * STEM_KC * 64 * 4; }

extern "C" hipError_t poem_launch_pack_conv7x7(const float* w, int Cout, void* out, hipStream_t s) {
  const int total = ((Cout + 31) / 32) * STEM_KC * 64;
  hipLaunchKernelGGL(pack_conv7x7_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w, Cout, (float4*)out, total);
  return hipGetLastError();
}

template <int CT>
__global__ __launch_bounds__(256) void conv7x7_s2_kernel(StemArgs A) {
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int Ho = A.H / 2, Wo = A.W / 2;
  ConvItem it;
  if (!conv_item(A.views, (A.Cout / 32) / CT, Ho * Wo / 32, it)) return;
  const int n = it.n, cg = it.cg;
  const int pix = it.pg * 32 + j, oy = pix / Wo, ox = pix % Wo;
  const int iy0 = 2 * oy - 3, ix0 = 2 * ox - 3;
  const float* __restrict__ xin = A.in + (size_t)n * 3 * A.H * A.W;
  const float4* __restrict__ wp = A.wp + (size_t)(cg * CT) * STEM_KC * 64 + lane;
  f32x16 acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = zero16();
#pragma unroll
  for (int cc = 0; cc < STEM_KC; ++cc) {
    float4 a[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) a[c] = wp[(c * STEM_KC + cc) * 64];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      // the tap of this k-step: both half-waves' (ci, ky, kx) are compile-time constants, the lane picks its own
      const int k0 = 8 * cc + t, k1 = k0 + 4;
      const int ci = h ? k1 / 49 : k0 / 49;
      const int ky = h ? (k1 % 49) / 7 : (k0 % 49) / 7;
      const int kx = h ? k1 % 7 : k0 % 7;
      const bool live = h ? k1 < STEM_K : k0 < STEM_K;
      const int iy = iy0 + ky, ix = ix0 + kx;
      // a padding tap (or a k of the zero padding) is a zero operand, never a read outside the image
      float b = 0.f;
      if (live && (unsigned)iy < (unsigned)A.H && (unsigned)ix < (unsigned)A.W) b = xin[(ci * A.H + iy) * A.W + ix];
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = mfma32((&a[c].x)[t], b, acc[c]);
    }
  }
  float* __restrict__ op = A.out + A.omap.at(n, 0, oy, ox);
  tile32_channels<CT>(cg * CT, h, A.Cout, no_group, [&](int co, int c, int r, int) {
    op[(size_t)co * A.omap.cs] = relu_nan(acc[c][r] * A.scale[co] + A.shift[co]);
  });
}

extern "C" hipError_t poem_launch_conv7x7_s2(const StemArgs* args, hipStream_t s) {
  const StemArgs& a = *args;
  if (a.H % 2 || a.W % 2 || ((a.H / 2) * (a.W / 2)) % 32 || a.Cout % 32) return hipErrorInvalidValue;
  if ((size_t)3 * a.H * a.W * 4 >= (1ull << 31)) return hipErrorInvalidValue;
  const int cot = a.Cout / 32, ptiles = (a.H / 2) * (a.W / 2) / 32;
  const int ct = cot % 2 == 0 ? 2 : 1;
  const long items = (long)a.views * (cot / ct) * ptiles;
  if ((items + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid = conv_item_grid(items), block(256);
  if (ct == 2) hipLaunchKernelGGL((conv7x7_s2_kernel<2>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv7x7_s2_kernel<1>), grid, block, 0, s, a);
  return hipGetLastError();
}

// ---- nn.MaxPool2d(3, 2, 1) ----------------------------------------------------------------------------------------------------
// torch's rule (aten/src/ATen/native/cpu/MaxPoolKernel.cpp): start at -inf, scan the window in (ky, kx) order and take `val` when
// val > max || isnan(val) -- a NaN stays, of equal values (+-0 included) the first one met stays
__device__ __forceinline__ void pool_take(float& m, float v) {
  if (v > m || v != v) m = v;
}

__global__ __launch_bounds__(256) void maxpool3x3_s2_kernel(PoolArgs A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int Ho = A.H / 2, Wo = A.W / 2;
  if (i >= (long)A.views * A.C * Ho * Wo) return;
  const int x = (int)(i % Wo);
  long r = i / Wo;
  const int y = (int)(r % Ho);
  r /= Ho;
  const int c = (int)(r % A.C);
  const long n = r / A.C;
  const float* __restrict__ p = A.in + A.imap.at(n, c, 0, 0);
  float m = -INFINITY;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * y - 1 + ky;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * x - 1 + kx;
      if ((unsigned)iy < (unsigned)A.H && (unsigned)ix < (unsigned)A.W) pool_take(m, p[(size_t)iy * A.imap.rs + ix]);
    }
  }
  A.out[A.omap.at(n, c, y, x)] = m;
}

extern "C" hipError_t poem_launch_maxpool3x3_s2(const PoolArgs* a, hipStream_t s) {
  if (a->H % 2 || a->W % 2) return hipErrorInvalidValue;
  const long blocks = ((long)a->views * a->C * (a->H / 2) * (a->W / 2) + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(maxpool3x3_s2_kernel, dim3((unsigned)blocks), dim3(256), 0, s, *a);
  return hipGetLastError();
}

// ---- 1x1 convolution of a strided pick / a 2x2 max-pool ------------------------------------------------------------------------
template <int CT, int POOL>
__global__ __launch_bounds__(256) void sconv1x1_kernel(SConvArgs A) {
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int Ho = A.H / 2, Wo = A.W / 2;
  ConvItem it;
  if (!conv_item(A.views, ((A.Cout + 31) / 32) / CT, Ho * Wo / 32, it)) return;
  const int n = it.n, cg = it.cg;
  const int pix = it.pg * 32 + j, oy = pix / Wo, ox = pix % Wo;
  const int KC = A.Cin / 8;
  // channel 4h at the top-left input pixel of the lane's output pixel
  const float* __restrict__ xp = A.in + A.imap.at(n, 4 * h, 2 * oy, 2 * ox);
  const float4* __restrict__ wp = A.wp + (size_t)(cg * CT) * KC * 64 + lane;
  f32x16 acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = zero16();
  for (int cc = 0; cc < KC; ++cc) {
    float4 a[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) a[c] = wp[((size_t)c * KC + cc) * 64];
    float b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float* __restrict__ p = xp + (size_t)(8 * cc + t) * A.imap.cs;
      if (POOL) {
        float m = -INFINITY;
        pool_take(m, p[0]);
        pool_take(m, p[1]);
        pool_take(m, p[A.imap.rs]);
        pool_take(m, p[A.imap.rs + 1]);
        b[t] = m;
      } else {
        b[t] = p[0];
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = mfma32((&a[c].x)[t], b[t], acc[c]);
  }
  float* __restrict__ op = A.out + A.omap.at(n, 0, oy, ox);
  tile32_channels<CT>(cg * CT, h, A.Cout, no_group, [&](int co, int c, int r, int) {
    float v = acc[c][r] + (A.shift ? A.shift[co] : 0.f);
    if (A.act == 1) v = 1.0f / (1.0f + expf(-v));
    op[(size_t)co * A.omap.cs] = v;
  });
}

extern "C" hipError_t poem_launch_sconv1x1(const SConvArgs* args, hipStream_t s) {
  const SConvArgs& a = *args;
  if (a.Cin % 8 || a.H % 2 || a.W % 2 || ((a.H / 2) * (a.W / 2)) % 32) return hipErrorInvalidValue;
  const int cot = (a.Cout + 31) / 32, ptiles = (a.H / 2) * (a.W / 2) / 32;
  const int ct = (cot % 4 == 0) ? 4 : (cot % 2 == 0) ? 2 : 1;
  const long items = (long)a.views * (cot / ct) * ptiles;
  if ((items + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid = conv_item_grid(items), block(256);
#define POEM_SCONV(CTV)                                                                        \
  {                                                                                            \
    if (a.pool) hipLaunchKernelGGL((sconv1x1_kernel<CTV, 1>), grid, block, 0, s, a);             \
    else hipLaunchKernelGGL((sconv1x1_kernel<CTV, 0>), grid, block, 0, s, a);                  \
  }
  switch (ct) {
    case 4: POEM_SCONV(4) break;
    case 2: POEM_SCONV(2) break;
    default: POEM_SCONV(1) break;
  }
#undef POEM_SCONV
  return hipGetLastError();
}
