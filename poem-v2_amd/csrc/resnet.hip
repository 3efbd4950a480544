// Row H2 of the scope table: what the ResNet-18/34/50 backbones (lib/models/backbones/resnet.py upstream) and the non-HRNet
// decode branch (lib/models/POEM.py:168-181,205-206) need besides the 3x3 convolutions of decode.hip and the 1x1 of hrnet.hip --
//   conv7x7_s2_kernel  the stem: relu(conv7x7(pad 3, stride 2) * scale + shift) of a plain (views, 3, H, W) image as an implicit
//                      GEMM on the fp32 matrix cores, K = 3 * 49 = 147 zero-padded to 152 (19 chunks of 8)
//   maxpool3x3_s2_kernel  nn.MaxPool2d(3, 2, 1), map in, map out, torch's bits (NaN propagates, padding is -inf)
//   upcat_pad_staged_kernel  [bilinear x2 of a | b] with a zero border, rounded as poem_upcat_conv3x3 rounds it while staging
//   sconv1x1_kernel    a 1x1 convolution whose operand is gathered from a map twice the output's size: POOL = 0 reads
//                      in(2y, 2x) (the stride-2 shortcut of a stage's first block), POOL = 1 reads max_pool2d(2, 2)
//                      (feat_in / uv_out of the non-HRNet decode branch; optional sigmoid)
// All three matrix kernels follow conv1x1_nchw_kernel of hrnet.hip: lane = pixel (32 raster-consecutive output pixels of one
// view), the packed weights are the A operand in fragment order (common.h), a wave owns CT channel tiles of one pixel tile,
// waves are independent (no LDS, no barriers), and the k order is fixed -- chunk after chunk, k-step t of chunk cc multiplies
// k = 8cc + t (lower half-wave) and 8cc + 4 + t (upper) -- so a result is bit-reproducible and does not depend on the other
// views of the launch.
#include "common.h"

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

struct StemArgs {
  const float* in;       // (views, 3, H, W) plain
  const float4* wp;
  const float* scale;
  const float* shift;
  float* out;            // map (views, Cout, H/2, W/2)
  long out_ns;
  int out_cs, out_rs, out_off;
  int Cout, H, W, views;
};

template <int CT>
__global__ __launch_bounds__(256) void conv7x7_s2_kernel(StemArgs A) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int Ho = A.H / 2, Wo = A.W / 2;
  const int ptiles = Ho * Wo / 32, cogroups = (A.Cout / 32) / CT;
  const long item = (long)blockIdx.x * 4 + wv;
  if (item >= (long)A.views * cogroups * ptiles) return;
  const int pt = (int)(item % ptiles);
  const int cg = (int)((item / ptiles) % cogroups);
  const int n = (int)(item / ((long)ptiles * cogroups));
  const int pix = pt * 32 + j, oy = pix / Wo, ox = pix % Wo;
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
  // epilogue: lane = pixel, register e of group g = channel 8g + 4h + e of the tile
  float* __restrict__ op = A.out + (size_t)n * A.out_ns + (size_t)oy * A.out_rs + ox + A.out_off;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int cbase = (cg * CT + c) * 32 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = cbase + 8 * g + e;
        op[(size_t)co * A.out_cs] = relu_nan(acc[c][4 * g + e] * A.scale[co] + A.shift[co]);
      }
    }
  }
}

// H, W even, (H/2 * W/2) % 32 == 0, Cout % 32 == 0, a view of the input below 2 GiB
extern "C" hipError_t poem_launch_conv7x7_s2(const float* in, const void* wp, const float* scale, const float* shift, float* out,
                                             long out_ns, int out_cs, int out_rs, int out_off, int views, int Cout, int H, int W,
                                             hipStream_t s) {
  if (H % 2 || W % 2 || ((H / 2) * (W / 2)) % 32 || Cout % 32) return hipErrorInvalidValue;
  if ((size_t)3 * H * W * 4 >= (1ull << 31)) return hipErrorInvalidValue;
  StemArgs a{in, (const float4*)wp, scale, shift, out, out_ns, out_cs, out_rs, out_off, Cout, H, W, views};
  const int cot = Cout / 32, ptiles = (H / 2) * (W / 2) / 32;
  const int ct = cot % 2 == 0 ? 2 : 1;
  const long items = (long)views * (cot / ct) * ptiles;
  if ((items + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((items + 3) / 4)), block(256);
  if (ct == 2) hipLaunchKernelGGL((conv7x7_s2_kernel<2>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv7x7_s2_kernel<1>), grid, block, 0, s, a);
  return hipGetLastError();
}

// ---- nn.MaxPool2d(3, 2, 1) ----------------------------------------------------------------------------------------------------
struct PoolArgs {
  const float* in;
  float* out;
  long in_ns, out_ns;
  int in_cs, in_rs, in_off, out_cs, out_rs, out_off;
  int C, H, W;           // of the input; the output is (H/2, W/2)
  long total;
};

// torch's rule (aten/src/ATen/native/cpu/MaxPoolKernel.cpp): start at -inf, scan the window in (ky, kx) order and take `val` when
// val > max || isnan(val) -- a NaN stays, of equal values (+-0 included) the first one met stays
__device__ __forceinline__ void pool_take(float& m, float v) {
  if (v > m || v != v) m = v;
}

__global__ __launch_bounds__(256) void maxpool3x3_s2_kernel(PoolArgs A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.total) return;
  const int Ho = A.H / 2, Wo = A.W / 2;
  const int x = (int)(i % Wo);
  long r = i / Wo;
  const int y = (int)(r % Ho);
  r /= Ho;
  const int c = (int)(r % A.C);
  const long n = r / A.C;
  const float* __restrict__ p = A.in + (size_t)n * A.in_ns + (size_t)c * A.in_cs + A.in_off;
  float m = -INFINITY;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * y - 1 + ky;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * x - 1 + kx;
      if ((unsigned)iy < (unsigned)A.H && (unsigned)ix < (unsigned)A.W) pool_take(m, p[(size_t)iy * A.in_rs + ix]);
    }
  }
  A.out[(size_t)n * A.out_ns + (size_t)c * A.out_cs + (size_t)y * A.out_rs + x + A.out_off] = m;
}

extern "C" hipError_t poem_launch_maxpool3x3_s2(const float* in, long in_ns, int in_cs, int in_rs, int in_off, float* out, long out_ns,
                                                int out_cs, int out_rs, int out_off, int views, int C, int H, int W, hipStream_t s) {
  if (H % 2 || W % 2) return hipErrorInvalidValue;
  PoolArgs a{in, out, in_ns, out_ns, in_cs, in_rs, in_off, out_cs, out_rs, out_off, C, H, W, (long)views * C * (H / 2) * (W / 2)};
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(maxpool3x3_s2_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---- [bilinear x2 of a | b] with a zero border, in the fused convolution's arithmetic ------------------------------------------
// upcat_pad_kernel of decode.hip with the interpolation evaluated as Conv3Stager evaluates it while poem_upcat_conv3x3 stages its
// input: the four tap weights multiplied out, then one multiply and three fmas.  (upcat_pad_kernel nests the two directions as
// torch does, which rounds differently in the last place.)  poem_conv3x3 of this tensor runs the same matrix instructions on the
// same operands as poem_upcat_conv3x3: the two routes of the non-HRNet decode branch give the same bits.
__global__ void upcat_pad_staged_kernel(const float* __restrict__ a, int Ca, const float* __restrict__ b, int Cb,
                                        float* __restrict__ out, int H, int W, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int Wp = W + 2, Hp = H + 2, C = Ca + Cb;
  const int xp = (int)(i % Wp);
  long t = i / Wp;
  const int yp = (int)(t % Hp);
  t /= Hp;
  const int c = (int)(t % C);
  const long n = t / C;
  const int x = xp - 1, y = yp - 1;
  float v = 0.f;
  if (x >= 0 && x < W && y >= 0 && y < H) {
    if (c < Ca) {
      const int h2 = H / 2, w2 = W / 2;
      const float sy = fmaxf((y + 0.5f) * 0.5f - 0.5f, 0.f), sx = fmaxf((x + 0.5f) * 0.5f - 0.5f, 0.f);
      const int y0 = (int)sy, x0 = (int)sx;
      const int y1 = min(y0 + 1, h2 - 1), x1 = min(x0 + 1, w2 - 1);
      const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
      const float q0 = hy * hx, q1 = hy * lx, q2 = ly * hx, q3 = ly * lx;
      const float* p = a + ((size_t)n * Ca + c) * h2 * w2;
      v = fmaf(q3, p[y1 * w2 + x1], fmaf(q2, p[y1 * w2 + x0], fmaf(q1, p[y0 * w2 + x1], q0 * p[y0 * w2 + x0])));
    } else {
      v = b[(((size_t)n * Cb + (c - Ca)) * H + y) * W + x];
    }
  }
  out[i] = v;
}

extern "C" hipError_t poem_launch_upcat_pad_staged(const float* a, int Ca, const float* b, int Cb, float* out, int views, int H, int W,
                                                   hipStream_t s) {
  if ((Ca && (H % 2 || W % 2)) || Ca + Cb <= 0) return hipErrorInvalidValue;
  const long total = (long)views * (Ca + Cb) * (H + 2) * (W + 2);
  if ((total + 255) / 256 > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(upcat_pad_staged_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, Ca, b, Cb, out, H, W, total);
  return hipGetLastError();
}

// ---- 1x1 convolution of a strided pick / a 2x2 max-pool ------------------------------------------------------------------------
struct SConvArgs {
  const float* in;       // map (views, Cin, 2 Ho, 2 Wo)
  const float4* wp;      // poem_pack_conv1x1 image
  const float* shift;    // (Cout) or null
  float* out;            // map (views, Cout, Ho, Wo)
  long in_ns, out_ns;
  int in_cs, in_rs, in_off, out_cs, out_rs, out_off;
  int Cin, Cout, Ho, Wo, act, views;      // act: 0 none, 1 sigmoid
};

template <int CT, int POOL>
__global__ __launch_bounds__(256) void sconv1x1_kernel(SConvArgs A) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int ptiles = A.Ho * A.Wo / 32, cogroups = ((A.Cout + 31) / 32) / CT;
  const long item = (long)blockIdx.x * 4 + wv;
  if (item >= (long)A.views * cogroups * ptiles) return;
  const int pt = (int)(item % ptiles);
  const int cg = (int)((item / ptiles) % cogroups);
  const int n = (int)(item / ((long)ptiles * cogroups));
  const int pix = pt * 32 + j, oy = pix / A.Wo, ox = pix % A.Wo;
  const int KC = A.Cin / 8;
  // channel 4h at the top-left input pixel of the lane's output pixel
  const float* __restrict__ xp = A.in + (size_t)n * A.in_ns + (size_t)(4 * h) * A.in_cs + (size_t)(2 * oy) * A.in_rs + 2 * ox + A.in_off;
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
      const float* __restrict__ p = xp + (size_t)(8 * cc + t) * A.in_cs;
      if (POOL) {
        float m = -INFINITY;
        pool_take(m, p[0]);
        pool_take(m, p[1]);
        pool_take(m, p[A.in_rs]);
        pool_take(m, p[A.in_rs + 1]);
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
  float* __restrict__ op = A.out + (size_t)n * A.out_ns + (size_t)oy * A.out_rs + ox + A.out_off;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int cbase = (cg * CT + c) * 32 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = cbase + 8 * g + e;
        if (co >= A.Cout) continue;
        float v = acc[c][4 * g + e] + (A.shift ? A.shift[co] : 0.f);
        if (A.act == 1) v = 1.0f / (1.0f + expf(-v));
        op[(size_t)co * A.out_cs] = v;
      }
    }
  }
}

// H, W (of the input) even, (H/2 * W/2) % 32 == 0, Cin % 8 == 0
extern "C" hipError_t poem_launch_sconv1x1(const float* in, long in_ns, int in_cs, int in_rs, int in_off, const void* wp,
                                           const float* shift, float* out, long out_ns, int out_cs, int out_rs, int out_off, int views,
                                           int Cin, int Cout, int H, int W, int pool, int act, hipStream_t s) {
  if (Cin % 8 || H % 2 || W % 2 || ((H / 2) * (W / 2)) % 32) return hipErrorInvalidValue;
  SConvArgs a{in, (const float4*)wp, shift, out, in_ns, out_ns, in_cs, in_rs, in_off, out_cs, out_rs, out_off,
              Cin, Cout, H / 2, W / 2, act, views};
  const int cot = (Cout + 31) / 32, ptiles = (H / 2) * (W / 2) / 32;
  const int ct = (cot % 4 == 0) ? 4 : (cot % 2 == 0) ? 2 : 1;
  const long items = (long)views * (cot / ct) * ptiles;
  if ((items + 3) / 4 > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((items + 3) / 4)), block(256);
#define POEM_SCONV(CTV)                                                                        \
  {                                                                                            \
    if (pool) hipLaunchKernelGGL((sconv1x1_kernel<CTV, 1>), grid, block, 0, s, a);             \
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
