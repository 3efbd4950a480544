// Row H of the scope table: what the HRNet-W40 backbone (lib/models/backbones/hrnet.py upstream) needs besides the 3x3
// convolutions of decode.hip --
//   conv1x1_nchw_kernel 1x1 convolution on NCHW (the Bottleneck's 64 -> 64, 256 -> 64, 64 -> 256, downsample.0 and the up-going
//                      fuse layers): D[co][pixel] = sum_ci W[co][ci] * X[ci][pixel] per view on the fp32 matrix cores
//   hrnet_fuse_kernel  the fuse sum of a HighResolutionModule (hrnet.py:226-233): relu(((t0 + t1) + t2) + t3) with the
//                      nearest-neighbour upsampling of the lower-resolution terms applied while they are read
// conv1x1 is conv3x3_kernel of decode.hip without taps: lane = pixel (32 raster-consecutive pixels of a view), the packed
// weights are the A operand --
//   WP[(cot * Cin/8 + cc) * 64 + lane] = float4( W[32cot + (lane&31)][8cc + 4(lane>>5) + 0..3] )   (rows >= Cout zero)
// -- k-step t of chunk cc reads channel 8cc + 4(lane>>5) + t at the lane's pixel: a dword load whose lane offset is worked out
// once and whose chunk part is a scalar offset of the view's buffer descriptor.  Input, residual and output are each
// addressed as element (n, c, y, x) at p[n * ns + c * cs + y * rs + x + off]: a plain map or the interior of a zero-bordered one.
// A wave owns CT channel tiles x PT pixel tiles; waves are independent (no LDS, no barriers).
#include "common.h"

__global__ void pack_conv1x1_kernel(const float* __restrict__ w, int Cout, int Cin, float4* __restrict__ out, int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int lane = i & 63, f = i >> 6;
  const int cc = f % (Cin / 8), cot = f / (Cin / 8);
  const int co = cot * 32 + (lane & 31), ci = 8 * cc + 4 * (lane >> 5);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (co < Cout) {
    const float* p = w + (size_t)co * Cin + ci;
    v = make_float4(p[0], p[1], p[2], p[3]);
  }
  out[i] = v;
}

extern "C" size_t poem_conv1x1_packed_floats(int Cout, int Cin) { return packed_linear_floats(Cout, Cin); }

extern "C" hipError_t poem_launch_pack_conv1x1(const float* w, int Cout, int Cin, void* out, hipStream_t s) {
  if (Cin % 8) return hipErrorInvalidValue;
  const int total = ((Cout + 31) / 32) * (Cin / 8) * 64;
  hipLaunchKernelGGL(pack_conv1x1_kernel, dim3((total + 255) / 256), dim3(256), 0, s, w, Cout, Cin, (float4*)out, total);
  return hipGetLastError();
}

struct Conv1Args {
  const float* in;
  const float4* wp;
  const float* shift;   // (Cout) per-channel offset (conv bias + BatchNorm folded) or null
  const float* res;     // optional residual, added BEFORE the activation
  float* out;
  long in_ns, res_ns, out_ns;
  int in_cs, in_rs, in_off;
  int res_cs, res_rs, res_off;
  int out_cs, out_rs, out_off;
  int Cin, Cout, H, W, relu, views;
};

template <int CT, int PT>
__global__ __launch_bounds__(256) void conv1x1_nchw_kernel(Conv1Args A) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int ptiles = A.H * A.W / 32, pgroups = ptiles / PT;
  const int cogroups = ((A.Cout + 31) / 32) / CT;
  const long item = (long)blockIdx.x * 4 + wv;
  if (item >= (long)A.views * cogroups * pgroups) return;
  const int pg = (int)(item % pgroups);
  const int cg = (int)((item / pgroups) % cogroups);
  const int n = (int)(item / ((long)pgroups * cogroups));
  const int KC = A.Cin / 8;
  const __amdgpu_buffer_rsrc_t xrs = frag_rsrc(A.in + (size_t)n * A.in_ns, (unsigned)((size_t)A.Cin * A.in_cs * 4));
  const __amdgpu_buffer_rsrc_t wrs = frag_rsrc(A.wp, 0xffffffffu);

  int xoff[PT];      // lane byte offset: channel 4h at the lane's pixel
  int py[PT], px[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int pix = (pg * PT + p) * 32 + j;
    py[p] = pix / A.W;
    px[p] = pix % A.W;
    xoff[p] = (4 * h * A.in_cs + py[p] * A.in_rs + px[p] + A.in_off) * 4;
  }
  f32x16 acc[CT][PT];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int p = 0; p < PT; ++p) acc[c][p] = zero16();
  const int wbase = (cg * CT) * KC * 1024;        // bytes
  // Two-stage software pipeline over the KC 8-channel chunks with pinned order (sched_barrier): the operands of chunk
  // q + 1 are in flight while the 4 * CT * PT MFMAs of chunk q issue.
  int cc = 0;
  float4 a0[CT], a1[CT];
  float b0[PT][4], b1[PT][4];
#define POEM_CLOAD(AW, B)                                                                                         \
  {                                                                                                               \
    const int woff_ = wbase + cc * 1024;                                                                          \
    const int soff_ = cc * 8 * A.in_cs * 4;                                                                       \
    _Pragma("unroll") for (int c = 0; c < CT; ++c) AW[c] = frag_load(wrs, lane * 16, woff_ + c * KC * 1024);      \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                 \
      _Pragma("unroll") for (int p = 0; p < PT; ++p)                                                              \
        B[p][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, xoff[p], soff_ + t * A.in_cs * 4, 0)); \
    if (cc + 1 < KC) ++cc;   /* saturates on the last chunk */                                                    \
  }
#define POEM_CMMA(AW, B)                                                                                          \
  _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                   \
    _Pragma("unroll") for (int c = 0; c < CT; ++c)                                                                \
      _Pragma("unroll") for (int p = 0; p < PT; ++p) acc[c][p] = mfma32((&AW[c].x)[t], B[p][t], acc[c][p]);
  POEM_CLOAD(a0, b0)
  int done = 0;
  for (; done + 1 < KC; done += 2) {
    POEM_CLOAD(a1, b1)
    __builtin_amdgcn_sched_barrier(0);
    POEM_CMMA(a0, b0)
    __builtin_amdgcn_sched_barrier(0);
    POEM_CLOAD(a0, b0)
    __builtin_amdgcn_sched_barrier(0);
    POEM_CMMA(a1, b1)
    __builtin_amdgcn_sched_barrier(0);
  }
  if (done < KC) { POEM_CMMA(a0, b0) }   // odd chunk count: the last chunk is already in (a0, b0)
#undef POEM_CLOAD
#undef POEM_CMMA
  // epilogue: shift, residual, ReLU; lane = pixel, register e = channel 8(e>>2) + 4h + (e&3)
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int cbase = (cg * CT + c) * 32 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = cbase + 8 * g + e;
        if (co >= A.Cout) continue;
        const float sh = A.shift ? A.shift[co] : 0.f;
#pragma unroll
        for (int p = 0; p < PT; ++p) {
          float v = acc[c][p][4 * g + e] + sh;
          if (A.res) v += A.res[(size_t)n * A.res_ns + (size_t)co * A.res_cs + py[p] * A.res_rs + px[p] + A.res_off];
          if (A.relu) v = relu_nan(v);
          A.out[(size_t)n * A.out_ns + (size_t)co * A.out_cs + py[p] * A.out_rs + px[p] + A.out_off] = v;
        }
      }
    }
  }
}

// Cin % 8 == 0, (H * W) % 32 == 0, a view of the input below 2 GiB (32-bit buffer offsets).
extern "C" hipError_t poem_launch_conv1x1_nchw(const float* in, long in_ns, int in_cs, int in_rs, int in_off, const void* wp,
                                               const float* shift, const float* res, long res_ns, int res_cs, int res_rs,
                                               int res_off, float* out, long out_ns, int out_cs, int out_rs, int out_off, int views,
                                               int Cin, int Cout, int H, int W, int relu, hipStream_t s) {
  if (Cin % 8 || (H * W) % 32) return hipErrorInvalidValue;
  if ((size_t)Cin * (size_t)in_cs * 4 >= (1ull << 31)) return hipErrorInvalidValue;
  Conv1Args a{in, (const float4*)wp, shift, res, out, in_ns, res_ns, out_ns, in_cs, in_rs, in_off, res_cs, res_rs, res_off,
              out_cs, out_rs, out_off, Cin, Cout, H, W, relu, views};
  const int cot = (Cout + 31) / 32, ptiles = H * W / 32;
  const int pt = (ptiles % 2 == 0) ? 2 : 1;
  const int ct = (cot % 5 == 0) ? 5 : (cot % 4 == 0) ? 4 : (cot % 3 == 0) ? 3 : (cot % 2 == 0) ? 2 : 1;
  const long items = (long)views * (cot / ct) * (ptiles / pt);
  const dim3 grid((unsigned)((items + 3) / 4)), block(256);
#define POEM_CONV1(CTV)                                                                                \
  {                                                                                                    \
    if (pt == 2) hipLaunchKernelGGL((conv1x1_nchw_kernel<CTV, 2>), grid, block, 0, s, a);                   \
    else hipLaunchKernelGGL((conv1x1_nchw_kernel<CTV, 1>), grid, block, 0, s, a);                           \
  }
  switch (ct) {
    case 5: POEM_CONV1(5) break;
    case 4: POEM_CONV1(4) break;
    case 3: POEM_CONV1(3) break;
    case 2: POEM_CONV1(2) break;
    default: POEM_CONV1(1) break;
  }
#undef POEM_CONV1
  return hipGetLastError();
}

// ---- fuse sum ---------------------------------------------------------------------------------------------------------------
struct FuseTerm {
  const float* p;
  long ns;
  int cs, rs, off, shift;      // element (n, c, y, x) of the sum reads p[n * ns + c * cs + (y >> shift) * rs + (x >> shift) + off]
};
struct FuseArgs {
  FuseTerm t[4];
  int nterms;
  float* out;
  long out_ns;
  int out_cs, out_rs, out_off;
  int C, H, W;
  long total;
};

// one thread per output element; the terms are added left to right as upstream adds them (y = y + t), then ReLU as torch
// evaluates it (a NaN stays a NaN)
__global__ __launch_bounds__(256) void hrnet_fuse_kernel(FuseArgs A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.total) return;
  const int x = (int)(i % A.W);
  long r = i / A.W;
  const int y = (int)(r % A.H);
  r /= A.H;
  const int c = (int)(r % A.C);
  const long n = r / A.C;
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < A.nterms) {
      const FuseTerm& t = A.t[k];
      const float u = t.p[(size_t)n * t.ns + (size_t)c * t.cs + (size_t)(y >> t.shift) * t.rs + (x >> t.shift) + t.off];
      v = k == 0 ? u : v + u;
    }
  }
  A.out[(size_t)n * A.out_ns + (size_t)c * A.out_cs + (size_t)y * A.out_rs + x + A.out_off] = relu_nan(v);
}

extern "C" hipError_t poem_launch_hrnet_fuse(const float* const* ptrs, const long* ns, const int* cs, const int* rs, const int* off,
                                             const int* shift, int nterms, float* out, long out_ns, int out_cs, int out_rs,
                                             int out_off, int views, int C, int H, int W, hipStream_t s) {
  if (nterms < 2 || nterms > 4) return hipErrorInvalidValue;
  FuseArgs a{};
  for (int k = 0; k < nterms; ++k) a.t[k] = FuseTerm{ptrs[k], ns[k], cs[k], rs[k], off[k], shift[k]};
  a.nterms = nterms;
  a.out = out;
  a.out_ns = out_ns; a.out_cs = out_cs; a.out_rs = out_rs; a.out_off = out_off;
  a.C = C; a.H = H; a.W = W;
  a.total = (long)views * C * H * W;
  const long blocks = (a.total + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hrnet_fuse_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}
