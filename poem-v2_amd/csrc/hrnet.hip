// Row H of the scope table: what the HRNet-W40 backbone (lib/models/backbones/hrnet.py upstream) needs besides the 3x3
// convolutions of decode.hip --
//   conv1x1_nchw_kernel 1x1 convolution on NCHW (the Bottleneck's 64 -> 64, 256 -> 64, 64 -> 256, downsample.0 and the up-going
//                      fuse layers): D[co][pixel] = sum_ci W[co][ci] * X[ci][pixel] per view on the fp32 matrix cores
//   hrnet_fuse_kernel  the fuse sum of a HighResolutionModule (hrnet.py:226-233): relu(((t0 + t1) + t2) + t3) with the
//                      nearest-neighbour upsampling of the lower-resolution terms applied while they are read
// conv1x1 is the direct main loop of conv.h with one tap: lane = pixel (32 raster-consecutive pixels of a view), the packed
// weights are the A operand --
//   WP[(cot * Cin/8 + cc) * 64 + lane] = float4( W[32cot + (lane&31)][8cc + 4(lane>>5) + 0..3] )   (rows >= Cout zero)
// -- k-step t of chunk cc reads channel 8cc + 4(lane>>5) + t at the lane's pixel: a dword load whose lane offset is worked out
// once and whose chunk part is a scalar offset of the view's buffer descriptor.  Input, residual and output are each a ConvMap.
// A wave owns CT channel tiles x PT pixel tiles; waves are independent (no LDS, no barriers).
#include "conv.h"

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

template <int CT, int PT>
__global__ __launch_bounds__(256) void conv1x1_nchw_kernel(Conv1Args A) {
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  ConvItem it;
  if (!conv_item(A.views, ((A.Cout + 31) / 32) / CT, A.H * A.W / 32 / PT, it)) return;
  const int n = it.n, cg = it.cg;
  const int KC = A.Cin / 8;
  // the map's offset rides in the lane offsets, the channel in the scalar offset
  const __amdgpu_buffer_rsrc_t xrs = frag_rsrc(A.in + (size_t)n * A.imap.ns, (unsigned)((size_t)A.Cin * A.imap.cs * 4));
  const __amdgpu_buffer_rsrc_t wrs = frag_rsrc(A.wp, 0xffffffffu);

  int xoff[PT];      // lane byte offset: channel 4h at the lane's pixel
  int py[PT], px[PT];
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    const int pix = (it.pg * PT + p) * 32 + j;
    py[p] = pix / A.W;
    px[p] = pix % A.W;
    xoff[p] = (4 * h * A.imap.cs + py[p] * A.imap.rs + px[p] + A.imap.off) * 4;
  }
  f32x16 acc[CT][PT];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int p = 0; p < PT; ++p) acc[c][p] = zero16();
  conv_direct_loop<CT, PT, 1>(acc, xrs, wrs, xoff, lane, (cg * CT) * KC * 1024, KC, A.imap.cs, 0);
  // epilogue: shift, residual, ReLU; lane = pixel, register 4g + e of tile c = channel (cg * CT + c) * 32 + 4h + 8g + e.  Written
  // out, not through tile32_channels of conv.h: through it ResNet-50 at 256 views took 51.7 ms instead of 51.1 (LABNOTES).
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
          if (A.res) v += A.res[A.rmap.at(n, co, py[p], px[p])];
          if (A.relu) v = relu_nan(v);
          A.out[A.omap.at(n, co, py[p], px[p])] = v;
        }
      }
    }
  }
}

extern "C" hipError_t poem_launch_conv1x1_nchw(const Conv1Args* args, hipStream_t s) {
  const Conv1Args& a = *args;
  if (a.Cin % 8 || (a.H * a.W) % 32) return hipErrorInvalidValue;
  if ((size_t)a.Cin * (size_t)a.imap.cs * 4 >= (1ull << 31)) return hipErrorInvalidValue;
  const int cot = (a.Cout + 31) / 32, ptiles = a.H * a.W / 32;
  const int pt = (ptiles % 2 == 0) ? 2 : 1;
  const int ct = (cot % 5 == 0) ? 5 : (cot % 4 == 0) ? 4 : (cot % 3 == 0) ? 3 : (cot % 2 == 0) ? 2 : 1;
  const dim3 grid = conv_item_grid((long)a.views * (cot / ct) * (ptiles / pt)), block(256);
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
// one thread per output element; the terms are added left to right as upstream adds them (y = y + t), then ReLU as torch
// evaluates it (a NaN stays a NaN)
__global__ __launch_bounds__(256) void hrnet_fuse_kernel(FuseArgs A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)A.views * A.C * A.H * A.W) return;
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
      const float u = t.p[t.map.at(n, c, y >> t.shift, x >> t.shift)];
      v = k == 0 ? u : v + u;
    }
  }
  A.out[A.omap.at(n, c, y, x)] = relu_nan(v);
}

extern "C" hipError_t poem_launch_hrnet_fuse(const FuseArgs* a, hipStream_t s) {
  if (a->nterms < 2 || a->nterms > 4) return hipErrorInvalidValue;
  const long blocks = ((long)a->views * a->C * a->H * a->W + 255) / 256;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hrnet_fuse_kernel, dim3((unsigned)blocks), dim3(256), 0, s, *a);
  return hipGetLastError();
}
