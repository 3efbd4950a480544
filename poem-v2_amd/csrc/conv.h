// The convolution family (decode.hip, hrnet.hip, resnet.hip): how a feature map is addressed, the argument blocks of the
// kernels whose launchers ops.cpp fills, and -- for the device passes only -- what the kernels of the three files share:
// the wave-item split, the direct two-stage main loop, the tile epilogue walks and the bilinear x2 tap rule.
#pragma once
#include <hip/hip_runtime.h>

// A map: element (n, c, y, x) of a (views, C, H, W) tensor is p[n * ns + c * cs + y * rs + x + off] -- a plain tensor or the
// interior of a zero-bordered one (off = the border's first row and column).  Kernels that read a map through a per-view buffer
// descriptor take its base from at(n, 0, 0, 0) and put the channel into the scalar offset.
struct ConvMap {
  long ns;
  int cs, rs, off;
  ConvMap() = default;
  __host__ __device__ ConvMap(long ns_, int cs_, int rs_, int off_) : ns(ns_), cs(cs_), rs(rs_), off(off_) {}
  __host__ __device__ ConvMap(int C, int H, int W) : ns((long)C * H * W), cs(H * W), rs(W), off(0) {}      // plain (views, C, H, W)
  __host__ __device__ size_t at(long n, int c, int y, int x) const { return (size_t)n * ns + (size_t)c * cs + y * rs + x + off; }
};

// conv1x1_nchw_kernel (hrnet.hip): Cin % 8 == 0, (H * W) % 32 == 0, a view of the input below 2 GiB (32-bit buffer offsets)
struct Conv1Args {
  const float* in;
  const float4* wp;
  const float* shift;   // (Cout) per-channel offset (conv bias + BatchNorm folded) or null
  const float* res;     // optional residual, added BEFORE the activation
  float* out;
  ConvMap imap, rmap, omap;
  int Cin, Cout, H, W, relu, views;
};

// hrnet_fuse_kernel (hrnet.hip): element (n, c, y, x) of the sum reads term k at (n, c, y >> shift, x >> shift)
struct FuseTerm {
  const float* p;
  ConvMap map;
  int shift;
};
struct FuseArgs {
  FuseTerm t[4];
  int nterms;           // 2..4
  float* out;
  ConvMap omap;
  int C, H, W, views;
};

// conv7x7_s2_kernel (resnet.hip): H, W even, (H/2 * W/2) % 32 == 0, Cout % 32 == 0, a view of the input below 2 GiB
struct StemArgs {
  const float* in;       // (views, 3, H, W) plain
  const float4* wp;
  const float* scale;
  const float* shift;
  float* out;            // map (views, Cout, H/2, W/2)
  ConvMap omap;
  int Cout, H, W, views;
};

// maxpool3x3_s2_kernel (resnet.hip): H, W even
struct PoolArgs {
  const float* in;
  float* out;
  ConvMap imap, omap;
  int C, H, W, views;    // of the input; the output is (H/2, W/2)
};

// sconv1x1_kernel (resnet.hip): H, W even, (H/2 * W/2) % 32 == 0, Cin % 8 == 0
struct SConvArgs {
  const float* in;       // map (views, Cin, H, W)
  const float4* wp;      // poem_pack_conv1x1 image
  const float* shift;    // (Cout) or null
  float* out;            // map (views, Cout, H/2, W/2)
  ConvMap imap, omap;
  int Cin, Cout, H, W, pool, act, views;        // pool: 0 = in(2y, 2x), 1 = max_pool2d(2, 2); act: 0 none, 1 sigmoid
};

#if defined(__HIPCC__)
#include "common.h"

// ---- wave items ---------------------------------------------------------------------------------------------------------------
// The direct kernels run four independent waves a block; wave `item` of the launch owns channel-tile group cg of pixel-tile group
// pg of view n, pg fastest.
static inline dim3 conv_item_grid(long items) { return dim3((unsigned)((items + 3) / 4)); }
struct ConvItem { int n, cg, pg; };
__device__ __forceinline__ bool conv_item(int views, int cogroups, int pgroups, ConvItem& it) {
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)views * cogroups * pgroups) return false;
  it.pg = (int)(item % pgroups);
  it.cg = (int)((item / pgroups) % cogroups);
  it.n = (int)(item / ((long)pgroups * cogroups));
  return true;
}

// ---- the direct main loop -----------------------------------------------------------------------------------------------------
// acc[c][p] += sum over the TAPS * KC (tap, 8-channel chunk) steps -- taps outer, chunks inner -- of A (packed weights: tile c
// of the wave's group, `wbase` its first byte, tile stride TAPS * KC KiB) times B (the input itself: lane = pixel, k-step t of
// chunk cc reads channel 8cc + 4(lane>>5) + t at the lane's byte offset xoff[p] -- channel 4(lane>>5) of tap (0, 0) -- plus the
// scalar offset of (chunk, tap, k-step); `plane` floats between channels, `row` between a 3x3's tap rows).
// Two-stage software pipeline with pinned order (sched_barrier): the operands of step q + 1 are in flight while the
// 4 * CT * PT MFMAs of step q issue.
template <int CT, int PT, int TAPS>
__device__ __forceinline__ void conv_direct_loop(f32x16 (&acc)[CT][PT], __amdgpu_buffer_rsrc_t xrs, __amdgpu_buffer_rsrc_t wrs,
                                                 const int (&xoff)[PT], int lane, int wbase, int KC, int plane, int row) {
  static_assert(TAPS == 9 || TAPS == 1, "3x3 or 1x1");
  const int total = TAPS * KC;
  int tap = 0, cc = 0, q = 0;
  float4 a0[CT], a1[CT];
  float b0[PT][4], b1[PT][4];
#define POEM_CLOAD(A, B)                                                                                          \
  {                                                                                                               \
    const int woff_ = wbase + (tap * KC + cc) * 1024;                                                             \
    const int soff_ = cc * 8 * plane * 4 + (TAPS == 1 ? 0 : ((tap / 3) * row + (tap % 3)) * 4);                   \
    _Pragma("unroll") for (int c = 0; c < CT; ++c) A[c] = frag_load(wrs, lane * 16, woff_ + c * TAPS * KC * 1024); \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                 \
      _Pragma("unroll") for (int p = 0; p < PT; ++p)                                                              \
        B[p][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, xoff[p], soff_ + t * plane * 4, 0)); \
    if constexpr (TAPS == 1) { if (cc + 1 < KC) ++cc; }              /* one tap: the step is the chunk */          \
    else if (q + 1 < total) { ++q; if (++cc == KC) { cc = 0; ++tap; } }   /* both saturate on the last step */     \
  }
#define POEM_CMMA(A, B)                                                                                           \
  _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                                   \
    _Pragma("unroll") for (int c = 0; c < CT; ++c)                                                                \
      _Pragma("unroll") for (int p = 0; p < PT; ++p) acc[c][p] = mfma32((&A[c].x)[t], B[p][t], acc[c][p]);
  POEM_CLOAD(a0, b0)
  int done = 0;
  for (; done + 1 < total; done += 2) {
    POEM_CLOAD(a1, b1)
    __builtin_amdgcn_sched_barrier(0);
    POEM_CMMA(a0, b0)
    __builtin_amdgcn_sched_barrier(0);
    POEM_CLOAD(a0, b0)
    __builtin_amdgcn_sched_barrier(0);
    POEM_CMMA(a1, b1)
    __builtin_amdgcn_sched_barrier(0);
  }
  if (done < total) { POEM_CMMA(a0, b0) }   // odd step count: the last step is already in (a0, b0)
#undef POEM_CLOAD
#undef POEM_CMMA
}

// ---- tile epilogues -----------------------------------------------------------------------------------------------------------
// Which output channel an accumulator register holds.  Both walks visit a wave's registers in (c, g, e) order, skip the channels
// of a last tile beyond Cout, and leave the per-element expression to the kernel: group(cb) is called once per run of four
// consecutive channels cb .. cb + 3 (a kernel's float4 scale / shift loads; the packed arrays are padded to whole tiles) and
// what it returns is handed on to elem(co, c, r, what group returned) for channel co = cb + (r & 3), held in register r of tile c.
// (conv3x3_s2p_kernel and conv1x1_nchw_kernel write the same walk out: the first batches its residual loads, the second lost time here.)
struct Affine4 { float4 sc, sh; };
__device__ __forceinline__ Affine4 affine4(const float* scale, const float* shift, int cb) {
  return Affine4{*reinterpret_cast<const float4*>(scale + cb), *reinterpret_cast<const float4*>(shift + cb)};
}
__device__ __forceinline__ int no_group(int) { return 0; }
// 32x32x2 tiles: lane = pixel, half-wave h; register r = 4g + e of tile c is channel (ct0 + c) * 32 + 4h + 8g + e
template <int CT, class Group, class Elem>
__device__ __forceinline__ void tile32_channels(int ct0, int h, int Cout, Group&& group, Elem&& elem) {
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cb = (ct0 + c) * 32 + 4 * h + 8 * g;
      const auto gs = group(cb);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (cb + e >= Cout) continue;
        elem(cb + e, c, 4 * g + e, gs);
      }
    }
}
// 16x16x4 tiles, two units of 16 pixels: lane (g = lane >> 4, j = lane & 15) holds, for pixel j of either unit, channel
// ch0 + 16c + 4g + e in register r = e of tile c
template <int CT16, class Group, class Elem>
__device__ __forceinline__ void tile16_channels(int ch0, int g, int Cout, Group&& group, Elem&& elem) {
#pragma unroll
  for (int c = 0; c < CT16; ++c) {
    const int cb = ch0 + c * 16 + 4 * g;
    const auto gs = group(cb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (cb + e >= Cout) continue;
      elem(cb + e, c, e, gs);
    }
  }
}

// ---- bilinear x2 --------------------------------------------------------------------------------------------------------------
// F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) along one axis: destination index d of a source of n
// samples reads i0 and i1 with weights h and l (src = (d + 0.5) / 2 - 0.5, clamped at 0).  Every route that interpolates takes
// its taps from here; the routes the tests hold bit for bit against each other differ only in how they combine the four taps.
struct Up2Tap { int i0, i1; float l, h; };
__device__ __forceinline__ Up2Tap up2_tap(int d, int n) {
  const float s = fmaxf((d + 0.5f) * 0.5f - 0.5f, 0.f);
  Up2Tap t;
  t.i0 = (int)s;
  t.i1 = min(t.i0 + 1, n - 1);
  t.l = s - (float)t.i0;
  t.h = 1.f - t.l;
  return t;
}
// the four taps p[y.i0 | y.i1][x.i0 | x.i1] of a plane of row length w, combined as torch nests the two directions ...
__device__ __forceinline__ float up2_nested(const float* p, int w, const Up2Tap& y, const Up2Tap& x) {
  return y.h * (x.h * p[y.i0 * w + x.i0] + x.l * p[y.i0 * w + x.i1]) + y.l * (x.h * p[y.i1 * w + x.i0] + x.l * p[y.i1 * w + x.i1]);
}
// ... or with the weights multiplied out, one multiply and three fmas: what the stagers of the fused convolution evaluate
__device__ __forceinline__ float up2_staged(const float* p, int w, const Up2Tap& y, const Up2Tap& x) {
  const float q0 = y.h * x.h, q1 = y.h * x.l, q2 = y.l * x.h, q3 = y.l * x.l;
  return fmaf(q3, p[y.i1 * w + x.i1], fmaf(q2, p[y.i1 * w + x.i0], fmaf(q1, p[y.i0 * w + x.i1], q0 * p[y.i0 * w + x.i0])));
}
#endif
