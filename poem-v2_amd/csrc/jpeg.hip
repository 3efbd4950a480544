// Device half of the JPEG route (include/poem_hip.h "baseline JPEG"): everything behind the Huffman decoder, for all images of a
// call in two launches.  Replaces, per view, what PIL / libjpeg do on one host thread inside webdataset's decode("rgb8")
// (dequantise -> 8x8 inverse DCT -> chroma up-sampling -> YCbCr -> RGB); the arithmetic is csrc/jpeg.h, shared with the host loops
// of csrc/jpeg.cpp, all 32-bit integers, bit-exact by construction.
//
//   jpeg_idct_kernel    one 8x8 block per 8 lanes (a wave holds 8 blocks, a 256-thread workgroup 32).  Lane r loads row r of the
//                       coefficients and of the component's quantisation table as one 16-byte load each, multiplies, and parks the
//                       products in the block's LDS tile; lane c then reads COLUMN c, runs the column pass and writes its results back
//                       over the column it read; lane r reads row r (two 16-byte LDS reads), runs the row pass and stores its 8 samples
//                       as ONE 8-byte store into the uint8 component plane.  A tile is 8 x 8 ints + 8 ints of padding: the column
//                       accesses of the 4 blocks of a 32-lane group then fall on 4 x 8 different banks (unpadded they would share 8).
//                       The quantisation rows come straight from the descriptors (L1 / L2 hits after the first block of an image): a
//                       workgroup's 32 blocks may belong to several images and components, so there is no one table to stage.
//   jpeg_colour_kernel  one lane per QUAD, 4 consecutive pixels of a row: Y and the chroma taps as byte loads through the edge rules
//                       of jpeg.h (neighbouring lanes share cache lines), 12 output bytes as three dwords where the destination sits
//                       on 4 bytes and all 4 pixels exist, byte stores otherwise (odd bases, odd widths, the last quad of a row).
// Ragged images go through prefix tables as in warp.hip: desc.block_base / desc.quad_base, searched per lane (<= 16 steps; the
// table is n * 464 bytes and stays in cache).  All byte offsets are 64-bit: 256 views of 640x480 are 2.4 M blocks and 236 MB of
// coefficients.  Memory-bound: per block 128 B of coefficients in and 64 B out, per pixel ~1.5 B in and 3 B out.
#include <hip/hip_runtime.h>
#include "../../include/poem_hip.h"
#include "jpeg.h"

namespace {

constexpr int kTile = 72;                    // ints per block tile in LDS: 64 + 8 of padding

// last i in [0, n) with base(i) <= idx; the bases are non-decreasing, images that hold nothing have empty ranges
template <class F>
__device__ __forceinline__ int find_image(int n, long long idx, F base) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base(mid) <= idx) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const poem_jpeg_desc_t* __restrict__ descs, const int16_t* __restrict__ coef,
                                                        long long coef_bytes, int n, long long total_blocks,
                                                        unsigned char* __restrict__ planes) {
  __shared__ __attribute__((aligned(16))) int tile[32 * kTile];
  const int r = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const long long gb = (long long)blockIdx.x * 32 + slot;
  int* t = tile + slot * kTile;
  bool live = gb < total_blocks;
  unsigned char* dst = nullptr;
  if (live) {
    const int i = find_image(n, gb, [&](int k) { return descs[k].block_base; });
    const poem_jpeg_desc_t& d = descs[i];
    long long local = gb - d.block_base;
    live = jpeg_desc_ok(d) && local < jpeg_desc_blocks(d) && d.block_base + jpeg_desc_blocks(d) <= total_blocks &&
           d.coef_offset <= coef_bytes &&
           (local + 1) * 128 <= coef_bytes - d.coef_offset;
    if (live) {
      const int4 cv = *reinterpret_cast<const int4*>(reinterpret_cast<const char*>(coef) + d.coef_offset + local * 128 + r * 16);
      int c = 0;
      long long plane_blocks = 0;                                  // blocks of this image in front of component c
      while (c + 1 < d.ncomp && local >= (long long)d.blocks_w[c] * d.blocks_h[c]) {
        local -= (long long)d.blocks_w[c] * d.blocks_h[c];
        plane_blocks += (long long)d.blocks_w[c] * d.blocks_h[c];
        ++c;
      }
      const int4 qv = *reinterpret_cast<const int4*>(&d.quant[c][r * 8]);
      const int bw = d.blocks_w[c], by = (int)(local / bw), bx = (int)(local % bw);
      dst = planes + (d.block_base + plane_blocks) * 64 + ((long long)by * 8 + r) * ((long long)bw * 8) + bx * 8;
      const int cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
      int p[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {                                // int16 coefficient x uint16 table entry, two per dword
        p[2 * k] = (int)(short)(cw[k] & 0xffff) * (int)(qw[k] & 0xffff);
        p[2 * k + 1] = (cw[k] >> 16) * (int)((unsigned)qw[k] >> 16);
      }
      *reinterpret_cast<int4*>(t + r * 8) = make_int4(p[0], p[1], p[2], p[3]);
      *reinterpret_cast<int4*>(t + r * 8 + 4) = make_int4(p[4], p[5], p[6], p[7]);
    }
  }
  __syncthreads();
  if (live) {                                                      // column r of the block: in place
    int x[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = t[k * 8 + r];
    jpeg_idct_pass(x, o, 11);
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k * 8 + r] = o[k];
  }
  __syncthreads();
  if (live) {                                                      // row r
    const int4 a = *reinterpret_cast<const int4*>(t + r * 8), b = *reinterpret_cast<const int4*>(t + r * 8 + 4);
    const int x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    int o[8];
    jpeg_idct_pass(x, o, 18);
    uint2 px;
    px.x = (unsigned)jpeg_sample(o[0]) | ((unsigned)jpeg_sample(o[1]) << 8) | ((unsigned)jpeg_sample(o[2]) << 16) |
           ((unsigned)jpeg_sample(o[3]) << 24);
    px.y = (unsigned)jpeg_sample(o[4]) | ((unsigned)jpeg_sample(o[5]) << 8) | ((unsigned)jpeg_sample(o[6]) << 16) |
           ((unsigned)jpeg_sample(o[7]) << 24);
    *reinterpret_cast<uint2*>(dst) = px;
  }
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const poem_jpeg_desc_t* __restrict__ descs, int n, long long total_quads,
                                                          long long total_blocks, const unsigned char* __restrict__ planes,
                                                          const long long* __restrict__ out_offsets, unsigned char* __restrict__ out,
                                                          long long out_bytes) {
  const long long gq = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gq >= total_quads) return;
  const int i = find_image(n, gq, [&](int k) { return descs[k].quad_base; });
  const poem_jpeg_desc_t& d = descs[i];
  if (!jpeg_desc_ok(d)) return;
  const int qpr = (d.width + 3) >> 2;
  const long long local = gq - d.quad_base;
  if (local >= (long long)d.height * qpr) return;
  const long long off = out_offsets[i], bytes = (long long)d.height * d.width * 3;
  if (off < 0 || off > out_bytes || bytes > out_bytes - off) return;                  // the image would not fit: leave it
  if (d.block_base + jpeg_desc_blocks(d) > total_blocks) return;                      // its planes are not in the workspace
  const int y = (int)(local / qpr), x4 = (int)(local % qpr) * 4;
  const unsigned char* plane[3];
  int pitch[3];
  {
    const unsigned char* p = planes + d.block_base * 64;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      plane[c] = p;
      pitch[c] = c < d.ncomp ? d.blocks_w[c] * 8 : 0;
      if (c < d.ncomp) p += (long long)d.blocks_w[c] * d.blocks_h[c] * 64;
    }
  }
  const int cnt = min(4, d.width - x4);
  unsigned rgb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) rgb[k] = k < cnt ? jpeg_pixel(d, plane, pitch, x4 + k, y) : 0u;
  unsigned char* o = out + off + ((long long)y * d.width + x4) * 3;
  if (cnt == 4 && ((uintptr_t)o & 3) == 0) {
    unsigned* w = reinterpret_cast<unsigned*>(o);
    w[0] = rgb[0] | (rgb[1] << 24);
    w[1] = (rgb[1] >> 8) | (rgb[2] << 16);
    w[2] = (rgb[2] >> 16) | (rgb[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) {
        o[3 * k] = (unsigned char)rgb[k];
        o[3 * k + 1] = (unsigned char)(rgb[k] >> 8);
        o[3 * k + 2] = (unsigned char)(rgb[k] >> 16);
      }
  }
}

}  // namespace

extern "C" hipError_t poem_launch_jpeg_reconstruct(const poem_jpeg_desc_t* descs, const int16_t* coef, long long coef_bytes,
                                                   const long long* out_offsets, unsigned char* out, long long out_bytes, int n,
                                                   long long total_blocks, long long total_quads, unsigned char* planes, hipStream_t s) {
  if (total_blocks > 0) {
    jpeg_idct_kernel<<<dim3((unsigned)((total_blocks + 31) / 32)), dim3(256), 0, s>>>(descs, coef, coef_bytes, n, total_blocks, planes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (total_quads > 0) {
    jpeg_colour_kernel<<<dim3((unsigned)((total_quads + 255) / 256)), dim3(256), 0, s>>>(descs, n, total_quads, total_blocks, planes,
                                                                                        out_offsets, out, out_bytes);
  }
  return hipGetLastError();
}
