// Baseline-JPEG reconstruction arithmetic shared by the host loops (csrc/jpeg.cpp) and the device kernels (csrc/jpeg.hip):
// inverse DCT, "fancy" chroma up-sampling and YCbCr -> RGB, all in 32-bit integers.  This is the CONTRACT of the device decode
// route: it restates libjpeg's default decompression path (jidctint.c "islow", jdsample.c h2v1 / h2v2 fancy up-sampling,
// jdcolor.c 16-bit fixed point) so that the bytes equal what PIL returns for the same stream -- provided the range guard below
// holds, which the entropy decoder checks per block and refuses the image otherwise.
//
// Range guard (POEM_JPEG_L1_MAX).  libjpeg-turbo runs this IDCT in SIMD on 16-bit lanes: the dequantised coefficients and the
// column pass's results are held as int16 (saturating packs), sums of two inputs of a pass are formed with 16-bit adds, and the
// products are accumulated in 32 bits.  Its C code and a plain restatement do not saturate, so out-of-range data decodes
// differently in each.  With L1 = sum over the 64 entries of a block of |coef * quant|:
//   - every output of one pass is a linear form  sum_k m_k x_k  of its 8 inputs whose multipliers are the scaled basis
//     sqrt(2) cos((2n+1) k pi / 16) * 2^13 (1 * 2^13 for k = 0) up to the rounding of the constants: |m_k| <= 11366;
//     every INTERMEDIATE of the pass is such a form too, with |m_k| <= 27431 (the largest, z2 + z3 on x3, is 20995 + 6436), and
//     in any other grouping of the same products (the SIMD code multiplies pairs by int16 constants) |m_k| < 2^15 per product;
//   - column pass: a column's inputs have L1_col <= L1, so |x_k| <= L1 fits int16, intermediates stay below 2^15 * L1 < 2^31, and
//     the result  w = (v + 2^10) >> 11  has |w| <= 11366 L1_col / 2048 + 1 = 5.55 L1_col + 1;
//   - row pass: the inputs of one row come from 8 different columns, so ANY partial sum of them is bounded by
//     sum_c (5.55 L1_col(c) + 1) <= 5.55 L1 + 8.  L1 <= 5900 keeps that at 32753 <= 32767: no workspace value and no 16-bit sum
//     of workspace values saturates or wraps, and the 32-bit accumulations stay below 2^15 * 32753 < 2^31;
//   - the final  (v + 2^17) >> 18  is then below 2^13, and clamp(v + 128, 0, 255) is what saturating packs give.
// So for L1 <= 5900 a 32-bit, a 64-bit and a 16-bit-saturating evaluation agree bit for bit.  Typical data is far inside:
// photographic blocks at quality 30..100 measure L1 <= ~3000, saturated 0/255 noise at quality 100 about 4700.
#ifndef POEM_JPEG_H
#define POEM_JPEG_H

#include <stdint.h>

#if defined(__HIP__) || defined(__CUDACC__)
#define POEM_JPEG_HD __host__ __device__ inline
#else
#define POEM_JPEG_HD inline
#endif

#define POEM_JPEG_L1_MAX 5900

POEM_JPEG_HD int jpeg_descale(int v, int s) { return (v + (1 << (s - 1))) >> s; }

// One 1-D pass: x[0..7] -> o[0..7], each result descaled by s bits (11 for the column pass, 18 for the row pass).
POEM_JPEG_HD void jpeg_idct_pass(const int (&x)[8], int (&o)[8], int s) {
  // even part
  int z1 = (x[2] + x[6]) * 4433;
  int t2 = z1 - x[6] * 15137;
  int t3 = z1 + x[2] * 6270;
  int t0 = (x[0] + x[4]) * 8192;          // << 13, written as a product: a shift of a negative int is undefined before C++20
  int t1 = (x[0] - x[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  // odd part
  t0 = x[7]; t1 = x[5]; t2 = x[3]; t3 = x[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * 9633;
  t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  o[0] = jpeg_descale(t10 + t3, s); o[7] = jpeg_descale(t10 - t3, s);
  o[1] = jpeg_descale(t11 + t2, s); o[6] = jpeg_descale(t11 - t2, s);
  o[2] = jpeg_descale(t12 + t1, s); o[5] = jpeg_descale(t12 - t1, s);
  o[3] = jpeg_descale(t13 + t0, s); o[4] = jpeg_descale(t13 - t0, s);
}

POEM_JPEG_HD int jpeg_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
POEM_JPEG_HD int jpeg_sample(int v) { return jpeg_clamp255(v + 128); }          // a row-pass result -> the stored sample

// Chroma up-sampling ("fancy"; used when the component is more than 2 samples wide -- a narrower one, i.e. an image of width <= 4,
// is replicated 2x1 / 2x2 instead, as libjpeg's jinit_upsampler chooses: jpeg_pixel below).  `row` / `row_other` point at rows of the component's plane, cw is the component's OWN width
// (ceil(W / 2), not the padded pitch), x the output column.
// Horizontal x2 only (4:2:2): the first output is p[0], the last p[cw-1].
POEM_JPEG_HD int jpeg_up_h2v1(const unsigned char* row, int cw, int x) {
  const int j = x >> 1, p = row[j];
  if (x & 1) return j == cw - 1 ? p : (3 * p + row[j + 1] + 2) >> 2;
  return j == 0 ? p : (3 * p + row[j - 1] + 1) >> 2;
}
// x2 both ways (4:2:0): row = plane row y >> 1, row_other = the row above (even y, clamped to 0) or below (odd y, clamped to
// ch - 1); c[j] = 3 row[j] + row_other[j].
POEM_JPEG_HD int jpeg_up_h2v2(const unsigned char* row, const unsigned char* row_other, int cw, int x) {
  const int j = x >> 1, c = 3 * row[j] + row_other[j];
  if (x & 1) return j == cw - 1 ? (4 * c + 7) >> 4 : (3 * c + (3 * row[j + 1] + row_other[j + 1]) + 7) >> 4;
  return j == 0 ? (4 * c + 8) >> 4 : (3 * c + (3 * row[j - 1] + row_other[j - 1]) + 8) >> 4;
}

// YCbCr -> RGB, 16-bit fixed point; packed as r | g << 8 | b << 16.
POEM_JPEG_HD unsigned jpeg_ycc_rgb(int y, int cb, int cr) {
  cb -= 128; cr -= 128;
  const int r = jpeg_clamp255(y + ((91881 * cr + 32768) >> 16));
  const int g = jpeg_clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  const int b = jpeg_clamp255(y + ((116130 * cb + 32768) >> 16));
  return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16);
}

// The sizes a descriptor implies, and whether they hang together (the kernels and the host loops address the planes through
// them, so a descriptor that fails this is skipped whole).  D = poem_jpeg_desc_t.
template <class D>
POEM_JPEG_HD bool jpeg_desc_ok(const D& d) {
  if (d.status != 0 || d.height < 1 || d.width < 1 || d.height > 65500 || d.width > 65500) return false;
  if (d.ncomp != 1 && d.ncomp != 3) return false;
  if (d.hs < 1 || d.hs > 2 || d.vs < 1 || d.vs > d.hs) return false;
  if (d.ncomp == 1 && (d.hs != 1 || d.vs != 1)) return false;
  const int cw = (d.width + d.hs - 1) / d.hs, ch = (d.height + d.vs - 1) / d.vs;
  if (d.blocks_w[0] < 1 || d.blocks_h[0] < 1 || d.blocks_w[0] > 8192 || d.blocks_h[0] > 8192) return false;
  if (d.blocks_w[0] * 8 < d.width || d.blocks_h[0] * 8 < d.height) return false;
  for (int c = 1; c < d.ncomp; ++c)
    if (d.blocks_w[c] < 1 || d.blocks_h[c] < 1 || d.blocks_w[c] > 8192 || d.blocks_h[c] > 8192 || d.blocks_w[c] * 8 < cw ||
        d.blocks_h[c] * 8 < ch)
      return false;
  return d.coef_offset >= 0 && (d.coef_offset & 15) == 0 && d.block_base >= 0 && d.quad_base >= 0;
}
template <class D>
POEM_JPEG_HD long long jpeg_desc_blocks(const D& d) {
  long long n = 0;
  for (int c = 0; c < d.ncomp; ++c) n += (long long)d.blocks_w[c] * d.blocks_h[c];
  return n;
}

// One output pixel from the three (or one) component planes of an image: planes[c] with pitch[c] bytes per row.
template <class D>
POEM_JPEG_HD unsigned jpeg_pixel(const D& d, const unsigned char* const* plane, const int* pitch, int x, int y) {
  const int Y = plane[0][(long long)y * pitch[0] + x];
  if (d.ncomp == 1) return (unsigned)Y * 0x010101u;
  int cb, cr;
  if (d.hs == 1) {
    cb = plane[1][(long long)y * pitch[1] + x];
    cr = plane[2][(long long)y * pitch[2] + x];
  } else {
    const int cw = (d.width + 1) >> 1;
    if (cw <= 2) {                  // libjpeg's rule (jdsample.c): fancy taps only when the component is wider than 2 samples
      const long long row = y >> (d.vs - 1);
      cb = plane[1][row * pitch[1] + (x >> 1)];
      cr = plane[2][row * pitch[2] + (x >> 1)];
    } else if (d.vs == 1) {
      cb = jpeg_up_h2v1(plane[1] + (long long)y * pitch[1], cw, x);
      cr = jpeg_up_h2v1(plane[2] + (long long)y * pitch[2], cw, x);
    } else {
      const int ch = (d.height + 1) >> 1, i = y >> 1;
      const int o = (y & 1) ? (i + 1 < ch ? i + 1 : ch - 1) : (i > 0 ? i - 1 : 0);
      cb = jpeg_up_h2v2(plane[1] + (long long)i * pitch[1], plane[1] + (long long)o * pitch[1], cw, x);
      cr = jpeg_up_h2v2(plane[2] + (long long)i * pitch[2], plane[2] + (long long)o * pitch[2], cw, x);
    }
  }
  return jpeg_ycc_rgb(Y, cb, cr);
}

#endif  // POEM_JPEG_H
