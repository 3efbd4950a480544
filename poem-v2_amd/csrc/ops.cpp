// Operator-level entry points of libpoem_hip.so (include/poem_hip.h names the reference call each one replaces): argument
// checks around the launchers of launchers.h.  Stream-ordered, no allocation.
#include <cmath>
#include <cstdint>
#include <cstring>
#include "engine.h"

extern "C" {

// ---- individual operators -------------------------------------------------------------------------------------
int poem_gemm(const float* x, int ldx, const void* w_packed, const float* bias, const float* residual, int ldr, float* y,
              int ldy, int M, int N, int K, int act, void* stream) {
  if (!x || !w_packed || !y || M <= 0 || N <= 0 || K <= 0 || K % 8 || ldx % 4 || ((uintptr_t)x & 15)) return POEM_E_ARG;
  if (act < 0 || act > 2) return POEM_E_ARG;
  HIPCHK(poem_launch_gemm(x, ldx, w_packed, bias, residual, ldr, y, ldy, M, N, K, act, (hipStream_t)stream));
  return POEM_OK;
}

int poem_gemm_ex(const float* x, int ldx, const void* w_packed, const float* bias, const float* residual, int ldr,
                 float* y, int ldy, int M, int N, int K, int act, int in_layout, int out_layout, void* stream) {
  if (!x || !w_packed || !y || M <= 0 || N <= 0 || K <= 0 || K % 8 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
    return POEM_E_ARG;
  if (!in_layout && ldx % 4) return POEM_E_ARG;
  if (out_layout && N % 32) return POEM_E_ARG;
  if (act < 0 || act > 2 || (in_layout & ~1) || (out_layout & ~1)) return POEM_E_ARG;
  HIPCHK(poem_launch_gemm2(x, ldx, w_packed, bias, residual, ldr, y, ldy, M, N, K, act, in_layout, out_layout,
                           (hipStream_t)stream));
  return POEM_OK;
}

int poem_pack_rows(const float* x, int rows, int cols, void* packed, void* stream) {
  return poem_pack_linear(x, rows, cols, packed, stream);
}

int poem_unpack_rows(const void* packed, int rows, int cols, float* x, void* stream) {
  if (!packed || !x || rows <= 0 || cols % 8) return POEM_E_ARG;
  HIPCHK(poem_launch_unpack_rows(packed, rows, cols, x, (hipStream_t)stream));
  return POEM_OK;
}

int poem_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int cols, float eps,
                   void* stream) {
  if (!x || !gamma || !beta || !y || rows <= 0 || cols <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_layernorm(x, gamma, beta, y, rows, cols, eps, (hipStream_t)stream));
  return POEM_OK;
}

int poem_pe_table_ex(const void* adapt_w_packed, const float* adapt_b, int embed, int fh, int fw, int max_views, int normalize,
                     float* scratch_sine, float* table, void* stream) {
  if (!adapt_w_packed || !adapt_b || !scratch_sine || !table || embed % 2 || (fh * fw) % 32) return POEM_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(poem_launch_sine_pe(scratch_sine, embed / 2, fh, fw, max_views, normalize != 0, s));
  HIPCHK(poem_launch_conv1x1(scratch_sine, adapt_w_packed, adapt_b, nullptr, nullptr, table, nullptr, (int)pe_views(max_views),
                             3 * embed / 2, embed, fh * fw, s));
  return POEM_OK;
}

int poem_pe_table(const void* adapt_w_packed, const float* adapt_b, int embed, int fh, int fw, int max_views,
                  float* scratch_sine, float* table, void* stream) {
  return poem_pe_table_ex(adapt_w_packed, adapt_b, embed, fh, fw, max_views, 1, scratch_sine, table, stream);
}

int poem_frustum_features(const poem_config_t* cfg, const float* cam_intr, const float* cam_extr, int views, int img0, int img1,
                          float* out, void* stream) {
  if (!cfg || !cam_intr || !cam_extr || !out || views <= 0 || cfg->depth_num <= 0 || cfg->feat_h <= 0 || cfg->feat_w <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_frustum_features(cam_intr, cam_extr, out, views, cfg->feat_h, cfg->feat_w, cfg->depth_num, cfg->lid != 0,
                                      cfg->depth_start, cfg->depth_end, cfg->position_range, img0, img1, (hipStream_t)stream));
  return POEM_OK;
}

int poem_input_proj(const float* feat, const void* w_packed, const float* bias, const float* table,
                    const int32_t* pe_index, float* x, int views, int in_channels, int embed, int hw, void* stream) {
  if (!feat || !w_packed || !x || views <= 0 || in_channels % 8 || hw % 32) return POEM_E_ARG;
  if (table && !pe_index) return POEM_E_ARG;
  HIPCHK(poem_launch_conv1x1(feat, w_packed, bias, table, pe_index, x, nullptr, views, in_channels, embed, hw, (hipStream_t)stream));
  return POEM_OK;
}

int poem_project_sample(const float* x, const float* bps, const float* centre, const int32_t* view_sample,
                        const float* cam_intr, const float* cam_extr, float* uv_scratch, float* g, int views, int embed,
                        int fh, int fw, int nsample, int img_w, int img_h, void* stream) {
  if (!x || !bps || !centre || !view_sample || !cam_intr || !cam_extr || !uv_scratch || !g || views <= 0) return POEM_E_ARG;
  // the inverse extrinsics live in the tail of the uv scratch: caller provides (views*S*2 + views*16) floats
  float* inv = uv_scratch + (size_t)views * nsample * 2;
  HIPCHK(poem_launch_project_sample(x, bps, centre, view_sample, cam_intr, cam_extr, inv, uv_scratch, g, views, embed, fh,
                                    fw, nsample, img_w, img_h, (hipStream_t)stream));
  return POEM_OK;
}

int poem_merge_reduce(const float* h2, const int32_t* view_offsets, float* m, int batch, int nsample, int half,
                      void* stream) {
  if (!h2 || !view_offsets || !m || half > 512 || batch <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_merge_reduce(h2, view_offsets, m, batch, nsample, half, (hipStream_t)stream));
  return POEM_OK;
}

int poem_merge_finalize(const float* g, const float* y, const int32_t* view_offsets, float* out, int batch, int nsample,
                        int embed, void* stream) {
  if (!g || !y || !view_offsets || !out || batch <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_merge_finalize(g, y, view_offsets, out, batch, nsample, embed, (hipStream_t)stream));
  return POEM_OK;
}

size_t poem_cross_attention_scratch_bytes(int batch, int nq, int nk, int embed, int heads) {
  if (batch <= 0 || nq <= 0 || nk <= 0 || heads <= 0 || embed % heads) return 0;
  return poem_cross_attention_scratch_floats(batch, nq, nk, embed, heads, 1) * sizeof(float);
}

int poem_cross_attention(const float* q, const float* k, const float* v, float* ctx, int batch, int nq, int nk, int embed,
                         int heads, void* scratch, size_t scratch_bytes, void* stream) {
  if (!q || !k || !v || !ctx || batch <= 0 || nq <= 0 || nk <= 0 || heads <= 0 || embed % heads) return POEM_E_ARG;
  if (!poem_cross_attention_fits(batch, nk, embed)) return POEM_E_UNSUPPORTED;      // images past 2 GiB (include/poem_hip.h)
  const size_t need = poem_cross_attention_scratch_bytes(batch, nq, nk, embed, heads);
  if (need && (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 15))) return POEM_E_WORKSPACE;
  HIPCHK(poem_launch_cross_attention(q, k, v, ctx, batch, nq, nk, embed, heads, embed, (float*)scratch,
                                     (hipStream_t)stream));
  return POEM_OK;
}

int poem_cross_attention_merged(const float* q, const float* k, const float* v, float* ctx, int batch, int nq, int nk, int embed,
                                int heads, void* scratch, size_t scratch_bytes, void* stream) {
  if (!q || !k || !v || !ctx || batch <= 0 || nq <= 0 || nk <= 0 || heads <= 0 || embed % heads) return POEM_E_ARG;
  if (!poem_cross_attention_fits(batch, nk, embed)) return POEM_E_UNSUPPORTED;      // images past 2 GiB (include/poem_hip.h)
  const size_t need = poem_cross_attention_scratch_bytes(batch, nq, nk, embed, heads);
  if (need && (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 15))) return POEM_E_WORKSPACE;
  const hipError_t e = poem_launch_cross_attention_merged_rm(q, k, v, ctx, batch, nq, nk, embed, heads, (float*)scratch, (hipStream_t)stream);
  if (e == hipErrorNotSupported) return POEM_E_UNSUPPORTED;
  HIPCHK(e);
  return POEM_OK;
}

int poem_pack_split_gemm(const float* w, int out_features, int in_features, void* image, float* scales, void* stream) {
  if (!w || !image || !scales || out_features <= 0 || in_features <= 0 || in_features % 16) return POEM_E_ARG;
  HIPCHK(poem_launch_pack_split_tiles(w, out_features, in_features, image, scales, 1, (hipStream_t)stream));
  return POEM_OK;
}

int poem_gemm_split(const float* x, int ldx, const void* image, const float* scales, const float* bias, const float* residual,
                    int ldr, float* y, int ldy, int m, int n, int k, int act, void* stream) {
  if (!x || !image || !scales || !y || m <= 0 || n <= 0 || k <= 0 || k % 16 || n % 32) return POEM_E_ARG;
  if (act < POEM_ACT_NONE || act > POEM_ACT_GELU) return POEM_E_ARG;
  poem_gemm_split_explicit(image, scales);
  const hipError_t e = poem_launch_gemm(x, ldx, image, bias, residual, ldr, y, ldy, m, n, k, act, (hipStream_t)stream);
  poem_gemm_split_explicit(nullptr, nullptr);
  if (e == hipErrorInvalidValue) return POEM_E_UNSUPPORTED;          // shape outside the panel kernel's range
  HIPCHK(e);
  return POEM_OK;
}

int poem_pack_split_linear(const float* w, int embed, void* image, float* scale, void* stream) {
  if (!w || !image || !scale || embed < 128 || embed > 1024 || (embed & (embed - 1))) return POEM_E_ARG;
  HIPCHK(poem_launch_pack_split(w, embed, image, scale, (hipStream_t)stream));
  return POEM_OK;
}

int poem_vector_attention_split(const float* query_xyz, const float* src_xyz, const float* anchor_xyz, const int32_t* idx,
                                int shared_idx, const float* qg, const float* kg, const float* v, int nsrc, const float* wd1,
                                const float* bd1, const void* wd2_image, const float* bd2, const void* wg1d2_image,
                                const void* wg2_image, const float* scales, float* out, int batch, int nq, int embed,
                                void* stream) {
  if (!query_xyz || (!src_xyz && !anchor_xyz) || !idx || !qg || !kg || !v || !wd1 || !bd1 || !wd2_image || !bd2 ||
      !wg1d2_image || !wg2_image || !scales || !out || batch <= 0 || nq <= 0 || nsrc <= 0)
    return POEM_E_ARG;
  if (embed < 128 || embed > 1024 || (embed & (embed - 1))) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_vector_attention_split(query_xyz, src_xyz, anchor_xyz, idx, shared_idx, qg, kg, v, nsrc, wd1, bd1,
                                            wd2_image, bd2, wg1d2_image, wg2_image, scales, out, batch, nq, embed, embed,
                                            embed, embed, (hipStream_t)stream));
  return POEM_OK;
}

int poem_cross_attention_split_f16x3(const float* q, const float* k, const float* v, float* ctx, int batch, int nq, int nk,
                                     int embed, int heads, void* scratch, size_t scratch_bytes, void* stream) {
  if (heads <= 0 || embed % heads || (embed / heads != 32 && embed / heads != 64)) return POEM_E_UNSUPPORTED;
  if (nk % 32) return POEM_E_UNSUPPORTED;      // no MASK form of the split-precision kernels
  poem_cross_attention_split(1);
  const int rc = poem_cross_attention(q, k, v, ctx, batch, nq, nk, embed, heads, scratch, scratch_bytes, stream);
  poem_cross_attention_split(0);
  return rc;
}

int poem_knn(const float* query_xyz, const float* src_xyz, int32_t* idx, int batch, int nq, int nsrc, void* stream) {
  if (!query_xyz || !src_xyz || !idx || batch <= 0 || nq <= 0 || nsrc < 32 || nsrc > 8192) return POEM_E_ARG;
  HIPCHK(poem_launch_knn(query_xyz, src_xyz, idx, batch, nq, nsrc, 0, (hipStream_t)stream));
  return POEM_OK;
}

int poem_knn_ex(const float* query_xyz, const float* src_xyz, int32_t* idx, int batch, int nq, int nsrc, int fma_contract,
                void* stream) {
  if (!query_xyz || !src_xyz || !idx || batch <= 0 || nq <= 0 || nsrc < 32 || nsrc > 8192 || (fma_contract & ~1)) return POEM_E_ARG;
  HIPCHK(poem_launch_knn(query_xyz, src_xyz, idx, batch, nq, nsrc, fma_contract, (hipStream_t)stream));
  return POEM_OK;
}

int poem_knn_k(const float* query_xyz, const float* src_xyz, int32_t* idx, int batch, int nq, int nsrc, int k, int ld,
               int fma_contract, void* stream) {
  if (!query_xyz || !src_xyz || !idx || batch <= 0 || nq <= 0 || nsrc < 1 || nsrc > 8192 || k < 1 || k > 64 || k > nsrc ||
      ld < k || (fma_contract & ~1))
    return POEM_E_ARG;
  HIPCHK(poem_launch_knn_k(query_xyz, src_xyz, idx, batch, nq, nsrc, k, ld, fma_contract, (hipStream_t)stream));
  return POEM_OK;
}

int poem_vector_attention_k(const float* query_xyz, const float* src_xyz, const int32_t* idx, int k, int ld, const float* q,
                            const float* key, const float* v, int nsrc, const float* wd1, const float* bd1,
                            const void* wd2_packed, const float* bd2, const void* wg1_packed, const float* bg1,
                            const void* wg2_packed, const float* bg2, float* out, int batch, int nq, int embed, void* stream) {
  if (!query_xyz || !src_xyz || !idx || !q || !key || !v || !wd1 || !bd1 || !wd2_packed || !bd2 || !wg1_packed || !bg1 ||
      !wg2_packed || !bg2 || !out || batch <= 0 || nq <= 0 || nsrc <= 0 || k < 1 || k > 64 || ld < k)
    return POEM_E_ARG;
  HIPCHK(poem_launch_vector_attention_k(query_xyz, src_xyz, idx, k, ld, q, key, v, nsrc, wd1, bd1, wd2_packed, bd2, wg1_packed, bg1,
                                        wg2_packed, bg2, out, batch, nq, embed, embed, embed, embed, 0, (hipStream_t)stream));
  return POEM_OK;
}

int poem_vector_attention(const float* query_xyz, const float* src_xyz, const float* anchor_xyz, const int32_t* idx,
                          int shared_idx, const float* q, const float* k, const float* v, int nsrc, const float* wd1,
                          const float* bd1, const void* wd2_packed, const float* bd2, const void* wg1_packed,
                          const float* bg1, const void* wg2_packed, const float* bg2, float* out, int batch, int nq,
                          int embed, void* stream) {
  if (!query_xyz || (!src_xyz && !anchor_xyz) || !idx || !q || !k || !v || !wd1 || !bd1 || !wd2_packed || !bd2 ||
      !wg1_packed || !bg1 || !wg2_packed || !bg2 || !out || batch <= 0 || nq <= 0)
    return POEM_E_ARG;
  HIPCHK(poem_launch_vector_attention(query_xyz, src_xyz, anchor_xyz, idx, shared_idx, q, k, v, nsrc, wd1, bd1, wd2_packed,
                                      bd2, wg1_packed, bg1, wg2_packed, bg2, out, batch, nq, embed, embed, embed, embed, 0,
                                      (hipStream_t)stream));
  return POEM_OK;
}

int poem_reg_update(const float* r, const float* w, const float* b, const float* xyz_in, float* xyz_out, int rows,
                    int embed, void* stream) {
  if (!r || !w || !b || !xyz_in || !xyz_out || rows <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_narrow_linear(r, embed, w, b, xyz_in, xyz_out, rows, embed, 3, (hipStream_t)stream));
  return POEM_OK;
}

int poem_triangulate_dlt(const float* uv, const float* cam_intr, const float* cam_mat, const int32_t* view_offsets,
                         int batch, int njoints, int invert, float* out_xyz, void* stream) {
  if (!uv || !cam_intr || !cam_mat || !view_offsets || !out_xyz || batch <= 0 || njoints <= 0 || (invert & ~1))
    return POEM_E_ARG;
  if ((int64_t)batch * njoints > INT32_MAX) return POEM_E_UNSUPPORTED;    // the launcher and the kernel index (sample, joint) in int
  HIPCHK(poem_launch_dlt(uv, cam_intr, cam_mat, view_offsets, out_xyz, batch, njoints, invert, (hipStream_t)stream));
  return POEM_OK;
}

int poem_heatmap_uv(const float* heatmaps, float* uv, int views, int njoints, int hm_h, int hm_w, float img_w, float img_h,
                    void* stream) {
  if (!heatmaps || !uv || views <= 0 || njoints <= 0 || hm_h <= 0 || hm_w <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_heatmap_uv(heatmaps, uv, views * njoints, hm_h, hm_w, img_w, img_h, (hipStream_t)stream));
  return POEM_OK;
}

int poem_heatmap_uv_conf(const float* heatmaps, float* uv, float* conf, int views, int njoints, int hm_h, int hm_w, float img_w,
                         float img_h, void* stream) {
  if (!heatmaps || !uv || !conf || views <= 0 || njoints <= 0 || hm_h <= 0 || hm_w <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_heatmap_uv_conf(heatmaps, uv, conf, views * njoints, hm_h, hm_w, img_w, img_h, (hipStream_t)stream));
  return POEM_OK;
}

int poem_dlt_confidence(const float* uv, const float* conf, const float* cam_intr, const float* cam_mat,
                        const int32_t* view_offsets, float* out_xyz, int32_t* sel_count, int batch, int njoints, int invert,
                        int mode, double threshold, void* stream) {
  if (!uv || !conf || !cam_intr || !cam_mat || !view_offsets || !out_xyz || batch <= 0 || njoints <= 0 || njoints > 4096 ||
      (invert & ~1) || (mode != POEM_DLT_THRESHOLD && mode != POEM_DLT_WEIGHTED))
    return POEM_E_ARG;
  // the lowering loop runs (threshold / 0.05) times at most; an infinite or absurd threshold would never get there
  if (mode == POEM_DLT_THRESHOLD && !(threshold <= 64.0)) return POEM_E_ARG;
  if ((int64_t)batch * njoints > INT32_MAX) return POEM_E_UNSUPPORTED;    // one limit for both triangulation entry points
  HIPCHK(poem_launch_dlt_confidence(uv, conf, cam_intr, cam_mat, view_offsets, out_xyz, sel_count, batch, njoints, invert, mode,
                                    threshold, (hipStream_t)stream));
  return POEM_OK;
}

int poem_dlt_robust(const float* uv, const float* cam_intr, const float* cam_mat, const int32_t* view_offsets, float* out_xyz,
                    uint8_t* inlier, int32_t* inlier_count, float* reproj_px, int batch, int njoints, int invert,
                    double inlier_px, int refine, void* stream) {
  if (!uv || !cam_intr || !cam_mat || !view_offsets || !out_xyz || batch <= 0 || njoints <= 0 || njoints > 4096 || (invert & ~1))
    return POEM_E_ARG;
  if (!(inlier_px > 0.0) || refine < 0 || refine > 16) return POEM_E_ARG;  // (NaN refused; +inf: every view in front of the point)
  if ((int64_t)batch * njoints > INT32_MAX) return POEM_E_ARG;             // the kernel indexes (sample, joint) in int
  HIPCHK(poem_launch_dlt_robust(uv, cam_intr, cam_mat, view_offsets, out_xyz, inlier, inlier_count, reproj_px, batch, njoints,
                                invert, inlier_px, refine, (hipStream_t)stream));
  return POEM_OK;
}

size_t poem_conv3x3_packed_bytes(int cout, int cin) {
  if (cout <= 0 || cin <= 0 || cin % 8) return 0;
  return poem_conv3x3_packed_floats(cout, cin) * sizeof(float);
}

int poem_pack_conv3x3(const float* w_oihw, int cout, int cin, void* packed, void* stream) {
  if (!w_oihw || !packed || cout <= 0 || cin <= 0 || cin % 8) return POEM_E_ARG;
  HIPCHK(poem_launch_pack_conv3x3(w_oihw, cout, cin, packed, (hipStream_t)stream));
  return POEM_OK;
}

int poem_conv3x3(const float* in_padded, const void* w_packed, const float* scale, const float* shift,
                 const float* residual, float* out, int views, int cin, int cout, int h, int w, int stride, int relu,
                 int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset, void* stream) {
  if (!in_padded || !w_packed || !scale || !shift || !out || views <= 0 || cin <= 0 || cin % 8 || cout <= 0) return POEM_E_ARG;
  if ((stride != 1 && stride != 2) || h <= 0 || w <= 0 || h % stride || w % stride || ((h / stride) * (w / stride)) % 32)
    return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_conv3x3(in_padded, w_packed, scale, shift, residual, out, views, cin, cout, h, w, stride, relu,
                             ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset), (hipStream_t)stream));
  return POEM_OK;
}

// an (h, w) map stays inside the view's c * cs floats for every channel: a plain map or the interior of a bordered one (the
// kernels read the input through a per-view buffer descriptor of that size)
static bool map_ok(const ConvMap& m, int h, int w) {
  return m.ns >= 0 && m.cs > 0 && m.rs >= w && m.off >= 0 && (int64_t)(h - 1) * m.rs + (w - 1) + m.off < (int64_t)m.cs;
}

int poem_conv3x3_ex(const float* in_padded, const void* w_packed, const float* scale, const float* shift, const float* residual,
                    int64_t res_view_stride, int res_ch_stride, int res_row_stride, int res_offset, int res_before_act, float* out,
                    int views, int cin, int cout, int h, int w, int stride, int relu, int64_t out_view_stride, int out_ch_stride,
                    int out_row_stride, int out_offset, void* stream) {
  if (!in_padded || !w_packed || !scale || !shift || !out || views <= 0 || cin <= 0 || cin % 8 || cout <= 0) return POEM_E_ARG;
  if ((stride != 1 && stride != 2) || h <= 0 || w <= 0 || h % stride || w % stride || ((h / stride) * (w / stride)) % 32)
    return POEM_E_UNSUPPORTED;
  if ((uint64_t)cin * (uint64_t)(h + 2) * (uint64_t)(w + 2) * 4 >= (1ull << 31)) return POEM_E_UNSUPPORTED;
  const ConvMap rmap((long)res_view_stride, res_ch_stride, res_row_stride, res_offset);
  const ConvMap omap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset);
  if (residual && !map_ok(rmap, h / stride, w / stride)) return POEM_E_ARG;
  if (!map_ok(omap, h / stride, w / stride)) return POEM_E_ARG;
  HIPCHK(poem_launch_conv3x3_ex(in_padded, w_packed, scale, shift, residual, rmap, res_before_act, out, views, cin, cout, h, w, stride,
                                relu, omap, (hipStream_t)stream));
  return POEM_OK;
}

size_t poem_conv1x1_packed_bytes(int cout, int cin) {
  if (cout <= 0 || cin <= 0 || cin % 8) return 0;
  return poem_conv1x1_packed_floats(cout, cin) * sizeof(float);
}

int poem_pack_conv1x1(const float* w_oi, int cout, int cin, void* packed, void* stream) {
  if (!w_oi || !packed || cout <= 0 || cin <= 0 || cin % 8) return POEM_E_ARG;
  HIPCHK(poem_launch_pack_conv1x1(w_oi, cout, cin, packed, (hipStream_t)stream));
  return POEM_OK;
}

int poem_conv1x1(const float* in, int64_t in_view_stride, int in_ch_stride, int in_row_stride, int in_offset, const void* w_packed,
                 const float* shift, const float* residual, int64_t res_view_stride, int res_ch_stride, int res_row_stride,
                 int res_offset, float* out, int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset,
                 int views, int cin, int cout, int h, int w, int relu, void* stream) {
  if (!in || !w_packed || !out || views <= 0 || cin <= 0 || cin % 8 || cout <= 0) return POEM_E_ARG;
  if (h <= 0 || w <= 0 || ((int64_t)h * w) % 32 || (int64_t)h * w >= (1ll << 29)) return POEM_E_UNSUPPORTED;
  const Conv1Args a{in, (const float4*)w_packed, shift, residual, out,
                    ConvMap((long)in_view_stride, in_ch_stride, in_row_stride, in_offset),
                    ConvMap((long)res_view_stride, res_ch_stride, res_row_stride, res_offset),
                    ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset), cin, cout, h, w, relu, views};
  if (!map_ok(a.imap, h, w)) return POEM_E_ARG;
  if ((uint64_t)cin * (uint64_t)in_ch_stride * 4 >= (1ull << 31)) return POEM_E_UNSUPPORTED;
  if (residual && !map_ok(a.rmap, h, w)) return POEM_E_ARG;
  if (!map_ok(a.omap, h, w)) return POEM_E_ARG;
  HIPCHK(poem_launch_conv1x1_nchw(&a, (hipStream_t)stream));
  return POEM_OK;
}

int poem_hrnet_fuse(const poem_fuse_term_t* terms, int nterms, float* out, int64_t out_view_stride, int out_ch_stride,
                    int out_row_stride, int out_offset, int views, int channels, int h, int w, void* stream) {
  if (!terms || !out || nterms < 2 || nterms > 4 || views <= 0 || channels <= 0 || h <= 0 || w <= 0) return POEM_E_ARG;
  FuseArgs a{};
  a.nterms = nterms;
  a.out = out;
  a.omap = ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset);
  a.C = channels; a.H = h; a.W = w; a.views = views;
  if (!map_ok(a.omap, h, w)) return POEM_E_ARG;
  for (int k = 0; k < nterms; ++k) {
    const poem_fuse_term_t& t = terms[k];
    if (!t.data || t.shift < 0 || t.shift > 3) return POEM_E_ARG;
    a.t[k] = FuseTerm{t.data, ConvMap((long)t.view_stride, t.ch_stride, t.row_stride, t.offset), t.shift};
    if (!map_ok(a.t[k].map, ((h - 1) >> t.shift) + 1, ((w - 1) >> t.shift) + 1)) return POEM_E_ARG;
  }
  if ((int64_t)views * channels * h * w > (int64_t)0x7fffffff * 256) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_hrnet_fuse(&a, (hipStream_t)stream));
  return POEM_OK;
}

// ---- ResNet-18/34/50 and the non-HRNet decode branch (csrc/resnet.hip) ----------------------------------------------------
size_t poem_conv7x7_packed_bytes(int cout) {
  if (cout <= 0) return 0;
  return poem_conv7x7_packed_floats(cout) * sizeof(float);
}

int poem_pack_conv7x7(const float* w_oihw, int cout, void* packed, void* stream) {
  if (!w_oihw || !packed || cout <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_pack_conv7x7(w_oihw, cout, packed, (hipStream_t)stream));
  return POEM_OK;
}

// (H/2) x (W/2) output pixels in whole 32-pixel tiles
static bool half_tiles(int h, int w) { return h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && ((int64_t)(h / 2) * (w / 2)) % 32 == 0; }

int poem_conv7x7_s2(const float* in, const void* w_packed, const float* scale, const float* shift, float* out,
                    int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset, int views, int cout, int h, int w,
                    void* stream) {
  if (!in || !w_packed || !scale || !shift || !out || views <= 0 || cout <= 0) return POEM_E_ARG;
  if (!half_tiles(h, w) || cout % 32 || (uint64_t)3 * (uint64_t)h * (uint64_t)w * 4 >= (1ull << 31)) return POEM_E_UNSUPPORTED;
  const StemArgs a{in, (const float4*)w_packed, scale, shift, out,
                   ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset), cout, h, w, views};
  if (!map_ok(a.omap, h / 2, w / 2)) return POEM_E_ARG;
  HIPCHK(poem_launch_conv7x7_s2(&a, (hipStream_t)stream));
  return POEM_OK;
}

int poem_maxpool3x3_s2(const float* in, int64_t in_view_stride, int in_ch_stride, int in_row_stride, int in_offset, float* out,
                       int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset, int views, int channels, int h,
                       int w, void* stream) {
  if (!in || !out || views <= 0 || channels <= 0) return POEM_E_ARG;
  if (h <= 0 || w <= 0 || h % 2 || w % 2) return POEM_E_UNSUPPORTED;
  const PoolArgs a{in, out, ConvMap((long)in_view_stride, in_ch_stride, in_row_stride, in_offset),
                   ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset), channels, h, w, views};
  if (!map_ok(a.imap, h, w)) return POEM_E_ARG;
  if (!map_ok(a.omap, h / 2, w / 2)) return POEM_E_ARG;
  if ((int64_t)views * channels * (h / 2) * (w / 2) > (int64_t)0x7fffffff * 256) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_maxpool3x3_s2(&a, (hipStream_t)stream));
  return POEM_OK;
}

int poem_conv1x1_s2(const float* in, int64_t in_view_stride, int in_ch_stride, int in_row_stride, int in_offset, const void* w_packed,
                    const float* shift, float* out, int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset,
                    int views, int cin, int cout, int h, int w, void* stream) {
  if (!in || !w_packed || !out || views <= 0 || cin <= 0 || cin % 8 || cout <= 0) return POEM_E_ARG;
  if (!half_tiles(h, w)) return POEM_E_UNSUPPORTED;
  const SConvArgs a{in, (const float4*)w_packed, shift, out, ConvMap((long)in_view_stride, in_ch_stride, in_row_stride, in_offset),
                    ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset), cin, cout, h, w, 0, 0, views};
  if (!map_ok(a.imap, h, w)) return POEM_E_ARG;
  if (!map_ok(a.omap, h / 2, w / 2)) return POEM_E_ARG;
  HIPCHK(poem_launch_sconv1x1(&a, (hipStream_t)stream));
  return POEM_OK;
}

int poem_upsample2_concat_pad_staged(const float* a, int ca, const float* b, int cb, float* out, int views, int h, int w, void* stream) {
  if (!out || views <= 0 || ca < 0 || cb < 0 || ca + cb <= 0 || (ca && !a) || (cb && !b) || h <= 0 || w <= 0) return POEM_E_ARG;
  if (ca && (h % 2 || w % 2)) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_upcat_pad_staged(a, ca, b, cb, out, views, h, w, (hipStream_t)stream));
  return POEM_OK;
}

int poem_maxpool2_conv1x1(const float* x, const void* w_packed, const float* bias, float* out, int views, int cin, int cout, int h,
                          int w, int act, void* stream) {
  if (!x || !w_packed || !bias || !out || views <= 0 || cin <= 0 || cin % 8 || cout <= 0 || act < 0 || act > 1) return POEM_E_ARG;
  if (!half_tiles(h, w) || (int64_t)h * w >= (1ll << 31)) return POEM_E_UNSUPPORTED;
  const SConvArgs a{x, (const float4*)w_packed, bias, out, ConvMap(cin, h, w), ConvMap(cout, h / 2, w / 2), cin, cout, h, w, 1, act, views};
  HIPCHK(poem_launch_sconv1x1(&a, (hipStream_t)stream));
  return POEM_OK;
}

int poem_conv3x3_down2(const float* in, const void* w_packed, const float* scale, const float* shift, const float* residual,
                       float* out, int views, int cin, int cout, int h, int w, int relu, int64_t out_view_stride,
                       int out_ch_stride, int out_row_stride, int out_offset, void* stream) {
  if (!in || !w_packed || !scale || !shift || !out || views <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return POEM_E_ARG;
  const hipError_t e = poem_launch_conv3x3_down2(in, w_packed, scale, shift, residual, out, views, cin, cout, h, w, relu,
                                                 ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset),
                                                 (hipStream_t)stream);
  if (e == hipErrorNotSupported) return POEM_E_UNSUPPORTED;
  HIPCHK(e);
  return POEM_OK;
}

int poem_upcat_conv3x3(const float* a_half, int ca, const float* b_full, int cb, const void* w_packed, const float* scale,
                       const float* shift, float* out, int views, int cout, int h, int w, int relu, int64_t out_view_stride,
                       int out_ch_stride, int out_row_stride, int out_offset, void* stream) {
  if ((!a_half && ca) || (!b_full && cb) || !w_packed || !scale || !shift || !out || views <= 0 || cout <= 0 || h <= 0 || w <= 0)
    return POEM_E_ARG;
  const hipError_t e = poem_launch_upcat_conv3x3(a_half, ca, b_full, cb, w_packed, scale, shift, out, views, cout, h, w, relu,
                                                 ConvMap((long)out_view_stride, out_ch_stride, out_row_stride, out_offset),
                                                 (hipStream_t)stream);
  if (e == hipErrorNotSupported) return POEM_E_UNSUPPORTED;
  HIPCHK(e);
  return POEM_OK;
}

int poem_upcat_conv3x3_pool_head(const float* a_half, int ca, const float* b_full, int cb, const void* w_packed, const float* scale,
                                 const float* shift, const float* head_w, const float* head_b, float* heatmaps, int views, int cout,
                                 int j, int h, int w, int relu, void* stream) {
  if (!a_half || !b_full || !w_packed || !scale || !shift || !head_w || !head_b || !heatmaps || views <= 0 || cout <= 0 || j <= 0 ||
      h <= 0 || w <= 0 || ca <= 0 || cb <= 0)
    return POEM_E_ARG;
  const hipError_t e = poem_launch_upcat_conv3x3_pool_head(a_half, ca, b_full, cb, w_packed, scale, shift, head_w, head_b, heatmaps, views,
                                                           cout, j, h, w, relu, (hipStream_t)stream);
  if (e == hipErrorNotSupported) return POEM_E_UNSUPPORTED;
  HIPCHK(e);
  return POEM_OK;
}

int poem_set_decode_option(const char* name, int value) {
  if (!name) return POEM_E_ARG;
  if (!strcmp(name, "s2_staging_wave")) { poem_decode_s2_staging_wave(value); return POEM_OK; }
  if (!strcmp(name, "row_stager")) { if (value < 0 || value > 3) return POEM_E_ARG; poem_decode_row_stager(value); return POEM_OK; }
  if (!strcmp(name, "pin32")) { poem_decode_pin32(value); return POEM_OK; }
  if (!strcmp(name, "pool_fused")) { poem_decode_pool_fused(value); return POEM_OK; }
  return POEM_E_ARG;
}

int poem_conv1x1_upsample2(const float* in, const void* w_packed, const float* bias, float* out, int views, int cin, int cout,
                           int h, int w, void* stream) {
  if (!in || !w_packed || !out || views <= 0 || cin <= 0 || cout <= 0 || h <= 0 || w <= 0) return POEM_E_ARG;
  const hipError_t e = poem_launch_conv1x1_up2(in, w_packed, bias, out, views, cin, cout, h, w, (hipStream_t)stream);
  if (e == hipErrorNotSupported) return POEM_E_UNSUPPORTED;
  HIPCHK(e);
  return POEM_OK;
}

int poem_upsample2_concat_pad(const float* a, int ca, const float* b, int cb, float* out, int views, int h, int w, int pad,
                              void* stream) {
  if (!out || views <= 0 || ca < 0 || cb < 0 || ca + cb <= 0 || (ca && !a) || (cb && !b) || h <= 0 || w <= 0) return POEM_E_ARG;
  if (pad < 0 || pad > 1 || (ca && (h % 2 || w % 2))) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_upcat_pad(a, ca, b, cb, out, views, h, w, pad, (hipStream_t)stream));
  return POEM_OK;
}

int poem_pool_conv1x1_sigmoid(const float* x, const float* w, const float* bias, float* heatmaps, int views, int c, int j,
                              int h, int w_, void* stream) {
  if (!x || !w || !bias || !heatmaps || views <= 0 || c <= 0 || j <= 0) return POEM_E_ARG;
  if (c > 64 || j > 32 || h % 2 || w_ % 2) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_pool_head(x, w, bias, heatmaps, views, c, j, h, w_, (hipStream_t)stream));
  return POEM_OK;
}

int poem_pa_epe(const float* pred, const float* gt, float* out, int batch, int npoints, void* stream) {
  if (!pred || !gt || !out || batch <= 0 || npoints < 3) return POEM_E_ARG;
  HIPCHK(poem_launch_pa_epe(pred, gt, out, batch, npoints, (hipStream_t)stream));
  return POEM_OK;
}

int poem_pck_accumulate(const float* pred, const float* gt, int batch, int npoints, double val_min, double val_max,
                        int steps, uint32_t* counts, double* dist_sum, uint32_t* n, float* dist_out, void* stream) {
  if (!pred || !gt || !counts || !dist_sum || !n || batch <= 0 || npoints <= 0 || steps <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_pck_accumulate(pred, gt, batch, npoints, val_min, val_max, steps, counts, dist_sum, n, dist_out,
                                    (hipStream_t)stream));
  return POEM_OK;
}

// ---- benchmark-protocol mesh scores (csrc/meshscore.hip) ---------------------------------------------------------------------------
int poem_pa_align(const float* pred, const float* gt, float* aligned, double* transform, int batch, int npoints, void* stream) {
  if (!pred || !gt || (!aligned && !transform) || batch <= 0 || npoints < 3 || ((uintptr_t)transform & 7)) return POEM_E_ARG;
  HIPCHK(poem_launch_pa_align(pred, gt, aligned, transform, batch, npoints, (hipStream_t)stream));
  return POEM_OK;
}

// workspace of a search that reduces: one double and nthr ints per launched block (sample, direction, chunk of query points)
size_t poem_nn_distance_workspace_bytes(int batch, int na, int nb, int nthr) {
  if (batch <= 0 || na <= 0 || nb <= 0 || nthr < 0 || nthr > 8 || na > (1 << 24) || nb > (1 << 24)) return 0;
  const size_t slots = poem_nn_distance_slots(batch, na, nb);
  return (slots * (sizeof(double) + (size_t)nthr * sizeof(int32_t)) + 7) & ~(size_t)7;
}

int poem_nn_distance(const float* a, int na, const float* b, int nb, float* dist_ab, float* dist_ba, const double* thresholds,
                     int nthr, int32_t* counts, double* sums, void* workspace, size_t workspace_bytes, int batch, void* stream) {
  if (!a || !b || na <= 0 || nb <= 0 || batch <= 0 || nthr < 0) return POEM_E_ARG;
  if (!dist_ab && !dist_ba && !counts && !sums) return POEM_E_ARG;
  if (counts && (!thresholds || nthr <= 0)) return POEM_E_ARG;
  if (((uintptr_t)sums & 7) || ((uintptr_t)workspace & 7)) return POEM_E_ARG;
  if (na > (1 << 24) || nb > (1 << 24) || nthr > 8) return POEM_E_UNSUPPORTED;      // the renderer's limit on a point count
  if (thresholds)
    for (int k = 0; k < nthr; ++k)          // NaN, negative or not strictly ascending (`!(x >= 0)` is true of a NaN)
      if (!(thresholds[k] >= 0.0) || (k > 0 && !(thresholds[k] > thresholds[k - 1]))) return POEM_E_ARG;
  if (poem_nn_distance_slots(batch, na, nb) > 0x7fffffffu) return POEM_E_UNSUPPORTED;     // one block per slot: the grid's x limit
  if (counts || sums) {
    if (!workspace || workspace_bytes < poem_nn_distance_workspace_bytes(batch, na, nb, counts ? nthr : 0)) return POEM_E_WORKSPACE;
  }
  HIPCHK(poem_launch_nn_distance(a, na, b, nb, dist_ab, dist_ba, thresholds, counts ? nthr : 0, counts, sums, workspace, batch,
                                 (hipStream_t)stream));
  return POEM_OK;
}

int poem_mano_to_openpose(const float* j_regressor, const float* verts, float* joints, int batch, int nverts, void* stream) {
  if (!j_regressor || !verts || !joints || batch <= 0) return POEM_E_ARG;
  if (nverts != 778) return POEM_E_UNSUPPORTED;          // the tip vertex ids are MANO's
  HIPCHK(poem_launch_mano_to_openpose(j_regressor, verts, joints, batch, nverts, (hipStream_t)stream));
  return POEM_OK;
}

int poem_rot6d_to_axis_angle(const float* params, float* pose_aa, float* betas, int batch, void* stream) {
  if (!params || !pose_aa || !betas || batch <= 0) return POEM_E_ARG;
  HIPCHK(poem_launch_rot6d_to_aa(params, pose_aa, betas, batch, (hipStream_t)stream));
  return POEM_OK;
}

size_t poem_mano_table_bytes(void) { return poem_mano_table_floats_impl() * sizeof(float); }

int poem_mano_prepare(const float* v_template, const float* shapedirs, const float* posedirs, const float* j_regressor,
                      const float* weights, void* table, void* stream) {
  if (!v_template || !shapedirs || !posedirs || !j_regressor || !weights || !table) return POEM_E_ARG;
  HIPCHK(poem_launch_mano_prepare(v_template, shapedirs, posedirs, j_regressor, weights, (float*)table, (hipStream_t)stream));
  return POEM_OK;
}

int poem_mano_lbs(const float* pose_aa, const float* betas, const void* table, int batch, int center_idx, float* verts,
                  float* joints, void* stream) {
  if (!pose_aa || !betas || !table || !verts || !joints || batch <= 0 || batch > 65535 || center_idx < -1 || center_idx > 20)
    return POEM_E_ARG;
  HIPCHK(poem_launch_mano_lbs(pose_aa, betas, (const float*)table, verts, joints, batch, center_idx, (hipStream_t)stream));
  return POEM_OK;
}

size_t poem_mano_fit_workspace_bytes(int batch) {
  if (batch <= 0) return 0;
  return sizeof(double) * poem_mano_fit_workspace_doubles_impl(batch);
}

int poem_mano_fit(const void* table, const float* target_verts, const float* x0_or_null, int batch, int iters, float shape_reg,
                  float pose_reg, void* workspace, size_t workspace_bytes, float* pose_aa, float* betas, float* tsl, float* verts,
                  float* joints, double* cost, int32_t* accepted, int32_t* status, void* stream) {
  if (batch < 0 || iters < 0 || iters > 64) return POEM_E_ARG;
  if (!(shape_reg >= 0.f) || !(pose_reg >= 0.f) || !std::isfinite(shape_reg) || !std::isfinite(pose_reg)) return POEM_E_ARG;
  if (batch == 0) return POEM_OK;
  if (!table || !target_verts || !workspace || !pose_aa || !betas || !tsl || !verts || !joints || !cost || !accepted || !status)
    return POEM_E_ARG;
  if (batch > 65535) return POEM_E_UNSUPPORTED;                              // one grid row per sample
  if (((uintptr_t)workspace & 7u) != 0) return POEM_E_ARG;
  if (workspace_bytes < poem_mano_fit_workspace_bytes(batch)) return POEM_E_WORKSPACE;
  poem_mano_fit_terms_t terms = {};             // term M alone, weight 1: the same launches on the 49-slot workspace
  terms.target_verts = target_verts;
  terms.mesh_weight = 1.f;
  HIPCHK(poem_launch_mano_fit_terms((const float*)table, &terms, 0, x0_or_null, batch, iters, shape_reg, pose_reg, (double*)workspace,
                                    pose_aa, betas, tsl, verts, joints, cost, accepted, status, (hipStream_t)stream));
  return POEM_OK;
}

size_t poem_mano_fit_terms_workspace_bytes(int batch) {
  if (batch <= 0) return 0;
  return sizeof(double) * poem_mano_fit_terms_workspace_doubles_impl(batch);
}

int poem_mano_fit_terms(const void* table, const poem_mano_fit_terms_t* terms, const float* x0_or_null, int batch, int iters,
                        float shape_reg, float pose_reg, void* workspace, size_t workspace_bytes, float* pose_aa, float* betas,
                        float* tsl, float* verts, float* joints, double* cost, int32_t* accepted, int32_t* status, void* stream) {
  if (batch < 0 || iters < 0 || iters > 64 || !terms) return POEM_E_ARG;
  if (!(shape_reg >= 0.f) || !(pose_reg >= 0.f) || !std::isfinite(shape_reg) || !std::isfinite(pose_reg)) return POEM_E_ARG;
  const bool M = terms->target_verts != nullptr, J = terms->joints3d != nullptr, K = terms->keypoints != nullptr;
  if (!M && !J && !K) return POEM_E_ARG;
  if (M && (!(terms->mesh_weight >= 0.f) || !std::isfinite(terms->mesh_weight))) return POEM_E_ARG;
  if (J != (terms->joints3d_weight != nullptr)) return POEM_E_ARG;
  if (!K && terms->keypoint_weight) return POEM_E_ARG;
  if (K) {
    if (!terms->keypoint_weight || !terms->cam_intr || !terms->cam_extr || !terms->view_offsets || terms->total_views < 0)
      return POEM_E_ARG;
    if (!(terms->image_scale > 0.f) || !std::isfinite(terms->image_scale)) return POEM_E_ARG;
    if (!M && !J && !x0_or_null) return POEM_E_ARG;                            // keypoints alone give no start
  }
  if (batch == 0) return POEM_OK;
  if (!table || !workspace || !pose_aa || !betas || !tsl || !verts || !joints || !cost || !accepted || !status) return POEM_E_ARG;
  if (batch > 65535 || (K && terms->total_views > 65535)) return POEM_E_UNSUPPORTED;
  if (((uintptr_t)workspace & 7u) != 0) return POEM_E_ARG;
  if (workspace_bytes < poem_mano_fit_terms_workspace_bytes(batch)) return POEM_E_WORKSPACE;
  HIPCHK(poem_launch_mano_fit_terms((const float*)table, terms, 1, x0_or_null, batch, iters, shape_reg, pose_reg, (double*)workspace,
                                    pose_aa, betas, tsl, verts, joints, cost, accepted, status, (hipStream_t)stream));
  return POEM_OK;
}

int poem_warp_affine(const uint8_t* src, const int64_t* src_offsets, const int32_t* src_hw, const double* m_inv,
                     const double* gain, float* out_f32, uint8_t* out_u8, int views, int out_h, int out_w, void* stream) {
  if (!src || !src_offsets || !src_hw || !m_inv || (!out_f32 && !out_u8) || views <= 0 || out_h <= 0 || out_w <= 0)
    return POEM_E_ARG;
  if (views > 65535 || out_h > 4 * 65535) return POEM_E_UNSUPPORTED;      // grid y / z limits
  HIPCHK(poem_launch_warp_affine(src, (const long long*)src_offsets, src_hw, m_inv, gain, out_f32, out_u8, views, out_h,
                                 out_w, (hipStream_t)stream));
  return POEM_OK;
}

// ---- baseline JPEG (csrc/jpeg.hip; the host half, poem_jpeg_entropy_decode / poem_jpeg_reconstruct_host, is csrc/jpeg.cpp) --------
size_t poem_jpeg_workspace_bytes(int64_t total_blocks) { return total_blocks > 0 ? (size_t)total_blocks * 64 : 0; }

int poem_jpeg_reconstruct(const poem_jpeg_desc_t* descs, const int16_t* coef, int64_t coef_bytes, const int64_t* out_offsets,
                          uint8_t* out, int64_t out_bytes, int n, int64_t total_blocks, int64_t total_quads, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (!descs || !coef || !out_offsets || !out || n <= 0 || coef_bytes < 0 || out_bytes < 0 || total_blocks < 0 || total_quads < 0)
    return POEM_E_ARG;
  if (((uintptr_t)descs & 15) || ((uintptr_t)coef & 15) || ((uintptr_t)out_offsets & 7) || ((uintptr_t)workspace & 15)) return POEM_E_ARG;
  // at most 2^24 - 1 workgroups of 256 threads per launch: below 2^32 threads, what the runtime guarantees
  if (n > 65535 || total_blocks > (((int64_t)1 << 24) - 1) * 32 || total_quads > (((int64_t)1 << 24) - 1) * 256) return POEM_E_UNSUPPORTED;
  if (total_blocks == 0 && total_quads == 0) return POEM_OK;                 // no image taken: nothing to write
  if (total_blocks > 0 && (!workspace || workspace_bytes < poem_jpeg_workspace_bytes(total_blocks))) return POEM_E_WORKSPACE;
  HIPCHK(poem_launch_jpeg_reconstruct(descs, coef, coef_bytes, (const long long*)out_offsets, out, out_bytes, n, total_blocks,
                                      total_quads, (unsigned char*)workspace, (hipStream_t)stream));
  return POEM_OK;
}

// ---- Huffman decoding on the device (csrc/jpeg_entropy.hip; the host half, poem_jpeg_entropy_prepare / _parallel_host, is jpeg.cpp) ---
size_t poem_jpeg_entropy_workspace_bytes(int n, int64_t total_subs) { return poem_jpeg_entropy_ws_bytes(n, total_subs); }

int poem_jpeg_entropy_device(poem_jpeg_desc_t* descs, const poem_jpeg_scan_t* scans, const poem_jpeg_huff_t* tables,
                             int64_t table_count, const uint8_t* packed, int64_t packed_bytes, int n, int subseq, int wg_threads,
                             int64_t total_subs, int64_t total_blocks, int16_t* coef, int64_t coef_bytes, int32_t* status,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (!descs || !scans || !tables || !packed || !coef || !status || n <= 0 || table_count < 0 || packed_bytes < 0 || total_subs < 0 ||
      total_blocks < 0 || coef_bytes < 0)
    return POEM_E_ARG;
  if (subseq == 0) subseq = 64;                                  // the defaults: the best of the shapes measured (LABNOTES)
  if (wg_threads == 0) wg_threads = 1024;
  if (subseq < 16 || subseq > 1024 || (subseq & (subseq - 1)) || wg_threads < 64 || wg_threads > 1024 || (wg_threads & 63)) return POEM_E_ARG;
  if (((uintptr_t)descs & 15) || ((uintptr_t)scans & 7) || ((uintptr_t)tables & 3) || ((uintptr_t)packed & 15) || ((uintptr_t)coef & 15) ||
      ((uintptr_t)status & 3) || ((uintptr_t)workspace & 15))
    return POEM_E_ARG;
  if (n > 65535 || total_blocks > (((int64_t)1 << 24) - 1) * 32) return POEM_E_UNSUPPORTED;
  if (!workspace || workspace_bytes < poem_jpeg_entropy_workspace_bytes(n, total_subs)) return POEM_E_WORKSPACE;
  HIPCHK(poem_launch_jpeg_entropy(descs, scans, tables, table_count, packed, packed_bytes, n, subseq, wg_threads, total_subs, total_blocks,
                                  coef, coef_bytes, status, workspace, (hipStream_t)stream));
  return POEM_OK;
}

// ---- mesh rendering (csrc/render.hip) ------------------------------------------------------------------------------------------
// workspace of a render: six floats per (mesh, view, vertex) -- linear in the view count, so that the number of views a workspace
// holds can be read back from its size (the view count itself, view_offsets[batch], lives on the device)
static size_t render_bytes_per_view(int nverts, int nmeshes) { return (size_t)24 * (size_t)nverts * (size_t)nmeshes; }

size_t poem_render_workspace_bytes(int total_views, int nverts, int nmeshes) {
  if (total_views <= 0 || nverts <= 0 || nmeshes <= 0) return 0;
  return (size_t)total_views * render_bytes_per_view(nverts, nmeshes);
}

int poem_render_mesh(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces, const float* cam_intr,
                     const float* cam_extr, const int32_t* view_offsets, const uint8_t* background, const float* lights, int nlights,
                     const float* albedo, float near_z, uint8_t* rgb, float* depth, int32_t* face_id, int nmeshes, int batch, int nverts,
                     int nfaces, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!verts || !faces || !vf_offsets || !vf_faces || !cam_intr || !cam_extr || !view_offsets || !lights || !albedo || !rgb || !workspace ||
      nmeshes <= 0 || batch <= 0 || nverts <= 0 || nfaces <= 0 || h <= 0 || w <= 0 || nlights < 0 || !(near_z > 0.f) ||
      ((uintptr_t)workspace & 7))
    return POEM_E_ARG;
  if (nlights > 8 || h > 16384 || w > 16384 || nmeshes > 65535 || nverts > (1 << 24) || nfaces > (1 << 24)) return POEM_E_UNSUPPORTED;
  const size_t per_view = render_bytes_per_view(nverts, nmeshes);
  const size_t cap = workspace_bytes / per_view;
  if (cap == 0) return POEM_E_WORKSPACE;
  const int view_cap = (int)(cap < 65535 ? cap : 65535);                 // grid y limit: at most 65535 views per call
  hipStream_t s = (hipStream_t)stream;
  float* vtx = (float*)workspace;
  HIPCHK(poem_launch_render_vertices(verts, faces, vf_offsets, vf_faces, cam_intr, cam_extr, view_offsets, lights, nlights, albedo, vtx, nullptr,
                                     nmeshes, batch, nverts, nfaces, view_cap, s));
  HIPCHK(poem_launch_render_raster(vtx, faces, view_offsets, background, rgb, depth, face_id, nmeshes, batch, nverts, nfaces, h, w, near_z,
                                   view_cap, s));
  return POEM_OK;
}

int poem_project_points(const float* points, const float* cam_intr, const float* cam_extr, const int32_t* view_offsets, float* uv, int batch,
                        int npoints, int total_views, void* stream) {
  if (!points || !cam_intr || !cam_extr || !view_offsets || !uv || batch <= 0 || npoints <= 0 || total_views <= 0 || ((uintptr_t)uv & 7))
    return POEM_E_ARG;
  if (total_views > 65535 || npoints > (1 << 24)) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_render_vertices(points, nullptr, nullptr, nullptr, cam_intr, cam_extr, view_offsets, nullptr, 0, nullptr, nullptr, uv, 1,
                                     batch, npoints, 0, total_views, (hipStream_t)stream));
  return POEM_OK;
}

int poem_draw_skeleton(const uint8_t* image, const float* joints_uv, const float* colours, uint8_t* out, int views, int h, int w,
                       void* stream) {
  if (!image || !joints_uv || !colours || !out || views <= 0 || h <= 0 || w <= 0) return POEM_E_ARG;
  if (views > 65535 || h > 16384 || w > 16384) return POEM_E_UNSUPPORTED;
  HIPCHK(poem_launch_skeleton(image, joints_uv, colours, out, views, h, w, (hipStream_t)stream));
  return POEM_OK;
}

// ---- loss terms (csrc/loss.hip) --------------------------------------------------------------------------------------------------
// workspace: one double per (block, slot) -- sized for the widest grid (vertices projected), whatever the configuration of a call
size_t poem_loss_workspace_bytes(int batch, int total_views) {
  if (batch <= 0 || total_views <= 0) return 0;
  return sizeof(double) * ((size_t)total_views * LOSS_VIEW_GROUPS * LOSS_VIEW_SLOTS + (size_t)batch * LOSS_SAMPLE_SLOTS);
}

int poem_loss_terms(const float* coords, const float* pred_joints_uv, const float* pred_pose, const float* pred_shape,
                    const float* master_joints_3d, const float* master_verts_3d, const float* target_joints_2d, const float* cam_intr,
                    const float* cam_extr, const int32_t* view_offsets, const float* mano_pose, const float* mano_shape,
                    const float* j_regressor, const poem_loss_cfg_t* cfg, int batch, int total_views, double* out, void* workspace,
                    size_t workspace_bytes, void* stream) {
  static_assert(POEM_LOSS_NTERMS == LOSS_NTERMS, "include/poem_hip.h and csrc/loss.h disagree on the result's layout");
  // a NULL j_regressor is an error, not a skipped term: upstream always adds the from-mesh joints to loss_recon
  if (!coords || !pred_joints_uv || !master_joints_3d || !master_verts_3d || !target_joints_2d || !cam_intr || !cam_extr || !view_offsets ||
      !j_regressor || !cfg || !out || !workspace || batch <= 0 || total_views <= 0 || batch > total_views ||
      ((uintptr_t)out & 7) || ((uintptr_t)workspace & 7))
    return POEM_E_ARG;
  if (cfg->parametric && (!pred_pose || !pred_shape || !mano_pose || !mano_shape)) return POEM_E_ARG;
  if (cfg->center_idx < 0 || cfg->center_idx > 20 || cfg->img_h <= 0 || cfg->img_w <= 0) return POEM_E_ARG;
  if (total_views > 65535) return POEM_E_UNSUPPORTED;                       // the renderer's limit on a ragged batch
  if (workspace_bytes < poem_loss_workspace_bytes(batch, total_views)) return POEM_E_WORKSPACE;
  LossArgs a{};
  a.coords = coords, a.pred_uv = pred_joints_uv, a.pred_pose = pred_pose, a.pred_shape = pred_shape;
  a.gt_joints = master_joints_3d, a.gt_verts = master_verts_3d, a.gt_uv = target_joints_2d;
  a.intr = cam_intr, a.extr = cam_extr, a.view_offsets = view_offsets;
  a.mano_pose = mano_pose, a.mano_shape = mano_shape, a.jreg = j_regressor;
  a.w_joints = cfg->joints_weight, a.w_verts = cfg->vertices_weight, a.w_joints_2d = cfg->joints_2d_weight;
  a.w_verts_2d = cfg->vertices_2d_weight, a.w_heatmap = cfg->heatmap_joints_weight;
  a.w_pose = cfg->pose_weight, a.w_shape = cfg->shape_weight;
  a.img_scale = sqrt((double)cfg->img_w * (double)cfg->img_w + (double)cfg->img_h * (double)cfg->img_h);      // POEM.py:372
  a.joints_l2 = cfg->joints_l2 != 0, a.verts_l2 = cfg->vertices_l2 != 0, a.parametric = cfg->parametric != 0;
  a.center_idx = cfg->center_idx;
  a.B = batch, a.BN = total_views;
  a.view_groups = cfg->vertices_2d_weight != 0.0 ? LOSS_VIEW_GROUPS : 1;
  a.part = (double*)workspace, a.out = out;
  HIPCHK(poem_launch_loss_terms(&a, (hipStream_t)stream));
  return POEM_OK;
}
}  // extern "C"
