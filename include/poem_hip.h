/* poem_hip.h -- C ABI of the MI355X-native POEM-v2 point-embedded decoder (libpoem_hip.so).
 *
 * Plain pointers and sizes only; every pointer is a DEVICE pointer unless the name ends in _host.  All entry
 * points are stream-ordered, allocate nothing, never throw, and return 0 on success or a negative POEM_E_* code.
 * Tensors are fp32, row-major/contiguous; indices are int32.  hipStream_t is passed as void*.
 *
 * Threading contract.  The operator-level entry points are re-entrant: they keep no host state, and two host threads may
 * call them concurrently on different streams.  A handle (poem_create) is used by ONE host thread at a time (its side
 * streams, events and cached index upload are per handle; different handles on different threads -- one thread per GPU --
 * are independent).  The opt-in split-precision modes carry their per-call context in thread-local host state that only the
 * call which installed it clears, so a forward on one thread never changes the arithmetic of a forward on another.
 * poem_last_hip_error is per thread.
 *
 * What each entry point replaces in the upstream reference (paths relative to the reference root) -- the
 * reference has no FFI of its own (it is pure Python on torch / pytorch3d / transformers), so these are the
 * native calls its hot path makes today:
 *
 *   poem_gemm                 torch.nn.Linear forward: every Linear of the path
 *                             (lib/models/bricks/pt_metro_transformer.py:180-181 embedding, :88-91 FFN, :25,38
 *                             reg_branch; point_transformers.py:49-56,86-87,138-142 fc1/fc2/w_qs/w_ks/w_vs;
 *                             ptEmb_head.py:701-707 merge_net_feature; BertSelfAttention query/key/value,
 *                             BertSelfOutput.dense)
 *   poem_layernorm            BertSelfOutput.LayerNorm / BertOutput.LayerNorm (transformers, call sites
 *                             pt_metro_transformer.py:57-74,88-91)
 *   poem_input_proj           nn.Conv2d 1x1 input_proj + positional table add (ptEmb_head.py:835,853-870)
 *   poem_pe_table             SinePositionalEncoding3D + adapt_pos3d (petr_transformer.py:434-469,
 *                             ptEmb_head.py:857-858), constant-folded per view count
 *   poem_project_sample       generate_grid_sample_proj + F.grid_sample (lib/utils/collation.py:48-65,
 *                             lib/utils/transform.py:898-930, ptEmb_head.py:873-883,900-901)
 *   poem_merge_reduce /       merge_features_mv / merge_features_sv around the two merge MLPs, on the Q1
 *   poem_merge_finalize       re-interpreted rows (ptEmb_head.py:745-771,910-926)
 *   poem_cross_attention      BertSelfAttention scores/softmax/context for encoder_hidden_states
 *                             (pt_metro_transformer.py:57-72; transformers v4 semantics)
 *   poem_knn                  pytorch3d.ops.knn_points(K=32) (point_transformers.py:83,134)
 *   poem_vector_attention     ptTransformerBlock._forward / ptTransformerBlock_CrossAttn._forward from
 *                             fc_delta to the softmax-weighted sum (point_transformers.py:88-95,144-151)
 *   poem_reg_update           reg_branch second Linear + xyz residual (pt_metro_transformer.py:38)
 *   poem_triangulate_dlt      batch_triangulate_dlt_torch + the ragged per-sample loop (lib/utils/triangulation.py:5-45,
 *                             lib/models/POEM.py:284-299) -- the stage that produces reference_joints
 *   poem_dlt_confidence /     triangulate_dlt (lib/utils/triangulation.py:111-148): the same stage with views selected by a
 *   poem_heatmap_uv_conf      confidence threshold that drops until two are left, or weighted by confidence; the confidence
 *                             is the heat map's peak, read out next to the expectation
 *   poem_dlt_robust           (no upstream counterpart) the same stage with views that disagree with the geometry of the others
 *                             left out: exhaustive two-view hypotheses, inlier count, refit, optional Gauss-Newton refinement
 *   poem_conv3x3 /            ConvBlock (Conv2d 3x3 + BatchNorm(eval) + ReLU, lib/models/bricks/conv.py:4-45) and the glue
 *   poem_upsample2_concat_pad around it in PtEmbedMultiviewStereoV2.feat_decode / uv_decode (lib/models/POEM.py:167-211:
 *   poem_pool_conv1x1_sigmoid F.interpolate x2 + torch.cat, max_pool2d + uv_out + sigmoid); poem_heatmap_uv is the read-out of
 *   poem_heatmap_uv           heatmap_stage (POEM.py:213-222, integral_heatmap2d) -- the stage that produces the head's
 *                             mlvl_feat and the per-view 2-D joints
 *   poem_pa_epe /             PAEval.feed + align_w_scale (lib/metrics/pa_eval.py:45-83,104-124) and _PCKMetric.feed
 *   poem_pck_accumulate       (lib/metrics/pck.py:36-96) -- device-side evaluation metrics
 *   poem_pa_align /           align_w_scale (lib/metrics/pa_eval.py:104-124) with the aligned set kept, and the nearest-neighbour loop
 *   poem_nn_distance          of the FreiHAND / HO3D protocol scripts (no upstream code): mesh F@5 / F@15, aligned AUC
 *   poem_mano_to_openpose     mano_to_openpose (lib/utils/transform.py:836-872) -- joints from mesh for the metrics (N3)
 *   poem_warp_affine          cv2.warpAffine + colour jitter + to_tensor / normalize of SimpleTransform2D.__call__
 *                             (lib/utils/transform.py:153-170) and the mirror warp of process_data_item
 *                             (lib/data_wds/multiview_wds.py:112-118) -- the image side of the input pipeline
 *   poem_rot6d_to_axis_angle  rot6d_to_aa of get_parametric_output (pt_metro_transformer.py:144-146, lib/utils/transform.py:448-466)
 *   poem_mano_lbs             manotorch ManoLayer.forward (pt_metro_transformer.py:120-124,147-148; ptEmb_head.py:732-736,886-892)
 *   poem_mano_fit             MANO pose / shape / translation fitted to a mesh (upstream only offline: lib/fit/frame_fit/one_frame_fit.py)
 *   poem_mano_fit_terms       ... and to 3-D joint targets and 2-D keypoints in N calibrated views per sample (what upstream's fitter fits)
 *   poem_render_mesh /        DrawingHandCallback's mesh overlay and 2-D skeleton (lib/utils/testing.py:101-192 -> OpenDRRenderer,
 *   poem_draw_skeleton /      lib/viztools/opendr_renderer.py:11-206, and draw_2d_skeleton, lib/viztools/draw.py:234-336): upstream renders on
 *   poem_project_points       the host through OpenGL, one view at a time; batch_cam_extr_transf + batch_cam_intr_projection in front of it
 *   poem_loss_terms           PtEmbedMultiviewStereoV2.compute_loss + loss_proj_to_multicam (lib/models/POEM.py:336-466), forward only;
 *                             the sums LossMetric.feed (lib/metrics/basic_metric.py:63-97) reads with .item() stay on the device
 *   poem_head_forward         POEM_Generalized_Head.forward + PtEmbedTRv4.forward (ptEmb_head.py:825-964,
 *                             lib/models/layers/ptEmb_transformer.py:371-376)
 */
#ifndef POEM_HIP_H
#define POEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POEM_OK 0
#define POEM_E_ARG (-1)        /* bad argument (null pointer, unsupported size, misaligned) */
#define POEM_E_WORKSPACE (-2)  /* workspace too small */
#define POEM_E_LAUNCH (-3)     /* HIP launch/runtime error (see poem_last_hip_error) */
#define POEM_E_UNSUPPORTED (-4)

/* Size limits (the kernels address batch-scaled tensors through 32-bit buffer offsets; DESIGN.md "Offsets past 4 GiB"):
 *   cross attention   batch * nkp * embed * 4 < 2^31 with nkp = 32 * ceil(nk / 32), the keys a sample owns in the K / V
 *                     images (each image below 2 GiB): poem_cross_attention[_merged] return POEM_E_UNSUPPORTED beyond it;
 *                     poem_head_forward / poem_decoder_forward likewise for batch * SP * embed * 4 >= 2^31 with
 *                     SP = 32 * ceil(nsample / 32) -- POEM-huge (embed 1024, nsample 4096) up to batch 127, POEM-medium
 *                     (embed 256) up to 511; at nsample 8192 half of that.
 *   vector attention  SP * embed * 4 (one sample's v rows) below 2 GiB; any batch.
 *   GEMM              any M: rows past 4 GiB of x run the 64-bit-pointer kernel; poem_gemm_split returns POEM_E_UNSUPPORTED
 *                     once m * ldx * 4 passes 4 GiB. */

#define POEM_ACT_NONE 0
#define POEM_ACT_RELU 1
#define POEM_ACT_GELU 2 /* erf form */

typedef struct poem_config {
  int32_t embed;       /* C: EMBED_DIMS = POINTS_FEAT_DIM = INPUT_FEAT_DIM (32..1024, multiple of 32) */
  int32_t in_channels; /* IN_CHANNELS (160), multiple of 8 */
  int32_t nsample;     /* S: N_SAMPLE (4096).  Any count with max(knn, 1 + max(anchor_idx)) <= S <= 8192.  S % C != 0 (a row of
                          the Q1 re-interpretation straddles channel lines) takes the operator sampling front end instead of the
                          fused one; S % 32 != 0 pads a sample's basis-point rows behind the sampling stage to whole 32-key
                          tiles and runs the masked forms of the cross attention (fp32 precision only). */
  int32_t nquery;      /* Q: 799 */
  int32_t heads;       /* NUM_ATTENTION_HEADS (4) */
  int32_t nblocks;     /* N_BLOCKS (3) */
  int32_t knn;         /* N_NEIGHBOR (ptEmb_transformer.py:30), 1..64 and <= nsample, nquery; N_NEIGHBOR_QUERY (:31) is the same
                          unless poem_set_option(h, "knn_query", k) says otherwise.  The release configs set 32 for both; counts
                          below 32 run the masked vector attention (the search's first k of its 32 nearest); a count above 32
                          switches both neighbour buffers to rows of 64 and the K <= 64 search / two-tile attention.  Block 0
                          takes the 32 fixed anchors whatever the keys say (assets/anchor.npy, point_transformers.py:10-32). */
  int32_t parametric;  /* TRANSFORMER.PARAMETRIC_OUTPUT */
  int32_t feat_h, feat_w; /* backbone feature map (16x16) */
  int32_t max_views;   /* largest views-per-sample the positional table is folded for */
  float radius;        /* RADIUS_SAMPLE (0.1) */
  float ln_eps;        /* BertConfig.layer_norm_eps (1e-12) */
  /* ABI 2: the positional-encoding switches of the reference's constructor.  No release config changes them. */
  int32_t pe_normalize;   /* POSITIONAL_ENCODING.NORMALIZE (1; lib/models/layers/petr_transformer.py:451-457) */
  int32_t petr_embedding; /* PETR_EMBEDDING (0; lib/models/heads/ptEmb_head.py:692,865-867): position_encoder of the cameras'
                           * frustum points is added to the positional embedding; four more weight tensors, listed last */
  int32_t depth_num;      /* DEPTH_NUM (32); with petr_embedding: 3 * depth_num must be a multiple of 8 */
  int32_t lid;            /* LID (0): linear-increasing depth bins (ptEmb_head.py:122-126) */
  int32_t reserved0;
  double depth_start, depth_end; /* DEPTH_START, DEPTH_END (0.0, 1.2) -- doubles, as the reference's Python scalars are:      */
  double position_range[6];      /* POSITION_RANGE (xmin ymin zmin xmax ymax zmax); each is rounded to fp32 where the reference's
                                  * tensor-scalar arithmetic rounds it */
} poem_config_t;

typedef struct poem_handle_s* poem_handle_t;

/* ---- library ------------------------------------------------------------------------------------------ */
int poem_abi_version(void);
int poem_last_hip_error(void);            /* hipError_t of the last failing runtime call on this thread */
const char* poem_error_string(int code);

/* ---- weights ------------------------------------------------------------------------------------------- */
/* Number of raw tensors / their element counts in canonical order (the order of
 * poem_v2_amd.weights.live_key_shapes == the reference's state_dict order of the live tensors). */
int poem_num_weight_tensors(const poem_config_t* cfg);
int64_t poem_weight_tensor_numel(const poem_config_t* cfg, int index);
/* Bytes of the packed device image (MFMA-fragment order weights + folded tables) the handle keeps. */
size_t poem_packed_bytes(const poem_config_t* cfg);
/* raw: host array of `n` device pointers to the raw fp32 tensors in canonical order.
 * bps (S,3), anchor (32,3) fp32, anchor_idx (32) int32, template_xyz (Q,3) fp32 metres: device pointers.
 * packed: caller-owned device buffer of poem_packed_bytes(); must outlive the handle. */
int poem_create(const poem_config_t* cfg, const void* const* raw_host, int n, const float* bps, const float* anchor,
                const int32_t* anchor_idx, const float* template_xyz, void* packed, size_t packed_bytes,
                void* stream, poem_handle_t* out);
void poem_destroy(poem_handle_t h);

/* ---- whole path ---------------------------------------------------------------------------------------- */
/* Bytes of the caller-owned workspace of a forward of `batch` samples with `total_views` views in all.  Passing
 * total_views = batch * cfg.max_views (the worst case of the batch size) makes poem_head_forward lay the workspace out
 * for that capacity whatever the batch's own view counts are: every pointer of the forward is then a function of the batch
 * size alone and ONE captured launch graph per batch size serves every view layout (a stream of ragged batches, the
 * reference's collation_random_n_views, lib/utils/collation.py:7-25).  A workspace sized for the batch's own total works
 * too; its graph is then shared by the layouts with that total only. */
size_t poem_workspace_bytes(poem_handle_t h, int batch, int total_views);
/* Diagnostics of the launch-graph cache, n >= 9 slots: [0] graph execs cached by this handle, [1] stream captures,
 * [2] hipGraphInstantiate calls, [3] forwards replayed from a graph, [4] forwards issued as plain launches,
 * [5] view-layout uploads (a forward whose layout equals the previous one uploads nothing), [6] retired execs parked in the
 * process, [7] parked execs taken over by a later capture (hipGraphExecUpdate), [8] updates the runtime refused, [9] (n >= 10)
 * parked execs passed over because their last launch was still running.  Retired execs are never destroyed (a runtime
 * workaround, csrc/handle.cpp): they are parked per device and re-used, so [6] is bounded by the largest number of execs ever
 * cached at once per (device, shape) -- 12 per handle -- not by the handles created or layouts met; a server that cycles many
 * model shapes should watch [6].  A parked exec is offered for update only on its own device and only after the launch it
 * was retired behind has completed.
 * A forward never blocks the host: the layout travels in a kernel's argument segment. */
int poem_graph_stats(poem_handle_t h, int64_t* out, int n);
/* view_offsets_host: B+1 prefix sums of views per sample (host memory, the reference's cam_view_num).
 * cam_extr is camera->master (as in the reference's img_metas["cam_extr"]).
 * out_xyz: (nblocks, B, Q, 3) metres in the master frame (all_coords_preds).
 * Parametric configs: out_xyz holds the pre-MANO stack; pose_aa (B,48) and betas (B,10) are written and the caller
 * finishes with its MANO layer + poem_finalize_parametric. */
int poem_head_forward(poem_handle_t h, const float* mlvl_feat, const float* cam_intr, const float* cam_extr,
                      const int32_t* view_offsets_host, int batch, const float* reference_joints, int img_w,
                      int img_h, float* out_xyz, float* pose_aa, float* betas, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Decoder only (PtEmbedTRv4.forward, lib/models/layers/ptEmb_transformer.py:371-376): normalised inputs
 * query_xyz (B,Q,3), query_feat (B,Q,C), pt_xyz (B,S,3), pt_feats (B,S,C) -> out_xyz_norm (nblocks,B,Q,3). */
int poem_decoder_forward(poem_handle_t h, const float* query_xyz, const float* query_feat, const float* pt_xyz,
                         const float* pt_feats, int batch, float* out_xyz_norm, float* pose_aa, float* betas,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Stream overlap (default on): the basis-point-side projections of all blocks and the neighbour searches run on two
 * internal side streams ordered against `stream` by events; everything is joined back before the call returns its
 * last launch, so the caller only ever synchronises its own stream.  0 = issue everything on `stream` in order. */
int poem_set_overlap(poem_handle_t h, int enable);
/* Query-side row-tile chains (csrc/chain.hip), default ON for embed in {128, 256, 512} in fp32 mode: the Linears, residual
 * adds and LayerNorms between the attention kernels of a decoder block (pt_metro_transformer.py:56-91,34-40) run as four chain
 * launches per block with the activations resident in LDS; 0 = one launch per operator (the round-1 sequence; A/B and tests). */
int poem_set_chains(poem_handle_t h, int enable);
/* Scheduling switches by name, for A/B measurements (results are unaffected): "overlap", "anchor_tables", "chains" as the
 * setters above; "knn_early" (default 1): in chain mode the neighbour searches of block i+1 are issued right behind block i's
 * coordinate update instead of at the top of block i+1; "fused_sampling" (default 1, fp32 mode, embed in {128, 256, 512}):
 * F.grid_sample + the Q1 view + merge_features_mv / _sv (lib/models/heads/ptEmb_head.py:900-926,745-771) as the two kernels of
 * csrc/merge.hip -- the sampled tensor (sum N, C, S) and merge_net[0]'s hidden layer never reach HBM, the debug tap "g"
 * does not exist; 0 = the operator sequence (poem_project_sample, poem_gemm x4, poem_merge_reduce / _finalize), same
 * results to fp32 round-off (the cross-view dot products reduce in another order); "chain_combine" (default 1, chain mode,
 * 4 heads): the chain kernel behind a cross attention merges the attention's split-key partials while it fills its tile
 * instead of a separate combine launch writing the context rows (bit-identical); "xattn_merge" (default -1 = for batches of one or two samples; fp32 mode, head
 * dim 64, 4096 keys): the cross attention kernel merges its four split-key partials through LDS and writes the context rows
 * itself -- no partials in HBM, "chain_combine" then has nothing to do (bit-identical; at batch 32 0.5 % slower end to end,
 * at batch 1 / 2 2-3 % faster); "tables_first" (default 1): the fused
 * sampling kernel is ordered behind the block-0 anchor-table build of the neighbour-search stream (a CU that hosts a table
 * block takes one sampling block instead of two; results unaffected); "graphs" (default 1): replay the launch list of a
 * forward as a hipGraph, keyed by (batch size, workspace, options) -- NOT by the view layout; "graph_eager" (default 0): capture
 * at the first forward of a key instead of the second.
 * Round 3: "tables_cached" (default 1): read the block-0 anchor tables folded at poem_create (0 = rebuild them on every
 * forward: same kernel, same inputs, bit-identical); "chain_tile" (default 0 = per launch): row-tile height of the chain
 * kernels, 1 = 32 rows, 2 = 64 rows (csrc/chain.hip), 3 = 16-row units on v_mfma_f32_16x16x4_f32 (csrc/chain16.hip) -- any
 * choice gives the same bits; "knn_fma" (default 0): neighbour distances rounded as pytorch3d's CUDA kernel (poem_knn_ex below)
 * -- the one switch that is NOT round-off neutral by design.
 * "knn_query" (round 6; default 0 = poem_config_t.knn): N_NEIGHBOR_QUERY, 0..64 and <= nquery -- part of the model's configuration,
 * not an A/B switch; poem_workspace_bytes follows it (a count above 32 widens the neighbour buffers).
 * Round 4, all bit-identical: "gemm_xcd_map" (default 1; process-wide): panel GEMM blocks of one XCD own a row range and all its
 * column panels (csrc/gemm.hip); "f1_split" (default 1): the basis-point GEMM of blocks >= 1 as a 4C- and a 2C-column launch;
 * "gemm_kslab" (default 1; process-wide): K >= 512 Linears on the K-slab kernel; "bps_defer" (default 0): 1 / 2 / 3 = the
 * basis-point GEMM of block i+1 behind block i's first / second cross attention / its chain instead of up front; "va_p1"
 * (default -1 = small batches): one-query blocks of the full vector attention (0 never, 1 / 2 always with 3 / 2 waves per SIMD);
 * "xattn_merge" -1 / 0 / 1 as above; "xattn_tail" (round 6, default 1; process-wide; bit-identical): the remainder items of a
 * cross-attention launch -- 4 of a CU pair's 100 at the headline batch, a 13th item on half of the SIMDs -- run as channel-tile
 * halves on every SIMD (csrc/attn.hip xattn_half_item); "xattn_half" (default 1; process-wide): a single sample's merged cross attention on
 * 32-channel-tile items (twice the blocks, 48 instead of 64 MFMAs per key tile each); "small_batch" (default 3), a bit mask of launch-count / dependency shortcuts: 1 = one input
 * launch (coordinates + inverse extrinsics + projection table) and no query-embedding broadcast where block 0 runs on the anchor
 * tables, 2 = block 0's anchor keys / values read out of the rows its chain projects (batches of <= 5 samples).
 * Round 5, bit-identical: "group_min_views" (default 0): the samples whose view count divides 8 run the whole sampling stage in
 * ONE kernel (csrc/merge.hip sample_group_kernel: bilinear sampling, merge_net[0], the cross-view dot / weighted sum and
 * merge_net[1]; the hidden rows of merge_features_mv, ptEmb_head.py:745-762, never reach HBM) when the batch has at least this
 * many views -- 0 = enough to give every CU two of the kernel's 8-tile units, -1 = never (two-kernel form for every sample);
 * which samples go where is decided on the device from the view layout; "group_xcd" (default 1): that kernel's units in
 * XCD-aware order (a view's feature planes and projection table are fetched by one L2); "d2_first" (default 1): the
 * feed-forward chain of a block is issued in front of the next block's neighbour searches, so the launch graph keeps it on the
 * hardware queue of the chain before it (a launch that waits for another queue costs 5-13 us in a replayed graph) and the
 * searches take the side queue; "wait_merge" (default -1 = 3; bit mask): 1 = the first cross attention is issued in front of
 * the side stream's remaining launches (same reason), 2 = the main stream waits for the later blocks' basis-point GEMMs once,
 * where block 0's vector cross attention waits for its anchor rows anyway, 4 (lab) = it waits for a block's neighbour searches
 * at the block's first cross attention.  Scheduling only.
 * The switches marked process-wide are launcher statics: setting one on any handle sets it for the process (the launch-graph
 * key carries the process's values).  Unknown names and out-of-range values return POEM_E_ARG. */
int poem_set_option(poem_handle_t h, const char* name, int value);
/* Block-0 anchor tables of poem_head_forward (default on, fp32 mode).  In the first decoder block every query's
 * neighbours are the 32 fixed anchors (anchor_points, lib/models/bricks/point_transformers.py:10-32) and every sample's
 * query coordinates are the hand template (lib/models/heads/ptEmb_head.py:886-894,935: ((c + t) - c) / r, i.e. t / r up
 * to the rounding of c + t), so fc_delta's output and fc_gamma.0's positional term of both vector attentions
 * (point_transformers.py:88-91,144-147) are computed once per forward from t / r for the Q x 32 (query, anchor) pairs
 * and shared by all samples; the per-sample kernel runs one C x C GEMM per neighbour column instead of three.  Results
 * differ from the per-sample form by fp32 round-off of the inputs only and do not depend on the batch.  0 = per-sample
 * form everywhere (the exact arithmetic of the reference).  poem_decoder_forward never uses the tables. */
int poem_set_anchor_tables(poem_handle_t h, int enable);
/* Arithmetic of the three C x C per-neighbour GEMMs inside the fused vector attention (everything else is fp32 always):
 *   POEM_PRECISION_FP32 (default): v_mfma_f32_32x32x2_f32, exact fp32 products, k-ordered fma chains;
 *   POEM_PRECISION_SPLIT_F16X3 (opt-in, embed >= 128): hi/lo f16 splits of both operands on the f16 matrix cores
 *     (w_hi x_hi + w_hi x_lo + w_lo x_hi, fp32 accumulation; csrc/vecattn_split.hip) -- products carry ~22 significant
 *     bits instead of 24; measured MPVPE against the reference fixtures is unchanged at the 1e-5 mm level.  The
 *     ReLU outputs inside the attention MLPs saturate at 937.5 (f16 range after the x64 pre-scale).
 * Returns POEM_E_UNSUPPORTED when the handle has no split images (embed < 128), when a neighbour count is not 32, and when
 * nsample is not a multiple of 32: the split-precision attention kernels have no masked forms (poem_cross_attention_split_f16x3
 * likewise refuses nk % 32 != 0). */
#define POEM_PRECISION_FP32 0
#define POEM_PRECISION_SPLIT_F16X3 1
/*   POEM_PRECISION_SPLIT_F16X3_ALL (opt-in): additionally every Linear that runs on the panel GEMM kernel (all of them
 *     except the K = 4C feed-forward output Linear and the narrow ones) uses the same hi/lo scheme -- weights split per 32-row
 *     tile at handle creation, activations scaled by 16, split in registers (saturating at |x| = 3750); and the two
 *     contractions of the cross attention for head dims 32 / 64 (from the same fp32 K/V fragment images, split in
 *     registers).  Softmaxes, LayerNorms, sampling, neighbour searches, the K = 4C Linear: exact fp32. */
#define POEM_PRECISION_SPLIT_F16X3_ALL 2
int poem_set_precision(poem_handle_t h, int mode);
/* Operator level of the split panel GEMM: image (ceil(n/32)*32 * k * 4 bytes) and scales (ceil(n/32) floats, device) from
 * poem_pack_split_gemm; y = act(x w^T + bias) + residual as poem_gemm.  POEM_E_UNSUPPORTED for shapes the panel kernel
 * does not take (k % 16, n % 32, a 32-column panel beyond 128 KiB of LDS). */
/* poem_cross_attention with the four split-key partials of a query tile merged inside the kernel (four waves of one block,
 * through LDS, chunk order: the bits of poem_cross_attention) -- what poem_head_forward runs under "xattn_merge" = 1.
 * POEM_E_UNSUPPORTED unless embed / heads == 64 and nk / 32 splits into four chunks of >= 8 key tiles (nk = 4096). */
int poem_cross_attention_merged(const float* q, const float* k, const float* v, float* ctx, int batch, int nq, int nk, int embed,
                                int heads, void* scratch, size_t scratch_bytes, void* stream);
/* poem_cross_attention with both contractions as hi/lo f16 splits (head dims 32 and 64; POEM_E_UNSUPPORTED otherwise);
 * same arguments, scratch and partial/combine structure as poem_cross_attention. */
int poem_cross_attention_split_f16x3(const float* q, const float* k, const float* v, float* ctx, int batch, int nq, int nk,
                                     int embed, int heads, void* scratch, size_t scratch_bytes, void* stream);
int poem_pack_split_gemm(const float* w, int out_features, int in_features, void* image, float* scales, void* stream);
int poem_gemm_split(const float* x, int ldx, const void* image, const float* scales, const float* bias, const float* residual,
                    int ldr, float* y, int ldy, int m, int n, int k, int act, void* stream);
int poem_finalize_parametric(poem_handle_t h, const float* mano_verts, const float* mano_joints,
                             const float* reference_joints, int batch, float* out_xyz, void* stream);
/* Timing of the dominant kernel (the fused vector attention) with HIP events recorded on the launch stream around
 * each of its launches inside poem_head_forward / poem_decoder_forward.  enable(h, n) allocates n event pairs
 * (0 disables); read() synchronises the recorded pairs and returns their count and summed duration. */
int poem_profile_enable(poem_handle_t h, int max_launches);
int poem_profile_read(poem_handle_t h, int* launches, float* total_ms, int reset);
/* The same for the anchored (table) launches of block 0 (poem_set_anchor_tables), which poem_profile_read leaves out:
 * call it before a resetting poem_profile_read. */
int poem_profile_read_anchored(poem_handle_t h, int* launches, float* total_ms);
/* Generic form: the spans poem_head_forward times between HIP events on the caller's stream, by kind.  (Read before a
 * resetting poem_profile_read.) */
#define POEM_PROF_VECATTN 0        /* the full fused vector attention (what poem_profile_read sums) */
#define POEM_PROF_VECATTN_ANCHORED 1
#define POEM_PROF_SAMPLING 2       /* input_proj .. merge finalize: the sampling front end of one forward */
int poem_profile_read_stage(poem_handle_t h, int stage, int* launches, float* total_ms);
/* Debug taps: copies of intermediate tensors of the LAST poem_head_forward on this handle (device->device).
 * name: "x","g","bps_feat","pt_xyz","query_xyz","b<i>.h_cross","b<i>.f_self","b<i>.f_cross","b<i>.xyz",
 * "b<i>.feats","b<i>.idx_self","b<i>.idx_cross".  Returns number of elements or <0. */
int64_t poem_tap(poem_handle_t h, const char* name, void* dst, int64_t dst_elems, void* stream);
int poem_enable_taps(poem_handle_t h, int enable);

/* ---- individual operators (same kernels the whole path launches) ----------------------------------------- */
size_t poem_packed_linear_bytes(int out_features, int in_features);
int poem_pack_linear(const float* w, int out_features, int in_features, void* packed, void* stream);
/* Y[M,N] = act(X[M,K] . W^T + bias) + residual ; ldx/ldr/ldy in floats; bias/residual may be NULL. */
int poem_gemm(const float* x, int ldx, const void* w_packed, const float* bias, const float* residual, int ldr,
              float* y, int ldy, int M, int N, int K, int act, void* stream);
/* Layout-aware GEMM.  Layouts: POEM_LAYOUT_RM (row-major, ld* in floats) or POEM_LAYOUT_PA ("packed activation":
 * the fragment order of poem_pack_linear applied to the activation rows; buffers hold ceil(M/32)*32 rows; the
 * residual shares the output layout).  PA->PA chains are how the whole path runs its Linears (coalesced 1 KiB
 * operand loads and result stores). */
#define POEM_LAYOUT_RM 0
#define POEM_LAYOUT_PA 1
int poem_gemm_ex(const float* x, int ldx, const void* w_packed, const float* bias, const float* residual, int ldr,
                 float* y, int ldy, int M, int N, int K, int act, int in_layout, int out_layout, void* stream);
/* row-major (rows, cols) <-> PA; poem_packed_linear_bytes(rows, cols) gives the PA size. */
int poem_pack_rows(const float* x, int rows, int cols, void* packed, void* stream);
int poem_unpack_rows(const void* packed, int rows, int cols, float* x, void* stream);
int poem_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int cols, float eps,
                   void* stream);
/* table: (sum_{N=1..max_views} N, C, H*W) */
int poem_pe_table(const void* adapt_w_packed, const float* adapt_b, int embed, int h, int w, int max_views,
                  float* scratch_sine, float* table, void* stream);
/* the same with SinePositionalEncoding3D's `normalize` argument (petr_transformer.py:451-457): 0 = plain cumulative counts */
int poem_pe_table_ex(const void* adapt_w_packed, const float* adapt_b, int embed, int h, int w, int max_views, int normalize,
                     float* scratch_sine, float* table, void* stream);
/* The input of position_encoder (BasePointEmbedHead.position_embeding, lib/models/heads/ptEmb_head.py:113-181;
 * inverse_sigmoid lib/utils/transform.py:1145-1161): out (views, 3 * depth_num, feat_h, feat_w), channel 3 d + axis = the
 * inverse sigmoid of the position_range-normalised master-frame coordinate of pixel (x, y)'s frustum point at depth d.
 * img0, img1 = img_metas["inp_img_shape"][0], [1].  Reads cfg's feat_h, feat_w, depth_num, lid, depth_*, position_range. */
int poem_frustum_features(const poem_config_t* cfg, const float* cam_intr, const float* cam_extr, int views, int img0, int img1,
                          float* out, void* stream);
/* x[v,c,p] = W[c,:] . feat[v,:,p] + b[c] + table[pe_index[v], c, p] */
int poem_input_proj(const float* feat, const void* w_packed, const float* bias, const float* table,
                    const int32_t* pe_index, float* x, int views, int in_channels, int embed, int hw, void* stream);
/* g[v,c,s] = bilinear sample of x[v,c] at the projection of (bps[s] + centre[view_sample[v]]) into view v.
 * uv_scratch: (views, S, 2) floats (pixel-space sample coordinates ix, iy). */
int poem_project_sample(const float* x, const float* bps, const float* centre, const int32_t* view_sample,
                        const float* cam_intr, const float* cam_extr, float* uv_scratch, float* g, int views,
                        int embed, int fh, int fw, int nsample, int img_w, int img_h, void* stream);
int poem_merge_reduce(const float* h2, const int32_t* view_offsets, float* m, int batch, int nsample, int half,
                      void* stream);
int poem_merge_finalize(const float* g, const float* y, const int32_t* view_offsets, float* out, int batch,
                        int nsample, int embed, void* stream);
/* q (B,Q,C) k,v (B,S,C) -> ctx (B,Q,C); softmax(q k^T / sqrt(C/heads)) v per head  (any S >= 1, C % 32 == 0,
 * C/heads in {8,16,32,64,128,256}).  k and v are first re-laid into MFMA fragment images -- whole 32-key tiles per sample, the
 * rows behind key S zero-filled and given weight exactly 0 by the kernels' masked forms --, then the key axis is processed
 * in fixed chunks whose partial (O, m, l) triples are merged in fixed order (a sample's result does not depend on the
 * batch it travels in); images and partials live in `scratch` (poem_cross_attention_scratch_bytes() bytes, 16-byte
 * aligned).  Inside the decoder the projection GEMM writes the images itself. */
size_t poem_cross_attention_scratch_bytes(int batch, int nq, int nk, int embed, int heads);
int poem_cross_attention(const float* q, const float* k, const float* v, float* ctx, int batch, int nq, int nk,
                         int embed, int heads, void* scratch, size_t scratch_bytes, void* stream);
/* Ragged batched DLT triangulation -- replaces lib/utils/triangulation.py:5-45 (batch_triangulate_dlt_torch) and the
 * per-sample loop of lib/models/POEM.py:284-299: uv (BN,J,2) pixels, cam_intr (BN,3,3), cam_mat (BN,4,4),
 * view_offsets (B+1) DEVICE int32 prefix sums of views per sample -> out_xyz (B,J,3) in the master frame.
 * invert=1: cam_mat is the batch's cam_extr (camera->master) and is inverted here (POEM.py:286);
 * invert=0: cam_mat is already master->camera (the `Extrs` argument of the reference function).
 * batch * njoints <= INT32_MAX (the kernels index (sample, joint) in 32 bits): POEM_E_UNSUPPORTED beyond it, here and
 * in poem_dlt_confidence; nothing is launched. */
int poem_triangulate_dlt(const float* uv, const float* cam_intr, const float* cam_mat, const int32_t* view_offsets,
                         int batch, int njoints, int invert, float* out_xyz, void* stream);
/* Heat-map read-out in front of the triangulation (tail of heatmap_stage, lib/models/POEM.py:213-222, with
 * integral_heatmap2d, lib/models/integal_pose.py:194-218): heatmaps (BN,J,Hh,Wh) non-negative (sigmoid outputs) ->
 * uv (BN,J,2) in image pixels: normalise by (sum + 1e-6), expectation of (x/Wh, y/Hh), scale by (img_w, img_h). */
int poem_heatmap_uv(const float* heatmaps, float* uv, int views, int njoints, int hm_h, int hm_w, float img_w, float img_h,
                    void* stream);
/* The same read-out with the joint's confidence: conf (BN,J) = the maximum of each map (what `confis` of
 * triangulate_dlt holds, lib/utils/triangulation.py:115), in (0, 1) for sigmoid maps; a NaN pixel gives NaN.  uv has
 * the bits poem_heatmap_uv writes. */
int poem_heatmap_uv_conf(const float* heatmaps, float* uv, float* conf, int views, int njoints, int hm_h, int hm_w,
                         float img_w, float img_h, void* stream);
/* Confidence-aware ragged DLT -- replaces triangulate_dlt (lib/utils/triangulation.py:111-148) and the per-sample loop
 * around it.  Arguments as poem_triangulate_dlt, plus conf (BN,J) and the optional sel_count (B,J) DEVICE int32 = the
 * number of cameras that entered each solve (may be NULL).
 * mode POEM_DLT_THRESHOLD: per joint a camera is used when conf > threshold; while at most one is and threshold > 0,
 *   threshold -= 0.05 in fp64 (:134-142) -- and, as upstream mutates its argument inside the joint loop, the lowered
 *   value is what the following joints of that sample start from.  The pass runs on the device inside the launch.
 *   threshold <= 64 (NaN refused).  A joint left with fewer than two cameras has no triangulation; sel_count tells.
 * mode POEM_DLT_WEIGHTED: both rows of view n are scaled by conf[n][j]; no view is dropped; threshold is ignored.
 * conf == 1 everywhere (weighted), or threshold 0 with positive conf, reproduces poem_triangulate_dlt bit for bit.
 * njoints <= 4096; batch * njoints <= INT32_MAX (POEM_E_UNSUPPORTED beyond it).  Stream-ordered like every other call:
 * no host synchronisation, no copy. */
#define POEM_DLT_THRESHOLD 1
#define POEM_DLT_WEIGHTED 2
int poem_dlt_confidence(const float* uv, const float* conf, const float* cam_intr, const float* cam_mat,
                        const int32_t* view_offsets, float* out_xyz, int32_t* sel_count, int batch, int njoints, int invert,
                        int mode, double threshold, void* stream);
/* Outlier-robust ragged DLT.  Upstream has NO counterpart (lib/utils/triangulation.py stops at triangulate_dlt, which trusts every
 * view's 2-D joint); the definition is the one below, restated in fp64 in tests/dlt_robust_util.py.  Arguments as
 * poem_dlt_confidence without conf / mode / threshold.  Per (sample, joint), deterministic and exhaustive (no random sampling):
 *   every pair of the sample's views gives a two-view solve (poem_triangulate_dlt's arithmetic); view v is an inlier of it iff
 *   its reprojection error is < inlier_px pixels AND its depth is > 0 (both strict: a NaN is never an inlier); the pair with the
 *   most inliers wins, ties by the smaller summed squared error of the inliers, then by the smaller a * N + c.  With >= 2
 *   inliers the joint is solved again over the inlier set (the bits poem_triangulate_dlt gives those views alone); otherwise,
 *   and for every joint of a sample with a camera that is not finite, over all views with an empty inlier set (the bits of
 *   poem_triangulate_dlt, NaN behaviour included).  Then `refine` (0..16) Gauss-Newton steps on the summed squared reprojection
 *   error of the views solved over, fp64, each kept only if the error gets strictly smaller.
 * Limit of the method: with 3 views and one outlier every pair explains itself (all counts tie at 2) and the residual
 * tie-break does not identify the outlier; an outlier is found where at least three clean views remain.
 * Optional outputs (each may be NULL): inlier (BN,J) uint8; inlier_count (B,J) int32 (0 after the fallback); reproj_px (BN,J)
 * fp32 = the final joint's reprojection error in every view in pixels, inlier or not, NaN where it is not finite.
 * inlier_px > 0 (NaN refused; +inf = every view in front of the point), njoints <= 4096, batch * njoints <= INT32_MAX, else
 * POEM_E_ARG.  Every sample needs 2..64 views: the caller checks that (nothing on the device is read by the host); a sample
 * outside it gets NaN joints and residuals and count 0.  Stream-ordered, no host synchronisation, no workspace. */
int poem_dlt_robust(const float* uv, const float* cam_intr, const float* cam_mat, const int32_t* view_offsets, float* out_xyz,
                    uint8_t* inlier, int32_t* inlier_count, float* reproj_px, int batch, int njoints, int invert,
                    double inlier_px, int refine, void* stream);
/* Convolutional glue between the backbone's multi-level features and the head -- replaces
 * PtEmbedMultiviewStereoV2.feat_decode / uv_decode (lib/models/POEM.py:167-211, HRNet branch) built from
 * lib/models/bricks/conv.py ConvBlocks.  The Python mirror (poem_v2_amd/decode.py) chains them exactly as the
 * reference methods do.
 * poem_pack_conv3x3: OIHW (cout,cin,3,3) weights -> MFMA fragment image (poem_conv3x3_packed_bytes bytes); cin % 8 == 0.
 * poem_conv3x3: in (views,cin,h+2,w+2) with a zero border; y = conv(in)*scale[c] + shift[c] (conv bias and eval-mode
 *   BatchNorm folded by the caller; arrays padded to a multiple of 32 channels), optional ReLU, optional lateral add
 *   residual (views,cout,h/stride,w/stride) AFTER the activation (POEM.py:185-186); element (n,c,y,x) is written to
 *   out[n*out_view_stride + c*out_ch_stride + y*out_row_stride + x + out_offset] so that the result can land inside
 *   the next conv's zero-bordered input.  stride 1|2 (padding 1), (h/stride)*(w/stride) % 32 == 0.  The ReLU is torch's: a NaN
 *   stays a NaN (compare + select, not a max) -- here and in every operator of this block that takes `relu`.
 * poem_upsample2_concat_pad: out (views, ca+cb, h+2*pad, w+2*pad) = [bilinear x2 (align_corners=False) of
 *   a (views,ca,h/2,w/2) | b (views,cb,h,w)] with a zero border of pad (0|1) pixels (F.interpolate + torch.cat,
 *   POEM.py:189,203-204); ca or cb may be 0.
 * poem_pool_conv1x1_sigmoid: x (views,c,h,w) -> max_pool2d(2,2) -> 1x1 conv (j x c, bias) -> sigmoid ->
 *   heatmaps (views,j,h/2,w/2)  (POEM.py:206-207); c <= 64, j <= 32.  The maximum is max_pool2d's: NaN if any of the four is. */
size_t poem_conv3x3_packed_bytes(int cout, int cin);
int poem_pack_conv3x3(const float* w_oihw, int cout, int cin, void* packed, void* stream);
int poem_conv3x3(const float* in_padded, const void* w_packed, const float* scale, const float* shift,
                 const float* residual, float* out, int views, int cin, int cout, int h, int w, int stride, int relu,
                 int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset, void* stream);
/* The HRNet-W40 backbone on the same kernels (lib/models/backbones/hrnet.py upstream).  A "map" below
 * is a (views, c, h, w) tensor given by a pointer and (view_stride, ch_stride, row_stride, offset) in floats: element (n,c,y,x)
 * is p[n*view_stride + c*ch_stride + y*row_stride + x + offset] -- a plain tensor (c*h*w, h*w, w, 0) or the interior of a
 * zero-bordered one (c*(h+2)*(w+2), (h+2)*(w+2), w+2, w+3).  A map must stay inside its own channel plane
 * ((h-1)*row_stride + w-1 + offset < ch_stride): POEM_E_ARG otherwise.
 * poem_conv3x3_ex: poem_conv3x3 whose residual is a map of its own and, with res_before_act != 0, is added BEFORE the
 *   activation: y = relu(conv(in)*scale + shift + residual), a BasicBlock (hrnet.py BasicBlock.forward).  With res_before_act
 *   == 0 and a plain residual the result is poem_conv3x3's, bit for bit.  Same kernels and routing as poem_conv3x3 (direct,
 *   LDS-staged 32- and 16-row tiles; stride 2 on the direct kernel).  POEM_E_ARG: null pointers, cin % 8; POEM_E_UNSUPPORTED:
 *   stride other than 1|2, (h/stride)*(w/stride) % 32, a bordered input view of 2 GiB or more.
 * poem_pack_conv1x1 / poem_conv1x1: 1x1 convolution, weights (cout, cin) row-major packed once (poem_conv1x1_packed_bytes
 *   bytes; cin % 8 == 0): out = act(sum_ci W[co][ci]*in[ci] + shift[co] + residual) with in, residual (optional, before the
 *   activation) and out each a map; shift (cout floats) may be null; relu 0|1.  Any cout; (h*w) % 32 == 0.  POEM_E_ARG: null
 *   pointers, cin % 8, a map outside its plane; POEM_E_UNSUPPORTED: (h*w) % 32, an input view (cin*in_ch_stride floats) of
 *   2 GiB or more.
 * poem_hrnet_fuse: the fuse sum of a HighResolutionModule (hrnet.py:226-233): out = relu(((t0 + t1) + t2) + t3) over 2..4
 *   terms added in that order; term k is a map read at (y >> shift, x >> shift), shift 0..3 -- shift > 0 is
 *   nn.Upsample(mode="nearest") of a lower-resolution map, never materialised.  ReLU as torch's (NaN propagates). */
typedef struct poem_fuse_term {
  const float* data;
  int64_t view_stride;
  int32_t ch_stride, row_stride, offset, shift;
} poem_fuse_term_t;
int poem_conv3x3_ex(const float* in_padded, const void* w_packed, const float* scale, const float* shift, const float* residual,
                    int64_t res_view_stride, int res_ch_stride, int res_row_stride, int res_offset, int res_before_act, float* out,
                    int views, int cin, int cout, int h, int w, int stride, int relu, int64_t out_view_stride, int out_ch_stride,
                    int out_row_stride, int out_offset, void* stream);
size_t poem_conv1x1_packed_bytes(int cout, int cin);
int poem_pack_conv1x1(const float* w_oi, int cout, int cin, void* packed, void* stream);
int poem_conv1x1(const float* in, int64_t in_view_stride, int in_ch_stride, int in_row_stride, int in_offset, const void* w_packed,
                 const float* shift, const float* residual, int64_t res_view_stride, int res_ch_stride, int res_row_stride,
                 int res_offset, float* out, int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset,
                 int views, int cin, int cout, int h, int w, int relu, void* stream);
int poem_hrnet_fuse(const poem_fuse_term_t* terms, int nterms, float* out, int64_t out_view_stride, int out_ch_stride,
                    int out_row_stride, int out_offset, int views, int channels, int h, int w, void* stream);
int poem_upsample2_concat_pad(const float* a, int ca, const float* b, int cb, float* out, int views, int h, int w, int pad,
                              void* stream);
/* The ResNet-18/34/50 backbones (lib/models/backbones/resnet.py upstream) and the non-HRNet decode
 * branch (lib/models/POEM.py:168-181,205-206) need four operators besides the ones above -- BasicBlock and Bottleneck bodies run
 * on poem_conv3x3_ex and poem_conv1x1 as they are.  Same contract: exact fp32 on v_mfma_f32_32x32x2_f32 in a fixed k order (bit-
 * reproducible; a view's result does not depend on the other views of the launch), maps as above, stream-ordered, no
 * allocation, refusals before any store.  POEM_E_ARG: null pointers, cin % 8, a map outside its plane; POEM_E_UNSUPPORTED: odd
 * h or w, (h/2)*(w/2) % 32 (the pooling operator: odd h or w only), cout % 32 (stem), a view of 2 GiB or more.  h, w are the INPUT's.
 * poem_pack_conv7x7 / poem_conv7x7_s2: the stem (resnet.py:161-163,209-211).  Weights (cout,3,7,7) OIHW packed once
 *   (poem_conv7x7_packed_bytes bytes): an implicit GEMM with K = 3*49 = 147 zero-padded to 152.  in (views,3,h,w) plain; out map
 *   (views,cout,h/2,w/2) = relu(conv7x7(in, padding 3, stride 2)*scale[c] + shift[c]), ReLU as torch's (NaN propagates).  A
 *   padding tap is a zero operand, never a read outside the image.
 * poem_maxpool3x3_s2: nn.MaxPool2d(3, 2, 1), map (views,channels,h,w) -> map (views,channels,h/2,w/2); the padding counts as
 *   -inf; torch's bits: the window is scanned in (ky,kx) order and a value replaces the maximum when val > max || isnan(val).
 * poem_conv1x1_s2: the shortcut of the first block of layer2..4 (resnet.py:188-191): out(y,x) = W*in(2y,2x) + shift, no
 *   activation; in map (views,cin,h,w), out map (views,cout,h/2,w/2); w_packed is the poem_pack_conv1x1 image; shift may be null.
 * poem_maxpool2_conv1x1: x (views,cin,h,w) plain -> max_pool2d(2,2) (torch's rule, as above) -> 1x1 convolution (w_packed: the
 *   poem_pack_conv1x1 image of (cout,cin); bias (cout)) -> act 0 none (feat_in, POEM.py:180-181) | 1 sigmoid (uv_out, :205-206) ->
 *   out (views,cout,h/2,w/2) plain.  Any cout.
 * poem_upsample2_concat_pad_staged: poem_upsample2_concat_pad with pad = 1 whose interpolation is rounded as poem_upcat_conv3x3
 *   rounds it while it stages its input (the tap weights multiplied out, one multiply and three fmas; the older operator nests
 *   the two directions as torch does): poem_conv3x3 of the result equals poem_upcat_conv3x3 bit for bit, so the fused and the
 *   two-launch route of the non-HRNet decode branch return the same bits. */
size_t poem_conv7x7_packed_bytes(int cout);
int poem_pack_conv7x7(const float* w_oihw, int cout, void* packed, void* stream);
int poem_conv7x7_s2(const float* in, const void* w_packed, const float* scale, const float* shift, float* out,
                    int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset, int views, int cout, int h, int w,
                    void* stream);
int poem_maxpool3x3_s2(const float* in, int64_t in_view_stride, int in_ch_stride, int in_row_stride, int in_offset, float* out,
                       int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset, int views, int channels, int h,
                       int w, void* stream);
int poem_conv1x1_s2(const float* in, int64_t in_view_stride, int in_ch_stride, int in_row_stride, int in_offset, const void* w_packed,
                    const float* shift, float* out, int64_t out_view_stride, int out_ch_stride, int out_row_stride, int out_offset,
                    int views, int cin, int cout, int h, int w, void* stream);
int poem_maxpool2_conv1x1(const float* x, const void* w_packed, const float* bias, float* out, int views, int cin, int cout, int h,
                          int w, int act, void* stream);
int poem_upsample2_concat_pad_staged(const float* a, int ca, const float* b, int cb, float* out, int views, int h, int w, void* stream);
/* A stride-2 ConvBlock of feat_decode (POEM.py:183-189: padding 1, stride 2) straight from the UNBORDERED input
 * (views,cin,h,w): LDS-staged, 16-channel matrix tiles; out / residual addressing as poem_conv3x3.  POEM_E_UNSUPPORTED for
 * shapes other than HRNet-W40's three (cout, h = w) = (80, 64), (160, 32), (320, 16): use poem_conv3x3(stride 2) on a
 * zero-bordered copy then. */
int poem_conv3x3_down2(const float* in, const void* w_packed, const float* scale, const float* shift, const float* residual,
                       float* out, int views, int cin, int cout, int h, int w, int relu, int64_t out_view_stride,
                       int out_ch_stride, int out_row_stride, int out_offset, void* stream);
/* Process-wide A/B switches of the decode operators (not per handle: these operators take no handle).  Results do not depend on
 * them.  "s2_staging_wave" (default 1): poem_conv3x3_down2 as persistent blocks of four MFMA waves plus a fifth wave that does
 * all the LDS-DMA staging; 0 = the round-3 kernel in which every wave stages and multiplies; 2..4 = the default kernel with
 * that many blocks per CU instead of the rule in decode.hip (measurement only; 0 / 1 restore the rule).
 * "row_stager" (default 3; bit 0: at w = 64, bit 1: at w = 32): poem_upcat_conv3x3 stages its fused input by rows (wave =
 * channel, lane = (row group, column), the source rows of a chunk loaded once) and runs two blocks per CU; 0 = the per-float
 * stager of the other widths.
 * "pin32" (default 1): the fused-input convolution with five 32-channel tiles (uv_decode's first, 480 -> 160) runs its taps as a
 * pinned two-stage pipeline (next tap's weights and operands requested before this tap's MFMAs); 0 = compiler-scheduled taps.
 * "pool_fused" (default 1): poem_upcat_conv3x3_pool_head takes the shapes it supports; 0 = it returns POEM_E_UNSUPPORTED (A/B of
 * the two-launch form).
 * POEM_E_ARG for an unknown name or an out-of-range value. */
int poem_set_decode_option(const char* name, int value);
/* feat_decode's tail in one launch (POEM.py:190-193: F.interpolate(x, scale_factor=2, mode="bilinear") followed by feat_in, a
 * 1x1 convolution with bias): in (views,cin,h,w) -> out (views,cout,2h,2w).  The convolution is applied BEFORE the
 * interpolation (they commute: both linear, the interpolation weights sum to one) on the matrix cores with the input and the
 * low-resolution result in LDS.  w_packed: poem_pack_linear image of the (cout, cin) weight.  POEM_E_UNSUPPORTED unless
 * h = w = 8, cin % 8 == 0, cout % 32 == 0, (cin + cout) * 256 B <= 160 KB: use poem_input_proj + poem_upsample2_concat_pad then. */
int poem_conv1x1_upsample2(const float* in, const void* w_packed, const float* bias, float* out, int views, int cin, int cout,
                           int h, int w, void* stream);
/* One uv_decode stage in one launch (POEM.py:203-205: F.interpolate x2, torch.cat, ConvBlock): stride-1 conv3x3 of
 * [bilinear x2 of a_half (views,ca,h/2,w/2) | b_full (views,cb,h,w)] with the concatenation, the zero border and the
 * upsampling applied while the input halo is staged in LDS -- the concatenated tensor never exists.  Same epilogue and output
 * addressing as poem_conv3x3.  The border is zero whatever a_half holds (a select, not a product with zero tap weights: a NaN or
 * Inf in a_half reaches the outputs F.interpolate + the convolution would give it, no others).  POEM_E_UNSUPPORTED for shapes the
 * LDS-staged kernel does not take (cout > 160, w > 64, 256 % w != 0, ...): call poem_upsample2_concat_pad + poem_conv3x3 then. */
int poem_upcat_conv3x3(const float* a_half, int ca, const float* b_full, int cb, const void* w_packed, const float* scale,
                       const float* shift, float* out, int views, int cout, int h, int w, int relu, int64_t out_view_stride,
                       int out_ch_stride, int out_row_stride, int out_offset, void* stream);
int poem_pool_conv1x1_sigmoid(const float* x, const float* w, const float* bias, float* heatmaps, int views, int c, int j,
                              int h, int w_, void* stream);
/* uv_decode's last stage AND the read-out head in one launch (POEM.py:203-207 upstream: F.interpolate x2, torch.cat, ConvBlock,
 * then max_pool2d(2, 2) + uv_out + sigmoid): poem_upcat_conv3x3 whose epilogue pools its own rows, contracts them with
 * head_w (j x cout, row-major) + head_b and writes sigmoid(.) to heatmaps (views, j, h/2, w/2) -- the convolution's
 * (views, cout, h, w) output, which nothing else reads, never reaches HBM.  Same bits as poem_upcat_conv3x3 +
 * poem_pool_conv1x1_sigmoid, NaN and Inf inputs included (the same NaN-keeping ReLU and maxima in the same order).
 * POEM_E_UNSUPPORTED unless w == 64, h % 4 == 0, 33 <= cout <= 48, 1 <= j <= 32, ca, cb positive multiples of 8 and the pooled rows
 * and head weights fit the staging tile ((128 cout + j cout + j) floats <= 6400: j <= 31 at cout 40, j <= 5 at cout 48): call the
 * two operators then. */
int poem_upcat_conv3x3_pool_head(const float* a_half, int ca, const float* b_full, int cb, const void* w_packed, const float* scale,
                                 const float* shift, const float* head_w, const float* head_b, float* heatmaps, int views, int cout,
                                 int j, int h, int w, int relu, void* stream);
/* Device-side evaluation metrics (replace the host loops of lib/metrics/pa_eval.py:45-83,104-124 and
 * lib/metrics/pck.py:36-96).
 * poem_pa_epe: pred, gt (B,P,3) -> out (B,2) = per-sample (Procrustes-aligned mean distance, plain mean distance);
 *   alignment = PAEval.align_w_scale (scipy orthogonal_procrustes with scale, no reflection handling).
 * poem_pck_accumulate: adds this batch to counts (P,steps) [#dist <= linspace(val_min,val_max,steps)[t]],
 *   dist_sum (P) fp64 and n (P); the caller zeroes them at reset and derives pck / auc / epe from them;
 *   dist_out (B,P) optionally receives this batch's distances (NULL to skip). */
int poem_pa_epe(const float* pred, const float* gt, float* out, int batch, int npoints, void* stream);
int poem_pck_accumulate(const float* pred, const float* gt, int batch, int npoints, double val_min, double val_max,
                        int steps, uint32_t* counts, double* dist_sum, uint32_t* n, float* dist_out, void* stream);
/* Benchmark-protocol mesh scores: the device pieces of the FreiHAND / HO3D numbers -- mesh F-scores at 5 / 15 mm, raw and
 * Procrustes-aligned, and the AUC of the aligned joints / vertices.  The reference tree has no code of these (the public protocol
 * scripts loop over samples on the host through open3d); what each call replaces upstream is named with it.
 * poem_pa_align: PAEval.align_w_scale (lib/metrics/pa_eval.py:104-124) with its result kept: pred, gt (B,P,3) ->
 *   aligned (B,P,3) fp32, the fp32 rounding of the fp64 points whose mean distance to gt poem_pa_epe reports (one solve behind
 *   both), and transform (B,13) fp64 = c, R (3x3 row-major), t with aligned = c R p + t.  Either output may be NULL, not both.
 * poem_nn_distance: for a (B,na,3) and b (B,nb,3) the distance of every point of a to its nearest point of b (dist_ab (B,na)) and of
 *   every point of b to its nearest of a (dist_ba (B,nb)) -- the per-sample nearest-neighbour loop of the protocol scripts, brute
 *   force, any na, nb up to 2^24.  Squares in fp32 in numpy's order ((dx*dx + dy*dy) + dz*dz), each operation rounded on its own; the
 *   minimum over the fp32 squares; one root per point, of the minimum, correctly rounded (through fp64).
 *   counts (B,2,nthr) int32 = #{(double)d < thresholds[t]} per direction (0: a -> b, 1: b -> a) -- STRICT `<`, as the protocol
 *   scripts compare (poem_pck_accumulate's `<=` is _PCKMetric's) -- written, not accumulated; sums (B,2) fp64 = the distances'
 *   sum.  Every output is optional (NULL), at least one is needed.  thresholds: nthr <= 8 doubles in HOST memory, read at the call,
 *   non-negative and ascending; needed with counts.  counts and sums are reduced in a fixed order through `workspace`
 *   (poem_nn_distance_workspace_bytes(batch, na, nb, nthr) bytes, 8-byte aligned; not read when both are NULL): no atomics, and a
 *   sample's bits do not depend on the batch it is in.
 *   NaN rule: a point with a NaN coordinate is nearest to nothing and nothing is nearest to it -- its own distance is NaN (NaN in
 *   dist_*, counted under no threshold, carried by sums), it never lowers another point's minimum, and a direction whose target
 *   set is all NaN gives NaN distances and zero counts.
 *   POEM_E_ARG: NULL a / b, non-positive sizes, all four outputs NULL, counts without thresholds, a NaN, negative or non-ascending
 *   threshold; POEM_E_UNSUPPORTED: na or nb above 2^24 (poem_render_mesh's limit on a point count), nthr > 8;
 *   POEM_E_WORKSPACE: counts or sums asked for and the workspace NULL or short. */
int poem_pa_align(const float* pred, const float* gt, float* aligned, double* transform, int batch, int npoints, void* stream);
size_t poem_nn_distance_workspace_bytes(int batch, int na, int nb, int nthr);
int poem_nn_distance(const float* a, int na, const float* b, int nb, float* dist_ab, float* dist_ba, const double* thresholds, int nthr,
                     int32_t* counts, double* sums, void* workspace, size_t workspace_bytes, int batch, void* stream);
/* mano_to_openpose (lib/utils/transform.py:836-872; called on predicted and ground-truth vertices by testing_step,
 * lib/models/POEM.py:602-603): j_regressor (16,nverts) MANO's th_J_regressor, verts (B,nverts,3) -> joints (B,21,3) in
 * OpenPose order (16 regressed joints + the 5 finger-tip vertices, re-ordered).  nverts must be 778. */
int poem_mano_to_openpose(const float* j_regressor, const float* verts, float* joints, int batch, int nverts, void* stream);
/* MANO linear blend skinning: the `ManoLayer(pose_aa, betas)` call of the medium_MANO tail
 * (lib/models/bricks/pt_metro_transformer.py:120-124,147-148: manotorch ManoLayer(joint_rot_mode="axisang", use_pca=False,
 * flat_hand_mean=True, center_idx=9)) and the head's zero-pose template (lib/models/heads/ptEmb_head.py:732-736,886-892).
 * pose_aa (B,48) axis-angle of the 16 joints, betas (B,10); assets as device buffers: v_template (778,3),
 * shapedirs (778,3,10), posedirs (778,3,135), j_regressor (16,778), weights (778,16)  [MANO_RIGHT.pkl fields; licence-gated,
 * never read from disk here].  -> verts (B,778,3), joints (B,21,3) in the 21-joint hand order (16 skeleton joints + the
 * finger-tip vertices 745,317,444,556,673), both minus joint center_idx (-1: not centred).  manotorch is absent from the
 * reference tree: restated from the published model in manopth / manotorch's evaluation order -- parity unpinned. */
/* The rotation half of get_parametric_output (pt_metro_transformer.py:144-146 -> rot6d_to_aa, lib/utils/transform.py:448-466:
 * pytorch3d rotation_6d_to_matrix -> matrix_to_quaternion -> quaternion_to_axis_angle): params (B,106) = 16 six-dimensional
 * rotations then 10 betas -> pose_aa (B,48), betas (B,10). */
int poem_rot6d_to_axis_angle(const float* params, float* pose_aa, float* betas, int batch, void* stream);
/* Round 6: the five asset arrays are re-laid once into a TABLE (poem_mano_table_bytes() bytes of device memory, 16-byte
 * aligned; poem_mano_prepare at layer creation -- coefficient-major blend shapes, joint regression composed with template and
 * shape basis in fp64, joint-major skinning weights: csrc/mano.hip) and every call takes that table: one launch over
 * (13 vertex tiles x batch) blocks instead of one block per sample. */
size_t poem_mano_table_bytes(void);
int poem_mano_prepare(const float* v_template, const float* shapedirs, const float* posedirs, const float* j_regressor,
                      const float* weights, void* table, void* stream);
int poem_mano_lbs(const float* pose_aa, const float* betas, const void* table, int batch, int center_idx, float* verts,
                  float* joints, void* stream);
/* The MANO layer INSIDE the forward of a parametric handle (get_parametric_output, pt_metro_transformer.py:139-151, and the last
 * layer of ptEmb_head.py:953-958): with a table attached, poem_head_forward runs Q3 -> Linears -> rot6d -> poem_mano_lbs in its
 * captured launch graph and writes the last layer of out_xyz as nan_to_num(joints | verts) + centre itself;
 * poem_decoder_forward replaces the last layer's rows by (joints | verts).  pose_aa / betas are returned as before.  The table is
 * caller-owned and must stay valid while attached; table = NULL detaches (the caller then runs its own layer and
 * poem_finalize_parametric).  POEM_E_UNSUPPORTED on a handle without PARAMETRIC_OUTPUT. */
int poem_attach_mano(poem_handle_t h, const void* table, int center_idx);
/* Fit MANO pose, shape and translation to a mesh (upstream only offline: lib/fit/frame_fit/one_frame_fit.py, hundreds of Adam
 * steps per frame on the host through manotorch).  Levenberg-Marquardt with the analytic Jacobian; csrc/mano_fit.hip.
 *   Unknowns per sample  x = (pose_aa[48], betas[10], tsl[3]), 61 in all.
 *   Model  V(x) = the MANO mesh as stated above (csrc/mano.hip), NOT centred, plus tsl.  Rodrigues is the smooth exponential map
 *     exp([aa]x), without poem_mano_lbs's +1e-8 (the two differ by about 1e-8 rad); value and derivative use their series below
 *     |aa| = 1e-2, so a joint at exactly zero has the three generators as its derivative.
 *   r = V(x) - target (2334 numbers);  c = sum r^2 + shape_reg |betas|^2 + pose_reg |pose_aa[3:]|^2;
 *   g = J^T r, H = J^T J, with the regularisers' terms added (reg * x_p to g_p, reg to H_pp).
 *   Start: x0 (batch,61) when given.  Otherwise: root rotation = the rigid, scale-free alignment of the zero-pose, zero-shape mesh
 *     onto the target (the rotation of PAEval.align_w_scale's solve, taken to axis-angle through the quaternion with its largest
 *     component first: finite at angle pi), fingers and betas 0, tsl = centroid of the target - centroid of the rotated mesh.
 *     That solve handles no reflection (as upstream's alignment): for a mirrored target its orthogonal factor is improper and is
 *     passed through the quaternion unchanged -- a finite start that is no alignment, left to the iteration.
 *   Iteration, exactly `iters` times, mu = 1e-3 at first:  solve (H + mu D) dx = -g with D = max(diag H, 1e-12) by Cholesky;
 *     evaluate c, g, H at x + dx; accept iff the new cost is strictly smaller (a NaN is never accepted); on accept
 *     mu <- max(mu / 10, 1e-9), otherwise mu <- min(10 mu, 1e8) and x, g, H stay.  A pivot that is not positive or not finite
 *     gives dx = 0, which the same rule rejects.
 *   -> pose_aa (batch,48), betas (batch,10), tsl (batch,3) fp32; verts (batch,778,3) and joints (batch,21,3) = the model at the
 *     result, rounded to fp32; cost (batch) fp64 = c at the result; accepted (batch) int32 = accepted steps; status (batch) int32:
 *     0, or bit 0 = the target is not finite, bit 1 = the start (or its cost) is not finite.  A flagged sample returns its start
 *     (zeros where the default start could not be formed), cost NaN, accepted 0, and touches no other sample.
 *   fp32 inputs, every step fp64, no floating-point atomics, every sum in a fixed order: a sample's bits do not depend on its
 *   batch or its position in it, and two calls give the same bits.  2 * iters + 4 launches on `stream`, no host synchronisation.
 *   workspace: poem_mano_fit_workspace_bytes(batch) bytes, 8-byte aligned, caller-owned, need not be zeroed.  After the call its
 *     head holds the solver's fp64 state, for diagnostics and tests: sample b's 3928 doubles begin at double 3928 * b --
 *     x[61] at 0 (the result), the last candidate x + dx at 64, g[61] at 128, c at 192, mu at 193, H (61 x 61, row-major) at 200.
 *   POEM_E_ARG (nothing launched, outputs untouched): iters outside 0..64, a negative or non-finite regulariser, a null required
 *   pointer, batch < 0, a misaligned workspace; POEM_E_WORKSPACE: a short workspace; POEM_E_UNSUPPORTED: batch > 65535.
 *   batch == 0 is POEM_OK without a launch.  2-D keypoint terms and joint targets: poem_mano_fit_terms below, of which this call
 *   is the case "term M alone, mesh_weight 1" (the same kernels, the same bits).  Not built: silhouette terms, per-vertex weights,
 *   PCA pose, left hands, a backward pass. */
size_t poem_mano_fit_workspace_bytes(int batch);
int poem_mano_fit(const void* table, const float* target_verts, const float* x0_or_null, int batch, int iters, float shape_reg,
                  float pose_reg, void* workspace, size_t workspace_bytes, float* pose_aa, float* betas, float* tsl, float* verts,
                  float* joints, double* cost, int32_t* accepted, int32_t* status, void* stream);
/* The fit with up to three data terms: the mesh (M), 3-D joint targets (J) and 2-D keypoints in N calibrated views per sample (K).
 * Unknowns, model, regularisers, the iteration (mu, D, accept iff strictly smaller, a failed pivot = rejected), the fp64 rule and
 * the fixed-order sums are exactly poem_mano_fit's.  P_j(x), j = 0..20, is the fit's own `joints` output: the 16 chain joints and
 * the five tip vertices in the 21-joint hand order, uncentred, plus tsl (the order of pred_joints_3d / pred_joints_uv).
 *   c = mesh_weight sum_v |V_v(x) - target_v|^2                                      (M, present iff target_verts != NULL)
 *     + sum_j w3[b,j] |P_j(x) - joints3d[b,j]|^2                                     (J, present iff joints3d != NULL)
 *     + sum_{view n of sample b} sum_j w2[n,j] |(pi_n(P_j(x)) - kp[n,j]) / image_scale|^2     (K, present iff keypoints != NULL)
 *     + shape_reg |betas|^2 + pose_reg |pose_aa[3:]|^2,        g and H the Gauss-Newton ones of these rows.
 *   pi_n(p): p_cam = inv(cam_extr[n]) p (batch_cam_extr_transf; the 4x4 inverted in fp64 in the kernel), h = cam_intr[n] p_cam with
 *     the full 3x3, (u, v) = (h_x, h_y) / h_z (batch_cam_intr_projection) -- the convention of poem_loss_terms and
 *     poem_project_points, without upstream's |z| < 1e-7 -> 1e-7 clamp, which has no derivative worth following.
 *   Depth: a keypoint of positive weight whose camera-frame depth p_cam.z is <= POEM_FIT_ZMIN makes that candidate's cost +inf, so
 *     the accept rule rejects it; at the start it sets status bit 2 and the sample returns its start like the other flags.
 *   Views are ragged: view_offsets (batch + 1, int32, on the device; the host never reads it) -- sample b owns views
 *     [view_offsets[b], view_offsets[b+1]), which may be one view or none; indices are clamped into [0, total_views].
 *   Weights: an entry of weight 0 contributes nothing and is not read into the arithmetic (compare and select, never 0 * value:
 *     missing keypoints are commonly NaN); a view whose 21 weights are all 0 leaves every bit of the call as if it were absent
 *     (its camera is not read either).  A weight that is negative, NaN or infinite sets status bit 0; so does a non-finite mesh
 *     target, and a non-finite joint target, keypoint or camera under a positive weight.
 *   Start: x0 when given; otherwise with M the default of poem_mano_fit; otherwise with J the same rigid rule on the 21 zero-pose,
 *     zero-shape joints against joints3d (a joint there of weight 0 or not finite sets status bit 1).  K alone needs x0.
 *   status: bit 0 an input is not finite / a weight is not valid, bit 1 the start (or its cost) is not finite, bit 2 (value 4) the
 *     start has a positive-weight keypoint at depth <= POEM_FIT_ZMIN.  Bit 2 is set by the joint-term kernel at the first
 *     evaluation (the joints at the start need the whole model), which a sample flagged with bit 0 or 1 never reaches: bit 2
 *     never comes together with them.  The mesh kernel still runs once for such a sample.
 *   Upstream (one_frame_fit.py) minimises lambda_reproj mean_{n,j}(w |delta / scale|^2) + 5 * 0.1 |betas|^2: the mean is the constant
 *     factor 1 / (21 views_b) per sample, so its data term is term K with keypoint_weight = lambda_reproj w / (21 views_b) and
 *     shape_reg = 0.5.  Its quaternion-norm and anatomical axis losses are NOT built, nor its Adam iteration.
 *   Kernels (csrc/mano_fit.hip): the joint-term kernel, one block per sample, runs next to the mesh kernel at every evaluation and
 *     writes one more slot of sums; terms J and K are accumulated per joint over the views in order (a 3x3 matrix, a 3-vector and a
 *     scalar), never as a per-view Jacobian.  Launches on `stream`, no host synchronisation: 2 + (iters + 1) (1 + [M] + [J or K]),
 *     i.e. 3 * iters + 5 with M and a joint term, 2 * iters + 4 with one of the two.
 *   workspace: poem_mano_fit_terms_workspace_bytes(batch); its head is poem_mano_fit's (3928 doubles per sample, same offsets).
 *   POEM_E_ARG (nothing launched, outputs untouched): no term present; term K with any of keypoints, keypoint_weight, cam_intr,
 *     cam_extr, view_offsets NULL or total_views < 0; a weight array without its values (or joints3d without joints3d_weight);
 *     mesh_weight negative or not finite (read with M only); image_scale not > 0 or not finite (read with K only); K alone without
 *     x0; a NULL `terms`; and everything poem_mano_fit refuses.  POEM_E_UNSUPPORTED: total_views > 65535, batch > 65535. */
#define POEM_FIT_ZMIN 1e-3        /* metres */
typedef struct {
  const float* target_verts;   float mesh_weight;              /* (batch,778,3) or NULL                        */
  const float* joints3d;       const float* joints3d_weight;   /* (batch,21,3), (batch,21), or both NULL       */
  const float* keypoints;      const float* keypoint_weight;   /* (total_views,21,2), (total_views,21)         */
  const float* cam_intr;       const float* cam_extr;          /* (total_views,3,3), (total_views,4,4)         */
  const int32_t* view_offsets; int total_views;                /* (batch+1) on the device; term K needs all six */
  float image_scale;                                           /* > 0, finite                                  */
} poem_mano_fit_terms_t;
size_t poem_mano_fit_terms_workspace_bytes(int batch);
int poem_mano_fit_terms(const void* table, const poem_mano_fit_terms_t* terms, const float* x0_or_null, int batch, int iters,
                        float shape_reg, float pose_reg, void* workspace, size_t workspace_bytes, float* pose_aa, float* betas,
                        float* tsl, float* verts, float* joints, double* cost, int32_t* accepted, int32_t* status, void* stream);
/* Crop / warp / normalise every view of a batch in one launch (replaces the per-view host chain of
 * lib/utils/transform.py:153-170: cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) -> colour jitter -> to_tensor ->
 * normalize(0.5, 1)).  src: the raw uint8 HxWx3 images back to back in one device blob; src_offsets (views) byte offset
 * of each image; src_hw (views,2) = (height, width); m_inv (views,6) fp64 = the INVERSE (destination -> source) 2x3 map,
 * i.e. what cv::warpAffine derives from the matrix it is given; gain (views,3) fp64 per-channel colour gains or NULL.
 * Outputs (either may be NULL, not both): out_f32 (views,3,out_h,out_w) = p / 255 - 0.5; out_u8 (views,out_h,out_w,3).
 * Arithmetic is OpenCV's 8-bit fixed-point bilinear path (1/32-pixel coordinates, 15-bit weights): integer, bit-exact.
 * Any out_u8 base and any 4-byte aligned out_f32 base will do: the wide stores are taken only when out_w % 4 == 0 and the bases
 * sit on 4 (out_u8) and 16 (out_f32) bytes, the scalar ones otherwise.  POEM_E_UNSUPPORTED: views > 65535 or out_h > 262140. */
int poem_warp_affine(const uint8_t* src, const int64_t* src_offsets, const int32_t* src_hw, const double* m_inv,
                     const double* gain, float* out_f32, uint8_t* out_u8, int views, int out_h, int out_w, void* stream);
/* Operator-level entry points of the opt-in split-precision vector attention (see poem_set_precision).
 * poem_pack_split_linear: w (embed,embed) row-major fp32 -> image (embed*embed*4 bytes: hi | lo f16 fragments of w * scale)
 *   and *scale (device float, the power of two the image carries).
 * poem_vector_attention_split: the COMPOSED form of poem_vector_attention -- qg = W_g1 q + (W_g1 b_d2 + b_g1),
 *   kg = W_g1 k (row stride embed), images of W_d2, W_g1 W_d2 and W_g2, scales = their three scales (device). */
int poem_pack_split_linear(const float* w, int embed, void* image, float* scale, void* stream);
int poem_vector_attention_split(const float* query_xyz, const float* src_xyz, const float* anchor_xyz, const int32_t* idx,
                                int shared_idx, const float* qg, const float* kg, const float* v, int nsrc, const float* wd1,
                                const float* bd1, const void* wd2_image, const float* bd2, const void* wg1d2_image,
                                const void* wg2_image, const float* scales, float* out, int batch, int nq, int embed,
                                void* stream);
/* idx (B,Q,32) int32: 32 nearest src points per query, ascending squared L2, ties -> lower index.  32 <= nsrc <= 8192 (a sample's
 * source coordinates are staged in LDS; poem_knn_k: 1 <= nsrc <= 8192); POEM_E_ARG beyond. */
int poem_knn(const float* query_xyz, const float* src_xyz, int32_t* idx, int batch, int nq, int nsrc, void* stream);
/* The same with a choice of the distance's rounding.  fma_contract = 0: ((dx*dx + dy*dy) + dz*dz), every operation rounded --
 * pytorch3d's CPU kernel (knn_cpu.cpp, built without FMA), the path BASELINE's parity bar is stated against, and what
 * poem_knn / poem_head_forward use.  fma_contract = 1: fma(dz, dz, fma(dy, dy, dx*dx)) -- pytorch3d's CUDA kernel
 * (knn.cu `dist += diff * diff` under nvcc's default -fmad=true), for comparing with results produced on a CUDA box;
 * whole path: poem_set_option(h, "knn_fma", 1).  The two differ by <= 1 ulp per distance and only reorder near-ties. */
int poem_knn_ex(const float* query_xyz, const float* src_xyz, int32_t* idx, int batch, int nq, int nsrc, int fma_contract,
                void* stream);
/* Vector attention core.  q (B,Q,C); k,v (B,NS,C) gathered by idx; idx (B,Q,32) or (32) when shared_idx!=0;
 * neighbour coordinates: anchor_xyz (32,3) when non-NULL, else src_xyz[b, idx];
 * wd1 (C,3)+bd1 raw; wd2, wg1, wg2 packed (C,C) + biases.  out r (B,Q,C) = sum_j softmax_j(a/sqrt(C)) * (v_j + pos_j). */
int poem_vector_attention(const float* query_xyz, const float* src_xyz, const float* anchor_xyz, const int32_t* idx,
                          int shared_idx, const float* q, const float* k, const float* v, int nsrc,
                          const float* wd1, const float* bd1, const void* wd2_packed, const float* bd2,
                          const void* wg1_packed, const float* bg1, const void* wg2_packed, const float* bg2,
                          float* out, int batch, int nq, int embed, void* stream);
/* Any neighbour count k in 1..64 (N_NEIGHBOR / N_NEIGHBOR_QUERY above 32).  poem_knn_k: the k nearest of poem_knn_ex's order,
 * idx (B,Q,ld) int32 with ld >= k (columns k..ld-1 untouched), 1 <= k <= nsrc.  poem_vector_attention_k: poem_vector_attention
 * over the first k columns of idx (B,Q,ld), neighbour coordinates src_xyz[b, idx] (no anchors), key rows `key` (B,NS,C);
 * softmax over the k neighbours, taken as 32-column tiles folded by an online softmax. */
int poem_knn_k(const float* query_xyz, const float* src_xyz, int32_t* idx, int batch, int nq, int nsrc, int k, int ld,
               int fma_contract, void* stream);
int poem_vector_attention_k(const float* query_xyz, const float* src_xyz, const int32_t* idx, int k, int ld, const float* q,
                            const float* key, const float* v, int nsrc, const float* wd1, const float* bd1,
                            const void* wd2_packed, const float* bd2, const void* wg1_packed, const float* bg1,
                            const void* wg2_packed, const float* bg2, float* out, int batch, int nq, int embed, void* stream);
/* xyz_out = xyz_in + r . W^T + b   (W (3,C) raw) */
int poem_reg_update(const float* r, const float* w, const float* b, const float* xyz_in, float* xyz_out, int rows,
                    int embed, void* stream);

/* ---- rendering (csrc/render.hip): the device side of `eval_single.py --draw` ------------------------------------------------------
 * poem_render_mesh draws `nmeshes` meshes per sample (one shared face list) into every view of a ragged batch.
 *   verts (nmeshes,B,V,3) master frame; faces (F,3); vf_offsets (V+1) / vf_faces (3F): the vertex -> face CSR table (the faces around
 *   vertex i are vf_faces[vf_offsets[i] .. vf_offsets[i+1]); vertex normals sum the face normals in that order); cam_intr (BN,3,3)
 *   (fx, fy, cx, cy are read), cam_extr (BN,4,4) camera->master, view_offsets (B+1) DEVICE int32 prefix sums; background
 *   (BN,H,W,3) uint8 shared by the meshes, or NULL = white; lights (L,6) = position in the CAMERA frame | colour; albedo (3).
 *   rgb (nmeshes,BN,H,W,3) uint8 = trunc(colour * 255); depth (nmeshes,BN,H,W) camera z, +inf where nothing is hit; face_id int32,
 *   -1 where nothing is hit; both may be NULL.
 *   Conventions: the sample point of pixel (x, y) is (x, y) in the intrinsics' pixel coordinates (integers are pixel centres);
 *   top-left fill rule; nearest depth wins, the lower face index at equal depth; faces with a vertex at z < near_z or without area are
 *   dropped whole (no clipping); no back-face culling; Lambert shading per vertex, perspective-correct interpolation.
 *   The view count BN = view_offsets[batch] stays on the device, so the host cannot hold the workspace against it: the call draws
 *   the first cap = workspace_bytes / poem_render_workspace_bytes(1, nverts, nmeshes) views of every mesh (the workspace is laid
 *   out for cap views and never addressed past them) and skips those past BN.  Pass poem_render_workspace_bytes(BN, ...) bytes or
 *   more (8-byte aligned) to draw every view; with fewer, the planes of views cap .. BN-1 in rgb / depth / face_id are left
 *   untouched.  POEM_E_WORKSPACE when the workspace holds no view.
 *   vf_offsets has nverts + 1 entries -- for the nverts of THIS call (vertices no face names have empty lists).  rgb, depth and
 *   face_id must not overlap background or each other.
 *   Invalid arguments (NULL, non-positive sizes, near_z <= 0) return POEM_E_ARG.  POEM_E_UNSUPPORTED: nlights > 8; h or w > 16384;
 *   nmeshes > 65535; nverts or nfaces > 2^24; views past 65535 in one call are not drawn.  Image planes are addressed with 64-bit offsets.
 * poem_project_points: points (B,P,3) master frame -> uv (BN,P,2) pixel coordinates in every view of the point's sample (the vertex
 *   stage of the renderer alone; total_views <= 65535, npoints <= 2^24).
 * poem_draw_skeleton: image, out (BN,H,W,3) uint8 (out may be image); joints_uv (BN,21,2) pixels; colours (21,3) in [0,1].  Joint j
 *   paints a disc of radius 6 px and a capsule of half-width 1.5 px to its parent (the wrist for j = 4k+1, else j-1) over the joints
 *   before it.  No anti-aliasing.  views <= 65535, h, w <= 16384. */
size_t poem_render_workspace_bytes(int total_views, int nverts, int nmeshes);
int poem_render_mesh(const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_faces, const float* cam_intr,
                     const float* cam_extr, const int32_t* view_offsets, const uint8_t* background, const float* lights, int nlights,
                     const float* albedo, float near_z, uint8_t* rgb, float* depth, int32_t* face_id, int nmeshes, int batch, int nverts,
                     int nfaces, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
int poem_project_points(const float* points, const float* cam_intr, const float* cam_extr, const int32_t* view_offsets, float* uv, int batch,
                        int npoints, int total_views, void* stream);
int poem_draw_skeleton(const uint8_t* image, const float* joints_uv, const float* colours, uint8_t* out, int views, int h, int w,
                       void* stream);

/* ---- loss terms (csrc/loss.hip): the VALUE of the reference's training losses, no backward pass ------------------------------------
 * poem_loss_terms evaluates every term of PtEmbedMultiviewStereoV2.compute_loss (lib/models/POEM.py:363-466 upstream) for a ragged batch
 * in one launch plus a one-block finalize; nothing returns to the host.
 *   coords (B,799,3): the last layer of all_coords_preds (21 joints, then 778 vertices); pred_joints_uv (BN,21,2); pred_pose (B,16,3) and
 *   pred_shape (B,10) when cfg->parametric (else ignored, may be NULL); master_joints_3d (B,21,3), master_verts_3d (B,778,3),
 *   target_joints_2d (BN,21,2), cam_intr (BN,3,3), cam_extr (BN,4,4) camera->master (its inverse is taken per view, POEM.py:383),
 *   view_offsets (B+1) DEVICE int32 prefix sums; mano_pose (BN,16,3) / mano_shape (BN,10) per view, read at the master view's row
 *   view_offsets[b] (POEM.py:439-444); j_regressor (16,778) MANO's th_J_regressor.  All fp32.
 *   out: POEM_LOSS_NTERMS doubles in device memory, in the key order of upstream's loss_dict:
 *     [0] loss_heatmap_joints  mean over (BN,21) of sum_2 ((uv_pred - uv_gt) / scale)^2, scale = sqrt(w^2 + h^2)        (POEM.py:372,377-379)
 *     [1] loss_3d_joints       MSE (joints_l2) or L1 of the predicted joints                                            (:404)
 *     [2] loss_3d_joints_from_mesh  the same on mano_to_openpose of the predicted and the ground-truth vertices         (:386-387,403)
 *     [3] loss_3d_verts        MSE (vertices_l2) or L1; parametric: (pred - c) - (gt - c), c = GROUND-TRUTH joint center_idx (:408-418)
 *     [4] loss_recon           the weighted sum of [1..3], [5..8]                                                       (:405,419,427,435,448)
 *     [5] loss_2d_joints       loss_proj_to_multicam: joints into every view of their sample, z = 1e-7 where |z| < 1e-7, the offset to
 *                              target_joints_2d clamped to +-scale/2, / scale, sum_2 of squares, mean over (BN,21)      (:336-361,422-427)
 *     [6] loss_2d_verts        the same for the vertices against the projected ground-truth vertices                    (:389-400,430-435)
 *     [7] loss_pose  [8] loss_shape   MSE against the master views' mano_pose / mano_shape                              (:438-448)
 *     [9] loss                 heatmap_joints_weight * [0] + [4]                                                        (:381,455)
 *   Terms upstream does not compute are not computed and come out as 0: [5] / [6] at a zero weight, [7] / [8] unless parametric.
 *   Every arithmetic step is fp64 (upstream: fp32); fixed-order reduction without floating-point atomics, so a call is reproducible
 *   bit for bit; a NaN input makes the terms it reaches NaN -- as torch.clamp does -- and leaves the others untouched.
 *   workspace: poem_loss_workspace_bytes(batch, total_views) bytes, 8-byte aligned, caller-owned (block partials; need not be zeroed).
 *   POEM_E_ARG: a NULL argument -- j_regressor included: the from-mesh term is part of loss_recon, a silent 0 would be a wrong loss --,
 *   non-positive sizes, batch > total_views, center_idx outside 0..20, misaligned out / workspace.  POEM_E_UNSUPPORTED: total_views >
 *   65535.  POEM_E_WORKSPACE: workspace_bytes too small.  None of them launches.  Rows are addressed with 64-bit offsets. */
#define POEM_LOSS_NTERMS 10
typedef struct poem_loss_cfg {
  double joints_weight, vertices_weight, joints_2d_weight, vertices_2d_weight, heatmap_joints_weight; /* LOSS.*_WEIGHT (POEM.py:125-129) */
  double pose_weight, shape_weight;             /* POSE_LOSS_WEIGHT, SHAPE_LOSS_WEIGHT (:130-131) */
  int32_t joints_l2, vertices_l2;               /* JOINTS_LOSS_TYPE / VERTICES_LOSS_TYPE == "l2": MSELoss, else L1Loss (:133-141) */
  int32_t parametric;                           /* HEAD.TRANSFORMER.PARAMETRIC_OUTPUT (:44) */
  int32_t center_idx;                           /* TRANSFORMER_CENTER_IDX (:45) */
  int32_t img_h, img_w;                         /* gt["image"].size(-2), .size(-1) (:369-370) */
} poem_loss_cfg_t;
size_t poem_loss_workspace_bytes(int batch, int total_views);
int poem_loss_terms(const float* coords, const float* pred_joints_uv, const float* pred_pose, const float* pred_shape,
                    const float* master_joints_3d, const float* master_verts_3d, const float* target_joints_2d, const float* cam_intr,
                    const float* cam_extr, const int32_t* view_offsets, const float* mano_pose, const float* mano_shape,
                    const float* j_regressor, const poem_loss_cfg_t* cfg, int batch, int total_views, double* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- baseline JPEG (csrc/jpeg.cpp, csrc/jpeg.h, csrc/jpeg.hip): the `image_<i>.jpg` members of a record shard without PIL ---------
 * Replaces webdataset's decode("rgb8") for JPEG members (PIL -> libjpeg on one Python thread): the serial half (marker parsing,
 * Huffman decoding) runs on host threads, the dense half (dequantisation, inverse DCT, chroma up-sampling, YCbCr -> RGB) on the
 * device, and writes the interleaved uint8 pixels where poem_warp_affine reads them.  The arithmetic (csrc/jpeg.h) restates
 * libjpeg's default path and gives PIL's bytes, or the image is REFUSED (status > 0) and the caller decodes it with PIL: refusing
 * is never an error of the call.
 * Accepted: SOF0 / SOF1, 8-bit samples, Huffman coding, ONE scan holding every component; 1 component, or 3 components taken as
 *   YCbCr with luma sampling 1x1, 2x1 or 2x2 and both chroma components 1x1; 8-bit quantisation tables; DRI / RSTn; byte stuffing;
 *   any APPn / COM segment (EXIF orientation is ignored, as Image.open ignores it).  Chroma is up-sampled as libjpeg does it: the
 *   3:1 "fancy" taps where the component is more than 2 samples wide, plain replication in images of width <= 4.
 * Refused: progressive, lossless, hierarchical or arithmetic-coded frames; 12-bit samples; 2 or 4 components; an Adobe APP14
 *   segment whose transform is not 1 on a 3-component image, or 'R','G','B' component ids without an Adobe segment (libjpeg may
 *   read either as RGB); any other sampling; 16-bit quantisation tables; a table a component names but no segment defined; a Huffman
 *   table that is not a prefix code; a second frame header, DNL, or any marker the grammar does not allow where it stands; an
 *   entropy stream that ends early, overruns a block, holds a DC value outside int16, lacks an expected RSTn or is not followed by
 *   EOI; a height or width of 0 or above 65500; a block whose dequantised coefficients sum (in magnitude) above 5900 -- the range
 *   guard derived in csrc/jpeg.h, beyond which libjpeg-turbo's 16-bit SIMD arithmetic and 32-bit arithmetic part ways.
 * poem_jpeg_desc_t: one image of a call.  Coefficients are int16, de-zigzagged (natural order, row-major 8x8), block after block in
 *   raster order of each component's block grid, component after component; the grids are padded to whole MCUs exactly as the scan
 *   holds them (blocks_w / blocks_h; a 1-component image has ceil(w/8) x ceil(h/8)).  quant[c] is COMPONENT c's table, natural order.
 * poem_jpeg_entropy_decode (host; no GPU is touched): n streams -> descs[n] and the coefficients, both in CALLER memory (pinned
 *   staging).  Headers are parsed first and the images that pass are given consecutive 16-byte aligned coef_offsets; totals[0] is the
 *   byte count that layout needs.  coef == NULL stops there (a size query: totals and the header fields of descs are valid);
 *   otherwise POEM_E_WORKSPACE when coef_bytes < totals[0] (nothing written to coef), else the scans are decoded by `threads` host
 *   threads (<= 0: 8; at most 16; a fixed number, never the machine's core count), image by image, each writing only its own
 *   range.  An image refused at this stage keeps its range (unused).  After it block_base / quad_base are the prefix sums over the
 *   images taken, totals = {coef bytes, blocks, quads, images taken}: a quad is a run of 4 pixels of one row, h * ceil(w / 4) per
 *   image.  Every read is checked against lengths[i], every write against coef_bytes.  The result does not depend on `threads`.
 *   status: 0 taken, 1 unsupported format, 2 malformed stream, 3 range guard.  POEM_E_ARG: NULL pointers, n <= 0, a negative length,
 *   coef off 16 bytes; POEM_E_UNSUPPORTED: n > 65535 (poem_warp_affine's limit), or no host memory for the n frame states.
 * poem_jpeg_reconstruct (device): descs, coef, out_offsets in DEVICE memory as uploaded; image i is written as (h, w, 3) uint8 RGB
 *   (a 1-component image replicated) at out + out_offsets[i]; refused images are skipped and nothing else of `out` is touched.  An
 *   image whose descriptor is inconsistent, whose coefficients end past coef_bytes or whose pixels end past out_bytes is skipped
 *   too.  Any alignment of out and the offsets will do (dword stores where a row segment sits on 4 bytes, byte stores elsewhere).
 *   workspace: poem_jpeg_workspace_bytes(total_blocks) = 64 total_blocks bytes for the uint8 component planes, 16-byte aligned;
 *   POEM_E_WORKSPACE when NULL or short.  total_blocks / total_quads = totals[1], totals[2].  POEM_E_ARG: NULL pointers, n <= 0,
 *   negative totals, misaligned coef / workspace (16).  POEM_E_UNSUPPORTED: n > 65535, or 2^24 workgroups or more in a launch (above
 *   32 (2^24 - 1) blocks or 256 (2^24 - 1) quads: about 2800 views of 640x480).  Nothing to do (no image taken) is POEM_OK without a launch; total_quads = 0 with blocks runs the inverse DCT
 *   alone (the planes stay in the workspace; tools/bench_jpeg.py times the two kernels that way).  All offsets are 64-bit.
 * poem_jpeg_reconstruct_host: the same through plain loops over csrc/jpeg.h, host memory, no GPU: pins the arithmetic to PIL where
 *   there is no device, and is what tools/jpeg_hostcheck.cpp drives under the sanitizers. */
typedef struct poem_jpeg_desc {
  int32_t status;                    /* 0 taken; > 0 refused (see above) */
  int32_t height, width, ncomp;      /* ncomp 1 | 3 */
  int32_t hs, vs;                    /* luma sampling factors: 1,1 | 2,1 | 2,2 */
  int32_t blocks_w[3], blocks_h[3];  /* block grid of each component, padded to whole MCUs */
  int64_t coef_offset, coef_bytes;   /* this image's range in the coefficient buffer (bytes; offset on 16) */
  int64_t block_base, quad_base;     /* blocks / quads of the images taken before this one */
  uint16_t quant[3][64];
} poem_jpeg_desc_t;
int poem_jpeg_entropy_decode(const uint8_t* const* streams, const int64_t* lengths, int n, poem_jpeg_desc_t* descs, int16_t* coef,
                             int64_t coef_bytes, int64_t* totals, int threads);
size_t poem_jpeg_workspace_bytes(int64_t total_blocks);
int poem_jpeg_reconstruct(const poem_jpeg_desc_t* descs, const int16_t* coef, int64_t coef_bytes, const int64_t* out_offsets,
                          uint8_t* out, int64_t out_bytes, int n, int64_t total_blocks, int64_t total_quads, void* workspace,
                          size_t workspace_bytes, void* stream);
int poem_jpeg_reconstruct_host(const poem_jpeg_desc_t* descs, const int16_t* coef, int64_t coef_bytes, const int64_t* out_offsets,
                               uint8_t* out, int64_t out_bytes, int n);

/* ---- baseline JPEG, Huffman decoding on the device (csrc/jpeg_entropy.h, csrc/jpeg_entropy.hip; opt-in) ------------------------------
 * The entropy stage of the route above without host threads: the host only parses the headers and packs the entropy-coded bytes
 * (about a fifth of the coefficients' size) for the upload; the device decodes them into the coefficient buffer poem_jpeg_reconstruct
 * reads.  A serial bit stream is decoded in parallel by cutting each image's segment into SUBSEQUENCES of `subseq` raw bytes (a
 * power of two, 16..1024; 0 = the default, 64) and iterating every subsequence's entry state to the fixed point, which is the
 * serial decoder's state by induction whatever the stream; poem_jpeg_entropy_decode is the yardstick:
 * status 0 exactly where it gives 0, the same coefficient bytes where taken, header-stage statuses equal (the same parser).  Which
 * of 2 / 3 a damaged scan gets may differ where it breaks two rules.
 * poem_jpeg_scan_t: one image's scan.  poem_jpeg_huff_t: one Huffman table as the decoders read it (9-bit look-up, then maxcode /
 *   valoff), 1424 bytes.  An image's distinct tables (at most 6) stand at tables[table_base ...]; dc_sel / ac_sel index them per
 *   component.
 * poem_jpeg_entropy_prepare (host; no GPU is touched): parses n streams' headers.  descs / totals[0..3] come out exactly as from
 *   poem_jpeg_entropy_decode's size query; scans[n]; totals[4] = bytes of the packed segments (each image's runs from its first
 *   entropy-coded byte to the END of its stream, on 16 bytes), totals[5] = tables, totals[6] = subsequences of the call, totals[7]
 *   = the most of one image.  packed == NULL stops there (tables may be NULL too); else POEM_E_WORKSPACE when packed_bytes <
 *   totals[4] or table_room < totals[5] (nothing written), else tables and bytes are copied.  Images refused at the header stage
 *   get an empty scan.  POEM_E_ARG: NULL pointers, n <= 0, a negative length or room, subseq not as above, packed off 16 bytes;
 *   POEM_E_UNSUPPORTED: n > 65535 or no host memory.
 * poem_jpeg_entropy_device: everything in DEVICE memory as uploaded.  Zeroes coef[0 .. coef_bytes), decodes, turns DC differences
 *   into predictions and applies the range guard; status[i] (int32, device) gets every image's status and descs[i].status the same,
 *   so that poem_jpeg_reconstruct skips what was refused here.  One workgroup of wg_threads lanes (64..1024, a multiple of 64;
 *   0 = 1024) per image converges with barriers only: no workgroup waits for another.  Every stream read is bounded by the scan's own
 *   byte range inside packed_bytes, every store by the image's own block range inside coef_bytes, every workspace index by
 *   total_subs; a scan record or descriptor that does not hang together refuses its image.  The first n int32 of the workspace
 *   hold the rounds each image took.  poem_jpeg_entropy_workspace_bytes(n, total_subs) says how large it must be (16-byte
 *   aligned).  POEM_E_ARG: NULL pointers, n <= 0, negative sizes, subseq / wg_threads not as above, coef / packed / workspace off
 *   16 bytes; POEM_E_WORKSPACE: workspace NULL or short; POEM_E_UNSUPPORTED: n > 65535.
 * poem_jpeg_entropy_parallel_host: the SAME algorithm in plain loops over csrc/jpeg_entropy.h (fixed point, prefix sum, write pass,
 *   DC pass, block pass), host memory, arguments as poem_jpeg_entropy_decode plus subseq and rounds[n] (may be NULL): where there
 *   is no device it pins the algorithm to the serial decoder, and tools/jpeg_entropycheck.cpp drives it under the sanitizers. */
typedef struct poem_jpeg_huff {
  uint16_t look[512];                /* 9-bit prefix -> (length << 8) | symbol; 0: longer than 9 bits, or no such code */
  int32_t maxcode[18];               /* largest code of each length (-1: none); [17] = sentinel */
  int32_t valoff[17];                /* index of the first symbol of a length minus its first code */
  uint8_t vals[256];
  int32_t reserved;
} poem_jpeg_huff_t;
typedef struct poem_jpeg_scan {
  int64_t byte_offset, byte_count;   /* the segment in the packed buffer (offset on 16) */
  int64_t sub_base;                  /* subsequences of the images before this one */
  int32_t sub_count;                 /* ceil(byte_count / subseq) */
  int32_t restart;                   /* DRI: MCUs per restart interval, 0 = none */
  int32_t table_base, table_count;
  uint8_t dc_sel[3], ac_sel[3];      /* per component: which of the image's tables */
  uint8_t reserved[2];
} poem_jpeg_scan_t;
int poem_jpeg_entropy_prepare(const uint8_t* const* streams, const int64_t* lengths, int n, int subseq, poem_jpeg_desc_t* descs,
                              poem_jpeg_scan_t* scans, poem_jpeg_huff_t* tables, int64_t table_room, uint8_t* packed,
                              int64_t packed_bytes, int64_t* totals);
size_t poem_jpeg_entropy_workspace_bytes(int n, int64_t total_subs);
int poem_jpeg_entropy_device(poem_jpeg_desc_t* descs, const poem_jpeg_scan_t* scans, const poem_jpeg_huff_t* tables,
                             int64_t table_count, const uint8_t* packed, int64_t packed_bytes, int n, int subseq, int wg_threads,
                             int64_t total_subs, int64_t total_blocks, int16_t* coef, int64_t coef_bytes, int32_t* status,
                             void* workspace, size_t workspace_bytes, void* stream);
int poem_jpeg_entropy_parallel_host(const uint8_t* const* streams, const int64_t* lengths, int n, int subseq, poem_jpeg_desc_t* descs,
                                    int16_t* coef, int64_t coef_bytes, int64_t* totals, int32_t* rounds);

#ifdef __cplusplus
}
#endif
#endif /* POEM_HIP_H */
