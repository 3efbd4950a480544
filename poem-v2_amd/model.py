"""``PtEmbedMultiviewStereoV2`` -- the caller of the hot path, inference side only (lib/models/POEM.py:39-332 upstream):
images -> backbone pyramid (HRNet, or ResNet-18 / 34 / 50 by ``BACKBONE.TYPE``) -> ``feat_decode`` / ``heatmap_stage`` -> ragged
DLT -> ``POEM_Generalized_Head`` -> the ``preds`` dict the reference's ``_forward_impl`` returns (same keys).

Which part runs where: the backbone is plain PyTorch-ROCm (backbone.py; out of the hot path), everything after it is
the HIP path (decode.py, triangulation.py, head.py -> libpoem_hip.so).  Training-mode noise on the reference joints
(POEM.py:272-281), gradients and summaries are not built; with a ``LOSS`` node in the config,
``compute_loss`` gives the VALUE of upstream's losses for a forward's ``preds`` (losses.py, forward only)."""
import numpy as np
import torch

from . import resnet  # noqa: F401  (registers ResNet18 / ResNet34 / ResNet50)
from .backbone import HRNet  # noqa: F401
from .builder import BACKBONE, MODEL, CN, build_head
from .decode import FEAT_SIZES, FeatureDecoders
from .fit import MAX_ITERS as MAX_FIT_ITERS, fit_mano
from .losses import LossMetric, PoemLoss
from .mano import ManoLayer
from .triangulation import triangulate_reference_joints


DLT_CONFIDENCE_MODES = ("off", "threshold", "weighted", "ransac")


def head_in_channels(backbone_name):
    """channels of the map ``feat_decode`` hands the head: feat_in's output (POEM.py:68-73,94-99) -- 160 / 128 / 512"""
    f = FEAT_SIZES[backbone_name]
    return f[2] if backbone_name == "HRNet" else f[1]


def build_img_backbone(cfg, device):
    """``cfg.TYPE`` through the BACKBONE registry (POEM.py:47); a missing node or TYPE means HRNet"""
    kind = "HRNet" if cfg is None or cfg.get("TYPE", None) is None else cfg.get("TYPE")
    cls = BACKBONE.get(kind) if isinstance(kind, str) else kind
    if cls is None:
        raise KeyError(f"{kind} is not in the {BACKBONE.name} registry")
    net = cls(cfg, device=device)
    if getattr(net, "name", None) not in FEAT_SIZES:                      # POEM.py:49
        raise ValueError(f"backbone {getattr(net, 'name', kind)!r}: the model takes one of {sorted(FEAT_SIZES)}")
    return net


def fit_keypoint_weight(cfg):
    """The model key FIT_MANO_KEYPOINTS -> weight_2d (0.0: off).  It must be a finite number >= 0 and needs FIT_MANO."""
    w2d = cfg.get("FIT_MANO_KEYPOINTS", None)
    if w2d is not None and (isinstance(w2d, (bool, str)) or not isinstance(w2d, (int, float)) or not np.isfinite(w2d) or w2d < 0):
        raise ValueError(f"FIT_MANO_KEYPOINTS = {w2d!r} must be a finite number >= 0 (the weight of the 2-D term; 0: off)")
    w2d = float(w2d or 0.0)
    if w2d > 0 and not bool(cfg.get("FIT_MANO", False)):
        raise ValueError("FIT_MANO_KEYPOINTS needs FIT_MANO")
    return w2d


@MODEL.register_module()
class PtEmbedMultiviewStereoV2:

    def __init__(self, cfg, device="cuda:0"):
        if not torch.cuda.is_available():
            raise RuntimeError("PtEmbedMultiviewStereoV2 runs on the MI355X HIP path only (no CPU fallback)")
        self.name = type(self).__name__
        self.cfg = cfg
        self.device = torch.device(cfg.get("DEVICE", device))
        preset = cfg.get("DATA_PRESET", CN({}))
        self.center_idx = int(preset.get("CENTER_IDX", 9))                       # POEM.py:50
        self.num_joints = 21
        self.img_backbone = build_img_backbone(cfg.get("BACKBONE", None), self.device)   # POEM.py:47
        self.ptEmb_head = build_head(cfg.HEAD, data_preset=preset)                # POEM.py:114
        want = head_in_channels(self.img_backbone.name)
        if getattr(self.ptEmb_head, "in_channels", None) is not None and int(self.ptEmb_head.in_channels) != want:
            raise ValueError(f"HEAD.IN_CHANNELS = {self.ptEmb_head.in_channels}, but the {self.img_backbone.name} backbone's "
                             f"feat_decode gives the head {want} channels")
        self.num_preds = self.ptEmb_head.num_preds
        # MANO_ASSETS at the model node (the same .npz path as MODEL.HEAD.MANO_ASSETS) reaches the head unless the head's own node
        # names some (head.py: template and MANO layer from them)
        if cfg.get("MANO_ASSETS", None) and not cfg.HEAD.get("MANO_ASSETS", None):
            self.ptEmb_head.set_mano_assets(cfg.get("MANO_ASSETS"))
            self.ptEmb_head.mano_assets_source = f"config:{cfg.get('MANO_ASSETS')}"       # (a config key, not a caller's call)
        # confidence-aware DLT (upstream's triangulate_dlt, lib/utils/triangulation.py:111-148): "off" | "threshold" | "weighted";
        # "ransac" (no upstream counterpart): views that disagree with the others' geometry are left out (triangulation.py).
        # DLT_INLIER_PX: the inlier radius in image pixels; the default 8.0 is two heat-map pixels at 256^2 images with 64^2 maps
        # and has NOT been measured on real data.  DLT_REFINE_ITERS: Gauss-Newton steps on the reprojection error (0..16)
        self.dlt_confidence = str(cfg.get("DLT_CONFIDENCE", "off")).lower()
        self.dlt_threshold = float(cfg.get("DLT_CONFIDENCE_THRESHOLD", 0.5))
        self.dlt_inlier_px = float(cfg.get("DLT_INLIER_PX", 8.0))
        self.dlt_refine_iters = int(cfg.get("DLT_REFINE_ITERS", 0))
        if self.dlt_confidence not in DLT_CONFIDENCE_MODES:
            raise ValueError(f"DLT_CONFIDENCE {self.dlt_confidence!r}: expected one of {DLT_CONFIDENCE_MODES}")
        if not self.dlt_inlier_px > 0 or not 0 <= self.dlt_refine_iters <= 16:
            raise ValueError(f"DLT_INLIER_PX = {self.dlt_inlier_px} must be > 0 and DLT_REFINE_ITERS = {self.dlt_refine_iters} in 0..16")
        # FIT_MANO (absent / false by default; no upstream counterpart in the forward: lib/fit/frame_fit/one_frame_fit.py fits offline):
        # MANO pose, shape and translation of the last layer's predicted vertices, fitted on the device after the forward (fit.py);
        # FIT_MANO_ITERS Levenberg-Marquardt iterations (0..64).  Needs the MANO assets (MANO_ASSETS here or at the head, or
        # set_mano_assets() before construction ends -- an importable manotorch counts).
        self.fit_mano = bool(cfg.get("FIT_MANO", False))
        self.fit_mano_iters = int(cfg.get("FIT_MANO_ITERS", 8))
        self._fit_layer = self._fit_layer_assets = None
        # FIT_MANO_KEYPOINTS (a float weight_2d; absent or 0: off): the fit also pulls its 21 joints onto the forward's own 2-D joints
        # in every view (fit.py term K): weight = weight_2d x pred_joints_conf (where the DLT mode reads confidences) x
        # pred_joints_inlier (where it is "ransac"), image_scale = max(H, W), the batch's cameras.  Its useful range on real data
        # has NOT been measured.
        self.fit_mano_keypoints = fit_keypoint_weight(cfg)
        if self.fit_mano:
            if not 0 <= self.fit_mano_iters <= MAX_FIT_ITERS:
                raise ValueError(f"FIT_MANO_ITERS = {self.fit_mano_iters} must be in 0..{MAX_FIT_ITERS}")
            if self.ptEmb_head._mano_assets is None:
                raise ValueError("FIT_MANO needs the MANO assets: set MANO_ASSETS (an .npz of v_template, shapedirs, posedirs, "
                                 "J_regressor, weights) at the model or its head")
        self.decoders = None
        # optional LOSS node (POEM.py:41-45,125-146): the loss VALUE of a forward; absent -> compute_loss raises, nothing else changes
        self.loss = None
        if cfg.get("LOSS", None) is not None:
            tr = cfg.HEAD.get("TRANSFORMER", CN({}))
            self.loss = PoemLoss(cfg.LOSS, parametric=bool(tr.get("PARAMETRIC_OUTPUT", False)),
                                 transformer_center_idx=int(tr.get("TRANSFORMER_CENTER_IDX", 9)))
        self.loss_metric = LossMetric(cfg)                                        # POEM.py:146 (allocates at its first feed)

    # -- weights ----------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd, strict=True):
        """Full-model checkpoint in the reference's key names: ``img_backbone.*``, ``feat_delayer.*`` / ``feat_in.*`` /
        ``uv_delayer.*`` / ``uv_out.*``, ``ptEmb_head.*`` (optionally behind ``module.``, as upstream's ``load_weights`` strips
        it).  The head takes the strict path of ``nn.Module.load_state_dict``: exactly the reference's dead tensors are
        swallowed (``weights.is_dead_reference_key``); an unknown ``ptEmb_head.*`` key, a missing live tensor or a live tensor
        of the wrong shape raises.  Returns the keys that were ignored (dead tensors)."""
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        ignored = self.img_backbone.load_state_dict(sd, prefix="img_backbone.")
        self.decoders = FeatureDecoders.load_reference_state_dict(sd, self.device, backbone=self.img_backbone.name)
        head_sd = {k[len("ptEmb_head."):]: v for k, v in sd.items() if k.startswith("ptEmb_head.")}
        self.ptEmb_head.load_state_dict(head_sd, strict=strict)
        ignored += ["ptEmb_head." + k for k in self.ptEmb_head.ignored_reference_keys]
        self.ptEmb_head.to(self.device).eval()
        return ignored

    def load_parts(self, backbone_sd, decoder_sd, head_sd, template=None):
        self.img_backbone.load_state_dict(backbone_sd)
        self.decoders = FeatureDecoders(decoder_sd, self.device, self.img_backbone.name)
        self.ptEmb_head.load_state_dict(head_sd, strict=False)
        if template is not None:
            self.ptEmb_head.set_template(template)
        self.ptEmb_head.to(self.device).eval()
        return self

    # -- losses (value only) ------------------------------------------------------------------------------------------
    def set_j_regressor(self, j_regressor):
        """MANO's ``th_J_regressor`` (16,778) for ``loss_3d_joints_from_mesh`` -- an input, the asset is licence-gated."""
        if self.loss is None:
            raise RuntimeError("set_j_regressor: the model was built without a LOSS node")
        self.loss.set_j_regressor(j_regressor)
        return self

    def compute_loss(self, preds, gt):
        """``(loss, loss_dict)`` of upstream's ``compute_loss`` (POEM.py:363-466) as 0-dim fp64 device tensors; no backward pass."""
        if self.loss is None:
            raise RuntimeError("compute_loss: the model was built without a LOSS node (cfg.LOSS, as in config/release/train_*.yaml)")
        return self.loss(preds, gt)

    # -- forward ----------------------------------------------------------------------------------------------------
    def extract_img_feat(self, img):
        return self.img_backbone(img)                                            # POEM.py:246

    @torch.no_grad()
    def _forward_impl(self, batch, **kwargs):
        """batch: ``image`` (BN,3,H,W), ``target_cam_intr`` (BN,3,3), ``target_cam_extr`` (BN,4,4), ``master_id``,
        ``cam_view_num`` (B,), ``master_joints_3d`` (only read when every sample has one view)   [POEM.py:250-332]"""
        if kwargs.get("mode", "test") == "train":
            raise NotImplementedError("training mode is outside the built path")
        img = batch["image"]
        img = img.view(-1, img.shape[-3], img.shape[-2], img.shape[-1]).to(self.device)
        views = np.asarray(batch["cam_view_num"]).astype(np.int64)
        batch_size, BN = len(views), img.shape[0]
        H, W = img.shape[-2:]
        img_feats = self.extract_img_feat(img)
        mlvl_feat = self.decoders.feat_decode(img_feats, self.img_backbone.name)            # :267
        conf = inlier = reproj = None
        if self.dlt_confidence in ("off", "ransac"):
            uv_pred = self.decoders.heatmap_stage(img_feats, W, H)                          # :270
        else:
            uv_pred, conf = self.decoders.heatmap_stage(img_feats, W, H, return_conf=True)
        K = batch["target_cam_intr"].reshape(-1, 3, 3).to(self.device)
        T = batch["target_cam_extr"].reshape(-1, 4, 4).to(self.device)
        if BN == batch_size:                                                                # :273,282-283
            ref_joints = batch["master_joints_3d"].reshape(-1, 21, 3).to(self.device)
        else:
            if views.min() < 2:
                raise ValueError("a batch mixing single-view and multi-view samples has no DLT solution for the former "
                                 "(upstream's SVD returns the null vector of a rank-2 system there)")
            if self.dlt_confidence == "ransac":
                ref_joints, inlier, reproj = triangulate_reference_joints(uv_pred, K, T, views, mode="ransac",
                                                                          inlier_px=self.dlt_inlier_px,
                                                                          refine=self.dlt_refine_iters, return_inliers=True)
            else:
                ref_joints = triangulate_reference_joints(uv_pred, K, T, views, conf=conf,  # :284-299
                                                          mode=None if conf is None else self.dlt_confidence,
                                                          threshold=self.dlt_threshold)
        img_metas = {"inp_img_shape": (H, W), "cam_intr": K, "cam_extr": T, "master_id": batch["master_id"],
                     "cam_view_num": views}
        preds = self.ptEmb_head(mlvl_feat=mlvl_feat, img_metas=img_metas, reference_joints=ref_joints)
        j = preds["all_coords_preds"][-1, :, :self.num_joints, :]
        v = preds["all_coords_preds"][-1, :, self.num_joints:, :]
        centre = j[:, self.center_idx, :].unsqueeze(1)
        preds.update(pred_joints_3d=j, pred_verts_3d=v, pred_joints_3d_rel=j - centre, pred_verts_3d_rel=v - centre,
                     pred_joints_uv=uv_pred, pred_ref_joints_3d=ref_joints)                 # :321-331
        if conf is not None:
            preds["pred_joints_conf"] = conf
        if inlier is not None:
            preds.update(pred_joints_inlier=inlier, pred_joints_reproj=reproj)
        if self.fit_mano and self.fit_mano_keypoints > 0:
            w2 = torch.full(uv_pred.shape[:2], self.fit_mano_keypoints, dtype=torch.float32, device=uv_pred.device)
            if conf is not None:
                w2 = w2 * conf
            if inlier is not None:
                w2 = torch.where(inlier, w2, torch.zeros_like(w2))
            fit = fit_mano(self._mano_fit_layer(), v.contiguous(), iters=self.fit_mano_iters, keypoints=uv_pred.float().contiguous(),
                           keypoint_weights=w2, cam_intr=K.float().contiguous(), cam_extr=T.float().contiguous(),
                           cam_view_num=views, image_scale=float(max(H, W)))
            preds.update(pred_mano_pose=fit.pose_aa, pred_mano_shape=fit.betas, pred_mano_tsl=fit.tsl, pred_mano_verts=fit.verts,
                         pred_mano_status=fit.status, pred_mano_joints=fit.joints, pred_mano_keypoint_weight=w2)
        elif self.fit_mano:
            fit = fit_mano(self._mano_fit_layer(), v.contiguous(), iters=self.fit_mano_iters)
            preds.update(pred_mano_pose=fit.pose_aa, pred_mano_shape=fit.betas, pred_mano_tsl=fit.tsl, pred_mano_verts=fit.verts,
                         pred_mano_status=fit.status)
        return preds

    def _mano_fit_layer(self):
        """The uncentred layer the fit reads its table from, built once from the head's assets (again if they were replaced)."""
        assets = self.ptEmb_head._mano_assets
        if assets is None:
            raise RuntimeError("FIT_MANO: the head has no MANO assets any more")
        if self._fit_layer is None or self._fit_layer_assets is not assets:
            self._fit_layer = ManoLayer.from_arrays(**assets, center_idx=None, device=self.device)
            self._fit_layer_assets = assets
        return self._fit_layer

    def testing_step(self, batch, step_idx=0, **kwargs):
        return self._forward_impl(batch, mode="test", **kwargs)

    def inference_step(self, batch, step_idx=0, **kwargs):
        return self._forward_impl(batch, mode="inference", **kwargs)

    def forward(self, inputs, step_idx=0, mode="test", **kwargs):                           # POEM.py:486-496
        if mode in ("val", "test"):
            return self.testing_step(inputs, step_idx, **kwargs)
        if mode == "inference":
            return self.inference_step(inputs, step_idx, **kwargs)
        raise ValueError(f"mode {mode} is not built (inference side only)")

    __call__ = forward
