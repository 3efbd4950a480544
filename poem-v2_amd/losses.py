"""The reference's training losses, evaluated on the device -- the VALUE only, there is no backward pass.

``PoemLoss`` is ``PtEmbedMultiviewStereoV2.compute_loss`` with ``loss_proj_to_multicam`` (lib/models/POEM.py:336-466 upstream): same
``LOSS`` keys and defaults (:41-42,125-131), same argument dicts, same keys of ``loss_dict`` in the same order.  Upstream loops over
the samples in Python -- two batched matmuls and a ``torch.linalg.inv`` each; here ``poem_loss_terms`` computes every term for the
ragged batch in one launch plus a one-block finalize (csrc/loss.hip), in fp64 throughout, and the values are 0-dim fp64 views into
its result buffer (upstream's are fp32).  ``LossMetric`` is upstream's class of that name
(lib/metrics/basic_metric.py:63-97) with the sums kept in one device tensor instead of one ``.item()`` per key and step."""
import ctypes

import torch

from . import dist as pdist

# upstream's order of insertion into loss_dict (POEM.py:380,451-465)
LOSS_KEYS = ("loss_heatmap_joints", "loss_3d_joints", "loss_3d_joints_from_mesh", "loss_3d_verts", "loss_recon", "loss_2d_joints",
             "loss_2d_verts", "loss_pose", "loss_shape", "loss")


def _dev32(t, device):
    return torch.as_tensor(t).detach().to(device=device, dtype=torch.float32).contiguous()


class PoemLoss:
    """``loss, loss_dict = PoemLoss(cfg.LOSS, parametric, transformer_center_idx, j_regressor)(preds, gt)``.

    ``loss_cfg``: upstream's ``LOSS`` node.  ``JOINTS_LOSS_WEIGHT``, ``VERTICES_LOSS_WEIGHT``, ``JOINTS_2D_LOSS_WEIGHT`` and
    ``HEATMAP_JOINTS_WEIGHT`` are required, as upstream; ``JOINTS_LOSS_TYPE`` "l2", ``VERTICES_LOSS_TYPE`` "l1",
    ``VERTICES_2D_LOSS_WEIGHT`` 0.0, ``POSE_LOSS_WEIGHT`` 0.001 and ``SHAPE_LOSS_WEIGHT`` 0.0005 are its defaults.
    ``TRIANGULATED_JOINTS_WEIGHT`` and ``EDGE_LOSS_WEIGHT`` stand in the release YAML (config/release/train_medium.yaml:230,235) but
    ``compute_loss`` never reads them: accepted and ignored.
    ``j_regressor``: MANO's ``th_J_regressor`` (16,778) -- an input, the asset is licence-gated.

    ``preds``: ``all_coords_preds`` (L,B,799,3), ``pred_joints_uv`` (BN,21,2), ``pred_pose`` (B,16,3) / ``pred_shape`` (B,10) when
    parametric.  ``gt``: ``cam_view_num``, ``master_joints_3d``, ``master_verts_3d``, ``target_joints_2d``, ``target_cam_intr``,
    ``target_cam_extr``, ``mano_pose`` / ``mano_shape`` per view when parametric, and ``image`` (or ``inp_img_shape`` = (H, W)).
    ``loss_2d_joints`` / ``loss_2d_verts`` appear only at a non-zero weight, ``loss_pose`` / ``loss_shape`` only when parametric.
    Stream-ordered: no ``.item()``, no synchronisation.  No CPU fallback."""

    def __init__(self, loss_cfg, parametric=False, transformer_center_idx=9, j_regressor=None):
        c = loss_cfg
        self.joints_loss_type = c.get("JOINTS_LOSS_TYPE", "l2")                          # POEM.py:41-42
        self.verts_loss_type = c.get("VERTICES_LOSS_TYPE", "l1")
        self.joints_weight = float(c["JOINTS_LOSS_WEIGHT"])                              # :125-131
        self.vertices_weight = float(c["VERTICES_LOSS_WEIGHT"])
        self.joints_2d_weight = float(c["JOINTS_2D_LOSS_WEIGHT"])
        self.heatmap_joints_weights = float(c["HEATMAP_JOINTS_WEIGHT"])
        self.vertices_2d_weight = float(c.get("VERTICES_2D_LOSS_WEIGHT", 0.0))
        self.pose_weight = float(c.get("POSE_LOSS_WEIGHT", 0.001))
        self.shape_weight = float(c.get("SHAPE_LOSS_WEIGHT", 0.0005))
        self.parametric_output = bool(parametric)
        self.transformer_center_idx = int(transformer_center_idx)
        self.j_regressor = None
        self._workspace = None
        if j_regressor is not None:
            self.set_j_regressor(j_regressor)

    def set_j_regressor(self, j_regressor):
        w = torch.as_tensor(j_regressor).detach().to(torch.float32)
        if tuple(w.shape) != (16, 778):
            raise ValueError(f"J_regressor must be (16,778), got {tuple(w.shape)}")
        self.j_regressor = w.contiguous()
        return self

    def keys(self):
        """The keys of ``loss_dict`` for this configuration, in upstream's order."""
        skip = set()
        if self.joints_2d_weight == 0:
            skip.add("loss_2d_joints")
        if self.vertices_2d_weight == 0:
            skip.add("loss_2d_verts")
        if not self.parametric_output:
            skip.update(("loss_pose", "loss_shape"))
        return [k for k in LOSS_KEYS if k not in skip]

    @staticmethod
    def _image_size(gt):
        if gt.get("image") is not None:
            return int(gt["image"].shape[-2]), int(gt["image"].shape[-1])                # POEM.py:369-370
        if gt.get("inp_img_shape") is not None:
            h, w = gt["inp_img_shape"]
            return int(h), int(w)
        raise KeyError("PoemLoss needs the image size for img_scale: gt['image'] (BN,3,H,W) or gt['inp_img_shape'] = (H, W)")

    def __call__(self, preds, gt):
        from . import hip
        from .triangulation import _offsets
        coords = preds["all_coords_preds"]
        if self.j_regressor is None:
            raise RuntimeError("PoemLoss needs MANO's th_J_regressor (16,778) for loss_3d_joints_from_mesh: it is an input, the asset is "
                               "licence-gated -- pass j_regressor= to PoemLoss or call set_j_regressor(t)")
        if not coords.is_cuda:
            raise RuntimeError("PoemLoss runs on the MI355X HIP path only (no CPU fallback)")
        dev = coords.device
        if self.j_regressor.device != dev:
            self.j_regressor = self.j_regressor.to(dev)
        views = [int(v) for v in gt["cam_view_num"]]
        B, BN = len(views), int(sum(views))
        H, W = self._image_size(gt)
        last = _dev32(coords[-1], dev)
        tensors = {"all_coords_preds[-1]": (last, (B, 799, 3)),
                   "pred_joints_uv": (_dev32(preds["pred_joints_uv"], dev), (BN, 21, 2)),
                   "master_joints_3d": (_dev32(gt["master_joints_3d"], dev).reshape(-1, 21, 3), (B, 21, 3)),
                   "master_verts_3d": (_dev32(gt["master_verts_3d"], dev).reshape(-1, 778, 3), (B, 778, 3)),
                   "target_joints_2d": (_dev32(gt["target_joints_2d"], dev).reshape(-1, 21, 2), (BN, 21, 2)),
                   "target_cam_intr": (_dev32(gt["target_cam_intr"], dev).reshape(-1, 3, 3), (BN, 3, 3)),
                   "target_cam_extr": (_dev32(gt["target_cam_extr"], dev).reshape(-1, 4, 4), (BN, 4, 4))}
        if self.parametric_output:
            tensors.update({"pred_pose": (_dev32(preds["pred_pose"], dev).reshape(-1, 16, 3), (B, 16, 3)),
                            "pred_shape": (_dev32(preds["pred_shape"], dev).reshape(-1, 10), (B, 10)),
                            "mano_pose": (_dev32(gt["mano_pose"], dev).reshape(-1, 16, 3), (BN, 16, 3)),
                            "mano_shape": (_dev32(gt["mano_shape"], dev).reshape(-1, 10), (BN, 10))})
        # the C ABI takes raw pointers: a wrong-shaped tensor would be an out-of-bounds device read where upstream raises
        for name, (t, shape) in tensors.items():
            if tuple(t.shape) != shape:
                raise RuntimeError(f"{name} shape {tuple(t.shape)} != {shape} (cam_view_num sums to {BN} views, {B} samples)")
        p = {name: hip.ptr(t) for name, (t, _) in tensors.items()}
        cfg = hip.PoemLossCfg(self.joints_weight, self.vertices_weight, self.joints_2d_weight, self.vertices_2d_weight,
                              self.heatmap_joints_weights, self.pose_weight, self.shape_weight, int(self.joints_loss_type == "l2"),
                              int(self.verts_loss_type == "l2"), int(self.parametric_output), self.transformer_center_idx, H, W)
        L = hip.lib()
        need = L.poem_loss_workspace_bytes(B, BN)
        if need == 0:
            raise RuntimeError(f"poem_loss_workspace_bytes({B}, {BN}) failed")
        ws = self._workspace
        if ws is None or ws.device != dev or ws.numel() * 8 < need:      # grow-only; calls on one stream are ordered
            ws = self._workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(hip.LOSS_NTERMS, dtype=torch.float64, device=dev)
        offs = _offsets(views, dev)
        with torch.cuda.device(dev):
            hip.check(L.poem_loss_terms(p["all_coords_preds[-1]"], p["pred_joints_uv"], p.get("pred_pose"), p.get("pred_shape"),
                                        p["master_joints_3d"], p["master_verts_3d"], p["target_joints_2d"], p["target_cam_intr"],
                                        p["target_cam_extr"], offs.data_ptr(), p.get("mano_pose"), p.get("mano_shape"),
                                        hip.ptr(self.j_regressor), ctypes.byref(cfg), B, BN, out.data_ptr(), ws.data_ptr(),
                                        ws.numel() * 8, hip.stream()), "poem_loss_terms")
        loss_dict = {k: out[LOSS_KEYS.index(k)] for k in self.keys()}
        return loss_dict["loss"], loss_dict


class LossMetric:
    """Batch-size-weighted running averages of the entries of a ``loss_dict`` -- upstream's ``LossMetric``
    (lib/metrics/basic_metric.py:63-97: ``feed(losses, batch_size)``, ``get_measures()``, ``get_loss(name)``, ``reset()``, ``count``;
    every key is an ``AverageMeter`` fed with ``update_by_mean``).  The sums live in ONE fp64 tensor on the device of the values fed,
    [sum_k ... | n_k ... | count]; the host is touched in ``get_measures`` / ``get_loss`` only.  ``reduce()`` is one all-reduce of that
    tensor with ``MeanEPE.reduce``'s contract: the local sums are left alone, so reducing twice never double counts."""

    def __init__(self, cfg=None):
        self.cfg = cfg
        self.reset()

    def reset(self):
        self._names = []
        self.acc = None
        self._global = None
        self.count = 0

    def is_empty(self):
        return self.count == 0

    def num_sample(self):
        return self.count

    def feed(self, losses, batch_size=1, **kwargs):
        items = [(k, v) for k, v in losses.items() if isinstance(v, torch.Tensor)]      # None and non-tensors are passed over, as upstream
        if items:
            new = [k for k, _ in items if k not in self._names]
            dev = items[0][1].device
            if self.acc is None or new:
                old, n_old = self.acc, len(self._names)
                self._names += new
                K = len(self._names)
                self.acc = torch.zeros(2 * K + 1, dtype=torch.float64, device=dev)
                if old is not None:
                    self.acc[:n_old] = old[:n_old]
                    self.acc[K:K + n_old] = old[n_old:2 * n_old]
                    self.acc[-1] = old[-1]
            K = len(self._names)
            vals = torch.stack([v.detach().reshape(()).to(device=self.acc.device, dtype=torch.float64) for _, v in items])
            if [k for k, _ in items] == self._names:
                self.acc[:K] += vals * batch_size                                        # update_by_mean: sum += val * n
                self.acc[K:2 * K] += batch_size
            else:
                idx = torch.tensor([self._names.index(k) for k, _ in items], device=self.acc.device)
                self.acc[:K].index_add_(0, idx, vals * batch_size)
                self.acc[K:2 * K].index_add_(0, idx, torch.full_like(vals, float(batch_size)))
            self.acc[-1] += batch_size
        self.count += batch_size
        self._global = None

    def reduce(self):
        """all-reduce(sum) of a copy of [sums..., counts..., count] over the process group; every rank must have fed the same keys."""
        if self.acc is not None:
            self._global = pdist.all_reduce_sum_(self.acc.clone())
        return self

    def _averages(self):
        if self.acc is None:
            return {}
        a = (self.acc if self._global is None else self._global).tolist()
        K = len(self._names)
        return {k: a[i] / a[K + i] for i, k in enumerate(self._names)}

    def get_measures(self, **kwargs):
        return self._averages()

    def get_loss(self, loss_name):
        return self._averages()[loss_name]

    def __str__(self):
        return " | ".join(f"{k}: {v:.4e}" for k, v in self._averages().items())
