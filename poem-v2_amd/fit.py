"""Fit MANO pose, shape and translation to a mesh, to 3-D joints and to 2-D keypoints in calibrated views on the MI355X
(include/poem_hip.h ``poem_mano_fit`` / ``poem_mano_fit_terms``; csrc/mano_fit.hip).

Upstream offers the MANO parameters of a frame only offline (lib/fit/frame_fit/one_frame_fit.py: hundreds of Adam steps per frame on
the host, through manotorch, on 2-D keypoints in N views).  Here: Levenberg-Marquardt on ``x = (pose_aa[48], betas[10], tsl[3])``
with the analytic Jacobian, every step fp64 on the device, no host synchronisation.  The model is the layer's mesh NOT centred
(whatever the layer's ``center_idx``) plus ``tsl``.  No CPU fallback.

The cost has up to three data terms (the header states them): the mesh, ``joints`` (B,21,3) with per-joint weights, and ``keypoints``
(sum(cam_view_num),21,2) in pixels with per-view, per-joint weights, projected by the batch's ``target_cam_intr`` /
``target_cam_extr`` and divided by ``image_scale``.  Keypoints alone determine the joints, NOT the twist of the bones nor (on
synthetic assets) the betas: judge such a fit by its joints and cost, its vertices only where a mesh term is present.

Not built: silhouette terms, per-vertex weights, PCA pose, left hands, a backward pass, graph capture of the fit; upstream's
quaternion-norm and anatomical axis losses."""
import ctypes
import math
from collections import namedtuple

import torch

from . import hip
from .triangulation import _offsets

ManoFit = namedtuple("ManoFit", ["pose_aa", "betas", "tsl", "verts", "joints", "cost", "accepted", "status"])
NV, NX, MAX_ITERS = 778, 61, 64
MAX_VIEWS = 65535
STATUS_TARGET_NOT_FINITE, STATUS_START_NOT_FINITE, STATUS_KEYPOINT_BEHIND_CAMERA = 1, 2, 4


def _number(name, v, positive=False):
    if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v) or v < 0 or (positive and not v > 0):
        raise ValueError(f"fit_mano: {name} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")


def _tensor(name, t, shape, ref):
    """``t`` is a float32 tensor of ``shape`` on ``ref``'s device"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"fit_mano: {name} must be a tensor, got {type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"fit_mano: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"fit_mano: {name} must be float32, got {t.dtype}")
    if t.device != ref.device:
        raise ValueError(f"fit_mano: {name} is on {t.device}, the layer is on {ref.device}")


def check_fit_arguments(table, verts, iters, init, shape_reg, pose_reg, joints=None, joint_weights=None, keypoints=None,
                        keypoint_weights=None, cam_intr=None, cam_extr=None, cam_view_num=None, image_scale=None, mesh_weight=1.0):
    """Everything ``fit_mano`` refuses, before a launch or an allocation: raises, or returns ``(batch, iters)``."""
    if not isinstance(table, torch.Tensor):
        raise TypeError("fit_mano: `layer` must be a poem_v2_amd.ManoLayer (it carries the prepared asset table `th_table`)")
    if verts is None and joints is None and keypoints is None:
        raise ValueError("fit_mano: at least one of verts, joints, keypoints must be given")
    if verts is not None:
        if not isinstance(verts, torch.Tensor):
            raise TypeError(f"fit_mano: verts must be a tensor, got {type(verts).__name__}")
        if verts.dim() != 3 or tuple(verts.shape[1:]) != (NV, 3):
            raise ValueError(f"fit_mano: verts must be (B,{NV},3), got {tuple(verts.shape)}")
        if verts.dtype != torch.float32:
            raise TypeError(f"fit_mano: verts must be float32, got {verts.dtype}")
        if verts.device != table.device:
            raise ValueError(f"fit_mano: verts are on {verts.device}, the layer is on {table.device}")
        B = int(verts.shape[0])
        _number("mesh_weight", mesh_weight)
    elif joints is not None:
        if not isinstance(joints, torch.Tensor) or joints.dim() != 3:
            raise ValueError("fit_mano: joints must be a (B,21,3) tensor")
        B = int(joints.shape[0])
    else:
        if cam_view_num is None:
            raise ValueError("fit_mano: keypoints need cam_intr, cam_extr, cam_view_num and image_scale")
        B = len(cam_view_num)
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"fit_mano: iters must be an int in 0..{MAX_ITERS}, got {iters!r}")
    _number("shape_reg", shape_reg)
    _number("pose_reg", pose_reg)
    if init is not None:
        if not isinstance(init, torch.Tensor):
            raise TypeError(f"fit_mano: init must be a (B,{NX}) tensor or None, got {type(init).__name__}")
        if tuple(init.shape) != (B, NX):
            raise ValueError(f"fit_mano: init must be ({B},{NX}) = (pose_aa | betas | tsl), got {tuple(init.shape)}")
        if init.dtype != torch.float32:
            raise TypeError(f"fit_mano: init must be float32, got {init.dtype}")
        if init.device != table.device:
            raise ValueError(f"fit_mano: init is on {init.device}, {'verts are' if verts is not None else 'the layer is'} on {table.device}")
    if joints is None:
        if joint_weights is not None:
            raise ValueError("fit_mano: joint_weights without joints")
    else:
        _tensor("joints", joints, (B, 21, 3), table)
        if joint_weights is not None:
            _tensor("joint_weights", joint_weights, (B, 21), table)
    if keypoints is None:
        extra = [n for n, v in (("keypoint_weights", keypoint_weights), ("cam_intr", cam_intr), ("cam_extr", cam_extr),
                                ("cam_view_num", cam_view_num), ("image_scale", image_scale)) if v is not None]
        if extra:
            raise ValueError(f"fit_mano: {', '.join(extra)} without keypoints")
    else:
        missing = [n for n, v in (("cam_intr", cam_intr), ("cam_extr", cam_extr), ("cam_view_num", cam_view_num),
                                  ("image_scale", image_scale)) if v is None]
        if missing:
            raise ValueError(f"fit_mano: keypoints need cam_intr, cam_extr, cam_view_num and image_scale ({', '.join(missing)} missing)")
        views = [int(v) for v in cam_view_num]
        if len(views) != B or any(v < 0 for v in views):
            raise ValueError(f"fit_mano: cam_view_num must hold {B} view counts >= 0, got {views}")
        total = sum(views)
        if total > MAX_VIEWS:
            raise ValueError(f"fit_mano: {total} views in one call; at most {MAX_VIEWS}")
        _tensor("keypoints", keypoints, (total, 21, 2), table)
        _tensor("cam_intr", cam_intr, (total, 3, 3), table)
        _tensor("cam_extr", cam_extr, (total, 4, 4), table)
        if keypoint_weights is not None:
            _tensor("keypoint_weights", keypoint_weights, (total, 21), table)
        _number("image_scale", image_scale, positive=True)
        if verts is None and joints is None and init is None:
            raise ValueError("fit_mano: keypoints alone give no start: pass init (B,61)")
    return B, int(iters)


def fit_mano(layer, verts=None, *, iters=8, init=None, shape_reg=0.0, pose_reg=0.0, joints=None, joint_weights=None, keypoints=None,
             keypoint_weights=None, cam_intr=None, cam_extr=None, cam_view_num=None, image_scale=None, mesh_weight=1.0):
    """``layer``: a :class:`poem_v2_amd.ManoLayer`; ``verts`` (B,778,3) fp32 on the layer's device, or None; ``init`` None (the rigid
    alignment of the template is the start) or (B,61) fp32 ``(pose_aa | betas | tsl)`` -> :class:`ManoFit` of device tensors:
    ``pose_aa`` (B,48), ``betas`` (B,10), ``tsl`` (B,3), the fitted ``verts`` (B,778,3) and ``joints`` (B,21,3), ``cost`` (B,) fp64
    (sum of squared residuals plus the regularisers), ``accepted`` (B,) int32 steps, ``status`` (B,) int32 (0; bit 0: an input is
    not finite or a weight not valid, bit 1: the start is not finite, bit 2: the start has a weighted keypoint behind its camera
    -- such a sample returns its start).

    ``joints`` (B,21,3) with ``joint_weights`` (B,21; ones by default) adds ``sum w |P_j - joints_j|^2``; ``keypoints``
    (sum(cam_view_num),21,2) in pixels with ``keypoint_weights`` (same,21; ones by default), ``cam_intr`` (.,3,3), ``cam_extr``
    (.,4,4) camera->master, ``cam_view_num`` (host ints, views per sample; 0 allowed) and ``image_scale`` adds
    ``sum w |(project(P_j) - keypoints_j) / image_scale|^2``; ``mesh_weight`` scales the mesh term.  A weight of 0 switches its
    entry off whatever it holds (NaN included).  Keypoints alone need ``init``.  With none of these arguments the call is
    ``poem_mano_fit``, as before."""
    table = getattr(layer, "th_table", None)
    B, iters = check_fit_arguments(table, verts, iters, init, shape_reg, pose_reg, joints, joint_weights, keypoints, keypoint_weights,
                                   cam_intr, cam_extr, cam_view_num, image_scale, mesh_weight)
    if not table.is_cuda:
        raise RuntimeError("fit_mano runs on the MI355X HIP path only (no CPU fallback)")
    dev = table.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = ManoFit(torch.empty(B, 48, **f32), torch.empty(B, 10, **f32), torch.empty(B, 3, **f32), torch.empty(B, NV, 3, **f32),
                  torch.empty(B, 21, 3, **f32), torch.empty(B, dtype=torch.float64, device=dev),
                  torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    if B == 0:
        return out
    L = hip.lib()
    tgt = None if verts is None else verts.detach().contiguous()
    x0 = None if init is None else init.detach().contiguous()
    outs = (hip.ptr(out.pose_aa), hip.ptr(out.betas), hip.ptr(out.tsl), hip.ptr(out.verts), hip.ptr(out.joints), out.cost.data_ptr(),
            out.accepted.data_ptr(), out.status.data_ptr())
    if joints is None and keypoints is None and mesh_weight == 1.0:
        need = L.poem_mano_fit_workspace_bytes(B)
        ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            hip.check(L.poem_mano_fit(hip.ptr(table), hip.ptr(tgt), hip.ptr(x0), B, iters, float(shape_reg), float(pose_reg),
                                      ws.data_ptr(), need, *outs, hip.stream()), "poem_mano_fit")
        return out
    keep = [tgt, x0]                              # the tensors the struct points into stay referenced until the call returns
    terms = hip.PoemManoFitTerms()
    terms.target_verts, terms.mesh_weight = hip.ptr(tgt), float(mesh_weight)
    if joints is not None:
        j3 = joints.detach().contiguous()
        w3 = torch.ones(B, 21, **f32) if joint_weights is None else joint_weights.detach().contiguous()
        keep += [j3, w3]
        terms.joints3d, terms.joints3d_weight = hip.ptr(j3), hip.ptr(w3)
    if keypoints is not None:
        kp, K, T = keypoints.detach().contiguous(), cam_intr.detach().contiguous(), cam_extr.detach().contiguous()
        w2 = torch.ones(kp.shape[0], 21, **f32) if keypoint_weights is None else keypoint_weights.detach().contiguous()
        offs = _offsets(cam_view_num, dev)
        keep += [kp, K, T, w2, offs]
        # (an empty tensor's data_ptr is 0, which the library would read as "absent": no view at all is still term K)
        p = lambda t: hip.ptr(t) or hip.ptr(table)                            # noqa: E731
        terms.keypoints, terms.keypoint_weight, terms.cam_intr, terms.cam_extr = p(kp), p(w2), p(K), p(T)
        terms.view_offsets, terms.total_views, terms.image_scale = offs.data_ptr(), int(kp.shape[0]), float(image_scale)
    need = L.poem_mano_fit_terms_workspace_bytes(B)
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.check(L.poem_mano_fit_terms(hip.ptr(table), ctypes.byref(terms), hip.ptr(x0), B, iters, float(shape_reg), float(pose_reg),
                                        ws.data_ptr(), need, *outs, hip.stream()), "poem_mano_fit_terms")
    return out
