"""Fit MANO pose, shape and translation to a mesh on the MI355X (include/poem_hip.h ``poem_mano_fit``; csrc/mano_fit.hip).

Upstream offers the MANO parameters of a predicted mesh only offline (lib/fit/frame_fit/one_frame_fit.py: hundreds of Adam steps
per frame on the host, through manotorch).  Here: Levenberg-Marquardt on ``x = (pose_aa[48], betas[10], tsl[3])`` with the
analytic Jacobian, every step fp64 on the device, ``2 * iters + 4`` launches and no host synchronisation.  The model is the
layer's mesh NOT centred (whatever the layer's ``center_idx``) plus ``tsl``.  No CPU fallback.

Not built: 2-D keypoint / silhouette terms, joint targets, per-vertex weights, PCA pose, left hands, a backward pass, graph
capture of the fit."""
import math
from collections import namedtuple

import torch

from . import hip

ManoFit = namedtuple("ManoFit", ["pose_aa", "betas", "tsl", "verts", "joints", "cost", "accepted", "status"])
NV, NX, MAX_ITERS = 778, 61, 64
STATUS_TARGET_NOT_FINITE, STATUS_START_NOT_FINITE = 1, 2


def check_fit_arguments(table, verts, iters, init, shape_reg, pose_reg):
    """Everything ``fit_mano`` refuses, before a launch or an allocation: raises, or returns ``(batch, iters)``."""
    if not isinstance(table, torch.Tensor):
        raise TypeError("fit_mano: `layer` must be a poem_v2_amd.ManoLayer (it carries the prepared asset table `th_table`)")
    if not isinstance(verts, torch.Tensor):
        raise TypeError(f"fit_mano: verts must be a tensor, got {type(verts).__name__}")
    if verts.dim() != 3 or tuple(verts.shape[1:]) != (NV, 3):
        raise ValueError(f"fit_mano: verts must be (B,{NV},3), got {tuple(verts.shape)}")
    if verts.dtype != torch.float32:
        raise TypeError(f"fit_mano: verts must be float32, got {verts.dtype}")
    if verts.device != table.device:
        raise ValueError(f"fit_mano: verts are on {verts.device}, the layer is on {table.device}")
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"fit_mano: iters must be an int in 0..{MAX_ITERS}, got {iters!r}")
    for name, reg in (("shape_reg", shape_reg), ("pose_reg", pose_reg)):
        if not isinstance(reg, (int, float)) or isinstance(reg, bool) or not math.isfinite(reg) or reg < 0:
            raise ValueError(f"fit_mano: {name} must be a finite number >= 0, got {reg!r}")
    if init is not None:
        if not isinstance(init, torch.Tensor):
            raise TypeError(f"fit_mano: init must be a (B,{NX}) tensor or None, got {type(init).__name__}")
        if tuple(init.shape) != (verts.shape[0], NX):
            raise ValueError(f"fit_mano: init must be ({verts.shape[0]},{NX}) = (pose_aa | betas | tsl), got {tuple(init.shape)}")
        if init.dtype != torch.float32:
            raise TypeError(f"fit_mano: init must be float32, got {init.dtype}")
        if init.device != verts.device:
            raise ValueError(f"fit_mano: init is on {init.device}, verts are on {verts.device}")
    return int(verts.shape[0]), int(iters)


def fit_mano(layer, verts, *, iters=8, init=None, shape_reg=0.0, pose_reg=0.0):
    """``layer``: a :class:`poem_v2_amd.ManoLayer`; ``verts`` (B,778,3) fp32 on the layer's device; ``init`` None (the rigid
    alignment of the template is the start) or (B,61) fp32 ``(pose_aa | betas | tsl)`` -> :class:`ManoFit` of device tensors:
    ``pose_aa`` (B,48), ``betas`` (B,10), ``tsl`` (B,3), the fitted ``verts`` (B,778,3) and ``joints`` (B,21,3), ``cost`` (B,) fp64
    (sum of squared residuals plus the regularisers), ``accepted`` (B,) int32 steps, ``status`` (B,) int32 (0; bit 0: the target is
    not finite, bit 1: the start is not finite -- such a sample returns its start)."""
    table = getattr(layer, "th_table", None)
    B, iters = check_fit_arguments(table, verts, iters, init, shape_reg, pose_reg)
    if not verts.is_cuda:
        raise RuntimeError("fit_mano runs on the MI355X HIP path only (no CPU fallback)")
    dev = verts.device
    f32 = dict(dtype=torch.float32, device=dev)
    out = ManoFit(torch.empty(B, 48, **f32), torch.empty(B, 10, **f32), torch.empty(B, 3, **f32), torch.empty(B, NV, 3, **f32),
                  torch.empty(B, 21, 3, **f32), torch.empty(B, dtype=torch.float64, device=dev),
                  torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    if B == 0:
        return out
    L = hip.lib()
    tgt = verts.detach().contiguous()
    x0 = None if init is None else init.detach().contiguous()
    need = L.poem_mano_fit_workspace_bytes(B)
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        hip.check(L.poem_mano_fit(hip.ptr(table), hip.ptr(tgt), hip.ptr(x0), B, iters, float(shape_reg), float(pose_reg),
                                  ws.data_ptr(), need, hip.ptr(out.pose_aa), hip.ptr(out.betas), hip.ptr(out.tsl), hip.ptr(out.verts),
                                  hip.ptr(out.joints), out.cost.data_ptr(), out.accepted.data_ptr(), out.status.data_ptr(),
                                  hip.stream()), "poem_mano_fit")
    return out
