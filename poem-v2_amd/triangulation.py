"""DLT triangulation of the 21 joints from per-view 2-D predictions -- the stage that produces the head's
``reference_joints`` (lib/models/POEM.py:284-299 upstream).  MI355X-native: one ``poem_triangulate_dlt`` launch for the
whole ragged batch instead of a Python loop of per-sample ``torch.linalg.svd`` calls.  No CPU fallback.

``batch_triangulate_dlt_torch`` keeps the reference function's name, argument meaning and result
(lib/utils/triangulation.py:5-45); ``triangulate_reference_joints`` is the ragged, path-level form.

Confidence-aware forms (``poem_heatmap_uv_conf`` + ``poem_dlt_confidence``): ``heatmap_to_uv(..., return_conf=True)`` also
returns each joint's heat-map peak, ``triangulate_reference_joints(..., conf=, mode=)`` discounts views by it, and
``triangulate_dlt`` keeps the name, arguments and result of upstream's one-sample function (triangulation.py:111-148).

Outlier-robust form (``poem_dlt_robust``, ``mode="ransac"``): views whose 2-D joint disagrees with the geometry of the others are
left out of the solve, with optional Gauss-Newton refinement of the reprojection error.  Upstream has nothing like it; its
definition is ``include/poem_hip.h`` and the fp64 restatement in tests/dlt_robust_util.py."""
import numpy as np
import torch

from . import hip


_OFFS_CACHE = {}


def _offsets(views, device):
    """(B+1,) int32 view offsets on the device.  A repeating layout re-uses its device tensor; a new one is staged through
    pinned memory and copied without blocking (a pageable H2D copy would hold the host until the stream has drained, i.e.
    until the previous forward has finished -- the stall the head's own layout upload avoids, csrc/forward.cpp)."""
    key = (tuple(int(v) for v in views), str(device))
    hit = _OFFS_CACHE.get(key)
    if hit is None:
        offs = np.concatenate([[0], np.cumsum(np.asarray(key[0], dtype=np.int64))]).astype(np.int32)
        hit = torch.from_numpy(offs).pin_memory().to(device, non_blocking=True)
        if len(_OFFS_CACHE) >= 64:
            _OFFS_CACHE.pop(next(iter(_OFFS_CACHE)))
        _OFFS_CACHE[key] = hit
    return hit


def triangulate_reference_joints(uv, cam_intr, cam_extr, cam_view_num, conf=None, mode=None, threshold=0.5,
                                 return_count=False, invert=True, inlier_px=8.0, refine=0, return_inliers=False):
    """uv (BN,J,2) pixel coordinates per view, cam_intr (BN,3,3), cam_extr (BN,4,4) camera->master (the batch's
    ``target_cam_extr``), cam_view_num (B,) views per sample -> (B,J,3) joints in the master frame.

    ``mode`` None / "off": every view counts the same (``poem_triangulate_dlt``; ``conf`` is not read).
    ``mode`` "threshold": upstream's ``triangulate_dlt`` per sample (lib/utils/triangulation.py:111-148): a view enters a
    joint's solve when ``conf`` (BN,J) > ``threshold``; the threshold drops by 0.05 until two views do, and stays lowered
    for the sample's following joints.  ``mode`` "weighted": each view's two rows are scaled by its confidence.
    ``return_count``: also the (B,J) int32 number of views each solve used.  ``invert=False``: ``cam_extr`` is already
    master->camera.  Both run inside one stream-ordered launch.

    ``mode`` "ransac" (``poem_dlt_robust``; upstream has no counterpart, ``conf`` is not read): a view whose 2-D joint disagrees
    with the geometry of the others is left out.  Every pair of the sample's views gives a hypothesis, a view within ``inlier_px``
    pixels of its reprojection and in front of the camera is its inlier, the pair with the most inliers (ties: smaller summed
    squared error, then the earlier pair) is solved again over its inliers; with fewer than two inliers, or a camera that is not
    finite, the plain solve over all views stands.  ``refine`` (0..16) Gauss-Newton steps on the reprojection error follow.
    Exhaustive and deterministic, 2..64 views per sample.  With three views and one outlier every pair explains itself and the
    outlier is not identified: the mode needs three clean views.  ``return_count``: the (B,J) inlier counts (0 after the
    fallback).  ``return_inliers``: ``(out, inlier (BN,J) bool, resid (BN,J) pixels)`` (``(out, count, inlier, resid)`` with both),
    ``resid`` being the final joint's reprojection error in every view, inlier or not."""
    if not uv.is_cuda:
        if mode == "ransac":
            raise ValueError("mode 'ransac' takes device tensors: it runs on the MI355X HIP path only (no CPU fallback)")
        raise RuntimeError("triangulate_reference_joints runs on the MI355X HIP path only (no CPU fallback)")
    views = [int(v) for v in cam_view_num]
    BN, J = uv.shape[0], uv.shape[1]
    if sum(views) != BN or min(views) < 2:
        raise ValueError("cam_view_num must sum to the number of views and every sample needs >= 2 views for DLT")
    f32 = lambda t: t.to(device=uv.device, dtype=torch.float32).contiguous()   # noqa: E731
    uv, cam_intr, cam_extr = f32(uv), f32(cam_intr), f32(cam_extr)
    out = torch.empty(len(views), J, 3, dtype=torch.float32, device=uv.device)
    offs = _offsets(views, uv.device)
    if return_inliers and mode != "ransac":
        raise ValueError("return_inliers needs mode 'ransac'")
    if mode in (None, "off"):
        if return_count:
            raise ValueError("return_count needs a confidence mode")
        hip.check(hip.lib().poem_triangulate_dlt(hip.ptr(uv), hip.ptr(cam_intr), hip.ptr(cam_extr), offs.data_ptr(),
                                                 len(views), J, int(bool(invert)), hip.ptr(out), hip.stream()),
                  "poem_triangulate_dlt")
        return out
    if mode == "ransac":
        if max(views) > 64:
            raise ValueError("mode 'ransac' takes at most 64 views per sample (the inlier set is one 64-bit mask)")
        inlier_px, refine = float(inlier_px), int(refine)
        if not inlier_px > 0 or not 0 <= refine <= 16:
            raise ValueError("mode 'ransac' needs inlier_px > 0 (inf allowed) and refine in 0..16")
        count = torch.empty(len(views), J, dtype=torch.int32, device=uv.device) if return_count else None
        inl = torch.empty(BN, J, dtype=torch.uint8, device=uv.device) if return_inliers else None
        resid = torch.empty(BN, J, dtype=torch.float32, device=uv.device) if return_inliers else None
        hip.check(hip.lib().poem_dlt_robust(hip.ptr(uv), hip.ptr(cam_intr), hip.ptr(cam_extr), offs.data_ptr(), hip.ptr(out),
                                            hip.ptr(inl, torch.uint8), hip.ptr(count, torch.int32), hip.ptr(resid), len(views), J,
                                            int(bool(invert)), inlier_px, refine, hip.stream()), "poem_dlt_robust")
        res = (out,) + ((count,) if return_count else ()) + ((inl.bool(), resid) if return_inliers else ())
        return res if len(res) > 1 else out
    if mode not in hip.DLT_MODES:
        raise ValueError(f"mode {mode!r}: expected None, 'off', 'threshold', 'weighted' or 'ransac'")
    if conf is None or tuple(conf.shape) != (BN, J):
        raise ValueError(f"mode {mode!r} needs conf of shape ({BN}, {J})")
    threshold = float(threshold)
    if mode == "threshold" and not threshold <= 64.0:
        raise ValueError("threshold must be a number <= 64 (confidences lie in (0, 1))")
    conf = f32(conf)
    count = torch.empty(len(views), J, dtype=torch.int32, device=uv.device) if return_count else None
    hip.check(hip.lib().poem_dlt_confidence(hip.ptr(uv), hip.ptr(conf), hip.ptr(cam_intr), hip.ptr(cam_extr), offs.data_ptr(),
                                            hip.ptr(out), hip.ptr(count, torch.int32), len(views), J, int(bool(invert)),
                                            hip.DLT_MODES[mode], threshold, hip.stream()), "poem_dlt_confidence")
    return (out, count) if return_count else out


def triangulate_dlt(pts, confis, Ks, Extrs, confi_thres=0.5):
    """Upstream's signature for one sample (lib/utils/triangulation.py:111-148): pts (N,J,2), confis (N,J), Ks (N,3,3),
    Extrs (N,4,4) master->camera (used as is), confi_thres -> (J,3).  numpy arrays are taken to the current device and the
    result comes back as numpy, like upstream's; device tensors give a device tensor."""
    as_np = isinstance(pts, np.ndarray)
    dev = torch.device("cuda", torch.cuda.current_device()) if as_np else pts.device
    t = lambda a: torch.as_tensor(a).to(device=dev, dtype=torch.float32)   # noqa: E731
    pts_t = t(pts)
    if pts_t.ndim != 3 or pts_t.shape[-1] != 2:
        raise ValueError("pts must be (N, J, 2)")
    out = triangulate_reference_joints(pts_t, t(Ks), t(Extrs), [pts_t.shape[0]], conf=t(confis), mode="threshold",
                                       threshold=confi_thres, invert=False)[0]
    return out.cpu().numpy().astype(pts.dtype) if as_np else out


def batch_triangulate_dlt_torch(kp2ds, Ks, Extrs):
    """kp2ds (B,N,J,2), Ks (B,N,3,3), Extrs (B,N,4,4) master->camera (used as is, like upstream) -> (B,J,3)."""
    if not kp2ds.is_cuda:
        raise RuntimeError("batch_triangulate_dlt_torch runs on the MI355X HIP path only (no CPU fallback)")
    B, N, J = kp2ds.shape[0], kp2ds.shape[1], kp2ds.shape[2]
    f32 = lambda t: t.to(dtype=torch.float32).contiguous()   # noqa: E731
    uv, K, T = f32(kp2ds).view(B * N, J, 2), f32(Ks).view(B * N, 3, 3), f32(Extrs).view(B * N, 4, 4)
    out = torch.empty(B, J, 3, dtype=torch.float32, device=kp2ds.device)
    offs = _offsets([N] * B, kp2ds.device)
    hip.check(hip.lib().poem_triangulate_dlt(hip.ptr(uv), hip.ptr(K), hip.ptr(T), offs.data_ptr(), B, J, 0, hip.ptr(out),
                                             hip.stream()), "poem_triangulate_dlt")
    return out


def heatmap_to_uv(uv_hmap, img_w, img_h, return_conf=False):
    """uv_hmap (BN,J,Hh,Wh) sigmoid heat maps -> (BN,J,2) pixel coordinates: the read-out at the end of the
    reference's ``heatmap_stage`` (lib/models/POEM.py:213-222 upstream; integral_heatmap2d, integal_pose.py:194-218).
    ``return_conf``: also (BN,J) confidences = each map's maximum, from the same launch (``poem_heatmap_uv_conf``)."""
    if not uv_hmap.is_cuda:
        raise RuntimeError("heatmap_to_uv runs on the MI355X HIP path only (no CPU fallback)")
    h = uv_hmap.to(dtype=torch.float32).contiguous()
    BN, J, Hh, Wh = h.shape
    uv = torch.empty(BN, J, 2, dtype=torch.float32, device=h.device)
    if return_conf:
        conf = torch.empty(BN, J, dtype=torch.float32, device=h.device)
        hip.check(hip.lib().poem_heatmap_uv_conf(hip.ptr(h), hip.ptr(uv), hip.ptr(conf), BN, J, Hh, Wh, float(img_w),
                                                 float(img_h), hip.stream()), "poem_heatmap_uv_conf")
        return uv, conf
    hip.check(hip.lib().poem_heatmap_uv(hip.ptr(h), hip.ptr(uv), BN, J, Hh, Wh, float(img_w), float(img_h), hip.stream()),
              "poem_heatmap_uv")
    return uv


def reference_joints_from_heatmaps(uv_hmap, cam_intr, cam_extr, cam_view_num, img_w, img_h, mode=None, threshold=0.5,
                                   inlier_px=8.0, refine=0):
    """Heat maps of every view -> per-view 2-D joints -> ragged DLT -> (B,J,3) reference joints: the two launches that
    replace POEM.py:213-222 + :284-299 upstream.  ``mode`` / ``threshold`` / ``inlier_px`` / ``refine`` as
    ``triangulate_reference_joints``: the confidences are the maps' own peaks (still two launches); "ransac" reads none."""
    if mode in (None, "off"):
        return triangulate_reference_joints(heatmap_to_uv(uv_hmap, img_w, img_h), cam_intr, cam_extr, cam_view_num)
    if mode == "ransac":
        return triangulate_reference_joints(heatmap_to_uv(uv_hmap, img_w, img_h), cam_intr, cam_extr, cam_view_num, mode=mode,
                                            inlier_px=inlier_px, refine=refine)
    uv, conf = heatmap_to_uv(uv_hmap, img_w, img_h, return_conf=True)
    return triangulate_reference_joints(uv, cam_intr, cam_extr, cam_view_num, conf=conf, mode=mode, threshold=threshold)
