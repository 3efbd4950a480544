"""Mean end-point error accumulated on the device and reduced across ranks with one all-reduce.

Same definition as the reference's ``MeanEPE.feed`` (lib/metrics/mean_epe.py:23-33 upstream): per sample the mean over
points of the L2 distance, summed over the batch; the running average divides by the number of samples.  The
reference calls ``.item()`` every batch (a host sync); here the two sums stay on the device until ``result()``."""
import torch

from . import dist as pdist


class MeanEPE:
    def __init__(self, name="", device="cpu"):
        self.name = f"{name}_mepe"
        self.acc = torch.zeros(2, dtype=torch.float64, device=device)   # this rank's [sum of per-sample means, n samples]
        self._global = None                                               # the all-reduced pair of the last reduce()

    def reset(self):
        self.acc.zero_()
        self._global = None

    def feed(self, pred_kp, gt_kp):
        assert pred_kp.dim() == 3, "pred shape should be (BATCH, NPOINTS, 1|2|3)"
        d = torch.norm(pred_kp - gt_kp, p="fro", dim=2).mean(dim=1)
        self.acc[0] += d.sum().double()
        self.acc[1] += d.shape[0]
        self._global = None

    def reduce(self):
        """all-reduce(sum) of [sum, count] over the process group (16 bytes: the path's only collective).  The local
        sums are left alone, so reducing after every step does not count earlier steps once per rank."""
        self._global = pdist.all_reduce_sum_(self.acc.clone())
        return self

    def result(self):
        s, n = (self.acc if self._global is None else self._global).tolist()
        return s / max(n, 1.0)

    def __str__(self):
        return f"{self.name}: {self.result():6.4f}"


# ---- the remaining evaluation metrics, accumulated on the device ---------------------------------
def _dev32(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


class PAEval:
    """Procrustes-aligned MPJPE / MPVPE -- device counterpart of ``PAEval`` (lib/metrics/pa_eval.py:16-124 upstream).

    Same ``feed`` signature, ``get_measures`` keys, ``get_result`` and string form.  The reference copies every batch to
    the host and calls scipy once per sample; here ``poem_pa_epe`` aligns the whole batch in one launch and the four
    sums stay on the device.  No CPU fallback."""

    def __init__(self, cfg=None, mesh_score=False, device="cuda"):
        self.mesh_score = mesh_score
        self.device = torch.device(device)
        self.acc = torch.zeros(5, dtype=torch.float64, device=self.device)   # this rank's pa_j, j, pa_v, v, count
        self._global = None                                                   # the all-reduced sums of the last reduce()
        self.count = 0

    def reset(self):
        self.acc.zero_()
        self._global = None
        self.count = 0

    def _pair(self, pred, gt):
        from . import hip
        pred, gt = _dev32(pred, self.device), _dev32(gt, self.device)
        if not pred.is_cuda:
            raise RuntimeError("PAEval runs on the MI355X HIP path only (no CPU fallback)")
        out = torch.empty(pred.shape[0], 2, dtype=torch.float32, device=self.device)
        hip.check(hip.lib().poem_pa_epe(hip.ptr(pred), hip.ptr(gt), hip.ptr(out), pred.shape[0], pred.shape[1],
                                        hip.stream()), "poem_pa_epe")
        return out.double().sum(0)

    def feed(self, pred_joints_3d_abs, joints_3d_abs, pred_verts_3d_abs=None, verts_3d_abs=None, **kwargs):
        b = pred_joints_3d_abs.shape[0]
        self.acc[0:2] += self._pair(pred_joints_3d_abs, joints_3d_abs)
        if self.mesh_score:
            self.acc[2:4] += self._pair(pred_verts_3d_abs, verts_3d_abs)
        self.acc[4] += b
        self.count += b
        self._global = None

    def reduce(self):
        """all-reduce(sum) of a copy: the rank-local sums stay what this rank fed, so a second ``reduce()`` or a ``feed``
        after it never counts anything once per rank (same contract as ``MeanEPE.reduce``)."""
        self._global = pdist.all_reduce_sum_(self.acc.clone())
        return self

    def get_measures(self, **kwargs):
        a = (self.acc if self._global is None else self._global).tolist()
        n = max(a[4], 1.0)
        m = {"pa_mpjpe": a[0] / n, "mpjpe": a[1] / n}
        if self.mesh_score:
            m["pa_mpvpe"], m["mpvpe"] = a[2] / n, a[3] / n
        return m

    def get_result(self):
        return self.get_measures()["pa_mpjpe"]

    def __str__(self):
        m = self.get_measures()
        s = f"pa_mpjpe(mm): {m['pa_mpjpe'] * 1000.0 :6.4f} | mpjpe: {m['mpjpe']:6.4f}"
        if self.mesh_score:
            s += f" | pa_mpvpe(mm): {m['pa_mpvpe'] * 1000.0:6.4f} | mpvpe: {m['mpvpe']:6.4f}"
        return s


class _PCKMetric:
    """PCK / AUC accumulators -- device counterpart of ``_PCKMetric`` (lib/metrics/pck.py:11-148 upstream): same config
    keys (VAL_MIN, VAL_MAX, STEPS, EVAL_TYPE), ``feed(preds, targs)``, ``get_pck_all`` and ``get_measures`` keys."""
    num_kp = 0
    _keys = {}

    def __init__(self, device="cuda", **cfg):
        self.val_min, self.val_max, self.steps = float(cfg["VAL_MIN"]), float(cfg["VAL_MAX"]), int(cfg["STEPS"])
        self.device = torch.device(device)
        self.reset()

    def reset(self):
        self.counts = torch.zeros(self.num_kp, self.steps, dtype=torch.int32, device=self.device)
        self.sum = torch.zeros(self.num_kp, dtype=torch.float64, device=self.device)
        self.n = torch.zeros(self.num_kp, dtype=torch.int32, device=self.device)
        self.dists = []          # per-batch (B, num_kp) distance tensors on the device (arbitrary-threshold queries)
        self.count = 0
        self._global = None      # (counts int64, n int64, sum fp64) over all ranks, set by reduce()

    def _get_predictions(self, preds, targs):
        pk_, tk_ = self._keys[self.eval_type]
        return preds[pk_].reshape(-1, self.num_kp, 3), targs[tk_].reshape(-1, self.num_kp, 3)

    def feed(self, preds, targs, **kwargs):
        from . import hip
        p, t = self._get_predictions(preds, targs)
        p, t = _dev32(p, self.device), _dev32(t, self.device)
        if not p.is_cuda:
            raise RuntimeError("PCK metrics run on the MI355X HIP path only (no CPU fallback)")
        d = torch.empty(p.shape[0], self.num_kp, dtype=torch.float32, device=self.device)
        hip.check(hip.lib().poem_pck_accumulate(hip.ptr(p), hip.ptr(t), p.shape[0], self.num_kp, self.val_min, self.val_max,
                                                self.steps, self.counts.data_ptr(), self.sum.data_ptr(), self.n.data_ptr(),
                                                hip.ptr(d), hip.stream()), "poem_pck_accumulate")
        self.dists.append(d)
        self.count += p.shape[0]
        self._global = None

    def reduce(self):
        """Sum the accumulators over ranks into a separate global copy (counts as int64 to stay exact); the rank-local
        accumulators are untouched, so reducing twice or feeding afterwards never double counts."""
        g = (self.counts.long(), self.n.long(), self.sum.clone())
        for t in g:
            pdist.all_reduce_sum_(t)
        self._global = g
        return self

    def get_pck_all(self, threshold):
        """Fraction of key points within ``threshold`` (every sample carries all key points, so the mean of per-key-point
        means is hits / total).  Before ``reduce()``: this rank's samples.  After it: all ranks' -- read from the reduced
        threshold histogram when ``threshold`` is one of its steps (the usual 0.02 = VAL_MAX is; no communication, so rank 0
        alone may print the metric); for any other threshold this rank's [hits, total] pair is all-reduced here and every
        rank must make the call."""
        import numpy as np
        if self._global is not None:
            steps = np.linspace(self.val_min, self.val_max, self.steps)
            hit = np.nonzero(np.isclose(steps, threshold, rtol=0, atol=1e-12))[0]
            if hit.size:
                counts, n, _ = self._global
                return float(counts[:, int(hit[0])].sum()) / max(float(n.sum()), 1.0)
        d = torch.cat(self.dists, 0) if self.dists else torch.zeros(0, self.num_kp, device=self.device)
        pair = torch.stack([(d.double() <= threshold).sum().double(), torch.tensor(float(d.numel()), dtype=torch.float64, device=d.device)])
        if self._global is not None:
            pdist.all_reduce_sum_(pair)
        hits, total = pair.tolist()
        return hits / max(total, 1.0)

    def get_measures(self):
        import numpy as np
        thresholds = np.linspace(self.val_min, self.val_max, self.steps)
        area_under_one = getattr(np, "trapezoid", getattr(np, "trapz", None))(np.ones_like(thresholds), thresholds)
        counts, n, dsum = (self.counts, self.n, self.sum) if self._global is None else self._global
        n = n.cpu().numpy().astype(np.float64)
        valid = n > 0
        curve = counts.cpu().numpy().astype(np.float64)[valid] / n[valid][:, None]
        epe = dsum.cpu().numpy()[valid] / n[valid]
        auc = getattr(np, "trapezoid", getattr(np, "trapz", None))(curve, thresholds, axis=1) / area_under_one
        return {"epe_mean_per_kp": epe, "pck_curve_per_kp": curve, "auc_per_kp": auc, "epe_mean_all": float(np.mean(epe)),
                "auc_all": float(np.mean(auc)), "thresholds": thresholds}

    def __str__(self):
        return f"h3dpck: {self.get_pck_all(0.02):6.4f}"


class Joint3DPCK(_PCKMetric):
    num_kp = 21
    _keys = {"joints_3d": ("pred_joints_3d", "master_joints_3d"), "joints_3d_rel": ("pred_joints_3d_rel", "master_joints_3d_rel")}

    def __init__(self, device="cuda", **cfg):
        self.eval_type = cfg.get("EVAL_TYPE", "joints_3d")
        if self.eval_type not in self._keys:
            raise ValueError(f"Unknown eval_type {self.eval_type} in {type(self).__name__}")
        super().__init__(device=device, **cfg)


class Vert3DPCK(_PCKMetric):
    num_kp = 778
    _keys = {"verts_3d": ("pred_verts_3d", "master_verts_3d"), "verts_3d_rel": ("pred_verts_3d_rel", "master_verts_3d_rel")}

    def __init__(self, device="cuda", **cfg):
        self.eval_type = cfg.get("EVAL_TYPE", "verts_3d")
        if self.eval_type not in self._keys:
            raise ValueError(f"Unknown eval_type {self.eval_type} in {type(self).__name__}")
        super().__init__(device=device, **cfg)


def mano_to_openpose(J_regressor, mano_verts):
    """MANO vertices (B,778,3) -> joints (B,21,3) in OpenPose order: the reference function of the same name
    (lib/utils/transform.py:836-872 upstream), which ``testing_step`` applies to predicted and ground-truth vertices
    before the joint metrics (lib/models/POEM.py:602-603).  ``J_regressor`` is MANO's ``th_J_regressor`` (16,778) -- an
    input, the asset is licence-gated.  One launch on the device; no CPU fallback."""
    from . import hip
    if not mano_verts.is_cuda:
        raise RuntimeError("mano_to_openpose runs on the MI355X HIP path only (no CPU fallback)")
    v = _dev32(mano_verts, mano_verts.device)
    w = _dev32(J_regressor, mano_verts.device)
    if tuple(w.shape) != (16, 778) or v.dim() != 3 or tuple(v.shape[1:]) != (778, 3):
        raise ValueError("J_regressor must be (16,778) and mano_verts (B,778,3)")
    out = torch.empty(v.shape[0], 21, 3, dtype=torch.float32, device=v.device)
    hip.check(hip.lib().poem_mano_to_openpose(hip.ptr(w), hip.ptr(v), hip.ptr(out), v.shape[0], 778, hip.stream()),
              "poem_mano_to_openpose")
    return out


# ---- benchmark-protocol mesh scores: F@5 / F@15 and the aligned AUC on the device -----------------
def procrustes_align(pred, gt, return_transform=False):
    """``PAEval.align_w_scale(gt, pred)`` (lib/metrics/pa_eval.py:104-124 upstream) for a batch, with the aligned set kept:
    pred, gt (B,P,3) device tensors -> aligned (B,P,3) fp32 -- the points whose mean distance to ``gt`` ``PAEval`` reports (one
    solve behind both).  ``return_transform``: also (B,13) fp64 = c, R (row-major), t with aligned = c R p + t.  One launch,
    one wave per sample; no CPU fallback."""
    from . import hip
    if not pred.is_cuda:
        raise RuntimeError("procrustes_align runs on the MI355X HIP path only (no CPU fallback)")
    p, g = _dev32(pred, pred.device), _dev32(gt, pred.device)
    if p.dim() != 3 or p.shape[2] != 3 or p.shape != g.shape or p.shape[1] < 3:
        raise ValueError(f"pred and gt must both be (B,P,3) with P >= 3, got {tuple(p.shape)} and {tuple(g.shape)}")
    out = torch.empty_like(p)
    tr = torch.empty(p.shape[0], 13, dtype=torch.float64, device=p.device) if return_transform else None
    with torch.cuda.device(p.device):
        hip.check(hip.lib().poem_pa_align(hip.ptr(p), hip.ptr(g), hip.ptr(out), None if tr is None else tr.data_ptr(), p.shape[0],
                                          p.shape[1], hip.stream()), "poem_pa_align")
    return (out, tr) if return_transform else out


def _nn_call(a, b, thresholds, want_dist, want_reduce, workspace=None):
    """poem_nn_distance on device tensors a (B,na,3), b (B,nb,3): (d_ab, d_ba, counts (B,2,T) int32, sums (B,2) fp64, workspace)"""
    import ctypes
    from . import hip
    if not a.is_cuda:
        raise RuntimeError("nearest-neighbour distances run on the MI355X HIP path only (no CPU fallback)")
    a, b = _dev32(a, a.device), _dev32(b, a.device)
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 3 or b.shape[2] != 3 or a.shape[0] != b.shape[0] or 0 in a.shape or 0 in b.shape:
        raise ValueError(f"a and b must be (B,na,3) and (B,nb,3), got {tuple(a.shape)} and {tuple(b.shape)}")
    B, na, nb, T = a.shape[0], a.shape[1], b.shape[1], len(thresholds)
    d_ab = torch.empty(B, na, dtype=torch.float32, device=a.device) if want_dist else None
    d_ba = torch.empty(B, nb, dtype=torch.float32, device=a.device) if want_dist else None
    counts = sums = None
    need = 0
    if want_reduce:
        counts = torch.empty(B, 2, T, dtype=torch.int32, device=a.device) if T else None
        sums = torch.empty(B, 2, dtype=torch.float64, device=a.device)
        need = hip.lib().poem_nn_distance_workspace_bytes(B, na, nb, T)
        if need == 0:
            raise RuntimeError(f"poem_nn_distance does not take batch {B}, na {na}, nb {nb}, {T} thresholds")
        if workspace is None or workspace.numel() < need or workspace.device != a.device:
            workspace = torch.empty(need, dtype=torch.uint8, device=a.device)
    thr = (ctypes.c_double * max(T, 1))(*[float(t) for t in thresholds])
    with torch.cuda.device(a.device):
        hip.check(hip.lib().poem_nn_distance(hip.ptr(a), na, hip.ptr(b), nb, hip.ptr(d_ab), hip.ptr(d_ba), thr if T else None, T,
                                             None if counts is None else counts.data_ptr(), None if sums is None else sums.data_ptr(),
                                             None if workspace is None else workspace.data_ptr(), need, B, hip.stream()),
                  "poem_nn_distance")
    return d_ab, d_ba, counts, sums, workspace


def nearest_distances(a, b):
    """a (B,na,3), b (B,nb,3) device tensors -> (d_ab (B,na), d_ba (B,nb)) fp32: the distance of every point of ``a`` to its nearest
    point of ``b`` and the other way round -- the nearest-neighbour loop of the FreiHAND / HO3D evaluation scripts, brute force
    in one launch.  A point with a NaN coordinate is nearest to nothing and nothing is nearest to it (include/poem_hip.h)."""
    return _nn_call(a, b, (), True, False)[:2]


class MeshFScore:
    """Mesh F-scores of the FreiHAND / HO3D protocols, accumulated on the device (the protocol scripts loop over samples on the host
    through open3d; the reference tree has no code of them).  Per sample: d_p = distance of every predicted vertex to its nearest
    ground-truth vertex, d_g the other way; precision = #{d_p < t} / Np, recall = #{d_g < t} / Ng (strict ``<``, as the
    scripts compare), F = 2 P R / (P + R), 0 where P + R = 0; the score is the mean of the per-sample F.  ``aligned``: the same
    on ``procrustes_align(pred, gt)`` as well (keys ``PA_...``).  The search and the alignment are kernels; P / R / F come from
    the integer counts in fp64.  No CPU fallback."""

    def __init__(self, thresholds=(0.005, 0.015), aligned=True, device="cuda"):
        self.thresholds = tuple(float(t) for t in thresholds)
        if not 1 <= len(self.thresholds) <= 8 or any(not (t >= 0) for t in self.thresholds) or \
                any(b <= a for a, b in zip(self.thresholds, self.thresholds[1:])):
            raise ValueError(f"thresholds must be 1..8 ascending non-negative lengths in metres, got {thresholds}")
        self.modes = ("", "PA_") if aligned else ("",)
        self.device = torch.device(device)
        M, T = len(self.modes), len(self.thresholds)
        # this rank's sums: per (mode, threshold) F, P, R; per mode the mean d_p and mean d_g; the sample count
        self.acc = torch.zeros(M * T * 3 + M * 2 + 1, dtype=torch.float64, device=self.device)
        self._global = None
        self._ws = None          # the search's workspace, grown as needed
        self._n = None           # ((Np, Ng), their device tensor)
        self.count = 0

    def reset(self):
        self.acc.zero_()
        self._global = None
        self.count = 0

    def feed(self, pred_verts, gt_verts, **kwargs):
        """pred_verts (B,Np,3), gt_verts (B,Ng,3) -> per-sample F (B, modes, T) fp64 on the device.  Launches and device
        arithmetic only: nothing is copied to the host."""
        pred, gt = _dev32(pred_verts, self.device), _dev32(gt_verts, self.device)
        if not pred.is_cuda:
            raise RuntimeError("MeshFScore runs on the MI355X HIP path only (no CPU fallback)")
        if len(self.modes) > 1 and pred.shape != gt.shape:
            raise ValueError("the aligned scores need vertex correspondence: pred and gt of one shape")
        M, T, B = len(self.modes), len(self.thresholds), pred.shape[0]
        # one search for every mode: the modes' sets stacked along the batch (a sample's bits do not depend on its batch)
        src = torch.cat([pred, procrustes_align(pred, gt)]) if M > 1 else pred
        tgt = torch.cat([gt, gt]) if M > 1 else gt
        _, _, counts, sums, self._ws = _nn_call(src, tgt, self.thresholds, False, True, self._ws)
        # (the point counts as a device tensor, filled on the device: a true division, and no copy in either direction)
        key = (src.shape[1], tgt.shape[1])
        if self._n is None or self._n[0] != key:
            self._n = (key, torch.cat([torch.full((1,), float(k), dtype=torch.float64, device=self.device) for k in key]))
        n = self._n[1]
        pr = counts.double().view(M, B, 2, T) / n[None, None, :, None]          # precision, recall
        p, r = pr[:, :, 0], pr[:, :, 1]                                          # (M,B,T)
        f = torch.where(p + r > 0, 2.0 * p * r / (p + r), torch.zeros_like(p))
        self.acc[:M * T * 3] += torch.stack([f.sum(1), p.sum(1), r.sum(1)], 2).reshape(-1)       # (M,T,3)
        self.acc[M * T * 3:-1] += (sums.view(M, B, 2) / n[None, None, :]).sum(1).reshape(-1)     # (M,2)
        self.acc[-1] += B
        self.count += B
        self._global = None
        return f.permute(1, 0, 2).contiguous()

    def reduce(self):
        """all-reduce(sum) of a copy: the rank-local sums stay what this rank fed (``PAEval.reduce``'s contract)."""
        self._global = pdist.all_reduce_sum_(self.acc.clone())
        return self

    def get_measures(self, **kwargs):
        a = (self.acc if self._global is None else self._global).tolist()
        M, T = len(self.modes), len(self.thresholds)
        n = max(a[-1], 1.0)
        m = {}
        for mi, mode in enumerate(self.modes):
            for ti, thr in enumerate(self.thresholds):
                f, p, r = a[(mi * T + ti) * 3:(mi * T + ti) * 3 + 3]
                key = f"{thr * 1000:g}"
                m[f"{mode}F@{key}"], m[f"{mode}precision@{key}"], m[f"{mode}recall@{key}"] = f / n, p / n, r / n
            m[f"{mode}chamfer_pred2gt"], m[f"{mode}chamfer_gt2pred"] = a[M * T * 3 + mi * 2] / n, a[M * T * 3 + mi * 2 + 1] / n
        return m

    def get_result(self):
        return self.get_measures()[f"F@{self.thresholds[0] * 1000:g}"]

    def __str__(self):
        m = self.get_measures()
        return " | ".join(f"{mode}F@{t * 1000:g}: {m[f'{mode}F@{t * 1000:g}']:6.4f}" for mode in self.modes for t in self.thresholds)


class _PAFeed:
    """``feed`` of the PCK metrics on Procrustes-aligned predictions: ``procrustes_align`` first, then the unchanged accumulation."""

    def feed(self, preds, targs, **kwargs):
        pk_, tk_ = self._keys[self.eval_type]
        p, t = self._get_predictions(preds, targs)
        p, t = _dev32(p, self.device), _dev32(t, self.device)
        if not p.is_cuda:
            raise RuntimeError("PCK metrics run on the MI355X HIP path only (no CPU fallback)")
        return super().feed({pk_: procrustes_align(p, t)}, {tk_: t}, **kwargs)


class PAJoint3DPCK(_PAFeed, Joint3DPCK):
    """``Joint3DPCK`` of the aligned joints: the PA-AUC column of the FreiHAND / HO3D protocols (VAL_MAX 0.05, STEPS 100 there)."""


class PAVert3DPCK(_PAFeed, Vert3DPCK):
    """``Vert3DPCK`` of the aligned vertices."""
