"""Cost of ``PoemLoss`` (one launch + a one-block finalize, fp64) next to the same terms composed from torch operators on the same GPU --
upstream's ``compute_loss`` with its Python loop over samples (lib/models/POEM.py:336-466), restated here in fp32 as upstream runs
it -- for the release and the all-terms configuration at 32 samples x 8 views, timed with HIP events in one process."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import poem_v2_amd as pk  # noqa: E402

TIPS = [744, 320, 443, 555, 672]
OPENPOSE = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]


def torch_compute_loss(lo, preds, gt, jreg):
    """upstream's compute_loss on torch operators, loop over samples included; ``lo`` is a PoemLoss (its weights and switches)."""
    views = gt["cam_view_num"]
    B = len(views)
    scale = math.sqrt(float(gt["image"].size(-1) ** 2 + gt["image"].size(-2) ** 2))
    crit = {"l2": torch.nn.functional.mse_loss, "l1": torch.nn.functional.l1_loss}
    cj, cv = crit[lo.joints_loss_type], crit[lo.verts_loss_type]
    gj, gv = gt["master_joints_3d"], gt["master_verts_3d"]
    hm = torch.mean(torch.sum(torch.pow((preds["pred_joints_uv"] - gt["target_joints_2d"]) / scale, 2), dim=2))
    T = torch.linalg.inv(gt["target_cam_extr"])
    K = gt["target_cam_intr"]
    pj, pv = preds["all_coords_preds"][-1, :, :21], preds["all_coords_preds"][-1, :, 21:]

    def openpose(v):
        return torch.cat([torch.matmul(jreg, v), v[:, TIPS]], dim=1)[:, OPENPOSE]

    def project(P):
        out = []
        for i in range(B):
            s, e = int(np.sum(views[:i])), int(np.sum(views[:i + 1]))
            sub = P[i].unsqueeze(0).repeat(views[i], 1, 1)
            cam = (T[s:e, :3, :3] @ sub.transpose(1, 2)).transpose(1, 2) + T[s:e, :3, 3].unsqueeze(1)
            res = (K[s:e] @ cam.transpose(1, 2)).transpose(1, 2)
            z = res[..., 2:]
            z[torch.abs(z) < 1e-7] = 1e-7
            out.append(res[..., 0:2] / z)
        return torch.concat(out, dim=0)

    def multicam(P, target):
        off = torch.clamp(project(P) - target, min=-.5 * scale, max=.5 * scale) / scale
        return torch.mean(torch.sum(torch.pow(off, 2), dim=2))

    gv2d = project(gv)                                       # upstream projects the ground-truth vertices whether or not they are read
    d = {"loss_heatmap_joints": hm, "loss_3d_joints": cj(pj, gj), "loss_3d_joints_from_mesh": cj(openpose(pv), openpose(gv))}
    if lo.parametric_output:
        c = gj[:, lo.transformer_center_idx].unsqueeze(1)
        d["loss_3d_verts"] = cv(pv - c, gv - c)
    else:
        d["loss_3d_verts"] = cv(pv, gv)
    recon = lo.joints_weight * (d["loss_3d_joints"] + d["loss_3d_joints_from_mesh"]) + lo.vertices_weight * d["loss_3d_verts"]
    if lo.joints_2d_weight != 0:
        d["loss_2d_joints"] = multicam(pj, gt["target_joints_2d"])
        recon = recon + lo.joints_2d_weight * d["loss_2d_joints"]
    if lo.vertices_2d_weight != 0:
        d["loss_2d_verts"] = multicam(pv, gv2d)
        recon = recon + lo.vertices_2d_weight * d["loss_2d_verts"]
    if lo.parametric_output:
        first = [int(np.sum(views[:j])) for j in range(B)]
        d["loss_pose"] = torch.nn.functional.mse_loss(preds["pred_pose"], gt["mano_pose"][first])
        d["loss_shape"] = torch.nn.functional.mse_loss(preds["pred_shape"], gt["mano_shape"][first])
        recon = recon + lo.pose_weight * d["loss_pose"] + lo.shape_weight * d["loss_shape"]
    d["loss_recon"] = recon
    d["loss"] = lo.heatmap_joints_weights * hm + recon
    return d


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    views = [a.views] * a.batch
    B, BN = a.batch, a.batch * a.views
    b = pk.inputs.synthetic_batch(views, seed=0)
    g = torch.Generator().manual_seed(1)
    gj = b["reference_joints"]
    gv = gj[:, 9:10] + 0.05 * torch.randn(B, 778, 3, generator=g)
    coords = torch.cat([gj, gv], 1) + 0.004 * torch.randn(B, 799, 3, generator=g)
    w = torch.exp(3.0 * torch.randn(16, 778, generator=g))
    jreg = (w / w.sum(1, keepdim=True)).to(dev)
    uv = 256.0 * torch.rand(BN, 21, 2, generator=g)
    preds = {"all_coords_preds": coords[None].to(dev), "pred_joints_uv": (uv + 2 * torch.randn(BN, 21, 2, generator=g)).to(dev),
             "pred_pose": 0.1 * torch.randn(B, 16, 3, generator=g).to(dev), "pred_shape": 0.1 * torch.randn(B, 10, generator=g).to(dev)}
    gt = {"cam_view_num": np.asarray(views), "image": torch.zeros(1, device=dev).expand(BN, 3, 256, 256), "master_joints_3d": gj.to(dev),
          "master_verts_3d": gv.to(dev), "target_joints_2d": uv.to(dev), "target_cam_intr": b["img_metas"]["cam_intr"].to(dev),
          "target_cam_extr": b["img_metas"]["cam_extr"].to(dev), "mano_pose": 0.1 * torch.randn(BN, 16, 3, generator=g).to(dev),
          "mano_shape": 0.1 * torch.randn(BN, 10, generator=g).to(dev)}
    res = {"samples": B, "views": a.views}
    configs = {"release": (pk.configs.loss_cfg(), False),
               "allterms": (pk.configs.loss_cfg(VERTICES_2D_LOSS_WEIGHT=0.5, JOINTS_LOSS_TYPE="l1", VERTICES_LOSS_TYPE="l2"), True)}
    for name, (node, parametric) in configs.items():
        lo = pk.PoemLoss(node, parametric=parametric, j_regressor=jreg)
        hip_d = lo(preds, gt)[1]
        ref_d = torch_compute_loss(lo, preds, gt, jreg)
        worst = max(abs(float(hip_d[k]) - float(ref_d[k])) / abs(float(hip_d[k])) for k in hip_d)
        t_hip = timed(lambda: lo(preds, gt), a.warmup, a.steps)
        t_ref = timed(lambda: torch_compute_loss(lo, preds, gt, jreg), a.warmup, a.steps)
        res[name] = {"poem_loss_ms": round(t_hip, 4), "torch_composition_ms": round(t_ref, 4), "ratio": round(t_ref / t_hip, 1),
                     "worst_relative_difference_fp32_composition": float(f"{worst:.2e}")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
