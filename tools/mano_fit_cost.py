"""Cost of the MANO fit: ``poem_v2_amd.fit_mano`` at ``iters`` 8 and 0 (the difference over 8 = one evaluation + one step launch),
next to one ``ManoLayer`` call (``poem_mano_lbs``), at B = 32 and B = 2 on seeded synthetic assets; the targets are the layer's own
meshes of seeded parameters (root rotations up to 2.8 rad, fingers sigma 0.4, betas sigma 1, tsl sigma 0.3 m) plus 2 mm noise.  HIP
events through the Python call, median of 20 after warm-up.

  python tools/mano_fit_cost.py                      ->  one JSON line per batch size
  python tools/mano_fit_cost.py --views N            ->  the same with the combined fit (mesh + 2-D keypoints in N views per sample,
                                                         weight 1e3) timed between two mesh-only timings: mesh / combined / mesh
  python tools/mano_fit_cost.py --one-fit B          ->  warm-up, then ONE fit of B samples (iters 8): what a kernel trace is taken of
                                                         (with --views N in front: the combined fit)
  python tools/mano_fit_cost.py --split TRACE.csv    ->  the kernel-trace CSV of such a run (the profiler's --kernel-trace, csv
                                                         output): per kernel of the LAST fit, launches and summed device time"""
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import poem_v2_amd as pk  # noqa: E402

DEV = "cuda:0"


def event_us(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) * 1e3


def case(layer, B):
    g = torch.Generator().manual_seed(17)
    axis = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1)
    pose = torch.cat([axis * 2.8 * torch.rand(B, 1, generator=g), 0.4 * torch.randn(B, 45, generator=g)], 1).to(DEV)
    betas, tsl = torch.randn(B, 10, generator=g).to(DEV), (0.3 * torch.randn(B, 1, 3, generator=g)).to(DEV)
    target = layer(pose, betas).verts + tsl + (2e-3 * torch.randn(B, 778, 3, generator=g)).to(DEV)
    return pose, betas, target.contiguous()


def keypoint_terms(layer, pose, betas, target, views):
    """``views`` cameras per sample on a ring 0.6 m around each hand, fx = 250, 256^2 images; keypoints = the clean joints'
    projections (``render.project_to_views``) -> the keyword arguments of the combined fit"""
    B = pose.shape[0]
    centre = target.mean(1).cpu().double()
    ang = 2 * np.pi * torch.arange(views, dtype=torch.float64) / views
    d = torch.stack([torch.cos(ang), 0.2 * torch.ones(views, dtype=torch.float64), torch.sin(ang)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    T = torch.zeros(B, views, 4, 4, dtype=torch.float64)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    for n in range(views):
        z = -d[n]
        x = torch.linalg.cross(up, z)
        x = x / x.norm()
        T[:, n, :3, 0], T[:, n, :3, 1], T[:, n, :3, 2], T[:, n, :3, 3], T[:, n, 3, 3] = x, torch.linalg.cross(z, x), z, centre + 0.6 * d[n], 1.0
    K = torch.tensor([[250.0, 0, 128], [0, 250, 128], [0, 0, 1]]).expand(B * views, 3, 3).contiguous().to(DEV)
    T = T.reshape(B * views, 4, 4).float().to(DEV)
    joints = layer(pose, betas).joints + (target.mean(1) - layer(pose, betas).verts.mean(1))[:, None]
    kp = pk.render.project_to_views(joints.contiguous(), K, T, [views] * B)
    return dict(keypoints=kp, keypoint_weights=torch.full((B * views, 21), 1e3, device=DEV), cam_intr=K, cam_extr=T,
                cam_view_num=[views] * B, image_scale=256.0)


def split(path):
    rows = list(csv.DictReader(open(path)))
    rows = [r for r in rows if "mano_fit" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "init" in r["Kernel_Name"]]
    last = rows[starts[-1]:]
    out = {}
    for r in last:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        n, t = out.get(name, (0, 0.0))
        out[name] = (n + 1, t + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    span = (int(last[-1]["End_Timestamp"]) - int(last[0]["Start_Timestamp"])) / 1e3
    print(json.dumps({"fits_in_trace": len(starts), "last_fit_launches": len(last), "first_start_to_last_end_us": round(span, 1),
                      "kernels_launches_and_sum_us": {k: [n, round(t, 1)] for k, (n, t) in out.items()}}))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--split":
        return split(sys.argv[2])
    layer = pk.ManoLayer(pk.mano.synthetic_mano_assets(3), center_idx=None, device=DEV)
    argv, views = sys.argv[1:], 0
    if len(argv) > 1 and argv[0] == "--views":
        views, argv = int(argv[1]), argv[2:]
    if len(argv) > 1 and argv[0] == "--one-fit":
        pose, betas, target = case(layer, int(argv[1]))
        kw = keypoint_terms(layer, pose, betas, target, views) if views else {}
        for _ in range(3):
            pk.fit_mano(layer, target, iters=8, **kw)
        torch.cuda.synchronize()
        return
    for B in (32, 2):
        pose, betas, target = case(layer, B)
        variants = {"fit_iters8": lambda: pk.fit_mano(layer, target, iters=8), "fit_iters0": lambda: pk.fit_mano(layer, target, iters=0),
                    "mano_lbs": lambda: layer(pose, betas)}
        if views:
            kw = keypoint_terms(layer, pose, betas, target, views)
            variants = {"fit_iters8": variants["fit_iters8"], f"combined_{views}views_iters8": lambda: pk.fit_mano(layer, target, iters=8, **kw),
                        "fit_iters8_again": variants["fit_iters8"], "fit_iters0": variants["fit_iters0"],
                        f"combined_{views}views_iters0": lambda: pk.fit_mano(layer, target, iters=0, **kw)}
        res = {}
        for name, fn in variants.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            res[name] = round(float(np.median([event_us(fn) for _ in range(20)])), 1)
        fit = pk.fit_mano(layer, target, iters=8)
        res["per_iteration"] = round((res["fit_iters8"] - res["fit_iters0"]) / 8, 1)
        print(json.dumps({"batch": B, "median_us": res, "accepted": fit.accepted.tolist()[:4], "flagged": int((fit.status != 0).sum())}))


if __name__ == "__main__":
    main()
