"""Cost of the MANO fit: ``poem_v2_amd.fit_mano`` at ``iters`` 8 and 0 (the difference over 8 = one evaluation + one step launch),
next to one ``ManoLayer`` call (``poem_mano_lbs``), at B = 32 and B = 2 on seeded synthetic assets; the targets are the layer's own
meshes of seeded parameters (root rotations up to 2.8 rad, fingers sigma 0.4, betas sigma 1, tsl sigma 0.3 m) plus 2 mm noise.  HIP
events through the Python call, median of 20 after warm-up.

  python tools/mano_fit_cost.py                      ->  one JSON line per batch size
  python tools/mano_fit_cost.py --one-fit B          ->  warm-up, then ONE fit of B samples (iters 8): what a kernel trace is taken of
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
    if len(sys.argv) > 2 and sys.argv[1] == "--one-fit":
        _, _, target = case(layer, int(sys.argv[2]))
        for _ in range(3):
            pk.fit_mano(layer, target, iters=8)
        torch.cuda.synchronize()
        return
    for B in (32, 2):
        pose, betas, target = case(layer, B)
        variants = {"fit_iters8": lambda: pk.fit_mano(layer, target, iters=8), "fit_iters0": lambda: pk.fit_mano(layer, target, iters=0),
                    "mano_lbs": lambda: layer(pose, betas)}
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
