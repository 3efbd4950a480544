"""Cost of the confidence paths in front of the head: ``poem_heatmap_uv_conf`` + ``poem_dlt_confidence`` (threshold, weighted)
against the plain pair ``poem_heatmap_uv`` + ``poem_triangulate_dlt``, per forward at batch 2 and batch 32 (ragged 2..10 views).
HIP events around each pair, the variants interleaved round by round, medians over the rounds.

  python tools/dlt_conf_cost.py [--rounds 200]   ->  one JSON line per batch size"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import poem_v2_amd as pk  # noqa: E402

tri = pk.triangulation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    args = ap.parse_args()
    dev = "cuda:0"
    for B in (2, 32):
        views = np.random.RandomState(5).randint(2, 11, size=B).tolist()
        b = pk.inputs.synthetic_batch(views, seed=77)["img_metas"]
        K, E = b["cam_intr"].to(dev), b["cam_extr"].to(dev)
        g = torch.Generator().manual_seed(44)
        hm = torch.sigmoid(4.0 * torch.randn(sum(views), 21, 32, 32, generator=g) - 3.0).to(dev)

        def plain():
            return tri.triangulate_reference_joints(tri.heatmap_to_uv(hm, 256.0, 256.0), K, E, views)

        def conf(mode):
            uv, c = tri.heatmap_to_uv(hm, 256.0, 256.0, return_conf=True)
            return tri.triangulate_reference_joints(uv, K, E, views, conf=c, mode=mode, threshold=0.5)

        variants = {"plain": plain, "threshold": lambda: conf("threshold"), "weighted": lambda: conf("weighted")}
        for fn in variants.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                z.record()
                z.synchronize()
                times[k].append(a.elapsed_time(z) * 1e3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        print(json.dumps({"batch": B, "views": int(sum(views)), "rounds": args.rounds,
                          "median_us": {k: round(v, 2) for k, v in med.items()},
                          "p10_p90_us": {k: [round(float(np.percentile(v, 10)), 2), round(float(np.percentile(v, 90)), 2)]
                                         for k, v in times.items()},
                          "extra_us_vs_plain": {k: round(med[k] - med["plain"], 2) for k in ("threshold", "weighted")}}))


if __name__ == "__main__":
    main()
