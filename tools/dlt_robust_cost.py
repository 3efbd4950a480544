"""Cost of the outlier-robust triangulation: ``poem_dlt_robust`` (``refine`` 0 and 4, all optional outputs) next to
``poem_dlt_confidence`` (threshold) and ``poem_triangulate_dlt`` on the same inputs -- B = 32 and B = 2 samples of 8 views, J = 21, one
outlier view per sample (tests/dlt_robust_util.make_case).  HIP events, median of 20 after warm-up: a single call between two events,
and per call in a run of 10 (the stage is launch-bound; the second figure takes the events' own cost out).

  python tools/dlt_robust_cost.py   ->  one JSON line per batch size"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import poem_v2_amd as pk  # noqa: E402
import dlt_robust_util as ru  # noqa: E402

tri = pk.triangulation.triangulate_reference_joints


def event_us(fn, calls):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    z.record()
    z.synchronize()
    return a.elapsed_time(z) * 1e3 / calls


def main():
    dev = "cuda:0"
    for B in (32, 2):
        views = [8] * B
        c = ru.make_case(views, [1] * B, 11)
        uv, K, E = [torch.from_numpy(c[k]).to(dev) for k in ("uv", "K", "E")]
        conf = 0.3 + 0.7 * torch.rand(uv.shape[:2], generator=torch.Generator().manual_seed(1)).to(dev)
        variants = {"plain": lambda: tri(uv, K, E, views),
                    "threshold": lambda: tri(uv, K, E, views, conf=conf, mode="threshold", threshold=0.5),
                    "ransac_refine0": lambda: tri(uv, K, E, views, mode="ransac", return_count=True, return_inliers=True),
                    "ransac_refine4": lambda: tri(uv, K, E, views, mode="ransac", refine=4, return_count=True, return_inliers=True)}
        res = {}
        for name, fn in variants.items():
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            res[name] = [round(float(np.median([event_us(fn, n) for _ in range(20)])), 1) for n in (1, 10)]
        print(json.dumps({"batch": B, "views": sum(views), "median_us_single_and_per_call_of_10": res}))


if __name__ == "__main__":
    main()
