"""Golden data for N_NEIGHBOR / N_NEIGHBOR_QUERY above 32 (33..64) from the upstream reference (build container only, like
make_golden.py, whose run_case does the work): stage taps at a toy width, hot weights at the small release shape (the
neighbour sets decide), the medium release shape at 64 / 64, and the large model (the P = 1 vector attention) at 40 / 33.
Every fixture records the reference's idx_self / idx_cross with K columns.  A fixture above BUDGET is thinned (thin()): every
IDX_STEP-th query row of the neighbour taps, and in the toy case strided columns of the whole sampling-stage tensors and every
second of the per-block rows; meta["thinned"] lists {tap: [axis, step]}, so that a test takes the same slice of its own tensor.

  python tests/golden/make_golden_k64.py [case ...]   ->  tests/golden/<case>.npz"""
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [GOLDEN]
sys.dont_write_bytecode = True

from make_golden import run_case  # noqa: E402

BUDGET = 1_000_000    # bytes: a fixture above it is thinned
IDX_STEP = 4
# the `full` case's whole sampling-stage tensors and its (already 9-strided) per-block rows: (axis, step)
THIN_FULL = {"tap.g": (2, 8), "tap.bps_feat": (1, 4), "tap.x": (3, 2), "tap.grid": (1, 4)}
THIN_FULL_BLOCK = (".h_attn", ".h_cross", ".f_self", ".f_cross", ".feats")

CASES = {
    "tinyk64": dict(model="medium", embed=32, nsample=1024, views=[2, 1, 3], seed=61, parametric=False, full=True, knn=64,
                    knn_query=40),
    "smallk64": dict(model="small", embed=128, nsample=4096, views=[3, 2], seed=62, parametric=False, full=False, gain=2.5,
                     ln_spread=0.3, knn=48, knn_query=64),
    "mediumk64": dict(model="medium", embed=256, nsample=4096, views=[4, 2], seed=63, parametric=False, full=False, knn=64,
                      knn_query=64),
    "largek64": dict(model="large", embed=512, nsample=4096, views=[3], seed=64, parametric=False, full=False, knn=40,
                     knn_query=33),
}

def thin(name):
    path = os.path.join(GOLDEN, f"{name}.npz")
    if os.path.getsize(path) <= BUDGET:
        return
    z = np.load(path)
    rec = {k: z[k] for k in z.files}
    meta = json.loads(bytes(rec["meta"]).decode())
    rules = {k: (1, IDX_STEP) for k in rec if ".idx_" in k}
    if meta["spec"]["full"]:
        rules.update({k: r for k, r in THIN_FULL.items() if k in rec})
        rules.update({k: (1, 2) for k in rec if k.endswith(THIN_FULL_BLOCK)})
    for k, (axis, step) in rules.items():
        sl = [slice(None)] * rec[k].ndim
        sl[axis] = slice(None, None, step)
        rec[k] = rec[k][tuple(sl)]
    meta["thinned"] = {k: list(r) for k, r in rules.items()}
    rec["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(path, **rec)
    print(f"{name}: thinned to {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    torch.set_num_threads(8)
    for n in sys.argv[1:] or list(CASES):
        run_case(n, CASES[n])
        thin(n)
