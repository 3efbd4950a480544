"""Golden data for an N_SAMPLE that is not a multiple of 32, not a multiple of the embed width, or above 4096, from the upstream
reference (build container only, like make_golden.py, whose run_case does the work; thinning as make_golden_k64.py).  A case
above 4096 basis points runs the reference on its own asset directory: the basis is a seeded poem_v2_amd.make_basis draw, and
the fixture stores it (key "bps") so that a test can hand the same points to the oracle and to the head.

  python tests/golden/make_golden_nsample.py [case ...]   ->  tests/golden/<case>.npz"""
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [GOLDEN]
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
from make_golden import run_case  # noqa: E402
from make_golden_k64 import BUDGET, IDX_STEP, THIN_FULL, THIN_FULL_BLOCK  # noqa: E402,F401
import poem_v2_amd as pk  # noqa: E402

BASIS_SEED = 8192

CASES = {
    # S % 32 = 8, S % C != 0: every stage tap
    "tinyns1000": dict(model="medium", embed=32, nsample=1000, views=[2, 1, 3], seed=71, parametric=False, full=True),
    # S % 32 = 0, S % C != 0: a width the fused sampling kernels would otherwise take; hot weights (the neighbour sets decide)
    "smallns1600": dict(model="small", embed=128, nsample=1600, views=[3, 2], seed=72, parametric=False, full=False, gain=2.5,
                        ln_spread=0.3),
    # release width, masked last key tile, one chunk of 94 key tiles
    "mediumns3000": dict(model="medium", embed=256, nsample=3000, views=[4, 2], seed=73, parametric=False, full=False),
    # above 4096: the search's LDS, eight key chunks
    "tinyns8192": dict(model="medium", embed=32, nsample=8192, views=[2, 1], seed=74, parametric=False, full=False),
    # the P = 1 vector attention and the streaming cross attention, masked
    "largens2500": dict(model="large", embed=512, nsample=2500, views=[3], seed=75, parametric=False, full=False),
}

_make_cwd = mg.make_cwd


def make_cwd(nsample):
    """make_golden.make_cwd, with a seeded basis of our own where the reference's shipped one is too small."""
    d = _make_cwd(min(nsample, 4096))
    if nsample > 4096:
        np.save(os.path.join(d, "assets", "bps.npy"), pk.make_basis(nsample, 0.1, BASIS_SEED)[None])
    return d


mg.make_cwd = make_cwd


def thin(name):
    """As make_golden_k64.thin (same rules, same meta["thinned"] record); stores the basis of a case above 4096 points."""
    path = os.path.join(GOLDEN, f"{name}.npz")
    z = np.load(path)
    rec = {k: z[k] for k in z.files}
    meta = json.loads(bytes(rec["meta"]).decode())
    big = meta["spec"]["nsample"] > 4096
    if big:
        rec["bps"] = pk.make_basis(meta["spec"]["nsample"], 0.1, BASIS_SEED)
        meta["basis"] = dict(seed=BASIS_SEED, radius=0.1)
    if os.path.getsize(path) <= BUDGET and not big:
        return
    rules = {}
    if os.path.getsize(path) + (rec["bps"].nbytes if big else 0) > BUDGET:
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
    print(f"{name}: rewritten, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    torch.set_num_threads(8)
    for n in sys.argv[1:] or list(CASES):
        run_case(n, CASES[n])
        thin(n)
