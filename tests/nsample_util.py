"""Helpers of test_nsample_oracle.py / test_nsample.py: cases whose basis is larger than the shipped 4096 points take it from
the fixture (or from a seeded poem_v2_amd.make_basis draw) -- the oracle through its consts, the head through an asset
directory of its own under the working directory, which is where the reference looks first as well."""
import os
import shutil

import numpy as np
import torch

import poem_v2_amd as pk
from util import ASSETS, case_setup

NAMES = ("tinyns1000", "smallns1600", "mediumns3000", "tinyns8192", "largens2500")


def thin(meta, key, t):
    """The slice the generator's thin() took of fixture tap `key` (meta["thinned"]: {tap: [axis, step]}), of a full tensor."""
    axis, step = meta.get("thinned", {}).get(key, (0, 1))
    sl = [slice(None)] * t.ndim
    sl[axis] = slice(None, None, step)
    return t[tuple(sl)]


def setup_case(spec, bps=None):
    """util.case_setup for any N_SAMPLE up to 8192: above 4096 the basis is `bps` (S,3) or make_basis(S, 0.1, spec seed)."""
    S = spec["nsample"]
    if S <= 4096:
        return case_setup(spec)
    cfg, w, consts, batch = case_setup(dict(spec, nsample=4096))
    import dataclasses
    cfg = dataclasses.replace(cfg, nsample=S)
    basis = np.asarray(bps, dtype=np.float32) if bps is not None else pk.make_basis(S, 0.1, spec["seed"])
    assert basis.shape == (S, 3)
    consts = dict(consts, bps=torch.from_numpy(basis.copy()))
    return cfg, w, consts, batch


def write_assets(root, bps):
    """<root>/assets with `bps` as the basis and the shipped anchors beside it."""
    d = os.path.join(str(root), "assets")
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "bps.npy"), np.asarray(bps, dtype=np.float32)[None])
    for f in ("anchor.npy", "anchor_idx.npy"):
        shutil.copy(os.path.join(ASSETS, f), os.path.join(d, f))
    return d
