"""N_NEIGHBOR / N_NEIGHBOR_QUERY above 32 (33..64) on the CPU: the oracle reproduces the reference fixtures of
tests/golden/make_golden_k64.py, and its neighbour search agrees with an independent k-d tree at K = 33, 48, 64."""
import numpy as np
import pytest
import torch

import poem_oracle as po
from util import case_setup, load_golden, run_oracle


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def _thin(meta, key, t):
    """The slice make_golden_k64.thin() took of fixture tap `key` (meta["thinned"]: {tap: [axis, step]}), of a full tensor."""
    axis, step = meta.get("thinned", {}).get(key, (0, 1))
    sl = [slice(None)] * t.ndim
    sl[axis] = slice(None, None, step)
    return t[tuple(sl)]


def _idx_taps_agree(taps, z, meta):
    """Every recorded neighbour tap has K columns; the oracle's sets match the reference's (identical for >= 99.5 % of the
    queries -- the rest are fp32 near-ties of the hot-weight case)."""
    spec = meta["spec"]
    for blk in range(1, spec.get("nblocks", 3)):
        for which, k in (("self", spec["knn_query"]), ("cross", spec["knn"])):
            want = torch.from_numpy(z[f"tap.b{blk}.idx_{which}"].astype(np.int64))
            got = _thin(meta, f"tap.b{blk}.idx_{which}", torch.as_tensor(taps[f"b{blk}.idx_{which}"]).long())
            assert want.shape[-1] == k and got.shape == want.shape, (blk, which)
            same = (torch.sort(got, -1).values == torch.sort(want, -1).values).all(-1)
            assert float(same.float().mean()) > 0.995, (blk, which)


def test_tinyk64_stage_taps():
    z, meta = load_golden("tinyk64")
    spec = meta["spec"]
    assert (spec["knn"], spec["knn_query"]) == (64, 40)
    cfg, w, consts, batch = case_setup(spec)
    taps = {}
    out = run_oracle(cfg, w, consts, batch, taps=taps)
    assert _maxdiff(_thin(meta, "tap.x", taps["x"]), z["tap.x"]) < 2e-5
    assert _maxdiff(_thin(meta, "tap.g", taps["g"]), z["tap.g"]) < 2e-5
    assert _maxdiff(_thin(meta, "tap.bps_feat", taps["bps_feat"]), z["tap.bps_feat"]) < 5e-5
    assert _maxdiff(taps["pt_xyz"], z["tap.pt_xyz"]) == 0.0
    assert _maxdiff(taps["query_xyz"], z["tap.query_xyz"]) == 0.0
    for i in range(3):
        for k, tol in (("h_cross", 2e-5), ("f_self", 2e-5), ("f_cross", 2e-5), ("feats", 5e-5)):
            assert _maxdiff(_thin(meta, f"tap.b{i}.{k}", taps[f"b{i}.{k}"][:, ::9]), z[f"tap.b{i}.{k}"]) < tol, (i, k)
        assert _maxdiff(taps[f"b{i}.xyz"], z[f"tap.b{i}.xyz"]) < 2e-5, i
    _idx_taps_agree(taps, z, meta)
    assert _maxdiff(out["all_coords_preds"], z["all_coords_preds"]) < 2e-6


@pytest.mark.parametrize("name", ["smallk64", "mediumk64", "largek64"])
def test_release_shapes_k64(name):
    z, meta = load_golden(name)
    spec = meta["spec"]
    assert max(spec["knn"], spec["knn_query"]) > 32
    cfg, w, consts, batch = case_setup(spec)
    taps = {}
    out = run_oracle(cfg, w, consts, batch, taps=taps)
    assert _maxdiff(taps["bps_feat"][:, ::64], z["tap.bps_feat"]) < 1e-4
    ref = z["all_coords_preds"]
    got = out["all_coords_preds"].numpy()
    err = np.linalg.norm(got[-1, :, 21:] - ref[-1, :, 21:], axis=-1)
    assert err.mean() < 1e-6, err.mean()
    assert _maxdiff(got, ref) < 5e-5
    _idx_taps_agree(taps, z, meta)


def test_k64_fixtures_depend_on_the_counts():
    """The hot-weight fixture really exercises counts above 32: the oracle at 32 / 32 lands more than 1e-3 m away."""
    import dataclasses
    z, meta = load_golden("smallk64")
    cfg, w, consts, batch = case_setup(meta["spec"])
    out = run_oracle(dataclasses.replace(cfg, knn=32, knn_query=32), w, consts, batch)["all_coords_preds"]
    assert _maxdiff(out, z["all_coords_preds"]) > 1e-3


@pytest.mark.parametrize("K", [33, 48, 64])
@pytest.mark.parametrize("NQ,NS,seed", [(799, 799, 3), (799, 4096, 4)])
def test_knn_indices_k64_against_an_independent_kd_tree(K, NQ, NS, seed):
    """As test_oracle_golden's k-d tree check, at K above 32: the same K neighbours in the same order wherever consecutive fp64
    distances are further apart than 1e-5 relative; inside near-tied groups only the set is compared."""
    from scipy.spatial import cKDTree
    g = torch.Generator().manual_seed(seed + K)
    q = (torch.rand(2, NQ, 3, generator=g) - 0.5) * 0.4
    s = q.clone() if NS == NQ else (torch.rand(2, NS, 3, generator=g) - 0.5) * 0.4
    got = po.knn_indices(q, s, K).numpy()
    assert got.shape == (2, NQ, K)
    strict = 0
    for b in range(2):
        d64, i64 = cKDTree(s[b].double().numpy()).query(q[b].double().numpy(), k=K + 1)
        d64 = d64 ** 2
        for i in range(NQ):
            gaps = np.diff(d64[i]) > 1e-5 * np.maximum(d64[i][1:], 1e-12)
            lo = 0
            for k in range(K):
                if gaps[k]:
                    if k == lo:
                        assert got[b, i, k] == i64[i, k]
                        strict += 1
                    else:
                        assert set(got[b, i, lo:k + 1]) == set(i64[i, lo:k + 1])
                    lo = k + 1
    assert strict > 0.95 * 2 * NQ * K


def test_config_check_takes_counts_up_to_64():
    """poem_config_t.knn: 1..64 and no more than the basis points (host-side check, no GPU)."""
    import ctypes
    from poem_v2_amd import hip
    L = hip.lib()
    for knn, nsample, ok in ((33, 1024, True), (64, 4096, True), (65, 1024, False), (48, 32, False), (32, 32, True)):
        cfg = hip.make_config(32, nsample=nsample, knn=knn)
        assert (L.poem_num_weight_tensors(ctypes.byref(cfg)) > 0) == ok, (knn, nsample)
