"""Any N_SAMPLE up to 8192 on the CPU: the oracle reproduces the reference fixtures of tests/golden/make_golden_nsample.py
(S = 1000, 1600, 3000, 8192, 2500: not a multiple of 32, not a multiple of the embed width, above 4096) at the bars
test_neighbours64_oracle.py sets for the same fixture classes; the configuration check takes the whole range; make_basis."""
import ctypes

import numpy as np
import pytest
import torch

import poem_v2_amd as pk
from poem_v2_amd import hip
from nsample_util import setup_case, thin
from util import load_golden, run_oracle


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def _idx_taps_agree(taps, z, meta):
    """The oracle's neighbour sets match the reference's: identical for >= 99.5 % of the queries."""
    spec = meta["spec"]
    for blk in range(1, 3):
        for which in ("self", "cross"):
            want = torch.from_numpy(z[f"tap.b{blk}.idx_{which}"].astype(np.int64))
            got = thin(meta, f"tap.b{blk}.idx_{which}", torch.as_tensor(taps[f"b{blk}.idx_{which}"]).long())
            assert want.shape[-1] == 32 and got.shape == want.shape, (blk, which)
            assert int(want.max()) < (799 if which == "self" else spec["nsample"])
            same = (torch.sort(got, -1).values == torch.sort(want, -1).values).all(-1)
            assert float(same.float().mean()) > 0.995, (blk, which)


def test_tinyns1000_stage_taps():
    z, meta = load_golden("tinyns1000")
    spec = meta["spec"]
    assert spec["nsample"] == 1000 and spec["nsample"] % 32 == 8 and spec["nsample"] % spec["embed"]
    cfg, w, consts, batch = setup_case(spec)
    taps = {}
    out = run_oracle(cfg, w, consts, batch, taps=taps)
    assert _maxdiff(thin(meta, "tap.x", taps["x"]), z["tap.x"]) < 2e-5
    assert _maxdiff(thin(meta, "tap.g", taps["g"]), z["tap.g"]) < 2e-5
    assert _maxdiff(thin(meta, "tap.bps_feat", taps["bps_feat"]), z["tap.bps_feat"]) < 5e-5
    assert _maxdiff(taps["pt_xyz"], z["tap.pt_xyz"]) == 0.0
    assert _maxdiff(taps["query_xyz"], z["tap.query_xyz"]) == 0.0
    for i in range(3):
        for k, tol in (("h_cross", 2e-5), ("f_self", 2e-5), ("f_cross", 2e-5), ("feats", 5e-5)):
            assert _maxdiff(thin(meta, f"tap.b{i}.{k}", taps[f"b{i}.{k}"][:, ::9]), z[f"tap.b{i}.{k}"]) < tol, (i, k)
        assert _maxdiff(taps[f"b{i}.xyz"], z[f"tap.b{i}.xyz"]) < 2e-5, i
    _idx_taps_agree(taps, z, meta)
    assert _maxdiff(out["all_coords_preds"], z["all_coords_preds"]) < 2e-6


@pytest.mark.parametrize("name", ["smallns1600", "mediumns3000", "tinyns8192", "largens2500"])
def test_release_shapes_nsample(name):
    z, meta = load_golden(name)
    spec = meta["spec"]
    cfg, w, consts, batch = setup_case(spec, z["bps"] if "bps" in z.files else None)
    assert consts["bps"].shape == (spec["nsample"], 3)
    taps = {}
    out = run_oracle(cfg, w, consts, batch, taps=taps)
    assert _maxdiff(taps["bps_feat"][:, ::64], z["tap.bps_feat"]) < 1e-4
    ref = z["all_coords_preds"]
    got = out["all_coords_preds"].numpy()
    err = np.linalg.norm(got[-1, :, 21:] - ref[-1, :, 21:], axis=-1)
    assert err.mean() < 1e-6, err.mean()
    assert _maxdiff(got, ref) < 5e-5
    _idx_taps_agree(taps, z, meta)


def test_config_check_takes_any_nsample_up_to_8192():
    """poem_config_t.nsample (host-side check, no GPU): any count from the neighbour count up to 8192."""
    L = hip.lib()
    for nsample, knn, ok in ((775, 32, True), (1000, 32, True), (1600, 32, True), (5000, 32, True), (8192, 64, True),
                             (8193, 32, False), (31, 32, False), (63, 64, False), (64, 64, True), (0, 1, False)):
        for embed in (32, 256):
            cfg = hip.make_config(embed, nsample=nsample, knn=knn)
            assert (L.poem_num_weight_tensors(ctypes.byref(cfg)) > 0) == ok, (nsample, knn, embed)


def test_make_basis_is_seeded_and_inside_the_ball():
    a, b, c = pk.make_basis(5000, 0.1, 7), pk.make_basis(5000, 0.1, 7), pk.make_basis(5000, 0.1, 8)
    assert a.shape == (5000, 3) and a.dtype == np.float32
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    r = np.linalg.norm(a.astype(np.float64), axis=1)
    assert r.max() <= 0.1 and r.min() >= 0.0
    # uniform in the ball: the fraction inside half the radius is 1/8, the mean radius 3/4 of it, no preferred direction
    assert abs((r < 0.05).mean() - 0.125) < 0.02 and abs(r.mean() / 0.1 - 0.75) < 0.01
    assert np.abs(a.mean(axis=0)).max() < 0.003
    assert np.linalg.norm(pk.make_basis(64, 2.5, 0).astype(np.float64), axis=1).max() <= 2.5
    with pytest.raises(ValueError):
        pk.make_basis(0, 0.1, 0)


def test_missing_basis_message_names_the_count_and_the_places(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError) as e:
        hip.load_assets(5000)
    msg = str(e.value)
    assert "5000" in msg and "bps.npy" in msg and str(tmp_path) in msg and "4096 points" in msg and "make_basis" in msg
