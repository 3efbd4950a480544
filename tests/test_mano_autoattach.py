"""The head derives its zero-pose template and its MANO layer from MANO assets by itself (config key ``MANO_ASSETS``), attaches
the layer to the engine's launch graph, follows a layer or centre that changes under a built engine, and refuses to decode a
reference checkpoint against the synthetic template.  Shapes: the ``tinymano`` head configuration of tests/golden (embed 32, 1024
basis points), batch 2 with 2 views each, ``synthetic_mano_assets``.  Every comparison is between two heads that launch the same
kernels on the same inputs: bit-equality, no tolerance.  Nothing here reads the reference tree."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import poem_v2_amd as pk
from poem_v2_amd.inputs import synthetic_batch
from util import batch_to

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EMBED, NSAMPLE, SEED, VIEWS, CENTRE = 32, 1024, 12, [2, 2], 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def assets_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mano") / "mano_assets.npz")
    np.savez(path, **pk.mano.synthetic_mano_assets(0))
    return path


@pytest.fixture(scope="module")
def batch():
    return synthetic_batch(VIEWS, seed=SEED)


def _head(parametric, assets=None, **extra):
    hc = pk.configs.head_cfg(EMBED, NSAMPLE, parametric)
    if assets is not None:
        hc["MANO_ASSETS"] = assets
    for k, v in extra.items():
        hc["TRANSFORMER"][k] = v
    head = pk.build_head(hc, data_preset=pk.CN({}))
    res = head.load_state_dict(pk.weights.seeded_state_dict(EMBED, seed=SEED, parametric=parametric), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return head.to(DEV).eval()


def _layer(seed=0, centre=CENTRE):
    return pk.ManoLayer.from_arrays(**pk.mano.synthetic_mano_assets(seed), center_idx=centre, device=DEV)


def _hand_wired(layer_seed=0, centre=CENTRE):
    """A parametric head wired the way INTEGRATION.md used to ask for: template and layer given by the caller."""
    head = _head(True)
    head.set_template(_layer(0, CENTRE).zero_pose_template())
    head.set_mano_layer(pk.ManoLayer(pk.mano.synthetic_mano_assets(layer_seed), center_idx=centre, device=DEV))
    return head


def _forward(head, batch, device=DEV):
    feat, metas, rj = batch_to(batch, device)
    with torch.no_grad():
        return head(feat, metas, rj)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _quiet_forward(head, batch):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = _forward(head, batch)
    assert not [str(w.message) for w in rec if "synthetic hand template" in str(w.message)]
    return out


def test_template_comes_from_the_assets(assets_path, batch):
    head = _head(False, assets_path)
    assert head._template_is_synthetic and head.mano_assets_source == f"config:{assets_path}"     # nothing derived before a forward
    out = _quiet_forward(head, batch)
    want = _layer().zero_pose_template()
    assert not head._template_is_synthetic and head.template.device == want.device
    assert torch.equal(head.template, want) and float(want[CENTRE].abs().max()) == 0.0
    assert head.mano_layer is None                                                               # no parametric tail: no layer installed
    other = _head(False)
    other.set_template(want)
    _same(out, _forward(other, batch))
    assert torch.isfinite(out["all_coords_preds"]).all()
    synth = _head(False)
    synth.set_template(pk.inputs.synthetic_template())
    assert not torch.equal(out["all_coords_preds"], _forward(synth, batch)["all_coords_preds"])   # (the template does reach the output)
    # the centre of the template is the head's TRANSFORMER_CENTER_IDX
    c4 = _head(False, assets_path, TRANSFORMER_CENTER_IDX=4)
    _quiet_forward(c4, batch)
    assert torch.equal(c4.template, _layer(0, 4).zero_pose_template())


def test_parametric_head_attaches_its_own_layer(assets_path, batch):
    head = _head(True, assets_path)
    out = _quiet_forward(head, batch)
    assert isinstance(head.mano_layer, pk.ManoLayer) and head.mano_layer.center_idx == CENTRE
    assert head._engine._mano is head.mano_layer.th_table                                        # the in-graph route ran
    wired = _hand_wired()
    want = _forward(wired, batch)
    assert wired._engine._mano is wired.mano_layer.th_table
    _same(out, want)
    assert out["pred_pose"].shape == (2, 16, 3) and out["pred_shape"].shape == (2, 10)
    for _ in range(2):                                                                           # capture, then a graph replay
        _same(_forward(head, batch), want)
    assert head._engine.graph_stats()["replays"] >= 1


def test_a_callers_template_and_layer_always_win(assets_path, batch):
    head = _head(True, assets_path)
    mine_t, mine_l = pk.inputs.synthetic_template(77), _layer(1, 4)
    head.set_template(mine_t)
    head.set_mano_layer(mine_l)
    out = _forward(head, batch)
    assert torch.equal(head.template.cpu(), mine_t) and head.mano_layer is mine_l
    wired = _head(True)
    wired.set_template(mine_t)
    wired.set_mano_layer(_layer(1, 4))
    _same(out, _forward(wired, batch))


def test_a_template_given_after_a_forward_survives_new_assets(assets_path, batch):
    """forward (template derived from the assets), ``set_template``, ``set_mano_assets``, forward: the caller's template stays."""
    head = _head(False, assets_path)
    first = _forward(head, batch)
    assert head._template_from_assets and torch.equal(head.template, _layer().zero_pose_template())
    mine = pk.inputs.synthetic_template(77)
    head.set_template(mine)
    head.set_mano_assets(pk.mano.synthetic_mano_assets(1))
    out = _quiet_forward(head, batch)
    assert torch.equal(head.template.cpu(), mine) and not head._template_is_synthetic
    wired = _head(False)
    wired.set_template(mine)
    _same(out, _forward(wired, batch))
    assert not torch.equal(out["all_coords_preds"], first["all_coords_preds"])
    # a template the head derived itself does follow new assets
    auto = _head(False, assets_path)
    _forward(auto, batch)
    auto.set_mano_assets(pk.mano.synthetic_mano_assets(1))
    _quiet_forward(auto, batch)
    assert torch.equal(auto.template, _layer(1).zero_pose_template())
    # the parametric head: the caller's template stays, the head's own layer follows the new assets
    par = _head(True, assets_path)
    _forward(par, batch)
    par.set_template(mine)
    par.set_mano_assets(pk.mano.synthetic_mano_assets(1))
    out = _quiet_forward(par, batch)
    assert torch.equal(par.template.cpu(), mine) and par._engine._mano is par.mano_layer.th_table
    wired = _head(True)
    wired.set_template(mine)
    wired.set_mano_layer(_layer(1))
    _same(out, _forward(wired, batch))


def test_the_engine_follows_a_strict_load(assets_path, batch):
    """forward, strict-load other weights, forward: the output changes and is a fresh head's on those weights."""
    head = _head(False, assets_path)
    first = _forward(head, batch)
    eng = head._engine
    other = pk.weights.seeded_state_dict(EMBED, seed=SEED + 1)
    res = head.load_state_dict(other, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    out = _forward(head, batch)
    assert head._engine is not eng
    assert not torch.equal(out["all_coords_preds"], first["all_coords_preds"])
    fresh = pk.build_head(pk.configs.head_cfg(EMBED, NSAMPLE, False), data_preset=pk.CN({}))
    fresh.load_state_dict(other, strict=True)
    fresh = fresh.to(DEV).eval()
    fresh.set_template(_layer().zero_pose_template())
    _same(out, _forward(fresh, batch))


def test_mano_assets_at_the_model_node_reach_the_head(assets_path, tmp_path, batch):
    """``MODEL.MANO_ASSETS`` of ``PtEmbedMultiviewStereoV2`` is the head's unless ``MODEL.HEAD.MANO_ASSETS`` is set."""
    node = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": pk.configs.head_cfg(EMBED, NSAMPLE, False), "DATA_PRESET": {"CENTER_IDX": 9},
            "DEVICE": DEV, "MANO_ASSETS": assets_path}
    model = pk.build_model(pk.CN(node))
    head = model.ptEmb_head
    assert head.mano_assets_source == f"config:{assets_path}"
    head.load_state_dict(pk.weights.seeded_state_dict(EMBED, seed=SEED), strict=True)
    head.to(DEV).eval()
    out = _quiet_forward(head, batch)
    assert torch.equal(head.template, _layer().zero_pose_template())
    _same(out, _forward(_head(False, assets_path), batch))
    other = str(tmp_path / "other.npz")
    np.savez(other, **pk.mano.synthetic_mano_assets(1))
    node["HEAD"] = dict(pk.configs.head_cfg(EMBED, NSAMPLE, False), MANO_ASSETS=other)
    head = pk.build_model(pk.CN(node)).ptEmb_head
    assert head.mano_assets_source == f"config:{other}"
    assert np.array_equal(head._mano_assets["weights"], pk.mano.synthetic_mano_assets(1)["weights"])


def test_replacing_the_layer_under_a_built_engine(assets_path, batch):
    head = _head(True, assets_path)
    first = _forward(head, batch)
    eng = head._engine
    head.mano_layer = _layer(1)                                   # plain attribute assignment, after the engine was built
    want = _forward(_hand_wired(layer_seed=1), batch)
    for _ in range(3):
        _same(_forward(head, batch), want)
    assert head._engine is eng and eng._mano is head.mano_layer.th_table      # re-attached, not rebuilt
    assert not torch.equal(first["all_coords_preds"][-1], want["all_coords_preds"][-1])
    assert torch.equal(first["all_coords_preds"][:-1], want["all_coords_preds"][:-1])   # only the last layer is the MANO layer's


def test_changing_the_centre_under_a_built_engine(assets_path, batch):
    head = _head(True, assets_path)
    first = _forward(head, batch)
    head.mano_layer.center_idx = 4
    want = _forward(_hand_wired(centre=4), batch)
    for _ in range(3):
        _same(_forward(head, batch), want)
    assert head._engine._mano_center == 4
    assert not torch.equal(first["all_coords_preds"][-1], want["all_coords_preds"][-1])


def test_index_less_device_still_attaches(assets_path, batch):
    hc = pk.configs.head_cfg(EMBED, NSAMPLE, True)
    hc["MANO_ASSETS"] = assets_path
    head = pk.build_head(hc, data_preset=pk.CN({}))
    head.load_state_dict(pk.weights.seeded_state_dict(EMBED, seed=SEED, parametric=True), strict=True)
    head = head.to("cuda").eval()
    out = _forward(head, batch, "cuda")
    assert head._engine._mano is head.mano_layer.th_table
    _same(out, _forward(_hand_wired(), batch))
    # the comparison behind it: an engine on "cuda" and a table on "cuda:0" are on the same device (the current one)
    from poem_v2_amd.head import _same_device
    cur = torch.cuda.current_device()
    assert _same_device(torch.device("cuda"), torch.device("cuda", cur)) and _same_device("cuda", "cuda")
    assert not _same_device(torch.device("cuda", cur + 1), torch.device("cuda")) and not _same_device("cpu", "cuda")

    class _IndexLessEngine:
        device = torch.device("cuda")

    table, centre = head._mano_to_attach(_IndexLessEngine())
    assert table is head.mano_layer.th_table and centre == CENTRE


def test_reference_checkpoint_without_assets_is_refused(batch):
    """A strict load that swallowed dead reference tensors is a real reference checkpoint: the synthetic template is refused,
    where every other load keeps the warning."""
    with open(os.path.join(ROOT, "tests", "golden", "dropin.json")) as f:
        fix = json.load(f)
    head = pk.build_head(pk.CN(dict(fix["head_cfg"], MAX_VIEWS=2)), data_preset=pk.CN(fix["data_preset"]))
    live = set(head.state_dict())
    seeded = pk.weights.seeded_state_dict(256, seed=0)
    sd = {k: seeded[k] if k in live else torch.zeros(shape) for k, shape, _ in fix["state_dict"]}
    head.load_state_dict(sd, strict=True)
    assert len(head.ignored_reference_keys) == len(sd) - 199
    head = head.to(DEV).eval()
    with pytest.raises(RuntimeError) as e:
        _forward(head, batch)
    assert "MANO_ASSETS" in str(e.value) and "set_template" in str(e.value) and "59 dead reference tensors" in str(e.value)
    assert head._engine is None                                   # refused before anything was built or launched
    head.set_template(pk.inputs.synthetic_template(1234))
    out = _forward(head, batch)["all_coords_preds"]
    assert out.shape == (3, 2, 799, 3) and torch.isfinite(out).all()
    # a live-only load on a fresh head keeps today's warning
    plain = _head(False)
    with pytest.warns(UserWarning, match="synthetic hand template"):
        _forward(plain, batch)
