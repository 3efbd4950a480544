"""The reference's OWN checkpoint loader on a model that carries this package's head (executed against
the reference tree): upstream's ``build_model`` builds upstream's full ``PtEmbedMultiviewStereoV2`` with ``POEM_Generalized_Head``
/ ``PtEmbedTRv4`` replaced in upstream's registries, and upstream's ``load_weights(model, path, strict=True)``
(lib/utils/net_utils.py:200-231, called from the model's constructor at lib/models/POEM.py:162) loads a checkpoint saved from the
pure-reference model.

WHICH FORM RUNS: the full model, built by upstream's own builder.  The harness (``tests/golden/ref_harness.py``) constructs it
with a randomly initialised HRNet backbone that is never run, so no pretrained backbone file is needed and the smaller form
(upstream's head alone inside a parent module) is not used.  Without a reference tree beside the repository the tests skip."""
import os
import sys
from collections import OrderedDict

import pytest
import torch

import poem_v2_amd as pk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_LIVE = 199


@pytest.fixture(scope="module")
def upstream(tmp_path_factory):
    """Upstream's builder and loader, the pure-reference model's state dict and two checkpoint files saved from it (a bare
    ``OrderedDict`` and the ``{"state_dict": {"module." + key: ...}}`` form of a DataParallel run)."""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import ref_harness as rh
    if not os.path.isdir(rh.REF_ROOT):
        pytest.skip("reference tree absent: upstream's own loader cannot be run")
    import yaml
    cwd = os.getcwd()
    try:
        CN, _ = rh.setup()
        from lib.utils import builder
        from lib.utils.net_utils import load_weights
        with open(os.path.join(rh.REF_ROOT, "config/release/train_medium.yaml")) as f:
            y = yaml.safe_load(f)

        def build(pretrained=None):
            cfg = CN(y)
            cfg.MODEL["PRETRAINED"] = pretrained
            return builder.build_model(cfg.MODEL, data_preset=cfg.DATA_PRESET, train=cfg.TRAIN)

        ref = build()
        import lib.models.heads.ptEmb_head as ref_head_mod
        assert type(ref.ptEmb_head) is ref_head_mod.POEM_Generalized_Head
        sd = OrderedDict((k, v.detach().clone()) for k, v in ref.state_dict().items())
        d = tmp_path_factory.mktemp("ckpt")
        bare, wrapped = str(d / "bare.pth.tar"), str(d / "wrapped.pth.tar")
        torch.save(sd, bare)
        torch.save({"epoch": 1, "state_dict": OrderedDict(("module." + k, v) for k, v in sd.items())}, wrapped)
        yield dict(builder=builder, build=build, load_weights=load_weights, sd=sd, bare=bare, wrapped=wrapped, root=rh.REF_ROOT)
    finally:
        os.chdir(cwd)


@pytest.fixture()
def hip_registered(upstream):
    """The block INTEGRATION.md section 1 adds to lib/models/__init__.py; upstream's own classes are put back afterwards."""
    HEAD, TRANSFORMER = upstream["builder"].HEAD, upstream["builder"].TRANSFORMER
    ref_head, ref_tr = HEAD.get("POEM_Generalized_Head"), TRANSFORMER.get("PtEmbedTRv4")
    cwd = os.getcwd()
    os.chdir(upstream["root"])                           # upstream reads config/ and assets/ relative to its root
    HEAD.register_module(name="POEM_Generalized_Head", force=True, module=pk.POEM_Generalized_Head)
    TRANSFORMER.register_module(name="PtEmbedTRv4", force=True, module=pk.PtEmbedTRv4)
    try:
        yield
    finally:
        HEAD.register_module(name="POEM_Generalized_Head", force=True, module=ref_head)
        TRANSFORMER.register_module(name="PtEmbedTRv4", force=True, module=ref_tr)
        os.chdir(cwd)


def _check_loaded(model, sd):
    head = model.ptEmb_head
    assert type(head) is pk.POEM_Generalized_Head and type(head.transformer) is pk.PtEmbedTRv4
    got = model.state_dict()
    live = [k for k in got if k.startswith("ptEmb_head.")]
    assert len(live) == N_LIVE
    for k, v in got.items():                             # the head's live tensors and everything else of the model, bit for bit
        assert torch.equal(v, sd[k]), k
    dead = sorted(k[len("ptEmb_head."):] for k in sd if k.startswith("ptEmb_head.") and k not in got)
    assert head.ignored_reference_keys == dead and len(dead) == 59
    assert head._reference_checkpoint_loaded
    assert sum(sd["ptEmb_head." + k].numel() for k in dead) > 31e6          # ~31.6 M parameters never read


def test_upstreams_load_weights_loads_a_reference_checkpoint_strict(upstream, hip_registered):
    model = upstream["build"]()                          # PRETRAINED empty: upstream's random initialisation
    assert type(model.ptEmb_head) is pk.POEM_Generalized_Head
    assert not torch.equal(model.state_dict()["ptEmb_head.input_proj.weight"], upstream["sd"]["ptEmb_head.input_proj.weight"])
    upstream["load_weights"](model, upstream["bare"], strict=True)
    _check_loaded(model, upstream["sd"])
    # the DataParallel form, through upstream's own "module." stripping, onto a model whose weights were scrambled in between
    with torch.no_grad():
        for p in model.ptEmb_head.parameters():
            p.zero_()
    upstream["load_weights"](model, upstream["wrapped"], strict=True)
    _check_loaded(model, upstream["sd"])


def test_upstreams_constructor_loads_cfg_pretrained(upstream, hip_registered):
    """lib/models/POEM.py:162: ``load_weights(self, pretrained=self.cfg.PRETRAINED)`` -- strict -- inside the constructor."""
    model = upstream["build"](pretrained=upstream["wrapped"])
    _check_loaded(model, upstream["sd"])


def test_upstreams_loader_still_refuses_a_foreign_checkpoint(upstream, hip_registered, tmp_path):
    model = upstream["build"]()
    sd = OrderedDict(upstream["sd"])
    sd["ptEmb_head.bogus.weight"] = torch.zeros(2)
    del sd["ptEmb_head.query_feat_embedding.weight"]
    path = str(tmp_path / "foreign.pth.tar")
    torch.save(sd, path)
    with pytest.raises(RuntimeError) as e:
        upstream["load_weights"](model, path, strict=True)
    msg = str(e.value)
    assert 'Missing key(s) in state_dict: "ptEmb_head.query_feat_embedding.weight".' in msg
    assert 'Unexpected key(s) in state_dict: "ptEmb_head.bogus.weight".' in msg
