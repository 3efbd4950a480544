"""ResNet-18/34/50 on the CPU: the key tables, the torch engine and the restatement of the non-HRNet decode branch against the
reference's own outputs (tests/golden/make_golden_resnet.py), the configuration rules, the device-free plan of the hip engine,
and the model's choice of backbone and decode table."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import poem_v2_amd as pk
import resnet_util as ru
from poem_v2_amd import backbone as bb
from poem_v2_amd import resnet as rn
from util import GOLDEN

CLASSES = {18: rn.ResNet18, 34: rn.ResNet34, 50: rn.ResNet50}


def _keys():
    with open(os.path.join(GOLDEN, "resnet_keys.json")) as f:
        return json.load(f)


def _npz(name):
    z = np.load(os.path.join(GOLDEN, name))
    return z, json.loads(bytes(z["meta"]).decode())


# ---- key tables and loading ---------------------------------------------------------------------------------------------
KEY_TABLES_AS_THEY_WERE = {  # version -> rows and sha256 of repr(_conv_specs), tensors and digest of the seed-0 weights
    18: (20, "b79f47db096b38b5cc8879a6fabb185f799f3520e9d6662447fb4ee42827d89d",
         100, "58c325cec6c3fbe9ce580bd88f419db35253ccc15c4b4e67dcc26073d991fccb"),
    34: (36, "cc387e02acb0110d7e7306e80cd2f89eefbaa17137ee2970979496d18a29a3c7",
         180, "b8250e351ba4636f4ad3c04a5e7dd58f6022df89f9c6de2ced14710404425478"),
    50: (53, "e0c0a3819e3561711e37284697786ec44917f2d364195c935424cc8bc0515645",
         265, "d187529c7be53279fd45a7230acd2f518716b16a447d1952c42cb7212d8244ed"),
}


def state_dict_digest(sd):
    """(tensor count, sha256 over key then bytes of every item in dict order)"""
    h = hashlib.sha256()
    for key, tensor in sd.items():
        h.update(key.encode())
        h.update(tensor.numpy().tobytes())
    return len(sd), h.hexdigest()


@pytest.mark.parametrize("version", ru.VERSIONS)
def test_key_tables_are_the_reference_models(version):
    table = _keys()[f"resnet{version}"]
    ref = {k: tuple(s) for k, s in table["backbone"].items()}
    live = rn.resnet_param_shapes(version)
    assert {k: s for k, s in ref.items() if not rn.is_dead_key(k)} == live
    dead = [k for k in ref if k not in live]
    assert "fc.weight" in dead and "fc.bias" in dead and all(k.startswith("fc.") or k.endswith(".num_batches_tracked") for k in dead)
    assert sorted(f"{s[0]}.weight" for s in rn._conv_specs(version)) == sorted(k for k in live if len(live[k]) == 4)
    # the table and the seeded weights the fixtures hang on, as recorded when the table was written out by hand
    rows, specs_sha, tensors, seeded_sha = KEY_TABLES_AS_THEY_WERE[version]
    specs = rn._conv_specs(version)
    assert (len(specs), hashlib.sha256(repr(specs).encode()).hexdigest()) == (rows, specs_sha)
    assert state_dict_digest(rn.seeded_resnet_state_dict(version, 0)) == (tensors, seeded_sha)
    # the decode stage: the same keys for every backbone, the channel table by the backbone's name
    name = f"resnet{version}"
    dec = {k: tuple(s) for k, s in table["decode"].items() if not k.startswith("uv_in.") and not k.endswith(".num_batches_tracked")}
    assert dec == pk.weights.decoder_key_shapes(name)
    assert set(dec) == set(pk.decode.FeatureDecoders.live_keys())
    c = pk.decode.FEAT_SIZES[name]
    assert c == rn.level_channels(version) == ((64, 128, 256, 512) if version != 50 else (256, 512, 1024, 2048))
    assert dec["feat_delayer.0.conv.weight"] == (c[2], c[3] + c[2], 3, 3) and dec["uv_delayer.2.conv.weight"] == (c[0], c[1] + c[0], 3, 3)
    assert dec["feat_in.conv.weight"] == (c[1], c[0], 1, 1) and dec["uv_out.conv.weight"] == (21, c[0], 1, 1)
    assert pk.model.head_in_channels(name) == c[1] and pk.model.head_in_channels("HRNet") == 160


def test_conv_specs_are_in_forward_order():
    assert [s[0] for s in rn._conv_specs(18)][:7] == ["conv1", "layer1.0.conv1", "layer1.0.conv2", "layer1.1.conv1", "layer1.1.conv2",
                                                     "layer2.0.conv1", "layer2.0.downsample.0"]
    s50 = rn._conv_specs(50)
    assert [s[0] for s in s50][1:5] == ["layer1.0.conv1", "layer1.0.conv2", "layer1.0.downsample.0", "layer1.0.conv3"]
    assert ("layer2.0.conv2", "layer2.0.bn2", 128, 128, 3, 2) in s50 and ("layer2.0.conv1", "layer2.0.bn1", 128, 256, 1, 1) in s50
    assert ("layer3.0.downsample.0", "layer3.0.downsample.1", 1024, 512, 1, 2) in s50          # the stride is on conv2 and the shortcut
    assert (len(rn._conv_specs(18)), len(rn._conv_specs(34)), len(s50)) == (20, 36, 53)
    with pytest.raises(KeyError):
        rn._conv_specs(101)


def test_loading_prefix_dead_keys_and_errors():
    sd = {"img_backbone." + k: v for k, v in rn.seeded_resnet_state_dict(18, 1).items()}
    sd["img_backbone.fc.weight"], sd["img_backbone.fc.bias"] = torch.zeros(1000, 512), torch.zeros(1000)
    sd["img_backbone.layer1.1.bn1.num_batches_tracked"] = torch.tensor(0)
    sd["ptEmb_head.other"] = torch.zeros(1)
    net = rn.ResNet18()
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 64, 64))
    ignored = net.load_state_dict(sd, prefix="img_backbone.")
    assert ignored == ["img_backbone.fc.weight", "img_backbone.fc.bias", "img_backbone.layer1.1.bn1.num_batches_tracked"]
    assert [tuple(y.shape) for y in net(image=torch.zeros(1, 3, 64, 64))] == [(1, 64, 16, 16), (1, 128, 8, 8), (1, 256, 4, 4), (1, 512, 2, 2)]
    plain = rn.seeded_resnet_state_dict(18, 1)
    with pytest.raises(KeyError):
        rn.ResNet18().load_state_dict({k: v for k, v in plain.items() if k != "layer3.0.downsample.1.running_var"})
    with pytest.raises(KeyError):
        rn.ResNet34().load_state_dict(plain)                                   # a ResNet-18 checkpoint
    with pytest.raises(ValueError):
        rn.ResNet18().load_state_dict(dict(plain, **{"conv1.weight": torch.zeros(64, 3, 3, 3)}))
    with pytest.raises(ValueError):
        rn.ResNet50().load_state_dict(dict(rn.seeded_resnet_state_dict(50, 1), **{"layer1.0.conv3.weight": torch.zeros(64, 64, 1, 1)}))


def test_registry_names_and_configuration_rules(monkeypatch):
    import torch.hub
    import torch.utils.model_zoo

    def called(*a, **k):
        raise AssertionError("a URL loader was called")
    monkeypatch.setattr(torch.utils.model_zoo, "load_url", called)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", called)
    monkeypatch.setattr(torch.hub, "load", called)
    for v, cls in CLASSES.items():
        assert pk.builder.BACKBONE.get(f"ResNet{v}") is cls
        net = pk.build_backbone(pk.CN({"TYPE": f"ResNet{v}", "PRETRAINED": False, "FREEZE_BATCHNORM": v != 34, "EARLY_RETURN": 4}))
        assert type(net) is cls and net.name == f"resnet{v}" and net.engine == "torch" and net.version == v
        with pytest.raises(ValueError, match="state dict"):
            pk.build_backbone(pk.CN({"TYPE": f"ResNet{v}", "PRETRAINED": True, "FREEZE_BATCHNORM": True}))
        with pytest.raises(ValueError, match="EARLY_RETURN"):
            cls({"EARLY_RETURN": 2})
        with pytest.raises(ValueError, match="ENGINE"):
            cls({"ENGINE": "miopen"})
        assert cls({"ENGINE": "hip"}).engine == "hip" and cls(None).engine == "torch"
    assert pk.builder.BACKBONE.get("ResNet101") is None and pk.builder.BACKBONE.get("HRNet") is bb.HRNet
    src = open(rn.__file__).read()
    assert "import torch.hub" not in src and "model_zoo" not in src.replace("``model_zoo", "") and "load_url" not in src


def test_freeze_batchnorm_changes_nothing():
    sd = rn.seeded_resnet_state_dict(18, 2)
    img = 0.3 * torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    a = rn.ResNet18({"FREEZE_BATCHNORM": True}, state_dict=sd)(img)
    b = rn.ResNet18({"FREEZE_BATCHNORM": False}, state_dict=sd)(img)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the torch engine and the decode restatement against the reference ---------------------------------------------------
@pytest.mark.parametrize("version", ru.VERSIONS)
def test_torch_engine_matches_reference_backbone_outputs(version):
    """The bar tests/test_backbone.py holds the HRNet fold to: max|d| < 2e-5 max|ref| per level (the fixture's r<v>_fp32_err, the
    reference's own fp32-vs-fp64 distance, is 0.3..0.6e-6 of max|ref| here: no wider bar is needed)."""
    z, meta = _npz("resnet.npz")
    sd = rn.seeded_resnet_state_dict(version, meta["seed"])
    assert len(sd) == meta["live_keys"][f"resnet{version}"]
    net = CLASSES[version](state_dict=sd)
    img = 0.3 * torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(meta["seed"]))
    ys = net(img)
    step = meta["channel_step"][f"resnet{version}"]
    assert [tuple(y.shape) for y in ys] == [(2, c, 16 >> i, 16 >> i) for i, c in enumerate(rn.level_channels(version))]
    for i, y in enumerate(ys):
        ref = torch.from_numpy(z[f"r{version}_level{i}"])
        err = float((y[:, ::step] - ref).abs().max())
        print(f"resnet{version} level {i}: max|d| = {err:.3e}  max|ref| = {float(ref.abs().max()):.3e}  reference fp32 round-off "
              f"{float(z[f'r{version}_fp32_err'][i]):.3e}")
        assert err < 2e-5 * float(ref.abs().max()), i


@pytest.mark.parametrize("name", ["resnet34", "resnet50"])
def test_decode_restatement_matches_reference_model_outputs(name):
    """tests/resnet_util.py against the reference model's own feat_decode(., name) / uv_decode / heatmap_stage, at the bars
    tests/test_decode.py holds its oracle to."""
    z, meta = _npz("resnet_decode.npz")
    h, w = meta["image"]
    feats = ru.synthetic_levels(name, meta["views"], h, w, meta["seed"])
    assert [tuple(f.shape[-2:]) for f in feats] == [(16, 32), (8, 16), (4, 8), (2, 4)]
    sd = pk.weights.seeded_decoder_state_dict(meta["seed"], backbone=name)
    with torch.no_grad():
        mlvl, hm = ru.feat_decode(feats, sd), ru.uv_decode(feats, sd)
        uv = ru.heatmap_stage(feats, sd, w, h)
    assert tuple(mlvl.shape) == (meta["views"], pk.decode.FEAT_SIZES[name][1], 8, 16) and tuple(hm.shape) == (meta["views"], 21, 8, 16)
    assert float((mlvl[:, ::8] - torch.from_numpy(z[f"{name}_mlvl_feat_s8"])).abs().max()) < 1e-5 * float(z[f"{name}_mlvl_feat_absmax"].reshape(-1)[0])
    assert float((hm[:, ::3] - torch.from_numpy(z[f"{name}_uv_hmap_s3"])).abs().max()) < 1e-6
    assert float((uv - torch.from_numpy(z[f"{name}_uv"])).abs().max()) < 1e-4      # pixels
    assert 5e-4 < float(hm.min()) and float(hm.max()) < 1 - 5e-4                   # logits within +-7.6: no saturated map


def test_fixtures_regenerate_from_their_generator(tmp_path):
    spec = importlib.util.spec_from_file_location("make_golden_resnet", os.path.join(GOLDEN, "make_golden_resnet.py"))
    mod = importlib.util.module_from_spec(spec)
    import torch.hub
    import torch.utils.model_zoo
    saved = torch.utils.model_zoo.load_url, torch.hub.load_state_dict_from_url
    cwd = os.getcwd()
    try:
        spec.loader.exec_module(mod)
        if not os.path.isdir(mod.rh.REF_ROOT):
            pytest.skip("reference tree absent: golden vectors regenerate in the build container only")
        mod.save(str(tmp_path), mod.build())
    finally:
        os.chdir(cwd)
        torch.utils.model_zoo.load_url, torch.hub.load_state_dict_from_url = saved
    for name in mod.FILES:
        assert (tmp_path / name).read_bytes() == open(os.path.join(GOLDEN, name), "rb").read(), name
        assert os.path.getsize(os.path.join(GOLDEN, name)) < (1 << 20)


# ---- the device-free plan -----------------------------------------------------------------------------------------------
def plan_digest(plan):
    """(launch count, sha256) of a plan's (kind, conv, geometry of every map) list"""
    g = lambda m: None if m is None else m.geometry      # noqa: E731
    rows = []
    for op in plan.ops:
        if op["kind"] == "fuse":
            rows.append(("fuse", "", g(op["out"]), tuple((g(m), s) for m, s in op["terms"])))
        else:
            rows.append((op["kind"], op.get("conv", ""), g(op.get("out")), g(op.get("in")), g(op.get("res"))))
    return len(rows), hashlib.sha256(repr(rows).encode()).hexdigest()


PLANS_AS_THEY_WERE = [  # plan, its arguments, (ops, sha256), buffers, nbytes
    ("hrnet", (3, 128, 256), (332, "ab45289f3b6921991096f987c8f0a98be72d6865a9f89d9beb1b57e55b0f490d"), 35, 43319040),
    ("hrnet", (1, 256, 256), (332, "f1ee9c511077331a3dfe076ebb0039f78821aea60b71169196f86085c6ace03b"), 33, 28169088),
    ("hrnet", (2, 512, 512), (332, "85b750a7c5ea5a8dd1c5d3b2031e82096ed6efbd12ef7c48ef51e0d862781f23"), 35, 222234112),
    ("resnet", (2, 128, 256, 18), (25, "cea32ca7282492b332c4cd6cc7847aaa73ead0bdcf9d8514d0cf8ad100802bc3"), 15, 12036096),
    ("resnet", (1, 256, 256, 18), (25, "e1d8d32a3dfefd54ffede069cd2ce271ca8dbc8d2e4190f3b48bb399b019f45b"), 15, 11637760),
    ("resnet", (2, 128, 256, 34), (41, "f22aaae4724ebecb805e294d3e1467e99a62b3dc63d903cca30827c7cfb2d410"), 16, 12281856),
    ("resnet", (1, 256, 256, 34), (41, "57e1f4b70d070ff43f8cfa0764d70924811c2af33a275b273130538b83a409d1"), 16, 11842560),
    ("resnet", (2, 128, 256, 50), (58, "4b087fa8e09ba6211f6dca6810b915e7a950fa08094b40657c35dde66d321df4"), 21, 29616128),
    ("resnet", (1, 256, 256, 50), (58, "b6d64878918cb59c6b989b789664c17fec245c364712b8ed9d04de5250365c21"), 21, 29258752),
]


@pytest.mark.parametrize("family,args,digest,buffers,nbytes", PLANS_AS_THEY_WERE,
                         ids=[f"{row[0]}-{'x'.join(map(str, row[1]))}" for row in PLANS_AS_THEY_WERE])
def test_plan_is_what_it_was(family, args, digest, buffers, nbytes):
    """recorded from the commits in which the plans were written out by hand: the first row before the ResNet engine shared
    HipPlan's helpers, the others before both plans were derived from the networks' descriptions"""
    plan = {"hrnet": bb.HipPlan, "resnet": rn.ResNetPlan}[family](*args)
    assert plan_digest(plan) == digest
    print(f"{family} {args}: {len(plan.buffers)} buffers, {plan.nbytes()} bytes")
    assert len(plan.buffers) <= buffers and plan.nbytes() <= nbytes


@pytest.mark.parametrize("version", ru.VERSIONS)
@pytest.mark.parametrize("views,h,w", [(2, 128, 256), (1, 256, 256)])
def test_plan(version, views, h, w):
    plan = rn.ResNetPlan(views, h, w, version)
    specs = rn._conv_specs(version)
    launched = [op["conv"] for op in plan.ops if "conv" in op]
    assert launched == [s[0] for s in specs]                                   # every convolution once, in _conv_specs order
    kinds = {}
    for op in plan.ops:
        kinds[op["kind"]] = kinds.get(op["kind"], 0) + 1
    n3 = sum(s[4] == 3 for s in specs)
    n1 = sum(s[4] == 1 and s[5] == 1 for s in specs)
    want = {"stem": 1, "pool3": 1, "conv3": n3, "conv1s2": 3, "level": 4}
    if n1:
        want["conv1"] = n1
    assert kinds == want and (n3, n1) == {18: (16, 0), 34: (32, 0), 50: (16, 33)}[version]
    assert len(plan.ops) - 4 == {18: 21, 34: 37, 50: 54}[version]               # launches; the four level copies are not launches
    by_name = {s[0]: s for s in specs}
    for op in plan.ops:
        if op["kind"] in ("conv3", "conv1", "conv1s2"):
            _, _, cout, cin, k, stride = by_name[op["conv"]]
            x, out = op["in"], op["out"]
            assert (x.c, out.c, op["stride"]) == (cin, cout, stride) and (out.h, out.w) == (x.h // stride, x.w // stride)
            assert (out.h * out.w) % 32 == 0
            if op["kind"] == "conv3":
                assert x.bordered, op["conv"]                                  # every 3x3 input is the interior of a bordered buffer
            if op["res"] is not None:
                assert op["res"].geometry[:3] == out.geometry[:3] and op["relu"]
    stem, pool = plan.ops[0], plan.ops[1]
    assert stem["kind"] == "stem" and stem["out"].geometry == (64, h // 2, w // 2, False)
    assert pool["in"] is stem["out"] and pool["out"].geometry[:3] == (64, h // 4, w // 4)
    levels = [op for op in plan.ops if op["kind"] == "level"]
    assert [op["index"] for op in levels] == [0, 1, 2, 3] and [op["in"] for op in levels] == plan.outputs
    assert [(m.c, m.h, m.w) for m in plan.outputs] == [(c, h >> (2 + i), w >> (2 + i)) for i, c in enumerate(rn.level_channels(version))]
    # a pooled buffer is written again only after the last launch that reads what it held
    last_read = {}
    for t, op in enumerate(plan.ops):
        for m in (op.get("in"), op.get("res")):
            if m is not None:
                last_read[m.vid] = t
    held = {}
    for t, op in enumerate(plan.ops):
        out = op.get("out")
        if out is not None:
            assert last_read.get(held.get(out.buf), -1) < t, (t, op.get("conv"))
            held[out.buf] = out.vid
    total = sum(4 * int(np.prod(plan.buffer_shape(b))) for b in range(len(plan.buffers)))
    assert plan.nbytes() == total > 0
    print(f"resnet{version} {views}x{h}x{w}: {len(plan.ops) - 4} launches, {len(plan.buffers)} buffers, {plan.nbytes() / 2 ** 20:.1f} MiB")


def test_plan_refuses_other_inputs():
    for h, w in ((64, 64), (224, 224), (128, 250), (0, 256)):
        with pytest.raises(ValueError):
            rn.ResNetPlan(1, h, w, 18)
    with pytest.raises(ValueError):
        rn.ResNetPlan(1, 256, 256, 101)
    net = rn.ResNet18({"ENGINE": "hip"})
    with pytest.raises(ValueError):
        net(torch.zeros(1, 3, 64, 64))                                         # the shape check comes before anything else


# ---- the model ----------------------------------------------------------------------------------------------------------
def _model_node(backbone, in_channels):
    node = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": dict(pk.configs.head_cfg(128), IN_CHANNELS=in_channels),
            "DATA_PRESET": {"CENTER_IDX": 9}}
    if backbone is not None:
        node["BACKBONE"] = backbone
    return pk.CN(node)


def test_model_builds_its_backbone_from_the_registry(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)              # the constructor allocates nothing on the device
    m = pk.build_model(_model_node({"TYPE": "ResNet34", "PRETRAINED": False, "FREEZE_BATCHNORM": True}, 128))
    assert type(m.img_backbone) is rn.ResNet34 and m.img_backbone.name == "resnet34" and m.img_backbone.engine == "torch"
    assert pk.decode.FEAT_SIZES[m.img_backbone.name] == (64, 128, 256, 512) and m.ptEmb_head.in_channels == 128
    assert type(pk.build_model(_model_node({"TYPE": "ResNet50", "ENGINE": "hip"}, 512)).img_backbone) is rn.ResNet50
    with pytest.raises(ValueError, match=r"160.*resnet34.*128"):
        pk.build_model(_model_node({"TYPE": "ResNet34"}, 160))
    with pytest.raises(ValueError, match=r"128.*HRNet.*160"):
        pk.build_model(_model_node(None, 128))
    with pytest.raises(ValueError, match="PRETRAINED"):
        pk.build_model(_model_node({"TYPE": "ResNet18", "PRETRAINED": True}, 128))
    with pytest.raises(KeyError):
        pk.build_model(_model_node({"TYPE": "ResNet101"}, 512))
    for node in (None, {"ENGINE": "torch"}):                                   # no TYPE: HRNet, as before
        m = pk.build_model(_model_node(node, 160))
        assert type(m.img_backbone) is bb.HRNet and m.img_backbone.name == "HRNet"


def test_eval_single_takes_a_backbone():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "scripts"))
    try:
        import eval_single
    finally:
        sys.path.pop(0)
    base = ["--cfg", "c.yaml", "--dataset", "DexYCBMV", "--view_min", "2", "--view_max", "4", "--model", "small", "-g", "0"]
    assert set(eval_single.BACKBONE_TYPES) == {"hrnet", "resnet18", "resnet34", "resnet50"}
    for kind in eval_single.BACKBONE_TYPES.values():
        assert pk.builder.BACKBONE.get(kind) is not None
    parser = eval_single.build_cli()
    assert not hasattr(parser.parse_args(base), "backbone")                   # absent unless given: hrnet
    assert parser.parse_args(base + ["--backbone", "resnet50"]).backbone == "resnet50"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--backbone", "resnet101"])
