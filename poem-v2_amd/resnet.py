"""ResNet-18 / 34 / 50 feature pyramids, the POEM-v1 lineage of backbones, on the two engines of backbone.py (``cfg.ENGINE``;
DESIGN.md section 7 row H2):

``"torch"`` (default)  plain PyTorch-ROCm / MIOpen.
``"hip"``              the same list of convolutions on the project's own gfx950 kernels: the stem on ``poem_conv7x7_s2`` and
                       ``poem_maxpool3x3_s2``, the stride-2 shortcuts on ``poem_conv1x1_s2`` (csrc/resnet.hip), the BasicBlock /
                       Bottleneck bodies on ``poem_conv3x3_ex`` and ``poem_conv1x1`` as the HRNet engine uses them.  Opt-in; exact fp32.

Behaviour follows the reference's lib/models/backbones/resnet.py: ``conv1`` (7x7, stride 2) -> ``bn1`` -> ReLU -> MaxPool2d(3, 2, 1)
-> ``layer1..4`` of BasicBlocks (18: [2,2,2,2], 34: [3,4,6,3]; :77-106) or Bottlenecks (50: [3,4,6,3], stride on ``conv2``;
:109-144); the forward returns the four levels finest first (``layer1`` .. ``layer4``), which is what the model's
``extract_img_feat`` hands on (POEM.py:229-237).  The state_dict key names are the reference's (``conv1`` / ``bn1``,
``layerL.B.conv{1,2,3}`` / ``bn{1,2,3}``, ``layerL.B.downsample.{0,1}``), so a checkpoint's ``img_backbone.*`` tensors load by
key; ``fc.*`` and ``*.num_batches_tracked`` are dead.  ``FrozenBatchNorm2d`` (:59-74) and an eval-mode ``nn.BatchNorm2d`` are the
same arithmetic (eps 1e-5), so ``FREEZE_BATCHNORM`` is accepted and changes nothing: every BatchNorm is folded into the
convolution in front of it once at load time (fp64), as backbone.py does.  ResNet-101 / 152 are not built (the model's own assert
excludes them), ``EARLY_RETURN`` below 4 is refused (the model needs all four levels), and ``PRETRAINED`` is refused: upstream
downloads ImageNet weights from a URL there, this package never opens a connection -- pass a state dict.

This module holds the family's description (``resnet``) and configuration rules; the key table, both engines and the classes'
behaviour are backbone.py's walkers over that description.  The hip engine's plan is ``ResNetPlan(views, H, W, version)``: the
launch list in ``_conv_specs`` order, zero-bordered buffers pooled by geometry, allocated zeroed once, only interiors written.
The four returned levels are fresh tensors of every call (copied out of the plan's buffers).  Inputs follow
``check_hip_input``.  The launches -- 21 / 37 / 54 of them -- go to the current stream with no host wait in between and are NOT
captured into a graph, as for HRNet, so at a handful of views the forward is bound by launch overhead."""
from .backbone import Graph, Plan, _Backbone, _cfg_get, conv_specs, param_shapes, seeded_state_dict
from .builder import BACKBONE

VERSIONS = {18: ("basic", (2, 2, 2, 2)), 34: ("basic", (3, 4, 6, 3)), 50: ("bottleneck", (3, 4, 6, 3))}
PLANES = (64, 128, 256, 512)


def level_channels(version):
    """channel counts of the four returned levels, finest first"""
    e = 4 if VERSIONS[int(version)][0] == "bottleneck" else 1
    return tuple(p * e for p in PLANES)


def resnet(g, version):
    """resnet.py:77-144, 152-: the shortcut of a block in front of the convolution that adds it"""
    kind, layers = VERSIONS[int(version)]
    basic = kind == "basic"
    x = g.maxpool3(g.conv("conv1", g.image, 64, 7, 2, relu=True))
    for L, (planes, nblocks) in enumerate(zip(PLANES, layers), start=1):
        cout = planes if basic else 4 * planes
        for b in range(nblocks):
            p, stride = f"layer{L}.{b}", (2 if b == 0 and L > 1 else 1)
            if basic:                                                # relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x))
                t = g.conv(f"{p}.conv1", x, planes, 3, stride, relu=True)
            else:                                                    # Bottleneck: 1x1 -> 3x3 (stride) -> 1x1, expansion 4
                t = g.conv(f"{p}.conv1", x, planes, 1, relu=True)
                t = g.conv(f"{p}.conv2", t, planes, 3, stride, relu=True)
            r = x if stride == 1 and x.c == cout else g.conv(f"{p}.downsample.0", x, cout, 1, stride)
            x = g.conv(f"{p}.conv2" if basic else f"{p}.conv3", t, cout, 3 if basic else 1, relu=True, res=r)
        g.level(x)


def _conv_specs(version):
    """``conv_specs`` of every live conv -> BatchNorm pair in the reference's key names, in the order a forward evaluates them."""
    return conv_specs(Graph(resnet, version))


def resnet_param_shapes(version):
    return param_shapes(_conv_specs(version))


def seeded_resnet_state_dict(version, seed=0):
    """the recipe of ``seeded_hrnet_state_dict``; the small convolution is the last one of every residual block"""
    last = ".conv2.weight" if VERSIONS[int(version)][0] == "basic" else ".conv3.weight"
    return seeded_state_dict(resnet_param_shapes(version), 7100 + 10 * int(version) + seed,
                             lambda name: 0.3 if name.endswith(last) and name.startswith("layer") else 1.0)


def is_dead_key(key):
    """a key of the reference's ResNet state_dict that no forward reads"""
    return key.startswith("fc.") or key.endswith(".num_batches_tracked")


class ResNetPlan(Plan):
    """``Plan`` of ResNet-``version``"""

    def __init__(self, views, H, W, version):
        self.version = int(version)
        if self.version not in VERSIONS:
            raise ValueError(f"ResNet-{version} is not built: one of {sorted(VERSIONS)}")
        super().__init__(Graph(resnet, self.version), views, H, W)


class _ResNet(_Backbone):
    """``ResNetNN(cfg)`` as the reference registers it (resnet.py:311-347)"""
    VERSION = None

    def _configure(self, cfg):
        self.version = v = int(self.VERSION)
        self.name = f"resnet{v}"                                         # resnet.py:152
        if _cfg_get(cfg, "PRETRAINED", False):
            raise ValueError(f"BACKBONE.PRETRAINED: upstream downloads ImageNet weights for {self.name} from a URL; this package "
                             "never opens a connection -- set PRETRAINED to False and pass the weights as a state dict "
                             "(load_state_dict)")
        early = _cfg_get(cfg, "EARLY_RETURN", 4)
        if early is not None and int(early) != 4:
            raise ValueError(f"BACKBONE.EARLY_RETURN = {early}: the model needs all four levels, only 4 (or absent) is accepted")
        self.freeze_batchnorm = bool(_cfg_get(cfg, "FREEZE_BATCHNORM", True))     # the same arithmetic either way (folded)
        graph = Graph(resnet, v)
        return graph, conv_specs(graph), lambda views, H, W: ResNetPlan(views, H, W, v)


@BACKBONE.register_module()
class ResNet18(_ResNet):
    VERSION = 18


@BACKBONE.register_module()
class ResNet34(_ResNet):
    VERSION = 34


@BACKBONE.register_module()
class ResNet50(_ResNet):
    VERSION = 50
