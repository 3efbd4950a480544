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

The hip engine is a device-free plan like ``HipPlan`` (``ResNetPlan(views, H, W, version)``): the launch list in
``_conv_specs`` order, zero-bordered buffers pooled by geometry, allocated zeroed once, only interiors written.  The four
returned levels are fresh tensors of every call (copied out of the plan's buffers).  Inputs follow ``check_hip_input``.  The
launches -- 21 / 37 / 54 of them -- go to the current stream with no host wait in between and are NOT captured into a graph, as
for HRNet, so at a handful of views the forward is bound by launch overhead."""
import torch
import torch.nn.functional as F

from .backbone import _FoldedConv, _HipEngine, _cfg_engine, HipPlan, check_hip_input
from .builder import BACKBONE

VERSIONS = {18: ("basic", (2, 2, 2, 2)), 34: ("basic", (3, 4, 6, 3)), 50: ("bottleneck", (3, 4, 6, 3))}
PLANES = (64, 128, 256, 512)


def level_channels(version):
    """channel counts of the four returned levels, finest first"""
    e = 4 if VERSIONS[int(version)][0] == "bottleneck" else 1
    return tuple(p * e for p in PLANES)


def _conv_specs(version):
    """(conv key, bn key, cout, cin, kernel, stride) of every live conv -> BatchNorm pair in the reference's key names, in the
    order a forward evaluates them (the shortcut of a block in front of the convolution that adds it)."""
    kind, layers = VERSIONS[int(version)]
    specs = [("conv1", "bn1", 64, 3, 7, 2)]
    cin = 64
    for L, (planes, nblocks) in enumerate(zip(PLANES, layers), start=1):
        for b in range(nblocks):
            p, stride = f"layer{L}.{b}", (2 if b == 0 and L > 1 else 1)
            if kind == "basic":
                cout = planes
                specs.append((f"{p}.conv1", f"{p}.bn1", planes, cin, 3, stride))
                if stride != 1 or cin != cout:
                    specs.append((f"{p}.downsample.0", f"{p}.downsample.1", cout, cin, 1, stride))
                specs.append((f"{p}.conv2", f"{p}.bn2", planes, planes, 3, 1))
            else:
                cout = 4 * planes
                specs.append((f"{p}.conv1", f"{p}.bn1", planes, cin, 1, 1))
                specs.append((f"{p}.conv2", f"{p}.bn2", planes, planes, 3, stride))
                if stride != 1 or cin != cout:
                    specs.append((f"{p}.downsample.0", f"{p}.downsample.1", cout, cin, 1, stride))
                specs.append((f"{p}.conv3", f"{p}.bn3", cout, planes, 1, 1))
            cin = cout
    return specs


def resnet_param_shapes(version):
    """name -> shape of every live tensor (conv weights + BatchNorm affine / statistics)."""
    shapes = {}
    for conv, bn, cout, cin, k, _ in _conv_specs(version):
        shapes[f"{conv}.weight"] = (cout, cin, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{bn}.{n}"] = (cout,)
    return shapes


def seeded_resnet_state_dict(version, seed=0):
    """Seeded weights with non-trivial BatchNorm statistics (the recipe of ``seeded_hrnet_state_dict``); the last convolution of
    every residual block is small so that activations stay O(1) through the layers without trained statistics."""
    kind = VERSIONS[int(version)][0]
    last = ".conv2.weight" if kind == "basic" else ".conv3.weight"
    g = torch.Generator().manual_seed(7100 + 10 * int(version) + seed)
    sd = {}
    for name, shape in resnet_param_shapes(version).items():
        if name.endswith("running_var"):
            sd[name] = 0.5 + torch.rand(shape, generator=g)
        elif name.endswith("running_mean"):
            sd[name] = 0.1 * torch.randn(shape, generator=g)
        elif len(shape) == 1 and name.endswith(".weight"):
            sd[name] = 1.0 + 0.2 * (torch.rand(shape, generator=g) * 2 - 1)
        elif len(shape) == 1:
            sd[name] = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            gain = 0.3 if name.endswith(last) and name.startswith("layer") else 1.0
            sd[name] = torch.randn(shape, generator=g) * (gain * (1.6 / fan_in) ** 0.5)
    return sd


def is_dead_key(key):
    """a key of the reference's ResNet state_dict that no forward reads"""
    return key.startswith("fc.") or key.endswith(".num_batches_tracked")


# ---- the "hip" engine -----------------------------------------------------------------------------------------------------
class ResNetPlan(HipPlan):
    """The hip engine's forward for one (views, H, W, version), device-free: ``ops`` (dicts: kind "stem" | "pool3" | "conv3" |
    "conv1" | "conv1s2" | "level"; ``conv`` = the _conv_specs key; ``in`` / ``out`` / ``res`` = _Map; level: ``index``) in launch
    order, ``buffers`` (geometry of buffer id) and ``outputs`` (the maps the four levels are copied out of)."""

    def __init__(self, views, H, W, version):
        self.version = int(version)
        if self.version not in VERSIONS:
            raise ValueError(f"ResNet-{version} is not built: one of {sorted(VERSIONS)}")
        super().__init__(views, H, W)

    def _conv1s2(self, name, x, cout):
        out = self._new(cout, x.h // 2, x.w // 2, False)
        self.ops.append({"kind": "conv1s2", "conv": name, "in": x, "out": out, "res": None, "stride": 2, "relu": False})
        return out

    def _build(self):
        kind, layers = VERSIONS[self.version]
        basic = kind == "basic"
        s = self._new(64, self.H // 2, self.W // 2, False)
        self.ops.append({"kind": "stem", "conv": "conv1", "in": None, "out": s, "res": None, "stride": 2, "relu": True})
        x = self._new(64, self.H // 4, self.W // 4, basic)               # a 3x3 convolution reads it next (BasicBlock)
        self.ops.append({"kind": "pool3", "in": s, "out": x})
        self._release(s)
        self.outputs = []
        for L, (planes, nblocks) in enumerate(zip(PLANES, layers), start=1):
            for b in range(nblocks):
                p, first = f"layer{L}.{b}", b == 0
                stride = 2 if first and L > 1 else 1
                final = L == 4 and b == nblocks - 1                      # nothing but the level copy reads it
                if basic:                                                # relu(bn2(conv2(relu(bn1(conv1(x))))) + shortcut(x))
                    t = self._conv3(f"{p}.conv1", x, planes, stride, True)
                    r = self._conv1s2(f"{p}.downsample.0", x, planes) if stride == 2 else x
                    y = self._conv3(f"{p}.conv2", t, planes, 1, True, res=r, bordered_out=not final)
                else:                                                    # Bottleneck: 1x1 -> 3x3 (stride) -> 1x1, expansion 4
                    t1 = self._conv1(f"{p}.conv1", x, planes, True)
                    t = self._conv3(f"{p}.conv2", t1, planes, stride, True, bordered_out=False)
                    self._release(t1)
                    if not first:
                        r = x
                    elif stride == 2:
                        r = self._conv1s2(f"{p}.downsample.0", x, 4 * planes)
                    else:
                        r = self._conv1(f"{p}.downsample.0", x, 4 * planes, False, bordered_out=False)
                    y = self._conv1(f"{p}.conv3", t, 4 * planes, True, res=r, bordered_out=False)
                self._release(t)
                if r is not x:
                    self._release(r)
                self._release(x)
                x = y
            self.ops.append({"kind": "level", "in": x, "index": L - 1})
            self.outputs.append(x)
        self._release(x)


class _ResNetHipEngine(_HipEngine):
    """The folded convolutions packed once for the kernels, and the buffers of every plan run so far."""

    def __init__(self, convs, device, version):
        self.version = version
        super().__init__(convs, device)

    def _pack(self, name, w, bias):
        if int(w.shape[-1]) != 7:
            return super()._pack(name, w, bias)
        hip, L = self.hip, self.hip.lib()
        cout, w = int(w.shape[0]), w.contiguous()
        packed = torch.empty(L.poem_conv7x7_packed_bytes(cout), dtype=torch.uint8, device=self.device)
        hip.check(L.poem_pack_conv7x7(hip.ptr(w), cout, packed.data_ptr(), hip.stream()), "poem_pack_conv7x7")
        return (packed, torch.ones_like(bias).contiguous(), bias.contiguous(), 3, cout)      # the scale is in the weight

    def _make_plan(self, views, H, W):
        return ResNetPlan(views, H, W, self.version)

    def _bind(self, plan, bufs):
        """plan.ops as (name, function, arguments) with every pointer resolved but the image's, or ("level", index, view)"""
        L, views = self.hip.lib(), plan.views
        ptr = lambda m: bufs[m.buf].data_ptr()      # noqa: E731
        calls = []
        for op in plan.ops:
            kind, x, out = op["kind"], op["in"], op.get("out")
            if kind == "level":
                src = bufs[x.buf]
                calls.append(("level", op["index"], src[:, :, 1:-1, 1:-1] if x.bordered else src))
            elif kind == "stem":
                packed, scale, shift, _, cout = self.w["conv1"]
                assert cout == out.c
                args = [None, packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), ptr(out), *out.strides, views, cout, plan.H, plan.W]
                calls.append(("poem_conv7x7_s2", L.poem_conv7x7_s2, args))
            elif kind == "pool3":
                args = [ptr(x), *x.strides, ptr(out), *out.strides, views, x.c, x.h, x.w]
                calls.append(("poem_maxpool3x3_s2", L.poem_maxpool3x3_s2, args))
            elif kind == "conv1s2":
                packed, _, shift, cin, cout = self.w[op["conv"]]
                assert (cin, cout) == (x.c, out.c), op["conv"]
                args = [ptr(x), *x.strides, packed.data_ptr(), shift.data_ptr(), ptr(out), *out.strides, views, cin, cout, x.h, x.w]
                calls.append(("poem_conv1x1_s2", L.poem_conv1x1_s2, args))
            else:
                what, fn, _, args = self._conv_call(op, ptr, views)
                calls.append((what, fn, args))
        return calls

    def forward(self, x):
        views, H, W = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
        plan, _, calls = self.plan(views, H, W)
        x = x.contiguous()
        outs = [None] * len(plan.outputs)
        stream, check = self.hip.stream(), self.hip.check
        for call in calls:
            if call[0] == "level":
                outs[call[1]] = call[2].clone(memory_format=torch.contiguous_format)
                continue
            what, fn, args = call
            if what == "poem_conv7x7_s2":                 # the image is the caller's tensor
                args = [self.hip.ptr(x)] + args[1:]
            check(fn(*args, stream), what)
        return outs


def _cfg_get(cfg, key, default=None):
    if cfg is None:
        return default
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


class _ResNet:
    """``ResNetNN(cfg)`` as the reference registers it (resnet.py:311-347); weights arrive through ``load_state_dict``."""
    VERSION = None

    def __init__(self, cfg=None, state_dict=None, device="cpu"):
        self.version = int(self.VERSION)
        self.name = f"resnet{self.version}"                              # resnet.py:152
        self.device = torch.device(device)
        self.engine = _cfg_engine(cfg)
        if _cfg_get(cfg, "PRETRAINED", False):
            raise ValueError(f"BACKBONE.PRETRAINED: upstream downloads ImageNet weights for {self.name} from a URL; this package "
                             "never opens a connection -- set PRETRAINED to False and pass the weights as a state dict "
                             "(load_state_dict)")
        early = _cfg_get(cfg, "EARLY_RETURN", 4)
        if early is not None and int(early) != 4:
            raise ValueError(f"BACKBONE.EARLY_RETURN = {early}: the model needs all four levels, only 4 (or absent) is accepted")
        self.freeze_batchnorm = bool(_cfg_get(cfg, "FREEZE_BATCHNORM", True))     # the same arithmetic either way (folded)
        self._specs = _conv_specs(self.version)
        self._shapes = resnet_param_shapes(self.version)
        self._hip = None
        self._built = False
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # -- weights ------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, prefix="", strict=False):
        missing = [k for k in self._shapes if prefix + k not in state_dict]
        if missing:
            raise KeyError(f"{self.name} checkpoint lacks {missing[:4]}{'...' if len(missing) > 4 else ''}")
        sd = {k: state_dict[prefix + k].detach().cpu() for k in self._shapes}
        for k, shape in self._shapes.items():
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)}, expected {shape}")
        self._convs = {conv: _FoldedConv(sd, conv, bn, stride, self.device) for conv, bn, _, _, _, stride in self._specs}
        if self.engine == "hip":
            self._hip = _ResNetHipEngine(self._convs, self.device, self.version)
        self._built = True
        return [k for k in state_dict if k.startswith(prefix) and k[len(prefix):] not in sd]    # ignored (fc, counters)

    def to(self, device):
        self.device = torch.device(device)
        if self._built:
            for c in self._convs.values():
                c.weight, c.bias = c.weight.to(self.device), c.bias.to(self.device)
            if self.engine == "hip":
                self._hip = _ResNetHipEngine(self._convs, self.device, self.version)
        return self

    def eval(self):
        return self

    # -- forward ------------------------------------------------------------------------------------------------
    def _block(self, p, x):
        c = self._convs
        out = c[f"{p}.conv1"](x, relu=True)
        out = c[f"{p}.conv2"](out, relu=f"{p}.conv3" in c)
        if f"{p}.conv3" in c:
            out = c[f"{p}.conv3"](out)
        res = c[f"{p}.downsample.0"](x) if f"{p}.downsample.0" in c else x
        return F.relu_(out.add_(res))

    @torch.no_grad()
    def forward(self, x=None, **kwargs):
        """x (BN,3,H,W) (or ``image=``, as upstream calls it) -> the four levels [(BN,C1,H/4,W/4) .. (BN,C4,H/32,W/32)]"""
        if x is None:
            x = kwargs["image"]
        if self.engine == "hip":
            check_hip_input(int(x.shape[-2]), int(x.shape[-1]))
        if not self._built:
            raise RuntimeError(f"{self.name} has no weights: call load_state_dict first")
        x = x.to(device=self.device, dtype=torch.float32)
        if self.engine == "hip":
            return self._hip.forward(x)
        x = self._convs["conv1"](x, relu=True)
        x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        levels = []
        for L, nblocks in enumerate(VERSIONS[self.version][1], start=1):
            for b in range(nblocks):
                x = self._block(f"layer{L}.{b}", x)
            levels.append(x)
        return levels

    __call__ = forward


@BACKBONE.register_module()
class ResNet18(_ResNet):
    VERSION = 18


@BACKBONE.register_module()
class ResNet34(_ResNet):
    VERSION = 34


@BACKBONE.register_module()
class ResNet50(_ResNet):
    VERSION = 50
