"""HRNet-W40 feature pyramid, and what every backbone of the package shares (resnet.py is the other family), on one of two
engines (``cfg.ENGINE``):

``"torch"`` (default)  plain PyTorch-ROCm / MIOpen -- what ``bench.py --e2e`` and every existing entry point run; its results
                       are untouched by the other engine's existence.
``"hip"``              the same list of convolutions on the project's own gfx950 kernels: the 3x3 convolutions on
                       ``poem_conv3x3_ex`` (residual before the ReLU, csrc/decode.hip), the 1x1 convolutions on ``poem_conv1x1``
                       and the fuse sums on ``poem_hrnet_fuse`` (csrc/hrnet.hip).  Opt-in; exact fp32.

Behaviour follows the reference's trimmed classification HRNet (lib/models/backbones/hrnet.py:240-420: stem of two
stride-2 3x3 convs, a Bottleneck stage, then 1 / 4 / 3 HighResolutionModules with 2 / 3 / 4 branches, the
classification head constructed but never run) with the widths of config/backbone/cls_hrnet_w40_*.yaml.  The state_dict
key names are the reference's (``conv1``, ``bn1``, ``layer1.N.*``, ``transitionS.I.*``, ``stageS.M.branches.B.K.*``,
``stageS.M.fuse_layers.I.J.*``), so a checkpoint's ``img_backbone.*`` tensors load by key; the dead classification
head (``incre_modules`` / ``downsamp_modules`` / ``final_layer`` / ``classifier``) is ignored.

A network is written once, as a function (``hrnet`` here) against ``Graph``: a recorder with the operations the networks
have -- conv -> folded BatchNorm -> [+ residual] -> [ReLU], the 3x3 max-pool, HRNet's fuse sum -- that turns it into a flat
node list without a device or an image size.  Everything else walks that list: the key table (``conv_specs``), the torch
engine (``run_graph``: every eval-mode BatchNorm is folded into the convolution in front of it once at load time in fp64, so
a forward is conv (+bias) -> [add] -> [ReLU] calls only, on whatever device the tensors live on), and the hip engine's plan.

The hip engine (``Plan`` + ``_HipEngine`` below).  ``HipPlan(views, H, W)`` is the node list turned into launches and the
buffers they read and write.  Layout and lifetime are derived: an activation that a 3x3 convolution reads is the interior of
a zero-bordered buffer, and a buffer returns to the pool of its geometry after the last launch that reads it.  A buffer keeps
the shape it was planned with, and a plan belongs to one (views, H, W); buffers are allocated zeroed once, and only interiors
are ever written, so the borders stay zero.  The four returned levels are fresh tensors of every call.  All launches go to the
current stream with no host wait in between; they are about 300 (``len(plan.ops)``) and are NOT captured into a graph, so at a
handful of views the forward is bound by launch overhead.  Inputs: H and W multiples of 32 with (H/32)*(W/32) a multiple of 32
(256x256, 128x256, 512x512; not 64x64 or 224x224): ``ValueError`` otherwise.  Memory: ``plan.nbytes()`` -- 6.7 GiB of
activations at 256 views of 256x256 (26.9 MiB per view), kept for as long as the HRNet object lives, once per distinct
(views, H, W) it has seen."""
import ctypes
from collections import namedtuple

import torch
import torch.nn.functional as F

from .builder import BACKBONE

ENGINES = ("torch", "hip")
BN_EPS = 1e-5
WIDTHS = (40, 80, 160, 320)                     # cls_hrnet_w40 NUM_CHANNELS of stage 4
STAGES = ((2, 1), (3, 4), (4, 3))               # (branches, modules) of stages 2..4; 4 BasicBlocks per branch
BLOCKS_PER_BRANCH = 4


# ---- describing a network ---------------------------------------------------------------------------------------------------
class _Value:
    """One activation of a description: ``c`` channels at 1 / 2**``down`` of the image's height and width.  ``border``: kept
    zero-bordered by the plan although no 3x3 convolution reads it (the one layout statement a description can make)."""
    __slots__ = ("vid", "c", "down", "border")

    def __init__(self, vid, c, down, border=False):
        self.vid, self.c, self.down, self.border = vid, c, down, border


class Node(namedtuple("Node", "op out x name k stride relu res terms", defaults=(None,) * 7)):
    """``op`` "conv" | "maxpool3" | "sum_relu" | "level"; ``x`` / ``res`` / ``terms`` = [(value, shift)] are what it reads"""
    __slots__ = ()

    @property
    def reads(self):
        return [v for v in (self.x, self.res) if v is not None] + [v for v, _ in self.terms or ()]


class Graph:
    """``Graph(describe, *args)``: the node list of the network that ``describe(graph, *args)`` writes out, in evaluation order;
    ``image`` is its input, ``readers[vid]`` the indices of the nodes that read a value, in order."""

    def __init__(self, describe, *args):
        self.nodes, self.values = [], []
        self.image = self._value(3, 0)
        describe(self, *args)
        self.readers = {v.vid: [] for v in self.values}
        for t, n in enumerate(self.nodes):
            for v in n.reads:
                self.readers[v.vid].append(t)

    def _value(self, c, down, border=False):
        self.values.append(_Value(len(self.values), c, down, border))
        return self.values[-1]

    def conv(self, name, x, cout, k, stride=1, relu=False, res=None, border=False):
        """conv -> folded BatchNorm -> [+ res] -> [ReLU]: the residual before the activation"""
        out = self._value(cout, x.down + stride.bit_length() - 1, border)
        self.nodes.append(Node("conv", out, x, name, k, stride, relu, res))
        return out

    def maxpool3(self, x):
        """MaxPool2d(3, 2, 1)"""
        self.nodes.append(Node("maxpool3", self._value(x.c, x.down + 1), x))
        return self.nodes[-1].out

    def sum_relu(self, terms):
        """relu(((t0 + t1) + t2) + ...) of [(value, shift)], a term 2**shift coarser read through nearest upsampling"""
        x, shift = terms[0]
        self.nodes.append(Node("sum_relu", self._value(x.c, x.down - shift), terms=list(terms)))
        return self.nodes[-1].out

    def level(self, x):
        """the next returned level is ``x``"""
        self.nodes.append(Node("level", None, x))


def hrnet(g, widths=WIDTHS):
    """hrnet.py:240-420"""
    x = g.conv("conv1", g.image, 64, 3, 2, relu=True)
    x = g.conv("conv2", x, 64, 3, 2, relu=True)
    for i in range(4):                                             # layer1: Bottleneck x4, planes 64, expansion 4
        p = f"layer1.{i}"
        t = g.conv(f"{p}.conv1", x, 64, 1, relu=True)
        t = g.conv(f"{p}.conv2", t, 64, 3, relu=True)
        r = g.conv(f"{p}.downsample.0", x, 256, 1) if i == 0 else x
        x = g.conv(f"{p}.conv3", t, 256, 1, relu=True, res=r)
    ys = [x]
    for s, (nb, nm) in enumerate(STAGES, start=1):
        cur, pre = widths[:nb], ys
        ys = []
        for i in range(nb):                                        # transition s (hrnet.py:319-344)
            if i < len(pre):                                       # hrnet.py:397-410: pre[-1], as upstream
                ys.append(pre[i] if cur[i] == pre[i].c else g.conv(f"transition{s}.{i}.0", pre[-1], cur[i], 3, relu=True))
            else:
                t = pre[-1]
                for j in range(i + 1 - len(pre)):
                    cout = cur[i] if j == i - len(pre) else pre[-1].c
                    t = g.conv(f"transition{s}.{i}.{j}.0", t, cout, 3, 2, relu=True)
                ys.append(t)
        for m in range(nm):
            ys = _hrnet_module(g, f"stage{s + 1}.{m}", ys)
    for y in ys:
        g.level(y)


def _hrnet_module(g, p, xs):
    nb, xs = len(xs), list(xs)
    for b in range(nb):
        for k in range(BLOCKS_PER_BRANCH):                         # BasicBlock: relu(conv2(relu(conv1(x))) + x)
            q, x = f"{p}.branches.{b}.{k}", xs[b]
            t = g.conv(f"{q}.conv1", x, x.c, 3, relu=True)
            # the coarsest branch's last map is read by 1x1 convolutions and its own sum only; the plan has always bordered it
            xs[b] = g.conv(f"{q}.conv2", t, x.c, 3, relu=True, res=x, border=(b == nb - 1 and k == BLOCKS_PER_BRANCH - 1))
    fused = []
    for i in range(nb):                                            # fuse layers (hrnet.py:177-212, 226-233)
        terms = []
        for j in range(nb):
            if j == i:
                terms.append((xs[j], 0))
            elif j > i:                                            # 1x1 at the low resolution; nearest upsampling in the sum
                terms.append((g.conv(f"{p}.fuse_layers.{i}.{j}.0", xs[j], xs[i].c, 1), j - i))
            else:
                t = xs[j]
                for k in range(i - j):
                    last = k == i - j - 1
                    t = g.conv(f"{p}.fuse_layers.{i}.{j}.{k}.0", t, xs[i].c if last else xs[j].c, 3, 2, relu=not last)
                terms.append((t, 0))
        fused.append(g.sum_relu(terms))
    return fused


# ---- the key table ----------------------------------------------------------------------------------------------------------
def conv_specs(graph):
    """(conv key, bn key, cout, cin, kernel, stride) of every conv -> BatchNorm pair in evaluation order.  The BatchNorm of
    ``....convN`` is ``....bnN`` and that of ``....0`` is ``....1`` in every key of the reference's."""
    specs = []
    for n in graph.nodes:
        if n.op == "conv":
            head, _, last = n.name.rpartition(".")
            bn = head + ("." if head else "") + ("1" if last == "0" else last.replace("conv", "bn"))
            specs.append((n.name, bn, n.out.c, n.x.c, n.k, n.stride))
    return specs


def _conv_specs(widths=WIDTHS):
    """``conv_specs`` of every live conv -> BatchNorm pair, in the reference's key names."""
    specs = conv_specs(Graph(hrnet, widths))
    # layer1.0's shortcut runs before the conv3 whose epilogue adds it but is listed after it: the seeded weights, and the
    # fixtures that hang on them, are drawn in this order
    i = [s[0] for s in specs].index("layer1.0.downsample.0")
    specs[i], specs[i + 1] = specs[i + 1], specs[i]
    return specs


def param_shapes(specs):
    """name -> shape of every live tensor (conv weights + BatchNorm affine / statistics)."""
    shapes = {}
    for conv, bn, cout, cin, k, _ in specs:
        shapes[f"{conv}.weight"] = (cout, cin, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{bn}.{n}"] = (cout,)
    return shapes


def seeded_state_dict(shapes, seed, gain):
    """Seeded weights with non-trivial BatchNorm statistics; ``gain(name)`` makes the last conv of every residual block small
    so that activations stay O(1) through the layers without trained statistics."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in shapes.items():
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
            sd[name] = torch.randn(shape, generator=g) * (gain(name) * (1.6 / fan_in) ** 0.5)
    return sd


def hrnet_param_shapes(widths=WIDTHS):
    return param_shapes(_conv_specs(widths))


def _hrnet_gain(name):
    if (".conv2.weight" in name and "branches" in name) or ".conv3.weight" in name:
        return 0.3
    return 0.45 if "fuse_layers" in name else 1.0


def seeded_hrnet_state_dict(seed=0, widths=WIDTHS):
    return seeded_state_dict(hrnet_param_shapes(widths), 7000 + seed, _hrnet_gain)


# ---- the "torch" engine -----------------------------------------------------------------------------------------------------
class _FoldedConv:
    """conv -> eval BatchNorm as one convolution with bias (fold in fp64, kept in fp32)."""

    def __init__(self, sd, conv, bn, stride, device):
        w = sd[f"{conv}.weight"].to(dtype=torch.float64)
        inv = sd[f"{bn}.weight"].to(torch.float64) / torch.sqrt(sd[f"{bn}.running_var"].to(torch.float64) + BN_EPS)
        self.weight = (w * inv.view(-1, 1, 1, 1)).float().to(device).contiguous()
        self.bias = (sd[f"{bn}.bias"].to(torch.float64) - sd[f"{bn}.running_mean"].to(torch.float64) * inv).float().to(device)
        self.stride = stride
        self.pad = w.shape[-1] // 2

    def __call__(self, x, relu=False):
        y = F.conv2d(x, self.weight, self.bias, stride=self.stride, padding=self.pad)
        return F.relu_(y) if relu else y


@torch.no_grad()
def run_graph(graph, convs, x):
    """The returned levels of ``graph`` for the image batch ``x``, on the folded convolutions ``convs`` in the dtype of ``x``
    and of their weights.  A value is dropped after the last node that reads it."""
    vals, levels = {graph.image.vid: x}, []
    for t, n in enumerate(graph.nodes):
        if n.op == "conv":
            y = convs[n.name](vals[n.x.vid], relu=n.relu and n.res is None)
            if n.res is not None:
                y = y.add_(vals[n.res.vid])
                y = F.relu_(y) if n.relu else y
        elif n.op == "maxpool3":
            y = F.max_pool2d(vals[n.x.vid], kernel_size=3, stride=2, padding=1)
        elif n.op == "sum_relu":
            y = None
            for v, shift in n.terms:
                term = F.interpolate(vals[v.vid], scale_factor=2 ** shift, mode="nearest") if shift else vals[v.vid]
                y = term if y is None else y + term
            y = F.relu(y)
        else:
            levels.append(vals[n.x.vid])
        if n.out is not None:
            vals[n.out.vid] = y
        for v in n.reads:
            if graph.readers[v.vid][-1] == t:
                vals.pop(v.vid, None)
    return levels


# ---- the "hip" engine -------------------------------------------------------------------------------------------------------
def _cfg_get(cfg, key, default=None):
    """``cfg.<key>`` of the BACKBONE node (a dict / CN, an object with attributes, or None)."""
    if cfg is None:
        return default
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


def _cfg_engine(cfg):
    eng = _cfg_get(cfg, "ENGINE", "torch")
    if eng not in ENGINES:
        raise ValueError(f"BACKBONE.ENGINE {eng!r}: expected one of {ENGINES}")
    return eng


def check_hip_input(H, W):
    """The shapes the kernels take: every level down to H/32 x W/32 is whole 32-pixel tiles."""
    if H <= 0 or W <= 0 or H % 32 or W % 32 or ((H // 32) * (W // 32)) % 32:
        raise ValueError(f'BACKBONE.ENGINE "hip" takes images whose H and W are multiples of 32 with (H/32)*(W/32) a multiple '
                         f"of 32 (256x256, 128x256, 512x512), not {H}x{W}: use the torch engine for it")


def _down2_takes(cout, h, w):
    """poem_conv3x3_down2's shapes (csrc/decode.hip conv3x3_s2_shape): it reads a PLAIN (unbordered) input."""
    return h == w and h % 16 == 0 and (cout, w) in ((80, 64), (160, 32), (320, 16))


class _Map:
    """One activation of a plan: (views, c, h, w) held by buffer ``buf`` -- the interior of a zero-bordered (views, c, h+2, w+2)
    buffer or a plain one.  ``buf < 0``: returned level -(buf + 1), a fresh tensor of every forward."""
    __slots__ = ("vid", "buf", "c", "h", "w", "bordered")

    def __init__(self, vid, buf, c, h, w, bordered):
        self.vid, self.buf, self.c, self.h, self.w, self.bordered = vid, buf, c, h, w, bordered

    @property
    def geometry(self):
        return (self.c, self.h, self.w, self.bordered)

    @property
    def strides(self):
        """(view, channel, row, offset) in floats: element (n, ch, y, x) at n*view + ch*channel + y*row + x + offset"""
        c, h, w = self.c, self.h, self.w
        if self.bordered:
            return (c * (h + 2) * (w + 2), (h + 2) * (w + 2), w + 2, w + 3)
        return (c * h * w, h * w, w, 0)


class Plan:
    """The hip engine's forward of ``graph`` for one (views, H, W), device-free: ``ops`` in launch order -- dicts of kind
    "stem" | "conv3" | "down2" | "conv1" | "conv1s2" (``conv`` = the conv_specs key; ``in`` / ``out`` / ``res`` = _Map; ``stride``,
    ``relu``), "pool3" (``in``, ``out``), "fuse" (``terms`` = [(_Map, shift)], ``out``), "input" (``out``: the image copied
    into a buffer) and "level" (``in``, ``index``: a returned level copied out of one) -- ``buffers`` (geometry of buffer id)
    and ``outputs`` (the maps of the four levels)."""
    STEM_CIN = 8          # a 3x3 stem's 3 input channels zero-padded to one 8-channel chunk

    def __init__(self, graph, views, H, W):
        check_hip_input(H, W)
        self.views, self.H, self.W = int(views), int(H), int(W)
        self.buffers, self.ops, self.outputs, self._free = [], [], [], {}
        self._build(graph)

    # -- buffers ----------------------------------------------------------------------------------------------------
    def _new(self, vid, c, down, bordered):
        geometry = (c, self.H >> down, self.W >> down, bordered)
        free = self._free.setdefault(geometry, [])
        if free:
            buf = free.pop()
        else:
            buf = len(self.buffers)
            self.buffers.append(geometry)
        return _Map(vid, buf, *geometry)

    def buffer_shape(self, buf):
        c, h, w, bordered = self.buffers[buf]
        return (self.views, c, h + 2, w + 2) if bordered else (self.views, c, h, w)

    def nbytes(self):
        total = 0
        for b in range(len(self.buffers)):
            n, c, h, w = self.buffer_shape(b)
            total += 4 * n * c * h * w
        return total

    # -- launches ---------------------------------------------------------------------------------------------------
    def _bordered(self, graph, v):
        """Zero-bordered if a 3x3 convolution takes it as its input -- unless its sole reader is a stride-2 3x3 without residual
        of a shape the LDS-staged ``poem_conv3x3_down2`` takes, which reads a plain map."""
        rd = [graph.nodes[t] for t in graph.readers[v.vid]]
        if len(rd) == 1 and rd[0].op == "conv" and (rd[0].k, rd[0].stride, rd[0].res) == (3, 2, None) \
                and _down2_takes(rd[0].out.c, self.H >> v.down, self.W >> v.down):
            return False
        return v.border or any(n.op == "conv" and n.k == 3 and n.x is v for n in rd)      # as its input, not as its residual

    def _build(self, graph):
        maps, img = {}, graph.image
        level_of = {n.x.vid: i for i, n in enumerate(n for n in graph.nodes if n.op == "level")}
        if any(graph.nodes[t].k == 3 for t in graph.readers[img.vid]):      # a 7x7 stem reads the caller's tensor instead
            maps[img.vid] = self._new(img.vid, self.STEM_CIN, 0, self._bordered(graph, img))
            self.ops.append({"kind": "input", "out": maps[img.vid]})
        for t, n in enumerate(graph.nodes):
            out = n.out
            if n.op == "level":                                  # copied out of its buffer: later layers may still read it
                m = maps[n.x.vid]
                if m.buf >= 0:
                    self.ops.append({"kind": "level", "in": m, "index": len(self.outputs)})
                self.outputs.append(m)
            elif n.op == "sum_relu" and all(graph.nodes[r].op == "level" for r in graph.readers[out.vid]):
                # a fuse sum that nothing but a level reads writes that level's fresh tensor itself
                maps[out.vid] = _Map(out.vid, -(level_of[out.vid] + 1), out.c, self.H >> out.down, self.W >> out.down, False)
            else:
                maps[out.vid] = self._new(out.vid, out.c, out.down, self._bordered(graph, out))
            if out is not None:
                self.ops.append(self._op(n, maps, maps[out.vid]))
            for vid in {v.vid for v in n.reads}:                 # after the output is allocated: a launch never writes what it reads
                m = maps.get(vid)
                if graph.readers[vid][-1] == t and m is not None and m.buf >= 0:
                    self._free[m.geometry].append(m.buf)

    def _op(self, n, maps, out):
        if n.op == "sum_relu":
            return {"kind": "fuse", "terms": [(maps[v.vid], shift) for v, shift in n.terms], "out": out}
        x = maps.get(n.x.vid)
        if n.op == "maxpool3":
            return {"kind": "pool3", "in": x, "out": out}
        res = None if n.res is None else maps[n.res.vid]
        if n.k == 7:
            kind = "stem"
            assert x is None and (n.stride, n.relu, res) == (2, True, None), n.name
        elif n.k == 3:
            kind = "conv3"
            if not x.bordered:                                   # a plain map feeds the LDS-staged stride-2 kernel only
                if n.stride != 2 or res is not None or not _down2_takes(out.c, x.h, x.w):
                    raise AssertionError(f"{n.name}: a plain input needs a shape poem_conv3x3_down2 takes")
                kind = "down2"
        else:
            kind = "conv1" if n.stride == 1 else "conv1s2"
            assert n.k == 1 and (n.stride == 1 or (n.stride, n.relu, res) == (2, False, None)), n.name
        return {"kind": kind, "conv": n.name, "in": x, "out": out, "res": res, "stride": n.stride, "relu": n.relu}


class HipPlan(Plan):
    """``Plan`` of HRNet"""

    def __init__(self, views, H, W, widths=WIDTHS):
        self.widths = tuple(widths)
        super().__init__(Graph(hrnet, self.widths), views, H, W)


def stem_weight(w):
    """conv1's folded (64, 3, 3, 3) weight with the input channels zero-padded to Plan.STEM_CIN"""
    out = torch.zeros(w.shape[0], Plan.STEM_CIN, 3, 3, dtype=w.dtype, device=w.device)
    out[:, :w.shape[1]] = w
    return out


class _PerForward:
    """What a bound plan learns only at a forward: the caller's image and the levels written straight into fresh tensors.
    The binders put these ``c_void_p`` slots into their argument lists; ``forward`` fills them before it launches."""

    def __init__(self, plan):
        self.image, self.image_ptr, self.levels = None, None, None
        self.level_ptrs = [ctypes.c_void_p() if m.buf < 0 else None for m in plan.outputs]


class _HipEngine:
    """The folded convolutions packed once for the kernels, and the buffers and bound launches of every plan run so far;
    ``plan_factory(views, H, W)`` makes the network's ``Plan``."""

    def __init__(self, convs, device, plan_factory):
        from . import hip
        from .decode import _pad32
        self.hip, self.device, self._pad32, self._plan_factory = hip, torch.device(device), _pad32, plan_factory
        self.w = {}                                      # conv key -> (packed weights, scale | None, shift, cin, cout)
        for name, c in convs.items():
            self.w[name] = self._pack(c.weight.to(self.device), c.bias.to(self.device))
        self._plans = {}

    def _pack(self, w, bias):
        hip, L = self.hip, self.hip.lib()
        if tuple(w.shape[1:]) == (3, 3, 3):              # a 3x3 stem: the plan pads the image to STEM_CIN channels
            w = stem_weight(w)
        cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        w = w.contiguous()
        if k == 7:
            packed = torch.empty(L.poem_conv7x7_packed_bytes(cout), dtype=torch.uint8, device=self.device)
            hip.check(L.poem_pack_conv7x7(hip.ptr(w), cout, packed.data_ptr(), hip.stream()), "poem_pack_conv7x7")
            return (packed, torch.ones_like(bias).contiguous(), bias.contiguous(), cin, cout)   # the scale is in the weight
        if k == 3:
            packed = torch.empty(L.poem_conv3x3_packed_bytes(cout, cin), dtype=torch.uint8, device=self.device)
            hip.check(L.poem_pack_conv3x3(hip.ptr(w), cout, cin, packed.data_ptr(), hip.stream()), "poem_pack_conv3x3")
            return (packed, self._pad32(torch.ones_like(bias)), self._pad32(bias), cin, cout)   # the scale is in the weight
        packed = torch.empty(L.poem_conv1x1_packed_bytes(cout, cin), dtype=torch.uint8, device=self.device)
        hip.check(L.poem_pack_conv1x1(hip.ptr(w), cout, cin, packed.data_ptr(), hip.stream()), "poem_pack_conv1x1")
        return (packed, None, bias.contiguous(), cin, cout)

    def plan(self, views, H, W):
        key = (views, H, W)
        if key not in self._plans:
            plan = self._plan_factory(views, H, W)
            bufs = [torch.zeros(plan.buffer_shape(b), dtype=torch.float32, device=self.device) for b in range(len(plan.buffers))]
            self._plans[key] = (plan, bufs) + self._bind(plan, bufs)
        return self._plans[key]

    # -- binding: one (name, function, arguments) per op, every pointer resolved or a slot of the plan's _PerForward ---------
    def _bind(self, plan, bufs):
        io = _PerForward(plan)
        ptr = lambda m: bufs[m.buf].data_ptr() if m.buf >= 0 else io.level_ptrs[-(m.buf + 1)]      # noqa: E731
        return [self._BINDERS[op["kind"]](self, op, ptr, plan, bufs, io) for op in plan.ops], io

    def _weights(self, op):
        packed, scale, shift, cin, cout = self.w[op["conv"]]
        x, out = op["in"], op["out"]
        assert (cin, cout) == (3 if x is None else x.c, out.c), op["conv"]
        return packed.data_ptr(), None if scale is None else scale.data_ptr(), shift.data_ptr(), cin, cout

    @staticmethod
    def _res(op, ptr):
        res = op["res"]
        return (ptr(res), *res.strides) if res is not None else (None, 0, 0, 0, 0)

    def _bind_input(self, op, ptr, plan, bufs, io):
        def copy_in(dst, stream):
            dst.copy_(io.image)
        return ("input", copy_in, [bufs[op["out"].buf][:, :3, 1:-1, 1:-1]])

    def _bind_level(self, op, ptr, plan, bufs, io):
        def copy_out(src, index, stream):
            io.levels[index] = src.clone(memory_format=torch.contiguous_format)
        x = op["in"]
        return ("level", copy_out, [bufs[x.buf][:, :, 1:-1, 1:-1] if x.bordered else bufs[x.buf], op["index"]])

    def _bind_stem(self, op, ptr, plan, bufs, io):
        packed, scale, shift, _, cout = self._weights(op)
        io.image_ptr, out = ctypes.c_void_p(), op["out"]                 # the image is the caller's tensor
        args = [io.image_ptr, packed, scale, shift, ptr(out), *out.strides, plan.views, cout, plan.H, plan.W]
        return ("poem_conv7x7_s2", self.hip.lib().poem_conv7x7_s2, args)

    def _bind_pool3(self, op, ptr, plan, bufs, io):
        x, out = op["in"], op["out"]
        args = [ptr(x), *x.strides, ptr(out), *out.strides, plan.views, x.c, x.h, x.w]
        return ("poem_maxpool3x3_s2", self.hip.lib().poem_maxpool3x3_s2, args)

    def _bind_conv3(self, op, ptr, plan, bufs, io):
        packed, scale, shift, cin, cout = self._weights(op)
        x, out = op["in"], op["out"]
        args = [ptr(x), packed, scale, shift, *self._res(op, ptr), 1, ptr(out), plan.views, cin, cout, x.h, x.w, op["stride"],
                int(op["relu"]), *out.strides]
        return ("poem_conv3x3_ex", self.hip.lib().poem_conv3x3_ex, args)

    def _bind_down2(self, op, ptr, plan, bufs, io):
        packed, scale, shift, cin, cout = self._weights(op)
        x, out = op["in"], op["out"]
        args = [ptr(x), packed, scale, shift, None, ptr(out), plan.views, cin, cout, x.h, x.w, int(op["relu"]), *out.strides]
        return ("poem_conv3x3_down2", self.hip.lib().poem_conv3x3_down2, args)

    def _bind_conv1(self, op, ptr, plan, bufs, io):
        packed, _, shift, cin, cout = self._weights(op)
        x, out = op["in"], op["out"]
        args = [ptr(x), *x.strides, packed, shift, *self._res(op, ptr), ptr(out), *out.strides, plan.views, cin, cout, x.h, x.w,
                int(op["relu"])]
        return ("poem_conv1x1", self.hip.lib().poem_conv1x1, args)

    def _bind_conv1s2(self, op, ptr, plan, bufs, io):
        packed, _, shift, cin, cout = self._weights(op)
        x, out = op["in"], op["out"]
        args = [ptr(x), *x.strides, packed, shift, ptr(out), *out.strides, plan.views, cin, cout, x.h, x.w]
        return ("poem_conv1x1_s2", self.hip.lib().poem_conv1x1_s2, args)

    def _bind_fuse(self, op, ptr, plan, bufs, io):
        terms, out = (self.hip.PoemFuseTerm * len(op["terms"]))(), op["out"]
        for t, (m, shift) in zip(terms, op["terms"]):
            ns, cs, rs, off = m.strides
            t.data, t.view_stride, t.ch_stride, t.row_stride, t.offset, t.shift = ptr(m), ns, cs, rs, off, shift
        args = [terms, len(terms), ptr(out), *out.strides, plan.views, out.c, out.h, out.w]
        return ("poem_hrnet_fuse", self.hip.lib().poem_hrnet_fuse, args)

    _BINDERS = {"input": _bind_input, "stem": _bind_stem, "pool3": _bind_pool3, "conv3": _bind_conv3, "down2": _bind_down2,
                "conv1": _bind_conv1, "conv1s2": _bind_conv1s2, "fuse": _bind_fuse, "level": _bind_level}

    def forward(self, x):
        views, H, W = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
        plan, _, calls, io = self.plan(views, H, W)
        if io.image_ptr is not None:
            x = x.contiguous()
            io.image_ptr.value = self.hip.ptr(x)
        io.image = x
        outs = io.levels = [None if m.buf >= 0 else torch.empty(views, m.c, m.h, m.w, dtype=torch.float32, device=self.device)
                            for m in plan.outputs]
        for slot, y in zip(io.level_ptrs, outs):
            if slot is not None:
                slot.value = y.data_ptr()
        stream, check = self.hip.stream(), self.hip.check
        for what, fn, args in calls:
            check(fn(*args, stream), what)
        io.image = io.levels = None
        return outs


# ---- the classes ------------------------------------------------------------------------------------------------------------
class _Backbone:
    """What ``HRNet`` and the ResNets share: weights arrive through ``load_state_dict`` and are folded once; ``forward`` runs
    the engine ``cfg.ENGINE`` names.  A family supplies ``_configure(cfg)``: it sets ``name``, applies the family's
    configuration rules and returns (description graph, conv_specs rows, plan factory)."""

    def __init__(self, cfg=None, state_dict=None, device="cpu"):
        self.device = torch.device(device)
        self.engine = _cfg_engine(cfg)
        self._graph, self._specs, self._plan_factory = self._configure(cfg)
        self._shapes = param_shapes(self._specs)
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
        self._built = True
        self._make_engine()
        return [k for k in state_dict if k.startswith(prefix) and k[len(prefix):] not in sd]    # ignored (dead keys)

    def _make_engine(self):
        if self.engine == "hip":
            self._hip = _HipEngine(self._convs, self.device, self._plan_factory)

    def to(self, device):
        self.device = torch.device(device)
        if self._built:
            for c in self._convs.values():
                c.weight, c.bias = c.weight.to(self.device), c.bias.to(self.device)
            self._make_engine()
        return self

    def eval(self):
        return self

    # -- forward ------------------------------------------------------------------------------------------------
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
        return run_graph(self._graph, self._convs, x)

    __call__ = forward


@BACKBONE.register_module()
class HRNet(_Backbone):
    """``HRNet(cfg)`` as the reference registers it (hrnet.py:444-454): levels of 40 / 80 / 160 / 320 channels"""

    def _configure(self, cfg):
        self.name = type(self).__name__
        return Graph(hrnet), _conv_specs(), HipPlan
