"""HRNet-W40 feature pyramid, on one of two engines (``cfg.ENGINE``):

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

Written as a flat list of folded convolutions instead of an nn.Module tree: every eval-mode BatchNorm is folded into
the convolution in front of it once at load time (fp64), so a forward is conv (+bias) -> [add] -> [ReLU] calls only.
The torch engine runs on whatever device its tensors live on (CPU for the parity test, MIOpen on the GPU).

The hip engine (``HipPlan`` + ``_HipEngine`` below).  ``HipPlan(views, H, W)`` is the forward written out once, without a
device: the list of launches in ``_conv_specs`` order and the buffers they read and write.  Every activation a 3x3
convolution reads is the interior of a zero-bordered buffer; buffers are pooled by geometry -- a buffer keeps the shape it was
planned with, and a plan belongs to one (views, H, W) -- allocated zeroed once, and only interiors are ever written, so the
borders stay zero.  The four returned levels are fresh tensors of every call.  All launches go to the current stream with no
host wait in between; they are about 300 (``len(plan.ops)``) and are NOT captured into a graph, so at a handful of views the
forward is bound by launch overhead.  Inputs: H and W multiples of 32 with (H/32)*(W/32) a multiple of 32 (256x256, 128x256,
512x512; not 64x64 or 224x224): ``ValueError`` otherwise.  Memory: ``plan.nbytes()`` -- 6.7 GiB of activations at 256 views of
256x256 (26.9 MiB per view), kept for as long as the HRNet object lives, once per distinct (views, H, W) it has seen."""
import torch
import torch.nn.functional as F

from .builder import BACKBONE

ENGINES = ("torch", "hip")
BN_EPS = 1e-5
WIDTHS = (40, 80, 160, 320)                     # cls_hrnet_w40 NUM_CHANNELS of stage 4
STAGES = ((2, 1), (3, 4), (4, 3))               # (branches, modules) of stages 2..4; 4 BasicBlocks per branch
BLOCKS_PER_BRANCH = 4


def _conv_specs(widths=WIDTHS):
    """(conv key, bn key, cout, cin, kernel, stride) of every live conv -> BatchNorm pair, in the reference's key names."""
    specs = []

    def conv_bn(conv, bn, cout, cin, k, stride=1):
        specs.append((conv, bn, cout, cin, k, stride))

    conv_bn("conv1", "bn1", 64, 3, 3, 2)
    conv_bn("conv2", "bn2", 64, 64, 3, 2)
    cin = 64
    for i in range(4):                                             # layer1: Bottleneck x4, planes 64, expansion 4
        p = f"layer1.{i}"
        conv_bn(f"{p}.conv1", f"{p}.bn1", 64, cin, 1)
        conv_bn(f"{p}.conv2", f"{p}.bn2", 64, 64, 3)
        conv_bn(f"{p}.conv3", f"{p}.bn3", 256, 64, 1)
        if i == 0:
            conv_bn(f"{p}.downsample.0", f"{p}.downsample.1", 256, cin, 1)
        cin = 256
    pre = [256]
    for s, (nb, nm) in enumerate(STAGES, start=1):
        cur = list(widths[:nb])
        for i in range(nb):                                        # transition s (hrnet.py:319-344)
            if i < len(pre):
                if cur[i] != pre[i]:
                    conv_bn(f"transition{s}.{i}.0", f"transition{s}.{i}.1", cur[i], pre[i], 3)
            else:
                for j in range(i + 1 - len(pre)):
                    cout = cur[i] if j == i - len(pre) else pre[-1]
                    conv_bn(f"transition{s}.{i}.{j}.0", f"transition{s}.{i}.{j}.1", cout, pre[-1], 3, 2)
        for m in range(nm):
            p = f"stage{s + 1}.{m}"
            for b in range(nb):
                for k in range(BLOCKS_PER_BRANCH):
                    q = f"{p}.branches.{b}.{k}"
                    conv_bn(f"{q}.conv1", f"{q}.bn1", cur[b], cur[b], 3)
                    conv_bn(f"{q}.conv2", f"{q}.bn2", cur[b], cur[b], 3)
            for i in range(nb):                                    # fuse layers (hrnet.py:177-212)
                for j in range(nb):
                    if j > i:
                        conv_bn(f"{p}.fuse_layers.{i}.{j}.0", f"{p}.fuse_layers.{i}.{j}.1", cur[i], cur[j], 1)
                    elif j < i:
                        for k in range(i - j):
                            cout = cur[i] if k == i - j - 1 else cur[j]
                            conv_bn(f"{p}.fuse_layers.{i}.{j}.{k}.0", f"{p}.fuse_layers.{i}.{j}.{k}.1", cout, cur[j], 3, 2)
        pre = cur
    return specs


def hrnet_param_shapes(widths=WIDTHS):
    """name -> shape of every live tensor (conv weights + BatchNorm affine / statistics)."""
    shapes = {}
    for conv, bn, cout, cin, k, _ in _conv_specs(widths):
        shapes[f"{conv}.weight"] = (cout, cin, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{bn}.{n}"] = (cout,)
    return shapes


def seeded_hrnet_state_dict(seed=0, widths=WIDTHS):
    """Seeded weights with non-trivial BatchNorm statistics; the second conv of every residual block is small so that
    activations stay O(1) through the ~100 layers without trained statistics."""
    g = torch.Generator().manual_seed(7000 + seed)
    sd = {}
    for name, shape in hrnet_param_shapes(widths).items():
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
            gain = 1.0
            if (".conv2.weight" in name and "branches" in name) or ".conv3.weight" in name:
                gain = 0.3
            elif "fuse_layers" in name:
                gain = 0.45
            sd[name] = torch.randn(shape, generator=g) * (gain * (1.6 / fan_in) ** 0.5)
    return sd


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


# ---- the "hip" engine -----------------------------------------------------------------------------------------------------
def _cfg_engine(cfg):
    """``cfg.ENGINE`` of the BACKBONE node (a dict / CN, an object with attributes, or None)."""
    if cfg is None:
        return "torch"
    eng = cfg.get("ENGINE", "torch") if hasattr(cfg, "get") else getattr(cfg, "ENGINE", "torch")
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


class HipPlan:
    """The hip engine's forward for one (views, H, W), device-free: ``ops`` (dicts: kind "input" | "conv3" | "down2" | "conv1" |
    "fuse"; ``conv`` = the _conv_specs key; ``in`` / ``out`` / ``res`` = _Map; fuse: ``terms`` = [(_Map, shift)]) in launch
    order, ``buffers`` (geometry of buffer id) and ``outputs`` (the four levels)."""
    STEM_CIN = 8          # conv1's 3 input channels zero-padded to one 8-channel chunk

    def __init__(self, views, H, W, widths=WIDTHS):
        check_hip_input(H, W)
        self.views, self.H, self.W, self.widths = int(views), int(H), int(W), tuple(widths)
        self.buffers, self.ops, self._free, self._nmaps = [], [], {}, 0
        self._build()

    # -- buffers ----------------------------------------------------------------------------------------------------
    def _new(self, c, h, w, bordered=True):
        free = self._free.setdefault((c, h, w, bordered), [])
        if free:
            buf = free.pop()
        else:
            buf = len(self.buffers)
            self.buffers.append((c, h, w, bordered))
        self._nmaps += 1
        return _Map(self._nmaps, buf, c, h, w, bordered)

    def _release(self, m):
        if m.buf >= 0:
            self._free[m.geometry].append(m.buf)

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
    def _conv3(self, name, x, cout, stride, relu, res=None, bordered_out=True, out=None):
        if out is None:
            out = self._new(cout, x.h // stride, x.w // stride, bordered_out)
        kind = "conv3"
        if not x.bordered:                                   # a plain map feeds the LDS-staged stride-2 kernel only
            if stride != 2 or res is not None or not _down2_takes(cout, x.h, x.w):
                raise AssertionError(f"{name}: a plain input needs a shape poem_conv3x3_down2 takes")
            kind = "down2"
        self.ops.append({"kind": kind, "conv": name, "in": x, "out": out, "res": res, "stride": stride, "relu": relu})
        return out

    def _conv1(self, name, x, cout, relu, res=None, bordered_out=True):
        out = self._new(cout, x.h, x.w, bordered_out)
        self.ops.append({"kind": "conv1", "conv": name, "in": x, "out": out, "res": res, "stride": 1, "relu": relu})
        return out

    def _build(self):
        x = self._new(self.STEM_CIN, self.H, self.W)
        self.ops.append({"kind": "input", "out": x})
        a = self._conv3("conv1", x, 64, 2, True)
        self._release(x)
        x = self._conv3("conv2", a, 64, 2, True, bordered_out=False)
        self._release(a)
        for i in range(4):                                                # layer1 (Bottleneck: hrnet.py Bottleneck.forward)
            p = f"layer1.{i}"
            t1 = self._conv1(f"{p}.conv1", x, 64, True)
            t2 = self._conv3(f"{p}.conv2", t1, 64, 1, True, bordered_out=False)
            self._release(t1)
            r = self._conv1(f"{p}.downsample.0", x, 256, False, bordered_out=False) if i == 0 else x
            y = self._conv1(f"{p}.conv3", t2, 256, True, res=r, bordered_out=(i == 3))
            self._release(t2)
            if r is not x:
                self._release(r)
            self._release(x)
            x = y
        ys, pre = [x], [256]
        for s, (nb, nm) in enumerate(STAGES, start=1):
            cur = list(self.widths[:nb])
            ys = self._transition(s, ys, pre, cur)
            for m in range(nm):
                ys = self._module(f"stage{s + 1}.{m}", ys, final=(s == len(STAGES) and m == nm - 1))
            pre = cur
        self.outputs = ys

    def _transition(self, s, ys, pre, cur):
        out = []
        for i in range(len(cur)):
            if i < len(ys):
                if cur[i] != pre[i]:
                    out.append(self._conv3(f"transition{s}.{i}.0", ys[-1], cur[i], 1, True))    # hrnet.py:397-410: ys[-1], as upstream
                else:
                    out.append(ys[i])
            else:
                t = ys[-1]
                for j in range(i + 1 - len(ys)):
                    cout = cur[i] if j == i - len(ys) else pre[-1]
                    t2 = self._conv3(f"transition{s}.{i}.{j}.0", t, cout, 2, True)
                    if t is not ys[-1]:
                        self._release(t)
                    t = t2
                out.append(t)
        for y in ys:
            if not any(y is o for o in out):
                self._release(y)
        return out

    def _module(self, p, xs, final):
        nb, xs = len(xs), list(xs)
        for b in range(nb):
            for k in range(BLOCKS_PER_BRANCH):                            # BasicBlock: relu(conv2(relu(conv1(x))) + x)
                q, x = f"{p}.branches.{b}.{k}", xs[b]
                t = self._conv3(f"{q}.conv1", x, x.c, 1, True)
                y = self._conv3(f"{q}.conv2", t, x.c, 1, True, res=x)
                self._release(t)
                self._release(x)
                xs[b] = y
        fused = []
        for i in range(nb):                                               # hrnet.py:226-233: y = ((t0 + t1) + t2) + t3
            terms, temps = [], []
            for j in range(nb):
                if j == i:
                    terms.append((xs[j], 0))
                elif j > i:                                               # 1x1 at the low resolution; nearest upsampling in the sum
                    t = self._conv1(f"{p}.fuse_layers.{i}.{j}.0", xs[j], xs[i].c, False, bordered_out=False)
                    temps.append(t)
                    terms.append((t, j - i))
                else:
                    t = xs[j]
                    for k in range(i - j):
                        last = k == i - j - 1
                        cout = xs[i].c if last else xs[j].c
                        nxt = xs[i].c if k + 1 == i - j - 1 else xs[j].c
                        plain = last or _down2_takes(nxt, t.h // 2, t.w // 2)   # what the next launch reads
                        t2 = self._conv3(f"{p}.fuse_layers.{i}.{j}.{k}.0", t, cout, 2, not last, bordered_out=not plain)
                        if t is not xs[j]:
                            self._release(t)
                        t = t2
                    temps.append(t)
                    terms.append((t, 0))
            x = xs[i]
            if final:
                self._nmaps += 1
                out = _Map(self._nmaps, -(i + 1), x.c, x.h, x.w, False)
            else:
                out = self._new(x.c, x.h, x.w, True)
            self.ops.append({"kind": "fuse", "terms": terms, "out": out})
            for t in temps:
                self._release(t)
            fused.append(out)
        for x in xs:
            self._release(x)
        return fused


def stem_weight(w):
    """conv1's folded (64, 3, 3, 3) weight with the input channels zero-padded to HipPlan.STEM_CIN"""
    out = torch.zeros(w.shape[0], HipPlan.STEM_CIN, 3, 3, dtype=w.dtype, device=w.device)
    out[:, :w.shape[1]] = w
    return out


class _HipEngine:
    """The folded convolutions packed once for the kernels, and the buffers of every plan run so far."""

    def __init__(self, convs, device):
        from . import hip
        from .decode import _pad32
        self.hip, self.device, self._pad32 = hip, torch.device(device), _pad32
        self.w = {}                                      # conv key -> (packed weights, scale | None, shift, cin, cout)
        for name, c in convs.items():
            self.w[name] = self._pack(name, c.weight.to(self.device), c.bias.to(self.device))
        self._plans = {}

    def _pack(self, name, w, bias):
        hip, L = self.hip, self.hip.lib()
        if name == "conv1":
            w = stem_weight(w)
        cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        w = w.contiguous()
        if k == 3:
            packed = torch.empty(L.poem_conv3x3_packed_bytes(cout, cin), dtype=torch.uint8, device=self.device)
            hip.check(L.poem_pack_conv3x3(hip.ptr(w), cout, cin, packed.data_ptr(), hip.stream()), "poem_pack_conv3x3")
            return (packed, self._pad32(torch.ones_like(bias)), self._pad32(bias), cin, cout)   # the scale is in the weight
        packed = torch.empty(L.poem_conv1x1_packed_bytes(cout, cin), dtype=torch.uint8, device=self.device)
        hip.check(L.poem_pack_conv1x1(hip.ptr(w), cout, cin, packed.data_ptr(), hip.stream()), "poem_pack_conv1x1")
        return (packed, None, bias.contiguous(), cin, cout)

    def _make_plan(self, views, H, W):
        return HipPlan(views, H, W)

    def plan(self, views, H, W):
        key = (views, H, W)
        if key not in self._plans:
            plan = self._make_plan(views, H, W)
            bufs = [torch.zeros(plan.buffer_shape(b), dtype=torch.float32, device=self.device) for b in range(len(plan.buffers))]
            self._plans[key] = (plan, bufs, self._bind(plan, bufs))
        return self._plans[key]

    def _bind(self, plan, bufs):
        """plan.ops as (function, arguments) with every pointer resolved; a returned level's pointer is filled per forward."""
        hip, L, views = self.hip, self.hip.lib(), plan.views
        ptr = lambda m: bufs[m.buf].data_ptr() if m.buf >= 0 else None      # noqa: E731
        calls = []
        for op in plan.ops:
            kind, out = op["kind"], op["out"]
            if kind == "input":
                calls.append(("input", bufs[out.buf][:, :3, 1:-1, 1:-1]))
                continue
            if kind == "fuse":
                terms = (hip.PoemFuseTerm * len(op["terms"]))()
                for t, (m, shift) in zip(terms, op["terms"]):
                    ns, cs, rs, off = m.strides
                    t.data, t.view_stride, t.ch_stride, t.row_stride, t.offset, t.shift = ptr(m), ns, cs, rs, off, shift
                calls.append(("poem_hrnet_fuse", L.poem_hrnet_fuse, out.buf, [terms, len(terms), ptr(out), *out.strides, views, out.c, out.h, out.w]))
                continue
            calls.append(self._conv_call(op, ptr, views))
        return calls

    def _conv_call(self, op, ptr, views):
        """one "conv3" | "down2" | "conv1" op as (name, function, output buffer, arguments)"""
        L, kind, out = self.hip.lib(), op["kind"], op["out"]
        packed, scale, shift, cin, cout = self.w[op["conv"]]
        x, res = op["in"], op["res"]
        assert (cin, cout) == (x.c, out.c), op["conv"]
        rptr, rstr = (ptr(res), res.strides) if res is not None else (None, (0, 0, 0, 0))
        if kind == "conv3":
            args = [ptr(x), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), rptr, *rstr, 1, ptr(out), views, cin, cout,
                    x.h, x.w, op["stride"], int(op["relu"]), *out.strides]
            return ("poem_conv3x3_ex", L.poem_conv3x3_ex, out.buf, args)
        if kind == "down2":
            args = [ptr(x), packed.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, ptr(out), views, cin, cout, x.h, x.w,
                    int(op["relu"]), *out.strides]
            return ("poem_conv3x3_down2", L.poem_conv3x3_down2, out.buf, args)
        args = [ptr(x), *x.strides, packed.data_ptr(), shift.data_ptr(), rptr, *rstr, ptr(out), *out.strides, views, cin, cout,
                x.h, x.w, int(op["relu"])]
        return ("poem_conv1x1", L.poem_conv1x1, out.buf, args)

    def forward(self, x):
        views, H, W = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
        plan, _, calls = self.plan(views, H, W)
        outs = [torch.empty(views, m.c, m.h, m.w, dtype=torch.float32, device=self.device) for m in plan.outputs]
        stream, check = self.hip.stream(), self.hip.check
        for call in calls:
            if call[0] == "input":
                call[1].copy_(x)
                continue
            what, fn, buf, args = call
            if buf < 0:                                   # a returned level: poem_hrnet_fuse's `out` is its third argument
                args = list(args)
                args[2] = outs[-(buf + 1)].data_ptr()
            check(fn(*args, stream), what)
        return outs


@BACKBONE.register_module()
class HRNet:
    """``HRNet(cfg)`` as the reference registers it (hrnet.py:444-454); weights arrive through ``load_state_dict``."""

    def __init__(self, cfg=None, state_dict=None, device="cpu"):
        self.name = type(self).__name__
        self.device = torch.device(device)
        self.engine = _cfg_engine(cfg)
        self._hip = None
        self._sd_keys = list(hrnet_param_shapes())
        self._built = False
        if state_dict is not None:
            self.load_state_dict(state_dict)

    # -- weights ------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, prefix="", strict=False):
        missing = [k for k in self._sd_keys if prefix + k not in state_dict]
        if missing:
            raise KeyError(f"HRNet checkpoint lacks {missing[:4]}{'...' if len(missing) > 4 else ''}")
        sd = {k: state_dict[prefix + k].detach().cpu() for k in self._sd_keys}
        for k, shape in hrnet_param_shapes().items():
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)}, expected {shape}")
        self._fold(sd)
        return [k for k in state_dict if k.startswith(prefix) and k[len(prefix):] not in sd]    # ignored (dead head)

    def to(self, device):
        self.device = torch.device(device)
        if self._built:
            for c in self._convs.values():
                c.weight, c.bias = c.weight.to(self.device), c.bias.to(self.device)
            if self.engine == "hip":
                self._hip = _HipEngine(self._convs, self.device)
        return self

    def eval(self):
        return self

    def _fold(self, sd):
        self._convs = {conv: _FoldedConv(sd, conv, bn, stride, self.device) for conv, bn, _, _, _, stride in _conv_specs()}
        if self.engine == "hip":
            self._hip = _HipEngine(self._convs, self.device)
        self._built = True

    # -- forward ------------------------------------------------------------------------------------------------
    def _basic(self, p, x):
        c = self._convs
        out = c[f"{p}.conv1"](x, relu=True)
        out = c[f"{p}.conv2"](out)
        return F.relu_(out.add_(x))

    def _bottleneck(self, p, x):
        c = self._convs
        out = c[f"{p}.conv1"](x, relu=True)
        out = c[f"{p}.conv2"](out, relu=True)
        out = c[f"{p}.conv3"](out)
        res = c[f"{p}.downsample.0"](x) if f"{p}.downsample.0" in c else x
        return F.relu_(out.add_(res))

    def _module(self, p, xs):
        c, nb = self._convs, len(xs)
        xs = list(xs)
        for b in range(nb):
            for k in range(BLOCKS_PER_BRANCH):
                xs[b] = self._basic(f"{p}.branches.{b}.{k}", xs[b])
        fused = []
        for i in range(nb):                                              # hrnet.py:226-233: y = ((t0 + t1) + t2) + t3
            y = None
            for j in range(nb):
                if j == i:
                    t = xs[j]
                elif j > i:
                    t = F.interpolate(c[f"{p}.fuse_layers.{i}.{j}.0"](xs[j]), scale_factor=2 ** (j - i), mode="nearest")
                else:
                    t = xs[j]
                    for k in range(i - j):
                        t = c[f"{p}.fuse_layers.{i}.{j}.{k}.0"](t, relu=k != i - j - 1)
                y = t if y is None else y + t
            fused.append(F.relu(y))
        return fused

    def _transition(self, s, ys, nb):
        c, out = self._convs, []
        for i in range(nb):
            if i < len(ys):
                name = f"transition{s}.{i}.0"
                out.append(c[name](ys[-1], relu=True) if name in c else ys[i])      # hrnet.py:397-410: ys[-1], as upstream
            else:
                t = ys[-1]
                for j in range(i + 1 - len(ys)):
                    t = c[f"transition{s}.{i}.{j}.0"](t, relu=True)
                out.append(t)
        return out

    @torch.no_grad()
    def forward(self, x):
        """x (BN,3,H,W) -> [(BN,40,H/4,W/4), (BN,80,H/8,W/8), (BN,160,H/16,W/16), (BN,320,H/32,W/32)]"""
        if self.engine == "hip":
            check_hip_input(int(x.shape[-2]), int(x.shape[-1]))
        if not self._built:
            raise RuntimeError("HRNet has no weights: call load_state_dict first")
        if self.engine == "hip":
            return self._hip.forward(x.to(device=self.device, dtype=torch.float32))
        c = self._convs
        x = x.to(device=self.device, dtype=torch.float32)
        x = c["conv1"](x, relu=True)
        x = c["conv2"](x, relu=True)
        for i in range(4):
            x = self._bottleneck(f"layer1.{i}", x)
        ys = [x]
        for s, (nb, nm) in enumerate(STAGES, start=1):
            ys = self._transition(s, ys, nb)
            for m in range(nm):
                ys = self._module(f"stage{s + 1}.{m}", ys)
        return ys

    __call__ = forward
