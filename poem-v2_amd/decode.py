"""The convolutional glue between the backbone's multi-level features and the head, MI355X-native:
``feat_decode`` / ``uv_decode`` / ``heatmap_stage`` of the reference model (lib/models/POEM.py:167-222 upstream) on the HIP
kernels of csrc/decode.hip -- the HRNet branch, and for the ResNet-18/34/50 pyramids the other one (POEM.py:59-86,168-181:
three [bilinear x2 | next finer level] -> ConvBlock stages, ``max_pool2d(2, 2)``, a 1x1 convolution; csrc/resnet.hip has the
last two in one launch).  No CPU fallback.

``FeatureDecoders`` holds what the reference model holds for this stage -- ``feat_delayer``, ``feat_in``,
``uv_delayer``, ``uv_out`` -- under the same state_dict key names, so a reference checkpoint's tensors load by key
(``load_reference_state_dict``; the unused ``uv_in`` and everything outside this stage are ignored).  Weights are packed
into MFMA fragment order once; conv bias and eval-mode BatchNorm fold into one per-channel affine applied in the conv
epilogue."""
import torch

from . import hip

FEAT_SIZE = (40, 80, 160, 320)
# channel counts of the four levels, finest first, by the backbone's ``.name`` (POEM.py:49-57)
FEAT_SIZES = {"HRNet": FEAT_SIZE, "resnet18": (64, 128, 256, 512), "resnet34": (64, 128, 256, 512),
              "resnet50": (256, 512, 1024, 2048)}
NUM_JOINTS = 21
BN_EPS = 1e-5


def _pad32(t):
    n = (t.numel() + 31) // 32 * 32
    out = torch.zeros(n, dtype=torch.float32, device=t.device)
    out[:t.numel()] = t
    return out


class _Conv3x3:
    def __init__(self, sd, name, device):
        w = sd[f"{name}.conv.weight"].to(device=device, dtype=torch.float32).contiguous()
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])
        nbytes = hip.lib().poem_conv3x3_packed_bytes(self.cout, self.cin)
        if nbytes == 0:
            raise RuntimeError(f"{name}: in_channels must be a multiple of 8")
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=device)
        hip.check(hip.lib().poem_pack_conv3x3(hip.ptr(w), self.cout, self.cin, self.packed.data_ptr(), hip.stream()),
                  "poem_pack_conv3x3")
        f64 = lambda k: sd[k].to(device=device, dtype=torch.float64)   # noqa: E731
        bias = f64(f"{name}.conv.bias")
        if f"{name}.norm.weight" in sd:
            inv = f64(f"{name}.norm.weight") / torch.sqrt(f64(f"{name}.norm.running_var") + BN_EPS)
            shift = (bias - f64(f"{name}.norm.running_mean")) * inv + f64(f"{name}.norm.bias")
        else:
            inv, shift = torch.ones_like(bias), bias
        self.scale, self.shift = _pad32(inv.float()), _pad32(shift.float())

    def __call__(self, x_padded, h, w, stride, out, out_strides, residual=None, relu=True):
        views = x_padded.shape[0]
        ns, cs, rs, off = out_strides
        hip.check(hip.lib().poem_conv3x3(hip.ptr(x_padded), self.packed.data_ptr(), hip.ptr(self.scale), hip.ptr(self.shift),
                                         hip.ptr(residual), hip.ptr(out), views, self.cin, self.cout, h, w, stride,
                                         int(relu), ns, cs, rs, off, hip.stream()), "poem_conv3x3")


def _conv_down2(self, x, h, w, out, out_strides, residual=None, relu=True):
    """stride-2 conv3x3 of the unbordered ``x`` in one LDS-staged launch (poem_conv3x3_down2); False when the shape is not taken."""
    ns, cs, rs, off = out_strides
    rc = hip.lib().poem_conv3x3_down2(hip.ptr(x), self.packed.data_ptr(), hip.ptr(self.scale), hip.ptr(self.shift),
                                      hip.ptr(residual), hip.ptr(out), x.shape[0], self.cin, self.cout, h, w, int(relu), ns, cs, rs,
                                      off, hip.stream())
    if rc == hip.POEM_E_UNSUPPORTED:
        return False
    hip.check(rc, "poem_conv3x3_down2")
    return True


def _conv_upcat(self, a, b, h, w, out, out_strides, relu=True):
    """conv3x3 of [bilinear x2 of a | b] in one launch (poem_upcat_conv3x3); False when the shape is not taken."""
    views = b.shape[0]
    ns, cs, rs, off = out_strides
    rc = hip.lib().poem_upcat_conv3x3(hip.ptr(a), int(a.shape[1]), hip.ptr(b), int(b.shape[1]), self.packed.data_ptr(),
                                      hip.ptr(self.scale), hip.ptr(self.shift), hip.ptr(out), views, self.cout, h, w, int(relu),
                                      ns, cs, rs, off, hip.stream())
    if rc == hip.POEM_E_UNSUPPORTED:
        return False
    hip.check(rc, "poem_upcat_conv3x3")
    return True


_Conv3x3.upcat = _conv_upcat
_Conv3x3.down2 = _conv_down2


K_SPLIT = 1024      # input channels per contraction of a _SplitConv3x3


class _SplitConv3x3:
    """A stage of the non-HRNet branch whose [bilinear x2 of a | b] input has more than K_SPLIT channels (ResNet-50's first two:
    3072 and 1536): the channels are contracted in groups of at most K_SPLIT -- first a's, then b's -- and the groups' sums are
    added in that order, each launch taking the sum so far as its residual; the last one adds the shift and applies the ReLU
    (poem_conv3x3_ex, residual before the activation).  One fixed-order fp32 chain over all 9 * 3072 = 27 648 products loses
    about twice the bits of three chains of 9216, and measured against fp64 it left the heat maps outside four times the CPU's
    fp32 round-off.  Still a fixed order: bit-reproducible, and a view's result does not depend on the others."""

    def __init__(self, sd, name, device, ca):
        w = sd[f"{name}.conv.weight"]
        self.cout, self.cin, self.ca = int(w.shape[0]), int(w.shape[1]), int(ca)
        spans = [(0, c0, min(c0 + K_SPLIT, self.ca)) for c0 in range(0, self.ca, K_SPLIT)]
        spans += [(1, c0, min(c0 + K_SPLIT, self.cin - self.ca)) for c0 in range(0, self.cin - self.ca, K_SPLIT)]
        self.groups = []
        for i, (src, c0, c1) in enumerate(spans):
            k0 = c0 + (self.ca if src else 0)
            conv = _Conv3x3(dict(sd, **{f"{name}.conv.weight": w[:, k0:k0 + c1 - c0]}), name, device)
            if i + 1 < len(spans):
                conv.shift = torch.zeros_like(conv.shift)        # the affine's offset is added once, by the last group
            self.groups.append((src, c0, c1, conv))

    def __call__(self, a, b, h, w, out):
        """a (views, ca, h/2, w/2), b (views, cin - ca, h, w) -> out (views, cout, h, w), all plain"""
        views, strides, part = b.shape[0], _plain_strides(self.cout, h, w), None
        for i, (src, c0, c1, conv) in enumerate(self.groups):
            t = b if src else a
            if (c0, c1) != (0, int(t.shape[1])):
                t = t[:, c0:c1].contiguous()
            xin = upsample2_concat_pad(None, t, h, w, 1) if src else upsample2_concat_pad(t, None, h, w, 1, staged=True)
            if i + 1 < len(self.groups):
                dst = torch.empty_like(out)
                conv(xin, h, w, 1, dst, strides, residual=part, relu=False)
            else:
                dst = out
                hip.check(hip.lib().poem_conv3x3_ex(hip.ptr(xin), conv.packed.data_ptr(), hip.ptr(conv.scale), hip.ptr(conv.shift),
                                                    hip.ptr(part), *strides, 1, hip.ptr(out), views, conv.cin, self.cout, h, w, 1, 1,
                                                    *strides, hip.stream()), "poem_conv3x3_ex")
            part = dst


def _padded_strides(c, h, w):
    """strides of an (n, c, h+2, w+2) zero-bordered tensor addressed by interior (y, x)."""
    return (c * (h + 2) * (w + 2), (h + 2) * (w + 2), w + 2, (w + 2) + 1)


def _plain_strides(c, h, w):
    return (c * h * w, h * w, w, 0)


def upsample2_concat_pad(a, b, h, w, pad, staged=False):
    """[bilinear x2 of a | b] with a zero border; a or b may be None.  ``staged`` (pad 1): the interpolation rounded as
    poem_upcat_conv3x3 rounds it, so that poem_conv3x3 of the result is that operator's, bit for bit (the non-HRNet branch)."""
    ref = a if a is not None else b
    views = ref.shape[0]
    ca = 0 if a is None else int(a.shape[1])
    cb = 0 if b is None else int(b.shape[1])
    out = torch.empty(views, ca + cb, h + 2 * pad, w + 2 * pad, dtype=torch.float32, device=ref.device)
    if staged:
        assert pad == 1
        hip.check(hip.lib().poem_upsample2_concat_pad_staged(hip.ptr(a), ca, hip.ptr(b), cb, hip.ptr(out), views, h, w, hip.stream()),
                  "poem_upsample2_concat_pad_staged")
        return out
    hip.check(hip.lib().poem_upsample2_concat_pad(hip.ptr(a), ca, hip.ptr(b), cb, hip.ptr(out), views, h, w, pad,
                                                  hip.stream()), "poem_upsample2_concat_pad")
    return out


class FeatureDecoders:
    """feat_decode / uv_decode / heatmap_stage of the reference model for the feature pyramid of ``backbone`` (its ``.name``:
    "HRNet" | "resnet18" | "resnet34" | "resnet50"); the state_dict keys are the same for every backbone."""

    def __init__(self, state_dict, device="cuda:0", backbone="HRNet"):
        if backbone not in FEAT_SIZES:
            raise ValueError(f"backbone {backbone!r}: expected one of {sorted(FEAT_SIZES)}")
        if not torch.cuda.is_available():
            raise RuntimeError("FeatureDecoders runs on the MI355X HIP path only (no CPU fallback)")
        self.device = torch.device(device)
        self.backbone, self.feat_size = backbone, FEAT_SIZES[backbone]
        self.fuse_upcat = [True, True, True]     # per uv_decode stage: poem_upcat_conv3x3 (one launch) vs upsample/concat + conv
        self.fuse_feat_in = True                 # feat_in + bilinear x2 in one launch (poem_conv1x1_upsample2)
        self.fuse_pool_head = True               # uv_decode's last stage + max-pool + uv_out + sigmoid in one launch
        sd = state_dict
        if backbone != "HRNet":
            self._check_weights(sd)                      # (before any packing: the groups below are cut by the table)

        def stage(name, i):
            f = self.feat_size
            if backbone != "HRNet" and f[3 - i] + f[2 - i] > K_SPLIT:
                return _SplitConv3x3(sd, f"{name}.{i}", self.device, ca=f[3 - i])
            return _Conv3x3(sd, f"{name}.{i}", self.device)

        with torch.cuda.device(self.device):
            self.feat_delayer = [stage("feat_delayer", i) for i in range(3)]
            self.uv_delayer = [stage("uv_delayer", i) for i in range(3)]
            w = sd["feat_in.conv.weight"].to(device=self.device, dtype=torch.float32)
            self.feat_in_w = hip.pack_linear(w.reshape(w.shape[0], w.shape[1]).contiguous())
            self.feat_in_b = sd["feat_in.conv.bias"].to(device=self.device, dtype=torch.float32).contiguous()
            self.feat_in_out = int(w.shape[0])
            w = sd["uv_out.conv.weight"].to(device=self.device, dtype=torch.float32)
            self.uv_out_w = w.reshape(w.shape[0], w.shape[1]).contiguous()
            self.uv_out_b = sd["uv_out.conv.bias"].to(device=self.device, dtype=torch.float32).contiguous()
            # poem_pool_conv1x1_sigmoid takes c <= 64 (raw weights); wider (ResNet-50's 256) goes to poem_maxpool2_conv1x1
            self.uv_out_packed = hip.pack_linear(self.uv_out_w) if self.uv_out_w.shape[1] > 64 else None

    def _check_weights(self, sd):
        """the decode stage's own channel counts against the selected (non-HRNet) table (POEM.py:59-86)"""
        f = self.feat_size
        stack = [(f[2 - i], f[3 - i] + f[2 - i]) for i in range(3)]
        names = [f"feat_delayer.{i}" for i in range(3)] + [f"uv_delayer.{i}" for i in range(3)] + ["feat_in", "uv_out"]
        got = [tuple(int(v) for v in sd[f"{n}.conv.weight"].shape[:2]) for n in names]
        want = stack + stack + [(f[1], f[0]), (NUM_JOINTS, f[0])]
        if got != want:
            raise ValueError(f"decode-stage weights (cout, cin) {got} are not the {self.backbone} table's {want}")

    @staticmethod
    def live_keys():
        keys = []
        for blk in [f"feat_delayer.{i}" for i in range(3)] + [f"uv_delayer.{i}" for i in range(3)]:
            keys += [f"{blk}.conv.weight", f"{blk}.conv.bias"] + [f"{blk}.norm.{n}" for n in
                                                                   ("weight", "bias", "running_mean", "running_var")]
        return keys + ["feat_in.conv.weight", "feat_in.conv.bias", "uv_out.conv.weight", "uv_out.conv.bias"]

    @classmethod
    def load_reference_state_dict(cls, state_dict, device="cuda:0", prefix="", backbone="HRNet"):
        """Pick this stage's tensors out of a full-model reference checkpoint (everything else is ignored)."""
        missing = [k for k in cls.live_keys() if prefix + k not in state_dict]
        if missing:
            raise KeyError(f"checkpoint lacks {missing[:4]}{'...' if len(missing) > 4 else ''}")
        return cls({k: state_dict[prefix + k] for k in cls.live_keys()}, device, backbone)

    def _check(self, mlvl_feats):
        if len(mlvl_feats) != 4:
            raise ValueError(f"expected the four {self.backbone} levels")
        out = []
        for f, c in zip(mlvl_feats, self.feat_size):
            if not f.is_cuda:
                raise RuntimeError("FeatureDecoders operates on device tensors only (no CPU path)")
            if f.shape[1] != c:
                raise ValueError(f"level with {f.shape[1]} channels, expected {c}")
            out.append(f.to(dtype=torch.float32).contiguous())
        return out

    def feat_decode(self, mlvl_feats, backbone="HRNet"):
        """(BN,40,64,64),(BN,80,32,32),(BN,160,16,16),(BN,320,8,8) -> mlvl_feat (BN,160,16,16)   [POEM.py:183-193]"""
        if backbone != self.backbone:
            raise ValueError(f"feat_decode for {backbone!r}: these decoders were built for {self.backbone!r}")
        f = self._check(mlvl_feats)
        if self.backbone != "HRNet":
            return self._resnet_feat_decode(f)
        views, r = f[0].shape[0], f[0].shape[-1]
        with torch.cuda.device(self.device):
            x, bordered = f[0], False
            for i, conv in enumerate(self.feat_delayer):
                ro = r // 2
                out = torch.empty(views, conv.cout, ro, ro, dtype=torch.float32, device=self.device)
                if bordered or not conv.down2(x, r, r, out, _plain_strides(conv.cout, ro, ro), residual=f[i + 1]):
                    # shapes the LDS-staged stride-2 kernel does not take: the direct kernel over zero-bordered tensors
                    if not bordered:
                        x = upsample2_concat_pad(None, x, r, r, 1)
                    if i == 2:
                        strides = _plain_strides(conv.cout, ro, ro)
                    else:                                                       # lands inside the next conv's input
                        out = torch.zeros(views, conv.cout, ro + 2, ro + 2, dtype=torch.float32, device=self.device)
                        strides = _padded_strides(conv.cout, ro, ro)
                    conv(x, r, r, 2, out, strides, residual=f[i + 1])
                    bordered = i < 2
                x, r = out, ro
            # feat_in is a 1x1 convolution: it commutes with the bilinear x2 in front of it (both linear, the interpolation
            # weights sum to one, so the bias passes through) -- applied at the low resolution it is a quarter of the FLOPs
            # and the (BN,320,16,16) intermediate never exists (POEM.py:190-193 upstream: interpolate, then feat_in)
            hw = r * r
            y = torch.empty(views, self.feat_in_out, 2 * r, 2 * r, dtype=torch.float32, device=self.device)
            rc = hip.lib().poem_conv1x1_upsample2(hip.ptr(x), self.feat_in_w.data_ptr(), hip.ptr(self.feat_in_b), hip.ptr(y),
                                                  views, int(x.shape[1]), self.feat_in_out, r, r, hip.stream()) \
                if self.fuse_feat_in else hip.POEM_E_UNSUPPORTED
            if rc == hip.POEM_E_UNSUPPORTED:                                     # other pyramid sizes: two launches
                y8 = torch.empty(views, self.feat_in_out, r, r, dtype=torch.float32, device=self.device)
                hip.check(hip.lib().poem_input_proj(hip.ptr(x), self.feat_in_w.data_ptr(), hip.ptr(self.feat_in_b), None, None,
                                                    hip.ptr(y8), views, int(x.shape[1]), self.feat_in_out, hw, hip.stream()),
                          "poem_input_proj")
                y = upsample2_concat_pad(y8, None, 2 * r, 2 * r, 0)              # (BN,160,16,16)
            else:
                hip.check(rc, "poem_conv1x1_upsample2")
        return y

    # -- the non-HRNet branch (POEM.py:168-181, 197-206) --------------------------------------------------------------
    def _up_stages(self, convs, f):
        """three times [bilinear x2 of x | next finer level] -> conv3x3 + BN + ReLU, from the coarsest level; any h x w"""
        rev = list(reversed(f))
        x, views = rev[0], f[0].shape[0]
        h, w = int(x.shape[-2]), int(x.shape[-1])
        for i, conv in enumerate(convs):
            h, w = 2 * h, 2 * w
            if tuple(rev[i + 1].shape[-2:]) != (h, w):
                raise ValueError(f"level of {tuple(rev[i + 1].shape[-2:])}, expected {(h, w)} (twice the coarser one)")
            y = torch.empty(views, conv.cout, h, w, dtype=torch.float32, device=self.device)
            if isinstance(conv, _SplitConv3x3):
                conv(x, rev[i + 1], h, w, y)
            elif not (self.fuse_upcat[i] and conv.upcat(x, rev[i + 1], h, w, y, _plain_strides(conv.cout, h, w))):
                conv(upsample2_concat_pad(x, rev[i + 1], h, w, 1, staged=True), h, w, 1, y, _plain_strides(conv.cout, h, w))
            x = y
        return x

    def _pool_conv1x1(self, x, w_packed, bias, cout, act):
        views, cin, h, w = (int(v) for v in x.shape)
        y = torch.empty(views, cout, h // 2, w // 2, dtype=torch.float32, device=self.device)
        hip.check(hip.lib().poem_maxpool2_conv1x1(hip.ptr(x), w_packed.data_ptr(), hip.ptr(bias), hip.ptr(y), views, cin, cout, h, w,
                                                  act, hip.stream()), "poem_maxpool2_conv1x1")
        return y

    def _resnet_feat_decode(self, f):
        """(BN,64,64,64) .. (BN,512,8,8) -> mlvl_feat (BN,128,32,32); four times the channels for ResNet-50   [POEM.py:168-181]"""
        with torch.cuda.device(self.device):
            x = self._up_stages(self.feat_delayer, f)
            return self._pool_conv1x1(x, self.feat_in_w, self.feat_in_b, self.feat_in_out, 0)

    def _resnet_uv_decode(self, f):
        with torch.cuda.device(self.device):
            x = self._up_stages(self.uv_delayer, f)
            if self.uv_out_packed is not None:
                return self._pool_conv1x1(x, self.uv_out_packed, self.uv_out_b, NUM_JOINTS, 1)
            views, c, h, w = (int(v) for v in x.shape)
            hm = torch.empty(views, NUM_JOINTS, h // 2, w // 2, dtype=torch.float32, device=self.device)
            hip.check(hip.lib().poem_pool_conv1x1_sigmoid(hip.ptr(x), hip.ptr(self.uv_out_w), hip.ptr(self.uv_out_b), hip.ptr(hm),
                                                          views, c, NUM_JOINTS, h, w, hip.stream()), "poem_pool_conv1x1_sigmoid")
        return hm

    def uv_decode(self, mlvl_feats):
        """-> uv_hmap (BN,21,32,32)   [POEM.py:197-207; the unused uv_feat of :208 is not computed]"""
        f = self._check(mlvl_feats)
        if self.backbone != "HRNet":
            return self._resnet_uv_decode(f)
        rev = list(reversed(f))
        views = f[0].shape[0]
        with torch.cuda.device(self.device):
            x, r = rev[0], rev[0].shape[-1]
            for i, conv in enumerate(self.uv_delayer):
                r *= 2
                if i == 2 and self.fuse_pool_head and self.fuse_upcat[i]:
                    # the last stage and the read-out head in one launch: its (BN,40,64,64) output is read by nothing else
                    hm = torch.empty(views, NUM_JOINTS, r // 2, r // 2, dtype=torch.float32, device=self.device)
                    rc = hip.lib().poem_upcat_conv3x3_pool_head(
                        hip.ptr(x), int(x.shape[1]), hip.ptr(rev[i + 1]), int(rev[i + 1].shape[1]), conv.packed.data_ptr(),
                        hip.ptr(conv.scale), hip.ptr(conv.shift), hip.ptr(self.uv_out_w), hip.ptr(self.uv_out_b), hip.ptr(hm), views,
                        conv.cout, NUM_JOINTS, r, r, 1, hip.stream())
                    if rc != hip.POEM_E_UNSUPPORTED:
                        hip.check(rc, "poem_upcat_conv3x3_pool_head")
                        return hm
                y = torch.empty(views, conv.cout, r, r, dtype=torch.float32, device=self.device)
                if not (self.fuse_upcat[i] and conv.upcat(x, rev[i + 1], r, r, y, _plain_strides(conv.cout, r, r))):   # one launch where it pays
                    conv(upsample2_concat_pad(x, rev[i + 1], r, r, 1), r, r, 1, y, _plain_strides(conv.cout, r, r))
                x = y
            hm = torch.empty(views, NUM_JOINTS, r // 2, r // 2, dtype=torch.float32, device=self.device)
            hip.check(hip.lib().poem_pool_conv1x1_sigmoid(hip.ptr(x), hip.ptr(self.uv_out_w), hip.ptr(self.uv_out_b),
                                                          hip.ptr(hm), views, int(x.shape[1]), NUM_JOINTS, r, r,
                                                          hip.stream()), "poem_pool_conv1x1_sigmoid")
        return hm

    def heatmap_stage(self, img_feats, W, H, return_conf=False):
        """-> uv_coord_im (BN,21,2) pixels   [POEM.py:213-222]; ``return_conf``: also the (BN,21) heat-map peaks.  Whichever
        route ``uv_decode`` took (read-out head fused into its last convolution, or two launches), the maps it returns
        are the same bits, and the confidence is read from them by the launch that reads the expectation."""
        from .triangulation import heatmap_to_uv
        return heatmap_to_uv(self.uv_decode(img_feats), W, H, return_conf=return_conf)
