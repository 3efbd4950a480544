"""The ResNet-18/34/50 backbones on the device: the four operators of csrc/resnet.hip through the C ABI, the whole backbone on
its hip engine, the non-HRNet branch of FeatureDecoders and the model-level caller with ``BACKBONE.TYPE = ResNet34``.

Yardstick: the CPU torch path in fp64, and in fp32 for the error scale (the torch engine is itself pinned to the reference's
ResNets by tests/golden/resnet.npz, the decode restatement by resnet_decode.npz).  Criterion (tests/test_backbone_hip.py's),
max norm per output tensor:

    max|HIP - fp64| <= 4 * max|fp32_cpu - fp64| + 1e-6 * max|fp64|

plus exact equality on small-integer data, sentinel-filled bordered outputs (no store outside the interior), junk-filled input
borders, and bit equality wherever the code promises it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import poem_oracle as po
import poem_v2_amd as pk
import resnet_util as ru
from poem_v2_amd import hip
from poem_v2_amd import resnet as rn
from resnet_util import criterion as _criterion
from test_backbone_hip import DEV, SENTINEL, _border_is, _buffer, _pack1, _plain

pytestmark = pytest.mark.gpu


def _bits_equal(got, ref):
    """the same NaN mask and, elsewhere, the same bits (-0 and +0 differ)"""
    got, ref = got.cpu(), ref.cpu()
    return torch.equal(got.isnan(), ref.isnan()) and \
        torch.equal(torch.nan_to_num(got, nan=1.0).view(torch.int32), torch.nan_to_num(ref, nan=1.0).view(torch.int32))


# ---- poem_conv7x7_s2 ----------------------------------------------------------------------------------------------------
class _Stem:
    def __init__(self, w, scale, shift):
        L = hip.lib()
        self.cout = int(w.shape[0])
        self.w = w.to(DEV).contiguous()
        self.packed = torch.empty(L.poem_conv7x7_packed_bytes(self.cout), dtype=torch.uint8, device=DEV)
        hip.check(L.poem_pack_conv7x7(hip.ptr(self.w), self.cout, self.packed.data_ptr(), hip.stream()), "poem_pack_conv7x7")
        self.scale, self.shift = scale.to(DEV).contiguous(), shift.to(DEV).contiguous()

    def __call__(self, x, out, out_strides, h=None, w=None, cout=None):
        return hip.lib().poem_conv7x7_s2(x.data_ptr(), self.packed.data_ptr(), hip.ptr(self.scale), hip.ptr(self.shift), out.data_ptr(),
                                         *out_strides, x.shape[0], cout or self.cout, h or x.shape[-2], w or x.shape[-1], hip.stream())


def _stem_ref(x, w, scale, shift, dtype):
    y = F.conv2d(x.to(dtype), w.to(dtype), stride=2, padding=3)
    return F.relu(y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1))


@pytest.mark.parametrize("h,w", [pytest.param(16, 32, id="16x32-all-halos-in-one-tile"), pytest.param(64, 128, id="64x128-row-tiles")])
@pytest.mark.parametrize("cout", [64, 32])
def test_conv7x7_s2(h, w, cout):
    views, ho, wo = 3, h // 2, w // 2
    g = torch.Generator().manual_seed(7 * h + cout)
    x = torch.randn(views, 3, h, w, generator=g)
    wt = torch.randn(cout, 3, 7, 7, generator=g) * (1.6 / 147) ** 0.5
    scale, shift = 1 + 0.2 * (2 * torch.rand(cout, generator=g) - 1), 0.3 * torch.randn(cout, generator=g)
    stem, xd = _Stem(wt, scale, shift), x.to(DEV)
    ref64, ref32 = _stem_ref(x, wt, scale, shift, torch.float64), _stem_ref(x, wt, scale, shift, torch.float32)
    outs = {}
    for out_b in (True, False):
        ob, oint, os_ = _buffer(torch.zeros(views, cout, ho, wo), out_b, SENTINEL, g)
        assert stem(xd, ob, os_) == 0
        _criterion(oint, ref64, ref32, f"conv7x7_s2 3->{cout} {h}x{w} out_b={out_b}")
        assert not out_b or _border_is(ob, SENTINEL), "a store outside the interior"
        outs[out_b] = oint.clone()
    assert torch.equal(outs[True], outs[False])
    # views are independent: the first two views of the 3-view launch are the 2-view launch, bit for bit
    o2 = torch.empty(2, cout, ho, wo, device=DEV)
    assert stem(xd[:2].contiguous(), o2, _plain(cout, ho, wo)) == 0
    assert torch.equal(o2, outs[False][:2])
    # small integers: exact
    xi = torch.randint(-3, 4, (views, 3, h, w), generator=g).float()
    wi = torch.randint(-2, 3, (cout, 3, 7, 7), generator=g).float()
    si = torch.randint(-5, 6, (cout,), generator=g).float()
    ob, oint, os_ = _buffer(torch.zeros(views, cout, ho, wo), True, SENTINEL, g)
    assert _Stem(wi, torch.ones(cout), si)(xi.to(DEV), ob, os_) == 0
    assert torch.equal(oint.cpu().double(), _stem_ref(xi, wi, torch.ones(cout), si, torch.float64)) and _border_is(ob, SENTINEL)
    # one NaN pixel (next to a corner, so that padded windows hold it too): torch's NaN mask
    xn = x.clone()
    xn[1, 2, 1, w - 2] = float("nan")
    on = torch.empty(views, cout, ho, wo, device=DEV)
    assert stem(xn.to(DEV), on, _plain(cout, ho, wo)) == 0
    refn = _stem_ref(xn, wt, scale, shift, torch.float32)
    assert bool(refn.isnan().any()) and torch.equal(on.cpu().isnan(), refn.isnan())


def test_conv7x7_s2_refusals():
    stem = _Stem(torch.zeros(64, 3, 7, 7), torch.ones(64), torch.zeros(64))
    x = torch.zeros(1, 3, 16, 32, device=DEV)
    out = torch.full((1, 64, 8, 16), SENTINEL, device=DEV)
    ps, L = _plain(64, 8, 16), hip.lib()
    assert stem(x, out, _plain(64, 7, 16), h=15) == hip.POEM_E_UNSUPPORTED                       # odd height
    assert stem(x, out, _plain(64, 8, 15), w=31) == hip.POEM_E_UNSUPPORTED                       # odd width
    assert stem(x, out, _plain(64, 8, 10), w=20) == hip.POEM_E_UNSUPPORTED                       # 80 output pixels
    assert stem(x, out, _plain(40, 8, 16), cout=40) == hip.POEM_E_UNSUPPORTED                    # cout % 32
    assert stem(x, out, (64 * 128, 128, 16, 1)) == -1                                            # leaves its plane
    assert stem(x, out, (64 * 128, 128, 15, 0)) == -1                                            # rows overlap
    assert L.poem_conv7x7_s2(None, None, None, None, None, *ps, 1, 64, 16, 32, None) == -1
    assert L.poem_conv7x7_packed_bytes(0) == 0 and L.poem_pack_conv7x7(None, 64, None, None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- poem_maxpool3x3_s2 -------------------------------------------------------------------------------------------------
def _pool3(xb, xs, ob, os_, views, c, h, w):
    return hip.lib().poem_maxpool3x3_s2(xb.data_ptr(), *xs, ob.data_ptr(), *os_, views, c, h, w, hip.stream())


@pytest.mark.parametrize("data", ["random", "negative", "special"])
def test_maxpool3x3_s2_is_torch_bit_for_bit(data):
    views, c, h, w = 3, 5, 8, 16
    g = torch.Generator().manual_seed(31)
    x = torch.randn(views, c, h, w, generator=g)
    if data == "negative":                                    # a zero pad would win every border window
        x = -x.abs() - 0.5
    elif data == "special":
        x[0, 1, 3, 5] = float("nan")
        x[1, 2, 4, :] = float("-inf")
        x[1, 2, 3:6, 0:3] = float("-inf")                     # a whole window of -inf
        x[2, 0, 0:3, 0:3] = torch.tensor([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]])
        x[2, 3, 2:5, 6:9] = torch.tensor([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0]])
        x[2, 0, 3:, :] = -x[2, 0, 3:, :].abs()
        x[2, 3, :, :6] = -x[2, 3, :, :6].abs() - 1
        x[2, 3, 5:, :] = -x[2, 3, 5:, :].abs() - 1
    ref = F.max_pool2d(x, 3, 2, 1)
    for in_b in (True, False):
        for out_b in (True, False):
            xb, _, xs = _buffer(x, in_b, "rand", g)            # junk in the border: the padding must count as -inf, unread
            ob, oint, os_ = _buffer(torch.zeros(views, c, h // 2, w // 2), out_b, SENTINEL, g)
            assert _pool3(xb, xs, ob, os_, views, c, h, w) == 0
            assert _bits_equal(oint, ref), (data, in_b, out_b)
            assert not out_b or _border_is(ob, SENTINEL)


def test_maxpool3x3_s2_refusals():
    x = torch.zeros(1, 5, 8, 16, device=DEV)
    out = torch.full((1, 5, 4, 8), SENTINEL, device=DEV)
    pi, po_ = _plain(5, 8, 16), _plain(5, 4, 8)
    assert _pool3(x, pi, out, po_, 1, 5, 7, 16) == hip.POEM_E_UNSUPPORTED                        # odd sizes
    assert _pool3(x, pi, out, po_, 1, 5, 8, 15) == hip.POEM_E_UNSUPPORTED
    assert _pool3(x, (5 * 128, 128, 16, 1), out, po_, 1, 5, 8, 16) == -1                         # input leaves its plane
    assert _pool3(x, pi, out, (5 * 32, 32, 7, 0), 1, 5, 8, 16) == -1                             # output rows overlap
    assert hip.lib().poem_maxpool3x3_s2(None, *pi, None, *po_, 1, 5, 8, 16, None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- poem_conv1x1_s2 ----------------------------------------------------------------------------------------------------
def _conv1s2(xb, xs, packed, shift, ob, os_, views, cin, cout, h, w):
    return hip.lib().poem_conv1x1_s2(xb.data_ptr(), *xs, packed.data_ptr(), hip.ptr(shift), ob.data_ptr(), *os_, views, cin, cout, h, w,
                                     hip.stream())


def _conv1s2_ref(x, wt, shift, dtype):
    return torch.einsum("oc,nchw->nohw", wt.to(dtype), x[:, :, ::2, ::2].to(dtype)) + shift.to(dtype).view(1, -1, 1, 1)


@pytest.mark.parametrize("cin,cout", [(64, 128), (256, 512), (1024, 2048)])
def test_conv1x1_s2(cin, cout):
    views, h, w = 2, 8, 16
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(views, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, generator=g) * (1.6 / cin) ** 0.5
    shift = 0.3 * torch.randn(cout, generator=g)
    packed, shift_d = _pack1(wt), shift.to(DEV)
    ref64, ref32 = _conv1s2_ref(x, wt, shift, torch.float64), _conv1s2_ref(x, wt, shift, torch.float32)
    first = None
    for in_b in (True, False):
        for out_b in (True, False):
            xb, _, xs = _buffer(x, in_b, "rand", g)
            ob, oint, os_ = _buffer(torch.zeros(views, cout, h // 2, w // 2), out_b, SENTINEL, g)
            assert _conv1s2(xb, xs, packed, shift_d, ob, os_, views, cin, cout, h, w) == 0
            _criterion(oint, ref64, ref32, f"conv1x1_s2 {cin}->{cout} in_b={in_b} out_b={out_b}")
            assert not out_b or _border_is(ob, SENTINEL)
            first = oint.clone() if first is None else first
            assert torch.equal(oint, first)                                   # the same bits whatever the maps
    xi = torch.randint(-3, 4, (views, cin, h, w), generator=g).float()
    wi = torch.randint(-2, 3, (cout, cin), generator=g).float()
    si = torch.randint(-5, 6, (cout,), generator=g).float()
    xb, _, xs = _buffer(xi, True, "rand", g)
    ob, oint, os_ = _buffer(torch.zeros(views, cout, h // 2, w // 2), True, SENTINEL, g)
    assert _conv1s2(xb, xs, _pack1(wi), si.to(DEV), ob, os_, views, cin, cout, h, w) == 0
    assert torch.equal(oint.cpu().double(), _conv1s2_ref(xi, wi, si, torch.float64)) and _border_is(ob, SENTINEL)


def test_conv1x1_s2_refusals():
    x = torch.zeros(1, 64, 8, 16, device=DEV)
    out = torch.full((1, 128, 4, 8), SENTINEL, device=DEV)
    packed, shift = _pack1(torch.zeros(128, 64)), torch.zeros(128, device=DEV)
    pi, po_ = _plain(64, 8, 16), _plain(128, 4, 8)
    assert _conv1s2(x, pi, packed, shift, out, po_, 1, 64, 128, 7, 16) == hip.POEM_E_UNSUPPORTED     # odd
    assert _conv1s2(x, pi, packed, shift, out, po_, 1, 64, 128, 8, 12) == hip.POEM_E_UNSUPPORTED     # 24 output pixels
    assert _conv1s2(x, pi, packed, shift, out, po_, 1, 60, 128, 8, 16) == -1                         # cin % 8
    assert _conv1s2(x, (64 * 128, 128, 16, 1), packed, shift, out, po_, 1, 64, 128, 8, 16) == -1     # input leaves its plane
    assert _conv1s2(x, pi, packed, shift, out, (128 * 32, 32, 7, 0), 1, 64, 128, 8, 16) == -1        # output rows overlap
    assert hip.lib().poem_conv1x1_s2(None, *pi, None, None, None, *po_, 1, 64, 128, 8, 16, None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- poem_maxpool2_conv1x1 ----------------------------------------------------------------------------------------------
def _pool_conv(x, packed, bias, out, cin, cout, h, w, act):
    return hip.lib().poem_maxpool2_conv1x1(x.data_ptr(), packed.data_ptr(), hip.ptr(bias), out.data_ptr(), x.shape[0], cin, cout, h, w, act,
                                           hip.stream())


def _pool_conv_ref(x, wt, bias, act, dtype):
    y = torch.einsum("oc,nchw->nohw", wt.to(dtype), F.max_pool2d(x.to(dtype), 2, 2)) + bias.to(dtype).view(1, -1, 1, 1)
    return torch.sigmoid(y) if act else y


@pytest.mark.parametrize("h,w", [(16, 16), (8, 16)])
@pytest.mark.parametrize("cin,cout,act", [(64, 128, 0), (256, 512, 0), (256, 21, 1), (64, 21, 1)])
def test_maxpool2_conv1x1(cin, cout, act, h, w):
    views = 3
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(views, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, generator=g) * (1.6 / cin) ** 0.5
    bias = 0.3 * torch.randn(cout, generator=g)
    xd, bd, packed = x.to(DEV), bias.to(DEV), _pack1(wt)
    out = torch.full((views, cout, h // 2, w // 2), SENTINEL, device=DEV)
    assert _pool_conv(xd, packed, bd, out, cin, cout, h, w, act) == 0
    ref64, ref32 = _pool_conv_ref(x, wt, bias, act, torch.float64), _pool_conv_ref(x, wt, bias, act, torch.float32)
    _criterion(out, ref64, ref32, f"maxpool2_conv1x1 {cin}->{cout} act={act} {h}x{w}")
    o2 = torch.empty(2, cout, h // 2, w // 2, device=DEV)                      # views are independent
    assert _pool_conv(xd[:2].contiguous(), packed, bd, o2, cin, cout, h, w, act) == 0
    assert torch.equal(o2, out[:2])
    if (cin, cout, act) == (64, 21, 1):                                       # the older read-out head on the same input
        hm = torch.empty(views, cout, h // 2, w // 2, device=DEV)
        hip.check(hip.lib().poem_pool_conv1x1_sigmoid(hip.ptr(xd), hip.ptr(wt.to(DEV).contiguous()), hip.ptr(bd), hip.ptr(hm), views, cin,
                                                      cout, h, w, hip.stream()), "poem_pool_conv1x1_sigmoid")
        _criterion(hm, ref64, ref32, "poem_pool_conv1x1_sigmoid on the same input")
    if not act:                                                               # small integers: exact; a NaN propagates as torch's
        xi = torch.randint(-3, 4, (views, cin, h, w), generator=g).float()
        wi = torch.randint(-2, 3, (cout, cin), generator=g).float()
        bi = torch.randint(-5, 6, (cout,), generator=g).float()
        assert _pool_conv(xi.to(DEV), _pack1(wi), bi.to(DEV), out, cin, cout, h, w, 0) == 0
        assert torch.equal(out.cpu().double(), _pool_conv_ref(xi, wi, bi, 0, torch.float64))
        xn = x.clone()
        xn[1, 3, 2, 5] = float("nan")
        assert _pool_conv(xn.to(DEV), packed, bd, out, cin, cout, h, w, 0) == 0
        refn = _pool_conv_ref(xn, wt, bias, 0, torch.float32)
        assert bool(refn.isnan().any()) and torch.equal(out.cpu().isnan(), refn.isnan())


def test_maxpool2_conv1x1_refusals():
    x = torch.zeros(1, 64, 16, 16, device=DEV)
    out = torch.full((1, 128, 8, 8), SENTINEL, device=DEV)
    packed, bias = _pack1(torch.zeros(128, 64)), torch.zeros(128, device=DEV)
    assert _pool_conv(x, packed, bias, out, 64, 128, 15, 16, 0) == hip.POEM_E_UNSUPPORTED            # odd
    assert _pool_conv(x, packed, bias, out, 64, 128, 16, 12, 0) == hip.POEM_E_UNSUPPORTED            # 48 output pixels
    assert _pool_conv(x, packed, bias, out, 60, 128, 16, 16, 0) == -1                                # cin % 8
    assert _pool_conv(x, packed, bias, out, 64, 128, 16, 16, 2) == -1                                # act
    assert hip.lib().poem_maxpool2_conv1x1(None, None, None, None, 1, 64, 128, 16, 16, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- the whole backbone -------------------------------------------------------------------------------------------------
SHAPES = {"2x128x256": (2, 128, 256), "1x256x256": (1, 256, 256), "1x128x256": (1, 128, 256)}
CASES = [(18, "2x128x256"), (18, "1x256x256"), (34, "2x128x256"), (34, "1x256x256"), (50, "1x128x256")]


def _images(views, h, w, seed):
    return 0.5 * torch.randn(views, 3, h, w, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def state_dicts():
    return {v: rn.seeded_resnet_state_dict(v, 0) for v in ru.VERSIONS}


@pytest.fixture(scope="module")
def cpu_refs(state_dicts):
    """(version, shape key) -> (image, fp64 levels, fp32 levels) of the CPU torch engine; computed once, never modified"""
    refs = {}
    for v in ru.VERSIONS:
        net32, net64 = ru.net_in(v, state_dicts[v]), ru.net_in(v, state_dicts[v], torch.float64)
        for version, key in CASES:
            if version == v:
                img = _images(*SHAPES[key], 17 + SHAPES[key][0])
                refs[(v, key)] = (img, ru.cpu_forward(net64, img.double()), net32(img))
    return refs


@pytest.fixture(scope="module")
def hip_nets(state_dicts):
    return {v: pk.build_backbone(pk.CN({"TYPE": f"ResNet{v}", "ENGINE": "hip"})).to(DEV) for v in ru.VERSIONS}


def _loaded(net, sd):
    if not net._built:
        net.load_state_dict(sd)
    return net


@pytest.mark.parametrize("version,key", CASES)
def test_backbone_levels_meet_the_criterion(hip_nets, state_dicts, cpu_refs, version, key):
    net = _loaded(hip_nets[version], state_dicts[version])
    assert net.engine == "hip" and net.name == f"resnet{version}"
    img, ref64, ref32 = cpu_refs[(version, key)]
    ys = net(img)
    assert [tuple(y.shape) for y in ys] == [tuple(r.shape) for r in ref64]
    for i, (y, r64, r32) in enumerate(zip(ys, ref64, ref32)):
        assert y.is_contiguous() and y.device.type == "cuda"
        _criterion(y, r64, r32, f"resnet{version} {key} level {i}")
    again = net(img.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(ys, again)), "two calls differ"
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(ys, again)), "a returned level was recycled"


@pytest.mark.parametrize("version", [18, 50])
def test_backbone_is_independent_of_what_ran_before(hip_nets, state_dicts, version):
    """3, 2, 3 views and alternating shapes on one engine against a freshly built engine per input: a stale border, a recycled
    buffer read too late or a plan reused across shapes would show"""
    net, sd = _loaded(hip_nets[version], state_dicts[version]), state_dicts[version]
    a3, b1 = _images(3, 128, 256, 5), _images(1, 256, 256, 6)
    a2 = a3[:2].contiguous()
    fresh = {}
    for name, img in (("a3", a3), ("a2", a2), ("b1", b1)):
        one = pk.build_backbone(pk.CN({"TYPE": f"ResNet{version}", "ENGINE": "hip"})).to(DEV)
        one.load_state_dict(sd)
        fresh[name] = [y.clone() for y in one(img)]
    for name, img in (("a3", a3), ("a2", a2), ("a3", a3), ("b1", b1), ("a3", a3), ("b1", b1)):
        got = net(img)
        assert all(torch.equal(x, y) for x, y in zip(got, fresh[name])), name
    assert all(torch.equal(x[:2], y) for x, y in zip(fresh["a3"], fresh["a2"]))          # views do not see each other


def test_hip_engine_refuses_other_shapes(hip_nets, state_dicts):
    net = _loaded(hip_nets[18], state_dicts[18])
    for h, w in ((64, 64), (224, 224), (128, 250)):
        with pytest.raises(ValueError):
            net(torch.zeros(1, 3, h, w))


# ---- the decoders, ResNet branch ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decode_refs():
    """backbone name -> (levels, decoder state dict, fp64 / fp32 feat_decode, fp64 / fp32 uv_decode) on the CPU"""
    refs = {}
    for name, views in (("resnet34", 2), ("resnet50", 1)):
        feats = ru.synthetic_levels(name, views, 128, 256, 3)
        sd = pk.weights.seeded_decoder_state_dict(2, backbone=name)
        f64, sd64 = [f.double() for f in feats], ru.cast_sd(sd, torch.float64)
        with torch.no_grad():
            refs[name] = (feats, sd, ru.feat_decode(f64, sd64), ru.feat_decode(feats, sd), ru.uv_decode(f64, sd64), ru.uv_decode(feats, sd))
    return refs


@pytest.mark.parametrize("name", ["resnet34", "resnet50"])
def test_decoders_resnet_branch(decode_refs, name):
    feats, sd, mlvl64, mlvl32, hm64, hm32 = decode_refs[name]
    views, c = feats[0].shape[0], pk.decode.FEAT_SIZES[name]
    dec = pk.decode.FeatureDecoders(sd, DEV, name)
    fd = [f.to(DEV) for f in feats]
    mlvl = dec.feat_decode(fd, name)
    assert tuple(mlvl.shape) == (views, c[1], 16, 32)
    _criterion(mlvl, mlvl64, mlvl32, f"{name} feat_decode")
    hm = dec.uv_decode(fd)
    assert tuple(hm.shape) == (views, 21, 16, 32)
    _criterion(hm, hm64, hm32, f"{name} uv_decode")
    # heat maps -> pixel coordinates inside the image; the confidence is the heat map's maximum
    uv, conf = dec.heatmap_stage(fd, 256, 128, return_conf=True)
    assert tuple(uv.shape) == (views, 21, 2) and tuple(conf.shape) == (views, 21)
    assert bool((uv[..., 0] >= 0).all()) and bool((uv[..., 0] <= 256).all()) and bool((uv[..., 1] >= 0).all()) and bool((uv[..., 1] <= 128).all())
    assert torch.equal(conf, hm.flatten(2).max(dim=-1).values)
    uv_ref = ru.heatmap_stage([f.double() for f in feats], ru.cast_sd(sd, torch.float64), 256, 128)
    assert float((uv.cpu().double() - uv_ref).abs().max()) < 5e-4 + 2.0 * float((hm.cpu().double() - hm64).abs().max()) * 256 * float(
        (hm64.shape[-1] * hm64.shape[-2] / hm64.sum(dim=(-1, -2))).max())          # tests/test_backbone.py's bound, pixels
    with pytest.raises(ValueError):
        dec.feat_decode(fd, "HRNet")
    with pytest.raises(ValueError):
        pk.decode.FeatureDecoders(pk.weights.seeded_decoder_state_dict(0), DEV, name)      # HRNet's channel table


@pytest.mark.parametrize("name", ["resnet34", "resnet50"])
def test_decoders_fused_and_unfused_routes_agree_in_bits(decode_refs, name):
    """[bilinear x2 | level] inside the convolution (poem_upcat_conv3x3, where it takes the shape) against
    poem_upsample2_concat_pad_staged + poem_conv3x3: the same bits, stage by stage and through both decoders"""
    feats, sd = decode_refs[name][:2]
    views = feats[0].shape[0]
    dec = pk.decode.FeatureDecoders(sd, DEV, name)
    fd = [f.to(DEV) for f in feats]
    taken = []
    for convs in (dec.feat_delayer, dec.uv_delayer):
        x = fd[3]
        for i, conv in enumerate(convs):
            b = fd[2 - i]
            h, w = int(b.shape[-2]), int(b.shape[-1])
            one, two = (torch.empty(views, conv.cout, h, w, device=DEV) for _ in range(2))
            if isinstance(conv, pk.decode._SplitConv3x3):                     # (ResNet-50's 3072 and 1536 channels: no fused form)
                conv(x, b, h, w, two)
                taken.append(False)
                x = two
                continue
            conv(pk.decode.upsample2_concat_pad(x, b, h, w, 1, staged=True), h, w, 1, two, _plain(conv.cout, h, w))
            took = conv.upcat(x, b, h, w, one, _plain(conv.cout, h, w))
            taken.append(bool(took))
            if took:
                assert torch.equal(one, two), (name, i)
            x = two
    print(f"{name}: stages on the fused route: {taken}")
    fused = (dec.feat_decode(fd, name), dec.uv_decode(fd))
    dec.fuse_upcat = [False, False, False]
    assert torch.equal(dec.feat_decode(fd, name), fused[0]) and torch.equal(dec.uv_decode(fd), fused[1])


def test_upsample2_concat_pad_staged_matches_torch():
    g = torch.Generator().manual_seed(9)
    a, b = torch.randn(2, 24, 4, 8, generator=g), torch.randn(2, 16, 8, 16, generator=g)
    ref = F.pad(torch.cat((F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=False), b), dim=1), (1, 1, 1, 1))
    ad, bd = a.to(DEV), b.to(DEV)
    got = pk.decode.upsample2_concat_pad(ad, bd, 8, 16, 1, staged=True)
    assert tuple(got.shape) == (2, 40, 10, 18) and float((got.cpu() - ref).abs().max()) < 1e-6      # the rounding of one fma chain
    assert torch.equal(got[:, 24:], pk.decode.upsample2_concat_pad(ad, bd, 8, 16, 1)[:, 24:]) and _border_is(got, 0.0)
    assert torch.equal(pk.decode.upsample2_concat_pad(ad, None, 8, 16, 1, staged=True), got[:, :24])
    assert torch.equal(pk.decode.upsample2_concat_pad(None, bd, 8, 16, 1, staged=True), got[:, 24:])
    L, out = hip.lib(), torch.full((2, 40, 10, 18), SENTINEL, device=DEV)
    assert L.poem_upsample2_concat_pad_staged(ad.data_ptr(), 24, bd.data_ptr(), 16, out.data_ptr(), 2, 7, 16, hip.stream()) == hip.POEM_E_UNSUPPORTED
    assert L.poem_upsample2_concat_pad_staged(None, 24, bd.data_ptr(), 16, out.data_ptr(), 2, 8, 16, hip.stream()) == -1
    assert L.poem_upsample2_concat_pad_staged(ad.data_ptr(), 24, bd.data_ptr(), 16, None, 2, 8, 16, hip.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- the model ----------------------------------------------------------------------------------------------------------
def _model(engine, views):
    node = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": dict(pk.configs.head_cfg(128), IN_CHANNELS=128), "DATA_PRESET": {"CENTER_IDX": 9},
            "BACKBONE": {"TYPE": "ResNet34", "ENGINE": engine, "PRETRAINED": False, "FREEZE_BATCHNORM": True}}
    model = pk.build_model(pk.CN(node))
    parts = (rn.seeded_resnet_state_dict(34, 0), pk.weights.seeded_decoder_state_dict(0, backbone="resnet34"),
             pk.weights.seeded_state_dict(128, seed=0, in_channels=128))
    model.load_parts(*parts, template=po.synthetic_template(1234))
    b = pk.inputs.synthetic_batch(views, seed=4)
    batch = {"image": pk.inputs.synthetic_images(sum(views), seed=4), "target_cam_intr": b["img_metas"]["cam_intr"],
             "target_cam_extr": b["img_metas"]["cam_extr"], "master_id": [0] * len(views), "cam_view_num": np.asarray(views)}
    return model, batch, b, parts


def test_model_with_resnet34_matches_staged_oracles():
    """images -> ResNet-34 (hip engine) -> feat_decode / heatmap_stage / DLT / head against the same chain built from the CPU torch
    ResNet + resnet_util's decode + the DLT / path oracles, stage by stage (tests/test_backbone.py's bars), and against the same
    model on the torch engine."""
    import dlt_oracle
    from util import oracle_consts, run_oracle
    views = [3, 2]
    model, batch, b, (bsd, dsd, hsd) = _model("hip", views)
    assert model.img_backbone.name == "resnet34" and model.img_backbone.engine == "hip" and model.decoders is not None
    assert model.decoders.backbone == "resnet34"
    seen, feats, decode = {}, model.extract_img_feat, model.decoders.feat_decode
    model.extract_img_feat = lambda x: seen.setdefault("pyr", feats(x))
    model.decoders.feat_decode = lambda f, name: seen.setdefault("mlvl", decode(f, name))
    preds = model(batch, 0, mode="test")
    del model.extract_img_feat, model.decoders.feat_decode
    for k in ("all_coords_preds", "pred_joints_3d", "pred_verts_3d", "pred_joints_3d_rel", "pred_verts_3d_rel", "pred_joints_uv",
              "pred_ref_joints_3d"):
        assert k in preds and bool(torch.isfinite(preds[k]).all()), k
    assert tuple(preds["pred_verts_3d"].shape) == (2, 778, 3) and tuple(preds["pred_joints_uv"].shape) == (5, 21, 2)
    assert tuple(preds["all_coords_preds"].shape) == (3, 2, 799, 3) and tuple(seen["mlvl"].shape) == (5, 128, 32, 32)
    pyr_d, img = seen["pyr"], batch["image"]
    pyr_c = rn.ResNet34(state_dict=bsd)(img)
    for yd, yc in zip(pyr_d, pyr_c):
        assert float((yd.cpu() - yc).abs().max()) < 1e-3 * float(yc.abs().max())
    pyr = [y.cpu() for y in pyr_d]
    mlvl_d, mlvl = seen["mlvl"], ru.feat_decode(pyr, dsd)
    assert float((mlvl_d.cpu() - mlvl).abs().max()) < 2e-5 * float(mlvl.abs().max())
    hm_d, hm = model.decoders.uv_decode(pyr_d).cpu(), ru.uv_decode(pyr, dsd)
    e_hm = float((hm_d - hm).abs().max())
    logit_scale = max(1.0, float(torch.logit(hm.double().clamp(1e-12, 1 - 1e-12)).abs().max()))
    assert e_hm < 2e-5 * logit_scale, (e_hm, logit_scale)
    import decode_oracle as do
    uv_same_hm = do.heatmap_to_uv(hm_d, 256, 256)
    assert float((preds["pred_joints_uv"].cpu() - uv_same_hm).abs().max()) < 5e-4      # pixels
    uv = ru.heatmap_stage(pyr, dsd, 256, 256)
    bound = 2.0 * e_hm * 256.0 * float((hm.shape[-1] * hm.shape[-2] / hm.sum(dim=(-1, -2))).max()) + 5e-4
    assert float((preds["pred_joints_uv"].cpu() - uv).abs().max()) < min(bound, 2e-2)
    rj = dlt_oracle.triangulate_reference_joints(preds["pred_joints_uv"].cpu(), b["img_metas"]["cam_intr"], b["img_metas"]["cam_extr"], views)
    assert float((preds["pred_ref_joints_3d"].cpu() - rj).abs().max()) < 5e-6          # metres
    ob = dict(b)
    ob["mlvl_feat"] = mlvl_d.cpu()
    ob["reference_joints"] = preds["pred_ref_joints_3d"].cpu()
    spec_cfg = po.PathConfig(embed=128, nsample=4096, parametric=False, in_channels=128)
    ref = run_oracle(spec_cfg, hsd, oracle_consts(4096), ob)["all_coords_preds"]
    got = preds["all_coords_preds"].cpu()
    mpvpe_mm = float((got[-1, :, 21:] - ref[-1, :, 21:]).norm(dim=-1).mean()) * 1e3
    assert mpvpe_mm < 1e-3, mpvpe_mm
    # the torch engine (MIOpen) under the same model: the backbone bar of the HRNet test
    tmodel, _, _, _ = _model("torch", views)
    assert tmodel.img_backbone.engine == "torch" and tmodel.img_backbone._hip is None
    for yd, yt in zip(pyr_d, tmodel.extract_img_feat(img.to(DEV))):
        assert float((yd - yt).abs().max()) < 1e-3 * float(yd.abs().max())
    tp = tmodel(batch, 0, mode="test")
    assert bool(torch.isfinite(tp["all_coords_preds"]).all()) and tp["all_coords_preds"].shape == preds["all_coords_preds"].shape
