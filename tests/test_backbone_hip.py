"""The HRNet backbone's hip engine on the device: the three new operators through the C ABI, the whole backbone, and the
model-level caller with ``BACKBONE.ENGINE = "hip"``.

Yardstick: the CPU torch engine (itself pinned to the reference's HRNet by tests/golden/backbone.npz), evaluated in fp64, and
in fp32 for the error scale.  Criterion (tests/test_gemm_forms.py's rule), max norm per output tensor:

    max|HIP - fp64| <= 4 * max|fp32_cpu - fp64| + 1e-6 * max|fp64|

plus exact equality on small-integer data (every partial sum is exact in fp32: any indexing mistake shows) and bit equality
wherever the code promises it."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import poem_v2_amd as pk
from poem_v2_amd import backbone as bb
from poem_v2_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _criterion(got, ref64, ref32, what=""):
    err = float((got.double().cpu() - ref64).abs().max())
    scale = float((ref32.double() - ref64).abs().max())
    bound = 4.0 * scale + 1e-6 * float(ref64.abs().max())
    print(f"{what}: max|hip - fp64| = {err:.3e}   max|fp32 - fp64| = {scale:.3e}   bound = {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _plain(c, h, w):
    return (c * h * w, h * w, w, 0)


def _bordered(c, h, w):
    return (c * (h + 2) * (w + 2), (h + 2) * (w + 2), w + 2, w + 3)


def _buffer(x, bordered, fill, g):
    """x (n,c,h,w) on the device as a plain tensor or inside a buffer whose border holds ``fill`` ("rand": junk that a wrong
    offset would read).  Returns (buffer, interior view, strides)."""
    n, c, h, w = x.shape
    if not bordered:
        t = x.to(DEV).contiguous()
        return t, t, _plain(c, h, w)
    buf = torch.randn(n, c, h + 2, w + 2, generator=g) * 7 if fill == "rand" else torch.full((n, c, h + 2, w + 2), float(fill))
    buf[:, :, 1:-1, 1:-1] = x
    buf = buf.to(DEV)
    return buf, buf[:, :, 1:-1, 1:-1], _bordered(c, h, w)


def _border_is(buf, value):
    b = buf.clone()
    b[:, :, 1:-1, 1:-1] = value
    return bool((b == value).all())


def _pad32(t):
    out = torch.zeros((t.numel() + 31) // 32 * 32, device=DEV)
    out[:t.numel()] = t.to(DEV)
    return out


# ---- poem_conv3x3_ex ----------------------------------------------------------------------------------------------------
class _Conv3:
    def __init__(self, w, scale, shift):
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])
        L = hip.lib()
        self.packed = torch.empty(L.poem_conv3x3_packed_bytes(self.cout, self.cin), dtype=torch.uint8, device=DEV)
        self.w = w.to(DEV).contiguous()
        hip.check(L.poem_pack_conv3x3(hip.ptr(self.w), self.cout, self.cin, self.packed.data_ptr(), hip.stream()))
        self.scale, self.shift = _pad32(scale), _pad32(shift)

    def ex(self, xp, h, w, stride, res, res_strides, pre, out, out_strides, relu=1):
        return hip.lib().poem_conv3x3_ex(hip.ptr(xp), self.packed.data_ptr(), hip.ptr(self.scale), hip.ptr(self.shift),
                                         None if res is None else res.data_ptr(), *res_strides, pre, out.data_ptr(), xp.shape[0],
                                         self.cin, self.cout, h, w, stride, relu, *out_strides, hip.stream())

    def old(self, xp, h, w, stride, res, out, out_strides, relu=1):
        return hip.lib().poem_conv3x3(hip.ptr(xp), self.packed.data_ptr(), hip.ptr(self.scale), hip.ptr(self.shift),
                                      hip.ptr(res), out.data_ptr(), xp.shape[0], self.cin, self.cout, h, w, stride, relu,
                                      *out_strides, hip.stream())


def _conv3_ref(x, w, scale, shift, res, stride, dtype):
    y = F.conv2d(x.to(dtype), w.to(dtype), stride=stride, padding=1)
    y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1) + res.to(dtype)
    return F.relu(y)


CONV3_SHAPES = [  # views, cin, cout, h, w, stride: the smallest shape that reaches each kernel family
    pytest.param(3, 40, 40, 8, 8, 1, id="direct-ct2-pt2-idle-waves"),
    pytest.param(3, 40, 40, 16, 16, 1, id="lds-16row"),
    pytest.param(2, 64, 64, 16, 16, 1, id="lds-32row"),
    pytest.param(2, 320, 320, 4, 8, 1, id="direct-ct5-pt1"),
    pytest.param(2, 40, 80, 16, 16, 2, id="stride2"),
]


@pytest.mark.parametrize("views,cin,cout,h,w,stride", CONV3_SHAPES)
def test_conv3x3_ex(views, cin, cout, h, w, stride):
    g = torch.Generator().manual_seed(cin * 1000 + cout + h + stride)
    ho, wo = h // stride, w // stride
    for integers in (False, True):
        if integers:
            x = torch.randint(-3, 4, (views, cin, h, w), generator=g).float()
            wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float()
            scale, shift = torch.ones(cout), torch.randint(-5, 6, (cout,), generator=g).float()
            res = torch.randint(-9, 10, (views, cout, ho, wo), generator=g).float()
        else:
            x = torch.randn(views, cin, h, w, generator=g)
            wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (9 * cin)) ** 0.5
            scale, shift = 1 + 0.2 * (2 * torch.rand(cout, generator=g) - 1), 0.3 * torch.randn(cout, generator=g)
            res = torch.randn(views, cout, ho, wo, generator=g)
        conv = _Conv3(wt, scale, shift)
        xp = F.pad(x, (1, 1, 1, 1)).to(DEV).contiguous()
        # residual before the ReLU, read from the interior of a buffer whose border is junk; output into a sentinel-filled buffer
        rbuf, _, rstr = _buffer(res, True, "rand", g)
        obuf, oint, ostr = _buffer(torch.zeros(views, cout, ho, wo), True, SENTINEL, g)
        assert conv.ex(xp, h, w, stride, rbuf, rstr, 1, obuf, ostr) == 0
        ref64 = _conv3_ref(x, wt, scale, shift, res, stride, torch.float64)
        if integers:
            assert torch.equal(oint.cpu().double(), ref64)
        else:
            _criterion(oint, ref64, _conv3_ref(x, wt, scale, shift, res, stride, torch.float32), f"conv3x3_ex {cin}->{cout} {h}x{w}/{stride}")
        assert _border_is(obuf, SENTINEL), "a store outside the interior"
        # the old order (activation, then a plain residual): poem_conv3x3's bits, with and without the residual
        rp = res.to(DEV).contiguous()
        for r in (rp, None):
            a, b = torch.empty(views, cout, ho, wo, device=DEV), torch.empty(views, cout, ho, wo, device=DEV)
            assert conv.old(xp, h, w, stride, r, a, _plain(cout, ho, wo)) == 0
            assert conv.ex(xp, h, w, stride, r, _plain(cout, ho, wo), 0, b, _plain(cout, ho, wo)) == 0
            assert torch.equal(a, b)


def test_conv3x3_ex_refusals():
    conv = _Conv3(torch.zeros(40, 40, 3, 3), torch.ones(40), torch.zeros(40))
    xp = torch.zeros(1, 40, 10, 10, device=DEV)
    out = torch.full((1, 40, 8, 8), SENTINEL, device=DEV)
    ps = _plain(40, 8, 8)
    assert conv.ex(xp, 8, 8, 3, None, (0, 0, 0, 0), 1, out, ps) == hip.POEM_E_UNSUPPORTED          # stride
    assert conv.ex(xp, 8, 6, 1, None, (0, 0, 0, 0), 1, out, _plain(40, 8, 6)) == hip.POEM_E_UNSUPPORTED   # 48 pixels
    assert conv.ex(xp, 8, 8, 1, out, (40 * 64, 64, 8, 9), 1, out, ps) == -1                        # residual outside its plane
    assert conv.ex(xp, 8, 8, 1, None, (0, 0, 0, 0), 1, out, (40 * 64, 64, 7, 0)) == -1             # rows overlap
    assert conv.ex(xp, 1 << 12, 1 << 12, 1, None, (0, 0, 0, 0), 1, out, _plain(40, 1 << 12, 1 << 12)) == hip.POEM_E_UNSUPPORTED   # >= 2 GiB
    L = hip.lib()
    assert L.poem_conv3x3_ex(None, None, None, None, None, 0, 0, 0, 0, 1, None, 1, 40, 40, 8, 8, 1, 1, *ps, None) == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- poem_conv1x1 -------------------------------------------------------------------------------------------------------
def _conv1(x_t, xs, packed, shift, res_t, rs, out_t, os_, views, cin, cout, h, w, relu):
    return hip.lib().poem_conv1x1(x_t.data_ptr(), *xs, packed.data_ptr(), hip.ptr(shift), None if res_t is None else res_t.data_ptr(),
                                  *rs, out_t.data_ptr(), *os_, views, cin, cout, h, w, relu, hip.stream())


def _pack1(wt):
    cout, cin = wt.shape
    L = hip.lib()
    packed = torch.empty(L.poem_conv1x1_packed_bytes(cout, cin), dtype=torch.uint8, device=DEV)
    wd = wt.to(DEV).contiguous()
    hip.check(L.poem_pack_conv1x1(hip.ptr(wd), cout, cin, packed.data_ptr(), hip.stream()), "poem_pack_conv1x1")
    torch.cuda.synchronize()
    return packed


def _conv1_ref(x, wt, shift, res, relu, dtype):
    y = torch.einsum("oc,nchw->nohw", wt.to(dtype), x.to(dtype)) + shift.to(dtype).view(1, -1, 1, 1)
    if res is not None:
        y = y + res.to(dtype)
    return F.relu(y) if relu else y


@pytest.mark.parametrize("h,w", [(4, 8), (16, 16)])
@pytest.mark.parametrize("cin,cout", [(64, 64), (256, 64), (64, 256), (320, 40), (80, 40), (40, 32), (8, 96), (24, 160)])
def test_conv1x1(cin, cout, h, w):
    views = 3
    g = torch.Generator().manual_seed(cin + 7 * cout + h)
    x = torch.randn(views, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, generator=g) * (1.6 / cin) ** 0.5
    shift, res = 0.3 * torch.randn(cout, generator=g), torch.randn(views, cout, h, w, generator=g)
    packed, shift_d = _pack1(wt), shift.to(DEV)
    refs = {r: (_conv1_ref(x, wt, shift, res if r else None, r, torch.float64), _conv1_ref(x, wt, shift, res if r else None, r, torch.float32))
            for r in (0, 1)}
    for in_b in (False, True):
        for out_b in (False, True):
            for with_res in (0, 1):                                     # residual + ReLU together, as the Bottleneck uses them
                xb, _, xs = _buffer(x, in_b, "rand", g)
                ob, oint, os_ = _buffer(torch.zeros(views, cout, h, w), out_b, SENTINEL, g)
                rb, _, rs = _buffer(res, in_b, "rand", g) if with_res else (None, None, (0, 0, 0, 0))
                assert _conv1(xb, xs, packed, shift_d, rb, rs, ob, os_, views, cin, cout, h, w, with_res) == 0
                _criterion(oint, *refs[with_res], f"conv1x1 {cin}->{cout} {h}x{w} in_b={in_b} out_b={out_b} res={with_res}")
                if out_b:
                    assert _border_is(ob, SENTINEL)
    # small integers: exact
    xi = torch.randint(-3, 4, (views, cin, h, w), generator=g).float()
    wi = torch.randint(-2, 3, (cout, cin), generator=g).float()
    si, ri = torch.randint(-5, 6, (cout,), generator=g).float(), torch.randint(-9, 10, (views, cout, h, w), generator=g).float()
    xb, _, xs = _buffer(xi, True, "rand", g)
    rb, _, rs = _buffer(ri, True, "rand", g)
    ob, oint, os_ = _buffer(torch.zeros(views, cout, h, w), True, SENTINEL, g)
    assert _conv1(xb, xs, _pack1(wi), si.to(DEV), rb, rs, ob, os_, views, cin, cout, h, w, 1) == 0
    assert torch.equal(oint.cpu().double(), _conv1_ref(xi, wi, si, ri, 1, torch.float64)) and _border_is(ob, SENTINEL)


def test_conv1x1_refusals():
    L = hip.lib()
    x = torch.zeros(1, 64, 4, 8, device=DEV)
    out = torch.full((1, 40, 4, 8), SENTINEL, device=DEV)
    packed, shift = _pack1(torch.zeros(40, 64)), torch.zeros(40, device=DEV)
    ps_i, ps_o = _plain(64, 4, 8), _plain(40, 4, 8)
    assert _conv1(x, ps_i, packed, shift, None, (0, 0, 0, 0), out, ps_o, 1, 64, 40, 4, 8, 0) == 0
    assert L.poem_conv1x1_packed_bytes(40, 60) == 0
    assert L.poem_pack_conv1x1(x.data_ptr(), 40, 60, packed.data_ptr(), hip.stream()) == -1                        # cin % 8
    assert _conv1(x, ps_i, packed, shift, None, (0, 0, 0, 0), out, ps_o, 1, 60, 40, 4, 8, 0) == -1                 # cin % 8
    assert _conv1(x, _plain(64, 4, 6), packed, shift, None, (0, 0, 0, 0), out, _plain(40, 4, 6), 1, 64, 40, 4, 6, 0) == hip.POEM_E_UNSUPPORTED
    big = 1 << 23                                                                                                   # 64 * 2^23 * 4 B = 2 GiB
    assert _conv1(x, (64 * big, big, 8, 0), packed, shift, None, (0, 0, 0, 0), out, ps_o, 1, 64, 40, 4, 8, 0) == hip.POEM_E_UNSUPPORTED
    assert _conv1(x, (64 * 32, 32, 8, 1), packed, shift, None, (0, 0, 0, 0), out, ps_o, 1, 64, 40, 4, 8, 0) == -1  # leaves its plane
    assert _conv1(x, ps_i, packed, shift, out, (40 * 32, 32, 7, 0), out, ps_o, 1, 64, 40, 4, 8, 0) == -1           # residual rows overlap
    assert L.poem_conv1x1(None, *ps_i, packed.data_ptr(), None, None, 0, 0, 0, 0, out.data_ptr(), *ps_o, 1, 64, 40, 4, 8, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 0).all())                                              # only the accepted call wrote


# ---- poem_hrnet_fuse ----------------------------------------------------------------------------------------------------
def _fuse(terms, out_t, out_strides, views, c, h, w):
    arr = (hip.PoemFuseTerm * len(terms))()
    for t, (tensor, strides, shift) in zip(arr, terms):
        t.data, t.view_stride, t.ch_stride, t.row_stride, t.offset, t.shift = tensor.data_ptr(), *strides, shift
    return hip.lib().poem_hrnet_fuse(arr, len(terms), out_t.data_ptr(), *out_strides, views, c, h, w, hip.stream())


@pytest.mark.parametrize("nb", [2, 3, 4])
def test_hrnet_fuse_is_torch_bit_for_bit(nb):
    """every position i of the branch's own (bordered) map among nb terms: terms j > i are 2^(j-i) coarser maps read through the
    nearest upsampling (shifts 1..3), terms j < i plain maps of the same size; bordered and plain output; one NaN."""
    views, c, h, w = 3, 5, 8, 16
    g = torch.Generator().manual_seed(40 + nb)
    for i in range(nb):
        maps = []
        for j in range(nb):
            s = max(0, j - i)
            maps.append(torch.randn(views, c, h >> s, w >> s, generator=g))
        maps[(i + 1) % nb][1, 2, 0, 1] = float("nan")
        maps[0][0, 0, 3, 3] = -50.0                                               # a sum that the ReLU clips
        y = None
        for j, m in enumerate(maps):                                              # hrnet.py:226-233
            t = F.interpolate(m, scale_factor=2 ** (j - i), mode="nearest") if j > i else m
            y = t if y is None else y + t
        ref = F.relu(y)
        assert bool(ref.isnan().any()) and not bool(ref.isnan().all())
        terms = []
        for j, m in enumerate(maps):
            buf, _, strides = _buffer(m, j == i, "rand", g)
            terms.append((buf, strides, max(0, j - i)))
        for out_b in (True, False):
            ob, oint, os_ = _buffer(torch.zeros(views, c, h, w), out_b, SENTINEL, g)
            assert _fuse(terms, ob, os_, views, c, h, w) == 0
            got = oint.cpu()
            assert torch.equal(got.isnan(), ref.isnan())
            assert torch.equal(torch.nan_to_num(got, nan=1.0).view(torch.int32), torch.nan_to_num(ref, nan=1.0).view(torch.int32))
            if out_b:
                assert _border_is(ob, SENTINEL)


def test_hrnet_fuse_refusals():
    a = torch.zeros(1, 2, 4, 4, device=DEV)
    out = torch.full((1, 2, 4, 4), SENTINEL, device=DEV)
    ps = _plain(2, 4, 4)
    assert _fuse([(a, ps, 0)], out, ps, 1, 2, 4, 4) == -1                           # one term
    assert _fuse([(a, ps, 0)] * 5, out, ps, 1, 2, 4, 4) == -1
    assert _fuse([(a, ps, 0), (a, ps, 4)], out, ps, 1, 2, 4, 4) == -1               # shift
    assert _fuse([(a, ps, 0), (a, (32, 16, 3, 0), 0)], out, ps, 1, 2, 4, 4) == -1   # rows overlap
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- the whole backbone -------------------------------------------------------------------------------------------------
def _cpu_forward(net, x):
    """the torch engine's forward (backbone.run_graph) in the dtype of ``x`` and of the net's folded weights"""
    return bb.run_graph(net._graph, net._convs, x)


@pytest.fixture(scope="module")
def hrnet_sd():
    return bb.seeded_hrnet_state_dict(0)


def _images(views, h, w, seed):
    return 0.5 * torch.randn(views, 3, h, w, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def cpu_refs(hrnet_sd):
    """input -> (image, fp64 levels, fp32 levels) of the CPU torch engine; computed once, never modified"""
    net32 = bb.HRNet(state_dict=hrnet_sd)
    net64 = bb.HRNet(state_dict=hrnet_sd)
    for c in net64._convs.values():
        c.weight, c.bias = c.weight.double(), c.bias.double()              # the same fp32-rounded folded weights, fp64 arithmetic
    refs = {}
    with torch.no_grad():
        for key, (views, h, w) in {"3x128x256": (3, 128, 256), "1x256x256": (1, 256, 256)}.items():
            img = _images(views, h, w, 11 + views)
            refs[key] = (img, _cpu_forward(net64, img.double()), net32(img))
    return refs


@pytest.fixture(scope="module")
def hip_net(hrnet_sd):
    return bb.HRNet({"ENGINE": "hip"}, state_dict=hrnet_sd, device=DEV)


@pytest.mark.parametrize("key", ["3x128x256", "1x256x256"])
def test_backbone_levels_meet_the_criterion(hip_net, cpu_refs, key):
    img, ref64, ref32 = cpu_refs[key]
    ys = hip_net(img)
    assert [tuple(y.shape) for y in ys] == [tuple(r.shape) for r in ref64]
    for i, (y, r64, r32) in enumerate(zip(ys, ref64, ref32)):
        assert y.is_contiguous() and y.device.type == "cuda"
        _criterion(y, r64, r32, f"{key} level {i}")
    again = hip_net(img.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(ys, again)), "two calls differ"
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(ys, again)), "a returned level was recycled"


def test_backbone_is_independent_of_what_ran_before(hip_net, hrnet_sd, cpu_refs):
    """3, 2, 3 views and 256^2, 128x256, 256^2 on one engine against a freshly built engine per input: a stale border or a
    plan reused across shapes would show"""
    a3, b1 = cpu_refs["3x128x256"][0], cpu_refs["1x256x256"][0]
    a2 = a3[:2].contiguous()
    fresh = {}
    for name, img in (("a3", a3), ("a2", a2), ("b1", b1)):
        fresh[name] = [y.clone() for y in bb.HRNet({"ENGINE": "hip"}, state_dict=hrnet_sd, device=DEV)(img)]
    for name, img in (("a3", a3), ("a2", a2), ("a3", a3), ("b1", b1), ("a3", a3), ("b1", b1)):
        got = hip_net(img)
        assert all(torch.equal(x, y) for x, y in zip(got, fresh[name])), name
    assert all(torch.equal(x[:2], y) for x, y in zip(fresh["a3"], fresh["a2"]))          # views do not see each other


# ---- the model ----------------------------------------------------------------------------------------------------------
def _model(engine, views):
    node = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": pk.configs.head_cfg(128), "DATA_PRESET": {"CENTER_IDX": 9}}
    if engine is not None:
        node["BACKBONE"] = {"ENGINE": engine}
    import poem_oracle as po
    model = pk.build_model(pk.CN(node))
    model.load_parts(bb.seeded_hrnet_state_dict(0), pk.weights.seeded_decoder_state_dict(0), pk.weights.seeded_state_dict(128, seed=0),
                     template=po.synthetic_template(1234))
    b = pk.inputs.synthetic_batch(views, seed=4)
    import numpy as np
    batch = {"image": pk.inputs.synthetic_images(sum(views), seed=4), "target_cam_intr": b["img_metas"]["cam_intr"],
             "target_cam_extr": b["img_metas"]["cam_extr"], "master_id": [0] * len(views), "cam_view_num": np.asarray(views)}
    return model, batch


def test_model_with_hip_backbone():
    views = [3, 2]
    model, batch = _model("hip", views)
    assert model.img_backbone.engine == "hip"
    seen, backbone = {}, model.extract_img_feat
    model.extract_img_feat = lambda x: seen.setdefault("pyr", backbone(x))
    preds = model(batch, 0, mode="test")
    del model.extract_img_feat
    for k in ("all_coords_preds", "pred_joints_3d", "pred_verts_3d", "pred_joints_3d_rel", "pred_verts_3d_rel", "pred_joints_uv",
              "pred_ref_joints_3d"):
        assert k in preds and bool(torch.isfinite(preds[k]).all()), k
    assert tuple(preds["pred_verts_3d"].shape) == (2, 778, 3) and tuple(preds["pred_joints_uv"].shape) == (5, 21, 2)
    pyr_c = bb.HRNet(state_dict=bb.seeded_hrnet_state_dict(0))(batch["image"])
    for yd, yc in zip(seen["pyr"], pyr_c):                                 # the bar tests/test_backbone.py holds MIOpen to
        assert float((yd.cpu() - yc).abs().max()) < 1e-3 * float(yc.abs().max())


_DEFAULT_ROUTE = r"""
import sys
sys.path[:0] = [{root!r}, {root!r} + "/oracle", {root!r} + "/tests"]
import torch
torch.backends.cudnn.deterministic = True          # MIOpen's reproducible solvers: without it two forwards of the DEFAULT engine differ
import test_backbone_hip as t
keys = ("all_coords_preds", "pred_joints_uv", "pred_ref_joints_3d", "pred_verts_3d")
def run(engine):
    model, batch = t._model(engine, [3, 2])
    preds = model(batch, 0, mode="test")
    return model, {{k: preds[k].clone() for k in keys}}
same = lambda a, b: all(torch.equal(a[k], b[k]) for k in keys)
warm_model, warm = run(None)                       # the process's first forward: MIOpen settles on its solvers here
first_model, first = run(None)                     # a model built and run before any "hip" engine exists in this process
assert first_model.img_backbone.engine == "torch" and first_model.img_backbone._hip is None
hip_model, _ = run("hip")
assert hip_model.img_backbone._hip is not None
later_model, later = run(None)                     # ENGINE absent, a hip engine alive next to it
assert later_model.img_backbone._hip is None and later_model.img_backbone.engine == "torch"
img = torch.ones(2, 3, 256, 256, device="cuda:0")
print("backbone alone, same model twice:", all(torch.equal(a, b) for a, b in zip(first_model.img_backbone(img), first_model.img_backbone(img))))
print("first forward of the process == second:", same(warm, first))
print("DEFAULT_ROUTE", "bit-equal" if same(first, later) else "differs")
"""


def test_default_route_is_untouched_by_a_hip_engine():
    """ENGINE absent: the forward's outputs are those of a model built before any hip engine existed in the process (a fresh
    process: this one may have built hip engines already).  The child runs MIOpen in its deterministic mode: with the default
    solvers two forwards of identical default-engine models differ in every key, hip engine or not, so bits could not be compared."""
    out = subprocess.run([sys.executable, "-c", _DEFAULT_ROUTE.format(root=ROOT)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "DEFAULT_ROUTE bit-equal" in out.stdout, out.stdout[-2000:]
