"""The HRNet backbone's engine switch and the hip engine's plan, without a device: ``cfg.ENGINE`` parsing, the input rule, the
launch list and buffer plan of ``HipPlan`` (geometry of every producer / consumer pair, buffer reuse, liveness), the 8-channel
padding of ``conv1`` and the new C ABI declarations.  The kernels themselves: tests/test_backbone_hip.py (GPU)."""
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

import poem_v2_amd as pk
from poem_v2_amd import backbone as bb
from poem_v2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((3, 128, 256), (1, 256, 256), (2, 512, 512))


# ---- configuration ------------------------------------------------------------------------------------------------------
def test_engine_parsing():
    assert bb.HRNet().engine == "torch" and bb.HRNet(None).engine == "torch"
    assert bb.HRNet({}).engine == "torch" and bb.HRNet(pk.CN({"PRETRAINED": None})).engine == "torch"
    assert bb.HRNet({"ENGINE": "torch"}).engine == "torch"
    assert bb.HRNet(pk.CN({"ENGINE": "hip"})).engine == "hip"

    class Node:
        ENGINE = "hip"
    assert bb.HRNet(Node()).engine == "hip"
    for bad in ("HIP", "miopen", "", None, 1):
        with pytest.raises(ValueError, match="ENGINE"):
            bb.HRNet({"ENGINE": bad})


@pytest.mark.parametrize("hw", [(64, 64), (224, 224), (256, 250), (32, 512)])
def test_hip_engine_refuses_inputs_outside_the_rule(hw):
    """before anything else: no weights, no device needed to be told that the shape is not taken"""
    net = bb.HRNet({"ENGINE": "hip"})
    with pytest.raises(ValueError, match=r"multiples of 32"):
        net(torch.zeros(1, 3, *hw))
    with pytest.raises(ValueError):
        bb.HipPlan(1, *hw)
    with pytest.raises(RuntimeError):                            # the torch engine takes them (and then misses its weights)
        bb.HRNet()(torch.zeros(1, 3, *hw))


def test_hip_engine_accepts_the_documented_inputs():
    for hw in ((256, 256), (128, 256), (512, 512), (256, 128), (1024, 32)):
        bb.check_hip_input(*hw)
    with pytest.raises(RuntimeError, match="no weights"):        # a shape it takes gets as far as the weights
        bb.HRNet({"ENGINE": "hip"})(torch.zeros(1, 3, 256, 256))


# ---- the plan -----------------------------------------------------------------------------------------------------------
def _specs():
    return {conv: (cout, cin, k, stride) for conv, _, cout, cin, k, stride in bb._conv_specs()}


def _maps(op):
    if op["kind"] == "fuse":
        return [m for m, _ in op["terms"]], op["out"]
    if op["kind"] == "input":
        return [], op["out"]
    return [op["in"]] + ([op["res"]] if op["res"] is not None else []), op["out"]


@pytest.mark.parametrize("views,H,W", SHAPES)
def test_plan_runs_every_convolution_once_in_spec_order(views, H, W):
    plan = bb.HipPlan(views, H, W)
    names = [op["conv"] for op in plan.ops if "conv" in op]
    spec = [s[0] for s in bb._conv_specs()]
    assert sorted(names) == sorted(spec) and len(set(names)) == len(names)
    # _conv_specs order, except that downsample.0 runs before the conv3 whose epilogue adds it
    i, j = spec.index("layer1.0.conv3"), spec.index("layer1.0.downsample.0")
    spec[i], spec[j] = spec[j], spec[i]
    assert names == spec
    assert plan.ops[0]["kind"] == "input" and sum(op["kind"] == "fuse" for op in plan.ops) == 2 * 1 + 3 * 4 + 4 * 3
    n_down2 = sum(op["kind"] == "down2" for op in plan.ops)
    assert n_down2 == (13 if (H, W) == (256, 256) else 0)        # the LDS-staged stride-2 kernel where it takes the shape


@pytest.mark.parametrize("views,H,W", SHAPES)
def test_plan_geometry_of_every_producer_and_consumer(views, H, W):
    plan, specs = bb.HipPlan(views, H, W), _specs()
    for op in plan.ops:
        kind, out = op["kind"], op["out"]
        if kind == "input":
            assert out.geometry == (8, H, W, True)
            continue
        if kind == "fuse":
            terms = op["terms"]
            assert 2 <= len(terms) <= 4
            own = [k for k, (m, s) in enumerate(terms) if m.bordered]
            assert len(own) == 1 and terms[own[0]][1] == 0                       # the branch's own map, at its own position
            for k, (m, s) in enumerate(terms):
                assert (m.c, m.h, m.w) == (out.c, out.h >> s, out.w >> s) and (m.h << s, m.w << s) == (out.h, out.w)
                assert s == max(0, k - own[0])                                   # term j > i is branch j's map, 2^(j-i) coarser
            continue
        cout, cin, k, stride = specs[op["conv"]]
        x = op["in"]
        assert x.c == (8 if op["conv"] == "conv1" else cin) and out.c == cout and op["stride"] == stride
        assert (out.h, out.w) == (x.h // stride, x.w // stride) and (out.h * out.w) % 32 == 0 and x.c % 8 == 0
        assert kind == {1: "conv1", 3: "conv3"}[k] or (kind == "down2" and k == 3)
        if kind == "conv3":
            assert x.bordered                                                    # a 3x3 convolution reads a zero border
        if kind == "down2":
            assert not x.bordered and op["res"] is None and bb._down2_takes(cout, x.h, x.w)
        if op["res"] is not None:
            assert (op["res"].c, op["res"].h, op["res"].w) == (out.c, out.h, out.w)
    assert [(m.buf, m.c, m.h, m.w, m.bordered) for m in plan.outputs] == [
        (-1 - i, c, H >> (2 + i), W >> (2 + i), False) for i, c in enumerate(bb.WIDTHS)]


@pytest.mark.parametrize("views,H,W", SHAPES)
def test_plan_buffers_keep_one_shape_and_hold_what_is_read(views, H, W):
    """No buffer under two geometries; a launch never writes a buffer it reads; every read finds the value its producer
    wrote (nothing was recycled while still needed); strides address the buffer's own interior."""
    plan = bb.HipPlan(views, H, W)
    holds = {}
    for op in plan.ops:
        ins, out = _maps(op)
        for m in ins + [out]:
            if m.buf >= 0:
                assert plan.buffers[m.buf] == m.geometry
                n, c, hh, ww = plan.buffer_shape(m.buf)
                ns, cs, rs, off = m.strides
                assert (n, c) == (views, m.c) and ns == c * hh * ww and cs == hh * ww and rs == ww
                assert (hh, ww, off) == ((m.h + 2, m.w + 2, m.w + 3) if m.bordered else (m.h, m.w, 0))
                assert (m.h - 1) * rs + (m.w - 1) + off < cs
        for m in ins:
            assert holds.get(m.buf) == m.vid, (op.get("conv"), m.buf)
            assert m.buf != out.buf
        holds[out.buf] = out.vid
    assert len(set(plan.buffers)) < len(plan.buffers) <= 40                      # pooled: far fewer buffers than launches
    assert plan.nbytes() == sum(4 * torch.Size(plan.buffer_shape(b)).numel() for b in range(len(plan.buffers)))


def test_plan_footprint_at_256_views_is_the_documented_one():
    plan = bb.HipPlan(256, 256, 256)
    assert 6.5 * 2 ** 30 < plan.nbytes() < 6.9 * 2 ** 30 and "6.7 GiB" in bb.__doc__
    assert 300 <= len(plan.ops) <= 340 and "about 300" in bb.__doc__


# ---- the stem -----------------------------------------------------------------------------------------------------------
def test_conv1_is_padded_to_eight_input_channels():
    g = torch.Generator().manual_seed(3)
    w = torch.randint(-3, 4, (64, 3, 3, 3), generator=g).float()
    x = torch.randint(-4, 5, (2, 3, 16, 32), generator=g).float()
    wp = bb.stem_weight(w)
    assert tuple(wp.shape) == (64, 8, 3, 3) and torch.equal(wp[:, :3], w) and not wp[:, 3:].any()
    xp = torch.zeros(2, 8, 16, 32)
    xp[:, :3] = x
    assert torch.equal(F.conv2d(xp, wp, stride=2, padding=1), F.conv2d(x, w, stride=2, padding=1))   # small integers: exact
    assert bb.HipPlan.STEM_CIN == 8


# ---- C ABI --------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("poem_conv3x3_ex", "poem_conv1x1_packed_bytes", "poem_pack_conv1x1", "poem_conv1x1", "poem_hrnet_fuse")


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poem_hip.h")).read(), flags=re.S)
    L = hip.lib()
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in hip.SIGNATURES and hasattr(L, name)
    # the ctypes argument lists against the header's parameter counts
    for name in NEW_ENTRIES:
        params = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(hip.SIGNATURES[name][1]) == len(params.split(",")), name
    assert "poem_fuse_term_t" in hdr and [f[0] for f in hip.PoemFuseTerm._fields_] == [
        "data", "view_stride", "ch_stride", "row_stride", "offset", "shift"]
    import ctypes
    assert ctypes.sizeof(hip.PoemFuseTerm) == 32


def test_launcher_declarations_match_their_definitions():
    spec = importlib.util.spec_from_file_location("check_abi_decls", os.path.join(ROOT, "tools", "check_abi_decls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    decls, bad = mod.main()
    assert not bad, bad
    for name in ("poem_launch_conv3x3_ex", "poem_launch_conv1x1_nchw", "poem_launch_pack_conv1x1", "poem_launch_hrnet_fuse"):
        assert name in decls


def test_refusals_need_no_device():
    """argument checks come before any launch"""
    L = hip.lib()
    assert L.poem_conv1x1_packed_bytes(40, 12) == 0 and L.poem_conv1x1_packed_bytes(40, 64) == 2 * 8 * 64 * 16
    assert L.poem_pack_conv1x1(None, 40, 64, None, None) == -1
    assert L.poem_hrnet_fuse(None, 2, None, 0, 0, 0, 0, 1, 1, 1, 1, None) == -1


# ---- command line -------------------------------------------------------------------------------------------------------
def test_eval_single_backbone_engine_flag():
    spec = importlib.util.spec_from_file_location("eval_single_be", os.path.join(ROOT, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    base = ["--cfg", "c.yaml", "--dataset", "HO3D", "--view_min", "2", "--view_max", "3", "--model", "small", "-g", "0"]
    assert getattr(es.build_cli().parse_args(base), "backbone_engine", "torch") == "torch"       # what main() reads
    assert es.build_cli().parse_args(base + ["--backbone-engine", "torch"]).backbone_engine == "torch"
    assert es.build_cli().parse_args(base + ["--backbone-engine", "hip"]).backbone_engine == "hip"
    assert "backbone_engine" not in vars(es.build_parser().parse_args(base))       # the pinned surface stays as it is
    with pytest.raises(SystemExit):
        es.build_cli().parse_args(base + ["--backbone-engine", "miopen"])
