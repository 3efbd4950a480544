"""Shared by tests/test_resnet_host.py and tests/test_resnet_hip.py.  TEST INFRASTRUCTURE -- NOT PRODUCT CODE.

A torch restatement of the non-HRNet branch of the reference model's decode stage (lib/models/POEM.py:168-181 ``feat_decode``,
:197-206 ``uv_decode``: the latter is the same code for every backbone, so oracle/decode_oracle.py's restatement serves) with
``ConvBlock`` = Conv2d -> BatchNorm2d(eval) -> ReLU, in the dtype of its inputs; PINNED by tests/golden/resnet_decode.npz, which
holds the reference model's own outputs.  Also: the seeded pyramids both test files and the fixture generator use, the torch
engine's forward in any dtype, and the criterion of tests/test_backbone_hip.py."""
import torch
import torch.nn.functional as F

import decode_oracle as do
from poem_v2_amd import resnet as rn
from poem_v2_amd.backbone import run_graph
from poem_v2_amd.decode import FEAT_SIZES
from poem_v2_amd.inputs import synthetic_resnet_pyramid

VERSIONS = (18, 34, 50)


def feat_decode(mlvl_feats, sd):
    """POEM.py:168-181: from the coarsest level, three [bilinear x2 | next finer level] -> ConvBlock, max_pool2d(2, 2), feat_in"""
    rev = list(reversed(mlvl_feats))
    x = rev[0]
    for i in range(3):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        x = torch.cat((x, rev[i + 1]), dim=1)
        x = do.conv_block(x, sd, f"feat_delayer.{i}")
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    return do.conv_block(x, sd, "feat_in", relu=False)


uv_decode = do.uv_decode
heatmap_stage = do.heatmap_stage


def synthetic_levels(backbone, views, h, w, seed):
    """seeded stand-ins for the four levels of an h x w image (h/4 x w/4 .. h/32 x w/32)"""
    return synthetic_resnet_pyramid(FEAT_SIZES[backbone], views, h, w, seed)


def cast_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def net_in(version, sd, dtype=torch.float32):
    """the torch engine on the CPU with its (fp32-rounded) folded weights held in ``dtype``"""
    net = {18: rn.ResNet18, 34: rn.ResNet34, 50: rn.ResNet50}[version](state_dict=sd)
    for c in net._convs.values():
        c.weight, c.bias = c.weight.to(dtype), c.bias.to(dtype)
    return net


def cpu_forward(net, x):
    """the torch engine's forward (backbone.run_graph) in the dtype of ``x`` (the class's own forward casts to fp32)"""
    return run_graph(net._graph, net._convs, x)


def criterion(got, ref64, ref32, what=""):
    """max|hip - fp64| <= 4 max|fp32_cpu - fp64| + 1e-6 max|fp64|   (tests/test_backbone_hip.py)"""
    err = float((got.double().cpu() - ref64).abs().max())
    scale = float((ref32.double() - ref64).abs().max())
    bound = 4.0 * scale + 1e-6 * float(ref64.abs().max())
    print(f"{what}: max|hip - fp64| = {err:.3e}   max|fp32 - fp64| = {scale:.3e}   bound = {bound:.3e}")
    assert err <= bound, (what, err, bound)
