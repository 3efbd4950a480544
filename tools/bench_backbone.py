#!/usr/bin/env python
"""Backbone forward time on one GPU: ``--backbone hrnet`` (HRNet-W40, the default) | ``resnet18`` | ``resnet34`` | ``resnet50``
on ``--engine torch`` (PyTorch-ROCm / MIOpen) or ``--engine hip`` (the project's own convolution kernels, poem_v2_amd/backbone.py
and resnet.py).  Prints one JSON line per engine named: per-forward median / min / max over ``--steps`` timed forwards (device
events around each), images/s, and the fraction of the fp32 matrix peak from the FLOP count of the backbone's description at
this input size.  Several engines (``--engine torch hip torch``) run one after the other in this process, each on a model of its
own: an A/B/A of one session.  ``--miopen-ab``: the older A/B of the torch engine's memory format and MIOpen find mode."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import poem_v2_amd as pk  # noqa: E402,F401
from poem_v2_amd import resnet  # noqa: E402
from poem_v2_amd.backbone import Graph, HRNet, hrnet, seeded_hrnet_state_dict  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12


def conv_flops(graph, H, W):
    """multiply-adds x 2 of every convolution of a description, per view (the image's 3 channels, not the padded ones), and of
    a 7x7 stem alone"""
    total = stem = 0
    for n in graph.nodes:
        if n.op == "conv":
            flops = 2 * n.k * n.k * n.x.c * n.out.c * (H >> n.out.down) * (W >> n.out.down)
            total += flops
            stem += flops if n.k == 7 else 0
    return total, stem


def build(backbone, engine, dev):
    if backbone == "hrnet":
        return HRNet({"ENGINE": engine}, state_dict=seeded_hrnet_state_dict(0), device=dev)
    version = int(backbone[len("resnet"):])
    cls = {18: resnet.ResNet18, 34: resnet.ResNet34, 50: resnet.ResNet50}[version]
    return cls({"ENGINE": engine}, state_dict=resnet.seeded_resnet_state_dict(version, 0), device=dev)


def miopen_ab(views, dev):
    img = pk.inputs.synthetic_images(views, seed=1).to(dev)
    for fmt in ("contiguous", "channels_last"):
        for bench in (False, True):
            torch.backends.cudnn.benchmark = bench
            net = HRNet(state_dict=seeded_hrnet_state_dict(0), device=dev)
            x = img
            if fmt == "channels_last":
                x = img.contiguous(memory_format=torch.channels_last)
                for c in net._convs.values():
                    c.weight = c.weight.contiguous(memory_format=torch.channels_last)
            t0 = time.perf_counter()
            net(x)
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            net(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                ys = net(x)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / 3
            print(f"{fmt:14s} miopen-benchmark={bench!s:5s} first call {first:6.1f} s, steady {dt * 1e3:7.1f} ms / {views} images "
                  f"({views / dt:7.0f} img/s)  out0 {tuple(ys[0].shape)} {ys[0].is_contiguous()}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("views", type=int, nargs="?", default=256)
    ap.add_argument("--engine", choices=("torch", "hip"), nargs="+", default=["torch"])
    ap.add_argument("--backbone", choices=("hrnet", "resnet18", "resnet34", "resnet50"), default="hrnet")
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--miopen-ab", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.miopen_ab:
        return miopen_ab(a.views, dev)
    H, W = a.size
    img = (0.5 * torch.randn(a.views, 3, H, W, generator=torch.Generator().manual_seed(1))).to(dev)
    extra = {}
    graph = Graph(hrnet) if a.backbone == "hrnet" else Graph(resnet.resnet, int(a.backbone[len("resnet"):]))
    per_view, stem = conv_flops(graph, H, W)
    flops = per_view * a.views
    if stem:
        extra = {"stem_gflop": round(stem * a.views / 1e9, 2)}
    for engine in a.engine:
        net = build(a.backbone, engine, dev)
        for _ in range(a.warmup):
            ys = net(img)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ys = net(img)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        med = statistics.median(times)
        print(json.dumps({"backbone": a.backbone, "engine": engine, "views": a.views, "size": [H, W], "steps": a.steps,
                          "ms_median": round(med, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                          "images_per_s": round(a.views / med * 1e3, 1), "gflop_per_view": round(flops / a.views / 1e9, 2),
                          "tflops": round(flops / med / 1e9, 2),
                          "fp32_matrix_peak_fraction": round(flops / (med * 1e-3) / FP32_MATRIX_PEAK, 4),
                          "checksum": float(sum(y.double().abs().mean() for y in ys)), **extra}), flush=True)
        del net, ys
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
