#!/usr/bin/env python
"""Headline benchmark of the hot path: samples/s (multi-view frames) of POEM-medium, 8 views, batch 32 per GPU
(BASELINE.json configs[1]); one "step" = one poem_head_forward over one resident synthetic batch + the metric feed +
the 16-byte metric all-reduce.  Prints ONE JSON line on rank 0 (contract in the task statement / DESIGN.md).

  python bench.py                       # 1 GPU, default steps: the headline line only
  python bench.py --full                # + roofline, opt-in / A-B legs, extra configs, E2E scopes, CPU / eager baselines
  python bench.py --dump-outputs DIR    # + the last timed step's outputs as DIR/<name>.npy
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT,):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import poem_v2_amd as pk  # noqa: E402
from poem_v2_amd import dist as pdist  # noqa: E402
from poem_v2_amd.metrics import MeanEPE  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz
F16_MFMA_PEAK_TFLOPS = 2516.6   # v_mfma_f32_32x32x16_f16: 1024 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz (dense)


def vecattn_flops_per_launch(B, C, Q=799, K=32):
    """Algorithmic FLOPs of one fused vector-attention launch: per (query, neighbour) pair three CxC
    Linears (fc_delta.2, fc_gamma.0, fc_gamma.2) + the 3->C Linear = 6C^2 + 6C (QK(6C + 2C^2) + 4QKC^2)."""
    return float(B) * Q * K * (6.0 * C * C + 6.0 * C)


def executed_flops(C, views, Q=799, S=4096, K=32, in_ch=160, hw=256, nblocks=3, tables=True, parametric=False):
    """FLOPs one poem_head_forward EXECUTES for a batch with ``views`` views per sample (composed
    Linears, hoisted cross-attention projections, block-0 anchor tables, dead last feed-forward) -- the launch list of
    csrc/api.cpp priced at 2 FLOP per multiply-add.  c2 (medium, 32 x 8 views): 2.82 TFLOP."""
    B, BN = len(views), sum(views)
    f = BN * 2.0 * C * in_ch * hw                                  # input_proj
    f += BN * S * (2.0 * C * C + 2.0 * C * (C // 2))               # merge MLP 0 on the Q1 rows
    f += B * S * (2.0 * (C // 2) ** 2 + 2.0 * (C // 2) * C)        # merge MLP 1
    for i in range(nblocks):
        t0 = tables and i == 0
        dead = (i == nblocks - 1) and not parametric
        f += B * S * 2.0 * C * (4 * C if t0 else 6 * C) + (B * 32 * 2.0 * C * 2 * C if t0 else 0)     # F1 (basis-point side)
        f += (1 if t0 else B) * Q * 2.0 * C * 2 * C                                                      # F2
        f += B * (2 * 4.0 * Q * S * C + 3 * 2.0 * Q * C * C)                                             # two cross attentions
        f += B * Q * 2.0 * C * (C if t0 else 3 * C) + (B * 32 * 2.0 * C * 2 * C if t0 else 0)            # F3
        f += 2 * B * Q * K * ((2.0 * C * C) if t0 else (6.0 * C * C + 6.0 * C))                          # vector attentions
        f += 3 * B * Q * 2.0 * C * C                                                                     # fc2 x2, cross query
        f += B * Q * 2.0 * C * (C if dead else 5 * C) + B * Q * 2.0 * C * 3                              # F4 + reg_branch.2
        if not dead:
            f += B * Q * 2.0 * 4 * C * C                                                                 # feed-forward output
    # (the block-0 anchor tables are folded once at poem_create, like the positional table: not part of a step)
    return f


def as_written_flops(C, views, Q=799, S=4096, K=32, in_ch=160, hw=256, nblocks=3):
    """FLOPs of the path AS THE REFERENCE WRITES IT (SURVEY.md section 8d's per-sample formula + input_proj): un-hoisted
    vector cross attention (fc1 / w_k / w_v on the gathered (Q, 32, C) rows), un-composed Linears, per-sample block 0, the
    last block's feed-forward.  c2 (medium, 8 views): 132.5 GFLOP per sample.  The step's rate on THIS count divided by
    the rate on the executed count is the algebra's gain (hoist, anchor tables, composed Linears), held to parity."""
    f = 0.0
    for n in views:
        f += n * 2.0 * C * in_ch * hw + S * n * 3.0 * C * C + 1.5 * S * C * C
        blk = (2.0 * C * C * (Q + S) + 2 * (4.0 * C * C * Q + 4.0 * C * C * S + 4.0 * Q * S * C)
               + (10.0 * C * C * Q + Q * K * (6.0 * C + 2.0 * C * C) + 4.0 * Q * K * C * C)
               + (4.0 * C * C * Q + 6.0 * C * C * Q * K + Q * K * (6.0 * C + 2.0 * C * C) + 4.0 * Q * K * C * C)
               + 2.0 * C * C * Q + 16.0 * C * C * Q)
        f += nblocks * blk
    return f


def sampling_stage_bytes(C, views, S=4096, hw=256):
    """algorithmic HBM bytes of the sampling stage = read x (N C hw fp32 per sample) + write bps_feat (S C fp32)."""
    return float(sum(views)) * C * hw * 4 + float(len(views)) * S * C * 4


def baseline_config_name(model, views, views_range, batch, parametric):
    """Which BASELINE.json config this invocation's per-GPU load is (the metric is quoted on configs[1])."""
    if views_range:
        return "BASELINE.json configs[4] per-GPU load" if (model, tuple(views_range), batch) == ("medium", (2, 10), 64) else "custom ragged load"
    key = (model, views, batch)
    if key == ("medium", 8, 32):
        return "BASELINE.json configs[2] per-GPU load (medium_MANO tail)" if parametric else "BASELINE.json configs[1]"
    if key == ("medium_MANO", 8, 32):
        return "BASELINE.json configs[2] per-GPU load"
    if key == ("large", 10, 16):
        return "BASELINE.json configs[3]"
    if key == ("small", 2, 1):
        return "BASELINE.json configs[0] shape"
    return "custom load"


def make_leg(C, views, parametric, dev, rank, rotate, seed0=1000):
    """Head with seeded weights + ``rotate`` resident synthetic batches of the given per-sample view counts.
    -> (head, [(mlvl_feat, img_metas, reference_joints, gt_verts) on the device], the first batch on the host)."""
    head = pk.build_head(pk.configs.head_cfg(C, parametric=parametric, max_views=max(10, max(views))), data_preset=pk.CN({}))
    head.load_state_dict(pk.weights.seeded_state_dict(C, seed=0, parametric=parametric), strict=False)
    head.set_template(pk.inputs.synthetic_template(1234))
    if parametric:
        # config c3's tail: rot6d -> axis-angle -> MANO linear blend skinning, all on the device (csrc/mano.hip).  The MANO
        # assets are licence-gated: a seeded synthetic asset set of MANO's shapes stands in (same arithmetic, same cost)
        head.set_mano_layer(pk.ManoLayer(pk.mano.synthetic_mano_assets(0), center_idx=9, device=dev))
    head = head.to(dev).eval()
    out, first = [], None
    for i in range(rotate):
        b = pk.inputs.synthetic_batch(views, seed=seed0 + rank + 7919 * i)        # every rank its own shard of samples
        first = first or b
        metas = dict(b["img_metas"])
        metas["cam_intr"], metas["cam_extr"] = metas["cam_intr"].to(dev), metas["cam_extr"].to(dev)
        rj = b["reference_joints"].to(dev)
        g = torch.Generator().manual_seed(77 + rank + i)
        gt = (b["reference_joints"][:, 9:10] + 0.05 * torch.randn(len(views), 778, 3, generator=g)).to(dev)   # synthetic GT
        out.append((b["mlvl_feat"].to(dev), metas, rj, gt))
    return head, out, first


def time_leg(head, batches, steps, warmup):
    """Mean seconds per step of ``head`` cycling through ``batches`` (no metric feed: the extra-config legs)."""
    with torch.no_grad():
        for i in range(warmup):
            head(*batches[i % len(batches)][:3])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            head(*batches[i % len(batches)][:3])
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def draw_views(rule, B, rng, lo=2, hi=10):
    """Views per sample of one batch as the reference's data pipeline draws them: ``gauss`` = int(round(gauss(4, 2))) clipped
    to the view range (lib/data_wds/multiview_wds.py:86-95 upstream, random_n_views); ``uniform`` = U{lo..hi}."""
    if rule == "gauss":
        return [int(min(max(lo, int(round(rng.gauss(4, 2)))), hi)) for _ in range(B)]
    return [rng.randint(lo, hi) for _ in range(B)]


def make_stream(B, rule, n_layouts, dev, seed=0, lo=2, hi=10):
    """``n_layouts`` batches of B samples whose VIEW LAYOUT differs from batch to batch (what collation_random_n_views hands the
    head every step, lib/utils/collation.py:7-25 upstream), all resident on the device: features are prefixes of one resident
    pool of B * hi views, the cameras of every layout are uploaded up front.  -> [(mlvl_feat, img_metas, reference_joints)]"""
    import random
    rng = random.Random(1000 + seed)
    g = torch.Generator().manual_seed(4000 + seed)
    pool = torch.randn(B * hi, 160, 16, 16, generator=g).to(dev)
    rj = (torch.tensor([0.0, 0.0, 0.6]) + 0.03 * torch.randn(B, 21, 3, generator=g)).to(dev)
    K = torch.tensor([[300.0, 0, 128.0], [0, 300.0, 128.0], [0, 0, 1]])
    items, prev = [], None
    while len(items) < n_layouts:
        views = draw_views(rule, B, rng, lo, hi)
        if views == prev and hi > lo:      # every batch differs from the one before it (small batches cannot all be distinct)
            continue
        prev = views
        bn = sum(views)
        extr = torch.cat([pk.inputs.ring_extrinsics(n, ring=max(8, hi), jitter=0.05 * torch.randn(n, generator=g)) for n in views], 0)
        metas = {"inp_img_shape": (256, 256), "cam_intr": K[None].repeat(bn, 1, 1).contiguous().to(dev),
                 "cam_extr": extr.contiguous().to(dev), "master_id": [0] * B, "cam_view_num": np.asarray(views, dtype=np.int64)}
        items.append((pool[:bn], metas, rj))
    return items


def time_stream(head, items, steps, warmup, start=0):
    """Mean seconds per forward of ``head`` walking through ``items`` (a new item every forward)."""
    with torch.no_grad():
        for i in range(warmup):
            head(*items[(start + i) % len(items)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            head(*items[(start + warmup + i) % len(items)])
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def fresh_layout_scope(head, dev, B, rule, steps, warmup=6):
    """A stream of batches with a FRESH view layout every forward against the same head replaying ONE layout (the batch of the
    stream whose view total is closest to the stream's mean): the launch graph is keyed by the batch size, not by the layout
    (csrc/forward.cpp), so the two must agree."""
    items = make_stream(B, rule, steps + warmup, dev, seed=B)
    totals = [int(it[1]["cam_view_num"].sum()) for it in items]
    with torch.no_grad():
        head(*items[0])
    eng = head._engine
    g0 = eng.graph_stats()
    sec = time_stream(head, items, steps, warmup)
    g1 = eng.graph_stats()
    timed_mean = float(np.mean([totals[(warmup + i) % len(items)] for i in range(steps)]))
    k = int(np.argmin([abs(t - timed_mean) for t in totals]))
    fixed = time_stream(head, [items[k]], steps, warmup)
    return {"batch": B, "view_rule": "int(round(gauss(4,2))) clipped to 2..10 (multiview_wds.py:86-95)" if rule == "gauss" else "U{2..10} (SURVEY 8d c5)",
            "layouts_timed": steps, "distinct_layouts": len({tuple(it[1]["cam_view_num"].tolist()) for it in items}),
            "mean_views_per_batch": timed_mean,
            "fresh_layout": {"samples_per_s": B / sec, "ms_per_forward": sec * 1e3},
            "fixed_layout": {"samples_per_s": B / fixed, "ms_per_forward": fixed * 1e3, "views_in_batch": totals[k]},
            "fresh_over_fixed": fixed / sec,
            "graph_cache_delta": {k2: g1[k2] - g0[k2] for k2 in ("captures", "instantiations", "replays", "plain_forwards", "layout_uploads")},
            "graph_cache_after": {k2: g1[k2] for k2 in ("cached_execs", "parked_execs", "exec_reuses", "exec_update_refusals")}}


def time_leg_streams(head, batches, steps, warmup, nstreams=2):
    """Mean seconds per forward with consecutive forwards issued round-robin on ``nstreams`` torch streams: the head keeps
    one engine (workspace, layout arrays, side streams, launch graphs) per stream, so forward k + 1 does not wait for
    forward k and the two share the chip -- throughput of a small-batch evaluation loop, not the latency of a forward."""
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    torch.cuda.synchronize()
    with torch.no_grad():
        for i in range(warmup * nstreams):
            with torch.cuda.stream(streams[i % nstreams]):
                head(*batches[i % len(batches)][:3])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            with torch.cuda.stream(streams[i % nstreams]):
                head(*batches[i % len(batches)][:3])
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def self_launch(args):
    """``python bench.py --gpus N`` without a launcher: start the N ranks here (torch.distributed.run, one process per GPU,
    rendezvous on 127.0.0.1) instead of silently measuring one.  Refuses loudly when the box has fewer GPUs -- unless
    POEM_SINGLE_DEVICE=1 asks for the functional rehearsal (gloo, every rank on cuda:0; numbers are not scaling numbers)."""
    import subprocess
    ndev = torch.cuda.device_count()
    env = dict(os.environ)
    if ndev < args.gpus:
        if os.environ.get("POEM_SINGLE_DEVICE") != "1":
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {ndev} GPU(s) visible; refusing to report a {args.gpus}-GPU line from "
                             f"fewer devices (POEM_SINGLE_DEVICE=1 rehearses the N-rank code path on one GPU over gloo)")
        env.setdefault("POEM_DIST_BACKEND", "gloo")
    port = pdist.free_port()
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def physical_cores():
    """Physical cores visible to this process (SMT siblings counted once)."""
    try:
        allowed = os.sched_getaffinity(0)
        seen, phys, core, cpu = set(), None, None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("processor"):
                cpu = int(line.split(":")[1])
            elif line.startswith("physical id"):
                phys = int(line.split(":")[1])
            elif line.startswith("core id"):
                core = int(line.split(":")[1])
                if cpu in allowed:
                    seen.add((phys, core))
        return max(1, len(seen))
    except Exception:
        return os.cpu_count() or 1


def cpu_baseline(model_embed, batch, n_samples):
    """The oracle (CPU restatement, as-written arithmetic incl. the un-hoisted cross attention) timed on the host
    cores on the first ``n_samples`` samples of the very batch the GPU processed -- the CHECKER used as a reported
    baseline, never as the thing measured on the GPU."""
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import poem_oracle as po
    from util import oracle_consts
    cfg = po.PathConfig(embed=model_embed)
    w = pk.weights.seeded_state_dict(model_embed, seed=0)
    consts = oracle_consts(4096)
    m = batch["img_metas"]
    views = [int(v) for v in m["cam_view_num"]]

    def run(lo, hi):
        a, b = int(np.sum(views[:lo])), int(np.sum(views[:hi]))
        with torch.no_grad():
            return po.head_forward(w, cfg, consts, batch["mlvl_feat"][a:b], m["cam_intr"][a:b], m["cam_extr"][a:b],
                                   views[lo:hi], batch["reference_joints"][lo:hi],
                                   inp_img_shape=m["inp_img_shape"])["all_coords_preds"]

    # pick the thread count the host runs this workload fastest with (1 sample each), then time the bounded sample
    phys = physical_cores()
    best_t, best_dt = phys, None
    for t in sorted({min(phys, c) for c in (16, 32, 64, phys)}):
        torch.set_num_threads(t)
        t0 = time.perf_counter()
        run(len(views) - 1, len(views))
        d = time.perf_counter() - t0
        if best_dt is None or d < best_dt:
            best_t, best_dt = t, d
    # the reference scripts pin OMP/MKL to one thread (scripts/eval.py:110-114 upstream): quote that setting too
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    run(len(views) - 1, len(views))
    one_thread = 1.0 / (time.perf_counter() - t0)
    torch.set_num_threads(best_t)
    t0 = time.perf_counter()
    out = run(0, n_samples)
    dt = time.perf_counter() - t0
    return {"value": n_samples / dt, "unit": "samples/s", "cores": best_t, "threads": best_t, "host_physical_cores": phys,
            "kind": "port", "one_thread_value": one_thread,
            "sample": f"first {n_samples} samples of the GPU's own batch (POEM-medium, {views[0]} views), one pass in "
                      f"{dt:.1f} s, torch CPU fp32, {best_t} threads (fastest of 16/32/64/{phys} on this host, "
                      f"{phys} physical cores)"}, out


def cpu_baseline_e2e(model_embed, batch, n_samples, threads, pyr_dev=None):
    """SURVEY 8d asks for the CPU baseline in BOTH timing scopes: this is the E2E one -- 256x256 images -> HRNet-W40 (plain
    PyTorch on the host cores, the backbone pinned to the reference's by tests/golden/backbone.npz) -> feat_decode + heat maps
    (oracle/decode_oracle.py) -> DLT (oracle/dlt_oracle.py) -> head (oracle/poem_oracle.py), on the first ``n_samples`` samples
    of the batch the GPU's E2E leg processed, same seeds.  The CHECKER used as a reported baseline."""
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import decode_oracle as do
    import dlt_oracle as dl
    import poem_oracle as po
    from util import oracle_consts
    from poem_v2_amd.backbone import HRNet, seeded_hrnet_state_dict
    m = batch["img_metas"]
    views = [int(v) for v in m["cam_view_num"]][:n_samples]
    nv = int(np.sum(views))
    torch.set_num_threads(threads)
    net = HRNet(state_dict=seeded_hrnet_state_dict(0), device="cpu")
    sd = pk.weights.seeded_decoder_state_dict(0)
    img = pk.inputs.synthetic_images(int(np.sum(m["cam_view_num"])), seed=1)[:nv]
    K, E, rj = m["cam_intr"][:nv], m["cam_extr"][:nv], batch["reference_joints"][:n_samples]
    vs = torch.repeat_interleave(torch.arange(n_samples), torch.tensor(views))
    T = torch.linalg.inv(E)
    pc = (T[:, None, :3, :3] @ rj[vs][..., None]).squeeze(-1) + T[:, None, :3, 3]
    q2 = (K[:, None] @ pc[..., None]).squeeze(-1)
    uv_true = q2[..., :2] / q2[..., 2:]
    cfg, w, consts = po.PathConfig(embed=model_embed), pk.weights.seeded_state_dict(model_embed, seed=0), oracle_consts(4096)
    t0 = time.perf_counter()
    with torch.no_grad():
        pyr = net(img)
        tb = time.perf_counter() - t0
        f160 = do.feat_decode(pyr, sd)
        uv = do.heatmap_stage(pyr, sd, 256, 256)
        uvb = uv_true + 1e-3 * (uv - uv.mean(dim=1, keepdim=True))
        rjp = dl.triangulate_reference_joints(uvb, K, E, views)
        out = po.head_forward(w, cfg, consts, f160, K, E, views, rjp, inp_img_shape=m["inp_img_shape"])["all_coords_preds"]
    dt = time.perf_counter() - t0
    staged = None
    if pyr_dev is not None:
        # Attribution of the E2E distance, stage by stage, each stage's restatement fed with the DEVICE's own input to that stage
        # (what tests/test_backbone.py asserts): the two chains differ by their BACKBONES (MIOpen's fp32 convolutions vs
        # PyTorch's CPU ones) and every later stage inherits and, with seeded random weights, amplifies that difference.
        kd = {k: (v[:nv] if k != "rjp" else v[:n_samples]).float().cpu() for k, v in pyr_dev.items() if k != "pyr"}
        pd = [y[:nv].float().cpu() for y in pyr_dev["pyr"]]
        rel = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(pd, pyr)]
        with torch.no_grad():
            f160d = do.feat_decode(pd, sd)
            uvd = do.heatmap_stage(pd, sd, 256, 256)
            rjd = dl.triangulate_reference_joints(kd["uvb"], K, E, views)
            head_d = po.head_forward(w, cfg, consts, kd["f160"], K, E, views, kd["rjp"], inp_img_shape=m["inp_img_shape"])["all_coords_preds"]
            chain_d = po.head_forward(w, cfg, consts, f160d, K, E, views,
                                      dl.triangulate_reference_joints(uv_true + 1e-3 * (uvd - uvd.mean(dim=1, keepdim=True)), K, E, views),
                                      inp_img_shape=m["inp_img_shape"])["all_coords_preds"]
            # conditioning of the head on THIS input: the same CPU restatement with its feature input perturbed at fp32
            # round-off level (relative 1e-7, seeded)
            gq = torch.Generator().manual_seed(9)
            head_p = po.head_forward(w, cfg, consts, kd["f160"] * (1.0 + 1e-7 * torch.randn(kd["f160"].shape, generator=gq)), K, E, views,
                                     kd["rjp"], inp_img_shape=m["inp_img_shape"])["all_coords_preds"]
        staged = {"head_on_device_inputs": head_d, "cpu_chain_on_device_pyramid": chain_d, "head_on_perturbed_inputs": head_p,
                  "feat_absmax": float(kd["f160"].abs().max()), "feat_std": float(kd["f160"].std()),
                  "mesh_extent_m": float((head_d[-1] - kd["rjp"][:, 9:10]).abs().max()),
                  "backbone_max_rel_diff_by_level": rel,
                  "feat_decode_max_rel_diff": float((kd["f160"] - f160d).abs().max() / f160d.abs().max()),
                  "heatmap_uv_max_abs_diff_px": float((kd["uv"] - uvd).abs().max()),
                  "dlt_joints_max_abs_diff_m": float((kd["rjp"] - rjd).abs().max())}
    return {"value": n_samples / dt, "unit": "samples/s", "cores": threads, "kind": "port", "backbone_s": tb,
            "sample": f"first {n_samples} sample(s) x {views[0]} views of the E2E leg's batch: images -> HRNet-W40 (PyTorch CPU fp32) -> "
                      f"feat_decode / heat maps -> DLT -> head restatement, one pass in {dt:.1f} s, {threads} threads"}, out, staged


def eager_baseline(model_embed, batch, n_samples, dev):
    """BASELINE.json configs[1] names a "PyTorch-ROCm baseline": the same restatement (the oracle) run eagerly on the
    GPU through PyTorch-ROCm's own kernels, on the same bounded sample as the CPU leg.  Reported, never shipped."""
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import poem_oracle as po
    from util import oracle_consts
    cfg = po.PathConfig(embed=model_embed)
    w = {k: v.to(dev) for k, v in pk.weights.seeded_state_dict(model_embed, seed=0).items()}
    consts = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in oracle_consts(4096).items()}
    m = batch["img_metas"]
    views = [int(v) for v in m["cam_view_num"]][:n_samples]
    bn = int(np.sum(views))
    args = (batch["mlvl_feat"][:bn].to(dev), m["cam_intr"][:bn].to(dev), m["cam_extr"][:bn].to(dev), views,
            batch["reference_joints"][:n_samples].to(dev))

    def run():
        with torch.no_grad():
            return po.head_forward(w, cfg, consts, *args, inp_img_shape=m["inp_img_shape"])["all_coords_preds"]

    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    return {"value": n_samples / dt, "unit": "samples/s", "kind": "port on PyTorch-ROCm eager (same GPU)",
            "sample": f"{n_samples} samples x {views[0]} views per pass, mean of {reps} passes"}


def slice_batch(b, lo, hi):
    """Samples [lo, hi) of a host batch of pk.inputs.synthetic_batch (views are stored sample after sample)."""
    views = np.asarray(b["img_metas"]["cam_view_num"], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(views)])
    v0, v1 = int(off[lo]), int(off[hi])
    metas = dict(b["img_metas"])
    metas["cam_intr"], metas["cam_extr"] = metas["cam_intr"][v0:v1].contiguous(), metas["cam_extr"][v0:v1].contiguous()
    metas["cam_view_num"], metas["master_id"] = views[lo:hi].copy(), [0] * (hi - lo)
    return b["mlvl_feat"][v0:v1].contiguous(), metas, b["reference_joints"][lo:hi].contiguous()


def to_dev(item, dev):
    f, m, r = item
    m = dict(m)
    m["cam_intr"], m["cam_extr"] = m["cam_intr"].to(dev), m["cam_extr"].to(dev)
    return f.to(dev), m, r.to(dev)


DUMP_LIMIT_BYTES = 60 << 20     # --dump-outputs stays under 64 MB in all


def dump_outputs(path, arrays):
    """``--dump-outputs``: each host tensor of ``arrays`` (name -> tensor) as ``path/<name>.npy`` in float32.  Outputs larger
    than DUMP_LIMIT_BYTES in all are written as a fixed, seeded sample of each flattened array (the same elements every run)."""
    os.makedirs(path, exist_ok=True)
    total = sum(t.numel() * 4 for t in arrays.values())
    for name, t in arrays.items():
        a = t.numpy().astype(np.float32, copy=False)
        if total > DUMP_LIMIT_BYTES:
            idx = np.random.RandomState(0).choice(a.size, size=max(1, a.size * DUMP_LIMIT_BYTES // total), replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(path, name + ".npy"), a)


def c5_global_leg(head, C, dev, rank, world, ksteps, rotate=3):
    """One GLOBAL ragged batch of 64 samples per step (views ~ U{2..10}, seed 5), the same on every rank, cut into contiguous
    sample ranges by dist.shard_by_views; each rank runs its shard, the step time is the slowest rank's.  Then the claim the
    sharding rests on is checked ACROSS processes: the shards' meshes, put together with the path's only collective (an
    all-reduce(sum) into a zero-padded (3,64,799,3) buffer: x + 0 is exact), are compared bit for bit with rank 0 running the
    whole batch of 64 in one forward (no kernel's arithmetic depends on the batch a sample runs in)."""
    views_g = np.random.RandomState(5).randint(2, 11, size=64)
    lo, hi = pdist.shard_by_views(views_g, rank, world)
    counts = torch.zeros(2 * world, dtype=torch.float64, device=dev)
    counts[rank], counts[world + rank] = hi - lo, float(views_g[lo:hi].sum())
    pdist.all_reduce_sum_(counts)
    globals_ = [pk.inputs.synthetic_batch(views_g.tolist(), seed=5000 + 7919 * i) for i in range(rotate)]   # rank-independent
    mine = [to_dev(slice_batch(g, lo, hi), dev) for g in globals_] if hi > lo else []
    with torch.no_grad():
        for i in range(3):
            if mine:
                head(*mine[i % len(mine)])
        pdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(ksteps):
            if mine:
                head(*mine[i % len(mine)])
        torch.cuda.synchronize()
        pdist.barrier()
        gdt = time.perf_counter() - t0
        tg = torch.tensor([gdt], dtype=torch.float64, device=dev)
        pdist.all_reduce_max_(tg)
        joined = torch.zeros(3, 64, 799, 3, dtype=torch.float32, device=dev)
        if mine:
            joined[:, lo:hi] = head(*mine[0])["all_coords_preds"]
        pdist.all_reduce_sum_(joined)
        out = {"value": 64 * ksteps / float(tg.item()), "unit": "samples/s", "ms_per_step": float(tg.item()) / ksteps * 1e3,
               "scaling": "strong", "samples_by_rank": [int(v) for v in counts[:world].tolist()],
               "views_by_rank": [int(v) for v in counts[world:].tolist()],
               "note": "one global batch of 64 ragged samples per step, dist.shard_by_views; max over ranks"}
        if rank == 0:
            whole = head(*to_dev(slice_batch(globals_[0], 0, 64), dev))["all_coords_preds"]
            out["sharded_bit_equal_to_single_process"] = bool(torch.equal(whole, joined))
            out["sharded_max_abs_diff_m"] = float((whole - joined).abs().max())
            del whole
        del joined, mine
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="samples per GPU (weak scaling)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--views-range", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                    help="ragged batch: views per sample ~ U{LO..HI}, seed 5 (BASELINE configs[4]: --views-range 2 10 --batch 64)")
    ap.add_argument("--model", default="medium", choices=list(pk.weights.MODEL_EMBED))
    ap.add_argument("--cpu-samples", type=int, default=4, help="0 disables the CPU baseline leg")
    ap.add_argument("--parametric", action="store_true",
                    help="medium_MANO-style parametric tail (BASELINE configs[2]); MANO itself is licence-gated, the bench "
                         "plugs a cheap device-side stand-in layer in its place")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end scope leg (images -> HRNet on PyTorch-ROCm -> verts)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "split_f16x3", "split_f16x3_all"],
                    help="fp32 (default, exact fp32 matrix-core products) | split_f16x3 (opt-in hi/lo f16 split of the vector "
                         "attention's C x C GEMMs; include/poem_hip.h)")
    ap.add_argument("--overlap", type=int, default=1, help="0: issue every kernel on one stream (A/B of the side streams)")
    ap.add_argument("--anchor-tables", type=int, default=1,
                    help="0: block 0's vector attentions in the per-sample form (A/B of poem_set_anchor_tables)")
    ap.add_argument("--chains", type=int, default=1,
                    help="0: one launch per query-side operator instead of the row-tile chain kernels (A/B of poem_set_chains)")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="poem_set_option switches for A/B runs, e.g. --option knn_early=0")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="skip the short legs for the other BASELINE per-GPU loads (c3 medium_MANO, c4 large x 10 views x 16, "
                         "c5 ragged 2-10 views x 64)")
    ap.add_argument("--headline-only", action="store_true",
                    help="with --full: the headline leg and its roofline events leg only (no opt-in / A-B / extra-config / pyramid / "
                         "E2E / input / CPU / eager legs)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: roofline events leg, scaling diagnostics, opt-in precision and A/B legs, "
                         "extra configs, pyramid / E2E / input scopes, CPU and eager baselines, the c5 global batch.  Off: the run "
                         "sets up, warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path returned in its last timed step as DIR/<name>.npy (float32), rank 0")
    ap.add_argument("--rotate", type=int, default=8, help="resident input batches cycled through the steps (>= 8 x 42 MB of "
                    "features outruns the 256 MB Infinity Cache, so the sampling front end is timed cold)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    legs = args.full and not args.headline_only     # the measurements beside the headline (--full)
    if not legs:
        args.no_e2e = args.no_extra_configs = True
        args.cpu_samples = 0
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)

    # POEM_DIST_BACKEND=gloo + POEM_SINGLE_DEVICE=1: rehearse the N-rank code path on a 1-GPU box (all ranks share cuda:0;
    # RCCL itself refuses two ranks on one device).  The driver's real runs use the default: nccl == RCCL, one GPU per rank.
    rank, local_rank, world = pdist.init_from_env(os.environ.get("POEM_DIST_BACKEND"))
    if os.environ.get("POEM_SINGLE_DEVICE") == "1":
        local_rank = 0
    if world != args.gpus:
        raise SystemExit(f"bench.py: WORLD_SIZE={world} does not match --gpus {args.gpus}")
    grouped = pdist.active()      # a process group exists: N > 1, or a one-rank group forced by POEM_DIST_FORCE_INIT=1
    assert torch.cuda.is_available(), "bench.py needs a GPU (the product path has no CPU fallback)"
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    C = pk.weights.MODEL_EMBED[args.model]
    views = [args.views] * args.batch
    if args.views_range:
        views = np.random.RandomState(5 + rank).randint(args.views_range[0], args.views_range[1] + 1, size=args.batch).tolist()
    parametric = bool(args.parametric or args.model == "medium_MANO")
    spec = dict(embed=C, nsample=4096, views=views, seed=0, parametric=parametric)
    head, batches, batch = make_leg(C, views, parametric, dev, rank, max(1, args.rotate))
    feat, metas, rj, gt_verts = batches[0]
    meter = MeanEPE("verts", device=dev)
    turn = [0]

    def step(which=None):
        """One pass of the hot path over one resident batch (the steps cycle through ``--rotate`` different batches; legs
        that compare outputs pass ``which=0``) + the metric feed + the path's only collective."""
        f_, m_, r_, g_ = batches[(turn[0] if which is None else which) % len(batches)]
        turn[0] += which is None
        preds = head(f_, m_, r_)
        meter.feed(preds["all_coords_preds"][-1, :, 21:], g_)
        meter.reduce()                                   # 16 B all-reduce (RCCL)
        return preds

    with torch.no_grad():
        for _ in range(args.warmup):
            step()
        eng = head._engine
        if args.precision != "fp32":
            head.set_precision(args.precision)
            for _ in range(args.warmup):
                step()
        if not args.anchor_tables:
            head.set_anchor_tables(False)
            for _ in range(args.warmup):
                step()
        for kv in args.option:
            k_, v_ = kv.split("=")
            eng.set_option(k_, int(v_))
        if args.option:
            for _ in range(args.warmup):
                step()
        if not args.chains:
            head.set_chains(False)
            for _ in range(args.warmup):
                step()
        if not args.overlap:
            eng.set_overlap(False)
            for _ in range(args.warmup):
                step()
        # The timed region runs the path exactly as it ships: launch-graph replay on, the library's HIP-event profile OFF (the
        # profile needs plain launches).  One torch event per step boundary on the launch stream (no host sync) gives the
        # per-step durations whose MEDIAN is reported beside the mean.
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        meter.reset()
        pdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(args.steps):
            preds = step()
            marks[i + 1].record()
        torch.cuda.synchronize()
        pdist.barrier()
        dt = time.perf_counter() - t0
        step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
        graph_stats = eng.graph_stats()
        mpvpe_timed = meter.result() * 1e3
        if args.dump_outputs and rank == 0:
            # copied now: the returned tensors live in the engine's buffers, which later forwards overwrite
            dump_outputs(args.dump_outputs, {k: v.detach().float().cpu() for k, v in preds.items()})
        if args.full:
            # separate short leg for the roofline: the same steps with the library's HIP events around the dominant kernel and
            # the sampling stage (plain launches, ~130 event records per step -- which is why it is not the timed region)
            ev_steps = max(2, min(args.steps, 6))
            eng.profile_enable(8 * ev_steps)
            for _ in range(ev_steps):
                step()
            torch.cuda.synchronize()
    dt_rank = dt
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    pdist.all_reduce_max_(tmax)
    dt = float(tmax.item())
    scale_diag = None
    if grouped and args.full:
        # what a reader of the scaling curve needs beside `value`: every rank's own step time (min / max / spread) and the
        # latency of the path's only collective (the 16-byte all-reduce of the metric sums), measured alone
        per = torch.zeros(world, dtype=torch.float64, device=dev)
        per[rank] = dt_rank / args.steps * 1e3
        pdist.all_reduce_sum_(per)
        probe = torch.zeros(2, dtype=torch.float64, device=dev)
        for _ in range(5):
            pdist.all_reduce_sum_(probe)
        torch.cuda.synchronize()
        pdist.barrier()
        t0 = time.perf_counter()
        for _ in range(50):
            pdist.all_reduce_sum_(probe)
        torch.cuda.synchronize()
        ar_us = (time.perf_counter() - t0) / 50 * 1e6
        scale_diag = {"ms_per_step_by_rank": [round(float(v), 4) for v in per.tolist()], "ms_per_step_min": float(per.min()),
                      "ms_per_step_max": float(per.max()), "allreduce_16B_latency_us": ar_us,
                      "note": "per-rank wall time of the timed region / steps (rank-local clocks, same barrier-bracketed region); "
                              "the all-reduce is timed alone, back to back, 50 calls"}
    n_fe = n_anch = n_launch = 0
    if args.full:
        n_fe, fe_ms = eng.profile_read_stage(2)            # the sampling front end (input_proj .. merge finalize), per forward
        n_anch, anch_ms = eng.profile_read_anchored()      # block 0's table form (one C x C GEMM per neighbour column)
        n_launch, va_ms = eng.profile_read()               # the full fused kernel (blocks 1, 2)
        eng.profile_enable(0)

    total_samples = args.batch * world * args.steps
    value = total_samples / dt
    res = {
        "metric": "samples/sec (multi-view frames) POEM-medium 8-view" if (args.model, args.views, args.views_range) == ("medium", 8, None)
        else f"samples/sec (multi-view frames) POEM-{args.model} " +
             (f"{args.views_range[0]}-{args.views_range[1]} views (ragged)" if args.views_range else f"{args.views}-view"),
        "value": value, "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "ms_per_step_median": step_ms[len(step_ms) // 2] if len(step_ms) % 2 else
        0.5 * (step_ms[len(step_ms) // 2 - 1] + step_ms[len(step_ms) // 2]),
        "ms_per_step_min": step_ms[0], "ms_per_step_max": step_ms[-1],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{baseline_config_name(args.model, args.views, args.views_range, args.batch, parametric)}: POEM-{args.model} head "
                               f"(POEM_Generalized_Head + PtEmbedTRv4), {('ragged ' + str(args.views_range)) if args.views_range else args.views} views, "
                               f"160x16x16 backbone features (256x256 input), batch {args.batch} per GPU, seeded weights, "
                               f"{len(batches)} input batches resident in HBM and cycled (features: {len(batches) * feat.numel() * 4 / 1e6:.0f} MB)",
                   "batch_per_gpu": args.batch, "views": args.views if not args.views_range else list(args.views_range), "embed": C,
                   "parallelism": f"dp{world}", "ranks_joined": world,
                   "process_group": (f"{torch.distributed.get_backend()} world_size={torch.distributed.get_world_size()}"
                                     if grouped else "single process")},
    }
    # whole step against the fp32 matrix pipe: FLOPs the launch list executes (not the as-written count) / step time
    ex = executed_flops(C, views, tables=bool(args.anchor_tables) and args.precision == "fp32", parametric=parametric)
    aw = as_written_flops(C, views)
    res["whole_step"] = {"executed_TFLOP_per_step": ex / 1e12, "executed_TFLOPs": ex / (dt / args.steps) / 1e12,
                         "frac_of_fp32_matrix_peak": ex / (dt / args.steps) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                         "as_written_TFLOP_per_step": aw / 1e12, "as_written_TFLOPs": aw / (dt / args.steps) / 1e12,
                         "algorithmic_efficiency": aw / ex,
                         "as_written_frac_of_fp32_matrix_peak": aw / (dt / args.steps) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                         "note": "per GPU; executed = 2 FLOP per multiply-add of every GEMM-shaped launch of csrc/api.cpp's "
                                 "sequence; as_written = SURVEY 8d's count of the reference's own arithmetic (un-hoisted cross "
                                 "attention, per-sample block 0, un-composed Linears): a rate above the pipe's peak on that count is "
                                 "algebra held to parity, not skipped work"}
    if n_fe > 0:
        fe_s = fe_ms / n_fe * 1e-3
        sb = sampling_stage_bytes(C, views)
        res["sampling_stage"] = {"span": "input_proj -> projection -> bilinear sampling -> merge MLPs -> bps_feat (HIP events)",
                                 "avg_ms": fe_ms / n_fe, "forwards_timed": n_fe, "share_of_step": (fe_ms / n_fe) / (dt / args.steps * 1e3),
                                 "algorithmic_bytes": sb, "GBps_algorithmic": sb / fe_s / 1e9,
                                 "hbm_frac_of_8TBps": sb / fe_s / 8e12,
                                 "executed_TFLOPs": (sum(views) * 4096 * 3.0 * C * C + len(views) * 4096 * 1.5 * C * C
                                                     + sum(views) * 2.0 * C * 160 * 256) / fe_s / 1e12,
                                 "note": "the stage is bound by the merge MLP's fp32 matrix work (SURVEY 8d), not by HBM: the GB/s "
                                         "figure shows how far the algorithmic bytes are from being the limiter"}
    if n_launch > 0:
        avg_s = va_ms / n_launch * 1e-3
        ach = vecattn_flops_per_launch(args.batch, C) / avg_s / 1e12
        # HBM bytes per launch from the committed PMC passes (tools/collect_profiles.sh; FETCH_SIZE x2 correction applied
        # by tools/pmc_summary.py) -- the counters need their own rocprofv3 runs, so the newest profile on disk is quoted
        traffic = None
        import glob
        for pmc in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json")), reverse=True):
            try:
                ks = json.load(open(pmc))["kernels"]
                # the full fused kernel (MODE 0), not the table builder / anchored form of block 0 (MODE 1 / 2)
                va = [v for k, v in ks.items() if k.startswith("vecattn_kernel") and "hbm_bytes_per_launch" in v
                      and not k.rstrip().endswith((", 1>", ", 2>"))]
                if va:
                    traffic = va[0]["hbm_bytes_per_launch"]
                    break
            except Exception:
                continue
        res["roofline"] = {"kernel": "vecattn_kernel (fused vector attention)", "bound": "mfma", "achieved": ach,
                           "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / FP32_MFMA_PEAK_TFLOPS,
                           "traffic": traffic,
                           "traffic_source": (f"quoted from {os.path.relpath(pmc, ROOT)}: separate rocprofv3 --pmc passes of this "
                                              "command (tools/collect_profiles.sh), NOT measured in the run that printed this line")
                           if traffic is not None else None,
                           "launches_timed": n_launch, "avg_launch_ms": va_ms / n_launch,
                           "share_of_step": (va_ms / ev_steps) / (dt / args.steps * 1e3)}
        if n_anch > 0:
            res["roofline"]["anchored_block0"] = {
                "kernel": "vecattn_kernel MODE 2 (block 0: positional products from the per-forward anchor tables)",
                "launches_timed": n_anch, "avg_launch_ms": anch_ms / n_anch, "share_of_step": (anch_ms / ev_steps) / (dt / args.steps * 1e3),
                "as_written_TFLOPs": vecattn_flops_per_launch(args.batch, C) / (anch_ms / n_anch * 1e-3) / 1e12,
                "executed_TFLOPs": vecattn_flops_per_launch(args.batch, C) / 3.0 / (anch_ms / n_anch * 1e-3) / 1e12,
                "note": "not part of `achieved`: a third of the as-written products are executed per sample"}
    if scale_diag is not None:
        res["scaling_diagnostics"] = scale_diag
    res["mpvpe_synthetic_gt_mm"] = mpvpe_timed
    res["timed_region"] = {"launch_graph_replays": graph_stats["replays"], "plain_launch_forwards": graph_stats["plain_forwards"],
                           "graph_captures": graph_stats["captures"], "view_layout_uploads": graph_stats["layout_uploads"],
                           "note": "counters of the head since its creation (warm-up included): the timed steps replay the launch graph; "
                                   "`ms_per_step` = wall time of the region / steps (value's basis), `ms_per_step_median` = median of the "
                                   "per-step GPU durations between events recorded on the launch stream"}
    if "roofline" in res:
        res["roofline"]["events_leg"] = (f"{ev_steps} steps right after the timed region with the library's HIP events on the launch stream "
                                         "(plain launches); the timed region itself runs without them")
    if args.precision != "fp32":
        res["dtype"] = "f32 (vector-attention C x C products as hi/lo f16 splits on the f16 matrix cores, fp32 accumulation)"
        if "roofline" in res:
            res["roofline"].update(kernel="vecattn_split_kernel", peak=F16_MFMA_PEAK_TFLOPS / 3.0,
                                   frac=res["roofline"]["achieved"] / (F16_MFMA_PEAK_TFLOPS / 3.0), traffic=None,
                                   note="peak = dense f16 MFMA peak / 3 (three MFMAs per fp32-equivalent product)")
    elif C >= 128 and not parametric and world == 1 and legs:
        # OPT-IN split-precision leg, reported beside the headline (never as `value`): same step with
        # poem_set_precision(SPLIT_F16X3); distance of its vertices from the fp32 path's on the same batch.
        try:
            with torch.no_grad():
                exact = step(0)["all_coords_preds"].clone()
                head.set_precision("split_f16x3")
                for _ in range(2):
                    got = step(0)["all_coords_preds"]
                eng.profile_enable(6 * args.steps)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                sdt = (time.perf_counter() - t0) / args.steps
                n_s, ms_s = eng.profile_read(reset=True)
                eng.profile_enable(0)
                head.set_precision("split_f16x3_all")
                for _ in range(2):
                    got_all = step(0)["all_coords_preds"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                adt = (time.perf_counter() - t0) / args.steps
                head.set_precision("fp32")
            res["split_f16x3_all_scope"] = {
                "value": args.batch * world / adt, "unit": "samples/s", "ms_per_step": adt * 1e3,
                "mpvpe_vs_fp32_path_mm": float(torch.norm(got_all[-1, :, 21:] - exact[-1, :, 21:], dim=-1).mean()) * 1e3,
                "note": "opt-in POEM_PRECISION_SPLIT_F16X3_ALL: the same hi/lo f16 scheme also in every panel GEMM (all Linears "
                        "but the K = 4C one) and in the two contractions of the cross attention (K / V images written as "
                        "hi | lo f16 by the projection GEMM); softmaxes, LayerNorms, sampling, neighbour searches: fp32"}
            d = float(torch.norm(got[-1, :, 21:] - exact[-1, :, 21:], dim=-1).mean()) * 1e3
            res["split_f16x3_scope"] = {"value": args.batch * world / sdt, "unit": "samples/s", "ms_per_step": sdt * 1e3,
                                        "mpvpe_vs_fp32_path_mm": d,
                                        "vecattn_split_avg_launch_ms": (ms_s / n_s) if n_s else None,
                                        "note": "opt-in poem_set_precision(POEM_PRECISION_SPLIT_F16X3): the vector attention's "
                                                "three C x C GEMMs as w_hi x_hi + w_hi x_lo + w_lo x_hi on v_mfma_f32_32x32x16_f16; "
                                                "everything else fp32; the headline `value` is the exact-fp32 default"}
        except Exception as e:
            res["split_f16x3_scope"] = {"error": repr(e)[:200]}
    if world == 1 and args.precision == "fp32" and args.anchor_tables and legs:
        # the same step with block 0's positional products evaluated per sample, term by term as the reference does
        # (poem_set_anchor_tables(0)): what the anchor tables buy, and how far the two forms are apart on this batch
        try:
            with torch.no_grad():
                tab = step(0)["all_coords_preds"].clone()
                head.set_anchor_tables(False)
                for _ in range(2):
                    per = step(0)["all_coords_preds"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                pdt = (time.perf_counter() - t0) / args.steps
                head.set_anchor_tables(True)
            res["per_sample_block0_scope"] = {
                "value": args.batch * world / pdt, "unit": "samples/s", "ms_per_step": pdt * 1e3,
                "mpvpe_vs_headline_path_mm": float(torch.norm(per[-1, :, 21:] - tab[-1, :, 21:], dim=-1).mean()) * 1e3,
                "note": "poem_set_anchor_tables(0): the first block's vector attentions evaluate fc_delta / fc_gamma.0's "
                        "positional term per (sample, query, anchor) from ((c + t) - c)/r like the reference; the headline "
                        "computes them once per forward from t/r (fixed anchors, template queries: DESIGN.md section 3)"}
        except Exception as e:
            res["per_sample_block0_scope"] = {"error": repr(e)[:200]}
    if (rank == 0 and world == 1 and not args.no_extra_configs and args.precision == "fp32" and args.anchor_tables and args.overlap
            and (args.model, args.views, args.views_range, args.batch, parametric) == ("medium", 8, None, 32, False)):
        # SMALL-PER-GPU-BATCH regime: the reference's evaluation runs --val_batch_size 2 (lib/opt.py:27-30 upstream), and
        # BASELINE configs[4] read as a GLOBAL batch of 64 is 8 samples per GPU.  Same head, same code path; only the batch.
        small = {}
        try:
            legs = [(f"B{b}", [8] * b) for b in (1, 2, 4, 8, 16)]
            legs.append(("B8_ragged_2to10views", np.random.RandomState(5).randint(2, 11, size=8).tolist()))
            for name, vws in legs:
                _, b2, _ = make_leg(C, vws, False, dev, rank, rotate=4, seed0=3000)       # (weights are seeded: the same head)
                n = len(vws)
                sec = time_leg(head, b2, steps=max(20, 160 // n), warmup=5)
                with torch.no_grad():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(10):
                        head(*b2[i % len(b2)][:3])
                        torch.cuda.synchronize()
                    lat = (time.perf_counter() - t0) / 10
                small[name] = {"samples_per_s": n / sec, "ms_per_forward": sec * 1e3, "ms_per_forward_synced": lat * 1e3,
                               "views_total": int(sum(vws)), "frac_of_headline_per_sample_rate": (n / sec) / value}
                if n <= 8:
                    sec2 = time_leg_streams(head, b2, steps=max(20, 160 // n), warmup=5, nstreams=2)
                    small[name]["two_streams"] = {"samples_per_s": n / sec2, "ms_per_forward_throughput": sec2 * 1e3,
                                                  "frac_of_headline_per_sample_rate": (n / sec2) / value}
                del b2
            small["note"] = ("POEM-medium head, 8 views (or ragged), batch B per forward, back-to-back forwards on resident inputs "
                             "(`ms_per_forward`; `_synced`: a device sync after every forward = latency incl. host enqueue); "
                             "`frac_of_headline_per_sample_rate` = this batch's samples/s over the batch-32 headline's; "
                             "`two_streams`: the same forwards issued alternately on two torch streams (one engine per stream, "
                             "head.py): consecutive forwards overlap on the GPU -- the throughput of a small-batch evaluation loop; "
                             "the latency of one forward is `ms_per_forward_synced`")
        except Exception as e:   # informational: never fail the bench line on it
            small["error"] = repr(e)[:200]
        res["small_batch_scope"] = small
        torch.cuda.empty_cache()
        # RAGGED STREAMS as the reference's data pipeline produces them: a fresh view layout every batch
        # (collation_random_n_views; evaluation at --val_batch_size 2, lib/opt.py:27-30 upstream)
        fresh = {}
        for name, (b_, rule, n_) in {"B2_gauss": (2, "gauss", 60), "B8_uniform": (8, "uniform", 40), "c5_B64_uniform": (64, "uniform", 12)}.items():
            try:
                with torch.no_grad():
                    fresh[name] = fresh_layout_scope(head, dev, b_, rule, n_)
            except Exception as e:   # informational: never fail the bench line on it
                fresh[name] = {"error": repr(e)[:200]}
            torch.cuda.empty_cache()
        res["fresh_layout_scope"] = fresh
        # the per-GPU loads of the other BASELINE configs, same code path, short legs (reported beside the headline)
        extras = {}
        legs = {"c3_medium_MANO_8views_batch32": ("medium_MANO", [8] * 32, True),
                "c4_large_10views_batch16": ("large", [10] * 16, False),
                "c5_medium_ragged_2to10views_batch64": ("medium", np.random.RandomState(5).randint(2, 11, size=64).tolist(), False)}
        for name, (model, vws, par) in legs.items():
            try:
                Cx = pk.weights.MODEL_EMBED[model]
                h2, b2, _ = make_leg(Cx, vws, par, dev, rank, rotate=3, seed0=2000)
                sec = time_leg(h2, b2, steps=max(3, args.steps // 2), warmup=2)
                exx = executed_flops(Cx, vws, parametric=par)
                extras[name] = {"value": len(vws) / sec, "unit": "samples/s", "ms_per_step": sec * 1e3, "batch_per_gpu": len(vws),
                                "views_total": int(sum(vws)), "executed_TFLOPs": exx / sec / 1e12,
                                "frac_of_fp32_matrix_peak": exx / sec / 1e12 / FP32_MFMA_PEAK_TFLOPS}
                if par:
                    extras[name]["note"] = ("parametric tail on the device and INSIDE the forward's launch graph (poem_attach_mano): Q3 "
                                            "flatten + Linears + rot6d -> axis-angle + MANO linear blend skinning (csrc/mano.hip) with a "
                                            "synthetic asset set of MANO's shapes.  Third-party legs unpinned upstream: manotorch's "
                                            "ManoLayer, the MANO assets and pytorch3d's rot6d -> axis-angle chain are absent from the "
                                            "reference tree -- the MPVPE bar of this config (tests: <= 1e-3 mm) is against the oracle's "
                                            "restatement of the published MANO model, not against the third-party code")
                    extras[name]["vs_headline"] = (len(vws) / sec) / res["value"]
                del h2, b2
                torch.cuda.empty_cache()
            except Exception as e:   # informational: never fail the bench line on it
                extras[name] = {"error": repr(e)[:200]}
        res["extra_configs"] = extras
        # What the first real `--gpus N` run should show for `c5_global_ragged_batch64` (strong scaling of one global batch of
        # 64): every rank's shard of that batch (dist.shard_by_views) timed ALONE on this GPU; an N-GPU step takes as long as
        # its slowest shard (no data-path collective), so predicted value(N) = 64 / max shard time.
        try:
            views_g = np.random.RandomState(5).randint(2, 11, size=64)
            glob_b = pk.inputs.synthetic_batch(views_g.tolist(), seed=5000)
            pred = {}
            for n in (1, 2, 4, 8):
                ms = []
                for r in range(n):
                    lo, hi = pdist.shard_by_views(views_g, r, n)
                    item = to_dev(slice_batch(glob_b, lo, hi), dev)
                    ms.append(time_leg(head, [item], steps=max(6, 48 // (hi - lo)), warmup=3) * 1e3)
                    del item
                pred[f"n{n}"] = {"shard_ms_alone": [round(v, 4) for v in ms], "predicted_ms_per_step": max(ms),
                                 "predicted_value": 64.0 / max(ms) * 1e3}
            for n in (2, 4, 8):
                pred[f"n{n}"]["predicted_speedup_vs_n1"] = pred[f"n{n}"]["predicted_value"] / pred["n1"]["predicted_value"]
            pred["note"] = ("POEM-medium, one global batch of 64 samples with 2..10 views (seed 5) cut by dist.shard_by_views; each "
                            "shard timed alone on this one GPU, back-to-back forwards on resident inputs; predicted N-GPU step = the "
                            "slowest shard (the path has no data-path collective; the 16-byte metric all-reduce is not in this leg); "
                            "compare with `c5_global_ragged_batch64` of a real --gpus N line")
            res["predicted_c5_strong_scaling"] = pred
            del glob_b
        except Exception as e:   # informational: never fail the bench line on it
            res["predicted_c5_strong_scaling"] = {"error": repr(e)[:200]}
        torch.cuda.empty_cache()
    if world == 1 and not args.views_range and not parametric and legs:
        # one stage earlier (SURVEY 8f rows N1 + N2): backbone pyramid -> feat_decode / heatmap_stage -> DLT -> head.  The
        # HRNet backbone itself is out of scope; its output pyramid is synthetic.  Reported beside the headline, never as it.
        try:
            from poem_v2_amd.triangulation import triangulate_reference_joints
            dec = pk.decode.FeatureDecoders(pk.weights.seeded_decoder_state_dict(0), dev)
            pyr = [f.to(dev) for f in pk.inputs.synthetic_pyramid(args.batch * args.views, seed=1)]
            # 2-D joints for the DLT: the batch's own joints projected into every view (the heat maps of random features
            # carry no hand); the heat-map stage still runs and is consumed
            vs = torch.repeat_interleave(torch.arange(args.batch), args.views).to(dev)
            T = torch.linalg.inv(metas["cam_extr"])
            pc = (T[:, None, :3, :3] @ rj[vs][..., None]).squeeze(-1) + T[:, None, :3, 3]
            q2 = (metas["cam_intr"][:, None] @ pc[..., None]).squeeze(-1)
            uv_true = (q2[..., :2] / q2[..., 2:]).contiguous()

            def pstep():
                f160 = dec.feat_decode(pyr)
                uv = dec.heatmap_stage(pyr, 256, 256)
                uvb = uv_true + 1e-3 * (uv - uv.mean(dim=1, keepdim=True))
                rjp = triangulate_reference_joints(uvb, metas["cam_intr"], metas["cam_extr"], spec["views"])
                return head(f160, metas, rjp)

            with torch.no_grad():
                for _ in range(2):
                    pstep()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ksteps = max(2, args.steps // 2)
                for _ in range(ksteps):
                    pstep()
                torch.cuda.synchronize()
                pdt = (time.perf_counter() - t0) / ksteps
            res["pyramid_scope"] = {"value": args.batch / pdt, "unit": "samples/s", "ms_per_step": pdt * 1e3,
                                    "stages": "HRNet-shaped pyramid (synthetic) -> feat_decode + heatmap_stage (HIP) -> "
                                              "ragged DLT (HIP) -> head"}
        except Exception as e:   # informational: never fail the bench line on it
            res["pyramid_scope"] = {"error": repr(e)[:200]}
        # END-TO-END scope (SURVEY 8d "E2E"): 256x256 images resident in HBM -> HRNet-W40 on plain PyTorch-ROCm (MIOpen; the
        # backbone is outside the hot path and has no kernels of ours) -> the same pyramid-scope chain -> verts.
        if not args.no_e2e and "error" not in res["pyramid_scope"]:
            try:
                from poem_v2_amd.backbone import HRNet, seeded_hrnet_state_dict
                net = HRNet(state_dict=seeded_hrnet_state_dict(0), device=dev).to(dev)
                img = pk.inputs.synthetic_images(args.batch * args.views, seed=1).to(dev)

                kept = {}

                def estep(keep=False):
                    pyr_ = net(img)
                    f160 = dec.feat_decode(pyr_)
                    uv = dec.heatmap_stage(pyr_, 256, 256)
                    uvb = uv_true + 1e-3 * (uv - uv.mean(dim=1, keepdim=True))
                    rjp = triangulate_reference_joints(uvb, metas["cam_intr"], metas["cam_extr"], spec["views"])
                    if keep:                                 # every stage's output of THIS forward (the attribution below)
                        kept.update(pyr=pyr_, f160=f160, uv=uv, uvb=uvb, rjp=rjp)
                    return head(f160, metas, rjp)

                with torch.no_grad():
                    estep()                                  # MIOpen picks / builds its solvers here
                    estep()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    esteps = 3
                    for _ in range(esteps):
                        estep()
                    torch.cuda.synchronize()
                    edt = (time.perf_counter() - t0) / esteps
                    t0 = time.perf_counter()
                    for _ in range(esteps):
                        net(img)
                    torch.cuda.synchronize()
                    bdt = (time.perf_counter() - t0) / esteps
                e2e_first = estep(keep=True)["all_coords_preds"][:, :2].cpu()
                nv2 = 2 * args.views                                               # the first 2 samples' stage outputs of THAT forward
                e2e_pyr = {k: ([y[:nv2].cpu() for y in v] if k == "pyr" else v[:(2 if k == "rjp" else nv2)].cpu()) for k, v in kept.items()}
                kept.clear()
                res["e2e_scope"] = {"value": args.batch / edt, "unit": "samples/s", "ms_per_step": edt * 1e3,
                                    "backbone_ms": bdt * 1e3,
                                    "stages": f"{args.batch * args.views} synthetic 256x256 images in HBM -> HRNet-W40 (PyTorch-ROCm "
                                              "eager / MIOpen fp32, BatchNorm folded) -> feat_decode + heatmap_stage (HIP) -> "
                                              "ragged DLT (HIP) -> head (HIP)"}
                del net, img
            except Exception as e:
                res["e2e_scope"] = {"error": repr(e)[:200]}
    # INPUT scope: the per-view crop / warp / normalise of the raw camera images, one launch per batch.
    # The boundary hands over host buffers here (decoded images), so both rates are given: the kernel alone (HIP events)
    # against HBM, and the whole warp_views call (pinned staging fill + one H2D copy + launch).
    if rank == 0 and world == 1 and not args.no_e2e:
        try:
            import numpy as _np
            g = _np.random.default_rng(0)
            nv = args.batch * args.views
            raws = [g.integers(0, 256, size=(480, 640, 3), dtype=_np.uint8) for _ in range(8)]
            imgs = [raws[i % 8] for i in range(nv)]
            Ms = [_np.array([[1.28, 0.0, -150.0 - (i % 7)], [0.0, 1.28, -90.0 - (i % 5)]], _np.float32) for i in range(nv)]
            for _ in range(2):
                pk.transform.warp_views(imgs, Ms, (256, 256), device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reps = 5
            for _ in range(reps):
                pk.transform.warp_views(imgs, Ms, (256, 256), device=dev)
            torch.cuda.synchronize()
            call_ms = (time.perf_counter() - t0) / reps * 1e3
            # kernel alone: parameters + images already resident
            import ctypes as _ct
            head_b = (nv * 88 + 15) & ~15
            blob = torch.zeros(head_b + nv * 480 * 640 * 3, dtype=torch.uint8, device=dev)
            hb = _np.zeros(head_b, _np.uint8)
            hb[0:8 * nv].view(_np.int64)[:] = _np.arange(nv) * 480 * 640 * 3
            hb[8 * nv:16 * nv].view(_np.int32)[:] = _np.tile(_np.array([480, 640], _np.int32), nv)
            hb[16 * nv:64 * nv].view(_np.float64)[:] = _np.asarray([pk.transform.invert_affine(m) for m in Ms]).reshape(-1)
            blob[:head_b] = torch.from_numpy(hb).to(dev)
            blob[head_b:] = torch.from_numpy(_np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
            outw = torch.empty(nv, 3, 256, 256, device=dev)
            base = blob.data_ptr()
            L = pk.hip.lib()

            def wk():
                pk.hip.check(L.poem_warp_affine(base + head_b, base, base + 8 * nv, base + 16 * nv, None, outw.data_ptr(), None,
                                                nv, 256, 256, pk.hip.stream()), "poem_warp_affine")
            wk()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                wk()
            e1.record()
            torch.cuda.synchronize()
            k_ms = e0.elapsed_time(e1) / 20
            alg = nv * (3 * 256 * 256 * 4 + 3 * 200 * 200)          # fp32 image written + the 200x200 source footprint read
            res["input_scope"] = {"views": nv, "source": "640x480x3 uint8", "kernel_ms": k_ms,
                                  "kernel_GBps_algorithmic": alg / k_ms / 1e6, "hbm_frac_of_8TBps": alg / k_ms / 1e6 / 8000.0,
                                  "call_ms_incl_pinned_fill_and_h2d": call_ms, "h2d_bytes": nv * 480 * 640 * 3,
                                  "stages": "raw uint8 views -> poem_warp_affine (crop/warp/to_tensor/normalize) -> (BN,3,256,256) fp32"}
            del blob, outw
        except Exception as e:
            res["input_scope"] = {"error": repr(e)[:200]}
    if rank == 0 and world == 1 and args.cpu_samples > 0 and not parametric:
        base, ref = cpu_baseline(C, batch, args.cpu_samples)
        res["cpu_baseline"] = base
        if "e2e_scope" in res and "error" not in res["e2e_scope"] and not args.views_range:
            try:
                eb, eout, staged = cpu_baseline_e2e(C, batch, min(2, args.cpu_samples), base["cores"], pyr_dev=e2e_pyr)
                res["e2e_scope"]["cpu_baseline"] = eb
                res["e2e_scope"]["speedup_vs_cpu"] = res["e2e_scope"]["value"] / eb["value"]
                mp = lambda a, b_: float(torch.norm(a[-1, :b_.shape[1], 21:] - b_[-1, :, 21:], dim=-1).mean()) * 1e3
                res["e2e_scope"]["mpvpe_vs_cpu_restatement_mm"] = mp(e2e_first, eout)
                res["e2e_scope"]["mpvpe_attribution"] = {
                    "backbone_max_rel_diff_by_level": staged["backbone_max_rel_diff_by_level"],
                    "feat_decode_max_rel_diff": staged["feat_decode_max_rel_diff"],
                    "heatmap_uv_max_abs_diff_px": staged["heatmap_uv_max_abs_diff_px"],
                    "dlt_joints_max_abs_diff_m": staged["dlt_joints_max_abs_diff_m"],
                    "head_vs_restatement_on_the_devices_own_inputs_mm": mp(e2e_first, staged["head_on_device_inputs"]),
                    "restatement_vs_itself_with_inputs_perturbed_1e-7_rel_mm": mp(staged["head_on_perturbed_inputs"], staged["head_on_device_inputs"]),
                    "head_input_feature_absmax": staged["feat_absmax"], "head_input_feature_std": staged["feat_std"],
                    "mesh_extent_around_its_centre_m": staged["mesh_extent_m"],
                    "cpu_chain_on_device_pyramid_vs_on_cpu_pyramid_mm": mp(staged["cpu_chain_on_device_pyramid"], eout),
                    "note": "`mpvpe_vs_cpu_restatement_mm` compares two END-TO-END chains whose BACKBONES differ: HRNet-W40 is outside "
                            "the hot path and runs on PyTorch-ROCm (MIOpen's fp32 convolution solvers), the CPU leg on PyTorch's CPU "
                            "convolutions; their pyramids differ at the relative level listed per pyramid level, and the chain behind "
                            "them -- seeded random weights, heat maps of features that show no hand -- amplifies an input difference "
                            "of that size to the last number (the SAME CPU code run on the two pyramids).  Stage by stage, each HIP "
                            "stage against its CPU restatement fed with the device's own input to that stage: the four numbers in "
                            "between (the parity bar, 1e-3 mm, applies to the head's; tests/test_backbone.py asserts all of them)"}
            except Exception as e:   # informational: never fail the bench line on it
                res["e2e_scope"]["cpu_baseline"] = {"error": repr(e)[:200]}
        with torch.no_grad():
            preds = step(0)                       # the batch the CPU leg restates (outside the timed region)
        got = preds["all_coords_preds"][:, :args.cpu_samples].cpu()
        res["mpvpe_vs_oracle_mm"] = float(torch.norm(got[-1, :, 21:] - ref[-1, :, 21:], dim=-1).mean()) * 1e3
        res["speedup_vs_cpu"] = value / base["value"]
        try:
            res["eager_baseline"] = eager_baseline(C, batch, args.cpu_samples, dev)
            res["speedup_vs_eager"] = value / res["eager_baseline"]["value"]
        except Exception as e:   # the eager leg is informational: never fail the bench line on it
            res["eager_baseline"] = {"error": repr(e)[:200]}
    if grouped and args.precision == "fp32" and legs and not args.views_range and not parametric:
        # BASELINE configs[4] as ONE global batch: 64 samples with 2..10 views each (seed 5), split over the ranks by
        # dist.shard_by_views (contiguous sample ranges balanced by their view counts) -- strong scaling of that batch, next
        # to the weak-scaling headline above.  No data-path collective: each rank runs its shard, the time is the slowest rank's.
        try:
            res["c5_global_ragged_batch64"] = c5_global_leg(head, C, dev, rank, world, max(5, args.steps))
        except Exception as e:
            res["c5_global_ragged_batch64"] = {"error": repr(e)[:200]}
    if rank == 0:
        print(json.dumps(res))
    pdist.shutdown()


if __name__ == "__main__":
    main()
