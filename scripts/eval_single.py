#!/usr/bin/env python
"""Single-setting evaluation of the hot path -- the drop-in counterpart of the reference's ``scripts/eval_single.py``.

Same command line (``--cfg --dataset --view_min --view_max --model -g --reload -p --draw``; ``--draw`` renders on the device and
needs the mesh topology: ``--faces FILE.npy``, panels under ``--draw-dir``; ``--losses --j-regressor FILE.npy`` with ``--shards`` adds the
averages of upstream's loss terms to the result line; ``--benchmark-scores`` adds the FreiHAND / HO3D leaderboard numbers, mesh
F@5 / F@15 and the aligned AUCs, as a ``"benchmark"`` block) and the same YAML edits
(scripts/eval_single.py:63-86 upstream: dataset URL / epoch size / view range, the four size fields derived from the
model category, PARAMETRIC_OUTPUT for medium_MANO), written back to ``--cfg`` exactly as upstream does.  What differs:

* the reference shells out to ``./ddp_python scripts/eval.py`` (full model: HRNet + heat-map stage + DLT + head).  This
  build owns the head / decoder path only, so the evaluation loop here feeds the head the tensors
  the reference's ``_forward_impl`` would hand it (lib/models/POEM.py:306-332): backbone features, cameras and
  triangulated reference joints;
* the dataset tars are not available offline: the source is the seeded synthetic generator of ``poem_v2_amd.inputs``
  with views per sample drawn from ``[view_min, view_max]`` the way ``collation_random_n_views`` does
  (lib/utils/collation.py:7-25 upstream).  ``--epoch_size`` bounds the run (default: 64 samples, not the dataset's).

One process per GPU: run directly (``-g 0``) or under ``python -m torch.distributed.run --nproc-per-node N``; ranks take
contiguous sample shards and the metric sums meet in one all-reduce (RCCL)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import poem_v2_amd as pk  # noqa: E402
from poem_v2_amd import dist as pdist  # noqa: E402
from poem_v2_amd.metrics import Joint3DPCK, MeanEPE, MeshFScore, PAEval, PAJoint3DPCK, PAVert3DPCK, Vert3DPCK  # noqa: E402
from poem_v2_amd.triangulation import triangulate_reference_joints  # noqa: E402

# scripts/eval_single.py:5-36 upstream (urls kept for the record; the tars are not shipped)
DATASET_META = {
    "HO3D": {"url": "data/dataset_tars/HO3D_mv_test/HO3D_mv_test-{000000..000002}.tar", "max_view": 5, "epoch_size": 2706},
    "DexYCB": {"url": "data/dataset_tars/DexYCB_mv/DexYCB_mv_test-{000000..000003}.tar", "max_view": 8, "epoch_size": 4950},
    "Arctic": {"url": "data/dataset_tars/Arctic_mv/Arctic_mv_val_p1-{000000..000045}.tar", "max_view": 8, "epoch_size": 17392},
    "Interhand": {"url": "data/dataset_tars/Interhand_mv/Interhand_mv_val-{000000..000022}.tar", "max_view": 8, "epoch_size": 85255},
    "Oakink": {"url": "data/dataset_tars/Oakink_mv/Oakink_mv_test-{000000..000045}.tar", "max_view": 4, "epoch_size": 21351},
    "Freihand": {"url": "data/dataset_tars/Freihand_mv/Freihand_mv_test-{000000..000000}.tar", "max_view": 1, "epoch_size": 3960},
}
MODEL_CATEGORY = ["small", "medium", "large", "huge", "medium_MANO"]
EMBED_SIZE = [128, 256, 512, 1024, 256]


def edit_cfg(cfg, dataset, model_type, view_range):
    """The in-place YAML edits of scripts/eval_single.py:63-86 upstream.  Returns the (possibly adjusted) view range."""
    if dataset not in DATASET_META:
        raise AssertionError(f"Dataset {dataset} not found in dataset_info.")
    if model_type not in MODEL_CATEGORY:
        raise AssertionError(f"Model category {model_type} not found in model_category.")
    meta = DATASET_META[dataset]
    test = cfg.setdefault("DATASET", {}).setdefault("TEST", {})
    tgt = test.setdefault("TARGET", {})
    tgt["URLS"] = meta["url"]
    test["EPOCH_SIZE"] = meta["epoch_size"]
    tgt["EPOCH_SIZE"] = meta["epoch_size"]
    if dataset == "Freihand":
        view_range = [1, 1]
        print("Setting view range to 1 for Freihand dataset.")
    tgt["VIEW_RANGE"] = list(view_range)
    embed = EMBED_SIZE[MODEL_CATEGORY.index(model_type)]
    head = cfg.setdefault("MODEL", {}).setdefault("HEAD", {})
    head.setdefault("POSITIONAL_ENCODING", {})["NUM_FEATS"] = embed // 2
    head.setdefault("TRANSFORMER", {})["INPUT_FEAT_DIM"] = embed
    head["POINTS_FEAT_DIM"] = embed
    head["EMBED_DIMS"] = embed
    head["TRANSFORMER"]["PARAMETRIC_OUTPUT"] = model_type == "medium_MANO"
    return view_range


def default_cfg():
    """A config tree with the release MODEL.HEAD subtree (config/release/train_medium.yaml:185-225 upstream)."""
    def plain(node):
        return {k: plain(v) if isinstance(v, dict) else v for k, v in dict(node).items()}
    head = plain(pk.configs.head_cfg(256))
    head.pop("MAX_VIEWS", None)
    return {"DATASET": {"TEST": {"TARGET": {}}}, "MODEL": {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": head}}


def loss_node(cfg):
    """The ``LOSS`` node of the evaluated config when it has one, else the release values (config/release/train_medium.yaml:226-235
    upstream, restated in ``poem_v2_amd.configs.loss_cfg``)."""
    node = cfg.get("MODEL", {}).get("LOSS")
    return dict(node) if node else dict(pk.configs.loss_cfg())


def check_losses_args(args):
    if not args.losses:
        return
    if not args.shards:
        raise SystemExit("--losses needs --shards: the loss terms read target_joints_2d and the heat maps' 2-D joints, which only the "
                         "record-shard scope has")
    if not args.j_regressor:
        raise SystemExit("--losses needs --j-regressor FILE.npy: MANO's th_J_regressor (16,778) for loss_3d_joints_from_mesh -- an input, "
                         "the asset is licence-gated (INTEGRATION.md)")


def random_views(n_samples, view_range, seed):
    rng = np.random.RandomState(seed)
    lo, hi = view_range
    return rng.randint(lo, hi + 1, size=n_samples).tolist()


def load_template(path):
    """(799,3) zero-pose hand template in metres (rows 0..20 joints, 21..798 vertices, centred at joint 9) from a ``.npy`` /
    ``.pt`` file: on a licensed machine, ManoLayer's zero-pose output (lib/models/heads/ptEmb_head.py:886-892 upstream)."""
    t = np.load(path) if path.endswith(".npy") else torch.load(path, map_location="cpu")
    return torch.as_tensor(np.asarray(t), dtype=torch.float32).reshape(799, 3)


def head_state_dict(sd):
    """The head's part of a checkpoint -- full model (``ptEmb_head.*``, optionally behind ``module.`` as upstream's ``load_weights``
    strips it) or head only -- for a plain ``head.load_state_dict(..., strict=True)``."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    if any(k.startswith("ptEmb_head.") for k in sd):
        sd = {k[len("ptEmb_head."):]: v for k, v in sd.items() if k.startswith("ptEmb_head.")}
    return sd


def install_template(head, reload, template, mano_assets=None):
    """Which hand template the head runs with, and a word for the result record.  A seeded synthetic template is only
    right for seeded synthetic weights: with ``--reload`` the template must come from ``--template`` or ``--mano-assets`` (the head
    derives it from the assets itself; it refuses to run a reference checkpoint on the synthetic one)."""
    if template:
        head.set_template(load_template(template))
        return f"file:{template}"
    if mano_assets:
        return f"mano-assets:{mano_assets}"
    if reload:
        return "synthetic (NO --template given with --reload: metrics are not meaningful for a real checkpoint)"
    head.set_template(pk.inputs.synthetic_template(1234))
    return "synthetic(seed=1234)"


class BenchmarkScores:
    """``--benchmark-scores``: the numbers of the FreiHAND / HO3D leaderboards that upstream's evaluation leaves to the protocol
    scripts -- mesh F-scores at 5 / 15 mm, raw and Procrustes-aligned, the AUC of the aligned joints / vertices over 0..50 mm in
    100 steps, and the symmetric mean nearest-vertex distance -- accumulated on the device next to the other metrics."""
    PCK = dict(VAL_MIN=0.0, VAL_MAX=0.05, STEPS=100)

    def __init__(self, device):
        self.f = MeshFScore(thresholds=(0.005, 0.015), aligned=True, device=device)
        self.pck_j = PAJoint3DPCK(device=device, EVAL_TYPE="joints_3d", **self.PCK)
        self.pck_v = PAVert3DPCK(device=device, EVAL_TYPE="verts_3d", **self.PCK)

    def feed(self, pred_joints, gt_joints, pred_verts, gt_verts):
        self.f.feed(pred_verts, gt_verts)
        self.pck_j.feed({"pred_joints_3d": pred_joints}, {"master_joints_3d": gt_joints})
        self.pck_v.feed({"pred_verts_3d": pred_verts}, {"master_verts_3d": gt_verts})

    def result(self):
        """The ``"benchmark"`` block, reduced over ranks like the other metrics (every rank calls it)."""
        m = self.f.reduce().get_measures()
        return {"F@5": m["F@5"], "F@15": m["F@15"], "PA_F@5": m["PA_F@5"], "PA_F@15": m["PA_F@15"],
                "pa_auc_j": self.pck_j.reduce().get_measures()["auc_all"], "pa_auc_v": self.pck_v.reduce().get_measures()["auc_all"],
                "chamfer_mm": 0.5 * (m["chamfer_pred2gt"] + m["chamfer_gt2pred"]) * 1e3}


class InlierFraction:
    """``--dlt-confidence ransac``: the share of (view, joint) pairs the robust triangulation kept, summed on the device (no read-back
    per batch) and reduced over ranks like the other metrics."""

    def __init__(self, device):
        self.acc = torch.zeros(2, dtype=torch.float64, device=device)           # (inliers, pairs)

    def feed(self, inlier):
        self.acc[0] += inlier.sum()
        self.acc[1] += inlier.numel()

    def result(self):
        n, total = pdist.all_reduce_sum_(self.acc.clone()).tolist()       # (every rank calls it; the local sums stay)
        return n / total if total else None


class ManoFitStats:
    """``--fit-mano``: the mean vertex distance between the fitted and the predicted mesh (mm), the number of flagged samples and,
    where the records carry ground-truth fits, the mean absolute betas error -- sums on the device, read once at the end."""

    def __init__(self, device):
        # (sum of distances, vertices, flagged, sum |dbeta|, betas, sum of reprojection distances in pixels, keypoints)
        self.acc = torch.zeros(7, dtype=torch.float64, device=device)

    def feed(self, fit_verts, pred_verts, status, betas=None, gt_betas=None):
        ok = (status == 0)
        d = torch.linalg.norm(fit_verts.double() - pred_verts.double(), dim=-1)[ok]
        self.acc[0] += d.sum()
        self.acc[1] += d.numel()
        self.acc[2] += (~ok).sum()
        if gt_betas is not None:
            e = (betas.double() - gt_betas.double()).abs()[ok]
            self.acc[3] += e.sum()
            self.acc[4] += e.numel()

    def feed_reproj(self, fit_joints, uv, weight, cam_intr, cam_extr, views, status):
        """``--fit-mano-keypoints``: pixel distance between the fitted joints' projections and the 2-D joints, over the entries of
        positive weight of unflagged samples"""
        views = [int(v) for v in views]
        proj = pk.render.project_to_views(fit_joints.contiguous(), cam_intr.float().contiguous(), cam_extr.float().contiguous(), views)
        ok = torch.repeat_interleave(status == 0, torch.as_tensor(views, device=status.device))
        use = (weight > 0) & ok[:, None]
        d = torch.linalg.norm(proj.double() - uv.double(), dim=-1)[use]
        self.acc[5] += d.sum()
        self.acc[6] += d.numel()

    def result(self, reproj=False):
        a = self.acc.tolist()
        res = {"mano_fit_residual_mm": a[0] / a[1] * 1e3 if a[1] else None, "mano_fit_flagged": int(a[2])}
        if a[4]:
            res["mano_fit_betas_mae"] = a[3] / a[4]
        if reproj:
            res["mano_fit_reproj_px"] = a[5] / a[6] if a[6] else None
        return res


def master_rows(batch):
    """row of each sample's master view in the per-view arrays of a collated batch"""
    views = np.asarray(batch["cam_view_num"]).astype(np.int64)
    first = np.concatenate([[0], np.cumsum(views)[:-1]]).astype(np.int64)
    master = batch["master_id"]
    master = master.cpu().numpy() if torch.is_tensor(master) else np.asarray(master)
    return torch.as_tensor(first + master.astype(np.int64).reshape(-1))


def evaluate(cfg, view_range, model_type, device, reload=None, epoch_size=64, batch_size=2, seed=0, verbose=True,
             pyramid=False, template=None, dlt_confidence="off", dlt_threshold=0.5, draw=None, mano_assets=None,
             benchmark_scores=False, dlt_inlier_px=8.0, dlt_refine=0, fit_mano_iters=None, fit_mano_keypoints=0.0):
    """``draw``: a ``DrawingHandCallback`` (rank 0, ``--draw --faces``) called with every batch.  This scope has no images: the panels
    show the meshes and skeletons over mid-grey views.  ``benchmark_scores``: add the ``"benchmark"`` block (``BenchmarkScores``).
    ``fit_mano_iters``: not None fits MANO pose / shape / translation to every predicted mesh (``pk.fit_mano``, needs ``mano_assets``)
    and adds ``mano_fit_residual_mm`` / ``mano_fit_flagged`` to the result.  ``fit_mano_keypoints`` > 0: the fit also takes the 2-D
    joints the reference joints were triangulated from, in every view, with that weight (times the confidences and the inlier mask
    where the DLT mode has them), and the result gains ``mano_fit_reproj_px``."""
    rank, _, world = pdist.env_world()
    fit_layer = fit_acc = None
    if fit_mano_iters is not None:
        if not mano_assets:
            raise SystemExit("--fit-mano needs the MANO assets: pass --mano-assets FILE.npz")
        fit_layer = pk.ManoLayer(pk.mano.normalise_mano_assets(mano_assets), center_idx=None, device=device)
        fit_acc = ManoFitStats(device)
    if dlt_confidence != "off" and not pyramid:
        raise SystemExit("--dlt-confidence reads the heat-map stage's output: it needs --pyramid or --shards (this scope starts "
                         "behind the heat-map stage)")
    inlier_acc = InlierFraction(device) if dlt_confidence == "ransac" else None
    head_node = pk.CN(cfg["MODEL"]["HEAD"])
    head_node["MAX_VIEWS"] = max(10, int(view_range[1]))
    if mano_assets:
        head_node["MANO_ASSETS"] = mano_assets       # template and (medium_MANO) the MANO layer come from the assets, in the head
    head = pk.build_head(head_node, data_preset=pk.CN({}))
    embed = head.embed_dims
    if reload:
        sd = torch.load(reload, map_location="cpu")
        sd = sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd
        head.load_state_dict(head_state_dict(sd), strict=True)
        if verbose and rank == 0:
            print(f"reloaded {reload}: {len(head.ignored_reference_keys)} dead tensors ignored")
    else:
        head.load_state_dict(pk.weights.seeded_state_dict(embed, seed=0, parametric=head.parametric_output), strict=False)
    template_source = install_template(head, reload, template, mano_assets)
    if head.parametric_output and not mano_assets:
        raise SystemExit("medium_MANO needs a MANO layer (licence-gated assets): pass --mano-assets FILE.npz (v_template, shapedirs, "
                         "posedirs, J_regressor, weights), or call head.set_mano_layer(fn) from Python")
    head = head.to(device).eval()
    # --pyramid: start one stage earlier, at the backbone's multi-level features (lib/models/POEM.py:264-270 upstream):
    # feat_decode gives the head's mlvl_feat, heatmap_stage the per-view 2-D joints that are triangulated
    decoders = None
    if pyramid:
        if reload:
            decoders = pk.decode.FeatureDecoders.load_reference_state_dict(sd, device)
        else:
            decoders = pk.decode.FeatureDecoders(pk.weights.seeded_decoder_state_dict(0), device)
    views_all = random_views(epoch_size, view_range, seed)
    lo, hi = pdist.shard_by_views(views_all, rank, world)
    mpvpe, mpjpe = MeanEPE("verts", device=device), MeanEPE("joints", device=device)
    pa = PAEval(None, mesh_score=True, device=device)                       # lib/models/POEM.py:147 upstream
    pck = dict(VAL_MIN=0.0, VAL_MAX=0.02, STEPS=20)                         # AUCCallback defaults, lib/utils/testing.py:31
    pck_j, pck_v = Joint3DPCK(device=device, EVAL_TYPE="joints_3d", **pck), Vert3DPCK(device=device, EVAL_TYPE="verts_3d", **pck)
    bench_scores = BenchmarkScores(device) if benchmark_scores else None
    n_done, t0, t_draw = 0, None, 0.0
    with torch.no_grad():
        for it, s in enumerate(range(lo, hi, batch_size)):
            views = views_all[s:min(s + batch_size, hi)]
            b = pk.inputs.synthetic_batch(views, seed=seed * 100003 + s)
            metas = dict(b["img_metas"])
            metas["cam_intr"], metas["cam_extr"] = metas["cam_intr"].to(device), metas["cam_extr"].to(device)
            # reference joints the way the full model gets them (lib/models/POEM.py:284-299): DLT over each sample's views
            # of the per-view 2-D joints (here: the synthetic joints projected into every view + 1 px noise)
            vs = torch.repeat_interleave(torch.arange(len(views)), torch.tensor(views))
            T = torch.linalg.inv(b["img_metas"]["cam_extr"])
            X = b["reference_joints"][vs]
            pc = (T[:, None, :3, :3] @ X[..., None]).squeeze(-1) + T[:, None, :3, 3]
            q = (b["img_metas"]["cam_intr"][:, None] @ pc[..., None]).squeeze(-1)
            gn = torch.Generator().manual_seed(seed * 31 + s)
            uv = (q[..., :2] / q[..., 2:] + torch.randn(q[..., :2].shape, generator=gn)).to(device)
            mlvl_feat = b["mlvl_feat"].to(device)
            if decoders is not None:
                pyr = [f.to(device) for f in pk.inputs.synthetic_pyramid(sum(views), seed=seed * 100003 + s)]
                mlvl_feat = decoders.feat_decode(pyr)                                   # POEM.py:267
                if dlt_confidence in ("off", "ransac"):
                    uv_pred = decoders.heatmap_stage(pyr, 256, 256)                     # POEM.py:270
                else:
                    uv_pred, conf = decoders.heatmap_stage(pyr, 256, 256, return_conf=True)
                # random features carry no hand: keep the pipeline honest (the kernels run, their output is consumed)
                # but triangulate a blend that stays near the synthetic joints so the head sees sane geometry
                uv = uv + 1e-3 * (uv_pred - uv_pred.mean(dim=1, keepdim=True))
            if min(views) >= 2 and dlt_confidence == "ransac":   # views that disagree with the others' geometry are left out
                rj, inl, _ = triangulate_reference_joints(uv, metas["cam_intr"], metas["cam_extr"], views, mode="ransac",
                                                          inlier_px=dlt_inlier_px, refine=dlt_refine, return_inliers=True)
                inlier_acc.feed(inl)
            elif min(views) >= 2 and dlt_confidence != "off":   # upstream's triangulate_dlt (lib/utils/triangulation.py:111-148)
                rj = triangulate_reference_joints(uv, metas["cam_intr"], metas["cam_extr"], views, conf=conf,
                                                  mode=dlt_confidence, threshold=dlt_threshold)
            elif min(views) >= 2:
                rj = triangulate_reference_joints(uv, metas["cam_intr"], metas["cam_extr"], views)
            else:                                        # single-view samples take the given joints (POEM.py:282-283)
                rj = b["reference_joints"].to(device)
            kp_conf, kp_inl = None, None
            if min(views) >= 2 and dlt_confidence == "ransac":
                kp_inl = inl
            elif min(views) >= 2 and dlt_confidence != "off":
                kp_conf = conf
            preds = head(mlvl_feat, metas, rj)["all_coords_preds"]
            g = torch.Generator().manual_seed(seed * 7919 + s)
            gt = (b["reference_joints"][:, 9:10] + 0.05 * torch.randn(len(views), 799, 3, generator=g)).to(device)
            mpjpe.feed(preds[-1, :, :21], gt[:, :21])      # lib/models/POEM.py:443-444 upstream: joints then verts
            mpvpe.feed(preds[-1, :, 21:], gt[:, 21:])
            pa.feed(preds[-1, :, :21], gt[:, :21], preds[-1, :, 21:], gt[:, 21:])
            pck_j.feed({"pred_joints_3d": preds[-1, :, :21]}, {"master_joints_3d": gt[:, :21]})
            pck_v.feed({"pred_verts_3d": preds[-1, :, 21:]}, {"master_verts_3d": gt[:, 21:]})
            if bench_scores is not None:
                bench_scores.feed(preds[-1, :, :21], gt[:, :21], preds[-1, :, 21:], gt[:, 21:])
            if fit_acc is not None:
                pv = preds[-1, :, 21:].contiguous()
                if fit_mano_keypoints > 0:
                    w2 = torch.full(uv.shape[:2], float(fit_mano_keypoints), dtype=torch.float32, device=device)
                    w2 = w2 if kp_conf is None else w2 * kp_conf
                    w2 = w2 if kp_inl is None else torch.where(kp_inl, w2, torch.zeros_like(w2))
                    cams = (metas["cam_intr"].float().contiguous(), metas["cam_extr"].float().contiguous())
                    fitted = pk.fit_mano(fit_layer, pv, iters=fit_mano_iters, keypoints=uv.float().contiguous(), keypoint_weights=w2,
                                         cam_intr=cams[0], cam_extr=cams[1], cam_view_num=views, image_scale=256.0)
                    fit_acc.feed_reproj(fitted.joints, uv, w2, cams[0], cams[1], views, fitted.status)
                else:
                    fitted = pk.fit_mano(fit_layer, pv, iters=fit_mano_iters)
                fit_acc.feed(fitted.verts, pv, fitted.status)
            if draw is not None:                           # rendering, the copy and the PNG files stay out of samples/s
                torch.cuda.synchronize(device)
                t_d = time.perf_counter()
                img_w, img_h = (int(v) for v in metas.get("inp_img_shape", (256, 256)))
                draw({"pred_verts_3d": preds[-1, :, 21:].contiguous(), "pred_joints_3d": preds[-1, :, :21].contiguous()},
                     {"image": torch.zeros(sum(views), 3, img_h, img_w, device=device), "cam_view_num": views,
                      "target_cam_intr": metas["cam_intr"], "target_cam_extr": metas["cam_extr"],
                      "master_verts_3d": gt[:, 21:], "master_joints_3d": gt[:, :21]}, it)
                torch.cuda.synchronize(device)
                t_draw += (time.perf_counter() - t_d) if it > 0 else 0.0
            if it == 0:                                    # first batch builds the engine; time from the second on
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
            else:
                n_done += len(views)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0 - t_draw if t0 else 0.0
    mpvpe.reduce(), mpjpe.reduce(), pa.reduce(), pck_j.reduce(), pck_v.reduce()
    pam = pa.get_measures()
    res = {"dataset_source": "synthetic", "scope": "pyramid->verts" if pyramid else "mlvl_feat->verts", "model": model_type, "embed": embed, "view_range": list(view_range),
           "samples": int(mpvpe.acc[1].item()), "MPVPE_mm_vs_synthetic_gt": mpvpe.result() * 1e3,
           "MPJPE_mm_vs_synthetic_gt": mpjpe.result() * 1e3, "PA_MPJPE_mm": pam["pa_mpjpe"] * 1e3,
           "PA_MPVPE_mm": pam["pa_mpvpe"] * 1e3, "auc_j": pck_j.get_measures()["auc_all"], "auc_v": pck_v.get_measures()["auc_all"],
           "samples_per_s_rank0": (n_done / dt) if dt > 0 and n_done else None, "world_size": world,
           "template_source": template_source}
    if bench_scores is not None:
        res["benchmark"] = bench_scores.result()
    if inlier_acc is not None:
        res["dlt_inlier_fraction"] = inlier_acc.result()
    if fit_acc is not None:
        res.update(fit_acc.result(reproj=fit_mano_keypoints > 0))
    return res


BACKBONE_TYPES = {"hrnet": "HRNet", "resnet18": "ResNet18", "resnet34": "ResNet34", "resnet50": "ResNet50"}


def evaluate_shards(cfg, view_range, model_type, device, shard_dir, dataset, reload=None, epoch_size=16, batch_size=2,
                    n_cams=8, raw_size=(640, 480), template=None, dlt_confidence="off", dlt_threshold=0.5, draw=None, losses=None,
                    mano_assets=None, backbone_engine="torch", backbone="hrnet", benchmark_scores=False, dlt_inlier_px=8.0,
                    dlt_refine=0, image_decode="host", fit_mano_iters=None, fit_mano_keypoints=0.0):
    """Images -> metrics from record shards (SURVEY 8f N4 in front of the model): ``MultiviewWebDataset`` over the URLS of the
    edited config (tar records: ``image_<i>.png|jpg`` + ``label.pyd``), the per-view crop / warp / normalise on the
    device (one launch per batch), ``collation_random_n_views``, then the model-level caller
    (``PtEmbedMultiviewStereoV2``: HRNet on PyTorch-ROCm -> decode / heat maps / DLT / head on HIP) and the device metrics
    against the records' ``master_joints_3d`` / ``master_verts_3d`` (lib/models/POEM.py:596-610 upstream).
    ``backbone_engine``: ``"hip"`` runs the backbone on the project's own convolution kernels (model key BACKBONE.ENGINE).
    ``backbone``: "hrnet" | "resnet18" | "resnet34" | "resnet50" sets MODEL.BACKBONE.TYPE and MODEL.HEAD.IN_CHANNELS (160 / 128 / 512).
    ``losses``: MANO's (16,778) joint regressor (``--losses --j-regressor``): every batch's loss terms (upstream's ``compute_loss``,
    value only) feed the model's ``loss_metric`` on the device and the result gains their batch-size-weighted averages.
    ``benchmark_scores``: add the ``"benchmark"`` block (``BenchmarkScores``), as ``evaluate`` does.
    ``image_decode``: ``"device"`` keeps the records' JPEG views encoded up to the batch's warp launch (Huffman decoding on host
    threads, reconstruction on the GPU, bit-equal to PIL; ``wds.EncodedImage``) and adds ``jpeg_device_fraction`` to the result: the
    share of those views the device route took (the rest went through PIL).  ``"device-entropy"``: the same with the Huffman
    decoding on the GPU as well (``poem_jpeg_entropy_device``); a batch in which the device refuses a scan is redone on ``"device"``'s route.
    ``fit_mano_iters``: not None sets the model keys FIT_MANO / FIT_MANO_ITERS (needs ``mano_assets``); the result gains
    ``mano_fit_residual_mm``, ``mano_fit_flagged`` and, where the records carry ``mano_shape``, ``mano_fit_betas_mae``.
    ``fit_mano_keypoints`` > 0 sets the model key FIT_MANO_KEYPOINTS; the result gains ``mano_fit_reproj_px``.
    The dataset tars are not available offline: when ``shard_dir`` holds no shard of the dataset's name, seeded synthetic
    shards of the same record layout are written there first."""
    rank, _, world = pdist.env_world()
    ds_node = cfg["DATASET"]["TEST"]["TARGET"]
    pattern = os.path.join(shard_dir, os.path.basename(ds_node["URLS"]))
    urls = pk.wds.expand_urls(pattern)
    if rank == 0 and not all(os.path.exists(u) for u in urls):
        synthetic_frame = pk.inputs.synthetic_frame
        os.makedirs(shard_dir, exist_ok=True)
        per = -(-epoch_size // len(urls))
        for si, u in enumerate(urls):
            pk.wds.write_shard(u, [synthetic_frame(si * per + i, n_cams=n_cams, raw=raw_size) for i in range(per)])
    pdist.barrier()
    node = pk.wds.dataset_cfg(pattern, view_range=view_range, device=str(device))
    dset = pk.MultiviewWebDataset(node, data_preset=node.DATA_PRESET, is_train=False, defer_images=True, rank=rank, world=world,
                                  image_decode=image_decode)
    pk.transform.reset_jpeg_counts()
    head_node = dict(cfg["MODEL"]["HEAD"])
    head_node["MAX_VIEWS"] = max(10, int(view_range[1]))
    model_node = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": head_node, "DATA_PRESET": {"CENTER_IDX": 9}, "DEVICE": str(device),
                  "DLT_CONFIDENCE": dlt_confidence, "DLT_CONFIDENCE_THRESHOLD": dlt_threshold, "DLT_INLIER_PX": dlt_inlier_px,
                  "DLT_REFINE_ITERS": dlt_refine}
    if losses is not None:
        model_node["LOSS"] = loss_node(cfg)
    if mano_assets:
        model_node["MANO_ASSETS"] = mano_assets
    fit_acc = None
    if fit_mano_iters is not None:
        if not mano_assets:
            raise SystemExit("--fit-mano needs the MANO assets: pass --mano-assets FILE.npz")
        model_node["FIT_MANO"], model_node["FIT_MANO_ITERS"] = True, int(fit_mano_iters)
        if fit_mano_keypoints > 0:
            model_node["FIT_MANO_KEYPOINTS"] = float(fit_mano_keypoints)
        fit_acc = ManoFitStats(device)
    if backbone_engine != "torch":
        model_node["BACKBONE"] = {"ENGINE": backbone_engine}
    if backbone != "hrnet":
        kind = BACKBONE_TYPES[backbone]
        model_node["BACKBONE"] = dict(model_node.get("BACKBONE", {}), TYPE=kind, PRETRAINED=False, FREEZE_BATCHNORM=True)
        head_node["IN_CHANNELS"] = pk.model.head_in_channels(pk.BACKBONE.get(kind)().name)
    model = pk.build_model(pk.CN(model_node))
    if losses is not None:
        model.set_j_regressor(losses)
    if reload:
        sd = torch.load(reload, map_location="cpu")
        model.load_state_dict(sd.get("state_dict", sd.get("model", sd)) if isinstance(sd, dict) else sd)
        template_source = install_template(model.ptEmb_head, reload, template, mano_assets)
    else:
        template_source = f"file:{template}" if template else f"mano-assets:{mano_assets}" if mano_assets else "synthetic(seed=1234)"
        from poem_v2_amd.backbone import seeded_hrnet_state_dict
        from poem_v2_amd.resnet import seeded_resnet_state_dict
        net = model.img_backbone
        model.load_parts(seeded_hrnet_state_dict(0) if net.name == "HRNet" else seeded_resnet_state_dict(net.version, 0),
                         pk.weights.seeded_decoder_state_dict(0, backbone=net.name),
                         pk.weights.seeded_state_dict(model.ptEmb_head.embed_dims, seed=0, in_channels=model.ptEmb_head.in_channels,
                                                      parametric=model.ptEmb_head.parametric_output),
                         template=load_template(template) if template else None if mano_assets
                         else pk.inputs.synthetic_template(1234))
    if model.ptEmb_head.parametric_output and not mano_assets:
        raise SystemExit("medium_MANO needs a MANO layer (licence-gated assets): pass --mano-assets FILE.npz")
    mpvpe, mpjpe = MeanEPE("verts", device=device), MeanEPE("joints", device=device)
    bench_scores = BenchmarkScores(device) if benchmark_scores else None
    inlier_acc = InlierFraction(device) if dlt_confidence == "ransac" else None
    n, t0, frames, steps, t_draw = 0, None, [], [0], [0.0]

    def run(frames):
        batch = pk.collation_random_n_views(frames, transform=dset.transform)
        if min(batch["cam_view_num"]) < 2 <= max(batch["cam_view_num"]):
            return 0                                         # upstream has no DLT answer for such a mix either
        preds = model(batch, 0, mode="test")
        gj = batch["master_joints_3d"].reshape(-1, 21, 3).to(device)     # the collation concatenates per-frame (21,3) arrays
        gv = batch["master_verts_3d"].reshape(-1, 778, 3).to(device)
        mpjpe.feed(preds["pred_joints_3d"], gj)
        mpvpe.feed(preds["pred_verts_3d"], gv)
        if inlier_acc is not None and "pred_joints_inlier" in preds:      # (absent when every sample has one view: no DLT)
            inlier_acc.feed(preds["pred_joints_inlier"])
        if bench_scores is not None:
            bench_scores.feed(preds["pred_joints_3d"], gj, preds["pred_verts_3d"], gv)
        if fit_acc is not None:
            gt_betas = None
            if batch.get("mano_shape", None) is not None:              # per view; the master view's row is the sample's
                ms = batch["mano_shape"]
                ms = (ms if torch.is_tensor(ms) else torch.as_tensor(np.asarray(ms))).reshape(-1, 10).to(device)
                gt_betas = ms[master_rows(batch).to(device)]
            fit_acc.feed(preds["pred_mano_verts"], preds["pred_verts_3d"], preds["pred_mano_status"], preds["pred_mano_shape"], gt_betas)
            if "pred_mano_joints" in preds:
                fit_acc.feed_reproj(preds["pred_mano_joints"], preds["pred_joints_uv"], preds["pred_mano_keypoint_weight"],
                                    batch["target_cam_intr"].reshape(-1, 3, 3).to(device), batch["target_cam_extr"].reshape(-1, 4, 4).to(device),
                                    batch["cam_view_num"], preds["pred_mano_status"])
        if losses is not None:                             # one launch + finalize, sums stay on the device (POEM.py:476,483 upstream)
            model.loss_metric.feed(model.compute_loss(preds, batch)[1], len(frames))
        if draw is not None:                               # kept out of samples/s, as in evaluate()
            torch.cuda.synchronize(device)
            t_d = time.perf_counter()
            draw(preds, batch, steps[0])
            torch.cuda.synchronize(device)
            t_draw[0] += (time.perf_counter() - t_d) if t0 is not None else 0.0
        steps[0] += 1
        return len(frames)

    for f in dset:
        frames.append(f)
        if len(frames) == batch_size:
            done = run(frames)
            frames = []
            if t0 is None:
                torch.cuda.synchronize(device)
                t0 = time.perf_counter()
            else:
                n += done
    if frames:
        n += run(frames)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0 - t_draw[0] if t0 else 0.0
    mpvpe.reduce(), mpjpe.reduce()
    res = {"dataset_source": f"record shards {pattern} (synthetic records)", "scope": "shards->images->verts",
           "model": model_type, "view_range": list(view_range), "samples": int(mpvpe.acc[1].item()),
           "MPVPE_mm_vs_record_gt": mpvpe.result() * 1e3, "MPJPE_mm_vs_record_gt": mpjpe.result() * 1e3,
           "samples_per_s_rank0": (n / dt) if dt > 0 and n else None, "world_size": world,
           "template_source": template_source}
    if losses is not None:
        res["losses"] = model.loss_metric.reduce().get_measures()
    if bench_scores is not None:
        res["benchmark"] = bench_scores.result()
    if inlier_acc is not None:
        res["dlt_inlier_fraction"] = inlier_acc.result()
    if fit_acc is not None:
        res.update(fit_acc.result(reproj=fit_mano_keypoints > 0))
    if image_decode in ("device", "device-entropy"):
        counts = pk.transform.jpeg_counts()
        seen = counts["taken"] + counts["refused"]
        res["jpeg_device_fraction"] = counts["taken"] / seen if seen else None      # None: the shards hold no JPEG view
    return res


def main(args):
    view_range = [args.view_min, args.view_max]
    check_losses_args(args)
    mano_assets = getattr(args, "mano_assets", None)          # (absent from a build_parser() namespace)
    robust = dict(dlt_inlier_px=getattr(args, "dlt_inlier_px", 8.0), dlt_refine=getattr(args, "dlt_refine", 0))
    if getattr(args, "fit_mano", False):                     # (both absent from a build_parser() namespace)
        robust["fit_mano_iters"] = int(getattr(args, "fit_mano_iters", 8))
        if not 0 <= robust["fit_mano_iters"] <= 64:
            raise SystemExit(f"--fit-mano-iters {robust['fit_mano_iters']}: expected 0..64")
    if hasattr(args, "fit_mano_keypoints"):                  # (absent from the namespace unless given)
        w2d = float(args.fit_mano_keypoints)
        if not getattr(args, "fit_mano", False) or not np.isfinite(w2d) or w2d < 0:
            raise SystemExit(f"--fit-mano-keypoints {w2d}: needs --fit-mano and a finite weight >= 0")
        robust["fit_mano_keypoints"] = w2d
    if args.cfg and os.path.exists(args.cfg):
        with open(args.cfg, "r") as f:
            cfg = yaml.load(f, Loader=yaml.FullLoader)
    else:
        cfg = default_cfg()
    view_range = edit_cfg(cfg, args.dataset, args.model, view_range)
    # upstream dumps the edited tree back to the same path from its single launcher process; under torch.distributed.run
    # every rank executes this script, so only rank 0 writes (via a rename: a concurrent reader sees the old or the new
    # file, never a truncated one) and the others keep their in-memory edit
    if args.cfg and int(os.environ.get("RANK", "0")) == 0:
        tmp = f"{args.cfg}.tmp{os.getpid()}"
        with open(tmp, "w") as f:
            yaml.dump(cfg, f)
        os.replace(tmp, args.cfg)
    rank, local_rank, world = pdist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("eval_single.py needs a GPU: the head runs on the MI355X HIP path only (no CPU fallback)")
    device = torch.device("cuda", local_rank if world > 1 else args.gpu_id)
    torch.cuda.set_device(device)
    draw = None
    if args.draw and rank == 0:
        if args.faces:
            faces = np.load(args.faces)
            if faces.ndim != 2 or faces.shape[1] != 3 or not np.issubdtype(faces.dtype, np.integer):
                raise SystemExit(f"--faces: {args.faces} holds {faces.dtype} {faces.shape}, expected an (F,3) integer array")
            if faces.min() < 0 or faces.max() >= 778:
                raise SystemExit(f"--faces: vertex ids must lie in [0, 778), found [{faces.min()}, {faces.max()}]")
            draw = pk.DrawingHandCallback(args.draw_dir, faces)
            print(f"--draw: panels [input | skeleton | mesh] per frame and view under {args.draw_dir}")
        else:
            print("--draw: the renderer needs the mesh topology: pass --faces FILE.npy, an (F,3) integer array (MANO's closed faces are "
                  "licence-gated, like the template: INTEGRATION.md); metrics only")
    j_regressor = None
    if args.losses:
        j_regressor = np.load(args.j_regressor)
        if j_regressor.shape != (16, 778):
            raise SystemExit(f"--j-regressor: {args.j_regressor} holds {j_regressor.dtype} {j_regressor.shape}, expected (16,778)")
    if args.shards:
        res = evaluate_shards(cfg, view_range, args.model, device, args.shards, args.dataset, reload=args.reload,
                              epoch_size=args.epoch_size, batch_size=args.batch_size, template=args.template,
                              dlt_confidence=args.dlt_confidence, dlt_threshold=args.dlt_threshold, draw=draw,
                              losses=j_regressor, mano_assets=mano_assets,
                              backbone_engine=getattr(args, "backbone_engine", "torch"),
                              backbone=getattr(args, "backbone", "hrnet"),
                              benchmark_scores=getattr(args, "benchmark_scores", False),
                              image_decode=getattr(args, "image_decode", "host"), **robust)
    else:
        res = evaluate(cfg, view_range, args.model, device, reload=args.reload, epoch_size=args.epoch_size,
                       batch_size=args.batch_size, pyramid=args.pyramid, template=args.template,
                       dlt_confidence=args.dlt_confidence, dlt_threshold=args.dlt_threshold, draw=draw, mano_assets=mano_assets,
                       benchmark_scores=getattr(args, "benchmark_scores", False), **robust)
    if rank == 0:
        exp_id = f"{args.dataset}_view_{view_range[0]}_{view_range[1]}_{args.model}"
        if args.model == "huge":
            # C = 1024 (dh = 256) is outside the widths the fused kernels are instantiated for (merge.hip / chain.hip: 128 / 256 /
            # 512): the head runs the round-1 operator sequence -- same results, ~100 samples/s at batch 8 instead of the
            # medium model's 1400 (not a BASELINE config; upstream's README lists only the other four models)
            res["note"] = "POEM-huge runs the operator sequence (no fused front end / chain kernels at embed 1024)"
        print(json.dumps({"exp_id": exp_id, **res}))
    if world > 1:
        torch.distributed.destroy_process_group()


def build_parser():
    parser = argparse.ArgumentParser(description="Eval Single Setting")
    parser.add_argument("--cfg", type=str, required=True, help="Path to the configuration file.")
    parser.add_argument("--dataset", type=str, required=True, help="Dataset name.")
    parser.add_argument("--view_min", type=int, required=True, help="Minimum view range.")
    parser.add_argument("--view_max", type=int, required=True, help="Maximum view range.")
    parser.add_argument("--model", type=str, required=True, help="Model category.")
    parser.add_argument("--gpu_id", "-g", type=int, default=0, required=True, help="GPU ID to run the evaluation.")
    parser.add_argument("--reload", type=str, default=None, help="Path to the checkpoint to reload.")
    parser.add_argument("--port", "-p", type=int, default=60000, help="Port to run the evaluation.")
    parser.add_argument("--draw", "-d", action="store_true", help="Visualize the results.")
    parser.add_argument("--epoch_size", type=int, default=64, help="Synthetic samples to evaluate (this build).")
    parser.add_argument("--pyramid", action="store_true",
                        help="start at the backbone's multi-level features: feat_decode + heatmap_stage on HIP (this build).")
    parser.add_argument("--shards", type=str, default=None, metavar="DIR",
                        help="evaluate the full model from record shards under DIR (the dataset's URLS pattern; synthetic "
                             "shards are written there when absent): tar records -> device transform -> model -> metrics")
    parser.add_argument("--template", type=str, default=None, metavar="FILE",
                        help="(799,3) zero-pose hand template (.npy / .pt; ManoLayer's zero-pose joints + vertices, centred at "
                             "joint 9).  With --reload either this or --mano-assets is required; synthetic otherwise (this build).")
    parser.add_argument("--dlt-confidence", choices=("off", "threshold", "weighted", "ransac"), default="off",
                        help="Discount views by their heat-map peak in the DLT of the reference joints (model key DLT_CONFIDENCE; "
                             "threshold = upstream's triangulate_dlt), or (ransac, no upstream counterpart) leave out the views that "
                             "disagree with the geometry of the others.  Needs --pyramid or --shards.")
    parser.add_argument("--dlt-threshold", type=float, default=0.5, help="confi_thres of --dlt-confidence threshold.")
    parser.add_argument("--batch_size", type=int, default=2, help="--val_batch_size of the reference (lib/opt.py:27-30).")
    parser.add_argument("--faces", type=str, default=None, metavar="FILE.npy",
                        help="(F,3) integer array of the mesh's triangles (on a licensed machine: ManoLayer.get_mano_closed_faces()); "
                             "with --draw the predicted and ground-truth meshes are rendered into every view on the device.")
    parser.add_argument("--draw-dir", type=str, default="./draw", help="where --draw writes its panels.")
    parser.add_argument("--losses", action="store_true",
                        help="with --shards: evaluate upstream's loss terms (compute_loss, value only) on the device for every batch and "
                             "add their averages to the result line.  Needs --j-regressor.")
    parser.add_argument("--j-regressor", type=str, default=None, metavar="FILE.npy",
                        help="(16,778) float array: MANO's th_J_regressor (on a licensed machine: ManoLayer.th_J_regressor), read by "
                             "loss_3d_joints_from_mesh.")
    return parser


def build_cli():
    """``build_parser()`` -- the argument surface the host tests pin key by key -- plus the arguments added since."""
    parser = build_parser()
    parser.add_argument("--mano-assets", type=str, default=None, metavar="FILE.npz",
                        help="MANO's five arrays (v_template, shapedirs, posedirs, J_regressor, weights; on a licensed machine: the fields "
                             "of MANO_RIGHT.pkl).  The head takes its zero-pose template and, for medium_MANO, its MANO layer from them: "
                             "--reload needs no --template, and medium_MANO runs (head config key MANO_ASSETS).")
    # (absent from the namespace unless given: the host tests pin the namespace of a plain command line key by key)
    parser.add_argument("--backbone-engine", choices=("torch", "hip"), default=argparse.SUPPRESS,
                        help="with --shards: what runs HRNet-W40 -- torch (PyTorch-ROCm / MIOpen, the default) or hip (the project's own "
                             "gfx950 convolution kernels; model key BACKBONE.ENGINE).  The other scopes start behind the backbone.")
    parser.add_argument("--backbone", choices=tuple(BACKBONE_TYPES), default=argparse.SUPPRESS,
                        help="with --shards: the image backbone (default hrnet); sets MODEL.BACKBONE.TYPE and MODEL.HEAD.IN_CHANNELS "
                             "(160 / 128 / 512).")
    parser.add_argument("--dlt-inlier-px", type=float, default=argparse.SUPPRESS,
                        help="--dlt-confidence ransac: the inlier radius in image pixels (model key DLT_INLIER_PX; default 8.0 = two "
                             "heat-map pixels at 256^2 images with 64^2 maps -- not measured on real data).")
    parser.add_argument("--dlt-refine", type=int, default=argparse.SUPPRESS,
                        help="--dlt-confidence ransac: Gauss-Newton steps on the reprojection error after the refit, 0..16 (model key "
                             "DLT_REFINE_ITERS; default 0).  The result line gains \"dlt_inlier_fraction\".")
    parser.add_argument("--benchmark-scores", action="store_true", default=argparse.SUPPRESS,
                        help="add a \"benchmark\" block to the result line: the FreiHAND / HO3D leaderboard numbers -- mesh F@5 / F@15, raw "
                             "and Procrustes-aligned (PA_), the AUC of the aligned joints / vertices over 0..50 mm (pa_auc_j / pa_auc_v) "
                             "and the symmetric mean nearest-vertex distance (chamfer_mm) -- computed on the device.")
    parser.add_argument("--fit-mano", action="store_true", default=argparse.SUPPRESS,
                        help="fit MANO pose, shape and translation to every predicted mesh on the device (Levenberg-Marquardt, "
                             "poem_v2_amd.fit_mano; model keys FIT_MANO / FIT_MANO_ITERS).  Needs --mano-assets.  The result line gains "
                             "mano_fit_residual_mm (mean vertex distance fitted - predicted), mano_fit_flagged and, where the records "
                             "carry ground-truth fits, mano_fit_betas_mae.")
    parser.add_argument("--fit-mano-iters", type=int, default=argparse.SUPPRESS, help="--fit-mano: LM iterations, 0..64 (default 8).")
    parser.add_argument("--fit-mano-keypoints", type=float, default=argparse.SUPPRESS, metavar="W",
                        help="--fit-mano: also fit the 21 joints to the 2-D joints of every view with weight W (times the confidences / the "
                             "RANSAC inlier mask where the DLT mode has them; model key FIT_MANO_KEYPOINTS).  The result line gains "
                             "mano_fit_reproj_px: the mean pixel distance between the fitted joints' projections and those 2-D joints.  "
                             "The useful range of W on real data has not been measured.")
    parser.add_argument("--image-decode", choices=("host", "device", "device-entropy"), default=argparse.SUPPRESS,
                        help="with --shards: who decodes the records' JPEG views -- host (PIL, the default) or device (Huffman decoding on "
                             "host threads, inverse DCT / up-sampling / colour on the GPU, bit-equal to PIL; a stream the device route "
                             "refuses falls back to PIL) or device-entropy (device, with the Huffman decoding on the GPU too).  Both device "
                             "routes add jpeg_device_fraction to the result line.")
    return parser


if __name__ == "__main__":
    main(build_cli().parse_args())
