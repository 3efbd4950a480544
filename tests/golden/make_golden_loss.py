"""Golden data for the loss terms from the upstream reference (build container only, like make_golden.py): upstream's OWN
``PtEmbedMultiviewStereoV2.compute_loss`` (lib/models/POEM.py:363-466), imported through ``ref_harness.setup()`` and called unbound on a
plain namespace that carries what the method reads -- the weights, the ``torch.nn`` criteria, ``mano_layer.th_J_regressor``,
``loss_proj_to_multicam``, ``num_joints``, ``parametric_output`` and ``transformer_center_idx``.

Inputs per case: cameras and ground-truth joints from ``poem_v2_amd.inputs.synthetic_batch``; ground-truth vertices = the centre joint
+ 0.05 N(0,1); predictions = ground truth + 4 mm noise (10-12 mm where the joints' criterion is L1 or the batch is one sample: see BAR32); 2-D targets = the projected joints + 1 px, predicted 2-D joints = targets + 2 px;
a seeded, positive, row-normalised 16 x 778 regressor.  Per case the file holds the fp32 inputs, upstream's fp32 ``loss_dict`` (``ref32``)
and the same terms evaluated here in fp64 (``ref64``): a dense torch expression without a loop over samples, with upstream's own
``mano_to_openpose`` on fp64 copies.  tests/test_loss_host.py holds ``ref32`` against ``ref64`` (2e-6 relative): that is what makes the
fp64 values a stand-in for the reference.

  release   views [3,1,4], release weights, 256 x 256: a single-view sample inside a ragged batch; no loss_2d_verts key
  allterms  views [2,10,1,5], VERTICES_2D_LOSS_WEIGHT 0.5, parametric, joints L1 / vertices L2, 320 x 240: every key
  clamp     views [4,2], targets uniform in the image, predictions projecting elsewhere: 10..90 % of the offsets clamped (asserted)
  zplane    one view, identity extrinsic, one predicted joint at z = 0 exactly: the |z| < 1e-7 rule, in fp32 and in fp64 alike
  single    views [1]
  many      views [1..9] (BN = 45), all terms: many blocks, several block groups
  nan       release with one predicted joint coordinate NaN: upstream's NaN pattern

  python tests/golden/make_golden_loss.py   ->  tests/golden/loss.npz   (byte for byte: the archive carries no time stamps)"""
import io
import json
import math
import os
import sys
import types
import zipfile

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path[:0] = [ROOT, GOLDEN]
sys.dont_write_bytecode = True

import ref_harness as rh  # noqa: E402
from poem_v2_amd.inputs import synthetic_batch  # noqa: E402

RELEASE = dict(JOINTS_LOSS_TYPE="l2", VERTICES_LOSS_TYPE="l1", HEATMAP_JOINTS_WEIGHT=10.0, TRIANGULATED_JOINTS_WEIGHT=10.0,
               JOINTS_LOSS_WEIGHT=1.0, VERTICES_LOSS_WEIGHT=1.0, JOINTS_2D_LOSS_WEIGHT=1.0, VERTICES_2D_LOSS_WEIGHT=0.0,
               EDGE_LOSS_WEIGHT=0.0)                                    # config/release/train_medium.yaml:226-235
ALLTERMS = dict(RELEASE, JOINTS_LOSS_TYPE="l1", VERTICES_LOSS_TYPE="l2", VERTICES_2D_LOSS_WEIGHT=0.5)
# upstream's fp32 value against the fp64 evaluation, relative.  loss_3d_joints_from_mesh cancels most -- regressed joints at 0.6 m that
# differ by the noise averaged over a joint's vertices -- and an L1 criterion does not average its round-off away: those cases draw 10 mm
BAR32 = 2e-6


def regressor(seed=7):
    g = torch.Generator().manual_seed(seed)
    w = torch.exp(3.0 * torch.randn(16, 778, generator=g))      # a few vertices carry a joint, as in MANO's sparse regressor
    return (w / w.sum(dim=1, keepdim=True)).float()


def draw_case(views, seed, H=256, W=256, noise=0.004):
    """The fp32 inputs of one case as a dict of tensors."""
    b = synthetic_batch(views, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    B, BN = len(views), sum(views)
    K = b["img_metas"]["cam_intr"].clone()
    K[:, 0, 2], K[:, 1, 2] = W / 2, H / 2
    E = b["img_metas"]["cam_extr"]
    gj = b["reference_joints"]
    gv = gj[:, 9:10] + 0.05 * torch.randn(B, 778, 3, generator=g)
    coords = torch.cat([gj, gv], 1) + noise * torch.randn(B, 799, 3, generator=g)
    vs = torch.repeat_interleave(torch.arange(B), torch.tensor(views))
    T = torch.linalg.inv(E.double())
    cam = gj.double()[vs] @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]
    h = cam @ K.double().transpose(1, 2)
    gt_uv = (h[..., :2] / h[..., 2:] + torch.randn(BN, 21, 2, generator=g).double()).float()
    pred_uv = gt_uv + 2.0 * torch.randn(BN, 21, 2, generator=g)
    mano_pose = 0.1 * torch.randn(BN, 16, 3, generator=g)
    mano_shape = 0.1 * torch.randn(BN, 10, generator=g)
    first = torch.tensor(np.concatenate([[0], np.cumsum(views)])[:-1])
    pred_pose = mano_pose[first] + 0.05 * torch.randn(B, 16, 3, generator=g)
    pred_shape = mano_shape[first] + 0.05 * torch.randn(B, 10, generator=g)
    return dict(coords=coords.float(), pred_uv=pred_uv, pred_pose=pred_pose, pred_shape=pred_shape, gt_joints=gj.float(),
                gt_verts=gv.float(), gt_uv=gt_uv, K=K.float(), E=E.float(), mano_pose=mano_pose, mano_shape=mano_shape)


def run_upstream(POEM, inp, views, loss, parametric, center_idx, H, W, jreg):
    """upstream's compute_loss, unbound, on a namespace -> its fp32 loss_dict as {key: float32}."""
    l1, l2 = torch.nn.L1Loss, torch.nn.MSELoss
    ns = types.SimpleNamespace(
        joints_weight=loss["JOINTS_LOSS_WEIGHT"], vertices_weight=loss["VERTICES_LOSS_WEIGHT"],
        joints_2d_weight=loss["JOINTS_2D_LOSS_WEIGHT"], heatmap_joints_weights=loss["HEATMAP_JOINTS_WEIGHT"],
        vertices_2d_weight=loss.get("VERTICES_2D_LOSS_WEIGHT", 0.0), pose_weight=loss.get("POSE_LOSS_WEIGHT", 0.001),
        shape_weight=loss.get("SHAPE_LOSS_WEIGHT", 0.0005),
        criterion_joints=(l2 if loss.get("JOINTS_LOSS_TYPE", "l2") == "l2" else l1)(),
        criterion_vertices=(l2 if loss.get("VERTICES_LOSS_TYPE", "l1") == "l2" else l1)(), criterion_parameters=l2(),
        mano_layer=types.SimpleNamespace(th_J_regressor=jreg), loss_proj_to_multicam=POEM.loss_proj_to_multicam, num_joints=21,
        parametric_output=parametric, transformer_center_idx=center_idx)
    BN = sum(views)
    preds = {"all_coords_preds": inp["coords"][None].clone(), "pred_joints_uv": inp["pred_uv"].clone(),
             "pred_pose": inp["pred_pose"].clone(), "pred_shape": inp["pred_shape"].clone()}
    gt = {"cam_view_num": np.asarray(views, dtype=np.int64), "image": torch.zeros(1).expand(BN, 3, H, W), "master_joints_3d": inp["gt_joints"].clone(),
          "master_verts_3d": inp["gt_verts"].clone(), "target_joints_2d": inp["gt_uv"].clone(), "target_cam_intr": inp["K"].clone(),
          "target_cam_extr": inp["E"].clone(), "mano_pose": inp["mano_pose"].clone(), "mano_shape": inp["mano_shape"].clone()}
    with torch.no_grad():
        loss_v, d = POEM.compute_loss(ns, preds, gt)
    assert d["loss"] is loss_v
    assert all(v.dtype == torch.float32 for v in d.values())
    return {k: np.float32(v.item()) for k, v in d.items()}


def dense64(mano_to_openpose, inp, views, loss, parametric, center_idx, H, W, jreg):
    """The same terms in fp64, dense over the batch (no loop over samples) -> ({key: float}, share of clamped joint offsets)."""
    d = {k: v.double() for k, v in inp.items()}
    B = len(views)
    s = math.sqrt(float(W ** 2 + H ** 2))
    vs = torch.repeat_interleave(torch.arange(B), torch.tensor(views))
    T = torch.linalg.inv(d["E"])
    pj, pv = d["coords"][:, :21], d["coords"][:, 21:]

    def proj(P):
        cam = P[vs] @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]
        h = cam @ d["K"].transpose(1, 2)
        z = h[..., 2:].clone()
        z[z.abs() < 1e-7] = 1e-7
        return h[..., :2] / z

    def offset(a, b):
        raw = a - b
        o = torch.clamp(raw, min=-.5 * s, max=.5 * s) / s
        return (o ** 2).sum(-1).mean(), float((raw.abs() > .5 * s).double().mean())

    cj = (lambda a, b: ((a - b) ** 2).mean()) if loss.get("JOINTS_LOSS_TYPE", "l2") == "l2" else (lambda a, b: (a - b).abs().mean())
    cv = (lambda a, b: ((a - b) ** 2).mean()) if loss.get("VERTICES_LOSS_TYPE", "l1") == "l2" else (lambda a, b: (a - b).abs().mean())
    out = {"loss_heatmap_joints": (((d["pred_uv"] - d["gt_uv"]) / s) ** 2).sum(-1).mean()}
    out["loss_3d_joints"] = cj(pj, d["gt_joints"])
    out["loss_3d_joints_from_mesh"] = cj(mano_to_openpose(jreg.double(), pv), mano_to_openpose(jreg.double(), d["gt_verts"]))
    if parametric:
        c = d["gt_joints"][:, center_idx:center_idx + 1]
        out["loss_3d_verts"] = cv(pv - c, d["gt_verts"] - c)
    else:
        out["loss_3d_verts"] = cv(pv, d["gt_verts"])
    recon = loss["JOINTS_LOSS_WEIGHT"] * (out["loss_3d_joints"] + out["loss_3d_joints_from_mesh"])
    recon = recon + loss["VERTICES_LOSS_WEIGHT"] * out["loss_3d_verts"]
    clamped = 0.0
    l2j = l2v = lp = ls = torch.zeros((), dtype=torch.float64)
    if loss["JOINTS_2D_LOSS_WEIGHT"] != 0:
        l2j, clamped = offset(proj(pj), d["gt_uv"])
    if loss.get("VERTICES_2D_LOSS_WEIGHT", 0.0) != 0:
        l2v, _ = offset(proj(pv), proj(d["gt_verts"]))
    if parametric:
        first = torch.tensor(np.concatenate([[0], np.cumsum(views)])[:-1])
        lp = ((d["pred_pose"] - d["mano_pose"][first]) ** 2).mean()
        ls = ((d["pred_shape"] - d["mano_shape"][first]) ** 2).mean()
    recon = recon + loss["JOINTS_2D_LOSS_WEIGHT"] * l2j
    recon = recon + loss.get("VERTICES_2D_LOSS_WEIGHT", 0.0) * l2v
    recon = recon + (loss.get("POSE_LOSS_WEIGHT", 0.001) * lp + loss.get("SHAPE_LOSS_WEIGHT", 0.0005) * ls)
    out["loss_recon"] = recon
    if loss["JOINTS_2D_LOSS_WEIGHT"] != 0:
        out["loss_2d_joints"] = l2j
    if loss.get("VERTICES_2D_LOSS_WEIGHT", 0.0) != 0:
        out["loss_2d_verts"] = l2v
    if parametric:
        out["loss_pose"], out["loss_shape"] = lp, ls
    out["loss"] = loss["HEATMAP_JOINTS_WEIGHT"] * out["loss_heatmap_joints"] + recon
    return {k: float(v) for k, v in out.items()}, clamped


def build():
    """-> {name: array} of the fixture (tests/test_loss_host.py calls this to check that loss.npz regenerates)."""
    rh.setup()
    from lib.models.POEM import PtEmbedMultiviewStereoV2 as POEM
    from lib.utils.transform import mano_to_openpose
    jreg = regressor()
    rec, meta = {"jreg": jreg.numpy()}, {}

    def record(name, inp, views, loss, parametric=False, center_idx=9, H=256, W=256, **extra):
        ref32 = run_upstream(POEM, inp, views, loss, parametric, center_idx, H, W, jreg)
        ref64, clamped = dense64(mano_to_openpose, inp, views, loss, parametric, center_idx, H, W, jreg)
        keys = list(ref32)
        assert keys == list(ref64), (keys, list(ref64))
        a32, a64 = np.array([ref32[k] for k in keys], np.float32), np.array([ref64[k] for k in keys], np.float64)
        assert (np.isnan(a32) == np.isnan(a64)).all(), (name, a32, a64)
        fin = ~np.isnan(a64)
        rel = np.abs(a32[fin].astype(np.float64) - a64[fin]) / np.abs(a64[fin])
        worst = dict(zip([k for k, f in zip(keys, fin) if f], [f"{r:.1e}" for r in rel]))
        assert rel.max() <= BAR32, f"{name}: upstream's fp32 value is too far from the fp64 one: redraw with a larger noise ({worst})"
        for k, v in inp.items():
            if parametric or k not in ("pred_pose", "pred_shape", "mano_pose", "mano_shape"):
                rec[f"{name}.{k}"] = v.numpy()
        rec[f"{name}.ref32"], rec[f"{name}.ref64"] = a32, a64
        meta[name] = dict(views=[int(v) for v in views], loss=loss, parametric=parametric, center_idx=center_idx, H=H, W=W, keys=keys,
                          nan_keys=[k for k, f in zip(keys, fin) if not f], clamped=clamped, **extra)
        print(f"{name}: views {views}  keys {len(keys)}  worst fp32-vs-fp64 {rel.max():.2e}  clamped {clamped:.2f}  "
              f"nan {meta[name]['nan_keys']}")
        return clamped

    views = [3, 1, 4]
    release = draw_case(views, 61)
    record("release", release, views, RELEASE)

    views = [2, 10, 1, 5]
    record("allterms", draw_case(views, 62, H=240, W=320, noise=0.01), views, ALLTERMS, parametric=True, H=240, W=320)

    # targets uniform in the image, predictions a hand's breadth off: the +-scale/2 clamp engages on a good share of the offsets
    views = [4, 2]
    inp = draw_case(views, 63)
    g = torch.Generator().manual_seed(163)
    inp["gt_uv"] = 256.0 * torch.rand(sum(views), 21, 2, generator=g)
    inp["coords"][:, :21] += torch.tensor([0.30, -0.25, 0.0])
    clamped = record("clamp", inp, views, RELEASE)
    assert 0.10 <= clamped <= 0.90, clamped

    # one view, identity extrinsic, K's last row (0,0,1): a predicted joint with z = 0 exactly projects to z = 0 in fp32 and fp64 alike
    views = [1]
    inp = draw_case(views, 64, noise=0.012)
    assert torch.equal(inp["E"][0], torch.eye(4)) and inp["K"][0, 2].tolist() == [0.0, 0.0, 1.0]
    inp["coords"][0, 3] = torch.tensor([0.01, 0.02, 0.0])
    record("zplane", inp, views, RELEASE)

    record("single", draw_case([1], 65, noise=0.012), [1], RELEASE)

    views = list(range(1, 10))
    record("many", draw_case(views, 66, noise=0.01), views, dict(ALLTERMS))

    views = [3, 1, 4]
    inp = {k: v.clone() for k, v in release.items()}
    inp["coords"][1, 5, 2] = float("nan")
    record("nan", inp, views, RELEASE, nan_at=[1, 5, 2])
    assert meta["nan"]["nan_keys"] == ["loss_3d_joints", "loss_recon", "loss_2d_joints", "loss"], meta["nan"]["nan_keys"]

    rec["meta"] = np.frombuffer(json.dumps(dict(cases=meta, bar32=BAR32), sort_keys=True).encode(), dtype=np.uint8)
    return rec


def save(path, rec):
    """np.savez_compressed without the archive's time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in rec.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


if __name__ == "__main__":
    rec = build()
    path = os.path.join(GOLDEN, "loss.npz")
    save(path, rec)
    print(f"loss: {len(rec) - 1} arrays, {os.path.getsize(path) / 1e3:.0f} kB")
