"""The loss terms on the host (no GPU): the fixture tests/golden/loss.npz -- upstream's own ``compute_loss`` in fp32 next to an fp64
evaluation of the same terms (tests/golden/make_golden_loss.py) -- an fp64 restatement of every term written HERE, and the host side
of ``PoemLoss`` / ``LossMetric`` / ``eval_single.py --losses``.

``restate`` shares nothing with the kernel and nothing with the generator's dense expression: plain numpy, one sample and one view
at a time, in upstream's order of operations.  It reproduces the fixture's fp64 values to 1e-12 and is the GPU tests' yardstick
(tests/test_loss.py) for inputs that are not in the fixture."""
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("release", "allterms", "clamp", "zplane", "single", "many", "nan")
INPUT_KEYS = ("coords", "pred_uv", "pred_pose", "pred_shape", "gt_joints", "gt_verts", "gt_uv", "K", "E", "mano_pose", "mano_shape")
ALL_KEYS = ["loss_heatmap_joints", "loss_3d_joints", "loss_3d_joints_from_mesh", "loss_3d_verts", "loss_recon", "loss_2d_joints",
            "loss_2d_verts", "loss_pose", "loss_shape", "loss"]                  # upstream's order (lib/models/POEM.py:380,451-465)
# mano_to_openpose (lib/utils/transform.py:864-869 upstream; CONST.MANO_KPID_2_VERTICES, lib/utils/misc.py:76-82)
TIPS = [744, 320, 443, 555, 672]
OPENPOSE = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]

_FIXTURE = []


def fixture():
    """-> (cases: {name: dict(meta fields, inp={key: fp32 array}, ref32, ref64)}, jreg (16,778) fp32); loaded once."""
    if not _FIXTURE:
        z = np.load(os.path.join(GOLDEN, "loss.npz"))
        meta = json.loads(bytes(z["meta"]).decode())
        cases = {}
        for name, m in meta["cases"].items():
            c = dict(m)
            c["inp"] = {k: z[f"{name}.{k}"] for k in INPUT_KEYS if f"{name}.{k}" in z.files}
            c["ref32"], c["ref64"] = z[f"{name}.ref32"], z[f"{name}.ref64"]
            cases[name] = c
        _FIXTURE.append((cases, z["jreg"], meta))
    return _FIXTURE[0][0], _FIXTURE[0][1]


def restate(inp, views, loss, parametric, center_idx, H, W, jreg):
    """Every term of upstream's compute_loss in fp64 numpy, sample by sample and view by view -> {key: float} in upstream's order."""
    x = {k: np.asarray(v, dtype=np.float64) for k, v in inp.items()}
    J = np.asarray(jreg, dtype=np.float64)
    B, offs = len(views), np.concatenate([[0], np.cumsum(views)]).astype(int)
    BN = int(offs[-1])
    scale = math.sqrt(float(W ** 2 + H ** 2))
    w2j, w2v = loss["JOINTS_2D_LOSS_WEIGHT"], loss.get("VERTICES_2D_LOSS_WEIGHT", 0.0)
    jl2, vl2 = loss.get("JOINTS_LOSS_TYPE", "l2") == "l2", loss.get("VERTICES_LOSS_TYPE", "l1") == "l2"

    def openpose(verts):
        return np.concatenate([J @ verts, verts[TIPS]], 0)[OPENPOSE]

    def project(Tinv, K, pts):
        out = np.empty((len(pts), 2))
        for i, p in enumerate(pts):
            h = K @ (Tinv[:3, :3] @ p + Tinv[:3, 3])
            z = h[2]
            if abs(z) < 1e-7:                            # False for a NaN
                z = 1e-7
            out[i] = h[:2] / z
        return out

    def offsets_sq(a, b):
        d = a - b
        lo, hi = -.5 * scale, .5 * scale
        d = np.where(d < lo, lo, np.where(d > hi, hi, d)) / scale      # torch.clamp: a NaN stays
        return (d ** 2).sum(-1)

    s_hm = s_j = s_m = s_v = s_2j = s_2v = s_p = s_s = 0.0
    for b in range(B):
        pj, pv = x["coords"][b, :21], x["coords"][b, 21:]
        gj, gv = x["gt_joints"][b], x["gt_verts"][b]
        dj, dm = pj - gj, openpose(pv) - openpose(gv)
        s_j += (dj ** 2).sum() if jl2 else np.abs(dj).sum()
        s_m += (dm ** 2).sum() if jl2 else np.abs(dm).sum()
        dv = (pv - gj[center_idx]) - (gv - gj[center_idx]) if parametric else pv - gv
        s_v += (dv ** 2).sum() if vl2 else np.abs(dv).sum()
        if parametric:
            s_p += ((x["pred_pose"][b] - x["mano_pose"][offs[b]]) ** 2).sum()
            s_s += ((x["pred_shape"][b] - x["mano_shape"][offs[b]]) ** 2).sum()
        for v in range(offs[b], offs[b + 1]):
            s_hm += (((x["pred_uv"][v] - x["gt_uv"][v]) / scale) ** 2).sum()
            Tinv = np.linalg.inv(x["E"][v])
            if w2j != 0:
                s_2j += offsets_sq(project(Tinv, x["K"][v], pj), x["gt_uv"][v]).sum()
            if w2v != 0:
                s_2v += offsets_sq(project(Tinv, x["K"][v], pv), project(Tinv, x["K"][v], gv)).sum()
    t = {"loss_heatmap_joints": s_hm / (BN * 21), "loss_3d_joints": s_j / (B * 63), "loss_3d_joints_from_mesh": s_m / (B * 63),
         "loss_3d_verts": s_v / (B * 2334)}
    l2j, l2v = (s_2j / (BN * 21) if w2j != 0 else 0.0), (s_2v / (BN * 778) if w2v != 0 else 0.0)
    lp, ls = (s_p / (B * 48), s_s / (B * 10)) if parametric else (0.0, 0.0)
    recon = loss["JOINTS_LOSS_WEIGHT"] * (t["loss_3d_joints"] + t["loss_3d_joints_from_mesh"])
    recon += loss["VERTICES_LOSS_WEIGHT"] * t["loss_3d_verts"]
    recon += w2j * l2j
    recon += w2v * l2v
    recon += loss.get("POSE_LOSS_WEIGHT", 0.001) * lp + loss.get("SHAPE_LOSS_WEIGHT", 0.0005) * ls
    t["loss_recon"] = recon
    if w2j != 0:
        t["loss_2d_joints"] = l2j
    if w2v != 0:
        t["loss_2d_verts"] = l2v
    if parametric:
        t["loss_pose"], t["loss_shape"] = lp, ls
    t["loss"] = loss["HEATMAP_JOINTS_WEIGHT"] * t["loss_heatmap_joints"] + recon
    return {k: float(v) for k, v in t.items()}


def restate_case(c, jreg, inp=None):
    return restate(c["inp"] if inp is None else inp, c["views"], c["loss"], c["parametric"], c["center_idx"], c["H"], c["W"], jreg)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
def test_fixture_holds_every_case_and_its_purpose():
    cases, jreg = fixture()
    assert sorted(cases) == sorted(CASES)
    assert jreg.shape == (16, 778) and jreg.dtype == np.float32 and (jreg > 0).all() and np.allclose(jreg.sum(1), 1, atol=1e-5)
    assert cases["release"]["views"] == [3, 1, 4] and "loss_2d_verts" not in cases["release"]["keys"]
    assert cases["allterms"]["keys"] == ALL_KEYS and (cases["allterms"]["H"], cases["allterms"]["W"]) == (240, 320)
    assert 0.10 <= cases["clamp"]["clamped"] <= 0.90
    assert cases["zplane"]["views"] == [1] and np.array_equal(cases["zplane"]["inp"]["E"][0], np.eye(4, dtype=np.float32))
    assert (cases["zplane"]["inp"]["coords"][0, :21, 2] == 0).sum() == 1
    assert cases["many"]["views"] == list(range(1, 10))
    assert cases["nan"]["nan_keys"] == ["loss_3d_joints", "loss_recon", "loss_2d_joints", "loss"]
    for c in cases.values():
        assert all(a.dtype == np.float32 for a in c["inp"].values())
        assert c["ref32"].dtype == np.float32 and c["ref64"].dtype == np.float64 and len(c["ref32"]) == len(c["keys"]) == len(c["ref64"])
        assert c["keys"] == [k for k in ALL_KEYS if k in c["keys"]]              # upstream's order


@pytest.mark.parametrize("name", CASES)
def test_upstream_fp32_agrees_with_the_fp64_values(name):
    """What makes the fp64 values a stand-in for the reference: on every finite term, 2e-6 relative."""
    c = fixture()[0][name]
    fin = ~np.isnan(c["ref64"])
    assert (np.isnan(c["ref32"]) == ~fin).all()
    rel = np.abs(c["ref32"][fin].astype(np.float64) - c["ref64"][fin]) / np.abs(c["ref64"][fin])
    print(name, dict(zip(np.array(c["keys"])[fin], rel)))
    assert rel.max() <= 2e-6


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_fp64_values(name):
    cases, jreg = fixture()
    c = cases[name]
    got = restate_case(c, jreg)
    assert list(got) == c["keys"]
    for k, ref in zip(c["keys"], c["ref64"]):
        if k in c["nan_keys"]:
            assert math.isnan(got[k]) and math.isnan(ref), k
        else:
            assert abs(got[k] - ref) <= 1e-12 * abs(ref), (k, got[k], ref)


def test_fixture_regenerates_from_its_generator(tmp_path):
    spec = importlib.util.spec_from_file_location("make_golden_loss", os.path.join(GOLDEN, "make_golden_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    cwd = os.getcwd()
    try:
        spec.loader.exec_module(mod)
        if not os.path.isdir(mod.rh.REF_ROOT):
            pytest.skip("reference tree absent: golden vectors regenerate in the build container only")
        mod.save(str(tmp_path / "loss.npz"), mod.build())
    finally:
        os.chdir(cwd)
    assert (tmp_path / "loss.npz").read_bytes() == open(os.path.join(GOLDEN, "loss.npz"), "rb").read()


# ---- PoemLoss on the host ---------------------------------------------------------------------------------------------------------
def _poem_loss(c, jreg=None):
    import poem_v2_amd as pk
    return pk.PoemLoss(pk.CN(c["loss"]), parametric=c["parametric"], transformer_center_idx=c["center_idx"], j_regressor=jreg)


def test_poem_loss_keys_follow_the_configuration():
    import poem_v2_amd as pk
    cases, _ = fixture()
    for c in cases.values():
        assert _poem_loss(c).keys() == c["keys"]
    assert pk.losses.LOSS_KEYS == tuple(ALL_KEYS)
    no2d = pk.PoemLoss(pk.configs.loss_cfg(JOINTS_2D_LOSS_WEIGHT=0.0))
    assert no2d.keys() == ["loss_heatmap_joints", "loss_3d_joints", "loss_3d_joints_from_mesh", "loss_3d_verts", "loss_recon", "loss"]


def test_poem_loss_reads_upstreams_keys_with_upstreams_defaults():
    import poem_v2_amd as pk
    req = dict(JOINTS_LOSS_WEIGHT=2.0, VERTICES_LOSS_WEIGHT=3.0, JOINTS_2D_LOSS_WEIGHT=4.0, HEATMAP_JOINTS_WEIGHT=5.0)
    lo = pk.PoemLoss(pk.CN(req))
    assert (lo.joints_loss_type, lo.verts_loss_type) == ("l2", "l1")                         # POEM.py:41-42
    assert (lo.joints_weight, lo.vertices_weight, lo.joints_2d_weight, lo.heatmap_joints_weights) == (2.0, 3.0, 4.0, 5.0)
    assert (lo.vertices_2d_weight, lo.pose_weight, lo.shape_weight) == (0.0, 0.001, 0.0005)   # :129-131
    assert (lo.parametric_output, lo.transformer_center_idx) == (False, 9)
    for k in req:                                                                             # no default upstream either
        with pytest.raises(KeyError):
            pk.PoemLoss(pk.CN({a: b for a, b in req.items() if a != k}))
    rel = pk.configs.loss_cfg()                              # the release node; the two keys compute_loss never reads are accepted
    assert rel["TRIANGULATED_JOINTS_WEIGHT"] == 10.0 and rel["EDGE_LOSS_WEIGHT"] == 0.0
    r = pk.PoemLoss(rel)
    assert (r.heatmap_joints_weights, r.joints_weight, r.vertices_weight, r.joints_2d_weight, r.vertices_2d_weight) == (10.0, 1.0, 1.0, 1.0, 0.0)


def _dicts(c, device="cpu", layers=2):
    """(preds, gt) in upstream's layout from a fixture case; the earlier decoder layers hold numbers that must not be read."""
    t = {k: torch.from_numpy(v).to(device) for k, v in c["inp"].items()}
    BN = sum(c["views"])
    stack = torch.cat([torch.full((layers - 1,) + tuple(t["coords"].shape), 7.0, device=device), t["coords"][None]], 0)
    preds = {"all_coords_preds": stack, "pred_joints_uv": t["pred_uv"]}
    gt = {"cam_view_num": np.asarray(c["views"]), "image": torch.zeros(1, device=device).expand(BN, 3, c["H"], c["W"]),
          "master_joints_3d": t["gt_joints"], "master_verts_3d": t["gt_verts"], "target_joints_2d": t["gt_uv"], "target_cam_intr": t["K"],
          "target_cam_extr": t["E"]}
    if c["parametric"]:
        preds.update(pred_pose=t["pred_pose"], pred_shape=t["pred_shape"])
        gt.update(mano_pose=t["mano_pose"], mano_shape=t["mano_shape"])
    return preds, gt


def test_poem_loss_refuses_cpu_tensors_and_a_missing_regressor():
    cases, jreg = fixture()
    c = cases["release"]
    preds, gt = _dicts(c)
    with pytest.raises(RuntimeError, match="licence-gated"):
        _poem_loss(c)(preds, gt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _poem_loss(c, jreg)(preds, gt)
    with pytest.raises(ValueError, match="16,778"):
        _poem_loss(c, jreg[:, :700])


def test_poem_loss_image_size_sources():
    import poem_v2_amd as pk
    size = pk.PoemLoss._image_size
    assert size({"image": torch.zeros(2, 3, 24, 32)}) == (24, 32)
    assert size({"inp_img_shape": (240, 320)}) == (240, 320)
    assert size({"image": torch.zeros(2, 3, 24, 32), "inp_img_shape": (1, 1)}) == (24, 32)
    with pytest.raises(KeyError, match="inp_img_shape"):
        size({})


def test_model_without_loss_node_has_no_loss():
    """The attributes exist on the class; building a model needs a GPU, so the wiring is checked on the source's own terms here and
    end to end in tests/test_loss.py."""
    import poem_v2_amd as pk
    m = object.__new__(pk.PtEmbedMultiviewStereoV2)
    m.loss = None
    with pytest.raises(RuntimeError, match="LOSS"):
        m.compute_loss({}, {})
    with pytest.raises(RuntimeError, match="LOSS"):
        m.set_j_regressor(np.zeros((16, 778), np.float32))


# ---- LossMetric -------------------------------------------------------------------------------------------------------------------
class _AverageMeter:
    """upstream's AverageMeter.update_by_mean (lib/metrics/basic_metric.py:51-54)"""

    def __init__(self):
        self.sum, self.count, self.avg = 0, 0, 0

    def update_by_mean(self, val, n=1):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _recorded_dicts():
    cases, _ = fixture()
    feeds = [("release", 3), ("allterms", 4), ("clamp", 2)]
    return [({k: torch.tensor(float(v), dtype=torch.float64) for k, v in zip(cases[n]["keys"], cases[n]["ref64"])}, bs) for n, bs in feeds]


def test_loss_metric_equals_upstreams_update_by_mean():
    import poem_v2_amd as pk
    lm = pk.LossMetric(None)
    assert lm.count == 0 and lm.is_empty() and lm.get_measures() == {}
    meters = {}
    for d, bs in _recorded_dicts():
        lm.feed(dict(d, skipped=None, also_skipped=1.5), bs)         # upstream passes over None and non-tensors
        for k, v in d.items():
            meters.setdefault(k, _AverageMeter()).update_by_mean(v.item(), bs)
    assert lm.count == 9 and lm.num_sample() == 9
    got = lm.get_measures()
    assert list(got) == list(meters)                                # keys in the order they first appeared
    for k, m in meters.items():
        assert abs(got[k] - m.avg) <= 1e-15 * abs(m.avg), (k, got[k], m.avg)
        assert lm.get_loss(k) == got[k]
    assert meters["loss_pose"].count == 4 and meters["loss"].count == 9      # a key fed once averages over its own feeds
    assert lm.acc.dtype == torch.float64 and lm.acc.numel() == 2 * len(meters) + 1
    lm.reset()
    assert lm.count == 0 and lm.get_measures() == {}


_WORKER = r'''
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import poem_v2_amd as pk
from poem_v2_amd import dist as pdist
from test_loss_host import _recorded_dicts
rank, local, world = pdist.init_from_env(backend="gloo")
assert world == 2
feeds = _recorded_dicts() * 2                     # six feeds; every rank feeds every key (allterms goes to both)
single = pk.LossMetric(None)
for d, bs in feeds:
    single.feed(d, bs)
mine = pk.LossMetric(None)
for d, bs in (feeds[:3] if rank == 0 else feeds[3:]):
    mine.feed(d, bs)
local_before = mine.acc.clone()
want = single.get_measures()
for _ in range(2):                                # a second reduce() changes nothing
    mine.reduce()
    got = mine.get_measures()
    assert list(got) == list(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-15 * abs(want[k]), (k, got[k], want[k])
    assert torch.equal(mine.acc, local_before) and mine.count == 9      # local sums untouched
    assert mine._global[-1].item() == 18
mine.feed(feeds[0][0], feeds[0][1])               # a feed after reduce() reads the local sums again
assert mine._global is None and mine.count == 12
pdist.barrier()
if rank == 0: print("LOSS_DP_OK")
torch.distributed.destroy_process_group()
'''


def test_loss_metric_reduce_gloo_world2(tmp_path):
    from poem_v2_amd.dist import free_port
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    port = str(free_port())
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", port, str(script), ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "LOSS_DP_OK" in out.stdout


# ---- eval_single.py ---------------------------------------------------------------------------------------------------------------
def _eval_single():
    spec = importlib.util.spec_from_file_location("eval_single", os.path.join(ROOT, "scripts", "eval_single.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_single_losses_flag_needs_shards_and_a_regressor(tmp_path):
    es = _eval_single()
    base = ["--cfg", str(tmp_path / "none.yaml"), "--dataset", "HO3D", "--view_min", "2", "--view_max", "3", "--model", "small", "-g", "0"]
    a = es.build_parser().parse_args(base)
    assert a.losses is False and a.j_regressor is None                       # defaults: the run is what it was
    es.check_losses_args(a)
    with pytest.raises(SystemExit, match="--shards"):
        es.check_losses_args(es.build_parser().parse_args(base + ["--losses", "--j-regressor", "j.npy"]))
    with pytest.raises(SystemExit, match="licence-gated"):
        es.check_losses_args(es.build_parser().parse_args(base + ["--losses", "--shards", str(tmp_path)]))
    es.check_losses_args(es.build_parser().parse_args(base + ["--losses", "--shards", str(tmp_path), "--j-regressor", "j.npy"]))


def test_eval_single_parser_defaults_are_unchanged():
    es = _eval_single()
    a = vars(es.build_parser().parse_args(["--cfg", "c.yaml", "--dataset", "HO3D", "--view_min", "2", "--view_max", "3", "--model", "small",
                                           "-g", "0"]))
    new = {"losses": False, "j_regressor": None}
    old = {"cfg": "c.yaml", "dataset": "HO3D", "view_min": 2, "view_max": 3, "model": "small", "gpu_id": 0, "reload": None, "port": 60000,
           "draw": False, "epoch_size": 64, "pyramid": False, "shards": None, "template": None, "dlt_confidence": "off",
           "dlt_threshold": 0.5, "batch_size": 2, "faces": None, "draw_dir": "./draw"}
    assert a == {**old, **new}


def test_eval_single_loss_node_comes_from_the_config_or_the_release_values():
    import poem_v2_amd as pk
    es = _eval_single()
    assert es.loss_node({"MODEL": {"HEAD": {}}}) == dict(pk.configs.loss_cfg())
    own = {"JOINTS_LOSS_WEIGHT": 2.0, "VERTICES_LOSS_WEIGHT": 1.0, "JOINTS_2D_LOSS_WEIGHT": 0.0, "HEATMAP_JOINTS_WEIGHT": 1.0}
    assert es.loss_node({"MODEL": {"HEAD": {}, "LOSS": own}}) == own
