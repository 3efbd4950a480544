"""csrc/mano_fit.hip's joint and keypoint terms through ``poem_mano_fit_terms`` (ctypes, every buffer between canary guards) and
``poem_v2_amd.fit_mano``, against the fp64 restatement of tests/mano_fit_terms_util.py (explicit rows view by view, central
differences of oracle/mano_oracle.py, LAPACK, a Python LM loop -- nothing shared with the kernels).  Synthetic assets, batches of at
most 4, at most 5 views per sample, at most 8 iterations.

Every tolerance is measured where it is used (``tu.eval_bars``): two summation orders x two Jacobian step sizes, four times the
spread plus the bound of a recursive fp64 sum of the rows.  Measured values on the MI355X: MEASURED below."""
import ctypes

import numpy as np
import pytest
import torch

import mano_fit_terms_util as tu
import mano_fit_util as u
import mano_oracle as mo

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
ST, ST_XC, ST_G, ST_C, ST_MU, ST_H = 3928, 64, 128, 192, 193, 200        # include/poem_hip.h: the workspace's diagnostic head
_GUARD, _CANARY = 64, 0x5A5A5A5A
E_ARG, E_WS, E_UNSUPPORTED = -1, -2, -4

# MEASURED (MI355X, relative unless a unit is given), written from this file's own output (LABNOTES "MANO fit" has all of it):
#   evaluation, four poses with 1 / 3 / 5 / 2 views: K only cost 0 .. 4.0e-16 (bars 4.7e-15 .. 2.1e-14), g 1.7e-13 (bars 1.1e-12 ..
#     2.6e-12), H 2.2e-13 (bars 1.25e-12 .. 1.7e-12); J only cost 1.5e-16 (bars 5.7e-15 ..), g 1.7e-13, H 3.3e-13 (bars 1.4e-12 ..);
#     M + J + K cost 4.3e-16 (bars 2.7e-13 ..), g 1.6e-13 (bars 1.5e-12 ..), H 2.9e-13 (bars 1.6e-12 ..); the same with regularisers
#   steps: sequences equal; |x - x_ref| 1.6e-9 .. 2.3e-9 ("far"), candidates 5.3e-9 .. 1.6e-8 ("overshoot"), 2.2e-9 ("crossing");
#     "far_reg" 1.2e-12 .. 2.3e-12 (bar 6.5e-8)
#   keypoints only: joints 8.4e-9 m from the restatement's (bar 6.8e-8 m), cost 5.4e-10 (bar 5.4e-9), 9.2e-6 mm from the true joints
#   combined: joints 1.1e-8 m from the restatement's (bar 6.8e-8 m), 0.0112 mm from the clean joints (mesh only: 0.2535 mm)


@pytest.fixture(scope="module")
def layer():
    import poem_v2_amd as pk
    return pk.ManoLayer(pk.mano.synthetic_mano_assets(3), center_idx=None, device=DEV)


class _Guarded:
    """n bytes of device memory between two canary zones"""
    def __init__(self, nbytes):
        self.n = (nbytes + 3) // 4
        self.buf = torch.full((self.n + 2 * _GUARD,), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf[_GUARD:].data_ptr()

    def guards_ok(self):
        return bool((self.buf[:_GUARD] == _CANARY).all()) and bool((self.buf[_GUARD + self.n:] == _CANARY).all())

    def untouched(self):
        return bool((self.buf == _CANARY).all())

    def read(self, dtype, shape):
        return self.buf[_GUARD:_GUARD + self.n].view(dtype)[:int(np.prod(shape))].reshape(shape).cpu()


_OUTS = (("pose_aa", torch.float32, 48), ("betas", torch.float32, 10), ("tsl", torch.float32, 3), ("verts", torch.float32, 2334),
         ("joints", torch.float32, 63), ("cost", torch.float64, 1), ("accepted", torch.int32, 1), ("status", torch.int32, 1))
_FIELDS = ("target_verts", "joints3d", "joints3d_weight", "keypoints", "keypoint_weight", "cam_intr", "cam_extr", "view_offsets")


def _batch(samples):
    """a list of one-sample terms (``tu.make_terms``, all with the same terms present) -> the call's arrays"""
    s0 = samples[0]
    d = dict(views=[0 if s["kp"] is None else int(s["kp"].shape[0]) for s in samples], mesh_weight=s0["mesh_weight"], scale=s0["scale"])
    d["target_verts"] = None if s0["target"] is None else torch.stack([s["target"] for s in samples])
    d["joints3d"] = None if s0["j3"] is None else torch.stack([s["j3"] for s in samples])
    d["joints3d_weight"] = None if s0["j3"] is None else torch.stack([s["w3"] for s in samples])
    for key, src in (("keypoints", "kp"), ("keypoint_weight", "w2"), ("cam_intr", "K"), ("cam_extr", "T")):
        d[key] = None if s0["kp"] is None else torch.cat([s[src] for s in samples])
    return d


def _raw(layer, samples, x0=None, iters=8, shape_reg=0.0, pose_reg=0.0, batch=None, ws_bytes=None, null=(), total_views=None,
         mesh_weight=None, scale=None, old=False):
    """``poem_mano_fit_terms`` (``old``: ``poem_mano_fit`` on the samples' meshes) with guarded buffers -> (rc, outputs dict or None
    when nothing was written, state (B,3928) fp64)"""
    import poem_v2_amd as pk
    L = pk.hip.lib()
    d = _batch(samples)
    B = len(samples)
    nb = B if batch is None else batch
    need = L.poem_mano_fit_workspace_bytes(B) if old else L.poem_mano_fit_terms_workspace_bytes(B)
    assert need == 8 * B * (ST + (49 if old else 50) * 1953)
    dev = {k: None if d[k] is None else d[k].to(DEV).contiguous() for k in _FIELDS[:-1]}
    offs = torch.tensor(np.concatenate([[0], np.cumsum(d["views"])]), dtype=torch.int32, device=DEV)
    x0d = None if x0 is None else x0.to(DEV).contiguous()
    ws = _Guarded(need)
    out = {k: _Guarded(B * n * torch.empty(0, dtype=dt).element_size()) for k, dt, n in _OUTS}
    p = {k: (None if k in null else g.ptr) for k, g in out.items()}
    t = pk.hip.PoemManoFitTerms()
    for k in _FIELDS[:-1]:
        setattr(t, k, None if dev[k] is None or k in null else (dev[k].data_ptr() or layer.th_table.data_ptr()))
    if d["keypoints"] is not None:
        t.view_offsets = None if "view_offsets" in null else offs.data_ptr()
        t.total_views = sum(d["views"]) if total_views is None else total_views
        t.image_scale = d["scale"] if scale is None else scale
    t.mesh_weight = d["mesh_weight"] if mesh_weight is None else mesh_weight
    tail = (None if "workspace" in null else ws.ptr, need if ws_bytes is None else ws_bytes, p["pose_aa"], p["betas"], p["tsl"], p["verts"],
            p["joints"], p["cost"], p["accepted"], p["status"], pk.hip.stream())
    table = None if "table" in null else layer.th_table.data_ptr()
    x0p = None if x0d is None else x0d.data_ptr()
    if old:
        rc = L.poem_mano_fit(table, dev["target_verts"].data_ptr(), x0p, nb, iters, shape_reg, pose_reg, *tail)
    else:
        rc = L.poem_mano_fit_terms(table, None if "terms" in null else ctypes.byref(t), x0p, nb, iters, shape_reg, pose_reg, *tail)
    torch.cuda.synchronize()
    assert ws.guards_ok() and all(g.guards_ok() for g in out.values()), "a guard element was written"
    if all(g.untouched() for g in out.values()):
        assert ws.untouched()
        return rc, None, None
    res = {k: out[k].read(dt, (B, n)) for k, dt, n in _OUTS}
    return rc, res, ws.read(torch.float64, (need // 8,))[:B * ST].reshape(B, ST)


def _x_of(res, i=slice(None)):
    return torch.cat([res["pose_aa"][i], res["betas"][i], res["tsl"][i]], -1)


def _same_bits(a, b, ia, ib, what=""):
    for k in a:
        assert a[k][ia].numpy().tobytes() == b[k][ib].numpy().tobytes(), (what, k)


# ---- the old entry point ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_x0", [False, True])
def test_mesh_only_with_weight_one_is_poem_mano_fit(layer, with_x0):
    """term M alone, mesh_weight 1: the bits of ``poem_mano_fit`` on all eight outputs and on the workspace head -- a clean, a
    flagged (NaN in the target) and another clean sample"""
    tg = u.recovery_case(noise_mm=2.0)["target"].clone()
    tg[1, 300, 1] = float("nan")
    samples = [tu.make_terms(target=tg[i]) for i in range(3)]
    x0 = u.seeded_params(31, 3) if with_x0 else None
    rc0, old, st0 = _raw(layer, samples, x0, iters=4, old=True)
    rc1, new, st1 = _raw(layer, samples, x0, iters=4)
    assert rc0 == rc1 == 0 and old["status"][:, 0].tolist() == [0, 1, 0]
    _same_bits(old, new, slice(None), slice(None))
    assert st0.numpy().tobytes() == st1.numpy().tobytes()
    assert min(int(new["accepted"][0]), int(new["accepted"][2])) >= 2          # (the runs did iterate)


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["K", "J", "MJK", "MJK_reg"])
def test_evaluation_matches_the_restatement(layer, kind):
    """iters = 0 from a given x0, the four ``eval_poses`` in one batch with 1, 3, 5 and 2 views: cost (the fp64 output), g and H
    (the workspace's diagnostic head) per sample under the measured bars.  "MJK_reg": the first sample with both regularisers."""
    reg = tu.REG if kind.endswith("_reg") else {}
    scene = tu.eval_scene(kind.replace("_reg", ""))
    scene = scene[:1] if reg else scene
    x0 = torch.stack([s[1] for s in scene])
    rc, res, st = _raw(layer, [s[2] for s in scene], x0, iters=0, **reg)
    assert rc == 0 and res["status"][:, 0].tolist() == [0] * len(scene) and res["accepted"][:, 0].tolist() == [0] * len(scene)
    assert torch.equal(_x_of(res), x0)                                        # iters = 0 returns the start
    fails = []
    for i, (name, xi, tm) in enumerate(scene):
        (c, g, H), bars = tu.eval_bars(xi, tm, **reg)
        eg = float((st[i, ST_G:ST_G + 61] - g).abs().max() / g.abs().max())
        eH = float((st[i, ST_H:ST_H + 3721].reshape(61, 61) - H).abs().max() / H.abs().max())
        ec = abs(float(res["cost"][i]) - float(c)) / float(c)
        print(f"{kind} {name}: cost {ec:.2e} (bar {bars['c']:.2e})  g {eg:.2e} (bar {bars['g']:.2e})  H {eH:.2e} (bar {bars['H']:.2e})")
        assert float(st[i, ST_C]) == float(res["cost"][i]) and float(st[i, ST_MU]) == 1e-3
        if not (ec <= bars["c"] and eg <= bars["g"] and eH <= bars["H"]):
            fails.append((name, ec, eg, eH, bars))
    assert not fails, fails


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def test_weight_zero_entries_are_not_read(layer):
    """NaN and inf under weight 0 (keypoints and joint targets) give the bits of the same call with finite values there"""
    scene = tu.eval_scene("MJK")
    x0 = torch.stack([s[1] for s in scene])
    clean = [s[2] for s in scene]
    dirty = []
    for tm in clean:
        kp, j3 = tm["kp"].clone(), tm["j3"].clone()
        off2, off3 = tm["w2"] == 0, tm["w3"] == 0
        kp[off2] = torch.tensor([float("nan"), float("inf")])
        j3[off3] = torch.tensor([float("-inf"), float("nan"), 1.0])
        dirty.append(dict(tm, kp=kp, j3=j3))
    assert sum(int((tm["w2"] == 0).sum()) for tm in clean) >= 8 and sum(int((tm["w3"] == 0).sum()) for tm in clean) >= 4
    rc0, a, sa = _raw(layer, clean, x0, iters=2)
    rc1, b, sb = _raw(layer, dirty, x0, iters=2)
    assert rc0 == rc1 == 0 and b["status"][:, 0].tolist() == [0, 0, 0, 0]
    _same_bits(a, b, slice(None), slice(None))
    assert sa.numpy().tobytes() == sb.numpy().tobytes()


def test_a_view_of_weight_zero_is_as_if_absent(layer):
    """a view whose 21 weights are all 0 -- keypoints and camera NaN -- in the middle of a sample's views: every bit of the call
    without that view"""
    scene = tu.eval_scene("K")
    x0 = torch.stack([s[1] for s in scene])
    clean = [s[2] for s in scene]
    tm = clean[1]                                                             # three views -> four, the new one second
    ins = lambda t, v: torch.cat([t[:1], v[None], t[1:]])                     # noqa: E731
    nan = float("nan")
    more = dict(tm, kp=ins(tm["kp"], torch.full((21, 2), nan)), w2=ins(tm["w2"], torch.zeros(21)),
                K=ins(tm["K"], torch.full((3, 3), nan)), T=ins(tm["T"], torch.full((4, 4), nan)))
    rc0, a, sa = _raw(layer, clean, x0, iters=2)
    rc1, b, sb = _raw(layer, [clean[0], more, clean[2], clean[3]], x0, iters=2)
    assert rc0 == rc1 == 0 and b["status"][:, 0].tolist() == [0, 0, 0, 0]
    _same_bits(a, b, slice(None), slice(None))
    assert sa.numpy().tobytes() == sb.numpy().tobytes()


def test_invalid_weights_and_values_flag_their_sample_only(layer):
    """a NaN keypoint under a positive weight, a negative and a NaN weight, a non-finite camera of a used view, a NaN joint target:
    status bit 0, the start comes back, and the neighbours keep their bits"""
    scene = tu.eval_scene("MJK")
    x0 = torch.stack([s[1] for s in scene])
    clean = [s[2] for s in scene]
    rc, ref, _ = _raw(layer, clean, x0, iters=2)
    assert rc == 0

    def put(key, index, value):
        t = clean[2][key].clone()
        assert key not in ("kp",) or float(clean[2]["w2"][index[:2]]) > 0
        t[index] = value
        return dict(clean[2], **{key: t})
    pos = tuple(int(v) for v in (clean[2]["w2"] > 0).nonzero()[0])
    pos3 = int((clean[2]["w3"] > 0).nonzero()[0])
    for bad in (put("kp", pos + (1,), float("nan")), put("w2", pos, -1.0), put("w2", pos, float("nan")), put("w3", pos3, -0.5),
                put("T", (pos[0], 1, 2), float("inf")), put("K", (pos[0], 0, 0), float("nan")), put("j3", (pos3, 0), float("nan"))):
        rc, res, _ = _raw(layer, [clean[0], clean[1], bad, clean[3]], x0, iters=2)
        assert rc == 0 and res["status"][:, 0].tolist() == [0, 0, 1, 0]
        assert torch.equal(_x_of(res, 2), x0[2]) and int(res["accepted"][2]) == 0 and bool(torch.isnan(res["cost"][2]))
        for i in (0, 1, 3):
            _same_bits(ref, res, i, i)


# ---- steps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far", "overshoot", "far_reg", "crossing"])
def test_one_and_two_steps(layer, name):
    """The restatement's accept / reject sequence (``tu.LM_EXPECT``, host-checked: "overshoot" is rejected twice, "crossing" once,
    by the depth rule: its first candidate puts a joint 0.84 mm in front of camera 0), the accepted point and the last candidate
    within the sum over the steps so far of cond2(H + mu D) (barH + barg) |dx| in 2-norms, as tests/test_mano_fit.py.  With keypoints
    alone twist and betas are free and that bar is of order 1e-2 .. 1: it says nothing.  So the two are ALSO held to the restatement's
    own error, measured as the keypoints-only test measures it: four times the distance between its runs with the Jacobians at
    H_STEP and H_STEP / 2, plus 2^-52 |x| (a rejected step leaves x = x0 exactly, in both)."""
    reg = tu.REG if name.endswith("_reg") else {}
    key = name.replace("_reg", "")
    x0, tm = tu.depth_cases()[key] if key == "crossing" else tu.lm_cases()[key]
    a = u.assets()
    ref = tu.lm(a, tm, x0, iters=2, **reg)
    ref2 = tu.lm(a, tm, x0, iters=2, h=tu.H_STEP / 2, **reg)
    assert ref["accepted"] == ref2["accepted"] == tu.LM_EXPECT[key]
    bar, x = 0.0, x0.double()
    for k in (1, 2):
        (c, g, H), bars = tu.eval_bars(x, tm, **reg)
        bar += u.condition_number(H, ref["mu"][k - 1]) * (bars["H2"] + bars["g2"]) * float(ref["dx"][k - 1].norm())
        rc, res, st = _raw(layer, [tm], x0[None], iters=k, **reg)
        assert rc == 0 and int(res["status"][0]) == 0
        assert int(res["accepted"][0]) == sum(ref["accepted"][:k]), (k, res["accepted"], ref["accepted"])
        ex = float((st[0, :61] - ref["xs"][k]).norm())
        ec = float((st[0, ST_XC:ST_XC + 61] - (x + ref["dx"][k - 1])).norm())
        rel_c = abs(float(res["cost"][0]) - ref["costs"][k]) / ref["costs"][k]
        print(f"{name} step {k}: |x - x_ref| {ex:.2e}  |cand - cand_ref| {ec:.2e} (bar {bar:.2e})  cost rel {rel_c:.2e}")
        assert ex <= bar and ec <= bar
        eps_x = 2.0 ** -52 * float(ref["xs"][k].norm())
        bar_x = 4 * float((ref["xs"][k] - ref2["xs"][k]).norm()) + eps_x
        bar_c = 4 * float(((x + ref["dx"][k - 1]) - (ref2["xs"][k - 1] + ref2["dx"][k - 1])).norm()) + eps_x
        print(f"{name} step {k}: spread bars: x {bar_x:.2e}, candidate {bar_c:.2e}")
        assert ex <= bar_x and ec <= bar_c
        x = ref["xs"][k]


# ---- fits ---------------------------------------------------------------------------------------------------------------------------
def _fit_kw(tm, views):
    kw = dict(keypoints=tm["kp"].to(DEV), keypoint_weights=tm["w2"].to(DEV), cam_intr=tm["K"].to(DEV), cam_extr=tm["T"].to(DEV),
              cam_view_num=views, image_scale=tm["scale"])
    return kw


def _layer_joint_bar(x):
    """tests/test_mano_fit.py ``test_fit_agrees_with_the_layer``'s bar for the joints at parameters x (B,61) fp32"""
    import poem_v2_amd as pk
    raw = pk.mano.synthetic_mano_assets(3)
    r64 = mo.mano_lbs(raw, x[:, :48], x[:, 48:58], center_idx=None)[1] + x[:, None, 58:].double()
    r32 = mo.mano_lbs(raw, x[:, :48], x[:, 48:58], center_idx=None, dtype=torch.float32)[1] + x[:, None, 58:]
    return r64, 4 * (r32.double() - r64).abs().flatten(1).amax(1) + 2.0 ** -23 * r64.abs().flatten(1).amax(1)


def test_keypoints_only(layer):
    """4 clean views, x0 = the mesh default start, no mesh term: joints and cost against the restatement's own fit.  Bars: joints
    4 (the restatement's spread between its two Jacobians + 2^-24 max|coordinate|, the rounding of the fp32 joints returned);
    cost 4 (the same spread of the cost, relative) + 1e-9.  The fit's joints are the layer's at the returned parameters.
    Vertices and betas are NOT compared: keypoints do not determine bone twist or, on these assets, the betas."""
    import poem_v2_amd as pk
    sc, x0, tm, r, r2 = tu.kponly_reference()
    fit = pk.fit_mano(layer, None, iters=8, init=x0[None].to(DEV), **_fit_kw(tm, [4]))
    assert fit.status.tolist() == [0] and int(fit.accepted[0]) >= 5
    j = fit.joints[0].cpu().double()
    bar = 4 * (float((r["joints"] - r2["joints"]).abs().max()) + 2.0 ** -24 * float(r["joints"].abs().max()))
    err = float((j - r["joints"]).abs().max())
    bar_c = 4 * abs(r["cost"] - r2["cost"]) / r["cost"] + 1e-9
    err_c = abs(float(fit.cost[0]) - r["cost"]) / r["cost"]
    true = float((j - sc["clean_joints"]).norm(dim=-1).mean())
    print(f"keypoints only: |joints - restated| {err:.3e} m (bar {bar:.3e})  cost rel {err_c:.2e} (bar {bar_c:.2e})  "
          f"{true * 1e3:.2e} mm from the true joints, accepted {int(fit.accepted[0])}")
    assert err <= bar and err_c <= bar_c
    x = torch.cat([fit.pose_aa, fit.betas, fit.tsl], -1).cpu()
    r64, lbar = _layer_joint_bar(x)
    m = layer(fit.pose_aa, fit.betas)
    assert float(((m.joints + fit.tsl[:, None]).cpu().double() - fit.joints.cpu().double()).abs().max()) <= float(lbar[0]) < 2e-6
    assert float((fit.joints.cpu().double() - r64).abs().max()) <= float(lbar[0])


def test_mesh_and_keypoints_combined(layer):
    """Mesh with 2 mm noise plus clean keypoints in 4 views, mesh_weight 1, weight_2d chosen on the CPU (``tu.COMBINED``; the host
    file checks that the restatement's joints then beat its mesh-only fit's).  The device's joints against the restatement's: bar
    4 (its spread between the two Jacobians + how far its joints still moved over its last two iterations + 2^-24 max|coordinate|)."""
    import poem_v2_amd as pk
    sc, tm, r, r2, mesh_only = tu.combined_reference()
    fit = pk.fit_mano(layer, sc["target"][None].to(DEV), iters=8, **_fit_kw(tm, [tu.COMBINED["views"]]))
    assert fit.status.tolist() == [0]
    moved = float((u.model(u.assets(), r["xs"][6][None])[1][0] - r["joints"]).abs().max())
    bar = 4 * (float((r["joints"] - r2["joints"]).abs().max()) + moved + 2.0 ** -24 * float(r["joints"].abs().max()))
    j = fit.joints[0].cpu().double()
    err = float((j - r["joints"]).abs().max())
    e_fit, e_mesh = float((j - sc["clean_joints"]).norm(dim=-1).mean()), float((mesh_only["joints"] - sc["clean_joints"]).norm(dim=-1).mean())
    err_c = abs(float(fit.cost[0]) - r["cost"]) / r["cost"]
    print(f"combined: |joints - restated| {err:.3e} m (bar {bar:.3e})  cost rel {err_c:.2e}  {e_fit * 1e3:.4f} mm from the clean joints "
          f"(mesh only, restated: {e_mesh * 1e3:.4f} mm)")
    assert err <= bar and e_fit < e_mesh
    assert err_c <= 4 * abs(r["costs"][6] - r["costs"][8]) / r["cost"] + 1e-9


def test_joint_targets_alone_start_from_the_rigid_rule(layer):
    """term J alone, no x0: the start is the rigid rule on the 21 zero-pose joints (against the restatement's Kabsch start, bar
    1e-9 + fp32 rounding of what is returned at iters = 0); a weight-0 joint there sets status bit 1"""
    import poem_v2_amd as pk
    sc = tu.fit_scene()
    j3 = sc["clean_joints"].float()
    fit = pk.fit_mano(layer, None, joints=j3[None].to(DEV), iters=0)
    ref = tu.joints_start(u.assets(), j3)
    x = torch.cat([fit.pose_aa, fit.betas, fit.tsl], -1)[0].cpu().double()
    print("joint start |x - ref|", float((x - ref).abs().max()))
    assert fit.status.tolist() == [0] and float((x - ref).abs().max()) <= 1e-9 + 2.0 ** -23 * float(ref.abs().max())
    fit = pk.fit_mano(layer, None, joints=j3[None].to(DEV), iters=8)
    assert fit.status.tolist() == [0] and float((fit.joints[0].cpu().double() - j3.double()).abs().max()) < 1e-6
    w = torch.ones(1, 21)
    w[0, 5] = 0
    fit = pk.fit_mano(layer, None, joints=j3[None].to(DEV), joint_weights=w.to(DEV), iters=2)
    assert fit.status.tolist() == [2] and int(fit.accepted[0]) == 0


# ---- depth --------------------------------------------------------------------------------------------------------------------------
def test_a_start_behind_a_camera_is_flagged(layer):
    """status 4, the start comes back (cost NaN, no accepted step), and the other samples keep their bits"""
    xb, tm = tu.depth_cases()["behind"]
    xc, _ = tu.lm_cases()["far"]
    tm3 = tu.lm_cases()["far"][1]
    rc, ref, _ = _raw(layer, [tm3, tm, tm3], torch.stack([xc, xc, xc]), iters=3)
    rc2, res, _ = _raw(layer, [tm3, tm, tm3], torch.stack([xc, xb, xc]), iters=3)
    assert rc == rc2 == 0 and ref["status"][:, 0].tolist() == [0, 0, 0] and res["status"][:, 0].tolist() == [0, 4, 0]
    assert torch.equal(_x_of(res, 1), xb) and int(res["accepted"][1]) == 0 and bool(torch.isnan(res["cost"][1]))
    for i in (0, 2):
        _same_bits(ref, res, i, i)


# ---- bits ---------------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_position_neighbours_or_call(layer):
    scene = tu.eval_scene("MJK")
    x0 = torch.stack([s[1] for s in scene])
    tms = [s[2] for s in scene]
    _, alone, sa = _raw(layer, [tms[1]], x0[1:2], iters=4)
    _, first, sf = _raw(layer, [tms[1], tms[2], tms[0]], x0[[1, 2, 0]], iters=4)
    _, last, sl = _raw(layer, [tms[3], tms[0], tms[2], tms[1]], x0[[3, 0, 2, 1]], iters=4)
    _, again, sg = _raw(layer, [tms[3], tms[0], tms[2], tms[1]], x0[[3, 0, 2, 1]], iters=4)
    _same_bits(alone, first, 0, 0)
    _same_bits(alone, last, 0, 3)
    _same_bits(last, again, slice(None), slice(None))
    assert sa[0].numpy().tobytes() == sf[0].numpy().tobytes() == sl[3].numpy().tobytes() and sl.numpy().tobytes() == sg.numpy().tobytes()
    assert int(alone["accepted"][0]) >= 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(layer):
    scene = tu.eval_scene("MJK")[:2]
    x0 = torch.stack([s[1] for s in scene])
    mjk = [s[2] for s in scene]
    konly = [s[2] for s in tu.eval_scene("K")[:2]]
    jonly = [s[2] for s in tu.eval_scene("J")[:2]]
    full = 8 * 2 * (ST + 50 * 1953)
    cases = [(mjk, dict(null=("target_verts", "joints3d", "joints3d_weight", "keypoints", "keypoint_weight")), E_ARG),      # no term
             (mjk, dict(null=("terms",)), E_ARG)]
    cases += [(mjk, dict(null=(k,)), E_ARG) for k in ("keypoint_weight", "cam_intr", "cam_extr", "view_offsets", "joints3d_weight")]
    cases += [(mjk, dict(null=("keypoints",)), E_ARG), (mjk, dict(null=("joints3d",)), E_ARG)]      # a weight array without its values
    cases += [(mjk, dict(total_views=-1), E_ARG), (mjk, dict(total_views=65536), E_UNSUPPORTED)]
    cases += [(mjk, dict(mesh_weight=v), E_ARG) for v in (-1.0, float("nan"), float("inf"))]
    cases += [(mjk, dict(scale=v), E_ARG) for v in (0.0, -256.0, float("nan"), float("inf"))]
    cases += [(mjk, kw, E_ARG) for kw in (dict(iters=-1), dict(iters=65), dict(shape_reg=-1.0), dict(pose_reg=float("nan")), dict(batch=-1))]
    cases += [(mjk, dict(null=(k,)), E_ARG) for k in ("table", "workspace", "pose_aa", "betas", "tsl", "verts", "joints", "cost", "accepted",
                                                       "status")]
    cases += [(mjk, dict(ws_bytes=full - 1), E_WS), (mjk, dict(ws_bytes=0), E_WS)]
    for samples, kw, code in cases:
        rc, res, _ = _raw(layer, samples, x0, **{"iters": 2, **kw})
        assert rc == code and res is None, (kw, rc)
    rc, res, _ = _raw(layer, konly, None, iters=2)                           # keypoints alone, no x0
    assert rc == E_ARG and res is None
    rc, res, _ = _raw(layer, mjk, x0, iters=2, batch=0)                      # batch 0: success, nothing launched
    assert rc == 0 and res is None
    for samples in (konly, jonly, mjk):                                      # ... and each of them runs
        rc, res, _ = _raw(layer, samples, x0, iters=2)
        assert rc == 0 and res["status"][:, 0].tolist() == [0, 0]
    rc, res, _ = _raw(layer, jonly, None, iters=2)                           # (weights of 0 in the joint targets: no rigid start)
    assert rc == 0 and res["status"][:, 0].tolist() == [2, 2]


def test_samples_without_views(layer):
    """a sample with 0 views next to one with views (its term K is empty; the mesh carries it), and a call with no view at all"""
    import poem_v2_amd as pk
    sc = tu.fit_scene(views=2)
    tg = u.recovery_case()["target"][[1, 1]].to(DEV)
    kw = dict(keypoints=sc["kp"].to(DEV), cam_intr=sc["K"].to(DEV), cam_extr=sc["T"].to(DEV), image_scale=256.0)
    both = pk.fit_mano(layer, tg, iters=4, cam_view_num=[2, 0], **kw)
    mesh = pk.fit_mano(layer, tg, iters=4)
    assert both.status.tolist() == [0, 0]
    none = pk.fit_mano(layer, tg, iters=4, keypoints=torch.zeros(0, 21, 2, device=DEV), cam_intr=torch.zeros(0, 3, 3, device=DEV),
                       cam_extr=torch.zeros(0, 4, 4, device=DEV), cam_view_num=[0, 0], image_scale=256.0)
    for k in pk.ManoFit._fields:                                             # no view: the mesh-only fit's bits
        assert getattr(none, k).cpu().numpy().tobytes() == getattr(mesh, k).cpu().numpy().tobytes(), k
        assert getattr(both, k)[1].cpu().numpy().tobytes() == getattr(mesh, k)[1].cpu().numpy().tobytes(), k


# ---- the model and the command line -------------------------------------------------------------------------------------------------
def test_model_key(tmp_path):
    """FIT_MANO_KEYPOINTS with DLT_CONFIDENCE "ransac" (the inlier mask is in the weights): ``pred_mano_joints`` appears,
    ``pred_mano_pose`` changes, the fit is the one made by hand from the forward's own outputs; without the key the forward's keys and
    bits are what they are with FIT_MANO alone."""
    import poem_oracle as po
    import poem_v2_amd as pk
    from poem_v2_amd import backbone as bb
    raw = pk.mano.synthetic_mano_assets(3)
    path = str(tmp_path / "mano.npz")
    np.savez(path, **raw)

    def build(extra):
        cfg = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": pk.configs.head_cfg(128), "DATA_PRESET": {"CENTER_IDX": 9},
               "DLT_CONFIDENCE": "ransac", "FIT_MANO": True, "FIT_MANO_ITERS": 4, "MANO_ASSETS": path, **extra}
        m = pk.build_model(pk.CN(cfg))
        return m.load_parts(bb.seeded_hrnet_state_dict(0), pk.weights.seeded_decoder_state_dict(0), pk.weights.seeded_state_dict(128, seed=0),
                            template=po.synthetic_template(1234))
    with pytest.raises(ValueError, match="FIT_MANO_KEYPOINTS"):
        build({"FIT_MANO_KEYPOINTS": -1.0})
    with pytest.raises(ValueError, match="FIT_MANO_KEYPOINTS"):
        build({"FIT_MANO": False, "FIT_MANO_KEYPOINTS": 1.0})
    views = [3, 3]
    b = pk.inputs.synthetic_batch(views, seed=4)
    img = pk.inputs.synthetic_images(sum(views), seed=4).to(DEV)
    batch = {"image": img, "target_cam_intr": b["img_metas"]["cam_intr"].to(DEV), "target_cam_extr": b["img_metas"]["cam_extr"].to(DEV),
             "master_id": [0] * len(views), "cam_view_num": np.asarray(views)}
    models = {"absent": build({}), "zero": build({"FIT_MANO_KEYPOINTS": 0.0}), "kp": build({"FIT_MANO_KEYPOINTS": 50.0})}
    pyr = models["absent"].extract_img_feat(img)            # one pyramid for all (MIOpen may pick other solvers on a later call)
    preds = {}
    for name, m in models.items():
        m.extract_img_feat = lambda x: pyr
        preds[name] = {k: v.clone() if torch.is_tensor(v) else v for k, v in m(batch, 0, mode="test").items()}
    base, p = preds["absent"], preds["kp"]
    new = {"pred_mano_joints", "pred_mano_keypoint_weight"}
    assert not new & set(base) and set(preds["zero"]) == set(base) and set(p) == set(base) | new
    for k, v in base.items():
        if torch.is_tensor(v):
            assert torch.equal(v, preds["zero"][k]), k
            assert k.startswith("pred_mano_") or torch.equal(v, p[k]), k
    assert not torch.equal(base["pred_mano_pose"], p["pred_mano_pose"])
    w2 = torch.where(p["pred_joints_inlier"], torch.full_like(p["pred_joints_reproj"], 50.0), torch.zeros_like(p["pred_joints_reproj"]))
    assert torch.equal(w2, p["pred_mano_keypoint_weight"]) and tuple(p["pred_mano_joints"].shape) == (2, 21, 3)
    layer = pk.ManoLayer(raw, center_idx=None, device=DEV)
    by_hand = pk.fit_mano(layer, p["pred_verts_3d"].contiguous(), iters=4, keypoints=p["pred_joints_uv"].contiguous(), keypoint_weights=w2,
                          cam_intr=batch["target_cam_intr"], cam_extr=batch["target_cam_extr"], cam_view_num=views,
                          image_scale=float(max(img.shape[-2:])))
    for k, f in (("pred_mano_pose", "pose_aa"), ("pred_mano_joints", "joints"), ("pred_mano_verts", "verts"), ("pred_mano_status", "status")):
        assert torch.equal(p[k], getattr(by_hand, f)), k                      # the same launches on the same inputs


def _eval_single(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    return es


def test_eval_single_reports_the_reprojection(tmp_path, capsys):
    import json
    import poem_v2_amd as pk
    es = _eval_single("eval_single_fit_terms")
    path = str(tmp_path / "mano.npz")
    np.savez(path, **pk.mano.synthetic_mano_assets(3))
    base = ["--cfg", str(tmp_path / "c.yaml"), "--dataset", "DexYCB", "--view_min", "2", "--view_max", "2", "--model", "small", "-g", "0",
            "--epoch_size", "4", "--mano-assets", path, "--fit-mano", "--fit-mano-iters", "4"]
    es.main(es.build_cli().parse_args(base + ["--fit-mano-keypoints", "100"]))
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print({k: res[k] for k in ("mano_fit_residual_mm", "mano_fit_flagged", "mano_fit_reproj_px")})
    assert res["samples"] == 4 and res["mano_fit_reproj_px"] is not None and 0 < res["mano_fit_reproj_px"] < 1e4
    es.main(es.build_cli().parse_args(base))
    assert "mano_fit_reproj_px" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])


def test_eval_single_shards_report_the_reprojection(tmp_path):
    import poem_v2_amd as pk
    es = _eval_single("eval_single_fit_terms_shards")
    path = str(tmp_path / "mano.npz")
    np.savez(path, **pk.mano.synthetic_mano_assets(3))
    cfg = es.default_cfg()
    view_range = es.edit_cfg(cfg, "DexYCB", "small", [2, 3])
    kw = dict(shard_dir=str(tmp_path / "shards"), dataset="DexYCB", epoch_size=4, batch_size=2, n_cams=4, raw_size=(160, 120),
              backbone="resnet18", backbone_engine="hip", mano_assets=path, fit_mano_iters=4)
    res = es.evaluate_shards(cfg, view_range, "small", torch.device(DEV), fit_mano_keypoints=100.0, **kw)
    print({k: res[k] for k in ("mano_fit_residual_mm", "mano_fit_flagged", "mano_fit_reproj_px")})
    assert res["samples"] == 4 and res["mano_fit_reproj_px"] is not None and res["mano_fit_reproj_px"] > 0
    plain = es.evaluate_shards(cfg, view_range, "small", torch.device(DEV), **kw)
    assert "mano_fit_reproj_px" not in plain and "mano_fit_residual_mm" in plain
