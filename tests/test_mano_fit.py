"""csrc/mano_fit.hip through ``poem_mano_fit`` (ctypes, every buffer between canary guards) and ``poem_v2_amd.fit_mano``, against
the fp64 restatement of tests/mano_fit_util.py (central differences of oracle/mano_oracle.py, LAPACK, a Python LM loop -- nothing
shared with the kernels).  Synthetic assets, batches of 1 to 3.

Every tolerance is measured where it is used (``_eval_bars``): the restatement's cost, gradient and normal matrix are formed in two
summation orders and from two Jacobians (extrapolated central differences at step h and h / 2); the bar is four times the sum of
the two spreads plus 2334 * 2^-53, the bound of a recursive fp64 sum of the 2334 rows, relative to max|H|, max|g| and the cost.
Measured values on the MI355X: MEASURED below."""
import numpy as np
import pytest
import torch

import mano_fit_util as u
import mano_oracle as mo

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
ST, ST_XC, ST_G, ST_C, ST_MU, ST_H = 3928, 64, 128, 192, 193, 200        # include/poem_hip.h: the workspace's diagnostic head
_GUARD, _CANARY = 64, 0x5A5A5A5A

# MEASURED (MI355X, relative unless a unit is given), written from this file's own output:
#   evaluation, four poses: cost 0 .. 4.4e-16 (bar 2.6e-13); g 1.6e-13 (bars 1.6e-12 .. 1.8e-12); H 3.3e-13 (bar 1.9e-12);
#     the step |dx - dx_ref| 5.5e-11 .. 6.4e-11 of |dx| = 3.1 .. 3.7 (bars 4.9e-7 .. 8.0e-7 at cond 2.6e4 .. 3.4e4)
#   one and two steps: "far" |x - x_ref| 5.7e-11, 6.1e-11 (bars 6.2e-7, 2.0e-6); "overshoot" 3.9e-9, 3.9e-9 and the rejected
#     candidate 7.0e-9 (bars 8.2e-4, 1.2e-3 at cond 1.8e6); accept / reject sequences equal
#     "far_reg" (shape_reg 0.5, pose_reg 0.25) 1.1e-11, 7.2e-12 (bars 8.6e-8, 1.6e-7); shape_reg 1e6: cost 6.4e-16 (bar 1.0e-9),
#     max|betas| 6.0e-8
#   recovery: |fit - target| 2.98e-8 m on all three samples (bars 1.4e-7 .. 1.7e-7 m), costs 9.900e-14 / 4.839e-14 / 3.825e-14 m^2 =
#     the restatement's to the digits printed, 5 / 5 / 6 accepted steps
#   noise: 0.481 / 0.566 / 0.491 mm from the clean mesh (targets 3.24 / 3.19 / 3.22 mm); |fit - restated| 1.49e-8 m (bars 7.9e-8 ..
#     1.1e-7 m); cost 0 .. 1.9e-16 from the restatement's (bar 1e-9)
#   the layer: verts 3.7e-8 .. 6.0e-8 m (bars 1.7e-7 .. 2.3e-7 m), joints 1.5e-8 .. 3.0e-8 m (bars 7.4e-8 .. 1.2e-7 m)


@pytest.fixture(scope="module")
def layer():
    import poem_v2_amd as pk
    return pk.ManoLayer(pk.mano.synthetic_mano_assets(3), center_idx=None, device=DEV)


class _Guarded:
    """n bytes of device memory between two canary zones"""
    def __init__(self, nbytes, fill=None):
        self.n = (nbytes + 3) // 4
        self.buf = torch.full((self.n + 2 * _GUARD,), _CANARY, dtype=torch.int32, device=DEV)
        if fill is not None:
            self.buf[_GUARD:_GUARD + self.n] = fill.contiguous().view(torch.int32).reshape(-1)

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


def _raw_fit(layer, target, x0=None, iters=8, shape_reg=0.0, pose_reg=0.0, batch=None, ws_bytes=None, null=()):
    """``poem_mano_fit`` with guarded buffers -> (rc, outputs dict or None when nothing was written, state (B,3928) fp64)"""
    import poem_v2_amd as pk
    L = pk.hip.lib()
    B = len(target)
    nb = B if batch is None else batch
    need = L.poem_mano_fit_workspace_bytes(B)
    assert need == 8 * B * (ST + 49 * 1953) and L.poem_mano_fit_workspace_bytes(0) == 0
    tgt = target.to(DEV).contiguous()
    x0d = None if x0 is None else x0.to(DEV).contiguous()
    ws = _Guarded(need)
    out = {k: _Guarded(B * n * torch.empty(0, dtype=dt).element_size()) for k, dt, n in _OUTS}
    p = {k: (None if k in null else g.ptr) for k, g in out.items()}
    rc = L.poem_mano_fit(None if "table" in null else layer.th_table.data_ptr(), None if "target" in null else tgt.data_ptr(),
                         None if x0d is None else x0d.data_ptr(), nb, iters, shape_reg, pose_reg,
                         None if "workspace" in null else ws.ptr, need if ws_bytes is None else ws_bytes, p["pose_aa"], p["betas"],
                         p["tsl"], p["verts"], p["joints"], p["cost"], p["accepted"], p["status"], pk.hip.stream())
    torch.cuda.synchronize()
    assert ws.guards_ok() and all(g.guards_ok() for g in out.values()), "a guard element was written"
    if all(g.untouched() for g in out.values()):
        assert ws.untouched()
        return rc, None, None
    res = {k: out[k].read(dt, (B, n)) for k, dt, n in _OUTS}
    return rc, res, ws.read(torch.float64, (need // 8,))[:B * ST].reshape(B, ST)


def _x_of(res, i=slice(None)):
    return torch.cat([res["pose_aa"][i], res["betas"][i], res["tsl"][i]], -1)


_eval_bars = u.eval_bars


# ---- evaluation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "zero_fingers", "tiny_joint", "angle_3.1"])
def test_evaluation_matches_the_restatement(layer, name):
    """iters = 0 from a given x0: cost (the fp64 output), g and H (the workspace's diagnostic head); one step: dx.  The table's
    composed regression is the restatement's (``composed_regression`` against the device's table)."""
    x0, target = u.eval_poses()[name], u.eval_target()
    (c, g, H), bars = _eval_bars(x0, target)
    rc, res, st = _raw_fit(layer, target[None], x0[None], iters=0)
    assert rc == 0 and int(res["status"][0]) == 0 and int(res["accepted"][0]) == 0
    assert torch.equal(_x_of(res, 0), x0)                                  # iters = 0 returns the start
    eg, eH = float((st[0, ST_G:ST_G + 61] - g).abs().max() / g.abs().max()), float((st[0, ST_H:ST_H + 3721].reshape(61, 61) - H).abs().max() / H.abs().max())
    ec = abs(float(res["cost"][0]) - float(c)) / float(c)
    print(f"{name}: cost {ec:.2e} (bar {bars['c']:.2e})  g {eg:.2e} (bar {bars['g']:.2e})  H {eH:.2e} (bar {bars['H']:.2e})")
    assert float(st[0, ST_C]) == float(res["cost"][0]) and float(st[0, ST_MU]) == 1e-3
    assert ec <= bars["c"] and eg <= bars["g"] and eH <= bars["H"]
    # the step: (H + mu D) dx = -g; first-order bound |ddx| <= cond2(M) (|dM| / |M| + |dg| / |g|) |dx| in 2-norms, the two relative
    # perturbations taken as the measured bars in the 2-norm, the condition number from the restatement's own matrix
    dx = u.solve_step(g, H, 1e-3)
    cond = u.condition_number(H, 1e-3)
    rc, res1, st1 = _raw_fit(layer, target[None], x0[None], iters=1)
    got = st1[0, ST_XC:ST_XC + 61] - x0.double()
    bar_dx = cond * (bars["H2"] + bars["g2"]) * float(dx.norm()) + 2.0 ** -52 * float(x0.double().norm())
    print(f"{name}: |dx - dx_ref| = {float((got - dx).norm()):.2e} (bar {bar_dx:.2e}, cond {cond:.2e}, |dx| {float(dx.norm()):.2e})")
    assert rc == 0 and float((got - dx).norm()) <= bar_dx
    if name == "random":
        import poem_v2_amd as pk
        jt, jsd = u.composed_regression(pk.mano.synthetic_mano_assets(3))
        tail = layer.th_table.cpu()[-(48 + 480):].double()
        assert np.array_equal(tail[:48].numpy(), jt.reshape(-1)) and np.array_equal(tail[48:].numpy(), jsd.reshape(-1))


# ---- one and two LM steps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["far", "overshoot", "far_reg"])
def test_one_and_two_steps(layer, name):
    """The same accept / reject sequence as the restatement ("far": accepted twice; "overshoot": accepted, rejected), the accepted
    point x and the last candidate x + dx within the sum over the steps so far of cond2(H + mu D) (barH + barg) |dx| (2-norms, as
    in the evaluation test; the perturbation of a later step by the earlier one's error is covered by the bars' factor 4).
    "far_reg": the "far" case with both regularisers non-zero (``u.REG``): the regularised cost decides the accept rule and the
    regularised g, H the solve.  The sequences themselves are the host file's business (``u.LM_EXPECT``)."""
    reg = u.REG if name.endswith("_reg") else {}
    x0, target = u.lm_cases()[name.replace("_reg", "")]
    a = u.assets()
    ref = u.lm(a, target, x0=x0, iters=2, **reg)
    assert ref["accepted"] == u.LM_EXPECT[name.replace("_reg", "")]
    bar, x = 0.0, x0.double()
    for k in (1, 2):
        (c, g, H), bars = _eval_bars(x, target, **reg)
        bar += u.condition_number(H, ref["mu"][k - 1]) * (bars["H2"] + bars["g2"]) * float(ref["dx"][k - 1].norm())
        rc, res, st = _raw_fit(layer, target[None], x0[None], iters=k, **reg)
        assert rc == 0 and int(res["status"][0]) == 0
        assert int(res["accepted"][0]) == sum(ref["accepted"][:k]), (k, res["accepted"], ref["accepted"])
        ex = float((st[0, :61] - ref["xs"][k]).norm())
        ec = float((st[0, ST_XC:ST_XC + 61] - (x + ref["dx"][k - 1])).norm())
        rel_c = abs(float(res["cost"][0]) - ref["costs"][k]) / ref["costs"][k]
        print(f"{name} step {k}: |x - x_ref| {ex:.2e}  |cand - cand_ref| {ec:.2e} (bar {bar:.2e})  cost rel {rel_c:.2e}")
        assert ex <= bar and ec <= bar
        assert float((_x_of(res, 0).double() - ref["xs"][k]).abs().max()) <= bar + 2.0 ** -24 * float(ref["xs"][k].abs().max())
        x = ref["xs"][k]


# ---- recovery, noise --------------------------------------------------------------------------------------------------------------
def test_recovery_from_the_default_start(layer):
    """Clean targets (root rotations up to 2.8 rad), default start, iters = 8.  Bar per sample, max over coordinates:
    4 (the restatement's own residual on the case + 2^-24 max|coordinate|, the rounding of the fp32 mesh that is returned)."""
    import poem_v2_amd as pk
    case, ref = u.recovery_case(), u.recovery_reference()
    fit = pk.fit_mano(layer, case["target"].to(DEV), iters=8)
    assert fit.status.tolist() == [0, 0, 0] and min(fit.accepted.tolist()) >= 4
    for i, r in enumerate(ref):
        t = case["target"][i].double()
        bar = 4 * (float((r["verts"] - t).abs().max()) + 2.0 ** -24 * float(t.abs().max()))
        err = float((fit.verts[i].cpu().double() - t).abs().max())
        print(f"sample {i}: |fit - target| {err:.3e} m (bar {bar:.3e})  cost {float(fit.cost[i]):.3e} (restatement {r['cost']:.3e})  accepted {int(fit.accepted[i])}")
        assert err <= bar
        # the parameters are recovered too where the problem pins them (not asserted on the mesh bar: conditioning)
        assert float((fit.betas[i].cpu() - case["x_true"][i, 48:58]).abs().max()) < 1e-3


def test_noisy_targets(layer):
    """2 mm noise per coordinate: the fitted mesh is nearer to the clean mesh than the noisy target is, and agrees with the
    restatement's fitted mesh -- meshes and costs, never parameters.  Bars: mesh 4 (how far the restatement's own mesh still moved
    over its last two iterations + 2^-24 max|coordinate|); cost 4 (the restatement's last two iterations' decrease) + the
    evaluation bar of the cost, relative."""
    import poem_v2_amd as pk
    case, ref = u.recovery_case(noise_mm=2.0), u.recovery_reference(noise_mm=2.0)
    fit = pk.fit_mano(layer, case["target"].to(DEV), iters=8)
    assert fit.status.tolist() == [0, 0, 0]
    for i, r in enumerate(ref):
        v = fit.verts[i].cpu().double()
        fitted, noisy = float((v - case["clean"][i]).norm(dim=-1).mean()), float((case["target"][i].double() - case["clean"][i]).norm(dim=-1).mean())
        moved = float((u.model(u.assets(), r["xs"][6][None])[0][0] - r["verts"]).abs().max())
        bar = 4 * (moved + 2.0 ** -24 * float(r["verts"].abs().max()))
        err = float((v - r["verts"]).abs().max())
        bar_c = 4 * abs(r["costs"][6] - r["costs"][8]) / r["cost"] + 1e-9
        err_c = abs(float(fit.cost[i]) - r["cost"]) / r["cost"]
        print(f"sample {i}: {fitted * 1e3:.3f} mm from clean (target {noisy * 1e3:.3f})  |fit - restated| {err:.3e} m (bar {bar:.3e})  cost rel {err_c:.2e} (bar {bar_c:.2e})")
        assert fitted < noisy and fitted < 0.25 * noisy
        assert err <= bar and err_c <= bar_c


# ---- bits -------------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_batch_or_call(layer):
    import poem_v2_amd as pk
    tg = u.recovery_case(noise_mm=2.0)["target"].to(DEV)
    other = u.recovery_case()["target"].to(DEV)
    alone = pk.fit_mano(layer, tg[1:2], iters=8)
    first = pk.fit_mano(layer, torch.cat([tg[1:2], other[:2]]), iters=8)
    last = pk.fit_mano(layer, torch.cat([other[:2], tg[1:2]]), iters=8)
    again = pk.fit_mano(layer, torch.cat([other[:2], tg[1:2]]), iters=8)
    for k in pk.ManoFit._fields:
        a = getattr(alone, k)[0].cpu().numpy().tobytes()
        assert a == getattr(first, k)[0].cpu().numpy().tobytes() == getattr(last, k)[2].cpu().numpy().tobytes(), k
        assert getattr(last, k).cpu().numpy().tobytes() == getattr(again, k).cpu().numpy().tobytes(), k


# ---- the layer ----------------------------------------------------------------------------------------------------------------------
def test_fit_agrees_with_the_layer(layer):
    """``layer(pose_aa, betas).verts + tsl`` against the fit's mesh, and the joints, under the bar tests/test_mano.py holds the LBS
    kernel to against its oracle (tests/tail_forms_util.py ``lbs_bar``, restated): per sample
    |a - b| <= 4 |fp32 oracle - fp64 oracle| + 2^-23 max|fp64 oracle|, the oracle evaluated at the fitted parameters."""
    import poem_v2_amd as pk
    fit = pk.fit_mano(layer, u.recovery_case(noise_mm=2.0)["target"].to(DEV), iters=8)
    m = layer(fit.pose_aa, fit.betas)
    raw = pk.mano.synthetic_mano_assets(3)
    x = _x_of({k: getattr(fit, k).cpu() for k in ("pose_aa", "betas", "tsl")})
    for name, got, mine, idx in (("verts", m.verts, fit.verts, 0), ("joints", m.joints, fit.joints, 1)):
        r64 = mo.mano_lbs(raw, x[:, :48], x[:, 48:58], center_idx=None)[idx] + x[:, None, 58:].double()
        r32 = mo.mano_lbs(raw, x[:, :48], x[:, 48:58], center_idx=None, dtype=torch.float32)[idx] + x[:, None, 58:]
        bar = 4 * (r32.double() - r64).abs().flatten(1).amax(1) + 2.0 ** -23 * r64.abs().flatten(1).amax(1)
        err = ((got + fit.tsl[:, None]).cpu().double() - mine.cpu().double()).abs().flatten(1).amax(1)
        print(name, "err", err.tolist(), "bar", bar.tolist())
        assert bool((err <= bar).all()) and float(bar.max()) < 2e-6
        assert bool(((mine.cpu().double() - r64).abs().flatten(1).amax(1) <= bar).all())


# ---- regularisers -------------------------------------------------------------------------------------------------------------------
def test_regularisers(layer):
    """Both regularisers non-zero at iters = 0 (c, g, H); the one- and two-step runs with them are ``test_one_and_two_steps[far_reg]``;
    a very large shape_reg returns betas near 0."""
    x0, target = u.eval_poses()["random"], u.eval_target()
    (c, g, H), bars = _eval_bars(x0, target, **u.REG)
    rc, res, st = _raw_fit(layer, target[None], x0[None], iters=0, **u.REG)
    assert rc == 0
    assert abs(float(res["cost"][0]) - float(c)) / float(c) <= bars["c"]
    assert float((st[0, ST_G:ST_G + 61] - g).abs().max() / g.abs().max()) <= bars["g"]
    assert float((st[0, ST_H:ST_H + 3721].reshape(61, 61) - H).abs().max() / H.abs().max()) <= bars["H"]
    (c0, _, _), _ = _eval_bars(x0, target)
    assert float(c) - float(c0) > 1.0                                      # (the terms carry weight in this case)
    import poem_v2_amd as pk
    tg = u.recovery_case()["target"]
    fit = pk.fit_mano(layer, tg.to(DEV), iters=8, shape_reg=1e6)
    ref = u.lm(u.assets(), tg[1], iters=8, shape_reg=1e6)
    assert float(fit.betas.abs().max()) < 1e-3 and fit.status.tolist() == [0, 0, 0]
    # the cost of the full regularised fit, as in the noise test: 4 (the restatement's own decrease over its last two iterations)
    # + 1e-9, relative
    bar_c = 4 * abs(ref["costs"][6] - ref["costs"][8]) / ref["cost"] + 1e-9
    err_c = abs(float(fit.cost[1]) - ref["cost"]) / ref["cost"]
    print(f"shape_reg 1e6: cost rel {err_c:.2e} (bar {bar_c:.2e})  max|betas| {float(fit.betas.abs().max()):.2e}")
    assert err_c <= bar_c


# ---- non-finite input ---------------------------------------------------------------------------------------------------------------
def test_non_finite_and_degenerate_targets(layer):
    import poem_v2_amd as pk
    tg = u.recovery_case()["target"].clone()
    clean = pk.fit_mano(layer, tg.to(DEV), iters=8)
    bad = tg.clone()
    bad[1, 400, 2] = float("nan")
    x0 = u.seeded_params(31, 3)
    for init in (None, x0.to(DEV)):
        ref = clean if init is None else pk.fit_mano(layer, tg.to(DEV), iters=8, init=init)
        fit = pk.fit_mano(layer, bad.to(DEV), iters=8, init=init)
        assert fit.status.tolist() == [0, 1, 0] and int(fit.accepted[1]) == 0 and bool(torch.isnan(fit.cost[1]))
        start = torch.zeros(61) if init is None else x0[1]
        assert torch.equal(_x_of({k: getattr(fit, k).cpu() for k in ("pose_aa", "betas", "tsl")})[1], start)
        for k in pk.ManoFit._fields:
            for i in (0, 2):
                assert getattr(fit, k)[i].cpu().numpy().tobytes() == getattr(ref, k)[i].cpu().numpy().tobytes(), (k, i)
    xbad = x0.clone()
    xbad[2, 50] = float("inf")
    fit = pk.fit_mano(layer, tg.to(DEV), iters=2, init=xbad.to(DEV))
    assert fit.status.tolist() == [0, 0, 2] and torch.equal(fit.betas[2].cpu(), xbad[2, 48:58])
    fit = pk.fit_mano(layer, torch.zeros(1, 778, 3, device=DEV), iters=8)          # a degenerate alignment: finite numbers or a flag
    assert int(fit.status[0]) != 0 or all(bool(torch.isfinite(getattr(fit, k)).all()) for k in ("pose_aa", "betas", "tsl", "verts", "joints", "cost"))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(layer):
    tg, x0 = u.recovery_case()["target"][:2], u.seeded_params(31, 2)
    E_ARG, E_WS = -1, -2
    cases = [(dict(iters=-1), E_ARG), (dict(iters=65), E_ARG), (dict(shape_reg=-1.0), E_ARG), (dict(pose_reg=float("nan")), E_ARG),
             (dict(shape_reg=float("inf")), E_ARG), (dict(batch=-1), E_ARG), (dict(ws_bytes=8 * 2 * (ST + 49 * 1953) - 1), E_WS),
             (dict(ws_bytes=0), E_WS)]
    cases += [(dict(null=(k,)), E_ARG) for k in ("table", "target", "workspace", "pose_aa", "betas", "tsl", "verts", "joints", "cost",
                                                 "accepted", "status")]
    for kw, code in cases:
        rc, res, _ = _raw_fit(layer, tg, x0, **{"iters": 2, **kw})
        assert rc == code and res is None, (kw, rc)
    rc, res, _ = _raw_fit(layer, tg, x0, iters=2, batch=0)                   # batch 0: success, nothing launched
    assert rc == 0 and res is None
    rc, res, _ = _raw_fit(layer, tg, x0, iters=64)                           # the largest count runs
    assert rc == 0 and res["status"][:, 0].tolist() == [0, 0]


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_model_key(tmp_path):
    import poem_oracle as po
    import poem_v2_amd as pk
    from poem_v2_amd import backbone as bb
    raw = pk.mano.synthetic_mano_assets(3)
    path = str(tmp_path / "mano.npz")
    np.savez(path, **raw)

    def build(extra):
        cfg = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": pk.configs.head_cfg(128), "DATA_PRESET": {"CENTER_IDX": 9}, **extra}
        m = pk.build_model(pk.CN(cfg))
        return m.load_parts(bb.seeded_hrnet_state_dict(0), pk.weights.seeded_decoder_state_dict(0), pk.weights.seeded_state_dict(128, seed=0),
                            template=po.synthetic_template(1234))
    with pytest.raises(ValueError, match="MANO"):
        build({"FIT_MANO": True})
    with pytest.raises(ValueError, match="FIT_MANO_ITERS"):
        build({"FIT_MANO": True, "FIT_MANO_ITERS": 65, "MANO_ASSETS": path})
    views = [2, 2]
    b = pk.inputs.synthetic_batch(views, seed=4)
    img = pk.inputs.synthetic_images(sum(views), seed=4).to(DEV)
    batch = {"image": img, "target_cam_intr": b["img_metas"]["cam_intr"].to(DEV), "target_cam_extr": b["img_metas"]["cam_extr"].to(DEV),
             "master_id": [0] * len(views), "cam_view_num": np.asarray(views)}
    models = {"absent": build({}), "false": build({"FIT_MANO": False}), "fit": build({"FIT_MANO": True, "FIT_MANO_ITERS": 6, "MANO_ASSETS": path})}
    pyr = models["absent"].extract_img_feat(img)            # one pyramid for all (MIOpen may pick other solvers on a later call)
    preds = {}
    for name, m in models.items():
        m.extract_img_feat = lambda x: pyr
        preds[name] = {k: v.clone() if torch.is_tensor(v) else v for k, v in m(batch, 0, mode="test").items()}
    base, p = preds["absent"], preds["fit"]
    new = {"pred_mano_pose", "pred_mano_shape", "pred_mano_tsl", "pred_mano_verts", "pred_mano_status"}
    assert not new & set(base) and set(preds["false"]) == set(base) and set(p) == set(base) | new
    for k, v in base.items():
        if torch.is_tensor(v):
            assert torch.equal(v, preds["false"][k]) and torch.equal(v, p[k]), k
    layer = pk.ManoLayer(raw, center_idx=None, device=DEV)
    by_hand = pk.fit_mano(layer, p["pred_verts_3d"].contiguous(), iters=6)
    assert tuple(p["pred_mano_pose"].shape) == (2, 48) and tuple(p["pred_mano_shape"].shape) == (2, 10) and tuple(p["pred_mano_tsl"].shape) == (2, 3)
    assert tuple(p["pred_mano_verts"].shape) == (2, 778, 3) and p["pred_mano_status"].dtype == torch.int32
    # within the recovery bar of the fit called by hand: 4 * 2^-24 max|coordinate| (the two are the same launches: in fact equal)
    bar = 4 * 2.0 ** -24 * float(by_hand.verts.abs().max())
    assert float((p["pred_mano_verts"] - by_hand.verts).abs().max()) <= bar
    assert torch.equal(p["pred_mano_status"], by_hand.status)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_eval_single_fit_mano(tmp_path, capsys):
    import importlib.util
    import json
    import os
    import poem_v2_amd as pk
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_single_mano_fit", os.path.join(root, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    path = str(tmp_path / "mano.npz")
    np.savez(path, **pk.mano.synthetic_mano_assets(3))
    base = ["--cfg", str(tmp_path / "c.yaml"), "--dataset", "DexYCB", "--view_min", "2", "--view_max", "2", "--model", "small", "-g", "0",
            "--epoch_size", "4", "--mano-assets", path]
    a = es.build_cli().parse_args(base + ["--fit-mano", "--fit-mano-iters", "5"])
    assert (a.fit_mano, a.fit_mano_iters) == (True, 5) and "fit_mano" not in vars(es.build_cli().parse_args(base))
    es.main(a)
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(f"mano_fit_residual_mm = {res['mano_fit_residual_mm']}, mano_fit_flagged = {res['mano_fit_flagged']}")
    assert res["mano_fit_flagged"] == 0 and res["mano_fit_residual_mm"] > 0 and res["samples"] == 4
    es.main(es.build_cli().parse_args(base))
    assert "mano_fit_residual_mm" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with pytest.raises(SystemExit):
        es.main(es.build_cli().parse_args(base[:-2] + ["--fit-mano"]))


def test_eval_single_shards_report_the_betas_error(tmp_path):
    """``evaluate_shards`` with the fit on synthetic records, which carry ``mano_shape``: the result gains the three keys, the betas
    error among them (read at each sample's master row); without the fit none of them."""
    import importlib.util
    import os
    import poem_v2_amd as pk
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_single_mano_fit_shards", os.path.join(root, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    path = str(tmp_path / "mano.npz")
    np.savez(path, **pk.mano.synthetic_mano_assets(3))
    batch = {"cam_view_num": [2, 3, 1], "master_id": torch.tensor([0, 1, 0])}
    assert es.master_rows(batch).tolist() == [0, 3, 5]
    cfg = es.default_cfg()
    view_range = es.edit_cfg(cfg, "DexYCB", "small", [2, 3])
    kw = dict(shard_dir=str(tmp_path / "shards"), dataset="DexYCB", epoch_size=4, batch_size=2, n_cams=4, raw_size=(160, 120),
              backbone="resnet18", backbone_engine="hip", mano_assets=path)
    res = es.evaluate_shards(cfg, view_range, "small", torch.device(DEV), fit_mano_iters=4, **kw)
    print({k: res[k] for k in ("mano_fit_residual_mm", "mano_fit_flagged", "mano_fit_betas_mae")})
    assert res["samples"] == 4 and res["mano_fit_flagged"] == 0
    assert res["mano_fit_residual_mm"] > 0 and np.isfinite(res["mano_fit_betas_mae"]) and res["mano_fit_betas_mae"] > 0
    plain = es.evaluate_shards(cfg, view_range, "small", torch.device(DEV), **kw)
    assert not {"mano_fit_residual_mm", "mano_fit_flagged", "mano_fit_betas_mae"} & set(plain)
    with pytest.raises(SystemExit):
        es.evaluate_shards(cfg, view_range, "small", torch.device(DEV), fit_mano_iters=4, **dict(kw, mano_assets=None))
