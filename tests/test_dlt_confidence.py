"""Confidence-aware triangulation of the reference joints: ``poem_heatmap_uv_conf`` + ``poem_dlt_confidence``
against upstream's own ``triangulate_dlt`` (lib/utils/triangulation.py:111-148) recorded in tests/golden/dlt_conf.npz
(tests/golden/make_golden_dlt_conf.py).  CPU: the fixture regenerates, and an fp64 restatement written here reproduces it,
carry-over of the lowered threshold included.  GPU (``-m gpu``): the kernels through the C ABI and the Python surface up to
the model's ``DLT_CONFIDENCE`` key.

Bars.  5e-6 m against upstream and against the fp64 SVD: the bar tests/test_dlt.py holds the plain DLT to (fp32 M = K.T on
the device against fp64 upstream, rays well apart by the generator's own assertion).  Everything else is equality of bits."""
import importlib.util
import json
import os
import time

import numpy as np
import pytest
import torch

from util import GOLDEN

DEV = "cuda:0"
BAR = 5e-6
CASES = ("all", "occluded", "carry", "high", "zero", "neg")
FIELDS = ("uv", "conf", "K", "E", "T", "X", "out", "count")


def _golden():
    z = np.load(os.path.join(GOLDEN, "dlt_conf.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    assert meta["bar"] == BAR and sorted(meta["cases"]) == sorted(CASES)
    return z, meta["cases"]


def _case(z, cases, name):
    c = {k: z[f"{name}.{k}"] for k in FIELDS}
    c["views"], c["threshold"] = cases[name]["views"], cases[name]["threshold"]
    return c


def _solve64(uv, K, T, scale):
    """fp64 DLT of one joint over the given views: rows (u M[2] - M[0], v M[2] - M[1]) * scale, smallest right singular vector."""
    M = K.astype(np.float64) @ T.astype(np.float64)[:, :3, :]
    uv = uv.astype(np.float64)
    rows = np.concatenate([uv[:, 0:1] * M[:, 2] - M[:, 0], uv[:, 1:2] * M[:, 2] - M[:, 1]], 0)
    vt = np.linalg.svd(rows * np.concatenate([scale, scale])[:, None])[2]
    return vt[-1, :3] / vt[-1, 3]


def restate(uv, conf, K, T, views, mode, threshold=0.5):
    """fp64 restatement of both modes.  threshold: cameras with conf > thr; while at most one and thr > 0, thr -= 0.05; the lowered
    thr is what the sample's next joint starts from.  weighted: every camera, rows scaled by conf.  -> out (B,J,3), count (B,J)."""
    offs = np.concatenate([[0], np.cumsum(views)])
    J = uv.shape[1]
    out, count = np.zeros((len(views), J, 3)), np.zeros((len(views), J), dtype=np.int32)
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        thr = float(threshold)
        for j in range(J):
            cf = conf[s:e, j].astype(np.float64)
            if mode == "threshold":
                while thr > 0 and int((cf > thr).sum()) <= 1:
                    thr -= 0.05
                sel = np.where(cf > thr)[0]
                scale = np.ones(len(sel))
            else:
                sel, scale = np.arange(e - s), cf
            out[b, j] = _solve64(uv[s:e, j][sel], K[s:e][sel], T[s:e][sel], scale)
            count[b, j] = len(sel)
    return out, count


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_fixture_regenerates_from_its_generator():
    spec = importlib.util.spec_from_file_location("make_golden_dlt_conf", os.path.join(GOLDEN, "make_golden_dlt_conf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.isdir(mod.rh.REF_ROOT):
        pytest.skip("reference tree absent: golden vectors regenerate in the build container only")
    rec = mod.build()
    z, _ = _golden()
    assert sorted(rec) == sorted(z.files)
    for k in z.files:
        if k.endswith(".out") or k.endswith(".plain"):
            assert np.abs(rec[k] - z[k]).max() < 1e-12, k          # an SVD's last bits may depend on the LAPACK build
        else:
            assert rec[k].dtype == z[k].dtype and np.array_equal(rec[k], z[k]), k


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_upstream(name):
    z, cases = _golden()
    c = _case(z, cases, name)
    assert c["out"].dtype == np.float64 and c["uv"].dtype == np.float32 and c["conf"].dtype == np.float32
    out, count = restate(c["uv"], c["conf"], c["K"], c["T"], c["views"], "threshold", c["threshold"])
    assert np.array_equal(count, c["count"])
    assert np.abs(out - c["out"]).max() < 1e-9
    assert c["count"].min() >= 2


def test_carry_over_changes_later_selections():
    """Case (c): some LATER joint of every sample uses other cameras than a fresh 0.5 would give it, in upstream's run and in the
    restatement alike; a restatement that restarts at 0.5 per joint reproduces ``count_fresh`` and not ``count``."""
    z, cases = _golden()
    c = _case(z, cases, "carry")
    fresh = z["carry.count_fresh"]
    differs = c["count"] != fresh
    assert differs.any(axis=1).all()
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        dropped = int(np.argmax((c["conf"][s:e] > 0.5).sum(0) <= 1))        # the joint where only one camera clears 0.5
        assert (c["conf"][s:e, dropped] > 0.5).sum() == 1
        assert differs[b, :dropped + 1].sum() == 0 and differs[b, dropped + 1:].sum() >= 1
    per_joint = np.stack([restate(c["uv"][:, j:j + 1], c["conf"][:, j:j + 1], c["K"], c["T"], c["views"], "threshold", 0.5)[1][:, 0]
                          for j in range(21)], 1)
    assert np.array_equal(per_joint, fresh)


@pytest.mark.parametrize("name", ["all", "occluded"])
def test_recorded_outputs_recover_the_noise_free_joints(name):
    z, cases = _golden()
    c = _case(z, cases, name)
    assert np.abs(c["out"] - c["X"]).max() < BAR
    out, _ = restate(c["uv"], c["conf"], c["K"], c["T"], c["views"], "threshold", c["threshold"])
    assert np.abs(out - c["X"]).max() < BAR
    if name == "occluded":                                            # what the feature is for
        assert np.linalg.norm(z["occluded.plain"] - c["X"], axis=-1).min() > 0.01


# ---- GPU ----------------------------------------------------------------------------------------------------------
def _dev(c, *names):
    return [torch.from_numpy(np.ascontiguousarray(c[n])).to(DEV) for n in names]


def _tri(c, mode, threshold=None, conf=None, **kw):
    import poem_v2_amd as pk
    uv, cf, K, T = _dev(c, "uv", "conf", "K", "T")
    return pk.triangulation.triangulate_reference_joints(uv, K, T, c["views"], conf=cf if conf is None else conf, mode=mode,
                                                         threshold=c["threshold"] if threshold is None else threshold,
                                                         invert=False, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_threshold_mode_matches_upstream(name):
    z, cases = _golden()
    c = _case(z, cases, name)
    got, count = _tri(c, "threshold", return_count=True)
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), c["count"])
    err = float(np.abs(got.double().cpu().numpy() - c["out"]).max())
    print(f"{name}: max |hip - upstream| = {err:.3e} m")
    assert err < BAR
    assert torch.equal(_tri(c, "threshold"), got)                          # sel_count is optional (NULL)
    # cam_extr (camera->master) inverted on the device, as the model calls it
    import poem_v2_amd as pk
    uv, cf, K, E = _dev(c, "uv", "conf", "K", "E")
    inv = pk.triangulation.triangulate_reference_joints(uv, K, E, c["views"], conf=cf, mode="threshold", threshold=c["threshold"])
    assert float(np.abs(inv.double().cpu().numpy() - c["out"]).max()) < BAR


@pytest.mark.gpu
def test_hip_upstream_signature_one_sample():
    import poem_v2_amd as pk
    z, cases = _golden()
    c = _case(z, cases, "carry")
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        got = pk.triangulation.triangulate_dlt(c["uv"][s:e], c["conf"][s:e], c["K"][s:e], c["T"][s:e], 0.5)
        assert isinstance(got, np.ndarray) and got.shape == (21, 3) and got.dtype == np.float32
        assert np.abs(got - c["out"][b]).max() < BAR
    s, e = offs[0], offs[1]
    dflt = pk.triangulation.triangulate_dlt(*[torch.from_numpy(c[k][s:e]).to(DEV) for k in ("uv", "conf", "K", "T")])
    assert dflt.is_cuda and float(np.abs(dflt.double().cpu().numpy() - c["out"][0]).max()) < BAR


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["occluded", "carry", "zero"])
def test_hip_weighted_mode_matches_fp64_svd(name):
    z, cases = _golden()
    c = _case(z, cases, name)
    if name == "zero":
        c["conf"] = np.maximum(c["conf"], np.float32(0.02))               # (a weight of exactly 0 on one of two views is no DLT)
    want, _ = restate(c["uv"], c["conf"], c["K"], c["T"], c["views"], "weighted")
    got, count = _tri(c, "weighted", return_count=True)
    assert np.array_equal(count.cpu().numpy(), np.repeat(np.asarray(c["views"], dtype=np.int32)[:, None], 21, 1))
    err = float(np.abs(got.double().cpu().numpy() - want).max())
    print(f"{name}: max |hip weighted - fp64 SVD| = {err:.3e} m")
    assert err < BAR
    if name == "occluded":                 # weights pull the answer towards the good views, they do not remove the bad ones
        plain = np.linalg.norm(z["occluded.plain"] - c["X"], axis=-1)
        assert (np.linalg.norm(want - c["X"], axis=-1) < plain).all()


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [True, False])
def test_hip_reproduces_plain_dlt_bit_for_bit(invert):
    """conf == 1 everywhere (weighted), a threshold of 0 or below with positive confidences, a threshold every view clears."""
    import poem_v2_amd as pk
    z, cases = _golden()
    for name in ("all", "occluded", "carry"):
        c = _case(z, cases, name)
        uv, cf, K = _dev(c, "uv", "conf", "K")
        mat = _dev(c, "E" if invert else "T")[0]
        tri = lambda **kw: pk.triangulation.triangulate_reference_joints(uv, K, mat, c["views"], invert=invert, **kw)  # noqa: E731
        plain = tri()
        assert torch.equal(tri(conf=torch.ones_like(cf), mode="weighted"), plain)
        assert torch.equal(tri(conf=cf, mode="threshold", threshold=0.0), plain)
        assert torch.equal(tri(conf=cf, mode="threshold", threshold=-1.0), plain)
        assert torch.equal(tri(conf=torch.full_like(cf, 0.75), mode="threshold", threshold=0.5), plain)
        assert torch.equal(tri(conf=cf, mode="off"), plain)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["threshold", "weighted"])
def test_hip_sample_alone_equals_sample_in_ragged_batch(mode):
    import poem_v2_amd as pk
    z, cases = _golden()
    for name in ("occluded", "carry", "high"):
        c = _case(z, cases, name)
        full, count = _tri(c, mode, return_count=True)
        offs = np.concatenate([[0], np.cumsum(c["views"])])
        for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
            uv, cf, K, T = [torch.from_numpy(c[k][s:e]).to(DEV) for k in ("uv", "conf", "K", "T")]
            one, n1 = pk.triangulation.triangulate_reference_joints(uv, K, T, [c["views"][b]], conf=cf, mode=mode,
                                                                    threshold=c["threshold"], invert=False, return_count=True)
            assert torch.equal(one[0], full[b]) and torch.equal(n1[0], count[b])


def _j70_inputs():
    """70 joints (more than one 64-thread block of dlt_kernel, more than one stride of dlt_conf_kernel's joint loop) of 3 samples
    with 2 / 3 / 4 views: the synthetic batch's cameras, points within 8 cm of each sample's hand, 1.5 px of noise, confidences
    in (0.05, 1)."""
    import poem_v2_amd as pk
    views = [2, 3, 4]
    b = pk.inputs.synthetic_batch(views, seed=70)
    K, E = b["img_metas"]["cam_intr"], b["img_metas"]["cam_extr"]
    T = torch.linalg.inv(E)
    g = torch.Generator().manual_seed(170)
    X = b["reference_joints"].mean(1, keepdim=True) + 0.08 * (torch.rand(len(views), 70, 3, generator=g) * 2 - 1)
    Xv = X[torch.repeat_interleave(torch.arange(len(views)), torch.tensor(views))]
    pc = (T[:, None, :3, :3] @ Xv[..., None]).squeeze(-1) + T[:, None, :3, 3]
    q = (K[:, None] @ pc[..., None]).squeeze(-1)
    uv = q[..., :2] / q[..., 2:] + 1.5 * torch.randn(sum(views), 70, 2, generator=g)
    conf = 0.05 + 0.95 * torch.rand(sum(views), 70, generator=g)
    return views, [t.contiguous().to(DEV) for t in (uv, conf, K, E, T)]


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [True, False])
def test_hip_one_solve_behind_both_kernels_at_70_joints(invert):
    """dlt_kernel and dlt_conf_kernel run one solve: at J = 70 the plain route equals the weighted route with confidence 1 and the
    threshold route with threshold 0 bit for bit, and on every route a sample alone equals the same sample in the ragged batch."""
    import poem_v2_amd as pk
    views, (uv, cf, K, E, T) = _j70_inputs()
    mat = E if invert else T
    tri = pk.triangulation.triangulate_reference_joints
    plain = tri(uv, K, mat, views, invert=invert)
    assert plain.shape == (3, 70, 3) and bool(torch.isfinite(plain).all())
    assert torch.equal(tri(uv, K, mat, views, invert=invert, conf=torch.ones_like(cf), mode="weighted"), plain)
    assert torch.equal(tri(uv, K, mat, views, invert=invert, conf=cf, mode="threshold", threshold=0.0), plain)
    offs = np.concatenate([[0], np.cumsum(views)])
    for mode in (None, "threshold", "weighted"):
        kw = dict(invert=invert) if mode is None else dict(invert=invert, mode=mode, threshold=0.5, return_count=True)
        full = tri(uv, K, mat, views, conf=cf, **kw)
        for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
            one = tri(uv[s:e], K[s:e], mat[s:e], [views[b]], conf=cf[s:e], **kw)
            if mode is None:
                assert torch.equal(one[0], full[b]), b
            else:                                                          # (joints, camera counts)
                assert torch.equal(one[0][0], full[0][b]) and torch.equal(one[1][0], full[1][b]), (mode, b)


@pytest.mark.gpu
def test_hip_feature_recovers_occluded_views():
    """Case (b) on the device: the plain DLT is more than 1 cm from the true joints on every joint, threshold mode is back on
    upstream's answer (5e-6 m), which is the true joints."""
    import poem_v2_amd as pk
    z, cases = _golden()
    c = _case(z, cases, "occluded")
    uv, K, T = _dev(c, "uv", "K", "T")
    plain = pk.triangulation.triangulate_reference_joints(uv, K, T, c["views"], invert=False).double().cpu().numpy()
    miss = np.linalg.norm(plain - c["X"], axis=-1)
    print(f"plain DLT misses by {miss.min() * 100:.2f}..{miss.max() * 100:.2f} cm")
    assert miss.min() > 0.01
    assert np.abs(plain - z["occluded.plain"]).max() < BAR
    got = _tri(c, "threshold").double().cpu().numpy()
    assert np.abs(got - c["out"]).max() < BAR and np.abs(got - c["X"]).max() < 2 * BAR


def _heatmaps(seed=44, views=5):
    g = torch.Generator().manual_seed(seed)
    return torch.sigmoid(4.0 * torch.randn(views, 21, 32, 32, generator=g) - 3.0)


@pytest.mark.gpu
def test_hip_heatmap_confidence():
    import poem_v2_amd as pk
    for hm, (w, h) in ((_heatmaps(), (256.0, 256.0)), (_heatmaps(7, 3)[:, :, :24, :20].contiguous(), (320.0, 240.0))):
        d = hm.to(DEV)
        uv, conf = pk.triangulation.heatmap_to_uv(d, w, h, return_conf=True)
        assert torch.equal(uv, pk.triangulation.heatmap_to_uv(d, w, h))               # bit-identical read-out
        assert conf.shape == hm.shape[:2] and torch.equal(conf, d.amax((-2, -1))) and torch.equal(conf.cpu(), hm.amax((-2, -1)))
        assert float(conf.min()) > 0 and float(conf.max()) < 1
    bad = _heatmaps()
    bad[1, 3, 7, 30] = float("nan")                       # one NaN pixel, not the lane's first or last: the map's confidence is NaN
    bad[2, 0, 0, 0] = float("nan")
    uv, conf = pk.triangulation.heatmap_to_uv(bad.to(DEV), 256.0, 256.0, return_conf=True)
    want = bad.amax((-2, -1))
    assert torch.equal(torch.isnan(conf).cpu(), torch.isnan(want)) and int(torch.isnan(want).sum()) == 2
    ok = ~torch.isnan(want)
    assert torch.equal(conf.cpu()[ok], want[ok])
    with pytest.raises(RuntimeError):
        pk.triangulation.heatmap_to_uv(bad, 256.0, 256.0, return_conf=True)              # CPU tensors: no fallback


@pytest.mark.gpu
def test_hip_confidence_same_through_both_readout_routes():
    """uv_decode with the read-out head fused into its last convolution, and as two launches: ``heatmap_stage(return_conf=True)``
    gives the same uv and confidence bits either way, equal to the stand-alone kernel on the maps and to their amax."""
    import decode_oracle as do
    import poem_v2_amd as pk
    feats = [f.to(DEV) for f in do.synthetic_mlvl_feats(5, 3)]
    dec = pk.decode.FeatureDecoders(do.seeded_decoder_state(3), DEV)
    assert dec.fuse_pool_head
    uv_f, conf_f = dec.heatmap_stage(feats, 256, 256, return_conf=True)
    assert torch.equal(uv_f, dec.heatmap_stage(feats, 256, 256))
    hm = dec.uv_decode(feats)
    uv_s, conf_s = pk.triangulation.heatmap_to_uv(hm, 256, 256, return_conf=True)
    assert torch.equal(conf_f, conf_s) and torch.equal(uv_f, uv_s) and torch.equal(conf_f, hm.amax((-2, -1)))
    dec.fuse_pool_head = False
    uv_2, conf_2 = dec.heatmap_stage(feats, 256, 256, return_conf=True)
    assert torch.equal(conf_2, conf_f) and torch.equal(uv_2, uv_f)
    rj = pk.triangulation.reference_joints_from_heatmaps
    b = pk.inputs.synthetic_batch([2, 3], seed=1)["img_metas"]
    K, E = b["cam_intr"].to(DEV), b["cam_extr"].to(DEV)
    assert torch.equal(rj(hm, K, E, [2, 3], 256, 256, mode="threshold", threshold=0.0), rj(hm, K, E, [2, 3], 256, 256))


@pytest.mark.gpu
def test_hip_arguments_are_checked():
    import poem_v2_amd as pk
    z, cases = _golden()
    c = _case(z, cases, "all")
    with pytest.raises(ValueError):
        _tri(c, "median")
    with pytest.raises(ValueError):
        _tri(c, "threshold", conf=torch.ones(3, 21, device=DEV))
    for thr in (float("inf"), float("nan"), 1e9):          # the lowering loop would never end
        with pytest.raises(ValueError):
            _tri(c, "threshold", threshold=thr)
    uv, cf, K, T = _dev(c, "uv", "conf", "K", "T")
    out = torch.empty(len(c["views"]), 21, 3, device=DEV)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(c["views"])]), dtype=torch.int32, device=DEV)
    call = lambda mode, thr: pk.hip.lib().poem_dlt_confidence(uv.data_ptr(), cf.data_ptr(), K.data_ptr(), T.data_ptr(),  # noqa: E731
                                                              offs.data_ptr(), out.data_ptr(), None, len(c["views"]), 21, 0, mode,
                                                              thr, pk.hip.stream())
    assert call(0, 0.5) == -1 and call(3, 0.5) == -1 and call(1, float("inf")) == -1 and call(1, float("nan")) == -1
    assert call(2, float("nan")) == 0                      # weighted mode does not read the threshold
    assert pk.hip.lib().poem_heatmap_uv_conf(uv.data_ptr(), uv.data_ptr(), None, 1, 1, 2, 2, 1.0, 1.0, pk.hip.stream()) == -1


def _queue_busy_gpu(ms):
    """A kernel that keeps the current stream busy for about `ms` milliseconds, so that anything the host waits for shows."""
    cycles = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(cycles)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    torch.cuda.synchronize()
    per_ms = cycles / max(a.elapsed_time(b), 1e-3)
    torch.cuda._sleep(int(per_ms * ms))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["threshold", "weighted"])
def test_hip_confidence_stage_is_stream_ordered(mode):
    """Read-out with confidence + confidence DLT issued twice behind a long kernel: the host is back while that kernel still runs
    (a blocking copy or a synchronisation would have waited for it), and the results are right once it has drained."""
    import poem_v2_amd as pk
    z, cases = _golden()
    c = _case(z, cases, "carry")
    hm = _heatmaps().to(DEV)
    uv, cf, K, T = _dev(c, "uv", "conf", "K", "T")          # resident before the clock starts: a pageable upload does wait
    run = lambda: (pk.triangulation.heatmap_to_uv(hm, 256.0, 256.0, return_conf=True),     # noqa: E731
                   pk.triangulation.triangulate_reference_joints(uv, K, T, c["views"], conf=cf, mode=mode, threshold=0.5,
                                                                 invert=False, return_count=True))
    (uv0, conf0), (rj0, n0) = run()                        # the view layout is staged once per layout (triangulation._offsets)
    torch.cuda.synchronize()
    _queue_busy_gpu(400)
    t0 = time.perf_counter()
    first, second = run(), run()
    done = torch.cuda.Event()
    done.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    still_busy = not done.query()
    torch.cuda.synchronize()
    assert still_busy, f"the host was held until the stream drained ({host_ms:.1f} ms)"
    for (uv1, conf), (rj, n) in (first, second):
        assert torch.equal(uv1, uv0) and torch.equal(conf, conf0) and torch.equal(rj, rj0) and torch.equal(n, n0)


def _build_model(extra):
    import poem_oracle as po
    import poem_v2_amd as pk
    from poem_v2_amd import backbone as bb
    cfg = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": pk.configs.head_cfg(128), "DATA_PRESET": {"CENTER_IDX": 9}, **extra}
    model = pk.build_model(pk.CN(cfg))
    model.load_parts(bb.seeded_hrnet_state_dict(0), pk.weights.seeded_decoder_state_dict(0), pk.weights.seeded_state_dict(128, seed=0),
                     template=po.synthetic_template(1234))
    return model


PRED_KEYS_TODAY = {"pred_joints_3d", "pred_verts_3d", "pred_joints_3d_rel", "pred_verts_3d_rel", "pred_joints_uv",
                   "pred_ref_joints_3d"}


@pytest.mark.gpu
def test_model_dlt_confidence_key():
    """One backbone pyramid through four models that differ in the key alone.  Absent / "off": the key set and every tensor of
    today's forward.  "threshold" at 0: the same bits plus ``pred_joints_conf``.  "threshold" at 0.5 and "weighted": the reference
    joints are the stage functions' on the model's own uv and confidence.  No mode holds the host where today's forward does not
    (the confidence stage by itself is held to "never": test_hip_confidence_stage_is_stream_ordered)."""
    import poem_v2_amd as pk
    views = [3, 2]
    b = pk.inputs.synthetic_batch(views, seed=4)
    img = pk.inputs.synthetic_images(sum(views), seed=4).to(DEV)
    K, E = b["img_metas"]["cam_intr"].to(DEV), b["img_metas"]["cam_extr"].to(DEV)
    batch = {"image": img, "target_cam_intr": K, "target_cam_extr": E, "master_id": [0] * len(views), "cam_view_num": np.asarray(views)}
    models = {"absent": _build_model({}), "off": _build_model({"DLT_CONFIDENCE": "off"}),
              "thr0": _build_model({"DLT_CONFIDENCE": "threshold", "DLT_CONFIDENCE_THRESHOLD": 0.0}),
              "thr": _build_model({"DLT_CONFIDENCE": "threshold"}),
              "weighted": _build_model({"DLT_CONFIDENCE": "weighted", "DLT_CONFIDENCE_THRESHOLD": 0.3})}
    assert models["thr"].dlt_threshold == 0.5 and models["absent"].dlt_confidence == "off"
    with pytest.raises(ValueError):
        _build_model({"DLT_CONFIDENCE": "median"})
    pyr = models["absent"].extract_img_feat(img)            # one pyramid for all (MIOpen may pick other solvers on a later call)
    preds = {}
    for name, m in models.items():
        m.extract_img_feat = lambda x: pyr
        preds[name] = {k: v.clone() if torch.is_tensor(v) else v for k, v in m(batch, 0, mode="test").items()}
    base = preds["absent"]
    today = models["absent"].decoders.heatmap_stage(pyr, 256, 256)
    rj_today = pk.triangulation.triangulate_reference_joints(today, K, E, views)
    assert torch.equal(base["pred_joints_uv"], today) and torch.equal(base["pred_ref_joints_3d"], rj_today)
    head_keys = set(base) - PRED_KEYS_TODAY
    assert "all_coords_preds" in head_keys and "pred_joints_conf" not in base
    assert set(preds["off"]) == set(base)
    for k in base:
        if torch.is_tensor(base[k]):
            assert torch.equal(preds["off"][k], base[k]), k
    for name in ("thr0", "thr", "weighted"):
        p = preds[name]
        assert set(p) == set(base) | {"pred_joints_conf"}
        assert tuple(p["pred_joints_conf"].shape) == (sum(views), 21)
        assert torch.equal(p["pred_joints_uv"], base["pred_joints_uv"])
        assert torch.equal(p["pred_joints_conf"], models[name].decoders.uv_decode(pyr).amax((-2, -1)))
    for k in base:
        if torch.is_tensor(base[k]):
            assert torch.equal(preds["thr0"][k], base[k]), k
    uv, conf = base["pred_joints_uv"], preds["thr"]["pred_joints_conf"]
    for name, mode, thr in (("thr", "threshold", 0.5), ("weighted", "weighted", 0.3)):
        want = pk.triangulation.triangulate_reference_joints(uv, K, E, views, conf=conf, mode=mode, threshold=thr)
        assert torch.equal(preds[name]["pred_ref_joints_3d"], want)
        assert torch.isfinite(preds[name]["all_coords_preds"]).all()
    # no ADDED host synchronisation: two forwards back to back behind a long kernel.  Where today's forward ("absent") is back
    # while that kernel still runs, so is every mode's (a blocking copy or a synchronisation would have waited for it)
    busy = {}
    for name, m in models.items():
        for _ in range(3):
            m(batch, 0, mode="test")                        # graphs captured, layouts resident
        torch.cuda.synchronize()
        _queue_busy_gpu(600)
        t0 = time.perf_counter()
        a, c = m(batch, 0, mode="test"), m(batch, 0, mode="test")
        done = torch.cuda.Event()
        done.record()
        host_ms = (time.perf_counter() - t0) * 1e3
        busy[name] = not done.query()
        torch.cuda.synchronize()
        print(f"{name}: two forwards issued in {host_ms:.1f} ms of host time, stream still busy: {busy[name]}")
        assert torch.equal(a["all_coords_preds"], preds[name]["all_coords_preds"])
        assert torch.equal(c["all_coords_preds"], preds[name]["all_coords_preds"])
    for name in ("off", "thr0", "thr", "weighted"):
        assert busy[name] or not busy["absent"], f"{name}: the host was held until the stream drained; without the key it is not"
