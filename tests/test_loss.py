"""The loss kernel on the GPU (csrc/loss.hip through ``PoemLoss`` and the C entry): every fixture case against the fixture's fp64 values
(1e-9 relative: same inputs, same precision, another summation order and inverse) and against upstream's own fp32 ``loss_dict``
(2e-6 + 1e-9: the fixture's condition, tests/test_loss_host.py), NaN propagation, the clamp at its bound, reproducibility, view order,
the workspace contract, stream order and the model-level wiring.  Inputs that are not in the fixture are held against
``test_loss_host.restate``."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

from test_loss_host import ALL_KEYS, CASES, _dicts, _poem_loss, fixture, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_RUNS = {}


def run_case(name, inp=None, **over):
    """PoemLoss on a fixture case (or on edited inputs / meta fields of it) -> ({key: float}, raw (10,) fp64 result, loss_dict)."""
    cases, jreg = fixture()
    c = dict(cases[name], **over)
    if inp is not None:
        c["inp"] = inp
    preds, gt = _dicts(c, DEV)
    loss, d = _poem_loss(c, jreg)(preds, gt)
    assert loss is d["loss"]
    buf = d["loss"]._base
    assert buf is not None and buf.dtype == torch.float64 and buf.numel() == 10 and all(v._base is buf and v.dim() == 0 for v in d.values())
    raw = buf.cpu().numpy().copy()
    return {k: float(v) for k, v in d.items()}, raw, d


def clean(name):
    if name not in _RUNS:
        _RUNS[name] = run_case(name)[:2]
    return _RUNS[name]


def weighted_sums(c, raw):
    t, lo = dict(zip(ALL_KEYS, raw)), c["loss"]
    recon = lo["JOINTS_LOSS_WEIGHT"] * (t["loss_3d_joints"] + t["loss_3d_joints_from_mesh"]) + lo["VERTICES_LOSS_WEIGHT"] * t["loss_3d_verts"] \
        + lo["JOINTS_2D_LOSS_WEIGHT"] * t["loss_2d_joints"] + lo.get("VERTICES_2D_LOSS_WEIGHT", 0.0) * t["loss_2d_verts"] \
        + lo.get("POSE_LOSS_WEIGHT", 0.001) * t["loss_pose"] + lo.get("SHAPE_LOSS_WEIGHT", 0.0005) * t["loss_shape"]
    return recon, lo["HEATMAP_JOINTS_WEIGHT"] * t["loss_heatmap_joints"] + recon


@pytest.mark.parametrize("name", CASES)
def test_every_term_against_the_fixture(name):
    c = fixture()[0][name]
    got, raw = clean(name)
    assert list(got) == c["keys"]
    for k, r64, r32 in zip(c["keys"], c["ref64"], c["ref32"]):
        print(f"{name}.{k}: hip {got[k]!r} fp64 {r64!r} upstream {r32!r}")
    for k, r64, r32 in zip(c["keys"], c["ref64"], c["ref32"]):
        if k in c["nan_keys"]:
            assert math.isnan(got[k]), k
            continue
        assert abs(got[k] - r64) <= 1e-9 * abs(r64), (k, got[k], r64)
        assert abs(got[k] - float(r32)) <= (2e-6 + 1e-9) * abs(r64), (k, got[k], r32)
    for k, slot in zip(ALL_KEYS, raw):                      # disabled terms: absent from the dict, exactly 0 in the buffer
        if k not in c["keys"]:
            assert slot == 0.0 and not np.signbit(slot), k
    if not c["nan_keys"]:
        recon, loss = weighted_sums(c, raw)
        assert abs(got["loss_recon"] - recon) <= 1e-12 * abs(recon) and abs(got["loss"] - loss) <= 1e-12 * abs(loss)


def test_nan_reaches_upstreams_terms_and_no_other():
    c = fixture()[0]["nan"]
    got, raw = clean("nan")
    base, raw0 = clean("release")
    assert [k for k in c["keys"] if math.isnan(got[k])] == c["nan_keys"]
    for k, a, b in zip(ALL_KEYS, raw, raw0):
        if k not in c["nan_keys"]:
            assert a.tobytes() == b.tobytes(), k            # the bits of the clean run


def test_clamp_at_its_bound():
    """320 x 240 makes the scale 400 and the bound 200 exactly; through a master view (identity extrinsic) a joint at (0.5, 0.25, 1)
    projects to (278, 203) exactly, so three targets put three offsets on +200, -200, +200: the result is the restatement's."""
    cases, jreg = fixture()
    c = cases["clamp"]
    inp = {k: v.copy() for k, v in c["inp"].items()}
    assert np.array_equal(inp["E"][0], np.eye(4)) and np.array_equal(inp["E"][4], np.eye(4)) and inp["K"][0, 0, 2] == 128
    inp["coords"][0, 2] = inp["coords"][1, 7] = (0.5, 0.25, 1.0)
    inp["gt_uv"][0, 2] = (78.0, 403.0)
    inp["gt_uv"][4, 7, 0] = 78.0
    got, _, _ = run_case("clamp", inp=inp, H=240, W=320)
    want = restate(inp, c["views"], c["loss"], c["parametric"], c["center_idx"], 240, 320, jreg)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (k, got[k], want[k])
    inside = {k: v.copy() for k, v in inp.items()}
    inside["gt_uv"][0, 2] = (78.0 + 1e-3, 403.0 - 1e-3)     # just inside the bound: the term moves, so the three offsets do count
    assert run_case("clamp", inp=inside, H=240, W=320)[0]["loss_2d_joints"] < got["loss_2d_joints"]


def test_two_runs_give_the_same_bits():
    a, b = run_case("many")[1], run_case("many")[1]
    assert a.tobytes() == b.tobytes() and a.tobytes() == clean("many")[1].tobytes()


def test_view_order_inside_a_sample():
    c = fixture()[0]["allterms"]
    rng = np.random.RandomState(3)
    perm, s = [], 0
    for n in c["views"]:
        perm += [s] + (s + 1 + rng.permutation(n - 1)).tolist()          # the master view stays first
        s += n
    assert sorted(perm) == list(range(s)) and perm != list(range(s))
    inp = {k: (v[perm] if k in ("pred_uv", "gt_uv", "K", "E", "mano_pose", "mano_shape") else v) for k, v in c["inp"].items()}
    got, raw, _ = run_case("allterms", inp=inp)
    base, raw0 = clean("allterms")
    for k in base:
        assert abs(got[k] - base[k]) <= 1e-12 * abs(base[k]), (k, got[k], base[k])
    for k in ("loss_pose", "loss_shape", "loss_3d_joints", "loss_3d_verts"):
        assert got[k] == base[k], k


def _raw_call(c, jreg, views=None, ws_short=0, null=None, total_views=None):
    """poem_loss_terms called directly; the result buffer starts as a sentinel -> (return code, buffer afterwards)."""
    import poem_v2_amd as pk
    L = pk.hip.lib()
    views = c["views"] if views is None else views
    B, BN = len(views), sum(views) if total_views is None else total_views
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c["inp"].items()}
    offs = torch.tensor(np.concatenate([[0], np.cumsum(views)]), dtype=torch.int32, device=DEV)
    J = torch.from_numpy(jreg).to(DEV)
    lo = c["loss"]
    cfg = pk.hip.PoemLossCfg(lo["JOINTS_LOSS_WEIGHT"], lo["VERTICES_LOSS_WEIGHT"], lo["JOINTS_2D_LOSS_WEIGHT"], lo.get("VERTICES_2D_LOSS_WEIGHT", 0.0),
                             lo["HEATMAP_JOINTS_WEIGHT"], 0.001, 0.0005, int(lo["JOINTS_LOSS_TYPE"] == "l2"), int(lo["VERTICES_LOSS_TYPE"] == "l2"),
                             int(c["parametric"]), c["center_idx"], c["H"], c["W"])
    need = L.poem_loss_workspace_bytes(B, min(BN, 65535))
    ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=DEV)
    out = torch.full((10,), -7.0, dtype=torch.float64, device=DEV)
    p = {k: (v.data_ptr() if k != null else None) for k, v in dict(t, jreg=J, offs=offs, out=out, ws=ws).items()}
    rc = L.poem_loss_terms(p["coords"], p["pred_uv"], p.get("pred_pose"), p.get("pred_shape"), p["gt_joints"], p["gt_verts"], p["gt_uv"], p["K"],
                           p["E"], p["offs"], p.get("mano_pose"), p.get("mano_shape"), p["jreg"], None if null == "cfg" else ctypes.byref(cfg),
                           B, BN, p["out"], p["ws"], need - ws_short, pk.hip.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def test_workspace_and_argument_contract():
    import poem_v2_amd as pk
    cases, jreg = fixture()
    c = cases["allterms"]
    L = pk.hip.lib()
    assert L.poem_loss_workspace_bytes(4, 18) == 8 * (18 * 4 * 3 + 4 * 5) and L.poem_loss_workspace_bytes(0, 3) == 0
    untouched = np.full(10, -7.0)
    rc, out = _raw_call(c, jreg)
    assert rc == 0 and np.array_equal(out, clean("allterms")[1])                       # the C entry by itself: PoemLoss's bits
    rc, out = _raw_call(c, jreg, ws_short=1)
    assert rc == -2 and np.array_equal(out, untouched)                                 # POEM_E_WORKSPACE, nothing launched
    rc, out = _raw_call(c, jreg, total_views=65536)
    assert rc == -4 and np.array_equal(out, untouched)                                 # POEM_E_UNSUPPORTED
    for null in ("coords", "pred_uv", "gt_joints", "gt_verts", "gt_uv", "K", "E", "offs", "jreg", "cfg", "out", "ws", "pred_pose", "mano_shape"):
        rc, out = _raw_call(c, jreg, null=null)
        assert rc == -1 and np.array_equal(out, untouched), null                       # POEM_E_ARG
    rc, out = _raw_call(c, jreg, total_views=3)                                        # fewer views than samples
    assert rc == -1 and np.array_equal(out, untouched)
    rc, _ = _raw_call(cases["release"], jreg, null="pred_pose")                         # not parametric: pose / shape are not read
    assert rc == 0


def _queue_busy_gpu(ms):
    cycles = 20_000_000
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(cycles)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    torch.cuda.synchronize()
    torch.cuda._sleep(int(cycles / max(a.elapsed_time(b), 1e-3) * ms))


def test_call_and_feed_are_stream_ordered():
    """PoemLoss and LossMetric.feed issued twice behind a long kernel: the host is back while that kernel still runs."""
    import poem_v2_amd as pk
    cases, jreg = fixture()
    c = cases["allterms"]
    preds, gt = _dicts(c, DEV)                               # resident before the clock starts: a pageable upload does wait
    lo = _poem_loss(c, jreg)
    lo.set_j_regressor(torch.from_numpy(jreg).to(DEV))
    metric = pk.LossMetric(None)
    metric.feed(lo(preds, gt)[1], 4)                         # the view layout is staged once per layout; the metric learns its keys
    torch.cuda.synchronize()
    _queue_busy_gpu(300)
    t0 = time.perf_counter()
    for _ in range(2):
        metric.feed(lo(preds, gt)[1], 4)
    done = torch.cuda.Event()
    done.record()
    host_ms = (time.perf_counter() - t0) * 1e3
    still_busy = not done.query()
    torch.cuda.synchronize()
    assert still_busy, f"the host was held until the stream drained ({host_ms:.1f} ms)"
    want = clean("allterms")[0]
    got = metric.get_measures()
    assert list(got) == c["keys"] and metric.count == 12
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-15 * abs(want[k]), k


def test_at_most_two_kernel_launches():
    """The C entry captured into a HIP graph (never replayed): its nodes are the launches it issues."""
    import poem_v2_amd as pk
    hiprt = pk.hip.lib()                                     # the HIP runtime the library itself is linked against
    cases, jreg = fixture()
    c = cases["allterms"]
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c["inp"].items()}
    B, BN = len(c["views"]), sum(c["views"])
    offs = torch.tensor(np.concatenate([[0], np.cumsum(c["views"])]), dtype=torch.int32, device=DEV)
    J = torch.from_numpy(jreg).to(DEV)
    lo = c["loss"]
    cfg = pk.hip.PoemLossCfg(lo["JOINTS_LOSS_WEIGHT"], lo["VERTICES_LOSS_WEIGHT"], lo["JOINTS_2D_LOSS_WEIGHT"], lo["VERTICES_2D_LOSS_WEIGHT"],
                             lo["HEATMAP_JOINTS_WEIGHT"], 0.001, 0.0005, 0, 1, 1, c["center_idx"], c["H"], c["W"])
    need = pk.hip.lib().poem_loss_workspace_bytes(B, BN)
    ws = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(10, dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    sp = ctypes.c_void_p(side.cuda_stream)
    assert hiprt.hipStreamBeginCapture(sp, 2) == 0                                      # hipStreamCaptureModeRelaxed
    rc = pk.hip.lib().poem_loss_terms(t["coords"].data_ptr(), t["pred_uv"].data_ptr(), t["pred_pose"].data_ptr(), t["pred_shape"].data_ptr(),
                                      t["gt_joints"].data_ptr(), t["gt_verts"].data_ptr(), t["gt_uv"].data_ptr(), t["K"].data_ptr(),
                                      t["E"].data_ptr(), offs.data_ptr(), t["mano_pose"].data_ptr(), t["mano_shape"].data_ptr(), J.data_ptr(),
                                      ctypes.byref(cfg), B, BN, out.data_ptr(), ws.data_ptr(), need, side.cuda_stream)
    assert hiprt.hipStreamEndCapture(sp, ctypes.byref(graph)) == 0
    assert rc == 0
    assert hiprt.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    hiprt.hipGraphDestroy(graph)
    assert 1 <= n.value <= 2, n.value


def test_model_compute_loss():
    """PtEmbedMultiviewStereoV2 with cfg.LOSS on a two-sample batch, views [2,3]: compute_loss on the forward's own preds is the
    restatement's; without cfg.LOSS compute_loss raises and the forward returns the same keys and bits."""
    import poem_oracle as po
    import poem_v2_amd as pk
    from poem_v2_amd import backbone as bb
    _, jreg = fixture()
    views = [2, 3]

    def build(extra):
        cfg = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": pk.configs.head_cfg(128), "DATA_PRESET": {"CENTER_IDX": 9}, **extra}
        m = pk.build_model(pk.CN(cfg))
        return m.load_parts(bb.seeded_hrnet_state_dict(0), pk.weights.seeded_decoder_state_dict(0), pk.weights.seeded_state_dict(128, seed=0),
                            template=po.synthetic_template(1234))

    loss_node = dict(pk.configs.loss_cfg(VERTICES_2D_LOSS_WEIGHT=0.25))
    plain, model = build({}), build({"LOSS": loss_node})
    b = pk.inputs.synthetic_batch(views, seed=4)
    g = torch.Generator().manual_seed(44)
    gj = b["reference_joints"]
    batch = {"image": pk.inputs.synthetic_images(sum(views), seed=4).to(DEV), "target_cam_intr": b["img_metas"]["cam_intr"].to(DEV),
             "target_cam_extr": b["img_metas"]["cam_extr"].to(DEV), "master_id": [0] * len(views), "cam_view_num": np.asarray(views),
             "master_joints_3d": gj, "master_verts_3d": gj[:, 9:10] + 0.05 * torch.randn(2, 778, 3, generator=g),
             "target_joints_2d": 256.0 * torch.rand(sum(views), 21, 2, generator=g)}          # (CPU tensors of the collation: moved by PoemLoss)
    pyr = plain.extract_img_feat(batch["image"])            # one pyramid for both (MIOpen may pick other solvers on a later call)
    plain.extract_img_feat = model.extract_img_feat = lambda x: pyr
    p0, p1 = plain(batch, 0, mode="test"), model(batch, 0, mode="test")
    assert set(p0) == set(p1)
    for k in p0:
        if torch.is_tensor(p0[k]):
            assert torch.equal(p0[k], p1[k]), k
    with pytest.raises(RuntimeError, match="LOSS"):
        plain.compute_loss(p0, batch)
    with pytest.raises(ValueError):
        model(batch, 0, mode="train")
    with pytest.raises(RuntimeError, match="licence-gated"):
        model.compute_loss(p1, batch)
    model.set_j_regressor(jreg)
    loss, d = model.compute_loss(p1, batch)
    model.loss_metric.feed(d, len(views))
    inp = dict(coords=p1["all_coords_preds"][-1].cpu().numpy(), pred_uv=p1["pred_joints_uv"].cpu().numpy(), gt_joints=gj.numpy(),
               gt_verts=batch["master_verts_3d"].numpy(), gt_uv=batch["target_joints_2d"].numpy(), K=b["img_metas"]["cam_intr"].numpy(),
               E=b["img_metas"]["cam_extr"].numpy())
    want = restate(inp, views, loss_node, False, 9, 256, 256, jreg)
    assert list(d) == list(want) and loss is d["loss"]
    for k in want:
        assert abs(float(d[k]) - want[k]) <= 1e-9 * abs(want[k]), (k, float(d[k]), want[k])
    assert model.loss_metric.count == 2 and model.loss_metric.get_loss("loss") == float(loss)
