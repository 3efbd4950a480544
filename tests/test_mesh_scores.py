"""Benchmark-protocol mesh scores (csrc/meshscore.hip, poem_v2_amd.metrics, scripts/eval_single.py --benchmark-scores) against
the two yardsticks of tests/mesh_scores_util.py: (a) the fp32 numpy restatement of the search, which the kernel must match bit
for bit, and (b) the fp64 scores on a k-d tree with the fp64 SVD alignment.

    nn_distance_kernel     (na, nb) of NN_SHAPES -- 1, around 64, both sides of the 256-point query chunk and of the    test_nn_shapes
    + nn_finalize_kernel   1024-point LDS chunk, 778, 799 x 4096 -- x B 1/3/5: dist bit-equal, counts equal, sums 1e-12
                           threshold 2^-7 met exactly / one place below; duplicates, identical sets                    test_nn_strict..., test_nn_dup...
                           one NaN point on either side, an all-NaN set                                                test_nn_nan_rule
                           B = 5 against five calls; each output NULL in turn                                          test_nn_batch..., test_nn_optional...
    pa_align_kernel        P 3/4/21/63/64/65/778 x B 1/4/5/9 against the fp64 alignment, transform, poem_pa_epe        test_pa_align_shapes
    MeshFScore             sigma 2 / 5 / 10 mm against (b); 4 + 2 feeds; reduce on a one-rank group                    test_mesh_fscore_*
                           pred = s R gt + t                                                                           test_similarity_invariance
    PAJoint3DPCK / Vert    against Joint3DPCK / Vert3DPCK fed procrustes_align's output                               test_pa_pck_classes
    eval_single            evaluate / evaluate_shards with and without the flag                                        test_eval_single_benchmark_block

The CPU tests hold (a) to (b), re-measure the figures recorded in the util file and check every refusal of the C ABI."""
import ctypes
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mesh_scores_util as ms
import metric_forms_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 777.0
E_ARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
THR = ms.THRESHOLDS


def _hip():
    from poem_v2_amd import hip
    return hip, hip.lib()


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _eval_single():
    spec = importlib.util.spec_from_file_location("eval_single_mesh_scores", os.path.join(ROOT, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    return es


# =====================================================================================================================
# CPU: the yardsticks, the recorded figures, the inputs
def test_fp32_search_against_the_kdtree():
    """(a) against (b): the fp32 restatement is the k-d tree's distances up to fp32 rounding -- and the recorded gap is the measured one"""
    gap_abs = gap_rel = 0.0
    for a, b in (ms.nn_case(2, 778, 778, 1), ms.nn_case(1, 799, 4096, 2), ms.fscore_case()):
        for x, y in zip(a, b):
            for d32, d64 in zip(ms.nn_ref32(x, y), ms.nn_ref64(x, y)):
                assert d32.dtype == np.float32 and d64.dtype == np.float64
                g = np.abs(d32.astype(np.float64) - d64)
                gap_abs, gap_rel = max(gap_abs, float(g.max())), max(gap_rel, float((g / d64).max()))
    print(f"fp32 search against the k-d tree: {gap_abs:.2e} m, {gap_rel:.2e} relative")
    assert ms.NN_GAP_ABS_MEASURED / 2 <= gap_abs <= ms.NN_GAP_ABS_MEASURED
    assert ms.NN_GAP_REL_MEASURED / 2 <= gap_rel <= ms.NN_GAP_REL_MEASURED
    assert gap_rel < 4 * ms.EPS32                                    # what fscore_delta allows the search


def test_scores_of_the_yardsticks():
    pred, gt = (a[0] for a in ms.fscore_case())
    same = ms.scores64(gt, gt)
    assert np.all(same["d_p"] == 0) and np.array_equal(same["F"], [1.0, 1.0]) and np.array_equal(same["P"], [1.0, 1.0])
    d_ab, d_ba = ms.nn_ref32(gt, gt)
    assert np.all(d_ab == 0) and np.all(d_ba == 0)
    # swapping the arguments swaps precision and recall (300 points against 778: the two differ)
    fwd, rev = ms.scores64(pred[:300], gt), ms.scores64(gt, pred[:300])
    assert np.array_equal(fwd["P"], rev["R"]) and np.array_equal(fwd["R"], rev["P"]) and np.array_equal(fwd["F"], rev["F"])
    assert not np.array_equal(fwd["P"], fwd["R"])
    a32, b32 = ms.nn_ref32(pred[:300], gt), ms.nn_ref32(gt, pred[:300])
    assert np.array_equal(a32[0], b32[1]) and np.array_equal(a32[1], b32[0])
    # P + R = 0: every point farther than the largest threshold -> F = 0, not NaN
    far = ms.scores64(gt + np.float32(1.0), gt)
    assert np.array_equal(far["P"], [0.0, 0.0]) and np.array_equal(far["R"], [0.0, 0.0]) and np.array_equal(far["F"], [0.0, 0.0])
    assert np.array_equal(ms.prf([0, 3], [0, 1], 4, 2)[2], [0.0, 2 * 0.75 * 0.5 / 1.25])
    # strict `<`: a distance on the threshold is not counted, in (a)'s counts and in (b)'s
    on = np.array([[0.0, 0.0, 2.0 ** -7]], dtype=np.float32)
    d = ms.nn_ref32(on, np.zeros((1, 3), dtype=np.float32))[0]
    assert d[0] == 2.0 ** -7 and ms.counts_ref(d, [2.0 ** -7]).tolist() == [0]
    assert ms.scores64(on, np.zeros((1, 3)), thresholds=[2.0 ** -7])["P"].tolist() == [0.0]


def test_nan_rule_of_the_yardstick():
    a, b = (x[0].copy() for x in ms.nn_case(1, 70, 80, 3))
    base = ms.nn_ref32(a, b)
    a[5, 1] = np.nan
    d_ab, d_ba = ms.nn_ref32(a, b)
    keep = np.arange(70) != 5
    assert np.isnan(d_ab[5]) and np.array_equal(d_ab[keep], base[0][keep])
    assert np.array_equal(d_ba, ms.nn_ref32(a[keep], b)[1]) and not np.isnan(d_ba).any()          # as if the point were not there
    d_ab, d_ba = ms.nn_ref32(np.full_like(a, np.nan), b)
    assert np.isnan(d_ab).all() and np.isnan(d_ba).all() and ms.counts_ref(d_ba, THR).tolist() == [0, 0]


def _align_samples():
    for P, B, pred, gt in ms.align_cases():
        for b in range(B):
            yield P, B, b, pred[b], gt[b]


def test_align_noise_is_the_recorded_one():
    worst, kept, dropped = 0.0, 0, 0
    for P, B, b, pred, gt in _align_samples():
        if ms.align64(pred, gt)[1] >= ms.PA_MIN_RATIO:
            worst, kept = max(worst, ms.align_noise(pred, gt)), kept + 1
        else:
            dropped += 1
    for pred, gt in (ms.fscore_case(), ms.similarity_case()):
        for p, g in zip(pred, gt):
            assert ms.align64(p, g)[1] >= ms.PA_MIN_RATIO
            worst = max(worst, ms.align_noise(p, g))
    print(f"fp64 alignment's own noise per coordinate: {worst:.2e} m over {kept} samples ({dropped} below the ratio)")
    assert ms.ALIGN_NOISE_MEASURED / 2 <= worst <= ms.ALIGN_NOISE_MEASURED and ms.ALIGN_NOISE == 4 * ms.ALIGN_NOISE_MEASURED
    assert kept >= 100 and all(any(ms.align64(p, g)[1] >= ms.PA_MIN_RATIO for P_, _, _, p, g in _align_samples() if P_ == P)
                               for P in ms.PA_POINTS if P > 3)      # three points are flat: pinned through poem_pa_epe


def test_fscore_inputs_are_what_they_claim():
    pred, gt = ms.fscore_case()
    assert pred.shape == gt.shape == (6, 778, 3) and pred.dtype == np.float32
    assert np.all(np.linalg.norm(gt.astype(np.float64) - np.array([0.1, -0.2, 0.2]), axis=-1) <= 0.1 + 1e-6)
    assert max(np.abs(pred).max(), np.abs(gt).max()) <= ms.FSCORE_MAX_COORD
    delta = ms.fscore_delta(max(THR))
    print(f"delta of the aligned bracket: {delta:.3e} m")
    assert 0.98 * ms.FSCORE_DELTA_MEASURED <= delta <= ms.FSCORE_DELTA_MEASURED
    near_worst, f5 = 0, []
    for b in range(6):
        for aligned in (False, True):
            s = ms.scores64(pred[b], gt[b], aligned=aligned)
            f5.append(float(s["F"][0]))
            assert 0.05 < s["F"][0] < 0.95, (b, aligned, s["F"])                  # the case can fail
            for d in (s["d_p"], s["d_g"]):
                for t in THR:
                    near_worst = max(near_worst, int((np.abs(d - t) <= ms.fscore_delta(t)).sum()))
        # raw: (a)'s counts are (b)'s -- no distance within the fp32 gap of a threshold
        s, d32 = ms.scores64(pred[b], gt[b]), ms.nn_ref32(pred[b], gt[b])
        assert np.array_equal(ms.prf(ms.counts_ref(d32[0], THR), ms.counts_ref(d32[1], THR), 778, 778)[2], s["F"])
    print(f"F@5 on the yardstick: {min(f5):.3f} .. {max(f5):.3f}; distances within delta of a threshold: {near_worst}")
    assert near_worst <= ms.FSCORE_NEAR_MAX                                        # the bracket may not hide a failure
    assert max(f5) > 0.85 and min(f5) < 0.15


# =====================================================================================================================
# CPU: the binding, the refusals, the command line
def test_signature_table_carries_the_new_exports():
    hip, L = _hip()
    for name in ("poem_pa_align", "poem_nn_distance", "poem_nn_distance_workspace_bytes"):
        assert name in hip.SIGNATURES and hasattr(L, name)
    assert L.poem_abi_version() == hip.ABI_VERSION == 3                            # symbols are only added
    import poem_v2_amd as pk
    for name in ("MeshFScore", "PAJoint3DPCK", "PAVert3DPCK", "procrustes_align", "nearest_distances"):
        assert getattr(pk, name) is getattr(pk.metrics, name)


def test_refusals_need_no_device():
    """every argument refusal comes from the .so before any launch: the pointers are host buffers nothing may read"""
    hip, L = _hip()
    buf = (ctypes.c_double * 64)()
    x = ctypes.addressof(buf)
    thr = (ctypes.c_double * 8)(0.005, 0.015, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07)
    big = 1 << 40

    def nn(a=x, na=4, b=x, nb=4, dab=x, dba=x, t=thr, nthr=2, counts=x, sums=x, ws=x, wsb=big, batch=1):
        return L.poem_nn_distance(a, na, b, nb, dab, dba, t, nthr, counts, sums, ws, wsb, batch, None)

    assert nn(a=None) == E_ARG and nn(b=None) == E_ARG
    assert nn(na=0) == E_ARG and nn(nb=-1) == E_ARG and nn(batch=0) == E_ARG and nn(nthr=-1) == E_ARG
    assert nn(dab=None, dba=None, counts=None, sums=None) == E_ARG
    assert nn(t=None) == E_ARG and nn(nthr=0) == E_ARG                              # counts without thresholds
    for bad in ((float("nan"), 0.01), (-0.001, 0.01), (0.01, 0.005), (0.01, 0.01)):
        assert nn(t=(ctypes.c_double * 2)(*bad)) == E_ARG, bad
    assert nn(na=(1 << 24) + 1) == E_UNSUPPORTED and nn(nb=(1 << 24) + 1) == E_UNSUPPORTED
    assert nn(nthr=9, t=(ctypes.c_double * 9)(*[0.001 * (i + 1) for i in range(9)])) == E_UNSUPPORTED
    need = L.poem_nn_distance_workspace_bytes(3, 778, 300, 2)
    assert need == 3 * (4 + 2) * (8 + 2 * 4) and need % 8 == 0
    assert L.poem_nn_distance_workspace_bytes(1, 256, 257, 1) == ((1 + 2) * 12 + 7) // 8 * 8
    assert nn(na=778, nb=300, batch=3, wsb=need - 1) == E_WORKSPACE and nn(ws=None) == E_WORKSPACE
    assert nn(na=778, nb=300, batch=3, counts=None, wsb=L.poem_nn_distance_workspace_bytes(3, 778, 300, 0) - 1) == E_WORKSPACE
    for args in ((0, 4, 4, 2), (1, 0, 4, 2), (1, 4, 0, 2), (1, 4, 4, 9), (1, 4, 4, -1), (1, (1 << 24) + 1, 4, 2)):
        assert L.poem_nn_distance_workspace_bytes(*args) == 0, args
    assert L.poem_pa_align(None, x, x, x, 1, 21, None) == E_ARG and L.poem_pa_align(x, None, x, x, 1, 21, None) == E_ARG
    assert L.poem_pa_align(x, x, None, None, 1, 21, None) == E_ARG                  # aligned or transform may be NULL, not both
    assert L.poem_pa_align(x, x, x, x, 0, 21, None) == E_ARG and L.poem_pa_align(x, x, x, x, 1, 2, None) == E_ARG
    # the Python surface: no CPU path
    from poem_v2_amd.metrics import MeshFScore, PAJoint3DPCK, nearest_distances, procrustes_align
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        procrustes_align(torch.zeros(1, 21, 3), torch.zeros(1, 21, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nearest_distances(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MeshFScore(device="cpu").feed(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PAJoint3DPCK(device="cpu", VAL_MIN=0.0, VAL_MAX=0.05, STEPS=100).feed({"pred_joints_3d": torch.zeros(1, 21, 3)},
                                                                             {"master_joints_3d": torch.zeros(1, 21, 3)})
    with pytest.raises(ValueError):
        MeshFScore(thresholds=(0.015, 0.005), device="cpu")
    with pytest.raises(ValueError, match="Unknown eval_type"):
        PAJoint3DPCK(device="cpu", VAL_MIN=0.0, VAL_MAX=0.05, STEPS=100, EVAL_TYPE="verts_3d")


def test_mesh_fscore_measure_keys():
    from poem_v2_amd.metrics import MeshFScore
    m = MeshFScore(device="cpu")                                                   # (construction and the empty read-out need no GPU)
    want = {f"{mode}{k}" for mode in ("", "PA_") for k in ("F@5", "F@15", "precision@5", "precision@15", "recall@5", "recall@15",
                                                             "chamfer_pred2gt", "chamfer_gt2pred")}
    assert set(m.get_measures()) == want and m.count == 0 and all(v == 0.0 for v in m.get_measures().values())
    assert set(MeshFScore(thresholds=(0.0025,), aligned=False, device="cpu").get_measures()) == {
        "F@2.5", "precision@2.5", "recall@2.5", "chamfer_pred2gt", "chamfer_gt2pred"}
    assert str(m).startswith("F@5: 0.0000 | F@15: 0.0000 | PA_F@5")


def test_eval_single_flag_and_plumbing(monkeypatch, tmp_path):
    es = _eval_single()
    base = ["--cfg", str(tmp_path / "c.yaml"), "--dataset", "HO3D", "--view_min", "2", "--view_max", "3", "--model", "small", "-g", "0"]
    assert es.build_cli().parse_args(base + ["--benchmark-scores"]).benchmark_scores is True
    assert "benchmark_scores" not in vars(es.build_cli().parse_args(base))          # absent unless given
    assert "benchmark_scores" not in vars(es.build_parser().parse_args(base + ["--shards", "d"]))
    seen = []
    monkeypatch.setattr(es, "evaluate", lambda *a, **k: (seen.append(("evaluate", k)), {})[1])
    monkeypatch.setattr(es, "evaluate_shards", lambda *a, **k: (seen.append(("shards", k)), {})[1])
    monkeypatch.setattr(es.pdist, "init_from_env", lambda *a, **k: (0, 0, 1))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    es.main(es.build_parser().parse_args(base))                                     # a namespace that never heard of the flag
    es.main(types.SimpleNamespace(**vars(es.build_parser().parse_args(base + ["--shards", str(tmp_path)]))))
    es.main(es.build_cli().parse_args(base + ["--benchmark-scores"]))
    es.main(es.build_cli().parse_args(base + ["--benchmark-scores", "--shards", str(tmp_path)]))
    assert [(w, k["benchmark_scores"]) for w, k in seen] == [("evaluate", False), ("shards", False), ("evaluate", True), ("shards", True)]


# =====================================================================================================================
# GPU: poem_nn_distance
def _nn(a, b, thr=THR, want=("ab", "ba", "counts", "sums")):
    """poem_nn_distance through the C ABI on (B,na,3), (B,nb,3) arrays: dict of the outputs asked for, as numpy.  Every output
    buffer is filled with a guard value and carries eight guard elements behind its end."""
    hip, L = _hip()
    ad, bd = _dev(a), _dev(b)
    B, na, nb, T = ad.shape[0], ad.shape[1], bd.shape[1], len(thr)
    sizes = {"ab": (B * na, torch.float32), "ba": (B * nb, torch.float32), "counts": (B * 2 * T, torch.int32), "sums": (B * 2, torch.float64)}
    bufs = {k: torch.full((sizes[k][0] + 8,), GUARD, dtype=sizes[k][1], device=DEV) for k in want}
    need = L.poem_nn_distance_workspace_bytes(B, na, nb, T if "counts" in want else 0)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
    ws.fill_(0x5A)
    tarr = (ctypes.c_double * max(T, 1))(*thr)
    p = {k: (bufs[k].data_ptr() if k in bufs else None) for k in sizes}
    rc = L.poem_nn_distance(hip.ptr(ad), na, hip.ptr(bd), nb, p["ab"], p["ba"], tarr, T, p["counts"], p["sums"], ws.data_ptr(), need, B,
                            hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "written past the workspace"
    out = {}
    for k, t in bufs.items():
        assert bool((t[-8:] == GUARD).all()), f"{k}: written past its end"
        out[k] = t[:-8].cpu().numpy()
    shapes = {"ab": (B, na), "ba": (B, nb), "counts": (B, 2, T), "sums": (B, 2)}
    return {k: v.reshape(shapes[k]) for k, v in out.items()}


def _same_bits(got, want):
    return got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _check_nn(got, a, b, thr=THR):
    d_ab, d_ba = ms.nn_ref32_batch(a, b)
    if "ab" in got:
        assert _same_bits(got["ab"], d_ab), np.abs(got["ab"] - d_ab).max()
    if "ba" in got:
        assert _same_bits(got["ba"], d_ba), np.abs(got["ba"] - d_ba).max()
    if "counts" in got:
        want = np.stack([ms.counts_ref(d_ab, thr), ms.counts_ref(d_ba, thr)], 1)
        assert np.array_equal(got["counts"], want), (got["counts"], want)
    if "sums" in got:
        want = np.stack([d_ab.astype(np.float64).sum(1), d_ba.astype(np.float64).sum(1)], 1)
        nan = np.isnan(want)                                             # sums carries a NaN distance
        assert np.array_equal(np.isnan(got["sums"]), nan), (got["sums"], want)
        assert np.all(np.abs(got["sums"] - want)[~nan] <= 1e-12 * np.abs(want)[~nan]), (got["sums"], want)      # the order of summation only


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb", ms.NN_SHAPES)
def test_nn_shapes(na, nb):
    for B in ms.NN_BATCHES:
        a, b = ms.nn_case(B, na, nb, 7 * na + nb + B)
        # thresholds that cut through the distances: the noisy copies lie a few millimetres off, the rest centimetres
        _check_nn(_nn(a, b, thr=(0.004, 0.005, 0.015, 0.04)), a, b, thr=(0.004, 0.005, 0.015, 0.04))


@pytest.mark.gpu
def test_nn_strictness_on_the_threshold():
    """threshold 2^-7 m: a point at exactly that distance is not counted, the fp32 value one place below is"""
    t = np.float32(2.0 ** -7)
    below = np.nextafter(t, np.float32(0))
    a = np.zeros((1, 70, 3), dtype=np.float32)
    a[0, :, 0] = np.arange(70, dtype=np.float32)                         # 70 points a metre apart, each with its own partner
    b = a.copy()
    b[0, :35, 1] = t
    b[0, 35:, 2] = -below
    got = _nn(a, b, thr=(float(t),))
    assert np.array_equal(got["ab"][0, :35], np.full(35, t)) and np.array_equal(got["ab"][0, 35:], np.full(35, below))
    assert got["counts"].tolist() == [[[35], [35]]]
    _check_nn(got, a, b, thr=(float(t),))
    assert _nn(a, b, thr=(float(below),))["counts"].tolist() == [[[0], [0]]]
    assert _nn(a, b, thr=(float(np.nextafter(t, np.float32(1))),))["counts"].tolist() == [[[70], [70]]]


@pytest.mark.gpu
def test_nn_duplicates_and_identical_sets():
    a, _ = ms.nn_case(2, 300, 300, 5)
    got = _nn(a, a.copy())
    assert not got["ab"].any() and not got["ba"].any() and np.all(got["counts"] == 300) and not got["sums"].any()
    a[:, 100:200] = a[:, :100]                                           # duplicates inside a set
    b = np.concatenate([a[:, :100], a[:, :100], a[:, 200:]], 1)[:, ::-1].copy()
    got = _nn(a, b)
    assert not got["ab"].any() and not got["ba"].any()
    _check_nn(got, a, b)


@pytest.mark.gpu
def test_nn_nan_rule():
    a, b = ms.nn_case(3, 300, 1100, 9)
    base = _nn(a, b)
    an, bn = a.copy(), b.copy()
    an[1, 257, 2] = np.nan                                               # sample 1: one NaN point in a (second query chunk)
    bn[2, 1050, 0] = np.nan                                              # sample 2: one in b (second LDS chunk)
    got = _nn(an, bn)
    _check_nn(got, an, bn)
    assert np.isnan(got["ab"][1, 257]) and np.isnan(got["ba"][2, 1050]) and np.isnan(got["ab"]).sum() == 1 and np.isnan(got["ba"]).sum() == 1
    assert np.isnan(got["sums"][1, 0]) and np.isnan(got["sums"][2, 1]) and np.isnan(got["sums"]).sum() == 2
    for k in ("ab", "ba", "counts", "sums"):                             # sample 0 is untouched
        assert np.array_equal(got[k][0], base[k][0])
    # the NaN point is as if it were not there for everybody else
    rest = _nn(np.delete(an[1:2], 257, axis=1), bn[1:2])
    assert _same_bits(got["ba"][1:2], rest["ba"]) and _same_bits(np.delete(got["ab"][1:2], 257, axis=1), rest["ab"])
    assert np.array_equal(got["counts"][1:2], rest["counts"])
    # an all-NaN set: NaN distances and zero counts in both directions
    got = _nn(a[:1], np.full_like(b[:1], np.nan))
    assert np.isnan(got["ab"]).all() and np.isnan(got["ba"]).all() and not got["counts"].any() and np.isnan(got["sums"]).all()
    _check_nn(got, a[:1], np.full_like(b[:1], np.nan))


@pytest.mark.gpu
def test_nn_batch_independence():
    a, b = ms.nn_case(5, 778, 799, 13)
    whole = _nn(a, b)
    for i in range(5):
        one = _nn(a[i:i + 1], b[i:i + 1])
        assert _same_bits(one["ab"], whole["ab"][i:i + 1]) and _same_bits(one["ba"], whole["ba"][i:i + 1])
        assert np.array_equal(one["counts"], whole["counts"][i:i + 1])
        assert np.array_equal(one["sums"].view(np.uint64), whole["sums"][i:i + 1].view(np.uint64))


@pytest.mark.gpu
def test_nn_optional_outputs():
    a, b = ms.nn_case(3, 513, 300, 17)
    full = _nn(a, b)
    _check_nn(full, a, b)
    for drop in ("ab", "ba", "counts", "sums"):
        got = _nn(a, b, want=tuple(k for k in ("ab", "ba", "counts", "sums") if k != drop))
        assert drop not in got
        for k, v in got.items():
            assert np.array_equal(v.view(np.uint8), full[k].view(np.uint8)), (drop, k)
    for only in ("ab", "ba", "counts", "sums"):
        got = _nn(a, b, want=(only,))
        assert np.array_equal(got[only].view(np.uint8), full[only].view(np.uint8)), only
    # the Python wrapper
    from poem_v2_amd.metrics import nearest_distances
    d_ab, d_ba = nearest_distances(_dev(a), _dev(b))
    assert _same_bits(d_ab.cpu().numpy(), full["ab"]) and _same_bits(d_ba.cpu().numpy(), full["ba"])


# =====================================================================================================================
# GPU: poem_pa_align
def _pa_align(pred, gt, want=("aligned", "transform")):
    hip, L = _hip()
    pd, gd = _dev(pred), _dev(gt)
    B, P = pd.shape[0], pd.shape[1]
    al = torch.full((B * P * 3 + 8,), GUARD, dtype=torch.float32, device=DEV) if "aligned" in want else None
    tr = torch.full((B * 13 + 8,), GUARD, dtype=torch.float64, device=DEV) if "transform" in want else None
    rc = L.poem_pa_align(hip.ptr(pd), hip.ptr(gd), None if al is None else al.data_ptr(), None if tr is None else tr.data_ptr(), B, P,
                         hip.stream())
    assert rc == 0, rc
    epe = torch.empty(B, 2, dtype=torch.float32, device=DEV)
    assert L.poem_pa_epe(hip.ptr(pd), hip.ptr(gd), hip.ptr(epe), B, P, hip.stream()) == 0
    torch.cuda.synchronize()
    out = {"epe": epe.cpu().numpy()}
    if al is not None:
        assert bool((al[-8:] == GUARD).all())
        out["aligned"] = al[:-8].cpu().numpy().reshape(B, P, 3)
    if tr is not None:
        assert bool((tr[-8:] == GUARD).all())
        out["transform"] = tr[:-8].cpu().numpy().reshape(B, 13)
    return out


def _apply(transform, pred):
    """c R p + t in fp64 for one sample"""
    c, R, t = transform[0], transform[1:10].reshape(3, 3), transform[10:13]
    return c * np.asarray(pred, dtype=np.float64).dot(R.T) + t


@pytest.mark.gpu
@pytest.mark.parametrize("P", ms.PA_POINTS)
def test_pa_align_shapes(P):
    """aligned and transform against the fp64 alignment at align_tol; poem_pa_epe's first output against the mean distance of the
    aligned set to gt at pa_tol.  The latter is held on the fp64 points c R p + t that `aligned` is the fp32 rounding of (worst case
    measured: 0.38 of pa_tol).  The fp32 tensor itself cannot meet pa_tol, whatever the kernel does: pa_tol is a few 1e-9 m, while
    rounding a 0.6 m coordinate to fp32 moves it by up to 3e-8 m, which a mean over 3 or 4 points does not average out -- measured
    8.2 (P = 3), 10.2 (P = 4), 0.96 (21), 0.71 (63), 1.01 (64), 0.74 (65), 0.42 (778) times pa_tol.  It is held to pa_tol plus that
    rounding, sqrt(3) EPS32 / 2 of the largest coordinate."""
    worst = worst_epe = worst_epe32 = 0.0
    for P_, B, pred, gt in ms.align_cases():
        if P_ != P:
            continue
        got = _pa_align(pred, gt)
        only_al, only_tr = _pa_align(pred, gt, want=("aligned",)), _pa_align(pred, gt, want=("transform",))
        assert _same_bits(only_al["aligned"], got["aligned"]) and np.array_equal(only_tr["transform"], got["transform"])
        for b in range(B):
            ref, ratio = ms.align64(pred[b], gt[b])
            mine = _apply(got["transform"][b], pred[b])
            R = got["transform"][b, 1:10].reshape(3, 3)
            assert np.abs(R.dot(R.T) - np.eye(3)).max() < 1e-12 and got["transform"][b, 0] > 0
            # the fp32 output is the rounding of the fp64 point the transform describes
            assert np.all(np.abs(got["aligned"][b].astype(np.float64) - mine) <= ms.align_tol(mine)), (P, B, b)
            # poem_pa_epe measures the same fp64 points: its first output is their mean distance to gt
            mean = float(np.mean(np.linalg.norm(mine - gt[b].astype(np.float64), axis=1)))
            worst_epe = max(worst_epe, abs(float(got["epe"][b, 0]) - mean) / mu.pa_tol(mean))
            mean32 = float(np.mean(np.linalg.norm(got["aligned"][b].astype(np.float64) - gt[b].astype(np.float64), axis=1)))
            worst_epe32 = max(worst_epe32, abs(float(got["epe"][b, 0]) - mean32) / mu.pa_tol(mean32))
            # ... and of the fp32 output, once the rounding of that output is allowed for: half a place per coordinate
            assert abs(float(got["epe"][b, 0]) - mean32) <= mu.pa_tol(mean32) + np.sqrt(3.0) * ms.EPS32 / 2 * np.abs(mine).max()
            assert abs(float(got["epe"][b, 0]) - mean) <= mu.pa_tol(mean), (P, B, b, got["epe"][b, 0], mean)
            if ratio >= ms.PA_MIN_RATIO:
                err = np.abs(got["aligned"][b].astype(np.float64) - ref)
                worst = max(worst, float((err / ms.align_tol(ref)).max()))
                assert np.all(err <= ms.align_tol(ref)), (P, B, b, err.max())
                assert np.all(np.abs(mine - ref) <= ms.align_tol(ref)), (P, B, b)
    print(f"P = {P}: aligned against fp64 at {worst:.3f} of the bar, poem_pa_epe against the aligned set at {worst_epe:.3f} of pa_tol "
          f"(against its fp32 rounding: {worst_epe32:.3f})")
    # a sample alone is the sample inside a batch, bit for bit
    P_, B, pred, gt = [c for c in ms.align_cases() if c[0] == P and c[1] == 9][0]
    whole, one = _pa_align(pred, gt), _pa_align(pred[6:7], gt[6:7])
    assert _same_bits(one["aligned"], whole["aligned"][6:7]) and np.array_equal(one["transform"], whole["transform"][6:7])
    from poem_v2_amd.metrics import procrustes_align
    al, tr = procrustes_align(_dev(pred), _dev(gt), return_transform=True)
    assert _same_bits(al.cpu().numpy(), whole["aligned"]) and np.array_equal(tr.cpu().numpy(), whole["transform"])
    assert _same_bits(procrustes_align(_dev(pred), _dev(gt)).cpu().numpy(), whole["aligned"])


# =====================================================================================================================
# GPU: MeshFScore
@pytest.fixture(scope="module")
def fscore_reference():
    """the F-score batch and yardstick (b) on it, computed once: {"pred", "gt", "raw": [scores64 per sample], "pa": [...]}"""
    pred, gt = ms.fscore_case()
    return {"pred": pred, "gt": gt, "raw": [ms.scores64(p, g) for p, g in zip(pred, gt)],
            "pa": [ms.scores64(p, g, aligned=True) for p, g in zip(pred, gt)]}


@pytest.mark.gpu
def test_mesh_fscore_against_the_kdtree(fscore_reference):
    from poem_v2_amd.metrics import MeshFScore, procrustes_align
    pred, gt, raw, pa = (fscore_reference[k] for k in ("pred", "gt", "raw", "pa"))
    m = MeshFScore(device=DEV)
    F = m.feed(_dev(pred), _dev(gt))
    assert F.is_cuda and F.dtype == torch.float64 and tuple(F.shape) == (6, 2, 2) and m.count == 6
    F = F.cpu().numpy()
    for b in range(6):
        assert 0.05 < raw[b]["F"][0] < 0.95
        assert np.array_equal(F[b, 0], raw[b]["F"]), (b, F[b, 0], raw[b]["F"])         # equal counts: the same fp64 expression
    # aligned: the counts behind F are bracketed by (b)'s distances
    got = _nn(procrustes_align(_dev(pred), _dev(gt)).cpu().numpy(), gt)
    for b in range(6):
        for di, d in enumerate((pa[b]["d_p"], pa[b]["d_g"])):
            for ti, t in enumerate(THR):
                delta = ms.fscore_delta(t)
                lo, hi = int((d < t - delta).sum()), int((d < t + delta).sum())
                assert hi - lo <= ms.FSCORE_NEAR_MAX and lo <= got["counts"][b, di, ti] <= hi, (b, di, ti, lo, got["counts"][b, di, ti], hi)
        p, r, f = ms.prf(got["counts"][b, 0], got["counts"][b, 1], 778, 778)
        assert np.array_equal(F[b, 1], f), (b, F[b, 1], f)
    meas = m.get_measures()
    for mi, (mode, ref, Fm) in enumerate((("", raw, F[:, 0]), ("PA_", pa, F[:, 1]))):
        for ti, key in enumerate(("5", "15")):
            assert abs(meas[f"{mode}F@{key}"] - Fm[:, ti].mean()) <= 1e-14
        # the distances' means: fp32 distances summed in fp64 against (b)'s fp64 distances
        want_p, want_g = np.mean([s["d_p"].mean() for s in ref]), np.mean([s["d_g"].mean() for s in ref])
        bar = 4 * ms.EPS32 * max(want_p, want_g) + (0 if not mode else np.sqrt(3.0) * ms.align_tol(ms.FSCORE_MAX_COORD))
        assert abs(meas[f"{mode}chamfer_pred2gt"] - want_p) <= bar and abs(meas[f"{mode}chamfer_gt2pred"] - want_g) <= bar
    for ti, key in enumerate(("5", "15")):                              # raw precision / recall: (b)'s, counts being equal
        assert abs(meas[f"precision@{key}"] - np.mean([s["P"][ti] for s in raw])) <= 1e-14
        assert abs(meas[f"recall@{key}"] - np.mean([s["R"][ti] for s in raw])) <= 1e-14
    assert m.get_result() == meas["F@5"]


@pytest.mark.gpu
def test_mesh_fscore_feeds_add_up(fscore_reference):
    from poem_v2_amd.metrics import MeshFScore
    pred, gt = _dev(fscore_reference["pred"]), _dev(fscore_reference["gt"])
    one, two = MeshFScore(device=DEV), MeshFScore(device=DEV)
    F6 = one.feed(pred, gt)
    F42 = torch.cat([two.feed(pred[:4], gt[:4]), two.feed(pred[4:], gt[4:])])
    assert torch.equal(F6, F42) and one.count == two.count == 6          # a sample's score does not depend on its batch
    a, b = one.get_measures(), two.get_measures()
    assert a.keys() == b.keys() and all(abs(a[k] - b[k]) <= 1e-14 * abs(a[k]) for k in a)        # fp64 sums in another order
    two.reset()
    assert two.count == 0 and not two.acc.any() and two.get_measures()["F@5"] == 0.0
    raw_only = MeshFScore(aligned=False, device=DEV)
    assert torch.equal(raw_only.feed(pred, gt)[:, 0], F6[:, 0]) and "PA_F@5" not in raw_only.get_measures()
    # P + R = 0 on the device: F = 0
    far = MeshFScore(aligned=False, device=DEV)
    assert not far.feed(pred + 1.0, gt).any() and far.get_measures()["F@15"] == 0.0


_REDUCE_WORKER = r'''
import os, sys, torch
for p in ("", "oracle", "tests"):
    sys.path.insert(0, os.path.join(sys.argv[1], p))
import torch.distributed as dist
import mesh_scores_util as ms
from poem_v2_amd import dist as pdist
from poem_v2_amd.metrics import MeshFScore
rank, local, world = pdist.init_from_env()
assert (rank, local, world) == (0, 0, 1) and pdist.active() and dist.get_world_size() == 1
dev = torch.device("cuda", local)
pred, gt = (torch.from_numpy(a).to(dev) for a in ms.fscore_case())
m = MeshFScore(device=dev)
m.feed(pred[:4], gt[:4]); before = m.get_measures(); acc = m.acc.clone()
m.reduce(); m.reduce()
assert m._global is not None and m._global.is_cuda and m._global.dtype == torch.float64
assert m.get_measures() == before and torch.equal(m.acc, acc), "reduce() twice counted twice"
m.feed(pred[4:], gt[4:])                                         # a feed after reduce(): the local sums were never the reduced ones
assert m._global is None and m.count == 6
whole = MeshFScore(device=dev); whole.feed(pred[:4], gt[:4]); whole.feed(pred[4:], gt[4:])
assert torch.equal(m.acc, whole.acc) and m.reduce().get_measures() == whole.get_measures()
pdist.barrier(); pdist.shutdown()
print("MESH_REDUCE_OK")
'''


@pytest.mark.gpu
def test_mesh_fscore_reduce_on_a_one_rank_group(tmp_path):
    """reduce() twice and a feed after reduce() never double count -- over a real (RCCL) all-reduce, on a forced one-rank group as
    tests/test_dist_gpu.py builds it"""
    from poem_v2_amd import dist as pdist
    drop = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "POEM_SINGLE_DEVICE", "POEM_DIST_BACKEND", "POEM_DIST_FORCE_INIT", "MASTER_PORT", "MASTER_ADDR")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["POEM_DIST_FORCE_INIT"] = "1"
    script = tmp_path / "mesh_reduce_worker.py"
    script.write_text(_REDUCE_WORKER)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                          "--master-port", str(pdist.free_port()), str(script), ROOT], capture_output=True, text=True, env=env, timeout=600)
    err = "\n".join(ln for ln in out.stderr.splitlines() if "NCCL WARN" not in ln and ln.strip())[-3000:]
    assert out.returncode == 0 and "MESH_REDUCE_OK" in out.stdout, (out.stdout[-1500:], err)


@pytest.mark.gpu
def test_similarity_invariance():
    """pred = s R gt + t: the aligned F@5 and F@15 are exactly 1 and the aligned AUC is its maximum"""
    from poem_v2_amd.metrics import MeshFScore, PAVert3DPCK, Vert3DPCK
    pred, gt = (_dev(a) for a in ms.similarity_case())
    m = MeshFScore(device=DEV)
    F = m.feed(pred, gt).cpu().numpy()
    assert np.all(F[:, 1] == 1.0) and np.all(F[:, 0] < 0.5)              # aligned exactly 1, raw far from it
    meas = m.get_measures()
    assert meas["PA_F@5"] == 1.0 and meas["PA_F@15"] == 1.0 and meas["PA_precision@5"] == 1.0 and meas["PA_recall@5"] == 1.0
    assert meas["PA_chamfer_pred2gt"] < 1e-6 and meas["chamfer_pred2gt"] > 1e-3
    cfg = dict(VAL_MIN=0.0, VAL_MAX=0.05, STEPS=100)
    pck, plain = PAVert3DPCK(device=DEV, **cfg), Vert3DPCK(device=DEV, **cfg)
    pck.feed({"pred_verts_3d": pred}, {"master_verts_3d": gt})
    plain.feed({"pred_verts_3d": pred}, {"master_verts_3d": gt})
    # every distance lies under the first positive threshold: the curve is (c, 1, 1, ..., 1) with c = the share of exact zeros
    top = 1.0 - 0.5 / 99.0
    auc = pck.get_measures()["auc_all"]
    assert top - 1e-12 <= auc <= 1.0 and np.all(pck.get_measures()["pck_curve_per_kp"][:, 1:] == 1.0)
    assert plain.get_measures()["auc_all"] < 0.9


@pytest.mark.gpu
def test_pa_pck_classes():
    from poem_v2_amd.metrics import Joint3DPCK, PAJoint3DPCK, PAVert3DPCK, Vert3DPCK, procrustes_align
    cfg = dict(VAL_MIN=0.0, VAL_MAX=0.05, STEPS=100)
    for pa_cls, cls, n, kp, kt in ((PAJoint3DPCK, Joint3DPCK, 21, "pred_joints_3d", "master_joints_3d"),
                                   (PAVert3DPCK, Vert3DPCK, 778, "pred_verts_3d", "master_verts_3d")):
        assert issubclass(pa_cls, cls) and pa_cls._keys is cls._keys and pa_cls.num_kp == n
        a, b = pa_cls(device=DEV, **cfg), cls(device=DEV, **cfg)
        for B, seed in ((5, 1), (2, 2)):
            pred, gt = (_dev(x) for x in mu.pa_generic(n, 50 + seed, B))
            a.feed({kp: pred}, {kt: gt})
            b.feed({kp: procrustes_align(pred, gt)}, {kt: gt})
        assert torch.equal(a.counts, b.counts) and torch.equal(a.sum, b.sum) and torch.equal(a.n, b.n) and a.count == b.count == 7
        assert all(torch.equal(x, y) for x, y in zip(a.dists, b.dists))
        assert 0.0 < a.get_measures()["auc_all"] == b.get_measures()["auc_all"] < 1.0
        with pytest.raises(ValueError, match="Unknown eval_type"):
            pa_cls(device=DEV, EVAL_TYPE="nonsense", **cfg)
        rel = pa_cls(device=DEV, EVAL_TYPE=kp[5:] + "_rel", **cfg)                        # the other key pair still works
        rel.feed({kp + "_rel": pred}, {kt + "_rel": gt})
        assert rel.count == 2


# =====================================================================================================================
# GPU: scripts/eval_single.py
EVALUATE_KEYS = {"dataset_source", "scope", "model", "embed", "view_range", "samples", "MPVPE_mm_vs_synthetic_gt", "MPJPE_mm_vs_synthetic_gt",
                 "PA_MPJPE_mm", "PA_MPVPE_mm", "auc_j", "auc_v", "samples_per_s_rank0", "world_size", "template_source"}
SHARDS_KEYS = {"dataset_source", "scope", "model", "view_range", "samples", "MPVPE_mm_vs_record_gt", "MPJPE_mm_vs_record_gt",
               "samples_per_s_rank0", "world_size", "template_source"}
BENCHMARK_KEYS = {"F@5", "F@15", "PA_F@5", "PA_F@15", "pa_auc_j", "pa_auc_v", "chamfer_mm"}


def _check_block(res, keys):
    assert set(res) == keys | {"benchmark"}
    blk = res["benchmark"]
    assert set(blk) == BENCHMARK_KEYS
    for k in BENCHMARK_KEYS - {"chamfer_mm"}:
        assert np.isfinite(blk[k]) and 0.0 <= blk[k] <= 1.0, (k, blk[k])
    assert np.isfinite(blk["chamfer_mm"]) and blk["chamfer_mm"] > 0
    assert blk["PA_F@15"] >= blk["PA_F@5"] and blk["F@15"] >= blk["F@5"]


@pytest.mark.gpu
def test_eval_single_benchmark_block(tmp_path):
    es = _eval_single()
    device = torch.device(DEV)
    cfg = es.default_cfg()
    view_range = es.edit_cfg(cfg, "DexYCB", "small", [2, 4])
    with_flag = es.evaluate(cfg, view_range, "small", device, epoch_size=6, batch_size=2, verbose=False, benchmark_scores=True)
    _check_block(with_flag, EVALUATE_KEYS)
    assert with_flag["samples"] == 6
    plain = es.evaluate(cfg, view_range, "small", device, epoch_size=6, batch_size=2, verbose=False)
    assert set(plain) == EVALUATE_KEYS                                   # without the flag: today's keys
    assert all(plain[k] == with_flag[k] for k in EVALUATE_KEYS - {"samples_per_s_rank0"})
    shards = dict(shard_dir=str(tmp_path / "shards"), dataset="DexYCB", epoch_size=4, batch_size=2, backbone="resnet18", backbone_engine="hip")
    with_flag = es.evaluate_shards(cfg, view_range, "small", device, benchmark_scores=True, **shards)
    _check_block(with_flag, SHARDS_KEYS)
    plain = es.evaluate_shards(cfg, view_range, "small", device, **shards)
    assert set(plain) == SHARDS_KEYS and plain["samples"] == with_flag["samples"] == 4      # (the views of a sample are drawn anew)
