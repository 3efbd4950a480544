"""Outlier-robust triangulation of the reference joints (``poem_dlt_robust``, ``mode="ransac"``).  Upstream has nothing to compare
with, so the yardstick is the fp64 restatement in tests/dlt_robust_util.py, written from the definition in include/poem_hip.h.

Inputs (dlt_robust_util.make_case): the synthetic batch's cameras and joints, uv = exact projection + 0.5 px noise in fp32, outlier
views displaced by 40 px.  An outlier is planted only where at least three clean views remain: with 3 views and one outlier every
pair explains itself, the counts tie at 2 and the tie-break does not identify the outlier -- that case is kept as a determinism
test against the restatement's own choice.

Bars.  5e-6 m for joints: the bar tests/test_dlt.py holds the plain solve to against an fp64 SVD on this rig (fp32 M = K.T on the
device against fp64).  5e-3 px for residuals: that bar seen through f / z = 300 / 0.6, times 2.  Masks, counts and everything said to
be "the same" are equality of bits.  The masks can be held to equality because the CPU test asserts that no final residual of the
input set lies within 1 px of the threshold (measured: 6.1 px), which an fp32 / fp64 difference of 5e-3 px cannot cross; in the
three-view case, where the winning pair decides the mask, the same is asserted of every hypothesis."""
import ctypes
import functools
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import dlt_robust_util as ru
from util import ROOT

DEV = "cuda:0"
BAR, BAR_PX, PX = 5e-6, 5e-3, 8.0
RAGGED, RAGGED_OUT = [2, 3, 4, 5, 8, 11], [0, 0, 1, 1, 1, 3]
ONE_OUTLIER = (2, 3, 4)                                        # the samples of RAGGED with exactly one outlier


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "ragged":
        return ru.make_case(RAGGED, RAGGED_OUT, 0)
    if name == "clean":
        return ru.make_case(RAGGED, [0] * len(RAGGED), 1)
    if name == "j70":
        return ru.make_case([2, 3, 4], [0, 0, 1], 70, J=70)
    if name == "tie3":
        return ru.make_case([3, 4], [1, 0], 5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name, refine=0, m32=False):
    c = _case(name)
    return ru.restate(c["uv"], c["K"], c["T"], c["views"], PX, refine=refine, m32=m32)


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_restatement_recovers_the_planted_masks_with_margin():
    """The issue's set: 2 and 3 views clean, 4 and 5 with one outlier, 8 and 11 with one (even seeds) or floor((N-1)/3) (odd seeds),
    seeds 0..5 (756 joint solves).  Asserted next to it: the margin that lets the GPU tests ask for equal masks."""
    margin, miss, miss_plain = np.inf, [], []
    for seed in range(6):
        nout = ru.n_outliers(RAGGED, seed % 2 == 1)
        c = ru.make_case(RAGGED, nout, seed)
        offs = np.concatenate([[0], np.cumsum(RAGGED)])
        for b, k in enumerate(nout):
            clean = int(c["planted"][offs[b]:offs[b + 1], 0].sum())
            assert clean == RAGGED[b] - k and (k == 0 or clean >= 3)
        out, inl, cnt, res = ru.restate(c["uv"], c["K"], c["T"], RAGGED, PX)
        assert np.array_equal(inl, c["planted"]), seed
        assert np.array_equal(cnt, np.repeat(np.asarray(RAGGED) - np.asarray(nout), 21).reshape(len(RAGGED), 21))
        margin = min(margin, float(np.abs(res - PX).min()))
        miss.append(np.linalg.norm(out - c["X"], axis=-1))
        miss_plain.append(np.linalg.norm(ru.plain(c["uv"], c["K"], c["T"], RAGGED) - c["X"], axis=-1))
    miss, miss_plain = np.concatenate(miss), np.concatenate(miss_plain)
    print(f"min |r - px| = {margin:.2f} px; robust misses by {miss.mean() * 1e3:.1f} mm (max {miss.max() * 1e3:.1f}), "
          f"plain by {miss_plain.mean() * 1e3:.1f} mm (max {miss_plain.max() * 1e3:.1f})")
    assert margin > 1.0
    assert miss.mean() < 0.2 * miss_plain.mean()
    for name in ("ragged", "clean", "j70"):                   # the cases the GPU tests use carry the same margin
        c = _case(name)
        _, inl, _, res = _want(name)
        assert np.array_equal(inl, c["planted"]) and float(np.nanmin(np.abs(res - PX))) > 1.0, name
    # three views, one outlier: the winner decides the mask, so every HYPOTHESIS has to be clear of the threshold -- and the case
    # shows the limit it is there for: the restatement's choice is not the planted mask
    c = _case("tie3")
    assert ru.hypothesis_margin(c, PX) > 1.0
    _, inl, cnt, _ = _want("tie3")
    assert not np.array_equal(inl[:3], c["planted"][:3]) and np.array_equal(inl[3:], c["planted"][3:]) and cnt[0].min() == 2


def test_key_order_breaks_ties_as_specified():
    assert ru.pick([(-2, 5.0, 1), (-3, 9.0, 7), (-3, 9.5, 2)]) == 1           # the count first
    assert ru.pick([(-3, 9.0, 7), (-3, 8.5, 9), (-2, 0.0, 1)]) == 1           # then the smaller sum
    assert ru.pick([(-3, 9.0, 7), (-3, 9.0, 3), (-3, 9.0, 5)]) == 1           # then the smaller a N + c
    assert ru.pick([(0, 0.0, 5), (0, 0.0, 1)]) == 1
    # a geometric tie: view 2 is a copy of view 1, so pairs (0,1) and (0,2) have one hypothesis and one (count, sum); (0,1) wins
    c = ru.one_sample(_case("clean"), 2)
    dup = {k: np.concatenate([c[k][:2], c[k][1:2], c[k][2:]]) for k in ("uv", "K", "T")}
    M = ru.view_matrices(dup["K"], dup["T"])
    hyp = ru.hypotheses(M, dup["uv"][:, 0], PX)
    keys = [k for k, _ in hyp]
    ids = {k[2]: k for k in keys}
    assert ids[0 * 5 + 1][:2] == ids[0 * 5 + 2][:2] and keys[ru.pick(keys)][2] != 0 * 5 + 2
    assert [k[2] for k in keys] == sorted(k[2] for k in keys)                 # pairs come in the order of a N + c


def test_fallback_below_two_inliers():
    """An inlier radius far below the noise leaves no pair with two inliers: the plain solve over all views, empty mask, count 0."""
    c = ru.one_sample(_case("clean"), 2)
    out, inl, cnt, res = ru.restate(c["uv"], c["K"], c["T"], c["views"], 1e-4)
    assert not inl.any() and not cnt.any()
    assert np.array_equal(out, ru.plain(c["uv"], c["K"], c["T"], c["views"]))
    assert np.isfinite(res).all() and res.max() < 3.0
    bad = dict(c, K=c["K"].copy())
    bad["K"][1, 0, 0] = np.nan                                 # a camera that is not finite: the same road, and NaN
    out, inl, cnt, res = ru.restate(bad["uv"], bad["K"], bad["T"], bad["views"], PX)
    assert np.isnan(out).all() and not inl.any() and not cnt.any() and np.isnan(res).all()


def test_refinement_cost_strictly_decreases():
    c = _case("ragged")
    *_, traces, _ = ru.restate(c["uv"], c["K"], c["T"], c["views"], PX, refine=16, want_trace=True)
    steps = 0
    for tr in traces:
        assert len(tr) >= 1 and all(b < a for a, b in zip(tr[:-1], tr[1:])), tr
        steps += len(tr) - 1
    assert steps >= len(traces)                                # the noisy input leaves every joint at least one useful step
    c16, c0 = _want("ragged", 16), _want("ragged")
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        cost = lambda w: np.where(w[1][s:e], w[3][s:e] ** 2, 0.0).sum(0)     # noqa: E731
        assert (cost(c16) <= cost(c0)).all()


def test_new_entry_point_is_declared_bound_and_exported():
    import poem_v2_amd as pk
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poem_hip.h")).read(), flags=re.S)
    name = "poem_dlt_robust"
    params = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
    assert name in pk.hip.SIGNATURES and hasattr(pk.hip.lib(), name)
    assert len(pk.hip.SIGNATURES[name][1]) == len(params.split(",")) == 14
    assert pk.hip.SIGNATURES[name][1][11] is ctypes.c_double and "double inlier_px" in params
    assert pk.hip.ABI_VERSION == 3 and pk.hip.DLT_MODES == {"threshold": 1, "weighted": 2}      # symbols are only added
    spec = importlib.util.spec_from_file_location("check_abi_decls", os.path.join(ROOT, "tools", "check_abi_decls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    decls, bad = mod.main()
    assert not bad and "poem_launch_dlt_robust" in decls
    # refusals come before any launch: no device needed
    L = pk.hip.lib()
    one = ctypes.c_void_p(16)                                  # any non-null pointer: nothing is dereferenced
    call = lambda px, refine, B=1, J=21: L.poem_dlt_robust(one, one, one, one, one, None, None, None, B, J, 0, px, refine, None)  # noqa: E731
    assert [call(px, 0) for px in (0.0, -1.0, float("nan"))] == [-1, -1, -1]
    assert call(PX, -1) == -1 and call(PX, 17) == -1 and call(PX, 0, J=4097) == -1 and call(PX, 0, B=1 << 20, J=4096) == -1


# ---- GPU ----------------------------------------------------------------------------------------------------------
def _dev(c, *names):
    return [torch.from_numpy(np.ascontiguousarray(c[n])).to(DEV) for n in names]


def _robust(c, px=PX, refine=0, invert=False, **kw):
    """-> (out, count, inlier, resid) on the device"""
    import poem_v2_amd as pk
    uv, K, mat = _dev(c, "uv", "K", "E" if invert else "T")
    return pk.triangulation.triangulate_reference_joints(uv, K, mat, c["views"], mode="ransac", inlier_px=px, refine=refine,
                                                         invert=invert, return_count=True, return_inliers=True, **kw)


def _plain(c, invert=False):
    import poem_v2_amd as pk
    uv, K, mat = _dev(c, "uv", "K", "E" if invert else "T")
    return pk.triangulation.triangulate_reference_joints(uv, K, mat, c["views"], invert=invert)


def _check_against(got, want, name):
    out, count, inlier, resid = got
    w_out, w_inl, w_cnt, w_res = want
    assert out.dtype == torch.float32 and count.dtype == torch.int32 and inlier.dtype == torch.bool and resid.dtype == torch.float32
    assert torch.equal(inlier.cpu(), torch.from_numpy(w_inl)) and torch.equal(count.cpu(), torch.from_numpy(w_cnt))
    err = float(np.abs(out.double().cpu().numpy() - w_out).max())
    err_px = float(np.abs(resid.double().cpu().numpy() - w_res).max())
    print(f"{name}: max |hip - fp64| = {err:.3e} m, residuals {err_px:.3e} px")
    assert err < BAR and err_px < BAR_PX


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "j70"])
def test_hip_masks_counts_joints_and_residuals(name):
    c = _case(name)
    got = _robust(c)
    assert tuple(got[0].shape) == (len(c["views"]), c["uv"].shape[1], 3) and tuple(got[2].shape) == c["uv"].shape[:2]
    _check_against(got, _want(name), name)
    assert torch.equal(got[2].cpu(), torch.from_numpy(c["planted"]))
    # the refit is the plain solve's own arithmetic: the bits poem_triangulate_dlt gives the planted inlier views alone
    for invert in (False, True):
        assert torch.equal(_robust(c, invert=invert)[0], _plain(ru.keep_views(c, c["planted"][:, 0]), invert=invert)), invert


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [True, False])
def test_hip_every_view_an_inlier_is_the_plain_solve_bit_for_bit(invert):
    c = _case("clean")
    plain = _plain(c, invert)
    for px in (1e6, float("inf")):
        out, count, inlier, _ = _robust(c, px=px, invert=invert)
        assert torch.equal(out, plain), px
        assert bool(inlier.all()) and torch.equal(count.cpu(), torch.tensor(c["views"], dtype=torch.int32)[:, None].expand(-1, 21))


@pytest.mark.gpu
def test_hip_recovers_from_one_outlier_view():
    c = _case("ragged")
    X = c["X"]
    miss = np.linalg.norm(_plain(c).double().cpu().numpy() - X, axis=-1)
    robust = _robust(c)[0]
    clean = _plain(ru.keep_views(c, c["planted"][:, 0]))
    gap = (robust.double() - clean.double()).abs().amax((1, 2)).cpu().numpy()
    for b in ONE_OUTLIER:
        print(f"sample {b} ({c['views'][b]} views): plain misses by up to {miss[b].max() * 100:.2f} cm, robust - clean = {gap[b]:.1e} m")
        assert miss[b].max() > 0.01 and gap[b] < BAR


@pytest.mark.gpu
def test_hip_sample_alone_equals_sample_in_batch_and_runs_repeat():
    c = _case("ragged")
    full, again = _robust(c), _robust(c)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        out, count, inlier, resid = _robust(ru.one_sample(c, b))
        assert torch.equal(out[0], full[0][b]) and torch.equal(count[0], full[1][b]), b
        assert torch.equal(inlier, full[2][s:e]) and torch.equal(resid, full[3][s:e]), b


@pytest.mark.gpu
def test_hip_three_views_one_outlier_is_deterministic():
    """Not identifying, but decided: the device makes the restatement's choice, twice."""
    c = _case("tie3")
    got = _robust(c)
    _check_against(got, _want("tie3"), "tie3")
    assert all(torch.equal(a, b) for a, b in zip(got, _robust(c)))
    assert int(got[1][0].min()) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("refine", [1, 4, 16])
def test_hip_refinement(refine):
    """The cost over the inliers, from the outputs, never rises; the joints are the restatement's refined joints within the plain
    solve's bar.  Measured on an MI355X: 7.4e-8 m for every `refine` (the restatement with fp32-formed M against fp64 M: 4.9e-8 m)."""
    c = _case("ragged")
    base, got = _robust(c), _robust(c, refine=refine)
    assert torch.equal(got[2], base[2]) and torch.equal(got[1], base[1])       # refinement moves the joint, not the inlier set
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    for s, e in zip(offs[:-1], offs[1:]):
        cost = lambda g: torch.where(g[2][s:e], g[3][s:e].double() ** 2, 0.0).sum(0)     # noqa: E731
        worst = float((cost(got) - cost(base)).max())
        assert worst <= 0.0, worst
    want = _want("ragged", refine)
    err = float(np.abs(got[0].double().cpu().numpy() - want[0]).max())
    spread = float(np.abs(_want("ragged", refine, True)[0] - want[0]).max())
    print(f"refine={refine}: max |hip - fp64| = {err:.3e} m (restatement with fp32 M against fp64 M: {spread:.3e} m)")
    assert err < BAR
    assert float(np.abs(got[3].double().cpu().numpy() - want[3]).max()) < BAR_PX


@pytest.mark.gpu
def test_hip_nan_handling():
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _case("ragged").items()}
    base = _robust(c)
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    c["uv"][offs[2] + 1, 5, 0] = np.nan                        # one view of the 4-view sample, joint 5
    c["uv"][offs[0] + 1, 7, 1] = np.nan                        # one view of the 2-view sample, joint 7
    c["K"][offs[3] + 2, 1, 1] = np.nan                         # a camera of the 5-view sample
    out, count, inlier, resid = _robust(c)
    assert bool(torch.isfinite(out[2, 5]).all()) and not bool(inlier[offs[2] + 1, 5]) and bool(torch.isnan(resid[offs[2] + 1, 5]))
    assert int(count[2, 5]) == int(inlier[offs[2]:offs[3], 5].sum()) >= 2
    assert bool(torch.isnan(out[0, 7]).all()) and int(count[0, 7]) == 0 and not bool(inlier[offs[0]:offs[1], 7].any())
    assert bool(torch.isnan(out[3]).all()) and not bool(count[3].any()) and not bool(inlier[offs[3]:offs[4]].any())
    assert bool(torch.isnan(resid[offs[3]:offs[4]]).all())
    # everything else keeps its bits
    keep_j = torch.ones(len(c["views"]), 21, dtype=torch.bool)
    keep_j[2, 5] = keep_j[0, 7] = False
    keep_j[3] = False
    keep_v = keep_j[torch.repeat_interleave(torch.arange(len(c["views"])), torch.tensor(c["views"]))]
    assert torch.equal(out.cpu()[keep_j], base[0].cpu()[keep_j]) and torch.equal(count.cpu()[keep_j], base[1].cpu()[keep_j])
    assert torch.equal(inlier.cpu()[keep_v], base[2].cpu()[keep_v]) and torch.equal(resid.cpu()[keep_v], base[3].cpu()[keep_v])
    _check_against((out[:1, :7], count[:1, :7], inlier[:2, :7], resid[:2, :7]),
                   tuple(w[:n, :7] for w, n in zip(_want("ragged"), (1, 2, 1, 2))), "untouched joints of the NaN sample")


def _raw_call(c, px=PX, refine=0, J=None, skip=(), B=None):
    """poem_dlt_robust through ctypes: every output between guard elements, `skip` outputs passed as NULL -> (rc, outputs)"""
    import poem_v2_amd as pk
    uv, K, T = _dev(c, "uv", "K", "T")
    views, Jc = c["views"], c["uv"].shape[1]
    offs = torch.tensor(np.concatenate([[0], np.cumsum(views)]), dtype=torch.int32, device=DEV)
    sizes = {"out": (len(views) * Jc * 3, torch.float32), "inlier": (sum(views) * Jc, torch.uint8),
             "count": (len(views) * Jc, torch.int32), "resid": (sum(views) * Jc, torch.float32)}
    bufs = {k: torch.full((n + 16,), 77, dtype=dt, device=DEV) for k, (n, dt) in sizes.items()}
    p = {k: (None if k in skip else bufs[k].data_ptr()) for k in bufs}
    rc = pk.hip.lib().poem_dlt_robust(uv.data_ptr(), K.data_ptr(), T.data_ptr(), offs.data_ptr(), p["out"], p["inlier"], p["count"],
                                      p["resid"], len(views) if B is None else B, Jc if J is None else J, 0, px, refine, pk.hip.stream())
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t[sizes[k][0]:] == 77).all()), f"{k}: written past its end"
        if k in skip or rc != 0:
            assert bool((t == 77).all()), f"{k}: written although not asked for"
    return rc, {k: t[:sizes[k][0]] for k, t in bufs.items()}


@pytest.mark.gpu
def test_hip_optional_outputs():
    c = _case("ragged")
    rc, full = _raw_call(c)
    assert rc == 0
    got = _robust(c)
    assert torch.equal(full["out"].view(-1, 21, 3), got[0]) and torch.equal(full["count"].view(-1, 21), got[1])
    assert torch.equal(full["inlier"].view(-1, 21).bool(), got[2]) and torch.equal(full["resid"].view(-1, 21), got[3])
    assert int(full["inlier"].max()) == 1
    for skip in (("inlier",), ("count",), ("resid",), ("inlier", "count", "resid")):
        rc, part = _raw_call(c, skip=skip)
        assert rc == 0 and all(torch.equal(part[k], full[k]) for k in full if k not in skip), skip


@pytest.mark.gpu
def test_hip_arguments_are_checked():
    import poem_v2_amd as pk
    c = ru.one_sample(_case("ragged"), 2)
    for px in (0.0, -1.0, float("nan")):
        assert _raw_call(c, px=px)[0] == -1
    for refine in (-1, 17):
        assert _raw_call(c, refine=refine)[0] == -1
    assert _raw_call(c, J=4097)[0] == -1
    assert _raw_call(c, px=float("inf"))[0] == 0 and _raw_call(c, refine=16)[0] == 0
    tri = pk.triangulation.triangulate_reference_joints
    uv, K, T = _dev(c, "uv", "K", "T")
    big = lambda t: t[:1].expand(65, *t.shape[1:]).contiguous()     # noqa: E731
    with pytest.raises(ValueError):
        tri(big(uv), big(K), big(T), [65], mode="ransac", invert=False)
    with pytest.raises(ValueError):
        tri(uv[:3], K[:3], T[:3], [2, 1], mode="ransac", invert=False)
    with pytest.raises(ValueError):
        tri(uv.cpu(), K.cpu(), T.cpu(), c["views"], mode="ransac", invert=False)
    for kw in (dict(inlier_px=0.0), dict(inlier_px=float("nan")), dict(refine=17), dict(refine=-1)):
        with pytest.raises(ValueError):
            tri(uv, K, T, c["views"], mode="ransac", invert=False, **kw)
    with pytest.raises(ValueError, match="ransac"):
        tri(uv, K, T, c["views"], mode="median", invert=False)
    with pytest.raises(ValueError):
        tri(uv, K, T, c["views"], return_inliers=True, invert=False)
    out = torch.empty(1, 21, 3, device=DEV)
    offs = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    assert pk.hip.lib().poem_dlt_confidence(uv.data_ptr(), uv.data_ptr(), K.data_ptr(), T.data_ptr(), offs.data_ptr(), out.data_ptr(), None,
                                            1, 21, 0, 3, 0.5, pk.hip.stream()) == -1


def _build_model(extra):
    import poem_oracle as po
    import poem_v2_amd as pk
    from poem_v2_amd import backbone as bb
    cfg = {"TYPE": "PtEmbedMultiviewStereoV2", "HEAD": pk.configs.head_cfg(128), "DATA_PRESET": {"CENTER_IDX": 9}, **extra}
    model = pk.build_model(pk.CN(cfg))
    model.load_parts(bb.seeded_hrnet_state_dict(0), pk.weights.seeded_decoder_state_dict(0), pk.weights.seeded_state_dict(128, seed=0),
                     template=po.synthetic_template(1234))
    return model


@pytest.mark.gpu
def test_model_ransac_key():
    import poem_v2_amd as pk
    views = [5, 5]
    b = pk.inputs.synthetic_batch(views, seed=4)
    img = pk.inputs.synthetic_images(sum(views), seed=4).to(DEV)
    K, E = b["img_metas"]["cam_intr"].to(DEV), b["img_metas"]["cam_extr"].to(DEV)
    batch = {"image": img, "target_cam_intr": K, "target_cam_extr": E, "master_id": [0] * len(views), "cam_view_num": np.asarray(views)}
    models = {"absent": _build_model({}), "ransac": _build_model({"DLT_CONFIDENCE": "ransac"}),
              "tuned": _build_model({"DLT_CONFIDENCE": "ransac", "DLT_INLIER_PX": 24.0, "DLT_REFINE_ITERS": 4})}
    assert (models["ransac"].dlt_inlier_px, models["ransac"].dlt_refine_iters) == (8.0, 0)
    assert (models["tuned"].dlt_inlier_px, models["tuned"].dlt_refine_iters) == (24.0, 4)
    for bad in ({"DLT_INLIER_PX": 0.0}, {"DLT_REFINE_ITERS": 17}):
        with pytest.raises(ValueError):
            _build_model({"DLT_CONFIDENCE": "ransac", **bad})
    pyr = models["absent"].extract_img_feat(img)            # one pyramid for all (MIOpen may pick other solvers on a later call)
    preds = {}
    for name, m in models.items():
        m.extract_img_feat = lambda x: pyr
        preds[name] = {k: v.clone() if torch.is_tensor(v) else v for k, v in m(batch, 0, mode="test").items()}
    base = preds["absent"]
    hm = models["absent"].decoders.uv_decode(pyr)
    rj = pk.triangulation.reference_joints_from_heatmaps
    # the default route: neither key, and the parent's bits
    assert "pred_joints_inlier" not in base and "pred_joints_reproj" not in base and "pred_joints_conf" not in base
    assert torch.equal(base["pred_ref_joints_3d"], rj(hm, K, E, views, 256, 256))
    for name, kw in (("ransac", {}), ("tuned", dict(inlier_px=24.0, refine=4))):
        p = preds[name]
        assert set(p) == set(base) | {"pred_joints_inlier", "pred_joints_reproj"}
        assert torch.equal(p["pred_ref_joints_3d"], rj(hm, K, E, views, 256, 256, mode="ransac", **kw))
        assert torch.equal(p["pred_joints_uv"], base["pred_joints_uv"])
        assert p["pred_joints_inlier"].dtype == torch.bool and tuple(p["pred_joints_inlier"].shape) == (sum(views), 21)
        assert p["pred_joints_reproj"].dtype == torch.float32 and tuple(p["pred_joints_reproj"].shape) == (sum(views), 21)
        uv = p["pred_joints_uv"]
        _, inl, res = pk.triangulation.triangulate_reference_joints(uv, K, E, views, mode="ransac", return_inliers=True, **kw)
        assert torch.equal(p["pred_joints_inlier"], inl) and torch.equal(p["pred_joints_reproj"], res)


@pytest.mark.gpu
def test_eval_single_prints_the_inlier_fraction(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("eval_single_dlt_robust", os.path.join(ROOT, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    base = ["--cfg", str(tmp_path / "c.yaml"), "--dataset", "DexYCB", "--view_min", "4", "--view_max", "5", "--model", "small", "-g", "0",
            "--epoch_size", "4", "--pyramid"]
    a = es.build_cli().parse_args(base + ["--dlt-confidence", "ransac", "--dlt-inlier-px", "6", "--dlt-refine", "2"])
    assert (a.dlt_confidence, a.dlt_inlier_px, a.dlt_refine) == ("ransac", 6.0, 2)
    assert "dlt_inlier_px" not in vars(es.build_cli().parse_args(base)) and "dlt_refine" not in vars(es.build_cli().parse_args(base))
    es.main(a)
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(f"dlt_inlier_fraction = {res['dlt_inlier_fraction']}")
    assert 0.0 < res["dlt_inlier_fraction"] <= 1.0 and res["samples"] == 4
    es.main(es.build_cli().parse_args(base))
    assert "dlt_inlier_fraction" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
