"""Pin the CPU oracle against golden vectors captured from the imported reference (tests/golden/make_golden.py)."""
import numpy as np
import pytest
import torch

import poem_oracle as po
from util import case_setup, load_golden, neighbour_report, run_oracle, stage_report


def _maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


@pytest.mark.parametrize("name", ["tiny", "tinymano", "tinypetr", "tinynonorm", "tinypetrlid", "tinyk", "tinycfg2", "tinycfg4"])
def test_tiny_stage_taps(name):
    z, meta = load_golden(name)
    cfg, w, consts, batch = case_setup(meta["spec"])
    taps = {}
    out = run_oracle(cfg, w, consts, batch, taps=taps)
    # sampling stage: full tensors
    assert _maxdiff(taps["x"], z["tap.x"]) < 2e-5                      # input_proj + positional table
    assert _maxdiff(taps["g"], z["tap.g"]) < 2e-5                      # projection + bilinear sampling
    assert _maxdiff(taps["bps_feat"], z["tap.bps_feat"]) < 5e-5        # Q1 + merge (sv and mv)
    assert _maxdiff(taps["pt_xyz"], z["tap.pt_xyz"]) == 0.0
    assert _maxdiff(taps["query_xyz"], z["tap.query_xyz"]) == 0.0
    assert out["all_coords_preds"].shape[0] == meta["spec"].get("nblocks", 3)
    for i in range(meta["spec"].get("nblocks", 3)):
        for k, tol in (("h_cross", 2e-5), ("f_self", 2e-5), ("f_cross", 2e-5), ("feats", 5e-5)):
            assert _maxdiff(taps[f"b{i}.{k}"][:, ::9], z[f"tap.b{i}.{k}"]) < tol, (i, k)
        assert _maxdiff(taps[f"b{i}.xyz"], z[f"tap.b{i}.xyz"]) < 2e-5, i
    assert _maxdiff(out["all_coords_preds"], z["all_coords_preds"]) < 2e-6   # metres
    if meta["spec"]["parametric"]:
        assert _maxdiff(out["pred_pose"], z["pred_pose"]) < 1e-4
        assert _maxdiff(out["pred_shape"], z["pred_shape"]) < 1e-5


@pytest.mark.parametrize("name", ["small", "medium", "large", "huge", "ragged", "mediummano", "mediumpetr", "smallk", "mediumk"])
def test_release_shapes(name):
    z, meta = load_golden(name)
    cfg, w, consts, batch = case_setup(meta["spec"])
    taps = {}
    out = run_oracle(cfg, w, consts, batch, taps=taps)
    assert _maxdiff(taps["bps_feat"][:, ::64], z["tap.bps_feat"]) < 1e-4
    ref = z["all_coords_preds"]
    got = out["all_coords_preds"].numpy()
    err = np.linalg.norm(got[-1, :, 21:] - ref[-1, :, 21:], axis=-1)     # per-vertex error, metres
    # MPVPE-vs-reference bar of BASELINE.json: 1e-3 mm = 1e-6 m
    assert err.mean() < 1e-6, err.mean()
    assert _maxdiff(got, ref) < 5e-5
    if meta["spec"]["parametric"]:     # medium_MANO tail (Q3 + rot6d -> axis-angle), toy MANO stand-in on both sides
        assert _maxdiff(out["pred_pose"], z["pred_pose"]) < 1e-4
        assert _maxdiff(out["pred_shape"], z["pred_shape"]) < 1e-5


def test_the_petr_and_normalize_switches_change_the_positional_embedding():
    """The round-5 fixtures really exercise the two switches: on the SAME inputs and weights the oracle's `x` moves by O(1) when
    PETR_EMBEDDING is dropped / NORMALIZE flipped, and the frustum features are not saturated (most of the synthetic cameras'
    frustum lies inside position_range)."""
    import dataclasses
    for name, field in (("tinypetr", "petr"), ("tinynonorm", "pe_normalize"), ("tinypetrlid", "petr")):
        z, meta = load_golden(name)
        cfg, w, consts, batch = case_setup(meta["spec"])
        taps, flipped = {}, {}
        run_oracle(cfg, w, consts, batch, taps=taps)
        run_oracle(dataclasses.replace(cfg, **{field: not getattr(cfg, field)}), w, consts, batch, taps=flipped)
        assert _maxdiff(taps["x"], z["tap.x"]) < 2e-5 and _maxdiff(flipped["x"], z["tap.x"]) > 0.05, name
        if cfg.petr:
            m = batch["img_metas"]
            f = po.frustum_features(cfg, m["cam_intr"], m["cam_extr"], 16, 16, m["inp_img_shape"])
            assert f.shape == (sum(meta["spec"]["views"]), 3 * cfg.depth_num, 16, 16)
            inside = float((f.abs() < 11.0).float().mean())          # |inverse_sigmoid| = 11.51 at the clamps
            assert 0.3 < inside < 1.0, inside


@pytest.mark.parametrize("name", ["small_hot", "medium_hot", "large_hot"])
def test_hot_weights_oracle_vs_reference(name):
    """Non-benign weights (block Linears x2.5, LayerNorm gains spread 0.3: coordinate updates ~1 normalised unit per block,
    neighbour sets of blocks 1, 2 far from the template's).  The restatement must stay at round-off distance from the
    reference *stage by stage*, and where a neighbour set differs it must be a near-tie of the 32nd / 33rd candidate --
    the reference's own sensitivity to summation order -- not an error of the restatement."""
    z, meta = load_golden(name)
    spec = meta["spec"]
    cfg, w, consts, batch = case_setup(spec)
    taps = {}
    out = run_oracle(cfg, w, consts, batch, taps=taps)
    upd = np.abs(z["tap.b0.xyz"] - z["tap.query_xyz"]).max()
    assert upd > 0.3, upd                                        # the case is hot: block 0 moves queries by O(1)
    rep = stage_report(z, spec, lambda n, shape, dt=None: taps[n], taps)
    for key, st in rep["stages"].items():
        assert st["path_clean"] <= 2e-6 * max(st["scale"], 1.0), (key, st)      # ~16 ulp of the tensor's scale
    for key, nb in rep["neighbours"].items():
        assert nb["set_equal"] >= 0.995, (key, nb)
        for b, q, gap in nb["flips"]:
            assert gap < 1e-5, (key, b, q, gap)                  # attributed: a near-tie in the reference's own distances
    ref, got = z["all_coords_preds"], out["all_coords_preds"].numpy()
    for layer in range(3):
        err = np.linalg.norm(got[layer, :, 21:] - ref[layer, :, 21:], axis=-1).mean(axis=1)
        assert err.max() < 1e-6, (layer, err)                    # the 1e-3 mm bar, every layer, every sample


ROUND3 = ["medium_g1", "medium_g4", "medium_g6", "small_tie", "small_tie_fma"]


@pytest.mark.parametrize("name", ROUND3)
def test_conditioning_sweep_and_cuda_rounding_oracle_vs_reference(name):
    """Round-3 fixtures.  ``medium_g{1,4,6}`` (+ ``medium_hot`` = gain 2.5): the same case with the block Linears scaled by the
    gain -- where two correct fp32 evaluations of the reference's arithmetic stop agreeing to 1e-3 mm.  ``*_fma``: the
    reference's neighbour search rounding its distances like pytorch3d's CUDA kernel (fma-contracted; poem_oracle.knn_distances)
    while the restatement keeps the CPU kernel's rounding.  Bars: every stage on the clean rows within 2e-6 of its scale (up to
    gain 2.5; 1e-5 / 5e-5 at gain 4 / 6, where the conditioning of the weights amplifies round-off stage by stage); every
    neighbour-set difference attributed to a near-tie (32nd / 33rd distance gap < 1e-5 relative); MPVPE <= 1e-3 mm up to gain
    2.5 and <= 1e-5 of the coordinates' magnitude beyond (at gain 4 the mesh has left the 0.1 m ball: |xyz| = 2.8 m, gain 6:
    632 m -- fp32 round-off of such coordinates alone is above the bar)."""
    import dataclasses
    z, meta = load_golden(name)
    spec = meta["spec"]
    cfg, w, consts, batch = case_setup(spec)
    ref = z["all_coords_preds"]
    scale = float(np.abs(ref).max())
    results = {}
    for fma in ([False, True] if spec.get("knn_fma") else [False]):
        taps = {}
        out = run_oracle(dataclasses.replace(cfg, knn_fma=fma), w, consts, batch, taps=taps)
        rep = stage_report(z, spec, lambda n, shape, dt=None: taps[n], taps)
        gain = spec.get("gain", 1.0)
        stage_tol = 2e-6 if gain <= 2.5 else (1e-5 if gain <= 4 else 5e-5)
        flips = 0
        for key, nb in rep["neighbours"].items():
            assert nb["set_equal"] >= 0.995, (key, nb)
            flips += len(nb["flips"])
            for b, q, gap in nb["flips"]:
                assert gap < 1e-5, (key, b, q, gap)
        # run with the OTHER rounding than the fixture's and a set did flip (small_tie_fma under the CPU rounding): the flipped
        # query's features differ by O(1e-2) and block 2 gathers that row into its neighbours' rows -- the stage bars hold for
        # the matching rounding only; the flip is attributed above and the mesh bar below still holds
        mismatched = bool(fma) != bool(spec.get("knn_fma")) and flips > 0
        for key, st in rep["stages"].items():
            if not mismatched:
                assert st["path_clean"] <= stage_tol * max(st["scale"], 1.0), (key, st)
        if name == "small_tie_fma":
            assert (flips > 0) == (not fma), (fma, flips)        # the matching rounding reproduces every set, the other one does not
        got = out["all_coords_preds"].numpy()
        err = max(float(np.linalg.norm(got[l, :, 21:] - ref[l, :, 21:], axis=-1).mean(axis=1).max()) for l in range(3))
        assert err < max(1e-6, 1e-5 * scale), (fma, err, scale)
        results[fma] = err
    if spec.get("gain", 1.0) <= 2.5:
        assert max(results.values()) < 1e-6, results             # the 1e-3 mm bar holds up to the hot operating point


def tie_pair_searches():
    """The searches the reference ran in the small_tie / small_tie_fma pair, with the coordinates it ran them on:
    -> [(fma, block, which, query_xyz, src_xyz, recorded idx)].  pt_xyz is an elementwise fp32 function of the inputs and equal
    in the reference and the restatement bit for bit (checked on the fixture's stored rows)."""
    out = []
    for name in ("small_tie", "small_tie_fma"):
        z, meta = load_golden(name)
        spec = meta["spec"]
        cfg, w, consts, batch = case_setup(spec)
        pt_xyz = ((consts["bps"][None] + batch["reference_joints"][:, 9:10]) - batch["reference_joints"][:, 9:10]) / cfg.radius
        assert np.array_equal(pt_xyz[:, ::64].numpy(), z["tap.pt_xyz"])
        for blk in (1, 2):
            xyz = torch.from_numpy(z[f"tap.b{blk - 1}.xyz"])
            for which, src in (("self", xyz), ("cross", pt_xyz)):
                out.append((bool(spec.get("knn_fma")), blk, which, xyz, src, torch.from_numpy(z[f"tap.b{blk}.idx_{which}"].astype(np.int64))))
    return out


def test_tie_pair_the_reference_itself_depends_on_the_third_partys_rounding():
    """small_tie / small_tie_fma: the reference's OWN head on one seeded case with pytorch3d's two distance roundings (CPU kernel
    / CUDA kernel).  Unlike round 3's *_fma fixtures -- bit-identical to their twins, so every test on them re-tested the twin --
    this pair differs: one block-1 cross search resolves a near-tie at rank 32 differently, and the outputs move by 0.15 mm.
    The restatement's neighbour search must reproduce EACH run's recorded index sets from the coordinates that run saw, with
    that run's rounding -- every query, no attribution -- and must NOT reproduce them with the other rounding."""
    za, zb = load_golden("small_tie")[0], load_golden("small_tie_fma")[0]
    diff = {k: int((np.sort(za["tap." + k], -1) != np.sort(zb["tap." + k], -1)).any(-1).sum())
            for k in ("b1.idx_self", "b1.idx_cross", "b2.idx_self", "b2.idx_cross")}
    assert diff["b1.idx_cross"] >= 1 and np.array_equal(za["tap.b0.xyz"], zb["tap.b0.xyz"]), diff
    assert float(np.abs(za["all_coords_preds"] - zb["all_coords_preds"]).max()) > 1e-5           # metres: the flip reaches the mesh
    wrong = 0
    for fma, blk, which, xyz, src, want in tie_pair_searches():
        got = po.knn_indices(xyz, src, 32, fma)
        assert torch.equal(torch.sort(got, -1).values, torch.sort(want, -1).values), (fma, blk, which)
        other = po.knn_indices(xyz, src, 32, not fma)
        wrong += int((torch.sort(other, -1).values != torch.sort(want, -1).values).any(-1).sum())
    assert wrong >= 2, wrong            # the block-1 cross search of each run is mis-reproduced by the other rounding


def near_tie_points(seed=12, B=2, NQ=200, NS=4096):
    """Queries within 1e-5 of the centre of a unit shell of sources: all NS distances of a query lie within 4e-5 of 1, i.e.
    consecutive sorted distances are ~1e-8 apart -- below fp32 resolution (1.2e-7): ties and near-ties everywhere, so the
    order at rank 32 is decided by HOW the distance is rounded."""
    g = torch.Generator().manual_seed(seed)
    q = 1e-5 * torch.randn(B, NQ, 3, generator=g)
    s = torch.nn.functional.normalize(torch.randn(B, NS, 3, generator=g), dim=-1)
    return q, s


def test_cuda_rounding_of_the_neighbour_distances_reorders_only_near_ties():
    """knn_distances(fma=True) -- nvcc's contraction of pytorch3d's accumulation loop -- against the CPU kernel's rounding:
    the two differ by a few 2^-23 relative per distance (the CPU form rounds three products and two sums, the fused form one
    product and two fused steps).  On scattered points they pick the same neighbour sets; on near-tied points they do
    not, and every difference is a pair of candidates within that round-off of each other."""
    g = torch.Generator().manual_seed(12)
    q = torch.randn(4, 799, 3, generator=g) * 0.4
    s = torch.randn(4, 4096, 3, generator=g) * 0.4
    d0, d1 = po.knn_distances(q, s, False), po.knn_distances(q, s, True)
    assert bool(((d0 - d1).abs() <= 2.5 * d0.abs() * 2.0 ** -23).all()) and bool((d0 != d1).any())
    i0, i1 = po.knn_indices(q, s, 32, False), po.knn_indices(q, s, 32, True)
    assert torch.equal(torch.sort(i0, -1).values, torch.sort(i1, -1).values)       # 3196 scattered queries: no set differs
    q, s = near_tie_points()
    d0 = po.knn_distances(q, s, False)
    i0, i1 = po.knn_indices(q, s, 32, False), po.knn_indices(q, s, 32, True)
    same = (torch.sort(i0, -1).values == torch.sort(i1, -1).values).all(-1)
    assert 0 < int((~same).sum())                                                   # the rounding decides here ...
    for b, qi in torch.nonzero(~same).tolist():
        sd = torch.sort(d0[b, qi]).values
        assert float((sd[32] - sd[31]) / sd[31]) < 5 * 2.0 ** -23                   # ... and only between near-tied candidates


@pytest.mark.parametrize("name", ["tiny", "medium", "ragged"])
def test_anchor_table_form_is_equivalent(name):
    """The HIP path's default evaluates block 0's positional terms once per forward from template / radius (every sample's
    query coordinates are ((c + t) - c) / r, the anchors are fixed -- quirk Q2).  Restated in the oracle
    (head_forward(anchor_tables=True)) it must stay at the reference fixture's round-off distance: the MPVPE bar, and no
    further from the fixture than twice the plain oracle (+ 2e-5 mm)."""
    z, meta = load_golden(name)
    cfg, w, consts, batch = case_setup(meta["spec"])
    ref = z["all_coords_preds"]
    mp = lambda o: float(np.linalg.norm(o["all_coords_preds"].numpy()[-1, :, 21:] - ref[-1, :, 21:], axis=-1).mean())
    plain = mp(run_oracle(cfg, w, consts, batch))
    tab = run_oracle(cfg, w, consts, batch, anchor_tables=True)
    assert mp(tab) < 1e-6, mp(tab)
    assert mp(tab) < 2 * plain + 2e-8, (mp(tab), plain)
    assert _maxdiff(tab["all_coords_preds"], ref) < 5e-5


def test_hoisted_cross_attention_is_equivalent():
    z, meta = load_golden("tiny")
    cfg, w, consts, batch = case_setup(meta["spec"])
    out = run_oracle(cfg, w, consts, batch, hoist=True)
    assert _maxdiff(out["all_coords_preds"], z["all_coords_preds"]) < 2e-6


def test_grid_sample_restatement_matches_torch():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 16, 16, generator=g)
    grid = torch.rand(3, 200, 2, generator=g) * 2.6 - 1.3      # includes out-of-range taps (zero padding)
    ref = torch.nn.functional.grid_sample(x, grid[:, :, None], align_corners=False).squeeze(-1)
    assert _maxdiff(po.grid_sample_bilinear(x, grid), ref) < 1e-5


def test_q1_quirk_addressing():
    # SURVEY Q1 probe: N=2, C=256, S=4096, (s,n,c)=(5,1,7) -> n'=0, c'=0, s'=2823
    N, C, S = 2, 256, 4096
    g = torch.arange(N * C * S, dtype=torch.float32).view(N, C, S)
    q = po.q1_rows(g)
    assert q.shape == (S, N, C)
    assert q[5, 1, 7] == g[0, 0, 2823]


def test_mean_epe_known_answer():
    z = np.load(__import__("os").path.join(__import__("util").GOLDEN, "mepe.npz"))
    pred, gt = torch.from_numpy(z["pred"]), torch.from_numpy(z["gt"])
    s1, n1 = po.mean_epe(pred, gt)
    s2, n2 = po.mean_epe(pred[:2] * 2, gt[:2])
    assert abs(s1 - float(z["sum1"])) < 1e-7 and abs(s2 - float(z["sum2"])) < 1e-7
    assert abs((s1 + s2) / (n1 + n2) - float(z["avg"])) < 1e-8


def test_q2_quirk_block0_takes_the_fixed_anchors_for_both_attentions():
    """SURVEY Q2 (point_transformers.py:10-32,71-79,129-136): in block 0 every query's 32 "neighbours" are the fixed
    anchors, for the self AND the cross attention; in the cross attention the anchor ids index the basis-point FEATURE
    rows while the coordinates are the anchors' template-space positions.  Pinned by the tiny fixture's block-0 taps
    (test_tiny_stage_taps); here the semantics themselves: only the 32 anchor rows of the basis-point features can
    influence block 0's vector cross attention."""
    z, meta = load_golden("tiny")
    cfg, w, consts, batch = case_setup(meta["spec"])
    g = torch.Generator().manual_seed(3)
    B, Q, S, C = 2, 799, meta["spec"]["nsample"], cfg.embed
    qxyz, qf = torch.randn(B, Q, 3, generator=g) * 0.3, torch.randn(B, Q, C, generator=g)
    pxyz, pf = torch.randn(B, S, 3, generator=g) * 0.3, torch.randn(B, S, C, generator=g)
    taps = {}
    with torch.no_grad():
        po.decoder_block(w, cfg, 0, qxyz, qf, pxyz, pf, consts, taps=taps)
    aidx = consts["anchor_idx"].long()
    assert aidx.numel() == 32 and int(aidx.max()) < 775
    assert torch.equal(taps["b0.idx_self"], aidx.view(1, 1, 32).expand(B, Q, 32))
    assert torch.equal(taps["b0.idx_cross"], taps["b0.idx_self"])
    # perturb a basis-point feature row that is NOT an anchor id: the vector cross attention of block 0 must not see it
    # (the two BERT cross attentions do attend to every row, so compare f_cross given identical h: use the taps' inputs)
    free = next(i for i in range(S) if i not in set(aidx.tolist()))
    p = "transformer.pt_metro_encoder.0."
    ke = po.linear(pf, w[p + "embedding.weight"], w[p + "embedding.bias"])
    ke2 = ke.clone(); ke2[:, free] += 1.0
    ke3 = ke.clone(); ke3[:, int(aidx[5])] += 1.0
    idx = taps["b0.idx_cross"]
    nxyz = consts["anchor"].view(1, 1, 32, 3).expand(B, Q, 32, 3)
    vp = p + "encoder.vec_attn.query_cross_attn."
    with torch.no_grad():
        f0 = po.vec_attn_cross(w, vp, qxyz, taps["b0.f_self"], ke, idx, nxyz)
        f1 = po.vec_attn_cross(w, vp, qxyz, taps["b0.f_self"], ke2, idx, nxyz)
        f2 = po.vec_attn_cross(w, vp, qxyz, taps["b0.f_self"], ke3, idx, nxyz)
    assert torch.equal(f0, f1) and not torch.equal(f0, f2)


def test_q3_quirk_flat_reshape_runs_of_799():
    """SURVEY Q3 (pt_metro_transformer.py:139-151): (B,799,C).reshape(-1,799) chunks each sample's 799*C floats into C
    consecutive runs of 799 -- row r of the Linear(799,1) input is flat[r*799:(r+1)*799], NOT channel r."""
    B, C = 2, 8
    feats = torch.arange(B * 799 * C, dtype=torch.float32).view(B, 799, C)
    wflat = torch.zeros(1, 799); wflat[0, 3] = 1.0            # picks element 3 of every run
    w = {"p.flat_verts.weight": wflat, "p.flat_verts.bias": torch.zeros(1),
         "p.mano_linear.weight": torch.zeros(106, C), "p.mano_linear.bias": torch.zeros(106)}
    w["p.mano_linear.weight"][96, 5] = 1.0                    # beta_0 <- run 5 of each sample
    w["p.mano_linear.bias"][0:96:6] = 1.0                     # a valid rot6d (x axis, y axis) so the tail stays finite
    w["p.mano_linear.bias"][4:96:6] = 1.0
    mano = lambda pose, betas: (torch.zeros(B, 778, 3), torch.zeros(B, 21, 3))   # noqa: E731
    xyz, pose, betas = po.parametric_tail(w, "p.", feats, torch.zeros(B, 799, 3), mano, C)
    flat = feats.reshape(B, -1)
    assert torch.equal(betas[:, 0], flat[:, 5 * 799 + 3])     # run 5, element 3 of the sample's flat storage
    assert float(flat[0, 5 * 799 + 3]) != float(feats[0, 3, 5])   # ... which is not (vertex 3, channel 5)


def test_split_precision_arithmetic_emulated_in_the_oracle():
    """The opt-in mode's arithmetic (vector-attention C x C products as f16 hi/lo splits, fp32 sums) emulated inside the
    CPU oracle on the POEM-small fixture: its MPVPE from the plain-fp32 oracle stays at fp32 re-ordering level, two orders
    below the 1e-3 mm bar (the pre-study behind csrc/vecattn_split.hip; tools/lab/split_precision_probe.py has the sweep)."""
    import torch.nn.functional as F
    z, meta = load_golden("small")
    cfg, w, consts, batch = case_setup(meta["spec"])
    ref = run_oracle(cfg, w, consts, batch)["all_coords_preds"]

    def split(x):
        hi = x.to(torch.float16).float()
        return hi, (x - hi).to(torch.float16).float()

    plain = po.linear

    def lin(x, wt, b=None):
        if wt.shape[0] != wt.shape[1] or x.dim() != 4:
            return F.linear(x, wt, b)
        (xh, xl), (wh, wl) = split(x), split(wt)
        y = F.linear(xh, wh) + F.linear(xl, wh) + F.linear(xh, wl)
        return y if b is None else y + b

    po.linear = lin
    try:
        got = run_oracle(cfg, w, consts, batch)["all_coords_preds"]
    finally:
        po.linear = plain
    d_mm = float((got[-1, :, 21:] - ref[-1, :, 21:]).norm(dim=-1).mean()) * 1e3
    assert 0 < d_mm < 1e-4, d_mm


@pytest.mark.parametrize("sl", [(slice(1, 3),), (slice(2, 3),)], ids=["all_views", "non_master_view"])
def test_nan_views_give_the_centre(sl):
    """ptEmb_head.py:944 (`torch.nan_to_num(interm_ref_pts)`) seen from the whole path: a sample with NaN backbone features --
    all its views, or only a non-master view (the NaN then enters through merge_features_mv's dot products) -- comes out as its
    hand centre in every layer; the other sample is untouched.  (The GPU twin: tests/test_hip_parity.py::test_nan_features_...)"""
    spec = dict(embed=32, nsample=1024, views=[1, 2], seed=19, parametric=False)
    cfg, w, consts, batch = case_setup(spec)
    clean = run_oracle(cfg, w, consts, batch)["all_coords_preds"]
    bad = dict(batch, mlvl_feat=batch["mlvl_feat"].clone())
    bad["mlvl_feat"][sl] = float("nan")
    out = run_oracle(cfg, w, consts, bad)["all_coords_preds"]
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, 1], batch["reference_joints"][1, 9].expand(3, 799, 3))
    assert torch.equal(out[:, 0], clean[:, 0])


NAN_FIXTURES = {"tinynan": 1, "tinynan2": 1, "smallnan": 1}      # fixture -> the sample whose view(s) are NaN


@pytest.mark.parametrize("name", sorted(NAN_FIXTURES))
def test_nan_fixtures_the_reference_itself_returns_the_centre(name):
    """Round-6 fixtures generated from the reference with one sample's feature maps NaN (all its views; only a non-master view):
    the REFERENCE returns that sample's hand centre in every layer (nan_to_num -> 0, x radius + centre) and finite values
    everywhere; the oracle reproduces the fixture, the poisoned sample bit for bit."""
    z, meta = load_golden(name)
    b = NAN_FIXTURES[name]
    ref = torch.from_numpy(z["all_coords_preds"])
    cfg, w, consts, batch = case_setup(meta["spec"])
    assert torch.isnan(batch["mlvl_feat"]).any()
    centre = batch["reference_joints"][b, 9]
    assert torch.isfinite(ref).all() and torch.equal(ref[:, b], centre.expand(3, 799, 3))
    out = run_oracle(cfg, w, consts, batch)["all_coords_preds"]
    assert torch.equal(out[:, b], ref[:, b])
    assert _maxdiff(out, ref) < 2e-6


@pytest.mark.parametrize("NQ,NS,seed", [(799, 799, 0), (799, 4096, 1), (64, 2048, 2)])
def test_neighbour_search_against_an_independent_kd_tree(NQ, NS, seed):
    """The neighbour search is the one stage whose upstream implementation (pytorch3d knn_points) is absent here, so the
    fixtures cannot pin it.  An implementation the oracle shares nothing with -- scipy's k-d tree, fp64 distances of the same
    fp32 coordinates -- must return the same 32 neighbours in the same order wherever the order is decided by more than
    fp32 rounding (consecutive fp64 distances further apart than 1e-5 relative); inside such near-ties only the SET of the
    tied group is compared.  What stays unpinned is the order inside near-ties, i.e. the rounding of the third party's
    kernels -- the `knn_fma` switch and the tie_pair fixtures are about exactly that."""
    from scipy.spatial import cKDTree
    g = torch.Generator().manual_seed(seed)
    q = (torch.rand(2, NQ, 3, generator=g) - 0.5) * 0.4
    s = q.clone() if NS == NQ else (torch.rand(2, NS, 3, generator=g) - 0.5) * 0.4
    got = po.knn_indices(q, s, 32).numpy()
    strict = 0
    for b in range(2):
        d64, i64 = cKDTree(s[b].double().numpy()).query(q[b].double().numpy(), k=33)
        d64 = d64 ** 2
        for i in range(NQ):
            gaps = np.diff(d64[i]) > 1e-5 * np.maximum(d64[i][1:], 1e-12)     # gaps[k]: neighbour k and k + 1 are well separated
            lo = 0
            for k in range(32):
                if gaps[k]:                                                    # a group of mutually near-tied neighbours ends at k
                    if k == lo:
                        assert got[b, i, k] == i64[i, k]
                        strict += 1
                    else:
                        assert set(got[b, i, lo:k + 1]) == set(i64[i, lo:k + 1])
                    lo = k + 1
    assert strict > 0.95 * 2 * NQ * 32          # nearly every position is decided by a clear gap


def test_neighbour_count_fixtures_depend_on_the_counts():
    """`tinyk` / `smallk` / `mediumk` (N_NEIGHBOR / N_NEIGHBOR_QUERY = 16 / 8, 20 / 12, 16 / 24; the reference head's own outputs)
    really exercise the two keys: the fixtures hold neighbour taps of exactly those widths, and on the hot-weight case the oracle
    with the release value 32 -- or with the two keys swapped -- lands millimetres away (6e-8 m with the right ones)."""
    import dataclasses
    for name, counts in (("tinyk", (16, 8)), ("smallk", (20, 12)), ("mediumk", (16, 24))):
        z, meta = load_golden(name)
        assert (meta["spec"]["knn"], meta["spec"]["knn_query"]) == counts
        for b in (1, 2):
            assert z[f"tap.b{b}.idx_cross"].shape[-1] == counts[0] and z[f"tap.b{b}.idx_self"].shape[-1] == counts[1]
    z, meta = load_golden("smallk")
    cfg, w, consts, batch = case_setup(meta["spec"])
    assert (cfg.knn, cfg.knn_query) == (20, 12)
    ref = z["all_coords_preds"]
    assert _maxdiff(run_oracle(cfg, w, consts, batch)["all_coords_preds"], ref) < 2e-6
    for other in (dataclasses.replace(cfg, knn=32, knn_query=0), dataclasses.replace(cfg, knn=12, knn_query=20)):
        assert _maxdiff(run_oracle(other, w, consts, batch)["all_coords_preds"], ref) > 1e-3
