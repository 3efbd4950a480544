"""N_NEIGHBOR / N_NEIGHBOR_QUERY above 32 (33..64) on the GPU: the K <= 64 neighbour search (poem_knn_k), the two-tile vector
attention (vecattn.hip MODE 4, poem_vector_attention_k) and the whole head against the reference fixtures of
tests/golden/make_golden_k64.py and the oracle."""
import math

import numpy as np
import pytest
import torch

import poem_oracle as po
from poem_v2_amd import hip
from util import batch_to, build_hip_head, case_setup, load_golden, run_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _md(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _thin(meta, key, t):
    """The slice make_golden_k64.thin() took of fixture tap `key` (meta["thinned"]: {tap: [axis, step]}), of a full tensor."""
    axis, step = meta.get("thinned", {}).get(key, (0, 1))
    sl = [slice(None)] * t.ndim
    sl[axis] = slice(None, None, step)
    return t[tuple(sl)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    hip.lib()


# ---- 1. neighbour search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("NQ,NS", [(799, 799), (799, 4096), (40, 64)])
@pytest.mark.parametrize("K", [33, 48, 64])
def test_knn_k_matches_oracle(K, NQ, NS, B, fma):
    g = torch.Generator().manual_seed(K + NQ + NS + B)
    qx = torch.rand(B, NQ, 3, generator=g) * 2 - 1
    sx = qx.clone() if NQ == NS else torch.rand(B, NS, 3, generator=g) * 2 - 1
    got = hip.knn(qx.to(DEV), sx.to(DEV), fma=fma, k=K).cpu().long()
    assert got.shape == (B, NQ, K)
    assert torch.equal(got, po.knn_indices(qx, sx, K, fma))


@pytest.mark.parametrize("K", [33, 64])
def test_knn_k_ties_nan_and_small_counts(K):
    """Many-way ties (every distance equal, and a lattice: the fall-back), NaN coordinates (fewer finite candidates than
    survivors need) and counts at or below 32 at a wider row stride all give the strict (distance, index) order."""
    g = torch.Generator().manual_seed(K)
    qx = torch.rand(2, 70, 3, generator=g) * 2 - 1
    same = torch.zeros(2, 4096, 3)
    assert torch.equal(hip.knn(qx.to(DEV), same.to(DEV), k=K).cpu().long(), po.knn_indices(qx, same, K))
    lat = torch.round((torch.rand(2, 4096, 3, generator=g) * 2 - 1) * 2) / 2
    ql = torch.round(qx * 2) / 2
    assert torch.equal(hip.knn(ql.to(DEV), lat.to(DEV), k=K).cpu().long(), po.knn_indices(ql, lat, K))
    sx = torch.rand(2, 300, 3, generator=g) * 2 - 1
    sx[:, 20:, 1] = float("nan")
    got = hip.knn(qx.to(DEV), sx.to(DEV), k=K).cpu().long()
    assert torch.equal(got[..., :20], po.knn_indices(qx, sx[:, :20], 20))
    assert bool(((got >= 0) & (got < 300)).all())
    sx = torch.rand(2, 799, 3, generator=g) * 2 - 1
    sx[0, 5, 0] = float("nan")
    ok = torch.ones(799, dtype=torch.bool)
    ok[5] = False
    got = hip.knn(qx.to(DEV), sx.to(DEV), k=K).cpu().long()
    assert torch.equal(got[1], po.knn_indices(qx[1:], sx[1:], K)[0])
    assert torch.equal(got[0], torch.nonzero(ok)[:, 0][po.knn_indices(qx[:1], sx[:1, ok], K)[0]])
    ties = torch.zeros(1, 128, 3)
    ties[0, :, 0] = torch.arange(128).float() // 2
    assert hip.knn(torch.zeros(1, 1, 3, device=DEV), ties.to(DEV), k=K).cpu()[0, 0].tolist() == list(range(K))
    idx = torch.full((2, 70, 64), -7, dtype=torch.int32, device=DEV)                    # K = 20 at row stride 64
    s = torch.rand(2, 500, 3, generator=g) * 2 - 1
    qd, sd = qx.to(DEV), s.to(DEV)                                                       # (kept alive across the launch)
    hip.check(hip.lib().poem_knn_k(hip.ptr(qd), hip.ptr(sd), idx.data_ptr(), 2, 70, 500, 20, 64, 0, hip.stream()))
    torch.cuda.synchronize()
    assert torch.equal(idx[..., :20].cpu().long(), po.knn_indices(qx, s, 20)) and bool((idx[..., 20:] == -7).all())


def _knn_k_rows64(qx, sx, K, fma):
    """poem_knn_k at row stride 64 into rows pre-filled with -7 (any K: never the K = 32, ld = 32 shortcut into the narrow kernel)."""
    B, NQ, NS = qx.shape[0], qx.shape[1], sx.shape[1]
    idx = torch.full((B, NQ, 64), -7, dtype=torch.int32, device=DEV)
    qd, sd = qx.to(DEV), sx.to(DEV)                                                      # (kept alive across the launch)
    hip.check(hip.lib().poem_knn_k(hip.ptr(qd), hip.ptr(sd), idx.data_ptr(), B, NQ, NS, K, 64, int(fma), hip.stream()))
    torch.cuda.synchronize()
    return idx.cpu().long()


def _wide_sources(case):
    g = torch.Generator().manual_seed(len(case))
    qx = torch.rand(2, 70, 3, generator=g) * 2 - 1
    if case == "same300":                               # every distance of a query equal: the fall-back rounds
        return qx, torch.zeros(2, 300, 3)
    return qx, torch.rand(2, {"ns130": 130, "ns500": 500}[case], 3, generator=g) * 2 - 1


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("case", ["ns130", "ns500", "same300"])
def test_wide_body_at_k32_equals_the_narrow_kernel(case, fma):
    """One query routine behind both kernels: knn_kernel_k at K = 32 (row stride 64) writes what knn_kernel writes, which is the
    oracle's order; columns 32..63 are not touched.  NS = 130: two 128-candidate pairs, the second all padding but two."""
    qx, sx = _wide_sources(case)
    got = _knn_k_rows64(qx, sx, 32, fma)
    narrow = hip.knn(qx.to(DEV), sx.to(DEV), fma=fma, k=32).cpu().long()
    assert torch.equal(got[..., :32], narrow) and torch.equal(narrow, po.knn_indices(qx, sx, 32, fma))
    assert bool((got[..., 32:] == -7).all())


@pytest.mark.parametrize("fma", [False, True])
def test_wide_body_at_k1_and_k_equal_to_ns(fma):
    qx, sx = _wide_sources("ns500")
    got = _knn_k_rows64(qx, sx, 1, fma)
    assert torch.equal(got[..., :1], po.knn_indices(qx, sx, 1, fma)) and bool((got[..., 1:] == -7).all())
    sx = sx[:, :40].contiguous()                        # K = NS = 40: every source, in order
    got = _knn_k_rows64(qx, sx, 40, fma)
    assert torch.equal(got[..., :40], po.knn_indices(qx, sx, 40, fma)) and bool((got[..., 40:] == -7).all())


# ---- 2. vector attention op ------------------------------------------------------------------------------------------------
def _va_case(C, K, seed, B=2, Q=101, NS=300):
    g = torch.Generator().manual_seed(seed)
    qxyz = torch.rand(B, Q, 3, generator=g) * 2 - 1
    sxyz = torch.rand(B, NS, 3, generator=g) * 2 - 1
    q, k, v = torch.randn(B, Q, C, generator=g), torch.randn(B, NS, C, generator=g), torch.randn(B, NS, C, generator=g)
    w = {}
    for n, shp in (("fc_delta.0", (C, 3)), ("fc_delta.2", (C, C)), ("fc_gamma.0", (C, C)), ("fc_gamma.2", (C, C))):
        w["p." + n + ".weight"] = torch.randn(*shp, generator=g) / math.sqrt(shp[1])
        w["p." + n + ".bias"] = torch.randn(shp[0], generator=g) * 0.1
    return qxyz, sxyz, q, k, v, w


def _va_hip(qxyz, sxyz, idx, q, k, v, w, nk):
    d = lambda t: t.to(DEV).contiguous()   # noqa: E731
    return hip.vector_attention(d(qxyz), d(sxyz), None, d(idx.int()), d(q), d(k), d(v),
                                d(w["p.fc_delta.0.weight"]), d(w["p.fc_delta.0.bias"]),
                                hip.pack_linear(d(w["p.fc_delta.2.weight"])), d(w["p.fc_delta.2.bias"]),
                                hip.pack_linear(d(w["p.fc_gamma.0.weight"])), d(w["p.fc_gamma.0.bias"]),
                                hip.pack_linear(d(w["p.fc_gamma.2.weight"])), d(w["p.fc_gamma.2.bias"]), nk=nk)


@pytest.mark.parametrize("C", [32, 128, 256, 512, 1024])
@pytest.mark.parametrize("K", [40, 64])
def test_vector_attention_k_core(K, C):
    """MODE 4 (plain form) against the oracle's block math over K neighbours in fp32, at the bar of test_vector_attention_core;
    at K = 40 the rows of neighbours 40..63 (idx at row stride 64) carry no weight: changing them leaves every bit."""
    qxyz, sxyz, q, k, v, w = _va_case(C, K, C + K)
    idx = po.knn_indices(qxyz, sxyz, 64)
    ik = idx[..., :K]
    nxyz = po.gather_xyz(sxyz, ik)
    ref = po._vec_attn_core(w, "p.", q, po.index_points(k, ik), po.index_points(v, ik), qxyz[:, :, None] - nxyz, C)
    out = _va_hip(qxyz, sxyz, idx, q, k, v, w, K)
    assert _md(out, ref) < 5e-5
    if K < 64:
        other = idx.clone()
        other[..., K:] = torch.flip(idx[..., K:], dims=[-1]) * 0 + 299      # different rows in the masked columns
        assert torch.equal(_va_hip(qxyz, sxyz, other, q, k, v, w, K), out)


# ---- 3. whole path vs the reference fixtures -------------------------------------------------------------------------------
def _taps_idx(eng, blk, which, B, Q=799):
    n = hip.lib().poem_tap(eng.handle, f"b{blk}.idx_{which}".encode(), None, 0, None)
    assert n == B * Q * 64, n                                            # the buffers' row stride is 64
    return eng.tap(f"b{blk}.idx_{which}", (B, Q, 64), torch.int32).cpu().long()


def test_tinyk64_stage_taps_on_the_gpu():
    z, meta = load_golden("tinyk64")
    spec = meta["spec"]
    cfg, w, consts, batch = case_setup(spec)
    head = build_hip_head(spec, DEV)
    feat, metas, rj = batch_to(batch, DEV)
    with torch.no_grad():
        head(feat, metas, rj)
    eng = head._engine
    eng.enable_taps(True)
    with torch.no_grad():
        out = head(feat, metas, rj)["all_coords_preds"].cpu()
    B, C = len(spec["views"]), spec["embed"]
    for i in range(3):
        for k, tol in (("h_cross", 2e-5), ("f_self", 2e-5), ("f_cross", 2e-5), ("feats", 5e-5)):
            got = _thin(meta, f"tap.b{i}.{k}", eng.tap(f"b{i}.{k}", (B, 799, C)).cpu()[:, ::9])
            assert _md(got, torch.from_numpy(z[f"tap.b{i}.{k}"])) < tol, (i, k)
        if i > 0:
            for which, kk in (("self", spec["knn_query"]), ("cross", spec["knn"])):
                got = _thin(meta, f"tap.b{i}.idx_{which}", _taps_idx(eng, i, which, B)[..., :kk])
                want = torch.from_numpy(z[f"tap.b{i}.idx_{which}"].astype(np.int64))
                same = (torch.sort(got, -1).values == torch.sort(want, -1).values).all(-1)
                assert float(same.float().mean()) > 0.995, (i, which)
    eng.enable_taps(False)
    assert _md(out, torch.from_numpy(z["all_coords_preds"])) < 5e-6


def test_smallk64_neighbour_sets_graphs_and_counts():
    """Hot weights (the neighbour sets decide) at 48 / 64: >= 99.5 % identical sets, every other one a rank-K near-tie of the
    reference's own distances, MPVPE < 1e-5 m; graph replay and plain launches agree bit for bit; the idx taps have stride 64;
    a head with 32 / 32 on the same weights lands > 1e-3 m away."""
    z, meta = load_golden("smallk64")
    spec = meta["spec"]
    cfg, w, consts, batch = case_setup(spec)
    feat, metas, rj = batch_to(batch, DEV)
    head = build_hip_head(spec, DEV)
    with torch.no_grad():
        a = head(feat, metas, rj)["all_coords_preds"].clone()
        b = head(feat, metas, rj)["all_coords_preds"].clone()            # replayed graph
        head.set_option("graphs", 0)
        c = head(feat, metas, rj)["all_coords_preds"].clone()            # plain launches
        head.set_option("graphs", 1)
    assert head._engine.graph_stats()["replays"] >= 1
    assert torch.equal(a, b) and torch.equal(a, c)
    ref = torch.from_numpy(z["all_coords_preds"])
    eng = head._engine
    eng.enable_taps(True)
    with torch.no_grad():
        head(feat, metas, rj)
    B, Q = len(spec["views"]), 799
    pt_xyz = eng.tap("pt_xyz", (B, spec["nsample"], 3)).cpu()
    for blk in (1, 2):
        xyz = torch.from_numpy(z[f"tap.b{blk - 1}.xyz"])
        for which, k in (("self", spec["knn_query"]), ("cross", spec["knn"])):
            want = torch.from_numpy(z[f"tap.b{blk}.idx_{which}"].astype(np.int64))
            got = _thin(meta, f"tap.b{blk}.idx_{which}", _taps_idx(eng, blk, which, B)[..., :k])
            assert want.shape == got.shape and want.shape[-1] == k
            same = (torch.sort(got, dim=-1).values == torch.sort(want, dim=-1).values).all(-1)
            assert float(same.float().mean()) > 0.995, (blk, which)
            step = meta.get("thinned", {}).get(f"tap.b{blk}.idx_{which}", (1, 1))[1]      # (fixture rows = every step-th query)
            for bb, q in torch.nonzero(~same).tolist():
                src = xyz if which == "self" else pt_xyz
                d = xyz[bb, q * step][None] - src[bb]
                d = d * d
                sd = torch.sort((d[:, 0] + d[:, 1]) + d[:, 2]).values
                assert float((sd[k] - sd[k - 1]) / sd[k - 1]) < 1e-5, (blk, which, bb, q)
    eng.enable_taps(False)
    mpvpe = torch.norm(a.cpu()[-1, :, 21:] - ref[-1, :, 21:], dim=-1).mean(dim=1)
    assert float(mpvpe.max()) < 1e-5, mpvpe
    full = build_hip_head(dict(spec, knn=32, knn_query=32), DEV)
    with torch.no_grad():
        d = full(feat, metas, rj)["all_coords_preds"]
    assert _md(d.cpu(), ref) > 1e-3


@pytest.mark.parametrize("name", ["mediumk64", "largek64"])
def test_release_shapes_k64_vs_reference(name):
    z, meta = load_golden(name)
    spec = meta["spec"]
    cfg, w, consts, batch = case_setup(spec)
    head = build_hip_head(spec, DEV)
    feat, metas, rj = batch_to(batch, DEV)
    with torch.no_grad():
        got = head(feat, metas, rj)["all_coords_preds"].cpu()
    ref = torch.from_numpy(z["all_coords_preds"])
    err = torch.norm(got[-1, :, 21:] - ref[-1, :, 21:], dim=-1)
    assert float(err.mean()) < 1e-6, float(err.mean())
    assert _md(got, ref) < 5e-5


# ---- 4. random sweep -------------------------------------------------------------------------------------------------------
def _random_specs_k64(n, seed=2064):
    g = np.random.default_rng(seed)
    counts = [(40, 40), (64, 12), (20, 57), (33, 64), (int(g.integers(1, 65)), int(g.integers(33, 65))),
              (int(g.integers(33, 65)), int(g.integers(1, 65)))]
    specs = []
    for i in range(n):
        C = int(g.choice([32, 64, 128]))
        heads = int(g.choice([h for h in (1, 2, 4, 8, 16) if C % h == 0 and C // h in (8, 16, 32, 64)]))
        B = int(g.integers(1, 4))
        specs.append(dict(embed=C, heads=heads, nblocks=int(g.integers(2, 5)), nsample=int(g.choice([1024, 2048])),
                          knn=counts[i][0], knn_query=counts[i][1], views=[int(v) for v in g.integers(1, 5, size=B)],
                          seed=300 + i, parametric=bool(g.integers(0, 4) == 0), pe_normalize=bool(g.integers(0, 2))))
    return specs


@pytest.mark.parametrize("spec", _random_specs_k64(6), ids=lambda s: "C{embed}h{heads}b{nblocks}S{nsample}k{knn}q{knn_query}".format(**s))
def test_random_constructor_configs_k64_vs_oracle(spec):
    cfg, w, consts, batch = case_setup(spec)
    assert (cfg.knn, cfg.knn_query) == (spec["knn"], spec["knn_query"])
    head = build_hip_head(spec, DEV)
    feat, metas, rj = batch_to(batch, DEV)
    with torch.no_grad():
        res = head(feat, metas, rj)
        again = head(feat, metas, rj)["all_coords_preds"]
    orc = run_oracle(cfg, w, consts, batch)
    got = res["all_coords_preds"].cpu()
    assert got.shape == orc["all_coords_preds"].shape
    assert torch.equal(res["all_coords_preds"], again)
    assert _md(got, orc["all_coords_preds"]) < 5e-6
    if spec["parametric"]:
        assert _md(res["pred_pose"], orc["pred_pose"]) < 2e-4
        assert _md(res["pred_shape"], orc["pred_shape"]) < 2e-5


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_counts_out_of_range_and_split_precision_are_refused():
    import ctypes
    L = hip.lib()
    for knn, nsample, ok in ((64, 1024, True), (65, 1024, False), (48, 32, False), (0, 1024, False)):
        cfg = hip.make_config(32, nsample=nsample, knn=knn)
        assert (L.poem_num_weight_tensors(ctypes.byref(cfg)) > 0) == ok, (knn, nsample)
    with pytest.raises(NotImplementedError):
        build_hip_head(dict(embed=128, nsample=1024, views=[2], seed=5, parametric=False, knn=65, knn_query=65), DEV)
    spec = dict(embed=128, nsample=1024, views=[2, 1], seed=7, parametric=False, knn=32, knn_query=64)
    feat, metas, rj = batch_to(case_setup(spec)[3], DEV)
    h2 = build_hip_head(spec, DEV)
    with pytest.raises(RuntimeError):
        h2.set_precision("split_f16x3")               # no engine yet: refused when the first forward creates it
        with torch.no_grad():
            h2(feat, metas, rj)
    h3 = build_hip_head(spec, DEV)
    with torch.no_grad():
        h3(feat, metas, rj)
    with pytest.raises(RuntimeError):
        h3.set_precision("split_f16x3")               # a live engine refuses at once


def test_raising_knn_query_on_a_live_engine_matches_a_fresh_head():
    """32 -> 64 on an engine that has run (and captured) at 32: the workspace grows with the wider neighbour rows, the next
    forward matches a head built at 32 / 64 bit for bit; and back."""
    spec = dict(embed=64, heads=2, nsample=1024, views=[2, 3], seed=8, parametric=False, knn=32, knn_query=32)
    feat, metas, rj = batch_to(case_setup(spec)[3], DEV)
    head = build_hip_head(spec, DEV)
    with torch.no_grad():
        a32 = [head(feat, metas, rj)["all_coords_preds"].clone() for _ in range(3)]
        head.set_option("knn_query", 64)
        a64 = [head(feat, metas, rj)["all_coords_preds"].clone() for _ in range(3)]
        fresh = build_hip_head(dict(spec, knn_query=64), DEV)(feat, metas, rj)["all_coords_preds"]
        head.set_option("knn_query", 32)
        b32 = head(feat, metas, rj)["all_coords_preds"]
    assert all(torch.equal(x, a64[0]) for x in a64) and torch.equal(a64[0], fresh)
    assert torch.equal(b32, a32[0]) and not torch.equal(a32[0], a64[0])
    with pytest.raises(RuntimeError):
        head.set_option("knn_query", 65)
