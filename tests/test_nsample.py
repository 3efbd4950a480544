"""Any N_SAMPLE up to 8192 on the GPU: the whole head against the reference fixtures of tests/golden/make_golden_nsample.py
(S = 1000, 1600, 3000, 8192, 2500), the cross attention with a partial last key tile (attn.hip MASK forms) against fp32 torch,
the masked instantiations against the unmasked ones, the bit-exact invariants (batch, graph replay, ragged layouts), the
standalone decoder on dense (B, S, C) features, a random sweep against the oracle, and the refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

import poem_oracle as po
import poem_v2_amd as pk
from poem_v2_amd import hip
from nsample_util import setup_case, thin, write_assets
from util import batch_to, build_hip_head, load_golden, run_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _md(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    hip.lib()


def _head(spec, consts, tmp_path, monkeypatch):
    """build_hip_head; a basis above the shipped 4096 points comes from <cwd>/assets (the engine is created at the first forward:
    the caller keeps the working directory until then)."""
    if spec["nsample"] > 4096:
        write_assets(tmp_path, consts["bps"].numpy())
        monkeypatch.chdir(tmp_path)
    return build_hip_head(spec, DEV)


# ---- 1. whole path vs the reference fixtures -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tinyns1000", "smallns1600", "mediumns3000", "tinyns8192", "largens2500"])
def test_head_vs_reference_fixture(name, tmp_path, monkeypatch):
    """MPVPE <= 1e-6 m in every layer; neighbour sets >= 99.5 % equal, every other one a rank-32 near-tie (< 1e-5 relative) of the
    distances; the tiny case's stage taps at the `tiny` bars."""
    z, meta = load_golden(name)
    spec = meta["spec"]
    S, C, B = spec["nsample"], spec["embed"], len(spec["views"])
    cfg, w, consts, batch = setup_case(spec, z["bps"] if "bps" in z.files else None)
    head = _head(spec, consts, tmp_path, monkeypatch)
    feat, metas, rj = batch_to(batch, DEV)
    with torch.no_grad():
        got = head(feat, metas, rj)["all_coords_preds"].cpu()
    ref = torch.from_numpy(z["all_coords_preds"])
    mpvpe = torch.norm(got[:, :, 21:] - ref[:, :, 21:], dim=-1).mean(dim=(1, 2))
    print(f"{name}: MPVPE per layer {mpvpe.tolist()} m, max |d| {_md(got, ref):.3e}")
    eng = head._engine
    eng.enable_taps(True)
    with torch.no_grad():
        again = head(feat, metas, rj)["all_coords_preds"].cpu()
    assert torch.equal(again, got)
    pt_xyz = eng.tap("pt_xyz", (B, S, 3)).cpu()
    assert _md(pt_xyz[:, ::64] if not spec["full"] else pt_xyz, torch.from_numpy(z["tap.pt_xyz"])) == 0.0
    bf = eng.tap("bps_feat", (B, S, C)).cpu()
    want_bf = torch.from_numpy(z["tap.bps_feat"])
    got_bf = thin(meta, "tap.bps_feat", bf) if spec["full"] else bf[:, ::64]
    print(f"{name}: bps_feat max |d| {_md(got_bf, want_bf):.3e}")
    assert _md(got_bf, want_bf) < (5e-5 if spec["full"] else 1e-4)
    if spec["full"]:
        g = eng.tap("g", (sum(spec["views"]), C, S)).cpu()
        assert _md(thin(meta, "tap.g", g), torch.from_numpy(z["tap.g"])) < 2e-5
        for i in range(3):
            for k, tol in (("h_cross", 2e-5), ("f_self", 2e-5), ("f_cross", 2e-5), ("feats", 5e-5)):
                t = thin(meta, f"tap.b{i}.{k}", eng.tap(f"b{i}.{k}", (B, 799, C)).cpu()[:, ::9])
                assert _md(t, torch.from_numpy(z[f"tap.b{i}.{k}"])) < tol, (i, k)
            assert _md(eng.tap(f"b{i}.xyz", (B, 799, 3)).cpu(), torch.from_numpy(z[f"tap.b{i}.xyz"])) < 2e-5, i
    for blk in (1, 2):
        xyz = torch.from_numpy(z[f"tap.b{blk - 1}.xyz"])
        for which in ("self", "cross"):
            want = torch.from_numpy(z[f"tap.b{blk}.idx_{which}"].astype(np.int64))
            full = eng.tap(f"b{blk}.idx_{which}", (B, 799, 32), torch.int32).cpu().long()
            assert int(full.min()) >= 0 and int(full.max()) < (799 if which == "self" else S)      # never a pad row
            got_i = thin(meta, f"tap.b{blk}.idx_{which}", full)
            same = (torch.sort(got_i, dim=-1).values == torch.sort(want, dim=-1).values).all(-1)
            assert float(same.float().mean()) > 0.995, (blk, which, float(same.float().mean()))
            step = meta.get("thinned", {}).get(f"tap.b{blk}.idx_{which}", (1, 1))[1]
            for bb, q in torch.nonzero(~same).tolist():
                src = xyz if which == "self" else pt_xyz
                d = xyz[bb, q * step][None] - src[bb]
                d = d * d
                sd = torch.sort((d[:, 0] + d[:, 1]) + d[:, 2]).values
                assert float((sd[32] - sd[31]) / sd[31]) < 1e-5, (blk, which, bb, q)
    eng.enable_taps(False)
    assert float(mpvpe.max()) <= 1e-6, mpvpe


# ---- 2. cross attention with an uneven key count ---------------------------------------------------------------------------
def _attn_ref(q, k, v, heads):
    B, NQ, C = q.shape
    dh = C // heads
    sp = lambda t: t.double().view(B, -1, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
    s = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(dh)
    return (torch.softmax(s, -1) @ sp(v)).permute(0, 2, 1, 3).reshape(B, NQ, C)


@pytest.mark.parametrize("NK", [40, 1000, 3000, 4100])
@pytest.mark.parametrize("C,heads,NQ", [(256, 4, 799), (128, 4, 100), (32, 4, 799), (64, 4, 70), (512, 4, 130), (1024, 4, 40), (64, 2, 33)])
def test_cross_attention_uneven_key_count(C, heads, NQ, NK):
    """poem_cross_attention at nk % 32 != 0, every head dim (8 .. 256: xattn_kernel and xattn_stream_kernel, masked), against
    fp32 torch at test_cross_attention's tolerance; a spiked key in the partial tile and one right in front of it.  The scratch
    (partials + images) is sized by whole key tiles."""
    g = torch.Generator().manual_seed(C + NQ + NK)
    B = 2
    q, k, v = (torch.randn(B, n, C, generator=g) for n in (NQ, NK, NK))
    q = q * 2.0
    k[0, NK - 1] = q[0, 5] * 3
    k[1, NK - (NK % 32) - 1] = q[1, 7] * 3
    out = hip.cross_attention(q.to(DEV), k.to(DEV), v.to(DEV), heads)
    err = _md(out, _attn_ref(q, k, v, heads))
    print(f"C{C} h{heads} NQ{NQ} NK{NK}: max |d| {err:.3e}")
    assert bool(torch.isfinite(out).all())
    assert err < 2e-5
    NKP = (NK + 31) // 32 * 32
    if NKP != NK:
        assert hip.lib().poem_cross_attention_scratch_bytes(B, NQ, NK, C, heads) == hip.lib().poem_cross_attention_scratch_bytes(B, NQ, NKP, C, heads)


_LAUNCHERS = {}


def _launcher(name, restype, argtypes):
    """A launcher of launchers.h that is not part of the public ABI (bound here, as tests/test_attention_forms.py does)."""
    if name not in _LAUNCHERS:
        fn = getattr(ctypes.CDLL(hip.LIB_PATH), name)
        fn.restype, fn.argtypes = restype, argtypes
        _LAUNCHERS[name] = fn
    return _LAUNCHERS[name]


def _images(k, v, NK, fill):
    """The K / V fragment images of attn.hip for (B, NK, C) keys / values, whole 32-key tiles per sample, the rows behind the
    last key set to `fill`."""
    B, _, C = k.shape
    NKP = (NK + 31) // 32 * 32
    nkt = NKP // 32
    kp = torch.full((B, NKP, C), fill, dtype=torch.float32)
    vp = torch.full((B, NKP, C), fill, dtype=torch.float32)
    kp[:, :NK], vp[:, :NK] = k, v
    # KI[(kt * C/8 + kco) * 64 + lane] = K[32 kt + (lane & 31)][8 kco + 4 (lane >> 5) + 0..3]
    ki = kp.view(B, nkt, 32, C // 8, 2, 4).permute(0, 1, 3, 4, 2, 5).contiguous()
    # VI[((kt * C/32 + vt) * 4 + g) * 64 + lane] = V[32 kt + 8 g + 4 (lane >> 5) + 0..3][32 vt + (lane & 31)]
    vi = vp.view(B, nkt, 4, 2, 4, C // 32, 32).permute(0, 1, 5, 2, 3, 6, 4).contiguous()
    return ki.view(-1), vi.view(-1)


@pytest.mark.parametrize("C,heads,NK,B,NQ", [(256, 4, 1000, 2, 799), (32, 4, 40, 2, 100), (512, 4, 3000, 1, 130), (256, 4, 4070, 2, 40)])
def test_rows_behind_the_last_key_carry_weight_exactly_zero(C, heads, NK, B, NQ):
    """poem_launch_cross_attention_img (and the merged launcher at 4070 keys) on images whose pad rows hold 1e30 instead of
    zeros: the context rows equal the zero-padded run bit for bit and are finite -- a dead column's numerator is exactly 0 whatever
    its raw score (overflowed or NaN) and whatever finite V row it would have weighted."""
    _vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    img = _launcher("poem_launch_cross_attention_img", _i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp])
    nfl = _launcher("poem_cross_attention_scratch_floats", _sz, [_i] * 6)
    g = torch.Generator().manual_seed(C + NK)
    q, k, v = (torch.randn(B, n, C, generator=g) for n in (NQ, NK, NK))
    qd = q.to(DEV)
    scratch = torch.empty(nfl(B, NQ, NK, C, heads, 0) + 64, dtype=torch.float32, device=DEV)
    outs = []
    for fill in (0.0, 1e30):
        ki, vi = (t.to(DEV) for t in _images(k, v, NK, fill))
        ctx = torch.empty_like(qd)
        assert img(hip.ptr(qd), C, hip.ptr(ki), hip.ptr(vi), hip.ptr(ctx), B, NQ, NK, C, heads, hip.ptr(scratch), hip.stream()) == 0
        torch.cuda.synchronize()
        outs.append(ctx.clone())
        if NK == 4070:
            mrg = _launcher("poem_launch_cross_attention_merged", _i, [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp])
            ctx2 = torch.empty_like(qd)
            assert mrg(hip.ptr(qd), C, NQ, hip.ptr(ki), hip.ptr(vi), hip.ptr(ctx2), B, NQ, NK, C, heads, hip.stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(ctx2, ctx)
    assert bool(torch.isfinite(outs[1]).all())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], hip.cross_attention(qd, k.to(DEV), v.to(DEV), heads))      # the row-major entry's own zero fill
    assert _md(outs[1], _attn_ref(q, k, v, heads)) < 2e-5


@pytest.mark.parametrize("NK", [3000, 4070, 4096])
def test_masked_remainder_halves_at_the_production_batch(NK):
    """xattn_masked_half_item: at C = 256, four heads, B = 32, 799 queries the 256-block launch deals 25 (3000 keys: one chunk) or
    100 (4070 / 4096 keys: four chunks) items to a CU pair against a round of 24 -- a remainder of 1 or 4 items, which runs as
    channel-tile halves (head dim 64, three waves per SIMD).  With dead columns (3000: 8, 4070: 26) against fp32 torch at
    test_cross_attention's tolerance and against the run with the halves switched off bit for bit; at 4096 keys the masked
    twin (forced, no dead column) with and without halves equals the unmasked kernel bit for bit."""
    halves = _launcher("poem_cross_attention_tail_halves", None, [ctypes.c_int])
    force = _launcher("poem_cross_attention_masked_form", None, [ctypes.c_int])
    B, NQ, C, heads = 32, 799, 256, 4
    props = torch.cuda.get_device_properties(0)
    items = B * heads * ((NK + 31) // 32 // (32 if NK > 4064 else (NK + 31) // 32)) * 25
    pairs = props.multi_processor_count // 2
    assert props.multi_processor_count % 16 == 0 and 0 < (items // pairs + (1 if items % pairs else 0)) % 24 <= 4, "no remainder halves at this shape on this chip"
    g = torch.Generator().manual_seed(NK)
    q, k, v = (torch.randn(B, n, C, generator=g) for n in (NQ, NK, NK))
    q = q * 2.0
    k[3, NK - 1] = q[3, 790] * 3                      # a spiked key in the last tile, seen by a query of the last (remainder) items
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    if NK % 32 == 0:
        plain = hip.cross_attention(qd, kd, vd, heads)
        force(1)
    try:
        with_halves = hip.cross_attention(qd, kd, vd, heads)
        halves(0)
        try:
            without = hip.cross_attention(qd, kd, vd, heads)
        finally:
            halves(1)
    finally:
        force(0)
    assert torch.equal(with_halves, without)
    if NK % 32 == 0:
        assert torch.equal(with_halves, plain)
    err = max(_md(with_halves[b:b + 1], _attn_ref(q[b:b + 1], k[b:b + 1], v[b:b + 1], heads)) for b in range(B))
    print(f"NK{NK} B32 masked halves: max |d| {err:.3e}")
    assert err < 2e-5


@pytest.mark.parametrize("NK,B,NQ", [(4100, 1, 799), (4070, 2, 40), (4090, 3, 799)])
def test_cross_attention_merged_uneven_key_count(NK, B, NQ):
    """poem_cross_attention_merged (xattn_kernel MERGE, and its channel-tile HALF items at one sample) at nk % 32 != 0: shapes it
    takes (four chunks of 32 tiles: 4065 .. 4096 keys) equal partials + combine bit for bit and fp32 torch to tolerance; 4100
    keys (129 tiles, one chunk) are not its shape."""
    g = torch.Generator().manual_seed(NK + B + NQ)
    C, heads = 256, 4
    q, k, v = (torch.randn(B, n, C, generator=g) for n in (NQ, NK, NK))
    q = q * 2.0
    k[0, NK - 1] = q[0, 5] * 4
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    a = hip.cross_attention(qd, kd, vd, heads)
    assert _md(a, _attn_ref(q, k, v, heads)) < 2e-5
    if NK > 4096:
        with pytest.raises(RuntimeError):
            hip.cross_attention(qd, kd, vd, heads, merged=True)
        return
    b = hip.cross_attention(qd, kd, vd, heads, merged=True)
    assert torch.equal(a, b)


@pytest.mark.parametrize("NK", [1000, 3000])
def test_cross_attention_merged_refuses_other_shapes(NK):
    q = torch.randn(1, 40, 256, device=DEV)
    k = torch.randn(1, NK, 256, device=DEV)
    with pytest.raises(RuntimeError):
        hip.cross_attention(q, k, k, 4, merged=True)


# ---- 3. masked form == unmasked form at zero dead columns ------------------------------------------------------------------
@pytest.mark.parametrize("C,heads,NK,B,NQ", [(256, 4, 4096, 3, 799), (256, 4, 4096, 32, 799), (256, 4, 4096, 32, 130), (128, 4, 1024, 2, 799), (32, 4, 1024, 2, 100),
                                             (64, 4, 64, 2, 70), (64, 8, 2048, 1, 50), (512, 4, 4096, 1, 200), (1024, 4, 2048, 1, 64)])
def test_masked_instantiation_with_no_dead_column_equals_the_unmasked_one(C, heads, NK, B, NQ):
    """On a key count divisible by 32 the MASK instantiations (forced through the launcher's test switch) give the unmasked
    kernels' bits: same items, same fma chains, a mask that touches nothing -- for xattn_kernel (at B = 32 with 799 queries a CU
    pair's 100 items leave a remainder of 4, which runs as xattn_masked_half_item halves; with 130 queries, 20 items, none do),
    xattn_stream_kernel and, at 4096 keys and head dim 64, the merged kernel."""
    L = hip.lib()
    sw = L.poem_cross_attention_masked_form
    sw.restype, sw.argtypes = None, [ctypes.c_int]
    g = torch.Generator().manual_seed(C + NK + B)
    q, k, v = (torch.randn(B, n, C, generator=g).to(DEV) for n in (NQ, NK, NK))
    forms = [False] + ([True] if (C // heads == 64 and NK == 4096) else [])
    for merged in forms:
        plain = hip.cross_attention(q, k, v, heads, merged=merged)
        sw(1)
        try:
            masked = hip.cross_attention(q, k, v, heads, merged=merged)
        finally:
            sw(0)
        assert torch.equal(plain, masked), merged


# ---- 4. bit-exact invariants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C", [(1000, 128), (3000, 256)])
def test_batch_graph_and_ragged_layout_invariants(S, C):
    """A sample alone equals the same sample inside a batch of five; graph replay equals plain launches; ragged view layouts
    [3, 1, 6] run (the operator front end sizes its launches by the batch's own view total) and match the oracle."""
    spec = dict(embed=C, nsample=S, views=[3, 1, 6, 2, 2], seed=81, parametric=False)
    cfg, w, consts, batch = setup_case(spec)
    head = build_hip_head(spec, DEV)
    feat, metas, rj = batch_to(batch, DEV)
    with torch.no_grad():
        a = head(feat, metas, rj)["all_coords_preds"].clone()
        b = head(feat, metas, rj)["all_coords_preds"].clone()
        c = head(feat, metas, rj)["all_coords_preds"].clone()            # replayed graph
        head.set_option("graphs", 0)
        d = head(feat, metas, rj)["all_coords_preds"].clone()
        head.set_option("graphs", 1)
    assert head._engine.graph_stats()["replays"] >= 1
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    offs = np.concatenate([[0], np.cumsum(spec["views"])])
    for i in (0, 2, 4):      # sample i alone (B = 1)
        m1 = dict(metas)
        m1["cam_intr"] = metas["cam_intr"][offs[i]:offs[i + 1]].contiguous()
        m1["cam_extr"] = metas["cam_extr"][offs[i]:offs[i + 1]].contiguous()
        m1["cam_view_num"] = [spec["views"][i]]
        with torch.no_grad():
            one = head(feat[offs[i]:offs[i + 1]].contiguous(), m1, rj[i:i + 1].contiguous())["all_coords_preds"]
        assert torch.equal(one[:, 0], a[:, i]), i
    sub = dict(spec, views=[3, 1, 6])
    cfg3, w3, consts3, batch3 = setup_case(sub)
    f3, m3, r3 = batch_to(batch3, DEV)
    with torch.no_grad():
        got3 = head(f3, m3, r3)["all_coords_preds"].cpu()
    assert _md(got3, run_oracle(cfg3, w3, consts3, batch3)["all_coords_preds"]) < 5e-6


# ---- 5. standalone decoder on dense (B, S, C) features ---------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 256])
def test_standalone_decoder_on_dense_features_equals_the_heads_decoder(C):
    """PtEmbedTRv4 (poem_decoder_forward) on the head's own dense (B, 1000, C) bps_feat / pt_xyz and its query inputs: the
    library pads the rows itself, and the coordinates equal the head's decoder run with the anchor tables off (the standalone
    entry never uses them) bit for bit."""
    spec = dict(embed=C, nsample=1000, views=[2, 3], seed=82, parametric=False)
    cfg, w, consts, batch = setup_case(spec)
    head = build_hip_head(spec, DEV)
    feat, metas, rj = batch_to(batch, DEV)
    B = 2
    with torch.no_grad():
        head(feat, metas, rj)
        eng = head._engine
        eng.set_anchor_tables(False)
        eng.enable_taps(True)
        head(feat, metas, rj)
        pt_feats = eng.tap("bps_feat", (B, 1000, C)).clone()
        pt_xyz = eng.tap("pt_xyz", (B, 1000, 3)).clone()
        qxyz = eng.tap("query_xyz", (B, 799, 3)).clone()
        want = torch.stack([eng.tap(f"b{i}.xyz", (B, 799, 3)).clone() for i in range(3)])
        eng.enable_taps(False)
        qf = head.state_dict()["query_feat_embedding.weight"][None].expand(B, -1, -1).contiguous()
        got, pose, shape = head.transformer(qxyz, qf, pt_xyz, pt_feats)
    assert pose is None and shape is None
    assert got.shape == want.shape
    assert torch.equal(got, want)


# ---- 6. random sweep -------------------------------------------------------------------------------------------------------
def _random_specs(n, seed=8192):
    g = np.random.default_rng(seed)
    fixed_s = [775, 8192, 4097, 8191]
    specs = []
    for i in range(n):
        C = int(g.choice([32, 64, 128]))
        heads = int(g.choice([h for h in (1, 2, 4, 8, 16) if C % h == 0 and C // h in (8, 16, 32, 64)]))
        B = int(g.integers(1, 4))
        S = fixed_s[i] if i < len(fixed_s) else int(g.integers(775, 8193))
        knn = int(g.choice([32, 32, int(g.integers(1, 65))]))
        specs.append(dict(embed=C, heads=heads, nblocks=int(g.integers(2, 4)), nsample=S, knn=knn, knn_query=knn,
                          views=[int(v) for v in g.integers(1, 4, size=B)], seed=400 + i, parametric=False))
    return specs


@pytest.mark.parametrize("spec", _random_specs(8), ids=lambda s: "C{embed}h{heads}b{nblocks}S{nsample}k{knn}".format(**s))
def test_random_nsample_configs_vs_oracle(spec, tmp_path, monkeypatch):
    cfg, w, consts, batch = setup_case(spec)
    head = _head(spec, consts, tmp_path, monkeypatch)
    feat, metas, rj = batch_to(batch, DEV)
    with torch.no_grad():
        res = head(feat, metas, rj)["all_coords_preds"]
        again = head(feat, metas, rj)["all_coords_preds"]
    orc = run_oracle(cfg, w, consts, batch)["all_coords_preds"]
    assert torch.equal(res, again)
    err = _md(res.cpu(), orc)
    print(f"S{spec['nsample']} C{spec['embed']}: max |d| vs oracle {err:.3e} m")
    assert err < 5e-6


# ---- 7. neighbour search up to 8192 sources, refusals ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("NS", [5000, 8191, 8192])
def test_knn_takes_8192_sources(NS, K):
    """poem_knn / poem_knn_k (knn_kernel, knn_kernel_k: 116 / 136 KB of LDS at 8192 sources) in the oracle's strict (distance,
    index) order; 8193 sources are refused."""
    g = torch.Generator().manual_seed(NS + K)
    q = (torch.rand(2, 799, 3, generator=g) * 2 - 1)
    s = (torch.rand(2, NS, 3, generator=g) * 2 - 1)
    got = hip.knn(q.to(DEV), s.to(DEV), k=K).cpu().long()
    assert torch.equal(got, po.knn_indices(q, s, K))
    with pytest.raises(RuntimeError):
        hip.knn(q.to(DEV), torch.zeros(2, 8193, 3, device=DEV), k=K)


def test_split_precision_and_missing_basis_are_refused(tmp_path, monkeypatch):
    spec = dict(embed=128, nsample=1000, views=[2, 1], seed=7, parametric=False)
    feat, metas, rj = batch_to(setup_case(spec)[3], DEV)
    h = build_hip_head(spec, DEV)
    with torch.no_grad():
        h(feat, metas, rj)
    with pytest.raises(RuntimeError):
        h.set_precision("split_f16x3_all")            # a live engine refuses at once: no masked split-precision kernels
    with pytest.raises(RuntimeError):
        h.set_precision("split_f16x3")
    ok = build_hip_head(dict(spec, nsample=1600), DEV)      # a multiple of 32 that is no multiple of embed: split precision is fine
    with torch.no_grad():
        a = ok(feat, metas, rj)["all_coords_preds"]
        ok.set_precision("split_f16x3_all")
        b = ok(feat, metas, rj)["all_coords_preds"]
    assert _md(a, b) < 1e-4
    q = torch.randn(1, 40, 128, device=DEV)
    k = torch.randn(1, 1000, 128, device=DEV)
    with pytest.raises(RuntimeError):
        hip.cross_attention(q, k, k, 4, split=True)
    monkeypatch.chdir(tmp_path)                       # no asset directory here, the shipped basis has 4096 points
    big = build_hip_head(dict(spec, embed=32, nsample=5000), DEV)
    with pytest.raises(FileNotFoundError) as e:
        with torch.no_grad():
            big(feat[:, :, :, :], metas, rj)
    assert "5000" in str(e.value) and "make_basis" in str(e.value)
    L = hip.lib()
    for nsample, okc in ((8192, True), (8193, False), (20, False)):
        cfg = hip.make_config(32, nsample=nsample)
        assert (L.poem_num_weight_tensors(ctypes.byref(cfg)) > 0) == okc
