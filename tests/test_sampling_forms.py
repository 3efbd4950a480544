"""The sampling-stage kernels (merge.hip: project_table / input_tables, sample_merge, sample_group, merge_tail; sample.hip: the
operator sequence project_uv, grid_sample, merge_reduce, merge_finalize) in every form the forward launches them, called through
their launchers at the smallest shapes at which each mechanism exists, and held against the float64 restatement of
tests/sampling_forms_util.py (itself held against the oracle's functions on the CPU, first test below).

Scenes.  A canonical batch of 17 samples -- view counts 1, 3, 2, 5, 4, 6, 8, 7, 9, 10 (N | 8 interleaved with the others) and seven
single-view samples -- with cameras that keep the points inside the image, straddle every border, look away from the points and
project with q_z = 0 (the |z| < 1e-7 clamp).  Every other batch is a selection of these samples (with repeats), so its rows must
be the canonical launch's rows of the same samples, bit for bit, whatever the batch and wherever the sample sits in it.

Bars.
  tables       weights and pixels: bit-equal to the fp32 function (floor, two differences, one product, masks, clamps) of the
               kernel's own (ix, iy); (ix, iy) under the end-to-end bar, per view.
  stage-local  on the kernel's own upstream output, a-priori bounds with u = 2^-24:
                 sampled value (q1)   4 u sum_k |w_k| |tap_k|                         (one product and three fused steps)
                 Linear               2 (K + 2) u (|x| |W|^T + |b|) + (input error) |W|^T      (test_chain_forms.py's bound)
                 view reduction       d_n = <h_n, h_0> in any order: |fl(d_n) - d_n| <= HALF u D_n, D_n = sum_c |h_n||h_0|;
                                      m = sum_{n=1}^{N-1} d_n h_n as a chain of N - 1 fused steps from 0: each term carries at
                                      most N - 1 roundings, so |fl(m) - m| <= (HALF + N - 1) u sum_n D_n |h_n|  (1.01 for the
                                      second-order terms)
                 / N, + q1            one rounding each: 2 u (|q1| + |y| / N)
  end to end   |HIP - fp64| <= 4 |fp32 - fp64| + 1e-6 max|fp64| from the cameras, per sample and separately for the basis points
               with a Q1 row in the first or last tile of a view and for the others, for the two-kernel, the grouped and the
               operator form; the ratios |HIP - fp64| / |fp32 - fp64| are printed.
  bit for bit  every claim of merge.hip's header (see the tests).

A NaN view.  The Q1 view gives basis point s of an N-view sample the Q1 rows s N .. s N + N - 1, which lie in view
(s N + n) / S: a view of NaN planes poisons the points whose rows touch it (all of them for N = 1), not the whole sample.  The
test holds exactly those rows to NaN (they are the rows where the restatement is NaN) and every other row to the clean bits."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import poem_oracle as po
import sampling_forms_util as sf
from poem_v2_amd import hip
from util import MergeTailArgs, SampleGroupArgs, SampleMergeArgs

gpu = pytest.mark.gpu
DEV = "cuda:0"
HIP_INVALID_VALUE = 1
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float

HEAD = [1, 3, 2, 5, 4, 6, 8, 7, 9, 10]      # N | 8 interleaved with the others
NPROTO1 = 7                                  # single-view samples behind them: the fillers of the large batches cycle through these
CANON_VIEWS = HEAD + [1] * NPROTO1


# =====================================================================================================================
# the restatement against the oracle (CPU)
def _scene_inputs(C, S, fh, fw, img_w, img_h, views, seed, kinds=None):
    V = sum(views)
    g = torch.Generator().manual_seed(seed)
    kinds = kinds or [sf.VIEW_KINDS[(v * 3 + 1) % 4] if v % 5 == 4 else ("inside" if v % 2 else "straddle") for v in range(V)]
    intr, extr = sf.make_cameras(kinds, img_w, img_h, seed + 1)
    return dict(x=torch.randn(V, C, fh * fw, generator=g), bps=sf.make_points(S, seed + 2),
                centre=torch.randn(len(views), 3, generator=g) * 0.02, intr=intr, extr=extr, kinds=kinds,
                view_sample=torch.repeat_interleave(torch.arange(len(views)), torch.tensor(views)))


def test_restatement_matches_the_oracle():
    """sampling_forms_util against oracle/poem_oracle.py's project_points, grid_sample_bilinear, q1_rows and merge_views in
    float64 (C = 128, S = 256, views [1, 3, 2], a non-square map and image, all four kinds of camera); the table variant through
    the 16-bit packing; the fp32 variant close to the fp64 one; the two h2 layouts and the q1 rows as index sets."""
    C, S, fh, fw, img_w, img_h, views = 128, 256, 8, 24, 384, 128, [1, 3, 2]
    sc = _scene_inputs(C, S, fh, fw, img_w, img_h, views, 7, kinds=["inside", "straddle", "behind", "clamp", "inside", "straddle"])
    W = sf.MergeWeights(C, 11)
    x, bps, centre, vs, intr, extr = sc["x"], sc["bps"], sc["centre"], sc["view_sample"], sc["intr"], sc["extr"]
    # oracle, float64
    world = bps.double()[None] + centre.double()[:, None]
    uv = po.project_points(world, intr.double(), extr.double(), vs)
    grid = uv * (1.0 / torch.tensor([img_w, img_h], dtype=torch.float64)) * 2 - 1
    g_o = po.grid_sample_bilinear(x.double().view(-1, C, fh, fw), grid)
    wd, offs = W.oracle_dict(), [0, 1, 4, 6]
    out_o = torch.stack([po.merge_views(wd, po.q1_rows(g_o[offs[i]:offs[i + 1]])) for i in range(3)])
    # the restatement
    ix, iy = sf.project_ixiy(bps, centre, vs, intr, extr, fh, fw, img_w, img_h)
    ix_o, iy_o = ((grid[..., 0] + 1) * fw - 1) / 2, ((grid[..., 1] + 1) * fh - 1) / 2
    for a, b in ((ix, ix_o), (iy, iy_o)):
        assert float(((a - b).abs() / (1 + b.abs())).max()) < 1e-9
    kinds_seen = {int(k) for k in (sf.table_from_ixiy(ix, iy, fh, fw)[0] != 0).sum(-1).unique()}
    assert {0, 1, 2, 4} <= kinds_seen, kinds_seen
    got = sf.stage_from_coordinates(x, bps, centre, vs, intr, extr, fh, fw, img_w, img_h, views, W)
    scale = float(out_o.abs().max())
    assert float((got["out"] - out_o).abs().max()) < 1e-10 * scale
    w, pix = sf.table_from_ixiy(ix, iy, fh, fw)
    assert int(pix.max()) < fh * fw and torch.equal(sf.unpack_tabo(sf.pack_tabo(pix)), pix)
    g_t = sf.sample_table(x.double(), w, sf.unpack_tabo(sf.pack_tabo(pix)))
    assert float((g_t - g_o).abs().max()) < 1e-10 * float(g_o.abs().max())
    tab = sf.stage_from_table(x, w, pix, views, W)
    assert torch.equal(tab["out"], got["out"])
    q1_o = torch.stack([po.q1_rows(g_o[offs[i]:offs[i + 1]])[:, 0] for i in range(3)])
    assert float((tab["q1"] - q1_o).abs().max()) < 1e-10 * float(q1_o.abs().max())
    # fp32 variant: the same function to fp32 round-off
    g32 = sf.stage_from_coordinates(x, bps, centre, vs, intr, extr, fh, fw, img_w, img_h, views, W, fp32=True)
    assert g32["out"].dtype == torch.float32
    assert float((g32["out"].double() - out_o).abs().max()) < 2e-4 * scale
    h = torch.randn(5, 3, 256, generator=torch.Generator().manual_seed(3))
    assert float((sf.reduce_views(h, fp32=True).double() - sf.reduce_views(h.double())).abs().max()) < 1e-3
    # index functions
    for Cx in (128, 256, 512):
        for Sx in (Cx, 8 * Cx):
            V = 3
            perm = sf.h2_permutation(V, Cx, Sx)
            assert torch.equal(torch.sort(perm).values, torch.arange(V * Sx)), (Cx, Sx)
            NSEG, XS = Sx // Cx, sf.xs_of(Cx)
            for v, c, seg in ((0, 0, 0), (1, XS, NSEG - 1), (2, Cx - 1, NSEG // 2), (1, XS - 1, 0)):
                R = sf.h2_row_major(v, c, seg, Cx, Sx)
                assert int(perm[R]) == sf.h2_tile_major(v, c, seg, Cx, Sx)
                assert R == v * Sx + c * NSEG + seg
            # a tile's XS rows are consecutive; tiles of a view, views back to back
            assert sf.h2_tile_major(1, XS + 5, 0, Cx, Sx) == (1 * (Cx // XS) * NSEG + NSEG) * XS + 5
            hits = torch.zeros(3 * Sx, dtype=torch.long)
            for b, (off, N) in enumerate(((0, 1), (1, 3), (4, 2))):
                rows = [sf.q1_row(b, off, N, v, c, seg, Cx, Sx) for v in range(off, off + N) for c in range(0, Cx, 37)
                        for seg in range(NSEG)]
                assert all(r == -1 or b * Sx <= r < (b + 1) * Sx for r in rows)
                r = torch.arange(N * Sx)
                hits += torch.bincount(b * Sx + r[r % N == 0] // N, minlength=3 * Sx)
            assert bool((hits == 1).all()), (Cx, Sx)
    # the launch mirror's cells are disjoint and reachable
    for ncu in (256, 64, 304):
        for kern, Cx, Sx in (("sample_merge", 128, 128), ("sample_group", 256, 2048), ("merge_tail", 512, 512)):
            for cell, n in sf.cell_counts(kern, Cx, Sx, ncu).items():
                assert sf.grid_cell(kern, Cx, Sx, n, n, ncu) == cell, (kern, Cx, Sx, ncu, cell, n)


# =====================================================================================================================
# GPU: launchers
_PROTOS = {
    "poem_launch_project_table": (_i, [_vp] * 8 + [_i] * 7 + [_vp]),
    "poem_launch_input_tables": (_i, [_vp] * 11 + [_i] * 8 + [_f, _vp]),
    "poem_launch_prep_xyz": (_i, [_vp] * 6 + [_i] * 3 + [_f, _vp]),
    "poem_launch_invert_extr": (_i, [_vp, _vp, _i, _vp]),
    "poem_launch_sample_merge": (_i, [ctypes.POINTER(SampleMergeArgs), _i, _vp]),
    "poem_launch_sample_group": (_i, [ctypes.POINTER(SampleGroupArgs), _i, _vp]),
    "poem_launch_merge_tail": (_i, [ctypes.POINTER(MergeTailArgs), _i, _vp]),
    "poem_sample_merge_supported": (_i, [_i, _i, _i]),
    "poem_device_cu_count": (_i, []),
    "poem_launch_project_uv": (_i, [_vp] * 7 + [_i] * 6 + [_vp]),
    "poem_launch_grid_sample": (_i, [_vp] * 3 + [_i] * 5 + [_vp]),
    "poem_launch_grid_sample_ex": (_i, [_vp] * 3 + [_i] * 6 + [_vp]),
    "poem_launch_project_sample": (_i, [_vp] * 9 + [_i] * 7 + [_vp]),
    "poem_launch_merge_reduce": (_i, [_vp] * 3 + [_i] * 3 + [_vp]),
    "poem_launch_merge_finalize": (_i, [_vp] * 4 + [_i] * 3 + [_vp]),
}
_FNS = {}


def _fn(name):
    if name not in _FNS:
        res, args = _PROTOS[name]
        _FNS[name] = ctypes.CFUNCTYPE(res, *args)((name, hip.lib()))
    return _FNS[name]


def _call(name, *args):
    rc = _fn(name)(*args, hip.stream())
    assert rc == 0, f"{name} returned {rc}"


@pytest.fixture(scope="module")
def ncu():
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    assert not torch.backends.cuda.matmul.allow_tf32, "the fp32 restatement needs full-precision fp32 GEMMs"
    n = _fn("poem_device_cu_count")()
    assert n > 0
    return n


_CANARY = 0x7FC0DEAD      # a NaN bit pattern no kernel writes
_GUARD = 64               # guard rows in front of and behind every output


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Guarded:
    """(rows, width) floats holding the canary, with guard rows in front and behind"""

    def __init__(self, rows, width):
        self.rows = rows
        self.buf = torch.full((rows + 2 * _GUARD, width), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf[_GUARD:].data_ptr()

    def take(self, what):
        assert bool((self.buf[:_GUARD] == _CANARY).all()) and bool((self.buf[_GUARD + self.rows:] == _CANARY).all()), \
            f"{what}: a guard row was written"
        return self.buf[_GUARD:_GUARD + self.rows].view(torch.float32)


class _Packed(sf.MergeWeights):
    def __init__(self, C, seed):
        super().__init__(C, seed, DEV)
        self.p00, self.p02, self.p10, self.p12 = (hip.pack_linear(w.contiguous()) for w in (self.w00, self.w02, self.w10, self.w12))
        torch.cuda.synchronize()


class _Scene:
    """A batch on the device: planes in both layouts, cameras, and the kernels' own tables (project_table on invert_extr's
    inverse, with its (ix, iy))."""

    def __init__(self, C, S, fh, fw, img_w, img_h, views, seed, kinds=None, bps=None, centre=None):
        self.C, self.S, self.fh, self.fw, self.hw, self.img = C, S, fh, fw, fh * fw, (img_w, img_h)
        self.views, self.V, self.B = list(views), sum(views), len(views)
        sc = _scene_inputs(C, S, fh, fw, img_w, img_h, views, seed, kinds)
        self.kinds = sc["kinds"]
        self.x = sc["x"].to(DEV)                                        # (V, C, hw)
        self.xt = self.x.transpose(1, 2).contiguous()                   # (V, hw, C)
        self.bps = (sc["bps"] if bps is None else bps).to(DEV).contiguous()
        self.centre = (sc["centre"] if centre is None else centre).to(DEV).contiguous()
        self.intr, self.extr = sc["intr"].to(DEV).contiguous(), sc["extr"].to(DEV).contiguous()
        self.view_sample = sc["view_sample"].to(DEV, torch.int32).contiguous()
        self.offs = torch.tensor([0] + torch.tensor(views).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
        self.inv = torch.empty(self.V, 16, device=DEV)
        _call("poem_launch_invert_extr", self.extr.data_ptr(), self.inv.data_ptr(), self.V)
        self.tw = torch.empty(self.V, S, 4, device=DEV)
        self.to = torch.empty(self.V, S, 2, dtype=torch.int32, device=DEV)
        self.uv = torch.empty(self.V, S, 2, device=DEV)
        _call("poem_launch_project_table", self.bps.data_ptr(), self.centre.data_ptr(), self.view_sample.data_ptr(), self.intr.data_ptr(),
              self.inv.data_ptr(), self.tw.data_ptr(), self.to.data_ptr(), self.uv.data_ptr(), self.V, C, fh, fw, S, img_w, img_h)
        torch.cuda.synchronize()
        self.pix = sf.unpack_tabo(self.to)


class _Batch:
    """samples `ids` of a scene (repeats allowed), their views gathered back to back"""

    def __init__(self, scene, ids=None):
        sc = self.scene = scene
        self.ids = list(range(sc.B)) if ids is None else list(ids)
        self.views = [sc.views[i] for i in self.ids]
        offs = sc.offs.tolist()
        self.vid = torch.tensor([v for i in self.ids for v in range(offs[i], offs[i + 1])], device=DEV)
        self.V, self.B = int(self.vid.numel()), len(self.ids)
        self.offs = torch.tensor([0] + torch.tensor(self.views).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
        self.view_sample = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.views)).to(DEV, torch.int32)


def _run_fused(batch, W, form="two", h2_tiled=1, xcd=1, views_dev=True, count=None, cap=None, gmin=1, xt=None, finite=True):
    """sample_group (form "grouped": as the forward launches the three kernels, the threshold `gmin` against the device count),
    sample_merge, merge_tail on `batch` -> dict(h2 (alloc views * S, C/2), q1, out (B, S, C), h2_views (alloc views,) bool: the
    views whose h2 rows were written).  `cap`: the capacity the launches are sized for (a.views), `count`: the count the kernels
    read from device memory; every buffer is allocated for the larger of the two."""
    sc = batch.scene
    C, S, HALF = sc.C, sc.S, sc.C // 2
    V, B = batch.V, batch.B
    cap = V if cap is None else cap
    count = V if count is None else count
    alloc = max(cap, count, V)
    pad = alloc - V
    xt_b = (sc.xt if xt is None else xt)[batch.vid]
    tw_b, to_b, vs_b = sc.tw[batch.vid], sc.to[batch.vid], batch.view_sample
    if pad:      # views past the batch: NaN planes, a valid table (pixel 0, weight 0), sample 0
        xt_b = torch.cat([xt_b, torch.full((pad, sc.hw, C), float("nan"), device=DEV)])
        tw_b = torch.cat([tw_b, torch.zeros(pad, S, 4, device=DEV)])
        to_b = torch.cat([to_b, torch.zeros(pad, S, 2, dtype=torch.int32, device=DEV)])
        vs_b = torch.cat([vs_b, torch.zeros(pad, dtype=torch.int32, device=DEV)])
    xt_b, tw_b, to_b, vs_b = xt_b.contiguous(), tw_b.contiguous(), to_b.contiguous(), vs_b.contiguous()
    cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
    h2, q1, out = _Guarded(alloc * S, HALF), _Guarded(B * S, C), _Guarded(B * S, C)
    sm = SampleMergeArgs()
    sm.xt, sm.tab, sm.tabo, sm.view_sample, sm.offs = xt_b.data_ptr(), tw_b.data_ptr(), to_b.data_ptr(), vs_b.data_ptr(), batch.offs.data_ptr()
    sm.w0, sm.b0, sm.w1, sm.b1 = W.p00.data_ptr(), W.b00.data_ptr(), W.p02.data_ptr(), W.b02.data_ptr()
    sm.h2, sm.q1 = h2.ptr, q1.ptr
    sm.views, sm.S, sm.hw, sm.B, sm.h2_tiled = cap, S, sc.hw, B, h2_tiled
    sm.views_dev = cnt.data_ptr() if views_dev else None
    # (forward.cpp: a shape the grouped kernel does not take -- NSEG % 8 != 0 -- never sets the threshold)
    group_ok = (S // C) % 8 == 0
    sm.group_min_views = gmin if (form == "grouped" and group_ok) else sf.INT_MAX
    sm.xcd_order = xcd
    mt = MergeTailArgs()
    mt.h2, mt.q1, mt.offs = h2.ptr, q1.ptr, batch.offs.data_ptr()
    mt.w0, mt.b0, mt.w1, mt.b1 = W.p10.data_ptr(), W.b10.data_ptr(), W.p12.data_ptr(), W.b12.data_ptr()
    mt.out, mt.B, mt.S, mt.h2_tiled = out.ptr, B, S, h2_tiled
    mt.group_min_views, mt.views_dev, mt.views = sm.group_min_views, sm.views_dev, cap
    what = f"C={C} S={S} hw={sc.hw} B={B} V={V} {form} tiled={h2_tiled} xcd={xcd} dev={views_dev} count={count} cap={cap} gmin={gmin}"
    if form == "grouped":
        sg = SampleGroupArgs()
        sg.sm = sm
        sg.w2, sg.b2, sg.w3, sg.b3, sg.out = mt.w0, mt.b0, mt.w1, mt.b1, out.ptr
        rc = _fn("poem_launch_sample_group")(ctypes.byref(sg), C, hip.stream())
        assert rc == (0 if group_ok else HIP_INVALID_VALUE), f"{what}: sample_group returned {rc}"
    rc = _fn("poem_launch_sample_merge")(ctypes.byref(sm), C, hip.stream())
    assert rc == 0, f"{what}: sample_merge returned {rc}"
    rc = _fn("poem_launch_merge_tail")(ctypes.byref(mt), C, hip.stream())
    assert rc == 0, f"{what}: merge_tail returned {rc}"
    torch.cuda.synchronize()
    res = dict(h2=h2.take(what + " h2"), q1=q1.take(what + " q1").view(B, S, C), out=out.take(what + " out").view(B, S, C), what=what)
    written = (_bits(res["h2"]) != _CANARY).view(alloc, S * HALF)
    res["h2_views"] = written.all(1)
    assert bool((written.all(1) | ~written.any(1)).all()), f"{what}: a view's h2 rows are partly written"
    if finite:
        assert bool(torch.isfinite(res["q1"]).all()) and bool(torch.isfinite(res["out"]).all()), f"{what}: a row of the batch is not finite"
    return res


def _run_operator(batch, W, x=None):
    """The operator sequence of forward.cpp on `batch`: project_uv, grid_sample, two GEMMs, merge_reduce, two GEMMs,
    merge_finalize -> dict(g (V, C, S), uv, h2 (row-major), out)"""
    sc = batch.scene
    C, S, V, B = sc.C, sc.S, batch.V, batch.B
    xb = (sc.x if x is None else x)[batch.vid].contiguous()
    intr, extr = sc.intr[batch.vid].contiguous(), sc.extr[batch.vid].contiguous()
    centre = sc.centre[torch.tensor(batch.ids, device=DEV)].contiguous()
    inv, uv = torch.empty(V, 16, device=DEV), torch.empty(V, S, 2, device=DEV)
    g = torch.empty(V, C, S, device=DEV)
    _call("poem_launch_project_uv", sc.bps.data_ptr(), centre.data_ptr(), batch.view_sample.data_ptr(), intr.data_ptr(), extr.data_ptr(),
          inv.data_ptr(), uv.data_ptr(), V, sc.fh, sc.fw, S, sc.img[0], sc.img[1])
    _call("poem_launch_grid_sample", xb.data_ptr(), uv.data_ptr(), g.data_ptr(), V, C, sc.fh, sc.fw, S)
    h1 = hip.gemm(g.view(V * S, C), W.p00, C, bias=W.b00, act=hip.ACT_RELU)
    h2 = hip.gemm(h1, W.p02, C // 2, bias=W.b02)
    m = torch.empty(B * S, C // 2, device=DEV)
    _call("poem_launch_merge_reduce", h2.data_ptr(), batch.offs.data_ptr(), m.data_ptr(), B, S, C // 2)
    y = hip.gemm(hip.gemm(m, W.p10, C // 2, bias=W.b10, act=hip.ACT_RELU), W.p12, C, bias=W.b12)
    out = torch.empty(B, S, C, device=DEV)
    _call("poem_launch_merge_finalize", g.data_ptr(), y.data_ptr(), batch.offs.data_ptr(), out.data_ptr(), B, S, C)
    torch.cuda.synchronize()
    return dict(g=g, uv=uv, h2=h2, out=out)


def _g_q1(g, views, S):
    """the n = 0 rows of the Q1 view of g (V, C, S) -> (B, S, C)"""
    C, rows, off, out = g.shape[1], g.reshape(-1, g.shape[1]), 0, []
    for N in views:
        out.append(rows[off * S:(off + N) * S].view(S, N, C)[:, 0])
        off += N
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------------------------
# canonical launch and references of a shape, shared by its tests
_CANON = {}
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _CANON.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


_MAPS = {"4x8": (4, 8, 256, 256), "16x16": (16, 16, 256, 256), "8x24": (8, 24, 384, 128)}


def _canon(C, S, mp):
    key = (C, S, mp)
    if key not in _CANON:
        fh, fw, iw, ih = _MAPS[mp]
        sc = _Scene(C, S, fh, fw, iw, ih, CANON_VIEWS, seed=1000 + C + S + fh)
        W = _Packed(C, seed=C)
        batch = _Batch(sc)
        two = _run_fused(batch, W)
        assert bool(two["h2_views"].all())
        _CANON[key] = dict(sc=sc, W=W, batch=batch, two=two)
    return _CANON[key]


def _refs(cn):
    """fp64 and fp32 restatements of the canonical batch from the cameras (computed once)"""
    if "r64" not in cn:
        sc, W = cn["sc"], cn["W"]
        a = (sc.x, sc.bps, sc.centre, sc.view_sample, sc.intr, sc.extr, sc.fh, sc.fw, sc.img[0], sc.img[1], sc.views, W)
        r64, r32 = sf.stage_from_coordinates(*a), sf.stage_from_coordinates(*a, fp32=True)
        cn["r64"] = {k: r64[k] for k in ("q1", "out")}
        cn["r32"] = {k: r32[k] for k in ("q1", "out")}
    return cn["r64"], cn["r32"]


def _assert_end_to_end(got, cn, form):
    """|HIP - fp64| <= 4 |fp32 - fp64| + 1e-6 max|fp64| per sample, on the edge points and on the others"""
    sc = cn["sc"]
    r64, r32 = _refs(cn)
    worst = 0.0
    for k in ("q1", "out"):
        for b, N in enumerate(sc.views):
            edge = sf.edge_points(N, sc.C, sc.S, DEV)
            for name, sel in (("edge", edge), ("inner", ~edge)):
                if not bool(sel.any()):
                    continue
                g, a, f = got[k][b][sel].double(), r64[k][b][sel], r32[k][b][sel].double()
                assert bool(torch.isfinite(g).all()), f"{form} {k} sample {b} {name}: non-finite"
                e, e32 = float((g - a).abs().max()), float((f - a).abs().max())
                bar = 4 * e32 + 1e-6 * float(a.abs().max())
                worst = max(worst, e / max(e32, 1e-300))
                assert e <= bar, (f"C={sc.C} S={sc.S} hw={sc.hw} {form} {k} sample {b} (N={N}) {name} points: |hip - fp64| = {e:.3e} > "
                                  f"4 |fp32 - fp64| + floor = {bar:.3e} (fp32: {e32:.3e})")
    _RATIOS[(sc.C, sc.S, sc.hw, form)] = worst
    print(f"sampling e2e ratio C={sc.C} S={sc.S} hw={sc.hw} {form}: max |hip - fp64| / |fp32 - fp64| = {worst:.3f}")


def _lin_bound(x_abs, ex, w, b, K):
    """a-priori bound of fl(x W^T + b) against the exact product of the exact x, |x_hat - x| <= ex"""
    wa = w.double().abs().T
    return ex @ wa + 2 * (K + 2) * sf.U32 * ((x_abs + ex) @ wa + b.double().abs())


def _assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = err > bound + 1e-30
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst {float((err / (bound + 1e-30)).max()):.2f} x the bound"


def _assert_stage_local(cn, got):
    """item 2 of the module docstring, on the kernel's own table, h2 and q1"""
    sc, W = cn["sc"], cn["W"]
    C, S, V, HALF = sc.C, sc.S, sc.V, sc.C // 2
    what = f"C={C} S={S} hw={sc.hw}"
    x64, tw = sc.x.double(), sc.tw.double()
    g64 = sf.sample_table(x64, tw, sc.pix)
    eg = 4 * sf.U32 * 1.0001 * sf.sample_table(x64, tw, sc.pix, absolute=True)
    _assert_within(got["q1"], _g_q1(g64, sc.views, S), _g_q1(eg, sc.views, S), what + " q1 against its own table")
    rows, er = g64.reshape(V * S, C), eg.reshape(V * S, C)
    a1 = rows @ W.w00.double().T + W.b00.double()
    e1 = _lin_bound(rows.abs(), er, W.w00, W.b00, C)
    h1 = F.relu(a1)
    ref = h1 @ W.w02.double().T + W.b02.double()
    e2 = _lin_bound(h1, e1, W.w02, W.b02, C)
    h2 = got["h2"][sf.h2_permutation(V, C, S, DEV)]          # row-major Q1 rows
    _assert_within(h2, ref, e2, what + " h2 against merge_net[0] of its own table's rows")
    del rows, er, a1, e1, h1, ref, e2, g64, eg
    off = 0
    for b, N in enumerate(sc.views):
        h = h2[off * S:(off + N) * S].double().view(S, N, HALF)
        m = sf.reduce_views(h)
        if N > 1:
            D = (h[:, 1:].abs() * h[:, :1].abs()).sum(-1, keepdim=True)
            em = (HALF + N - 1) * sf.U32 * 1.01 * (D * h[:, 1:].abs()).sum(1)
        else:
            em = torch.zeros_like(m)
        a3 = m @ W.w10.double().T + W.b10.double()
        e3 = _lin_bound(m.abs(), em, W.w10, W.b10, HALF)
        h3 = F.relu(a3)
        y = h3 @ W.w12.double().T + W.b12.double()
        ey = _lin_bound(h3, e3, W.w12, W.b12, HALF)
        q1 = got["q1"][b].double()
        bound = ey / N + 2 * sf.U32 * (q1.abs() + (y.abs() + ey) / N)
        _assert_within(got["out"][b], q1 + y / N, bound, what + f" out of sample {b} (N={N}) against the merge of its own h2 and q1")
        off += N


def _assert_q1_against_operator_g(cn, two, op):
    """The fused kernels' sampled values (q1) against the operator sequence's g read through the Q1 view at n = 0.  Both are the
    four-term sum nw, ne, sw, se of the same taps and the same weights, but not the same chain: the fused kernels write it with
    explicit fmaf (nw product rounded, three fused steps), grid_sample_kernel leaves the contraction to the compiler, which rounds
    the ne product and fuses the nw one onto it.  Bit equality does not hold (measured on the MI355X, LABNOTES: about 15 % of the
    elements differ, by one ulp, rarely two); what holds for either is the four-term bound 4 u sum |w| |tap| against fp64 of the same table --
    q1 in _assert_stage_local, g here -- and so twice it between them."""
    sc = cn["sc"]
    x64, tw = sc.x.double(), sc.tw.double()
    eg = 4 * sf.U32 * 1.0001 * sf.sample_table(x64, tw, sc.pix, absolute=True)
    what = f"C={sc.C} S={sc.S} hw={sc.hw}"
    _assert_within(op["g"], sf.sample_table(x64, tw, sc.pix), eg, what + " operator g against its own table")
    gq = _g_q1(op["g"], sc.views, sc.S)
    _assert_within(two["q1"], gq.double(), 2 * _g_q1(eg, sc.views, sc.S), what + " fused q1 against the operator sequence's g")
    ne = _bits(two["q1"]) != _bits(gq)
    print(f"sampling q1 / g {what}: {int(ne.sum())} of {ne.numel()} elements differ, max |q1 - g| = "
          f"{float((two['q1'] - gq).abs().max()):.3e} at max|g| = {float(gq.abs().max()):.3f}")


# shapes (C, S) of the issue's table with a map each; C = 128, S = 1024 on every map
SHAPES = [(128, 128, "4x8"), (128, 1024, "16x16"), (128, 1024, "4x8"), (128, 1024, "8x24"), (128, 2048, "8x24"), (256, 256, "8x24"),
          (256, 2048, "4x8"), (512, 512, "16x16"), (512, 4096, "4x8")]
GROUP_SHAPE = {128: (128, 1024, "4x8"), 256: (256, 2048, "4x8"), 512: (512, 4096, "4x8")}      # smallest S with NSEG % 8 == 0
SMALL_SHAPE = {128: (128, 128, "4x8"), 256: (256, 256, "8x24"), 512: (512, 512, "16x16")}      # NSEG = 1


def _same(got, want, what):
    if not torch.equal(_bits(got), _bits(want)):
        rows = (_bits(got) != _bits(want)).flatten(1).any(1).nonzero().flatten()
        pytest.fail(f"{what}: {rows.numel()} of {got.shape[0]} blocks differ, first {rows[:8].tolist()}")


def _assert_same_as_canon(res, batch, cn, what, grouped=False):
    """every sample's q1 / out rows and every view's h2 rows are the canonical launch's (where written: the grouped kernel keeps
    the h2 rows of the samples it takes on the chip)"""
    two, ids = cn["two"], torch.tensor(batch.ids, device=DEV)
    sc = cn["sc"]
    _same(res["out"], two["out"][ids], what + " out")
    _same(res["q1"], two["q1"][ids], what + " q1")
    hv = res["h2"].view(-1, sc.S * sc.C // 2)[:batch.V]
    want = two["h2"].view(sc.V, -1)[batch.vid]
    n8 = torch.tensor([N in (1, 2, 4, 8) for N in batch.views], device=DEV)[batch.view_sample.long()]
    expect = ~n8 if grouped else torch.ones_like(n8)
    assert torch.equal(res["h2_views"][:batch.V], expect), f"{what}: the views with h2 rows are not the ones expected"
    assert not bool(res["h2_views"][batch.V:].any()), f"{what}: h2 rows of views past the batch were written"
    _same(hv[expect], want[expect], what + " h2")


# =====================================================================================================================
@gpu
def test_supported_shapes_table(ncu):
    """poem_sample_merge_supported: the chain widths, S a multiple of C and of 64, at most 65536 pixels"""
    ok = _fn("poem_sample_merge_supported")
    table = [((128, 128, 32), 1), ((128, 4096, 256), 1), ((256, 256, 1024), 1), ((512, 512, 192), 1), ((512, 4096, 256), 1),
             ((128, 128 * 3 + 64, 256), 0),      # S not a multiple of C
             ((128, 200, 256), 0),
             ((128, 128, 65536), 1), ((128, 128, 65537), 0),
             ((64, 4096, 256), 0), ((32, 4096, 256), 0), ((384, 384 * 8, 256), 0)]
    for args, want in table:
        assert ok(*args) == want, (args, want)
    # S a multiple of C but not of 64 does not exist at these widths (64 | C): the S % 64 term only backs S % C up
    assert all(C % 64 == 0 for C in (128, 256, 512))


@gpu
@pytest.mark.parametrize("mp", list(_MAPS))
def test_tables(mp, ncu):
    """project_table: weights / pixels bit-equal to the fp32 function of its own (ix, iy), (ix, iy) under the end-to-end bar per
    view; input_tables: bit-equal tables (invert_extr's inverse, centre = reference_joints[:, 9]) and prep_xyz's outputs.  Views
    inside the image, straddling every border (0, 1, 2 and 4 valid corners), behind the camera and with q_z = 0."""
    fh, fw, iw, ih = _MAPS[mp]
    S, Q, views = 1000, 50, [1, 3, 2, 4]
    kinds = ["inside", "straddle", "behind", "clamp", "straddle", "inside", "straddle", "behind", "straddle", "clamp"]
    g = torch.Generator().manual_seed(5)
    rj = (torch.randn(len(views), 21, 3, generator=g) * 0.02).to(DEV)
    sc = _Scene(128, S, fh, fw, iw, ih, views, seed=77, kinds=kinds, centre=rj[:, 9].cpu())
    ix, iy = sc.uv[..., 0], sc.uv[..., 1]
    w_exp, pix_exp = sf.table_from_ixiy(ix, iy, fh, fw)
    assert torch.equal(_bits(sc.tw), _bits(w_exp)), "weights are not the fp32 function of (ix, iy)"
    in_range = (ix.abs() < 2.0 ** 30) & (iy.abs() < 2.0 ** 30)
    assert torch.equal(sc.pix[in_range], pix_exp[in_range]), "tap pixels are not the fp32 function of (ix, iy)"
    assert int(sc.pix.max()) < fh * fw and bool((sc.tw[~in_range] == 0).all())
    corners = (sc.tw != 0).sum(-1)
    strad = torch.tensor([k == "straddle" for k in kinds], device=DEV)
    assert {0, 1, 2, 4} <= {int(c) for c in corners[strad].unique()}, "the straddling views miss a kind of border point"
    clamp = torch.tensor([k == "clamp" for k in kinds], device=DEV)
    assert bool((corners[clamp] == 0).all()) and bool((ix[clamp].abs() > 1e6).all())
    assert bool((corners[torch.tensor([k == "inside" for k in kinds], device=DEV)] == 4).any())
    a = (sc.bps, sc.centre, sc.view_sample, sc.intr, sc.extr, fh, fw, iw, ih)
    r64 = sf.project_ixiy(*a)
    r32 = sf.project_ixiy(*a, dtype=torch.float32, inv=torch.linalg.inv(sc.extr.double()).float())
    for name, got, a64, a32 in (("ix", ix, r64[0], r32[0]), ("iy", iy, r64[1], r32[1])):
        for v in range(sc.V):
            e, e32 = float((got[v].double() - a64[v]).abs().max()), float((a32[v].double() - a64[v]).abs().max())
            bar = 4 * e32 + 1e-6 * float(a64[v].abs().max())
            assert e <= bar, f"{name} view {v} ({kinds[v]}): |hip - fp64| = {e:.3e} > {bar:.3e} (fp32: {e32:.3e})"
    # input_tables
    tmpl = torch.randn(Q, 3, generator=g).mul(0.05).to(DEV)
    tw2, to2 = torch.empty_like(sc.tw), torch.empty_like(sc.to)
    B = sc.B
    outs = [[torch.full((n,), float("nan"), device=DEV) for n in (B * 3, B * S * 3, B * Q * 3)] for _ in range(2)]
    _call("poem_launch_input_tables", sc.bps.data_ptr(), rj.data_ptr(), tmpl.data_ptr(), sc.view_sample.data_ptr(), sc.intr.data_ptr(),
          sc.extr.data_ptr(), tw2.data_ptr(), to2.data_ptr(), outs[0][0].data_ptr(), outs[0][1].data_ptr(), outs[0][2].data_ptr(), sc.V, B, S, Q,
          fh, fw, iw, ih, 0.1)
    _call("poem_launch_prep_xyz", rj.data_ptr(), sc.bps.data_ptr(), tmpl.data_ptr(), outs[1][0].data_ptr(), outs[1][1].data_ptr(),
          outs[1][2].data_ptr(), B, S, Q, 0.1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(tw2), _bits(sc.tw)) and torch.equal(to2, sc.to), "input_tables' tables differ from project_table's"
    for a_, b_, name in zip(outs[0], outs[1], ("centre", "pt_xyz", "query_xyz")):
        assert bool(torch.isfinite(a_).all()) and torch.equal(_bits(a_), _bits(b_)), name
    assert torch.equal(outs[0][0].view(B, 3), rj[:, 9])


@gpu
@pytest.mark.parametrize("C,S,mp", SHAPES)
def test_stage_accuracy_in_every_form(C, S, mp, ncu):
    """The canonical batch in the two-kernel form: sentinels, stage-local bounds, the end-to-end bar; the grouped form (threshold
    1: every N | 8 sample grouped) bit-equal to it where the shape offers it, refused where it does not; the operator sequence
    under the same bar, its sampled tensor g -- read through the Q1 view at n = 0 -- against the fused q1
    (_assert_q1_against_operator_g: within the four-term bound; the two are not the same chain)."""
    cn = _canon(C, S, mp)
    sc, W, batch, two = cn["sc"], cn["W"], cn["batch"], cn["two"]
    _assert_stage_local(cn, two)
    _assert_end_to_end(two, cn, "two-kernel")
    grp = _run_fused(batch, W, form="grouped", gmin=1)
    if (S // C) % 8 == 0:
        _assert_same_as_canon(grp, batch, cn, f"C={C} S={S} grouped", grouped=True)
        _assert_end_to_end(grp, cn, "grouped")
    else:      # the launcher refused (asserted in _run_fused): everything went through the other two kernels
        _assert_same_as_canon(grp, batch, cn, f"C={C} S={S} grouped refused", grouped=False)
    op = _run_operator(batch, W)
    _assert_end_to_end(dict(q1=_g_q1(op["g"], sc.views, S), out=op["out"]), cn, "operator")
    assert torch.equal(_bits(op["uv"]), _bits(sc.uv)), "project_uv and project_table disagree on (ix, iy)"
    _assert_q1_against_operator_g(cn, two, op)


@gpu
def test_batches_reach_every_grid_cell(ncu):
    """The batches of test_rows_do_not_depend_on_the_batch, through the mirror of merge.hip's launch arithmetic, reach every
    (kernel, C, cell) -- work items below the persistent grid's limit, equal to it, one view / sample above it, a little above
    twice it -- that the device's CU count allows."""
    reached = set()
    for C in (128, 256, 512):
        for kern, (Cx, S, _), batches in _cell_batches(C, ncu):
            for ids in batches:
                views = sum(CANON_VIEWS[i] for i in ids)
                cell = sf.grid_cell(kern, Cx, S, views, len(ids), ncu)
                if cell:
                    reached.add((kern, C, cell))
    want = {(k, C, cell) for C in (128, 256, 512) for k, shp in (("sample_merge", SMALL_SHAPE[C]), ("merge_tail", SMALL_SHAPE[C]),
                                                                   ("sample_group", GROUP_SHAPE[C]))
            for cell in sf.cell_counts(k, shp[0], shp[1], ncu)}
    print("sampling grid cells reached:", sorted(reached))
    assert want - reached == set(), f"cells no batch reaches: {sorted(want - reached)}"
    assert {c for _, _, c in want} == set(sf.CELLS) or ncu % 8, sorted(want)


def _ids_for_views(T):
    """samples of the canonical batch with T views in all: the ragged head as far as it fits, then single-view fillers"""
    ids, v = [], 0
    for i, N in enumerate(HEAD):
        if v + N <= T:
            ids.append(i)
            v += N
    k = 0
    while v < T:
        ids.append(len(HEAD) + k % NPROTO1)
        k, v = k + 1, v + 1
    return ids


def _ids_for_samples(Bt):
    return list(range(min(Bt, len(HEAD)))) + [len(HEAD) + k % NPROTO1 for k in range(max(0, Bt - len(HEAD)))]


def _cell_batches(C, ncu):
    """[(kernel, shape, [sample ids of a batch, ...])]: per kernel the batches that put its work items in each grid cell"""
    out = []
    for kern, shp in (("sample_merge", SMALL_SHAPE[C]), ("merge_tail", SMALL_SHAPE[C]), ("sample_group", GROUP_SHAPE[C])):
        counts = sf.cell_counts(kern, shp[0], shp[1], ncu)
        mk = _ids_for_samples if kern == "merge_tail" else _ids_for_views
        out.append((kern, shp, [mk(n) for n in counts.values()]))
    return out


@gpu
@pytest.mark.parametrize("C", [128, 256, 512])
def test_rows_do_not_depend_on_the_batch(C, ncu):
    """A sample's rows are the same bits whatever batch it sits in and wherever: batches that put each kernel's work items below,
    at, just above and above twice the persistent grid (second and third trips of the persistent loops on small problems), in
    the two-kernel form and, at the grouped shape, in the grouped form; a batch in reverse order."""
    for kern, shp, batches in _cell_batches(C, ncu):
        cn = _canon(*shp)
        for ids in batches:
            batch = _Batch(cn["sc"], ids)
            what = f"C={C} S={shp[1]} {kern} cell batch B={batch.B} V={batch.V}"
            if kern == "sample_group":
                _assert_same_as_canon(_run_fused(batch, cn["W"], form="grouped", gmin=1), batch, cn, what + " grouped", grouped=True)
            else:
                _assert_same_as_canon(_run_fused(batch, cn["W"]), batch, cn, what)
            del batch
    for shp in (SMALL_SHAPE[C], GROUP_SHAPE[C]):
        cn = _canon(*shp)
        batch = _Batch(cn["sc"], list(reversed(range(len(CANON_VIEWS)))) + [4, 4, 1])
        for form in ("two", "grouped"):
            if form == "grouped" and shp is SMALL_SHAPE[C]:
                continue
            _assert_same_as_canon(_run_fused(batch, cn["W"], form=form, gmin=1), batch, cn, f"C={C} S={shp[1]} reversed {form}",
                                  grouped=form == "grouped")


@gpu
@pytest.mark.parametrize("C", [128, 256, 512])
def test_bit_identical_forms(C, ncu):
    """merge.hip's claims, at both S with NSEG % 8 == 0 where the grouped kernel is involved: xcd_order 0 = 1 (grid a multiple of
    8 and not), h2_tiled 0 = 1 after merge_tail with h2 itself the stated permutation, views_dev = nullptr = views_dev -> views,
    the threshold at count = group_min_views - 1 and = group_min_views, and batches of only N | 8, of no N | 8 and mixed."""
    shapes = [GROUP_SHAPE[C]] + ([(128, 2048, "8x24")] if C == 128 else [])
    for shp in shapes:
        cn = _canon(*shp)
        sc, W, full = cn["sc"], cn["W"], cn["batch"]
        S = shp[1]
        upv = sf.launch_shape("sample_group", C, S, 1, 1, ncu)[1]
        # xcd_order: grids of 8 k and not (units = views * upv, below the grid limit), and the full batch
        n8 = [i for i, N in enumerate(CANON_VIEWS) if N == 1]
        grids = set()
        for ids in ([n8[k % len(n8)] for k in range(8)], [n8[k % len(n8)] for k in range(5)] + [2], None):
            batch = full if ids is None else _Batch(sc, ids)
            units = batch.V * upv
            grids.add(min(units, 2 * ncu) % 8 == 0)
            for xcd in (0, 1):
                res = _run_fused(batch, W, form="grouped", gmin=1, xcd=xcd)
                _assert_same_as_canon(res, batch, cn, f"C={C} S={S} xcd_order={xcd} units={units}", grouped=True)
        assert grids == ({True} if upv % 8 == 0 and ncu % 4 == 0 else {True, False}), (C, S, grids)      # (C = 512: 16 units per view)
        # the threshold, against the device count
        for gmin, grouped in ((sc.V + 1, False), (sc.V, True)):
            res = _run_fused(full, W, form="grouped", gmin=gmin)
            _assert_same_as_canon(res, full, cn, f"C={C} S={S} count={sc.V} group_min_views={gmin}", grouped=grouped)
        # only N | 8 (the other two kernels return early: no h2 row at all), no N | 8, mixed (the canonical batch itself, above)
        for ids in ([0, 2, 4, 6, 10, 11], [1, 3, 5, 7, 8, 9]):
            batch = _Batch(sc, ids)
            res = _run_fused(batch, W, form="grouped", gmin=1)
            _assert_same_as_canon(res, batch, cn, f"C={C} S={S} samples {ids} grouped", grouped=True)
    for shp in (SMALL_SHAPE[C], GROUP_SHAPE[C]):
        cn = _canon(*shp)
        sc, W, full, two = cn["sc"], cn["W"], cn["batch"], cn["two"]
        row = _run_fused(full, W, h2_tiled=0)
        _same(row["out"], two["out"], f"C={C} S={shp[1]} h2_tiled=0 out")
        _same(row["q1"], two["q1"], f"C={C} S={shp[1]} h2_tiled=0 q1")
        assert torch.equal(_bits(two["h2"][sf.h2_permutation(sc.V, C, shp[1], DEV)]), _bits(row["h2"])), "h2 layouts: not the stated permutation"
        null = _run_fused(full, W, views_dev=False)
        _assert_same_as_canon(null, full, cn, f"C={C} S={shp[1]} views_dev=nullptr")
        # ... which also switches the grouped kernel off, whatever the threshold
        null = _run_fused(full, W, form="grouped", gmin=1, views_dev=False)
        _assert_same_as_canon(null, full, cn, f"C={C} S={shp[1]} views_dev=nullptr, threshold 1")


@gpu
def test_sample_scan_past_one_block(ncu):
    """300 samples at C = 128 (256 threads per block), all single-view but the last (N = 3): the `for (b = tid; b < B; ...)` scans
    of sample_merge / merge_tail must see it on their second trip, or they return early and its rows keep the sentinel."""
    cn = _canon(128, 1024, "4x8")
    ids = [len(HEAD) + k % NPROTO1 for k in range(299)] + [1]
    batch = _Batch(cn["sc"], ids)
    assert batch.B == 300 and batch.views[-1] == 3 and set(batch.views[:-1]) == {1}
    for form in ("grouped", "two"):
        res = _run_fused(batch, cn["W"], form=form, gmin=1)
        _assert_same_as_canon(res, batch, cn, f"B=300 {form}", grouped=form == "grouped")


@gpu
@pytest.mark.parametrize("C", [128, 256, 512])
def test_device_view_count_against_the_capacity(C, ncu):
    """The count the kernels read from device memory, below and ABOVE the capacity the launches are sized for (every buffer is
    allocated for the larger one, so a missing clamp shows as overwritten sentinels): below -- the rows of the views past the
    count keep their sentinel; above -- only the capacity's views are sampled: with the capacity at a sample boundary, the h2 and
    q1 rows of the last sample keep their sentinel, its out rows are not finite (merge_tail walks the B samples of the host
    argument and meets the unwritten h2 rows), every other sample is the clean launch's."""
    for shp, forms in ((SMALL_SHAPE[C], ("two",)), (GROUP_SHAPE[C], ("two", "grouped"))):
        cn = _canon(*shp)
        sc, W, two = cn["sc"], cn["W"], cn["two"]
        ids = list(range(len(HEAD))) + [10, 3]          # the last sample: N = 5
        batch = _Batch(sc, ids)
        for form in forms:
            grouped = form == "grouped"
            res = _run_fused(batch, W, form=form, gmin=1, cap=batch.V + 3)
            _assert_same_as_canon(res, batch, cn, f"C={C} S={shp[1]} {form} count below the capacity", grouped=grouped)
            nlast = batch.views[-1]
            cap = batch.V - nlast
            res = _run_fused(batch, W, form=form, gmin=1, cap=cap, count=batch.V, finite=False)
            what = f"C={C} S={shp[1]} {form} count {batch.V} above the capacity {cap}"
            assert not bool(res["h2_views"][cap:].any()), f"{what}: h2 rows of views past the capacity were written"
            assert bool((_bits(res["q1"][-1]) == _CANARY).all()), f"{what}: q1 rows of the sample past the capacity were written"
            assert not bool(torch.isfinite(res["out"][-1]).any()), f"{what}: finite out rows from unwritten h2 rows"
            head = torch.tensor(ids[:-1], device=DEV)
            _same(res["out"][:-1], two["out"][head], what + " out")
            _same(res["q1"][:-1], two["q1"][head], what + " q1")
            n8 = torch.tensor([N in (1, 2, 4, 8) for N in batch.views], device=DEV)[batch.view_sample.long()][:cap]
            assert torch.equal(res["h2_views"][:cap], ~n8 if grouped else torch.ones_like(n8)), what


@gpu
@pytest.mark.parametrize("C", [128, 256, 512])
def test_nan_view_stays_in_its_rows(C, ncu):
    """One view of NaN planes in a single-view sample and one in a three-view sample: the rows of those samples that the
    restatement makes NaN (module docstring) are NaN, every other row of the batch is the clean launch's, bit for bit -- in the
    two-kernel, the grouped and the operator form."""
    for shp in (SMALL_SHAPE[C], GROUP_SHAPE[C]):
        cn = _canon(*shp)
        sc, W, batch, two = cn["sc"], cn["W"], cn["batch"], cn["two"]
        S = shp[1]
        offs = sc.offs.tolist()
        bad_views = [offs[0], offs[1] + 1]            # sample 0 (N = 1), view 1 of sample 1 (N = 3)
        x = sc.x.clone()
        x[bad_views] = float("nan")
        xt = x.transpose(1, 2).contiguous()
        nan_rows = torch.zeros(sc.B, S, dtype=torch.bool, device=DEV)
        nan_rows[0] = True
        r = torch.arange(3 * S, device=DEV)
        nan_rows[1] = ((r // S) == 1).view(S, 3).any(1)
        clean_op = _run_operator(batch, W)
        for form in ("two", "grouped", "operator"):
            if form == "grouped" and (S // C) % 8:
                continue
            if form == "operator":
                got, want = _run_operator(batch, W, x=x)["out"], clean_op["out"]
            else:
                got, want = _run_fused(batch, W, form=form, gmin=1, xt=xt, finite=False)["out"], two["out"]
            what = f"C={C} S={S} {form} NaN views {bad_views}"
            assert bool(torch.isnan(got[nan_rows]).all()), f"{what}: a row fed by the NaN view has finite outputs"
            assert torch.equal(_bits(got[~nan_rows]), _bits(want[~nan_rows])), f"{what}: other rows changed"


@gpu
def test_map_of_65536_pixels_all_four_corners(ncu):
    """hw = 65536 (256 x 256), the top of the 16-bit tap pixels, C = 128, two views: the first points are aimed at the four
    corners of view 0 (identity camera), so that pixel 65535 and the high halves of both tap dwords carry weight; stage-local and
    end-to-end bars, and the operator sequence (grid_sample's unstaged form) with bit-equal sampled values."""
    C, S, fh, fw = 128, 128, 256, 256
    d, f = 0.5, 2.0 * fw
    targets = [(-0.3, -0.4), (0.4, 0.2), (254.7, 254.6), (255.3, 255.4), (255.2, -0.2), (-0.4, 255.3), (254.5, 0.5), (0.5, 254.5),
               (255.0, 255.0), (254.999, 254.999), (-1.2, 100.0), (256.3, 256.1), (254.6, 255.2), (255.2, 254.7), (-0.3, 0.3), (0.3, -0.4)]
    bps = sf.make_points(S, 9)
    for k, (ix, iy) in enumerate(targets):          # img = map: ix = u - 0.5, u = f x / d + 128
        bps[k] = torch.tensor([(ix + 0.5 - 128.0) * d / f, (iy + 0.5 - 128.0) * d / f, 0.0])
    intr, extr = sf.make_cameras(["inside", "straddle"], fw, fh, 3)
    intr[0] = torch.tensor([[f, 0, 128.0], [0, f, 128.0], [0, 0, 1]])
    extr[0] = torch.eye(4)
    extr[0, 2, 3] = -d                               # p_cam = p_master + (0, 0, d)
    sc = _Scene(C, S, fh, fw, fw, fh, [2], seed=65, bps=bps, centre=torch.zeros(1, 3))
    sc.intr, sc.extr = intr.to(DEV).contiguous(), extr.to(DEV).contiguous()
    _call("poem_launch_invert_extr", sc.extr.data_ptr(), sc.inv.data_ptr(), sc.V)
    _call("poem_launch_project_table", sc.bps.data_ptr(), sc.centre.data_ptr(), sc.view_sample.data_ptr(), sc.intr.data_ptr(),
          sc.inv.data_ptr(), sc.tw.data_ptr(), sc.to.data_ptr(), sc.uv.data_ptr(), sc.V, C, fh, fw, S, fw, fh)
    torch.cuda.synchronize()
    sc.pix = sf.unpack_tabo(sc.to)
    t0w, t0p = sc.tw[0, :len(targets)], sc.pix[0, :len(targets)]
    for k in range(4):      # every tap slot (low and high halves of both dwords) reaches the last pixel and pixel 0 with weight
        assert bool(((t0p[:, k] == 65535) & (t0w[:, k] > 0)).any()), f"tap {k} never reads pixel 65535"
        assert bool(((t0p[:, k] == 0) & (t0w[:, k] > 0)).any()), f"tap {k} never reads pixel 0"
    assert float(sc.uv[0, 3, 0]) > 255.0 and float(sc.uv[0, 0, 0]) < 0.0
    assert _fn("poem_sample_merge_supported")(C, S, fh * fw) == 1
    W = _Packed(C, seed=C)
    batch = _Batch(sc)
    two = _run_fused(batch, W)
    cn = dict(sc=sc, W=W, batch=batch, two=two)
    _assert_stage_local(cn, two)
    _assert_end_to_end(two, cn, "two-kernel")
    op = _run_operator(batch, W)
    _assert_end_to_end(dict(q1=_g_q1(op["g"], sc.views, S), out=op["out"]), cn, "operator")
    _assert_q1_against_operator_g(cn, two, op)


# =====================================================================================================================
# the operator sequence on maps whose staged planes do not fit in 64 KB of LDS
@gpu
@pytest.mark.parametrize("fh,fw", [(32, 64), (64, 64), (256, 256)])
def test_operator_sampling_on_large_maps(fh, fw, ncu):
    """poem_launch_grid_sample / poem_launch_project_sample at 2048 pixels (the last size whose 8 staged planes fit in 64 KB),
    4096 and 65536 (C = 32, five views, S = 256) against F.grid_sample in float64 on the kernel's own coordinates, within the
    four-term bound 4 u sum |w| |tap| plus the coordinates' own rounding (none: fp64 of the same fp32 (ix, iy))."""
    C, S, views = 32, 256, [2, 3]
    sc = _Scene(C, S, fh, fw, 256, 256, views, seed=fh + fw)
    V = sc.V
    g1, g2 = torch.full((V, C, S), float("nan"), device=DEV), torch.full((V, C, S), float("nan"), device=DEV)
    inv, uv2 = torch.empty(V, 16, device=DEV), torch.empty(V, S, 2, device=DEV)
    _call("poem_launch_grid_sample", sc.x.data_ptr(), sc.uv.data_ptr(), g1.data_ptr(), V, C, fh, fw, S)
    _call("poem_launch_project_sample", sc.x.data_ptr(), sc.bps.data_ptr(), sc.centre.data_ptr(), sc.view_sample.data_ptr(), sc.intr.data_ptr(),
          sc.extr.data_ptr(), inv.data_ptr(), uv2.data_ptr(), g2.data_ptr(), V, C, fh, fw, S, 256, 256)
    torch.cuda.synchronize()
    assert torch.equal(_bits(uv2), _bits(sc.uv)) and torch.equal(_bits(g1), _bits(g2))
    ix, iy = sc.uv[..., 0].double(), sc.uv[..., 1].double()
    grid = torch.stack([(2 * ix + 1) / fw - 1, (2 * iy + 1) / fh - 1], dim=-1)[:, :, None]       # (V, S, 1, 2)
    ref = F.grid_sample(sc.x.double().view(V, C, fh, fw), grid, mode="bilinear", padding_mode="zeros", align_corners=False)[..., 0]
    w, pix = sf.table_from_ixiy(ix, iy, fh, fw)
    # (grid -> ix inside F.grid_sample is not exact in fp64: a relative 4e-16 of the coordinate, times the plane's slope)
    bound = 4 * sf.U32 * 1.0001 * sf.sample_table(sc.x.double(), w, pix, absolute=True) + 1e-9
    _assert_within(g1, ref, bound, f"grid_sample {fh}x{fw}")
    assert float((sf.sample_table(sc.x.double(), w, pix) - ref).abs().max()) < 1e-9


@gpu
def test_grid_sample_staged_and_unstaged_forms_agree(ncu):
    """The two forms of grid_sample_kernel (planes staged in LDS / taps from global memory) are the same expression in the same
    order: bit-equal at 16 x 16 and at 2048 pixels, where both can run; the staged form refuses a map it cannot hold."""
    for fh, fw, C in ((16, 16, 32), (32, 64, 20)):
        sc = _Scene(C, 300, fh, fw, 256, 256, [3, 1], seed=fh)
        gs = [torch.full((sc.V, C, 300), float("nan"), device=DEV) for _ in range(2)]
        for staged in (0, 1):
            _call("poem_launch_grid_sample_ex", sc.x.data_ptr(), sc.uv.data_ptr(), gs[staged].data_ptr(), sc.V, C, fh, fw, 300, staged)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(gs[0]).all()) and torch.equal(_bits(gs[0]), _bits(gs[1])), (fh, fw)
    rc = _fn("poem_launch_grid_sample_ex")(sc.x.data_ptr(), sc.uv.data_ptr(), gs[0].data_ptr(), sc.V, 20, 64, 64, 300, 1, hip.stream())
    assert rc == HIP_INVALID_VALUE, rc


@gpu
def test_head_on_a_64x64_map_operator_against_fused(ncu):
    """A 64 x 64 feature map through the head: the fused front end (default) and the operator sequence (fused_sampling = 0, whose
    grid_sample cannot stage 4096-pixel planes) agree on bps_feat within the bar of test_fused_sampling_vs_operator_sequence."""
    import poem_v2_amd as pk
    from util import batch_to, build_hip_head
    views = [2, 3, 1]
    spec = dict(embed=128, nsample=1024, views=views, seed=31, parametric=False)
    b = pk.inputs.synthetic_batch(views, seed=31)
    b["mlvl_feat"] = torch.randn(sum(views), 160, 64, 64, generator=torch.Generator().manual_seed(31))
    head = build_hip_head(spec, DEV)
    feat, metas, rj = batch_to(b, DEV)
    with torch.no_grad():
        head(feat, metas, rj)                         # (the head builds its engine for the map that arrives)
    eng = head._engine
    eng.enable_taps(True)
    bf = {}
    for mode in (1, 0):
        head.set_option("fused_sampling", mode)
        with torch.no_grad():
            head(feat, metas, rj)
        bf[mode] = eng.tap("bps_feat", (len(views), 1024, 128)).cpu()
    eng.enable_taps(False)
    assert (eng.cfg.feat_h, eng.cfg.feat_w) == (64, 64)
    scale = float(bf[1].abs().max())
    assert bool(torch.isfinite(bf[0]).all()) and bool(torch.isfinite(bf[1]).all())
    assert float((bf[1] - bf[0]).abs().max()) < 1e-5 * max(scale, 1.0), (float((bf[1] - bf[0]).abs().max()), scale)
