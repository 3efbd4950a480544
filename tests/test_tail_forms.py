"""The parametric tail and the glue kernels (misc.hip: q3_flatten, rot6d_to_aa, finalize, finalize_param, param_rows, compose_weight,
compose_bias, gather_anchor_rows, pad_rows, broadcast, canon_xyz, view_layout; mano.hip: mano_prepare, mano_lbs, mano_recentre) in
every form the forward launches them, called through their launchers (the MANO kernels and the refusals through the C ABI) at the
smallest shapes at which each mechanism exists, with canary-filled guards in front of and behind every output, and held against
the restatement of tests/tail_forms_util.py (itself held against oracle/poem_oracle.py and oracle/mano_oracle.py on the CPU, first
tests below).

Bars, each derived and none measured; u = 2^-24.
  q3_flatten   |got - fp64| <= 1.01 (ceil(Q / 64) + 7) u (sum_m |x_m w_m| + |b|): a lane's chain of ceil(Q / 64) fused steps, six
               butterfly adds, one bias add (1.01: second-order terms).
  rot6d        Rodrigues(aa) in fp64 against the fp64 Gram-Schmidt matrix of the same fp32 six numbers (input rounding outside the
               bar), max entry difference, worst per rung (angle, row scale, shear) of the ladder.  Yardstick: the oracle's own fp32
               chain on the CPU on the same rung (re-measured by a CPU test: 0 at angle 0, ~1e-7 .. 1e-6 for shear <= 0.7, up to
               ~1e-5 for shear 30, independent of the scale).  Bar: 4 x the yardstick + 2^-23 (the project's fp32-against-fp64
               factor; one ulp of a unit entry where the yardstick is exactly 0), and for shear <= 0.7 never more than the flat 2e-6
               of tests/test_mano.py.  Exact: all-zero six numbers -> +0; a NaN or Inf among a joint's six numbers -> that joint's
               three outputs NaN, every other output the clean launch's bits; betas bit copies.
  finalize     bit-equal to fp32 torch nan_to_num(x) * r + c (a product and a sum, each rounded: an fma would differ) on random
               data and on data seeded with NaN, +-Inf, -0, denormals; the MANO rows bit-equal to nan_to_num(joints | verts) + c,
               without reading xyz's last layer; finalize_param the same bits; param_rows a bit copy.
  compose      |got - fp64| <= u |fp64| + Cm 2^-53 sum |a| |b|: one fp32 rounding of an fp64 sum in any order, fused or not.
  gather, pad, broadcast, canon_xyz, view_layout     bit / integer equality.
  mano table   template, D and W regions bit-equal to the restated layout, zeros in the padded columns and coefficients; J_t and
               J_sd within u |fp64| + 778 . 2^-53 sum |terms|.
  mano LBS     |HIP - fp64| <= 4 |mano_oracle fp32 - fp64| + 2^-23 max|fp64| per sample, joints and vertices separately, the
               yardstick on the CPU for the same inputs; a sample's bits do not depend on the batch or on its place in it; a NaN
               sample is NaN where the fp64 reference is and leaves every other sample's bits alone.

Measured on the MI355X (printed by the tests under `pytest -s`; tables in LABNOTES.md, "Tail forms").  rot6d, worst kernel error
over the yardstick on a rung: 1.51 (shear 0), 1.59 (0.7), 1.15 (30); worst kernel error over the bar 0.40.  LBS, worst
|HIP - fp64| / |fp32 oracle - fp64| over samples, seeds and centres: 2.95 on vertices, 3.68 on joints (where the 2^-23 floor is the
larger half of the bar); worst |HIP - fp64| over the bar 0.71."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mano_oracle as mo
import poem_oracle as po
import tail_forms_util as tf
from poem_v2_amd import hip
from poem_v2_amd.mano import synthetic_mano_assets
from util import ViewLayoutArgs

gpu = pytest.mark.gpu
DEV = "cuda:0"
POEM_E_ARG = -1
_vp, _i, _f, _l = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long


# =====================================================================================================================
# the restatement against the oracles, the ladder's conditions, the yardsticks (CPU)
def test_restatement_matches_the_oracle():
    """q3_ref against parametric_tail's first Linear; finalize_ref against head_forward's last lines (both heads); the MANO table
    read back as LBS in fp64 against mano_oracle.mano_lbs in fp64 to 1e-12 (seeds 0 and 3, every kind of centre); view_layout_ref
    against the definition, view by view."""
    g = torch.Generator().manual_seed(1)
    feats, w, b = torch.randn(2, 799, 6, generator=g), torch.randn(799, generator=g), torch.randn(1, generator=g)
    t, T = tf.q3_ref(feats, w, b)
    want = po.linear(feats.double().reshape(-1, 799), w.double()[None], b.double()).reshape(-1, 6)
    assert float((t - want).abs().max()) < 1e-12 and bool((T >= t.abs()).all())
    xyz, c = torch.randn(3, 2, 22, 3, generator=g), torch.randn(2, 3, generator=g)
    out = torch.nan_to_num(xyz)
    cc = c[None, :, None, :]
    assert torch.equal(tf.finalize_ref(xyz, c, 0.1), out * 0.1 + cc)
    verts, joints = xyz[-1, :, 21:], xyz[-1, :, :21]
    para = torch.cat([out[:-1] * 0.1 + cc, out[-1:] + cc])
    assert torch.equal(tf.finalize_mano_ref(verts, joints, c), para[-1]) and torch.equal(tf.param_rows_ref(verts, joints), xyz[-1])
    pose, betas, _ = tf.lbs_cases()
    for seed in (0, 3):
        a = synthetic_mano_assets(seed)
        tab = tf.mano_table(a)
        assert tf.table_flat32(tab).size == tf.TABLE_FLOATS
        for centre in (-1, 9, 4):
            v, j = tf.lbs_from_table(tab, pose, betas, centre)
            vo, jo = mo.mano_lbs(a, pose, betas, center_idx=centre, dtype=torch.float64)
            assert float((v - vo).abs().max()) < 1e-12 and float((j - jo).abs().max()) < 1e-12, (seed, centre)
    for name, views in tf.LAYOUT_BATCHES.items():
        offs, vs, pe = tf.view_layout_ref(views)
        assert offs[-1] == sum(views) == len(vs) and len(offs) == len(views) + 1 <= tf.LAYOUT_MAX_BATCH + 1 and offs[-1] <= 65535
        for v in {0, len(vs) // 3, len(vs) - 1}:
            s = int(np.searchsorted(offs, v, side="right")) - 1
            assert vs[v] == s and pe[v] == views[s] * (views[s] - 1) // 2 + (v - offs[s]), (name, v)
    assert sum(tf.LAYOUT_BATCHES["both_limits"]) == 65535 and len(tf.LAYOUT_BATCHES["both_limits"]) == tf.LAYOUT_MAX_BATCH


def test_view_layout_args_mirror_matches_merge_h(repo_root):
    import os
    import re
    src = open(os.path.join(repo_root, "poem-v2_amd", "csrc", "merge.h")).read()
    assert int(re.search(r"#define POEM_LAYOUT_MAX_BATCH (\d+)", src).group(1)) == tf.LAYOUT_MAX_BATCH
    body = re.sub(r"//[^\n]*", "", re.search(r"struct ViewLayoutArgs\s*\{(.*?)\};", src, re.S).group(1))
    decls = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert decls == ["int* offs", "int* view_sample", "int* pe_index", "int B", "unsigned short off16[POEM_LAYOUT_MAX_BATCH + 1]"]
    assert [n for n, _ in ViewLayoutArgs._fields_] == ["offs", "view_sample", "pe_index", "B", "off16"]
    assert ViewLayoutArgs.off16.offset == 28 and ctypes.sizeof(ViewLayoutArgs) == 3360


_LADDER = {}


def _ladder():
    if not _LADDER:
        d6, rung, rungs = tf.rot6d_ladder()
        yard = tf.rot6d_yardstick(d6, rung, len(rungs))
        _LADDER.update(d6=d6, rung=rung, rungs=rungs, yard=yard, bars=tf.rot6d_bars(yard, rungs), Rgs=tf.gram_schmidt64(d6))
    return _LADDER


def test_rot6d_ladder_conditions_and_yardstick():
    """The ladder reaches all four candidate branches and both tie patterns of the fp32 chain (q_abs = [1, 1, 1, 1] exactly:
    120 degrees about (1, 1, 1) / sqrt 3; candidates 1 and 2 exactly equal and the largest: 180 degrees about (1, 1, 0) / sqrt 2),
    and the oracle's own chain is a rotation on every tie (judged by the rotation, not by the axis sign).  The yardstick
    re-measured: 0 at angle 0, <= 2e-6 for shear <= 0.7, <= 5e-5 for shear 30, the same for the three scales to a factor 4."""
    L = _ladder()
    d6, rung, rungs, yard = L["d6"], L["rung"], L["rungs"], L["yard"]
    assert len(rungs) == 135 and d6.shape == (135 * 51, 6)
    qa = tf.q_abs32(d6)
    assert set(qa.argmax(-1).tolist()) == {0, 1, 2, 3}
    all_four = (qa == qa[:, :1]).all(-1)
    tie12 = (qa[:, 1] == qa[:, 2]) & (qa[:, 1] > qa[:, 0]) & (qa[:, 1] > qa[:, 3])
    assert int(all_four.sum()) >= 1 and bool((qa[all_four] == 1).all()), int(all_four.sum())
    assert int(tie12.sum()) >= 1, int(tie12.sum())
    ties = all_four | tie12
    aa = po.matrix_to_axis_angle(po.rotation_6d_to_matrix(d6[ties]))
    assert float(tf.rotation_error(aa, L["Rgs"][ties]).max()) < 2e-6
    by = {}
    for r, (ang, sc, mix) in enumerate(rungs):
        y = float(yard[r])
        by.setdefault((ang, mix), []).append(y)
        if ang == 0.0:
            assert y == 0.0, (ang, sc, mix, y)
        assert y <= (2e-6 if mix <= 0.7 else 5e-5), (ang, sc, mix, y)
    for (ang, mix), ys in by.items():
        assert max(ys) <= 4 * min(ys) + 2.0 ** -23, (ang, mix, ys)
    for mix in tf.SHEARS:
        ys = [float(yard[r]) for r, k in enumerate(rungs) if k[2] == mix]
        print(f"rot6d yardstick shear {mix}: worst {max(ys):.3e}, median {sorted(ys)[len(ys) // 2]:.3e}")
    # all-zero six numbers: the oracle returns exact +0
    z = po.matrix_to_axis_angle(po.rotation_6d_to_matrix(torch.zeros(1, 6)))
    assert bool((z.view(torch.int32) == 0).all())


def test_lbs_yardstick_and_cases():
    """The 33 cases: every one of the 135 pose-corrective coefficients is, in one case, among the only non-zero ones; the fp32
    oracle's own distance from fp64 (the yardstick of the LBS bar) is between 1e-9 and 1e-6 m on every case."""
    pose, betas, names = tf.lbs_cases()
    R = mo.rodrigues(pose.double().reshape(-1, 16, 3))
    feat = (R[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(len(names), 135).abs()
    single = feat[1:16]
    assert bool(((single > 1e-3).sum(0) == 1).all()) and bool(((single > 1e-3).sum(1) == 9).all())
    assert float(feat[0].max()) == 0.0
    for seed in (0, 3):
        a = synthetic_mano_assets(seed)
        v64, j64 = mo.mano_lbs(a, pose, betas, center_idx=9, dtype=torch.float64)
        v32, j32 = mo.mano_lbs(a, pose, betas, center_idx=9, dtype=torch.float32)
        for r64, r32 in ((v64, v32), (j64, j32)):
            bar, e32 = tf.lbs_bar(r64, r32)
            assert float(e32.max()) < 1e-6 and float(bar.min()) > 1e-9, (seed, float(e32.max()), float(bar.min()))
        print(f"mano LBS yardstick seed {seed}: |fp32 - fp64| verts {float((v32 - v64).abs().max()):.3e} joints {float((j32 - j64).abs().max()):.3e}")


# =====================================================================================================================
# GPU: launchers
_PROTOS = {
    "poem_launch_q3_flatten": (_i, [_vp] * 4 + [_i] * 3 + [_vp]),
    "poem_launch_rot6d_to_aa": (_i, [_vp] * 3 + [_i, _vp]),
    "poem_launch_finalize": (_i, [_vp] * 3 + [_i] * 3 + [_f, _vp, _vp, _vp]),
    "poem_launch_finalize_param": (_i, [_vp] * 4 + [_i] * 2 + [_vp]),
    "poem_launch_param_rows": (_i, [_vp] * 3 + [_i] * 2 + [_vp]),
    "poem_launch_compose_weight": (_i, [_vp] * 3 + [_i] * 3 + [_vp]),
    "poem_launch_compose_bias": (_i, [_vp] * 4 + [_i] * 2 + [_vp]),
    "poem_launch_gather_anchor_rows": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "poem_launch_pad_rows": (_i, [_vp, _vp] + [_i] * 4 + [_vp]),
    "poem_launch_broadcast": (_i, [_vp, _vp, _l, _i, _vp]),
    "poem_launch_canon_xyz": (_i, [_vp, _vp, _i, _f, _vp]),
    "poem_launch_view_layout": (_i, [ctypes.POINTER(ViewLayoutArgs), _vp]),
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
def dev():
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    return DEV


_CANARY = 0x7FC0DEAD      # a NaN bit pattern no kernel writes
_GUARD = 256              # guard elements in front of and behind every output (1 KiB: keeps the 16-byte alignment)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want, what):
    g, w = _bits(got).flatten().cpu(), _bits(want).flatten().cpu()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = (g != w).nonzero().flatten()
        i = int(bad[0])
        pytest.fail(f"{what}: {bad.numel()} of {g.numel()} elements differ, first at {i}: got {int(g[i]) & 0xFFFFFFFF:#010x} "
                    f"want {int(w[i]) & 0xFFFFFFFF:#010x}")


class _Guarded:
    """n 32-bit elements holding the canary, with guard elements in front and behind"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * _GUARD,), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf[_GUARD:].data_ptr()

    def guards_ok(self):
        return bool((self.buf[:_GUARD] == _CANARY).all()) and bool((self.buf[_GUARD + self.n:] == _CANARY).all())

    def untouched(self):
        return bool((self.buf == _CANARY).all())

    def take(self, what, dtype=torch.float32):
        torch.cuda.synchronize()
        assert self.guards_ok(), f"{what}: a guard element was written"
        out = self.buf[_GUARD:_GUARD + self.n]
        return out.view(torch.float32) if dtype == torch.float32 else out


def _d(t):
    return t.to(DEV).contiguous()


def _padded(t):
    """t on the device with canary elements in front of it and behind it: an input whose index rule is under test, so that a row
    taken from one place too far is the canary and not a neighbour's plausible value"""
    buf = torch.full((t.numel() + 2 * _GUARD,), _CANARY, dtype=torch.int32, device=DEV)
    buf[_GUARD:_GUARD + t.numel()] = _bits(t).flatten().to(DEV)
    return buf[_GUARD:_GUARD + t.numel()].view(torch.float32).view(t.shape)


# ---------------------------------------------------------------------------------------------------------------------
# 1. q3_flatten
def _q3(feats, w, b, what):
    B, Q, C = feats.shape
    t = _Guarded(B * C)
    _call("poem_launch_q3_flatten", feats.data_ptr(), w.data_ptr(), b.data_ptr(), t.ptr, B, Q, C)
    return t.take(what).view(B, C)


@gpu
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 799])
def test_q3_flatten(Q, dev):
    """feats (B, Q, C) read as rows of Q floats, one wave per row, four waves per block: B C of 1, 3, 6, 18 (block tails of 1, 2, 3
    waves) and 128, 384; Q below, at and above a wave; the a-priori bar; one NaN poisons exactly its row."""
    for B in (1, 3):
        for C in (1, 6, 128):
            g = torch.Generator().manual_seed(Q * 1000 + B * 10 + C)
            feats, w, b = torch.randn(B, Q, C, generator=g), torch.randn(Q, generator=g), torch.randn(1, generator=g)
            what = f"q3_flatten B={B} Q={Q} C={C}"
            got = _q3(_d(feats), _d(w), _d(b), what)
            ref, T = tf.q3_ref(feats, w, b)
            err = (got.cpu().double() - ref).abs()
            bound = tf.q3_bound(Q, T)
            assert bool((err <= bound).all()), f"{what}: worst {float((err / bound).max()):.2f} x the bound"
            flat = (B * Q * C * 2) // 3
            poisoned = feats.clone()
            poisoned.view(-1)[flat] = float("nan")
            nan = _q3(_d(poisoned), _d(w), _d(b), what + " NaN")
            row = flat // Q
            assert bool(torch.isnan(nan.view(-1)[row])), f"{what}: the NaN's row {row} is {float(nan.view(-1)[row])}"
            keep = torch.ones(B * C, dtype=torch.bool, device=DEV)
            keep[row] = False
            _same(nan.view(-1)[keep], got.view(-1)[keep], what + " rows beside the NaN's")


# ---------------------------------------------------------------------------------------------------------------------
# 2. rot6d_to_aa
def _rot6d(par, what):
    B = par.shape[0]
    pose, betas = _Guarded(B * 48), _Guarded(B * 10)
    _call("poem_launch_rot6d_to_aa", par.data_ptr(), pose.ptr, betas.ptr, B)
    return pose.take(what + " pose").view(B, 16, 3), betas.take(what + " betas").view(B, 10)


_BETA_BITS = [0x7FC12345, 0xFFC00001 - (1 << 32), 0x7F800001, 0x7F800000, 0xFF800000 - (1 << 32), 0x80000000 - (1 << 32), 0x00000001,
              0x3F800000, 0x00000000, 0x807FFFFF - (1 << 32)]


@gpu
def test_rot6d_ladder_under_four_times_the_oracle(dev):
    """The ladder in launches of B = 1, 3, 4, 5 in turn (16, 48 rotations; 64: exactly one block; 80: a second block), each with
    guards; per rung the kernel's worst rotation error under 4 x the oracle's fp32 chain + 2^-23, and under 2e-6 for shear <= 0.7."""
    L = _ladder()
    d6, rung, rungs, yard, bars = L["d6"], L["rung"], L["rungs"], L["yard"], L["bars"]
    n = d6.shape[0]
    total = -(-n // (13 * 16)) * 13 * 16
    src = torch.arange(total) % n                       # (the tail wraps round to the first rungs)
    par = torch.zeros(total // 16, 106)
    par[:, :96] = d6[src].reshape(-1, 96)
    par[:, 96:] = torch.tensor(_BETA_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    par_d = _d(par)
    aa, b0 = [], 0
    while b0 < par.shape[0]:
        for B in (1, 3, 4, 5):
            chunk = par_d[b0:b0 + B]
            pose, betas = _rot6d(chunk, f"rot6d ladder samples {b0}..{b0 + B}")
            _same(betas, chunk[:, 96:], f"rot6d betas of samples {b0}..{b0 + B}")
            aa.append(pose.reshape(-1, 3).cpu())
            b0 += B
    aa = torch.cat(aa)
    assert aa.shape[0] == total and bool(torch.isfinite(aa).all())
    err = tf.rotation_error(aa, L["Rgs"][src])
    worst = tf.per_rung(err, rung[src], len(rungs))
    assert float(torch.linalg.norm(aa.double(), dim=-1).max()) <= 2 * math.pi + 1e-5
    bad = [(rungs[r], float(worst[r]), float(bars[r]), float(yard[r])) for r in range(len(rungs)) if not float(worst[r]) <= float(bars[r])]
    for mix in tf.SHEARS:
        sel = [r for r, k in enumerate(rungs) if k[2] == mix]
        ratio = max(float(worst[r]) / float(yard[r]) for r in sel if float(yard[r]) > 0)
        print(f"rot6d shear {mix}: worst kernel error {max(float(worst[r]) for r in sel):.3e}, worst kernel / yardstick {ratio:.2f}, "
              f"worst kernel / bar {max(float(worst[r]) / float(bars[r]) for r in sel):.2f}")
    assert not bad, f"{len(bad)} rungs (angle, scale, shear) over the bar: (rung, kernel, bar, yardstick) {bad[:6]}"


@gpu
def test_rot6d_exact_cases(dev):
    """B = 3: all-zero six numbers give exact +0; a NaN, +Inf or -Inf in any one of a joint's six numbers makes that joint's three
    outputs NaN and leaves every other output of the launch (pose and betas) with the clean launch's bits."""
    L = _ladder()
    g = torch.Generator().manual_seed(4)
    pick = torch.randperm(L["d6"].shape[0], generator=g)[:48]
    par = torch.zeros(3, 106)
    par[:, :96] = L["d6"][pick].reshape(3, 96)
    par[:, 96:] = torch.randn(3, 10, generator=g)
    par[1, 5 * 6:5 * 6 + 6] = 0.0
    clean_pose, clean_betas = _rot6d(_d(par), "rot6d clean")
    assert bool((_bits(clean_pose[1, 5]) == 0).all()), f"all-zero six numbers: {clean_pose[1, 5].tolist()}"
    assert bool(torch.isfinite(clean_pose).all())
    b, j = 2, 11
    keep = torch.ones(3, 16, dtype=torch.bool, device=DEV)
    keep[b, j] = False
    for k in range(6):
        for val in (float("nan"), float("inf"), float("-inf")):
            p = par.clone()
            p[b, j * 6 + k] = val
            what = f"rot6d {val} in number {k} of sample {b} joint {j}"
            pose, betas = _rot6d(_d(p), what)
            assert bool(torch.isnan(pose[b, j]).all()), f"{what}: outputs {pose[b, j].tolist()}"
            _same(pose[keep], clean_pose[keep], what + ": the other joints")
            _same(betas, clean_betas, what + ": betas")


# ---------------------------------------------------------------------------------------------------------------------
# 3. finalize, finalize_param, param_rows
RADIUS = 0.17            # not a power of two


def _finalize(xyz, centre, L, B, Q, verts=None, joints=None, what="finalize"):
    out = _Guarded(L * B * Q * 3)
    _call("poem_launch_finalize", xyz.data_ptr(), centre.data_ptr(), out.ptr, L, B, Q, RADIUS,
          None if verts is None else verts.data_ptr(), None if joints is None else joints.data_ptr())
    return out.take(what).view(L, B, Q, 3)


@gpu
@pytest.mark.parametrize("special", [False, True])
def test_finalize_family_bit_for_bit(special, dev):
    """L in {1, 3}, B in {1, 3}, Q in {22, 799}: finalize bit-equal to fp32 torch's nan_to_num(x) * r + c -- two roundings; with
    MANO pointers the earlier layers keep those bits, the last is nan_to_num(joints | verts) + c bit for bit and does not read xyz's
    last layer; finalize_param (centre from ref_joints[:, 9]) gives the same bits; param_rows is a bit copy."""
    for L in (1, 3):
        for B in (1, 3):
            for Q in (22, 799):
                g = torch.Generator().manual_seed(L * 100 + B * 10 + Q)
                xyz = torch.randn(L, B, Q, 3, generator=g)
                rj = torch.randn(B, 21, 3, generator=g) * 0.3
                verts, joints = torch.randn(B, Q - 21, 3, generator=g) * 0.1, torch.randn(B, 21, 3, generator=g) * 0.1
                if special:
                    tf.seed_specials(xyz, 1)
                    tf.seed_specials(verts, 2)
                    tf.seed_specials(joints, 3, frac=0.1)
                    rj[0, 9, 0], rj[B - 1, 9, 2] = 0.0, -0.0
                centre = rj[:, 9].contiguous()
                what = f"L={L} B={B} Q={Q} special={special}"
                xyz_d, c_d, v_d, j_d, rj_d = _d(xyz), _d(centre), _padded(verts), _padded(joints), _d(rj)
                plain = _finalize(xyz_d, c_d, L, B, Q, what="finalize " + what)
                ref = tf.finalize_ref(xyz, centre, RADIUS)
                assert not special or bool(torch.isfinite(ref).all())
                _same(plain, ref, "finalize " + what)
                want_last = tf.finalize_mano_ref(verts, joints, centre)
                mano = _finalize(xyz_d, c_d, L, B, Q, v_d, j_d, what="finalize with MANO " + what)
                _same(mano[:L - 1], plain[:L - 1], "finalize with MANO, earlier layers " + what)
                _same(mano[L - 1], want_last, "finalize with MANO, last layer " + what)
                poisoned = xyz_d.clone()
                poisoned[L - 1] = torch.full((B, Q, 3), _CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
                _same(_finalize(poisoned, c_d, L, B, Q, v_d, j_d, what="finalize with MANO, canary xyz " + what), mano,
                      "finalize with MANO over a canary last layer " + what)
                fp = _Guarded(B * Q * 3)
                _call("poem_launch_finalize_param", v_d.data_ptr(), j_d.data_ptr(), rj_d.data_ptr(), fp.ptr, B, Q)
                _same(fp.take("finalize_param " + what).view(B, Q, 3), mano[L - 1], "finalize_param " + what)
                pr = _Guarded(B * Q * 3)
                _call("poem_launch_param_rows", v_d.data_ptr(), j_d.data_ptr(), pr.ptr, B, Q)
                _same(pr.take("param_rows " + what).view(B, Q, 3), tf.param_rows_ref(verts, joints), "param_rows " + what)


# ---------------------------------------------------------------------------------------------------------------------
# 4. compose_weight, compose_bias
@gpu
@pytest.mark.parametrize("N,Cm,K", [(5, 7, 3), (1, 1, 1), (128, 128, 128)])
def test_compose(N, Cm, K, dev):
    g = torch.Generator().manual_seed(N + Cm + K)
    A, Bm = torch.randn(N, Cm, generator=g), torch.randn(Cm, K, generator=g)
    b1, b2 = torch.randn(Cm, generator=g), torch.randn(N, generator=g)
    A_d, B_d, b1_d, b2_d = _d(A), _d(Bm), _d(b1), _d(b2)
    out = _Guarded(N * K)
    _call("poem_launch_compose_weight", A_d.data_ptr(), B_d.data_ptr(), out.ptr, N, Cm, K)
    got = out.take(f"compose_weight {N} {Cm} {K}").view(N, K).cpu().double().numpy()
    for with_b2 in (False, True):
        W, TW, b, Tb = tf.compose_ref(A, Bm, b1, b2 if with_b2 else None)
        ob = _Guarded(N)
        _call("poem_launch_compose_bias", A_d.data_ptr(), b1_d.data_ptr(), b2_d.data_ptr() if with_b2 else None, ob.ptr, N, Cm)
        gb = ob.take(f"compose_bias {N} {Cm} b2={with_b2}").cpu().double().numpy()
        assert np.all(np.abs(gb - b) <= tf.compose_bound(b, Tb, Cm)), f"compose_bias N={N} Cm={Cm} b2={with_b2}"
    assert np.all(np.abs(got - W) <= tf.compose_bound(W, TW, Cm)), f"compose_weight N={N} Cm={Cm} K={K}"


# ---------------------------------------------------------------------------------------------------------------------
# 5. gather_anchor_rows, pad_rows, broadcast, canon_xyz
def _pattern(*shape, seed=0):
    """random bit patterns that are finite floats, a few NaN among them: data movement must keep every bit"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g)
    t.view(-1)[::97] = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)
    return t


@gpu
def test_gather_anchor_rows(dev):
    NS = 57
    g = torch.Generator().manual_seed(8)
    idx = torch.randperm(NS - 1, generator=g)[:32].to(torch.int32)          # non-monotone, every index below NS - 1
    assert int(idx.max()) < NS and not bool((idx[1:] > idx[:-1]).all())
    for B in (1, 3):
        for C in (4, 128):
            for ld in (C, C + 4):
                src = _pattern(B * NS, ld, seed=B + C + ld)
                want = torch.stack([src[b * NS + idx.long(), :C] for b in range(B)]).reshape(B * 32, C)
                for with_ident in (False, True):
                    what = f"gather B={B} C={C} ld={ld} ident={with_ident}"
                    dst, ident = _Guarded(B * 32 * C), _Guarded(32)
                    src_d, idx_d = _d(src), _d(idx)
                    _call("poem_launch_gather_anchor_rows", src_d.data_ptr(), ld, idx_d.data_ptr(), NS, dst.ptr, B, C,
                          ident.ptr if with_ident else None)
                    _same(dst.take(what).view(B * 32, C), want, what)
                    if with_ident:
                        assert ident.take(what + " ident", torch.int32).tolist() == list(range(32)), what
                    else:
                        torch.cuda.synchronize()
                        assert ident.untouched()


@gpu
def test_pad_rows(dev):
    for S in (1, 31, 32):
        for SP in (S, S + 1, 64):
            for W in (3, 128):
                for B in (1, 3):
                    what = f"pad_rows S={S} SP={SP} W={W} B={B}"
                    src = _pattern(B, S, W, seed=S + SP + W + B)
                    src[B - 1, S - 1] = float("nan")                  # a NaN source row stays
                    want = torch.zeros(B, SP, W)
                    want[:, :S] = src
                    dst, src_d = _Guarded(B * SP * W), _padded(src)
                    _call("poem_launch_pad_rows", src_d.data_ptr(), dst.ptr, B, S, SP, W)
                    got = dst.take(what).view(B, SP, W)
                    _same(got, want, what)
                    assert bool((_bits(got[:, S:]) == 0).all()), what + ": pad rows are not +0"


@gpu
def test_broadcast(dev):
    for per in (1, 255, 256, 257):
        for copies in (1, 3):
            what = f"broadcast per={per} copies={copies}"
            src = _pattern(per, seed=per + copies)
            dst, src_d = _Guarded(per * copies), _d(src)
            _call("poem_launch_broadcast", src_d.data_ptr(), dst.ptr, per, copies)
            _same(dst.take(what).view(copies, per), src[None].expand(copies, per), what)


@gpu
def test_canon_xyz(dev):
    """bit-equal to numpy's fp32 division, 0, -0, denormals (in and out), Inf and NaN included"""
    for n in (1, 3 * 799):
        g = torch.Generator().manual_seed(n)
        t = torch.randn(n, generator=g) * 0.1
        if n > 1:
            sp = torch.tensor([0x00000000, 0x80000000 - (1 << 32), 0x00000001, 0x807FFFFF - (1 << 32), 0x00800000, 0x00000123, 0x7F800000,
                               0xFF800000 - (1 << 32), 0x7FC00000, 0x7F7FFFFF, 0x00200000], dtype=torch.int64).to(torch.int32).view(torch.float32)
            t[5:5 + len(sp)] = sp
            t[300:300 + len(sp)] = sp
        for radius in (0.1, 3.0, 1e-3):
            with np.errstate(over="ignore"):                         # (FLT_MAX / 1e-3 is Inf on both sides)
                want = torch.from_numpy(t.numpy() / np.float32(radius))
            assert want.dtype == torch.float32
            out, t_d = _Guarded(n), _d(t)
            _call("poem_launch_canon_xyz", t_d.data_ptr(), out.ptr, n, radius)
            _same(out.take(f"canon_xyz n={n}"), want, f"canon_xyz n={n} radius={radius}")


# ---------------------------------------------------------------------------------------------------------------------
# 6. view_layout
@gpu
@pytest.mark.parametrize("name", list(tf.LAYOUT_BATCHES))
def test_view_layout(name, dev):
    """offs, view_sample, pe_index exactly the integer restatement: one sample, the 1663-sample limit of the argument block,
    a mixed batch, 1663 samples of 65535 views (both limits: the last 16-bit offset is 0xFFFF), one sample of 64 views."""
    views = tf.LAYOUT_BATCHES[name]
    offs, vs, pe = tf.view_layout_ref(views)
    B, BN = len(views), int(offs[-1])
    o, s, p = _Guarded(B + 1), _Guarded(BN), _Guarded(BN)
    a = ViewLayoutArgs()
    a.offs, a.view_sample, a.pe_index, a.B = o.ptr, s.ptr, p.ptr, B
    for b in range(B + 1):
        a.off16[b] = int(offs[b])
    rc = _fn("poem_launch_view_layout")(ctypes.byref(a), hip.stream())
    assert rc == 0
    for got, want, what in ((o, offs, "offs"), (s, vs, "view_sample"), (p, pe, "pe_index")):
        g = got.take(f"view_layout {name} {what}", torch.int32).cpu().numpy()
        assert np.array_equal(g, want), f"view_layout {name}: {what} differs at {np.nonzero(g != want)[0][:8].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# 7. mano_prepare, mano_lbs, mano_recentre (through the C ABI)
_MANO = {}


def _mano(seed):
    """assets, restated table, the kernel's table (guards checked) for a seed, once"""
    if seed not in _MANO:
        a = synthetic_mano_assets(seed)
        dv = {k: _d(torch.from_numpy(v)) for k, v in a.items()}
        assert hip.lib().poem_mano_table_bytes() == 4 * tf.TABLE_FLOATS
        table = _Guarded(tf.TABLE_FLOATS)
        rc = hip.lib().poem_mano_prepare(dv["v_template"].data_ptr(), dv["shapedirs"].data_ptr(), dv["posedirs"].data_ptr(),
                                         dv["J_regressor"].data_ptr(), dv["weights"].data_ptr(), table.ptr, hip.stream())
        assert rc == 0
        _MANO[seed] = dict(assets=a, tab=tf.mano_table(a), table=table, got=table.take(f"mano table seed {seed}"))
    return _MANO[seed]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _MANO.clear()
    _LADDER.clear()
    _LBS.clear()


def _lbs(m, pose, betas, centre, what):
    B = pose.shape[0]
    verts, joints = _Guarded(B * 778 * 3), _Guarded(B * 63)
    rc = hip.lib().poem_mano_lbs(pose.data_ptr(), betas.data_ptr(), m["table"].ptr, B, centre, verts.ptr, joints.ptr, hip.stream())
    assert rc == 0, f"{what}: poem_mano_lbs returned {rc}"
    return verts.take(what + " verts").view(B, 778, 3), joints.take(what + " joints").view(B, 21, 3)


@gpu
@pytest.mark.parametrize("seed", [0, 3])
def test_mano_table(seed, dev):
    """The table of mano_prepare against the layout restated from mano.hip's header: template, D and W regions bit for bit -- zeros
    in the padded vertex columns 778..831 and in coefficients 145..147 -- and the two composed joint regressions within one fp32
    rounding of the fp64 sums."""
    m = _mano(seed)
    got, tab = m["got"].cpu(), m["tab"]
    want = torch.from_numpy(tf.table_flat32(tab))
    for name, lo, hi in (("template", tf.OFF_VT, tf.OFF_D), ("D", tf.OFF_D, tf.OFF_W), ("W", tf.OFF_W, tf.OFF_JT)):
        _same(got[lo:hi], want[lo:hi], f"mano table seed {seed}: {name} region")
    D = got[tf.OFF_D:tf.OFF_W].view(tf.K4, 3, tf.VP, 4)
    assert bool((_bits(D[:, :, tf.NV:]) == 0).all()) and bool((_bits(D[tf.K4 - 1, :, :, 1:]) == 0).all())
    assert bool((D[tf.K4 - 1, :, :tf.NV, 0] != 0).all())                         # coefficient 144 is there
    assert bool((_bits(got[tf.OFF_VT:tf.OFF_D].view(3, tf.VP)[:, tf.NV:]) == 0).all())
    assert bool((_bits(got[tf.OFF_W:tf.OFF_JT].view(tf.NJ, tf.VP)[:, tf.NV:]) == 0).all())
    for name, lo, hi, ref, T in (("J_t", tf.OFF_JT, tf.OFF_JSD, tab["JT"], tab["TJT"]),
                                 ("J_sd", tf.OFF_JSD, tf.TABLE_FLOATS, tab["JSD"].ravel(), tab["TJSD"].ravel())):
        err = np.abs(got[lo:hi].double().numpy() - ref)
        bound = tf.U32 * np.abs(ref) + 778 * tf.U64 * T
        assert np.all(err <= bound), f"mano table seed {seed}: {name} worst {float((err / bound).max()):.2f} x the bound"


_LBS = {}


def _lbs_full(seed, centre):
    """the 33 cases in one launch, and the fp64 / fp32 oracles of the same inputs, once per (seed, centre)"""
    key = (seed, centre)
    if key not in _LBS:
        m = _mano(seed)
        pose, betas, names = tf.lbs_cases()
        v, j = _lbs(m, _d(pose), _d(betas), centre, f"mano_lbs seed {seed} centre {centre} B=33")
        r64 = mo.mano_lbs(m["assets"], pose, betas, center_idx=centre, dtype=torch.float64)
        r32 = mo.mano_lbs(m["assets"], pose, betas, center_idx=centre, dtype=torch.float32)
        _LBS[key] = dict(pose=pose, betas=betas, names=names, v=v, j=j, r64=r64, r32=r32)
    return _LBS[key]


@gpu
@pytest.mark.parametrize("centre", [-1, 9, 4])
@pytest.mark.parametrize("seed", [0, 3])
def test_mano_lbs_under_four_times_the_oracle(seed, centre, dev):
    """B = 33: zero pose, each finger joint alone at 0.9 rad with the pose-corrective basis in place, 0.6 randn, every joint at 3 rad
    and at 2 pi, betas randn and +-5 -- per sample, joints and vertices separately, |HIP - fp64| <= 4 |fp32 oracle - fp64| +
    2^-23 max|fp64|.  centre: none, a kinematic joint (9), a finger tip (4: the re-centring launch)."""
    c = _lbs_full(seed, centre)
    worst = 0.0
    for name, got, r64, r32 in (("verts", c["v"], c["r64"][0], c["r32"][0]), ("joints", c["j"], c["r64"][1], c["r32"][1])):
        assert bool(torch.isfinite(got).all())
        err = (got.cpu().double() - r64).abs().flatten(1).amax(1)
        bar, e32 = tf.lbs_bar(r64, r32)
        ratio = err / e32.clamp(min=1e-300)
        worst = max(worst, float(ratio.max()))
        print(f"mano LBS seed {seed} centre {centre} {name}: worst |hip - fp64| {float(err.max()):.3e}, |fp32 - fp64| {float(e32.max()):.3e}, "
              f"worst ratio {float(ratio.max()):.2f} ({c['names'][int(ratio.argmax())]}), worst err / bar {float((err / bar).max()):.2f}")
        bad = (err > bar).nonzero().flatten().tolist()
        assert not bad, (f"mano_lbs seed {seed} centre {centre} {name}: over the bar in " +
                         ", ".join(f"{c['names'][b]} ({float(err[b]):.3e} > {float(bar[b]):.3e}, fp32 {float(e32[b]):.3e})" for b in bad[:6]))
    if centre >= 0:
        assert float(c["j"][:, centre].abs().max()) == 0.0


@gpu
@pytest.mark.parametrize("centre", [-1, 9, 4])
def test_mano_lbs_bits_do_not_depend_on_the_batch(centre, dev):
    """B = 1 and B = 2 (another order, another place) give the rows of the B = 33 launch bit for bit; a NaN in one sample's pose
    or betas makes that sample NaN where the fp64 reference is NaN and leaves the other 32 samples' bits alone."""
    seed = 3
    m, c = _mano(seed), _lbs_full(seed, centre)
    pose, betas = c["pose"], c["betas"]
    for ids in ([0], [17], [32], [20, 5], [32, 31]):
        v, j = _lbs(m, _d(pose[ids]), _d(betas[ids]), centre, f"mano_lbs centre {centre} samples {ids}")
        _same(v, c["v"][ids], f"mano_lbs centre {centre} samples {ids}: verts against the B=33 launch")
        _same(j, c["j"][ids], f"mano_lbs centre {centre} samples {ids}: joints against the B=33 launch")
    nan = float("nan")
    for b, where in ((13, "pose joint 7"), (32, "pose root"), (0, "betas")):
        p, be = pose.clone(), betas.clone()
        if where == "betas":
            be[b, 4] = nan
        else:
            p[b, 0 if where == "pose root" else 7 * 3 + 1] = nan
        what = f"mano_lbs centre {centre} NaN in {where} of sample {b}"
        v, j = _lbs(m, _d(p), _d(be), centre, what)
        r64 = mo.mano_lbs(m["assets"], p[b:b + 1], be[b:b + 1], center_idx=centre, dtype=torch.float64)
        for name, got, ref in (("verts", v, r64[0]), ("joints", j, r64[1])):
            isn = torch.isnan(ref[0])
            assert bool(isn.any()) and bool(torch.isnan(got[b].cpu())[isn].all()), f"{what}: {name} finite where the reference is NaN"
        keep = torch.ones(33, dtype=torch.bool, device=DEV)
        keep[b] = False
        _same(v[keep], c["v"][keep], what + ": the other samples' verts")
        _same(j[keep], c["j"][keep], what + ": the other samples' joints")


# ---------------------------------------------------------------------------------------------------------------------
# refusals
@gpu
def test_refusals_leave_the_outputs_alone(dev):
    """poem_rot6d_to_axis_angle, poem_mano_prepare, poem_mano_lbs: POEM_E_ARG for each null pointer, batch 0, batch 65536 (LBS),
    center_idx -2 and 21, with every canary-filled output untouched."""
    L = hip.lib()
    m = _mano(0)
    par = _d(torch.randn(2, 106))
    pose_o, betas_o = _Guarded(2 * 48), _Guarded(2 * 10)
    good = [par.data_ptr(), pose_o.ptr, betas_o.ptr]
    cases = [[None if k == i else p for k, p in enumerate(good)] + [2] for i in range(3)] + [good + [0], good + [-1]]
    for args in cases:
        assert L.poem_rot6d_to_axis_angle(*args, hip.stream()) == POEM_E_ARG, args
    dv = [_d(torch.from_numpy(m["assets"][k])) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")]
    table_o = _Guarded(tf.TABLE_FLOATS)
    good = [t.data_ptr() for t in dv] + [table_o.ptr]
    for i in range(6):
        args = [None if k == i else p for k, p in enumerate(good)]
        assert L.poem_mano_prepare(*args, hip.stream()) == POEM_E_ARG, i
    pose, betas = _d(torch.zeros(2, 48)), _d(torch.zeros(2, 10))
    verts_o, joints_o = _Guarded(2 * 778 * 3), _Guarded(2 * 63)
    good = dict(pose=pose.data_ptr(), betas=betas.data_ptr(), table=m["table"].ptr, batch=2, centre=9, verts=verts_o.ptr, joints=joints_o.ptr)
    bad = [dict(good, **{k: None}) for k in ("pose", "betas", "table", "verts", "joints")]
    bad += [dict(good, batch=0), dict(good, batch=65536), dict(good, centre=-2), dict(good, centre=21)]
    for a in bad:
        rc = L.poem_mano_lbs(a["pose"], a["betas"], a["table"], a["batch"], a["centre"], a["verts"], a["joints"], hip.stream())
        assert rc == POEM_E_ARG, a
    torch.cuda.synchronize()
    for o, name in ((pose_o, "pose"), (betas_o, "betas"), (table_o, "table"), (verts_o, "verts"), (joints_o, "joints")):
        assert o.untouched(), f"a refused call wrote {name}"
