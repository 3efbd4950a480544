"""csrc/dlt.hip -- ``dlt_kernel`` and ``dlt_conf_kernel`` alone, in every form: through ``poem_triangulate_dlt`` /
``poem_dlt_confidence`` (ctypes, every output between canary-filled guards) and through ``poem_v2_amd.triangulation``.

The restatement, the derivation of the solve's bar and the construction of the conditioning ladder are in
tests/dlt_forms_util.py (module docstring).  In short: M and the rows are restated exactly in fp32 (Fraction + one rounding per
operation) in BOTH roundings the compiler may pick for ``u * M2 - M0``; the reference of the solve is the fp64 SVD with the sign
x3 >= 0; the bar is  u |X*| + c e sigma1^2 / (sigma3^2 - sigma4^2) (1 + |X*|) / x3  with c counted from the kernel's roundings.
The end-to-end bar is 4 x the error of ``dlt_oracle`` in fp32 on the CPU (re-signed) + 2^-23 max |X*|, per sample.

Bit-for-bit claims that tests/test_dlt_confidence.py already asserts in the same form and that are therefore NOT repeated here:
"weighted mode with confidence 1 equals the plain kernel" and "threshold mode with threshold 0 and positive confidences equals the
plain kernel" (test_hip_reproduces_plain_dlt_bit_for_bit, test_hip_one_solve_behind_both_kernels_at_70_joints).

Every loop of the kernels is bounded, which is why the non-finite and degenerate inputs below end: the Jacobi loop runs 12 sweeps
of 6 rotations at most whatever G holds (a NaN makes ``off <= 1e-40 * diag`` false; an infinite G made it ``inf <= inf``, TRUE, which
left (1e7, 0, 0) for an infinite uv until these tests found it -- the rule now asks for a finite diag), the view loop runs
offs[b+1] - offs[b] times, and the threshold pass leaves ``while (thr > 0)`` after at most threshold / 0.05 <= 1280 lowerings because
``poem_dlt_confidence`` refuses threshold > 64 and NaN.  Read in dlt.hip:62-76,126-135 and ops.cpp before the first run."""
import numpy as np
import pytest
import torch

import dlt_forms_util as du
import dlt_oracle as do
from test_dlt import _dlt_inputs, _golden
from test_dlt_confidence import restate as restate_conf

DEV = "cuda:0"
_CANARY = 0x7FC0DEAD      # a NaN bit pattern no kernel writes
_GUARD = 256
SHAPES = [(1, 1), (1, 21), (3, 21), (4, 16), (5, 13), (67, 1), (2, 64), (2, 65), (2, 70)]


# =====================================================================================================================================
# CPU: the restatement and every condition on the inputs
# =====================================================================================================================================
def test_rne24_is_the_fp32_rounding():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(size=400) * 10.0 ** rng.integers(-20, 20, 400), [1.0, -1.0, 0.0, 2.0 ** -100]])
    half = np.float64(2 ** 24) + np.arange(1, 41, dtype=np.float64)                # odd ones sit half way between two fp32
    for v in np.concatenate([x, half, -half, half * 2.0 ** -40]):
        assert float(du.rne24(du.Fraction(float(v)))) == float(np.float32(v)), v
    assert int(np.sum(np.float32(half) != half)) == 20                             # (the ties are ties, and go to even)
    # an exact result that a detour through fp64 rounds twice: 1 + 2^-24 + 2^-60 is above the tie, fp64 puts it ON the tie
    q = du.Fraction(1) + du.Fraction(2.0 ** -24) + du.Fraction(2.0 ** -60)
    assert float(du.rne24(q)) == 1.0 + 2.0 ** -23 and float(np.float32(float(q))) == 1.0


def test_restatement_agrees_with_the_oracle_in_fp64_once_resigned():
    c = du.mixed_batch(4, 6, seed=11, lo=2, hi=9)
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    uv, K, T = (torch.from_numpy(c[k]).double() for k in ("uv", "K", "T"))
    rows = du.rows_fp64(c["uv"], c["K"], c["T"])
    signs = [0, 0]
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        with du.resigned_svd():
            got = do.batch_triangulate_dlt(uv[s:e][None], K[s:e][None], T[s:e][None])[0].numpy()
        raw = do.batch_triangulate_dlt(uv[s:e][None], K[s:e][None], T[s:e][None])[0].numpy()      # LAPACK's own sign
        for j in range(6):
            Xp, sv, x = du.solve_svd(rows[j, s:e])
            Xm = du.solve_svd(rows[j, s:e], sign=-1)[0]
            assert np.abs(got[j] - Xp).max() <= 1e-12 * max(1.0, np.abs(Xp).max()), (b, j)
            dp, dm = np.abs(raw[j] - Xp).max(), np.abs(raw[j] - Xm).max()
            assert min(dp, dm) <= 1e-12 and max(dp, dm) > 0.5 * du.sign_gap(Xp, x[3]), (b, j, dp, dm)
            assert abs(np.abs(Xm - Xp).max() / du.sign_gap(Xp, x[3]) - 1) < 1e-3
            signs[int(dm < dp)] += 1
    print(f"fp64 oracle, LAPACK's sign: {signs[0]} joints with x3 >= 0, {signs[1]} with x3 < 0")


def test_fixture_joints_sit_at_one_of_the_two_signs():
    """tests/golden/dlt.npz (upstream's own fp32 run).  The two signs are 2e-7 |X| / x3 apart (asserted here against the fp64
    solve: it is the exact gap); every upstream joint lies within the oracle's 2e-6 m of the nearer one, and its two distances
    differ by no more than that gap.  Upstream's fp32 SVD noise (about 5e-7 m) is larger than the gap at these depths (1.4e-7 m), so
    which sign a joint is nearer to is a tally, printed, and not an identification."""
    z, cases = _golden()
    tally = [0, 0]
    for name in ("u8", "u2", "ragged"):
        views, seed = cases[name]["views"], cases[name]["seed"]
        uv, K, Emat = _dlt_inputs(views, seed)
        T = torch.linalg.inv(Emat).numpy()
        rows = du.rows_fp64(uv.numpy(), K.numpy(), T)
        offs = np.concatenate([[0], np.cumsum(views)])
        for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
            for j in range(21):
                Xp, sv, x = du.solve_svd(rows[j, s:e])
                Xm = du.solve_svd(rows[j, s:e], sign=-1)[0]
                gap = np.abs(Xm - Xp).max()
                assert abs(gap / du.sign_gap(Xp, x[3]) - 1) < 1e-3 and x[3] > 0.05
                up = z[name][b, j].astype(np.float64)
                dp, dm = np.abs(up - Xp).max(), np.abs(up - Xm).max()
                assert min(dp, dm) < 2e-6 and abs(dp - dm) <= gap * (1 + 1e-9), (name, b, j, dp, dm, gap)
                tally[int(dm < dp)] += 1
    print(f"upstream fixture: {tally[0]} joints nearer to x3 >= 0, {tally[1]} nearer to x3 < 0")
    assert sum(tally) == 16 * 21


@pytest.mark.parametrize("invert", [False, True])
def test_ladders_have_the_properties_claimed(invert):
    L = du.ladder(invert)
    assert len(L["views"]) == 40 and sum(L["views"]) == 290 and L["uv"].shape == (290, du.LADDER_J, 2)
    assert all(a.dtype == np.float32 for a in (L["uv"], L["K"], L["mat"]))
    offs = np.concatenate([[0], np.cumsum(L["views"])])
    per_rung = np.zeros(len(du.RUNGS), dtype=int)
    forms = [du.rows_fp64(L["uv"], L["K"], L["T64"])] if invert else None
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        r = du.RUNGS[L["rung"][b]]
        if invert:
            sols = [[du.solve_svd(forms[0][j, s:e]) for j in range(du.LADDER_J)]]
        else:
            sols = [[(q["Xs"], q["s"], [0, 0, 0, q["x3"]]) for q in du.ladder_refs(f)[b]] for f in (True, False)]
        for sol in sols:
            for Xs, sv, x in sol:
                assert r / np.sqrt(10) <= sv[0] / sv[2] < r * np.sqrt(10), (b, r, sv)
                assert x[3] > 0.05 and 0.5 * L["dist"][b] < np.abs(Xs).max() < 1.5 * L["dist"][b] + 0.4
        per_rung[L["rung"][b]] += du.LADDER_J
    assert (per_rung == 24).all()                                                  # "about 20 joints per rung"
    assert L["base"][L["rung"] == 0].max() > 0.1 and L["base"][L["rung"] == 4].min() < 1e-4
    print("baselines per rung (m):", [f"{L['base'][L['rung'] == i].min():.2e}..{L['base'][L['rung'] == i].max():.2e}" for i in range(5)])


def test_jacobi_restatement_stays_under_half_the_bar_and_low_rungs_are_one_rounding():
    """The numpy fp64 restatement of the kernel's own algorithm over the solve-local ladder, both roundings: under HALF the bar on
    every joint, converged before the 12-sweep cap; on the rungs up to 1e2 the bar's second term is below u |X*|."""
    L = du.ladder(False)
    worst_unit, worst_bar = 0.0, 0.0
    for fused in (True, False):
        for b, refs in enumerate(du.ladder_refs(fused)):
            for q in refs:
                err = np.abs(q["Xj"] - q["Xs"]).max()
                assert err <= 0.5 * q["bar"] and q["sweeps"] < 12, (b, err, q["bar"], q["sweeps"])
                worst_unit, worst_bar = max(worst_unit, err / q["unit"]), max(worst_bar, err / q["bar"])
                if L["rung"][b] <= 1:
                    assert q["t2"] < q["t1"], (b, q["t2"], q["t1"])
    print(f"fp64 Jacobi restatement: worst error {worst_unit:.3g} perturbation units, {worst_bar:.3g} of the bar")


def test_sign_batch_needs_the_sign_rule():
    """On the samples whose master frame lies on the negative side of the rig the rotations leave x3 < 0 (fp64 restatement of the
    kernel's Jacobi, both roundings): without the flip these joints would be the OTHER sign's answer, 2e-7 |X| / x3 away -- more
    than the bar, which is asserted too."""
    c = du.sign_batch()
    for fused in (True, False):
        neg = 0
        for b in range(len(c["views"])):
            rows = du.rows_of(c["uv"][4 * b:4 * b + 4], c["K"][4 * b:4 * b + 4], c["T"][4 * b:4 * b + 4], fused)
            for j in range(5):
                q = du.joint_ref(rows[j])
                x3_raw = du.solve_jacobi(rows[j], raw=True)[2]
                assert q["x3"] > 0.05 and np.abs(q["Xj"] - q["Xs"]).max() <= 0.5 * q["bar"] and q["sweeps"] < 12
                if x3_raw < 0:
                    neg += 1
                    assert du.sign_gap(q["Xs"], q["x3"]) > 1.5 * q["bar"], (b, j, du.sign_gap(q["Xs"], q["x3"]), q["bar"])
        assert 10 <= neg <= 20, neg
    print(f"sign batch: the rotations leave x3 < 0 on {neg} of 25 joints")


def test_exact_extrinsics_invert_exactly():
    E = du.exact_extrinsics(np.random.default_rng(5), 40).astype(np.float64)
    Ti = np.linalg.inv(E)
    assert np.array_equal(Ti.astype(np.float32).astype(np.float64), Ti)
    for a, b in zip(E, Ti):
        assert np.array_equal(a @ b, np.eye(4)) and np.array_equal(b @ a, np.eye(4))
    assert len({tuple(np.abs(a[:3, :3]).argmax(1)) for a in E}) >= 3              # more than one permutation


# =====================================================================================================================================
# GPU
# =====================================================================================================================================
class _Guarded:
    """n 32-bit elements holding the canary, with guard elements in front and behind"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * _GUARD,), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf[_GUARD:].data_ptr()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == _CANARY).all())

    def take(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:_GUARD] == _CANARY).all()) and bool((self.buf[_GUARD + self.n:] == _CANARY).all()), \
            f"{what}: a guard element was written"
        return self.buf[_GUARD:_GUARD + self.n].cpu().numpy().view(np.uint32)


class _Batch:
    """A batch resident on the device; ``run`` launches all of it or one sample of it (pointers moved to that sample)."""

    def __init__(self, c):
        self.c, self.views = c, [int(v) for v in c["views"]]
        self.offs_np = np.concatenate([[0], np.cumsum(self.views)]).astype(np.int32)
        self.J = c["uv"].shape[1]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)           # noqa: E731
        self.t = {k: up(c[k]) for k in ("uv", "conf", "K", "T", "E") if k in c}
        self.offs = up(self.offs_np)
        self._one = {}

    def run(self, mode=None, thr=0.5, invert=False, sample=None, mat=None, offs=None, B=None):
        """-> (out (B,J,3) as uint32 bits, count (B,J) int32 or None)."""
        import poem_v2_amd as pk
        L, J = pk.hip.lib(), self.J
        v0 = 0 if sample is None else int(self.offs_np[sample])
        if sample is not None:
            n = self.views[sample]
            if n not in self._one:
                self._one[n] = torch.tensor([0, n], dtype=torch.int32, device=DEV)
            offs, B = self._one[n], 1
        elif offs is None:
            offs, B = self.offs, len(self.views)
        m = self.t["E" if invert else "T"] if mat is None else mat
        p = dict(uv=self.t["uv"].data_ptr() + v0 * J * 8, K=self.t["K"].data_ptr() + v0 * 36, mat=m.data_ptr() + v0 * 64)
        out = _Guarded(B * J * 3)
        what = f"mode {mode} invert {invert} sample {sample} B {B} J {J}"
        if mode is None:
            rc = L.poem_triangulate_dlt(p["uv"], p["K"], p["mat"], offs.data_ptr(), B, J, int(invert), out.ptr, pk.hip.stream())
            assert rc == 0, (what, rc)
            return out.take(what).reshape(B, J, 3), None
        cnt = _Guarded(B * J)
        rc = L.poem_dlt_confidence(p["uv"], self.t["conf"].data_ptr() + v0 * J * 4, p["K"], p["mat"], offs.data_ptr(), out.ptr, cnt.ptr,
                                   B, J, int(invert), pk.hip.DLT_MODES[mode], float(thr), pk.hip.stream())
        assert rc == 0, (what, rc)
        return out.take(what).reshape(B, J, 3), cnt.take(what + " (sel_count)").view(np.int32).reshape(B, J)


def _f(bits):
    return bits.view(np.float32).astype(np.float64)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} words differ"


_LADDER_RUNS = {}


def _ladder_run(invert):
    if invert not in _LADDER_RUNS:
        L = du.ladder(invert)
        c = dict(views=L["views"], uv=L["uv"], K=L["K"], T=L["mat"], E=L["mat"])
        _LADDER_RUNS[invert] = _f(_Batch(c).run(invert=invert)[0])
    return _LADDER_RUNS[invert]


@pytest.mark.gpu
def test_hip_solve_local_ladder():
    """invert = 0: the kernel sees the rows the restatement knows.  Every joint of the launch within the bar of ONE row rounding
    (printed); per rung the error in units of the bar, in bare perturbation units, and over the fp32 SVD's error on the same rows.
    The header's claim ("closer to the fp64 SVD than an fp32 SVD") is held on the rungs up to 1e3, where a rig can be."""
    L = du.ladder(False)
    got = _ladder_run(False)
    assert np.isfinite(got).all()
    ok, table = {}, {}
    for fused in (True, False):
        refs = du.ladder_refs(fused)
        rel = np.array([[np.abs(got[b, j] - q["Xs"]).max() / q["bar"] for j, q in enumerate(r)] for b, r in enumerate(refs)])
        ok[fused] = bool((rel <= 1.0).all())
        table[fused] = rel
        print(f"rows {'fused fl(u*M2 - M0)' if fused else 'two-step fl(fl(u*M2) - M0)'}: worst error / bar = {rel.max():.3g}")
    assert ok[True] or ok[False], "the kernel lies within the bar of neither row rounding"
    fused = ok[True]
    print("the kernel's rows are " + ("FUSED" if fused else "TWO-STEP"))
    refs = du.ladder_refs(fused)
    for ri, r in enumerate(du.RUNGS):
        e_hip, e_32, units, nrm = [], [], [], []
        for b in np.where(L["rung"] == ri)[0]:
            for j, q in enumerate(refs[b]):
                err = np.abs(got[b, j] - q["Xs"]).max()
                e_hip.append(err)
                e_32.append(np.abs(q["X32"] - q["Xs"]).max())
                units.append(err / q["unit"])
                nrm.append(du.U * np.abs(q["Xs"]).max())
        e_hip, e_32, nrm = np.array(e_hip), np.array(e_32), np.array(nrm)
        print(f"rung {r:.0e}: error/bar {table[fused][L['rung'] == ri].max():.3g}  error/unit {max(units):.3g}  max err hip {e_hip.max():.3e} m, "
              f"fp32 SVD {e_32.max():.3e} m;  in fp32 roundings of |X*|: hip {np.max(e_hip / nrm):.3g}, fp32 SVD {np.max(e_32 / nrm):.3g};  "
              f"hip worse than the fp32 SVD on {int((e_hip > e_32).sum())} of {len(e_hip)} joints")
        if r <= 1e3:
            assert np.max(e_hip / nrm) <= np.max(e_32 / nrm), f"rung {r:.0e}: the kernel is further from the fp64 SVD than an fp32 SVD"
        if r <= 1e2:
            assert np.max(e_hip / nrm) <= 2.0                                      # one fp32 rounding of the fp64 answer (t2 < t1)


@pytest.mark.gpu
def test_hip_sign_rule():
    """The sign batch (tests/dlt_forms_util.py::sign_batch) against the solve's bar: on its joints with x3 < 0 before the flip the
    other sign's answer is more than a bar away (CPU test above), so the bar holds only with the rule x3 >= 0."""
    c = du.sign_batch()
    got = _f(_Batch(c).run()[0])
    ok = {}
    for fused in (True, False):
        rel = []
        for b in range(len(c["views"])):
            rows = du.rows_of(c["uv"][4 * b:4 * b + 4], c["K"][4 * b:4 * b + 4], c["T"][4 * b:4 * b + 4], fused)
            rel += [np.abs(got[b, j] - du.joint_ref(rows[j])["Xs"]).max() / du.joint_ref(rows[j])["bar"] for j in range(5)]
        ok[fused] = max(rel) <= 1.0
        print(f"sign batch, rows {'fused' if fused else 'two-step'}: worst error / bar = {max(rel):.3g}")
    assert ok[True] or ok[False]


@pytest.mark.gpu
def test_hip_end_to_end_ladder():
    """invert = 1 on generic fp32 camera->master matrices.  Reference: fp64 from the fp32 inputs throughout (inverse, M, rows, SVD,
    sign).  Yardstick: dlt_oracle in fp32 on the CPU on the same inputs, re-signed.  Bar 4 x yardstick + 2^-23 max |X*| per sample."""
    L = du.ladder(True)
    got = _ladder_run(True)
    offs = np.concatenate([[0], np.cumsum(L["views"])])
    with du.resigned_svd():
        yard = do.triangulate_reference_joints(torch.from_numpy(L["uv"]), torch.from_numpy(L["K"]), torch.from_numpy(L["mat"]),
                                               L["views"]).double().numpy()
    rows = du.rows_fp64(L["uv"], L["K"], L["T64"])
    e_hip, e_y, bar = np.zeros(40), np.zeros(40), np.zeros(40)
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        Xs = np.stack([du.solve_svd(rows[j, s:e])[0] for j in range(du.LADDER_J)])
        e_hip[b], e_y[b] = np.abs(got[b] - Xs).max(), np.abs(yard[b] - Xs).max()
        bar[b] = 4 * e_y[b] + 2.0 ** -23 * np.abs(Xs).max()
    for ri, r in enumerate(du.RUNGS):
        m = L["rung"] == ri
        print(f"rung {r:.0e}: |HIP - fp64| / |fp32 oracle - fp64| per sample {np.min(e_hip[m] / e_y[m]):.3g}..{np.max(e_hip[m] / e_y[m]):.3g}"
              f" (rung maxima {e_hip[m].max():.3e} / {e_y[m].max():.3e} m), worst error / bar {np.max(e_hip[m] / bar[m]):.3g}")
    for b in range(40):
        assert e_hip[b] <= bar[b], (b, du.RUNGS[L["rung"][b]], L["views"][b], e_hip[b], e_y[b], bar[b])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["u8", "u2", "ragged"])
def test_hip_fixture_cases_against_the_yardstick(name):
    """The three rigs of tests/golden/dlt.npz, which tests/test_dlt.py holds to a flat 5e-6 m against upstream's recorded fp32
    output (that bar stays there: it is the check against upstream's own numbers, whose sign is LAPACK's).  Here the same cases
    against the fp64 reference with the stated sign and the yardstick bar, which is tighter on every sample (asserted)."""
    z, cases = _golden()
    views, seed = cases[name]["views"], cases[name]["seed"]
    uv, K, Emat = _dlt_inputs(views, seed)
    with du.resigned_svd():
        yard = do.triangulate_reference_joints(uv, K, Emat, views).double().numpy()
    T64 = np.linalg.inv(Emat.double().numpy())
    rows = du.rows_fp64(uv.numpy(), K.numpy(), T64)
    bt = _Batch(dict(views=views, uv=uv.numpy(), K=K.numpy(), E=Emat.numpy(), T=T64.astype(np.float32)))
    got = _f(bt.run(invert=True)[0])
    offs = np.concatenate([[0], np.cumsum(views)])
    worst = 0.0
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        Xs = np.stack([du.solve_svd(rows[j, s:e])[0] for j in range(21)])
        bar = 4 * np.abs(yard[b] - Xs).max() + 2.0 ** -23 * np.abs(Xs).max()
        err = np.abs(got[b] - Xs).max()
        worst = max(worst, err / bar)
        assert bar < 5e-6 and err <= bar, (name, b, err, bar)
    print(f"{name}: worst |HIP - fp64| over 4 x yardstick + 2^-23 |X| = {worst:.3g}")


@pytest.mark.gpu
def test_hip_python_surface_gives_the_c_entry_bits():
    import poem_v2_amd as pk
    for invert in (False, True):
        L = du.ladder(invert)
        uv, K, mat = (torch.from_numpy(L[k]).to(DEV) for k in ("uv", "K", "mat"))
        py = pk.triangulation.triangulate_reference_joints(uv, K, mat, L["views"], invert=invert)
        assert np.array_equal(py.cpu().numpy().astype(np.float64), _ladder_run(invert))
    c = du.mixed_batch(3, 21, seed=3)
    bt = _Batch(c)
    for mode in ("threshold", "weighted"):
        out, cnt = pk.triangulation.triangulate_reference_joints(bt.t["uv"], bt.t["K"], bt.t["E"], c["views"], conf=bt.t["conf"], mode=mode,
                                                                 threshold=0.5, return_count=True)
        want, wcnt = bt.run(mode, 0.5, invert=True)
        _same(out.cpu().numpy().view(np.uint32), want, mode)
        assert np.array_equal(cnt.cpu().numpy(), wcnt)


@pytest.mark.gpu
@pytest.mark.parametrize("B,J", SHAPES)
def test_hip_every_sample_equals_itself_alone(B, J):
    """B * J equal to, below and above a multiple of dlt_kernel's 64 threads; J below, at and above dlt_conf_kernel's 64 threads;
    2 to 16 views mixed.  Both kernels, both modes: each sample's bits are those of the same sample launched alone."""
    bt = _Batch(du.mixed_batch(B, J, seed=100 * B + J))
    assert min(bt.views) == 2 or B == 1
    assert max(bt.views) == 16 or B == 1
    for k, (mode, invert) in enumerate(((None, False), (None, True), ("threshold", True), ("weighted", False))):
        full, cnt = bt.run(mode, 0.5, invert)
        assert np.isfinite(_f(full)).all()
        for b in range(B):
            one, c1 = bt.run(mode, 0.5, invert, sample=b)
            _same(one[0], full[b], f"{mode} sample {b}")
            if cnt is not None:
                assert np.array_equal(c1[0], cnt[b])
        if mode == "weighted":
            assert np.array_equal(cnt, np.repeat(np.asarray(bt.views, dtype=np.int32)[:, None], J, 1))
        if mode == "threshold":
            sel, _ = du.selections(bt.c["conf"], bt.views, 0.5)
            assert np.array_equal(cnt, np.array([[len(s) for s in row] for row in sel], dtype=np.int32))


@pytest.mark.gpu
def test_hip_64_views_in_one_sample():
    """The long accumulation: one sample of 64 views against the solve's bar, plain and weighted, in the launch's row rounding."""
    rng = np.random.default_rng(64)
    rig = du._Rig(rng, 64, np.array([0.06, -0.04, 0.6]), 5)
    uv, K, T, _ = rig.build(0.3, False)
    uv = (uv + rng.normal(size=uv.shape) * 0.5).astype(np.float32)
    conf = rng.uniform(0.05, 1.0, (64, 5)).astype(np.float32)
    bt = _Batch(dict(views=[64], uv=uv, conf=conf, K=K, T=T))
    plain = _f(bt.run()[0])[0]
    wgt, cnt = bt.run("weighted")
    assert (cnt == 64).all()
    wgt = _f(wgt)[0]
    ok = {}
    for fused in (True, False):
        rows = du.rows_of(uv, K, T, fused)
        rel = []
        for j in range(5):
            q, qw = du.joint_ref(rows[j]), du.joint_ref(rows[j], conf[:, j])
            assert q["sweeps"] < 12 and np.abs(q["Xj"] - q["Xs"]).max() <= 0.5 * q["bar"] and q["s"][0] / q["s"][2] < 100
            rel += [np.abs(plain[j] - q["Xs"]).max() / q["bar"], np.abs(wgt[j] - qw["Xs"]).max() / qw["bar"]]
        ok[fused] = max(rel) <= 1.0
        print(f"64 views, rows {'fused' if fused else 'two-step'}: worst error / bar = {max(rel):.3g}")
    assert ok[True] or ok[False]


@pytest.mark.gpu
def test_hip_weights_scaled_by_a_power_of_two_change_nothing():
    """G scales by 4^k and every rotation angle is a ratio of its entries: the bits of confidence 1, hence of the plain kernel."""
    c = du.mixed_batch(5, 13, seed=7)
    for invert in (False, True):
        plain = _Batch(c).run(invert=invert)[0]
        for k in (0, -10, 7):
            bt = _Batch(dict(c, conf=np.full_like(c["conf"], 2.0 ** k)))
            _same(bt.run("weighted", invert=invert)[0], plain, f"confidence 2^{k}")
        # per VIEW powers of two are not a common factor: the answer must move (the weights are read at all)
        cf = np.ones_like(c["conf"])
        cf[::2] = 0.25
        assert not np.array_equal(_Batch(dict(c, conf=cf)).run("weighted", invert=invert)[0], plain)


def _pack(c, keep):
    """The batch with only the views keep[b] (local indices) of every sample."""
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    idx = np.concatenate([offs[b] + np.asarray(k) for b, k in enumerate(keep)]).astype(int)
    return dict(views=[len(k) for k in keep], **{k: c[k][idx] for k in ("uv", "conf", "K", "T", "E")})


@pytest.mark.gpu
def test_hip_zero_weight_views_are_views_left_out():
    """Weighted mode, confidence exactly 0 on some views: the dropped views add +0.0 to G, the bits are the plain kernel's on a batch
    holding only the other views."""
    c = du.mixed_batch(4, 16, seed=21, lo=3, hi=16)
    rng = np.random.default_rng(22)
    keep = [np.sort(rng.choice(n, size=max(2, n - 1 - n // 3), replace=False)) for n in c["views"]]
    conf = np.zeros_like(c["conf"])
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    for b, k in enumerate(keep):
        conf[offs[b] + k] = 1.0
    assert any(len(k) < n for k, n in zip(keep, c["views"]))
    for invert in (False, True):
        got, cnt = _Batch(dict(c, conf=conf)).run("weighted", invert=invert)
        _same(got, _Batch(_pack(c, keep)).run(invert=invert)[0], "zero weights")
        assert np.array_equal(cnt, np.repeat(np.asarray(c["views"], dtype=np.int32)[:, None], 16, 1))     # counted, not dropped


@pytest.mark.gpu
def test_hip_threshold_mode_is_the_plain_kernel_on_the_selected_views():
    """Every (sample, joint) of a threshold launch equals the plain kernel on that joint's selected views packed as a sample of
    their own -- including joints that come after a lowered threshold and use it."""
    c = du.mixed_batch(3, 21, seed=31, lo=4, hi=9)
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    conf = (0.55 + 0.45 * c["conf"]).astype(np.float64)                             # everybody clears 0.5 ...
    conf[offs[0]:offs[1], 5] = np.linspace(0.10, 0.31, c["views"][0])              # ... but here: lowered until two do (to 0.2)
    conf[offs[0] + 1, 6:] = 0.35                                                    # in only because joint 5 lowered the threshold
    conf[offs[0] + 2, 6:] = 0.12                                                    # out all the same
    conf[offs[1], ::2] = 0.3                                                        # sample 1 stays at 0.5: out
    conf[offs[1] + 1, 1::2] = 0.5                                                   # exactly the threshold: out (conf > thr)
    # one camera clears 0.5 at the first joint of sample 2, the others hold 0.25 EXACTLY.  Five lowerings in fp64 give
    # 0.25000000000000006, which 0.25 does not exceed: a sixth follows, to 0.2.  (Lowered in fp32 steps the threshold would be
    # 0.2499999963, the five would pass, and the joints behind would start from 0.25 and not from 0.2.)
    conf[offs[2]:offs[3], 0] = 0.25
    conf[offs[2], 0] = 0.9
    conf[offs[2] + 3, 1:] = 0.22                                                    # in at the lowered 0.2 only
    conf[offs[2] + 4, 1:] = 0.1                                                     # out
    c = dict(c, conf=conf.astype(np.float32))
    sel, thrs = du.selections(c["conf"], c["views"], 0.5)
    fresh, _ = du.selections(c["conf"][:, 6:], c["views"], 0.5)
    assert thrs[0][4] == 0.5 and thrs[0][5] < 0.31 and thrs[0][20] == thrs[0][5] and thrs[1][20] == 0.5
    assert 0.2 < thrs[2][0] < 0.21 and thrs[2][20] == thrs[2][0] and all(3 in sel[2][j] and 4 not in sel[2][j] for j in range(1, 21))
    assert any(len(sel[0][j]) != len(fresh[0][j - 6]) for j in range(6, 21))        # a later joint selects other views for it
    for invert in (False, True):
        got, cnt = _Batch(c).run("threshold", 0.5, invert)
        assert np.array_equal(cnt, np.array([[len(s) for s in row] for row in sel], dtype=np.int32)) and cnt.min() >= 2
        views, uv, K, T, E = [], [], [], [], []
        for b in range(3):
            for j in range(21):
                idx = offs[b] + sel[b][j]
                views.append(len(idx))
                uv.append(c["uv"][idx, j:j + 1]), K.append(c["K"][idx]), T.append(c["T"][idx]), E.append(c["E"][idx])
        packed = dict(views=views, uv=np.concatenate(uv), K=np.concatenate(K), T=np.concatenate(T), E=np.concatenate(E))
        _same(got.reshape(63, 1, 3), _Batch(packed).run(invert=invert)[0], f"threshold, invert {invert}")
    want, wcount = restate_conf(c["uv"], c["conf"], c["K"], c["T"], c["views"], "threshold", 0.5)
    assert np.array_equal(wcount, cnt) and np.abs(_f(got) - want).max() < 5e-6      # and it is upstream's answer (that file's bar)


@pytest.mark.gpu
def test_hip_exact_inverse_is_the_given_inverse():
    c = du.mixed_batch(4, 16, seed=41)
    E = du.exact_extrinsics(np.random.default_rng(42), sum(c["views"]))
    T = np.linalg.inv(E.astype(np.float64)).astype(np.float32) + np.float32(0.0)
    # uv from these cameras: points in front of every camera are not needed for equality of bits, finite output is
    bt = _Batch(dict(c, E=E, T=T))
    for mode in (None, "threshold", "weighted"):
        a, b = bt.run(mode, 0.5, True), bt.run(mode, 0.5, False)
        _same(a[0], b[0], f"exact inverse, mode {mode}")
        assert np.isfinite(_f(a[0])).all()
        if mode:
            assert np.array_equal(a[1], b[1])


def _with(c, **edits):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    for k, (idx, val) in edits.items():
        out[k][idx] = val
    return out


@pytest.mark.gpu
def test_hip_non_finite_inputs_stay_where_they_are():
    """The NaN rule: a non-finite uv of one joint in one view makes that joint's three outputs NaN; a NaN in a view's K or matrix
    makes every joint of that sample NaN; a NaN confidence is a view not selected (threshold: ``conf > thr`` is false) or a NaN joint
    (weighted).  Every other output keeps the clean launch's bits.  The loops are bounded (module docstring), so these end."""
    c = du.mixed_batch(3, 21, seed=51, lo=3, hi=6)
    c["conf"][:] = np.float32(0.9)
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    v1 = int(offs[1]) + 1                                                          # a view of sample 1
    nan, inf = np.float32("nan"), np.float32("inf")
    runs = [(None, False), (None, True), ("threshold", False), ("weighted", True)]
    clean = {r: _Batch(c).run(r[0], 0.5, r[1]) for r in runs}

    def check(edit, nan_mask, what):
        for r in runs:
            got, cnt = _Batch(edit).run(r[0], 0.5, r[1])
            isn = np.isnan(_f(got))
            assert np.array_equal(isn, np.broadcast_to(nan_mask[..., None], isn.shape)), (what, r, isn.sum())
            _same(got[~nan_mask], clean[r][0][~nan_mask], f"{what} {r}: the other joints")
            if cnt is not None:
                assert np.array_equal(cnt, clean[r][1]), (what, r)
    joint = np.zeros((3, 21), dtype=bool)
    joint[1, 7] = True
    check(_with(c, uv=((v1, 7, 0), nan)), joint, "NaN u")
    check(_with(c, uv=((v1, 7, 1), inf)), joint, "+Inf v")
    sample = np.zeros((3, 21), dtype=bool)
    sample[1] = True
    check(_with(c, K=((v1, 1, 1), nan)), sample, "NaN in K")
    check(_with(c, T=((v1, 1, 2), nan), E=((v1, 0, 3), nan)), sample, "NaN in the camera matrix")
    # confidence
    e = _with(c, conf=((v1, 7), nan))
    got, cnt = _Batch(e).run("threshold", 0.5, False)
    want = clean[("threshold", False)][1].copy()
    want[1, 7] -= 1
    assert np.array_equal(cnt, want) and want[1, 7] >= 2
    keep = [np.arange(n) for n in c["views"]]
    keep[1] = np.array([i for i in range(c["views"][1]) if i != 1])
    without = _Batch(_pack(c, keep)).run("threshold", 0.5, False)[0]
    _same(got[1, 7], without[1, 7], "NaN confidence, threshold mode: the launch without that view")
    rest = ~joint
    _same(got[rest], clean[("threshold", False)][0][rest], "NaN confidence, threshold mode: the other joints")
    got, cnt = _Batch(e).run("weighted", 0.5, True)
    assert np.array_equal(np.isnan(_f(got)).all(-1), joint) and np.array_equal(np.isnan(_f(got)).any(-1), joint)
    _same(got[rest], clean[("weighted", True)][0][rest], "NaN confidence, weighted mode: the other joints")


@pytest.mark.gpu
def test_hip_fewer_than_two_views():
    """Through the C entry only (the Python surface refuses): a joint whose threshold pass ends with 0 or 1 selected view, and a
    one-view sample in the plain kernel, have no triangulation -- their VALUE is not asserted.  sel_count tells, every other joint
    and sample has the clean bits, the guards hold (``_Batch.run`` checks them on every launch)."""
    c = du.mixed_batch(3, 21, seed=61, lo=3, hi=5)
    c["conf"][:] = np.float32(0.9)
    offs = np.concatenate([[0], np.cumsum(c["views"])])
    for thr in (0.0, 0.5):
        clean, ccnt = _Batch(c).run("threshold", thr, False)
        conf = c["conf"].copy()
        j0, j1 = (4, 11) if thr == 0.0 else (20, 20)     # at 0.5 the lowered threshold must not reach a later joint: the last ones
        conf[offs[0]:offs[1], j0] = -1.0                 # nobody, however far the threshold falls
        conf[offs[2]:offs[3], j1] = -1.0
        conf[offs[2] + 1, j1] = 0.9                      # one camera
        got, cnt = _Batch(dict(c, conf=conf)).run("threshold", thr, False)
        want = ccnt.copy()
        want[0, j0], want[2, j1] = 0, 1
        assert np.array_equal(cnt, want)
        rest = np.ones((3, 21), dtype=bool)
        rest[0, j0] = rest[2, j1] = False
        _same(got[rest], clean[rest], f"threshold {thr}: the other joints")
    # plain kernel: sample 1 of three has ONE view
    bt = _Batch(c)
    n0, n2 = c["views"][0], c["views"][2]
    offs1 = torch.tensor([0, n0, n0 + 1, n0 + 1 + n2], dtype=torch.int32, device=DEV)
    assert n0 + 1 + n2 <= sum(c["views"])
    got = bt.run(offs=offs1, B=3)[0]
    _same(got[0], bt.run(sample=0)[0][0], "the sample in front of the one-view sample")
    tail = {k: c[k][n0 + 1:n0 + 1 + n2] for k in ("uv", "conf", "K", "T", "E")}
    _same(got[2], _Batch(dict(tail, views=[n2])).run()[0][0], "the sample behind the one-view sample")


@pytest.mark.gpu
def test_hip_refuses_a_grid_past_int32():
    """batch * njoints must fit an int (include/poem_hip.h): POEM_E_UNSUPPORTED, nothing launched, outputs untouched."""
    import poem_v2_amd as pk
    L = pk.hip.lib()
    bt = _Batch(du.mixed_batch(2, 4, seed=71))
    out, cnt = _Guarded(64), _Guarded(64)
    p = [bt.t[k].data_ptr() for k in ("uv", "conf", "K", "T")]
    st = pk.hip.stream()
    assert L.poem_triangulate_dlt(p[0], p[2], p[3], bt.offs.data_ptr(), 65536, 32768, 0, out.ptr, st) == pk.hip.POEM_E_UNSUPPORTED
    assert L.poem_triangulate_dlt(p[0], p[2], p[3], bt.offs.data_ptr(), 1 << 30, 2, 0, out.ptr, st) == pk.hip.POEM_E_UNSUPPORTED
    for mode in (1, 2):
        assert L.poem_dlt_confidence(p[0], p[1], p[2], p[3], bt.offs.data_ptr(), out.ptr, cnt.ptr, 1 << 20, 4096, 0, mode, 0.5, st) \
            == pk.hip.POEM_E_UNSUPPORTED
    assert L.poem_dlt_confidence(p[0], p[1], p[2], p[3], bt.offs.data_ptr(), out.ptr, cnt.ptr, 2, 4097, 0, 1, 0.5, st) == -1
    assert out.untouched() and cnt.untouched()
    assert L.poem_triangulate_dlt(p[0], p[2], p[3], bt.offs.data_ptr(), 2, 4, 0, out.ptr, st) == 0          # and the call still works
    assert not out.untouched()
