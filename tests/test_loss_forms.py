"""csrc/loss.hip -- ``loss_terms_kernel`` and ``loss_finalize_kernel`` at a size where every loop makes more than one trip:
B = 300 samples with 1, 2, 3, 1, ... views, 600 views.  With the vertex projection the finalize adds 2400 view-block partials
(ten trips of its 256 threads), 300 sample partials (two trips), and ``sample_of_view`` searches nine levels.  Through
``poem_loss_terms`` (ctypes; the result and the workspace between canary guards) and ``PoemLoss``.  The reference is
``test_loss_host.restate`` (fp64 numpy).  The fixture cases keep their 1e-9 in tests/test_loss.py.

The bar: gamma * term, term >= 0 a mean of non-negative elements, gamma = (D + R) e with e = 2^-53
-------------------------------------------------------------------------------------------------
D, the depth of the two reductions.  Kernel (loss.hip): a thread's own strided loop (10 trips over 2334 vertex coordinates for
loss_3d_verts, else 1), 6 butterfly levels, 3 adds over the waves, the finalize's strided loop (ceil(blocks / 256) trips: 10 for
2400 view blocks, 3 for 600, 2 for 300 samples), 6 + 3 again, the division by the count: at most 10 + 9 + 10 + 9 + 1 = 39.  The
reference (restate): ``s += x.sum()`` once per sample or view, a chain of BN = 600 at most, over numpy's pairwise sums of at most
2334 numbers (depth <= 8 + log2(2334 / 8) < 17): 617.  D = 39 + 617 = 656, the same for every term (the larger counts are used).
R, the roundings of one element, each weighted by how much larger its operands are than its result on THESE inputs (asserted on
the CPU, ``test_big_batch_keeps_the_conditions_of_the_bar``):
  heat-map joints    ((p - g) / s)^2 summed over two axes: (1 + 1) 2 + 1 + 1 = 6                                            R = 8
  3-D joints, pose, shape   (p - g), then a square or an absolute value: 1 2 + 1 = 3                                         R = 4
  3-D vertices       parametric: (p - c) - (g - c), three roundings on operands <= 2 |d| / 0.05 = 40 |d|, squared: 240       R = 256
  joints from mesh   two regressions of 778 terms (13 in-thread + 6 butterfly, two roundings each = 38, twice) on
                     sum |w v| <= 1.3 against |d| >= 0.04: 76 * 1.3 / 0.04 = 2470, squared                                   R = 8192
  2-D joints, 2-D vertices   the 4x4 inverse (Gauss-Jordan: 4 steps x 3 roundings, rigid matrix, growth <= 2: 24), R p + t (6),
                     K c (5), u = hx / hz with hz >= 0.2 of its operands: (24 + 6 + 5) 5 2 = 350 of |u| <= 600 px; the offset is
                     compared to a target in the same image, |u| / |d| <= 30 on average over a view (asserted as
                     sum |u||d| / sum d^2), squared: 350 * 30 * 2 = 21000, once for the kernel, once for restate's own inverse  R = 65536
  loss_recon, loss   weighted sums of the above: the weighted sum of their bars, plus 8 e of the result.
gamma is about 7e-14 for the plain terms and 7e-12 for the projected ones: a dropped or doubled element of 12600 is 1e-4.
The measured worst error over its bar is printed (``pytest -s``) and recorded in LABNOTES.md."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from test_loss_host import ALL_KEYS, _dicts, _poem_loss, fixture, restate

DEV = "cuda:0"
E = 2.0 ** -53
B = 300
VIEWS = [1 + (b % 3) for b in range(B)]
BN = sum(VIEWS)
H, W = 240, 320                                   # scale 400 exactly, the clamp's bound 200
D_RED = 656
R_ELEM = {"loss_heatmap_joints": 8, "loss_3d_joints": 4, "loss_3d_joints_from_mesh": 8192, "loss_3d_verts": 256,
          "loss_2d_joints": 65536, "loss_2d_verts": 65536, "loss_pose": 4, "loss_shape": 4}
_CANARY = 0x7FC0DEAD
_GUARD = 256

CONFIGS = {   # name: (vertices projected, parametric, joints l2, vertices l2, centre)
    "projected": (True, True, True, False, 9),
    "l1_joints": (False, False, False, True, 0),
    "all_l2": (False, True, True, True, 20),
}


def loss_cfg(v2d, jl2, vl2, j2d=1.0):
    return {"JOINTS_LOSS_WEIGHT": 1.0, "VERTICES_LOSS_WEIGHT": 2.0, "JOINTS_2D_LOSS_WEIGHT": j2d, "VERTICES_2D_LOSS_WEIGHT": 0.25 if v2d else 0.0,
            "HEATMAP_JOINTS_WEIGHT": 10.0, "JOINTS_LOSS_TYPE": "l2" if jl2 else "l1", "VERTICES_LOSS_TYPE": "l2" if vl2 else "l1"}


def bars(ref, lo):
    """{key: bar} for a restated result."""
    bar = {k: (D_RED + R_ELEM[k]) * E * abs(v) for k, v in ref.items() if k in R_ELEM}
    g = lambda k: bar.get(k, 0.0)                                                   # noqa: E731
    recon = lo["JOINTS_LOSS_WEIGHT"] * (g("loss_3d_joints") + g("loss_3d_joints_from_mesh")) + lo["VERTICES_LOSS_WEIGHT"] * g("loss_3d_verts") \
        + lo["JOINTS_2D_LOSS_WEIGHT"] * g("loss_2d_joints") + lo["VERTICES_2D_LOSS_WEIGHT"] * g("loss_2d_verts") \
        + 0.001 * g("loss_pose") + 0.0005 * g("loss_shape")
    bar["loss_recon"] = recon + 8 * E * abs(ref["loss_recon"])
    bar["loss"] = bar["loss_recon"] + lo["HEATMAP_JOINTS_WEIGHT"] * g("loss_heatmap_joints") + 8 * E * abs(ref["loss"])
    return bar


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _project(Em, K, pts):
    T = np.linalg.inv(Em.astype(np.float64))
    c = pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    h = c @ K.astype(np.float64).T
    return h[:, :2] / h[:, 2:]


_BIG = []


def big_batch():
    """The ragged batch of the module docstring (built once, never changed: tests copy what they edit).  Every sample has its own
    offset between prediction and ground truth (3-D: +-[0.05, 0.15] m per axis; heat-map uv: +-[5, 15] px; projected joints against
    their targets: +-[20, 60] px) and every view a camera of its own, so that a view credited to the wrong sample, or a sample
    read twice, moves a term by many bars.  The master view of sample 299 is the identity with the clamp test's K; joint 2 of that
    sample sits on the clamp's bound on both axes (test_loss.py::test_clamp_at_its_bound), joint 3 projects to hz = 0 exactly."""
    if _BIG:
        return _BIG[0]
    g = np.random.default_rng(300)
    sgn = lambda *s: g.choice([-1.0, 1.0], s)                                       # noqa: E731
    box = lambda n: np.concatenate([g.uniform(-0.3, 0.3, (B, n, 2)), g.uniform(0.55, 0.95, (B, n, 1))], -1)   # noqa: E731
    gt_j, gt_v = box(21), box(778)
    c3 = sgn(B, 1, 3) * g.uniform(0.05, 0.15, (B, 1, 3))
    coords = np.concatenate([gt_j, gt_v], 1) + c3 + g.normal(size=(B, 799, 3)) * 0.002
    Em = np.tile(np.eye(4), (BN, 1, 1))
    K = np.zeros((BN, 3, 3))
    for v in range(BN):
        Em[v, :3, :3] = _rodrigues(g.normal(size=3) * 0.06)
        Em[v, :3, 3] = g.uniform(-0.1, 0.1, 3)
        K[v] = [[g.uniform(250, 350), 0, g.uniform(150, 170)], [0, g.uniform(250, 350), g.uniform(110, 130)], [0, 0, 1]]
    offs = np.concatenate([[0], np.cumsum(VIEWS)])
    Em[offs[299]] = np.eye(4)
    K[offs[299]] = [[300, 0, 128], [0, 300, 128], [0, 0, 1]]
    Em, K = Em.astype(np.float32), K.astype(np.float32)
    gt_uv = np.zeros((BN, 21, 2))
    pred_uv = np.zeros((BN, 21, 2))
    for b in range(B):
        o2 = sgn(2) * g.uniform(20, 60, 2)
        o1 = sgn(2) * g.uniform(5, 15, 2)
        for v in range(offs[b], offs[b + 1]):
            gt_uv[v] = _project(Em[v], K[v], gt_j[b].astype(np.float32)) + o2
            pred_uv[v] = gt_uv[v] + o1 + g.normal(size=(21, 2)) * 0.5
    inp = dict(coords=coords, pred_uv=pred_uv, pred_pose=g.normal(size=(B, 16, 3)), pred_shape=g.normal(size=(B, 10)), gt_joints=gt_j,
               gt_verts=gt_v, gt_uv=gt_uv, K=K, E=Em, mano_pose=g.normal(size=(BN, 16, 3)), mano_shape=g.normal(size=(BN, 10)))
    inp = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in inp.items()}
    v0 = offs[299]
    inp["coords"][299, 2] = (0.5, 0.25, 1.0)                                        # -> (278, 203) through the identity view
    inp["gt_uv"][v0, 2] = (78.0, 403.0)                                             # offsets +200 and -200: on the bound
    inp["coords"][299, 3] = (0.125, -0.25, 0.0)                                     # hz = 0 exactly in that view
    _BIG.append(inp)
    return inp


_REFS = {}


def reference(name, inp=None, views=None, tag=None):
    """restate on the big batch in one of CONFIGS; cached (the projected configuration walks a million points in Python)."""
    key = (name, tag)
    if key not in _REFS:
        v2d, par, jl2, vl2, c = CONFIGS[name]
        _REFS[key] = restate(big_batch() if inp is None else inp, VIEWS if views is None else views, loss_cfg(v2d, jl2, vl2), par, c, H, W,
                             fixture()[1])
    return _REFS[key]


def dyadic_batch():
    """coords, ground truth, pose and shape as multiples of 2^-6 in [-2, 2], and a regressor whose rows are one-hot or hold 2^-k
    weights: every difference, square, absolute value and partial sum of the 3-D, pose and shape terms is exact in fp64 whatever
    the order, so each mean must equal Fraction(sum) / count rounded once."""
    g = np.random.default_rng(64)
    q = lambda *s: g.integers(-128, 129, s).astype(np.float32) / np.float32(64)     # noqa: E731
    big = big_batch()
    inp = dict(big, coords=q(B, 799, 3), gt_joints=q(B, 21, 3), gt_verts=q(B, 778, 3), pred_pose=q(B, 16, 3), pred_shape=q(B, 10),
               mano_pose=q(BN, 16, 3), mano_shape=q(BN, 10))
    jreg = np.zeros((16, 778), np.float32)
    for m in range(16):
        idx = g.choice(778, size=1 + m % 4, replace=False)
        jreg[m, idx] = [[1.0], [0.5, 0.5], [0.5, 0.25, 0.25], [0.25, 0.25, 0.25, 0.25]][m % 4]
    return inp, jreg


def exact_means(inp, jreg, par, jl2, vl2, c):
    """The 3-D, pose and shape terms of a dyadic batch in exact rational arithmetic -> {key: float}, each rounded once."""
    from test_loss_host import OPENPOSE, TIPS
    f = lambda a: np.rint(np.asarray(a, np.float64) * 4096).astype(np.int64)        # noqa: E731  (units of 2^-12: products of 2^-6 ...)
    crit = lambda d, l2: int((d * d).sum()) if l2 else int(np.abs(d).sum()) * 4096  # noqa: E731  (... squares in 2^-24, |d| scaled up to it)
    co, gj, gv = f(inp["coords"]), f(inp["gt_joints"]), f(inp["gt_verts"])
    Jr = np.rint(jreg.astype(np.float64) * 4).astype(np.int64)                      # weights in quarters
    offs = np.concatenate([[0], np.cumsum(VIEWS)])
    s_j = s_m = s_v = s_p = s_s = 0
    for b in range(B):
        pj, pv = co[b, :21], co[b, 21:]
        s_j += crit(pj - gj[b], jl2)
        op = lambda v: np.concatenate([Jr @ v, 4 * v[TIPS]], 0)[OPENPOSE]            # noqa: E731  (quarters of 2^-12)
        dm = op(pv) - op(gv[b])
        s_m += Fraction(int((dm * dm).sum()), 16) if jl2 else Fraction(int(np.abs(dm).sum()) * 4096, 4)
        s_v += crit((pv - gj[b, c]) - (gv[b] - gj[b, c]) if par else pv - gv[b], vl2)
        if par:
            s_p += crit(f(inp["pred_pose"][b]) - f(inp["mano_pose"][offs[b]]), True)
            s_s += crit(f(inp["pred_shape"][b]) - f(inp["mano_shape"][offs[b]]), True)
    unit = Fraction(1, 4096 * 4096)
    out = {"loss_3d_joints": s_j * unit / (B * 63), "loss_3d_joints_from_mesh": s_m * unit / (B * 63), "loss_3d_verts": s_v * unit / (B * 2334)}
    if par:
        out.update(loss_pose=s_p * unit / (B * 48), loss_shape=s_s * unit / (B * 10))
    return {k: float(v) for k, v in out.items()}                                    # Fraction -> float rounds once, to nearest


def reorder_samples(inp, order):
    """The batch with its samples (and their views) in another order -> (inp, views)."""
    offs = np.concatenate([[0], np.cumsum(VIEWS)])
    vi = np.concatenate([np.arange(offs[b], offs[b + 1]) for b in order])
    per_view = ("pred_uv", "gt_uv", "K", "E", "mano_pose", "mano_shape")
    return {k: np.ascontiguousarray(v[vi] if k in per_view else v[np.asarray(order)]) for k, v in inp.items()}, [VIEWS[b] for b in order]


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_big_batch_makes_every_loop_take_a_second_trip():
    assert B == 300 and BN == 600 and VIEWS[:4] == [1, 2, 3, 1] and B > 256 and BN * 4 > 256 * 9 and BN > 256
    assert math.ceil(math.log2(B)) == 9                                             # sample_of_view: nine halvings
    inp = big_batch()
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in inp.values())
    offs = np.concatenate([[0], np.cumsum(VIEWS)])
    assert [VIEWS[b] for b in (0, 255, 256, 299)] == [1, 1, 2, 3] and offs[257] > 256


def test_big_batch_keeps_the_conditions_of_the_bar():
    """What R_ELEM assumes about the inputs (module docstring)."""
    inp = {k: v.astype(np.float64) for k, v in big_batch().items()}
    _, jreg = fixture()
    d3 = inp["coords"][:, 21:] - inp["gt_verts"]
    keep = np.ones(B, dtype=bool)
    assert np.abs(d3).min() >= 0.04 and np.abs(inp["coords"]).max() <= 1.3 and np.abs(jreg).sum(1).max() <= 1.0 + 1e-5
    offs = np.concatenate([[0], np.cumsum(VIEWS)])
    worst, hz_min, umax = 0.0, np.inf, 0.0
    for b in range(B):
        for v in range(offs[b], offs[b + 1]):
            pts = inp["coords"][b, :21].copy()
            if b == 299:
                pts = np.delete(pts, [2, 3], 0)
            u = _project(inp["E"][v], inp["K"][v], pts)
            gu = np.delete(inp["gt_uv"][v], [2, 3], 0) if b == 299 else inp["gt_uv"][v]
            d = np.clip(u - gu, -200, 200)
            worst = max(worst, float((np.abs(u) * np.abs(d)).sum() / (d * d).sum()))
            T = np.linalg.inv(inp["E"][v])
            cz = pts @ T[2, :3] + T[2, 3]
            hz_min = min(hz_min, float((cz / (np.abs(pts) @ np.abs(T[2, :3]) + abs(T[2, 3]))).min()))
            umax = max(umax, float(np.abs(u).max()))
    print(f"sum |u||d| / sum d^2 per view <= {worst:.3g}; hz over its operands >= {hz_min:.3g}; |u| <= {umax:.4g} px")
    assert worst <= 30 and hz_min >= 0.2 and umax <= 600 and keep.all()


def test_view_ownership_moves_the_projected_joints_by_many_bars():
    """The first view of a sample credited to the sample in front of it, or the last one to the sample behind it, at samples 0, 255,
    256 and 299: loss_2d_joints moves by more than a thousand bars, so agreement with the restatement is agreement on who owns
    each of these views."""
    ref = reference("l1_joints")
    bar = bars(ref, loss_cfg(False, False, True))["loss_2d_joints"]
    moved = []
    for b in (0, 255, 256, 299):
        for first in (True, False):
            views = list(VIEWS)
            if first and b > 0:
                views[b - 1] += 1
                views[b] -= 1
            elif not first and b < B - 1:
                views[b + 1] += 1
                views[b] -= 1
            else:
                continue
            got = restate(big_batch(), views, loss_cfg(False, False, True), False, 0, H, W, fixture()[1])
            moved.append(abs(got["loss_2d_joints"] - ref["loss_2d_joints"]) / bar)
    print(f"a view credited to a neighbour moves loss_2d_joints by {min(moved):.3g}..{max(moved):.3g} bars")
    assert len(moved) == 6 and min(moved) > 1e3


def test_exact_means_are_the_restatement_on_the_dyadic_batch():
    inp, jreg = dyadic_batch()
    for par, jl2, vl2, c in ((True, True, False, 9), (False, False, True, 0)):
        want = exact_means(inp, jreg, par, jl2, vl2, c)
        got = restate(inp, VIEWS, loss_cfg(False, jl2, vl2, j2d=0.0), par, c, H, W, jreg)
        for k, v in want.items():
            assert got[k] == v, (k, got[k], v)                                      # fp64 numpy is exact here too, in its own order
        assert all(v > 0 for v in want.values())


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
class _Guarded:
    def __init__(self, nbytes):
        self.n = (nbytes + 3) // 4
        self.buf = torch.full((self.n + 2 * _GUARD,), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf[_GUARD:].data_ptr()

    def guards_ok(self):
        return bool((self.buf[:_GUARD] == _CANARY).all()) and bool((self.buf[_GUARD + self.n:] == _CANARY).all())

    def untouched(self):
        return bool((self.buf == _CANARY).all())


_RESIDENT = {}


def _device(inp, jreg):
    key = (id(inp), id(jreg))
    if key not in _RESIDENT:
        _RESIDENT.clear()                                                           # one batch resident at a time
        _RESIDENT[key] = ({k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}, torch.from_numpy(np.ascontiguousarray(jreg)).to(DEV), inp)
    return _RESIDENT[key][:2]


def launch(inp, views, lo, par, c, jreg=None, ws_bytes=None):
    """poem_loss_terms on a batch -> (return code, the ten terms as a (10,) fp64 array or None when nothing was written)."""
    import poem_v2_amd as pk
    L = pk.hip.lib()
    jreg = fixture()[1] if jreg is None else jreg
    t, J = _device(inp, jreg)
    nb, nv = len(views), int(sum(views))
    offs = torch.tensor(np.concatenate([[0], np.cumsum(views)]), dtype=torch.int32, device=DEV)
    cfg = pk.hip.PoemLossCfg(lo["JOINTS_LOSS_WEIGHT"], lo["VERTICES_LOSS_WEIGHT"], lo["JOINTS_2D_LOSS_WEIGHT"], lo["VERTICES_2D_LOSS_WEIGHT"],
                             lo["HEATMAP_JOINTS_WEIGHT"], 0.001, 0.0005, int(lo["JOINTS_LOSS_TYPE"] == "l2"), int(lo["VERTICES_LOSS_TYPE"] == "l2"),
                             int(par), c, H, W)
    need = L.poem_loss_workspace_bytes(nb, nv)
    assert need == 8 * (nv * 4 * 3 + nb * 5)
    ws, out = _Guarded(need), _Guarded(80)
    p = {k: v.data_ptr() for k, v in t.items()}
    rc = L.poem_loss_terms(p["coords"], p["pred_uv"], p["pred_pose"], p["pred_shape"], p["gt_joints"], p["gt_verts"], p["gt_uv"], p["K"], p["E"],
                           offs.data_ptr(), p["mano_pose"], p["mano_shape"], J.data_ptr(), ctypes.byref(cfg), nb, nv, out.ptr, ws.ptr,
                           need if ws_bytes is None else ws_bytes, pk.hip.stream())
    torch.cuda.synchronize()
    assert ws.guards_ok() and out.guards_ok(), "a guard element of the workspace or of the result was written"
    if out.untouched():
        assert ws.untouched()
        return rc, None
    return rc, out.buf[_GUARD:_GUARD + 20].cpu().numpy().view(np.float64).copy()


_RUNS = {}


def run(name):
    if name not in _RUNS:
        v2d, par, jl2, vl2, c = CONFIGS[name]
        rc, raw = launch(big_batch(), VIEWS, loss_cfg(v2d, jl2, vl2), par, c)
        assert rc == 0
        _RUNS[name] = raw
    return _RUNS[name]


def _hold(raw, ref, lo, what):
    """every term of a raw result against a restated one, within its bar; disabled terms exactly +0 -> worst error / bar"""
    bar, worst = bars(ref, lo), 0.0
    for k, got in zip(ALL_KEYS, raw):
        if k not in ref:
            assert got == 0.0 and not np.signbit(got), (what, k)
            continue
        r = abs(got - ref[k]) / bar[k]
        print(f"{what}.{k}: hip {got!r} restated {ref[k]!r} error / bar {r:.3g}")
        worst = max(worst, r)
    for k, got in zip(ALL_KEYS, raw):
        if k in ref:
            assert abs(got - ref[k]) <= bar[k], (what, k, got, ref[k], bar[k])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_hip_big_ragged_batch(name):
    v2d, par, jl2, vl2, c = CONFIGS[name]
    worst = _hold(run(name), reference(name), loss_cfg(v2d, jl2, vl2), name)
    print(f"{name}: worst error over its bar {worst:.3g}")


@pytest.mark.gpu
def test_hip_poem_loss_gives_the_c_entry_bits():
    c = dict(views=VIEWS, inp=big_batch(), H=H, W=W, parametric=True, center_idx=9, loss=loss_cfg(True, True, False))
    preds, gt = _dicts(c, DEV)
    _, d = _poem_loss(c, fixture()[1])(preds, gt)
    raw = run("projected")
    assert list(d) == ALL_KEYS
    for k, v in zip(ALL_KEYS, raw):
        assert float(d[k]) == v, k


@pytest.mark.gpu
def test_hip_exact_sums():
    """The dyadic batch: the 3-D, pose and shape means equal Fraction(sum) / count rounded once -- a dropped or doubled element, or
    a sample read by no thread or by two, shows exactly -- and the same bits come out with the samples in reverse order."""
    inp, jreg = dyadic_batch()
    rinp, rviews = reorder_samples(inp, list(range(B - 1, -1, -1)))
    for par, jl2, vl2, c in ((True, True, False, 9), (False, False, True, 0), (True, False, True, 20)):
        lo = loss_cfg(False, jl2, vl2, j2d=0.0)
        rc, raw = launch(inp, VIEWS, lo, par, c, jreg=jreg)
        assert rc == 0
        got = dict(zip(ALL_KEYS, raw))
        for k, v in exact_means(inp, jreg, par, jl2, vl2, c).items():
            assert got[k] == v, (k, got[k], v, (got[k] - v) / v)
        assert got["loss_2d_joints"] == 0.0 and got["loss_2d_verts"] == 0.0
        rc, rev = launch(rinp, rviews, lo, par, c, jreg=jreg)
        assert rc == 0
        for k in ("loss_3d_joints", "loss_3d_joints_from_mesh", "loss_3d_verts", "loss_pose", "loss_shape"):
            assert rev[ALL_KEYS.index(k)] == got[k], k


@pytest.mark.gpu
def test_hip_nan_reaches_its_terms_and_no_other():
    """Sample 257 is read by a thread of the finalize on its SECOND trip (257 = 1 + 256); view 599 is the last of all.  A NaN joint
    coordinate reaches the joint terms, a NaN vertex coordinate the vertex terms, a NaN target the two 2-D joint terms; every other
    term keeps the clean launch's bits."""
    name = "projected"
    v2d, par, jl2, vl2, c = CONFIGS[name]
    clean = run(name)
    cases = {"joint of sample 257": (("coords", (257, 4, 1)), {"loss_3d_joints", "loss_2d_joints"}),
             "vertex of sample 257": (("coords", (257, 21 + 100, 0)), {"loss_3d_joints_from_mesh", "loss_3d_verts", "loss_2d_verts"}),
             "target of view 599": (("gt_uv", (599, 20, 1)), {"loss_heatmap_joints", "loss_2d_joints"})}
    for what, ((key, idx), nan_terms) in cases.items():
        inp = dict(big_batch())
        inp[key] = inp[key].copy()
        inp[key][idx] = np.float32("nan")
        rc, raw = launch(inp, VIEWS, loss_cfg(v2d, jl2, vl2), par, c)
        assert rc == 0
        recon_nan = bool(nan_terms - {"loss_heatmap_joints"})
        for k, got, was in zip(ALL_KEYS, raw, clean):
            if k in nan_terms or k == "loss" or (k == "loss_recon" and recon_nan):
                assert math.isnan(got), (what, k, got)
            else:
                assert got.tobytes() == was.tobytes(), (what, k, got, was)


@pytest.mark.gpu
def test_hip_clamp_and_z_rule_at_scale():
    """Sample 299 carries a joint on the clamp's bound and a joint with hz = 0 (big_batch); both rules are compare-and-select in
    the kernel.  Moving the target just inside the bound must lower the term, so the clamped offsets do count; the whole result is
    the restatement's either way."""
    lo = loss_cfg(False, False, True)
    base = run("l1_joints")
    inp = dict(big_batch())
    inp["gt_uv"] = inp["gt_uv"].copy()
    v0 = sum(VIEWS[:299])
    assert tuple(inp["gt_uv"][v0, 2]) == (78.0, 403.0) and tuple(inp["coords"][299, 3]) == (0.125, -0.25, 0.0)
    inp["gt_uv"][v0, 2] = (78.0 + 1e-2, 403.0 - 1e-2)
    rc, raw = launch(inp, VIEWS, lo, False, 0)
    assert rc == 0 and raw[ALL_KEYS.index("loss_2d_joints")] < base[ALL_KEYS.index("loss_2d_joints")]
    _hold(raw, reference("l1_joints", inp=inp, tag="inside"), lo, "inside the bound")
    # the two joints by themselves, exactly: offsets (+200, -200) -> 0.25 + 0.25; hz = 0 -> 1e-7 -> both offsets clamped -> 0.5
    one = {k: v[299:300] if v.shape[0] == B else v[v0:v0 + 1] for k, v in big_batch().items()}
    ref = restate(one, [1], lo, False, 0, H, W, fixture()[1])
    rc, raw1 = launch(one, [1], lo, False, 0)
    assert rc == 0
    _hold(raw1, ref, lo, "sample 299, master view")


@pytest.mark.gpu
def test_hip_order_and_determinism():
    """Two runs give the same bits.  The samples in reverse order (each with its views): every term within the bar of the same
    restated values (another order of the same sums)."""
    name = "projected"
    v2d, par, jl2, vl2, c = CONFIGS[name]
    lo = loss_cfg(v2d, jl2, vl2)
    first = run(name)
    rc, again = launch(big_batch(), VIEWS, lo, par, c)
    assert rc == 0 and again.tobytes() == first.tobytes()
    rinp, rviews = reorder_samples(big_batch(), list(range(B - 1, -1, -1)))
    assert rviews[0] == VIEWS[-1] and np.array_equal(rinp["coords"][0], big_batch()["coords"][299])
    rc, rev = launch(rinp, rviews, lo, par, c)
    assert rc == 0
    worst = _hold(rev, reference(name), lo, "reversed")
    bar = bars(reference(name), lo)
    for k, a, b_ in zip(ALL_KEYS, rev, first):
        assert abs(a - b_) <= bar[k], (k, a, b_)
    print(f"reversed order: worst error over its bar {worst:.3g}")


@pytest.mark.gpu
def test_hip_refusals_leave_result_and_workspace_alone():
    lo = loss_cfg(True, True, False)
    rc, raw = launch(big_batch(), VIEWS, lo, True, 9, ws_bytes=8 * (BN * 12 + B * 5) - 1)
    assert rc == -2 and raw is None                                                 # POEM_E_WORKSPACE
    rc, raw = launch(big_batch(), VIEWS, lo, True, 21)
    assert rc == -1 and raw is None                                                 # centre outside 0..20
