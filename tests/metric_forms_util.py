"""Plain-Python side of tests/test_metric_forms.py: the fp64 / fp32 restatements of the metric and heat-map read-out operations,
the case generators and the bars.  Nothing here touches the GPU; the CPU tests of tests/test_metric_forms.py check the
restatements against oracle/metrics_oracle.py and oracle/dlt_oracle.py, re-measure every measured bar and assert that the inputs
are the ones the case tables claim.  TEST INFRASTRUCTURE -- NOT PRODUCT CODE."""
import numpy as np
import torch

import metrics_oracle as mo

EPS32 = 2.0 ** -23          # one fp32 rounding is half of this, relative

# ---------------------------------------------------------------------------------------------------------------------
# bars
# poem_pa_epe: out is one fp32 rounding of an fp64 mean (EPS32 |ref| covers it twice over) plus what the fp64 reference itself
# is unsure of.  That was measured on the CPU (test_pa_reference_noise_is_the_recorded_one): the reference run again on every rung
# of the three flatness ladders after the two cyclic permutations of the axes -- largest disagreement 3.5e-17 m -- and after
# doubling both sets and halving the result -- 1.91e-10 m; the latter is no rounding noise but the `+ 1e-8` of s1 and s2, which
# is not scale-free (1e-8 / |pred_c| of the aligned set's size).  The larger of the two, times four.  It is a length: a case
# whose coordinates are millimetres carries it in millimetres (`unit`).
PA_NOISE_MEASURED = 1.91e-10
PA_NOISE = 4 * PA_NOISE_MEASURED


def pa_tol(ref, unit=1.0):
    return EPS32 * abs(ref) + PA_NOISE * unit


# poem_mano_to_openpose: fp32 torch.matmul of the same data against the fp64 product, on the CPU, per regressor of
# mano_regressors() over the batches of mano_cases() (test_mano_bar_is_the_measured_one); the kernel gets four times that.  The
# signed regressor's rows sum ~230 weights of size ~1 with both signs, hence its larger figure.
MANO_FP32_MEASURED = {"synthetic": 9.6e-8, "signed": 6.2e-6, "onehot": 9.0e-8}
MANO_TOL = {k: 4 * v for k, v in MANO_FP32_MEASURED.items()}

# poem_heatmap_uv: upstream's own fp32 arithmetic (oracle/dlt_oracle.py) against the fp64 restatement below on every shape x map
# count x form x image size of the tables, as a fraction of the image size: 1.35e-7 at the worst (3.4e-5 px of 256;
# test_heatmap_bar_is_the_measured_one); the kernel gets twice that.
HEATMAP_FP32_MEASURED = 1.35e-7
HEATMAP_TOL = 2 * HEATMAP_FP32_MEASURED


# ---------------------------------------------------------------------------------------------------------------------
# poem_pa_epe
PA_POINTS = (3, 4, 21, 63, 64, 65, 778)
PA_BATCHES = (1, 4, 5, 9)
LADDER = (1.0, 1e-2, 1e-4, 1e-6, 1e-8, 0.0)
LADDER_SIDES = ("gt", "pred", "both")


def pa_svd(pred, gt):
    """centred, normalised sets and the SVD of align_w_scale (pa_eval.py:104-124) in fp64: (m1, m2, s1, t1, u, w, vt)"""
    g, p = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    t1, t2 = g.mean(0), p.mean(0)
    m1, m2 = g - t1, p - t2
    s1, s2 = np.linalg.norm(m1) + 1e-8, np.linalg.norm(m2) + 1e-8
    m1, m2 = m1 / s1, m2 / s2
    u, w, vt = np.linalg.svd(m2.T.dot(m1).T)           # scipy.linalg.orthogonal_procrustes(m1, m2)
    return m1, m2, s1, t1, u, w, vt


def pa_ref(pred, gt, third=1.0):
    """(aligned mean distance, raw mean distance) of one sample, fp64.  third = -1: the other sign of the third singular pair,
    U diag(1, 1, -1) V^T -- the answer LAPACK may as well give when the third singular value is exactly 0."""
    g, p = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    m1, m2, s1, t1, u, w, vt = pa_svd(p, g)
    R = (u * np.array([1.0, 1.0, third])).dot(vt)
    aligned = m2.dot(R.T) * w.sum() * s1 + t1
    return float(np.mean(np.linalg.norm(aligned - g, axis=1))), float(np.mean(np.linalg.norm(p - g, axis=1)))


def pa_sigma_ratio(pred, gt):
    w = pa_svd(pred, gt)[5]
    return float(w[2] / w[0])


def pa_min_over_rotations(pred, gt):
    """Collinear gt: M has rank 1 and U V^T is fixed only up to an orthogonal 2x2 block Q on the two null pairs; whatever LAPACK
    picks, upstream's answer is R = U diag(1, Q) V^T for some Q.  Smallest aligned mean distance over that family: Q a rotation
    or a reflection by every angle of a half-degree grid, then three times a hundredfold finer grid about the best angle.  The
    distance is smooth in the angle with a curvature below the set's size (~0.1 m / rad^2), so the last step, 9e-9 rad, leaves the
    minimum known to ~1e-17 m."""
    g = np.asarray(gt, dtype=np.float64)
    m1, m2, s1, t1, u, w, vt = pa_svd(pred, gt)

    def dist(th, mirror):
        c, s = np.cos(th), np.sin(th)
        D = np.eye(3)
        D[1:, 1:] = np.array([[c, s], [s, -c]]) if mirror else np.array([[c, -s], [s, c]])
        aligned = m2.dot(u.dot(D).dot(vt).T) * w.sum() * s1 + t1
        return float(np.mean(np.linalg.norm(aligned - g, axis=1)))

    best = np.inf
    for mirror in (False, True):
        centre, step = np.pi, 2 * np.pi / 720
        grid = centre + step * np.arange(-360, 360)
        for _ in range(4):
            vals = [dist(th, mirror) for th in grid]
            centre = grid[int(np.argmin(vals))]
            best = min(best, min(vals))
            step /= 100.0
            grid = centre + step * np.arange(-100, 101)
    return best


def pa_generic(P, seed, B=1):
    """(pred, gt) fp32 (B,P,3): a hand-sized cloud 0.6 m in front of the camera and a noisy, rotated, scaled, shifted copy"""
    rng = np.random.RandomState(seed)
    gt = 0.08 * rng.randn(B, P, 3) + np.array([0.0, 0.0, 0.6])
    q = np.stack([random_rotation(rng) for _ in range(B)])
    c = gt.mean(1, keepdims=True)
    pred = np.einsum("bpd,bed->bpe", gt - c, q) * (1.0 + 0.1 * rng.randn(B, 1, 1)) + c
    pred = pred + 0.02 * rng.randn(B, P, 3) + 0.01 * rng.randn(B, 1, 3)
    return pred.astype(np.float32), gt.astype(np.float32)


def random_rotation(rng, det=1.0):
    q, r = np.linalg.qr(rng.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) * det < 0:
        q[:, 2] = -q[:, 2]
    return q


def pa_forms(P, B, seed):
    """name -> (pred, gt, unit) fp32 (B,P,3); every sample of a batch is different"""
    rng = np.random.RandomState(seed + 1000)
    pred, gt = pa_generic(P, seed, B)
    g64 = gt.astype(np.float64)
    c = g64.mean(1, keepdims=True)
    out = {"generic": (pred, gt, 1.0), "same": (gt.copy(), gt, 1.0)}
    for name, det in (("similar", 1.0), ("mirror", -1.0)):
        q = np.stack([random_rotation(rng, det) for _ in range(B)])
        moved = np.einsum("bpd,bed->bpe", g64 - c, q) * (0.6 + rng.rand(B, 1, 1)) + c + 0.05 * rng.randn(B, 1, 3)
        out[name] = (moved.astype(np.float32), gt, 1.0)
    out["point"] = (np.broadcast_to((c + 0.03).astype(np.float32), gt.shape).copy(), gt, 1.0)
    for name, shift in (("far1000", 1000.0), ("far1e5", 1e5)):
        out[name] = ((pred.astype(np.float64) + shift).astype(np.float32), (g64 + shift).astype(np.float32), 1.0)
    out["mm"] = ((pred.astype(np.float64) * 1000.0).astype(np.float32), (g64 * 1000.0).astype(np.float32), 1000.0)
    return out


def pa_ladder(side, factor, seed=5):
    """21 points about the origin, the z extent of `side` ("gt", "pred", "both") multiplied by `factor`; the other set generic.
    No offset along z, so that fp32 keeps the small extents (and 0 stays 0)."""
    rng = np.random.RandomState(seed)
    gt = 0.08 * rng.randn(21, 3)
    pred = (gt.dot(random_rotation(rng).T) * 1.1 + 0.03 * rng.randn(21, 3)) if side != "both" else gt + 0.03 * rng.randn(21, 3)
    if side in ("gt", "both"):
        gt[:, 2] *= factor
    if side in ("pred", "both"):
        pred[:, 2] *= factor
    shift = np.array([0.02, -0.01, 0.0])
    return (pred + shift).astype(np.float32), gt.astype(np.float32)


def pa_collinear(seed=9):
    """gt on one line -- the x axis, so that it is one exactly and M has rank 1 -- and a generic pred"""
    rng = np.random.RandomState(seed)
    gt = np.zeros((21, 3))
    gt[:, 0] = 0.08 * rng.randn(21)
    pred = gt.dot(random_rotation(rng).T) + 0.03 * rng.randn(21, 3) + 0.01
    return pred.astype(np.float32), gt.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# poem_pck_accumulate
PCK_POINTS = (1, 21, 63, 64, 65, 778)
PCK_BATCHES = (1, 3, 8)
GRIDS = ((0.0, 0.05, 20), (0.01, 0.03, 7))


def pck_dist(pred, gt, contract=False):
    """(B,P) fp32 distances with upstream's order, sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded on its own.
    contract = True: what a compiler that fuses each addition with the product beside it would give,
    sqrt(fma(dz, dz, fma(dy, dy, dx*dx))) -- the fused operations through fp64, where a product of two fp32 values is exact."""
    d = np.asarray(pred, dtype=np.float32) - np.asarray(gt, dtype=np.float32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        if not contract:
            return np.sqrt((dx * dx + dy * dy) + dz * dz)
        xx = dx * dx
        xy = (dy.astype(np.float64) * dy + xx).astype(np.float32)
        return np.sqrt((dz.astype(np.float64) * dz + xy).astype(np.float32))


def pck_ref(dist, vmin, vmax, steps):
    """(counts (P,steps) int64, n (P) int64, sum (P) fp64) of (B,P) fp32 distances: float64(d) <= numpy.linspace threshold"""
    thr = np.linspace(vmin, vmax, steps)
    with np.errstate(invalid="ignore"):
        counts = (dist.astype(np.float64)[:, :, None] <= thr[None, None, :]).sum(0)
        return counts.astype(np.int64), np.full(dist.shape[1], dist.shape[0], dtype=np.int64), dist.astype(np.float64).sum(0)


def pck_sum_tol(dist):
    """fp64 summation of n terms: n 2^-53 sum|d|, doubled, per key point"""
    d = np.nan_to_num(dist.astype(np.float64), nan=0.0, posinf=0.0)
    return 2.0 * dist.shape[0] * 2.0 ** -53 * d.sum(0)


def pck_random(B, P, seed):
    rng = np.random.RandomState(seed)
    gt = (0.08 * rng.randn(B, P, 3) + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    pred = (gt + 0.012 * rng.randn(B, P, 3)).astype(np.float32)
    return pred, gt


def pck_edge(vmin, vmax, steps):
    """gt = 0, pred = (d, 0, 0) with d = float32(thr_t) and its two neighbours for every threshold, as one (3, steps, 3) batch;
    the distance is sqrt(d*d) in fp32 -- d again unless d*d leaves the normal range"""
    thr = np.linspace(vmin, vmax, steps).astype(np.float32)
    d = np.stack([np.nextafter(thr, np.float32(-1)), thr, np.nextafter(thr, np.float32(1))])
    pred = np.zeros((3, steps, 3), dtype=np.float32)
    pred[:, :, 0] = np.abs(d)
    return pred, np.zeros_like(pred)


TRIPLE_GRID = (0.0, 0.3125, 5)        # steps of 5/64: 5 * 2^-6, 5 * 2^-5 and 5 * 2^-4 are thresholds 1, 2 and 4


def pck_triples():
    """3-4-5 triples times 2^-6, 2^-5, 2^-4 in the three axis orders, about a gt whose subtraction is exact: (3, 9, 3)"""
    gt = np.tile(np.array([0.5, -0.25, 0.75], dtype=np.float32), (3, 9, 1))
    off = np.zeros((3, 9, 3), dtype=np.float32)
    for i, k in enumerate((6, 5, 4)):
        for j, t in enumerate(((3, 4, 0), (0, -3, 4), (-4, 0, 3))):
            off[:, i * 3 + j] = np.array(t, dtype=np.float32) * np.float32(2.0 ** -k)
    return gt + off, gt


def pck_contraction(seed=0, B=8, P=65, grid=(0.0, 0.05, 20)):
    """Random triples for the contraction test: (pred, gt, grid).  A uniformly random triple sits within a place of a threshold
    once in ~1e7, so each is drawn as a random direction times a random threshold of the grid, its dz re-solved in fp64 from the
    rounded dx, dy and moved by -2..2 places: the distances land within a few places of a threshold, on both sides.  gt = 0, so
    that the differences the kernel forms are the triples themselves."""
    rng = np.random.RandomState(seed)
    thr = np.linspace(*grid)
    t = thr[rng.randint(1, grid[2], size=(B, P))]
    v = rng.randn(B, P, 3)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    d = (v * t[..., None]).astype(np.float32)
    dz = np.sqrt(np.maximum(t * t - d[..., 0].astype(np.float64) ** 2 - d[..., 1].astype(np.float64) ** 2, 0.0)).astype(np.float32)
    k = rng.randint(-2, 3, size=(B, P))
    for s in (1, 2):
        dz = np.where(k >= s, np.nextafter(dz, np.float32(1)), dz)
        dz = np.where(k <= -s, np.nextafter(dz, np.float32(-1)), dz)
    d[..., 2] = dz * np.sign(v[..., 2]).astype(np.float32)
    return d, np.zeros_like(d), grid


# ---------------------------------------------------------------------------------------------------------------------
# poem_mano_to_openpose
MANO_BATCHES = (1, 2, 5)


def mano_ref(J, V):
    """fp64 regressor . vertices and the five tip vertices, in OpenPose order; not rounded to fp32"""
    J, V = np.asarray(J, dtype=np.float32), np.asarray(V, dtype=np.float32)
    joints = np.einsum("jv,bvd->bjd", J.astype(np.float64), V.astype(np.float64))
    tips = V[:, list(mo.MANO_TIP_VERTICES)].astype(np.float64)
    return np.concatenate([joints, tips], axis=1)[:, list(mo.OPENPOSE_FROM_MANO)]


def mano_regressors():
    """name -> (16,778) fp32: the synthetic MANO-like one; one with negative and exactly zero weights on every row; one whose
    rows 0, 7 and 15 are one-hot (vertices 0, 389, 777: the first lane's first, a middle and the last vertex)"""
    base = mo.synthetic_j_regressor(11)
    rng = np.random.RandomState(21)
    signed = (rng.randn(16, 778) * (rng.rand(16, 778) < 0.3)).astype(np.float32)
    assert (signed < 0).any(1).all() and (signed == 0).any(1).all()
    onehot = base.copy()
    for r, v in ONE_HOT_ROWS:
        onehot[r] = 0
        onehot[r, v] = 1.0
    return {"synthetic": base, "signed": signed, "onehot": onehot}


ONE_HOT_ROWS = ((0, 0), (7, 389), (15, 777))


def mano_cases():
    return [(name, J, mo.synthetic_mano_verts(B, 30 + B)) for name, J in mano_regressors().items() for B in MANO_BATCHES]


def mano_fp32_error(J, V):
    got = torch.matmul(torch.from_numpy(J), torch.from_numpy(V)).numpy().astype(np.float64)
    return float(np.max(np.abs(got - np.einsum("jv,bvd->bjd", J.astype(np.float64), V.astype(np.float64)))))


# ---------------------------------------------------------------------------------------------------------------------
# poem_heatmap_uv / poem_heatmap_uv_conf
HM_SHAPES = ((1, 1), (4, 4), (8, 8), (5, 13), (24, 40), (40, 24), (32, 32), (64, 64))
HM_MAPS = (1, 4, 5, 21, 105)
HM_IMAGES = ((256.0, 256.0), (640.0, 480.0))          # (img_w, img_h)


def heatmap_ref(hm, img_w, img_h):
    """fp64 restatement of dlt_oracle.heatmap_to_uv for maps (M,Hh,Wh) -> (M,2): the sums in fp64, but the weights the fp32
    quotients float32(x) / float32(Wh) and the denominator the fp32 sum + 1e-6f, as upstream forms them (csrc/dlt.hip)"""
    h = hm.detach().cpu().to(torch.float32)
    M, Hh, Wh = h.shape
    h64 = h.double()
    den = (h64.sum((1, 2)).float() + torch.tensor(1e-6, dtype=torch.float32)).double()
    wx = (torch.arange(Wh, dtype=torch.float32) / torch.tensor(float(Wh), dtype=torch.float32)).double()
    wy = (torch.arange(Hh, dtype=torch.float32) / torch.tensor(float(Hh), dtype=torch.float32)).double()
    u = (h64.sum(1) * wx).sum(1) / den * float(img_w)
    v = (h64.sum(2) * wy).sum(1) / den * float(img_h)
    return torch.stack([u, v], 1)


def heatmap_forms(maps, hh, hw, seed):
    """name -> (maps,hh,hw) fp32"""
    g = torch.Generator().manual_seed(seed)
    return {"sigmoid": torch.sigmoid(4.0 * torch.randn(maps, hh, hw, generator=g) - 3.0),
            "zero": torch.zeros(maps, hh, hw),
            "constant": torch.full((maps, hh, hw), 0.37),
            "tiny": torch.full((maps, hh, hw), 1e-7)}


def heatmap_one_hots(hh, hw):
    """((5,hh,hw) maps, [(y, x)]): the four corners and an interior pixel, values 1, 0.5, 0.25, 1 and 0.75"""
    at = [(0, 0), (0, hw - 1), (hh - 1, 0), (hh - 1, hw - 1), (hh // 2, hw // 3)]
    hm = torch.zeros(5, hh, hw)
    for m, ((y, x), v) in enumerate(zip(at, (1.0, 0.5, 0.25, 1.0, 0.75))):
        hm[m, y, x] = v
    return hm, at


def heatmap_fp32_error(hm, img_w, img_h):
    """upstream's fp32 read-out against the fp64 restatement, as a fraction of the image size"""
    import dlt_oracle as do
    got = do.heatmap_to_uv(hm[None], img_w, img_h)[0].double()
    return float(((got - heatmap_ref(hm, img_w, img_h)).abs() / torch.tensor([img_w, img_h], dtype=torch.float64)).max())
