"""Plain-Python side of tests/test_mesh_scores.py: the two yardsticks of the benchmark-protocol mesh scores, the case generators
and the bars.  Nothing here touches the GPU and nothing here is the code under test.

    (a) nn_ref32    the search of csrc/meshscore.hip restated in fp32 numpy, operation for operation: squares
                    ((dx*dx + dy*dy) + dz*dz) each rounded on its own, the minimum over the fp32 squares ignoring NaN squares
                    (numpy.fmin), one correctly rounded fp32 root of the minimum.  The kernel must match it bit for bit.
    (b) scores64    the scores in fp64 on scipy.spatial.cKDTree; its aligned side on the fp64 SVD alignment of
                    metric_forms_util.pa_svd (PAEval.align_w_scale, lib/metrics/pa_eval.py:104-124 upstream).

The CPU tests of tests/test_mesh_scores.py hold (a) to (b), re-measure every recorded figure below and assert that the inputs are
what they claim.  TEST INFRASTRUCTURE -- NOT PRODUCT CODE."""
import numpy as np
from scipy.spatial import cKDTree

import metric_forms_util as mu

EPS32 = mu.EPS32
THRESHOLDS = (0.005, 0.015)

# the chunk lengths of nn_distance_kernel (csrc/meshscore.hip NN_QUERIES, NN_TARGETS): query points per block, target points per
# pass through LDS
NN_QUERIES, NN_TARGETS = 256, 1024
NN_SHAPES = ((1, 1), (1, 300), (63, 65), (64, 64), (65, 63), (255, 257), (257, 255), (778, 778), (799, 4096), (4096, 799),
             # both sides of the query chunk and of the LDS chunk: L - 1, L, L + 1, 2 L + 1 on either side
             (256, 255), (256, 513), (513, 256), (1023, 1025), (1024, 1024), (1025, 1023), (2049, 257), (257, 2049))
NN_BATCHES = (1, 3, 5)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the fp32 search
def nn_ref32(a, b):
    """a (na,3), b (nb,3) fp32 -> (d_ab (na,), d_ba (nb,)) fp32.  The square of b - a is the square of a - b exactly (a sign), so one
    matrix serves both directions.  numpy.fmin ignores a NaN operand and gives NaN only for an all-NaN row: the NaN rule."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = a[:, None, :] - b[None, :, :]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        return np.sqrt(np.fmin.reduce(d2, axis=1)), np.sqrt(np.fmin.reduce(d2, axis=0))


def nn_ref32_batch(a, b):
    out = [nn_ref32(x, y) for x, y in zip(a, b)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def counts_ref(d, thresholds):
    """(..., n) fp32 distances -> (..., T) int64: #{float64(d) < thr}, strict; a NaN is counted under no threshold"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(d).astype(np.float64)[..., None] < np.asarray(thresholds, dtype=np.float64)).sum(-2)


def prf(count_p, count_g, n_p, n_g):
    """precision, recall, F in fp64 from integer counts -- the expression MeshFScore.feed evaluates with torch ops"""
    p, r = np.asarray(count_p, dtype=np.float64) / float(n_p), np.asarray(count_g, dtype=np.float64) / float(n_g)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(p + r > 0, 2.0 * p * r / (p + r), 0.0)
    return p, r, f


# ---------------------------------------------------------------------------------------------------------------------
# (b) fp64 on a k-d tree
def nn_ref64(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return cKDTree(b).query(a)[0], cKDTree(a).query(b)[0]


def align64(pred, gt):
    """fp64 aligned set of one sample (align_w_scale(gt, pred)) and the singular-value ratio w3 / w1"""
    m1, m2, s1, t1, u, w, vt = mu.pa_svd(pred, gt)
    return m2.dot(u.dot(vt).T) * w.sum() * s1 + t1, float(w[2] / w[0])


def scores64(pred, gt, thresholds=THRESHOLDS, aligned=False):
    """one sample -> dict(d_p, d_g, P (T,), R (T,), F (T,)) in fp64"""
    src = align64(pred, gt)[0] if aligned else np.asarray(pred, dtype=np.float64)
    d_p, d_g = nn_ref64(src, gt)
    thr = np.asarray(thresholds, dtype=np.float64)
    p, r, f = prf((d_p[:, None] < thr).sum(0), (d_g[:, None] < thr).sum(0), len(d_p), len(d_g))
    return {"d_p": d_p, "d_g": d_g, "P": p, "R": r, "F": f}


# (a) against (b) on nn_cases' (778, 778) and (799, 4096) clouds and the F-score batch: the largest gap of an fp32 distance to the
# fp64 one, absolute (metres) and relative to the distance (test_fp32_search_against_the_kdtree re-measures both).  The fp32 square
# carries three roundings of the differences and two of the sum, the root half a place more: a few EPS32 of the distance.
NN_GAP_ABS_MEASURED = 3.9e-9
NN_GAP_REL_MEASURED = 1.2e-7


# ---------------------------------------------------------------------------------------------------------------------
# cases
def nn_case(B, na, nb, seed):
    """two hand-sized clouds 0.3 m from the origin, b a noisy copy of a where the sizes allow: distances from 0.1 mm to centimetres"""
    rng = np.random.RandomState(seed)
    a = 0.05 * rng.randn(B, na, 3) + np.array([0.05, -0.1, 0.3])
    b = 0.05 * rng.randn(B, nb, 3) + np.array([0.05, -0.1, 0.3])
    n = min(na, nb)
    b[:, :n] = a[:, :n] + 0.004 * rng.randn(B, n, 3)
    return a.astype(np.float32), b.astype(np.float32)


FSCORE_SIGMA = (0.002, 0.002, 0.005, 0.005, 0.010, 0.010)      # one per sample of the F-score batch


def fscore_case(seed=11):
    """(pred, gt) fp32 (6,778,3): gt uniform in a ball of 0.1 m, 0.3 m from the origin; pred = gt + sigma * noise"""
    rng = np.random.RandomState(seed)
    B = len(FSCORE_SIGMA)
    v = rng.randn(B, 778, 3)
    v *= (0.1 * np.cbrt(rng.rand(B, 778, 1))) / np.linalg.norm(v, axis=-1, keepdims=True)
    gt = v + np.array([0.1, -0.2, 0.2])                         # |centre| = 0.3
    pred = gt + np.array(FSCORE_SIGMA)[:, None, None] * rng.randn(B, 778, 3)
    return pred.astype(np.float32), gt.astype(np.float32)


def similarity_case(B=4, P=778, seed=23):
    """pred = s R gt + t exactly in fp64, rounded to fp32: the aligned set is gt up to fp32 rounding of the inputs"""
    rng = np.random.RandomState(seed)
    gt = 0.05 * rng.randn(B, P, 3) + np.array([0.0, 0.1, 0.4])
    q = np.stack([mu.random_rotation(rng) for _ in range(B)])
    pred = np.einsum("bpd,bed->bpe", gt, q) * (0.7 + 0.6 * rng.rand(B, 1, 1)) + 0.1 * rng.randn(B, 1, 3)
    return pred.astype(np.float32), gt.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# poem_pa_align
PA_POINTS, PA_BATCHES = mu.PA_POINTS, mu.PA_BATCHES
PA_MIN_RATIO = 1e-2          # below it the rotation's third sign is not unique; those branches are pinned through poem_pa_epe


def align_cases():
    """[(P, B, pred, gt)] over PA_POINTS x PA_BATCHES, metric_forms_util's generic clouds"""
    return [(P, B) + mu.pa_generic(P, 300 + 10 * P + B, B) for P in PA_POINTS for B in PA_BATCHES]


def align_noise(pred, gt):
    """what the fp64 reference itself is unsure of, per coordinate of the aligned set, measured the way PA_NOISE_MEASURED was: the
    reference after the two cyclic permutations of the axes, and after doubling both sets and halving the result"""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    base = align64(p, g)[0]
    worst = 0.0
    for r in (1, 2):
        worst = max(worst, float(np.abs(np.roll(align64(np.roll(p, r, 1), np.roll(g, r, 1))[0], -r, 1) - base).max()))
    return max(worst, float(np.abs(align64(2 * p, 2 * g)[0] / 2 - base).max()))


# the largest align_noise over align_cases(), fscore_case() and similarity_case() (test_align_noise_is_the_recorded_one): as for
# PA_NOISE_MEASURED it is the `+ 1e-8` of s1 and s2, which is not scale-free, not rounding -- largest on the four-point sets
# (6.98e-9 m), 9e-10 m at 778 points
ALIGN_NOISE_MEASURED = 7.0e-9
ALIGN_NOISE = 4 * ALIGN_NOISE_MEASURED


def align_tol(ref):
    """per coordinate: one fp32 rounding of the fp64 point (EPS32 |ref| covers it twice over) plus the reference's own noise"""
    return EPS32 * np.abs(ref) + ALIGN_NOISE


# the aligned counts of MeshFScore are bracketed on (b)'s distances, #{d < t - delta} <= count <= #{d < t + delta}: a coordinate
# of the kernel's aligned set is within align_tol of the fp64 one, so a point moves by at most sqrt(3) times that, and the fp32
# search adds a few EPS32 of a distance at the threshold (4 EPS32 t covers NN_GAP_REL_MEASURED twice over).
FSCORE_MAX_COORD = 0.4       # the F-score batch lies within 0.3 + 0.1 m of the origin (test_fscore_inputs_are_what_they_claim)


def fscore_delta(t, max_coord=FSCORE_MAX_COORD):
    return float(np.sqrt(3.0) * (EPS32 * max_coord + ALIGN_NOISE) + 4 * EPS32 * t)


# fscore_delta(0.015) for the F-score batch, recorded (test_fscore_delta_is_the_recorded_one)
FSCORE_DELTA_MEASURED = 1.39e-7
# and what the bracket may hide: of the 778 distances of a (sample, mode, direction, threshold) of the F-score batch, how many lie
# within delta of the threshold -- the test asserts at most FSCORE_NEAR_MAX on (b) alone
FSCORE_NEAR_MAX = 2
